"""The 8-bit sample formats (VBX_SAMPLE_U8 / ULAW / ALAW, vbx_g711_table) at every layer above the C ABI, checked without a GPU: the
header's text, the Python mirror, the built library's exports, the C++ mirror, the Rust layers, the plain-C example, where the
kernels live, the profile names the API units register, and what the 8-bit instantiations cost."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vox_box.rs_amd", "csrc")
TAGS = ("u8", "ulaw", "alaw")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_defines_the_formats_and_keeps_the_abi():
    h = _read("include", "voxbox_hip.h")
    flat = " ".join(re.sub(r"/\*.*?\*/", "", h, flags=re.S).split())
    assert re.search(r"#define VBX_SAMPLE_U8 16\b", h) and re.search(r"#define VBX_SAMPLE_ULAW 17\b", h) and re.search(r"#define VBX_SAMPLE_ALAW 18\b", h)
    assert re.search(r"#define VBX_ABI_VERSION 5\b", h)                      # the change only adds
    for name, val in (("PCM16", 1), ("PCM24", 2), ("PCM32", 3), ("F32", 4), ("F64", 5)):
        assert re.search(r"#define VBX_SAMPLE_%s %d\b" % (name, val), h)      # the old values stay
    assert "int vbx_g711_table(int format, int16_t *h_out );" in flat
    block = h[h.index("host-resident recordings (ABI 5, added)"):h.index("multi-GPU: frame-range sharding")]
    for text in ("(b - 128) / 127", "0x84", "0x108", "b ^ 0x55", "~b & 0xff", "32124", "32256", "no zero code", "DESIGN.md section 5k",
                 "6 to 15 and 19 and above", "no alignment requirement", "unpack_u8 / unpack_ulaw / unpack_alaw", "vbx_g711_table"):
        assert text in block, text
    # the contract stands beside every call that takes a format
    assert block.count("equals, bit for bit, what the same call writes for PCM16 on the decoded int16 samples") >= 6
    assert block.count("what it writes for F64 on (b - 128) / 127") >= 6


def test_python_mirror(pkg):
    assert (pkg.SAMPLE_U8, pkg.SAMPLE_ULAW, pkg.SAMPLE_ALAW) == (16, 17, 18)
    assert (pkg.SAMPLE_PCM16, pkg.SAMPLE_PCM24, pkg.SAMPLE_PCM32, pkg.SAMPLE_F32, pkg.SAMPLE_F64) == (1, 2, 3, 4, 5)
    vbm = inspect.getmodule(pkg.VoxBox)
    assert {f: vbm._SAMPLE_SRC_BYTES[f] for f in (16, 17, 18)} == {16: 1, 17: 1, 18: 1}
    assert vbm._SAMPLE_SRC_BYTES[1] == 2 and vbm._SAMPLE_SRC_BYTES[2] == 3 and vbm._SAMPLE_SRC_BYTES[5] == 8
    assert vbm._SAMPLE_OUT_DTYPE[16] == np.float64 and vbm._SAMPLE_OUT_DTYPE[17] == np.int16 and vbm._SAMPLE_OUT_DTYPE[18] == np.int16
    assert np.dtype(np.uint8) not in vbm._SAMPLE_OF_DTYPE                     # never inferred from a dtype: uint8 is also packed PCM24
    assert "vbx_g711_table" in pkg.exported_symbols()
    lib = pkg.load_library()
    assert lib.vbx_g711_table.argtypes == [C.c_int32, C.POINTER(C.c_int16)] and lib.vbx_abi_version() == 5
    assert list(inspect.signature(pkg.g711_table).parameters) == ["format"]
    # what the host calls are handed: a uint8 array with the format named; an 8-bit format with any other array is refused
    codes = np.arange(24, dtype=np.uint8)
    keep, fmt, addr, ch, n = pkg.VoxBox._host_audio(codes, pkg.SAMPLE_ULAW, 1, None)
    assert (fmt, ch, n, addr) == (17, 1, 24, keep.ctypes.data)
    assert pkg.VoxBox._host_audio(codes.reshape(8, 3), pkg.SAMPLE_U8, 1, None)[3:] == (3, 8)      # [T, C]: the channels follow
    assert pkg.VoxBox._host_audio(bytes(codes), pkg.SAMPLE_ALAW, 2, None)[3:] == (2, 12)
    assert pkg.VoxBox._host_audio(codes, None, 1, None)[1] == pkg.SAMPLE_PCM24 and pkg.VoxBox._host_audio(codes, None, 1, None)[4] == 8
    for bad in (codes.astype(np.int16), codes.astype(np.float32), codes.astype(np.float64)):
        with pytest.raises(AssertionError):
            pkg.VoxBox._host_audio(bad, pkg.SAMPLE_ULAW, 1, None)
    with pytest.raises(AssertionError):
        pkg.VoxBox._host_audio(codes, pkg.SAMPLE_PCM16, 1, None)


def test_null_arguments_are_refused_without_a_gpu(pkg):
    lib = pkg.load_library()
    assert lib.vbx_g711_table(17, None) == -1 and lib.vbx_g711_table(6, None) == -1
    assert lib.vbx_unpack_samples(None, None, 0, 17, 1, 0, None) == -1 and b"null context" in lib.vbx_last_error(None)
    assert lib.vbx_internal_clips_pack(None, 17, None, None, 0, 480, None, None) == -1


def test_cpp_mirror_compiles_with_the_formats():
    hdr = os.path.join(ROOT, "vox_box.rs_amd", "host")
    src = ('#include "voxbox.hpp"\n'
           'int main(){ std::array<int16_t, 256> t = voxbox::g711_table(VBX_SAMPLE_ULAW);\n'
           '  voxbox::ClipFormat f = voxbox::clip_format(VBX_SAMPLE_ALAW, 64);\n'
           '  static_assert(VBX_SAMPLE_U8 == 16 && VBX_SAMPLE_ULAW == 17 && VBX_SAMPLE_ALAW == 18, "the header\'s values");\n'
           '  return t[0] + f.format; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", hdr, "-x", "c++", "-"],
                       input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    assert "vbx_g711_table(" in _read("vox_box.rs_amd", "host", "voxbox.hpp")


def test_rust_layers():
    ffi_path = os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")
    before = open(ffi_path).read()
    subprocess.run(["python3", os.path.join(ROOT, "tools", "gen_rust_ffi.py")], check=True, capture_output=True)
    assert open(ffi_path).read() == before, "bindings/rust/src/ffi.rs is stale: run tools/gen_rust_ffi.py"
    for line in ("pub const VBX_SAMPLE_U8: c_int = 16;", "pub const VBX_SAMPLE_ULAW: c_int = 17;", "pub const VBX_SAMPLE_ALAW: c_int = 18;",
                 "pub fn vbx_g711_table(format: c_int, h_out: *mut i16) -> c_int;"):
        assert line in before, line
    gpu = _read("bindings", "rust", "src", "gpu.rs")
    assert "pub fn g711_table(" in gpu and "ffi::vbx_g711_table(" in gpu
    assert "ffi::VBX_SAMPLE_U8 | ffi::VBX_SAMPLE_ULAW | ffi::VBX_SAMPLE_ALAW => 1" in gpu        # one byte per source sample
    assert "ffi::VBX_SAMPLE_PCM16 | ffi::VBX_SAMPLE_ULAW | ffi::VBX_SAMPLE_ALAW => 2" in gpu     # an int16 plane
    assert "_ => 4 }" not in gpu                                               # no size rule that would take an 8-bit format for 4 bytes


def test_the_c_example_compiles_and_links(pkg, tmp_path):
    """examples/telephone_clips.c: plain C against the header, every entry point it uses resolves in the library"""
    lib = os.path.join(ROOT, "vox_box.rs_amd", "lib")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "telephone_clips.c"),
                        "-L", lib, "-lvoxbox_hip", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib", "-lm", "-o", str(tmp_path / "telephone_clips")],
                       text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    src = _read("examples", "telephone_clips.c")
    assert "vbx_analyze_clips(" in src and "VBX_SAMPLE_ULAW" in src and "VBX_SAMPLE_ALAW" in src and "vbx_g711_table(" in src


def test_the_kernels_live_in_their_units():
    read = lambda f: open(os.path.join(CSRC, f)).read()
    assert os.path.exists(os.path.join(CSRC, "k_sample8.hip"))
    # every unit under csrc/ is built: the Makefile takes them by wildcard, so the new unit needs no list entry
    mk = _read("vox_box.rs_amd", "Makefile")
    assert "$(wildcard csrc/*.hip)" in mk and "$(wildcard csrc/*.hpp)" in mk
    k8 = read("k_sample8.hip")
    assert '#include "vbx_session_ingest_all.hpp"' in k8 and '#include "vbx_clips_pack.hpp"' in k8
    for f in ("UNPACK_U8", "UNPACK_ULAW", "UNPACK_ALAW"):
        assert "launch_ingest_all_as<%s>" % f in k8 and "launch_pack_as<%s>" % f in k8, f
        assert "launch_unpack_as<%s>" % f in read("k_reader.hip") and "launch_unpack_all_as<%s>" % f in read("k_reader.hip"), f
        assert "launch_ingest_as<%s>" % f in read("k_session.hip"), f
        # the two counted units keep their five instantiations
        assert f not in read("k_clips.hip") and f not in read("k_session_channels.hip"), f
    assert "__global__" not in k8                                              # no kernel of its own, no decode pass
    # the templates moved, once each, into headers both units include
    ph, ih = read("vbx_clips_pack.hpp"), read("vbx_session_ingest_all.hpp")
    assert "void clips_pack_kernel(" in ph and "void session_ingest_all_kernel(" in ih
    assert "void clips_pack_kernel(" not in read("k_clips.hip") and "void session_ingest_all_kernel(" not in read("k_session_channels.hip")
    assert '#include "vbx_clips_pack.hpp"' in read("k_clips.hip") and '#include "vbx_session_ingest_all.hpp"' in read("k_session_channels.hip")
    # one decode, shared by the kernels and the host table; no table in the kernels
    dec = read("vbx_sample8.hpp")
    assert "ulaw_value(" in dec and "alaw_value(" in dec and "u8_value(" in dec and "0x84" in dec and "0x108" in dec
    assert '#include "vbx_sample8.hpp"' in read("vbx_reader.hpp") and '#include "vbx_sample8.hpp"' in read("vbx_host.cpp")
    assert "ulaw_value(" in read("vbx_host.cpp") and "int vbx_g711_table(" in read("vbx_host.cpp")
    for f in ("k_reader.hip", "k_session.hip", "k_sample8.hip", "vbx_reader.hpp", "vbx_clips_pack.hpp", "vbx_session_ingest_all.hpp"):
        assert "0x84" not in read(f) and "__constant__" not in read(f), f
    kh = read("vbx_kernels.hpp")
    assert "UNPACK_U8 = 16, UNPACK_ULAW = 17, UNPACK_ALAW = 18" in kh
    assert "void launch_session_ingest_all8(" in kh and "void launch_clips_pack8(" in kh
    assert "UNPACK_U8 == VBX_SAMPLE_U8 && UNPACK_ULAW == VBX_SAMPLE_ULAW" in read("vbx_api_clips.hip")


def test_the_profile_names_are_registered():
    read = lambda f: open(os.path.join(CSRC, f)).read()
    for unit, stems in (("vbx_api_host.hip", ("unpack_", "unpack_all_")), ("vbx_api_session.hip", ("session_ingest_", "session_ingest_all_")),
                        ("vbx_api_clips.hip", ("clips_pack_",))):
        text = read(unit)
        for stem in stems:
            for tag in TAGS:
                assert '"' + stem + tag + '"' in text, (unit, stem + tag)


def test_the_8bit_kernels_have_no_scratch_and_no_spills():
    """the committed record is what tools/resource_usage.sh prints for the three units as they stand"""
    built = []
    for unit in ("k_reader.hip", "k_session.hip", "k_sample8.hip"):
        r = subprocess.run([os.path.join(ROOT, "tools", "resource_usage.sh"), os.path.join("vox_box.rs_amd", "csrc", unit)],
                           cwd=ROOT, text=True, capture_output=True)
        assert r.returncode == 0, r.stderr
        built += [ln for ln in r.stdout.splitlines() if re.search(r"ILi1[678]E", ln)]      # the instantiations for formats 16, 17, 18
    usage = _read("profiles", "sample8", "resource_usage.txt")
    rows = [ln for ln in usage.splitlines() if re.search(r"ILi1[678]E", ln)]
    # unpack, unpack_all tiled and element, session_ingest; session_ingest_all and clips_pack: three formats each
    assert len(rows) == 18 and [ln.split() for ln in rows] == [ln.split() for ln in built]
    for stem, count in (("unpack_kernel", 3), ("unpack_all_tiled_kernel", 3), ("unpack_all_elem_kernel", 3), ("session_ingest_kernel", 3),
                        ("session_ingest_all_kernel", 3), ("clips_pack_kernel", 3)):
        assert sum(stem + "ILi" in ln for ln in rows) == count, stem
    for ln in rows:
        assert re.search(r"scratch\s+0\b", ln) and re.search(r"vspill\s+0\b", ln) and re.search(r"sspill\s+0\b", ln), ln
