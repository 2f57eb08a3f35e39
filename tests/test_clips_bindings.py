"""A batch of variable-length clips from one call (vbx_clips_plan, vbx_analyze_clips) at every layer above the C ABI, checked without a
GPU: the header's text, the structs' sizes and offsets through a compiled C probe, the Python mirror, the built library's exports,
the C++ mirror, the Rust layers, the plain-C example, where the kernels live and what they cost."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vbx_clips_plan", "vbx_analyze_clips")


def _header():
    h = open(os.path.join(ROOT, "include", "voxbox_hip.h")).read()
    return h, " ".join(re.sub(r"/\*.*?\*/", "", h, flags=re.S).split())


def test_header_declares_the_clip_batch():
    h, flat = _header()
    assert "typedef struct { int32_t format; int32_t reserved; size_t group_frames; } vbx_clip_format;" in flat
    assert "typedef struct { int64_t row_start; int64_t n_rows; int64_t group; int64_t plane_frame; } vbx_clip_row;" in flat
    assert ("int vbx_clips_plan(const size_t *h_len, size_t n_clips, size_t frame_len, size_t stride, size_t group_frames, "
            "vbx_clip_row *h_rows , size_t *h_total_rows, size_t *h_n_groups);") in flat
    m = re.search(r"int vbx_analyze_clips\((.*?)\);", flat)
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == ["vbx_ctx *ctx", "const void *const *h_clip", "const size_t *h_len", "size_t n_clips", "const vbx_clip_format *h_fmt",
                    "size_t frame_len", "size_t stride", "const vbx_analysis_params *h_params", "const vbx_analysis_ext *h_ext",
                    "const vbx_pitch_track_params *h_track", "double *out_records", "size_t record_ld", "int32_t *status3",
                    "const vbx_pitch_track_outputs *h_outputs"], args
    assert re.search(r"#define VBX_ABI_VERSION 5\b", h)                      # the change only adds
    assert re.search(r"#define VBX_CLIPS_MIN_GROUP_FRAMES 64\b", h) and re.search(r"#define VBX_CLIPS_PLANE_BYTES 268435456\b", h)
    # the block sits behind the multi-channel sessions and before the multi-GPU block, and says what it promises
    a, b, c = (h.index("live sessions over several channels (ABI 5, added)"), h.index("a batch of variable-length clips (ABI 5, added)"),
               h.index("multi-GPU: frame-range sharding"))
    assert a < b < c
    block = h[b:c]
    for n in NEW + ("vbx_clip_format", "vbx_clip_row", "bit for bit", "clips_pack_<fmt>", "clips_deliver", "[plane_frame_b]", "[row_start_b]",
                    "WAIT ON THE HOST", "NOT capturable", "vbx_track_stitch_f64", "vbx_internal_last_", "DESIGN.md section 5j", "is not read",
                    "overlap or repeat", "never read", "0x7fffffff", "vbx_unpack_samples", "tests/test_gpu_clips.py"):
        assert n in block, n
    assert "vbx_internal_clips_pack" not in h                                # the test hook stays out of the public header


def test_c_layout_matches_the_ctypes_mirrors(pkg, tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "voxbox_hip.h"\n'
           'int main(void){ printf("%zu %zu %zu %zu\\n", sizeof(vbx_clip_format), offsetof(vbx_clip_format, format),\n'
           '  offsetof(vbx_clip_format, reserved), offsetof(vbx_clip_format, group_frames));\n'
           '  printf("%zu %zu %zu %zu %zu\\n", sizeof(vbx_clip_row), offsetof(vbx_clip_row, row_start), offsetof(vbx_clip_row, n_rows),\n'
           '  offsetof(vbx_clip_row, group), offsetof(vbx_clip_row, plane_frame)); return 0; }\n')
    c = tmp_path / "layout.c"
    c.write_text(src)
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], text=True, capture_output=True, check=True).stdout.split()]
    F, R = pkg.ClipFormat, pkg.ClipRow
    assert got[:4] == [C.sizeof(F), F.format.offset, F.reserved.offset, F.group_frames.offset] == [16, 0, 4, 8]
    assert got[4:] == [C.sizeof(R), R.row_start.offset, R.n_rows.offset, R.group.offset, R.plane_frame.offset] == [32, 0, 8, 16, 24]


def test_python_mirror_and_exports(pkg):
    assert set(NEW) <= set(pkg.exported_symbols())
    lib = pkg.load_library()
    for n in NEW + ("vbx_internal_clips_pack",):
        assert hasattr(lib, n), n
    assert lib.vbx_abi_version() == 5
    vp, sz = C.c_void_p, C.c_size_t
    assert [f[0] for f in pkg.ClipFormat._fields_] == ["format", "reserved", "group_frames"]
    assert [f[0] for f in pkg.ClipRow._fields_] == ["row_start", "n_rows", "group", "plane_frame"]
    assert lib.vbx_clips_plan.argtypes == [C.POINTER(sz), sz, sz, sz, sz, C.POINTER(pkg.ClipRow), C.POINTER(sz), C.POINTER(sz)]
    a = lib.vbx_analyze_clips.argtypes
    assert len(a) == 14 and a[1] == C.POINTER(vp) and a[2] == C.POINTER(sz) and a[4] == C.POINTER(pkg.ClipFormat)
    assert a[7] == C.POINTER(pkg.AnalysisParams) and a[8] == C.POINTER(pkg.AnalysisExt) and a[9] == C.POINTER(pkg.PitchTrackParams)
    assert a[13] == C.POINTER(pkg.PitchTrackOutputs)
    assert len(lib.vbx_internal_clips_pack.argtypes) == 8
    assert list(inspect.signature(pkg.clips_plan).parameters) == ["lengths", "frame_len", "stride", "group_frames"]
    assert list(inspect.signature(pkg.VoxBox.analyze_clips).parameters)[:8] == ["self", "clips", "lengths", "params", "ext", "track", "format",
                                                                               "group_frames"]
    assert pkg.CLIPS_MIN_GROUP_FRAMES == 64 and pkg.CLIPS_PLANE_BYTES == 1 << 28
    f = pkg.ClipFormat.make(pkg.SAMPLE_F32, 128)
    assert (f.format, f.reserved, f.group_frames) == (pkg.SAMPLE_F32, 0, 128)
    rows, total, groups = pkg.clips_plan([1199, 1200, 1680, 0], 1200, 480)
    assert rows.tolist() == [[0, 0, -1, 0], [0, 1, 0, 0], [1, 2, 0, 3], [3, 0, -1, 0]] and (total, groups) == (3, 1)


def test_null_arguments_are_refused_without_a_gpu(pkg):
    lib = pkg.load_library()
    assert lib.vbx_analyze_clips(None, None, None, 0, None, 1200, 480, None, None, None, None, 0, None, None) == -1
    assert b"null context" in lib.vbx_last_error(None)
    assert lib.vbx_internal_clips_pack(None, 1, None, None, 0, 480, None, None) == -1
    assert lib.vbx_clips_plan(None, 1, 1200, 480, 0, None, None, None) == -1


def test_cpp_mirror_compiles_with_the_clip_batch():
    hdr = os.path.join(ROOT, "vox_box.rs_amd", "host")
    src = ('#include "voxbox.hpp"\n'
           'int main(){ voxbox::Context c(0); voxbox::AnalysisParams p = voxbox::analysis_params(48000.0);\n'
           '  const void *clips[2] = {nullptr, nullptr}; const size_t len[2] = {1200, 4800};\n'
           '  voxbox::ClipsPlan pl = voxbox::clips_plan(len, 2, 1200, 480);\n'
           '  voxbox::analyze_clips(c, clips, len, 2, voxbox::clip_format(VBX_SAMPLE_PCM16), 1200, 480, p, nullptr, nullptr, nullptr, 36);\n'
           '  voxbox::analyze_clips(c, clips, len, 2, voxbox::clip_format(VBX_SAMPLE_F64, 64), 1200, 480, p, nullptr, nullptr, nullptr, 36, nullptr, nullptr);\n'
           '  static_assert(sizeof(voxbox::ClipRow) == 32 && sizeof(voxbox::ClipFormat) == 16, "four int64; two int32 and a size");\n'
           '  return (int)(pl.total_rows + pl.n_groups + (size_t)pl.rows[1].row_start); }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", hdr, "-x", "c++", "-"],
                       input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(hdr, "voxbox.hpp")).read()
    for n in NEW:
        assert n + "(" in text, n


def test_rust_layers_name_every_entry_point():
    gpu = open(os.path.join(ROOT, "bindings", "rust", "src", "gpu.rs")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for n in NEW:
        assert "pub fn " + n + "(" in ffi, n
        assert "ffi::" + n in gpu, n
    assert "pub struct VbxClipFormat {" in ffi and "pub struct VbxClipRow {" in ffi and "pub plane_frame: i64," in ffi
    assert "pub fn analyze_clips(&self" in gpu and "pub fn clips_plan(" in gpu
    m = re.search(r"pub fn vbx_analyze_clips\((.*?)\) -> c_int;", ffi, re.S)
    for part in ("ctx: *mut VbxCtx", "h_clip: *const *const c_void", "h_len: *const usize", "h_fmt: *const VbxClipFormat",
                 "h_outputs: *const VbxPitchTrackOutputs"):
        assert part in m.group(1), part


def test_the_c_example_compiles_and_links(pkg, tmp_path):
    """examples/clip_batch.c: plain C against the header, every entry point it uses resolves in the library"""
    lib = os.path.join(ROOT, "vox_box.rs_amd", "lib")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "clip_batch.c"),
                        "-L", lib, "-lvoxbox_hip", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib", "-lm", "-o", str(tmp_path / "clip_batch")],
                       text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(ROOT, "examples", "clip_batch.c")).read()
    assert "vbx_analyze_clips(" in src and "vbx_clips_plan(" in src and "vbx_clip_row" in src


def test_the_kernels_live_in_their_unit():
    read = lambda f: open(os.path.join(ROOT, "vox_box.rs_amd", "csrc", f)).read()
    k = read("k_clips.hip")
    assert "clips_pack_kernel" in k and "clips_deliver_kernel" in k and '#include "vbx_reader.hpp"' in k
    # the readers' own arithmetic, not a copy of it
    assert "read_one<FMT>" in k and "read_group_wide<FMT>" in k
    assert "pcm24_value" not in k and "8388607" not in k and "2147483647" not in k
    kh = read("vbx_kernels.hpp")
    assert "void launch_clips_pack(" in kh and "void launch_clips_deliver(" in kh and "struct clip_entry_t" in kh
    assert "int vbx_clips_plan(" in read("vbx_host.cpp")
    api = read("vbx_api_clips.hip")
    for name in ("clips_pack_pcm16", "clips_pack_pcm24", "clips_pack_pcm32", "clips_pack_f32", "clips_pack_f64", "clips_deliver"):
        assert '"' + name + '"' in api, name
    assert '#include "vbx_ctx.hpp"' in api and "int vbx_analyze_clips(" in api and "int vbx_internal_clips_pack(" in api
    for other in ("vbx_api.hip", "vbx_api_frames.hip", "vbx_api_host.hip", "vbx_api_session.hip", "vbx_api_path.hip", "vbx_api_f32.hip"):
        assert "clips_pack" not in read(other), other


def test_the_new_kernels_have_no_scratch_and_no_spills():
    """the committed record is what tools/resource_usage.sh prints for the unit as it stands"""
    r = subprocess.run([os.path.join(ROOT, "tools", "resource_usage.sh"), os.path.join("vox_box.rs_amd", "csrc", "k_clips.hip")],
                       cwd=ROOT, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    built = [ln for ln in r.stdout.splitlines() if "clips_pack_kernel" in ln or "clips_deliver_kernel" in ln]
    usage = open(os.path.join(ROOT, "profiles", "analyze_clips", "resource_usage.txt")).read()
    rows = [ln for ln in usage.splitlines() if "clips_pack_kernel" in ln or "clips_deliver_kernel" in ln]
    assert len(rows) == 6 and [ln.split() for ln in rows] == [ln.split() for ln in built]
    for ln in rows:
        assert re.search(r"scratch\s+0\b", ln) and re.search(r"vspill\s+0\b", ln) and re.search(r"sspill\s+0\b", ln), ln
