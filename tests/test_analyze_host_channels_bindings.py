"""Every channel of a host-resident recording from one upload (vbx_unpack_channels, vbx_analyze_host_channels) at every layer above
the C ABI, checked without a GPU: the header, the Python mirror, the built library's exports, the C++ mirror and the Rust layers."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vbx_unpack_channels", "vbx_analyze_host_channels")


def _header():
    h = open(os.path.join(ROOT, "include", "voxbox_hip.h")).read()
    return h, " ".join(re.sub(r"/\*.*?\*/", "", h, flags=re.S).split())


def test_header_declares_the_channel_forms():
    h, flat = _header()
    assert ("int vbx_unpack_channels(vbx_ctx *ctx, const void *d_src, size_t n_sample_frames, int format, int channels, "
            "const int32_t *h_channels, size_t n_sel, void *d_out, size_t plane_ld);") in flat
    assert ("int vbx_analyze_host_channels(vbx_ctx *ctx, const void *h_audio, size_t n_sample_frames, const vbx_host_audio *h_fmt, "
            "const int32_t *h_channels, size_t n_sel, size_t frame_len, size_t stride, const vbx_analysis_params *h_params, "
            "const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track, const int64_t *h_seg_start, size_t n_segments, "
            "const vbx_channel_outputs *h_out , size_t record_ld);") in flat
    assert "typedef struct { double *records; int32_t *status3; const vbx_pitch_track_outputs *outputs; } vbx_channel_outputs;" in flat
    assert re.search(r"#define VBX_HOST_MAX_CHANNELS 64\b", h)
    assert re.search(r"#define VBX_ABI_VERSION 5\b", h)                      # the change only adds
    # the single-channel forms are what they were
    assert "int vbx_unpack_samples(vbx_ctx *ctx, const void *d_src, size_t n_sample_frames, int format, int channels, int channel, void *d_out);" in flat
    assert "typedef struct { int32_t format; int32_t channels; int32_t channel; int32_t reserved; size_t chunk_frames; } vbx_host_audio;" in flat
    # what the header promises, in the block of the host-resident recordings
    block = h[h.index("host-resident recordings (ABI 5, added)"):h.index("multi-GPU: frame-range sharding")]
    for n in NEW + ("vbx_channel_outputs", "VBX_HOST_MAX_CHANNELS", "unpack_all_pcm16", "n_sel * F * (16 kmax + 16)"):
        assert n in block, n


def test_python_mirror_and_exports(pkg):
    assert set(NEW) <= set(pkg.exported_symbols())
    lib = pkg.load_library()
    for n in NEW:
        assert hasattr(lib, n), n
    assert lib.vbx_abi_version() == 5
    assert C.sizeof(pkg.ChannelOutputs) == 24
    assert [f[0] for f in pkg.ChannelOutputs._fields_] == ["records", "status3", "outputs"]
    assert pkg.HOST_MAX_CHANNELS == 64
    a = lib.vbx_unpack_channels.argtypes
    assert len(a) == 9 and a[5] == C.c_void_p and a[6] == C.c_size_t and a[8] == C.c_size_t
    a = lib.vbx_analyze_host_channels.argtypes
    assert len(a) == 15 and a[3] == C.POINTER(pkg.HostAudio) and a[13] == C.POINTER(pkg.ChannelOutputs) and a[14] == C.c_size_t
    assert list(inspect.signature(pkg.VoxBox.unpack_channels).parameters) == ["self", "src", "n_sample_frames", "format", "channels", "select",
                                                                              "out", "plane_ld"]
    host = list(inspect.signature(pkg.VoxBox.analyze_host).parameters)
    both = list(inspect.signature(pkg.VoxBox.analyze_host_channels).parameters)
    assert both == [("select" if p == "channel" else p) for p in host]          # what analyze_host takes, a selection for the channel


def test_null_context_is_refused_without_a_gpu(pkg):
    lib = pkg.load_library()
    assert lib.vbx_unpack_channels(None, None, 0, 1, 1, None, 1, None, 0) == -1
    assert lib.vbx_analyze_host_channels(None, None, 0, None, None, 1, 1200, 480, None, None, None, None, 0, None, 36) == -1


def test_cpp_mirror_compiles_with_the_delegates():
    hdr = os.path.join(ROOT, "vox_box.rs_amd", "host")
    src = ('#include "voxbox.hpp"\n'
           'int main(){ voxbox::Context c(0); voxbox::AnalysisParams p = voxbox::analysis_params(48000.0);\n'
           '  voxbox::HostAudio a = voxbox::host_audio(VBX_SAMPLE_PCM16, 2);\n'
           '  const int32_t sel[2] = {1, 0};\n'
           '  voxbox::ChannelOutputs o[2] = {};\n'
           '  static_assert(sizeof(voxbox::ChannelOutputs) == 24, "three pointers");\n'
           '  static_assert(VBX_HOST_MAX_CHANNELS == 64, "the cap");\n'
           '  voxbox::unpack_channels(c, nullptr, 0, VBX_SAMPLE_PCM16, 2, sel, 2, nullptr, 0);\n'
           '  voxbox::analyze_host_channels(c, nullptr, 0, a, sel, 2, 1200, 480, p, nullptr, nullptr, voxbox::Segments{}, o, 36);\n'
           '  return 0; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", hdr, "-x", "c++", "-"],
                       input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(hdr, "voxbox.hpp")).read()
    for n in NEW:
        assert n + "(" in text, n


def test_rust_layers_name_both_entry_points():
    gpu = open(os.path.join(ROOT, "bindings", "rust", "src", "gpu.rs")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for n in NEW:
        assert "ffi::" + n + "(" in gpu, n
        assert "pub fn " + n + "(" in ffi, n
    assert "pub fn unpack_channels<" in gpu and "pub fn analyze_host_channels(&self" in gpu
    assert "pub struct VbxChannelOutputs" in ffi and "pub const VBX_HOST_MAX_CHANNELS: usize = 64;" in ffi
    m = re.search(r"pub fn vbx_analyze_host_channels\((.*?)\) -> c_int;", ffi, re.S)
    assert "h_channels: *const i32" in m.group(1) and "h_out: *const VbxChannelOutputs" in m.group(1) and "record_ld: usize" in m.group(1)
    m = re.search(r"pub fn vbx_unpack_channels\((.*?)\) -> c_int;", ffi, re.S)
    assert "h_channels: *const i32" in m.group(1) and "plane_ld: usize" in m.group(1)


def test_the_kernel_lives_beside_the_reader():
    read = lambda f: open(os.path.join(ROOT, "vox_box.rs_amd", "csrc", f)).read()
    reader = read("k_reader.hip")
    assert "unpack_all_tiled_kernel" in reader and "unpack_all_elem_kernel" in reader and "__shared__" in reader
    assert "void launch_unpack_all(" in read("vbx_kernels.hpp")
    api = read("vbx_api_host.hip")
    for name in ("unpack_all_pcm16", "unpack_all_pcm24", "unpack_all_pcm32", "unpack_all_f32", "unpack_all_f64"):
        assert '"' + name + '"' in api, name
