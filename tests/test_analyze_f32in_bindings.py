"""The fused frame loop on float32 samples (vbx_analyze_frames_ex_f32in, vbx_f32_to_f64) at every layer above the C ABI, checked
without a GPU: the header, the Python mirror, the built library's exports, the C++ mirror, the Rust safe layer, and where the new
kernels live."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vox_box.rs_amd", "csrc")
NEW = ("vbx_f32_to_f64", "vbx_analyze_frames_ex_f32in")
TAIL = ("size_t n_frames, size_t frame_len, size_t stride, const vbx_analysis_params *h_params, const vbx_analysis_ext *h_ext, "
        "const vbx_pitch_track_params *h_track , const int64_t *h_seg_start, size_t n_segments, double *out_records, "
        "size_t record_ld, int32_t *status3, const vbx_pitch_track_outputs *h_outputs);")
NEW_UNITS = ("k_spectral_f32in.hip", "k_front_f32in.hip", "k_lists_f32in.hip", "k_burg_f32in.hip", "k_burg_lags_f32in.hip",
             "k_burg_lags_f32in_a.hip", "k_burg_lags_f32in_b.hip")


def _header():
    h = open(os.path.join(ROOT, "include", "voxbox_hip.h")).read()
    return h, " ".join(re.sub(r"/\*.*?\*/", "", h, flags=re.S).split())


def test_header_declares_the_float_input_forms():
    h, flat = _header()
    assert "int vbx_f32_to_f64(vbx_ctx *ctx, const float *x, size_t n_samples, double *out);" in flat
    assert "int vbx_analyze_frames_ex_f32in(vbx_ctx *ctx, const float *x, " + TAIL in flat
    assert re.search(r"#define VBX_ABI_VERSION 5\b", h)                      # the change only adds
    # the forms beside it are what they were
    assert "int vbx_analyze_frames_ex_f64(vbx_ctx *ctx, const double *x, " + TAIL in flat
    assert "int vbx_analyze_frames_ex_pcm16(vbx_ctx *ctx, const int16_t *pcm, " + TAIL in flat
    assert "int vbx_pcm16_to_f64(vbx_ctx *ctx, const int16_t *pcm, size_t n_samples, double *out);" in flat
    # no _f32in forms of the plain or tracked names: the one call covers them
    assert "vbx_analyze_frames_f32in" not in flat and "vbx_analyze_frames_tracked_f32in" not in flat
    # what the header promises
    assert "_f32in, not _f32" in h and "BIT FOR BIT" in h and "4-byte alignment" in h


def test_python_mirror_and_exports(pkg):
    src = open(os.path.join(ROOT, "vox_box.rs_amd", "voxbox.py")).read()
    m = re.search(r'"vbx_analyze_frames_ex_f32in": \(C\.c_int, \[(.*?)\]\)', src, re.S)
    assert m and " ".join(m.group(1).split()) == ("vp, vp, sz, sz, sz, C.POINTER(AnalysisParams), C.POINTER(AnalysisExt), "
                                                  "C.POINTER(PitchTrackParams), vp, sz, vp, sz, vp, C.POINTER(PitchTrackOutputs)")
    assert '"vbx_f32_to_f64": (C.c_int, [vp, vp, sz, vp])' in src
    assert set(NEW) <= set(pkg.exported_symbols())
    lib = pkg.load_library()
    for n in NEW:
        assert hasattr(lib, n), n
    a = lib.vbx_analyze_frames_ex_f32in.argtypes
    assert len(a) == 14 and a[1] == C.c_void_p and a[6] == C.POINTER(pkg.AnalysisExt) and a[7] == C.POINTER(pkg.PitchTrackParams)
    assert a[13] == C.POINTER(pkg.PitchTrackOutputs)
    assert list(a) == list(lib.vbx_analyze_frames_ex_f64.argtypes) == list(lib.vbx_analyze_frames_ex_pcm16.argtypes)
    assert list(lib.vbx_f32_to_f64.argtypes) == list(lib.vbx_pcm16_to_f64.argtypes)
    assert lib.vbx_abi_version() == 5
    sig = inspect.signature(pkg.VoxBox.analyze_frames_ex_f32in)
    assert list(sig.parameters) == list(inspect.signature(pkg.VoxBox.analyze_frames_ex).parameters)
    assert list(inspect.signature(pkg.VoxBox.f32_to_f64).parameters) == ["self", "x", "out"]


def test_null_context_is_refused_without_a_gpu(pkg):
    lib = pkg.load_library()
    assert lib.vbx_f32_to_f64(None, None, 0, None) == -1
    assert lib.vbx_analyze_frames_ex_f32in(None, None, 0, 1200, 480, None, None, None, None, 0, None, 36, None, None) == -1


def test_cpp_mirror_compiles_with_the_delegates():
    hdr = os.path.join(ROOT, "vox_box.rs_amd", "host")
    src = ('#include "voxbox.hpp"\n'
           'int main(){ voxbox::Context c(0); voxbox::AnalysisParams p = voxbox::analysis_params(48000.0);\n'
           '  voxbox::AnalysisExt e = voxbox::analysis_ext(0.25, true);\n'
           '  voxbox::PitchTrackParams t = voxbox::pitch_track_params(4);\n'
           '  voxbox::PitchTrackOutputs o{};\n'
           '  const float *x = nullptr;\n'
           '  voxbox::f32_to_f64(c, x, 0, nullptr);\n'
           '  voxbox::analyze_frames_ex_f32in(c, x, 0, 1200, 480, p, nullptr, nullptr, voxbox::Segments{}, nullptr, 36);\n'
           '  voxbox::analyze_frames_ex_f32in(c, x, 0, 1200, 480, p, &e, &t, voxbox::Segments{}, nullptr, 38, nullptr, &o);\n'
           '  return 0; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", hdr, "-x", "c++", "-"],
                       input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(hdr, "voxbox.hpp")).read()
    for n in NEW:
        assert n + "(" in text, n


def test_rust_layer_calls_the_float_abi():
    gpu = open(os.path.join(ROOT, "bindings", "rust", "src", "gpu.rs")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    lib = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for n in NEW:
        assert "ffi::" + n + "(" in gpu, n
        assert "pub fn " + n + "(" in ffi, n
    assert "pub struct F32Batch" in gpu and "F32Batch" in lib
    assert len(re.findall(r"pub fn analyze_ex_f32in\(&self", gpu)) == 1
    assert len(re.findall(r"pub fn analyze_ex\(&self", gpu)) == 2            # FrameBatch and PcmBatch: no third one
    body = gpu[gpu.index("pub struct F32Batch"):]
    body = body[:body.index("// ------")]
    assert "DeviceBuf<'g, f32>" in body and "ffi::vbx_f32_to_f64(" in body and "ffi::vbx_analyze_frames_ex_f32in(" in body
    m = re.search(r"pub fn vbx_analyze_frames_ex_f32in\((.*?)\) -> c_int;", ffi, re.S)
    assert "x: *const f32" in m.group(1) and "h_ext: *const VbxAnalysisExt" in m.group(1)
    assert "h_track: *const VbxPitchTrackParams" in m.group(1) and "out_records: *mut f64" in m.group(1)
    assert "pub fn vbx_f32_to_f64(ctx: *mut VbxCtx, x: *const f32, n_samples: usize, out: *mut f64) -> c_int;" in ffi


def test_new_kernels_live_in_new_translation_units():
    """The float instantiations are additions in translation units of their own (the Makefile's wildcard picks them up); the units
    of the f64 / PCM kernels instantiate no float-input form, so their kernels are compiled from what they were."""
    for u in NEW_UNITS:
        assert os.path.getsize(os.path.join(CSRC, u)) > 0, u
    assert "$(wildcard csrc/*.hip)" in open(os.path.join(ROOT, "vox_box.rs_amd", "Makefile")).read()
    read = lambda f: open(os.path.join(CSRC, f)).read()
    assert "SP_ANALYZE, 3, float>" in read("k_spectral_f32in.hip") and "float>" not in read("k_spectral.hip")
    hdr = read("vbx_spectral_1200.hpp")
    assert "typename TIN = double>" in hdr and "if constexpr (F32)" in hdr       # a compile-time choice, not a runtime flag
    assert "f32_to_f64_kernel" in read("k_front_f32in.hip") and "frame_peak_f32in_kernel" in read("k_front_f32in.hip")
    assert "frame_rms_f32in_kernel" in read("k_front_f32in.hip")
    lists = read("k_lists_f32in.hip")
    assert "pitch_frame_mfma<ALIAS, float>" in lists and "lpc_exact_list_kernel<float>" in lists and "lpc_ref_kernel<false, 12, true>" in lists
    burg = read("k_burg_f32in.hip")
    assert "launch_burg_t<double, float>" in burg and "launch_burg_list_t<float>" in burg
    assert "launch_burg_resampled_t<float>" in burg and "launch_burg_resampled_list_t<float>" in burg
    inst = read("k_burg_lags_f32in_a.hip") + read("k_burg_lags_f32in_b.hip")
    for p in (8, 10, 12, 13, 14, 16):                                            # every instantiated order of the one-pass lag kernels
        assert f"launch_burg_lags_p<{p}, float>" in inst and f"launch_burg_lags_resampled_p<{p}, float>" in inst
    for old in ("k_pitch.hip", "k_lpc_exact.hip", "k_lpc_ref.hip", "k_burg.hip", "k_burg_resampled.hip", "k_front.hip", "k_front_ex.hip"):
        assert "f32in" not in read(old), old
