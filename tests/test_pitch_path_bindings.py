"""The pitch path (vbx_pitch_path_f64, vbx_frame_peak_f64) at every layer above the C ABI, checked without a GPU: the header,
the Python mirror, the C++ mirror and the Rust safe layer."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_path():
    h = open(os.path.join(ROOT, "include", "voxbox_hip.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\} vbx_pitch_path_params;", h).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    fields = re.findall(r"(\w+)\s*[,;]", body)
    assert fields == ["voicing_threshold", "silence_threshold", "octave_cost", "octave_jump_cost", "voiced_unvoiced_cost",
                      "ceiling_hz", "time_step", "chunk_frames"]
    flat = " ".join(re.sub(r"/\*.*?\*/", "", h, flags=re.S).split())
    assert ("int vbx_frame_peak_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride, "
            "double *out_peak);") in flat
    assert ("int vbx_pitch_path_f64(vbx_ctx *ctx, const vbx_pitch *cand, const int32_t *count, const int32_t *status, "
            "size_t n_frames, size_t kmax, const double *local_peak, const int64_t *h_seg_start, size_t n_segments, "
            "const vbx_pitch_path_params *h_params, vbx_pitch *out_path, int32_t *out_index);") in flat
    assert "int vbx_internal_last_path_chunks_redone(vbx_ctx *ctx, int64_t *h_out);" in flat
    assert re.search(r"#define VBX_ABI_VERSION 5\b", h)                      # the change only adds
    assert "src/periodic.rs:320-354" in h and "src/periodic.rs:394-395" in h


def test_python_mirror(pkg):
    src = open(os.path.join(ROOT, "vox_box.rs_amd", "voxbox.py")).read()
    assert '"vbx_frame_peak_f64": (C.c_int, [vp, vp, sz, sz, sz, vp])' in src
    assert '"vbx_pitch_path_f64": (C.c_int, [vp, vp, vp, vp, sz, sz, vp, vp, sz, C.POINTER(PitchPathParams), vp, vp])' in src
    assert '"vbx_internal_last_path_chunks_redone": (C.c_int, [vp, C.POINTER(C.c_int64)])' in src
    P = pkg.PitchPathParams
    assert [n for n, _ in P._fields_] == ["voicing_threshold", "silence_threshold", "octave_cost", "octave_jump_cost",
                                          "voiced_unvoiced_cost", "ceiling_hz", "time_step", "chunk_frames"]
    assert C.sizeof(P) == 7 * 8 + C.sizeof(C.c_size_t)
    d = P.make()                                               # Praat's "To Pitch (ac)"
    assert (d.silence_threshold, d.voicing_threshold, d.octave_cost, d.octave_jump_cost, d.voiced_unvoiced_cost,
            d.ceiling_hz, d.time_step, d.chunk_frames) == (0.03, 0.45, 0.01, 0.35, 0.14, 600.0, 0.01, 0)
    for m in ("frame_peak", "pitch_path", "pitch_track", "last_path_chunks_redone"):
        assert callable(getattr(pkg.VoxBox, m))
    assert {"vbx_frame_peak_f64", "vbx_pitch_path_f64", "vbx_internal_last_path_chunks_redone"} <= set(pkg.exported_symbols())
    lib = pkg.load_library()
    for n in ("vbx_frame_peak_f64", "vbx_pitch_path_f64", "vbx_internal_last_path_chunks_redone"):
        assert hasattr(lib, n)


def test_cpp_mirror_compiles_with_the_path():
    hdr = os.path.join(ROOT, "vox_box.rs_amd", "host")
    src = ('#include "voxbox.hpp"\n'
           'int main(){ voxbox::Context c(0); voxbox::PitchPathParams p = voxbox::pitch_path_params(0.01, 0.2, 0.5);\n'
           '  voxbox::Frames f; voxbox::PitchExtractor::frame_peak(c, f, nullptr);\n'
           '  voxbox::PitchExtractor::pitch_path(c, nullptr, nullptr, nullptr, 0, 4, nullptr, voxbox::Segments{}, p, nullptr, nullptr);\n'
           '  voxbox::PitchExtractor::pitch_track(c, f, 48000.0, 0.2, 75.0, 600.0, 15, voxbox::Segments{}, p, nullptr, nullptr);\n'
           '  return p.chunk_frames == 0 ? 0 : 1; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", hdr, "-x", "c++", "-"],
                       input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr


def test_rust_layer_calls_the_path_abi():
    gpu = open(os.path.join(ROOT, "bindings", "rust", "src", "gpu.rs")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert re.search(r"pub fn pitch_path\(&self[^{]*\{.*?ffi::vbx_pitch_path_f64\(", gpu, re.S)
    assert re.search(r"pub fn frame_peak\(&self\)", gpu) and "ffi::vbx_frame_peak_f64(" in gpu
    assert "pub struct PitchPathParams" in gpu and "pub fn from_extractor(voiced_unvoiced_cost: f64, voicing_threshold: f64)" in gpu
    assert "pub struct VbxPitchPathParams" in ffi and "pub fn vbx_pitch_path_f64(" in ffi
    assert "PitchPathParams" in open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
