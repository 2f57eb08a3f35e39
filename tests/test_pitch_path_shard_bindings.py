"""The pitch path's shard hand-off (vbx_pitch_path_segment_peaks_f64, vbx_pitch_path_shard_begin_f64 / _enter / _finish) at every
layer above the C ABI, checked without a GPU: the header, the Python mirror, the C++ mirror and the Rust safe layer."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vbx_pitch_path_segment_peaks_f64", "vbx_pitch_path_shard_begin_f64", "vbx_pitch_path_shard_enter_f64",
         "vbx_pitch_path_shard_finish_f64")


def test_header_declares_the_hand_off():
    h = open(os.path.join(ROOT, "include", "voxbox_hip.h")).read()
    flat = " ".join(re.sub(r"/\*.*?\*/", "", h, flags=re.S).split())
    assert ("int vbx_pitch_path_segment_peaks_f64(vbx_ctx *ctx, const double *local_peak, size_t n_frames, const int64_t *h_seg_start, "
            "size_t n_segments, double *out_peak);") in flat
    assert ("int vbx_pitch_path_shard_begin_f64(vbx_ctx *ctx, const vbx_pitch *cand, const int32_t *count, const int32_t *status, "
            "size_t n_frames, size_t kmax, const double *local_peak, const double *seg_peak, const int64_t *h_seg_start, "
            "size_t n_segments, const vbx_pitch_path_params *h_params, size_t first, int continues_prev, int continues_next);") in flat
    assert ("int vbx_pitch_path_shard_enter_f64(vbx_ctx *ctx, const double *d_state_in, double *d_state_out, int32_t *d_back_map, "
            "int32_t *d_changed);") in flat
    assert ("int vbx_pitch_path_shard_finish_f64(vbx_ctx *ctx, const int32_t *d_end_state, vbx_pitch *out_path, size_t path_ld, "
            "int32_t *out_index);") in flat
    assert re.search(r"#define VBX_PITCH_PATH_STATES 64\b", h)
    assert re.search(r"#define VBX_ABI_VERSION 5\b", h)                      # the change only adds
    assert "The pitch path across a shard cut (ABI 5, added)" in h
    # the plan's comment no longer says that only the formant track crosses a cut
    assert "Only the formant track is carried across a cut" not in h


def test_python_mirror(pkg):
    src = open(os.path.join(ROOT, "vox_box.rs_amd", "voxbox.py")).read()
    assert '"vbx_pitch_path_segment_peaks_f64": (C.c_int, [vp, vp, sz, vp, sz, vp])' in src
    assert ('"vbx_pitch_path_shard_begin_f64": (C.c_int, [vp, vp, vp, vp, sz, sz, vp, vp, vp, sz, C.POINTER(PitchPathParams), sz, i32, i32])'
            in src)
    assert '"vbx_pitch_path_shard_enter_f64": (C.c_int, [vp, vp, vp, vp, vp])' in src
    assert '"vbx_pitch_path_shard_finish_f64": (C.c_int, [vp, vp, vp, sz, vp])' in src
    lib = pkg.load_library()
    assert set(NAMES) <= set(pkg.exported_symbols())
    for n in NAMES:
        assert hasattr(lib, n)
    assert len(lib.vbx_pitch_path_shard_begin_f64.argtypes) == 14 and lib.vbx_pitch_path_shard_begin_f64.restype is C.c_int
    assert len(lib.vbx_pitch_path_shard_enter_f64.argtypes) == 5 and len(lib.vbx_pitch_path_shard_finish_f64.argtypes) == 5
    for m in ("pitch_path_segment_peaks", "pitch_path_shard_begin", "pitch_path_shard_enter", "pitch_path_shard_finish"):
        assert callable(getattr(pkg.VoxBox, m))
    for f in ("path_end_states", "stitch_path", "path_handoff"):
        assert callable(getattr(pkg.shard, f))
    assert pkg.shard.PATH_STATES == 64
    # a null context is refused by every entry, before anything else is looked at
    p = pkg.PitchPathParams.make()
    assert lib.vbx_pitch_path_segment_peaks_f64(None, None, 0, None, 0, None) == -1
    assert lib.vbx_pitch_path_shard_begin_f64(None, None, None, None, 0, 4, None, None, None, 0, C.byref(p), 0, 0, 0) == -1
    assert lib.vbx_pitch_path_shard_enter_f64(None, None, None, None, None) == -1
    assert lib.vbx_pitch_path_shard_finish_f64(None, None, None, 2, None) == -1


def test_cpp_mirror_compiles_with_the_hand_off():
    hdr = os.path.join(ROOT, "vox_box.rs_amd", "host")
    src = ('#include "voxbox.hpp"\n'
           'int main(){ voxbox::Context c(0); voxbox::PitchPathParams p = voxbox::pitch_path_params(0.01);\n'
           '  voxbox::ShardPlan pl = voxbox::shard_plan(6000, 3, 1, voxbox::Segments{});\n'
           '  voxbox::PitchPathShard::segment_peaks(c, nullptr, 0, voxbox::Segments{}, nullptr);\n'
           '  voxbox::PitchPathShard::begin(c, nullptr, nullptr, nullptr, 4, nullptr, nullptr, pl, p);\n'
           '  voxbox::PitchPathShard::enter(c, nullptr, nullptr, nullptr);\n'
           '  voxbox::PitchPathShard::finish(c, nullptr, nullptr);\n'
           '  std::vector<voxbox::ShardPlan> plans(2); plans[0].plan.continues_next = 1;\n'
           '  std::vector<std::vector<int32_t>> maps(2, std::vector<int32_t>(VBX_PITCH_PATH_STATES, 3));\n'
           '  return voxbox::PitchPathShard::end_states(maps, plans)[0] == 3 ? 0 : 1; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", hdr, "-x", "c++", "-"],
                       input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr


def test_rust_layer_calls_the_hand_off_abi():
    gpu = open(os.path.join(ROOT, "bindings", "rust", "src", "gpu.rs")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for n in NAMES:
        assert f"pub fn {n}(" in ffi and f"ffi::{n}(" in gpu, n
    assert "pub const VBX_PITCH_PATH_STATES: usize = 64;" in ffi
    assert "pub struct PathShard" in gpu
    for m in (r"pub fn begin\(gpu: &'g Gpu", r"pub fn enter\(&self, state_in: Option<&\[f64\]>\)", r"pub fn finish\(self, end_state: Option<i32>\)",
              r"pub fn path_end_states\(", r"pub fn path_segment_peaks\("):
        assert re.search(m, gpu), m
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert "PathShard" in lib_rs and "path_end_states" in lib_rs
