"""The tracked frame loop (vbx_analyze_frames_tracked_f64 / _pcm16) at every layer above the C ABI, checked without a GPU: the
header, the Python mirror, the built library's exports, the C++ mirror and the Rust safe layer."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    h = open(os.path.join(ROOT, "include", "voxbox_hip.h")).read()
    return h, " ".join(re.sub(r"/\*.*?\*/", "", h, flags=re.S).split())


def _fields(h, name):
    body = re.search(r"typedef struct \{([^{}]*)\} " + name + ";", h).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)\s*[,;]", body)


def test_header_declares_the_tracked_frame_loop():
    h, flat = _header()
    assert _fields(h, "vbx_pitch_track_params") == ["kmax", "path"]
    assert _fields(h, "vbx_pitch_track_outputs") == ["cand", "count", "peak", "index"]
    tail = ("size_t n_frames, size_t frame_len, size_t stride, const vbx_analysis_params *h_params, "
            "const vbx_pitch_track_params *h_track, const int64_t *h_seg_start, size_t n_segments, double *out_records, "
            "size_t record_ld, int32_t *status3, const vbx_pitch_track_outputs *h_outputs);")
    assert "int vbx_analyze_frames_tracked_f64(vbx_ctx *ctx, const double *x, " + tail in flat
    assert "int vbx_analyze_frames_tracked_pcm16(vbx_ctx *ctx, const int16_t *pcm, " + tail in flat
    assert re.search(r"#define VBX_ABI_VERSION 5\b", h)                      # the change only adds
    # the plain forms are what they were
    assert ("int vbx_analyze_frames_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride, "
            "const vbx_analysis_params *h_params, const int64_t *h_seg_start, size_t n_segments, double *out_records, "
            "size_t record_ld, int32_t *status3);") in flat
    # the workspace the header promises, and the sharding note
    assert "F * (16 kmax + 16)" in h and "NOT carried across a shard cut" in h


def test_python_mirror_and_exports(pkg):
    src = open(os.path.join(ROOT, "vox_box.rs_amd", "voxbox.py")).read()
    for name in ("vbx_analyze_frames_tracked_f64", "vbx_analyze_frames_tracked_pcm16"):
        m = re.search(r'"' + name + r'": \(C\.c_int, \[(.*?)\]\)', src, re.S)
        assert m, name
        args = " ".join(m.group(1).split())
        assert args == ("vp, vp, sz, sz, sz, C.POINTER(AnalysisParams), C.POINTER(PitchTrackParams), vp, sz, vp, sz, vp, "
                        "C.POINTER(PitchTrackOutputs)")
    T, O = pkg.PitchTrackParams, pkg.PitchTrackOutputs
    assert [n for n, _ in T._fields_] == ["kmax", "path"]
    assert [n for n, _ in O._fields_] == ["cand", "count", "peak", "index"]
    assert T._fields_[1][1] is pkg.PitchPathParams
    # the C layout: size_t + the path struct (7 doubles + size_t), no padding on LP64; four pointers
    assert C.sizeof(T) == C.sizeof(C.c_size_t) + C.sizeof(pkg.PitchPathParams) == 72
    assert T.path.offset == 8 and C.sizeof(O) == 4 * C.sizeof(C.c_void_p)
    t = T.make(kmax=4)
    assert t.kmax == 4 and t.path.time_step == 0.0 and t.path.voicing_threshold == 0.45      # time_step 0: the batch's own hop
    assert T.make(kmax=15, time_step=0.005, silence_threshold=0.0).path.time_step == 0.005
    for m in ("analyze_frames_tracked", "analyze_frames_tracked_pcm16"):
        assert callable(getattr(pkg.VoxBox, m))
    names = {"vbx_analyze_frames_tracked_f64", "vbx_analyze_frames_tracked_pcm16"}
    assert names <= set(pkg.exported_symbols())
    lib = pkg.load_library()
    for n in names:
        assert hasattr(lib, n)
        assert getattr(lib, n).argtypes[6] == C.POINTER(T) and getattr(lib, n).argtypes[12] == C.POINTER(O)


def test_c_layout_matches_the_ctypes_mirrors(pkg, tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "voxbox_hip.h"\n'
           'int main(void){ printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(vbx_pitch_track_params), offsetof(vbx_pitch_track_params, path),\n'
           '  sizeof(vbx_pitch_track_outputs), offsetof(vbx_pitch_track_outputs, count), offsetof(vbx_pitch_track_outputs, peak),\n'
           '  offsetof(vbx_pitch_track_outputs, index)); return 0; }\n')
    c = tmp_path / "layout.c"
    c.write_text(src)
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)],
                       text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], text=True, capture_output=True, check=True).stdout.split()]
    T, O = pkg.PitchTrackParams, pkg.PitchTrackOutputs
    assert got == [C.sizeof(T), T.path.offset, C.sizeof(O), O.count.offset, O.peak.offset, O.index.offset]


def test_cpp_mirror_compiles_with_both_delegates():
    hdr = os.path.join(ROOT, "vox_box.rs_amd", "host")
    src = ('#include "voxbox.hpp"\n'
           'int main(){ voxbox::Context c(0); voxbox::Frames f; voxbox::AnalysisParams p{};\n'
           '  voxbox::PitchTrackParams t = voxbox::pitch_track_params(4, voxbox::pitch_path_params(0.0, 0.2, 0.5));\n'
           '  voxbox::PitchTrackParams d = voxbox::pitch_track_params();\n'
           '  voxbox::PitchTrackOutputs o{};\n'
           '  voxbox::analyze_frames_tracked(c, f, p, t, voxbox::Segments{}, nullptr, 36);\n'
           '  voxbox::analyze_frames_tracked(c, f, p, t, voxbox::Segments{}, nullptr, 36, nullptr, &o);\n'
           '  voxbox::analyze_frames_tracked_pcm16(c, nullptr, 0, 1200, 480, p, d, voxbox::Segments{}, nullptr, 36, nullptr, &o);\n'
           '  return (t.kmax == 4 && d.kmax == 15 && d.path.time_step == 0.0) ? 0 : 1; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", hdr, "-x", "c++", "-"],
                       input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr


def test_rust_layer_calls_the_tracked_abi():
    gpu = open(os.path.join(ROOT, "bindings", "rust", "src", "gpu.rs")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert "ffi::vbx_analyze_frames_tracked_f64(" in gpu and "ffi::vbx_analyze_frames_tracked_pcm16(" in gpu
    assert len(re.findall(r"pub fn analyze_tracked\(&self", gpu)) == 2       # FrameBatch and PcmBatch, next to `pub fn analyze`
    assert "pub struct VbxPitchTrackParams" in ffi and "pub struct VbxPitchTrackOutputs" in ffi
    assert "pub fn vbx_analyze_frames_tracked_f64(" in ffi and "pub fn vbx_analyze_frames_tracked_pcm16(" in ffi
    m = re.search(r"pub fn vbx_analyze_frames_tracked_f64\((.*?)\) -> c_int;", ffi, re.S)
    assert "h_track: *const VbxPitchTrackParams" in m.group(1) and "h_outputs: *const VbxPitchTrackOutputs" in m.group(1)
    gen = open(os.path.join(ROOT, "tools", "gen_rust_ffi.py")).read()
    assert "VbxPitchTrackParams" in gen and "VbxPitchTrackOutputs" in gen      # the mirrors come from the generator's prelude
