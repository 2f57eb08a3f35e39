"""The formant_extraction example's frame loop (vbx_analyze_frames_ex_f64 / _pcm16, vbx_find_formants_resampled_f64) at every layer
above the C ABI, checked without a GPU: the header, the Python mirror, the built library's exports, the C++ mirror and the Rust
safe layer."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vbx_record_doubles_ex", "vbx_analyze_frames_ex_f64", "vbx_analyze_frames_ex_pcm16", "vbx_find_formants_resampled_f64")


def _header():
    h = open(os.path.join(ROOT, "include", "voxbox_hip.h")).read()
    return h, " ".join(re.sub(r"/\*.*?\*/", "", h, flags=re.S).split())


def _fields(h, name):
    body = re.search(r"typedef struct \{([^{}]*)\} " + name + ";", h).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)\s*[,;]", body)


def test_header_declares_the_example_frame_loop():
    h, flat = _header()
    assert _fields(h, "vbx_analysis_ext") == ["formant_resample_ratio", "formant_sample_rate", "rms"]
    assert re.search(r"double formant_resample_ratio;.*double formant_sample_rate;.*int32_t rms;", h, re.S)
    assert "size_t vbx_record_doubles_ex(const vbx_analysis_params *h_params, const vbx_analysis_ext *h_ext);" in flat
    tail = ("size_t n_frames, size_t frame_len, size_t stride, const vbx_analysis_params *h_params, const vbx_analysis_ext *h_ext, "
            "const vbx_pitch_track_params *h_track , const int64_t *h_seg_start, size_t n_segments, double *out_records, "
            "size_t record_ld, int32_t *status3, const vbx_pitch_track_outputs *h_outputs);")
    assert "int vbx_analyze_frames_ex_f64(vbx_ctx *ctx, const double *x, " + tail in flat
    assert "int vbx_analyze_frames_ex_pcm16(vbx_ctx *ctx, const int16_t *pcm, " + tail in flat
    assert ("int vbx_find_formants_resampled_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride, "
            "double sample_rate, double resample_ratio, size_t n_coeffs, const int64_t *h_seg_start, size_t n_segments, "
            "const vbx_resonance *h_est_init, size_t n_est, vbx_resonance *out_formants, vbx_resonance *out_res, "
            "int32_t *out_res_count, double *out_coeffs, int32_t *status);") in flat
    assert re.search(r"#define VBX_ABI_VERSION 5\b", h)                      # the change only adds
    # the forms it extends are what they were
    assert ("int vbx_analyze_frames_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride, "
            "const vbx_analysis_params *h_params, const int64_t *h_seg_start, size_t n_segments, double *out_records, "
            "size_t record_ld, int32_t *status3);") in flat
    assert ("int vbx_analyze_frames_pcm16(vbx_ctx *ctx, const int16_t *pcm, size_t n_frames, size_t frame_len, size_t stride, "
            "const vbx_analysis_params *h_params, const int64_t *h_seg_start, size_t n_segments, double *out_records, "
            "size_t record_ld, int32_t *status3);") in flat
    track_tail = ("const vbx_analysis_params *h_params, const vbx_pitch_track_params *h_track, const int64_t *h_seg_start, "
                  "size_t n_segments, double *out_records, size_t record_ld, int32_t *status3, const vbx_pitch_track_outputs *h_outputs);")
    assert "int vbx_analyze_frames_tracked_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride, " + track_tail in flat
    assert "int vbx_analyze_frames_tracked_pcm16(vbx_ctx *ctx, const int16_t *pcm, size_t n_frames, size_t frame_len, size_t stride, " + track_tail in flat
    assert ("int vbx_find_formants_f64(vbx_ctx *ctx, const double *x, size_t n_frames, size_t frame_len, size_t stride, double sample_rate, "
            "size_t n_coeffs, const int64_t *h_seg_start,") in flat
    assert "size_t vbx_record_doubles(const vbx_analysis_params *h_params);" in flat
    assert _fields(h, "vbx_pitch_track_params") == ["kmax", "path"]
    # what the header promises: the record layout, the example's literal form, the fallback's workspace bound
    assert "[ pitch | formants | mfcc | lpc | rms ]" in h and "256 MiB" in h
    assert "params.sample_rate = 10000 with formant_sample_rate = 10000" in h and "a caller who wants true Hz" in h


def test_python_mirror_and_exports(pkg):
    src = open(os.path.join(ROOT, "vox_box.rs_amd", "voxbox.py")).read()
    for name in ("vbx_analyze_frames_ex_f64", "vbx_analyze_frames_ex_pcm16"):
        m = re.search(r'"' + name + r'": \(C\.c_int, \[(.*?)\]\)', src, re.S)
        assert m, name
        assert " ".join(m.group(1).split()) == ("vp, vp, sz, sz, sz, C.POINTER(AnalysisParams), C.POINTER(AnalysisExt), "
                                               "C.POINTER(PitchTrackParams), vp, sz, vp, sz, vp, C.POINTER(PitchTrackOutputs)")
    E = pkg.AnalysisExt
    assert [(n, t) for n, t in E._fields_] == [("formant_resample_ratio", C.c_double), ("formant_sample_rate", C.c_double),
                                               ("rms", C.c_int32)]
    assert C.sizeof(E) == 24 and E.formant_sample_rate.offset == 8 and E.rms.offset == 16
    e = E.make()
    assert (e.formant_resample_ratio, e.formant_sample_rate, e.rms) == (0.0, 0.0, 0)          # asks for nothing
    e = E.make(10000.0 / 44100.0, formant_sample_rate=10000.0, rms=True)
    assert (e.formant_resample_ratio, e.formant_sample_rate, e.rms) == (10000.0 / 44100.0, 10000.0, 1)
    for m in ("analyze_frames_ex", "analyze_frames_ex_pcm16"):
        assert callable(getattr(pkg.VoxBox, m))
        assert list(inspect.signature(getattr(pkg.VoxBox, m)).parameters)[2:5] == ["params", "ext", "track"]
    p = inspect.signature(pkg.VoxBox.find_formants).parameters["resample_ratio"]
    assert p.default == 1.0
    assert set(NEW) <= set(pkg.exported_symbols())
    lib = pkg.load_library()
    for n in NEW:
        assert hasattr(lib, n), n
    for n in NEW[1:3]:
        a = getattr(lib, n).argtypes
        assert len(a) == 14 and a[6] == C.POINTER(E) and a[7] == C.POINTER(pkg.PitchTrackParams) and a[13] == C.POINTER(pkg.PitchTrackOutputs)
    assert lib.vbx_find_formants_resampled_f64.argtypes[5:8] == [C.c_double, C.c_double, C.c_size_t]
    assert len(lib.vbx_find_formants_resampled_f64.argtypes) == len(lib.vbx_find_formants_f64.argtypes) + 1
    assert lib.vbx_abi_version() == 5


def test_record_doubles_ex_adds_the_rms_column_last(pkg):
    """vbx_record_doubles_ex is host arithmetic: every existing column keeps its offset, RMS is one more column at the end."""
    lib = pkg.load_library()
    for kw in (dict(), dict(lpc_order=0), dict(formant_order=0), dict(mfcc=None), dict(lpc_order=0, formant_order=0, mfcc=None)):
        p = pkg.AnalysisParams.make(48000.0, **kw)
        rec = int(lib.vbx_record_doubles(C.byref(p)))
        assert rec == max(c0 + w for c0, w in p.columns().values())
        assert int(lib.vbx_record_doubles_ex(C.byref(p), None)) == rec
        assert int(lib.vbx_record_doubles_ex(C.byref(p), C.byref(pkg.AnalysisExt.make()))) == rec
        assert int(lib.vbx_record_doubles_ex(C.byref(p), C.byref(pkg.AnalysisExt.make(0.25, formant_sample_rate=12000.0)))) == rec
        assert int(lib.vbx_record_doubles_ex(C.byref(p), C.byref(pkg.AnalysisExt.make(0.25, rms=True)))) == rec + 1
    assert int(lib.vbx_record_doubles_ex(None, None)) == 0


def test_c_layout_matches_the_ctypes_mirror(pkg, tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "voxbox_hip.h"\n'
           'int main(void){ printf("%zu %zu %zu %zu\\n", sizeof(vbx_analysis_ext), offsetof(vbx_analysis_ext, formant_resample_ratio),\n'
           '  offsetof(vbx_analysis_ext, formant_sample_rate), offsetof(vbx_analysis_ext, rms)); return 0; }\n')
    c = tmp_path / "layout.c"
    c.write_text(src)
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)],
                       text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], text=True, capture_output=True, check=True).stdout.split()]
    E = pkg.AnalysisExt
    assert got == [C.sizeof(E), E.formant_resample_ratio.offset, E.formant_sample_rate.offset, E.rms.offset]


def test_cpp_mirror_compiles_with_the_delegates():
    hdr = os.path.join(ROOT, "vox_box.rs_amd", "host")
    src = ('#include "voxbox.hpp"\n'
           'int main(){ voxbox::Context c(0); voxbox::Frames f; voxbox::AnalysisParams p = voxbox::analysis_params(48000.0);\n'
           '  voxbox::AnalysisExt none = voxbox::analysis_ext();\n'
           '  voxbox::AnalysisExt e = voxbox::analysis_ext(10000.0 / 44100.0, true, 10000.0);\n'
           '  voxbox::PitchTrackParams t = voxbox::pitch_track_params(4);\n'
           '  voxbox::PitchTrackOutputs o{};\n'
           '  voxbox::analyze_frames_ex(c, f, p, e, nullptr, voxbox::Segments{}, nullptr, 38);\n'
           '  voxbox::analyze_frames_ex(c, f, p, e, &t, voxbox::Segments{}, nullptr, 38, nullptr, &o);\n'
           '  voxbox::analyze_frames_ex_pcm16(c, nullptr, 0, 1200, 480, p, none, nullptr, voxbox::Segments{}, nullptr, 36);\n'
           '  voxbox::analyze_frames_ex_pcm16(c, nullptr, 0, 1200, 480, p, e, &t, voxbox::Segments{}, nullptr, 38, nullptr, &o);\n'
           '  std::vector<voxbox::Resonance> est(4);\n'
           '  voxbox::find_formants(c, f, 10000.0, 13, voxbox::Segments{}, est, nullptr, nullptr, nullptr, nullptr, nullptr, 10000.0 / 44100.0);\n'
           '  return (voxbox::record_doubles(p, e) == voxbox::record_doubles(p) + 1 && voxbox::record_doubles(p, none) == 36 &&\n'
           '          none.rms == 0 && e.rms == 1 && e.formant_sample_rate == 10000.0) ? 0 : 1; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", hdr, "-x", "c++", "-"],
                       input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(hdr, "voxbox.hpp")).read()
    for n in NEW:
        assert n + "(" in text, n                                            # every new entry point has its delegate


def test_rust_layer_calls_the_example_abi():
    gpu = open(os.path.join(ROOT, "bindings", "rust", "src", "gpu.rs")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    lib = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for n in NEW:
        assert "ffi::" + n + "(" in gpu, n
        assert "pub fn " + n + "(" in ffi, n
    assert len(re.findall(r"pub fn analyze_ex\(&self", gpu)) == 2            # FrameBatch and PcmBatch, next to `pub fn analyze`
    assert "pub struct AnalysisExt" in gpu and "AnalysisExt" in lib
    m = re.search(r"pub struct VbxAnalysisExt \{(.*?)\}", ffi, re.S)
    assert m and re.findall(r"pub (\w+): (\w+),", m.group(1)) == [("formant_resample_ratio", "f64"), ("formant_sample_rate", "f64"),
                                                                  ("rms", "i32")]
    m = re.search(r"pub fn vbx_analyze_frames_ex_pcm16\((.*?)\) -> c_int;", ffi, re.S)
    assert "pcm: *const i16" in m.group(1) and "h_ext: *const VbxAnalysisExt" in m.group(1)
    assert "h_track: *const VbxPitchTrackParams" in m.group(1) and "h_outputs: *const VbxPitchTrackOutputs" in m.group(1)
    m = re.search(r"pub fn vbx_find_formants_resampled_f64\((.*?)\) -> c_int;", ffi, re.S)
    assert "sample_rate: f64,\n        resample_ratio: f64,\n        n_coeffs: usize" in m.group(1)
    # find_formants takes its ratio through the new entry point; the resampler on its own keeps a caller
    body = gpu[gpu.index("pub fn find_formants("):gpu.index("// spectrum.rs: EstimateFormants")]
    assert "ffi::vbx_find_formants_resampled_f64(" in body and "ffi::vbx_resample_linear_f64(" not in body
    assert "pub fn resample(&self, resample_ratio: f64)" in gpu and "ffi::vbx_resample_linear_f64(" in gpu
    gen = open(os.path.join(ROOT, "tools", "gen_rust_ffi.py")).read()
    assert "VbxAnalysisExt" in gen and '"vbx_analysis_ext": "VbxAnalysisExt"' in gen     # the mirror comes from the generator's prelude


def test_new_kernels_live_in_new_translation_units():
    """The resampled loaders and the RMS kernels are additions: the sources of the kernels they are modelled on are untouched
    files, and every new unit is picked up by the Makefile's wildcard."""
    csrc = os.path.join(ROOT, "vox_box.rs_amd", "csrc")
    units = ["k_burg_resampled.hip", "k_front_ex.hip"] + [f"k_burg_resampled_p{p}.hip" for p in (8, 10, 12, 13, 14, 16)]
    for u in units:
        assert os.path.getsize(os.path.join(csrc, u)) > 0, u
    assert "$(wildcard csrc/*.hip)" in open(os.path.join(ROOT, "vox_box.rs_amd", "Makefile")).read()
    hpp = open(os.path.join(csrc, "vbx_burg_resampled.hpp")).read()
    assert "burg_lags_resampled_kernel" in hpp and "#pragma clang fp contract(off)" in hpp
    for p in (8, 10, 12, 13, 14, 16):
        assert f"VBX_BURG_RESAMPLED_INSTANTIATE({p})" in open(os.path.join(csrc, f"k_burg_resampled_p{p}.hip")).read()
