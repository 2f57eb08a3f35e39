"""vbx_pitch_boersma_f64 through the layers above the kernel: the exported symbol, the ctypes signature against the header, the C++
delegate, the Rust layer, and examples/pitch_boersma.c (compiled here; run where there is a GPU)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TO_CTYPES = {"vbx_ctx *": "vp", "const double *": "vp", "size_t": "sz", "double": "dbl", "vbx_pitch *": "vp", "int32_t *": "vp"}


def _declaration():
    h = open(os.path.join(ROOT, "include", "voxbox_hip.h")).read()
    m = re.search(r"\nint vbx_pitch_boersma_f64\(([^;]*)\);", h)
    assert m, "include/voxbox_hip.h does not declare vbx_pitch_boersma_f64"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_the_symbol_is_exported(pkg):
    assert "vbx_pitch_boersma_f64" in pkg.exported_symbols()
    assert hasattr(pkg.load_library(), "vbx_pitch_boersma_f64")
    h = open(os.path.join(ROOT, "include", "voxbox_hip.h")).read()
    assert re.search(r"#define VBX_ABI_VERSION 5\b", h)          # added under the same ABI version


def test_ctypes_signature_matches_the_header(pkg):
    args = _declaration()
    names = [a.split()[-1].lstrip("*") for a in args]
    assert names == ["ctx", "x", "n_frames", "frame_len", "stride", "window", "sample_rate", "threshold", "fmin", "fmax", "kmax",
                     "out_cand", "out_count", "status"]
    kinds = []
    for a in args:
        t = a[:a.rindex(a.split()[-1].lstrip("*"))].strip()
        t = t if not t.endswith("*") else t[:-1].strip() + " *"
        kinds.append(C_TO_CTYPES[t])
    src = open(os.path.join(ROOT, "vox_box.rs_amd", "voxbox.py")).read()
    assert f'"vbx_pitch_boersma_f64": (C.c_int, [{", ".join(kinds)}])' in src
    # the same argument list as vbx_pitch_f64: the two calls are interchangeable at a call site
    assert '"vbx_pitch_f64": (C.c_int, [' + ", ".join(kinds) + "])" in src
    import ctypes as C
    fn = pkg.load_library().vbx_pitch_boersma_f64
    assert fn.restype is C.c_int and len(fn.argtypes) == 14
    assert [fn.argtypes[i] for i in (6, 7, 8, 9)] == [C.c_double] * 4 and [fn.argtypes[i] for i in (2, 3, 4, 10)] == [C.c_size_t] * 4


def test_cpp_delegate_compiles(tmp_path):
    src = ('#include "voxbox.hpp"\n'
           'int main(){ voxbox::Context c(0); voxbox::Frames f;\n'
           '  voxbox::Pitched::pitch_boersma(c, f, 48000.0, 0.2, 75.0, 600.0, 15, nullptr, nullptr, nullptr); return 0; }\n')
    p = tmp_path / "t.cpp"
    p.write_text(src)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "vox_box.rs_amd", "host"), str(p)], text=True, capture_output=True)
    assert r.returncode == 0, r.stderr


def test_rust_layer_calls_the_entry_point():
    gpu = open(os.path.join(ROOT, "bindings", "rust", "src", "gpu.rs")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert "pub fn vbx_pitch_boersma_f64(" in ffi
    assert re.search(r"pub fn pitch_boersma_all\(&self[^{]*\{.*?ffi::vbx_pitch_boersma_f64\(", gpu, re.S)


def _build_example(tmp_path):
    exe = str(tmp_path / "pitch_boersma")
    lib = os.path.join(ROOT, "vox_box.rs_amd", "lib")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "pitch_boersma.c"), "-L", lib, "-lvoxbox_hip",
                        "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib", "-lm", "-o", exe], text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_c_example_compiles_and_links(pkg, tmp_path):
    """examples/pitch_boersma.c: plain C against the header, every entry point it uses resolves in the library"""
    _build_example(tmp_path)
    src = open(os.path.join(ROOT, "examples", "pitch_boersma.c")).read()
    for fn in ("vbx_pitch_boersma_f64(", "vbx_frame_peak_f64(", "vbx_pitch_path_f64(", "vbx_pitch_f64("):
        assert fn in src, fn


@pytest.mark.gpu
def test_the_c_example_runs(pkg, tmp_path):
    """A 180 -> 240 Hz glide: the tracked contour stays voiced and on the glide.  The bound is the glide's own spread inside one
    frame (60 Hz/s over 25 ms: 1.5 Hz of ~200, 0.75 %) with a factor of two to spare, not a claim about the refinement."""
    exe = _build_example(tmp_path)
    r = subprocess.run([exe], text=True, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("frame")]
    assert len(rows) >= 9, r.stdout
    for ln in rows:
        glide, path, ref = (float(v) for v in re.findall(r"([-\d.]+) Hz", ln))
        assert abs(path - glide) <= 0.015 * glide, ln
    assert "worst relative error" in r.stdout.splitlines()[-1]
