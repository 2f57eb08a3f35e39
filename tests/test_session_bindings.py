"""Live sessions (vbx_session_*) at every layer above the C ABI, checked without a GPU: the header, the Python mirror, the built
library's exports, the C++ mirror, the Rust layers and the plain-C example."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vbx_session_plan", "vbx_session_open", "vbx_session_push", "vbx_session_push_device", "vbx_session_mark_utterance",
       "vbx_session_reset", "vbx_session_info", "vbx_session_close")


def _header():
    h = open(os.path.join(ROOT, "include", "voxbox_hip.h")).read()
    return h, " ".join(re.sub(r"/\*.*?\*/", "", h, flags=re.S).split())


def test_header_declares_the_session():
    h, flat = _header()
    assert "typedef struct vbx_session vbx_session;" in flat
    assert ("typedef struct { size_t lo, hi; size_t warm; int continues_prev; size_t read_from; size_t keep_from; } vbx_session_plan_t;") in flat
    assert ("int vbx_session_plan(size_t consumed, size_t utt_frame, size_t n_new, size_t frame_len, size_t stride, "
            "vbx_session_plan_t *h_out);") in flat
    assert ("int vbx_session_open(vbx_ctx *ctx, const vbx_host_audio *h_fmt , size_t frame_len, size_t stride, "
            "const vbx_analysis_params *h_params, const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track, "
            "size_t max_block_sample_frames, vbx_session **out);") in flat
    for name, block in (("vbx_session_push", "h_block"), ("vbx_session_push_device", "d_block")):
        m = re.search(r"int " + name + r"\((.*?)\);", flat)
        args = [a.strip() for a in m.group(1).split(",")]
        assert args == ["vbx_session *s", "const void *" + block, "size_t n_sample_frames", "double *out_records", "size_t record_ld",
                        "int32_t *status3", "size_t status_ld", "const vbx_pitch_track_outputs *h_outputs", "size_t *h_n_frames"], args
    assert "int vbx_session_mark_utterance(vbx_session *s);" in flat and "int vbx_session_reset(vbx_session *s);" in flat
    assert "int vbx_session_info(const vbx_session *s, size_t *h_consumed, size_t *h_frames, size_t *h_carried);" in flat
    assert "void vbx_session_close(vbx_session *s);" in flat
    assert re.search(r"#define VBX_ABI_VERSION 5\b", h)                      # the change only adds
    # the block sits behind the host-resident recordings and before the multi-GPU block, and says what it promises
    a, b, c = h.index("host-resident recordings (ABI 5, added)"), h.index("live sessions (ABI 5, added)"), h.index("multi-GPU: frame-range sharding")
    assert a < b < c
    block = h[b:c]
    for n in NEW + ("vbx_session_plan_t", "bit for bit", "VBX_SHARD_WARM_FRAMES", "session_ingest", "session_deliver", "vbx_pitch_path_f64",
                    "max_block_sample_frames", "h_seg_start = [0, m1, m2, ...]", "DESIGN.md section 5g"):
        assert n in block, n
    assert "vbx_internal_session_ingest" not in h                             # the test hook stays out of the public header
    # the host-resident declarations are what they were
    assert "int vbx_unpack_samples(vbx_ctx *ctx, const void *d_src, size_t n_sample_frames, int format, int channels, int channel, void *d_out);" in flat
    assert "typedef struct { int32_t format; int32_t channels; int32_t channel; int32_t reserved; size_t chunk_frames; } vbx_host_audio;" in flat
    assert ("int vbx_analyze_host(vbx_ctx *ctx, const void *h_audio, size_t n_sample_frames, const vbx_host_audio *h_fmt, size_t frame_len, "
            "size_t stride, const vbx_analysis_params *h_params, const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track, "
            "const int64_t *h_seg_start, size_t n_segments, double *out_records , size_t record_ld, int32_t *status3 , "
            "const vbx_pitch_track_outputs *h_outputs );") in flat
    assert ("int vbx_host_chunk_plan(size_t n_frames, size_t chunk_frames, size_t c, size_t frame_len, size_t stride, "
            "const int64_t *h_seg_start, size_t n_segments, vbx_shard_plan_t *h_out, size_t *s0, size_t *s1);") in flat


def test_python_mirror_and_exports(pkg):
    assert set(NEW) <= set(pkg.exported_symbols())
    lib = pkg.load_library()
    for n in NEW + ("vbx_internal_session_ingest",):
        assert hasattr(lib, n), n
    assert lib.vbx_abi_version() == 5
    vp, sz = C.c_void_p, C.c_size_t
    assert [f[0] for f in pkg.SessionPlan._fields_] == ["lo", "hi", "warm", "continues_prev", "read_from", "keep_from"]
    assert C.sizeof(pkg.SessionPlan) == 48 and pkg.SessionPlan.read_from.offset == 32
    assert lib.vbx_session_plan.argtypes == [sz, sz, sz, sz, sz, C.POINTER(pkg.SessionPlan)]
    a = lib.vbx_session_open.argtypes
    assert len(a) == 9 and a[1] == C.POINTER(pkg.HostAudio) and a[4] == C.POINTER(pkg.AnalysisParams) and a[7] == sz and a[8] == C.POINTER(vp)
    for fn in (lib.vbx_session_push, lib.vbx_session_push_device):
        assert fn.argtypes == [vp, vp, sz, vp, sz, vp, sz, C.POINTER(pkg.PitchTrackOutputs), C.POINTER(sz)]
    assert lib.vbx_session_info.argtypes == [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    assert lib.vbx_session_close.restype is None and lib.vbx_session_close.argtypes == [vp]
    assert len(lib.vbx_internal_session_ingest.argtypes) == 10
    assert list(inspect.signature(pkg.session_plan).parameters) == ["consumed", "utt_frame", "n_new", "frame_len", "stride"]
    assert list(inspect.signature(pkg.VoxBox.session).parameters) == ["self", "params", "ext", "track", "format", "channels", "channel",
                                                                      "frame_len", "stride", "max_block"]
    assert list(inspect.signature(pkg.Session.push).parameters)[:5] == ["self", "block", "out", "status", "outputs"]
    assert list(inspect.signature(pkg.Session.push_device).parameters)[:6] == ["self", "block", "n_sample_frames", "out", "status", "outputs"]
    for m in ("mark_utterance", "reset", "info", "close", "__enter__", "__exit__"):
        assert callable(getattr(pkg.Session, m)), m


def test_null_arguments_are_refused_without_a_gpu(pkg):
    lib = pkg.load_library()
    h = C.c_void_p()
    n = C.c_size_t(7)
    assert lib.vbx_session_open(None, None, 1200, 480, None, None, None, 4800, C.byref(h)) == -1 and not h.value      # NULL context
    assert lib.vbx_session_push(None, None, 0, None, 0, None, 0, None, C.byref(n)) == -1                               # NULL session
    assert lib.vbx_session_push_device(None, None, 480, None, 36, None, 0, None, None) == -1
    assert lib.vbx_session_mark_utterance(None) == -1 and lib.vbx_session_reset(None) == -1
    assert lib.vbx_session_info(None, None, None, None) == -1
    assert lib.vbx_session_close(None) is None                                                                         # a no-op
    assert lib.vbx_internal_session_ingest(None, 1, 1, 0, None, 0, 0, None, 0, None) == -1
    assert b"null session" in lib.vbx_last_error(None) or b"null context" in lib.vbx_last_error(None)


def test_cpp_mirror_compiles_with_the_session():
    hdr = os.path.join(ROOT, "vox_box.rs_amd", "host")
    src = ('#include "voxbox.hpp"\n'
           'int main(){ voxbox::Context c(0); voxbox::AnalysisParams p = voxbox::analysis_params(48000.0);\n'
           '  voxbox::session s(c, voxbox::host_audio(VBX_SAMPLE_PCM16, 2, 1), 1200, 480, p, nullptr, nullptr, 4800);\n'
           '  size_t n = s.push(nullptr, 0, nullptr, 36);\n'
           '  n += s.push_device(nullptr, 0, nullptr, 36, nullptr, 0, nullptr);\n'
           '  s.mark_utterance(); s.reset();\n'
           '  voxbox::SessionPlan pl = voxbox::session_plan(0, 0, 1200, 1200, 480);\n'
           '  static_assert(sizeof(voxbox::SessionPlan) == 48, "five sizes and a flag");\n'
           '  return (int)(n + s.info().frames + pl.hi); }\n')
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
    assert "pub struct VbxSession {" in ffi and "pub struct VbxSessionPlan {" in ffi
    assert "pub fn session(&self" in gpu and "pub struct Session<" in gpu and "impl<'g> Drop for Session<'g>" in gpu
    assert "pub fn session_plan(" in gpu
    m = re.search(r"pub fn vbx_session_push\((.*?)\) -> c_int;", ffi, re.S)
    for part in ("s: *mut VbxSession", "h_block: *const c_void", "status_ld: usize", "h_outputs: *const VbxPitchTrackOutputs", "h_n_frames: *mut usize"):
        assert part in m.group(1), part
    m = re.search(r"pub fn vbx_session_open\((.*?)\) -> c_int;", ffi, re.S)
    assert "h_fmt: *const VbxHostAudio" in m.group(1) and "out: *mut *mut VbxSession" in m.group(1)
    assert "pub fn vbx_session_info(\n        s: *const VbxSession" in ffi or "pub fn vbx_session_info(s: *const VbxSession" in ffi


def test_the_c_example_compiles_and_links(pkg, tmp_path):
    """examples/live_session.c: plain C against the header, every entry point it uses resolves in the library"""
    lib = os.path.join(ROOT, "vox_box.rs_amd", "lib")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "live_session.c"),
                        "-L", lib, "-lvoxbox_hip", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(tmp_path / "live_session")],
                       text=True, capture_output=True)
    assert r.returncode == 0, r.stderr


def test_the_kernels_live_in_their_own_unit():
    read = lambda f: open(os.path.join(ROOT, "vox_box.rs_amd", "csrc", f)).read()
    k = read("k_session.hip")
    assert "session_ingest_kernel" in k and "session_deliver_kernel" in k and '#include "vbx_reader.hpp"' in k
    assert "read_one<FMT>" in k and "read_group_wide<FMT>" in k             # the readers' own arithmetic, not a copy of it
    assert '#include "vbx_reader.hpp"' in read("k_reader.hip")
    hpp = read("vbx_kernels.hpp")
    assert "void launch_session_ingest(" in hpp and "void launch_session_deliver(" in hpp
    assert "session_carry_samples" in read("vbx_host.hpp") and "int vbx_session_plan(" in read("vbx_host.cpp")
    api = read("vbx_api_session.hip")
    for name in ("session_ingest_pcm16", "session_ingest_pcm24", "session_ingest_pcm32", "session_ingest_f32", "session_ingest_f64", "session_deliver"):
        assert '"' + name + '"' in api, name
    usage = open(os.path.join(ROOT, "profiles", "session", "resource_usage.txt")).read()
    rows = [ln for ln in usage.splitlines() if "session_ingest_kernel" in ln or "session_deliver_kernel" in ln]
    assert len(rows) == 6
    for ln in rows:
        assert re.search(r"scratch\s+0\b", ln) and re.search(r"vspill\s+0\b", ln) and re.search(r"sspill\s+0\b", ln), ln
