"""A session pool (vbx_pool_open, vbx_pool_push[_device], vbx_pool_mark_utterance, vbx_pool_reset_stream, vbx_pool_info, vbx_pool_close,
vbx_pool_plan) at every layer above the C ABI, checked without a GPU: the header, the Python mirror, the built library's exports, the
C++ mirror, the Rust layers, the plain-C example, where the kernels live and what they cost."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vbx_pool_plan", "vbx_pool_open", "vbx_pool_push", "vbx_pool_push_device", "vbx_pool_mark_utterance", "vbx_pool_reset_stream",
       "vbx_pool_info", "vbx_pool_close")


def _header():
    h = open(os.path.join(ROOT, "include", "voxbox_hip.h")).read()
    return h, " ".join(re.sub(r"/\*.*?\*/", "", h, flags=re.S).split())


def test_header_declares_the_pool():
    h, flat = _header()
    assert "typedef struct vbx_pool vbx_pool;" in flat
    assert "typedef struct { int32_t stream; const void *block; size_t n_sample_frames; } vbx_pool_entry;" in flat
    assert "typedef struct { int64_t row_start; int64_t n_rows; } vbx_pool_rows;" in flat
    assert "typedef struct { vbx_session_plan_t plan; int64_t row_start; int64_t n_rows; int64_t frames; int64_t plane_frame; } vbx_pool_plan_row;" in flat
    assert ("int vbx_pool_plan(const size_t *h_consumed, const size_t *h_utt_frame, const size_t *h_n_new, size_t n_entries, size_t frame_len, "
            "size_t stride, vbx_pool_plan_row *h_rows , size_t *h_total_rows, size_t *h_call_frames);") in flat
    assert ("int vbx_pool_open(vbx_ctx *ctx, const vbx_host_audio *h_fmt , size_t frame_len, size_t stride, const vbx_analysis_params *h_params, "
            "const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track, size_t max_streams, size_t max_block_sample_frames, "
            "size_t max_tick_sample_frames, vbx_pool **out);") in flat
    for name in ("vbx_pool_push", "vbx_pool_push_device"):
        m = re.search(r"int " + name + r"\((.*?)\);", flat)
        args = [a.strip() for a in m.group(1).split(",")]
        assert args == ["vbx_pool *pool", "const vbx_pool_entry *h_entries", "size_t n_entries", "double *out_records", "size_t record_ld",
                        "int32_t *status3", "size_t status_ld", "const vbx_pitch_track_outputs *h_outputs", "vbx_pool_rows *h_rows",
                        "size_t *h_total_rows"], args
    assert "int vbx_pool_mark_utterance(vbx_pool *pool, int32_t stream);" in flat and "int vbx_pool_reset_stream(vbx_pool *pool, int32_t stream);" in flat
    assert "int vbx_pool_info(const vbx_pool *pool, int32_t stream, size_t *h_consumed, size_t *h_frames, size_t *h_carried);" in flat
    assert "void vbx_pool_close(vbx_pool *pool);" in flat
    assert re.search(r"#define VBX_ABI_VERSION 5\b", h)                      # the change only adds
    # the block sits behind the clips and before the multi-GPU block, and says what it promises
    a, b, c = (h.index("a batch of variable-length clips (ABI 5, added)"), h.index("a pool of live streams (ABI 5, added)"),
               h.index("multi-GPU: frame-range sharding"))
    assert a < b < c
    block = h[b:c]
    for n in NEW + ("bit for bit", "pool_ingest_<fmt>", "tracker_stitch_pool", "pool_deliver", "ONE upload", "VBX_MAX_FRAME_LEN", "channels == 1",
                    "vbx_session_path_bind", "is NOT offered", "vbx_pitch_path_f64", "DESIGN.md section 5l", "listed twice", "max_tick_sample_frames",
                    "vbx_session_plan", "ceil(span / stride)", "0x7fffffff"):
        assert n in block, n
    assert "vbx_internal_pool_ingest" not in h                                # the test hook stays out of the public header
    # the one-channel session is what it was
    assert ("int vbx_session_push(vbx_session *s, const void *h_block, size_t n_sample_frames, double *out_records , size_t record_ld, "
            "int32_t *status3 , size_t status_ld, const vbx_pitch_track_outputs *h_outputs , size_t *h_n_frames);") in flat


def test_python_mirror_and_exports(pkg):
    assert set(NEW) <= set(pkg.exported_symbols())
    lib = pkg.load_library()
    for n in NEW + ("vbx_internal_pool_ingest",):
        assert hasattr(lib, n), n
    assert lib.vbx_abi_version() == 5
    vp, sz = C.c_void_p, C.c_size_t
    assert [f[0] for f in pkg.PoolEntry._fields_] == ["stream", "block", "n_sample_frames"] and C.sizeof(pkg.PoolEntry) == 24
    assert pkg.PoolEntry.block.offset == 8
    assert [f[0] for f in pkg.PoolRows._fields_] == ["row_start", "n_rows"] and C.sizeof(pkg.PoolRows) == 16
    assert [f[0] for f in pkg.PoolPlanRow._fields_] == ["plan", "row_start", "n_rows", "frames", "plane_frame"]
    assert C.sizeof(pkg.PoolPlanRow) == 48 + 32 and pkg.PoolPlanRow.row_start.offset == 48
    assert lib.vbx_pool_plan.argtypes == [C.POINTER(sz)] * 3 + [sz] * 3 + [C.POINTER(pkg.PoolPlanRow), C.POINTER(sz), C.POINTER(sz)]
    a = lib.vbx_pool_open.argtypes
    assert len(a) == 11 and a[1] == C.POINTER(pkg.HostAudio) and a[4] == C.POINTER(pkg.AnalysisParams) and a[7:10] == [sz] * 3 and a[10] == C.POINTER(vp)
    for fn in (lib.vbx_pool_push, lib.vbx_pool_push_device):
        assert fn.argtypes == [vp, C.POINTER(pkg.PoolEntry), sz, vp, sz, vp, sz, C.POINTER(pkg.PitchTrackOutputs), C.POINTER(pkg.PoolRows), C.POINTER(sz)]
    assert lib.vbx_pool_mark_utterance.argtypes == [vp, C.c_int32] and lib.vbx_pool_reset_stream.argtypes == [vp, C.c_int32]
    assert lib.vbx_pool_info.argtypes == [vp, C.c_int32] + [C.POINTER(sz)] * 3 and lib.vbx_pool_close.restype is None
    assert len(lib.vbx_internal_pool_ingest.argtypes) == 7
    assert list(inspect.signature(pkg.pool_plan).parameters) == ["consumed", "utt_frame", "n_new", "frame_len", "stride"]
    assert list(inspect.signature(pkg.VoxBox.pool).parameters) == ["self", "params", "ext", "track", "format", "frame_len", "stride", "max_streams",
                                                                   "max_block", "max_tick"]
    assert list(inspect.signature(pkg.Pool.push).parameters)[:5] == ["self", "entries", "out", "status", "outputs"]
    assert list(inspect.signature(pkg.Pool.push_device).parameters)[:5] == ["self", "entries", "out", "status", "outputs"]
    assert list(inspect.signature(pkg.Pool.info).parameters) == ["self", "stream"]
    for m in ("mark_utterance", "reset_stream", "info", "close", "__enter__", "__exit__"):
        assert callable(getattr(pkg.Pool, m)), m


def test_null_arguments_are_refused_without_a_gpu(pkg):
    lib = pkg.load_library()
    h = C.c_void_p()
    n = C.c_size_t(7)
    assert lib.vbx_pool_open(None, None, 200, 80, None, None, None, 8, 160, 1280, C.byref(h)) == -1 and not h.value
    assert lib.vbx_pool_push(None, None, 0, None, 0, None, 0, None, None, C.byref(n)) == -1                   # NULL pool
    assert lib.vbx_pool_push_device(None, None, 1, None, 4, None, 0, None, None, None) == -1
    assert b"null pool" in lib.vbx_last_error(None)
    assert lib.vbx_pool_mark_utterance(None, 0) == -1 and lib.vbx_pool_reset_stream(None, 0) == -1
    assert lib.vbx_pool_info(None, 0, None, None, None) == -1
    lib.vbx_pool_close(None)                                                                               # a no-op
    assert lib.vbx_internal_pool_ingest(None, 1, None, 0, 160, None, None) == -1
    assert lib.vbx_pool_plan(None, None, None, 2, 200, 80, None, None, None) == -1


def test_cpp_mirror_compiles_with_the_pool():
    hdr = os.path.join(ROOT, "vox_box.rs_amd", "host")
    src = ('#include "voxbox.hpp"\n'
           'int main(){ voxbox::Context c(0); voxbox::AnalysisParams p = voxbox::analysis_params(8000.0);\n'
           '  voxbox::pool q(c, voxbox::host_audio(VBX_SAMPLE_ULAW, 1, 0), 200, 80, p, nullptr, nullptr, 8, 160, 1280);\n'
           '  voxbox::PoolEntry e[1] = {}; voxbox::PoolRows r[1];\n'
           '  size_t n = q.push(e, 1, nullptr, 4, nullptr, 0, nullptr, r);\n'
           '  n += q.push_device(e, 1, nullptr, 4);\n'
           '  q.mark_utterance(0); q.reset_stream(0);\n'
           '  size_t a[1] = {0}, b[1] = {0}, d[1] = {200};\n'
           '  voxbox::PoolPlan pl = voxbox::pool_plan(a, b, d, 1, 200, 80);\n'
           '  static_assert(sizeof(voxbox::PoolPlanRow) == 80 && sizeof(voxbox::PoolEntry) == 24, "the session plan and four counts; slot, block, length");\n'
           '  return (int)(n + q.info(0).frames + pl.call_frames + (size_t)pl.rows[0].plane_frame); }\n')
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
    assert "pub struct VbxPool {" in ffi and "pub struct VbxPoolEntry {" in ffi and "pub struct VbxPoolRows {" in ffi
    assert "pub struct VbxPoolPlanRow {" in ffi and "pub plan: VbxSessionPlan," in ffi and "pub block: *const c_void," in ffi
    assert "pub fn pool(&self" in gpu and "pub struct Pool<" in gpu and "pub fn pool_plan(" in gpu and "impl Drop for Pool<" in gpu
    m = re.search(r"pub fn vbx_pool_push\((.*?)\) -> c_int;", ffi, re.S)
    for part in ("pool: *mut VbxPool", "h_entries: *const VbxPoolEntry", "n_entries: usize", "h_rows: *mut VbxPoolRows", "h_total_rows: *mut usize"):
        assert part in m.group(1), part
    m = re.search(r"pub fn vbx_pool_open\((.*?)\) -> c_int;", ffi, re.S)
    assert "max_streams: usize" in m.group(1) and "max_tick_sample_frames: usize" in m.group(1) and "out: *mut *mut VbxPool" in m.group(1)


def test_the_c_example_compiles_and_links(pkg, tmp_path):
    """examples/call_pool.c: plain C against the header, every entry point it uses resolves in the library"""
    lib = os.path.join(ROOT, "vox_box.rs_amd", "lib")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "call_pool.c"),
                        "-L", lib, "-lvoxbox_hip", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib", "-lm", "-o", str(tmp_path / "call_pool")],
                       text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(ROOT, "examples", "call_pool.c")).read()
    assert "vbx_pool_open(" in src and "vbx_pool_push(" in src and "vbx_pool_reset_stream(" in src and "VBX_SAMPLE_ULAW" in src


def test_the_kernels_live_in_their_units():
    read = lambda f: open(os.path.join(ROOT, "vox_box.rs_amd", "csrc", f)).read()
    k = read("k_pool.hip")
    assert "pool_ingest_kernel" in k and "pool_deliver_kernel" in k and '#include "vbx_reader.hpp"' in k
    # the readers' own arithmetic, not a copy of it
    assert "read_one<FMT>" in k and "read_group_wide<FMT>" in k
    for restated in ("pcm24_value", "8388607", "2147483647", "0x84", "0x55", "127.0"):
        assert restated not in k, restated
    for f in ("k_clips.hip", "k_session.hip", "k_session_channels.hip", "k_sample8.hip", "k_reader.hip"):
        assert "pool_" not in read(f), f
    assert "tracker_stitch_pool_kernel" in read("k_tracker.hip")
    kh = read("vbx_kernels.hpp")
    assert "void launch_pool_ingest(" in kh and "void launch_pool_deliver(" in kh and "void launch_tracker_stitch_pool(" in kh and "struct pool_entry_t {" in kh
    assert "int vbx_pool_plan(" in read("vbx_host.cpp") and "size_t pool_carry_samples(" in read("vbx_host.hpp")
    api = read("vbx_api_pool.hip")
    for name in ("pool_ingest_pcm16", "pool_ingest_pcm24", "pool_ingest_pcm32", "pool_ingest_f32", "pool_ingest_f64", "pool_ingest_u8", "pool_ingest_ulaw",
                 "pool_ingest_alaw", "tracker_stitch_pool", "pool_deliver"):
        assert '"' + name + '"' in api, name
    assert "int vbx_internal_pool_ingest(" in api and "struct vbx_pool {" in api


def test_the_new_kernels_have_no_scratch_and_no_spills():
    """the committed record is what tools/resource_usage.sh prints for the units as they stand"""
    usage = open(os.path.join(ROOT, "profiles", "pool", "resource_usage.txt")).read()
    r = subprocess.run([os.path.join(ROOT, "tools", "resource_usage.sh"), os.path.join("vox_box.rs_amd", "csrc", "k_pool.hip")],
                       cwd=ROOT, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    built = [ln for ln in r.stdout.splitlines() if "pool_ingest_kernel" in ln or "pool_deliver_kernel" in ln]
    rows = [ln for ln in usage.splitlines() if "pool_ingest_kernel" in ln or "pool_deliver_kernel" in ln]
    assert len(rows) == 9 and sum("pool_ingest_kernel" in ln for ln in rows) == 8 and [ln.split() for ln in rows] == [ln.split() for ln in built]
    r = subprocess.run([os.path.join(ROOT, "tools", "resource_usage.sh"), os.path.join("vox_box.rs_amd", "csrc", "k_tracker.hip")],
                       cwd=ROOT, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    built = [ln for ln in r.stdout.splitlines() if "tracker_stitch_pool_kernel" in ln]
    stitch_rows = [ln for ln in usage.splitlines() if "tracker_stitch_pool_kernel" in ln]
    assert len(stitch_rows) == 6 and [ln.split() for ln in stitch_rows] == [ln.split() for ln in built]
    rows += stitch_rows
    assert len(rows) == 15
    for ln in rows:
        assert re.search(r"scratch\s+0\b", ln) and re.search(r"vspill\s+0\b", ln) and re.search(r"sspill\s+0\b", ln), ln
