"""A multi-channel live session (vbx_session_open_channels, vbx_session_push_channels[_device], vbx_session_channels_plan) at every
layer above the C ABI, checked without a GPU: the header, the Python mirror, the built library's exports, the C++ mirror, the Rust
layers, the plain-C example, where the kernels live and what they cost."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vbx_session_channels_plan", "vbx_session_open_channels", "vbx_session_push_channels", "vbx_session_push_channels_device",
       "vbx_session_path_bind_channels")


def _header():
    h = open(os.path.join(ROOT, "include", "voxbox_hip.h")).read()
    return h, " ".join(re.sub(r"/\*.*?\*/", "", h, flags=re.S).split())


def test_header_declares_the_multi_channel_session():
    h, flat = _header()
    assert ("typedef struct { vbx_session_plan_t push; size_t frames; size_t base; size_t keep; size_t len; size_t plane_frames; size_t plane_ld; "
            "size_t call_frames; size_t capacity; } vbx_session_channels_plan_t;") in flat
    assert ("int vbx_session_channels_plan(size_t consumed, size_t utt_frame, size_t n_new, size_t frame_len, size_t stride, size_t elem_bytes, "
            "size_t n_sel, vbx_session_channels_plan_t *h_out, int64_t *h_seg_start);") in flat
    assert ("int vbx_session_open_channels(vbx_ctx *ctx, const vbx_host_audio *h_fmt , const int32_t *h_channels, size_t n_sel, size_t frame_len, "
            "size_t stride, const vbx_analysis_params *h_params, const vbx_analysis_ext *h_ext, const vbx_pitch_track_params *h_track, "
            "size_t max_block_sample_frames, vbx_session **out);") in flat
    for name, block in (("vbx_session_push_channels", "h_block"), ("vbx_session_push_channels_device", "d_block")):
        m = re.search(r"int " + name + r"\((.*?)\);", flat)
        args = [a.strip() for a in m.group(1).split(",")]
        assert args == ["vbx_session *s", "const void *" + block, "size_t n_sample_frames", "const vbx_channel_outputs *h_out", "size_t record_ld",
                        "size_t status_ld", "size_t *h_n_frames"], args
    assert ("typedef struct { vbx_pitch *out_path; int32_t *out_index; uint8_t *out_forced; vbx_path_commit *d_commit; } "
            "vbx_channel_path_outputs;") in flat
    assert ("int vbx_session_path_bind_channels(vbx_session *s, double peak_ref, size_t max_pending, const vbx_channel_path_outputs *h_out , "
            "size_t path_ld);") in flat
    assert re.search(r"#define VBX_ABI_VERSION 5\b", h)                      # the change only adds
    # the block sits behind the online path and before the multi-GPU block, and says what it promises
    a, b, c = (h.index("the pitch path while the lists arrive (ABI 5, added)"), h.index("live sessions over several channels (ABI 5, added)"),
               h.index("multi-GPU: frame-range sharding"))
    assert a < b < c
    block = h[b:c]
    for n in NEW + ("vbx_session_channels_plan_t", "bit for bit", "session_ingest_all", "session_deliver_all", "[0, Q, 2Q, ...]", "256 bytes",
                    "do not mix", "VBX_HOST_MAX_CHANNELS", "vbx_session_mark_utterance", "DESIGN.md section 5i", "pitch_path_online_all",
                    "vbx_channel_path_outputs"):
        assert n in block, n
    assert "vbx_internal_session_ingest_channels" not in h                    # the test hook stays out of the public header
    # the one-channel session and the shared output struct are what they were
    assert ("int vbx_session_push(vbx_session *s, const void *h_block, size_t n_sample_frames, double *out_records , size_t record_ld, "
            "int32_t *status3 , size_t status_ld, const vbx_pitch_track_outputs *h_outputs , size_t *h_n_frames);") in flat
    assert "typedef struct { double *records; int32_t *status3; const vbx_pitch_track_outputs *outputs; } vbx_channel_outputs;" in flat


def test_python_mirror_and_exports(pkg):
    assert set(NEW) <= set(pkg.exported_symbols())
    lib = pkg.load_library()
    for n in NEW + ("vbx_internal_session_ingest_channels",):
        assert hasattr(lib, n), n
    assert lib.vbx_abi_version() == 5
    vp, sz = C.c_void_p, C.c_size_t
    assert [f[0] for f in pkg.SessionChannelsPlan._fields_] == ["push", "frames", "base", "keep", "len", "plane_frames", "plane_ld", "call_frames",
                                                               "capacity"]
    assert C.sizeof(pkg.SessionChannelsPlan) == 48 + 8 * 8 and pkg.SessionChannelsPlan.frames.offset == 48
    assert lib.vbx_session_channels_plan.argtypes == [sz] * 7 + [C.POINTER(pkg.SessionChannelsPlan), C.POINTER(C.c_int64)]
    a = lib.vbx_session_open_channels.argtypes
    assert len(a) == 11 and a[1] == C.POINTER(pkg.HostAudio) and a[3] == sz and a[6] == C.POINTER(pkg.AnalysisParams) and a[10] == C.POINTER(vp)
    for fn in (lib.vbx_session_push_channels, lib.vbx_session_push_channels_device):
        assert fn.argtypes == [vp, vp, sz, C.POINTER(pkg.ChannelOutputs), sz, sz, C.POINTER(sz)]
    assert len(lib.vbx_internal_session_ingest_channels.argtypes) == 13
    assert [f[0] for f in pkg.ChannelPathOutputs._fields_] == ["out_path", "out_index", "out_forced", "d_commit"] and C.sizeof(pkg.ChannelPathOutputs) == 32
    assert lib.vbx_session_path_bind_channels.argtypes == [vp, C.c_double, sz, C.POINTER(pkg.ChannelPathOutputs), sz]
    assert list(inspect.signature(pkg.SessionChannels.bind_path).parameters) == ["self", "out_path", "commit", "peak_ref", "max_pending", "path_ld",
                                                                                "out_index", "out_forced"]
    assert list(inspect.signature(pkg.session_channels_plan).parameters) == ["consumed", "utt_frame", "n_new", "frame_len", "stride", "elem_bytes",
                                                                             "n_sel"]
    assert list(inspect.signature(pkg.VoxBox.session_channels).parameters) == ["self", "params", "ext", "track", "format", "channels", "select",
                                                                               "frame_len", "stride", "max_block"]
    assert list(inspect.signature(pkg.SessionChannels.push).parameters)[:5] == ["self", "block", "out", "status", "outputs"]
    assert list(inspect.signature(pkg.SessionChannels.push_device).parameters)[:6] == ["self", "block", "n_sample_frames", "out", "status", "outputs"]
    for m in ("mark_utterance", "reset", "info", "close", "__enter__", "__exit__"):
        assert callable(getattr(pkg.SessionChannels, m)), m


def test_null_arguments_are_refused_without_a_gpu(pkg):
    lib = pkg.load_library()
    h = C.c_void_p()
    n = C.c_size_t(7)
    assert lib.vbx_session_open_channels(None, None, None, 2, 1200, 480, None, None, None, 4800, C.byref(h)) == -1 and not h.value
    assert lib.vbx_session_push_channels(None, None, 0, None, 0, 0, C.byref(n)) == -1                     # NULL session
    assert lib.vbx_session_push_channels_device(None, None, 480, None, 36, 0, None) == -1
    assert b"null session" in lib.vbx_last_error(None)
    assert lib.vbx_session_path_bind_channels(None, 1.0, 64, None, 2) == -1
    assert lib.vbx_internal_session_ingest_channels(None, 1, 2, None, 2, None, 0, 0, 0, None, 0, None, 0) == -1
    assert lib.vbx_session_channels_plan(0, 0, 480, 1200, 480, 2, 2, None, None) == -1


def test_cpp_mirror_compiles_with_the_multi_channel_session():
    hdr = os.path.join(ROOT, "vox_box.rs_amd", "host")
    src = ('#include "voxbox.hpp"\n'
           'int main(){ voxbox::Context c(0); voxbox::AnalysisParams p = voxbox::analysis_params(48000.0);\n'
           '  const int32_t sel[2] = {1, 0}; voxbox::ChannelOutputs out[2] = {};\n'
           '  voxbox::session_channels s(c, voxbox::host_audio(VBX_SAMPLE_PCM16, 2, 0), sel, 2, 1200, 480, p, nullptr, nullptr, 4800);\n'
           '  size_t n = s.push(nullptr, 0, out, 36);\n'
           '  n += s.push_device(nullptr, 0, out, 36, 0);\n'
           '  vbx_channel_path_outputs po[2] = {}; s.bind_path(1.0, 64, po);\n'
           '  s.mark_utterance(); s.reset();\n'
           '  int64_t seg[2];\n'
           '  voxbox::SessionChannelsPlan pl = voxbox::session_channels_plan(0, 0, 1200, 1200, 480, 2, 2, seg);\n'
           '  static_assert(sizeof(voxbox::SessionChannelsPlan) == 112, "the push plan and eight sizes");\n'
           '  return (int)(n + s.info().frames + pl.call_frames + (size_t)seg[1]); }\n')
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
    assert "pub struct VbxSessionChannelsPlan {" in ffi and "pub push: VbxSessionPlan," in ffi
    assert "pub struct VbxChannelPathOutputs {" in ffi and "pub fn bind_path(&self, peak_ref: f64, max_pending: usize, rows: &[PathRows" in gpu
    assert "pub fn session_channels(&self" in gpu and "pub struct SessionChannels<" in gpu and "pub fn session_channels_plan(" in gpu
    m = re.search(r"pub fn vbx_session_push_channels\((.*?)\) -> c_int;", ffi, re.S)
    for part in ("s: *mut VbxSession", "h_block: *const c_void", "h_out: *const VbxChannelOutputs", "status_ld: usize", "h_n_frames: *mut usize"):
        assert part in m.group(1), part
    m = re.search(r"pub fn vbx_session_open_channels\((.*?)\) -> c_int;", ffi, re.S)
    assert "h_channels: *const i32" in m.group(1) and "n_sel: usize" in m.group(1) and "out: *mut *mut VbxSession" in m.group(1)


def test_the_c_example_compiles_and_links(pkg, tmp_path):
    """examples/live_array.c: plain C against the header, every entry point it uses resolves in the library"""
    lib = os.path.join(ROOT, "vox_box.rs_amd", "lib")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "live_array.c"),
                        "-L", lib, "-lvoxbox_hip", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(tmp_path / "live_array")],
                       text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(ROOT, "examples", "live_array.c")).read()
    assert "vbx_session_open_channels(" in src and "vbx_session_push_channels(" in src and "vbx_channel_outputs" in src


def test_the_kernels_live_in_their_units():
    read = lambda f: open(os.path.join(ROOT, "vox_box.rs_amd", "csrc", f)).read()
    k = read("k_session_channels.hip")
    assert "session_ingest_all_kernel" in k and "session_deliver_all_kernel" in k and '#include "vbx_reader.hpp"' in k
    # the readers' own arithmetic and the reader's own tile code, not a copy of either
    assert "read_one<FMT>" in k and "read_group_wide<FMT>" in k and "lds_one<FMT>" in k and "lds_stage_tile(" in k
    assert "pcm24_value" not in k and "8388607" not in k and "2147483647" not in k
    hpp, reader = read("vbx_reader.hpp"), read("k_reader.hip")
    assert "lds_one(const uint32_t *tile" in hpp and "void lds_stage_tile(" in hpp
    assert "lds_one<FMT>" in reader and "lds_stage_tile(" in reader and "lds_one(const uint32_t *tile" not in reader
    assert "tracker_stitch_all_kernel" in read("k_tracker.hip")
    # the online path of all channels: a unit of its own beside k_pitch_path.hip, on the same per-frame device functions, without FMA
    pc, pp, step = read("k_pitch_path_channels.hip"), read("k_pitch_path.hip"), read("vbx_pitch_path_step.hpp")
    assert "pp_online_all_kernel" in pc and "pp_online_all" not in pp
    for n in ("pp_fetch(", "pp_decode<G>(", "pp_step<G>(", "pp_leader<G>("):
        assert n in pc and n in pp, n
    for n in ("void pp_fetch(", "void pp_decode(", "double pp_step(", "int pp_leader("):
        assert n in step and n not in pc and n not in pp, n
    for text in (pc, pp, step):
        assert "#pragma clang fp contract(off)" in text and "fma(" not in text
    assert '#include "vbx_pitch_path_step.hpp"' in pc and '#include "vbx_pitch_path_step.hpp"' in pp
    assert '"pitch_path_online_all"' in read("vbx_api_path.hip") and "void launch_pitch_path_online_all(" in read("vbx_kernels.hpp")
    kh = read("vbx_kernels.hpp")
    assert "void launch_session_ingest_all(" in kh and "void launch_session_deliver_all(" in kh and "void launch_tracker_stitch_all(" in kh
    assert "int vbx_session_channels_plan(" in read("vbx_host.cpp")
    api = read("vbx_api_session.hip")
    for name in ("session_ingest_all_pcm16", "session_ingest_all_pcm24", "session_ingest_all_pcm32", "session_ingest_all_f32", "session_ingest_all_f64",
                 "session_deliver_all", "tracker_stitch_all"):
        assert '"' + name + '"' in api, name


def test_the_new_kernels_have_no_scratch_and_no_spills():
    """the committed record is what tools/resource_usage.sh prints for the unit as it stands"""
    r = subprocess.run([os.path.join(ROOT, "tools", "resource_usage.sh"), os.path.join("vox_box.rs_amd", "csrc", "k_session_channels.hip")],
                       cwd=ROOT, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    built = [ln for ln in r.stdout.splitlines() if "session_ingest_all_kernel" in ln or "session_deliver_all_kernel" in ln]
    usage = open(os.path.join(ROOT, "profiles", "session_channels", "resource_usage.txt")).read()
    rows = [ln for ln in usage.splitlines() if "session_ingest_all_kernel" in ln or "session_deliver_all_kernel" in ln]
    assert len(rows) == 6 and [ln.split() for ln in rows] == [ln.split() for ln in built]
    r = subprocess.run([os.path.join(ROOT, "tools", "resource_usage.sh"), os.path.join("vox_box.rs_amd", "csrc", "k_tracker.hip")],
                       cwd=ROOT, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    built = [ln for ln in r.stdout.splitlines() if "tracker_stitch_all_kernel" in ln]
    stitch_rows = [ln for ln in usage.splitlines() if "tracker_stitch_all_kernel" in ln]
    assert len(stitch_rows) == 6 and [ln.split() for ln in stitch_rows] == [ln.split() for ln in built]
    rows += stitch_rows
    assert len(rows) == 12
    r = subprocess.run([os.path.join(ROOT, "tools", "resource_usage.sh"), os.path.join("vox_box.rs_amd", "csrc", "k_pitch_path_channels.hip")],
                       cwd=ROOT, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    built = [ln for ln in r.stdout.splitlines() if "pp_online_all_kernel" in ln]
    path_rows = [ln for ln in usage.splitlines() if "pp_online_all_kernel" in ln]
    assert len(path_rows) == 5 and [ln.split() for ln in path_rows] == [ln.split() for ln in built]
    rows += path_rows
    for ln in rows:
        assert re.search(r"scratch\s+0\b", ln) and re.search(r"vspill\s+0\b", ln) and re.search(r"sspill\s+0\b", ln), ln
