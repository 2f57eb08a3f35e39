"""A pool's live pitch contours (vbx_pool_path_bind, vbx_pool_path_slot_rows, vbx_pool_path_outputs) at every layer above the C ABI,
checked without a GPU: the header, the Python mirror, the built library's exports, the host arithmetic, the C++ mirror, the Rust
layers, the plain-C example, where the kernel lives and what it costs."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vbx_pool_path_slot_rows", "vbx_pool_path_bind")


def _header():
    h = open(os.path.join(ROOT, "include", "voxbox_hip.h")).read()
    return h, " ".join(re.sub(r"/\*.*?\*/", "", h, flags=re.S).split())


def test_header_declares_the_binding():
    h, flat = _header()
    assert ("typedef struct { vbx_pitch *out_path; int32_t *out_index; uint8_t *out_forced; vbx_path_commit *d_commit; } "
            "vbx_pool_path_outputs;") in flat
    assert "size_t vbx_pool_path_slot_rows(size_t max_pending, size_t max_block_sample_frames, size_t stride);" in flat
    assert ("int vbx_pool_path_bind(vbx_pool *pool, double peak_ref, size_t max_pending, const vbx_pool_path_outputs *h_out, size_t path_ld, "
            "size_t slot_rows);") in flat
    assert re.search(r"#define VBX_ABI_VERSION 5\b", h)                      # the change only adds
    a, b = h.index("a pool of live streams (ABI 5, added)"), h.index("multi-GPU: frame-range sharding")
    block = h[a:b]
    for n in NEW + ("vbx_pool_path_outputs", "ABI 5, added; DESIGN.md section 5m", "pitch_path_online_pool", "ONE more launch", "DEFERRED",
                    "EMPTY tick", "slot_rows", "max_pending + ceil(max_block_sample_frames / stride)", "bit for bit", "are not touched",
                    "`first` of the first, n and n_forced summed, `pending` of the", "vbx_path_stream_reset", "2^24", "without h_track"):
        assert n in block, n
    assert "is NOT offered for pool slots" not in h                          # the limit this lifts
    assert block.index("void vbx_pool_close(vbx_pool *pool);") < block.index("} vbx_pool_path_outputs;")
    # the pool's tick and its table are what they were
    assert ("int vbx_pool_mark_utterance(vbx_pool *pool, int32_t stream);" in flat and "int vbx_pool_reset_stream(vbx_pool *pool, int32_t stream);" in flat)
    kh = open(os.path.join(ROOT, "vox_box.rs_amd", "csrc", "vbx_kernels.hpp")).read()
    assert "uint64_t pad;                                         // (144 bytes" in kh


def test_python_mirror_and_exports(pkg):
    assert set(NEW) <= set(pkg.exported_symbols())
    lib = pkg.load_library()
    for n in NEW:
        assert hasattr(lib, n), n
    assert lib.vbx_abi_version() == 5
    vp, sz = C.c_void_p, C.c_size_t
    assert [f[0] for f in pkg.PoolPathOutputs._fields_] == ["out_path", "out_index", "out_forced", "d_commit"] and C.sizeof(pkg.PoolPathOutputs) == 32
    assert lib.vbx_pool_path_slot_rows.argtypes == [sz] * 3 and lib.vbx_pool_path_slot_rows.restype is sz
    assert lib.vbx_pool_path_bind.argtypes == [vp, C.c_double, sz, C.POINTER(pkg.PoolPathOutputs), sz, sz]
    assert list(inspect.signature(pkg.pool_path_slot_rows).parameters) == ["max_pending", "max_block", "stride"]
    assert list(inspect.signature(pkg.Pool.bind_path).parameters) == ["self", "out_path", "commit", "peak_ref", "max_pending", "path_ld", "slot_rows",
                                                                      "out_index", "out_forced"]


def test_null_arguments_are_refused_without_a_gpu(pkg):
    lib = pkg.load_library()
    po = pkg.PoolPathOutputs()
    assert lib.vbx_pool_path_bind(None, 1.0, 64, None, 2, 66) == -1
    assert b"null pool" in lib.vbx_last_error(None)
    assert lib.vbx_pool_path_bind(None, 1.0, 64, C.byref(po), 2, 66) == -1


def test_slot_rows_is_the_formula(pkg):
    lib = pkg.load_library()
    for mp, mb, st in [(64, 160, 80), (64, 161, 80), (1, 1, 1), (3, 400, 160), (64, 100, 480), (512, 51440, 160), (1 << 24, 1 << 20, 7), (64, 0, 80)]:
        want = mp + -(-mb // st)
        assert lib.vbx_pool_path_slot_rows(mp, mb, st) == want == pkg.pool_path_slot_rows(mp, mb, st), (mp, mb, st)
    assert pkg.pool_path_slot_rows(64, 100, 480) == 65                       # stride > max_block: still one frame may complete
    assert lib.vbx_pool_path_slot_rows(64, 160, 0) == 0                      # no stride: no answer


def test_cpp_mirror_compiles_with_the_binding():
    hdr = os.path.join(ROOT, "vox_box.rs_amd", "host")
    src = ('#include "voxbox.hpp"\n'
           'int main(){ voxbox::Context c(0); voxbox::AnalysisParams p = voxbox::analysis_params(8000.0);\n'
           '  vbx_pitch_track_params t{}; t.kmax = 4;\n'
           '  voxbox::pool q(c, voxbox::host_audio(VBX_SAMPLE_ULAW, 1, 0), 200, 80, p, nullptr, &t, 8, 160, 1280);\n'
           '  const size_t rows = voxbox::pool_path_slot_rows(64, 160, 80);\n'
           '  voxbox::PoolPathOutputs o{}; static_assert(sizeof(o) == 32, "four device pointers");\n'
           '  q.bind_path(1.0, 64, o, 2, rows);\n'
           '  q.mark_utterance(0); voxbox::PoolEntry e[1] = {};\n'
           '  return (int)(rows + q.push(e, 0, nullptr, 4)); }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", hdr, "-x", "c++", "-"],
                       input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(hdr, "voxbox.hpp")).read()
    for n in NEW:
        assert n + "(" in text, n


def test_rust_layers_name_the_entry_points():
    gpu = open(os.path.join(ROOT, "bindings", "rust", "src", "gpu.rs")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for n in NEW:
        assert "pub fn " + n + "(" in ffi, n
        assert "ffi::" + n in gpu, n
    assert "pub struct VbxPoolPathOutputs {" in ffi and "pub d_commit: *mut VbxPathCommit," in ffi
    m = re.search(r"pub fn vbx_pool_path_bind\((.*?)\) -> c_int;", ffi, re.S)
    for part in ("pool: *mut VbxPool", "peak_ref: f64", "max_pending: usize", "h_out: *const VbxPoolPathOutputs", "path_ld: usize", "slot_rows: usize"):
        assert part in m.group(1), part
    assert "pub fn bind_path(&self, peak_ref: f64, max_pending: usize, slot_rows: usize, rows: &PathRows<'g>)" in gpu
    assert "pub fn path_slot_rows(max_pending: usize, max_block: usize, stride: usize) -> usize" in gpu


def test_the_c_example_compiles_and_links(pkg, tmp_path):
    """examples/call_pool_pitch.c: plain C against the header, every entry point it uses resolves in the library"""
    lib = os.path.join(ROOT, "vox_box.rs_amd", "lib")
    path = os.path.join(ROOT, "examples", "call_pool_pitch.c")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), path,
                        "-L", lib, "-lvoxbox_hip", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib", "-lm", "-o", str(tmp_path / "call_pool_pitch")],
                       text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    src = open(path).read()
    for n in ("vbx_pool_open(", "vbx_pool_path_slot_rows(", "vbx_pool_path_bind(", "vbx_pool_mark_utterance(", "vbx_pool_push(pool, entries, n,",
              "VBX_SAMPLE_ULAW", "EMPTY"):
        assert n in src, n


def test_the_kernel_lives_in_its_own_unit():
    read = lambda f: open(os.path.join(ROOT, "vox_box.rs_amd", "csrc", f)).read()
    k = read("k_pitch_path_pool.hip")
    assert "pp_online_pool_kernel" in k and "void launch_pitch_path_online_pool(" in k and "__launch_bounds__(64)" in k
    for call in ("pp_fetch(", "pp_decode<G>(", "pp_step<G>(", "pp_leader<G>("):
        assert call in k, call
    assert "#pragma clang fp contract(off)" in k and '#include "vbx_pitch_path_step.hpp"' in k and "fma(" not in k
    assert "ALL THREE" in k and "k_pitch_path_channels.hip" in k                 # where a change to the scan's body has to be made
    for f in ("k_pitch_path.hip", "k_pitch_path_channels.hip", "vbx_pitch_path_step.hpp", "k_pool.hip", "k_tracker.hip"):
        assert "pp_online_pool" not in read(f), f
    kh = read("vbx_kernels.hpp")
    assert "void launch_pitch_path_online_pool(" in kh and "struct pp_pool_row_t {" in kh and "struct pp_online_pool_t {" in kh
    assert "size_t vbx_pool_path_slot_rows(" in read("vbx_host.cpp")
    api = read("vbx_api_pool.hip")
    assert '"pitch_path_online_pool"' in api and "int vbx_pool_path_bind(" in api and "launch_pitch_path_online_pool(" in api
    assert api.count("q->ring.upload(") == 2 and api.count("launch_pitch_path_online_pool(") == 1    # one upload and one path launch per kind of tick


def test_the_new_kernel_has_no_scratch_and_no_spills():
    """the committed record is what tools/resource_usage.sh prints for the unit as it stands"""
    usage = open(os.path.join(ROOT, "profiles", "pool_path", "resource_usage.txt")).read()
    r = subprocess.run([os.path.join(ROOT, "tools", "resource_usage.sh"), os.path.join("vox_box.rs_amd", "csrc", "k_pitch_path_pool.hip")],
                       cwd=ROOT, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    built = [ln for ln in r.stdout.splitlines() if "pp_online_pool_kernel" in ln]
    rows = [ln for ln in usage.splitlines() if "pp_online_pool_kernel" in ln]
    assert len(rows) == 5 and [ln.split() for ln in rows] == [ln.split() for ln in built]
    assert len(built) == len([ln for ln in r.stdout.splitlines() if "kernel" in ln.lower() and ln.startswith("_Z")])   # the unit's only kernels
    for g, ln in zip((4, 8, 16, 32, 64), rows):
        assert "pp_online_pool_kernelILi%dE" % g in ln, ln
        assert re.search(r"scratch\s+0\b", ln) and re.search(r"vspill\s+0\b", ln) and re.search(r"sspill\s+0\b", ln), ln
