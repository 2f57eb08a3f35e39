"""Layout as a tested dimension: every entry point of include/voxbox_hip.h that computes on device pointers is run in a canonical
layout (dense batch, every address 0 mod 16) and then on THE SAME FRAMES with its buffers moved, all inside fenced arenas
(tests/layout_arena.py).  Not run here: the memory helpers (vbx_malloc / vbx_memcpy_* / vbx_memset) and the two RCCL calls, which need
a communicator (vbx_gather_records_f64, a copy; vbx_comm_stitch_tracks_f64, whose kernel is vbx_track_stitch_f64's, run below).

  A  x at 8 mod 16 (float: 4 and 12; PCM: 2 mod 4)        E  stride > frame_len, odd, NaN (PCM: -32768) in the gaps
  B  window at 8 mod 16 (float: 4)                        F  A + B + C + D at once
  C  every output at its smallest legal alignment          G  leading dimensions with padding (record_ld, r_stride)
  D  odd stride < frame_len (frames alternate between      H  each optional output in turn NULL
     0 and 8 mod 16), and stride = 1

and, crossed with the canonical layout and F, n_frames in {1, 2, fpb - 1, fpb, fpb + 1, 211} (fpb: the kernel's frames per block,
listed beside each shape below; each size has a canonical call of its own).  Every layout case has 37 frames (stride 1: 77).  The
profile names "mfcc", "pitch" and "formant_resonances" each cover several kernels: which one ran is asserted from the library's
probes (vbx_internal_last_mfcc_form, vbx_internal_last_pitch_form, the one-pass Burg's and the pair root finder's hand-over counts),
and the vector two-stage MFCC kernel, which no default dispatch reaches at these settings, runs in a context created under
VBX_MFCC_DFT2=1.  Asserted for every case: fences, padding and inputs
intact; every output bit for bit the canonical call's; no NaN the canonical call's output does not have; no output element left
unwritten; and once per (entry point, shape) the canonical call against the CPU oracle with the project's tolerances (rel_close 1e-6,
Hz 1e-4, counts and statuses exact), that at least one frame has a non-trivial result, and from vbx_profile_names that the kernel the
shape was chosen for ran.

Kernels with an alignment branch, the predicate (quoted from the source) and the layouts that take the element-wise side.  The
side of every case is computed from its addresses and stride with these predicates (BRANCHES below) and test_zz_report asserts that
both sides were reached:

  kernel (profile name)              predicate for the 16-byte path                                         shapes       fallback in
  autocorr_fewlags / autocorr_lpc    k_lpc.hip: full && (x & 15) == 0 && (stride & 1) == 0                  512, 1024    A D E F (100, 1200: never full)
  burg (direct)                      k_burg.hip: ((xf | window) & 15) == 0, per frame                      512x9, 1024x12   A B D E F
  burg_lags (one pass)               vbx_burg_fast.hpp: whole && (x & 15) == 0 && (stride & 1) == 0         512x12, 1200x16, 2048x8    A D E F
                                     (segmented, n > 1280: ((xf | window) & 15) == 0 per frame)
  pitch / autocorr_fft / mfcc, 1200  k_spectral.hip: ((xf | window) & 15) == 0, per frame                   1200, 1103   A B D E F
  the same, power-of-two kernels     vbx_spectral_pow2.hpp: ((xf | window) & 15) == 0, per frame            1024, 2048, 4096   A B D E F
  autocorr_fft output rows           k_spectral.hip / vbx_spectral_pow2.hpp: (out_r & 15) == 0 && (n_lags & 1) == 0     C F, odd n_lags
  fused loop on PCM, 1200            k_spectral.hip: (x16 & 3) == 0 per frame; window: (window & 15) == 0   1200         A D F
  pcm16 (vbx_pcm16_to_f64)           k_front.hip: ((pcm & 3) | (out & 15)) == 0                                          A C F

The alignment audit that precedes this file (every cast of a caller's pointer to a wider type): the {double, double} stores and loads
on out_cand (vbx_pitch_f64: lane list, LDS list, k_long.hip), on `out` of vbx_estimate_formants_f64, out_formants of
vbx_find_formants_f64 and `formants` of vbx_track_stitch_f64 promise the compiler 8 bytes now (load_pair8 / store_pair8,
vbx_device.hpp), the whole-Vec list is parked in the output row only where the rows are 16-byte aligned, and the records of
vbx_analyze_frames_* stay REJECTED at 8 mod 16 (asserted below).  cand of vbx_pitch_path_f64, the polynomial arrays and the rows of
vbx_to_resonance_c64 go through the 8-byte structs res_t / pitch_t / cplx_t: clear."""
import ctypes as C
import importlib
import json
import os
import time

import numpy as np
import pytest

import layout_arena as la
import parity_asserts as pa
from conftest import rel_close

pytestmark = pytest.mark.gpu

SR = 48000.0
F_MAIN = 37                      # frames per layout case (batch sizes below add their own)
F_PRIME = 211
REPORT = {"cases": 0, "kernels_seen": {}, "branch_sides": {}, "probes": {}, "wall_seconds": 0.0}
_T0 = [None]
f64, f32, i32, i16, c128 = np.float64, np.float32, np.int32, np.int16, np.complex128


# ---- frames ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def speech(vb):
    """10 s of the synthetic speech the other GPU tests use (voiced glide + an unvoiced second)."""
    d = vb.synth_speech(10 * 48000, sample_offset=2 * 48000)
    a = d.numpy()
    d.free()
    return a


@pytest.fixture(scope="module", autouse=True)
def profiled(vb):
    if _T0[0] is None:
        _T0[0] = time.time()
    vb.profile(True)
    yield
    vb.profile(False)


class FrameSet:
    """Dense frames [F, N] and, for a view with stride < N, the 1-D signal they are windows of."""

    def __init__(self, speech, N, F, mode, dtype=f64):
        self.N, self.F, self.mode = N, F, mode
        sig = speech
        if dtype == i16:
            sig = np.round(speech * (0.9 * 32767.0)).astype(i16)
        elif dtype == f32:
            sig = speech.astype(f32)
        if mode == "hop":                                    # ordinary frames + two rectangular ones with x[0] != 0 (the fold seed)
            hop = min(480, (sig.size - N) // max(F - 1, 1)) if F > 1 else 480
            fr = la.windows(sig[7001:], N, hop, F).copy()
            rng = np.random.default_rng(N * 7 + F)
            for t in {min(1, F - 1), F // 2}:
                r = rng.uniform(-0.8, 0.8, N)
                fr[t] = np.round(r * 32767.0).astype(i16) if dtype == i16 else r.astype(dtype)
            self.frames, self.signal, self.stride = fr, None, N
        else:
            s = 1 if mode == "one" else (441 if N > 441 else (N // 2) | 1)
            assert s % 2 == 1 and s < N
            self.signal = np.ascontiguousarray(sig[12345:12345 + (F - 1) * s + N])
            self.frames, self.stride = la.windows(self.signal, N, s, F), s


_FS = {}


def frameset(speech, N, F, mode, dtype=f64):
    key = (N, F, mode, np.dtype(dtype).str)
    if key not in _FS:
        if len(_FS) > 24:
            _FS.clear()
        _FS[key] = FrameSet(speech, N, F, mode, dtype)
    return _FS[key]


def gap_stride(N):
    return N + (5 if N % 2 == 0 else 4)                      # odd, > N


# ---- the alignment branches: which side a case is on (predicates quoted from the sources) ------------------------------------

def _per_frame(x, es, stride, F, pred):
    sides = {pred(x + t * stride * es) for t in range(F)}
    return "vector" if sides == {True} else "fallback" if sides == {False} else "both"


BRANCHES = {
    # vec16 = full && sizeof(T) == 8 && EPL % 2 == 0 && (((uintptr_t)x) & 15) == 0 && (stride & 1) == 0      (k_lpc.hip)
    "k_lpc.hip:vec16": lambda c: None if c["N"] not in (512, 1024) or c["es"] != 8 else
        ("vector" if c["x"] % 16 == 0 and c["stride"] % 2 == 0 else "fallback"),
    # vec = have && (lig + 1) * EPL <= n && ((((uintptr_t)xf) | ((uintptr_t)window)) & 15) == 0                 (k_burg.hip)
    "k_burg.hip:vec": lambda c: _per_frame(c["x"], 8, c["stride"], c["F"], lambda xf: (xf | (c["w"] or 0)) % 16 == 0),
    # wide = whole && ((((uintptr_t)x) & 15) == 0 && (stride & 1) == 0)                                       (vbx_burg_fast.hpp)
    "vbx_burg_fast.hpp:wide": lambda c: None if c["N"] > 1280 else ("vector" if c["x"] % 16 == 0 and c["stride"] % 2 == 0 else "fallback"),
    # al = ((((uintptr_t)xf) | ((uintptr_t)window)) & 15) == 0 && base + EPL <= n     (vbx_burg_fast.hpp, segmented lag kernel)
    "vbx_burg_fast.hpp:al": lambda c: None if c["N"] <= 1280 else
        _per_frame(c["x"], 8, c["stride"], c["F"], lambda xf: (xf | (c["w"] or 0)) % 16 == 0),
    # al = ((((uintptr_t)xf) | ((uintptr_t)a.window)) & 15) == 0                        (k_spectral.hip, vbx_spectral_pow2.hpp)
    "k_spectral.hip:al": lambda c: _per_frame(c["x"], 8, c["stride"], c["F"], lambda xf: (xf | (c["w"] or 0)) % 16 == 0),
    "vbx_spectral_pow2.hpp:al": lambda c: _per_frame(c["x"], 8, c["stride"], c["F"], lambda xf: (xf | (c["w"] or 0)) % 16 == 0),
    # al = ((((uintptr_t)a.out_r) & 15) == 0) && (a.n_lags & 1) == 0                   (k_spectral.hip, vbx_spectral_pow2.hpp)
    "spectral:out_r al": lambda c: "vector" if c["out"] % 16 == 0 and c["lags"] % 2 == 0 else "fallback",
    # (((uintptr_t)x16) & 3) == 0, per frame                                                          (k_spectral.hip, PCM)
    "k_spectral.hip:x16": lambda c: _per_frame(c["x"], 2, c["stride"], c["F"], lambda xf: xf % 4 == 0),
    # aligned = ((pcm & 3) | (out & 15)) == 0                                                                (k_front.hip)
    "k_front.hip:aligned": lambda c: "vector" if c["x"] % 4 == 0 and c["out"] % 16 == 0 else "fallback",
}


def note_branch(names, **c):
    for name in names:
        side = BRANCHES[name](c)
        if side is not None:
            got = REPORT["branch_sides"].setdefault(name, {})
            for s in (("vector", "fallback") if side == "both" else (side,)):
                got[s] = got.get(s, 0) + 1


# ---- running one call inside an arena ------------------------------------------------------------------------------------------

def arena_call(vb, label, inputs, outputs, call):
    """inputs: name -> (array, residue[, inout]); outputs: name -> (dtype, rows, cols, ld, residue).  Returns finish()."""
    a = la.Arena(la.DeviceBackend(vb), label)
    for name, spec in inputs.items():
        a.input(name, spec[0], residue=spec[1], inout=len(spec) > 2 and spec[2])
    for name, (dt, rows, cols, ld, res) in outputs.items():
        a.output(name, dt, rows, cols, ld=ld, residue=res)
    a.place()
    addr = {n: a[n] for n in a.bufs}
    print("layout case:", label, flush=True)                 # the last line printed names the case a fault belongs to
    REPORT["cases"] += 1
    try:
        rc = call(addr)
        vb._check(rc)
    except Exception:
        a.backend.free()
        raise
    return a.finish(), addr


def min_res(dt):
    return 8 if np.dtype(dt).itemsize >= 8 else 4


def in_res(dt, which):
    """Layout A / B residue of an input of this type: doubles 8; floats 4 (and 12 as "A12"); PCM 2."""
    return {8: 8, 4: which if which in (4, 12) else 4, 2: 2}[min(np.dtype(dt).itemsize, 8)]


def same(label, got, want, skip=()):
    for name in want:
        if name in skip:
            assert name not in got
            continue
        la.assert_same_bits(label, name, got[name], want[name])
        la.assert_no_new_nan(label, name, got[name], want[name])
        la.assert_written(label, name, got[name])


def kernels_ran(vb, label, wanted):
    names = set(vb.profile_report())
    REPORT["kernels_seen"][label] = sorted(names)
    assert set(wanted) <= names, (label, "expected kernels", sorted(wanted), "profiled", sorted(names))


class Op:
    """A frame-batch entry point at one shape."""

    def __init__(self, id, call, N, outs, kernels, fpb, oracle, p=None, window=False, dtype=f64, optional=(), branches=(),
                 ld_pad=None, policy=None, env=None, keep_aligned=(), form=None, ctx_env=None):
        self.id, self.call, self.N, self.outs, self.kernels, self.fpb = id, call, N, outs, set(kernels), fpb
        self.oracle, self.p, self.window, self.dtype, self.optional = oracle, p or {}, window, np.dtype(dtype), optional
        self.branches, self.ld_pad, self.policy, self.env = branches, ld_pad, policy, env
        self.form = form                                     # what vbx_internal_last_mfcc_form / _pitch_form must say after the canonical call
        self.ctx_env = ctx_env                               # switches the library reads when a context is created: a context of its own
        self.keep_aligned = keep_aligned                     # outputs whose misalignment the entry point REJECTS (asserted on its own)

    def __repr__(self):
        return self.id


def run_op(vb, pkg, op, fs, lay, label):
    F, N, dt = fs.F, fs.N, op.dtype
    mode = lay.get("stride", "dense")
    if mode == "dense":
        stride, xbuf = N, fs.frames.reshape(-1)
    elif mode == "gap":
        stride = gap_stride(N)
        xbuf = la.gapped_view(fs.frames, stride, la.PCM_FENCE if dt == i16 else np.nan)
    else:
        stride, xbuf = fs.stride, fs.signal
    inputs = {"x": (xbuf, lay.get("x_res", 0))}
    if op.window:
        w = pkg.window_table(pkg.WINDOW_HANNING, N)
        inputs["window"] = (w.astype(f32) if dt == f32 else w, lay.get("w_res", 0))
    outputs, null = {}, set(lay.get("null", ()))
    for spec in op.outs(F, N, op.p):
        name, odt, rows, cols = spec if len(spec) == 4 else (spec[0], spec[1], F, spec[2])
        if name in null:
            continue
        fixed = name in op.keep_aligned
        outputs[name] = (odt, rows, cols, lay.get("ld", {}).get(name), min_res(odt) if lay.get("out_min") and not fixed else 0)
    ld = {n: (s[3] if s[3] is not None else s[2]) for n, s in outputs.items()}
    vb.profile_reset()
    got, addr = arena_call(vb, label, inputs, outputs,
                           lambda a: op.call(vb, F, N, stride, a["x"], a.get("window"), a, op.p, ld))
    first_out = op.outs(F, N, op.p)[0][0]
    note_branch(op.branches, x=addr["x"], w=addr.get("window"), stride=stride, F=F, N=N, es=dt.itemsize,
                out=addr.get(first_out, 0), lags=op.p.get("lags", 0))
    return got


def layouts_of(op):
    d = op.dtype
    lays = [("A", dict(x_res=in_res(d, 4)))]
    if d == f32:
        lays.append(("A12", dict(x_res=12)))
    if op.window:
        lays.append(("B", dict(w_res=in_res(d, 4))))
    lays += [("C", dict(out_min=True)), ("E", dict(stride="gap"))]
    for name in op.optional:
        lays.append(("H-" + name, dict(null=(name,))))
    if op.ld_pad:
        for k, ld in enumerate(op.ld_pad):
            lays.append((f"G{k}", dict(ld=ld)))
    return lays


LAY_F = dict(x_res=8, w_res=8, out_min=True, stride="view")


def lay_f(op):
    return dict(LAY_F, x_res=in_res(op.dtype, 4), w_res=in_res(op.dtype, 4))


def check_op(vb, pkg, oracle, speech, op, monkeypatch):
    if op.ctx_env:
        for k, v in op.ctx_env.items():
            monkeypatch.setenv(k, v)
        own = pkg.VoxBox(0)
        for k in op.ctx_env:
            monkeypatch.delenv(k)
        own.profile(True)
        try:
            _check_op(own, pkg, oracle, speech, op, monkeypatch)
        finally:
            own.close()
    else:
        _check_op(vb, pkg, oracle, speech, op, monkeypatch)
    REPORT["ops_run"] = REPORT.get("ops_run", 0) + 1


def _check_op(vb, pkg, oracle, speech, op, monkeypatch):
    if op.env:
        for k, v in op.env.items():
            monkeypatch.setenv(k, v)
    old_policy = vb.lpc_policy
    if op.policy is not None:
        vb.lpc_policy = op.policy
    try:
        N = op.N
        F = F_MAIN
        # -- dense frames: the canonical call, the oracle, the kernel, then layouts A B C E G H
        fs = frameset(speech, N, F, "hop", op.dtype)
        canon = run_op(vb, pkg, op, fs, {}, f"{op.id} canonical F={F}")
        kernels_ran(vb, op.id, op.kernels)
        # several kernels share the profile names "mfcc", "pitch" and "formant_resonances": the library's probes say which one ran
        if op.id.startswith("mfcc"):
            REPORT["probes"][op.id] = {"mfcc_form": int(vb.L.vbx_internal_last_mfcc_form(vb.ctx))}
            assert REPORT["probes"][op.id]["mfcc_form"] == op.form, (op.id, REPORT["probes"][op.id], op.form)
        elif op.form is not None:                            # the pitch shapes (the reference-faithful f32 kernel has a name of its own)
            REPORT["probes"][op.id] = {"pitch_form": int(vb.L.vbx_internal_last_pitch_form(vb.ctx)),
                                       "spectral_split": int(vb.L.vbx_internal_last_spectral_split(vb.ctx))}
            assert REPORT["probes"][op.id]["pitch_form"] == op.form, (op.id, REPORT["probes"][op.id], op.form)
            if op.id == "pitch-4096-k4":                     # the 4096-point plan's two-kernel form
                assert REPORT["probes"][op.id]["spectral_split"] == 1, REPORT["probes"][op.id]
        elif op.id.startswith("find_formants"):              # -1: the call did not take the one-pass Burg / the conjugate-pair roots
            REPORT["probes"][op.id] = {"burg_direct_count": vb.last_burg_direct_count(), "roots_direct_count": vb.last_roots_direct_count()}
            fast = op.p["p"] == 12
            assert (REPORT["probes"][op.id]["burg_direct_count"] >= 0) == fast and (REPORT["probes"][op.id]["roots_direct_count"] >= 0) == fast, \
                (op.id, REPORT["probes"][op.id])
        for name in canon:
            la.assert_written(op.id, name, canon[name])
        op.oracle(oracle, pkg, op, fs.frames, canon, vb)
        for tag, lay in layouts_of(op):
            got = run_op(vb, pkg, op, fs, lay, f"{op.id} {tag} F={F}")
            same(f"{op.id} layout {tag}", got, canon, skip=lay.get("null", ()))
        # -- the odd-stride view and stride 1: their own frames, their own canonical calls; D, F
        fsd = frameset(speech, N, F, "odd", op.dtype)
        canon_d = run_op(vb, pkg, op, fsd, {}, f"{op.id} canonical(odd-stride frames) F={F}")
        same(f"{op.id} layout D", run_op(vb, pkg, op, fsd, dict(stride="view"), f"{op.id} D stride={fsd.stride} F={F}"), canon_d)
        same(f"{op.id} layout F", run_op(vb, pkg, op, fsd, lay_f(op), f"{op.id} F stride={fsd.stride} F={F}"), canon_d)
        F1 = 2 * F_MAIN + 3
        fs1 = frameset(speech, N, F1, "one", op.dtype)
        canon_1 = run_op(vb, pkg, op, fs1, {}, f"{op.id} canonical(stride-1 frames) F={F1}")
        same(f"{op.id} layout D1", run_op(vb, pkg, op, fs1, dict(stride="view"), f"{op.id} D stride=1 F={F1}"), canon_1)
        # -- batch sizes, canonical and F
        sizes = sorted({1, 2, max(op.fpb - 1, 1), op.fpb, op.fpb + 1, F_PRIME})
        for Fb in sizes:
            fsb = frameset(speech, N, Fb, "odd", op.dtype)
            cb = run_op(vb, pkg, op, fsb, {}, f"{op.id} canonical F={Fb}")
            for name in cb:
                la.assert_written(f"{op.id} F={Fb}", name, cb[name])
            same(f"{op.id} layout F, n_frames={Fb}", run_op(vb, pkg, op, fsb, lay_f(op), f"{op.id} F F={Fb}"), cb)
    finally:
        if op.policy is not None:
            vb.lpc_policy = old_policy


# ---- the entry points: calls ---------------------------------------------------------------------------------------------------

def c_autocorr(vb, F, N, S, x, w, o, p, ld):
    return vb.L.vbx_autocorrelate_f64(vb.ctx, x, F, N, S, w, p["lags"], o["r"])


def c_autocorr_lpc(vb, F, N, S, x, w, o, p, ld):
    return vb.L.vbx_autocorr_lpc_f64(vb.ctx, x, F, N, S, w, p["p"], p.get("norm", 0), o.get("r"), o.get("lpc"))


def c_burg(vb, F, N, S, x, w, o, p, ld):
    return vb.L.vbx_lpc_burg_f64(vb.ctx, x, F, N, S, w, p["p"], o["coeffs"], o.get("status"))


def c_pitch(vb, F, N, S, x, w, o, p, ld):
    return vb.L.vbx_pitch_f64(vb.ctx, x, F, N, S, w, SR, 0.2, 75.0, 600.0, p["kmax"], o["cand"], o.get("count"), o.get("status"))


def c_mfcc(vb, F, N, S, x, w, o, p, ld):
    return vb.L.vbx_mfcc_f64(vb.ctx, x, F, N, S, w, 13, 100.0, p.get("hi", 8000.0), SR, o["mfcc"], o.get("status"))


EST0 = np.array([[320.0, 1.0], [1440.0, 1.0], [2760.0, 1.0], [3200.0, 1.0]])


def _segs(F):
    return np.array(sorted({0, F // 3, (2 * F) // 3} if F >= 6 else {0}), dtype=np.int64)


def c_formants(vb, F, N, S, x, w, o, p, ld):
    seg = _segs(F)
    return vb.L.vbx_find_formants_f64(vb.ctx, x, F, N, S, SR, p["p"], seg.ctypes.data, seg.size, EST0.ctypes.data, 4,
                                      o["formants"], o.get("res"), o.get("res_count"), o.get("coeffs"), o.get("status"))


def c_rms(vb, F, N, S, x, w, o, p, ld):
    return vb.L.vbx_rms_f64(vb.ctx, x, F, N, S, w, o["rms"])


def c_peak(vb, F, N, S, x, w, o, p, ld):
    return vb.L.vbx_frame_peak_f64(vb.ctx, x, F, N, S, o["peak"])


def c_preemph(vb, F, N, S, x, w, o, p, ld):
    return vb.L.vbx_preemphasis_f64(vb.ctx, x, F, N, S, 0.1, o["out"])


def c_resample(vb, F, N, S, x, w, o, p, ld):
    return vb.L.vbx_resample_linear_f64(vb.ctx, x, F, N, S, p["ratio"], o["out"])


def _aparams(pkg, p):
    return pkg.AnalysisParams.make(SR, lpc_order=p.get("lpc", 12), formant_order=p.get("fo", 12), est_init=EST0,
                                   mfcc=p.get("mfcc", (13, 100.0, 8000.0)))


def c_analyze(vb, F, N, S, x, w, o, p, ld):
    seg = _segs(F)
    assert p["rec"] == vb.L.vbx_record_doubles(C.byref(p["params"]))
    fn = vb.L.vbx_analyze_frames_pcm16 if p.get("pcm") else vb.L.vbx_analyze_frames_f64
    return fn(vb.ctx, x, F, N, S, C.byref(p["params"]), seg.ctypes.data, seg.size, o["records"], ld["records"], o.get("status3"))


def c_autocorr_f32(vb, F, N, S, x, w, o, p, ld):
    fn = vb.L.vbx_autocorrelate_f32_wide if p.get("wide") else vb.L.vbx_autocorrelate_f32
    return fn(vb.ctx, x, F, N, S, w, p["lags"], o["r"])


def c_autocorr_lpc_f32(vb, F, N, S, x, w, o, p, ld):
    fn = vb.L.vbx_autocorr_lpc_f32_wide if p.get("wide") else vb.L.vbx_autocorr_lpc_f32
    return fn(vb.ctx, x, F, N, S, w, p["p"], 0, o.get("r"), o.get("lpc"))


def c_burg_f32(vb, F, N, S, x, w, o, p, ld):
    fn = vb.L.vbx_lpc_burg_f32_wide if p.get("wide") else vb.L.vbx_lpc_burg_f32
    return fn(vb.ctx, x, F, N, S, w, p["p"], o["coeffs"], o.get("status"))


def c_mfcc_f32(vb, F, N, S, x, w, o, p, ld):
    return vb.L.vbx_mfcc_f32(vb.ctx, x, F, N, S, w, 13, 100.0, 8000.0, SR, o["mfcc"], o.get("status"))


def c_pitch_f32(vb, F, N, S, x, w, o, p, ld):
    fn = vb.L.vbx_pitch_f32_wide if p.get("wide") else vb.L.vbx_pitch_f32
    return fn(vb.ctx, x, F, N, S, w, SR, 0.2, 75.0, 600.0, p["kmax"], o["cand"], o.get("count"), o.get("status"))


# ---- the entry points: canonical call against the oracle (the assertions of tests/test_gpu_parity.py / test_gpu_f32.py) ---------

def _win(oracle, op, frames):
    return frames.astype(f64) * oracle.window("hanning", op.N) if op.window else frames.astype(f64)


def _some(mask, what):
    assert np.any(mask), "nothing non-trivial in this case: " + what


def o_autocorr(oracle, pkg, op, frames, got, vb):
    pa.autocorrelate_rows(oracle, _win(oracle, op, frames), op.p["lags"], got["r"], op.id)
    _some(got["r"][:, 0] != 0.0, "r[0]")


def o_autocorr_lpc(oracle, pkg, op, frames, got, vb):
    xw, p, norm = _win(oracle, op, frames), op.p["p"], op.p.get("norm", 0)
    if op.policy == pkg.LPC_POLICY_PLAIN:
        # "the rows of rounds 1-5": the assertion of tests/test_gpu_lpc_exact.py -- bit for bit the EXACT policy's rows except the
        # rows its probe lists and redoes; and those EXACT rows are held to the oracle like any other
        vb.lpc_policy = pkg.LPC_POLICY_EXACT
        try:
            r_e, a_e = vb.autocorr_lpc(xw, p, normalize=bool(norm))
            listed = vb.last_lpc_exact_count()
        finally:
            vb.lpc_policy = pkg.LPC_POLICY_PLAIN
        assert np.array_equal(got["r"].view(np.int64), r_e.view(np.int64))
        differs = ~np.all(got["lpc"].view(np.int64) == a_e.view(np.int64), axis=1)
        assert listed >= 0 and int(differs.sum()) <= listed, (op.id, int(differs.sum()), listed)
        pa.autocorr_lpc_rows(oracle, xw, p, norm, r_e, a_e, op.id)
    else:
        pa.autocorr_lpc_rows(oracle, xw, p, norm, got["r"], got["lpc"], op.id)
    _some(np.abs(got["lpc"][:, 1]) > 0.0, "a1")


def o_burg(oracle, pkg, op, frames, got, vb):
    pa.burg_rows(oracle, _win(oracle, op, frames), op.p["p"], got["coeffs"], got["status"][:, 0], op.id)
    _some(got["status"][:, 0] == 0, "status 0")


def o_pitch(oracle, pkg, op, frames, got, vb):
    """The rule of _check_pitch (tests/test_gpu_parity.py): status and count exact, entries past the count zero, the top candidate
    by classify_top (tests/analyze_reference.py), a whole list as a set ordered by frequency within 1e-4 relative in Hz."""
    from analyze_reference import classify_top
    xw, kmax, voiced = _win(oracle, op, frames), op.p["kmax"], 0
    for f in range(xw.shape[0]):
        es, ec, en = oracle.pitch(xw[f], SR, 0.2, 75.0, 600.0)
        g = got["cand"][f].reshape(kmax, 2)
        assert got["status"][f, 0] == es and got["count"][f, 0] == (en if es == 0 else 0), (op.id, f, es, en, got["count"][f, 0])
        k = min(kmax, en)
        assert np.all(g[k:] == 0.0), (op.id, f, "entries past count are zero")
        if es != 0:
            assert np.all(g == 0.0)
            continue
        assert classify_top(g[0], ec, en) in ("ok", "swap"), (op.id, f, g[0], ec[:2])
        voiced += int(g[0, 0] > 0.0)
        if kmax >= en:
            a, b = g[:k][np.argsort(g[:k, 0], kind="stable")], ec[:k][np.argsort(ec[:k, 0], kind="stable")]
            assert np.all(np.abs(a[:, 0] - b[:, 0]) <= 1e-4 * np.abs(b[:, 0]) + 1e-12), (op.id, f, "frequencies")
    assert voiced > 0, "no voiced frame in this case"


def o_mfcc(oracle, pkg, op, frames, got, vb):
    pa.mfcc_rows(oracle, _win(oracle, op, frames), 13, 100.0, op.p.get("hi", 8000.0), SR, got["mfcc"], got["status"][:, 0], op.id)
    _some(got["status"][:, 0] == 0, "status 0")


def o_formants(oracle, pkg, op, frames, got, vb):
    F = frames.shape[0]
    seg, est, stable = set(int(s) for s in _segs(F)), EST0.copy(), 0
    for f in range(F):
        if f in seg:
            est = EST0.copy()
        s, est, res, coeffs = oracle.find_formants(frames[f].astype(f64), SR, op.p["p"], est)
        assert got["status"][f, 0] == s, (op.id, f)
        if s != 0:
            continue
        n = got["res_count"][f, 0]
        assert n == np.count_nonzero(res[:, 0]), (op.id, f, n, res[:, 0])          # the oracle's rows are zero padded to 32
        assert np.all(rel_close(got["coeffs"][f], coeffs)), (op.id, f, "burg")
        assert np.all(np.abs(got["res"][f].reshape(-1, 2)[:n, 0] - res[:n, 0]) <= 1e-4 * np.abs(res[:n, 0])), (op.id, f, "res")
        # the tracker's step on the GPU's own resonance row (the rows agree to 1e-10: the step picks the same entries)
        assert np.all(np.abs(got["formants"][f].reshape(-1, 2)[:, 0] - est[:, 0]) <= 1e-4 * np.abs(est[:, 0])), (op.id, f, "formants")
        stable += 1
    assert stable > 0


def o_rms(oracle, pkg, op, frames, got, vb):
    xw = _win(oracle, op, frames)
    for f in range(xw.shape[0]):
        assert np.all(rel_close(got["rms"][f], oracle.rms(xw[f]), 1e-12)), (op.id, f)
    _some(got["rms"] > 0, "rms")


def o_peak(oracle, pkg, op, frames, got, vb):
    assert np.array_equal(got["peak"][:, 0], np.max(np.abs(frames), axis=1))
    _some(got["peak"] > 0, "peak")


def o_preemph(oracle, pkg, op, frames, got, vb):
    for f in range(frames.shape[0]):
        assert np.all(rel_close(got["out"][f], oracle.preemphasis(frames[f], 0.1), 1e-12)), (op.id, f)
    _some(got["out"] != 0, "out")


def o_resample(oracle, pkg, op, frames, got, vb):
    for f in range(frames.shape[0]):
        assert np.array_equal(got["out"][f], oracle.resample_linear(frames[f], op.p["ratio"])), (op.id, f)
    _some(got["out"] != 0, "out")


def o_analyze(oracle, pkg, op, frames, got, vb):
    """The fused record against the oracle's frame loop (tests/analyze_reference.py), column by column."""
    import analyze_reference as ar
    p, F = op.p["params"], frames.shape[0]
    fr = frames.astype(f64) / 32767.0 if op.p.get("pcm") else frames
    mf = op.p.get("mfcc", (13, 100.0, 8000.0))
    rec, st, top2, counts = ar.oracle_records(oracle, fr.reshape(-1), op.N, op.N, range(F), SR, (0.2, 75.0, 600.0),
                                              int(p.lpc_order), int(p.formant_order), EST0, mf, _segs(F))
    cols, g, voiced = p.columns(), got["records"], 0
    assert np.array_equal(got["status3"], st), (op.id, np.argwhere(got["status3"] != st)[:4])
    for f in range(F):
        if st[0, f] == 0:
            kind = ar.classify_top(g[f, 0:2], top2[f], counts[f])
            assert kind in ("ok", "swap"), (op.id, f, kind, g[f, 0:2], top2[f])
            voiced += int(g[f, 0] > 0)
        if "formants" in cols and st[1, f] == 0:
            c0, cw = cols["formants"]
            assert np.all(np.abs(g[f, c0:c0 + cw:2] - rec[f, c0:c0 + cw:2]) <= 1e-4 * np.abs(rec[f, c0:c0 + cw:2])), (op.id, f, "formants")
        if "mfcc" in cols and st[2, f] == 0:
            c0, cw = cols["mfcc"]
            assert np.all(rel_close(g[f, c0:c0 + cw], rec[f, c0:c0 + cw])), (op.id, f, "mfcc")
        if "lpc" in cols:
            c0, cw = cols["lpc"]
            assert np.all(rel_close(g[f, c0:c0 + cw], rec[f, c0:c0 + cw])), (op.id, f, "lpc")
    assert voiced > 0


def _win32(oracle, op, frames):
    """Windower<f32>: the windowed product is an f32."""
    return (frames * oracle.window("hanning", op.N).astype(f32)).astype(f32) if op.window else frames


def o_autocorr_f32(oracle, pkg, op, frames, got, vb):
    x = _win32(oracle, op, frames)
    if op.p.get("wide"):
        pa.rounded_once(got["r"], vb.autocorrelate(x.astype(f64), op.p["lags"]), op.id)
        pa.autocorrelate_rows(oracle, x.astype(f64), op.p["lags"], got["r"], op.id)
    else:
        pa.autocorrelate_f32_rows(oracle, x, op.p["lags"], got["r"], op.id)
    _some(got["r"][:, 0] != 0, "r[0]")


def o_autocorr_lpc_f32(oracle, pkg, op, frames, got, vb):
    x, p = _win32(oracle, op, frames), op.p["p"]
    if op.p.get("wide"):
        r64, a64 = vb.autocorr_lpc(x.astype(f64), p)
        pa.rounded_once(got["r"], r64, op.id)
        pa.rounded_once(got["lpc"], a64, op.id)
        pa.autocorr_lpc_rows(oracle, x.astype(f64), p, 0, r64, a64, op.id)
    else:
        pa.autocorrelate_f32_rows(oracle, x, p + 1, got["r"], op.id)
        pa.lpc_f32_rows(oracle, got["r"], p, got["lpc"], None, op.id)
    _some(np.abs(got["lpc"][:, 1]) > 0, "a1")


def o_burg_f32(oracle, pkg, op, frames, got, vb):
    x, p = _win32(oracle, op, frames), op.p["p"]
    if op.p.get("wide"):
        c64, s64 = vb.lpc_praat(x.astype(f64), p)
        assert np.array_equal(got["status"][:, 0], s64)
        pa.rounded_once(got["coeffs"], c64, op.id)
        pa.burg_rows(oracle, x.astype(f64), p, c64, s64, op.id)
    else:
        pa.burg_f32_rows(oracle, x, p, got["coeffs"], got["status"][:, 0], op.id)
    _some(got["status"][:, 0] == 0, "status 0")


def o_mfcc_f32(oracle, pkg, op, frames, got, vb):
    x = _win32(oracle, op, frames)
    m64, s64 = vb.mfcc(x.astype(f64), 13, (100.0, 8000.0), SR)
    assert np.array_equal(got["status"][:, 0], s64)
    pa.rounded_once(got["mfcc"], m64, op.id)
    pa.mfcc_rows(oracle, x.astype(f64), 13, 100.0, 8000.0, SR, m64, s64, op.id)
    _some(got["status"][:, 0] == 0, "status 0")


def o_pitch_f32(oracle, pkg, op, frames, got, vb):
    x, kmax = _win32(oracle, op, frames), op.p["kmax"]
    cand = got["cand"].reshape(-1, kmax, 2)
    if op.p.get("wide"):
        c64, k64, s64 = vb.pitch(x.astype(f64), SR, 0.2, 75.0, 600.0, kmax=kmax)
        pa.rounded_once(cand, c64, op.id)
        assert np.array_equal(got["count"][:, 0], k64) and np.array_equal(got["status"][:, 0], s64)
        voiced = int(np.sum(cand[:, 0, 0] > 0))
    else:
        n_cmp, _, voiced = pa.pitch_f32_rows(oracle, x, SR, 0.2, 75.0, 600.0, cand, got["count"][:, 0], got["status"][:, 0], op.id)
        assert n_cmp >= x.shape[0] // 2
    assert voiced > 0, "no voiced frame in this case"


def outs_autocorr(F, N, p):
    return [("r", f64, p["lags"])]


def outs_autocorr_lpc(F, N, p):
    return [("r", f64, p["p"] + 1), ("lpc", f64, p["p"] + 1)]


def outs_burg(F, N, p):
    return [("coeffs", f64, p["p"]), ("status", i32, 1)]


def outs_pitch(F, N, p):
    return [("cand", f64, 2 * p["kmax"]), ("count", i32, 1), ("status", i32, 1)]


def outs_mfcc(F, N, p):
    return [("mfcc", f64, 13), ("status", i32, 1)]


def outs_formants(F, N, p):
    return [("formants", f64, 8), ("res", f64, 64), ("res_count", i32, 1), ("coeffs", f64, p["p"]), ("status", i32, 1)]


def outs_analyze(F, N, p):
    return [("records", f64, p["rec"]), ("status3", i32, 3, F)]


def _f32(outs):
    return lambda F, N, p: [(n, f32 if dt == f64 else dt, c) for n, dt, c in outs(F, N, p)]


def _analyze_op(pkg, id, N, kernels, fpb, pcm=False, branches=(), **kw):
    p = dict(kw, pcm=pcm)
    p["params"] = _aparams(pkg, p)
    p["rec"] = max(c0 + w for c0, w in p["params"].columns().values())      # == vbx_record_doubles (asserted where the op runs)
    ld0 = p["rec"] + 2 - (p["rec"] & 1)                     # the smallest even value above the record size
    return Op(id, c_analyze, N, outs_analyze, kernels, fpb, o_analyze, p=p, dtype=i16 if pcm else f64, optional=("status3",),
              branches=branches, ld_pad=[{"records": ld0}, {"records": ld0 + 4}], keep_aligned=("records",))


def make_ops(pkg):
    """Shapes chosen from the dispatch in vbx_api.hip; fpb = the kernel's frames per block (AC_FPW = 16, k_lpc.hip; BF_FPW = 16, 8 up
    to 512 samples, vbx_burg_fast.hpp; LX_FPW = 16; the spectral, pitch, MFCC and long-frame kernels take one frame per block,
    the direct Burg 64 / lane-group frames: 4 at orders <= 16)."""
    sp, p2 = ("k_spectral.hip:al",), ("vbx_spectral_pow2.hpp:al",)
    ops = [
        # few-lag autocorrelation: full lengths (both sides of vec16) and partial ones
        Op("autocorr-512x13", c_autocorr, 512, outs_autocorr, {"autocorr_fewlags"}, 16, o_autocorr, dict(lags=13), branches=("k_lpc.hip:vec16",)),
        Op("autocorr-1024x17-win", c_autocorr, 1024, outs_autocorr, {"autocorr_fewlags"}, 16, o_autocorr, dict(lags=17), window=True,
           branches=("k_lpc.hip:vec16",)),
        Op("autocorr-100x7", c_autocorr, 100, outs_autocorr, {"autocorr_fewlags"}, 16, o_autocorr, dict(lags=7)),
        Op("autocorr-1200x13-win", c_autocorr, 1200, outs_autocorr, {"autocorr_fewlags"}, 16, o_autocorr, dict(lags=13), window=True),
        # the FFT lag form (1200-point plan, even and odd lag counts: both sides of the output rows' branch) and a padded frame
        Op("autocorr-1200x1200-win", c_autocorr, 1200, outs_autocorr, {"autocorr_fft"}, 1, o_autocorr, dict(lags=1200), window=True,
           branches=sp + ("spectral:out_r al",)),
        Op("autocorr-1103x1103", c_autocorr, 1103, outs_autocorr, {"autocorr_fft"}, 1, o_autocorr, dict(lags=1103), branches=sp + ("spectral:out_r al",)),
        Op("autocorr-2048x40-win", c_autocorr, 2048, outs_autocorr, {"autocorr_fft"}, 1, o_autocorr, dict(lags=40), window=True,
           branches=p2 + ("spectral:out_r al",)),
        # the matrix-core tiles below 512 samples, and the long-frame tiles
        Op("autocorr-333x333", c_autocorr, 333, outs_autocorr, {"autocorr_tiles"}, 1, o_autocorr, dict(lags=333)),
        Op("autocorr-4097x40", c_autocorr, 4097, outs_autocorr, {"autocorr_long"}, 1, o_autocorr, dict(lags=40)),
        Op("autocorr-5000x65-win", c_autocorr, 5000, outs_autocorr, {"autocorr_long"}, 1, o_autocorr, dict(lags=65), window=True),
        Op("autocorr-1024x18-reference", c_autocorr, 1024, outs_autocorr, {"autocorr_ref"}, 1, o_autocorr, dict(lags=18), policy=pkg.LPC_POLICY_REFERENCE),
        # autocorrelate -> lpc fused, the three policies; a general shape (three launches)
        Op("autocorr_lpc-512x12-exact", c_autocorr_lpc, 512, outs_autocorr_lpc, {"autocorr_lpc", "lpc_exact_list"}, 16, o_autocorr_lpc,
           dict(p=12), window=True, optional=("r", "lpc"), branches=("k_lpc.hip:vec16",), policy=pkg.LPC_POLICY_EXACT),
        Op("autocorr_lpc-1024x16-plain-norm", c_autocorr_lpc, 1024, outs_autocorr_lpc, {"autocorr_lpc"}, 16, o_autocorr_lpc,
           dict(p=16, norm=1), window=True, optional=("r", "lpc"), branches=("k_lpc.hip:vec16",), policy=pkg.LPC_POLICY_PLAIN),
        Op("autocorr_lpc-1200x12-reference", c_autocorr_lpc, 1200, outs_autocorr_lpc, {"lpc_ref"}, 1, o_autocorr_lpc,
           dict(p=12), window=True, optional=("r", "lpc"), policy=pkg.LPC_POLICY_REFERENCE),
        Op("autocorr_lpc-700x20-general", c_autocorr_lpc, 700, outs_autocorr_lpc, {"autocorr_tiles", "levinson_rows"}, 16, o_autocorr_lpc,
           dict(p=20), window=True, optional=("r", "lpc"), policy=pkg.LPC_POLICY_EXACT),
        # Burg: one pass at two orders and lengths (+ the segmented lag kernel above 1280), the direct form
        Op("burg-512x12", c_burg, 512, outs_burg, {"burg_lags", "burg_recursion", "burg_direct_list"}, 8, o_burg, dict(p=12),
           optional=("status",), branches=("vbx_burg_fast.hpp:wide",)),
        Op("burg-1200x16-win", c_burg, 1200, outs_burg, {"burg_lags", "burg_recursion"}, 16, o_burg, dict(p=16), window=True,
           optional=("status",), branches=("vbx_burg_fast.hpp:wide",)),
        Op("burg-2048x8", c_burg, 2048, outs_burg, {"burg_lags", "burg_recursion"}, 16, o_burg, dict(p=8), optional=("status",),
           branches=("vbx_burg_fast.hpp:al",)),
        Op("burg-512x9-direct", c_burg, 512, outs_burg, {"burg"}, 4, o_burg, dict(p=9), window=True, optional=("status",),
           branches=("k_burg.hip:vec",)),
        Op("burg-1024x12-forced-direct", c_burg, 1024, outs_burg, {"burg"}, 4, o_burg, dict(p=12), optional=("status",),
           branches=("k_burg.hip:vec",), env={"VBX_BURG_DIRECT": "1"}),
        Op("burg-5000x10-long", c_burg, 5000, outs_burg, {"burg_long"}, 1, o_burg, dict(p=10), optional=("status",)),
        # pitch: lane list (kmax 1, 4), LDS list (65), the whole Vec; the plans; matrix-core form below 512; long frames
        Op("pitch-1200-k1", c_pitch, 1200, outs_pitch, {"pitch"}, 1, o_pitch, dict(kmax=1), window=True, optional=("count", "status"), branches=sp, form=400),
        Op("pitch-1200-k4", c_pitch, 1200, outs_pitch, {"pitch"}, 1, o_pitch, dict(kmax=4), window=True, optional=("count", "status"), branches=sp, form=400),
        Op("pitch-1200-k65", c_pitch, 1200, outs_pitch, {"pitch"}, 1, o_pitch, dict(kmax=65), window=True, optional=("count", "status"), branches=sp, form=401),
        Op("pitch-1200-whole", c_pitch, 1200, outs_pitch, {"pitch"}, 1, o_pitch, dict(kmax=302), window=True, optional=("count", "status"), branches=sp, form=402),
        Op("pitch-1103-k4", c_pitch, 1103, outs_pitch, {"pitch"}, 1, o_pitch, dict(kmax=4), window=True, optional=("count", "status"), branches=sp, form=400),
        Op("pitch-1024-k4", c_pitch, 1024, outs_pitch, {"pitch"}, 1, o_pitch, dict(kmax=4), window=True, optional=("count", "status"), branches=p2, form=500),
        Op("pitch-2048-k2", c_pitch, 2048, outs_pitch, {"pitch"}, 1, o_pitch, dict(kmax=2), window=True, optional=("count", "status"), branches=p2, form=600),
        Op("pitch-4096-k4", c_pitch, 4096, outs_pitch, {"pitch"}, 1, o_pitch, dict(kmax=4), window=True, optional=("count", "status"), branches=p2, form=700),
        Op("pitch-4096-whole", c_pitch, 4096, outs_pitch, {"pitch"}, 1, o_pitch, dict(kmax=1026), window=True, optional=("count", "status"), branches=p2, form=701),
        Op("pitch-400-k4", c_pitch, 400, outs_pitch, {"pitch"}, 1, o_pitch, dict(kmax=4), window=True, optional=("count", "status"), form=200),
        Op("pitch-4097-k4", c_pitch, 4097, outs_pitch, {"autocorr_long", "pitch_long"}, 1, o_pitch, dict(kmax=4), window=True,
           optional=("count", "status"), form=100),
        Op("pitch-5000-k70", c_pitch, 5000, outs_pitch, {"autocorr_long", "pitch_long"}, 1, o_pitch, dict(kmax=70), window=True,
           optional=("count", "status"), form=100),
        # MFCC: Goertzel, two-stage / matrix-core, the transforms' own bins, interpolated, chirp-z, long
        Op("mfcc-337", c_mfcc, 337, outs_mfcc, {"mfcc"}, 1, o_mfcc, window=True, optional=("status",), form=6),
        Op("mfcc-400", c_mfcc, 400, outs_mfcc, {"mfcc"}, 1, o_mfcc, window=True, optional=("status",), form=4),
        Op("mfcc-1000", c_mfcc, 1000, outs_mfcc, {"mfcc"}, 1, o_mfcc, window=True, optional=("status",), form=4),
        Op("mfcc-700", c_mfcc, 700, outs_mfcc, {"mfcc"}, 1, o_mfcc, window=True, optional=("status",), form=4),
        Op("mfcc-1200", c_mfcc, 1200, outs_mfcc, {"mfcc"}, 1, o_mfcc, window=True, optional=("status",), branches=sp, form=1),
        Op("mfcc-1024", c_mfcc, 1024, outs_mfcc, {"mfcc"}, 1, o_mfcc, window=True, optional=("status",), branches=p2, form=1),
        Op("mfcc-2048", c_mfcc, 2048, outs_mfcc, {"mfcc"}, 1, o_mfcc, window=True, optional=("status",), branches=p2, form=1),
        Op("mfcc-4096", c_mfcc, 4096, outs_mfcc, {"mfcc"}, 1, o_mfcc, window=True, optional=("status",), branches=p2, form=1),
        Op("mfcc-1103-interp", c_mfcc, 1103, outs_mfcc, {"mfcc"}, 1, o_mfcc, window=True, optional=("status",), form=2),
        Op("mfcc-1103-czt", c_mfcc, 1103, outs_mfcc, {"mfcc"}, 1, o_mfcc, dict(hi=16000.0), window=True, optional=("status",), form=3),
        # the vector two-stage DFT: lengths whose factorisation does not fit the matrix-core tiles; VBX_MFCC_DFT2=1, read when a
        # context is created, keeps it covered at 1200 (tests/test_gpu_parity.py::test_mfcc_four_kernels_agree does the same)
        Op("mfcc-1200-dft2", c_mfcc, 1200, outs_mfcc, {"mfcc"}, 1, o_mfcc, window=True, optional=("status",), form=5,
           ctx_env={"VBX_MFCC_DFT2": "1"}),
        Op("mfcc-5000-long", c_mfcc, 5000, outs_mfcc, {"mfcc_long"}, 1, o_mfcc, window=True, optional=("status",), form=7),
        # find_formants: Burg one pass + pair roots (12), the reference's root iteration (order 9: outside the list)
        Op("find_formants-1200x12", c_formants, 1200, outs_formants, {"burg_lags", "formant_resonances", "tracker"}, 16, o_formants, dict(p=12),
           optional=("res", "res_count", "coeffs", "status")),
        Op("find_formants-512x9", c_formants, 512, outs_formants, {"burg", "formant_resonances", "tracker"}, 4, o_formants, dict(p=9),
           optional=("res", "res_count", "coeffs", "status")),
        # front end
        Op("rms-1200-win", c_rms, 1200, lambda F, N, p: [("rms", f64, 1)], {"rms"}, 1, o_rms, window=True),
        Op("frame_peak-1200", c_peak, 1200, lambda F, N, p: [("peak", f64, 1)], {"frame_peak"}, 1, o_peak),
        Op("preemphasis-1200", c_preemph, 1200, lambda F, N, p: [("out", f64, N)], {"preemphasis"}, 1, o_preemph),
        Op("preemphasis-5000", c_preemph, 5000, lambda F, N, p: [("out", f64, N)], {"preemphasis_long"}, 1, o_preemph),
        Op("resample-1200x0.25", c_resample, 1200, lambda F, N, p: [("out", f64, 300)], {"resample"}, 1, o_resample, dict(ratio=0.25)),
        # the fused loops
        _analyze_op(pkg, "analyze-1200", 1200, {"analyze", "tracker"}, 1, branches=sp),
        _analyze_op(pkg, "analyze-1103", 1103, {"analyze", "tracker"}, 1, branches=sp),
        _analyze_op(pkg, "analyze-1024", 1024, {"analyze", "tracker"}, 1, branches=p2),
        _analyze_op(pkg, "analyze_pcm16-1200", 1200, {"analyze", "tracker"}, 1, pcm=True, branches=("k_spectral.hip:x16",)),
        _analyze_op(pkg, "analyze_pcm16-1024", 1024, {"analyze", "pcm16", "tracker"}, 1, pcm=True),
        # Sample = f32: the reference-faithful and the wide forms
        Op("autocorr_f32-512x13", c_autocorr_f32, 512, _f32(outs_autocorr), {"autocorr_f32_exact"}, 1, o_autocorr_f32, dict(lags=13), window=True, dtype=f32),
        Op("autocorr_f32_wide-512x13", c_autocorr_f32, 512, _f32(outs_autocorr), {"autocorr_fewlags_f32"}, 16, o_autocorr_f32, dict(lags=13, wide=1),
           window=True, dtype=f32),
        Op("autocorr_f32_wide-1200x200", c_autocorr_f32, 1200, _f32(outs_autocorr), {"widen_frames", "narrow"}, 1, o_autocorr_f32, dict(lags=200, wide=1),
           window=True, dtype=f32),
        Op("autocorr_lpc_f32-512x12", c_autocorr_lpc_f32, 512, _f32(outs_autocorr_lpc), {"autocorr_f32_exact", "levinson_f32_exact"}, 1, o_autocorr_lpc_f32,
           dict(p=12), window=True, dtype=f32, optional=("r", "lpc")),
        Op("autocorr_lpc_f32_wide-512x12", c_autocorr_lpc_f32, 512, _f32(outs_autocorr_lpc), {"autocorr_lpc_f32"}, 16, o_autocorr_lpc_f32,
           dict(p=12, wide=1), window=True, dtype=f32, optional=("r", "lpc")),
        Op("burg_f32-512x12", c_burg_f32, 512, _f32(outs_burg), {"burg_f32_exact"}, 64, o_burg_f32, dict(p=12), window=True, dtype=f32, optional=("status",)),
        Op("burg_f32_wide-512x12", c_burg_f32, 512, _f32(outs_burg), {"burg_f32"}, 4, o_burg_f32, dict(p=12, wide=1), window=True, dtype=f32,
           optional=("status",)),
        Op("mfcc_f32-1200", c_mfcc_f32, 1200, _f32(outs_mfcc), {"widen_frames", "mfcc", "narrow"}, 1, o_mfcc_f32, window=True, dtype=f32, optional=("status",), form=1),
        Op("pitch_f32-1200-k4", c_pitch_f32, 1200, _f32(outs_pitch), {"pitch_f32_exact", "narrow"}, 1, o_pitch_f32, dict(kmax=4), window=True, dtype=f32,
           optional=("count", "status")),
        Op("pitch_f32_wide-1200-k4", c_pitch_f32, 1200, _f32(outs_pitch), {"widen_frames", "pitch", "narrow"}, 1, o_pitch_f32, dict(kmax=4, wide=1), window=True,
           dtype=f32, optional=("count", "status"), form=400),
    ]
    return ops


def _op_ids():
    import __graft_entry__ as g
    return [op.id for op in make_ops(g.load_package())]


@pytest.mark.parametrize("op_id", _op_ids())
def test_frame_batch_entry_point_across_layouts(vb, pkg, oracle, speech, monkeypatch, op_id):
    op = next(o for o in make_ops(pkg) if o.id == op_id)
    check_op(vb, pkg, oracle, speech, op, monkeypatch)


# ---- the fused loops reject records at 8 mod 16 (the alignment the header asks for), and leave everything untouched ----------------

@pytest.mark.parametrize("pcm", [False, True])
def test_analyze_rejects_records_off_16_bytes(vb, pkg, speech, pcm):
    N, F = 1200, 5
    fs = frameset(speech, N, F, "hop", i16 if pcm else f64)
    p = _aparams(pkg, {})
    rec = int(vb.L.vbx_record_doubles(C.byref(p)))
    ld = rec + (rec & 1)
    a = la.Arena(la.DeviceBackend(vb), "analyze records at 8 mod 16")
    a.input("x", fs.frames.reshape(-1))
    a.output("records", f64, F, rec, ld=ld, residue=8)
    a.output("status3", i32, 3, F, residue=4)
    a.place()
    fn = vb.L.vbx_analyze_frames_pcm16 if pcm else vb.L.vbx_analyze_frames_f64
    rc = fn(vb.ctx, a["x"], F, N, N, C.byref(p), None, 0, a["records"], ld, a["status3"])
    msg = vb.L.vbx_last_error(vb.ctx).decode()
    assert rc == -1 and "records must be 16-byte aligned" in msg, (rc, msg)
    out = a.finish()                                         # fences intact ...
    assert la.unwritten(out["records"]).shape[0] == out["records"].size          # ... and nothing written
    assert la.unwritten(out["status3"]).shape[0] == out["status3"].size
    assert vb.autocorrelate(np.ones((2, 64)), 3).shape == (2, 3)                 # the context is still usable


# ---- entry points on rows (no Windower view): lpc, polynomials, resonances, tracker, dct, path, front end --------------------------

def _rows_cases(inputs, outputs, in_names, skip_out_min=()):
    """canonical + A (each input in turn off alignment) + C (outputs at their smallest alignment) + F (all at once)."""
    def place(in_off, out_min):
        i = {n: ((s[0], min(in_res(s[0].dtype, 4), 8) if n in in_off else 0) + tuple(s[2:])) for n, s in inputs.items()}
        o = {n: (dt, r, c, ld, min_res(dt) if out_min and n not in skip_out_min else 0) for n, (dt, r, c, ld, _) in outputs.items()}
        return i, o
    cases = [("canonical", place((), False))]
    for n in in_names:
        cases.append(("A-" + n, place((n,), False)))
    cases.append(("C", place((), True)))
    cases.append(("F", place(in_names, True)))
    return cases


def _run_rows(vb, id, inputs, outputs, in_names, call, kernels, skip=(), skip_out_min=()):
    canon = None
    for tag, (i, o) in _rows_cases(inputs, outputs, in_names, skip_out_min):
        vb.profile_reset()
        got, _ = arena_call(vb, f"{id} {tag}", i, o, call)
        if canon is None:
            canon = got
            kernels_ran(vb, id, kernels)
            for n in got:
                if n not in skip:
                    la.assert_written(id, n, got[n])
        else:
            same(f"{id} layout {tag}", got, canon)
    return canon


@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, F_PRIME])
@pytest.mark.parametrize("policy", ["exact", "reference"])
def test_lpc_rows(vb, pkg, oracle, F, policy):
    """vbx_lpc_f64 / vbx_lpc_mut_f64 (one lane per row, 64 rows per block) incl. layout G: r_stride = n_coeffs + 1 + 3 with NaN in
    the padding, and H: out_kc NULL."""
    p = 12
    rng = np.random.default_rng(F)
    x = rng.standard_normal((F, 400)) * np.hanning(400)
    r = np.stack([oracle.autocorrelate(x[f], p + 1) for f in range(F)])
    rpad = np.full((F, p + 4), np.nan)
    rpad[:, :p + 1] = r
    old = vb.lpc_policy
    vb.lpc_policy = pkg.LPC_POLICY_REFERENCE if policy == "reference" else pkg.LPC_POLICY_EXACT
    kern = {"levinson_ref_rows"} if policy == "reference" else {"levinson_rows"}
    try:
        outs = {"ac": (f64, F, p + 1, None, 0), "kc": (f64, F, p, None, 0)}
        canon = _run_rows(vb, f"lpc_mut-{policy}-F{F}", {"r": (r, 0)}, outs, ("r",),
                          lambda a: vb.L.vbx_lpc_mut_f64(vb.ctx, a["r"], F, p + 1, p, a["ac"], a["kc"]), kern)
        for f in range(F):
            assert np.all(rel_close(canon["ac"][f], oracle.lpc(r[f], p))), f
            assert canon["kc"][f, p - 1] == canon["ac"][f, p]
        for res in (0, 8):                                   # G: padded rows, NaN in the padding; H: no kc; vbx_lpc_f64
            got, _ = arena_call(vb, f"lpc_mut G r_stride={p + 4} r%16={res}", {"r": (rpad, res)}, outs,
                                lambda a: vb.L.vbx_lpc_mut_f64(vb.ctx, a["r"], F, p + 4, p, a["ac"], a["kc"]))
            same("lpc_mut layout G", got, canon)
            got, _ = arena_call(vb, f"lpc_mut H-kc r%16={res}", {"r": (rpad, res)}, {"ac": (f64, F, p + 1, None, res)},
                                lambda a: vb.L.vbx_lpc_mut_f64(vb.ctx, a["r"], F, p + 4, p, a["ac"], None))
            same("lpc_mut layout H-kc", got, {"ac": canon["ac"]})
            got, _ = arena_call(vb, f"lpc G r_stride={p + 4} r%16={res}", {"r": (rpad, res)}, {"ac": (f64, F, p + 1, None, res)},
                                lambda a: vb.L.vbx_lpc_f64(vb.ctx, a["r"], F, p + 4, p, a["ac"]))
            same("lpc layout G", got, {"ac": canon["ac"]})
    finally:
        vb.lpc_policy = old


@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, F_PRIME])
def test_normalize_and_dct_rows(vb, oracle, F):
    rng = np.random.default_rng(F + 1)
    rows = rng.standard_normal((F, 13))
    canon = _run_rows(vb, f"normalize-F{F}", {"data": (rows, 0, True)}, {}, ("data",),
                      lambda a: vb.L.vbx_normalize_f64(vb.ctx, a["data"], F, 13), {"normalize_rows"})
    for f in range(F):
        assert np.all(rel_close(canon["data"][f], oracle.normalize(rows[f]), 1e-14))
    canon = _run_rows(vb, f"dct-F{F}", {"in": (rows, 0)}, {"out": (f64, F, 13, None, 0)}, ("in",),
                      lambda a: vb.L.vbx_dct_f64(vb.ctx, a["in"], F, 13, a["out"]), {"dct_rows"})
    for f in range(F):
        assert np.all(rel_close(canon["out"][f], oracle.dct(rows[f])))


@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, F_PRIME])
def test_f32_rows(vb, oracle, speech, F):
    """vbx_normalize_f32 (in place), vbx_lpc_mut_f32 and vbx_lpc_mut_f32_wide on float rows at 0, 4, 8 and 12 mod 16; out_kc NULL;
    r_stride with NaN padding.  The assertions of tests/test_gpu_f32.py::test_normalize_and_lpc_f32, every row."""
    p, n = 12, 512
    x = (la.windows(speech.astype(f32), n, 97, F) * oracle.window("hanning", n).astype(f32)).astype(f32)
    r = np.stack([oracle.autocorrelate_f32(row, p + 1) for row in x])
    canon = None
    for res in (0, 4, 8, 12):
        vb.profile_reset()
        got, _ = arena_call(vb, f"normalize_f32 F={F} data%16={res}", {"data": (r, res, True)}, {},
                            lambda a: vb.L.vbx_normalize_f32(vb.ctx, a["data"], F, p + 1))
        if canon is None:
            canon = got
            kernels_ran(vb, f"normalize_f32-F{F}", {"normalize_rows_f32"})
            pa.normalize_f32_rows(oracle, r, got["data"])
        else:
            same(f"normalize_f32 data%16={res}", got, canon)
    rn = canon["data"]
    rpad = np.full((F, p + 4), np.nan, dtype=f32)
    rpad[:, :p + 1] = rn
    for wide, fn, kern in ((False, vb.L.vbx_lpc_mut_f32, "levinson_f32_exact"), (True, vb.L.vbx_lpc_mut_f32_wide, "levinson_rows_f32")):
        canon = None
        for res in (0, 4, 8, 12):
            vb.profile_reset()
            outs = {"ac": (f32, F, p + 1, None, res), "kc": (f32, F, p, None, res)}
            got, _ = arena_call(vb, f"lpc_mut_f32{'_wide' if wide else ''} F={F} %16={res}", {"r": (rn, res)}, outs,
                                lambda a: fn(vb.ctx, a["r"], F, p + 1, p, a["ac"], a["kc"]))
            if canon is None:
                canon = got
                kernels_ran(vb, f"lpc_mut_f32{'_wide' if wide else ''}-F{F}", {kern})
                for name in got:
                    la.assert_written("lpc_mut_f32", name, got[name])
                if wide:
                    ac64, kc64 = vb.lpc_mut(rn.astype(f64), p)
                    pa.rounded_once(got["ac"], ac64)
                    pa.rounded_once(got["kc"], kc64)
                    for f in range(F):
                        assert np.all(rel_close(ac64[f], oracle.lpc(rn[f].astype(f64), p))), f
                else:
                    pa.lpc_f32_rows(oracle, rn, p, got["ac"], got["kc"])
            else:
                same(f"lpc_mut_f32 %16={res}", got, canon)
            got, _ = arena_call(vb, f"lpc_mut_f32{'_wide' if wide else ''} G+H F={F} %16={res}", {"r": (rpad, res)}, {"ac": (f32, F, p + 1, None, res)},
                                lambda a: fn(vb.ctx, a["r"], F, p + 4, p, a["ac"], None))
            same("lpc_mut_f32 padded rows, no kc", got, {"ac": canon["ac"]})


@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, F_PRIME])
@pytest.mark.parametrize("deg", [8, 12])
def test_polynomial_rows(vb, pkg, oracle, F, deg):
    """vbx_find_roots_c64 (in place), vbx_laguerre_c64, vbx_div_polynomial_c64, vbx_to_resonance_c64 and the c32 forms: arrays of
    {re, im} at 8 mod 16 (what C gives an array of vbx_complex), statuses at 4 mod 16."""
    rng = np.random.default_rng(deg * 100 + F)
    polys = (rng.standard_normal((F, deg + 1)) + 0j).astype(c128)
    polys[:, -1] = 1.0
    canon = _run_rows(vb, f"find_roots-{deg}-F{F}", {"polys": (polys, 0, True)}, {"status": (i32, F, 1, None, 0)}, ("polys",),
                      lambda a: vb.L.vbx_find_roots_c64(vb.ctx, a["polys"], F, deg + 1, a["status"]), {"find_roots"})
    assert pa.find_roots_rows(oracle, polys, canon["polys"], canon["status"][:, 0], f"find_roots-{deg}") > 0
    roots = canon["polys"][:, :deg].copy()
    start = pkg.voxbox._Complex(-2.0, -2.0)
    canon_l = _run_rows(vb, f"laguerre-{deg}-F{F}", {"polys": (polys, 0)}, {"out": (c128, F, 1, None, 0)}, ("polys",),
                        lambda a: vb.L.vbx_laguerre_c64(vb.ctx, a["polys"], F, deg + 1, start, a["out"]), {"laguerre"})
    for f in range(F):                                   # a root found by Laguerre: the tolerance of test_find_roots_random
        z = oracle.laguerre(polys[f], complex(-2.0, -2.0))
        assert abs(canon_l["out"][f, 0] - z) <= 1e-7 * max(1.0, abs(z)), (f, canon_l["out"][f, 0], z)
    others = (rng.uniform(-2, 2, F) + 1j * rng.uniform(-2, 2, F)).astype(c128)
    canon_d = _run_rows(vb, f"div_polynomial-{deg}-F{F}", {"polys": (polys, 0, True), "others": (others, 0)},
                        {"rem": (c128, F, deg + 1, None, 0), "status": (i32, F, 1, None, 0)}, ("polys", "others"),
                        lambda a: vb.L.vbx_div_polynomial_c64(vb.ctx, a["polys"], a["others"], F, deg + 1, a["rem"], a["status"]),
                        {"div_polynomial"})
    for f in range(F):                                   # the assertion of test_div_polynomial, every row
        es, eq, er = oracle.div_polynomial(polys[f], complex(others[f]))
        assert canon_d["status"][f, 0] == es, f
        assert np.allclose(canon_d["polys"][f], eq, rtol=1e-12, atol=1e-13) and np.allclose(canon_d["rem"][f], er, rtol=1e-12, atol=1e-13), f
    canon_r = _run_rows(vb, f"to_resonance-{deg}-F{F}", {"roots": (roots, 0)},
                        {"res": (f64, F, 2 * deg, None, 0), "count": (i32, F, 1, None, 0)}, ("roots",),
                        lambda a: vb.L.vbx_to_resonance_c64(vb.ctx, a["roots"], F, deg, SR, a["res"], a["count"]), {"to_resonance"})
    some = 0
    for f in range(F):
        e = oracle.to_resonance(roots[f], SR)
        n = canon_r["count"][f, 0]
        assert n == e.shape[0]
        assert np.all(rel_close(canon_r["res"][f].reshape(-1, 2)[:n], e, 1e-10)) and np.all(canon_r["res"][f, 2 * n:] == 0.0)
        some += int(n > 0)
    assert some > 0
    # the Complex<f32> instantiation: vbx_complex32 arrays at 4 and 12 mod 16 (4 mod 8: all C gives them) as well as 8
    P32 = polys.real.astype(f32)
    p32 = P32.astype(np.complex64)
    canon32 = None
    for res in (0, 4, 8, 12):
        vb.profile_reset()
        got, _ = arena_call(vb, f"find_roots_c32-{deg}-F{F} polys%16={res}", {"polys": (p32, res, True)},
                            {"status": (i32, F, 1, None, 4 if res else 0)},
                            lambda a: vb.L.vbx_find_roots_c32(vb.ctx, a["polys"], F, deg + 1, a["status"]))
        if canon32 is None:
            canon32 = got
            kernels_ran(vb, f"find_roots_c32-{deg}-F{F}", {"find_roots_f32"})
            assert pa.find_roots_f32_rows(oracle, P32, got["polys"], got["status"][:, 0], "find_roots_c32") > 0
        else:
            same(f"find_roots_c32 polys%16={res}", got, canon32)
    start32 = pkg.voxbox._Complex32(-2.0, -2.0)
    canon_l32 = None
    for res in (0, 4, 8, 12):
        vb.profile_reset()
        got, _ = arena_call(vb, f"laguerre_c32-{deg}-F{F} %16={res}", {"polys": (p32, res)}, {"out": (np.complex64, F, 1, None, res)},
                            lambda a: vb.L.vbx_laguerre_c32(vb.ctx, a["polys"], F, deg + 1, start32, a["out"]))
        if canon_l32 is None:
            canon_l32 = got
            kernels_ran(vb, f"laguerre_c32-{deg}-F{F}", {"laguerre_f32"})
            la.assert_written("laguerre_c32", "out", got["out"])
            for f in range(F):       # test_roots_f32_kats: within 1e-4 of the f32 oracle's limit; or, where f32 rounding sends the two
                # iterations to different roots, a root of the polynomial by test_find_roots_f32_random's residual bound
                zo, z = complex(oracle.laguerre_f32(P32[f], complex(-2.0, -2.0))), complex(got["out"][f, 0])
                pv = abs(np.polyval(P32[f, ::-1].astype(f64), z))
                scale = np.polyval(np.abs(P32[f, ::-1]).astype(f64), abs(z))
                assert abs(z - zo) <= 1e-4 * abs(zo) or pv <= 2e-4 * scale, (f, z, zo, pv / scale)
        else:
            same(f"laguerre_c32 %16={res}", got, canon_l32)


@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, F_PRIME, 419, 1300])
def test_tracker_rows(vb, pkg, oracle, F):
    """vbx_estimate_formants_f64: the plain scan (segments shorter than 384 frames) and, at 419 frames in one utterance, the chunked
    scan, at 1300 frames the chunked scan with three segments of 433; rows of vbx_resonance at 8 mod 16 in and out."""
    rng = np.random.default_rng(F + 5)
    n_res = 6
    res = np.zeros((F, n_res, 2))
    res[:, :, 0] = np.sort(rng.uniform(200.0, 4000.0, (F, n_res)), axis=1)
    res[:, :, 1] = rng.uniform(20.0, 300.0, (F, n_res))
    status = (rng.uniform(0, 1, F) < 0.1).astype(i32)
    for nseg in (1, 3):
        seg = np.array(sorted({0, F // 3, (2 * F) // 3})[:nseg] if F >= 6 else [0], dtype=np.int64)
        bounds = list(seg) + [F]                             # tracker_wants_chunks (vbx_api.hip): the longest utterance has >= 384 frames
        chunked = max(int(bounds[k + 1]) - int(bounds[k]) for k in range(seg.size)) >= 384
        canon = _run_rows(vb, f"estimate_formants-F{F}-seg{seg.size}", {"res": (res.reshape(F, -1), 0), "frame_status": (status, 0)},
                          {"out": (f64, F, 8, None, 0)}, ("res", "frame_status"),
                          lambda a: vb.L.vbx_estimate_formants_f64(vb.ctx, a["res"], F, n_res, seg.ctypes.data, seg.size,
                                                                   EST0.ctypes.data, 4, a["frame_status"], a["out"]),
                          {"tracker_chunked"} if chunked else {"tracker"})
        est, segs = EST0.copy(), set(int(s) for s in seg)
        for f in range(F):
            if f in segs:
                est = EST0.copy()
            if status[f] == 0:
                est = oracle.estimate_formants(est, res[f])
            assert np.array_equal(canon["out"][f].reshape(4, 2), est), (F, nseg, f)
        assert F < 63 or np.any(canon["out"] != np.tile(EST0.reshape(-1), (F, 1)))


def test_track_stitch_rows(vb, pkg, speech):
    """vbx_track_stitch_f64 on the rows of a find_formants call: formants and d_state_in at 8 mod 16, d_changed at 4 mod 16."""
    N, F = 1200, 60
    fs = frameset(speech, N, F, "hop")
    results = {}
    for tag, fres, sres, cres in (("canonical", 0, 0, 0), ("F", 8, 8, 4)):
        a = la.Arena(la.DeviceBackend(vb), f"track_stitch {tag}")
        a.input("x", fs.frames.reshape(-1))
        a.input("state", np.array([[500.0, 80.0], [1500.0, 90.0], [2500.0, 100.0], [3500.0, 120.0]]), residue=sres)
        a.output("formants", f64, F, 8, residue=fres)
        a.output("changed", i32, 1, 1, residue=cres)
        a.place()
        print("layout case: track_stitch", tag, flush=True)
        vb._check(vb.L.vbx_find_formants_f64(vb.ctx, a["x"], F, N, N, SR, 12, None, 0, EST0.ctypes.data, 4, a["formants"], None, None, None, None))
        vb.profile_reset()
        vb._check(vb.L.vbx_track_stitch_f64(vb.ctx, a["formants"], F, 8, 20, F, a["state"], a["changed"]))
        assert "tracker_stitch" in vb.profile_report()
        results[tag] = a.finish()
        REPORT["cases"] += 1
    assert results["canonical"]["changed"][0, 0] > 0         # the state really differed: rows were rewritten
    same("track_stitch layout F", results["F"], results["canonical"])


@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, F_PRIME, 1500])
@pytest.mark.parametrize("kmax", [1, 4, 15])
def test_pitch_path_rows(vb, pkg, speech, F, kmax):
    """vbx_pitch_path_f64 over the lists of a pitch call: cand (vbx_pitch) at 8 mod 16, count / status / out_index at 4 mod 16,
    local_peak at 8; H: out_index NULL, status NULL.  The canonical call against the sequential model (tests/pitch_path_model.py)."""
    import pitch_path_model as M
    N, hop = 1200, 240
    sig = speech[:(F - 1) * hop + N]
    cand, cnt, st = vb.pitch(sig, SR, 0.2, 75.0, 600.0, kmax=kmax, frame_len=N, stride=hop, n_frames=F, window=vb.window(pkg.WINDOW_HANNING, N))
    peak = np.max(np.abs(la.windows(sig, N, hop, F)), axis=1)
    seg = np.array(sorted({0, F // 3, (2 * F) // 3}) if F >= 6 else [0], dtype=np.int64)
    params = pkg.PitchPathParams.make(time_step=hop / SR)
    ins = {"cand": (cand.reshape(F, -1), 0), "count": (cnt, 0), "status": (st, 0), "peak": (peak, 0)}
    outs = {"path": (f64, F, 2, None, 0), "index": (i32, F, 1, None, 0)}

    def call(a):
        return vb.L.vbx_pitch_path_f64(vb.ctx, a["cand"], a["count"], a.get("status"), F, kmax, a["peak"], seg.ctypes.data, seg.size,
                                       C.byref(params), a["path"], a.get("index"))
    canon = _run_rows(vb, f"pitch_path-k{kmax}-F{F}", ins, outs, ("cand", "count", "status", "peak"), call, {"pitch_path_spec", "pitch_path_write"})
    p = dict(M.DEFAULTS, time_step=hop / SR)
    tab = M.frame_table(cand, cnt, st, peak, seg, p)
    own_p, own_i = M.outputs(tab, M.states_from_index(tab, canon["index"][:, 0]))
    assert np.array_equal(own_p.view(np.int64), canon["path"].view(np.int64))            # out_path is what out_index selects
    mp, mi = M.outputs(tab, M.path_states(tab, seg))
    diff = np.nonzero(mi != canon["index"][:, 0])[0]
    if diff.size:                                            # only inside a near tie of the model's scores (test_gpu_pitch_path.py)
        st_g = M.states_from_index(tab, canon["index"][:, 0])
        for s0, s1 in M.segments(seg, tab["F"]):
            if s1 > s0 and np.any((diff >= s0) & (diff < s1)):
                sa, sb = M.path_score(tab, M.path_states(tab, seg), s0, s1), M.path_score(tab, st_g, s0, s1)
                assert abs(sa - sb) <= 1e-12 * max(abs(sa), abs(sb), 1.0)
    if F >= 63:
        assert np.any(canon["path"][:, 0] > 0)
    ins8 = {n: (s[0], in_res(s[0].dtype, 4)) for n, s in ins.items()}
    got, _ = arena_call(vb, f"pitch_path H-index k{kmax} F{F}", ins8, {"path": (f64, F, 2, None, 8)}, call)
    same("pitch_path H-index", got, {"path": canon["path"]})
    if np.all(st == 0):
        ins_ns = {n: s for n, s in ins8.items() if n != "status"}
        got, _ = arena_call(vb, f"pitch_path H-status k{kmax} F{F}", ins_ns, {n: (dt, r, c, ld, min_res(dt)) for n, (dt, r, c, ld, _) in outs.items()}, call)
        same("pitch_path H-status", got, canon)


def test_sinc_and_extremum_points(vb, oracle, speech):
    """vbx_interpolate_sinc_f64 / vbx_improve_extremum_f64 / _ex_f64 on one lag curve: y, the query points and the outputs at 8 mod
    16, status at 4 mod 16 (the inputs of tests/test_gpu_parity.py::test_interpolate_sinc_points / test_improve_extremum_points)."""
    N = 1200
    x = speech[1000:1000 + N] * oracle.window("hanning", N)
    r = oracle.normalize(oracle.autocorrelate(x, N)) / oracle.window("hanning_lag", N)
    y = np.concatenate([r, np.zeros(N)])
    b = N // 2
    offset, nx = -b - 1, 2 * b + 1
    rng = np.random.default_rng(1)
    xs = np.concatenate([rng.uniform(b + 2, 2 * b, 300), [b + 101.0, -1.0, nx + 5.0, b + 1.5]])
    m = xs.size
    canon = _run_rows(vb, "interpolate_sinc", {"y": (y, 0), "xs": (xs, 0)}, {"out": (f64, m, 1, None, 0), "status": (i32, m, 1, None, 0)},
                      ("y", "xs"), lambda a: vb.L.vbx_interpolate_sinc_f64(vb.ctx, a["y"], y.size, offset, nx, a["xs"], m, 30, a["out"], a["status"]),
                      {"sinc_points"})
    for i, xv in enumerate(xs):
        es, ev = oracle.interpolate_sinc(y, offset, nx, xv, 30)
        assert canon["status"][i, 0] == es and abs(canon["out"][i, 0] - ev) <= 1e-9 * max(1.0, abs(ev)), (xv, canon["out"][i], ev)
    peaks = [k for k in range(1, b - 1) if y[k - 1] < y[k] > y[k + 1] and 80 < k < 590]
    assert peaks
    ix = np.array([k + 0.01 * ((k * 7) % 10) - offset for k in peaks] + [0.0, float(nx), nx + 3.0])
    m2 = ix.size
    outs = {"xy": (f64, m2, 2, None, 0), "status": (i32, m2, 1, None, 0)}
    canon = _run_rows(vb, "improve_extremum", {"y": (y, 0), "ixmid": (ix, 0)}, outs, ("y", "ixmid"),
                      lambda a: vb.L.vbx_improve_extremum_f64(vb.ctx, a["y"], y.size, offset, nx, a["ixmid"], m2, 1200, a["xy"], a["status"]),
                      {"extremum_points"})
    for i, v in enumerate(ix):
        es, ex, ey = oracle.improve_extremum_sinc(y, offset, nx, v, 1200)
        assert canon["status"][i, 0] == es
        assert abs(canon["xy"][i, 0] - ex) <= 1e-6 * max(1.0, abs(ex)) and abs(canon["xy"][i, 1] - ey) <= 1e-6 * max(1.0, abs(ey)), (v, canon["xy"][i])
    canon_p = _run_rows(vb, "improve_extremum_ex parabolic", {"y": (y, 0), "ixmid": (ix, 0)}, outs, ("y", "ixmid"),
                        lambda a: vb.L.vbx_improve_extremum_ex_f64(vb.ctx, a["y"], y.size, offset, nx, a["ixmid"], m2, 1, 0, 1, a["xy"], a["status"]),
                        {"extremum_points"})
    for i, v in enumerate(ix):
        es, ex, ey = oracle.improve_extremum(y, offset, nx, v, 1, 0, True)
        assert canon_p["status"][i, 0] == es
        if es == 0:
            assert abs(canon_p["xy"][i, 0] - ex) <= 1e-14 * max(1.0, abs(ex)) and abs(canon_p["xy"][i, 1] - ey) <= 1e-14 * max(1.0, abs(ey))


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 100003])
def test_synth_speech_output(vb, pkg, n):
    """vbx_synth_speech_f64 writes n samples at out, at 0 and at 8 mod 16, and nothing beside them."""
    canon = None
    for res in (0, 8):
        vb.profile_reset()
        got, _ = arena_call(vb, f"synth_speech n={n} out%16={res}", {}, {"out": (f64, 1, n, None, res)},
                            lambda a: vb.L.vbx_synth_speech_f64(vb.ctx, a["out"], n, 48000 * 3 + 17, SR, 0x5EED0001))
        la.assert_written("synth_speech", "out", got["out"])
        if canon is None:
            canon = got
            assert "synth" in vb.profile_report()
            host = importlib.import_module(pkg.__name__ + ".synth").synth_speech(n, 48000 * 3 + 17)
            assert np.max(np.abs(host - got["out"][0])) < 1e-9
        else:
            same("synth_speech out at 8 mod 16", got, canon)


@pytest.mark.parametrize("n", [1, 2, 7, 4096, 4097, 100003])
def test_pcm16_to_f64(vb, speech, n):
    """vbx_pcm16_to_f64: pcm at 2 mod 4, out at 8 mod 16 (both sides of k_front.hip's `aligned`), odd and even counts."""
    pcm = np.round(speech[:n] * 30000.0).astype(i16)
    canon = None
    for tag, pres, ores in (("canonical", 0, 0), ("A", 2, 0), ("C", 0, 8), ("F", 2, 8), ("A6", 6, 0)):
        vb.profile_reset()
        got, addr = arena_call(vb, f"pcm16_to_f64 n={n} {tag}", {"pcm": (pcm, pres)}, {"out": (f64, 1, n, None, ores)},
                               lambda a: vb.L.vbx_pcm16_to_f64(vb.ctx, a["pcm"], n, a["out"]))
        note_branch(("k_front.hip:aligned",), x=addr["pcm"], out=addr["out"])
        if canon is None:
            canon = got
            kernels_ran(vb, f"pcm16-{n}", {"pcm16"})
            assert np.array_equal(got["out"][0], pcm.astype(f64) / 32767.0)
        else:
            same(f"pcm16_to_f64 {tag}", got, canon)


@pytest.mark.parametrize("F", [1, 2, 3, F_PRIME])
def test_ring_frames(vb, speech, F):
    """vbx_ring_frames_f64: the ring at 8 mod 16, out at 8 mod 16, a view that wraps around the ring's end, odd stride."""
    N, stride = 512, 161
    cap = (F - 1) * stride + N
    head = cap - 37
    ring = np.ascontiguousarray(speech[100:100 + cap])
    want = np.stack([ring[(head + t * stride + np.arange(N)) % cap] for t in range(F)])
    for tag, rres, ores in (("canonical", 0, 0), ("A", 8, 0), ("C", 0, 8), ("F", 8, 8)):
        vb.profile_reset()
        got, _ = arena_call(vb, f"ring_frames F={F} {tag}", {"ring": (ring, rres)}, {"out": (f64, F, N, None, ores)},
                            lambda a: vb.L.vbx_ring_frames_f64(vb.ctx, a["ring"], cap, head, F, N, stride, a["out"]))
        assert "ring_frames" in vb.profile_report()
        same(f"ring_frames {tag}", got, {"out": want})


@pytest.mark.parametrize("res", [0, 8])
def test_in_place_forms_the_header_allows(vb, oracle, speech, res):
    """vbx_preemphasis_f64 with out == x on a dense batch, vbx_normalize_f64 in place, inside an arena."""
    F, N = 19, 1200
    fr = la.windows(speech, N, 480, F).copy()
    got, _ = arena_call(vb, f"preemphasis in place x%16={res}", {"x": (fr, res, True)}, {},
                        lambda a: vb.L.vbx_preemphasis_f64(vb.ctx, a["x"], F, N, N, 0.1, a["x"]))
    for f in range(F):
        assert np.all(rel_close(got["x"][f], oracle.preemphasis(fr[f], 0.1), 1e-12)), f
    sep, _ = arena_call(vb, f"preemphasis separate x%16={res}", {"x": (fr, res)}, {"out": (f64, F, N, None, res)},
                        lambda a: vb.L.vbx_preemphasis_f64(vb.ctx, a["x"], F, N, N, 0.1, a["out"]))
    la.assert_same_bits("preemphasis in place == separate", "x", got["x"], sep["out"])
    got, _ = arena_call(vb, f"normalize in place data%16={res}", {"data": (fr, res, True)}, {},
                        lambda a: vb.L.vbx_normalize_f64(vb.ctx, a["data"], F, N))
    for f in range(F):
        assert np.all(rel_close(got["data"][f], oracle.normalize(fr[f]), 1e-14)), f


def test_zz_report(vb):
    """Both sides of every alignment branch were reached (computed per case from its addresses and stride with the predicates in
    BRANCHES); the report of the run, kept as a file when VBX_TEST_REPORT_DIR is set (profiles/layouts/report.json is one)."""
    REPORT["wall_seconds"] = round(time.time() - (_T0[0] or time.time()), 1)
    print("\nlayout matrix:", json.dumps({k: REPORT[k] for k in ("cases", "branch_sides", "wall_seconds")}))
    out = os.environ.get("VBX_TEST_REPORT_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "layouts_report.json"), "w") as fh:
            json.dump(REPORT, fh, indent=1, sort_keys=True)
    if REPORT.get("ops_run", 0) < len(_op_ids()) or "pcm16-100003" not in REPORT["kernels_seen"]:
        return                                               # a selection of the file (-k, --lf): the counts below are of the whole file
    for name in BRANCHES:
        sides = REPORT["branch_sides"].get(name, {})
        assert sides.get("vector", 0) > 0 and sides.get("fallback", 0) > 0, (name, sides)
