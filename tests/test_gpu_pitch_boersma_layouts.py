"""vbx_pitch_boersma_f64 in fenced arenas (tests/layout_arena.py): odd bases for x, window, out_cand and out_count, odd strides,
a gapped view whose gaps hold NaN.  Every layout must equal the aligned dense call bit for bit, touch no canary and use no
sample outside its frames."""
import numpy as np
import pytest

import layout_arena as la

pytestmark = pytest.mark.gpu

SR = 48000.0
TH, FMIN, FMAX = 0.2, 75.0, 600.0
F = 37


def _call(vb, label, frames_1d, N, S, window, kmax, rx=0, rw=0, rc=0, rn=0, rs=0, fmax=FMAX, status=True):
    a = la.Arena(la.DeviceBackend(vb), label)
    a.input("x", frames_1d, residue=rx)
    if window is not None:
        a.input("window", window, residue=rw)
    a.output("cand", np.float64, F, 2 * kmax, residue=rc)
    a.output("count", np.int32, F, 1, residue=rn)
    if status:
        a.output("status", np.int32, F, 1, residue=rs)
    a.place()
    rc_ = vb.L.vbx_pitch_boersma_f64(vb.ctx, a["x"], F, N, S, a["window"] if window is not None else None, SR, TH, FMIN, fmax, kmax,
                                     a["cand"], a["count"], a["status"] if status else None)
    assert rc_ == 0, (label, vb.last_error() if hasattr(vb, "last_error") else rc_)
    return a.finish()


def _same(label, got, canon):
    for nm in got:
        la.assert_no_new_nan(label, nm, got[nm], canon[nm])
        la.assert_same_bits(label, nm, got[nm], canon[nm])


@pytest.fixture(scope="module")
def speech(vb):
    d = vb.synth_speech(F * 1500 + 4096, sample_offset=48000)
    x = d.numpy()
    d.free()
    return x


@pytest.mark.parametrize("N,hop,kmax,use_win,fmax", [(1200, 480, 4, True, FMAX), (1281, 401, 15, True, FMAX), (64, 33, 2, False, 30000.0)])
def test_layouts_equal_the_aligned_dense_call(vb, pkg, speech, N, hop, kmax, use_win, fmax):
    sig = speech[:(F - 1) * hop + N]
    dense = la.windows(sig, N, hop, F)
    win = pkg.window_table(pkg.WINDOW_HANNING, N) if use_win else None
    canon = _call(vb, f"canonical N={N}", dense.reshape(-1), N, N, win, kmax, fmax=fmax)
    for nm in canon:
        la.assert_written("canonical", nm, canon[nm])
    assert np.all(canon["status"] == 0) and np.all(canon["count"] >= 1)
    # the hop-strided view, every base odd
    _same("view odd bases", _call(vb, "view odd bases", sig, N, hop, win, kmax, rx=8, rw=8, rc=8, rn=4, rs=12, fmax=fmax), canon)
    _same("view x%16=0 cand%16=8", _call(vb, "view", sig, N, hop, win, kmax, rx=0, rw=8, rc=8, rn=12, rs=4, fmax=fmax), canon)
    # odd strides above the frame length: the gaps hold NaN, a sample used outside a frame shows up in the output
    for S in (N + 1, N + 7):
        gv = la.gapped_view(dense, S)
        _same(f"gapped S={S}", _call(vb, f"gapped S={S}", gv, N, S, win, kmax, rx=8, rc=8, rn=8, rs=8, fmax=fmax), canon)
    # status NULL
    got = _call(vb, "status NULL", dense.reshape(-1), N, N, win, kmax, rx=8, rc=8, rn=4, fmax=fmax, status=False)
    _same("status NULL", got, {k: canon[k] for k in got})
