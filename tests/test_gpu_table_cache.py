"""The context's cache of host-built device tables (csrc/vbx_table_cache.hpp): the bound on the interpolation tables, and that a table
served from the cache is the table a fresh context builds."""
import numpy as np
import pytest

SR = 48000.0


def _recording(vb, n, hop, F):
    return vb.synth_speech((F - 1) * hop + n)


def _mfcc(pkg, vb, n, F, hi=8000.0):
    hop = 2 * n // 5
    mf, st = vb.mfcc(_recording(vb, n, hop, F), 13, (100.0, hi), SR, frame_len=n, stride=hop, n_frames=F, window=vb.window(pkg.WINDOW_HANNING, n))
    return mf, st


def _primes_from(lo, count):
    out, n = [], lo
    while len(out) < count:
        if all(n % d for d in range(2, int(n ** 0.5) + 1)):
            out.append(n)
        n += 1
    return out


@pytest.mark.gpu
def test_interpolation_tables_are_bounded_and_rebuilt_alike(pkg):
    """66 distinct interpolation tables in one context: more than the 64 the cache keeps of that kind, so the 65th miss drains the
    device and drops them.  The lengths are the first 66 primes from 601 on (601 .. 1039: the range 601 .. 1021 holds only 63): no
    factorisation for the composite kernels, no common divisor with the transform, so vbx_mfcc_f64 interpolates each from the fused
    kernel's transform -- checked on the CPU first through the table builder, then on every call through the probe."""
    import ctypes as C
    lengths = _primes_from(601, 66)
    assert len(set(lengths)) == 66 and lengths[0] == 601 and lengths[-1] == 1039
    fn = pkg.load_library().vbx_internal_mfcc_interp_table
    fn.restype = C.c_int
    fn.argtypes = [C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    keys = set()
    for n in lengths:
        bins, bad = pkg.mfcc_bins(n, 13, 100.0, 8000.0, SR)
        desc, need = (C.c_int32 * 8)(), C.c_size_t(0)
        assert not bad and fn(n, int(bins[0]), int(bins[-1] - bins[0]), desc, None, 0, C.byref(need)) == 1, n
        keys.add((n, int(bins[0]), int(bins[-1] - bins[0])))
    assert len(keys) >= 65
    with pkg.VoxBox(0) as vb:
        first = None
        for n in lengths:
            mf, st = _mfcc(pkg, vb, n, 2)
            assert int(vb.L.vbx_internal_last_mfcc_interp(vb.ctx)) == 1, n
            assert np.all(st == 0) and np.all(np.isfinite(mf)), n
            first = (mf, st) if first is None else first
        again = _mfcc(pkg, vb, lengths[0], 2)                     # its table went with the others: built again
        assert int(vb.L.vbx_internal_last_mfcc_interp(vb.ctx)) == 1
    with pkg.VoxBox(0) as fresh:
        alone = _mfcc(pkg, fresh, lengths[0], 2)
    for a in (again, alone):
        assert a[0].tobytes() == first[0].tobytes() and a[1].tobytes() == first[1].tobytes()


def _call_mfcc(n, hi=8000.0):
    return lambda pkg, vb: _mfcc(pkg, vb, n, 4, hi)


def _call_dct(pkg, vb):
    return (vb.dct(np.random.default_rng(13).standard_normal((4, 13))),)


def _call_resample(ratio):
    return lambda pkg, vb: (vb.resample_linear(_recording(vb, 1200, 480, 4), ratio, frame_len=1200, stride=480, n_frames=4),)


def _call_pitch(n):
    return lambda pkg, vb: vb.pitch(_recording(vb, n, 2 * n // 5, 4), SR, 0.2, 75.0, 600.0, kmax=4, frame_len=n, stride=2 * n // 5, n_frames=4,
                                    window=vb.window(pkg.WINDOW_HANNING, n))


def _call_pitch_f32(pkg, vb):
    x = np.lib.stride_tricks.sliding_window_view(_recording(vb, 1200, 480, 4).numpy(), 1200)[::480][:4].astype(np.float32)
    return vb.pitch_f32(x, SR, 0.2, 75.0, 600.0, kmax=4, window=pkg.window_table(pkg.WINDOW_HANNING, 1200))


def _est0(pkg):
    return np.array([[f, 1.0] for f in pkg.MALE_FORMANT_ESTIMATES])


def _call_formants(pkg, vb):
    ff = vb.find_formants(_recording(vb, 1200, 480, 4), SR, 12, _est0(pkg), frame_len=1200, stride=480, n_frames=4)
    return tuple(ff[k] for k in ("formants", "res", "count", "coeffs", "status"))


def _call_record(n, hop):
    def call(pkg, vb):
        params = pkg.AnalysisParams.make(SR, pitch=(0.2, 75.0, 600.0), lpc_order=12, formant_order=12, est_init=_est0(pkg), mfcc=(13, 100.0, 8000.0))
        return vb.analyze_frames(_recording(vb, n, hop, 4), params, frame_len=n, stride=hop, n_frames=4)
    return call


# one call per kind of table (the shapes of tools/experiments/bitcompare_libs.py --tables); env: read when the context is created
CALLS = {
    "mfcc-337-goertzel": (_call_mfcc(337), None), "mfcc-400-mfma": (_call_mfcc(400), None), "mfcc-1200-fft": (_call_mfcc(1200), None),
    "mfcc-1103-interp": (_call_mfcc(1103), None), "mfcc-1103-czt": (_call_mfcc(1103, 16000.0), None), "mfcc-5000-long": (_call_mfcc(5000), None),
    "mfcc-1200-dft2": (_call_mfcc(1200), ("VBX_MFCC_DFT2", "1")), "mfcc-1103-czt-split": (_call_mfcc(1103, 16000.0), ("VBX_MFCC_CZT_SPLIT", "1")),
    "dct-13": (_call_dct, None), "resample-0.5": (_call_resample(0.5), None), "resample-1.5": (_call_resample(1.5), None),
    "pitch_f32-1200": (_call_pitch_f32, None), "pitch-1200": (_call_pitch(1200), None), "pitch-1024": (_call_pitch(1024), None),
    "find_formants-1200": (_call_formants, None), "record-1200/480": (_call_record(1200, 480), None), "record-1103/441": (_call_record(1103, 441), None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CALLS))
def test_hit_equals_miss(pkg, monkeypatch, name):
    """the first call (every table built), the second call in the same context (every table from the cache) and a call in a fresh
    context return identical bytes"""
    call, env = CALLS[name]
    if env:
        monkeypatch.setenv(*env)
    with pkg.VoxBox(0) as vb:
        miss = call(pkg, vb)
        hit = call(pkg, vb)
    with pkg.VoxBox(0) as fresh:
        alone = call(pkg, fresh)
    assert len(miss) == len(hit) == len(alone) and len(miss) >= 1
    for m, h, a in zip(miss, hit, alone):
        assert np.asarray(m).size > 0
        assert np.asarray(m).tobytes() == np.asarray(h).tobytes() == np.asarray(a).tobytes()
