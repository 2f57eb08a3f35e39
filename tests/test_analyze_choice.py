"""choose_analyze (csrc/k_spectral.hip, csrc/vbx_spectral_pow2.hpp) through vbx_internal_analyze_choice: which instance of the fused
analysis kernel a launch takes, decided in one place.  No GPU: the probe makes no HIP call.

The expected values are NOT this code's: tests/golden/analyze_choice_named.txt is what the launcher of the tree before choose_analyze
existed launched for the same descriptions (a recording build, tools/analyze_choice/), kernel symbol, dynamic LDS and batching."""
import itertools

import pytest

from analyze_choice_cases import (FAMILY_1200, FAMILY_F32IN, FAMILY_POW2, SP_ANALYZE, SP_ANALYZE_INTERP, SP_ANALYZE_INTERP_SPLIT,
                                  SP_ANALYZE_SPLIT, SP_MFCC_HALF, SP_MFCC_ONLY, named_launches, probe, probe_kw)

NAMED = named_launches()


@pytest.mark.parametrize("case", NAMED, ids=[c[0] for c in NAMED])
def test_the_choice_is_what_the_launcher_launched_before(pkg, case):
    name, ints, doubles, F, want = case
    got = probe(pkg, ints, doubles)
    assert got is not None
    assert {k: got[k] for k in want} == want, name
    if not got["refused"]:
        split = got["mode"] in (SP_ANALYZE_SPLIT, SP_ANALYZE_INTERP_SPLIT)
        assert split == (got["per_launch"] > 0)
        assert got["burg"] == 0 or got["burg_fusable"] == 1


def test_the_named_launches_cover_the_forms():
    """What the fixture must hold (one of each): the recorded launches say so themselves."""
    by = {c[0]: c[4] for c in NAMED}
    assert len(by) >= 30
    assert by["headline_f64"] == dict(by["headline_f64"], family=FAMILY_1200, spec=1, waves=3, lpc=1, mf=1, full=1, mode=SP_ANALYZE)
    assert by["headline_pcm16"]["spec"] == 2 and by["headline_f32"]["family"] == FAMILY_F32IN
    assert by["coeffs20_generic"]["spec"] == 0 and by["coeffs20_generic"]["waves"] == 3
    assert by["whole_vec_parked"]["waves"] == 3 and by["whole_vec_base8_lds"]["waves"] == 2
    assert by["whole_vec_base8_lds"]["lds"] > by["whole_vec_parked"]["lds"]
    assert by["n1103_interp"]["mode"] == SP_ANALYZE_INTERP and by["n1103_interp"]["full"] == 0
    assert by["n1024"]["family"] == by["n512"]["family"] == by["n2048"]["family"] == FAMILY_POW2 and by["n512"]["full"] == 0
    assert by["n4096_split"]["mode"] == SP_ANALYZE_SPLIT and by["n4096_split"]["per_launch"] >= 1024
    assert by["n4096_fused_no_scratch"]["mode"] == by["n4096_fused_small_scratch"]["mode"] == SP_ANALYZE
    assert by["n3001_odd_split"]["mode"] == SP_ANALYZE_SPLIT and by["n3000_interp_split"]["mode"] == SP_ANALYZE_INTERP_SPLIT
    assert by["mfcc_only_2400_half"]["mode"] == SP_MFCC_ONLY and by["mfcc_only_4096_half"]["mode"] == SP_MFCC_HALF
    assert by["burg_f64"]["burg"] == 1 and by["burg_f64"]["spec"] == 1 and by["burg_pcm16"]["spec"] == 2
    for refused in ("burg_refused_pcm16_mfcc_no_lpc", "burg_refused_generic", "burg_refused_f32", "pcm16_refused_not_1200"):
        assert by[refused]["refused"] == 1


def test_a_burg_request_agrees_with_spectral_burg_fusable_over_the_grid(pkg):
    """spectral_burg_fusable(L) is the choice's own answer to L with a BURG request: over the probe's whole grid, asking with BURG
    requested is refused exactly where it says no -- and a launch-specialised instance is what it says yes to."""
    asked = 0
    for n, kind, (lpc, coeffs), defer, kmax, aligned, allow_spec, lag_rcp, mode in itertools.product(
            (512, 1024, 1103, 1199, 1200, 2048, 4096), (0, 1, 2), ((0, 0), (1, 0), (0, 13), (1, 13), (1, 20)), (0, 1), (1, 4, 64, 65, 302), (0, 1),
            (0, 1), (0, 1), (0, 1, 2)):
        if (defer and not coeffs) or (mode == 1 and not coeffs) or (mode == 2 and coeffs):
            continue
        kw = dict(n=n, kind=kind, lpc=lpc, coeffs=coeffs, nb=n // 6, b_lo=2, defer=defer, kmax=kmax, aligned=aligned, allow_spec=allow_spec,
                  lag_rcp=lag_rcp, mode=mode, n_lags=n if mode == 2 else 0)
        plain, burg = probe_kw(pkg, **kw), probe_kw(pkg, burg=1, **kw)
        assert plain is not None and burg is not None, kw
        asked += 1
        assert plain["burg_fusable"] == burg["burg_fusable"] == 1 - burg["refused"], kw
        if not burg["refused"]:
            assert burg["burg"] == 1 and burg["spec"] in (1, 2) and burg["spec"] == plain["spec"] and burg["waves"] == 3, kw
            assert {k: burg[k] for k in ("family", "lpc", "mf", "full", "mode", "lds")} == {k: plain[k] for k in ("family", "lpc", "mf", "full", "mode", "lds")}, kw
        else:
            # refused: no launch-specialised instance, or the one form that has no BURG instance (PCM frames, MFCC without LPC)
            assert plain["refused"] or plain["spec"] == 0 or (plain["spec"] == 2 and plain["mf"] and not plain["lpc"]), kw
    assert asked > 5000
