"""vbx_internal_analyze_choice (what choose_analyze answers for a launch given in plain numbers; no GPU) and the recorded launches of
tests/golden/analyze_choice_named.txt: the head of the transcript tools/analyze_choice/driver.cpp printed in a recording build of the
tree BEFORE choose_analyze existed -- what launch_analyze launched then, kernel symbol by kernel symbol."""
import ctypes as C
import os
import re

import numpy as np

OUT_FIELDS = ("refused", "family", "plan", "lpc", "mf", "full", "mode", "waves", "sample", "spec", "burg", "list", "full_off", "lds", "lds_scan",
              "lds_refine", "ncurve", "reach", "cand_cap", "row_doubles", "list_ints", "per_launch", "split_row_bytes", "burg_fusable")
IN_FIELDS = ("n", "kind", "kmax", "lpc", "coeffs", "nb", "b_lo", "interp", "defer", "allow_spec", "lag_rcp", "whole_curve", "aligned", "ld_odd", "mode",
             "n_lags", "scratch", "burg")
FAMILY_1200, FAMILY_F32IN, FAMILY_POW2 = 0, 1, 2
SP_ANALYZE, SP_MFCC_ONLY, SP_AC_ONLY, SP_MFCC_HALF, SP_ANALYZE_INTERP, SP_ANALYZE_SPLIT, SP_ANALYZE_INTERP_SPLIT, SP_MFCC_ONLY_INTERP = range(8)


def probe(pkg, ints, doubles):
    """-> dict of OUT_FIELDS, or None where the probe refuses the description (a shape with no form of the interpolation tables)."""
    fn = pkg.load_library().vbx_internal_analyze_choice
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]
    ip = np.ascontiguousarray(ints, dtype=np.int64)
    dp = np.ascontiguousarray(doubles, dtype=np.float64)
    assert ip.size == len(IN_FIELDS) and dp.size == 2
    out = np.zeros(len(OUT_FIELDS), dtype=np.int64)
    if fn(ip.ctypes.data, dp.ctypes.data, out.ctypes.data) != 0:
        return None
    return dict(zip(OUT_FIELDS, (int(v) for v in out)))


def probe_kw(pkg, sample_rate=48000.0, fmin=75.0, **kw):
    d = dict(n=1200, kind=0, kmax=4, lpc=0, coeffs=0, nb=0, b_lo=0, interp=0, defer=0, allow_spec=1, lag_rcp=1, whole_curve=0, aligned=1, ld_odd=0,
             mode=0, n_lags=0, scratch=0, burg=0)
    assert set(kw) <= set(d), set(kw) - set(d)
    d.update(kw)
    return probe(pkg, [d[k] for k in IN_FIELDS], [sample_rate, fmin])


_KERNEL = re.compile(r"launch (?:void )?vbx::(\w+)(?:<([^<>]*)>)?\(")
_GEOMETRY = re.compile(r" grid=(\d+),1,1 block=(\d+),1,1 lds=(\d+) args=")
_TIN = {"double": (0, 0, 0), "float": (0, 0, 1), "vbx::sp_launch_f64_t": (1, 0, 0), "vbx::sp_launch_pcm16_t": (2, 0, 0),
        "vbx::sp_launch_f64_burg_t": (1, 1, 0), "vbx::sp_launch_pcm16_burg_t": (2, 1, 0)}      # -> (spec, burg, float32 unit)


def named_launches():
    """[(name, ints, doubles, F, expected)]: expected = the OUT_FIELDS the recorded launch pins down."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "analyze_choice_named.txt")
    cases, cur = [], None
    for line in open(path):
        if line.startswith("call "):
            m = re.match(r"call (\S+) in=([-\d,]+);(\S+),(\S+) F=(\d+) plan=(\d+) burg=(\d+)", line)
            cur = {"name": m.group(1), "ints": [int(v) for v in m.group(2).split(",")], "doubles": [float(m.group(3)), float(m.group(4))],
                   "F": int(m.group(5)), "plan": int(m.group(6)), "launches": [], "result": None}
            cases.append(cur)
        elif line.startswith("  launch "):
            m, g = _KERNEL.search(line), _GEOMETRY.search(line)
            assert m and g, line
            cur["launches"].append((m.group(1), m.group(2), int(g.group(1)), int(g.group(2)), int(g.group(3))))
        elif line.startswith("  result "):
            m = re.match(r"  result (\w+) spec=(\d+) batches=(\d+) per=(\d+)", line)
            cur["result"] = (m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)))
    out = []
    for c in cases:
        what, spec, batches, per = c["result"]
        exp = {"refused": int(what == "refused"), "sample": c["ints"][1], "burg": c["ints"][17]}
        if what != "refused":
            kernel, targs, grid, block, lds = c["launches"][0]
            t = [v.strip() for v in targs.split(",")]
            b = lambda v: int(v == "true")
            if kernel == "analyze_kernel":
                tin_spec, tin_burg, f32 = _TIN[t[5]]
                exp.update(family=FAMILY_F32IN if f32 else FAMILY_1200, lpc=b(t[0]), mf=b(t[1]), full=b(t[2]), mode=int(t[3]), waves=int(t[4]),
                           spec=tin_spec, burg=tin_burg, lds=lds)
                assert tin_spec == spec and block == 64
            else:
                assert kernel == "analyze_pow2_kernel"
                exp.update(family=FAMILY_POW2, lpc=b(t[1]), mf=b(t[2]), full=b(t[3]), mode=int(t[4]), spec=0, lds=lds)
            exp["plan"] = c["plan"]
            exp["per_launch"] = per
            if what == "split":
                names = [l[0] for l in c["launches"]]
                assert names == ["analyze_pow2_kernel", "scan_curve_kernel", "refine_list_kernel", "refine_far_kernel"] * batches
                assert batches == -(-c["F"] // per) and grid == min(per, c["F"])
                exp.update(lds_refine=c["launches"][2][4], lds_scan=c["launches"][3][4])
            else:
                assert len(c["launches"]) == 1 and grid == c["F"] - (7 if exp["burg"] else 0)
        out.append((c["name"], c["ints"], c["doubles"], c["F"], exp))
    return out
