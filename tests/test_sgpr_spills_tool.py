"""tools/experiments/sgpr_spills.py on a hand-written kernel: an entry block that stores two scalar registers into lanes of v40
(one loaded from the argument block, one a literal), a loop of two blocks with one reload each, and a tail without any."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ASM = """
\t.type\ttoy_kernel,@function
toy_kernel:
; %bb.0:
\ts_load_dwordx2 s[4:5], s[0:1], 0x18
\ts_mov_b32 s6, 0x54442d18
\ts_waitcnt lgkmcnt(0)
                                        ; implicit-def: $vgpr40 : SGPR spill to VGPR lane
\tv_writelane_b32 v40, s5, 0
\tv_writelane_b32 v40, s6, 1
\ts_mov_b32 s7, 0
.LBB0_1:
\tv_readlane_b32 s8, v40, 0
\ts_add_i32 s7, s7, s8
\ts_cmp_lt_i32 s7, 64
\ts_cbranch_scc0 .LBB0_3
; %bb.2:
\tv_readlane_b32 s9, v40, 1
\tv_readlane_b32 s10, v3, 0
\ts_branch .LBB0_1
.LBB0_3:
\ts_endpgm
.Lfunc_end0:
\t.size\ttoy_kernel, .Lfunc_end0-toy_kernel
\t.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           32
        .value_kind:     by_value
    .name:           toy_kernel
    .private_segment_fixed_size: 0
    .sgpr_count:     12
    .sgpr_spill_count: 2
    .vgpr_count:     41
    .vgpr_spill_count: 0
...
\t.end_amdgpu_metadata
"""


def _tool():
    spec = importlib.util.spec_from_file_location("sgpr_spills", os.path.join(ROOT, "tools", "experiments", "sgpr_spills.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_blocks_loop_depth_and_traced_values():
    t = _tool()
    lines = ASM.split("\n")
    assert list(t.function_bodies(lines)) == ["toy_kernel"]
    rep = t.analyse(lines, "toy_kernel", trips={".LBB0_1": 10.0})
    assert rep["spill_vgprs"] == [40]                            # v3's lane read is the kernel's own, not a reload
    assert rep["loops"] == 1 and rep["loop_headers"] == {".LBB0_1": 2}
    rows = {r["block"]: r for r in rep["rows"]}
    assert set(rows) == {"%bb.0", ".LBB0_1", "%bb.2"}            # the tail has no access and no row
    assert (rows["%bb.0"]["stores"], rows["%bb.0"]["reloads"], rows["%bb.0"]["depth"]) == (2, 0, 0)
    assert rows["%bb.0"]["stored"] == ["const 0x54442d18", "kernarg+0x1c"]
    assert (rows[".LBB0_1"]["stores"], rows[".LBB0_1"]["reloads"], rows[".LBB0_1"]["depth"], rows[".LBB0_1"]["header"]) == (0, 1, 1, ".LBB0_1")
    assert rows[".LBB0_1"]["values"] == ["kernarg+0x1c"]
    assert (rows["%bb.2"]["reloads"], rows["%bb.2"]["depth"], rows["%bb.2"]["header"]) == (1, 1, ".LBB0_1")
    assert rows["%bb.2"]["values"] == ["const 0x54442d18"]
    tot = rep["totals"]
    assert (tot["stores"], tot["reloads"], tot["stores_in_loops"], tot["reloads_in_loops"]) == (2, 2, 0, 2)
    assert tot["weighted"] == 2 + 10.0 * 2                       # the entry's stores once, the loop's reloads ten times
    assert rep["meta"][".sgpr_spill_count"] == "2" and rep["meta"][".vgpr_count"] == "41" and rep["meta"][".sgpr_count"] == "12"
    assert rep["instructions"] == 14
