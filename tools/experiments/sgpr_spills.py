#!/usr/bin/env python3
"""Where a kernel instance spills scalar registers into vector lanes, counted from its assembly (CPU only; nothing runs on a GPU).

The compiler keeps an SGPR it has no room for in one lane of a reserved VGPR: the store is a v_writelane_b32 into that VGPR, the
reload a v_readlane_b32 from it.  Both are vector instructions.  This tool reads the device assembly of one translation unit

    hipcc <the Makefile's flags> --cuda-device-only -S csrc/k_spectral.hip -o k_spectral.s        (or the .s of --save-temps)

and prints, for one kernel instance, every basic block that holds such an access: its spill stores and reloads, its loop depth
(natural loops of the block graph: dominators, back edges), the header of its innermost loop, and per access the value the lane
holds where that can be traced in the block graph's layout: the s_load of the kernel argument block it came from (byte offset),
an s_mov of a literal, or the instruction that last wrote the register.  Per instance it prints the code object metadata's
sgpr_count, sgpr_spill_count, vgpr_count and scratch bytes.

Executed counts are static counts times trip counts, and the trip counts are not in the assembly: --trips HEADER=N[,HEADER=N...]
gives the passes per frame of the loop whose header is that label (from the device work counters, the -DVBX_EXP_STOP builds'
counter differences, or brent_cells.py); a block's weight is the product over the loops around it, a loop without a figure
counts once.  Blocks outside every loop run at most once per frame, so their total is an upper bound.

usage: sgpr_spills.py k_spectral.s --list
       sgpr_spills.py k_spectral.s --kernel 'analyze_kernelILb1ELb1ELb1ELi0ELi3Ed' [--trips .LBB16_40=11,...] [--blocks]
"""
import argparse
import re
import sys

LABEL = re.compile(r"^([.\w$]+):")
BB_COMMENT = re.compile(r"^; %bb\.(\d+):")
SPILL_DEF = re.compile(r"implicit-def: \$vgpr(\d+) : SGPR spill to VGPR lane")
WRITELANE = re.compile(r"^v_writelane_b32\s+v(\d+),\s*(\S+?),\s*(\d+)")
READLANE = re.compile(r"^v_readlane_b32\s+(s\d+|vcc_lo|vcc_hi),\s*v(\d+),\s*(\d+)")
BRANCH = re.compile(r"^(s_branch|s_cbranch_\w+)\s+([.\w$]+)")
ENDS = ("s_endpgm", "s_setpc_b64", "s_trap")
SREG = re.compile(r"^s(\d+)$")
SRANGE = re.compile(r"^s\[(\d+):(\d+)\]$")


class Block:
    def __init__(self, name, line):
        self.name, self.line = name, line
        self.insts = []                  # (line number, text)
        self.succ = []
        self.stores, self.reloads = [], []   # (line number, lane, sgpr)
        self.depth, self.header = 0, None


def function_bodies(lines):
    """-> {symbol: (first line index, last line index)} of every function in the file"""
    out, cur, start = {}, None, 0
    for i, l in enumerate(lines):
        if cur is None:
            m = LABEL.match(l)
            if m and not m.group(1).startswith(".") and i > 0 and "@function" in lines[i - 1]:
                cur, start = m.group(1), i + 1
        elif l.startswith(".Lfunc_end"):
            out[cur] = (start, i)
            cur = None
    return out


def sgprs_of(operand):
    m = SREG.match(operand)
    if m:
        return [int(m.group(1))]
    m = SRANGE.match(operand)
    if m:
        return list(range(int(m.group(1)), int(m.group(2)) + 1))
    return []


def parse_blocks(lines, first, last):
    """-> (blocks in layout order, spill VGPR numbers)"""
    blocks, spill_regs = [], set()
    cur = Block("entry", first)
    blocks.append(cur)
    for i in range(first, last):
        raw = lines[i]
        m = SPILL_DEF.search(raw)
        if m:
            spill_regs.add(int(m.group(1)))
        text = raw.strip()
        if not text:
            continue
        m = LABEL.match(text)
        mb = BB_COMMENT.match(text)
        if m or mb:
            name = m.group(1) if m else "%bb." + mb.group(1)
            if cur.insts or cur.name != "entry":
                nxt = Block(name, i + 1)
                if not cur.insts or not cur.insts[-1][1].startswith(("s_branch", "s_endpgm", "s_setpc_b64")):
                    cur.succ.append(nxt.name)                        # falls through
                blocks.append(nxt)
                cur = nxt
            else:
                cur.name = name
            continue
        if text.startswith((";", ".")):
            continue
        text = text.split(";")[0].strip()
        if cur.insts and cur.insts[-1][1].startswith("s_cbranch"):   # a conditional branch in mid-block: the block ended there
            nxt = Block("%s+%d" % (cur.name, len(cur.insts)), i + 1)
            cur.succ.append(nxt.name)
            blocks.append(nxt)
            cur = nxt
        cur.insts.append((i + 1, text))
        mbr = BRANCH.match(text)
        if mbr:
            cur.succ.append(mbr.group(2))
    if not spill_regs:                                               # no marker comments (hand-written input): lane writes name them
        for b in blocks:
            for _, t in b.insts:
                m = WRITELANE.match(t)
                if m:
                    spill_regs.add(int(m.group(1)))
    for b in blocks:
        for ln, t in b.insts:
            m = WRITELANE.match(t)
            if m and int(m.group(1)) in spill_regs:
                b.stores.append((ln, int(m.group(3)), m.group(2)))
            m = READLANE.match(t)
            if m and int(m.group(2)) in spill_regs:
                b.reloads.append((ln, int(m.group(3)), m.group(1)))
    return blocks, spill_regs


def loop_depths(blocks):
    """Natural loops: dominators by iteration over bit sets, a back edge u -> h where h dominates u.  Sets depth and header."""
    idx = {b.name: k for k, b in enumerate(blocks)}
    n = len(blocks)
    succ = [[idx[s] for s in b.succ if s in idx] for b in blocks]
    pred = [[] for _ in range(n)]
    for u in range(n):
        for v in succ[u]:
            pred[v].append(u)
    full = (1 << n) - 1
    dom = [full] * n
    dom[0] = 1
    changed = True
    while changed:
        changed = False
        for v in range(1, n):
            d = full
            for p in pred[v]:
                d &= dom[p]
            if not pred[v]:
                d = 0                                                # unreachable
            d |= 1 << v
            if d != dom[v]:
                dom[v] = d
                changed = True
    loops = {}                                                       # header -> set of blocks
    for u in range(n):
        for h in succ[u]:
            if dom[u] >> h & 1:
                body = loops.setdefault(h, {h})
                stack = [u]
                while stack:
                    x = stack.pop()
                    if x in body:
                        continue
                    body.add(x)
                    stack.extend(pred[x])
    for h, body in loops.items():
        for x in body:
            blocks[x].depth += 1
    for k, b in enumerate(blocks):                                   # innermost: the smallest loop that holds the block
        inner = [h for h, body in loops.items() if k in body]
        b.header = blocks[min(inner, key=lambda h: len(loops[h]))].name if inner else None
        b.headers = [blocks[h].name for h in inner]
    return {blocks[h].name: sorted(blocks[x].name for x in body) for h, body in loops.items()}


def origins(blocks):
    """What each spill store put into its lane: walks the layout backwards from the store to the last writer of the SGPR."""
    flat = [(ln, t) for b in blocks for (ln, t) in b.insts]
    pos = {ln: k for k, (ln, _) in enumerate(flat)}
    by_lane = {}                                                     # lane -> [(line, origin)]
    for b in blocks:
        for ln, lane, src in b.stores:
            what = "?"
            regs = sgprs_of(src)
            if regs:
                r = regs[0]
                for k in range(pos[ln] - 1, max(pos[ln] - 4000, -1), -1):
                    t = flat[k][1]
                    parts = t.replace(",", " ").split()
                    if len(parts) < 2 or parts[0].startswith(("s_cmp", "s_cbranch", "s_branch", "s_waitcnt", "s_nop", "s_bitcmp")):
                        continue
                    dst = sgprs_of(parts[1])
                    if r not in dst:
                        continue
                    if parts[0].startswith("s_load_dword") and len(parts) >= 4:
                        try:
                            off = int(parts[3], 0) + 4 * dst.index(r)
                            what = "kernarg+0x%x" % off if parts[2] in ("s[0:1]", "s[4:5]", "s[8:9]") else "load %s+0x%x" % (parts[2], off)
                        except ValueError:
                            what = parts[0]
                    elif parts[0] in ("s_mov_b32", "s_mov_b64", "s_movk_i32") and not parts[2].startswith(("s", "v", "exec", "vcc")):
                        what = "const %s" % parts[2]
                    else:
                        what = parts[0]
                    break
                if what == "?" and r < 16:
                    what = "s%d as the kernel was entered (s[0:1]: the argument segment's address)" % r if r < 2 else "s%d as the kernel was entered" % r
            elif src.startswith(("vcc", "exec")):
                what = src
            by_lane.setdefault(lane, []).append((ln, what))
    return by_lane


def origin_of_reload(by_lane, lane, line):
    w = by_lane.get(lane)
    if not w:
        return "?"
    before = [x for x in w if x[0] < line]
    kinds = sorted({x[1] for x in w})
    pick = max(before)[1] if before else w[0][1]
    return pick if len(kinds) == 1 else "%s (lane reused: %s)" % (pick, ", ".join(kinds))


def metadata(lines, symbol):
    """The entry of `symbol` in the code object metadata (amdhsa.kernels), as a dict of its scalar fields."""
    entries, cur = [], None
    for l in lines:
        s = l.strip()
        if s.startswith("- .") and l.startswith("  - "):
            cur = {}
            entries.append(cur)
            s = s[2:]
        if cur is not None:
            m = re.match(r"^(\.[\w]+):\s*(\S.*)?$", s)
            if m and m.group(2) is not None and not l.startswith("      "):
                cur[m.group(1)] = m.group(2).strip("'\"")
    for e in entries:
        if e.get(".name") == symbol:
            return e
    return {}


def analyse(lines, symbol, trips=None):
    bodies = function_bodies(lines)
    first, last = bodies[symbol]
    blocks, spill_regs = parse_blocks(lines, first, last)
    loops = loop_depths(blocks)
    by_lane = origins(blocks)
    trips = trips or {}
    rep = {"symbol": symbol, "instructions": sum(len(b.insts) for b in blocks), "blocks": len(blocks), "loops": len(loops),
           "spill_vgprs": sorted(spill_regs), "rows": [], "meta": metadata(lines, symbol)}
    tot = {"stores": 0, "reloads": 0, "stores_in_loops": 0, "reloads_in_loops": 0, "weighted": 0.0}
    for b in blocks:
        if not b.stores and not b.reloads:
            continue
        w = 1.0
        for h in getattr(b, "headers", []):
            w *= trips.get(h, 1.0)
        row = {"block": b.name, "line": b.line, "depth": b.depth, "header": b.header, "stores": len(b.stores), "reloads": len(b.reloads),
               "weight": w, "values": sorted({origin_of_reload(by_lane, lane, ln) for ln, lane, _ in b.reloads}),
               "stored": sorted({what for ln, lane, _ in b.stores for (l2, what) in by_lane.get(lane, []) if l2 == ln})}
        rep["rows"].append(row)
        tot["stores"] += len(b.stores); tot["reloads"] += len(b.reloads)
        if b.depth:
            tot["stores_in_loops"] += len(b.stores); tot["reloads_in_loops"] += len(b.reloads)
        tot["weighted"] += w * (len(b.stores) + len(b.reloads))
    rep["totals"] = tot
    rep["loop_headers"] = {h: len(body) for h, body in loops.items()}
    return rep


def print_report(rep, show_blocks=True):
    m, t = rep["meta"], rep["totals"]
    print("kernel %s" % rep["symbol"])
    print("  metadata: sgpr_count %s  sgpr_spill_count %s  vgpr_count %s  vgpr_spill_count %s  scratch %s B  lds %s B" % (
        m.get(".sgpr_count"), m.get(".sgpr_spill_count"), m.get(".vgpr_count"), m.get(".vgpr_spill_count"),
        m.get(".private_segment_fixed_size"), m.get(".group_segment_fixed_size")))
    print("  %d instructions, %d blocks, %d loops, spill VGPRs %s" % (rep["instructions"], rep["blocks"], rep["loops"],
                                                                      ["v%d" % r for r in rep["spill_vgprs"]]))
    print("  spill stores %d (in loops %d, straight-line %d)   reloads %d (in loops %d, straight-line %d)" % (
        t["stores"], t["stores_in_loops"], t["stores"] - t["stores_in_loops"],
        t["reloads"], t["reloads_in_loops"], t["reloads"] - t["reloads_in_loops"]))
    print("  accesses weighted by --trips: %.1f" % t["weighted"])
    if show_blocks:
        print("  %-16s %8s %5s %-14s %6s %7s %8s  values" % ("block", "line", "depth", "loop header", "stores", "reloads", "weight"))
        for r in rep["rows"]:
            vals = "; ".join((["reload: " + ", ".join(r["values"])] if r["values"] else []) + (["store: " + ", ".join(r["stored"])] if r["stored"] else []))
            print("  %-16s %8d %5d %-14s %6d %7d %8.1f  %s" % (r["block"], r["line"], r["depth"], r["header"] or "-", r["stores"], r["reloads"], r["weight"], vals))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm")
    ap.add_argument("--list", action="store_true", help="the kernels of the file with their metadata, and their static spill counts")
    ap.add_argument("--kernel", help="a substring of the instance's (mangled) symbol; it must select one")
    ap.add_argument("--trips", default="", help="HEADER=N,... passes per frame of the loops with these header labels")
    ap.add_argument("--no-blocks", action="store_true")
    a = ap.parse_args(argv)
    with open(a.asm) as fh:
        lines = fh.read().split("\n")
    bodies = function_bodies(lines)
    if a.list or not a.kernel:
        for sym in bodies:
            rep = analyse(lines, sym)
            m, t = rep["meta"], rep["totals"]
            print("%-84s sgpr %4s sspill %4s vgpr %4s scratch %5s | stores %3d reloads %3d (in loops %3d)" % (
                sym[:84], m.get(".sgpr_count"), m.get(".sgpr_spill_count"), m.get(".vgpr_count"), m.get(".private_segment_fixed_size"),
                t["stores"], t["reloads"], t["reloads_in_loops"]))
        return 0
    hits = [s for s in bodies if a.kernel in s]
    if len(hits) != 1:
        print("--kernel selects %d symbols: %s" % (len(hits), hits), file=sys.stderr)
        return 2
    trips = {}
    for kv in filter(None, a.trips.split(",")):
        k, v = kv.split("=")
        trips[k] = float(v)
    print_report(analyse(lines, hits[0], trips), not a.no_blocks)
    return 0


if __name__ == "__main__":
    sys.exit(main())
