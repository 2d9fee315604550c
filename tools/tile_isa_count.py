"""Diagnostic: static instruction-category count of k_render_tile's phases from the ISA.

Compiles sdhip_tile.hip with -DST_MARK=1 (asm comments ";@T n" at the phase-timer points
and ";@M n" at the item-loop boundaries, no code of their own) to gfx950 assembly, takes
one kernel instance and counts, per marked region in program order, MFMA / VALU / SALU /
LDS / VMEM / wait instructions.  Static counts: a region inside the item loop runs once per
item, the rest once per step.  The scheduler may move arithmetic across the markers, so the
split is approximate.  usage: tile_isa_count.py [P=2] [ZIN=0] [RPW=2] [LATE=1] [SRC=file]
(the default is the C2 kernel; C1: RPW=2 LATE=0, C4: RPW=1 LATE=0; SRC: another revision's
sdhip_tile.hip, beside its headers)

The "issue" column is the region's vector-issue cycles per wave (the
issue-budget model): a plain VALU instruction holds the SIMD's vector issue 4 cycles, a
transcendental (v_sin / v_exp / v_log / v_rcp / v_rsq / v_sqrt; counted in "trans", a subset
of "valu") 8, an MFMA 8 of its 16.  The "item loop" line sums the item regions (M20-M27): the
budget one item of one wave takes from the issue port its SIMD's two waves share.  The "per
step" line sums every other region of the step loop (M30 .. M39: head, box pass, ray_col,
stage, the ray sums of both rays, output stores, late ray pass, step tail) -- what a wave
issues once per step whatever the item count.  It is a static upper bound: the head is run
by D / 16 of the 8 waves, the box pass by 4 of them, and the split / overflow / frustum-edge
branches are in it with both arms (pair it with SQ_INSTS_VALU of a PMC pass)."""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from scenedino_amd import build as b  # noqa: E402

# ST_T(i) closes phase i (sdhip_tile.hip); ST_M(i) opens an item-loop phase
T_PHASE = {0: "ray_pass (next ray)", 1: "head", 2: "itemA(0)", 3: "ray_col", 4: "barrier X",
           5: "stage + tap_addrs", 6: "item loop", 7: "epilogue", 8: "vmcnt", 9: "barrier Y",
           10: "ray pass: z", 11: "ray pass: geo + colour", 12: "ray pass: box"}
M_PHASE = {20: "item A: records + tap bases", 21: "item A: taps (tr reads + MFMA)",
           22: "item A: positional code (frags + MFMA)", 23: "item A: relu / pack X",
           24: "item A: sigma MFMA, softplus, alpha, scan", 25: "(after item A)",
           26: "item B: weight, depth / colour sums", 27: "item B: hidden-space compositing",
           28: "(after item B)",
           30: "head (waves < D / 16)", 39: "(after the step loop)",
           40: "late pass: split-part geometry", 41: "late pass: z draw, projection, masks",
           42: "late pass: colour taps, verify, tap address", 43: "late pass: record writes, colour",
           44: "late pass: flag, step tail",
           50: "stage: box union", 51: "stage: geometry, split / overflow", 52: "stage: DMA address + issue",
           53: "stage: (after DMA) ray fetch",
           60: "ray sums: 5 row sums", 61: "ray sums: hidden butterfly + store", 62: "(after ray sums)"}


def region_name(start, end):
    """A region between two markers: an M marker names what follows it, a T marker what
    precedes it."""
    if start and start[0] == "M":
        return f"{start}: {M_PHASE.get(int(start[1:]), '')}"
    if end and end[0] == "T":
        return f"{end}: {T_PHASE.get(int(end[1:]), '')}"
    return f"{start or 'entry'}..{end or 'end'}"


def cat(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_waitcnt") or op.startswith("s_barrier") or op.startswith("s_nop"):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "scratch_", "flat_")):
        return "vmem"
    return "other"


TRANS = ("v_sin", "v_cos", "v_exp", "v_log", "v_rcp", "v_rsq", "v_sqrt")
ISSUE = {"valu": 4, "trans": 4, "mfma": 8}  # trans: its 4 cycles on top of the VALU 4


def issue(d):
    return sum(w * d.get(c, 0) for c, w in ISSUE.items())


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    P, ZIN, RPW, LATE = kv.get("P", "2"), kv.get("ZIN", "0"), kv.get("RPW", "2"), kv.get("LATE", "1")
    sym = f"_Z13k_render_tileILi{P}ELb{ZIN}ELi{RPW}ELb{LATE}EEv7st_args:"
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "t.s")
        flags = [f for f in b.FLAGS if not f.startswith("--offload-arch")]
        subprocess.run([b.hipcc(), "--offload-arch=gfx950", "--cuda-device-only", "-S"] + flags +
                       ["-DST_MARK=1", "-o", out,
                        os.path.abspath(kv.get("SRC", os.path.join(b.HERE, "csrc", "sdhip_tile.hip")))],
                       check=True, cwd=td)
        lines = open(out).read().split("\n")
    i0 = next(i for i, l in enumerate(lines) if l.startswith(sym))
    i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith(".Lfunc_end"))
    regs, cur = [], [None, None, {}]
    regs.append(cur)
    for l in lines[i0:i1 + 1]:
        m = re.search(r";@([TM]) (\d+)", l)
        if m:
            cur[1] = m.group(1) + m.group(2)
            cur = [cur[1], None, {}]
            regs.append(cur)
            continue
        t = l.strip()
        if not t or t.startswith((";", ".", "_")) or t.endswith(":"):
            continue
        op = t.split()[0]
        c = cat(op)
        cur[2][c] = cur[2].get(c, 0) + 1
        if op.startswith(TRANS):
            cur[2]["trans"] = cur[2].get("trans", 0) + 1
    cols = ["mfma", "valu", "trans", "salu", "lds", "vmem", "wait", "other"]
    print(f"k_render_tile<P={P}, ZIN={ZIN}, RPW={RPW}, LATE={LATE}>: static instructions per region "
          "(program order)")
    print(f"{'region':48s}" + "".join(f"{c:>7s}" for c in cols) + f"{'issue':>7s}")
    tot, item, step, in_loop = {}, {}, {}, False
    for start, end, d in regs:
        if start == "M30":
            in_loop = True
        elif start == "M39":
            in_loop = False
        if not d:
            continue
        label = region_name(start, end)
        print(f"{label[:48]:48s}" + "".join(f"{d.get(c, 0):7d}" for c in cols) + f"{issue(d):7d}")
        in_item = bool(start) and start[0] == "M" and 20 <= int(start[1:]) <= 27
        for c in cols:
            tot[c] = tot.get(c, 0) + d.get(c, 0)
        if in_item:  # the kernel holds two copies of item A (item 0, items 1..): the last = the loop's
            item[start] = d
        elif in_loop:
            for c in cols:
                step[c] = step.get(c, 0) + d.get(c, 0)
    print(f"{'total':48s}" + "".join(f"{tot.get(c, 0):7d}" for c in cols) + f"{issue(tot):7d}")
    isum = {c: sum(d.get(c, 0) for d in item.values()) for c in cols}
    print(f"{'item loop (M20-M27), per item and wave':48s}" + "".join(f"{isum[c]:7d}" for c in cols) +
          f"{issue(isum):7d}")
    print(f"{'per step (M30..M39 less the items), per wave':48s}" + "".join(f"{step.get(c, 0):7d}" for c in cols) +
          f"{issue(step):7d}")


if __name__ == "__main__":
    main()
