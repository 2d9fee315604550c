"""Diagnostic: compare the gfx950 device assembly of the working tree with that of another
git revision, kernel by kernel -- the check of a source change that should not change code.
Each .hip unit (default: all of build.SOURCES) and the headers at REV go to a temporary
directory (build_rev.checkout); both sides compile with build.FLAGS + --cuda-device-only -S.
The assembly is split per function symbol (body and kernel descriptor), comments and the
.file / .loc / .ident lines are stripped, block labels lose their function index, and the
texts are compared.  One line per kernel:
  same|DIFF | instructions rev | new | vgpr rev | new | scratch rev | new | symbol
Text comparison only.  Exit status 1 if any kernel differs or exists on one side only.
usage: asm_diff.py REV [unit ...]      (unit: sdhip_vit.hip)"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

from build_rev import checkout  # puts the repository root on sys.path
from scenedino_amd import build as b


def assemble(job):
    src, out = job
    subprocess.run([b.hipcc()] + b.FLAGS + ["--cuda-device-only", "-S", "-w", "-o", out, src], check=True,
                   cwd=os.path.dirname(out))


def kernels(path):
    """{symbol: (text lines, instructions, vgprs, scratch bytes)} of one assembly file."""
    out, sym, body = {}, None, []
    if not os.path.exists(path):
        return out
    for raw in open(path):
        line = raw.split(";", 1)[0].strip()
        m = re.match(r"\.type\s+(\S+),@function", line)
        if m:
            sym, body = m.group(1), []
        elif sym is None or not line or re.match(r"\.(file|loc|ident)\b", line):
            pass
        elif line.startswith(".size") and line.split()[1].rstrip(",") == sym:
            field = lambda name: next((l.split()[1] for l in body if l.startswith(name + " ")), "-")  # noqa: E731
            ninst = sum(1 for l in body if not l.startswith(".") and not l.endswith(":"))
            out[sym] = (body, ninst, field(".amdhsa_next_free_vgpr"), field(".amdhsa_private_segment_fixed_size"))
            sym = None
        else:
            body.append(re.sub(r"\.L(BB|func_end|func_begin)\d+", r".L\1", line))
    return out


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    rev, want = sys.argv[1], {os.path.basename(a) for a in sys.argv[2:]}
    units = [u for u in b.SOURCES if not want or os.path.basename(u) in want]
    if want and len(units) != len(want):
        sys.exit("unknown unit among: " + " ".join(sorted(want)))
    ndiff = 0
    with tempfile.TemporaryDirectory(prefix="sdasm_") as tmp:
        old_root = checkout(rev, os.path.join(tmp, "rev"))
        asm = lambda u, side: os.path.join(tmp, f"{os.path.basename(u)}.{side}.s")  # noqa: E731
        jobs = [(os.path.join(old_root, u), asm(u, "rev")) for u in units if os.path.exists(os.path.join(old_root, u))]
        jobs += [(os.path.join(b.HERE, u), asm(u, "new")) for u in units]
        jobs.sort(key=lambda j: -os.path.getsize(j[0]))  # the largest units first
        with ThreadPoolExecutor(min(16, len(jobs))) as ex:
            list(ex.map(assemble, jobs))
        print(f"# device assembly, {rev} | working tree; build.py flags + --cuda-device-only -S\n"
              "# same/DIFF | instructions rev | new | VGPRs rev | new | scratch bytes rev | new | symbol")
        for u in units:
            old, new = kernels(asm(u, "rev")), kernels(asm(u, "new"))
            rows, bad = [], 0
            for s in sorted(set(old) | set(new)):
                if s not in old or s not in new:
                    rows.append(f"DIFF | only in {'new' if s in new else 'rev'} | {s}")
                    bad += 1
                    continue
                o, n = old[s], new[s]
                bad += o[0] != n[0]
                rows.append(f"{'same' if o[0] == n[0] else 'DIFF'} | {o[1]} | {n[1]} | vgpr {o[2]} | {n[2]} | "
                            f"scratch {o[3]} | {n[3]} | {s}")
            print(f"# {os.path.basename(u)}: {len(old)} kernels at rev, {len(new)} new, {bad} differ")
            print("\n".join(rows))
            ndiff += bad
    print(f"# total: {ndiff} differ")
    return 1 if ndiff else 0


if __name__ == "__main__":
    sys.exit(main())
