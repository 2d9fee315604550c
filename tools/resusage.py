"""Print VGPR/AGPR/spill/occupancy per kernel of a HIP source (device-only compile).
usage: python tools/resusage.py [file.hip] [extra hipcc flags...]"""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from scenedino_amd import build as b  # noqa: E402

src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(b.HERE, "csrc", "sdhip_field.hip")
cmd = [b.hipcc()] + b.FLAGS + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                               *sys.argv[2:], src, "-o", os.devnull]  # the shipped build's flags
out = subprocess.run(cmd, capture_output=True, text=True).stderr
rows, cur = [], None
for line in out.splitlines():
    m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
    if not m:
        if "error" in line:
            print(line)
        continue
    t = m.group(1).strip()
    if t.startswith("Function Name:"):
        cur = {"name": t.split(":", 1)[1].strip()}
        rows.append(cur)
    elif cur is not None and ":" in t:
        k, v = t.split(":", 1)
        cur[k.strip()] = v.strip()
for r in rows:
    g = r.get
    print(f"{r['name'][:58]:58s} v={g('VGPRs')} a={g('AGPRs')} vspill={g('VGPRs Spill')} "
          f"sspill={g('SGPRs Spill')} occ={g('Occupancy [waves/SIMD]')} lds={g('LDS Size [bytes/block]')}")
