"""Diagnostic: build libsdhip.so from the HIP sources of another git revision into
scenedino_amd/variants/<name>.so (tools/build_variant.py on that revision's sources) -- the A
side of an interleaved A/B against the working tree (tools/gpu_session.sh ab:CFG:<name>:REPS).
usage: build_rev.py <rev> <name> [-DX=1 ...]"""
import os
import subprocess
import sys
import tempfile

from build_variant import build

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def checkout(rev, tmp):
    """scenedino_amd/csrc and include of rev under tmp; returns its scenedino_amd directory."""
    files = subprocess.run(["git", "ls-tree", "-r", "--name-only", rev, "scenedino_amd/csrc", "include"],
                           cwd=ROOT, check=True, capture_output=True, text=True).stdout.split()
    for f in files:
        dst = os.path.join(tmp, f)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        with open(dst, "wb") as fh:
            fh.write(subprocess.run(["git", "show", f"{rev}:{f}"], cwd=ROOT, check=True,
                                    capture_output=True).stdout)
    return os.path.join(tmp, "scenedino_amd")


if __name__ == "__main__":
    print(build(sys.argv[2], sys.argv[3:], checkout(sys.argv[1], tempfile.mkdtemp(prefix="sdrev_"))))
