"""Diagnostic: build libsdhip.so with extra -D switches into scenedino_amd/variants/<name>.so
(same sources and flags as scenedino_amd/build.py).  usage: build_variant.py name -DA=1 ..."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from scenedino_amd import build as b  # noqa: E402


def build(name, defs, root=b.HERE):
    """variants/<name>.so from the sources under root (a scenedino_amd directory)."""
    od = os.path.join(b.HERE, "variants", "_obj_" + name)
    os.makedirs(od, exist_ok=True)

    def one(src):
        o = os.path.join(od, os.path.basename(src) + ".o")
        subprocess.run([b.hipcc()] + b.FLAGS + defs + ["-c", "-o", o, os.path.join(root, src)], check=True)
        return o

    with ThreadPoolExecutor(8) as ex:
        objs = list(ex.map(one, [s for s in b.SOURCES if os.path.exists(os.path.join(root, s))]))
    out = os.path.join(b.HERE, "variants", name + ".so")
    subprocess.run([b.hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs, check=True)
    return out


if __name__ == "__main__":
    print(build(sys.argv[1], sys.argv[2:]))
