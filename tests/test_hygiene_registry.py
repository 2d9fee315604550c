"""CPU side of the memory-hygiene tests: the ratchet that every stream entry point of
include/sdhip.h has a hygiene case (tests/_arena.py REGISTRY) or a stated reason not to, and
the proof that the arena itself is not vacuous."""
import os
import re

import torch

import _arena
from _arena import Arena, run3
from conftest import ROOT


def _entry_points():
    src = open(os.path.join(ROOT, "include", "sdhip.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return sorted(set(re.findall(r"\bint\s+(sd_\w+)\s*\([^;{}]*?void\s*\*\s*stream\s*\)\s*;", src)))


def test_header_parse_finds_the_entry_points():
    names = _entry_points()
    for n in ("sd_spin", "sd_gemm", "sd_ln_gemm", "sd_render_proj", "sd_crop3d_compact",
              "sd_ssc_confusion", "sd_mlp_train_bwd"):
        assert n in names
    assert "sd_conv_wgrad_work" not in names and "sd_reserve_cus" not in names
    assert len(names) == 58, names


def test_every_entry_point_has_a_hygiene_case():
    names = _entry_points()
    tables = (_arena.REGISTRY, _arena.EXEMPT, _arena.PENDING)
    missing = [n for n in names if not any(n in t for t in tables)]
    assert not missing, ("entry points without a memory-hygiene case (add one and list it in "
                         f"tests/_arena.py REGISTRY): {missing}")
    stale = [n for t in tables for n in t if n not in names]
    assert not stale, f"listed but not in include/sdhip.h: {stale}"
    twice = [n for n in names if sum(n in t for t in tables) > 1]
    assert not twice, f"listed in more than one table: {twice}"
    assert all(r.strip() for r in _arena.EXEMPT.values())
    assert all(r.strip() for r in _arena.PENDING.values())


def test_registered_cases_exist():
    """Every registry value names a test function of the file it points to."""
    for name, tid in _arena.REGISTRY.items():
        path, func = tid.split("::")
        src = open(os.path.join(ROOT, path)).read()
        assert re.search(rf"^def {re.escape(func)}\(", src, flags=re.M), (name, tid)
        assert name in src or name[3:] in src, (name, tid)


def test_pending_list_only_shrinks():
    """PENDING holds the entry points whose case is still to be written.  Adding to it is how a
    new kernel would dodge the ratchet, so the list is pinned here: shrink both together."""
    assert sorted(_arena.PENDING) == sorted(PENDING_PINNED)


PENDING_PINNED = []


# ---- the harness is not vacuous: a deliberately sloppy torch "kernel" on CPU tensors ----------
def _sloppy(kind):
    x = torch.arange(15, dtype=torch.float32).view(3, 5)

    def body(ar):
        xv = ar.input("x", x, ld=8)
        out = ar.output("out", (3, 5), torch.float32, ld=7)
        ar.arm()
        out.copy_(2 * xv)                      # the kernel proper
        if ar.poison is None:
            return
        ints, off = ar.raw("out")
        flat = ints.view(torch.float32)
        if kind == "front":
            flat[off - 1] = 1.0                # one element before the payload
        elif kind == "back":
            flat[off + 3 * 7 + 2] = 1.0        # behind the last row gap
        elif kind == "gap":
            flat[off + 1 * 7 + 5] = 1.0        # row 1, column 5 of a 5-wide row (ld 7)
        elif kind == "unwritten":
            ints[off + 2 * 7 + 4] = _arena.sentinel_bits(torch.float32)
        elif kind == "input":
            xi, xo = ar.raw("x")
            xi.view(torch.float32)[xo + 3] = -1.0
        elif kind == "input_gap":
            xi, xo = ar.raw("x")
            xi.view(torch.float32)[xo + 6] = -1.0
        elif kind == "leak":
            xi, xo = ar.raw("x")               # reads one element past a row: poison leaks in
            out[0, 0] = out[0, 0] + 0 * xi.view(torch.float32)[xo + 5]

    return run3("cpu", body)


def test_arena_clean_kernel_passes():
    findings, plain = _sloppy("none")
    assert findings == []
    assert torch.equal(plain["out"], 2 * torch.arange(15, dtype=torch.float32).view(3, 5))


def test_arena_reports_margin_gap_and_unwritten():
    for kind, word in (("front", "front margin"), ("back", "back margin"), ("gap", "row gap"),
                       ("unwritten", "never written"), ("input", "read-only input changed"),
                       ("input_gap", "row gap")):
        findings, _ = _sloppy(kind)
        assert sum(word in f for f in findings) == 2, (kind, findings)  # once per poisoned run
    findings, _ = _sloppy("gap")
    assert "row 1, column 5" in findings[0]
    findings, _ = _sloppy("unwritten")
    assert "row 2, column 4" in findings[0]


def test_arena_reports_poison_leaking_into_the_result():
    findings, _ = _sloppy("leak")
    # 0 * NaN = NaN differs from the plain run; 0 * 1e30 = 0 does not: hence both poisons
    assert sum("nan-poisoned run differs" in f for f in findings) == 1, findings
    assert not any("finite-poisoned run differs" in f for f in findings)


def test_arena_layout():
    ar = Arena("cpu", "nan")
    v = ar.output("o", (300, 10), torch.bfloat16, ld=18, tile_rows=256)
    ints, off = ar.raw("o")
    assert v.data_ptr() % 16 == 0 and v.stride() == (18, 1)
    assert off * 2 >= max(4096, 256 * 18 * 2)
    assert (ints.numel() - off - 300 * 18) * 2 >= max(4096, 256 * 18 * 2)
    w = ar.work("w", 37)
    assert w.numel() == 37 and torch.isnan(w).all()
    k = ar.output("k", (2, 3, 4), torch.int32)
    assert int(k[0, 0, 0]) < 0 and k.is_contiguous()
