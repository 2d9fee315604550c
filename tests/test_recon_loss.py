"""CPU: scenedino_amd.losses.ReconstructionLoss's torch route against the reference's own
float64 results (tests/golden/recon_loss.npz, written by tests/golden/make_golden_recon.py from
tests/_recon_inputs.py's inputs), the reference's quirks, make_loss / dropin wiring and the C
ABI of sd_recon_loss_fwd / _bwd.

Tolerances.  Gradients: the torch route runs the reference's op sequence in the same precision,
so a gradient's L2 norm and its dot with a fixed direction agree with the golden's float64
values to 1e-12 of the norm, and its stored float32 subset to float32 rounding (2^-23).
Metrics: the reference accumulates them in float32 tensors, so float32 rounding (2e-7 relative
holds two roundings)."""
from __future__ import annotations

import builtins
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _recon_inputs as ri
from conftest import GOLDEN, ROOT
from test_dropin import fake_reference  # noqa: F401  (fixture)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "recon_loss.npz"))


def _run(name, dtype=torch.float64):
    from scenedino_amd.losses import make_loss
    cfg, raw = ri.case(name)
    data = ri.convert(raw, dtype=dtype)
    loss = make_loss(cfg)
    res = loss(data)
    res["rec_loss"].backward()
    return loss, data, res


@pytest.mark.parametrize("name", list(ri.CASES))
def test_torch_route_matches_the_reference(golden, name):
    loss, data, res = _run(name)
    assert loss.last_route == "torch"
    names = [str(s) for s in golden[name + "/names"]]
    assert loss.get_loss_metric_names() == names and list(res) == names
    for k, v in res.items():
        ref = float(golden[f"{name}/metric/{k}"])
        assert v.dim() == 0 and (k == "rec_loss" or not v.requires_grad)
        assert abs(v.item() - ref) <= 2e-7 * abs(ref), (k, v.item(), ref)
    lv = ri.leaves(data) + (ri.leaves(data, "fine") if "fine" in data else [])
    seen = 0
    for lname, t in lv:
        key = f"{name}/norm/{lname}"
        if key not in golden.files:
            assert t.grad is None or not t.grad.any(), lname
            continue
        seen += 1
        g = t.grad.double().reshape(-1)
        n = float(golden[key])
        r = ri.projection(g)
        assert abs(float(g.norm()) - n) <= 1e-12 * n, lname
        assert abs(float((g * r).sum()) - float(golden[f"{name}/dot/{lname}"])) \
            <= 1e-12 * n * float(r.norm()), lname
        sub = torch.from_numpy(golden[f"{name}/sub/{lname}"]).double()
        mine = ri.subset(g)
        assert mine.shape == sub.shape
        assert float((mine - sub).norm()) <= 2.0 ** -23 * float(sub.norm()), lname
    assert seen >= 3


@pytest.mark.parametrize("key", list(ri.SHAPES))
def test_margins_of_the_shared_inputs(golden, key):
    """No argmin over views and no policy threshold can flip in float32: the top-2 view margin
    and the distance of every policy sum from 0.9 are >= 1e-5 (two orders above float32
    rounding of values below 1), and the policy masks a real share of the pixels."""
    from scenedino_amd.losses import reconstruction_loss as rl
    name = "shipped_" + key
    assert float(golden[name + "/view_margin"]) >= 1e-5
    assert float(golden[name + "/policy_margin"]) >= 1e-5
    assert 0.05 <= float(golden[name + "/masked"]) <= 0.6
    # the same two margins from this package's functions on the same inputs
    cfg, raw = ri.case(name)
    d = ri.convert(raw, grad=False)
    c0 = d["coarse"][0]
    b, pc, h, w, nv, ch = c0["rgb"].shape
    gt = d["rgb_gt"].unsqueeze(-2).expand(c0["rgb"].shape)
    e = rl.l1_ssim(c0["rgb"].permute(0, 1, 4, 5, 2, 3).reshape(-1, ch, h, w),
                   gt.permute(0, 1, 4, 5, 2, 3).reshape(-1, ch, h, w))
    top = e.view(b, pc, nv, h, w).topk(2, dim=2, largest=False).values
    assert float((top[:, :, 1] - top[:, :, 0]).min()) == pytest.approx(
        float(golden[name + "/view_margin"]), rel=1e-9)
    s = (c0["invalid"] * c0["weights"].unsqueeze(-1)).sum(-2)
    assert float((s - 0.9).abs().min()) == pytest.approx(float(golden[name + "/policy_margin"]),
                                                         rel=1e-9)


def test_depth_pairing_quirk_is_reproduced(golden):
    """(n, pc) = (2, 2): the reference pairs depth patches in (pc, n) order with image patches
    in (n, pc) order.  A same-order pairing gives a different regulariser."""
    from scenedino_amd.losses import reconstruction_loss as rl
    loss, data, res = _run("shipped_p16")
    ref = float(golden["shipped_p16/metric/edge_aware_smoothness"])
    assert abs(res["edge_aware_smoothness"].item() - ref) <= 2e-7 * abs(ref)
    d = data["coarse"][0]["depth"].detach()
    n, pc, h, w = d.shape
    u = 1 / d.reshape(-1, 1, h, w).clamp(1e-3, 80)
    u = u / u.mean(dim=[2, 3], keepdim=True)
    naive = rl.edge_aware_smoothness(rl._gt_patches(data, h, w), u, temperature=1).mean().item()
    assert abs(naive - ref) > 1e-3 * abs(ref)
    assert not torch.equal(rl.paired_depth(d), d.reshape(-1, h, w))


def test_a_zero_regulariser_is_dropped():
    """Constant depth: the depth regulariser is exactly zero, contributes nothing (neither a
    value nor a NaN gradient) and its metric reads 0."""
    from scenedino_amd.losses import make_loss
    cfg, raw = ri.case("shipped_odd")
    raw["coarse"][0]["depth"].fill_(7.0)
    data = ri.convert(raw)
    res = make_loss(cfg)(data)
    assert res["edge_aware_smoothness"].item() == 0.0
    res["rec_loss"].backward()
    c = data["coarse"][0]
    assert not c["depth"].grad.any()
    want = res["loss_rgb_coarse"] + 0.2 * res["loss_dino_coarse"] \
        + 0.25 * res["dino_edge_aware_smoothness"]
    assert res["rec_loss"].item() == pytest.approx(want.item(), rel=1e-12)


def test_a_nan_row_is_skipped_by_the_dino_term():
    from scenedino_amd.losses import make_loss
    cfg, raw = ri.case("p8_grid_artifacts")
    data = ri.convert(raw, grad=False)
    full = make_loss(cfg)(data)["loss_dino_coarse"].item()
    down = data["coarse"][0]["dino_features_downsampled"]
    C = down.shape[-1]
    rows = 1 - torch.nn.functional.cosine_similarity(
        5 * (down.reshape(-1, C) + data["dino_artifacts"].reshape(-1, C)),
        5 * data["dino_gt"].reshape(-1, C), dim=1)
    assert full == pytest.approx(rows.mean().item(), rel=1e-12)
    down.view(-1, C)[3, 5] = float("nan")
    got = make_loss(cfg)(data)
    keep = torch.ones(rows.numel(), dtype=torch.bool)
    keep[3] = False
    assert got["loss_dino_coarse"].item() == pytest.approx(rows[keep].mean().item(), rel=1e-12)
    assert bool(torch.isfinite(got["rec_loss"]))


def test_make_loss_and_metric_names(golden):
    from scenedino_amd.losses import ReconstructionLoss, StegoLoss, make_loss
    for name, (cfg, _, _) in ri.CASES.items():
        loss = make_loss(cfg)
        assert type(loss) is ReconstructionLoss
        assert loss.get_loss_metric_names() == [str(s) for s in golden[name + "/names"]]
    assert type(make_loss({"type": "stego"})) is StegoLoss
    with pytest.raises(ValueError):
        make_loss({"type": "other"})
    with pytest.raises(ValueError):
        make_loss(ri.shipped(invalid_policy="sometimes"))
    with pytest.raises(ValueError):
        make_loss(ri.shipped(coarse={"criterion": "l3"}))
    with pytest.raises(ValueError):
        make_loss(ri.shipped(regularizations=[{"type": "unknown", "lambda": 1}]))


def test_cpu_tensors_and_outside_configs_take_the_torch_route():
    from scenedino_amd.losses import make_loss
    cfg, raw = ri.case("shipped_odd")
    loss = make_loss(cfg)
    assert "device" in loss.native_domain(ri.convert(raw, dtype=torch.float32, grad=False))
    for name in ("l1", "l2", "median", "fine"):
        c, r = ri.case(name)
        assert make_loss(c).native_domain(ri.convert(r, dtype=torch.float32, grad=False))


def test_install_native_loss_resolves_here_without_kornia(fake_reference, monkeypatch):  # noqa: F811
    from scenedino_amd import dropin
    from scenedino_amd.losses import ReconstructionLoss, StegoLoss
    (fake_reference / "scenedino" / "losses" / "__init__.py").write_text("import kornia\n")
    (fake_reference / "scenedino" / "losses" / "base_loss.py").write_text("class BaseLoss:\n    pass\n")
    real_import = builtins.__import__

    def no_kornia(name, *a, **kw):
        if name == "kornia" or name.startswith("kornia."):
            raise ImportError("kornia is not installed")
        return real_import(name, *a, **kw)

    monkeypatch.setattr(builtins, "__import__", no_kornia)
    monkeypatch.delitem(sys.modules, "kornia", raising=False)
    dropin.install(native_loss=True)
    from scenedino.losses import make_loss
    from scenedino.losses.base_loss import BaseLoss
    assert BaseLoss.__module__ == "scenedino.losses.base_loss"
    assert type(make_loss(ri.shipped())) is ReconstructionLoss
    assert type(make_loss({"type": "stego"})) is StegoLoss
    with pytest.raises(ValueError):
        make_loss({"type": "other"})


def test_default_install_leaves_the_reference_losses_alone(fake_reference):  # noqa: F811
    from scenedino_amd import dropin
    dropin.install()
    assert importlib.import_module("scenedino.losses").MARK == "reference losses"


# ------------------------------------------------------------------------ C ABI
def test_entry_points_are_exported_and_abi_is_13():
    from scenedino_amd import _lib
    lib = _lib.load()
    for n in ("sd_recon_loss_work", "sd_recon_loss_fwd", "sd_recon_loss_bwd"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert lib.sd_abi_version() == 13 and _lib.ABI_VERSION == 13
    assert lib.sd_recon_loss_work(32, 768, 32) == 2 * 32 + 32 * 12 + 32
    assert lib.sd_recon_loss_work(4, 0, 0) == 8
    assert lib.sd_recon_loss_work(0, 64, 1) == -1 and lib.sd_recon_loss_work(4, 100, 1) == -1


def test_args_struct_layout_matches_the_c_header(tmp_path):
    from scenedino_amd import _lib
    py, cname = _lib.SdReconLossArgs, "sd_recon_loss_args"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sdhip.h"', "int main(void){",
             f'printf("size %zu\\n", sizeof({cname}));']
    for fname, _ in py._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(out[::2], map(int, out[1::2])))
    assert ctypes.sizeof(py) == got["size"]
    for fname, _ in py._fields_:
        assert getattr(py, fname).offset == got[fname], fname
    assert (_lib.SD_RL_POLICY_WEIGHT, _lib.SD_RL_POLICY_STRICT, _lib.SD_RL_POLICY_NONE) == (0, 1, 2)


def test_invalid_arguments_return_error_before_any_launch():
    """Validation runs before any HIP call, so this needs no device."""
    from scenedino_amd import _lib
    lib = _lib.load()
    ok = dict(rgb=16, rgb_gt=16, invalid=16, weights=16, depth=16, dino=16, dino_down=16,
              dino_gt=16, P=4, R=4, h=8, w=8, nv=4, K=8, C=64, Cd=64, dino_dtype=_lib.SD_F32,
              policy=_lib.SD_RL_POLICY_WEIGHT, work=16, rec=16, terms=16, sel=16, edge=16,
              dmean=16, count=16, g_rec=16, d_rgb=16, d_depth=16, d_dino=16, d_down=16)
    bad = [dict(ok, rgb=None), dict(ok, rgb_gt=None), dict(ok, work=None), dict(ok, P=0),
           dict(ok, h=1), dict(ok, w=17), dict(ok, nv=9), dict(ok, nv=0), dict(ok, C=96),
           dict(ok, C=832), dict(ok, Cd=32), dict(ok, policy=3), dict(ok, invalid=None),
           dict(ok, weights=None), dict(ok, dino_dtype=_lib.SD_F16), dict(ok, dino_gt=None),
           dict(ok, R=0), dict(ok, rgb=20), dict(ok, dino=24), dict(ok, d_dino=8)]
    for fn in (lib.sd_recon_loss_fwd, lib.sd_recon_loss_bwd):
        assert fn(None, None) == -1
        for args in bad:
            rc = fn(ctypes.byref(_lib.SdReconLossArgs(**args)), None)
            assert rc == -1 and b"sd_recon_loss" in lib.sd_last_error() \
                and b"invalid" in lib.sd_last_error(), args
    for args in (dict(ok, rec=None), dict(ok, terms=None)):
        assert lib.sd_recon_loss_fwd(ctypes.byref(_lib.SdReconLossArgs(**args)), None) == -1
    for args in (dict(ok, g_rec=None), dict(ok, sel=None), dict(ok, dmean=None),
                 dict(ok, edge=None), dict(ok, count=None)):
        assert lib.sd_recon_loss_bwd(ctypes.byref(_lib.SdReconLossArgs(**args)), None) == -1
