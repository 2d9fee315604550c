"""CPU: ``mode="upsample-gt"`` behind its switch, and the torch route of MultiScaleCropGT
(scenedino_amd/models/backbones/dino/upsampler.py).

tests/golden/msc_gt.npz (tests/golden/make_golden_msc.py) holds the reference's own
``forward_chunk`` / ``_accumulate_predictions`` / ``InterpolatedGT`` in float64 for injected views
and a stub gt encoder with fixed grids; the torch route reproduces it to 1e-12.  The reference
ran with kornia's ``warp_perspective`` replaced by this package's restatement, so the fixture
pins the reference's control flow (view order, flip reversal, mask padding, NaN handling,
channel chunking, normalisation) and everything else except kornia's warp itself; the warp
restatement has its own tests below, from its definition.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _msc_inputs as mi
from test_encoder import CONF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP = dict(CONF, mode="upsample-gt", downsampler_arch=None, upsampler_arch="multiscale-crop",
          image_size=[32, 64])


def _up():
    from scenedino_amd.models.backbones.dino import upsampler
    return upsampler


def _wrapper(grids, V=4, size=(24, 40), **kw):
    return _up().MultiScaleCropGT(mi.FixedGrids(grids), num_views=V, image_size=size, **kw)


# ---------------------------------------------------------------------- construction
@pytest.mark.parametrize("arch", ["multiscale-crop", "bilinear"])
def test_switch_builds_the_wrapper(arch):
    from scenedino_amd.models.backbones import make_backbone
    up = _up()
    m = make_backbone(dict(UP, upsampler_arch=arch), upsample_gt=True)
    assert isinstance(m.gt_wrapper, up.MultiScaleCropGT if arch == "multiscale-crop"
                      else up.InterpolatedGT)
    assert m.downsampler is None and m.downsample(torch.zeros(1, 4, 4, 384)) is None
    assert not [k for k in m.state_dict() if k.startswith("gt_wrapper.")]
    assert m.gt_wrapper.gt_encoder is m.gt_encoder
    assert "gt_encoder.model.vit.norm.bias" in m.state_dict()
    from scenedino_amd.models.backbones.dino.dinov2_module import DINOv2Module
    assert DINOv2Module.from_conf(UP, upsample_gt=True).gt_wrapper is not None


def test_without_the_switch_it_still_raises():
    from scenedino_amd.models.backbones import make_backbone
    with pytest.raises(NotImplementedError, match="upsample_gt=True"):
        make_backbone(UP)
    with pytest.raises(NotImplementedError):
        make_backbone(UP, upsample_gt=False)
    with pytest.raises(NotImplementedError):
        make_backbone(dict(UP, upsampler_arch="spline"), upsample_gt=True)


def test_module_ground_truth_pass_uses_the_wrapper():
    """dinov2_module.py:160-168 with a stub wrapper, the flip_avg_gt branch included."""
    from scenedino_amd.models.backbones import make_backbone
    m = make_backbone(dict(UP, flip_avg_gt=True), upsample_gt=True)
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(1, 5, 4, 6, generator=g), torch.randn(1, 5, 4, 6, generator=g)
    x = torch.randn(1, 3, 4, 6, generator=g)
    seen = []

    def wrapper(im):
        seen.append(im)
        return [a if len(seen) == 1 else b]

    m.gt_wrapper = None
    object.__setattr__(m, "gt_wrapper", wrapper)
    out = m(x, ground_truth=True)
    assert torch.equal(seen[0], x) and torch.equal(seen[1], x.flip([-1]))
    assert torch.equal(out[0], F.normalize(b.flip([-1]) + a, dim=1))
    m.flip_avg_gt = False
    assert m(x, ground_truth=True)[0] is b


def test_dropin_keeps_the_config_on_the_native_module(monkeypatch):
    """install(upsample_gt=True): _ref_make_model builds the native DINOv2Module with its
    wrapper; by default the mode still goes to the reference's make_backbone."""
    import inspect
    import sys
    import types
    from scenedino_amd import dropin, models as amd_models
    from scenedino_amd.models.backbones.dino.dinov2_module import DINOv2Module
    ref = types.ModuleType("scenedino.models.backbones")
    ref.make_backbone = lambda conf: "reference backbone"
    monkeypatch.setitem(sys.modules, "scenedino.models.backbones", ref)
    monkeypatch.setattr(amd_models, "make_model",
                        lambda config, dconf, encoder, downstream_head: encoder)
    monkeypatch.setattr(dropin, "_NATIVE_ENCODER", True)
    assert dropin._UPSAMPLE_GT is False
    assert dropin._ref_make_model({"encoder": UP}) == "reference backbone"
    monkeypatch.setattr(dropin, "_UPSAMPLE_GT", True)
    enc = dropin._ref_make_model({"encoder": UP})
    assert isinstance(enc, DINOv2Module) and enc.gt_wrapper is not None and enc.downsampler is None
    assert inspect.signature(dropin.install).parameters["upsample_gt"].default is False


# ---------------------------------------------------------------------------- golden
def test_torch_route_reproduces_the_reference():
    """The reference's float64 results (see the module docstring for what they pin)."""
    up, c, inp = _up(), mi.GOLDEN, mi.golden_inputs()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "msc_gt.npz"))
    enc = mi.FixedGrids(inp["grids"])
    w = up.MultiScaleCropGT(enc, num_views=c["V"], image_size=(c["H"], c["W"]))
    w.sample_views = lambda n: (inp["boxes"][:n], inp["flips"][:n])
    out = w(inp["images"])
    assert isinstance(out, list) and len(out) == 1 and w.last_route == "torch"
    assert enc.calls == [(c["B"] * c["V"], 3, c["H"], c["W"])]
    want = torch.from_numpy(gold["forward_chunk"])
    assert out[0].dtype == torch.float64 and out[0].shape == want.shape
    assert (out[0] - want).abs().max().item() <= 1e-12
    T = up.view_transforms(inp["boxes"], inp["flips"], (c["H"], c["W"])).double()
    acc = w._accumulate_predictions(inp["acc"].clone(), T)
    assert (acc - torch.from_numpy(gold["accumulate"])).abs().max().item() <= 1e-12
    ip = up.InterpolatedGT("bilinear", mi.FixedGrids(inp["grids"]), (c["H"], c["W"]))
    got = ip(torch.zeros(c["B"] * c["V"], 3, c["H"], c["W"]))
    assert (got[0] - torch.from_numpy(gold["interpolated"])).abs().max().item() <= 1e-12
    assert isinstance(up.build_gt_upsampling_wrapper("bicubic", enc, (8, 8)), up.InterpolatedGT)


def test_result_does_not_depend_on_the_chunking():
    up = _up()
    g = torch.Generator().manual_seed(3)
    n, V = 5, 4  # 20 views > max_chunk: the reference's chunked branch
    grids = torch.randn(V, 4, 2, 3, generator=g, dtype=torch.float64)

    class PerView(mi.FixedGrids):  # grids that depend on the view's pixels, not on its position
        def forward(self, x):
            return [self.grids.repeat(x.shape[0] // V, 1, 1, 1) * x.mean((1, 2, 3)).view(-1, 1, 1, 1)]

    images = torch.rand(n, 3, 12, 16, generator=g, dtype=torch.float64) + 0.5
    w = up.MultiScaleCropGT(PerView(grids), num_views=V, image_size=(12, 16))
    torch.manual_seed(5)
    views = up.MultiScaleCropGT.sample_views(w, n)
    w.sample_views = lambda k: views
    chunked = w(images)[0]
    w.max_chunk = 1000
    assert torch.equal(chunked, w(images)[0]) and chunked.shape == (n, 4, 12, 16)


# ------------------------------------------------------------------ warp restatement
def _plain(grid, size):
    u = F.interpolate(grid, size=size, mode="bilinear")
    return u / torch.linalg.norm(u, dim=1, keepdim=True)


def test_identity_flip_and_outside_transforms():
    g = torch.Generator().manual_seed(1)
    H, W = 18, 52
    grid = torch.randn(1, 6, 3, 4, generator=g, dtype=torch.float64)
    w = _wrapper(None, size=(H, W))
    eye = torch.eye(3, dtype=torch.float64)
    # identity T, equal grids in all views: the flipped view's grid is the flipped grid
    feats = torch.stack([grid[0], grid[0], grid[0].flip(-1), grid[0]])[None]
    out = w.accumulate(feats, eye.expand(1, 2, 3, 3), H, W)
    assert (out - _plain(grid, (H, W))).abs().max().item() <= 1e-12
    # a pure-flip T on flipped grids equals the base view
    flip = torch.tensor([[-1.0, 0, W - 1], [0, 1, 0], [0, 0, 1]], dtype=torch.float64)
    feats = torch.stack([grid[0].flip(-1), grid[0].flip(-1), grid[0].flip(-1), grid[0]])[None]
    out = w.accumulate(feats, flip.expand(1, 2, 3, 3), H, W)
    assert (out - _plain(grid, (H, W))).abs().max().item() <= 1e-12
    # every pixel mapped outside: the mean of the two base views
    away = torch.tensor([[1.0, 0, 10 * W], [0, 1, 0], [0, 0, 1]], dtype=torch.float64)
    other = torch.randn(4, 6, 3, 4, generator=g, dtype=torch.float64)
    out = w.accumulate(other[None], away.expand(1, 2, 3, 3), H, W, normalize=False)
    up2 = F.interpolate(other[2:], size=(H, W), mode="bilinear")
    assert (out[0] - (up2[0].flip(-1) + up2[1]) / 2).abs().max().item() <= 1e-12
    # no augmented view at all
    out = _wrapper(None, V=2, size=(H, W)).accumulate(other[None, 2:], eye.expand(1, 0, 3, 3),
                                                      H, W, normalize=False)
    assert (out[0] - (up2[0].flip(-1) + up2[1]) / 2).abs().max().item() <= 1e-12


def test_partially_valid_view_counts_per_pixel():
    """One-hot view grids, no normalisation: channel k holds view k's weight, so a crop's
    support and the divisor show directly."""
    up, H, W = _up(), 24, 40
    feats = torch.zeros(1, 3, 3, 3, 5, dtype=torch.float64)
    for k in range(3):
        feats[0, k, k] = 1.0
    T = up.view_transforms(torch.tensor([[[8, 6, 20, 12]]]), torch.tensor([[False]]), (H, W)).double()
    out = _wrapper(None, V=3, size=(H, W)).accumulate(feats, T, H, W, normalize=False)[0]
    inside = torch.zeros(H, W, dtype=torch.bool)
    inside[6:18, 8:28] = True
    assert torch.equal(out[0] > 0, inside)  # the box maps onto the whole view
    # T is stored in float32: the box's rim samples a hair outside the view
    assert bool((out[0][6:18, 8:28] - 1 / 3).abs().max() <= 1e-5)
    assert bool((out[1][0, :5] - 0.5).abs().max() <= 1e-12)  # far outside: two base views
    assert bool((out[2][12, 18] - 1 / 3).abs() <= 1e-12) and bool((out[2][0, 0] - 0.5).abs() <= 1e-12)


# ----------------------------------------------------------------------------- views
def test_transform_maps_box_corners_to_image_corners():
    up, H, W = _up(), 24, 40
    boxes = torch.tensor([[[4, 3, 28, 16], [10, 6, 24, 14]]])
    T = up.view_transforms(boxes, torch.tensor([[False, True]]), (H, W)).double()[0]
    x0, y0, w, h = boxes[0, 0].tolist()
    for (u, v), (a, b) in zip([(x0, y0), (x0 + w - 1, y0 + h - 1)], [(0, 0), (W - 1, H - 1)]):
        p = T[0] @ torch.tensor([u, v, 1.0], dtype=torch.float64)
        assert abs(p[0] / p[2] - a) <= 1e-5 and abs(p[1] / p[2] - b) <= 1e-5
    x0, y0, w, h = boxes[0, 1].tolist()  # flipped first: box columns count from the right
    for (u, v), (a, b) in zip([(W - 1 - x0, y0), (W - 1 - (x0 + w - 1), y0 + h - 1)],
                              [(0, 0), (W - 1, H - 1)]):
        p = T[1] @ torch.tensor([u, v, 1.0], dtype=torch.float64)
        assert abs(p[0] / p[2] - a) <= 1e-5 and abs(p[1] / p[2] - b) <= 1e-5


def test_augmented_image_is_the_resized_crop():
    up, H, W = _up(), 24, 40
    g = torch.Generator().manual_seed(2)
    img = torch.rand(1, 3, H, W, generator=g, dtype=torch.float64)
    boxes = torch.tensor([[[4, 3, 28, 16], [10, 6, 24, 14]]])
    flips = torch.tensor([[False, True]])
    w = _wrapper(None, size=(H, W))
    views = w._get_augmentations(img, up.view_transforms(boxes, flips, (H, W)).double())
    assert views.shape == (1, 4, 3, H, W)
    assert torch.equal(views[:, -1], img) and torch.equal(views[:, -2], img.flip(-1))
    for k in range(2):
        x0, y0, bw, bh = boxes[0, k].tolist()
        src = img.flip(-1) if bool(flips[0, k]) else img
        want = F.interpolate(src[..., y0:y0 + bh, x0:x0 + bw], size=(H, W), mode="bilinear",
                             align_corners=True)
        assert (views[:, k] - want).abs().max().item() <= 1e-6  # T is stored in float32


def test_default_draws():
    H, W = 24, 40
    w = _wrapper(None, V=5, size=(H, W))
    assert w.ratio == pytest.approx(((W / H) / 1.2, (W / H) * 1.2)) and w.scale == (0.5, 1.0)
    torch.manual_seed(11)
    boxes, flips = w.sample_views(40)
    torch.manual_seed(11)
    again = w.sample_views(40)
    assert torch.equal(boxes, again[0]) and torch.equal(flips, again[1])
    assert boxes.shape == (40, 3, 4) and flips.shape == (40, 3) and flips.dtype == torch.bool
    x0, y0, bw, bh = boxes.unbind(-1)
    assert bool((x0 >= 0).all() and (y0 >= 0).all() and (x0 + bw <= W).all() and (y0 + bh <= H).all())
    frac = (bw * bh).double() / (H * W)
    assert 0.45 <= frac.min() and frac.max() <= 1.0 and frac.std() > 0.05
    asp = bw.double() / bh.double()
    assert bool((asp >= w.ratio[0] * 0.9).all() and (asp <= w.ratio[1] * 1.1).all())
    assert 0.2 < flips.double().mean() < 0.8 and len(set(x0.flatten().tolist())) > 3


def test_fallback_branch():
    H, W = 24, 40
    # no box of this aspect fits the image: the central fallback
    w = _wrapper(None, size=(H, W), ratio=(100.0, 200.0))
    boxes, _ = w.sample_views(3)
    assert bool((boxes == torch.tensor([0, 11, 40, 2])).all())
    w = _wrapper(None, size=(H, W), ratio=(0.01, 0.02))
    boxes, _ = w.sample_views(2)
    assert bool((boxes == torch.tensor([19, 0, 2, 24])).all())


# ------------------------------------------------------------------------------- ABI
def test_entry_point_is_exported_without_an_abi_bump():
    from scenedino_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "sd_msc_gt") and "sd_msc_gt" in _lib.SIGNATURES
    assert lib.sd_abi_version() == 13 and _lib.ABI_VERSION == 13


def test_args_struct_layout_matches_the_c_header(tmp_path):
    from scenedino_amd import _lib
    py, cname = _lib.SdMscGtArgs, "sd_msc_gt_args"
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


def test_invalid_arguments_return_error_before_any_launch():
    """Validation runs before any HIP call, so this needs no device."""
    from scenedino_amd import _lib
    lib = _lib.load()
    ok = dict(feat=16, T=16, out=32, B=1, V=4, C=8, hp=2, wp=2, H=4, W=4, normalize=1)
    for bad in (dict(V=9), dict(V=1), dict(C=1025), dict(C=0), dict(feat=0), dict(out=0),
                dict(T=0), dict(feat=20), dict(H=0), dict(wp=0), dict(B=0)):
        a = _lib.SdMscGtArgs(**dict(ok, **bad))
        assert lib.sd_msc_gt(ctypes.byref(a), None) == -1, bad
        assert b"sd_msc_gt" in lib.sd_last_error()
    assert lib.sd_msc_gt(None, None) == -1
