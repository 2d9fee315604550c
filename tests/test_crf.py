"""Dense CRF (scenedino_amd/downstream_head/crf.py) on the CPU: the torch route against the
brute-force float64 oracle of tests/_crf_oracle.py on its three fixtures, the wrapper around the
model (image conversion, unaries, the reference's ``dense_crf`` signature), SemanticHead's
``native_crf`` switch and ``dropin.install(native_crf=True)``."""
from __future__ import annotations

import importlib
import inspect
import sys

import numpy as np
import pytest
import torch

import _crf_oracle as O
import _stego_oracle as so


def _crf():
    from scenedino_amd.downstream_head import crf
    return crf


def _torch_q(fx, **params):
    crf = _crf()
    C = fx["unary"].shape[1]
    U = torch.from_numpy(fx["unary"].T.copy())  # float64: the route's sums take it as it is
    labels, qs = crf.crf_inference(torch.from_numpy(fx["image"].copy()), [U], want_q=True, **params)
    assert crf.last_route == "torch"
    assert labels.shape == (1, U.shape[1]) and qs[0].shape == (C, U.shape[1]) and qs[0].dtype == torch.float32
    return labels[0].numpy(), qs[0].numpy().T


# ----------------------------------------------------------------------------- model
@pytest.mark.parametrize("shape", O.FIXTURES)
def test_fixture_figures_and_non_vacuity_of_the_oracle(shape):
    """The oracle's own figures: every part of the model shows in the labels."""
    fx = O.fixture(*shape)
    labels = fx["labels"].reshape(-1)
    changed = int((fx["out"] != labels).sum())
    below = tuple(int((fx["margin"] < t).sum()) for t in (1e-3, 1e-2, 2e-2))
    assert (changed, below) == O.FIGURES[shape]
    assert changed >= 0.01 * labels.size
    one = O.oracle(fx["image"], fx["unary"], **dict(O.DEFAULTS, iters=1)).argmax(1)
    no_g = O.oracle(fx["image"], fx["unary"], **dict(O.DEFAULTS, w_g=0.0)).argmax(1)
    assert (one != fx["out"]).any() and (no_g != fx["out"]).any()
    assert np.array_equal(O.oracle(fx["image"], fx["unary"], **dict(O.DEFAULTS, iters=0)).argmax(1), labels)


@pytest.mark.parametrize("shape", O.FIXTURES)
def test_torch_route_matches_the_oracle(shape):
    """|dQ| <= 1e-6: the float32 rounding of the output of float64 sums."""
    fx = O.fixture(*shape)
    labels, Q = _torch_q(fx)
    err = float(np.abs(Q - fx["Q"]).max())
    print(f"torch route {shape}: max |dQ| = {err:.3g}")
    assert err <= 1e-6
    wide = fx["margin"] > 1e-5
    assert np.array_equal(labels[wide], fx["out"][wide])


def test_torch_route_parameters_and_zero_iterations():
    fx = O.fixture(13, 37, 2)
    for params in (dict(iters=1), dict(w_g=0.0), dict(iters=3, sxy_g=1.5, w_b=2.0, sxy_b=7.0, srgb=9.0)):
        want = O.oracle(fx["image"], fx["unary"], **dict(O.DEFAULTS, **params))
        _, Q = _torch_q(fx, **params)
        assert float(np.abs(Q - want).max()) <= 1e-6, params
    labels, _ = _torch_q(fx, iters=0)
    assert np.array_equal(labels, fx["labels"].reshape(-1))


def test_several_results_of_one_image_equal_single_inferences():
    crf = _crf()
    img = torch.from_numpy(O.fixture(13, 37, 2)["image"].copy())
    g = torch.Generator().manual_seed(0)
    labs = [torch.randint(0, c, (13 * 37,), generator=g) for c in (19, 2, 27)]
    U = [crf.unary_from_labels(lab, c) for lab, c in zip(labs, (19, 2, 27))]
    both, qs = crf.crf_inference(img, U, want_q=True, iters=2)
    for r in range(3):
        one, q1 = crf.crf_inference(img, [U[r]], want_q=True, iters=2)
        assert torch.equal(one[0], both[r]) and torch.equal(q1[0], qs[r])


# --------------------------------------------------------------------------- wrapper
def test_unary_of_a_one_hot_and_num_classes_none():
    crf = _crf()
    g = torch.Generator().manual_seed(1)
    lab = torch.randint(0, 7, (6, 10), generator=g)
    lab[0, 0] = 6
    U = crf.unary_from_labels(lab, 7)
    onehot = torch.nn.functional.one_hot(lab.reshape(-1), 7).t().float().reshape(7, 6, 10)
    want = -torch.log(torch.softmax(onehot, dim=0)).reshape(7, 60)
    torch.testing.assert_close(U, want, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(crf.unary_from_logits(onehot, (6, 10)), want, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(U.numpy().T, O.onehot_unary(lab.numpy(), 7), rtol=1e-6)
    image = torch.rand(3, 6, 10, generator=g)
    a = crf.dense_crf_labels(image, lab)             # max + 1 = 7
    b = crf.dense_crf_labels(image, lab, num_classes=7)
    assert a.shape == lab.shape and a.dtype == lab.dtype and torch.equal(a, b)
    # logits at a coarser size are resized bilinearly, align_corners=False
    coarse = torch.randn(3, 3, 5, generator=g)
    up = torch.nn.functional.interpolate(coarse[None], size=(6, 10), mode="bilinear", align_corners=False)[0]
    torch.testing.assert_close(crf.unary_from_logits(coarse, (6, 10)),
                               -torch.log_softmax(up, 0).reshape(3, 60))


def test_image_conversion_truncates_and_clamps():
    crf = _crf()
    x = torch.tensor([-0.5, 0.0, 0.4999 / 255, 1.9999 / 255, 0.5, 254.999 / 255, 1.0, 1.7])
    image = x.view(1, 2, 4).expand(3, 2, 4)
    u8 = crf.image_to_uint8(image)
    assert u8.shape == (2, 4, 3) and u8.dtype == torch.uint8 and u8.is_contiguous()
    assert u8[..., 0].reshape(-1).tolist() == [0, 0, 0, 1, 127, 254, 255, 255]
    assert "clamp" in inspect.getdoc(crf.image_to_uint8) and "wrap" in inspect.getdoc(crf.image_to_uint8)


def test_dense_crf_keeps_the_reference_signature():
    crf = _crf()
    assert list(inspect.signature(crf.dense_crf).parameters) == ["image_tensor", "output_logits"]
    assert (crf.MAX_ITER, crf.POS_W, crf.POS_XY_STD, crf.Bi_W, crf.Bi_XY_STD, crf.Bi_RGB_STD) == (10, 3, 0.3, 4, 20, 3)
    g = torch.Generator().manual_seed(2)
    image, logits = torch.rand(3, 6, 10, generator=g), torch.randn(4, 3, 5, generator=g)
    Q = crf.dense_crf(image, logits)
    assert isinstance(Q, np.ndarray) and Q.shape == (4, 6, 10)
    np.testing.assert_allclose(Q.sum(0), 1.0, atol=1e-6)
    u8 = crf.image_to_uint8(image).numpy()
    want = O.oracle(u8, crf.unary_from_logits(logits, (6, 10)).numpy().T.astype(np.float64), **O.DEFAULTS)
    assert float(np.abs(Q.reshape(4, -1).T - want).max()) <= 1e-6
    Q1 = crf.dense_crf(torch.rand(3, 1, 7, generator=g), torch.randn(2, 1, 7, generator=g))  # 1 x 7 image
    assert Q1.shape == (2, 1, 7) and np.isfinite(Q1).all()


# ------------------------------------------------------------------------ SemanticHead
def _head_data(n=1, v=1, h=6, w=10, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"coarse": [{"rgb": torch.rand(n, v, h, w, 1, 3, generator=g),
                        "dino_features": torch.randn(n, v, h, w, 1, 768, generator=g)}],
            "sample_surface_sigma": None, "sample_surface_dino_features": None}


def test_semantic_head_switch():
    from scenedino_amd.downstream_head.semantic_head import SemanticHead
    head = SemanticHead(**so.HEAD_ARGS, mode="3d", apply_crf=True).eval()
    assert head.native_crf is False
    with pytest.raises(NotImplementedError, match="pydensecrf"):
        head.forward_training(_head_data())
    head.native_crf = True
    torch.manual_seed(0)
    data = head.forward_training(_head_data())
    res = data["segmentation"]["results"]
    raw = ("direct_cluster", "stego_cluster")
    assert list(res) == list(raw) + [k + "_crf" for k in raw]
    crf = _crf()
    image = data["coarse"][0]["rgb"][0, 0, :, :, 0].permute(2, 0, 1)
    for k in raw:
        a, b = res[k]["segs_pred"], res[k + "_crf"]["segs_pred"]
        assert set(res[k + "_crf"]) == {"segs_pred"}
        assert a.shape == b.shape == (1, 1, 6, 10, 1) and a.dtype == b.dtype == torch.int64
        assert torch.equal(b[0, 0], crf.dense_crf_labels(image, a[0, 0], num_classes=19))
    # the switch changes nothing without apply_crf
    plain = SemanticHead(**so.HEAD_ARGS, mode="3d").eval()
    plain.native_crf = True
    assert list(plain.forward_training(_head_data())["segmentation"]["results"]) == list(raw)


# ----------------------------------------------------------------------------- drop-in
@pytest.fixture
def fake_reference(tmp_path, monkeypatch):
    """A stand-in ``scenedino`` checkout (the pattern of tests/test_metrics.py) whose
    downstream_head/crf.py needs a package that is not installed, as the reference's does."""
    root = tmp_path / "ref"
    files = {
        "scenedino/__init__.py": "",
        "scenedino/renderer/__init__.py": "from .nerf import NeRFRenderer\n",
        "scenedino/renderer/nerf.py": "class NeRFRenderer:\n    origin = 'reference'\n",
        "scenedino/models/__init__.py": "def make_model(config, downstream_config=None):\n    return 0\n",
        "scenedino/models/bts.py": "class BTSNet:\n    origin = 'reference'\n",
        "scenedino/common/__init__.py": "",
        "scenedino/common/ray_sampler.py": "class ImageRaySampler:\n    origin = 'reference'\n",
        "scenedino/downstream_head/__init__.py": "from .crf import dense_crf\n",
        "scenedino/downstream_head/crf.py": "import a_module_that_is_not_installed\n"
                                            "def dense_crf(image_tensor, output_logits):\n    return 'reference'\n",
    }
    for rel, txt in files.items():
        f = root / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(txt)
    saved = {k: v for k, v in sys.modules.items() if k == "scenedino" or k.startswith("scenedino.")}
    for k in saved:
        del sys.modules[k]
    monkeypatch.syspath_prepend(str(root))
    yield root
    for k in [k for k in sys.modules if k == "scenedino" or k.startswith("scenedino.")]:
        del sys.modules[k]
    sys.modules.update(saved)
    from scenedino_amd import dropin
    dropin._NATIVE_CRF = False


def test_install_native_crf_registers_dense_crf(fake_reference):
    from scenedino_amd import dropin
    assert inspect.signature(dropin.install).parameters["native_crf"].default is False
    dropin.install(native_crf=True)
    from scenedino.downstream_head.crf import dense_crf
    assert dense_crf is _crf().dense_crf
    assert importlib.import_module("scenedino.downstream_head").dense_crf is dense_crf
    assert dropin._NATIVE_CRF is True


def test_install_native_crf_leaves_an_importable_reference_module(fake_reference):
    (fake_reference / "scenedino" / "downstream_head" / "crf.py").write_text(
        "def dense_crf(image_tensor, output_logits):\n    return 'reference'\n")
    from scenedino_amd import dropin
    dropin.install(native_crf=True)
    from scenedino.downstream_head.crf import dense_crf
    assert dense_crf(None, None) == "reference"


def test_install_without_the_switch_registers_nothing(fake_reference):
    from scenedino_amd import dropin
    dropin.install()
    assert "scenedino.downstream_head.crf" not in sys.modules and dropin._NATIVE_CRF is False
    with pytest.raises(ImportError):
        importlib.import_module("scenedino.downstream_head.crf")
