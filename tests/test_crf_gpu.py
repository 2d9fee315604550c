"""Dense CRF on the GPU: the native route (sd_dense_crf, csrc/sdhip_crf.hip) against the float64
oracle of tests/_crf_oracle.py on its three fixtures, batching and repeatability bit for bit,
image batches through SemanticHead, one case at the full 192 x 640 size against the torch route,
and the edges of the native domain."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

import _crf_oracle as O
import _stego_oracle as so

# Largest |Q - oracle Q| the native route showed over the three fixtures on an MI355X
# (24 x 80: 2.01e-3, 13 x 37: 2.45e-4, 8 x 300: 8.77e-4), from the f16 rounding of the bilateral
# weights and of n_j Q_j; the bound is 4 x that for other inputs' rounding (8.04e-3), rounded up to
# one digit (cap 1e-2: beyond it the margin rule would exclude more than 1 % of a fixture).
Q_MEASURED = 2.01e-3
Q_BOUND = 9e-3
MAX_EXCLUDED = 0.01


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()
    return "cuda"


def _crf():
    from scenedino_amd.downstream_head import crf
    return crf


def _native(image, unaries, dev, **params):
    """image (H, W, 3) uint8 numpy, unaries [(c, N) float32 tensors] -> (labels (R, N), [Q (c, N)])."""
    crf = _crf()
    labels, qs = crf.crf_inference(torch.from_numpy(image.copy()).to(dev), [u.to(dev) for u in unaries],
                                   want_q=True, **params)
    assert crf.last_route == "native"
    return labels, qs


def _unary(fx):
    return torch.from_numpy(fx["unary"].T.copy()).float()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", O.FIXTURES)
def test_native_matches_the_oracle(gpu, shape):
    fx = O.fixture(*shape)
    labels, qs = _native(fx["image"], [_unary(fx)], gpu)
    Q, got = qs[0].cpu().numpy().T.astype(np.float64), labels[0].cpu().numpy()
    err = float(np.abs(Q - fx["Q"]).max())
    wide = fx["margin"] > 2 * Q_BOUND
    print(f"native {shape}: max |dQ| = {err:.3g}, excluded {int((~wide).sum())} of {wide.size}, "
          f"label mismatches on wide-margin pixels {int((got[wide] != fx['out'][wide]).sum())}, "
          f"anywhere {int((got != fx['out']).sum())}")
    assert err <= Q_BOUND
    assert float((~wide).mean()) <= MAX_EXCLUDED
    assert np.array_equal(got[wide], fx["out"][wide])
    assert np.array_equal(got, Q.argmax(1))


@functools.lru_cache(maxsize=None)
def _four_results():
    """One image (13 x 37) with four label maps of 19, 19, 27 and 2 classes."""
    crf = _crf()
    image = O.fixture(13, 37, 2)["image"]
    g = torch.Generator().manual_seed(5)
    classes = (19, 19, 27, 2)
    return image, [crf.unary_from_labels(torch.randint(0, c, (13 * 37,), generator=g), c) for c in classes]


@pytest.mark.gpu
def test_batched_results_equal_single_calls_bit_for_bit(gpu):
    image, unaries = _four_results()
    labels, qs = _native(image, unaries, gpu)
    for r, u in enumerate(unaries):
        l1, q1 = _native(image, [u], gpu)
        assert torch.equal(l1[0], labels[r]), r
        assert torch.equal(q1[0].view(torch.int32), qs[r].view(torch.int32)), r
    assert len({tuple(lab.tolist()) for lab in labels[:2]}) == 2  # the two 19-class maps differ


@pytest.mark.gpu
def test_repeated_call_is_bit_equal(gpu):
    fx = O.fixture(8, 300, 27)
    a = _native(fx["image"], [_unary(fx)], gpu)
    b = _native(fx["image"], [_unary(fx)], gpu)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][0].view(torch.int32), b[1][0].view(torch.int32))


@pytest.mark.gpu
def test_image_batch_through_semantic_head_equals_single_images(gpu):
    from scenedino_amd.downstream_head.semantic_head import SemanticHead
    crf = _crf()
    head = SemanticHead(**so.HEAD_ARGS, mode="3d", apply_crf=True)
    head.load_state_dict(so.head_state(11), strict=False)
    head = head.to(gpu).eval()
    head.native_crf = True
    g = torch.Generator().manual_seed(7)
    n, v, h, w = 2, 2, 8, 12
    rgb = torch.rand(n, v, h, w, 1, 3, generator=g).to(gpu)
    feats = torch.randn(n, v, h, w, 1, 768, generator=g).to(gpu)

    def run(sl):
        data = {"coarse": [{"rgb": rgb[sl], "dino_features": feats[sl]}],
                "sample_surface_sigma": None, "sample_surface_dino_features": None}
        with torch.no_grad():
            return head.forward_training(data)["segmentation"]["results"]

    full = run((slice(None), slice(None)))
    assert crf.last_route == "native"
    assert list(full) == ["direct_cluster", "stego_cluster", "direct_cluster_crf", "stego_cluster_crf"]
    for i in range(n):
        for j in range(v):
            one = run((slice(i, i + 1), slice(j, j + 1)))
            for k in full:
                a, b = full[k]["segs_pred"][i, j], one[k]["segs_pred"][0, 0]
                assert a.shape == b.shape == (h, w, 1) and a.dtype == b.dtype == torch.int64
                assert torch.equal(a, b), (k, i, j)
    for k in ("direct_cluster", "stego_cluster"):  # each image refined from its own raw labels
        image = rgb[1, 0, :, :, 0].permute(2, 0, 1)
        want = crf.dense_crf_labels(image, full[k]["segs_pred"][1, 0], num_classes=19)
        assert torch.equal(full[k + "_crf"]["segs_pred"][1, 0], want)


@pytest.mark.gpu
def test_full_size_against_the_torch_route(gpu):
    """192 x 640, 19 classes, 2 iterations: indices and tiling at the real size.  The torch route on
    the GPU (tied to the oracle by the small cases) is the reference; same bound and margin rule."""
    crf = _crf()
    image, labels = O.make_fixture(192, 640, 19)
    img = torch.from_numpy(image).to(gpu)
    U = crf.unary_from_labels(torch.from_numpy(labels).to(gpu), 19)
    got_l, got_q = crf.crf_inference(img, [U], want_q=True, iters=2)
    assert crf.last_route == "native"
    native, crf._NATIVE = crf._NATIVE, False
    try:
        want_l, want_q = crf.crf_inference(img, [U], want_q=True, iters=2)
        assert crf.last_route == "torch"
    finally:
        crf._NATIVE = native
    err = float((got_q[0] - want_q[0]).abs().max())
    top = want_q[0].topk(2, dim=0).values
    wide = (top[0] - top[1]) > 2 * Q_BOUND
    print(f"native 192 x 640: max |dQ| = {err:.3g}, excluded {int((~wide).sum())} of {wide.numel()}, "
          f"labels changed by the CRF {int((want_l[0].cpu() != torch.from_numpy(labels).reshape(-1)).sum())}")
    assert err <= Q_BOUND
    assert float((~wide).float().mean()) <= MAX_EXCLUDED
    assert torch.equal(got_l[0][wide], want_l[0][wide])


@pytest.mark.gpu
def test_outside_the_native_domain(gpu):
    """A non-contiguous image, 65 classes and sxy_g above SD_CRF_MAX_SXY_G take the torch route; the
    entry point itself rejects them before any launch, with sd_last_error text."""
    from scenedino_amd import _lib
    crf = _crf()
    lib = _lib.load()
    g = torch.Generator().manual_seed(9)
    H, W = 6, 10
    wide = torch.randint(0, 256, (H, 2 * W, 3), generator=g, dtype=torch.uint8).to(gpu)
    img = wide[:, ::2]
    assert not img.is_contiguous()
    U2 = crf.unary_from_labels(torch.randint(0, 2, (H * W,), generator=g), 2).to(gpu)
    U65 = crf.unary_from_labels(torch.randint(0, 65, (H * W,), generator=g), 65).to(gpu)
    dense = img.contiguous()
    l_ref, q_ref = crf.crf_inference(dense, [U2], want_q=True)
    assert crf.last_route == "native"
    l_nc, q_nc = crf.crf_inference(img, [U2], want_q=True)
    assert crf.last_route == "torch"
    assert float((q_nc[0] - q_ref[0]).abs().max()) <= Q_BOUND
    crf.crf_inference(dense, [U65])
    assert crf.last_route == "torch"
    crf.crf_inference(dense, [U2], sxy_g=0.71)
    assert crf.last_route == "torch"
    crf.crf_inference(dense, [U2], sxy_g=0.7)
    assert crf.last_route == "native"

    work = torch.empty(1 << 20, dtype=torch.uint8, device=gpu)
    labels = torch.full((H * W,), -7, dtype=torch.int64, device=gpu)

    def call(classes=(2,), unary=U2, **kw):
        a = _lib.SdCrfArgs(image=dense.data_ptr(), unary=unary.data_ptr(), work=work.data_ptr(),
                           labels=labels.data_ptr(), q=None, H=H, W=W, n_results=len(classes), iters=1,
                           classes=(ctypes.c_int32 * 8)(*classes), w_g=3.0, sxy_g=0.3, w_b=4.0,
                           sxy_b=20.0, srgb=3.0)
        for k, val in kw.items():
            setattr(a, k, val)
        return lib.sd_dense_crf(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    for bad in (dict(classes=(65,), unary=U65), dict(classes=(1,)), dict(sxy_g=0.71), dict(sxy_g=0.0),
                dict(iters=65), dict(iters=-1), dict(H=0), dict(W=4097), dict(n_results=9), dict(srgb=0.0),
                dict(sxy_b=float("nan")), dict(w_b=-1.0), dict(work=None), dict(labels=None),
                dict(image=dense.data_ptr() + 1)):
        assert call(**bad) == -1, bad
        assert b"sd_dense_crf" in lib.sd_last_error()
    assert lib.sd_dense_crf(None, None) == -1
    assert lib.sd_dense_crf_work(6, 10, 1, (ctypes.c_int32 * 8)(65)) == -1
    assert b"sd_dense_crf_work" in lib.sd_last_error()
    assert lib.sd_dense_crf_work(2048, 1024, 1, (ctypes.c_int32 * 8)(2)) == -1  # N > 2^20
    torch.cuda.synchronize()
    assert bool((labels == -7).all())  # no rejected call wrote anything
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(((labels == 0) | (labels == 1)).all())
