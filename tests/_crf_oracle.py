"""Brute-force oracle of the dense CRF (scenedino_amd/downstream_head/crf.py's model) in numpy
float64: the full N x N kernel matrices, no truncation, no blocking; and the seeded fixtures the
CRF tests share.

    f^g_i = (x_i, y_i) / sxy_g,   f^b_i = (x_i / sxy_b, y_i / sxy_b, rgb_i / srgb)
    k^p_ij = exp(-|f^p_i - f^p_j|^2 / 2)  (j = i included),   n^p_i = (sum_j k^p_ij + 1e-20)^(-1/2)
    Q^0 = softmax(-U),   Q^{t+1}_i = softmax(-U_i + sum_p w_p n^p_i sum_j k^p_ij n^p_j Q^t_j)
"""
from __future__ import annotations

import functools
import math

import numpy as np

DEFAULTS = dict(iters=10, w_g=3.0, sxy_g=0.3, w_b=4.0, sxy_b=20.0, srgb=3.0)

# (H, W, C): 19 classes at the patch-grid aspect; N = 481 is no multiple of any tile and C = 2 is
# the smallest class count; 8 x 300 is wider than the bilateral truncation distance (5.68 x 20 =
# 113.6 pixels), so the native kernel skips key blocks there
FIXTURES = ((24, 80, 19), (13, 37, 2), (8, 300, 27))
# per fixture: labels the oracle changes, pixels below top-two margin 1e-3 / 1e-2 / 2e-2
FIGURES = {(24, 80, 19): (202, (0, 0, 1)), (13, 37, 2): (10, (0, 0, 0)), (8, 300, 27): (207, (1, 7, 17))}


def softmax(x):
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def onehot_unary(labels, C):
    """-log softmax of the one-hot logits of labels (N) -> (N, C) float64."""
    logits = np.zeros((labels.size, C))
    logits[np.arange(labels.size), labels.reshape(-1)] = 1.0
    return -np.log(softmax(logits))


def oracle(image, unary, iters=10, w_g=3.0, sxy_g=0.3, w_b=4.0, sxy_b=20.0, srgb=3.0):
    """image (H, W, 3) uint8, unary (N, C) -> Q^{iters} (N, C) float64."""
    H, W = image.shape[:2]
    N = H * W
    yy, xx = np.divmod(np.arange(N), W)
    pos = np.stack([xx, yy], axis=1).astype(np.float64)
    fg = pos / sxy_g
    fb = np.concatenate([pos / sxy_b, image.reshape(N, 3).astype(np.float64) / srgb], axis=1)
    Ks, ns = [], []
    for f in (fg, fb):
        d2 = ((f[:, None, :] - f[None, :, :]) ** 2).sum(-1)
        K = np.exp(-0.5 * d2)
        Ks.append(K)
        ns.append((K.sum(1) + 1e-20) ** -0.5)
    U = np.asarray(unary, dtype=np.float64)
    Q = softmax(-U)
    for _ in range(iters):
        msg = np.zeros_like(Q)
        for w, K, n in zip((w_g, w_b), Ks, ns):
            msg += w * n[:, None] * (K @ (n[:, None] * Q))
        Q = softmax(msg - U)
    return Q


def margin(Q):
    """Top-two margin per pixel of Q (N, C)."""
    s = np.sort(Q, axis=1)
    return s[:, -1] - s[:, -2]


def make_fixture(H, W, C):
    """Seeded scene: (image (H, W, 3) uint8, noisy labels (H, W) int64).  Draws, in order, on
    default_rng(0): the palette, the colour noise, the flip mask, the replacement labels."""
    rng = np.random.default_rng(0)
    bands = min(C, 5)
    clean = np.broadcast_to(np.arange(W) * bands // W, (H, W)).copy()
    clean[H // 4:H // 2, W // 3:W // 2] = bands - 1
    palette = rng.integers(0, 256, (C, 3))
    image = np.clip(palette[clean] + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
    flip = rng.random((H, W)) < 0.15
    labels = clean.astype(np.int64)
    labels[flip] = rng.integers(0, C, int(flip.sum()))  # one draw per flipped pixel
    return image, labels


@functools.lru_cache(maxsize=None)
def fixture(H, W, C):
    """The fixture with its oracle result: dict of image, labels, unary (N, C), Q (N, C) float64
    at the default parameters, out (N) its argmax, margin (N).  Computed once; do not modify."""
    image, labels = make_fixture(H, W, C)
    U = onehot_unary(labels, C)
    Q = oracle(image, U, **DEFAULTS)
    fx = {"image": image, "labels": labels, "unary": U, "Q": Q, "out": Q.argmax(1), "margin": margin(Q)}
    for v in fx.values():
        v.setflags(write=False)
    return fx


LSE = lambda C: math.log(math.e + C - 1)  # noqa: E731  (the unary of a one-hot: LSE - [c = label])
