"""f64 oracle and seeded inputs of the SSCBench pooling tests (sd_ssc_pool, sscbench.pool_voxels;
evaluate_model_sscbench.py:727-745).  numpy only."""
import numpy as np

# An f32 alpha carries at most about 2^-24 of absolute error here (measured 4.9e-8) and the
# ascending f32 sum adds less; labels are compared where the oracle's top-two mean-scale scores
# differ by more than 8x that.
MARGIN = 2.0 ** -21
MAX_EXCLUDED = 0.005  # share of voxels a case may exclude as near-ties

# (coarse dims, factor, n_classes, seed)
CASES = [
    ((3, 5, 7), 2, 19, 0),     # odd nz, partial last wave
    ((3, 5, 7), 2, 27, 5),
    ((2, 3, 33), 4, 19, 2),    # more than one wave per plane, nz not a multiple of anything
    ((1, 2, 32), 8, 19, 3),
    ((2, 256, 32), 2, 19, 4),  # the SSCBench column indexing
]


def make_inputs(dims, f, n_classes, seed):
    """sigma = softplus(2 randn) with 30 % zeros (f32), random labels (uint8), on the fine grid."""
    rng = np.random.default_rng(seed)
    shape = tuple(f * d for d in dims)
    x = 2.0 * rng.standard_normal(shape)
    sigma = np.logaddexp(0.0, x).astype(np.float32)
    sigma[rng.random(shape) < 0.3] = 0.0
    label = rng.integers(0, n_classes, shape).astype(np.uint8)
    return sigma, label


def blocks(a, f):
    """(f cx, f cy, f cz, ...) -> (cx, cy, cz, f^3, ...): the children of every coarse voxel in
    ascending (a, b, c) order."""
    cx, cy, cz = (d // f for d in a.shape[:3])
    rest = a.shape[3:]
    a = a.reshape((cx, f, cy, f, cz, f) + rest)
    a = np.moveaxis(a, (1, 3, 5), (3, 4, 5))
    return a.reshape((cx, cy, cz, f ** 3) + rest)


def oracle(sigma, label, f, voxel_size, n_classes):
    """f64 scores (cx, cy, cz, n_classes) at mean scale, labels under torch.argmax's rule for
    finite scores (lowest index among equals), the top-two margin, and the max-pooled sigma."""
    s = sigma.astype(np.float64)
    # the kernel's exponent is the f32 product of f32(-voxel_size) and sigma
    t = (np.float32(-voxel_size) * sigma).astype(np.float64)
    alpha = 1.0 - np.exp(t)
    onehot = label[..., None] == np.arange(n_classes)
    scores = blocks(alpha[..., None] * onehot, f).mean(axis=3)
    labels = scores.argmax(-1).astype(np.uint8)
    top = np.sort(scores, axis=-1)
    margin = top[..., -1] - top[..., -2] if n_classes > 1 else np.full(labels.shape, np.inf)
    return scores, labels, margin, blocks(s, f).max(axis=3).astype(np.float32)


def hand_built(f=2):
    """Eight coarse voxels in a row along z, one rule each: returns the fine sigma (f, f, 8 f)
    f32 and label uint8, n_classes, the expected labels (8,) and the expected densities (8,)
    (NaN where the density must be NaN)."""
    n = 8
    sigma = np.zeros((f, f, n * f), np.float32)
    label = np.zeros((f, f, n * f), np.uint8)
    want = np.zeros(n, np.uint8)

    def vox(k):
        return sigma[:, :, k * f:(k + 1) * f], label[:, :, k * f:(k + 1) * f]
    # 0: all-zero densities with non-zero labels -> 0
    s, l = vox(0); l[...] = 7; want[0] = 0
    # 1: a single class
    s, l = vox(1); s[...] = 1.5; l[...] = 11; want[1] = 11
    # 2: an exact two-class tie (the same densities, mirrored) -> the lower class
    s, l = vox(2); s[...] = 0.75; l[:f // 2] = 9; l[f // 2:] = 4; want[2] = 4
    # 3: a NaN child: NaN density; its class is the first NaN score
    s, l = vox(3); s[...] = 2.0; l[...] = 3; s[0, 0, 0] = np.nan; l[0, 0, 0] = 12; want[3] = 12
    # 4: two NaN classes: the first (lowest) one wins, although 17 has the larger finite share
    s, l = vox(4); s[...] = 2.0; l[...] = 17; s[0, 0, 0] = np.nan; l[0, 0, 0] = 12
    s[-1, -1, -1] = np.nan; l[-1, -1, -1] = 5; want[4] = 5
    # 5: labels >= n_classes are ignored (their density still pools)
    s, l = vox(5); s[...] = 3.0; l[...] = 200; s[0, 0, 0] = 0.25; l[0, 0, 0] = 2; want[5] = 2
    # 6: the weights decide, not the head count
    s, l = vox(6); s[...] = 0.01; l[...] = 1; s[0, 0, 0] = 9.0; l[0, 0, 0] = 18; want[6] = 18
    # 7: only ignored labels -> all scores 0 -> 0
    s, l = vox(7); s[...] = 1.0; l[...] = 19; want[7] = 0
    want_sigma = np.array([0.0, 1.5, 0.75, np.nan, np.nan, 3.0, 9.0, 1.0], np.float32)
    return sigma, label, 19, want, want_sigma
