/* sdhip_ssc_pool.h -- C ABI of the SSCBench fine-to-coarse voxel pooling kernel
 * (scenedino_amd/csrc/sdhip_ssc_pool.hip), part of libsdhip.so beside include/sdhip.h: the
 * reduction of sscbench/evaluate_model_sscbench.py:727-745 (alpha-weighted one-hot class votes
 * average-pooled, densities max-pooled, kernel = stride = downsample factor) for a field queried
 * on a grid `factor` times finer than the scored one.
 *
 * Conventions of sdhip.h hold: the entry point validates its arguments before any launch and
 * returns -1 with sd_last_error() text, -2 if the launch failed, 0 otherwise; every pointer is
 * 16-byte aligned and on the device; `stream` is a hipStream_t.  One launch, no scratch buffer,
 * no atomics: a coarse voxel belongs to one lane that walks its children in a fixed order, so a
 * repeated call gives the same bits.
 */
#ifndef SDHIP_SSC_POOL_H
#define SDHIP_SSC_POOL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* sigma_f (f cx, f cy, f cz) f32 and seg_f (f cx, f cy, f cz) uint8 are the fine densities and
 * per-point class ids, sigma_out / seg_out (cx, cy, cz) the pooled ones; all z-fastest and
 * contiguous.  voxel_size is the fine voxel's edge.  Per coarse voxel (I, J, K), f = factor:
 *   children   the f^3 fine voxels (f I + a, f J + b, f K + c), 0 <= a, b, c < f
 *   alpha      1.0f - expf(t), t the f32 product of (float)(-voxel_size) and sigma (separately
 *              rounded; the accurate expf): 1 - torch.exp(-VOXEL_SIZE * sigmas_block)
 *   score[c]   the f32 sum of alpha over the children with seg_f == c, added in ascending
 *              (a, b, c) order, then divided by f^3: F.avg_pool3d of alpha * one_hot(seg_f) bit
 *              for bit.  A child with seg_f >= n_classes votes for no class (its density still
 *              counts below).
 *   seg_out    argmax_c score[c] over all n_classes, absent classes included (score 0), under
 *              torch.argmax's rule: the lowest index among equals, a NaN score counts as the
 *              maximum (the first NaN class wins); an all-zero voxel gives 0.
 *   sigma_out  the max over the children, NaN propagating: F.max_pool3d(kernel f, stride f), the
 *              rule of sd_grow3.
 * Every element of sigma_out and seg_out is written; nothing else is.
 * Domain: factor in {2, 4, 8}; 1 <= n_classes <= SD_SSC_POOL_MAX_CLASSES; cx, cy, cz > 0 with
 * f^3 cx cy cz < 2^31; voxel_size finite and > 0; the outputs overlap neither an input nor
 * each other. */
#define SD_SSC_POOL_MAX_CLASSES 32
int sd_ssc_pool(const float *sigma_f, const uint8_t *seg_f, int64_t cx, int64_t cy, int64_t cz,
                int32_t factor, float voxel_size, int32_t n_classes, float *sigma_out,
                uint8_t *seg_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SDHIP_SSC_POOL_H */
