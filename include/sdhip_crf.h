/* sdhip_crf.h -- C ABI of the dense-CRF kernels (scenedino_amd/csrc/sdhip_crf.hip), part of
 * libsdhip.so beside include/sdhip.h: mean-field inference of a fully connected CRF with a
 * Gaussian and a bilateral Potts potential (pydensecrf's DenseCRF2D with its default arguments,
 * scenedino/downstream_head/crf.py), the pair sums evaluated exactly instead of on the
 * permutohedral lattice, for up to 8 results of one image in one call.
 *
 * Conventions of sdhip.h hold: an entry point validates its arguments before any launch and
 * returns -1 with sd_last_error() text, -2 if a launch failed, 0 otherwise; every pointer is
 * 16-byte aligned; the scratch size comes from sd_dense_crf_work; no floating-point atomics: a
 * query tile belongs to one workgroup that walks its key blocks in ascending order, so a
 * repeated call gives the same bits.  `stream` is a hipStream_t.
 */
#ifndef SDHIP_CRF_H
#define SDHIP_CRF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One image of N = H W pixels (pixel i at x = i % W, y = i / W), uint8 colours (H, W, 3), and
 * n_results results; result r has classes[r] classes and its columns start at
 * off_r = classes[0] + ... + classes[r - 1] of the packed column axis (CT = off_{n_results}).
 *   unary  (CT, N) f32, class-major: U_i(c) of result r at unary[(off_r + c) N + i]
 *   k^g_ij = exp(-((dx^2 + dy^2) / sxy_g^2) / 2)
 *   k^b_ij = exp(-((dx^2 + dy^2) / sxy_b^2 + (dr^2 + dg^2 + db^2) / srgb^2) / 2)   (j = i included)
 *   n^p_i  = (sum_j k^p_ij + 1e-20)^(-1/2)
 *   Q^0_i  = softmax_c(-U_i)
 *   Q^{t+1}_i = softmax_c(-U_i(c) + sum_p w_p n^p_i sum_j k^p_ij n^p_j Q^t_j(c)),  t < iters
 *   labels (n_results, N) int64: labels[r N + i] = argmax_c Q^{iters}_i(c), lowest index on a tie
 *   q      NULL, or (CT, N) f32 laid out as unary: Q^{iters}
 * Every element of labels (and of q) is written; nothing else is, outside `work`.
 *
 * Numerics.  The squared distances are sums of integer products in f32 (exact for |dx|, |dy| <
 * 2^11 and any uint8 colours), so the exponent is formed from exact terms; no |f_i|^2 + |f_j|^2
 * - 2 f_i.f_j cancellation.  The bilateral weights (in [0, 1]) and n^b_j Q_j are rounded to f16
 * for the weights x Q product on MFMA; accumulation, unaries, norms and softmax are f32 (the
 * bilateral row sums of n^b in f64).  The bilateral sums drop a pair only where its spatial
 * factor is <= 1e-7, a distance >= 5.68 sxy_b (whole 32-key blocks outside that window are
 * skipped); the Gaussian term is a stencil of radius ceil(5.68 sxy_g) under the same rule.
 *
 * One launch per mean-field iteration (plus set-up: features, norms, Q^0); Q ping-pongs in
 * `work`, which needs no initialisation by the caller.
 * Domain: 1 <= H, W <= 4096, H W <= 2^20, 1 <= n_results <= 8, 2 <= classes[r] <= 64,
 * 0 <= iters <= 64, sxy_b > 0, srgb > 0, 0 < sxy_g <= SD_CRF_MAX_SXY_G (stencil radius <= 4),
 * w_g, w_b finite and >= 0. */
#define SD_CRF_MAX_RESULTS 8
#define SD_CRF_MAX_CLASSES 64
#define SD_CRF_MAX_SXY_G 0.7f
typedef struct sd_crf_args {
    const uint8_t *image;  /* (H, W, 3) */
    const float *unary;    /* (CT, N) */
    void *work;            /* sd_dense_crf_work bytes */
    int64_t *labels;       /* (n_results, N) */
    float *q;              /* NULL or (CT, N) */
    int32_t H, W, n_results, iters;
    int32_t classes[SD_CRF_MAX_RESULTS];
    float w_g, sxy_g, w_b, sxy_b, srgb, pad_;
} sd_crf_args;
int64_t sd_dense_crf_work(int32_t H, int32_t W, int32_t n_results, const int32_t *classes);
int sd_dense_crf(const sd_crf_args *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SDHIP_CRF_H */
