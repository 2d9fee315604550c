/* sdhip_metrics.h -- C ABI of the evaluation-metric kernels (scenedino_amd/csrc/
 * sdhip_metrics.hip), part of libsdhip.so beside include/sdhip.h: the per-image depth scores,
 * the per-view DINO feature scores and the segmentation confusion matrices of
 * scenedino/common/metrics.py, each as one fused pass with no host read.
 *
 * Conventions of sdhip.h hold: an entry point validates its arguments before any launch and
 * returns -1 with sd_last_error() text, -2 if a launch failed, 0 otherwise; every pointer is
 * 16-byte aligned; scratch sizes come from the *_work function beside it; no floating-point
 * atomics: per-workgroup partial sums are added in workgroup order, so a repeated launch gives
 * the same bits.  `stream` is a hipStream_t.
 */
#ifndef SDHIP_METRICS_H
#define SDHIP_METRICS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* compute_depth_metrics (metrics.py:49-113) on n images of hw pixels, f32.  Image i of gt
 * starts at gt + i gt_stride, of pred at pred + i pred_stride (elements; pred is normally
 * view 0 of an (n, v, h, w) tensor: pred_stride = v hw), each image contiguous.
 *   p = clamp(pred, 1e-3, 80), valid = gt != 0, r = max(gt / p, p / gt)
 *   out row i (8 floats): abs_rel = sqrt(mean |gt - p| / gt), sq_rel = sqrt(mean (gt - p)^2 / gt)
 *   (square roots as the reference writes them), rmse, rmse_log, a1, a2, a3 = mean(r < 1.25^k),
 *   and the valid count; the means run over the valid pixels, so an image without one gives
 *   seven NaNs and count 0.
 * Per pixel the reference's f32 operations (IEEE division, logf); the sums are kept in f64
 * (the threshold and valid counts in integers), one partial per 2048 pixels in `work`
 * (sd_depth_metrics_work bytes), added in order by a second kernel and rounded to f32 once.
 * Domain: 1 <= n <= 65535, 1 <= hw <= 2^24, strides >= hw. */
int64_t sd_depth_metrics_work(int64_t n, int64_t hw);
int sd_depth_metrics(const float *gt, int64_t gt_stride, const float *pred, int64_t pred_stride,
                     int64_t n, int64_t hw, void *work, float *out, void *stream);

/* compute_dino_metrics (metrics.py:195-215): pred (n, v, P, C) in pred_dtype (SD_F32 or
 * SD_BF16), gt (n, v, P, C) f32, both contiguous.  out (v + 1, 3) f32: row j holds view j's
 *   l1  = mean over (n, P, C) of |pred - gt|,   l2 = mean of (pred - gt)^2,
 *   cos = mean over (n, P) of  <p, g> / (max(|p|, 1e-8) max(|g|, 1e-8))   (F.cosine_similarity)
 * and row v the three means over the views (view rows added in order in f32, divided by v).
 * One wave per row with 16-byte loads, every row of both tensors read once; a workgroup's rows
 * lie in one (n, v) slab and its three f64 partial sums go to `work` (sd_dino_metrics_work
 * bytes); a second kernel adds them in order.
 * Domain: n, v, P >= 1, v <= 64, C % 64 == 0, 64 <= C <= 768, n v P < 2^40. */
int64_t sd_dino_metrics_work(int64_t n, int64_t v, int64_t P, int32_t C);
int sd_dino_metrics(const void *pred, int32_t pred_dtype, const float *gt, int64_t n, int64_t v,
                    int64_t P, int32_t C, void *work, float *out, void *stream);

/* compute_seg_metrics (metrics.py:230-247) for up to 8 results at once: target (n, hw) int64
 * contiguous, prediction r image i at pred[r] + i pred_stride[r] (int64 elements; the stride
 * picks view 0 of an (n, v, hw) tensor).  conf holds n_results (gt_classes, n_classes) int32
 * matrices, conf[r][t][p] = number of pixels with target t >= 0 and prediction p, and one more
 * word: the number of pixels with target >= gt_classes or, with a target >= 0, any prediction
 * outside [0, n_classes) (such a pixel adds to no bin of the results it is out of range for;
 * the reference fails inside bincount / reshape on them).  conf is zeroed on the stream first;
 * the target is read once for all results.  Integer LDS histograms flushed with integer global
 * atomics: deterministic.
 * Domain: 1 <= n_results <= 8, n, hw >= 1, n hw < 2^40, gt_classes, n_classes >= 1,
 * n_results gt_classes n_classes <= 8192, pred_stride[r] >= hw. */
#define SD_SEG_MAX_RESULTS 8
#define SD_SEG_MAX_BINS 8192
typedef struct sd_seg_confusion_args {
    const int64_t *target;
    const int64_t *pred[SD_SEG_MAX_RESULTS];
    int64_t pred_stride[SD_SEG_MAX_RESULTS];
    int64_t n, hw;
    int32_t n_results, gt_classes, n_classes, pad_;
    int32_t *conf;         /* (n_results gt_classes n_classes + 1) */
} sd_seg_confusion_args;
int sd_seg_confusion(const sd_seg_confusion_args *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SDHIP_METRICS_H */
