// sdhip_metrics.hip -- the evaluation metrics of scenedino/common/metrics.py on gfx950 (CDNA4),
// each as one fused pass with no host read (include/sdhip_metrics.h):
//
//   sd_depth_metrics  compute_depth_metrics (:49-113).  The reference makes about twenty
//                     full-map elementwise passes; here a workgroup reads 2048 pixels of gt and
//                     pred once, forms the reference's f32 terms per pixel (IEEE division, logf)
//                     and keeps their sums in f64, the threshold and valid counts in integers.
//                     Grid (parts, n); k_depth_final adds an image's partials in order.
//   sd_dino_metrics   compute_dino_metrics (:195-215).  The bandwidth path: one wave per row of
//                     C channels, 16-byte loads, both tensors read once.  |p - g| and (p - g)^2
//                     stay in per-lane f64 sums over the wave's rows; only the three sums of the
//                     cosine cross lanes per row.  A workgroup's rows lie in one (n, v) slab, so
//                     its partial belongs to one view; k_dino_final adds a view's partials in
//                     order and forms the row of means.
//   sd_seg_confusion  compute_seg_metrics (:230-247) for up to 8 results: the target is read
//                     once, one LDS histogram per workgroup for all results (integer LDS
//                     atomics), flushed with one integer global atomic per non-zero bin.
//
// No floating-point atomics anywhere: a repeated launch gives the same bits.
#include "sdhip_common.h"

#include "../../include/sdhip_metrics.h"

extern "C" void sd_set_error(const char *msg);

typedef __attribute__((ext_vector_type(4))) float mt_f4;
typedef __attribute__((ext_vector_type(4))) uint32_t mt_u4;

// wave sums in a fixed (butterfly) order
__device__ __forceinline__ double mt_wave_sum(double x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    return x;
}
__device__ __forceinline__ float mt_wave_sum(float x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    return x;
}
__device__ __forceinline__ int mt_wave_sum(int x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// ---------------------------------------------------------------------------
// depth
// ---------------------------------------------------------------------------
#define DM_CHUNK 2048      // pixels per workgroup: 8 per thread
#define DM_WORDS 8         // f64 words per partial: 4 sums, 4 counts
#define DM_MAX_HW ((int64_t)1 << 24)

static __host__ __device__ inline int64_t dm_parts(int64_t hw) { return (hw + DM_CHUNK - 1) / DM_CHUNK; }

__global__ void __launch_bounds__(256) k_depth_partial(const float *__restrict__ gt, int64_t gt_stride,
                                                       const float *__restrict__ pred,
                                                       int64_t pred_stride, int64_t hw,
                                                       double *__restrict__ work) {
    __shared__ double sh[4][DM_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t img = blockIdx.y, part = blockIdx.x;
    const float *g = gt + img * gt_stride, *p = pred + img * pred_stride;
    const int64_t i0 = part * DM_CHUNK;
    float gv[8], pv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int64_t i = i0 + tid + 256 * j;
        const bool in = i < hw;
        gv[j] = in ? g[i] : 0.f;  // gt 0: not a valid pixel
        pv[j] = in ? p[i] : 1.f;
    }
    double s_abs = 0.0, s_sq = 0.0, s_rmse = 0.0, s_log = 0.0;
    int n1 = 0, n2 = 0, n3 = 0, nv = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float y = gv[j];
        float x = pv[j];
        x = x < 1e-3f ? 1e-3f : (x > 80.f ? 80.f : x);  // torch.clamp: a NaN stays a NaN
        if (y != 0.f) {
            const float ra = y / x, rb = x / y;
            const float r = (ra > rb || ra != ra) ? ra : rb;  // torch.maximum: NaN wins
            n1 += r < 1.25f;
            n2 += r < 1.5625f;
            n3 += r < 1.953125f;
            const float d = y - x, sq = d * d;
            const float dl = logf(y) - logf(x);
            s_rmse += (double)sq;
            s_log += (double)(dl * dl);
            s_abs += (double)(fabsf(d) / y);
            s_sq += (double)(sq / y);
            ++nv;
        }
    }
    s_abs = mt_wave_sum(s_abs); s_sq = mt_wave_sum(s_sq);
    s_rmse = mt_wave_sum(s_rmse); s_log = mt_wave_sum(s_log);
    n1 = mt_wave_sum(n1); n2 = mt_wave_sum(n2); n3 = mt_wave_sum(n3); nv = mt_wave_sum(nv);
    if (lane == 0) {
        sh[wave][0] = s_abs; sh[wave][1] = s_sq; sh[wave][2] = s_rmse; sh[wave][3] = s_log;
        sh[wave][4] = (double)n1; sh[wave][5] = (double)n2; sh[wave][6] = (double)n3;
        sh[wave][7] = (double)nv;
    }
    __syncthreads();
    if (tid < DM_WORDS)
        work[(img * gridDim.x + part) * DM_WORDS + tid] =
            ((sh[0][tid] + sh[1][tid]) + sh[2][tid]) + sh[3][tid];
}

// one wave per image: the partials added in order (lane-strided, then the butterfly)
__global__ void __launch_bounds__(64) k_depth_final(const double *__restrict__ work, int64_t parts,
                                                    float *__restrict__ out) {
    const int lane = threadIdx.x;
    const int64_t img = blockIdx.x;
    const double *w = work + img * parts * DM_WORDS;
    double s[DM_WORDS];
#pragma unroll
    for (int q = 0; q < DM_WORDS; ++q) s[q] = 0.0;
    for (int64_t k = lane; k < parts; k += 64)
#pragma unroll
        for (int q = 0; q < DM_WORDS; ++q) s[q] += w[k * DM_WORDS + q];
#pragma unroll
    for (int q = 0; q < DM_WORDS; ++q) s[q] = mt_wave_sum(s[q]);
    if (lane != 0) return;
    const double cnt = s[7];  // 0 / 0 = NaN for an image without a valid pixel, as the reference
    float *o = out + img * 8;
    o[0] = (float)sqrt(s[0] / cnt);
    o[1] = (float)sqrt(s[1] / cnt);
    o[2] = (float)sqrt(s[2] / cnt);
    o[3] = (float)sqrt(s[3] / cnt);
    o[4] = (float)(s[4] / cnt);
    o[5] = (float)(s[5] / cnt);
    o[6] = (float)(s[6] / cnt);
    o[7] = (float)cnt;
}

static bool dm_shape_ok(int64_t n, int64_t hw) { return n >= 1 && n <= 65535 && hw >= 1 && hw <= DM_MAX_HW; }

extern "C" int64_t sd_depth_metrics_work(int64_t n, int64_t hw) {
    if (!dm_shape_ok(n, hw)) {
        sd_set_error("sd_depth_metrics_work: invalid argument (1 <= n <= 65535, 1 <= hw <= 2^24)");
        return -1;
    }
    return n * dm_parts(hw) * DM_WORDS * (int64_t)sizeof(double);
}

extern "C" int sd_depth_metrics(const float *gt, int64_t gt_stride, const float *pred,
                                int64_t pred_stride, int64_t n, int64_t hw, void *work, float *out,
                                void *stream) {
    if (!gt || !pred || !work || !out || !dm_shape_ok(n, hw) || gt_stride < hw || pred_stride < hw ||
        (((uintptr_t)gt | (uintptr_t)pred | (uintptr_t)work | (uintptr_t)out) & 15)) {
        sd_set_error("sd_depth_metrics: invalid argument (1 <= n <= 65535, 1 <= hw <= 2^24, image "
                     "strides >= hw, 16-B aligned gt / pred / work / out)");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    const int64_t parts = dm_parts(hw);
    hipLaunchKernelGGL(k_depth_partial, dim3((unsigned)parts, (unsigned)n), dim3(256), 0, s, gt,
                       gt_stride, pred, pred_stride, hw, (double *)work);
    hipLaunchKernelGGL(k_depth_final, dim3((unsigned)n), dim3(64), 0, s, (const double *)work, parts,
                       out);
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_depth_metrics: launch failed");
        return -2;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// dino
// ---------------------------------------------------------------------------
#define DN_MAX_BPS 1024    // workgroups per (n, v) slab
#define DN_MIN_ROWS 16     // rows per workgroup below which the slab gets fewer workgroups
#define DN_MAX_V 64
#define DN_EPS 1e-8f       // F.cosine_similarity's default eps

struct dn_plan {
    int64_t per;  // rows per workgroup
    int bps;      // workgroups per slab
};

static __host__ __device__ inline dn_plan dn_make_plan(int64_t P) {
    dn_plan q;
    int64_t bps = (P + DN_MIN_ROWS - 1) / DN_MIN_ROWS;
    if (bps > DN_MAX_BPS) bps = DN_MAX_BPS;
    q.per = (P + bps - 1) / bps;
    q.bps = (int)((P + q.per - 1) / q.per);
    return q;
}

// X16: pred is bf16.  A lane owns 4 (f32) or 8 (bf16) consecutive channels per step: one 16-byte
// load of pred, one or two of gt; C / 4 <= 192 (3 steps), C / 8 <= 96 (2 steps).
template <bool X16>
__global__ void __launch_bounds__(256) k_dino_partial(const void *__restrict__ pred,
                                                      const float *__restrict__ gt, int64_t P, int C,
                                                      int64_t per, double *__restrict__ work) {
    __shared__ double sh[4][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t slab = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * per;
    const int64_t r1 = r0 + per < P ? r0 + per : P;
    constexpr int W = X16 ? 8 : 4, NJ = X16 ? 2 : 3;
    const int nchunk = C / W;
    double a1 = 0.0, a2 = 0.0, ac = 0.0;
    for (int64_t r = r0 + wave; r < r1; r += 4) {
        const int64_t base = (slab * P + r) * C;
        float l1 = 0.f, l2 = 0.f, dot = 0.f, np = 0.f, ng = 0.f;
        float pv[NJ][W], gv[NJ][W];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = lane + 64 * j;
#pragma unroll
            for (int i = 0; i < W; ++i) pv[j][i] = gv[j][i] = 0.f;
            if (c < nchunk) {
                const int64_t e = base + (int64_t)c * W;
                if (X16) {
                    const mt_u4 h = *(const mt_u4 *)((const uint16_t *)pred + e);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        pv[j][2 * i] = bf16lo(h[i]);
                        pv[j][2 * i + 1] = bf16hi(h[i]);
                    }
                    const mt_f4 g0 = *(const mt_f4 *)(gt + e), g1 = *(const mt_f4 *)(gt + e + 4);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        gv[j][i] = g0[i];
                        gv[j][4 + i] = g1[i];
                    }
                } else {
                    const mt_f4 p0 = *(const mt_f4 *)((const float *)pred + e);
                    const mt_f4 g0 = *(const mt_f4 *)(gt + e);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        pv[j][i] = p0[i];
                        gv[j][i] = g0[i];
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const float x = pv[j][i], y = gv[j][i], d = x - y;
                l1 += fabsf(d);
                l2 = fmaf(d, d, l2);
                dot = fmaf(x, y, dot);
                np = fmaf(x, x, np);
                ng = fmaf(y, y, ng);
            }
        a1 += (double)l1;
        a2 += (double)l2;
        // the lanes' f32 partials (at most 12 channels each) cross the wave in f64:
        // x1 / max(|x1|, eps) . x2 / max(|x2|, eps)
        const double sd = mt_wave_sum((double)dot);
        const double sp = mt_wave_sum((double)np), sg = mt_wave_sum((double)ng);
        ac += sd / (fmax(sqrt(sp), (double)DN_EPS) * fmax(sqrt(sg), (double)DN_EPS));
    }
    a1 = mt_wave_sum(a1);
    a2 = mt_wave_sum(a2);
    if (lane == 0) {
        sh[wave][0] = a1; sh[wave][1] = a2; sh[wave][2] = ac;  // ac: the same in every lane
    }
    __syncthreads();
    if (tid < 3)
        work[(slab * gridDim.x + blockIdx.x) * 3 + tid] =
            ((sh[0][tid] + sh[1][tid]) + sh[2][tid]) + sh[3][tid];
}

// wave w adds the partials of views w, w + 4, ... (image by image, lane-strided over the slab's
// workgroups, then the butterfly); thread q < 3 then forms the row of means
__global__ void __launch_bounds__(256) k_dino_final(const double *__restrict__ work, int64_t n, int v,
                                                    int64_t P, int C, int bps,
                                                    float *__restrict__ out) {
    __shared__ float rows[DN_MAX_V][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int j = wave; j < v; j += 4) {
        double s[3] = {0.0, 0.0, 0.0};
        for (int64_t i = 0; i < n; ++i) {
            const double *w = work + (i * v + j) * bps * 3;
            for (int k = lane; k < bps; k += 64)
#pragma unroll
                for (int q = 0; q < 3; ++q) s[q] += w[k * 3 + q];
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) s[q] = mt_wave_sum(s[q]);
        if (lane == 0) {
            const double rows_n = (double)n * (double)P;
            rows[j][0] = (float)(s[0] / (rows_n * (double)C));
            rows[j][1] = (float)(s[1] / (rows_n * (double)C));
            rows[j][2] = (float)(s[2] / rows_n);
#pragma unroll
            for (int q = 0; q < 3; ++q) out[j * 3 + q] = rows[j][q];
        }
    }
    __syncthreads();
    if (tid < 3) {
        float m = 0.f;
        for (int j = 0; j < v; ++j) m += rows[j][tid];
        out[v * 3 + tid] = m / (float)v;
    }
}

static bool dn_shape_ok(int64_t n, int64_t v, int64_t P, int32_t C) {
    return n >= 1 && v >= 1 && v <= DN_MAX_V && P >= 1 && C >= 64 && C <= 768 && C % 64 == 0 &&
           n <= 65535 / v && n * v <= ((int64_t)1 << 40) / P;
}

extern "C" int64_t sd_dino_metrics_work(int64_t n, int64_t v, int64_t P, int32_t C) {
    if (!dn_shape_ok(n, v, P, C)) {
        sd_set_error("sd_dino_metrics_work: invalid argument (n, v, P >= 1, v <= 64, n v <= 65535, "
                     "n v P <= 2^40, 64 <= C <= 768, C % 64 == 0)");
        return -1;
    }
    return n * v * dn_make_plan(P).bps * 3 * (int64_t)sizeof(double);
}

extern "C" int sd_dino_metrics(const void *pred, int32_t pred_dtype, const float *gt, int64_t n,
                               int64_t v, int64_t P, int32_t C, void *work, float *out,
                               void *stream) {
    if (!pred || !gt || !work || !out || !dn_shape_ok(n, v, P, C) ||
        (pred_dtype != SD_F32 && pred_dtype != SD_BF16) ||
        (((uintptr_t)pred | (uintptr_t)gt | (uintptr_t)work | (uintptr_t)out) & 15)) {
        sd_set_error("sd_dino_metrics: invalid argument (n, v, P >= 1, v <= 64, n v <= 65535, "
                     "n v P <= 2^40, 64 <= C <= 768, C % 64 == 0, pred f32 or bf16, 16-B aligned "
                     "pred / gt / work / out)");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    const dn_plan q = dn_make_plan(P);
    const dim3 grid((unsigned)q.bps, (unsigned)(n * v));
    if (pred_dtype == SD_BF16)
        hipLaunchKernelGGL(k_dino_partial<true>, grid, dim3(256), 0, s, pred, gt, P, (int)C, q.per,
                           (double *)work);
    else
        hipLaunchKernelGGL(k_dino_partial<false>, grid, dim3(256), 0, s, pred, gt, P, (int)C, q.per,
                           (double *)work);
    hipLaunchKernelGGL(k_dino_final, dim3(1), dim3(256), 0, s, (const double *)work, n, (int)v, P,
                       (int)C, q.bps, out);
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_dino_metrics: launch failed");
        return -2;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// segmentation
// ---------------------------------------------------------------------------
#define SG_PIXELS 4096     // pixels per workgroup and sweep: 16 per thread
#define SG_MAX_WG 1024

__global__ void __launch_bounds__(256) k_seg_confusion(const sd_seg_confusion_args a) {
    __shared__ uint32_t hist[SD_SEG_MAX_BINS + 1];
    const int per = a.gt_classes * a.n_classes, nbins = a.n_results * per;
    for (int i = threadIdx.x; i <= nbins; i += 256) hist[i] = 0;
    __syncthreads();
    const int64_t total = a.n * a.hw;
    uint32_t bad = 0;
    for (int64_t i0 = (int64_t)blockIdx.x * SG_PIXELS; i0 < total; i0 += (int64_t)gridDim.x * SG_PIXELS) {
#pragma unroll 4
        for (int j = 0; j < SG_PIXELS / 256; ++j) {
            const int64_t i = i0 + threadIdx.x + 256 * j;
            if (i >= total) break;
            const int64_t t = a.target[i];
            if (t < 0) continue;  // dropped with its predictions, whatever they are
            const int64_t img = i / a.hw, px = i - img * a.hw;
            const bool t_ok = t < a.gt_classes;
            bool p_ok = true;
            for (int r = 0; r < a.n_results; ++r) {
                const int64_t p = a.pred[r][img * a.pred_stride[r] + px];
                if ((uint64_t)p < (uint64_t)a.n_classes) {
                    if (t_ok) atomicAdd(&hist[r * per + (int)t * a.n_classes + (int)p], 1u);
                } else {
                    p_ok = false;
                }
            }
            bad += !(t_ok && p_ok);
        }
    }
    if (bad) atomicAdd(&hist[nbins], bad);
    __syncthreads();
    for (int i = threadIdx.x; i <= nbins; i += 256) {
        const uint32_t c = hist[i];
        if (c) atomicAdd((uint32_t *)a.conf + i, c);
    }
}

extern "C" int sd_seg_confusion(const sd_seg_confusion_args *a, void *stream) {
    bool ok = a && a->target && a->conf && a->n_results >= 1 && a->n_results <= SD_SEG_MAX_RESULTS &&
              a->n >= 1 && a->hw >= 1 && a->n <= ((int64_t)1 << 40) / a->hw && a->gt_classes >= 1 &&
              a->n_classes >= 1 && a->gt_classes <= SD_SEG_MAX_BINS &&
              a->n_classes <= SD_SEG_MAX_BINS &&
              (int64_t)a->n_results * a->gt_classes * a->n_classes <= SD_SEG_MAX_BINS &&
              !(((uintptr_t)a->target | (uintptr_t)a->conf) & 15);
    for (int r = 0; ok && r < a->n_results; ++r)
        ok = a->pred[r] && !((uintptr_t)a->pred[r] & 15) && a->pred_stride[r] >= a->hw;
    if (!ok) {
        sd_set_error("sd_seg_confusion: invalid argument (1 <= n_results <= 8, n, hw >= 1, "
                     "n hw <= 2^40, n_results gt_classes n_classes <= 8192, prediction strides >= hw, "
                     "16-B aligned target / predictions / conf)");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    const int nbins = a->n_results * a->gt_classes * a->n_classes;
    if (hipMemsetAsync(a->conf, 0, (size_t)(nbins + 1) * sizeof(int32_t), s) != hipSuccess) {
        sd_set_error("sd_seg_confusion: memset failed");
        return -2;
    }
    int64_t nwg = (a->n * a->hw + SG_PIXELS - 1) / SG_PIXELS;
    if (nwg > SG_MAX_WG) nwg = SG_MAX_WG;
    hipLaunchKernelGGL(k_seg_confusion, dim3((unsigned)nwg), dim3(256), 0, s, *a);
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_seg_confusion: launch failed");
        return -2;
    }
    return 0;
}
