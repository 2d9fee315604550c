// sdhip_crf.hip -- mean-field inference of the fully connected CRF of
// scenedino/downstream_head/crf.py on gfx950 (CDNA4), for up to 8 results of one image per call
// (include/sdhip_crf.h).  One iteration is Q' = softmax(-U + K.Q) with the N x N kernel matrix K
// never stored: the flash-attention loop without the row maximum.
//
//   k_crf_prep    per pixel: x, y, r, g, b as f32 (structure of arrays, padded to 64 pixels with a
//                 far-away position so that a padded key has weight 0) and the Gaussian norm n^g.
//   k_crf_sweep   one workgroup = 64 consecutive pixels (queries), one wave = 16 of them.  The
//                 workgroup walks the 32-key blocks of the linear pixel axis that meet the window
//                 |d| < 5.68 sxy_b around its queries, in ascending order, every block once.  Per
//                 block a lane forms the 8 bilateral weights of its (query, key group) from exact
//                 squared distances (f32 sums of integer products: no cancellation), which are the
//                 A fragment of mfma_f32_16x16x32_f16; the B fragments are 16-byte loads of n^b Q
//                 (f16, [column][pixel]), one per 16 packed class columns: the pair weights are
//                 paid once for all results.
//                 NORM = true: the same sweep summing the f32 weights in f64 (n^b), once per call.
//                 Otherwise the messages go to LDS and a thread per (query, result) adds the
//                 Gaussian stencil on the f32 Q, subtracts the unaries and takes the softmax.
//   k_crf_init    Q^0 = softmax(-U).
//
// One launch per iteration, Q ping-pongs in `work`; no floating-point atomics.
#include "sdhip_common.h"

#include "../../include/sdhip_crf.h"

#include <math.h>

extern "C" void sd_set_error(const char *msg);

typedef __attribute__((ext_vector_type(8))) _Float16 crf_h8;
typedef __attribute__((ext_vector_type(4))) float crf_f4;

#define CRF_TILE 64          // queries per workgroup
#define CRF_KB 32            // keys per block (one MFMA k step)
#define CRF_CHUNK 8          // 16-column tiles per sweep of the keys
#define CRF_TRUNC 5.68       // exp(-5.68^2 / 2) < 1e-7
#define CRF_FAR 1e8f         // position of a padded pixel
#define CRF_MAX_CUT2 1e8f    // window radius^2 clamp: beyond any 4096 x 4096 image
#define CRF_MAX_RG 4

struct crf_k {
    const float *feat;       // x, y, r, g, b at feat + k Npad
    const float *unary;
    float *nb, *ng;
    int H, W, N, Npad, R, CT, ntiles, ldm;
    int cls[SD_CRF_MAX_RESULTS], off[SD_CRF_MAX_RESULTS];
    float ea, ec;            // log2(e) / (2 sxy_b^2), log2(e) / (2 srgb^2)
    float cut2;              // (5.68 sxy_b)^2
    int rc;                  // ceil(5.68 sxy_b)
    float ga;                // 1 / (2 sxy_g^2)
    int rg;                  // ceil(5.68 sxy_g)
    float w_g, w_b;
};

struct crf_out {
    _Float16 *nq;            // next n^b Q, f16 (CTp, Npad), or NULL
    float *qf;               // next Q, f32 (CT, Npad), or NULL
    int64_t *labels;         // (R, N), or NULL (not the last iteration)
    float *q;                // (CT, N), or NULL
};

__global__ void __launch_bounds__(256) k_crf_prep(const uint8_t *__restrict__ image, crf_k p,
                                                  float *__restrict__ feat) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.Npad) return;
    float x = CRF_FAR, y = CRF_FAR, r = 0.f, g = 0.f, b = 0.f, ng = 0.f;
    if (i < p.N) {
        const int yi = i / p.W, xi = i - yi * p.W;
        x = (float)xi; y = (float)yi;
        r = (float)image[3 * (size_t)i]; g = (float)image[3 * (size_t)i + 1];
        b = (float)image[3 * (size_t)i + 2];
        float s = 0.f;
        for (int dy = -p.rg; dy <= p.rg; ++dy) {
            if ((unsigned)(yi + dy) >= (unsigned)p.H) continue;
            for (int dx = -p.rg; dx <= p.rg; ++dx)
                if ((unsigned)(xi + dx) < (unsigned)p.W) s += expf(-(float)(dx * dx + dy * dy) * p.ga);
        }
        ng = 1.f / sqrtf(s + 1e-20f);
    }
    feat[i] = x; feat[p.Npad + i] = y; feat[2 * (size_t)p.Npad + i] = r;
    feat[3 * (size_t)p.Npad + i] = g; feat[4 * (size_t)p.Npad + i] = b;
    p.ng[i] = ng;
}

// row: the c logits of (pixel i, result r) in LDS -> softmax, the next Q (f32 and n^b Q in f16),
// on the last iteration the label and Q^{iters}
__device__ __forceinline__ void crf_finish(const crf_k &p, const crf_out &o, float *row, int c, int cb,
                                           int r, int i, float nb_i) {
    float m = row[0];
    for (int k = 1; k < c; ++k) m = fmaxf(m, row[k]);
    float s = 0.f;
    for (int k = 0; k < c; ++k) {
        const float e = expf(row[k] - m);
        row[k] = e;
        s += e;
    }
    const float inv = 1.f / s;
    float best = -1.f;
    int am = 0;
    for (int k = 0; k < c; ++k) {
        const float q = row[k] * inv;
        if (q > best) { best = q; am = k; }
        if (o.qf) o.qf[(size_t)(cb + k) * p.Npad + i] = q;
        if (o.nq) o.nq[(size_t)(cb + k) * p.Npad + i] = (_Float16)(nb_i * q);
        if (o.q) o.q[(size_t)(cb + k) * p.N + i] = q;
    }
    if (o.labels) o.labels[(size_t)r * p.N + i] = am;
}

__global__ void __launch_bounds__(256) k_crf_init(crf_k p, crf_out o, int have_nb) {
    extern __shared__ float Ms[];
    const int p0 = blockIdx.x * CRF_TILE;
    for (int item = threadIdx.x; item < CRF_TILE * p.R; item += 256) {
        const int q = item & (CRF_TILE - 1), r = item >> 6, i = p0 + q;
        if (i >= p.N) continue;
        const int c = p.cls[r], cb = p.off[r];
        float *row = Ms + q * p.ldm + cb;
        for (int k = 0; k < c; ++k) row[k] = -p.unary[(size_t)(cb + k) * p.N + i];
        crf_finish(p, o, row, c, cb, r, i, have_nb ? p.nb[i] : 0.f);
    }
}

template <bool NORM>
__global__ void __launch_bounds__(256) k_crf_sweep(crf_k p, const _Float16 *__restrict__ nq_in,
                                                   const float *__restrict__ qf_in, crf_out o) {
    extern __shared__ float Ms[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = blockIdx.x * CRF_TILE;
    const int p1 = min(p0 + CRF_TILE - 1, p.N - 1);
    // the tile's bounding box: one row segment, or (wrapping a row end) the full width
    const int qy0 = p0 / p.W, qy1 = p1 / p.W;
    const int qx0 = qy0 == qy1 ? p0 - qy0 * p.W : 0;
    const int qx1 = qy0 == qy1 ? p1 - qy1 * p.W : p.W - 1;
    const int qi = p0 + 16 * wave + (lane & 15);  // < Npad
    const int kg = 8 * (lane >> 4);
    const size_t np = (size_t)p.Npad;
    const float xq = p.feat[qi], yq = p.feat[np + qi], rq = p.feat[2 * np + qi];
    const float gq = p.feat[3 * np + qi], bq = p.feat[4 * np + qi];
    const int ky_lo = max(0, qy0 - p.rc), ky_hi = min(p.H - 1, qy1 + p.rc);
    double rs = 0.0;
    const int nchunk = NORM ? 1 : (p.ntiles + CRF_CHUNK - 1) / CRF_CHUNK;
    for (int chunk = 0; chunk < nchunk; ++chunk) {
        const int t0 = chunk * CRF_CHUNK;
        const int nt = min(CRF_CHUNK, p.ntiles - t0);
        crf_f4 acc[CRF_CHUNK];
#pragma unroll
        for (int t = 0; t < CRF_CHUNK; ++t) acc[t] = crf_f4{0.f, 0.f, 0.f, 0.f};
        int next_b = 0;
        for (int ky = ky_lo; ky <= ky_hi; ++ky) {
            const int dy = ky < qy0 ? qy0 - ky : (ky > qy1 ? ky - qy1 : 0);
            const float rem = p.cut2 - (float)dy * (float)dy;
            if (!(rem > 0.f)) continue;        // every pair of this row is at >= the cut
            const int hx = (int)sqrtf(rem) + 1;  // |dx| >= hx: d^2 >= the cut
            const int xlo = max(0, qx0 - hx), xhi = min(p.W - 1, qx1 + hx);
            const int b_lo = max((ky * p.W + xlo) / CRF_KB, next_b);
            const int b_hi = (ky * p.W + xhi) / CRF_KB;
            for (int b = b_lo; b <= b_hi; ++b) {
                const int k0 = b * CRF_KB + kg;
                float kx[8], kyv[8], kr[8], kgr[8], kb[8];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const crf_f4 vx = *(const crf_f4 *)(p.feat + k0 + 4 * h);
                    const crf_f4 vy = *(const crf_f4 *)(p.feat + np + k0 + 4 * h);
                    const crf_f4 vr = *(const crf_f4 *)(p.feat + 2 * np + k0 + 4 * h);
                    const crf_f4 vg = *(const crf_f4 *)(p.feat + 3 * np + k0 + 4 * h);
                    const crf_f4 vb = *(const crf_f4 *)(p.feat + 4 * np + k0 + 4 * h);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        kx[4 * h + j] = vx[j]; kyv[4 * h + j] = vy[j]; kr[4 * h + j] = vr[j];
                        kgr[4 * h + j] = vg[j]; kb[4 * h + j] = vb[j];
                    }
                }
                float w[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float dx = xq - kx[j], dyf = yq - kyv[j];
                    const float dr = rq - kr[j], dg = gq - kgr[j], db = bq - kb[j];
                    const float s2 = fmaf(dyf, dyf, dx * dx);                  // exact integers
                    const float c2 = fmaf(db, db, fmaf(dg, dg, dr * dr));
                    w[j] = __builtin_amdgcn_exp2f(-fmaf(s2, p.ea, c2 * p.ec));
                }
                if (NORM) {
                    if (k0 + 8 > p.N)  // padded keys: far away, but sxy_b may be farther
#pragma unroll
                        for (int j = 0; j < 8; ++j) w[j] = k0 + j < p.N ? w[j] : 0.f;
                    rs += (double)(((w[0] + w[1]) + (w[2] + w[3])) + ((w[4] + w[5]) + (w[6] + w[7])));
                } else {
                    crf_h8 a;
#pragma unroll
                    for (int j = 0; j < 8; ++j) a[j] = (_Float16)w[j];
#pragma unroll
                    for (int t = 0; t < CRF_CHUNK; ++t)
                        if (t < nt) {
                            const crf_h8 bf = *(const crf_h8 *)(nq_in + (size_t)(16 * (t0 + t) + (lane & 15)) * np + k0);
                            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bf, acc[t], 0, 0, 0);
                        }
                }
            }
            if (b_hi >= next_b) next_b = b_hi + 1;
        }
        if (!NORM) {
            // C layout: column lane & 15, row 4 (lane >> 4) + reg
#pragma unroll
            for (int t = 0; t < CRF_CHUNK; ++t)
                if (t < nt)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        Ms[(16 * wave + 4 * (lane >> 4) + g) * p.ldm + 16 * (t0 + t) + (lane & 15)] = acc[t][g];
        }
    }
    if (NORM) {
        rs += __shfl_xor(rs, 16);
        rs += __shfl_xor(rs, 32);
        if (lane < 16 && qi < p.N) p.nb[qi] = (float)(1.0 / sqrt(rs + 1e-20));
        return;
    }
    __syncthreads();
    for (int item = tid; item < CRF_TILE * p.R; item += 256) {
        const int q = item & (CRF_TILE - 1), r = item >> 6, i = p0 + q;
        if (i >= p.N) continue;
        const int c = p.cls[r], cb = p.off[r];
        float *row = Ms + q * p.ldm + cb;
        const float nb_i = p.nb[i], sb = p.w_b * nb_i;
        for (int k = 0; k < c; ++k) row[k] = fmaf(sb, row[k], -p.unary[(size_t)(cb + k) * p.N + i]);
        const int yi = i / p.W, xi = i - yi * p.W;
        const float sg = p.w_g * p.ng[i];
        for (int dy = -p.rg; dy <= p.rg; ++dy) {
            if ((unsigned)(yi + dy) >= (unsigned)p.H) continue;
            for (int dx = -p.rg; dx <= p.rg; ++dx) {
                if ((unsigned)(xi + dx) >= (unsigned)p.W) continue;
                const int j = i + dy * p.W + dx;
                const float kw = sg * expf(-(float)(dx * dx + dy * dy) * p.ga) * p.ng[j];
                for (int k = 0; k < c; ++k) row[k] = fmaf(kw, qf_in[(size_t)(cb + k) * np + j], row[k]);
            }
        }
        crf_finish(p, o, row, c, cb, r, i, nb_i);
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
struct crf_plan {
    int64_t N, Npad;
    int CT, CTp;
    int off[SD_CRF_MAX_RESULTS];
    int64_t o_feat, o_nb, o_ng, o_qf, o_nq, qf_bytes, nq_bytes, total;
};

static bool crf_make_plan(int32_t H, int32_t W, int32_t R, const int32_t *classes, crf_plan &q) {
    if (H < 1 || H > 4096 || W < 1 || W > 4096 || (int64_t)H * W > ((int64_t)1 << 20) || R < 1 ||
        R > SD_CRF_MAX_RESULTS || !classes)
        return false;
    q.N = (int64_t)H * W;
    q.Npad = (q.N + CRF_TILE - 1) / CRF_TILE * CRF_TILE;
    q.CT = 0;
    for (int r = 0; r < R; ++r) {
        if (classes[r] < 2 || classes[r] > SD_CRF_MAX_CLASSES) return false;
        q.off[r] = q.CT;
        q.CT += classes[r];
    }
    q.CTp = (q.CT + 15) / 16 * 16;
    auto up = [](int64_t b) { return (b + 255) / 256 * 256; };
    q.qf_bytes = up((int64_t)q.CT * q.Npad * 4);
    q.nq_bytes = up((int64_t)q.CTp * q.Npad * 2);
    q.o_feat = 0;
    q.o_nb = q.o_feat + up(5 * q.Npad * 4);
    q.o_ng = q.o_nb + up(q.Npad * 4);
    q.o_qf = q.o_ng + up(q.Npad * 4);
    q.o_nq = q.o_qf + 2 * q.qf_bytes;
    q.total = q.o_nq + 2 * q.nq_bytes;
    return true;
}

extern "C" int64_t sd_dense_crf_work(int32_t H, int32_t W, int32_t n_results, const int32_t *classes) {
    crf_plan q;
    if (!crf_make_plan(H, W, n_results, classes, q)) {
        sd_set_error("sd_dense_crf_work: invalid argument (1 <= H, W <= 4096, H W <= 2^20, "
                     "1 <= n_results <= 8, 2 <= classes[r] <= 64)");
        return -1;
    }
    return q.total;
}

extern "C" int sd_dense_crf(const sd_crf_args *a, void *stream) {
    crf_plan q;
    auto pos = [](float v) { return v > 0.f && v < INFINITY; };
    auto nonneg = [](float v) { return v >= 0.f && v < INFINITY; };
    if (!a || !a->image || !a->unary || !a->work || !a->labels ||
        !crf_make_plan(a->H, a->W, a->n_results, a->classes, q) || a->iters < 0 || a->iters > 64 ||
        !pos(a->sxy_b) || !pos(a->srgb) || !pos(a->sxy_g) || !(a->sxy_g <= SD_CRF_MAX_SXY_G) ||
        !nonneg(a->w_g) || !nonneg(a->w_b) ||
        (((uintptr_t)a->image | (uintptr_t)a->unary | (uintptr_t)a->work | (uintptr_t)a->labels |
          (uintptr_t)a->q) & 15)) {
        sd_set_error("sd_dense_crf: invalid argument (1 <= H, W <= 4096, H W <= 2^20, 1 <= n_results "
                     "<= 8, 2 <= classes[r] <= 64, 0 <= iters <= 64, sxy_b, srgb > 0, 0 < sxy_g <= 0.7, "
                     "w_g, w_b >= 0 and finite, 16-B aligned image / unary / work / labels / q)");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    char *wk = (char *)a->work;
    crf_k p;
    float *feat = (float *)(wk + q.o_feat);
    p.feat = feat;
    p.unary = a->unary;
    p.nb = (float *)(wk + q.o_nb);
    p.ng = (float *)(wk + q.o_ng);
    p.H = a->H; p.W = a->W; p.N = (int)q.N; p.Npad = (int)q.Npad; p.R = a->n_results;
    p.CT = q.CT; p.ntiles = q.CTp / 16; p.ldm = q.CTp + 1;
    for (int r = 0; r < SD_CRF_MAX_RESULTS; ++r) {
        p.cls[r] = r < a->n_results ? a->classes[r] : 0;
        p.off[r] = r < a->n_results ? q.off[r] : 0;
    }
    const double log2e = 1.4426950408889634;
    p.ea = (float)(log2e * 0.5 / ((double)a->sxy_b * a->sxy_b));
    p.ec = (float)(log2e * 0.5 / ((double)a->srgb * a->srgb));
    const double cut = CRF_TRUNC * (double)a->sxy_b;
    p.cut2 = cut * cut < (double)CRF_MAX_CUT2 ? (float)(cut * cut) : CRF_MAX_CUT2;
    p.rc = (int)ceil(sqrt((double)p.cut2));
    p.ga = (float)(0.5 / ((double)a->sxy_g * a->sxy_g));
    p.rg = (int)ceil(CRF_TRUNC * (double)a->sxy_g);
    if (p.rg > CRF_MAX_RG) p.rg = CRF_MAX_RG;
    p.w_g = a->w_g; p.w_b = a->w_b;

    float *qf[2] = {(float *)(wk + q.o_qf), (float *)(wk + q.o_qf + q.qf_bytes)};
    _Float16 *nq[2] = {(_Float16 *)(wk + q.o_nq), (_Float16 *)(wk + q.o_nq + q.nq_bytes)};
    const unsigned tiles = (unsigned)(q.Npad / CRF_TILE);
    const int lds = CRF_TILE * p.ldm * (int)sizeof(float);
    const int iters = a->iters;
    // padded keys and columns of n^b Q: zero (a padded key has weight 0, and 0 x 0 = 0)
    if (iters > 0 && hipMemsetAsync(nq[0], 0, (size_t)(2 * q.nq_bytes), s) != hipSuccess) {
        sd_set_error("sd_dense_crf: memset failed");
        return -2;
    }
    sd_lds_attr((const void *)k_crf_init, lds);
    sd_lds_attr((const void *)k_crf_sweep<false>, lds);
    hipLaunchKernelGGL(k_crf_prep, dim3((unsigned)((q.Npad + 255) / 256)), dim3(256), 0, s, a->image, p, feat);
    const crf_out none = {nullptr, nullptr, nullptr, nullptr};
    if (iters > 0)
        hipLaunchKernelGGL(k_crf_sweep<true>, dim3(tiles), dim3(256), 0, s, p, (const _Float16 *)nullptr,
                           (const float *)nullptr, none);
    {
        crf_out o = {nullptr, nullptr, nullptr, nullptr};
        if (iters > 0) { o.nq = nq[0]; o.qf = qf[0]; }
        else { o.labels = a->labels; o.q = a->q; }
        hipLaunchKernelGGL(k_crf_init, dim3(tiles), dim3(256), lds, s, p, o, iters > 0 ? 1 : 0);
    }
    for (int t = 0; t < iters; ++t) {
        const int in = t & 1, out = in ^ 1;
        crf_out o = {nullptr, nullptr, nullptr, nullptr};
        if (t + 1 < iters) { o.nq = nq[out]; o.qf = qf[out]; }
        else { o.labels = a->labels; o.q = a->q; }
        hipLaunchKernelGGL(k_crf_sweep<false>, dim3(tiles), dim3(256), lds, s, p, (const _Float16 *)nq[in],
                           (const float *)qf[in], o);
    }
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_dense_crf: launch failed");
        return -2;
    }
    return 0;
}
