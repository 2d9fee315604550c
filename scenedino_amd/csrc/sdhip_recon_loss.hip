// sdhip_recon_loss.hip -- the first training stage's ReconstructionLoss on gfx950 (CDNA4):
// photometric L1 + SSIM (minimum over the rendered views, masked by the invalid policy), cosine
// DINO reconstruction and the two edge-aware smoothness regularisers, forward and backward
// (scenedino/losses/reconstruction_loss.py:175-356 with training/loss/scenedino.yaml;
// scenedino_amd/losses/reconstruction_loss.py holds the same arithmetic in torch ops).
//
// Forward, two launches.  k_rl_fwd's workgroups (256 threads) take one of three roles by index:
//   patch  one workgroup per patch (h, w <= 16: thread = pixel).  rgb_gt and one view of rgb at
//          a time sit in LDS as zero-bordered channel planes; per view the 3 x 3 Gaussian
//          statistics give clamp(1 - n / d, 0, 1) / 2 per channel, mixed 0.85 / 0.15 with L1;
//          minimum over views (ties kept as a bit mask, as amin's backward shares them), the
//          invalid policy over K x nv, the patch sum; then u = (1 / clamp(depth)) / patch mean
//          and sum |du| exp(-|d rgb_gt|) to the right and down neighbours.
//   dino   one workgroup per (patch, 64 channels): lane = (column, 4 channels), a wave walks
//          the rows with the current and next row in registers (each element is read once, 16
//          bytes per lane for f32); the right neighbour comes from lane + 4.
//          sum_c |d dino| exp(-25 |d rgb_gt|).
//   rows   one wave per row of the downsampled features: 1 - cos(T (pred + artifacts), T gt)
//          with torch's eps (1e-8 on each norm).
// Every workgroup writes one partial (rows: one per row) into work; k_rl_final (one workgroup)
// adds them in index order, skips and counts NaN rows as nanmean does, and writes the four
// terms and rec_loss.  No atomics: a repeated launch gives the same bits.
//
// Backward, one launch (k_rl_bwd, the same three roles), scaled by the upstream gradient read
// from device memory:
//   patch  per view, each pixel that selected the view (and is valid, and whose 1 - n / d lies
//          inside the clamp) writes dS/d mu_x, dS/d E[x^2], dS/d E[xy] times its upstream weight
//          into LDS coefficient planes; d rgb at a pixel gathers them over its 3 x 3
//          neighbourhood (the window is symmetric) and adds the L1 sign.  The depth gradient
//          carries the patch-mean normalisation: (g_j - sum_k g_k u_k / N) / mean.
//   dino   sign(d) times the edge weights the forward saved, one walk with three rows in flight.
//   rows   d (1 - cos) / d pred, zero weight on the rows nanmean skipped.
#include "sdhip_common.h"

#include <math.h>
#include <stdio.h>

extern "C" void sd_set_error(const char *msg);

#define RL_T 256
#define RL_ROWS 18              // 16 + the zero border
#define RL_STRIDE_MAX 48        // plane row stride = w + 32: the two (w = 16) or four (w = 8)
                                // rows a 32-lane group touches land on disjoint banks
#define RL_PLANE (RL_ROWS * RL_STRIDE_MAX)
#define RL_C1 0.0001f           // 0.01^2
#define RL_C2 0.0009f           // 0.03^2
#define RL_G0 0.0947f           // corner, edge, centre of the 3 x 3 Gaussian window
#define RL_G1 0.1183f
#define RL_G2 0.1478f
#define RL_COS_EPS 1e-8f

typedef __attribute__((ext_vector_type(4))) __bf16 rl_h4;

// fixed-order block sum (every thread calls it; red holds RL_T floats)
__device__ __forceinline__ float rl_block_sum(float v, float *red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = RL_T / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ float rl_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// 3 x 3 Gaussian of a zero-bordered plane at interior offset o (row stride S)
__device__ __forceinline__ float rl_gauss(const float *p, int o, int S) {
    const float c = (p[o - S - 1] + p[o - S + 1]) + (p[o + S - 1] + p[o + S + 1]);
    const float e = (p[o - S] + p[o - 1]) + (p[o + 1] + p[o + S]);
    return (RL_G0 * c + RL_G1 * e) + RL_G2 * p[o];
}
// the same of the product of two planes
__device__ __forceinline__ float rl_gauss2(const float *p, const float *q, int o, int S) {
    const float c = (p[o - S - 1] * q[o - S - 1] + p[o - S + 1] * q[o - S + 1]) +
                    (p[o + S - 1] * q[o + S - 1] + p[o + S + 1] * q[o + S + 1]);
    const float e = (p[o - S] * q[o - S] + p[o - 1] * q[o - 1]) +
                    (p[o + 1] * q[o + 1] + p[o + S] * q[o + S]);
    return (RL_G0 * c + RL_G1 * e) + RL_G2 * (p[o] * q[o]);
}

__device__ __forceinline__ float rl_absdiff3(const float *gt, int o0, int o1) {
    return ((fabsf(gt[o0] - gt[o1]) + fabsf(gt[RL_PLANE + o0] - gt[RL_PLANE + o1])) +
            fabsf(gt[2 * RL_PLANE + o0] - gt[2 * RL_PLANE + o1])) / 3.f;
}

__device__ __forceinline__ float rl_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

__device__ __forceinline__ f32x4 rl_load4(const float *p) { return *(const f32x4 *)p; }
__device__ __forceinline__ f32x4 rl_load4(const __bf16 *p) {
    const rl_h4 v = *(const rl_h4 *)p;
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
__device__ __forceinline__ void rl_store4(float *p, f32x4 v) { *(f32x4 *)p = v; }
__device__ __forceinline__ void rl_store4(__bf16 *p, f32x4 v) {
    *(rl_h4 *)p = rl_h4{(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
}
__device__ __forceinline__ float rl_abs4(f32x4 a, f32x4 b) {
    return (fabsf(a[0] - b[0]) + fabsf(a[1] - b[1])) + (fabsf(a[2] - b[2]) + fabsf(a[3] - b[3]));
}

// work layout (floats): [photometric (P) | depth (P) | dino (P * C / 64) | rows (R)]
__host__ __device__ inline int64_t rl_off_depth(const sd_recon_loss_args &a) { return a.P; }
__host__ __device__ inline int64_t rl_off_dino(const sd_recon_loss_args &a) { return 2 * a.P; }
__host__ __device__ inline int64_t rl_off_rows(const sd_recon_loss_args &a) {
    return 2 * a.P + (a.dino ? a.P * (a.C / 64) : 0);
}

// SSIM statistics of one pixel and channel: x plane xs, gt plane gy at offset o
struct RlStat {
    float mux, muy, A1, A2, B1, B2;
};
__device__ __forceinline__ RlStat rl_stat(const float *xs, const float *gy, int o, int S,
                                          float muy, float syy) {
    RlStat r;
    r.mux = rl_gauss(xs, o, S);
    r.muy = muy;
    const float sxx = rl_gauss2(xs, xs, o, S), sxy = rl_gauss2(xs, gy, o, S);
    const float mxx = r.mux * r.mux, myy = muy * muy, mxy = r.mux * muy;
    r.A1 = 2.f * mxy + RL_C1;
    r.A2 = 2.f * (sxy - mxy) + RL_C2;
    r.B1 = (mxx + myy) + RL_C1;
    r.B2 = ((sxx - mxx) + (syy - myy)) + RL_C2;
    return r;
}

// ------------------------------------------------------------------------ forward roles
__device__ void rl_patch_fwd(const sd_recon_loss_args &a, const int p, float *sm) {
    const int tid = threadIdx.x, h = a.h, w = a.w, nv = a.nv, S = w + 32, npx = h * w;
    float *gt = sm, *xs = sm + 3 * RL_PLANE, *dp = sm + 6 * RL_PLANE, *red = sm + 7 * RL_PLANE;
    for (int i = tid; i < 7 * RL_PLANE; i += RL_T) sm[i] = 0.f;
    __syncthreads();
    const bool on = tid < npx;
    const int y = on ? tid / w : 0, x = on ? tid - y * w : 0;
    const int o = (y + 1) * S + (x + 1);
    const int64_t pix = (int64_t)p * npx + (on ? tid : 0);
    float di = 0.f;
    if (on) {
#pragma unroll
        for (int c = 0; c < 3; ++c) gt[c * RL_PLANE + o] = a.rgb_gt[pix * 3 + c];
        if (a.depth) di = 1.f / fminf(fmaxf(a.depth[pix], 1e-3f), 80.f);
    }
    __syncthreads();
    float muy[3], syy[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        muy[c] = rl_gauss(gt + c * RL_PLANE, o, S);
        syy[c] = rl_gauss2(gt + c * RL_PLANE, gt + c * RL_PLANE, o, S);
    }

    // invalid policy over K x nv (weight_guided: every view's weighted sum over 0.9; strict:
    // every view has an invalid sample)
    bool invalid = false;
    if (on && a.policy != SD_RL_POLICY_NONE) {
        const float *iv = a.invalid + pix * a.K * nv, *wt = a.weights + pix * a.K;
        float s[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) s[v] = 0.f;
        for (int k = 0; k < a.K; ++k) {
            const float wk = a.policy == SD_RL_POLICY_WEIGHT ? wt[k] : 0.f;
#pragma unroll
            for (int v = 0; v < 8; ++v)
                if (v < nv) {
                    const float q = iv[k * nv + v];
                    if (a.policy == SD_RL_POLICY_WEIGHT) s[v] += q * wk;
                    else if (q > 0.5f) s[v] = 1.f;
                }
        }
        invalid = true;
#pragma unroll
        for (int v = 0; v < 8; ++v)
            if (v < nv) invalid = invalid && (s[v] > (a.policy == SD_RL_POLICY_WEIGHT ? 0.9f : 0.5f));
    }

    float best = INFINITY;
    uint32_t mask = 0;
    for (int v = 0; v < nv; ++v) {
        __syncthreads();
        float xv[3] = {0.f, 0.f, 0.f};
        if (on) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                xv[c] = a.rgb[(pix * nv + v) * 3 + c];
                xs[c * RL_PLANE + o] = xv[c];
            }
        }
        __syncthreads();
        if (on) {
            float ss = 0.f, l1 = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const RlStat st = rl_stat(xs + c * RL_PLANE, gt + c * RL_PLANE, o, S, muy[c], syy[c]);
                const float t = 1.f - (st.A1 * st.A2) / (st.B1 * st.B2);
                ss += fminf(fmaxf(t, 0.f), 1.f) / 2.f;
                l1 += fabsf(xv[c] - gt[c * RL_PLANE + o]);
            }
            const float err = 0.85f * (ss / 3.f) + 0.15f * (l1 / 3.f);
            if (err < best) {
                best = err;
                mask = 1u << v;
            } else if (err == best) {
                mask |= 1u << v;
            }
        }
    }
    if (on && a.sel) a.sel[pix] = (int32_t)(mask | (invalid ? 0u : 256u));
    const float sp = rl_block_sum(on && !invalid ? best : 0.f, red);
    if (tid == 0) a.work[p] = sp;

    // edge weights of rgb_gt: temperature 1 for the depth term, 25 saved for the DINO term
    float ex1 = 0.f, ey1 = 0.f;
    if (on) {
        float ex25 = 0.f, ey25 = 0.f;
        if (x < w - 1) {
            const float d = rl_absdiff3(gt, o, o + 1);
            ex1 = expf(-d);
            ex25 = expf(-25.f * d);
        }
        if (y < h - 1) {
            const float d = rl_absdiff3(gt, o, o + S);
            ey1 = expf(-d);
            ey25 = expf(-25.f * d);
        }
        if (a.edge) {
            a.edge[pix * 2] = ex25;
            a.edge[pix * 2 + 1] = ey25;
        }
    }
    if (a.depth) {
        const float m = rl_block_sum(di, red) / (float)npx;
        const float u = di / m;
        if (on) dp[o] = u;
        __syncthreads();
        float t = 0.f;
        if (on) {
            if (x < w - 1) t += fabsf(u - dp[o + 1]) * ex1;
            if (y < h - 1) t += fabsf(u - dp[o + S]) * ey1;
        }
        const float sd = rl_block_sum(t, red);
        if (tid == 0) {
            a.work[rl_off_depth(a) + p] = sd;
            if (a.dmean) a.dmean[p] = m;
        }
    }
}

template <typename TD>
__device__ void rl_dino_fwd(const sd_recon_loss_args &a, const int p, const int chunk, float *sm) {
    const int tid = threadIdx.x, h = a.h, w = a.w, npx = h * w, C = a.C;
    float *ew = sm, *red = sm + 2 * RL_T;
    if (tid < npx) {
        const int y = tid / w, x = tid - y * w;
        const float *g = a.rgb_gt + ((int64_t)p * npx + tid) * 3;
        float ex = 0.f, ey = 0.f;
        if (x < w - 1)
            ex = expf(-25.f * (((fabsf(g[0] - g[3]) + fabsf(g[1] - g[4])) + fabsf(g[2] - g[5])) / 3.f));
        if (y < h - 1) {
            const float *d = g + 3 * w;
            ey = expf(-25.f * (((fabsf(g[0] - d[0]) + fabsf(g[1] - d[1])) + fabsf(g[2] - d[2])) / 3.f));
        }
        ew[2 * tid] = ex;
        ew[2 * tid + 1] = ey;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63, x = lane >> 2, q = lane & 3;
    const bool act = x < w;
    const TD *base = (const TD *)a.dino + (int64_t)p * npx * C + chunk * 64 + wave * 16 + q * 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 cur = act ? rl_load4(base + (int64_t)x * C) : zero;
    float acc = 0.f;
    for (int y = 0; y < h; ++y) {
        const f32x4 nxt = (act && y + 1 < h) ? rl_load4(base + (int64_t)((y + 1) * w + x) * C) : zero;
        f32x4 rt;
#pragma unroll
        for (int j = 0; j < 4; ++j) rt[j] = __shfl_down(cur[j], 4);
        if (act) {
            if (x < w - 1) acc += rl_abs4(cur, rt) * ew[2 * (y * w + x)];
            if (y < h - 1) acc += rl_abs4(cur, nxt) * ew[2 * (y * w + x) + 1];
        }
        cur = nxt;
    }
    const float s = rl_block_sum(acc, red);
    if (tid == 0) a.work[rl_off_dino(a) + (int64_t)p * (C / 64) + chunk] = s;
}

// one row's operands in registers: Cd <= 768 -> at most 3 float4 per lane
struct RlRow {
    f32x4 av[3], bv[3];
    float dot, na, nb;
};
__device__ __forceinline__ RlRow rl_row_load(const sd_recon_loss_args &a, int64_t row, int lane) {
    RlRow r;
    const int n4 = a.Cd / 4;
    const float T = a.temperature;
    float dot = 0.f, na2 = 0.f, nb2 = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = lane + 64 * i;
        r.av[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        r.bv[i] = r.av[i];
        if (j < n4) {
            f32x4 pv = rl_load4(a.dino_down + row * a.Cd + 4 * j);
            if (a.dino_artifacts) pv = pv + rl_load4(a.dino_artifacts + row * a.Cd + 4 * j);
            r.av[i] = pv * T;
            r.bv[i] = rl_load4(a.dino_gt + row * a.Cd + 4 * j) * T;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dot += r.av[i][e] * r.bv[i][e];
                na2 += r.av[i][e] * r.av[i][e];
                nb2 += r.bv[i][e] * r.bv[i][e];
            }
        }
    }
    r.dot = rl_wave_sum(dot);
    r.na = sqrtf(rl_wave_sum(na2));
    r.nb = sqrtf(rl_wave_sum(nb2));
    return r;
}

__device__ void rl_rows_fwd(const sd_recon_loss_args &a, const int blk) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blk * 4 + wave;
    if (row >= a.R) return;
    const RlRow r = rl_row_load(a, row, lane);
    const float cs = r.dot / (fmaxf(r.na, RL_COS_EPS) * fmaxf(r.nb, RL_COS_EPS));
    if (lane == 0) a.work[rl_off_rows(a) + row] = 1.f - cs;
}

__global__ void __launch_bounds__(RL_T) k_rl_fwd(const sd_recon_loss_args a, const int nb_dino) {
    __shared__ float sm[7 * RL_PLANE + RL_T];
    const int b = blockIdx.x, P = (int)a.P;
    if (b < P) {
        rl_patch_fwd(a, b, sm);
    } else if (b < P + nb_dino) {
        const int nch = a.C / 64, i = b - P;
        if (a.dino_dtype == SD_BF16) rl_dino_fwd<__bf16>(a, i / nch, i % nch, sm);
        else rl_dino_fwd<float>(a, i / nch, i % nch, sm);
    } else {
        rl_rows_fwd(a, b - P - nb_dino);
    }
}

// strided partial sums, then the fixed-order block sum
__device__ float rl_sum_range(const float *v, int64_t n, float *red) {
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += RL_T) s += v[i];
    return rl_block_sum(s, red);
}

__global__ void __launch_bounds__(RL_T) k_rl_final(const sd_recon_loss_args a) {
    __shared__ float red[RL_T];
    const float npix = (float)a.P * (float)(a.h * a.w);
    const float s_rgb = rl_sum_range(a.work, a.P, red);
    const float s_dep = a.depth ? rl_sum_range(a.work + rl_off_depth(a), a.P, red) : 0.f;
    const float s_din = a.dino ? rl_sum_range(a.work + rl_off_dino(a), a.P * (a.C / 64), red) : 0.f;
    float s_row = 0.f, n_row = 0.f;
    if (a.dino_down) {
        const float *v = a.work + rl_off_rows(a);
        float s = 0.f, c = 0.f;
        for (int64_t i = threadIdx.x; i < a.R; i += RL_T) {
            const float l = v[i];
            if (l == l) {  // nanmean: NaN rows are neither summed nor counted
                s += l;
                c += 1.f;
            }
        }
        s_row = rl_block_sum(s, red);
        n_row = rl_block_sum(c, red);
    }
    if (threadIdx.x) return;
    const float t_rgb = s_rgb / npix;
    const float t_cos = a.dino_down ? s_row / n_row : 0.f;
    const float t_dep = a.depth ? s_dep / npix : 0.f;
    const float t_din = a.dino ? (s_din / (float)a.C) / npix : 0.f;
    float rec = t_rgb * a.lambda_coarse;
    if (a.dino_down) rec += (t_cos * a.lambda_coarse) * a.lambda_dino;
    if (t_dep != 0.f) rec += t_dep * a.lambda_depth;
    if (t_din != 0.f) rec += t_din * a.lambda_dsmooth;
    a.terms[0] = t_rgb;
    a.terms[1] = t_cos;
    a.terms[2] = t_dep;
    a.terms[3] = t_din;
    a.rec[0] = rec;
    if (a.count) a.count[0] = n_row;
}

// ------------------------------------------------------------------------ backward roles
__device__ void rl_patch_bwd(const sd_recon_loss_args &a, const int p, float *sm) {
    const int tid = threadIdx.x, h = a.h, w = a.w, nv = a.nv, S = w + 32, npx = h * w;
    float *gt = sm, *xs = sm + 3 * RL_PLANE, *co = sm + 6 * RL_PLANE, *dp = sm + 15 * RL_PLANE,
          *red = sm + 16 * RL_PLANE;
    for (int i = tid; i < 16 * RL_PLANE; i += RL_T) sm[i] = 0.f;
    __syncthreads();
    const bool on = tid < npx;
    const int y = on ? tid / w : 0, x = on ? tid - y * w : 0;
    const int o = (y + 1) * S + (x + 1);
    const int64_t pix = (int64_t)p * npx + (on ? tid : 0);
    const float g = a.g_rec[0];
    const float npix = (float)a.P * (float)npx;
    if (on) {
#pragma unroll
        for (int c = 0; c < 3; ++c) gt[c * RL_PLANE + o] = a.rgb_gt[pix * 3 + c];
    }
    __syncthreads();

    if (a.d_rgb) {
        float muy[3], syy[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            muy[c] = rl_gauss(gt + c * RL_PLANE, o, S);
            syy[c] = rl_gauss2(gt + c * RL_PLANE, gt + c * RL_PLANE, o, S);
        }
        const uint32_t sel = on ? (uint32_t)a.sel[pix] : 0u;
        const uint32_t mask = sel & 255u;
        // upstream weight of this pixel's selected views: valid, shared among amin's ties
        const float wq = (on && (sel & 256u) && mask)
                             ? ((g * a.lambda_coarse) / npix) / (float)__popc(mask) : 0.f;
        for (int v = 0; v < nv; ++v) {
            __syncthreads();
            float xv[3] = {0.f, 0.f, 0.f};
            if (on) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    xv[c] = a.rgb[(pix * nv + v) * 3 + c];
                    xs[c * RL_PLANE + o] = xv[c];
                }
            }
            __syncthreads();
            const float wv = ((mask >> v) & 1u) ? wq : 0.f;
            float gl[3] = {0.f, 0.f, 0.f};
            if (on) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float ca = 0.f, cb = 0.f, cc = 0.f;
                    if (wv != 0.f) {
                        const RlStat st =
                            rl_stat(xs + c * RL_PLANE, gt + c * RL_PLANE, o, S, muy[c], syy[c]);
                        const float D = st.B1 * st.B2, Sv = (st.A1 * st.A2) / D, t = 1.f - Sv;
                        if (t >= 0.f && t <= 1.f) {
                            const float up = (wv * (0.85f / 3.f)) * -0.5f;
                            ca = up * ((2.f * st.muy * (st.A2 - st.A1)) / D -
                                       Sv * (2.f * st.mux) * (1.f / st.B1 - 1.f / st.B2));
                            cb = up * (-Sv / st.B2);
                            cc = up * ((2.f * st.A1) / D);
                        }
                        gl[c] = (wv * (0.15f / 3.f)) * rl_sign(xv[c] - gt[c * RL_PLANE + o]);
                    }
                    co[(3 * c) * RL_PLANE + o] = ca;
                    co[(3 * c + 1) * RL_PLANE + o] = cb;
                    co[(3 * c + 2) * RL_PLANE + o] = cc;
                }
            }
            __syncthreads();
            if (on) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float ga = rl_gauss(co + (3 * c) * RL_PLANE, o, S);
                    const float gb = rl_gauss(co + (3 * c + 1) * RL_PLANE, o, S);
                    const float gc = rl_gauss(co + (3 * c + 2) * RL_PLANE, o, S);
                    a.d_rgb[(pix * nv + v) * 3 + c] =
                        ((ga + (2.f * xv[c]) * gb) + gt[c * RL_PLANE + o] * gc) + gl[c];
                }
            }
        }
    }

    if (a.d_depth) {
        float di = 0.f;
        bool inr = false;
        if (on) {
            const float d = a.depth[pix];
            inr = d >= 1e-3f && d <= 80.f;
            di = 1.f / fminf(fmaxf(d, 1e-3f), 80.f);
        }
        const float m = a.dmean[p];
        const float u = di / m;
        __syncthreads();
        if (on) dp[o] = u;
        __syncthreads();
        float gj = 0.f;
        if (on) {
            if (x < w - 1) gj += rl_sign(u - dp[o + 1]) * expf(-rl_absdiff3(gt, o, o + 1));
            if (x > 0) gj -= rl_sign(dp[o - 1] - u) * expf(-rl_absdiff3(gt, o - 1, o));
            if (y < h - 1) gj += rl_sign(u - dp[o + S]) * expf(-rl_absdiff3(gt, o, o + S));
            if (y > 0) gj -= rl_sign(dp[o - S] - u) * expf(-rl_absdiff3(gt, o - S, o));
        }
        const float gu = rl_block_sum(on ? gj * u : 0.f, red);
        if (on) {
            const float sc = (g * a.lambda_depth) / npix;
            const float ddi = ((gj - gu / (float)npx) / m) * sc;
            a.d_depth[pix] = inr ? -(di * di) * ddi : 0.f;
        }
    }
}

template <typename TD>
__device__ void rl_dino_bwd(const sd_recon_loss_args &a, const int p, const int chunk) {
    const int tid = threadIdx.x, h = a.h, w = a.w, npx = h * w, C = a.C;
    const int wave = tid >> 6, lane = tid & 63, x = lane >> 2, q = lane & 3;
    const bool act = x < w;
    const int64_t off = (int64_t)p * npx * C + chunk * 64 + wave * 16 + q * 4;
    const TD *base = (const TD *)a.dino + off;
    TD *out = (TD *)a.d_dino + off;
    const float *ew = a.edge + (int64_t)p * npx * 2;
    const float sc = ((a.g_rec[0] * a.lambda_dsmooth) / (float)C) / ((float)a.P * (float)npx);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 prv = zero, cur = act ? rl_load4(base + (int64_t)x * C) : zero;
    for (int y = 0; y < h; ++y) {
        const f32x4 nxt = (act && y + 1 < h) ? rl_load4(base + (int64_t)((y + 1) * w + x) * C) : zero;
        f32x4 rt, lt;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            rt[j] = __shfl_down(cur[j], 4);
            lt[j] = __shfl_up(cur[j], 4);
        }
        if (act) {
            const int i = y * w + x;
            const float er = x < w - 1 ? ew[2 * i] : 0.f, el = x > 0 ? ew[2 * (i - 1)] : 0.f;
            const float ed = y < h - 1 ? ew[2 * i + 1] : 0.f, eu = y > 0 ? ew[2 * (i - w) + 1] : 0.f;
            f32x4 gv;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float t = 0.f;
                if (x < w - 1) t += rl_sign(cur[j] - rt[j]) * er;
                if (x > 0) t -= rl_sign(lt[j] - cur[j]) * el;
                if (y < h - 1) t += rl_sign(cur[j] - nxt[j]) * ed;
                if (y > 0) t -= rl_sign(prv[j] - cur[j]) * eu;
                gv[j] = t * sc;
            }
            rl_store4(out + (int64_t)i * C, gv);
        }
        prv = cur;
        cur = nxt;
    }
}

__device__ void rl_rows_bwd(const sd_recon_loss_args &a, const int blk) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blk * 4 + wave;
    if (row >= a.R) return;
    const RlRow r = rl_row_load(a, row, lane);
    const float nae = fmaxf(r.na, RL_COS_EPS), nbe = fmaxf(r.nb, RL_COS_EPS);
    const float cs = r.dot / (nae * nbe), loss = 1.f - cs;
    // d loss / d pred = -T d cos / d a;  rows nanmean skipped carry no weight
    const float up = loss == loss ? ((a.g_rec[0] * a.lambda_coarse) * a.lambda_dino) / a.count[0] : 0.f;
    const float kb = 1.f / (nae * nbe);
    const float ka = r.na > RL_COS_EPS ? cs / (r.na * r.na) : 0.f;
    const float s = -(up * a.temperature);
    const int n4 = a.Cd / 4;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = lane + 64 * i;
        if (j < n4) rl_store4(a.d_down + row * a.Cd + 4 * j, (r.bv[i] * kb - r.av[i] * ka) * s);
    }
}

__global__ void __launch_bounds__(RL_T) k_rl_bwd(const sd_recon_loss_args a, const int nb_patch,
                                                  const int nb_dino) {
    __shared__ float sm[16 * RL_PLANE + RL_T];
    const int b = blockIdx.x;
    if (b < nb_patch) {
        rl_patch_bwd(a, b, sm);
    } else if (b < nb_patch + nb_dino) {
        const int nch = a.C / 64, i = b - nb_patch;
        if (a.dino_dtype == SD_BF16) rl_dino_bwd<__bf16>(a, i / nch, i % nch);
        else rl_dino_bwd<float>(a, i / nch, i % nch);
    } else {
        rl_rows_bwd(a, b - nb_patch - nb_dino);
    }
}

// ------------------------------------------------------------------------ C ABI
static bool rl_aligned(const void *p) { return ((uintptr_t)p & 15) == 0; }

static const char *rl_validate(const sd_recon_loss_args *a, bool bwd) {
    if (!a) return "null args";
    if (!a->rgb || !a->rgb_gt || !a->work) return "rgb, rgb_gt and work are required";
    if (a->P < 1 || a->P > 0x3fffff) return "1 <= P < 2^22";
    if (a->h < 2 || a->h > 16 || a->w < 2 || a->w > 16) return "2 <= h, w <= 16";
    if (a->nv < 1 || a->nv > 8) return "1 <= nv <= 8";
    if (a->policy != SD_RL_POLICY_WEIGHT && a->policy != SD_RL_POLICY_STRICT &&
        a->policy != SD_RL_POLICY_NONE)
        return "policy is weight_guided, strict or none";
    if (a->policy != SD_RL_POLICY_NONE && (!a->invalid || a->K < 1)) return "the policy needs invalid (K >= 1)";
    if (a->policy == SD_RL_POLICY_WEIGHT && !a->weights) return "weight_guided needs weights";
    if (a->dino && (a->C < 64 || a->C > 768 || a->C % 64)) return "C % 64 == 0, 64 <= C <= 768";
    if (a->dino && a->dino_dtype != SD_F32 && a->dino_dtype != SD_BF16) return "dino is f32 or bf16";
    if (a->dino_down) {
        if (!a->dino_gt) return "dino_down needs dino_gt";
        if (a->Cd < 64 || a->Cd > 768 || a->Cd % 64) return "Cd % 64 == 0, 64 <= Cd <= 768";
        if (a->R < 1 || a->R > 0x3fffffff) return "1 <= R < 2^30";
    }
    if (!rl_aligned(a->rgb) || !rl_aligned(a->rgb_gt) || !rl_aligned(a->invalid) ||
        !rl_aligned(a->weights) || !rl_aligned(a->depth) || !rl_aligned(a->dino) ||
        !rl_aligned(a->dino_down) || !rl_aligned(a->dino_gt) || !rl_aligned(a->dino_artifacts) ||
        !rl_aligned(a->work) || !rl_aligned(a->rec) || !rl_aligned(a->terms) || !rl_aligned(a->sel) ||
        !rl_aligned(a->edge) || !rl_aligned(a->dmean) || !rl_aligned(a->count) ||
        !rl_aligned(a->g_rec) || !rl_aligned(a->d_rgb) || !rl_aligned(a->d_depth) ||
        !rl_aligned(a->d_dino) || !rl_aligned(a->d_down))
        return "pointers are 16-byte aligned";
    if (!bwd) {
        if (!a->rec || !a->terms) return "rec and terms are required";
    } else {
        if (!a->g_rec) return "g_rec is required";
        if (a->d_rgb && !a->sel) return "d_rgb needs the forward's sel";
        if (a->d_depth && (!a->depth || !a->dmean)) return "d_depth needs depth and the forward's dmean";
        if (a->d_dino && (!a->dino || !a->edge)) return "d_dino needs dino and the forward's edge";
        if (a->d_down && (!a->dino_down || !a->count)) return "d_down needs dino_down and the forward's count";
    }
    return nullptr;
}

static int rl_fail(const char *fn, const char *why) {
    static thread_local char buf[256];
    snprintf(buf, sizeof buf, "%s: invalid argument (%s)", fn, why);
    sd_set_error(buf);
    return -1;
}

extern "C" int64_t sd_recon_loss_work(int64_t P, int32_t C, int64_t R) {
    if (P < 1 || P > 0x3fffff || C < 0 || C > 768 || C % 64 || R < 0 || R > 0x3fffffff) {
        sd_set_error("sd_recon_loss_work: invalid argument (1 <= P < 2^22, C % 64 == 0, C <= 768, "
                     "0 <= R < 2^30)");
        return -1;
    }
    return 2 * P + P * (C / 64) + R;
}

extern "C" int sd_recon_loss_fwd(const sd_recon_loss_args *a, void *stream) {
    if (const char *why = rl_validate(a, false)) return rl_fail("sd_recon_loss_fwd", why);
    const int64_t nb_dino = a->dino ? a->P * (a->C / 64) : 0;
    const int64_t nb_rows = a->dino_down ? (a->R + 3) / 4 : 0;
    const int64_t nb = a->P + nb_dino + nb_rows;
    if (nb > 0x7fffffffLL) return rl_fail("sd_recon_loss_fwd", "too many workgroups");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_rl_fwd, dim3((unsigned)nb), dim3(RL_T), 0, s, *a, (int)nb_dino);
    hipLaunchKernelGGL(k_rl_final, dim3(1), dim3(RL_T), 0, s, *a);
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_recon_loss_fwd: launch failed");
        return -2;
    }
    return 0;
}

extern "C" int sd_recon_loss_bwd(const sd_recon_loss_args *a, void *stream) {
    if (const char *why = rl_validate(a, true)) return rl_fail("sd_recon_loss_bwd", why);
    const int64_t nb_patch = (a->d_rgb || a->d_depth) ? a->P : 0;
    const int64_t nb_dino = a->d_dino ? a->P * (a->C / 64) : 0;
    const int64_t nb_rows = a->d_down ? (a->R + 3) / 4 : 0;
    const int64_t nb = nb_patch + nb_dino + nb_rows;
    if (nb > 0x7fffffffLL) return rl_fail("sd_recon_loss_bwd", "too many workgroups");
    if (nb == 0) return 0;
    hipLaunchKernelGGL(k_rl_bwd, dim3((unsigned)nb), dim3(RL_T), 0, (hipStream_t)stream, *a,
                       (int)nb_patch, (int)nb_dino);
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_recon_loss_bwd: launch failed");
        return -2;
    }
    return 0;
}
