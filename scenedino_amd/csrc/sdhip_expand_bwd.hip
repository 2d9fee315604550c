// sdhip_expand_bwd.hip -- backward of MlpDimReduction.transform_expand on gfx950 (CDNA4).
//
// Forward (dim_reduction.py:22-25; sd_seg_query's dino_full):
//   h = relu(W1 x + b1),  e = W2 h + b2,  n = |e|,  y = e / max(n, 1e-12)
// Backward from dy (P, d_full) f32, nothing saved by the forward:
//   de = (dy - y (y . dy)) / n   for n >= 1e-12,   dy / 1e-12 otherwise (torch's clamp_min)
//   dh = (W2^T de) o [h > 0],    dx = W1^T dh
// and the rows the weight gradients need (h, de, dh, a bf16 copy of x) as bf16: dW2 = de^T h,
// db2 = sum de, dW1 = dh^T x, db1 = sum dh are sd_conv_wgrad calls with taps = 1 on those
// rows (fixed-order partial sums; models/backbones/dino/dim_reduction.py).
//
// Work unit: one wave = 32 rows (lane = row, the column of v_mfma_f32_32x32x16_bf16's B
// operand, as in k_seg_head); weights are the A operands (rows = output features), read from
// plain row-major bf16 matrices (16 KiB .. 192 KiB, L2-resident).  Hidden vectors stay in
// registers: an accumulator tile is converted in place into the next product's B operand,
// which permutes k (register 8 s + j of lane half hh holds row 16 s + 8 (j >> 2) + 4 hh +
// (j & 3) of the tile); the A loads apply the same permutation (two 8-byte reads).
//   layer 1  h (128 x 32)            16 MFMAs
//   pass 1   per 32-column tile of d_full: e tile (8 MFMAs), n^2 += e^2, e.dy += e dy (f32)
//   pass 2   per tile: e again (8), de in f32 -> bf16 rows out, dh += W2^T[:, tile] de (8)
//   mask     dh o [h > 0] -> bf16 rows out;  dx (64 x 32) = W1^T dh, 16 MFMAs, f32 out
// A 32 x d_full f32 tile is never held: e is computed twice instead (d_full / 32 x 8 MFMAs).
// No atomics, no LDS, no cross-wave sum: a repeated launch gives the same bits.
#include "sdhip_common.h"

extern "C" void sd_set_error(const char *msg);

#define XB_DR 64   // reduced DINO dims
#define XB_DL 128  // latent dims
#define XB_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

typedef __attribute__((ext_vector_type(4))) float xb_f4;
typedef __attribute__((ext_vector_type(4))) __bf16 xb_h4;

// A operand, natural k: lane (r, hh) holds W[row][k0 + 8 hh .. + 7]
__device__ __forceinline__ bf16x8 xb_a_nat(const __bf16 *__restrict__ W, int ld, int row, int k0,
                                           int hh) {
    return *(const bf16x8 *)(W + (int64_t)row * ld + k0 + 8 * hh);
}

// A operand, permuted k (the B operand is an accumulator half converted in place): element j
// <- column c0 + 8 (j >> 2) + 4 hh + (j & 3)
__device__ __forceinline__ bf16x8 xb_a_perm(const __bf16 *__restrict__ W, int ld, int row, int c0,
                                            int hh) {
    const __bf16 *p = W + (int64_t)row * ld + c0 + 4 * hh;
    const xb_h4 lo = *(const xb_h4 *)p, hi = *(const xb_h4 *)(p + 8);
    bf16x8 a;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        a[j] = lo[j];
        a[4 + j] = hi[j];
    }
    return a;
}

// accumulator registers 8 s .. 8 s + 7 as a bf16 B operand
__device__ __forceinline__ bf16x8 xb_cvt(const f32x16 &acc, int s) {
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (__bf16)acc[8 * s + j];
    return r;
}

// the same with relu: max with +0 on the 16-bit patterns (k_seg_head's sg_relu_b)
__device__ __forceinline__ bf16x8 xb_relu(const f32x16 &acc, int s) {
    typedef __attribute__((ext_vector_type(8))) short s16x8_t;
    s16x8_t v = __builtin_bit_cast(s16x8_t, xb_cvt(acc, s));
    v = __builtin_elementwise_max(v, (s16x8_t)0);
    return __builtin_bit_cast(bf16x8, v);
}

// vec[32 t + (i & 3) + 8 (i >> 2) + 4 hh], i = 0..15: the rows lane half hh holds of tile t
__device__ __forceinline__ f32x16 xb_rows(const float *__restrict__ vec, int t, int hh) {
    f32x16 r;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const xb_f4 v = *(const xb_f4 *)(vec + 32 * t + 8 * g + 4 * hh);
        r[4 * g] = v[0]; r[4 * g + 1] = v[1]; r[4 * g + 2] = v[2]; r[4 * g + 3] = v[3];
    }
    return r;
}

// a B operand (k-step q of a 128- or d_full-wide row) to bf16 row storage: elements 0..3 at
// column 16 q + 4 hh, 4..7 at 16 q + 8 + 4 hh
__device__ __forceinline__ void xb_store_b(__bf16 *row, int q, int hh, const bf16x8 &v) {
    xb_h4 lo, hi;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        lo[j] = v[j];
        hi[j] = v[4 + j];
    }
    *(xb_h4 *)(row + 16 * q + 4 * hh) = lo;
    *(xb_h4 *)(row + 16 * q + 8 + 4 * hh) = hi;
}

template <bool X16>
__global__ void __launch_bounds__(64) k_expand_bwd(const sd_expand_bwd_args a, const int DF) {
    const int lane = threadIdx.x;
    const int r = lane & 31, hh = lane >> 5;
    const int64_t p = (int64_t)blockIdx.x * 32 + r;
    const bool ok = p < a.P;  // ragged last tile: rows past P compute on zeros, store nothing
    const int T2 = DF / 32;
    const __bf16 *w1 = (const __bf16 *)a.w1, *w2 = (const __bf16 *)a.w2;
    const __bf16 *w1t = (const __bf16 *)a.w1t, *w2t = (const __bf16 *)a.w2t;

    // ---- x as B operands (k-step s: dims 16 s + 8 hh .. + 7), as k_seg_head reads them ----
    bf16x8 xb[XB_DR / 16];
#pragma unroll
    for (int s = 0; s < XB_DR / 16; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) xb[s][j] = (__bf16)0.f;
    if (ok) {
        if (X16) {
            const bf16x8 *src = (const bf16x8 *)a.x + p * (XB_DR / 8);
#pragma unroll
            for (int s = 0; s < XB_DR / 16; ++s) xb[s] = src[2 * s + hh];
        } else {
            const xb_f4 *src = (const xb_f4 *)((const float *)a.x + p * XB_DR);
#pragma unroll
            for (int s = 0; s < XB_DR / 16; ++s) {
                const xb_f4 u = src[4 * s + 2 * hh], v = src[4 * s + 2 * hh + 1];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    xb[s][j] = (__bf16)u[j];
                    xb[s][4 + j] = (__bf16)v[j];
                }
            }
            if (a.xb) {
                bf16x8 *dst = (bf16x8 *)a.xb + p * (XB_DR / 8);
#pragma unroll
                for (int s = 0; s < XB_DR / 16; ++s) dst[2 * s + hh] = xb[s];
            }
        }
    }

    // ---- layer 1: h = relu(W1 x + b1) as B operands hb[k-step 0..7] ----
    bf16x8 hb[XB_DL / 16];
#pragma unroll
    for (int t = 0; t < XB_DL / 32; ++t) {
        f32x16 acc = xb_rows(a.b1, t, hh);
#pragma unroll
        for (int s = 0; s < XB_DR / 16; ++s)
            acc = XB_MFMA(xb_a_nat(w1, XB_DR, 32 * t + r, 16 * s, hh), xb[s], acc);
        hb[2 * t] = xb_relu(acc, 0);
        hb[2 * t + 1] = xb_relu(acc, 1);
    }
    if (a.h && ok) {
        __bf16 *row = (__bf16 *)a.h + p * XB_DL;
#pragma unroll
        for (int q = 0; q < XB_DL / 16; ++q) xb_store_b(row, q, hh, hb[q]);
    }

    // e tile t = W2[32 t .. + 31] h + b2 (rows of lane half hh in accumulator order)
    auto e_tile = [&](int t) {
        f32x16 acc = xb_rows(a.b2, t, hh);
#pragma unroll
        for (int q = 0; q < XB_DL / 16; ++q)
            acc = XB_MFMA(xb_a_perm(w2, XB_DL, 32 * t + r, 16 * q, hh), hb[q], acc);
        return acc;
    };
    // dy[p][32 t + 8 g + 4 hh + e] in the accumulator's register order (4 g + e)
    auto dy_tile = [&](int t) {
        f32x16 d;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            xb_f4 v = {0.f, 0.f, 0.f, 0.f};
            if (ok) v = *(const xb_f4 *)(a.dy + p * DF + 32 * t + 8 * g + 4 * hh);
            d[4 * g] = v[0]; d[4 * g + 1] = v[1]; d[4 * g + 2] = v[2]; d[4 * g + 3] = v[3];
        }
        return d;
    };

    // ---- pass 1: n^2 = |e|^2 and e . dy, f32 ----
    float n2 = 0.f, edy = 0.f;
    for (int t = 0; t < T2; ++t) {
        const f32x16 e = e_tile(t), d = dy_tile(t);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            n2 = fmaf(e[i], e[i], n2);
            edy = fmaf(e[i], d[i], edy);
        }
    }
    n2 += __shfl_xor(n2, 32);
    edy += __shfl_xor(edy, 32);
    // de = (dy - e c) inv:  inv = 1 / n, c = (e . dy) / n^2;  n < 1e-12: the clamp is a
    // constant denominator, de = dy / 1e-12
    const float n = sqrtf(n2);
    float inv = 1e12f, c = 0.f;
    if (n >= 1e-12f) {
        inv = 1.f / n;
        c = (edy * inv) * inv;
    }

    // ---- pass 2: de per tile (bf16 rows out), dh += W2^T[:, tile] de ----
    f32x16 dh[XB_DL / 32];
#pragma unroll
    for (int lt = 0; lt < XB_DL / 32; ++lt)
#pragma unroll
        for (int i = 0; i < 16; ++i) dh[lt][i] = 0.f;
    for (int t = 0; t < T2; ++t) {
        const f32x16 e = e_tile(t), d = dy_tile(t);
        f32x16 de;
#pragma unroll
        for (int i = 0; i < 16; ++i) de[i] = (d[i] - e[i] * c) * inv;
        const bf16x8 deb[2] = {xb_cvt(de, 0), xb_cvt(de, 1)};
        if (a.de && ok) {
            __bf16 *row = (__bf16 *)a.de + p * DF + 32 * t;
            xb_store_b(row, 0, hh, deb[0]);
            xb_store_b(row, 1, hh, deb[1]);
        }
#pragma unroll
        for (int lt = 0; lt < XB_DL / 32; ++lt)
#pragma unroll
            for (int s = 0; s < 2; ++s)
                dh[lt] = XB_MFMA(xb_a_perm(w2t, DF, 32 * lt + r, 32 * t + 16 * s, hh), deb[s], dh[lt]);
    }

    // ---- ReLU mask (register i of tile lt is the row hb[2 lt + (i >> 3)][i & 7] holds) ----
    bf16x8 dhb[XB_DL / 16];
#pragma unroll
    for (int lt = 0; lt < XB_DL / 32; ++lt) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            // h is relu'd: +0 or positive.  The 16-bit patterns are tested on the register
            // words (a per-element bit cast of the bf16 vector compiled to one compare per
            // vector)
            typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
            const uint32_t w = __builtin_bit_cast(u32x4_t, hb[2 * lt + (i >> 3)])[(i & 7) >> 1];
            const uint32_t bits = (i & 1) ? (w >> 16) : (w & 0xffffu);
            if (bits == 0u) dh[lt][i] = 0.f;
        }
        dhb[2 * lt] = xb_cvt(dh[lt], 0);
        dhb[2 * lt + 1] = xb_cvt(dh[lt], 1);
    }
    if (a.dh && ok) {
        __bf16 *row = (__bf16 *)a.dh + p * XB_DL;
#pragma unroll
        for (int q = 0; q < XB_DL / 16; ++q) xb_store_b(row, q, hh, dhb[q]);
    }

    // ---- dx = W1^T dh, f32 ----
#pragma unroll
    for (int t = 0; t < XB_DR / 32; ++t) {
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int q = 0; q < XB_DL / 16; ++q)
            acc = XB_MFMA(xb_a_perm(w1t, XB_DL, 32 * t + r, 16 * q, hh), dhb[q], acc);
        if (ok) {
            float *dst = a.dx + p * XB_DR + 32 * t + 4 * hh;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *(xb_f4 *)(dst + 8 * g) = xb_f4{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        }
    }
}

extern "C" int sd_expand_bwd(const sd_expand_bwd_args *a, const sd_seg_head *h, void *stream) {
    const bool ptrs = a && h && a->x && a->dy && a->w1 && a->w2 && a->w1t && a->w2t && a->b1 &&
                      a->b2 && a->dx;
    if (!ptrs || a->P < 1 || h->d_in != XB_DR || h->d_latent != XB_DL || h->d_full <= 0 ||
        h->d_full % 32 || h->d_full > 4096 || (a->x_dtype != SD_F32 && a->x_dtype != SD_BF16) ||
        (((uintptr_t)a->x | (uintptr_t)a->dy | (uintptr_t)a->w1 | (uintptr_t)a->w2 |
          (uintptr_t)a->w1t | (uintptr_t)a->w2t | (uintptr_t)a->b1 | (uintptr_t)a->b2 |
          (uintptr_t)a->dx | (uintptr_t)a->h | (uintptr_t)a->de | (uintptr_t)a->dh |
          (uintptr_t)a->xb) & 15)) {
        sd_set_error("sd_expand_bwd: invalid argument (P >= 1, d_in 64, d_latent 128, "
                     "d_full % 32 == 0, x f32 or bf16, 16-B aligned non-null operands)");
        return -1;
    }
    const int64_t nblk = (a->P + 31) / 32;
    if (nblk > 0x7fffffffLL) {
        sd_set_error("sd_expand_bwd: too many rows");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    if (a->x_dtype == SD_BF16)
        hipLaunchKernelGGL((k_expand_bwd<true>), dim3((unsigned)nblk), dim3(64), 0, s, *a, h->d_full);
    else
        hipLaunchKernelGGL((k_expand_bwd<false>), dim3((unsigned)nblk), dim3(64), 0, s, *a, h->d_full);
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_expand_bwd: launch failed");
        return -2;
    }
    return 0;
}
