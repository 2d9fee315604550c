// scenedino_amd: backward kernels of the ViT encoder for gfx950 (the training path of
// models/backbones/dino/vit.py, driven by models/backbones/dino/vit_autograd.py).
//
// Linear data gradients reuse the forward GEMM (sd_gemm on transposed weight packs) and
// linear weight / bias gradients reuse sd_conv_wgrad (taps = 1); this unit holds what the
// forward has no counterpart for:
//   * sd_attention_bwd: dQ, dK, dV of the head_dim-64 flash attention, S and P recomputed per
//     tile on v_mfma_f32_32x32x16_bf16;
//   * sd_layernorm_bwd: dx (written or accumulated into the residual-stream gradient), dw, db;
//   * sd_gelu_bwd: the exact-erf GELU derivative on a bf16 gradient.
// No float atomics anywhere: every sum is owned by one workgroup (attention) or goes through
// per-part partial sums added in a fixed order (LayerNorm), so a repeated launch gives the same
// bits.
//
// sd_attention_bwd.  Every workgroup is one wave that owns a 32-row tile, and every matrix
// product is a 32 x 32 x 16 MFMA of two operands that are contiguous along the reduction
// index ("NT" form), read from LDS tiles:
//   A operand: lane (r = lane % 32, h = lane / 32), k-step s reads A[r][16 s + 8 h .. + 7];
//   B operand: the same read of B^T;
//   accumulator register x of lane (r, h) holds C[8 (x / 4) + 4 h + x % 4][r].
// Tiles whose reduction index is the token index are staged transposed (scalar LDS writes;
// V comes from the forward's V^T that way, Q / dO / K from their token-major rows).
//   k_ab_stats (one wave per 32 queries): S^T = K Q^T over all key blocks, online
//     (max, sum) per query in the log2 domain -> lse2 = m + log2 l, and D = sum_e dO O.
//   k_ab_dkv (one wave per 32 keys): for every query tile S^T = K Q^T, dP^T = V dO^T,
//     P^T = exp2(S^T scale log2e - lse2), dS^T = P^T o (dP^T - D); dV += P^T dO,
//     dK += dS^T Q, accumulated in registers over the query tiles.
//   k_ab_dq (one wave per 32 queries): for every key block S = Q K^T, dP = dO V^T, dS;
//     dQ += dS K.
// Keys >= T get P = 0 (the forward's -inf mask), query rows >= T are staged as zeros with
// P forced to 0, and only token rows < T are stored.  Both main loops load the next tile's
// rows into registers before they work on the current one (a kernel trace at 481 tokens x 6
// heads: k_ab_dkv 58 -> 42 us, k_ab_dq 39 -> 34 us; k_ab_stats 12 us).
#include "sdhip_common.h"

extern "C" void sd_set_error(const char *msg);

typedef __attribute__((ext_vector_type(4))) float vb_f4;
typedef __attribute__((ext_vector_type(4))) __bf16 vb_bf4;

#define VB_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)
#define VB_HD 64
#define VB_LQ 72  // bf16 per LDS row of a 32 x 64 tile (144-B rows)
#define VB_LT 40  // bf16 per LDS row of a 64 x 32 / 32 x 32 tile (80-B rows)

__device__ __forceinline__ f32x16 vb_zero16() {
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    return z;
}

// row of accumulator register x for lane half h
__device__ __forceinline__ int vb_row(int x, int h) { return 8 * (x >> 2) + 4 * h + (x & 3); }

// MFMA operand fragment of an LDS tile: row r, reduction columns 16 s + 8 h .. + 7
__device__ __forceinline__ bf16x8 vb_frag(const __bf16 *tile, int ld, int r, int s, int h) {
    return *(const bf16x8 *)(tile + r * ld + 16 * s + 8 * h);
}

// 32 token rows x 64 values from src (row stride ld elements) starting at row0, as four 16-B
// chunks per lane (chunk c = lane + 64 i: row c / 8, columns 8 (c % 8) ..); rows >= limit read
// as zero.  Split into the global loads and the LDS stores so that a loop can issue the next
// tile's loads before it works on the current one.
__device__ __forceinline__ void vb_load(const __bf16 *src, int64_t ld, int row0, int limit,
                                        bf16x8 (&v)[4], int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i, row = c >> 3, col = (c & 7) * 8;
#pragma unroll
        for (int u = 0; u < 8; ++u) v[i][u] = (__bf16)0.f;
        if (row0 + row < limit) v[i] = *(const bf16x8 *)(src + (int64_t)(row0 + row) * ld + col);
    }
}

// rm: row-major tile (VB_LQ), tr (optional): transposed tile [64][VB_LT]
__device__ __forceinline__ void vb_store(const bf16x8 (&v)[4], __bf16 *rm, __bf16 *tr, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i, row = c >> 3, col = (c & 7) * 8;
        *(bf16x8 *)(rm + row * VB_LQ + col) = v[i];
        if (tr) {
#pragma unroll
            for (int u = 0; u < 8; ++u) tr[(col + u) * VB_LT + row] = v[i][u];
        }
    }
}

__device__ __forceinline__ void vb_stage(const __bf16 *src, int64_t ld, int row0, int limit,
                                         __bf16 *rm, __bf16 *tr, int lane) {
    bf16x8 v[4];
    vb_load(src, ld, row0, limit, v, lane);
    vb_store(v, rm, tr, lane);
}

// keys j0 .. j0 + 31 of a head's V^T plane (64, Tp) -> V[j][e] row-major (VB_LQ); chunk
// c = lane + 64 i: head-dim row c / 4, keys j0 + 8 (c % 4) ..
__device__ __forceinline__ void vb_load_vt(const __bf16 *Vh, int Tp, int j0, bf16x8 (&v)[4], int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i, e = c >> 2, jc = (c & 3) * 8;
        v[i] = *(const bf16x8 *)(Vh + (int64_t)e * Tp + j0 + jc);
    }
}

__device__ __forceinline__ void vb_store_vt(const bf16x8 (&v)[4], __bf16 *rm, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i, e = c >> 2, jc = (c & 3) * 8;
#pragma unroll
        for (int u = 0; u < 8; ++u) rm[(jc + u) * VB_LQ + e] = v[i][u];
    }
}

__device__ __forceinline__ void vb_stage_vt(const __bf16 *Vh, int Tp, int j0, __bf16 *rm, int lane) {
    bf16x8 v[4];
    vb_load_vt(Vh, Tp, j0, v, lane);
    vb_store_vt(v, rm, lane);
}

__global__ void __launch_bounds__(64) k_ab_stats(const __bf16 *__restrict__ Q,
                                                 const __bf16 *__restrict__ K,
                                                 const __bf16 *__restrict__ AO,
                                                 const __bf16 *__restrict__ dAO, int T, int Tp,
                                                 int H, float sl2e, float *__restrict__ lse,
                                                 float *__restrict__ dsum) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int bh = blockIdx.y, b = bh / H, head = bh - b * H;
    const int q = blockIdx.x * 32 + r;
    const __bf16 *Qh = Q + (int64_t)bh * T * VB_HD;
    const __bf16 *Kh = K + (int64_t)bh * Tp * VB_HD;
    bf16x8 qb[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int u = 0; u < 8; ++u) qb[s][u] = (__bf16)0.f;
        if (q < T) qb[s] = *(const bf16x8 *)(Qh + (int64_t)q * VB_HD + 16 * s + 8 * h);
    }
    float m = -INFINITY, l = 0.f;
    for (int jb = 0; jb < T; jb += 32) {  // jb + 31 < Tp: Tp is a multiple of 64
        f32x16 st = vb_zero16();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const bf16x8 kf = *(const bf16x8 *)(Kh + (int64_t)(jb + r) * VB_HD + 16 * s + 8 * h);
            st = VB_MFMA(kf, qb[s], st);
        }
        float mx = -INFINITY;
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            if (jb + vb_row(x, h) >= T) st[x] = -INFINITY;
            mx = fmaxf(mx, st[x]);
        }
        const float mnew = fmaxf(m, mx * sl2e);
        const float ms = mnew == -INFINITY ? 0.f : mnew;  // a half with no valid key yet
        float ps = 0.f;
#pragma unroll
        for (int x = 0; x < 16; ++x) ps += __builtin_amdgcn_exp2f(fmaf(st[x], sl2e, -ms));
        l = fmaf(l, __builtin_amdgcn_exp2f(m - ms), ps);
        m = mnew;
    }
    // the two lane halves hold disjoint keys of the same query
    const float mo = __shfl_xor(m, 32), lo = __shfl_xor(l, 32);
    const float M = fmaxf(m, mo);  // finite: key 0 is always valid
    const float m0 = h ? mo : m, l0 = h ? lo : l, m1 = h ? m : mo, l1 = h ? l : lo;
    const float L = l0 * __builtin_amdgcn_exp2f(m0 - M) + l1 * __builtin_amdgcn_exp2f(m1 - M);
    float d = 0.f;
    if (q < T) {
        const int64_t off = ((int64_t)b * T + q) * (int64_t)(H * VB_HD) + head * VB_HD + 32 * h;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const bf16x8 o = *(const bf16x8 *)(AO + off + 8 * s), g = *(const bf16x8 *)(dAO + off + 8 * s);
#pragma unroll
            for (int u = 0; u < 8; ++u) d = fmaf((float)o[u], (float)g[u], d);
        }
    }
    const float dO = __shfl_xor(d, 32);
    if (q < T && h == 0) {
        lse[(int64_t)bh * T + q] = M + __log2f(L);
        dsum[(int64_t)bh * T + q] = d + dO;
    }
}

__global__ void __launch_bounds__(64) k_ab_dkv(const __bf16 *__restrict__ Q,
                                               const __bf16 *__restrict__ K,
                                               const __bf16 *__restrict__ Vt,
                                               const __bf16 *__restrict__ dAO,
                                               const float *__restrict__ lse,
                                               const float *__restrict__ dsum, int T, int Tp, int H,
                                               float sl2e, float scale, __bf16 *__restrict__ dqkv) {
    __shared__ __attribute__((aligned(16))) __bf16 sK[32 * VB_LQ], sV[32 * VB_LQ], sQ[32 * VB_LQ],
        sdO[32 * VB_LQ], sQt[64 * VB_LT], sdOt[64 * VB_LT], sPt[32 * VB_LT], sdSt[32 * VB_LT];
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int bh = blockIdx.y, b = bh / H, head = bh - b * H;
    const int j0 = blockIdx.x * 32;
    const int C = H * VB_HD;
    const __bf16 *Qh = Q + (int64_t)bh * T * VB_HD;
    const __bf16 *dOh = dAO + (int64_t)b * T * C + head * VB_HD;
    vb_stage(K + (int64_t)bh * Tp * VB_HD, VB_HD, j0, Tp, sK, nullptr, lane);
    vb_stage_vt(Vt + (int64_t)bh * VB_HD * Tp, Tp, j0, sV, lane);
    __syncthreads();
    bf16x8 kf[4], vf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        kf[s] = vb_frag(sK, VB_LQ, r, s, h);
        vf[s] = vb_frag(sV, VB_LQ, r, s, h);
    }
    f32x16 dk[2], dv[2];
    dk[0] = dk[1] = dv[0] = dv[1] = vb_zero16();
    bf16x8 nq[4], ng[4];  // the next query tile's Q / dO rows, loaded a tile ahead
    vb_load(Qh, VB_HD, 0, T, nq, lane);
    vb_load(dOh, C, 0, T, ng, lane);
    for (int i0 = 0; i0 < T; i0 += 32) {
        __syncthreads();  // the previous tile's fragment reads are done
        vb_store(nq, sQ, sQt, lane);
        vb_store(ng, sdO, sdOt, lane);
        const bool qok = i0 + r < T;
        const float ls = qok ? lse[(int64_t)bh * T + i0 + r] : 0.f;
        const float dd = qok ? dsum[(int64_t)bh * T + i0 + r] : 0.f;
        if (i0 + 32 < T) {  // in flight under this tile's products
            vb_load(Qh, VB_HD, i0 + 32, T, nq, lane);
            vb_load(dOh, C, i0 + 32, T, ng, lane);
        }
        __syncthreads();
        f32x16 st = vb_zero16(), dp = vb_zero16();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            st = VB_MFMA(kf[s], vb_frag(sQ, VB_LQ, r, s, h), st);
            dp = VB_MFMA(vf[s], vb_frag(sdO, VB_LQ, r, s, h), dp);
        }
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int j = vb_row(x, h);
            const bool ok = qok && j0 + j < T;
            const float p = ok ? __builtin_amdgcn_exp2f(fmaf(st[x], sl2e, -ls)) : 0.f;
            // a single key: the softmax is the constant 1 and its gradient exactly zero (dP - D
            // would leave the rounding difference of two differently ordered sums)
            const float ds = ok && T > 1 ? p * (dp[x] - dd) : 0.f;
            sPt[j * VB_LT + r] = (__bf16)p;
            sdSt[j * VB_LT + r] = (__bf16)ds;
        }
        __syncthreads();
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                dv[nt] = VB_MFMA(vb_frag(sPt, VB_LT, r, s, h), vb_frag(sdOt, VB_LT, 32 * nt + r, s, h), dv[nt]);
                dk[nt] = VB_MFMA(vb_frag(sdSt, VB_LT, r, s, h), vb_frag(sQt, VB_LT, 32 * nt + r, s, h), dk[nt]);
            }
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int tok = j0 + vb_row(x, h);
            if (tok < T) {
                __bf16 *row = dqkv + ((int64_t)b * T + tok) * (int64_t)(3 * C) + head * VB_HD + 32 * nt + r;
                row[C] = (__bf16)(dk[nt][x] * scale);
                row[2 * C] = (__bf16)dv[nt][x];
            }
        }
}

__global__ void __launch_bounds__(64) k_ab_dq(const __bf16 *__restrict__ Q,
                                              const __bf16 *__restrict__ K,
                                              const __bf16 *__restrict__ Vt,
                                              const __bf16 *__restrict__ dAO,
                                              const float *__restrict__ lse,
                                              const float *__restrict__ dsum, int T, int Tp, int H,
                                              float sl2e, float scale, __bf16 *__restrict__ dqkv) {
    __shared__ __attribute__((aligned(16))) __bf16 sQ[32 * VB_LQ], sdO[32 * VB_LQ], sK[32 * VB_LQ],
        sV[32 * VB_LQ], sKt[64 * VB_LT], sdS[32 * VB_LT];
    __shared__ float s_lse[32], s_d[32];
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int bh = blockIdx.y, b = bh / H, head = bh - b * H;
    const int i0 = blockIdx.x * 32;
    const int C = H * VB_HD;
    const __bf16 *Kh = K + (int64_t)bh * Tp * VB_HD;
    const __bf16 *Vh = Vt + (int64_t)bh * VB_HD * Tp;
    vb_stage(Q + (int64_t)bh * T * VB_HD, VB_HD, i0, T, sQ, nullptr, lane);
    vb_stage(dAO + (int64_t)b * T * C + head * VB_HD, C, i0, T, sdO, nullptr, lane);
    if (lane < 32) {
        const bool ok = i0 + lane < T;
        s_lse[lane] = ok ? lse[(int64_t)bh * T + i0 + lane] : 0.f;
        s_d[lane] = ok ? dsum[(int64_t)bh * T + i0 + lane] : 0.f;
    }
    __syncthreads();
    bf16x8 qf[4], gf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        qf[s] = vb_frag(sQ, VB_LQ, r, s, h);
        gf[s] = vb_frag(sdO, VB_LQ, r, s, h);
    }
    float rl[16], rd[16];
#pragma unroll
    for (int x = 0; x < 16; ++x) {
        rl[x] = s_lse[vb_row(x, h)];
        rd[x] = s_d[vb_row(x, h)];
    }
    f32x16 dq[2];
    dq[0] = dq[1] = vb_zero16();
    bf16x8 nk[4], nv[4];  // the next key block's K rows / V^T columns, loaded a block ahead
    vb_load(Kh, VB_HD, 0, Tp, nk, lane);
    vb_load_vt(Vh, Tp, 0, nv, lane);
    for (int j0 = 0; j0 < T; j0 += 32) {  // j0 + 31 < Tp
        __syncthreads();
        vb_store(nk, sK, sKt, lane);
        vb_store_vt(nv, sV, lane);
        if (j0 + 32 < T) {  // in flight under this block's products
            vb_load(Kh, VB_HD, j0 + 32, Tp, nk, lane);
            vb_load_vt(Vh, Tp, j0 + 32, nv, lane);
        }
        __syncthreads();
        f32x16 st = vb_zero16(), dp = vb_zero16();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            st = VB_MFMA(qf[s], vb_frag(sK, VB_LQ, r, s, h), st);
            dp = VB_MFMA(gf[s], vb_frag(sV, VB_LQ, r, s, h), dp);
        }
        const bool kok = j0 + r < T;
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int i = vb_row(x, h);
            const bool ok = kok && i0 + i < T;
            const float p = ok ? __builtin_amdgcn_exp2f(fmaf(st[x], sl2e, -rl[x])) : 0.f;
            sdS[i * VB_LT + r] = (__bf16)(ok && T > 1 ? p * (dp[x] - rd[x]) : 0.f);  // T == 1: k_ab_dkv's note
        }
        __syncthreads();
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int s = 0; s < 2; ++s)
                dq[nt] = VB_MFMA(vb_frag(sdS, VB_LT, r, s, h), vb_frag(sKt, VB_LT, 32 * nt + r, s, h), dq[nt]);
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int tok = i0 + vb_row(x, h);
            if (tok < T)
                dqkv[((int64_t)b * T + tok) * (int64_t)(3 * C) + head * VB_HD + 32 * nt + r] =
                    (__bf16)(dq[nt][x] * scale);
        }
}

extern "C" int sd_attention_bwd(const sd_attn_bwd_args *args, void *stream) {
    if (!args) {
        sd_set_error("sd_attention_bwd: null args");
        return -1;
    }
    const sd_attn_bwd_args &g = *args;
    const bool ok = g.q && g.k && g.vt && g.ao && g.d_ao && g.d_qkv && g.work && g.head_dim == VB_HD &&
                    g.B > 0 && g.heads > 0 && g.tokens > 0 && g.tokens_pad >= g.tokens &&
                    g.tokens_pad % 64 == 0 && g.scale > 0.f &&
                    (int64_t)g.B * g.heads * g.tokens_pad * VB_HD < ((int64_t)1 << 31) &&
                    (int64_t)g.B * g.heads <= 65535 &&
                    ((uintptr_t)g.q | (uintptr_t)g.k | (uintptr_t)g.vt | (uintptr_t)g.ao |
                     (uintptr_t)g.d_ao | (uintptr_t)g.d_qkv | (uintptr_t)g.work) % 16 == 0;
    if (!ok) {
        sd_set_error("sd_attention_bwd: invalid argument (head_dim 64, tokens_pad >= tokens, "
                     "tokens_pad % 64 == 0, scale > 0, 16-byte aligned non-null pointers)");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    const int T = g.tokens, Tp = g.tokens_pad, H = g.heads;
    const float sl2e = g.scale * 1.4426950408889634f;
    float *lse = g.work, *dsum = g.work + (int64_t)g.B * H * T;
    const dim3 grid((unsigned)((T + 31) / 32), (unsigned)(g.B * H));
    hipLaunchKernelGGL(k_ab_stats, grid, dim3(64), 0, s, (const __bf16 *)g.q, (const __bf16 *)g.k,
                       (const __bf16 *)g.ao, (const __bf16 *)g.d_ao, T, Tp, H, sl2e, lse, dsum);
    hipLaunchKernelGGL(k_ab_dkv, grid, dim3(64), 0, s, (const __bf16 *)g.q, (const __bf16 *)g.k,
                       (const __bf16 *)g.vt, (const __bf16 *)g.d_ao, (const float *)lse,
                       (const float *)dsum, T, Tp, H, sl2e, g.scale, (__bf16 *)g.d_qkv);
    hipLaunchKernelGGL(k_ab_dq, grid, dim3(64), 0, s, (const __bf16 *)g.q, (const __bf16 *)g.k,
                       (const __bf16 *)g.vt, (const __bf16 *)g.d_ao, (const float *)lse,
                       (const float *)dsum, T, Tp, H, sl2e, g.scale, (__bf16 *)g.d_qkv);
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_attention_bwd: launch failed");
        return -2;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// LayerNorm backward: one wave per row (k_layernorm's lane layout: 4 consecutive channels
// per 256-channel chunk), a workgroup (4 waves) per part of the rows.  Each wave keeps its
// dw / db partial sums in registers over its rows; the 4 waves add through LDS in wave order
// and k_lb_reduce adds the parts in a fixed order.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float vb_wave_sum(float x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

template <int PER4, bool DYF32>
__global__ void __launch_bounds__(256) k_lb(sd_ln_bwd_args g) {
    __shared__ float red[4][2][256 * PER4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C = g.C;
    const int64_t per = (g.rows + g.nparts - 1) / g.nparts;
    const int64_t r0 = (int64_t)blockIdx.x * per;
    const int64_t r1 = r0 + per < g.rows ? r0 + per : g.rows;
    const float inv_c = 1.f / (float)C;
    vb_f4 wv[PER4], adw[PER4], adb[PER4];
#pragma unroll
    for (int i = 0; i < PER4; ++i) {
        const int c = 4 * lane + 256 * i;
        wv[i] = c < C ? *(const vb_f4 *)(g.w + c) : vb_f4{0.f, 0.f, 0.f, 0.f};
        adw[i] = adb[i] = vb_f4{0.f, 0.f, 0.f, 0.f};
    }
    for (int64_t row = r0 + wave; row < r1; row += 4) {
        const float *xr = g.x + row * C;
        vb_f4 v[PER4], dy[PER4];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < PER4; ++i) {
            const int c = 4 * lane + 256 * i;
            v[i] = dy[i] = vb_f4{0.f, 0.f, 0.f, 0.f};
            if (c < C) {
                v[i] = *(const vb_f4 *)(xr + c);
                if (DYF32) {
                    dy[i] = *(const vb_f4 *)((const float *)g.dy + row * C + c);
                } else {
                    const vb_bf4 t = *(const vb_bf4 *)((const __bf16 *)g.dy + row * C + c);
#pragma unroll
                    for (int u = 0; u < 4; ++u) dy[i][u] = (float)t[u];
                }
            }
            s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
        }
        const float mean = vb_wave_sum(s) * inv_c;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < PER4; ++i) {
            if (4 * lane + 256 * i < C) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float d = v[i][u] - mean;
                    q = fmaf(d, d, q);
                }
            }
        }
        const float rstd = __builtin_amdgcn_rsqf(vb_wave_sum(q) * inv_c + g.eps);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < PER4; ++i) {
            if (4 * lane + 256 * i < C) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float xh = (v[i][u] - mean) * rstd;
                    const float gw = dy[i][u] * wv[i][u];
                    v[i][u] = xh;
                    s1 += gw;
                    s2 = fmaf(gw, xh, s2);
                    adw[i][u] = fmaf(dy[i][u], xh, adw[i][u]);
                    adb[i][u] += dy[i][u];
                }
            }
        }
        const float m1 = vb_wave_sum(s1) * inv_c, m2 = vb_wave_sum(s2) * inv_c;
#pragma unroll
        for (int i = 0; i < PER4; ++i) {
            const int c = 4 * lane + 256 * i;
            if (c < C) {
                float *o = g.dx + row * C + c;
                vb_f4 d;
#pragma unroll
                for (int u = 0; u < 4; ++u) d[u] = rstd * (dy[i][u] * wv[i][u] - m1 - v[i][u] * m2);
                if (g.accumulate) {
                    const vb_f4 old = *(const vb_f4 *)o;
#pragma unroll
                    for (int u = 0; u < 4; ++u) d[u] += old[u];
                }
                *(vb_f4 *)o = d;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < PER4; ++i) {
        const int c = 4 * lane + 256 * i;
        *(vb_f4 *)&red[wave][0][c] = adw[i];
        *(vb_f4 *)&red[wave][1][c] = adb[i];
    }
    __syncthreads();
    float *part = g.work + (int64_t)blockIdx.x * 2 * C;
    for (int c = threadIdx.x; c < 2 * C; c += 256) {
        const int k = c >= C, cc = c - k * C;
        part[c] = ((red[0][k][cc] + red[1][k][cc]) + red[2][k][cc]) + red[3][k][cc];
    }
}

// 32 columns of [dw | db] per workgroup: eight thread groups each add a contiguous eighth of
// the parts in part order, then the eight sums are added in group order (a fixed order: the
// same bits from launch to launch; one thread per column over all the parts took 7 - 60 us)
__global__ void __launch_bounds__(256) k_lb_reduce(const float *__restrict__ work, int nparts, int C,
                                                   float *__restrict__ dw, float *__restrict__ db) {
    __shared__ float red[8][32];
    const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    const int p0 = nparts * sl / 8, p1 = nparts * (sl + 1) / 8;
    float s = 0.f;
    if (c < 2 * C) {
#pragma unroll 4
        for (int p = p0; p < p1; ++p) s += work[(int64_t)p * 2 * C + c];
    }
    red[sl][cl] = s;
    __syncthreads();
    if (sl != 0 || c >= 2 * C) return;
    float *dst = c < C ? dw : db;
    if (!dst) return;
    float t = red[0][cl];
#pragma unroll
    for (int k = 1; k < 8; ++k) t += red[k][cl];
    dst[c < C ? c : c - C] = t;
}

extern "C" int32_t sd_layernorm_bwd_parts(int64_t rows) {
    const int64_t n = (rows + 3) / 4;
    return (int32_t)(n < 1 ? 1 : n > 256 ? 256 : n);
}

extern "C" int sd_layernorm_bwd(const sd_ln_bwd_args *args, void *stream) {
    if (!args) {
        sd_set_error("sd_layernorm_bwd: null args");
        return -1;
    }
    const sd_ln_bwd_args &g = *args;
    const bool ok = g.x && g.w && g.dy && g.dx && g.work && g.rows >= 0 && g.C > 0 && g.C <= 1024 &&
                    g.C % 4 == 0 && g.nparts >= 1 && g.nparts <= 65535 &&
                    ((uintptr_t)g.x | (uintptr_t)g.w | (uintptr_t)g.dy | (uintptr_t)g.dx |
                     (uintptr_t)g.work | (uintptr_t)g.dw | (uintptr_t)g.db) % 16 == 0;
    if (!ok) {
        sd_set_error("sd_layernorm_bwd: invalid argument (C <= 1024, C % 4 == 0, nparts >= 1, "
                     "16-byte aligned non-null x, w, dy, dx, work)");
        return -1;
    }
    if (g.rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int per = (g.C + 255) / 256;
    const dim3 grid((unsigned)g.nparts);
#define SD_LB(PER)                                                                      \
    do {                                                                                \
        if (g.dy_f32)                                                                   \
            hipLaunchKernelGGL((k_lb<PER, true>), grid, dim3(256), 0, s, g);            \
        else                                                                            \
            hipLaunchKernelGGL((k_lb<PER, false>), grid, dim3(256), 0, s, g);           \
    } while (0)
    if (per == 1) SD_LB(1);
    else if (per == 2) SD_LB(2);
    else if (per == 3) SD_LB(3);
    else SD_LB(4);
#undef SD_LB
    if (g.dw || g.db)
        hipLaunchKernelGGL(k_lb_reduce, dim3((unsigned)((2 * g.C + 31) / 32)), dim3(256), 0, s,
                           (const float *)g.work, g.nparts, g.C, g.dw, g.db);
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_layernorm_bwd: launch failed");
        return -2;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// GELU backward (exact erf, SD_EPI_GELU's activation): du = dh (Phi(u) + u phi(u)), f32 math
// on bf16 operands, 8 elements per thread.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_gelu_bwd(const bf16x8 *__restrict__ u,
                                                  const bf16x8 *__restrict__ dh, int64_t n8,
                                                  bf16x8 *__restrict__ du) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const bf16x8 uv = u[i], gv = dh[i];
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float x = (float)uv[j];
        const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752f));
        const float pdf = 0.39894228040143268f * expf(-0.5f * x * x);
        o[j] = (__bf16)((float)gv[j] * (cdf + x * pdf));
    }
    du[i] = o;
}

extern "C" int sd_gelu_bwd(const void *u, const void *dh, int64_t n, void *du, void *stream) {
    if (!u || !dh || !du || n < 0 || n % 8 ||
        ((uintptr_t)u | (uintptr_t)dh | (uintptr_t)du) % 16 != 0) {
        sd_set_error("sd_gelu_bwd: invalid argument (n % 8 == 0, 16-byte aligned)");
        return -1;
    }
    if (n == 0) return 0;
    const int64_t n8 = n / 8;
    hipLaunchKernelGGL(k_gelu_bwd, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, (const bf16x8 *)u, (const bf16x8 *)dh, n8, (bf16x8 *)du);
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_gelu_bwd: launch failed");
        return -2;
    }
    return 0;
}
