// sdhip_stego_train.hip -- StegoClusterHead in train mode on gfx950 (CDNA4).
//
// Reference: scenedino/downstream_head/semantic_head.py:285-305 under forward_training
// (:122-235), whose inputs are always detached: weight gradients only, no input gradient.
// Forward, per row (1x1 convolutions as matrices; Dropout2d as per-group column scales):
//   xh  = x / max(|x|, 1e-10)      (normalize; x as given otherwise)
//   lin = Wl xh + bl,  mid = relu(Wn1 xh + bn1),  non = Wn2 mid + bn2
//   e   = m_lin o lin + m_non o non,   y = e / max(|e|, 1e-10)
// Backward from dy (M, 64):
//   n = max(|e|, 1e-10),  de = (dy - y (y . dy)) / n   (|e| < 1e-10: de = dy / 1e-10, the
//   clamp is a constant denominator -- sd_expand_bwd's rule),
//   dlin = m_lin o de,  dnon = m_non o de,  dmid = (Wn2^T dnon) o [mid > 0]
// written as bf16 rows; the six parameter gradients are sd_conv_wgrad calls (taps = 1) on
// them and the saved xh / mid rows (downstream_head/semantic_head.py).
//
// Work unit: one wave = 32 rows (lane = row, the column of v_mfma_f32_32x32x16_bf16's B
// operand, as in k_expand_bwd), four waves per workgroup.  xh stays in registers as B operands
// (d_in / 16 k-steps); mid is never held: each 32-feature tile of it is converted in place into
// the B operand of Wn2's product (the k permutation of sdhip_expand_bwd.hip) and, when saved,
// stored as bf16 rows.  The forward's A operands come from LDS: the workgroup stages one
// 32-row tile of [Wl; Wn1] (and the matching 64 x 32 slice of Wn2) per step, double-buffered,
// the next tile's global loads in flight under the current tile's MFMAs (a wave alone, at one
// wave per SIMD, waited a full L2 round trip per MFMA).  The backward reads Wn2^T from global.
// No atomics, no cross-wave sum: a repeated launch gives the same bits.
#include "sdhip_common.h"

extern "C" void sd_set_error(const char *msg);

#define ST_DC 64  // code dims
#define ST_EPS 1e-10f
#define ST_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

typedef __attribute__((ext_vector_type(4))) float st_f4;
typedef __attribute__((ext_vector_type(4))) __bf16 st_h4;

// A operand, natural k: lane (r, hh) holds W[row][k0 + 8 hh .. + 7]
__device__ __forceinline__ bf16x8 st_a_nat(const __bf16 *__restrict__ W, int ld, int row, int k0,
                                           int hh) {
    return *(const bf16x8 *)(W + (int64_t)row * ld + k0 + 8 * hh);
}

// A operand, permuted k (the B operand is an accumulator half converted in place): element j
// <- column c0 + 8 (j >> 2) + 4 hh + (j & 3)
__device__ __forceinline__ bf16x8 st_a_perm(const __bf16 *__restrict__ W, int ld, int row, int c0,
                                            int hh) {
    const __bf16 *p = W + (int64_t)row * ld + c0 + 4 * hh;
    const st_h4 lo = *(const st_h4 *)p, hi = *(const st_h4 *)(p + 8);
    bf16x8 a;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        a[j] = lo[j];
        a[4 + j] = hi[j];
    }
    return a;
}

// accumulator registers 8 s .. 8 s + 7 as a bf16 B operand
__device__ __forceinline__ bf16x8 st_cvt(const f32x16 &acc, int s) {
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (__bf16)acc[8 * s + j];
    return r;
}

// the same with relu: max with +0 on the 16-bit patterns (k_seg_head's sg_relu_b)
__device__ __forceinline__ bf16x8 st_relu(const f32x16 &acc, int s) {
    typedef __attribute__((ext_vector_type(8))) short s16x8_t;
    s16x8_t v = __builtin_bit_cast(s16x8_t, st_cvt(acc, s));
    v = __builtin_elementwise_max(v, (s16x8_t)0);
    return __builtin_bit_cast(bf16x8, v);
}

// vec[32 t + (i & 3) + 8 (i >> 2) + 4 hh], i = 0..15: the rows lane half hh holds of tile t;
// vec == NULL: ones (the dropout scales of a pass without dropout)
__device__ __forceinline__ f32x16 st_rows(const float *__restrict__ vec, int t, int hh) {
    f32x16 r;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        st_f4 v = {1.f, 1.f, 1.f, 1.f};
        if (vec) v = *(const st_f4 *)(vec + 32 * t + 8 * g + 4 * hh);
        r[4 * g] = v[0]; r[4 * g + 1] = v[1]; r[4 * g + 2] = v[2]; r[4 * g + 3] = v[3];
    }
    return r;
}

// a B operand (k-step q of a row) to bf16 row storage: elements 0..3 at column
// 16 q + 4 hh, 4..7 at 16 q + 8 + 4 hh
__device__ __forceinline__ void st_store_b(__bf16 *row, int q, int hh, const bf16x8 &v) {
    st_h4 lo, hi;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        lo[j] = v[j];
        hi[j] = v[4 + j];
    }
    *(st_h4 *)(row + 16 * q + 4 * hh) = lo;
    *(st_h4 *)(row + 16 * q + 8 + 4 * hh) = hi;
}

// an accumulator tile t of a (M, 64) f32 row: registers 4 g + e <- column 32 t + 8 g + 4 hh + e
__device__ __forceinline__ f32x16 st_load_c(const float *__restrict__ row, int t, int hh, bool ok) {
    f32x16 d;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        st_f4 v = {0.f, 0.f, 0.f, 0.f};
        if (ok) v = *(const st_f4 *)(row + 32 * t + 8 * g + 4 * hh);
        d[4 * g] = v[0]; d[4 * g + 1] = v[1]; d[4 * g + 2] = v[2]; d[4 * g + 3] = v[3];
    }
    return d;
}
__device__ __forceinline__ void st_store_c(float *row, int t, int hh, const f32x16 &acc) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
        *(st_f4 *)(row + 32 * t + 8 * g + 4 * hh) =
            st_f4{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
}

// LDS of k_stego_fwd: two buffers of one staged weight tile each -- 32 rows of Wl / Wn1 (rows
// padded by 16 B against bank conflicts of the 16-B A reads) and the matching 64 x 32 slice
// of Wn2 (rows padded to 80 B)
#define ST_W2LD 40
template <int DIN>
struct st_lds {
    static constexpr int LDW = DIN + 8;
    static constexpr int TILE = 32 * LDW;         // bf16 elements
    static constexpr int SLICE = ST_DC * ST_W2LD;  // bf16 elements
    static constexpr int BYTES = 2 * (TILE + SLICE) * 2;
};

template <int DIN>
__global__ void __launch_bounds__(256) k_stego_fwd(const sd_stego_train_args a) {
    constexpr int NK = DIN / 16, LDW = st_lds<DIN>::LDW;
    constexpr int NT = DIN / 32 + ST_DC / 32;  // staged tiles: Wn1's, then Wl's two
    constexpr int CH = 32 * (DIN / 8) / 256;   // 16-B chunks of a tile per thread
    extern __shared__ __attribute__((aligned(16))) unsigned char st_smem[];
    __bf16 *wt = (__bf16 *)st_smem;                       // [2][TILE]
    __bf16 *w2 = wt + 2 * st_lds<DIN>::TILE;              // [2][SLICE]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    // every wave stays to the end (barriers below); a wave past M computes on zeros
    const int64_t p = ((int64_t)blockIdx.x * 4 + wave) * 32 + r;
    const bool ok = p < a.M;  // ragged last tile: rows past M compute on zeros, store nothing
    const __bf16 *wl = (const __bf16 *)a.wl, *wn1 = (const __bf16 *)a.wn1;
    const __bf16 *wn2 = (const __bf16 *)a.wn2;

    // ---- weight tile t (32 rows of Wn1, t < DIN / 32, with Wn2[:, 32 t ..]; then Wl's two
    //      tiles) global -> registers -> LDS, in two halves of CH / 2 chunks per thread ----
    constexpr int NM = DIN / 32, HC = CH / 2;
    bf16x8 pre[HC], pre2;
    auto gload = [&](int t, int half) {
        const __bf16 *src = t < NM ? wn1 + (int64_t)t * 32 * DIN : wl + (int64_t)(t - NM) * 32 * DIN;
#pragma unroll
        for (int i = 0; i < HC; ++i) pre[i] = *(const bf16x8 *)(src + (tid + 256 * (half * HC + i)) * 8);
        if (t < NM && half == 0)
            pre2 = *(const bf16x8 *)(wn2 + (tid >> 2) * DIN + 32 * t + 8 * (tid & 3));
    };
    auto lstore = [&](int t, int half, int b) {
#pragma unroll
        for (int i = 0; i < HC; ++i) {
            const int q = tid + 256 * (half * HC + i), row = q / (DIN / 8), c8 = q % (DIN / 8);
            *(bf16x8 *)(wt + b * st_lds<DIN>::TILE + row * LDW + 8 * c8) = pre[i];
        }
        if (t < NM && half == 0)
            *(bf16x8 *)(w2 + b * st_lds<DIN>::SLICE + (tid >> 2) * ST_W2LD + 8 * (tid & 3)) = pre2;
    };
    gload(0, 0);
    lstore(0, 0, 0);
    gload(0, 1);
    lstore(0, 1, 0);

    // ---- xh = x / max(|x|, eps) as B operands (k-step s: dims 16 s + 8 hh .. + 7) ----
    const st_f4 *src = (const st_f4 *)(a.x + (ok ? p : 0) * DIN);
    float n2 = 0.f;
    if (ok && a.normalize) {
#pragma unroll 4
        for (int s = 0; s < NK; ++s) {
            const st_f4 u = src[4 * s + 2 * hh], v = src[4 * s + 2 * hh + 1];
#pragma unroll
            for (int j = 0; j < 4; ++j) n2 = fmaf(u[j], u[j], n2);
#pragma unroll
            for (int j = 0; j < 4; ++j) n2 = fmaf(v[j], v[j], n2);
        }
    }
    n2 += __shfl_xor(n2, 32);
    const float xinv = a.normalize ? 1.f / fmaxf(sqrtf(n2), ST_EPS) : 1.f;
    bf16x8 xb[NK];
#pragma unroll
    for (int s = 0; s < NK; ++s) {
        st_f4 u = {0.f, 0.f, 0.f, 0.f}, v = {0.f, 0.f, 0.f, 0.f};
        if (ok) {
            u = src[4 * s + 2 * hh];
            v = src[4 * s + 2 * hh + 1];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            xb[s][j] = (__bf16)(u[j] * xinv);
            xb[s][4 + j] = (__bf16)(v[j] * xinv);
        }
    }
    if (a.xh && ok) {
        bf16x8 *dst = (bf16x8 *)a.xh + p * (DIN / 8);
#pragma unroll
        for (int s = 0; s < NK; ++s) dst[2 * s + hh] = xb[s];
    }
    __syncthreads();

    // ---- staged tiles.  Per 32-feature tile of mid: relu(Wn1 xh + bn1), then
    //      non += Wn2[:, tile] mid; last, lin = Wl xh + bl (so lin is not live across the
    //      sweep).  Tile t + 1 is in flight from global, half by half, while tile t's MFMAs
    //      read LDS; one barrier per tile (double buffer) ----
    f32x16 lin[ST_DC / 32], non[ST_DC / 32];
#pragma unroll
    for (int t = 0; t < ST_DC / 32; ++t) non[t] = st_rows(a.bn2, t, hh);
#pragma unroll 1
    for (int t = 0; t < NT; ++t) {
        const int b = t & 1;
        const bool more = t + 1 < NT;
        const __bf16 *wrow = wt + b * st_lds<DIN>::TILE + r * LDW + 8 * hh;
        f32x16 acc = t < NM ? st_rows(a.bn1, t, hh) : st_rows(a.bl, t - NM, hh);
        if (more) gload(t + 1, 0);
#pragma unroll
        for (int s = 0; s < NK / 2; ++s) {
            // at most 8 LDS reads ahead: hoisting the whole half costs the registers xh needs
            if (s % 8 == 0) __builtin_amdgcn_sched_barrier(0);
            acc = ST_MFMA(*(const bf16x8 *)(wrow + 16 * s), xb[s], acc);
        }
        if (more) {
            lstore(t + 1, 0, b ^ 1);
            gload(t + 1, 1);
        }
#pragma unroll
        for (int s = NK / 2; s < NK; ++s) {
            if (s % 8 == 0) __builtin_amdgcn_sched_barrier(0);
            acc = ST_MFMA(*(const bf16x8 *)(wrow + 16 * s), xb[s], acc);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (more) lstore(t + 1, 1, b ^ 1);
        if (t < NM) {
            const bf16x8 mb[2] = {st_relu(acc, 0), st_relu(acc, 1)};
            if (a.mid && ok) {
                __bf16 *row = (__bf16 *)a.mid + p * DIN + 32 * t;
                st_store_b(row, 0, hh, mb[0]);
                st_store_b(row, 1, hh, mb[1]);
            }
            const __bf16 *w2b = w2 + b * st_lds<DIN>::SLICE;
#pragma unroll
            for (int ct = 0; ct < ST_DC / 32; ++ct)
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    non[ct] = ST_MFMA(st_a_perm(w2b, ST_W2LD, 32 * ct + r, 16 * s, hh), mb[s], non[ct]);
        } else if (t == NM) {
            lin[0] = acc;
        } else {
            lin[1] = acc;
        }
        __syncthreads();
    }

    // ---- e = m_lin o lin + m_non o non, y = e / max(|e|, eps) ----
    const int64_t grp = ok ? p / a.rows_per_group : 0;
    const float *ml = a.m_lin ? a.m_lin + grp * ST_DC : nullptr;
    const float *mn = a.m_non ? a.m_non + grp * ST_DC : nullptr;
    float e2 = 0.f;
#pragma unroll
    for (int t = 0; t < ST_DC / 32; ++t) {
        const f32x16 sl = st_rows(ml, t, hh), sn = st_rows(mn, t, hh);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            lin[t][i] = sl[i] * lin[t][i] + sn[i] * non[t][i];
            e2 = fmaf(lin[t][i], lin[t][i], e2);
        }
    }
    e2 += __shfl_xor(e2, 32);
    const float einv = 1.f / fmaxf(sqrtf(e2), ST_EPS);
    if (ok) {
        if (a.e) {
            float *row = a.e + p * ST_DC;
#pragma unroll
            for (int t = 0; t < ST_DC / 32; ++t) st_store_c(row, t, hh, lin[t]);
        }
        float *row = a.y + p * ST_DC;
#pragma unroll
        for (int t = 0; t < ST_DC / 32; ++t) {
            f32x16 yv;
#pragma unroll
            for (int i = 0; i < 16; ++i) yv[i] = lin[t][i] * einv;
            st_store_c(row, t, hh, yv);
        }
    }
}

__global__ void __launch_bounds__(256) k_stego_bwd(const sd_stego_train_args a) {
    const int DIN = a.d_in;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int64_t p0 = ((int64_t)blockIdx.x * 4 + wave) * 32;
    if (p0 >= a.M) return;
    const int64_t p = p0 + r;
    const bool ok = p < a.M;
    const int64_t pr = ok ? p : 0;
    const __bf16 *wn2t = (const __bf16 *)a.wn2t;

    // ---- de from e and dy (f32) ----
    f32x16 e[ST_DC / 32], d[ST_DC / 32];
    float n2 = 0.f, edy = 0.f;
#pragma unroll
    for (int t = 0; t < ST_DC / 32; ++t) {
        e[t] = st_load_c(a.e + pr * ST_DC, t, hh, ok);
        d[t] = st_load_c(a.dy + pr * ST_DC, t, hh, ok);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            n2 = fmaf(e[t][i], e[t][i], n2);
            edy = fmaf(e[t][i], d[t][i], edy);
        }
    }
    n2 += __shfl_xor(n2, 32);
    edy += __shfl_xor(edy, 32);
    // de = (dy - e c) inv: inv = 1 / n, c = (e . dy) / n^2; n < eps: de = dy / eps
    const float n = sqrtf(n2);
    float inv = 1.f / ST_EPS, c = 0.f;
    if (n >= ST_EPS) {
        inv = 1.f / n;
        c = (edy * inv) * inv;
    }
    const float *ml = a.m_lin ? a.m_lin + (pr / a.rows_per_group) * ST_DC : nullptr;
    const float *mn = a.m_non ? a.m_non + (pr / a.rows_per_group) * ST_DC : nullptr;
    bf16x8 dnb[ST_DC / 16];
#pragma unroll
    for (int t = 0; t < ST_DC / 32; ++t) {
        const f32x16 sl = st_rows(ml, t, hh), sn = st_rows(mn, t, hh);
        f32x16 dl, dn;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float de = (d[t][i] - e[t][i] * c) * inv;
            dl[i] = sl[i] * de;
            dn[i] = sn[i] * de;
        }
        dnb[2 * t] = st_cvt(dn, 0);
        dnb[2 * t + 1] = st_cvt(dn, 1);
        if (ok) {
            if (a.dlin) {
                __bf16 *row = (__bf16 *)a.dlin + p * ST_DC + 32 * t;
                st_store_b(row, 0, hh, st_cvt(dl, 0));
                st_store_b(row, 1, hh, st_cvt(dl, 1));
            }
            if (a.dnon) {
                __bf16 *row = (__bf16 *)a.dnon + p * ST_DC + 32 * t;
                st_store_b(row, 0, hh, dnb[2 * t]);
                st_store_b(row, 1, hh, dnb[2 * t + 1]);
            }
        }
    }
    if (!a.dmid) return;

    // ---- dmid = (Wn2^T dnon) o [mid > 0], per 32-feature tile ----
    for (int mt = 0; mt < DIN / 32; ++mt) {
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int q = 0; q < ST_DC / 16; ++q)
            acc = ST_MFMA(st_a_perm(wn2t, ST_DC, 32 * mt + r, 16 * q, hh), dnb[q], acc);
        if (ok) {
            // mid was stored by st_store_b: register 8 s + j of this tile lies at column
            // 32 mt + 16 s + 8 (j >> 2) + 4 hh + (j & 3); relu'd, so +0 or positive
            const uint16_t *mrow = (const uint16_t *)a.mid + p * DIN + 32 * mt;
            __bf16 *drow = (__bf16 *)a.dmid + p * DIN + 32 * mt;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                typedef __attribute__((ext_vector_type(4))) uint16_t u16x4_t;
                const u16x4_t lo = *(const u16x4_t *)(mrow + 16 * s + 4 * hh);
                const u16x4_t hi = *(const u16x4_t *)(mrow + 16 * s + 8 + 4 * hh);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (lo[j] == 0) acc[8 * s + j] = 0.f;
                    if (hi[j] == 0) acc[8 * s + 4 + j] = 0.f;
                }
                st_store_b(drow, s, hh, st_cvt(acc, s));
            }
        }
    }
}

static bool st_common_ok(const sd_stego_train_args *a) {
    return a && a->M >= 1 && (a->d_in == 384 || a->d_in == 768) && a->d_code == ST_DC &&
           a->rows_per_group >= 1 && (a->M + 127) / 128 <= 0x7fffffffLL &&
           ((!a->m_lin && !a->m_non) || (a->M - 1) / a->rows_per_group < a->n_groups);
}

extern "C" int sd_stego_train_fwd(const sd_stego_train_args *a, void *stream) {
    const bool ptrs = a && a->x && a->wl && a->wn1 && a->wn2 && a->bl && a->bn1 && a->bn2 && a->y;
    if (!ptrs || !st_common_ok(a) ||
        (((uintptr_t)a->x | (uintptr_t)a->wl | (uintptr_t)a->wn1 | (uintptr_t)a->wn2 |
          (uintptr_t)a->bl | (uintptr_t)a->bn1 | (uintptr_t)a->bn2 | (uintptr_t)a->m_lin |
          (uintptr_t)a->m_non | (uintptr_t)a->y | (uintptr_t)a->xh | (uintptr_t)a->mid |
          (uintptr_t)a->e) & 15)) {
        sd_set_error("sd_stego_train_fwd: invalid argument (M >= 1, d_in 384 or 768, d_code 64, "
                     "rows_per_group >= 1 with enough mask groups, 16-B aligned non-null operands)");
        return -1;
    }
    const unsigned nblk = (unsigned)((a->M + 127) / 128);
    hipStream_t s = (hipStream_t)stream;
    if (a->d_in == 768) {
        sd_lds_attr((const void *)k_stego_fwd<768>, st_lds<768>::BYTES);
        hipLaunchKernelGGL((k_stego_fwd<768>), dim3(nblk), dim3(256), st_lds<768>::BYTES, s, *a);
    } else {
        sd_lds_attr((const void *)k_stego_fwd<384>, st_lds<384>::BYTES);
        hipLaunchKernelGGL((k_stego_fwd<384>), dim3(nblk), dim3(256), st_lds<384>::BYTES, s, *a);
    }
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_stego_train_fwd: launch failed");
        return -2;
    }
    return 0;
}

extern "C" int sd_stego_train_bwd(const sd_stego_train_args *a, void *stream) {
    const bool ptrs = a && a->e && a->dy && (!a->dmid || (a->mid && a->wn2t));
    if (!ptrs || !st_common_ok(a) ||
        (((uintptr_t)a->e | (uintptr_t)a->dy | (uintptr_t)a->mid | (uintptr_t)a->wn2t |
          (uintptr_t)a->m_lin | (uintptr_t)a->m_non | (uintptr_t)a->dlin | (uintptr_t)a->dnon |
          (uintptr_t)a->dmid) & 15)) {
        sd_set_error("sd_stego_train_bwd: invalid argument (M >= 1, d_in 384 or 768, d_code 64, "
                     "rows_per_group >= 1 with enough mask groups, e and dy, mid and wn2t with "
                     "dmid, 16-B aligned operands)");
        return -1;
    }
    const unsigned nblk = (unsigned)((a->M + 127) / 128);
    hipLaunchKernelGGL(k_stego_bwd, dim3(nblk), dim3(256), 0, (hipStream_t)stream, *a);
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_stego_train_bwd: launch failed");
        return -2;
    }
    return 0;
}
