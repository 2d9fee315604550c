// sdhip_stego_corr.hip -- the downstream stage's STEGO correlation loss on gfx950 (CDNA4), forward
// and backward, without a (nc, P, Q) tensor in memory
// (scenedino/downstream_head/semantic_head.py:181-188,268-270 builds the six correlation tensors,
// scenedino/losses/stego_loss.py:40-46,71-79 reduces them; scenedino_amd/losses/stego_loss.py holds
// the same arithmetic in torch ops).
//
// For one pair with A, B the DINO rows (nc, P, d) / (nc, Q, d), a, b the code rows (.., 64),
// x^ = x / max(|x|, 1e-10), D = A^ B^T, S = a^ b^T, N = nc P Q:
//   loss = -w / N sum max(S, 0) (D' - shift),   D' = D                      (pointwise off)
//                                               D' = D - r[n, p] + g        (pointwise on)
// with r[n, p] = A^[n, p] . mean_q B^[n, q] the row mean of D and g = mean r (the reference
// removes the row means and restores the global mean; the second mean it removes is zero).
// Up to three pairs share the A side; a pair without partner rows is the self pair (B = A, b = a).
//
// Prep (k_sc_norm, one wave per row): bf16 copies of the normalised DINO and code rows and the
// inverse norms of the code rows.  Pointwise: k_sc_bbar (the mean of the bf16 B^ rows the MFMA
// reads, so r is the row mean of the D that is computed), k_sc_rmean (r), k_sc_g (g).
//
// Sweeps.  A workgroup is one wave that owns 32 rows of one crop ("owner" side) and walks the
// other side's rows 32 at a time; every product is a 32 x 32 x 16 bf16 MFMA in the NT form of
// sdhip_vit_bwd.hip (A operand lane (r, h) reads row r, reduction columns 16 s + 8 h .. + 7; the
// accumulator register x of lane (r, h) holds C[8 (x / 4) + 4 h + x % 4][r]).  The owner's DINO
// tile sits in LDS (32 x d bf16), its code fragments in registers; the swept DINO rows come
// straight from global memory (L2) in groups of eight fragments, one group ahead of the MFMAs;
// the swept code tile goes through LDS (row-major for S, transposed for the gradient product),
// loaded a tile ahead.  Ragged tiles are masked.
//   k_sc_fwd  owner = 32 p rows, every pair: sum max(S, 0) D'' (D'' = D' - shift) per pair, one
//             partial per workgroup; k_sc_final adds them in index order and scales by -w / N.
//   k_sc_bwd  recomputes D and S twice: the p-owned sweep gives da^ = sum_pairs sum_q G b^ with
//             G = -w up / N 1[S > 0] D'' (rounded to bf16 for the second MFMA), the q-owned
//             sweep of each pair gives db^ = sum_p G a^; both write f32 rows that one workgroup
//             owns.  k_sc_bwd_fin applies the normalisation rule dx = (dx^ - x^ (x^ . dx^)) /
//             max(|x|, 1e-10) and, for a self pair, adds both sides first.
// No atomics: every sum has one owner or is added in index order; a repeated launch gives the
// same bits.  The upstream gradients (one per pair) are read from device memory.
#include "sdhip_common.h"

#include <stdio.h>

extern "C" void sd_set_error(const char *msg);

typedef __attribute__((ext_vector_type(4))) __bf16 sc_bf4;

#define SC_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)
#define SC_CODE 64
#define SC_LA(D) ((D) + 8)   // bf16 per LDS row of the owner's DINO tile (1552-B / 784-B rows:
                             // consecutive rows start four banks apart)
#define SC_LQ 72             // bf16 per LDS row of a 32 x 64 tile
#define SC_LT 40             // bf16 per LDS row of a 64 x 32 / 32 x 32 tile
#define SC_EPS 1e-10f
#define SC_MAX_ROWS (1 << 24)

__device__ __forceinline__ f32x16 sc_zero16() {
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    return z;
}
__device__ __forceinline__ bf16x8 sc_zero8() {
    bf16x8 z;
#pragma unroll
    for (int i = 0; i < 8; ++i) z[i] = (__bf16)0.f;
    return z;
}
__device__ __forceinline__ int sc_row(int x, int h) { return 8 * (x >> 2) + 4 * h + (x & 3); }
__device__ __forceinline__ bf16x8 sc_frag(const __bf16 *tile, int ld, int r, int s, int h) {
    return *(const bf16x8 *)(tile + r * ld + 16 * s + 8 * h);
}
// butterfly sum: every lane ends with the same value, the same bits on every launch
__device__ __forceinline__ float sc_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// ------------------------------------------------------------------------ work layout
struct ScLayout {
    int64_t dino_a, code_a, inv_a, dhat_a, part;       // byte offsets
    int64_t dino_b[3], code_b[3], inv_b[3], bbar[3], rmean[3], dhat_b[3];
    int64_t g;
    int64_t total;
    int64_t rows_a, rows_b[3];  // rows_b: 0 for a self pair
    int32_t Qi[3];              // swept rows of the pair (P for a self pair)
    int32_t tiles_p;
    int64_t nwg_p;
};

static int64_t sc_up(int64_t v) { return (v + 255) & ~(int64_t)255; }

static ScLayout sc_layout(int64_t nc, int P, int Q, int d, int n_pairs, const bool *self) {
    ScLayout L = {};
    int64_t o = 0;
    auto take = [&](int64_t bytes) { int64_t at = o; o += sc_up(bytes); return at; };
    L.rows_a = nc * P;
    L.tiles_p = (P + 31) / 32;
    L.nwg_p = nc * L.tiles_p;
    L.dino_a = take(L.rows_a * d * 2);
    L.code_a = take(L.rows_a * SC_CODE * 2);
    L.inv_a = take(L.rows_a * 4);
    L.dhat_a = take(L.rows_a * SC_CODE * 4);
    L.part = take(3 * L.nwg_p * 4);
    L.g = take(16);
    for (int i = 0; i < 3; ++i) {
        const bool on = i < n_pairs;
        const bool sf = on && self[i];
        L.rows_b[i] = on && !sf ? nc * Q : 0;
        L.Qi[i] = sf ? P : Q;
        L.dino_b[i] = sf ? L.dino_a : take(L.rows_b[i] * d * 2);
        L.code_b[i] = sf ? L.code_a : take(L.rows_b[i] * SC_CODE * 2);
        L.inv_b[i] = sf ? L.inv_a : take(L.rows_b[i] * 4);
        L.bbar[i] = take(on ? nc * d * 4 : 0);
        L.rmean[i] = take(on ? L.rows_a * 4 : 0);
        L.dhat_b[i] = take(on ? nc * (int64_t)L.Qi[i] * SC_CODE * 4 : 0);
    }
    L.total = o;
    return L;
}

// ------------------------------------------------------------------------ prep
struct ScNormJobs {
    const void *src[8];
    __bf16 *dst[8];
    float *inv[8];       // null: not kept
    int64_t start[9];    // first global row of the set; start[n] = all rows
    int32_t width[8], f32[8];
    int32_t n;
};

__global__ void __launch_bounds__(256) k_sc_norm(const ScNormJobs J) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= J.start[J.n]) return;
    int s = 0;
    while (s + 1 < J.n && row >= J.start[s + 1]) ++s;
    const int64_t lr = row - J.start[s];
    const int W = J.width[s];
    f32x4 v[3];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = 4 * lane + 256 * i;
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < W) {
            if (J.f32[s]) {
                v[i] = *(const f32x4 *)((const float *)J.src[s] + lr * W + c);
            } else {
                const sc_bf4 b = *(const sc_bf4 *)((const __bf16 *)J.src[s] + lr * W + c);
#pragma unroll
                for (int u = 0; u < 4; ++u) v[i][u] = (float)b[u];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) ss = fmaf(v[i][u], v[i][u], ss);
    }
    const float den = fmaxf(sqrtf(sc_wave_sum(ss)), SC_EPS);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = 4 * lane + 256 * i;
        if (c < W) {
            sc_bf4 b;
#pragma unroll
            for (int u = 0; u < 4; ++u) b[u] = (__bf16)(v[i][u] / den);
            *(sc_bf4 *)(J.dst[s] + lr * W + c) = b;
        }
    }
    if (lane == 0 && J.inv[s]) J.inv[s][lr] = 1.f / den;
}

struct ScPoint {
    const __bf16 *dino_a;
    const __bf16 *dino_b[3];
    float *bbar[3], *rmean[3];
    float *g;
    int32_t Qi[3];
    int32_t P, d;
    int64_t rows_a;
};

// grid (nc, n_pairs): bbar[i][n][c] = mean_q B^[n, q, c]
__global__ void __launch_bounds__(256) k_sc_bbar(const ScPoint a) {
    const int n = blockIdx.x, i = blockIdx.y, Q = a.Qi[i], d = a.d;
    const __bf16 *B = a.dino_b[i] + (int64_t)n * Q * d;
    for (int cp = threadIdx.x; 2 * cp < d; cp += 256) {
        float s0 = 0.f, s1 = 0.f;
        for (int q = 0; q < Q; ++q) {
            const uint32_t w = *(const uint32_t *)(B + (int64_t)q * d + 2 * cp);
            s0 += bf16lo(w);
            s1 += bf16hi(w);
        }
        a.bbar[i][(int64_t)n * d + 2 * cp] = s0 / (float)Q;
        a.bbar[i][(int64_t)n * d + 2 * cp + 1] = s1 / (float)Q;
    }
}

// grid (ceil(rows_a / 4), n_pairs), one wave per row: rmean[i][row] = A^[row] . bbar[i][n]
__global__ void __launch_bounds__(256) k_sc_rmean(const ScPoint a) {
    const int lane = threadIdx.x & 63, i = blockIdx.y, d = a.d;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows_a) return;
    const int64_t n = row / a.P;
    const __bf16 *x = a.dino_a + row * d;
    const float *m = a.bbar[i] + n * d;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int c = 4 * lane + 256 * k;
        if (c < d) {
            const sc_bf4 b = *(const sc_bf4 *)(x + c);
            const f32x4 mv = *(const f32x4 *)(m + c);
#pragma unroll
            for (int u = 0; u < 4; ++u) s = fmaf((float)b[u], mv[u], s);
        }
    }
    s = sc_wave_sum(s);
    if (lane == 0) a.rmean[i][row] = s;
}

// fixed-order block sum over 256 threads
__device__ __forceinline__ float sc_block_sum(float v, float *red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// grid (n_pairs): g[i] = mean rmean[i]
__global__ void __launch_bounds__(256) k_sc_g(const ScPoint a) {
    __shared__ float red[256];
    const int i = blockIdx.x;
    float s = 0.f;
    for (int64_t k = threadIdx.x; k < a.rows_a; k += 256) s += a.rmean[i][k];
    s = sc_block_sum(s, red);
    if (threadIdx.x == 0) a.g[i] = s / (float)a.rows_a;
}

// ------------------------------------------------------------------------ sweeps
struct ScSweep {
    const __bf16 *dino_a, *code_a;
    const __bf16 *dino_b[3], *code_b[3];
    const float *rmean[3];   // null: pointwise off
    const float *g;
    const float *up;         // bwd: (3) upstream gradients
    float *part;             // fwd: (3, nwg_p)
    float *dhat_a, *dhat_b[3];
    float weight[3], shift[3];
    int32_t Qi[3];
    int64_t nq_start[4];     // bwd: first workgroup of each pair's q-owned sweep (after nwg_p)
    int64_t nwg_p;
    int32_t P, n_pairs, tiles_p;
};

template <int D>
struct ScLds {
    __bf16 own[32 * SC_LA(D)];
    __bf16 y[32 * SC_LQ];
    __bf16 yt[SC_CODE * SC_LT];
    __bf16 gt[32 * SC_LT];
};

// rows x0 .. x0 + 31 of X (per-crop base, row stride d) into the owner tile; rows >= limit as zero
template <int D>
__device__ __forceinline__ void sc_stage_owner(const __bf16 *X, int x0, int limit, __bf16 *own,
                                               int lane) {
    constexpr int per_row = D / 8, chunks = 32 * per_row;
#pragma unroll 4
    for (int c = lane; c < chunks; c += 64) {
        const int row = c / per_row, col = (c - row * per_row) * 8;
        bf16x8 v = sc_zero8();
        if (x0 + row < limit) v = *(const bf16x8 *)(X + (int64_t)(x0 + row) * D + col);
        *(bf16x8 *)(own + row * SC_LA(D) + col) = v;
    }
}

// swept code rows y0 .. y0 + 31 (row stride 64) as four 16-B chunks per lane; split into the
// global loads and the LDS stores (row-major and transposed tiles) so that the next tile's rows
// are in flight under the current tile's products
__device__ __forceinline__ void sc_load_code(const __bf16 *Yc, int y0, int limit, bf16x8 (&v)[4],
                                             int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i, row = c >> 3, col = (c & 7) * 8;
        v[i] = sc_zero8();
        if (y0 + row < limit) v[i] = *(const bf16x8 *)(Yc + (int64_t)(y0 + row) * SC_CODE + col);
    }
}
__device__ __forceinline__ void sc_store_code(const bf16x8 (&v)[4], __bf16 *rm, __bf16 *tr, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i, row = c >> 3, col = (c & 7) * 8;
        *(bf16x8 *)(rm + row * SC_LQ + col) = v[i];
#pragma unroll
        for (int u = 0; u < 8; ++u) tr[(col + u) * SC_LT + row] = v[i][u];
    }
}

// One owner tile against every swept row of one pair.
//   own_r[x]: the row mean of owner row sc_row(x, h) (p-owned sweep) or 0
//   swp_r:    per-crop row means of the swept side (q-owned sweep) or null
//   cst:      g - shift;  coef: -w up / N (bwd)
// fwd: returns this lane's sum of max(S, 0) D''; bwd: adds G y^ into dx.
template <bool BWD, int D>
__device__ __forceinline__ float sc_pair(ScLds<D> &L, const bf16x8 (&of)[4], const __bf16 *Yd,
                                         const __bf16 *Yc, int Y, int x0, int X,
                                         const float (&own_r)[16], const float *swp_r, float cst,
                                         float coef, f32x16 (&dx)[2], int lane) {
    const int r = lane & 31, h = lane >> 5;
    constexpr int G = D / 128;  // groups of eight reduction steps
    float lsum = 0.f;
    bf16x8 nv[4];  // the next tile's swept code rows
    sc_load_code(Yc, 0, Y, nv, lane);
    for (int y0 = 0; y0 < Y; y0 += 32) {
        const bool yok = y0 + r < Y;
        const int yr = yok ? y0 + r : Y - 1;
        const __bf16 *yrow = Yd + (int64_t)yr * D + 8 * h;
        bf16x8 yf[2][8];  // swept DINO fragments: one group in the MFMAs, the next in flight
#pragma unroll
        for (int s = 0; s < 8; ++s) yf[0][s] = *(const bf16x8 *)(yrow + 16 * s);
        const float sr = swp_r && yok ? swp_r[y0 + r] : 0.f;
        __syncthreads();  // the previous tile's fragment reads are done
        sc_store_code(nv, L.y, L.yt, lane);
        if (y0 + 32 < Y) sc_load_code(Yc, y0 + 32, Y, nv, lane);
        f32x16 dt = sc_zero16(), st = sc_zero16();
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (g + 1 < G) {
#pragma unroll
                for (int s = 0; s < 8; ++s) yf[(g + 1) & 1][s] = *(const bf16x8 *)(yrow + 16 * (8 * (g + 1) + s));
            }
#pragma unroll
            for (int s = 0; s < 8; ++s)
                dt = SC_MFMA(sc_frag(L.own, SC_LA(D), r, 8 * g + s, h), yf[g & 1][s], dt);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 4; ++s) st = SC_MFMA(of[s], sc_frag(L.y, SC_LQ, r, s, h), st);
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int i = sc_row(x, h);
            const bool ok = yok && x0 + i < X;
            const float dd = ((dt[x] - own_r[x]) - sr) + cst;
            if (BWD) {
                L.gt[i * SC_LT + r] = (__bf16)(ok && st[x] > 0.f ? coef * dd : 0.f);
            } else {
                lsum += ok ? fmaxf(st[x], 0.f) * dd : 0.f;
            }
        }
        if (BWD) {
            __syncthreads();
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    dx[nt] = SC_MFMA(sc_frag(L.gt, SC_LT, r, s, h),
                                     sc_frag(L.yt, SC_LT, 32 * nt + r, s, h), dx[nt]);
        }
    }
    return lsum;
}

__device__ __forceinline__ void sc_owner_code(const __bf16 *Xc, int x0, int X, bf16x8 (&of)[4],
                                              int lane) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        of[s] = sc_zero8();
        if (x0 + r < X) of[s] = *(const bf16x8 *)(Xc + (int64_t)(x0 + r) * SC_CODE + 16 * s + 8 * h);
    }
}

__device__ __forceinline__ void sc_store_dx(const f32x16 (&dx)[2], float *out, int x0, int X, int lane) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int row = x0 + sc_row(x, h);
            if (row < X) out[(int64_t)row * SC_CODE + 32 * nt + r] = dx[nt][x];
        }
}

// the p-owned sweep over every pair: the forward's partial sums or the backward's da^
template <bool BWD, int D>
__device__ __forceinline__ void sc_p_sweep(const ScSweep &a, ScLds<D> &L, int64_t wg, int lane) {
    const int h = lane >> 5;
    const int64_t n = wg / a.tiles_p;
    const int x0 = (int)(wg - n * a.tiles_p) * 32;
    const int P = a.P;
    sc_stage_owner<D>(a.dino_a + n * P * D, x0, P, L.own, lane);
    bf16x8 of[4];
    sc_owner_code(a.code_a + n * P * SC_CODE, x0, P, of, lane);
    f32x16 dx[2];
    dx[0] = dx[1] = sc_zero16();
    for (int i = 0; i < a.n_pairs; ++i) {
        const int Q = a.Qi[i];
        float own_r[16];
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int row = x0 + sc_row(x, h);
            own_r[x] = a.rmean[i] && row < P ? a.rmean[i][n * P + row] : 0.f;
        }
        const float cst = (a.rmean[i] ? a.g[i] : 0.f) - a.shift[i];
        const float N = (float)((double)(a.nwg_p / a.tiles_p) * (double)P * (double)Q);
        const float coef = BWD ? (-a.weight[i] * a.up[i]) / N : 0.f;
        const float ls = sc_pair<BWD, D>(L, of, a.dino_b[i] + n * Q * D, a.code_b[i] + n * Q * SC_CODE,
                                         Q, x0, P, own_r, nullptr, cst, coef, dx, lane);
        if (!BWD) {
            const float t = sc_wave_sum(ls);
            if (lane == 0) a.part[i * a.nwg_p + wg] = t;
        }
    }
    if (BWD) sc_store_dx(dx, a.dhat_a + n * P * SC_CODE, x0, P, lane);
}

template <int D>
__global__ void __launch_bounds__(64) k_sc_fwd(const ScSweep a) {
    __shared__ __attribute__((aligned(16))) ScLds<D> L;
    sc_p_sweep<false, D>(a, L, blockIdx.x, threadIdx.x);
}

template <int D>
__global__ void __launch_bounds__(64) k_sc_bwd(const ScSweep a) {
    __shared__ __attribute__((aligned(16))) ScLds<D> L;
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (b < a.nwg_p) {
        sc_p_sweep<true, D>(a, L, b, lane);
        return;
    }
    // the q-owned sweep of pair i: owner = 32 partner rows, swept = the p rows
    int i = 0;
    while (i + 1 < a.n_pairs && b - a.nwg_p >= a.nq_start[i + 1]) ++i;
    const int Q = a.Qi[i], P = a.P;
    const int tiles_q = (Q + 31) / 32;
    const int64_t wq = b - a.nwg_p - a.nq_start[i];
    const int64_t n = wq / tiles_q;
    const int x0 = (int)(wq - n * tiles_q) * 32;
    sc_stage_owner<D>(a.dino_b[i] + n * Q * D, x0, Q, L.own, lane);
    bf16x8 of[4];
    sc_owner_code(a.code_b[i] + n * Q * SC_CODE, x0, Q, of, lane);
    f32x16 dx[2];
    dx[0] = dx[1] = sc_zero16();
    float own_r[16];
#pragma unroll
    for (int x = 0; x < 16; ++x) own_r[x] = 0.f;
    const float cst = (a.rmean[i] ? a.g[i] : 0.f) - a.shift[i];
    const float N = (float)((double)(a.nwg_p / a.tiles_p) * (double)P * (double)Q);
    const float coef = (-a.weight[i] * a.up[i]) / N;
    sc_pair<true, D>(L, of, a.dino_a + n * P * D, a.code_a + n * P * SC_CODE, P, x0, Q, own_r,
                     a.rmean[i] ? a.rmean[i] + n * P : nullptr, cst, coef, dx, lane);
    sc_store_dx(dx, a.dhat_b[i] + n * Q * SC_CODE, x0, Q, lane);
}

struct ScFinal {
    const float *part;
    float *loss;
    float scale[3];   // -w / N
    int64_t nwg_p;
    int32_t n_pairs;
};

// one workgroup: loss[i] = scale[i] * sum of the pair's partials in index order
__global__ void __launch_bounds__(256) k_sc_final(const ScFinal a) {
    __shared__ float red[256];
    for (int i = 0; i < 3; ++i) {
        float s = 0.f;
        if (i < a.n_pairs)
            for (int64_t k = threadIdx.x; k < a.nwg_p; k += 256) s += a.part[i * a.nwg_p + k];
        s = sc_block_sum(s, red);
        if (threadIdx.x == 0) a.loss[i] = i < a.n_pairs ? a.scale[i] * s : 0.f;
    }
}

struct ScFinJobs {
    const float *x[4];      // the un-normalised code rows
    const float *inv[4];
    const float *dh[4];     // dx^ sums
    const float *dh2[4];    // a second sum on the same rows (the self pair's q side) or null
    float *out[4];
    int64_t start[5];
    int32_t n;
};

// one wave per row, lane = column: dx = (dx^ - x^ (x^ . dx^)) / max(|x|, 1e-10)
__global__ void __launch_bounds__(256) k_sc_bwd_fin(const ScFinJobs J) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= J.start[J.n]) return;
    int s = 0;
    while (s + 1 < J.n && row >= J.start[s + 1]) ++s;
    const int64_t at = (row - J.start[s]) * SC_CODE + lane;
    float v = J.dh[s][at];
    if (J.dh2[s]) v += J.dh2[s][at];
    const float inv = J.inv[s][row - J.start[s]];
    const float xh = J.x[s][at] * inv;
    const float dot = sc_wave_sum(xh * v);
    J.out[s][at] = (v - xh * dot) * inv;
}

// ------------------------------------------------------------------------ C ABI
static bool sc_aligned(const void *p) { return ((uintptr_t)p & 15) == 0; }

static int sc_fail(const char *fn, const char *why) {
    static thread_local char buf[256];
    snprintf(buf, sizeof buf, "%s: invalid argument (%s)", fn, why);
    sd_set_error(buf);
    return -1;
}

static const char *sc_shape(int64_t nc, int P, int Q, int d, int n_pairs) {
    if (d != 384 && d != 768) return "d is 384 or 768";
    if (P < 1 || P > 4096 || Q < 1 || Q > 4096) return "1 <= P, Q <= 4096";
    if (n_pairs < 1 || n_pairs > 3) return "1 <= n_pairs <= 3";
    if (nc < 1 || nc * (P > Q ? P : Q) > SC_MAX_ROWS) return "nc >= 1, nc max(P, Q) <= 2^24";
    return nullptr;
}

static const char *sc_validate(const sd_stego_corr_args *a, bool bwd, bool *self) {
    if (!a) return "null args";
    if (a->code_dim != SC_CODE) return "code width is 64";
    if (const char *why = sc_shape(a->nc, a->P, a->Q, a->d, a->n_pairs)) return why;
    if (a->dino_dtype != SD_F32 && a->dino_dtype != SD_BF16) return "DINO rows are f32 or bf16";
    if (!a->dino_a || !a->stego_a || !a->work) return "dino_a, stego_a and work are required";
    if (!sc_aligned(a->dino_a) || !sc_aligned(a->stego_a) || !sc_aligned(a->work) ||
        !sc_aligned(a->loss) || !sc_aligned(a->up) || !sc_aligned(a->d_a))
        return "pointers are 16-byte aligned";
    int n_self = 0;
    for (int i = 0; i < a->n_pairs; ++i) {
        if ((a->dino_b[i] == nullptr) != (a->stego_b[i] == nullptr))
            return "a pair has both partner row sets, or neither (the self pair)";
        self[i] = a->dino_b[i] == nullptr;
        n_self += self[i];
        if (!sc_aligned(a->dino_b[i]) || !sc_aligned(a->stego_b[i]) || !sc_aligned(a->d_b[i]))
            return "pointers are 16-byte aligned";
        if (bwd && self[i] && a->d_b[i]) return "the self pair's gradient lands in d_a";
    }
    if (n_self > 1) return "at most one self pair";
    const ScLayout L = sc_layout(a->nc, a->P, a->Q, a->d, a->n_pairs, self);
    if (a->work_bytes < L.total) return "work_bytes is below sd_stego_corr_work";
    if (!bwd && !a->loss) return "loss is required";
    if (bwd && !a->up) return "up is required";
    return nullptr;
}

extern "C" int64_t sd_stego_corr_work(int64_t nc, int32_t P, int32_t Q, int32_t d, int32_t n_pairs,
                                      int32_t has_self) {
    if (const char *why = sc_shape(nc, P, Q, d, n_pairs)) {
        sc_fail("sd_stego_corr_work", why);
        return -1;
    }
    bool self[3] = {has_self != 0, false, false};
    return sc_layout(nc, P, Q, d, n_pairs, self).total;
}

static ScSweep sc_sweep_args(const sd_stego_corr_args *a, const ScLayout &L) {
    char *w = (char *)a->work;
    ScSweep s = {};
    s.dino_a = (const __bf16 *)(w + L.dino_a);
    s.code_a = (const __bf16 *)(w + L.code_a);
    s.g = (const float *)(w + L.g);
    s.up = a->up;
    s.part = (float *)(w + L.part);
    s.dhat_a = (float *)(w + L.dhat_a);
    int64_t at = 0;
    for (int i = 0; i < 3; ++i) {
        s.dino_b[i] = (const __bf16 *)(w + L.dino_b[i]);
        s.code_b[i] = (const __bf16 *)(w + L.code_b[i]);
        s.rmean[i] = a->pointwise ? (const float *)(w + L.rmean[i]) : nullptr;
        s.dhat_b[i] = (float *)(w + L.dhat_b[i]);
        s.weight[i] = a->weight[i];
        s.shift[i] = a->shift[i];
        s.Qi[i] = L.Qi[i];
        s.nq_start[i] = at;
        if (i < a->n_pairs) at += a->nc * ((L.Qi[i] + 31) / 32);
    }
    s.nq_start[3] = at;
    s.nwg_p = L.nwg_p;
    s.P = a->P;
    s.n_pairs = a->n_pairs;
    s.tiles_p = L.tiles_p;
    return s;
}

extern "C" int sd_stego_corr_fwd(const sd_stego_corr_args *a, void *stream) {
    bool self[3] = {false, false, false};
    if (const char *why = sc_validate(a, false, self)) return sc_fail("sd_stego_corr_fwd", why);
    const ScLayout L = sc_layout(a->nc, a->P, a->Q, a->d, a->n_pairs, self);
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)a->work;

    ScNormJobs J = {};
    int64_t rows = 0;
    auto job = [&](const void *src, int64_t off, int64_t inv_off, int64_t n, int width, bool f32) {
        J.src[J.n] = src;
        J.dst[J.n] = (__bf16 *)(w + off);
        J.inv[J.n] = inv_off >= 0 ? (float *)(w + inv_off) : nullptr;
        J.start[J.n] = rows;
        J.width[J.n] = width;
        J.f32[J.n] = f32;
        rows += n;
        J.start[++J.n] = rows;
    };
    const bool df32 = a->dino_dtype == SD_F32;
    job(a->dino_a, L.dino_a, -1, L.rows_a, a->d, df32);
    job(a->stego_a, L.code_a, L.inv_a, L.rows_a, SC_CODE, true);
    for (int i = 0; i < a->n_pairs; ++i)
        if (!self[i]) {
            job(a->dino_b[i], L.dino_b[i], -1, L.rows_b[i], a->d, df32);
            job(a->stego_b[i], L.code_b[i], L.inv_b[i], L.rows_b[i], SC_CODE, true);
        }
    hipLaunchKernelGGL(k_sc_norm, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, J);

    if (a->pointwise) {
        ScPoint p = {};
        p.dino_a = (const __bf16 *)(w + L.dino_a);
        p.g = (float *)(w + L.g);
        p.P = a->P;
        p.d = a->d;
        p.rows_a = L.rows_a;
        for (int i = 0; i < 3; ++i) {
            p.dino_b[i] = (const __bf16 *)(w + L.dino_b[i]);
            p.bbar[i] = (float *)(w + L.bbar[i]);
            p.rmean[i] = (float *)(w + L.rmean[i]);
            p.Qi[i] = L.Qi[i];
        }
        hipLaunchKernelGGL(k_sc_bbar, dim3((unsigned)a->nc, a->n_pairs), dim3(256), 0, st, p);
        hipLaunchKernelGGL(k_sc_rmean, dim3((unsigned)((L.rows_a + 3) / 4), a->n_pairs), dim3(256), 0,
                           st, p);
        hipLaunchKernelGGL(k_sc_g, dim3(a->n_pairs), dim3(256), 0, st, p);
    }

    const ScSweep s = sc_sweep_args(a, L);
    if (a->d == 384) hipLaunchKernelGGL(k_sc_fwd<384>, dim3((unsigned)L.nwg_p), dim3(64), 0, st, s);
    else hipLaunchKernelGGL(k_sc_fwd<768>, dim3((unsigned)L.nwg_p), dim3(64), 0, st, s);
    ScFinal f = {};
    f.part = s.part;
    f.loss = a->loss;
    f.nwg_p = L.nwg_p;
    f.n_pairs = a->n_pairs;
    for (int i = 0; i < a->n_pairs; ++i)
        f.scale[i] = -a->weight[i] / (float)((double)a->nc * (double)a->P * (double)L.Qi[i]);
    hipLaunchKernelGGL(k_sc_final, dim3(1), dim3(256), 0, st, f);
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_stego_corr_fwd: launch failed");
        return -2;
    }
    return 0;
}

extern "C" int sd_stego_corr_bwd(const sd_stego_corr_args *a, void *stream) {
    bool self[3] = {false, false, false};
    if (const char *why = sc_validate(a, true, self)) return sc_fail("sd_stego_corr_bwd", why);
    const ScLayout L = sc_layout(a->nc, a->P, a->Q, a->d, a->n_pairs, self);
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)a->work;
    const ScSweep s = sc_sweep_args(a, L);
    const int64_t nb = L.nwg_p + s.nq_start[3];
    if (nb > 0x7fffffffLL) return sc_fail("sd_stego_corr_bwd", "too many workgroups");
    if (a->d == 384) hipLaunchKernelGGL(k_sc_bwd<384>, dim3((unsigned)nb), dim3(64), 0, st, s);
    else hipLaunchKernelGGL(k_sc_bwd<768>, dim3((unsigned)nb), dim3(64), 0, st, s);

    ScFinJobs J = {};
    int64_t rows = 0;
    if (a->d_a) {
        J.x[0] = a->stego_a;
        J.inv[0] = (const float *)(w + L.inv_a);
        J.dh[0] = s.dhat_a;
        for (int i = 0; i < a->n_pairs; ++i)
            if (self[i]) J.dh2[0] = s.dhat_b[i];
        J.out[0] = a->d_a;
        J.start[0] = 0;
        rows = L.rows_a;
        J.start[++J.n] = rows;
    }
    for (int i = 0; i < a->n_pairs; ++i)
        if (!self[i] && a->d_b[i]) {
            J.x[J.n] = a->stego_b[i];
            J.inv[J.n] = (const float *)(w + L.inv_b[i]);
            J.dh[J.n] = s.dhat_b[i];
            J.out[J.n] = a->d_b[i];
            J.start[J.n] = rows;
            rows += L.rows_b[i];
            J.start[++J.n] = rows;
        }
    if (rows > 0)
        hipLaunchKernelGGL(k_sc_bwd_fin, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, J);
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_stego_corr_bwd: launch failed");
        return -2;
    }
    return 0;
}
