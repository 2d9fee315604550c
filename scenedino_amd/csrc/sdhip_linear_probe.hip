// sdhip_linear_probe.hip -- one pass of LinearHead (scenedino/downstream_head/semantic_head.py:
// 460-477) behind forward_training's _norm and Dropout2d, on gfx950 (CDNA4): logits, argmax,
// cross-entropy and the gradients of W and b, the only gradients there are (the rows are
// detached).
//
// Per row i of x (N, d), with optional column scales m (one row of m per rows_per_group rows):
//   xh_i = (normalize ? x_i / max(|x_i|, 1e-10) : x_i) o m      (normalised first, masked second)
//   z_i = W xh_i + b,  pred_i = argmax_k z_ik
//   valid rows (0 <= target_i < C):  l_i = logsumexp(z_i) - z_i[target_i],
//   g_i = softmax(z_i) - onehot(target_i),  gW = sum g_i xh_i^T,  gb = sum g_i
//
// sdhip_probe.hip's tile walk: a workgroup (4 waves) walks a contiguous range of 32-row tiles:
//   A  each wave reads 8 rows coalesced (4 rows of loads in flight), sums |x|^2 (butterfly, fixed
//      order) and leaves bf16(x o m) in an LDS tile with the row scale r_i = 1 / max(|x_i|, eps)
//      beside it: z_i = r_i (W bf16(x_i o m)) + b
//   B  logits on v_mfma_f32_32x32x16_bf16: W (hi + lo bf16 halves, rows padded to 32) is the A
//      operand, the tile's rows the B operand; the waves split the k-steps and wave 0 adds the
//      four partial tiles in wave order, then takes argmax, logsumexp and softmax - onehot per
//      row and leaves G (32 rows x 32 classes, zero on ignored rows) in LDS
//   C  gW += G^T Xh from the LDS tile, not from a re-read: every thread owns columns tid,
//      tid + 256, ... and keeps its (classes x columns) sums in registers, rows in order
// Each workgroup's loss, count, gW and gb go to `work` and k_lprobe_reduce adds them in
// workgroup order (16 chunks of workgroups, then the chunks): no atomics, a repeated launch
// gives the same bits.
#include "sdhip_common.h"

extern "C" void sd_set_error(const char *msg);

#define LP_MAXC 32
#define LP_MAXWG 512
#define LP_EPS 1e-10f
#define LP_GS 36  // floats per row of G in LDS (16-byte rows)
#define LP_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

typedef __attribute__((ext_vector_type(4))) float lp_f4;
typedef __attribute__((ext_vector_type(4))) __bf16 lp_h4;
typedef __attribute__((ext_vector_type(2))) float lp_f2;

struct lp_plan {
    int64_t ntiles, per;  // 32-row tiles, tiles per workgroup
    int nwg;
};

static __host__ __device__ inline lp_plan lp_make_plan(int64_t N) {
    lp_plan q;
    q.ntiles = (N + 31) / 32;
    q.per = (q.ntiles + LP_MAXWG - 1) / LP_MAXWG;
    q.nwg = (int)((q.ntiles + q.per - 1) / q.per);
    return q;
}

// floats of the W pack at the head of work: hi and lo bf16 halves, 32 rows of d
static __host__ __device__ inline int64_t lp_pack_floats(int d) { return (int64_t)LP_MAXC * d; }
// floats of one workgroup's partials: loss, count, gW, gb
static __host__ __device__ inline int64_t lp_part_floats(int d, int C) { return 2 + (int64_t)C * d + C; }

#define LP_PARTS_BYTES (3 * 64 * 16 * 4)
static inline int lp_lds_bytes(int d) {
    return 32 * LP_GS * 4 + LP_PARTS_BYTES + 32 * 4 + LP_MAXC * 4 + 32 * (d + 8) * 2;
}

__global__ void __launch_bounds__(256) k_lprobe_pack(const sd_linear_probe_args a) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= LP_MAXC * a.d) return;
    const int k = e / a.d;
    const float v = k < a.C ? a.W[e] : 0.f;
    __bf16 *hi = (__bf16 *)a.work, *lo = hi + LP_MAXC * a.d;
    const __bf16 h = (__bf16)v;
    hi[e] = h;
    lo[e] = (__bf16)(v - (float)h);
}

// X16: x is bf16.  CP: classes padded (the register sums of phase C), C <= CP.  NJ: f4 loads per
// lane and row in phase A and columns per thread in phase C, d <= 256 NJ.
template <bool X16, int CP, int NJ>
__global__ void __launch_bounds__(256) k_lprobe(const sd_linear_probe_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lp_lds[];
    const int d = a.d, C = a.C, ld = d + 8;
    float *G = (float *)lp_lds;                                        // 32 x LP_GS
    float *parts = G + 32 * LP_GS;                                     // 3 x 64 x 16
    float *rscale = parts + LP_PARTS_BYTES / 4;                        // 32
    float *bias = rscale + 32;                                         // 32
    __bf16 *tile = (__bf16 *)(bias + LP_MAXC);                         // 32 x (d + 8)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const lp_plan q = lp_make_plan(a.N);
    const int64_t t0 = (int64_t)blockIdx.x * q.per;
    const int64_t t1 = t0 + q.per < q.ntiles ? t0 + q.per : q.ntiles;
    const __bf16 *whi = (const __bf16 *)a.work, *wlo = whi + LP_MAXC * d;
    const bool has_t = a.target != nullptr, grad = a.gW != nullptr;

    lp_f2 gw[CP / 2][NJ];  // classes in pairs: one packed fma per pair and column
#pragma unroll
    for (int k = 0; k < CP / 2; ++k)
#pragma unroll
        for (int j = 0; j < NJ; ++j) gw[k][j] = lp_f2{0.f, 0.f};
    float gbs = 0.f, lsum = 0.f;
    int nval = 0;
    if (tid < LP_MAXC) bias[tid] = tid < C ? a.b[tid] : 0.f;
    for (int e = tid; e < 32 * LP_GS; e += 256) G[e] = 0.f;
    __syncthreads();

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t row0 = t * 32;
        // ---- A: rows 8 wave .. + 7 -> bf16(x o m) in the tile, 1 / |x| ----
#pragma unroll
        for (int rg = 0; rg < 2; ++rg) {
            lp_f4 v[4][NJ];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t row = row0 + 8 * wave + 4 * rg + u;
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int c4 = lane + 64 * j;
                    v[u][j] = lp_f4{0.f, 0.f, 0.f, 0.f};
                    if (row < a.N && c4 < d / 4) {
                        if (X16) {
                            const lp_h4 h = *(const lp_h4 *)((const __bf16 *)a.x + row * d + 4 * c4);
                            v[u][j] = lp_f4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
                        } else {
                            v[u][j] = *(const lp_f4 *)((const float *)a.x + row * d + 4 * c4);
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int lr = 8 * wave + 4 * rg + u;
                const int64_t row = row0 + lr;
                const bool ok = row < a.N;
                const float *mrow = (a.m && ok) ? a.m + (row / a.rows_per_group) * d : nullptr;
                float n2 = 0.f;
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int c4 = lane + 64 * j;
                    if (c4 < d / 4) {
                        lp_f4 w = v[u][j];
#pragma unroll
                        for (int i = 0; i < 4; ++i) n2 = fmaf(w[i], w[i], n2);
                        if (mrow) {
                            const lp_f4 mv = *(const lp_f4 *)(mrow + 4 * c4);
                            w = lp_f4{w[0] * mv[0], w[1] * mv[1], w[2] * mv[2], w[3] * mv[3]};
                        }
                        *(lp_h4 *)(tile + lr * ld + 4 * c4) =
                            lp_h4{(__bf16)w[0], (__bf16)w[1], (__bf16)w[2], (__bf16)w[3]};
                    }
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) n2 += __shfl_xor(n2, off);
                if (lane == 0)
                    rscale[lr] = !ok ? 0.f : a.normalize ? 1.f / fmaxf(sqrtf(n2), LP_EPS) : 1.f;
            }
        }
        __syncthreads();

        // ---- B: logits, k-steps split over the waves ----
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        for (int s = wave; s < d / 16; s += 4) {
            const bf16x8 b = *(const bf16x8 *)(tile + r * ld + 16 * s + 8 * hh);
            const bf16x8 ah = *(const bf16x8 *)(whi + r * d + 16 * s + 8 * hh);
            const bf16x8 al = *(const bf16x8 *)(wlo + r * d + 16 * s + 8 * hh);
            acc = LP_MFMA(ah, b, acc);
            acc = LP_MFMA(al, b, acc);
        }
        if (wave > 0) {
            float *dst = parts + ((wave - 1) * 64 + lane) * 16;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *(lp_f4 *)(dst + 4 * g) = lp_f4{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        }
        __syncthreads();
        if (wave == 0) {
            for (int w = 0; w < 3; ++w) {
                const float *src = parts + (w * 64 + lane) * 16;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const lp_f4 pv = *(const lp_f4 *)(src + 4 * g);
                    acc[4 * g] += pv[0]; acc[4 * g + 1] += pv[1];
                    acc[4 * g + 2] += pv[2]; acc[4 * g + 3] += pv[3];
                }
            }
            // register i of lane half hh: class (i & 3) + 8 (i >> 2) + 4 hh, increasing in i
            const float rs = rscale[r];
            const bool in = row0 + r < a.N;
            float z[16];
            float best = -INFINITY;
            int bk = LP_MAXC;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int k = (i & 3) + 8 * (i >> 2) + 4 * hh;
                z[i] = k < C ? fmaf(acc[i], rs, bias[k]) : -INFINITY;
                if (k < C && z[i] > best) {
                    best = z[i];
                    bk = k;
                }
            }
            const float ob = __shfl_xor(best, 32);
            const int ok2 = __shfl_xor(bk, 32);
            if (ob > best || (ob == best && ok2 < bk)) bk = ok2;
            if (bk >= C) bk = 0;  // a row of NaNs
            if (hh == 0 && in) a.pred[row0 + r] = bk;
            if (has_t) {
                const float mx = fmaxf(best, ob);
                float ex[16], se = 0.f, zt = 0.f;
                const int64_t tg = in ? a.target[row0 + r] : -1;
                const bool valid = tg >= 0 && tg < C;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int k = (i & 3) + 8 * (i >> 2) + 4 * hh;
                    ex[i] = k < C ? expf(z[i] - mx) : 0.f;
                    se += ex[i];
                    if (k == tg) zt = z[i];
                }
                se += __shfl_xor(se, 32);
                zt += __shfl_xor(zt, 32);  // one half holds the class, the other 0
                float l = valid ? (mx + logf(se)) - zt : 0.f;
                if (a.row_loss && hh == 0 && in) a.row_loss[row0 + r] = l;
                if (grad) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int k = (i & 3) + 8 * (i >> 2) + 4 * hh;
                        G[r * LP_GS + k] = valid ? ex[i] / se - (k == tg ? 1.f : 0.f) : 0.f;
                    }
                }
                // the 32 rows of the tile in a fixed order (both lane halves hold the same l)
#pragma unroll
                for (int off = 16; off >= 1; off >>= 1) l += __shfl_xor(l, off);
                lsum += l;
                nval += __popcll(__ballot(valid && hh == 0));
            }
        }
        __syncthreads();

        // ---- C: gW += G^T Xh from the tile, thread-owned columns, rows in order ----
        if (grad) {
#pragma unroll 2
            for (int lr = 0; lr < 32; ++lr) {
                const float rs = rscale[lr];
                float xv[NJ];
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int c = tid + 256 * j;
                    xv[j] = c < d ? (float)tile[lr * ld + c] * rs : 0.f;
                }
#pragma unroll
                for (int k4 = 0; k4 < CP / 4; ++k4) {
                    const lp_f4 g = *(const lp_f4 *)(G + lr * LP_GS + 4 * k4);
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < NJ; ++j)
                            gw[2 * k4 + i][j] = __builtin_elementwise_fma(
                                lp_f2{g[2 * i], g[2 * i + 1]}, lp_f2{xv[j], xv[j]}, gw[2 * k4 + i][j]);
                }
            }
            if (tid < C)
                for (int lr = 0; lr < 32; ++lr) gbs += G[lr * LP_GS + tid];
        }
        __syncthreads();
    }

    float *out = a.work + lp_pack_floats(d) + (int64_t)blockIdx.x * lp_part_floats(d, C);
    if (tid == 0) {
        out[0] = lsum;
        ((int *)out)[1] = nval;
    }
    if (grad) {
#pragma unroll
        for (int k = 0; k < CP; ++k)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int c = tid + 256 * j;
                if (k < C && c < d) out[2 + k * d + c] = gw[k >> 1][j][k & 1];
            }
        if (tid < C) out[2 + C * d + tid] = gbs;
    }
}

// the partials added in workgroup order: a 1024-thread block owns 64 output elements, wave c of
// its 16 adds the c-th sixteenth of the workgroups in order (64 consecutive floats per read) and
// the 16 sums are added in order
__global__ void __launch_bounds__(1024) k_lprobe_reduce(const sd_linear_probe_args a, const int nwg) {
    __shared__ float sums[16][64];
    const int el = threadIdx.x & 63, chunk = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + el;
    const int nW = a.C * a.d, nred = 2 + (a.gW ? nW + a.C : 0);
    const int64_t ps = lp_part_floats(a.d, a.C);
    const float *part = a.work + lp_pack_floats(a.d);
    const int per = (nwg + 15) / 16;
    const int g0 = chunk * per, g1 = g0 + per < nwg ? g0 + per : nwg;
    float s = 0.f;
    int n = 0;
    if (e == 1) {
        for (int g = g0; g < g1; ++g) n += ((const int *)part)[g * ps + 1];
        s = __int_as_float(n);
    } else if (e < nred) {
        for (int g = g0; g < g1; ++g) s += part[g * ps + e];
    }
    sums[chunk][el] = s;
    __syncthreads();
    if (chunk != 0 || e >= nred) return;
    if (e == 1) {
        n = 0;
        for (int c = 0; c < 16; ++c) n += __float_as_int(sums[c][el]);
        a.n_valid[0] = n;
        return;
    }
    s = 0.f;
    for (int c = 0; c < 16; ++c) s += sums[c][el];
    if (e == 0) a.loss_sum[0] = s;
    else if (e < 2 + nW) a.gW[e - 2] = s;
    else a.gb[e - 2 - nW] = s;
}

static bool lp_shape_ok(int64_t N, int32_t d, int32_t C) {
    return N >= 1 && N < ((int64_t)1 << 40) && d >= 64 && d <= 768 && d % 64 == 0 && C >= 1 &&
           C <= LP_MAXC;
}

extern "C" int64_t sd_linear_probe_work(int64_t N, int32_t d, int32_t C) {
    if (!lp_shape_ok(N, d, C)) {
        sd_set_error("sd_linear_probe_work: invalid argument (N >= 1, 64 <= d <= 768, "
                     "d % 64 == 0, 1 <= C <= 32)");
        return -1;
    }
    return lp_pack_floats(d) + (int64_t)lp_make_plan(N).nwg * lp_part_floats(d, C);
}

template <bool X16, int CP>
static void lp_launch(const sd_linear_probe_args &a, int nwg, int lds, hipStream_t s) {
    if (a.d <= 256) {
        sd_lds_attr((const void *)k_lprobe<X16, CP, 1>, lds);
        hipLaunchKernelGGL((k_lprobe<X16, CP, 1>), dim3(nwg), dim3(256), lds, s, a);
    } else {
        sd_lds_attr((const void *)k_lprobe<X16, CP, 3>, lds);
        hipLaunchKernelGGL((k_lprobe<X16, CP, 3>), dim3(nwg), dim3(256), lds, s, a);
    }
}

template <bool X16>
static void lp_launch_c(const sd_linear_probe_args &a, int nwg, int lds, hipStream_t s) {
    // the register sums of phase C are sized by the padded class count; without a gradient the
    // smallest variant serves every C
    if (!a.gW || a.C <= 8) lp_launch<X16, 8>(a, nwg, lds, s);
    else if (a.C <= 20) lp_launch<X16, 20>(a, nwg, lds, s);
    else lp_launch<X16, 32>(a, nwg, lds, s);
}

extern "C" int sd_linear_probe(const sd_linear_probe_args *a, void *stream) {
    bool ok = a && a->x && a->W && a->b && a->work && a->pred && lp_shape_ok(a->N, a->d, a->C) &&
              (a->x_dtype == SD_F32 || a->x_dtype == SD_BF16) && a->rows_per_group >= 1 &&
              !(a->m && (a->N - 1) / a->rows_per_group >= a->n_groups);
    if (ok) {
        if (a->target) ok = a->loss_sum && a->n_valid && (a->gW != nullptr) == (a->gb != nullptr);
        else ok = !a->loss_sum && !a->n_valid && !a->gW && !a->gb && !a->row_loss;
    }
    if (ok)
        ok = !(((uintptr_t)a->x | (uintptr_t)a->m | (uintptr_t)a->W | (uintptr_t)a->b |
                (uintptr_t)a->target | (uintptr_t)a->work | (uintptr_t)a->pred |
                (uintptr_t)a->loss_sum | (uintptr_t)a->n_valid | (uintptr_t)a->gW |
                (uintptr_t)a->gb | (uintptr_t)a->row_loss) & 15);
    if (!ok) {
        sd_set_error("sd_linear_probe: invalid argument (N >= 1, 64 <= d <= 768, d % 64 == 0, "
                     "1 <= C <= 32, x f32 or bf16, rows_per_group >= 1 with enough mask groups, "
                     "16-B aligned operands; target NULL: pred only, every other output NULL; "
                     "gW and gb need target and each other)");
        return -1;
    }
    const lp_plan q = lp_make_plan(a->N);
    const int lds = lp_lds_bytes(a->d);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_lprobe_pack, dim3((LP_MAXC * a->d + 255) / 256), dim3(256), 0, s, *a);
    if (a->x_dtype == SD_BF16) lp_launch_c<true>(*a, q.nwg, lds, s);
    else lp_launch_c<false>(*a, q.nwg, lds, s);
    if (a->target) {
        const int nred = 2 + (a->gW ? a->C * a->d + a->C : 0);
        hipLaunchKernelGGL(k_lprobe_reduce, dim3((nred + 63) / 64), dim3(1024), 0, s, *a, q.nwg);
    }
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_linear_probe: launch failed");
        return -2;
    }
    return 0;
}
