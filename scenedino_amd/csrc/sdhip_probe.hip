// sdhip_probe.hip -- one pass of KMeansParamHead._kmeans_cosine and its loss statistics
// (scenedino/downstream_head/semantic_head.py:361-373) on gfx950 (CDNA4).
//
// Per row i of x (N, d), with optional column scales m (the Dropout2d of forward_training,
// one row of m per rows_per_group rows) and row weights w:
//   xh_i = (x_i o m) / max(|x_i o m|, 1e-12),  s_ik = xh_i . c_k,  label_i = argmax_k s_ik
//   S_k = sum_{label_i = k} w_i xh_i,          counts_k = #{label_i = k}
// The labels are piecewise constant in the centres, so the reference's loss is
// -(1/N) sum_k c_k . S_k with S held constant: no backward kernel.
//
// A workgroup (4 waves) walks a contiguous range of 32-row tiles:
//   A  each wave reads 8 rows coalesced, scales them, sums |.|^2 (butterfly, fixed order) and
//      leaves bf16(x o m) in an LDS tile; argmax is invariant to the positive row scale
//   B  scores on v_mfma_f32_32x32x16_bf16: centres (hi + lo bf16 halves, rows padded to 32)
//      are the A operand, the tile's rows the B operand; the waves split the k-steps and
//      wave 0 adds the four partial tiles in wave order, then takes the argmax (lowest index
//      on ties)
//   C  every thread owns columns c = tid, tid + 256, ... of an LDS copy of S and adds the
//      tile's rows in row order from the f32 values (re-read, L2-resident): no atomics
// Each workgroup's S and counts go to `work` and k_probe_reduce adds them in workgroup order:
// a repeated launch gives the same bits.
#include "sdhip_common.h"

extern "C" void sd_set_error(const char *msg);

#define PB_MAXK 32
#define PB_MAXWG 512
#define PB_EPS 1e-12f
#define PB_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

typedef __attribute__((ext_vector_type(4))) float pb_f4;
typedef __attribute__((ext_vector_type(4))) __bf16 pb_h4;

struct pb_plan {
    int64_t ntiles, per;  // 32-row tiles, tiles per workgroup
    int nwg;
};

static __host__ __device__ inline pb_plan pb_make_plan(int64_t N) {
    pb_plan q;
    q.ntiles = (N + 31) / 32;
    q.per = (q.ntiles + PB_MAXWG - 1) / PB_MAXWG;
    q.nwg = (int)((q.ntiles + q.per - 1) / q.per);
    return q;
}

// floats of the centre pack at the head of work: hi and lo bf16 halves, 32 rows of d
static __host__ __device__ inline int64_t pb_pack_floats(int d) { return (int64_t)PB_MAXK * d; }

// LDS bytes of the score stage (tile of bf16 rows, later the waves' partial score tiles)
static __host__ __device__ inline int pb_stage_bytes(int d) {
    const int tile = 32 * (d + 8) * 2, parts = 3 * 64 * 16 * 4;
    return tile > parts ? tile : parts;
}

__global__ void __launch_bounds__(256) k_probe_pack(const sd_cluster_probe_args a) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= PB_MAXK * a.d) return;
    const int k = e / a.d;
    const float v = k < a.K ? a.centres[e] : 0.f;
    __bf16 *hi = (__bf16 *)a.work, *lo = hi + PB_MAXK * a.d;
    const __bf16 h = (__bf16)v;
    hi[e] = h;
    lo[e] = (__bf16)(v - (float)h);
}

template <bool X16>
__global__ void __launch_bounds__(256) k_probe(const sd_cluster_probe_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pb_lds[];
    const int d = a.d, K = a.K, ld = d + 8;
    float *S = (float *)pb_lds;                                   // K d
    __bf16 *tile = (__bf16 *)(pb_lds + (size_t)K * d * 4);        // 32 x (d + 8)
    float *parts = (float *)tile;                                 // 3 x 64 x 16, after the MFMAs
    float *rscale = (float *)((unsigned char *)tile + pb_stage_bytes(d));  // 32: w_i / |x_i o m|
    int *rlab = (int *)(rscale + 32);                             // 32
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const pb_plan q = pb_make_plan(a.N);
    const int64_t t0 = (int64_t)blockIdx.x * q.per;
    const int64_t t1 = t0 + q.per < q.ntiles ? t0 + q.per : q.ntiles;
    const __bf16 *chi = (const __bf16 *)a.work, *clo = chi + PB_MAXK * d;

    for (int e = tid; e < K * d; e += 256) S[e] = 0.f;
    int cnt = 0;
    __syncthreads();

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t row0 = t * 32;
        // ---- A: rows 8 wave .. + 7 -> bf16(x o m) in the tile, w / |x o m| ----
        for (int lr = 8 * wave; lr < 8 * wave + 8; ++lr) {
            const int64_t row = row0 + lr;
            const bool ok = row < a.N;
            const float *mrow = (a.m && ok) ? a.m + (row / a.rows_per_group) * d : nullptr;
            float n2 = 0.f;
            for (int c4 = lane; c4 < d / 4; c4 += 64) {
                pb_f4 v = {0.f, 0.f, 0.f, 0.f};
                if (ok) {
                    if (X16) {
                        const pb_h4 u = *(const pb_h4 *)((const __bf16 *)a.x + row * d + 4 * c4);
                        v = pb_f4{(float)u[0], (float)u[1], (float)u[2], (float)u[3]};
                    } else {
                        v = *(const pb_f4 *)((const float *)a.x + row * d + 4 * c4);
                    }
                    if (mrow) {
                        const pb_f4 mv = *(const pb_f4 *)(mrow + 4 * c4);
                        v = pb_f4{v[0] * mv[0], v[1] * mv[1], v[2] * mv[2], v[3] * mv[3]};
                    }
                }
                pb_h4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    n2 = fmaf(v[j], v[j], n2);
                    o[j] = (__bf16)v[j];
                }
                *(pb_h4 *)(tile + lr * ld + 4 * c4) = o;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) n2 += __shfl_xor(n2, off);
            if (lane == 0) {
                float sc = 0.f;
                if (ok) sc = (a.w ? a.w[row] : 1.f) / fmaxf(sqrtf(n2), PB_EPS);
                rscale[lr] = sc;
            }
        }
        __syncthreads();

        // ---- B: scores, k-steps split over the waves ----
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        for (int s = wave; s < d / 16; s += 4) {
            const bf16x8 b = *(const bf16x8 *)(tile + r * ld + 16 * s + 8 * hh);
            const bf16x8 ah = *(const bf16x8 *)(chi + r * d + 16 * s + 8 * hh);
            const bf16x8 al = *(const bf16x8 *)(clo + r * d + 16 * s + 8 * hh);
            acc = PB_MFMA(ah, b, acc);
            acc = PB_MFMA(al, b, acc);
        }
        __syncthreads();  // every wave is done with the tile: its space takes the partials
        if (wave > 0) {
            float *dst = parts + ((wave - 1) * 64 + lane) * 16;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *(pb_f4 *)(dst + 4 * g) = pb_f4{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        }
        __syncthreads();
        if (wave == 0) {
            for (int w = 0; w < 3; ++w) {
                const float *src = parts + (w * 64 + lane) * 16;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const pb_f4 v = *(const pb_f4 *)(src + 4 * g);
                    acc[4 * g] += v[0]; acc[4 * g + 1] += v[1];
                    acc[4 * g + 2] += v[2]; acc[4 * g + 3] += v[3];
                }
            }
            // register i of lane half hh: centre (i & 3) + 8 (i >> 2) + 4 hh, increasing in i
            float best = -INFINITY;
            int bk = PB_MAXK;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int k = (i & 3) + 8 * (i >> 2) + 4 * hh;
                if (k < K && acc[i] > best) {
                    best = acc[i];
                    bk = k;
                }
            }
            const float ob = __shfl_xor(best, 32);
            const int ok2 = __shfl_xor(bk, 32);
            if (ob > best || (ob == best && ok2 < bk)) bk = ok2;
            if (bk >= K) bk = 0;  // a row of NaNs
            if (hh == 0) {
                rlab[r] = bk;
                if (row0 + r < a.N) a.labels[row0 + r] = bk;
            }
        }
        __syncthreads();

        // ---- C: S[label] += w xh, thread-owned columns, rows in order ----
        const int nrow = a.N - row0 < 32 ? (int)(a.N - row0) : 32;
        for (int c = tid; c < d; c += 256) {
            for (int lr = 0; lr < nrow; ++lr) {
                const int64_t row = row0 + lr;
                float v = X16 ? (float)((const __bf16 *)a.x)[row * d + c] : ((const float *)a.x)[row * d + c];
                if (a.m) v *= a.m[(row / a.rows_per_group) * d + c];
                S[rlab[lr] * d + c] += v * rscale[lr];
            }
        }
        if (tid < K)
            for (int lr = 0; lr < nrow; ++lr) cnt += rlab[lr] == tid;
        __syncthreads();
    }

    float *out = a.work + pb_pack_floats(d) + (int64_t)blockIdx.x * ((int64_t)K * d + K);
    for (int e = tid; e < K * d; e += 256) out[e] = S[e];
    if (tid < K) ((int *)(out + (int64_t)K * d))[tid] = cnt;
}

// the partials added in workgroup order: one element of S (or of counts) per thread
__global__ void __launch_bounds__(256) k_probe_reduce(const sd_cluster_probe_args a, const int nwg) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int nS = a.K * a.d;
    const int64_t ps = (int64_t)nS + a.K;
    const float *part = a.work + pb_pack_floats(a.d);
    if (e < nS) {
        float s = 0.f;
        for (int g = 0; g < nwg; ++g) s += part[g * ps + e];
        a.S[e] = s;
    } else if (e < nS + a.K) {
        int s = 0;
        for (int g = 0; g < nwg; ++g) s += ((const int *)part)[g * ps + e];
        a.counts[e - nS] = s;
    }
}

static bool pb_shape_ok(int64_t N, int32_t d, int32_t K) {
    return N >= 1 && N < ((int64_t)1 << 40) && d >= 64 && d <= 768 && d % 64 == 0 && K >= 1 &&
           K <= PB_MAXK;
}

extern "C" int64_t sd_cluster_probe_work(int64_t N, int32_t d, int32_t K) {
    if (!pb_shape_ok(N, d, K)) {
        sd_set_error("sd_cluster_probe_work: invalid argument (N >= 1, 64 <= d <= 768, "
                     "d % 64 == 0, 1 <= K <= 32)");
        return -1;
    }
    return pb_pack_floats(d) + (int64_t)pb_make_plan(N).nwg * ((int64_t)K * d + K);
}

extern "C" int sd_cluster_probe(const sd_cluster_probe_args *a, void *stream) {
    const bool ptrs = a && a->x && a->centres && a->work && a->labels && a->S && a->counts;
    if (!ptrs || !pb_shape_ok(a->N, a->d, a->K) ||
        (a->x_dtype != SD_F32 && a->x_dtype != SD_BF16) || a->rows_per_group < 1 ||
        (a->m && (a->N - 1) / a->rows_per_group >= a->n_groups) ||
        (((uintptr_t)a->x | (uintptr_t)a->m | (uintptr_t)a->centres | (uintptr_t)a->w |
          (uintptr_t)a->work | (uintptr_t)a->labels | (uintptr_t)a->S | (uintptr_t)a->counts) & 15)) {
        sd_set_error("sd_cluster_probe: invalid argument (N >= 1, 64 <= d <= 768, d % 64 == 0, "
                     "1 <= K <= 32, x f32 or bf16, rows_per_group >= 1 with enough mask groups, "
                     "16-B aligned non-null operands)");
        return -1;
    }
    const pb_plan q = pb_make_plan(a->N);
    const int lds = a->K * a->d * 4 + pb_stage_bytes(a->d) + 32 * 4 + 32 * 4;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_probe_pack, dim3((PB_MAXK * a->d + 255) / 256), dim3(256), 0, s, *a);
    if (a->x_dtype == SD_BF16) {
        sd_lds_attr((const void *)k_probe<true>, lds);
        hipLaunchKernelGGL((k_probe<true>), dim3(q.nwg), dim3(256), lds, s, *a);
    } else {
        sd_lds_attr((const void *)k_probe<false>, lds);
        hipLaunchKernelGGL((k_probe<false>), dim3(q.nwg), dim3(256), lds, s, *a);
    }
    const int nred = a->K * a->d + a->K;
    hipLaunchKernelGGL(k_probe_reduce, dim3((nred + 255) / 256), dim3(256), 0, s, *a, q.nwg);
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_cluster_probe: launch failed");
        return -2;
    }
    return 0;
}
