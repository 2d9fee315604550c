// sdhip_crop3d.hip -- the downstream stage's 3-D surface crops
// (BTSDownstreamWrapper.sample_3d_crop, scenedino/training/trainer_downstream.py:216-292).
//
// sd_crop3d_centres : per frame, the depth-quantile limits of view 0 (torch.quantile with linear
//                     interpolation over the depths below z_far), the bin counts, one drawn pixel
//                     per bin in torch.nonzero order, its back-projected centre and the sample
//                     points around it.  One workgroup per frame, no sort: a radix select on the
//                     order-preserving integer key of the f32 depths (8 bits per pass, four
//                     passes over the map) tracks every wanted rank at once; the 256-bin
//                     histograms live in LDS and hold integer counts, so the result does not
//                     depend on the order of the adds.
// sd_crop3d_compact : keeps the crops with more than n_samples occupied samples and, of each,
//                     the first n_samples occupied rows (wave ballots and popcount prefixes).
#include "sdhip_common.h"

extern "C" void sd_set_error(const char *msg);

#define C3_THREADS 1024                      // one workgroup per frame: 16 waves on one CU
#define C3_WAVES (C3_THREADS / SD_WAVE)
#define C3_MAX_CROPS 8
#define C3_MAX_T (2 * C3_MAX_CROPS)          // tracked ranks: min, max, floor / ceil per inner limit
#define C3_AHEAD 8                           // loads in flight per lane while walking the map

#define C3C_THREADS 256                      // sd_crop3d_compact: one workgroup per crop
#define C3C_WAVES (C3C_THREADS / SD_WAVE)
#define C3C_MAX_SAMPLES 4096
#define C3C_MAX_CROPS 64

// f32 -> u32 with the same order (negative values flipped whole, others in the sign bit)
__device__ __forceinline__ uint32_t c3_key(float d) {
    const uint32_t u = __float_as_uint(d);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float c3_unkey(uint32_t k) {
    return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ uint32_t c3_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, SD_WAVE);
    return v;
}
__device__ __forceinline__ uint64_t c3_lanes_below(int lane) { return (1ull << lane) - 1ull; }

// C3_AHEAD loads of one lane, 64 pixels apart, issued together: one wave walks its segment with
// a single load in flight otherwise, and a pass costs the L2 latency once per 64 pixels
__device__ __forceinline__ void c3_load(const float *__restrict__ d, int i, int end, float fill,
                                        float *__restrict__ v) {
#pragma unroll
    for (int u = 0; u < C3_AHEAD; ++u) v[u] = i + u * SD_WAVE < end ? d[i + u * SD_WAVE] : fill;
}

// i / n_crops as the f32 quantile, times (m - 1) in f32: the rank ATen's quantile interpolates at
__device__ __forceinline__ float c3_rank(int i, int n_crops, uint32_t m) {
    const float q = (float)((double)i / (double)n_crops);
    return __fmul_rn(q, (float)(m - 1u));
}

__global__ void __launch_bounds__(C3_THREADS) k_crop3d_centres(const sd_crop3d_args a, float xs,
                                                               float xe, float ys, float ye) {
    __shared__ uint32_t hist[C3_MAX_T * 256];
    __shared__ uint32_t t_prefix[C3_MAX_T], t_rank[C3_MAX_T], g_prefix[C3_MAX_T];
    __shared__ int t_group[C3_MAX_T];
    __shared__ int n_groups;
    __shared__ uint32_t m_sel;
    __shared__ float lim_s[C3_MAX_CROPS + 1];
    __shared__ uint32_t wcnt[C3_WAVES][C3_MAX_CROPS], woff[C3_WAVES][C3_MAX_CROPS];
    __shared__ uint32_t tot[C3_MAX_CROPS], rsel[C3_MAX_CROPS];
    __shared__ int pix[C3_MAX_CROPS];
    __shared__ float ctr[C3_MAX_CROPS][3];

    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & (SD_WAVE - 1), wave = tid / SD_WAVE;
    const int nc = a.n_crops, T = 2 * nc;
    const int N = a.h * a.w;
    const float *__restrict__ d = a.depth + (int64_t)f * a.depth_stride;
    const float z_far = a.z_far;
    // wave `wave` walks pixels [p0, p1) 64 at a time: row-major order is wave, step, lane
    const int seg = (((N + C3_WAVES - 1) / C3_WAVES) + SD_WAVE - 1) & ~(SD_WAVE - 1);
    const int p0 = min(N, wave * seg), p1 = min(N, p0 + seg);

    for (int i = tid; i < C3_MAX_T * 256; i += C3_THREADS) hist[i] = 0;
    if (tid < C3_MAX_T) {
        t_prefix[tid] = 0; t_rank[tid] = 0; t_group[tid] = 0; g_prefix[tid] = 0;
    }
    if (tid == 0) n_groups = 1;
    __syncthreads();

    // ---- radix select: after pass p every target knows the top 8 (p + 1) bits of its key ----
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        // the groups' prefixes in registers: a read of g_prefix per pixel and group would wait on
        // LDS behind every histogram add.  No key has the filler's prefix (at most 24 bits).
        uint32_t gp[C3_MAX_T];
#pragma unroll
        for (int g = 0; g < C3_MAX_T; ++g) gp[g] = g < n_groups ? g_prefix[g] : 0xffffffffu;
        const bool few = n_groups <= 4;  // the first two passes: a handful of exponents
        for (int i0 = p0; i0 < p1; i0 += SD_WAVE * C3_AHEAD) {
            float dvs[C3_AHEAD];
            c3_load(d, i0 + lane, p1, z_far, dvs);
#pragma unroll
            for (int u = 0; u < C3_AHEAD; ++u) {
                if (i0 + u * SD_WAVE >= p1) break;
                const float dv = dvs[u];
                int bin = -1;
                if (dv < z_far) {
                    const uint32_t key = c3_key(dv);
                    const uint32_t hi = pass ? key >> (shift + 8) : 0u;
                    int grp = -1;
#pragma unroll
                    for (int g = 0; g < 4; ++g) grp = gp[g] == hi ? g : grp;
                    if (!few) {
#pragma unroll
                        for (int g = 4; g < C3_MAX_T; ++g) grp = gp[g] == hi ? g : grp;
                    }
                    if (grp >= 0) bin = grp * 256 + (int)((key >> shift) & 255u);
                }
                // depths cluster in a few exponents: fold the wave's most common bins into one
                // add each before the remaining lanes add on their own
                bool todo = bin >= 0;
                for (int it = 0; it < 4; ++it) {
                    const uint64_t act = __ballot(todo);
                    if (!act) break;
                    const int lead = __ffsll((unsigned long long)act) - 1;
                    const int b0 = __shfl(bin, lead, SD_WAVE);
                    const uint64_t same = __ballot(todo && bin == b0);
                    if (lane == lead) atomicAdd(&hist[b0], (uint32_t)__popcll(same));
                    if (bin == b0) todo = false;
                    if (__popcll(same) < 16) break;  // spread digits: folding no longer pays
                }
                if (todo) atomicAdd(&hist[bin], 1u);
            }
        }
        __syncthreads();
        if (pass == 0) {  // the selection's size and the wanted ranks
            if (wave == 0) {
                uint32_t s = hist[4 * lane] + hist[4 * lane + 1] + hist[4 * lane + 2] +
                             hist[4 * lane + 3];
                s = c3_wave_sum(s);
                if (lane == 0) m_sel = s;
            }
            __syncthreads();
            const uint32_t m = m_sel;
            if (m == 0) break;
            if (tid < T) {
                uint32_t r;
                if (tid == 0) r = 0;
                else if (tid == 1) r = m - 1;
                else {
                    const float rk = c3_rank(tid >> 1, nc, m);
                    r = (uint32_t)((tid & 1) ? ceilf(rk) : floorf(rk));
                }
                t_rank[tid] = min(r, m - 1);
            }
            __syncthreads();
        }
        if (wave < T) {  // one wave per target: find its digit in its group's histogram
            const uint32_t *hg = hist + t_group[wave] * 256;
            const uint32_t k = t_rank[wave];
            const uint32_t h0 = hg[4 * lane], h1 = hg[4 * lane + 1], h2 = hg[4 * lane + 2],
                           h3 = hg[4 * lane + 3];
            const uint32_t s = h0 + h1 + h2 + h3;
            uint32_t incl = s;
#pragma unroll
            for (int o = 1; o < SD_WAVE; o <<= 1) {
                const uint32_t v = __shfl_up(incl, o, SD_WAVE);
                if (lane >= o) incl += v;
            }
            const uint32_t excl = incl - s;
            if (k >= excl && k < incl) {
                uint32_t c = excl;
                int j = 0;
                if (k >= c + h0) { c += h0; j = 1;
                    if (k >= c + h1) { c += h1; j = 2;
                        if (k >= c + h2) { c += h2; j = 3; } } }
                t_prefix[wave] = (t_prefix[wave] << 8) | (uint32_t)(4 * lane + j);
                t_rank[wave] = k - c;
            }
        }
        __syncthreads();
        if (pass < 3) {
            if (tid == 0) {  // targets with equal prefixes share a histogram
                int g_n = 0;
                for (int t = 0; t < T; ++t) {
                    int g = 0;
                    while (g < g_n && g_prefix[g] != t_prefix[t]) ++g;
                    if (g == g_n) g_prefix[g_n++] = t_prefix[t];
                    t_group[t] = g;
                }
                n_groups = g_n;
            }
            for (int i = tid; i < C3_MAX_T * 256; i += C3_THREADS) hist[i] = 0;
            __syncthreads();
        }
    }
    const uint32_t m = m_sel;

    // ---- limits ------------------------------------------------------------------------
    if (tid <= nc) {
        float l;
        if (m == 0) l = __uint_as_float(0x7fc00000u);  // nothing below z_far: no quantile
        else if (tid == 0) l = c3_unkey(t_prefix[0]);
        else if (tid == nc) l = c3_unkey(t_prefix[1]);
        else {
            const float lo = c3_unkey(t_prefix[2 * tid]), hi = c3_unkey(t_prefix[2 * tid + 1]);
            const float rk = c3_rank(tid, nc, m);
            const float wgt = __fsub_rn(rk, floorf(rk));
            const float diff = __fsub_rn(hi, lo);  // ATen's lerp, every step rounded on its own
            l = wgt < 0.5f ? __fadd_rn(lo, __fmul_rn(wgt, diff))
                           : __fsub_rn(hi, __fmul_rn(diff, __fsub_rn(1.0f, wgt)));
            l = fminf(fmaxf(l, lo), hi);
        }
        lim_s[tid] = l;
        a.limits[(int64_t)f * (nc + 1) + tid] = l;
    }
    __syncthreads();
    float lim[C3_MAX_CROPS + 1];
#pragma unroll
    for (int b = 0; b <= C3_MAX_CROPS; ++b) lim[b] = lim_s[min(b, nc)];

    // ---- bin counts per wave segment -----------------------------------------------------
    {
        uint32_t cnt[C3_MAX_CROPS];
#pragma unroll
        for (int b = 0; b < C3_MAX_CROPS; ++b) cnt[b] = 0;
        if (m != 0)
            for (int i0 = p0; i0 < p1; i0 += SD_WAVE * C3_AHEAD) {
                float dvs[C3_AHEAD];
                c3_load(d, i0 + lane, p1, nanf(""), dvs);  // NaN: in no bin
#pragma unroll
                for (int u = 0; u < C3_AHEAD; ++u)
#pragma unroll
                    for (int b = 0; b < C3_MAX_CROPS; ++b)
                        cnt[b] += (b < nc && dvs[u] > lim[b] && dvs[u] < lim[b + 1]) ? 1u : 0u;
            }
#pragma unroll
        for (int b = 0; b < C3_MAX_CROPS; ++b) {
            const uint32_t s = c3_wave_sum(cnt[b]);
            if (lane == 0) wcnt[wave][b] = s;
        }
    }
    __syncthreads();
    if (tid < nc) {
        uint32_t run = 0;
        for (int w = 0; w < C3_WAVES; ++w) { woff[w][tid] = run; run += wcnt[w][tid]; }
        tot[tid] = run;
        // torch.randint(count) from a uniform draw: f32 product, truncated, kept below count
        const float u = a.u_pick[(int64_t)f * nc + tid];
        const uint32_t r = (uint32_t)max(0, (int)__fmul_rn(u, (float)run));
        rsel[tid] = run ? min(r, run - 1) : 0u;
        pix[tid] = -1;
    }
    __syncthreads();

    // ---- locate the drawn pixel of each bin: only the waves whose segment holds one rescan ----
    {
        bool need = false;
        uint32_t run[C3_MAX_CROPS], want[C3_MAX_CROPS];
#pragma unroll
        for (int b = 0; b < C3_MAX_CROPS; ++b) {
            const bool live = b < nc && tot[min(b, nc - 1)] != 0;
            run[b] = live ? woff[wave][b] : 0u;
            want[b] = live ? rsel[b] : 0xffffffffu;
            need = need || (live && want[b] >= run[b] && want[b] < run[b] + wcnt[wave][b]);
        }
        if (need)
            for (int i0 = p0; i0 < p1; i0 += SD_WAVE * C3_AHEAD) {
                float dvs[C3_AHEAD];
                c3_load(d, i0 + lane, p1, nanf(""), dvs);
#pragma unroll
                for (int u = 0; u < C3_AHEAD; ++u) {
                    if (i0 + u * SD_WAVE >= p1) break;
                    const float dv = dvs[u];
#pragma unroll
                    for (int b = 0; b < C3_MAX_CROPS; ++b) {
                        const bool inb = b < nc && dv > lim[b] && dv < lim[b + 1];
                        const uint64_t mask = __ballot(inb);
                        const uint32_t at =
                            run[b] + (uint32_t)__popcll(mask & c3_lanes_below(lane));
                        if (inb && at == want[b]) pix[b] = i0 + u * SD_WAVE + lane;
                        run[b] += (uint32_t)__popcll(mask);
                    }
                }
            }
    }
    __syncthreads();

    // ---- centre = camera centre + unit ray * depth, product and sum rounded separately --------
    if (tid < nc) {
        const int p = pix[tid];
        const bool ok = tot[tid] != 0 && p >= 0;
        float c[3] = {0.0f, 0.0f, 0.0f};
        int row = -1, col = -1;
        if (ok) {
            row = p / a.w; col = p - row * a.w;
            float r[11];
            sd_ray_at(a.poses + (int64_t)f * a.pose_stride, a.projs + (int64_t)f * a.proj_stride,
                      (int64_t)col, (int64_t)row, (int64_t)a.w, (int64_t)a.h, xs, xe, ys, ye, 0.0f,
                      0.0f, 0.0f, r);
            const float dd = d[p];
#pragma unroll
            for (int j = 0; j < 3; ++j) c[j] = __fadd_rn(r[j], __fmul_rn(r[3 + j], dd));
        } else {
            tot[tid] = 0;
        }
        const int64_t o = (int64_t)f * nc + tid;
        a.count[o] = (int32_t)tot[tid];
        a.pixel[2 * o] = row; a.pixel[2 * o + 1] = col;
#pragma unroll
        for (int j = 0; j < 3; ++j) { ctr[tid][j] = c[j]; a.centre[3 * o + j] = c[j]; }
    }
    __syncthreads();
    const int per = a.S * 3, n_out = nc * per;
    const int64_t ob = (int64_t)f * n_out;
    for (int i = tid; i < n_out; i += C3_THREADS) {
        const int b = i / per, j = (i - b * per) % 3;
        a.points[ob + i] = tot[b] ? __fadd_rn(ctr[b][j], a.shift[ob + i]) : 0.0f;
    }
}

// One workgroup per crop.  Every workgroup counts the occupied samples of all C <= 64 crops
// itself (C S floats out of L2), so the cross-crop prefix is one wave ballot and nothing waits
// on another workgroup.  U: the copy unit of a code row (16 bytes, or 4 for odd row sizes).
template <typename U>
__global__ void __launch_bounds__(C3C_THREADS) k_crop3d_compact(const sd_crop3d_compact_args a,
                                                                int row_units) {
    __shared__ uint32_t nocc[C3C_MAX_CROPS];
    __shared__ uint32_t wcnt[C3C_WAVES];
    __shared__ int rowidx[C3C_MAX_SAMPLES];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & (SD_WAVE - 1), wave = tid / SD_WAVE;
    const int C = a.C, S = a.S, ns = a.n_samples;
    const float thr = a.thr;
    if (tid < C3C_MAX_CROPS) nocc[tid] = 0;
    __syncthreads();
    for (int cc = 0; cc < C; ++cc) {
        const float *sg = a.sigma + (int64_t)cc * S;
        uint32_t n = 0;
        for (int s = tid; s < S; s += C3C_THREADS) n += sg[s] > thr ? 1u : 0u;
        n = c3_wave_sum(n);
        if (lane == 0 && n) atomicAdd(&nocc[cc], n);
    }
    __syncthreads();
    const bool kept_l = lane < C && a.crop_ok[min(lane, C - 1)] > 0 && nocc[lane] > (uint32_t)ns;
    const uint64_t kept = __ballot(kept_l);
    const int n_valid = __popcll(kept);
    const bool mine = (kept >> c) & 1ull;
    const int slot = mine ? __popcll(kept & c3_lanes_below(c)) : -1;
    if (tid == 0) {
        a.slot[c] = slot;
        if (c == 0) a.n_valid[0] = n_valid;
    }
    U *__restrict__ out = (U *)a.codes_out;
    if (c >= n_valid) {  // output crop c stays empty
        const int64_t base = (int64_t)c * ns * row_units;
        U z;
        memset(&z, 0, sizeof(U));
        for (int i = tid; i < ns * row_units; i += C3C_THREADS) out[base + i] = z;
        for (int i = tid; i < ns; i += C3C_THREADS) a.occ_out[(int64_t)c * ns + i] = 0.0f;
    }
    if (!mine) return;

    // the first n_samples occupied rows of this crop, in order
    const float *sg = a.sigma + (int64_t)c * S;
    const int seg = (((S + C3C_WAVES - 1) / C3C_WAVES) + SD_WAVE - 1) & ~(SD_WAVE - 1);
    const int s0 = min(S, wave * seg), s1 = min(S, s0 + seg);
    {
        uint32_t n = 0;
        for (int s = s0 + lane; s < s1; s += SD_WAVE) n += sg[s] > thr ? 1u : 0u;
        n = c3_wave_sum(n);
        if (lane == 0) wcnt[wave] = n;
    }
    __syncthreads();
    uint32_t run = 0;
    for (int w = 0; w < wave; ++w) run += wcnt[w];
    for (int i0 = s0; i0 < s1 && run < (uint32_t)ns; i0 += SD_WAVE) {
        const int s = i0 + lane;
        const bool occ = s < s1 && sg[s] > thr;
        const uint64_t mask = __ballot(occ);
        const uint32_t at = run + (uint32_t)__popcll(mask & c3_lanes_below(lane));
        if (occ && at < (uint32_t)ns) rowidx[at] = s;
        run += (uint32_t)__popcll(mask);
    }
    __syncthreads();
    const U *__restrict__ in = (const U *)a.codes + (int64_t)c * S * row_units;
    const int64_t ob = (int64_t)slot * ns * row_units;
    for (int i = tid; i < ns * row_units; i += C3C_THREADS) {
        const int j = i / row_units, e = i - j * row_units;
        out[ob + i] = in[(int64_t)rowidx[j] * row_units + e];
    }
    for (int j = tid; j < ns; j += C3C_THREADS)
        a.occ_out[(int64_t)slot * ns + j] = __fsub_rn(1.0f, expf(-sg[rowidx[j]]));
}

extern "C" int sd_crop3d_centres(const sd_crop3d_args *a, void *stream) {
    if (!a || !a->depth || !a->poses || !a->projs || !a->u_pick || !a->shift || !a->limits ||
        !a->count || !a->pixel || !a->centre || !a->points || a->n < 1 || a->h < 1 || a->w < 1 ||
        a->n_crops < 1 || a->n_crops > C3_MAX_CROPS || a->S < 1 ||
        (int64_t)a->h * a->w > (1 << 24) || (int64_t)a->n_crops * a->S * 3 > 0x7fffffffLL ||
        a->depth_stride < (int64_t)a->h * a->w || a->pose_stride < 16 || a->proj_stride < 9) {
        sd_set_error("sd_crop3d_centres: invalid argument (n, S >= 1, 1 <= n_crops <= 8, "
                     "1 <= h w <= 2^24, frame strides covering one view, non-null operands)");
        return -1;
    }
    const double pw = 2.0 / (double)a->w, ph = 2.0 / (double)a->h;
    const float xs = (float)(-1.0 + 0.5 * pw), xe = (float)(1.0 - 0.5 * pw);
    const float ys = (float)(-1.0 + 0.5 * ph), ye = (float)(1.0 - 0.5 * ph);
    hipLaunchKernelGGL(k_crop3d_centres, dim3((unsigned)a->n), dim3(C3_THREADS), 0,
                       (hipStream_t)stream, *a, xs, xe, ys, ye);
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_crop3d_centres: launch failed");
        return -2;
    }
    return 0;
}

extern "C" int sd_crop3d_compact(const sd_crop3d_compact_args *a, void *stream) {
    const int esize = a && a->codes_dtype == SD_BF16 ? 2 : 4;
    if (!a || !a->sigma || !a->codes || !a->crop_ok || !a->codes_out || !a->occ_out ||
        !a->n_valid || !a->slot || a->C < 1 || a->C > C3C_MAX_CROPS || a->S < 1 || a->D < 1 ||
        a->n_samples < 1 || a->n_samples > C3C_MAX_SAMPLES ||
        (a->codes_dtype != SD_F32 && a->codes_dtype != SD_BF16) || ((a->D * esize) & 3) ||
        (int64_t)a->S * a->D * esize > 0x7fffffffLL ||
        (int64_t)a->n_samples * a->D * esize > 0x7fffffffLL ||
        (((uintptr_t)a->codes | (uintptr_t)a->codes_out) & 15)) {
        sd_set_error("sd_crop3d_compact: invalid argument (1 <= C <= 64, S, D >= 1, 1 <= n_samples "
                     "<= 4096, f32 or bf16 codes with rows of whole 4-byte words, 16-B aligned)");
        return -1;
    }
    const int row_bytes = a->D * esize;
    hipStream_t s = (hipStream_t)stream;
    if (row_bytes % 16 == 0)
        hipLaunchKernelGGL(k_crop3d_compact<uint4>, dim3((unsigned)a->C), dim3(C3C_THREADS), 0, s,
                           *a, row_bytes / 16);
    else
        hipLaunchKernelGGL(k_crop3d_compact<uint32_t>, dim3((unsigned)a->C), dim3(C3C_THREADS), 0,
                           s, *a, row_bytes / 4);
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_crop3d_compact: launch failed");
        return -2;
    }
    return 0;
}
