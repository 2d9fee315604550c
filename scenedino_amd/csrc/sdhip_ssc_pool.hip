// sdhip_ssc_pool.hip -- fine-to-coarse pooling of the supersampled SSCBench query
// (include/sdhip_ssc_pool.h; sscbench/evaluate_model_sscbench.py:727-745 with
// downsample_factor 2 / 4 / 8).
//
// One lane per coarse (y, z) voxel of one coarse x-plane.  For each of the f x f fine (x, y)
// rows under it the lane reads its f contiguous fine z values as one 8-byte (f = 2), one 16-byte
// (f = 4) or two 16-byte (f = 8) loads and its f labels as one 2 / 4 / 8-byte load; the fine
// index of a run is a multiple of f, so the run is naturally aligned, and neighbouring lanes read
// neighbouring runs.  The per-class vote sums live in LDS as [class][lane]: a lane touches its own
// column only (no barrier, no atomics; lanes of a wave hit consecutive words whatever their
// classes' rows, a multiple of 32 banks apart), and a runtime class id indexes LDS instead of a
// per-lane register array.  The
// children are added in ascending (a, b, c) order, which reproduces F.avg_pool3d's f32 sums bit
// for bit; a bandwidth kernel (5 bytes per fine voxel read, 5 / f^3 written).
#include "sdhip_common.h"

#include "../../include/sdhip_ssc_pool.h"

#include <math.h>

extern "C" void sd_set_error(const char *msg);

#define SP_BLOCK 256

__device__ __forceinline__ float sp_nanmax(float m, float v) { return (v > m || v != v) ? v : m; }

template <int F> struct sp_labels;
template <> struct sp_labels<2> { typedef uint16_t type; };
template <> struct sp_labels<4> { typedef uint32_t type; };
template <> struct sp_labels<8> { typedef uint64_t type; };

template <int F>
__device__ __forceinline__ void sp_load_run(const float *__restrict__ p, float (&v)[F]) {
    if constexpr (F == 2) {
        typedef __attribute__((ext_vector_type(2))) float f32x2;
        const f32x2 t = *(const f32x2 *)p;
        v[0] = t[0]; v[1] = t[1];
    } else {
#pragma unroll
        for (int q = 0; q < F / 4; ++q) {
            const f32x4 t = *(const f32x4 *)(p + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * q + e] = t[e];
        }
    }
}

template <int F>
__global__ void __launch_bounds__(SP_BLOCK)
k_ssc_pool(const float *__restrict__ sigma_f, const uint8_t *__restrict__ seg_f, int cx, int cy,
           int cz, int blocks_per_plane, float neg_vox, int n_classes,
           float *__restrict__ sigma_out, uint8_t *__restrict__ seg_out) {
    extern __shared__ float acc[];  // [n_classes][SP_BLOCK]
    const int tid = threadIdx.x;
    const int I = blockIdx.x / blocks_per_plane;
    const int q = (blockIdx.x - I * blocks_per_plane) * SP_BLOCK + tid;  // (J, K) of the plane
    if (q >= cy * cz) return;  // no barrier below: a lane owns its LDS column
    const int J = q / cz, K = q - J * cz;
    for (int c = 0; c < n_classes; ++c) acc[c * SP_BLOCK + tid] = 0.f;
    const int64_t fy = (int64_t)F * cy, fz = (int64_t)F * cz;
    float smax = -INFINITY;
    for (int a = 0; a < F; ++a)
        for (int b = 0; b < F; ++b) {
            const int64_t i = (((int64_t)F * I + a) * fy + ((int64_t)F * J + b)) * fz + (int64_t)F * K;
            float s[F];
            sp_load_run<F>(sigma_f + i, s);
            const uint64_t labs = *(const typename sp_labels<F>::type *)(seg_f + i);
#pragma unroll
            for (int c = 0; c < F; ++c) {
                smax = sp_nanmax(smax, s[c]);
                const float alpha = 1.0f - expf(neg_vox * s[c]);
                const int lab = (int)((labs >> (8 * c)) & 0xffu);
                if (lab < n_classes) acc[lab * SP_BLOCK + tid] += alpha;
            }
        }
    const float inv = (float)(F * F * F);
    float best = acc[tid] / inv;
    int bi = 0;
    for (int c = 1; c < n_classes; ++c) {  // torch.argmax: first maximum, NaN is the maximum
        const float v = acc[c * SP_BLOCK + tid] / inv;
        if (best == best && (v > best || v != v)) {
            best = v;
            bi = c;
        }
    }
    const int64_t o = ((int64_t)I * cy + J) * cz + K;
    sigma_out[o] = smax;
    seg_out[o] = (uint8_t)bi;
}

static bool sp_overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

extern "C" int sd_ssc_pool(const float *sigma_f, const uint8_t *seg_f, int64_t cx, int64_t cy,
                           int64_t cz, int32_t factor, float voxel_size, int32_t n_classes,
                           float *sigma_out, uint8_t *seg_out, void *stream) {
    const int64_t lim = (int64_t)1 << 31;
    if (!sigma_f || !seg_f || !sigma_out || !seg_out || (factor != 2 && factor != 4 && factor != 8) ||
        n_classes < 1 || n_classes > SD_SSC_POOL_MAX_CLASSES || cx <= 0 || cy <= 0 || cz <= 0 ||
        cx >= lim || cy >= lim || cz >= lim || !(voxel_size > 0.f) || !isfinite(voxel_size)) {
        sd_set_error("sd_ssc_pool: invalid argument (factor 2 / 4 / 8, 1 <= n_classes <= 32, "
                     "positive dims, voxel_size > 0)");
        return -1;
    }
    const int64_t f3 = (int64_t)factor * factor * factor;
    if (cx * cy >= lim || cx * cy * cz >= lim || cx * cy * cz * f3 >= lim) {
        sd_set_error("sd_ssc_pool: the fine grid must hold fewer than 2^31 voxels");
        return -1;
    }
    const int64_t nc = cx * cy * cz, nf = nc * f3;
    if (((uintptr_t)sigma_f | (uintptr_t)seg_f | (uintptr_t)sigma_out | (uintptr_t)seg_out) & 15) {
        sd_set_error("sd_ssc_pool: sigma_f / seg_f / sigma_out / seg_out must be 16-byte aligned");
        return -1;
    }
    if (sp_overlap(sigma_out, nc * 4, sigma_f, nf * 4) || sp_overlap(sigma_out, nc * 4, seg_f, nf) ||
        sp_overlap(seg_out, nc, sigma_f, nf * 4) || sp_overlap(seg_out, nc, seg_f, nf) ||
        sp_overlap(sigma_out, nc * 4, seg_out, nc)) {
        sd_set_error("sd_ssc_pool: sigma_out / seg_out must not overlap an input or each other");
        return -1;
    }
    const int bpp = (int)((cy * cz + SP_BLOCK - 1) / SP_BLOCK);
    const int64_t blocks = (int64_t)bpp * cx;  // <= cx cy cz < 2^31
    const dim3 grid((unsigned)blocks), block(SP_BLOCK);
    const size_t lds = (size_t)n_classes * SP_BLOCK * sizeof(float);  // <= 32 KiB
    const float neg_vox = -voxel_size;
    hipStream_t st = (hipStream_t)stream;
    if (factor == 2)
        hipLaunchKernelGGL(k_ssc_pool<2>, grid, block, lds, st, sigma_f, seg_f, (int)cx, (int)cy,
                           (int)cz, bpp, neg_vox, n_classes, sigma_out, seg_out);
    else if (factor == 4)
        hipLaunchKernelGGL(k_ssc_pool<4>, grid, block, lds, st, sigma_f, seg_f, (int)cx, (int)cy,
                           (int)cz, bpp, neg_vox, n_classes, sigma_out, seg_out);
    else
        hipLaunchKernelGGL(k_ssc_pool<8>, grid, block, lds, st, sigma_f, seg_f, (int)cx, (int)cy,
                           (int)cz, bpp, neg_vox, n_classes, sigma_out, seg_out);
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_ssc_pool: launch failed");
        return -2;
    }
    return 0;
}
