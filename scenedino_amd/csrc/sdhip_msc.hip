// sdhip_msc.hip -- fused multi-scale-crop DINO targets (mode "upsample-gt").
//
// sd_msc_gt replaces MultiScaleCropGT_kornia.forward_chunk after the gt encoder
// (scenedino/models/backbones/dino/upsampler.py:81-130,170-181): the bilinear upsampling of every
// view's token grid to the image, the warp_perspective of the augmented views back onto the
// image, the nearest-mode validity warp, the NaN-masked nanmean over views and the channel L2
// normalisation.  Every output value is a fixed linear combination of at most 16 token cells per
// augmented view (2 x 2 pixel taps of the warp, each 2 x 2 token taps of the upsampling) and 4
// per base view, so nothing of image size is materialised but the output.
//
// One workgroup (4 waves) owns 64 consecutive pixels of one image row.  Tap indices and weights
// depend on the pixel only: every wave computes them once (separably: 4 column and 4 row entries
// per augmented view) and then walks its quarter of the channels; lane = pixel, so every store
// is one 256-byte row segment.  The channel norm sums the squares per wave, then the four
// partial sums in wave order through LDS; each wave then rescales the values it wrote itself (the
// same thread reads back its own stores).  Recomputing the values in a second sweep instead of
// reading them back was measured 5.6 x slower at the production shape.  No atomics,
// fixed summation order: a repeated launch gives the same bits.
#include "sdhip_common.h"

extern "C" void sd_set_error(const char *msg);

#define MSC_PX 64     // pixels per workgroup (one wave's lanes)
#define MSC_WAVES 4   // waves per workgroup, each a quarter of the channels

// F.interpolate(mode="bilinear", align_corners=False) taps of output index p on n input cells
// (ATen area_pixel_compute_source_index): cells i0, i1 with weights l0, l1.
__device__ __forceinline__ void msc_up(int p, float scale, int n, int &i0, int &i1, float &l0,
                                       float &l1) {
    const float s = fmaxf(((float)p + 0.5f) * scale - 0.5f, 0.f);
    const int c = min((int)s, n - 1);
    i0 = c;
    i1 = c + (c < n - 1 ? 1 : 0);
    l1 = s - (float)c;
    l0 = 1.f - l1;
}

// The four (token cell, weight) entries along one axis of the zero-padded bilinear sample at
// pixel coordinate x of an n_px-wide upsampled grid with n_tok cells: pixel taps floor(x) and
// floor(x) + 1 (weight 0 outside the image), each through msc_up.
__device__ __forceinline__ void msc_axis(float x, int n_px, float scale, int n_tok, int (&idx)[4],
                                         float (&w)[4]) {
    const float f = floorf(x);
    const float t1 = x - f, t0 = 1.f - t1;
    const int p0 = (int)f;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int p = p0 + t;
        const bool in = p >= 0 && p <= n_px - 1;
        float l0, l1;
        msc_up(min(max(p, 0), n_px - 1), scale, n_tok, idx[2 * t], idx[2 * t + 1], l0, l1);
        const float tw = t ? t1 : t0;
        w[2 * t] = in ? tw * l0 : 0.f;
        w[2 * t + 1] = in ? tw * l1 : 0.f;
    }
}

template <int NA>
struct MscTaps {
    // augmented views: token column / row offset (row * wp) and weight per axis entry
    int ax[NA > 0 ? NA : 1][4], ay[NA > 0 ? NA : 1][4];
    float awx[NA > 0 ? NA : 1][4], awy[NA > 0 ? NA : 1][4];
    // base views: the image (bx) and its flip (fx) share the rows
    int bx[2], fx[2], by[2];
    float bwx[2], fwx[2], bwy[2];
    float cnt;
};

template <int NA>
__device__ __forceinline__ float msc_value(const MscTaps<NA> &t, const float *__restrict__ g,
                                           int64_t view_stride) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const float *gk = g + k * view_stride;
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float q = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) q += t.awx[k][c] * gk[(uint32_t)(t.ay[k][r] + t.ax[k][c])];
            s += t.awy[k][r] * q;
        }
        acc += s;
    }
    {
        const float *gf = g + NA * view_stride;
        acc += t.bwy[0] * (t.fwx[0] * gf[(uint32_t)(t.by[0] + t.fx[0])] +
                           t.fwx[1] * gf[(uint32_t)(t.by[0] + t.fx[1])]) +
               t.bwy[1] * (t.fwx[0] * gf[(uint32_t)(t.by[1] + t.fx[0])] +
                           t.fwx[1] * gf[(uint32_t)(t.by[1] + t.fx[1])]);
        const float *gb = gf + view_stride;
        acc += t.bwy[0] * (t.bwx[0] * gb[(uint32_t)(t.by[0] + t.bx[0])] +
                           t.bwx[1] * gb[(uint32_t)(t.by[0] + t.bx[1])]) +
               t.bwy[1] * (t.bwx[0] * gb[(uint32_t)(t.by[1] + t.bx[0])] +
                           t.bwx[1] * gb[(uint32_t)(t.by[1] + t.bx[1])]);
    }
    return acc / t.cnt;
}

template <int NA, bool NORM>
__global__ __launch_bounds__(MSC_PX *MSC_WAVES) void k_msc_gt(sd_msc_gt_args a, int nbx) {
    __shared__ float s_ss[MSC_WAVES][MSC_PX];
    const int lane = threadIdx.x & (MSC_PX - 1), wave = threadIdx.x / MSC_PX;
    const int64_t blk = blockIdx.x;
    const int bxi = (int)(blk % nbx);
    const int64_t rest = blk / nbx;
    const int v = (int)(rest % a.H), b = (int)(rest / a.H);
    const int u_raw = bxi * MSC_PX + lane;
    const bool live = u_raw < a.W;
    const int u = live ? u_raw : a.W - 1;
    const int hp = a.hp, wp = a.wp, H = a.H, W = a.W, C = a.C;
    const float sx = (float)wp / (float)W, sy = (float)hp / (float)H;

    MscTaps<NA> t;
    {
        int i0, i1;
        msc_up(u, sx, wp, t.bx[0], t.bx[1], t.bwx[0], t.bwx[1]);
        msc_up(W - 1 - u, sx, wp, t.fx[0], t.fx[1], t.fwx[0], t.fwx[1]);
        msc_up(v, sy, hp, i0, i1, t.bwy[0], t.bwy[1]);
        t.by[0] = i0 * wp;
        t.by[1] = i1 * wp;
    }
    int nvalid = 0;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const float *T = a.T + ((int64_t)b * NA + k) * 9;
        const float fu = (float)u, fv = (float)v;
        const float p0 = (T[0] * fu + T[1] * fv) + T[2];
        const float p1 = (T[3] * fu + T[4] * fv) + T[5];
        const float p2 = (T[6] * fu + T[7] * fv) + T[8];
        const float x = p0 / p2, y = p1 / p2;
        const float rx = rintf(x), ry = rintf(y);
        // NaN compares false: invalid
        const bool valid = rx >= 0.f && rx <= (float)(W - 1) && ry >= 0.f && ry <= (float)(H - 1);
        // an invalid view is masked out whatever it sampled; keep its coordinates finite
        msc_axis(valid ? x : 0.f, W, sx, wp, t.ax[k], t.awx[k]);
        msc_axis(valid ? y : 0.f, H, sy, hp, t.ay[k], t.awy[k]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            t.ay[k][e] *= wp;
            if (!valid) t.awx[k][e] = 0.f;
        }
        nvalid += valid ? 1 : 0;
    }
    t.cnt = (float)(2 + nvalid);

    const int64_t hw = (int64_t)hp * wp, view_stride = (int64_t)C * hw;
    const int64_t HW = (int64_t)H * W;
    const float *feat = a.feat + (int64_t)b * (NA + 2) * view_stride;
    float *out = a.out + (int64_t)b * C * HW + (int64_t)v * W + u;
    const int cq = (C + MSC_WAVES - 1) / MSC_WAVES;
    const int c_lo = min(wave * cq, C), c_hi = min(c_lo + cq, C);

    float ss = 0.f;
#pragma unroll 2
    for (int c = c_lo; c < c_hi; ++c) {
        const float val = msc_value<NA>(t, feat + c * hw, view_stride);
        ss += val * val;
        if (live) out[c * HW] = val;
    }
    if (!NORM) return;
    s_ss[wave][lane] = ss;
    __syncthreads();
    const float n = sqrtf(((s_ss[0][lane] + s_ss[1][lane]) + s_ss[2][lane]) + s_ss[3][lane]);
    if (!live) return;
    for (int c = c_lo; c < c_hi; ++c) out[c * HW] = out[c * HW] / n;
}

template <int NA>
static void msc_launch(const sd_msc_gt_args &a, int nbx, unsigned nblk, hipStream_t s) {
    if (a.normalize)
        hipLaunchKernelGGL((k_msc_gt<NA, true>), dim3(nblk), dim3(MSC_PX * MSC_WAVES), 0, s, a, nbx);
    else
        hipLaunchKernelGGL((k_msc_gt<NA, false>), dim3(nblk), dim3(MSC_PX * MSC_WAVES), 0, s, a, nbx);
}

extern "C" int sd_msc_gt(const sd_msc_gt_args *a, void *stream) {
    if (!a || !a->feat || !a->out || a->B < 1 || a->V < 2 || a->V > 8 || a->C < 1 ||
        a->C > 1024 || a->hp < 1 || a->wp < 1 || a->H < 1 || a->W < 1 || (a->V > 2 && !a->T) ||
        (((uintptr_t)a->feat | (uintptr_t)a->out | (uintptr_t)a->T) & 15)) {
        sd_set_error("sd_msc_gt: invalid argument (B >= 1, 2 <= V <= 8, 1 <= C <= 1024, hp, wp, "
                     "H, W >= 1, 16-B aligned non-null operands)");
        return -1;
    }
    const int nbx = (a->W + MSC_PX - 1) / MSC_PX;
    const int64_t nblk = (int64_t)nbx * a->H * a->B;
    if ((int64_t)a->hp * a->wp > 0x7fffffffLL || nblk > 0x7fffffffLL) {
        sd_set_error("sd_msc_gt: token grid or image too large");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    switch (a->V - 2) {
    case 0: msc_launch<0>(*a, nbx, (unsigned)nblk, s); break;
    case 1: msc_launch<1>(*a, nbx, (unsigned)nblk, s); break;
    case 2: msc_launch<2>(*a, nbx, (unsigned)nblk, s); break;
    case 3: msc_launch<3>(*a, nbx, (unsigned)nblk, s); break;
    case 4: msc_launch<4>(*a, nbx, (unsigned)nblk, s); break;
    case 5: msc_launch<5>(*a, nbx, (unsigned)nblk, s); break;
    default: msc_launch<6>(*a, nbx, (unsigned)nblk, s); break;
    }
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_msc_gt: launch failed");
        return -2;
    }
    return 0;
}
