// scenedino_amd: backward kernels of the DPT decoder for gfx950 (the training path of
// models/backbones/dino/dpt_head.py).
//
// The data gradients of the decoder's convolutions reuse the forward GEMM (sd_gemm with
// rotated / transposed weight packs, models/backbones/dino/dpt_autograd.py); this unit holds
// what the forward has no counterpart for:
//   * sd_conv_wgrad: dW[Cout, taps Cin] = sum over output pixels p of dY[p, :]^T im2col(X)[p, :]
//     and db = sum_p dY[p, :], f32 accumulation on bf16 MFMA (v_mfma_f32_32x32x16_bf16);
//   * sd_upsample2x_bwd: the adjoint of sd_upsample2x, written as a gather;
//   * sd_relu_bwd: the pre-activation ReLU mask (and the residual unit's skip) on a gradient.
//
// sd_conv_wgrad.  Both operands have the reduction dimension (pixels) as their row dimension:
// dY rows are (pixel, Cout), im2col rows are (pixel, taps Cin).  A workgroup (4 waves) owns a
// TM x 128 output tile (TM = 64 or 128 rows of Cout) and a contiguous range of 32-pixel chunks
// (its "part").  A chunk's dY tile (32 x TM) and im2col tile (32 x 128) go through registers
// into LDS as they lie in memory (pixel-major rows), one chunk ahead of the one being
// multiplied, and the MFMA operands are read transposed (ds_read_b64_tr_b16), as k_wgrad /
// k_mlp_wgrad of sdhip_mlp.hip do.  LDS row strides are 64 or 192 B mod 256 (192 B for 64
// columns, 320 B for 128): the 4 rows x 64 B of a half-wave's transposed read then fall in 4
// disjoint 16-bank groups (sdhip_mlp.hip's note on k_mlp_wgrad's stage).
// The im2col loader follows the forward's rules (sdhip_vit.hip's conv A-tile loader): column
// k = tap Cin + ci, tap = 3 ky + kx, input pixel (oy stride + ky - 1, ox stride + kx - 1),
// out-of-image taps read as zero, the optional pre-activation ReLU applied as the tile is
// loaded.  Cin % 64 == 0, so a 16-byte granule never straddles a tap.
// Every part writes its f32 partial tile to the caller's workspace; k_cw_reduce sums the
// partials in part order into dW / db (no float atomics: bit-identical from launch to launch).
// db comes from the column-tile-0 workgroups, which sum their dY tile's columns in f32.
#include "sdhip_common.h"
#include "sdhip_point.h"
#include "sdhip_render.h"

#define CW_TN 128   // output columns (taps Cin) per workgroup
#define CW_CH 32    // pixels per chunk
#define CW_SB 160   // LDS row stride of the im2col tile (elements): 320 B
#define CW_WGS_PER_CU 2

typedef __attribute__((ext_vector_type(4))) short cw_s16x4;

__device__ __forceinline__ uint2 cw_tr(const void *lds_addr) {
    const cw_s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) cw_s16x4 *)(uintptr_t)lds_addr);
    return __builtin_bit_cast(uint2, v);
}

// relu on two packed bf16: a negative element (sign bit set) becomes +0
__device__ __forceinline__ uint32_t cw_relu2(uint32_t v) {
    if (v & 0x8000u) v &= 0xffff0000u;
    if (v & 0x80000000u) v &= 0x0000ffffu;
    return v;
}

struct cw_geom {
    int OH, OW, K, mt, nct, nrt;  // output size, taps Cin, row tiles of 32 per workgroup, tile counts
    int64_t M, nchunk;            // output pixels, chunks of 32
};

static __host__ __device__ inline cw_geom cw_geometry(const sd_conv_wgrad_args &g) {
    cw_geom q;
    q.OH = (g.H - 1) / g.stride + 1;
    q.OW = (g.W - 1) / g.stride + 1;
    q.K = g.taps * g.Cin;
    q.mt = g.Cout > 64 ? 4 : 2;
    q.nrt = (g.Cout + 32 * q.mt - 1) / (32 * q.mt);
    q.nct = (q.K + CW_TN - 1) / CW_TN;
    q.M = (int64_t)g.B * q.OH * q.OW;
    q.nchunk = (q.M + CW_CH - 1) / CW_CH;
    return q;
}

// MT: 32-row tiles of Cout per workgroup (2: 64 x 128, wave w owns row tile w & 1 and column
// tiles 2 (w >> 1) .. + 1; 4: 128 x 128, wave w owns row tile w and the four column tiles)
template <int MT>
__global__ void __launch_bounds__(256) k_conv_wgrad(const sd_conv_wgrad_args g) {
    typedef T16<SD_BF16> Tr;
    typedef typename Tr::Frag Frag;
    constexpr int TM = 32 * MT;
    constexpr int SA = MT == 4 ? 160 : 96;  // dY tile row stride (elements): 320 / 192 B
    constexpr int NTW = MT == 4 ? 4 : 2;    // column tiles per wave
    constexpr int GA = TM / 8;              // 16-byte granules per dY tile row
    constexpr int NLA = CW_CH * GA / 256;   // dY granules per thread (1 or 2)
    __shared__ __attribute__((aligned(16))) uint16_t sA[CW_CH * SA];
    __shared__ __attribute__((aligned(16))) uint16_t sB[CW_CH * CW_SB];
    const cw_geom q = cw_geometry(g);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rtile = blockIdx.y / q.nct, ctile = blockIdx.y - rtile * q.nct;
    const int co0 = rtile * TM, k0 = ctile * CW_TN;
    // this part's chunks [c_lo, c_hi)
    const int64_t per = (q.nchunk + g.nparts - 1) / g.nparts;
    const int64_t c_lo = (int64_t)blockIdx.x * per;
    const int64_t c_hi = c_lo + per < q.nchunk ? c_lo + per : q.nchunk;
    // zero the pad columns once (the loads never write them)
    for (int i = tid; i < CW_CH * SA / 8; i += 256) ((uint4 *)sA)[i] = uint4{0u, 0u, 0u, 0u};
    for (int i = tid; i < CW_CH * CW_SB / 8; i += 256) ((uint4 *)sB)[i] = uint4{0u, 0u, 0u, 0u};
    // per-thread granules.  dY: granule tid + 256 i -> row / GA, column 8 (% GA).  im2col:
    // granules tid, tid + 256 -> rows tid / 16 and 16 + tid / 16, column 8 (tid % 16): the
    // column's tap and channel are fixed per thread
    const int bcol = 8 * (tid & 15), brow = tid >> 4;
    const int kk = k0 + bcol;
    const bool bk_ok = kk < q.K;
    const int tap = kk / g.Cin, ci = kk - tap * g.Cin;
    const int pad = g.taps == 9 ? 1 : 0;
    const int ky = g.taps == 9 ? tap / 3 : 0, kx = g.taps == 9 ? tap - 3 * (tap / 3) : 0;
    const uint16_t *dy = (const uint16_t *)g.dy, *x = (const uint16_t *)g.x;
    uint4 ra[NLA], rb[2];
    auto gload = [&](int64_t c) {
        const int64_t p0 = c * CW_CH;
#pragma unroll
        for (int i = 0; i < NLA; ++i) {
            const int gi = tid + 256 * i, row = gi / GA, co = co0 + 8 * (gi - row * GA);
            const int64_t p = p0 + row;
            ra[i] = uint4{0u, 0u, 0u, 0u};
            if (p < q.M && co < g.Cout) ra[i] = *(const uint4 *)(dy + p * g.Cout + co);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int64_t p = p0 + brow + 16 * i;
            rb[i] = uint4{0u, 0u, 0u, 0u};
            if (p < q.M && bk_ok) {
                const uint32_t pu = (uint32_t)p, t = pu / (uint32_t)q.OW;  // M < 2^31
                const int ox = (int)(pu - t * (uint32_t)q.OW);
                const int b = (int)(t / (uint32_t)q.OH), oy = (int)(t - (uint32_t)b * (uint32_t)q.OH);
                const int iy = oy * g.stride + ky - pad, ix = ox * g.stride + kx - pad;
                if (iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) {
                    uint4 v = *(const uint4 *)(x + (((int64_t)b * g.H + iy) * g.W + ix) * g.Cin + ci);
                    if (g.relu_in) {
                        v.x = cw_relu2(v.x); v.y = cw_relu2(v.y);
                        v.z = cw_relu2(v.z); v.w = cw_relu2(v.w);
                    }
                    rb[i] = v;
                }
            }
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < NLA; ++i) {
            const int gi = tid + 256 * i, row = gi / GA, col = 8 * (gi - row * GA);
            *(uint4 *)(sA + row * SA + col) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) *(uint4 *)(sB + (brow + 16 * i) * CW_SB + bcol) = rb[i];
    };
    // transposed-read lane address (k_wgrad): group G = lane >> 4 (column base 16 (G & 1),
    // k base 8 (G >> 1)), lane 4 qq + pp of the group: row kb + qq, columns cbase .. + 3
    const int G = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
    const int kb = 8 * (G >> 1), cbase = 16 * (G & 1) + 4 * pp;
    const int rt = MT == 4 ? wave : (wave & 1);
    const int ct0 = MT == 4 ? 0 : 2 * (wave >> 1);
    f32x16 acc[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    const bool do_db = ctile == 0 && g.db != nullptr && tid < TM;
    float dbacc = 0.f;
    auto compute = [&]() {
#pragma unroll
        for (int s = 0; s < 2; ++s) {  // two k-steps of 16 pixels
            const uint16_t *pa = sA + (16 * s + kb + qq) * SA + 32 * rt + cbase;
            const uint2 a0 = cw_tr(pa), a1 = cw_tr(pa + 4 * SA);
            const Frag af = __builtin_bit_cast(Frag, uint4{a0.x, a0.y, a1.x, a1.y});
#pragma unroll
            for (int j = 0; j < NTW; ++j) {
                const uint16_t *pb = sB + (16 * s + kb + qq) * CW_SB + 32 * (ct0 + j) + cbase;
                const uint2 b0 = cw_tr(pb), b1 = cw_tr(pb + 4 * CW_SB);
                const Frag bf = __builtin_bit_cast(Frag, uint4{b0.x, b0.y, b1.x, b1.y});
                acc[j] = Tr::mma32(af, bf, acc[j]);
            }
        }
        if (do_db) {
#pragma unroll 8
            for (int r = 0; r < CW_CH; ++r)
                dbacc += __builtin_bit_cast(float, (uint32_t)sA[r * SA + tid] << 16);
        }
    };
    if (c_lo < c_hi) gload(c_lo);
    for (int64_t c = c_lo; c < c_hi; ++c) {
        __syncthreads();  // the previous chunk's LDS reads are done (first: the pads are zero)
        lstore();
        __syncthreads();
        if (c + 1 < c_hi) gload(c + 1);
        compute();
    }
    // partial tile: register e of acc[j] = C[32 rt + 8 (e >> 2) + 4 h + (e & 3)][32 (ct0 + j) + r]
    const int r = lane & 31, h = lane >> 5;
    float *out = g.work + (int64_t)blockIdx.x * g.Cout * (q.K + 1);
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
        const int col = k0 + 32 * (ct0 + j) + r;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int co = co0 + 32 * rt + 8 * (e >> 2) + 4 * h + (e & 3);
            if (co < g.Cout && col < q.K) out[(int64_t)co * q.K + col] = acc[j][e];
        }
    }
    if (do_db && co0 + tid < g.Cout) out[(int64_t)g.Cout * q.K + co0 + tid] = dbacc;
}

// the partials summed in part order: one float4 of dW (or one element of db) per thread
__global__ void __launch_bounds__(256) k_cw_reduce(const sd_conv_wgrad_args g) {
    const int64_t nw = (int64_t)g.Cout * g.taps * g.Cin;  // % 4 == 0
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t ps = nw + g.Cout;  // floats per part
    if (e < nw / 4) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int p = 0; p < g.nparts; ++p) {
            const float4 v = *(const float4 *)(g.work + p * ps + 4 * e);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        ((float4 *)g.dw)[e] = s;
    } else if (g.db && e - nw / 4 < g.Cout) {
        const int64_t co = e - nw / 4;
        float s = 0.f;
        for (int p = 0; p < g.nparts; ++p) s += g.work[p * ps + nw + co];
        g.db[co] = s;
    }
}

static bool cw_shape_ok(const sd_conv_wgrad_args *g) {
    return g && g->B > 0 && g->H > 0 && g->W > 0 && g->Cin > 0 && g->Cin % 64 == 0 &&
           g->Cout > 0 && g->Cout % 8 == 0 && (g->taps == 1 || g->taps == 9) &&
           (g->stride == 1 || g->stride == 2) && g->nparts >= 0 &&
           (int64_t)g->B * g->H * g->W * g->Cin < ((int64_t)1 << 31) &&
           (int64_t)g->B * g->H * g->W * g->Cout < ((int64_t)1 << 31) &&
           (int64_t)g->Cout * g->taps * g->Cin < ((int64_t)1 << 28);
}

// parts for a shape: CW_WGS_PER_CU workgroups per CU over the output tiles, at most one part
// per chunk, no empty part
static int cw_auto_parts(const sd_conv_wgrad_args &g) {
    const cw_geom q = cw_geometry(g);
    const int64_t tiles = (int64_t)q.nrt * q.nct;
    int64_t want = ((int64_t)CW_WGS_PER_CU * sd_num_cus() + tiles - 1) / tiles;
    if (want > q.nchunk) want = q.nchunk;
    if (want < 1) want = 1;
    const int64_t per = (q.nchunk + want - 1) / want;
    return (int)((q.nchunk + per - 1) / per);
}

extern "C" int32_t sd_conv_wgrad_parts(const sd_conv_wgrad_args *g) {
    if (!cw_shape_ok(g)) {
        sd_set_error("sd_conv_wgrad_parts: invalid argument (taps 1 or 9, stride 1 or 2, "
                     "Cin % 64 == 0, Cout % 8 == 0)");
        return -1;
    }
    return cw_auto_parts(*g);
}

extern "C" int64_t sd_conv_wgrad_work(const sd_conv_wgrad_args *g) {
    if (!cw_shape_ok(g)) {
        sd_set_error("sd_conv_wgrad_work: invalid argument (taps 1 or 9, stride 1 or 2, "
                     "Cin % 64 == 0, Cout % 8 == 0)");
        return -1;
    }
    const int np = g->nparts > 0 ? g->nparts : cw_auto_parts(*g);
    return (int64_t)np * g->Cout * ((int64_t)g->taps * g->Cin + 1);
}

extern "C" int sd_conv_wgrad(const sd_conv_wgrad_args *g, void *stream) {
    if (!cw_shape_ok(g) || !g->x || !g->dy || !g->work || !g->dw || g->nparts <= 0 ||
        ((uintptr_t)g->x | (uintptr_t)g->dy | (uintptr_t)g->work | (uintptr_t)g->dw) % 16 != 0) {
        sd_set_error("sd_conv_wgrad: invalid argument (taps 1 or 9, stride 1 or 2, "
                     "Cin % 64 == 0, Cout % 8 == 0, 16-byte aligned operands, nparts from "
                     "sd_conv_wgrad_parts)");
        return -1;
    }
    const cw_geom q = cw_geometry(*g);
    if (g->nparts > q.nchunk) {
        sd_set_error("sd_conv_wgrad: more parts than 32-pixel chunks");
        return -1;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)g->nparts, (unsigned)(q.nrt * q.nct));
    if (q.mt == 4)
        hipLaunchKernelGGL(k_conv_wgrad<4>, grid, dim3(256), 0, st, *g);
    else
        hipLaunchKernelGGL(k_conv_wgrad<2>, grid, dim3(256), 0, st, *g);
    const int64_t nred = (int64_t)g->Cout * q.K / 4 + g->Cout;
    hipLaunchKernelGGL(k_cw_reduce, dim3((unsigned)((nred + 255) / 256)), dim3(256), 0, st, *g);
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_conv_wgrad: launch failed");
        return -2;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// Adjoint of k_upsample2x (align_corners=True bilinear x2) as a gather: one thread per (input
// pixel, 8 channels) sums its contributing output pixels in a fixed order.  The per-axis
// weights are recomputed with the forward's own f32 expressions (the products of the two axes'
// weights are formed here, the forward nests them: the transpose of its interpolation matrix
// up to f32 rounding).  An input row iy receives from output rows
// oy with floor(sh oy) in {iy - 1, iy}; with 1 / sh = 2 + 1 / (H - 1) those lie in
// [2 iy - 3, 2 iy + 4].
// ---------------------------------------------------------------------------
__device__ __forceinline__ void ub_axis(int i, int n, int on, float w[8], int &o0) {
    const float sc = on > 1 ? (float)(n - 1) / (float)(on - 1) : 0.f;
    o0 = 2 * i - 3;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int o = o0 + j;
        float wt = 0.f;
        if (o >= 0 && o < on) {
            const float f = sc * (float)o;
            const int i0 = (int)f;
            const int ip = i0 < n - 1 ? 1 : 0;
            const float l = f - (float)i0;
            if (i0 == i) wt += 1.f - l;
            if (i0 + ip == i) wt += l;  // ip == 0 (last row): the forward reads row i0 twice
        }
        w[j] = wt;
    }
}

__global__ void __launch_bounds__(256) k_upsample2x_bwd(const __bf16 *__restrict__ go, int B, int H,
                                                        int W, int C, __bf16 *__restrict__ gi) {
    const int OH = 2 * H, OW = 2 * W, C8 = C / 8;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)B * H * W * C8) return;
    const int c8 = (int)(gid % C8);
    const int64_t pix = gid / C8;
    const int ix = (int)(pix % W);
    const int64_t t = pix / W;
    const int iy = (int)(t % H), b = (int)(t / H);
    float wy[8], wx[8];
    int oy0, ox0;
    ub_axis(iy, H, OH, wy, oy0);
    ub_axis(ix, W, OW, wx, ox0);
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = 0.f;
    const __bf16 *base = go + (int64_t)b * OH * OW * C + c8 * 8;
#pragma unroll
    for (int jy = 0; jy < 8; ++jy) {
        if (wy[jy] == 0.f) continue;
#pragma unroll
        for (int jx = 0; jx < 8; ++jx) {
            if (wx[jx] == 0.f) continue;
            const float wgt = wy[jy] * wx[jx];
            const bf16x8 v = *(const bf16x8 *)(base + ((int64_t)(oy0 + jy) * OW + ox0 + jx) * C);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += wgt * (float)v[j];
        }
    }
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (__bf16)s[j];
    *(bf16x8 *)(gi + pix * C + c8 * 8) = o;
}

extern "C" int sd_upsample2x_bwd(const void *gout, int32_t B, int32_t H, int32_t W, int32_t C,
                                 void *gin, void *stream) {
    if (!gout || !gin || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 ||
        ((uintptr_t)gout | (uintptr_t)gin) % 16 != 0) {
        sd_set_error("sd_upsample2x_bwd: invalid argument (C % 8 == 0, 16-byte aligned)");
        return -1;
    }
    const int64_t n = (int64_t)B * H * W * (C / 8);
    hipLaunchKernelGGL(k_upsample2x_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, (const __bf16 *)gout, B, H, W, C, (__bf16 *)gin);
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_upsample2x_bwd: launch failed");
        return -2;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// out = (x > 0 ? g : 0) (+ res) on bf16, 8 elements (16 bytes) per thread: the gradient through
// a pre-activation ReLU, optionally with the residual unit's skip gradient added (f32 sum, one
// rounding).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_relu_bwd(const bf16x8 *__restrict__ x,
                                                  const bf16x8 *__restrict__ g,
                                                  const bf16x8 *__restrict__ res, int64_t n8,
                                                  bf16x8 *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const bf16x8 xv = x[i], gv = g[i];
    bf16x8 o;
    if (res) {
        const bf16x8 rv = res[i];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            o[j] = (__bf16)(((float)xv[j] > 0.f ? (float)gv[j] : 0.f) + (float)rv[j]);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (float)xv[j] > 0.f ? gv[j] : (__bf16)0.f;
    }
    out[i] = o;
}

extern "C" int sd_relu_bwd(const void *x, const void *g, const void *res, int64_t n, void *out,
                           void *stream) {
    if (!x || !g || !out || n < 0 || n % 8 ||
        ((uintptr_t)x | (uintptr_t)g | (uintptr_t)res | (uintptr_t)out) % 16 != 0) {
        sd_set_error("sd_relu_bwd: invalid argument (n % 8 == 0, 16-byte aligned)");
        return -1;
    }
    if (n == 0) return 0;
    const int64_t n8 = n / 8;
    hipLaunchKernelGGL(k_relu_bwd, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, (const bf16x8 *)x, (const bf16x8 *)g,
                       (const bf16x8 *)res, n8, (bf16x8 *)out);
    if (hipGetLastError() != hipSuccess) {
        sd_set_error("sd_relu_bwd: launch failed");
        return -2;
    }
    return 0;
}
