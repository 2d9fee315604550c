// sdhip_tile.hip -- LDS-staged projected-grid render (gfx950 / CDNA4, 16-bit modes).
//
// Same computation as k_render_proj (sdhip_proj.hip: NeRFRenderer.composite over
// BTSNet.forward, nerf.py:230-449 / bts.py:271-595, on the projected grid
// P = W_in[:, :C] G + b_in), organised so that the bilinear P taps come from LDS instead
// of the vector-memory path.  Per sample the taps are 4 x 256 B; through global loads
// every byte passes the CU's texture path (~64 B/clk), which bounds k_render_proj.  Rays
// of neighbouring pixels sample neighbouring texels, so one workgroup renders a GROUP of
// 8 consecutive rays at a time (one per wave) and stages the bounding box of all their
// taps, read once from L2 by LDS-DMA, in LDS.
//
// Workgroup = 8 waves, one workgroup per CU.  Step n: wave w renders ray 8 G_n + w.
//   item 0    ray pass of the wave's NEXT ray (geometry, taps, colours -> LDS records,
//             tap bounding box -> LDS), the DINO head of the previous group (below),
//             then item 0 of the current ray
//   barrier X union of the next group's boxes; if it fits the tile buffer, the waves
//             issue the LDS-DMA of those P texels, row by row of the box (else the group
//             goes to the overflow list and the fallback kernel renders it)
//   items 1.. of the current ray (taps from the current tile buffer), ray epilogue:
//             depth / colour stored, the composited hidden sum_k w_k relu(h_k) -> LDS
//   vmcnt(0), barrier Y
// Blend as MFMA: hidden[h][j] = sum_{tap q, sample s} P_q(s)[h] * Wb[(s, q)][j] with the
// block-diagonal bilinear weights Wb[(s, q)][j] = w_q(j) [s == j]; A (P taps) is read with
// ds_read_b64_tr_b16 (lane 4q + p of a 16-lane group addresses tap q of the group's
// sample, columns 4p..4p+3; lane i receives hidden 16 t + i of the 4 taps).  Per 16-sample
// item: 2 K-chunks of 8 samples x 8 hidden tiles = 16 MFMA 16x16x32, no blend VALU.
// Then as k_render_proj: + W_code . code (16 MFMA), ReLU, sigma (4 MFMA), softplus,
// alpha, DPP transmittance scan, and hidden-space compositing (v_pk_fma_f16 of the packed
// hidden pairs into packed f16 per-lane partial sums).  The output layer is linear, so
//   dino = sum_k w_k (W h_k + b) = W (sum_k w_k h_k) + b sum_k w_k          (nerf.py:394)
// and is applied per GROUP: hsum of the 8 rays as the B operand (8 of 16 columns),
// D / 16 MFMA tiles spread over the waves.
#include "sdhip_render.h"

constexpr int ST_NW = 8;    // NW: waves per workgroup (2 per SIMD) = rays per group at one ray per wave
#define ST_TEX 288          // LDS bytes per staged texel: 256 B of P + 32 B pad
#define ST_TEXQ 18          // 16-byte chunks per staged texel
#define ST_MAXP 2           // K <= 128 (two samples per lane in the ray pass)
#define ST_BOX_EPS (1.f / 1024.f)  // late order's box pass: texel-border margin of a part endpoint
#define ST_MAXKW 8          // DMA columns (1-KiB pieces of a box row) per wave: rows <= 8 x 8 x 64 / 18 texels

// diagnostic build only (ST_PROF=1): per-phase s_memtime cycles summed over all waves
// (tools/tile_prof.py); the outputs are unchanged
#ifndef ST_PROF
#define ST_PROF 0
#endif
#if ST_PROF
__device__ unsigned long long st_prof[32];
#define ST_T(i)                                                  \
    {                                                            \
        const uint64_t _t = __builtin_amdgcn_s_memtime();        \
        pacc[i] += (uint32_t)(_t - tlast);                       \
        tlast = _t;                                              \
    }
extern "C" int sd_tile_prof(unsigned long long *out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(st_prof), sizeof(st_prof)) != hipSuccess) return -2;
    if (reset) {
        unsigned long long z[32] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(st_prof), z, sizeof(z)) != hipSuccess) return -2;
    }
    return 0;
}
#elif defined(ST_MARK) && ST_MARK
#define ST_T(i) asm volatile(";@T " #i)
#else
#define ST_T(i)
#endif
// diagnostic build only (ST_MARK=1): asm comments at the item-loop phase boundaries (20..28)
// and inside the per-step phases (30 / 39: the step loop's first and last statement, 40..44
// late ray pass, 50..53 stage, 60..62 ray sums), for the static instruction-category count of
// tools/tile_isa_count.py (no code of their own; the scheduler may still move arithmetic
// across them, so the split is approximate)
#ifndef ST_MARK
#define ST_MARK 0
#endif
#if ST_MARK
#define ST_M(i) asm volatile(";@M " #i)
// a marker pinned after the value x is computed (and before its later uses)
#define ST_MV(i, x) asm volatile(";@M " #i : "+v"(x))
#else
#define ST_M(i)
#define ST_MV(i, x)
#endif

struct st_args {
    sd_render_args a;
    sd_head m;
    int32_t *ovf;           // overflow lists (sdhip_render.h): [gridDim.x] counts, [gridDim.x][ovf_cap] blocks
    int32_t ovf_cap;
    int32_t ngroups;        // ceil(R / NW)
    int32_t tile_bytes;     // bytes per tile buffer (multiple of 1024)
};

// LDS image (byte offsets): boxes, hidden sums, weight sums, ray words, then the sample
// records [NW waves][2][K] x 40 B and two tile buffers.  The code-column and sigma A
// fragments live in VGPRs for the whole kernel (loaded from global memory once).
// boxes [2][NW waves] x 32 B, u16x2 packed (min, max): per half ray (16 B), or, when a wave
// step holds 64 samples (K R_pw = 64), per quarter = 16-sample row (halves = unions of two)
#define ST_L_BOX 0
// hidden-sum rows padded to 272 B: the DINO head reads the same 8-B slot of the NW rows in
// one instruction (256-B rows put them on one bank pair: 8-way conflicts)
#define ST_HS_ROW 272
// rpw = rays per wave and step (2 for K <= 32 and the late order's K = 64: a group is NW rpw rays)
constexpr int ST_L_HS = ST_L_BOX + 2 * ST_NW * 32;  // [NW rpw rays][128] 16-bit hidden sums
__host__ __device__ constexpr int st_l_ws(int rpw) { return ST_L_HS + ST_NW * rpw * ST_HS_ROW; }  // [NW rpw] f32 weight sums
__host__ __device__ constexpr int st_l_ray(int rpw) { return st_l_ws(rpw) + 16 * 4; }  // [NW waves][2] x rpw x 32 B ray words 0..7 (LDS-DMA)
__host__ __device__ constexpr int st_l_rec(int rpw) { return st_l_ray(rpw) + ST_NW * 2 * 32 * rpw; }  // records: [NW waves][2][rpw K] x 40 B
static_assert(st_l_rec(1) % 16 == 0 && st_l_rec(2) % 16 == 0, "record area alignment");

// record bytes for samples-per-wave-step kw = rpw K: two buffers per wave, or (late step
// order, below) one buffer and 16 B of verification flags behind it
__host__ __device__ constexpr int st_rec_bytes(int kw, bool late = false) {
    return late ? ST_NW * kw * 40 + 16 : ST_NW * 2 * kw * 40;
}

// one butterfly level of a 16-lane row sum over two values: out = a + a(lane - RA) on the
// lanes of banks MA (groups of 4 lanes), b + b(lane - RB) on the lanes of banks MB (MA | MB =
// every bank, so both bank-masked DPP adds together write every lane of out).  One asm
// statement: the compiler does not fold a partially masked DPP move into its user.  No
// s_nop past the first statement (NOP = "s_nop 1\n\t" there): the statements are volatile,
// so they stay in program order, and every later one reads values written at least two
// VALU ops before it (the callers' ordering); out is written, never read.
#define ST_BFLY(NOP, out, a, b, RA, RB, MA, MB)                                               \
    asm volatile(NOP "v_add_f32_dpp %0, %1, %1 row_ror:" #RA " row_mask:0xf bank_mask:" #MA "\n\t" \
                 "v_add_f32_dpp %0, %2, %2 row_ror:" #RB " row_mask:0xf bank_mask:" #MB      \
                 : "=&v"(out) : "v"(a), "v"(b))

// packed u16x2 (x | y << 16) component-wise min / max
__device__ __forceinline__ uint32_t st_min2(uint32_t a, uint32_t b) {
    typedef __attribute__((ext_vector_type(2))) unsigned short u16x2;
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a),
                                                                  __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ uint32_t st_max2(uint32_t a, uint32_t b) {
    typedef __attribute__((ext_vector_type(2))) unsigned short u16x2;
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a),
                                                                  __builtin_bit_cast(u16x2, b)));
}
// component-wise min / max over each 16-lane row by DPP (quad_perm xor 1, xor 2,
// row_half_mirror, row_mirror: every step's sources are inside the row), no LDS round trip
template <bool MAX>
__device__ __forceinline__ uint32_t st_row_red2(uint32_t v) {
#define ST_RSTEP(ctrl)                                                                        \
    {                                                                                         \
        const uint32_t o = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, (ctrl), 0xf, 0xf, false); \
        v = MAX ? st_max2(v, o) : st_min2(v, o);                                              \
    }
    ST_RSTEP(0xB1)
    ST_RSTEP(0x4E)
    ST_RSTEP(0x141)
    ST_RSTEP(0x140)
#undef ST_RSTEP
    return v;
}
// row-reduced value -> wave-uniform reduction of rows [r0, r1]
template <bool MAX>
__device__ __forceinline__ uint32_t st_rows2(uint32_t v, int r0, int r1) {
    uint32_t acc = (uint32_t)__builtin_amdgcn_readlane((int)v, 16 * r0);
    for (int r = r0 + 1; r <= r1; ++r) {
        const uint32_t o = (uint32_t)__builtin_amdgcn_readlane((int)v, 16 * r);
        acc = MAX ? st_max2(acc, o) : st_min2(acc, o);
    }
    return acc;
}
__device__ __forceinline__ uint32_t st_wave_min2(uint32_t v) { return st_rows2<false>(st_row_red2<false>(v), 0, 3); }
__device__ __forceinline__ uint32_t st_wave_max2(uint32_t v) { return st_rows2<true>(st_row_red2<true>(v), 0, 3); }

// tile pitch (texels per staged row): pitch mod 8 in 2..6, so that the four taps
// n, n + 1, n + pitch, n + pitch + 1 of a sample (288 B = 8 banks apart per texel) land
// on four disjoint 8-bank groups of a transposed read
// (round 6: pitch = 4 mod 8, conflict-free for the two samples of a half-wave read when they
// sit 1 or 2 texels apart along an epipolar line, measured C2 neutral and C1 +5 % -- the
// extra pad texels split more boxes; not kept)
__device__ __forceinline__ int st_pitch(int tw) {
    const int r = tw & 7;
    return tw + (r == 7 ? 3 : r == 0 ? 2 : r == 1 ? 1 : 0);
}

__device__ __forceinline__ void st_barrier_lds() {
    // wave's LDS writes visible, then the workgroup barrier; vector-memory loads (and
    // LDS-DMA) stay in flight across it
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

typedef __attribute__((address_space(3))) void lds_void;

// the per-ray and per-sample f32 output stores (plain: write-through measured no faster)
__device__ __forceinline__ void st_out(float *p, float v) { *p = v; }

// 4-byte LDS-DMA (ray words), inline asm for the reason given at sd_dma16 (sdhip_render.h)
__device__ __forceinline__ void st_dma4(const void *src, uint32_t lds_addr) {
    lds_addr = __builtin_amdgcn_readfirstlane(lds_addr);
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off"
                 :: "v"(src), "s"(lds_addr) : "memory");
}
// 16-byte LDS-DMA through a buffer resource: lane data from rsrc + soff + voff to
// lds_addr + 16 * lane (active lanes only).  The per-lane part of a staged box row's
// address (voff) is the same for every row, the row base (soff) is wave-uniform.
__device__ __forceinline__ void st_dma_buf16(__amdgpu_buffer_rsrc_t rs, uint32_t voff, uint32_t soff,
                                             uint32_t lds_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds"
                 :: "v"(voff), "s"(rs), "s"(lds_addr), "s"(soff) : "memory");
}
typedef __attribute__((ext_vector_type(4))) short s16x4;

// Record word q0.x = {LDS byte address of the sample's tap (x0, y0) | inv_f << 30 | invc << 31}
// (written by tap_addrs / late_pass, which mask the address to 18 bits: LDS is 160 KiB
// < 2^18 B, so bits 18..29 of the word are zero and the flags sit above bit 23).  The tap
// base of a lane = address + lane_off in ONE instruction: v_mad_u32_u24 multiplies the low
// 24 bits of the word -- the address alone -- by 1 (an and + an add before).
#define ST_ADDR_MASK 0x3ffffu
static_assert(160 * 1024 <= ST_ADDR_MASK + 1 && ST_ADDR_MASK < (1u << 24), "tap address field of q0.x");
__device__ __forceinline__ uint32_t st_tap_base(uint32_t q0x, uint32_t lane_off) {
    uint32_t d;
    asm("v_mad_u32_u24 %0, %1, 1, %2" : "=v"(d) : "v"(q0x), "v"(lane_off));
    return d;
}

__device__ __forceinline__ uint2 st_tr(uint32_t addr) {
    const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(uintptr_t)addr);
    return __builtin_bit_cast(uint2, v);
}

// A camera record whose fused projection (words 24..35, all sd_project_fast reads) is held in
// registers, read in front of the code that uses it: through the record's pointer the
// compiler re-read them by scalar loads at their first uses, two dependent waits in every
// sample slot of the late ray pass.  The other words (the frustum-edge re-projection of
// sd_outside_exact, a rare divergent branch) still come from memory.  Indices are constants
// after inlining, so an access is one register or one load, as before.
struct st_cam {
    sd_cfloat *m;
    const float *p;  // words 24..35
    int o;
    __device__ __forceinline__ float operator[](int i) const { return i + o >= 24 ? p[i + o - 24] : m[i + o]; }
    __device__ __forceinline__ st_cam operator+(int d) const { return st_cam{m, p, o + d}; }
};

// ZIN: depths given (args.z, parity tests) instead of drawn in the kernel.  A template
// parameter, not a branch: with both paths in one body the compiler's wait for the z loads
// also drains other loads on the drawing path.
// RPW = 2 (K <= 32, and K = 64 under LATE): every wave takes TWO neighbouring rays per step
// -- the ray pass runs their 2 K samples on the 64 lanes (LATE: two per lane), a group is
// 2 NW rays (one tile box, barrier pair, DINO head and set of DMA issues per 16 rays), the
// items of ray A then of ray B, one sum epilogue per ray.  The per-step phases that cost the
// same at any K are paid once per two rays (round-4 phase split at K = 32: items only 23 %
// of the wave time).
// LATE (128-sample wave steps only: K = 64 at RPW = 2, K = 128 at RPW = 1): the "late" step
// order on ONE record buffer per wave.  The ray pass of the next group runs at the END of
// the step, behind the epilogue that read the finished group's records, and writes into
// the same buffer; the tap boxes the step's staging needs at barrier X come from a box pass
// over the 8 endpoints of the wave's four 32-sample parts (projected pixel coordinates are
// monotone along a ray, so a part's box is spanned by its first and last sample).  The tile
// geometry is then known when the ray pass runs: it writes the LDS tap addresses itself
// (no tap_addrs) and VERIFIES every sample against its part's staged box; a miss flags the
// group, which goes to the overflow list like a box that does not fit.  Step n:
//   head(n-1) on the waves with a DINO tile | box pass(n+1) on the upper four waves, each for
//   a wave pair; ray_col(n), item 0, barrier X, stage(n+1), items 1.., vmcnt(0), epilogue(n),
//   ray pass(n+1), barrier Y, flag check(n+1)
template <int P, bool ZIN, int RPW, bool LATE = false>
__global__ void __launch_bounds__(64 * ST_NW) __attribute__((amdgpu_waves_per_eu(ST_NW / 4)))
k_render_tile(const st_args sa) {
    // The previous group's DINO head runs before the step's ray pass.  Mode 3: its first
    // W_dino tile is loaded in the step before, behind the staging (the loads land under the
    // items, and the 16 VGPRs are live only across the step boundary, not the items).  That
    // prefetch costs 16-20 VGPRs: the two-rays-per-wave body (245 VGPRs) would spill, so it
    // runs mode 2, the W_dino loads inside the head.
    constexpr int HPRE = RPW == 2 ? 2 : 3;
    constexpr int GR = ST_NW * RPW;  // rays per group
    constexpr int ST_L_WS = st_l_ws(RPW), ST_L_RAY = st_l_ray(RPW), ST_L_REC = st_l_rec(RPW);
    typedef typename RMode<P>::F Tr;  // operands upstream of sigma (f16 in both modes)
    typedef typename RMode<P>::H Th;  // DINO head (bf16 in the bf16 mode)
    typedef typename Tr::Frag Frag;
    typedef typename Tr::Frag4 Frag4;
    typedef typename Tr::E E;
    const sd_render_args &a = sa.a;
    const sd_head &m = sa.m;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
#if ST_PROF
    uint32_t pacc[19] = {};
    uint64_t tlast = __builtin_amdgcn_s_memtime();
#endif
    const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_void *)lds;  // LDS byte address of lds[0]

    const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int K = LATE ? 128 / RPW : a.K, nsub = K >> 4;   // samples / items per ray
    const int KW = K * RPW, nsubw = KW >> 4;  // per wave and step
    const int R = (int)a.R, rps = (int)a.rays_per_sb;
    const int D = m.D, ndt = D >> 4;
    const int Wf = a.Wf, Hf = a.Hf;
    const uint32_t plane_bytes = (uint32_t)Hf * Wf * SD_DH * 2;

    // records: SoA per (wave, buffer): q0 [K] x 16 B | q1 [K] x 16 B | c [K] x 8 B
    //   q0 = {x0 | y0 << 15 | inv_f << 30 | invc << 31, (w00, w01), (w10, w11), r}
    //   q1 = {x, y, z~, z}   c = {g, b}
    // (RPW = 2: record k' = r K + k is sample k of the wave's ray r)
    // (LATE: one buffer per wave, whatever buf)
    const uint32_t rec_base = ST_L_REC + (uint32_t)wave * (LATE ? 1 : 2) * KW * 40;
    auto rq0 = [&](int buf) { return (uint4 *)(lds + rec_base + (LATE ? 0 : buf) * KW * 40); };
    auto rq1 = [&](int buf) { return (f32x4 *)(lds + rec_base + (LATE ? 0 : buf) * KW * 40 + KW * 16); };
    auto rqc = [&](int buf) { return (float2 *)(lds + rec_base + (LATE ? 0 : buf) * KW * 40 + KW * 32); };
    const uint32_t tile0 = ST_L_REC + st_rec_bytes(KW, LATE);
    // LATE: verification flags [2] (one word per box slot) in the 16 B in front of the tiles
    const uint32_t flag0 = tile0 - 16;

    // XCD-aware group ranges (workgroups b, b + 8, ... share an XCD, speed only)
    const int NG = sa.ngroups;
    const int nx = (gridDim.x % 8 == 0) ? 8 : 1;
    const int xcd = blockIdx.x % nx, lb = blockIdx.x / nx, nwg = gridDim.x / nx;
    const int glo = (int)((int64_t)NG * xcd / nx), ghi = (int)((int64_t)NG * (xcd + 1) / nx);
    const int gfirst = glo + lb;
    const int nsteps = gfirst < ghi ? (ghi - gfirst + nwg - 1) / nwg : 0;
    int novf = 0;  // this workgroup's overflow blocks (workgroup-uniform)
    int32_t *ovf_list = sa.ovf + gridDim.x + (int64_t)blockIdx.x * sa.ovf_cap;
    if (nsteps == 0) {  // workgroup-uniform
        if (threadIdx.x == 0) sa.ovf[blockIdx.x] = 0;
        return;
    }

    const float zstep = (float)(1.0 / (double)K), zend = (float)(1.0 - 1.0 / (double)K);
    const int64_t cplane = (int64_t)a.Hc * a.Wc * 4;

    // ---- ray pass: lane = sample k = 64 p + lane --------------------------------------
    // ray words 0..7 (origin, direction, near, far) of a later step's ray, fetched by
    // LDS-DMA one step ahead (completed by the step's closing vmcnt(0)), so the ray pass
    // reads them from LDS instead of waiting on scalar loads
    const int nrw = min(a.ray_dim, 8);
    // memory index of the wave's ray r, given ray = GR grp + RPW wave (the wave's first
    // slot): RPW = 2 pairs ray w with ray w + NW of the group, so the two halves a group
    // splits into when its tap box overflows (kh = K below: the halves are the rays of slot
    // 0 and of slot 1) are the group's left and right 8 rays -- as adjacent pairs (2 w,
    // 2 w + 1) both halves spanned the whole strip and 2.5 % of the C1 offset-pose rays went
    // to the per-ray fallback kernel (52 us of a 0.43 ms frame)
    auto rmap = [&](int ray_, int r) { return RPW == 1 ? ray_ + r : ray_ - RPW * wave + r * ST_NW + wave; };
    // the wave's RPW rays: lane 8 r + w fetches word w of ray r
    auto ray_fetch = [&](int ray, int slot) {
        const int r = lane >> 3, w = lane & 7;
        if (r < RPW && w < nrw && rmap(ray, r) < R)
            st_dma4(a.rays + (int64_t)rmap(ray, r) * a.ray_dim + w,
                    lds0 + ST_L_RAY + (wave * 2 + slot) * 32 * RPW);
    };
    // this lane's ray of the wave's RPW for ray-pass sample slot p (record k' = 64 p + lane
    // = r K + k; the early order's two rays have K <= 32 -- p = 0 only, r = lane / K)
    const int rsl = RPW == 1 ? 0 : min(lane / K, RPW - 1);
    auto rsl_p = [&](int p) { return RPW == 1 ? 0 : min((64 * p + lane) / K, RPW - 1); };
    auto kl_p = [&](int p) { return RPW == 1 ? 64 * p + lane : 64 * p + lane - rsl_p(p) * K; };
    const float *rl = nullptr;  // this ray pass's words of the wave's first ray (set by ray_pass)
    auto load_ray_z = [&](int ray, float zq[2 * ST_MAXP]) {
        float zo[ST_MAXP];
        if (ZIN) {
            if (RPW == 1) {
                const float *zr = a.z + (int64_t)ray * K;
#pragma unroll
                for (int p = 0; p < ST_MAXP; ++p) zo[p] = zr[min(64 * p + lane, K - 1)];
            } else {
                zo[1] = 0.f;
#pragma unroll
                for (int p = 0; p < ST_MAXP; ++p) {
                    if (64 * p >= KW) break;  // wave-uniform
                    const float *zr = a.z + (int64_t)min(rmap(ray, rsl_p(p)), R - 1) * K;
                    zo[p] = zr[min(kl_p(p), K - 1)];  // (lanes past 2 K: K = 16)
                }
            }
        } else {
            zo[1] = 0.f;
#pragma unroll
            for (int p = 0; p < ST_MAXP; ++p) {
                if (64 * p >= KW) break;  // wave-uniform: KW <= 64 draws one sample per lane
                const int r = rsl_p(p);
                const float *rw = rl + 8 * r;
                const float near = rw[6], far = rw[7];
                const uint64_t base = a.z_offset + (uint64_t)rmap(ray, r) * (uint64_t)K;
                const int k = RPW == 1 ? min(64 * p + lane, K - 1) : kl_p(p);
                zo[p] = sd_z_sample_rng(near, far, K, k, sd_uniform(a.z_seed, base + k), zstep, zend,
                                    a.z_lindisp);
            }
        }
#pragma unroll
        for (int p = 0; p < ST_MAXP; ++p) {
            float nx2 = __shfl_down(zo[p], 1, 64);
            const float first_next = p + 1 < ST_MAXP
                ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(
                      __builtin_bit_cast(int, zo[p + 1 < ST_MAXP ? p + 1 : p]), 0))
                : zo[p];
            if (lane == 63) nx2 = (p + 1 < ST_MAXP && 64 * (p + 1) < KW) ? first_next : zo[p];
            zq[2 * p] = zo[p];
            zq[2 * p + 1] = nx2;
        }
    };
    // the colour texel loads of sample k = lane are left in flight (cpend) and finished
    // by ray_col at the end of the item that ran the pass
    ColPend cpend;
    // tap boxes per half ray: samples [0, kh) and [kh, K), kh = 16 (nsub / 2) -- a group
    // whose whole box does not fit a tile buffer is staged and rendered half by half
    // (RPW = 2: the halves are the two rays)
    const int kh = RPW == 1 ? 16 * (nsub >> 1) : K;
    auto ray_pass = [&](int ray, int buf, int slot) {
        uint32_t bmin0 = 0xffffffffu, bmax0 = 0u, bmin1 = 0xffffffffu, bmax1 = 0u;
        if (ray < R) {
            // wave-uniform (readfirstlane: the u32 divide runs on the VALU, and a VGPR
            // address would turn the camera-record reads into vector loads); a group's rays
            // share their super-batch (rays_per_sb % GR == 0)
            const int sbi = __builtin_amdgcn_readfirstlane((int)((unsigned)ray / (unsigned)rps));
            rl = (const float *)(lds + ST_L_RAY + (wave * 2 + slot) * 32 * RPW);
            // colour view = encoder view (the single-frame render, ids_render = ids_encoder):
            // the host passes the same camera records for both (cam_c == cam_f), so the
            // colour taps are the encoder-view taps at equal resolution (kernel-uniform test)
            const bool same_cam = a.cam_c == a.cam_f && a.Wc == Wf && a.Hc == Hf;
            float zq[2 * ST_MAXP];
            load_ray_z(ray, zq);
            ST_T(10);
            uint4 *r0 = rq0(buf);
            f32x4 *r1 = rq1(buf);
            float2 *rc = rqc(buf);
#pragma unroll
            for (int p = 0; p < ST_MAXP; ++p) {
                const int k = 64 * p + lane;  // record k' (RPW = 2: ray rsl_p(p)'s sample kl_p(p))
                if (64 * p < KW && k < KW && (RPW == 1 || rmap(ray, rsl_p(p)) < R)) {
                    const float *rw = rl + 8 * rsl_p(p);
                    const float ox = rw[0], oy = rw[1], oz = rw[2], dx = rw[3], dy = rw[4], dz = rw[5];
                    const float z0 = zq[2 * p];
                    const float px = ox + z0 * dx, py = oy + z0 * dy, pz = oz + z0 * dz;  // nerf.py:252
                    const PointGeo geo = sd_point_geo_fast((sd_cfloat *)(a.cam_f + sbi * SD_CAM_WORDS), px, py, pz,
                                                Wf, Hf);
                    const uint32_t x0 = (uint32_t)geo.t.x0, y0 = (uint32_t)geo.t.y0;
                    bool ic;
                    Taps tc;
                    if (same_cam) {  // colour view = encoder view: the same projection and taps
                        tc = geo.t;
                        ic = geo.inv_f;
                    } else {
                        tc = sd_color_taps_fast((sd_cfloat *)(a.cam_c + sbi * SD_CAM_WORDS), a.Wc, a.Hc, px, py, pz, ic);
                    }
                    const uint32_t xy = x0 | (y0 << 15) | (geo.inv_f ? 1u << 30 : 0u) |
                                        (ic ? 1u << 31 : 0u);
                    const uint4 wp = sd_pack_w<SD_F16>(geo.t.w00, geo.t.w01, geo.t.w10, geo.t.w11);
                    r1[k] = f32x4{geo.v[0], geo.v[1], geo.v[2], z0};
                    if (p == 0) {
                        sd_color_issue(a.img + (int64_t)sbi * cplane, tc, cpend);
                        r0[k] = uint4{xy, wp.x, wp.y, 0u};  // colour word written by ray_col
                    } else {
                        float col[3];
                        sd_sample_rgb(a.img + (int64_t)sbi * cplane, tc, col);
                        r0[k] = uint4{xy, wp.x, wp.y, __builtin_bit_cast(uint32_t, col[0])};
                        rc[k] = float2{col[1], col[2]};
                    }
                    const uint32_t lo = x0 | (y0 << 16);
                    if (k < kh) {
                        bmin0 = st_min2(bmin0, lo);
                        bmax0 = st_max2(bmax0, lo + 0x00010001u);
                    } else {
                        bmin1 = st_min2(bmin1, lo);
                        bmax1 = st_max2(bmax1, lo + 0x00010001u);
                    }
                }
            }
        }
        ST_T(11);
        uint8_t *bw = lds + ST_L_BOX + (slot * ST_NW + wave) * 32;
        if (KW == 64) {
            // one sample per lane: quarter q = row q (items 4 q'.. of the step), halves =
            // lanes [0, 32) and [32, 64)
            const uint32_t mnv = st_row_red2<false>(lane < 32 ? bmin0 : bmin1);
            const uint32_t mxv = st_row_red2<true>(lane < 32 ? bmax0 : bmax1);
            uint32_t q[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                q[2 * r] = st_rows2<false>(mnv, r, r);
                q[2 * r + 1] = st_rows2<true>(mxv, r, r);
            }
            ST_T(12);
            if (lane == 0) {
                *(uint4 *)bw = uint4{q[0], q[1], q[2], q[3]};
                *(uint4 *)(bw + 16) = uint4{q[4], q[5], q[6], q[7]};
            }
        } else {
            bmin0 = st_wave_min2(bmin0);
            bmax0 = st_wave_max2(bmax0);
            bmin1 = st_wave_min2(bmin1);
            bmax1 = st_wave_max2(bmax1);
            ST_T(12);
            if (lane == 0) *(uint4 *)bw = uint4{bmin0, bmax0, bmin1, bmax1};
        }
    };
    auto ray_col = [&](int ray, int buf) {
        if (rmap(ray, rsl) < R && lane < KW) {
            float col[3];
            sd_color_finish(cpend, col);
            // the texels' unused fourth words stay live to here: freed at the loads' issue,
            // the compiler reused the first one's register two instructions later and put
            // the wait for that load -- a memory latency in every step -- behind the issue
            // (late order only: the early K = 32 body has no four registers to spare)
            if constexpr (LATE)
                asm volatile("" :: "v"(cpend.a[3]), "v"(cpend.b[3]), "v"(cpend.c[3]), "v"(cpend.d[3]));
            rq0(buf)[lane].w = __builtin_bit_cast(uint32_t, col[0]);
            rqc(buf)[lane] = float2{col[1], col[2]};
        }
    };

    // ---- per-step tile geometry (workgroup-uniform) -----------------------------------
    struct Tile {
        int bx0, by0, tw, th, pitch, ok, split;
    };
    // union of the NW waves' boxes of slot over parts [p0, p1): a wave's entry holds NPART
    // (min, max) pairs -- the 4 quarters when KW = 64, else the 2 halves -- so half h =
    // parts [h NPART / 2, (h + 1) NPART / 2), the whole group = [0, NPART).  One copy of the
    // code for every part range (a select chain per range grew the kernel by half: i-cache)
    // (LATE: always the four 32-sample parts of the 128-sample wave step)
    const int NPART = (LATE || KW == 64) ? 4 : 2;
    auto box_union = [&](int slot, int p0, int p1, uint32_t &mn, uint32_t &mx) {
        // lane 2 i + h reads wave i's parts 2 h, 2 h + 1 (one LDS read; a loop over the parts
        // was four dependent LDS round trips: +45 % stage time at C2), then a wave reduction
        const uint4 *bx = (const uint4 *)(lds + ST_L_BOX + slot * ST_NW * 32);
        mn = 0xffffffffu;
        mx = 0u;
        if (lane < 2 * ST_NW) {
            const uint4 v = bx[lane];
            const int pa = 2 * (lane & 1);
            if (pa >= p0 && pa < p1) {
                mn = v.x;
                mx = v.y;
            }
            if (pa + 1 >= p0 && pa + 1 < p1) {
                mn = st_min2(mn, v.z);
                mx = st_max2(mx, v.w);
            }
        }
        static_assert(2 * ST_NW <= 16, "box entries in lane row 0");
        mn = st_rows2<false>(st_row_red2<false>(mn), 0, 0);
        mx = st_rows2<true>(st_row_red2<true>(mx), 0, 0);
    };
    // a box row of tw texels = tw x 18 16-B chunks = ceil(tw x 18 / 64) 1-KiB DMA pieces;
    // the box fits when its rows at the tile pitch fit the buffer
    auto geom = [&](uint32_t mn, uint32_t mx) {
        Tile t;
        t.bx0 = (int)(mn & 0xffffu);
        t.by0 = (int)(mn >> 16);
        t.tw = (int)(mx & 0xffffu) - t.bx0 + 1;
        t.th = (int)(mx >> 16) - t.by0 + 1;
        t.pitch = t.tw > 0 ? st_pitch(t.tw) : 1;
        t.ok = (mn != 0xffffffffu) && t.tw > 0 && t.th > 0 &&
               t.th * t.pitch * ST_TEX <= sa.tile_bytes && (t.tw * ST_TEXQ + 63) / 64 <= ST_MAXKW * ST_NW;
        t.split = 0;
        return t;
    };
    // this wave's share of the LDS-DMA of tile t into tile buffer tb: box row ty, piece c
    // (1 KiB = 64 lanes x 16 B, chunks 64 c .. 64 c + 63 of the row) goes to wave c % NW.
    // The lane's chunk (texel tx, part) and so its offset inside the row are the same for
    // every row: computed once per piece, then each row is one buffer_load ... lds with the
    // row's base as the scalar offset.  The texels' 32-B pad chunks (part 16, 17) and the
    // lanes past the row end are masked off (they are never read).
    auto dma = [&](const Tile &t, int tb, int sbi) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void *)((const uint8_t *)a.grid + (int64_t)__builtin_amdgcn_readfirstlane(sbi) * plane_bytes), 0,
            plane_bytes, 0x00020000);
        const uint32_t dst0 = lds0 + tile0 + (uint32_t)tb * (uint32_t)sa.tile_bytes;
        const int nk = (t.tw * ST_TEXQ + 63) >> 6;
        const uint32_t rowb = (uint32_t)t.pitch * ST_TEX;
        // the lane id through a volatile move: the per-piece (tx, part) below are then
        // computed here, not hoisted out of the step loop as 8 loop-invariant VGPRs (spilled
        // at 256 VGPRs: a scratch reload -- and its vmcnt(0) -- in front of every DMA piece)
        uint32_t ln;
        asm volatile("v_mov_b32 %0, %1" : "=v"(ln) : "v"(lane));
#pragma unroll
        for (int kk = 0; kk < ST_MAXKW; ++kk) {
            const int c = wave + ST_NW * kk;
            if (c >= nk) break;  // wave-uniform
            const uint32_t ci = (uint32_t)c * 64u + ln;
            const uint32_t tx = __umulhi(ci, 238609295u);  // ci / 18
            const uint32_t part = ci - 18u * tx;
            const uint32_t sx = (uint32_t)min(t.bx0 + (int)tx, Wf - 1);
            const uint32_t voff = sx * 256u + part * 16u;
            if (part < 16u && (int)tx < t.tw) {
                for (int ty = 0; ty < t.th; ++ty) {
                    const uint32_t sy = (uint32_t)min(t.by0 + ty, Hf - 1);
                    st_dma_buf16(rs, voff, __builtin_amdgcn_readfirstlane(sy * (uint32_t)Wf * 256u),
                                 __builtin_amdgcn_readfirstlane(dst0 + (uint32_t)ty * rowb + (uint32_t)c * 1024u));
                }
            }
        }
    };
    // geometry of slot's group for tile buffer tb, DMA issued: the whole box if it fits,
    // else (nsub >= 2) the first half's box when both halves fit (split = 1: the second
    // half is staged mid-step), else (KW = 64) the first quarter's when all four fit
    // (split = 3: restaged before items 1, 2, 3 -- the C1 offset-pose groups whose halves
    // overflow, 0.25 % of the rays), else the group goes to the overflow list (ok = 0).
    // An empty part (its rays past R) fits.
    auto stage = [&](int slot, int tb, int grp, int sbi) {
        ST_M(50);
        uint32_t mn, mx;
        box_union(slot, 0, NPART, mn, mx);
        ST_M(51);
        Tile t = geom(mn, mx);
        if (mn == 0xffffffffu) return t;  // no valid ray in the group
        if (!t.ok && nsub >= 2) {
#pragma unroll 1
            for (int np = 2; np <= NPART; np *= 2) {  // halves, then quarters
                bool all = true;
                for (int q = 0; q < np && all; ++q) {
                    uint32_t pn, px;
                    box_union(slot, q * NPART / np, (q + 1) * NPART / np, pn, px);
                    all = pn == 0xffffffffu || geom(pn, px).ok;
                }
                if (all) {
                    box_union(slot, 0, NPART / np, mn, mx);
                    t = geom(mn, mx);
                    t.ok = 1;
                    t.split = np - 1;
                    break;
                }
            }
        }
        if (!t.ok) {
            if (wave == 0 && lane == 0) {  // the group's rays as GR / SD_LIST_BLK list blocks
                for (int b = 0; b < GR / SD_LIST_BLK; ++b)
                    ovf_list[novf + b] = grp * (GR / SD_LIST_BLK) + b;
            }
            novf += GR / SD_LIST_BLK;
            return t;
        }
        ST_M(52);
        dma(t, tb, sbi);
        ST_M(53);
        return t;
    };

    // once a group's tile geometry is known (after stage), each wave rewrites its ray's
    // record words q0.x = {x0 | y0 << 15 | flags << 30} as {LDS byte address of tap (x0, y0)
    // in tile buffer tb | flags << 30}: an item then reads the 4 tap bases it needs with
    // two ds_read2_b32 instead of computing its own and exchanging them by ds_bpermute (a
    // chain of dependent LDS round trips at the head of every item).  Split groups: the
    // second half ray's samples get the second half's geometry.
    auto tap_addrs = [&](int rbuf, int tb, const Tile &t, int ray_) {
        if (!t.ok || ray_ >= R) return;
        // part q of a split group (split + 1 parts) = items [q nsubw / np, (q + 1) nsubw / np)
        // of the step (as the box halves / quarters of ray_pass): its records' geometry
        int gx[ST_MAXP], gy[ST_MAXP], gp[ST_MAXP];
#pragma unroll
        for (int p = 0; p < ST_MAXP; ++p) {
            gx[p] = t.bx0;
            gy[p] = t.by0;
            gp[p] = t.pitch;
        }
        const int np = t.split + 1;
#pragma unroll 1
        for (int q = 1; q < np; ++q) {
            uint32_t mn1, mx1;
            box_union(rbuf, q * NPART / np, (q + 1) * NPART / np, mn1, mx1);
            const Tile tq = geom(mn1, mx1);
            const int s0 = q * nsubw / np, s1 = (q + 1) * nsubw / np;
#pragma unroll
            for (int p = 0; p < ST_MAXP; ++p) {
                const int it = (64 * p + lane) >> 4;
                const bool mine = it >= s0 && it < s1;
                gx[p] = mine ? tq.bx0 : gx[p];
                gy[p] = mine ? tq.by0 : gy[p];
                gp[p] = mine ? tq.pitch : gp[p];
            }
        }
        const uint32_t tbase = lds0 + tile0 + (uint32_t)tb * (uint32_t)sa.tile_bytes;
        uint32_t *w = (uint32_t *)rq0(rbuf);
#pragma unroll
        for (int p = 0; p < ST_MAXP; ++p) {
            const int k = 64 * p + lane;
            if (64 * p < KW && k < KW) {
                const uint32_t xy = w[4 * k];
                const int bx0 = gx[p], by0 = gy[p], pch = gp[p];
                const int x0 = (int)(xy & 0x7fffu), y0 = (int)((xy >> 15) & 0x7fffu);
                const uint32_t ad = tbase + (uint32_t)(((y0 - by0) * pch + (x0 - bx0)) * ST_TEX);
                w[4 * k] = (ad & ST_ADDR_MASK) | (xy & 0xc0000000u);
            }
        }
    };

    // ---- late step order (LATE): box pass, verifying ray pass -------------------------
    // depth and encoder-view projection of sample k of the ray with memory index rmem (its
    // words at rw): the ONE routine of both passes, so the taps (x0, y0) the box pass takes
    // at a part's endpoints are the ray pass's own, bit for bit
    auto cam_p = [&](int sbi_, float PJ[12]) {
        sd_cfloat *c = (sd_cfloat *)(a.cam_f + sbi_ * SD_CAM_WORDS) + 24;
#pragma unroll
        for (int i = 0; i < 12; ++i) PJ[i] = c[i];
    };
    auto samp_geo = [&](const float *rw, int rmem, int k, int sbi_, const float *PJ, float &z0, float &px,
                        float &py, float &pz) {
        if (ZIN)
            z0 = a.z[(int64_t)rmem * K + k];
        else
            z0 = sd_z_sample_rng(rw[6], rw[7], K, k,
                                 sd_uniform(a.z_seed, a.z_offset + (uint64_t)rmem * (uint64_t)K + k), zstep,
                                 zend, a.z_lindisp);
        px = rw[0] + z0 * rw[3];  // nerf.py:252
        py = rw[1] + z0 * rw[4];
        pz = rw[2] + z0 * rw[5];
        return sd_point_geo_fast(st_cam{(sd_cfloat *)(a.cam_f + sbi_ * SD_CAM_WORDS), PJ, 0}, px, py, pz, Wf, Hf);
    };
    // the wave's box entry of box slot `slot` (= ray-word slot) from the endpoints of its four
    // 32-sample parts: lane e < 8 (every lane runs its e = lane & 7) takes record
    // 32 (e >> 1) + 31 (e & 1).  Along a ray z is sorted and (a + z b) / (c + z d), the clamp
    // and the floor are monotone, so the part's taps lie between its endpoints' -- wherever
    // that fails (a texel-border rounding, a ray through the camera plane, unsorted given
    // depths) late_pass's verification sends the group to the fallback.
    // PACKED: the routine is lane-independent and only 8 lanes of a wave carry an endpoint,
    // so the upper four waves run it for two waves each -- lanes [0, 8) of wave w >= NW / 2
    // take the endpoints of wave w - NW / 2, lanes [8, 16) its own (rows 1..3 repeat row 0)
    // -- and the lower four, which run the DINO head meanwhile (D = 64: tiles 0..3), skip
    // it: the SIMD issues the depth-draw + samp_geo stream once per wave pair, and the waves
    // barrier X waits for no longer run it behind their head.  The other wave's ray words
    // are in LDS since the barrier behind the step that fetched them (the prologue has one of
    // its own); the same box words go to the same LDS slots.
    auto box_pass = [&](int ray_, int slot, int sbi_) {
        if (wave < ST_NW / 2) return;  // wave-uniform
        float PJ[12];
        cam_p(sbi_, PJ);
        const int e = lane & 7;
        const int tw = wave - ST_NW / 2 + (ST_NW / 2) * ((lane >> 3) & 1);  // the endpoint's wave
        const int kr = 32 * (e >> 1) + ((e & 1) ? 31 : 0);
        const int r = RPW == 1 ? 0 : kr / K, k = kr - r * K;
        // rmap for wave tw (ray_ - RPW wave = the group's first ray)
        const int rmem = ray_ - RPW * wave + (RPW == 1 ? tw : r * ST_NW + tw);
        uint32_t mn = 0xffffffffu, mx = 0u;
        if (rmem < R) {
            const float *rw = (const float *)(lds + ST_L_RAY + (tw * 2 + slot) * 32 * RPW) + 8 * r;
            float z0, px, py, pz;
            const PointGeo geo = samp_geo(rw, rmem, k, sbi_, PJ, z0, px, py, pz);
            // an endpoint within ST_BOX_EPS texels of a texel border also claims the texel
            // across it: where a ray's samples all project onto (nearly) one point -- render
            // pose = encoder pose, pixel centres on texel borders -- the rounding noise of
            // the projection moves interior samples across the border the endpoints sit on
            const float fx = geo.t.w01 + geo.t.w11, fy = geo.t.w10 + geo.t.w11;  // ~ ix - x0, iy - y0
            const int xl = max(geo.t.x0 - (fx < ST_BOX_EPS ? 1 : 0), 0);
            const int yl = max(geo.t.y0 - (fy < ST_BOX_EPS ? 1 : 0), 0);
            const int xh = min(geo.t.x0 + (fx > 1.f - ST_BOX_EPS ? 1 : 0), Wf - 1);
            const int yh = min(geo.t.y0 + (fy > 1.f - ST_BOX_EPS ? 1 : 0), Hf - 1);
            mn = (uint32_t)xl | ((uint32_t)yl << 16);
            mx = ((uint32_t)xh | ((uint32_t)yh << 16)) + 0x00010001u;
        }
        // a part's two ends sit in lanes 2 q, 2 q + 1 (quad_perm [1, 0, 3, 2])
        mn = st_min2(mn, (uint32_t)__builtin_amdgcn_mov_dpp((int)mn, 0xB1, 0xf, 0xf, false));
        mx = st_max2(mx, (uint32_t)__builtin_amdgcn_mov_dpp((int)mx, 0xB1, 0xf, 0xf, false));
        // lane 2 q (+ 8 for the wave's own entry) writes part q's (min, max) pair: one 8-B
        // store of 8 lanes (eight v_readlane and two 16-B stores of lane 0 per wave before)
        if (lane < 16 && (lane & 1) == 0)
            *(uint2 *)(lds + ST_L_BOX + (slot * ST_NW + tw) * 32 + 8 * (e >> 1)) = uint2{mn, mx};
    };
    // the ray pass behind the epilogue: the records of the group staged as t (box / ray-word
    // slot `slot`, tile buffer tb) into the wave's one record buffer.  The tile geometry is
    // known, so q0.x is written as {LDS byte address of tap (x0, y0) | flags << 30} directly
    // (tap_addrs' form), each sample with the geometry of its part when the group is split;
    // a sample whose taps are not inside that box sets the slot's flag word (late_check).
    // The colour loads of slot p = 0 stay in flight (cpend) across the step boundary.
    auto late_pass = [&](int ray_, int slot, int tb, const Tile &t, int sbi_) {
        if (!t.ok) return;  // workgroup-uniform: an overflowed or empty group has no records
        ST_M(40);
        float PJ[12];  // the fused projection, read once for both sample slots
        cam_p(sbi_, PJ);
        int gx[ST_MAXP], gy[ST_MAXP], gp[ST_MAXP], gw[ST_MAXP], gh[ST_MAXP];
#pragma unroll
        for (int p = 0; p < ST_MAXP; ++p) {
            gx[p] = t.bx0;
            gy[p] = t.by0;
            gp[p] = t.pitch;
            gw[p] = t.tw;
            gh[p] = t.th;
        }
        const int np = t.split + 1;
#pragma unroll 1
        for (int q = 1; q < np; ++q) {  // part q = items [q nsubw / np, (q + 1) nsubw / np)
            uint32_t mn1, mx1;
            box_union(slot, q * NPART / np, (q + 1) * NPART / np, mn1, mx1);
            const Tile tq = geom(mn1, mx1);
            const int s0 = q * nsubw / np, s1 = (q + 1) * nsubw / np;
#pragma unroll
            for (int p = 0; p < ST_MAXP; ++p) {
                const int it = (64 * p + lane) >> 4;
                const bool mine = it >= s0 && it < s1;
                gx[p] = mine ? tq.bx0 : gx[p];
                gy[p] = mine ? tq.by0 : gy[p];
                gp[p] = mine ? tq.pitch : gp[p];
                gw[p] = mine ? tq.tw : gw[p];
                gh[p] = mine ? tq.th : gh[p];
            }
        }
        const uint32_t tbase = lds0 + tile0 + (uint32_t)tb * (uint32_t)sa.tile_bytes;
        const float *rl_ = (const float *)(lds + ST_L_RAY + (wave * 2 + slot) * 32 * RPW);
        const bool same_cam = a.cam_c == a.cam_f && a.Wc == Wf && a.Hc == Hf;
        uint4 *r0 = rq0(0);
        f32x4 *r1 = rq1(0);
        float2 *rc = rqc(0);
        bool miss = false;
        // one slot's samples (record 64 p + lane): geometry, verification, record words q1 and
        // q0.x .. q0.z (wq), the four colour texel loads issued into cp
        auto slot_samples = [&](int p, ColPend &cp, uint32_t wq[3]) {
            const int kr = 64 * p + lane;  // record k' = sample k of the wave's ray r
            const int r = RPW == 1 ? 0 : kr / K, k = kr - r * K;
            const int rmem = rmap(ray_, r);
            ST_M(41);
            float z0, px, py, pz;
            const PointGeo geo = samp_geo(rl_ + 8 * r, rmem, k, sbi_, PJ, z0, px, py, pz);
            ST_MV(42, z0);
            bool ic;
            Taps tc;
            if (same_cam) {  // colour view = encoder view (ray_pass)
                tc = geo.t;
                ic = geo.inv_f;
            } else {
                tc = sd_color_taps_fast((sd_cfloat *)(a.cam_c + sbi_ * SD_CAM_WORDS), a.Wc, a.Hc, px, py, pz, ic);
            }
            const int dx = geo.t.x0 - gx[p], dy = geo.t.y0 - gy[p];
            miss |= (uint32_t)dx >= (uint32_t)(gw[p] - 1) || (uint32_t)dy >= (uint32_t)(gh[p] - 1);
            const uint32_t ad = tbase + (uint32_t)((dy * gp[p] + dx) * ST_TEX);
            wq[0] = (ad & ST_ADDR_MASK) | (geo.inv_f ? 1u << 30 : 0u) | (ic ? 1u << 31 : 0u);
            const uint4 wp = sd_pack_w<SD_F16>(geo.t.w00, geo.t.w01, geo.t.w10, geo.t.w11);
            wq[1] = wp.x;
            wq[2] = wp.y;
            ST_M(43);
            r1[kr] = f32x4{geo.v[0], geo.v[1], geo.v[2], z0};
            sd_color_issue(a.img + (int64_t)sbi_ * cplane, tc, cp);
        };
        // Slot 1 first, its colour loads (c1) left in flight under the whole of slot 0's
        // geometry and finished behind it: loads return in order, so the wait for them is
        // vmcnt(4) and slot 0's four, issued later, stay in flight for ray_col.  In slot order
        // the wave stood one memory latency in every step, waiting for slot 1's texels right
        // behind their issue.  Every sample's arithmetic is unchanged (sd_color_finish is
        // sd_sample_rgb's arithmetic and order).  A slot's samples are one ray's (K = 64:
        // slot p = the wave's ray p; K = 128: both the one ray), so the tests are wave-uniform,
        // and slot 1's ray, NW rays behind slot 0's, is only there when slot 0's is: nested, so
        // that no path reaches slot 1's finish without slot 0's loads behind slot 1's (on such
        // a path the compiler's wait would be vmcnt(0), cpend's loads included).
        static_assert(ST_MAXP == 2, "late_pass: slot 1 is record 64 + lane");
        if (rmap(ray_, 0) < R) {
            const bool two = rmap(ray_, RPW - 1) < R;
            ColPend c1;
            uint32_t w1[3] = {0u, 0u, 0u}, w0[3];
            if (two) slot_samples(1, c1, w1);
            slot_samples(0, cpend, w0);
            r0[lane] = uint4{w0[0], w0[1], w0[2], 0u};  // colour word written by ray_col
            if (two) {
                float col[3];
                sd_color_finish(c1, col);
                // (the texels' unused fourth words stay live to here: freed at the loads'
                // issue, their registers were reused by slot 0's geometry, which then waited
                // for the loads to land before it could write them)
                asm volatile("" :: "v"(c1.a[3]), "v"(c1.b[3]), "v"(c1.c[3]), "v"(c1.d[3]));
                r0[64 + lane] = uint4{w1[0], w1[1], w1[2], __builtin_bit_cast(uint32_t, col[0])};
                rc[64 + lane] = float2{col[1], col[2]};
            }
        }
        ST_M(44);
        if (__builtin_amdgcn_ballot_w64(miss) != 0ull && lane == 0)
            *(volatile uint32_t *)(lds + flag0 + 4 * slot) = 1u;
    };
    // after the barrier behind late_pass: a flagged group is not rendered from its tile (the
    // DMA already issued for it is wasted and harmless) but listed for the fallback kernel,
    // as stage lists a box that does not fit.  The flag is workgroup-uniform, so is novf.
    auto late_check = [&](int slot, Tile &t, int g_) {
        if (!t.ok) return;
        const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane(
            (int)*(volatile uint32_t *)(lds + flag0 + 4 * slot));
        if (!f) return;
        t.ok = 0;
        if (wave == 0 && lane == 0) {
            for (int b = 0; b < GR / SD_LIST_BLK; ++b)
                ovf_list[novf + b] = g_ * (GR / SD_LIST_BLK) + b;
        }
        novf += GR / SD_LIST_BLK;
    };

    // ---- DINO head of one group (hsum of its NW rays in LDS) --------------------------
    // W_dino fragments of tile dt (4 x 16 B per lane).  The head runs before the step's ray
    // pass, so its wait for them does not also wait for the ray pass's colour loads (issued
    // later, consumed after item 0)
    typedef typename Th::Frag HFrag;
    // RPW = 2: this wave's DINO bias slice (tile dt = wave) in registers for the whole kernel
    // -- as a global load inside the head it put one memory latency in front of every step's
    // ray pass (C1 -1 %); at RPW = 1 the 4 VGPRs (and the rescheduling) cost more than the
    // load (`profiles/r5_bias_hoist_ab.txt`)
    constexpr bool BDH = RPW == 2;
    f32x4 bdw = {0.f, 0.f, 0.f, 0.f};
    if (BDH && wave < ndt) bdw = *(const f32x4 *)(m.b_dino + 16 * wave + 4 * g);
    auto head_w = [&](int dt, HFrag w[4]) {
        const HFrag *wo = (const HFrag *)m.w_out + (int64_t)dt * 4 * SD_WAVE + lane;
#pragma unroll
        for (int s = 0; s < 4; ++s) w[s] = wo[s * SD_WAVE];
    };
    auto head = [&](int grp, const HFrag w0[4]) {
        if (wave >= ndt) return;
        const int slot = j < GR ? j : 0;  // B columns j >= GR: not stored
        typename Th::Frag Bh[4];
        const uint8_t *hs = lds + ST_L_HS + slot * ST_HS_ROW;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint2 lo = *(const uint2 *)(hs + (32 * s + 4 * g) * 2);
            const uint2 hi = *(const uint2 *)(hs + (32 * s + 16 + 4 * g) * 2);
            Bh[s] = __builtin_bit_cast(typename Th::Frag, uint4{lo.x, lo.y, hi.x, hi.y});
        }
        const float ws = *(const float *)(lds + ST_L_WS + slot * 4);
        const int ray = GR * grp + (RPW == 1 ? j : (j % RPW) * ST_NW + j / RPW);  // hs row j = wave RPW + r
        const bool store = j < GR && ray < R;
        for (int dt = wave; dt < ndt; dt += ST_NW) {
            HFrag wl[4];
            if (HPRE == 3 && dt == wave) {
#pragma unroll
                for (int s = 0; s < 4; ++s) wl[s] = w0[s];
            } else {
                head_w(dt, wl);
            }
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 4; ++s) o = Th::mma(wl[s], Bh[s], o);
            // rows 4 g + r of tile dt = dims 16 dt + 4 g + r, column j = ray slot
            const int dim = 16 * dt + 4 * g;
            const f32x4 bd = (BDH && dt == wave) ? bdw : *(const f32x4 *)(m.b_dino + dim);
            f32x4 res;
#pragma unroll
            for (int r = 0; r < 4; ++r) res[r] = o[r] + ws * bd[r];
            if (store) *(f32x4 *)(a.dino + (int64_t)ray * a.ld_dino + dim) = res;
        }
    };

    // per-lane constant part of the transposed-read addresses: tap q = (lane & 15) >> 2
    // of a sample, columns 4 p .. 4 p + 3
    const int tq = (lane & 15) >> 2, tp = lane & 3;
    // B operand masks: lane (j, g) carries sample j's weights in K-chunk j >> 3 iff
    // ((j & 7) >> 1) == g, at elements 4 (j & 1) .. + 3
    const bool bsel = ((j & 7) >> 1) == g;
    const bool bc0 = bsel && (j >> 3) == 0, bc1 = bsel && (j >> 3) == 1;
    const bool br1 = (j & 1) != 0;
    // The four (chunk, r) positions, one instruction per B word (8 per item; as selects on
    // bc0 / bc1 / br1 the compiler nested 12 v_cndmask on 5 SGPR pairs): chunk 0's two as
    // all-ones / zero lane masks in VGPRs (v_and_b32), chunk 1's two as lane masks in SGPR
    // pairs (one v_cndmask each).  Two and two is what the register file has room for: all
    // four in VGPRs put the K = 64 kernel at 242 VGPRs and a K = 32 one into vector spills,
    // all four in SGPR pairs add to the 100-odd scalar spills.  The empty asm statements keep
    // the compiler from folding either form back into the nested selects.
    uint32_t bm[2] = {bc0 && !br1 ? ~0u : 0u, bc0 && br1 ? ~0u : 0u};
    uint64_t bq[2] = {__builtin_amdgcn_ballot_w64(bc1 && !br1), __builtin_amdgcn_ballot_w64(bc1 && br1)};
    asm volatile("" : "+v"(bm[0]), "+v"(bm[1]));
    asm volatile("" : "+s"(bq[0]), "+s"(bq[1]));
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    // this lane's code-column weight fragments (16x16x32 and 16x16x16 operands) and sigma
    // weights (every row of the sigma A fragment holds W_out[0] at hid(s, g, e),
    // mlp_pack.py), held in VGPRs for the whole kernel
    Frag wpe[8];
    Frag4 wpe1[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        wpe[t] = ((const Frag *)m.w_pe)[t * SD_WAVE + lane];
        wpe1[t] = ((const Frag4 *)((const uint8_t *)m.w_pe + 8 * SD_WAVE * 16))[t * SD_WAVE + lane];
    }
    uint4 wsig_r[4];
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) wsig_r[s2] = ((const uint4 *)m.w_sig)[s2 * SD_WAVE + lane];
    // a wait the compiler SEES (the builtin, not inline asm: vmcnt(0), expcnt / lgkmcnt
    // unconstrained): without it its wait-count tracking keeps these 20 loads pending into
    // the item loop and guards their first uses there with vmcnt(19) .. vmcnt(0) -- which the
    // hardware also counts the in-flight tile LDS-DMA against, so every item waited for the
    // next group's staging to land
    __builtin_amdgcn_s_waitcnt(0x0F70);

    // ---- prologue: records + tile of step 0 -------------------------------------------
    int grp = gfirst;
    int ray = GR * grp + RPW * wave;  // the wave's first ray of the step
    int sbi = __builtin_amdgcn_readfirstlane((int)((unsigned)min(GR * grp, R - 1) / (unsigned)rps));
    ray_fetch(ray, 0);
    ray_fetch(GR * (grp + nwg) + RPW * wave, 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    Tile cur;
    if constexpr (LATE) {
        if (threadIdx.x == 0) *(uint2 *)(lds + flag0) = uint2{0u, 0u};
        __syncthreads();  // the packed box pass reads another wave's ray words
        box_pass(ray, 0, sbi);
        st_barrier_lds();
        cur = stage(0, 0, grp, sbi);
        late_pass(ray, 0, 0, cur, sbi);  // (its colour loads: finished by step 0's ray_col)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        late_check(0, cur, grp);
    } else {
        ray_pass(ray, 0, 0);
        ray_col(ray, 0);
        st_barrier_lds();
        cur = stage(0, 0, grp, sbi);
        tap_addrs(0, 0, cur, ray);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    int prev_grp = -1, prev_ok = 0;
    HFrag hwn[4];  // HPRE 3: W_dino tile `wave` for the next step's head
#if ST_PROF
#pragma unroll
    for (int i = 0; i < 19; ++i) pacc[i] = 0;
    tlast = __builtin_amdgcn_s_memtime();
#endif
    for (int n = 0; n < nsteps; ++n) {
        ST_M(30);
        const int buf = n & 1;
        const bool has_next = n + 1 < nsteps;
        const int ngrp = grp + nwg;
        const int nray = GR * ngrp + RPW * wave;
        const int nsbi = has_next ? __builtin_amdgcn_readfirstlane((int)((unsigned)min(GR * ngrp, R - 1) / (unsigned)rps)) : 0;
        uint32_t lane_off = (uint32_t)((tq & 1) + (tq >> 1) * cur.pitch) * ST_TEX + 8u * (uint32_t)tp;

        // per-ray compositing state (RPW = 2: reset between the wave's two rays)
        float Tc, dpart, wpart, cpart[3];
        // per-lane partial sums sum_k w_k relu(h_k) over this lane's samples (one per item:
        // K / 16 = 1..8 terms), packed f16 pairs in X's element order; the 16-lane sums of
        // the epilogue are f32
        f16x2 hacc16[16];
        auto reset = [&]() {
            Tc = 1.f;
            dpart = wpart = cpart[0] = cpart[1] = cpart[2] = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) hacc16[i] = f16x2{(_Float16)0.f, (_Float16)0.f};
        };
        reset();

        // An item is split in two: A = records, taps, MFMA MLP, sigma, alpha, local
        // transmittance scan; B = weights with the carried transmittance, compositing sums,
        // per-sample outputs.
        struct IState {
            Frag X[4];
            float alpha, excl, tmul, zk, col[3];
        };
        auto itemA = [&](int sub, IState &st) {
            ST_M(20);
            const int kr = sub * 16 + j;                                 // record k'
            // the last sample of its ray (k = K - 1): lane 15 of the ray's last item -- a
            // wave-uniform test and a lane constant (k itself: 2 VALU and 2 compares an item)
            const bool last = j == 15 && (sub + 1) % nsub == 0;
            const uint4 q0 = rq0(buf)[kr];
            const f32x4 q1 = rq1(buf)[kr];
            const float2 cgb = rqc(buf)[kr];
            // z of the next sample, read by every lane (no exec branch around the read): behind
            // the ray's last sample it is the next ray's first z or, behind the buffer's last
            // record, a word of the colour array -- not used
            const float znext = ((const float *)&rq1(buf)[kr + 1])[3];
            const float v[3] = {q1[0], q1[1], q1[2]};
            st.zk = q1[3];
            const float delta = last ? 1e10f : znext - st.zk;
            st.col[0] = __builtin_bit_cast(float, q0.w);
            st.col[1] = cgb.x;
            st.col[2] = cgb.y;
            // tap bases of samples 8 c + 2 g + r, written by tap_addrs
            uint32_t base[2][2];
            const uint32_t *aw = (const uint32_t *)rq0(buf) + 4 * (sub * 16 + 2 * g);
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int r = 0; r < 2; ++r) base[c][r] = st_tap_base(aw[4 * (8 * c + r)], lane_off);
            // block-diagonal weight fragments of the two K-chunks
            ST_M(21);
            const uint32_t w01 = q0.y, w23 = q0.z;
            const uint4 b0 = {w01 & bm[0], w23 & bm[0], w01 & bm[1], w23 & bm[1]};
            const bool c10 = __builtin_amdgcn_inverse_ballot_w64(bq[0]);
            const bool c11 = __builtin_amdgcn_inverse_ballot_w64(bq[1]);
            const uint4 b1 = {c10 ? w01 : 0u, c10 ? w23 : 0u, c11 ? w01 : 0u, c11 ? w23 : 0u};
            const Frag B0 = __builtin_bit_cast(Frag, b0), B1 = __builtin_bit_cast(Frag, b1);
            f32x4 acc[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const uint2 a00 = st_tr(base[0][0] + 32u * t), a01 = st_tr(base[0][1] + 32u * t);
                const uint2 a10 = st_tr(base[1][0] + 32u * t), a11 = st_tr(base[1][1] + 32u * t);
                const Frag A0 = __builtin_bit_cast(Frag, uint4{a00.x, a00.y, a01.x, a01.y});
                const Frag A1 = __builtin_bit_cast(Frag, uint4{a10.x, a10.y, a11.x, a11.y});
                acc[t] = Tr::mma(A0, B0, zero4);
                acc[t] = Tr::mma(A1, B1, acc[t]);
            }
            ST_MV(22, acc[7]);
            // positional-code columns: all 16x16x32 steps first, then the 16x16x16 ones
            // (a 16x16x16 MFMA whose accumulator input is the result of the directly
            // preceding 16x16x32 MFMA read a stale accumulator: hipcc 7.2, gfx950,
            // VGPR-form accumulators)
            {
                Frag f0;
                Frag4 f1;
                sd_code_frags<Frag, Frag4, E>(v, g, f0, f1);
#pragma unroll
                for (int t = 0; t < 8; ++t) acc[t] = Tr::mma(wpe[t], f0, acc[t]);
#pragma unroll
                for (int t = 0; t < 8; ++t) acc[t] = Tr::mma16(wpe1[t], f1, acc[t]);
            }
            ST_MV(23, acc[7]);
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) {
                const uint4 u = {sd_relu2(sd_pack2<E>(acc[2 * s2][0], acc[2 * s2][1])),
                                 sd_relu2(sd_pack2<E>(acc[2 * s2][2], acc[2 * s2][3])),
                                 sd_relu2(sd_pack2<E>(acc[2 * s2 + 1][0], acc[2 * s2 + 1][1])),
                                 sd_relu2(sd_pack2<E>(acc[2 * s2 + 1][2], acc[2 * s2 + 1][3]))};
                st.X[s2] = __builtin_bit_cast(Frag, u);
            }
            ST_MV(24, st.X[3]);
            f32x4 sg = zero4;
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) sg = Tr::mma(__builtin_bit_cast(Frag, wsig_r[s2]), st.X[s2], sg);
            const float sigma = sd_softplus_fast(sg[0] + m.b_sigma);
            // alpha compositing (nerf.py:376-389)
            float alpha = 1.f - __expf(-fabsf(delta) * fmaxf(sigma, 0.f));
            if (a.hard_alpha_cap && last) alpha = 1.f;
            const float incl = sd_scan_mul16((1.f - alpha) + 1e-10f);
            st.alpha = alpha;
            st.excl = SD_DPP1(incl, 0x111);
            st.tmul = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, incl), 15));
            ST_MV(25, st.tmul);
        };
        auto itemB = [&](int sub, const IState &st) {
            ST_M(26);
            const int k = sub * 16 + j;  // record k'
            const float w = st.alpha * (Tc * st.excl);
            Tc *= st.tmul;
            dpart += w * st.zk;
            wpart += w;
            cpart[0] += w * st.col[0];
            cpart[1] += w * st.col[1];
            cpart[2] += w * st.col[2];
            ST_MV(27, cpart[2]);
            // hidden-space compositing: one v_pk_fma_f16 per packed pair of relu(h) (X is f16
            // in both modes, RMode)
            const f16x2 ww = __builtin_bit_cast(f16x2, sd_pack2<_Float16>(w, w));
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) {
                const uint4 u = __builtin_bit_cast(uint4, st.X[s2]);
                const uint32_t d4[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    hacc16[4 * s2 + q] = __builtin_elementwise_fma(__builtin_bit_cast(f16x2, d4[q]), ww,
                                                                   hacc16[4 * s2 + q]);
            }
            // weight and alpha into the sample's record (q1.x / .y are dead once itemA has
            // read the point); the ray epilogue stores every per-sample output coalesced
            if (g == 0) *(float2 *)&rq1(buf)[k] = float2{w, st.alpha};
            ST_M(28);
        };

        // item 0 with the next ray's pass and the previous group's head
        HFrag hw[4];
        IState s0;
        if constexpr (LATE) {
            // the previous group's head, the next group's boxes from its part endpoints, the
            // colours the late pass of the step before left in flight, then item 0
            if (HPRE == 2 && prev_ok) head(prev_grp, hw);
            if (HPRE == 3 && prev_ok) head(prev_grp, hwn);
            ST_T(1);
            if (has_next) box_pass(nray, buf ^ 1, nsbi);
            ST_T(12);
            if (cur.ok) ray_col(ray, buf);
            ST_T(3);
            if (cur.ok && rmap(ray, 0) < R) itemA(0, s0);
            ST_T(2);
        } else {
            if (HPRE == 2 && prev_ok) head(prev_grp, hw);
            if (HPRE == 3 && prev_ok) head(prev_grp, hwn);
            ST_T(1);
            if (has_next) ray_pass(nray, buf ^ 1, buf ^ 1);
            ST_T(0);
            if (cur.ok && ray < R) itemA(0, s0);
            ST_T(2);
            if (has_next) ray_col(nray, buf ^ 1);
            ST_T(3);
        }
        st_barrier_lds();  // X: next boxes visible; the head has read the hsum area
        ST_T(4);
        // LATE: the flag word of box slot buf (read behind barrier Y of the step before, set
        // again by the late pass of the next step) cleared between the two
        if (LATE && threadIdx.x == 0) *(volatile uint32_t *)(lds + flag0 + 4 * buf) = 0u;
        Tile nxt = {0, 0, 0, 0, 1, 0, 0};
        if (has_next) {
            nxt = stage(buf ^ 1, buf ^ 1, ngrp, nsbi);
            if (!LATE) tap_addrs(buf ^ 1, buf ^ 1, nxt, nray);
        }
        // the rays of step n + 2 into ray slot buf (its words, step n's rays, were read by
        // the ray pass of step n - 1): issued here, they land under this step's items (issued
        // in front of the closing vmcnt(0), as before, every step waited one memory latency)
        if (n + 2 < nsteps) ray_fetch(GR * (ngrp + nwg) + RPW * wave, buf);
        // HPRE 3: the next step's head weights (this group's; hwn was read by this step's head)
        if (HPRE == 3 && cur.ok && wave < ndt) head_w(wave, hwn);
        ST_T(5);
        // split group: items of the first half ray from the current tile, then the second
        // half's box is staged into the same buffer (workgroup-uniform branch, taken by
        // every wave: it holds barriers).  One item loop for both cases keeps the kernel
        // small (a second inlined copy of the items measured slower).
        // (RPW = 2: the first half is ray A -- a split group restages at the ray boundary)
        // (split = 3: every quarter = item of the step is staged on its own)
        const int npart = cur.split + 1;
        int qn = 1, bnd = npart > 1 ? nsubw / npart : nsubw;  // the next part, its first item
        // ray epilogue of the wave's ray r: sums over the 16 sample lanes of every row
        auto ray_sums = [&](int r) {
            ST_M(60);
            const float dsum = sd_rowsum16(dpart), wsum = sd_rowsum16(wpart);
            const float c0s = sd_rowsum16(cpart[0]), c1s = sd_rowsum16(cpart[1]),
                        c2s = sd_rowsum16(cpart[2]);
            uint8_t *hs = lds + ST_L_HS + (wave * RPW + r) * ST_HS_ROW;
            // the 32 hidden sums q = 4 t + r reduced over the 16 sample lanes of the row as a
            // butterfly (64 VALU ops instead of 32 x 4): bank-masked DPP halves the live
            // values at the first two levels, quad permutes finish -- lane bank b then holds
            // q = i + 8 b, i = 0..7 (hidden 16 (2 b + (i >> 2)) + 4 g + (i & 3))
            {
                float u[16], v[8];
                ST_M(61);
                // Level 1 on the packed pairs, without the 32 f16 -> f32 unpackings: hidden
                // sum q = 4 t + r of the butterfly's f32 [t][r] order is half r & 1 of the
                // pair hacc16[4 s2 + q'] with t = 2 s2 + (q' >> 1), r = 2 (q' & 1) + half, and
                // level 1 adds, on the lanes of banks 0, 1, pair a = [4 s2 + q'] of this lane
                // and of lane - 8, on banks 2, 3 pair b = [4 (s2 + 2) + q'] likewise.  Two
                // DPP moves (the second bank-masked) gather the rotated pair, a third (no permutation)
                // this lane's own, and one v_fma_mix_f32 per half adds them: own * 1.0 + rot
                // with both f16 operands widened inside the instruction.  Bit-equal to the
                // v_add_f32 of the two v_cvt_f32_f16 results it replaces: widening f16 to f32 is
                // exact (f16 denormals are normal f32 values; they are honoured by both forms),
                // own * 1.0 is exact, so both forms round the same real sum own + rot once, to
                // nearest even -- a multiple of 2^-24 below 2^17, never an f32 denormal -- and
                // the add commutes; inf and NaN propagate alike (5 VALU per pair of hidden sums
                // instead of 8: -24 a ray; tests/test_tile_step_trim.py evaluates both forms
                // over f16 pairs on the CPU).  The DPP moves are builtins (the
                // compiler keeps their hazards); the fma_mix statements are volatile, so they
                // stay in order in front of level 2, which reads u[i], u[i + 8] through DPP:
                // u[8] is written at least 7 VALU ops before the first level-2 statement
                // (which still opens with s_nop 1), u[15] 14 ops before the last.
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int i = 4 * (2 * s2 + (q >> 1)) + 2 * (q & 1);
                        const int pa = __builtin_bit_cast(int, hacc16[4 * s2 + q]);
                        const int pb = __builtin_bit_cast(int, hacc16[4 * (s2 + 2) + q]);
                        // row_ror:8 of a on every bank (no old value to set up), of b over banks 2, 3
                        int rot = __builtin_amdgcn_mov_dpp(pa, 0x128, 0xf, 0xf, true);
                        rot = __builtin_amdgcn_update_dpp(rot, pb, 0x128, 0xf, 0xc, false);
                        const int own = __builtin_amdgcn_update_dpp(pa, pb, 0xE4, 0xf, 0xc, false);  // quad_perm [0, 1, 2, 3]
                        asm volatile("v_fma_mix_f32 %0, %2, 1.0, %3 op_sel:[0,0,0] op_sel_hi:[1,0,1]\n\t"
                                     "v_fma_mix_f32 %1, %2, 1.0, %3 op_sel:[1,0,1] op_sel_hi:[1,0,1]"
                                     : "=&v"(u[i]), "=&v"(u[i + 1]) : "v"(own), "v"(rot));
                    }
                ST_BFLY("s_nop 1\n\t", v[0], u[0], u[8], 12, 4, 0x5, 0xa);
#pragma unroll
                for (int i = 1; i < 8; ++i) ST_BFLY("", v[i], u[i], u[i + 8], 12, 4, 0x5, 0xa);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    v[i] += SD_DPP0(v[i], 0xb1);  // quad_perm [1, 0, 3, 2]
                    v[i] += SD_DPP0(v[i], 0x4e);  // quad_perm [2, 3, 0, 1]
                }
                if ((j & 3) == 0) {
                    const int b = j >> 2;
                    typedef typename Th::E EH;  // the head's operand type
                    *(uint2 *)(hs + (32 * b + 4 * g) * 2) =
                        uint2{sd_pack2<EH>(v[0], v[1]), sd_pack2<EH>(v[2], v[3])};
                    *(uint2 *)(hs + (32 * b + 16 + 4 * g) * 2) =
                        uint2{sd_pack2<EH>(v[4], v[5]), sd_pack2<EH>(v[6], v[7])};
                }
            }
            if (lane == 0) {
                *(float *)(lds + ST_L_WS + (wave * RPW + r) * 4) = wsum;
                st_out(a.depth + (int64_t)rmap(ray, r) * a.ld_depth, dsum);
                float *rp = a.rgb + (int64_t)rmap(ray, r) * a.ld_rgb;
                st_out(rp, c0s); st_out(rp + 1, c1s); st_out(rp + 2, c2s);
            }
            ST_M(62);
        };
        for (int sub = 0; sub < nsubw; ++sub) {
            if (sub == bnd) {  // workgroup-uniform
                st_barrier_lds();  // every wave is done with the previous part's taps
                uint32_t mn1, mx1;
                box_union(buf, qn * NPART / npart, (qn + 1) * NPART / npart, mn1, mx1);
                ++qn;
                bnd = qn < npart ? qn * nsubw / npart : nsubw;
                cur = geom(mn1, mx1);  // fits (or is empty): checked when the split was chosen
                cur.ok = 1;
                dma(cur, buf, sbi);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                st_barrier_lds();
                lane_off = (uint32_t)((tq & 1) + (tq >> 1) * cur.pitch) * ST_TEX + 8u * (uint32_t)tp;
            }
            const int r = RPW == 1 ? 0 : sub / nsub;
            const bool act = cur.ok && rmap(ray, r) < R;
            if (act) {
                if (sub) itemA(sub, s0);
                itemB(sub, s0);
            }
            if (RPW > 1 && (sub + 1) % nsub == 0 && sub + 1 < nsubw) {  // ray r done
                if (act) ray_sums(r);
                reset();
            }
        }
        // this wave's LDS-DMA (next tile, ray words) landed -- waited here, in front of the
        // epilogue's output stores: vmcnt counts stores too, and a wait behind them held every
        // step for their acknowledgement (~1 memory latency)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ST_T(6);
        if (cur.ok && rmap(ray, RPW - 1) < R) ray_sums(RPW - 1);
        if (cur.ok) {
            // per-sample outputs of the wave's RPW rays, lane = record k' (one coalesced store
            // per array)
#pragma unroll
            for (int p = 0; p < ST_MAXP; ++p) {
                const int kr = 64 * p + lane;
                const int rr = RPW == 1 ? 0 : min(kr / K, RPW - 1);
                const int k = kr - rr * K;
                if (64 * p < KW && kr < KW && rmap(ray, rr) < R) {
                    const int64_t rk = (int64_t)rmap(ray, rr) * K;
                    const f32x4 q1v = rq1(buf)[kr];
                    const uint4 q0v = rq0(buf)[kr];
                    const uint32_t fl = q0v.x >> 30;
                    if (a.weights) st_out(a.weights + rk + k, q1v[0]);
                    if (a.alphas) st_out(a.alphas + rk + k, q1v[1]);
                    if (a.invalid_f) a.invalid_f[rk + k] = (uint8_t)(fl & 1u);
                    if (a.invalid) st_out(a.invalid + rk + k, fl ? 1.f : 0.f);
                    if (a.rgb_samps) {
                        const float2 cgb = rqc(buf)[kr];
                        float *rsp = a.rgb_samps + (rk + k) * 3;
                        st_out(rsp, __builtin_bit_cast(float, q0v.w));
                        st_out(rsp + 1, cgb.x);
                        st_out(rsp + 2, cgb.y);
                    }
                }
            }
        }
        ST_T(7);
        if constexpr (LATE) {
            // the epilogue has read the records: the next group's go into the same buffer
            if (has_next) late_pass(nray, buf ^ 1, buf ^ 1, nxt, nsbi);
            ST_T(0);
        }
        prev_grp = grp;
        prev_ok = cur.ok;
        grp = ngrp;
        ray = nray;
        sbi = nsbi;
        cur = nxt;
        ST_T(8);
        st_barrier_lds();  // Y: next tile complete; hsum of this group written
        ST_T(9);
        if constexpr (LATE) late_check(buf ^ 1, cur, grp);  // (cur, grp: the next step's by now)
        ST_M(39);
    }
    if (threadIdx.x == 0) sa.ovf[blockIdx.x] = novf;
    if (prev_ok) head(prev_grp, hwn);  // (mode 3: loaded in the last step)
#if ST_PROF
    if (lane < 19) {
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < 19; ++i) v = lane == i ? pacc[i] : v;
        atomicAdd(&st_prof[lane], (unsigned long long)v);
    }
    if (lane == 0) atomicAdd(&st_prof[31], 1ull);
#endif
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static int sd_check_last(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        sd_set_error(hipGetErrorString(e));
        (void)what;
        return -2;
    }
    return 0;
}

// Step order (sd_render_tile_order; the tests switch it in-process):
//   0  the default routing: late order at K = 64 (C2: both poses 8-10 % faster than the early
//      order), early order everywhere else -- at K = 128 the late order measured +1 % at the
//      offset pose, inside the run-to-run spread, and -2.5 % at the identity pose (C4,
//      `profiles/r7_late/ab_c4.txt`), so it stays a diagnostic there
//   3  late order for the 128-sample wave steps: K = 64 two rays per wave, K = 128 one
//   4  early order (the ray pass at the start of the step) at every K
// Any other value only queries the setting.
static int st_order_v = 0;
extern "C" int32_t sd_render_tile_order(int32_t order) {
    const int prev = st_order_v;
    if (order == 0 || order == 3 || order == 4) st_order_v = order;
    return prev;
}

// the late step order (k_render_tile<.., LATE>): 128-sample wave steps
static bool st_late(int K) { return st_order_v == 3 ? (K == 64 || K == 128) : st_order_v == 0 && K == 64; }

// rays per wave and step: two for K <= 32, and for the late order at K = 64
static int st_rpw(int K) { return K <= 32 || (K == 64 && st_late(K)) ? 2 : 1; }

static int st_lds_fixed(int K) {
    const int rpw = st_rpw(K);
    return st_l_rec(rpw) + st_rec_bytes(K * rpw, st_late(K));
}

// test hook (sd_render_tile_cap): tile buffers capped at this many bytes, 0 = no cap
static int st_cap_bytes = 0;
extern "C" int32_t sd_render_tile_cap(int32_t bytes) {
    const int prev = st_cap_bytes;
    st_cap_bytes = bytes > 0 ? bytes : 0;
    return prev;
}

static int st_tile_bytes(int K) {
    const int avail = 160 * 1024 - st_lds_fixed(K);
    const int b = ((avail / 2) / 1024) * 1024;
    return st_cap_bytes ? min(b, (st_cap_bytes / 1024) * 1024) : b;
}

// Can the tile kernel take this render?  (colour in exactly one render view, batches of
// whole groups, K <= 128, room for one tile buffer pair.)  The late order guards every ray
// of its last group against R, so it also takes a single batch of any ray count.
extern "C" int sd_render_tile_ok(const sd_render_args *a, const sd_head *m) {
    return a->nv == 1 && a->K % 16 == 0 && a->K <= 128 &&
           (a->rays_per_sb % (ST_NW * st_rpw(a->K)) == 0 ||
            (st_late(a->K) && a->R == a->rays_per_sb)) &&
           m->D % 16 == 0 && m->D <= 512 && a->Wf < 32768 && a->Hf < 32768 &&
           st_tile_bytes(a->K) >= 16 * 1024;
}

// Launch; ovf: device int32 [sd_ovf_words(R, sd_num_cus())] (the per-workgroup overflow
// lists, sdhip_render.h; every count written by the kernel).
extern "C" int sd_render_tile_launch(const sd_render_args *a, const sd_head *m, int32_t *ovf,
                                     void *stream) {
    hipStream_t s = (hipStream_t)stream;
    st_args sa;
    sa.a = *a;
    sa.m = *m;
    sa.ovf = ovf;
    const int ncu = sd_num_cus();
    sa.ovf_cap = (int32_t)sd_ovf_cap(a->R, ncu);
    const int rpw = st_rpw(a->K);
    sa.ngroups = (int)((a->R + ST_NW * rpw - 1) / (ST_NW * rpw));
    sa.tile_bytes = st_tile_bytes(a->K);
    const int lds_bytes = st_lds_fixed(a->K) + 2 * sa.tile_bytes;
    auto go = [&](auto kern) {
        sd_lds_attr((const void *)kern, lds_bytes);
        hipLaunchKernelGGL(kern, dim3((unsigned)ncu), dim3(64 * ST_NW), lds_bytes, s, sa);
    };
    const bool zin = a->z != nullptr;
#define ST_GO(RPWV, LATEV)                                                                            \
    if (m->dtype == SD_F16) {                                                                         \
        if (zin) go(k_render_tile<SD_F16, true, RPWV, LATEV>);                                        \
        else go(k_render_tile<SD_F16, false, RPWV, LATEV>);                                           \
    } else {                                                                                          \
        if (zin) go(k_render_tile<SD_BF16, true, RPWV, LATEV>);                                       \
        else go(k_render_tile<SD_BF16, false, RPWV, LATEV>);                                          \
    }
    if (st_late(a->K) && rpw == 2) {
        ST_GO(2, true)
    } else if (st_late(a->K)) {
        ST_GO(1, true)
    } else if (rpw == 2) {
        ST_GO(2, false)
    } else {
        ST_GO(1, false)
    }
#undef ST_GO
    return sd_check_last("sd_render_proj (tile kernel)");
}
