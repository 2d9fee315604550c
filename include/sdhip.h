/*
 * sdhip.h -- C ABI of the MI355X (gfx950) SceneDINO render hot path.
 *
 * libsdhip.so is a plain C-ABI shared library: raw device pointers, sizes and a
 * hipStream_t (passed as void*), int status returns (0 = ok, <0 = error; text via
 * sd_last_error()).  No torch types cross the boundary.  The caller owns and
 * allocates every buffer; launches are asynchronous on the given stream; the
 * library keeps no mutable global state beyond the per-thread error string.
 *
 * The reference (tum-vision/scenedino) is pure Python/PyTorch: its boundary for
 * this path is the Python plugin API (scenedino.renderer.NeRFRenderer,
 * scenedino.models.BTSNet, scenedino.common.ray_sampler.ImageRaySampler).  Each
 * entry point below replaces the reference computation cited next to it; the
 * Python mirror in scenedino_amd/ binds them with ctypes.
 *
 * Layouts (all row-major, float32 unless stated):
 *   rays        (R, ray_dim>=8)  [o(3), d(3), near, far, (frame_id, x, y)]
 *   z           (R, K)
 *   camera rec  SD_CAM_WORDS (36) floats: w2c rows 0..2 (12 floats, 3x4), K (9 floats,
 *               3x3), 3 zeros, then the fused projection P = K . w2c[:3] (12 floats,
 *               3x4, rounded once from an exact product) that the 16-bit render kernels
 *               use in place of the two-step pts_into_camera / project_to_image
 *   grid        (B, Hf, Wf, C) NHWC, element type = the FIELD dtype of the MLP dtype:
 *               sd_field_dtype(SD_F32) = SD_F32, sd_field_dtype(SD_BF16) =
 *               sd_field_dtype(SD_F16) = SD_F16 -- the bf16 mode keeps every operand
 *               upstream of sigma (grid, W_in, projected grid, taps, code) in f16 and
 *               only the DINO output layer in bf16.  The render / field
 *               entry points check the caller's grid_dtype against it (ABI 10).
 *   colour img  (B, nv, Hc, Wc, 4) NHWC4 float32 (rgb + pad)
 */
#ifndef SDHIP_H
#define SDHIP_H

#include <stdint.h>

#define SD_CAM_WORDS 36  /* floats per camera record (see layout above) */
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

enum sd_dtype { SD_F32 = 0, SD_BF16 = 1, SD_F16 = 2 };

/* Last error text of the calling thread ("" if none). */
const char *sd_last_error(void);

/* Library / ABI version (bumped on any signature change).  10: grid_dtype fields in
 * sd_render_args / sd_field_args, sd_field_dtype.  11: sd_seg_head.frag_layout.
 * 12: sd_conv_wgrad, sd_upsample2x_bwd, sd_relu_bwd (DPT decoder backward). */
int sd_abi_version(void);

/* Element type of the grids the field / render kernels read for an MLP of `dtype`
 * (sd_mlp.dtype / sd_head.dtype): SD_F32 -> SD_F32, SD_BF16 and SD_F16 -> SD_F16.
 * Returns -1 for an unknown dtype.  Pack a grid for sd_render_fused / sd_field_query with
 * sd_pack_grid / sd_cast_grid(dtype = sd_field_dtype(mlp dtype)); sd_project_grid* write
 * the projected grid in sd_field_dtype(mlp->dtype). */
int sd_field_dtype(int dtype);

/* Leave n CUs of the device to other kernels: the persistent one-workgroup-per-CU grids
 * (projection, tile render and its fallback, field query, ...) launch on the device's CUs
 * minus n, rounded down to a multiple of 8.  For the multi-GPU step, whose RCCL all-gather of
 * the previous frame (one workgroup per channel, NCCL_MAX_NCHANNELS) runs beside the render:
 * a persistent workgroup whose CU that kernel holds would start only after it.  Process-wide;
 * set it before sizing sd_render_proj's work (sd_render_proj_work_bytes depends on it).
 * Returns the previous value. */
int32_t sd_reserve_cus(int32_t n);

/* Diagnostic: nblocks single-wave workgroups spinning for `us` microseconds on the stream
 * (stands in for another stream's kernel holding CUs, tools/contention_ab.py). */
int sd_spin(int32_t nblocks, float us, void *stream);

/* Frustum ray generation, bit-exact with the reference's fp32 arithmetic.
 * Replaces util.unproj_map + util.gen_rays + ImageRaySampler.sample
 *   (scenedino/common/util.py:113-158, util.py:253-285,
 *    scenedino/common/ray_sampler.py:439-513).
 * poses_c2w (n_views,4,4), Ks (n_views,3,3) normalised intrinsics,
 * frame_ids (n_views); rays_out (n_views, H, W, 11). */
int sd_gen_rays(const float *poses_c2w, const float *Ks, const float *frame_ids,
                int64_t n_views, int64_t H, int64_t W, float z_near, float z_far,
                float *rays_out, void *stream);

/* Patch ray sampling (training batches): PatchRaySampler.sample with snap_to_grid
 * (scenedino/common/ray_sampler.py:136-287).  The caller draws the patch positions with the
 * reference's own RNG calls (host) and passes them as patches (B, n_patches, 4) int32:
 * [view, top-left y, top-left x, DINO cell row * dino_w + col].  Only the sampled pixels'
 * rays are generated (bit-exact with sd_gen_rays / util.gen_rays); the rgb target
 * (images (B, V, channels, H, W)) and the DINO target (dino (B, V, dino_c, dino_h, dino_w):
 * per pixel if dino_upscaled, else one row per patch) are gathered alongside.
 * Outputs: rays (B, n_patches*ph*pw, 11), rgb_out (B, n_patches*ph*pw, channels),
 * dino_out (B, n_patches*ph*pw, dino_c) or (B, n_patches, dino_c); rgb_out / dino_out may
 * be NULL.  All pointers are device pointers except the struct itself. */
typedef struct sd_patch_args {
    const float *poses;      /* (B, V, 4, 4) camera-to-world                               */
    const float *Ks;         /* (B, V, 3, 3) normalised intrinsics                         */
    const float *frame_ids;  /* (V) ray frame-id column                                    */
    const int32_t *patches;  /* (B, n_patches, 4)                                          */
    const float *images;     /* (B, V, channels, H, W) or NULL                             */
    const float *dino;       /* (B, V, dino_c, dino_h, dino_w) or NULL                     */
    float *rays;
    float *rgb_out;
    float *dino_out;
    int64_t B, V, H, W;
    int32_t n_patches, ph, pw, channels;
    int32_t dino_c, dino_h, dino_w, dino_upscaled;
    float z_near, z_far;
} sd_patch_args;

int sd_patch_rays(const sd_patch_args *args, void *stream);

/* Channels-last f32 grid (n elements, n % 4 == 0) -> element type dtype (SD_BF16 / SD_F16),
 * same layout: the NHWC gather operand of sd_render_fused / sd_field_query when the grid
 * already is channels-last (sd_pack_grid transposes an NCHW one).  A plain conversion: for
 * the render / field kernels pass dtype = sd_field_dtype(mlp dtype) (f16 in both 16-bit
 * modes) and set grid_dtype to the same value. */
int sd_cast_grid(const float *grid_nhwc, int64_t n, int dtype, void *out, void *stream);

/* Stratified inverse-depth (lindisp) or linear z sampling.
 * Replaces NeRFRenderer.sample_coarse (scenedino/renderer/nerf.py:121-141).
 * u == NULL: jitter drawn from a counter-based RNG keyed by (seed, offset);
 * u != NULL: jitter read from u (R, K) -> bit-exact with the reference. */
int sd_sample_z(const float *rays, int64_t R, int64_t ray_dim, int64_t K, int lindisp,
                const float *u, uint64_t seed, uint64_t offset, float *z_out, void *stream);

/* NCHW float32 feature grid (B,C,H,W) -> NHWC (B,H,W,C) in element type dtype (a plain
 * conversion; the render / field kernels read sd_field_dtype(mlp dtype), see above).
 * Layout step for F.grid_sample over BTSNet.grid_f_features (bts.py:299-309). */
int sd_pack_grid(const float *grid_nchw, int64_t B, int64_t C, int64_t H, int64_t W,
                 int dtype, void *out_nhwc, void *stream);

/* NCHW colour images (B*nv, 3, H, W) -> NHWC4 float32 (B*nv, H, W, 4).
 * Layout step for BTSNet.sample_colors' F.grid_sample (bts.py:348-358). */
int sd_pack_image(const float *img_nchw, int64_t N, int64_t H, int64_t W, float *out_nhwc4,
                  void *stream);

/* Camera records of n views: out (n, 36) = [w2c rows 0..2 (3x4) | K (3x3) | 0 0 0 | K.w2c (3x4)], the
 * operands of pts_into_camera / project_to_image (pinhole.py:40-84) as the field
 * kernels read them.  w2c: (n, 4, 4) with element stride s_w (>= 16) between views,
 * inner 4x4 contiguous; Ks: (n, 3, 3), stride s_k (>= 9). */
int sd_cam_records(const float *w2c, int64_t s_w, const float *Ks, int64_t s_k, int64_t n,
                   float *out, void *stream);

/* sd_pack_image + sd_cam_records in one launch (the per-frame render inputs of
 * BTSNet.encode's colour images and encoder cameras; same outputs as the two calls). */
int sd_frame_inputs(const float *img_nchw, int64_t N, int64_t H, int64_t W, float *out_nhwc4,
                    const float *w2c, int64_t s_w, const float *Ks, int64_t s_k, int64_t n,
                    float *out_cam, void *stream);

/* The operands of sd_frame_inputs, for sd_project_grid_nhwc_inputs below. */
typedef struct sd_frame_args {
    const float *img_nchw; int64_t N, H, W; float *out_nhwc4;
    const float *w2c; int64_t s_w; const float *Ks; int64_t s_k; int64_t n; float *out_cam;
} sd_frame_args;

/* Per-point MLP parameters, pre-packed (by the host) into MFMA fragment order.
 * ResnetFC(n_blocks=0): out = W_out relu(W_in x + b_in) + b_out
 *   (scenedino/models/prediction_heads/resnetfc.py:135-203). */
typedef struct sd_mlp {
    const void *w_in;      /* [C/16+3][4][64][8] of dtype (layer-1 A fragments)            */
    const float *b_in_h;   /* [4][2][16] hidden bias, accumulator-row order                */
    const float *w_sig_h;  /* [4][2][16] W_out row 0 (sigma), accumulator-row order        */
    float b_sigma;         /* b_out[0]                                                     */
    const void *w_out;     /* layer-2 A fragments for the D dino rows (dtype-specific)     */
    const float *b_dino;   /* b_out[1:1+D]                                                 */
    int32_t C;             /* grid channels (multiple of 32)                               */
    int32_t D;             /* dino dims (multiple of 32)                                   */
    int32_t dtype;         /* SD_F32 (exact-f32 MFMA), SD_BF16 or SD_F16 (16-bit MFMA,   */
                           /* f32 accumulate); grids and w_in are in sd_field_dtype(dtype) */
                           /* (f16 for SD_BF16 too), the dino output layer in dtype        */
    int32_t d_hidden;      /* must be 128                                                  */
    const float *b_empty_h; /* learn_empty (bts.py:311-319), NULL if off: [4][2][16]       */
                           /* b_in + W_in[:, :C] . empty_feature in accumulator-row order:  */
                           /* the layer-1 pre-code activation of a point outside the       */
                           /* encoder frustum (sd_render_fused / sd_field_query only)       */
    int32_t proj_flags;    /* sd_project_grid*: bit 0 (SD_PROJ_EXACT_GRID) = the f32 grid   */
                           /* enters the MFMA as a hi + lo f16 pair (hi = f16(g), lo =      */
                           /* f16(g - hi)): P within ~2^-12 of W16 . G instead of W16 . G16 */
                           /* -- twice the MFMAs; configs[3]'s K = 128 renders need it for  */
                           /* the 1e-2 m depth bound.  0 = one f16 rounding.    */
    int32_t pad_mlp;
} sd_mlp;

#define SD_PROJ_EXACT_GRID 1

/* Fused coarse render of R rays x K samples: point generation, projection into the
 * encoder view, positional code, bilinear feature gather, MFMA MLP, softplus,
 * colour sampling in nv render views, alpha compositing (sequential
 * transmittance per ray) of depth / DINO features / colour.
 * Replaces NeRFRenderer.composite + BTSNet.forward + sample_features + sample_colors
 *   (nerf.py:230-449, bts.py:271-441, bts.py:476-595).
 * Optional per-sample outputs may be NULL. */
typedef struct sd_render_args {
    const float *rays; int64_t ray_dim; int64_t R; int64_t rays_per_sb; int32_t K;
    const float *z;                       /* (R, K)                                */
    const void *grid; int32_t Hf, Wf;     /* (B, Hf, Wf, C) NHWC                   */
    const float *cam_f;                   /* (B, 36)                               */
    const float *img; int32_t nv, Hc, Wc; /* (B, nv, Hc, Wc, 4) or NULL if nv==0   */
    const float *cam_c;                   /* (B, nv, 36); may alias cam_f (nv == 1, */
                                          /* colour view = encoder view): the render */
                                          /* kernels then re-use the encoder taps    */
                                          /* for the colours at equal resolution     */
    int32_t hard_alpha_cap;
    /* required outputs */
    float *depth;      /* (R)        */
    float *dino;       /* (R, D)     */
    float *rgb;        /* (R, 3 nv)  */
    /* optional outputs (NULL = not wanted) */
    float *weights;    /* (R, K)         */
    float *alphas;     /* (R, K)         */
    float *invalid;    /* (R, K, nv)     */
    uint8_t *invalid_f;/* (R, K)         */
    float *rgb_samps;  /* (R, K, 3 nv)   */
    /* In-kernel z sampling (sd_render_proj only): with z == NULL the kernel draws
     * each ray's depths itself exactly as sd_sample_z(rays, R, ray_dim, K, z_lindisp,
     * NULL, z_seed, z_offset) would (NeRFRenderer.sample_coarse, nerf.py:121-141),
     * so the (R, K) depth array never goes through HBM.  Ignored when z != NULL. */
    int32_t z_lindisp;
    uint64_t z_seed, z_offset;
    /* Scratch of sd_render_proj_work_bytes(R, D) bytes (sd_render_proj only; NULL when
     * that is 0): for wide DINO heads the kernel composites the 128-d hidden vectors,
     * sum_k w_k relu(h_k), and applies W_dino once per ray afterwards (the output layer is
     * linear: sum_k w_k (W h_k + b) = W sum_k w_k h_k + b sum_k w_k, nerf.py:394 over
     * resnetfc.py:199). */
    float *work;
    /* Row strides (in floats) of depth / dino / rgb; 0 = dense (1, D, 3 nv).  Lets the caller
     * render straight into one packed [dino | depth | rgb] row per ray, e.g. the send buffer
     * of the multi-GPU all-gather (sd_render_proj only; sd_render_fused requires 0).  The dino
     * rows are written as 16-byte vectors: dino must be 16-byte aligned and ld_dino % 4 == 0
     * (packed rows put dino first and pad the row to a multiple of 4 floats), else -1. */
    int64_t ld_depth, ld_dino, ld_rgb;
    /* Element type of `grid`, checked against what the kernel reads (ABI 10): sd_render_fused
     * sd_field_dtype(mlp->dtype); sd_render_proj SD_F16 (the projected grid of both 16-bit
     * modes).  A mismatch returns -1 instead of reading the bits as another type. */
    int32_t grid_dtype;
    int32_t pad1;
} sd_render_args;

int sd_render_fused(const sd_render_args *args, const sd_mlp *mlp, void *stream);

/* ---- projected-grid render (16-bit modes) ----------------------------------
 * F.grid_sample is linear in the grid and its bilinear weights sum to one, so the
 * grid part of ResnetFC's first layer commutes with the feature gather
 * (bts.py:299-328 then resnetfc.py:163):
 *     W_in[:, :C] . sample(G, xy) + b_in  ==  sample(W_in[:, :C] . G + b_in, xy).
 * sd_project_grid evaluates P = W_in[:, :C] . G + b_in once per grid PIXEL (an MFMA
 * GEMM over C); sd_render_proj then gathers 128-channel P taps per sample and adds
 * the positional-code columns by MFMA.  Same outputs as sd_render_fused up to
 * rounding order (16-bit modes only; the f32 parity mode keeps sd_render_fused). */

/* grid_nchw (B, C, Hf, Wf) float32 -> out (B, Hf, Wf, 128) in sd_field_dtype(mlp->dtype)
 * (f16 for both 16-bit modes; mlp->dtype must be SD_BF16 or SD_F16),
 * plain NHWC: out[b][y][x][n] = P[y][x][n], 256 B per grid pixel.
 * Uses mlp->w_in chunks 0..C/16-1 and mlp->b_in_h. */
int sd_project_grid(const float *grid_nchw, int64_t B, int64_t Hf, int64_t Wf,
                    const sd_mlp *mlp, void *out, void *stream);

/* Same from a channels-last grid (B, Hf, Wf, C) float32 -- the layout the native encoder's
 * DPT writes (its NCHW-shaped grid_f_features is a permuted view of it). */
int sd_project_grid_nhwc(const float *grid_nhwc, int64_t B, int64_t Hf, int64_t Wf,
                         const sd_mlp *mlp, void *out, void *stream);

/* sd_project_grid_nhwc + sd_frame_inputs(*frame) -- a new frame's render inputs -- in ONE
 * launch where the streaming projection kernel takes the grid (C = 256): its workgroups
 * pack the image and write the camera records before their grid sweep (one kernel
 * boundary fewer per frame).  Same outputs as the two calls (which it makes otherwise). */
int sd_project_grid_nhwc_inputs(const float *grid_nhwc, int64_t B, int64_t Hf, int64_t Wf,
                                const sd_mlp *mlp, void *out, const sd_frame_args *frame,
                                void *stream);

/* Head of the projected render: code columns of W_in and the output layer, packed
 * for 16x16x32 MFMA (scenedino_amd/mlp_pack.py documents the fragment maps). */
typedef struct sd_head {
    const void *w_pe;      /* [8][64][8] ++ [8][64][4] code-column A fragments, dtype */
    const void *w_sig;     /* [4][64][8]    W_out row 0 (sigma) A fragments, dtype    */
    const void *w_out;     /* [D/16][4][64][8] W_out rows 1..D A fragments, dtype     */
    const float *b_dino;   /* b_out[1:1+D]                                            */
    float b_sigma;         /* b_out[0]                                                */
    int32_t D;             /* multiple of 16, <= 512                                  */
    int32_t dtype;         /* SD_BF16 or SD_F16: w_out (the DINO head) in dtype; w_pe and */
                           /* w_sig in sd_field_dtype(dtype) = f16 in both modes          */
} sd_head;

/* args->grid = the projected grid (B, Hf, Wf, 128) f16 from sd_project_grid (grid_dtype
 * SD_F16); K % 16 == 0.
 * Outputs as sd_render_fused; args->z may be NULL (in-kernel z sampling, see above). */
int sd_render_proj(const sd_render_args *args, const sd_head *head, void *stream);

/* Bytes of args->work sd_render_proj needs for R rays and a D-dim DINO head (0: none). */
int64_t sd_render_proj_work_bytes(int64_t R, int32_t D);

/* Test hook: cap the tile kernel's tile buffers at `bytes` (rounded down to KiB; 0 = no cap;
 * below 16 KiB the per-ray kernel renders everything), so a test can force tap boxes into
 * the per-workgroup overflow lists and the per-ray fallback behind the tile kernel.  Returns
 * the previous cap.  Process-wide, not thread-safe; the shipped path never sets it. */
int32_t sd_render_tile_cap(int32_t bytes);

/* Test hook: the tile kernel's step order.  0 = the default routing (late order at K = 64,
 * early order elsewhere); 3 = late order (one record buffer, box pass + verifying ray pass)
 * for K = 64 (two rays per wave) and K = 128; 4 = early order at every K (two rays per wave
 * for K <= 32 only).  Starts at 0.  Returns the previous setting; any other value only
 * queries.  Process-wide, not thread-safe; the shipped path never sets it. */
int32_t sd_render_tile_order(int32_t order);

/* Per-point field query without compositing (BTSNet.forward on raw points,
 * bts.py:476-595; SSCBench predict_grid / demo inference_3d).  Points are
 * (B, P, 3); outputs sigma (B,P), dino (B,P,D); colour outputs optional. */
typedef struct sd_field_args {
    const float *xyz; int64_t B; int64_t P;
    const void *grid; int32_t Hf, Wf;
    const float *cam_f;                   /* (B, 36)            */
    const float *img; int32_t nv, Hc, Wc; /* may be NULL / nv=0 */
    const float *cam_c;                   /* (B, nv, 36)        */
    float *sigma;      /* (B, P)             */
    float *dino;       /* (B, P, D)          */
    float *rgb;        /* (B, P, 3 nv) or NULL */
    float *invalid;    /* (B, P, nv) or NULL   */
    uint8_t *invalid_f;/* (B, P) or NULL       */
    int32_t dino_dtype;/* SD_F32 (0), or SD_BF16: dino written as bf16 (the input a
                        * following sd_seg_query rounds to bf16 anyway: half the bytes) */
    int32_t grid_dtype;/* element type of grid (ABI 10): sd_field_dtype(mlp->dtype); checked */
    /* Visiting order of the ceil(B P / 32) tiles of 32 consecutive points, or NULL (natural
     * order).  Speed only (every output stays at its point's index): an order in which
     * consecutive tiles project onto neighbouring texels keeps the grid taps in the XCD's
     * L2 (the SSCBench voxel columns sorted by projected pixel, BTSNet.query). */
    const int32_t *tile_order;
} sd_field_args;

int sd_field_query(const sd_field_args *args, const sd_mlp *mlp, void *stream);

/* Standalone alpha compositing for an arbitrary (non-fused) field model.
 * Replaces nerf.py:343-405.  sigma,z (R,K); feat (R,K,F) optional, rgb (R,K,Cc). */
int sd_composite(const float *z, const float *sigma, const float *feat, int64_t F,
                 const float *rgb, int64_t Cc, int64_t R, int32_t K, int32_t hard_alpha_cap,
                 float *weights, float *alphas, float *depth, float *feat_out, float *rgb_out,
                 void *stream);

/* ---- Differentiable (training) field path (sdhip_train.hip) ----------------- */

/* MLP input rows of the training path: per point the projection / frustum mask
 * (pinhole.py:40-112), the bilinear border gather of the C grid channels
 * (bts.py:299-309, F.grid_sample align_corners=False) and the 39-d positional code
 * (positional_encoding.py:13-80), written as x_out (B*P, C+40) = [feat | code | 1]
 * (bts.py:321-328; the constant 1 column carries the ResnetFC biases through its GEMMs).  grid_nhwc (B, Hf, Wf, C) f32.  Colour samples / masks as
 * sd_field_query (bts.py:330-441; rgb, invalid, img, cam_c may be NULL / nv = 0).
 * x_out element type x_dtype: SD_F32, or SD_F16 / SD_BF16 (the MLP's autocast dtype). */
int sd_field_gather(const float *xyz, int64_t B, int64_t P, const float *grid_nhwc,
                    int32_t C, int32_t Hf, int32_t Wf, const float *cam_f,
                    const float *img, int32_t nv, int32_t Hc, int32_t Wc,
                    const float *cam_c, void *x_out, int32_t x_dtype /* sd_dtype */,
                    uint8_t *invalid_f, float *rgb, float *invalid, void *stream);

/* Backward of the feature gather (grid_sample input gradient, bts.py:299-309):
 * dgrid_nhwc (B, Hf, Wf, C) += bilinear scatter of dx[:, :C] (row stride ldx).
 * Accumulates with f32 atomics: the caller zeroes dgrid_nhwc. */
int sd_field_gather_bwd(const float *xyz, int64_t B, int64_t P, const void *dx,
                        int32_t dx_dtype /* sd_dtype */, int64_t ldx, int32_t C, int32_t Hf,
                        int32_t Wf, const float *cam_f, float *dgrid_nhwc, void *stream);

/* NHWC f32 (B, H, W, C) -> NCHW f32 (B, C, H, W): the grid gradient of the training path
 * back in the encoder's layout (inverse of sd_pack_grid with dtype SD_F32). */
int sd_unpack_grid(const float *grid_nhwc, int64_t B, int64_t C, int64_t H, int64_t W,
                   float *grid_nchw, void *stream);

/* Backward of sd_composite (alpha compositing, nerf.py:376-405): upstream gradients
 * of depth (R), feat_out (R,F), rgb_out (R,Cc), weights (R,K), alphas (R,K) (any may be
 * NULL) -> d_sigma (R,K) and, when non-NULL, d_feat (R,K,F) / d_rgb (R,K,Cc).
 * K <= 512.  Division-free reverse transmittance recurrence (sdhip_train.hip). */
int sd_composite_bwd(const float *z, const float *sigma, const float *feat, int64_t F,
                     const float *rgb, int64_t Cc, int64_t R, int32_t K,
                     int32_t hard_alpha_cap, const float *g_depth, const float *g_feat,
                     const float *g_rgb, const float *g_weights, const float *g_alphas,
                     float *d_sigma, float *d_feat, float *d_rgb, void *stream);

/* ---- SSCBench voxel query (sdhip_seg.hip) ---------------------------------- */

/* Voxel-centre grid of nx*ny*nz voxels, flat index (ix*ny + iy)*nz + iz (meshgrid ij),
 * centre_j = f32(f64(f32 origin_j) + vox*coord_j + vox*0.5), moved by the rigid transform
 * T (rows 0..2 of a 4x4, fp64) and stored as f32 (pts_out (n, 3), device).  Bit-exact with
 * generate_point_grid -> TSDFVolume.vox2world -> rigid_transform -> .float()
 *   (sscbench/point_utils.py:17-82, sscbench/fusion.py:203-219,407-411,
 *    sscbench/evaluate_model_sscbench.py:270-278).
 * origin (3) and T (12, row-major rows 0..2) are HOST pointers read during the call. */
int sd_voxel_points(const double *origin, double vox, int64_t nx, int64_t ny, int64_t nz,
                    const double *T, float *pts_out, void *stream);

/* Folded MlpDimReduction.transform_expand + SemanticHead("stego_kmeans"), pre-packed by
 * the host into 32x32x16 MFMA fragment order (scenedino_amd/seg_pack.py documents every
 * map).  W1/W2: dim_reduction linear_in / linear_out; L = Wl W2, M = Wn1 W2 with Wl, Wn1,
 * Wn2 the StegoClusterHead 1x1 convolutions; centres = normalised cluster centres. */
typedef struct sd_seg_head {
    const void *w1;        /* bf16 [d_latent/32][d_in/16][64][8]                      */
    const float *b1;       /* [d_latent/32][2][16] accumulator-row order              */
    const void *w2;        /* bf16 [d_full/32][d_latent/16][64][8]                    */
    const float *b2;       /* [d_full/32][2][16]                                      */
    const void *wl;        /* bf16 [d_code/32][d_latent/16][64][8]  L = Wl W2         */
    const float *bl;       /* [d_code/32][2][16]  Wl b2                               */
    const float *bo;       /* [d_code/32][2][16]  bl + bn2                            */
    const void *wm;        /* bf16 [d_full/32][d_latent/16][64][8]  M = Wn1 W2        */
    const float *bm;       /* [d_full/32][2][16]  Wn1 b2                              */
    const float *bn1;      /* [d_full/32][2][16]                                      */
    const void *wn2;       /* bf16 [d_code/32][d_full/16][64][8]                      */
    const void *centres;   /* normalised centres as bf16 A fragments, hi and lo halves:
                            * [ceil(n_clusters/32)][2][d_code/16][64][8], rows = clusters
                            * (zero rows pad the last tile), permuted k order          */
    const int32_t *assign; /* [n_clusters] pseudo_assignment                           */
    int32_t n_clusters;    /* 1..256                                                   */
    int32_t d_in;          /* 64  (reduced DINO dims)                                  */
    int32_t d_latent;      /* 128                                                      */
    int32_t d_full;        /* multiple of 32 (768)                                     */
    int32_t d_code;        /* 64                                                       */
    /* optional fp8 norm product (NULL: bf16 w2).  OCP e4m3 fragments of W2 * 2^-e_w for
     * v_mfma_scale_f32_32x32x64_f8f6f4, [d_full/32][d_latent/64][64][32] bytes, k order
     * the fp8 accumulator-as-operand permutation (scenedino_amd/seg_pack.py); used for
     * |W2 h + b2| of the labels/seg outputs (dino_full keeps the bf16 w2)            */
    const void *w2_f8;
    float w2_f8_scale;     /* 2^e_w                                                    */
    int32_t pad0;
    /* the norm by the Gram form |e|^2 = h^T G h + 2 g.h + |b2|^2 (every bf16 launch):
     * G = W2^T W2 as bf16 hi + lo fragments, tile t = 16 fragments (hi k-steps 0..7,
     * lo 0..7), [d_latent/32][16][64][8], permuted k order                           */
    const void *wg;
    const float *g2;       /* [d_latent/32][2][16]  2 W2^T b2                         */
    float b2sq;            /* |b2|^2                                                   */
    /* SD_SEG_FRAG32 (0): the maps above, v_mfma_f32_32x32x16_bf16 fragments (needed by
     * the fp8 norm, w2_f8).  SD_SEG_FRAG16 (1, ABI 11, the default record): the same
     * products on v_mfma_f32_16x16x32_bf16 (lane l: row / column l & 15, k = 8 (l >> 4) + j;
     * accumulator register i of lane group g = l >> 4 holds row 4 g + i), every map with
     * 16-row tiles and 32-deep k-steps:
     *   w1 [d_latent/16][d_in/32][64][8]  W1[16 t + (l&15)][32 s + 8 (l>>4) + j]
     *   w2, wm [d_full/16][d_latent/32][64][8], wl [d_code/16][d_latent/32][64][8],
     *   wn2 [d_code/16][d_full/32][64][8]  W[16 t + (l&15)][perm16(q, l>>4, j)],
     *     perm16(q, g, j) = 32 q + 16 (j >> 2) + 4 g + (j & 3)
     *   wg [d_latent/32][16][64][8]: fragment i of tile t = G hi (i & 4 == 0) or lo of
     *     row tile 2 t + (i >> 3), k-step i & 3
     *   centres [ceil(n_clusters/16)][2][d_code/32][64][8]
     *   row vectors (b1, b2, bl, bo, bm, bn1, g2) [d/16][4][4]: vec[16 t + 4 g + i]
     * (scenedino_amd/seg_pack.py builds both)                                           */
    int32_t frag_layout;
} sd_seg_head;

#define SD_SEG_FRAG32 0
#define SD_SEG_FRAG16 1

/* Grow: out = 3x3x3 max filter of the (nx, ny, nz) f32 density grid in (z fastest),
 * F.max_pool3d(kernel_size=3, stride=1, padding=1) as evaluate_model_sscbench.py:755-756
 * applies it (NaN propagates; out-of-grid neighbours never win).  in != out,
 * nx * ny * nz < 2^31. */
int sd_grow3(const float *in, int64_t nx, int64_t ny, int64_t nz, float *out, void *stream);

/* Per-point segmentation head on P DINO codes dino (P, d_in), SD_F32 or SD_BF16 (16-B
 * aligned; the kernel's first MFMA takes them as bf16 either way).
 * Replaces BTSNet.forward(predict_segmentation=True)'s encoder.expand_dim +
 * downstream_head(..., "stego_kmeans") (bts.py:584-592, dim_reduction.py:22-25,
 * semantic_head.py:107-111,285-373) and, with seg, the SSCBench alpha-weighted class pick
 * (evaluate_model_sscbench.py:727-742, factor 1).  Outputs (device, NULL = not wanted):
 *   labels    (P) int32  pseudo_assignment[argmax_k cos(stego, c_k)]
 *   seg       (P) uint8  alpha > 0 ? label : 0, alpha = 1 - exp(-voxel_size * sigma)
 *                        (needs sigma (P) f32)
 *   dino_full (P, d_full) f32  transform_expand output (L2-normalised)
 * At least one output; labels/seg need the stego fields of h. */
int sd_seg_query(const void *dino, int32_t dino_dtype, int64_t P, const sd_seg_head *h,
                 const float *sigma, float voxel_size, int32_t *labels, uint8_t *seg,
                 float *dino_full, void *stream);

/* ---- DINO / DINOv2 ViT encoder (sdhip_vit.hip) -------------------------------
 * Replaces timm's VisionTransformer forward as the reference runs it
 * (scenedino/models/backbones/dino/vit.py:48-62,112-189 via DINOv2Encoder.forward,
 * dinov2_module.py:230-288): patch embedding, pre-LN blocks (qkv + softmax attention +
 * proj, GELU MLP, optional DINOv2 layer scale), final norm.  Residual stream fp32,
 * GEMM operands bf16, fp32 accumulation. */

enum sd_epilogue {
    SD_EPI_BF16 = 0,   /* out bf16 (M, ldo) = acc + bias                                  */
    SD_EPI_GELU = 1,   /* out bf16 = gelu_erf(acc + bias)           (timm Mlp fc1 + act)   */
    SD_EPI_F32 = 2,    /* out f32 = acc + bias                                             */
    SD_EPI_RESID = 3,  /* out f32 += gamma * (acc + bias)  (residual add, ls1/ls2 gamma)   */
    SD_EPI_QKV = 4,    /* scatter qkv columns into q (B,H,T,hd), k (B,H,Tp,hd),            */
                       /* vt (B,H,hd,Tp) bf16 (timm Attention reshape/permute)             */
    SD_EPI_PATCH = 5,  /* out f32 (B, patches+1, N): row b*(patches+1)+1+p = acc+bias+pos  */
    SD_EPI_SHUF = 6,   /* ConvTranspose2d(k, stride k): row m = input pixel (b, y, x),      */
                       /* column n = (dy k + dx) Cout + co -> out bf16 NHWC                 */
                       /* (B, in_h k, in_w k, Cout)[b, y k + dy, x k + dx, co] = acc + bias[n] */
    SD_EPI_NCHW = 7    /* out f32 NCHW (B, N, plane): row m = b * plane + p (plane = tokens) */
};

/* C = A (M, K) . W (N, K)^T (+ bias) with the epilogue above; A, W bf16 row-major
 * (W = nn.Linear weight layout), K % 32 == 0, lda % 8 == 0. */
typedef struct sd_gemm_args {
    const void *a; int64_t lda;
    const void *w;
    const float *bias;          /* (N) or NULL                                           */
    int64_t M, N, K;
    int32_t epi;
    void *out; int64_t ldo;     /* output / residual, element stride between rows        */
    const float *gamma;         /* SD_EPI_RESID layer scale (N) or NULL (= 1)            */
    void *q, *k, *vt;           /* SD_EPI_QKV destinations (k is its K output only);
                                 * SD_EPI_RESID: q (or NULL) = a bf16 (B, tokens - 1, N)
                                 * copy of the updated rows without each image's first
                                 * (class) token -- the timm intermediate-layer grid,
                                 * tokens_to_nhwc's output                                */
    int32_t tokens, heads, head_dim, tokens_pad;
    const float *pos;           /* SD_EPI_PATCH position embedding (patches+1, N)        */
    int32_t patches;
    /* residuals added by the BF16 / F32 epilogues: bf16 (M, N) row stride ldo, or NULL     */
    const void *res, *res2;
    /* implicit 3x3 convolution, padding 1 (conv != 0): a = NHWC bf16 input (B, H, W, Cin),
     * rows m = output pixels (B, OH, OW), k = (ky, kx, ci) (K = 9 Cin, Cin % 64 == 0),
     * w = (Cout, 3, 3, Cin); relu_in applies ReLU to the input as it is loaded (the
     * pre-activation of DPT's residual conv units) */
    int32_t conv, H, W, Cin, stride, OH, OW, relu_in;
    int32_t shuf_k, in_h, in_w; /* SD_EPI_SHUF geometry                                  */
} sd_gemm_args;

int sd_gemm(const sd_gemm_args *args, void *stream);

/* nn.LayerNorm(K, eps) fused into the prologue of a GEMM (timm Block: norm1 -> attn.qkv,
 * norm2 -> mlp.fc1, vit.py:112-189 over timm's VisionTransformer): out = EPI(LN(x) W^T + b)
 * for x (M, K) f32 rows, dense with row stride K (K = C in {384, 768}), W = args->w (N, K)
 * bf16; args->a is unused.  SD_EPI_QKV needs head_dim % 8 == 0 and tokens_pad % 8 == 0.
 * epi SD_EPI_QKV / SD_EPI_GELU / SD_EPI_BF16 with the sd_gemm fields they read.  The
 * normalised rows are the bf16 ones sd_layernorm would write (same arithmetic). */
int sd_ln_gemm(const sd_gemm_args *args, const float *x, const float *ln_w, const float *ln_b,
               float eps, void *stream);

/* softmax(q k^T * scale) v per (batch, head); q (B,H,T,64), k (B,H,Tp,64),
 * vt (B,H,64,Tp) bf16 with rows/columns T..Tp-1 zero; out (B, T, H*64) bf16.
 * tokens_pad (Tp) is any multiple of 64 >= tokens: it is the V^T row stride and the K plane
 * size only.  Like sd_attention_bwd, the kernels visit the keys below ceil64(tokens) and
 * mask those >= tokens, so a larger tokens_pad gives the same bits as the tight one.
 * head_dim == 64, B * heads <= 65535, scale finite and > 0 (the running maximum is taken on
 * the raw scores); anything else returns -1 before any launch. */
int sd_attention(const void *q, const void *k, const void *vt, int32_t B, int32_t heads,
                 int32_t tokens, int32_t tokens_pad, int32_t head_dim, float scale, void *out,
                 void *stream);

/* nn.LayerNorm(C, eps) over rows of x (rows, C) f32 -> out (rows, C) bf16 (out_f32 = 0,
 * the next GEMM's operand) or f32 (out_f32 = 1, the encoder's final norm). */
int sd_layernorm(const float *x, int64_t rows, int32_t C, const float *w, const float *b,
                 float eps, void *out, int32_t out_f32, void *stream);

/* The encoder's final norm into the DPT's last token grid (vit.py:188 over timm's
 * VisionTransformer.norm, then the prefix tokens dropped and the optional L2 normalisation
 * of dinov2_module.py:270-287): x (B, T, C) f32 rows -> out (B, npix, C) bf16 for tokens
 * n_prefix .. n_prefix + npix - 1 = sd_layernorm (out_f32 = 1) followed by
 * sd_tokens_to_nhwc, bit for bit, in one launch. */
int sd_layernorm_nhwc(const float *x, int32_t B, int32_t T, int32_t C, const float *w,
                      const float *b, float eps, int32_t n_prefix, int32_t npix, int32_t l2norm,
                      void *out, void *stream);

/* img (B,3,H,W) in [-1,1] -> normalised ((x/2+0.5 - mean)/std) im2col patches
 * (B*Np, Kp) bf16 (zero-padded columns >= 3 p p), and class-token rows of x (B, Np+1, C):
 * x[b,0,:] = cls + pos[0,:].  mean3/std3: HOST pointers (3). */
int sd_patchify(const float *img, int32_t B, int32_t H, int32_t W, int32_t p, int32_t Kp,
                const float *mean3, const float *std3, void *patches, const float *cls,
                const float *pos, float *x, int32_t C, void *stream);

/* x (B, T, C) f32 -> out (B, C, gh, gw): tokens n_prefix .. n_prefix+gh*gw-1 as a grid,
 * optionally L2-normalised over C (F.normalize, eps 1e-12). */
int sd_tokens_to_grid(const float *x, int32_t B, int32_t T, int32_t C, int32_t n_prefix,
                      int32_t gh, int32_t gw, int32_t l2norm, float *out, void *stream);

/* ---- DPT decoder pieces (sdhip_vit.hip; dpt_head.py:23-236) -------------------
 * The convolutions of the DPT head run through sd_gemm (1x1: plain GEMM; 3x3: conv = 1;
 * ConvTranspose2d(k, stride k): SD_EPI_SHUF; the last one writes NCHW f32 for the field
 * kernels: SD_EPI_NCHW).  Activations are NHWC bf16. */

/* x (B, T, C) f32 -> out (B, npix, C) bf16: tokens n_prefix .. n_prefix+npix-1, optionally
 * L2-normalised (the DPT inputs: ViT block outputs / normalised final tokens). */
int sd_tokens_to_nhwc(const float *x, int32_t B, int32_t T, int32_t C, int32_t n_prefix,
                      int32_t npix, int32_t l2norm, void *out, void *stream);

/* F.interpolate(scale_factor=2, mode="bilinear", align_corners=True) on NHWC bf16
 * (FeatureFusionBlock, dpt_head.py:157): in (B, H, W, C) -> out (B, 2H, 2W, C). */
int sd_upsample2x(const void *in, int32_t B, int32_t H, int32_t W, int32_t C, void *out,
                  void *stream);

/* ---- DPT decoder backward (sdhip_dpt_bwd.hip) ---------------------------------
 * The data gradients of the decoder's convolutions are sd_gemm calls on rotated /
 * transposed weight packs; these are the pieces the forward has no counterpart for. */

/* Weight and bias gradient of a convolution of the DPT head (3x3 padding 1, stride 1 or 2:
 * taps = 9; 1x1 / the GEMM of a ConvTranspose2d(k, stride k): taps = 1) from its NHWC bf16
 * input x (B, H, W, Cin) and output gradient dy (B, OH, OW, Cout), OH = (H - 1) / stride + 1:
 *   dw[co][tap Cin + ci] = sum_p dy[p][co] * im2col(x)[p][tap Cin + ci]   (tap = 3 ky + kx)
 *   db[co]               = sum_p dy[p][co]                                (db may be NULL)
 * in f32, dw in sd_gemm's packed weight order (Cout, ky, kx, ci).  relu_in: x is read
 * through the pre-activation ReLU, as sd_gemm's relu_in reads it.  The output pixels are
 * split into nparts contiguous parts (sd_conv_wgrad_parts: enough to fill the device) whose
 * f32 partial sums go to work (sd_conv_wgrad_work floats) and are added in part order: no
 * float atomics, the result is bit-identical from launch to launch.
 * Cin % 64 == 0, Cout % 8 == 0, all pointers 16-byte aligned; anything else returns -1
 * before any launch. */
typedef struct sd_conv_wgrad_args {
    const void *x, *dy;
    int32_t B, H, W, Cin, Cout, taps, stride, relu_in;
    int32_t nparts, pad; /* nparts: sd_conv_wgrad_parts (or any 1 .. ceil(B OH OW / 32)) */
    float *work;
    float *dw, *db;
} sd_conv_wgrad_args;

/* Parts sd_conv_wgrad should use for this shape on the current device (nparts is ignored),
 * and the f32 elements of work for args->nparts parts (nparts 0: for that default).
 * -1 on an invalid shape. */
int32_t sd_conv_wgrad_parts(const sd_conv_wgrad_args *args);
int64_t sd_conv_wgrad_work(const sd_conv_wgrad_args *args);
int sd_conv_wgrad(const sd_conv_wgrad_args *args, void *stream);

/* Adjoint of sd_upsample2x: gout (B, 2H, 2W, C) bf16 -> gin (B, H, W, C) bf16, every input
 * pixel summing its contributing output pixels in a fixed order (deterministic).
 * C % 8 == 0. */
int sd_upsample2x_bwd(const void *gout, int32_t B, int32_t H, int32_t W, int32_t C, void *gin,
                      void *stream);

/* out = (x > 0 ? g : 0) (+ res) over n bf16 elements (res may be NULL): the gradient through
 * a pre-activation ReLU, with the skip gradient of a residual unit added.  n % 8 == 0. */
int sd_relu_bwd(const void *x, const void *g, const void *res, int64_t n, void *out,
                void *stream);

/* ---- ViT encoder backward (sdhip_vit_bwd.hip) ----------------------------------
 * The training path of the native DINO / DINOv2 encoder (scenedino/models/backbones/dino/
 * vit.py:112-189 run with autograd when encoder_freeze is false, dinov2_module.py:176-183,
 * and optimised in its own Adam group, scenedino/training/trainer.py:561-573).  Linear data
 * gradients are sd_gemm calls on transposed weight packs and linear weight / bias gradients
 * are sd_conv_wgrad calls with taps = 1 (models/backbones/dino/vit_autograd.py); these are
 * the three operations the forward has no counterpart for.  No float atomics: a launch
 * repeated on the same inputs gives the same bits.  Added without an ABI bump (entry points
 * and structs only). */

/* Backward of sd_attention (head_dim 64) from the forward's operands: q (B, heads, tokens, 64),
 * k (B, heads, tokens_pad, 64), vt (B, heads, 64, tokens_pad), the forward output
 * ao (B, tokens, heads 64) and its gradient d_ao (same layout), all bf16.  Per (batch, head):
 *   P = softmax(scale Q K^T), dV = P^T dO, dP = dO V^T, D_i = sum_e dO_ie O_ie,
 *   dS = P o (dP - D), dQ = scale dS K, dK = scale dS^T Q
 * with S and P recomputed per 32 x 32 tile on v_mfma_f32_32x32x16_bf16 (f32 accumulation,
 * exp2 in the log2 domain); no tokens x tokens matrix reaches memory.  Three launches: the
 * softmax row statistics (log-sum-exp and D per query) into work, then one workgroup per
 * 32-key block summing dK / dV over all query tiles and one per 32-query tile summing dQ
 * over all key blocks, in registers -- no sum crosses a workgroup.
 * d_qkv (B tokens, 3 heads 64) bf16 rows, column which (heads 64) + head 64 + e (which =
 * 0 q, 1 k, 2 v): the inverse of the SD_EPI_QKV scatter, read as it lies by the qkv
 * GEMM's data and weight gradients.  Keys >= tokens are masked as the forward masks them,
 * only the first `tokens` rows are written, k and vt are only read.  tokens == 1: dq and dk
 * are exactly zero and dv = d_ao.
 * work: 2 B heads tokens floats.  head_dim == 64, tokens >= 1, tokens_pad >= tokens,
 * tokens_pad % 64 == 0, scale > 0, pointers 16-byte aligned; anything else returns -1
 * before any launch. */
typedef struct sd_attn_bwd_args {
    const void *q, *k, *vt, *ao, *d_ao;
    void *d_qkv;
    float *work;
    int32_t B, heads, tokens, tokens_pad, head_dim;
    float scale;
} sd_attn_bwd_args;
int sd_attention_bwd(const sd_attn_bwd_args *args, void *stream);

/* Backward of sd_layernorm: x (rows, C) f32 is the LayerNorm input (mean and rstd are
 * recomputed as the forward computes them), w its weight, dy (rows, C) the gradient of its
 * output, bf16 or f32 (dy_f32).  dx (rows, C) f32 = rstd (g - mean(g) - xhat mean(g xhat)),
 * g = dy w, written, or added to what dx holds (accumulate: the residual-stream gradient).
 * dw[c] = sum_rows dy xhat, db[c] = sum_rows dy, f32 (both may be NULL): the rows are split
 * into nparts contiguous parts (sd_layernorm_bwd_parts(rows), or any count >= 1) whose
 * partial sums go to work (2 nparts C floats) and are added in a fixed order (eight contiguous
 * runs of parts, each in part order, then the eight sums in order).
 * C <= 1024, C % 4 == 0 (sd_layernorm's domain), pointers 16-byte aligned; anything else
 * returns -1 before any launch. */
typedef struct sd_ln_bwd_args {
    const float *x, *w;
    const void *dy;
    int64_t rows;
    int32_t C, dy_f32, accumulate, nparts;
    float eps;
    int32_t pad;
    float *dx, *work, *dw, *db;
} sd_ln_bwd_args;
int32_t sd_layernorm_bwd_parts(int64_t rows);
int sd_layernorm_bwd(const sd_ln_bwd_args *args, void *stream);

/* du = dh gelu'(u) over n bf16 elements, exact-erf GELU (SD_EPI_GELU's):
 * gelu'(u) = Phi(u) + u phi(u), evaluated in f32.  n % 8 == 0, 16-byte aligned. */
int sd_gelu_bwd(const void *u, const void *dh, int64_t n, void *du, void *stream);

/* ---- transform_expand backward (sdhip_expand_bwd.hip) ---------------------------
 * Backward of sd_seg_query's dino_full = MlpDimReduction.transform_expand
 * (scenedino/models/backbones/dino/dim_reduction.py:22-25), which the reference's training
 * step differentiates right after the render (scenedino/training/trainer.py:288,441-445) and
 * whose linear_in / linear_out sit in its first Adam group (trainer.py:565-568).  Nothing is
 * saved by the forward; per 32-row tile (one wave) the kernel recomputes
 *   h = relu(W1 x + b1), e = W2 h + b2, n = |e|, y = e / max(n, 1e-12)
 * and forms
 *   de = (dy - y (y . dy)) / n  (n >= 1e-12; dy / 1e-12 below, torch's clamp_min branch),
 *   dh = (W2^T de) o [h > 0],  dx = W1^T dh.
 * Products on v_mfma_f32_32x32x16_bf16 with f32 accumulation; n, y . dy and de in f32.  The
 * weight gradients dW2 = de^T h, db2 = sum de, dW1 = dh^T x, db1 = sum dh are sd_conv_wgrad
 * calls with taps = 1 on the bf16 rows written here.  No atomics: a repeated launch gives
 * the same bits.  Added without an ABI bump (an entry point and a struct only).
 * h names the record the forward used (its d_in 64, d_latent 128, d_full % 32 == 0 are the
 * domain); the operands below are plain row-major copies of the same bf16 weights
 * (scenedino_amd/seg_pack.py PackedExpandBwd), independent of the record's frag_layout.
 * P >= 1 (ragged last tiles are masked), all pointers 16-byte aligned; anything else
 * returns -1 before any launch. */
typedef struct sd_expand_bwd_args {
    const void *x;         /* (P, 64) codes, x_dtype SD_F32 or SD_BF16                    */
    const float *dy;       /* (P, d_full) f32 gradient of dino_full                       */
    const void *w1, *w2;   /* bf16 row-major W1 (128, 64), W2 (d_full, 128)               */
    const void *w1t, *w2t; /* bf16 row-major W1^T (64, 128), W2^T (128, d_full)           */
    const float *b1, *b2;  /* f32 (128), (d_full)                                         */
    int64_t P;
    int32_t x_dtype, pad;
    float *dx;             /* (P, 64) f32                                                 */
    /* bf16 rows for the weight gradients, each may be NULL (not wanted): h (P, 128),
     * de (P, d_full), dh (P, 128), xb (P, 64) = bf16(x) (written for SD_F32 x only)    */
    void *h, *de, *dh, *xb;
} sd_expand_bwd_args;
int sd_expand_bwd(const sd_expand_bwd_args *args, const sd_seg_head *h, void *stream);

/* ---- STEGO head training (sdhip_stego_train.hip, sdhip_probe.hip) ----------------
 * The downstream stage (training_type: downstream_training) trains SemanticHead on a frozen
 * feature field (scenedino/downstream_head/semantic_head.py:122-235).  Its inputs are always
 * detached, so StegoClusterHead (:285-305) needs weight gradients only.  Added without an ABI
 * bump (entry points and structs only).
 *
 * sd_stego_train_fwd, per row of x (M, d_in) f32, un-normalised (Dropout2d as per-group column
 * scales m_lin / m_non (n_groups, 64), row r using group r / rows_per_group; NULL: ones):
 *   xh  = x / max(|x|, 1e-10)     (normalize != 0; x itself otherwise: rows that were
 *                                  normalised and then dropped out, forward_training's crops)
 *   lin = Wl xh + bl,  mid = relu(Wn1 xh + bn1),  non = Wn2 mid + bn2
 *   e   = m_lin o lin + m_non o non,   y = e / max(|e|, 1e-10)
 * on v_mfma_f32_32x32x16_bf16 with f32 accumulation.  y (M, 64) f32 is written; xh, mid (bf16
 * (M, d_in)) and e (f32 (M, 64)) are saved where their pointer is not NULL (all NULL: the
 * forward-only pass; y does not depend on what is saved).
 * sd_stego_train_bwd, from dy (M, 64) f32 and the saved e, mid:
 *   n = |e|,  de = (dy - y (y . dy)) / n   (n < 1e-10: dy / 1e-10, the clamp branch as
 *   sd_expand_bwd takes it),  dlin = m_lin o de,  dnon = m_non o de,
 *   dmid = (Wn2^T dnon) o [mid > 0]
 * written as bf16 rows dlin, dnon (M, 64), dmid (M, d_in), each may be NULL (not wanted).  The
 * six parameter gradients are sd_conv_wgrad calls with taps = 1 on those rows and xh / mid.
 * No input gradient, no atomics: a repeated launch gives the same bits.  Ragged last tiles are
 * masked.  M >= 1, d_in 384 or 768 (mid channels = d_in), d_code 64, pointers 16-byte
 * aligned; anything else returns -1 before any launch. */
typedef struct sd_stego_train_args {
    const float *x;              /* (M, d_in) f32 (forward)                                  */
    const void *wl, *wn1, *wn2;  /* bf16 row-major Wl (64, d_in), Wn1 (d_in, d_in), Wn2 (64, d_in) */
    const void *wn2t;            /* bf16 row-major Wn2^T (d_in, 64) (backward, with dmid)    */
    const float *bl, *bn1, *bn2; /* f32 (64), (d_in), (64)                                   */
    const float *m_lin, *m_non;  /* f32 (n_groups, 64) or NULL                               */
    int64_t M, rows_per_group, n_groups;
    int32_t d_in, d_code;
    int32_t normalize, pad;      /* normalize 0: xh = x as given (rows the caller normalised) */
    float *y;                    /* (M, 64) f32 (forward out)                                */
    void *xh, *mid;              /* bf16 (M, d_in): forward out (may be NULL); mid backward in */
    float *e;                    /* (M, 64) f32: forward out (may be NULL), backward in      */
    const float *dy;             /* (M, 64) f32 (backward)                                   */
    void *dlin, *dnon, *dmid;    /* bf16 (M, 64), (M, 64), (M, d_in) (backward out)          */
} sd_stego_train_args;
int sd_stego_train_fwd(const sd_stego_train_args *args, void *stream);
int sd_stego_train_bwd(const sd_stego_train_args *args, void *stream);

/* One pass of KMeansParamHead._kmeans_cosine (semantic_head.py:361-373) and its loss
 * statistics over x (N, d), SD_F32 or SD_BF16, with optional column scales m (n_groups, d)
 * (row r using group r / rows_per_group), centres (K, d) f32 already L2-normalised, optional
 * row weights w (N):
 *   xh_i = (x_i o m) / max(|x_i o m|, 1e-12),  label_i = argmax_k xh_i . c_k (lowest index on
 *   ties),  S_k = sum_{label_i = k} w_i xh_i (f32),  counts_k = #{label_i = k}.
 * Scores on v_mfma_f32_32x32x16_bf16 (centres as hi + lo bf16 halves); S is summed in f32 from
 * the unrounded rows, per workgroup into work (sd_cluster_probe_work floats) and then in
 * workgroup order: no atomics, a repeated launch gives the same bits.  The reference's loss is
 * -(1/N) sum_k c_k . S_k with S held constant.
 * N >= 1, 64 <= d <= 768, d % 64 == 0, 1 <= K <= 32, pointers 16-byte aligned; anything else
 * returns -1 before any launch. */
typedef struct sd_cluster_probe_args {
    const void *x;
    const float *m, *centres, *w;
    int64_t N, rows_per_group, n_groups;
    int32_t d, K, x_dtype, pad;
    float *work;
    int32_t *labels; /* (N)    */
    float *S;        /* (K, d) */
    int32_t *counts; /* (K)    */
} sd_cluster_probe_args;
int64_t sd_cluster_probe_work(int64_t N, int32_t d, int32_t K);
int sd_cluster_probe(const sd_cluster_probe_args *args, void *stream);

/* One pass of LinearHead (semantic_head.py:460-477) behind forward_training's _norm and Dropout2d
 * (sdhip_linear_probe.hip): logits, argmax, cross-entropy and the gradients of W and b over the
 * detached rows x (N, d), SD_F32 or SD_BF16, with optional column scales m (n_groups, d) (row r
 * using group r / rows_per_group), W (C, d) f32, b (C) f32, optional targets (N) int64.  Added
 * without an ABI bump (entry points and a struct only).
 *   xh_i = (normalize ? x_i / max(|x_i|, 1e-10) : x_i) o m   (normalised first, masked second:
 *   unlike sd_cluster_probe),  z_i = W xh_i + b,  pred_i = argmax_k z_ik (lowest index on ties);
 *   for rows with 0 <= target_i < C (anything else, e.g. -1, is ignored):
 *   l_i = logsumexp(z_i) - z_i[target_i] (max-subtracted),  g_i = softmax(z_i) - onehot(target_i);
 *   loss_sum = sum l_i,  n_valid = #valid,  gW = sum g_i xh_i^T (C, d),  gb = sum g_i (C).
 * Logits on v_mfma_f32_32x32x16_bf16 (W as hi + lo bf16 halves, rows rounded to bf16 in an LDS
 * tile); the rows are read once, gW is summed in f32 from that tile in row order.  Per-workgroup
 * partials go to work (sd_linear_probe_work floats) and are added in workgroup order: no
 * atomics, a repeated launch gives the same bits.  A zero row with normalize gives z = b.
 * target NULL: pred only, and every other output pointer must be NULL.  gW and gb are both NULL
 * (no gradient) or both set; row_loss (N, 0 on ignored rows) is optional.
 * N >= 1, 64 <= d <= 768, d % 64 == 0, 1 <= C <= 32, pointers 16-byte aligned; anything else
 * returns -1 before any launch. */
typedef struct sd_linear_probe_args {
    const void *x;
    const float *m, *W, *b;
    const int64_t *target; /* (N) or NULL */
    int64_t N, rows_per_group, n_groups;
    int32_t d, C, x_dtype, normalize;
    float *work;
    int32_t *pred;    /* (N)                 */
    float *loss_sum;  /* (1)                 */
    int32_t *n_valid; /* (1)                 */
    float *gW, *gb;   /* (C, d), (C) or NULL */
    float *row_loss;  /* (N) or NULL         */
} sd_linear_probe_args;
int64_t sd_linear_probe_work(int64_t N, int32_t d, int32_t C);
int sd_linear_probe(const sd_linear_probe_args *args, void *stream);

/* ---- first-stage ReconstructionLoss (sdhip_recon_loss.hip) -----------------------
 * scenedino/losses/reconstruction_loss.py:175-356 under training/loss/scenedino.yaml's options,
 * forward and backward, on patch-flattened tensors (P = n * pc patches of h x w pixels).  Added
 * without an ABI bump (entry points and a struct only).
 *   rgb term     per pixel and view: 0.85 mean_c clamp(1 - SSIM, 0, 1) / 2 + 0.15 mean_c |rgb -
 *                rgb_gt| on zero-padded 3 x 3 Gaussian statistics (window 0.0947 / 0.1183 /
 *                0.1478, C1 = 0.01^2, C2 = 0.03^2); minimum over the nv views; zero where the
 *                policy marks the pixel invalid (SD_RL_POLICY_WEIGHT: every view's sum_k invalid
 *                * weights > 0.9; _STRICT: every view has an invalid > 0.5; _NONE); mean over
 *                all P h w pixels.
 *   cosine term  nanmean over the R rows of 1 - cos(T (dino_down + dino_artifacts), T dino_gt),
 *                each norm clamped at 1e-8.
 *   depth term   u = (1 / clamp(depth, 1e-3, 80)) / its patch mean; mean over pixels of
 *                |u - u_right| exp(-|d rgb_gt|_right) + |u - u_down| exp(-|d rgb_gt|_down), |d
 *                rgb_gt| the channel mean.  depth patch p pairs with rgb_gt patch p: the caller
 *                passes the order it wants paired (the reference pairs (pc, n) with (n, pc)).
 *   dino term    the same with mean_c |d dino| and exp(-25 |d rgb_gt|).
 *   rec = rgb lambda_coarse + cosine lambda_coarse lambda_dino + depth lambda_depth + dino
 *         lambda_dsmooth, a regulariser that is exactly zero left out.
 * A term whose input pointer is NULL (depth; dino; dino_down) is not computed and reads 0.
 * sd_recon_loss_fwd writes rec (1 float), terms (4 floats: rgb, cosine, depth, dino) and the
 * state the backward reads, each where its pointer is not NULL: sel (P h w int32: bit v set if
 * view v attains the minimum, bit 8 set if the pixel is valid), edge (P h w 2: the DINO term's
 * right / down weights), dmean (P: the patch means of 1 / clamp(depth)), count (1: rows the
 * nanmean kept).  work holds sd_recon_loss_work(P, C, R) floats (C = 0 without dino, R = 0
 * without dino_down); partial sums are added in index order, no atomics: a repeated launch
 * gives the same bits.  Two launches.
 * sd_recon_loss_bwd reads the upstream gradient of rec from device memory (g_rec, 1 float) and
 * writes each of d_rgb (P, h, w, nv, 3), d_depth (P, h, w), d_dino (P, h, w, C) in dino_dtype,
 * d_down (R, Cd) whose pointer is not NULL, in one launch (none if all are NULL).  weights and
 * invalid only pass through comparisons and get no gradient.
 * Domain: 2 <= h, w <= 16, 1 <= nv <= 8, C and Cd % 64 == 0 and <= 768, f32 tensors (dino f32 or
 * bf16), pointers 16-byte aligned; anything else returns -1 before any launch. */
enum { SD_RL_POLICY_WEIGHT = 0, SD_RL_POLICY_STRICT = 1, SD_RL_POLICY_NONE = 2 };
typedef struct sd_recon_loss_args {
    const float *rgb;            /* (P, h, w, nv, 3)                                        */
    const float *rgb_gt;         /* (P, h, w, 3)                                            */
    const float *invalid;        /* (P, h, w, K, nv); may be NULL with SD_RL_POLICY_NONE    */
    const float *weights;        /* (P, h, w, K); SD_RL_POLICY_WEIGHT only                  */
    const float *depth;          /* (P, h, w) or NULL                                       */
    const void *dino;            /* (P, h, w, C) dino_dtype or NULL                         */
    const float *dino_down;      /* (R, Cd) or NULL                                         */
    const float *dino_gt;        /* (R, Cd)                                                 */
    const float *dino_artifacts; /* (R, Cd) or NULL                                         */
    int64_t P, R;
    int32_t h, w, nv, K, C, Cd, dino_dtype, policy;
    float lambda_coarse, lambda_dino, temperature, lambda_depth, lambda_dsmooth, pad;
    float *work;                 /* sd_recon_loss_work floats                               */
    float *rec, *terms;          /* forward out: (1), (4)                                   */
    int32_t *sel;                /* state: forward out, backward in                         */
    float *edge, *dmean, *count;
    const float *g_rec;          /* backward: upstream gradient of rec (1)                  */
    float *d_rgb, *d_depth;      /* backward out, each may be NULL                          */
    void *d_dino;
    float *d_down;
} sd_recon_loss_args;
int64_t sd_recon_loss_work(int64_t P, int32_t C, int64_t R);
int sd_recon_loss_fwd(const sd_recon_loss_args *args, void *stream);
int sd_recon_loss_bwd(const sd_recon_loss_args *args, void *stream);

/* ---- downstream-stage STEGO correlation loss (sdhip_stego_corr.hip) ---------------
 * Replaces the six correlation tensors of scenedino/downstream_head/semantic_head.py:181-188,
 * 268-270 and their reduction in scenedino/losses/stego_loss.py:40-46,71-79 (forward and
 * backward) without a (nc, P, Q) tensor in memory.  Added without an ABI bump (entry points and
 * a struct only).
 * Up to three pairs share the A side: dino_a (nc, P, d) and stego_a (nc, P, 64), un-normalised.
 * Pair i has partner rows dino_b[i] (nc, Q, d) and stego_b[i] (nc, Q, 64); a pair with both
 * NULL is the self pair (B = A, b = a, Q = P; at most one).  With x^ = x / max(|x|, 1e-10),
 * D = A^ B^T and S = a^ b^T per crop, N = nc P Q:
 *   loss[i] = -weight[i] / N sum max(S, 0) (D' - shift[i])
 *   D' = D (pointwise 0) or D - r[n, p] + g with r the mean of D over q and g the mean of r
 *   (pointwise 1: the reference removes the row means in place and restores the global mean).
 * D and S are bf16 MFMA products of the rounded normalised rows with f32 accumulation.
 * sd_stego_corr_fwd writes loss (3 floats, 0 for pairs >= n_pairs) and leaves the normalised
 * rows and centring terms in work for sd_stego_corr_bwd, which reads the upstream gradient of
 * every loss from device memory (up, 3 floats) and writes d loss / d stego_a into d_a (nc, P, 64)
 * and d loss / d stego_b[i] into d_b[i] (nc, Q, 64), each optional; the self pair's two sides
 * both land in d_a.  The DINO rows get no gradient.  No atomics, sums in a fixed order: a
 * repeated call gives the same bits.
 * Domain: d in {384, 768}, code_dim 64, 1 <= P, Q <= 4096, nc >= 1 with nc max(P, Q) <= 2^24,
 * 1 <= n_pairs <= 3, DINO rows SD_F32 or SD_BF16 (dino_dtype), code rows f32, contiguous,
 * 16-byte aligned; work holds work_bytes >= sd_stego_corr_work(...) bytes (has_self: one of the
 * pairs is the self pair).  Anything else returns -1 with sd_last_error() set. */
typedef struct sd_stego_corr_args {
    const void *dino_a;        /* (nc, P, d)                                              */
    const void *dino_b[3];     /* (nc, Q, d) or NULL                                      */
    const float *stego_a;      /* (nc, P, 64)                                             */
    const float *stego_b[3];   /* (nc, Q, 64) or NULL                                     */
    float weight[3], shift[3];
    int64_t nc;
    int32_t P, Q, d, code_dim, n_pairs, dino_dtype, pointwise, pad;
    void *work;
    int64_t work_bytes;
    float *loss;               /* fwd: (3)                                                */
    const float *up;           /* bwd: (3) upstream gradients                             */
    float *d_a;                /* bwd: (nc, P, 64) or NULL                                */
    float *d_b[3];             /* bwd: (nc, Q, 64) or NULL                                */
} sd_stego_corr_args;
int64_t sd_stego_corr_work(int64_t nc, int32_t P, int32_t Q, int32_t d, int32_t n_pairs,
                           int32_t has_self);
int sd_stego_corr_fwd(const sd_stego_corr_args *args, void *stream);
int sd_stego_corr_bwd(const sd_stego_corr_args *args, void *stream);

/* ---- multi-scale-crop DINO targets (sdhip_msc.hip) --------------------------------
 * MultiScaleCropGT_kornia.forward_chunk after the gt encoder
 * (scenedino/models/backbones/dino/upsampler.py:170-181 with _accumulate_predictions :81-130
 * and _affine_transform_valid_pixels :56-79), the loss targets of mode "upsample-gt".  Added
 * without an ABI bump (an entry point and a struct only).
 * feat holds the gt encoder's final token grids of the V views of each image in the
 * reference's order: 0..V-3 augmented, V-2 the horizontally flipped image, V-1 the image.
 * T[b,k] maps pixel coordinates of the image to pixel coordinates of augmented view k (the
 * matrix the reference inverts at :103 and warp_perspective inverts back).  Per pixel (u, v)
 * and channel, with U_k the grid of view k upsampled to (H, W) by F.interpolate(bilinear,
 * align_corners=False) (:170):
 *   view V-1 gives U(u, v), view V-2 gives U(W-1-u, v) (:116), both always valid (:124);
 *   view k < V-2: (x, y) = (p0 / p2, p1 / p2) of p = T_k (u, v, 1)^T, the zero-padded bilinear
 *   sample of U_k at (x, y) (:105-110), valid iff 0 <= rint(x) <= W-1 and 0 <= rint(y) <= H-1
 *   (the nearest-mode warp of a ones mask, :69-78);
 *   out = (sum over valid views) / (number of valid views)  (:126-130), then with normalize
 *   divided by its L2 norm over the C channels, no epsilon (:181).
 * Tap indices and weights are computed once per pixel; one launch, no atomics, sums in a fixed
 * order: a repeated launch gives the same bits.
 * Domain: B >= 1, 2 <= V <= 8, 1 <= C <= 1024, hp, wp, H, W >= 1, hp wp < 2^31, pointers
 * 16-byte aligned (T may be NULL at V = 2); anything else returns -1 before any launch. */
typedef struct sd_msc_gt_args {
    const float *feat;  /* (B, V, C, hp, wp) f32                                             */
    const float *T;     /* (B, V-2, 3, 3) f32                                                */
    float *out;         /* (B, C, H, W) f32                                                  */
    int32_t B, V, C, hp, wp, H, W;
    int32_t normalize;  /* != 0: divide by the channel L2 norm                               */
} sd_msc_gt_args;
int sd_msc_gt(const sd_msc_gt_args *args, void *stream);

/* ---- downstream-stage 3-D surface crops (sdhip_crop3d.hip) ------------------------
 * BTSDownstreamWrapper.sample_3d_crop (scenedino/training/trainer_downstream.py:216-292)
 * around the field query.  Added without an ABI bump (entry points and structs only).
 *
 * sd_crop3d_centres, per frame f (one workgroup each; view 0 of depth, poses, projs):
 *   sel      = {d : d < z_far}, m = |sel|
 *   limits[i] = torch.quantile(sel, i / n_crops), linear interpolation: exact order statistics
 *              at floor / ceil of the f32 rank (float)(i / n_crops) * (float)(m - 1), ATen's
 *              lerp kept inside [s_floor, s_ceil]; limits[0] / limits[n_crops] the exact
 *              minimum / maximum.  m = 0: NaN, and every crop of the frame has count 0.
 *   count[i]  = #{pixels : limits[i] < d < limits[i+1]}
 *   pixel[i]  = (row, col) of the r-th such pixel in row-major order, r = min((int)(u_pick[i] *
 *              (float)count[i]), count[i] - 1); (-1, -1) where count[i] = 0
 *   centre[i] = camera centre + unit ray of the pixel (as sd_gen_rays) * d[pixel], product and
 *              sum rounded separately
 *   points[i] = centre[i] + shift[i] (S rows); zeros where count[i] = 0
 * Integer histograms and counts only: a repeated call gives the same bits.
 * Domain: n, S >= 1, 1 <= n_crops <= 8, h w <= 2^24; contiguous f32 operands; the strides are
 * the elements between two frames' view 0.  Anything else returns -1. */
typedef struct sd_crop3d_args {
    const float *depth;    /* frame f at depth + f depth_stride: (h, w)                      */
    const float *poses;    /* frame f at poses + f pose_stride: (4, 4) camera to world        */
    const float *projs;    /* frame f at projs + f proj_stride: (3, 3) normalised intrinsics  */
    const float *u_pick;   /* (n, n_crops) in [0, 1)                                          */
    const float *shift;    /* (n, n_crops, S, 3)                                              */
    float *limits;         /* (n, n_crops + 1)                                                */
    int32_t *count;        /* (n, n_crops)                                                    */
    int32_t *pixel;        /* (n, n_crops, 2)                                                 */
    float *centre;         /* (n, n_crops, 3)                                                 */
    float *points;         /* (n, n_crops, S, 3)                                              */
    int64_t depth_stride, pose_stride, proj_stride;
    int32_t n, h, w, n_crops, S;
    float z_far;
} sd_crop3d_args;
int sd_crop3d_centres(const sd_crop3d_args *args, void *stream);

/* sd_crop3d_compact: crop c of sigma (C, S) / codes (C, S, D) is kept iff crop_ok[c] > 0 and
 * #{sigma[c] > thr} > n_samples (both strict).  Kept crops keep their order: slot[c] is the
 * output index (-1: dropped) and n_valid their number.  Output crop slot[c] holds the first
 * n_samples rows of crop c with sigma > thr, in order: the code rows copied bit for bit and
 * occ_out = 1 - exp(-sigma).  Output crops >= n_valid are zero.
 * Domain: 1 <= C <= 64, S, D >= 1, 1 <= n_samples <= 4096, codes SD_F32 or SD_BF16 with rows of
 * whole 4-byte words, codes / codes_out 16-byte aligned.  Anything else returns -1. */
typedef struct sd_crop3d_compact_args {
    const float *sigma;      /* (C, S)                                                        */
    const void *codes;       /* (C, S, D)                                                     */
    const int32_t *crop_ok;  /* (C): sd_crop3d_centres' count                                 */
    void *codes_out;         /* (C, n_samples, D), the type of codes                          */
    float *occ_out;          /* (C, n_samples)                                                */
    int32_t *n_valid;        /* (1)                                                           */
    int32_t *slot;           /* (C)                                                           */
    int32_t C, S, D, n_samples, codes_dtype;
    float thr;
} sd_crop3d_compact_args;
int sd_crop3d_compact(const sd_crop3d_compact_args *args, void *stream);

/* ---- training path: fused ResnetFC MLP (sdhip_mlp.hip) ---------------------- */

/* ResnetFC(n_blocks=0) forward / backward of the training path under autocast
 * (scenedino/models/prediction_heads/resnetfc.py:135-203, bts.py:516-541 softplus,
 * scenedino/training/base_trainer.py:223,251 with_amp), on the sd_field_gather rows
 * x (N, ldx) = [feat (C) | code | 1] in dtype (SD_F16 / SD_BF16); columns kx .. ldx-1 are
 * padding whose contents never reach a result.  Fragments pre-packed by the host
 * (scenedino_amd/mlp_pack.py PackedTrainMLP documents the maps).
 * sd_mlp_train_fwd: h (N, 136) dtype = [relu(W_in x + b_in) | 1 | 0..], sigma (N) f32 =
 *   softplus(out_0), dino (N, D) f32 = out_1..D.
 * sd_mlp_train_bwd: from d_sigma (N), d_dino (N, D) f32: dy (N, 72) dtype = [d dino | d out_0
 *   | 0..], dh (N, 128) dtype = d relu-input, dx (N, lddx) dx_dtype = [dH W_in[:, :C] | 0..];
 *   the weight gradients are dh^T x and dy^T h (caller's GEMMs).  D <= 64, C % 32 == 0.
 *   Fused grid_sample backward (dgrid != NULL; replaces dx + sd_field_gather_bwd, bts.py:
 *   299-309): dX[:, :C], rounded to dtype like the autocast Linear's input gradient, is
 *   scattered with the forward gather's bilinear weights straight into the NHWC f32 grid
 *   gradient dgrid (N / P, Hf, Wf, C) (f32 atomics; the rows never reach HBM).  xyz (N, 3)
 *   are the points, P the points per encoder frame, cam_f the (N / P) encoder camera
 *   records; dx may then be NULL.  (N / P) * Hf * Wf * C < 2^31. */
typedef struct sd_mlp_train_args {
    const void *x;
    int64_t N;
    int32_t ldx, kx;       /* row length of x / dx, used columns (d_in + 1)              */
    int32_t dtype, D, C;
    int32_t lddx;          /* row length of dx (C: feature columns only; ldx: + zero columns) */
    int32_t dx_dtype;      /* SD_F32, or dtype: 16-bit dx rows (the autocast gradient dtype)  */
    int32_t pad;
    const void *w1f;       /* [4][ceil(kx/16)][64][8]  [W_in | b_in] A fragments          */
    const void *w2f;       /* [ceil((D+1)/32)][8][64][8] W_out B fragments (dino, out_0)   */
    const float *b_out;    /* (1 + D)                                                     */
    void *h;
    float *sigma, *dino;
    const float *d_sigma, *d_dino;
    const void *wtf;       /* [4][ceil((D+1)/16)][64][8] W_out^T A fragments              */
    const void *wxf;       /* [C/32][8][64][8] W_in B fragments (dX)                       */
    void *dy, *dh;
    void *dx;
    const float *xyz;      /* fused scatter (dgrid != NULL): (N, 3) points                  */
    const float *cam_f;    /* (N / P, SD_CAM_WORDS) encoder camera records                 */
    float *dgrid;          /* (N / P, Hf, Wf, C) f32, accumulated into; NULL: write dx       */
    int64_t P;
    int32_t Hf, Wf;
} sd_mlp_train_args;

/* Weight gradients of the training MLP: part[w] (Ma_pad x Nb_pad f32, pads to 32) =
 * sum over workgroup w's contiguous range of the N points of A[p]^T B[p], A (N, lda) and
 * B (N, ldb) 16-bit rows of which the first Ma / Nb columns are used (dW1 = dH^T X,
 * dW_o = dY^T [H | 1]); the caller sums the nparts partials.  Ma <= 128, Nb <= 320,
 * both multiples of 8. */
typedef struct sd_wgrad_args {
    const void *a, *b;
    int64_t N;
    int32_t lda, ldb, Ma, Nb, dtype, nparts;
    float *part;           /* (nparts, Ma_pad, Nb_pad)                                    */
} sd_wgrad_args;

int sd_wgrad(const sd_wgrad_args *args, void *stream);

/* Both weight gradients of the training MLP in one pass over the rows sd_mlp_train_fwd /
 * _bwd leave (the Linear backward of resnetfc.py:135-203 under autocast): dW1 = dh^T x
 * (x: ldx-strided rows, kx = d_in + 1 used columns, the ones column giving db_in) and
 * dW_o = dy^T [h | 1] (dy: (N, 72) = [d dino | d out_0 | 0..], h: (N, 136)).  The outputs
 * are the f32 gradients in the parameters' layout: dw_in (128, kx - 1), db_in (128),
 * dw_out (1 + D, 128) and db_out (1 + D) with row 0 = out_0 (sigma), rows 1..D = dino --
 * resnetfc.py's lin_out rows.  work: sd_mlp_train_wgrad_work(nparts) f32 of scratch for
 * the nparts partial sums (deterministic: fixed summation order).  kx <= 320, kx % 8 == 0,
 * D <= 64, D % 8 == 0. */
typedef struct sd_mlp_wgrad_args {
    const void *x, *dh, *dy, *h;
    int64_t N;
    int32_t ldx, kx, D, dtype, nparts, pad;
    float *work;
    float *dw_in, *db_in, *dw_out, *db_out;
} sd_mlp_wgrad_args;

int64_t sd_mlp_train_wgrad_work(int32_t nparts);
int sd_mlp_train_wgrad(const sd_mlp_wgrad_args *args, void *stream);

int sd_mlp_train_fwd(const sd_mlp_train_args *args, void *stream);
int sd_mlp_train_bwd(const sd_mlp_train_args *args, void *stream);

/* ---- training loss: PatchSalienceDownsampler (sdhip_down.hip) -------------- */

/* PatchSalienceDownsampler.forward_patches (scenedino/models/backbones/dino/downsampler.py:
 * 82-98): N patches of S = ph*pw feature vectors (C channels, x (N, S, C) f32): salience
 * s = w.x + b (1x1 conv), weights a = softmax(s * pw + pb) over the patch, out = sum a x,
 * L2-normalised if normalize.  sd_salience_fwd writes out (N, C), sal (N, S) and wmap (N, S)
 * (either may be NULL) and ynorm (N) (|sum a x|, needed by the backward when normalising:
 * written and read only with normalize != 0, and may be NULL otherwise).
 * sd_salience_bwd takes g_out (N, C) and optionally g_sal / g_wmap (N, S), reads x, out,
 * sal, wmap, ynorm, and writes gx (N, S, C) plus per-patch partial parameter gradients
 * gw_part (N, C), gpw_part / gpb_part (N, S), gb_part (N) (the caller sums over N).
 * S <= 1024, C <= 1024, C % 4 == 0; x, w, out, g_out, gx, gw_part 16-byte aligned. */
typedef struct sd_salience_args {
    const float *x;
    const float *w;        /* conv.weight (C)                                              */
    const float *b;        /* conv.bias (1, device; NULL: no bias)                          */
    const float *pw;       /* patch_weight (S)                                             */
    const float *pb;       /* patch_bias (S)                                               */
    int64_t N;
    int32_t S, C, normalize, pad;
    float *out;            /* forward output; backward input                               */
    float *sal;            /* forward output; backward input                               */
    float *wmap;           /* forward output; backward input                               */
    float *ynorm;          /* forward output; backward input                               */
    const float *g_out, *g_sal, *g_wmap;
    float *gx, *gw_part, *gpw_part, *gpb_part, *gb_part;
} sd_salience_args;

int sd_salience_fwd(const sd_salience_args *args, void *stream);
int sd_salience_bwd(const sd_salience_args *args, void *stream);

/* ---- SSCBench scoring (sdhip_ssc.hip) --------------------------------------- */

/* Camera field-of-view mask of the voxel grid (uint8 0/1, flat index as sd_voxel_points):
 * generate_point_grid's fov_mask (sscbench/point_utils.py:17-82, get_fov_mask :6-15) with
 * TSDFVolume.cam2pix (sscbench/fusion.py:222-232): fp64 camera points, pixel =
 * round-half-even(x fx / z + cx) with fx, fy, cx, cy the f32-rounded intrinsics, inside
 * [0, img_w) x [0, img_h) and z > 0.  origin (3), T (12: rows 0..2 of the 4x4) and cam_k
 * (9, row-major 3x3) are HOST pointers read during the call. */
int sd_voxel_fov(const double *origin, double vox, int64_t nx, int64_t ny, int64_t nz,
                 const double *T, const double *cam_k, int img_w, int img_h, uint8_t *fov_out,
                 void *stream);

/* Scoring configuration of sd_ssc_confusion (HOST struct, read during the call). */
typedef struct sd_ssc_args {
    float sigma_cutoff;          /* SIGMA_CUTOFF (evaluate_model_sscbench.py:57): 0.2         */
    int32_t additional_invalids; /* USE_ADDITIONAL_INVALIDS (:52)                            */
    int32_t inv_zmax;            /* identify_additional_invalids' height cut (:821): 7        */
    int32_t n_sizes;             /* evaluation ranges (SIZES, :49), at most 4                 */
    int32_t crop_x[4];           /* range s keeps x in [0, crop_x[s]) ...                     */
    int32_t crop_y0[4];          /* ... and y in [crop_y0[s], crop_y1[s]) (:496-501)          */
    int32_t crop_y1[4];
    int32_t n_pred_labels;       /* classes of the prediction (19 cityscapes classes)         */
    uint8_t pred_lut[256];       /* cityscapes_to_label (label_maps.yaml), values 0..15       */
    uint8_t target_lut[256];     /* sscbench_to_label (255 -> 255)                            */
    uint8_t target_known[256];   /* 1 where the raw target value is a key of sscbench_to_label */
    int32_t n_target_labels;     /* number of keys (informational, > 0)                       */
} sd_ssc_args;

/* One frame's SSCBench counts (evaluate_model_sscbench.py:366-367 convert_voxels,
 * :452-456 identify_additional_invalids (:814-827), :492 the density cut-off, :496-525
 * compute_occupancy_numbers / _segmentation / _recall_segmentation (:862-925)): conf
 * (n_sizes*256 + 1) uint32 on the device receives, per range s, the 16 x 16 matrix
 * conf[s][16 y_true + y_pred] over the voxels with y_true != 255 inside the FOV, and in its
 * last word the number of voxels whose label has no lookup-table entry (the reference's
 * dict lookup raises on those; the caller must too).  pred (nx,ny,nz) uint8 cityscapes
 * classes, sigma (nx,ny,nz) f32 (grown densities), target (nx,ny,nz) uint8 raw SSCBench
 * labels, fov (nx,ny,nz) uint8; all device, 16-byte aligned, nz a multiple of 16 (<= 64).
 * conf is zeroed on the stream first. */
int sd_ssc_confusion(const uint8_t *pred, const float *sigma, const uint8_t *target,
                     const uint8_t *fov, int64_t nx, int64_t ny, int64_t nz,
                     const sd_ssc_args *args, uint32_t *conf, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SDHIP_H */
