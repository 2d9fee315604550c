"""ctypes binding of libsdhip.so (the C ABI declared in include/sdhip.h).

The product path has no fallback: if the shared library is missing or a call
fails, this module raises.  Only raw device pointers, sizes and the current HIP
stream cross the boundary.
"""
from __future__ import annotations

import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# SDHIP_LIB: alternative build of the same library (diagnostic builds only)
LIB_PATH = os.environ.get("SDHIP_LIB") or os.path.join(_HERE, "libsdhip.so")
ABI_VERSION = 13
CAM_WORDS = 36  # floats per camera record (include/sdhip.h SD_CAM_WORDS)

SD_F32 = 0
SD_BF16 = 1
SD_F16 = 2
TORCH_DTYPE = {SD_F32: torch.float32, SD_BF16: torch.bfloat16, SD_F16: torch.float16}
SD_OF_TORCH = {v: k for k, v in TORCH_DTYPE.items()}
# element type of the render / field kernels' grid operands (the NHWC grid, the projected
# grid P) and of every MLP operand upstream of sigma, per precision mode: f16 in both 16-bit
# modes -- the bf16 mode keeps bf16 for the DINO output layer only (include/sdhip.h sd_mlp,
# csrc/sdhip_render.h RMode; SURVEY §8(c)'s 1e-2 m depth contract)
FIELD_DTYPE = {SD_F32: SD_F32, SD_BF16: SD_F16, SD_F16: SD_F16}

_vp = ctypes.c_void_p
_i64 = ctypes.c_int64
_i32 = ctypes.c_int32


class SdMlp(ctypes.Structure):
    _fields_ = [
        ("w_in", _vp), ("b_in_h", _vp), ("w_sig_h", _vp), ("b_sigma", ctypes.c_float),
        ("w_out", _vp), ("b_dino", _vp),
        ("C", _i32), ("D", _i32), ("dtype", _i32), ("d_hidden", _i32),
        ("b_empty_h", _vp), ("proj_flags", _i32), ("pad_mlp", _i32),
    ]


class SdFrameArgs(ctypes.Structure):
    """sd_frame_args (include/sdhip.h): sd_frame_inputs' operands."""
    _fields_ = [("img_nchw", _vp), ("N", _i64), ("H", _i64), ("W", _i64), ("out_nhwc4", _vp),
                ("w2c", _vp), ("s_w", _i64), ("Ks", _vp), ("s_k", _i64), ("n", _i64),
                ("out_cam", _vp)]


class SdHead(ctypes.Structure):
    _fields_ = [
        ("w_pe", _vp), ("w_sig", _vp), ("w_out", _vp), ("b_dino", _vp),
        ("b_sigma", ctypes.c_float), ("D", _i32), ("dtype", _i32),
    ]


class SdRenderArgs(ctypes.Structure):
    _fields_ = [
        ("rays", _vp), ("ray_dim", _i64), ("R", _i64), ("rays_per_sb", _i64), ("K", _i32),
        ("z", _vp),
        ("grid", _vp), ("Hf", _i32), ("Wf", _i32),
        ("cam_f", _vp),
        ("img", _vp), ("nv", _i32), ("Hc", _i32), ("Wc", _i32),
        ("cam_c", _vp),
        ("hard_alpha_cap", _i32),
        ("depth", _vp), ("dino", _vp), ("rgb", _vp),
        ("weights", _vp), ("alphas", _vp), ("invalid", _vp), ("invalid_f", _vp),
        ("rgb_samps", _vp),
        ("z_lindisp", _i32), ("z_seed", ctypes.c_uint64), ("z_offset", ctypes.c_uint64),
        ("work", _vp),
        ("ld_depth", _i64), ("ld_dino", _i64), ("ld_rgb", _i64),
        ("grid_dtype", _i32), ("pad1", _i32),
    ]


class SdFieldArgs(ctypes.Structure):
    _fields_ = [
        ("xyz", _vp), ("B", _i64), ("P", _i64),
        ("grid", _vp), ("Hf", _i32), ("Wf", _i32),
        ("cam_f", _vp),
        ("img", _vp), ("nv", _i32), ("Hc", _i32), ("Wc", _i32),
        ("cam_c", _vp),
        ("sigma", _vp), ("dino", _vp), ("rgb", _vp), ("invalid", _vp), ("invalid_f", _vp),
        ("dino_dtype", _i32), ("grid_dtype", _i32), ("tile_order", _vp),
    ]


class SdSegHead(ctypes.Structure):
    _fields_ = [
        ("w1", _vp), ("b1", _vp), ("w2", _vp), ("b2", _vp),
        ("wl", _vp), ("bl", _vp), ("bo", _vp), ("wm", _vp), ("bm", _vp), ("bn1", _vp),
        ("wn2", _vp), ("centres", _vp), ("assign", _vp),
        ("n_clusters", _i32), ("d_in", _i32), ("d_latent", _i32), ("d_full", _i32),
        ("d_code", _i32), ("w2_f8", _vp), ("w2_f8_scale", ctypes.c_float), ("pad0", _i32),
        ("wg", _vp), ("g2", _vp), ("b2sq", ctypes.c_float), ("frag_layout", _i32),
    ]


class SdGemmArgs(ctypes.Structure):
    _fields_ = [
        ("a", _vp), ("lda", _i64), ("w", _vp), ("bias", _vp), ("M", _i64), ("N", _i64),
        ("K", _i64), ("epi", _i32), ("out", _vp), ("ldo", _i64), ("gamma", _vp),
        ("q", _vp), ("k", _vp), ("vt", _vp),
        ("tokens", _i32), ("heads", _i32), ("head_dim", _i32), ("tokens_pad", _i32),
        ("pos", _vp), ("patches", _i32),
        ("res", _vp), ("res2", _vp),
        ("conv", _i32), ("H", _i32), ("W", _i32), ("Cin", _i32), ("stride", _i32), ("OH", _i32),
        ("OW", _i32), ("relu_in", _i32),
        ("shuf_k", _i32), ("in_h", _i32), ("in_w", _i32),
    ]


class SdPatchArgs(ctypes.Structure):
    """sd_patch_args (include/sdhip.h): PatchRaySampler batch."""
    _fields_ = [
        ("poses", _vp), ("Ks", _vp), ("frame_ids", _vp), ("patches", _vp), ("images", _vp),
        ("dino", _vp), ("rays", _vp), ("rgb_out", _vp), ("dino_out", _vp),
        ("B", _i64), ("V", _i64), ("H", _i64), ("W", _i64),
        ("n_patches", _i32), ("ph", _i32), ("pw", _i32), ("channels", _i32),
        ("dino_c", _i32), ("dino_h", _i32), ("dino_w", _i32), ("dino_upscaled", _i32),
        ("z_near", ctypes.c_float), ("z_far", ctypes.c_float),
    ]


class SdMlpTrainArgs(ctypes.Structure):
    """sd_mlp_train_args (include/sdhip.h): fused training MLP."""
    _fields_ = [
        ("x", _vp), ("N", _i64), ("ldx", _i32), ("kx", _i32), ("dtype", _i32), ("D", _i32),
        ("C", _i32), ("lddx", _i32), ("dx_dtype", _i32), ("pad", _i32), ("w1f", _vp), ("w2f", _vp), ("b_out", _vp), ("h", _vp),
        ("sigma", _vp), ("dino", _vp), ("d_sigma", _vp), ("d_dino", _vp), ("wtf", _vp),
        ("wxf", _vp), ("dy", _vp), ("dh", _vp), ("dx", _vp), ("xyz", _vp), ("cam_f", _vp),
        ("dgrid", _vp), ("P", _i64), ("Hf", _i32), ("Wf", _i32),
    ]


class SdWgradArgs(ctypes.Structure):
    """sd_wgrad_args (include/sdhip.h): training-MLP weight gradients."""
    _fields_ = [("a", _vp), ("b", _vp), ("N", _i64), ("lda", _i32), ("ldb", _i32),
                ("Ma", _i32), ("Nb", _i32), ("dtype", _i32), ("nparts", _i32), ("part", _vp)]


class SdMlpWgradArgs(ctypes.Structure):
    """sd_mlp_wgrad_args (include/sdhip.h): both training-MLP weight gradients."""
    _fields_ = [("x", _vp), ("dh", _vp), ("dy", _vp), ("h", _vp), ("N", _i64), ("ldx", _i32),
                ("kx", _i32), ("D", _i32), ("dtype", _i32), ("nparts", _i32), ("pad", _i32),
                ("work", _vp), ("dw_in", _vp), ("db_in", _vp), ("dw_out", _vp), ("db_out", _vp)]


class SdConvWgradArgs(ctypes.Structure):
    """sd_conv_wgrad_args (include/sdhip.h): weight / bias gradient of a DPT convolution."""
    _fields_ = [("x", _vp), ("dy", _vp), ("B", _i32), ("H", _i32), ("W", _i32), ("Cin", _i32),
                ("Cout", _i32), ("taps", _i32), ("stride", _i32), ("relu_in", _i32),
                ("nparts", _i32), ("pad", _i32), ("work", _vp), ("dw", _vp), ("db", _vp)]


class SdAttnBwdArgs(ctypes.Structure):
    """sd_attn_bwd_args (include/sdhip.h): backward of sd_attention."""
    _fields_ = [("q", _vp), ("k", _vp), ("vt", _vp), ("ao", _vp), ("d_ao", _vp), ("d_qkv", _vp),
                ("work", _vp), ("B", _i32), ("heads", _i32), ("tokens", _i32),
                ("tokens_pad", _i32), ("head_dim", _i32), ("scale", ctypes.c_float)]


class SdLnBwdArgs(ctypes.Structure):
    """sd_ln_bwd_args (include/sdhip.h): backward of sd_layernorm."""
    _fields_ = [("x", _vp), ("w", _vp), ("dy", _vp), ("rows", _i64), ("C", _i32),
                ("dy_f32", _i32), ("accumulate", _i32), ("nparts", _i32),
                ("eps", ctypes.c_float), ("pad", _i32), ("dx", _vp), ("work", _vp), ("dw", _vp),
                ("db", _vp)]


class SdExpandBwdArgs(ctypes.Structure):
    """sd_expand_bwd_args (include/sdhip.h): backward of transform_expand."""
    _fields_ = [("x", _vp), ("dy", _vp), ("w1", _vp), ("w2", _vp), ("w1t", _vp), ("w2t", _vp),
                ("b1", _vp), ("b2", _vp), ("P", _i64), ("x_dtype", _i32), ("pad", _i32),
                ("dx", _vp), ("h", _vp), ("de", _vp), ("dh", _vp), ("xb", _vp)]


class SdStegoTrainArgs(ctypes.Structure):
    """sd_stego_train_args (include/sdhip.h): StegoClusterHead in train mode."""
    _fields_ = [("x", _vp), ("wl", _vp), ("wn1", _vp), ("wn2", _vp), ("wn2t", _vp), ("bl", _vp),
                ("bn1", _vp), ("bn2", _vp), ("m_lin", _vp), ("m_non", _vp), ("M", _i64),
                ("rows_per_group", _i64), ("n_groups", _i64), ("d_in", _i32), ("d_code", _i32),
                ("normalize", _i32), ("pad", _i32), ("y", _vp), ("xh", _vp), ("mid", _vp), ("e", _vp), ("dy", _vp), ("dlin", _vp),
                ("dnon", _vp), ("dmid", _vp)]


class SdClusterProbeArgs(ctypes.Structure):
    """sd_cluster_probe_args (include/sdhip.h): cosine k-means labels and loss statistics."""
    _fields_ = [("x", _vp), ("m", _vp), ("centres", _vp), ("w", _vp), ("N", _i64),
                ("rows_per_group", _i64), ("n_groups", _i64), ("d", _i32), ("K", _i32),
                ("x_dtype", _i32), ("pad", _i32), ("work", _vp), ("labels", _vp), ("S", _vp),
                ("counts", _vp)]


class SdLinearProbeArgs(ctypes.Structure):
    """sd_linear_probe_args (include/sdhip.h): linear-probe logits, cross-entropy and gradients."""
    _fields_ = [("x", _vp), ("m", _vp), ("W", _vp), ("b", _vp), ("target", _vp), ("N", _i64),
                ("rows_per_group", _i64), ("n_groups", _i64), ("d", _i32), ("C", _i32),
                ("x_dtype", _i32), ("normalize", _i32), ("work", _vp), ("pred", _vp),
                ("loss_sum", _vp), ("n_valid", _vp), ("gW", _vp), ("gb", _vp), ("row_loss", _vp)]


class SdReconLossArgs(ctypes.Structure):
    """sd_recon_loss_args (include/sdhip.h): the first stage's ReconstructionLoss."""
    _fields_ = [("rgb", _vp), ("rgb_gt", _vp), ("invalid", _vp), ("weights", _vp), ("depth", _vp),
                ("dino", _vp), ("dino_down", _vp), ("dino_gt", _vp), ("dino_artifacts", _vp),
                ("P", _i64), ("R", _i64), ("h", _i32), ("w", _i32), ("nv", _i32), ("K", _i32),
                ("C", _i32), ("Cd", _i32), ("dino_dtype", _i32), ("policy", _i32),
                ("lambda_coarse", ctypes.c_float), ("lambda_dino", ctypes.c_float),
                ("temperature", ctypes.c_float), ("lambda_depth", ctypes.c_float),
                ("lambda_dsmooth", ctypes.c_float), ("pad", ctypes.c_float),
                ("work", _vp), ("rec", _vp), ("terms", _vp), ("sel", _vp), ("edge", _vp),
                ("dmean", _vp), ("count", _vp), ("g_rec", _vp), ("d_rgb", _vp), ("d_depth", _vp),
                ("d_dino", _vp), ("d_down", _vp)]


class SdStegoCorrArgs(ctypes.Structure):
    """sd_stego_corr_args (include/sdhip.h): the downstream stage's fused correlation loss."""
    _fields_ = [("dino_a", _vp), ("dino_b", _vp * 3), ("stego_a", _vp), ("stego_b", _vp * 3),
                ("weight", ctypes.c_float * 3), ("shift", ctypes.c_float * 3), ("nc", _i64),
                ("P", _i32), ("Q", _i32), ("d", _i32), ("code_dim", _i32), ("n_pairs", _i32),
                ("dino_dtype", _i32), ("pointwise", _i32), ("pad", _i32), ("work", _vp),
                ("work_bytes", _i64), ("loss", _vp), ("up", _vp), ("d_a", _vp), ("d_b", _vp * 3)]


class SdMscGtArgs(ctypes.Structure):
    """sd_msc_gt_args (include/sdhip.h): multi-scale-crop DINO targets."""
    _fields_ = [("feat", _vp), ("T", _vp), ("out", _vp), ("B", _i32), ("V", _i32), ("C", _i32),
                ("hp", _i32), ("wp", _i32), ("H", _i32), ("W", _i32), ("normalize", _i32)]


class SdCrop3dArgs(ctypes.Structure):
    """sd_crop3d_args (include/sdhip.h): quantile bins, pixel pick, crop centres, sample points."""
    _fields_ = [("depth", _vp), ("poses", _vp), ("projs", _vp), ("u_pick", _vp), ("shift", _vp),
                ("limits", _vp), ("count", _vp), ("pixel", _vp), ("centre", _vp), ("points", _vp),
                ("depth_stride", _i64), ("pose_stride", _i64), ("proj_stride", _i64),
                ("n", _i32), ("h", _i32), ("w", _i32), ("n_crops", _i32), ("S", _i32),
                ("z_far", ctypes.c_float)]


class SdCrop3dCompactArgs(ctypes.Structure):
    """sd_crop3d_compact_args (include/sdhip.h): keep the crops with enough occupied samples."""
    _fields_ = [("sigma", _vp), ("codes", _vp), ("crop_ok", _vp), ("codes_out", _vp),
                ("occ_out", _vp), ("n_valid", _vp), ("slot", _vp), ("C", _i32), ("S", _i32),
                ("D", _i32), ("n_samples", _i32), ("codes_dtype", _i32), ("thr", ctypes.c_float)]


class SdSalienceArgs(ctypes.Structure):
    """sd_salience_args (include/sdhip.h): PatchSalienceDownsampler forward / backward."""
    _fields_ = [
        ("x", _vp), ("w", _vp), ("b", _vp), ("pw", _vp), ("pb", _vp), ("N", _i64),
        ("S", _i32), ("C", _i32), ("normalize", _i32), ("pad", _i32),
        ("out", _vp), ("sal", _vp), ("wmap", _vp), ("ynorm", _vp),
        ("g_out", _vp), ("g_sal", _vp), ("g_wmap", _vp),
        ("gx", _vp), ("gw_part", _vp), ("gpw_part", _vp), ("gpb_part", _vp), ("gb_part", _vp),
    ]


class SdSscArgs(ctypes.Structure):
    """sd_ssc_args (include/sdhip.h): SSCBench scoring configuration."""
    _fields_ = [
        ("sigma_cutoff", ctypes.c_float), ("additional_invalids", _i32), ("inv_zmax", _i32),
        ("n_sizes", _i32), ("crop_x", _i32 * 4), ("crop_y0", _i32 * 4), ("crop_y1", _i32 * 4),
        ("n_pred_labels", _i32), ("pred_lut", ctypes.c_uint8 * 256),
        ("target_lut", ctypes.c_uint8 * 256), ("target_known", ctypes.c_uint8 * 256),
        ("n_target_labels", _i32),
    ]


SEG_MAX_RESULTS = 8   # include/sdhip_metrics.h SD_SEG_MAX_RESULTS
SEG_MAX_BINS = 8192   # SD_SEG_MAX_BINS


class SdSegConfusionArgs(ctypes.Structure):
    """sd_seg_confusion_args (include/sdhip_metrics.h): confusion matrices of up to 8 results."""
    _fields_ = [
        ("target", _vp), ("pred", _vp * SEG_MAX_RESULTS), ("pred_stride", _i64 * SEG_MAX_RESULTS),
        ("n", _i64), ("hw", _i64),
        ("n_results", _i32), ("gt_classes", _i32), ("n_classes", _i32), ("pad_", _i32),
        ("conf", _vp),
    ]


CRF_MAX_RESULTS = 8    # include/sdhip_crf.h SD_CRF_MAX_RESULTS
CRF_MAX_CLASSES = 64   # SD_CRF_MAX_CLASSES
CRF_MAX_SXY_G = 0.7    # SD_CRF_MAX_SXY_G


class SdCrfArgs(ctypes.Structure):
    """sd_crf_args (include/sdhip_crf.h): dense-CRF inference for up to 8 results of one image."""
    _fields_ = [
        ("image", _vp), ("unary", _vp), ("work", _vp), ("labels", _vp), ("q", _vp),
        ("H", _i32), ("W", _i32), ("n_results", _i32), ("iters", _i32),
        ("classes", _i32 * CRF_MAX_RESULTS),
        ("w_g", ctypes.c_float), ("sxy_g", ctypes.c_float), ("w_b", ctypes.c_float),
        ("sxy_b", ctypes.c_float), ("srgb", ctypes.c_float), ("pad_", ctypes.c_float),
    ]


(SD_EPI_BF16, SD_EPI_GELU, SD_EPI_F32, SD_EPI_RESID, SD_EPI_QKV, SD_EPI_PATCH, SD_EPI_SHUF,
 SD_EPI_NCHW) = range(8)

# (name, argtypes) of every exported entry point; tests check the .so exports all.
SIGNATURES = {
    "sd_last_error": [],
    "sd_abi_version": [],
    "sd_field_dtype": [ctypes.c_int],
    "sd_reserve_cus": [ctypes.c_int32],
    "sd_spin": [ctypes.c_int32, ctypes.c_float, _vp],
    "sd_ln_gemm": [ctypes.POINTER(SdGemmArgs), _vp, _vp, _vp, ctypes.c_float, _vp],
    "sd_gen_rays": [_vp, _vp, _vp, _i64, _i64, _i64, ctypes.c_float, ctypes.c_float, _vp, _vp],
    "sd_sample_z": [_vp, _i64, _i64, _i64, ctypes.c_int, _vp, ctypes.c_uint64, ctypes.c_uint64,
                    _vp, _vp],
    "sd_patch_rays": [ctypes.POINTER(SdPatchArgs), _vp],
    "sd_pack_grid": [_vp, _i64, _i64, _i64, _i64, ctypes.c_int, _vp, _vp],
    "sd_pack_image": [_vp, _i64, _i64, _i64, _vp, _vp],
    "sd_cam_records": [_vp, _i64, _vp, _i64, _i64, _vp, _vp],
    "sd_frame_inputs": [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp],
    "sd_render_fused": [ctypes.POINTER(SdRenderArgs), ctypes.POINTER(SdMlp), _vp],
    "sd_field_query": [ctypes.POINTER(SdFieldArgs), ctypes.POINTER(SdMlp), _vp],
    "sd_field_gather": [_vp, _i64, _i64, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp,
                        _vp, _i32, _vp, _vp, _vp, _vp],
    "sd_field_gather_bwd": [_vp, _i64, _i64, _vp, _i32, _i64, _i32, _i32, _i32, _vp, _vp, _vp],
    "sd_unpack_grid": [_vp, _i64, _i64, _i64, _i64, _vp, _vp],
    "sd_composite_bwd": [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp,
                         _vp, _vp, _vp, _vp, _vp],
    "sd_project_grid": [_vp, _i64, _i64, _i64, ctypes.POINTER(SdMlp), _vp, _vp],
    "sd_project_grid_nhwc": [_vp, _i64, _i64, _i64, ctypes.POINTER(SdMlp), _vp, _vp],
    "sd_project_grid_nhwc_inputs": [_vp, _i64, _i64, _i64, ctypes.POINTER(SdMlp), _vp,
                                    ctypes.POINTER(SdFrameArgs), _vp],
    "sd_cast_grid": [_vp, _i64, ctypes.c_int, _vp, _vp],
    "sd_render_proj": [ctypes.POINTER(SdRenderArgs), ctypes.POINTER(SdHead), _vp],
    "sd_render_proj_work_bytes": [_i64, _i32],
    "sd_render_tile_cap": [_i32],
    "sd_render_tile_order": [_i32],
    "sd_composite": [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp,
                     _vp],
    "sd_voxel_points": [ctypes.POINTER(ctypes.c_double), ctypes.c_double, _i64, _i64, _i64,
                        ctypes.POINTER(ctypes.c_double), _vp, _vp],
    "sd_grow3": [_vp, _i64, _i64, _i64, _vp, _vp],
    "sd_seg_query": [_vp, _i32, _i64, ctypes.POINTER(SdSegHead), _vp, ctypes.c_float, _vp, _vp,
                     _vp, _vp],
    "sd_voxel_fov": [ctypes.POINTER(ctypes.c_double), ctypes.c_double, _i64, _i64, _i64,
                     ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), _i32, _i32,
                     _vp, _vp],
    "sd_ssc_confusion": [_vp, _vp, _vp, _vp, _i64, _i64, _i64, ctypes.POINTER(SdSscArgs), _vp,
                         _vp],
    "sd_mlp_train_fwd": [ctypes.POINTER(SdMlpTrainArgs), _vp],
    "sd_mlp_train_bwd": [ctypes.POINTER(SdMlpTrainArgs), _vp],
    "sd_wgrad": [ctypes.POINTER(SdWgradArgs), _vp],
    "sd_mlp_train_wgrad": [ctypes.POINTER(SdMlpWgradArgs), _vp],
    "sd_mlp_train_wgrad_work": [_i32],
    "sd_salience_fwd": [ctypes.POINTER(SdSalienceArgs), _vp],
    "sd_salience_bwd": [ctypes.POINTER(SdSalienceArgs), _vp],
    "sd_gemm": [ctypes.POINTER(SdGemmArgs), _vp],
    "sd_attention": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, ctypes.c_float, _vp, _vp],
    "sd_layernorm": [_vp, _i64, _i32, _vp, _vp, ctypes.c_float, _vp, _i32, _vp],
    "sd_patchify": [_vp, _i32, _i32, _i32, _i32, _i32, ctypes.POINTER(ctypes.c_float),
                    ctypes.POINTER(ctypes.c_float), _vp, _vp, _vp, _vp, _i32, _vp],
    "sd_tokens_to_grid": [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp],
    "sd_tokens_to_nhwc": [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp],
    "sd_layernorm_nhwc": [_vp, _i32, _i32, _i32, _vp, _vp, ctypes.c_float, _i32, _i32, _i32, _vp, _vp],
    "sd_upsample2x": [_vp, _i32, _i32, _i32, _i32, _vp, _vp],
    "sd_conv_wgrad_parts": [ctypes.POINTER(SdConvWgradArgs)],
    "sd_conv_wgrad_work": [ctypes.POINTER(SdConvWgradArgs)],
    "sd_conv_wgrad": [ctypes.POINTER(SdConvWgradArgs), _vp],
    "sd_upsample2x_bwd": [_vp, _i32, _i32, _i32, _i32, _vp, _vp],
    "sd_relu_bwd": [_vp, _vp, _vp, _i64, _vp, _vp],
    "sd_attention_bwd": [ctypes.POINTER(SdAttnBwdArgs), _vp],
    "sd_layernorm_bwd_parts": [_i64],
    "sd_layernorm_bwd": [ctypes.POINTER(SdLnBwdArgs), _vp],
    "sd_gelu_bwd": [_vp, _vp, _i64, _vp, _vp],
    "sd_expand_bwd": [ctypes.POINTER(SdExpandBwdArgs), ctypes.POINTER(SdSegHead), _vp],
    "sd_stego_train_fwd": [ctypes.POINTER(SdStegoTrainArgs), _vp],
    "sd_stego_train_bwd": [ctypes.POINTER(SdStegoTrainArgs), _vp],
    "sd_cluster_probe_work": [_i64, _i32, _i32],
    "sd_cluster_probe": [ctypes.POINTER(SdClusterProbeArgs), _vp],
    "sd_linear_probe_work": [_i64, _i32, _i32],
    "sd_linear_probe": [ctypes.POINTER(SdLinearProbeArgs), _vp],
    "sd_recon_loss_work": [_i64, _i32, _i64],
    "sd_recon_loss_fwd": [ctypes.POINTER(SdReconLossArgs), _vp],
    "sd_recon_loss_bwd": [ctypes.POINTER(SdReconLossArgs), _vp],
    "sd_stego_corr_work": [_i64, _i32, _i32, _i32, _i32, _i32],
    "sd_stego_corr_fwd": [ctypes.POINTER(SdStegoCorrArgs), _vp],
    "sd_stego_corr_bwd": [ctypes.POINTER(SdStegoCorrArgs), _vp],
    "sd_msc_gt": [ctypes.POINTER(SdMscGtArgs), _vp],
    "sd_crop3d_centres": [ctypes.POINTER(SdCrop3dArgs), _vp],
    "sd_crop3d_compact": [ctypes.POINTER(SdCrop3dCompactArgs), _vp],
    # include/sdhip_metrics.h
    "sd_depth_metrics_work": [_i64, _i64],
    "sd_depth_metrics": [_vp, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp],
    "sd_dino_metrics_work": [_i64, _i64, _i64, _i32],
    "sd_dino_metrics": [_vp, _i32, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _vp],
    "sd_seg_confusion": [ctypes.POINTER(SdSegConfusionArgs), _vp],
    # include/sdhip_crf.h
    "sd_dense_crf_work": [_i32, _i32, _i32, ctypes.POINTER(_i32)],
    "sd_dense_crf": [ctypes.POINTER(SdCrfArgs), _vp],
    # include/sdhip_ssc_pool.h
    "sd_ssc_pool": [_vp, _vp, _i64, _i64, _i64, _i32, ctypes.c_float, _i32, _vp, _vp, _vp],
}

_lib = None


def load(path: str = LIB_PATH):
    """Load libsdhip.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(
            f"scenedino_amd: HIP library {path} is missing. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950).")
    lib = ctypes.CDLL(path)
    missing = [name for name in SIGNATURES if not hasattr(lib, name)]
    if missing:  # entry points added without an ABI bump (the ViT / expand backward): an older build
        raise RuntimeError(f"scenedino_amd: {path} lacks {', '.join(missing)}; rebuild it "
                           "(`python -c 'import __graft_entry__ as g; g.build()'`)")
    for name, argt in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argt
        fn.restype = ctypes.c_int
    lib.sd_last_error.restype = ctypes.c_char_p
    lib.sd_render_proj_work_bytes.restype = ctypes.c_int64
    lib.sd_mlp_train_wgrad_work.restype = ctypes.c_int64
    lib.sd_conv_wgrad_work.restype = ctypes.c_int64
    lib.sd_cluster_probe_work.restype = ctypes.c_int64
    lib.sd_linear_probe_work.restype = ctypes.c_int64
    lib.sd_recon_loss_work.restype = ctypes.c_int64
    lib.sd_stego_corr_work.restype = ctypes.c_int64
    lib.sd_depth_metrics_work.restype = ctypes.c_int64
    lib.sd_dino_metrics_work.restype = ctypes.c_int64
    lib.sd_dense_crf_work.restype = ctypes.c_int64
    if lib.sd_abi_version() != ABI_VERSION:
        raise RuntimeError("scenedino_amd: libsdhip.so ABI version mismatch; rebuild it")
    _lib = lib
    return lib


def _check(rc: int, what: str):
    if rc != 0:
        msg = _lib.sd_last_error().decode(errors="replace") if _lib else ""
        raise RuntimeError(f"scenedino_amd: {what} failed (rc={rc}): {msg}")


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_of(t: torch.Tensor):
    if t.device.type != "cuda":
        raise RuntimeError("scenedino_amd: HIP kernels need tensors on a ROCm (cuda) device; "
                           f"got {t.device}")
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _req(t: torch.Tensor, name: str, dtype=torch.float32):
    if t.dtype != dtype:
        raise TypeError(f"scenedino_amd: {name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"scenedino_amd: {name} must be contiguous")
    return t


# ---------------------------------------------------------------------------
# thin wrappers (torch tensors in, torch tensors out; all on the same device)
# ---------------------------------------------------------------------------
def gen_rays(poses_c2w, Ks, frame_ids, H, W, z_near, z_far):
    lib = load()
    v = poses_c2w.shape[0]
    out = torch.empty(v, H, W, 11, device=poses_c2w.device, dtype=torch.float32)
    _check(lib.sd_gen_rays(ptr(_req(poses_c2w, "poses")), ptr(_req(Ks, "Ks")),
                           ptr(_req(frame_ids, "frame_ids")), v, H, W, float(z_near),
                           float(z_far), ptr(out), stream_of(out)), "sd_gen_rays")
    return out


def mlp_train_fwd(args: SdMlpTrainArgs, ref_tensor):
    lib = load()
    _check(lib.sd_mlp_train_fwd(ctypes.byref(args), stream_of(ref_tensor)), "sd_mlp_train_fwd")


def mlp_train_bwd(args: SdMlpTrainArgs, ref_tensor):
    lib = load()
    _check(lib.sd_mlp_train_bwd(ctypes.byref(args), stream_of(ref_tensor)), "sd_mlp_train_bwd")


def wgrad(a, b, Ma, Nb, nparts=None):
    """sum_p a[p, :Ma]^T b[p, :Nb] over the rows of two 16-bit (N, *) matrices (sd_wgrad):
    (Ma, Nb) f32."""
    lib = load()
    N = a.shape[0]
    MaP, NbP = (Ma + 31) // 32 * 32, (Nb + 31) // 32 * 32
    if nparts is None:  # ~2 workgroups per CU over the column splits (5 tiles each)
        splits = (NbP // 32 + 4) // 5
        nparts = max(1, min(512 // splits, (N + 511) // 512))
    part = torch.empty(nparts, MaP, NbP, device=a.device)
    g = SdWgradArgs(a=a.data_ptr(), b=b.data_ptr(), N=N, lda=a.stride(0), ldb=b.stride(0),
                    Ma=Ma, Nb=Nb, dtype=SD_OF_TORCH[a.dtype], nparts=nparts,
                    part=part.data_ptr())
    _check(lib.sd_wgrad(ctypes.byref(g), stream_of(a)), "sd_wgrad")
    return part.sum(0)[:Ma, :Nb]


def mlp_train_wgrad(x, dh, dy, h, kx, D, nparts=None):
    """Both weight gradients of the training MLP (sd_mlp_train_wgrad) from the 16-bit rows
    of sd_mlp_train_fwd / _bwd: (dw_in (128, kx - 1), db_in (128), dw_out (1 + D, 128),
    db_out (1 + D)) f32, lin_out rows in the parameter order (out_0 first)."""
    lib = load()
    N, ldx = x.shape
    dev = x.device
    if nparts is None:  # one workgroup per CU
        nparts = max(1, min(torch.cuda.get_device_properties(dev).multi_processor_count,
                            (N + 31) // 32))
    work = torch.empty(int(lib.sd_mlp_train_wgrad_work(nparts)), device=dev)
    dw_in = torch.empty(128, kx - 1, device=dev)
    db_in = torch.empty(128, device=dev)
    dw_out = torch.empty(1 + D, 128, device=dev)
    db_out = torch.empty(1 + D, device=dev)
    g = SdMlpWgradArgs(x=x.data_ptr(), dh=dh.data_ptr(), dy=dy.data_ptr(), h=h.data_ptr(), N=N,
                       ldx=ldx, kx=kx, D=D, dtype=SD_OF_TORCH[x.dtype], nparts=nparts,
                       work=work.data_ptr(), dw_in=dw_in.data_ptr(), db_in=db_in.data_ptr(),
                       dw_out=dw_out.data_ptr(), db_out=db_out.data_ptr())
    _check(lib.sd_mlp_train_wgrad(ctypes.byref(g), stream_of(x)), "sd_mlp_train_wgrad")
    return dw_in, db_in, dw_out, db_out


def salience_fwd(args: SdSalienceArgs, ref_tensor):
    lib = load()
    _check(lib.sd_salience_fwd(ctypes.byref(args), stream_of(ref_tensor)), "sd_salience_fwd")


def salience_bwd(args: SdSalienceArgs, ref_tensor):
    lib = load()
    _check(lib.sd_salience_bwd(ctypes.byref(args), stream_of(ref_tensor)), "sd_salience_bwd")


def patch_rays(args: SdPatchArgs, ref_tensor):
    lib = load()
    _check(lib.sd_patch_rays(ctypes.byref(args), stream_of(ref_tensor)), "sd_patch_rays")


def sample_z(rays, K, lindisp, u=None, seed=0, offset=0, out=None):
    lib = load()
    R, rd = rays.shape
    z = out if out is not None else torch.empty(R, K, device=rays.device, dtype=torch.float32)
    if u is not None:
        _req(u, "u")
        if tuple(u.shape) != (R, K):
            raise ValueError(f"jitter u must be ({R},{K}), got {tuple(u.shape)}")
    _check(lib.sd_sample_z(ptr(_req(rays, "rays")), R, rd, K, int(bool(lindisp)), ptr(u),
                           ctypes.c_uint64(seed & (2**64 - 1)),
                           ctypes.c_uint64(offset & (2**64 - 1)), ptr(z), stream_of(z)),
           "sd_sample_z")
    return z


def channels_last(g: torch.Tensor) -> bool:
    """(B, C, H, W) tensor whose storage is NHWC (the native encoder's grid layout)."""
    return g.dim() == 4 and not g.is_contiguous() and g.permute(0, 2, 3, 1).is_contiguous()


def pack_grid(grid, dtype):
    """(B, C, H, W) f32 grid -> NHWC (B, H, W, C) in dtype: sd_pack_grid transposes an NCHW
    grid; a channels-last one is returned as its NHWC view (f32) or cast (sd_cast_grid)."""
    lib = load()
    B, C, H, W = grid.shape
    if channels_last(grid):
        nhwc = _req(grid.permute(0, 2, 3, 1), "grid")
        if dtype == SD_F32:
            return nhwc
        out = torch.empty(B, H, W, C, device=grid.device, dtype=TORCH_DTYPE[dtype])
        _check(lib.sd_cast_grid(ptr(nhwc), nhwc.numel(), dtype, ptr(out), stream_of(out)),
               "sd_cast_grid")
        return out
    grid = grid.contiguous()
    out = torch.empty(B, H, W, C, device=grid.device, dtype=TORCH_DTYPE[dtype])
    _check(lib.sd_pack_grid(ptr(_req(grid, "grid")), B, C, H, W, dtype, ptr(out),
                            stream_of(out)), "sd_pack_grid")
    return out


def pack_image(img_nchw):
    lib = load()
    N, c3, H, W = img_nchw.shape
    assert c3 == 3, "colour images must have 3 channels"
    out = torch.empty(N, H, W, 4, device=img_nchw.device, dtype=torch.float32)
    _check(lib.sd_pack_image(ptr(_req(img_nchw, "images")), N, H, W, ptr(out), stream_of(out)),
           "sd_pack_image")
    return out


def _cam_operands(poses_w2c, Ks):
    w = poses_w2c.float().reshape(-1, 4, 4)
    k = Ks.float().reshape(-1, 3, 3)
    if w.stride()[1:] != (4, 1):
        w = w.contiguous()
    if k.stride()[1:] != (3, 1):
        k = k.contiguous()
    n = w.shape[0]
    if k.shape[0] != n:
        raise ValueError("poses and intrinsics must have the same number of views")
    return w, k, n, (w.stride(0) if n > 1 else 16), (k.stride(0) if n > 1 else 9)


def frame_inputs(img_nchw, poses_w2c, Ks):
    """pack_image(img_nchw) and cam_records(poses_w2c, Ks) in one launch (sd_frame_inputs)."""
    lib = load()
    N, c3, H, W = img_nchw.shape
    assert c3 == 3, "colour images must have 3 channels"
    w, k, n, sw, sk = _cam_operands(poses_w2c, Ks)
    img = torch.empty(N, H, W, 4, device=img_nchw.device, dtype=torch.float32)
    cam = torch.empty(*poses_w2c.shape[:-2], CAM_WORDS, device=w.device, dtype=torch.float32)
    _check(lib.sd_frame_inputs(ptr(_req(img_nchw, "images")), N, H, W, ptr(img), ptr(w), sw,
                               ptr(k), sk, n, ptr(cam), stream_of(img)), "sd_frame_inputs")
    return img, cam


def cam_records(poses_w2c, Ks):
    """(..., 4, 4) w2c and (..., 3, 3) K -> (..., CAM_WORDS) camera records (one launch)."""
    lib = load()
    lead = poses_w2c.shape[:-2]
    w = poses_w2c.float().reshape(-1, 4, 4)
    k = Ks.float().reshape(-1, 3, 3)
    if w.stride()[1:] != (4, 1):
        w = w.contiguous()
    if k.stride()[1:] != (3, 1):
        k = k.contiguous()
    n = w.shape[0]
    if k.shape[0] != n:
        raise ValueError("poses and intrinsics must have the same number of views")
    out = torch.empty(*lead, CAM_WORDS, device=w.device, dtype=torch.float32)
    _check(lib.sd_cam_records(ptr(w), w.stride(0) if n > 1 else 16, ptr(k),
                              k.stride(0) if n > 1 else 9, n, ptr(out), stream_of(out)),
           "sd_cam_records")
    return out


def render_fused(args: SdRenderArgs, mlp: SdMlp, ref_tensor):
    lib = load()
    _check(lib.sd_render_fused(ctypes.byref(args), ctypes.byref(mlp), stream_of(ref_tensor)),
           "sd_render_fused")


SD_PROJ_EXACT_GRID = 1
SD_SEG_FRAG32 = 0  # sd_seg_head.frag_layout (include/sdhip.h)
SD_SEG_FRAG16 = 1


def _with_flags(mlp: SdMlp, exact_grid: bool) -> SdMlp:
    """A copy of the MLP record with sd_mlp.proj_flags for one projection call."""
    m = SdMlp.from_buffer_copy(mlp)
    m.proj_flags = SD_PROJ_EXACT_GRID if exact_grid else 0
    return m


def project_grid(grid, mlp: SdMlp, dtype, exact_grid: bool = False):
    """P = W_in[:, :C] . grid + b_in per pixel: (B, Hf, Wf, 128) in FIELD_DTYPE[dtype] (f16
    for both 16-bit modes; plain NHWC, 256 B per pixel).  grid (B, C, Hf, Wf) f32, NCHW or
    channels-last.  exact_grid: the grid as a hi + lo f16 operand pair (SD_PROJ_EXACT_GRID)."""
    lib = load()
    mlp = _with_flags(mlp, exact_grid)
    B, C, H, W = grid.shape
    out = torch.empty(B, H, W, 128, device=grid.device, dtype=TORCH_DTYPE[FIELD_DTYPE[dtype]])
    if channels_last(grid):
        _check(lib.sd_project_grid_nhwc(ptr(_req(grid.permute(0, 2, 3, 1), "grid")), B, H, W,
                                        ctypes.byref(mlp), ptr(out), stream_of(out)),
               "sd_project_grid_nhwc")
        return out
    _check(lib.sd_project_grid(ptr(_req(grid.contiguous(), "grid")), B, H, W, ctypes.byref(mlp),
                               ptr(out), stream_of(out)), "sd_project_grid")
    return out


def project_grid_inputs(grid, mlp: SdMlp, dtype, img_nchw, poses_w2c, Ks, exact_grid: bool = False):
    """project_grid(grid) and frame_inputs(img_nchw, poses_w2c, Ks) in one launch
    (sd_project_grid_nhwc_inputs; channels-last grids -- others take the two calls).
    Returns (P, packed image, camera records)."""
    if not channels_last(grid):
        img, cam = frame_inputs(img_nchw, poses_w2c, Ks)
        return project_grid(grid, mlp, dtype, exact_grid), img, cam
    lib = load()
    mlp = _with_flags(mlp, exact_grid)
    B, C, H, W = grid.shape
    N, c3, Hc, Wc = img_nchw.shape
    assert c3 == 3, "colour images must have 3 channels"
    w, k, n, sw, sk = _cam_operands(poses_w2c, Ks)
    out = torch.empty(B, H, W, 128, device=grid.device, dtype=TORCH_DTYPE[FIELD_DTYPE[dtype]])
    img = torch.empty(N, Hc, Wc, 4, device=img_nchw.device, dtype=torch.float32)
    cam = torch.empty(*poses_w2c.shape[:-2], CAM_WORDS, device=w.device, dtype=torch.float32)
    fa = SdFrameArgs(img_nchw=ptr(_req(img_nchw, "images")), N=N, H=Hc, W=Wc, out_nhwc4=ptr(img),
                     w2c=ptr(w), s_w=sw, Ks=ptr(k), s_k=sk, n=n, out_cam=ptr(cam))
    _check(lib.sd_project_grid_nhwc_inputs(ptr(_req(grid.permute(0, 2, 3, 1), "grid")), B, H, W,
                                           ctypes.byref(mlp), ptr(out), ctypes.byref(fa),
                                           stream_of(out)), "sd_project_grid_nhwc_inputs")
    return out, img, cam


def render_proj_work_bytes(R: int, D: int) -> int:
    return int(load().sd_render_proj_work_bytes(R, D))


def render_tile_cap(nbytes: int) -> int:
    """Test hook (sd_render_tile_cap): cap the tile buffers, returns the previous cap."""
    return int(load().sd_render_tile_cap(int(nbytes)))


def render_tile_order(order: int) -> int:
    """Test hook (sd_render_tile_order, include/sdhip.h): the tile kernel's step order,
    0 = default, 3 = late order, 4 = early order; returns the previous setting.  Any other
    value only queries it."""
    return int(load().sd_render_tile_order(int(order)))


def render_proj(args: SdRenderArgs, head: SdHead, ref_tensor):
    lib = load()
    _check(lib.sd_render_proj(ctypes.byref(args), ctypes.byref(head), stream_of(ref_tensor)),
           "sd_render_proj")


def field_query(args: SdFieldArgs, mlp: SdMlp, ref_tensor):
    lib = load()
    _check(lib.sd_field_query(ctypes.byref(args), ctypes.byref(mlp), stream_of(ref_tensor)),
           "sd_field_query")


def voxel_fov(origin, voxel_size, dims, T, cam_k, img_w, img_h, device):
    """SSCBench field-of-view mask (sd_voxel_fov): (nx*ny*nz,) uint8 0/1 on device."""
    lib = load()
    nx, ny, nz = (int(d) for d in dims)
    o = (ctypes.c_double * 3)(*[float(v) for v in origin])
    Tm = torch.as_tensor(T, dtype=torch.float64).reshape(-1, 4)[:3].flatten().tolist()
    t = (ctypes.c_double * 12)(*Tm)
    km = (ctypes.c_double * 9)(*torch.as_tensor(cam_k, dtype=torch.float64)
                               .reshape(3, 3).flatten().tolist())
    out = torch.empty(nx * ny * nz, device=device, dtype=torch.uint8)
    _check(lib.sd_voxel_fov(o, float(voxel_size), nx, ny, nz, t, km, int(img_w), int(img_h),
                            ptr(out), stream_of(out)), "sd_voxel_fov")
    return out


def ssc_confusion(pred, sigma, target, fov, args: SdSscArgs, conf):
    """One frame's SSCBench confusion matrices (sd_ssc_confusion) into ``conf``
    ((n_sizes*256 + 1,) int32 viewed as uint32, device)."""
    lib = load()
    nx, ny, nz = (int(d) for d in pred.shape)
    _check(lib.sd_ssc_confusion(ptr(pred), ptr(sigma), ptr(target), ptr(fov), nx, ny, nz,
                                ctypes.byref(args), ptr(conf), stream_of(conf)),
           "sd_ssc_confusion")


def voxel_points(origin, voxel_size, dims, T, device):
    """SSCBench voxel-centre grid (sd_voxel_points): (nx*ny*nz, 3) float32 on device.
    origin (3,), T (4, 4) or (3, 4): host numbers (float64)."""
    lib = load()
    nx, ny, nz = (int(d) for d in dims)
    o = (ctypes.c_double * 3)(*[float(v) for v in origin])
    Tm = torch.as_tensor(T, dtype=torch.float64).reshape(-1, 4)[:3].flatten().tolist()
    t = (ctypes.c_double * 12)(*Tm)
    out = torch.empty(nx * ny * nz, 3, device=device, dtype=torch.float32)
    _check(lib.sd_voxel_points(o, float(voxel_size), nx, ny, nz, t, ptr(out), stream_of(out)),
           "sd_voxel_points")
    return out


def grow3(sig):
    """3x3x3 max filter of a (nx, ny, nz) f32 density grid (sd_grow3): F.max_pool3d(
    sig[None], 3, 1, 1)[0] of evaluate_model_sscbench.py:755-756."""
    lib = load()
    _req(sig, "sig")
    if sig.dim() != 3:
        raise ValueError("grow3: sig must be (nx, ny, nz)")
    out = torch.empty_like(sig)
    _check(lib.sd_grow3(ptr(sig), sig.shape[0], sig.shape[1], sig.shape[2], ptr(out),
                        stream_of(sig)), "sd_grow3")
    return out


SSC_POOL_MAX_CLASSES = 32  # include/sdhip_ssc_pool.h SD_SSC_POOL_MAX_CLASSES


def ssc_pool(sigma_f, seg_f, factor, voxel_size, n_classes=19):
    """Fine-to-coarse pooling of a supersampled voxel query (sd_ssc_pool, include/
    sdhip_ssc_pool.h): sigma_f (f cx, f cy, f cz) f32 and seg_f (same shape) uint8 ->
    sigma (cx, cy, cz) f32 (max over the f^3 children) and seg (cx, cy, cz) uint8 (argmax of
    the average-pooled alpha votes), evaluate_model_sscbench.py:727-745."""
    lib = load()
    _req(sigma_f, "sigma_f")
    _req(seg_f, "seg_f", torch.uint8)
    f = int(factor)
    if sigma_f.dim() != 3 or seg_f.shape != sigma_f.shape or f < 1 or \
            any(int(d) % f for d in sigma_f.shape):
        raise ValueError("ssc_pool: sigma_f / seg_f must share one (f cx, f cy, f cz) shape")
    cx, cy, cz = (int(d) // f for d in sigma_f.shape)
    sigma = torch.empty(cx, cy, cz, device=sigma_f.device, dtype=torch.float32)
    seg = torch.empty(cx, cy, cz, device=sigma_f.device, dtype=torch.uint8)
    _check(lib.sd_ssc_pool(ptr(sigma_f), ptr(seg_f), cx, cy, cz, f, float(voxel_size),
                           int(n_classes), ptr(sigma), ptr(seg), stream_of(sigma_f)),
           "sd_ssc_pool")
    return sigma, seg


def seg_query(dino, rec: SdSegHead, sigma=None, voxel_size=0.2, want_labels=True,
              want_seg=False, want_full=False):
    """Folded transform_expand + stego k-means head (sd_seg_query) on dino (P, 64) f32 or
    bf16.  Returns (labels int32 (P) | None, seg uint8 (P) | None, dino_full (P, d_full) |
    None)."""
    lib = load()
    dt = SD_BF16 if dino.dtype == torch.bfloat16 else SD_F32
    _req(dino, "dino", torch.bfloat16 if dt == SD_BF16 else torch.float32)
    P = dino.shape[0]
    dev = dino.device
    labels = torch.empty(P, device=dev, dtype=torch.int32) if want_labels else None
    seg = torch.empty(P, device=dev, dtype=torch.uint8) if want_seg else None
    full = torch.empty(P, rec.d_full, device=dev) if want_full else None
    if want_seg:
        if sigma is None or sigma.numel() != P:
            raise ValueError("seg_query: want_seg needs sigma (P,)")
        _req(sigma, "sigma")
    _check(lib.sd_seg_query(ptr(dino), dt, P, ctypes.byref(rec), ptr(sigma), float(voxel_size),
                            ptr(labels), ptr(seg), ptr(full), stream_of(dino)), "sd_seg_query")
    return labels, seg, full


def composite(z, sigma, feat, rgb, hard_alpha_cap, want_weights=True):
    lib = load()
    R, K = z.shape
    dev = z.device
    F = feat.shape[-1] if feat is not None else 0
    Cc = rgb.shape[-1] if rgb is not None else 0
    weights = torch.empty(R, K, device=dev)
    alphas = torch.empty(R, K, device=dev)
    depth = torch.empty(R, device=dev)
    feat_out = torch.empty(R, F, device=dev) if feat is not None else None
    rgb_out = torch.empty(R, Cc, device=dev) if rgb is not None else None
    _check(lib.sd_composite(ptr(_req(z, "z")), ptr(_req(sigma, "sigma")),
                            ptr(feat if feat is None else _req(feat, "feat")), F,
                            ptr(rgb if rgb is None else _req(rgb, "rgb")), Cc, R, K,
                            int(bool(hard_alpha_cap)), ptr(weights), ptr(alphas), ptr(depth),
                            ptr(feat_out), ptr(rgb_out), stream_of(depth)), "sd_composite")
    return weights, alphas, depth, feat_out, rgb_out


def field_gather(xyz, grid_nhwc, cam_f, img=None, cam_c=None, colors=True,
                 dtype=torch.float32):
    """sd_field_gather: xyz (B,P,3), grid_nhwc (B,Hf,Wf,C) f32 -> x (B,P,C+40) = [feat|code|1],
    invalid_f (B,P) bool, rgb (B,P,3nv) | None, invalid (B,P,nv) | None."""
    lib = load()
    B, P, _ = xyz.shape
    _, Hf, Wf, C = grid_nhwc.shape
    dev = xyz.device
    x = torch.empty(B, P, C + 40, device=dev, dtype=dtype)
    invf = torch.empty(B, P, device=dev, dtype=torch.bool)
    nv, Hc, Wc = 0, 0, 0
    if colors:  # img: pack_image output (B*nv, Hc, Wc, 4); cam_c (B, nv, CAM_WORDS)
        nv, Hc, Wc = cam_c.shape[1], img.shape[1], img.shape[2]
    rgb = torch.empty(B, P, 3 * nv, device=dev) if colors else None
    inv = torch.empty(B, P, nv, device=dev) if colors else None
    _check(lib.sd_field_gather(ptr(_req(xyz, "xyz")), B, P, ptr(_req(grid_nhwc, "grid")), C, Hf,
                               Wf, ptr(_req(cam_f, "cam_f")), ptr(img), nv, Hc, Wc, ptr(cam_c),
                               ptr(x), SD_OF_TORCH[dtype], ptr(invf), ptr(rgb), ptr(inv),
                               stream_of(x)),
           "sd_field_gather")
    return x, invf, rgb, inv


def field_gather_bwd(xyz, dx, cam_f, Hf, Wf, C, dgrid=None):
    """sd_field_gather_bwd: dx (B,P,>=C) f32 / f16 / bf16 rows -> dgrid (B,Hf,Wf,C) f32
    (zeros, or accumulated into the given dgrid)."""
    lib = load()
    B, P, _ = xyz.shape
    if dx.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        dx = dx.float()
    dx = dx.contiguous()
    if dgrid is None:
        dgrid = torch.zeros(B, Hf, Wf, C, device=xyz.device)
    _req(dgrid, "dgrid")
    _check(lib.sd_field_gather_bwd(ptr(_req(xyz, "xyz")), B, P, ptr(dx), SD_OF_TORCH[dx.dtype],
                                   dx.shape[-1], C, Hf, Wf,
                                   ptr(_req(cam_f, "cam_f")), ptr(dgrid), stream_of(dgrid)),
           "sd_field_gather_bwd")
    return dgrid


def unpack_grid(grid_nhwc):
    """sd_unpack_grid: (B,H,W,C) f32 -> (B,C,H,W) f32."""
    lib = load()
    B, H, W, C = grid_nhwc.shape
    out = torch.empty(B, C, H, W, device=grid_nhwc.device)
    _check(lib.sd_unpack_grid(ptr(_req(grid_nhwc, "grid")), B, C, H, W, ptr(out),
                              stream_of(out)), "sd_unpack_grid")
    return out


def composite_bwd(z, sigma, feat, rgb, hard_alpha_cap, g_depth, g_feat, g_rgb, g_weights,
                  g_alphas, need_feat=True, need_rgb=False):
    """sd_composite_bwd -> d_sigma (R,K), d_feat (R,K,F) | None, d_rgb (R,K,Cc) | None."""
    lib = load()
    R, K = z.shape
    F = feat.shape[-1] if feat is not None else 0
    Cc = rgb.shape[-1] if rgb is not None else 0
    g = [None if t is None else _req(t.float().contiguous(), n) for t, n in
         ((g_depth, "g_depth"), (g_feat, "g_feat"), (g_rgb, "g_rgb"), (g_weights, "g_weights"),
          (g_alphas, "g_alphas"))]
    if feat is None:
        g[1] = None
    if rgb is None:
        g[2] = None
    d_sigma = torch.empty(R, K, device=z.device)
    d_feat = torch.empty(R, K, F, device=z.device) if (need_feat and g[1] is not None) else None
    d_rgb = torch.empty(R, K, Cc, device=z.device) if (need_rgb and g[2] is not None) else None
    _check(lib.sd_composite_bwd(ptr(_req(z, "z")), ptr(_req(sigma, "sigma")),
                                ptr(feat if feat is None else _req(feat, "feat")), F,
                                ptr(rgb if rgb is None else _req(rgb, "rgb")), Cc, R, K,
                                int(bool(hard_alpha_cap)), *[ptr(t) for t in g], ptr(d_sigma),
                                ptr(d_feat), ptr(d_rgb), stream_of(d_sigma)), "sd_composite_bwd")
    return d_sigma, d_feat, d_rgb


# ---------------------------------------------------------------------------
# ViT encoder kernels (sdhip_vit.hip)
# ---------------------------------------------------------------------------
def gemm(a, w, bias, epi, out=None, gamma=None, qkv=None, tokens=0, heads=0, pos=None,
         patches=0, grid_out=None):
    """sd_gemm: a (M, K) bf16 (row stride a.stride(0)), w (N, K) bf16 contiguous.
    SD_EPI_RESID with grid_out (B, tokens - 1, N)-shaped bf16: also writes the updated rows
    without each image's class token there (tokens_to_nhwc's output, no extra launch)."""
    lib = load()
    M, K = a.shape
    N = w.shape[0]
    if a.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or a.stride(1) != 1:
        raise TypeError("sd_gemm: a, w must be bf16 with unit inner stride")
    _req(w, "w", torch.bfloat16)
    g = SdGemmArgs(a=a.data_ptr(), lda=a.stride(0), w=w.data_ptr(),
                   bias=bias.data_ptr() if bias is not None else None, M=M, N=N, K=K, epi=epi,
                   out=out.data_ptr() if out is not None else None,
                   ldo=out.stride(-2) if out is not None else 0,
                   gamma=gamma.data_ptr() if gamma is not None else None)
    if qkv is not None:
        q, k, vt = qkv
        g.q, g.k, g.vt = q.data_ptr(), k.data_ptr(), vt.data_ptr()
        g.tokens, g.heads, g.head_dim, g.tokens_pad = tokens, heads, q.shape[-1], k.shape[-2]
    if pos is not None:
        g.pos, g.patches = pos.data_ptr(), patches
    if grid_out is not None:
        _req(grid_out, "grid_out", torch.bfloat16)
        if grid_out.numel() != (M // tokens) * (tokens - 1) * N:
            raise ValueError("sd_gemm: grid_out must hold (M / tokens) x (tokens - 1) x N values")
        g.q, g.tokens = grid_out.data_ptr(), tokens
    _check(lib.sd_gemm(ctypes.byref(g), stream_of(a)), "sd_gemm")


def ln_gemm(x, ln_w, ln_b, eps, w, bias, epi, out=None, qkv=None, tokens=0, heads=0):
    """sd_ln_gemm: LN(x) w^T + bias with the epilogue epi; x (M, C) f32, w (N, C) bf16."""
    lib = load()
    M, C = x.shape
    N = w.shape[0]
    _req(x, "x")
    _req(w, "w", torch.bfloat16)
    g = SdGemmArgs(a=None, lda=C, w=w.data_ptr(), bias=bias.data_ptr() if bias is not None else None,
                   M=M, N=N, K=C, epi=epi, out=out.data_ptr() if out is not None else None,
                   ldo=out.stride(-2) if out is not None else 0)
    if qkv is not None:
        q, k, vt = qkv
        g.q, g.k, g.vt = q.data_ptr(), k.data_ptr(), vt.data_ptr()
        g.tokens, g.heads, g.head_dim, g.tokens_pad = tokens, heads, q.shape[-1], k.shape[-2]
    _check(lib.sd_ln_gemm(ctypes.byref(g), ptr(x), ptr(_req(ln_w, "ln_w")), ptr(_req(ln_b, "ln_b")),
                          float(eps), stream_of(x)), "sd_ln_gemm")


def attention(q, k, vt, scale, out):
    lib = load()
    B, H, T, hd = q.shape
    _check(lib.sd_attention(ptr(q), ptr(k), ptr(vt), B, H, T, k.shape[-2], hd, float(scale),
                            ptr(out), stream_of(q)), "sd_attention")


def layernorm(x, w, b, eps, out):
    lib = load()
    rows, C = x.shape
    _check(lib.sd_layernorm(ptr(_req(x, "x")), rows, C, ptr(w), ptr(b), float(eps), ptr(out),
                            int(out.dtype == torch.float32), stream_of(x)), "sd_layernorm")


def patchify(img, p, Kp, mean, std, patches, cls, pos, x):
    lib = load()
    B, _, H, W = img.shape
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    sd = (ctypes.c_float * 3)(*[float(v) for v in std])
    _check(lib.sd_patchify(ptr(_req(img, "img")), B, H, W, p, Kp, m, sd, ptr(patches), ptr(cls),
                           ptr(pos), ptr(x), x.shape[-1], stream_of(img)), "sd_patchify")


def tokens_to_grid(x, B, T, C, n_prefix, gh, gw, l2norm):
    lib = load()
    out = torch.empty(B, C, gh, gw, device=x.device, dtype=torch.float32)
    _check(lib.sd_tokens_to_grid(ptr(_req(x, "x")), B, T, C, n_prefix, gh, gw, int(bool(l2norm)),
                                 ptr(out), stream_of(x)), "sd_tokens_to_grid")
    return out


# ---------------------------------------------------------------------------
# DPT decoder helpers
# ---------------------------------------------------------------------------
def conv3x3(x, w, bias, stride=1, relu_in=False, epi=None, out=None, res=None, res2=None):
    """Implicit-GEMM 3x3 convolution, padding 1: x (B, H, W, Cin) bf16 NHWC, w (Cout, 9 Cin)
    bf16 (k order ky, kx, ci) -> (B, OH, OW, Cout) bf16 (or f32 NCHW with epi=SD_EPI_NCHW)."""
    lib = load()
    B, H, W, Cin = x.shape
    _req(x, "x", torch.bfloat16)
    _req(w, "w", torch.bfloat16)
    Cout = w.shape[0]
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    epi = SD_EPI_BF16 if epi is None else epi
    M = B * OH * OW
    if out is None:
        out = (torch.empty(B, Cout, OH, OW, device=x.device) if epi == SD_EPI_NCHW else
               torch.empty(B, OH, OW, Cout, device=x.device,
                           dtype=torch.float32 if epi == SD_EPI_F32 else torch.bfloat16))
    g = SdGemmArgs(a=x.data_ptr(), lda=9 * Cin, w=w.data_ptr(),
                   bias=bias.data_ptr() if bias is not None else None, M=M, N=Cout, K=9 * Cin,
                   epi=epi, out=out.data_ptr(), ldo=Cout,
                   res=res.data_ptr() if res is not None else None,
                   res2=res2.data_ptr() if res2 is not None else None,
                   conv=1, H=H, W=W, Cin=Cin, stride=stride, OH=OH, OW=OW,
                   relu_in=int(bool(relu_in)), tokens=OH * OW)
    _check(lib.sd_gemm(ctypes.byref(g), stream_of(x)), "sd_gemm(conv3x3)")
    return out


def linear_nhwc(x, w, bias, epi=None, out=None, shuf=None, res=None):
    """1x1 convolution / ConvTranspose2d(k, stride k) on NHWC bf16 x (B, H, W, Cin):
    w (N, Cin) bf16.  shuf=k: SD_EPI_SHUF into (B, H k, W k, N / k^2)."""
    lib = load()
    B, H, W, Cin = x.shape
    _req(x, "x", torch.bfloat16)
    _req(w, "w", torch.bfloat16)
    N = w.shape[0]
    M = B * H * W
    if shuf is not None:
        epi = SD_EPI_SHUF
        out = torch.empty(B, H * shuf, W * shuf, N // (shuf * shuf), device=x.device,
                          dtype=torch.bfloat16) if out is None else out
    else:
        epi = SD_EPI_BF16 if epi is None else epi
        out = torch.empty(B, H, W, N, device=x.device, dtype=torch.bfloat16) if out is None else out
    g = SdGemmArgs(a=x.data_ptr(), lda=Cin, w=w.data_ptr(),
                   bias=bias.data_ptr() if bias is not None else None, M=M, N=N, K=Cin, epi=epi,
                   out=out.data_ptr(), ldo=N, res=res.data_ptr() if res is not None else None,
                   shuf_k=shuf or 0, in_h=H, in_w=W)
    _check(lib.sd_gemm(ctypes.byref(g), stream_of(x)), "sd_gemm(1x1)")
    return out


def layernorm_nhwc(x, w, b, eps, B, T, C, n_prefix, gh, gw, l2norm):
    """sd_layernorm_nhwc: LayerNorm of the non-prefix token rows of x (B T, C) f32 straight
    into a (B, gh, gw, C) bf16 grid (= layernorm(out_f32) + tokens_to_nhwc, one launch)."""
    lib = load()
    out = torch.empty(B, gh, gw, C, device=x.device, dtype=torch.bfloat16)
    _check(lib.sd_layernorm_nhwc(ptr(_req(x, "x")), B, T, C, ptr(_req(w, "w")), ptr(_req(b, "b")),
                                 float(eps), n_prefix, gh * gw, int(bool(l2norm)), ptr(out),
                                 stream_of(x)), "sd_layernorm_nhwc")
    return out


def tokens_to_nhwc(x, B, T, C, n_prefix, gh, gw, l2norm):
    lib = load()
    out = torch.empty(B, gh, gw, C, device=x.device, dtype=torch.bfloat16)
    _check(lib.sd_tokens_to_nhwc(ptr(_req(x, "x")), B, T, C, n_prefix, gh * gw, int(bool(l2norm)),
                                 ptr(out), stream_of(x)), "sd_tokens_to_nhwc")
    return out


def upsample2x(x):
    lib = load()
    B, H, W, C = x.shape
    out = torch.empty(B, 2 * H, 2 * W, C, device=x.device, dtype=torch.bfloat16)
    _check(lib.sd_upsample2x(ptr(_req(x, "x", torch.bfloat16)), B, H, W, C, ptr(out),
                             stream_of(x)), "sd_upsample2x")
    return out


# ---------------------------------------------------------------------------
# DPT decoder backward (sdhip_dpt_bwd.hip)
# ---------------------------------------------------------------------------
def conv_wgrad_args(B, H, W, Cin, Cout, taps=9, stride=1, relu_in=False, nparts=0):
    """sd_conv_wgrad_args of a shape (no pointers): for sd_conv_wgrad_parts / _work."""
    return SdConvWgradArgs(B=B, H=H, W=W, Cin=Cin, Cout=Cout, taps=taps, stride=stride,
                           relu_in=int(bool(relu_in)), nparts=nparts)


def conv_wgrad_parts(B, H, W, Cin, Cout, taps=9, stride=1):
    """Pixel parts sd_conv_wgrad uses for this shape on the current device."""
    lib = load()
    g = conv_wgrad_args(B, H, W, Cin, Cout, taps, stride)
    n = int(lib.sd_conv_wgrad_parts(ctypes.byref(g)))
    if n <= 0:
        _check(-1, "sd_conv_wgrad_parts")
    return n


def conv_wgrad(x, dy, taps=9, stride=1, relu_in=False, bias=True, nparts=None):
    """sd_conv_wgrad: x (B, H, W, Cin), dy (B, OH, OW, Cout) bf16 NHWC -> (dw (Cout, taps Cin)
    f32 in the packed (Cout, ky, kx, ci) order, db (Cout) f32 or None)."""
    lib = load()
    B, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    _req(x, "x", torch.bfloat16)
    _req(dy, "dy", torch.bfloat16)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    if tuple(dy.shape) != (B, OH, OW, Cout):
        raise ValueError(f"sd_conv_wgrad: dy must be {(B, OH, OW, Cout)}, got {tuple(dy.shape)}")
    g = conv_wgrad_args(B, H, W, Cin, Cout, taps, stride, relu_in)
    if nparts is None:
        nparts = int(lib.sd_conv_wgrad_parts(ctypes.byref(g)))
        if nparts <= 0:
            _check(-1, "sd_conv_wgrad_parts")
    g.nparts = int(nparts)
    nwork = int(lib.sd_conv_wgrad_work(ctypes.byref(g)))
    if nwork <= 0:
        _check(-1, "sd_conv_wgrad_work")
    work = torch.empty(nwork, device=x.device)
    dw = torch.empty(Cout, taps * Cin, device=x.device)
    db = torch.empty(Cout, device=x.device) if bias else None
    g.x, g.dy, g.work, g.dw = x.data_ptr(), dy.data_ptr(), work.data_ptr(), dw.data_ptr()
    g.db = db.data_ptr() if bias else None
    _check(lib.sd_conv_wgrad(ctypes.byref(g), stream_of(x)), "sd_conv_wgrad")
    return dw, db


def upsample2x_bwd(gout):
    """sd_upsample2x_bwd: gout (B, 2H, 2W, C) bf16 -> (B, H, W, C) bf16."""
    lib = load()
    B, OH, OW, C = gout.shape
    if OH % 2 or OW % 2:
        raise ValueError("sd_upsample2x_bwd: gout must be (B, 2H, 2W, C)")
    gin = torch.empty(B, OH // 2, OW // 2, C, device=gout.device, dtype=torch.bfloat16)
    _check(lib.sd_upsample2x_bwd(ptr(_req(gout, "gout", torch.bfloat16)), B, OH // 2, OW // 2, C,
                                 ptr(gin), stream_of(gout)), "sd_upsample2x_bwd")
    return gin


def relu_bwd(x, g, res=None):
    """sd_relu_bwd: (x > 0 ? g : 0) (+ res) on bf16 tensors of one shape."""
    lib = load()
    _req(x, "x", torch.bfloat16)
    _req(g, "g", torch.bfloat16)
    if g.shape != x.shape or (res is not None and _req(res, "res", torch.bfloat16).shape != x.shape):
        raise ValueError("sd_relu_bwd: x, g and res must have one shape")
    out = torch.empty_like(x)
    _check(lib.sd_relu_bwd(ptr(x), ptr(g), ptr(res), x.numel(), ptr(out), stream_of(x)),
           "sd_relu_bwd")
    return out


# ---------------------------------------------------------------------------
# ViT encoder backward (sdhip_vit_bwd.hip)
# ---------------------------------------------------------------------------
def attention_bwd(q, k, vt, ao, d_ao, scale, out=None):
    """sd_attention_bwd: q (B, H, T, 64), k (B, H, Tp, 64), vt (B, H, 64, Tp), ao / d_ao
    (B T, H 64) bf16 -> d_qkv (B T, 3 H 64) bf16, columns [dq | dk | dv] per head."""
    lib = load()
    B, H, T, hd = q.shape
    for t, n in ((q, "q"), (k, "k"), (vt, "vt"), (ao, "ao"), (d_ao, "d_ao")):
        _req(t, n, torch.bfloat16)
    if ao.numel() != B * T * H * hd or d_ao.numel() != ao.numel():
        raise ValueError("sd_attention_bwd: ao and d_ao must hold B x T x H x head_dim values")
    if out is None:
        out = torch.empty(B * T, 3 * H * hd, device=q.device, dtype=torch.bfloat16)
    _req(out, "d_qkv", torch.bfloat16)
    work = torch.empty(2 * B * H * T, device=q.device)
    g = SdAttnBwdArgs(q=q.data_ptr(), k=k.data_ptr(), vt=vt.data_ptr(), ao=ao.data_ptr(),
                      d_ao=d_ao.data_ptr(), d_qkv=out.data_ptr(), work=work.data_ptr(), B=B,
                      heads=H, tokens=T, tokens_pad=k.shape[-2], head_dim=hd, scale=float(scale))
    _check(lib.sd_attention_bwd(ctypes.byref(g), stream_of(q)), "sd_attention_bwd")
    return out


def layernorm_bwd(x, w, dy, eps, dx=None, accumulate=False, want_wb=True, nparts=None):
    """sd_layernorm_bwd: x (rows, C) f32 (the LayerNorm input), dy (rows, C) bf16 / f32 ->
    (dx f32 -- written, or added into the given dx with accumulate --, dw, db f32 | None)."""
    lib = load()
    rows, C = x.shape
    _req(x, "x")
    _req(w, "w")
    if dy.dtype not in (torch.bfloat16, torch.float32) or not dy.is_contiguous() or dy.shape != x.shape:
        raise TypeError("sd_layernorm_bwd: dy must be contiguous bf16 / f32 shaped as x")
    if dx is None:
        if accumulate:
            raise ValueError("sd_layernorm_bwd: accumulate needs the buffer to add into")
        dx = torch.empty_like(x)
    _req(dx, "dx")
    if dx.shape != x.shape:
        raise ValueError("sd_layernorm_bwd: dx must be shaped as x")
    if nparts is None:
        nparts = int(lib.sd_layernorm_bwd_parts(rows))
    work = torch.empty(int(nparts) * 2 * C, device=x.device)
    dw = torch.empty(C, device=x.device) if want_wb else None
    db = torch.empty(C, device=x.device) if want_wb else None
    g = SdLnBwdArgs(x=x.data_ptr(), w=w.data_ptr(), dy=dy.data_ptr(), rows=rows, C=C,
                    dy_f32=int(dy.dtype == torch.float32), accumulate=int(bool(accumulate)),
                    nparts=int(nparts), eps=float(eps), dx=dx.data_ptr(), work=work.data_ptr(),
                    dw=dw.data_ptr() if want_wb else None, db=db.data_ptr() if want_wb else None)
    _check(lib.sd_layernorm_bwd(ctypes.byref(g), stream_of(x)), "sd_layernorm_bwd")
    return dx, dw, db


def gelu_bwd(u, dh):
    """sd_gelu_bwd: dh * gelu_erf'(u) on bf16 tensors of one shape."""
    lib = load()
    _req(u, "u", torch.bfloat16)
    _req(dh, "dh", torch.bfloat16)
    if u.shape != dh.shape:
        raise ValueError("sd_gelu_bwd: u and dh must have one shape")
    out = torch.empty_like(u)
    _check(lib.sd_gelu_bwd(ptr(u), ptr(dh), u.numel(), ptr(out), stream_of(u)), "sd_gelu_bwd")
    return out


# ---------------------------------------------------------------------------
# transform_expand backward (sdhip_expand_bwd.hip)
# ---------------------------------------------------------------------------
def expand_bwd(x, rec: SdSegHead, pack, dy, want_w1=True, want_w2=True):
    """sd_expand_bwd: x (P, 64) f32 / bf16, the forward's record, pack (seg_pack.PackedExpandBwd
    of the same weights), dy (P, d_full) f32 -> (dx (P, 64) f32, h (P, 128), de (P, d_full),
    dh (P, 128), xb (P, 64)) -- the last four bf16 rows for the weight gradients: h and de only
    with want_w2, dh and xb only with want_w1 (None otherwise; xb is x itself if x is bf16)."""
    lib = load()
    dt = SD_BF16 if x.dtype == torch.bfloat16 else SD_F32
    _req(x, "x", torch.bfloat16 if dt == SD_BF16 else torch.float32)
    _req(dy, "dy")
    P, DF, dev, bf = x.shape[0], rec.d_full, x.device, torch.bfloat16
    if tuple(x.shape) != (P, 64) or tuple(dy.shape) != (P, DF) or pack.d_full != DF:
        raise ValueError(f"sd_expand_bwd: x must be (P, 64) and dy (P, {DF}); got "
                         f"{tuple(x.shape)}, {tuple(dy.shape)}")
    dx = torch.empty(P, 64, device=dev)
    h = torch.empty(P, 128, device=dev, dtype=bf) if want_w2 else None
    de = torch.empty(P, DF, device=dev, dtype=bf) if want_w2 else None
    dh = torch.empty(P, 128, device=dev, dtype=bf) if want_w1 else None
    xb = None
    if want_w1:
        xb = x if dt == SD_BF16 else torch.empty(P, 64, device=dev, dtype=bf)
    g = SdExpandBwdArgs(x=x.data_ptr(), dy=dy.data_ptr(), w1=pack.w1.data_ptr(),
                        w2=pack.w2.data_ptr(), w1t=pack.w1t.data_ptr(), w2t=pack.w2t.data_ptr(),
                        b1=pack.b1.data_ptr(), b2=pack.b2.data_ptr(), P=P, x_dtype=dt,
                        dx=dx.data_ptr(), h=ptr(h), de=ptr(de), dh=ptr(dh),
                        xb=ptr(xb) if dt == SD_F32 else None)
    _check(lib.sd_expand_bwd(ctypes.byref(g), ctypes.byref(rec), stream_of(x)), "sd_expand_bwd")
    return dx, h, de, dh, xb


# ---------------------------------------------------------------------------
# STEGO head training (sdhip_stego_train.hip, sdhip_probe.hip)
# ---------------------------------------------------------------------------
def _stego_args(pack, M, m_lin, m_non, rows_per_group):
    G = 0
    for m in (m_lin, m_non):
        if m is not None:
            _req(m, "dropout scales")
            if m.dim() != 2 or m.shape[1] != 64:
                raise ValueError("sd_stego_train: dropout scales must be (G, 64)")
            G = m.shape[0] if G == 0 else min(G, m.shape[0])
    return SdStegoTrainArgs(wl=pack.wl.data_ptr(), wn1=pack.wn1.data_ptr(), wn2=pack.wn2.data_ptr(),
                            wn2t=pack.wn2t.data_ptr(), bl=pack.bl.data_ptr(),
                            bn1=pack.bn1.data_ptr(), bn2=pack.bn2.data_ptr(), m_lin=ptr(m_lin),
                            m_non=ptr(m_non), M=M, rows_per_group=int(rows_per_group),
                            n_groups=G, d_in=pack.d_in, d_code=64)


def stego_train_fwd(x, pack, m_lin=None, m_non=None, rows_per_group=1, save=False,
                    normalize=True):
    """sd_stego_train_fwd: x (M, d_in) f32, pack (seg_pack.PackedStegoTrain) ->
    (y (M, 64) f32, saved) with saved = (xh, mid bf16 (M, d_in), e f32 (M, 64)) or None."""
    lib = load()
    _req(x, "x")
    M, dev = x.shape[0], x.device
    if x.dim() != 2 or x.shape[1] != pack.d_in:
        raise ValueError(f"sd_stego_train_fwd: x must be (M, {pack.d_in}), got {tuple(x.shape)}")
    g = _stego_args(pack, M, m_lin, m_non, rows_per_group)
    y = torch.empty(M, 64, device=dev)
    saved = None
    if save:
        saved = (torch.empty(M, pack.d_in, device=dev, dtype=torch.bfloat16),
                 torch.empty(M, pack.d_in, device=dev, dtype=torch.bfloat16),
                 torch.empty(M, 64, device=dev))
        g.xh, g.mid, g.e = (t.data_ptr() for t in saved)
    g.x, g.y, g.normalize = x.data_ptr(), y.data_ptr(), int(bool(normalize))
    _check(lib.sd_stego_train_fwd(ctypes.byref(g), stream_of(x)), "sd_stego_train_fwd")
    return y, saved


def stego_train_bwd(dy, saved, pack, m_lin=None, m_non=None, rows_per_group=1, want_lin=True,
                    want_non2=True, want_non1=True):
    """sd_stego_train_bwd: dy (M, 64) f32 and the forward's saved rows -> bf16 rows (dlin
    (M, 64), dnon (M, 64), dmid (M, d_in)), None where not wanted."""
    lib = load()
    _req(dy, "dy")
    xh, mid, e = saved
    M, dev, bf = e.shape[0], e.device, torch.bfloat16
    if tuple(dy.shape) != (M, 64):
        raise ValueError(f"sd_stego_train_bwd: dy must be {(M, 64)}, got {tuple(dy.shape)}")
    g = _stego_args(pack, M, m_lin, m_non, rows_per_group)
    dlin = torch.empty(M, 64, device=dev, dtype=bf) if want_lin else None
    dnon = torch.empty(M, 64, device=dev, dtype=bf) if want_non2 else None
    dmid = torch.empty(M, pack.d_in, device=dev, dtype=bf) if want_non1 else None
    g.e, g.mid, g.dy = e.data_ptr(), mid.data_ptr(), dy.data_ptr()
    g.dlin, g.dnon, g.dmid = ptr(dlin), ptr(dnon), ptr(dmid)
    _check(lib.sd_stego_train_bwd(ctypes.byref(g), stream_of(dy)), "sd_stego_train_bwd")
    return dlin, dnon, dmid


def cluster_probe(x, centres, m=None, rows_per_group=1, w=None):
    """sd_cluster_probe: x (N, d) f32 / bf16, centres (K, d) f32 L2-normalised, optional column
    scales m (G, d) and row weights w (N) -> (labels (N) int32, S (K, d) f32, counts (K) int32)."""
    lib = load()
    dt = SD_BF16 if x.dtype == torch.bfloat16 else SD_F32
    _req(x, "x", TORCH_DTYPE[dt])
    _req(centres, "centres")
    N, d = x.shape
    K, dev = centres.shape[0], x.device
    if centres.shape[1] != d or (m is not None and (_req(m, "m").dim() != 2 or m.shape[1] != d)) \
            or (w is not None and _req(w, "w").numel() != N):
        raise ValueError("sd_cluster_probe: centres (K, d), m (G, d), w (N) must match x (N, d)")
    nwork = int(lib.sd_cluster_probe_work(N, d, K))
    if nwork <= 0:
        _check(-1, "sd_cluster_probe_work")
    work = torch.empty(nwork, device=dev)
    labels = torch.empty(N, device=dev, dtype=torch.int32)
    S = torch.empty(K, d, device=dev)
    counts = torch.empty(K, device=dev, dtype=torch.int32)
    g = SdClusterProbeArgs(x=x.data_ptr(), m=ptr(m), centres=centres.data_ptr(), w=ptr(w), N=N,
                           rows_per_group=int(rows_per_group),
                           n_groups=m.shape[0] if m is not None else 0, d=d, K=K, x_dtype=dt,
                           work=work.data_ptr(), labels=labels.data_ptr(), S=S.data_ptr(),
                           counts=counts.data_ptr())
    _check(lib.sd_cluster_probe(ctypes.byref(g), stream_of(x)), "sd_cluster_probe")
    return labels, S, counts


def linear_probe(x, W, b, target=None, m=None, rows_per_group=1, normalize=True, want_grad=False,
                 want_row_loss=False):
    """sd_linear_probe: x (N, d) f32 / bf16, W (C, d) f32, b (C) f32, optional targets (N) of an
    integer dtype (rows outside [0, C) are ignored) and column scales m (G, d) ->
    (pred (N) int32, loss_sum (1) f32, n_valid (1) int32, gW (C, d), gb (C), row_loss (N)); an
    output that was not asked for (no target; want_grad / want_row_loss False) is None."""
    lib = load()
    dt = SD_BF16 if x.dtype == torch.bfloat16 else SD_F32
    _req(x, "x", TORCH_DTYPE[dt])
    _req(W, "W"), _req(b, "b")
    N, d = x.shape
    C, dev = W.shape[0], x.device
    if W.dim() != 2 or W.shape[1] != d or b.numel() != C \
            or (m is not None and (_req(m, "m").dim() != 2 or m.shape[1] != d)) \
            or (target is not None and target.numel() != N):
        raise ValueError("sd_linear_probe: W (C, d), b (C), m (G, d), target (N) must match x (N, d)")
    if target is None and (want_grad or want_row_loss):
        raise ValueError("sd_linear_probe: gradients and row losses need a target")
    nwork = int(lib.sd_linear_probe_work(N, d, C))
    if nwork <= 0:
        _check(-1, "sd_linear_probe_work")
    if target is not None:
        if target.is_floating_point() or target.dtype == torch.bool or target.device != dev:
            raise ValueError("sd_linear_probe: target must be an integer tensor on x's device")
        target = target.reshape(N).to(torch.int64).contiguous()
    work = torch.empty(nwork, device=dev)
    pred = torch.empty(N, device=dev, dtype=torch.int32)
    loss_sum = torch.empty(1, device=dev) if target is not None else None
    n_valid = torch.empty(1, device=dev, dtype=torch.int32) if target is not None else None
    gW = torch.empty(C, d, device=dev) if want_grad else None
    gb = torch.empty(C, device=dev) if want_grad else None
    row_loss = torch.empty(N, device=dev) if want_row_loss else None
    g = SdLinearProbeArgs(x=x.data_ptr(), m=ptr(m), W=W.data_ptr(), b=b.data_ptr(),
                          target=ptr(target), N=N, rows_per_group=int(rows_per_group),
                          n_groups=m.shape[0] if m is not None else 0, d=d, C=C, x_dtype=dt,
                          normalize=int(bool(normalize)), work=work.data_ptr(),
                          pred=pred.data_ptr(), loss_sum=ptr(loss_sum), n_valid=ptr(n_valid),
                          gW=ptr(gW), gb=ptr(gb), row_loss=ptr(row_loss))
    _check(lib.sd_linear_probe(ctypes.byref(g), stream_of(x)), "sd_linear_probe")
    return pred, loss_sum, n_valid, gW, gb, row_loss


# ---------------------------------------------------------------------------
# first-stage ReconstructionLoss (sdhip_recon_loss.hip)
# ---------------------------------------------------------------------------
SD_RL_POLICY_WEIGHT, SD_RL_POLICY_STRICT, SD_RL_POLICY_NONE = range(3)


def _recon_args(rgb, rgb_gt, invalid, weights, depth, dino, down, dino_gt, artifacts, cfg):
    P, h, w, nv, _ = rgb.shape
    _req(rgb, "rgb"), _req(rgb_gt, "rgb_gt")
    if tuple(rgb.shape) != (P, h, w, nv, 3) or tuple(rgb_gt.shape) != (P, h, w, 3):
        raise ValueError("sd_recon_loss: rgb must be (P, h, w, nv, 3) and rgb_gt (P, h, w, 3)")
    g = SdReconLossArgs(rgb=rgb.data_ptr(), rgb_gt=rgb_gt.data_ptr(), P=P, h=h, w=w, nv=nv,
                        policy=int(cfg["policy"]), lambda_coarse=cfg["lambda_coarse"],
                        lambda_dino=cfg["lambda_dino"], temperature=cfg["temperature"],
                        lambda_depth=cfg["lambda_depth"], lambda_dsmooth=cfg["lambda_dsmooth"])
    if g.policy != SD_RL_POLICY_NONE:
        K = invalid.shape[3]
        if tuple(_req(invalid, "invalid").shape) != (P, h, w, K, nv) or (
                g.policy == SD_RL_POLICY_WEIGHT
                and tuple(_req(weights, "weights").shape) != (P, h, w, K)):
            raise ValueError("sd_recon_loss: invalid must be (P, h, w, K, nv), weights (P, h, w, K)")
        g.invalid, g.K = invalid.data_ptr(), K
        if g.policy == SD_RL_POLICY_WEIGHT:
            g.weights = weights.data_ptr()
    if depth is not None:
        if tuple(_req(depth, "depth").shape) != (P, h, w):
            raise ValueError("sd_recon_loss: depth must be (P, h, w)")
        g.depth = depth.data_ptr()
    if dino is not None:
        dt = SD_BF16 if dino.dtype == torch.bfloat16 else SD_F32
        _req(dino, "dino", TORCH_DTYPE[dt])
        if dino.dim() != 4 or tuple(dino.shape[:3]) != (P, h, w):
            raise ValueError("sd_recon_loss: dino must be (P, h, w, C)")
        g.dino, g.C, g.dino_dtype = dino.data_ptr(), dino.shape[3], dt
    if down is not None:
        R, Cd = down.shape
        _req(down, "dino_down"), _req(dino_gt, "dino_gt")
        if tuple(dino_gt.shape) != (R, Cd) or (
                artifacts is not None and tuple(_req(artifacts, "dino_artifacts").shape) != (R, Cd)):
            raise ValueError("sd_recon_loss: dino_down, dino_gt, dino_artifacts must be (R, C)")
        g.dino_down, g.dino_gt, g.dino_artifacts = down.data_ptr(), dino_gt.data_ptr(), ptr(artifacts)
        g.R, g.Cd = R, Cd
    return g


def recon_loss_fwd(rgb, rgb_gt, invalid, weights, depth, dino, down, dino_gt, artifacts, cfg):
    """sd_recon_loss_fwd on patch-flattened tensors (include/sdhip.h) -> (rec () f32, terms (4)
    f32 = [rgb, cosine, depth smoothness, dino smoothness], state for recon_loss_bwd).  cfg:
    policy (SD_RL_POLICY_*), lambda_coarse, lambda_dino, temperature, lambda_depth,
    lambda_dsmooth.  depth / dino / down may be None (term absent)."""
    lib = load()
    g = _recon_args(rgb, rgb_gt, invalid, weights, depth, dino, down, dino_gt, artifacts, cfg)
    dev, npx = rgb.device, g.P * g.h * g.w
    nwork = int(lib.sd_recon_loss_work(g.P, g.C, g.R))
    if nwork <= 0:
        _check(-1, "sd_recon_loss_work")
    # one f32 buffer: [count | pad to 8 | dmean (P, padded to 4) | edge | work]
    o_dmean = 8
    o_edge = o_dmean + (g.P + 3) // 4 * 4
    o_work = o_edge + (2 * npx + 3) // 4 * 4
    buf = torch.empty(o_work + nwork, device=dev)
    sel = torch.empty(npx, device=dev, dtype=torch.int32)
    rec, terms = torch.empty((), device=dev), torch.empty(4, device=dev)
    base = buf.data_ptr()
    g.rec, g.terms, g.count = rec.data_ptr(), terms.data_ptr(), base
    g.dmean, g.edge, g.work = base + 4 * o_dmean, base + 4 * o_edge, base + 4 * o_work
    g.sel = sel.data_ptr()
    _check(lib.sd_recon_loss_fwd(ctypes.byref(g), stream_of(rgb)), "sd_recon_loss_fwd")
    return rec, terms, (buf, sel)


def recon_loss_bwd(g_rec, rgb, rgb_gt, depth, dino, down, dino_gt, artifacts, cfg, state, need):
    """sd_recon_loss_bwd: g_rec () f32 on the device, the forward's operands and state, need =
    (rgb, depth, dino, down) flags -> (d_rgb, d_depth, d_dino, d_down), None where not needed."""
    lib = load()
    cfg = dict(cfg, policy=SD_RL_POLICY_NONE)  # the mask is in the saved state
    g = _recon_args(rgb, rgb_gt, None, None, depth, dino, down, dino_gt, artifacts, cfg)
    buf, sel = state
    npx = g.P * g.h * g.w
    o_dmean = 8
    o_edge = o_dmean + (g.P + 3) // 4 * 4
    o_work = o_edge + (2 * npx + 3) // 4 * 4
    base = buf.data_ptr()
    g.count, g.dmean, g.edge, g.work = base, base + 4 * o_dmean, base + 4 * o_edge, base + 4 * o_work
    g.sel, g.g_rec = sel.data_ptr(), _req(g_rec, "g_rec").data_ptr()
    d_rgb = torch.empty_like(rgb) if need[0] else None
    d_depth = torch.empty_like(depth) if need[1] and depth is not None else None
    d_dino = torch.empty_like(dino) if need[2] and dino is not None else None
    d_down = torch.empty_like(down) if need[3] and down is not None else None
    g.d_rgb, g.d_depth, g.d_dino, g.d_down = ptr(d_rgb), ptr(d_depth), ptr(d_dino), ptr(d_down)
    _check(lib.sd_recon_loss_bwd(ctypes.byref(g), stream_of(rgb)), "sd_recon_loss_bwd")
    return d_rgb, d_depth, d_dino, d_down


# ---------------------------------------------------------------------------
# downstream-stage STEGO correlation loss (sdhip_stego_corr.hip)
# ---------------------------------------------------------------------------
def _stego_corr_args(dino_a, stego_a, partners, weights, shifts, pointwise):
    """partners: one (dino_b, stego_b) per pair, (None, None) for the self pair."""
    if dino_a.dim() != 3 or stego_a.dim() != 3 or not 1 <= len(partners) <= 3 \
            or len(weights) != len(partners) or len(shifts) != len(partners):
        raise ValueError("sd_stego_corr: dino_a (nc, P, d), stego_a (nc, P, code), 1..3 pairs with "
                         "a weight and a shift each")
    dt = {torch.float32: SD_F32, torch.bfloat16: SD_BF16}.get(dino_a.dtype, SD_F16)
    nc, P, d = dino_a.shape
    code = stego_a.shape[2]
    for t, name in ((dino_a, "dino_a"), (stego_a, "stego_a")):
        if not t.is_contiguous():
            raise ValueError(f"sd_stego_corr: {name} must be contiguous")
    _req(stego_a, "stego_a")
    if tuple(stego_a.shape[:2]) != (nc, P):
        raise ValueError("sd_stego_corr: stego_a must be (nc, P, code)")
    g = SdStegoCorrArgs(dino_a=dino_a.data_ptr(), stego_a=stego_a.data_ptr(), nc=nc, P=P, Q=P, d=d,
                        code_dim=code, n_pairs=len(partners), dino_dtype=dt,
                        pointwise=int(bool(pointwise)))
    Q = None
    for i, (db, sb) in enumerate(partners):
        g.weight[i], g.shift[i] = float(weights[i]), float(shifts[i])
        if db is None and sb is None:
            continue
        if db is None or sb is None or db.dtype != dino_a.dtype:
            raise ValueError("sd_stego_corr: a pair has both partner row sets of dino_a's dtype, or "
                             "neither (the self pair)")
        if not db.is_contiguous() or not _req(sb, "stego_b").is_contiguous():
            raise ValueError("sd_stego_corr: partner rows must be contiguous")
        if db.dim() != 3 or db.shape[0] != nc or db.shape[2] != d or tuple(sb.shape) != (
                nc, db.shape[1], code) or Q not in (None, db.shape[1]):
            raise ValueError("sd_stego_corr: partners must be (nc, Q, d) and (nc, Q, code), one Q")
        Q = db.shape[1]
        g.dino_b[i], g.stego_b[i] = db.data_ptr(), sb.data_ptr()
    if Q is not None:
        g.Q = Q
    return g


def stego_corr_fwd(dino_a, stego_a, partners, weights, shifts, pointwise):
    """sd_stego_corr_fwd (include/sdhip.h): dino_a (nc, P, d) f32 / bf16, stego_a (nc, P, 64) f32,
    partners = [(dino_b (nc, Q, d), stego_b (nc, Q, 64)) or (None, None) for the self pair] ->
    (loss (3) f32 on the device, work for stego_corr_bwd)."""
    lib = load()
    g = _stego_corr_args(dino_a, stego_a, partners, weights, shifts, pointwise)
    has_self = int(any(db is None for db, _ in partners))
    nbytes = int(lib.sd_stego_corr_work(g.nc, g.P, g.Q, g.d, g.n_pairs, has_self))
    nbytes = max(nbytes, 0)  # outside the domain: the call below reports why
    dev = dino_a.device
    work = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    loss = torch.empty(3, device=dev)
    g.work, g.work_bytes, g.loss = work.data_ptr(), nbytes, loss.data_ptr()
    _check(lib.sd_stego_corr_fwd(ctypes.byref(g), stream_of(dino_a)), "sd_stego_corr_fwd")
    return loss, work


def stego_corr_bwd(up, dino_a, stego_a, partners, weights, shifts, pointwise, work, need):
    """sd_stego_corr_bwd: up (3) f32 upstream gradients on the device, the forward's operands
    and work, need = (stego_a, partner 0, ...) flags -> (d_a, [d_b per pair]), None where not
    needed or for the self pair (its gradient is in d_a)."""
    lib = load()
    g = _stego_corr_args(dino_a, stego_a, partners, weights, shifts, pointwise)
    g.work, g.work_bytes = work.data_ptr(), work.numel()
    g.up = _req(up, "up").data_ptr()
    d_a = torch.empty_like(stego_a) if need[0] else None
    d_b = []
    for i, (db, sb) in enumerate(partners):
        d_b.append(torch.empty_like(sb) if sb is not None and need[1 + i] else None)
        g.d_b[i] = ptr(d_b[i])
    g.d_a = ptr(d_a)
    _check(lib.sd_stego_corr_bwd(ctypes.byref(g), stream_of(dino_a)), "sd_stego_corr_bwd")
    return d_a, d_b


# ---------------------------------------------------------------------------
# multi-scale-crop DINO targets (sdhip_msc.hip)
# ---------------------------------------------------------------------------
def msc_gt(feat, T, H, W, normalize=True):
    """sd_msc_gt: feat (B, V, C, hp, wp) f32 token grids (views 0..V-3 augmented, V-2 flipped,
    V-1 the image), T (B, V-2, 3, 3) f32 image -> augmented-view pixel homographies (None or
    empty at V = 2) -> out (B, C, H, W) f32, the valid-view mean, L2-normalised over C with
    ``normalize``."""
    lib = load()
    _req(feat, "feat")
    if feat.dim() != 5:
        raise ValueError(f"sd_msc_gt: feat must be (B, V, C, hp, wp), got {tuple(feat.shape)}")
    B, V, C, hp, wp = feat.shape
    if V > 2:
        if T is None or tuple(_req(T, "T").shape) != (B, V - 2, 3, 3) or T.device != feat.device:
            raise ValueError(f"sd_msc_gt: T must be ({B}, {V - 2}, 3, 3) on {feat.device}")
    out = torch.empty(B, C, int(H), int(W), device=feat.device)
    g = SdMscGtArgs(feat=feat.data_ptr(), T=T.data_ptr() if V > 2 else None, out=out.data_ptr(),
                    B=B, V=V, C=C, hp=hp, wp=wp, H=int(H), W=int(W), normalize=int(normalize))
    _check(lib.sd_msc_gt(ctypes.byref(g), stream_of(feat)), "sd_msc_gt")
    return out


# ---------------------------------------------------------------------------
# downstream-stage 3-D surface crops (sdhip_crop3d.hip)
# ---------------------------------------------------------------------------
def crop3d_centres(depth, poses, projs, z_far, u_pick, shift):
    """sd_crop3d_centres: depth (n, V, h, w), poses (n, V', 4, 4) c2w, projs (n, V', 3, 3), all
    f32 (view 0 of each is read), u_pick (n, n_crops) in [0, 1), shift (n, n_crops, S, 3) ->
    limits (n, n_crops + 1) f32, count (n, n_crops) i32, pixel (n, n_crops, 2) i32 (row, col; -1
    where the bin is empty), centre (n, n_crops, 3) f32, points (n, n_crops, S, 3) f32."""
    lib = load()
    _req(depth, "depth"), _req(poses, "poses"), _req(projs, "projs")
    _req(u_pick, "u_pick"), _req(shift, "shift")
    if depth.dim() != 4 or poses.dim() != 4 or projs.dim() != 4 or u_pick.dim() != 2:
        raise ValueError("sd_crop3d_centres: depth (n, V, h, w), poses (n, V, 4, 4), projs "
                         "(n, V, 3, 3), u_pick (n, n_crops)")
    n, _, h, w = depth.shape
    nc = u_pick.shape[1]
    if (tuple(poses.shape[::2]) != (n, 4) or poses.shape[3] != 4 or tuple(projs.shape[::2]) != (n, 3)
            or projs.shape[3] != 3 or u_pick.shape[0] != n or shift.dim() != 4
            or tuple(shift.shape[:2]) != (n, nc) or shift.shape[3] != 3
            or any(t.device != depth.device for t in (poses, projs, u_pick, shift))):
        raise ValueError("sd_crop3d_centres: operand shapes / devices do not match")
    S = shift.shape[2]
    dev = depth.device
    limits = torch.empty(n, nc + 1, device=dev)
    count = torch.empty(n, nc, device=dev, dtype=torch.int32)
    pixel = torch.empty(n, nc, 2, device=dev, dtype=torch.int32)
    centre = torch.empty(n, nc, 3, device=dev)
    points = torch.empty(n, nc, S, 3, device=dev)
    g = SdCrop3dArgs(depth=depth.data_ptr(), poses=poses.data_ptr(), projs=projs.data_ptr(),
                     u_pick=u_pick.data_ptr(), shift=shift.data_ptr(), limits=limits.data_ptr(),
                     count=count.data_ptr(), pixel=pixel.data_ptr(), centre=centre.data_ptr(),
                     points=points.data_ptr(), depth_stride=depth.stride(0),
                     pose_stride=poses.stride(0), proj_stride=projs.stride(0), n=n, h=h, w=w,
                     n_crops=nc, S=S, z_far=float(z_far))
    _check(lib.sd_crop3d_centres(ctypes.byref(g), stream_of(depth)), "sd_crop3d_centres")
    return limits, count, pixel, centre, points


def crop3d_compact(sigma, codes, crop_ok, thr, n_samples):
    """sd_crop3d_compact: sigma (C, S) f32, codes (C, S, D) f32 | bf16, crop_ok (C) i32 ->
    codes_out (C, n_samples, D), occ_out (C, n_samples) f32 = 1 - exp(-sigma), n_valid (1) i32,
    slot (C) i32.  Crops past n_valid are zero."""
    lib = load()
    _req(sigma, "sigma"), _req(crop_ok, "crop_ok", torch.int32)
    if codes.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"sd_crop3d_compact: codes must be float32 or bfloat16, got {codes.dtype}")
    _req(codes, "codes", codes.dtype)
    if (sigma.dim() != 2 or codes.dim() != 3 or tuple(codes.shape[:2]) != tuple(sigma.shape)
            or tuple(crop_ok.shape) != (sigma.shape[0],)
            or codes.device != sigma.device or crop_ok.device != sigma.device):
        raise ValueError("sd_crop3d_compact: sigma (C, S), codes (C, S, D), crop_ok (C)")
    C, S, D = codes.shape
    dev = sigma.device
    codes_out = torch.empty(C, int(n_samples), D, device=dev, dtype=codes.dtype)
    occ_out = torch.empty(C, int(n_samples), device=dev)
    n_valid = torch.empty(1, device=dev, dtype=torch.int32)
    slot = torch.empty(C, device=dev, dtype=torch.int32)
    g = SdCrop3dCompactArgs(sigma=sigma.data_ptr(), codes=codes.data_ptr(),
                            crop_ok=crop_ok.data_ptr(), codes_out=codes_out.data_ptr(),
                            occ_out=occ_out.data_ptr(), n_valid=n_valid.data_ptr(),
                            slot=slot.data_ptr(), C=C, S=S, D=D, n_samples=int(n_samples),
                            codes_dtype=SD_OF_TORCH[codes.dtype], thr=float(thr))
    _check(lib.sd_crop3d_compact(ctypes.byref(g), stream_of(sigma)), "sd_crop3d_compact")
    return codes_out, occ_out, n_valid, slot


def _image_rows(t, name):
    """(n, hw) view whose rows are contiguous -> its image stride in elements."""
    n, hw = t.shape
    if hw > 1 and t.stride(1) != 1:
        raise ValueError(f"scenedino_amd: {name} must have contiguous images")
    s = t.stride(0) if n > 1 else hw
    if s < hw or t.data_ptr() % 16:
        raise ValueError(f"scenedino_amd: {name} must be 16-byte aligned with image stride >= hw")
    return s


def depth_metrics(gt, pred, out=None, work=None):
    """sd_depth_metrics: gt, pred (n, hw) f32 views with contiguous rows (any image stride) ->
    out (n, 8) f32: abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, valid count."""
    lib = load()
    if gt.dtype != torch.float32 or pred.dtype != torch.float32:
        raise TypeError("sd_depth_metrics: gt and pred must be float32")
    if gt.dim() != 2 or gt.shape != pred.shape or gt.device != pred.device:
        raise ValueError("sd_depth_metrics: gt and pred (n, hw) on one device")
    n, hw = gt.shape
    sg, sp = _image_rows(gt, "gt"), _image_rows(pred, "pred")
    nbytes = int(lib.sd_depth_metrics_work(n, hw))
    if nbytes < 0:
        _check(-1, "sd_depth_metrics_work")
    if work is None:
        work = torch.empty(nbytes, device=gt.device, dtype=torch.uint8)
    if out is None:
        out = torch.empty(n, 8, device=gt.device, dtype=torch.float32)
    if work.numel() * work.element_size() < nbytes or not _req(out, "out").shape == (n, 8):
        raise ValueError("sd_depth_metrics: work too small or out not (n, 8)")
    _check(lib.sd_depth_metrics(ptr(gt), sg, ptr(pred), sp, n, hw, ptr(work), ptr(out),
                                stream_of(gt)), "sd_depth_metrics")
    return out


def dino_metrics(pred, gt, out=None, work=None):
    """sd_dino_metrics: pred (n, v, P, C) f32 | bf16, gt (n, v, P, C) f32, contiguous ->
    out (v + 1, 3) f32: l1, l2, cos per view, their means over the views in the last row."""
    lib = load()
    if pred.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"sd_dino_metrics: pred must be float32 or bfloat16, got {pred.dtype}")
    _req(pred, "pred", pred.dtype), _req(gt, "gt")
    if pred.dim() != 4 or pred.shape != gt.shape or pred.device != gt.device:
        raise ValueError("sd_dino_metrics: pred and gt (n, v, P, C) on one device")
    n, v, P, C = pred.shape
    nbytes = int(lib.sd_dino_metrics_work(n, v, P, C))
    if nbytes < 0:
        _check(-1, "sd_dino_metrics_work")
    if work is None:
        work = torch.empty(nbytes, device=gt.device, dtype=torch.uint8)
    if out is None:
        out = torch.empty(v + 1, 3, device=gt.device, dtype=torch.float32)
    if work.numel() * work.element_size() < nbytes or not _req(out, "out").shape == (v + 1, 3):
        raise ValueError("sd_dino_metrics: work too small or out not (v + 1, 3)")
    _check(lib.sd_dino_metrics(ptr(pred), SD_OF_TORCH[pred.dtype], ptr(gt), n, v, P, C, ptr(work),
                               ptr(out), stream_of(gt)), "sd_dino_metrics")
    return out


def seg_confusion(target, preds, gt_classes, n_classes, conf=None):
    """sd_seg_confusion: target (n, hw) int64 contiguous, preds a list of up to 8 (n, hw) int64
    views with contiguous rows (any image stride) -> conf (R gt_classes n_classes + 1) int32:
    the R matrices, then the count of pixels with an out-of-range label."""
    lib = load()
    _req(target, "target", torch.int64)
    R = len(preds)
    if target.dim() != 2 or not 1 <= R <= SEG_MAX_RESULTS:
        raise ValueError("sd_seg_confusion: target (n, hw) and 1 to 8 predictions")
    n, hw = target.shape
    g = SdSegConfusionArgs(target=target.data_ptr(), n=n, hw=hw, n_results=R,
                           gt_classes=int(gt_classes), n_classes=int(n_classes))
    for r, p in enumerate(preds):
        if p.dtype != torch.int64 or p.shape != target.shape or p.device != target.device:
            raise ValueError("sd_seg_confusion: predictions must be int64 (n, hw) on target's device")
        g.pred[r] = p.data_ptr()
        g.pred_stride[r] = _image_rows(p, "prediction")
    nbins = R * int(gt_classes) * int(n_classes)
    if gt_classes < 1 or n_classes < 1 or nbins > SEG_MAX_BINS:
        raise ValueError("sd_seg_confusion: n_results gt_classes n_classes must be in 1..8192")
    if conf is None:
        conf = torch.empty(nbins + 1, device=target.device, dtype=torch.int32)
    if not _req(conf, "conf", torch.int32).shape == (nbins + 1,):
        raise ValueError("sd_seg_confusion: conf must be (n_results gt_classes n_classes + 1) int32")
    g.conf = conf.data_ptr()
    _check(lib.sd_seg_confusion(ctypes.byref(g), stream_of(target)), "sd_seg_confusion")
    return conf


def dense_crf(image, unary, classes, iters, w_g, sxy_g, w_b, sxy_b, srgb, want_q=False, work=None):
    """sd_dense_crf: image (H, W, 3) uint8, unary (CT, H W) f32 (the results' class rows stacked,
    CT = sum(classes)), both contiguous -> (labels (R, H W) int64, Q (CT, H W) f32 or None)."""
    lib = load()
    _req(image, "image", torch.uint8), _req(unary, "unary")
    R = len(classes)
    if image.dim() != 3 or image.shape[2] != 3 or not 1 <= R <= CRF_MAX_RESULTS:
        raise ValueError("sd_dense_crf: image (H, W, 3) and 1 to 8 results")
    H, W = int(image.shape[0]), int(image.shape[1])
    N, CT = H * W, int(sum(classes))
    if tuple(unary.shape) != (CT, N) or unary.device != image.device:
        raise ValueError("sd_dense_crf: unary must be (sum(classes), H W) on the image's device")
    cls = (_i32 * CRF_MAX_RESULTS)(*[int(c) for c in classes])
    nbytes = int(lib.sd_dense_crf_work(H, W, R, cls))
    if nbytes < 0:
        _check(-1, "sd_dense_crf_work")
    if work is None:
        work = torch.empty(nbytes, device=image.device, dtype=torch.uint8)
    if work.numel() * work.element_size() < nbytes:
        raise ValueError("sd_dense_crf: work too small")
    labels = torch.empty(R, N, device=image.device, dtype=torch.int64)
    q = torch.empty(CT, N, device=image.device, dtype=torch.float32) if want_q else None
    a = SdCrfArgs(image=image.data_ptr(), unary=unary.data_ptr(), work=work.data_ptr(),
                  labels=labels.data_ptr(), q=None if q is None else q.data_ptr(), H=H, W=W,
                  n_results=R, iters=int(iters), classes=cls, w_g=w_g, sxy_g=sxy_g, w_b=w_b,
                  sxy_b=sxy_b, srgb=srgb)
    _check(lib.sd_dense_crf(ctypes.byref(a), stream_of(image)), "sd_dense_crf")
    return labels, q


def reserve_cus(n: int) -> int:
    """sd_reserve_cus: leave n CUs to other kernels (RCCL beside the render); previous value."""
    return int(load().sd_reserve_cus(int(n)))


def spin(nblocks: int, us: float, stream=None) -> None:
    """sd_spin (diagnostic): nblocks single-wave workgroups holding CUs for us microseconds."""
    s = stream if stream is not None else torch.cuda.current_stream()
    _check(load().sd_spin(int(nblocks), float(us), ctypes.c_void_p(s.cuda_stream)), "sd_spin")
