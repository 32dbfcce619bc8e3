"""ctypes binding of ``libnsff_hip.so`` (C-ABI declared in ``include/nsff_render.h``).

PyTorch is used here only as the owner of device memory and of the HIP stream; every
call below passes raw device pointers and the current stream handle to the library.
There is no CPU fallback: a missing library, a CPU tensor or a non-zero return code
raises ``RuntimeError``.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# NSFF_LIB overrides the library path (kernel A/B experiments only)
LIB_PATH = os.environ.get("NSFF_LIB") or os.path.join(_HERE, "libnsff_hip.so")

RAW_STRIDE = 16
ABI_VERSION = 32
MAX_FREQS = 24

_ERR = {-1: "NSFF_ERR_INVALID (bad shape/flag/unsupported architecture)",
        -2: "NSFF_ERR_NULL (required pointer missing)",
        -3: "NSFF_ERR_ALIGN (pointer not 16-byte aligned)",
        -4: "NSFF_ERR_HIP",
        -5: "NSFF_ERR_UNSUPPORTED (a valid request outside what the kernels are built for)"}

_fp = C.c_void_p  # device pointers travel as integers


class ModelDesc(C.Structure):
    _fields_ = [("D", C.c_int32), ("W", C.c_int32), ("skip", C.c_int32),
                ("in_xyz", C.c_int32), ("in_dir", C.c_int32), ("in_a", C.c_int32),
                ("in_t", C.c_int32), ("use_viewdir", C.c_int32),
                ("has_transient", C.c_int32), ("has_flow", C.c_int32),
                ("flow_scale", C.c_float), ("skip_mask", C.c_int32)]


class FieldArgs(C.Structure):
    _fields_ = [("n_points", C.c_int64), ("precision", C.c_int32), ("tile_points", C.c_int32),
                ("pts_per_ray", C.c_int32),
                ("static_mode", C.c_int32), ("transient_mode", C.c_int32),
                ("flow_heads", C.c_int32),
                ("xyz", _fp), ("n_freqs", C.c_int32), ("freqs", C.c_float * MAX_FREQS),
                ("dir_emb", _fp), ("a_emb", _fp), ("t_emb", _fp),
                ("x_emb", _fp), ("ld_emb", C.c_int32),
                ("off_xyz", C.c_int32), ("off_dir", C.c_int32), ("off_a", C.c_int32),
                ("off_t", C.c_int32), ("raw", _fp), ("save_acts", _fp), ("save_xin", _fp), ("save_masks", _fp),
                ("save_side", _fp), ("t_bias", _fp), ("t_bias_rows", C.c_int32), ("reserved0", C.c_int32),
                ("s_bias", _fp), ("s_bias_rows", C.c_int32), ("launch_form", C.c_int32), ("save_lo_delta", C.c_int64 * 3)]


class TimeBiasJob(C.Structure):
    _fields_ = [("desc", C.POINTER(ModelDesc)), ("w", _fp * 8), ("b", _fp * 8), ("t_rows", _fp), ("out", _fp),
                ("table", _fp), ("ts", _fp), ("n_table", C.c_int64), ("max_t", C.c_int64), ("delta", C.c_int32), ("pad_", C.c_int32),
                ("rows_out", _fp)]


MAX_TIME_BIAS_JOBS = 4


class RngJob(C.Structure):
    _fields_ = [("out", _fp), ("numel", C.c_int64), ("offset", C.c_uint64), ("kind", C.c_int32), ("grid", C.c_uint32)]


MAX_RNG_JOBS = 12


class RngCoarse(C.Structure):
    _fields_ = [("rays", _fp), ("z_lin", _fp), ("zs", _fp), ("xyz", _fp), ("n_samples", C.c_int32), ("perturb", C.c_float),
                ("job", C.c_int32), ("pad_", C.c_int32)]


_COMPOSITE_PTRS_IN = ["raw", "raw_fw", "raw_bw", "zs", "xyz", "xyz_fw", "xyz_bw",
                      "noise_static", "noise_transient", "noise_fw", "noise_bw", "visibility"]
_COMPOSITE_PTRS_OUT = ["static_rgbs", "transient_rgbs", "flows_fw", "flows_bw",
                       "static_sigmas", "transient_sigmas", "static_alphas", "transient_alphas",
                       "static_weights", "transient_weights", "weights",
                       "xyzs_fw_bw", "xyzs_bw_fw", "disoccs_fw", "disoccs_bw",
                       "depth", "rgb", "transient_alpha", "transient_rgb",
                       "static_only_rgb", "static_only_depth",
                       "xyz_exp", "flow_fw_exp", "flow_bw_exp", "xyz_fw_exp", "xyz_bw_exp",
                       "rgb_fw", "rgb_bw", "disocc_fw", "disocc_bw"]


class FrustumArgs(C.Structure):
    _fields_ = [("w2c", _fp), ("ts", _fp), ("K4", C.c_float * 4), ("n_cams", C.c_int32), ("n_frames", C.c_int32),
                ("H", C.c_int32), ("W", C.c_int32)]


class CompositeArgs(C.Structure):
    _fields_ = ([("n_rays", C.c_int64), ("n_samples", C.c_int32), ("has_transient", C.c_int32),
                 ("has_rgb", C.c_int32), ("flow_mode", C.c_int32), ("want_disocc", C.c_int32),
                 ("noise_std", C.c_float), ("z_far", C.c_float)]
                + [(n, _fp) for n in _COMPOSITE_PTRS_IN]
                + [(n, _fp) for n in _COMPOSITE_PTRS_OUT]
                + [("vis", FrustumArgs)])


_CBWD_IN = ["raw", "raw_fw", "raw_bw", "zs", "xyz", "f_fw", "f_bw", "noise_static", "noise_transient", "noise_fw", "noise_bw"]
_CBWD_G = ["g_static_sigmas", "g_transient_sigmas", "g_static_weights", "g_transient_weights", "g_weights", "g_depth",
           "g_rgb", "g_transient_alpha", "g_transient_rgb", "g_so_rgb", "g_so_depth", "g_xyz_exp", "g_flow_fw_exp",
           "g_flow_bw_exp", "g_rgb_fw", "g_rgb_bw"]
_CBWD_OUT = ["scratch", "d_raw", "d_raw_fw", "d_raw_bw", "d_f_fw", "d_f_bw"]


class CompositeBwdArgs(C.Structure):
    _fields_ = ([("n_rays", C.c_int64), ("n_samples", C.c_int32), ("has_transient", C.c_int32), ("flow_mode", C.c_int32),
                 ("noise_std", C.c_float)] + [(n, _fp) for n in _CBWD_IN + _CBWD_G + _CBWD_OUT])


class FieldBwdArgs(C.Structure):
    _fields_ = [("n_points", C.c_int64), ("static_mode", C.c_int32), ("transient_mode", C.c_int32),
                ("d_raw", _fp), ("raw", _fp), ("gmax", _fp), ("masks", _fp), ("dpre", _fp), ("dhead", _fp),
                ("d_xin", _fp), ("d_side", _fp), ("dpre_lo_delta", C.c_int64)]


class WgradJob(C.Structure):
    _fields_ = [("a", _fp), ("b", _fp), ("a_rows", C.c_int32), ("b_rows", C.c_int32), ("out_off", C.c_int64), ("trunk", C.c_int32),
                ("pad_", C.c_int32), ("a_lo_delta", C.c_int64), ("b_lo_delta", C.c_int64)]


class FoldGradArgs(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("pad_", C.c_int32), ("g", _fp), ("gb", _fp), ("w_final", _fp), ("b_final", _fp),
                ("w_head", _fp * 16), ("d_w_head", _fp * 16), ("d_b_head", _fp * 16), ("d_w_final", _fp), ("d_b_final", _fp)]


class FoldDenseArgs(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("accumulate", C.c_int32), ("ld_head", C.c_int32), ("ld_dhead", C.c_int32),
                ("g", _fp), ("g2", _fp), ("gb", _fp), ("gb2", _fp), ("w_head", _fp), ("w_final", _fp), ("b_final", _fp),
                ("d_w_head", _fp), ("d_b_head", _fp), ("d_w_final", _fp), ("d_b_final", _fp)]


class SplatArgs(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("n_planes", C.c_int32), ("K4", C.c_float * 4),
                ("P", C.c_float * 12), ("scale", C.c_float),
                ("xyz", _fp), ("flow", _fp), ("rgb", _fp), ("alpha", _fp), ("accum", _fp), ("work", _fp),
                ("work_bytes", C.c_int64)]


class MpiArgs(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("n_planes", C.c_int32), ("dt", C.c_float),
                ("accum_fw", _fp), ("accum_bw", _fp), ("static_rgb", _fp), ("static_alpha", _fp), ("zs", _fp),
                ("rgb", _fp), ("depth", _fp)]


_LOSS_IN = ["rgb_fine", "rgb_coarse", "depth_fine", "depth_coarse", "t_weights", "s_weights", "xyz_fw", "xyz_bw", "rgb_fw",
            "rgb_bw", "disocc_fw", "disocc_bw", "disoccs_fw", "disoccs_bw", "xyzs_fw_bw", "xyzs_bw_fw", "xyzs_fine",
            "xyzs_fw", "xyzs_bw", "rgbs", "disps", "ts", "cam_ids", "uv_fw", "uv_bw", "Ks", "Ps", "hyper", "stats", "terms",
            "term_w"]
LOSS_GRADS = ["g_rgb_fine", "g_rgb_coarse", "g_depth_fine", "g_depth_coarse", "g_t_weights", "g_s_weights", "g_xyz_fw",
              "g_xyz_bw", "g_rgb_fw", "g_rgb_bw", "g_xyzs_fw_bw", "g_xyzs_bw_fw", "g_xyzs_fw", "g_xyzs_bw"]


class LossArgs(C.Structure):
    _fields_ = ([("n_rays", C.c_int64), ("n_samples", C.c_int32), ("n_keep", C.c_int32), ("n_frames", C.c_int32),
                 ("max_t", C.c_int32), ("topk", C.c_double), ("thickness", C.c_int32), ("pad_", C.c_int32)]
                + [(n, _fp) for n in _LOSS_IN] + [("weights", _fp), ("per_ray", _fp), ("coef", _fp)]
                + [(n, _fp) for n in LOSS_GRADS])


class FlowGradArgs(C.Structure):
    _fields_ = [("n_points", C.c_int64), ("zs", _fp), ("z_far", C.c_float), ("accumulate", C.c_int32), ("col_a", C.c_int32),
                ("col_b", C.c_int32), ("pad_", C.c_int32), ("g_a", _fp * 4), ("g_b", _fp * 4), ("out", _fp)]


class SsimArgs(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("window", C.c_int32),
                ("gt", _fp), ("pred", _fp), ("mask", _fp), ("map", _fp), ("mean_map", _fp), ("sums", _fp),
                ("scratch", _fp), ("scratch_bytes", C.c_int64)]


class LpipsWeights(C.Structure):
    _fields_ = [("conv_w", _fp * 5), ("conv_b", _fp * 5), ("lin", _fp * 5)]


class LpipsArgs(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("normalize", C.c_int32),
                ("gt", _fp), ("pred", _fp), ("valid", _fp), ("packed", _fp), ("map", _fp), ("sums", _fp),
                ("workspace", _fp), ("workspace_bytes", C.c_int64)]


_FINISH_PTRS = ["rgb", "gt", "valid", "depth", "lut", "rgb_clipped", "rgb_u8", "sums", "depth_range", "depth_u8", "depth_rgb_u8"]


class FrameFinishArgs(C.Structure):
    _fields_ = ([("n_frames", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("pad_", C.c_int32)]
                + [(n, _fp) for n in _FINISH_PTRS] + [("scratch", _fp), ("scratch_bytes", C.c_int64)])


_PANEL_IN = ["gt", "pred", "depth", "transient_alpha", "static_rgb", "static_depth", "mask", "disp", "ssim_loss"]
_PANEL_LUT = ["lut_depth", "lut_mask"]
_PANEL_OUT = ["ranges", "grid_u8", "rmse_u8", "ssim_u8", "rmse_blend_u8", "ssim_blend_u8"]
PANEL_FIELDS = ("depth", "static_depth", "neg_disp", "neg_rmse", "neg_ssim")          # the rows of `ranges`


class ValPanelsArgs(C.Structure):
    _fields_ = ([("n_frames", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("pad_", C.c_int32)]
                + [(n, _fp) for n in _PANEL_IN + _PANEL_LUT + _PANEL_OUT] + [("scratch", _fp), ("scratch_bytes", C.c_int64)])


FLOW_UNKNOWN = 1e10           # NSFF_FLOW_UNKNOWN: both components of an induced-flow pixel without a valid projection


class FlowMapsArgs(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("n_poses", C.c_int32), ("max_t", C.c_int32),
                ("share_gt_scale", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("xyz", _fp * 2), ("Ps", _fp), ("ts", _fp), ("flow", _fp * 2), ("gt", _fp * 2), ("mask", _fp),
                ("epe_sums", _fp), ("epe_counts", _fp), ("maxrad", _fp), ("scale", _fp), ("image", _fp * 2), ("gt_image", _fp * 2),
                ("scratch", _fp), ("scratch_bytes", C.c_int64)]


TRACK_MAX_POINTS, TRACK_MAX_TRACKS, TRACK_MAX_STEPS = 0x7fffffff, 1 << 20, 1 << 11      # NSFF_TRACK_MAX_*


class TrackStepArgs(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("pts_per_row", C.c_int32), ("direction", C.c_int32), ("max_t", C.c_int32),
                ("n_poses", C.c_int32), ("fixed_view", C.c_int32), ("pad_", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("raw", _fp), ("xyz_in", _fp), ("t_in", _fp), ("alive_in", _fp), ("xyz_out", _fp), ("t_out", _fp), ("alive_out", _fp),
                ("Ps", _fp), ("uv", _fp), ("depth", _fp)]


class TrackDrawArgs(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("n_steps", C.c_int32), ("n_tracks", C.c_int32),
                ("uv", _fp), ("ok", _fp), ("image", _fp), ("lut", _fp), ("out", _fp), ("scratch", _fp), ("scratch_bytes", C.c_int64)]


ERODE_MAX_K = 31              # NSFF_ERODE_MAX_K


class MotionMapsArgs(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("epipolar", C.c_int32),
                ("alpha", C.c_float), ("beta", C.c_float), ("threshold", C.c_float), ("pad_", C.c_float),
                ("flow_fw", _fp), ("flow_bw", _fp), ("Fm", _fp), ("err", _fp), ("valid", _fp), ("raw", _fp),
                ("counts", _fp), ("err_sums", _fp), ("scratch", _fp), ("scratch_bytes", C.c_int64)]


class MaskErodeArgs(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("k", C.c_int32),
                ("src", _fp), ("dst", _fp), ("zero_counts", _fp), ("scratch", _fp), ("scratch_bytes", C.c_int64)]


OPTFLOW_MIN_SIZE, OPTFLOW_TILE, OPTFLOW_K, OPTFLOW_FUSED = 16, 32, 3, 1       # NSFF_OPTFLOW_*
OPTFLOW_PAIRS = ((16, 2), (32, 2), (32, 3), (32, 4), (32, 6))                # the (tile, k) the fused iteration is built for


class OptflowIterArgs(C.Structure):
    _fields_ = [("n_pairs", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("iters", C.c_int32),
                ("fused", C.c_int32), ("tile", C.c_int32), ("k", C.c_int32), ("pad_", C.c_int32),
                ("lam", C.c_float), ("theta", C.c_float), ("tau", C.c_float), ("pad1_", C.c_float),
                ("consts", _fp), ("state", _fp * 2)]


class OptflowArgs(C.Structure):
    _fields_ = [("n_pairs", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("channels", C.c_int32),
                ("levels", C.c_int32), ("warps", C.c_int32), ("iters", C.c_int32), ("median", C.c_int32),
                ("fused", C.c_int32), ("tile", C.c_int32), ("k", C.c_int32), ("pad_", C.c_int32),
                ("lam", C.c_float), ("theta", C.c_float), ("tau", C.c_float), ("pad1_", C.c_float),
                ("images0", _fp), ("images1", _fp), ("flow", _fp), ("scratch", _fp), ("scratch_bytes", C.c_int64)]


DISPARITY_TILE, DISPARITY_K, DISPARITY_FUSED = 32, 3, 1                        # NSFF_DISPARITY_*
DISPARITY_PAIRS = ((16, 2), (32, 2), (32, 3), (32, 4), (32, 6))               # the (tile, k) the fused relaxation is built for


class DisparitySparseArgs(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("min_parallax", C.c_float),
                ("flow_fw", _fp), ("flow_bw", _fp), ("Pm", _fp), ("valid", _fp), ("masks", _fp), ("n", _fp), ("c", _fp), ("counts", _fp),
                ("scratch", _fp), ("scratch_bytes", C.c_int64)]


class DisparityRelaxArgs(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("iters", C.c_int32),
                ("fused", C.c_int32), ("tile", C.c_int32), ("k", C.c_int32), ("pad_", C.c_int32),
                ("lam", C.c_float), ("sigma", C.c_float), ("n", _fp), ("c", _fp), ("grey", _fp), ("state", _fp * 2)]


class DisparityDenseArgs(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("levels", C.c_int32),
                ("iters", C.c_int32), ("fused", C.c_int32), ("tile", C.c_int32), ("k", C.c_int32),
                ("lam", C.c_float), ("sigma", C.c_float), ("n", _fp), ("c", _fp), ("grey", _fp), ("disps", _fp),
                ("scratch", _fp), ("scratch_bytes", C.c_int64)]


DISPARITY_MAX_SPAN = 8                                                        # NSFF_DISPARITY_MAX_SPAN


class DisparitySpanArgs(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("span", C.c_int32),
                ("min_parallax", C.c_float), ("pad_", C.c_int32),
                ("flow_fw", _fp), ("flow_bw", _fp), ("Pm", _fp), ("valid", _fp), ("masks", _fp), ("n", _fp), ("c", _fp), ("votes", _fp),
                ("counts", _fp), ("scratch", _fp), ("scratch_bytes", C.c_int64)]

MOTION_MAX_SPAN, PROPAGATE_MAX_REACH = 8, 8                                   # NSFF_MOTION_MAX_SPAN, NSFF_PROPAGATE_MAX_REACH


class MotionSpanArgs(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("span", C.c_int32),
                ("threshold", C.c_float), ("pad_", C.c_int32),
                ("flow_fw", _fp), ("flow_bw", _fp), ("Fm", _fp), ("hop_scale", _fp), ("valid", _fp),
                ("err", _fp), ("hops", _fp), ("raw", _fp), ("counts", _fp), ("scratch", _fp), ("scratch_bytes", C.c_int64)]


class MaskPropagateArgs(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("reach", C.c_int32),
                ("src", _fp), ("flow_fw", _fp), ("flow_bw", _fp), ("valid", _fp), ("dst", _fp), ("hits", _fp), ("zero_counts", _fp),
                ("scratch", _fp), ("scratch_bytes", C.c_int64)]


FLOW_MEDIAN_MAX_RADIUS, FLOW_MEDIAN_TILED = 7, 1                              # NSFF_FLOW_MEDIAN_*


class FlowMedianArgs(C.Structure):
    _fields_ = [("n_pairs", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("radius", C.c_int32),
                ("sigma_i", C.c_float), ("sigma_s", C.c_float), ("tiled", C.c_int32), ("pad_", C.c_int32),
                ("flow", _fp), ("grey", _fp), ("valid", _fp), ("out", _fp)]


RAY_RECORD = 16
_DRAW_OUT =["rays", "rgbs", "ts", "cam_ids", "disps", "rays_mask", "uv_fw", "uv_bw", "rand_idx"]


class RayDrawArgs(C.Structure):
    _fields_ = ([("n_frames", C.c_int64), ("n_pixels", C.c_int64), ("frame", C.c_int64), ("batch", C.c_int64),
                 ("records", _fp), ("cdf", _fp), ("u", _fp)] + [(n, _fp) for n in _DRAW_OUT])


FRAME_TABLE = 16                # floats per frame of nsff_ray_records' table: c2w (3,4) row-major | shift_near | 3 unused


class RayRecordArgs(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("first_frame", C.c_int32),
                ("frame_count", C.c_int32), ("image_u8", C.c_int32), ("mask_u8", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("near", C.c_float),
                ("n_pixels", C.c_int64), ("images", _fp), ("disps", _fp), ("masks", _fp), ("flow_fw", _fp), ("flow_bw", _fp),
                ("frame_table", _fp), ("records", _fp)]


RESIZE_LANCZOS_U8, RESIZE_NEAREST_PIL, RESIZE_NEAREST_CV, RESIZE_LINEAR_CV = range(4)      # NSFF_RESIZE_*
RESIZE_MAX_KSIZE = 49
ERR_UNSUPPORTED = -5


class FrameResizeArgs(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("filter", C.c_int32), ("channels", C.c_int32), ("pad_", C.c_int32),
                ("src_h", C.c_int32), ("src_w", C.c_int32), ("dst_h", C.c_int32), ("dst_w", C.c_int32),
                ("ksize_x", C.c_int32), ("ksize_y", C.c_int32), ("ratio", C.c_float * 2), ("src", _fp), ("dst", _fp),
                ("x_start", _fp), ("x_count", _fp), ("x_weights", _fp), ("y_start", _fp), ("y_count", _fp), ("y_weights", _fp)]


class SceneScaleArgs(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("n_points", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("disp_rank", C.c_int32 * 2), ("points", _fp), ("vis", _fp), ("w2c", _fp), ("K", _fp), ("disps", _fp),
                ("stats", _fp), ("disp_os", _fp), ("depth_os", _fp), ("pix", _fp), ("work", _fp), ("work_bytes", C.c_int64)]


# name -> (restype, argtypes); also the list of symbols the header declares
_SIGNATURES = {
    "nsff_abi_version": (C.c_int, []),
    "nsff_range_flags": (C.c_int, [_fp, C.c_int32, _fp]),
    "nsff_last_field_kernel": (C.c_int, []),
    "nsff_last_field_grid": (C.c_int, []),
    "nsff_field_mfma_shape": (C.c_int, [C.POINTER(ModelDesc), C.POINTER(FieldArgs)]),
    "nsff_repack_field_weights": (C.c_int, [C.POINTER(ModelDesc), _fp, _fp, _fp]),
    "nsff_field_query_repacked": (C.c_int, [C.POINTER(ModelDesc), _fp, _fp, C.POINTER(FieldArgs), _fp]),
    "nsff_last_field_mfma_shape": (C.c_int, []),
    "nsff_field_phase_program": (C.c_int, [C.POINTER(ModelDesc), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int),
                                   C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "nsff_field_launch_plan": (C.c_int, [C.POINTER(ModelDesc), C.POINTER(FieldArgs), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "nsff_time_bias_rows": (C.c_int, [C.POINTER(ModelDesc)]),
    "nsff_time_bias": (C.c_int, [C.POINTER(TimeBiasJob), C.c_int32, C.c_int64, C.c_void_p]),
    "nsff_rng_draws": (C.c_int, [C.POINTER(RngJob), C.c_int32, C.c_uint64, C.c_void_p]),
    "nsff_rng_draws_coarse": (C.c_int, [C.POINTER(RngJob), C.c_int32, C.c_uint64, C.POINTER(RngCoarse), C.c_void_p]),
    "nsff_side_bias": (C.c_int, [C.POINTER(ModelDesc), _fp, _fp, _fp, _fp, C.c_int64, _fp, C.c_void_p]),
    "nsff_last_hip_error": (C.c_char_p, []),
    "nsff_packed_bytes": (C.c_int, [C.POINTER(ModelDesc), C.c_int, C.POINTER(C.c_size_t)]),
    "nsff_param_count": (C.c_int, [C.POINTER(ModelDesc)]),
    "nsff_pack_weights": (C.c_int, [C.POINTER(ModelDesc), C.c_int, C.POINTER(_fp), _fp, _fp]),
    "nsff_pack_weights_ex": (C.c_int, [C.POINTER(ModelDesc), C.c_int, C.POINTER(_fp), _fp, C.c_int32, _fp]),
    "nsff_fold_heads": (C.c_int, [C.POINTER(ModelDesc), C.c_int, C.POINTER(_fp), _fp, _fp]),
    "nsff_posenc": (C.c_int, [_fp, C.c_int64, C.POINTER(C.c_float), C.c_int, _fp, _fp]),
    "nsff_time_rows": (C.c_int, [_fp, C.c_int64, C.c_int32, _fp, C.c_int64, C.c_int64, _fp, _fp, _fp]),
    "nsff_time_rows_backward": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int64, C.c_int64, C.c_int64, C.c_int32, _fp, _fp]),
    "nsff_field_query": (C.c_int, [C.POINTER(ModelDesc), _fp, C.POINTER(FieldArgs), _fp]),
    "nsff_coarse_samples": (C.c_int, [_fp, C.c_int64, _fp, C.c_int32, C.c_float, _fp, _fp, _fp, _fp]),
    "nsff_fine_samples": (C.c_int, [_fp, C.c_int64, _fp, _fp, C.c_int32, C.c_int32, _fp, _fp, _fp, _fp,
                                    C.c_int32, _fp, _fp, _fp, _fp, _fp]),
    "nsff_sample_pdf": (C.c_int, [_fp, _fp, C.c_int64, C.c_int32, _fp, C.c_int32, C.c_int32,
                                  C.c_float, _fp, _fp]),
    "nsff_warp_points": (C.c_int, [_fp, _fp, _fp, C.c_int64, C.c_float, _fp, _fp, _fp]),
    "nsff_composite": (C.c_int, [C.POINTER(CompositeArgs), _fp]),
    "nsff_frustum_visibility": (C.c_int, [C.POINTER(FrustumArgs), _fp, C.c_int64, _fp, _fp]),
    "nsff_frame_rays": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32, C.c_int32, C.c_float,
                                  C.c_float, C.c_int64, C.c_int64, _fp, _fp]),
    "nsff_ray_records": (C.c_int, [C.POINTER(RayRecordArgs), _fp]),
    "nsff_resize_ksize": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "nsff_resize_table": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nsff_frame_resize": (C.c_int, [C.POINTER(FrameResizeArgs), _fp]),
    "nsff_scene_scale_work_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "nsff_scene_scale": (C.c_int, [C.POINTER(SceneScaleArgs), _fp]),
    "nsff_bwd_packed_bytes": (C.c_int, [C.POINTER(ModelDesc), C.POINTER(C.c_size_t)]),
    "nsff_pack_weights_bwd": (C.c_int, [C.POINTER(ModelDesc), C.POINTER(_fp), _fp, _fp]),
    "nsff_field_backward": (C.c_int, [C.POINTER(ModelDesc), _fp, C.POINTER(FieldBwdArgs), _fp]),
    "nsff_field_input_backward": (C.c_int, [_fp, C.c_int32, C.c_int32, _fp, C.c_int64, C.c_int32, C.POINTER(C.c_float), C.c_int32,
                                            C.c_int32, _fp, _fp, _fp]),
    "nsff_train_dims": (C.c_int, [C.POINTER(ModelDesc), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "nsff_weight_grad_scratch": (C.c_int64, [C.POINTER(WgradJob), C.c_int32, C.c_int64, C.c_int32]),
    "nsff_weight_grad": (C.c_int, [C.POINTER(WgradJob), C.c_int32, C.c_int64, C.c_int32, _fp, _fp, _fp, _fp, _fp]),
    "nsff_weight_grad_accumulate": (C.c_int, [C.POINTER(WgradJob), C.c_int32, C.c_int64, C.c_int32, _fp, _fp, C.c_int64,
                                              _fp, _fp, _fp]),
    "nsff_weight_grad_accumulate_aux": (C.c_int, [C.POINTER(WgradJob), C.c_int32, C.c_int64, C.c_int32, _fp, _fp, C.c_int64,
                                                  _fp, _fp, _fp, _fp]),
    "nsff_absmax_raw": (C.c_int, [_fp, C.c_int64, _fp, _fp]),
    "nsff_last_bwd_kernel": (C.c_int, []),
    "nsff_last_bwd_grid": (C.c_int, []),
    "nsff_field_bwd_phase_program": (C.c_int, [C.POINTER(ModelDesc), C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_uint32), C.c_int32,
                                                C.POINTER(C.c_uint32), C.c_int32]),
    "nsff_field_bwd_launch_plan": (C.c_int, [C.POINTER(ModelDesc), C.POINTER(FieldBwdArgs), C.c_int32, C.c_int32, C.c_int32,
                                             C.POINTER(C.c_int32), C.c_int32]),
    "nsff_fold_grads": (C.c_int, [C.POINTER(FoldGradArgs), _fp]),
    "nsff_fold_grads_dense": (C.c_int, [C.POINTER(FoldDenseArgs), _fp]),
    "nsff_pack_weights_bwd_ex": (C.c_int, [C.POINTER(ModelDesc), C.POINTER(_fp), _fp, _fp, _fp]),
    "nsff_absmax": (C.c_int, [_fp, C.c_int64, _fp, _fp]),
    "nsff_adam_step": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int64, _fp, _fp, C.c_double, C.c_double, C.c_double, C.c_double, _fp]),
    "nsff_adam_step_segments": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int64, _fp, _fp, C.c_double, C.c_double, C.c_double, C.c_double,
                                          _fp, C.c_int, _fp, _fp]),
    "nsff_sgd_step": (C.c_int, [_fp, _fp, _fp, C.c_int64, _fp, _fp, C.c_double, C.c_double, _fp, C.c_int, _fp, _fp]),
    "nsff_radam_step": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int64, _fp, _fp, C.c_double, C.c_double, C.c_double, C.c_double,
                                  _fp, C.c_int, _fp, _fp]),
    "nsff_composite_backward": (C.c_int, [C.POINTER(CompositeBwdArgs), _fp]),
    "nsff_flow_grad": (C.c_int, [C.POINTER(FlowGradArgs), _fp]),
    "nsff_nerfw_loss": (C.c_int, [C.POINTER(LossArgs), C.c_int, _fp]),
    "nsff_nerfw_loss_work_bytes": (C.c_size_t, [C.c_longlong]),
    "nsff_nerfw_loss_ex": (C.c_int, [C.POINTER(LossArgs), C.c_int, _fp, C.c_size_t, _fp]),
    "nsff_last_loss_path": (C.c_int, []),
    "nsff_splat_planes": (C.c_int, [C.POINTER(SplatArgs), _fp]),
    "nsff_splat_work_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "nsff_mpi_composite": (C.c_int, [C.POINTER(MpiArgs), _fp]),
    "nsff_ssim_scratch_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "nsff_ssim": (C.c_int, [C.POINTER(SsimArgs), _fp]),
    "nsff_lpips_packed_bytes": (C.c_int64, []),
    "nsff_lpips_pack": (C.c_int, [C.POINTER(LpipsWeights), _fp, _fp]),
    "nsff_lpips_dims": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "nsff_lpips_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "nsff_lpips": (C.c_int, [C.POINTER(LpipsArgs), _fp]),
    "nsff_frame_finish_scratch_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "nsff_frame_finish": (C.c_int, [C.POINTER(FrameFinishArgs), _fp]),
    "nsff_val_panels_scratch_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "nsff_val_panels": (C.c_int, [C.POINTER(ValPanelsArgs), _fp]),
    "nsff_flow_maps_scratch_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "nsff_flow_maps": (C.c_int, [C.POINTER(FlowMapsArgs), _fp]),
    "nsff_track_step": (C.c_int, [C.POINTER(TrackStepArgs), _fp]),
    "nsff_track_draw_scratch_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "nsff_track_draw": (C.c_int, [C.POINTER(TrackDrawArgs), _fp]),
    "nsff_motion_maps_scratch_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "nsff_motion_maps": (C.c_int, [C.POINTER(MotionMapsArgs), _fp]),
    "nsff_mask_erode": (C.c_int, [C.POINTER(MaskErodeArgs), _fp]),
    "nsff_optflow_grey": (C.c_int, [_fp, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _fp]),
    "nsff_optflow_down": (C.c_int, [_fp, _fp, C.c_int32, C.c_int32, C.c_int32, _fp]),
    "nsff_optflow_up": (C.c_int, [_fp, _fp, C.c_int32, C.c_int32, C.c_int32, _fp]),
    "nsff_optflow_median": (C.c_int, [_fp, _fp, C.c_int32, C.c_int32, C.c_int32, _fp]),
    "nsff_optflow_warp": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int32, C.c_int32, C.c_int32, _fp]),
    "nsff_optflow_iterate": (C.c_int, [C.POINTER(OptflowIterArgs), _fp]),
    "nsff_optflow_result_slot": (C.c_int, [C.c_int32, C.c_int32]),
    "nsff_optflow_levels": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "nsff_optflow_scratch_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "nsff_optflow": (C.c_int, [C.POINTER(OptflowArgs), _fp]),
    "nsff_disparity_sparse_scratch_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "nsff_disparity_sparse": (C.c_int, [C.POINTER(DisparitySparseArgs), _fp]),
    "nsff_disparity_push": (C.c_int, [_fp] * 6 + [C.c_int32, C.c_int32, C.c_int32, _fp]),
    "nsff_disparity_pull": (C.c_int, [_fp] * 4 + [C.c_int32, C.c_int32, C.c_int32, _fp]),
    "nsff_disparity_relax": (C.c_int, [C.POINTER(DisparityRelaxArgs), _fp]),
    "nsff_disparity_result_slot": (C.c_int, [C.c_int32, C.c_int32]),
    "nsff_disparity_levels": (C.c_int, [C.c_int32, C.c_int32]),
    "nsff_disparity_dense_scratch_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "nsff_disparity_dense": (C.c_int, [C.POINTER(DisparityDenseArgs), _fp]),
    "nsff_disparity_span_scratch_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "nsff_disparity_span": (C.c_int, [C.POINTER(DisparitySpanArgs), _fp]),
    "nsff_motion_span_scratch_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "nsff_motion_span": (C.c_int, [C.POINTER(MotionSpanArgs), _fp]),
    "nsff_mask_propagate": (C.c_int, [C.POINTER(MaskPropagateArgs), _fp]),
    "nsff_flow_median": (C.c_int, [C.POINTER(FlowMedianArgs), _fp]),
    "nsff_cdf": (C.c_int, [_fp, C.c_int64, C.c_int64, _fp, _fp]),
    "nsff_ray_draw": (C.c_int, [C.POINTER(RayDrawArgs), _fp]),
    "nsff_prof_enable": (C.c_int, [C.c_int]),
    "nsff_prof_collect": (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "nsff_prof_collect_clock": (C.c_int, [C.POINTER(C.c_int64)] + [C.POINTER(C.c_double)] * 5),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def load():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C nsff_pl_amd/csrc`).  There is no CPU fallback for the render path.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if lib.nsff_abi_version() != ABI_VERSION:
            raise RuntimeError("libnsff_hip.so ABI version mismatch")
        _lib = lib
    return _lib


def _check(rc, what):
    if rc != 0:
        msg = _ERR.get(rc, f"error {rc}")
        if rc == -4:
            msg += ": " + load().nsff_last_hip_error().decode()
        raise RuntimeError(f"{what} failed: {msg}")


def require_gpu_tensor(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what} must be a GPU tensor: the NSFF render path runs only on the "
                           "HIP kernels of libnsff_hip.so (no CPU fallback)")


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), "need contiguous fp32 GPU tensor"
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ----------------------------------------------------------------------------------
def model_desc(model):
    """NsffModelDesc of a NeRF module.  The reference constructor (models/nerf.py:34-40) takes any width W and a
    list of skip layers; the gfx950 kernels are built for W = 256 trunks, 2..8 layers deep, with any set of skip layers
    among 1..D-1 (inference and training alike) -- anything else is
    refused here, by name."""
    if model.W != 256:
        raise RuntimeError(f"unsupported NeRF architecture: W={model.W} (the gfx950 field kernels tile W=256 trunks "
                           "into 4 x 64-neuron wave blocks; other widths are not built)")
    skips = sorted(set(int(s) for s in model.skips))
    if not 2 <= model.D <= 8 or any(not 1 <= s < model.D for s in skips):
        raise RuntimeError(f"unsupported NeRF architecture: D={model.D}, skips={list(model.skips)} (need 2 <= D <= 8 "
                           "and every skip layer in 1..D-1; a skip at layer 0 would concatenate the input with itself)")
    mask = sum(1 << s for s in skips)
    return ModelDesc(D=model.D, W=model.W, skip=skips[0] if len(skips) == 1 else 0, skip_mask=mask if len(skips) != 1 else 0,
                     in_xyz=model.in_channels_xyz,
                     in_dir=model.in_channels_dir,
                     in_a=model.in_channels_a if model.use_viewdir else 0,
                     in_t=model.in_channels_t, use_viewdir=int(model.use_viewdir),
                     has_transient=int(model.encode_transient),
                     has_flow=int(getattr(model, "has_flow_heads", hasattr(model, "transient_flow_fw"))),
                     flow_scale=float(getattr(model, "flow_scale", 0.0)))


def param_list(model):
    """Parameter tensors in the order nsff_pack_weights documents."""
    def lin(m):
        layer = m[0] if isinstance(m, torch.nn.Sequential) else m
        return [layer.weight, layer.bias]
    out = []
    for i in range(model.D):
        out += lin(getattr(model, f"static_xyz_encoding_{i + 1}"))
    out += lin(model.static_xyz_encoding_final)
    if model.use_viewdir:
        out += lin(model.static_dir_encoding)
    out += lin(model.static_sigma) + lin(model.static_rgb)
    if model.encode_transient:
        for i in range(model.D):
            out += lin(getattr(model, f"transient_xyz_encoding_{i + 1}"))
        out += lin(model.transient_xyz_encoding_final)
        out += lin(model.transient_sigma) + lin(model.transient_rgb)
        if hasattr(model, "transient_flow_fw"):
            out += lin(model.transient_flow_fw) + lin(model.transient_flow_bw)
    return out


def packed_bytes(desc, precision=0):
    n = C.c_size_t(0)
    _check(load().nsff_packed_bytes(C.byref(desc), int(precision), C.byref(n)), "nsff_packed_bytes")
    return n.value


PACK_SKIP_FOLD = 1


def pack_weights(desc, params, packed, precision=0, fold=True):
    """fold=False: without the folded head rows inference launches read (include/nsff_render.h: NSFF_PACK_SKIP_FOLD)."""
    lib = load()
    if lib.nsff_param_count(C.byref(desc)) != len(params):
        raise RuntimeError("parameter list does not match the model description")
    keep = [p.detach().contiguous().float() for p in params]
    for p in keep:
        require_gpu_tensor(p, "model parameter")
    arr = (_fp * len(keep))(*[p.data_ptr() for p in keep])
    _check(lib.nsff_pack_weights_ex(C.byref(desc), int(precision), arr, _ptr(packed), 0 if fold else PACK_SKIP_FOLD,
                                    _stream()), "nsff_pack_weights_ex")
    return keep  # caller keeps temporaries alive until the stream has consumed them


def fold_heads(desc, params, packed, precision):
    keep = [p.detach().contiguous().float() for p in params]
    arr = (_fp * len(keep))(*[p.data_ptr() for p in keep])
    _check(load().nsff_fold_heads(C.byref(desc), int(precision), arr, _ptr(packed), _stream()), "nsff_fold_heads")
    return keep


def time_rows_backward(g_cur, g_next, g_prev, ts, max_t, n_table):
    """d_table (n_table, width) of E[ts], E[clamp(ts + 1)], E[clamp(ts - 1)] for the (n, width) cotangents given (None = absent)."""
    gs = [None if g is None else g.contiguous() for g in (g_cur, g_next, g_prev)]
    width = next(g for g in gs if g is not None).shape[1]
    assert ts.dtype == torch.int64 and ts.is_cuda and ts.is_contiguous()
    d = torch.empty(int(n_table), width, device=ts.device)
    _check(load().nsff_time_rows_backward(_ptr(gs[0]), _ptr(gs[1]), _ptr(gs[2]), C.c_void_p(ts.data_ptr()), ts.shape[0],
                                          int(max_t), int(n_table), width, _ptr(d), _stream()), "nsff_time_rows_backward")
    return d


def time_rows(table, ts, max_t, want_next=True, want_prev=True):
    """(E[clamp(ts + 1, max=max_t)], E[clamp(ts - 1, min=0)]) of an embedding table in one launch (rendering.py:218,224)."""
    n, width = ts.shape[0], table.shape[1]
    if want_next and want_prev:     # (one buffer: the two re-queries of a call can then run as ONE field launch over 2 n rays)
        both = torch.empty(2, n, width, device=table.device)
        nxt, prv = both[0], both[1]
    else:
        nxt = torch.empty(n, width, device=table.device) if want_next else None
        prv = torch.empty(n, width, device=table.device) if want_prev else None
    assert ts.dtype == torch.int64 and ts.is_cuda and ts.is_contiguous()
    _check(load().nsff_time_rows(_ptr(table), table.shape[0], width, C.c_void_p(ts.data_ptr()), n, int(max_t),
                                 _ptr(nxt), _ptr(prv), _stream()), "nsff_time_rows")
    return nxt, prv


def posenc(x, freqs, out):
    f = [float(v) for v in freqs]
    arr = (C.c_float * len(f))(*f)
    _check(load().nsff_posenc(_ptr(x), x.shape[0], arr, len(f), _ptr(out), _stream()), "nsff_posenc")


def field_query(model, raw, n_points, pts_per_ray, static_mode, transient_mode, flow_heads=0,
                xyz=None, freqs=None, dir_emb=None, a_emb=None, t_emb=None,
                x_emb=None, emb_offsets=(0, -1, -1, -1), save_acts=None, save_xin=None, save_masks=None, save_side=None,
                precision=None, t_bias=None, s_bias=None, save_lo=False):
    from . import config
    desc = model_desc(model)
    prec = config.precision_code(model) if precision is None else precision
    saves = not (save_acts is None and save_xin is None and save_masks is None and save_side is None)
    # (training forwards run the folded step program too: one pack form)
    packed = model.packed(prec)
    a = FieldArgs()
    a.precision, a.tile_points = prec, config.get_tile_points()
    a.launch_form = 0 if config.get_persistent() else 1
    a.n_points, a.pts_per_ray = int(n_points), int(pts_per_ray)
    a.static_mode, a.transient_mode, a.flow_heads = int(static_mode), int(transient_mode), int(flow_heads)
    a.xyz = _ptr(xyz)
    if freqs is not None:
        f = [float(v) for v in freqs]
        if len(f) > MAX_FREQS:
            raise RuntimeError("too many embedding frequencies")
        a.n_freqs = len(f)
        for i, v in enumerate(f):
            a.freqs[i] = v
    a.dir_emb, a.a_emb, a.t_emb = _ptr(dir_emb), _ptr(a_emb), _ptr(t_emb)
    a.x_emb = _ptr(x_emb)
    a.ld_emb = int(x_emb.shape[1]) if x_emb is not None else 0
    a.off_xyz, a.off_dir, a.off_a, a.off_t = [int(v) for v in emb_offsets]
    a.raw = _ptr(raw)
    a.save_acts = None if save_acts is None else save_acts.data_ptr()
    a.save_xin = None if save_xin is None else save_xin.data_ptr()
    a.save_masks = None if save_masks is None else save_masks.data_ptr()
    a.save_side = None if save_side is None else save_side.data_ptr()
    if save_lo:                                 # (field_grad.alloc_saves: the remainder plane of a saved tensor directly behind it)
        for i, t in enumerate((save_acts, save_xin, save_side)):
            a.save_lo_delta[i] = 0 if t is None else lo_delta(t)
    if t_bias is not None:                      # (n_rays, rows, 256) from time_bias(): the time code's part of the input layers
        a.t_bias, a.t_bias_rows = _ptr(t_bias), int(t_bias.shape[1])
    if s_bias is not None:                      # (n_rays, 1, 256) from side_bias(): [dir | a]'s part of static_dir_encoding
        a.s_bias, a.s_bias_rows = _ptr(s_bias), int(s_bias.shape[1])
    # the 16x16x32 form of the hand-scheduled inference kernel -- the default where it covers the launch -- reads a second buffer, built
    # at the first launch that is planned for it (NSFF_H3A_SHAPE is read per launch; 32: nothing is asked and nothing is built)
    if os.environ.get("NSFF_H3A_SHAPE") != "32" and prec == config.PRECISIONS["f16x3"] and not saves and \
            load().nsff_field_mfma_shape(C.byref(desc), C.byref(a)) == 16:
        _check(load().nsff_field_query_repacked(C.byref(desc), _ptr(packed), _ptr(model.packed(REPACKED)), C.byref(a), _stream()),
               "nsff_field_query_repacked")
        return
    _check(load().nsff_field_query(C.byref(desc), _ptr(packed), C.byref(a), _stream()), "nsff_field_query")


def lo_delta(t):
    """Elements from a tensor to its remainder twin: the three-product buffers are allocated as (2, ...) -- plane 0 the fp16 values
    (the tensor every caller holds), plane 1 value - fp16(value) -- so the twin of any slice of plane 0 sits numel(plane) further on."""
    n = t.numel()
    if t.untyped_storage().nbytes() < (t.storage_offset() + 2 * n) * t.element_size():
        raise RuntimeError("three-product backward: this buffer has no remainder plane behind it (field_grad.alloc_saves(..., x3=True))")
    return n


def side_bias(model, dir_rows, a_rows=None):
    """(n_rays, 1, 256) fp32: per ray, the folded bias + the [dir | a] columns' product of static_dir_encoding (nsff_side_bias);
    field_query(..., s_bias=) then runs the view-direction static trunk on the hand-scheduled kernel."""
    from . import config
    desc = model_desc(model)
    n_rays = int(dir_rows.shape[0])
    assert dir_rows.shape == (n_rays, desc.in_dir) and (desc.in_a == 0 or (a_rows is not None and a_rows.shape == (n_rays, desc.in_a)))
    packed = model.packed(config.PRECISIONS["f16x3"])      # (the folded bias row lives in the inference pack)
    w = model.static_dir_encoding[0].weight.detach()
    out = torch.empty(n_rays, 1, 256, device=dir_rows.device, dtype=torch.float32)
    _check(load().nsff_side_bias(C.byref(desc), _ptr(packed), _ptr(w), _ptr(dir_rows), _ptr(a_rows) if desc.in_a > 0 else None,
                                 n_rays, _ptr(out), _stream()), "nsff_side_bias")
    return out


_DEVICE_RNG_GEOMETRY = {}


def fused_draws(plan, device, values=True, coarse=None):
    """The draws ``[(kind, shape)]`` (kind "rand" | "randn") of torch's default generator of `device`, in order, by ONE launch
    (nsff_rng_draws): bit-identical to calling torch.rand / torch.randn in that order, and the generator is left where those
    calls would leave it.  values=False for entries whose numbers nobody reads: give a list of booleans -- such a draw only
    advances the generator (its tensor is None).  -> list of float32 tensors.
    coarse = (rays, z_lin, perturb, zs, xyz): plan[0] is the stratified-sampling draw of the call (perturb > 0); the launch
    computes the coarse depths from it where it is drawn (nsff_rng_draws_coarse) -- `coarse_samples` is not needed then."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _DEVICE_RNG_GEOMETRY:
        p = torch.cuda.get_device_properties(idx)
        _DEVICE_RNG_GEOMETRY[idx] = p.multi_processor_count * (p.max_threads_per_multi_processor // 256)
    max_grid = _DEVICE_RNG_GEOMETRY[idx]
    gen = torch.cuda.default_generators[idx]
    seed, offset = gen.initial_seed(), gen.get_offset()
    wanted = values if isinstance(values, (list, tuple)) else [bool(values)] * len(plan)
    sizes = []
    for kind, shape in plan:
        n = 1
        for s in shape:
            n *= int(s)
        sizes.append(n)
    total = sum(n for n, w in zip(sizes, wanted) if w)
    buf = torch.empty(max(total, 1), device=dev, dtype=torch.float32)        # ONE allocation; the draws are views of it
    outs, jobs, at = [], [], 0
    for (kind, shape), numel, want in zip(plan, sizes, wanted):
        if numel == 0:                              # (torch returns before it touches the generator)
            outs.append(torch.empty(*shape, device=dev, dtype=torch.float32))
            continue
        grid = min(max_grid, (numel + 255) // 256)
        if coarse is not None and not outs and not want:     # the perturbation draw: consumed by the launch itself
            jobs.append((None, numel, offset, 0, grid))
            outs.append(None)
        elif want:
            t = buf[at:at + numel].view(*shape)
            at += numel
            jobs.append((t, numel, offset, 1 if kind == "randn" else 0, grid))
            outs.append(t)
        else:
            outs.append(None)
        offset += ((numel - 1) // (1024 * grid) + 1) * 4
    hook = None
    if coarse is not None:
        rays, z_lin, perturb, zs, xyz = coarse
        assert plan and plan[0][0] == "rand" and tuple(plan[0][1]) == (rays.shape[0], z_lin.shape[0]) and perturb > 0
        if sizes[0]:
            hook = RngCoarse(_ptr(rays), _ptr(z_lin), _ptr(zs), _ptr(xyz), int(z_lin.shape[0]), float(perturb), 0, 0)
    for k in range(0, len(jobs), MAX_RNG_JOBS):
        part = jobs[k:k + MAX_RNG_JOBS]
        arr = (RngJob * len(part))()
        for j, (t, numel, off, kind, grid) in enumerate(part):
            arr[j].out, arr[j].numel, arr[j].offset, arr[j].kind, arr[j].grid = (None if t is None else t.data_ptr()), numel, off, kind, grid
        with torch.cuda.device(idx):
            _check(load().nsff_rng_draws_coarse(arr, len(part), seed, C.byref(hook) if (hook is not None and k == 0) else None, _stream()),
                   "nsff_rng_draws")
    gen.set_offset(offset)
    return outs


_FUSED_DRAWS_OK = {}


def fused_draws_match_torch(device):
    """True when :func:`fused_draws` reproduces torch's generator on `device` -- checked ONCE per device, on first use: fused_draws
    restates three ATen internals (the launch geometry of calc_execution_policy, the Philox offset accounting, the uniform /
    normal transforms), and a torch or hiprand upgrade could change any of them without an error.  A few thousand rand / randn
    numbers (several grid sizes, a size that is not a multiple of four) are drawn both ways from the same saved generator state
    and compared bit for bit, the generator's final offset included; the state is restored afterwards, so the check draws
    nothing from the caller's stream of numbers.  On a mismatch the render path uses the torch calls (as NSFF_TORCH_RNG=1 does)
    and says so once."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx in _FUSED_DRAWS_OK:
        return _FUSED_DRAWS_OK[idx]
    if torch.cuda.is_current_stream_capturing():          # (never decided inside a capture: the caller draws with torch there anyway)
        return False
    gen = torch.cuda.default_generators[idx]
    state = gen.get_state()
    ok = True
    try:
        plan = [("rand", (7, 64)), ("randn", (1031,)), ("rand", (3, 5, 2)), ("randn", (70000,)), ("rand", (300001,))]
        gen.manual_seed(0x5EED1234)
        gen.set_offset(8)
        mine = fused_draws(plan, torch.device("cuda", idx))
        end_mine = gen.get_offset()
        gen.manual_seed(0x5EED1234)
        gen.set_offset(8)
        with torch.cuda.device(idx):
            ref = [(torch.rand if k == "rand" else torch.randn)(*shape, device=torch.device("cuda", idx)) for k, shape in plan]
        end_ref = gen.get_offset()
        ok = end_mine == end_ref and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(mine, ref))
    except Exception:                                      # an API that moved is a mismatch as well
        ok = False
    finally:
        gen.set_state(state)
    if not ok:
        import warnings
        warnings.warn("nsff_pl_amd: the fused generator kernel (nsff_rng_draws) no longer reproduces torch.rand / torch.randn on "
                      f"cuda:{idx} (torch {torch.__version__}); render_rays draws with the torch calls instead (slower by ~1 %, same "
                      "numbers as the reference)")
    _FUSED_DRAWS_OK[idx] = ok
    return ok


def time_bias_rows(model):
    """rows per ray of time_bias() for this model (0: no dynamic trunk)"""
    return load().nsff_time_bias_rows(C.byref(model_desc(model)))


def time_bias(jobs, index=None):
    """jobs: [(model, t_rows (n_rays, in_t))] (at most MAX_TIME_BIAS_JOBS, one n_rays) -> [(n_rays, rows, 256) fp32]: per ray,
    bias + time-code columns' product of the dynamic trunk's layer 0 and skip layers (nsff_time_bias: ONE launch for all
    jobs); field_query(..., t_bias=) then multiplies no time-code column.
    index = (table (n_table, in_t), ts (n_rays,) int64, max_t): jobs are [(model, delta)], delta in (0, +1, -1) -- the launch
    gathers table[clamp(ts + delta)] itself (no separate gather / neighbour-row launches) and ALSO returns the gathered rows:
    -> (outs, {delta: (n_rays, in_t)}); the rows of +1 and -1 are the two halves of one buffer."""
    assert 1 <= len(jobs) <= MAX_TIME_BIAS_JOBS
    arr = (TimeBiasJob * len(jobs))()
    keep, outs, per_model, pair = [], [], {}, None
    rows_of = {}
    if index is not None:
        table, ts, max_t = index
        assert ts.dtype == torch.int64 and ts.is_cuda and ts.is_contiguous() and ts.dim() == 1, "ts: one int64 frame index per ray"
        n_rays, width = int(ts.shape[0]), int(table.shape[1])
        deltas = sorted({int(d) for _, d in jobs})
        if 1 in deltas and -1 in deltas:
            both = torch.empty(2, n_rays, width, device=table.device, dtype=torch.float32)
            rows_of[1], rows_of[-1] = both[0], both[1]
        for d in deltas:
            if d not in rows_of:
                rows_of[d] = torch.empty(n_rays, width, device=table.device, dtype=torch.float32)
        written = set()
    else:
        n_rays = int(jobs[0][1].shape[0])
    for j, (model, t_rows) in enumerate(jobs):
        if id(model) not in per_model:
            desc = model_desc(model)
            lins = [getattr(model, f"transient_xyz_encoding_{l + 1}")[0] for l in [0] + sorted(set(int(v) for v in model.skips))]
            wb = [(m.weight.detach(), m.bias.detach()) for m in lins]
            for w, b in wb:
                _ptr(w), _ptr(b)                # (contiguous fp32 GPU tensors, or an assertion)
            per_model[id(model)] = (desc, C.pointer(desc), wb)
        desc, pdesc, wb = per_model[id(model)]
        if index is not None:
            delta, t_rows = int(t_rows), None
            assert width == desc.in_t
        else:
            assert t_rows.shape == (n_rays, desc.in_t)
        # (consecutive jobs of one model get adjacent halves of one buffer: see rendering._inference's merged re-query)
        dev = wb[0][0].device
        if j + 1 < len(jobs) and jobs[j + 1][0] is model and pair is None:
            pair = torch.empty(2, n_rays, len(wb), 256, device=dev, dtype=torch.float32)
            out = pair[0]
        elif pair is not None:
            out, pair = pair[1], None
        else:
            out = torch.empty(n_rays, len(wb), 256, device=dev, dtype=torch.float32)
        arr[j].desc = pdesc
        for i, (w, b) in enumerate(wb):
            arr[j].w[i], arr[j].b[i] = w.data_ptr(), b.data_ptr()
        arr[j].t_rows, arr[j].out = _ptr(t_rows), _ptr(out)
        if index is not None:
            arr[j].table, arr[j].ts = _ptr(table), ts.data_ptr()
            arr[j].n_table, arr[j].max_t, arr[j].delta = int(table.shape[0]), int(max_t), delta
            if delta not in written:                # (the first job of a delta leaves the gathered rows behind)
                arr[j].rows_out = _ptr(rows_of[delta])
                written.add(delta)
        outs.append(out)
    keep.append(per_model)
    _check(load().nsff_time_bias(arr, len(jobs), n_rays, _stream()), "nsff_time_bias")
    return outs if index is None else (outs, rows_of)


def coarse_samples(rays, z_lin, perturb, perturb_rand, zs, xyz):
    _check(load().nsff_coarse_samples(_ptr(rays), rays.shape[0], _ptr(z_lin), z_lin.shape[0],
                                      float(perturb), _ptr(perturb_rand), _ptr(zs), _ptr(xyz), _stream()),
           "nsff_coarse_samples")


def fine_samples(rays, z_lin, zs_coarse, n_importance, w_static, w_transient, u_static, u_transient,
                 u_per_ray, samples_static, samples_transient, zs_fine, xyz_fine):
    _check(load().nsff_fine_samples(_ptr(rays), rays.shape[0], _ptr(z_lin), _ptr(zs_coarse),
                                    z_lin.shape[0], int(n_importance), _ptr(w_static), _ptr(w_transient),
                                    _ptr(u_static), _ptr(u_transient), int(u_per_ray),
                                    _ptr(samples_static), _ptr(samples_transient),
                                    _ptr(zs_fine), _ptr(xyz_fine), _stream()), "nsff_fine_samples")


def sample_pdf(bins, weights, u, u_per_ray, eps, samples):
    _check(load().nsff_sample_pdf(_ptr(bins), _ptr(weights), weights.shape[0], weights.shape[1],
                                  _ptr(u), samples.shape[1], int(u_per_ray), float(eps),
                                  _ptr(samples), _stream()), "nsff_sample_pdf")


def warp_points(raw, xyz, zs, z_far, xyz_fw, xyz_bw):
    _check(load().nsff_warp_points(_ptr(raw), _ptr(xyz), _ptr(zs), zs.numel(), float(z_far),
                                   _ptr(xyz_fw), _ptr(xyz_bw), _stream()), "nsff_warp_points")


def frustum_args(w2c, ts, K4, n_cams, n_frames, H, W):
    """NsffFrustumArgs: w2c (n_cams * n_frames, 12) fp32 and ts (>= 1,) int64 on the device (the frame is ts[0])."""
    assert w2c.is_cuda and w2c.dtype == torch.float32 and w2c.is_contiguous() and w2c.shape == (n_cams * n_frames, 12)
    assert ts.is_cuda and ts.dtype == torch.int64 and ts.is_contiguous() and ts.numel() >= 1
    a = FrustumArgs(w2c=w2c.data_ptr(), ts=ts.data_ptr(), n_cams=int(n_cams), n_frames=int(n_frames), H=int(H), W=int(W))
    a.K4[:] = [float(v) for v in K4]
    a._keep = (w2c, ts)                      # the structure only holds addresses
    return a


def frustum_visibility(vis, xyz, out):
    _check(load().nsff_frustum_visibility(C.byref(vis), _ptr(xyz), xyz.shape[0], _ptr(out), _stream()),
           "nsff_frustum_visibility")


def composite(vis=None, **kw):
    a = CompositeArgs()
    for k, v in kw.items():
        if k in _COMPOSITE_PTRS_IN or k in _COMPOSITE_PTRS_OUT:
            setattr(a, k, _ptr(v))
        else:
            setattr(a, k, v)
    if vis is not None:
        a.vis = vis
    _check(load().nsff_composite(C.byref(a), _stream()), "nsff_composite")


def frame_rays(K4, c2w12, H, W, near, shift_near, first, count, rays):
    k = (C.c_float * 4)(*[float(v) for v in K4])
    m = (C.c_float * 12)(*[float(v) for v in c2w12])
    _check(load().nsff_frame_rays(k, m, int(H), int(W), float(near), float(shift_near), int(first), int(count),
                                  _ptr(rays), _stream()), "nsff_frame_rays")


REPACKED = 101          # PackCache key of the f16x3 pack in the 16x16x32 operand order (nsff_repack_field_weights)


def repack_weights(desc, packed, repacked):
    _check(load().nsff_repack_field_weights(C.byref(desc), _ptr(packed), _ptr(repacked), _stream()), "nsff_repack_field_weights")


def last_field_mfma_shape():
    """16 or 32: the MFMA shape of the trunk phases of the last f16x3 field launch (include/nsff_render.h)."""
    return int(load().nsff_last_field_mfma_shape())


BWD_PACK = 100          # PackCache key of the transposed fp16 weight pack (nsff_pack_weights_bwd)


def bwd_packed_bytes(desc):
    n = C.c_size_t(0)
    _check(load().nsff_bwd_packed_bytes(C.byref(desc), C.byref(n)), "nsff_bwd_packed_bytes")
    return n.value


def pack_weights_bwd(desc, params, packed, fwd_packed=None):
    """fwd_packed: the f16x3 forward pack of the same weights (folded heads): its fp32 scratch supplies the folded products."""
    arr = (_fp * len(params))(*[p.data_ptr() for p in params])
    _check(load().nsff_pack_weights_bwd_ex(C.byref(desc), arr, _ptr(packed), _ptr(fwd_packed), _stream()), "nsff_pack_weights_bwd_ex")


def last_bwd_kernel():
    """'h3b' (the hand-scheduled body), 'c' (compiler-scheduled) or 'c+h3b' (a view-direction model's both-trunk launch: static trunk
    on the compiler-scheduled kernel, dynamic trunk on the hand-scheduled one): which kernel(s) the last field_backward launch took"""
    return {0: "c", 1: "h3b", 2: "c+h3b", 3: "x3"}[load().nsff_last_bwd_kernel()]      # x3: the three-product kernel (config.set_grad_precision)


def last_bwd_grid():
    """workgroups of the last hand-scheduled data-gradient launch (= compute units for a persistent one; 0: none)"""
    return load().nsff_last_bwd_grid()


PLAN_WORDS = 12            # NSFF_PLAN_WORDS


def field_launch_plan(desc, args, n_cus, no_persist=False):
    """Host-only: what nsff_field_query would launch for (ModelDesc, FieldArgs) on a device of n_cus compute units ->
    (NSFF_KERNEL_* code or negative error, [record of PLAN_WORDS ints per launch]) -- include/nsff_render.h::nsff_field_launch_plan."""
    out = (C.c_int32 * (3 * PLAN_WORDS))()
    code = load().nsff_field_launch_plan(C.byref(desc), C.byref(args), int(n_cus), int(bool(no_persist)), out, 3)
    recs = [list(out[i * PLAN_WORDS:(i + 1) * PLAN_WORDS]) for i in range(3)]
    return code, [r for r in recs if r[0] != 0]


def field_bwd_launch_plan(desc, args, n_cus, kernel_override=None, persist=True):
    """Host-only: what nsff_field_backward would launch (kernel_override "c" as NSFF_BWD_KERNEL=c, persist False as
    NSFF_BWD_PERSIST=0) -> (0 c / 1 h3b / 2 c+h3b / 3 x3 or negative error, records) -- nsff_field_bwd_launch_plan."""
    out = (C.c_int32 * (2 * PLAN_WORDS))()
    code = load().nsff_field_bwd_launch_plan(C.byref(desc), C.byref(args), int(n_cus), ord(kernel_override) if kernel_override else 0,
                                                      int(bool(persist)), out, 2)
    recs = [list(out[i * PLAN_WORDS:(i + 1) * PLAN_WORDS]) for i in range(2)]
    return code, [r for r in recs if r[0] != 0]


def field_bwd_phase_program(model, dynamic, want_xin, n_tiles, max_phases=32):
    """(descriptors (n, 8) uint32 numpy, segment byte offsets) of the hand-scheduled backward body for one trunk, or (None, offsets)
    when it does not cover the trunk (host-only: no GPU needed)."""
    import numpy as np
    desc = model_desc(model)
    out = (C.c_uint32 * (8 * max_phases))()
    segs = (C.c_uint32 * 48)()
    n = load().nsff_field_bwd_phase_program(C.byref(desc), 1 if dynamic else 0, 1 if want_xin else 0, int(n_tiles), out, max_phases, segs, 48)
    if n < 0:
        raise RuntimeError(f"nsff_field_bwd_phase_program failed ({n})")
    offs = np.array(list(segs), np.uint32)
    return (np.array(list(out), np.uint32).reshape(max_phases, 8)[:n] if n > 0 else None), offs


def field_backward(model, n_points, static, transient, d_raw, raw, gmax, masks, dpre, dhead, d_xin, d_side=None, x3=False):
    desc = model_desc(model)
    a = FieldBwdArgs(n_points=int(n_points), static_mode=2 if static else 0, transient_mode=2 if transient else 0,
                     d_raw=_ptr(d_raw), raw=_ptr(raw), gmax=_ptr(gmax), masks=masks.data_ptr(), dpre=dpre.data_ptr(),
                     dhead=dhead.data_ptr(), d_xin=_ptr(d_xin), d_side=_ptr(d_side), dpre_lo_delta=lo_delta(dpre) if x3 else 0)
    _check(load().nsff_field_backward(C.byref(desc), _ptr(model.packed(BWD_PACK)), C.byref(a), _stream()),
           "nsff_field_backward")


def train_dims(model):
    """(xin_rows, t_row0, side_rows) of the training buffers of `model` (include/nsff_render.h: nsff_train_dims)."""
    desc = model_desc(model)
    xr, t0, sr = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _check(load().nsff_train_dims(C.byref(desc), C.byref(xr), C.byref(t0), C.byref(sr)), "nsff_train_dims")
    return xr.value, t0.value, sr.value


def field_input_backward(d_xin, t_row0, xyz, pts_per_ray, freqs, in_t, want_xyz, want_t):
    """(d_xyz (P,3) or None, d_t (n_rays, in_t) or None) from the (P, xin_rows) trunk-input gradient."""
    P, xin_rows = d_xin.shape
    n_rays = P // pts_per_ray
    d_xyz = torch.empty(P, 3, device=d_xin.device) if want_xyz else None
    d_t = torch.empty(n_rays, in_t, device=d_xin.device) if want_t else None
    f = [float(v) for v in freqs]
    arr = (C.c_float * max(len(f), 1))(*f)
    _check(load().nsff_field_input_backward(_ptr(d_xin), int(xin_rows), int(t_row0), _ptr(xyz), n_rays, int(pts_per_ray), arr,
                                            len(f), int(in_t), _ptr(d_xyz), _ptr(d_t), _stream()), "nsff_field_input_backward")
    return d_xyz, d_t


def _wgrad_jobs(jobs, with_off):
    return (WgradJob * len(jobs))(*[WgradJob(a=j[0], b=j[1], a_rows=j[2], b_rows=j[3], out_off=j[4] if with_off else 0, trunk=j[5],
                                             a_lo_delta=j[6] if len(j) > 6 else 0, b_lo_delta=j[7] if len(j) > 7 else 0) for j in jobs])


def weight_grad(jobs, n_tiles, n_splits, out, bias, gmax):
    """jobs: list of (a_ptr, b_ptr, a_rows, b_rows, out_off, trunk[, a_lo_delta, b_lo_delta]); out / bias receive the final (summed,
    unscaled) gradients; gmax: the 16 column maxima of the raw-record gradient (absmax)."""
    arr = _wgrad_jobs(jobs, True)
    n = load().nsff_weight_grad_scratch(arr, len(jobs), int(n_tiles), int(n_splits))
    if n < 0:
        raise RuntimeError("nsff_weight_grad_scratch failed")
    scratch = torch.empty(n, device=out.device)
    _check(load().nsff_weight_grad(arr, len(jobs), int(n_tiles), int(n_splits), _ptr(scratch), _ptr(out), _ptr(bias),
                                   _ptr(gmax), _stream()), "nsff_weight_grad")


def weight_grad_accumulate(jobs, n_tiles, n_splits, grad_map, grad_base_ptr, gmax, aux=None):
    """The same GEMMs, accumulated straight into the parameters' gradient memory.  grad_map: (n,4) int32 device tensor of
    NsffGradMapEntry rows; grad_base_ptr: device address the map's `dst` offsets count from; aux: fp32 tensor that receives
    the entries with dst < 0 (dense sums for the folded parameters)."""
    arr = _wgrad_jobs(jobs, False)
    n = load().nsff_weight_grad_scratch(arr, len(jobs), int(n_tiles), int(n_splits))
    if n < 0:
        raise RuntimeError("nsff_weight_grad_scratch failed")
    assert grad_map.dtype == torch.int32 and grad_map.is_contiguous() and grad_map.shape[1] == 4
    scratch = torch.empty(n, device=gmax.device)
    _check(load().nsff_weight_grad_accumulate_aux(arr, len(jobs), int(n_tiles), int(n_splits), _ptr(scratch),
                                                  C.c_void_p(grad_map.data_ptr()), grad_map.shape[0], C.c_void_p(grad_base_ptr),
                                                  _ptr(aux), _ptr(gmax), _stream()), "nsff_weight_grad_accumulate_aux")
    return scratch


def fold_grads(g, gb, w_final, b_final, head_rows, d_w_final, d_b_final):
    """nsff_fold_grads: head_rows = [(w_row (256,) tensor, d_w_row (256,) view of .grad, d_b (1,) view of .grad)] per folded row;
    every tensor fp32 contiguous on the GPU; the d_* are accumulated into."""
    a = FoldGradArgs(n_rows=len(head_rows), g=_ptr(g), gb=_ptr(gb), w_final=_ptr(w_final), b_final=_ptr(b_final),
                     d_w_final=_ptr(d_w_final), d_b_final=_ptr(d_b_final))
    for r, (w, dw, db) in enumerate(head_rows):
        a.w_head[r], a.d_w_head[r], a.d_b_head[r] = w.data_ptr(), dw.data_ptr(), db.data_ptr()
    _check(load().nsff_fold_grads(C.byref(a), _stream()), "nsff_fold_grads")


def fold_grads_dense(g, gb, w_head, w_final, b_final, d_w_head, d_b_head, d_w_final, d_b_final, accumulate, g2=None, gb2=None):
    """nsff_fold_grads_dense: g (R, 256) [+ g2], gb (R,) [+ gb2]: dense sum / row sums of the folded layer's job; w_head (R, >= 256)
    a (possibly column-sliced) view of the folded layer's weight -- its row stride is passed on --, d_w_head likewise; w_final
    (256, 256), b_final (256,).  accumulate: add to / store into the d_* tensors (fp32 GPU tensors, rows contiguous)."""
    R = int(g.shape[0])
    for t in (g, g2, gb, gb2, w_final, b_final, d_w_final, d_b_final, d_b_head):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous())
    for t in (w_head, d_w_head):
        assert t.is_cuda and t.dtype == torch.float32 and t.shape[0] == R and t.shape[1] == 256 and t.stride(1) == 1
    a = FoldDenseArgs(n_rows=R, accumulate=1 if accumulate else 0, ld_head=int(w_head.stride(0)), ld_dhead=int(d_w_head.stride(0)),
                      g=g.data_ptr(), g2=None if g2 is None else g2.data_ptr(), gb=gb.data_ptr(), gb2=None if gb2 is None else gb2.data_ptr(),
                      w_head=w_head.data_ptr(), w_final=w_final.data_ptr(), b_final=b_final.data_ptr(), d_w_head=d_w_head.data_ptr(),
                      d_b_head=d_b_head.data_ptr(), d_w_final=d_w_final.data_ptr(), d_b_final=d_b_final.data_ptr())
    _check(load().nsff_fold_grads_dense(C.byref(a), _stream()), "nsff_fold_grads_dense")


def absmax(x):
    """max |x| as a device scalar (one launch, no host round trip).  For a raw-record gradient (P, RAW_STRIDE): the 16 COLUMN
    maxima -- what field_backward / weight_grad* derive their scales from (one per trunk for the fragments, one per head row)."""
    x = x.contiguous()
    if x.dim() == 2 and x.shape[1] == RAW_STRIDE:
        out = torch.empty(RAW_STRIDE, device=x.device, dtype=torch.float32)
        _check(load().nsff_absmax_raw(_ptr(x), x.shape[0], _ptr(out), _stream()), "nsff_absmax_raw")
        return out
    out = torch.empty((), device=x.device, dtype=torch.float32)
    _check(load().nsff_absmax(_ptr(x), x.numel(), _ptr(out), _stream()), "nsff_absmax")
    return out


def adam_step(param, grad, exp_avg, exp_avg_sq, state, lr, beta1, beta2, eps, weight_decay, seg_start=None, seg_used=None):
    """One Adam step on flat buffers (include/nsff_render.h: nsff_adam_step); state / lr are device tensors.  With
    ``seg_start`` (int64, n_seg + 1 offsets) and ``seg_used`` (int32, n_seg): parameter tensors whose gradient slice is
    identically zero this step are skipped as torch.optim.Adam skips ``grad is None`` (nsff_adam_step_segments)."""
    if seg_start is None:
        _check(load().nsff_adam_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), _ptr(state), _ptr(lr),
                                     float(beta1), float(beta2), float(eps), float(weight_decay), _stream()), "nsff_adam_step")
        return
    _check(load().nsff_adam_step_segments(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), _ptr(state),
                                          _ptr(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                                          C.c_void_p(seg_start.data_ptr()), int(seg_used.numel()),
                                          C.c_void_p(seg_used.data_ptr()), _stream()),
           "nsff_adam_step_segments")


def _segments(seg_start, seg_used):
    if seg_start is None:
        return None, 0, None
    return C.c_void_p(seg_start.data_ptr()), int(seg_used.numel()), C.c_void_p(seg_used.data_ptr())


def sgd_step(param, grad, momentum_buf, state, lr, momentum, weight_decay, seg_start=None, seg_used=None):
    """One torch.optim.SGD step (dampening 0, no Nesterov) on flat buffers (include/nsff_render.h: nsff_sgd_step); state / lr are
    device tensors, ``momentum_buf`` is None when ``momentum == 0``.  ``seg_start`` / ``seg_used`` as in :func:`adam_step`."""
    _check(load().nsff_sgd_step(_ptr(param), _ptr(grad), _ptr(momentum_buf), param.numel(), _ptr(state), _ptr(lr), float(momentum),
                                float(weight_decay), *_segments(seg_start, seg_used), _stream()), "nsff_sgd_step")


def radam_step(param, grad, exp_avg, exp_avg_sq, state, lr, beta1, beta2, eps, weight_decay, seg_start=None, seg_used=None):
    """One RAdam step with decoupled weight decay on flat buffers (include/nsff_render.h: nsff_radam_step); state (8 floats) / lr
    are device tensors.  ``seg_start`` / ``seg_used`` as in :func:`adam_step`."""
    _check(load().nsff_radam_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), _ptr(state), _ptr(lr),
                                  float(beta1), float(beta2), float(eps), float(weight_decay), *_segments(seg_start, seg_used),
                                  _stream()), "nsff_radam_step")


def composite_backward(n_rays, n_samples, has_transient, flow_mode, noise_std, **tensors):
    a = CompositeBwdArgs(n_rays=int(n_rays), n_samples=int(n_samples), has_transient=int(has_transient),
                         flow_mode=int(flow_mode), noise_std=float(noise_std))
    for k, v in tensors.items():
        setattr(a, k, _ptr(v))
    _check(load().nsff_composite_backward(C.byref(a), _stream()), "nsff_composite_backward")


def flow_grad(zs, z_far, out, accumulate, col_a=-1, g_a=(), col_b=-1, g_b=()):
    """out (P,16) (+)= masked sums of the (P,3) cotangents g_a into columns col_a.., g_b into col_b.. (nsff_flow_grad)."""
    a = FlowGradArgs(n_points=int(out.shape[0]), zs=_ptr(zs), z_far=float(z_far), accumulate=int(bool(accumulate)),
                     col_a=int(col_a), col_b=int(col_b), out=_ptr(out))
    if len(g_a) > 4 or len(g_b) > 4:
        raise ValueError("flow_grad: at most four cotangents per group")
    keep = [g.contiguous() for g in list(g_a) + list(g_b)]          # (alive until the launch is enqueued)
    for i, g in enumerate(keep[:len(g_a)]):
        a.g_a[i] = _ptr(g)
    for i, g in enumerate(keep[len(g_a):]):
        a.g_b[i] = _ptr(g)
    _check(load().nsff_flow_grad(C.byref(a), _stream()), "nsff_flow_grad")


def nerfw_loss(mode, n_rays, n_samples, n_keep, n_frames, max_t, topk=1.0, thickness=1, work=None, **tensors):
    """mode 1: the terms into tensors['terms']; mode 2: gradients into tensors['g_*'] (include/nsff_render.h).
    work: None = nsff_nerfw_loss (rank counting, <= 4096 rays); a uint8 GPU tensor of nerfw_loss_work_bytes(n_rays) bytes =
    nsff_nerfw_loss_ex (radix select, <= LOSS_MAX_RAYS rays)."""
    a = LossArgs(n_rays=int(n_rays), n_samples=int(n_samples), n_keep=int(n_keep), n_frames=int(n_frames), max_t=int(max_t),
                 topk=float(topk), thickness=int(thickness))
    for k, v in tensors.items():
        if v is None:
            continue
        if not torch.is_tensor(v):
            raise TypeError(f"nerfw_loss: {k} must be a tensor")
        if v.dtype == torch.int64:
            assert v.is_cuda and v.is_contiguous()
            setattr(a, k, v.data_ptr())
        else:
            setattr(a, k, _ptr(v))
    if work is None:
        _check(load().nsff_nerfw_loss(C.byref(a), int(mode), _stream()), "nsff_nerfw_loss")
        return
    if not (torch.is_tensor(work) and work.is_cuda and work.dtype == torch.uint8 and work.is_contiguous()):
        raise TypeError("nerfw_loss: work must be a contiguous uint8 GPU tensor")
    _check(load().nsff_nerfw_loss_ex(C.byref(a), int(mode), work.data_ptr(), work.numel(), _stream()), "nsff_nerfw_loss_ex")


LOSS_MAX_RAYS = 1 << 20                       # NSFF_LOSS_MAX_RAYS


def nerfw_loss_work_bytes(n_rays):
    """bytes of workspace nsff_nerfw_loss_ex needs for n_rays rays (0: outside 1 .. LOSS_MAX_RAYS)"""
    return int(load().nsff_nerfw_loss_work_bytes(int(n_rays)))


def last_loss_path():
    """which selection the last loss call of this process launched: 0 none yet, 1 rank counting, 2 radix select"""
    return int(load().nsff_last_loss_path())


def splat_work_bytes(H, W, S):
    return int(load().nsff_splat_work_bytes(int(H), int(W), int(S)))


def splat_planes(H, W, S, K4, P12, scale, xyz, flow, rgb, alpha, accum, work=None):
    """work: uint8 device tensor of splat_work_bytes(H, W, S) bytes (binned far path) or None (device-scope atomics)."""
    a = SplatArgs(H=int(H), W=int(W), n_planes=int(S), scale=float(scale), xyz=_ptr(xyz), flow=_ptr(flow),
                  rgb=_ptr(rgb), alpha=_ptr(alpha), accum=_ptr(accum))
    if work is not None:
        assert work.is_cuda and work.is_contiguous() and work.dtype == torch.uint8
        a.work, a.work_bytes = work.data_ptr(), work.numel()
    a.K4[:] = [float(v) for v in K4]
    a.P[:] = [float(v) for v in P12]
    _check(load().nsff_splat_planes(C.byref(a), _stream()), "nsff_splat_planes")


def mpi_composite(H, W, S, dt, accum_fw, accum_bw, static_rgb, static_alpha, zs, rgb, depth):
    a = MpiArgs(H=int(H), W=int(W), n_planes=int(S), dt=float(dt), accum_fw=_ptr(accum_fw), accum_bw=_ptr(accum_bw),
                static_rgb=_ptr(static_rgb), static_alpha=_ptr(static_alpha), zs=_ptr(zs), rgb=_ptr(rgb),
                depth=_ptr(depth))
    _check(load().nsff_mpi_composite(C.byref(a), _stream()), "nsff_mpi_composite")


KERNEL_NAMES = {0: None, 1: "f32", 2: "h3_64", 3: "h3_8wave", 4: "h3a", 5: "h3_save", 7: "h3a_tb", 8: "h3a_side", 9: "h3a_save"}


def _dptr(t, dtype, what):
    """Device pointer of a contiguous GPU tensor of `dtype` (None passes through)."""
    if t is None:
        return None
    require_gpu_tensor(t, what)
    if t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"{what}: need a contiguous {dtype} tensor, got {t.dtype}"
                           f"{'' if t.is_contiguous() else ' (non-contiguous)'}")
    return t.data_ptr()


# ---- the frame kernels' argument structs are filled by the three helpers below
_F32, _F64, _U8, _I32, _I64 = torch.float32, torch.float64, torch.uint8, torch.int32, torch.int64
_MASK = "uint8, or bool taken as its uint8 view"          # a row's dtype


def _bind(a, who, dev, *rows):
    """Device pointers into the struct `a`, in the order given.  A row is (field, tensor, dtype, numel[, member[, index]]): a None
    tensor is skipped; any other must be a contiguous GPU tensor of `dtype` (_MASK: uint8 or bool) with `numel` elements on `dev`,
    and its pointer goes to a.<field> -- or to a.<member> / a.<member>[index], where `field` is the tensor's name in a refusal.
    numel None is a workspace: any size, which goes to a.<field>_bytes."""
    for row in rows:
        t = row[1]
        if t is None:
            continue
        field, dtype, numel = row[0], row[2], row[3]
        if dtype is _MASK:
            t, dtype = (t.view(torch.uint8) if t.dtype == torch.bool else t), torch.uint8
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
            _dptr(t, dtype, f"{who}: {field}")                     # raises and says which; a good tensor costs no formatting
        if numel is None:
            numel = t.numel()
            setattr(a, field + "_bytes", numel)
        if t.numel() != numel or t.device != dev:
            raise RuntimeError(f"{who}: {field} has {t.numel()} elements on {t.device}, expected {numel} on {dev}")
        if len(row) == 4:
            setattr(a, field, t.data_ptr())
        elif len(row) == 5:
            setattr(a, row[4], t.data_ptr())
        else:
            getattr(a, row[4])[row[5]] = t.data_ptr()


def _scratch(scratch, wanted, dev, nbytes, *dims, zeroed=True):
    """The caller's scratch as it is; without one and where `wanted`, a fresh one of nbytes(*dims) bytes (16 at least) -- zeroed for
    the per-frame reductions, any content for a workspace -- else None.  The library is asked only then.  It is bound as the
    workspace row ("scratch", ..., _U8, None)."""
    if scratch is None and wanted:
        return (torch.zeros if zeroed else torch.empty)(max(nbytes(*dims), 16), dtype=torch.uint8, device=dev)
    return scratch


def _launch(name, a, dev):
    with torch.cuda.device(dev):
        _check(getattr(load(), name)(C.byref(a), _stream()), name)


def ssim_scratch_bytes(n_frames, H, W):
    return int(load().nsff_ssim_scratch_bytes(int(n_frames), int(H), int(W)))


def ssim(gt, pred, mask=None, map=None, mean_map=None, sums=None, scratch=None):
    """nsff_ssim on (F, H, W, 3) fp32 image pairs: the kornia 0.5.4 SSIM loss map (F, H, W, 3), its channel mean (F, H*W) and
    the per-frame sums (F, 3) fp64 [loss, masked loss, masked pixels] -- whichever outputs are given.  mask (F, H*W) bool / uint8.
    scratch: uint8 tensor of ssim_scratch_bytes() bytes, zero before its first use (a fresh zeroed one when None)."""
    require_gpu_tensor(gt, "ssim: image_gt")
    require_gpu_tensor(pred, "ssim: image_pred")
    if gt.dim() != 4 or gt.shape[-1] != 3 or pred.shape != gt.shape:
        raise RuntimeError(f"ssim: need (F, H, W, 3) image pairs of one shape, got {tuple(gt.shape)} and {tuple(pred.shape)}")
    F, H, W = (int(v) for v in gt.shape[:3])
    px, dev = F * H * W, gt.device
    a = SsimArgs(n_frames=F, H=H, W=W, window=11)
    _bind(a, "ssim", dev, ("image_gt", gt, _F32, px * 3, "gt"), ("image_pred", pred, _F32, px * 3, "pred"), ("mask", mask, _MASK, px),
          ("map", map, _F32, px * 3), ("mean_map", mean_map, _F32, px), ("sums", sums, _F64, F * 3),
          ("scratch", _scratch(scratch, sums is not None, dev, ssim_scratch_bytes, F, H, W), _U8, None))
    _launch("nsff_ssim", a, dev)


LPIPS_MIN_SIZE = 31           # NSFF_LPIPS_MIN_SIZE
LPIPS_CONV_SHAPES = ((64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3))


def lpips_dims(H, W):
    """((h, w),) * 5: the feature-map size of each of the five taps for an H x W image."""
    if H < LPIPS_MIN_SIZE or W < LPIPS_MIN_SIZE:
        raise ValueError(f"lpips: a {H} x {W} image is below the smallest size AlexNet's second pooling leaves a pixel of "
                         f"({LPIPS_MIN_SIZE} x {LPIPS_MIN_SIZE})")
    hw = (C.c_int32 * 10)()
    _check(load().nsff_lpips_dims(int(H), int(W), hw), "nsff_lpips_dims")
    return tuple((hw[2 * l], hw[2 * l + 1]) for l in range(5))


def lpips_workspace_bytes(n_frames, H, W):
    return int(load().nsff_lpips_workspace_bytes(int(n_frames), int(H), int(W)))


def lpips_pack(conv_w, conv_b, lin):
    """nsff_lpips_pack: the five conv weights (cout, cin, k, k), biases (cout,) and lin vectors (cout,) -- contiguous fp32 GPU
    tensors -- into a new packed buffer."""
    for l, shape in enumerate(LPIPS_CONV_SHAPES):
        for t, want, what in ((conv_w[l], shape, "weight"), (conv_b[l], shape[:1], "bias"), (lin[l], shape[:1], "lin weight")):
            require_gpu_tensor(t, f"lpips: layer {l} {what}")
            if tuple(t.shape) != want:
                raise RuntimeError(f"lpips: layer {l} {what} has shape {tuple(t.shape)}, expected {want}")
    dev = conv_w[0].device
    packed = torch.empty(int(load().nsff_lpips_packed_bytes()) // 4, dtype=torch.float32, device=dev)
    w = LpipsWeights()
    for l in range(5):
        w.conv_w[l] = _dptr(conv_w[l], torch.float32, "lpips: weight")
        w.conv_b[l] = _dptr(conv_b[l], torch.float32, "lpips: bias")
        w.lin[l] = _dptr(lin[l], torch.float32, "lpips: lin weight")
    with torch.cuda.device(dev):
        _check(load().nsff_lpips_pack(C.byref(w), packed.data_ptr(), _stream()), "nsff_lpips_pack")
    return packed


def lpips(packed, gt, pred, valid=None, map=None, sums=None, normalize=False, workspace=None):
    """nsff_lpips on (F, H, W, 3) fp32 image pairs: the spatial map (F, H, W) and the per-frame sums (F, 3) fp64 [map, map over
    valid, valid pixels] -- whichever outputs are given.  valid (F, H*W) bool / uint8.  workspace: uint8 tensor of
    lpips_workspace_bytes() bytes (a fresh one when None)."""
    require_gpu_tensor(gt, "lpips: image_gt")
    require_gpu_tensor(pred, "lpips: image_pred")
    if gt.dim() != 4 or gt.shape[-1] != 3 or pred.shape != gt.shape:
        raise RuntimeError(f"lpips: need (F, H, W, 3) image pairs of one shape, got {tuple(gt.shape)} and {tuple(pred.shape)}")
    F, H, W = (int(v) for v in gt.shape[:3])
    lpips_dims(H, W)                                             # refuses an image that is too small by name
    px, dev = F * H * W, gt.device
    need = lpips_workspace_bytes(F, H, W)
    if need == 0:
        raise RuntimeError(f"lpips: {F} frames of {H} x {W} are outside what one call takes (1 .. 32767 frames, H * W < 2^31)")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    a = LpipsArgs(n_frames=F, H=H, W=W, normalize=int(bool(normalize)))
    _bind(a, "lpips", dev, ("image_gt", gt, _F32, px * 3, "gt"), ("image_pred", pred, _F32, px * 3, "pred"), ("valid", valid, _MASK, px),
          ("packed weights", packed, _F32, packed.numel(), "packed"), ("map", map, _F32, px), ("sums", sums, _F64, F * 3),
          ("workspace", workspace, _U8, None))
    _launch("nsff_lpips", a, dev)


def frame_finish_scratch_bytes(n_frames, H, W):
    return int(load().nsff_frame_finish_scratch_bytes(int(n_frames), int(H), int(W)))


def frame_finish(rgb, gt=None, valid=None, depth=None, lut=None, rgb_clipped=None, rgb_u8=None, sums=None, depth_range=None,
                 depth_u8=None, depth_rgb_u8=None, scratch=None):
    """nsff_frame_finish on F frames: rgb / gt (F, H, W, 3) fp32, valid (F, H, W) bool / uint8, depth (F, H, W) fp32, lut (256, 3)
    uint8 -> whichever of rgb_clipped (F, H, W, 3) fp32, rgb_u8 (F, H, W, 3) uint8, sums (F, 3) fp64, depth_range (F, 2) fp32,
    depth_u8 (F, H, W) uint8 and depth_rgb_u8 (F, H, W, 3) uint8 are given.  scratch: uint8 tensor of
    frame_finish_scratch_bytes() bytes, zero before its first use (a fresh zeroed one when None)."""
    require_gpu_tensor(rgb, "frame_finish: rgb")
    if rgb.dim() != 4 or rgb.shape[-1] != 3:
        raise RuntimeError(f"frame_finish: need (F, H, W, 3) frames, got {tuple(rgb.shape)}")
    F, H, W = (int(v) for v in rgb.shape[:3])
    px, dev = F * H * W, rgb.device
    a = FrameFinishArgs(n_frames=F, H=H, W=W)
    scratch = _scratch(scratch, sums is not None or depth_range is not None, dev, frame_finish_scratch_bytes, F, H, W)
    _bind(a, "frame_finish", dev, ("scratch", scratch, _U8, None), ("rgb", rgb, _F32, px * 3), ("gt", gt, _F32, px * 3), ("valid", valid, _MASK, px),
          ("depth", depth, _F32, px), ("lut", lut, _U8, 768), ("rgb_clipped", rgb_clipped, _F32, px * 3), ("rgb_u8", rgb_u8, _U8, px * 3),
          ("sums", sums, _F64, F * 3), ("depth_range", depth_range, _F32, F * 2), ("depth_u8", depth_u8, _U8, px),
          ("depth_rgb_u8", depth_rgb_u8, _U8, px * 3))
    _launch("nsff_frame_finish", a, dev)


def val_panels_scratch_bytes(n_frames, H, W):
    return int(load().nsff_val_panels_scratch_bytes(int(n_frames), int(H), int(W)))


def panel_grid_shape(H, W, n_tiles):
    """(GH, GW) of make_grid(n_tiles images of H x W, nrow=3, padding=2)."""
    return -(-int(n_tiles) // 3) * (int(H) + 2) + 2, 3 * (int(W) + 2) + 2


def val_panels(F, H, W, pred, gt=None, depth=None, transient_alpha=None, static_rgb=None, static_depth=None, mask=None, disp=None,
               ssim_loss=None, lut_depth=None, lut_mask=None, ranges=None, grid_u8=None, rmse_u8=None, ssim_u8=None,
               rmse_blend_u8=None, ssim_blend_u8=None, scratch=None):
    """nsff_val_panels on F frames of H x W pixels: fp32 inputs of F*H*W[*3] elements, lut_* (256, 3) uint8 -> whichever of ranges
    (F, 5, 2) fp32, grid_u8 (F, GH, GW, 3), rmse_u8 / ssim_u8 (F, H, W) and rmse_blend_u8 / ssim_blend_u8 (F, H, W, 3) uint8 are given.
    scratch: uint8 tensor of val_panels_scratch_bytes() bytes, zero before its first use (a fresh zeroed one when None)."""
    F, H, W = int(F), int(H), int(W)
    require_gpu_tensor(pred, "val_panels: pred")
    dev, n = pred.device, F * H * W
    n_tiles = 3 + (3 if transient_alpha is not None else 0) + (mask is not None) + (disp is not None)
    GH, GW = panel_grid_shape(H, W, n_tiles)
    a = ValPanelsArgs(n_frames=F, H=H, W=W)
    _bind(a, "val_panels", dev, ("scratch", _scratch(scratch, True, dev, val_panels_scratch_bytes, F, H, W), _U8, None),
          ("gt", gt, _F32, n * 3), ("pred", pred, _F32, n * 3), ("depth", depth, _F32, n),
          ("transient_alpha", transient_alpha, _F32, n), ("static_rgb", static_rgb, _F32, n * 3), ("static_depth", static_depth, _F32, n),
          ("mask", mask, _F32, n), ("disp", disp, _F32, n), ("ssim_loss", ssim_loss, _F32, n * 3), ("lut_depth", lut_depth, _U8, 768),
          ("lut_mask", lut_mask, _U8, 768), ("ranges", ranges, _F32, F * 10), ("grid_u8", grid_u8, _U8, F * GH * GW * 3),
          ("rmse_u8", rmse_u8, _U8, n), ("ssim_u8", ssim_u8, _U8, n), ("rmse_blend_u8", rmse_blend_u8, _U8, n * 3),
          ("ssim_blend_u8", ssim_blend_u8, _U8, n * 3))
    _launch("nsff_val_panels", a, dev)


def flow_maps_scratch_bytes(n_frames, H, W):
    return int(load().nsff_flow_maps_scratch_bytes(int(n_frames), int(H), int(W)))


def flow_maps(F, H, W, xyz=(None, None), K4=None, Ps=None, ts=None, max_t=0, flow=(None, None), gt=(None, None), mask=None,
              epe_sums=None, epe_counts=None, maxrad=None, scale=None, share_gt_scale=False, image=(None, None),
              gt_image=(None, None), scratch=None):
    """nsff_flow_maps on F frames of H x W pixels; every pair is (forward, backward), either entry may be None.  xyz (F, H*W, 3)
    fp32 NDC points -> flow (F, H, W, 2) fp32 with K4 = (fx, fy, cx, cy), Ps (N, 3, 4) fp32, ts (F,) int32, max_t; flow (written, or
    the caller's own where xyz is None) against gt (F, H, W, 2) [and mask (F, H, W) bool / uint8] -> epe_sums (F, 2, 3) fp64 and
    epe_counts (F, 2, 3) int64; maxrad (F, 2, 2) fp32 out; image / gt_image (F, H, W, 3) uint8 coloured on scale (F, 2, 2) fp32 or, without
    one, on maxrad.  scratch: uint8 tensor of flow_maps_scratch_bytes() bytes, zero before its first use (a fresh one when None)."""
    F, H, W = int(F), int(H), int(W)
    n = F * H * W
    a = FlowMapsArgs(n_frames=F, H=H, W=W, max_t=int(max_t), share_gt_scale=int(bool(share_gt_scale)))
    if K4 is not None:
        a.fx, a.fy, a.cx, a.cy = (float(v) for v in K4)
    first = next((t for t in list(xyz) + list(flow) + list(gt) if t is not None), None)
    require_gpu_tensor(first, "flow_maps: points / flow")
    dev = first.device
    if Ps is not None:
        a.n_poses = int(Ps.numel() // 12)
    pairs = [row for d, tag in enumerate(("fw", "bw")) for row in (
        (f"xyz_{tag}", xyz[d], _F32, n * 3, "xyz", d), (f"flow_{tag}", flow[d], _F32, n * 2, "flow", d),
        (f"gt_{tag}", gt[d], _F32, n * 2, "gt", d), (f"image_{tag}", image[d], _U8, n * 3, "image", d),
        (f"gt_image_{tag}", gt_image[d], _U8, n * 3, "gt_image", d))]
    _bind(a, "flow_maps", dev, *pairs, ("Ps", Ps, _F32, a.n_poses * 12), ("ts", ts, _I32, F), ("mask", mask, _MASK, n),
          ("epe_sums", epe_sums, _F64, F * 6), ("epe_counts", epe_counts, _I64, F * 6), ("maxrad", maxrad, _F32, F * 4),
          ("scale", scale, _F32, F * 4),
          ("scratch", _scratch(scratch, epe_sums is not None or maxrad is not None, dev, flow_maps_scratch_bytes, F, H, W), _U8, None))
    _launch("nsff_flow_maps", a, dev)


def track_step(n_rows, pts_per_row, direction, max_t, xyz_in, t_in, alive_in, raw=None, xyz_out=None, t_out=None, alive_out=None,
               K4=None, Ps=None, fixed_view=False, uv=None, depth=None):
    """nsff_track_step: one step of a track chain (raw given), or the projection of its first slab (raw None); one launch."""
    a = TrackStepArgs()
    a.n_rows, a.pts_per_row, a.direction, a.max_t = int(n_rows), int(pts_per_row), int(direction), int(max_t)
    if Ps is not None:
        a.n_poses, a.fixed_view = int(Ps.shape[0]), int(bool(fixed_view))
        a.fx, a.fy, a.cx, a.cy = (float(v) for v in K4)
    a.raw, a.xyz_in, a.xyz_out = _ptr(raw), _ptr(xyz_in), _ptr(xyz_out)
    a.t_in, a.t_out = _dptr(t_in, torch.int32, "t_in"), _dptr(t_out, torch.int32, "t_out")
    a.alive_in, a.alive_out = _dptr(alive_in, torch.uint8, "alive_in"), _dptr(alive_out, torch.uint8, "alive_out")
    a.Ps, a.uv, a.depth = _ptr(Ps), _ptr(uv), _ptr(depth)
    _launch("nsff_track_step", a, xyz_in.device)


def track_draw_scratch_bytes(H, W):
    return int(load().nsff_track_draw_scratch_bytes(int(H), int(W)))


def track_draw(H, W, n_steps, n_tracks, uv, ok, image, lut, out, scratch):
    """nsff_track_draw: the trails of n_tracks tracks of n_steps segments on a copy of `image`; three launches."""
    a = TrackDrawArgs(H=int(H), W=int(W), n_steps=int(n_steps), n_tracks=int(n_tracks))
    a.uv, a.ok = _ptr(uv), _dptr(ok, torch.uint8, "ok")
    a.image, a.lut, a.out = _dptr(image, torch.uint8, "image"), _dptr(lut, torch.uint8, "lut"), _dptr(out, torch.uint8, "out")
    a.scratch, a.scratch_bytes = _dptr(scratch, torch.uint8, "scratch"), int(scratch.numel())
    _launch("nsff_track_draw", a, image.device)


def motion_maps_scratch_bytes(n_frames, H, W):
    return int(load().nsff_motion_maps_scratch_bytes(int(n_frames), int(H), int(W)))


def motion_maps(flows_fw, flows_bw, Fm=None, alpha=0.01, beta=0.5, threshold=1.0, err=None, valid=None, raw=None, counts=None,
                err_sums=None, scratch=None):
    """nsff_motion_maps on (F, H, W, 2) fp32 flows: the forward-backward check and, with Fm (F, 2, 3, 3) fp32, the distance from the
    epipolar line (without Fm: the check alone) -> err (F, 2, H, W) fp32, valid (F, 2, H, W) uint8, raw (F, H, W) uint8 (0 dynamic,
    255 static), counts (F, 5) int64 [valid fw, valid bw, over fw, over bw, dynamic] with err_sums (F, 2) fp64 -- whichever are
    given.  scratch: uint8 tensor of motion_maps_scratch_bytes() bytes, zero before its first use (a fresh one when None)."""
    require_gpu_tensor(flows_fw, "motion_maps: flows_fw")
    F, H, W = (int(v) for v in flows_fw.shape[:3])
    n, dev = F * H * W, flows_fw.device
    a = MotionMapsArgs(n_frames=F, H=H, W=W, epipolar=int(Fm is not None), alpha=float(alpha), beta=float(beta),
                       threshold=float(threshold))
    _bind(a, "motion_maps", dev, ("flow_fw", flows_fw, _F32, n * 2), ("flow_bw", flows_bw, _F32, n * 2), ("Fm", Fm, _F32, F * 18),
          ("err", err, _F32, n * 2), ("valid", valid, _U8, n * 2), ("raw", raw, _U8, n), ("counts", counts, _I64, F * 5),
          ("err_sums", err_sums, _F64, F * 2),
          ("scratch", _scratch(scratch, counts is not None, dev, motion_maps_scratch_bytes, F, H, W), _U8, None))
    _launch("nsff_motion_maps", a, dev)


def mask_erode(src, dst, k, zero_counts=None, scratch=None):
    """nsff_mask_erode: dst = cv2.erode(src, ones((k, k))) per frame of (F, H, W) uint8 images; zero_counts (F,) int64: the zero
    pixels of each eroded frame.  scratch as for motion_maps."""
    require_gpu_tensor(src, "mask_erode: src")
    F, H, W = (int(v) for v in src.shape)
    px, dev = F * H * W, src.device
    a = MaskErodeArgs(n_frames=F, H=H, W=W, k=int(k))
    _bind(a, "mask_erode", dev, ("src", src, _U8, px), ("dst", dst, _U8, px), ("zero_counts", zero_counts, _I64, F),
          ("scratch", _scratch(scratch, zero_counts is not None, dev, motion_maps_scratch_bytes, F, H, W), _U8, None))
    _launch("nsff_mask_erode", a, dev)


# ---- TV-L1 optical flow (csrc/optflow.hip).  Planes are contiguous fp32 (n, H, W) GPU tensors; the stage calls return their output.
def _planes(t, what, dtype=torch.float32):
    _dptr(t, dtype, what)
    if t.dim() != 3:
        raise RuntimeError(f"{what}: need (n, H, W) planes, got {tuple(t.shape)}")
    return tuple(int(v) for v in t.shape)


def optflow_grey(src):
    """nsff_optflow_grey: (n, H, W, 3) uint8 -> (n, H, W) fp32 grey on the 0..255 scale; (n, H, W) fp32 is copied."""
    channels = 3 if src.dtype == torch.uint8 else 1
    _dptr(src, torch.uint8 if channels == 3 else torch.float32, "optflow_grey: src")
    if src.dim() != (4 if channels == 3 else 3) or (channels == 3 and src.shape[-1] != 3):
        raise RuntimeError(f"optflow_grey: src: need (n, H, W, 3) uint8 or (n, H, W) float32, got {tuple(src.shape)}")
    n, H, W = (int(v) for v in src.shape[:3])
    dst = torch.empty(n, H, W, dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _check(load().nsff_optflow_grey(src.data_ptr(), dst.data_ptr(), n, H, W, channels, _stream()), "nsff_optflow_grey")
    return dst


def _optflow_planes(name, src, out_hw=None):
    n, H, W = _planes(src, f"optflow_{name}: src")
    oh, ow = ((H + 1) // 2, (W + 1) // 2) if name == "down" else (out_hw or (H, W))
    if name == "up" and ((oh + 1) // 2, (ow + 1) // 2) != (H, W):
        raise RuntimeError(f"optflow_up: a {H} x {W} level is not the half of {oh} x {ow}")
    dst = torch.empty(n, oh, ow, dtype=torch.float32, device=src.device)
    dims = (n, oh, ow) if name == "up" else (n, H, W)
    with torch.cuda.device(src.device):
        _check(getattr(load(), f"nsff_optflow_{name}")(src.data_ptr(), dst.data_ptr(), *dims, _stream()), f"nsff_optflow_{name}")
    return dst


def optflow_down(src):
    """nsff_optflow_down: one pyramid step, (n, H, W) -> (n, (H+1)//2, (W+1)//2)."""
    return _optflow_planes("down", src)


def optflow_up(src, out_hw):
    """nsff_optflow_up: (n, h, w) coarse planes to the finer level out_hw = (H, W), values doubled."""
    return _optflow_planes("up", src, tuple(int(v) for v in out_hw))


def optflow_median(src):
    """nsff_optflow_median: the 3 x 3 median of every (n, H, W) plane, replicated border."""
    return _optflow_planes("median", src)


def optflow_warp(I0, I1, u):
    """nsff_optflow_warp: I0, I1 (P, H, W), u (2, P, H, W) -> consts (5, P, H, W): Ix | Iy | g | rho_c | I1w."""
    P, H, W = _planes(I0, "optflow_warp: I0")
    _dptr(I1, torch.float32, "optflow_warp: I1"), _dptr(u, torch.float32, "optflow_warp: u")
    if tuple(I1.shape) != (P, H, W) or tuple(u.shape) != (2, P, H, W):
        raise RuntimeError(f"optflow_warp: I1 {tuple(I1.shape)} / u {tuple(u.shape)} do not go with I0 {(P, H, W)}")
    consts = torch.empty(5, P, H, W, dtype=torch.float32, device=I0.device)
    with torch.cuda.device(I0.device):
        _check(load().nsff_optflow_warp(I0.data_ptr(), I1.data_ptr(), u.data_ptr(), consts.data_ptr(), P, H, W, _stream()),
               "nsff_optflow_warp")
    return consts


def optflow_result_slot(iters, k):
    return int(load().nsff_optflow_result_slot(int(iters), int(k)))


def optflow_iterate(consts, state, iters, lam=0.15, theta=0.3, tau=0.25, fused=True, tile=0, k=0, other=None):
    """nsff_optflow_iterate: `iters` TV-L1 iterations from state (6, P, H, W) = u1 | u2 | p11 | p12 | p21 | p22 with consts
    (5 or 4, P, H, W); returns the new state (one of `state` -- which is overwritten when more than one launch runs -- and `other`,
    a second buffer of its shape, fresh when None).  fused: k iterations per launch on tile x tile pixels ((0, 0): the default)."""
    _dptr(consts, torch.float32, "optflow_iterate: consts"), _dptr(state, torch.float32, "optflow_iterate: state")
    if state.dim() != 4 or state.shape[0] != 6 or consts.dim() != 4 or consts.shape[0] < 4 or consts.shape[1:] != state.shape[1:]:
        raise RuntimeError(f"optflow_iterate: need state (6, P, H, W) and consts (5, P, H, W), got {tuple(state.shape)} and {tuple(consts.shape)}")
    other = torch.empty_like(state) if other is None else other
    _dptr(other, torch.float32, "optflow_iterate: other")
    if other.shape != state.shape or other.device != state.device or other.data_ptr() == state.data_ptr():
        raise RuntimeError("optflow_iterate: other must be a second buffer of the state's shape and device")
    P, H, W = (int(v) for v in state.shape[1:])
    a = OptflowIterArgs(n_pairs=P, H=H, W=W, iters=int(iters), fused=int(bool(fused)), tile=int(tile), k=int(k), lam=float(lam),
                        theta=float(theta), tau=float(tau), consts=consts.data_ptr())
    a.state[0], a.state[1] = state.data_ptr(), other.data_ptr()
    _launch("nsff_optflow_iterate", a, state.device)
    per_launch = (int(k) or OPTFLOW_K) if fused else 1
    return (state, other)[optflow_result_slot(iters, per_launch)]


def optflow_levels(H, W, levels):
    return int(load().nsff_optflow_levels(int(H), int(W), int(levels)))


def optflow_scratch_bytes(n_pairs, H, W, levels):
    return int(load().nsff_optflow_scratch_bytes(int(n_pairs), int(H), int(W), int(levels)))


def optflow(images0, images1, flow, levels=5, warps=5, iters=30, lam=0.15, theta=0.3, tau=0.25, median=True, fused=True, tile=0, k=0,
            scratch=None):
    """nsff_optflow: flow (P, H, W, 2) fp32 from images0[p] to images1[p] -- (P, H, W, 3) uint8 or (P, H, W) fp32, both alike.
    scratch: a uint8 tensor of optflow_scratch_bytes() bytes, any content (a fresh one when None)."""
    channels = 3 if images0.dtype == torch.uint8 else 1
    dtype = torch.uint8 if channels == 3 else torch.float32
    p0, p1 = _dptr(images0, dtype, "optflow: images0"), _dptr(images1, dtype, "optflow: images1")
    P, H, W = (int(v) for v in images0.shape[:3])
    dev = images0.device
    if images1.shape != images0.shape or images1.device != dev or tuple(flow.shape) != (P, H, W, 2) or flow.device != dev:
        raise RuntimeError(f"optflow: images1 {tuple(images1.shape)} / flow {tuple(flow.shape)} do not go with images0 {tuple(images0.shape)} on {dev}")
    a = OptflowArgs(n_pairs=P, H=H, W=W, channels=channels, levels=int(levels), warps=int(warps), iters=int(iters), median=int(bool(median)),
                    fused=int(bool(fused)), tile=int(tile), k=int(k), lam=float(lam), theta=float(theta), tau=float(tau),
                    images0=p0, images1=p1, flow=_dptr(flow, torch.float32, "optflow: flow"))
    _bind(a, "optflow", dev, ("scratch", _scratch(scratch, True, dev, optflow_scratch_bytes, P, H, W, levels, zeroed=False), _U8, None))
    _launch("nsff_optflow", a, dev)
    return flow


def flow_median(flow, grey, out, valid=None, radius=7, sigma_i=12.75, sigma_s=7.0, tiled=True):
    """nsff_flow_median (csrc/flowmedian.hip): out (P, H, W, 2) fp32 = the image-guided weighted median of flow (P, H, W, 2) fp32 with
    the guide grey (P, H, W) fp32 and valid (P, H, W) uint8 optional; out must not overlap flow."""
    require_gpu_tensor(flow, "flow_median: flow")
    if flow.dim() != 4 or flow.shape[-1] != 2:
        raise RuntimeError(f"flow_median: flow: need (P, H, W, 2), got {tuple(flow.shape)}")
    P, H, W = (int(v) for v in flow.shape[:3])
    px, dev = P * H * W, flow.device
    a = FlowMedianArgs(n_pairs=P, H=H, W=W, radius=int(radius), sigma_i=float(sigma_i), sigma_s=float(sigma_s), tiled=int(bool(tiled)))
    _bind(a, "flow_median", dev, ("flow", flow, _F32, px * 2), ("grey", grey, _F32, px), ("valid", valid, _U8, px), ("out", out, _F32, px * 2))
    _launch("nsff_flow_median", a, dev)
    return out


# ---- disparity from flow and poses (csrc/depth.hip).  Planes are contiguous fp32 (F, H, W) GPU tensors.
def disparity_sparse_scratch_bytes(n_frames, H, W):
    return int(load().nsff_disparity_sparse_scratch_bytes(int(n_frames), int(H), int(W)))


def disparity_sparse(flows_fw, flows_bw, Pm, valid=None, masks=None, min_parallax=0.5, counts=None, scratch=None):
    """nsff_disparity_sparse on (F, H, W, 2) fp32 flows with the parallax rows Pm (F, 2, 12) fp32, valid (F, 2, H, W) uint8 and masks
    (F, H, W) uint8 optional -> (n, c), each (F, H, W) fp32; counts (F,) int64: the known pixels of each frame.  scratch: a uint8
    tensor of disparity_sparse_scratch_bytes() bytes, zero before its first use (a fresh one when None)."""
    require_gpu_tensor(flows_fw, "disparity_sparse: flows_fw")
    F, H, W = (int(v) for v in flows_fw.shape[:3])
    px, dev = F * H * W, flows_fw.device
    n, c = (torch.empty(F, H, W, dtype=torch.float32, device=dev) for _ in range(2))
    a = DisparitySparseArgs(n_frames=F, H=H, W=W, min_parallax=float(min_parallax), n=n.data_ptr(), c=c.data_ptr())
    _bind(a, "disparity_sparse", dev, ("flow_fw", flows_fw, _F32, px * 2), ("flow_bw", flows_bw, _F32, px * 2), ("Pm", Pm, _F32, F * 24),
          ("valid", valid, _U8, px * 2), ("masks", masks, _U8, px), ("counts", counts, _I64, F),
          ("scratch", _scratch(scratch, counts is not None, dev, disparity_sparse_scratch_bytes, F, H, W), _U8, None))
    _launch("nsff_disparity_sparse", a, dev)
    return n, c


def disparity_span_scratch_bytes(n_frames, H, W):
    return int(load().nsff_disparity_span_scratch_bytes(int(n_frames), int(H), int(W)))


def disparity_span(flows_fw, flows_bw, Pm, span, valid=None, masks=None, min_parallax=0.5, counts=None, votes=None, scratch=None,
                   out=None):
    """nsff_disparity_span (csrc/parallax.hip) on (F, H, W, 2) fp32 flows with the parallax rows Pm (F, 2, span, 12) fp32 of the
    neighbours f +- 1 .. f +- span, valid (F, 2, H, W) uint8 and masks (F, H, W) uint8 optional -> (n, c, votes): n and c (F, H, W)
    fp32 (the caller's pair ``out`` or fresh tensors), votes (F, H, W) uint8, the votes of each pixel (a fresh tensor when None).
    counts (F,) int64: the known pixels of each frame.  scratch: a uint8 tensor of disparity_span_scratch_bytes() bytes, zero before
    its first use (a fresh one when None)."""
    require_gpu_tensor(flows_fw, "disparity_span: flows_fw")
    F, H, W = (int(v) for v in flows_fw.shape[:3])
    px, dev, span = F * H * W, flows_fw.device, int(span)
    n, c = out if out is not None else (torch.empty(F, H, W, dtype=torch.float32, device=dev) for _ in range(2))
    if votes is None:
        votes = torch.empty(F, H, W, dtype=torch.uint8, device=dev)
    a = DisparitySpanArgs(n_frames=F, H=H, W=W, span=span, min_parallax=float(min_parallax))
    _bind(a, "disparity_span", dev, ("flow_fw", flows_fw, _F32, px * 2), ("flow_bw", flows_bw, _F32, px * 2), ("n", n, _F32, px),
          ("c", c, _F32, px), ("Pm", Pm, _F32, F * 24 * span), ("valid", valid, _U8, px * 2), ("masks", masks, _U8, px),
          ("votes", votes, _U8, px), ("counts", counts, _I64, F),
          ("scratch", _scratch(scratch, counts is not None, dev, disparity_span_scratch_bytes, F, H, W), _U8, None))
    _launch("nsff_disparity_span", a, dev)
    return n, c, votes


def motion_span_scratch_bytes(n_frames, H, W):
    return int(load().nsff_motion_span_scratch_bytes(int(n_frames), int(H), int(W)))


def motion_span(flows_fw, flows_bw, Fm, hop_scale, span, valid=None, threshold=1.0, err=None, hops=None, raw=None, counts=None,
                scratch=None):
    """nsff_motion_span (csrc/motionspan.hip) on (F, H, W, 2) fp32 flows with the matrices Fm (F, 2, span, 3, 3) fp32 of the neighbours
    f +- 1 .. f +- span and hop_scale (span) fp32, valid (F, 2, H, W) uint8 optional -> raw (F, H, W) uint8 (0 dynamic, 255 static; a
    fresh tensor when None), returned; err (F, 2, H, W) fp32, hops (F, 2, H, W) uint8, counts (F, 3) int64 [over fw, over bw, dynamic]
    -- whichever are given.  scratch: a uint8 tensor of motion_span_scratch_bytes() bytes, zero before its first use (a fresh one
    when None)."""
    require_gpu_tensor(flows_fw, "motion_span: flows_fw")
    F, H, W = (int(v) for v in flows_fw.shape[:3])
    px, dev, span = F * H * W, flows_fw.device, int(span)
    if raw is None:
        raw = torch.empty(F, H, W, dtype=torch.uint8, device=dev)
    a = MotionSpanArgs(n_frames=F, H=H, W=W, span=span, threshold=float(threshold))
    _bind(a, "motion_span", dev, ("flow_fw", flows_fw, _F32, px * 2), ("flow_bw", flows_bw, _F32, px * 2), ("Fm", Fm, _F32, F * 18 * span),
          ("hop_scale", hop_scale, _F32, span), ("valid", valid, _U8, px * 2), ("err", err, _F32, px * 2), ("hops", hops, _U8, px * 2),
          ("raw", raw, _U8, px), ("counts", counts, _I64, F * 3),
          ("scratch", _scratch(scratch, counts is not None, dev, motion_span_scratch_bytes, F, H, W), _U8, None))
    _launch("nsff_motion_span", a, dev)
    return raw


def mask_propagate(src, flows_fw, flows_bw, reach, valid=None, dst=None, hits=None, zero_counts=None, scratch=None):
    """nsff_mask_propagate (csrc/motionspan.hip): dst (F, H, W) uint8 = src with "dynamic" (0) carried along the chained flow from
    the frames f +- 1 .. f +- reach (a fresh tensor when None), returned; hits (F, H, W) uint8 and zero_counts (F,) int64 where
    given.  scratch as for motion_span."""
    require_gpu_tensor(src, "mask_propagate: src")
    F, H, W = (int(v) for v in src.shape)
    px, dev = F * H * W, src.device
    if dst is None:
        dst = torch.empty(F, H, W, dtype=torch.uint8, device=dev)
    a = MaskPropagateArgs(n_frames=F, H=H, W=W, reach=int(reach))
    _bind(a, "mask_propagate", dev, ("src", src, _U8, px), ("flow_fw", flows_fw, _F32, px * 2), ("flow_bw", flows_bw, _F32, px * 2),
          ("valid", valid, _U8, px * 2), ("dst", dst, _U8, px), ("hits", hits, _U8, px), ("zero_counts", zero_counts, _I64, F),
          ("scratch", _scratch(scratch, zero_counts is not None, dev, motion_span_scratch_bytes, F, H, W), _U8, None))
    _launch("nsff_mask_propagate", a, dev)
    return dst


def _same_planes(who, first, **others):
    shape = _planes(first, f"{who}: c")
    for name, t in others.items():
        if _planes(t, f"{who}: {name}") != shape or t.device != first.device:
            raise RuntimeError(f"{who}: {name} {tuple(t.shape)} on {t.device} does not go with c {shape} on {first.device}")
    return shape


def disparity_push(c, n, grey):
    """nsff_disparity_push: one pyramid step of the planes c, n, grey, (F, H, W) -> (F, (H+1)//2, (W+1)//2) each."""
    F, H, W = _same_planes("disparity_push", c, n=n, grey=grey)
    out = tuple(torch.empty(F, (H + 1) // 2, (W + 1) // 2, dtype=torch.float32, device=c.device) for _ in range(3))
    with torch.cuda.device(c.device):
        _check(load().nsff_disparity_push(c.data_ptr(), n.data_ptr(), grey.data_ptr(), *(t.data_ptr() for t in out), F, H, W, _stream()),
               "nsff_disparity_push")
    return out


def disparity_pull(c, n, parent, hw=None):
    """nsff_disparity_pull: d = n / c where c > 0, else the parent's value at (y >> 1, x >> 1) (parent None: 0).  c and n None: the
    nearest-neighbour upsampling of parent to hw = (H, W)."""
    if c is None:
        F, (H, W) = _planes(parent, "disparity_pull: parent")[0], (int(v) for v in hw)
        dev = parent.device
    else:
        F, H, W = _same_planes("disparity_pull", c, n=n)
        dev = c.device
    if parent is not None and (_planes(parent, "disparity_pull: parent") != (F, (H + 1) // 2, (W + 1) // 2) or parent.device != dev):
        raise RuntimeError(f"disparity_pull: parent {tuple(parent.shape)} is not the level above {(F, H, W)}")
    d = torch.empty(F, H, W, dtype=torch.float32, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        _check(load().nsff_disparity_pull(ptr(c), ptr(n), ptr(parent), d.data_ptr(), F, H, W, _stream()), "nsff_disparity_pull")
    return d


def disparity_result_slot(iters, k):
    return int(load().nsff_disparity_result_slot(int(iters), int(k)))


def disparity_relax(d, n, c, grey, iters, lam=8.0, sigma=12.75, fused=False, tile=0, k=0, other=None):
    """nsff_disparity_relax: `iters` weighted-Jacobi iterations from d (F, H, W) with the planes n, c and the guide grey; returns the
    new d (one of `d` -- which is overwritten when more than one launch runs -- and `other`, a second buffer of its shape, fresh
    when None).  fused: k iterations per launch on tile x tile pixels ((0, 0): the default pair)."""
    F, H, W = _same_planes("disparity_relax", c, n=n, grey=grey, d=d)
    other = torch.empty_like(d) if other is None else other
    _dptr(other, torch.float32, "disparity_relax: other")
    if other.shape != d.shape or other.device != d.device or other.data_ptr() == d.data_ptr():
        raise RuntimeError("disparity_relax: other must be a second buffer of d's shape and device")
    a = DisparityRelaxArgs(n_frames=F, H=H, W=W, iters=int(iters), fused=int(bool(fused)), tile=int(tile), k=int(k), lam=float(lam),
                           sigma=float(sigma), n=n.data_ptr(), c=c.data_ptr(), grey=grey.data_ptr())
    a.state[0], a.state[1] = d.data_ptr(), other.data_ptr()
    _launch("nsff_disparity_relax", a, d.device)
    per_launch = (int(k) or DISPARITY_K) if fused else 1
    return (d, other)[disparity_result_slot(iters, per_launch)]


def disparity_levels(H, W):
    return int(load().nsff_disparity_levels(int(H), int(W)))


def disparity_dense_scratch_bytes(n_frames, H, W):
    return int(load().nsff_disparity_dense_scratch_bytes(int(n_frames), int(H), int(W)))


def disparity_dense(n, c, grey, disps, levels=3, iters=30, lam=8.0, sigma=12.75, fused=False, tile=0, k=0, scratch=None):
    """nsff_disparity_dense: disps (F, H, W) fp32 from the planes n, c and the guide grey.  scratch: a uint8 tensor of
    disparity_dense_scratch_bytes() bytes, any content (a fresh one when None)."""
    F, H, W = _same_planes("disparity_dense", c, n=n, grey=grey, disps=disps)
    a = DisparityDenseArgs(n_frames=F, H=H, W=W, levels=int(levels), iters=int(iters), fused=int(bool(fused)), tile=int(tile), k=int(k),
                           lam=float(lam), sigma=float(sigma), n=n.data_ptr(), c=c.data_ptr(), grey=grey.data_ptr(), disps=disps.data_ptr())
    dev = c.device
    _bind(a, "disparity_dense", dev, ("scratch", _scratch(scratch, True, dev, disparity_dense_scratch_bytes, F, H, W, zeroed=False), _U8, None))
    _launch("nsff_disparity_dense", a, dev)
    return disps


def cdf(weights, out):
    """out (F, N) fp64 = per-frame inclusive prefix sum of weights (F, N) fp32."""
    F, N = weights.shape
    if tuple(out.shape) != (F, N):
        raise RuntimeError("cdf: output shape mismatch")
    with torch.cuda.device(weights.device):
        _check(load().nsff_cdf(_dptr(weights, torch.float32, "cdf: weights"), F, N, _dptr(out, torch.float64, "cdf: out"),
                               _stream()), "nsff_cdf")


def ray_draw(records, frame, u, cdf, out):
    """nsff_ray_draw: records (N_frames, N_pixels, 16) fp32, u (B) fp32 uniforms, cdf (N_frames, N_pixels) fp64 or None
    (uniform); out: the batch tensors by name (_DRAW_OUT; cam_ids / rand_idx may be absent)."""
    NF, NP = int(records.shape[0]), int(records.shape[1])
    if records.dim() != 3 or records.shape[2] != RAY_RECORD:
        raise RuntimeError(f"ray_draw: records must be (N_frames, N_pixels, {RAY_RECORD})")
    B = int(u.numel())
    a = RayDrawArgs(n_frames=NF, n_pixels=NP, frame=int(frame), batch=B, records=_dptr(records, torch.float32, "ray_draw: records"),
                    cdf=_dptr(cdf, torch.float64, "ray_draw: cdf"), u=_dptr(u, torch.float32, "ray_draw: u"))
    for n in _DRAW_OUT:
        t = out.get(n)
        setattr(a, n, _dptr(t, torch.int64 if n in ("ts", "cam_ids", "rand_idx") else torch.float32, f"ray_draw: {n}"))
    with torch.cuda.device(records.device):
        _check(load().nsff_ray_draw(C.byref(a), _stream()), "nsff_ray_draw")


def ray_records(K4, frame_table, images, disps, masks, flow_fw, flow_bw, near, first_frame, frame_count, records):
    """nsff_ray_records: images (F,H,W,3) uint8 / fp32, disps (F,H,W) fp32, masks (F,H,W) uint8 / fp32, flows (F,H,W,2) fp32 or
    None, frame_table (F, FRAME_TABLE) fp32, all on the GPU -> records[first_frame : first_frame + frame_count] of the
    (F, H*W, 16) output, one launch."""
    F, H, W = (int(v) for v in images.shape[:3])

    def either(t, what):
        if t.dtype not in (torch.uint8, torch.float32):
            raise RuntimeError(f"{what}: need a uint8 or float32 tensor, got {t.dtype}")
        return _dptr(t, t.dtype, what)
    a = RayRecordArgs(n_frames=F, H=H, W=W, first_frame=int(first_frame), frame_count=int(frame_count),
                      image_u8=int(images.dtype == torch.uint8), mask_u8=int(masks.dtype == torch.uint8),
                      fx=float(K4[0]), fy=float(K4[1]), cx=float(K4[2]), cy=float(K4[3]), near=float(near),
                      n_pixels=int(records.shape[1]), images=either(images, "ray_records: images"),
                      disps=_dptr(disps, torch.float32, "ray_records: disps"), masks=either(masks, "ray_records: masks"),
                      flow_fw=_dptr(flow_fw, torch.float32, "ray_records: flows_fw"),
                      flow_bw=_dptr(flow_bw, torch.float32, "ray_records: flows_bw"),
                      frame_table=_dptr(frame_table, torch.float32, "ray_records: frame table"),
                      records=_dptr(records, torch.float32, "ray_records: out"))
    _launch("nsff_ray_records", a, records.device)


def resize_ksize(filter, n_in, n_out):
    """nsff_resize_ksize: weights per output index of the table, or the (negative) error code."""
    return int(load().nsff_resize_ksize(int(filter), int(n_in), int(n_out)))


def resize_table(filter, n_in, n_out):
    """nsff_resize_table on the host: (start (n_out) int32, count (n_out) int32, weights (n_out, ksize) int32 / fp32 or None) as
    CPU tensors.  A Lanczos table wider than RESIZE_MAX_KSIZE (a downscale beyond 8x) is refused."""
    filter, n_in, n_out = int(filter), int(n_in), int(n_out)
    ksize = resize_ksize(filter, n_in, n_out)
    if ksize == ERR_UNSUPPORTED:
        raise RuntimeError(f"resize: {n_in} -> {n_out} is a {n_in / n_out:.2f}x downscale; the Lanczos kernel holds tables up to "
                           f"{RESIZE_MAX_KSIZE} taps, a downscale of at most 8x")
    if ksize < 0:
        _check(ksize, "nsff_resize_ksize")
    start, count = torch.empty(n_out, dtype=torch.int32), torch.empty(n_out, dtype=torch.int32)
    weights = None
    if filter in (RESIZE_LANCZOS_U8, RESIZE_LINEAR_CV):
        weights = torch.empty(n_out, ksize, dtype=torch.int32 if filter == RESIZE_LANCZOS_U8 else torch.float32)
    _check(load().nsff_resize_table(filter, n_in, n_out, start.data_ptr(), count.data_ptr(),
                                    None if weights is None else weights.data_ptr()), "nsff_resize_table")
    return start, count, weights


def frame_resize(filter, src, dst, x_table, y_table, ratio=(1.0, 1.0)):
    """nsff_frame_resize: src (F, h, w, C) -> dst (F, H, W, C), contiguous GPU tensors, uint8 (LANCZOS_U8, NEAREST_PIL) or fp32;
    x_table / y_table: resize_table()'s triples for (w -> W) and (h -> H) on the same device."""
    filter = int(filter)
    dtype = torch.uint8 if filter in (RESIZE_LANCZOS_U8, RESIZE_NEAREST_PIL) else torch.float32
    F, h, w, ch = (int(v) for v in src.shape)
    if dst.dim() != 4 or int(dst.shape[0]) != F or int(dst.shape[3]) != ch or dst.device != src.device:
        raise RuntimeError(f"frame_resize: dst {tuple(dst.shape)} on {dst.device} does not go with src {tuple(src.shape)} on {src.device}")
    H, W = int(dst.shape[1]), int(dst.shape[2])
    a = FrameResizeArgs(n_frames=F, filter=filter, channels=ch, src_h=h, src_w=w, dst_h=H, dst_w=W,
                        src=_dptr(src, dtype, "frame_resize: src"), dst=_dptr(dst, dtype, "frame_resize: dst"))
    a.ratio[0], a.ratio[1] = float(ratio[0]), float(ratio[1])
    wdtype = torch.int32 if filter == RESIZE_LANCZOS_U8 else torch.float32
    for axis, (start, count, weights), n in (("x", x_table, W), ("y", y_table, H)):
        if start.numel() != n or count.numel() != n or start.device != src.device:
            raise RuntimeError(f"frame_resize: the {axis} table has {start.numel()} entries on {start.device}, expected {n} on {src.device}")
        setattr(a, f"{axis}_start", _dptr(start, torch.int32, f"frame_resize: {axis}_start"))
        setattr(a, f"{axis}_count", _dptr(count, torch.int32, f"frame_resize: {axis}_count"))
        setattr(a, f"{axis}_weights", _dptr(weights, wdtype, f"frame_resize: {axis}_weights"))
        setattr(a, f"ksize_{axis}", 1 if weights is None else int(weights.shape[1]))
    _launch("nsff_frame_resize", a, src.device)


def scene_scale_work_bytes(n_frames, n_points, H, W):
    """nsff_scene_scale_work_bytes: the workspace of one scene_scale call in bytes, 0 where the shape is refused."""
    return int(load().nsff_scene_scale_work_bytes(int(n_frames), int(n_points), int(H), int(W)))


def scene_scale(points, vis, w2c, K, disps, disp_rank, want_pix=False, work=None, out=None):
    """nsff_scene_scale on contiguous GPU tensors: points (N,3) fp64, vis (F,N) uint8, w2c (F,3,4) fp64, K (3,3) fp32, disps
    (F,H,W) fp32; disp_rank: the two 0-based ranks of the disparity order statistics.  Returns (stats (F,8) fp64, disp_os (F,2)
    fp32, depth_os (F,2) fp64, pix (F,N) int32 or None) on the device.  work: a uint8 GPU tensor of scene_scale_work_bytes()
    bytes with any content (a fresh one when None); out: write into these four tensors (pix may be None) instead of new ones."""
    require_gpu_tensor(disps, "scene_scale: disps")
    if disps.dim() != 3 or vis.dim() != 2 or points.dim() != 2:
        raise RuntimeError(f"scene_scale: need disps (F,H,W), vis (F,N) and points (N,3), got {tuple(disps.shape)}, "
                           f"{tuple(vis.shape)} and {tuple(points.shape)}")
    (F, H, W), N, dev = (int(v) for v in disps.shape), int(points.shape[0]), disps.device
    if tuple(points.shape) != (N, 3) or tuple(vis.shape) != (F, N) or tuple(w2c.shape) != (F, 3, 4) or tuple(K.shape) != (3, 3):
        raise RuntimeError(f"scene_scale: points {tuple(points.shape)}, vis {tuple(vis.shape)}, w2c {tuple(w2c.shape)}, K "
                           f"{tuple(K.shape)} do not go with {F} frames of {N} points")
    need = scene_scale_work_bytes(F, N, H, W)
    if work is None and need > 0:
        work = torch.empty(need, dtype=torch.uint8, device=dev)
    if out is not None:
        stats, disp_os, depth_os, pix = out
        if (stats.numel(), disp_os.numel(), depth_os.numel()) != (8 * F, 2 * F, 2 * F) or (pix is not None and pix.numel() != F * N):
            raise RuntimeError(f"scene_scale: out must be (F,8), (F,2), (F,2) and (F,N) or None for F = {F}, N = {N}")
    else:
        stats = torch.empty(F, 8, dtype=torch.float64, device=dev)
        disp_os = torch.empty(F, 2, dtype=torch.float32, device=dev)
        depth_os = torch.empty(F, 2, dtype=torch.float64, device=dev)
        pix = torch.empty(F, N, dtype=torch.int32, device=dev) if want_pix else None
    a = SceneScaleArgs(n_frames=F, n_points=N, H=H, W=W, disp_rank=(C.c_int32 * 2)(int(disp_rank[0]), int(disp_rank[1])),
                       points=_dptr(points, torch.float64, "scene_scale: points"), vis=_dptr(vis, torch.uint8, "scene_scale: vis"),
                       w2c=_dptr(w2c, torch.float64, "scene_scale: w2c"), K=_dptr(K, torch.float32, "scene_scale: K"),
                       disps=_dptr(disps, torch.float32, "scene_scale: disps"), stats=_dptr(stats, torch.float64, "scene_scale: stats"),
                       disp_os=_dptr(disp_os, torch.float32, "scene_scale: disp_os"),
                       depth_os=_dptr(depth_os, torch.float64, "scene_scale: depth_os"), pix=_dptr(pix, torch.int32, "scene_scale: pix"),
                       work=_dptr(work, torch.uint8, "scene_scale: work"), work_bytes=0 if work is None else work.numel())
    _launch("nsff_scene_scale", a, dev)
    return stats, disp_os, depth_os, pix


def range_flags(out, clear):
    """nsff_range_flags: the current device's value-domain word -> out (a 1-element int32 GPU tensor), cleared when `clear`"""
    assert out.is_cuda and out.dtype == torch.int32 and out.numel() >= 1
    _check(load().nsff_range_flags(out.data_ptr(), 1 if clear else 0, _stream()), "nsff_range_flags")


def last_field_kernel():
    """name of the kernel the last field_query of this process launched (include/nsff_render.h: NSFF_KERNEL_*)"""
    return KERNEL_NAMES[load().nsff_last_field_kernel()]


def last_field_grid():
    """Workgroups of the last field launch when it ran the hand-scheduled inference kernel (0 otherwise): the CU count for a
    persistent launch, one (two: both trunks) per 128-point tile otherwise (include/nsff_render.h::nsff_last_field_grid)."""
    return int(load().nsff_last_field_grid())


def h3a_program(model, static_mode, transient_mode, fold_t=False, side_fold=False, persist=False):
    """(steps, n_static_steps, phases_static, phases_dynamic) of an f16x3 inference launch, from the host-side builders alone
    (no GPU): steps = [(w_off_words, bias_off_words or None, nks, pre, post, head)], phases_* = [[8 dwords]] or [].
    fold_t: the dynamic trunk's program of a launch that is given t_bias (time code folded into per-ray bias rows);
    side_fold: the static trunk's program of a view-direction launch that is given s_bias ([dir | a] folded into per-ray rows);
    persist: the programs of a persistent launch (the last segment's B phase requests the next tile's first weight slots; [] for a
    trunk that does not end with a 256-wide segment)."""
    desc = model_desc(model)
    steps = (C.c_uint32 * (28 * 4))()
    ps, pd = (C.c_uint32 * (36 * 8))(), (C.c_uint32 * (36 * 8))()
    n, ns, nph = C.c_int(0), C.c_int(0), (C.c_int * 2)()
    _check(load().nsff_field_phase_program(C.byref(desc), int(static_mode), int(transient_mode), int(bool(fold_t)) | (2 if side_fold else 0) | (4 if persist else 0), steps, C.byref(n), C.byref(ns), ps, pd, nph),
           "nsff_field_phase_program")
    out = []
    for i in range(n.value):
        w, b, packed = steps[4 * i], steps[4 * i + 1], steps[4 * i + 2]
        out.append((w, None if b == 0xFFFFFFFF else b, packed & 0xFF, (packed >> 8) & 0xFF, (packed >> 16) & 0xFF, packed >> 24))
    rows = lambda arr, k: [[int(arr[8 * i + j]) for j in range(8)] for i in range(k)]
    return out, ns.value, rows(ps, nph[0]), rows(pd, nph[1])


def prof_enable(on):
    _check(load().nsff_prof_enable(int(bool(on))), "nsff_prof_enable")


def prof_collect():
    """(launches, ms, algorithmic flops, executed flops, shader clock in GHz or None) of the field launches since prof_enable."""
    n, ms, fl, ex, tk, tms = C.c_int64(0), C.c_double(0), C.c_double(0), C.c_double(0), C.c_double(0), C.c_double(0)
    _check(load().nsff_prof_collect_clock(C.byref(n), C.byref(ms), C.byref(fl), C.byref(ex), C.byref(tk), C.byref(tms)),
           "nsff_prof_collect_clock")
    ghz = tk.value / tms.value * 1e-6 if tms.value > 0 else None
    if ghz is not None and not (0.5 < ghz < 3.0):       # counters of different XCDs disagreeing, a wrapped stamp: no claim
        ghz = None
    return n.value, ms.value, fl.value, ex.value, ghz
