"""ctypes binding of libgsaj_hip.so (C ABI: include/gsaj.h).

The library is the product: there is no Python / CPU fallback.  If it has not been built
(`python __graft_entry__.py build` or `make -C gs-slam-analytica_jacobian_amd/csrc`) importing
this module raises ImportError -- loudly, so a GPU run can never silently use something else.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
CSRC = os.path.join(PKG_ROOT, "csrc")
LIB_PATH = os.environ.get("GSAJ_LIB_PATH") or os.path.join(PKG_ROOT, "lib", "libgsaj_hip.so")  # override: A/B kernel experiments
HEADER = os.path.join(os.path.dirname(PKG_ROOT), "include", "gsaj.h")

c_int, c_float, c_double, c_size_t, c_void_p = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t, ctypes.c_void_p
P = c_void_p  # every device / host pointer travels as void*

# ---- the argument groups of the rasteriser entry points, each spelled once (the groups csrc/api.hip and gsaj/rasterizer.py build;
# DESIGN.md "Argument groups"); tests/test_cpu_signatures.py holds every entry against the header type by type
_PDM = [c_int, c_int, c_int]                        # P, D, M
_BG_WH = [P, c_int, c_int]                          # bg, W, H
_SCENE_BWD = [P, P, P, P, c_float, P, P]            # means3D, shs, colors_precomp, scales, scale_modifier, rotations, cov3D_precomp
_SCENE_FWD = _SCENE_BWD[:3] + [P] + _SCENE_BWD[3:]  # the forward family has opacities after colors_precomp
_VIEW_FWD = [P, P, P, c_float, c_float]             # viewmatrix, projmatrix, campos, tanfovx, tanfovy
_VIEW_BWD = _VIEW_FWD[:2] + [P] + _VIEW_FWD[2:]     # the backward family has projmatrix_raw after projmatrix
_FWD_OUT = [P] * 5                                  # out_color, out_depth, out_opacity, radii, n_touched
_FWD_STATE = _FWD_OUT + [P, P, c_size_t, c_int, c_int, P, c_int]  # + geom_ws, binning_ws, binning_ws_bytes, capacity, tile_list_capacity, image_ws, flags
_BWD_STATE = [P] * 4                                # radii, geom_ws, binning_ws, image_ws
_LOSS = [c_int, c_float, c_float]                   # loss_flags, alpha, rgb_boundary_threshold
_IMAGES = [P] * 3                                   # color, depth, opacity: the forward's images (the backward forms of the loss)
_LOSS_GT = [P] * 5                                  # gt_color, gt_depth, grad_mask, exposure_a, exposure_b
_GRADS = [P] * 12                                   # dL_dmean2D .. dL_drot, dL_dtau, dL_dtau_sum
_FWD = _PDM + _BG_WH + _SCENE_FWD + _VIEW_FWD + [c_int]                        # P .. prefiltered of the one-call forwards
_BWD = _PDM + [c_int] + _BG_WH + _SCENE_BWD + _VIEW_BWD + _BWD_STATE          # P, D, M, R .. image_ws of everything run on a finished forward
_BWD_BATCH = [c_int] + _PDM + [c_int] + _BWD[4:]                              # K, P, D, M, capacity ..
_PREPROCESS = _PDM + [c_int, c_int] + _SCENE_FWD + _VIEW_FWD + [c_int, P, P, P, P]  # P, D, M, W, H .. prefiltered, radii, n_touched, geom_ws, image_ws
_JAC_LOSS = _BWD + [P] + _LOSS + _IMAGES + _LOSS_GT + [c_float, P, P, P]      # .. jac_ws, the loss, irls_delta, gn_partials, jac_out, stream
_JAC_LOSS_BATCH = _BWD_BATCH + _LOSS + _IMAGES + _LOSS_GT + [c_int, P, c_float, P, P, P]  # .. exposure_stride, jac_ws, irls_delta, gn_partials, jac_out, stream
_GN_STEP_BATCH = [c_int, P, c_int, P] + [c_float] * 5 + [P, P, P, c_size_t, P]  # K, partials, n_partials, active, the LM scalars, projection, states, skip, its stride, stream

# name -> (restype, argtypes); must list every function include/gsaj.h declares
SIGNATURES = {
    "gsaj_last_error": (ctypes.c_char_p, []),
    "gsaj_version": (c_int, []),
    "gsaj_geom_workspace_bytes": (c_size_t, [c_int]),
    "gsaj_image_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gsaj_binning_workspace_bytes": (c_size_t, [c_int]),
    "gsaj_forward_preprocess": (c_int, _PREPROCESS + [P]),
    "gsaj_forward_num_rendered": (c_int, [c_int, c_int, P, P, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "gsaj_forward_render": (c_int, [c_int] * 5 + [P, P, P, P, P, c_size_t, P, P, P, P, P, c_int, P]),
    "gsaj_rasterize_forward": (c_int, _FWD + _FWD_OUT + [P, P, c_size_t, P, ctypes.POINTER(c_int), c_int, P]),
    "gsaj_rasterize_forward_async": (c_int, _FWD + _FWD_STATE + [P]),
    "gsaj_rasterize_forward_batch": (c_int, [c_int] + _FWD + _FWD_STATE + [P]),
    "gsaj_rasterize_backward_batch": (c_int, _BWD_BATCH + [P, P] + _GRADS + [c_int, P]),
    "gsaj_fused_loss_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gsaj_rasterize_forward_loss": (c_int, _FWD + _FWD_STATE + _LOSS + _LOSS_GT + [P, P, P]),
    "gsaj_rasterize_backward_loss": (c_int, _BWD + _LOSS + _IMAGES + _LOSS_GT + _GRADS + [P]),
    "gsaj_fused_loss_batch_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gsaj_rasterize_forward_loss_batch": (c_int, [c_int] + _FWD + _FWD_STATE + _LOSS + _LOSS_GT + [c_int, P, P, P, P]),
    "gsaj_rasterize_backward_loss_batch": (c_int, _BWD_BATCH + _LOSS + _IMAGES + _LOSS_GT + [c_int] + _GRADS + [c_int, P]),
    "gsaj_forward_aborted_count": (c_int, [c_int, c_int, P, P, ctypes.POINTER(c_int)]),
    "gsaj_set_tile_band": (c_int, [c_int, c_int, P, c_int, c_int, P]),
    "gsaj_forward_preprocess_cap": (c_int, _PREPROCESS + [c_int, c_int, P]),
    "gsaj_rasterize_backward": (c_int, _BWD + [P, P] + _GRADS + [P]),
    "gsaj_mark_visible": (c_int, [c_int, P, P, P, P, P]),
    "gsaj_debug_export": (c_int, [c_int] * 4 + [P] * 3 + [P] * 11 + [P]),
    "gsaj_debug_launch_plan": (c_int, [c_int] * 4 + [ctypes.POINTER(c_int)]),
    "gsaj_debug_lds_budget": (c_int, [c_int] * 8 + [ctypes.POINTER(c_int)]),
    "gsaj_debug_export_taken": (c_int, [c_int, c_int, c_int, P, P, P, P, P]),
    "gsaj_debug_export_view_sums": (c_int, [c_int, P, P, P]),
    "gsaj_debug_export_view_sums_gather": (c_int, [c_int, c_int, c_int, c_int, P, P, P, P, P]),
    "gsaj_profile_begin": (c_int, [c_int]),
    "gsaj_profile_end": (c_int, [P, P]),
    "gsaj_dense_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gsaj_dense_backward": (c_int, [c_int, c_int, c_int] + [P] * 7 + [P] * 4 + [P, c_int, P, P]),
    "gsaj_dense_project_workspace_bytes": (c_size_t, [c_int]),
    "gsaj_dense_project": (c_int, [c_int] * 5 + [P] * 6 + [c_double, c_double] + [P] * 6 + [P, P]),
    "gsaj_dense_render": (c_int, [c_int, c_int, c_int] + [P] * 5 + [P, P, P]),
    "gsaj_pose_jacobians": (c_int, [c_int, P, P, P, c_double, c_double, c_int, c_int, P, P, P]),
    "gsaj_dense_tau": (c_int, [c_int, c_int, c_int] + [P] * 11 + [P, P, P]),
    "gsaj_dist2_workspace_bytes": (c_size_t, [c_int]),
    "gsaj_dist2": (c_int, [c_int, P, P, P, P]),
    "gsaj_debug_dist2_order": (c_int, [c_int, P, P, P, P]),
    "gsaj_pose_state_floats": (c_int, []),
    "gsaj_pose_adam_step": (c_int, [P, P] + [c_float] * 8 + [P, P, P, P]),
    "gsaj_pose_adam_step_batch": (c_int, [c_int, P, P, P] + [c_float] * 8 + [P, P, P, c_size_t, P]),
    "gsaj_forward_abort_flag": (c_void_p, [c_int, c_int, P]),
    "gsaj_loss_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gsaj_densification_stats": (c_int, [c_int, c_int] + [P] * 7 + [P]),
    "gsaj_isotropic_workspace_bytes": (c_size_t, [c_int]),
    "gsaj_isotropic_loss": (c_int, [c_int, c_int, c_float, P, P, c_int, P, P, P]),
    "gsaj_loss_seeds": (c_int, [c_int, c_int, c_int, c_float, c_float] + [P] * 8 + [P] * 4 + [P, P]),
    "gsaj_loss_seeds_batch": (c_int, [c_int] + [c_int, c_int, c_int, c_float, c_float] + [P] * 8 + [P] * 4 + [P, P]),
    "gsaj_ssim_workspace_bytes": (c_size_t, [c_int] * 4),
    "gsaj_ssim_forward": (c_int, [c_int] * 4 + [P] * 6),
    "gsaj_ssim_backward": (c_int, [c_int] * 4 + [P] * 6),
    "gsaj_refine_loss_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gsaj_refine_loss_seeds": (c_int, [c_int, c_int, c_float] + [P] * 6),
    "gsaj_seed_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gsaj_depth_stats": (c_int, [c_int, c_int, P, P, c_float, P, P, c_float, P, P, P, P]),
    "gsaj_keyframe_depth_prior": (c_int, [c_int, c_int, P, P, P, c_float, P, P, P, P, P]),
    "gsaj_seed_select": (c_int, [c_int, c_int, P, P, c_float, c_float, c_double, ctypes.c_uint32, P, P]),
    "gsaj_seed_count": (c_int, [P, P, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "gsaj_debug_seed_pixels": (c_int, [c_int, c_int, c_int, P, P, P]),
    "gsaj_seed_gaussians": (c_int, [c_int, c_int, c_int, P, P, P, P] + [c_double] * 4 + [c_float, c_int, c_int, c_int] + [P] * 6 + [P, P, P]),
    "gsaj_grad_mask_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gsaj_grad_intensity": (c_int, [c_int, c_int, P, P, P]),
    "gsaj_grad_mask": (c_int, [c_int, c_int, P, c_float, c_int, P, P, P, P]),
    "gsaj_covis_pack": (c_int, [c_int, c_int, P, ctypes.POINTER(c_int), ctypes.c_uint32, P, P]),
    "gsaj_covis_query": (c_int, [c_int, P, P, c_int, ctypes.c_uint32, P, P]),
    "gsaj_covis_prune_mask": (c_int, [c_int, P, ctypes.c_uint32, P, c_int, c_int, P, P, P, P]),
    "gsaj_compact_workspace_bytes": (c_size_t, [c_int]),
    "gsaj_compact_plan": (c_int, [c_int, P, c_int, P, P]),
    "gsaj_compact_count": (c_int, [P, P, ctypes.POINTER(c_int)]),
    "gsaj_compact_rows": (c_int, [c_int, c_int, ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), ctypes.POINTER(c_int), P, P]),
    "gsaj_densify_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gsaj_densify_plan": (c_int, [c_int] * 4 + [P, P, c_int, P, P] + [c_float] * 4 + [c_int, c_int, P, P, P]),
    "gsaj_densify_counts": (c_int, [P, P, ctypes.POINTER(c_int)]),
    "gsaj_densify_rows": (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), ctypes.POINTER(c_int),
                                  ctypes.POINTER(c_int), P, P, P]),
    "gsaj_densify_children": (c_int, [c_int, c_int, c_int, P, P, P, P, ctypes.c_uint64, P, P, P, P, P]),
    "gsaj_densify_noise": (c_int, [c_int, c_int, ctypes.c_uint64, P, P]),
    "gsaj_map_step": (c_int, [c_int, c_int, c_int, c_int, P, P]),
    "gsaj_eval_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gsaj_eval_frame": (c_int, [c_int, c_int, c_int, c_int] + [P] * 7),
    "gsaj_pose_jac_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gsaj_pose_jac_partial_rows": (c_int, [c_int, c_int]),
    "gsaj_rasterize_pose_jacobian": (c_int, _BWD + [P] + [P] * 5 + [P] * 4 + [P]),
    "gsaj_rasterize_pose_jacobian_loss": (c_int, _JAC_LOSS),
    "gsaj_gn_state_floats": (c_int, []),
    "gsaj_pose_gn_step": (c_int, [P, c_int] + [c_float] * 5 + [P, P, P, P]),
    "gsaj_rasterize_pose_jacobian_loss8": (c_int, _JAC_LOSS),
    "gsaj_gn8_state_floats": (c_int, []),
    "gsaj_pose_gn8_step": (c_int, [P, c_int] + [c_float] * 5 + [P, P, P, P]),
    "gsaj_pose_jac_batch_workspace_bytes": (c_size_t, [c_int] * 4),
    "gsaj_rasterize_pose_jacobian_loss_batch": (c_int, _JAC_LOSS_BATCH),
    "gsaj_rasterize_pose_jacobian_loss8_batch": (c_int, _JAC_LOSS_BATCH),
    "gsaj_pose_gn_step_batch": (c_int, _GN_STEP_BATCH),
    "gsaj_pose_gn8_step_batch": (c_int, _GN_STEP_BATCH),
    "gsaj_pose_gn_select": (c_int, [c_int, P, c_int, P, P, P, P]),
    "gsaj_pyramid_bytes": (c_size_t, [c_int] * 5),
    "gsaj_pyramid_level": (c_int, [c_int] * 6 + [ctypes.POINTER(c_int)] * 2 + [ctypes.POINTER(c_size_t)] * 3),
    "gsaj_pyramid_build": (c_int, [c_int, c_int, c_int, P, P, P, c_float, P, P]),
    "gsaj_pose_gn_relevel": (c_int, [P, c_int, P, c_float, P, P]),
    "gsaj_undistort_map": (c_int, [c_int, c_int, P, P, P, P, P, P]),
    "gsaj_frame_ingest": (c_int, [c_int] * 5 + [c_size_t, P, P, P, P, c_size_t, c_double, c_int, P, P, P]),
    "gsaj_stereo_workspace_bytes": (c_int, [c_int] * 4 + [ctypes.POINTER(c_size_t)]),
    "gsaj_debug_stereo_offsets": (c_int, [c_int] * 4 + [ctypes.POINTER(c_size_t)] * 2),
    "gsaj_rectify_u8": (c_int, [c_int] * 4 + [c_size_t, P, P, P, P, c_size_t, P, P]),
    "gsaj_stereo_match": (c_int, [c_int, c_int, P, c_size_t, P, c_size_t] + [c_int] * 8 + [P, c_size_t, P, P, c_double, P]),
    "gsaj_rgbd_align_partial_rows": (c_int, [c_int, c_int]),
    "gsaj_rgbd_align": (c_int, [c_int, c_int] + [c_float] * 4 + [P] * 6 + [c_float] * 7 + [P] * 6),
    "gsaj_rgbd_align8": (c_int, [c_int, c_int] + [c_float] * 4 + [P] * 6 + [c_float] * 7 + [P] * 7),
    "gsaj_motion_stereo_bytes": (c_int, [c_int] * 4 + [ctypes.POINTER(c_size_t)]),
    "gsaj_debug_motion_stereo_offsets": (c_int, [c_int] * 4 + [ctypes.POINTER(c_size_t)] * 3),
    "gsaj_motion_stereo": (c_int, [c_int, c_int, P, c_size_t, P, c_size_t] + [c_float] * 4 + [P, P, c_float, c_float] + [c_int] * 8 +
                           [P, c_size_t, P, P, P]),
    "gsaj_grey_u8": (c_int, [c_int, c_int, P, P, c_size_t, P]),
}

_lib = None


def build(verbose=False):
    """hipcc --offload-arch=gfx950 build of every kernel file into lib/libgsaj_hip.so."""
    cmd = ["make", "-C", CSRC, "-j8"]
    if not verbose:
        cmd.append("-s")
    subprocess.check_call(cmd)
    return LIB_PATH


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libgsaj_hip.so is missing (%s). Build the HIP extension first: "
            "`python __graft_entry__.py` or `make -C %s`. There is no CPU fallback." % (LIB_PATH, CSRC))
    # PyTorch supplies device memory and streams, so ITS HIP runtime must be the one the process
    # initialises: import it before dlopen()ing the kernels (two runtimes in one process fail with
    # "no ROCm-capable device is detected").
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class GsajError(RuntimeError):
    pass


def check(rc, what):
    """Negative return codes become exceptions carrying gsaj_last_error()."""
    if rc < 0:
        msg = load().gsaj_last_error().decode("utf-8", "replace")
        if rc == -1:
            raise Exception(msg or ("%s: invalid argument" % what))  # reference raises plain Exception for bad combos
        raise GsajError("%s failed (%d): %s" % (what, rc, msg))
    return rc
