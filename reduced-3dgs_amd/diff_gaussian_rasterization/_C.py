"""`diff_gaussian_rasterization._C` -- operator set of the MI355X-native rasterizer.

Same symbols, positional signatures, return tuples and error behaviour as the reference's pybind
module (submodules/diff-gaussian-rasterization/ext.cpp:16-25, rasterize_points.h:18-92), implemented as
thin marshalling over the C ABI of libr3dgs_hip.so (include/r3dgs_rasterizer.h).  PyTorch is plumbing
only here: device memory (outputs + the three opaque state blobs), the current HIP stream, contiguity.

There is NO fallback: if the HIP library is missing or fails to load, importing this module raises.
"""
import ctypes as C
import threading
import weakref
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(os.path.dirname(_HERE), "libr3dgs_hip.so")
if os.environ.get("R3DGS_LIB"):   # A/B builds (tools/build_variant.py): a path, or the tag of libr3dgs_hip_<tag>.so
    _v = os.environ["R3DGS_LIB"]
    _LIB_PATH = _v if os.sep in _v else os.path.join(os.path.dirname(_HERE), f"libr3dgs_hip_{_v}.so")
if not os.path.exists(_LIB_PATH):
    raise ImportError(f"{_LIB_PATH} not found: build it with `python reduced-3dgs_amd/build.py` "
                      "(the rasterizer has no CPU or PyTorch fallback)")
_lib = C.CDLL(_LIB_PATH)

_ALLOC = C.CFUNCTYPE(C.c_void_p, C.c_size_t, C.c_void_p)
_vp, _i, _f, _ll, _sz, _str = C.c_void_p, C.c_int, C.c_float, C.c_longlong, C.c_size_t, C.c_char_p


class _AdamSegment(C.Structure):   # r3dgs_adam_segment (include/r3dgs_optim.h)
    _fields_ = [("param", _vp), ("grad", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp), ("n", _ll),
                ("lerp_weight", _f), ("beta2", _f), ("addcmul_value", _f), ("bc2_sqrt", _f), ("eps", _f), ("step_size", _f)]


class _AdamCapturableSegment(C.Structure):   # r3dgs_adam_capturable_segment (include/r3dgs_optim.h)
    _fields_ = [("param", _vp), ("grad", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp), ("step", _vp), ("lr", _vp),
                ("n", _ll), ("lr_value", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double)]


class _DensifyTensor(C.Structure):   # r3dgs_densify_tensor (include/r3dgs_densify.h); filled by r3dgs_model_state.fill_table
    _fields_ = [("src", _vp), ("dst", _vp), ("row_words", _i), ("kind", _i)]


_McmcTensor = _DensifyTensor   # r3dgs_mcmc_tensor (include/r3dgs_mcmc.h): the same shape, so the same class


# ---- the C ABI of libr3dgs_hip.so, once: {group: (sentence, {name: (restype, [argtypes])})}, a row for every prototype under
# include/ (tests/test_abi_table.py holds names, arity and the kind of every parameter to the headers; the package itself never
# reads them).  "required" is what every build of the library exports; each other group is a family an older A/B build loaded
# through R3DGS_LIB may lack, with the sentence _need(group) then raises ({lib}: the library's path).
_BLOBS_EXACT = [_ALLOC, _vp, _ALLOC, _vp, _ALLOC, _vp]   # three (allocator, user) pairs: geometry, binning, image
_BLOBS_RESERVED = [_vp, _vp, _vp, _i]                    # the three blobs sized up front + the pair reservation
# what a forward takes behind its blobs and its (P, degrees, M[, ragged tables]) head, by colour source:
# background, W, H, the source's arrays .. tan_fovx, tan_fovy, prefiltered, out_color, touched, transmittance, radii, counter
# mode, debug, stream
_FWD_TAIL = [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _f, _f, _i, _vp, _vp, _vp, _vp, _i, _i, _vp]
_FWD_PARAMS_TAIL = [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _f, _f, _i, _vp, _vp, _vp, _vp, _i, _i, _vp]
_FWD_QUANT_TAIL = [_vp, _i, _i, _vp, _i, _vp, _vp, _vp, _f, _vp, _vp, _vp, _f, _f, _i, _vp, _vp, _vp, _vp, _i, _i, _vp]
_NO_SUCH = "the loaded libr3dgs_hip.so has no {}: rebuild it with build.py".format
_NO_FAMILY = "{{lib}} has no {}: rebuild it with build.py".format
_ABI = {
    "required": (None, {
        # include/r3dgs_rasterizer.h
        "r3dgs_version": (_str, []),
        "r3dgs_last_error": (_str, []),
        "r3dgs_geometry_bytes": (_sz, [_i]),
        "r3dgs_geometry_bytes_lean": (_sz, [_i]),
        "r3dgs_binning_bytes": (_sz, [_i, _i, _i, _i]),
        "r3dgs_image_bytes": (_sz, [_i, _i]),
        "r3dgs_binning_capacity": (_i, [_i, _i, _i, _sz]),
        "r3dgs_mark_visible": (_i, [_i, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_forward": (_i, _BLOBS_EXACT + [_i, _vp, _i] + _FWD_TAIL),
        "r3dgs_inference_forward": (_i, _BLOBS_EXACT + [_i, _vp, _i, _vp, _vp, _vp] + _FWD_TAIL),
        "r3dgs_reserve_hint": (_i, [_i, _i, _i]),
        "r3dgs_reserve_hint_view": (_i, [_i, _i, _i, _vp]),
        "r3dgs_forward_reserved": (_ll, _BLOBS_RESERVED + [_i, _vp, _i] + _FWD_TAIL),
        "r3dgs_inference_forward_reserved": (_ll, _BLOBS_RESERVED + [_i, _vp, _i, _vp, _vp, _vp] + _FWD_TAIL),
        "r3dgs_pass_query": (_i, [_ll, _i, _vp, _vp, _vp, _vp]),
        "r3dgs_reserve_overflow_events": (_ll, [_vp, _vp]),
        "r3dgs_pass_pairs": (_i, [_ll, _i]),
        "r3dgs_forward_pairs": (_i, []),
        "r3dgs_set_tight_rects": (_i, [_i]),
        "r3dgs_export_rects": (_i, [_i, _vp, _vp, _vp]),
        "r3dgs_set_tile_order": (_i, [_i]),
        "r3dgs_set_sh_cache": (_i, [_i]),
        "r3dgs_set_f64_chain": (_i, [_i]),
        "r3dgs_forward_hint": (None, [_i]),
        "r3dgs_export_tile_order": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_reserve_forget": (None, []),
        "r3dgs_reserve_forget_view": (None, [_vp]),
        "r3dgs_backward": (_i, [_i, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _f, _f,   # .. tan_fovy
                                _vp, _vp, _vp, _vp, _vp,                             # radii, the three blobs, dL_dpix
                                _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,         # the nine gradients
                                _f, _i, _vp]),
        # absolute screen-space gradients: r3dgs_backward's parameters, then dL_dmean2D_abs, the workspace and its size
        # (rows an older library may lack: _OPTIONAL_ROWS below)
        "r3dgs_absgrad_workspace_floats": (_sz, [_i]),
        "r3dgs_backward_absgrad": (_i, [_i, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _f, _f,
                                        _vp, _vp, _vp, _vp, _vp,
                                        _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                        _f, _i, _vp, _vp, _vp, _sz]),
        "r3dgs_export_binning": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_colour_variance_accumulate": (_i, [_i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_profile_enable": (_i, [_i]),
        "r3dgs_profile_stage_count": (_i, []),
        "r3dgs_profile_stage_name": (_str, [_i]),
        "r3dgs_profile_read": (_i, [_vp, _vp]),
        # include/r3dgs_aux.h
        "r3dgs_aux_maps": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_aux_maps_backward_workspace_bytes": (_sz, [_i, _i, _i, _i]),
        "r3dgs_aux_maps_backward": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp, _f, _vp, _vp, _vp,   # .. radii
                                         _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),   # 3 upstream, 6 outputs
        "r3dgs_aux_maps_backward_screen": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp, _f, _vp, _vp, _vp,
                                                _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,   # 3 upstream, 6 outputs
                                                _vp, _vp, _vp, _vp]),                          # dL_dconic, dL_dz
        # include/r3dgs_distortion.h
        "r3dgs_distortion_map": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp]),
        "r3dgs_distortion_map_backward_workspace_bytes": (_sz, [_i, _i, _i, _i]),
        "r3dgs_distortion_map_backward": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _f, _f, _vp, _vp, _f, _f, _vp, _vp, _f, _vp, _vp,
                                               _vp,                                             # .. radii
                                               _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),   # upstream, moments, 6 outputs
        "r3dgs_distortion_backward_screen": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _f, _f, _vp, _vp, _f, _f, _vp, _vp, _f, _vp, _vp,
                                                  _vp,                                             # .. radii
                                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,          # upstream, moments, 6 outputs
                                                  _vp, _vp, _vp, _vp]),                            # dL_dconic, dL_dz
        # include/r3dgs_features.h
        "r3dgs_feature_maps": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
        "r3dgs_feature_maps_backward_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
        "r3dgs_feature_maps_backward": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp, _f, _vp, _vp, _vp,   # .. radii
                                             _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),   # features .. 7 outputs
        "r3dgs_feature_maps_backward_screen": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp, _f, _vp, _vp,
                                                    _vp,                                           # .. radii
                                                    _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,   # features .. 7 outputs
                                                    _vp, _vp, _vp, _vp]),                          # dL_dconic, dL_dz
        # include/r3dgs_importance.h
        "r3dgs_contribution_scores_workspace_bytes": (_sz, [_i, _i, _i, _i]),
        "r3dgs_contribution_scores": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
        # include/r3dgs_mcmc.h; called by r3dgs_mcmc.py
        "r3dgs_mcmc_workspace_bytes": (_sz, [_i, _i]),
        "r3dgs_mcmc_noise": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _f, _vp]),
        "r3dgs_mcmc_plan": (_i, [_i, _vp, _f, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_mcmc_move": (_i, [_i, _i, _i, _i, _f, _i, C.POINTER(_McmcTensor), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        # include/r3dgs_mip.h; called by r3dgs_mip.py
        "r3dgs_mip_opacity": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _f, _f, _i, _i, _f, _vp, _vp, _vp]),
        "r3dgs_mip_opacity_backward": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _f, _f, _i, _i, _f, _vp,   # .. dL_draw_eff
                                            _vp, _vp, _vp, _vp, _vp, _vp]),                                  # 5 outputs, stream
        "r3dgs_mip_filter3d_workspace_bytes": (_sz, [_i, _i]),
        "r3dgs_mip_filter3d": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_mip_filtered": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_mip_filtered_backward": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        # include/r3dgs_normals.h; called by r3dgs_normals.py
        "r3dgs_gaussian_normals": (_i, [_i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
        "r3dgs_gaussian_normals_backward": (_i, [_i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_depth_normal_workspace_bytes": (_sz, [_i, _i]),
        "r3dgs_depth_normal": (_i, [_i, _i, _f, _f, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
        "r3dgs_depth_normal_backward": (_i, [_i, _i, _f, _f, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
        # include/r3dgs_camera.h
        "r3dgs_camera_backward_workspace_bytes": (_sz, [_i]),
        "r3dgs_camera_backward": (_i, [_i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _i, _vp, _vp, _vp, _f, _f,   # .. tan_fovy
                                       _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),   # radii, blob, 3 sums, 3 outputs
        "r3dgs_camera_backward_maps_workspace_bytes": (_sz, [_i]),
        "r3dgs_camera_backward_maps": (_i, [_i, _i, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _f, _f, _vp,   # .. radii
                                            _vp, _vp, _vp, _vp, _vp, _vp, _vp]),                     # 3 sums, 2 outputs
        # include/r3dgs_reduction.h
        "r3dgs_min_pixel_size": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_sphere_ellipsoid_intersection": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_min_redundancy": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_kmeans_workspace_bytes": (_sz, [_i, _i]),
        "r3dgs_kmeans": (_i, [_i, _i, _vp, _vp, _f, _i, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_knn_max_k": (_i, []),                                    # the knn calls are made by simple_knn/_C.py
        "r3dgs_knn_workspace_bytes": (_sz, [_i]),
        "r3dgs_knn": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_knn_query_workspace_bytes": (_sz, [_i]),
        "r3dgs_knn_query": (_i, [_i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_pack_view_stats": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_reduce_shards": (_i, [_i, _ll, _ll, _ll, _vp, _vp, _vp]),
        # include/r3dgs_loss.h, the loss behind an exposure and a mask; called by r3dgs_exposure.py (rows an older library may
        # lack: _OPTIONAL_ROWS below).  B, C, H, W, img1, img2, exposure, per_image, mask, per_image, mask_target ..
        "r3dgs_exposure_loss_workspace_bytes": (_sz, [_i, _i, _i, _i]),
        "r3dgs_exposure_loss_forward": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _f,   # .. lambda
                                             _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),      # 5 outputs, partials, workspace
        "r3dgs_exposure_loss_backward": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _i,
                                              _vp, _vp, _f, _f, _vp, _vp, _vp, _sz, _vp]),   # partials, grad, coefs, 2 outputs
        "r3dgs_exposure_apply": (_i, [_i, _i, _i, _vp, _vp, _i, _i, _vp, _vp]),
    }),
    "params": (_NO_SUCH("raw-parameter entry points"), {   # raster from the model's raw parameters
        "r3dgs_forward_params": (_i, _BLOBS_EXACT + [_i, _vp, _i] + _FWD_PARAMS_TAIL),
        "r3dgs_forward_params_reserved": (_ll, _BLOBS_RESERVED + [_i, _vp, _i] + _FWD_PARAMS_TAIL),
        "r3dgs_backward_params": (_i, [_i, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _f, _f,   # .. tan_fovy
                                       _vp, _vp, _vp, _vp, _vp,                               # radii, the three blobs, dL_dpix
                                       _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,      # the ten gradients
                                       _f, _i, _vp]),
        "r3dgs_backward_params_absgrad": (_i, [_i, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _f, _f,
                                               _vp, _vp, _vp, _vp, _vp,
                                               _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                               _f, _i, _vp, _vp, _vp, _sz]),
        "r3dgs_activate_params": (_i, [_i, _vp, _vp, _vp, _vp, _vp]),
    }),
    "quantised": (_NO_SUCH("quantised entry points"), {   # include/r3dgs_quantised.h
        "r3dgs_quantised_forward": (_i, _BLOBS_EXACT + [_i, _vp, _i, _vp, _vp, _vp] + _FWD_QUANT_TAIL),
        "r3dgs_quantised_forward_reserved": (_ll, _BLOBS_RESERVED + [_i, _vp, _i, _vp, _vp, _vp] + _FWD_QUANT_TAIL),
        "r3dgs_quantised_decode": (_i, [_i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_quantised_bytes": (_sz, [_i, C.POINTER(_i), _i]),
    }),
    "quantised_grad": (_NO_SUCH("r3dgs_quantised_codebook_grad"), {   # the lookup's adjoint
        "r3dgs_quantised_codebook_grad_workspace_bytes": (_sz, [_i]),
        "r3dgs_quantised_codebook_grad": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    }),
    "reduce_shards_mixed": (_NO_SUCH("r3dgs_reduce_shards_mixed"), {
        "r3dgs_reduce_shards_mixed": (_i, [_i, _ll, _ll, _ll, _ll, _vp, _vp, _vp]),
    }),
    "bwd_segments": (_NO_SUCH("r3dgs_set_bwd_segments"), {
        "r3dgs_set_bwd_segments": (_i, [_i]),
        "r3dgs_bwd_units_cap": (_i, [_i, _i, _i]),
    }),
    "loss": (_NO_FAMILY("fused loss (r3dgs_l1_ssim_forward)"), {   # include/r3dgs_loss.h
        "r3dgs_ssim_window": (None, [_vp]),
        "r3dgs_l1_ssim_workspace_bytes": (_sz, [_i, _i, _i, _i]),
        "r3dgs_l1_ssim_forward": (_i, [_i, _i, _i, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_l1_ssim_backward": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _i, _f, _vp, _vp]),
        "r3dgs_l1_workspace_bytes": (_sz, [_ll]),
        "r3dgs_l1_forward": (_i, [_ll, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_l1_backward": (_i, [_ll, _vp, _vp, _vp, _vp, _vp]),
    }),
    "adam": (_NO_FAMILY("fused Adam (r3dgs_adam_step)"), {   # include/r3dgs_optim.h
        "r3dgs_adam_step": (_i, [_i, C.POINTER(_AdamSegment), _vp]),
        "r3dgs_adam_step_capturable": (_i, [_i, C.POINTER(_AdamCapturableSegment), _vp]),
    }),
    "adam_visible": (_NO_FAMILY("visibility-gated Adam (r3dgs_adam_step_visible)"), {
        "r3dgs_adam_step_visible": (_i, [_i, C.POINTER(_AdamSegment), C.POINTER(_i), _vp, _ll, _vp]),
        "r3dgs_adam_step_capturable_visible": (_i, [_i, C.POINTER(_AdamCapturableSegment), C.POINTER(_i), _vp, _ll, _vp]),
    }),
    "train_stats": (_NO_FAMILY("training statistics (r3dgs_visible_means)"), {   # include/r3dgs_trainstats.h
        "r3dgs_train_stats_workspace_bytes": (_sz, [_i]),
        "r3dgs_visible_means": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_alpha_regul_backward": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_densification_stats": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp]),
    }),
    "metrics": (_NO_FAMILY("evaluation metrics (r3dgs_image_metrics)"), {   # include/r3dgs_metrics.h
        "r3dgs_image_metrics_workspace_bytes": (_sz, [_i, _i, _i]),
        "r3dgs_image_metrics": (_i, [_i, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp]),
        "r3dgs_row_mse_workspace_bytes": (_sz, [_ll, _ll]),
        "r3dgs_row_mse": (_i, [_ll, _ll, _vp, _vp, _vp, _vp, _vp]),
        "r3dgs_image_to_uint8": (_i, [_i, _i, _i, _vp, _vp, _vp]),
    }),
    "densify": (_NO_FAMILY("densification (r3dgs_densify_plan)"), {   # include/r3dgs_densify.h; called by r3dgs_densify.py
        "r3dgs_densify_workspace_bytes": (_sz, [_i]),
        "r3dgs_densify_plan": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _i, _f, _f, _vp, _vp, _vp]),
        "r3dgs_prune_plan": (_i, [_i, _vp, _vp, _vp, _vp]),
        "r3dgs_densify_move": (_i, [_i, _i, _i, _i, _i, C.POINTER(_DensifyTensor), _vp, _vp, _vp, _vp, _vp, _vp]),
    }),
}


# Rows that joined a group after libraries with that group were built: a library without them still has the group, and the calls
# that want them say so (_need_rows).  {family: (sentence, names)}
_OPTIONAL_ROWS = {
    "absgrad": (_NO_SUCH("absolute-gradient entry points (r3dgs_backward_absgrad)"),
                ("r3dgs_absgrad_workspace_floats", "r3dgs_backward_absgrad", "r3dgs_backward_params_absgrad")),
    "exposure": (_NO_SUCH("exposure loss entry points (r3dgs_exposure_loss_forward)"),
                 ("r3dgs_exposure_loss_workspace_bytes", "r3dgs_exposure_loss_forward", "r3dgs_exposure_loss_backward",
                  "r3dgs_exposure_apply")),
}


def _apply_abi(lib):
    """Sets restype / argtypes of every row on `lib` -> the set of groups it has.  An optional group is there when the library
    exports all of its names; a name of the required group that is missing raises AttributeError.  Names of _OPTIONAL_ROWS do
    not count for either: the ones `lib` lacks are skipped."""
    later = {name for _, names in _OPTIONAL_ROWS.values() for name in names}
    present = set()
    for group, (_, rows) in _ABI.items():
        if group != "required" and not all(hasattr(lib, name) for name in rows if name not in later):
            continue
        present.add(group)
        for name, (restype, argtypes) in rows.items():
            if name in later and not hasattr(lib, name):
                continue
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return present


_present = _apply_abi(_lib)
# names of _OPTIONAL_ROWS the loaded library lacks
_missing_rows = {name for _, names in _OPTIONAL_ROWS.values() for name in names if not hasattr(_lib, name)}


def _need(group, error=RuntimeError):
    if group not in _present:
        raise error(_ABI[group][0].format(lib=_LIB_PATH))


def _need_rows(family, error=RuntimeError):
    sentence, names = _OPTIONAL_ROWS[family]
    if any(name in _missing_rows for name in names):
        raise error(sentence)


def has_absgrad():
    """Whether the loaded library has the absolute-gradient backward (r3dgs_backward_absgrad)."""
    return not any(name in _missing_rows for name in _OPTIONAL_ROWS["absgrad"][1])


LIBRARY_PATH = _LIB_PATH

# ---- compiled torch binding of the hot calls (csrc_torch/r3dgs_torch.cpp; the reference's layer is a torch C++ extension
# too, DGR/ext.cpp:16-25).  It names the entry points it wants (entry_points()) and is handed their addresses in the library
# loaded above, so both bindings drive ONE library instance; an optional one whose group the library lacks is left out.
# R3DGS_BINDING = auto (default: compiled if it was built, else ctypes) | torch (required) | ctypes.
_ext = None
_ext_loaded = None
_binding_request = os.environ.get("R3DGS_BINDING", "auto")
if _binding_request not in ("auto", "torch", "ctypes"):
    raise ImportError(f"R3DGS_BINDING={_binding_request!r}: expected auto, torch or ctypes")
if _binding_request != "ctypes":
    try:
        from . import _r3dgs_torch as _ext_loaded
        _rows = {name for group in _present for name in _ABI[group][1]}
        _ext_loaded.bind({name: C.cast(getattr(_lib, name), _vp).value for name, _ in _ext_loaded.entry_points() if name in _rows and name not in _missing_rows})
        _ext = _ext_loaded
    except ImportError:
        if _binding_request == "torch":
            raise
        _ext_loaded = None


def binding():
    """'torch': rasterize_gaussians / rasterize_gaussians_backward / mark_visible go through the compiled torch extension
    (diff_gaussian_rasterization/_r3dgs_torch.so); 'ctypes': through this module's ctypes marshalling.  Same library, same
    kernels, same results bit for bit (tests/test_gpu_parity.py runs both)."""
    return "torch" if _ext is not None else "ctypes"


def set_binding(name):
    """'torch' | 'ctypes' -> the previous setting.  'torch' needs the extension to have been built (build.py)."""
    global _ext
    before = binding()
    if name == "torch":
        if _ext_loaded is None:
            raise RuntimeError("the compiled torch binding is not built (reduced-3dgs_amd/build.py) or R3DGS_BINDING=ctypes")
        _ext = _ext_loaded
    elif name == "ctypes":
        _ext = None
    else:
        raise ValueError(name)
    return before


_NO_TENSOR = torch.Tensor([])


def _t(x):
    return _NO_TENSOR if x is None else x



def profile_enable(on, only=None):
    """Per-stage HIP-event timing inside the library (include/r3dgs_rasterizer.h r3dgs_profile_*).
    only: iterable of stage names to time alone (every event record is a packet on the stream)."""
    if on and only:
        n = _lib.r3dgs_profile_stage_count()
        names = [_lib.r3dgs_profile_stage_name(k).decode() for k in range(n)]
        code = 0
        for name in only:
            code |= 1 << (names.index(name) + 1)
        _lib.r3dgs_profile_enable(code)
    else:
        _lib.r3dgs_profile_enable(int(bool(on)))


def profile_read():
    """-> {stage_name: (total_ms, launches)} since the last read; waits for the recorded events."""
    n = _lib.r3dgs_profile_stage_count()
    ms = (C.c_double * n)()
    cnt = (C.c_int * n)()
    _check(_lib.r3dgs_profile_read(ms, cnt), "profile_read")
    return {_lib.r3dgs_profile_stage_name(k).decode(): (ms[k], cnt[k]) for k in range(n)}


def version():
    return _lib.r3dgs_version().decode()


def _check(status, what):
    if status < 0:
        raise RuntimeError(f"{what}: {_lib.r3dgs_last_error().decode()}")
    return status


def _ptr(t):
    """Device pointer of a tensor, or NULL for an absent optional input (empty tensor, as the reference's
    wrapper passes `torch.Tensor([])` for missing arguments, diff_gaussian_rasterization/__init__.py:209-218)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


def _dev(t, dev, dtype=torch.float32):
    """An input as the library reads it: on `dev`, of `dtype`, contiguous (copied if it is not); None for an absent one."""
    if t is None or t.numel() == 0:
        return None
    if t.device != dev:
        raise RuntimeError(f"expected a tensor on {dev}, got {t.device}")
    if t.dtype != dtype:
        raise RuntimeError(f"expected {str(dtype)[6:]}, got {t.dtype}")
    return t.contiguous()


class _Blob:
    """One caller-owned, resizable byte buffer (resizeFunctional of rasterize_points.cu:33-41)."""

    def __init__(self, dev):
        self.dev = dev
        self.tensor = torch.empty(0, dtype=torch.uint8, device=dev)
        self.error = None

        def alloc(nbytes, _user):
            try:
                self.tensor = torch.empty(int(nbytes), dtype=torch.uint8, device=self.dev)
                return self.tensor.data_ptr()
            except Exception as e:  # an exception cannot cross the C frame: keep it, hand back NULL
                self.error = e
                return None

        self.cb = _ALLOC(alloc)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _on_device:
    """`with torch.cuda.device(dev)` only when dev is not already current (the context manager costs ~10 us)."""

    __slots__ = ("ctx",)

    def __init__(self, dev):
        self.ctx = None if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


class NumRendered:
    """The `num_rendered` slot of the forward's return tuple (rasterize_points.cu:221), with the reference's meaning:
    the sum over the visible Gaussians of the tile count of their 3-sigma squares.  The asynchronous forward does not
    wait for the number: it lives on the device, and this object fetches it the first time someone looks (int(),
    index, comparison, print) -- the training loop never does, it only hands the object back to
    rasterize_gaussians_backward.  `.capacity` is the pair capacity the binning buffer was sized with, `.pairs` the
    (tile, Gaussian) pairs the pass binned (<= num_rendered: opacity-aware rects leave out tiles a Gaussian cannot
    reach; equal with set_tight_rects(False))."""

    __slots__ = ("ticket", "capacity", "_value", "_flags", "_pairs")

    def __init__(self, ticket, capacity, value=None, pairs=None):
        self.ticket, self.capacity, self._value, self._flags, self._pairs = ticket, capacity, value, 0, pairs

    def _resolve(self, wait=True):
        if self._value is None:
            r, v, cap, fl = _i(), _i(), _i(), _i()
            st = _check(_lib.r3dgs_pass_query(self.ticket, int(wait), C.byref(r), C.byref(v), C.byref(cap),
                                              C.byref(fl)), "num_rendered")
            if st == 1:
                self._value, self._flags = r.value, fl.value
        return self._value

    @property
    def pairs(self):
        if self._pairs is None:
            self._pairs = _check(_lib.r3dgs_pass_pairs(self.ticket, 1), "pairs")
        return self._pairs

    @property
    def truncated(self):
        """True if num_rendered exceeded the reservation of this pass (the farthest pairs were dropped)."""
        self._resolve()
        return bool(self._flags & 1)

    def ready(self):
        return self._resolve(wait=False) is not None

    def __int__(self):
        return self._resolve()

    __index__ = __int__

    def __float__(self):
        return float(self._resolve())

    def __eq__(self, other):
        return int(self) == other

    def __lt__(self, other):
        return int(self) < other

    def __le__(self, other):
        return int(self) <= other

    def __gt__(self, other):
        return int(self) > other

    def __ge__(self, other):
        return int(self) >= other

    def __hash__(self):
        return hash(int(self))

    def __bool__(self):
        return int(self) != 0

    def __repr__(self):
        return str(int(self))


_size_cache = {}


def _blob_bytes(kind, *key):
    k = (kind,) + key
    v = _size_cache.get(k)
    if v is None:
        if kind == "geom":
            v = _lib.r3dgs_geometry_bytes(*key)
        elif kind == "geom_lean":
            v = _lib.r3dgs_geometry_bytes_lean(*key)
        elif kind == "bin":
            v = _lib.r3dgs_binning_bytes(*key)
        else:
            v = _lib.r3dgs_image_bytes(*key)
        if v == 0:
            raise RuntimeError(f"rasterize_gaussians: {_lib.r3dgs_last_error().decode()}")
        if len(_size_cache) > 4096:
            _size_cache.clear()
        _size_cache[k] = v
    return v


# ---- strict mode (the default) -------------------------------------------------------------------------------------
# The asynchronous forward runs on a pair RESERVATION.  The reference never drops a pair (it sizes its buffer from the
# exact count, rasterizer_impl.cu:441-450), so a pass whose pair count exceeded its reservation must not reach a
# consumer: in strict mode the forward looks at the pass's published numbers before it returns -- they appear ~40 us
# into the pass, long before it ends, so the GPU keeps working on the rest of the pass while the host goes on -- and a
# truncated pass is redone on the exact-size path (same stream, same output tensors: the redo overwrites them in
# stream order).  What the caller gets is therefore always the exact result; the reservation only decides how often a
# redo happens.  R3DGS_STRICT=0 / set_strict(False) selects the old fire-and-forget behaviour (a RuntimeWarning after
# the fact), for host-side A/B measurements only.
_strict = os.environ.get("R3DGS_STRICT", "1") != "0"
_stats = {"reserved_passes": 0, "exact_passes": 0, "redone_passes": 0}
_overflow_seen = 0
_calls = 0


def set_strict(on):
    """True (default): a pass that overflowed its pair reservation is detected before its outputs are returned and
    redone on the exact-size path.  False: nothing waits; such a pass drops its farthest pairs and only warns."""
    global _strict
    _strict = bool(on)


def is_strict():
    return _strict


def pass_stats():
    """{reserved_passes, exact_passes, redone_passes, overflow_events}: how the forwards of this process were issued."""
    d = dict(_stats)
    d["overflow_events"] = reserve_overflow_events()
    return d


def reserve_forget():
    """Forget the pair counts learnt so far (new scene; tests): the next pass of each image size is an exact-size one."""
    _lib.r3dgs_reserve_forget()


def reserve_overflow_events():
    """Passes whose pair count exceeded their reservation so far (strict mode redid them; the reservation grows)."""
    return int(_lib.r3dgs_reserve_overflow_events(None, None))


def _watch_overflow():
    global _overflow_seen, _calls
    _calls += 1
    if _calls & 15:
        return
    r, cap = _i(), _i()
    n = int(_lib.r3dgs_reserve_overflow_events(C.byref(r), C.byref(cap)))
    if n > _overflow_seen:
        _overflow_seen = n
        import warnings
        warnings.warn(f"diff_gaussian_rasterization (strict mode OFF): a pass needed {r.value} (tile, Gaussian) pairs but "
                      f"{cap.value} were reserved; its farthest pairs were dropped and the reservation has been raised",
                      RuntimeWarning)


_tracked_views = {}   # device address of a view matrix -> weakref of the tensor that owns it


def _track_view(vm):
    """The library remembers pair counts per camera under the device address of its view matrix.  When that tensor dies
    the address may be handed to another camera: tell the library to forget it.  Every scene/cameras.py Camera
    owns its matrix for the whole run, so this registers once per camera; a matrix that is a temporary (uploaded per
    iteration, a converted copy) is forgotten as soon as it is freed and its passes use the image size's largest recent
    count instead."""
    ptr = vm.data_ptr()
    ref = _tracked_views.get(ptr)
    if ref is not None and ref() is vm:
        return
    if len(_tracked_views) > 65536:
        _tracked_views.clear()
    _tracked_views[ptr] = weakref.ref(vm)
    weakref.finalize(vm, _forget_view, ptr, id(vm))


def _forget_view(ptr, ident):
    ref = _tracked_views.get(ptr)
    if ref is not None and ref() is not None:
        # a live tensor has registered this address since (a fresh wrapper over the same storage every iteration --
        # stacked[i], .view() -- dies while its successor is in use): the camera's learnt pair count stays
        return
    if ref is not None:
        del _tracked_views[ptr]
    try:
        _lib.r3dgs_reserve_forget_view(ptr)
    except Exception:   # interpreter shutdown
        pass


def _forward_prologue(P, dev, H, W, strict_override):
    """What every forward wrapper does once its arguments are checked -> (empty, trains, strict).  empty: the result for
    P == 0 (a black image, nothing rendered, empty state), else None; trains: what hint_next_forward said about this forward
    (one-shot, per thread like the library's own r3dgs_forward_hint state), or whether gradients are enabled; strict: the
    module's mode, or the caller's override."""
    if P == 0:
        e = torch.empty(0, dtype=torch.uint8, device=dev)
        return (NumRendered(0, 0, 0, 0), torch.zeros((3, H, W), dtype=torch.float32, device=dev),
                torch.zeros((0,), dtype=torch.int32, device=dev), e, e.clone(), e.clone()), False, False
    hint = getattr(_tls, "next_forward_trains", None)
    _tls.next_forward_trains = None
    return (None, torch.is_grad_enabled() if hint is None else hint,
            _strict if strict_override is None else bool(strict_override))


def _zero_grads(dev, *shapes):
    """A backward's result for P == 0: zeros of the given shapes."""
    return tuple(torch.zeros(s, dtype=torch.float32, device=dev) for s in shapes)


def _pair_capacity(R, P, W, H, binningBuffer):
    """The pair capacity the forward carved the binning blob with: R says (a NumRendered), or -- R a plain int from an older
    caller -- what the blob's size implies."""
    if isinstance(R, NumRendered):
        return R.capacity
    return _lib.r3dgs_binning_capacity(P, W, H, int(binningBuffer.numel())) if binningBuffer.numel() else 0


def _seen(*result):
    """A non-empty forward's six-tuple on its way out: kept for the thread's forward_state recorder, if one is open."""
    rec = getattr(_tls, "forward_recorder", None)
    if rec is not None:
        rec.result = result
    return result


def _reserved_result(strict, ticket, reserve, rendered, flags, out_color, radii, geom, binning, img):
    """A pass issued on a reservation (either binding; rendered < 0: not fetched yet) -> the forward's six-tuple, or None:
    strict mode found the pass truncated and the caller redoes it on the exact-size path."""
    nr = NumRendered(ticket, reserve, rendered if rendered >= 0 else None)
    nr._flags = flags
    _stats["reserved_passes"] += 1
    if not strict:
        _watch_overflow()
        return _seen(nr, out_color, radii, geom, binning, img)
    if not nr.truncated:   # waits for the pass's header (not for the pass)
        return _seen(nr, out_color, radii, geom, binning, img)
    _stats["redone_passes"] += 1
    return None


def _exact_result(rendered, out_color, radii, geom, binning, img):
    """An exact-size pass -> the forward's six-tuple."""
    _stats["exact_passes"] += 1
    pairs = int(_lib.r3dgs_forward_pairs())   # pairs actually binned (<= num_rendered, what the blob was carved for)
    return _seen(NumRendered(0, max(int(rendered), 1), rendered, pairs), out_color, radii, geom, binning, img)


def _drive_forward(fn_exact, fn_reserved, args, what, dev, P, W, H, vm_ptr, lean, counters, out_color, radii, exact, debug,
                   _reserve, strict):
    """The ctypes forward of every source, called with `dev` current: `args` is what the source's two entry points take
    behind the blobs (the pointers of out_color, radii and the counters among them), `what` names the caller in errors.
    Asynchronous path: blobs sized up front from a pair reservation, one graph launch, no wait for the pass.  The
    exact-size path (allocator callbacks, one wait in the middle) runs when nothing is known about this view size yet, in
    debug mode, when asked for -- and to redo a pass that overflowed its reservation (strict mode)."""
    reserve = 0 if (exact or debug) else _lib.r3dgs_reserve_hint_view(P, W, H, vm_ptr)
    if _reserve is not None:   # tests: a chosen reservation
        reserve = int(_reserve)
    if reserve > 0:
        u8 = dict(dtype=torch.uint8, device=dev)
        geom = torch.empty(_blob_bytes("geom_lean" if lean else "geom", P), **u8)
        binning = torch.empty(_blob_bytes("bin", P, W, H, reserve), **u8)
        img = torch.empty(_blob_bytes("img", W, H), **u8)
        ticket = fn_reserved(geom.data_ptr(), binning.data_ptr(), img.data_ptr(), reserve, *args)
        if ticket < 0:
            _check(-1, what)
        out = _reserved_result(strict, ticket, reserve, -1, 0, out_color, radii, geom, binning, img)
        if out is not None:
            return out
        if counters is not None:   # the redo below: counter mode accumulates into its outputs
            counters[0].zero_()
            counters[1].zero_()
        del geom, binning, img
    geom, binning, img = _Blob(dev), _Blob(dev), _Blob(dev)
    rendered = fn_exact(geom.cb, None, binning.cb, None, img.cb, None, *args)
    for blob in (geom, binning, img):
        if blob.error is not None:   # e.g. torch OOM inside the allocator callback: surface the original exception
            raise blob.error
    _check(rendered, what)
    return _exact_result(rendered, out_color, radii, geom.tensor, binning.tensor, img.tensor)


def _forward_common(ragged, background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                    viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degrees, campos,
                    prefiltered, debug, counters=None, exact=False, _reserve=None, _strict_override=None):
    if means3D.dim() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")  # rasterize_points.cu:158-161
    dev = means3D.device
    if dev.type != "cuda":
        raise RuntimeError("the MI355X rasterizer needs device tensors (no CPU path)")
    P, H, W = int(means3D.size(0)), int(image_height), int(image_width)
    empty, trains, strict = _forward_prologue(P, dev, H, W, _strict_override)
    if empty is not None:
        return empty
    if _ext is not None and ragged is None and counters is None and not exact and not debug and _reserve is None:
        # the hot call: compiled marshalling (csrc_torch/r3dgs_torch.cpp), same library entry points as below
        if viewmatrix is not None and viewmatrix.is_contiguous() and viewmatrix.dtype == torch.float32:
            _track_view(viewmatrix)
        res = _ext.forward_reserved(
            _t(background), means3D, _t(colors), _t(opacity), _t(scales), _t(rotations), float(scale_modifier),
            _t(cov3D_precomp), _t(viewmatrix), _t(projmatrix), float(tan_fovx), float(tan_fovy), H, W, _t(sh), _t(degrees),
            _t(campos), bool(prefiltered), bool(trains), strict)
        if res[0]:
            out = _reserved_result(strict, *res)
            if out is not None:
                return out
        del res        # the reservation did not hold, or ticket == 0 (nothing known about this view size yet):
        exact = True   # the exact-size path below
    out_color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    radii = torch.empty((P,), dtype=torch.int32, device=dev)
    bg = _dev(background, dev)
    m3, col, op = _dev(means3D, dev), _dev(colors, dev), _dev(opacity, dev)
    sc, rot, cov = _dev(scales, dev), _dev(rotations, dev), _dev(cov3D_precomp, dev)
    vm, pm, cp = _dev(viewmatrix, dev), _dev(projmatrix, dev), _dev(campos, dev)
    shc, deg = _dev(sh, dev), _dev(degrees, dev, torch.int32)
    touched = transm = None
    if counters is not None:
        touched, transm = counters
    _lib.r3dgs_forward_hint(int(trains))   # holds for the redo of an overflowed pass as well
    with _on_device(dev):
        tail = (_ptr(bg), W, H, _ptr(m3), _ptr(shc), _ptr(col), _ptr(op), _ptr(sc), float(scale_modifier), _ptr(rot),
                _ptr(cov), _ptr(vm), _ptr(pm), _ptr(cp), float(tan_fovx), float(tan_fovy), int(bool(prefiltered)),
                _ptr(out_color), _ptr(touched), _ptr(transm), _ptr(radii), int(counters is not None),
                int(bool(debug)), _stream())
        if ragged is None:
            head = (P, _ptr(deg), int(shc.size(1)) if shc is not None else 0)
            fn_exact, fn_reserved = _lib.r3dgs_forward, _lib.r3dgs_forward_reserved
        else:
            coeffs, perband, cumsum = (_dev(t, dev, torch.int32) for t in ragged)
            head = (P, _ptr(deg), int(perband.numel()) if perband is not None else 0, _ptr(coeffs), _ptr(perband),
                    _ptr(cumsum))
            fn_exact, fn_reserved = _lib.r3dgs_inference_forward, _lib.r3dgs_inference_forward_reserved
        if vm is not None:
            _track_view(vm)
        # no SH direction derivatives will be left (render-only / ragged SH / precomputed colours): the lean blob
        lean = not trains or ragged is not None or shc is None or col is not None
        return _drive_forward(fn_exact, fn_reserved, head + tail, "rasterize_gaussians", dev, P, W, H, _ptr(vm), lean,
                              counters, out_color, radii, exact, debug, _reserve, strict)


def rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                        viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degrees, campos,
                        prefiltered, debug):
    """RasterizeGaussiansCUDA (rasterize_points.cu:136-222) ->
    (num_rendered, out_color[3,H,W], radii[P], geomBuffer, binningBuffer, imgBuffer).
    num_rendered is a NumRendered: an int-like that is only fetched from the device when looked at."""
    return _forward_common(None, background, means3D, colors, opacity, scales, rotations, scale_modifier,
                           cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh,
                           degrees, campos, prefiltered, debug)


def rasterize_gaussians_variableSH_bands(background, means3D, colors, opacity, scales, rotations, scale_modifier,
                                         cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height,
                                         image_width, sh, perBandPrimitiveCount, cumSumPrimitiveCount, coeffsNum,
                                         degrees, campos, prefiltered, debug):
    """RasterizeGaussiansVariableSHBandsCUDA (rasterize_points.cu:43-134): inference-only forward over the
    ragged, degree-sorted SH buffer."""
    return _forward_common((coeffsNum, perBandPrimitiveCount, cumSumPrimitiveCount), background, means3D, colors,
                           opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
                           tan_fovx, tan_fovy, image_height, image_width, sh, degrees, campos, prefiltered, debug)


_grad_arena = None


def set_gradient_arena(fn):
    """Extension for multi-GPU training (not in the reference): `fn(name, shape) -> float32 CUDA tensor or None`
    supplies the storage of the backward's outputs (names: means2D, colors, opacity, means3D, cov3D, sh, scales,
    rotations).  A view-parallel trainer hands out views of its flat all-reduce buffer, so the gradients are born
    inside it and no packing copy is needed (multiview.ViewParallelExchange.arena).  None restores torch.empty."""
    global _grad_arena
    _grad_arena = fn


def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier,
                                 cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh,
                                 degrees, campos, geomBuffer, R, binningBuffer, imageBuffer, lambda_sh_sparsity,
                                 debug, _want_conic=False, _absgrad=False):
    """RasterizeGaussiansBackwardCUDA (rasterize_points.cu:224-305) -> (dL_dmeans2D[P,3], dL_dcolors[P,3],
    dL_dopacity[P,1], dL_dmeans3D[P,3], dL_dcov3D[P,6], dL_dsh[P,M,3], dL_dscales[P,3], dL_drotations[P,4]).
    _absgrad: + dL_dmeans2D_abs[P,3] as the LAST element (include/r3dgs_rasterizer.h r3dgs_backward_absgrad): the per-pixel
    absolute values of what dL_dmeans2D sums, third column zero; the other outputs are the plain call's bit for bit."""
    if _absgrad:
        _need_rows("absgrad")
    dev = means3D.device
    P = int(means3D.size(0))
    H, W = int(dL_dout_color.size(1)), int(dL_dout_color.size(2))
    M = int(sh.size(1)) if (sh is not None and sh.numel() != 0) else 0
    opts = dict(dtype=torch.float32, device=dev)
    if P == 0:
        return _zero_grads(dev, (0, 3), (0, 3), (0, 1), (0, 3), (0, 6), (0, M, 3), (0, 3), (0, 4)) + (
            _zero_grads(dev, (0, 3)) if _absgrad else ())
    if _ext is not None and _grad_arena is None:
        cap = _pair_capacity(R, P, W, H, binningBuffer)
        return tuple((_ext.backward_absgrad if _absgrad else _ext.backward)(_t(background), means3D, _t(radii), _t(colors), _t(scales), _t(rotations),
                                   float(scale_modifier), _t(cov3D_precomp), _t(viewmatrix), _t(projmatrix), float(tan_fovx),
                                   float(tan_fovy), dL_dout_color, _t(sh), _t(degrees), _t(campos), geomBuffer, int(cap),
                                   binningBuffer, imageBuffer, float(lambda_sh_sparsity), bool(debug), bool(_want_conic)))

    def e(name, *s):  # every element is written by the library
        if _grad_arena is not None:
            t = _grad_arena(name, s)
            if t is not None:
                if tuple(t.shape) != s or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
                    raise RuntimeError(f"gradient arena returned an unusable tensor for {name}")
                return t
        return torch.empty(s, **opts)
    dL_dmeans3D, dL_dmeans2D = e("means3D", P, 3), e("means2D", P, 3)
    dL_dcolors, dL_dopacity = e("colors", P, 3), e("opacity", P, 1)
    dL_dcov3D, dL_dsh, dL_dscales, dL_drotations = e("cov3D", P, 6), e("sh", P, M, 3), e("scales", P, 3), e("rotations", P, 4)
    dL_dconic = torch.empty((P, 2, 2), **opts) if _want_conic else None
    bg, m3 = _dev(background, dev), _dev(means3D, dev)
    col, sc, rot, cov = (_dev(t, dev) for t in (colors, scales, rotations, cov3D_precomp))
    vm, pm, cp = _dev(viewmatrix, dev), _dev(projmatrix, dev), _dev(campos, dev)
    g, shc = _dev(dL_dout_color, dev), _dev(sh, dev)
    deg, rad = _dev(degrees, dev, torch.int32), _dev(radii, dev, torch.int32)
    cap = _pair_capacity(R, P, W, H, binningBuffer)
    abs_out, abs_tail = _absgrad_tail(_absgrad, P, cap, opts)
    with _on_device(dev):
        st = (_lib.r3dgs_backward_absgrad if _absgrad else _lib.r3dgs_backward)(
            P, _ptr(deg), M, int(cap), _ptr(bg), W, H, _ptr(m3), _ptr(shc), _ptr(col), _ptr(sc),
            float(scale_modifier), _ptr(rot), _ptr(cov), _ptr(vm), _ptr(pm), _ptr(cp),
            float(tan_fovx), float(tan_fovy), _ptr(rad), _ptr(geomBuffer), _ptr(binningBuffer),
            _ptr(imageBuffer), _ptr(g), _ptr(dL_dmeans2D), _ptr(dL_dconic), _ptr(dL_dopacity),
            _ptr(dL_dcolors), _ptr(dL_dmeans3D), _ptr(dL_dcov3D), _ptr(dL_dsh), _ptr(dL_dscales),
            _ptr(dL_drotations), float(lambda_sh_sparsity), int(bool(debug)), _stream(), *abs_tail)
    _check(st, "rasterize_gaussians_backward")
    out = (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations)
    out = out + (dL_dconic,) if _want_conic else out
    return out + (abs_out,) if _absgrad else out


def _absgrad_tail(absgrad, P, cap, opts):
    """-> (dL_dmeans2D_abs or None, the three trailing arguments of the *_absgrad entry points or ()).  The workspace is the
    call's own: its contents mean nothing before or after."""
    if not absgrad:
        return None, ()
    out = torch.empty((P, 3), **opts)
    n = int(_lib.r3dgs_absgrad_workspace_floats(int(cap)))
    ws = torch.empty((n,), **opts)
    return out, (out.data_ptr(), ws.data_ptr(), n)


# ---- raster from the model's raw parameters (include/r3dgs_rasterizer.h r3dgs_*_params) ---------------------------------
# The tensors travel as GaussianModel stores them: _xyz, _features_dc [P,1,3], _features_rest [P,M-1,3], _opacity, _scaling
# (log), _rotation (unnormalised).  The kernels apply the activations; the backward returns gradients of exactly these
# tensors, each written whole by the library into storage of the leaf's own shape -- no cat, narrow or copy on either side.
# A tensor that would need a copy (not contiguous, not float32) is refused instead of converted.

def _param(t, dev, name):
    if t.device != dev:
        raise RuntimeError(f"{name}: expected a tensor on {dev}, got {t.device}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: the raw-parameter path needs float32, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: the raw-parameter path needs a contiguous tensor")
    return t


def _check_params(xyz, features_dc, features_rest, opacity, scaling, rotation, degrees):
    """-> (P, M, device); the refusals of the raw-parameter path (same messages as csrc_torch/r3dgs_torch.cpp)."""
    if xyz.dim() != 2 or xyz.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    dev = xyz.device
    if dev.type != "cuda":
        raise RuntimeError("the MI355X rasterizer needs device tensors (no CPU path)")
    P = int(xyz.size(0))
    if features_dc.dim() != 3 or tuple(features_dc.shape) != (P, 1, 3):
        raise RuntimeError("features_dc must have dimensions (num_points, 1, 3)")
    no_rest = features_rest is None or features_rest.numel() == 0
    if not no_rest and (features_rest.dim() != 3 or features_rest.size(0) != P or features_rest.size(2) != 3):
        raise RuntimeError("features_rest must have dimensions (num_points, M-1, 3)")
    M = 1 if no_rest else 1 + int(features_rest.size(1))
    if M > 16:
        raise RuntimeError("features_rest must have dimensions (num_points, M-1, 3) with M <= 16")
    if tuple(scaling.shape) != (P, 3):
        raise RuntimeError("scaling must have dimensions (num_points, 3)")
    if tuple(rotation.shape) != (P, 4):
        raise RuntimeError("rotation must have dimensions (num_points, 4)")
    if opacity.numel() != P:
        raise RuntimeError("opacity must have dimensions (num_points, 1)")
    if degrees.numel() != P:
        raise RuntimeError("degrees must have one entry per point")
    for t, name in ((xyz, "means3D"), (features_dc, "features_dc"), (opacity, "opacity"), (scaling, "scaling"),
                    (rotation, "rotation")) + (() if no_rest else ((features_rest, "features_rest"),)):
        _param(t, dev, name)
    return P, M, dev


def rasterize_gaussian_params(background, xyz, features_dc, features_rest, degrees, opacity, scaling, rotation,
                              scale_modifier, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, campos,
                              prefiltered, debug, exact=False, _reserve=None, _strict_override=None):
    """rasterize_gaussians from the model's raw parameters -> (num_rendered, out_color[3,H,W], radii[P], geomBuffer,
    binningBuffer, imgBuffer); same asynchronous / exact-size / strict-mode behaviour."""
    _need("params")
    P, M, dev = _check_params(xyz, features_dc, features_rest, opacity, scaling, rotation, degrees)
    H, W = int(image_height), int(image_width)
    empty, trains, strict = _forward_prologue(P, dev, H, W, _strict_override)
    if empty is not None:
        return empty
    rest = _NO_TENSOR if M == 1 else features_rest
    if viewmatrix is not None and viewmatrix.is_contiguous() and viewmatrix.dtype == torch.float32:
        _track_view(viewmatrix)
    if _ext is not None:
        common = (_t(background), xyz, features_dc, rest, degrees, opacity, scaling, rotation, float(scale_modifier),
                  _t(viewmatrix), _t(projmatrix), float(tan_fovx), float(tan_fovy), H, W, _t(campos), bool(prefiltered), bool(trains))
        if not exact and not debug:
            res = _ext.forward_params_reserved(*common, strict, int(_reserve or 0))
            if res[0]:
                out = _reserved_result(strict, *res)
                if out is not None:
                    return out
            del res
        return _exact_result(*_ext.forward_params(*common, bool(debug)))
    out_color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    radii = torch.empty((P,), dtype=torch.int32, device=dev)
    bg, vm, pm, cp = (_dev(t, dev) for t in (background, viewmatrix, projmatrix, campos))
    deg = _dev(degrees, dev, torch.int32)
    _lib.r3dgs_forward_hint(int(trains))
    with _on_device(dev):
        args = (P, _ptr(deg), M, _ptr(bg), W, H, _ptr(xyz), _ptr(features_dc), _ptr(rest), _ptr(opacity), _ptr(scaling),
                float(scale_modifier), _ptr(rotation), _ptr(vm), _ptr(pm), _ptr(cp), float(tan_fovx), float(tan_fovy),
                int(bool(prefiltered)), _ptr(out_color), None, None, _ptr(radii), 0, int(bool(debug)), _stream())
        return _drive_forward(_lib.r3dgs_forward_params, _lib.r3dgs_forward_params_reserved, args, "rasterize_gaussian_params",
                              dev, P, W, H, _ptr(vm), not trains, None, out_color, radii, exact, debug, _reserve, strict)


def rasterize_gaussian_params_backward(background, xyz, radii, features_dc, features_rest, degrees, opacity, scaling, rotation,
                                       scale_modifier, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, campos,
                                       geomBuffer, R, binningBuffer, imageBuffer, lambda_sh_sparsity, debug, _want_2d=False,
                                       _absgrad=False):
    """-> (dL_dmeans2D[P,3], dL_dopacity[P,1], dL_dxyz[P,3], dL_dfeatures_dc[P,1,3], dL_dfeatures_rest[P,M-1,3],
    dL_dscaling[P,3], dL_drotation[P,4]): gradients of the tensors passed in (raw scaling / rotation included).
    _want_2d: + (dL_dcolors[P,3], dL_dconic[P,2,2]), the per-Gaussian sums camera_backward reads (the ctypes marshalling).
    _absgrad: + dL_dmeans2D_abs[P,3] as the LAST element, as rasterize_gaussians_backward."""
    _need("params")
    if _absgrad:
        _need_rows("absgrad")
    P, M, dev = _check_params(xyz, features_dc, features_rest, opacity, scaling, rotation, degrees)
    H, W = int(dL_dout_color.size(1)), int(dL_dout_color.size(2))
    opts = dict(dtype=torch.float32, device=dev)
    if P == 0:
        return _zero_grads(dev, (0, 3), (0, 1), (0, 3), (0, 1, 3), (0, M - 1, 3), (0, 3), (0, 4)) + (
            _zero_grads(dev, (0, 3), (0, 2, 2)) if _want_2d else ()) + (_zero_grads(dev, (0, 3)) if _absgrad else ())
    rest = _NO_TENSOR if M == 1 else features_rest
    cap = _pair_capacity(R, P, W, H, binningBuffer)
    if _ext is not None and not _want_2d:
        return tuple((_ext.backward_params_absgrad if _absgrad else _ext.backward_params)(_t(background), xyz, _t(radii), features_dc, rest, degrees, opacity, scaling, rotation,
                                          float(scale_modifier), _t(viewmatrix), _t(projmatrix), float(tan_fovx), float(tan_fovy),
                                          dL_dout_color, _t(campos), geomBuffer, int(cap), binningBuffer, imageBuffer,
                                          float(lambda_sh_sparsity), bool(debug)))
    e = lambda *s: torch.empty(s, **opts)   # every element is written by the library
    dL_dmeans3D, dL_dmeans2D, dL_dopacity = e(P, 3), e(P, 3), e(P, 1)
    dL_ddc, dL_drest, dL_dscaling, dL_drotation = e(P, 1, 3), e(P, M - 1, 3), e(P, 3), e(P, 4)
    scratch = e(P, 9)   # dL_dcolor [P,3] + dL_dcov3D [P,6]: written by the C ABI, no leaf on this path
    dL_dconic = e(P, 2, 2) if _want_2d else None
    bg, vm, pm, cp = (_dev(t, dev) for t in (background, viewmatrix, projmatrix, campos))
    g, deg, rad = _dev(dL_dout_color, dev), _dev(degrees, dev, torch.int32), _dev(radii, dev, torch.int32)
    abs_out, abs_tail = _absgrad_tail(_absgrad, P, cap, opts)
    with _on_device(dev):
        st = (_lib.r3dgs_backward_params_absgrad if _absgrad else _lib.r3dgs_backward_params)(
            P, _ptr(deg), M, int(cap), _ptr(bg), W, H, _ptr(xyz), _ptr(features_dc), _ptr(rest),
            _ptr(scaling), float(scale_modifier), _ptr(rotation), _ptr(vm), _ptr(pm), _ptr(cp),
            float(tan_fovx), float(tan_fovy), _ptr(rad), _ptr(geomBuffer), _ptr(binningBuffer),
            _ptr(imageBuffer), _ptr(g), _ptr(dL_dmeans2D), _ptr(dL_dconic), _ptr(dL_dopacity),
            scratch.data_ptr(), _ptr(dL_dmeans3D), scratch.data_ptr() + 12 * P, _ptr(dL_ddc),
            _ptr(dL_drest), _ptr(dL_dscaling), _ptr(dL_drotation), float(lambda_sh_sparsity),
            int(bool(debug)), _stream(), *abs_tail)
    _check(st, "rasterize_gaussian_params_backward")
    out = (dL_dmeans2D, dL_dopacity, dL_dmeans3D, dL_ddc, dL_drest, dL_dscaling, dL_drotation)
    out = out + (scratch.view(-1)[:3 * P].view(P, 3), dL_dconic) if _want_2d else out
    return out + (abs_out,) if _absgrad else out


def activate_params(scaling, rotation):
    """(exp(scaling), F.normalize(rotation)) evaluated by the functions the raw-parameter kernels use (csrc/param_math.h):
    the existing entry points fed these give the fused path's image and binning bit for bit."""
    _need("params")
    dev = scaling.device
    if dev.type != "cuda":
        raise RuntimeError("the MI355X rasterizer needs device tensors (no CPU path)")
    P = int(scaling.size(0))
    if scaling.dim() != 2 or scaling.size(1) != 3:
        raise RuntimeError("scaling must have dimensions (num_points, 3)")
    if tuple(rotation.shape) != (P, 4):
        raise RuntimeError("rotation must have dimensions (num_points, 4)")
    _param(scaling, dev, "scaling")
    _param(rotation, dev, "rotation")
    if _ext is not None:
        return tuple(_ext.activate_params(scaling, rotation))
    s, q = torch.empty_like(scaling), torch.empty_like(rotation)
    if P:
        with _on_device(dev):
            _check(_lib.r3dgs_activate_params(P, _ptr(scaling), _ptr(rotation), _ptr(s), _ptr(q), _stream()), "activate_params")
    return s, q


# ---- the quantised (codebook-indexed) model: include/r3dgs_quantised.h ------------------------------------------------
# Inference only.  The arrays are read in place; a tensor that would need a copy is refused.

def _check_quantised(xyz, geom_ids, sh_ids, codebooks, perBandPrimitiveCount, cumSumPrimitiveCount, coeffsNum):
    """-> (P, xyz_is_half, device); the refusals of the quantised path."""
    dev = xyz.device
    if dev.type != "cuda":
        raise RuntimeError("the MI355X rasterizer needs device tensors (no CPU path)")
    if xyz.dim() != 2 or xyz.size(1) != 3:
        raise RuntimeError("xyz must have dimensions (num_points, 3)")
    if xyz.dtype not in (torch.float16, torch.float32):
        raise RuntimeError(f"xyz: the quantised path needs float16 or float32, got {xyz.dtype}")
    P = int(xyz.size(0))
    if geom_ids.dtype != torch.uint8 or tuple(geom_ids.shape) != (P, 8):
        raise RuntimeError("geom_ids must be uint8 with dimensions (num_points, 8)")
    if sh_ids.dtype != torch.uint8 or sh_ids.dim() != 1:
        raise RuntimeError("sh_ids must be a flat uint8 tensor")
    if codebooks.dtype != torch.float32 or tuple(codebooks.shape) != (20, 256):
        raise RuntimeError("codebooks must be float32 with dimensions (20, 256)")
    for t, name in ((perBandPrimitiveCount, "perBandPrimitiveCount"), (cumSumPrimitiveCount, "cumSumPrimitiveCount"),
                    (coeffsNum, "coeffsNum")):
        if t.dtype != torch.int32 or t.numel() != 4:
            raise RuntimeError(f"{name} must be int32 with 4 entries (degrees 0..3)")
    for t, name in ((xyz, "xyz"), (geom_ids, "geom_ids"), (sh_ids, "sh_ids"), (codebooks, "codebooks"),
                    (perBandPrimitiveCount, "perBandPrimitiveCount"), (cumSumPrimitiveCount, "cumSumPrimitiveCount"),
                    (coeffsNum, "coeffsNum")):
        if t.device != dev:
            raise RuntimeError(f"{name}: expected a tensor on {dev}, got {t.device}")
        if not t.is_contiguous():
            raise RuntimeError(f"{name}: the quantised path needs a contiguous tensor")
    return P, int(xyz.dtype == torch.float16), dev


def rasterize_gaussians_quantised(background, xyz, geom_ids, sh_ids, codebooks, scale_modifier, viewmatrix, projmatrix,
                                  tan_fovx, tan_fovy, image_height, image_width, perBandPrimitiveCount, cumSumPrimitiveCount,
                                  coeffsNum, campos, prefiltered, debug, counters=None, exact=False, _reserve=None,
                                  _strict_override=None):
    """rasterize_gaussians_variableSH_bands over the quantised model (xyz half or float [P,3], geom_ids uint8 [P,8], sh_ids
    uint8 ragged, codebooks float [20,256]; r3dgs_quantised.QuantisedModel holds them) -> (num_rendered, out_color[3,H,W],
    radii[P], geomBuffer, binningBuffer, imgBuffer); same asynchronous / exact-size / strict-mode behaviour.  `counters`:
    (out_touched_pixels int32 [P], out_transmittance float [P]) for counter mode.  sh_ids is not length-checked against the
    band tables here (they live on the device); QuantisedModel builds them together."""
    _need("quantised")
    P, half, dev = _check_quantised(xyz, geom_ids, sh_ids, codebooks, perBandPrimitiveCount, cumSumPrimitiveCount, coeffsNum)
    H, W = int(image_height), int(image_width)
    empty, _, strict = _forward_prologue(P, dev, H, W, _strict_override)   # (no backward exists for this model: trains is moot)
    if empty is not None:
        return empty
    out_color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    radii = torch.empty((P,), dtype=torch.int32, device=dev)
    bg, vm, pm, cp = (_dev(t, dev) for t in (background, viewmatrix, projmatrix, campos))
    touched = transm = None
    if counters is not None:
        touched, transm = counters
    if vm is not None:
        _track_view(vm)
    _lib.r3dgs_forward_hint(0)   # no backward exists for this model
    with _on_device(dev):
        args = (P, None, 4, _ptr(coeffsNum), _ptr(perBandPrimitiveCount), _ptr(cumSumPrimitiveCount), _ptr(bg), W, H,
                xyz.data_ptr(), half, geom_ids.data_ptr(), sh_ids.data_ptr() if sh_ids.numel() else None, codebooks.data_ptr(),
                float(scale_modifier), _ptr(vm), _ptr(pm), _ptr(cp), float(tan_fovx), float(tan_fovy), int(bool(prefiltered)),
                _ptr(out_color), _ptr(touched), _ptr(transm), _ptr(radii), int(counters is not None), int(bool(debug)),
                _stream())
        return _drive_forward(_lib.r3dgs_quantised_forward, _lib.r3dgs_quantised_forward_reserved, args,
                              "rasterize_gaussians_quantised", dev, P, W, H, _ptr(vm), True, counters, out_color, radii, exact,
                              debug, _reserve, strict)


def quantised_decode(xyz, geom_ids, sh_ids, codebooks, perBandPrimitiveCount, cumSumPrimitiveCount, coeffsNum, want_xyz=True):
    """The dense fp32 tensors the reference's load_ply returns for the model, decoded on the device by the functions the
    quantised kernels use (csrc/quant_math.h) -> (xyz [P,3], features_dc [P,1,3], features_rest [P,15,3], opacity [P,1],
    scaling [P,3], rotation [P,4], degrees int32 [P,1]).  want_xyz=False: the positions are not decoded (xyz_out NULL) and
    the first entry is None -- for a caller that holds them in float already."""
    _need("quantised")
    P, half, dev = _check_quantised(xyz, geom_ids, sh_ids, codebooks, perBandPrimitiveCount, cumSumPrimitiveCount, coeffsNum)
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)   # every element is written by the library
    out = (f(P, 3) if want_xyz else None, f(P, 1, 3), f(P, 15, 3), f(P, 1), f(P, 3), f(P, 4),
           torch.empty((P, 1), dtype=torch.int32, device=dev))
    if P:
        with _on_device(dev):
            _check(_lib.r3dgs_quantised_decode(P, _ptr(coeffsNum), _ptr(perBandPrimitiveCount), _ptr(cumSumPrimitiveCount),
                                               xyz.data_ptr(), half, geom_ids.data_ptr(),
                                               sh_ids.data_ptr() if sh_ids.numel() else geom_ids.data_ptr(),
                                               codebooks.data_ptr(), *(_ptr(t) for t in out), _stream()), "quantised_decode")
    return out


QUANTISED_GRAD_CHUNK = 1024   # csrc/quant_math.h kQuantGradChunk: consecutive Gaussians one wave sums before the next chunk
QUANTISED_GRAD_MAX_GROUPS = 2048   # kQuantGradMaxGroups: above that many chunks a wave takes a run of them


def _check_quantised_grads(geom_ids, sh_ids, perBandPrimitiveCount, cumSumPrimitiveCount, coeffsNum, grads):
    """-> (P, device); the refusals of quantised_codebook_grad."""
    dev = geom_ids.device
    if dev.type != "cuda":
        raise RuntimeError("the MI355X rasterizer needs device tensors (no CPU path)")
    if geom_ids.dtype != torch.uint8 or geom_ids.dim() != 2 or geom_ids.size(1) != 8:
        raise RuntimeError("geom_ids must be uint8 with dimensions (num_points, 8)")
    P = int(geom_ids.size(0))
    if sh_ids.dtype != torch.uint8 or sh_ids.dim() != 1:
        raise RuntimeError("sh_ids must be a flat uint8 tensor")
    tables = ((perBandPrimitiveCount, "perBandPrimitiveCount"), (cumSumPrimitiveCount, "cumSumPrimitiveCount"),
              (coeffsNum, "coeffsNum"))
    for t, name in tables:
        if t.dtype != torch.int32 or t.numel() != 4:
            raise RuntimeError(f"{name} must be int32 with 4 entries (degrees 0..3)")
    shapes = (("dL_dfeatures_dc", (P, 1, 3)), ("dL_dfeatures_rest", (P, 15, 3)), ("dL_dopacity", (P, 1)),
              ("dL_dscaling", (P, 3)), ("dL_drotation", (P, 4)))
    for t, (name, shape) in zip(grads, shapes):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape):
            raise RuntimeError(f"{name} must be float32 with dimensions {shape} (or None)")
    for t, name in ((geom_ids, "geom_ids"), (sh_ids, "sh_ids")) + tables + tuple(
            (t, n) for t, (n, _) in zip(grads, shapes) if t is not None):
        if t.device != dev:
            raise RuntimeError(f"{name}: expected a tensor on {dev}, got {t.device}")
        if not t.is_contiguous():
            raise RuntimeError(f"{name}: quantised_codebook_grad needs a contiguous tensor")
    return P, dev


def quantised_codebook_grad(geom_ids, sh_ids, perBandPrimitiveCount, cumSumPrimitiveCount, coeffsNum, dL_dfeatures_dc,
                            dL_dfeatures_rest, dL_dopacity, dL_dscaling, dL_drotation):
    """The adjoint of quantised_decode in the codebooks (include/r3dgs_quantised.h r3dgs_quantised_codebook_grad): the
    gradients of the decoded tensors, shaped as quantised_decode returns them (None = zeros), summed into the centres the ids
    name -> dL_dcodebooks float32 [20,256].  Double accumulation in a fixed order, one rounding, no atomics: the same inputs
    give the same bits.  Rows of dL_dfeatures_rest above a Gaussian's degree are not read."""
    _need("quantised_grad")
    grads = (dL_dfeatures_dc, dL_dfeatures_rest, dL_dopacity, dL_dscaling, dL_drotation)
    if _ext is not None:
        return _ext.quantised_codebook_grad(geom_ids, sh_ids, perBandPrimitiveCount, cumSumPrimitiveCount, coeffsNum,
                                            *(_t(t) for t in grads))
    P, dev = _check_quantised_grads(geom_ids, sh_ids, perBandPrimitiveCount, cumSumPrimitiveCount, coeffsNum, grads)
    out = torch.empty((20, 256), dtype=torch.float32, device=dev)   # every entry is written by the library
    work = torch.empty(int(_lib.r3dgs_quantised_codebook_grad_workspace_bytes(P)), dtype=torch.uint8, device=dev)
    with _on_device(dev):
        _check(_lib.r3dgs_quantised_codebook_grad(P, _ptr(coeffsNum), _ptr(perBandPrimitiveCount), _ptr(cumSumPrimitiveCount),
                                                  _ptr(geom_ids), _ptr(sh_ids), *(_ptr(t) for t in grads), out.data_ptr(),
                                                  _ptr(work), _stream()), "quantised_codebook_grad")
    return out


def quantised_bytes(P, per_band_count, xyz_is_half):
    """Resident bytes of a quantised model with `per_band_count` Gaussians of degree 0..3 (needs no GPU)."""
    _need("quantised")
    counts = (_i * 4)(*[int(c) for c in per_band_count])
    n = int(_lib.r3dgs_quantised_bytes(int(P), counts, int(bool(xyz_is_half))))
    if n == 0:
        raise RuntimeError(f"quantised_bytes: {_lib.r3dgs_last_error().decode()}")
    return n


def mark_visible(means3D, viewmatrix, projmatrix):
    """markVisible (rasterize_points.cu:307-326): bool[P], view-space z > 0.2."""
    if _ext is not None:
        return _ext.mark_visible(means3D, _t(viewmatrix), _t(projmatrix))
    dev = means3D.device
    P = int(means3D.size(0))
    present = torch.zeros((P,), dtype=torch.bool, device=dev)
    if P:
        m3, vm, pm = _dev(means3D, dev), _dev(viewmatrix, dev), _dev(projmatrix, dev)
        with _on_device(dev):
            _check(_lib.r3dgs_mark_visible(P, _ptr(m3), _ptr(vm), _ptr(pm), _ptr(present), _stream()), "mark_visible")
    return present


def export_binning(P, R, H, W, geomBuffer, binningBuffer, imageBuffer):
    """Debug accessor (not in the reference): sorted 64-bit keys in the reference's format, point list, tile
    ranges, n_contrib, final T and tiles_touched of a finished forward -- for bit-exact integer parity tests."""
    dev = geomBuffer.device
    gx, gy = (W + 15) // 16, (H + 15) // 16
    cap = _pair_capacity(R, P, W, H, binningBuffer)
    if isinstance(R, NumRendered):
        R = R.pairs
    R = min(int(R), cap)
    keys = torch.empty((R,), dtype=torch.int64, device=dev)
    plist = torch.empty((R,), dtype=torch.int32, device=dev)
    ranges = torch.empty((gx * gy, 2), dtype=torch.int32, device=dev)
    n_contrib = torch.empty((H * W,), dtype=torch.int32, device=dev)
    final_T = torch.empty((H * W,), dtype=torch.float32, device=dev)
    tiles = torch.empty((P,), dtype=torch.int32, device=dev)
    with _on_device(dev):
        _check(_lib.r3dgs_export_binning(P, cap, R, W, H, _ptr(geomBuffer), _ptr(binningBuffer), _ptr(imageBuffer),
                                         _ptr(keys), _ptr(plist), _ptr(ranges), _ptr(n_contrib), _ptr(final_T),
                                         _ptr(tiles), _stream()), "export_binning")
    return dict(keys=keys, point_list=plist, ranges=ranges, n_contrib=n_contrib, final_T=final_T, tiles_touched=tiles)


def export_rects(P, geomBuffer):
    """Debug accessor (not in the reference): the tile rect (x0, y0, x1, y1; exclusive maxima) every Gaussian was binned
    into, int32[P,4] (rows of culled Gaussians are undefined)."""
    out = torch.empty((P, 4), dtype=torch.int16, device=geomBuffer.device)
    with _on_device(geomBuffer.device):
        _check(_lib.r3dgs_export_rects(P, _ptr(geomBuffer), _ptr(out), _stream()), "export_rects")
    return out.to(torch.int32) & 0xFFFF


def set_tight_rects(on):
    """True (default): a Gaussian is binned into the tiles of the reference's 3-sigma square that it can actually reach
    with alpha >= 1/255 (bounding box of that ellipse); False: into the whole square, i.e. lists identical to the
    reference's.  Image, radii, num_rendered and gradients are the same either way.  Returns the previous setting."""
    return bool(_lib.r3dgs_set_tight_rects(int(bool(on))))


def tight_rects():
    return bool(_lib.r3dgs_set_tight_rects(-1))


_tls = threading.local()   # .next_forward_trains: None / absent = nobody said -- a forward under torch.no_grad() is a rendering


def hint_next_forward(will_backward):
    """The autograd wrapper says whether any input of the forward it is about to issue needs a gradient.  A forward that
    no backward will follow (rendering under no_grad) skips what it would only do for the backward's sake (the SH direction
    derivatives, 36 B per visible Gaussian).  One-shot: the call after the next forward trains again."""
    _tls.next_forward_trains = bool(will_backward)


class forward_state:
    """`with forward_state() as st:` -- st.result is the six-tuple (num_rendered, out_color, radii, geomBuffer,
    binningBuffer, imgBuffer) of the last non-empty forward this thread issued inside the block, through whichever
    wrapper or autograd function (None: there was none, e.g. P == 0).  How r3dgs_render.render(aux=...) gets at the state
    blobs of the forward it has just run; nothing is kept outside such a block."""

    def __init__(self):
        self.result = None

    def __enter__(self):
        self._outer = getattr(_tls, "forward_recorder", None)
        _tls.forward_recorder = self
        return self

    def __exit__(self, *a):
        _tls.forward_recorder = self._outer


# ---- the replay calls: what their wrappers share (DESIGN.md "Replay passes", the host contract) ----------------------------
_NO_CPU_PATH = "the MI355X rasterizer needs device tensors (no CPU path)"


def _subset(what, kind, names, allowed):
    """`names` as a tuple; a name outside `allowed` is refused (kind: what a name is called in the message)."""
    names = tuple(names)
    for name in names:
        if name not in allowed:
            raise ValueError(f"{what}: unknown {kind} {name!r} (expected a subset of {allowed})")
    return names


def _replay_state(what, who, P, R, H, W, geomBuffer, binningBuffer, imageBuffer, model=None, fallback=None):
    """The state of a replay call -> (P, H, W, pair capacity, device).  The device is the `model` tensor's, and the three
    buffers must live there too; model=None: the state buffers' own (the image buffer's, the geometry buffer's behind an empty
    one).  Host tensors are refused unless P == 0; then nothing says where, and it is `fallback` if that is a device, else the
    current device, as the forward's empty result.  who: the subject of the one-device refusal.  R: a NumRendered, or a plain
    pair capacity (_pair_capacity)."""
    P, H, W = int(P), int(H), int(W)
    dev = model.device if model is not None else imageBuffer.device if imageBuffer.numel() else geomBuffer.device
    if P and dev.type != "cuda":
        raise RuntimeError(_NO_CPU_PATH)
    if dev.type != "cuda":
        dev = fallback if fallback is not None and fallback.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    if P and not (geomBuffer.device == binningBuffer.device == imageBuffer.device == (imageBuffer.device if model is None else dev)):
        raise RuntimeError(f"{what}: {who} must live on one device")
    return P, H, W, int(_pair_capacity(R, P, W, H, binningBuffer)) if P else 0, dev


def _workspace(what, nbytes, dev, work):
    """The workspace of a call whose size query said `nbytes`, from torch's caching allocator (at least one byte: never a NULL
    pointer).  A query that says 0 although there is `work` has failed: refused with the library's message."""
    if nbytes == 0 and work:
        _check(-1, f"{what}_workspace_bytes")
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


AUX_MAPS = ("depth", "alpha", "median_depth")


def aux_maps(P, R, H, W, geomBuffer, binningBuffer, imageBuffer, maps=AUX_MAPS, checks=False):
    """r3dgs_aux_maps (include/r3dgs_aux.h) over the three buffers a forward returned -> {name: float [1,H,W]} for the names
    in `maps` (any subset of AUX_MAPS): "depth" = sum z alpha T over the blended entries (not normalised), "alpha" = 1 - final
    T, "median_depth" = z of the first entry that leaves T < 0.5 (0: none).  R: the forward's num_rendered (a NumRendered) or
    the pair capacity of its binning buffer.  checks=True adds "T_check" (float [H,W]) and "n_check" (int32 [H,W]): the pass's
    own final T and last contributor.  The buffers are only read; the maps carry no gradient."""
    maps = _subset("aux_maps", "map", maps, AUX_MAPS)
    P, H, W, cap, dev = _replay_state("aux_maps", "the three state buffers", P, R, H, W, geomBuffer, binningBuffer, imageBuffer)
    if _ext is not None:
        got = _ext.aux_maps(P, cap, H, W, geomBuffer, binningBuffer, imageBuffer, "depth" in maps, "alpha" in maps,
                            "median_depth" in maps, bool(checks))
        out = {name: t for name, t in zip(AUX_MAPS, got[:3]) if name in maps}
        if checks:
            out["T_check"], out["n_check"] = got[3], got[4]
        return out
    out = {name: torch.empty((1, H, W), dtype=torch.float32, device=dev) for name in maps}
    if checks:
        out["T_check"] = torch.empty((H, W), dtype=torch.float32, device=dev)
        out["n_check"] = torch.empty((H, W), dtype=torch.int32, device=dev)
    with _on_device(dev):
        _check(_lib.r3dgs_aux_maps(P, cap, W, H, _ptr(geomBuffer), _ptr(binningBuffer), _ptr(imageBuffer),
                                   _ptr(out.get("depth")), _ptr(out.get("alpha")), _ptr(out.get("median_depth")),
                                   _ptr(out.get("T_check")), _ptr(out.get("n_check")), _stream()), "aux_maps")
    return out


AUX_GRADS = ("means2D", "means3D", "opacity", "scales", "rotations", "cov3D")
_AUX_GRAD_COLS = dict(means2D=3, means3D=3, opacity=1, scales=3, rotations=4, cov3D=6)


# the two screen-space outputs of the _screen entry points (what camera_backward_maps reads next to "means2D")
SCREEN_GRADS = ("conic", "z")
_SCREEN_GRAD_COLS = dict(conic=4, z=1)
_AUX_GRAD_COLS.update(_SCREEN_GRAD_COLS)


def aux_maps_backward(P, R, H, W, geomBuffer, binningBuffer, imageBuffer, viewmatrix, projmatrix, tanfovx, tanfovy, means3D,
                      scales, scale_modifier, rotations, cov3D_precomp, radii, dL_ddepth=None, dL_dalpha=None, dL_dmedian=None,
                      want=AUX_GRADS, _screen=False):
    """r3dgs_aux_maps_backward (include/r3dgs_aux.h): the gradients of the maps of `aux_maps` over the same three buffers.
    dL_ddepth / dL_dalpha / dL_dmedian: float tensors of H*W elements (any shape), None = zero.  scales / rotations are the
    ACTIVATED values (or cov3D_precomp is given and they are empty).  -> {name: float [P, cols]} for the names in `want` (a
    subset of AUX_GRADS); "opacity" is the gradient of the raw opacity, "means2D" what densification reads.  The buffers are
    only read; the workspace is allocated here, per call, from torch's caching allocator.
    _screen=True (`aux_maps_backward_screen`): r3dgs_aux_maps_backward_screen -- `want` may also name the SCREEN_GRADS "conic"
    [P,4] (A, B, 0, C) and "z" [P,1], the screen-space sums camera_backward_maps reads next to "means2D"; with none of
    "means3D" .. "cov3D" wanted the model is frozen and the chain behind those sums is skipped."""
    names, native = _screen_variant(_screen, AUX_GRADS, "r3dgs_aux_maps_backward")
    want = _subset("aux_maps_backward", "gradient", want, names)
    P, H, W, cap, dev = _replay_state("aux_maps_backward", "the state buffers and the model", P, R, H, W, geomBuffer,
                                      binningBuffer, imageBuffer, means3D)
    ups = []
    for name, g in (("dL_ddepth", dL_ddepth), ("dL_dalpha", dL_dalpha), ("dL_dmedian", dL_dmedian)):
        g = _dev(g, dev)
        if g is not None and g.numel() != H * W:
            raise RuntimeError(f"aux_maps_backward: {name} has {g.numel()} elements, the image {H * W}")
        ups.append(g)
    return _map_backward("aux_maps_backward", dev, P, cap, H, W, (geomBuffer, binningBuffer, imageBuffer),
                         (viewmatrix, projmatrix, tanfovx, tanfovy, means3D, scales, scale_modifier, rotations, cov3D_precomp, radii),
                         (lambda: _lib.r3dgs_aux_maps_backward_workspace_bytes(P, cap, W, H), native),
                         (), [_ptr(g) for g in ups], names, _AUX_GRAD_COLS, want)


# a map backward and its _screen form, by the sibling's name
_SCREEN_ENTRY = {"r3dgs_aux_maps_backward": "r3dgs_aux_maps_backward_screen",
                 "r3dgs_distortion_map_backward": "r3dgs_distortion_backward_screen",
                 "r3dgs_feature_maps_backward": "r3dgs_feature_maps_backward_screen"}


def _screen_variant(screen, names, entry):
    """(every output of the call in its order, the native call) of the map backward `entry` or of its _screen form."""
    if not screen:
        return names, getattr(_lib, entry)
    return names + SCREEN_GRADS, getattr(_lib, _SCREEN_ENTRY[entry])


def aux_maps_backward_screen(*args, **kwargs):
    """r3dgs_aux_maps_backward_screen (include/r3dgs_aux.h): `aux_maps_backward` whose `want` may also name "conic" and "z"."""
    return aux_maps_backward(*args, _screen=True, **kwargs)


def distortion_backward_screen(*args, **kwargs):
    """r3dgs_distortion_backward_screen (include/r3dgs_distortion.h): `distortion_map_backward` whose `want` may also name
    "conic" and "z" (the latter behind dm / dz of the mapping)."""
    return distortion_map_backward(*args, _screen=True, **kwargs)


def feature_maps_backward_screen(*args, **kwargs):
    """r3dgs_feature_maps_backward_screen (include/r3dgs_features.h): `feature_maps_backward` whose `want` may also name
    "conic" and "z" (zeros: a feature map does not read the depth)."""
    return feature_maps_backward(*args, _screen=True, **kwargs)


def _map_backward(what, dev, P, cap, H, W, buffers, geometry, native, lead, trail, names, cols, want):
    """The body of the three map backwards, behind the unit's own checks -> {name: float [P, cols[name]]} for the names in
    `want`.  geometry: viewmatrix, projmatrix, tanfovx, tanfovy, means3D, scales, scale_modifier, rotations, cov3D_precomp,
    radii, as the wrappers take them.  native: the unit's (workspace query, call); lead / trail: the call's own arguments
    in front of viewmatrix and behind radii; names: every output of the call, in its order."""
    out = {name: torch.empty((P, cols[name]), dtype=torch.float32, device=dev) for name in want}
    if P == 0:
        return out
    viewmatrix, projmatrix, tanfovx, tanfovy, means3D, scales, scale_modifier, rotations, cov3D_precomp, radii = geometry
    m3, sc, rot, cov = _dev(means3D, dev), _dev(scales, dev), _dev(rotations, dev), _dev(cov3D_precomp, dev)
    rad = _dev(radii, dev, torch.int32)
    vm, pm = _dev(viewmatrix, dev), _dev(projmatrix, dev)
    query, call = native
    with _on_device(dev):
        work = _workspace(what, query(), dev, cap)
        _check(call(P, cap, W, H, *[_ptr(b) for b in buffers], *lead, _ptr(vm), _ptr(pm), float(tanfovx), float(tanfovy), _ptr(m3),
                    _ptr(sc), float(scale_modifier), _ptr(rot), _ptr(cov), _ptr(rad), *trail,
                    *[_ptr(out.get(name)) for name in names], work.data_ptr(), _stream()), what)
    return out


def depth_mapping(mapping):
    """The (near, far) pair the distortion calls take: True / None / (0, 0) = the linear mapping m = z; (near, far) with
    0 < near < far = 2DGS's m = far / (far - near) (1 - near / z).  Anything else raises ValueError."""
    if mapping is True or mapping is None:
        return 0.0, 0.0
    try:
        near, far = (float(v) for v in mapping)
    except (TypeError, ValueError):
        raise ValueError(f"distortion: expected True or a (near, far) pair, got {mapping!r}") from None
    if not ((near == 0.0 and far == 0.0) or 0.0 < near < far):
        raise ValueError(f"distortion: need near = far = 0 (the linear mapping) or 0 < near < far, got ({near}, {far})")
    return near, far


def distortion_map(P, R, H, W, geomBuffer, binningBuffer, imageBuffer, near=0.0, far=0.0, want_moments=False):
    """r3dgs_distortion_map (include/r3dgs_distortion.h) over the three buffers a forward returned -> float [1,H,W]: per pixel
    sum_{j<k} w_j w_k (m_k - m_j)^2 over the Gaussians the forward blended (w = alpha T, m the mapped depth: linear for
    near = far = 0, 2DGS's for 0 < near < far).  want_moments=True -> (map, moments float [2,H,W]): what distortion_map_backward
    reads.  R as in aux_maps.  One launch, no host wait; the buffers are only read; the map carries no gradient."""
    near, far = depth_mapping((near, far))
    P, H, W, cap, dev = _replay_state("distortion_map", "the three state buffers", P, R, H, W, geomBuffer, binningBuffer,
                                      imageBuffer)
    out = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    moments = torch.empty((2, H, W), dtype=torch.float32, device=dev) if want_moments else None
    with _on_device(dev):
        _check(_lib.r3dgs_distortion_map(P, cap, W, H, _ptr(geomBuffer), _ptr(binningBuffer), _ptr(imageBuffer), near, far,
                                         _ptr(out), _ptr(moments), _stream()), "distortion_map")
    return (out, moments) if want_moments else out


def distortion_map_backward(P, R, H, W, geomBuffer, binningBuffer, imageBuffer, viewmatrix, projmatrix, tanfovx, tanfovy, means3D,
                            scales, scale_modifier, rotations, cov3D_precomp, radii, dL_ddistortion, moments, near=0.0, far=0.0,
                            want=AUX_GRADS, _screen=False):
    """r3dgs_distortion_map_backward (include/r3dgs_distortion.h): the gradients of the map of `distortion_map` over the same
    three buffers, from dL_ddistortion (float, H*W elements, any shape; None = zero) and the `moments` that call returned for
    the same (near, far).  Everything else as aux_maps_backward: activated scales / rotations or cov3D_precomp -> {name: float
    [P, cols]} for the names in `want` (a subset of AUX_GRADS).  The workspace is allocated here, per call.  _screen=True: as
    in aux_maps_backward."""
    near, far = depth_mapping((near, far))
    names, native = _screen_variant(_screen, AUX_GRADS, "r3dgs_distortion_map_backward")
    want = _subset("distortion_map_backward", "gradient", want, names)
    P, H, W, cap, dev = _replay_state("distortion_map_backward", "the state buffers and the model", P, R, H, W, geomBuffer,
                                      binningBuffer, imageBuffer, means3D)
    g, mom = _dev(dL_ddistortion, dev), _dev(moments, dev)
    if g is not None and g.numel() != H * W:
        raise RuntimeError(f"distortion_map_backward: dL_ddistortion has {g.numel()} elements, the image {H * W}")
    if g is not None and P and (mom is None or mom.numel() != 2 * H * W):
        raise RuntimeError(f"distortion_map_backward: moments must have {2 * H * W} elements (distortion_map(want_moments=True))")
    return _map_backward("distortion_map_backward", dev, P, cap, H, W, (geomBuffer, binningBuffer, imageBuffer),
                         (viewmatrix, projmatrix, tanfovx, tanfovy, means3D, scales, scale_modifier, rotations, cov3D_precomp, radii),
                         (lambda: _lib.r3dgs_distortion_map_backward_workspace_bytes(P, cap, W, H), native),
                         (near, far), (_ptr(g), _ptr(mom)), names, _AUX_GRAD_COLS, want)


FEATURE_MAX_CHANNELS = 512   # R3DGS_FEATURE_MAX_CHANNELS (include/r3dgs_features.h)
FEATURE_GRADS = ("features",) + AUX_GRADS


def _feature_tensor(features, P, dev, what):
    """`features` as the library reads it: float32 [P, C] on `dev`, contiguous (copied if it is not); refused otherwise."""
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] != P:
        shape = tuple(features.shape) if isinstance(features, torch.Tensor) else type(features).__name__
        raise ValueError(f"{what}: features must be a [P, C] tensor with P = {P}, got {shape}")
    C_ = int(features.shape[1])
    if not 1 <= C_ <= FEATURE_MAX_CHANNELS:
        raise ValueError(f"{what}: need 1 <= C <= {FEATURE_MAX_CHANNELS} feature channels, got C = {C_}")
    if features.dtype != torch.float32:
        raise ValueError(f"{what}: features must be float32, got {str(features.dtype)[6:]}")
    if P and dev is not None and features.device != dev:
        raise ValueError(f"{what}: features must live on {dev}, got {features.device}")
    return features.detach().contiguous(), C_


def feature_maps(P, R, H, W, geomBuffer, binningBuffer, imageBuffer, features):
    """r3dgs_feature_maps (include/r3dgs_features.h) over the three buffers a forward returned: features float32 [P, C] ->
    float [C, H, W], out[c] = sum over the blended Gaussians of features[id, c] * alpha * T (not normalised, no background
    term).  R: the forward's num_rendered (a NumRendered) or the pair capacity of its binning buffer.  The buffers are only
    read; the map carries no gradient."""
    feats, C_ = _feature_tensor(features, int(P), None, "feature_maps")
    P, H, W, cap, dev = _replay_state("feature_maps", "the three state buffers", P, R, H, W, geomBuffer, binningBuffer, imageBuffer,
                                      fallback=features.device)
    _feature_tensor(features, P, dev, "feature_maps")
    out = torch.empty((C_, H, W), dtype=torch.float32, device=dev)
    with _on_device(dev):
        _check(_lib.r3dgs_feature_maps(P, cap, W, H, _ptr(geomBuffer), _ptr(binningBuffer), _ptr(imageBuffer), _ptr(feats),
                                       C_, out.data_ptr(), _stream()), "feature_maps")
    return out


def feature_maps_backward(P, R, H, W, geomBuffer, binningBuffer, imageBuffer, viewmatrix, projmatrix, tanfovx, tanfovy, means3D,
                          scales, scale_modifier, rotations, cov3D_precomp, radii, features, dL_dout, want=FEATURE_GRADS, _screen=False):
    """r3dgs_feature_maps_backward (include/r3dgs_features.h): dL_dout (C*H*W elements, None = zero) -> {name: float [P, cols]}
    for the names in `want` (a subset of FEATURE_GRADS): "features" [P, C] and the geometry gradients of aux_maps_backward, in
    its units.  With only "features" wanted the geometry is frozen: the geometric sums and the per-Gaussian chain are skipped and
    viewmatrix .. cov3D_precomp may be None.  The buffers are only read; the workspace is allocated here, per call, from
    torch's caching allocator.  _screen=True: as in aux_maps_backward."""
    names, native = _screen_variant(_screen, FEATURE_GRADS, "r3dgs_feature_maps_backward")
    want = _subset("feature_maps_backward", "gradient", want, names)
    P, H, W, cap, dev = _replay_state("feature_maps_backward", "the state buffers and the features", P, R, H, W, geomBuffer,
                                      binningBuffer, imageBuffer, features)
    feats, C_ = _feature_tensor(features, P, dev, "feature_maps_backward")
    g = _dev(dL_dout, dev)
    if g is not None and g.numel() != C_ * H * W:
        raise RuntimeError(f"feature_maps_backward: dL_dout has {g.numel()} elements, the map {C_ * H * W}")
    return _map_backward("feature_maps_backward", dev, P, cap, H, W, (geomBuffer, binningBuffer, imageBuffer),
                         (viewmatrix, projmatrix, tanfovx, tanfovy, means3D, scales, scale_modifier, rotations, cov3D_precomp, radii),
                         (lambda: _lib.r3dgs_feature_maps_backward_workspace_bytes(P, cap, C_, W, H), native),
                         (), (_ptr(feats), C_, _ptr(g)), names, dict(_AUX_GRAD_COLS, features=C_), want)


SCORES = ("sum", "max", "count", "views")
_SCORE_DTYPES = dict(sum=torch.float64, max=torch.float32, count=torch.int64, views=torch.int32)


def _score_tensor(t, dev, name, numel, dtype):
    """An input or output of contribution_scores as the library takes it, in place: refused instead of converted or copied."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"contribution_scores: {name} must be a tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise RuntimeError(f"contribution_scores: {name} must be a device tensor (no CPU path), got {t.device}")
    if dev is not None and t.device != dev:
        raise RuntimeError(f"contribution_scores: {name} must live on {dev}, got {t.device}")
    if t.dtype != dtype:
        raise RuntimeError(f"contribution_scores: {name} must be {str(dtype)[6:]}, got {str(t.dtype)[6:]}")
    if t.numel() != numel:
        raise RuntimeError(f"contribution_scores: {name} has {t.numel()} elements, expected {numel}")
    if not t.is_contiguous():
        raise RuntimeError(f"contribution_scores: {name} must be contiguous (it is written and read in place, never copied)")
    return t


def contribution_scores(P, R, H, W, geomBuffer, binningBuffer, imageBuffer, pixel_weight=None, out=None, accumulate=False,
                        checks=False):
    """r3dgs_contribution_scores (include/r3dgs_importance.h) over the three buffers a forward returned -> {name: tensor [P]}:
    "sum" (float64) of pixel_weight * alpha * T over the pixels that blend a Gaussian, "max" (float32) of alpha * T, "count"
    (int64) of those pixels, "views" (int32) = count > 0.  pixel_weight: float32 of H*W elements or None (ones); a pixel of
    weight 0 is left out of all four.  out: None (all four, allocated here) or a dict of any of the four names to [P] tensors
    that are written in place -- the names it lacks are not computed.  accumulate: fold the view into what `out` holds instead
    of overwriting it.  R: the forward's num_rendered (a NumRendered) or the pair capacity of its binning buffer.
    checks=True adds "T_check" (float [H,W]) and "n_check" (int32 [H,W]): the walk's own final T and last contributor.
    Host, non-contiguous and wrong-dtype tensors are refused, nothing is copied; the buffers are only read; the workspace is
    allocated here, per call, from torch's caching allocator."""
    P, H, W = int(P), int(H), int(W)
    if P < 0 or H < 1 or W < 1:
        raise ValueError(f"contribution_scores: need P >= 0 and H, W >= 1, got P = {P}, {W}x{H}")
    dev = None
    for t in (imageBuffer, geomBuffer, pixel_weight, *(out.values() if isinstance(out, dict) else ())):
        if isinstance(t, torch.Tensor) and t.numel() and t.device.type == "cuda":
            dev = t.device
            break
    if P and (dev is None or imageBuffer.device.type != "cuda"):
        raise RuntimeError(_NO_CPU_PATH)
    if out is not None:
        if not isinstance(out, dict) or any(name not in SCORES for name in out):
            raise ValueError(f"contribution_scores: out must be a dict with names among {SCORES}")
        for name, t in out.items():
            _score_tensor(t, dev, name, P, _SCORE_DTYPES[name])
    elif accumulate:
        raise ValueError("contribution_scores: accumulate needs the buffers to fold into (out=...)")
    if pixel_weight is not None:
        _score_tensor(pixel_weight, dev, "pixel_weight", H * W, torch.float32)
    if P and not (geomBuffer.device == binningBuffer.device == imageBuffer.device == dev):
        raise RuntimeError("contribution_scores: the state buffers, the weights and the outputs must live on one device")
    if dev is None:   # P == 0 and nothing says where: the current device, as the forward's empty result
        dev = torch.device("cuda", torch.cuda.current_device())
    if out is None:
        out = {name: torch.empty(P, dtype=_SCORE_DTYPES[name], device=dev) for name in SCORES}
    cap = int(_pair_capacity(R, P, W, H, binningBuffer)) if P else 0
    res = dict(out)
    if _ext is not None:
        got = _ext.contribution_scores(P, cap, H, W, geomBuffer, binningBuffer, imageBuffer, _t(pixel_weight),
                                       *[_t(out.get(name)) for name in SCORES], bool(accumulate), bool(checks))
        if checks:
            res["T_check"], res["n_check"] = got
        return res
    if checks:
        res["T_check"] = torch.empty((H, W), dtype=torch.float32, device=dev)
        res["n_check"] = torch.empty((H, W), dtype=torch.int32, device=dev)
    with _on_device(dev):
        work = _workspace("contribution_scores", _lib.r3dgs_contribution_scores_workspace_bytes(P, cap, W, H), dev, P and cap)
        _check(_lib.r3dgs_contribution_scores(
            P, cap, W, H, _ptr(geomBuffer), _ptr(binningBuffer), _ptr(imageBuffer), _ptr(pixel_weight),
            *[_ptr(out.get(name)) for name in SCORES], int(bool(accumulate)), _ptr(res.get("T_check")), _ptr(res.get("n_check")),
            work.data_ptr(), _stream()), "contribution_scores")
    return res


CAMERA_GRADS = ("viewmatrix", "projmatrix", "campos")
_CAMERA_GRAD_SHAPES = dict(viewmatrix=(4, 4), projmatrix=(4, 4), campos=(3,))


def _cam_tensor(t, dev, name, numel=None, dtype=torch.float32):
    """An input of camera_backward as the library reads it, in place: refused instead of converted.  None / empty -> None."""
    if t is None or t.numel() == 0:
        return None
    if t.device.type != "cuda":
        raise RuntimeError(f"camera_backward: {name}: the MI355X rasterizer needs device tensors (no CPU path)")
    if t.device != dev:
        raise RuntimeError(f"camera_backward: {name}: expected a tensor on {dev}, got {t.device}")
    if t.dtype != dtype:
        raise RuntimeError(f"camera_backward: {name}: expected {str(dtype)[6:]}, got {str(t.dtype)[6:]}")
    if not t.is_contiguous():
        raise RuntimeError(f"camera_backward: {name}: expected a contiguous tensor")
    if numel is not None and t.numel() != numel:
        raise RuntimeError(f"camera_backward: {name}: expected {numel} elements, got {t.numel()}")
    return t.detach()


def camera_backward(means3D, degrees, sh, sh_rest, scales, rotations, scale_modifier, cov3D_precomp, raw_params, viewmatrix,
                    projmatrix, campos, tanfovx, tanfovy, image_height, image_width, radii, geomBuffer, dL_dmeans2D, dL_dconic,
                    dL_dcolors, want=CAMERA_GRADS):
    """r3dgs_camera_backward (include/r3dgs_camera.h): the partial derivatives of the loss with respect to viewmatrix [4,4],
    projmatrix [4,4] and campos [3] -- taken as independent inputs, in their own (transposed, row-vector) layout -- from the
    per-Gaussian sums a backward has just written: dL_dmeans2D [P,3], dL_dconic [P,2,2] (rasterize_gaussians_backward's
    `_want_conic`) and dL_dcolors [P,3].  raw_params False: sh [P,M,3] (None / empty: precomputed colours, campos gets zeros),
    scales / rotations activated or cov3D_precomp; True: sh = features_dc, sh_rest = features_rest, scales / rotations the
    model's raw tensors.  geomBuffer: the forward's.  -> {name: tensor} for the names in `want` (a subset of CAMERA_GRADS).
    Two launches, no host wait; the workspace comes from torch's caching allocator per call.  Tensors are read in place: a
    host tensor, a wrong dtype or a non-contiguous tensor is refused."""
    want = _subset("camera_backward", "gradient", want, CAMERA_GRADS)
    if means3D.dim() != 2 or means3D.size(1) != 3:
        raise RuntimeError("camera_backward: means3D must have dimensions (num_points, 3)")
    dev = means3D.device
    if dev.type != "cuda":
        raise RuntimeError("camera_backward: means3D: the MI355X rasterizer needs device tensors (no CPU path)")
    P, H, W = int(means3D.size(0)), int(image_height), int(image_width)
    raw = bool(raw_params)
    m3 = _cam_tensor(means3D, dev, "means3D")
    vm, pm = _cam_tensor(viewmatrix, dev, "viewmatrix", 16), _cam_tensor(projmatrix, dev, "projmatrix", 16)
    cp = _cam_tensor(campos, dev, "campos", 3)
    shc, rest = _cam_tensor(sh, dev, "sh"), _cam_tensor(sh_rest, dev, "sh_rest")
    sc, rot = _cam_tensor(scales, dev, "scales", 3 * P), _cam_tensor(rotations, dev, "rotations", 4 * P)
    cov = _cam_tensor(cov3D_precomp, dev, "cov3D_precomp", 6 * P)
    deg, rad = _cam_tensor(degrees, dev, "degrees", P, torch.int32), _cam_tensor(radii, dev, "radii", P, torch.int32)
    g2 = _cam_tensor(dL_dmeans2D, dev, "dL_dmeans2D", 3 * P)
    gcon, gcol = _cam_tensor(dL_dconic, dev, "dL_dconic", 4 * P), _cam_tensor(dL_dcolors, dev, "dL_dcolors", 3 * P)
    geom = _cam_tensor(geomBuffer, dev, "geomBuffer", dtype=torch.uint8)
    if P and (vm is None or pm is None or cp is None):
        raise RuntimeError("camera_backward: viewmatrix, projmatrix and campos are needed")
    if shc is None:
        M = 0
    elif raw:
        if tuple(shc.shape) != (P, 1, 3):
            raise RuntimeError("camera_backward: features_dc must have dimensions (num_points, 1, 3)")
        M = 1 if rest is None else 1 + int(rest.size(1))
        if rest is not None and (rest.dim() != 3 or rest.size(0) != P or rest.size(2) != 3):
            raise RuntimeError("camera_backward: features_rest must have dimensions (num_points, M-1, 3)")
    else:
        if shc.dim() != 3 or shc.size(0) != P or shc.size(2) != 3:
            raise RuntimeError("camera_backward: sh must have dimensions (num_points, M, 3)")
        M = int(shc.size(1))
    out = {name: torch.empty(_CAMERA_GRAD_SHAPES[name], dtype=torch.float32, device=dev) for name in want}
    with _on_device(dev):
        work = _workspace("camera_backward", _lib.r3dgs_camera_backward_workspace_bytes(P), dev, False)   # (P == 0: no bytes)
        _check(_lib.r3dgs_camera_backward(
            P, _ptr(deg), M, W, H, _ptr(m3), _ptr(shc), _ptr(rest), _ptr(sc), float(scale_modifier), _ptr(rot), _ptr(cov), int(raw),
            _ptr(vm), _ptr(pm), _ptr(cp), float(tanfovx), float(tanfovy), _ptr(rad), _ptr(geom), _ptr(g2), _ptr(gcon), _ptr(gcol),
            *[_ptr(out.get(name)) for name in CAMERA_GRADS], work.data_ptr(), _stream()), "camera_backward")
    return out


CAMERA_MAP_GRADS = ("viewmatrix", "projmatrix")


def camera_backward_maps(means3D, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tanfovx, tanfovy,
                         image_height, image_width, radii, dL_dmeans2D=None, dL_dconic=None, dL_dz=None, want=CAMERA_MAP_GRADS):
    """r3dgs_camera_backward_maps (include/r3dgs_camera.h): the partial derivatives of a loss on the replay maps with respect to
    viewmatrix [4,4] and projmatrix [4,4] -- independent inputs, in their own (transposed, row-vector) layout -- from the
    per-Gaussian sums a _screen map backward has just written: dL_dmeans2D [P,3], dL_dconic [P,4] (A, B, -, C), dL_dz [P]
    (None = zero).  scales / rotations ACTIVATED, or cov3D_precomp.  -> {name: tensor} for the names in `want` (a subset of
    CAMERA_MAP_GRADS).  Two launches, no host wait; the workspace comes from torch's caching allocator per call.  Tensors are
    read in place: a host tensor, a wrong dtype or a non-contiguous tensor is refused."""
    want = _subset("camera_backward_maps", "gradient", want, CAMERA_MAP_GRADS)
    if means3D.dim() != 2 or means3D.size(1) != 3:
        raise RuntimeError("camera_backward_maps: means3D must have dimensions (num_points, 3)")
    dev = means3D.device
    if dev.type != "cuda":
        raise RuntimeError("camera_backward_maps: means3D: the MI355X rasterizer needs device tensors (no CPU path)")
    P, H, W = int(means3D.size(0)), int(image_height), int(image_width)

    def take(t, name, numel=None, dtype=torch.float32):
        try:
            return _cam_tensor(t, dev, name, numel, dtype)
        except RuntimeError as e:   # the refusals of camera_backward, under this call's name
            raise RuntimeError(str(e).replace("camera_backward:", "camera_backward_maps:", 1)) from None
    m3 = take(means3D, "means3D")
    vm, pm = take(viewmatrix, "viewmatrix", 16), take(projmatrix, "projmatrix", 16)
    sc, rot = take(scales, "scales", 3 * P), take(rotations, "rotations", 4 * P)
    cov = take(cov3D_precomp, "cov3D_precomp", 6 * P)
    rad = take(radii, "radii", P, torch.int32)
    g2, gcon, gz = take(dL_dmeans2D, "dL_dmeans2D", 3 * P), take(dL_dconic, "dL_dconic", 4 * P), take(dL_dz, "dL_dz", P)
    if P and (vm is None or pm is None):
        raise RuntimeError("camera_backward_maps: viewmatrix and projmatrix are needed")
    out = {name: torch.empty((4, 4), dtype=torch.float32, device=dev) for name in want}
    with _on_device(dev):
        work = _workspace("camera_backward_maps", _lib.r3dgs_camera_backward_maps_workspace_bytes(P), dev, False)
        _check(_lib.r3dgs_camera_backward_maps(
            P, W, H, _ptr(m3), _ptr(sc), float(scale_modifier), _ptr(rot), _ptr(cov), _ptr(vm), _ptr(pm), float(tanfovx),
            float(tanfovy), _ptr(rad), _ptr(g2), _ptr(gcon), _ptr(gz), *[_ptr(out.get(name)) for name in CAMERA_MAP_GRADS],
            work.data_ptr(), _stream()), "camera_backward_maps")
    return out


def set_sh_cache(on):
    """True (default): a backward without a sparsity term uses the SH direction derivatives the forward left instead of
    reading the SH tensor again; False: it reads the rows.  Same gradients, bit for bit.  Returns the previous setting."""
    return bool(_lib.r3dgs_set_sh_cache(int(bool(on))))


def sh_cache():
    return bool(_lib.r3dgs_set_sh_cache(-1))


def set_f64_chain(on):
    """True (default): the per-Gaussian backward evaluates the covariance chain (backward.cu:228-306, 311-374) in double and
    rounds once; False: in fp32, as the reference does.  Returns the previous setting."""
    return bool(_lib.r3dgs_set_f64_chain(int(bool(on))))


def f64_chain():
    return bool(_lib.r3dgs_set_f64_chain(-1))


def set_tile_order(on):
    """True (default): the backward blend starts its tiles heaviest first; False: row-major.  Same gradients, bit for bit.
    Returns the previous setting."""
    return bool(_lib.r3dgs_set_tile_order(int(bool(on))))


def tile_order():
    return bool(_lib.r3dgs_set_tile_order(-1))


def set_bwd_segments(on):
    """True (default): the backward blend walks a long tile list -- at least max(2 S, 75 % of the pass's mean list length)
    entries, S = 128 (R3DGS_BWD_SEG_LEN, R3DGS_BWD_SEG_FACTOR; include/r3dgs_rasterizer.h) -- in segments of S entries, several
    workgroups per tile, from checkpoints the forward leaves; False: one workgroup per tile.  Gradients agree to rounding (the state at a
    segment's end is the forward's running product instead of the backward's own division chain).  A forward issued while
    this is off leaves no checkpoints, and its backward never splits.  Returns the previous setting."""
    _need("bwd_segments")
    return bool(_lib.r3dgs_set_bwd_segments(int(bool(on))))


def bwd_segments():
    _need("bwd_segments")
    return bool(_lib.r3dgs_set_bwd_segments(-1))


def export_tile_order(H, W, imageBuffer, P=0, num_rendered=0, binningBuffer=None):
    """Debug accessor (not in the reference): quad_depth int32[tiles, 4] (deepest contributor of each 8x8 quadrant, left by
    the forward) and -- given the binning buffer, P and num_rendered of the pass -- the launch order of the last backward
    over this state: `lists`, eight dicts (tile, segment, segments int64 arrays and the unit `words` they were read from, each
    list heaviest first, and `walk`, the
    entries per list segment its units walk, 0 = whole tiles), and `units`, their concatenation."""
    n = ((W + 15) // 16) * ((H + 15) // 16)
    qd = torch.empty((n, 4), dtype=torch.int32, device=imageBuffer.device)
    out = dict(quad_depth=qd)
    order, R = None, 0
    if binningBuffer is not None and binningBuffer.numel():
        R = (num_rendered.capacity if isinstance(num_rendered, NumRendered) else
             _lib.r3dgs_binning_capacity(int(P), W, H, int(binningBuffer.numel())))
        _need("bwd_segments")
        cap = int(_lib.r3dgs_bwd_units_cap(R, W, H))
        order = torch.empty((cap + 2 * _ORDER_LISTS,), dtype=torch.int32, device=imageBuffer.device)
    with _on_device(imageBuffer.device):
        _check(_lib.r3dgs_export_tile_order(int(P), int(R), W, H, _ptr(binningBuffer) if order is not None else None,
                                            _ptr(imageBuffer), _ptr(qd), _ptr(order) if order is not None else None,
                                            _stream()), "export_tile_order")
    if order is not None:
        o = order.cpu().numpy().astype("int64") & 0xFFFFFFFF
        per = cap // _ORDER_LISTS
        lists = []
        for g in range(_ORDER_LISTS):   # list g: made from the 4 x 4 tile blocks g, g + 8, ...; consumed as entries b // 8 of list b % 8
            cnt, walk_log2 = int(o[cap + 2 * g]), int(o[cap + 2 * g + 1])
            u = o[g * per:g * per + cnt]
            lists.append(dict(unit_fields(u), words=u, walk=(1 << walk_log2) if walk_log2 else 0))
        out["lists"] = lists
        out["units"] = {k: np.concatenate([l[k] for l in lists]) for k in ("tile", "segment", "segments")}
    return out


_ORDER_LISTS = 8


def unit_fields(u):
    """The fields of unit words (csrc/unit_order.h unit_unpack; tests/test_unit_order_cpu.py holds the masks to the header)."""
    return dict(tile=u & 0xFFFFF, segment=(u >> 20) & 63, segments=u >> 26)


def rasterize_gaussians_counters(*args):
    """Forward in counter mode (calculate_mean_transmittance, forward.cu:560-564): same arguments as
    rasterize_gaussians; additionally returns (touched_pixels int32[P], transmittance fp32[P]).
    This is the building block of calculate_colours_variance (reduced_3dgs.cu:89-140)."""
    means3D = args[1]
    P = int(means3D.size(0))
    touched = torch.zeros((P,), dtype=torch.int32, device=means3D.device)
    transm = torch.zeros((P,), dtype=torch.float32, device=means3D.device)
    out = _forward_common(None, *args, counters=(touched, transm))
    return out + (touched, transm)


def calculate_colours_variance_partial(cam_positions, means3D, opacity, scales, rotations, cam_viewmatrices,
                                       cam_projmatrices, tan_fovxs, tan_fovys, image_height, image_width, sh, degrees,
                                       max_sh_deg):
    """The accumulation part of Reduced3DGS::calculateColourVariance (reduced_3dgs.cu:41-198) over the given cameras,
    WITHOUT the final divisions: (accum[P,max_sh_deg], wSum[P,1], mean[P,1,3], S[P,1,3]).  A camera-sharded run calls
    this per rank and merges the partials (multiview.merge_colour_variance)."""
    if means3D.dim() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    dev = means3D.device
    P = int(means3D.size(0))
    D = int(max_sh_deg)
    opts = dict(dtype=torch.float32, device=dev)
    accum = torch.zeros((P, D), **opts)
    wSum, wSumSq = torch.zeros((P, 1), **opts), torch.zeros((P, 1), **opts)
    mean, variance = torch.zeros((P, 1, 3), **opts), torch.zeros((P, 1, 3), **opts)
    if P:
        m3, shc, deg = _dev(means3D, dev), _dev(sh, dev), _dev(degrees, dev, torch.int32)
        M = int(shc.size(1))
        cams = _dev(cam_positions, dev)
        Hs, Ws = image_height.tolist(), image_width.tolist()
        txs, tys = tan_fovxs.tolist(), tan_fovys.tolist()
        bg = torch.zeros(3, **opts)
        empty = torch.Tensor([])
        for i in range(int(cams.size(0)) if cams is not None else 0):
            touched = torch.zeros((P,), dtype=torch.int32, device=dev)
            transm = torch.zeros((P,), **opts)
            out = _forward_common(None, bg, m3, empty, opacity, scales, rotations, 1.0, empty, cam_viewmatrices[i],
                                  cam_projmatrices[i], txs[i], tys[i], Hs[i], Ws[i], shc, deg, cams[i], False, False,
                                  counters=(touched, transm))
            radii = out[2]
            with _on_device(dev):
                _check(_lib.r3dgs_colour_variance_accumulate(P, _ptr(deg), M, D, _ptr(m3), cams[i].data_ptr(),
                                                             _ptr(shc), _ptr(radii), _ptr(touched), _ptr(transm),
                                                             _ptr(wSum), _ptr(wSumSq), _ptr(mean), _ptr(variance),
                                                             _ptr(accum), _stream()), "calculate_colours_variance")
    return accum, wSum, mean, variance


def calculate_colours_variance(cam_positions, means3D, opacity, scales, rotations, cam_viewmatrices, cam_projmatrices,
                               tan_fovxs, tan_fovys, image_height, image_width, sh, degrees, max_sh_deg):
    """Reduced3DGS::calculateColourVariance (reduced_3dgs.cu:41-203) ->
    (colourDistances[P,max_sh_deg], variance[P,1,3], mean[P,1,3]).  Per camera: the counter-mode forward
    (touched pixels + summed transmittance per Gaussian) followed by ONE fused per-Gaussian accumulate kernel,
    instead of the reference's ~25 small torch operators per camera.  The four per-camera parameter tensors are
    read back once (the reference does a blocking .item() per value and camera)."""
    accum, wSum, mean, variance = calculate_colours_variance_partial(
        cam_positions, means3D, opacity, scales, rotations, cam_viewmatrices, cam_projmatrices, tan_fovxs, tan_fovys,
        image_height, image_width, sh, degrees, max_sh_deg)
    return accum / wSum, variance / wSum.view(-1, 1, 1), mean


def _dev_u8(t, dev):
    if t.device != dev:
        raise RuntimeError("all tensors must live on the same GPU")
    if t.dtype == torch.bool:
        t = t.view(torch.uint8) if t.is_contiguous() else t.contiguous().view(torch.uint8)
    if t.dtype != torch.uint8:
        raise RuntimeError("expected a bool tensor")
    return t.contiguous()


def _need_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: tensors must be on a GPU (no CPU path)")
    return t.device


def find_minimum_projected_pixel_size(w2ndc_transforms, w2ndc_transforms_inverse, means3D, image_height, image_width):
    """Reduced3DGS::calculatePixelSize (reduced_3dgs.cu:240-264) -> pixel_values[P,1] (10000 where unseen).
    One launch for all cameras; the image sizes stay on the device."""
    dev = _need_gpu(means3D, "find_minimum_projected_pixel_size")
    P = int(means3D.size(0))
    out = torch.empty((P, 1), dtype=torch.float32, device=dev)
    if P:
        m, mi = _dev(w2ndc_transforms, dev), _dev(w2ndc_transforms_inverse, dev)
        Hs, Ws = _dev(image_height, dev, torch.int32), _dev(image_width, dev, torch.int32)
        with _on_device(dev):
            _check(_lib.r3dgs_min_pixel_size(P, int(w2ndc_transforms.size(0)), _ptr(m), _ptr(mi), _ptr(_dev(means3D, dev)),
                                             _ptr(Hs), _ptr(Ws), _ptr(out), _stream()),
                   "find_minimum_projected_pixel_size")
    return out


def sphere_ellipsoid_intersection(means3D, scales, rotations, neighbours_indices, sphere_radius, knn):
    """Reduced3DGS::intersectionTest (reduced_3dgs.cu:205-238) -> (redundancy_values int32[P,1],
    intersection_mask bool[P,knn])."""
    dev = _need_gpu(means3D, "sphere_ellipsoid_intersection")
    P, knn = int(means3D.size(0)), int(knn)
    red = torch.empty((P, 1), dtype=torch.int32, device=dev)
    mask = torch.empty((P, knn), dtype=torch.bool, device=dev)
    if P:
        nbr = _dev(neighbours_indices, dev, torch.int32)
        if nbr.numel() != P * knn:
            raise RuntimeError("neighbours_indices must hold P * knn entries")
        with _on_device(dev):
            _check(_lib.r3dgs_sphere_ellipsoid_intersection(
                P, knn, _ptr(_dev(means3D, dev)), _ptr(_dev(scales, dev)), _ptr(_dev(rotations, dev)),
                _ptr(nbr), _ptr(_dev(sphere_radius, dev)), _ptr(red), mask.data_ptr() if knn else None,
                _stream()), "sphere_ellipsoid_intersection")
    return red, mask


def allocate_minimum_redundancy_value(redundancy_values, neighbours_indices, intersection_mask, knn):
    """Reduced3DGS::assignFinalRedundancyValue (reduced_3dgs.cu:268-287) -> (minimum_redundancy_values int32[P,1],)."""
    dev = _need_gpu(redundancy_values, "allocate_minimum_redundancy_value")
    P, knn = int(redundancy_values.size(0)), int(knn)
    out = torch.empty((P, 1), dtype=torch.int32, device=dev)
    if P:
        nbr, msk = _dev(neighbours_indices, dev, torch.int32), _dev_u8(intersection_mask, dev)
        if nbr.numel() != P * knn or msk.numel() != P * knn:
            raise RuntimeError("neighbours_indices / intersection_mask must hold P * knn entries")
        with _on_device(dev):
            _check(_lib.r3dgs_min_redundancy(P, knn, _ptr(_dev(redundancy_values, dev, torch.int32)), _ptr(nbr), _ptr(msk),
                                             _ptr(out), _stream()), "allocate_minimum_redundancy_value")
    return (out,)


def kmeans_cuda(values, centers, tol, max_iterations, _want_iterations=False):
    """Reduced3DGS::kmeans (reduced_3dgs.cu:290-340) -> (ids int32[n,1], centers fp32[n_centers]).  Values sorted
    once, one binary-search pass per update; the whole Lloyd loop is enqueued at once with the convergence flag on
    the device (the reference scans all centres per value and reads the shift back every iteration)."""
    dev = _need_gpu(values, "kmeans_cuda")
    n, nc = int(values.size(0)), int(centers.size(0))
    ids = torch.zeros((n, 1), dtype=torch.int32, device=dev)
    new_centers = torch.empty((nc,), dtype=torch.float32, device=dev)
    iters = torch.zeros((1,), dtype=torch.int32, device=dev)
    with _on_device(dev):
        ws_bytes = _lib.r3dgs_kmeans_workspace_bytes(n, nc)
        if ws_bytes == 0:
            raise RuntimeError(f"kmeans_cuda: {_lib.r3dgs_last_error().decode()}")
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        _check(_lib.r3dgs_kmeans(n, nc, _ptr(_dev(values, dev)), _ptr(_dev(centers, dev)), float(tol),
                                 int(max_iterations), _ptr(ids), _ptr(new_centers), _ptr(iters), _ptr(ws),
                                 _stream()), "kmeans_cuda")
    if _want_iterations:
        return ids, new_centers, iters
    return ids, new_centers


def pack_view_stats(viewspace_grad, radii, grad_norm_out, visible_out, radii_out):
    """One launch for the per-view densification statistics of a view-parallel step (include/r3dgs_reduction.h
    r3dgs_pack_view_stats): ||viewspace_grad[:, :2]|| where radii > 0, the visibility indicator and a copy of radii,
    written into caller-provided (exchange-buffer) tensors."""
    dev = _need_gpu(viewspace_grad, "pack_view_stats")
    P = int(radii.numel())
    if P == 0:
        return
    vg, rd = _dev(viewspace_grad, dev), _dev(radii, dev, torch.int32)
    for t, dt in ((grad_norm_out, torch.float32), (visible_out, torch.float32), (radii_out, torch.int32)):
        if t.device != dev or t.dtype != dt or t.numel() != P or not t.is_contiguous():
            raise RuntimeError("pack_view_stats: outputs must be contiguous [P] tensors on the same GPU")
    with _on_device(dev):
        _check(_lib.r3dgs_pack_view_stats(P, _ptr(vg), _ptr(rd), _ptr(grad_norm_out), _ptr(visible_out), _ptr(radii_out),
                                          _stream()), "pack_view_stats")


def reduce_shards(recv, world, shard_begin, sum_len, out):
    """Local half of the view-parallel exchange (include/r3dgs_reduction.h r3dgs_reduce_shards): recv [world, shard]
    fp32 buffer whose tail (global element index >= sum_len) holds int32 radii -> out [shard]."""
    dev = _need_gpu(recv, "reduce_shards")
    shard = int(out.numel())
    if recv.numel() != world * shard or not recv.is_contiguous() or not out.is_contiguous():
        raise RuntimeError("reduce_shards: recv must be a contiguous [world, shard] buffer")
    with _on_device(dev):
        _check(_lib.r3dgs_reduce_shards(int(world), shard, int(shard_begin), int(sum_len), recv.data_ptr(),
                                        out.data_ptr(), _stream()), "reduce_shards")


def reduce_shards_mixed(recv, world, shard_begin, sum_len, half_end, out):
    """r3dgs_reduce_shards_mixed (include/r3dgs_reduction.h): as reduce_shards, with the words [sum_len, half_end) of the
    buffer holding bfloat16 pairs (fp32 accumulation in rank order, one rounding to nearest even)."""
    _need("reduce_shards_mixed")
    dev = _need_gpu(recv, "reduce_shards_mixed")
    shard = int(out.numel())
    if recv.numel() != world * shard or not recv.is_contiguous() or not out.is_contiguous():
        raise RuntimeError("reduce_shards_mixed: recv must be a contiguous [world, shard] buffer")
    with _on_device(dev):
        _check(_lib.r3dgs_reduce_shards_mixed(int(world), shard, int(shard_begin), int(sum_len), int(half_end),
                                              recv.data_ptr(), out.data_ptr(), _stream()), "reduce_shards_mixed")


# ---- fused L1 + D-SSIM training loss (include/r3dgs_loss.h, csrc/loss.hip); the autograd surface is r3dgs_loss.py.
# Inputs are checked there (device fp32, contiguous, same shape); these calls only allocate and launch, on the current
# stream, without a host synchronisation, so a forward + backward pair can be captured in a graph.

def ssim_window():
    """The 11 fp32 weights of the reference's 1-D SSIM window (utils/loss_utils.py:24-26), computed on the host."""
    _need("loss")
    w = (C.c_float * 11)()
    _lib.r3dgs_ssim_window(w)
    return np.array(w[:], np.float32)


def _loss_scratch(what, nbytes, dev):
    """The scratch tensor of a loss call whose size query said `nbytes`; 0 refuses `what`, "<call>: invalid <size>"."""
    if nbytes == 0:
        raise RuntimeError(what)
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev)


def l1_ssim_forward(img1, img2, B, Cc, H, W, lambda_dssim, want_partials, want_map):
    """-> (l1, ssim, loss, dssim, ssim_image[B], ssim_map or empty, partials[3,B,C,H,W] or empty); 0-d tensors for the
    scalars.  One tile kernel + one fixed-order reduction."""
    _need("loss")
    if _ext is not None:
        return _ext.l1_ssim_forward(img1, img2, B, Cc, H, W, float(lambda_dssim), bool(want_partials), bool(want_map))
    dev = img1.device
    f32 = dict(dtype=torch.float32, device=dev)
    l1, ssim, loss, dssim = (torch.empty((), **f32) for _ in range(4))
    per_image = torch.empty((B,), **f32)
    ssim_map = torch.empty((B, Cc, H, W), **f32) if want_map else _NO_TENSOR
    partials = torch.empty((3, B, Cc, H, W), **f32) if want_partials else _NO_TENSOR
    with _on_device(dev):
        ws = _loss_scratch(f"l1_ssim_forward: invalid shape {B}x{Cc}x{H}x{W}",
                           _lib.r3dgs_l1_ssim_workspace_bytes(B, Cc, H, W), dev)
        _check(_lib.r3dgs_l1_ssim_forward(B, Cc, H, W, _ptr(img1), _ptr(img2), float(lambda_dssim), _ptr(l1), _ptr(ssim),
                                          _ptr(per_image), _ptr(loss), _ptr(dssim), _ptr(ssim_map), _ptr(partials),
                                          _ptr(ws), _stream()), "l1_ssim_forward")
    return l1, ssim, loss, dssim, per_image, ssim_map, partials


def l1_ssim_backward(img1, img2, partials, grad_l1, coef_l1, grad_ssim, ssim_grad_mode, coef_ssim, B, Cc, H, W):
    """-> d/d img1 [B,C,H,W] (r3dgs_l1_ssim_backward).  grad_l1 / grad_ssim: device tensors (empty: absent);
    ssim_grad_mode 0: scalar upstream of the mean, 1: per image [B], 2: per pixel [B,C,H,W]."""
    _need("loss")
    if _ext is not None:
        return _ext.l1_ssim_backward(img1, img2, partials, grad_l1, float(coef_l1), grad_ssim, int(ssim_grad_mode),
                                     float(coef_ssim), B, Cc, H, W)
    dev = img1.device
    dx = torch.empty((B, Cc, H, W), dtype=torch.float32, device=dev)
    with _on_device(dev):
        _check(_lib.r3dgs_l1_ssim_backward(B, Cc, H, W, _ptr(img1), _ptr(img2), _ptr(partials), _ptr(grad_l1),
                                           float(coef_l1), _ptr(grad_ssim), int(ssim_grad_mode), float(coef_ssim), _ptr(dx),
                                           _stream()), "l1_ssim_backward")
    return dx


def l1_forward(x, y):
    """mean |x - y| over all elements (0-d tensor): one chunk kernel + the fixed-order reduction."""
    _need("loss")
    if _ext is not None:
        return _ext.l1_forward(x, y)
    dev = x.device
    n = x.numel()
    out = torch.empty((), dtype=torch.float32, device=dev)
    with _on_device(dev):
        ws = _loss_scratch(f"l1_forward: invalid element count {n}", _lib.r3dgs_l1_workspace_bytes(n), dev)
        _check(_lib.r3dgs_l1_forward(n, _ptr(x), _ptr(y), _ptr(out), _ptr(ws), _stream()), "l1_forward")
    return out


def l1_backward(x, y, grad):
    """grad[0] * sign(x - y) / n, shaped like x."""
    _need("loss")
    if _ext is not None:
        return _ext.l1_backward(x, y, grad)
    dev = x.device
    dx = torch.empty_like(x)
    with _on_device(dev):
        _check(_lib.r3dgs_l1_backward(x.numel(), _ptr(x), _ptr(y), _ptr(grad), _ptr(dx), _stream()), "l1_backward")
    return dx


# ---- the same loss behind a per-image exposure and a pixel mask (include/r3dgs_loss.h r3dgs_exposure_*, csrc/loss.hip); the
# autograd surface is r3dgs_exposure.py, which checks the inputs.  exposure / mask: device tensors, empty for an absent one;
# exposure [B,3,4] or [3,4], mask [B,H,W] or [H,W] in memory (per image: the leading B).

def has_exposure_loss():
    """Whether the loaded library has the exposure loss (r3dgs_exposure_loss_forward)."""
    return not any(name in _missing_rows for name in _OPTIONAL_ROWS["exposure"][1])


def exposure_loss_workspace_bytes(B, Cc, H, W):
    """r3dgs_exposure_loss_workspace_bytes: 0 for an invalid shape."""
    _need_rows("exposure")
    return int(_lib.r3dgs_exposure_loss_workspace_bytes(int(B), int(Cc), int(H), int(W)))


def exposure_loss_forward(img1, img2, exposure, exposure_per_image, mask, mask_per_image, mask_target, B, Cc, H, W,
                          lambda_dssim, want_partials, _workspace=None):
    """-> (l1, ssim, loss, dssim, ssim_image[B], partials[3,B,C,H,W] or empty); 0-d tensors for the scalars.  One tile kernel
    + the fixed-order reduction.  _workspace (tests): a uint8 device tensor to use instead of this call's own."""
    _need_rows("exposure")
    if _ext is not None and _workspace is None:
        return _ext.exposure_loss_forward(img1, img2, _t(exposure), bool(exposure_per_image), _t(mask), bool(mask_per_image),
                                          bool(mask_target), B, Cc, H, W, float(lambda_dssim), bool(want_partials))
    dev = img1.device
    f32 = dict(dtype=torch.float32, device=dev)
    l1, ssim, loss, dssim = (torch.empty((), **f32) for _ in range(4))
    per_image = torch.empty((B,), **f32)
    partials = torch.empty((3, B, Cc, H, W), **f32) if want_partials else _NO_TENSOR
    with _on_device(dev):
        ws = _workspace
        if ws is None:
            ws = _loss_scratch(f"exposure_loss_forward: invalid shape {B}x{Cc}x{H}x{W}",
                               _lib.r3dgs_exposure_loss_workspace_bytes(B, Cc, H, W), dev)
        _check(_lib.r3dgs_exposure_loss_forward(B, Cc, H, W, _ptr(img1), _ptr(img2), _ptr(exposure), int(exposure_per_image),
                                                _ptr(mask), int(mask_per_image), int(mask_target), float(lambda_dssim),
                                                _ptr(l1), _ptr(ssim), _ptr(per_image), _ptr(loss), _ptr(dssim), _ptr(partials),
                                                _ptr(ws), ws.numel(), _stream()), "exposure_loss_forward")
    return l1, ssim, loss, dssim, per_image, partials


def exposure_loss_backward(img1, img2, exposure, exposure_per_image, mask, mask_per_image, mask_target, partials, grad_loss,
                           coef_l1, coef_ssim, want_exposure_grad, B, Cc, H, W, _workspace=None):
    """-> (d/d img1 [B,C,H,W], d/d exposure shaped like `exposure` or empty) (r3dgs_exposure_loss_backward)."""
    _need_rows("exposure")
    if _ext is not None and _workspace is None:
        return _ext.exposure_loss_backward(img1, img2, _t(exposure), bool(exposure_per_image), _t(mask), bool(mask_per_image),
                                           bool(mask_target), partials, grad_loss, float(coef_l1), float(coef_ssim),
                                           bool(want_exposure_grad), B, Cc, H, W)
    dev = img1.device
    f32 = dict(dtype=torch.float32, device=dev)
    dx = torch.empty((B, Cc, H, W), **f32)
    dE = torch.empty((B, 3, 4) if exposure_per_image else (3, 4), **f32) if want_exposure_grad else _NO_TENSOR
    with _on_device(dev):
        ws = _workspace
        if ws is None:
            ws = _loss_scratch(f"exposure_loss_backward: invalid shape {B}x{Cc}x{H}x{W}",
                               _lib.r3dgs_exposure_loss_workspace_bytes(B, Cc, H, W), dev)
        _check(_lib.r3dgs_exposure_loss_backward(B, Cc, H, W, _ptr(img1), _ptr(img2), _ptr(exposure), int(exposure_per_image),
                                                 _ptr(mask), int(mask_per_image), int(mask_target), _ptr(partials),
                                                 _ptr(grad_loss), float(coef_l1), float(coef_ssim), _ptr(dx), _ptr(dE),
                                                 _ptr(ws), ws.numel(), _stream()), "exposure_loss_backward")
    return dx, dE


def exposure_apply(img, exposure, exposure_per_image, clamp01, B, H, W):
    """-> clamp?(x E[:, :3] + E[:, 3]) [B,3,H,W] (r3dgs_exposure_apply)."""
    _need_rows("exposure")
    if _ext is not None:
        return _ext.exposure_apply(img, exposure, bool(exposure_per_image), bool(clamp01), B, H, W)
    dev = img.device
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    with _on_device(dev):
        _check(_lib.r3dgs_exposure_apply(B, H, W, _ptr(img), _ptr(exposure), int(exposure_per_image), int(clamp01), _ptr(out),
                                         _stream()), "exposure_apply")
    return out


# ---- fused Adam step (include/r3dgs_optim.h, csrc/optim.hip); the optimizer is r3dgs_optim.Adam, which checks the tensors
# (one device, fp32, contiguous, matching sizes) and computes the scalars.  One launch per 32 tensors on the current stream,
# no host synchronisation.

def _adam_segments(params, grads, exp_avgs, exp_avg_sqs, scalars):
    segs = (_AdamSegment * len(params))()
    for i, (p, g, m, v) in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs)):
        segs[i] = _AdamSegment(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), *scalars[6 * i:6 * i + 6])
    return segs


def _adam_capturable_segments(params, grads, exp_avgs, exp_avg_sqs, steps, lrs, scalars):
    segs = (_AdamCapturableSegment * len(params))()
    for i, (p, g, m, v, step, lr) in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs, steps, lrs)):
        segs[i] = _AdamCapturableSegment(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr(), _ptr(lr),
                                         p.numel(), *scalars[4 * i:4 * i + 4])
    return segs


def _adam(what, fn, pack, per, lists, scalars, radii=None):
    """The ctypes route of the four adam_step* functions: `pack` makes the segments of entry point `fn` from the tensor lists
    and `per` scalars per tensor; radii: the gated forms' tail (row lengths, radii, P)."""
    params, n = lists[0], len(lists[0])
    if any(len(l) != n for l in lists) or len(scalars) != per * n:
        raise RuntimeError(f"{what}: list lengths differ")
    if n == 0:
        return None
    tail = ()
    if radii is not None:
        P = radii.numel()
        tail = ((_i * n)(*_row_lens(params, P, what)), _ptr(radii), P)
    segs = pack(*lists, scalars)
    with _on_device(params[0].device):
        _check(fn(n, segs, *tail, _stream()), what)
    return None


def _row_lens(params, P, what):
    """Floats per Gaussian of each [P, ...] tensor (the C ABI checks n == P * row_len again)."""
    out = []
    for t in params:
        if t.dim() < 1 or t.shape[0] != P:
            raise RuntimeError(f"{what}: a tensor of shape {tuple(t.shape)} is not [P, ...] with P = {P}")
        out.append(t.numel() // P if P else 1)
    return out


def adam_step(params, grads, exp_avgs, exp_avg_sqs, scalars):
    """One Adam step of the tensors (lists of equal length, params[0]'s device).  scalars: a flat list of six Python floats
    per tensor -- 1 - beta1, beta2, 1 - beta2, bc2_sqrt, eps, step_size (r3dgs_adam_segment) -- each rounded to fp32 once."""
    _need("adam")
    if _ext is not None:
        return _ext.adam_step(params, grads, exp_avgs, exp_avg_sqs, scalars)
    return _adam("adam_step", _lib.r3dgs_adam_step, _adam_segments, 6, (params, grads, exp_avgs, exp_avg_sqs), scalars)


def adam_step_capturable(params, grads, exp_avgs, exp_avg_sqs, steps, lrs, scalars):
    """The capturable step: steps[i] a device float32 count (read + 1, then bumped), lrs[i] a 0-d device float32 lr or an
    empty tensor; scalars: a flat list of lr_value, beta1, beta2, eps per tensor (r3dgs_adam_capturable_segment)."""
    _need("adam")
    if _ext is not None:
        return _ext.adam_step_capturable(params, grads, exp_avgs, exp_avg_sqs, steps, lrs, scalars)
    return _adam("adam_step_capturable", _lib.r3dgs_adam_step_capturable, _adam_capturable_segments, 4,
                 (params, grads, exp_avgs, exp_avg_sqs, steps, lrs), scalars)


def adam_step_visible(params, grads, exp_avgs, exp_avg_sqs, scalars, radii):
    """adam_step for the Gaussians with radii > 0 only (radii: the rasterizer's device int32 [P]; every tensor [P, ...]).
    The rows of the others keep their bits and their gradients are not looked at (r3dgs_adam_step_visible)."""
    _need("adam_visible")
    if _ext is not None:
        return _ext.adam_step_visible(params, grads, exp_avgs, exp_avg_sqs, scalars, radii)
    return _adam("adam_step_visible", _lib.r3dgs_adam_step_visible, _adam_segments, 6, (params, grads, exp_avgs, exp_avg_sqs),
                 scalars, radii)


def adam_step_capturable_visible(params, grads, exp_avgs, exp_avg_sqs, steps, lrs, scalars, radii):
    """adam_step_capturable for the Gaussians with radii > 0 only; radii is read at replay, like steps and lrs."""
    _need("adam_visible")
    if _ext is not None:
        return _ext.adam_step_capturable_visible(params, grads, exp_avgs, exp_avg_sqs, steps, lrs, scalars, radii)
    return _adam("adam_step_capturable_visible", _lib.r3dgs_adam_step_capturable_visible, _adam_capturable_segments, 4,
                 (params, grads, exp_avgs, exp_avg_sqs, steps, lrs), scalars, radii)


# ---- per-iteration training statistics (include/r3dgs_trainstats.h, csrc/train_stats.hip); the surface is r3dgs_train_stats.py,
# which checks the tensors (one device, dtypes, shapes, contiguity).  These calls only allocate and launch, on the current
# stream, without a host synchronisation, so they can be captured in a graph.

def visible_means(radii, opacity, features_rest):
    """-> (visibility bool[P], n_visible int32 0-d, alpha_mean fp32 0-d or None, sh_abs_mean fp32 0-d or None) of
    r3dgs_visible_means.  opacity: raw fp32 [P] / [P,1] or None; features_rest: fp32 [P,M-1,3] or None (M - 1 may be 0: the mean
    of nothing, NaN).  P == 0 gives n_visible = 0 and NaN means without a launch."""
    _need("train_stats")
    dev = _need_gpu(radii, "visible_means")
    P = int(radii.numel())
    M = 1 if features_rest is None else int(features_rest.size(1)) + 1
    if _ext is not None:
        vis, n, alpha, sh = _ext.visible_means(radii, _t(opacity), _t(features_rest), opacity is not None, features_rest is not None, M)
        return vis, n, (None if opacity is None else alpha), (None if features_rest is None else sh)
    f32 = dict(dtype=torch.float32, device=dev)
    vis = torch.empty((P,), dtype=torch.bool, device=dev)
    if P == 0:
        nan = torch.full((), float("nan"), **f32)
        return (vis, torch.zeros((), dtype=torch.int32, device=dev), None if opacity is None else nan,
                None if features_rest is None else nan.clone())
    n = torch.empty((), dtype=torch.int32, device=dev)
    alpha = None if opacity is None else torch.empty((), **f32)
    sh = None if features_rest is None else torch.empty((), **f32)
    with _on_device(dev):
        ws = torch.empty((_lib.r3dgs_train_stats_workspace_bytes(P),), dtype=torch.uint8, device=dev)
        _check(_lib.r3dgs_visible_means(P, M, radii.data_ptr(), _ptr(opacity), _ptr(features_rest), vis.data_ptr(), n.data_ptr(),
                                        _ptr(alpha), _ptr(sh), ws.data_ptr(), _stream()), "visible_means")
    return vis, n, alpha, sh


def alpha_regul_backward(radii, opacity, upstream, n_visible, grad):
    """grad[i] += upstream * (radii[i] > 0) * sigmoid'(opacity[i]) / n_visible, in place (r3dgs_alpha_regul_backward);
    upstream, n_visible: 0-d device tensors."""
    _need("train_stats")
    dev = _need_gpu(radii, "alpha_regul_backward")
    if _ext is not None:
        return _ext.alpha_regul_backward(radii, opacity, upstream, n_visible, grad)
    P = int(radii.numel())
    if P:
        with _on_device(dev):
            _check(_lib.r3dgs_alpha_regul_backward(P, radii.data_ptr(), opacity.data_ptr(), upstream.data_ptr(),
                                                   n_visible.data_ptr(), grad.data_ptr(), _stream()), "alpha_regul_backward")
    return None


def densification_stats(viewspace_grad, radii, xyz_gradient_accum, denom, max_radii2D):
    """train.py:134 and gaussian_model.py:693-695 in one launch, in place on the three accumulators
    (r3dgs_densification_stats)."""
    _need("train_stats")
    dev = _need_gpu(radii, "densification_stats")
    if _ext is not None:
        return _ext.densification_stats(viewspace_grad, radii, xyz_gradient_accum, denom, max_radii2D)
    P = int(radii.numel())
    if P:
        with _on_device(dev):
            _check(_lib.r3dgs_densification_stats(P, viewspace_grad.data_ptr(), radii.data_ptr(), xyz_gradient_accum.data_ptr(),
                                                  denom.data_ptr(), max_radii2D.data_ptr(), _stream()), "densification_stats")
    return None


# ---- evaluation metrics (include/r3dgs_metrics.h, csrc/metrics.hip); the surface is r3dgs_metrics.py, which checks the
# tensors (device, dtypes, shapes, contiguity).  These calls only launch, on the current stream, into tensors the caller
# owns, without a host synchronisation, so they can be captured in a graph.  ctypes only: two launches per view.

GT_F32_CHW, GT_U8_CHW, GT_U8_HWC = 0, 1, 2      # R3DGS_GT_*
METRICS_CLAMP, METRICS_QUANTISE8 = 1, 2         # R3DGS_METRICS_*
METRICS_ROW = 9                                 # R3DGS_METRICS_ROW


def image_metrics_workspace_bytes(Cc, H, W):
    """Bytes of device scratch r3dgs_image_metrics needs for a [C,H,W] image (0: a shape it refuses)."""
    _need("metrics")
    return int(_lib.r3dgs_image_metrics_workspace_bytes(Cc, H, W))


def image_metrics(image, gt, gt_layout, flags, row, workspace):
    """Writes the float64 row [METRICS_ROW] of image [C,H,W] against gt (r3dgs_image_metrics); workspace: uint8 tensor of
    image_metrics_workspace_bytes(C, H, W) bytes."""
    _need("metrics")
    Cc, H, W = image.shape
    with _on_device(image.device):
        _check(_lib.r3dgs_image_metrics(Cc, H, W, image.data_ptr(), gt.data_ptr(), int(gt_layout), int(flags), row.data_ptr(),
                                        workspace.data_ptr(), _stream()), "image_metrics")
    return row


def row_mse(a, b, rows):
    """-> float64 [rows]: the mean squared error of each of the `rows` equal contiguous slices of a and b (r3dgs_row_mse)."""
    _need("metrics")
    dev = a.device
    n = a.numel() // rows
    out = torch.empty((rows,), dtype=torch.float64, device=dev)
    with _on_device(dev):
        ws_bytes = _lib.r3dgs_row_mse_workspace_bytes(rows, n)
        if ws_bytes == 0:
            raise RuntimeError(f"row_mse: invalid shape, {rows} rows of {n}")
        ws = torch.empty((ws_bytes // 8,), dtype=torch.float64, device=dev)
        _check(_lib.r3dgs_row_mse(rows, n, a.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), _stream()), "row_mse")
    return out


def image_to_uint8(image):
    """-> uint8 [H,W,C] of image [C,H,W]: save_image's 8-bit rounding (r3dgs_image_to_uint8)."""
    _need("metrics")
    Cc, H, W = image.shape
    out = torch.empty((H, W, Cc), dtype=torch.uint8, device=image.device)
    with _on_device(image.device):
        _check(_lib.r3dgs_image_to_uint8(Cc, H, W, image.data_ptr(), out.data_ptr(), _stream()), "image_to_uint8")
    return out
