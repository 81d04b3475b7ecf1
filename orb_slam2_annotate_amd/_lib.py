"""Loader of liborbfe.so (the HIP/gfx950 product library) and its ctypes prototypes.

There is no CPU fallback: if the library is missing the import fails loudly, and every
compute entry point returns ORBFE_ERR_HIP on a machine without a gfx950 device.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
import os as _os

# $ORBFE_LIB: an alternative build of the library (A/B runs of compile-time variants, tools/ab_build.sh); default in-tree
LIB_PATH = Path(_os.environ["ORBFE_LIB"]) if _os.environ.get("ORBFE_LIB") else PKG_DIR / "liborbfe.so"

KFDB_RELOC, KFDB_LOOP = 0, 1  # orbfe_kfdb_group_candidates modes
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28

STAGES = ["h2d", "pyramid", "fast", "octree", "blur", "orient_desc", "d2h", "match"]
ORBFE_OK, ERR_INVALID, ERR_CAPACITY, ERR_HIP, ERR_NOMEM = 0, -1, -2, -3, -4
DEBUG_STREAM_H2D, DEBUG_STREAM_D2H = -1, -2  # orbfe_debug_stall_extractor_stream: the pipelined path's copy streams


class OrbfeError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"liborbfe error {code}: {msg}")
        self.code = code


class FrameViewC(C.Structure):
    _fields_ = [("n", C.c_int32), ("x", C.c_void_p), ("y", C.c_void_p), ("octave", C.c_void_p),
                ("angle", C.c_void_p), ("u_right", C.c_void_p), ("desc", C.c_void_p),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("resident", C.c_void_p)]


class Sim3LegC(C.Structure):
    """orbfe_sim3_leg: one direction of one SearchBySim3 candidate (src/ORBmatcher.cc:1251-1477)."""
    _fields_ = [("Rw", C.c_float * 9), ("tw", C.c_float * 3), ("sR", C.c_float * 9), ("t", C.c_float * 3),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("log_scale_factor", C.c_float), ("n_levels", C.c_int32)]


class CameraPoseC(C.Structure):
    """orbfe_camera_pose: what Frame::isInFrustum reads of the Frame (src/Frame.cc:292-353)."""
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("mbf", C.c_float),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("log_scale_factor", C.c_float), ("n_levels", C.c_int32)]


class PoseOptStatsC(C.Structure):
    """orbfe_poseopt_stats."""
    _fields_ = [("rounds", C.c_int32), ("iterations", C.c_int32 * 4), ("trials", C.c_int32 * 4),
                ("lam", C.c_double * 4), ("chi2", C.c_double * 4)]


class LbaStatsC(C.Structure):
    """orbfe_lba_stats."""
    _fields_ = [("rounds", C.c_int32), ("stopped", C.c_int32), ("host_syncs", C.c_int32), ("n_level1", C.c_int32),
                ("iterations", C.c_int32 * 2), ("trials", C.c_int32 * 2), ("termination", C.c_int32 * 2),
                ("lam", C.c_double * 2), ("chi2", C.c_double * 2)]


class EssGraphStatsC(C.Structure):
    """orbfe_essgraph_stats."""
    _fields_ = [("iterations", C.c_int32), ("trials", C.c_int32), ("termination", C.c_int32), ("stopped", C.c_int32),
                ("host_syncs", C.c_int32), ("n_free", C.c_int32), ("blocks_A", C.c_int32), ("blocks_L", C.c_int32),
                ("solve_failures", C.c_int32), ("lam", C.c_double), ("chi2_initial", C.c_double), ("chi2", C.c_double)]


class OptSim3StatsC(C.Structure):
    """orbfe_optsim3_stats."""
    _fields_ = [("rounds", C.c_int32), ("n_bad", C.c_int32), ("iterations", C.c_int32 * 2), ("trials", C.c_int32 * 2),
                ("lam", C.c_double * 2), ("chi2", C.c_double * 2)]


class KeyFrameCameraC(C.Structure):
    """orbfe_keyframe_camera: what LocalMapping::CreateNewMapPoints reads of a key frame besides its keypoints."""
    _fields_ = [("Tcw", C.c_float * 12), ("Ow", C.c_float * 3),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("invfx", C.c_float), ("invfy", C.c_float), ("mb", C.c_float), ("mbf", C.c_float),
                ("depth", C.c_void_p), ("x_raw", C.c_void_p), ("y_raw", C.c_void_p)]


class FeatVecC(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("node_ids", C.c_void_p), ("offsets", C.c_void_p),
                ("indices", C.c_void_p)]


# every symbol include/orbfe.h declares (tests/test_cabi_symbols.py checks the header against this)
EXPORTS = [
    "orbfe_last_error", "orbfe_device_count", "orbfe_extractor_create", "orbfe_extractor_destroy",
    "orbfe_extractor_get_levels", "orbfe_extractor_get_scale_factor", "orbfe_extractor_get_scale_factors",
    "orbfe_extractor_get_inverse_scale_factors", "orbfe_extractor_get_scale_sigma_squares",
    "orbfe_extractor_get_inverse_scale_sigma_squares", "orbfe_extractor_get_features_per_level",
    "orbfe_extractor_get_umax", "orbfe_extractor_max_keypoints", "orbfe_extractor_max_keypoints_for", "orbfe_extract", "orbfe_extract_batch",
    "orbfe_extract_batch_device", "orbfe_extract_batch_device_async", "orbfe_extract_batch_pipelined", "orbfe_host_alloc", "orbfe_host_free", "orbfe_extract_stereo_frame", "orbfe_extractor_synchronize", "orbfe_extractor_level_size", "orbfe_extractor_get_pyramid_level",
    "orbfe_extractor_pyramid_level_device", "orbfe_extractor_debug_candidates",
    "orbfe_extractor_debug_blurred_level", "orbfe_extractor_debug_host_octree", "orbfe_debug_octree_host", "orbfe_debug_octree_device", "orbfe_debug_octree_carve", "orbfe_debug_geometry",
    "orbfe_debug_resize_tables", "orbfe_debug_resize_tiles", "orbfe_extractor_set_streams", "orbfe_extractor_set_fused", "orbfe_extractor_set_pyramid_blur", "orbfe_extractor_set_pyramid_chain", "orbfe_set_blur_pass_order", "orbfe_extractor_set_fast_mode", "orbfe_extractor_set_schedule", "orbfe_extractor_set_desc_tiles", "orbfe_extractor_set_blur_spec", "orbfe_gaussian_blur7_spec", "orbfe_extractor_profile", "orbfe_extractor_profile_get",
    "orbfe_stage_name", "orbfe_resize_linear", "orbfe_gaussian_blur7", "orbfe_descriptor_distance",
    "orbfe_hamming_matrix", "orbfe_search_by_bow", "orbfe_search_by_bow_kf",
    "orbfe_search_for_triangulation", "orbfe_frame_upload", "orbfe_frame_release", "orbfe_frame_get_view", "orbfe_search_by_bow_resident", "orbfe_search_by_bow_kf_resident", "orbfe_search_for_triangulation_multi", "orbfe_fuse_search_multi", "orbfe_search_by_bow_multi", "orbfe_search_by_bow_kf_multi", "orbfe_search_by_projection_keyframe_multi", "orbfe_frame_from_extractor", "orbfe_frame_from_device", "orbfe_frame_set_featvec", "orbfe_compute_stereo_matches", "orbfe_stereo_match_batch_device", "orbfe_vocabulary_load_text", "orbfe_vocabulary_create", "orbfe_vocabulary_destroy",
    "orbfe_vocabulary_info", "orbfe_vocabulary_transform", "orbfe_vocabulary_featvec_batch_device",
    "orbfe_bow_match_consecutive_batch_device", "orbfe_bow_match_consecutive_batch_device_async", "orbfe_bow_match_consecutive_stereo_batch_device_async", "orbfe_cvt_gray", "orbfe_cvt_gray_batch_device",
    "orbfe_distinctive_descriptors", "orbfe_features_in_area", "orbfe_search_by_projection",
    "orbfe_search_by_projection_last_frame", "orbfe_search_by_projection_keyframe",
    "orbfe_search_by_projection_sim3", "orbfe_search_for_initialization", "orbfe_debug_last_claim_rounds", "orbfe_fuse_search", "orbfe_search_by_sim3",
    "orbfe_init_undistort_rectify_map", "orbfe_rectifier_create", "orbfe_rectifier_destroy", "orbfe_remap", "orbfe_remap_batch_device", "orbfe_extract_stereo_rectified_batch_device_async",
    "orbfe_undistort_points", "orbfe_undistort_keypoints_batch_device", "orbfe_compute_image_bounds",
    "orbfe_stereo_from_rgbd", "orbfe_frame_synchronize", "orbfe_debug_stall_extractor_stream", "orbfe_debug_extractor_stream_idle",
    "orbfe_debug_stall_thread_stream", "orbfe_debug_thread_stream_idle",
    "orbfe_vocabulary_transform_bow", "orbfe_kfdb_create", "orbfe_kfdb_destroy", "orbfe_kfdb_add", "orbfe_kfdb_erase",
    "orbfe_kfdb_clear", "orbfe_kfdb_size", "orbfe_kfdb_query", "orbfe_kfdb_score", "orbfe_kfdb_group_candidates",
    "orbfe_mappoints_create", "orbfe_mappoints_destroy", "orbfe_mappoints_capacity", "orbfe_mappoints_update",
    "orbfe_project_in_frustum", "orbfe_search_local_points",
    "orbfe_pose_optimization", "orbfe_pose_optimization_batch", "orbfe_pose_optimization_mappoints",
    "orbfe_triangulate_matches", "orbfe_triangulate_matches_multi",
    "orbfe_sim3_ransac", "orbfe_sim3_ransac_multi", "orbfe_sim3_triples_from_draws", "orbfe_sim3_max_iterations",
    "orbfe_pnp_ransac", "orbfe_pnp_ransac_multi", "orbfe_pnp_refine_multi", "orbfe_pnp_solve_multi", "orbfe_pnp_sets_from_draws",
    "orbfe_optimize_sim3", "orbfe_optimize_sim3_multi",
    "orbfe_local_bundle_adjustment", "orbfe_bundle_adjustment", "orbfe_local_bundle_adjustment_mappoints",
    "orbfe_optimize_essential_graph", "orbfe_essential_graph_correct_points", "orbfe_essential_graph_correct_mappoints",
    "orbfe_block_sparse_solve7", "orbfe_mappoints_positions",
    "orbfe_initializer_ransac", "orbfe_initializer_ransac_multi", "orbfe_initializer_normalize", "orbfe_initializer_sets_from_draws",
    "orbfe_initializer_reconstruct", "orbfe_initializer_reconstruct_multi",
    "orbfe_obsgraph_create", "orbfe_obsgraph_destroy", "orbfe_obsgraph_clear", "orbfe_obsgraph_set_keyframes",
    "orbfe_obsgraph_set_points", "orbfe_obsgraph_add_observations", "orbfe_obsgraph_erase_observations",
    "orbfe_obsgraph_erase_keyframe", "orbfe_obsgraph_get_row", "orbfe_obsgraph_votes", "orbfe_obsgraph_culling_counts",
    "orbfe_obsgraph_update_normal_depth", "orbfe_obsgraph_update_normal_depth_mappoints",
    "orbfe_obsgraph_update_connections", "orbfe_obsgraph_local_keyframes",
    "orbfe_obsgraph_enable_keyframe_points", "orbfe_obsgraph_set_keyframe_points", "orbfe_obsgraph_assign_keyframe_points",
    "orbfe_obsgraph_get_keyframe_points", "orbfe_obsgraph_keyframe_points_union", "orbfe_obsgraph_tracked_points",
    "orbfe_obsgraph_enable_keyframe_descriptors", "orbfe_obsgraph_set_keyframe_descriptors",
    "orbfe_obsgraph_set_keyframe_descriptors_frame", "orbfe_obsgraph_get_keyframe_descriptors",
    "orbfe_obsgraph_distinctive_descriptors", "orbfe_obsgraph_distinctive_descriptors_mappoints", "orbfe_mappoints_descriptors",
    "orbfe_project_fuse", "orbfe_fuse_mappoints",
    "orbfe_project_last_frame", "orbfe_search_last_frame_mappoints", "orbfe_project_keyframe",
    "orbfe_search_keyframe_mappoints_multi",
    "orbfe_project_sim3", "orbfe_search_by_sim3_mappoints_multi", "orbfe_search_by_projection_sim3_mappoints",
    "orbfe_correct_loop_sim3s", "orbfe_correct_loop_points", "orbfe_correct_loop_mappoints",
    "orbfe_gba_propagate_keyframes", "orbfe_gba_update_points", "orbfe_gba_update_mappoints",
    "orbfe_stereo_points_select", "orbfe_count_close_points", "orbfe_create_stereo_points",
    "orbfe_triangulated_points_select", "orbfe_create_triangulated_points",
]

_lib = None


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's).  Two HIP/HSA
    runtimes in one process cannot both own the GPU, so when torch is installed but not imported
    yet, its runtime is loaded first and liborbfe.so binds to it by SONAME -- `import torch` then
    works in either order.  No torch module is imported here; without torch this is a no-op."""
    import importlib.util
    import os
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    hip = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(hip):
        try:
            C.CDLL(hip, mode=C.RTLD_GLOBAL)
        except OSError:
            pass  # fall back to the system runtime


def load():
    """Load liborbfe.so; raises (never falls back) when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    _share_hip_runtime_with_torch()
    L = C.CDLL(str(LIB_PATH))
    L.orbfe_last_error.restype = C.c_char_p
    L.orbfe_stage_name.restype = C.c_char_p
    L.orbfe_extractor_get_scale_factor.restype = C.c_float
    L.orbfe_extractor_create.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(C.c_void_p)]
    L.orbfe_extractor_destroy.argtypes = [C.c_void_p]
    L.orbfe_extractor_destroy.restype = None
    vp, ci, cf, cs = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    L.orbfe_extractor_get_levels.argtypes = [vp]
    L.orbfe_extractor_get_scale_factor.argtypes = [vp]
    for n in ("scale_factors", "inverse_scale_factors", "scale_sigma_squares", "inverse_scale_sigma_squares",
              "features_per_level", "umax"):
        getattr(L, f"orbfe_extractor_get_{n}").argtypes = [vp, vp]
    L.orbfe_extractor_max_keypoints.argtypes = [vp]
    L.orbfe_extract.argtypes = [vp, vp, ci, ci, ci, vp, vp, ci, vp]
    L.orbfe_extract_batch.argtypes = [vp, vp, ci, ci, ci, ci, cs, vp, vp, ci, vp]
    L.orbfe_extract_batch_device.argtypes = [vp, vp, ci, ci, ci, ci, cs, vp, vp, ci, vp]
    L.orbfe_extract_batch_pipelined.argtypes = [vp, vp, ci, ci, ci, ci, cs, vp, vp, ci, vp, ci]
    L.orbfe_host_alloc.argtypes = [C.POINTER(vp), cs]
    L.orbfe_host_free.argtypes = [vp]
    L.orbfe_host_free.restype = None
    L.orbfe_extract_batch_device_async.argtypes = [vp, vp, ci, ci, ci, ci, cs, vp, vp, ci, vp]
    L.orbfe_extractor_synchronize.argtypes = [vp]
    L.orbfe_extractor_level_size.argtypes = [vp, ci, ci, ci, vp, vp]
    L.orbfe_extractor_get_pyramid_level.argtypes = [vp, ci, ci, vp, ci]
    L.orbfe_extractor_pyramid_level_device.argtypes = [vp, ci, ci, vp, vp, vp, vp]
    L.orbfe_extractor_debug_candidates.argtypes = [vp, ci, ci, vp, vp, vp, ci]
    L.orbfe_extractor_debug_blurred_level.argtypes = [vp, ci, ci, vp, ci]
    L.orbfe_extractor_profile.argtypes = [vp, ci]
    L.orbfe_extractor_debug_host_octree.argtypes = [vp, ci]
    L.orbfe_extractor_profile_get.argtypes = [vp, vp, vp, vp]
    L.orbfe_extractor_set_streams.argtypes = [vp, ci]
    L.orbfe_stage_name.argtypes = [ci]
    L.orbfe_resize_linear.argtypes = [ci, vp, ci, ci, ci, vp, ci, ci, ci]
    L.orbfe_gaussian_blur7.argtypes = [ci, vp, ci, ci, ci, vp, ci]
    L.orbfe_descriptor_distance.argtypes = [ci, vp, vp, ci, vp]
    L.orbfe_hamming_matrix.argtypes = [ci, vp, ci, vp, ci, vp]
    fvp = C.POINTER(FeatVecC)
    L.orbfe_search_by_bow.argtypes = [ci, vp, vp, vp, ci, fvp, vp, vp, ci, fvp, cf, ci, vp]
    L.orbfe_search_by_bow_kf.argtypes = [ci, vp, vp, vp, ci, fvp, vp, vp, vp, ci, fvp, cf, ci, vp]
    L.orbfe_search_for_triangulation.argtypes = [ci, vp, vp, vp, vp, vp, vp, ci, fvp, vp, vp, vp, vp, vp, vp, vp,
                                                 ci, fvp, vp, cf, cf, vp, vp, ci, ci, ci, vp]
    L.orbfe_compute_stereo_matches.argtypes = [vp, ci, vp, ci, vp, vp, ci, vp, vp, ci, cf, cf, vp, vp]
    L.orbfe_extract_stereo_frame.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, ci, cf, cf, vp, vp]
    L.orbfe_stereo_match_batch_device.argtypes = [vp, ci, vp, vp, vp, ci, cf, cf, vp, vp, vp]
    L.orbfe_vocabulary_load_text.argtypes = [C.c_char_p, ci, C.POINTER(C.c_void_p)]
    L.orbfe_vocabulary_create.argtypes = [ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, C.POINTER(C.c_void_p)]
    L.orbfe_vocabulary_destroy.argtypes = [vp]
    L.orbfe_vocabulary_destroy.restype = None
    L.orbfe_vocabulary_info.argtypes = [vp, vp, vp, vp, vp]
    L.orbfe_vocabulary_transform.argtypes = [vp, vp, ci, ci, vp, vp, vp]
    L.orbfe_vocabulary_featvec_batch_device.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp]
    L.orbfe_bow_match_consecutive_batch_device.argtypes = [vp, ci, vp, vp, vp, ci, ci, cf, ci, vp, vp]
    L.orbfe_bow_match_consecutive_batch_device_async.argtypes = [vp, vp, ci, vp, vp, vp, ci, ci, cf, ci, vp, vp]
    L.orbfe_cvt_gray.argtypes = [ci, vp, ci, ci, ci, ci, ci, vp, ci]
    L.orbfe_cvt_gray_batch_device.argtypes = [ci, vp, ci, ci, ci, ci, cs, ci, ci, vp, ci, cs]
    L.orbfe_distinctive_descriptors.argtypes = [ci, vp, vp, ci, vp]
    fwp = C.POINTER(FrameViewC)
    L.orbfe_features_in_area.argtypes = [ci, fwp, ci, vp, vp, vp, vp, vp, ci, vp, vp]
    L.orbfe_search_by_projection.argtypes = [ci, fwp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, cf, cf, vp, vp]
    L.orbfe_search_by_projection_last_frame.argtypes = [ci, fwp, vp, ci, cf, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                        ci, cf, ci, vp, vp]
    L.orbfe_search_by_projection_keyframe.argtypes = [ci, fwp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, cf, ci, ci, vp, vp]
    L.orbfe_search_by_projection_sim3.argtypes = [ci, fwp, vp, ci, vp, ci, vp, vp, vp, vp, vp, cf, vp, vp]
    L.orbfe_set_blur_pass_order.argtypes = [ci]
    L.orbfe_set_blur_pass_order.restype = ci
    L.orbfe_debug_last_claim_rounds.argtypes = []
    L.orbfe_debug_last_claim_rounds.restype = ci
    L.orbfe_search_for_initialization.argtypes = [ci, fwp, fwp, vp, vp, ci, cf, ci, vp, vp]
    L.orbfe_fuse_search.argtypes = [ci, fwp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, cf, ci, vp]
    L.orbfe_search_by_sim3.argtypes = [ci, fwp, fwp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, cf, vp, vp]
    L.orbfe_frame_upload.argtypes = [ci, fwp, vp, C.POINTER(C.c_void_p)]
    L.orbfe_frame_release.argtypes = [vp]
    L.orbfe_frame_release.restype = None
    L.orbfe_frame_get_view.argtypes = [vp]
    L.orbfe_frame_get_view.restype = fwp
    L.orbfe_search_by_bow_resident.argtypes = [vp, vp, vp, cf, ci, vp]
    L.orbfe_search_by_bow_kf_resident.argtypes = [vp, vp, vp, vp, cf, ci, vp]
    L.orbfe_search_for_triangulation_multi.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, vp]
    L.orbfe_fuse_search_multi.argtypes = [ci, ci, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, cf, ci, vp]
    L.orbfe_search_by_bow_multi.argtypes = [ci, vp, vp, vp, cf, ci, vp, vp]
    L.orbfe_search_by_bow_kf_multi.argtypes = [vp, vp, ci, vp, vp, cf, ci, vp, vp]
    L.orbfe_search_by_projection_keyframe_multi.argtypes = [ci, fwp, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp]
    L.orbfe_frame_from_extractor.argtypes = [vp, ci, fwp, vp, ci, C.POINTER(C.c_void_p)]
    L.orbfe_frame_from_device.argtypes = [ci, vp, vp, fwp, vp, ci, C.POINTER(C.c_void_p)]
    L.orbfe_frame_set_featvec.argtypes = [vp, vp]
    L.orbfe_frame_synchronize.argtypes = [vp]
    L.orbfe_debug_stall_extractor_stream.argtypes = [vp, ci, ci]
    L.orbfe_debug_extractor_stream_idle.argtypes = [vp, ci]
    L.orbfe_debug_stall_thread_stream.argtypes = [ci, ci]
    L.orbfe_debug_thread_stream_idle.argtypes = [ci]
    L.orbfe_init_undistort_rectify_map.argtypes = [ci, vp, vp, ci, vp, vp, ci, ci, vp, vp]
    L.orbfe_rectifier_create.argtypes = [ci, vp, vp, ci, ci, ci, C.POINTER(C.c_void_p)]
    L.orbfe_rectifier_destroy.argtypes = [vp]
    L.orbfe_rectifier_destroy.restype = None
    L.orbfe_remap.argtypes = [vp, vp, ci, ci, ci, vp, ci]
    L.orbfe_remap_batch_device.argtypes = [vp, vp, ci, ci, ci, ci, cs, vp, ci, cs]
    L.orbfe_extract_stereo_rectified_batch_device_async.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, cs, vp, vp, vp, ci, vp]
    L.orbfe_bow_match_consecutive_stereo_batch_device_async.argtypes = [vp, vp, ci, vp, vp, vp, ci, ci, cf, ci, vp, vp]
    L.orbfe_undistort_points.argtypes = [ci, vp, ci, vp, vp, ci, vp]
    L.orbfe_undistort_keypoints_batch_device.argtypes = [ci, vp, vp, ci, ci, vp, vp, ci, vp]
    L.orbfe_compute_image_bounds.argtypes = [ci, ci, ci, vp, vp, ci, vp]
    L.orbfe_stereo_from_rgbd.argtypes = [ci, vp, vp, vp, ci, vp, ci, ci, ci, cf, vp, vp]
    L.orbfe_extractor_max_keypoints_for.argtypes = [vp, ci, ci]
    L.orbfe_debug_octree_host.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, ci]
    L.orbfe_debug_octree_device.argtypes = [ci, ci, ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp]
    L.orbfe_debug_octree_carve.argtypes = [ci, ci, vp]
    L.orbfe_debug_geometry.argtypes = [ci, cf, ci, ci, ci, ci, ci, vp, vp, vp, ci]
    L.orbfe_debug_resize_tables.argtypes = [ci, ci, ci, ci, vp, vp, vp, vp]
    L.orbfe_debug_resize_tiles.argtypes = [ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]
    i64 = C.c_int64
    L.orbfe_vocabulary_transform_bow.argtypes = [vp, vp, ci, ci, vp, vp, ci, vp]
    L.orbfe_kfdb_create.argtypes = [ci, ci, C.POINTER(C.c_void_p)]
    L.orbfe_kfdb_destroy.argtypes = [vp]
    L.orbfe_kfdb_destroy.restype = None
    L.orbfe_kfdb_add.argtypes = [vp, i64, vp, vp, ci]
    L.orbfe_kfdb_erase.argtypes = [vp, i64]
    L.orbfe_kfdb_clear.argtypes = [vp]
    L.orbfe_kfdb_size.argtypes = [vp]
    L.orbfe_kfdb_query.argtypes = [vp, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp]
    L.orbfe_kfdb_score.argtypes = [vp, vp, vp, ci, ci, vp, vp]
    L.orbfe_kfdb_group_candidates.argtypes = [ci, cf, ci, vp, vp, vp, vp, vp, vp, ci, vp]
    cpp = C.POINTER(CameraPoseC)
    L.orbfe_mappoints_create.argtypes = [ci, ci, C.POINTER(C.c_void_p)]
    L.orbfe_mappoints_destroy.argtypes = [vp]
    L.orbfe_mappoints_destroy.restype = None
    L.orbfe_mappoints_capacity.argtypes = [vp]
    L.orbfe_mappoints_update.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp]
    L.orbfe_project_in_frustum.argtypes = [vp, ci, vp, vp, cpp, cf, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbfe_search_local_points.argtypes = [vp, ci, vp, vp, cpp, cf, fwp, vp, ci, vp, cf, cf, vp, vp, vp]
    L.orbfe_pose_optimization.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbfe_pose_optimization_batch.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbfe_pose_optimization_mappoints.argtypes = [vp, ci, vp, fwp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp]
    kcp = C.POINTER(KeyFrameCameraC)
    L.orbfe_triangulate_matches_multi.argtypes = [ci, fwp, kcp, ci, vp, kcp, vp, vp, vp, ci, cf, vp, vp, vp, vp]
    L.orbfe_triangulate_matches.argtypes = [ci, fwp, kcp, fwp, kcp, vp, vp, vp, ci, cf, vp, vp, vp]
    L.orbfe_sim3_ransac_multi.argtypes = [ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp]
    L.orbfe_optimize_sim3_multi.argtypes = [ci, ci] + [vp] * 18
    L.orbfe_local_bundle_adjustment.argtypes = [ci, ci, ci, vp, vp, vp, ci, vp, ci] + [vp] * 13
    L.orbfe_bundle_adjustment.argtypes = [ci, ci, ci, vp, vp, vp, ci, vp, ci] + [vp] * 6 + [ci, ci] + [vp] * 5
    L.orbfe_local_bundle_adjustment_mappoints.argtypes = [vp, ci, vp, ci, ci, vp, vp, vp, ci] + [vp] * 13
    L.orbfe_optimize_essential_graph.argtypes = [ci, ci, vp, vp, vp, ci, vp, vp, vp, ci, ci, vp, vp, vp, vp]
    L.orbfe_essential_graph_correct_points.argtypes = [ci, ci, vp, vp, ci, vp, vp, vp]
    L.orbfe_essential_graph_correct_mappoints.argtypes = [vp, ci, vp, vp, ci, vp, vp]
    L.orbfe_block_sparse_solve7.argtypes = [ci, ci] + [vp] * 7
    L.orbfe_mappoints_positions.argtypes = [vp, ci, vp, vp]
    L.orbfe_optimize_sim3.argtypes = [ci, ci] + [vp] * 9 + [C.c_float, ci] + [vp] * 6
    L.orbfe_sim3_ransac.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp]
    L.orbfe_sim3_triples_from_draws.argtypes = [ci, ci, vp, vp]
    L.orbfe_pnp_ransac_multi.argtypes = [ci, ci, ci, ci] + [vp] * 12
    L.orbfe_pnp_ransac.argtypes = [ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp]
    L.orbfe_pnp_refine_multi.argtypes = [ci, ci, ci, ci] + [vp] * 12
    L.orbfe_pnp_solve_multi.argtypes = [ci, ci, ci, ci] + [vp] * 20
    L.orbfe_pnp_sets_from_draws.argtypes = [ci, ci, vp, vp]
    L.orbfe_sim3_max_iterations.argtypes = [ci, C.c_double, ci, ci]
    L.orbfe_initializer_ransac_multi.argtypes = [ci, ci, ci, ci] + [vp] * 14
    L.orbfe_initializer_ransac.argtypes = [ci, ci, vp, vp, vp, C.c_float, ci] + [vp] * 7
    L.orbfe_initializer_normalize.argtypes = [ci, vp, vp]
    L.orbfe_initializer_sets_from_draws.argtypes = [ci, ci, vp, vp]
    L.orbfe_initializer_reconstruct_multi.argtypes = [ci, ci, ci, ci] + [vp] * 19
    L.orbfe_initializer_reconstruct.argtypes = [ci, ci, vp, ci, vp, vp, C.c_float, vp] + [vp] * 9
    L.orbfe_obsgraph_create.argtypes = [ci, ci, ci, ci, C.POINTER(C.c_void_p)]
    L.orbfe_obsgraph_destroy.argtypes = [vp]
    L.orbfe_obsgraph_destroy.restype = None
    L.orbfe_obsgraph_clear.argtypes = [vp]
    L.orbfe_obsgraph_set_keyframes.argtypes = [vp, ci, vp, vp, vp, vp]
    L.orbfe_obsgraph_set_points.argtypes = [vp, ci, vp, vp, vp]
    L.orbfe_obsgraph_add_observations.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    L.orbfe_obsgraph_erase_observations.argtypes = [vp, ci, vp, vp, vp]
    L.orbfe_obsgraph_erase_keyframe.argtypes = [vp, ci, vp, ci, vp]
    L.orbfe_obsgraph_get_row.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp]
    L.orbfe_obsgraph_votes.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp]
    L.orbfe_obsgraph_culling_counts.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp]
    L.orbfe_obsgraph_update_normal_depth.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp, vp]
    L.orbfe_obsgraph_update_normal_depth_mappoints.argtypes = [vp, vp, ci, vp, vp, ci, vp]
    L.orbfe_obsgraph_update_connections.argtypes = [ci] + [vp] * 9
    L.orbfe_obsgraph_local_keyframes.argtypes = [ci] + [vp] * 10 + [vp, ci, vp, vp]
    L.orbfe_obsgraph_enable_keyframe_points.argtypes = [vp, ci]
    L.orbfe_obsgraph_set_keyframe_points.argtypes = [vp, ci, ci, vp]
    L.orbfe_obsgraph_assign_keyframe_points.argtypes = [vp, ci, vp, vp, vp]
    L.orbfe_obsgraph_get_keyframe_points.argtypes = [vp, ci, ci, vp, vp]
    L.orbfe_obsgraph_keyframe_points_union.argtypes = [vp, ci, vp, vp, ci, vp, vp]
    L.orbfe_obsgraph_tracked_points.argtypes = [vp, ci, vp, ci, vp]
    L.orbfe_obsgraph_enable_keyframe_descriptors.argtypes = [vp, ci]
    L.orbfe_obsgraph_set_keyframe_descriptors.argtypes = [vp, ci, ci, vp]
    L.orbfe_obsgraph_set_keyframe_descriptors_frame.argtypes = [vp, ci, vp]
    L.orbfe_obsgraph_get_keyframe_descriptors.argtypes = [vp, ci, vp, vp]
    L.orbfe_obsgraph_distinctive_descriptors.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    L.orbfe_obsgraph_distinctive_descriptors_mappoints.argtypes = [vp, vp, ci, vp, vp, vp, vp]
    L.orbfe_mappoints_descriptors.argtypes = [vp, ci, vp, vp]
    L.orbfe_project_fuse.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbfe_fuse_mappoints.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, ci, cf, ci, vp, vp]
    L.orbfe_project_last_frame.argtypes = [vp, ci, vp, vp, vp, cpp, vp, ci, cf, ci, vp, vp, vp, vp, vp, vp]
    L.orbfe_search_last_frame_mappoints.argtypes = [vp, ci, vp, vp, vp, vp, cpp, fwp, vp, ci, vp, ci, cf, ci, vp, vp, vp]
    L.orbfe_project_keyframe.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbfe_search_keyframe_mappoints_multi.argtypes = [vp, fwp, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp]
    L.orbfe_project_sim3.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbfe_search_by_sim3_mappoints_multi.argtypes = [vp, vp, fwp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, cf, vp, vp]
    L.orbfe_search_by_projection_sim3_mappoints.argtypes = [vp, ci, vp, vp, cpp, fwp, vp, ci, vp, cf, vp, vp, vp]
    L.orbfe_correct_loop_sim3s.argtypes = [ci, vp, vp, ci, vp, vp, vp, vp]
    L.orbfe_correct_loop_points.argtypes = [ci, vp, vp, vp, vp, ci, vp, vp, vp, vp]
    L.orbfe_correct_loop_mappoints.argtypes = [vp, vp, ci, vp, vp, vp, vp, ci, vp, vp, ci, ci, vp, vp, vp, vp]
    L.orbfe_gba_propagate_keyframes.argtypes = [ci, ci] + [vp] * 10
    L.orbfe_gba_update_points.argtypes = [ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp]
    L.orbfe_gba_update_mappoints.argtypes = [vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp]
    L.orbfe_stereo_points_select.argtypes = [ci, vp, vp, vp, vp, vp, vp, cpp, cf, ci, vp, ci, vp, ci] + [vp] * 8
    L.orbfe_count_close_points.argtypes = [ci, vp, vp, vp, cf, vp, vp]
    L.orbfe_create_stereo_points.argtypes = [vp, vp, vp, ci, cpp, ci, vp, vp, vp, cf, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp]
    L.orbfe_triangulated_points_select.argtypes = [ci, ci, vp, vp, vp, i64, vp, vp, vp, vp, vp, ci, ci] + [vp] * 9
    L.orbfe_create_triangulated_points.argtypes = [vp, vp, vp, ci, kcp, ci, vp, vp, kcp, vp, vp, vp, ci, cf, vp, ci] + [vp] * 7
    _lib = L
    return L


def check(rc: int) -> int:
    if rc < 0:
        raise OrbfeError(rc, load().orbfe_last_error().decode("utf-8", "replace"))
    return rc


def ptr(a):
    if a is None:
        return None
    return a.ctypes.data_as(C.c_void_p)
