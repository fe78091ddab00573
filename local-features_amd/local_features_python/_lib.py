"""ctypes binding of liblf_mkd.so (include/lf_mkd.h).  No fallback: if the HIP library is
missing or no gfx950 device is visible, construction raises."""
import ctypes
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
LIB_PATH = os.environ.get("LF_MKD_LIB", os.path.join(_ROOT, "liblf_mkd.so"))   # override: A/B builds
MODEL_DIR = os.path.join(_ROOT, "models", "mkd")

FLAG_KERNEL_TIMING = 1
FLAG_UNFUSED_KEYPOINTS = 2
FLAG_DETECT_STEPWISE = 4
VERIFY_NO_REFINE = 1     # lf_mkd_verify_homography* / _fundamental*: the best RANSAC candidate as is, no least-squares refit
MATCH_MUTUAL = 1         # lf_mkd_match_pairs_device: keep a match only if the other direction agrees
GUIDE_HOMOGRAPHY, GUIDE_FUNDAMENTAL = 0, 1   # lf_mkd_match_guided_pairs_device: what the pair's nine model floats are
ANGLE_SHADER, ANGLE_EXACT, ANGLE_EXACT_ZERO = 0, 1, 2
POOL_DEFAULT, POOL_F16X3, POOL_F32, POOL_F16_FP6 = 0, 1, 2, 3   # lf_mkd_pool_mode; the default is the f16x3 split
PCA_NAMES = ("liberty", "notredame", "yosemite")   # enum MKDPCA, lib.rs:26-32

# every symbol include/lf_mkd.h declares
SYMBOLS = (
    "lf_mkd_create", "lf_mkd_create_from_file", "lf_mkd_destroy", "lf_mkd_last_error",
    "lf_mkd_describe_patches", "lf_mkd_describe_patches_device", "lf_mkd_raw_descriptors_device",
    "lf_mkd_set_image", "lf_mkd_set_image_device", "lf_mkd_set_images_device", "lf_mkd_describe_keypoints",
    "lf_mkd_set_image_u8", "lf_mkd_set_images_u8_device", "lf_mkd_detect_u8", "lf_mkd_detect_times",
    "lf_mkd_describe_keypoints_frames_device",
    "lf_mkd_describe_keypoints_device", "lf_mkd_sample_patches_device", "lf_mkd_get_pyramid_level",
    "lf_mkd_get_pyramid_level_apron",
    "lf_mkd_build_constants", "lf_mkd_kernel_times", "lf_mkd_kernel_clock", "lf_mkd_synchronize", "lf_mkd_version",
    "lf_mkd_orient_keypoints", "lf_mkd_orient_keypoints_device", "lf_mkd_get_coarse_layer",
    "lf_mkd_detect_extrema", "lf_mkd_detect_extrema_device", "lf_mkd_filter_extrema_device", "lf_mkd_detect",
    "lf_mkd_match", "lf_mkd_match_device", "lf_mkd_match_both_device", "lf_mkd_match_pairs_device", "lf_mkd_match_guided_pairs_device", "lf_mkd_match_overflowed", "lf_mkd_stream_create", "lf_mkd_stream_frame",
    "lf_mkd_detect_frames_device", "lf_mkd_orient_keypoints_blocked",
    "lf_mkd_comm_unique_id", "lf_mkd_comm_create", "lf_mkd_comm_destroy", "lf_mkd_comm_info", "lf_mkd_allgather_descriptors",
    "lf_mkd_comm_loopback", "lf_mkd_comm_last_form", "lf_mkd_plan_upload", "lf_mkd_detect_recordings",
    "lf_mkd_verify_homography", "lf_mkd_verify_homography_device",
    "lf_mkd_verify_fundamental", "lf_mkd_verify_fundamental_device",
    "lf_mkd_quantize_descriptors", "lf_mkd_quantize_descriptors_device", "lf_mkd_match_q8", "lf_mkd_match_q8_device",
    "lf_mkd_match_q8_plan", "lf_mkd_match_q8_pairs_device", "lf_mkd_match_q8_guided_pairs_device", "lf_mkd_match_q8_pairs_plan",
    "lf_mkd_knn_q8", "lf_mkd_knn_q8_device", "lf_mkd_knn_q8_plan",
    "lf_mkd_match_q8_grouped", "lf_mkd_match_q8_grouped_device", "lf_mkd_match_q8_grouped_plan", "lf_mkd_vote_groups_device",
    "lf_mkd_edge_layout_device", "lf_mkd_gather_edge_rows_device", "lf_mkd_match_q8_edges_device",
    "lf_mkd_build_tracks_device",
    "lf_mkd_track_table_plan", "lf_mkd_track_table_device", "lf_mkd_gather_track_rows_device",
    "lf_mkd_link_table_plan", "lf_mkd_link_table_device",
    "lf_mkd_select_edges_plan", "lf_mkd_select_edges_device",
    "lf_mkd_covisibility_plan", "lf_mkd_covisibility_device",
    "lf_mkd_two_view_pose", "lf_mkd_two_view_pose_device",
    "lf_mkd_triangulate_tracks", "lf_mkd_triangulate_tracks_device",
    "lf_mkd_resect_camera", "lf_mkd_resect_cameras_device",
    "lf_mkd_track_descriptors", "lf_mkd_track_descriptors_device",
    "lf_mkd_bundle_adjust", "lf_mkd_bundle_adjust_device",
    "lf_mkd_bundle_adjust_intrinsics", "lf_mkd_bundle_adjust_intrinsics_device",
    "lf_mkd_view_graph_plan", "lf_mkd_view_graph", "lf_mkd_view_graph_device",
    "lf_mkd_tree_poses", "lf_mkd_tree_poses_device",
    "lf_mkd_global_positions_plan", "lf_mkd_global_positions", "lf_mkd_global_positions_device",
)
Q8_SCALE = 256.0         # the default scale of the 8-bit descriptors (lf_mkd.h: byte = clamp(rint(x * scale), -127, 127) + 128)
KNN_MAX = 16             # LF_MKD_KNN_MAX: the largest k of lf_mkd_knn_q8_device
TRACKS_ACCUMULATE = 1    # LF_MKD_TRACKS_ACCUMULATE: lf_mkd_build_tracks_device adds its links to the forest d_track holds
TRACKS_DUP_TILE = 256    # LF_MKD_TRACKS_DUP_TILE: rows one workgroup of its d_track_dup launch owns
TRACK_TABLE_CONSISTENT = 1   # LF_MKD_TRACK_TABLE_CONSISTENT: lf_mkd_track_table_device takes only tracks with dup == 0
LINK_TABLE_LOCAL = 1     # LF_MKD_LINK_TABLE_LOCAL: lf_mkd_link_table_device writes rows local to their images, not pool rows
SELECT_SKIP_SELF = 1     # LF_MKD_SELECT_SKIP_SELF: lf_mkd_select_edges_device does not offer column i to row i
SELECT_UNIQUE = 2        # LF_MKD_SELECT_UNIQUE: one pool, every unordered pair at most once, as (smaller, larger)
COVIS_ACCUMULATE = 1     # LF_MKD_COVIS_ACCUMULATE: lf_mkd_covisibility_device adds to what d_covis holds
BA_REFINE_FOCAL = 1      # LF_MKD_BA_REFINE_FOCAL: lf_mkd_bundle_adjust_intrinsics_device refines the groups' focal scale
BA_REFINE_PRINCIPAL = 2  # LF_MKD_BA_REFINE_PRINCIPAL: ... and the groups' principal-point shift
RESECT_ALL = 1           # LF_MKD_RESECT_ALL: lf_mkd_resect_cameras_device resects registered images too
VIEW_GRAPH_USE_UNCHECKED = 1     # LF_MKD_VIEW_GRAPH_USE_UNCHECKED: lf_mkd_view_graph_device keeps edges that close no triangle
VIEW_GRAPH_AUTO_ROOT = 0xFFFFFFFF    # LF_MKD_VIEW_GRAPH_AUTO_ROOT: its root is the image with the most kept incident edges
GLOBAL_POSITIONS_MAX_SWEEPS = 4096   # LF_MKD_GLOBAL_POSITIONS_MAX_SWEEPS: the largest sweeps of lf_mkd_global_positions_device
COVIS_FORM_LDS = 256     # LF_MKD_COVIS_FORM_LDS: in covisibility_plan's form, workgroups count in LDS first
SELECT_MAX_K = 32        # LF_MKD_SELECT_MAX_K: the largest k of lf_mkd_select_edges_device
COMM_ID_BYTES = 128
GATHER_DIRECT, GATHER_RING = 0, 1


class Params(ctypes.Structure):
    _fields_ = [
        ("max_image_width", ctypes.c_uint32), ("max_image_height", ctypes.c_uint32),
        ("max_features", ctypes.c_uint32), ("patch_scale_factor", ctypes.c_float),
        ("device", ctypes.c_int32), ("angle_mode", ctypes.c_int32), ("pool_mode", ctypes.c_int32),
        ("flags", ctypes.c_uint32), ("max_frames", ctypes.c_uint32), ("n_scales", ctypes.c_uint32),
        ("max_blobs", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 1),
    ]


KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4")])

_lib = None


def model_path(pca):
    if pca not in PCA_NAMES:
        raise RuntimeError("Invalid PCA argument")   # python/src/lib.rs:60-64
    return os.path.join(MODEL_DIR, f"concat-pca-{pca}.safetensors")


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not built: run `make -C local-features_amd` "
                           "(or __graft_entry__.build()); there is no CPU fallback")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64/libhsa-runtime64, and a
    # process that loads the system copy first and torch's second ends up with two HSA runtimes (torch
    # then sees no device).  Callers hand us torch device pointers and streams, so let torch load its
    # runtime first; liblf_mkd.so's libamdhip64.so.7 dependency then binds to the copy already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    L.lf_mkd_version.restype = ctypes.c_char_p
    L.lf_mkd_last_error.restype = ctypes.c_char_p
    L.lf_mkd_last_error.argtypes = [vp]
    L.lf_mkd_create.argtypes = [ctypes.POINTER(Params), vp, vp, vp, ctypes.POINTER(vp)]
    L.lf_mkd_create_from_file.argtypes = [ctypes.POINTER(Params), ctypes.c_char_p, ctypes.POINTER(vp)]
    L.lf_mkd_destroy.argtypes = [vp]
    L.lf_mkd_destroy.restype = None
    L.lf_mkd_describe_patches.argtypes = [vp, vp, u64, vp]
    L.lf_mkd_describe_patches_device.argtypes = [vp, vp, u64, vp, vp]
    L.lf_mkd_raw_descriptors_device.argtypes = [vp, vp, u64, vp, vp]
    L.lf_mkd_set_image.argtypes = [vp, vp, u32, u32]
    L.lf_mkd_set_image_device.argtypes = [vp, vp, u32, u32, vp]
    L.lf_mkd_set_images_device.argtypes = [vp, vp, u32, u32, u32, vp]
    L.lf_mkd_set_image_u8.argtypes = [vp, vp, u32, u32]
    L.lf_mkd_set_images_u8_device.argtypes = [vp, vp, u32, u32, u32, vp]
    L.lf_mkd_describe_keypoints_frames_device.argtypes = [vp, vp, vp, u64, vp, vp]
    L.lf_mkd_describe_keypoints.argtypes = [vp, vp, u64, vp]
    L.lf_mkd_describe_keypoints_device.argtypes = [vp, vp, u64, vp, vp]
    L.lf_mkd_sample_patches_device.argtypes = [vp, vp, u64, vp, vp]
    L.lf_mkd_get_pyramid_level.argtypes = [vp, u32, vp, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.lf_mkd_get_pyramid_level_apron.argtypes = [vp, u32, vp, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.lf_mkd_kernel_clock.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.lf_mkd_synchronize.argtypes = [vp]
    L.lf_mkd_orient_keypoints.argtypes = [vp, vp, u64, vp, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.lf_mkd_orient_keypoints_device.argtypes = [vp, vp, vp, u64, vp, vp, u64, ctypes.POINTER(u64),
                                                 ctypes.POINTER(u64), vp]
    L.lf_mkd_get_coarse_layer.argtypes = [vp, u32, vp]
    pu64 = ctypes.POINTER(u64)
    L.lf_mkd_detect_extrema.argtypes = [vp, vp, u64, pu64, pu64]
    L.lf_mkd_detect_extrema_device.argtypes = [vp, vp, vp, u64, pu64, pu64, vp]
    L.lf_mkd_filter_extrema_device.argtypes = [vp, vp, u64, u32, ctypes.c_float, vp, vp, pu64, vp]
    L.lf_mkd_detect.argtypes = [vp, vp, u32, u32, u32, ctypes.c_float, vp, vp, u64, pu64, pu64, pu64]
    L.lf_mkd_detect_u8.argtypes = L.lf_mkd_detect.argtypes
    L.lf_mkd_detect_times.argtypes = [vp] + [ctypes.POINTER(ctypes.c_double)] * 3
    L.lf_mkd_match_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, ctypes.c_float, vp, vp, vp, vp]
    L.lf_mkd_match.argtypes = [vp, vp, u64, vp, u64, ctypes.c_float, vp]
    L.lf_mkd_match_both_device.argtypes = [vp, vp, u64, vp, u64, ctypes.c_float, vp, vp, vp]
    L.lf_mkd_match_pairs_device.argtypes = [vp, vp, vp, u64, vp, vp, u64, u32, ctypes.c_float, u32, vp, vp, vp, vp, vp]
    L.lf_mkd_match_guided_pairs_device.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, u64, vp, u32, u32, ctypes.c_float,
                                                   ctypes.c_float, u32, vp, vp, vp, vp, vp]
    L.lf_mkd_match_overflowed.argtypes = [vp, vp, ctypes.POINTER(u64)]
    L.lf_mkd_quantize_descriptors_device.argtypes = [vp, vp, u64, ctypes.c_float, vp, vp]
    L.lf_mkd_quantize_descriptors.argtypes = [vp, vp, u64, ctypes.c_float, vp]
    L.lf_mkd_match_q8_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, ctypes.c_float, vp, vp, vp, vp]
    L.lf_mkd_match_q8.argtypes = [vp, vp, u64, vp, u64, ctypes.c_float, vp]
    L.lf_mkd_match_q8_plan.argtypes = [u64, u64, u32, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u64)]
    L.lf_mkd_match_q8_pairs_device.argtypes = L.lf_mkd_match_pairs_device.argtypes
    L.lf_mkd_match_q8_guided_pairs_device.argtypes = L.lf_mkd_match_guided_pairs_device.argtypes
    L.lf_mkd_match_q8_pairs_plan.argtypes = [u64, u64, u32, u32, ctypes.POINTER(u32), ctypes.POINTER(u64)]
    L.lf_mkd_knn_q8_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, u32, vp, vp, vp]
    L.lf_mkd_knn_q8.argtypes = [vp, vp, u64, vp, u64, u32, vp, vp]
    L.lf_mkd_knn_q8_plan.argtypes = [u64, u64, u32, u32, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u64)]
    L.lf_mkd_match_q8_grouped_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, ctypes.c_float, vp, vp, vp, vp]
    L.lf_mkd_match_q8_grouped.argtypes = [vp, vp, u64, vp, u64, vp, ctypes.c_float, vp, vp, vp]
    L.lf_mkd_match_q8_grouped_plan.argtypes = [u64, u64, u32, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u64)]
    L.lf_mkd_vote_groups_device.argtypes = [vp, vp, u64, vp, u32, vp, u64, u32, vp, vp]
    L.lf_mkd_edge_layout_device.argtypes = [vp, vp, u32, u64, vp, u32, vp, vp]
    L.lf_mkd_gather_edge_rows_device.argtypes = [vp, vp, u32, vp, u32, u64, vp, vp, u64, u32, vp, vp]
    L.lf_mkd_match_q8_edges_device.argtypes = [vp, vp, vp, u32, u64, vp, vp, u32, u64, vp, vp, vp, u64, vp, u64, u32,
                                               ctypes.c_float, u32, vp, vp, vp, vp, vp]
    L.lf_mkd_build_tracks_device.argtypes = [vp, vp, u32, u64, vp, vp, vp, u64, u32, vp, u32, vp, vp, vp, vp]
    L.lf_mkd_track_table_plan.argtypes = [u64, u32, vp, vp, vp, vp]
    L.lf_mkd_track_table_device.argtypes = [vp, vp, u32, u64, vp, vp, vp, u32, u32, u64, u64, vp, vp, vp, vp, vp, vp]
    L.lf_mkd_gather_track_rows_device.argtypes = [vp, vp, u32, u64, vp, vp, u64, vp, vp]
    L.lf_mkd_link_table_plan.argtypes = [u64, u32, vp, vp, vp, vp, vp]
    L.lf_mkd_link_table_device.argtypes = [vp, vp, u32, u64, vp, vp, vp, u64, u32, vp, u32, u32, u64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.lf_mkd_select_edges_plan.argtypes = [u32, u32, u32, u64, u32, vp, vp, vp, vp, vp]
    L.lf_mkd_select_edges_device.argtypes = [vp, vp, u32, u32, u32, u32, u32, u64, vp, vp, vp, vp, vp, vp, vp]
    L.lf_mkd_covisibility_plan.argtypes = [u32, u64, u64, u64, u32, vp, vp, vp, vp]
    L.lf_mkd_covisibility_device.argtypes = [vp, vp, u64, vp, u64, vp, u32, vp, vp, u64, u32, vp, vp]
    L.lf_mkd_two_view_pose_device.argtypes = [vp, vp, u64, vp, vp, u32, vp, u32, vp, vp, vp, vp, u64, ctypes.c_float, u32, vp, vp,
                                              vp, vp, vp, vp]
    L.lf_mkd_two_view_pose.argtypes = [vp, vp, vp, vp, vp, u64, vp, u64, vp, ctypes.c_float, u32, vp, vp, vp, vp, vp]
    L.lf_mkd_triangulate_tracks_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, vp, vp, vp, u32, ctypes.c_float, u32, u32,
                                                   vp, vp, vp, vp, vp]
    L.lf_mkd_triangulate_tracks.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, vp, vp, u32, ctypes.c_float, u32, u32, vp, vp, vp,
                                            vp]
    L.lf_mkd_resect_cameras_device.argtypes = [vp, vp, vp, u32, u64, vp, vp, u64, vp, vp, vp, ctypes.c_float, ctypes.c_float, u32,
                                               u32, u32, u32, u32, vp, vp, vp, vp, vp]
    L.lf_mkd_resect_camera.argtypes = [vp, vp, u64, vp, vp, u64, vp, ctypes.c_float, ctypes.c_float, u32, u32, u32, u32, u32, vp,
                                       vp, vp, vp]
    L.lf_mkd_track_descriptors_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, vp, u32, vp, ctypes.c_float, ctypes.c_float,
                                                  vp, vp, vp]
    L.lf_mkd_track_descriptors.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u32, vp, ctypes.c_float, ctypes.c_float, vp, vp]
    L.lf_mkd_bundle_adjust_device.argtypes = [vp, vp, vp, u32, u64, vp, u64, vp, vp, u64, vp, vp, vp, vp, vp, vp, ctypes.c_float,
                                              ctypes.c_float, u32, u32, ctypes.c_float, u32, vp, vp, vp, vp, vp, vp]
    L.lf_mkd_bundle_adjust.argtypes = [vp, vp, vp, u32, u64, vp, u64, vp, vp, u64, vp, vp, vp, vp, vp, ctypes.c_float,
                                       ctypes.c_float, u32, u32, ctypes.c_float, u32, vp, vp, vp, vp, vp]
    L.lf_mkd_bundle_adjust_intrinsics_device.argtypes = [vp, vp, vp, u32, u64, vp, u64, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp, u32, u32,
                                                         ctypes.c_float, ctypes.c_float, u32, u32, ctypes.c_float, u32, vp, vp, vp, vp,
                                                         vp, vp, vp, vp]
    L.lf_mkd_bundle_adjust_intrinsics.argtypes = [vp, vp, vp, u32, u64, vp, u64, vp, vp, u64, vp, vp, vp, vp, vp, vp, u32, u32,
                                                  ctypes.c_float, ctypes.c_float, u32, u32, ctypes.c_float, u32, vp, vp, vp, vp, vp,
                                                  vp, vp]
    L.lf_mkd_view_graph_plan.argtypes = [u32, u32, u32, u32, u32, u32, vp, vp, vp]
    L.lf_mkd_view_graph_device.argtypes = [vp, vp, vp, u32, vp, vp, u32, ctypes.c_float, u32, u32, u32, u32, u32, vp, u64, vp, vp,
                                           vp, vp, vp, vp, vp, vp]
    L.lf_mkd_view_graph.argtypes = [vp, vp, vp, u32, vp, vp, u32, ctypes.c_float, u32, u32, u32, u32, u32, vp, u64, vp, vp, vp, vp,
                                    vp, vp, vp]
    L.lf_mkd_tree_poses_device.argtypes = [vp, vp, vp, vp, u32, vp, vp, u32, u32, vp, vp]
    L.lf_mkd_tree_poses.argtypes = [vp, vp, vp, vp, u32, vp, vp, u32, u32, vp]
    L.lf_mkd_global_positions_plan.argtypes = [u32, u64, u32, vp, vp]
    L.lf_mkd_global_positions_device.argtypes = [vp, vp, vp, u32, u64, vp, u64, vp, vp, u64, vp, vp, vp, vp, u32, u32,
                                                 ctypes.c_float, u32, u32, vp, vp, vp, vp, vp, vp, vp]
    L.lf_mkd_global_positions.argtypes = [vp, vp, vp, u32, u64, vp, u64, vp, vp, u64, vp, vp, vp, u32, u32, ctypes.c_float, u32,
                                          u32, vp, vp, vp, vp, vp, vp]
    L.lf_mkd_verify_homography.argtypes = [vp, vp, u64, vp, u64, vp, u32, ctypes.c_float, u32, u32, vp, vp, vp]
    L.lf_mkd_verify_homography_device.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, ctypes.c_float, u32, u32, vp, vp, vp, vp]
    L.lf_mkd_verify_fundamental.argtypes = L.lf_mkd_verify_homography.argtypes
    L.lf_mkd_verify_fundamental_device.argtypes = L.lf_mkd_verify_homography_device.argtypes
    L.lf_mkd_stream_create.argtypes = [vp, u32, u32, u32, ctypes.c_float, u64, vp, vp, vp, vp]
    L.lf_mkd_stream_frame.argtypes = [vp, vp]
    L.lf_mkd_orient_keypoints_blocked.argtypes = [vp, vp, u64, u32, vp, u64, vp, vp, vp, u64, pu64, pu64]
    L.lf_mkd_detect_frames_device.argtypes = [vp, vp, u32, u32, u32, u32, ctypes.c_float, vp, vp, vp, u64, pu64, pu64,
                                              pu64, vp]
    L.lf_mkd_build_constants.argtypes = [vp] * 7
    i32 = ctypes.c_int32
    L.lf_mkd_comm_unique_id.argtypes = [vp]
    L.lf_mkd_comm_create.argtypes = [vp, vp, i32, i32, ctypes.POINTER(vp)]
    L.lf_mkd_comm_destroy.argtypes = [vp]
    L.lf_mkd_comm_info.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.lf_mkd_allgather_descriptors.argtypes = [vp, vp, vp, vp, i32, vp]
    L.lf_mkd_comm_loopback.argtypes = [vp, vp, vp, vp, u64, vp]
    L.lf_mkd_comm_last_form.argtypes = [vp]
    L.lf_mkd_detect_recordings.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.lf_mkd_plan_upload.argtypes = [u32, u32, u32, u32, vp, u32, ctypes.POINTER(u32), ctypes.POINTER(ctypes.c_double),
                                     ctypes.POINTER(ctypes.c_double)]
    L.lf_mkd_kernel_times.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                      ctypes.POINTER(u64)]
    _lib = L
    return L


def plan_upload(width, height, bytes_per_pixel=4, n_scales=4):
    """(cuts, modelled_us, one_piece_us): the pieces lf_mkd_detect[_u8] would upload a frame of this size in (lf_mkd_plan_upload;
    needs no device)."""
    cuts = (ctypes.c_uint32 * 16)()
    n, a, b = ctypes.c_uint32(), ctypes.c_double(), ctypes.c_double()
    rc = load_library().lf_mkd_plan_upload(width, height, bytes_per_pixel, n_scales, cuts, 16, ctypes.byref(n), ctypes.byref(a),
                                           ctypes.byref(b))
    if rc != 0:
        raise RuntimeError(f"lf_mkd_plan_upload failed ({rc})")
    return [int(cuts[i]) for i in range(min(n.value, 16))], a.value, b.value


def comm_unique_id():
    """Rank 0: the 128-byte RCCL identifier the other ranks need for Comm(...)."""
    buf = (ctypes.c_uint8 * COMM_ID_BYTES)()
    rc = load_library().lf_mkd_comm_unique_id(buf)
    if rc != 0:
        raise RuntimeError(f"lf_mkd_comm_unique_id failed ({rc}): RCCL is not loadable")
    return bytes(buf)


def match_q8_plan(na, nb, num_cus=0):
    """(a_blocks, b_splits, scratch_bytes): the grid lf_mkd_match_q8_device launches for this size and the scratch it needs
    (lf_mkd_match_q8_plan; needs no device).  num_cus 0: 256."""
    a, s, b = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    L = load_library()
    rc = L.lf_mkd_match_q8_plan(na, nb, num_cus, ctypes.byref(a), ctypes.byref(s), ctypes.byref(b))
    if rc != 0:
        raise RuntimeError(f"lf_mkd_match_q8_plan failed ({rc}): {L.lf_mkd_last_error(None).decode()}")
    return a.value, s.value, b.value


def knn_q8_plan(na, nb, k, num_cus=0):
    """(a_blocks, b_splits, scratch_bytes): the grid lf_mkd_knn_q8_device launches for this size and k and the scratch it
    needs (lf_mkd_knn_q8_plan; needs no device).  num_cus 0: 256."""
    a, s, b = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    L = load_library()
    rc = L.lf_mkd_knn_q8_plan(na, nb, k, num_cus, ctypes.byref(a), ctypes.byref(s), ctypes.byref(b))
    if rc != 0:
        raise RuntimeError(f"lf_mkd_knn_q8_plan failed ({rc}): {L.lf_mkd_last_error(None).decode()}")
    return a.value, s.value, b.value


def match_q8_grouped_plan(na, nb, num_cus=0):
    """(a_blocks, b_splits, scratch_bytes): the grid lf_mkd_match_q8_grouped_device launches for this size and the scratch it
    needs (lf_mkd_match_q8_grouped_plan; needs no device).  num_cus 0: 256."""
    a, s, b = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    L = load_library()
    rc = L.lf_mkd_match_q8_grouped_plan(na, nb, num_cus, ctypes.byref(a), ctypes.byref(s), ctypes.byref(b))
    if rc != 0:
        raise RuntimeError(f"lf_mkd_match_q8_grouped_plan failed ({rc}): {L.lf_mkd_last_error(None).decode()}")
    return a.value, s.value, b.value


def match_q8_pairs_plan(na_total, nb_total, n_pairs, both_directions=False):
    """(block_rows, workgroups): the a rows one workgroup of lf_mkd_match_q8_pairs_device owns and the grid the call launches
    for these totals -- floor(na_total / block_rows) + n_pairs, plus the same over b with both_directions
    (lf_mkd_match_q8_pairs_plan; needs no device)."""
    r, w = ctypes.c_uint32(), ctypes.c_uint64()
    L = load_library()
    rc = L.lf_mkd_match_q8_pairs_plan(na_total, nb_total, n_pairs, 1 if both_directions else 0, ctypes.byref(r), ctypes.byref(w))
    if rc != 0:
        raise RuntimeError(f"lf_mkd_match_q8_pairs_plan failed ({rc}): {L.lf_mkd_last_error(None).decode()}")
    return r.value, w.value


def track_table_plan(n_rows_total, min_len=2):
    """(key_bits, passes, block_rows, scratch_bytes) of lf_mkd_track_table_device for a pool of n_rows_total rows: the bits
    of floor(n_rows_total / min_len) -- the bound on the number of tracks the host knows --, the radix passes that sort
    them, the rows one workgroup sorts and the handle's scratch (lf_mkd_track_table_plan; needs no device)."""
    k, p, r, b = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    L = load_library()
    rc = L.lf_mkd_track_table_plan(n_rows_total, min_len, ctypes.byref(k), ctypes.byref(p), ctypes.byref(r), ctypes.byref(b))
    if rc != 0:
        raise RuntimeError(f"lf_mkd_track_table_plan failed ({rc}): {L.lf_mkd_last_error(None).decode()}")
    return k.value, p.value, r.value, b.value


def link_table_plan(ea_capacity, n_edges):
    """(slot_entries, slots, scan_fanout, scan_levels, scratch_bytes) of lf_mkd_link_table_device for n_edges edges whose a
    side's layout has ea_capacity entries: the entries of one slot, the slots (floor(ea_capacity / slot_entries) + n_edges,
    the grid), the fan-out and the levels of the scan over the slots, and the handle's scratch (lf_mkd_link_table_plan;
    needs no device)."""
    e, f, l = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    n, b = ctypes.c_uint64(), ctypes.c_uint64()
    L = load_library()
    rc = L.lf_mkd_link_table_plan(ea_capacity, n_edges, ctypes.byref(e), ctypes.byref(n), ctypes.byref(f), ctypes.byref(l),
                                  ctypes.byref(b))
    if rc != 0:
        raise RuntimeError(f"lf_mkd_link_table_plan failed ({rc}): {L.lf_mkd_last_error(None).decode()}")
    return e.value, n.value, f.value, l.value, b.value


def select_edges_plan(n_a, n_b, k, edge_capacity=None, flags=0):
    """(compiled_k, rows_per_workgroup, workgroups, launches, scratch_bytes) of lf_mkd_select_edges_device for an
    [n_a][n_b] vote table and k picks a row: the instantiation that serves k, the rows one workgroup of the selection takes
    (4: one wave per row; 1: a workgroup per row or per segment of one), its grid, the launches of the call and the handle's
    scratch (lf_mkd_select_edges_plan; needs no device).  edge_capacity None: n_a * k."""
    ck, r, l = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    w, b = ctypes.c_uint64(), ctypes.c_uint64()
    L = load_library()
    cap = n_a * k if edge_capacity is None else edge_capacity
    rc = L.lf_mkd_select_edges_plan(n_a, n_b, k, cap, flags, ctypes.byref(ck), ctypes.byref(r), ctypes.byref(w), ctypes.byref(l),
                                    ctypes.byref(b))
    if rc != 0:
        raise RuntimeError(f"lf_mkd_select_edges_plan failed ({rc}): {L.lf_mkd_last_error(None).decode()}")
    return ck.value, r.value, w.value, l.value, b.value


def covisibility_plan(n_images, track_capacity, obs_capacity, n_edges=0, flags=0):
    """(form, workgroups, launches, scratch_bytes) of lf_mkd_covisibility_device: the lanes that share a track (4 .. 64) plus
    COVIS_FORM_LDS iff workgroups count into a private table in LDS first, the grid of the first counting launch, the launches
    of the call and the handle's scratch (lf_mkd_covisibility_plan; needs no device)."""
    f, l = ctypes.c_uint32(), ctypes.c_uint32()
    w, b = ctypes.c_uint64(), ctypes.c_uint64()
    L = load_library()
    rc = L.lf_mkd_covisibility_plan(n_images, track_capacity, obs_capacity, n_edges, flags, ctypes.byref(f), ctypes.byref(w),
                                    ctypes.byref(l), ctypes.byref(b))
    if rc != 0:
        raise RuntimeError(f"lf_mkd_covisibility_plan failed ({rc}): {L.lf_mkd_last_error(None).decode()}")
    return f.value, w.value, l.value, b.value


def view_graph_plan(n_images, n_edges, tree_rounds=16, iterations=10, flags=0, with_match=False):
    """(launches, scratch_bytes, form) of lf_mkd_view_graph_device: the launches of the call (3 + tree_rounds + iterations, 2
    more with edges, one more with the match arrays), the handle's scratch and the form (0: the dense table of
    representatives) (lf_mkd_view_graph_plan; needs no device)."""
    l, f = ctypes.c_uint32(), ctypes.c_uint32()
    b = ctypes.c_uint64()
    L = load_library()
    rc = L.lf_mkd_view_graph_plan(n_images, n_edges, tree_rounds, iterations, flags, 1 if with_match else 0, ctypes.byref(l),
                                  ctypes.byref(b), ctypes.byref(f))
    if rc != 0:
        raise RuntimeError(f"lf_mkd_view_graph_plan failed ({rc}): {L.lf_mkd_last_error(None).decode()}")
    return l.value, b.value, f.value


def global_positions_plan(n_images, track_capacity, sweeps=50):
    """(launches, scratch_bytes) of lf_mkd_global_positions_device: 4 + 3 sweeps launches (none without images) and the
    handle's scratch (lf_mkd_global_positions_plan; needs no device)."""
    l, b = ctypes.c_uint32(), ctypes.c_uint64()
    L = load_library()
    rc = L.lf_mkd_global_positions_plan(n_images, track_capacity, sweeps, ctypes.byref(l), ctypes.byref(b))
    if rc != 0:
        raise RuntimeError(f"lf_mkd_global_positions_plan failed ({rc}): {L.lf_mkd_last_error(None).decode()}")
    return l.value, b.value


class Comm:
    """One rank's RCCL communicator on a handle's device (lf_mkd_comm_create): the all-gather of descriptor shards, the
    path's one collective, through the C boundary."""

    def __init__(self, handle, unique_id, n_ranks, rank):
        self._c = None
        self.handle, self.n_ranks, self.rank = handle, n_ranks, rank
        self.calls = 0                  # lf_mkd_allgather_descriptors calls made through this communicator
        c = ctypes.c_void_p()
        ident = (ctypes.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        handle._check(handle.L.lf_mkd_comm_create(handle._h, ident, n_ranks, rank, ctypes.byref(c)), "lf_mkd_comm_create")
        self._c = c

    def info(self):
        """(RCCL version code, ranks, this rank)"""
        v, n, r = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        self.handle._check(self.handle.L.lf_mkd_comm_info(self._c, ctypes.byref(v), ctypes.byref(n), ctypes.byref(r)),
                           "lf_mkd_comm_info")
        return v.value, n.value, r.value

    def allgather_descriptors(self, d_buf, counts, mode=GATHER_DIRECT, stream=None):
        """d_buf: device pointer of the [sum(counts)][128] f32 gathered set, this rank's rows already at their offset."""
        arr = (ctypes.c_uint64 * len(counts))(*[int(c) for c in counts])
        self.calls += 1
        self.handle._device_call(stream, lambda s: self.handle.L.lf_mkd_allgather_descriptors(
            self.handle._h, self._c, arr, d_buf, mode, s), "lf_mkd_allgather_descriptors")

    def loopback(self, d_src, d_dst, n_rows, stream=None):
        """n_rows descriptors from d_src to this very rank and back into d_dst: one group of ncclSend + ncclRecv through
        the posting routine of the direct gather (lf_mkd_comm_loopback)."""
        self.handle._device_call(stream, lambda s: self.handle.L.lf_mkd_comm_loopback(
            self.handle._h, self._c, d_src, d_dst, n_rows, s), "lf_mkd_comm_loopback")

    def last_form(self):
        """GATHER_DIRECT / GATHER_RING as the latest gather ran (-1: none yet)"""
        return self.handle.L.lf_mkd_comm_last_form(self._c)

    def close(self):
        if self._c is not None:
            self.handle.L.lf_mkd_comm_destroy(self._c)
            self._c = None

    def __del__(self):
        self.close()


class MkdHandle:
    """Thin owner of one lf_mkd handle.  Host arrays are numpy; device arguments are raw
    pointers (ints), e.g. torch.Tensor.data_ptr()."""

    def __init__(self, pca="liberty", max_features=2000, max_image_width=0, max_image_height=0,
                 patch_scale_factor=24.0, device=0, angle_mode=ANGLE_SHADER, pool_mode=POOL_DEFAULT, flags=0,
                 max_frames=1, n_scales=4, max_blobs=8000):
        self._h = None
        self.n_scales = n_scales
        self.max_features = max_features
        self.L = load_library()
        p = Params(max_image_width=max_image_width, max_image_height=max_image_height,
                   max_features=max_features, patch_scale_factor=patch_scale_factor,
                   device=device, angle_mode=angle_mode, pool_mode=pool_mode, flags=flags,
                   max_frames=max_frames, n_scales=n_scales, max_blobs=max_blobs)
        h = ctypes.c_void_p()
        rc = self.L.lf_mkd_create_from_file(ctypes.byref(p), model_path(pca).encode(), ctypes.byref(h))
        if rc != 0:
            raise RuntimeError(f"lf_mkd_create failed ({rc}): {self.L.lf_mkd_last_error(None).decode()}")
        self._h = h

    def close(self):
        if self._h is not None:
            self.L.lf_mkd_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {self.L.lf_mkd_last_error(self._h).decode()}")

    # --- host-pointer entry points -----------------------------------------------------------
    def describe_patches(self, patches):
        p = np.ascontiguousarray(patches, np.float32).reshape(-1, 32, 32)
        out = np.empty((p.shape[0], 128), np.float32)
        self._check(self.L.lf_mkd_describe_patches(self._h, p.ctypes.data, p.shape[0], out.ctypes.data),
                    "lf_mkd_describe_patches")
        return out

    def set_image(self, img):
        """f32 frame in [0, 1], or the uint8 luma it would be made from (1 B/px to the device, converted there: same bits)"""
        if img.ndim != 2:
            raise RuntimeError("image must be 2-D")
        if img.dtype == np.uint8:
            a = np.ascontiguousarray(img)
            self._check(self.L.lf_mkd_set_image_u8(self._h, a.ctypes.data, a.shape[1], a.shape[0]), "lf_mkd_set_image_u8")
            return
        a = np.ascontiguousarray(img, np.float32)
        self._check(self.L.lf_mkd_set_image(self._h, a.ctypes.data, a.shape[1], a.shape[0]), "lf_mkd_set_image")

    def describe_keypoints(self, kps):
        k = np.ascontiguousarray(kps)
        if k.dtype != KEYPOINT_DTYPE:
            k = np.ascontiguousarray(k, np.float32).reshape(-1, 5)
        n = k.shape[0]
        out = np.empty((n, 128), np.float32)
        self._check(self.L.lf_mkd_describe_keypoints(self._h, k.ctypes.data, n, out.ctypes.data),
                    "lf_mkd_describe_keypoints")
        return out

    def orient_keypoints(self, extrema, max_out=None):
        """extrema [n,4] (x, y, size, response) -> (keypoints [m,5] (x, y, size, angle_deg, response), dropped).
        Ordered by extremum, then histogram bin."""
        e = np.ascontiguousarray(extrema, np.float32).reshape(-1, 4)
        n = e.shape[0]
        cap = 18 * n if max_out is None else int(max_out)
        out = np.empty((max(cap, 1), 5), np.float32)
        m, dropped = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.L.lf_mkd_orient_keypoints(self._h, e.ctypes.data, n, out.ctypes.data, cap, ctypes.byref(m),
                                                   ctypes.byref(dropped)), "lf_mkd_orient_keypoints")
        return out[:m.value].copy(), dropped.value

    def detect_extrema(self, max_out=1 << 16):
        """Extrema of the loaded frame(s): ([m,4] (x, y, size, contrast), dropped).  Ordered by frame, scan cube, lane."""
        out = np.empty((max(max_out, 1), 4), np.float32)
        m, dropped = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.L.lf_mkd_detect_extrema(self._h, out.ctypes.data, max_out, ctypes.byref(m),
                                                 ctypes.byref(dropped)), "lf_mkd_detect_extrema")
        return out[:m.value].copy(), dropped.value

    def detect_into(self, img, top_n, min_size, kps, desc):
        """lf_mkd_detect / lf_mkd_detect_u8 (by the frame's dtype) into caller-held arrays kps [cap,5] f32, desc [cap,128] f32:
        (m, dropped_blobs, dropped_features).  What a caller that reuses its buffers pays: the C call and nothing else."""
        if img.ndim != 2:
            raise RuntimeError("image must be 2-D")
        cap = kps.shape[0]
        assert kps.dtype == np.float32 and desc.dtype == np.float32 and desc.shape[0] == cap and kps.flags.c_contiguous and desc.flags.c_contiguous
        m, db, df = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        if img.dtype == np.uint8:
            a = np.ascontiguousarray(img)
            fn, what = self.L.lf_mkd_detect_u8, "lf_mkd_detect_u8"
        else:
            a = np.ascontiguousarray(img, np.float32)
            fn, what = self.L.lf_mkd_detect, "lf_mkd_detect"
        self._check(fn(self._h, a.ctypes.data, a.shape[1], a.shape[0], top_n, min_size, kps.ctypes.data, desc.ctypes.data, cap,
                       ctypes.byref(m), ctypes.byref(db), ctypes.byref(df)), what)
        return m.value, db.value, df.value

    def detect_recordings(self):
        """(recorded pipelines held, of them with a banded upload, distinct requests remembered) -- lf_mkd_detect_recordings"""
        a, b, c = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self.L.lf_mkd_detect_recordings(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
                    "lf_mkd_detect_recordings")
        return a.value, b.value, c.value

    def detect_times(self):
        """(upload_ms, pipeline_ms, readback_ms) of the latest detect call; needs FLAG_KERNEL_TIMING."""
        a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        self._check(self.L.lf_mkd_detect_times(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "lf_mkd_detect_times")
        return a.value, b.value, c.value

    def detect(self, img, top_n=0, min_size=0.0, max_out=None):
        """lf_mkd_detect (f32 frame) or lf_mkd_detect_u8 (uint8 frame): (keypoints [m,5], descriptors [m,128], dropped_blobs,
        dropped_features)."""
        cap = int(max_out if max_out is not None else self.max_features)
        kps = np.empty((max(cap, 1), 5), np.float32)
        desc = np.empty((max(cap, 1), 128), np.float32)
        if cap == 0:
            m, db, df = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
            a = np.ascontiguousarray(img) if img.dtype == np.uint8 else np.ascontiguousarray(img, np.float32)
            fn = self.L.lf_mkd_detect_u8 if img.dtype == np.uint8 else self.L.lf_mkd_detect
            self._check(fn(self._h, a.ctypes.data, a.shape[1], a.shape[0], top_n, min_size, kps.ctypes.data, desc.ctypes.data, 0,
                           ctypes.byref(m), ctypes.byref(db), ctypes.byref(df)), "lf_mkd_detect")
            return kps[:0].copy(), desc[:0].copy(), db.value, df.value
        m, db, df = self.detect_into(img, top_n, min_size, kps, desc)
        return kps[:m].copy(), desc[:m].copy(), db, df

    def match(self, a, b, ratio=0.8):
        """match_features (examples/match_images/src/main.rs:8-27): int32 [na], index into b or -1."""
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 128)
        b = np.ascontiguousarray(b, np.float32).reshape(-1, 128)
        out = np.empty(len(a), np.int32)
        self._check(self.L.lf_mkd_match(self._h, a.ctypes.data, len(a), b.ctypes.data, len(b), ratio, out.ctypes.data),
                    "lf_mkd_match")
        return out

    def quantize(self, desc, scale=Q8_SCALE):
        """lf_mkd_quantize_descriptors: [n,128] f32 -> [n,128] uint8, byte = clamp(rint(x * scale), -127, 127) + 128."""
        d = np.ascontiguousarray(desc, np.float32).reshape(-1, 128)
        out = np.empty((len(d), 128), np.uint8)
        self._check(self.L.lf_mkd_quantize_descriptors(self._h, d.ctypes.data, len(d), scale, out.ctypes.data),
                    "lf_mkd_quantize_descriptors")
        return out

    def match_q8(self, qa, qb, ratio=0.8):
        """lf_mkd_match_q8: `match` over 8-bit descriptors [n,128] uint8, decided on exact integer similarities."""
        a = np.ascontiguousarray(qa, np.uint8).reshape(-1, 128)
        b = np.ascontiguousarray(qb, np.uint8).reshape(-1, 128)
        out = np.empty(len(a), np.int32)
        self._check(self.L.lf_mkd_match_q8(self._h, a.ctypes.data, len(a), b.ctypes.data, len(b), ratio, out.ctypes.data),
                    "lf_mkd_match_q8")
        return out

    def knn_q8(self, qa, qb, k):
        """lf_mkd_knn_q8: each row's k best rows of qb over 8-bit descriptors [n,128] uint8 -> (index [na,k] int32,
        score [na,k] int32), larger similarity first, among equal ones the higher index first; -1 / INT32_MIN beyond the
        number of candidates."""
        a = np.ascontiguousarray(qa, np.uint8).reshape(-1, 128)
        b = np.ascontiguousarray(qb, np.uint8).reshape(-1, 128)
        index, score = np.empty((len(a), int(k)), np.int32), np.empty((len(a), int(k)), np.int32)
        self._check(self.L.lf_mkd_knn_q8(self._h, a.ctypes.data, len(a), b.ctypes.data, len(b), k, index.ctypes.data,
                                         score.ctypes.data), "lf_mkd_knn_q8")
        return index, score

    def match_q8_grouped(self, qa, qb, groups_b, ratio=0.8):
        """lf_mkd_match_q8_grouped: the ratio test against the best neighbour from another group over 8-bit descriptors
        [n,128] uint8, groups_b [nb] uint32 -> (match [na] int32: the best row of qb or -1, best [na] int32, rival [na] int32:
        the best score among the rows of another group than the best's, INT32_MIN if there is none)."""
        a = np.ascontiguousarray(qa, np.uint8).reshape(-1, 128)
        b = np.ascontiguousarray(qb, np.uint8).reshape(-1, 128)
        g = np.ascontiguousarray(groups_b, np.uint32).reshape(-1)
        if len(g) != len(b):
            raise RuntimeError("match_q8_grouped: groups_b needs one id per row of qb")
        match, best, rival = (np.empty(len(a), np.int32) for _ in range(3))
        self._check(self.L.lf_mkd_match_q8_grouped(self._h, a.ctypes.data, len(a), b.ctypes.data, len(b), g.ctypes.data, ratio,
                                                   match.ctypes.data, best.ctypes.data, rival.ctypes.data),
                    "lf_mkd_match_q8_grouped")
        return match, best, rival

    def verify_homography(self, kps_a, kps_b, match, n_hypotheses=2048, threshold=3.0, seed=0, flags=0):
        """lf_mkd_verify_homography: kps_a [na,5], kps_b [nb,5] f32 rows, match int32 [na] (index into b or -1) ->
        (H [3,3] f32, verified int32 [na], stats uint32 [4])."""
        a = np.ascontiguousarray(kps_a, np.float32).reshape(-1, 5)
        b = np.ascontiguousarray(kps_b, np.float32).reshape(-1, 5)
        m = np.ascontiguousarray(match, np.int32).reshape(-1)
        if len(m) != len(a):
            raise RuntimeError("verify_homography: match must have one entry per row of kps_a")
        H = np.empty(9, np.float32)
        ver = np.empty(max(len(a), 1), np.int32)
        st = np.empty(4, np.uint32)
        self._check(self.L.lf_mkd_verify_homography(self._h, a.ctypes.data, len(a), b.ctypes.data, len(b), m.ctypes.data,
                                                     n_hypotheses, threshold, seed, flags, H.ctypes.data, ver.ctypes.data,
                                                     st.ctypes.data), "lf_mkd_verify_homography")
        return H.reshape(3, 3), ver[:len(a)].copy(), st

    def verify_fundamental(self, kps_a, kps_b, match, n_hypotheses=2048, threshold=1.5, seed=0, flags=0):
        """lf_mkd_verify_fundamental: as verify_homography -> (F [3,3] f32, verified int32 [na], stats uint32 [4])."""
        a = np.ascontiguousarray(kps_a, np.float32).reshape(-1, 5)
        b = np.ascontiguousarray(kps_b, np.float32).reshape(-1, 5)
        m = np.ascontiguousarray(match, np.int32).reshape(-1)
        if len(m) != len(a):
            raise RuntimeError("verify_fundamental: match must have one entry per row of kps_a")
        F = np.empty(9, np.float32)
        ver = np.empty(max(len(a), 1), np.int32)
        st = np.empty(4, np.uint32)
        self._check(self.L.lf_mkd_verify_fundamental(self._h, a.ctypes.data, len(a), b.ctypes.data, len(b), m.ctypes.data,
                                                      n_hypotheses, threshold, seed, flags, F.ctypes.data, ver.ctypes.data,
                                                      st.ctypes.data), "lf_mkd_verify_fundamental")
        return F.reshape(3, 3), ver[:len(a)].copy(), st

    def two_view_pose(self, F, K_a, K_b, kps_a, kps_b, match, min_parallax_deg=1.0, flags=0, points=True):
        """lf_mkd_two_view_pose: F [3,3] f32 (b^T F a = 0, pixels), K_a / K_b = (fx, fy, cx, cy), kps_a [na,5], kps_b [nb,5]
        f32 rows, match int32 [na] (index into b or -1: pass the verifier's `verified`) -> (R [3,3] f32, t [3] f32, stats
        uint32 [4], sigma [3] f32, points [na,4] f32 or None)."""
        f = np.ascontiguousarray(F, np.float32).reshape(9)
        ka, kb = np.ascontiguousarray(K_a, np.float32).reshape(4), np.ascontiguousarray(K_b, np.float32).reshape(4)
        a = np.ascontiguousarray(kps_a, np.float32).reshape(-1, 5)
        b = np.ascontiguousarray(kps_b, np.float32).reshape(-1, 5)
        m = np.ascontiguousarray(match, np.int32).reshape(-1)
        if len(m) != len(a):
            raise RuntimeError("two_view_pose: match must have one entry per row of kps_a")
        R, t, st, sg = np.empty(9, np.float32), np.empty(3, np.float32), np.empty(4, np.uint32), np.empty(3, np.float32)
        pts = np.empty((max(len(a), 1), 4), np.float32) if points else None
        self._check(self.L.lf_mkd_two_view_pose(self._h, f.ctypes.data, ka.ctypes.data, kb.ctypes.data, a.ctypes.data, len(a),
                                                 b.ctypes.data, len(b), m.ctypes.data, min_parallax_deg, flags, R.ctypes.data,
                                                 t.ctypes.data, st.ctypes.data, sg.ctypes.data,
                                                 pts.ctypes.data if points else None), "lf_mkd_two_view_pose")
        return R.reshape(3, 3), t, st, sg, pts[:len(a)].copy() if points else None

    def triangulate_tracks(self, kps, track_offsets, obs_row, obs_image, intrinsics, poses, max_reproj_px=4.0, rounds=2,
                           flags=0, err=True, obs_state=True):
        """lf_mkd_triangulate_tracks: kps [rows,5] f32, track_offsets uint64 [n_tracks + 1], obs_row int32 / obs_image uint32
        [n_obs], intrinsics [n_images,4] f32 (fx, fy, cx, cy), poses [n_images,12] f32 (R row-major, then t; world to camera)
        -> (points [n_tracks,4] f32, stats uint32 [n_tracks,4], err [n_tracks,2] f32 or None, obs_state uint32 [n_obs] or None;
        `obs_state` may be an array to start from: entries outside every track's range keep its values)."""
        k = np.ascontiguousarray(kps, np.float32).reshape(-1, 5)
        off = np.ascontiguousarray(track_offsets, np.uint64).reshape(-1)
        row, img = np.ascontiguousarray(obs_row, np.int32).reshape(-1), np.ascontiguousarray(obs_image, np.uint32).reshape(-1)
        K = np.ascontiguousarray(intrinsics, np.float32).reshape(-1, 4)
        P = np.ascontiguousarray(poses, np.float32).reshape(-1, 12)
        if len(off) < 1 or len(row) != len(img) or len(K) != len(P):
            raise RuntimeError("triangulate_tracks: track_offsets needs n_tracks + 1 entries, obs_row and obs_image one entry "
                               "per observation, intrinsics and poses one row per image")
        n, n_obs = len(off) - 1, len(row)
        pts, st = np.empty((max(n, 1), 4), np.float32), np.empty((max(n, 1), 4), np.uint32)
        er = np.empty((max(n, 1), 2), np.float32) if err else None
        if obs_state is True:
            os_ = np.zeros(max(n_obs, 1), np.uint32)
        elif obs_state is None or obs_state is False:
            os_ = None
        else:
            os_ = np.array(obs_state, np.uint32).reshape(-1)
            if len(os_) != n_obs:
                raise RuntimeError("triangulate_tracks: obs_state needs one entry per observation")
        at = lambda x: x.ctypes.data if x is not None and x.size else None
        self._check(self.L.lf_mkd_triangulate_tracks(self._h, at(k), len(k), off.ctypes.data, n, at(row), at(img), n_obs, at(K),
                                                      at(P), len(K), max_reproj_px, rounds, flags, pts.ctypes.data,
                                                      st.ctypes.data, at(er), at(os_)), "lf_mkd_triangulate_tracks")
        return pts[:n], st[:n], er[:n] if err else None, os_[:n_obs] if os_ is not None else None

    def resect_camera(self, kps, row_track, points, intrinsics, max_reproj_px=4.0, min_parallax_deg=0.0, n_samples=512,
                      min_inliers=12, rounds=3, seed=0, flags=0, err=True, row_state=True):
        """lf_mkd_resect_camera, ONE image: kps [rows,5] f32 (its rows), row_track int32 [rows] (the table index of a row's track
        or -1), points [n_tracks,4] f32 (X, Y, Z, the parallax cosine; (0, 0, 0, 2): none), intrinsics [4] f32 (fx, fy, cx, cy)
        -> (pose [12] f32: R row-major, then t, all zero for none; stats uint32 [4] = M, inliers, reason, winning candidate;
        err [2] f32 or None; row_state uint32 [rows] or None: 0 no correspondence, 1 correspondence, 2 inlier).  The image is
        image 0 of a device call: pass seed + i to get image i of a batch."""
        k = np.ascontiguousarray(kps, np.float32).reshape(-1, 5)
        rt = np.ascontiguousarray(row_track, np.int32).reshape(-1)
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        K = np.ascontiguousarray(intrinsics, np.float32).reshape(-1)
        if len(rt) != len(k) or len(K) != 4:
            raise RuntimeError("resect_camera: row_track needs one entry per row of kps, intrinsics 4 values")
        pose, st = np.zeros(12, np.float32), np.zeros(4, np.uint32)
        er = np.zeros(2, np.float32) if err else None
        rs = np.zeros(max(len(k), 1), np.uint32) if row_state else None
        at = lambda x: x.ctypes.data if x is not None and x.size else None
        self._check(self.L.lf_mkd_resect_camera(self._h, at(k), len(k), at(rt), at(pts), len(pts), K.ctypes.data, max_reproj_px,
                                                min_parallax_deg, n_samples, min_inliers, rounds, seed & 0xFFFFFFFF, flags,
                                                pose.ctypes.data, st.ctypes.data, at(er), rs.ctypes.data if row_state else None),
                    "lf_mkd_resect_camera")
        return pose, st, er, rs[:len(k)] if row_state else None

    def track_descriptors(self, q8, track_offsets, obs_row, obs_state=None, min_state=2, points=None, min_parallax_deg=0.0,
                          scale=Q8_SCALE, stats=True):
        """lf_mkd_track_descriptors: q8 uint8 [rows,128] (the pool's quantised rows), track_offsets uint64 [n_tracks + 1],
        obs_row int32 [n_obs], optionally obs_state uint32 [n_obs] with min_state (an observation contributes iff its state is
        at least min_state) and points [n_tracks,4] f32 with min_parallax_deg (a track is described iff its point passes
        resection's rule) -> (desc uint8 [n_tracks,128]: the sum of the contributors' centred rows, normalised and quantised
        with `scale`, or the zero row, all 128; stats int32 [n_tracks,2] = contributors, smallest similarity of a contributor
        with the row (INT32_MIN for a zero row), or None)."""
        q = np.ascontiguousarray(q8, np.uint8).reshape(-1, 128)
        off = np.ascontiguousarray(track_offsets, np.uint64).reshape(-1)
        row = np.ascontiguousarray(obs_row, np.int32).reshape(-1)
        st = None if obs_state is None else np.ascontiguousarray(obs_state, np.uint32).reshape(-1)
        pts = None if points is None else np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        n, n_obs = len(off) - 1, len(row)
        if len(off) < 1 or (st is not None and len(st) != n_obs) or (pts is not None and len(pts) != n):
            raise RuntimeError("track_descriptors: track_offsets needs n_tracks + 1 entries, obs_state one entry per observation, "
                               "points one row per track")
        desc = np.empty((max(n, 1), 128), np.uint8)
        ds = np.empty((max(n, 1), 2), np.int32) if stats else None
        at = lambda x: x.ctypes.data if x is not None and x.size else None
        self._check(self.L.lf_mkd_track_descriptors(self._h, at(q), len(q), off.ctypes.data, n, at(row), n_obs, at(st), min_state,
                                                     at(pts), min_parallax_deg, scale, desc.ctypes.data, at(ds)),
                    "lf_mkd_track_descriptors")
        return desc[:n], ds[:n] if stats else None

    def view_graph(self, edge_a, edge_b, R, pose_stats, n_images, max_loop_deg=3.0, min_front=0, root=VIEW_GRAPH_AUTO_ROOT,
                   tree_rounds=16, iterations=10, flags=0, edge_offsets_a=None, match=None, residual=True):
        """lf_mkd_view_graph: edge_a / edge_b uint32 [n_edges], R f32 [n_edges, 9] and pose_stats uint32 [n_edges, 4] as
        two_view_pose gave them, optionally the matches' edge layout (edge_offsets_a uint64 [n_edges + 1]) and the match array
        -> (rotations f32 [n_images, 9], all zero for an image without one; edge_stats uint32 [n_edges, 4] = closed,
        consistent, state (0 not usable, 1 rejected, 2 unchecked, 3 supported), the pair's representative; residual f32
        [n_edges] or None; image_stats uint32 [n_images, 4] = kept edges, round, tree edge, rejected edges; counts uint32 [8] =
        usable, supported, rejected, unchecked, kept, labelled, root, 0; the match array with the entries of the edges that are
        not kept at -1, or None)."""
        ea = np.ascontiguousarray(edge_a, np.uint32).reshape(-1)
        eb = np.ascontiguousarray(edge_b, np.uint32).reshape(-1)
        r = np.ascontiguousarray(R, np.float32).reshape(-1, 9)
        ps = np.ascontiguousarray(pose_stats, np.uint32).reshape(-1, 4)
        n = len(ea)
        if len(eb) != n or len(r) != n or len(ps) != n:
            raise RuntimeError("view_graph: edge_b, R and pose_stats need one row per entry of edge_a")
        if (edge_offsets_a is None) != (match is None):
            raise RuntimeError("view_graph: edge_offsets_a and match go together")
        off = m = out = None
        if match is not None:
            off = np.ascontiguousarray(edge_offsets_a, np.uint64).reshape(-1)
            m = np.ascontiguousarray(match, np.int32).reshape(-1)
            if len(off) != n + 1:
                raise RuntimeError("view_graph: edge_offsets_a needs n_edges + 1 entries")
            out = np.empty(max(len(m), 1), np.int32)
        rot, es = np.zeros((max(n_images, 1), 9), np.float32), np.zeros((max(n, 1), 4), np.uint32)
        res = np.zeros(max(n, 1), np.float32) if residual else None
        ims, counts = np.zeros((max(n_images, 1), 4), np.uint32), np.zeros(8, np.uint32)
        at = lambda x: x.ctypes.data if x is not None and x.size else None
        self._check(self.L.lf_mkd_view_graph(self._h, at(ea), at(eb), n, at(r), at(ps), n_images, max_loop_deg, min_front, root,
                                             tree_rounds, iterations, flags, off.ctypes.data if off is not None else None,
                                             len(m) if m is not None else 0, m.ctypes.data if m is not None else None,
                                             out.ctypes.data if out is not None else None, rot.ctypes.data, es.ctypes.data,
                                             res.ctypes.data if residual else None, ims.ctypes.data, counts.ctypes.data),
                    "lf_mkd_view_graph")
        return (rot[:n_images], es[:n], res[:n] if residual else None, ims[:n_images], counts,
                out[:len(m)] if out is not None else None)

    def tree_poses(self, edge_a, edge_b, t, rotations, image_stats, max_depth=64):
        """lf_mkd_tree_poses: edge_a / edge_b uint32 [n_edges] and t f32 [n_edges, 3] as two_view_pose gave them, rotations f32
        [n_images, 9] and image_stats uint32 [n_images, 4] as view_graph gave them -> poses f32 [n_images, 12]: the view
        graph's rotation and a centre one unit step from the tree parent's; the zero row for an image whose chain of tree
        edges does not reach the root within max_depth steps."""
        ea = np.ascontiguousarray(edge_a, np.uint32).reshape(-1)
        eb = np.ascontiguousarray(edge_b, np.uint32).reshape(-1)
        tt = np.ascontiguousarray(t, np.float32).reshape(-1, 3)
        rot = np.ascontiguousarray(rotations, np.float32).reshape(-1, 9)
        ims = np.ascontiguousarray(image_stats, np.uint32).reshape(-1, 4)
        n, n_images = len(ea), len(rot)
        if len(eb) != n or len(tt) != n or len(ims) != n_images:
            raise RuntimeError("tree_poses: edge_b and t need one row per entry of edge_a, image_stats one row per rotation")
        poses = np.zeros((max(n_images, 1), 12), np.float32)
        at = lambda x: x.ctypes.data if x is not None and x.size else None
        self._check(self.L.lf_mkd_tree_poses(self._h, at(ea), at(eb), at(tt), n, at(rot), at(ims), n_images, max_depth,
                                             poses.ctypes.data), "lf_mkd_tree_poses")
        return poses[:n_images]

    def global_positions(self, kps, image_offsets, track_offsets, obs_row, obs_image, row_track, intrinsics, poses, sweeps=50,
                         warm=3, robust_deg=0.2, min_obs=2, flags=0, points=True, obs_state=True, trace=True):
        """lf_mkd_global_positions: kps [rows,5] f32, image_offsets uint64 [n_images + 1], the track table (track_offsets uint64
        [n_tracks + 1], obs_row int32 / obs_image uint32 [n_obs]), row_track int32 [rows], intrinsics [n_images,4] f32, poses
        [n_images,12] f32 (rotations held, centres the start) -> (poses [n_images,12] f32 in the gauge centroid 0 / rms radius
        1, points [n_tracks,4] f32 or None, obs_state uint32 [n_obs] or None, image_stats uint32 [n_images,4] = usable rows,
        weighted rows, sweeps held, reason; trace float64 [sweeps,4] = cost, weighted observations, held cameras, unsolved
        points, or None; counts uint32 [8])."""
        k = np.ascontiguousarray(kps, np.float32).reshape(-1, 5)
        ioff = np.ascontiguousarray(image_offsets, np.uint64).reshape(-1)
        toff = np.ascontiguousarray(track_offsets, np.uint64).reshape(-1)
        row, img = np.ascontiguousarray(obs_row, np.int32).reshape(-1), np.ascontiguousarray(obs_image, np.uint32).reshape(-1)
        rt = np.ascontiguousarray(row_track, np.int32).reshape(-1)
        K = np.ascontiguousarray(intrinsics, np.float32).reshape(-1, 4)
        P = np.ascontiguousarray(poses, np.float32).reshape(-1, 12)
        n_images, n_tracks, n_obs = len(K), max(len(toff), 1) - 1, len(row)
        if len(ioff) != n_images + 1 or len(img) != n_obs or len(P) != n_images or len(rt) != len(k):
            raise RuntimeError("global_positions: image_offsets needs n_images + 1 entries, obs_row and obs_image one entry per "
                               "observation, row_track one per row, intrinsics and poses one row per image")
        po, xo = np.zeros((max(n_images, 1), 12), np.float32), np.zeros((max(n_tracks, 1), 4), np.float32) if points else None
        so = np.zeros(max(n_obs, 1), np.uint32) if obs_state else None
        ims, counts = np.zeros((max(n_images, 1), 4), np.uint32), np.zeros(8, np.uint32)
        tr = np.zeros((max(sweeps, 1), 4), np.float64) if trace else None
        at = lambda x: x.ctypes.data if x is not None and x.size else None
        self._check(self.L.lf_mkd_global_positions(self._h, at(k), ioff.ctypes.data, n_images, len(k), at(toff), n_tracks, at(row),
                                                   at(img), n_obs, at(rt), at(K), at(P), sweeps, warm, robust_deg, min_obs, flags,
                                                   po.ctypes.data, xo.ctypes.data if points else None,
                                                   so.ctypes.data if obs_state else None, ims.ctypes.data,
                                                   tr.ctypes.data if trace else None, counts.ctypes.data),
                    "lf_mkd_global_positions")
        return (po[:n_images], xo[:n_tracks] if points else None, so[:n_obs] if obs_state else None, ims[:n_images],
                tr[:sweeps] if trace else None, counts)

    def bundle_adjust(self, kps, image_offsets, track_offsets, obs_row, obs_image, points, intrinsics, poses, obs_state=None,
                      camera_fixed=None, max_reproj_px=4.0, lambda0=1e-3, iterations=10, cg_iterations=10, cg_tol=0.1, flags=0,
                      obs_state_out=True):
        """lf_mkd_bundle_adjust: kps [rows,5] f32, image_offsets uint64 [n_images + 1], the track table (track_offsets uint64
        [n_tracks + 1], obs_row int32 / obs_image uint32 [n_obs]), points [n_tracks,4] f32, intrinsics [n_images,4] f32, poses
        [n_images,12] f32, optional obs_state uint32 [n_obs] (the triangulation call's) and camera_fixed uint32 [n_images]
        (non-zero: the pose is held) -> (poses [n_images,12] f32, points [n_tracks,4] f32, obs_state uint32 [n_obs] or None,
        trace float64 [iterations,8] = cost, cost', lambda, accepted, CG steps, inliers, held cameras, held points; counts
        uint32 [4] = free cameras, free points, active observations, accepted steps)."""
        k = np.ascontiguousarray(kps, np.float32).reshape(-1, 5)
        ioff = np.ascontiguousarray(image_offsets, np.uint64).reshape(-1)
        toff = np.ascontiguousarray(track_offsets, np.uint64).reshape(-1)
        row, img = np.ascontiguousarray(obs_row, np.int32).reshape(-1), np.ascontiguousarray(obs_image, np.uint32).reshape(-1)
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        K = np.ascontiguousarray(intrinsics, np.float32).reshape(-1, 4)
        P = np.ascontiguousarray(poses, np.float32).reshape(-1, 12)
        n_images, n_tracks, n_obs = len(K), len(pts), len(row)
        st = None if obs_state is None else np.ascontiguousarray(obs_state, np.uint32).reshape(-1)
        fx = None if camera_fixed is None else np.ascontiguousarray(camera_fixed, np.uint32).reshape(-1)
        if (len(ioff) != n_images + 1 or len(toff) != n_tracks + 1 or len(img) != n_obs or len(P) != n_images or
                (st is not None and len(st) != n_obs) or (fx is not None and len(fx) != n_images)):
            raise RuntimeError("bundle_adjust: image_offsets needs n_images + 1 entries, track_offsets n_tracks + 1, obs_row, "
                               "obs_image and obs_state one entry per observation, intrinsics, poses and camera_fixed one row per "
                               "image")
        po, xo = np.zeros((max(n_images, 1), 12), np.float32), np.zeros((max(n_tracks, 1), 4), np.float32)
        so = np.zeros(max(n_obs, 1), np.uint32) if obs_state_out else None
        trace, counts = np.zeros((max(iterations, 1), 8), np.float64), np.zeros(4, np.uint32)
        at = lambda x: x.ctypes.data if x is not None and x.size else None
        self._check(self.L.lf_mkd_bundle_adjust(self._h, at(k), ioff.ctypes.data, n_images, len(k), toff.ctypes.data, n_tracks,
                                                at(row), at(img), n_obs, at(pts), at(K), at(P), at(st), at(fx), max_reproj_px, lambda0,
                                                iterations, cg_iterations, cg_tol, flags, po.ctypes.data, xo.ctypes.data,
                                                so.ctypes.data if obs_state_out else None, trace.ctypes.data, counts.ctypes.data),
                    "lf_mkd_bundle_adjust")
        return po[:n_images], xo[:n_tracks], so[:n_obs] if obs_state_out else None, trace, counts

    def bundle_adjust_intrinsics(self, kps, image_offsets, track_offsets, obs_row, obs_image, points, intrinsics, poses,
                                 obs_state=None, camera_fixed=None, camera_group=None, n_groups=1, refine=BA_REFINE_FOCAL,
                                 max_reproj_px=4.0, lambda0=1e-3, iterations=10, cg_iterations=10, cg_tol=0.1, flags=0,
                                 obs_state_out=True):
        """lf_mkd_bundle_adjust_intrinsics: bundle_adjust's arrays, camera_group uint32 [n_images] (the lens of an image; None:
        one group; an id >= n_groups: constant intrinsics) and refine = BA_REFINE_FOCAL | BA_REFINE_PRINCIPAL -> (poses, points,
        intrinsics [n_images,4] f32, groups [n_groups,3] f32 = (s, dx, dy), obs_state or None, trace float64 [iterations,9] =
        bundle_adjust's eight and the held groups, counts uint32 [5] = its four and the free groups)."""
        k = np.ascontiguousarray(kps, np.float32).reshape(-1, 5)
        ioff = np.ascontiguousarray(image_offsets, np.uint64).reshape(-1)
        toff = np.ascontiguousarray(track_offsets, np.uint64).reshape(-1)
        row, img = np.ascontiguousarray(obs_row, np.int32).reshape(-1), np.ascontiguousarray(obs_image, np.uint32).reshape(-1)
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        K = np.ascontiguousarray(intrinsics, np.float32).reshape(-1, 4)
        P = np.ascontiguousarray(poses, np.float32).reshape(-1, 12)
        n_images, n_tracks, n_obs = len(K), len(pts), len(row)
        st = None if obs_state is None else np.ascontiguousarray(obs_state, np.uint32).reshape(-1)
        fx = None if camera_fixed is None else np.ascontiguousarray(camera_fixed, np.uint32).reshape(-1)
        gr = None if camera_group is None else np.ascontiguousarray(camera_group, np.uint32).reshape(-1)
        if (len(ioff) != n_images + 1 or len(toff) != n_tracks + 1 or len(img) != n_obs or len(P) != n_images or
                (st is not None and len(st) != n_obs) or (fx is not None and len(fx) != n_images) or
                (gr is not None and len(gr) != n_images)):
            raise RuntimeError("bundle_adjust_intrinsics: image_offsets needs n_images + 1 entries, track_offsets n_tracks + 1, "
                               "obs_row, obs_image and obs_state one entry per observation, intrinsics, poses, camera_fixed and "
                               "camera_group one row per image")
        po, xo = np.zeros((max(n_images, 1), 12), np.float32), np.zeros((max(n_tracks, 1), 4), np.float32)
        ko, go = np.zeros((max(n_images, 1), 4), np.float32), np.zeros((max(n_groups, 1), 3), np.float32)
        so = np.zeros(max(n_obs, 1), np.uint32) if obs_state_out else None
        trace, counts = np.zeros((max(iterations, 1), 9), np.float64), np.zeros(5, np.uint32)
        at = lambda x: x.ctypes.data if x is not None and x.size else None
        self._check(self.L.lf_mkd_bundle_adjust_intrinsics(
            self._h, at(k), ioff.ctypes.data, n_images, len(k), toff.ctypes.data, n_tracks, at(row), at(img), n_obs, at(pts), at(K),
            at(P), at(st), at(fx), at(gr), n_groups, refine, max_reproj_px, lambda0, iterations, cg_iterations, cg_tol, flags,
            po.ctypes.data, xo.ctypes.data, ko.ctypes.data, go.ctypes.data, so.ctypes.data if obs_state_out else None,
            trace.ctypes.data, counts.ctypes.data), "lf_mkd_bundle_adjust_intrinsics")
        return po[:n_images], xo[:n_tracks], ko[:n_images], go[:n_groups], so[:n_obs] if obs_state_out else None, trace, counts

    def orient_keypoints_blocked(self, extremum_data, n_extrema, indices, max_out, block_len=256):
        """The reference's ExtremumLocations.data (blocked) + FilteredExtrema.indices in, KeypointIndices-style arrays out:
        (extremum index per keypoint, orientation per keypoint, keypoints [m,5])."""
        data = np.ascontiguousarray(extremum_data, np.float32)
        idx = np.ascontiguousarray(indices, np.uint32)
        kei = np.empty(max(max_out, 1), np.uint32)
        ori = np.empty(max(max_out, 1), np.float32)
        kps = np.empty((max(max_out, 1), 5), np.float32)
        m, dropped = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.L.lf_mkd_orient_keypoints_blocked(self._h, data.ctypes.data, n_extrema, block_len, idx.ctypes.data,
                                                           len(idx), kei.ctypes.data, ori.ctypes.data, kps.ctypes.data,
                                                           max_out, ctypes.byref(m), ctypes.byref(dropped)),
                    "lf_mkd_orient_keypoints_blocked")
        return kei[:m.value].copy(), ori[:m.value].copy(), kps[:m.value].copy(), dropped.value

    def coarse_layer(self, layer, width, height):
        out = np.empty((height, width), np.float32)
        self._check(self.L.lf_mkd_get_coarse_layer(self._h, layer, out.ctypes.data), "lf_mkd_get_coarse_layer")
        return out

    def pyramid_level(self, level):
        w, h = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self.L.lf_mkd_get_pyramid_level(self._h, level, None, ctypes.byref(w), ctypes.byref(h)),
                    "lf_mkd_get_pyramid_level")
        out = np.empty((h.value, w.value), np.float32)
        self._check(self.L.lf_mkd_get_pyramid_level(self._h, level, out.ctypes.data, None, None),
                    "lf_mkd_get_pyramid_level")
        return out

    def pyramid_level_apron(self, level):
        """(level with its mirrored apron [(h + 2a), (w + 2a)], a)."""
        w, h, a = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self.L.lf_mkd_get_pyramid_level_apron(self._h, level, None, ctypes.byref(w), ctypes.byref(h),
                                                          ctypes.byref(a)), "lf_mkd_get_pyramid_level_apron")
        out = np.empty((h.value + 2 * a.value, w.value + 2 * a.value), np.float32)
        self._check(self.L.lf_mkd_get_pyramid_level_apron(self._h, level, out.ctypes.data, None, None, None),
                    "lf_mkd_get_pyramid_level_apron")
        return out, a.value

    # --- device-pointer entry points ---------------------------------------------------------
    # `stream`: a HIP stream handle (e.g. torch.cuda.Stream().cuda_stream) on which the work is enqueued, in order with
    # whatever the caller has enqueued there.  None / 0 selects the handle's OWN non-blocking stream (lf_mkd.h), which is
    # NOT ordered with torch's streams -- and 0 is also what torch's default stream reports as its handle.  So that the
    # default is safe for torch callers, a call without a stream first waits for the device (the inputs a torch kernel is
    # still producing are complete) and returns only when its own work is done: synchronous, like the host-pointer
    # entry points.  Callers that want asynchrony pass a real stream.
    def _device_call(self, stream, fn, what):
        own = not stream
        if own:
            import sys
            t = sys.modules.get("torch")
            if t is not None and t.cuda.is_available() and t.cuda.is_initialized():
                t.cuda.synchronize()
        self._check(fn(None if own else stream), what)
        if own:
            self.synchronize()

    def describe_patches_device(self, d_patches, n, d_out, stream=None):
        self._device_call(stream, lambda s: self.L.lf_mkd_describe_patches_device(self._h, d_patches, n, d_out, s),
                          "lf_mkd_describe_patches_device")

    def raw_descriptors_device(self, d_patches, n, d_raw, stream=None):
        self._device_call(stream, lambda s: self.L.lf_mkd_raw_descriptors_device(self._h, d_patches, n, d_raw, s),
                          "lf_mkd_raw_descriptors_device")

    def set_image_device(self, d_image, width, height, stream=None):
        self._device_call(stream, lambda s: self.L.lf_mkd_set_image_device(self._h, d_image, width, height, s),
                          "lf_mkd_set_image_device")

    def set_images_device(self, d_images, n_frames, width, height, stream=None):
        self._device_call(stream, lambda s: self.L.lf_mkd_set_images_device(self._h, d_images, n_frames, width, height, s),
                          "lf_mkd_set_images_device")

    def set_images_u8_device(self, d_images, n_frames, width, height, stream=None):
        self._device_call(stream, lambda s: self.L.lf_mkd_set_images_u8_device(self._h, d_images, n_frames, width, height, s),
                          "lf_mkd_set_images_u8_device")

    def describe_keypoints_frames_device(self, d_kps, d_frame_of_kp, n, d_out, stream=None):
        self._device_call(stream, lambda s: self.L.lf_mkd_describe_keypoints_frames_device(self._h, d_kps, d_frame_of_kp, n,
                                                                                         d_out, s),
                          "lf_mkd_describe_keypoints_frames_device")

    def describe_keypoints_device(self, d_kps, n, d_out, stream=None):
        self._device_call(stream, lambda s: self.L.lf_mkd_describe_keypoints_device(self._h, d_kps, n, d_out, s),
                          "lf_mkd_describe_keypoints_device")

    def orient_keypoints_device(self, d_extrema, d_frame_of_extremum, n, d_out, d_frame_of_kp, max_out, stream=None):
        """Returns (written, dropped); waits for the stream (the count comes back to the host)."""
        m, dropped = ctypes.c_uint64(), ctypes.c_uint64()
        self._device_call(stream, lambda s: self.L.lf_mkd_orient_keypoints_device(
            self._h, d_extrema, d_frame_of_extremum, n, d_out, d_frame_of_kp, max_out, ctypes.byref(m),
            ctypes.byref(dropped), s), "lf_mkd_orient_keypoints_device")
        return m.value, dropped.value

    def detect_extrema_device(self, d_out, d_frame_of, max_out, stream=None):
        m, dropped = ctypes.c_uint64(), ctypes.c_uint64()
        self._device_call(stream, lambda s: self.L.lf_mkd_detect_extrema_device(
            self._h, d_out, d_frame_of, max_out, ctypes.byref(m), ctypes.byref(dropped), s), "lf_mkd_detect_extrema_device")
        return m.value, dropped.value

    def filter_extrema_device(self, d_extrema, n, top_n, min_size, d_out, d_index=None, stream=None):
        m = ctypes.c_uint64()
        self._device_call(stream, lambda s: self.L.lf_mkd_filter_extrema_device(
            self._h, d_extrema, n, top_n, min_size, d_out, d_index, ctypes.byref(m), s), "lf_mkd_filter_extrema_device")
        return m.value

    def match_device(self, d_a, na, d_b, nb, d_match, ratio=0.8, d_exclude_lo=None, d_exclude_hi=None, d_best=None,
                     d_second=None, stream=None):
        self._device_call(stream, lambda s: self.L.lf_mkd_match_device(
            self._h, d_a, na, d_b, nb, d_exclude_lo, d_exclude_hi, ratio, d_match, d_best, d_second, s), "lf_mkd_match_device")

    def quantize_descriptors_device(self, d_desc, n, d_q, scale=Q8_SCALE, stream=None):
        """lf_mkd_quantize_descriptors_device: d_desc [n][128] f32 -> d_q [n][128] uint8"""
        self._device_call(stream, lambda s: self.L.lf_mkd_quantize_descriptors_device(self._h, d_desc, n, scale, d_q, s),
                          "lf_mkd_quantize_descriptors_device")

    def match_q8_device(self, d_a, na, d_b, nb, d_match, ratio=0.8, d_exclude_lo=None, d_exclude_hi=None, d_best=None,
                        d_second=None, stream=None):
        """lf_mkd_match_q8_device: match_device over 8-bit rows; d_best / d_second are int32 (exact integer similarities)"""
        self._device_call(stream, lambda s: self.L.lf_mkd_match_q8_device(
            self._h, d_a, na, d_b, nb, d_exclude_lo, d_exclude_hi, ratio, d_match, d_best, d_second, s), "lf_mkd_match_q8_device")

    def knn_q8_device(self, d_a, na, d_b, nb, k, d_index, d_score=None, d_exclude_lo=None, d_exclude_hi=None, stream=None):
        """lf_mkd_knn_q8_device: d_index / d_score [na][k] int32, each a row's k best b rows (exact integer similarities)"""
        self._device_call(stream, lambda s: self.L.lf_mkd_knn_q8_device(
            self._h, d_a, na, d_b, nb, d_exclude_lo, d_exclude_hi, k, d_index, d_score, s), "lf_mkd_knn_q8_device")

    def match_q8_grouped_device(self, d_a, na, d_b, nb, d_group_of_b, d_match, ratio=0.8, d_exclude_lo=None, d_exclude_hi=None,
                                d_best=None, d_rival=None, stream=None):
        """lf_mkd_match_q8_grouped_device: d_match / d_best / d_rival [na] int32; the rival is the best score among the b rows
        whose group (d_group_of_b [nb] uint32) differs from the best's"""
        self._device_call(stream, lambda s: self.L.lf_mkd_match_q8_grouped_device(
            self._h, d_a, na, d_b, nb, d_group_of_b, d_exclude_lo, d_exclude_hi, ratio, d_match, d_best, d_rival, s),
            "lf_mkd_match_q8_grouped_device")

    def vote_groups_device(self, d_match, na, d_group_of_b, nb, n_groups_b, d_votes, d_group_of_a=None, n_groups_a=1, stream=None):
        """lf_mkd_vote_groups_device: d_votes [n_groups_a][n_groups_b] uint32, zeroed and then counted"""
        self._device_call(stream, lambda s: self.L.lf_mkd_vote_groups_device(
            self._h, d_match, na, d_group_of_a, n_groups_a, d_group_of_b, nb, n_groups_b, d_votes, s), "lf_mkd_vote_groups_device")

    def match_both_device(self, d_a, na, d_b, nb, d_match_ab, d_match_ba, ratio=0.8, stream=None):
        """both directions in one call: match_ab [na] = match(a, b), match_ba [nb] = match(b, a)"""
        self._device_call(stream, lambda s: self.L.lf_mkd_match_both_device(self._h, d_a, na, d_b, nb, ratio, d_match_ab,
                                                                             d_match_ba, s), "lf_mkd_match_both_device")

    def match_pairs_device(self, d_a, d_offsets_a, na_total, d_b, d_offsets_b, nb_total, n_pairs, d_match_ab, d_match_ba=None,
                           ratio=0.8, flags=0, d_best=None, d_second=None, stream=None):
        """lf_mkd_match_pairs_device: n_pairs match problems in one launch, laid out as the batched verifiers take them
        (device pointers; see include/lf_mkd.h).  flags: MATCH_MUTUAL."""
        self._device_call(stream, lambda s: self.L.lf_mkd_match_pairs_device(
            self._h, d_a, d_offsets_a, na_total, d_b, d_offsets_b, nb_total, n_pairs, ratio, flags, d_match_ab, d_match_ba,
            d_best, d_second, s), "lf_mkd_match_pairs_device")

    def match_q8_pairs_device(self, d_a, d_offsets_a, na_total, d_b, d_offsets_b, nb_total, n_pairs, d_match_ab, d_match_ba=None,
                              ratio=0.8, flags=0, d_best=None, d_second=None, stream=None):
        """lf_mkd_match_q8_pairs_device: match_pairs_device over 8-bit rows, each pair decided as match_q8_device decides it
        alone; d_best / d_second are int32 (device pointers; see include/lf_mkd.h).  flags: MATCH_MUTUAL."""
        self._device_call(stream, lambda s: self.L.lf_mkd_match_q8_pairs_device(
            self._h, d_a, d_offsets_a, na_total, d_b, d_offsets_b, nb_total, n_pairs, ratio, flags, d_match_ab, d_match_ba,
            d_best, d_second, s), "lf_mkd_match_q8_pairs_device")

    def edge_layout_device(self, d_image_offsets, n_images, n_rows_total, d_edge_image, n_edges, d_edge_offsets, stream=None):
        """lf_mkd_edge_layout_device: d_edge_offsets [n_edges + 1] uint64 = the exclusive prefix sum of the row counts of the
        images d_edge_image [n_edges] uint32 names in the pool (d_image_offsets [n_images + 1] uint64); one call per side"""
        self._device_call(stream, lambda s: self.L.lf_mkd_edge_layout_device(
            self._h, d_image_offsets, n_images, n_rows_total, d_edge_image, n_edges, d_edge_offsets, s), "lf_mkd_edge_layout_device")

    def gather_edge_rows_device(self, d_src, row_bytes, d_image_offsets, n_images, n_rows_total, d_edge_image, d_edge_offsets,
                                capacity_rows, n_edges, d_dst, stream=None):
        """lf_mkd_gather_edge_rows_device: the rows (row_bytes each, a multiple of 4 up to 512) of every edge's image from the
        pool d_src into the edge layout d_dst [capacity_rows]"""
        self._device_call(stream, lambda s: self.L.lf_mkd_gather_edge_rows_device(
            self._h, d_src, row_bytes, d_image_offsets, n_images, n_rows_total, d_edge_image, d_edge_offsets, capacity_rows,
            n_edges, d_dst, s), "lf_mkd_gather_edge_rows_device")

    def match_q8_edges_device(self, d_a, d_image_offsets_a, n_images_a, na_total, d_b, d_image_offsets_b, n_images_b, nb_total,
                              d_edge_a, d_edge_b, d_edge_offsets_a, ea_capacity, n_edges, d_match_ab, d_edge_offsets_b=None,
                              eb_capacity=0, d_match_ba=None, ratio=0.8, flags=0, d_best=None, d_second=None, stream=None):
        """lf_mkd_match_q8_edges_device: edge e = image d_edge_a[e] of pool a against image d_edge_b[e] of pool b, each decided
        as match_q8_device decides the two images alone; the outputs live in the edge layouts (device pointers; see
        include/lf_mkd.h).  flags: MATCH_MUTUAL."""
        self._device_call(stream, lambda s: self.L.lf_mkd_match_q8_edges_device(
            self._h, d_a, d_image_offsets_a, n_images_a, na_total, d_b, d_image_offsets_b, n_images_b, nb_total, d_edge_a,
            d_edge_b, d_edge_offsets_a, ea_capacity, d_edge_offsets_b, eb_capacity, n_edges, ratio, flags, d_match_ab, d_match_ba,
            d_best, d_second, s), "lf_mkd_match_q8_edges_device")

    def build_tracks_device(self, d_image_offsets, n_images, n_rows_total, d_edge_a, d_edge_b, d_edge_offsets_a, ea_capacity,
                            n_edges, d_match, d_track, d_track_len=None, d_track_dup=None, flags=0, stream=None):
        """lf_mkd_build_tracks_device: d_track [n_rows_total] int32 = the smallest pool row of every row's connected component
        under the links d_match holds in the a side's edge layout; d_track_len / d_track_dup [n_rows_total] uint32, per label
        the track's rows and its conflicting rows (device pointers; see include/lf_mkd.h).  flags: TRACKS_ACCUMULATE."""
        self._device_call(stream, lambda s: self.L.lf_mkd_build_tracks_device(
            self._h, d_image_offsets, n_images, n_rows_total, d_edge_a, d_edge_b, d_edge_offsets_a, ea_capacity, n_edges, d_match,
            flags, d_track, d_track_len, d_track_dup, s), "lf_mkd_build_tracks_device")

    def track_table_device(self, d_image_offsets, n_images, n_rows_total, d_track, d_track_len, d_track_dup, min_len, flags,
                           track_capacity, obs_capacity, d_track_offsets, d_obs_row, d_obs_image, d_row_track, d_counts,
                           stream=None):
        """lf_mkd_track_table_device: the CSR table of the tracks d_track / d_track_len / d_track_dup [n_rows_total] describe
        -- d_track_offsets [track_capacity + 1] uint64, d_obs_row int32 and d_obs_image uint32 (nullable) [obs_capacity],
        d_row_track int32 [n_rows_total] (nullable), d_counts uint32 [4] (device pointers; see include/lf_mkd.h).  flags:
        TRACK_TABLE_CONSISTENT."""
        self._device_call(stream, lambda s: self.L.lf_mkd_track_table_device(
            self._h, d_image_offsets, n_images, n_rows_total, d_track, d_track_len, d_track_dup, min_len, flags, track_capacity,
            obs_capacity, d_track_offsets, d_obs_row, d_obs_image, d_row_track, d_counts, s), "lf_mkd_track_table_device")

    def gather_track_rows_device(self, d_src, row_bytes, n_rows_total, d_obs_row, d_counts, obs_capacity, d_dst, stream=None):
        """lf_mkd_gather_track_rows_device: d_dst row k = d_src row d_obs_row[k] for k < min(d_counts[1], obs_capacity), rows
        of row_bytes bytes (a multiple of 4 up to 512); an index outside the pool gives a zero row"""
        self._device_call(stream, lambda s: self.L.lf_mkd_gather_track_rows_device(
            self._h, d_src, row_bytes, n_rows_total, d_obs_row, d_counts, obs_capacity, d_dst, s),
            "lf_mkd_gather_track_rows_device")

    def link_table_device(self, d_image_offsets, n_images, n_rows_total, d_edge_a, d_edge_b, d_edge_offsets_a, ea_capacity,
                          n_edges, d_match, min_links, flags, link_capacity, d_link_offsets, d_link_a, d_link_b, d_link_edge,
                          d_edge_links, d_match_kept, d_counts, stream=None):
        """lf_mkd_link_table_device: the CSR table of the links d_match holds in the a side's edge layout -- d_link_offsets
        [n_edges + 1] uint64, d_link_a / d_link_b int32 and d_link_edge uint32 (nullable) [link_capacity], d_edge_links uint32
        [n_edges] (nullable), d_match_kept int32 like d_match (nullable; may be d_match), d_counts uint32 [4] (device pointers;
        see include/lf_mkd.h).  flags: LINK_TABLE_LOCAL."""
        self._device_call(stream, lambda s: self.L.lf_mkd_link_table_device(
            self._h, d_image_offsets, n_images, n_rows_total, d_edge_a, d_edge_b, d_edge_offsets_a, ea_capacity, n_edges, d_match,
            min_links, flags, link_capacity, d_link_offsets, d_link_a, d_link_b, d_link_edge, d_edge_links, d_match_kept,
            d_counts, s), "lf_mkd_link_table_device")

    def select_edges_device(self, d_votes, n_a, n_b, k, min_votes, flags, edge_capacity, d_rank, d_rank_votes, d_edge_a, d_edge_b,
                            d_edge_votes, d_counts, stream=None):
        """lf_mkd_select_edges_device: per row of d_votes [n_a][n_b] uint32 its k best columns (larger votes first, among
        equal ones the lower column) -- d_rank int32 / d_rank_votes uint32 [n_a][k] (nullable) -- and the edges those picks
        make, d_edge_a / d_edge_b / d_edge_votes (nullable) uint32 [edge_capacity] padded with 0xFFFFFFFF, d_counts uint32 [4]
        (device pointers; see include/lf_mkd.h).  flags: SELECT_SKIP_SELF, SELECT_UNIQUE."""
        self._device_call(stream, lambda s: self.L.lf_mkd_select_edges_device(
            self._h, d_votes, n_a, n_b, k, min_votes, flags, edge_capacity, d_rank, d_rank_votes, d_edge_a, d_edge_b,
            d_edge_votes, d_counts, s), "lf_mkd_select_edges_device")

    def covisibility_device(self, d_track_offsets, track_capacity, d_obs_image, obs_capacity, d_table_counts, n_images, d_edge_a,
                            d_edge_b, n_edges, flags, d_covis, stream=None):
        """lf_mkd_covisibility_device: d_covis uint32 [n_images][n_images] = per pair of images the tracks of the table
        d_track_offsets uint64 [track_capacity + 1] / d_obs_image uint32 [obs_capacity] / d_table_counts (lf_mkd_track_table_device's
        outputs) that both see, the diagonal the tracks an image sees; the pairs d_edge_a / d_edge_b uint32 [n_edges] (nullable)
        name are zeroed (device pointers; see include/lf_mkd.h).  flags: COVIS_ACCUMULATE."""
        self._device_call(stream, lambda s: self.L.lf_mkd_covisibility_device(
            self._h, d_track_offsets, track_capacity, d_obs_image, obs_capacity, d_table_counts, n_images, d_edge_a, d_edge_b,
            n_edges, flags, d_covis, s), "lf_mkd_covisibility_device")

    def two_view_pose_device(self, d_kps, n_rows_total, d_edge_a, d_edge_b, n_edges, d_intrinsics, n_images, d_F, d_link_offsets,
                             d_link_a, d_link_b, link_capacity, d_R, d_t, d_stats, d_sigma=None, d_points=None,
                             min_parallax_deg=1.0, flags=0, stream=None):
        """lf_mkd_two_view_pose_device: per edge the relative pose its F gives under d_intrinsics [n_images][4] (fx, fy, cx,
        cy), voted by the edge's links (a link table of pool rows) -- d_R f32 [n_edges][9], d_t f32 [n_edges][3], d_stats
        uint32 [n_edges][4], d_sigma f32 [n_edges][3] (nullable), d_points f32 [link_capacity][4] (nullable) (device
        pointers; see include/lf_mkd.h)."""
        self._device_call(stream, lambda s: self.L.lf_mkd_two_view_pose_device(
            self._h, d_kps, n_rows_total, d_edge_a, d_edge_b, n_edges, d_intrinsics, n_images, d_F, d_link_offsets, d_link_a,
            d_link_b, link_capacity, min_parallax_deg, flags, d_R, d_t, d_stats, d_sigma, d_points, s),
            "lf_mkd_two_view_pose_device")

    def triangulate_tracks_device(self, d_kps, n_rows_total, d_track_offsets, track_capacity, d_obs_row, d_obs_image,
                                  obs_capacity, d_table_counts, d_intrinsics, d_poses, n_images, d_points, d_stats, d_err=None,
                                  d_obs_state=None, max_reproj_px=4.0, rounds=2, flags=0, stream=None):
        """lf_mkd_triangulate_tracks_device: per track of the table d_track_offsets uint64 [track_capacity + 1] / d_obs_row int32
        / d_obs_image uint32 [obs_capacity] / d_table_counts (lf_mkd_track_table_device's outputs) its 3-D point under
        d_intrinsics [n_images][4] and d_poses [n_images][12] (R row-major, then t; world to camera) -- d_points f32
        [track_capacity][4], d_stats uint32 [track_capacity][4], d_err f32 [track_capacity][2] (nullable), d_obs_state uint32
        [obs_capacity] (nullable) (device pointers; see include/lf_mkd.h)."""
        self._device_call(stream, lambda s: self.L.lf_mkd_triangulate_tracks_device(
            self._h, d_kps, n_rows_total, d_track_offsets, track_capacity, d_obs_row, d_obs_image, obs_capacity, d_table_counts,
            d_intrinsics, d_poses, n_images, max_reproj_px, rounds, flags, d_points, d_stats, d_err, d_obs_state, s),
            "lf_mkd_triangulate_tracks_device")

    def resect_cameras_device(self, d_kps, d_image_offsets, n_images, n_rows_total, d_row_track, d_points, track_capacity,
                              d_table_counts, d_intrinsics, d_poses, d_poses_out, d_stats, d_err=None, d_row_state=None,
                              max_reproj_px=4.0, min_parallax_deg=0.0, n_samples=512, min_inliers=12, rounds=3, seed=0, flags=0,
                              stream=None):
        """lf_mkd_resect_cameras_device: per image that is not registered (an all-zero R in d_poses [n_images][12]; every image
        with RESECT_ALL) its pose from the keypoints it owns (d_image_offsets uint64 [n_images + 1] over d_kps) in tracks with a
        point (d_row_track int32 [n_rows_total], d_points f32 [track_capacity][4], d_table_counts) under d_intrinsics
        [n_images][4] -- d_poses_out f32 [n_images][12] (may be d_poses), d_stats uint32 [n_images][4], d_err f32 [n_images][2]
        (nullable), d_row_state uint32 [n_rows_total] (nullable) (device pointers; see include/lf_mkd.h)."""
        self._device_call(stream, lambda s: self.L.lf_mkd_resect_cameras_device(
            self._h, d_kps, d_image_offsets, n_images, n_rows_total, d_row_track, d_points, track_capacity, d_table_counts,
            d_intrinsics, d_poses, max_reproj_px, min_parallax_deg, n_samples, min_inliers, rounds, seed & 0xFFFFFFFF, flags,
            d_poses_out, d_stats, d_err, d_row_state, s), "lf_mkd_resect_cameras_device")

    def track_descriptors_device(self, d_q, n_rows_total, d_track_offsets, track_capacity, d_obs_row, obs_capacity, d_table_counts,
                                 d_desc, d_desc_stats=None, d_obs_state=None, min_state=2, d_points=None, min_parallax_deg=0.0,
                                 scale=Q8_SCALE, stream=None):
        """lf_mkd_track_descriptors_device: per track of the table d_track_offsets uint64 [track_capacity + 1] / d_obs_row int32
        [obs_capacity] / d_table_counts (lf_mkd_track_table_device's outputs) one 8-bit row from the rows d_q uint8
        [n_rows_total][128] of its observations (d_obs_state uint32 [obs_capacity], nullable: those of at least min_state;
        d_points f32 [track_capacity][4], nullable: the tracks whose point passes resection's rule) -- d_desc uint8
        [track_capacity][128], d_desc_stats int32 [track_capacity][2] (nullable) (device pointers; see include/lf_mkd.h)."""
        self._device_call(stream, lambda s: self.L.lf_mkd_track_descriptors_device(
            self._h, d_q, n_rows_total, d_track_offsets, track_capacity, d_obs_row, obs_capacity, d_table_counts, d_obs_state,
            min_state, d_points, min_parallax_deg, scale, d_desc, d_desc_stats, s), "lf_mkd_track_descriptors_device")

    def view_graph_device(self, d_edge_a, d_edge_b, n_edges, d_R, d_pose_stats, n_images, d_rotations, d_edge_stats,
                          d_image_stats, d_counts, d_edge_residual=None, d_edge_offsets_a=None, ea_capacity=0, d_match=None,
                          d_match_out=None, max_loop_deg=3.0, min_front=0, root=VIEW_GRAPH_AUTO_ROOT, tree_rounds=16,
                          iterations=10, flags=0, stream=None):
        """lf_mkd_view_graph_device: the triangle vote over the posed edges (d_edge_a / d_edge_b uint32 [n_edges], d_R f32
        [n_edges][9], d_pose_stats uint32 [n_edges][4]), the images' global rotations by a tree and quaternion averaging over
        the kept edges -- d_rotations f32 [n_images][9], d_edge_stats uint32 [n_edges][4], d_image_stats uint32 [n_images][4],
        d_counts uint32 [8], d_edge_residual f32 [n_edges] (nullable), and with d_edge_offsets_a / ea_capacity / d_match the
        filtered d_match_out (may be d_match) (device pointers; see include/lf_mkd.h)."""
        self._device_call(stream, lambda s: self.L.lf_mkd_view_graph_device(
            self._h, d_edge_a, d_edge_b, n_edges, d_R, d_pose_stats, n_images, max_loop_deg, min_front, root, tree_rounds,
            iterations, flags, d_edge_offsets_a, ea_capacity, d_match, d_match_out, d_rotations, d_edge_stats, d_edge_residual,
            d_image_stats, d_counts, s), "lf_mkd_view_graph_device")

    def tree_poses_device(self, d_edge_a, d_edge_b, d_t, n_edges, d_rotations, d_image_stats, n_images, d_poses, max_depth=64,
                          stream=None):
        """lf_mkd_tree_poses_device: initial poses d_poses f32 [n_images][12] from the view graph's rotations, its tree
        (d_image_stats uint32 [n_images][4]) and the tree edges' translations d_t f32 [n_edges][3] (device pointers; see
        include/lf_mkd.h)."""
        self._device_call(stream, lambda s: self.L.lf_mkd_tree_poses_device(
            self._h, d_edge_a, d_edge_b, d_t, n_edges, d_rotations, d_image_stats, n_images, max_depth, d_poses, s),
            "lf_mkd_tree_poses_device")

    def global_positions_device(self, d_kps, d_image_offsets, n_images, n_rows_total, d_track_offsets, track_capacity, d_obs_row,
                                d_obs_image, obs_capacity, d_table_counts, d_row_track, d_intrinsics, d_poses, d_poses_out,
                                d_image_stats, d_counts, d_points_out=None, d_obs_state=None, d_trace=None, sweeps=50, warm=3,
                                robust_deg=0.2, min_obs=2, flags=0, stream=None):
        """lf_mkd_global_positions_device: all camera centres and all track points at once under the rotations of d_poses
        [n_images][12] -- d_poses_out (may be d_poses), d_image_stats uint32 [n_images][4], d_counts uint32 [8], and the
        optional d_points_out f32 [track_capacity][4], d_obs_state uint32 [obs_capacity] and d_trace f64 [sweeps][4] (device
        pointers; see include/lf_mkd.h)."""
        self._device_call(stream, lambda s: self.L.lf_mkd_global_positions_device(
            self._h, d_kps, d_image_offsets, n_images, n_rows_total, d_track_offsets, track_capacity, d_obs_row, d_obs_image,
            obs_capacity, d_table_counts, d_row_track, d_intrinsics, d_poses, sweeps, warm, robust_deg, min_obs, flags, d_poses_out,
            d_points_out, d_obs_state, d_image_stats, d_trace, d_counts, s), "lf_mkd_global_positions_device")

    def bundle_adjust_device(self, d_kps, d_image_offsets, n_images, n_rows_total, d_track_offsets, track_capacity, d_obs_row,
                             d_obs_image, obs_capacity, d_table_counts, d_points, d_intrinsics, d_poses, d_poses_out, d_points_out,
                             d_trace, d_counts, d_obs_state=None, d_camera_fixed=None, d_obs_state_out=None, max_reproj_px=4.0,
                             lambda0=1e-3, iterations=10, cg_iterations=10, cg_tol=0.1, flags=0, stream=None):
        """lf_mkd_bundle_adjust_device: Levenberg-Marquardt over the free cameras of d_poses [n_images][12] and the free points
        of d_points [track_capacity][4] on the track table's observations, the reduced camera system by preconditioned
        conjugate gradients -- d_poses_out (may be d_poses), d_points_out (may be d_points), d_trace f64 [iterations][8],
        d_counts uint32 [4], d_obs_state_out uint32 [obs_capacity] (nullable); d_obs_state and d_camera_fixed uint32
        [n_images] are optional inputs (device pointers; see include/lf_mkd.h)."""
        self._device_call(stream, lambda s: self.L.lf_mkd_bundle_adjust_device(
            self._h, d_kps, d_image_offsets, n_images, n_rows_total, d_track_offsets, track_capacity, d_obs_row, d_obs_image,
            obs_capacity, d_table_counts, d_points, d_intrinsics, d_poses, d_obs_state, d_camera_fixed, max_reproj_px, lambda0,
            iterations, cg_iterations, cg_tol, flags, d_poses_out, d_points_out, d_obs_state_out, d_trace, d_counts, s),
            "lf_mkd_bundle_adjust_device")

    def bundle_adjust_intrinsics_device(self, d_kps, d_image_offsets, n_images, n_rows_total, d_track_offsets, track_capacity,
                                        d_obs_row, d_obs_image, obs_capacity, d_table_counts, d_points, d_intrinsics, d_poses,
                                        d_poses_out, d_points_out, d_intrinsics_out, d_trace, d_counts, d_obs_state=None,
                                        d_camera_fixed=None, d_camera_group=None, n_groups=1, refine=BA_REFINE_FOCAL,
                                        d_group_out=None, d_obs_state_out=None, max_reproj_px=4.0, lambda0=1e-3, iterations=10,
                                        cg_iterations=10, cg_tol=0.1, flags=0, stream=None):
        """lf_mkd_bundle_adjust_intrinsics_device: bundle_adjust_device with the intrinsics of the images that share a lens
        refined -- d_camera_group uint32 [n_images] (nullable: one group), refine = BA_REFINE_FOCAL | BA_REFINE_PRINCIPAL;
        d_intrinsics_out [n_images][4] (may be d_intrinsics), d_group_out [n_groups][3] (nullable), d_trace f64
        [iterations][9], d_counts uint32 [5] (device pointers; see include/lf_mkd.h)."""
        self._device_call(stream, lambda s: self.L.lf_mkd_bundle_adjust_intrinsics_device(
            self._h, d_kps, d_image_offsets, n_images, n_rows_total, d_track_offsets, track_capacity, d_obs_row, d_obs_image,
            obs_capacity, d_table_counts, d_points, d_intrinsics, d_poses, d_obs_state, d_camera_fixed, d_camera_group, n_groups,
            refine, max_reproj_px, lambda0, iterations, cg_iterations, cg_tol, flags, d_poses_out, d_points_out, d_intrinsics_out,
            d_group_out, d_obs_state_out, d_trace, d_counts, s), "lf_mkd_bundle_adjust_intrinsics_device")

    def match_guided_pairs_device(self, d_a, d_kps_a, d_offsets_a, na_total, d_b, d_kps_b, d_offsets_b, nb_total, d_model, n_pairs,
                                  d_match_ab, d_match_ba=None, kind=GUIDE_HOMOGRAPHY, threshold=3.0, ratio=0.8, flags=0,
                                  d_best=None, d_second=None, stream=None):
        """lf_mkd_match_guided_pairs_device: match_pairs_device with every row's candidates restricted to the rows that pass
        the verifier's inlier test with it under the pair's model d_model [n_pairs][9] (device pointers; see
        include/lf_mkd.h).  kind: GUIDE_HOMOGRAPHY / GUIDE_FUNDAMENTAL; flags: MATCH_MUTUAL."""
        self._device_call(stream, lambda s: self.L.lf_mkd_match_guided_pairs_device(
            self._h, d_a, d_kps_a, d_offsets_a, na_total, d_b, d_kps_b, d_offsets_b, nb_total, d_model, n_pairs, kind, threshold,
            ratio, flags, d_match_ab, d_match_ba, d_best, d_second, s), "lf_mkd_match_guided_pairs_device")

    def match_q8_guided_pairs_device(self, d_a, d_kps_a, d_offsets_a, na_total, d_b, d_kps_b, d_offsets_b, nb_total, d_model, n_pairs,
                                     d_match_ab, d_match_ba=None, kind=GUIDE_HOMOGRAPHY, threshold=3.0, ratio=0.8, flags=0,
                                     d_best=None, d_second=None, stream=None):
        """lf_mkd_match_q8_guided_pairs_device: match_guided_pairs_device over 8-bit rows -- the same keypoints, model, kind and
        threshold, each row decided as match_q8_device decides it over its admissible rows alone; d_best / d_second are int32
        (device pointers; see include/lf_mkd.h).  flags: MATCH_MUTUAL."""
        self._device_call(stream, lambda s: self.L.lf_mkd_match_q8_guided_pairs_device(
            self._h, d_a, d_kps_a, d_offsets_a, na_total, d_b, d_kps_b, d_offsets_b, nb_total, d_model, n_pairs, kind, threshold,
            ratio, flags, d_match_ab, d_match_ba, d_best, d_second, s), "lf_mkd_match_q8_guided_pairs_device")

    def verify_homography_device(self, d_kps_a, d_offsets_a, d_kps_b, d_offsets_b, d_match, n_pairs, d_H, d_verified, d_stats,
                                 n_hypotheses=2048, threshold=3.0, seed=0, flags=0, stream=None):
        """lf_mkd_verify_homography_device: n_pairs problems in one call (device pointers; see include/lf_mkd.h)."""
        self._device_call(stream, lambda s: self.L.lf_mkd_verify_homography_device(
            self._h, d_kps_a, d_offsets_a, d_kps_b, d_offsets_b, d_match, n_pairs, n_hypotheses, threshold, seed, flags, d_H,
            d_verified, d_stats, s), "lf_mkd_verify_homography_device")

    def verify_fundamental_device(self, d_kps_a, d_offsets_a, d_kps_b, d_offsets_b, d_match, n_pairs, d_F, d_verified, d_stats,
                                  n_hypotheses=2048, threshold=1.5, seed=0, flags=0, stream=None):
        """lf_mkd_verify_fundamental_device: n_pairs problems in one call (device pointers; see include/lf_mkd.h)."""
        self._device_call(stream, lambda s: self.L.lf_mkd_verify_fundamental_device(
            self._h, d_kps_a, d_offsets_a, d_kps_b, d_offsets_b, d_match, n_pairs, n_hypotheses, threshold, seed, flags, d_F,
            d_verified, d_stats, s), "lf_mkd_verify_fundamental_device")

    def match_overflowed(self, stream=None):
        """Rows of the latest match call that were redone by the full scan (diagnostic; waits for the call)."""
        n = ctypes.c_uint64()
        self._check(self.L.lf_mkd_match_overflowed(self._h, stream, ctypes.byref(n)), "lf_mkd_match_overflowed")
        return n.value

    def detect_frames_device(self, d_images, n_frames, width, height, top_n, min_size, d_keypoints, d_frame_of_kp,
                             d_descriptors, max_out, stream=None):
        """Batch of frames through the whole pipeline; returns (keypoints written, dropped_blobs, dropped_features)."""
        m, db, df = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._device_call(stream, lambda s: self.L.lf_mkd_detect_frames_device(
            self._h, d_images, n_frames, width, height, top_n, min_size, d_keypoints, d_frame_of_kp, d_descriptors, max_out,
            ctypes.byref(m), ctypes.byref(db), ctypes.byref(df), s), "lf_mkd_detect_frames_device")
        return m.value, db.value, df.value

    def stream_create(self, width, height, top_n, min_size, max_out, d_image, d_keypoints, d_descriptors, d_counts):
        """Records the per-frame detect+describe pipeline as a hipGraph over fixed device buffers."""
        self._check(self.L.lf_mkd_stream_create(self._h, width, height, top_n, min_size, max_out, d_image, d_keypoints,
                                                d_descriptors, d_counts), "lf_mkd_stream_create")

    def stream_frame(self, stream=None):
        self._device_call(stream, lambda s: self.L.lf_mkd_stream_frame(self._h, s), "lf_mkd_stream_frame")

    def sample_patches_device(self, d_kps, n, d_patches, stream=None):
        self._device_call(stream, lambda s: self.L.lf_mkd_sample_patches_device(self._h, d_kps, n, d_patches, s),
                          "lf_mkd_sample_patches_device")

    def kernel_times(self):
        """(kernel_ms, 0.0, batches) summed since the previous call; needs FLAG_KERNEL_TIMING.
        (The second value was the separate whitening kernel before it was fused into mkd_pool.)"""
        a, b, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_uint64()
        self._check(self.L.lf_mkd_kernel_times(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n)),
                    "lf_mkd_kernel_times")
        return a.value, b.value, n.value

    def kernel_clock(self, stream=None):
        """(shader MHz sustained during the latest describe launch, lifetime of its workgroup 0 in ms); FLAG_KERNEL_TIMING."""
        mhz, ms = ctypes.c_double(), ctypes.c_double()
        self._check(self.L.lf_mkd_kernel_clock(self._h, stream, ctypes.byref(mhz), ctypes.byref(ms)), "lf_mkd_kernel_clock")
        return mhz.value, ms.value

    def synchronize(self):
        self._check(self.L.lf_mkd_synchronize(self._h), "lf_mkd_synchronize")
