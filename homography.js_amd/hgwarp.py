"""ctypes binding of lib/libhgwarp.so (C ABI: include/hgwarp.h).

Plumbing only: used by tests/, bench.py and __graft_entry__.py.  The product's host side is the drop-in JavaScript
class js/Homography.mjs over the N-API addon; this module exposes the same C entry points to Python 1:1 and adds
nothing on top (no CPU fallback: if the library or a gfx950 GPU is missing, calls raise).

The directory name contains a dot, so load this file by path:
    import importlib.util, sys
    spec = importlib.util.spec_from_file_location("hgwarp", ".../homography.js_amd/hgwarp.py")
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# HGWARP_LIB: another build of the SAME library (the sanitizer build lib/libhgwarp_asan.so, tools/run_asan.sh)
LIB_PATH = os.environ.get("HGWARP_LIB") or os.path.join(HERE, "lib", "libhgwarp.so")

HG_AFFINE, HG_PROJECTIVE = 0, 1
# sampling modes of the inverse warps (hg_set_sampling): nearest is the reference's pixel copy, bilinear is opt-in
SAMPLE_NEAREST, SAMPLE_BILINEAR = 0, 1
# formats of the source field of an inverse warp (hg_field_*): int32 pixel index / interleaved float32 (sx, sy) per output pixel
FIELD_INDEX, FIELD_COORDS = 0, 1
# element types of the planes of a bilinear remap (hg_remap_bilinear_frames_device)
ELEM_F32, ELEM_U8 = 0, 1
# blend modes of the mosaic (hg_mosaic_frames_device): the last contributor's pixel, the contributors' mean, their feathered mean
MOSAIC_LAST, MOSAIC_MEAN, MOSAIC_FEATHER = 0, 1, 2
# order statistics of the robust mosaic (hg_mosaic_robust_device), and the frames over one 64 x 4 tile it stages in LDS (HG_ROBUST_LMAX)
ROBUST_MEDIAN, ROBUST_TRIMMED, ROBUST_MIN, ROBUST_MAX = 0, 1, 2, 3
ROBUST_LMAX = 64
# (B, C) of the named cubics of the bicubic remap (hg_remap_bicubic_frames_device)
CUBIC_CATMULL_ROM, CUBIC_MITCHELL, CUBIC_BSPLINE = (0.0, 0.5), (1 / 3, 1 / 3), (1.0, 0.0)
# descriptor kinds of the matcher (hg_match_descriptors_frames_device): binary rows under the Hamming distance, byte vectors under squared L2
DESC_BITS, DESC_U8 = 0, 1
# the keypoint detector (hg_detect_describe_frames_device): the distance a keypoint keeps from the borders, the bytes of a descriptor, the direction bins
DETECT_MARGIN, DETECT_DESC_BYTES, DETECT_BINS = 16, 32, 32
# refining transforms on the pixels (hg_align_refine_frames_device): the status of a frame, the doubles of a frame's record of sums
ALIGN_CONVERGED, ALIGN_MAX_ITER, ALIGN_TOO_FEW, ALIGN_SINGULAR, ALIGN_WORSE, ALIGN_BAD_INPUT = 0, 1, 2, 3, 4, 5
ALIGN_SUMS = 66
ALIGN_INFO = np.dtype([("status", np.int32), ("updates", np.int32), ("n_valid_first", np.int32), ("n_valid_last", np.int32),
                       ("rms_first", np.float64), ("rms_last", np.float64), ("gain", np.float64), ("bias", np.float64)])
# adjusting a frame set over all pairs (hg_bundle_adjust_frames_device): the limits, the status of a call and of a frame, the doubles of a
# pair's record of sums, the records of d_info
BUNDLE_MAX_FRAMES, BUNDLE_MAX_PAIRS = 256, 8192
BUNDLE_CONVERGED, BUNDLE_MAX_ITER, BUNDLE_STALLED, BUNDLE_SINGULAR = 0, 1, 2, 3
BUNDLE_FRAME_ADJUSTED, BUNDLE_FRAME_FIXED, BUNDLE_FRAME_UNANCHORED, BUNDLE_FRAME_BAD_INPUT = 0, 1, 2, 3
BUNDLE_SUMS = 154
BUNDLE_INFO = np.dtype([("status", np.int32), ("rounds", np.int32), ("accepted", np.int32), ("n_valid_first", np.int32), ("n_valid_last", np.int32),
                        ("pad", np.int32), ("rms_first", np.float64), ("rms_last", np.float64), ("lambda_last", np.float64)])
BUNDLE_PAIR_INFO = np.dtype([("n_valid_first", np.int32), ("n_valid_last", np.int32), ("rms_first", np.float64), ("rms_last", np.float64)])
# thin-plate splines (hg_tps_solve_frames_device): the most control points of a frame, the status of a frame, the doubles in front of a record's points
TPS_MAX_POINTS = 1024
TPS_OK, TPS_SINGULAR, TPS_BAD_INPUT = 0, 1, 2
TPS_HEAD = 16
# camera models (hg_field_camera_frames_device): the canvas surfaces, the doubles of a frame's record, the rounds of the fixed-point undistortion
SURFACE_PLANE, SURFACE_CYLINDER, SURFACE_SPHERE = 0, 1, 2
CAMERA_RECORD_DOUBLES = 32
CAMERA_UNDISTORT_ITERS = 20

# every symbol include/hgwarp.h declares (tests check that the built library exports all of them)
EXPORTS = [
    "hg_version", "hg_device_count", "hg_create", "hg_create_on_stream", "hg_destroy", "hg_last_error", "hg_sync",
    "hg_device_alloc", "hg_device_free", "hg_copy_to_host", "hg_copy_to_device", "hg_copy_to_host_async", "hg_host_alloc", "hg_host_free", "hg_ctx_device",
    "hg_multi_create", "hg_multi_destroy", "hg_multi_last_error", "hg_multi_device_count", "hg_multi_ctx", "hg_multi_partition", "hg_multi_plan_fanout", "hg_multi_peer_note", "hg_multi_peer_access", "hg_multi_set_image",
    "hg_multi_piecewise_set_mesh", "hg_multi_warp_piecewise_batch", "hg_multi_warp_geometric_batch", "hg_multi_warp_piecewise_batch_images",
    "hg_multi_warp_geometric_batch_images", "hg_multi_frame", "hg_enqueue_copy_to_host", "hg_stream_wait_event",
    "hg_solve_affine", "hg_invert_affine", "hg_solve_projective", "hg_transform_limits", "hg_minmax_xy", "hg_js_round",
    "hg_triangulate",
    "hg_set_image", "hg_set_image_device", "hg_set_images_device",
    "hg_warp_inverse_geometric", "hg_warp_inverse_geometric_device", "hg_geometric_set_frames", "hg_geometric_set_frames_points", "hg_get_geometric_matrices",
    "hg_warp_inverse_geometric_frames_device", "hg_warp_inverse_geometric_batch_device", "hg_pack_offsets",
    "hg_piecewise_set_mesh", "hg_piecewise_prepare", "hg_warp_inverse_piecewise", "hg_warp_inverse_piecewise_device",
    "hg_piecewise_set_frames", "hg_warp_inverse_piecewise_frames_device", "hg_warp_inverse_piecewise_batch_device",
    "hg_piecewise_set_frames_src", "hg_warp_inverse_piecewise_src_batch_device", "hg_piecewise_frame_min_src",
    "hg_get_tri_map", "hg_get_tri_map_fused", "hg_get_matrices", "hg_warp_inverse_piecewise_via_map",
    "hg_warp_forward_geometric", "hg_warp_forward_piecewise", "hg_warp_forward_geometric_device", "hg_warp_forward_geometric_batch_device",
    "hg_warp_forward_piecewise_device", "hg_warp_forward_piecewise_batch_device",
    "hg_solve_affine_triangles", "hg_warp_inverse_piecewise_state", "hg_warp_forward_piecewise_state",
    "hg_upload_on_copy_stream", "hg_fence_copies", "hg_download_behind_warps", "hg_fence_downloads",
    "hg_set_timing", "hg_last_kernel_ms", "hg_kernel_ms_stats", "hg_last_piecewise_kernel", "hg_last_piecewise_variant", "hg_last_geometric_kernel", "hg_last_piecewise_self", "hg_last_piecewise_flag", "hg_last_forward_kernel", "hg_forward_tiles_admissible", "hg_redone_frames", "hg_layout_walks", "hg_span_cache_stats", "hg_set_option", "hg_xcc_count", "hg_selftest_division", "hg_projective_plain_range", "hg_affine_one_fma_form",
    "hg_set_sampling", "hg_get_sampling", "hg_multi_set_sampling",
    "hg_pack_field_offsets", "hg_field_inverse_geometric", "hg_field_inverse_geometric_device", "hg_field_inverse_geometric_frames_device",
    "hg_field_inverse_piecewise", "hg_field_inverse_piecewise_frames_device", "hg_remap_index_device", "hg_remap_bilinear_f32_device",
    "hg_field_forward_geometric", "hg_field_forward_geometric_batch_device", "hg_field_forward_piecewise", "hg_field_forward_piecewise_batch_device",
    "hg_last_forward_field_kernel",
    "hg_pack_plane_offsets", "hg_remap_index_frames_device", "hg_remap_bilinear_frames_device", "hg_remap_bilinear_u8_device",
    "hg_points_to_source_geometric_frames_device", "hg_points_to_source_piecewise_frames_device",
    "hg_points_to_output_geometric_batch_device", "hg_points_to_output_piecewise_batch_device",
    "hg_pyramid_levels", "hg_pyramid_layout", "hg_pyramid_build_device", "hg_remap_trilinear_frames_device", "hg_remap_aniso_frames_device",
    "hg_mosaic_frames_device", "hg_mosaic_overlap_stats_device", "hg_mosaic_solve_gains", "hg_mosaic_frames_gain_device",
    "hg_remap_bicubic_frames_device",
    "hg_fit_sample_indices", "hg_fit_matches_frames_device",
    "hg_align_scale_matrix", "hg_align_refine_frames_device",
    "hg_bundle_layout", "hg_bundle_adjust_frames_device", "hg_bundle_chain_from_pairs", "hg_bundle_invert_matrix",
    "hg_tps_layout", "hg_tps_solve_frames_device", "hg_tps_field_layout", "hg_field_tps_frames_device", "hg_points_tps_frames_device",
    "hg_camera_pack_record", "hg_camera_limits", "hg_camera_focals_from_matrix", "hg_camera_rotation_from_matrix",
    "hg_field_camera_frames_device", "hg_points_camera_to_source_frames_device", "hg_points_camera_to_canvas_frames_device",
    "hg_flow_layout", "hg_flow_dense_frames_device", "hg_field_compose_frames_device",
    "hg_match_descriptors_frames_device",
    "hg_detect_layout", "hg_describe_pattern", "hg_detect_describe_frames_device",
    "hg_mosaic_multiband_layout", "hg_mosaic_multiband_device",
    "hg_mosaic_robust_device",
]


class Geom(C.Structure):
    _fields_ = [("x_off", C.c_int32), ("y_off", C.c_int32), ("obj_w", C.c_int32), ("obj_h", C.c_int32)]


class TriMapDef(C.Structure):
    """hg_tri_map_def: what the reference's shared map field was rasterised from (include/hgwarp.h, reference-state forms)."""
    _fields_ = [("points", C.POINTER(C.c_float)), ("n_points", C.c_int), ("triangles", C.POINTER(C.c_uint32)), ("n_triangles", C.c_int),
                ("width", C.c_int32), ("height", C.c_int32), ("y_off", C.c_int32)]


class HgError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"hgwarp error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """Loads libhgwarp.so (raises if it has not been built: there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HgError(-1, f"{LIB_PATH} is missing: build it with `make -C homography.js_amd` (or __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    vp, i, sz, d = C.c_void_p, C.c_int, C.c_size_t, C.c_double
    f32p, f64p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    sig = {
        "hg_version": (i, []), "hg_device_count": (i, [C.POINTER(i)]),
        "hg_create": (i, [i, C.POINTER(vp)]), "hg_create_on_stream": (i, [i, vp, C.POINTER(vp)]), "hg_destroy": (None, [vp]),
        "hg_last_error": (C.c_char_p, [vp]), "hg_sync": (i, [vp]),
        "hg_device_alloc": (i, [vp, sz, C.POINTER(vp)]), "hg_device_free": (i, [vp, vp]), "hg_copy_to_host": (i, [vp, vp, vp, sz]), "hg_copy_to_device": (i, [vp, vp, vp, sz]),
        "hg_copy_to_host_async": (i, [vp, vp, vp, sz]), "hg_host_alloc": (i, [sz, C.POINTER(vp)]), "hg_host_free": (i, [vp]), "hg_ctx_device": (i, [vp]),
        "hg_multi_create": (i, [C.POINTER(i), i, C.POINTER(vp)]), "hg_multi_destroy": (None, [vp]), "hg_multi_last_error": (C.c_char_p, [vp]),
        "hg_multi_device_count": (i, [vp]), "hg_multi_ctx": (vp, [vp, i]),
        "hg_multi_partition": (i, [i, i, i, C.POINTER(i), C.POINTER(i)]),
        "hg_multi_plan_fanout": (i, [i, vp, vp, i]), "hg_multi_peer_note": (C.c_char_p, [vp]), "hg_multi_peer_access": (i, [vp, i, i]),
        "hg_multi_set_image": (i, [vp, u8p, i, i]), "hg_multi_piecewise_set_mesh": (i, [vp, f32p, i, C.POINTER(C.c_uint32), i, i, i]),
        "hg_multi_warp_piecewise_batch": (i, [vp, f32p, C.POINTER(Geom), i, C.POINTER(vp)]),
        "hg_multi_warp_geometric_batch": (i, [vp, i, f32p, f32p, C.POINTER(Geom), i, C.POINTER(vp)]),
        "hg_multi_frame": (i, [vp, i, C.POINTER(i), C.POINTER(vp), C.POINTER(sz)]),
        "hg_multi_warp_piecewise_batch_images": (i, [vp, f32p, C.POINTER(Geom), i, C.POINTER(vp), i, i, C.POINTER(vp)]),
        "hg_multi_warp_geometric_batch_images": (i, [vp, i, f32p, f32p, C.POINTER(Geom), i, C.POINTER(vp), i, i, C.POINTER(vp)]),
        "hg_enqueue_copy_to_host": (i, [vp, vp, vp, sz]), "hg_stream_wait_event": (i, [vp, vp]),
        "hg_solve_affine": (i, [f32p, f32p, f32p]), "hg_invert_affine": (i, [f32p, f32p]), "hg_solve_projective": (i, [f32p, f32p, f64p]),
        "hg_transform_limits": (i, [i, f64p, d, d, f64p]), "hg_minmax_xy": (i, [f32p, i, f64p]), "hg_js_round": (d, [d]),
        "hg_triangulate": (i, [f32p, i, C.POINTER(C.c_uint32), i, C.POINTER(i)]),
        "hg_set_image": (i, [vp, u8p, i, i]), "hg_set_image_device": (i, [vp, vp, i, i]),
        "hg_set_images_device": (i, [vp, vp, i, i, i, sz]),
        "hg_warp_inverse_geometric": (i, [vp, i, f64p, Geom, u8p]), "hg_warp_inverse_geometric_device": (i, [vp, i, f64p, Geom, vp]),
        "hg_geometric_set_frames": (i, [vp, i, f64p, C.POINTER(Geom), C.POINTER(sz), i]),
        "hg_geometric_set_frames_points": (i, [vp, i, f32p, f32p, C.POINTER(Geom), C.POINTER(sz), i]),
        "hg_get_geometric_matrices": (i, [vp, f64p, i]),
        "hg_warp_inverse_geometric_frames_device": (i, [vp, vp]),
        "hg_warp_inverse_geometric_batch_device": (i, [vp, i, f64p, C.POINTER(Geom), C.POINTER(sz), i, vp]),
        "hg_pack_offsets": (i, [C.POINTER(Geom), i, C.POINTER(sz), C.POINTER(sz)]),
        "hg_piecewise_set_mesh": (i, [vp, f32p, i, C.POINTER(C.c_uint32), i, i, i]),
        "hg_piecewise_prepare": (i, [vp, f32p, Geom]),
        "hg_warp_inverse_piecewise": (i, [vp, u8p]), "hg_warp_inverse_piecewise_device": (i, [vp, vp]),
        "hg_piecewise_set_frames": (i, [vp, f32p, C.POINTER(Geom), C.POINTER(sz), i]),
        "hg_warp_inverse_piecewise_frames_device": (i, [vp, vp]),
        "hg_warp_inverse_piecewise_batch_device": (i, [vp, f32p, C.POINTER(Geom), C.POINTER(sz), i, vp]),
        "hg_piecewise_set_frames_src": (i, [vp, f32p, C.POINTER(C.c_int32), f32p, C.POINTER(Geom), C.POINTER(sz), i]),
        "hg_warp_inverse_piecewise_src_batch_device": (i, [vp, f32p, C.POINTER(C.c_int32), f32p, C.POINTER(Geom), C.POINTER(sz), i, vp]),
        "hg_piecewise_frame_min_src": (i, [f32p, i, C.POINTER(C.c_int32)]),
        "hg_get_tri_map": (i, [vp, C.POINTER(C.c_int16), sz]), "hg_get_tri_map_fused": (i, [vp, C.POINTER(C.c_int16), sz]),
        "hg_get_matrices": (i, [vp, f32p, f32p]), "hg_warp_inverse_piecewise_via_map": (i, [vp, u8p]),
        "hg_last_piecewise_kernel": (i, [vp]), "hg_last_piecewise_variant": (i, [vp]), "hg_last_geometric_kernel": (i, [vp]), "hg_last_piecewise_self": (i, [vp]), "hg_last_piecewise_flag": (i, [vp]), "hg_last_forward_kernel": (i, [vp]), "hg_set_option": (i, [vp, C.c_char_p, i]),
        "hg_set_sampling": (i, [vp, i]), "hg_get_sampling": (i, [vp, C.POINTER(i)]), "hg_multi_set_sampling": (i, [vp, i]), "hg_redone_frames": (C.c_long, [vp]), "hg_layout_walks": (C.c_long, [vp]), "hg_xcc_count": (i, [vp]),
        "hg_span_cache_stats": (i, [vp, C.POINTER(C.c_int64)]),
        "hg_selftest_division": (i, [vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
        "hg_projective_plain_range": (i, [f64p, Geom]), "hg_affine_one_fma_form": (i, [f32p, Geom]), "hg_forward_tiles_admissible": (i, [i, f64p, i, i, Geom]),
        "hg_set_timing": (i, [vp, i]), "hg_last_kernel_ms": (i, [vp, f32p]),
        "hg_kernel_ms_stats": (i, [vp, f64p, C.POINTER(i)]),
        "hg_warp_forward_geometric": (i, [vp, i, f64p, Geom, u8p]),
        "hg_warp_forward_piecewise": (i, [vp, f32p, i, i, Geom, u8p]),
        "hg_warp_forward_geometric_device": (i, [vp, i, f64p, Geom, vp]),
        "hg_warp_forward_geometric_batch_device": (i, [vp, i, f64p, C.POINTER(Geom), C.POINTER(sz), i, vp]),
        "hg_warp_forward_piecewise_device": (i, [vp, f32p, i, i, Geom, vp]),
        "hg_warp_forward_piecewise_batch_device": (i, [vp, f32p, i, i, C.POINTER(Geom), C.POINTER(sz), i, vp]),
        "hg_upload_on_copy_stream": (i, [vp, vp, vp, sz]), "hg_fence_copies": (i, [vp]), "hg_download_behind_warps": (i, [vp, vp, vp, sz]), "hg_fence_downloads": (i, [vp]),
        "hg_solve_affine_triangles": (i, [f32p, f32p, i, C.POINTER(C.c_uint32), i, f32p]),
        "hg_pack_field_offsets": (i, [C.POINTER(Geom), i, i, C.POINTER(sz), C.POINTER(sz)]),
        "hg_field_inverse_geometric": (i, [vp, i, f64p, Geom, i, vp]), "hg_field_inverse_geometric_device": (i, [vp, i, f64p, Geom, i, vp]),
        "hg_field_inverse_geometric_frames_device": (i, [vp, i, C.POINTER(sz), vp]),
        "hg_field_inverse_piecewise": (i, [vp, i, vp]), "hg_field_inverse_piecewise_frames_device": (i, [vp, i, C.POINTER(sz), vp]),
        "hg_field_forward_geometric": (i, [vp, i, f64p, Geom, vp]),
        "hg_field_forward_geometric_batch_device": (i, [vp, i, f64p, C.POINTER(Geom), C.POINTER(sz), i, vp]),
        "hg_field_forward_piecewise": (i, [vp, f32p, i, i, Geom, vp]),
        "hg_field_forward_piecewise_batch_device": (i, [vp, f32p, i, i, C.POINTER(Geom), C.POINTER(sz), i, vp]),
        "hg_last_forward_field_kernel": (i, [vp]),
        "hg_remap_index_device": (i, [vp, vp, sz, vp, sz, i, vp]),
        "hg_remap_bilinear_f32_device": (i, [vp, vp, sz, vp, i, i, i, vp]),
        "hg_remap_bilinear_u8_device": (i, [vp, vp, sz, vp, i, i, i, vp]),
        "hg_pack_plane_offsets": (i, [C.POINTER(Geom), i, sz, C.POINTER(sz), C.POINTER(sz)]),
        "hg_remap_index_frames_device": (i, [vp, C.POINTER(Geom), i, vp, C.POINTER(sz), vp, sz, i, sz, i, vp, C.POINTER(sz)]),
        "hg_remap_bilinear_frames_device": (i, [vp, C.POINTER(Geom), i, vp, C.POINTER(sz), vp, i, i, i, sz, i, i, vp, C.POINTER(sz)]),
        "hg_pyramid_levels": (i, [i, i]),
        "hg_pyramid_layout": (i, [i, i, i, i, i, C.POINTER(sz), C.POINTER(sz)]),
        "hg_pyramid_build_device": (i, [vp, vp, i, i, i, sz, i, i, i, vp, sz]),
        "hg_remap_trilinear_frames_device": (i, [vp, C.POINTER(Geom), i, vp, C.POINTER(sz), vp, i, i, i, sz, i, i, vp, C.POINTER(sz), vp, sz, i]),
        "hg_remap_bicubic_frames_device": (i, [vp, C.POINTER(Geom), i, vp, C.POINTER(sz), vp, i, i, i, sz, i, i, vp, C.POINTER(sz), C.c_float, C.c_float]),
        "hg_remap_aniso_frames_device": (i, [vp, C.POINTER(Geom), i, vp, C.POINTER(sz), vp, i, i, i, sz, i, i, vp, C.POINTER(sz), vp, sz, i, i]),
        "hg_mosaic_frames_device": (i, [vp, C.POINTER(Geom), i, vp, C.POINTER(sz), vp, C.POINTER(sz), i, i, i, i, i, C.c_float, Geom, vp, vp]),
        "hg_mosaic_frames_gain_device": (i, [vp, C.POINTER(Geom), i, vp, C.POINTER(sz), vp, C.POINTER(sz), i, i, i, i, i, C.c_float, Geom, vp, vp, C.POINTER(C.c_float)]),
        "hg_mosaic_robust_device": (i, [vp, C.POINTER(Geom), i, vp, C.POINTER(sz), vp, C.POINTER(sz), i, i, C.c_float, C.POINTER(C.c_float), Geom, vp, vp]),
        "hg_mosaic_overlap_stats_device": (i, [vp, C.POINTER(Geom), i, vp, C.POINTER(sz), vp, C.POINTER(sz), i, Geom, vp]),
        "hg_mosaic_solve_gains": (i, [C.POINTER(C.c_uint64), i, i, C.c_double, C.c_double, C.POINTER(C.c_float)]),
        "hg_mosaic_multiband_layout": (i, [C.POINTER(Geom), i, Geom, i, i, C.POINTER(sz)]),
        "hg_mosaic_multiband_device": (i, [vp, C.POINTER(Geom), i, vp, C.POINTER(sz), vp, C.POINTER(sz), i, i, i, i, C.c_float, i, Geom, vp, vp, vp,
                                           C.POINTER(C.c_float), vp, sz]),
        "hg_fit_sample_indices": (i, [i, C.c_uint32, i, C.POINTER(C.c_int32), i, i, C.POINTER(C.c_int32)]),
        "hg_fit_matches_frames_device": (i, [vp, i, vp, i, C.POINTER(C.c_int32), i, d, i, C.c_uint32, vp, i, vp, vp, vp, vp, vp]),
        "hg_align_scale_matrix": (i, [i, f64p, i, i, f64p]),
        "hg_align_refine_frames_device": (i, [vp, i, vp, i, i, i, sz, vp, i, i, i, sz, i, i, i, i, i, i, i, i, d, i, vp, vp, vp, vp]),
        "hg_bundle_layout": (i, [i, i, i, i, C.POINTER(sz)]),
        "hg_bundle_adjust_frames_device": (i, [vp, i, i, i, i, u8p, C.POINTER(C.c_int32), i, vp, i, C.POINTER(C.c_int32), vp, i, d, d, d, vp, vp, vp,
                                               vp, vp, sz]),
        "hg_bundle_chain_from_pairs": (i, [i, i, C.POINTER(C.c_int32), i, f64p, i, f64p]),
        "hg_bundle_invert_matrix": (i, [i, f64p, f64p]),
        "hg_tps_layout": (i, [i, i, C.POINTER(sz), C.POINTER(sz)]),
        "hg_tps_solve_frames_device": (i, [vp, vp, i, vp, i, i, i, d, vp, vp, vp]),
        "hg_tps_field_layout": (i, [C.POINTER(Geom), i, i, C.POINTER(sz)]),
        "hg_field_tps_frames_device": (i, [vp, vp, i, C.POINTER(Geom), i, i, i, i, i, C.POINTER(sz), vp, vp]),
        "hg_points_tps_frames_device": (i, [vp, vp, i, i, vp, i, i, vp]),
        "hg_camera_pack_record": (i, [f64p, d, d, d, d, f64p, i, i, f64p]),
        "hg_camera_limits": (i, [f64p, i, i, i, d, d, d, C.POINTER(C.c_int32)]),
        "hg_camera_focals_from_matrix": (i, [f64p, f64p, f64p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "hg_camera_rotation_from_matrix": (i, [f64p, f64p, f64p, f64p]),
        "hg_field_camera_frames_device": (i, [vp, vp, C.POINTER(Geom), i, i, i, i, d, d, d, i, C.POINTER(sz), vp]),
        "hg_points_camera_to_source_frames_device": (i, [vp, vp, i, i, d, d, d, vp, i, i, vp]),
        "hg_points_camera_to_canvas_frames_device": (i, [vp, vp, i, i, d, d, d, vp, i, i, vp]),
        "hg_flow_layout": (i, [i, i, i, i, i, i, C.POINTER(sz)]),
        "hg_flow_dense_frames_device": (i, [vp, vp, i, sz, vp, i, sz, i, i, i, i, i, i, d, d, C.POINTER(sz), vp, vp, vp, vp, vp]),
        "hg_field_compose_frames_device": (i, [vp, C.POINTER(Geom), i, vp, C.POINTER(sz), vp, i, i, i, sz, vp, C.POINTER(sz)]),
        "hg_match_descriptors_frames_device": (i, [vp, i, i, sz, vp, i, C.POINTER(C.c_int32), i, vp, i, C.POINTER(C.c_int32), i, d, C.c_uint32, i,
                                                   vp, vp, vp, vp, vp, vp]),
        "hg_detect_layout": (i, [i, i, i, i, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "hg_describe_pattern": (i, [C.POINTER(C.c_int8)]),
        "hg_detect_describe_frames_device": (i, [vp, vp, i, i, i, sz, i, i, i, C.c_int64, sz, vp, vp, vp, vp]),
        "hg_points_to_source_geometric_frames_device": (i, [vp, vp, i, i, vp]),
        "hg_points_to_source_piecewise_frames_device": (i, [vp, vp, i, i, vp]),
        "hg_points_to_output_geometric_batch_device": (i, [vp, i, f64p, C.POINTER(Geom), i, vp, i, i, vp]),
        "hg_points_to_output_piecewise_batch_device": (i, [vp, f32p, i, i, C.POINTER(Geom), i, vp, i, i, vp]),
        "hg_warp_inverse_piecewise_state": (i, [vp, f32p, i, C.POINTER(TriMapDef), i, i, Geom, u8p]),
        "hg_warp_forward_piecewise_state": (i, [vp, f32p, i, C.POINTER(TriMapDef), i, i, i, i, Geom, u8p]),
    }
    older = "HGWARP_LIB" in os.environ       # A/B tooling (tools/ab*.sh) loads an OLDER build beside the current one: it may lack newer symbols
    for name, (res, args) in sig.items():
        if older and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def _f64(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def _geoms(gs):
    arr = (Geom * len(gs))(*[Geom(*[int(v) for v in g]) for g in gs])
    return arr


def _check(code, ctx=None):
    if code != 0:
        msg = lib().hg_last_error(ctx)
        raise HgError(code, msg.decode() if msg else "?")


# ------------------------------------------------------------------ host-side solves (no GPU needed)

def solve_affine(src, dst):
    (_, s), (_, d) = _f32(src), _f32(dst)
    out = np.empty(6, np.float32)
    _check(lib().hg_solve_affine(s, d, out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def solve_affine_triangles(src_pts, dst_pts, tris):
    """affineMatrixFromTriangles per triangle of a mesh (:785-804): (T, 6) float32, on the host."""
    (s, sp), (d, dp) = _f32(src_pts), _f32(dst_pts)
    t = np.ascontiguousarray(tris, np.uint32)
    out = np.empty((t.size // 3, 6), np.float32)
    _check(lib().hg_solve_affine_triangles(sp, dp, min(s.size, d.size) // 2, t.ctypes.data_as(C.POINTER(C.c_uint32)), t.size // 3,
                                           out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def _map_def(points, tris, width, height, y_off):
    p, pp = _f32(points)
    t = np.ascontiguousarray(tris, np.uint32)
    return TriMapDef(pp, p.size // 2, t.ctypes.data_as(C.POINTER(C.c_uint32)), t.size // 3, int(width), int(height), int(y_off)), (p, t)


def invert_affine(m):
    _, p = _f32(m)
    out = np.empty(6, np.float32)
    _check(lib().hg_invert_affine(p, out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def solve_projective(src, dst):
    (_, s), (_, d) = _f32(src), _f32(dst)
    out = np.empty(8, np.float64)
    _check(lib().hg_solve_projective(s, d, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def transform_limits(kind, m, w, h):
    _, p = _f64(m)
    out = np.empty(4, np.float64)
    _check(lib().hg_transform_limits(int(kind), p, float(w), float(h), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def minmax_xy(pts):
    a, p = _f32(pts)
    out = np.empty(4, np.float64)
    _check(lib().hg_minmax_xy(p, a.size, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def frame_min_src(src_pts):
    """(minSrcX, minSrcY) a fresh instance would hold for one frame's source points (hg_piecewise_frame_min_src)."""
    a, p = _f32(src_pts)
    out = (C.c_int32 * 2)()
    _check(lib().hg_piecewise_frame_min_src(p, a.size // 2, out))
    return int(out[0]), int(out[1])


def projective_plain_range(m, geom):
    """True if the projective kernel may use its shared-reciprocal division for this frame (host-side range proof)."""
    a = np.ascontiguousarray(m, np.float64)
    return bool(lib().hg_projective_plain_range(a.ctypes.data_as(C.POINTER(C.c_double)), Geom(*[int(v) for v in geom])))


def affine_one_fma_form(inv, geom):
    """1 where the piecewise row kernel may evaluate an inverse matrix's two sums with one fma each (hg_affine_one_fma_form)."""
    a = np.ascontiguousarray(inv, np.float32)
    return bool(lib().hg_affine_one_fma_form(a.ctypes.data_as(C.POINTER(C.c_float)), Geom(*[int(v) for v in geom])))


def forward_tiles_admissible(kind, m, w, h, geom):
    """0 = scatter + gather, 1 = k_fwd_tiles admissible, 2 = admissible with a trusted inverse (include/hgwarp.h)."""
    a = np.zeros(8, np.float64)
    mm = np.ascontiguousarray(m, np.float64).ravel()
    a[:mm.size] = mm
    return int(lib().hg_forward_tiles_admissible(int(kind), a.ctypes.data_as(C.POINTER(C.c_double)), int(w), int(h), Geom(*[int(v) for v in geom])))


def js_round(x):
    return lib().hg_js_round(float(x))


def triangulate(pts):
    """Delaunay triangles (uint32, 3 per triangle) of interleaved x,y points: where the reference calls Delaunator (:1216)."""
    a, p = _f32(pts)
    n = a.size // 2
    out = np.empty(max(2 * n, 1) * 3, np.uint32)
    cnt = C.c_int(0)
    _check(lib().hg_triangulate(p, n, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size // 3, C.byref(cnt)))
    return out[:3 * cnt.value].copy()


def pack_offsets(geoms):
    g = _geoms(geoms)
    offs = (C.c_size_t * len(geoms))()
    total = C.c_size_t(0)
    _check(lib().hg_pack_offsets(g, len(geoms), offs, C.byref(total)))
    return list(offs), total.value


def pack_field_offsets(geoms, fmt):
    """(offsets, total bytes) of the packed field layout of a frame set: 256-byte aligned starts, 4 (FIELD_INDEX) or 8 (FIELD_COORDS) bytes per pixel."""
    g = _geoms(geoms)
    offs = (C.c_size_t * max(len(geoms), 1))()
    total = C.c_size_t(0)
    _check(lib().hg_pack_field_offsets(g, len(geoms), int(fmt), offs, C.byref(total)))
    return list(offs)[:len(geoms)], total.value


def pack_plane_offsets(geoms, px_bytes):
    """(offsets, total bytes) of the packed OUTPUT layout of a frames remap: 256-byte aligned starts, px_bytes per pixel."""
    g = _geoms(geoms)
    offs = (C.c_size_t * max(len(geoms), 1))()
    total = C.c_size_t(0)
    _check(lib().hg_pack_plane_offsets(g, len(geoms), int(px_bytes), offs, C.byref(total)))
    return list(offs)[:len(geoms)], total.value


def tps_layout(n_points, n_frames):
    """(record bytes per frame, solve scratch bytes) of hg_tps_solve_frames_device: a record is 16 + 4 n_points doubles; the scratch is 0
    while the system fits LDS (n_points <= 69), else n_frames x (n_points + 3)^2 doubles."""
    rec, scr = C.c_size_t(0), C.c_size_t(0)
    _check(lib().hg_tps_layout(int(n_points), int(n_frames), C.byref(rec), C.byref(scr)))
    return rec.value, scr.value


def tps_field_layout(geoms, step):
    """Scratch bytes of hg_field_tps_frames_device at `step`: the node lattices of the frames as f64 pairs (0 at step 1)."""
    total = C.c_size_t(0)
    _check(lib().hg_tps_field_layout(_geoms(geoms) if len(geoms) else None, len(geoms), int(step), C.byref(total)))
    return total.value


def camera_pack_record(rotation, focal, principal, w, h, distortion=None):
    """hg_camera_pack_record: the 32-double record of one camera.  rotation: 3 x 3, camera <- world; focal: f or (fx, fy); principal: (cx, cy);
    distortion: (k1, k2, p1, p2, k3) or None; w, h: the picture's size (r2_max comes from its corners and edge midpoints)."""
    _, rp = _f64(np.asarray(rotation, np.float64).reshape(9))
    fx, fy = (float(focal), float(focal)) if np.isscalar(focal) else (float(focal[0]), float(focal[1]))
    dk = None
    if distortion is not None:
        dk, dp = _f64(np.asarray(distortion, np.float64).reshape(5))
    out = np.empty(CAMERA_RECORD_DOUBLES, np.float64)
    _check(lib().hg_camera_pack_record(rp, fx, fy, float(principal[0]), float(principal[1]), dp if dk is not None else None, int(w), int(h),
                                       out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def camera_limits(record, w, h, surface, scale, u0, v0):
    """hg_camera_limits: the window (x_off, y_off, w, h) of the canvas that holds the frame of `record`, one pixel of margin included."""
    _, rp = _f64(np.asarray(record, np.float64).reshape(CAMERA_RECORD_DOUBLES))
    out = (C.c_int32 * 4)()
    _check(lib().hg_camera_limits(rp, int(w), int(h), int(surface), float(scale), float(u0), float(v0), out))
    return tuple(int(v) for v in out)


def camera_focals_from_matrix(h9):
    """hg_camera_focals_from_matrix: (f_from, f_to, ok_from, ok_to) of a homography between pictures in principal-point coordinates."""
    _, hp = _f64(np.asarray(h9, np.float64).reshape(9))
    f0, f1, k0, k1 = C.c_double(0), C.c_double(0), C.c_int(0), C.c_int(0)
    _check(lib().hg_camera_focals_from_matrix(hp, C.byref(f0), C.byref(f1), C.byref(k0), C.byref(k1)))
    return f0.value, f1.value, bool(k0.value), bool(k1.value)


def camera_rotation_from_matrix(h9, k_from, k_to):
    """hg_camera_rotation_from_matrix: the rotation (3 x 3, TO camera <- FROM camera) nearest to K_to^-1 H K_from; K = (fx, fy, cx, cy)."""
    _, hp = _f64(np.asarray(h9, np.float64).reshape(9))
    _, ap = _f64(np.asarray(k_from, np.float64).reshape(4))
    _, bp = _f64(np.asarray(k_to, np.float64).reshape(4))
    out = np.empty(9, np.float64)
    _check(lib().hg_camera_rotation_from_matrix(hp, ap, bp, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out.reshape(3, 3)


def flow_layout(w, h, channels, n_frames, n_to_sets, levels):
    """Scratch bytes of hg_flow_dense_frames_device: the luma copies of 4-channel planes, the pyramids of both plane sets and two flow
    buffers per level."""
    total = C.c_size_t()
    _check(lib().hg_flow_layout(int(w), int(h), int(channels), int(n_frames), int(n_to_sets), int(levels), C.byref(total)))
    return total.value


def flow_default_levels(w, h):
    """The default number of levels of a flow: as many as leave the coarsest level at least 16 pixels on its shorter side (at least 1, at most 12)."""
    n, s = 1, min(int(w), int(h))
    while n < 12 and ((s + 1) >> 1) >= 16:
        s = (s + 1) >> 1
        n += 1
    return n


def pyramid_levels(w, h):
    """Levels of the full mip pyramid of a w x h plane: 1 + ceil(log2(max(w, h))); 0 for w or h < 1."""
    return lib().hg_pyramid_levels(int(w), int(h))


def pyramid_layout(w, h, elem, channels, levels):
    """(offsets, total bytes) of ONE pyramid buffer: offsets[k], k = 1 .. levels-1, is where level k starts (256-byte aligned); offsets[0] = 0
    is unused -- level 0 stays the caller's plane."""
    offs = (C.c_size_t * max(int(levels), 1))()
    total = C.c_size_t(0)
    _check(lib().hg_pyramid_layout(int(w), int(h), int(elem), int(channels), int(levels), offs, C.byref(total)))
    return list(offs)[:int(levels)], total.value


def mosaic_solve_gains(stats, channels, sigma_n=10.0, sigma_g=0.1):
    """One exposure gain per frame (float32, F of them) from the overlap statistics of Context.mosaic_overlap_stats_device -- an array of
    F * F * 2 uint64 --: Brown & Lowe's gain compensation, solved on the host in double.  sigma_n: the intensity error on the 0..255 scale,
    sigma_g: the prior that keeps the gains near 1 (the paper's values are the defaults HERE; the C entry has none).  Frames that cover nothing
    get 1.0."""
    st = np.ascontiguousarray(stats, dtype=np.uint64).ravel()
    n = int(round((st.size // 2) ** 0.5))
    assert n * n * 2 == st.size, "stats must hold F * F * 2 words"
    gains = np.ones(n, np.float32)
    _check(lib().hg_mosaic_solve_gains(st.ctypes.data_as(C.POINTER(C.c_uint64)) if n else None, n, int(channels), float(sigma_n), float(sigma_g),
                                       gains.ctypes.data_as(C.POINTER(C.c_float)) if n else None))
    return gains


def mosaic_multiband_layout(geoms, canvas, channels, n_bands):
    """The bytes of scratch Context.mosaic_multiband_device needs for these windows (hg_mosaic_multiband_layout): the labels, one flag byte
    per pixel of every frame's grid, levels 1..n_bands-1 of every frame's image and weight pyramids and of the blended pyramid."""
    total = C.c_size_t(0)
    _check(lib().hg_mosaic_multiband_layout(_geoms(geoms) if len(geoms) else None, len(geoms), Geom(*[int(v) for v in canvas]), int(channels), int(n_bands),
                                            C.byref(total)))
    return total.value


def _counts(counts, n_frames=None):
    """The host counts of a fit as (array or None, ctypes pointer or None, F)."""
    if counts is None:
        return None, None, int(n_frames)
    a = np.ascontiguousarray(counts, dtype=np.int32).ravel()
    return a, (a.ctypes.data_as(C.POINTER(C.c_int32)) if a.size else None), a.size


def fit_sample_indices(kind, seed, counts, n_points, n_hyp):
    """The samples the device draws for a fit with d_samples NULL (hg_fit_sample_indices): an (F, n_hyp, 4) int32 array for the F frames of
    `counts` (matches per frame), -1 in all four slots of an invalid hypothesis and in the fourth slot for affine."""
    a, p, F = _counts(counts)
    out = np.empty((F, max(int(n_hyp), 0), 4), np.int32)
    _check(lib().hg_fit_sample_indices(int(kind), int(seed) & 0xffffffff, F, p, int(n_points), int(n_hyp),
                                       out.ctypes.data_as(C.POINTER(C.c_int32)) if out.size else None))
    return out


def align_scale_matrix(kind, m, level_in, level_out):
    """A transform between two planes, both at pyramid level level_in, converted to level_out (hg_align_scale_matrix): 8 doubles in the fit's
    layouts.  A position at level k is x_k = (x_0 + 0.5) 2^-k - 0.5."""
    a = np.ascontiguousarray(m, dtype=np.float64).ravel()
    assert a.size == 8, "a matrix is 8 doubles"
    out = np.empty(8, np.float64)
    _check(lib().hg_align_scale_matrix(int(kind), a.ctypes.data_as(C.POINTER(C.c_double)), int(level_in), int(level_out),
                                       out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def bundle_layout(kind, n_frames, n_pairs, n_points):
    """Scratch bytes of hg_bundle_adjust_frames_device for a shape (0 for no frames)."""
    total = C.c_size_t(0)
    _check(lib().hg_bundle_layout(int(kind), int(n_frames), int(n_pairs), int(n_points), C.byref(total)))
    return total.value


def bundle_info_bytes(n_frames, n_pairs):
    """Bytes of d_info of hg_bundle_adjust_frames_device: the call's record, one int32 per frame padded to 8 bytes, one record per pair."""
    return 48 + ((4 * int(n_frames) + 7) & ~7) + 24 * int(n_pairs)


def bundle_split_info(raw, n_frames, n_pairs):
    """(call record as BUNDLE_INFO, frame status int32 array, pair records as BUNDLE_PAIR_INFO) from the bytes of d_info."""
    raw = np.ascontiguousarray(raw, np.uint8)
    o = 48 + ((4 * int(n_frames) + 7) & ~7)
    return (raw[:48].view(BUNDLE_INFO)[0].copy(), raw[48:48 + 4 * int(n_frames)].view(np.int32).copy(),
            raw[o:o + 24 * int(n_pairs)].view(BUNDLE_PAIR_INFO).copy())


def bundle_chain_from_pairs(kind, n_frames, pairs, pair_mats, anchor=0):
    """Frame -> canvas matrices chained from pairwise ones (hg_bundle_chain_from_pairs; host only): pair_mats[p] maps frame pairs[p][0] to
    frame pairs[p][1]; the anchor is the identity, frames are reached breadth-first, unreached frames come back as NaNs.  (n_frames, 8)."""
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    pm = np.ascontiguousarray(pair_mats, dtype=np.float64).reshape(-1, 8)
    assert pm.shape[0] == pr.shape[0], "one matrix per pair"
    out = np.empty((int(n_frames), 8), np.float64)
    _check(lib().hg_bundle_chain_from_pairs(int(kind), int(n_frames), pr.ctypes.data_as(C.POINTER(C.c_int32)) if pr.size else None, pr.shape[0],
                                            pm.ctypes.data_as(C.POINTER(C.c_double)) if pm.size else None, int(anchor),
                                            out.ctypes.data_as(C.POINTER(C.c_double)) if out.size else None))
    return out


def bundle_invert_matrix(kind, m):
    """The inverse of a matrix in the fit's layouts (hg_bundle_invert_matrix; host only): the adjugate divided through by its last entry."""
    a = np.ascontiguousarray(m, dtype=np.float64).ravel()
    assert a.size == 8, "a matrix is 8 doubles"
    out = np.empty(8, np.float64)
    _check(lib().hg_bundle_invert_matrix(int(kind), a.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def align_refine_coarse_to_fine(ctx, kind, d_from, wf, hf, n_frames, d_to, wt, ht, n_to_sets, channels, mats, levels, rect=None, step=2,
                                photometric=True, n_iter=10, eps=0.01, min_valid=None, from_stride_bytes=None, to_stride_bytes=None):
    """Context.align_refine_frames_device from pyramid level levels - 1 down to level 0: both pyramids are built on the device
    (pyramid_build_device), every level is refined from the result of the coarser one, and only the matrices travel -- they are converted
    between levels on the host (align_scale_matrix).  mats: (n_frames, 8) doubles at level 0; rect: (rx, ry, rw, rh) at level 0 (None: the
    whole FROM plane), shrunk to the pixels of each level whose centres lie inside it; the same step, n_iter, eps and min_valid (None: P)
    at every level.  A frame a level fails keeps that level's input (the call's rule), so the walk goes on from there.
    Returns (mats (n_frames, 8), info of level 0 as ALIGN_INFO records)."""
    F, levels = int(n_frames), int(levels)
    mats = np.ascontiguousarray(mats, dtype=np.float64).reshape(F, 8).copy()
    assert 1 <= levels <= min(pyramid_levels(wf, hf), pyramid_levels(wt, ht)), "levels must exist on both sides"
    P = (8 if int(kind) == HG_PROJECTIVE else 6) + (2 if photometric else 0)
    min_valid = P if min_valid is None else int(min_valid)
    rect = (0, 0, int(wf), int(hf)) if rect is None else tuple(int(v) for v in rect)
    fs = int(wf) * int(hf) * int(channels) if from_stride_bytes is None else int(from_stride_bytes)
    ts = int(wt) * int(ht) * int(channels) if to_stride_bytes is None else int(to_stride_bytes)
    fo, f_total = pyramid_layout(wf, hf, ELEM_U8, channels, levels)
    to, t_total = pyramid_layout(wt, ht, ELEM_U8, channels, levels)
    d_fp = ctx.alloc(max(f_total * F, 256))
    d_tp = ctx.alloc(max(t_total * int(n_to_sets), 256))
    d_m = ctx.alloc(F * (64 + 48))
    d_i = d_m + F * 64
    try:
        if levels > 1:
            ctx.pyramid_build_device(d_from, wf, hf, F, fs, ELEM_U8, channels, levels, d_fp, f_total)
            ctx.pyramid_build_device(d_to, wt, ht, int(n_to_sets), ts, ELEM_U8, channels, levels, d_tp, t_total)
        info = np.zeros(F, ALIGN_INFO)
        fsz, tsz = [(int(wf), int(hf))], [(int(wt), int(ht))]
        for _ in range(1, levels):                                            # (a level halves the one below, rounding up)
            fsz.append(((fsz[-1][0] + 1) >> 1, (fsz[-1][1] + 1) >> 1))
            tsz.append(((tsz[-1][0] + 1) >> 1, (tsz[-1][1] + 1) >> 1))
        for k in range(levels - 1, -1, -1):
            cur = np.stack([align_scale_matrix(kind, m, 0, k) if np.isfinite(m).all() else m for m in mats]) if F else mats
            (lw, lh), (tw, th) = fsz[k], tsz[k]
            # the level-k pixels whose centres, x_0 = (x_k + 0.5) 2^k - 0.5, lie inside the rectangle
            lo = lambda a: -((-(2 * a + 1 - (1 << k))) // (2 << k))
            hi = lambda b: (2 * b - 1 - (1 << k)) // (2 << k)
            x0, y0 = max(lo(rect[0]), 0), max(lo(rect[1]), 0)
            x1, y1 = min(hi(rect[0] + rect[2]), lw - 1), min(hi(rect[1] + rect[3]), lh - 1)
            ctx.to_device(d_m, cur)
            ctx.align_refine_frames_device(kind, d_from if k == 0 else d_fp + fo[k], lw, lh, F, d_to if k == 0 else d_tp + to[k], tw, th, n_to_sets, channels,
                                           (x0, y0, x1 - x0 + 1, y1 - y0 + 1), d_m, d_m, d_i, step=step, photometric=photometric, n_iter=n_iter, eps=eps,
                                           min_valid=min_valid, from_stride_bytes=fs if k == 0 else f_total, to_stride_bytes=ts if k == 0 else t_total)
            ctx.sync()
            got = ctx.to_host(d_m, F * 64).view(np.float64).reshape(F, 8)
            info = ctx.to_host(d_i, F * 48).view(ALIGN_INFO).copy()
            mats = np.stack([align_scale_matrix(kind, m, k, 0) if np.isfinite(m).all() else m for m in got]) if F else got
        return mats, info
    finally:
        for p in (d_fp, d_tp, d_m):
            ctx.free(p)


def detect_layout(W, H, cell, per_cell):
    """(cells_x, cells_y, n_slots) of a W x H plane under cell x cell cells that keep per_cell keypoints each (hg_detect_layout): n_slots is the
    capacity of a plane's keypoint list."""
    cx, cy, ns = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib().hg_detect_layout(int(W), int(H), int(cell), int(per_cell), C.byref(cx), C.byref(cy), C.byref(ns)))
    return cx.value, cy.value, ns.value


def describe_pattern():
    """The sampling pattern of the descriptor (hg_describe_pattern): an int8 array of shape (32, 256, 4), {ax, ay, bx, by} of test b under bin k."""
    out = np.empty((DETECT_BINS, 256, 4), np.int8)
    _check(lib().hg_describe_pattern(out.ctypes.data_as(C.POINTER(C.c_int8))))
    return out


def _field_array(fmt, h, w):
    return np.empty((max(h, 0), max(w, 0)), np.int32) if int(fmt) == FIELD_INDEX else np.empty((max(h, 0), max(w, 0), 2), np.float32)


def device_count():
    n = C.c_int(0)
    code = lib().hg_device_count(C.byref(n))
    return n.value if code == 0 else 0


# ------------------------------------------------------------------ context

def _remap_bicubic_frames(handle, geoms, d_coords, d_planes, w, h, n_planes, plane_stride_bytes, elem, channels, d_out, b, c, field_offsets, out_offsets):
    """hg_remap_bicubic_frames_device for Context.remap_bicubic_frames_device, whose parameter C would hide the ctypes alias."""
    fo = (C.c_size_t * len(geoms))(*field_offsets) if field_offsets is not None else None
    oo = (C.c_size_t * len(geoms))(*out_offsets) if out_offsets is not None else None
    return lib().hg_remap_bicubic_frames_device(handle, _geoms(geoms), len(geoms), C.c_void_p(int(d_coords)), fo, C.c_void_p(int(d_planes)),
                                                int(w), int(h), int(n_planes), int(plane_stride_bytes), int(elem), int(channels),
                                                C.c_void_p(int(d_out)), oo, float(b), float(c))


class Context:
    """One hg_ctx (one GPU, one stream) == the device side of one Homography instance."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        self._n_pts = self._n_tris = 0
        L = lib()
        if stream is None:
            code = L.hg_create(int(device), C.byref(self._h))
        else:
            code = L.hg_create_on_stream(int(device), C.c_void_p(int(stream)), C.byref(self._h))
        if code != 0:
            self._h = C.c_void_p()
            _check(code)

    def close(self):
        if self._h:
            lib().hg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _c(self, code):
        _check(code, self._h)

    # ---- plumbing
    def sync(self):
        self._c(lib().hg_sync(self._h))

    def alloc(self, nbytes):
        p = C.c_void_p()
        self._c(lib().hg_device_alloc(self._h, int(nbytes), C.byref(p)))
        return p.value

    def free(self, dptr):
        self._c(lib().hg_device_free(self._h, C.c_void_p(dptr)))

    def to_host(self, dptr, nbytes, offset=0):
        out = np.empty(int(nbytes), np.uint8)
        self._c(lib().hg_copy_to_host(self._h, out.ctypes.data_as(C.c_void_p), C.c_void_p(dptr + offset), int(nbytes)))
        return out

    def download_behind_warps(self, out, dptr, offset=0):
        """D2H into the uint8 array `out` on the context's download stream, ordered behind the warps issued so far (hg_download_behind_warps);
        `out` must stay alive until fence_downloads()."""
        self._c(lib().hg_download_behind_warps(self._h, out.ctypes.data_as(C.c_void_p), C.c_void_p(dptr + offset), int(out.nbytes)))

    def fence_downloads(self):
        self._c(lib().hg_fence_downloads(self._h))

    def to_device(self, dptr, arr, offset=0):
        a = np.ascontiguousarray(arr)
        self._c(lib().hg_copy_to_device(self._h, C.c_void_p(dptr + offset), a.ctypes.data_as(C.c_void_p), a.nbytes))

    def set_timing(self, on=True):
        self._c(lib().hg_set_timing(self._h, 1 if on else 0))

    def last_kernel_ms(self):
        ms = C.c_float(0)
        self._c(lib().hg_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def last_forward_kernel(self):
        """1 = scatter + gather, 2 = k_fwd_tiles (see include/hgwarp.h)"""
        return lib().hg_last_forward_kernel(self._h)

    def last_piecewise_kernel(self):
        """0 none, 1 k_pw_rows (4-row groups), 2 k_pw_rows (1 row), 3 k_pw_patch, 4 k_pw_fused, 5 k_pw_tile."""
        return lib().hg_last_piecewise_kernel(self._h)

    def last_piecewise_variant(self):
        """Variant code of the instantiation that ran (include/hgwarp.h); 0 with an older library."""
        L = lib()
        return L.hg_last_piecewise_variant(self._h) if hasattr(L, "hg_last_piecewise_variant") else 0

    def last_geometric_kernel(self):
        """-1 none, 100 * KIND + 10 * NW + S for k_geo_fast<KIND, NW, S>, 1000 + 10 * kind + S for k_geo<kind, S> (include/hgwarp.h)."""
        return lib().hg_last_geometric_kernel(self._h)

    def last_piecewise_self(self):
        """1 if the row workgroups of the last fused run evaluated their own spans (no row lists), 0 if they read k_tri_spans' lists."""
        return lib().hg_last_piecewise_self(self._h)

    def last_piecewise_flag(self):
        """Status word of the last frame a fused run flagged (diagnostics; include/hgwarp.h)."""
        return lib().hg_last_piecewise_flag(self._h)

    def redone_frames(self):
        """Frames redone through the materialised map since the context was created."""
        return lib().hg_redone_frames(self._h)

    def layout_walks(self):
        """Host walks over the triangles of a frame set (layout estimates) since the context was created."""
        return lib().hg_layout_walks(self._h)

    def span_cache_stats(self):
        """The span cache of the row warp kernel: builds, warps that ran from it, groups valid / not cached and bytes held of the current
        build, and the state of the last inverse piecewise warp ("off", "build", "use")."""
        out = (C.c_int64 * 6)()
        self._c(lib().hg_span_cache_stats(self._h, out))
        return {"builds": out[0], "use_calls": out[1], "groups_valid": out[2], "groups_not_cached": out[3], "bytes": out[4],
                "state": ("off", "build", "use")[out[5]]}

    def xcc_count(self):
        """XCCs the warp kernels' block id -> row band mapping assumes (read from the device at creation, or option 'xcc')."""
        return lib().hg_xcc_count(self._h)

    def set_option(self, key, value):
        """Layout knobs of the piecewise fast path ("min_row_groups", "patch"); results never depend on them."""
        self._c(lib().hg_set_option(self._h, key.encode(), int(value)))

    def set_sampling(self, mode):
        """SAMPLE_NEAREST (default, the reference's pixel copy) or SAMPLE_BILINEAR for the inverse warps called from now on."""
        self._c(lib().hg_set_sampling(self._h, int(mode)))

    @property
    def sampling(self):
        m = C.c_int(-1)
        self._c(lib().hg_get_sampling(self._h, C.byref(m)))
        return m.value

    def selftest_division(self, samples, seed=1):
        """Mismatches between the shared-reciprocal division of the projective kernel and IEEE division (must be 0)."""
        bad = C.c_uint64(0)
        self._c(lib().hg_selftest_division(self._h, int(samples), int(seed), C.byref(bad)))
        return bad.value

    def kernel_ms_stats(self):
        """(total ms, launches) of the dominant kernel since set_timing(True)."""
        tot, n = C.c_double(0), C.c_int(0)
        self._c(lib().hg_kernel_ms_stats(self._h, C.byref(tot), C.byref(n)))
        return tot.value, n.value

    # ---- image
    def set_image(self, rgba):
        a = np.ascontiguousarray(rgba, dtype=np.uint8)
        h, w = a.shape[:2]
        self._c(lib().hg_set_image(self._h, a.ctypes.data_as(C.POINTER(C.c_uint8)), w, h))

    def set_image_device(self, dptr, w, h):
        self._c(lib().hg_set_image_device(self._h, C.c_void_p(int(dptr)), int(w), int(h)))

    def set_images_device(self, dptr, w, h, n_images, stride_bytes):
        self._c(lib().hg_set_images_device(self._h, C.c_void_p(int(dptr)), int(w), int(h), int(n_images), int(stride_bytes)))

    # ---- affine / projective
    def warp_inverse_geometric(self, kind, m, geom):
        _, p = _f64(m)
        g = Geom(*[int(v) for v in geom])
        out = np.zeros((max(g.obj_h, 0), max(g.obj_w, 0), 4), np.uint8)
        self._c(lib().hg_warp_inverse_geometric(self._h, int(kind), p, g, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def warp_inverse_geometric_device(self, kind, m, geom, d_out):
        """One affine / projective frame into device memory (asynchronous; sync() settles it)."""
        a, p = _f64(m)
        assert a.size >= (6 if int(kind) == 0 else 8)
        self._c(lib().hg_warp_inverse_geometric_device(self._h, int(kind), p, Geom(*[int(v) for v in geom]), C.c_void_p(int(d_out))))

    def warp_forward_geometric(self, kind, m, geom):
        _, p = _f64(m)
        g = Geom(*[int(v) for v in geom])
        out = np.zeros((max(g.obj_h, 0), max(g.obj_w, 0), 4), np.uint8)
        self._c(lib().hg_warp_forward_geometric(self._h, int(kind), p, g, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def warp_forward_piecewise(self, dst_pts, max_src_x, max_src_y, geom):
        d, dp = _f32(dst_pts)
        assert d.size == 2 * self._n_pts, "one x,y pair per mesh point"
        g = Geom(*[int(v) for v in geom])
        out = np.zeros((max(g.obj_h, 0), max(g.obj_w, 0), 4), np.uint8)
        self._c(lib().hg_warp_forward_piecewise(self._h, dp, int(max_src_x), int(max_src_y), g, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    # reference-state forms: the cached matrices as they stood + the definition of the map the shared field held
    def warp_inverse_piecewise_state(self, fwd_mats, dst_pts, tris, min_src_x, min_src_y, geom):
        m, mp = _f32(fwd_mats)
        g = Geom(*[int(v) for v in geom])
        d, keep = _map_def(dst_pts, tris, g.obj_w, g.obj_h, g.y_off)
        out = np.zeros((max(g.obj_h, 0), max(g.obj_w, 0), 4), np.uint8)
        self._c(lib().hg_warp_inverse_piecewise_state(self._h, mp, m.size // 6, C.byref(d), int(min_src_x), int(min_src_y), g, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def warp_forward_piecewise_state(self, fwd_mats, map_pts, map_tris, map_w, map_h, map_y_off, min_src_x, min_src_y, max_src_x, max_src_y, geom):
        m, mp = _f32(fwd_mats)
        g = Geom(*[int(v) for v in geom])
        d, keep = _map_def(map_pts, map_tris, map_w, map_h, map_y_off)
        out = np.zeros((max(g.obj_h, 0), max(g.obj_w, 0), 4), np.uint8)
        self._c(lib().hg_warp_forward_piecewise_state(self._h, mp, m.size // 6, C.byref(d), int(min_src_x), int(min_src_y), int(max_src_x), int(max_src_y), g,
                                                      out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def warp_forward_geometric_batch_device(self, kind, mats, geoms, offsets, d_out):
        m, p = _f64(mats)
        assert m.size == 8 * len(geoms)
        offs = (C.c_size_t * len(geoms))(*offsets) if offsets is not None else None
        self._c(lib().hg_warp_forward_geometric_batch_device(self._h, int(kind), p, _geoms(geoms), offs, len(geoms), C.c_void_p(int(d_out))))

    def warp_forward_piecewise_batch_device(self, dst_pts, max_src_x, max_src_y, geoms, offsets, d_out):
        d, dp = _f32(dst_pts)
        assert d.size == 2 * self._n_pts * len(geoms), "frames x mesh points x,y pairs"
        offs = (C.c_size_t * len(geoms))(*offsets) if offsets is not None else None
        self._c(lib().hg_warp_forward_piecewise_batch_device(self._h, dp, int(max_src_x), int(max_src_y), _geoms(geoms), offs, len(geoms), C.c_void_p(int(d_out))))

    def geometric_set_frames(self, kind, mats, geoms, offsets=None):
        m, p = _f64(mats)
        assert m.size == 8 * len(geoms)
        offs = (C.c_size_t * len(geoms))(*offsets) if offsets is not None else None
        self._c(lib().hg_geometric_set_frames(self._h, int(kind), p, _geoms(geoms), offs, len(geoms)))

    def geometric_set_frames_points(self, kind, from_pts, to_pts, geoms, offsets=None):
        """Frames as point sets: the matrices (from -> to) are solved on the device at every warp, like the reference's :994."""
        per = 6 if int(kind) == 0 else 8
        (a, ap), (b, bp) = _f32(from_pts), _f32(to_pts)
        assert a.size == per * len(geoms) and b.size == per * len(geoms)
        offs = (C.c_size_t * len(geoms))(*offsets) if offsets is not None else None
        self._c(lib().hg_geometric_set_frames_points(self._h, int(kind), ap, bp, _geoms(geoms), offs, len(geoms)))

    def geometric_points_args(self, kind, from_pts, to_pts, geoms, offsets=None):
        """The ctypes arguments of geometric_set_frames_points, built once (bench.py --points fresh)."""
        per = 6 if int(kind) == 0 else 8
        (a, ap), (b, bp) = _f32(from_pts), _f32(to_pts)
        assert a.size == per * len(geoms) and b.size == per * len(geoms)
        offs = (C.c_size_t * len(geoms))(*offsets) if offsets is not None else None
        return (a, b, int(kind), ap, bp, _geoms(geoms), offs, len(geoms))

    def geometric_set_frames_points_prepared(self, args):
        self._c(lib().hg_geometric_set_frames_points(self._h, args[2], args[3], args[4], args[5], args[6], args[7]))

    def get_geometric_matrices(self, n_frames):
        out = np.empty((int(n_frames), 8), np.float64)
        self._c(lib().hg_get_geometric_matrices(self._h, out.ctypes.data_as(C.POINTER(C.c_double)), int(n_frames)))
        return out

    def warp_inverse_geometric_frames_device(self, d_out):
        self._c(lib().hg_warp_inverse_geometric_frames_device(self._h, C.c_void_p(int(d_out))))

    # ---- source fields and remaps (include/hgwarp.h, HG_FIELD_*)
    def field_inverse_geometric(self, kind, m, geom, fmt):
        """The source field of warp_inverse_geometric(kind, m, geom): (h, w) int32 (FIELD_INDEX) or (h, w, 2) float32 (FIELD_COORDS)."""
        a, p = _f64(m)
        assert a.size >= (6 if int(kind) == 0 else 8)
        g = Geom(*[int(v) for v in geom])
        out = _field_array(fmt, g.obj_h, g.obj_w)
        self._c(lib().hg_field_inverse_geometric(self._h, int(kind), p, g, int(fmt), out.ctypes.data_as(C.c_void_p)))
        return out

    def field_inverse_geometric_device(self, kind, m, geom, fmt, d_field):
        a, p = _f64(m)
        assert a.size >= (6 if int(kind) == 0 else 8)
        self._c(lib().hg_field_inverse_geometric_device(self._h, int(kind), p, Geom(*[int(v) for v in geom]), int(fmt), C.c_void_p(int(d_field))))

    def field_inverse_geometric_frames_device(self, fmt, d_field, offsets=None):
        """The fields of the staged geometric frame set; offsets=None: packed as pack_field_offsets does."""
        offs = (C.c_size_t * len(offsets))(*offsets) if offsets is not None else None
        self._c(lib().hg_field_inverse_geometric_frames_device(self._h, int(fmt), offs, C.c_void_p(int(d_field))))

    def field_inverse_piecewise(self, fmt):
        """The source field of the prepared piecewise frame: (h, w) int32 or (h, w, 2) float32."""
        g = self._geom
        out = _field_array(fmt, g.obj_h, g.obj_w)
        self._c(lib().hg_field_inverse_piecewise(self._h, int(fmt), out.ctypes.data_as(C.c_void_p)))
        return out

    def field_inverse_piecewise_frames_device(self, fmt, d_field, offsets=None):
        """The fields of the staged piecewise frame set (settled inside the call); offsets=None: packed as pack_field_offsets does."""
        offs = (C.c_size_t * len(offsets))(*offsets) if offsets is not None else None
        self._c(lib().hg_field_inverse_piecewise_frames_device(self._h, int(fmt), offs, C.c_void_p(int(d_field))))

    # the source field of the FORWARD warps: (h, w) int32, the flat source index the last writer of each output pixel reads, -1 where none
    def field_forward_geometric(self, kind, m, geom):
        a, p = _f64(m)
        assert a.size >= (6 if int(kind) == 0 else 8)
        g = Geom(*[int(v) for v in geom])
        out = _field_array(FIELD_INDEX, g.obj_h, g.obj_w)
        self._c(lib().hg_field_forward_geometric(self._h, int(kind), p, g, out.ctypes.data_as(C.c_void_p)))
        return out

    def field_forward_geometric_batch_device(self, kind, mats, geoms, offsets, d_field):
        """offsets=None: packed as pack_field_offsets(geoms, FIELD_INDEX) does (asynchronous)."""
        m, p = _f64(mats)
        assert m.size == 8 * len(geoms)
        offs = (C.c_size_t * len(geoms))(*offsets) if offsets is not None else None
        self._c(lib().hg_field_forward_geometric_batch_device(self._h, int(kind), p, _geoms(geoms), offs, len(geoms), C.c_void_p(int(d_field))))

    def field_forward_piecewise(self, dst_pts, max_src_x, max_src_y, geom):
        d, dp = _f32(dst_pts)
        assert d.size == 2 * self._n_pts, "one x,y pair per mesh point"
        g = Geom(*[int(v) for v in geom])
        out = _field_array(FIELD_INDEX, g.obj_h, g.obj_w)
        self._c(lib().hg_field_forward_piecewise(self._h, dp, int(max_src_x), int(max_src_y), g, out.ctypes.data_as(C.c_void_p)))
        return out

    def field_forward_piecewise_batch_device(self, dst_pts, max_src_x, max_src_y, geoms, offsets, d_field):
        """No deferred redo: queued runs are settled first, frames the tile kernels flag are redone before it returns; on the scatter path the
        launches are asynchronous on the stream.  offsets=None: packed."""
        d, dp = _f32(dst_pts)
        assert d.size == 2 * self._n_pts * len(geoms), "frames x mesh points x,y pairs"
        offs = (C.c_size_t * len(geoms))(*offsets) if offsets is not None else None
        self._c(lib().hg_field_forward_piecewise_batch_device(self._h, dp, int(max_src_x), int(max_src_y), _geoms(geoms), offs, len(geoms), C.c_void_p(int(d_field))))

    def last_forward_field_kernel(self):
        """0 = no forward field yet, 1 = scatter + winner buffer, 2 = the tile-binned kernels (include/hgwarp.h)."""
        return lib().hg_last_forward_field_kernel(self._h)

    # ---- point lists (include/hgwarp.h, hg_points_*): n_sets lists of n_points interleaved x,y float32 in GPU memory, frame f reads list
    # f % n_sets; d_out receives frames x n_points x 2 float32, both words 0x7fc00000 where a point is unmapped
    def points_to_source_geometric_frames_device(self, d_points, n_points, n_sets, d_out):
        """Output-window positions -> source coordinates through the staged geometric frame set (asynchronous)."""
        self._c(lib().hg_points_to_source_geometric_frames_device(self._h, C.c_void_p(d_points), int(n_points), int(n_sets), C.c_void_p(d_out)))

    def points_to_source_piecewise_frames_device(self, d_points, n_points, n_sets, d_out):
        """Output-window positions -> source coordinates through the staged piecewise frame set (settled inside the call)."""
        self._c(lib().hg_points_to_source_piecewise_frames_device(self._h, C.c_void_p(d_points), int(n_points), int(n_sets), C.c_void_p(d_out)))

    def points_to_output_geometric_batch_device(self, kind, mats, geoms, d_points, n_points, n_sets, d_out):
        """Source positions -> window-relative output positions under len(geoms) x 8 FORWARD matrices (asynchronous)."""
        m, p = _f64(mats)
        assert m.size == 8 * len(geoms)
        self._c(lib().hg_points_to_output_geometric_batch_device(self._h, int(kind), p, _geoms(geoms), len(geoms), C.c_void_p(d_points),
                                                                 int(n_points), int(n_sets), C.c_void_p(d_out)))

    def points_to_output_piecewise_batch_device(self, dst_pts, max_src_x, max_src_y, geoms, d_points, n_points, n_sets, d_out):
        """Source positions -> window-relative output positions through the forward map and the frames' forward matrices (asynchronous)."""
        d, dp = _f32(dst_pts)
        assert d.size == 2 * self._n_pts * len(geoms), "frames x mesh points x,y pairs"
        self._c(lib().hg_points_to_output_piecewise_batch_device(self._h, dp, int(max_src_x), int(max_src_y), _geoms(geoms), len(geoms),
                                                                 C.c_void_p(d_points), int(n_points), int(n_sets), C.c_void_p(d_out)))

    def remap_index_device(self, d_field, n_px, d_src, n_src_px, pixel_bytes, d_out):
        """out[i] = src[field[i]] where 0 <= field[i] < n_src_px, else zeros; pixels of 1, 2, 4, 8 or 16 bytes (asynchronous)."""
        self._c(lib().hg_remap_index_device(self._h, C.c_void_p(int(d_field)), int(n_px), C.c_void_p(int(d_src)), int(n_src_px), int(pixel_bytes),
                                            C.c_void_p(int(d_out))))

    def remap_bilinear_f32_device(self, d_coords, n_px, d_src, w, h, channels, d_out):
        """Bilinear gather of 1..4 interleaved float32 channels of a w x h source through a FIELD_COORDS field (asynchronous)."""
        self._c(lib().hg_remap_bilinear_f32_device(self._h, C.c_void_p(int(d_coords)), int(n_px), C.c_void_p(int(d_src)), int(w), int(h), int(channels),
                                                   C.c_void_p(int(d_out))))

    def remap_bilinear_u8_device(self, d_coords, n_px, d_src, w, h, channels, d_out):
        """The same gather for 1..4 interleaved uint8 channels: the f32 blend, then min(255, floor(v + 0.5)) (asynchronous)."""
        self._c(lib().hg_remap_bilinear_u8_device(self._h, C.c_void_p(int(d_coords)), int(n_px), C.c_void_p(int(d_src)), int(w), int(h), int(channels),
                                                  C.c_void_p(int(d_out))))

    def remap_index_frames_device(self, geoms, d_field, d_planes, n_src_px, n_planes, plane_stride_bytes, pixel_bytes, d_out,
                                  field_offsets=None, out_offsets=None):
        """remap_index_device for a whole frame set in one launch: frame f is the flat list of obj_w * obj_h pixels of geoms[f] and reads plane
        f % n_planes.  field_offsets=None: packed as pack_field_offsets does; out_offsets=None: as pack_plane_offsets(geoms, pixel_bytes) does."""
        fo = (C.c_size_t * len(geoms))(*field_offsets) if field_offsets is not None else None
        oo = (C.c_size_t * len(geoms))(*out_offsets) if out_offsets is not None else None
        self._c(lib().hg_remap_index_frames_device(self._h, _geoms(geoms), len(geoms), C.c_void_p(int(d_field)), fo, C.c_void_p(int(d_planes)),
                                                   int(n_src_px), int(n_planes), int(plane_stride_bytes), int(pixel_bytes), C.c_void_p(int(d_out)), oo))

    def remap_bilinear_frames_device(self, geoms, d_coords, d_planes, w, h, n_planes, plane_stride_bytes, elem, channels, d_out,
                                     field_offsets=None, out_offsets=None):
        """remap_bilinear_f32_device (elem ELEM_F32) or remap_bilinear_u8_device (ELEM_U8) for a whole frame set in one launch;
        out_offsets=None: packed as pack_plane_offsets(geoms, channels * element size) does."""
        fo = (C.c_size_t * len(geoms))(*field_offsets) if field_offsets is not None else None
        oo = (C.c_size_t * len(geoms))(*out_offsets) if out_offsets is not None else None
        self._c(lib().hg_remap_bilinear_frames_device(self._h, _geoms(geoms), len(geoms), C.c_void_p(int(d_coords)), fo, C.c_void_p(int(d_planes)),
                                                      int(w), int(h), int(n_planes), int(plane_stride_bytes), int(elem), int(channels),
                                                      C.c_void_p(int(d_out)), oo))

    def remap_bicubic_frames_device(self, geoms, d_coords, d_planes, w, h, n_planes, plane_stride_bytes, elem, channels, d_out,
                                    B=0.0, C=0.5, field_offsets=None, out_offsets=None):
        """remap_bilinear_frames_device with the 4 x 4 taps of the (B, C) cubic, for enlargements: CUBIC_CATMULL_ROM (the default),
        CUBIC_MITCHELL, CUBIC_BSPLINE or any pair in [0, 1]; reads level 0 only, uint8 results clamped to 0..255 on both sides."""
        # (the parameter C is the header's name and hides the ctypes alias in here: the call itself is made outside)
        self._c(_remap_bicubic_frames(self._h, geoms, d_coords, d_planes, w, h, n_planes, plane_stride_bytes, elem, channels, d_out, B, C,
                                      field_offsets, out_offsets))

    def pyramid_build_device(self, d_planes, w, h, n_planes, plane_stride_bytes, elem, channels, levels, d_pyr, pyr_stride_bytes):
        """Levels 1 .. levels-1 of the mip pyramid of every plane, pyramid p at d_pyr + p * pyr_stride_bytes in pyramid_layout's layout;
        asynchronous, one launch per level."""
        self._c(lib().hg_pyramid_build_device(self._h, C.c_void_p(int(d_planes)), int(w), int(h), int(n_planes), int(plane_stride_bytes), int(elem),
                                              int(channels), int(levels), C.c_void_p(int(d_pyr)), int(pyr_stride_bytes)))

    def remap_trilinear_frames_device(self, geoms, d_coords, d_planes, w, h, n_planes, plane_stride_bytes, elem, channels, d_out,
                                      d_pyr, pyr_stride_bytes, levels, field_offsets=None, out_offsets=None):
        """remap_bilinear_frames_device with minification filtering: every pixel reads the pyramid level(s) its footprint in the field asks
        for (frames are read as obj_w x obj_h arrays); levels == 1 is the bilinear frames remap, bit for bit."""
        fo = (C.c_size_t * len(geoms))(*field_offsets) if field_offsets is not None else None
        oo = (C.c_size_t * len(geoms))(*out_offsets) if out_offsets is not None else None
        self._c(lib().hg_remap_trilinear_frames_device(self._h, _geoms(geoms), len(geoms), C.c_void_p(int(d_coords)), fo, C.c_void_p(int(d_planes)),
                                                       int(w), int(h), int(n_planes), int(plane_stride_bytes), int(elem), int(channels),
                                                       C.c_void_p(int(d_out)), oo, C.c_void_p(int(d_pyr)), int(pyr_stride_bytes), int(levels)))

    def remap_aniso_frames_device(self, geoms, d_coords, d_planes, w, h, n_planes, plane_stride_bytes, elem, channels, d_out,
                                  d_pyr, pyr_stride_bytes, levels, max_aniso, field_offsets=None, out_offsets=None):
        """remap_trilinear_frames_device with anisotropic filtering: up to max_aniso (1..16) probes along the longer of a pixel's two steps
        in the field, each from the finer level(s) the shorter step allows, averaged; max_aniso == 1 is the trilinear remap, bit for bit."""
        fo = (C.c_size_t * len(geoms))(*field_offsets) if field_offsets is not None else None
        oo = (C.c_size_t * len(geoms))(*out_offsets) if out_offsets is not None else None
        self._c(lib().hg_remap_aniso_frames_device(self._h, _geoms(geoms), len(geoms), C.c_void_p(int(d_coords)), fo, C.c_void_p(int(d_planes)),
                                                   int(w), int(h), int(n_planes), int(plane_stride_bytes), int(elem), int(channels),
                                                   C.c_void_p(int(d_out)), oo, C.c_void_p(int(d_pyr)), int(pyr_stride_bytes), int(levels), int(max_aniso)))

    def mosaic_frames_device(self, geoms, d_coords, d_frames, elem, channels, w, h, mode, feather, canvas, d_canvas, d_weight=0,
                             field_offsets=None, frame_offsets=None, gains=None):
        """The frames of a set blended into ONE canvas (asynchronous): frame f's pixels (obj_w x obj_h, `channels` elements of `elem`) lie at
        (x_off, y_off) of destination space and count where its FIELD_COORDS field is finite.  mode MOSAIC_LAST paints in frame order,
        MOSAIC_MEAN averages, MOSAIC_FEATHER weights by the distance to the w x h source's border, capped at `feather`.  canvas = (x, y, width,
        height): d_canvas gets every pixel of it tightly packed, d_weight (0: none) one float32 per pixel.  field_offsets=None: packed as
        pack_field_offsets does; frame_offsets=None: as pack_plane_offsets(geoms, channels * element size) does.  gains (None: none): one
        factor per frame, finite and > 0, applied to every contributor's colour channels -- not to the alpha of a 4-channel frame -- before the
        blend (mosaic_solve_gains)."""
        fo = (C.c_size_t * len(geoms))(*field_offsets) if field_offsets is not None else None
        po = (C.c_size_t * len(geoms))(*frame_offsets) if frame_offsets is not None else None
        if gains is not None:
            gv = np.ascontiguousarray(gains, dtype=np.float32).ravel()
            assert gv.size == len(geoms), "one gain per frame"
            self._c(lib().hg_mosaic_frames_gain_device(self._h, _geoms(geoms) if len(geoms) else None, len(geoms), C.c_void_p(int(d_coords) or None), fo,
                                                       C.c_void_p(int(d_frames) or None), po, int(elem), int(channels), int(w), int(h), int(mode), float(feather),
                                                       Geom(*[int(v) for v in canvas]), C.c_void_p(int(d_canvas) or None), C.c_void_p(int(d_weight) or None),
                                                       gv.ctypes.data_as(C.POINTER(C.c_float)) if gv.size else None))
            return
        self._c(lib().hg_mosaic_frames_device(self._h, _geoms(geoms) if len(geoms) else None, len(geoms), C.c_void_p(int(d_coords) or None), fo,
                                              C.c_void_p(int(d_frames) or None), po, int(elem), int(channels), int(w), int(h), int(mode), float(feather),
                                              Geom(*[int(v) for v in canvas]), C.c_void_p(int(d_canvas) or None), C.c_void_p(int(d_weight) or None)))

    def mosaic_robust_device(self, geoms, d_coords, d_frames, channels, mode, canvas, d_canvas, d_weight=0, trim=0.0,
                             field_offsets=None, frame_offsets=None, gains=None):
        """The u8 frames of a set (at most 256) blended into ONE canvas by an order statistic per pixel and channel (asynchronous), so that
        what covers a pixel in a minority of the frames drops out: mode ROBUST_MEDIAN, ROBUST_TRIMMED (the mean of what is left when the
        share `trim`, in [0, 0.5), is cut off at both ends), ROBUST_MIN or ROBUST_MAX of the contributors' bytes.  geoms, d_coords, d_frames,
        canvas, d_canvas, d_weight (0: none; the number of contributors), the offsets and gains are mosaic_frames_device's; a gained value is a
        byte again before it is ranked."""
        fo = (C.c_size_t * len(geoms))(*field_offsets) if field_offsets is not None else None
        po = (C.c_size_t * len(geoms))(*frame_offsets) if frame_offsets is not None else None
        gp = None
        if gains is not None:
            gv = np.ascontiguousarray(gains, dtype=np.float32).ravel()
            assert gv.size == len(geoms), "one gain per frame"
            gp = gv.ctypes.data_as(C.POINTER(C.c_float)) if gv.size else None
        self._c(lib().hg_mosaic_robust_device(self._h, _geoms(geoms) if len(geoms) else None, len(geoms), C.c_void_p(int(d_coords) or None), fo,
                                              C.c_void_p(int(d_frames) or None), po, int(channels), int(mode), float(trim), gp,
                                              Geom(*[int(v) for v in canvas]), C.c_void_p(int(d_canvas) or None), C.c_void_p(int(d_weight) or None)))

    def mosaic_multiband_device(self, geoms, d_coords, d_frames, elem, channels, w, h, feather, n_bands, canvas, d_canvas, d_work, work_bytes,
                                d_weight=0, d_labels=0, field_offsets=None, frame_offsets=None, gains=None):
        """The frames of a set blended into ONE canvas in n_bands (1..8) frequency bands (asynchronous): every canvas pixel is owned by the
        contributor with the largest feather weight (capped at `feather`), low frequencies are blended across the seams between owners over
        a wide range and high frequencies over a narrow one.  The arguments are mosaic_frames_device's; d_work: 256-byte aligned scratch of
        work_bytes >= mosaic_multiband_layout(geoms, canvas, channels, n_bands); d_weight (0: none): 1.0 where a frame owns the pixel;
        d_labels (0: none): one int32 per canvas pixel, the owner's index or -1."""
        fo = (C.c_size_t * len(geoms))(*field_offsets) if field_offsets is not None else None
        po = (C.c_size_t * len(geoms))(*frame_offsets) if frame_offsets is not None else None
        gp = None
        if gains is not None:
            gv = np.ascontiguousarray(gains, dtype=np.float32).ravel()
            assert gv.size == len(geoms), "one gain per frame"
            gp = gv.ctypes.data_as(C.POINTER(C.c_float)) if gv.size else None
        vp = lambda v: C.c_void_p(int(v) or None)
        self._c(lib().hg_mosaic_multiband_device(self._h, _geoms(geoms) if len(geoms) else None, len(geoms), vp(d_coords), fo, vp(d_frames), po, int(elem),
                                                 int(channels), int(w), int(h), float(feather), int(n_bands), Geom(*[int(v) for v in canvas]), vp(d_canvas),
                                                 vp(d_weight), vp(d_labels), gp, vp(d_work), int(work_bytes)))

    def fit_matches_frames_device(self, kind, d_matches, n_points, counts, n_frames, threshold, n_hyp, seed, d_mats, d_counts, d_samples=0, refit=True,
                                  d_min_mats=0, d_best=0, d_mask=0):
        """hg_fit_matches_frames_device: one transform per frame from n_frames x n_points (x, y, u, v) float32 matches on the device (counts: per
        frame on the host, or None for all), by RANSAC over n_hyp hypotheses (drawn from `seed`, or read from d_samples) and, with refit, least
        squares over the best one's inliers.  Asynchronous; every output is device memory, 0 = not wanted."""
        _, p, _ = _counts(counts, n_frames)
        vp = lambda v: C.c_void_p(int(v) or None)
        self._c(lib().hg_fit_matches_frames_device(self._h, int(kind), vp(d_matches), int(n_points), p, int(n_frames), float(threshold), int(n_hyp),
                                                   int(seed) & 0xffffffff, vp(d_samples), 1 if refit else 0, vp(d_mats), vp(d_min_mats), vp(d_counts),
                                                   vp(d_best), vp(d_mask)))

    def align_refine_frames_device(self, kind, d_from, wf, hf, n_frames, d_to, wt, ht, n_to_sets, channels, rect, d_mats_in, d_mats_out, d_info,
                                   step=2, photometric=True, n_iter=10, eps=0.01, min_valid=None, d_sums=0, from_stride_bytes=None, to_stride_bytes=None):
        """hg_align_refine_frames_device: the transforms of n_frames frames (8 doubles each at d_mats_in, FROM -> TO, the fit's layouts) refined
        on the pixels -- Gauss-Newton on the intensity difference between the u8 FROM plane of every frame (wf x hf x channels) and TO plane
        f % n_to_sets (wt x ht), over the FROM pixels of rect = (rx, ry, rw, rh) taken every `step`; with photometric a gain and a bias are
        fitted too.  At most n_iter updates, stopping when the rectangle's corners move less than eps TO pixels; min_valid (None: P) valid
        samples are needed.  d_mats_out (may be d_mats_in) gets the matrices, d_info one ALIGN_INFO record per frame, d_sums (0: not wanted)
        ALIGN_SUMS doubles per frame: the sums of the first pass.  Asynchronous; a local refinement: start within a few pixels."""
        vp = lambda v: C.c_void_p(int(v) or None)
        P = (8 if int(kind) == HG_PROJECTIVE else 6) + (2 if photometric else 0)
        fs = int(wf) * int(hf) * int(channels) if from_stride_bytes is None else int(from_stride_bytes)
        ts = int(wt) * int(ht) * int(channels) if to_stride_bytes is None else int(to_stride_bytes)
        rx, ry, rw, rh = [int(v) for v in rect]
        self._c(lib().hg_align_refine_frames_device(self._h, int(kind), vp(d_from), int(wf), int(hf), int(n_frames), fs, vp(d_to), int(wt), int(ht),
                                                    int(n_to_sets), ts, int(channels), rx, ry, rw, rh, int(step), int(photometric), int(n_iter), float(eps),
                                                    P if min_valid is None else int(min_valid), vp(d_mats_in), vp(d_mats_out), vp(d_info), vp(d_sums)))

    def bundle_adjust_frames_device(self, kind, w, h, n_frames, fixed, pairs, d_matches, n_points, counts, d_mats_in, d_mats_out, d_info, d_scratch,
                                    scratch_bytes, d_mask=0, n_iter=10, eps=0.01, lambda0=1e-3, huber=0.0, d_pair_sums=0):
        """hg_bundle_adjust_frames_device: the frame -> canvas matrices of n_frames frames of w x h (8 doubles each at d_mats_in, the fit's
        layouts) adjusted over all pairs at once by Levenberg-Marquardt.  fixed: one flag per frame (host; at least one set); pairs: (n_pairs,
        2) frame indices (host); d_matches: n_pairs lists of n_points (x, y, u, v) float32, (x, y) in the pair's first frame; counts: slots
        used per pair (host; None: all); d_mask (0: none): the fit's inlier mask.  At most n_iter rounds, stopping when no frame corner moves
        eps canvas pixels; lambda0: the first damping; huber (pixels, 0: off).  d_mats_out may be d_mats_in; d_info gets
        bundle_info_bytes(n_frames, n_pairs) bytes (bundle_split_info), d_pair_sums (0: not wanted) BUNDLE_SUMS doubles per pair, the records
        of the first pass; d_scratch: bundle_layout's bytes.  Asynchronous."""
        vp = lambda v: C.c_void_p(int(v) or None)
        fx = np.ascontiguousarray(fixed, dtype=np.uint8).ravel()
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        assert fx.size == int(n_frames), "one fixed flag per frame"
        cn = None
        if counts is not None:
            cn = np.ascontiguousarray(counts, dtype=np.int32).ravel()
            assert cn.size == pr.shape[0], "one count per pair"
        self._c(lib().hg_bundle_adjust_frames_device(self._h, int(kind), int(w), int(h), int(n_frames),
                                                     fx.ctypes.data_as(C.POINTER(C.c_uint8)) if fx.size else None,
                                                     pr.ctypes.data_as(C.POINTER(C.c_int32)) if pr.size else None, pr.shape[0], vp(d_matches),
                                                     int(n_points), cn.ctypes.data_as(C.POINTER(C.c_int32)) if cn is not None and cn.size else None,
                                                     vp(d_mask), int(n_iter), float(eps), float(lambda0), float(huber), vp(d_mats_in), vp(d_mats_out),
                                                     vp(d_info), vp(d_pair_sums), vp(d_scratch), int(scratch_bytes)))

    def tps_solve_frames_device(self, d_from, n_from_sets, d_to, n_to_sets, n_points, n_frames, d_records, d_status, smoothing=0.0, d_scratch=0):
        """hg_tps_solve_frames_device: one thin-plate spline per frame through n_points pairs (from -> to, (x, y) float32 lists on the device;
        frame f reads from-list f % n_from_sets and to-list f % n_to_sets), smoothing = lambda >= 0 in the normalised frame (0 interpolates).
        d_records gets 16 + 4 n_points doubles per frame, d_status one int32 (TPS_*); d_scratch: tps_layout's bytes (0 where none are needed).
        Asynchronous."""
        vp = lambda v: C.c_void_p(int(v) or None)
        self._c(lib().hg_tps_solve_frames_device(self._h, vp(d_from), int(n_from_sets), vp(d_to), int(n_to_sets), int(n_points), int(n_frames),
                                                 float(smoothing), vp(d_records), vp(d_status), vp(d_scratch)))

    def field_tps_frames_device(self, d_records, n_points, geoms, w, h, fmt, d_field, step=1, field_offsets=None, d_scratch=0):
        """hg_field_tps_frames_device: the source field (FIELD_INDEX / FIELD_COORDS) of the frames' splines over the windows `geoms` into a
        source of w x h pixels; step > 1 evaluates a lattice and blends (an approximation; d_scratch: tps_field_layout's bytes).  Asynchronous."""
        fo = (C.c_size_t * len(geoms))(*field_offsets) if field_offsets is not None else None
        vp = lambda v: C.c_void_p(int(v) or None)
        self._c(lib().hg_field_tps_frames_device(self._h, vp(d_records), int(n_points), _geoms(geoms) if len(geoms) else None, len(geoms), int(w), int(h),
                                                 int(fmt), int(step), fo, vp(d_field), vp(d_scratch)))

    def field_camera_frames_device(self, d_records, geoms, w, h, surface, scale, u0, v0, fmt, d_field, field_offsets=None):
        """hg_field_camera_frames_device: the source field (FIELD_INDEX / FIELD_COORDS) of the cameras at d_records (32 doubles each) over the
        canvas windows `geoms` of a SURFACE_* at `scale` pixels per radian around (u0, v0), into a source of w x h pixels.  Asynchronous."""
        vp = C.c_void_p
        offs = (C.c_size_t * len(field_offsets))(*[int(o) for o in field_offsets]) if field_offsets is not None else None
        self._c(lib().hg_field_camera_frames_device(self._h, vp(d_records), _geoms(geoms) if len(geoms) else None, len(geoms), int(w), int(h), int(surface),
                                                    float(scale), float(u0), float(v0), int(fmt), offs, vp(d_field)))

    def points_camera_to_source_frames_device(self, d_records, n_frames, surface, scale, u0, v0, d_points, n_pts, n_sets, d_out):
        """hg_points_camera_to_source_frames_device: n_sets lists of n_pts absolute canvas positions to source positions of the frames' cameras
        (frame f reads list f % n_sets); a point behind the camera or beyond r2_max is the NaN pattern.  Asynchronous."""
        vp = C.c_void_p
        self._c(lib().hg_points_camera_to_source_frames_device(self._h, vp(d_records), int(n_frames), int(surface), float(scale), float(u0), float(v0),
                                                               vp(d_points), int(n_pts), int(n_sets), vp(d_out)))

    def points_camera_to_canvas_frames_device(self, d_records, n_frames, surface, scale, u0, v0, d_points, n_pts, n_sets, d_out):
        """hg_points_camera_to_canvas_frames_device: the same lists, source positions to canvas positions.  Asynchronous."""
        vp = C.c_void_p
        self._c(lib().hg_points_camera_to_canvas_frames_device(self._h, vp(d_records), int(n_frames), int(surface), float(scale), float(u0), float(v0),
                                                               vp(d_points), int(n_pts), int(n_sets), vp(d_out)))

    def points_tps_frames_device(self, d_records, n_points, n_frames, d_points, n_pts, n_sets, d_out):
        """hg_points_tps_frames_device: n_sets lists of n_pts absolute from-space positions through the frames' splines (frame f reads list
        f % n_sets); d_out gets n_frames x n_pts (x, y) float32, NaN / NaN for a position that is not finite or a failed frame.  Asynchronous."""
        vp = lambda v: C.c_void_p(int(v) or None)
        self._c(lib().hg_points_tps_frames_device(self._h, vp(d_records), int(n_points), int(n_frames), vp(d_points), int(n_pts), int(n_sets), vp(d_out)))

    def flow_dense_frames_device(self, d_from, n_frames, d_to, n_to_sets, w, h, channels, d_field, d_scratch, levels=None, n_iter=4, radius=3,
                                 min_eig=1.0, max_update=1.0, field_offsets=None, d_flow=0, d_residual=0, d_good=0, from_stride_bytes=None,
                                 to_stride_bytes=None):
        """hg_flow_dense_frames_device: pyramidal dense Lucas-Kanade between n_frames pairs of u8 planes (w x h x channels, 1 or 4): FROM plane f
        is registered onto TO plane f % n_to_sets.  d_field gets, per frame, a FIELD_COORDS field over TO's grid whose values are FROM positions
        (the NaN pattern where they leave the plane); d_flow (0: not wanted) the raw (u, v) pairs at the field's offsets, d_residual one byte per
        pixel, d_good the level-0 good flags.  levels=None: flow_default_levels(w, h); d_scratch: flow_layout's bytes.  Asynchronous."""
        vp = lambda v: C.c_void_p(int(v) or None)
        fo = (C.c_size_t * int(n_frames))(*field_offsets) if field_offsets is not None else None
        fs = int(w) * int(h) * int(channels) if from_stride_bytes is None else int(from_stride_bytes)
        ts = int(w) * int(h) * int(channels) if to_stride_bytes is None else int(to_stride_bytes)
        self._c(lib().hg_flow_dense_frames_device(self._h, vp(d_from), int(n_frames), fs, vp(d_to), int(n_to_sets), ts, int(w), int(h), int(channels),
                                                  flow_default_levels(w, h) if levels is None else int(levels), int(n_iter), int(radius),
                                                  float(min_eig), float(max_update), fo, vp(d_field), vp(d_flow), vp(d_residual), vp(d_good),
                                                  vp(d_scratch)))

    def field_compose_frames_device(self, geoms, d_outer, d_inner, wi, hi, n_inner, inner_stride_bytes, d_out, outer_offsets=None, out_offsets=None):
        """hg_field_compose_frames_device: the FIELD_COORDS fields at d_outer chained with the inner fields (wi x hi pairs each, frame f reads
        inner field f % n_inner): the bilinear frames remap of the inner field as a 2-channel float32 plane where the outer coordinate and both
        results are finite, the NaN pattern elsewhere.  Arguments as remap_bilinear_frames_device.  Asynchronous."""
        fo = (C.c_size_t * len(geoms))(*outer_offsets) if outer_offsets is not None else None
        oo = (C.c_size_t * len(geoms))(*out_offsets) if out_offsets is not None else None
        vp = lambda v: C.c_void_p(int(v) or None)
        self._c(lib().hg_field_compose_frames_device(self._h, _geoms(geoms) if len(geoms) else None, len(geoms), vp(d_outer), fo, vp(d_inner), int(wi),
                                                     int(hi), int(n_inner), int(inner_stride_bytes), vp(d_out), oo))

    def match_descriptors_frames_device(self, kind, desc_bytes, stride, d_query, n_query, counts_q, n_frames, d_train, n_train, counts_t, n_train_sets,
                                        d_counts, ratio=0.8, max_distance=0xffffffff, cross_check=False, d_query_pts=0, d_train_pts=0, d_matches=0,
                                        d_pairs=0, d_nn=0):
        """hg_match_descriptors_frames_device: per frame the nearest and second-nearest of n_train train descriptors (list f % n_train_sets) for
        each of n_query query descriptors (rows of `stride` bytes, the first desc_bytes of them data; kind DESC_BITS: Hamming, DESC_U8: squared
        L2), the ratio test (0 = none), the distance cap and the optional cross-check.  counts_q / counts_t: rows used per list, on the host, or
        None for all.  d_counts gets the accepted pairs per frame; d_pairs the compacted (i, j) lists, d_matches the (x, y, u, v) slots a fit
        reads (needs both point buffers), d_nn {j1, d1, d2, accepted} per query.  Asynchronous; every output is device memory, 0 = not wanted."""
        _, pq, _ = _counts(counts_q, n_frames)
        _, pt, _ = _counts(counts_t, n_train_sets)
        vp = lambda v: C.c_void_p(int(v) or None)
        self._c(lib().hg_match_descriptors_frames_device(self._h, int(kind), int(desc_bytes), int(stride), vp(d_query), int(n_query), pq, int(n_frames),
                                                         vp(d_train), int(n_train), pt, int(n_train_sets), float(ratio), int(max_distance) & 0xffffffff,
                                                         1 if cross_check else 0, vp(d_query_pts), vp(d_train_pts), vp(d_counts), vp(d_matches),
                                                         vp(d_pairs), vp(d_nn)))

    def detect_describe_frames_device(self, d_planes, w, h, n_planes, channels, d_counts, cell=32, per_cell=2, min_response=10 ** 10, desc_stride=32,
                                      plane_stride_bytes=None, d_points=0, d_desc=0, d_info=0):
        """hg_detect_describe_frames_device: the keypoints of n_planes u8 planes of w x h x channels (1 or 4) on the device -- Harris corners in
        integers, the best per_cell of every cell x cell cell, an orientation bin and a 256-bit descriptor each.  d_counts gets the keypoints
        per plane; d_points the (x, y) float32 positions, d_desc rows of desc_stride bytes (the first 32 the descriptor), d_info {int64 R, int32
        bin, int32 flat index}, each n_planes x detect_layout(...)[2] slots: what match_descriptors_frames_device takes as a query or train side.
        Asynchronous; every output is device memory, 0 = not wanted."""
        vp = lambda v: C.c_void_p(int(v) or None)
        stride = int(w) * int(h) * int(channels) if plane_stride_bytes is None else int(plane_stride_bytes)
        self._c(lib().hg_detect_describe_frames_device(self._h, vp(d_planes), int(w), int(h), int(n_planes), stride, int(channels), int(cell), int(per_cell),
                                                       int(min_response), int(desc_stride), vp(d_counts), vp(d_points), vp(d_desc), vp(d_info)))

    def mosaic_overlap_stats_device(self, geoms, d_coords, d_frames, channels, canvas, d_stats, field_offsets=None, frame_offsets=None):
        """The overlaps of a set of uint8 frames measured on the device (asynchronous): d_stats gets F * F * 2 uint64 words -- for every ordered
        pair (a, b) the canvas pixels both frames contribute to and frame a's summed intensity (colour channels, no alpha) over them.  The
        arguments are mosaic_frames_device's; at most 256 frames.  mosaic_solve_gains turns the downloaded words into gains."""
        fo = (C.c_size_t * len(geoms))(*field_offsets) if field_offsets is not None else None
        po = (C.c_size_t * len(geoms))(*frame_offsets) if frame_offsets is not None else None
        self._c(lib().hg_mosaic_overlap_stats_device(self._h, _geoms(geoms) if len(geoms) else None, len(geoms), C.c_void_p(int(d_coords) or None), fo,
                                                     C.c_void_p(int(d_frames) or None), po, int(channels), Geom(*[int(v) for v in canvas]),
                                                     C.c_void_p(int(d_stats) or None)))

    # ---- piecewise
    def piecewise_set_mesh(self, src_pts, tris, min_src_x, min_src_y):
        s, sp = _f32(src_pts)
        t = np.ascontiguousarray(tris, dtype=np.uint32)
        self._c(lib().hg_piecewise_set_mesh(self._h, sp, s.size // 2, t.ctypes.data_as(C.POINTER(C.c_uint32)), t.size // 3,
                                            int(min_src_x), int(min_src_y)))
        self._n_pts, self._n_tris = s.size // 2, t.size // 3      # the C ABI takes plain pointers: sizes are checked on this side

    def piecewise_prepare(self, dst_pts, geom):
        d, dp = _f32(dst_pts)
        assert d.size == 2 * self._n_pts, "one x,y pair per mesh point"
        self._geom = Geom(*[int(v) for v in geom])
        self._c(lib().hg_piecewise_prepare(self._h, dp, self._geom))

    def _out_array(self):
        g = self._geom
        return np.zeros((max(g.obj_h, 0), max(g.obj_w, 0), 4), np.uint8)

    def warp_inverse_piecewise(self):
        out = self._out_array()
        self._c(lib().hg_warp_inverse_piecewise(self._h, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def warp_inverse_piecewise_via_map(self):
        out = self._out_array()
        self._c(lib().hg_warp_inverse_piecewise_via_map(self._h, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def get_tri_map(self, fused=False):
        g = self._geom
        m = np.empty(max(g.obj_w, 0) * max(g.obj_h, 0), np.int16)
        fn = lib().hg_get_tri_map_fused if fused else lib().hg_get_tri_map
        self._c(fn(self._h, m.ctypes.data_as(C.POINTER(C.c_int16)), m.size))
        return m

    def get_matrices(self, n_tris):
        assert n_tris == self._n_tris, "the library fills n_triangles x 6 floats"
        fwd = np.empty((n_tris, 6), np.float32)
        inv = np.empty((n_tris, 6), np.float32)
        self._c(lib().hg_get_matrices(self._h, fwd.ctypes.data_as(C.POINTER(C.c_float)), inv.ctypes.data_as(C.POINTER(C.c_float))))
        return fwd, inv

    def piecewise_set_frames(self, dst_pts, geoms, offsets=None):
        d, dp = _f32(dst_pts)
        assert d.size == 2 * self._n_pts * len(geoms), "frames x mesh points x,y pairs"
        offs = (C.c_size_t * len(geoms))(*offsets) if offsets is not None else None
        self._c(lib().hg_piecewise_set_frames(self._h, dp, _geoms(geoms), offs, len(geoms)))

    def _src_args(self, src_pts, min_src, dst_pts, geoms, offsets):
        (s, sp), (d, dp) = _f32(src_pts), _f32(dst_pts)
        n = len(geoms)
        assert s.size == 2 * self._n_pts * n and d.size == 2 * self._n_pts * n, "frames x mesh points x,y pairs on both sides"
        ms = msp = None
        if min_src is not None:
            ms = np.ascontiguousarray(min_src, dtype=np.int32)
            assert ms.size == 2 * n, "one {minSrcX, minSrcY} pair per frame"
            msp = ms.ctypes.data_as(C.POINTER(C.c_int32))
        offs = (C.c_size_t * n)(*offsets) if offsets is not None else None
        if n == 1:
            self._geom = Geom(*[int(v) for v in geoms[0]])      # (the single-frame forms and taps describe this frame)
        return (s, d, ms), (sp, msp, dp, _geoms(geoms), offs, n)

    def piecewise_set_frames_src(self, src_pts, min_src, dst_pts, geoms, offsets=None):
        """Frames that bring their own source points (hg_piecewise_set_frames_src); min_src=None passes NULL: each frame's minima are
        the rounded bounding-box minimum of its own source points."""
        keep, args = self._src_args(src_pts, min_src, dst_pts, geoms, offsets)
        self._c(lib().hg_piecewise_set_frames_src(self._h, *args))

    def warp_inverse_piecewise_src_batch_device(self, src_pts, min_src, dst_pts, geoms, offsets, d_out):
        keep, args = self._src_args(src_pts, min_src, dst_pts, geoms, offsets)
        self._c(lib().hg_warp_inverse_piecewise_src_batch_device(self._h, *args, C.c_void_p(int(d_out))))

    def frame_set_args(self, dst_pts, geoms, offsets=None):
        """The ctypes arguments of piecewise_set_frames, built once: a caller that uploads one of a few point sets per step
        (bench.py --points fresh) then pays only the C call.  Returns an opaque tuple for piecewise_set_frames_prepared."""
        d, dp = _f32(dst_pts)
        assert d.size == 2 * self._n_pts * len(geoms), "frames x mesh points x,y pairs"
        offs = (C.c_size_t * len(geoms))(*offsets) if offsets is not None else None
        return (d, dp, _geoms(geoms), offs, len(geoms))

    def piecewise_set_frames_prepared(self, args):
        self._c(lib().hg_piecewise_set_frames(self._h, args[1], args[2], args[3], args[4]))

    def warp_inverse_piecewise_frames_device(self, d_out):
        self._c(lib().hg_warp_inverse_piecewise_frames_device(self._h, C.c_void_p(int(d_out))))


# ------------------------------------------------------------------ several GPUs, one host thread (hg_multi_*)

def multi_plan_fanout(access):
    """Copy plan of the shared-source fan-out (pure function, no GPU): access = G x G array, access[p, q] != 0 when device q copies
    straight out of device p's memory.  Returns a list of (dst, src or -1 = host buffer, slice, phase)."""
    a = np.ascontiguousarray(access, np.uint8)
    G = a.shape[0]
    assert a.shape == (G, G)
    n = lib().hg_multi_plan_fanout(G, a.ctypes.data, None, 0)
    if n < 0:
        raise RuntimeError("hg_multi_plan_fanout: bad arguments")
    ops = np.zeros((max(n, 1), 4), np.int32)
    lib().hg_multi_plan_fanout(G, a.ctypes.data, ops.ctypes.data, n)
    return [tuple(int(v) for v in ops[k]) for k in range(n)]


def multi_partition(n_frames, n_devices, index):
    """(first, count): the contiguous block of frames device `index` of `n_devices` warps (pure function, no GPU)."""
    first, count = C.c_int(0), C.c_int(0)
    _check(lib().hg_multi_partition(int(n_frames), int(n_devices), int(index), C.byref(first), C.byref(count)))
    return first.value, count.value


class PinnedBuffer:
    """Page-locked host memory from hg_host_alloc, exposed as a numpy uint8 array."""

    def __init__(self, nbytes):
        self._p = C.c_void_p()
        _check(lib().hg_host_alloc(int(nbytes), C.byref(self._p)))
        self.array = np.ctypeslib.as_array(C.cast(self._p, C.POINTER(C.c_uint8)), shape=(int(nbytes),))

    @property
    def ptr(self):
        return self._p.value

    def free(self):
        if self._p:
            self.array = None
            lib().hg_host_free(self._p)
            self._p = C.c_void_p()


class Multi:
    """hg_multi: the batch caller loop spread over several devices of one node from ONE host thread."""

    def __init__(self, devices):
        ids = (C.c_int * len(devices))(*[int(d) for d in devices])
        self._h = C.c_void_p()
        code = lib().hg_multi_create(ids, len(devices), C.byref(self._h))
        if code != 0:
            self._h = C.c_void_p()
            msg = lib().hg_multi_last_error(None)
            raise HgError(code, msg.decode() if msg else "?")
        self._n_pts = 0
        self._geoms = []

    def _c(self, code):
        if code != 0:
            msg = lib().hg_multi_last_error(self._h)
            raise HgError(code, msg.decode() if msg else "?")

    def peer_note(self):
        """'' when every pair of distinct devices has peer access, else a text naming the pairs without it."""
        msg = lib().hg_multi_peer_note(self._h)
        return msg.decode() if msg else ""

    def peer_access(self, from_index, to_index):
        return lib().hg_multi_peer_access(self._h, int(from_index), int(to_index))

    def close(self):
        if self._h:
            lib().hg_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_count(self):
        return lib().hg_multi_device_count(self._h)

    def set_option(self, key, value):
        for k in range(self.device_count()):
            ctx = lib().hg_multi_ctx(self._h, k)
            _check(lib().hg_set_option(C.c_void_p(ctx), key.encode(), int(value)), C.c_void_p(ctx))

    def set_sampling(self, mode):
        """Context.set_sampling on every per-device context."""
        self._c(lib().hg_multi_set_sampling(self._h, int(mode)))

    def set_image(self, rgba):
        a = np.ascontiguousarray(rgba, dtype=np.uint8)
        h, w = a.shape[:2]
        self._c(lib().hg_multi_set_image(self._h, a.ctypes.data_as(C.POINTER(C.c_uint8)), w, h))

    def piecewise_set_mesh(self, src_pts, tris, min_src_x, min_src_y):
        s, sp = _f32(src_pts)
        t = np.ascontiguousarray(tris, dtype=np.uint32)
        self._c(lib().hg_multi_piecewise_set_mesh(self._h, sp, s.size // 2, t.ctypes.data_as(C.POINTER(C.c_uint32)), t.size // 3, int(min_src_x), int(min_src_y)))
        self._n_pts = s.size // 2

    def warp_piecewise_batch(self, dst_pts, geoms, out_ptrs=None):
        """out_ptrs: None (frames stay on their devices) or one host address per frame."""
        d, dp = _f32(dst_pts)
        assert d.size == 2 * self._n_pts * len(geoms)
        ptrs = (C.c_void_p * len(geoms))(*[C.c_void_p(int(p)) for p in out_ptrs]) if out_ptrs is not None else None
        self._geoms = [tuple(int(v) for v in g) for g in geoms]
        self._c(lib().hg_multi_warp_piecewise_batch(self._h, dp, _geoms(geoms), len(geoms), ptrs))

    @staticmethod
    def _image_ptrs(images, n):
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        assert len(imgs) == n and all(im.shape == imgs[0].shape and im.ndim == 3 and im.shape[2] == 4 for im in imgs), "one H x W x 4 image per frame"
        return imgs, (C.c_void_p * n)(*[C.c_void_p(im.ctypes.data) for im in imgs]), imgs[0].shape[1], imgs[0].shape[0]

    def warp_piecewise_batch_images(self, dst_pts, geoms, images, out_ptrs=None):
        """One source per frame (the video loop): images[f] is frame f's H x W x 4 uint8 source; every device uploads its own block."""
        d, dp = _f32(dst_pts)
        assert d.size == 2 * self._n_pts * len(geoms)
        keep, iptrs, w, h = self._image_ptrs(images, len(geoms))
        ptrs = (C.c_void_p * len(geoms))(*[C.c_void_p(int(p)) for p in out_ptrs]) if out_ptrs is not None else None
        self._geoms = [tuple(int(v) for v in g) for g in geoms]
        self._c(lib().hg_multi_warp_piecewise_batch_images(self._h, dp, _geoms(geoms), len(geoms), iptrs, w, h, ptrs))

    def warp_geometric_batch_images(self, kind, from_pts, to_pts, geoms, images, out_ptrs=None):
        per = 6 if int(kind) == 0 else 8
        (a, ap), (b, bp) = _f32(from_pts), _f32(to_pts)
        assert a.size == per * len(geoms) and b.size == per * len(geoms)
        keep, iptrs, w, h = self._image_ptrs(images, len(geoms))
        ptrs = (C.c_void_p * len(geoms))(*[C.c_void_p(int(p)) for p in out_ptrs]) if out_ptrs is not None else None
        self._geoms = [tuple(int(v) for v in g) for g in geoms]
        self._c(lib().hg_multi_warp_geometric_batch_images(self._h, int(kind), ap, bp, _geoms(geoms), len(geoms), iptrs, w, h, ptrs))

    def warp_geometric_batch(self, kind, from_pts, to_pts, geoms, out_ptrs=None):
        per = 6 if int(kind) == 0 else 8
        (a, ap), (b, bp) = _f32(from_pts), _f32(to_pts)
        assert a.size == per * len(geoms) and b.size == per * len(geoms)
        ptrs = (C.c_void_p * len(geoms))(*[C.c_void_p(int(p)) for p in out_ptrs]) if out_ptrs is not None else None
        self._geoms = [tuple(int(v) for v in g) for g in geoms]
        self._c(lib().hg_multi_warp_geometric_batch(self._h, int(kind), ap, bp, _geoms(geoms), len(geoms), ptrs))

    def frame(self, f):
        """(device index, device pointer, bytes) of frame f of the last batch."""
        dev, ptr, n = C.c_int(0), C.c_void_p(), C.c_size_t(0)
        self._c(lib().hg_multi_frame(self._h, int(f), C.byref(dev), C.byref(ptr), C.byref(n)))
        return dev.value, ptr.value, n.value

    def frame_to_host(self, f):
        dev, ptr, n = self.frame(f)
        out = np.empty(n, np.uint8)
        ctx = C.c_void_p(lib().hg_multi_ctx(self._h, dev))
        _check(lib().hg_copy_to_host(ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), n), ctx)
        g = self._geoms[f]
        return out.reshape(max(g[3], 0), max(g[2], 0), 4)
