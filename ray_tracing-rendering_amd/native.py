"""ctypes binding of ``librtr_hip.so`` (the C ABI of include/rtr_hip.h).

There is no CPU fallback: if the library is missing or no GPU is visible, every device entry
point raises.  The oracle under ``oracle/`` is test infrastructure and is never loaded here."""
import ctypes as C
import os
import weakref

import numpy as np

from . import _abi as A
from .scene import Scene

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

_STATUS = {A.RTR_ERR_INVALID: "RTR_ERR_INVALID", A.RTR_ERR_UNSUPPORTED: "RTR_ERR_UNSUPPORTED",
           A.RTR_ERR_DEVICE: "RTR_ERR_DEVICE", A.RTR_ERR_NO_SCENE: "RTR_ERR_NO_SCENE",
           A.RTR_ERR_CANCELLED: "RTR_ERR_CANCELLED", A.RTR_ERR_NOMEM: "RTR_ERR_NOMEM"}

# every symbol include/rtr_hip.h declares (librtr_hip.so) ...
EXPORTS = ("rtr_abi_version", "rtr_device_count", "rtr_create", "rtr_destroy", "rtr_set_stream",
           "rtr_upload_scene", "rtr_render_device", "rtr_render_host", "rtr_render_tiles_host", "rtr_plan_chunks", "rtr_li_samples", "rtr_li_rays",
           "rtr_synchronize", "rtr_cancel", "rtr_get_stats", "rtr_last_error", "rtr_sample_seed", "rtr_validate_scene",
           "rtr_accum_create", "rtr_accum_render", "rtr_accum_resolve", "rtr_accum_tiles", "rtr_accum_destroy",
           "rtr_accum_create_ex", "rtr_accum_render_tiles", "rtr_accum_moments", "rtr_accum_errors", "rtr_accum_refine",
           "rtr_denoise_defaults", "rtr_accum_features", "rtr_accum_denoise", "rtr_denoise_host",
           "rtr_query_closest", "rtr_query_occluded", "rtr_query_closest_device", "rtr_query_occluded_device",
           "rtr_set_camera", "rtr_get_camera", "rtr_accum_reset", "rtr_temporal_defaults", "rtr_history_create",
           "rtr_history_clear", "rtr_history_destroy", "rtr_history_planes", "rtr_accum_denoise_temporal",
           "rtr_display_defaults", "rtr_display_srgb_thresholds", "rtr_display_histogram", "rtr_display_host",
           "rtr_display_device", "rtr_accum_resolve_device", "rtr_accum_features_device", "rtr_accum_denoise_device",
           "rtr_accum_denoise_temporal_device", "rtr_gather_defaults", "rtr_gather_occlusion", "rtr_gather_radiance",
           "rtr_gather_occlusion_device", "rtr_gather_radiance_device", "rtr_gather_ray",
           "rtr_probe_visibility", "rtr_probe_radiance", "rtr_probe_visibility_device", "rtr_probe_radiance_device",
           "rtr_probe_ray", "rtr_sh_basis", "rtr_sh_irradiance", "rtr_probe_lookup", "rtr_probe_lookup_device",
           "rtr_probe_lookup_one", "rtr_capture_defaults", "rtr_capture_cube", "rtr_capture_cube_device", "rtr_capture_ray",
           "rtr_cube_lookup", "rtr_cube_lookup_device", "rtr_cube_lookup_one", "rtr_latlong_direction",
           "rtr_cube_to_latlong", "rtr_write_rgbe", "rtr_cube_filter_defaults", "rtr_cube_filter", "rtr_cube_filter_device",
           "rtr_cube_filter_one", "rtr_cube_chain_plan", "rtr_cube_chain_lookup", "rtr_cube_chain_lookup_device",
           "rtr_cube_chain_lookup_one", "rtr_probe_depth_defaults", "rtr_probe_depth", "rtr_probe_depth_device",
           "rtr_probe_depth_ray", "rtr_octa_encode", "rtr_octa_decode", "rtr_probe_lookup_visible",
           "rtr_probe_lookup_visible_device", "rtr_probe_lookup_visible_one", "rtr_brdf_table", "rtr_brdf_table_device",
           "rtr_brdf_entry_one", "rtr_brdf_fetch_one", "rtr_shade_ibl", "rtr_shade_ibl_device", "rtr_shade_ibl_one",
           "rtr_preview_defaults", "rtr_preview_ray", "rtr_preview_samples", "rtr_preview_samples_device", "rtr_preview",
           "rtr_preview_device", "rtr_capture_set_lookup", "rtr_capture_set_lookup_device", "rtr_capture_set_lookup_one",
           "rtr_shade_ibl_set", "rtr_shade_ibl_set_device", "rtr_shade_ibl_set_one", "rtr_preview_set", "rtr_preview_set_device")
# ... and include/rtr_hip_test.h (librtr_hip_test.so: device unit kernels of the parity tests, not part of the product)
TEST_EXPORTS = ("rtr_test_hits", "rtr_test_materials", "rtr_test_lights", "rtr_test_li", "rtr_test_reference_order",
                "rtr_test_stream8", "rtr_test_sincos_exhaustive", "rtr_test_shared_division", "rtr_test_issue_rates", "rtr_test_last_kernel",
                "rtr_test_last_gather", "rtr_test_last_probe", "rtr_test_last_capture", "rtr_test_last_probe_depth",
                "rtr_test_temporal_planes", "rtr_test_scene_plan", "rtr_test_flat_hits", "rtr_test_pair_frames",
                "rtr_test_pair_frame_host", "rtr_test_pair_cast", "rtr_test_pair_cast_text", "rtr_test_pair_resident", "rtr_test_queue_blocks_host", "rtr_test_queue_pack_host",
                "rtr_test_scatter", "rtr_test_materials_ms", "rtr_test_scatter_ms", "rtr_test_lights_ms", "rtr_test_pow5",
                "rtr_test_pow5_host", "rtr_test_udiv", "rtr_test_scene_consts", "rtr_test_accum_load",
                "rtr_test_accum_plan", "rtr_test_accum_commit", "rtr_test_rcp_lane", "rtr_test_sqrt_lane",
                "rtr_test_lane_specials", "rtr_test_lane_host", "rtr_test_draw_forms", "rtr_test_draw_callers",
                "rtr_test_draw_host", "rtr_test_draw_host_range")
_TEST_LIB = None


class SceneInfoC(C.Structure):
    _fields_ = [("stack_words", C.c_int32), ("has_media", C.c_int32), ("needs_uv", C.c_int32),
                ("graph_depth", C.c_int32), ("fast_ok", C.c_int32), ("fast_instances", C.c_int32),
                ("fast_refs", C.c_int32), ("fast_stack_words", C.c_int32), ("compiled_subtrees", C.c_int32),
                ("program_steps", C.c_int32), ("inverted_boxes", C.c_int32), ("top_trees", C.c_int32)]


class KernelRecordC(C.Structure):
    """rtr_kernel_record of include/rtr_hip_test.h"""
    _fields_ = [(name, C.c_int32) for name in ("pipeline", "integrator", "trav", "ms", "sorted", "shade_phases", "lean",
                                               "quadlit", "sort", "media", "machine", "accum", "pair", "queue")]


class GatherRecordC(C.Structure):
    """rtr_gather_record of include/rtr_hip_test.h"""
    _fields_ = [(name, C.c_int32) for name in ("integ", "trav", "broadcast", "lg")]


class ProbeRecordC(C.Structure):
    """rtr_probe_record of include/rtr_hip_test.h"""
    _fields_ = [(name, C.c_int32) for name in ("integ", "trav", "lg")]


class CaptureRecordC(C.Structure):
    """rtr_capture_record of include/rtr_hip_test.h"""
    _fields_ = [(name, C.c_int32) for name in ("integ", "trav", "lg")]


class ProbeDepthRecordC(C.Structure):
    """rtr_probe_depth_record of include/rtr_hip_test.h"""
    _fields_ = [(name, C.c_int32) for name in ("trav", "lg")]


class ScenePlanC(C.Structure):
    """rtr_scene_plan of include/rtr_hip_test.h"""
    _fields_ = [(name, C.c_int32) for name in (
        "fast_ok", "has_media", "flat_scene", "flat_guarded", "lean_materials", "quad_lights_only", "uv_order_dependent",
        "machine_ok", "guarded_program", "top_tree", "needs_uv", "n_material_types", "shared_div", "pair_cast", "n_steps",
        "n_visits", "n_refs", "fast_stack_words", "walk_stack_words", "n_tie_refs", "n_guard_refs", "pick_trav", "mega_trav",
        "mega_ms", "mega_sorted", "mega_pair", "n_finish")]


# rtr_finish_record of include/rtr_hip_test.h
FINISH_DTYPE = np.dtype([("kind", "<i4"), ("material", "<i4"), ("levels", "<i4"), ("flip", "<i4"), ("op", "<f8", (2, 3)),
                         ("g", "<f8", (4,))])


# rtr_pair_frame_record and rtr_pair_record of include/rtr_hip_test.h
PAIR_FRAME_DTYPE = np.dtype([("ao", "<f8", (3,)), ("ad", "<f8", (3,)), ("bo", "<f8", (3,)), ("bd", "<f8", (3,)),
                             ("fo", "<f8", (3,)), ("fd", "<f8", (3,)), ("same_frame", "<i4"), ("pad", "<i4")])
PAIR_DTYPE = np.dtype([("ao", "<f8", (3,)), ("ad", "<f8", (3,)), ("a_tmax", "<f8"), ("bo", "<f8", (3,)), ("bd", "<f8", (3,)),
                       ("b_tmax", "<f8"), ("a_t", "<f8"), ("s_a_t", "<f8"), ("a_ref", "<i4"), ("a_inst", "<i4"),
                       ("b_hit", "<i4"), ("s_a_ref", "<i4"), ("s_a_inst", "<i4"), ("s_b_hit", "<i4"), ("recasts", "<i4"),
                       ("pad", "<i4")])
assert PAIR_DTYPE.itemsize == 160
QUEUE_BLOCK_DTYPE = np.dtype([(name, "<i4") for name in ("slot", "quarter", "chunk", "s0", "s1", "ref_s0", "ref_s1", "pad")])
MS_LEAN, MS_FULL, MS_QUADLIT = 0, 1, 2  # RT_MS_* (csrc/rt_device.h): the material-set instantiations of the kernels
FRAME_SHAPES = ("none", "T", "R", "TR", "RT", "other")  # FInst::shape (csrc/rt_device.h: RT_SHAPE_*)


class RtrError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("%s (%d): %s" % (_STATUS.get(code, "rtr_status"), code, message))
        self.code = code
        self.message = message


def library_path():
    # RTR_HIP_LIBRARY lets a tuning run point at an alternative build of the same ABI
    return os.environ.get("RTR_HIP_LIBRARY") or os.path.join(_HERE, "librtr_hip.so")


def lib():
    """Load librtr_hip.so; raises if it has not been built (``__graft_entry__.build()``)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise RtrError(A.RTR_ERR_DEVICE, "HIP library %s is missing: run __graft_entry__.build(); there is no "
                       "CPU fallback" % path)
    L = C.CDLL(path)
    P = C.POINTER
    vp = C.c_void_p
    L.rtr_abi_version.restype = C.c_uint32
    L.rtr_device_count.restype = C.c_int
    L.rtr_create.argtypes = [C.c_int, P(vp)]
    L.rtr_destroy.argtypes = [vp]
    L.rtr_destroy.restype = None
    L.rtr_set_stream.argtypes = [vp, vp]
    L.rtr_upload_scene.argtypes = [vp, P(A.SceneDescC)]
    L.rtr_render_device.argtypes = [vp, P(A.RenderParamsC), vp, C.c_int64, C.c_int]
    L.rtr_render_host.argtypes = [vp, P(A.RenderParamsC), vp, C.c_int64]
    L.rtr_plan_chunks.argtypes = [vp, P(A.RenderParamsC)]
    L.rtr_li_samples.argtypes = [vp, P(A.RenderParamsC), vp, vp, C.c_int64]
    L.rtr_synchronize.argtypes = [vp]
    L.rtr_cancel.argtypes = [vp]
    L.rtr_get_stats.argtypes = [vp, P(A.RenderStatsC)]
    L.rtr_last_error.argtypes = [vp]
    L.rtr_last_error.restype = C.c_char_p
    L.rtr_sample_seed.argtypes = [C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.rtr_sample_seed.restype = C.c_uint32
    L.rtr_validate_scene.argtypes = [P(A.SceneDescC), P(SceneInfoC), C.c_char_p, C.c_size_t]
    L.rtr_li_rays.argtypes = [vp, P(A.RenderParamsC), vp, vp, C.c_int64]
    L.rtr_accum_create.argtypes = [vp, P(A.RenderParamsC), P(vp)]
    L.rtr_accum_render.argtypes = [vp, vp, C.c_int32, C.c_int]
    L.rtr_accum_resolve.argtypes = [vp, vp, vp, C.c_int64, vp]
    L.rtr_accum_tiles.argtypes = [vp, vp, vp, vp, C.c_int64, P(C.c_int64)]
    L.rtr_accum_destroy.argtypes = [vp]
    L.rtr_accum_destroy.restype = None
    L.rtr_accum_create_ex.argtypes = [vp, P(A.RenderParamsC), C.c_uint32, P(vp)]
    L.rtr_accum_render_tiles.argtypes = [vp, vp, vp, C.c_int64, C.c_int]
    L.rtr_accum_moments.argtypes = [vp, vp, vp, C.c_int64]
    L.rtr_accum_errors.argtypes = [vp, vp, vp, C.c_int64, P(C.c_int64)]
    L.rtr_accum_refine.argtypes = [vp, vp, C.c_double, C.c_int32, C.c_int32, C.c_int, P(C.c_int32)]
    L.rtr_denoise_defaults.argtypes = [P(A.DenoiseParamsC)]
    L.rtr_denoise_defaults.restype = None
    L.rtr_accum_features.argtypes = [vp, vp, C.c_int32, vp, C.c_int64]
    L.rtr_accum_denoise.argtypes = [vp, vp, P(A.DenoiseParamsC), vp, C.c_int64, vp]
    L.rtr_denoise_host.argtypes = [vp, P(A.DenoiseParamsC), C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp]
    L.rtr_query_closest.argtypes = [vp, vp, vp, C.c_int64, C.c_int32]
    L.rtr_query_occluded.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int32]
    L.rtr_query_closest_device.argtypes = [vp, vp, vp, C.c_int64, C.c_int32, C.c_int]
    L.rtr_query_occluded_device.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int32, C.c_int]
    L.rtr_set_camera.argtypes = [vp, P(A.CameraC)]
    L.rtr_get_camera.argtypes = [vp, P(A.CameraC)]
    L.rtr_accum_reset.argtypes = [vp, vp, C.c_uint32]
    L.rtr_temporal_defaults.argtypes = [P(A.TemporalParamsC)]
    L.rtr_temporal_defaults.restype = None
    L.rtr_history_create.argtypes = [vp, P(A.RenderParamsC), P(vp)]
    L.rtr_history_clear.argtypes = [vp, vp]
    L.rtr_history_destroy.argtypes = [vp]
    L.rtr_history_destroy.restype = None
    L.rtr_history_planes.argtypes = [vp, vp, vp, C.c_int64]
    L.rtr_accum_denoise_temporal.argtypes = [vp, vp, vp, P(A.DenoiseParamsC), P(A.TemporalParamsC), vp, C.c_int64, vp]
    L.rtr_display_defaults.argtypes = [P(A.DisplayParamsC)]
    L.rtr_display_defaults.restype = None
    L.rtr_display_srgb_thresholds.argtypes = [vp]
    L.rtr_display_srgb_thresholds.restype = None
    L.rtr_display_histogram.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_int64, vp, P(C.c_int64)]
    L.rtr_display_host.argtypes = [vp, P(A.DisplayParamsC), C.c_int32, C.c_int32, vp, C.c_int64, vp, vp, P(A.DisplayResultC)]
    L.rtr_display_device.argtypes = [vp, P(A.DisplayParamsC), C.c_int32, C.c_int32, vp, C.c_int64, vp, vp,
                                     P(A.DisplayResultC), C.c_int]
    for name, argtypes in A.DEVICE_OUTPUT_SIGNATURES.items():
        getattr(L, name).argtypes = argtypes
    L.rtr_gather_defaults.argtypes = [P(A.GatherParamsC)]
    L.rtr_gather_defaults.restype = None
    L.rtr_gather_occlusion.argtypes = [vp, P(A.GatherParamsC), vp, vp, C.c_int64]
    L.rtr_gather_radiance.argtypes = [vp, P(A.RenderParamsC), P(A.GatherParamsC), vp, vp, C.c_int64]
    L.rtr_gather_occlusion_device.argtypes = [vp, P(A.GatherParamsC), vp, vp, C.c_int64, C.c_int]
    L.rtr_gather_radiance_device.argtypes = [vp, P(A.RenderParamsC), P(A.GatherParamsC), vp, vp, C.c_int64, C.c_int]
    L.rtr_gather_ray.argtypes = [P(A.GatherParamsC), vp, C.c_int64, C.c_int32, vp]
    L.rtr_probe_visibility.argtypes = [vp, P(A.GatherParamsC), vp, vp, C.c_int64]
    L.rtr_probe_radiance.argtypes = [vp, P(A.RenderParamsC), P(A.GatherParamsC), vp, vp, C.c_int64]
    L.rtr_probe_visibility_device.argtypes = [vp, P(A.GatherParamsC), vp, vp, C.c_int64, C.c_int]
    L.rtr_probe_radiance_device.argtypes = [vp, P(A.RenderParamsC), P(A.GatherParamsC), vp, vp, C.c_int64, C.c_int]
    L.rtr_probe_ray.argtypes = [P(A.GatherParamsC), vp, C.c_int64, C.c_int32, vp]
    L.rtr_sh_basis.argtypes = [vp, vp]
    L.rtr_sh_basis.restype = None
    L.rtr_sh_irradiance.argtypes = [vp, vp, vp]
    L.rtr_probe_lookup.argtypes = [vp, P(A.ProbeGridC), vp, vp, vp, C.c_int64]
    L.rtr_probe_lookup_device.argtypes = [vp, P(A.ProbeGridC), vp, vp, vp, C.c_int64, C.c_int]
    L.rtr_probe_lookup_one.argtypes = [P(A.ProbeGridC), vp, vp, vp]
    L.rtr_probe_depth_defaults.argtypes = [P(A.ProbeDepthParamsC)]
    L.rtr_probe_depth_defaults.restype = None
    L.rtr_probe_depth.argtypes = [vp, P(A.ProbeDepthParamsC), vp, vp, C.c_int64]
    L.rtr_probe_depth_device.argtypes = [vp, P(A.ProbeDepthParamsC), vp, vp, C.c_int64, C.c_int]
    L.rtr_probe_depth_ray.argtypes = [P(A.ProbeDepthParamsC), vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, vp]
    L.rtr_octa_encode.argtypes = [vp, vp]
    L.rtr_octa_encode.restype = None
    L.rtr_octa_decode.argtypes = [vp, vp]
    L.rtr_octa_decode.restype = None
    L.rtr_probe_lookup_visible.argtypes = [vp, P(A.ProbeGridC), vp, vp, P(A.ProbeVisibleParamsC), vp, vp, C.c_int64]
    L.rtr_probe_lookup_visible_device.argtypes = [vp, P(A.ProbeGridC), vp, vp, P(A.ProbeVisibleParamsC), vp, vp, C.c_int64,
                                                  C.c_int]
    L.rtr_probe_lookup_visible_one.argtypes = [P(A.ProbeGridC), vp, vp, P(A.ProbeVisibleParamsC), vp, vp]
    L.rtr_capture_defaults.argtypes = [P(A.CaptureParamsC)]
    L.rtr_capture_defaults.restype = None
    L.rtr_capture_cube.argtypes = [vp, P(A.RenderParamsC), P(A.CaptureParamsC), vp, vp, C.c_int64]
    L.rtr_capture_cube_device.argtypes = [vp, P(A.RenderParamsC), P(A.CaptureParamsC), vp, vp, C.c_int64, C.c_int]
    L.rtr_capture_ray.argtypes = [P(A.CaptureParamsC), vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp]
    L.rtr_cube_lookup.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int64]
    L.rtr_cube_lookup_device.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int64, C.c_int]
    L.rtr_cube_lookup_one.argtypes = [C.c_int32, vp, vp, vp]
    L.rtr_latlong_direction.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp]
    L.rtr_cube_to_latlong.argtypes = [C.c_int32, vp, C.c_int32, C.c_int32, vp]
    L.rtr_write_rgbe.argtypes = [C.c_char_p, C.c_int32, C.c_int32, vp]
    L.rtr_cube_filter_defaults.argtypes = [P(A.CubeFilterParamsC)]
    L.rtr_cube_filter_defaults.restype = None
    L.rtr_cube_filter.argtypes = [vp, P(A.CubeFilterParamsC), vp, vp, C.c_int64]
    L.rtr_cube_filter_device.argtypes = [vp, P(A.CubeFilterParamsC), vp, vp, C.c_int64, C.c_int]
    L.rtr_cube_filter_one.argtypes = [P(A.CubeFilterParamsC), vp, C.c_int32, C.c_int32, C.c_int32, vp]
    L.rtr_cube_chain_plan.argtypes = [C.c_int32, C.c_int32, vp, P(C.c_int64)]
    L.rtr_cube_chain_lookup.argtypes = [vp, vp, C.c_int32, vp, C.c_int64, vp, vp, C.c_int64]
    L.rtr_cube_chain_lookup_device.argtypes = [vp, vp, C.c_int32, vp, C.c_int64, vp, vp, C.c_int64, C.c_int]
    L.rtr_cube_chain_lookup_one.argtypes = [vp, C.c_int32, vp, vp, vp]
    L.rtr_brdf_table.argtypes = [vp, P(A.BrdfParamsC), vp]
    L.rtr_brdf_table_device.argtypes = [vp, P(A.BrdfParamsC), vp, C.c_int]
    L.rtr_brdf_entry_one.argtypes = [P(A.BrdfParamsC), C.c_int32, C.c_int32, vp]
    L.rtr_brdf_fetch_one.argtypes = [C.c_int32, C.c_int32, vp, C.c_double, C.c_double, vp]
    L.rtr_shade_ibl.argtypes = [vp, P(A.ShadeEnvC), vp, vp, C.c_int64]
    L.rtr_shade_ibl_device.argtypes = [vp, P(A.ShadeEnvC), vp, vp, C.c_int64, C.c_int]
    L.rtr_shade_ibl_one.argtypes = [P(A.ShadeEnvC), vp, vp]
    L.rtr_preview_defaults.argtypes = [P(A.PreviewParamsC)]
    L.rtr_preview_defaults.restype = None
    L.rtr_preview_ray.argtypes = [P(A.CameraC), P(A.PreviewParamsC), C.c_int32, C.c_int32, C.c_int32, vp]
    L.rtr_preview_samples.argtypes = [vp, P(A.PreviewParamsC), vp]
    L.rtr_preview_samples_device.argtypes = [vp, P(A.PreviewParamsC), vp, C.c_int]
    L.rtr_preview.argtypes = [vp, P(A.PreviewParamsC), P(A.ShadeEnvC), vp, C.c_int64, vp]
    L.rtr_preview_device.argtypes = [vp, P(A.PreviewParamsC), P(A.ShadeEnvC), vp, C.c_int64, vp, C.c_int]
    L.rtr_capture_set_lookup.argtypes = [vp, P(A.CaptureSetC), vp, C.c_int32, vp, C.c_int64, vp, vp, C.c_int64]
    L.rtr_capture_set_lookup_device.argtypes = [vp, P(A.CaptureSetC), vp, C.c_int32, vp, C.c_int64, vp, vp, C.c_int64, C.c_int]
    L.rtr_capture_set_lookup_one.argtypes = [P(A.CaptureSetC), vp, C.c_int32, vp, vp, vp]
    L.rtr_shade_ibl_set.argtypes = [vp, P(A.ShadeEnvC), P(A.CaptureSetC), vp, vp, C.c_int64]
    L.rtr_shade_ibl_set_device.argtypes = [vp, P(A.ShadeEnvC), P(A.CaptureSetC), vp, vp, C.c_int64, C.c_int]
    L.rtr_shade_ibl_set_one.argtypes = [P(A.ShadeEnvC), P(A.CaptureSetC), vp, vp]
    L.rtr_preview_set.argtypes = [vp, P(A.PreviewParamsC), P(A.ShadeEnvC), P(A.CaptureSetC), vp, C.c_int64, vp]
    L.rtr_preview_set_device.argtypes = [vp, P(A.PreviewParamsC), P(A.ShadeEnvC), P(A.CaptureSetC), vp, C.c_int64, vp, C.c_int]
    if L.rtr_abi_version() != A.RTR_ABI_VERSION:
        raise RtrError(A.RTR_ERR_INVALID, "librtr_hip.so ABI version mismatch")
    _LIB = L
    return L


def test_lib():
    """librtr_hip_test.so (include/rtr_hip_test.h): the device unit kernels the parity tests and tools/ drive.  Loaded on
    first use; never needed to render."""
    global _TEST_LIB
    if _TEST_LIB is not None:
        return _TEST_LIB
    lib()  # the product library first: the test library links against it
    path = os.environ.get("RTR_HIP_TEST_LIBRARY") or os.path.join(os.path.dirname(library_path()), "librtr_hip_test.so")
    if not os.path.exists(path):
        path = os.path.join(_HERE, "librtr_hip_test.so")
    if not os.path.exists(path):
        raise RtrError(A.RTR_ERR_DEVICE, "test library %s is missing: run __graft_entry__.build()" % path)
    T = C.CDLL(path, mode=C.RTLD_GLOBAL)
    vp = C.c_void_p
    for name in ("rtr_test_hits", "rtr_test_materials", "rtr_test_lights", "rtr_test_scatter"):
        getattr(T, name).argtypes = [vp, vp, C.c_int64]
    for name in ("rtr_test_materials_ms", "rtr_test_scatter_ms", "rtr_test_lights_ms"):
        getattr(T, name).argtypes = [vp, vp, C.c_int64, C.c_int32]
    T.rtr_test_pow5.argtypes = [vp, vp, vp, C.c_int64]
    T.rtr_test_pow5_host.argtypes = [vp, vp, C.c_int64]
    T.rtr_test_li.argtypes = [vp, C.POINTER(A.RenderParamsC), vp, C.c_int64]
    T.rtr_test_reference_order.argtypes = [vp, C.c_int]
    T.rtr_test_stream8.argtypes = [vp, C.c_int64, C.c_int]
    T.rtr_test_sincos_exhaustive.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    T.rtr_test_issue_rates.argtypes = [vp, C.POINTER(C.c_double), C.c_int]
    T.rtr_test_shared_division.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    T.rtr_test_last_kernel.argtypes = [vp, C.POINTER(KernelRecordC), C.c_size_t]
    T.rtr_test_last_gather.argtypes = [vp, C.POINTER(GatherRecordC), C.c_size_t]
    T.rtr_test_last_probe.argtypes = [vp, C.POINTER(ProbeRecordC), C.c_size_t]
    T.rtr_test_last_capture.argtypes = [vp, C.POINTER(CaptureRecordC), C.c_size_t]
    T.rtr_test_last_probe_depth.argtypes = [vp, C.POINTER(ProbeDepthRecordC), C.c_size_t]
    T.rtr_test_temporal_planes.argtypes = [vp] + [C.c_int32] * 6 + [C.POINTER(A.CameraC), C.POINTER(A.CameraC), C.c_int,
                                                                    C.POINTER(A.TemporalParamsC)] + [vp] * 8
    T.rtr_test_scene_plan.argtypes = [C.POINTER(A.SceneDescC), C.c_int32, C.c_int32, C.POINTER(ScenePlanC), vp, C.c_int64,
                                      vp, C.c_int64]
    T.rtr_test_flat_hits.argtypes = [vp, vp, C.c_int64, C.c_int, C.POINTER(C.c_int32)]
    T.rtr_test_pair_frames.argtypes = [C.POINTER(A.SceneDescC), vp, C.c_int64, C.POINTER(C.c_int32)]
    T.rtr_test_pair_frame_host.argtypes = [C.c_int32, vp, vp, C.c_int64]
    T.rtr_test_pair_cast.argtypes = [vp, vp, C.c_int64]
    T.rtr_test_pair_cast_text.argtypes = [vp, vp, C.c_int64, C.c_int32]
    T.rtr_test_pair_resident.argtypes = [vp, vp, C.c_int64, C.c_int32]
    T.rtr_test_queue_blocks_host.argtypes = [C.c_int32] * 6 + [vp, C.c_int64]
    T.rtr_test_queue_pack_host.argtypes = [C.c_int32] * 3 + [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), vp]
    T.rtr_test_udiv.argtypes = [vp, vp, C.c_int64, vp, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    T.rtr_test_scene_consts.argtypes = [vp, vp, vp, C.c_int64, C.POINTER(C.c_int32)]
    for name in ("rtr_test_rcp_lane", "rtr_test_sqrt_lane"):
        getattr(T, name).argtypes = [vp] + [C.POINTER(C.c_uint64)] * 3 + [vp]
    T.rtr_test_lane_specials.argtypes = [vp, C.c_int64]
    T.rtr_test_lane_host.argtypes = [C.c_int32, C.c_int32, vp, vp, vp, C.c_int64]
    T.rtr_test_draw_forms.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 3
    T.rtr_test_draw_callers.argtypes = [vp, C.c_uint64, C.c_int64] + [C.POINTER(C.c_uint64)] * 3
    T.rtr_test_draw_host.argtypes = [vp, vp, C.c_int64]
    T.rtr_test_draw_host_range.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    T.rtr_test_accum_load.argtypes = [vp, vp, vp, vp, vp, C.c_int64]
    T.rtr_test_accum_plan.argtypes = [vp, C.c_int64] + [C.c_int32] * 4 + [C.c_double, vp, vp, vp, vp, C.POINTER(C.c_int32)]
    T.rtr_test_accum_commit.argtypes = [vp, C.c_int64, vp, C.c_int32] + [vp] * 7
    _TEST_LIB = T
    return T


def validate_scene(scene):
    """Host-only scene check (no GPU needed).  Returns the scene facts; raises RtrError."""
    L = lib()
    d = scene.desc()
    info = SceneInfoC()
    msg = C.create_string_buffer(256)
    rc = L.rtr_validate_scene(C.byref(d), C.byref(info), msg, len(msg))
    if rc != 0:
        raise RtrError(rc, msg.value.decode())
    return {"stack_words": info.stack_words, "has_media": bool(info.has_media), "needs_uv": bool(info.needs_uv),
            "graph_depth": info.graph_depth, "fast_ok": bool(info.fast_ok), "fast_instances": info.fast_instances,
            "fast_refs": info.fast_refs, "fast_stack_words": info.fast_stack_words,
            "compiled_subtrees": info.compiled_subtrees, "program_steps": info.program_steps,
            "inverted_boxes": info.inverted_boxes, "top_trees": info.top_trees}


def scene_plan(scene, integrator=4, flags=0):
    """rtr_test_scene_plan (include/rtr_hip_test.h; no GPU needed): what lowering finds out about ``scene`` and the kernel
    a megakernel render with ``integrator`` and ``flags`` would run, as a dict of the rtr_scene_plan members plus
    ``ref_flags``, the ``reserved`` word of every reference record (int32 array), and ``finish``, the finish records
    (``FINISH_DTYPE`` array, one per reference; empty for a scene that gets none).  Raises RtrError for a rejected scene."""
    T = test_lib()
    d = scene.desc()
    plan = ScenePlanC()
    rc = T.rtr_test_scene_plan(C.byref(d), int(integrator), int(flags), C.byref(plan), None, 0, None, 0)
    if rc != 0:
        raise RtrError(rc, "scene rejected")
    ref_flags = np.zeros(plan.n_refs, dtype=np.int32)
    finish = np.zeros(plan.n_finish, dtype=FINISH_DTYPE)
    T.rtr_test_scene_plan(C.byref(d), int(integrator), int(flags), C.byref(plan), ref_flags.ctypes.data, len(ref_flags),
                          finish.ctypes.data, len(finish))
    out = {name: int(getattr(plan, name)) for name, _ in ScenePlanC._fields_}
    out["ref_flags"] = ref_flags
    out["finish"] = finish
    return out


def pair_frames(scene):
    """rtr_test_pair_frames (include/rtr_hip_test.h; no GPU needed): the frame shape of every instance of ``scene``'s
    sub-scene 0 as a list of ``FRAME_SHAPES`` names.  Raises RtrError for a rejected scene."""
    T = test_lib()
    d = scene.desc()
    n = C.c_int32(0)
    rc = T.rtr_test_pair_frames(C.byref(d), None, 0, C.byref(n))
    if rc != 0:
        raise RtrError(rc, "scene rejected")
    shapes = np.zeros(n.value, dtype=np.int32)
    T.rtr_test_pair_frames(C.byref(d), shapes.ctypes.data, len(shapes), C.byref(n))
    return [FRAME_SHAPES[k] for k in shapes]


def pair_frame_host(shape, ops, ao, ad, bo, bd):
    """rtr_test_pair_frame_host (include/rtr_hip_test.h; no GPU needed): the host build of the pair cast's frame block for
    a frame of ``shape`` (a ``FRAME_SHAPES`` name but "other") with operands ``ops`` ((2, 3): outer, inner) on n ray pairs
    given as (n, 3) arrays.  Returns the ``PAIR_FRAME_DTYPE`` records."""
    recs = np.zeros(len(ao), dtype=PAIR_FRAME_DTYPE)
    recs["ao"], recs["ad"], recs["bo"], recs["bd"] = ao, ad, bo, bd
    ops = np.ascontiguousarray(ops, dtype=np.float64).reshape(6)
    rc = test_lib().rtr_test_pair_frame_host(FRAME_SHAPES.index(shape), ops.ctypes.data, recs.ctypes.data, len(recs))
    if rc != 0:
        raise RtrError(rc, "rtr_test_pair_frame_host")
    return recs


def pow5_host(x):
    """rtr_test_pow5_host (include/rtr_hip_test.h; no GPU needed): the host build of the device's pow5 over an array."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    rc = test_lib().rtr_test_pow5_host(x.ctypes.data, out.ctypes.data, x.size)
    if rc != 0:
        raise RtrError(rc, "rtr_test_pow5_host")
    return out


def lane_specials():
    """rtr_test_lane_specials (include/rtr_hip_test.h; no GPU needed): the edge values of the lane-division kernels, float64."""
    n = test_lib().rtr_test_lane_specials(None, 0)
    out = np.zeros(n, dtype=np.uint64)
    test_lib().rtr_test_lane_specials(out.ctypes.data, n)
    return out.view(np.float64)


LANE_OPS = ("rcp", "sqrt")


def lane_host(op, a, coarse_bits=0):
    """rtr_test_lane_host (include/rtr_hip_test.h; no GPU needed): 1.0 / a (``op`` "rcp") or sqrt(a) ("sqrt") through the
    host build of the short forms, element by element, the seeds' low ``coarse_bits`` bits cleared.  Returns (results,
    took_short)."""
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    out, took = np.zeros_like(a), np.zeros(a.size, dtype=np.int32)
    rc = test_lib().rtr_test_lane_host(LANE_OPS.index(op), int(coarse_bits), a.ctypes.data, out.ctypes.data, took.ctypes.data, a.size)
    if rc != 0:
        raise RtrError(rc, "rtr_test_lane_host")
    return out, took.astype(bool)


def draw_host(s):
    """rtr_test_draw_host (include/rtr_hip_test.h; no GPU needed): the host build of the joined form of a draw in (-1, 1)
    over the states ``s`` (uint32): -1 + s * 2^-31, float64."""
    s = np.ascontiguousarray(s, dtype=np.uint32).ravel()
    out = np.zeros(s.size, dtype=np.float64)
    rc = test_lib().rtr_test_draw_host(s.ctypes.data, out.ctypes.data, s.size)
    if rc != 0:
        raise RtrError(rc, "rtr_test_draw_host")
    return out


def draw_host_range(first, count, stride=1, threads=1):
    """rtr_test_draw_host_range (include/rtr_hip_test.h; no GPU needed): the joined form beside the plain text on the
    states first, first + stride, ... (``count`` of them), over ``threads`` threads.  Returns (mismatches, tested)."""
    bad, tested = C.c_uint64(0), C.c_uint64(0)
    rc = test_lib().rtr_test_draw_host_range(int(first), int(count), int(stride), int(threads), C.byref(bad), C.byref(tested))
    if rc != 0:
        raise RtrError(rc, "rtr_test_draw_host_range")
    return bad.value, tested.value


def queue_blocks_host(n_tiles, spp, chunks, guided=(0, 0, 0)):
    """rtr_test_queue_blocks_host (include/rtr_hip_test.h; no GPU needed): the host build of the job queue's block decode
    for every block of a launch over ``n_tiles`` tiles, ``chunks`` partial sums of ``spp`` samples, ``guided`` = (n_big,
    big_spp, small_spp) of a guided split.  Returns the ``QUEUE_BLOCK_DTYPE`` records, one per block id."""
    recs = np.zeros(n_tiles * chunks * 4, dtype=QUEUE_BLOCK_DTYPE)
    rc = test_lib().rtr_test_queue_blocks_host(n_tiles, spp, chunks, *[int(g) for g in guided], recs.ctypes.data, len(recs))
    if rc != 0:
        raise RtrError(rc, "rtr_test_queue_blocks_host")
    return recs


def queue_pack_host(i, j, s_end):
    """rtr_test_queue_pack_host: (lo, hi) halves of the parked word for pixel (i, j) and ``s_end``, and what unpacking
    them gives back, as ((lo, hi), (i, j, s_end))."""
    lo, hi = C.c_uint32(0), C.c_uint32(0)
    out = np.zeros(3, dtype=np.int32)
    rc = test_lib().rtr_test_queue_pack_host(int(i), int(j), int(s_end), C.byref(lo), C.byref(hi), out.ctypes.data)
    if rc != 0:
        raise RtrError(rc, "rtr_test_queue_pack_host")
    return (lo.value, hi.value), tuple(int(v) for v in out)


def _defaults(struct, c_function, allowed_fields, overrides):
    """A ``struct`` filled by the library's ``c_function`` (rtr_*_defaults), then the ``allowed_fields`` that ``overrides``
    names replaced; TypeError for any other name.  The subject in the message is the middle of the function's name."""
    p = struct()
    getattr(lib(), c_function)(C.byref(p))
    for k, v in overrides.items():
        if k not in allowed_fields:
            raise TypeError("no %s parameter %r" % (c_function.split("_")[1], k))
        setattr(p, k, v)
    return p


def denoise_defaults(**overrides):
    """rtr_denoise_params with the library's defaults (rtr_denoise_defaults), fields replaced by ``overrides``."""
    return _defaults(A.DenoiseParamsC, "rtr_denoise_defaults",
                     ("iterations", "feature_spp", "sigma_l", "sigma_n", "sigma_a", "sigma_z"), overrides)


def temporal_defaults(**overrides):
    """rtr_temporal_params with the library's defaults (rtr_temporal_defaults), fields replaced by ``overrides``."""
    return _defaults(A.TemporalParamsC, "rtr_temporal_defaults", ("alpha_min", "tau_z", "tau_n", "min_weight"), overrides)


def display_defaults(**overrides):
    """rtr_display_params with the library's defaults (rtr_display_defaults), fields replaced by ``overrides``."""
    return _defaults(A.DisplayParamsC, "rtr_display_defaults",
                     ("auto_exposure", "meter_permille", "tone_curve", "encoding", "exposure", "key", "white"), overrides)


def gather_defaults(**overrides):
    """rtr_gather_params with the library's defaults (rtr_gather_defaults: samples 64, seed 0, point_base 0, flags 0, time 0,
    t_min 0.001, t_max inf), fields replaced by ``overrides``; ``reference_order=True`` sets RTR_FLAG_REFERENCE_ORDER."""
    if overrides.pop("reference_order", False):
        overrides.setdefault("flags", A.FLAG_REFERENCE_ORDER)  # onto the default flags, 0; an explicit flags= replaces them
    return _defaults(A.GatherParamsC, "rtr_gather_defaults", ("samples", "seed", "point_base", "flags", "time", "t_min", "t_max"),
                     overrides)


def gather_points(points, normals):
    """A ``GATHER_POINT_DTYPE`` array from (n, 3) positions and normals (or ``points`` already such an array)."""
    if isinstance(points, np.ndarray) and points.dtype == A.GATHER_POINT_DTYPE:
        return np.ascontiguousarray(points)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    pts = np.zeros(len(p), dtype=A.GATHER_POINT_DTYPE)
    pts["p"], pts["n"] = p, np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    return pts


def gather_rays(points, normals=None, params=None, **overrides):
    """rtr_gather_ray for every sample of every point (host only, no context): the ``RAY_DTYPE`` rays [n, samples] the
    gathers cast, with the generator state after the direction's draws.  Raises RtrError for a bad point or bad params."""
    return _ray_table("rtr_gather_ray", gather_points(points, normals), params, overrides)


def _ray_table(c_function, pts, params, overrides):
    """``c_function`` (rtr_gather_ray / rtr_probe_ray) for every sample of every record of ``pts``: ``RAY_DTYPE`` [n, samples]"""
    ray_of = getattr(lib(), c_function)
    gp = params if params is not None else gather_defaults(**overrides)
    n_s = int(gp.samples)
    if not 1 <= n_s <= A.GATHER_MAX_SAMPLES:
        raise RtrError(A.RTR_ERR_INVALID, "%s: samples outside 1 .. 2^20" % c_function)
    rays = np.zeros((len(pts), n_s), dtype=A.RAY_DTYPE)
    base, stride, size = pts.ctypes.data, pts.dtype.itemsize, A.RAY_DTYPE.itemsize
    for k in range(len(pts)):
        for s in range(n_s):
            rc = ray_of(C.byref(gp), base + k * stride, k, s, rays.ctypes.data + (k * n_s + s) * size)
            if rc != 0:
                raise RtrError(rc, "%s: bad params or bad point at index %d" % (c_function, k))
    return rays


def probe_points(points):
    """A ``PROBE_POINT_DTYPE`` array from (n, 3) positions (or ``points`` already such an array)."""
    if isinstance(points, np.ndarray) and points.dtype == A.PROBE_POINT_DTYPE:
        return np.ascontiguousarray(points)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    pts = np.zeros(len(p), dtype=A.PROBE_POINT_DTYPE)
    pts["p"] = p
    return pts


def probe_rays(points, params=None, **overrides):
    """rtr_probe_ray for every sample of every probe (host only, no context): the ``RAY_DTYPE`` rays [n, samples] the probe
    kernels cast, uniform over the sphere, with the generator state after the direction's draws."""
    return _ray_table("rtr_probe_ray", probe_points(points), params, overrides)


def sh_basis(directions):
    """rtr_sh_basis: the nine basis functions [..., 9] at the directions [..., 3] (taken as given: pass unit vectors)."""
    d = np.ascontiguousarray(directions, dtype=np.float64)
    flat = d.reshape(-1, 3)
    y = np.zeros((len(flat), 9))
    L = lib()
    for k in range(len(flat)):
        L.rtr_sh_basis(flat.ctypes.data + 24 * k, y.ctypes.data + 72 * k)
    return y.reshape(d.shape[:-1] + (9,))


def sh_irradiance(c, normals):
    """rtr_sh_irradiance: irradiance [..., 3] of the normals [..., 3] under the coefficients ``c`` ([9, 3], the ``c`` of a
    ``PROBE_SH_DTYPE`` record).  Raises RtrError for a bad normal."""
    c = np.ascontiguousarray(c, dtype=np.float64)
    if c.shape != (9, 3):
        raise ValueError("c must be [9, 3]")
    n = np.ascontiguousarray(normals, dtype=np.float64)
    flat = n.reshape(-1, 3)
    E = np.zeros((len(flat), 3))
    L = lib()
    for k in range(len(flat)):
        rc = L.rtr_sh_irradiance(c.ctypes.data, flat.ctypes.data + 24 * k, E.ctypes.data + 24 * k)
        if rc != 0:
            raise RtrError(rc, "rtr_sh_irradiance: bad normal at index %d" % k)
    return E.reshape(n.shape)


def probe_grid(origin, spacing, dims):
    """An rtr_probe_grid: probe (ix, iy, iz) stands at origin + (ix, iy, iz) * spacing, index ix + dims[0] * (iy + dims[1] * iz)."""
    g = A.ProbeGridC()
    for a in range(3):
        g.origin[a], g.spacing[a], g.dims[a] = float(origin[a]), float(spacing[a]), int(dims[a])
    return g


def probe_lookup_host(grid, probes, points, normals=None):
    """rtr_probe_lookup_one for every query (host only, no context): a ``GATHER_OUT_DTYPE`` array.  Raises RtrError for a bad
    grid or a bad query."""
    L = lib()
    probes = np.ascontiguousarray(probes, dtype=A.PROBE_SH_DTYPE)
    if len(probes) != grid.dims[0] * grid.dims[1] * grid.dims[2]:
        raise ValueError("probes must hold dims[0] * dims[1] * dims[2] records")
    q = gather_points(points, normals)
    out = np.zeros(len(q), dtype=A.GATHER_OUT_DTYPE)
    for k in range(len(q)):
        rc = L.rtr_probe_lookup_one(C.byref(grid), probes.ctypes.data, q.ctypes.data + 48 * k, out.ctypes.data + 32 * k)
        if rc != 0:
            raise RtrError(rc, "rtr_probe_lookup_one: bad grid, or bad query at index %d" % k)
    return out


def probe_depth_defaults(**overrides):
    """rtr_probe_depth_params with the library's defaults (rtr_probe_depth_defaults: map_size 16, samples 8, seed 0,
    point_base 0, jitter 1, time 0, t_min 0.001), fields replaced by ``overrides``.  ``t_max`` has no default: a block
    without it is rejected by every entry."""
    return _defaults(A.ProbeDepthParamsC, "rtr_probe_depth_defaults",
                     ("map_size", "samples", "seed", "point_base", "jitter", "time", "t_min", "t_max"), overrides)


def probe_depth_rays(points, params=None, **overrides):
    """rtr_probe_depth_ray for every sample of every texel of every probe (host only, no context): ``RAY_DTYPE``
    [n, T, T, samples] (row b, then column a), the rays rtr_probe_depth casts."""
    dp = params if params is not None else probe_depth_defaults(**overrides)
    pts = probe_points(points)
    T, N = int(dp.map_size), int(dp.samples)
    if not (1 <= T <= A.PROBE_DEPTH_MAX_MAP and 1 <= N <= A.GATHER_MAX_SAMPLES):
        raise RtrError(A.RTR_ERR_INVALID, "rtr_probe_depth_ray: map_size or samples out of range")
    rays = np.zeros((len(pts), T, T, N), dtype=A.RAY_DTYPE)
    ray_of, size, flat = lib().rtr_probe_depth_ray, A.RAY_DTYPE.itemsize, 0
    for k in range(len(pts)):
        for b in range(T):
            for a in range(T):
                for s in range(N):
                    rc = ray_of(C.byref(dp), pts.ctypes.data + 24 * k, k, a, b, s, rays.ctypes.data + flat * size)
                    if rc != 0:
                        raise RtrError(rc, "rtr_probe_depth_ray: bad params or bad probe at index %d" % k)
                    flat += 1
    return rays


def octa_encode(directions):
    """rtr_octa_encode: the points [..., 2] of the octahedral square of the directions [..., 3] (need not be unit)."""
    d = np.ascontiguousarray(directions, dtype=np.float64)
    flat = d.reshape(-1, 3)
    uv = np.zeros((len(flat), 2))
    L = lib()
    for k in range(len(flat)):
        L.rtr_octa_encode(flat.ctypes.data + 24 * k, uv.ctypes.data + 16 * k)
    return uv.reshape(d.shape[:-1] + (2,))


def octa_decode(uv):
    """rtr_octa_decode: the unit directions [..., 3] of the points [..., 2] of the octahedral square."""
    uv = np.ascontiguousarray(uv, dtype=np.float64)
    flat = uv.reshape(-1, 2)
    d = np.zeros((len(flat), 3))
    L = lib()
    for k in range(len(flat)):
        L.rtr_octa_decode(flat.ctypes.data + 16 * k, d.ctypes.data + 24 * k)
    return d.reshape(uv.shape[:-1] + (3,))


def probe_visible_params(map_size, normal_bias=0.0):
    """An rtr_probe_visible_params"""
    vp = A.ProbeVisibleParamsC()
    vp.map_size, vp.normal_bias = int(map_size), float(normal_bias)
    return vp


def _visible_inputs(grid, probes, depth, map_size):
    """(SH records, depth records [probes * T * T], T) of a visible lookup; ``depth`` may be [probes, T, T]"""
    probes = np.ascontiguousarray(probes, dtype=A.PROBE_SH_DTYPE)
    n = grid.dims[0] * grid.dims[1] * grid.dims[2]
    if len(probes) != n:
        raise ValueError("probes must hold dims[0] * dims[1] * dims[2] records")
    depth = np.ascontiguousarray(depth, dtype=A.PROBE_DEPTH_DTYPE)
    T = int(map_size) if map_size is not None else (depth.shape[-1] if depth.ndim == 3 else int(round((depth.size / max(n, 1)) ** 0.5)))
    if depth.size != n * T * T:
        raise ValueError("depth must hold T * T records per probe")
    return probes, depth.reshape(-1), T


def probe_lookup_visible_host(grid, probes, depth, points, normals=None, normal_bias=0.0, map_size=None, params=None):
    """rtr_probe_lookup_visible_one for every query (host only, no context): a ``GATHER_OUT_DTYPE`` array.  Raises RtrError
    for a bad grid, bad params or a bad query."""
    L = lib()
    probes, depth, T = _visible_inputs(grid, probes, depth, map_size if params is None else params.map_size)
    vp = params if params is not None else probe_visible_params(T, normal_bias)
    q = gather_points(points, normals)
    out = np.zeros(len(q), dtype=A.GATHER_OUT_DTYPE)
    for k in range(len(q)):
        rc = L.rtr_probe_lookup_visible_one(C.byref(grid), probes.ctypes.data, depth.ctypes.data, C.byref(vp),
                                            q.ctypes.data + 48 * k, out.ctypes.data + 32 * k)
        if rc != 0:
            raise RtrError(rc, "rtr_probe_lookup_visible_one: bad grid or params, or bad query at index %d" % k)
    return out


def capture_defaults(**overrides):
    """rtr_capture_params with the library's defaults (rtr_capture_defaults: face_size 32, samples 16, seed 0, point_base 0,
    jitter 1, time 0), fields replaced by ``overrides``."""
    return _defaults(A.CaptureParamsC, "rtr_capture_defaults", ("face_size", "samples", "seed", "point_base", "jitter", "time"),
                     overrides)


def capture_ray(point, face, a, b, s=0, index_in_call=0, params=None, **overrides):
    """rtr_capture_ray (host only, no context): ray ``s`` through texel (``a``, ``b``) of face ``face`` of the centre
    ``point`` ([3]) at ``index_in_call``, as a one-element ``RAY_DTYPE`` array with the generator state after the jitter's
    draws.  Raises RtrError for a bad centre, bad params or an index outside the capture."""
    cp = params if params is not None else capture_defaults(**overrides)
    pt = probe_points(np.asarray(point, dtype=np.float64).reshape(1, 3))
    ray = np.zeros(1, dtype=A.RAY_DTYPE)
    rc = lib().rtr_capture_ray(C.byref(cp), pt.ctypes.data, int(index_in_call), int(face), int(a), int(b), int(s), ray.ctypes.data)
    if rc != 0:
        raise RtrError(rc, "rtr_capture_ray: bad params, bad centre or an index outside the capture")
    return ray


def capture_rays(points, params=None, **overrides):
    """rtr_capture_ray for every sample of every texel of every centre: ``RAY_DTYPE`` [n, 6, S, S, samples] (row b, then
    column a), the rays rtr_capture_cube casts."""
    cp = params if params is not None else capture_defaults(**overrides)
    pts = probe_points(points)
    S, N = int(cp.face_size), int(cp.samples)
    if not (1 <= S <= A.CAPTURE_MAX_FACE and 1 <= N <= A.GATHER_MAX_SAMPLES):
        raise RtrError(A.RTR_ERR_INVALID, "rtr_capture_ray: face_size or samples out of range")
    rays = np.zeros((len(pts), 6, S, S, N), dtype=A.RAY_DTYPE)
    ray_of, size, flat = lib().rtr_capture_ray, A.RAY_DTYPE.itemsize, 0
    for k in range(len(pts)):
        for f in range(6):
            for b in range(S):
                for a in range(S):
                    for s in range(N):
                        rc = ray_of(C.byref(cp), pts.ctypes.data + 24 * k, k, f, a, b, s, rays.ctypes.data + flat * size)
                        if rc != 0:
                            raise RtrError(rc, "rtr_capture_ray: bad params or bad centre at index %d" % k)
                        flat += 1
    return rays


def _cube_texels(texels, face_size=None):
    """(face size, the 6 S^2 ``GATHER_OUT_DTYPE`` records) of one capture given as records or as a [6, S, S] array of them"""
    t = np.ascontiguousarray(texels, dtype=A.GATHER_OUT_DTYPE)
    S = int(face_size) if face_size is not None else (t.shape[-1] if t.ndim == 3 else int(round((t.size / 6) ** 0.5)))
    if not 1 <= S <= A.CAPTURE_MAX_FACE or t.size != 6 * S * S:
        raise ValueError("a capture holds 6 * S * S records, 1 <= S <= %d" % A.CAPTURE_MAX_FACE)
    return S, t.reshape(-1)


def cube_lookup_host(texels, directions, face_size=None):
    """rtr_cube_lookup_one for every direction ([n, 3]; host only, no context): a ``GATHER_OUT_DTYPE`` array."""
    S, t = _cube_texels(texels, face_size)
    q = probe_points(directions)
    out = np.zeros(len(q), dtype=A.GATHER_OUT_DTYPE)
    L = lib()
    for k in range(len(q)):
        rc = L.rtr_cube_lookup_one(S, t.ctypes.data, q.ctypes.data + 24 * k, out.ctypes.data + 32 * k)
        if rc != 0:
            raise RtrError(rc, "rtr_cube_lookup_one")
    return out


def latlong_direction(width, height, i, j):
    """rtr_latlong_direction: the direction [3] of the centre of texel (i, j) of a width x height equirectangular map."""
    d = np.zeros(3)
    rc = lib().rtr_latlong_direction(int(width), int(height), int(i), int(j), d.ctypes.data)
    if rc != 0:
        raise RtrError(rc, "rtr_latlong_direction: bad size or texel outside the map")
    return d


def cube_to_latlong(texels, width, height, face_size=None):
    """rtr_cube_to_latlong: the capture resampled to an equirectangular image [height, width, 3], row 0 the top."""
    S, t = _cube_texels(texels, face_size)
    out = np.zeros((int(height), int(width), 3))
    rc = lib().rtr_cube_to_latlong(S, t.ctypes.data, int(width), int(height), out.ctypes.data)
    if rc != 0:
        raise RtrError(rc, "rtr_cube_to_latlong: bad size")
    return out


def write_rgbe(path, rgb):
    """rtr_write_rgbe: the image ``rgb`` [H, W, 3] (row 0 the top) as a flat-scanline Radiance .hdr file at ``path``."""
    a = np.ascontiguousarray(rgb, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("an (H, W, 3) image expected")
    rc = lib().rtr_write_rgbe(os.fsencode(path), a.shape[1], a.shape[0], a.ctypes.data)
    if rc != 0:
        raise RtrError(rc, "rtr_write_rgbe: bad size, or %s cannot be written" % path)


def cube_filter_defaults(**overrides):
    """rtr_cube_filter_params with the library's defaults (rtr_cube_filter_defaults: face_in 32, face_out 16, alpha 0.25,
    cos_cut 0), fields replaced by ``overrides``."""
    return _defaults(A.CubeFilterParamsC, "rtr_cube_filter_defaults", ("face_in", "face_out", "alpha", "cos_cut"), overrides)


def _filter_cubes(texels, fp):
    """The source records of a filter call as a flat array, and how many cubes of 6 * face_in^2 they are"""
    t = np.ascontiguousarray(texels, dtype=A.GATHER_OUT_DTYPE).reshape(-1)
    per = 6 * int(fp.face_in) ** 2
    if per <= 0 or t.size % per:
        raise ValueError("the source holds whole cubes of 6 * face_in^2 records")
    return t, t.size // per


def cube_filter_host(texels, params=None, **overrides):
    """rtr_cube_filter_one for every output texel of every cube (host only, no context; a loop for tests): the
    ``GATHER_OUT_DTYPE`` records [n_cubes, 6, face_out, face_out] of the source ``texels`` ([n_cubes, 6, face_in, face_in]
    or flat)."""
    fp = params if params is not None else cube_filter_defaults(**overrides)
    L = lib()
    So = int(fp.face_out)
    if not 1 <= So <= A.CUBE_FILTER_MAX_FACE or not 1 <= int(fp.face_in) <= A.CUBE_FILTER_MAX_FACE:
        raise RtrError(A.RTR_ERR_INVALID, "rtr_cube_filter_one: face_in or face_out outside 1 .. 512")
    t, n = _filter_cubes(texels, fp)
    out = np.zeros((n, 6, So, So), dtype=A.GATHER_OUT_DTYPE)
    per_in, flat = 6 * int(fp.face_in) ** 2 * 32, 0
    for k in range(n):
        for f in range(6):
            for b in range(So):
                for a in range(So):
                    rc = L.rtr_cube_filter_one(C.byref(fp), t.ctypes.data + k * per_in, f, a, b, out.ctypes.data + 32 * flat)
                    if rc != 0:
                        raise RtrError(rc, "rtr_cube_filter_one: bad params")
                    flat += 1
    return out


def cube_chain_plan(face_size, n_levels):
    """rtr_cube_chain_plan: (levels, n_records) -- a ctypes array of ``n_levels`` rtr_cube_level for a capture of
    ``face_size`` and the records all levels hold."""
    levels = (A.CubeLevelC * max(int(n_levels), 1))()
    n = C.c_int64()
    rc = lib().rtr_cube_chain_plan(int(face_size), int(n_levels), C.byref(levels), C.byref(n))
    if rc != 0:
        raise RtrError(rc, "rtr_cube_chain_plan: face_size outside 1 .. 4096 or n_levels outside 1 .. 13")
    return levels, int(n.value)


def cube_levels(levels):
    """A ctypes array of rtr_cube_level from ``levels``: such an array, or (face_size, offset, alpha) triples"""
    if isinstance(levels, C.Array) and levels._type_ is A.CubeLevelC:
        return levels
    arr = (A.CubeLevelC * max(len(levels), 1))()
    for i, (s, o, a) in enumerate(levels):
        arr[i] = A.CubeLevelC(int(s), 0, int(o), float(a))
    return arr


def cube_queries(directions, alpha):
    """A ``CUBE_QUERY_DTYPE`` array from (n, 3) directions and alphas (a number or [n])"""
    d = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    q = np.zeros(len(d), dtype=A.CUBE_QUERY_DTYPE)
    q["d"], q["alpha"] = d, alpha
    return q


def cube_chain_lookup_host(levels, texels, queries, n_levels=None):
    """rtr_cube_chain_lookup_one for every query (``CUBE_QUERY_DTYPE``; host only, no context): a ``GATHER_OUT_DTYPE`` array."""
    lv = cube_levels(levels)
    n_levels = len(levels) if n_levels is None else int(n_levels)
    t = np.ascontiguousarray(texels, dtype=A.GATHER_OUT_DTYPE).reshape(-1)
    q = np.ascontiguousarray(queries, dtype=A.CUBE_QUERY_DTYPE)
    out = np.zeros(len(q), dtype=A.GATHER_OUT_DTYPE)
    L = lib()
    for k in range(len(q)):
        rc = L.rtr_cube_chain_lookup_one(C.byref(lv), n_levels, t.ctypes.data, q.ctypes.data + 32 * k, out.ctypes.data + 32 * k)
        if rc != 0:
            raise RtrError(rc, "rtr_cube_chain_lookup_one: bad chain")
    return out


def brdf_params(n_mu, n_rough, nodes=128):
    """An rtr_brdf_params"""
    bp = A.BrdfParamsC()
    bp.n_mu, bp.n_rough, bp.nodes = int(n_mu), int(n_rough), int(nodes)
    return bp


def brdf_table_host(n_mu, n_rough, nodes=128, params=None):
    """rtr_brdf_entry_one for every entry (host only, no context; a loop for tests): ``BRDF_ENTRY_DTYPE`` [n_rough, n_mu]."""
    bp = params if params is not None else brdf_params(n_mu, n_rough, nodes)
    if not (1 <= bp.n_mu <= A.BRDF_MAX and 1 <= bp.n_rough <= A.BRDF_MAX):
        raise RtrError(A.RTR_ERR_INVALID, "rtr_brdf_entry_one: n_mu or n_rough outside 1 .. 256")
    out = np.zeros((bp.n_rough, bp.n_mu), dtype=A.BRDF_ENTRY_DTYPE)
    L = lib()
    for r in range(bp.n_rough):
        for c in range(bp.n_mu):
            rc = L.rtr_brdf_entry_one(C.byref(bp), r, c, out.ctypes.data + 16 * (r * bp.n_mu + c))
            if rc != 0:
                raise RtrError(rc, "rtr_brdf_entry_one: bad params")
    return out


def brdf_fetch_one(table, mu, rough):
    """rtr_brdf_fetch_one: (a, b) of the bilinear fetch at (mu, rough) in ``table`` (``BRDF_ENTRY_DTYPE`` [n_rough, n_mu])."""
    t = np.ascontiguousarray(table, dtype=A.BRDF_ENTRY_DTYPE)
    if t.ndim != 2:
        raise ValueError("table must be [n_rough, n_mu]")
    out = np.zeros(1, dtype=A.BRDF_ENTRY_DTYPE)
    rc = lib().rtr_brdf_fetch_one(t.shape[1], t.shape[0], t.ctypes.data, float(mu), float(rough), out.ctypes.data)
    if rc != 0:
        raise RtrError(rc, "rtr_brdf_fetch_one: a table axis outside 1 .. 256 or a non-finite coordinate")
    return float(out["a"][0]), float(out["b"][0])


def shade_queries(points, normals, views, base, roughness, metallic):
    """A ``SHADE_QUERY_DTYPE`` array from (n, 3) points, normals, view vectors and base colours (or one colour) and
    roughness / metallic (numbers or [n])"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    q = np.zeros(len(p), dtype=A.SHADE_QUERY_DTYPE)
    q["p"], q["n"], q["v"], q["base"] = p, normals, views, base
    q["roughness"], q["metallic"] = roughness, metallic
    return q


def _address(x, dtype):
    """(address, object to keep alive, records) of an array member of a shade environment: a device pointer given as an
    int, or host records"""
    if x is None:
        return None, None, 0
    if isinstance(x, (int, np.integer)):
        return int(x), None, None
    a = np.ascontiguousarray(x, dtype=dtype)
    return a.ctypes.data, a, a.size


def shade_env(table, grid=None, probes=None, depth=None, visible=None, levels=None, chain=None, parts=None, n_records=None,
              n_mu=None, n_rough=None, n_levels=None):
    """An rtr_shade_env.  ``table``, ``probes``, ``depth`` and ``chain`` are host records (numpy; the table
    [n_rough, n_mu]) or device pointers (ints; then ``n_mu`` / ``n_rough`` / ``n_records`` say how many); ``grid`` an
    rtr_probe_grid, ``visible`` an rtr_probe_visible_params (with ``depth``) or None, ``levels`` what ``cube_levels``
    takes.  ``parts`` defaults to the parts whose arrays are given.  The struct keeps what it points to alive."""
    e = A.ShadeEnvC()
    keep = []
    if parts is None:
        parts = (A.SHADE_DIFFUSE if probes is not None else 0) | (A.SHADE_SPECULAR if chain is not None else 0)
    e.parts = int(parts)
    if not isinstance(table, (int, np.integer)) and table is not None:
        t = np.ascontiguousarray(table, dtype=A.BRDF_ENTRY_DTYPE)
        if t.ndim == 2:
            n_rough, n_mu = (t.shape[0] if n_rough is None else n_rough), (t.shape[1] if n_mu is None else n_mu)
        table = t
    e.table, k, _ = _address(table, A.BRDF_ENTRY_DTYPE)
    keep.append(k)
    e.n_mu, e.n_rough = int(n_mu or 0), int(n_rough or 0)
    if grid is not None:
        keep.append(grid)
        e.grid = C.addressof(grid)
    e.probes, k, _ = _address(probes, A.PROBE_SH_DTYPE)
    keep.append(k)
    e.depth, k, _ = _address(depth, A.PROBE_DEPTH_DTYPE)
    keep.append(k)
    if visible is not None:
        keep.append(visible)
        e.visible = C.addressof(visible)
    if levels is not None:
        lv = cube_levels(levels)
        keep.append(lv)
        e.levels, e.n_levels = C.addressof(lv), len(levels) if n_levels is None else int(n_levels)
    e.chain, k, records = _address(chain, A.GATHER_OUT_DTYPE)
    keep.append(k)
    e.n_records = int(n_records) if n_records is not None else int(records or 0)
    e._keep = keep
    return e


def shade_ibl_one(env, queries):
    """rtr_shade_ibl_one for every query (``SHADE_QUERY_DTYPE``; host only, no context) under a ``shade_env`` of host
    arrays: a ``GATHER_OUT_DTYPE`` array.  Raises RtrError for a bad environment or a bad query."""
    q = np.ascontiguousarray(queries, dtype=A.SHADE_QUERY_DTYPE).reshape(-1)
    out = np.zeros(len(q), dtype=A.GATHER_OUT_DTYPE)
    L = lib()
    for k in range(len(q)):
        rc = L.rtr_shade_ibl_one(C.byref(env), q.ctypes.data + 112 * k, out.ctypes.data + 32 * k)
        if rc != 0:
            raise RtrError(rc, "rtr_shade_ibl_one: bad environment, or bad query at index %d" % k)
    return out


def capture_set(volumes, fallback=-1):
    """An rtr_capture_set from ``CAPTURE_VOLUME_DTYPE`` records (or rows of sixteen numbers in struct order: centre,
    proxy_lo, proxy_hi, reach_lo, reach_hi, fade) and the capture read where none reaches (-1: none).  The struct keeps its
    volumes alive; ``.records`` is that array.  The rules are the library's: a bad set fails the call that takes it."""
    v = np.asarray(volumes)
    if v.dtype != A.CAPTURE_VOLUME_DTYPE:
        v = np.ascontiguousarray(np.asarray(volumes, dtype=np.float64).reshape(-1, 16)).view(A.CAPTURE_VOLUME_DTYPE)
    v = np.ascontiguousarray(v).reshape(-1).copy()
    s = A.CaptureSetC()
    s.n_captures, s.fallback, s.volumes = len(v), int(fallback), v.ctypes.data
    s.records = v
    return s


def capture_queries(points, directions, alpha):
    """A ``CAPTURE_QUERY_DTYPE`` array from (n, 3) points and directions and alphas (a number or [n])"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    q = np.zeros(len(p), dtype=A.CAPTURE_QUERY_DTYPE)
    q["p"], q["d"], q["alpha"] = p, directions, alpha
    return q


def capture_set_lookup_host(cset, levels, records, queries, n_levels=None):
    """rtr_capture_set_lookup_one for every query (``CAPTURE_QUERY_DTYPE``; host only, no context) over the level-major
    records of ``cset`` (``capture_set``); ``levels`` is the plan of one capture.  A ``GATHER_OUT_DTYPE`` array."""
    lv = cube_levels(levels)
    n_levels = len(levels) if n_levels is None else int(n_levels)
    t = np.ascontiguousarray(records, dtype=A.GATHER_OUT_DTYPE).reshape(-1)
    q = np.ascontiguousarray(queries, dtype=A.CAPTURE_QUERY_DTYPE).reshape(-1)
    out = np.zeros(len(q), dtype=A.GATHER_OUT_DTYPE)
    L = lib()
    for k in range(len(q)):
        rc = L.rtr_capture_set_lookup_one(C.byref(cset), C.byref(lv), n_levels, t.ctypes.data, q.ctypes.data + 64 * k,
                                          out.ctypes.data + 32 * k)
        if rc != 0:
            raise RtrError(rc, "rtr_capture_set_lookup_one: bad set or chain")
    return out


def shade_ibl_set_one(env, cset, queries):
    """rtr_shade_ibl_set_one for every query: ``shade_ibl_one`` with the specular record from the capture set ``cset``
    (``env.chain`` holds the set level-major; ``cset`` may be None without SPECULAR)."""
    q = np.ascontiguousarray(queries, dtype=A.SHADE_QUERY_DTYPE).reshape(-1)
    out = np.zeros(len(q), dtype=A.GATHER_OUT_DTYPE)
    L = lib()
    for k in range(len(q)):
        rc = L.rtr_shade_ibl_set_one(C.byref(env), _set_ref(cset), q.ctypes.data + 112 * k, out.ctypes.data + 32 * k)
        if rc != 0:
            raise RtrError(rc, "rtr_shade_ibl_set_one: bad environment or set, or bad query at index %d" % k)
    return out


def _set_ref(cset):
    return None if cset is None else C.byref(cset)


def preview_params(width, height, grid=1, region=None, t_min=None, reference_order=False):
    """An rtr_preview_params from rtr_preview_defaults: a ``width`` x ``height`` image, ``grid`` x ``grid`` rays per
    pixel, ``region`` (x0, y0, x1, y1) or the whole image"""
    p = A.PreviewParamsC()
    lib().rtr_preview_defaults(C.byref(p))
    x0, y0, x1, y1 = region if region is not None else (0, 0, width, height)
    p.image_width, p.image_height = int(width), int(height)
    p.x0, p.y0, p.x1, p.y1 = int(x0), int(y0), int(x1), int(y1)
    p.grid = int(grid)
    if t_min is not None:
        p.t_min = float(t_min)
    p.flags = A.FLAG_REFERENCE_ORDER if reference_order else 0
    return p


def preview_rays(camera, params):
    """The rays of a preview's region through rtr_preview_ray (host only, no context): ``RAY_DTYPE`` [h, w, grid^2] under
    ``camera`` (what ``camera_struct`` takes).  Raises RtrError for bad params."""
    cam = camera_struct(camera)
    h, w, kk = params.y1 - params.y0, params.x1 - params.x0, params.grid * params.grid
    rays = np.zeros((max(h, 0), max(w, 0), max(kk, 0)), dtype=A.RAY_DTYPE)
    L = lib()
    if rays.size == 0 and L.rtr_preview_ray(C.byref(cam), C.byref(params), 0, 0, 0, np.zeros(1, A.RAY_DTYPE).ctypes.data) != 0:
        raise RtrError(A.RTR_ERR_INVALID, "rtr_preview_ray: bad params")
    for j in range(h):
        for i in range(w):
            for s in range(kk):
                rc = L.rtr_preview_ray(C.byref(cam), C.byref(params), params.x0 + i, params.y0 + j, s,
                                       rays.ctypes.data + 80 * ((j * w + i) * kk + s))
                if rc != 0:
                    raise RtrError(rc, "rtr_preview_ray: bad params")
    return rays


def srgb_thresholds():
    """rtr_display_srgb_thresholds: the 256 doubles S that define RTR_ENCODE_SRGB (code = how many of S[1..255] are <= t)."""
    out = np.zeros(256, dtype=np.float64)
    lib().rtr_display_srgb_thresholds(out.ctypes.data)
    return out


def _display_result(r):
    return {"scale": r.scale, "metered": r.metered, "n_metered": int(r.n_metered)}


def camera_struct(cam):
    """An ``rtr_camera`` from a ``CAMERA_DTYPE`` record (``Scene.camera``, one element), a mapping of its fields, or a
    ready ``CameraC``."""
    if isinstance(cam, A.CameraC):
        return cam
    if isinstance(cam, np.ndarray):
        rec = np.ascontiguousarray(cam, dtype=A.CAMERA_DTYPE).reshape(-1)
        if len(rec) != 1:
            raise ValueError("one camera record expected")
        return A.CameraC.from_buffer_copy(rec.tobytes())
    out = A.CameraC()
    for name, ctype in A.CameraC._fields_:
        v = np.asarray(cam[name], dtype=np.float64).reshape(-1)
        setattr(out, name, float(v[0]) if ctype is C.c_double else ctype(*v))
    return out


def denoise_host(ctx, color, q, count, feat, params=None, rgb8=False, out=None):
    """rtr_denoise_host on ``ctx``: the denoiser over host planes of a region (row 0 = its lowest row) -- ``color``
    (H, W, 3) linear mean, ``q`` (H, W) second moments, ``count`` (H, W) samples of the pixel's tile (0: not a tap, its
    output keeps the value of ``out``), ``feat`` (H, W, 7) features; what a tile-sharded render gathers from its shards'
    resolve / moments / tiles / features.  Returns linear (H, W, 3) float64, or with ``rgb8`` the 8-bit store (Y
    flipped) as ``Accumulator.denoise``."""
    color = np.ascontiguousarray(color, dtype=np.float64)
    h, w = color.shape[:2]
    q = np.ascontiguousarray(q, dtype=np.float64)
    count = np.ascontiguousarray(count, dtype=np.int32)
    feat = np.ascontiguousarray(feat, dtype=np.float64)
    if color.shape != (h, w, 3) or q.shape != (h, w) or count.shape != (h, w) or feat.shape != (h, w, A.FEATURES):
        raise ValueError("planes of shapes (H, W, 3), (H, W), (H, W), (H, W, 7) expected")
    dtype = np.uint8 if rgb8 else np.float64
    if out is None:
        out = np.zeros((h, w, 3), dtype=dtype)
    elif out.shape != (h, w, 3) or out.dtype != dtype or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous %s array of shape (%d, %d, 3)" % (np.dtype(dtype).name, h, w))
    prm = params if params is not None else denoise_defaults()
    ctx._chk(ctx._L.rtr_denoise_host(ctx._h, C.byref(prm), w, h, color.ctypes.data, q.ctypes.data, count.ctypes.data,
                                     feat.ctypes.data, None if rgb8 else out.ctypes.data, out.ctypes.data if rgb8 else None))
    return out


def _records_out(out, n, dtype):
    """The output array of a query, gather or probe entry: ``out`` if it can take ``n`` records of ``dtype``, a zeroed
    array when it is None."""
    if out is None:
        return np.zeros(n, dtype=dtype)
    if out.dtype != dtype or len(out) < n or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous array of at least %d records of the entry's output dtype" % n)
    return out


def _into_tail(in_ptr, out_ptr, n, blocking):
    """The last four arguments of a gather, probe or lookup device entry"""
    return C.c_void_p(in_ptr), C.c_void_p(out_ptr), int(n), 1 if blocking else 0


class Context:
    """One GPU.  Mirrors the life cycle of the reference's ``Renderer`` object
    (renderer/renderer.h:22-28): create, give it a scene, render, cancel."""

    def __init__(self, device=0):
        self._L = lib()
        h = C.c_void_p()
        rc = self._L.rtr_create(int(device), C.byref(h))
        if rc != 0:
            raise RtrError(rc, self._L.rtr_last_error(None).decode())
        self._h = h
        self.device = int(device)
        self.scene = None
        self.camera_updated = False  # set_camera replaced the camera ``scene`` was uploaded with
        self._accums = weakref.WeakSet()  # (and histories: everything whose handle dies with the context)

    def close(self):
        if getattr(self, "_h", None):
            for a in list(self._accums):  # rtr_destroy frees them: their handles die with the context
                a._h = None
            self._L.rtr_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise RtrError(rc, self._L.rtr_last_error(self._h).decode())

    def set_stream(self, stream_handle):
        """Run the kernels on an existing hipStream_t (e.g. ``torch.cuda.current_stream().cuda_stream``)."""
        self._chk(self._L.rtr_set_stream(self._h, C.c_void_p(stream_handle or None)))

    def upload(self, scene):
        if not isinstance(scene, Scene):
            raise TypeError("expected a flattened Scene")
        d = scene.desc()
        self._chk(self._L.rtr_upload_scene(self._h, C.byref(d)))
        self.scene = scene
        self.camera_updated = False

    def set_camera(self, cam):
        """rtr_set_camera: a new camera (a ``CAMERA_DTYPE`` record, a mapping of its fields or a ``CameraC``) for every
        call issued from now on, without another upload; the image is the bits of an upload with that camera.
        Accumulators need ``reset`` before they render again.  ``Context.scene`` stays the uploaded scene;
        ``Context.camera_updated`` says whether the context's camera differs from ``scene.camera`` (``Renderer`` then puts
        it back before it renders that scene, and ``camera_ray`` follows the context's camera)."""
        c = camera_struct(cam)
        self._chk(self._L.rtr_set_camera(self._h, C.byref(c)))
        self.camera_updated = self.scene is None or bytes(c) != self.scene.camera.tobytes()

    def camera(self):
        """rtr_get_camera: the current camera as a one-element ``CAMERA_DTYPE`` array."""
        c = A.CameraC()
        self._chk(self._L.rtr_get_camera(self._h, C.byref(c)))
        return np.frombuffer(bytes(c), dtype=A.CAMERA_DTYPE).copy()

    def history(self, params):
        """A cleared temporal history (rtr_history_*) for the image size and region of ``params``."""
        h = History(self, params)
        self._accums.add(h)
        return h

    def render_into(self, params, device_ptr, row_stride, blocking=False):
        """Linear mean radiance of params' region into a device buffer of doubles."""
        self._chk(self._L.rtr_render_device(self._h, C.byref(params), C.c_void_p(device_ptr), int(row_stride),
                                            1 if blocking else 0))

    def render(self, params, out=None):
        """Blocking render to a host array (H, W, 3) of the region (includes the D2H copy).  Pixels of
        tiles the call does not own or, after a cancel, did not finish keep the values of ``out``."""
        h, w = params.y1 - params.y0, params.x1 - params.x0
        if out is None:
            out = np.zeros((h, w, 3), dtype=np.float64)
        if out.shape != (h, w, 3) or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float64 array of shape (%d, %d, 3)" % (h, w))
        self._chk(self._L.rtr_render_host(self._h, C.byref(params), out.ctypes.data, w))
        return out

    def plan_chunks(self, params):
        """Partial sums per pixel the library would use for ``params`` (its own choice when spp_chunks = 0)."""
        n = self._L.rtr_plan_chunks(self._h, C.byref(params))
        if n < 0:
            self._chk(n)
        return n

    def li_samples(self, params, ijs):
        """``Integrator::Li`` of the camera samples ``ijs`` ((n, 3) int32: pixel i, pixel j, sample index):
        radiance (n, 3), not divided by spp."""
        ijs = np.ascontiguousarray(ijs, dtype=np.int32).reshape(-1, 3)
        out = np.zeros((len(ijs), 3), dtype=np.float64)
        self._chk(self._L.rtr_li_samples(self._h, C.byref(params), ijs.ctypes.data, out.ctypes.data, len(ijs)))
        return out

    def li_rays(self, params, origins, directions, times, rng_states):
        """``Integrator::Li`` of arbitrary rays (n, 3) / (n, 3) / (n,) with the xorshift32 state (n,) the reference's
        generator would hold on entry: radiance (n, 3)."""
        n = len(origins)
        rays = np.zeros(n, dtype=A.LI_RAY_DTYPE)
        rays["origin"], rays["direction"], rays["time"], rays["rng_state"] = origins, directions, times, rng_states
        out = np.zeros((n, 3), dtype=np.float64)
        self._chk(self._L.rtr_li_rays(self._h, C.byref(params), rays.ctypes.data, out.ctypes.data, n))
        return out

    # ray queries (include/rtr_hip.h: rtr_query_*)
    @staticmethod
    def make_rays(origins, directions, times=None, t_min=0.001, t_max=np.inf, rng_states=None):
        """An ``RAY_DTYPE`` array from (n, 3) origins and directions; ``times`` (default 0), ``t_min``, ``t_max`` and
        ``rng_states`` (default 1; read only where the scene has media) are scalars or (n,) arrays."""
        o = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
        rays = np.zeros(len(o), dtype=A.RAY_DTYPE)
        rays["origin"], rays["direction"] = o, np.asarray(directions, dtype=np.float64).reshape(-1, 3)
        rays["time"] = 0.0 if times is None else times
        rays["t_min"], rays["t_max"] = t_min, t_max
        rays["rng_state"] = 1 if rng_states is None else rng_states
        return rays

    def _rays(self, origins, directions, times, t_min, t_max, rng_states):
        if isinstance(origins, np.ndarray) and origins.dtype == A.RAY_DTYPE:
            return np.ascontiguousarray(origins)
        return self.make_rays(origins, directions, times, t_min, t_max, rng_states)

    def query_closest(self, origins, directions=None, times=None, t_min=0.001, t_max=np.inf, rng_states=None,
                      reference_order=False, out=None):
        """``world->hit(ray, t_min, t_max, rec)`` of the uploaded scene for n rays (rtr_query_closest): a structured
        ``RAY_HIT_DTYPE`` array.  ``origins`` may be a ready ``RAY_DTYPE`` array (the other ray arguments are then
        ignored).  Blocking; raises RtrError (RTR_ERR_INVALID) naming the first bad ray, with ``out`` untouched."""
        rays = self._rays(origins, directions, times, t_min, t_max, rng_states)
        out = _records_out(out, len(rays), A.RAY_HIT_DTYPE)
        flags = A.FLAG_REFERENCE_ORDER if reference_order else 0
        self._chk(self._L.rtr_query_closest(self._h, rays.ctypes.data, out.ctypes.data, len(rays), flags))
        return out

    def query_occluded(self, origins, directions=None, times=None, t_min=0.001, t_max=np.inf, rng_states=None,
                       reference_order=False, return_rng=False):
        """Whether anything is hit in [t_min, t_max] (rtr_query_occluded): a bool array, or with ``return_rng`` the
        pair (bool array, uint32 generator states after the call)."""
        rays = self._rays(origins, directions, times, t_min, t_max, rng_states)
        occ = np.zeros(len(rays), dtype=np.uint8)
        rng = np.zeros(len(rays), dtype=np.uint32) if return_rng else None
        flags = A.FLAG_REFERENCE_ORDER if reference_order else 0
        self._chk(self._L.rtr_query_occluded(self._h, rays.ctypes.data, occ.ctypes.data,
                                             rng.ctypes.data if return_rng else None, len(rays), flags))
        return (occ.astype(bool), rng) if return_rng else occ.astype(bool)

    def query_closest_into(self, rays_ptr, hits_ptr, n, reference_order=False, blocking=False):
        """rtr_query_closest_device: n ``RAY_DTYPE`` records at device pointer ``rays_ptr`` -> ``RAY_HIT_DTYPE`` records at
        ``hits_ptr`` (e.g. a torch tensor's ``data_ptr()``), on the context stream behind what is queued there."""
        self._chk(self._L.rtr_query_closest_device(self._h, C.c_void_p(rays_ptr), C.c_void_p(hits_ptr), int(n),
                                                   A.FLAG_REFERENCE_ORDER if reference_order else 0, 1 if blocking else 0))

    def query_occluded_into(self, rays_ptr, occluded_ptr, n, rng_out_ptr=None, reference_order=False, blocking=False):
        """rtr_query_occluded_device: one byte per ray at ``occluded_ptr`` and, unless None, one uint32 at ``rng_out_ptr``."""
        self._chk(self._L.rtr_query_occluded_device(self._h, C.c_void_p(rays_ptr), C.c_void_p(occluded_ptr),
                                                    C.c_void_p(rng_out_ptr or None), int(n),
                                                    A.FLAG_REFERENCE_ORDER if reference_order else 0, 1 if blocking else 0))

    # hemisphere gathers (include/rtr_hip.h: rtr_gather_*)
    def gather_occlusion(self, points, normals=None, samples=64, seed=0, t_max=np.inf, t_min=0.001, time=0.0, point_base=0,
                         reference_order=False, params=None, out=None):
        """rtr_gather_occlusion: ``samples`` cosine-distributed rays about every normal, any-hit cast in [t_min, t_max] and
        reduced on the device.  Returns a ``GATHER_OUT_DTYPE`` array: ``count`` unblocked samples (count / samples is the
        ambient occlusion), ``v`` the unnormalised bent normal, ``valid`` 1.  ``points`` may be a ready
        ``GATHER_POINT_DTYPE`` array; ``params`` a ready rtr_gather_params (the keyword values are then ignored).
        Blocking; raises RtrError (RTR_ERR_INVALID) naming the first bad point, with ``out`` untouched."""
        gp = params if params is not None else gather_defaults(
            samples=samples, seed=seed, t_max=t_max, t_min=t_min, time=time, point_base=point_base, reference_order=reference_order)
        pts = gather_points(points, normals)
        out = _records_out(out, len(pts), A.GATHER_OUT_DTYPE)
        self._chk(self._L.rtr_gather_occlusion(self._h, C.byref(gp), pts.ctypes.data, out.ctypes.data, len(pts)))
        return out

    def gather_radiance(self, params, points, normals=None, samples=64, seed=0, time=0.0, point_base=0, gather_params=None,
                        out=None):
        """rtr_gather_radiance: the mean of ``Integrator::Li`` over ``samples`` cosine-distributed rays about every normal
        under ``params`` (an rtr_render_params: integrator, max_depth, rr_start_depth, flags); irradiance is pi * v."""
        gp = gather_params if gather_params is not None else gather_defaults(samples=samples, seed=seed, time=time,
                                                                             point_base=point_base)
        pts = gather_points(points, normals)
        out = _records_out(out, len(pts), A.GATHER_OUT_DTYPE)
        self._chk(self._L.rtr_gather_radiance(self._h, C.byref(params), C.byref(gp), pts.ctypes.data, out.ctypes.data, len(pts)))
        return out

    def gather_occlusion_into(self, points_ptr, out_ptr, n, params=None, blocking=False, **overrides):
        """rtr_gather_occlusion_device: n ``GATHER_POINT_DTYPE`` records at device pointer ``points_ptr`` ->
        ``GATHER_OUT_DTYPE`` records at ``out_ptr``, on the context stream behind what is queued there."""
        gp = params if params is not None else gather_defaults(**overrides)
        self._chk(self._L.rtr_gather_occlusion_device(self._h, C.byref(gp), *_into_tail(points_ptr, out_ptr, n, blocking)))

    def gather_radiance_into(self, params, points_ptr, out_ptr, n, gather_params=None, blocking=False, **overrides):
        """rtr_gather_radiance_device: the device-pointer form of ``gather_radiance``."""
        gp = gather_params if gather_params is not None else gather_defaults(**overrides)
        self._chk(self._L.rtr_gather_radiance_device(self._h, C.byref(params), C.byref(gp),
                                                     *_into_tail(points_ptr, out_ptr, n, blocking)))

    @staticmethod
    def gather_rays(points, normals=None, params=None, **overrides):
        """The rays the gathers cast, ``RAY_DTYPE`` [n, samples], through rtr_gather_ray (``native.gather_rays``)."""
        return gather_rays(points, normals, params, **overrides)

    # light probes (include/rtr_hip.h: rtr_probe_*)
    def probe_visibility(self, points, samples=64, seed=0, t_max=np.inf, t_min=0.001, time=0.0, point_base=0,
                         reference_order=False, params=None, out=None):
        """rtr_probe_visibility: ``samples`` rays uniform over the sphere from every point, any-hit cast in [t_min, t_max],
        the unblocked ones projected onto nine spherical harmonics and reduced on the device.  Returns a ``PROBE_VIS_DTYPE``
        array (``c`` [9], ``count`` unblocked samples, ``valid`` 1).  Blocking; raises RtrError (RTR_ERR_INVALID) naming the
        first bad point, with ``out`` untouched."""
        gp = params if params is not None else gather_defaults(
            samples=samples, seed=seed, t_max=t_max, t_min=t_min, time=time, point_base=point_base, reference_order=reference_order)
        pts = probe_points(points)
        out = _records_out(out, len(pts), A.PROBE_VIS_DTYPE)
        self._chk(self._L.rtr_probe_visibility(self._h, C.byref(gp), pts.ctypes.data, out.ctypes.data, len(pts)))
        return out

    def probe_radiance(self, params, points, samples=64, seed=0, time=0.0, point_base=0, gather_params=None, out=None):
        """rtr_probe_radiance: ``Integrator::Li`` of ``samples`` rays uniform over the sphere from every point under
        ``params`` (an rtr_render_params), projected onto nine spherical harmonics per channel.  Returns a
        ``PROBE_SH_DTYPE`` array (``c`` [9, 3]); the coefficient estimate is 4 pi * c (``sh_irradiance`` applies it)."""
        gp = gather_params if gather_params is not None else gather_defaults(samples=samples, seed=seed, time=time,
                                                                             point_base=point_base)
        pts = probe_points(points)
        out = _records_out(out, len(pts), A.PROBE_SH_DTYPE)
        self._chk(self._L.rtr_probe_radiance(self._h, C.byref(params), C.byref(gp), pts.ctypes.data, out.ctypes.data, len(pts)))
        return out

    def probe_visibility_into(self, points_ptr, out_ptr, n, params=None, blocking=False, **overrides):
        """rtr_probe_visibility_device: n ``PROBE_POINT_DTYPE`` records at device pointer ``points_ptr`` ->
        ``PROBE_VIS_DTYPE`` records at ``out_ptr``, on the context stream behind what is queued there."""
        gp = params if params is not None else gather_defaults(**overrides)
        self._chk(self._L.rtr_probe_visibility_device(self._h, C.byref(gp), *_into_tail(points_ptr, out_ptr, n, blocking)))

    def probe_radiance_into(self, params, points_ptr, out_ptr, n, gather_params=None, blocking=False, **overrides):
        """rtr_probe_radiance_device: the device-pointer form of ``probe_radiance``."""
        gp = gather_params if gather_params is not None else gather_defaults(**overrides)
        self._chk(self._L.rtr_probe_radiance_device(self._h, C.byref(params), C.byref(gp),
                                                    *_into_tail(points_ptr, out_ptr, n, blocking)))

    @staticmethod
    def probe_rays(points, params=None, **overrides):
        """The rays the probe kernels cast, ``RAY_DTYPE`` [n, samples], through rtr_probe_ray (``native.probe_rays``)."""
        return probe_rays(points, params, **overrides)

    def probe_lookup(self, grid, probes, points, normals=None, out=None):
        """rtr_probe_lookup: irradiance at the queries (points, normals) from the ``PROBE_SH_DTYPE`` records of ``grid`` (an
        rtr_probe_grid: ``native.probe_grid``), trilinear in the coefficients.  Returns a ``GATHER_OUT_DTYPE`` array
        (``v`` the irradiance, ``count`` the corners used, ``valid``).  Blocking; needs no scene."""
        probes = np.ascontiguousarray(probes, dtype=A.PROBE_SH_DTYPE)
        if len(probes) != grid.dims[0] * grid.dims[1] * grid.dims[2]:
            raise ValueError("probes must hold dims[0] * dims[1] * dims[2] records")
        q = gather_points(points, normals)
        out = _records_out(out, len(q), A.GATHER_OUT_DTYPE)
        self._chk(self._L.rtr_probe_lookup(self._h, C.byref(grid), probes.ctypes.data, q.ctypes.data, out.ctypes.data, len(q)))
        return out

    def probe_lookup_into(self, grid, probes_ptr, queries_ptr, out_ptr, n, blocking=False):
        """rtr_probe_lookup_device: the same over device pointers, on the context stream behind what is queued there."""
        self._chk(self._L.rtr_probe_lookup_device(self._h, C.byref(grid), C.c_void_p(probes_ptr),
                                                  *_into_tail(queries_ptr, out_ptr, n, blocking)))

    # probe distance maps (include/rtr_hip.h: rtr_probe_depth*, rtr_probe_lookup_visible*)
    def probe_depth(self, points, depth_params=None, out=None, **overrides):
        """rtr_probe_depth: the ``PROBE_DEPTH_DTYPE`` records [n, T, T] (row, column) of the octahedral distance maps of
        the probes ``points``; ``t_max`` must be given.  Blocking; raises RtrError (RTR_ERR_INVALID) naming the first bad
        probe, with ``out`` untouched."""
        dp = depth_params if depth_params is not None else probe_depth_defaults(**overrides)
        pts = probe_points(points)
        T = int(dp.map_size)
        flat = _records_out(None if out is None else out.reshape(-1), len(pts) * T * T, A.PROBE_DEPTH_DTYPE)
        self._chk(self._L.rtr_probe_depth(self._h, C.byref(dp), pts.ctypes.data, flat.ctypes.data, len(pts)))
        return flat[:len(pts) * T * T].reshape(len(pts), T, T)

    def probe_depth_into(self, points_ptr, out_ptr, n, depth_params=None, blocking=False, **overrides):
        """rtr_probe_depth_device: n ``PROBE_POINT_DTYPE`` probes at device pointer ``points_ptr`` -> n * T * T
        ``PROBE_DEPTH_DTYPE`` records at ``out_ptr``, on the context stream behind what is queued there."""
        dp = depth_params if depth_params is not None else probe_depth_defaults(**overrides)
        self._chk(self._L.rtr_probe_depth_device(self._h, C.byref(dp), *_into_tail(points_ptr, out_ptr, n, blocking)))

    @staticmethod
    def probe_depth_rays(points, params=None, **overrides):
        """The rays rtr_probe_depth casts, ``RAY_DTYPE`` [n, T, T, samples], through rtr_probe_depth_ray
        (``native.probe_depth_rays``)."""
        return probe_depth_rays(points, params, **overrides)

    def probe_lookup_visible(self, grid, probes, depth, points, normals=None, normal_bias=0.0, map_size=None, params=None,
                             out=None):
        """rtr_probe_lookup_visible: ``probe_lookup`` with every corner weighed by what its probe's distance map
        (``depth``: ``PROBE_DEPTH_DTYPE`` [probes, T, T]) says of the way to the query.  Blocking; needs no scene."""
        probes, depth, T = _visible_inputs(grid, probes, depth, map_size if params is None else params.map_size)
        vp = params if params is not None else probe_visible_params(T, normal_bias)
        q = gather_points(points, normals)
        out = _records_out(out, len(q), A.GATHER_OUT_DTYPE)
        self._chk(self._L.rtr_probe_lookup_visible(self._h, C.byref(grid), probes.ctypes.data, depth.ctypes.data, C.byref(vp),
                                                   q.ctypes.data, out.ctypes.data, len(q)))
        return out

    def probe_lookup_visible_into(self, grid, probes_ptr, depth_ptr, params, queries_ptr, out_ptr, n, blocking=False):
        """rtr_probe_lookup_visible_device: the same over device pointers, on the context stream behind what is queued
        there; ``params`` is an rtr_probe_visible_params (``native.probe_visible_params``)."""
        self._chk(self._L.rtr_probe_lookup_visible_device(self._h, C.byref(grid), C.c_void_p(probes_ptr), C.c_void_p(depth_ptr),
                                                          C.byref(params), *_into_tail(queries_ptr, out_ptr, n, blocking)))

    # environment captures (include/rtr_hip.h: rtr_capture_*, rtr_cube_*)
    def capture_cube_records(self, params, points, capture_params=None, out=None, **overrides):
        """rtr_capture_cube: the ``GATHER_OUT_DTYPE`` records [n, 6, S, S] (face, row, column) of the cube maps about the
        centres ``points`` under ``params`` (an rtr_render_params).  Blocking; raises RtrError (RTR_ERR_INVALID) naming the
        first bad centre, with ``out`` untouched."""
        cp = capture_params if capture_params is not None else capture_defaults(**overrides)
        pts = probe_points(points)
        S = int(cp.face_size)
        flat = _records_out(None if out is None else out.reshape(-1), len(pts) * 6 * S * S, A.GATHER_OUT_DTYPE)
        self._chk(self._L.rtr_capture_cube(self._h, C.byref(params), C.byref(cp), pts.ctypes.data, flat.ctypes.data, len(pts)))
        return flat[:len(pts) * 6 * S * S].reshape(len(pts), 6, S, S)

    def capture_cube(self, params, points, face_size=32, samples=16, seed=0, jitter=1, time=0.0, point_base=0):
        """The mean radiance float64 [n, 6, S, S, 3] of ``capture_cube_records`` and its valid mask, bool [n, 6, S, S]."""
        rec = self.capture_cube_records(params, points, face_size=face_size, samples=samples, seed=seed, jitter=jitter,
                                        time=time, point_base=point_base)
        return np.ascontiguousarray(rec["v"]), rec["valid"] != 0

    def capture_cube_into(self, params, points_ptr, out_ptr, n, capture_params=None, blocking=False, **overrides):
        """rtr_capture_cube_device: n ``PROBE_POINT_DTYPE`` centres at device pointer ``points_ptr`` -> n * 6 * S * S
        ``GATHER_OUT_DTYPE`` records at ``out_ptr``, on the context stream behind what is queued there."""
        cp = capture_params if capture_params is not None else capture_defaults(**overrides)
        self._chk(self._L.rtr_capture_cube_device(self._h, C.byref(params), C.byref(cp),
                                                  *_into_tail(points_ptr, out_ptr, n, blocking)))

    @staticmethod
    def capture_rays(points, params=None, **overrides):
        """The rays a capture casts, ``RAY_DTYPE`` [n, 6, S, S, samples], through rtr_capture_ray (``native.capture_rays``)."""
        return capture_rays(points, params, **overrides)

    def cube_lookup(self, texels, directions, face_size=None, out=None):
        """rtr_cube_lookup: the radiance of one capture (6 * S * S records, or [6, S, S]) along the directions [n, 3],
        bilinear inside a face.  Returns a ``GATHER_OUT_DTYPE`` array (``count`` the texels used).  Blocking; needs no scene."""
        S, t = _cube_texels(texels, face_size)
        q = probe_points(directions)
        out = _records_out(out, len(q), A.GATHER_OUT_DTYPE)
        self._chk(self._L.rtr_cube_lookup(self._h, S, t.ctypes.data, q.ctypes.data, out.ctypes.data, len(q)))
        return out

    def cube_lookup_into(self, face_size, texels_ptr, directions_ptr, out_ptr, n, blocking=False):
        """rtr_cube_lookup_device: the same over device pointers, on the context stream behind what is queued there."""
        self._chk(self._L.rtr_cube_lookup_device(self._h, int(face_size), C.c_void_p(texels_ptr),
                                                 *_into_tail(directions_ptr, out_ptr, n, blocking)))

    # filtered cube maps (include/rtr_hip.h: rtr_cube_filter*, rtr_cube_chain_*)
    def cube_filter(self, texels, params=None, out=None, **overrides):
        """rtr_cube_filter: the GGX-filtered records [n_cubes, 6, face_out, face_out] of the source cubes ``texels``
        ([n_cubes, 6, face_in, face_in] or flat).  Blocking; needs no scene."""
        fp = params if params is not None else cube_filter_defaults(**overrides)
        t, n = _filter_cubes(texels, fp)
        So = int(fp.face_out)
        flat = _records_out(None if out is None else out.reshape(-1), n * 6 * So * So, A.GATHER_OUT_DTYPE)
        self._chk(self._L.rtr_cube_filter(self._h, C.byref(fp), t.ctypes.data, flat.ctypes.data, n))
        return flat[:n * 6 * So * So].reshape(n, 6, So, So)

    def cube_filter_into(self, texels_ptr, out_ptr, n_cubes, params=None, blocking=False, **overrides):
        """rtr_cube_filter_device: n_cubes * 6 * face_in^2 records at device pointer ``texels_ptr`` -> n_cubes * 6 *
        face_out^2 at ``out_ptr``, on the context stream behind what is queued there."""
        fp = params if params is not None else cube_filter_defaults(**overrides)
        self._chk(self._L.rtr_cube_filter_device(self._h, C.byref(fp), *_into_tail(texels_ptr, out_ptr, n_cubes, blocking)))

    def cube_chain_lookup(self, levels, texels, queries, out=None, n_levels=None):
        """rtr_cube_chain_lookup: the seam-aware lookup of ``queries`` (``CUBE_QUERY_DTYPE``) in the chain ``levels`` over the
        records ``texels``, two levels blended by alpha.  Returns a ``GATHER_OUT_DTYPE`` array.  Blocking; needs no scene."""
        lv = cube_levels(levels)
        t = np.ascontiguousarray(texels, dtype=A.GATHER_OUT_DTYPE).reshape(-1)
        q = np.ascontiguousarray(queries, dtype=A.CUBE_QUERY_DTYPE)
        out = _records_out(out, len(q), A.GATHER_OUT_DTYPE)
        self._chk(self._L.rtr_cube_chain_lookup(self._h, C.byref(lv), len(levels) if n_levels is None else int(n_levels),
                                                t.ctypes.data, len(t), q.ctypes.data, out.ctypes.data, len(q)))
        return out

    def cube_chain_lookup_into(self, levels, texels_ptr, n_records, queries_ptr, out_ptr, n, blocking=False, n_levels=None):
        """rtr_cube_chain_lookup_device: the same over device pointers (``levels`` stays a host table), on the context
        stream behind what is queued there."""
        lv = cube_levels(levels)
        self._chk(self._L.rtr_cube_chain_lookup_device(self._h, C.byref(lv), len(levels) if n_levels is None else int(n_levels),
                                                       C.c_void_p(texels_ptr), int(n_records),
                                                       *_into_tail(queries_ptr, out_ptr, n, blocking)))

    # capture sets (include/rtr_hip.h: rtr_capture_set*)
    def capture_set_lookup(self, cset, levels, records, queries, out=None, n_levels=None):
        """rtr_capture_set_lookup: the box-projected, blended lookup of ``queries`` (``CAPTURE_QUERY_DTYPE``) in the set
        ``cset`` (``native.capture_set``) over its level-major ``records``; ``levels`` is the plan of one capture.  Returns a
        ``GATHER_OUT_DTYPE`` array.  Blocking; needs no scene."""
        lv = cube_levels(levels)
        t = np.ascontiguousarray(records, dtype=A.GATHER_OUT_DTYPE).reshape(-1)
        q = np.ascontiguousarray(queries, dtype=A.CAPTURE_QUERY_DTYPE).reshape(-1)
        out = _records_out(out, len(q), A.GATHER_OUT_DTYPE)
        c = max(int(cset.n_captures), 1)
        self._chk(self._L.rtr_capture_set_lookup(self._h, C.byref(cset), C.byref(lv), len(levels) if n_levels is None else int(n_levels),
                                                 t.ctypes.data, len(t) // c, q.ctypes.data, out.ctypes.data, len(q)))
        return out

    def capture_set_lookup_into(self, cset, levels, records_ptr, n_records, queries_ptr, out_ptr, n, blocking=False, n_levels=None):
        """rtr_capture_set_lookup_device: the same over device pointers (``cset`` and ``levels`` stay on the host;
        ``n_records`` is one capture's count), on the context stream behind what is queued there."""
        lv = cube_levels(levels)
        self._chk(self._L.rtr_capture_set_lookup_device(self._h, C.byref(cset), C.byref(lv),
                                                        len(levels) if n_levels is None else int(n_levels),
                                                        C.c_void_p(records_ptr), int(n_records),
                                                        *_into_tail(queries_ptr, out_ptr, n, blocking)))

    # image-based shading (include/rtr_hip.h: rtr_brdf_*, rtr_shade_ibl*)
    def brdf_table(self, n_mu, n_rough, nodes=128, params=None, out=None):
        """rtr_brdf_table: the environment BRDF table, ``BRDF_ENTRY_DTYPE`` [n_rough, n_mu].  Blocking; needs no scene."""
        bp = params if params is not None else brdf_params(n_mu, n_rough, nodes)
        n = max(int(bp.n_mu), 0) * max(int(bp.n_rough), 0)
        flat = _records_out(None if out is None else out.reshape(-1), n, A.BRDF_ENTRY_DTYPE)
        self._chk(self._L.rtr_brdf_table(self._h, C.byref(bp), flat.ctypes.data))
        return flat[:n].reshape(int(bp.n_rough), int(bp.n_mu))

    def brdf_table_into(self, out_ptr, n_mu, n_rough, nodes=128, params=None, blocking=False):
        """rtr_brdf_table_device: n_rough * n_mu ``BRDF_ENTRY_DTYPE`` records at device pointer ``out_ptr``, on the context
        stream behind what is queued there."""
        bp = params if params is not None else brdf_params(n_mu, n_rough, nodes)
        self._chk(self._L.rtr_brdf_table_device(self._h, C.byref(bp), C.c_void_p(out_ptr), 1 if blocking else 0))

    def shade_ibl(self, env, queries, out=None, captures=None):
        """rtr_shade_ibl: the radiance of the ``SHADE_QUERY_DTYPE`` queries under ``env`` (``native.shade_env`` of host
        arrays), a ``GATHER_OUT_DTYPE`` array.  Blocking; needs no scene; raises RtrError naming the first bad query.
        ``captures`` (``native.capture_set``): rtr_shade_ibl_set -- ``env.chain`` holds that set level-major."""
        q = np.ascontiguousarray(queries, dtype=A.SHADE_QUERY_DTYPE).reshape(-1)
        out = _records_out(out, len(q), A.GATHER_OUT_DTYPE)
        if captures is None:
            self._chk(self._L.rtr_shade_ibl(self._h, C.byref(env), q.ctypes.data, out.ctypes.data, len(q)))
        else:
            self._chk(self._L.rtr_shade_ibl_set(self._h, C.byref(env), C.byref(captures), q.ctypes.data, out.ctypes.data, len(q)))
        return out

    def shade_ibl_into(self, env, queries_ptr, out_ptr, n, blocking=False, captures=None):
        """rtr_shade_ibl_device: the same over device pointers (``env``: ``native.shade_env`` of device pointers; the
        struct, its grid, visible params and levels stay on the host), on the context stream behind what is queued there.
        ``captures``: rtr_shade_ibl_set_device."""
        if captures is None:
            self._chk(self._L.rtr_shade_ibl_device(self._h, C.byref(env), *_into_tail(queries_ptr, out_ptr, n, blocking)))
        else:
            self._chk(self._L.rtr_shade_ibl_set_device(self._h, C.byref(env), C.byref(captures),
                                                       *_into_tail(queries_ptr, out_ptr, n, blocking)))

    # baked previews (include/rtr_hip.h: rtr_preview_*)
    def preview(self, params, env, out=None, return_lit=False, captures=None):
        """rtr_preview: the frame of ``params``' region shaded under ``env`` (``native.shade_env`` of host arrays) from the
        context's current camera: linear (h, w, 3) float64, row 0 the lowest row, or with ``return_lit`` the pair
        (linear, lit (h, w) int32).  Blocking.  ``out`` may be a view with strided rows: only region pixels are written.
        ``captures`` (``native.capture_set``): rtr_preview_set -- ``env.chain`` holds that set level-major."""
        h, w = params.y1 - params.y0, params.x1 - params.x0

        def run(linear, stride, lit):
            if captures is None:
                return self._L.rtr_preview(self._h, C.byref(params), C.byref(env), linear, stride, lit)
            return self._L.rtr_preview_set(self._h, C.byref(params), C.byref(env), C.byref(captures), linear, stride, lit)

        if h <= 0 or w <= 0:  # an empty region: the library's error
            self._chk(run(np.zeros(3).ctypes.data, 1, None))
        if out is None:
            out = np.zeros((h, w, 3), dtype=np.float64)
        if (out.dtype != np.float64 or out.shape != (h, w, 3) or out.strides[2] != 8 or out.strides[1] != 24 or
                (h > 1 and (out.strides[0] % 24 or out.strides[0] < 24 * w))):
            raise ValueError("out must be a float64 array of shape (%d, %d, 3) whose rows are whole pixels apart" % (h, w))
        stride = out.strides[0] // 24 if h > 1 else w
        lit = np.zeros((max(h, 0), stride), dtype=np.int32) if return_lit else None
        self._chk(run(out.ctypes.data, stride, lit.ctypes.data if return_lit else None))
        return (out, lit[:, :w]) if return_lit else out

    def preview_into(self, params, env, linear_ptr, row_stride, lit_ptr=None, blocking=False, captures=None):
        """rtr_preview_device: the same into device pointers (``env``: ``native.shade_env`` of device pointers), rows
        ``row_stride`` pixels apart, on the context stream behind what is queued there -- the bakes included; the layout
        ``display_into`` reads.  ``captures``: rtr_preview_set_device."""
        tail = (C.c_void_p(linear_ptr), int(row_stride), C.c_void_p(lit_ptr or None), 1 if blocking else 0)
        if captures is None:
            self._chk(self._L.rtr_preview_device(self._h, C.byref(params), C.byref(env), *tail))
        else:
            self._chk(self._L.rtr_preview_set_device(self._h, C.byref(params), C.byref(env), C.byref(captures), *tail))

    def preview_samples(self, params, out=None):
        """rtr_preview_samples: the G-buffer of a preview, ``PREVIEW_SAMPLE_DTYPE`` [h, w, grid^2].  Blocking."""
        h, w, kk = params.y1 - params.y0, params.x1 - params.x0, params.grid * params.grid
        n = max(h, 0) * max(w, 0) * max(kk, 0)
        flat = _records_out(None if out is None else out.reshape(-1), n, A.PREVIEW_SAMPLE_DTYPE)
        self._chk(self._L.rtr_preview_samples(self._h, C.byref(params), flat.ctypes.data))
        return flat[:n].reshape(h, w, kk)

    def preview_samples_into(self, params, out_ptr, blocking=False):
        """rtr_preview_samples_device: h * w * grid^2 ``PREVIEW_SAMPLE_DTYPE`` records at device pointer ``out_ptr``."""
        self._chk(self._L.rtr_preview_samples_device(self._h, C.byref(params), C.c_void_p(out_ptr), 1 if blocking else 0))

    def preview_rays(self, params):
        """The rays a preview casts, ``RAY_DTYPE`` [h, w, grid^2], through rtr_preview_ray under the context's current
        camera (``native.preview_rays``)."""
        return preview_rays(self.camera(), params)

    # display transform (include/rtr_hip.h: rtr_display_*)
    @staticmethod
    def _linear_image(linear):
        """(array, width, height, row stride in pixels) of an (H, W, 3) float64 image whose rows may be strided"""
        a = np.asarray(linear, dtype=np.float64)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("an (H, W, 3) image expected")
        h, w = a.shape[:2]
        if a.strides[2] != 8 or a.strides[1] != 24 or a.strides[0] % 24 or a.strides[0] < 24 * w:
            a = np.ascontiguousarray(a)
        return a, w, h, a.strides[0] // 24

    def luminance_histogram(self, linear):
        """rtr_display_histogram: (the 512 counts of the metering pass as uint32, the number of metered pixels) of an
        (H, W, 3) linear image."""
        a, w, h, stride = self._linear_image(linear)
        hist = np.zeros(A.DISPLAY_BINS, dtype=np.uint32)
        n = C.c_int64(0)
        self._chk(self._L.rtr_display_histogram(self._h, w, h, a.ctypes.data, stride, hist.ctypes.data, C.byref(n)))
        return hist, int(n.value)

    def display(self, linear, params=None, mapped=False):
        """rtr_display_host: the display transform (``params``: an rtr_display_params, default ``display_defaults()``)
        of an (H, W, 3) linear image whose row 0 is the lowest row.  Returns ``(rgb8, result)`` -- (H, W, 3) uint8 with
        the TOP row first and a dict of scale, metered, n_metered -- or with ``mapped`` ``(rgb8, t, result)``, t the
        tone-mapped values in [0, 1] as (H, W, 3) float64 in the input's row order."""
        a, w, h, stride = self._linear_image(linear)
        prm = params if params is not None else display_defaults()
        rgb8 = np.zeros((h, w, 3), dtype=np.uint8)
        t = np.zeros((h, w, 3), dtype=np.float64) if mapped else None
        res = A.DisplayResultC()
        self._chk(self._L.rtr_display_host(self._h, C.byref(prm), w, h, a.ctypes.data, stride, rgb8.ctypes.data,
                                           t.ctypes.data if mapped else None, C.byref(res)))
        return (rgb8, t, _display_result(res)) if mapped else (rgb8, _display_result(res))

    def display_into(self, linear_ptr, row_stride, width, height, rgb8_ptr, params=None, mapped_ptr=None, blocking=False):
        """rtr_display_device: the transform of ``height`` rows of ``width`` pixels at device pointer ``linear_ptr``
        (``row_stride`` pixels apart) into ``rgb8_ptr`` (bytes, top row first) and / or ``mapped_ptr`` (doubles), on the
        context stream behind what is queued there -- a non-blocking ``render_into`` included.  Returns the result dict
        when ``blocking``, else None."""
        prm = params if params is not None else display_defaults()
        res = A.DisplayResultC()
        self._chk(self._L.rtr_display_device(self._h, C.byref(prm), int(width), int(height), C.c_void_p(linear_ptr),
                                             int(row_stride), C.c_void_p(rgb8_ptr or None), C.c_void_p(mapped_ptr or None),
                                             C.byref(res) if blocking else None, 1 if blocking else 0))
        return _display_result(res) if blocking else None

    def camera_ray(self, params, i, j):
        """The pixel-centre ray of pixel (i, j) of the image ``params`` describes, as a one-element ``RAY_DTYPE`` array with
        the query defaults (t_min 0.001, t_max inf): u = (i + 0.5) / (W - 1), v = (j + 0.5) / (H - 1), origin = the
        camera's, direction = lower_left_corner + u horizontal + v vertical - origin in the reference's operation order
        (camera.h get_ray without a lens offset), time = time0; no draw."""
        if self.scene is None:
            raise RtrError(A.RTR_ERR_NO_SCENE, "camera_ray before upload")
        cam = self.camera()  # the context's current camera: scene.camera unless set_camera replaced it
        u = (i + 0.5) / (params.image_width - 1)
        v = (j + 0.5) / (params.image_height - 1)
        o = np.asarray(cam["origin"], dtype=np.float64).reshape(3)
        d = (np.asarray(cam["lower_left_corner"], dtype=np.float64).reshape(3) + u * np.asarray(cam["horizontal"], dtype=np.float64).reshape(3)
             + v * np.asarray(cam["vertical"], dtype=np.float64).reshape(3)) - o
        return self.make_rays(o[None, :], d[None, :], times=float(np.asarray(cam["time0"]).reshape(-1)[0]))

    def accumulator(self, params, moments=False):
        """A progressive accumulator (rtr_accum_*) bound to ``params``' region, image size, tile sharding, seed,
        integrator, depths, pipeline and flags (its spp and spp_chunks are ignored) and to the scene uploaded now.
        ``moments``: it also keeps per-pixel second moments (RTR_ACCUM_MOMENTS), for ``errors`` and ``refine``."""
        a = Accumulator(self, params, moments)
        self._accums.add(a)
        return a

    def synchronize(self):
        self._chk(self._L.rtr_synchronize(self._h))

    def cancel(self):
        self._chk(self._L.rtr_cancel(self._h))

    def stats(self):
        s = A.RenderStatsC()
        self._chk(self._L.rtr_get_stats(self._h, C.byref(s)))
        return {"samples": s.samples, "closest_segments": s.closest_segments, "shadow_segments": s.shadow_segments,
                "device_ms": s.device_ms, "kernel_launches": s.kernel_launches, "pipeline": s.pipeline,
                "spp_chunks": s.spp_chunks, "cancelled": bool(s.cancelled), "flags_in_effect": s.flags_in_effect}

    def last_kernel(self):
        """The kernel instantiation the last render call launched (include/rtr_hip_test.h: rtr_kernel_record), as a dict;
        None before any render of this context launched one."""
        r = KernelRecordC()
        self._chk(test_lib().rtr_test_last_kernel(self._h, C.byref(r), C.sizeof(r)))
        if r.pipeline < 0:
            return None
        return {name: int(getattr(r, name)) for name, _ in KernelRecordC._fields_}

    def last_gather(self):
        """The gather kernel the last gather call launched (include/rtr_hip_test.h: rtr_gather_record), as a dict; None
        before any gather of this context launched one."""
        r = GatherRecordC()
        self._chk(test_lib().rtr_test_last_gather(self._h, C.byref(r), C.sizeof(r)))
        if r.trav < 0:
            return None
        return {name: int(getattr(r, name)) for name, _ in GatherRecordC._fields_}

    def last_probe(self):
        """The probe kernel the last probe_visibility / probe_radiance call launched (include/rtr_hip_test.h:
        rtr_probe_record), as a dict; None before any such call of this context launched one."""
        r = ProbeRecordC()
        self._chk(test_lib().rtr_test_last_probe(self._h, C.byref(r), C.sizeof(r)))
        if r.trav < 0:
            return None
        return {name: int(getattr(r, name)) for name, _ in ProbeRecordC._fields_}

    def last_probe_depth(self):
        """The distance-map kernel the last probe_depth call launched (include/rtr_hip_test.h: rtr_probe_depth_record), as
        a dict; None before any such call of this context launched one."""
        r = ProbeDepthRecordC()
        self._chk(test_lib().rtr_test_last_probe_depth(self._h, C.byref(r), C.sizeof(r)))
        if r.trav < 0:
            return None
        return {name: int(getattr(r, name)) for name, _ in ProbeDepthRecordC._fields_}

    def last_capture(self):
        """The capture kernel the last capture_cube call launched (include/rtr_hip_test.h: rtr_capture_record), as a dict;
        None before any such call of this context launched one."""
        r = CaptureRecordC()
        self._chk(test_lib().rtr_test_last_capture(self._h, C.byref(r), C.sizeof(r)))
        if r.trav < 0:
            return None
        return {name: int(getattr(r, name)) for name, _ in CaptureRecordC._fields_}

    def reference_order(self, on):
        """Force the reference-order traversal for rtr_test_hits (renders use params.flags)."""
        self._chk(test_lib().rtr_test_reference_order(self._h, 1 if on else 0))

    def stream8(self, n_doubles, repeat=1):
        """Counter calibration: stream n_doubles doubles in and out, 8 bytes per lane (include/rtr_hip_test.h)."""
        self._chk(test_lib().rtr_test_stream8(self._h, int(n_doubles), int(repeat)))

    def sincos_exhaustive(self):
        """All 2^32 sampler angles: (how many give sincos(phi) != (sin(phi), cos(phi)) in some bit, how many the kernel
        compared) (include/rtr_hip_test.h)."""
        n, tested = C.c_uint64(0), C.c_uint64(0)
        self._chk(test_lib().rtr_test_sincos_exhaustive(self._h, C.byref(n), C.byref(tested)))
        return int(n.value), int(tested.value)

    def draw_forms(self):
        """rtr_test_draw_forms (include/rtr_hip_test.h): all 2^32 generator states through the joined form of a draw in
        (-1, 1) and the plain text: (states where it differs in some bit, states compared, such a state + 1 or 0)."""
        n, tested, first = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._chk(test_lib().rtr_test_draw_forms(self._h, C.byref(n), C.byref(tested), C.byref(first)))
        return int(n.value), int(tested.value), int(first.value)

    def draw_callers(self, seed, n):
        """rtr_test_draw_callers (include/rtr_hip_test.h): every function that draws, with the joined form and in the plain
        text, from ``n`` states seeded by ``seed``: (lanes where an output bit or an exit state differs, lanes compared,
        such a lane's starting state or 0)."""
        bad, tested, first = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._chk(test_lib().rtr_test_draw_callers(self._h, int(seed), int(n), C.byref(bad), C.byref(tested), C.byref(first)))
        return int(bad.value), int(tested.value), int(first.value)

    def sincos_mismatches(self):
        """All 2^32 sampler angles: how many give sincos(phi) != (sin(phi), cos(phi)) in some bit (include/rtr_hip_test.h)."""
        return self.sincos_exhaustive()[0]

    ISSUE_CLASSES = ("v_fma_f64", "v_add_f64", "v_mul_f64", "v_rcp_f64", "v_rsq_f64", "v_cmp_lt_f64", "v_cndmask_b32",
                     "v_mov_b32", "v_fma_f32", "s_and_b64", "v_div_scale_f64", "v_div_fixup_f64", "v_cmp_f64+s_and_b64",
                     "v_cndmask_b32 (scalar-pair mask)", "v_min_f32", "v_cmp_f32+v_cndmask_b32", "v_cndmask_b32 (4 destinations)",
                     "v_cmp_f64+v_cndmask_b32")

    def issue_rates(self):
        """Shader cycles per wave-instruction and class with four waves on every SIMD (include/rtr_hip_test.h)."""
        out = (C.c_double * len(self.ISSUE_CLASSES))()
        self._chk(test_lib().rtr_test_issue_rates(self._h, out, len(self.ISSUE_CLASSES)))
        return dict(zip(self.ISSUE_CLASSES, [float(x) for x in out]))

    def shared_division_exhaustive(self):
        """2^32 operand pairs: (how many quotients of the shared-reciprocal division differ from n / d, how many pairs the
        kernel compared) (include/rtr_hip_test.h)."""
        n, tested = C.c_uint64(0), C.c_uint64(0)
        self._chk(test_lib().rtr_test_shared_division(self._h, C.byref(n), C.byref(tested)))
        return int(n.value), int(tested.value)

    def udiv_mismatches(self, numerators, divisors):
        """rtr_test_udiv (include/rtr_hip_test.h): every numerator over every divisor through udiv and through n / d; (how
        many quotients differ in any bit, how many pairs were compared)."""
        num = np.ascontiguousarray(numerators, dtype=np.float64).ravel()
        div = np.ascontiguousarray(divisors, dtype=np.float64).ravel()
        n, tested = C.c_uint64(0), C.c_uint64(0)
        self._chk(test_lib().rtr_test_udiv(self._h, num.ctypes.data, len(num), div.ctypes.data, len(div), C.byref(n),
                                           C.byref(tested)))
        return int(n.value), int(tested.value)

    def lane_mismatches(self, op):
        """rtr_test_rcp_lane / _sqrt_lane (include/rtr_hip_test.h; ``op`` one of LANE_OPS): (operands whose result differs
        from the compiler's, operands compared, operands in waves that voted for the short form, a mismatch as four uint64:
        operand, 0, result, expected)."""
        n, tested, short = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        first = np.zeros(4, dtype=np.uint64)
        fn = getattr(test_lib(), "rtr_test_%s_lane" % op)
        self._chk(fn(self._h, C.byref(n), C.byref(tested), C.byref(short), first.ctypes.data))
        return int(n.value), int(tested.value), int(short.value), first

    def scene_consts(self):
        """rtr_test_scene_consts (include/rtr_hip_test.h): the uploaded scene's table of shading constants and its second
        evaluation by the test library, each as a dict: ``inv_n_lights``, ``pi``, ``rcp_pi`` (and all of it as uint64 bits in
        ``words``), ``lights`` (n, 4) float64 = len2(U), its reciprocal, len2(V), its reciprocal, ``safe`` (n,) int."""
        nl = C.c_int32(0)
        self._chk(test_lib().rtr_test_scene_consts(self._h, None, None, 0, C.byref(nl)))
        words = 4 + 5 * nl.value
        a, b = np.zeros(words, dtype=np.uint64), np.zeros(words, dtype=np.uint64)
        self._chk(test_lib().rtr_test_scene_consts(self._h, a.ctypes.data, b.ctypes.data, words, C.byref(nl)))

        def view(w):
            per = w[4:].reshape(nl.value, 5)
            return {"words": w, "inv_n_lights": float(w[:1].view(np.float64)[0]), "pi": float(w[2:3].view(np.float64)[0]), "rcp_pi": float(w[3:4].view(np.float64)[0]),
                    "lights": np.ascontiguousarray(per[:, :4]).view(np.float64), "safe": (per[:, 4] & 0xffffffff).astype(np.int64)}
        return view(a), view(b)

    def shared_division_mismatches(self):
        """2^32 operand pairs: how many quotients of the shared-reciprocal division differ from n / d (include/rtr_hip_test.h)."""
        return self.shared_division_exhaustive()[0]

    def temporal_planes(self, color, q, count, feat, hist, have, cam, prev, image_size, origin, params=None, c=None, var=None):
        """rtr_test_temporal_planes (include/rtr_hip_test.h): the temporal kernels alone over host planes of a region at
        ``origin`` = (x0, y0) of an image of ``image_size`` = (W, H) -- planes as ``denoise_host`` takes them, ``hist`` (H, W,
        10) as ``History.planes`` returns it, cameras as ``set_camera`` takes them.  Returns (c' (H, W, 3), var' (H, W),
        the history written (H, W, 10)); pixels with count 0 keep the values of ``c`` and ``var`` (zeros if not given)."""
        color = np.ascontiguousarray(color, dtype=np.float64)
        h, w = color.shape[:2]
        q = np.ascontiguousarray(q, dtype=np.float64)
        count = np.ascontiguousarray(count, dtype=np.int32)
        feat = np.ascontiguousarray(feat, dtype=np.float64)
        hist = np.ascontiguousarray(hist, dtype=np.float64)
        if (color.shape != (h, w, 3) or q.shape != (h, w) or count.shape != (h, w) or feat.shape != (h, w, A.FEATURES)
                or hist.shape != (h, w, 10)):
            raise ValueError("planes of shapes (H, W, 3), (H, W), (H, W), (H, W, 7), (H, W, 10) expected")
        c = np.zeros((h, w, 3)) if c is None else np.array(c, dtype=np.float64, order="C")
        var = np.zeros((h, w)) if var is None else np.array(var, dtype=np.float64, order="C")
        if c.shape != (h, w, 3) or var.shape != (h, w):
            raise ValueError("c of shape (H, W, 3) and var of shape (H, W) expected")
        new = np.zeros((h, w, 10))
        tp = params if params is not None else temporal_defaults()
        cc, pc = camera_struct(cam), camera_struct(prev)
        self._chk(test_lib().rtr_test_temporal_planes(
            self._h, w, h, int(image_size[0]), int(image_size[1]), int(origin[0]), int(origin[1]), C.byref(cc), C.byref(pc),
            1 if have else 0, C.byref(tp), color.ctypes.data, q.ctypes.data, count.ctypes.data, feat.ctypes.data,
            hist.ctypes.data, c.ctypes.data, var.ctypes.data, new.ctypes.data))
        return c, var, new

    def accum_plan(self, count, err, tile_s1, mode, spp=0, spp_min=1, spp_max=1, threshold=1.0):
        """rtr_test_accum_plan (include/rtr_hip_test.h): k_accum_plan alone over n tiles.  Returns (targets (n,) int32, the
        active list (n,) int32 with -1 from ``n_active`` on, n_active)."""
        count = np.ascontiguousarray(count, dtype=np.int32)
        err = np.ascontiguousarray(err, dtype=np.float64)
        s1 = np.array(tile_s1, dtype=np.int32, order="C")
        if count.ndim != 1 or err.shape != count.shape or s1.shape != count.shape:
            raise ValueError("count, err and tile_s1 of one shape (n,) expected")
        active = np.full(len(count), -1, dtype=np.int32)
        na = C.c_int32(-1)
        self._chk(test_lib().rtr_test_accum_plan(self._h, len(count), int(mode), int(spp), int(spp_min), int(spp_max),
                                                 float(threshold), count.ctypes.data, err.ctypes.data, s1.ctypes.data,
                                                 active.ctypes.data, C.byref(na)))
        return s1, active, int(na.value)

    def accum_commit(self, active, n_active, done, tile_s1, partial, q_part, sum, q, count):
        """rtr_test_accum_commit (include/rtr_hip_test.h): k_accum_commit alone over n tiles; ``partial`` and ``sum`` (n, 3,
        256), ``q_part`` and ``q`` (n, 256) or both None.  Returns (sum, q, count) after the kernel, as new arrays."""
        ints = [np.ascontiguousarray(a, dtype=np.int32) for a in (active, done, tile_s1)]
        n = len(ints[0])
        partial = np.ascontiguousarray(partial, dtype=np.float64)
        sum_ = np.array(sum, dtype=np.float64, order="C")
        cnt = np.array(count, dtype=np.int32, order="C")
        if any(a.shape != (n,) for a in ints) or cnt.shape != (n,) or partial.shape != (n, 3, 256) or sum_.shape != (n, 3, 256):
            raise ValueError("n tiles: int arrays (n,), partial and sum (n, 3, 256) expected")
        if (q is None) != (q_part is None):
            raise ValueError("q and q_part go together")
        qq = qp = None
        if q is not None:
            qp = np.ascontiguousarray(q_part, dtype=np.float64)
            qq = np.array(q, dtype=np.float64, order="C")
            if qp.shape != (n, 256) or qq.shape != (n, 256):
                raise ValueError("q_part and q of shape (n, 256) expected")
        self._chk(test_lib().rtr_test_accum_commit(
            self._h, n, ints[0].ctypes.data, int(n_active), ints[1].ctypes.data, ints[2].ctypes.data, partial.ctypes.data,
            None if qp is None else qp.ctypes.data, sum_.ctypes.data, None if qq is None else qq.ctypes.data, cnt.ctypes.data))
        return sum_, qq, cnt

    def flat_hits(self, recs, with_uv=True):
        """rtr_test_flat_hits (include/rtr_hip_test.h): ``HIT_DTYPE`` records through the closest-hit cast of the flat
        kernels.  Returns (records, whether the scene has finish records); RtrError where no flat kernel runs the scene."""
        out = np.ascontiguousarray(recs.copy())
        used = C.c_int32(0)
        self._chk(test_lib().rtr_test_flat_hits(self._h, out.ctypes.data, len(out), 1 if with_uv else 0, C.byref(used)))
        return out, bool(used.value)

    def pair_cast(self, ao, ad, bo, bd, a_tmax=np.inf, b_tmax=np.inf, recast=True):
        """rtr_test_pair_cast_text (include/rtr_hip_test.h): trace_pair on n ray pairs ((n, 3) arrays; t_max scalars or (n,))
        next to the two single casts of the flat kernels.  ``recast``: the lean kernels' text (True) or the per-frame
        fallback of the other pair-cast kernels.  Returns the ``PAIR_DTYPE`` records."""
        recs = np.zeros(len(ao), dtype=PAIR_DTYPE)
        recs["ao"], recs["ad"], recs["bo"], recs["bd"] = ao, ad, bo, bd
        recs["a_tmax"], recs["b_tmax"] = a_tmax, b_tmax
        self._chk(test_lib().rtr_test_pair_cast_text(self._h, recs.ctypes.data, len(recs), 1 if recast else 0))
        return recs

    def pair_resident(self, ao, ad, bo, bd, a_tmax=np.inf, b_tmax=np.inf, casts=1):
        """rtr_test_pair_resident (include/rtr_hip_test.h): ``casts`` pair casts of every lane with the job-queue kernel's
        resident shadow request, B parked for the first cast only.  Returns the ``PAIR_DTYPE`` records."""
        recs = np.zeros(len(ao), dtype=PAIR_DTYPE)
        recs["ao"], recs["ad"], recs["bo"], recs["bd"] = ao, ad, bo, bd
        recs["a_tmax"], recs["b_tmax"] = a_tmax, b_tmax
        self._chk(test_lib().rtr_test_pair_resident(self._h, recs.ctypes.data, len(recs), casts))
        return recs

    # device unit kernels over golden-vector records (include/rtr_hip_test.h)
    def test_records(self, kind, recs, params=None, ms=None):
        """kind: "hits", "materials", "scatter", "lights", "li" over their record arrays, or "pow5" over an array of
        doubles.  ms (``MS_LEAN`` / ``MS_FULL`` / ``MS_QUADLIT``; materials, scatter and lights only): the material-set
        instantiation of the kernels; raises RtrError (RTR_ERR_UNSUPPORTED) where the scene is not of that class."""
        out = np.ascontiguousarray(recs.copy())
        if kind == "pow5":
            x = np.ascontiguousarray(recs, dtype=np.float64)
            out = np.zeros_like(x)
            self._chk(test_lib().rtr_test_pow5(self._h, x.ctypes.data, out.ctypes.data, x.size))
            return out
        if ms is not None:
            fn = getattr(test_lib(), "rtr_test_%s_ms" % kind)
            self._chk(fn(self._h, out.ctypes.data, len(out), int(ms)))
            return out
        fn = getattr(test_lib(), "rtr_test_" + kind)
        if kind == "li":
            self._chk(fn(self._h, C.byref(params), out.ctypes.data, len(out)))
        else:
            self._chk(fn(self._h, out.ctypes.data, len(out)))
        return out


class Accumulator:
    """Progressive sample accumulation (include/rtr_hip.h: rtr_accum_*): every owned tile continues its one running
    sum per pixel from its own sample count, so the image after passes ending at T is the bits of
    ``Context.render`` with spp = T and spp_chunks = 1.  Use as a context manager or call ``close()``."""

    def __init__(self, ctx, params, moments=False):
        self._ctx = ctx
        self._L = ctx._L
        self.params = params
        self.moments_kept = bool(moments)
        h = C.c_void_p()
        ctx._chk(self._L.rtr_accum_create_ex(ctx._h, C.byref(params), A.ACCUM_MOMENTS if moments else 0, C.byref(h)))
        self._h = h
        self.shape = (params.y1 - params.y0, params.x1 - params.x0)

    def _handle(self):
        if not self._h:
            raise RtrError(A.RTR_ERR_INVALID, "accumulator closed")
        return self._h

    def render(self, spp_target, blocking=True):
        """One pass: every owned tile continues to ``spp_target`` samples (raises RtrError, RTR_ERR_CANCELLED
        after rtr_cancel: the tiles then hold their old or their new samples)."""
        self._ctx._chk(self._L.rtr_accum_render(self._ctx._h, self._handle(), int(spp_target), 1 if blocking else 0))

    def load_state(self, sum, q, count):
        """rtr_test_accum_load (include/rtr_hip_test.h, the test library): synthetic state into the accumulator -- ``sum``
        (n, 3, 256) and ``q`` (n, 256; None without moments) float64 in the tile layout, every lane given, ``count`` (n,)
        int32, n the owned tiles in the order of ``tiles()``."""
        sum = np.ascontiguousarray(sum, dtype=np.float64)
        count = np.ascontiguousarray(count, dtype=np.int32)
        n = len(count)
        if sum.shape != (n, 3, 256) or count.shape != (n,):
            raise ValueError("sum of shape (n, 3, 256) and count of shape (n,) expected")
        if q is not None:
            q = np.ascontiguousarray(q, dtype=np.float64)
            if q.shape != (n, 256):
                raise ValueError("q of shape (n, 256) expected")
        self._ctx._chk(test_lib().rtr_test_accum_load(self._ctx._h, self._handle(), sum.ctypes.data,
                                                      None if q is None else q.ctypes.data, count.ctypes.data, n))

    def _out(self, out, dtype):
        h, w = self.shape
        if out is None:
            return np.zeros((h, w, 3), dtype=dtype)
        if out.shape != (h, w, 3) or out.dtype != dtype or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous %s array of shape (%d, %d, 3)" % (np.dtype(dtype).name, h, w))
        return out

    def resolve(self, out=None):
        """Linear mean radiance (H, W, 3) float64 of the region, row 0 = its lowest row; pixels of tiles this
        accumulator does not own or that hold no sample keep the values of ``out``."""
        out = self._out(out, np.float64)
        self._ctx._chk(self._L.rtr_accum_resolve(self._ctx._h, self._handle(), out.ctypes.data, self.shape[1], None))
        return out

    def rgb8(self, out=None):
        """The bytes ``RenderBuffer.to_rgb8()`` gives for the region (Y flipped: row 0 = its top row), (H, W, 3)
        uint8; pixels of tiles not owned or without samples keep the values of ``out``."""
        out = self._out(out, np.uint8)
        self._ctx._chk(self._L.rtr_accum_resolve(self._ctx._h, self._handle(), None, 0, out.ctypes.data))
        return out

    def tiles(self):
        """(tile ids in the reference's dispatch numbering, samples per tile) as two int32 arrays."""
        n = C.c_int64(0)
        self._ctx._chk(self._L.rtr_accum_tiles(self._ctx._h, self._handle(), None, None, 0, C.byref(n)))
        ids = np.zeros(n.value, dtype=np.int32)
        counts = np.zeros(n.value, dtype=np.int32)
        self._ctx._chk(self._L.rtr_accum_tiles(self._ctx._h, self._handle(), ids.ctypes.data, counts.ctypes.data,
                                               n.value, C.byref(n)))
        return ids, counts

    def render_tiles(self, targets, blocking=True):
        """One pass with a target per owned tile, in the order of ``tiles()`` (rtr_accum_render_tiles)."""
        t = np.ascontiguousarray(targets, dtype=np.int32)
        self._ctx._chk(self._L.rtr_accum_render_tiles(self._ctx._h, self._handle(), t.ctypes.data, len(t),
                                                      1 if blocking else 0))

    def moments(self, out=None):
        """The raw second moments Q = sum of y * y over the samples, (H, W) float64 like ``resolve``; pixels of tiles
        not owned or without samples keep the values of ``out``."""
        h, w = self.shape
        if out is None:
            out = np.zeros((h, w), dtype=np.float64)
        elif out.shape != (h, w) or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float64 array of shape (%d, %d)" % (h, w))
        self._ctx._chk(self._L.rtr_accum_moments(self._ctx._h, self._handle(), out.ctypes.data, w))
        return out

    def errors(self):
        """The error estimate of every owned tile (include/rtr_hip.h), float64 in the order of ``tiles()``."""
        n = C.c_int64(0)
        self._ctx._chk(self._L.rtr_accum_errors(self._ctx._h, self._handle(), None, 0, C.byref(n)))
        err = np.zeros(n.value, dtype=np.float64)
        self._ctx._chk(self._L.rtr_accum_errors(self._ctx._h, self._handle(), err.ctypes.data, n.value, C.byref(n)))
        return err

    def refine(self, threshold, spp_min, spp_max, blocking=True):
        """One refinement pass decided on the device (rtr_accum_refine): tiles below ``spp_min`` go there, tiles whose
        error is above ``threshold`` double their samples up to ``spp_max``, the others stop.  Returns the number of
        tiles refined (0: done), or -1 when not blocking."""
        n = C.c_int32(-1)
        self._ctx._chk(self._L.rtr_accum_refine(self._ctx._h, self._handle(), float(threshold), int(spp_min),
                                                int(spp_max), 1 if blocking else 0, C.byref(n)))
        return int(n.value)

    def features(self, feature_spp, out=None):
        """First-hit features of ``feature_spp`` camera samples per pixel (rtr_accum_features), (H, W, 7) float64 like
        ``resolve``: albedo 0..2, normal 3..5, depth 6; pixels of tiles not owned keep the values of ``out``."""
        h, w = self.shape
        if out is None:
            out = np.zeros((h, w, A.FEATURES), dtype=np.float64)
        elif out.shape != (h, w, A.FEATURES) or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float64 array of shape (%d, %d, %d)" % (h, w, A.FEATURES))
        self._ctx._chk(self._L.rtr_accum_features(self._ctx._h, self._handle(), int(feature_spp), out.ctypes.data, w))
        return out

    def denoise(self, params=None, rgb8=False, out=None):
        """The denoised image (rtr_accum_denoise; ``params``: an rtr_denoise_params, default ``denoise_defaults()``):
        linear (H, W, 3) float64 like ``resolve``, or with ``rgb8`` the bytes of ``rgb8()``.  Pixels of tiles without
        samples keep the values of ``out``.  Needs an accumulator with moments and every tile of its region."""
        prm = params if params is not None else denoise_defaults()
        if rgb8:
            out = self._out(out, np.uint8)
            self._ctx._chk(self._L.rtr_accum_denoise(self._ctx._h, self._handle(), C.byref(prm), None, 0, out.ctypes.data))
        else:
            out = self._out(out, np.float64)
            self._ctx._chk(self._L.rtr_accum_denoise(self._ctx._h, self._handle(), C.byref(prm), out.ctypes.data,
                                                     self.shape[1], None))
        return out

    def reset(self, seed):
        """rtr_accum_reset: every owned tile back to 0 samples, cached features dropped, bound to the context's current
        camera, with a new seed -- afterwards indistinguishable from a fresh accumulator created with ``seed``."""
        self._ctx._chk(self._L.rtr_accum_reset(self._ctx._h, self._handle(), int(seed) & 0xFFFFFFFF))
        self.params.seed = int(seed) & 0xFFFFFFFF

    def denoise_temporal(self, history, params=None, temporal=None, rgb8=False, out=None):
        """``denoise`` with ``history`` (a ``History`` of the same region) reprojected and blended in before the filter
        (rtr_accum_denoise_temporal; ``temporal``: an rtr_temporal_params, default ``temporal_defaults()``).  The
        history then holds this frame, whichever output was asked for."""
        prm = params if params is not None else denoise_defaults()
        tp = temporal if temporal is not None else temporal_defaults()
        out = self._out(out, np.uint8 if rgb8 else np.float64)
        self._ctx._chk(self._L.rtr_accum_denoise_temporal(
            self._ctx._h, self._handle(), history._handle(), C.byref(prm), C.byref(tp), None if rgb8 else out.ctypes.data,
            0 if rgb8 else self.shape[1], out.ctypes.data if rgb8 else None))
        return out

    # device outputs (include/rtr_hip.h: rtr_accum_*_device): raw device pointers, e.g. a torch tensor's ``data_ptr()``,
    # on the context stream behind what is queued there -- a non-blocking ``render`` included.  Which pixels are written
    # is decided on the device: pixels of tiles without samples (or not owned) keep what the buffers hold.
    def resolve_into(self, linear_ptr, row_stride, rgb8_ptr=None, blocking=False):
        """rtr_accum_resolve_device: ``resolve`` into ``linear_ptr`` (doubles, ``row_stride`` pixels from row to row) and /
        or ``rgb8`` into ``rgb8_ptr`` (bytes, rows of the region's width, top row first); either may be None."""
        self._ctx._chk(self._L.rtr_accum_resolve_device(self._ctx._h, self._handle(), C.c_void_p(linear_ptr or None),
                                                        int(row_stride), C.c_void_p(rgb8_ptr or None), 1 if blocking else 0))

    def features_into(self, feature_spp, feat_ptr, row_stride, blocking=False):
        """rtr_accum_features_device: ``features`` into ``feat_ptr``, 7 doubles per pixel, ``row_stride`` pixels per row."""
        self._ctx._chk(self._L.rtr_accum_features_device(self._ctx._h, self._handle(), int(feature_spp),
                                                         C.c_void_p(feat_ptr or None), int(row_stride), 1 if blocking else 0))

    def denoise_into(self, linear_ptr, row_stride, rgb8_ptr=None, params=None, blocking=False):
        """rtr_accum_denoise_device: ``denoise`` into the buffers of ``resolve_into``."""
        prm = params if params is not None else denoise_defaults()
        self._ctx._chk(self._L.rtr_accum_denoise_device(self._ctx._h, self._handle(), C.byref(prm), C.c_void_p(linear_ptr or None),
                                                        int(row_stride), C.c_void_p(rgb8_ptr or None), 1 if blocking else 0))

    def denoise_temporal_into(self, history, linear_ptr, row_stride, rgb8_ptr=None, params=None, temporal=None, blocking=False):
        """rtr_accum_denoise_temporal_device: ``denoise_temporal`` into the buffers of ``resolve_into``.  The cameras are
        taken at the call and the history advances when it returns: frames may be queued one behind the other."""
        prm = params if params is not None else denoise_defaults()
        tp = temporal if temporal is not None else temporal_defaults()
        self._ctx._chk(self._L.rtr_accum_denoise_temporal_device(
            self._ctx._h, self._handle(), history._handle(), C.byref(prm), C.byref(tp), C.c_void_p(linear_ptr or None),
            int(row_stride), C.c_void_p(rgb8_ptr or None), 1 if blocking else 0))

    def close(self):
        if getattr(self, "_h", None):
            self._L.rtr_accum_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class History:
    """The last frame of ``Accumulator.denoise_temporal`` (include/rtr_hip.h: rtr_history_*): per pixel of the region 10
    doubles and the camera they were seen from.  Use as a context manager or call ``close()``."""

    def __init__(self, ctx, params):
        self._ctx = ctx
        self._L = ctx._L
        h = C.c_void_p()
        ctx._chk(self._L.rtr_history_create(ctx._h, C.byref(params), C.byref(h)))
        self._h = h
        self.shape = (params.y1 - params.y0, params.x1 - params.x0)

    def _handle(self):
        if not self._h:
            raise RtrError(A.RTR_ERR_INVALID, "history closed")
        return self._h

    def clear(self):
        """Forget everything: the next frame has no history."""
        self._ctx._chk(self._L.rtr_history_clear(self._ctx._h, self._handle()))

    def planes(self, out=None):
        """What the next frame will read, (H, W, 10) float64, row 0 = the lowest row: demodulated colour 0..2, mu1 3,
        mu2 4, effective sample count 5 (0: no history), depth 6, normal 7..9."""
        h, w = self.shape
        if out is None:
            out = np.zeros((h, w, A.HISTORY), dtype=np.float64)
        elif out.shape != (h, w, A.HISTORY) or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float64 array of shape (%d, %d, %d)" % (h, w, A.HISTORY))
        self._ctx._chk(self._L.rtr_history_planes(self._ctx._h, self._handle(), out.ctypes.data, w))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._L.rtr_history_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
