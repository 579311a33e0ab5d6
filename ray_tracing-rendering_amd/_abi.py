"""ctypes / numpy mirrors of the C ABI in ``include/rtr_hip.h`` and of the golden-vector
records in ``include/rtr_testrec.h``.  Pure layout: no device code, no oracle."""
import ctypes as C

import numpy as np

RTR_ABI_VERSION = 4  # 4: the accumulator entry points rtr_accum_* (include/rtr_hip.h)

# status codes (rtr_status)
RTR_OK = 0
RTR_ERR_INVALID = -1
RTR_ERR_UNSUPPORTED = -2
RTR_ERR_DEVICE = -3
RTR_ERR_NO_SCENE = -4
RTR_ERR_CANCELLED = -5
RTR_ERR_NOMEM = -6

# node / material / texture / light tags
(NODE_BVH, NODE_LIST, NODE_TRANSLATE, NODE_ROTATE_Y, NODE_FLIP_FACE, NODE_MEDIUM, NODE_SPHERE,
 NODE_MOVING_SPHERE, NODE_XY_RECT, NODE_XZ_RECT, NODE_YZ_RECT) = range(11)
MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_DIFFUSE_LIGHT, MAT_PBR, MAT_ISOTROPIC = range(6)
TEX_SOLID, TEX_CHECKER, TEX_NOISE, TEX_IMAGE = range(4)
LIGHT_QUAD, LIGHT_POINT, LIGHT_SPOT, LIGHT_DIRECTIONAL, LIGHT_ENV_UNIFORM, LIGHT_ENV_MAP = 0, 1, 2, 3, 4, 5

INTEGRATOR_PATH, INTEGRATOR_RR, INTEGRATOR_PBR, INTEGRATOR_NEE, INTEGRATOR_MIS = 0, 1, 2, 3, 4
PIPELINE_AUTO, PIPELINE_MEGAKERNEL, PIPELINE_WAVEFRONT = 0, 1, 2
FLAG_REFERENCE_ORDER = 1
FLAG_WF_PERSISTENT = 2
FLAG_SORTED_SHADING = 4
FLAG_SPLIT_CASTS = 8
FLAG_STATIC_GRID = 16
ACCUM_MOMENTS = 1  # rtr_accum_create_ex: keep per-pixel second moments (adaptive sampling)

NODE_DTYPE = np.dtype([("type", "<i4"), ("a", "<i4"), ("b", "<i4"), ("reserved", "<i4"), ("f", "<f8", (10,))])
MATERIAL_DTYPE = np.dtype([("type", "<i4"), ("tex", "<i4", (4,)), ("reserved", "<i4", (3,)), ("f", "<f8", (4,))])
TEXTURE_DTYPE = np.dtype([("type", "<i4"), ("a", "<i4"), ("b", "<i4"), ("reserved", "<i4"), ("f", "<f8", (4,))])
PERLIN_DTYPE = np.dtype([("ranvec", "<f8", (256, 3)), ("perm_x", "<i4", (256,)), ("perm_y", "<i4", (256,)),
                         ("perm_z", "<i4", (256,))])
IMAGE_DTYPE = np.dtype([("width", "<i4"), ("height", "<i4"), ("offset", "<u8")])
LIGHT_DTYPE = np.dtype([("type", "<i4"), ("reserved", "<i4"), ("f", "<f8", (16,))])
CAMERA_DTYPE = np.dtype([("origin", "<f8", (3,)), ("lower_left_corner", "<f8", (3,)), ("horizontal", "<f8", (3,)),
                         ("vertical", "<f8", (3,)), ("u", "<f8", (3,)), ("v", "<f8", (3,)), ("w", "<f8", (3,)),
                         ("lens_radius", "<f8"), ("time0", "<f8"), ("time1", "<f8")])
assert NODE_DTYPE.itemsize == 96 and MATERIAL_DTYPE.itemsize == 64 and TEXTURE_DTYPE.itemsize == 48
assert PERLIN_DTYPE.itemsize == 9216 and IMAGE_DTYPE.itemsize == 16 and LIGHT_DTYPE.itemsize == 136
assert CAMERA_DTYPE.itemsize == 192
LI_RAY_DTYPE = np.dtype([("origin", "<f8", (3,)), ("direction", "<f8", (3,)), ("time", "<f8"), ("rng_state", "<u4"),
                         ("pad", "<u4")])  # rtr_li_ray
assert LI_RAY_DTYPE.itemsize == 64
# ray queries (rtr_query_*): rtr_ray in, rtr_ray_hit out
RAY_DTYPE = np.dtype([("origin", "<f8", (3,)), ("direction", "<f8", (3,)), ("time", "<f8"), ("t_min", "<f8"),
                      ("t_max", "<f8"), ("rng_state", "<u4"), ("pad", "<u4")])
RAY_HIT_DTYPE = np.dtype([("t", "<f8"), ("p", "<f8", (3,)), ("n", "<f8", (3,)), ("u", "<f8"), ("v", "<f8"),
                          ("hit", "<i4"), ("front_face", "<i4"), ("material", "<i4"), ("rng_out", "<u4")])
assert RAY_DTYPE.itemsize == 80 and RAY_HIT_DTYPE.itemsize == 88
# hemisphere gathers (rtr_gather_*): rtr_gather_point in, rtr_gather_out out
GATHER_POINT_DTYPE = np.dtype([("p", "<f8", (3,)), ("n", "<f8", (3,))])
GATHER_OUT_DTYPE = np.dtype([("v", "<f8", (3,)), ("count", "<i4"), ("valid", "<i4")])
assert GATHER_POINT_DTYPE.itemsize == 48 and GATHER_OUT_DTYPE.itemsize == 32
GATHER_MAX_SAMPLES = 1 << 20
# light probes (rtr_probe_*): rtr_probe_point in, rtr_probe_vis / rtr_probe_sh out
PROBE_POINT_DTYPE = np.dtype([("p", "<f8", (3,))])
PROBE_VIS_DTYPE = np.dtype([("c", "<f8", (9,)), ("count", "<i4"), ("valid", "<i4")])
PROBE_SH_DTYPE = np.dtype([("c", "<f8", (9, 3)), ("count", "<i4"), ("valid", "<i4")])
assert PROBE_POINT_DTYPE.itemsize == 24 and PROBE_VIS_DTYPE.itemsize == 80 and PROBE_SH_DTYPE.itemsize == 224
PROBE_GRID_MAX = 1 << 24
CAPTURE_MAX_FACE = 4096  # rtr_capture_cube / rtr_cube_lookup: the largest face_size

# golden-vector records (rtr_testrec.h, packed)
LI_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("s", "<i4"), ("rng_exit", "<u4"), ("L", "<f8", (3,)),
                     ("n_closest", "<i4"), ("n_shadow", "<i4")])
HIT_DTYPE = np.dtype([("o", "<f8", (3,)), ("d", "<f8", (3,)), ("time", "<f8"), ("t_min", "<f8"), ("t_max", "<f8"),
                      ("rng_in", "<u4"), ("rng_out", "<u4"), ("hit", "<i4"), ("front_face", "<i4"),
                      ("material", "<i4"), ("pad", "<i4"), ("t", "<f8"), ("p", "<f8", (3,)), ("n", "<f8", (3,)),
                      ("u", "<f8"), ("v", "<f8")])
MAT_DTYPE = np.dtype([("material", "<i4"), ("front_face", "<i4"), ("rng_in", "<u4"), ("rng_out", "<u4"),
                      ("p", "<f8", (3,)), ("n", "<f8", (3,)), ("u", "<f8"), ("v", "<f8"), ("wo", "<f8", (3,)),
                      ("wi_in", "<f8", (3,)), ("sample_ok", "<i4"), ("is_specular", "<i4"),
                      ("is_transmission", "<i4"), ("pad", "<i4"), ("s_wi", "<f8", (3,)), ("s_f", "<f8", (3,)),
                      ("s_pdf", "<f8"), ("eval", "<f8", (3,)), ("pdf", "<f8"), ("emitted", "<f8", (3,))])
LIGHTREC_DTYPE = np.dtype([("light", "<i4"), ("pad", "<i4"), ("p", "<f8", (3,)), ("u", "<f8", (2,)),
                           ("dir", "<f8", (3,)), ("Li", "<f8", (3,)), ("wi", "<f8", (3,)), ("pdf", "<f8"),
                           ("dist", "<f8"), ("is_delta", "<i4"), ("pad2", "<i4"), ("pdf_dir", "<f8")])
assert LI_DTYPE.itemsize == 48 and HIT_DTYPE.itemsize == 168 and MAT_DTYPE.itemsize == 256
assert LIGHTREC_DTYPE.itemsize == 152
RNG_BLOCK_DOUBLES = 1 + 16 + 8 + 3 + 2 + 3 + 3 + 3 + 3 + 1


class CameraC(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("lower_left_corner", C.c_double * 3), ("horizontal", C.c_double * 3),
                ("vertical", C.c_double * 3), ("u", C.c_double * 3), ("v", C.c_double * 3), ("w", C.c_double * 3),
                ("lens_radius", C.c_double), ("time0", C.c_double), ("time1", C.c_double)]


class SceneDescC(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("root", C.c_int32), ("n_nodes", C.c_int32),
                ("n_list_children", C.c_int32), ("n_materials", C.c_int32), ("n_textures", C.c_int32),
                ("n_perlin", C.c_int32), ("n_images", C.c_int32), ("n_lights", C.c_int32), ("reserved", C.c_int32),
                ("n_image_bytes", C.c_uint64), ("nodes", C.c_void_p), ("list_children", C.c_void_p),
                ("materials", C.c_void_p), ("textures", C.c_void_p), ("perlin", C.c_void_p),
                ("images", C.c_void_p), ("image_bytes", C.c_void_p), ("lights", C.c_void_p),
                ("camera", CameraC), ("background", C.c_double * 3)]


class RenderParamsC(C.Structure):
    _fields_ = [("image_width", C.c_int32), ("image_height", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32),
                ("x1", C.c_int32), ("y1", C.c_int32), ("spp", C.c_int32), ("max_depth", C.c_int32),
                ("rr_start_depth", C.c_int32), ("integrator", C.c_int32), ("seed", C.c_uint32),
                ("pipeline", C.c_int32), ("tile_first", C.c_int32), ("tile_stride", C.c_int32),
                ("spp_chunks", C.c_int32), ("flags", C.c_int32)]


class RenderStatsC(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("closest_segments", C.c_uint64), ("shadow_segments", C.c_uint64),
                ("device_ms", C.c_double), ("kernel_launches", C.c_int32), ("pipeline", C.c_int32),
                ("spp_chunks", C.c_int32), ("cancelled", C.c_int32), ("flags_in_effect", C.c_int32),
                ("reserved", C.c_int32)]


class RayC(C.Structure):
    """rtr_ray (include/rtr_hip.h): one ray of rtr_query_*"""
    _fields_ = [("origin", C.c_double * 3), ("direction", C.c_double * 3), ("time", C.c_double), ("t_min", C.c_double),
                ("t_max", C.c_double), ("rng_state", C.c_uint32), ("pad", C.c_uint32)]


class RayHitC(C.Structure):
    """rtr_ray_hit (include/rtr_hip.h): the hit record of rtr_query_closest"""
    _fields_ = [("t", C.c_double), ("p", C.c_double * 3), ("n", C.c_double * 3), ("u", C.c_double), ("v", C.c_double),
                ("hit", C.c_int32), ("front_face", C.c_int32), ("material", C.c_int32), ("rng_out", C.c_uint32)]


assert C.sizeof(RayC) == RAY_DTYPE.itemsize and C.sizeof(RayHitC) == RAY_HIT_DTYPE.itemsize


class GatherParamsC(C.Structure):
    """rtr_gather_params (include/rtr_hip.h): the hemisphere gathers rtr_gather_occlusion / rtr_gather_radiance"""
    _fields_ = [("samples", C.c_int32), ("seed", C.c_uint32), ("point_base", C.c_uint32), ("flags", C.c_int32),
                ("time", C.c_double), ("t_min", C.c_double), ("t_max", C.c_double), ("reserved", C.c_double * 2)]


GATHER_PARAMS_SIZE = 56
assert C.sizeof(GatherParamsC) == GATHER_PARAMS_SIZE


class ProbeGridC(C.Structure):
    """rtr_probe_grid (include/rtr_hip.h): the regular grid of rtr_probe_lookup"""
    _fields_ = [("origin", C.c_double * 3), ("spacing", C.c_double * 3), ("dims", C.c_int32 * 3), ("pad", C.c_int32)]


PROBE_GRID_SIZE = 64
assert C.sizeof(ProbeGridC) == PROBE_GRID_SIZE


class ProbeDepthParamsC(C.Structure):
    """rtr_probe_depth_params (include/rtr_hip.h): the distance maps of rtr_probe_depth"""
    _fields_ = [("map_size", C.c_int32), ("samples", C.c_int32), ("seed", C.c_uint32), ("point_base", C.c_uint32),
                ("jitter", C.c_int32), ("pad", C.c_int32), ("time", C.c_double), ("t_min", C.c_double), ("t_max", C.c_double)]


class ProbeVisibleParamsC(C.Structure):
    """rtr_probe_visible_params (include/rtr_hip.h): the visibility-weighted grid lookup rtr_probe_lookup_visible"""
    _fields_ = [("map_size", C.c_int32), ("pad", C.c_int32), ("normal_bias", C.c_double), ("reserved", C.c_double * 2)]


PROBE_DEPTH_PARAMS_SIZE, PROBE_VISIBLE_PARAMS_SIZE = 48, 32
assert C.sizeof(ProbeDepthParamsC) == PROBE_DEPTH_PARAMS_SIZE and C.sizeof(ProbeVisibleParamsC) == PROBE_VISIBLE_PARAMS_SIZE
# rtr_probe_depth_texel: one texel of a probe's octahedral distance map
PROBE_DEPTH_DTYPE = np.dtype([("mean", "<f8"), ("mean2", "<f8"), ("hits", "<i4"), ("back", "<i4"), ("valid", "<i4"),
                              ("pad", "<i4")])
assert PROBE_DEPTH_DTYPE.itemsize == 32
PROBE_DEPTH_MAX_MAP = 64


class CaptureParamsC(C.Structure):
    """rtr_capture_params (include/rtr_hip.h): the environment captures of rtr_capture_cube"""
    _fields_ = [("face_size", C.c_int32), ("samples", C.c_int32), ("seed", C.c_uint32), ("point_base", C.c_uint32),
                ("jitter", C.c_int32), ("pad", C.c_int32), ("time", C.c_double), ("reserved", C.c_double * 2)]


CAPTURE_PARAMS_SIZE = 48
assert C.sizeof(CaptureParamsC) == CAPTURE_PARAMS_SIZE


class CubeFilterParamsC(C.Structure):
    """rtr_cube_filter_params (include/rtr_hip.h): one GGX-filtered level of rtr_cube_filter"""
    _fields_ = [("face_in", C.c_int32), ("face_out", C.c_int32), ("alpha", C.c_double), ("cos_cut", C.c_double),
                ("pad", C.c_int32 * 2)]


class CubeLevelC(C.Structure):
    """rtr_cube_level (include/rtr_hip.h): one level of a chain of filtered cubes"""
    _fields_ = [("face_size", C.c_int32), ("pad", C.c_int32), ("offset", C.c_int64), ("alpha", C.c_double)]


CUBE_FILTER_PARAMS_SIZE, CUBE_LEVEL_SIZE = 32, 24
assert C.sizeof(CubeFilterParamsC) == CUBE_FILTER_PARAMS_SIZE and C.sizeof(CubeLevelC) == CUBE_LEVEL_SIZE
CUBE_QUERY_DTYPE = np.dtype([("d", "<f8", (3,)), ("alpha", "<f8")])  # rtr_cube_query
assert CUBE_QUERY_DTYPE.itemsize == 32
CUBE_FILTER_MAX_FACE, CUBE_CHAIN_MAX_LEVELS = 512, 13


class BrdfParamsC(C.Structure):
    """rtr_brdf_params (include/rtr_hip.h): the environment BRDF table of rtr_brdf_table"""
    _fields_ = [("n_mu", C.c_int32), ("n_rough", C.c_int32), ("nodes", C.c_int32), ("pad", C.c_int32),
                ("reserved", C.c_double * 2)]


class ShadeEnvC(C.Structure):
    """rtr_shade_env (include/rtr_hip.h): what rtr_shade_ibl shades under; every pointer member is a c_void_p"""
    _fields_ = [("parts", C.c_int32), ("n_levels", C.c_int32), ("grid", C.c_void_p), ("probes", C.c_void_p),
                ("depth", C.c_void_p), ("visible", C.c_void_p), ("levels", C.c_void_p), ("chain", C.c_void_p),
                ("n_records", C.c_int64), ("table", C.c_void_p), ("n_mu", C.c_int32), ("n_rough", C.c_int32)]


BRDF_PARAMS_SIZE, SHADE_ENV_SIZE = 32, 80
assert C.sizeof(BrdfParamsC) == BRDF_PARAMS_SIZE and C.sizeof(ShadeEnvC) == SHADE_ENV_SIZE
BRDF_ENTRY_DTYPE = np.dtype([("a", "<f8"), ("b", "<f8")])  # rtr_brdf_entry
SHADE_QUERY_DTYPE = np.dtype([("p", "<f8", (3,)), ("n", "<f8", (3,)), ("v", "<f8", (3,)), ("base", "<f8", (3,)),
                              ("roughness", "<f8"), ("metallic", "<f8")])  # rtr_shade_query
assert BRDF_ENTRY_DTYPE.itemsize == 16 and SHADE_QUERY_DTYPE.itemsize == 112
BRDF_MAX = 256
SHADE_DIFFUSE, SHADE_SPECULAR = 1, 2


class CaptureVolumeC(C.Structure):
    """rtr_capture_volume (include/rtr_hip.h): where a capture of a set was taken, the box its reflections are projected
    onto, the box of points it serves and the width of the band over which its weight rises"""
    _fields_ = [("centre", C.c_double * 3), ("proxy_lo", C.c_double * 3), ("proxy_hi", C.c_double * 3),
                ("reach_lo", C.c_double * 3), ("reach_hi", C.c_double * 3), ("fade", C.c_double)]


class CaptureSetC(C.Structure):
    """rtr_capture_set (include/rtr_hip.h): 1 .. 16 volumes and the capture read where none reaches (-1: none)"""
    _fields_ = [("n_captures", C.c_int32), ("fallback", C.c_int32), ("volumes", C.c_void_p)]


CAPTURE_VOLUME_SIZE, CAPTURE_SET_SIZE, CAPTURE_SET_MAX = 128, 16, 16
assert C.sizeof(CaptureVolumeC) == CAPTURE_VOLUME_SIZE and C.sizeof(CaptureSetC) == CAPTURE_SET_SIZE
CAPTURE_VOLUME_DTYPE = np.dtype([("centre", "<f8", (3,)), ("proxy_lo", "<f8", (3,)), ("proxy_hi", "<f8", (3,)),
                                 ("reach_lo", "<f8", (3,)), ("reach_hi", "<f8", (3,)), ("fade", "<f8")])  # rtr_capture_volume
CAPTURE_QUERY_DTYPE = np.dtype([("p", "<f8", (3,)), ("d", "<f8", (3,)), ("alpha", "<f8"), ("pad", "<f8")])  # rtr_capture_query
assert CAPTURE_VOLUME_DTYPE.itemsize == 128 and CAPTURE_QUERY_DTYPE.itemsize == 64


class PreviewParamsC(C.Structure):
    """rtr_preview_params (include/rtr_hip.h): a frame shaded from a bake, rtr_preview / rtr_preview_samples"""
    _fields_ = [("image_width", C.c_int32), ("image_height", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32),
                ("x1", C.c_int32), ("y1", C.c_int32), ("grid", C.c_int32), ("flags", C.c_int32), ("t_min", C.c_double),
                ("reserved", C.c_double * 3)]


PREVIEW_PARAMS_SIZE = 64
assert C.sizeof(PreviewParamsC) == PREVIEW_PARAMS_SIZE
PREVIEW_SAMPLE_DTYPE = np.dtype([("q", SHADE_QUERY_DTYPE), ("direct", "<f8", (3,)), ("kind", "<i4"),
                                 ("material", "<i4")])  # rtr_preview_sample
assert PREVIEW_SAMPLE_DTYPE.itemsize == 144
PREVIEW_MISS, PREVIEW_EMITTER, PREVIEW_SURFACE = 0, 1, 2
PREVIEW_MAX_GRID = 8


class DenoiseParamsC(C.Structure):
    """rtr_denoise_params (include/rtr_hip.h): the a-trous denoiser of rtr_accum_denoise / rtr_denoise_host"""
    _fields_ = [("iterations", C.c_int32), ("feature_spp", C.c_int32), ("sigma_l", C.c_double),
                ("sigma_n", C.c_double), ("sigma_a", C.c_double), ("sigma_z", C.c_double), ("reserved", C.c_double * 4)]


DENOISE_PARAMS_SIZE = 72
assert C.sizeof(DenoiseParamsC) == DENOISE_PARAMS_SIZE
FEATURES = 7  # doubles per pixel of rtr_accum_features: albedo 3, normal 3, depth 1


class TemporalParamsC(C.Structure):
    """rtr_temporal_params (include/rtr_hip.h): the reprojection stage of rtr_accum_denoise_temporal"""
    _fields_ = [("alpha_min", C.c_double), ("tau_z", C.c_double), ("tau_n", C.c_double), ("min_weight", C.c_double),
                ("reserved", C.c_double * 4)]


TEMPORAL_PARAMS_SIZE = 64
assert C.sizeof(TemporalParamsC) == TEMPORAL_PARAMS_SIZE
HISTORY = 10  # doubles per pixel of rtr_history_planes: c 3, mu1, mu2, n, z, nn 3


class DisplayParamsC(C.Structure):
    """rtr_display_params (include/rtr_hip.h): the display transform of rtr_display_host / rtr_display_device"""
    _fields_ = [("auto_exposure", C.c_int32), ("meter_permille", C.c_int32), ("tone_curve", C.c_int32),
                ("encoding", C.c_int32), ("exposure", C.c_double), ("key", C.c_double), ("white", C.c_double),
                ("reserved", C.c_double * 5)]


class DisplayResultC(C.Structure):
    """rtr_display_result (include/rtr_hip.h): the scale a display call used and what it metered"""
    _fields_ = [("scale", C.c_double), ("metered", C.c_double), ("n_metered", C.c_int64), ("reserved", C.c_int64)]


DISPLAY_PARAMS_SIZE, DISPLAY_RESULT_SIZE = 80, 32
assert C.sizeof(DisplayParamsC) == DISPLAY_PARAMS_SIZE and C.sizeof(DisplayResultC) == DISPLAY_RESULT_SIZE
TONE_CLAMP, TONE_REINHARD, TONE_ACES = 0, 1, 2
ENCODE_GAMMA2, ENCODE_SRGB = 0, 1
DISPLAY_BINS = 512  # bins of rtr_display_histogram: 16 per octave from 2^-20 to 2^12

# the device forms of the accumulator outputs (include/rtr_hip.h): their argument types in the header's order -- handles
# and device pointers are void pointers, everything returns int
_P, _VP = C.POINTER, C.c_void_p
DEVICE_OUTPUT_SIGNATURES = {
    "rtr_accum_resolve_device": [_VP, _VP, _VP, C.c_int64, _VP, C.c_int],
    "rtr_accum_features_device": [_VP, _VP, C.c_int32, _VP, C.c_int64, C.c_int],
    "rtr_accum_denoise_device": [_VP, _VP, _P(DenoiseParamsC), _VP, C.c_int64, _VP, C.c_int],
    "rtr_accum_denoise_temporal_device": [_VP, _VP, _VP, _P(DenoiseParamsC), _P(TemporalParamsC), _VP, C.c_int64, _VP,
                                          C.c_int],
}


def make_params(width, height, spp, *, integrator=INTEGRATOR_MIS, seed=1, max_depth=50, rr_start_depth=3,
                region=None, pipeline=PIPELINE_AUTO, tile_first=0, tile_stride=1, spp_chunks=1, flags=0):
    """Build an ``rtr_render_params``.  Defaults follow the reference driver (main.cpp:102,
    mis_path_integrator.h:237)."""
    x0, y0, x1, y1 = region if region is not None else (0, 0, width, height)
    p = RenderParamsC()
    p.image_width, p.image_height = int(width), int(height)
    p.x0, p.y0, p.x1, p.y1 = int(x0), int(y0), int(x1), int(y1)
    p.spp, p.max_depth, p.rr_start_depth = int(spp), int(max_depth), int(rr_start_depth)
    p.integrator, p.seed, p.pipeline = int(integrator), int(seed) & 0xFFFFFFFF, int(pipeline)
    p.tile_first, p.tile_stride = int(tile_first), int(tile_stride)
    p.spp_chunks = int(spp_chunks)
    p.flags = int(flags)
    return p
