"""MI355X-native path tracer behind the reference's ``Renderer::render`` boundary.

The directory name carries a hyphen (it mirrors the upstream repository name), so import it
with ``importlib.import_module("ray_tracing-rendering_amd")``.

Layout:
  csrc/      hand-written HIP kernels (gfx950: register-resident megakernel, wavefront stages) + the C ABI of
             include/rtr_hip.h -> librtr_hip.so
  host/      C++ host layer mirroring the reference's scene-description API + flattening
  scene.py   flattened scene container / .rtrs files
  native.py  ctypes binding of librtr_hip.so (fails loudly when the library is missing)
  renderer.py  Renderer / RenderBuffer mirror of renderer/renderer.h, tile sharding across ranks
"""
from . import _abi  # noqa: F401
from ._abi import (INTEGRATOR_MIS, INTEGRATOR_RR, PIPELINE_AUTO, PIPELINE_MEGAKERNEL,  # noqa: F401
                   PIPELINE_WAVEFRONT, RAY_DTYPE, RAY_HIT_DTYPE, GATHER_POINT_DTYPE, GATHER_OUT_DTYPE, make_params)
from .scene import Scene  # noqa: F401


def __getattr__(name):
    # device-facing pieces are imported lazily so CPU-only tooling can use Scene / _abi
    if name in ("native", "renderer", "hostscene", "build"):
        import importlib
        return importlib.import_module(__name__ + "." + name)
    if name in ("Context", "RtrError", "library_path", "denoise_defaults", "denoise_host", "temporal_defaults",
                "History", "display_defaults", "srgb_thresholds", "gather_defaults", "gather_rays",
                "probe_rays", "sh_basis", "sh_irradiance", "probe_grid", "capture_defaults", "capture_ray", "capture_rays",
                "cube_lookup_host", "latlong_direction", "cube_to_latlong", "write_rgbe", "cube_filter_defaults",
                "cube_filter_host", "cube_chain_plan", "cube_chain_lookup_host", "cube_queries", "brdf_table_host",
                "brdf_fetch_one", "shade_env", "shade_queries", "shade_ibl_one", "capture_set", "capture_queries",
                "capture_set_lookup_host", "shade_ibl_set_one"):
        from . import native
        return getattr(native, name)
    if name in ("Renderer", "RenderBuffer", "ProbeGrid", "Cubemap", "CubeChain", "CaptureSet", "BrdfTable", "IblEnvironment", "render_sharded", "tiles_of_rank", "gather_tiles", "pack_tiles", "unpack_tiles"):
        from . import renderer
        return getattr(renderer, name)
    raise AttributeError(name)
