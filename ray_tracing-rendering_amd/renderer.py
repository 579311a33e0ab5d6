"""Host-side mirror of the reference's ``Renderer`` / ``RenderBuffer``
(renderer/renderer.h:17-142, renderer/render_buffer.h:11-84) on top of the HIP library, and the
multi-GPU tile sharding (one process per GPU, no data-path collective)."""
import itertools

import numpy as np

from . import _abi as A

TILE = 16  # renderer.h:40


class RenderBuffer:
    """``RenderBuffer`` (render_buffer.h:11-33): height x width gamma-space colours, row 0 =
    bottom row.  ``linear`` additionally keeps the linear mean radiance the device produced."""

    def __init__(self, width, height):
        self.width, self.height = int(width), int(height)
        self.pixels = np.zeros((self.height, self.width, 3), dtype=np.float64)
        self.linear = np.zeros_like(self.pixels)

    def get_data(self):
        return self.pixels

    def store_linear(self, linear, region=None):
        """write_color_to_buffer (renderer.h:126-140): sqrt gamma, clamp to [0, 1]."""
        x0, y0, x1, y1 = region if region is not None else (0, 0, self.width, self.height)
        self.linear[y0:y1, x0:x1] = linear
        self.pixels[y0:y1, x0:x1] = np.clip(np.sqrt(linear), 0.0, 1.0)

    def to_rgb8(self):
        """The bytes save_to_png writes (render_buffer.h:35-55): Y flipped, uchar(c * 255) truncation."""
        return (self.pixels[::-1] * 255.0).astype(np.uint8)

    def save_to_png(self, filename, rgb8=None):
        """8-bit RGB PNG with the reference's pixel bytes (render_buffer.h:35-55).  The reference
        encodes with stb_image_write; the zlib stream differs, the decoded pixels do not.  ``rgb8``: write these
        (height, width, 3) uint8 pixels, top row first -- what ``Renderer.display`` returns -- instead of ``to_rgb8()``."""
        import struct
        import zlib
        if rgb8 is None:
            rgb = self.to_rgb8()
        else:
            rgb = np.ascontiguousarray(rgb8)
            if rgb.shape != (self.height, self.width, 3) or rgb.dtype != np.uint8:
                raise ValueError("rgb8 must be a uint8 array of shape (%d, %d, 3)" % (self.height, self.width))
        raw = b"".join(b"\x00" + rgb[j].tobytes() for j in range(self.height))

        def chunk(tag, data):
            return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

        png = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", self.width, self.height, 8, 2, 0, 0, 0)) +
               chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))
        with open(filename, "wb") as f:
            f.write(png)
        return True


def output_filename(scene_id, integrator_id, timestamp=None):
    """``output/sceneNN_integratorK_<unixtime>.png`` (main.cpp:134-142)."""
    import time
    t = int(time.time()) if timestamp is None else int(timestamp)
    return "output/scene%02d_integrator%d_%d.png" % (scene_id, integrator_id, t)


def tiles_of_rank(width, height, rank, world):
    """Tile indices (reference dispatch order, renderer.h:61-62) owned by ``rank`` of ``world``:
    index % world == rank.  The union over ranks is every tile exactly once."""
    tx, ty = (width + TILE - 1) // TILE, (height + TILE - 1) // TILE
    return list(range(rank, tx * ty, world))


def tile_rect(width, height, tile_index):
    tx, ty = (width + TILE - 1) // TILE, (height + TILE - 1) // TILE
    y = (ty - 1) - tile_index // tx
    x = tile_index % tx
    return x * TILE, y * TILE, min(x * TILE + TILE, width), min(y * TILE + TILE, height)


def ownership_mask(width, height, rank, world):
    m = np.zeros((height, width), dtype=bool)
    for t in tiles_of_rank(width, height, rank, world):
        x0, y0, x1, y1 = tile_rect(width, height, t)
        m[y0:y1, x0:x1] = True
    return m


class Renderer:
    """``Renderer`` (renderer.h:17-120) driving one GPU through the C ABI."""

    def __init__(self, device=0, context=None):
        from .native import Context
        self._ctx = context if context is not None else Context(device)
        self._spp = 10          # Settings::samples_per_pixel default (renderer.h:20)
        self._max_depth = 50
        self._integrator = A.INTEGRATOR_MIS
        self.pipeline = A.PIPELINE_AUTO
        self.seed = 1
        self._rendering = False
        self._cancel_requested = False

    def set_integrator(self, integrator_id):
        """Integrator ids of the reference CLI (main.cpp:52): 1 = RR path, 4 = MIS path."""
        self._integrator = int(integrator_id)

    def set_samples(self, samples):
        self._spp = int(samples)

    def set_max_depth(self, depth):
        self._max_depth = int(depth)

    def cancel(self):
        self._cancel_requested = True  # (render_progressive: also between its passes)
        self._ctx.cancel()

    def is_rendering(self):
        return self._rendering

    def render(self, scene, target_buffer, rank=0, world=1):
        """``Renderer::render(world, cam, background, target_buffer, lights)`` with the scene
        already flattened; fills the tiles ``rank`` owns."""
        self._rendering = True
        try:
            self._scene_on_device(scene)
            p = A.make_params(target_buffer.width, target_buffer.height, self._spp, integrator=self._integrator,
                              seed=self.seed, max_depth=self._max_depth, pipeline=self.pipeline, tile_first=rank,
                              tile_stride=world, spp_chunks=0)
            linear = self._ctx.render(p)
            if world > 1:
                own = ownership_mask(target_buffer.width, target_buffer.height, rank, world)
                linear = np.where(own[..., None], linear, target_buffer.linear)
            target_buffer.store_linear(linear)
        finally:
            self._rendering = False
        return target_buffer

    def render_progressive(self, scene, target_buffer, targets, rank=0, world=1, denoise=None):
        """Progressive ``render``: a generator that, for each of the increasing sample counts ``targets``, continues
        the per-pixel sums of the tiles ``rank`` owns to that many samples (one accumulator, include/rtr_hip.h:
        rtr_accum_*), stores the image into ``target_buffer`` and yields the count.  The image at count T is the
        bits of a render with spp = T and spp_chunks = 1.  ``cancel()`` ends it: the buffer then holds the last
        count yielded.  ``denoise`` (an rtr_denoise_params, e.g. ``denoise_defaults()``): the accumulator keeps moments
        and the image stored after the last pass is the denoised one (rtr_accum_denoise; with world > 1 the ranks'
        planes are gathered and passed through rtr_denoise_host).  Bad schedules or denoise parameters raise
        ValueError here, before any device call."""
        targets = [int(t) for t in targets]
        if not targets or targets[0] < 1 or any(b <= a for a, b in zip(targets, targets[1:])):
            raise ValueError("targets must be a non-empty, strictly increasing list of sample counts >= 1: %r" % (targets,))
        check_denoise(denoise)
        self._cancel_requested = False
        return self._progressive(scene, target_buffer, targets, rank, world, denoise)

    def _progressive(self, scene, target_buffer, targets, rank, world, denoise):
        from .native import RtrError
        self._rendering = True
        try:
            self._scene_on_device(scene)
            p = A.make_params(target_buffer.width, target_buffer.height, 1, integrator=self._integrator, seed=self.seed,
                              max_depth=self._max_depth, pipeline=self.pipeline, tile_first=rank, tile_stride=world)
            with self._ctx.accumulator(p, moments=denoise is not None) as acc:
                for t in targets:
                    if self._cancel_requested:
                        return
                    try:
                        acc.render(t)
                    except RtrError as e:
                        if e.code == A.RTR_ERR_CANCELLED:
                            return
                        raise
                    # pixels of tiles other ranks own keep what the buffer holds
                    if denoise is not None and t == targets[-1]:
                        target_buffer.store_linear(self._denoised(acc, denoise, target_buffer, rank, world))
                    else:
                        target_buffer.store_linear(acc.resolve(target_buffer.linear.copy()))
                    yield t
        finally:
            self._rendering = False

    def render_adaptive(self, scene, target_buffer, threshold, spp_min, spp_max, rank=0, world=1, denoise=None):
        """Adaptive ``render``: a generator of refinement passes over the tiles ``rank`` owns (one accumulator with
        second moments, include/rtr_hip.h: rtr_accum_refine).  The first pass takes every tile to ``spp_min`` samples;
        each later one doubles the samples of the tiles whose error estimate is above ``threshold`` (1/255 = one 8-bit
        step of the stored image), up to ``spp_max``.  After each pass the image goes into ``target_buffer`` and
        (pass number from 1, tiles refined, samples rendered so far) is yielded; it ends when no tile is left to refine
        or on ``cancel()``.  A tile holding T samples is the bits of a render with spp = T and spp_chunks = 1.
        ``denoise`` (an rtr_denoise_params): once no tile is left to refine, the buffer takes the denoised image
        (as ``render_progressive``).  Bad arguments raise ValueError here, before any device call."""
        threshold = float(threshold)
        if not threshold > 0.0:
            raise ValueError("threshold must be > 0: %r" % threshold)
        if int(spp_min) != spp_min or int(spp_max) != spp_max or not 1 <= spp_min <= spp_max:
            raise ValueError("need integers 1 <= spp_min <= spp_max: %r, %r" % (spp_min, spp_max))
        check_denoise(denoise)
        self._cancel_requested = False
        return self._adaptive(scene, target_buffer, threshold, int(spp_min), int(spp_max), rank, world, denoise)

    def _adaptive(self, scene, target_buffer, threshold, spp_min, spp_max, rank, world, denoise):
        from .native import RtrError
        self._rendering = True
        try:
            self._scene_on_device(scene)
            p = A.make_params(target_buffer.width, target_buffer.height, 1, integrator=self._integrator, seed=self.seed,
                              max_depth=self._max_depth, pipeline=self.pipeline, tile_first=rank, tile_stride=world)
            total = 0
            with self._ctx.accumulator(p, moments=True) as acc:
                for k in itertools.count(1):
                    if self._cancel_requested:
                        return
                    try:
                        n_active = acc.refine(threshold, spp_min, spp_max)
                    except RtrError as e:
                        if e.code == A.RTR_ERR_CANCELLED:
                            return
                        raise
                    if n_active == 0:
                        if denoise is not None:
                            target_buffer.store_linear(self._denoised(acc, denoise, target_buffer, rank, world))
                        return
                    total += self._ctx.stats()["samples"]
                    target_buffer.store_linear(acc.resolve(target_buffer.linear.copy()))
                    yield k, n_active, total
        finally:
            self._rendering = False

    def render_sequence(self, scene, cameras, target_buffer, spp, seeds=None, denoise=None, temporal=None, rank=0, world=1,
                        display=None):
        """The frames of a moving camera: a generator with ONE upload of ``scene`` and, per camera of ``cameras`` (each
        what ``Context.set_camera`` takes), set_camera, a reset of one accumulator with the frame's seed, a pass to
        ``spp`` samples and the store into ``target_buffer``; yields the frame index once the buffer holds that frame.
        ``seeds``: one per frame (default ``self.seed + frame``; frames sharing a seed share their noise pattern, which a
        temporal blend cannot average away).  ``denoise`` (an rtr_denoise_params) filters each frame; ``temporal`` (an
        rtr_temporal_params; ``denoise`` then defaults to ``denoise_defaults()``) blends the reprojected last frame in
        first (rtr_accum_denoise_temporal) over one history that lives as long as the generator.  Single rank:
        ``world`` > 1 raises ValueError.  Afterwards the context keeps the last camera (``Context.camera_updated``); the
        other render methods of this class put ``scene.camera`` back before they render ``scene``.

        ``display`` (an rtr_display_params): each frame stays on the device -- reset, a non-blocking pass, the device form
        of the resolve or denoise (rtr_accum_*_device) and rtr_display_device are queued on the context stream into
        device buffers the generator owns (torch tensors: import torch before this package, as bench.py does), and only
        the frame's display bytes come back, in one copy.  They are left in ``target_buffer.display_rgb8`` -- (height,
        width, 3) uint8, top row first, for ``target_buffer.save_to_png(filename, rgb8=target_buffer.display_rgb8)``;
        the buffer's ``linear`` and ``pixels`` are not touched.  Without ``display`` nothing changes."""
        from .native import denoise_defaults
        if world != 1 or rank != 0:
            raise ValueError("render_sequence is single rank (a temporal history is not sharded)")
        cameras = list(cameras)
        seeds = [self.seed + k for k in range(len(cameras))] if seeds is None else list(seeds)
        if len(seeds) != len(cameras):
            raise ValueError("one seed per camera expected: %d seeds, %d cameras" % (len(seeds), len(cameras)))
        if int(spp) != spp or spp < 1:
            raise ValueError("spp must be an integer >= 1: %r" % (spp,))
        if temporal is not None and not isinstance(temporal, A.TemporalParamsC):
            raise ValueError("temporal must be None or rtr_temporal_params (temporal_defaults())")
        if temporal is not None and denoise is None:
            denoise = denoise_defaults()
        check_denoise(denoise)
        if display is not None and not isinstance(display, A.DisplayParamsC):
            raise ValueError("display must be None or rtr_display_params (display_defaults())")
        self._cancel_requested = False
        return self._sequence(scene, cameras, target_buffer, int(spp), seeds, denoise, temporal, display)

    def _sequence(self, scene, cameras, target_buffer, spp, seeds, denoise, temporal, display=None):
        from .native import RtrError
        self._rendering = True
        try:
            self._scene_on_device(scene, own_camera=False)  # every frame sets its camera
            p = A.make_params(target_buffer.width, target_buffer.height, 1, integrator=self._integrator, seed=seeds[0] if seeds else 0,
                              max_depth=self._max_depth, pipeline=self.pipeline)
            hist = self._ctx.history(p) if temporal is not None else None
            try:
                with self._ctx.accumulator(p, moments=denoise is not None) as acc:
                    if display is not None:
                        import torch
                        w, h = target_buffer.width, target_buffer.height
                        d_lin = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:%d" % self._ctx.device)
                        d_rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device=d_lin.device)
                        torch.cuda.synchronize(d_lin.device)  # the library works on a stream of its own
                    for k, (cam, seed) in enumerate(zip(cameras, seeds)):
                        if self._cancel_requested:
                            return
                        self._ctx.set_camera(cam)
                        acc.reset(seed)
                        if display is not None:  # the device chain: nothing below waits but the copy of the bytes
                            acc.render(spp, blocking=False)
                            if temporal is not None:
                                acc.denoise_temporal_into(hist, d_lin.data_ptr(), w, None, denoise, temporal)
                            elif denoise is not None:
                                acc.denoise_into(d_lin.data_ptr(), w, None, denoise)
                            else:
                                acc.resolve_into(d_lin.data_ptr(), w)
                            self._ctx.display_into(d_lin.data_ptr(), w, w, h, d_rgb.data_ptr(), display)
                            self._ctx.synchronize()
                            if self._ctx.stats()["cancelled"]:
                                return
                            target_buffer.display_rgb8 = d_rgb.cpu().numpy()
                            yield k
                            continue
                        try:
                            acc.render(spp)
                        except RtrError as e:
                            if e.code == A.RTR_ERR_CANCELLED:
                                return
                            raise
                        if temporal is not None:
                            target_buffer.store_linear(acc.denoise_temporal(hist, denoise, temporal, out=target_buffer.linear.copy()))
                        elif denoise is not None:
                            target_buffer.store_linear(acc.denoise(denoise, out=target_buffer.linear.copy()))
                        else:
                            target_buffer.store_linear(acc.resolve(target_buffer.linear.copy()))
                        yield k
            finally:
                if hist is not None:
                    hist.close()
        finally:
            self._rendering = False

    def display(self, target_buffer, params=None):
        """The display transform (include/rtr_hip.h: rtr_display_host; ``params``: an rtr_display_params, default
        ``display_defaults()``) of the buffer's linear image: (height, width, 3) uint8 with the top row first, for
        ``RenderBuffer.save_to_png(filename, rgb8=...)``.  Metering is global: in a sharded render call it on the rank
        that holds the gathered image."""
        return self._ctx.display(target_buffer.linear, params)[0]

    def capture_environment(self, scene, centre, face_size=32, samples=16, seed=None, jitter=1, time=0.0):
        """A ``Cubemap`` of what surrounds ``centre`` ([3]) in ``scene`` under this renderer's integrator and depth
        (include/rtr_hip.h: rtr_capture_cube): mean radiance of ``samples`` rays through every texel of six faces."""
        self._scene_on_device(scene, own_camera=False)
        p = A.make_params(2, 2, 1, integrator=self._integrator, seed=self.seed, max_depth=self._max_depth)
        rec = self._ctx.capture_cube_records(p, np.asarray(centre, dtype=np.float64).reshape(1, 3), face_size=face_size,
                                             samples=samples, seed=self.seed if seed is None else seed, jitter=jitter, time=time)
        return Cubemap(rec[0])

    def capture_environments(self, scene, volumes, face_size=32, samples=16, levels=5, fallback=-1, seed=None, jitter=1):
        """A ``CaptureSet`` of ``scene``: one capture per volume (``CAPTURE_VOLUME_DTYPE`` records) from its centre under this
        renderer's integrator and depth, filtered into ``levels`` levels, baked in place on the device
        (include/rtr_hip.h: CAPTURE SETS)."""
        self._scene_on_device(scene, own_camera=False)
        p = A.make_params(2, 2, 1, integrator=self._integrator, seed=self.seed, max_depth=self._max_depth)
        return CaptureSet.bake(self._ctx, p, volumes, face_size=face_size, samples=samples, levels=levels, fallback=fallback,
                               seed=self.seed if seed is None else seed, jitter=jitter)

    def render_preview(self, scene, env, target_buffer, grid=1, display=None):
        """The baked preview of ``scene`` under ``env`` (an ``IblEnvironment``) into ``target_buffer``
        (include/rtr_hip.h: rtr_preview): ``grid`` x ``grid`` pixel-centred rays per pixel, each hit shaded from the
        probes, the cube chain and the table instead of being path traced.  ``display`` (an rtr_display_params): the
        environment goes to the device once, rtr_preview_device and rtr_display_device follow each other on the context's
        stream with no host wait, and the bytes are left in ``target_buffer.display_rgb8`` (top row first) beside the
        linear image."""
        from . import native
        if display is not None and not isinstance(display, A.DisplayParamsC):
            raise ValueError("display must be None or rtr_display_params (display_defaults())")
        self._scene_on_device(scene)
        w, h = target_buffer.width, target_buffer.height
        p = native.preview_params(w, h, grid)
        if display is None:
            target_buffer.store_linear(env.render(self._ctx, p))
            return target_buffer
        import torch
        dev = "cuda:%d" % self._ctx.device
        host = env.env()
        keep = []

        def on_device(records):  # the records of one array of the environment as bytes on the device
            t = torch.from_numpy(np.ascontiguousarray(records).reshape(-1).view(np.uint8).copy()).to(dev)
            keep.append(t)
            return t.data_ptr()

        kw = {}
        if env.grid is not None:
            kw.update(grid=env.grid.grid(), probes=on_device(np.asarray(env.grid.coefficients, dtype=A.PROBE_SH_DTYPE)))
            vis = _visible_of(host)
            if vis is not None:
                kw.update(depth=on_device(np.asarray(env.grid.depth, dtype=A.PROBE_DEPTH_DTYPE)),
                          visible=native.probe_visible_params(vis.map_size, vis.normal_bias))
        if env.chain is not None:
            kw.update(levels=env.chain.levels, chain=on_device(np.asarray(env.chain.records, dtype=A.GATHER_OUT_DTYPE)),
                      n_records=host.n_records)
        d_env = native.shade_env(on_device(env.table.entries), n_mu=host.n_mu, n_rough=host.n_rough, **kw)
        d_lin = torch.zeros((h, w, 3), dtype=torch.float64, device=dev)
        d_rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(d_lin.device)  # the library works on a stream of its own
        self._ctx.preview_into(p, d_env, d_lin.data_ptr(), w, captures=env.captures)
        self._ctx.display_into(d_lin.data_ptr(), w, w, h, d_rgb.data_ptr(), display)
        self._ctx.synchronize()
        target_buffer.store_linear(d_lin.cpu().numpy())
        target_buffer.display_rgb8 = d_rgb.cpu().numpy()
        return target_buffer

    def _scene_on_device(self, scene, own_camera=True):
        """Upload ``scene`` unless the context holds it already.  ``own_camera``: a scene that is there but is seen from
        another camera since ``Context.set_camera`` (a ``render_sequence``) gets its own camera back, so a render of
        ``scene`` is always the image of ``scene.camera``."""
        if self._ctx.scene is not scene:
            self._ctx.upload(scene)
        elif own_camera and self._ctx.camera_updated:
            self._ctx.set_camera(scene.camera)

    def _denoised(self, acc, params, target_buffer, rank, world):
        """The denoised image of ``acc`` over the buffer's linear image.  world > 1: every rank's resolve, moments,
        counts and features are summed over the default torch.distributed group (each pixel is owned by one rank, the
        others contribute zeros) and denoised with rtr_denoise_host: the bits of the unsharded rtr_accum_denoise."""
        if world == 1:
            return acc.denoise(params, out=target_buffer.linear.copy())
        import torch
        import torch.distributed as dist
        from .native import denoise_host
        h, w = acc.shape
        own = ownership_mask(w, h, rank, world)
        ids, counts = acc.tiles()
        count = np.zeros((h, w), dtype=np.int32)
        for t, n in zip(ids, counts):
            x0, y0, x1, y1 = tile_rect(w, h, int(t))
            count[y0:y1, x0:x1] = n
        planes = [acc.resolve(), acc.moments(), count, acc.features(params.feature_spp)]
        planes = [np.where(own.reshape(own.shape + (1,) * (x.ndim - 2)), x, 0) for x in planes]
        summed = []
        for x in planes:
            t = torch.from_numpy(np.ascontiguousarray(x))
            dist.all_reduce(t)
            summed.append(t.numpy())
        return denoise_host(self._ctx, *summed, params=params, out=target_buffer.linear.copy())


class ProbeGrid:
    """A regular grid of radiance probes (include/rtr_hip.h: rtr_probe_grid and rtr_probe_sh records): ``dims`` probes from
    ``origin`` every ``spacing``, probe (ix, iy, iz) at index ix + dims[0] * (iy + dims[1] * iz).  ``bake`` fills the
    coefficients with rtr_probe_radiance, ``irradiance`` reads them with rtr_probe_lookup."""

    def __init__(self, origin, spacing, dims, coefficients=None):
        self.origin = np.asarray(origin, dtype=np.float64).reshape(3)
        self.spacing = np.asarray(spacing, dtype=np.float64).reshape(3)
        self.dims = tuple(int(d) for d in dims)
        n = self.dims[0] * self.dims[1] * self.dims[2]
        if len(self.dims) != 3 or min(self.dims) < 1 or n > A.PROBE_GRID_MAX:
            raise ValueError("dims must be three counts >= 1 with a product <= 2^24")
        if not (np.isfinite(self.origin).all() and np.isfinite(self.spacing).all() and (self.spacing > 0).all()):
            raise ValueError("origin must be finite, spacing finite and > 0")
        self.coefficients = np.zeros(n, dtype=A.PROBE_SH_DTYPE) if coefficients is None else \
            np.ascontiguousarray(coefficients, dtype=A.PROBE_SH_DTYPE)
        if len(self.coefficients) != n:
            raise ValueError("coefficients must hold %d records" % n)
        self.depth = None  # ``bake(depth=T)``: PROBE_DEPTH_DTYPE [n, T, T]
        self._ctx = None

    @classmethod
    def in_box(cls, lo, hi, dims):
        """The grid whose first and last probes stand on the corners ``lo`` and ``hi`` (an axis with one probe: at ``lo``)."""
        lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
        steps = np.maximum(np.asarray(dims, dtype=np.float64) - 1.0, 1.0)
        spacing = (hi - lo) / steps
        return cls(lo, np.where(spacing > 0, spacing, 1.0), dims)

    def positions(self):
        """[n, 3] probe positions in index order: origin + (ix, iy, iz) * spacing"""
        iz, iy, ix = np.meshgrid(*(np.arange(d, dtype=np.float64) for d in self.dims[::-1]), indexing="ij")
        idx = np.stack([ix, iy, iz], axis=-1).reshape(-1, 3)
        return self.origin + idx * self.spacing

    def grid(self):
        from . import native
        return native.probe_grid(self.origin, self.spacing, self.dims)

    def bake(self, ctx, params, samples=64, seed=0, time=0.0, depth=None, depth_samples=8, max_distance=None, classify=None):
        """rtr_probe_radiance at every probe under ``params`` (an rtr_render_params) on the scene ``ctx`` holds.
        ``depth``: the size T of an octahedral distance map per probe (rtr_probe_depth with ``depth_samples`` rays per
        texel, misses at ``max_distance``: by default 1.5 x the length of ``spacing``), kept in ``self.depth`` as
        ``PROBE_DEPTH_DTYPE`` [n, T, T]; None bakes none.  ``classify``: with a map, ``self.classify`` afterwards (True: its
        default fraction; a number: that fraction)."""
        self.coefficients = ctx.probe_radiance(params, self.positions(), samples=samples, seed=seed, time=time)
        self.depth = None
        if depth is not None:
            t_max = float(max_distance) if max_distance is not None else 1.5 * float(np.sqrt((self.spacing * self.spacing).sum()))
            self.depth = ctx.probe_depth(self.positions(), map_size=int(depth), samples=int(depth_samples), seed=seed, time=time,
                                         t_max=t_max)
            if classify is not None and classify is not False:
                self.classify() if classify is True else self.classify(float(classify))
        self._ctx = ctx
        return self

    def classify(self, back_fraction=0.25):
        """Sets ``valid = 0`` on every probe whose distance map saw the inside of surfaces on more than ``back_fraction`` of
        its hits (sum(back) > back_fraction * sum(hits)): a probe inside geometry, which no lookup should use.  Returns the
        bool mask [n] of the probes it invalidated."""
        if self.depth is None:
            raise ValueError("classify needs distance maps: bake with depth=T first")
        back = self.depth["back"].reshape(len(self.depth), -1).sum(axis=1, dtype=np.int64)
        hits = self.depth["hits"].reshape(len(self.depth), -1).sum(axis=1, dtype=np.int64)
        inside = back > back_fraction * hits
        self.coefficients["valid"][inside] = 0
        return inside

    def irradiance(self, points, normals, ctx=None, visible=None, normal_bias=None):
        """rtr_probe_lookup: [n, 3] irradiance at the queries; rows whose eight corners are all invalid are zero.  ``ctx``:
        the context that runs it (default: the one that baked).  ``visible`` (default: distance maps were baked):
        rtr_probe_lookup_visible, every corner weighed by its probe's distance map, tested ``normal_bias`` off the surface
        (default 0.25 x the smallest spacing)."""
        ctx = ctx if ctx is not None else self._ctx
        if ctx is None:
            raise ValueError("irradiance needs a context: bake first or pass ctx")
        if visible is None:
            visible = self.depth is not None
        if not visible:
            return ctx.probe_lookup(self.grid(), self.coefficients, points, normals)["v"]
        if self.depth is None:
            raise ValueError("a visible lookup needs distance maps: bake with depth=T first")
        bias = float(normal_bias) if normal_bias is not None else 0.25 * float(self.spacing.min())
        return ctx.probe_lookup_visible(self.grid(), self.coefficients, self.depth, points, normals, normal_bias=bias)["v"]


class Cubemap:
    """One environment capture (include/rtr_hip.h: rtr_capture_cube): ``texels``, ``GATHER_OUT_DTYPE`` records [6, S, S]
    (face, row, column).  ``lookup`` reads it along directions (rtr_cube_lookup_one, or rtr_cube_lookup on a context),
    ``to_latlong`` resamples it to the equirectangular layout of the reference's EnvironmentLight, ``save_hdr`` writes that
    as a Radiance .hdr file an EnvironmentLight can read, ``prefilter`` makes the chain of GGX-filtered levels a glossy
    object reads (``CubeChain``)."""

    def __init__(self, texels):
        t = np.ascontiguousarray(texels, dtype=A.GATHER_OUT_DTYPE)
        if t.ndim != 3 or t.shape[0] != 6 or t.shape[1] != t.shape[2] or not 1 <= t.shape[1] <= A.CAPTURE_MAX_FACE:
            raise ValueError("texels must be [6, S, S] records, 1 <= S <= %d" % A.CAPTURE_MAX_FACE)
        self.texels = t
        self.face_size = int(t.shape[1])

    @property
    def radiance(self):
        """[6, S, S, 3] mean radiance"""
        return self.texels["v"]

    def lookup(self, directions, ctx=None):
        """[n, 3] radiance along the directions [n, 3], bilinear inside a face; zero where the lookup is invalid.
        ``ctx``: a context to run it on the device (default: on the host)."""
        from . import native
        if ctx is not None:
            return ctx.cube_lookup(self.texels, directions)["v"]
        return native.cube_lookup_host(self.texels, directions)["v"]

    def to_latlong(self, width, height):
        """rtr_cube_to_latlong: [height, width, 3], row 0 the top (+y), the centre column towards +x."""
        from . import native
        return native.cube_to_latlong(self.texels, width, height)

    def save_hdr(self, path, width, height):
        """``to_latlong(width, height)`` written with rtr_write_rgbe."""
        from . import native
        native.write_rgbe(path, self.to_latlong(width, height))

    def prefilter(self, levels=5, cos_cut=0.0, ctx=None):
        """A ``CubeChain`` of ``levels`` levels (rtr_cube_chain_plan): level 0 is this capture, level i its GGX filter
        (rtr_cube_filter) at the plan's alpha and face size.  ``ctx``: a context to filter on the device (default: the
        host loop of rtr_cube_filter_one, for small cubes)."""
        from . import native
        plan, n_records = native.cube_chain_plan(self.face_size, levels)
        records = np.zeros(n_records, dtype=A.GATHER_OUT_DTYPE)
        records[:6 * self.face_size ** 2] = self.texels.reshape(-1)
        for lv in list(plan)[1:]:
            fp = native.cube_filter_defaults(face_in=self.face_size, face_out=lv.face_size, alpha=lv.alpha, cos_cut=cos_cut)
            level = ctx.cube_filter(self.texels, fp) if ctx is not None else native.cube_filter_host(self.texels, fp)
            records[lv.offset:lv.offset + 6 * lv.face_size ** 2] = level.reshape(-1)
        return CubeChain(plan, records)


class CubeChain:
    """A capture and its filtered levels (include/rtr_hip.h: rtr_cube_chain_*): ``levels``, a ctypes array of
    rtr_cube_level, and ``records``, the ``GATHER_OUT_DTYPE`` records of all of them."""

    def __init__(self, levels, records):
        self.levels = levels
        self.records = np.ascontiguousarray(records, dtype=A.GATHER_OUT_DTYPE).reshape(-1)

    def __len__(self):
        return len(self.levels)

    def level(self, i):
        """Level ``i`` as a ``Cubemap``"""
        lv = self.levels[i]
        S = lv.face_size
        return Cubemap(self.records[lv.offset:lv.offset + 6 * S * S].reshape(6, S, S))

    def lookup_records(self, directions, roughness, ctx=None):
        """The ``GATHER_OUT_DTYPE`` records of the seam-aware lookup along the directions [n, 3] at ``roughness`` (a number
        or [n]); alpha = roughness squared, the levels around it blended."""
        from . import native
        r = np.asarray(roughness, dtype=np.float64)
        q = native.cube_queries(directions, r * r)
        if ctx is not None:
            return ctx.cube_chain_lookup(self.levels, self.records, q)
        return native.cube_chain_lookup_host(self.levels, self.records, q)

    def lookup(self, directions, roughness, ctx=None):
        """[n, 3] radiance of ``lookup_records``; zero where the lookup is invalid."""
        return self.lookup_records(directions, roughness, ctx)["v"]

    def save_hdr(self, prefix, width, height):
        """Every level as a width x height equirectangular Radiance file: ``prefix``.hdr for level 0, ``prefix``.L<i>.hdr
        for level i.  Returns the paths."""
        paths = []
        for i in range(len(self.levels)):
            paths.append("%s.hdr" % prefix if i == 0 else "%s.L%d.hdr" % (prefix, i))
            self.level(i).save_hdr(paths[-1], width, height)
        return paths


class CaptureSet:
    """Several captures of one scene with the boxes they serve (include/rtr_hip.h: rtr_capture_set*): ``volumes``,
    ``CAPTURE_VOLUME_DTYPE`` records, ``fallback`` (the capture read where none reaches, or -1), ``levels``, the plan of ONE
    capture, and ``records``, the ``GATHER_OUT_DTYPE`` records of all captures level-major.  A lookup projects the
    direction onto the proxy box of every capture that reaches the point and blends what they hold."""

    def __init__(self, volumes, levels, records, fallback=-1):
        from . import native
        self._set = native.capture_set(volumes, fallback)
        self.volumes, self.fallback = self._set.records, int(fallback)
        self.levels = levels
        self.records = np.ascontiguousarray(records, dtype=A.GATHER_OUT_DTYPE).reshape(-1)
        if len(self.records) % len(self.volumes):
            raise ValueError("records must hold the same number of records for every capture")

    def __len__(self):
        return len(self.volumes)

    @property
    def n_records(self):
        """records of one capture"""
        return len(self.records) // len(self.volumes)

    def set(self):
        """The rtr_capture_set over the host volumes"""
        return self._set

    @classmethod
    def bake(cls, ctx, render_params, volumes, face_size=32, samples=16, levels=5, fallback=-1, seed=0, jitter=1, cos_cut=0.0):
        """One rtr_capture_cube_device call over the volumes' centres and one rtr_cube_filter_device call per further
        level, straight into the level-major array on the device and with no host wait between them; the records come
        back once at the end.  ``ctx`` holds the scene; ``render_params`` an rtr_render_params (integrator, depth)."""
        import torch
        from . import native
        vols = native.capture_set(volumes, fallback).records
        C_ = len(vols)
        plan, n_records = native.cube_chain_plan(face_size, levels)
        dev = "cuda:%d" % ctx.device
        d_centres = torch.from_numpy(native.probe_points(vols["centre"]).view(np.uint8).reshape(-1).copy()).to(dev)
        d_set = torch.zeros(C_ * n_records * 32, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(d_set.device)  # the library works on a stream of its own
        base = d_set.data_ptr()
        ctx.capture_cube_into(render_params, d_centres.data_ptr(), base, C_, face_size=face_size, samples=samples, seed=seed,
                              jitter=jitter)
        for lv in list(plan)[1:]:
            ctx.cube_filter_into(base, base + C_ * lv.offset * 32, C_, face_in=face_size, face_out=lv.face_size, alpha=lv.alpha,
                                 cos_cut=cos_cut)
        ctx.synchronize()
        return cls(vols, plan, d_set.cpu().numpy().view(A.GATHER_OUT_DTYPE), fallback)

    def chain(self, k):
        """Capture ``k`` as a ``CubeChain``"""
        C_ = len(self.volumes)
        parts = []
        for lv in self.levels:
            F = 6 * lv.face_size * lv.face_size
            parts.append(self.records[lv.offset * C_ + k * F:lv.offset * C_ + (k + 1) * F])
        return CubeChain(self.levels, np.concatenate(parts))

    def lookup_records(self, points, directions, roughness, ctx=None):
        """The ``GATHER_OUT_DTYPE`` records of rtr_capture_set_lookup at the points [n, 3] along the directions [n, 3] at
        ``roughness`` (a number or [n]; alpha = roughness squared); ``ctx``: a context to run it on the device."""
        from . import native
        r = np.asarray(roughness, dtype=np.float64)
        q = native.capture_queries(points, directions, r * r)
        if ctx is not None:
            return ctx.capture_set_lookup(self._set, self.levels, self.records, q)
        return native.capture_set_lookup_host(self._set, self.levels, self.records, q)

    def lookup(self, points, directions, roughness, ctx=None):
        """[n, 3] radiance of ``lookup_records``; zero where the lookup is invalid."""
        return self.lookup_records(points, directions, roughness, ctx)["v"]


class BrdfTable:
    """The environment BRDF table of the split-sum approximation (include/rtr_hip.h: rtr_brdf_table): ``entries``,
    ``BRDF_ENTRY_DTYPE`` [n_rough, n_mu]; int f_spec cos dw ~ F0 * a + b at (mu, roughness)."""

    def __init__(self, entries):
        t = np.ascontiguousarray(entries, dtype=A.BRDF_ENTRY_DTYPE)
        if t.ndim != 2 or not (1 <= t.shape[0] <= A.BRDF_MAX and 1 <= t.shape[1] <= A.BRDF_MAX):
            raise ValueError("entries must be [n_rough, n_mu] records, 1 .. %d each" % A.BRDF_MAX)
        self.entries = t

    @classmethod
    def make(cls, n_mu=32, n_rough=32, nodes=128, ctx=None):
        """rtr_brdf_table on ``ctx``; without one the host loop of rtr_brdf_entry_one (for small tables)."""
        from . import native
        return cls(ctx.brdf_table(n_mu, n_rough, nodes) if ctx is not None else native.brdf_table_host(n_mu, n_rough, nodes))

    def fetch(self, mu, rough):
        """(a, b) of rtr_brdf_fetch_one at (mu, rough)"""
        from . import native
        return native.brdf_fetch_one(self.entries, mu, rough)


class IblEnvironment:
    """What rtr_shade_ibl shades under: a ``ProbeGrid`` (diffuse; its distance maps select the visible lookup), a
    ``CubeChain`` or a ``CaptureSet`` (specular; a set runs the rtr_*_set entries) and a ``BrdfTable``.  ``grid`` or
    ``chain`` may be None: that part is left out."""

    def __init__(self, grid, chain, table, normal_bias=None):
        if grid is None and chain is None:
            raise ValueError("an environment needs a grid, a chain or both")
        self.grid, self.chain, self.table = grid, chain, table
        self.normal_bias = normal_bias

    @property
    def captures(self):
        """The rtr_capture_set of a ``CaptureSet`` environment, or None"""
        return self.chain.set() if isinstance(self.chain, CaptureSet) else None

    def env(self):
        """The rtr_shade_env over the host arrays"""
        from . import native
        kw = {}
        if self.grid is not None:
            kw.update(grid=self.grid.grid(), probes=self.grid.coefficients)
            if self.grid.depth is not None:
                bias = float(self.normal_bias) if self.normal_bias is not None else 0.25 * float(self.grid.spacing.min())
                kw.update(depth=self.grid.depth, visible=native.probe_visible_params(self.grid.depth.shape[-1], bias))
        if self.chain is not None:
            kw.update(levels=self.chain.levels, chain=self.chain.records)
            if isinstance(self.chain, CaptureSet):
                kw.update(n_records=self.chain.n_records)
        return native.shade_env(self.table.entries, **kw)

    def shade_records(self, points, normals, views, base, roughness, metallic, ctx=None):
        """The ``GATHER_OUT_DTYPE`` records of rtr_shade_ibl; ``ctx``: the context that runs it (default: the grid's
        baking context, else the host loop of rtr_shade_ibl_one)."""
        from . import native
        q = native.shade_queries(points, normals, views, base, roughness, metallic)
        ctx = ctx if ctx is not None else (self.grid._ctx if self.grid is not None else None)
        if ctx is not None:
            return ctx.shade_ibl(self.env(), q, captures=self.captures)
        if self.captures is not None:
            return native.shade_ibl_set_one(self.env(), self.captures, q)
        return native.shade_ibl_one(self.env(), q)

    def shade(self, points, normals, views, base, roughness, metallic, ctx=None):
        """[n, 3] radiance towards the viewers: points, normals and view vectors [n, 3], base colour [n, 3] or one colour,
        roughness and metallic numbers or [n]; zero where a lookup is invalid."""
        return self.shade_records(points, normals, views, base, roughness, metallic, ctx)["v"]

    def render(self, ctx, params, return_lit=False):
        """rtr_preview: the frame of the scene ``ctx`` holds, seen from its current camera and shaded under this
        environment; ``params`` from ``native.preview_params``.  Linear (h, w, 3), row 0 the lowest row; with
        ``return_lit`` also the (h, w) count of samples per pixel that found something to add."""
        return ctx.preview(params, self.env(), return_lit=return_lit, captures=self.captures)


def _visible_of(env):
    """The rtr_probe_visible_params an rtr_shade_env points to, or None"""
    import ctypes
    return ctypes.cast(env.visible, ctypes.POINTER(A.ProbeVisibleParamsC)).contents if env.visible else None


def check_denoise(params):
    """ValueError unless ``params`` is None or valid rtr_denoise_params (the checks of rtr_accum_denoise)."""
    import math
    if params is None:
        return
    if not isinstance(params, A.DenoiseParamsC):
        raise ValueError("denoise must be None or rtr_denoise_params (denoise_defaults())")
    if not 0 <= params.iterations <= 10:
        raise ValueError("denoise iterations must be in 0..10: %r" % params.iterations)
    if params.feature_spp < 1:
        raise ValueError("denoise feature_spp must be >= 1: %r" % params.feature_spp)
    for k in ("sigma_l", "sigma_n", "sigma_a", "sigma_z"):
        v = getattr(params, k)
        if not (v > 0.0 and math.isfinite(v)):
            raise ValueError("denoise %s must be finite and > 0: %r" % (k, v))
    if any(r != 0.0 for r in params.reserved):
        raise ValueError("denoise reserved fields must be 0")


def _tile_view(t, width, height):
    """(H, W, 3) tensor -> view [tile row (j // 16), tile column, 16, 16, 3]; H and W must be multiples of 16."""
    return t.view(height // TILE, TILE, width // TILE, TILE, 3).permute(0, 2, 1, 3, 4)


def _tile_coords(tiles, width, height):
    import torch
    tx, ty = (width + TILE - 1) // TILE, (height + TILE - 1) // TILE
    idx = torch.as_tensor(list(tiles), dtype=torch.long)
    return (ty - 1) - idx // tx, idx % tx


def pack_tiles(fb, tiles, width, height):
    """The 16x16 tiles ``tiles`` (reference dispatch numbering) of framebuffer ``fb`` (torch tensor
    (H, W, 3), row 0 = bottom row, host or device) as one dense (n, 16, 16, 3) tensor on the same device:
    what a rank sends to the gathering rank -- its own tiles and nothing else (50 MB per GPU
    for C5 instead of the 403 MB frame).  Pixels past the image edge are zero."""
    import torch
    hp, wp = (height + TILE - 1) // TILE * TILE, (width + TILE - 1) // TILE * TILE
    if (hp, wp) != (height, width):
        padded = torch.zeros((hp, wp, 3), dtype=fb.dtype, device=fb.device)
        padded[:height, :width] = fb
        fb = padded
    ty, tx = _tile_coords(tiles, width, height)
    return _tile_view(fb.contiguous(), wp, hp)[ty.to(fb.device), tx.to(fb.device)].contiguous()


def unpack_tiles(parts, tile_lists, width, height, out=None):
    """Inverse of pack_tiles on the host: scatter each rank's dense tile block into the (H, W, 3) image.
    Returns (image as a numpy array, per-tile coverage count as a (tiles_y, tiles_x) array)."""
    import torch
    hp, wp = (height + TILE - 1) // TILE * TILE, (width + TILE - 1) // TILE * TILE
    full = torch.zeros((hp, wp, 3), dtype=torch.float64)
    if out is not None:
        full[:height, :width] = torch.from_numpy(np.ascontiguousarray(out))
    covered = torch.zeros((hp // TILE, wp // TILE), dtype=torch.int32)
    view = _tile_view(full, wp, hp)
    for part, tiles in zip(parts, tile_lists):
        ty, tx = _tile_coords(tiles, width, height)
        view[ty, tx] = part[:len(ty)].to(torch.float64)
        covered.index_put_((ty, tx), torch.ones(len(ty), dtype=torch.int32), accumulate=True)
    return full[:height, :width].numpy(), covered.numpy()


def gather_tiles(fb, width, height, rank, world, group=None, dst=0, tile_first=None, tile_stride=None):
    """Host-side framebuffer gather of a tile-sharded render: every rank packs the tiles it owns
    (``index % tile_stride == tile_first``, default rank / world), copies them to the host once and sends
    them to ``dst`` over a CPU-capable process group (gloo); no collective touches the render itself.
    Returns on ``dst`` (image, coverage) as unpack_tiles does, elsewhere (None, None).  ``bytes_sent`` of
    the last call is kept on the function for reporting."""
    import torch
    import torch.distributed as dist
    stride = world if tile_stride is None else tile_stride
    firsts = list(range(world)) if tile_first is None else [tile_first - rank + r for r in range(world)]
    lists = [tiles_of_rank(width, height, firsts[r], stride) for r in range(world)]
    mine = pack_tiles(fb, lists[rank], width, height).cpu()
    gather_tiles.bytes_sent = int(mine.numel() * mine.element_size())
    if world == 1:
        return unpack_tiles([mine], lists, width, height)
    n_max = max(len(t) for t in lists)
    if len(mine) < n_max:  # ragged shares (tile count not a multiple of world): pad to the largest
        pad = torch.zeros((n_max, TILE, TILE, 3), dtype=mine.dtype)
        pad[:len(mine)] = mine
        mine = pad
    parts = [torch.empty_like(mine) for _ in range(world)] if rank == dst else None
    dist.gather(mine, parts, dst=dst, group=group)
    if rank != dst:
        return None, None
    return unpack_tiles(parts, lists, width, height)


def render_sharded(render_fn, width, height, rank, world, group=None, dst=0):
    """Tile-sharded render over the ranks of a ``torch.distributed`` job.

    ``render_fn(tile_first, tile_stride) -> (H, W, 3) float64`` renders this rank's tiles (other
    pixels are ignored).  The framebuffer is gathered on the host: every rank sends the tiles it owns
    (and only those) to ``dst`` over any backend that moves CPU tensors (gloo).  No collective takes part
    in the render itself.  Returns the full image on ``dst`` and None elsewhere."""
    part = np.ascontiguousarray(render_fn(rank, world), dtype=np.float64)
    if world == 1:
        return part
    import torch
    image, covered = gather_tiles(torch.from_numpy(part), width, height, rank, world, group=group, dst=dst)
    if rank != dst:
        return None
    if not np.all(covered == 1):
        raise RuntimeError("tile sharding does not partition the image")
    return image
