"""The restatement of the baked preview (include/rtr_hip.h: rtr_preview_*) for tests/test_preview_cpu.py and
tests/test_preview.py: the rays in numpy, the material mapping from the scene description, the pixel reduction over
rtr_shade_ibl_one, and the environments the tests shade under (tests/_ibl_cases.py, moved over the scene)."""
import ctypes as C

import numpy as np

import _golden as G
import _ibl_cases as IC

A = G.A
N = G.rtr.native

SAMPLE = A.PREVIEW_SAMPLE_DTYPE
MISS, EMITTER, SURFACE = A.PREVIEW_MISS, A.PREVIEW_EMITTER, A.PREVIEW_SURFACE
SCENES = (21, 7, 23, 24)        # every field restated
TEXTURED = (1, 35)              # textures no public call evaluates: base is not restated
# (miss, lambertian, metal, dielectric, PBR, emitter) of the 1024 pixel-centre rays of a 32 x 32 image, classified on the
# CPU with the oracle's rto_hits
COUNTS = {21: (183, 836, 0, 0, 0, 5), 7: (183, 836, 0, 0, 0, 5), 23: (256, 577, 0, 64, 127, 0), 24: (842, 0, 58, 63, 61, 0)}
RAGGED = (3, 5, 30, 21)


def numpy_rays(cam, W, H, k, region=None, t_min=0.001):
    """RAY of the contract, ``RAY_DTYPE`` [h, w, k * k]: every operation a numpy float64 operation in the stated order"""
    x0, y0, x1, y1 = region if region is not None else (0, 0, W, H)
    cam = np.asarray(cam).reshape(-1)[0]
    s = np.arange(k * k)
    a, b = (s % k).astype(np.float64), (s // k).astype(np.float64)
    i = np.arange(x0, x1, dtype=np.float64)[None, :, None]
    j = np.arange(y0, y1, dtype=np.float64)[:, None, None]
    kd = np.float64(k)
    u = (i + (a + 0.5) / kd) / np.float64(W - 1) + 0.0 * j
    v = (j + (b + 0.5) / kd) / np.float64(H - 1) + 0.0 * i
    rays = np.zeros(u.shape, dtype=A.RAY_DTYPE)
    for c in range(3):
        rays["origin"][..., c] = cam["origin"][c]
        rays["direction"][..., c] = ((cam["lower_left_corner"][c] + u * cam["horizontal"][c]) + v * cam["vertical"][c]) - cam["origin"][c]
    rays["time"], rays["t_min"], rays["t_max"], rays["rng_state"] = cam["time0"], t_min, np.inf, 1
    return rays


def hit_records(rays):
    """the oracle's ``HIT_DTYPE`` input records of ``RAY_DTYPE`` rays (flattened)"""
    r = rays.reshape(-1)
    h = np.zeros(len(r), dtype=A.HIT_DTYPE)
    h["o"], h["d"], h["time"], h["t_min"], h["t_max"], h["rng_in"] = r["origin"], r["direction"], r["time"], r["t_min"], r["t_max"], 1
    return h


def _solid(scene, tex):
    t = scene.textures[tex]
    return t["f"][:3].copy() if t["type"] == A.TEX_SOLID else None


def samples_of(scene, rays, hits, miss_direct=None):
    """SAMPLE of the contract from the scene description: ``PREVIEW_SAMPLE_DTYPE`` of the shape of ``rays`` from hit records
    (``RAY_HIT_DTYPE`` of rtr_query_closest or the oracle's ``HIT_DTYPE``: hit, front_face, material, p, n) and the values of
    the missing rays ([n_miss, 3], None: 0).  Also the bool mask of the samples whose every field is restated: False where a
    value comes from a texture that is not a solid colour (q.base, roughness, metallic or direct stay 0 there)."""
    r, h = rays.reshape(-1), hits.reshape(-1)
    out = np.zeros(len(r), dtype=SAMPLE)
    full = np.ones(len(r), dtype=bool)
    miss = h["hit"] == 0
    out["kind"][miss], out["material"][miss] = MISS, -1
    if miss_direct is not None:
        out["direct"][miss] = miss_direct
    for k in np.flatnonzero(~miss):
        m = scene.materials[h["material"][k]]
        out["material"][k] = h["material"][k]
        if m["type"] == A.MAT_DIFFUSE_LIGHT:
            out["kind"][k] = EMITTER
            if h["front_face"][k]:
                c = _solid(scene, m["tex"][0])
                full[k] = c is not None
                if c is not None:
                    out["direct"][k] = c
            continue
        out["kind"][k] = SURFACE
        q = out["q"][k]
        q["p"], q["n"], q["v"] = h["p"][k], h["n"][k], -r["direction"][k]
        if m["type"] == A.MAT_METAL:
            q["base"], q["roughness"], q["metallic"] = m["f"][:3], m["f"][3], 1.0
        elif m["type"] == A.MAT_DIELECTRIC:
            q["base"], q["roughness"], q["metallic"] = 1.0, 0.0, 1.0
        elif m["type"] == A.MAT_PBR:
            c = [_solid(scene, m["tex"][t]) for t in range(3)]
            full[k] = all(x is not None for x in c)
            if full[k]:
                q["base"], q["roughness"], q["metallic"] = c[0], c[1][0], c[2][0]
        else:
            assert m["type"] == A.MAT_LAMBERTIAN
            c = _solid(scene, m["tex"][0])
            full[k] = c is not None
            q["roughness"], q["metallic"] = 1.0, 0.0
            if c is not None:
                q["base"] = c
    return out.reshape(rays.shape), full.reshape(rays.shape)


def counts_of(scene, samples):
    """(miss, lambertian, metal, dielectric, PBR, emitter) of sample records"""
    s = samples.reshape(-1)
    types = np.where(s["material"] >= 0, scene.materials["type"][np.maximum(s["material"], 0)], -1)
    return (int((s["kind"] == MISS).sum()), int((types == A.MAT_LAMBERTIAN).sum()), int((types == A.MAT_METAL).sum()),
            int((types == A.MAT_DIELECTRIC).sum()), int((types == A.MAT_PBR).sum()), int((s["kind"] == EMITTER).sum()))


def shade_samples(host_env, samples):
    """(v [n, 3], added [n] bool) per sample of PIXEL: what the sample adds and whether it adds anything; the SURFACE
    samples through rtr_shade_ibl_one, whose refusal of a BAD query is "adds nothing" """
    s = np.ascontiguousarray(samples.reshape(-1))
    v = s["direct"].copy()
    added = s["kind"] != SURFACE
    L = N.lib()
    out = np.zeros(1, dtype=A.GATHER_OUT_DTYPE)
    base = s.ctypes.data
    for k in np.flatnonzero(s["kind"] == SURFACE):
        rc = L.rtr_shade_ibl_one(C.byref(host_env), base + SAMPLE.itemsize * int(k), out.ctypes.data)
        if rc == 0 and out["valid"][0]:
            v[k], added[k] = out["v"][0], True
        else:
            v[k] = 0.0
    return v, added


def frame_of(host_env, samples):
    """PIXEL of the contract over [h, w, k * k] sample records: (linear [h, w, 3], lit [h, w] int32)"""
    h, w, kk = samples.shape
    v, added = shade_samples(host_env, samples)
    v, added = v.reshape(h, w, kk, 3), added.reshape(h, w, kk)
    acc = np.zeros((h, w, 3), dtype=np.float64)
    for s in range(kk):
        acc = np.where(added[:, :, s, None], acc + v[:, :, s], acc)
    return np.float64(1.0 / kk) * acc, added.sum(axis=2).astype(np.int32)


def environment(points, depth=True):
    """tests/_ibl_cases.py: environment((2, 2, 2), chain (4, 3), table (4, 4), T = 1) -- invalid probe 1 with NaN, NaN texel
    of face 3 -- with the grid moved over the middle half of the bounding box of ``points`` ([n, 3]); ``depth`` False: the
    same without distance maps"""
    env = IC.environment((2, 2, 2), (4, 3), (4, 4), 1)
    lo, hi = points.min(axis=0), points.max(axis=0)
    ext = np.where(hi > lo, hi - lo, 1.0)
    env["origin"] = tuple(float(x) for x in lo + 0.25 * ext)
    env["spacing"] = tuple(float(x) for x in 0.5 * ext)
    env["normal_bias"] = float(0.01 * ext.min())
    if depth:  # distances on the scale of the scene
        env["depth"]["mean"] *= float(ext.max())
        env["depth"]["mean2"] *= float(ext.max()) ** 2
    else:
        env["depth"] = None
    return env
