"""What the CPU tests (test_oracle_golden.py) and the GPU tests (test_shading_edges.py) of the shading-edge vectors share:
the fixture names, NaN-aware comparisons, and the selectors that find -- from a record's own inputs -- the records of a
named case (oracle/ref_harness.cpp: materials-edge, scatter-edge, lights-edge).  Test infrastructure only."""
import numpy as np

import _golden as G

A = G.A

EDGE_SCENE = 1014  # harness scene: one sphere per material class / texture class / end of the roughness clamp
MATERIAL_EDGE_SCENES = [EDGE_SCENE, 21, 23, 35]
SCATTER_FILES = {"scatter_scene09.bin": 9, "scatter_scene1014.bin": EDGE_SCENE, "scatter_edge_scene1014.bin": EDGE_SCENE}
LIGHT_EDGE_SCENES = [21, 23, 15, 17, 18, 19, 24, 26]
MAT_FLOAT_FIELDS = ("s_wi", "s_f", "s_pdf", "eval", "pdf", "emitted")
LIGHT_FLOAT_FIELDS = ("Li", "wi", "pdf", "dist", "pdf_dir")
POW5_FILES = ["pow5_%d.bin" % k for k in range(7)]  # 65536 pairs (x, glibc pow(x, 5.0)) in slices below 160 KB


def pow5_pairs():
    """x and glibc's pow(x, 5.0) of all slices, (65536, 2), and the manifest's count of values the library's pow5 misses"""
    xy = np.concatenate([np.fromfile(G.os.path.join(G.GOLD, n), dtype="<f8").reshape(-1, 2) for n in POW5_FILES])
    return xy, sum(G.MANIFEST["files"][n]["info"]["differs_from_pow5_host"] for n in POW5_FILES)


def material_edge_name(sid):
    return "materials_edge_scene%02d.bin" % sid


def light_edge_name(sid):
    return "lights_edge_scene%02d.bin" % sid


def edge_files():
    """every fixture whose manifest entry carries per-case record counts"""
    return [material_edge_name(s) for s in MATERIAL_EDGE_SCENES] + ["scatter_edge_scene1014.bin"] + \
        [light_edge_name(s) for s in LIGHT_EDGE_SCENES]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b):
    """elementwise: equal in every bit, a NaN equal to a NaN of any payload"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (np.isnan(a) & np.isnan(b)) | (bits(a) == bits(b))


def close(a, b, rtol):
    """test_gpu_parity._close, with bit-equal values (infinities) and NaN pairs counted as close"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return same(a, b) | (np.abs(a - b) <= rtol * np.maximum(np.abs(b), 1e-300) + 1e-300)


def rows(mask):
    mask = np.asarray(mask)
    return mask if mask.ndim == 1 else mask.reshape(mask.shape[0], -1).all(axis=1)


def material_types(sc, recs):
    return sc.materials["type"][recs["material"]]


def first_texture_types(sc, recs):
    """type of the texture tex[0] of each record's material (-1: the material has none)"""
    t0 = sc.materials["tex"][recs["material"], 0]
    return np.where(t0 >= 0, sc.textures["type"][np.maximum(t0, 0)], -1)


def sample_written(sc, gold):
    """records whose BSDFSample the reference writes (tests/test_oracle_golden.py: test_material_vectors)"""
    types = material_types(sc, gold)
    return np.isin(types, [A.MAT_LAMBERTIAN, A.MAT_METAL, A.MAT_DIELECTRIC]) | ((types == A.MAT_PBR) & (gold["sample_ok"] == 1))


def scatter_written(sc, gold):
    """records whose attenuation and scattered ray the reference's scatter() writes: every class but diffuse_light and
    PBRMaterial, which return false at once"""
    return np.isin(material_types(sc, gold), [A.MAT_LAMBERTIAN, A.MAT_METAL, A.MAT_DIELECTRIC, A.MAT_ISOTROPIC])


def dielectric_straddle(sc, recs, scatter):
    """dielectric records whose refraction_ratio * sin_theta lies within 1e-12 of 1.0 (material.h:158-163, :179-183)"""
    types = material_types(sc, recs)
    ir = sc.materials["f"][recs["material"], 0]
    wo = recs["wo"]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(recs["front_face"] != 0, 1.0 / ir, ir)
        d = -wo / np.linalg.norm(wo, axis=1, keepdims=True) if scatter else wo
        cos = np.minimum((d * recs["n"]).sum(axis=1), 1.0)
        sin = np.sqrt(1.0 - cos * cos)
        return (types == A.MAT_DIELECTRIC) & (np.abs(ratio * sin - 1.0) < 1e-12)


def quad_alpha_beta_edge(sc, recs):
    """QuadLight pdf() records that leave one unit in front of the light along -normal and land on alpha or beta in {0, 1}
    within 1e-12 (quad_light.h:58-69)"""
    l = sc.lights["f"][recs["light"]]
    q, u, v, n = l[:, 0:3], l[:, 3:6], l[:, 6:9], l[:, 12:15]
    sel = (sc.lights["type"][recs["light"]] == A.LIGHT_QUAD) & (recs["dir"] == -n).all(axis=1)
    planar = recs["p"] - n - q  # t = 1, direction = -normal
    alpha = (planar * u).sum(axis=1) / (u * u).sum(axis=1)
    beta = (planar * v).sum(axis=1) / (v * v).sum(axis=1)
    sel &= np.abs(((q - recs["p"]) * n).sum(axis=1) + 1.0) < 1e-9
    on = (np.abs(alpha * (1 - alpha)) < 1e-12) | (np.abs(beta * (1 - beta)) < 1e-12)
    return sel & on


def spot_straddle(sc, recs):
    """SpotLight records whose cos_theta lies within 1e-12 of cos_cutoff (spot_light.h:23-25)"""
    l = sc.lights["f"][recs["light"]]
    d = l[:, 0:3] - recs["p"]
    with np.errstate(invalid="ignore", divide="ignore"):
        wi = d / np.linalg.norm(d, axis=1, keepdims=True)
        cos = (-wi * l[:, 3:6]).sum(axis=1)
        return (sc.lights["type"][recs["light"]] == A.LIGHT_SPOT) & (np.abs(cos - l[:, 9]) < 1e-12)
