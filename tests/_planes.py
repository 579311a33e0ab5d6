"""Synthetic input planes for the a-trous filter and the temporal stage, and scalar references of both written from the
text of include/rtr_hip.h alone ("Filter" and the temporal comment): plain Python floats, one pixel at a time, a dict
keyed by (y, x), taps in the documented order.  The builders of the filter's planes and the scalar references look at
neither _denoise_ref nor _temporal_ref: the CPU tests hold those restatements to these references, the GPU tests hold
the kernels to the restatements.  Only the temporal cases at the end use _temporal_ref, for its cameras and to make the
history of a first frame.  Test infrastructure.

Planes are (H, W, ...) arrays of a region, row 0 = its lowest row, as rtr_denoise_host takes them."""
import math

import numpy as np

INT32_MAX = 2147483647
COUNTS = (0, 1, 2, 3, 7, INT32_MAX)
ALBEDOS = (0.0, float(np.nextafter(1e-3, 0.0)), 1e-3, float(np.nextafter(1e-3, 1.0)), 0.5, 0.73, 1.0)
DEPTHS = (0.0, -0.0, -1.0, 1e-3, float(np.nextafter(1e-3, 0.0)), float(np.nextafter(1e-3, 1.0)), 1.0, 5.5, 1e6)


def _draw(rng, values, n):
    """n draws from ``values`` in which every value occurs as soon as n >= len(values): a shuffled round robin"""
    return np.asarray(values)[rng.permutation(np.arange(n) % len(values))]


def planes(h, w, seed, valid=None):
    """(color (h, w, 3), q (h, w), count (h, w) int32, feat (h, w, 7)) from ``seed``.  With a boolean mask ``valid`` the
    holes are exactly its False pixels; without one the counts are drawn from COUNTS, zeros included, and one pixel is
    made valid if none is.  Every plane holds NaN where count is 0."""
    rng = np.random.default_rng(seed)
    n = h * w
    color = rng.uniform(0.0, 2.0, (h, w, 3))
    if valid is None:
        count = _draw(rng, COUNTS, n).reshape(h, w)
        if not (count > 0).any():
            count[rng.integers(h), rng.integers(w)] = 2
    else:
        valid = np.asarray(valid, dtype=bool)
        assert valid.shape == (h, w) and valid.any()
        count = np.where(valid, _draw(rng, COUNTS[1:], n).reshape(h, w), 0)
    count = count.astype(np.int32)
    y = 0.2126 * color[..., 0] + 0.7152 * color[..., 1] + 0.0722 * color[..., 2]
    # the second moment of a sample variance of r * y^2; one pixel in five lies below n * y^2 (a negative variance, clamped)
    r = np.where(rng.uniform(size=(h, w)) < 0.2, rng.uniform(-0.5, -0.01, (h, w)), rng.uniform(0.0, 1.0, (h, w)))
    q = count.astype(np.float64) * (y * y) * (1.0 + r)
    feat = np.zeros((h, w, 7))
    feat[..., 0:3] = _draw(rng, ALBEDOS, 3 * n).reshape(h, w, 3)
    nn = rng.normal(size=(h, w, 3))
    nn /= np.sqrt((nn * nn).sum(-1))[..., None]
    nn[rng.uniform(size=(h, w)) < 0.15] = 0.0  # a medium event or a miss
    feat[..., 3:6] = nn
    feat[..., 6] = _draw(rng, DEPTHS, n).reshape(h, w)
    hole = count == 0
    color[hole], q[hole], feat[hole] = np.nan, np.nan, np.nan
    return color, q, count, feat


def patterns(h, w):
    """the hole patterns as masks of the VALID pixels, by name (those that fit an h x w plane)"""
    yy, xx = np.mgrid[0:h, 0:w]
    out = {"checkerboard": (xx + yy) % 2 == 0}
    cy, cx = min(16, h - 1), min(15, w - 1)  # on a workgroup border where the plane has one
    out["lone_valid"] = (yy == cy) & (xx == cx)
    out["lone_hole"] = ~out["lone_valid"]
    for s in (15, 16, 17):
        if s < h - 1 and s < w - 1:
            out["seam_%d" % s] = (yy != s) & (xx != s)
    if h >= 3 and w >= 3:
        out["frame"] = (yy == 0) | (yy == h - 1) | (xx == 0) | (xx == w - 1)
    return out


# ---- the filter, from the "Filter" comment of include/rtr_hip.h --------------------------------------------------


def _lum(c):
    return 0.2126 * c[0] + 0.7152 * c[1] + 0.0722 * c[2]


def _max(a, b):
    return a if a > b else b


def _dist2(a, b):
    e = (a[0] - b[0], a[1] - b[1], a[2] - b[2])
    return e[0] * e[0] + e[1] * e[1] + e[2] * e[2]


def _prepare_pixel(m, Q, n, a):
    """(c_p, var_p) of the filter definition"""
    if n < 2:
        var = 1e30
    else:
        l = _lum(m)
        var = _max((1.0 / n) * Q - l * l, 0.0) / float(n - 1) / float(n)
    la = _max(_lum(a), 1e-3)
    var = var / (la * la)
    return [m[k] / a[k] if a[k] > 1e-3 else m[k] for k in range(3)], var


K3 = {-1: 1.0 / 4.0, 0: 1.0 / 2.0, 1: 1.0 / 4.0}
H5 = {-2: 1.0 / 16.0, -1: 4.0 / 16.0, 0: 6.0 / 16.0, 1: 4.0 / 16.0, 2: 1.0 / 16.0}


def scalar_pass(px, step, sigma_l, sigma_n, sigma_a, sigma_z):
    """one a-trous pass over ``px``: {(y, x): dict(c, var, a, nn, z)} of the valid pixels -> the same with c', var'"""
    out = {}
    for (y, x), P in px.items():
        gs = gw = 0.0
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                Q = px.get((y + dy, x + dx))
                if Q is None:
                    continue
                gs += K3[dx] * K3[dy] * Q["var"]
                gw += K3[dx] * K3[dy]
        g = gs / gw
        lp = _lum(P["c"])
        zz = _max(P["z"], 1e-3)
        l_den = sigma_l * sigma_l * g + 1e-10
        z_den = sigma_z * sigma_z * (float(step) * float(step)) * (zz * zz)
        sw = sv = 0.0
        s = [0.0, 0.0, 0.0]
        for dy in (-2, -1, 0, 1, 2):
            for dx in (-2, -1, 0, 1, 2):
                Q = px.get((y + step * dy, x + step * dx))
                if Q is None:
                    continue
                dl = lp - _lum(Q["c"])
                w_l = 1.0 / (1.0 + dl * dl / l_den)
                w_n = 1.0 / (1.0 + _dist2(P["nn"], Q["nn"]) / (sigma_n * sigma_n))
                w_a = 1.0 / (1.0 + _dist2(P["a"], Q["a"]) / (sigma_a * sigma_a))
                dz = P["z"] - Q["z"]
                w_z = 1.0 / (1.0 + dz * dz / z_den)
                wt = H5[dx] * H5[dy] * w_l * w_n * w_a * w_z
                sw += wt
                for k in range(3):
                    s[k] += wt * Q["c"][k]
                sv += wt * wt * Q["var"]
        out[(y, x)] = dict(P, c=[s[k] / sw for k in range(3)], var=sv / (sw * sw))
    return out


def scalar_denoise(color, q, count, feat, iterations, sigma_l, sigma_n, sigma_a, sigma_z):
    """the linear output (h, w, 3) of the filter; NaN where count is 0"""
    h, w = count.shape
    px = {}
    for y in range(h):
        for x in range(w):
            n = int(count[y, x])
            if n == 0:
                continue
            m = [float(v) for v in color[y, x]]
            f = [float(v) for v in feat[y, x]]
            c, var = _prepare_pixel(m, float(q[y, x]), n, f[0:3])
            px[(y, x)] = dict(c=c, var=var, a=f[0:3], nn=f[3:6], z=f[6], m=m)
    for k in range(iterations):
        px = scalar_pass(px, 2 ** k, sigma_l, sigma_n, sigma_a, sigma_z)
    out = np.full((h, w, 3), np.nan)
    for (y, x), P in px.items():
        if iterations == 0:
            out[y, x] = P["m"]
        else:
            out[y, x] = [P["c"][k] * P["a"][k] if P["a"][k] > 1e-3 else P["c"][k] for k in range(3)]
    return out


# ---- the temporal stage, from the temporal comment of include/rtr_hip.h -----------------------------------------


def _vec(cam, name):
    return [float(v) for v in np.asarray(cam[name], dtype=np.float64).reshape(3)]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else math.nan  # (NaN stays NaN; math.sqrt raises on a negative)


def scalar_blend(color, q, count, feat, hist, have, cam, prev, W, H, x0, y0, alpha_min, tau_z, tau_n, min_weight):
    """(c' (h, w, 3), var' (h, w), the history written (h, w, 10)); c' and var' are NaN where count is 0"""
    h, w = count.shape
    org, llc, hor, ver = (_vec(cam, k) for k in ("origin", "lower_left_corner", "horizontal", "vertical"))
    porg, pllc, phor, pver = (_vec(prev, k) for k in ("origin", "lower_left_corner", "horizontal", "vertical"))
    pu, pv, pw = (_vec(prev, k) for k in ("u", "v", "w"))
    c_out, v_out, new = np.full((h, w, 3), np.nan), np.full((h, w), np.nan), np.zeros((h, w, 10))
    for y in range(h):
        for x in range(w):
            n = int(count[y, x])
            if n == 0:
                continue
            i, j = x0 + x, y0 + y
            m = [float(v) for v in color[y, x]]
            f = [float(v) for v in feat[y, x]]
            a, nn, z = f[0:3], f[3:6], f[6]
            la = _max(_lum(a), 1e-3)
            c = [m[k] / a[k] if a[k] > 1e-3 else m[k] for k in range(3)]
            mu1, mu2, n_cur = _lum(m), (1.0 / n) * float(q[y, x]), float(n)
            n_new = n_cur
            found = None
            if have and z > 0.0:
                su, sv = (i + 0.5) / (W - 1), (j + 0.5) / (H - 1)
                d = [llc[k] + su * hor[k] + sv * ver[k] - org[k] for k in range(3)]
                length = _sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
                P = [org[k] + (z / length) * d[k] for k in range(3)]
                qv = [P[k] - porg[k] for k in range(3)]
                e = [pllc[k] - porg[k] for k in range(3)]
                zc = -_dot(qv, pw)
                if zc > 0.0:
                    F = -_dot(e, pw)
                    kk = F / zc
                    s = (kk * _dot(qv, pu) - _dot(e, pu)) / _dot(phor, pu)
                    t = (kk * _dot(qv, pv) - _dot(e, pv)) / _dot(pver, pv)
                    hx, hy = s * (W - 1) - 0.5, t * (H - 1) - 0.5
                    z_exp = _sqrt(_dot(qv, qv))
                    if math.isfinite(hx) and math.isfinite(hy):  # a position that is not finite has no tap in the region
                        fx0, fy0 = math.floor(hx), math.floor(hy)
                        fx, fy = hx - float(fx0), hy - float(fy0)
                        sw = 0.0
                        sums = [0.0] * 6  # c 0..2, mu1, mu2, n
                        for ty, tx, wt in ((fy0, fx0, (1.0 - fx) * (1.0 - fy)), (fy0, fx0 + 1, fx * (1.0 - fy)),
                                           (fy0 + 1, fx0, (1.0 - fx) * fy), (fy0 + 1, fx0 + 1, fx * fy)):
                            if not (x0 <= tx <= x0 + w - 1 and y0 <= ty <= y0 + h - 1):
                                continue
                            tap = [float(v) for v in hist[ty - y0, tx - x0]]
                            if not tap[5] > 0.0:
                                continue
                            if not abs(z_exp - tap[6]) <= tau_z * _max(z_exp, 1e-3):
                                continue
                            if not _dist2(nn, tap[7:10]) <= tau_n:
                                continue
                            sw += wt
                            for k in range(6):
                                sums[k] += wt * tap[k]
                        if sw >= min_weight:
                            found = [v / sw for v in sums]
            if found is not None:
                alpha = _max(n_cur / (n_cur + found[5]), alpha_min)
                c = [alpha * c[k] + (1.0 - alpha) * found[k] for k in range(3)]
                mu1 = alpha * mu1 + (1.0 - alpha) * found[3]
                mu2 = alpha * mu2 + (1.0 - alpha) * found[4]
                n_new = n_cur / alpha
            if n_new < 2.0:
                var = 1e30
            else:
                var = _max(mu2 - mu1 * mu1, 0.0) / (n_new - 1.0) / n_new
            var = var / (la * la)
            c_out[y, x], v_out[y, x] = c, var
            new[y, x] = c + [mu1, mu2, n_new, z] + nn
    return c_out, v_out, new


# ---- an analytic world for the temporal inputs: a back wall and a nearer, tilted square plate --------------------

WALL_Z = -6.0
PLATE_CENTRE = np.array([0.2, 0.1, -2.5])
PLATE_NORMAL = np.array([0.6, 0.0, 0.8])  # |n_plate - n_wall|^2 = 0.4: more than the default tau_n
PLATE_HALF = 0.8
WALL_NORMAL = np.array([0.0, 0.0, 1.0])


def world_features(cam, W, H, x0, y0, w, h):
    """feat (h, w, 7) of the pixel-centre rays of ``cam`` (a mapping of the camera's fields) over the region: depth t *
    |d| of the unnormalised ray, the surface's normal and albedo; a ray that meets nothing is a miss (albedo 1, normal
    and depth 0)"""
    org = np.asarray(cam["origin"], dtype=np.float64)
    su = ((x0 + np.arange(w)) + 0.5) / (W - 1)
    sv = ((y0 + np.arange(h)) + 0.5) / (H - 1)
    d = (np.asarray(cam["lower_left_corner"]) + su[None, :, None] * np.asarray(cam["horizontal"]) +
         sv[:, None, None] * np.asarray(cam["vertical"]) - org)
    length = np.sqrt((d * d).sum(-1))
    with np.errstate(all="ignore"):
        t_wall = (WALL_Z - org[2]) / d[..., 2]
        t_plate = ((PLATE_CENTRE - org) @ PLATE_NORMAL) / (d @ PLATE_NORMAL)
    hit = org + t_plate[..., None] * d - PLATE_CENTRE
    ex = np.cross((0.0, 1.0, 0.0), PLATE_NORMAL)
    on_plate = (t_plate > 0.0) & (np.abs(hit @ ex) <= PLATE_HALF) & (np.abs(hit[..., 1]) <= PLATE_HALF)
    on_wall = ~on_plate & (t_wall > 0.0)
    feat = np.zeros((h, w, 7))
    feat[..., 0:3] = 1.0
    feat[on_plate, 0:3], feat[on_plate, 3:6] = (0.73, 0.5, 0.25), PLATE_NORMAL
    feat[on_wall, 0:3], feat[on_wall, 3:6] = (0.5, 0.5, 0.73), WALL_NORMAL
    feat[..., 6] = np.where(on_plate, t_plate * length, np.where(on_wall, t_wall * length, 0.0))
    return feat


def world_planes(cam, W, H, x0, y0, w, h, seed, holes=0.05):
    """(color, q, count, feat) of the world seen from ``cam``: random colours and counts (from COUNTS, a share ``holes``
    of them 0 and NaN-filled) over world_features"""
    rng = np.random.default_rng(seed)
    color = rng.uniform(0.0, 2.0, (h, w, 3))
    count = _draw(rng, COUNTS[1:], h * w).reshape(h, w)
    count = np.where(rng.uniform(size=(h, w)) < holes, 0, count).astype(np.int32)
    if not (count > 0).any():
        count[0, 0] = 2
    y = 0.2126 * color[..., 0] + 0.7152 * color[..., 1] + 0.0722 * color[..., 2]
    q = count.astype(np.float64) * (y * y) * (1.0 + rng.uniform(-0.2, 1.0, (h, w)))
    feat = world_features(cam, W, H, x0, y0, w, h)
    hole = count == 0
    color[hole], q[hole], feat[hole] = np.nan, np.nan, np.nan
    return color, q, count, feat


# ---- temporal cases: (planes of this frame, history of the last one, cameras, parameters) by name ----------------

IMAGE_W, IMAGE_H = 64, 48
TEMPORAL_DEFAULTS = dict(alpha_min=0.05, tau_z=0.1, tau_n=0.25, min_weight=0.25)  # rtr_temporal_defaults


def temporal_regions():
    """name -> (x0, y0, w, h): each shape inside the image and flush with its far corner, and the whole image"""
    out = {}
    for h, w in ((1, 1), (1, 17), (17, 16), (33, 21)):
        # (under a static camera the positions of column 6 and of row 7 round to just below the pixel centre: the first
        # tap of such a pixel of the first column or row lies at x0 - 1 or y0 - 1)
        out["%dx%d_inside" % (h, w)] = (6, 7, w, h)
        out["%dx%d_corner" % (h, w)] = (IMAGE_W - w, IMAGE_H - h, w, h)
    out["whole"] = (0, 0, IMAGE_W, IMAGE_H)
    return out


def base_camera(vfov=40.0):
    import _temporal_ref as T
    return T.look_at_camera((0.3, 0.2, 5.0), (0.3, 0.2, 4.0), (0.0, 1.0, 0.0), vfov, IMAGE_W / IMAGE_H, focus_dist=4.0)


def lens_shifted(cam, dx, dy):
    """``cam`` with its image rectangle moved by (dx, dy) pixels in its own plane: every reprojected position moves by the
    same amount whatever its depth"""
    out = dict(cam)
    out["lower_left_corner"] = (cam["lower_left_corner"] - dx * cam["horizontal"] / (IMAGE_W - 1) -
                                dy * cam["vertical"] / (IMAGE_H - 1))
    return out


def previous_cameras(cam):
    """name -> the camera the history was seen from"""
    import _temporal_ref as T
    return {"static": dict(cam),
            "half_pixel": lens_shifted(cam, 0.5, 0.5),
            "pixel_and_a_quarter": lens_shifted(cam, 1.25, -1.25),
            "sideways": T.moved_camera(cam, translate=(0.35, -0.1, 0.0)),   # parallax: the plate's silhouette disoccludes
            "yaw_90": T.moved_camera(cam, yaw_deg=90.0),    # what is in front of prev lies far outside its image
            "yaw_180": T.moved_camera(cam, yaw_deg=180.0),                   # every zc <= 0
            "dolly": T.moved_camera(cam, translate=(0.0, 0.0, -8.0)),        # past the plate: its points lie behind prev
            "fov": base_camera(50.0)}


MOVES = ("static", "half_pixel", "pixel_and_a_quarter", "sideways", "yaw_90", "yaw_180", "dolly", "fov")
SPECIALS = ("depths", "hand_history", "alpha_one", "alpha_tiny", "n_below_two", "edge_depth", "edge_normal", "edge_weight_at",
            "edge_weight_above")
TEMPORAL_CASES = tuple("%s-%s" % (m, r) for m in MOVES for r in temporal_regions()) + tuple(
    "%s-%s" % (s, r) for s in SPECIALS[:5] for r in ("17x16_inside", "whole")) + tuple("%s-whole" % s for s in SPECIALS[5:])


def _first_history(prev, region, seed, holes):
    """the planes of a frame seen from ``prev`` and the history a frame on a cleared history leaves"""
    import _temporal_ref as T
    x0, y0, w, h = region
    a = world_planes(prev, IMAGE_W, IMAGE_H, x0, y0, w, h, seed, holes)
    return T.blend(*a, np.zeros((h, w, 10)), False, prev, prev, IMAGE_W, IMAGE_H, x0, y0, **TEMPORAL_DEFAULTS)[6]


def _edge_value(z_exp, z_tol, sign):
    """(a tap depth whose distance from z_exp is z_tol exactly, the next double beyond it) or None if no double is"""
    at = z_exp + sign * z_tol
    beyond = float(np.nextafter(at, sign * math.inf))
    if abs(z_exp - at) == z_tol and abs(z_exp - beyond) > z_tol:
        return at, beyond
    return None


def temporal_case(name):
    """The inputs of one frame as a dict: color, q, count, feat, hist, have, cam, prev, W, H, x0, y0 and the four
    parameters (the arguments of _temporal_ref.blend by name), plus ``marks``: pixels (y, x) of the region a case was
    built around, by what should happen there."""
    import zlib

    import _temporal_ref as T
    kind, rname = name.split("-")
    region = temporal_regions()[rname]
    x0, y0, w, h = region
    seed = zlib.crc32(name.encode())
    cam = base_camera()
    tp = dict(TEMPORAL_DEFAULTS)
    marks = {}
    edge = kind.startswith("edge_")
    holes = 0.0 if edge or kind == "n_below_two" else 0.08
    prev = previous_cameras(cam)[kind if kind in MOVES else ("static" if kind == "depths" else "half_pixel")]
    hist = _first_history(prev, region, seed, holes)
    color, q, count, feat = world_planes(cam, IMAGE_W, IMAGE_H, x0, y0, w, h, seed + 1, holes)
    rng = np.random.default_rng(seed + 2)
    valid = count > 0
    if kind == "depths":  # no history where z <= 0; 1e300 and the largest double overflow z_exp to inf, the
        # smallest double is absorbed by the origin: q = 0 and zc = 0 exactly
        z = feat[..., 6]
        z[valid] = np.where(rng.uniform(size=valid.sum()) < 0.5, z[valid],
                            _draw(rng, (0.0, -0.0, -1.0, 1e300, 1.7976931348623157e308, 5e-324), int(valid.sum())))
    elif kind == "hand_history":  # counts a frame never writes, and holes next to valid taps
        n = hist[..., 5]
        n[...] = np.where(rng.uniform(size=(h, w)) < 0.4, n, _draw(rng, (0.0, -2.0, 0.5, 1e9), h * w).reshape(h, w))
        hist[rng.uniform(size=(h, w)) < 0.1] = 0.0
    elif kind == "alpha_one":
        tp["alpha_min"] = 1.0
    elif kind == "alpha_tiny":  # n_cur / (n_cur + n_h) decides everywhere
        tp["alpha_min"] = 1e-12
    elif kind == "n_below_two":  # alpha = 1 / 1.5, n' = 1.5: the variance is 1e30
        count[valid] = 1
        q[valid] = (0.2126 * color[..., 0] + 0.7152 * color[..., 1] + 0.0722 * color[..., 2])[valid] ** 2 * 1.5
        hist[..., 5] = np.where(hist[..., 5] > 0.0, 0.5, 0.0)
    elif edge:
        args = (hist, True, cam, prev, IMAGE_W, IMAGE_H, x0, y0)
        info = T.blend(color, q, count, feat, *args, **tp)[7]
        px, py, z_exp, _ = T.reproject(cam, prev, IMAGE_W, IMAGE_H, x0, y0, feat[..., 6])
        on_wall = (feat[..., 3:6] == WALL_NORMAL).all(-1)
        # pixels three apart: the 2 x 2 taps of one are not those of another
        picks = [(y, x) for y in range(1, h - 2, 3) for x in range(1, w - 2, 3) if info["accepted"][y, x] == 4 and on_wall[y, x]]
        marks = {"at": [], "beyond": []}
        for k, (y, x) in enumerate(picks):
            ty, tx = int(math.floor(py[y, x])) - y0, int(math.floor(px[y, x])) - x0  # the first tap
            assert (hist[ty:ty + 2, tx:tx + 2, 7:10] == WALL_NORMAL).all()
            side = "at" if k % 2 == 0 else "beyond"
            if kind == "edge_depth":
                ze = float(z_exp[y, x])
                found = _edge_value(ze, tp["tau_z"] * max(ze, 1e-3), 1.0 if k % 4 < 2 else -1.0)
                if found is None:
                    continue
                hist[ty, tx, 6] = found[0] if side == "at" else found[1]
            elif kind == "edge_normal":  # |(0, 0, 1) - (e, 0, 1)|^2 = e * e, and 0.5 * 0.5 is tau_n itself
                hist[ty, tx, 7] = 0.5 if side == "at" else float(np.nextafter(0.5, 1.0))
            else:  # two taps of four are holes: sw is the sum of the other two
                hist[ty, tx + 1], hist[ty + 1, tx + 1] = 0.0, 0.0
                if len(marks["at"]) == 0:
                    marks["at"].append((y, x))
                continue
            marks[side].append((y, x))
        if kind.startswith("edge_weight"):
            y, x = marks["at"][0]
            sw = float(T.blend(color, q, count, feat, *args, **tp)[7]["sw"][y, x])
            assert 0.25 < sw < 0.75
            tp["min_weight"] = sw if kind == "edge_weight_at" else float(np.nextafter(sw, 1.0))
            marks = {"at": marks["at"]} if kind == "edge_weight_at" else {"beyond": marks["at"]}
    return dict(color=color, q=q, count=count, feat=feat, hist=hist, have=True, cam=cam, prev=prev, W=IMAGE_W, H=IMAGE_H,
                x0=x0, y0=y0, marks=marks, **tp)


def blend_args(case):
    """the arguments of _temporal_ref.blend / scalar_blend from a case"""
    return ([case[k] for k in ("color", "q", "count", "feat", "hist", "have", "cam", "prev", "W", "H", "x0", "y0")],
            {k: case[k] for k in ("alpha_min", "tau_z", "tau_n", "min_weight")})
