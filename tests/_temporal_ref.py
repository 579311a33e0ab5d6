"""numpy restatement of the temporal stage of rtr_accum_denoise_temporal (include/rtr_hip.h), operation for operation:
only + - * / sqrt floor and compares in IEEE binary64, so it gives the device's bits.  The a-trous passes are those of
_denoise_ref.  Test infrastructure.

Planes are (H, W, ...) arrays of the region, row 0 = its lowest row; a history is (H, W, 10): demodulated colour 0..2,
mu1 3, mu2 4, effective sample count 5 (0: none), depth 6, normal 7..9.  A camera is a CAMERA_DTYPE record (or any
mapping of its fields)."""
import numpy as np

import _denoise_ref as D

HISTORY = 10


def _v(cam, name):
    return np.asarray(cam[name], dtype=np.float64).reshape(3)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def reproject(cam, prev, W, H, x0, y0, z):
    """Where the first hits of the region's pixels (depth plane ``z``, seen from ``cam``) lie in the image of ``prev``:
    (x, y, z_exp, zc) in full-image pixel coordinates; meaningful where z > 0 and zc > 0."""
    h, w = z.shape
    org, llc, hor, ver = _v(cam, "origin"), _v(cam, "lower_left_corner"), _v(cam, "horizontal"), _v(cam, "vertical")
    porg, pllc, phor, pver = _v(prev, "origin"), _v(prev, "lower_left_corner"), _v(prev, "horizontal"), _v(prev, "vertical")
    pu, pv, pw = _v(prev, "u"), _v(prev, "v"), _v(prev, "w")
    with np.errstate(all="ignore"):
        su = ((x0 + np.arange(w)).astype(np.float64) + 0.5) / np.float64(W - 1)
        sv = ((y0 + np.arange(h)).astype(np.float64) + 0.5) / np.float64(H - 1)
        su, sv = su[None, :], sv[:, None]
        d = np.stack([llc[k] + su * hor[k] + sv * ver[k] - org[k] for k in range(3)], axis=-1)
        length = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
        zl = z / length
        q = np.stack([(org[k] + zl * d[..., k]) - porg[k] for k in range(3)], axis=-1)
        e = pllc - porg
        zc = -_dot(q, pw)
        F = -_dot(e, pw)
        k = F / zc
        s = (k * _dot(q, pu) - _dot(e, pu)) / _dot(phor, pu)
        t = (k * _dot(q, pv) - _dot(e, pv)) / _dot(pver, pv)
        x = s * np.float64(W - 1) - 0.5
        y = t * np.float64(H - 1) - 0.5
        z_exp = np.sqrt(_dot(q, q))
    return x, y, z_exp, zc


def blend(color, q, count, feat, hist, have, cam, prev, W, H, x0, y0, alpha_min, tau_z, tau_n, min_weight):
    """The stage in front of the filter: (c', var', a, nn, z, valid, new history, info); info holds the masks the tests
    look at: ``has_history``, ``accepted`` (taps accepted per pixel, 0..4), ``rejected`` (taps turned down per pixel, by the
    first compare that failed: ``border`` outside the region, ``empty`` history n <= 0, ``depth``, ``normal``) and the pixels
    without history because z <= 0 (``no_depth``), zc <= 0 (``behind``) or sw < min_weight (``light``), and ``sw`` itself."""
    color = np.asarray(color, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    count = np.asarray(count)
    feat = np.asarray(feat, dtype=np.float64)
    hist = np.asarray(hist, dtype=np.float64)
    h, w = count.shape
    valid = count > 0
    a, nn, z = feat[..., 0:3], feat[..., 3:6], feat[..., 6]
    with np.errstate(all="ignore"):
        n_cur = count.astype(np.float64)
        la = D.lum(a)
        la = np.where(la > 1e-3, la, 1e-3)
        c = np.where(a > 1e-3, color / a, color)
        mu1 = D.lum(color)
        mu2 = (1.0 / n_cur) * q
        ne = n_cur
        accepted = np.zeros((h, w), dtype=np.int32)
        has = np.zeros((h, w), dtype=bool)
        rejected = {k: np.zeros((h, w), dtype=np.int32) for k in ("border", "empty", "depth", "normal")}
        no_depth = behind = light = np.zeros((h, w), dtype=bool)
        sw = np.zeros((h, w))
        if have:
            x, y, z_exp, zc = reproject(cam, prev, W, H, x0, y0, z)
            ok = valid & (z > 0.0) & (zc > 0.0)
            fx0, fy0 = np.floor(x), np.floor(y)
            fx, fy = x - fx0, y - fy0
            z_tol = tau_z * np.where(z_exp > 1e-3, z_exp, 1e-3)
            sw = np.zeros((h, w))
            hs = np.zeros((h, w, 6))  # c 0..2, mu1, mu2, n
            for tap in range(4):
                tx, ty = fx0 + float(tap & 1), fy0 + float(tap >> 1)
                inside = ok & (tx >= float(x0)) & (tx <= float(x0 + w - 1)) & (ty >= float(y0)) & (ty <= float(y0 + h - 1))
                ix = (np.where(inside, tx, float(x0)) - x0).astype(np.int64)
                iy = (np.where(inside, ty, float(y0)) - y0).astype(np.int64)
                ht = hist[iy, ix]
                has_n = ht[..., 5] > 0.0
                ez = z_exp - ht[..., 6]
                z_ok = np.where(ez < 0.0, -ez, ez) <= z_tol
                e = nn - ht[..., 7:10]
                n_ok = e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2] <= tau_n
                acc = inside & has_n & z_ok & n_ok
                # why a tap was turned down, in the order of the compares
                rejected["border"] += ok & ~inside
                rejected["empty"] += inside & ~has_n
                rejected["depth"] += inside & has_n & ~z_ok
                rejected["normal"] += inside & has_n & z_ok & ~n_ok
                wt = (fx if tap & 1 else 1.0 - fx) * (fy if tap >> 1 else 1.0 - fy)
                sw = np.where(acc, sw + wt, sw)
                hs = np.where(acc[..., None], hs + wt[..., None] * ht[..., 0:6], hs)
                accepted += acc
            has = ok & (sw >= min_weight)
            no_depth, behind, light = valid & ~(z > 0.0), valid & (z > 0.0) & ~(zc > 0.0), ok & ~(sw >= min_weight)
            n_h = hs[..., 5] / sw
            alpha = n_cur / (n_cur + n_h)
            alpha = np.where(alpha > alpha_min, alpha, alpha_min)
            beta = 1.0 - alpha
            c = np.where(has[..., None], alpha[..., None] * c + beta[..., None] * (hs[..., 0:3] / sw[..., None]), c)
            mu1 = np.where(has, alpha * mu1 + beta * (hs[..., 3] / sw), mu1)
            mu2 = np.where(has, alpha * mu2 + beta * (hs[..., 4] / sw), mu2)
            ne = np.where(has, n_cur / alpha, n_cur)
        dv = mu2 - mu1 * mu1
        var = np.where(dv > 0.0, dv, 0.0) / (ne - 1.0) / ne
        var = np.where(ne < 2.0, 1e30, var)
        var = var / (la * la)
    new = np.zeros((h, w, HISTORY))
    new[..., 0:3], new[..., 3], new[..., 4], new[..., 5], new[..., 6], new[..., 7:10] = c, mu1, mu2, ne, z, nn
    new[~valid] = 0.0
    return c, var, a, nn, z, valid, new, {"has_history": has, "accepted": accepted, "rejected": rejected, "no_depth": no_depth,
                                          "behind": behind, "light": light, "sw": sw}


def denoise_temporal(color, q, count, feat, hist, have, cam, prev, W, H, x0, y0, prm, tp):
    """(linear output (H, W, 3) with NaN where count is 0, the history after the frame, info) for an rtr_denoise_params
    ``prm`` and an rtr_temporal_params ``tp``"""
    c, var, a, nn, z, valid, new, info = blend(color, q, count, feat, hist, have, cam, prev, W, H, x0, y0, tp.alpha_min,
                                               tp.tau_z, tp.tau_n, tp.min_weight)
    for k in range(prm.iterations):
        c, var = D.atrous_pass(c, var, a, nn, z, valid, 1 << k, prm.sigma_l * prm.sigma_l, prm.sigma_n * prm.sigma_n,
                               prm.sigma_a * prm.sigma_a, prm.sigma_z * prm.sigma_z)
    with np.errstate(all="ignore"):
        out = np.asarray(color, dtype=np.float64).copy() if prm.iterations == 0 else np.where(a > 1e-3, c * a, c)
    return np.where(valid[..., None], out, np.nan), new, info


# ---- cameras for the tests -----------------------------------------------------------------------------------------

CAMERA_FIELDS = ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w", "lens_radius", "time0", "time1")


def camera_dict(cam):
    """a CAMERA_DTYPE record (or mapping) as a dict of float64 arrays / floats"""
    out = {}
    for name in CAMERA_FIELDS:
        v = np.asarray(cam[name], dtype=np.float64).reshape(-1)
        out[name] = v.copy() if len(v) == 3 else float(v[0])
    return out


def look_at_camera(lookfrom, lookat, vup, vfov_deg, aspect, focus_dist=1.0, aperture=0.0, time0=0.0, time1=0.0):
    """the reference's camera constructor (renderer/camera.h) in numpy"""
    lookfrom, lookat, vup = (np.asarray(x, dtype=np.float64) for x in (lookfrom, lookat, vup))
    hh = np.tan(np.deg2rad(vfov_deg) / 2)
    vh, vw = 2.0 * hh, aspect * 2.0 * hh
    w = lookfrom - lookat
    w = w / np.sqrt(w @ w)
    u = np.cross(vup, w)
    u = u / np.sqrt(u @ u)
    v = np.cross(w, u)
    hor, ver = focus_dist * vw * u, focus_dist * vh * v
    return {"origin": lookfrom, "lower_left_corner": lookfrom - hor / 2 - ver / 2 - focus_dist * w, "horizontal": hor,
            "vertical": ver, "u": u, "v": v, "w": w, "lens_radius": aperture / 2, "time0": float(time0), "time1": float(time1)}


def moved_camera(cam, translate=(0.0, 0.0, 0.0), yaw_deg=0.0):
    """``cam`` moved by ``translate`` and turned by ``yaw_deg`` about the world y axis through its origin"""
    c = camera_dict(cam)
    a = np.deg2rad(yaw_deg)
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    org = c["origin"] + np.asarray(translate, dtype=np.float64)
    out = dict(c)
    out["lower_left_corner"] = org + R @ (c["lower_left_corner"] - c["origin"])
    out["origin"] = org
    for k in ("horizontal", "vertical", "u", "v", "w"):
        out[k] = R @ c[k]
    return out


def camera_record(cam):
    """a camera mapping as a one-element CAMERA_DTYPE array (what Scene.camera holds)"""
    from _golden import A
    rec = np.zeros(1, dtype=A.CAMERA_DTYPE)
    for name in CAMERA_FIELDS:
        rec[name][0] = cam[name]
    return rec


def scene_with_camera(sc, cam):
    """a copy of the flattened scene ``sc`` whose camera is ``cam``"""
    out = type(sc).from_bytes(sc.to_bytes())
    out.camera[:] = camera_record(cam)
    return out
