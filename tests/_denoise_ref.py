"""numpy restatement of the a-trous denoiser of rtr_accum_denoise / rtr_denoise_host (include/rtr_hip.h), operation for
operation: only + - * / sqrt and compares in IEEE binary64, so it gives the device's bits.  Test infrastructure."""
import numpy as np

K3 = (0.25, 0.5, 0.25)
H5 = (0.0625, 0.25, 0.375, 0.25, 0.0625)


def lum(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def _shift(x, dx, dy):
    """s[y, x] = x[y + dy, x + dx] where that is inside the array, else zero (False)"""
    out = np.zeros_like(x)
    h, w = x.shape[:2]
    ny, nx = h - abs(dy), w - abs(dx)
    if ny <= 0 or nx <= 0:
        return out
    out[max(0, -dy):max(0, -dy) + ny, max(0, -dx):max(0, -dx) + nx] = x[max(0, dy):max(0, dy) + ny, max(0, dx):max(0, dx) + nx]
    return out


def prepare(color, q, count, feat):
    """(demodulated colour, variance of the mean / lum(albedo)^2, albedo, normal, depth, valid)"""
    valid = count > 0
    n = count.astype(np.float64)
    a, nn, z = feat[..., 0:3], feat[..., 3:6], feat[..., 6]
    with np.errstate(all="ignore"):
        scale = 1.0 / n
        ym = lum(color)
        d = scale * q - ym * ym
        var = np.where(d > 0.0, d, 0.0) / (n - 1.0) / n
        var = np.where(count >= 2, var, 1e30)
        la = lum(a)
        la = np.where(la > 1e-3, la, 1e-3)
        var = var / (la * la)
        c = np.where(a > 1e-3, color / a, color)
    return c, var, a, nn, z, valid


def atrous_pass(c, var, a, nn, z, valid, step, sl2, sn2, sa2, sz2):
    with np.errstate(all="ignore"):
        gs = np.zeros_like(var)
        gw = np.zeros_like(var)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                m = _shift(valid, dx, dy)
                wk = K3[dx + 1] * K3[dy + 1]
                gs = gs + np.where(m, wk * _shift(var, dx, dy), 0.0)
                gw = gw + np.where(m, wk, 0.0)
        g = gs / gw
        lp = lum(c)
        l_den = sl2 * g + 1e-10
        zz = np.where(z > 1e-3, z, 1e-3)
        z_den = sz2 * (float(step) * float(step)) * (zz * zz)
        sw = np.zeros_like(var)
        s = np.zeros_like(c)
        sv = np.zeros_like(var)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ox, oy = step * dx, step * dy
                m = _shift(valid, ox, oy)
                cq, vq, aq, nq, zq = (_shift(x, ox, oy) for x in (c, var, a, nn, z))
                dl = lp - lum(cq)
                wl = 1.0 / (1.0 + dl * dl / l_den)
                e = nn - nq
                wn = 1.0 / (1.0 + (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2]) / sn2)
                f = a - aq
                wa = 1.0 / (1.0 + (f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1] + f[..., 2] * f[..., 2]) / sa2)
                ez = z - zq
                wz = 1.0 / (1.0 + ez * ez / z_den)
                wt = H5[dx + 2] * H5[dy + 2] * wl * wn * wa * wz
                sw = sw + np.where(m, wt, 0.0)
                s = s + np.where(m[..., None], wt[..., None] * cq, 0.0)
                sv = sv + np.where(m, wt * wt * vq, 0.0)
        return s / sw[..., None], sv / (sw * sw)


def denoise(color, q, count, feat, iterations, sigma_l, sigma_n, sigma_a, sigma_z):
    """Linear output (H, W, 3) of the region (row 0 = its lowest row); pixels with count 0 are NaN (the device leaves
    them alone).  Inputs as rtr_denoise_host takes them."""
    color = np.asarray(color, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    count = np.asarray(count)
    feat = np.asarray(feat, dtype=np.float64)
    c, var, a, nn, z, valid = prepare(color, q, count, feat)
    for k in range(iterations):
        c, var = atrous_pass(c, var, a, nn, z, valid, 1 << k, sigma_l * sigma_l, sigma_n * sigma_n,
                             sigma_a * sigma_a, sigma_z * sigma_z)
    out = color.copy() if iterations == 0 else np.where(a > 1e-3, c * a, c)
    return np.where(valid[..., None], out, np.nan)


def denoise_params(prm):
    """the keyword arguments of ``denoise`` from an rtr_denoise_params"""
    return dict(iterations=prm.iterations, sigma_l=prm.sigma_l, sigma_n=prm.sigma_n, sigma_a=prm.sigma_a,
                sigma_z=prm.sigma_z)


def rgb8(linear):
    """the 8-bit store of k_accum_resolve, Y flipped (top row first)"""
    with np.errstate(invalid="ignore"):
        g = np.sqrt(linear)
        g = np.where(g < 0.0, 0.0, np.where(g > 1.0, 1.0, g))
        return (g * 255).astype(np.uint8)[::-1]
