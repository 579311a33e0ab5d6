"""Numpy / Python restatement of the light probes, written from the contract in include/rtr_hip.h (rtr_probe_*, rtr_sh_*):
the sphere direction, the nine basis functions, the projection and its reduction, the irradiance of a normal and the
grid lookup.  Only + - * / sqrt and compares, in the header's operation order, so the bits are the library's.  The seed,
xorshift32 and the reduction are the gathers' (tests/_gather_ref.py).  Test infrastructure only."""
import numpy as np

import _gather_ref as GR

K0 = 0.28209479177387814
K1 = 0.4886025119029199
K2 = 1.0925484305920792
K3 = 0.31539156525252005
K4 = 0.5462742152960396
A_BAND = (3.141592653589793,) + (2.0943951023931953,) * 3 + (0.7853981633974483,) * 5
FOUR_PI = 12.566370614359172


def rays(n_points, samples, seed=0, point_base=0):
    """(directions [n, N, 3], generator states after the draws [n, N] uint32) of every sample of every probe: the
    rejection loop of the gathers (draws z, y, x), then unit; no normal, no near_zero step"""
    n = int(n_points)
    k = (np.arange(n, dtype=np.uint64) + np.uint64(point_base)) & GR.M32
    state = GR.sample_seed(seed, k[:, None], np.arange(samples, dtype=np.uint64)[None, :])
    ux = np.zeros((n, samples))
    uy = np.zeros((n, samples))
    uz = np.zeros((n, samples))
    todo = np.ones((n, samples), dtype=bool)
    while todo.any():
        s = state[todo]
        s = GR.xorshift(s)
        z = -1.0 + s.astype(np.float64) * 2.0 ** -31
        s = GR.xorshift(s)
        y = -1.0 + s.astype(np.float64) * 2.0 ** -31
        s = GR.xorshift(s)
        x = -1.0 + s.astype(np.float64) * 2.0 ** -31
        state[todo] = s
        ux[todo], uy[todo], uz[todo] = x, y, z
        rejected = x * x + y * y + z * z >= 1
        idx = np.flatnonzero(todo)
        todo.flat[idx[~rejected]] = False
    r = 1.0 / np.sqrt(ux * ux + uy * uy + uz * uz)
    return np.stack([r * ux, r * uy, r * uz], axis=-1), state.astype(np.uint32)


def basis(d):
    """Y [..., 9] of directions d [..., 3]"""
    d = np.asarray(d, dtype=np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([K0 + 0.0 * x, K1 * y, K1 * z, K1 * x, K2 * (x * y), K2 * (y * z), K3 * (3.0 * (z * z) - 1.0),
                     K2 * (x * z), K4 * (x * x - y * y)], axis=-1)


def visibility(directions, blocked):
    """(count [n], c [n, 9]) of rtr_probe_visibility from the directions [n, N, 3] and the blocked flags [n, N]"""
    open_ = ~np.asarray(blocked, dtype=bool)
    x = np.where(open_[..., None], basis(directions), 0.0)
    return GR.reduce(open_.astype(np.int32), divide=False), GR.reduce(x)


def radiance(directions, L):
    """c [n, 9, 3] of rtr_probe_radiance from the directions [n, N, 3] and the radiance of every ray [n, N, 3]"""
    return GR.reduce(basis(directions)[..., :, None] * np.asarray(L, dtype=np.float64)[..., None, :])


def irradiance(c, normal):
    """rtr_sh_irradiance of c [9, 3] for one normal [3] (need not be normalised)"""
    c = np.asarray(c, dtype=np.float64)
    n = np.asarray(normal, dtype=np.float64)
    r = 1.0 / np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
    y = basis(np.array([r * n[0], r * n[1], r * n[2]]))
    E = np.zeros(3)
    for ch in range(3):
        e = 0.0
        for i in range(9):
            e = e + (A_BAND[i] * y[i]) * c[i, ch]
        E[ch] = FOUR_PI * e
    return E


def axis(p, origin, spacing, dim):
    """(i0, w0, w1) of one axis of the grid lookup"""
    f = (p - origin) / spacing
    f = min(max(f, 0.0), float(dim - 1))
    i0 = int(f)
    if i0 > dim - 2:
        i0 = max(dim - 2, 0)
    t = f - float(i0)
    if dim == 1:
        t = 0.0
    return i0, 1.0 - t, t


def lookup(origin, spacing, dims, probes, points, normals):
    """rtr_probe_lookup: a GATHER_OUT_DTYPE array for the queries (points [n, 3], normals [n, 3]) in the grid whose probes
    (PROBE_SH_DTYPE, dims[0] * dims[1] * dims[2] of them) lie in the header's order"""
    import _golden as G
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    normals = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(len(points), dtype=G.A.GATHER_OUT_DTYPE)
    for q in range(len(points)):
        ax = [axis(float(points[q, a]), float(origin[a]), float(spacing[a]), int(dims[a])) for a in range(3)]
        wsum, used = 0.0, 0
        acc = np.zeros((9, 3))
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    ix = min(ax[0][0] + dx, dims[0] - 1)
                    iy = min(ax[1][0] + dy, dims[1] - 1)
                    iz = min(ax[2][0] + dz, dims[2] - 1)
                    w = (ax[0][1 + dx] * ax[1][1 + dy]) * ax[2][1 + dz]
                    probe = probes[ix + dims[0] * (iy + dims[1] * iz)]
                    if w > 0 and probe["valid"] != 0:
                        wsum = wsum + w
                        acc = acc + w * probe["c"]
                        used += 1
        if used:
            out["v"][q] = irradiance((1.0 / wsum) * acc, normals[q])
            out["count"][q], out["valid"][q] = used, 1
    return out


def displaced_points(sid, distance, n=48):
    """the first ``n`` golden hit points of scene ``sid``, moved ``distance`` along their normal into free space"""
    p, nrm = GR.golden_points(sid, n)
    return p + distance * nrm
