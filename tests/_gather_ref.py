"""Numpy / Python restatement of the hemisphere gathers, written from the contract in include/rtr_hip.h (rtr_gather_*):
the per-sample seed, xorshift32, the ray direction, and the reduction order.  Only + - * / sqrt and compares, in the
header's operation order, so the bits are the library's.  Test infrastructure only."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def mix32(h):
    """murmur3 finalizer of include/rtr_seed.h on uint32 values held in uint64 arrays"""
    h = _u64(h) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def sample_seed(seed, k, s):
    """rtr_sample_seed_inline(seed, 1, 0, (int32_t)k, s): pixel index = k modulo 2^32"""
    pix = _u64(k) & M32
    h = mix32((pix * np.uint64(0x9E3779B1) & M32) + (_u64(s) * np.uint64(0x85EBCA77) & M32) + np.uint64(0xC2B2AE3D)
              + ((np.uint64(seed) & M32) * np.uint64(0x27D4EB2F) & M32))
    return np.where(h == 0, np.uint64(0x9E3779B9), h)


def xorshift(s):
    s = s ^ ((s << np.uint64(13)) & M32)
    s = s ^ (s >> np.uint64(17))
    s = s ^ ((s << np.uint64(5)) & M32)
    return s


def _unit(x, y, z):
    r = 1.0 / np.sqrt(x * x + y * y + z * z)
    return r * x, r * y, r * z


def group_size(n_samples):
    g = 1
    while g < 64 and g < n_samples:
        g *= 2
    return g


def rays(points, normals, samples, seed=0, point_base=0):
    """(directions [n, N, 3], generator states after the draws [n, N] uint32) of every sample of every point"""
    normals = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    n = len(normals)
    k = (np.arange(n, dtype=np.uint64) + np.uint64(point_base)) & M32
    state = sample_seed(seed, k[:, None], np.arange(samples, dtype=np.uint64)[None, :])
    wx, wy, wz = _unit(normals[:, 0], normals[:, 1], normals[:, 2])
    ux = np.zeros((n, samples))
    uy = np.zeros((n, samples))
    uz = np.zeros((n, samples))
    todo = np.ones((n, samples), dtype=bool)
    while todo.any():  # the rejection loop: z, y, x draws until the point lies inside the unit ball
        s = state[todo]
        s = xorshift(s)
        z = -1.0 + s.astype(np.float64) * 2.0 ** -31
        s = xorshift(s)
        y = -1.0 + s.astype(np.float64) * 2.0 ** -31
        s = xorshift(s)
        x = -1.0 + s.astype(np.float64) * 2.0 ** -31
        state[todo] = s
        ux[todo], uy[todo], uz[todo] = x, y, z
        rejected = x * x + y * y + z * z >= 1
        idx = np.flatnonzero(todo)
        todo.flat[idx[~rejected]] = False
    ux, uy, uz = _unit(ux, uy, uz)
    sx, sy, sz = wx[:, None] + ux, wy[:, None] + uy, wz[:, None] + uz
    near = (np.abs(sx) < 1e-8) & (np.abs(sy) < 1e-8) & (np.abs(sz) < 1e-8)
    sx = np.where(near, wx[:, None], sx)
    sy = np.where(near, wy[:, None], sy)
    sz = np.where(near, wz[:, None], sz)
    dx, dy, dz = _unit(sx, sy, sz)
    return np.stack([dx, dy, dz], axis=-1), state.astype(np.uint32)


def reduce(x, divide=True):
    """The contract's reduction of x [n, N, ...] over its sample axis: lanes of G = min(64, bit_ceil(N)) take the samples
    l, l + G, ... in order (rows of a [ceil(N / G), G] reshape, added sequentially), then the xor butterfly, then
    (1.0 / N) * a unless not ``divide`` (integer counts)."""
    x = np.asarray(x)
    n, N = x.shape[:2]
    g = group_size(N)
    rows = -(-N // g)
    pad = np.zeros((n, rows * g) + x.shape[2:], dtype=x.dtype)  # lanes without a sample carry +0.0 / 0
    pad[:, :N] = x
    pad = pad.reshape((n, rows, g) + x.shape[2:])
    a = np.zeros((n, g) + x.shape[2:], dtype=x.dtype)
    for r in range(rows):
        a = a + pad[:, r]
    lane = np.arange(g)
    off = g // 2
    while off >= 1:
        a = a + a[:, lane ^ off]
        off //= 2
    return (1.0 / N) * a[:, 0] if divide else a[:, 0]


def reduce_scalar(xs):
    """The same for one point and one component, as a plain loop over lanes written from the header's text."""
    N = len(xs)
    g = group_size(N)
    a = [0.0] * g
    for lane in range(g):
        s = lane
        while s < N:
            a[lane] = a[lane] + float(xs[s])
            s += g
    off = g // 2
    while off >= 1:
        a = [a[lane] + a[lane ^ off] for lane in range(g)]
        off //= 2
    return (1.0 / N) * a[0]


def hit_records(points, directions, states, t_min=0.001, t_max=np.inf, time=0.0):
    """HIT_DTYPE input records (flattened [n * N]) of the gather rays, for the oracle's rto_hits"""
    import _golden as G
    n, N = directions.shape[:2]
    recs = np.zeros(n * N, dtype=G.A.HIT_DTYPE)
    recs["o"] = np.repeat(np.asarray(points, dtype=np.float64).reshape(-1, 3), N, axis=0)
    recs["d"] = directions.reshape(-1, 3)
    recs["time"], recs["t_min"], recs["t_max"] = time, t_min, t_max
    recs["rng_in"] = states.reshape(-1)
    return recs


def oracle_blocked(scene, points, normals, samples, seed=0, t_min=0.001, t_max=np.inf, point_base=0):
    """(directions [n, N, 3], blocked [n, N]) with ``blocked`` from the pinned CPU oracle's closest hit of every ray"""
    import _golden as G
    d, st = rays(points, normals, samples, seed, point_base)
    ora = G.oracle_records(scene, "rto_hits", hit_records(points, d, st, t_min, t_max))
    return d, (ora["hit"] == 1).reshape(len(d), samples)


_POINTS = {}


def golden_points(sid, n=48):
    """(p, n) of the first ``n`` hits of the reference's own hit vectors of golden scene ``sid``"""
    import _golden as G
    if (sid, n) not in _POINTS:
        gold = G.records("hits_scene%02d.bin" % sid, G.A.HIT_DTYPE)
        gold = gold[gold["hit"] == 1][:n]
        assert len(gold) == n
        _POINTS[sid, n] = (gold["p"].copy(), gold["n"].copy())
    return _POINTS[sid, n]


def occlusion(directions, blocked):
    """(count [n], v [n, 3]) of an occlusion gather from the directions [n, N, 3] and the blocked flags [n, N]"""
    open_ = ~np.asarray(blocked, dtype=bool)
    x = np.where(open_[..., None], directions, 0.0)
    return reduce(open_.astype(np.int32), divide=False), reduce(x)
