"""Numpy / Python restatement of the environment captures, written from the contract in include/rtr_hip.h (rtr_capture_*,
rtr_cube_*, rtr_latlong_direction, rtr_write_rgbe): the ray through a texel, the reduction, the cube lookup and the RGBE
bytes.  Only + - * / sqrt and compares, in the header's operation order, so the bits are the library's.  The xorshift32
step and the reduction are the gathers' (tests/_gather_ref.py).  Test infrastructure only."""
import math

import numpy as np

import _gather_ref as GR

M32 = GR.M32


def sample_seed(seed, width, i, j, s):
    """rtr_sample_seed_inline(seed, width, i, j, s) of include/rtr_seed.h on uint64 arrays: pixel = j * width + i mod 2^32"""
    u = GR._u64
    pix = ((u(j) & M32) * np.uint64(width) + (u(i) & M32)) & M32
    h = GR.mix32((pix * np.uint64(0x9E3779B1) & M32) + (u(s) * np.uint64(0x85EBCA77) & M32) + np.uint64(0xC2B2AE3D)
                 + ((np.uint64(seed) & M32) * np.uint64(0x27D4EB2F) & M32))
    return np.where(h == 0, np.uint64(0x9E3779B9), h)


def rays(n_centres, face_size, samples, seed=0, point_base=0, jitter=1):
    """(directions [n, 6, S, S, N, 3], generator states after the draws [n, 6, S, S, N] uint32) of every ray of a capture;
    axes: centre, face f, row b, column a, sample s"""
    n, S, N = int(n_centres), int(face_size), int(samples)
    k = ((np.arange(n, dtype=np.uint64) + np.uint64(point_base)) & M32).reshape(n, 1, 1, 1, 1)
    f = np.arange(6, dtype=np.uint64).reshape(1, 6, 1, 1, 1)
    b = np.arange(S, dtype=np.uint64).reshape(1, 1, S, 1, 1)
    a = np.arange(S, dtype=np.uint64).reshape(1, 1, 1, S, 1)
    s = np.arange(N, dtype=np.uint64).reshape(1, 1, 1, 1, N)
    e = (f * np.uint64(S) + b) * np.uint64(S) + a
    state = np.broadcast_to(sample_seed(seed, 6 * S * S, e, k, s), (n, 6, S, S, N)).copy()
    if jitter:
        state = GR.xorshift(state)
        ju = state.astype(np.float64) * 2.0 ** -32
        state = GR.xorshift(state)
        jv = state.astype(np.float64) * 2.0 ** -32
    else:
        ju = jv = np.full(state.shape, 0.5)
    u = (2.0 * (a.astype(np.float64) + ju)) / float(S) - 1.0
    v = (2.0 * (b.astype(np.float64) + jv)) / float(S) - 1.0
    one = np.ones_like(u)
    table = ((one, -v, -u), (-one, -v, u), (u, one, v), (u, -one, -v), (u, -v, one), (-u, -v, -one))
    d0 = np.zeros(state.shape + (3,))
    for face in range(6):
        for axis in range(3):
            d0[:, face, ..., axis] = table[face][axis][:, face]
    x, y, z = d0[..., 0], d0[..., 1], d0[..., 2]
    r = 1.0 / np.sqrt(x * x + y * y + z * z)
    return np.stack([r * x, r * y, r * z], axis=-1), state.astype(np.uint32)


def reduce(L):
    """The mean radiance [n, 6, S, S, 3] of the capture whose rays returned L [n, 6, S, S, N, 3]: the gathers' reduction per
    texel"""
    L = np.asarray(L, dtype=np.float64)
    shape = L.shape
    return GR.reduce(L.reshape((-1,) + shape[-2:])).reshape(shape[:-2] + (3,))


def _axis(c, S):
    """(i0, w0, w1) of one face axis of the lookup"""
    g = ((c + 1.0) * float(S)) * 0.5 - 0.5
    g = min(max(g, 0.0), float(S - 1))
    i0 = int(g)
    if i0 > S - 2:
        i0 = max(S - 2, 0)
    t = g - float(i0)
    if S == 1:
        t = 0.0
    return i0, 1.0 - t, t


def face_uv(d):
    """(face, u, v) of a finite direction of non-zero length, or None"""
    x, y, z = (float(c) for c in d)
    if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
        return None
    with np.errstate(over="ignore"):
        length = float(np.sqrt(np.float64(x) * x + np.float64(y) * y + np.float64(z) * z))
    if not (0.0 < length < math.inf):
        return None
    ax, ay, az = abs(x), abs(y), abs(z)
    if ax >= ay and ax >= az:
        return (0, -z / ax, -y / ax) if x > 0 else (1, z / ax, -y / ax)
    if ay >= az:
        return (2, x / ay, z / ay) if y > 0 else (3, x / ay, -z / ay)
    return (4, x / az, -y / az) if z > 0 else (5, -x / az, -y / az)


def lookup_one(texels, d):
    """rtr_cube_lookup_one: (v [3], count, valid) of the capture ``texels`` (GATHER_OUT_DTYPE [6, S, S]) along d"""
    S = texels.shape[1]
    fuv = face_uv(d)
    if fuv is None:
        return np.zeros(3), 0, 0
    f, u, v = fuv
    ia0, *wa = _axis(u, S)
    ib0, *wb = _axis(v, S)
    acc = np.zeros(3)
    used, ok = 0, True
    for db in range(2):
        for da in range(2):
            ia, ib = min(ia0 + da, S - 1), min(ib0 + db, S - 1)
            w = wa[da] * wb[db]
            if w > 0:
                t = texels[f, ib, ia]
                ok = ok and t["valid"] != 0
                used += 1
                acc = acc + w * t["v"]
    if not ok:
        return np.zeros(3), 0, 0
    return acc, used, 1


def lookup(texels, directions):
    """rtr_cube_lookup: a GATHER_OUT_DTYPE array for the directions [n, 3]"""
    out = np.zeros(len(directions), dtype=texels.dtype)
    with np.errstate(invalid="ignore"):  # an invalid texel may hold NaN: its product is never the result
        for k, d in enumerate(directions):
            out["v"][k], out["count"][k], out["valid"][k] = lookup_one(texels, d)
    return out


def latlong_direction(W, H, i, j):
    u, v = (i + 0.5) / W, (j + 0.5) / H
    phi, theta = 2.0 * math.pi * u - math.pi, math.pi * v
    return np.array([math.sin(theta) * math.cos(phi), math.cos(theta), -math.sin(theta) * math.sin(phi)])


def rgbe_bytes(rgb):
    """The bytes of rtr_write_rgbe for the image rgb [H, W, 3]"""
    rgb = np.asarray(rgb, dtype=np.float64)
    H, W = rgb.shape[:2]
    out = bytearray(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (H, W))
    for j in range(H):
        for i in range(W):
            c = [float(x) if x > 0.0 else 0.0 for x in rgb[j, i]]  # negative and NaN: 0
            m = max(c)
            if m < 1e-32:
                out += bytes(4)
            elif not m < 2.0 ** 127:
                out += bytes([255] * 4)
            else:
                f, e = math.frexp(m)
                scale = (f * 256.0) / m
                out += bytes([min(int(x * scale), 255) for x in c] + [e + 128])
    return bytes(out)


def rgbe_decode(data):
    """(H, W, 3) float64 of the texels a reader gets from the bytes of a flat-scanline file: byte * 2^(e - 136), 0 for e = 0"""
    head, _, body = data.partition(b"\n\n")
    assert head.split(b"\n")[0] == b"#?RADIANCE" and b"FORMAT=32-bit_rle_rgbe" in head
    line, _, texels = body.partition(b"\n")
    parts = line.split()
    assert parts[0] == b"-Y" and parts[2] == b"+X"
    H, W = int(parts[1]), int(parts[3])
    q = np.frombuffer(texels, dtype=np.uint8).reshape(H, W, 4).astype(np.float64)
    scale = np.where(q[..., 3] == 0, 0.0, 2.0 ** (q[..., 3] - 136.0))
    return q[..., :3] * scale[..., None]
