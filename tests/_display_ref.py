"""numpy restatement of the display transform (include/rtr_hip.h: rtr_display_*): metering, scale, tone curves and both
encodings in the header's operation order.  numpy float64 is IEEE binary64 and every step is + - * / sqrt, a compare or
an integer bit operation, so the kernels are held to these bits.  Test infrastructure only."""
import numpy as np

BINS = 512
BIAS = 0x3EB0  # bits(2^-20) >> 48
TONE_CLAMP, TONE_REINHARD, TONE_ACES = 0, 1, 2
ENCODE_GAMMA2, ENCODE_SRGB = 0, 1


def lum(c):
    """0.2126 * c.x + 0.7152 * c.y + 0.0722 * c.z, left to right"""
    with np.errstate(all="ignore"):
        return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def bin_of(y):
    """the bin of luminances that are metered (y >= 2^-20, not NaN)"""
    y = np.array(y, dtype=np.float64)  # a contiguous copy of the same shape
    m = (y.view(np.uint64) >> np.uint64(48)).astype(np.int64) - BIAS
    return np.where(y >= 2.0 ** 12, BINS - 1, m)


def bin_edge(m):
    """the lower edge of bin m: the double with bits (m + 0x3EB0) << 48"""
    return (np.asarray(np.asarray(m, dtype=np.int64) + BIAS, dtype=np.uint64) << np.uint64(48)).view(np.float64)


def metered_mask(img):
    img = np.asarray(img, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.isfinite(img).all(axis=-1) & (lum(img) >= 2.0 ** -20)


def histogram(img):
    """(the 512 counts, n_metered) of an (H, W, 3) image"""
    img = np.asarray(img, dtype=np.float64)
    mask = metered_mask(img)
    hist = np.bincount(bin_of(lum(img)[mask]), minlength=BINS).astype(np.uint32)
    assert len(hist) == BINS
    return hist, int(mask.sum())


def pick_scale(hist, auto_exposure, meter_permille, exposure, key):
    """(scale, metered, n_metered) from a histogram"""
    if not auto_exposure:
        return np.float64(exposure), np.float64(0.0), 0
    n = int(np.asarray(hist, dtype=np.int64).sum())
    if n == 0:
        return np.float64(exposure), np.float64(0.0), 0
    T = (n * int(meter_permille) + 999) // 1000
    m = int(np.searchsorted(np.cumsum(np.asarray(hist, dtype=np.int64)), T, side="left"))
    metered = np.float64(bin_edge(m))
    with np.errstate(all="ignore"):
        return (np.float64(exposure) * np.float64(key)) / metered, metered, n


def tone(x, curve, white):
    with np.errstate(all="ignore"):
        if curve == TONE_REINHARD:
            white = np.float64(white)
            u = x * (1.0 + x / (white * white)) / (1.0 + x)
        elif curve == TONE_ACES:
            u = (x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14)
        else:
            u = x
        return np.where(u > 0.0, np.where(u < 1.0, u, 1.0), 0.0)


def encode(t, encoding, thresholds):
    if encoding == ENCODE_SRGB:
        return np.searchsorted(np.asarray(thresholds, dtype=np.float64)[1:], t, side="right").astype(np.uint8)
    return (np.sqrt(t) * 255).astype(np.uint8)


def srgb_formula():
    """the 256 thresholds by the header's formula (numpy's pow: within a few ulp of the library's table)"""
    v = np.arange(256) / 255.0
    s = np.where(v <= 0.04045, v / 12.92, np.power((v + 0.055) / 1.055, 2.4))
    s[0] = 0.0
    return s


def display(img, p, thresholds):
    """(rgb8 with the TOP row first, t in the input's row order, dict(scale, metered, n_metered)) of an (H, W, 3) image
    whose row 0 is the lowest row; ``p`` has the fields of rtr_display_params"""
    img = np.asarray(img, dtype=np.float64)
    hist = histogram(img)[0] if p.auto_exposure else None
    scale, metered, n = pick_scale(hist, p.auto_exposure, p.meter_permille, p.exposure, p.key)
    with np.errstate(all="ignore"):
        x = np.where(np.isfinite(img) & (img > 0.0), np.minimum(scale * img, 1e30), 0.0)
    t = tone(x, p.tone_curve, p.white)
    rgb8 = encode(t, p.encoding, thresholds)[::-1]
    return np.ascontiguousarray(rgb8), t, {"scale": float(scale), "metered": float(metered), "n_metered": n}
