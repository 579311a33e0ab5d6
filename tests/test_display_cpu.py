"""The display transform (include/rtr_hip.h: rtr_display_*) without a GPU: the library exports and the header declares the
entry points, the struct layouts match _abi.py, the defaults are valid, null contexts are refused before any device call,
the exported sRGB table is the header's formula, and the numpy restatement the GPU tests hold the kernels to
(tests/_display_ref.py) is checked against itself and against RenderBuffer.to_rgb8."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _display_ref as R
import _golden as G

A = G.A
rtr = G.rtr

SYMBOLS = ("rtr_display_defaults", "rtr_display_srgb_thresholds", "rtr_display_histogram", "rtr_display_host",
           "rtr_display_device")


def test_library_exports_and_header_declares_the_entry_points():
    lib = rtr.native.lib()
    text = open(os.path.join(G.ROOT, "include", "rtr_hip.h")).read()
    declared = set(re.findall(r"\b(rtr_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    for name in SYMBOLS:
        assert name in rtr.native.EXPORTS and name in declared
        assert getattr(lib, name) is not None
    assert "typedef struct rtr_display_params" in text and "typedef struct rtr_display_result" in text
    for name, value in (("RTR_TONE_CLAMP", 0), ("RTR_TONE_REINHARD", 1), ("RTR_TONE_ACES", 2), ("RTR_ENCODE_GAMMA2", 0),
                        ("RTR_ENCODE_SRGB", 1)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, text).group(1)) == value
    assert (A.TONE_CLAMP, A.TONE_REINHARD, A.TONE_ACES, A.ENCODE_GAMMA2, A.ENCODE_SRGB) == (0, 1, 2, 0, 1)
    assert (R.TONE_CLAMP, R.TONE_REINHARD, R.TONE_ACES, R.ENCODE_GAMMA2, R.ENCODE_SRGB) == (0, 1, 2, 0, 1)
    assert int(re.search(r"#define RTR_ABI_VERSION (\d+)", text).group(1)) == 4 == A.RTR_ABI_VERSION  # new symbols only
    assert lib.rtr_abi_version() == 4


def test_struct_layout_matches_the_header(tmp_path):
    pf = ("auto_exposure", "meter_permille", "tone_curve", "encoding", "exposure", "key", "white", "reserved")
    rf = ("scale", "metered", "n_metered", "reserved")
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rtr_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(rtr_display_params), sizeof(rtr_display_result));\n' +
                   "".join('  printf(" %%zu", offsetof(rtr_display_params, %s));\n' % f for f in pf) +
                   "".join('  printf(" %%zu", offsetof(rtr_display_result, %s));\n' % f for f in rf) +
                   '  return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I" + os.path.join(G.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], stdout=subprocess.PIPE, check=True).stdout.split()]
    want = ([C.sizeof(A.DisplayParamsC), C.sizeof(A.DisplayResultC)] + [getattr(A.DisplayParamsC, f).offset for f in pf] +
            [getattr(A.DisplayResultC, f).offset for f in rf])
    assert got == want
    assert got[0] == A.DISPLAY_PARAMS_SIZE == 80 and got[1] == A.DISPLAY_RESULT_SIZE == 32


def test_defaults_are_valid():
    p = rtr.native.display_defaults()
    assert (p.auto_exposure, p.meter_permille, p.tone_curve, p.encoding) == (0, 500, A.TONE_CLAMP, A.ENCODE_GAMMA2)
    assert (p.exposure, p.key, p.white) == (1.0, 0.18, 4.0)
    assert list(p.reserved) == [0.0] * 5
    for v in (p.exposure, p.key, p.white):
        assert 0.0 < v < math.inf
    q = rtr.native.display_defaults(auto_exposure=1, tone_curve=A.TONE_ACES, white=2.5)
    assert (q.auto_exposure, q.tone_curve, q.white, q.meter_permille) == (1, A.TONE_ACES, 2.5, 500)
    with pytest.raises(TypeError):
        rtr.native.display_defaults(gamma=2.2)
    with pytest.raises(TypeError):
        rtr.native.display_defaults(reserved=1.0)
    rtr.native.lib().rtr_display_defaults(None)  # ignored
    rtr.native.lib().rtr_display_srgb_thresholds(None)  # ignored


def test_null_contexts_are_refused():
    L = rtr.native.lib()
    prm = rtr.native.display_defaults()
    img = (C.c_double * 12)()
    rgb = (C.c_uint8 * 12)(*([0xA5] * 12))
    t = (C.c_double * 12)(*([-7.0] * 12))
    hist = (C.c_uint32 * 512)(*([0xA5A5A5A5] * 512))
    n = C.c_int64(-3)
    res = A.DisplayResultC()
    assert L.rtr_display_histogram(None, 2, 2, img, 2, hist, C.byref(n)) == A.RTR_ERR_INVALID
    assert L.rtr_display_host(None, C.byref(prm), 2, 2, img, 2, rgb, t, C.byref(res)) == A.RTR_ERR_INVALID
    assert L.rtr_display_device(None, C.byref(prm), 2, 2, img, 2, rgb, t, None, 0) == A.RTR_ERR_INVALID
    assert list(rgb) == [0xA5] * 12 and list(t) == [-7.0] * 12 and set(hist) == {0xA5A5A5A5} and n.value == -3


def _ulps(a, b):
    return np.abs(np.asarray(a, dtype=np.float64).view(np.int64) - np.asarray(b, dtype=np.float64).view(np.int64))


def test_srgb_thresholds():
    s = rtr.native.srgb_thresholds()
    assert s.shape == (256,) and s.dtype == np.float64
    assert s[0] == 0.0 and s[255] == 1.0
    assert (np.diff(s) > 0.0).all()
    # the table, not the formula, defines the encoding: this only guards against a wrong formula
    assert _ulps(s, R.srgb_formula()).max() <= 4
    assert s[10] == (10 / 255.0) / 12.92 and s[11] > (11 / 255.0) / 12.92  # the linear toe ends between codes 10 and 11


def test_bin_edges_invert_the_bin_function():
    m = np.arange(R.BINS)
    edges = R.bin_edge(m)
    assert edges[0] == 2.0 ** -20 and edges[16] == 2.0 ** -19 and edges[511] == 2.0 ** 12 * (31.0 / 32.0)
    assert (np.diff(edges) > 0.0).all()
    assert np.array_equal(R.bin_of(edges), m)
    below = np.nextafter(edges, 0.0)
    assert np.array_equal(R.bin_of(below)[1:], m[1:] - 1)
    assert below[0] < 2.0 ** -20  # not metered
    img = np.stack([below[:1]] * 3, axis=-1)[None]
    assert not R.metered_mask(img).any() and R.metered_mask(np.stack([edges[:1]] * 3, axis=-1)[None]).all()
    # the top bin is open-ended
    assert R.bin_of(np.array([2.0 ** 12, np.nextafter(2.0 ** 12, 0.0), 1e300, np.inf])).tolist() == [511, 511, 511, 511]
    # 16 bins per octave
    assert np.array_equal(R.bin_of(np.array([1.0, 2.0, 4.0])), np.array([320, 336, 352]))


def test_histogram_and_scale_of_the_restatement():
    img = np.zeros((2, 3, 3))
    img[0, 0] = 1.0        # y = 1 up to rounding
    img[0, 1] = 4.0
    img[0, 2] = np.nan
    img[1, 0] = (np.inf, 0.0, 0.0)
    img[1, 1] = 2.0 ** -30  # too dark
    img[1, 2] = 4.0
    hist, n = R.histogram(img)
    assert n == 3 and hist.sum() == 3
    b1, b4 = int(R.bin_of(R.lum(img[0, 0]))), int(R.bin_of(R.lum(img[0, 1])))
    assert hist[b1] == 1 and hist[b4] == 2
    scale, metered, k = R.pick_scale(hist, 1, 333, 2.0, 0.18)  # T = 1: the first pixel
    assert k == 3 and metered == R.bin_edge(b1) and scale == (2.0 * 0.18) / metered
    scale, metered, k = R.pick_scale(hist, 1, 334, 2.0, 0.18)  # T = 2
    assert metered == R.bin_edge(b4)
    assert R.pick_scale(hist, 0, 500, 2.0, 0.18) == (2.0, 0.0, 0)
    assert R.pick_scale(np.zeros(512, dtype=np.uint32), 1, 500, 2.0, 0.18) == (2.0, 0.0, 0)


def test_gamma2_path_of_the_restatement_is_to_rgb8():
    rng = np.random.default_rng(11)
    lin = rng.uniform(0.0, 1.5, (23, 31, 3)) * rng.choice([1e-3, 1.0, 40.0], (23, 31, 1))
    lin[3, 4] = 0.0
    lin[5, 6] = 1.0
    buf = rtr.RenderBuffer(31, 23)
    buf.store_linear(lin)
    rgb8, t, res = R.display(lin, rtr.native.display_defaults(), rtr.native.srgb_thresholds())
    assert rgb8.dtype == np.uint8 and np.array_equal(rgb8, buf.to_rgb8())
    assert res == {"scale": 1.0, "metered": 0.0, "n_metered": 0}
    assert t.min() >= 0.0 and t.max() == 1.0


def test_srgb_code_of_the_restatement_brackets_the_transfer():
    s = rtr.native.srgb_thresholds()
    t = np.concatenate([s, np.nextafter(s[1:], 0.0), [0.5, 0.999999]])
    code = R.encode(t, R.ENCODE_SRGB, s)
    assert np.array_equal(code[:256], np.arange(256)) and np.array_equal(code[256:511], np.arange(255))
    assert code[-2] == 187 and code[-1] == 254  # 0.5 linear is sRGB 187.5...


def test_save_to_png_takes_display_bytes(tmp_path):
    import zlib
    buf = rtr.RenderBuffer(5, 4)
    rgb = np.arange(60, dtype=np.uint8).reshape(4, 5, 3)
    assert buf.save_to_png(str(tmp_path / "a.png"), rgb8=rgb)
    data = open(tmp_path / "a.png", "rb").read()
    idat = data.index(b"IDAT")
    n = int.from_bytes(data[idat - 4:idat], "big")
    raw = zlib.decompress(data[idat + 4:idat + 4 + n])
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(4, 16)
    assert (rows[:, 0] == 0).all() and np.array_equal(rows[:, 1:].reshape(4, 5, 3), rgb)
    with pytest.raises(ValueError):
        buf.save_to_png(str(tmp_path / "b.png"), rgb8=rgb[:3])
    assert buf.save_to_png(str(tmp_path / "c.png"))  # default behaviour: the buffer's own bytes
