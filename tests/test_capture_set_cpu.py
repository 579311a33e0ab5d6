"""Capture sets (include/rtr_hip.h: rtr_capture_set*) without a GPU: the declarations and layouts, the rules of a set, and
the host-only rtr_capture_set_lookup_one and rtr_shade_ibl_set_one against the numpy restatement of the contract
(tests/_capture_set_ref.py) bit for bit; the old behaviour as a special case; and what box projection means, on a cube
whose texels hold the wall point they see."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _capture_set_cases as SC
import _capture_set_ref as SR
import _golden as G
import _ibl_cases as IC

rtr = G.rtr
A = rtr._abi
N = rtr.native

NAMES = ("rtr_capture_set_lookup", "rtr_capture_set_lookup_device", "rtr_capture_set_lookup_one", "rtr_shade_ibl_set",
         "rtr_shade_ibl_set_device", "rtr_shade_ibl_set_one", "rtr_preview_set", "rtr_preview_set_device")
INV = A.RTR_ERR_INVALID


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _header():
    return open(os.path.join(G.ROOT, "include", "rtr_hip.h")).read()


def _body(name):
    body = re.search(r"typedef struct %s \{[^\n]*\n(.*?)\} %s;" % (name, name), _header(), re.S).group(1)
    return " ".join(re.sub(r"/\*.*?\*/", "", body, flags=re.S).split())


def test_declared_exported_and_the_abi_version_stays():
    text = _header()
    lib = N.lib()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in N.EXPORTS
        getattr(lib, name)
    assert A.RTR_ABI_VERSION == 4 and lib.rtr_abi_version() == 4
    assert re.search(r"#define RTR_ABI_VERSION 4\b", text)


def test_struct_layouts():
    assert _body("rtr_capture_volume") == ("double centre[3]; double proxy_lo[3], proxy_hi[3]; double reach_lo[3], reach_hi[3]; "
                                           "double fade;")
    assert _body("rtr_capture_set") == "int32_t n_captures, fallback; const rtr_capture_volume* volumes;"
    assert _body("rtr_capture_query") == "double p[3], d[3], alpha, pad;"
    assert C.sizeof(A.CaptureVolumeC) == 128 == A.CAPTURE_VOLUME_DTYPE.itemsize and C.sizeof(A.CaptureSetC) == 16
    assert A.CAPTURE_QUERY_DTYPE.itemsize == 64
    assert list(A.CAPTURE_VOLUME_DTYPE.names) == [n for n, _ in A.CaptureVolumeC._fields_]
    assert list(A.CAPTURE_QUERY_DTYPE.names) == ["p", "d", "alpha", "pad"]


# ---- bits ----

@pytest.mark.parametrize("fallback", (-1, 0))
@pytest.mark.parametrize("chain", SC.CHAINS)
@pytest.mark.parametrize("count", SC.COUNTS)
def test_lookup_one_equals_the_restatement(count, chain, fallback):
    vols = SC.volumes(count)
    levels, rec = SC.records(count, chain)
    q = SC.queries(count, chain[0], 64)
    if fallback >= 0:
        fallback = count - 1  # the last capture: the one with the invalid texel
    got = N.capture_set_lookup_host(N.capture_set(vols, fallback), levels, rec, q)
    want = SR.set_lookup(vols, fallback, levels, rec, q, A.GATHER_OUT_DTYPE)
    assert _same_bits(got, want)
    n_special, n_bad = len(SC.special_queries(count, chain[0])), len(SC.bad_queries())
    assert n_special + n_bad < 64 and got["valid"][n_special + n_bad:].any()
    bad = got[n_special:n_special + n_bad]
    assert not bad["valid"].any() and not bad["count"].any() and not bad["v"].any()  # every BAD spelling: the zero record
    # on the face of the faded volume 0: left out -- volume 1 alone takes it, or nobody; of the unfaded volume 1: taken in
    assert got["valid"][1] == (1 if fallback >= 0 else 0)
    if count >= 2:
        assert got["valid"][0] == 1 and got["count"][0] == got["count"][16]  # one capture, as where volume 0 alone reaches
        assert got["valid"][2] == 1
        assert got["count"][11] == 2 * got["count"][16]  # two captures in the overlap, one outside it
    else:
        assert got["valid"][0] == (1 if fallback >= 0 else 0)
    assert got["valid"][15] == (1 if fallback >= 0 else 0)  # nobody reaches p: the fallback, or the zero record
    if chain[0] > 1:
        assert got["valid"][17] == 0 and not got["v"][17].any()  # an invalid texel under a tap of a contributing capture
        if count > 1:
            assert got["valid"][18] == 1  # the same texel, of a capture that does not reach p: not read


def test_signed_zeros_in_d_take_no_part():
    vols = SC.volumes(2)
    levels, rec = SC.records(2, (4, 3))
    q = SC.special_queries(2, 4)[5:7]
    got = N.capture_set_lookup_host(N.capture_set(vols, -1), levels, rec, q)
    assert got["valid"].all() and _same_bits(got[0], got[1])


def test_the_sum_order_is_part_of_the_contract():
    """Two overlapping volumes with unequal weights and the same two swapped: (+0 + a) + b and (+0 + b) + a are one IEEE
    sum, so two captures can not show the order -- both orders are held to the restatement, and give the same bits.  Three
    overlapping volumes do show it: (a + b) + c against (c + a) + b differs in at least one bit over the queries."""
    chain = (4, 3)
    levels, n = SC.FR.plan(*chain)
    rng = np.random.default_rng(21)
    q = np.zeros(48, dtype=A.CAPTURE_QUERY_DTYPE)
    q["p"], q["d"], q["alpha"] = rng.uniform(0.05, 0.95, (48, 3)), rng.normal(size=(48, 3)), rng.uniform(0.0, 1.0, 48)

    def run(vols, chains):
        C_ = len(vols)
        rec = np.zeros(C_ * n, dtype=A.GATHER_OUT_DTYPE)
        for k, ch in enumerate(chains):  # chain layout -> level-major
            for S, at, _ in levels:
                F = 6 * S * S
                rec[at * C_ + k * F:at * C_ + (k + 1) * F] = ch[at:at + F]
        got = N.capture_set_lookup_host(N.capture_set(vols, -1), levels, rec, q)
        assert _same_bits(got, SR.set_lookup(vols, -1, levels, rec, q, A.GATHER_OUT_DTYPE))
        assert got["valid"].all()
        return got

    chains = []
    for k in range(3):
        ch = np.zeros(n, dtype=A.GATHER_OUT_DTYPE)
        ch["v"], ch["count"], ch["valid"] = rng.uniform(0.0, 2.0, (n, 3)), 4, 1
        chains.append(ch)
    V3 = SC.volume((0.5, 0.25, 0.625), (-3.0,) * 3, (3.0,) * 3, (-0.5,) * 3, (1.5,) * 3, 2.0)  # reaches [0, 1]^3, w < 1
    two = run(np.array([SC.V0, SC.V1]), chains[:2])
    swapped = run(np.array([SC.V1, SC.V0]), chains[1::-1])
    assert _same_bits(two, swapped)
    weights = [SR.weight(SC.V0, [float(x) for x in p]) for p in q["p"]]
    assert any(w is not None and w != 1.0 for w in weights)  # unequal weights occur: volume 1 has 1
    three = run(np.array([SC.V0, SC.V1, V3]), chains)
    rotated = run(np.array([V3, SC.V0, SC.V1]), [chains[2], chains[0], chains[1]])
    assert (three["count"] == 3 * two["count"] // 2).all()
    assert not _same_bits(three["v"], rotated["v"])
    assert np.allclose(three["v"], rotated["v"], rtol=1e-14, atol=0)


@pytest.mark.parametrize("parts", (1, 2, 3))
@pytest.mark.parametrize("chain", SC.CHAINS)
@pytest.mark.parametrize("count", SC.COUNTS)
def test_shade_set_one_equals_the_restatement(count, chain, parts):
    env = dict(SC.shade_environment(count, chain), parts=parts)
    vols = SC.volumes(count)
    fallback = count - 1 if chain[0] == 1 else -1
    q = IC.queries(env, 64)
    got = N.shade_ibl_set_one(SC.native_env(env, parts, count), N.capture_set(vols, fallback), q)
    want = SR.shade(env, vols, fallback, q, A.GATHER_OUT_DTYPE)
    assert _same_bits(got, want)
    assert got["valid"].any()
    if parts == 1:  # the set is not looked at
        assert _same_bits(got, N.shade_ibl_set_one(SC.native_env(env, parts, count), None, q))
        assert _same_bits(got, N.shade_ibl_one(SC.native_env(env, parts, count), q))


# ---- the old behaviour as a special case ----

@pytest.mark.parametrize("chain", SC.CHAINS)
def test_a_set_that_reaches_nothing_is_the_chain_lookup(chain):
    vols = SC.no_reach_volumes()
    levels, rec = SC.records(1, chain)
    q = SC.queries(1, chain[0], 64)
    got = N.capture_set_lookup_host(N.capture_set(vols, 0), levels, rec, q)
    along_d = N.cube_chain_lookup_host(levels, rec, N.cube_queries(q["d"], q["alpha"]))
    bad = np.array([SR.query_bad(x["p"], x["d"], x["alpha"]) for x in q])
    assert _same_bits(got[~bad], along_d[~bad]) and got["valid"][~bad].any()
    assert not got["valid"][bad].any()  # a non-finite p is BAD for the set alone


@pytest.mark.parametrize("parts", (2, 3))
@pytest.mark.parametrize("chain", SC.CHAINS)
def test_shading_under_a_set_that_reaches_nothing_is_the_plain_shader(chain, parts):
    env = dict(SC.shade_environment(1, chain), parts=parts)
    q = IC.queries(env, 64)
    ne = SC.native_env(env, parts, 1)
    got = N.shade_ibl_set_one(ne, N.capture_set(SC.no_reach_volumes(), 0), q)
    assert _same_bits(got, N.shade_ibl_one(ne, q)) and got["valid"].any()


# ---- meaning ----

@pytest.mark.parametrize("seed", (1, 2, 3))
def test_box_projection_returns_the_wall_point_the_ray_hits(seed):
    """A cube of half-size 1.5 captured from its centre, S = 8, one level; texel v = the wall point its centre direction
    sees.  The box-projected lookup returns p + t d within 64 ulp of the largest coordinate wherever no tap crosses a seam
    (measured: 8.9e-16 absolute on coordinates up to 3.5); the lookup along d itself lands on another face for a quarter."""
    S = SC.ROOM_FACE
    levels, _ = SC.FR.plan(S, 1)
    rec = SC.wall_point_cube()
    q = SC.room_queries(seed)
    hit, kept, other = SC.room_classes(q)
    got = N.capture_set_lookup_host(N.capture_set(SC.room_volume(), -1), levels, rec, q)
    assert got["valid"].all() and (got["count"] == 4).all()
    tol = 64 * np.spacing(np.abs(hit).max())
    err = np.abs(got["v"] - hit)[kept].max()
    print("seed %d: compared %.3f, another face %.3f, max abs error %.3g (bound %.3g)" %
          (seed, kept.mean(), other[kept].mean(), err, tol))
    assert err <= tol
    assert kept.mean() >= 0.75
    assert other[kept].mean() >= 0.2
    along_d = N.cube_chain_lookup_host(levels, rec, N.cube_queries(q["d"], 0.0))
    far = np.abs(along_d["v"] - hit).max(axis=1)
    assert (far[kept & other] > 1e-3).all()  # the lookup the plain shader does lands elsewhere: the test can see the difference
    assert far.max() > 1.0


# ---- argument checks ----

def _lookup_rc(cset, levels, rec, q):
    lv = N.cube_levels(levels)
    out = np.zeros(1, dtype=A.GATHER_OUT_DTYPE)
    return N.lib().rtr_capture_set_lookup_one(None if cset is None else C.byref(cset), C.byref(lv), len(levels), rec.ctypes.data,
                                              q.ctypes.data, out.ctypes.data)


def _spoiled():
    """(what, volumes, fallback): one broken rule each"""
    out = []
    for member in ("centre", "proxy_lo", "proxy_hi", "reach_lo", "reach_hi"):
        for value in (math.nan, math.inf, -math.inf):
            v = SC.volumes(2)
            v[member][1][2] = value
            out.append((member + " not finite", v, -1))
    for value in (math.nan, math.inf, -0.0, -0.25):
        v = SC.volumes(2)
        v["fade"][1] = value
        out.append(("fade %r" % value, v, -1))
    for member, axis, value in (("centre", 0, -2.0), ("centre", 1, 2.0), ("centre", 2, 5.0),  # on a proxy face, outside
                                ("reach_lo", 0, -2.5), ("reach_hi", 1, 2.5), ("reach_lo", 2, 1.5)):  # leaves the proxy; empty
        v = SC.volumes(1)
        v[member][0][axis] = value
        out.append(("%s[%d] = %g" % (member, axis, value), v, -1))
    out.append(("fallback -2", SC.volumes(2), -2))
    out.append(("fallback = n_captures", SC.volumes(2), 2))
    return out


def test_the_rules_of_a_set():
    levels, rec = SC.records(2, (4, 3))
    q = SC.queries(2, 4, 1)
    assert _lookup_rc(N.capture_set(SC.volumes(2), 1), levels, rec, q) == 0
    for what, vols, fallback in _spoiled():
        assert _lookup_rc(N.capture_set(vols, fallback), levels, rec, q) == INV, what
    v = SC.volumes(1)
    v["reach_lo"][0], v["reach_hi"][0] = v["proxy_lo"][0], v["proxy_hi"][0]  # reach = proxy, and a reach of one point: allowed
    assert _lookup_rc(N.capture_set(v, -1), SC.records(1, (4, 3))[0], rec, q) == 0
    v["reach_hi"][0] = v["reach_lo"][0]
    assert _lookup_rc(N.capture_set(v, -1), SC.records(1, (4, 3))[0], rec, q) == 0
    for n in (0, 17):
        s = N.capture_set(SC.volumes(2), -1)
        s.n_captures = n
        assert _lookup_rc(s, levels, rec, q) == INV, n
    big = np.array([SC.V0] * 16, dtype=A.CAPTURE_VOLUME_DTYPE)
    l16, r16 = SC.records(16, (1, 1))
    assert _lookup_rc(N.capture_set(big, 15), l16, r16, q) == 0
    s = N.capture_set(SC.volumes(2), -1)
    s.volumes = None
    assert _lookup_rc(s, levels, rec, q) == INV
    assert _lookup_rc(None, levels, rec, q) == INV
    lib = N.lib()
    s = N.capture_set(SC.volumes(2), -1)
    lv = N.cube_levels(levels)
    out = np.zeros(1, dtype=A.GATHER_OUT_DTYPE)
    for args in ((None, C.byref(lv), 3, rec.ctypes.data, q.ctypes.data, out.ctypes.data),
                 (C.byref(s), None, 3, rec.ctypes.data, q.ctypes.data, out.ctypes.data),
                 (C.byref(s), C.byref(lv), 0, rec.ctypes.data, q.ctypes.data, out.ctypes.data),
                 (C.byref(s), C.byref(lv), 3, None, q.ctypes.data, out.ctypes.data),
                 (C.byref(s), C.byref(lv), 3, rec.ctypes.data, None, out.ctypes.data),
                 (C.byref(s), C.byref(lv), 3, rec.ctypes.data, q.ctypes.data, None)):
        assert lib.rtr_capture_set_lookup_one(*args) == INV
    # a context comes before any device work
    assert lib.rtr_capture_set_lookup(None, C.byref(s), C.byref(lv), 3, rec.ctypes.data, len(rec) // 2, q.ctypes.data, out.ctypes.data, 1) == INV
    assert lib.rtr_capture_set_lookup_device(None, C.byref(s), C.byref(lv), 3, rec.ctypes.data, len(rec) // 2, q.ctypes.data,
                                             out.ctypes.data, 1, 1) == INV


def test_the_shader_checks_the_set_for_the_specular_part_only():
    env = SC.shade_environment(2, (4, 3))
    q = IC.queries(env, 1)
    out = np.zeros(1, dtype=A.GATHER_OUT_DTYPE)
    lib = N.lib()

    def rc(parts, cset):
        ne = SC.native_env(dict(env, parts=parts), parts, 2)
        return lib.rtr_shade_ibl_set_one(C.byref(ne), None if cset is None else C.byref(cset), q.ctypes.data, out.ctypes.data)

    good = N.capture_set(SC.volumes(2), -1)
    broken = N.capture_set(SC.volumes(2), 5)
    for parts in (1, 2, 3):
        assert rc(parts, good) == 0
        assert rc(parts, None) == (INV if parts & 2 else 0)  # a NULL set with SPECULAR off
        assert rc(parts, broken) == (INV if parts & 2 else 0)
    ne = SC.native_env(env, 3, 2)
    ne.n_records = len(env["records"]) // 2 - 1  # a level outside one capture's count
    assert lib.rtr_shade_ibl_set_one(C.byref(ne), C.byref(good), q.ctypes.data, out.ctypes.data) == INV
    bad = IC.bad_queries(q[0])
    ne = SC.native_env(env, 3, 2)
    for k in range(len(bad)):
        assert lib.rtr_shade_ibl_set_one(C.byref(ne), C.byref(good), bad[k:k + 1].ctypes.data, out.ctypes.data) == INV, k
    assert lib.rtr_shade_ibl_set(None, C.byref(ne), C.byref(good), q.ctypes.data, out.ctypes.data, 1) == INV
    assert lib.rtr_shade_ibl_set_device(None, C.byref(ne), C.byref(good), q.ctypes.data, out.ctypes.data, 1, 1) == INV
    pp = N.preview_params(8, 8)
    assert lib.rtr_preview_set(None, C.byref(pp), C.byref(ne), C.byref(good), out.ctypes.data, 8, None) == INV
    assert lib.rtr_preview_set_device(None, C.byref(pp), C.byref(ne), C.byref(good), out.ctypes.data, 8, None, 1) == INV


# ---- the command line ----

GOOD_LINE = "0 0 0  -1 -1 -1  1 1 1  -1,-1,-1  1 1 1  0.25  # centre, proxy, reach, fade\n"


@pytest.mark.parametrize("text, word", (
    ("0 0 0 -1 -1 -1 1 1 1 -1 -1 -1 1 1 1\n", "line 1"),                       # fifteen numbers
    (GOOD_LINE + "0 0 0 -1 -1 -1 1 1 1 -1 -1 -1 1 1 1 0 7\n", "line 2"),       # seventeen
    ("# nothing\n\n" + GOOD_LINE.replace("0.25", "wide"), "line 3"),           # a word
    ("# only a comment\n", "1..16"),                                            # no volume
    (GOOD_LINE * 17, "1..16"),                                                  # too many
    (GOOD_LINE.replace("-1,-1,-1", "-2,-1,-1"), "not a capture set"),           # reach leaves the proxy
    (GOOD_LINE.replace("0.25", "-0.0"), "not a capture set"),                   # fade -0.0
))
def test_the_command_line_refuses_a_malformed_set_before_a_context_is_made(tmp_path, text, word):
    import subprocess
    cli = os.path.join(os.path.dirname(N.library_path()), "rtr_cli")
    path = tmp_path / "set.txt"
    path.write_text(text)
    args = [cli, "21", "4", "--width", "32", "--preview", "1", "--out", str(tmp_path / "x.ppm"), "--probes", "2,2,2", "--probe-box",
            "100,100,100,450,450,450", "--face", "8", "--capture-levels", "2", "--brdf-table", "4,3", "--capture-set", str(path)]
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    err = r.stderr.decode()
    assert r.returncode == 2 and "--capture-set" in err and word in err, err
    assert "rtr_create" not in err and not (tmp_path / "x.ppm").exists()  # refused while parsing: no context was asked for
    r = subprocess.run(args[:-2] + ["--capture", "278,400,400", "--capture-fallback", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 2 and b"--capture-fallback goes with --capture-set" in r.stderr
