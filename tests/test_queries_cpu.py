"""CPU-only checks of the ray-query boundary (include/rtr_hip.h: rtr_query_*): declarations, exports, record layouts
and the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import _golden as G

A = G.A
rtr = G.rtr

ENTRIES = ("rtr_query_closest", "rtr_query_occluded", "rtr_query_closest_device", "rtr_query_occluded_device")
_SIZES = {"double": 8, "int32_t": 4, "uint32_t": 4}


def _header():
    return open(os.path.join(G.ROOT, "include", "rtr_hip.h")).read()


def _struct_layout(name):
    """(field, offset, bytes) of `typedef struct name { ... } name;` as a C compiler lays it out (natural alignment)"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    off, out = 0, []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for f in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", f)
            size = _SIZES[ctype] * int(m.group(2) or 1)
            off = (off + _SIZES[ctype] - 1) // _SIZES[ctype] * _SIZES[ctype]
            out.append((m.group(1), off, size))
            off += size
    return out, (off + 7) // 8 * 8


def test_header_declares_the_entries_and_exports_list_them():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(rtr_[a-z_0-9]+)\s*\(", text))
    lib = rtr.native.lib()
    for name in ENTRIES:
        assert name in declared and name in rtr.native.EXPORTS
        assert getattr(lib, name) is not None


def test_abi_version_is_still_4():
    assert re.search(r"#define RTR_ABI_VERSION (\d+)", _header()).group(1) == "4"
    assert A.RTR_ABI_VERSION == 4 and rtr.native.lib().rtr_abi_version() == 4


def test_record_layouts_match_the_header():
    assert C.sizeof(A.RayC) == A.RAY_DTYPE.itemsize == 80
    assert C.sizeof(A.RayHitC) == A.RAY_HIT_DTYPE.itemsize == 88
    for name, ctype, dtype in (("rtr_ray", A.RayC, A.RAY_DTYPE), ("rtr_ray_hit", A.RayHitC, A.RAY_HIT_DTYPE)):
        fields, size = _struct_layout(name)
        assert size == dtype.itemsize == C.sizeof(ctype)
        assert [f for f, _, _ in fields] == list(dtype.names) == [f for f, _ in ctype._fields_]
        for f, off, nbytes in fields:
            assert dtype.fields[f][1] == off == getattr(ctype, f).offset, (name, f)
            assert dtype.fields[f][0].itemsize == nbytes == getattr(ctype, f).size, (name, f)


def test_null_context_is_invalid():
    lib = rtr.native.lib()
    rays = np.zeros(1, dtype=A.RAY_DTYPE)
    hits = np.zeros(1, dtype=A.RAY_HIT_DTYPE)
    occ = np.zeros(1, dtype=np.uint8)
    assert lib.rtr_query_closest(None, rays.ctypes.data, hits.ctypes.data, 1, 0) == A.RTR_ERR_INVALID
    assert lib.rtr_query_occluded(None, rays.ctypes.data, occ.ctypes.data, None, 1, 0) == A.RTR_ERR_INVALID
    assert lib.rtr_query_closest_device(None, rays.ctypes.data, hits.ctypes.data, 1, 0, 1) == A.RTR_ERR_INVALID
    assert lib.rtr_query_occluded_device(None, rays.ctypes.data, occ.ctypes.data, None, 1, 0, 1) == A.RTR_ERR_INVALID


def test_make_rays_fills_the_defaults():
    rays = rtr.Context.make_rays([[0, 1, 2], [3, 4, 5]], [[0, 0, 1], [1, 0, 0]])
    assert rays.dtype == A.RAY_DTYPE and len(rays) == 2
    assert (rays["t_min"] == 0.001).all() and np.isinf(rays["t_max"]).all() and (rays["time"] == 0).all()
    assert (rays["rng_state"] == 1).all() and (rays["pad"] == 0).all()
    assert rays["origin"][1].tolist() == [3, 4, 5] and rays["direction"][0].tolist() == [0, 0, 1]


def test_query_kernels_are_in_the_product_and_no_test_kernel_is():
    syms = subprocess.run(["nm", "-D", "--defined-only", rtr.native.library_path()], stdout=subprocess.PIPE).stdout.decode()
    assert "k_query_closest" in syms and "k_query_any" in syms
    assert "k_test_" not in syms
