"""The device forms of the accumulator outputs (include/rtr_hip.h: rtr_accum_resolve_device, _features_device,
_denoise_device, _denoise_temporal_device) without a GPU: the library exports them, the header declares them, _abi.py
declares them with the header's signatures, and a null context is refused before anything is touched."""
import ctypes as C
import os
import re

import _golden as G

A = G.A
rtr = G.rtr

SYMBOLS = ("rtr_accum_resolve_device", "rtr_accum_features_device", "rtr_accum_denoise_device",
           "rtr_accum_denoise_temporal_device")

# a parameter of the header as its ctypes type: handles and buffers are void pointers in the binding
_CTYPES = {"rtr_context*": C.c_void_p, "rtr_accum*": C.c_void_p, "rtr_history*": C.c_void_p, "double*": C.c_void_p,
           "uint8_t*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32, "int": C.c_int,
           "const rtr_denoise_params*": C.POINTER(A.DenoiseParamsC), "const rtr_temporal_params*": C.POINTER(A.TemporalParamsC)}


def _header():
    text = open(os.path.join(G.ROOT, "include", "rtr_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _declaration(name):
    """(return type, [parameter types]) of `name` as the header declares it"""
    m = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, "%s is not declared" % name
    types = []
    for prm in m.group(2).split(","):
        words = prm.replace("*", " * ").split()
        assert len(words) >= 2, prm  # a type and a name
        types.append(" ".join(words[:-1]).replace(" *", "*"))
    return m.group(1), types


def test_library_exports_and_header_declares_the_entry_points():
    lib = rtr.native.lib()
    declared = set(re.findall(r"\b(rtr_[a-z_0-9]+)\s*\(", _header()))
    for name in SYMBOLS:
        assert name in rtr.native.EXPORTS and name in declared
        assert getattr(lib, name) is not None
    assert int(re.search(r"#define RTR_ABI_VERSION (\d+)", _header()).group(1)) == 4 == A.RTR_ABI_VERSION  # new symbols only
    assert lib.rtr_abi_version() == 4


def test_abi_declares_the_headers_signatures():
    lib = rtr.native.lib()
    assert set(A.DEVICE_OUTPUT_SIGNATURES) == set(SYMBOLS)
    for name in SYMBOLS:
        ret, types = _declaration(name)
        assert ret == "int"
        assert A.DEVICE_OUTPUT_SIGNATURES[name] == [_CTYPES[t] for t in types], name
        assert list(getattr(lib, name).argtypes) == A.DEVICE_OUTPUT_SIGNATURES[name]  # what the binding calls with
        assert types[-1] == "int"  # `blocking` comes last
    # the same parameters as the host forms, plus `blocking`
    for name in SYMBOLS:
        host = _declaration(name[:-len("_device")])[1]
        assert _declaration(name)[1] == host + ["int"], name


def test_null_contexts_are_refused():
    L = rtr.native.lib()
    prm, tp = rtr.native.denoise_defaults(), rtr.native.temporal_defaults()
    lin = (C.c_double * 12)(*([-7.0] * 12))
    rgb = (C.c_uint8 * 12)(*([0xA5] * 12))
    feat = (C.c_double * 28)(*([-7.0] * 28))
    for blocking in (0, 1):
        assert L.rtr_accum_resolve_device(None, None, lin, 2, rgb, blocking) == A.RTR_ERR_INVALID
        assert L.rtr_accum_features_device(None, None, 1, feat, 2, blocking) == A.RTR_ERR_INVALID
        assert L.rtr_accum_denoise_device(None, None, C.byref(prm), lin, 2, rgb, blocking) == A.RTR_ERR_INVALID
        assert L.rtr_accum_denoise_temporal_device(None, None, None, C.byref(prm), C.byref(tp), lin, 2, rgb,
                                                   blocking) == A.RTR_ERR_INVALID
    assert list(lin) == [-7.0] * 12 and list(rgb) == [0xA5] * 12 and list(feat) == [-7.0] * 28
