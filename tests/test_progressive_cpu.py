"""Progressive accumulation (include/rtr_hip.h: rtr_accum_*) without a GPU: the library exports the entry points,
the header and the Python mirror agree on ABI version 4, null handles and arguments are refused before any device
call, and Renderer.render_progressive rejects bad schedules before it touches its context."""
import ctypes as C
import os
import re

import pytest

import _golden as G

A = G.A
rtr = G.rtr

ACCUM_SYMBOLS = ("rtr_accum_create", "rtr_accum_render", "rtr_accum_resolve", "rtr_accum_tiles", "rtr_accum_destroy")


def test_library_exports_the_accumulator():
    lib = rtr.native.lib()
    for name in ACCUM_SYMBOLS:
        assert name in rtr.native.EXPORTS
        assert getattr(lib, name) is not None


def test_abi_version_4_in_header_and_mirror():
    text = open(os.path.join(G.ROOT, "include", "rtr_hip.h")).read()
    assert int(re.search(r"#define RTR_ABI_VERSION (\d+)", text).group(1)) == 4
    assert A.RTR_ABI_VERSION == 4
    assert rtr.native.lib().rtr_abi_version() == 4


def test_null_handles_and_arguments_are_refused():
    L = rtr.native.lib()
    p = A.make_params(64, 64, 1)
    out = C.c_void_p()
    n = C.c_int64(0)
    fake = C.c_void_p(0x1000)  # never dereferenced: the context is checked first
    assert L.rtr_accum_create(None, C.byref(p), C.byref(out)) == A.RTR_ERR_INVALID
    assert L.rtr_accum_render(None, None, 4, 1) == A.RTR_ERR_INVALID
    assert L.rtr_accum_render(None, fake, 4, 1) == A.RTR_ERR_INVALID
    assert L.rtr_accum_resolve(None, None, None, 0, None) == A.RTR_ERR_INVALID
    assert L.rtr_accum_tiles(None, None, None, None, 0, C.byref(n)) == A.RTR_ERR_INVALID
    L.rtr_accum_destroy(None)  # ignored


class _StubContext:
    """stands in for native.Context: any device call fails the test"""
    scene = None

    def __getattr__(self, name):
        raise AssertionError("device call %s before the schedule was checked" % name)


@pytest.mark.parametrize("targets", [[], [0], [-1, 4], [4, 4], [4, 2], [1, 2, 2, 3], [8, 16, 12]])
def test_render_progressive_rejects_bad_schedules(targets):
    r = rtr.Renderer(context=_StubContext())
    with pytest.raises(ValueError):
        r.render_progressive(object(), rtr.RenderBuffer(16, 16), targets)
