"""Access to tests/golden/ (fixtures produced by oracle/gen_golden.py from the unmodified
reference) and to the CPU oracle library.  Test infrastructure only."""
import ctypes as C
import gzip
import importlib
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
rtr = importlib.import_module("ray_tracing-rendering_amd")
A = rtr._abi

with open(os.path.join(GOLD, "manifest.json")) as _f:
    MANIFEST = json.load(_f)


def scene(scene_id):
    """Flattened scene walked from the reference's own object graph."""
    p = os.path.join(GOLD, "scene%02d.rtrs" % scene_id)
    if os.path.exists(p):
        return rtr.Scene.load(p)
    with gzip.open(p + ".gz", "rb") as f:
        return rtr.Scene.from_bytes(f.read())


def records(name, dtype):
    return np.fromfile(os.path.join(GOLD, name), dtype=dtype)


def image(name):
    info = MANIFEST["files"][name]
    a = np.fromfile(os.path.join(GOLD, name), dtype="<f8")
    return a.reshape(info["height"], info["width"], 3), info


def rel_l2(a, b):
    """SURVEY 8(d) parity figure on linear mean radiance."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ---- the CPU oracle (oracle/librtr_oracle.so) ------------------------------------------
_ORACLE = None


def oracle():
    global _ORACLE
    if _ORACLE is None:
        so = os.path.join(ROOT, "oracle", "librtr_oracle.so")
        src = os.path.join(ROOT, "oracle", "rt_oracle.cpp")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "port"], check=True,
                           stdout=subprocess.DEVNULL)
        lib = C.CDLL(so)
        P = C.POINTER
        lib.rto_render.argtypes = [P(A.SceneDescC), P(A.RenderParamsC), C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        lib.rto_li.argtypes = [P(A.SceneDescC), P(A.RenderParamsC), C.c_void_p, C.c_int64]
        for fn in (lib.rto_hits, lib.rto_hits_running_guard, lib.rto_materials, lib.rto_scatter, lib.rto_lights):
            fn.argtypes = [P(A.SceneDescC), C.c_void_p, C.c_int64]
        lib.rto_rng_block.argtypes = [C.c_uint32, C.c_void_p]
        lib.rto_sample_seed.argtypes = [C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        lib.rto_sample_seed.restype = C.c_uint32
        _ORACLE = lib
    return _ORACLE


def oracle_render(sc, params, threads=0):
    """Linear mean radiance (H, W, 3) of the params' region + stats dict, from the CPU oracle."""
    lib = oracle()
    h, w = params.y1 - params.y0, params.x1 - params.x0
    out = np.zeros((h, w, 3), dtype=np.float64)
    stats = np.zeros(3, dtype=np.uint64)
    d = sc.desc()
    rc = lib.rto_render(C.byref(d), C.byref(params), out.ctypes.data, w, threads, stats.ctypes.data)
    assert rc == 0, rc
    return out, {"samples": int(stats[0]), "closest_segments": int(stats[1]), "shadow_segments": int(stats[2])}


def oracle_records(sc, fn_name, recs, params=None):
    lib = oracle()
    out = np.ascontiguousarray(recs.copy())
    d = sc.desc()
    fn = getattr(lib, fn_name)
    if params is not None:
        rc = fn(C.byref(d), C.byref(params), out.ctypes.data, len(out))
    else:
        rc = fn(C.byref(d), out.ctypes.data, len(out))
    assert rc == 0, rc
    return out


# ---- measured residue of the device against the reference (GPU tests) ---------------------------
# Where the device calls OCML (sin / cos / log / acos / atan2) and the reference glibc, a last-ulp difference can
# flip a rare branch.  Instead of a round percentage, every such test states the EXACT number of mismatching
# records it measured on an MI355X (tests/golden/gpu_residue.json, written by a run with RTR_RESIDUE_OUT set)
# and fails above that number + 1.
_RESIDUE_FILE = os.path.join(GOLD, "gpu_residue.json")
try:
    with open(_RESIDUE_FILE) as _f:
        EXPECTED_RESIDUE = json.load(_f)
except OSError:
    EXPECTED_RESIDUE = {}
MEASURED_RESIDUE = {}


def residue(key, measured, loose_bar):
    """Record `measured` (a count or a float figure) under `key`; assert it against the committed measurement
    (+1 for counts; x2, at least 1e-15, for float figures), or against `loose_bar` while no measurement is committed."""
    MEASURED_RESIDUE[key] = measured
    out = os.environ.get("RTR_RESIDUE_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(MEASURED_RESIDUE, f, indent=1, sort_keys=True)
    print("residue %s = %r" % (key, measured))
    if key in EXPECTED_RESIDUE:
        exp = EXPECTED_RESIDUE[key]
        bar = exp + 1 if isinstance(exp, int) else max(exp * 2, 1e-15)
        assert measured <= bar, "%s: measured %r, committed measurement %r" % (key, measured, exp)
    else:
        assert measured <= loose_bar, "%s: measured %r above the provisional bar %r" % (key, measured, loose_bar)
