"""rtr_set_camera / rtr_get_camera / rtr_accum_reset (include/rtr_hip.h) on the GPU: after a camera update a context
renders the bits of a context that uploaded the same scene with that camera -- one-shot renders of both pipelines,
rtr_li_samples, features and accumulator passes -- and an accumulator that was not reset refuses to render."""
import ctypes as C

import numpy as np
import pytest

import _golden as G
import _randscene as R
import _temporal_ref as T

A = G.A
rtr = G.rtr

pytestmark = pytest.mark.gpu

W = H = 32
SPP = 4


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _scene(sid):
    if sid == "media":
        return R.random_scene(14, media=True)
    if sid == "top":
        return R.random_scene(5, n_objects=90)
    return G.scene(sid)


def _camera2(sc):
    cam = T.camera_dict(sc.camera)
    step = 0.03 * np.sqrt(cam["horizontal"] @ cam["horizontal"])
    return T.moved_camera(cam, translate=step * cam["u"] + 0.5 * step * cam["v"], yaw_deg=4.0)


@pytest.fixture(scope="module")
def pair():
    a, b = rtr.Context(0), rtr.Context(0)
    yield a, b
    a.close()
    b.close()


@pytest.fixture(params=[21, 23, "media", "top"])
def updated(request, pair, monkeypatch):
    """(scene id, context A: uploaded with camera 1, then set_camera(camera 2); context B: uploaded with camera 2;
    camera 2)"""
    sid = request.param
    if sid == "top":
        monkeypatch.setenv("RTR_TOP_MIN", "2")  # read at upload (rt_compile.h): the per-lane instance walk
    a, b = pair
    sc = _scene(sid)
    cam2 = _camera2(sc)
    a.upload(sc)
    if sid == "top":
        assert rtr.native.validate_scene(sc)["top_trees"] == 1
    warm = a.render(A.make_params(W, H, 1, seed=1))  # camera 1 has been on the device
    a.set_camera(cam2)
    b.upload(T.scene_with_camera(sc, cam2))
    assert not np.array_equal(_bits(warm), _bits(b.render(A.make_params(W, H, 1, seed=1))))  # the cameras differ
    return sid, a, b, cam2


@pytest.mark.parametrize("chunks", [1, 0])
def test_one_shot_renders_equal_an_upload_with_that_camera(updated, chunks):
    sid, a, b, _ = updated
    for pipe in (A.PIPELINE_MEGAKERNEL, A.PIPELINE_WAVEFRONT):
        p = A.make_params(W, H, SPP, seed=7, pipeline=pipe, spp_chunks=chunks)
        try:
            want = b.render(p)
        except rtr.RtrError as e:  # the wavefront pipeline does not run every graph
            assert pipe == A.PIPELINE_WAVEFRONT and e.code == A.RTR_ERR_UNSUPPORTED
            with pytest.raises(rtr.RtrError):
                a.render(p)
            continue
        assert np.array_equal(_bits(a.render(p)), _bits(want))
        assert a.stats()["spp_chunks"] == b.stats()["spp_chunks"]


def test_li_samples_features_and_accumulators_equal_an_upload_with_that_camera(updated):
    sid, a, b, cam2 = updated
    p = A.make_params(W, H, SPP, seed=9)
    jj, ii = np.mgrid[0:H:3, 0:W:3]
    ijs = np.stack([ii.ravel(), jj.ravel(), (ii.ravel() + jj.ravel()) % SPP], axis=1)
    assert np.array_equal(_bits(a.li_samples(p, ijs)), _bits(b.li_samples(p, ijs)))
    # an accumulator of A that goes through a camera update and a reset: samples and features of another camera and
    # another seed first, then set_camera (the same camera 2 again: any update makes it stale), then reset(9).
    # (Accumulators run the megakernel pipeline only -- RTR_PIPELINE_WAVEFRONT is RTR_ERR_UNSUPPORTED at creation -- so
    # "both pipelines" applies to the one-shot renders above, not here.)
    with a.accumulator(A.make_params(W, H, SPP, seed=4), moments=True) as xa, b.accumulator(p, moments=True) as xb:
        xa.render(2)
        xa.features(1)
        a.set_camera(cam2)
        with pytest.raises(rtr.RtrError) as e:
            xa.render(SPP)
        assert e.value.code == A.RTR_ERR_INVALID
        xa.reset(9)
        assert (xa.tiles()[1] == 0).all()
        assert np.array_equal(_bits(xa.features(2)), _bits(xb.features(2)))
        xa.render(SPP)
        xb.render(SPP)
        assert np.array_equal(_bits(xa.resolve()), _bits(xb.resolve()))
        assert np.array_equal(_bits(xa.moments()), _bits(xb.moments()))
        assert np.array_equal(_bits(xa.resolve()), _bits(b.render(A.make_params(W, H, SPP, seed=9, spp_chunks=1))))


def test_accumulator_created_before_the_update_needs_a_reset(pair):
    a, b = pair
    sc = G.scene(21)
    cam2 = _camera2(sc)
    a.upload(sc)
    b.upload(T.scene_with_camera(sc, cam2))
    p = A.make_params(W, H, 1, seed=3)
    with a.accumulator(p, moments=True) as acc:
        acc.render(SPP)
        acc.features(1)
        old = acc.resolve()
        a.set_camera(cam2)
        for call in (lambda: acc.render(2 * SPP), lambda: acc.render_tiles(np.full(len(acc.tiles()[0]), 2 * SPP)),
                     lambda: acc.refine(1e-3, 1, 2 * SPP), lambda: acc.features(1), lambda: acc.denoise()):
            with pytest.raises(rtr.RtrError) as e:
                call()
            assert e.value.code == A.RTR_ERR_INVALID and "rtr_accum_reset" in e.value.message
        # what it holds belongs to camera 1 and can still be read
        assert np.array_equal(_bits(acc.resolve()), _bits(old))
        assert (acc.tiles()[1] == SPP).all() and np.isfinite(acc.moments()).all() and len(acc.errors()) == len(acc.tiles()[0])
        # reset: a fresh accumulator with the new seed, under camera 2
        acc.reset(11)
        assert (acc.tiles()[1] == 0).all()
        assert np.array_equal(acc.resolve(np.full((H, W, 3), -3.0)), np.full((H, W, 3), -3.0))  # no samples: untouched
        with b.accumulator(A.make_params(W, H, 1, seed=11), moments=True) as fresh:
            assert np.array_equal(_bits(acc.features(1)), _bits(fresh.features(1)))
            acc.render(2)
            acc.render(SPP)
            fresh.render(SPP)
            assert np.array_equal(_bits(acc.resolve()), _bits(fresh.resolve()))
            assert np.array_equal(_bits(acc.moments()), _bits(fresh.moments()))
            assert np.array_equal(_bits(acc.denoise()), _bits(fresh.denoise()))
        # after a re-upload it stays invalid, reset included
        a.upload(sc)
        with pytest.raises(rtr.RtrError) as e:
            acc.reset(1)
        assert e.value.code == A.RTR_ERR_INVALID
        with pytest.raises(rtr.RtrError):
            acc.render(2 * SPP)


def test_errors_and_round_trip():
    sc = G.scene(21)
    with rtr.Context(0) as c:
        with pytest.raises(rtr.RtrError) as e:
            c.set_camera(sc.camera)
        assert e.value.code == A.RTR_ERR_NO_SCENE
        with pytest.raises(rtr.RtrError) as e:
            c.camera()
        assert e.value.code == A.RTR_ERR_NO_SCENE
        c.upload(sc)
        assert c.camera().tobytes() == sc.camera.tobytes()
        cam2 = T.camera_record(_camera2(sc))
        c.set_camera(cam2)
        assert c.camera().tobytes() == cam2.tobytes()
        assert c._L.rtr_set_camera(c._h, None) == A.RTR_ERR_INVALID
        for field, value in (("origin", np.nan), ("w", np.inf), ("lens_radius", -np.inf), ("time1", np.nan)):
            bad = cam2.copy()
            if bad[field].ndim == 2:
                bad[field][0, 1] = value
            else:
                bad[field][0] = value
            with pytest.raises(rtr.RtrError) as e:
                c.set_camera(bad)
            assert e.value.code == A.RTR_ERR_INVALID
        assert c.camera().tobytes() == cam2.tobytes()  # a refused camera changes nothing
        # moving spheres: their boxes were built for the ray times of the uploaded camera
        moving = G.scene(1)
        assert (moving.nodes["type"] == A.NODE_MOVING_SPHERE).any()
        c.upload(moving)
        cam = moving.camera.copy()
        t_hi = max(0.0, float(cam["time0"][0]), float(cam["time1"][0]))
        inside = cam.copy()
        inside["time1"][0] = 0.5 * t_hi
        c.set_camera(inside)
        for field, value in (("time1", t_hi + 0.5), ("time0", -0.25)):
            outside = cam.copy()
            outside[field][0] = value
            with pytest.raises(rtr.RtrError) as e:
                c.set_camera(outside)
            assert e.value.code == A.RTR_ERR_UNSUPPORTED and "rtr_upload_scene" in e.value.message
        assert c.camera().tobytes() == inside.tobytes()


def test_renders_queued_before_the_update_keep_their_camera(pair):
    """eight renders queued back to back without blocking, then set_camera, then one more: the host is far ahead of
    the device when the camera changes (a launch takes microseconds, a render far longer), so an update that reached
    the device copy of the scene at once, and not in stream order, would change the renders still waiting in the queue"""
    import torch
    a, b = pair
    sc = G.scene(21)
    cam2 = _camera2(sc)
    a.upload(sc)
    b.upload(sc)
    S, N = 64, 8
    p = A.make_params(S, S, 16, seed=5)
    want1 = b.render(p)
    b.set_camera(cam2)
    want2 = b.render(p)
    outs = [torch.zeros((S, S, 3), dtype=torch.float64, device="cuda:0") for _ in range(N + 1)]
    a.render(p)  # warm: nothing is allocated or compiled inside the queue below
    a.synchronize()
    for k in range(N):
        a.render_into(p, outs[k].data_ptr(), S, blocking=False)
    a.set_camera(cam2)  # no device work, no wait
    a.render_into(p, outs[N].data_ptr(), S, blocking=False)
    a.synchronize()
    for k in range(N):
        assert np.array_equal(_bits(outs[k].cpu().numpy()), _bits(want1)), "queued render %d" % k
    assert np.array_equal(_bits(outs[N].cpu().numpy()), _bits(want2))


def test_renderer_and_camera_ray_follow_the_camera(pair):
    """after a render_sequence (or any set_camera) Renderer.render(scene) is still the image of scene.camera, and
    Context.camera_ray builds the ray of the camera the context renders with"""
    a, b = pair
    sc = G.scene(21)
    r = rtr.Renderer(context=a)
    r.seed = 3
    r.set_samples(SPP)
    buf = rtr.RenderBuffer(W, H)
    cams = [_camera2(sc), T.moved_camera(_camera2(sc), yaw_deg=5.0)]
    assert list(r.render_sequence(sc, cams, buf, SPP)) == [0, 1]
    assert a.scene is sc and a.camera_updated
    p = A.make_params(W, H, 1)
    ray = a.camera_ray(p, 7, 9)
    assert np.array_equal(ray["origin"][0], T.camera_record(cams[1])["origin"][0])
    moved = buf.to_rgb8().copy()
    r.render(sc, buf)
    assert not a.camera_updated and a.camera().tobytes() == sc.camera.tobytes()
    fresh = rtr.Renderer(context=b)
    fresh.seed = 3
    fresh.set_samples(SPP)
    b.upload(T.scene_with_camera(sc, cams[0]))  # b holds another scene object: the render below uploads sc
    want = rtr.RenderBuffer(W, H)
    fresh.render(sc, want)
    assert np.array_equal(buf.linear, want.linear) and not np.array_equal(buf.to_rgb8(), moved)
    assert np.array_equal(a.camera_ray(p, 7, 9)["origin"][0], np.asarray(sc.camera["origin"][0]))
    # the progressive driver as well
    a.set_camera(cams[1])
    got = rtr.RenderBuffer(W, H)
    assert list(r.render_progressive(sc, got, [SPP])) == [SPP]
    want = rtr.RenderBuffer(W, H)
    assert list(fresh.render_progressive(sc, want, [SPP])) == [SPP]
    assert np.array_equal(got.linear, want.linear)
    # a camera equal to the scene's own is no update
    a.set_camera(cams[1])
    a.set_camera(sc.camera)
    assert not a.camera_updated
