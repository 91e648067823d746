"""Temporal accumulation on the MI355X: tacc_kernel must give the host form's bits (the same body,
dev_temporal.h) on every scene over a still, a moved and a rotated step, through host buffers and torch tensors on a
non-default stream; and it must leave the render's state alone -- the next frame is bit-identical to a run without it."""
import numpy as np
import pytest

from mort_amd import hip, host
from mort_amd import structs as S

pytestmark = pytest.mark.gpu

OUTS = ("history", "accum", "variance", "rgba")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, what):
    for k in OUTS:
        assert (_bits(a[k]) == _bits(b[k])).all(), f"{what}: {k} differs"


def _sequence(cam0):
    """Three cameras: frame 0, the same camera (still), then W, then a mouse drag."""
    c1 = S.Camera.from_buffer_copy(cam0)
    c2 = host.camera_input(S.Camera.from_buffer_copy(c1), "W")
    c3 = host.camera_input(S.Camera.from_buffer_copy(c2), None, (6, -3))
    return [cam0, c1, c2, c3]


@pytest.mark.parametrize("sid", range(1, 11))
def test_temporal_matches_host_on_every_scene(gpu_ctx, sid):
    world, cam0 = host.build_scene(sid, width=96, spp=4)
    W, H = cam0.image_width, cam0.image_height
    gpu_ctx.upload_world(world)
    gpu_ctx.rng_seed(69420, W, H)
    hg = hh = None
    prev = None
    for i, cam in enumerate(_sequence(cam0)):
        acc = gpu_ctx.render(cam, want_accum=True)["accum"]
        f = gpu_ctx.render_features(cam)
        g = gpu_ctx.temporal(prev, cam, acc, f["normal"], f["depth"], hg)
        h = hip.temporal_host(prev, cam, acc, f["normal"], f["depth"], hh, nthreads=16)
        _same(g, h, f"scene {sid} step {i}")
        hg, hh, prev = g["history"], h["history"], cam
    assert (hg[0, ..., 3] > 4).any(), "some history survived the moves"


def test_device_form_on_a_stream_matches_host_buffers(gpu_ctx):
    import torch
    world, cam0 = host.build_scene(6, width=160, spp=4)
    W, H = cam0.image_width, cam0.image_height
    gpu_ctx.upload_world(world)
    gpu_ctx.rng_seed(69420, W, H)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    th = hip.TemporalHistory(W, H, backend=("device", gpu_ctx))
    hb = hip.TemporalHistory(W, H, backend=gpu_ctx)
    nrm, dep = (torch.zeros(W * H * c, dtype=torch.float32, device=dev) for c in (3, 1))
    alb = torch.zeros(W * H * 3, dtype=torch.float32, device=dev)
    for i, cam in enumerate(_sequence(cam0)):
        acc = gpu_ctx.render(cam, want_accum=True)["accum"]
        f = gpu_ctx.render_features(cam)
        ref = hb.step(acc, f["normal"], f["depth"], cam)
        with torch.cuda.stream(stream):
            acc_t = torch.from_numpy(acc.reshape(-1).copy()).to(dev, non_blocking=False)
            gpu_ctx.render_features_device(cam, alb, nrm, dep)
            out = th.step(acc_t, nrm, dep, cam)
        stream.synchronize()
        assert (out["accum"].cpu().numpy().view(np.uint32) == ref["accum"].reshape(-1).view(np.uint32)).all(), i
        assert (out["variance"].cpu().numpy().view(np.uint32) == ref["variance"].reshape(-1).view(np.uint32)).all(), i
        assert (out["rgba"].cpu().numpy() == ref["rgba"].reshape(-1)).all(), i
        assert (th.history.cpu().numpy().view(np.uint32) == hb.history.reshape(-1).view(np.uint32)).all(), i
        assert (out["samples"].cpu().numpy() == ref["samples"]).all()
    assert th.frames == 4


@pytest.mark.parametrize("sid,mode", [(1, hip.MODE_MEGA), (6, hip.MODE_WAVE), (9, hip.MODE_MEGA)])
def test_temporal_leaves_the_next_frame_alone(gpu_ctx, sid, mode):
    world, cam = host.build_scene(sid, width=128, spp=4)
    W, H = cam.image_width, cam.image_height
    gpu_ctx.upload_world(world)
    moved = host.camera_input(S.Camera.from_buffer_copy(cam), "D")

    def frames(extra):
        gpu_ctx.rng_seed(69420, W, H)
        first = gpu_ctx.render(cam, mode=mode, want_accum=True)
        if extra:
            f = gpu_ctx.render_features(cam)
            r = gpu_ctx.temporal(None, cam, first["accum"], f["normal"], f["depth"], None)
            r = gpu_ctx.temporal(cam, cam, first["accum"], f["normal"], f["depth"], r["history"])
            f2 = gpu_ctx.render_features(moved)
            gpu_ctx.temporal(cam, moved, first["accum"], f2["normal"], f2["depth"], r["history"])
        out = gpu_ctx.render(cam, mode=mode, want_accum=True, want_segments=mode == hip.MODE_MEGA)
        out["states"] = gpu_ctx.rng_store(W, H)
        return out

    a, b = frames(False), frames(True)
    assert (a["rgba"] == b["rgba"]).all()
    assert (a["accum"].view(np.uint32) == b["accum"].view(np.uint32)).all()
    assert (a["states"] == b["states"]).all()
    assert a["stats"]["segments"] == b["stats"]["segments"]
    if a["segments_px"] is not None:
        assert (a["segments_px"] == b["segments_px"]).all()


def test_still_accumulation_on_the_gpu_is_the_mean(gpu_ctx):
    world, cam = host.build_scene(6, width=128, spp=4)
    W, H = cam.image_width, cam.image_height
    gpu_ctx.upload_world(world)
    gpu_ctx.rng_seed(69420, W, H)
    f = gpu_ctx.render_features(cam)
    th = hip.TemporalHistory(W, H, backend=gpu_ctx)
    accs = []
    for _ in range(6):
        accs.append(gpu_ctx.render(cam, want_accum=True)["accum"].astype(np.float64))
        out = th.step(accs[-1].astype(np.float32), f["normal"], f["depth"], cam)
    np.testing.assert_allclose(out["accum"], np.mean(accs, axis=0), rtol=1e-6, atol=1e-7)
    assert (out["samples"] == 24).all() and (th.history[1, ..., 2] == 6).all()
