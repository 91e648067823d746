"""The SVGF filter stage on the MI355X: svgf_prep_kernel / svgf_iter_kernel must give the host form's bits (the
same bodies, dev_svgf.h) on every scene with the temporal variance and without it, wherever they read their taps from
(MORT_SVGF_TAPS: LDS tiles or global memory), on ragged, large and many-tile frames, through host buffers and torch tensors on a
non-default stream; and they must leave the render's state alone -- the next frame is bit-identical to a run without them."""
import numpy as np
import pytest

from mort_amd import hip, host
from tests.test_gpu_temporal import _bits, _sequence

pytestmark = pytest.mark.gpu

OUTS = ("accum", "variance", "rgba")
TAPS = (None, "lds", "global")  # the default mix, every tile, no tile


def _set_taps(monkeypatch, taps):
    if taps is None:
        monkeypatch.delenv("MORT_SVGF_TAPS", raising=False)
    else:
        monkeypatch.setenv("MORT_SVGF_TAPS", taps)


def _same(a, b, what):
    for k in OUTS:
        assert (_bits(a[k]) == _bits(b[k])).all(), f"{what}: {k} differs"


@pytest.mark.parametrize("sid", range(1, 11))
def test_svgf_matches_host_on_every_scene(gpu_ctx, monkeypatch, sid):
    world, cam0 = host.build_scene(sid, width=96, spp=4)
    W, H = cam0.image_width, cam0.image_height
    gpu_ctx.upload_world(world)
    gpu_ctx.rng_seed(69420, W, H)
    hist = prev = None
    for i, cam in enumerate(_sequence(cam0)):
        acc = gpu_ctx.render(cam, want_accum=True)["accum"]
        f = gpu_ctx.render_features(cam)
        t = gpu_ctx.temporal(prev, cam, acc, f["normal"], f["depth"], hist)
        hist, prev = t["history"], cam
        for V in (t["variance"], None):
            h = hip.svgf_host(t["accum"], f["albedo"], f["normal"], f["depth"], V, nthreads=16)
            for taps in TAPS:
                _set_taps(monkeypatch, taps)
                g = gpu_ctx.svgf(t["accum"], f["albedo"], f["normal"], f["depth"], V)
                _same(g, h, f"scene {sid} step {i} variance {'given' if V is not None else 'none'} taps {taps}")
    assert (t["variance"] >= 0).any(), "some pixels came with a temporal variance"


def _random_frame(W, H, seed):
    """features of random structure (flat regions, edges, misses) at any size, without a render"""
    g = np.random.default_rng(seed)
    C = g.uniform(0, 2, (H, W, 3)).astype(np.float32)
    A = np.repeat(np.repeat(g.uniform(0, 1, ((H + 15) // 16, (W + 15) // 16, 3)), 16, axis=0), 16, axis=1)[:H, :W].astype(np.float32)
    N = g.normal(size=(H, W, 3)) * 0.2 + np.array([0, 0, 1.0])
    N = (N / np.linalg.norm(N, axis=-1, keepdims=True)).astype(np.float32)
    D = (g.uniform(1, 10, (H, W)) + 0.01 * np.arange(W)[None, :]).astype(np.float32)
    miss = np.repeat(np.repeat(g.random(((H + 7) // 8, (W + 7) // 8)) < 0.2, 8, axis=0), 8, axis=1)[:H, :W]
    D[miss] = 0
    N[miss] = 0
    V = g.uniform(0.001, 0.5, (H, W)).astype(np.float32)
    V[g.random((H, W)) < 0.1] = -1.0
    return C, A, N, D, V


# ragged; wider than one LDS tile in both directions and off the 64 / 4 grid; one pixel; one row; one narrow column -- each with
# 0, 1, 2 (the two tiled steps), 3 and 5 iterations; and 1200x675 with the defaults and the five-iteration chain
SMALL = [(97, 55), (333, 41), (1, 1), (130, 1), (3, 70)]
CASES = [(W, H, it) for W, H in SMALL for it in (3, 5, 1, 2, 0)] + [(1200, 675, 3), (1200, 675, 5)]


@pytest.mark.parametrize("W,H,iterations", CASES)
def test_svgf_sizes_match_host(gpu_ctx, monkeypatch, W, H, iterations):
    pset = dict(iterations=iterations)
    C, A, N, D, V = _random_frame(W, H, W * 1000 + H)
    p = hip.SvgfParams(**pset)
    for var in (V, None):
        h = hip.svgf_host(C, A, N, D, var, params=p, nthreads=16)
        for taps in TAPS:
            _set_taps(monkeypatch, taps)
            g = gpu_ctx.svgf(C, A, N, D, var, params=p)
            _same(g, h, f"{W}x{H} {pset} variance {'given' if var is not None else 'none'} taps {taps}")


def test_device_form_on_a_stream_matches_host_buffers(gpu_ctx):
    import torch
    world, cam = host.build_scene(6, width=160, spp=4)
    W, H = cam.image_width, cam.image_height
    gpu_ctx.upload_world(world)
    gpu_ctx.rng_seed(69420, W, H)
    acc = gpu_ctx.render(cam, want_accum=True)["accum"]
    f = gpu_ctx.render_features(cam)
    t = gpu_ctx.temporal(None, cam, acc, f["normal"], f["depth"], None)
    t = gpu_ctx.temporal(cam, cam, gpu_ctx.render(cam, want_accum=True)["accum"], f["normal"], f["depth"], t["history"])
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    for V in (t["variance"], None):
        ref = gpu_ctx.svgf(t["accum"], f["albedo"], f["normal"], f["depth"], V)
        with torch.cuda.stream(stream):
            ins = [torch.from_numpy(np.ascontiguousarray(a).reshape(-1).copy()).to(dev) for a in (t["accum"], f["albedo"], f["normal"], f["depth"])]
            v_t = torch.from_numpy(V.reshape(-1).copy()).to(dev) if V is not None else None
            out = torch.zeros(W * H * 3, dtype=torch.float32, device=dev)
            vout = torch.zeros(W * H, dtype=torch.float32, device=dev)
            rgba = torch.zeros(W * H * 4, dtype=torch.uint8, device=dev)
            assert gpu_ctx.svgf_device(W, H, *ins, variance=v_t, accum_out=out, variance_out=vout, rgba_out=rgba) is None
        stream.synchronize()
        assert (out.cpu().numpy().view(np.uint32) == ref["accum"].reshape(-1).view(np.uint32)).all()
        assert (vout.cpu().numpy().view(np.uint32) == ref["variance"].reshape(-1).view(np.uint32)).all()
        assert (rgba.cpu().numpy() == ref["rgba"].reshape(-1)).all()
        sec = gpu_ctx.svgf_device(W, H, *ins, variance=v_t, accum_out=out, params=hip.SvgfParams(iterations=2), sync=True)
        assert sec > 0


@pytest.mark.parametrize("sid,mode", [(1, hip.MODE_MEGA), (6, hip.MODE_WAVE), (9, hip.MODE_MEGA)])
def test_svgf_leaves_the_next_frame_alone(gpu_ctx, sid, mode):
    world, cam = host.build_scene(sid, width=128, spp=4)
    W, H = cam.image_width, cam.image_height
    gpu_ctx.upload_world(world)

    def frames(extra):
        gpu_ctx.rng_seed(69420, W, H)
        first = gpu_ctx.render(cam, mode=mode, want_accum=True)
        if extra:
            f = gpu_ctx.render_features(cam)
            r = gpu_ctx.svgf(first["accum"], f["albedo"], f["normal"], f["depth"], None)
            gpu_ctx.svgf(first["accum"], f["albedo"], f["normal"], f["depth"], r["variance"], params=hip.SvgfParams(iterations=5))
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
