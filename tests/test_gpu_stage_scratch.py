"""The stages' shared scratch on the MI355X: the feature pass, the denoiser, the temporal step and the SVGF filter
stage their host buffers through ONE device allocation of the context and keep the filters' float4 planes in ONE other, so stages
alternating on a context -- at sizes that grow, shrink and re-carve those allocations, and on two streams back to back -- must
still give the host forms' bits, every output of every call."""
import functools

import numpy as np
import pytest

from mort_amd import hip, host
from tests.test_gpu_svgf import _random_frame
from tests.test_gpu_temporal import _bits

pytestmark = pytest.mark.gpu

SIZES = [(97, 55), (5, 3)]  # ragged, more than one workgroup each way; smaller than one workgroup
THREE = dict(iterations=3)


@functools.lru_cache(maxsize=None)
def _frame(W, H):
    """the random frame of a size, a second colour for the temporal step after the reset, and a camera of that size"""
    C, A, N, D, V = _random_frame(W, H, W * 1000 + H)
    C2 = np.random.default_rng(W + H).uniform(0, 2, (H, W, 3)).astype(np.float32)
    _, cam = host.build_scene(6, width=W, spp=4, aspect=W / (H + 0.5))
    assert (cam.image_width, cam.image_height) == (W, H)
    return dict(C=C, A=A, N=N, D=D, V=V, C2=C2, cam=cam)


@functools.lru_cache(maxsize=None)
def _host(stage, W, H):
    """the host form of a stage at a size, computed once and left unchanged"""
    f = _frame(W, H)
    if stage == "denoise":
        return hip.denoise_host(f["C"], f["A"], f["N"], f["D"], params=hip.DenoiseParams(**THREE), nthreads=16)
    if stage == "svgf":
        return hip.svgf_host(f["C"], f["A"], f["N"], f["D"], None, params=hip.SvgfParams(**THREE), nthreads=16)
    if stage == "svgf_var":
        return hip.svgf_host(f["C"], f["A"], f["N"], f["D"], f["V"], params=hip.SvgfParams(**THREE), nthreads=16)
    assert stage == "temporal"
    first = hip.temporal_host(None, f["cam"], f["C"], f["N"], f["D"], None, nthreads=16)
    return first, hip.temporal_host(f["cam"], f["cam"], f["C2"], f["N"], f["D"], first["history"], nthreads=16)


def _same(got, ref, keys, what):
    for k in keys:
        assert got[k].shape == ref[k].shape and (_bits(got[k]) == _bits(ref[k])).all(), f"{what}: {k} differs"


def _denoise(ctx, W, H):
    f = _frame(W, H)
    _same(ctx.denoise(f["C"], f["A"], f["N"], f["D"], params=hip.DenoiseParams(**THREE)), _host("denoise", W, H), ("accum", "rgba"), f"denoise {W}x{H}")


def _svgf(ctx, W, H, with_variance):
    f = _frame(W, H)
    got = ctx.svgf(f["C"], f["A"], f["N"], f["D"], f["V"] if with_variance else None, params=hip.SvgfParams(**THREE))
    _same(got, _host("svgf_var" if with_variance else "svgf", W, H), ("accum", "variance", "rgba"), f"svgf {W}x{H} variance {with_variance}")


def _temporal(ctx, W, H):
    f = _frame(W, H)
    ref0, ref1 = _host("temporal", W, H)
    keys = ("history", "accum", "variance", "rgba")
    got0 = ctx.temporal(None, f["cam"], f["C"], f["N"], f["D"], None)
    _same(got0, ref0, keys, f"temporal {W}x{H} reset")
    _same(ctx.temporal(f["cam"], f["cam"], f["C2"], f["N"], f["D"], got0["history"]), ref1, keys, f"temporal {W}x{H} with a history")


def test_host_buffer_forms_interleaved_at_two_sizes(gpu_ctx):
    (W, H), (w, h) = SIZES
    world, cam = host.build_scene(6, width=97, spp=4)
    gpu_ctx.upload_world(world)
    _denoise(gpu_ctx, W, H)
    _svgf(gpu_ctx, w, h, False)
    _temporal(gpu_ctx, W, H)
    _svgf(gpu_ctx, W, H, True)
    _denoise(gpu_ctx, w, h)
    _temporal(gpu_ctx, w, h)
    _same(gpu_ctx.render_features(cam), hip.render_features_host(world, cam, nthreads=16), ("albedo", "normal", "depth"), "features of scene 6")
    _denoise(gpu_ctx, W, H)


@pytest.mark.parametrize("first", ["denoise", "svgf"])
@pytest.mark.parametrize("W,H", SIZES)
def test_device_forms_back_to_back_on_two_streams(gpu_ctx, W, H, first):
    import torch
    dev = torch.device("cuda:0")
    f = _frame(W, H)
    ins = [torch.from_numpy(np.ascontiguousarray(f[k]).reshape(-1).copy()).to(dev) for k in ("C", "A", "N", "D")]
    n = W * H
    outs = {s: dict(accum=torch.zeros(n * 3, dtype=torch.float32, device=dev), variance=torch.zeros(n, dtype=torch.float32, device=dev),
                    rgba=torch.zeros(n * 4, dtype=torch.uint8, device=dev)) for s in ("denoise", "svgf")}
    torch.cuda.synchronize(dev)  # the inputs are there before either stream starts
    streams = {s: torch.cuda.Stream(device=dev) for s in ("denoise", "svgf")}

    def launch(stage):
        o = outs[stage]
        with torch.cuda.stream(streams[stage]):
            if stage == "denoise":
                r = gpu_ctx.denoise_device(W, H, *ins, accum_out=o["accum"], rgba_out=o["rgba"], params=hip.DenoiseParams(**THREE))
            else:
                r = gpu_ctx.svgf_device(W, H, *ins, accum_out=o["accum"], variance_out=o["variance"], rgba_out=o["rgba"], params=hip.SvgfParams(**THREE))
        assert r is None, "an asynchronous call: it returns no device time"

    launch(first)
    launch("svgf" if first == "denoise" else "denoise")
    for s in streams.values():
        s.synchronize()
    for stage, keys in (("denoise", ("accum", "rgba")), ("svgf", ("accum", "variance", "rgba"))):
        ref = _host(stage, W, H)
        for k in keys:
            assert (_bits(outs[stage][k].cpu().numpy()) == _bits(ref[k]).reshape(-1)).all(), f"{stage} after {first} first, {W}x{H}: {k} differs"
