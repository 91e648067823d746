"""Visibility-weighted irradiance volumes on the MI355X (depth.hip, volume.hip): probe_depth_kernel and
volume_sample_visible_kernel must give the host forms' answers (the same bodies, dev_depth.h) and the restatement's of
tests/depth_ref.py over the oracle at tolerance 0 -- outputs as raw words, any NaN equal to any NaN -- at probe counts that leave
partial groups of four waves, at point counts that leave partial waves and groups, at the three strides, under the masks; on torch
tensors and torch streams, straight from the hits tensor of a closest-hit query; and they must write nothing past their outputs."""
import ctypes as C

import numpy as np
import pytest

from mort_amd import hip
from tests import depth_cases as DC
from tests import depth_ref as D
from tests import volume_cases as K

pytestmark = pytest.mark.gpu

F = np.float32
NS = (1, 63, 64, 65, 255, 256, 257, 1000)
NPROBES = (1, 3, 4, 5, 9)
INVALID, NO_WORLD = -1, -4


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda:0"))


def _mixed(g, seed=2):
    """1000 of the sampler's points in a fixed shuffled order, so that every prefix holds every kind"""
    pts = DC.sampler_points(g, 900)
    return pts[np.random.default_rng(seed).permutation(len(pts))[:1000]]


# ---------------------------------------------------------------------------------------------------------------- the bake

@pytest.mark.parametrize("s", (1, 3))
@pytest.mark.parametrize("name", DC.WORLDS)
def test_bake_device_equals_host_equals_restatement(name, s):
    """a context of its own per world; the far probe (3) and the NaN probe (4) are among the first five"""
    import torch
    w = DC.world(name)[0]
    want = DC.maps(name, s)
    probes = DC.probes(name)
    params = DC.params(name, s)
    for tree in ((False, True) if DC.has_tree(name) else (False,)):
        DC.same(hip.probe_depth_bake_host(w, params, probes, tree=tree, nthreads=4)["depth"], want, f"{name} s {s} host tree {tree}")
    with hip.Context(0) as ctx:
        ctx.upload_world(w)
        for n in NPROBES:
            got = ctx.probe_depth_bake(params, probes[:n])
            assert got["seconds"] > 0
            DC.same(got["depth"], want[:n], f"{name} s {s} n {n} device")
        # the _device form into the head of a larger tensor: the bytes past 800 n keep theirs
        pr_t = _dev(probes).view(torch.float32)
        for n in (1, 5, 9):
            out_t = torch.full((n * 800 + 4096,), 0xa5, dtype=torch.uint8, device="cuda:0")
            ctx.probe_depth_bake_device(params, pr_t[:4 * n], out_t[:n * 800], sync=True)
            out = out_t.cpu().numpy()
            assert (out[n * 800:] == 0xa5).all(), f"n={n}: maps written past the batch"
            DC.same(out[:n * 800].view(F).reshape(n, 200), want[:n], f"{name} s {s} n {n} into the head of a larger tensor")


def test_bake_on_a_torch_stream_and_status_codes():
    import torch
    name, s = "scene6", 2
    w = DC.world(name)[0]
    want = DC.maps(name, s)
    params = DC.params(name, s)
    dev = torch.device("cuda:0")
    L = hip.lib()
    with hip.Context(0) as ctx:
        n = DC.N_PROBES
        buf = torch.zeros(n * 16 + n * 800 + 256, dtype=torch.uint8, device=dev)
        d_pr, d_dm = buf.data_ptr(), buf.data_ptr() + n * 16
        pp = C.byref(params)
        call = lambda q, m, p, d: L.mort_hip_probe_depth_bake_device(ctx._h, q, m, p, d, None, None)  # noqa: E731
        assert call(pp, n, d_pr, d_dm) == NO_WORLD, "no world uploaded"
        assert ctx.volume_sample_visible(K.grid((1, 1, 1)), K.records(K.grid((1, 1, 1))), DC.random_maps(K.grid((1, 1, 1))),
                                         hip.VOLUME_VIS_PARAMS(), np.ones((3, 6), dtype=F))["out"].shape == (3, 4), "the sampler needs no world"
        ctx.upload_world(w)
        assert call(pp, 0, d_pr, d_dm) == 0, "an empty batch launches nothing"
        for a in ((None, n, d_pr, d_dm), (pp, n, None, d_dm), (pp, n, d_pr, None), (pp, n, d_pr + 4, d_dm), (pp, n, d_pr, d_dm + 8),
                  (pp, n, d_pr, d_pr), (pp, n, d_pr, d_dm - 16)):
            assert call(*a) == INVALID, a
        for bad in (hip.DEPTH_PARAMS(0, 1.0), hip.DEPTH_PARAMS(9, 1.0), hip.DEPTH_PARAMS(2, 0.0), hip.DEPTH_PARAMS(2, np.inf), hip.DEPTH_PARAMS(2, np.nan)):
            assert call(C.byref(bad), n, d_pr, d_dm) == INVALID
        torch.cuda.synchronize()
        assert (buf == 0).all(), "a refused call writes nothing"
        # a stream other than the context's: one asynchronous call, then a timed one
        stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(stream):
            pr_t = _dev(DC.probes(name)).view(torch.float32)
            out = [torch.zeros(n * 200, dtype=torch.float32, device=dev) for _ in range(2)]
            assert ctx.probe_depth_bake_device(params, pr_t, out[0]) is None
            sec = ctx.probe_depth_bake_device(params, pr_t, out[1], sync=True)
        stream.synchronize()
        assert sec > 0
        a, b = (o.cpu().numpy().reshape(n, 200) for o in out)
        assert a.tobytes() == b.tobytes()
        DC.same(a, want, "the bake on a torch stream")


# ------------------------------------------------------------------------------------------------------------- the sampler

@pytest.mark.parametrize("mask", ["ones", "holes", "fractional"])
@pytest.mark.parametrize("count", K.COUNTS)
def test_sampler_device_equals_host_equals_restatement(gpu_ctx, count, mask):
    g = K.grid(count)
    rec = K.records(g, mask)
    maps = DC.random_maps(g)
    if mask == "holes":
        maps[rec[:, 27] == 0] = np.nan
    pts = _mixed(g)
    assert len(pts) == max(NS)
    for bias, minv in ((0.25, 0.05), (0.0, 0.0)):
        vp = hip.VOLUME_VIS_PARAMS(bias, minv)
        want = D.sample_visible(g, rec, maps, bias, minv, pts[:, :3], pts[:, 3:])
        DC.same(hip.volume_sample_visible_host(g, rec, maps, vp, pts, nthreads=4)["out"], want, f"grid {count} {mask} host")
        for n in NS if minv else (65, 1000):
            got = gpu_ctx.volume_sample_visible(g, rec, maps, vp, pts[:n])["out"]
            DC.same(got, want[:n], f"grid {count} {mask} bias {bias} min {minv} n={n} device")


def test_sampler_strides_and_bytes_past_the_batch(gpu_ctx):
    import torch
    g = K.grid((4, 3, 2))
    rec, maps = K.records(g, "fractional"), DC.random_maps(g)
    pts = _mixed(g)
    vp = hip.VOLUME_VIS_PARAMS(0.1, 0.05)
    want = D.sample_visible(g, rec, maps, 0.1, 0.05, pts[:, :3], pts[:, 3:])
    rec_t, map_t = _dev(rec), _dev(maps)
    for stride, fill in ((24, 0), (40, 0xa5), (40, 0xff), (48, 0xa5)):
        for n in (1, 63, 65, 257, 1000):  # the last group is partial: its lanes past n must not store
            pts_t = _dev(K.strided(pts[:n], stride, fill))
            out_t = torch.full((n * 16 + 4096,), 0xa5, dtype=torch.uint8, device="cuda:0")
            sec = gpu_ctx.volume_sample_visible_device(g, rec_t, map_t, vp, pts_t, out_t[:n * 16], stride=stride, sync=True)
            assert sec > 0
            out = out_t.cpu().numpy()
            assert (out[n * 16:] == 0xa5).all(), f"n={n}: output written past the batch"
            DC.same(out[:n * 16].view(F).reshape(-1, 4), want[:n], f"stride {stride} fill {fill:#x} n={n}")
        DC.same(gpu_ctx.volume_sample_visible(g, rec, maps, vp, K.strided(pts, stride, fill), stride=stride)["out"], want, f"stride {stride} host-buffer form")


def test_identity_against_the_plain_sampler_on_the_device(gpu_ctx):
    """with every m1 = FLT_MAX, volume_sample_device's words (the points whose squared offset overflows, r = +inf, left out)"""
    import torch
    g = K.grid((5, 4, 3))
    pts = _mixed(g)
    with np.errstate(invalid="ignore", over="ignore"):
        near = ~(np.abs(pts[:, :3]) > 1e18).any(1)
    assert near.sum() > 900
    rec_t, map_t, pts_t = _dev(K.records(g, "fractional")), _dev(DC.flt_max_maps(g)), _dev(pts)
    out = [torch.zeros(4 * len(pts), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    gpu_ctx.volume_sample_device(g, rec_t, pts_t, out[0], sync=True)
    gpu_ctx.volume_sample_visible_device(g, rec_t, map_t, hip.VOLUME_VIS_PARAMS(0.25, 0.05), pts_t, out[1], sync=True)
    plain, vis = (o.cpu().numpy().reshape(-1, 4) for o in out)
    DC.same(vis[near], plain[near], "identity on the device")


def test_sampler_on_a_torch_stream(gpu_ctx):
    import torch
    g = K.grid((5, 4, 3))
    rec, maps = K.records(g, "fractional"), DC.random_maps(g)
    pts = _mixed(g)
    vp = hip.VOLUME_VIS_PARAMS(0.25, 0.05)
    want = D.sample_visible(g, rec, maps, 0.25, 0.05, pts[:, :3], pts[:, 3:])
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rec_t, map_t, pts_t = _dev(rec), _dev(maps), _dev(pts)
        out = [torch.zeros(4 * len(pts), dtype=torch.float32, device=dev) for _ in range(2)]
        assert gpu_ctx.volume_sample_visible_device(g, rec_t, map_t, vp, pts_t, out[0]) is None  # seconds == NULL: enqueued, not waited for
        sec = gpu_ctx.volume_sample_visible_device(g, rec_t, map_t, vp, pts_t, out[1], sync=True)
    stream.synchronize()
    assert sec > 0
    a, b = (o.cpu().numpy().reshape(-1, 4) for o in out)
    assert a.tobytes() == b.tobytes()
    DC.same(a, want, "on a torch stream")


def test_zero_copy_chain_on_scene_6():
    """probes -> probe_depth_bake_device; camera rays -> query_closest_device -> the hits tensor ->
    volume_sample_visible_device(stride=48), nothing copied: bit for bit the host chain and the restatement"""
    import torch
    world, cam, rays, hits = K.scene6()
    g, want_maps = DC.scene6_maps()
    rec = K.records(g, "ones", seed=9)
    vp = hip.VOLUME_VIS_PARAMS(5.0, 0.05)
    params = hip.DEPTH_PARAMS(2, float(DC.SCENE6_CAP))
    host_maps = hip.probe_depth_bake_host(world, params, hip.volume_probes(g), nthreads=4)["depth"]
    want = hip.volume_sample_visible_host(g, rec, host_maps, vp, hits, nthreads=4)["out"]
    DC.same(want, D.sample_visible(g, rec, want_maps, 5.0, 0.05, hits["p"], hits["normal"]), "scene 6 host chain")
    dev = torch.device("cuda:0")
    n = len(rays)
    with hip.Context(0) as ctx:
        ctx.upload_world(world)
        rays_t = torch.from_numpy(rays.reshape(-1).copy()).to(dev)
        hits_t = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
        out_t = torch.zeros(n * 4, dtype=torch.float32, device=dev)
        map_t = torch.zeros(g.probes * 200, dtype=torch.float32, device=dev)
        ctx.probe_depth_bake_device(params, _dev(hip.volume_probes(g)).view(torch.float32), map_t)
        ctx.query_closest_device(rays_t, hits_t)
        ctx.volume_sample_visible_device(g, _dev(rec), map_t, vp, hits_t, out_t, stride=48, sync=True)
        DC.same(map_t.cpu().numpy().reshape(-1, 200), want_maps, "scene 6 maps on the device")
        DC.same(out_t.cpu().numpy().reshape(-1, 4), want, "scene 6 zero-copy chain")


def test_sampler_argument_checks_on_the_device():
    import torch
    g = K.grid((2, 2, 2))
    n, stride = 5, 48
    L = hip.lib()
    dev = torch.device("cuda:0")
    with hip.Context(0) as ctx:
        span16 = ((n - 1) * stride + 24 + 15) // 16 * 16
        buf = torch.zeros(8 * 128 + 8 * 800 + span16 + n * 16 + 4096, dtype=torch.uint8, device=dev)
        base = buf.data_ptr()
        d_rec, d_map = base, base + 8 * 128
        d_pts = d_map + 8 * 800
        d_out = d_pts + span16
        assert all(a % 16 == 0 for a in (d_rec, d_map, d_pts, d_out))
        gp, good = C.byref(g), hip.VOLUME_VIS_PARAMS(0.5, 0.05)
        call = lambda q, r, d, v, m, p, s, o: L.mort_hip_volume_sample_visible_device(ctx._h, q, r, d, C.byref(v) if v is not None else None, m, p, s, o, None, None)  # noqa: E731
        assert call(gp, d_rec, d_map, good, 0, d_pts, stride, d_out) == 0, "an empty batch launches nothing"
        for a in ((None, d_rec, d_map, good), (gp, None, d_map, good), (gp, d_rec, None, good), (gp, d_rec, d_map, None)):
            assert call(*a, n, d_pts, stride, d_out) == INVALID
        assert call(gp, d_rec, d_map, good, n, None, stride, d_out) == INVALID and call(gp, d_rec, d_map, good, n, d_pts, stride, None) == INVALID
        for bias, minv in ((-1.0, 0.05), (np.nan, 0.05), (np.inf, 0.05), (0.5, -0.1), (0.5, 1.5), (0.5, np.nan)):
            assert call(gp, d_rec, d_map, hip.VOLUME_VIS_PARAMS(bias, minv), n, d_pts, stride, d_out) == INVALID, (bias, minv)
        for bad in (0, 20, 46):
            assert call(gp, d_rec, d_map, good, n, d_pts, bad, d_out) == INVALID, bad
        assert call(gp, d_rec, d_map, good, n, d_pts, stride, d_map + 8 * 800 - 16) == INVALID  # the output over the maps' tail
        assert call(gp, d_rec, d_map, good, n, d_pts, stride, d_map) == INVALID
        assert call(gp, d_rec, d_map, good, n, d_pts, stride, d_pts + 32) == INVALID
        for a in ((d_rec + 4, d_map, d_pts, d_out), (d_rec, d_map + 8, d_pts, d_out), (d_rec, d_map, d_pts + 8, d_out + 16), (d_rec, d_map, d_pts, d_out + 4)):
            assert call(gp, a[0], a[1], good, n, a[2], stride, a[3]) == INVALID, "not 16-byte aligned"
        torch.cuda.synchronize()
        assert (buf == 0).all(), "a refused call writes nothing"
