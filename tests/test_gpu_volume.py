"""Irradiance volumes on the MI355X (volume.hip): volume_sample_kernel and volume_pack_kernel must give the host
forms' answers (the same bodies, dev_volume.h) and the restatement's of tests/volume_ref.py at tolerance 0 -- outputs as raw
words, any NaN equal to any NaN -- at point counts that leave partial waves and partial groups, at the three strides, under masks
that make neighbouring lanes skip different corners; on torch tensors and torch streams, straight from the hits tensor of a
closest-hit query; and they must write nothing past their outputs and leave the render's state alone."""
import ctypes as C

import numpy as np
import pytest

from mort_amd import hip, host
from tests import oracle_lib as O
from tests import volume_cases as K
from tests import volume_ref as V

pytestmark = pytest.mark.gpu

F = np.float32
NS = (1, 63, 64, 65, 255, 256, 257, 1000)
INVALID = -1


def _same(got, want, what):
    bad = np.flatnonzero((K.words(got) != K.words(want)).reshape(len(want), -1).any(1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} differ, first {bad[0]}: {got[bad[0]]} / {want[bad[0]]}"


def _mixed(g, seed=2):
    """1000 of the parity points in a fixed shuffled order, so that every prefix holds every kind"""
    pts = K.points(g, 900, seed)
    return pts[np.random.default_rng(seed).permutation(len(pts))[:1000]]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda:0"))


@pytest.mark.parametrize("mask", ["ones", "holes", "fractional"])
@pytest.mark.parametrize("count", K.COUNTS)
def test_device_equals_host_equals_restatement(gpu_ctx, count, mask):
    g = K.grid(count)
    rec = K.records(g, mask)
    pts = _mixed(g)
    assert len(pts) == max(NS)
    want = V.sample(g, rec, pts[:, :3], pts[:, 3:])
    _same(hip.volume_sample_host(g, rec, pts, nthreads=4)["out"], want, f"grid {count} {mask} host")
    for n in NS:
        got = gpu_ctx.volume_sample(g, rec, pts[:n])["out"]
        _same(got, want[:n], f"grid {count} {mask} n={n} device")
    if mask == "holes" and g.probes > 1:
        fin = np.isfinite(pts).all(1)
        assert np.isfinite(want[fin]).all(), "a masked probe's NaN poisons nothing"
        # neighbouring lanes skip different corners: the contributing sets differ inside a wave
        used = []
        V.sample(g, rec, pts[:64, :3], pts[:64, 3:], census=used)
        assert len(set(used[0].tolist())) > 1


def test_strides_on_tensors(gpu_ctx):
    import torch
    g = K.grid((4, 3, 2))
    rec = K.records(g, "fractional")
    pts = _mixed(g)[:257]
    want = V.sample(g, rec, pts[:, :3], pts[:, 3:])
    rec_t = _dev(rec)
    for stride, fill in ((24, 0), (40, 0xa5), (40, 0xff), (48, 0xa5)):
        pts_t = _dev(K.strided(pts, stride, fill))
        out_t = torch.zeros(4 * len(pts), dtype=torch.float32, device=pts_t.device)
        sec = gpu_ctx.volume_sample_device(g, rec_t, pts_t, out_t, stride=stride, sync=True)
        assert sec > 0
        _same(out_t.cpu().numpy().reshape(-1, 4), want, f"stride {stride} fill {fill:#x}")
        _same(gpu_ctx.volume_sample(g, rec, K.strided(pts, stride, fill), stride=stride)["out"], want, f"stride {stride} host-buffer form")


def test_pack_device_equals_host(gpu_ctx):
    import torch
    for n in (1, 7, 8, 9, 31, 32, 33, 1000):
        rng = np.random.default_rng(n)
        sh = rng.uniform(-3, 3, size=(n, 27)).astype(F)
        sh.view(np.uint32)[0, 5] = 0x7fc12345  # a NaN payload travels
        sh.view(np.uint32)[n // 2, 26] = 0xffa00001
        wt = rng.uniform(0, 2, size=n).astype(F)
        for w in (wt, None):
            want = hip.volume_pack_host(sh, w)["records"]
            assert (want.view(np.uint32) == V.pack(sh, w).view(np.uint32)).all()
            got = gpu_ctx.volume_pack(sh, w)["records"]
            assert (got.view(np.uint32) == want.view(np.uint32)).all(), (n, w is None)
            # the _device form into the head of a larger tensor: the bytes past 128 n keep theirs
            rec_t = torch.full((n * 128 + 256,), 0xa5, dtype=torch.uint8, device="cuda:0")
            gpu_ctx.volume_pack_device(_dev(sh).view(torch.float32), rec_t[:n * 128], weight=_dev(w).view(torch.float32) if w is not None else None, sync=True)
            out = rec_t.cpu().numpy()
            assert (out[n * 128:] == 0xa5).all(), f"n={n}: records written past the batch"
            assert (out[:n * 128].view(np.uint32) == want.view(np.uint32).reshape(-1)).all()


def test_bytes_past_the_batch_are_untouched(gpu_ctx):
    import torch
    g = K.grid((5, 4, 3))
    rec = K.records(g)
    pts = _mixed(g)
    want = V.sample(g, rec, pts[:, :3], pts[:, 3:])
    rec_t, pts_t = _dev(rec), _dev(pts)
    for n in (1, 63, 65, 255, 257, 1000):  # the last group is partial: its lanes past n must not store
        out_t = torch.full((n * 16 + 4096,), 0xa5, dtype=torch.uint8, device="cuda:0")
        gpu_ctx.volume_sample_device(g, rec_t, pts_t[:n * 24], out_t[:n * 16], sync=True)
        out = out_t.cpu().numpy()
        assert (out[n * 16:] == 0xa5).all(), f"n={n}: output written past the batch"
        _same(out[:n * 16].view(F).reshape(-1, 4), want[:n], f"n={n} into the head of a larger tensor")


def test_device_form_on_a_torch_stream(gpu_ctx):
    """on a stream other than the context's; one asynchronous call, then a timed one: equal results, the restatement's"""
    import torch
    g = K.grid((5, 4, 3))
    rec = K.records(g, "fractional")
    pts = _mixed(g)
    want = V.sample(g, rec, pts[:, :3], pts[:, 3:])
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rec_t, pts_t = _dev(rec), _dev(pts)
        out = [torch.zeros(4 * len(pts), dtype=torch.float32, device=dev) for _ in range(2)]
        assert gpu_ctx.volume_sample_device(g, rec_t, pts_t, out[0]) is None  # seconds == NULL: enqueued, not waited for
        sec = gpu_ctx.volume_sample_device(g, rec_t, pts_t, out[1], sync=True)
    stream.synchronize()
    assert sec > 0
    a, b = (o.cpu().numpy().reshape(-1, 4) for o in out)
    assert a.tobytes() == b.tobytes()
    _same(a, want, "on a torch stream")
    # the context's own stream (stream == NULL) gives the same
    out2 = torch.zeros(4 * len(pts), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    sec = C.c_double(0)
    assert hip.lib().mort_hip_volume_sample_device(gpu_ctx._h, C.byref(g), rec_t.data_ptr(), len(pts), pts_t.data_ptr(), 24, out2.data_ptr(), None, C.byref(sec)) == 0
    _same(out2.cpu().numpy().reshape(-1, 4), want, "on the context's stream")


def test_zero_copy_chain_on_scene_6(gpu_ctx):
    """camera rays -> query_closest_device -> the hits tensor -> volume_sample_device(stride=48), nothing copied: bit for bit the
    host chain"""
    import torch
    world, cam, rays, hits = K.scene6()
    g = K.scene6_grid()
    rec = K.records(g, "ones", seed=9)
    want = hip.volume_sample_host(g, rec, hits, nthreads=4)["out"]
    _same(want, V.sample(g, rec, hits["p"], hits["normal"]), "scene 6 host chain")
    gpu_ctx.upload_world(world)
    dev = torch.device("cuda:0")
    n = len(rays)
    rays_t = torch.from_numpy(rays.reshape(-1).copy()).to(dev)
    hits_t = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
    out_t = torch.zeros(n * 4, dtype=torch.float32, device=dev)
    rec_t = _dev(rec)
    gpu_ctx.query_closest_device(rays_t, hits_t)
    gpu_ctx.volume_sample_device(g, rec_t, hits_t, out_t, stride=48, sync=True)
    _same(out_t.cpu().numpy().reshape(-1, 4), want, "scene 6 zero-copy chain")


def test_samples_leave_the_render_alone():
    """two frames with a sample before and between them equal two frames on a fresh context: image, accumulators, segment counts,
    RNG states, and the second frame's statistics"""
    world, cam = host.build_scene(1, width=160, spp=4)
    W, H = cam.image_width, cam.image_height
    g = K.grid((4, 3, 2))
    rec, pts = K.records(g), _mixed(g)

    def frames(with_samples):
        out = []
        with hip.Context(0) as ctx:
            if with_samples:  # before the world is uploaded: a sample needs none
                ctx.volume_sample(g, rec, pts)
            ctx.upload_world(world)
            ctx.rng_seed(69420, W, H)
            for f in range(2):
                if with_samples and f:
                    ctx.volume_sample(g, rec, pts)
                    ctx.volume_pack(rec[:, :27].copy())
                r = ctx.render(cam, want_accum=True, want_segments=True)
                r["states"] = ctx.rng_store(W, H, O.STATE_DTYPE)
                out.append(r)
        return out

    plain, mixed = frames(False), frames(True)
    for f, (a, b) in enumerate(zip(plain, mixed)):
        assert (a["rgba"] == b["rgba"]).all(), f
        assert (a["accum"].view(np.uint32) == b["accum"].view(np.uint32)).all(), f
        assert (a["segments_px"] == b["segments_px"]).all(), f
        for k in ("d", "v", "bf", "bfd", "be", "bed"):
            assert (a["states"][k] == b["states"][k]).all(), (f, k)
        for k in ("segments", "pixels", "eff_samples", "rng_draws", "reference_walks", "kernel_name", "kernel_vgprs", "kernel_lds_bytes", "scene_in_lds"):
            assert a["stats"][k] == b["stats"][k], (f, k)


def test_argument_checks_on_the_device_and_no_world():
    import torch
    g = K.grid((2, 2, 2))
    rec = K.records(g)
    n, stride = 5, 48
    pts = _mixed(g)[:n]
    L = hip.lib()
    dev = torch.device("cuda:0")
    with hip.Context(0) as ctx:  # no world is ever uploaded
        span = (n - 1) * stride + 24
        span16 = (span + 15) // 16 * 16
        buf = torch.zeros(8 * 128 + span16 + n * 16 + 4096, dtype=torch.uint8, device=dev)
        base = buf.data_ptr()
        d_rec, d_pts, d_out = base, base + 8 * 128, base + 8 * 128 + span16
        assert all(a % 16 == 0 for a in (d_rec, d_pts, d_out))
        gp = C.byref(g)
        call = lambda q, r, m, p, s, o: L.mort_hip_volume_sample_device(ctx._h, q, r, m, p, s, o, None, None)  # noqa: E731
        assert call(gp, d_rec, 0, d_pts, stride, d_out) == 0, "an empty batch launches nothing"
        for a in ((None, d_rec, n, d_pts, stride, d_out), (gp, None, n, d_pts, stride, d_out), (gp, d_rec, n, None, stride, d_out),
                  (gp, d_rec, n, d_pts, stride, None)):
            assert call(*a) == INVALID
        for bad in (0, 20, 23, 25, 46):
            assert call(gp, d_rec, n, d_pts, bad, d_out) == INVALID, bad
        for kw in (dict(spacing=(0, 1, 1)), dict(count=(0, 2, 2)), dict(count=(2, 2, 4097)), dict(origin=(np.nan, 0, 0)), dict(count=(2048, 2048, 512))):
            q = hip.VOLUME_GRID(kw.get("origin", (0, 0, 0)), kw.get("spacing", (1, 1, 1)), kw.get("count", (2, 2, 2)), 0.5)
            assert call(C.byref(q), d_rec, n, d_pts, stride, d_out) == INVALID, kw
        assert call(gp, d_rec, n, d_pts, stride, d_pts + span - 8) == INVALID   # the output over the last point
        assert call(gp, d_rec, n, d_pts, stride, d_pts + 32) == INVALID          # between two points is inside the span
        assert call(gp, d_rec, n, d_pts, stride, d_rec + 8 * 128 - 16) == INVALID  # over the records' tail
        for a in ((d_rec + 4, d_pts, d_out), (d_rec, d_pts + 8, d_out + 16), (d_rec, d_pts, d_out + 4)):
            assert call(gp, a[0], n, a[1], stride, a[2]) == INVALID, "not 16-byte aligned"
        pk = lambda m, s, w, r: L.mort_hip_volume_pack_device(ctx._h, m, s, w, r, None, None)  # noqa: E731
        assert pk(0, d_rec, None, d_out) == 0
        assert pk(2, None, None, d_out) == INVALID and pk(2, d_rec, None, None) == INVALID
        assert pk(2, d_rec, None, d_rec + 208) == INVALID and pk(2, d_rec + 4, None, d_out) == INVALID and pk(2, d_rec, d_pts + 4, d_out) == INVALID
        torch.cuda.synchronize()
        assert (buf == 0).all(), "a refused call writes nothing"
        # and the checks refuse nothing they should not: a context with no world uploaded samples and packs
        want = V.sample(g, rec, pts[:, :3], pts[:, 3:])
        _same(ctx.volume_sample(g, rec, K.strided(pts, stride), stride=stride)["out"], want, "no world uploaded")
        buf[:8 * 128] = _dev(rec)
        buf[8 * 128:8 * 128 + span] = _dev(K.strided(pts, stride)[:span])
        sec = C.c_double(0)
        assert L.mort_hip_volume_sample_device(ctx._h, gp, d_rec, n, d_pts, stride, d_out, None, C.byref(sec)) == 0 and sec.value > 0
        _same(buf[8 * 128 + span16:8 * 128 + span16 + n * 16].cpu().numpy().view(F).reshape(-1, 4), want, "side by side in one allocation")
        assert (ctx.volume_pack(rec[:, :27].copy())["records"].view(np.uint32) == rec.view(np.uint32)).all()
