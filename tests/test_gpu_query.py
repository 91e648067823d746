"""Ray queries on the MI355X (query.hip): query_closest_kernel and query_occluded_kernel must give the host forms'
answers (the same bodies, dev_query.h) and the CPU oracle's world::hit, tolerance 0, on the ray sets of tests/query_rays.py --
primary, secondary, interval, far, axis -- with and without streams; at every batch size around a wave and a group; on torch
tensors and torch streams; and they must leave the render's state alone."""
import ctypes as C

import numpy as np
import pytest

from mort_amd import hip, host
from tests import oracle_lib as O
from tests import query_rays as Q

pytestmark = pytest.mark.gpu

# scenes 1 and 10: reference BVHs (the item loop's threaded walk); 3: flat lists; 6, 7, 9: the unified tree, 7 and 9 with media;
# two awkward worlds (instances under chains in the tree; a list scanned after a medium: the item loop with media);
# two random reference BVHs (one `ties`, one above the limit on the LDS images); three random worlds
WORLDS = ("scene1", "scene3", "scene6", "scene7", "scene9", "scene10", "flat:boxes_and_instances", "flat:media_then_list",
          "bvhrandom:ties_64_s0", "bvhrandom:ties_670_s1", "random:0", "random:3", "random:7") + tuple(f"genrandom:{n}" for n in Q.GEN_RANDOM_PICK)
SIZES = (1, 63, 64, 65, 255, 256, 257, 1296)
NO_WORLD, INVALID = -4, -1


def _same_records(a, b, what):
    """two query results field by field, NaNs read as one word (tests/query_rays.py _words)"""
    for k in ("p", "normal", "t", "u", "v"):
        assert (Q._words(a[k]) == Q._words(b[k])).all(), f"{what}: {k} differs"
    for k in ("mat_type", "mat_idx", "flags"):
        assert (a[k] == b[k]).all(), f"{what}: {k} differs"


@pytest.mark.parametrize("name", WORLDS)
def test_device_equals_host_equals_oracle(gpu_ctx, name):
    s = Q.build(name)
    Q.census(s)
    assert len(s.all) <= 20000
    gpu_ctx.upload_world(s.world)
    tree = Q.reach(s.world)["tree"]
    # without streams: media passed over
    got = gpu_ctx.query_closest(s.all)["hits"]
    Q.assert_hits_equal(s.world, got, s.rec, s.hit, f"{name} device")
    _same_records(got, hip.query_closest_host(s.world, s.all, tree=tree, nthreads=16)["hits"], f"{name} device / host")
    # with streams: media as world::hit evaluates them, the streams advanced in place
    streams = s.streams0.copy()
    got = gpu_ctx.query_closest(s.all, states=streams)["hits"]
    Q.assert_hits_equal(s.world, got, s.mrec, s.mhit, f"{name} device with streams", with_media=True)
    assert streams.tobytes() == s.streams.tobytes(), f"{name}: final stream states differ from the oracle's"
    hs = s.streams0.copy()
    _same_records(got, hip.query_closest_host(s.world, s.all, states=hs, tree=tree, nthreads=16)["hits"], f"{name} device / host with streams")
    assert hs.tobytes() == streams.tobytes()
    # occlusion
    occ = gpu_ctx.query_occluded(s.all)["occluded"]
    bad = np.flatnonzero(occ != s.hit.astype(np.uint8))
    assert bad.size == 0, f"{name}: occlusion differs for {bad.size} rays, first {bad[0]}: {s.all[bad[0]]}"
    assert (occ == hip.query_occluded_host(s.world, s.all, tree=tree, nthreads=16)["occluded"]).all()


def _mixed(s, waves=24, seed=3):
    """far, axis, interval and ordinary rays in every wave of 64: 6 + 6 + 20 + 32 of them, shuffled within the wave"""
    rng = np.random.default_rng(seed)
    pools = [np.arange(s.slices[k].start, s.slices[k].stop) for k in ("far", "axis", "interval")]
    pools.append(np.concatenate([np.arange(s.slices[k].start, s.slices[k].start + 400) for k in ("primary", "secondary")]))
    share = (6, 6, 20, 32)
    idx = []
    for w in range(waves):
        lane = np.concatenate([np.take(pool, np.arange(w * m, (w + 1) * m), mode="wrap") for pool, m in zip(pools, share)])
        idx.append(rng.permutation(lane))
    return np.concatenate(idx)


@pytest.mark.parametrize("name", ["scene7", "scene1", "scene6"])
def test_far_axis_and_ordinary_rays_in_one_wave(gpu_ctx, name):
    s = Q.build(name)
    idx = _mixed(s)
    rays = np.ascontiguousarray(s.all[idx])
    gpu_ctx.upload_world(s.world)
    Q.assert_hits_equal(s.world, gpu_ctx.query_closest(rays)["hits"], s.rec[idx], s.hit[idx], f"{name} mixed")
    streams = np.ascontiguousarray(s.streams0[idx])
    got = gpu_ctx.query_closest(rays, states=streams)["hits"]
    Q.assert_hits_equal(s.world, got, s.mrec[idx], s.mhit[idx], f"{name} mixed with streams", with_media=True)
    assert streams.tobytes() == np.ascontiguousarray(s.streams[idx]).tobytes()
    assert (gpu_ctx.query_occluded(rays)["occluded"] == s.hit[idx].astype(np.uint8)).all()


@pytest.mark.parametrize("name", ["scene7", "scene1"])
def test_partial_waves_and_groups(gpu_ctx, name):
    """n around a wave (64) and a group (256): the rays past n are not there, the bytes past n are not written"""
    import torch
    s = Q.build(name)
    idx = _mixed(s)
    gpu_ctx.upload_world(s.world)
    dev = torch.device("cuda:0")
    nmax = max(SIZES)
    rays_t = torch.from_numpy(np.ascontiguousarray(s.all[idx[:nmax + 64]])).to(dev)
    for n in SIZES:
        sub = idx[:n]
        # host-buffer forms
        Q.assert_hits_equal(s.world, gpu_ctx.query_closest(np.ascontiguousarray(s.all[sub]))["hits"], s.rec[sub], s.hit[sub], f"{name} n={n}")
        streams = np.ascontiguousarray(s.streams0[sub])
        got = gpu_ctx.query_closest(np.ascontiguousarray(s.all[sub]), states=streams)["hits"]
        Q.assert_hits_equal(s.world, got, s.mrec[sub], s.mhit[sub], f"{name} n={n} with streams", with_media=True)
        assert streams.tobytes() == np.ascontiguousarray(s.streams[sub]).tobytes()
        assert (gpu_ctx.query_occluded(np.ascontiguousarray(s.all[sub]))["occluded"] == s.hit[sub].astype(np.uint8)).all()
        # _device forms into the head of larger tensors: the tail keeps its bytes
        hits_t = torch.full(((n + 64) * 48,), 0xa5, dtype=torch.uint8, device=dev)
        st_t = torch.from_numpy(np.ascontiguousarray(s.streams0[idx[:n + 64]]).view(np.uint8).reshape(-1).copy()).to(dev)
        occ_t = torch.full((n + 64,), 0xa5, dtype=torch.uint8, device=dev)
        gpu_ctx.query_closest_device(rays_t[:n], hits_t[:n * 48], states=st_t[:n * 48], sync=True)
        gpu_ctx.query_occluded_device(rays_t[:n], occ_t[:n], sync=True)
        h = hits_t.cpu().numpy()
        assert (h[n * 48:] == 0xa5).all() and (occ_t.cpu().numpy()[n:] == 0xa5).all(), f"n={n}: written past the batch"
        _same_records(h[:n * 48].view(hip.HIT_DTYPE), got, f"{name} n={n} device form")
        st = st_t.cpu().numpy()
        assert st[:n * 48].tobytes() == streams.tobytes() and st[n * 48:].tobytes() == np.ascontiguousarray(s.streams0[idx[n:n + 64]]).tobytes()
        assert (occ_t.cpu().numpy()[:n] == s.hit[sub].astype(np.uint8)).all()


def test_device_form_on_a_torch_stream(gpu_ctx):
    """on a stream other than the context's; one asynchronous call, then a timed one: equal results, the oracle's"""
    import torch
    s = Q.build("scene9")
    gpu_ctx.upload_world(s.world)
    dev = torch.device("cuda:0")
    n = len(s.all)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rays = torch.from_numpy(s.all.copy()).to(dev)
        out = [torch.zeros(n * 48, dtype=torch.uint8, device=dev) for _ in range(2)]
        occ = [torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2)]
        st = [torch.from_numpy(s.streams0.view(np.uint8).reshape(-1).copy()).to(dev) for _ in range(2)]
        assert gpu_ctx.query_closest_device(rays, out[0], states=st[0]) is None  # seconds == NULL: enqueued, not waited for
        assert gpu_ctx.query_occluded_device(rays, occ[0]) is None
        sec = gpu_ctx.query_closest_device(rays, out[1], states=st[1], sync=True)
        sec_o = gpu_ctx.query_occluded_device(rays, occ[1], sync=True)
    stream.synchronize()
    assert sec > 0 and sec_o > 0
    a, b = (o.cpu().numpy().view(hip.HIT_DTYPE) for o in out)
    assert a.tobytes() == b.tobytes() and (occ[0] == occ[1]).all() and (st[0] == st[1]).all()
    Q.assert_hits_equal(s.world, a, s.mrec, s.mhit, "scene9 on a torch stream", with_media=True)
    assert st[0].cpu().numpy().tobytes() == s.streams.tobytes()
    assert (occ[0].cpu().numpy() == s.hit.astype(np.uint8)).all()
    # the context's own stream (stream == NULL) gives the same
    out2 = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sec = C.c_double(0)
    assert hip.lib().mort_hip_query_closest_device(gpu_ctx._h, n, rays.data_ptr(), None, out2.data_ptr(), None, C.byref(sec)) == 0
    Q.assert_hits_equal(s.world, out2.cpu().numpy().view(hip.HIT_DTYPE), s.rec, s.hit, "scene9 on the context's stream")


@pytest.mark.parametrize("sid", [1, 9])
def test_queries_leave_the_render_alone(sid):
    """two frames with queries before, between and after them equal two frames on a fresh context: image, accumulators, segment
    counts, RNG states, and the second frame's statistics (its tile order comes from the first frame's costs)"""
    world, cam = host.build_scene(sid, width=160, spp=4)
    W, H = cam.image_width, cam.image_height
    s = Q.build(f"scene{sid}")
    rays = np.ascontiguousarray(s.all[:2000])

    def frames(with_queries):
        out = []
        with hip.Context(0) as ctx:
            ctx.upload_world(world)
            if with_queries:
                ctx.query_closest(rays)  # before any rng_seed: queries need no pixel RNG
            ctx.rng_seed(69420, W, H)
            for f in range(2):
                if with_queries:
                    ctx.query_closest(rays)
                    ctx.query_closest(rays, states=s.streams0[:2000].copy())
                    ctx.query_occluded(rays)
                r = ctx.render(cam, want_accum=True, want_segments=True)
                r["states"] = ctx.rng_store(W, H, O.STATE_DTYPE)
                out.append(r)
        return out

    plain, mixed = frames(False), frames(True)
    for f, (a, b) in enumerate(zip(plain, mixed)):
        assert (a["rgba"] == b["rgba"]).all(), f
        assert (a["accum"].view(np.uint32) == b["accum"].view(np.uint32)).all(), f
        assert (a["segments_px"] == b["segments_px"]).all(), f
        for k in ("d", "v", "bf", "bfd", "be", "bed"):  # every field of the 48-byte record; its 4 padding bytes are never written
            assert (a["states"][k] == b["states"][k]).all(), (f, k)
        for k in ("segments", "pixels", "eff_samples", "rng_draws", "reference_walks", "kernel_name", "kernel_vgprs", "kernel_lds_bytes", "scene_in_lds"):
            assert a["stats"][k] == b["stats"][k], (f, k)


def test_queries_ignore_the_partition(gpu_ctx):
    s = Q.build("scene6")
    gpu_ctx.upload_world(s.world)
    whole = gpu_ctx.query_closest(s.all)["hits"]
    occ = gpu_ctx.query_occluded(s.all)["occluded"]
    try:
        gpu_ctx.set_partition(1, 2)
        assert gpu_ctx.query_closest(s.all)["hits"].tobytes() == whole.tobytes()
        assert (gpu_ctx.query_occluded(s.all)["occluded"] == occ).all()
    finally:
        gpu_ctx.set_partition(0, 1)
    Q.assert_hits_equal(s.world, whole, s.rec, s.hit, "scene6")


def test_argument_checks_on_the_device():
    import torch
    s = Q.build("scene2")
    L = hip.lib()
    rays = np.ascontiguousarray(s.all[:64])
    dev = torch.device("cuda:0")
    with hip.Context(0) as ctx:
        for call in (lambda: ctx.query_closest(rays), lambda: ctx.query_occluded(rays)):
            with pytest.raises(hip.MortHipError) as e:
                call()
            assert e.value.status == NO_WORLD
        buf = torch.zeros(64 * 48 * 4, dtype=torch.uint8, device=dev)
        base = buf.data_ptr()
        assert L.mort_hip_query_closest_device(ctx._h, 64, base, None, base + 64 * 32, None, None) == NO_WORLD
        ctx.upload_world(s.world)
        torch.cuda.synchronize()
        # an empty batch launches nothing and is fine; NULL buffers, overlapping buffers and misaligned device buffers are not
        assert L.mort_hip_query_closest_device(ctx._h, 0, base, None, base + 64 * 32, None, None) == 0
        assert L.mort_hip_query_occluded_device(ctx._h, 0, base, base + 64 * 32, None, None) == 0
        assert L.mort_hip_query_closest(ctx._h, 0, rays.ctypes.data, None, rays.ctypes.data + 4096, None) == 0
        assert L.mort_hip_query_closest_device(ctx._h, 64, None, None, base, None, None) == INVALID
        assert L.mort_hip_query_closest_device(ctx._h, 64, base, None, None, None, None) == INVALID
        assert L.mort_hip_query_occluded_device(ctx._h, 64, base, None, None, None) == INVALID
        assert L.mort_hip_query_closest_device(ctx._h, 64, base, None, base + 64 * 32 - 16, None, None) == INVALID  # records over the rays' tail
        assert L.mort_hip_query_closest_device(ctx._h, 64, base, base + 64 * 32 + 48, base + 64 * 32, None, None) == INVALID  # streams over the records
        assert L.mort_hip_query_occluded_device(ctx._h, 64, base, base + 63 * 32, None, None) == INVALID
        assert L.mort_hip_query_closest_device(ctx._h, 64, base + 4, None, base + 64 * 48, None, None) == INVALID  # not 16-byte aligned
        hits = np.zeros(64, dtype=hip.HIT_DTYPE)
        assert L.mort_hip_query_closest(ctx._h, 64, rays.ctypes.data, None, rays.ctypes.data + 16, None) == INVALID
        assert L.mort_hip_query_closest(ctx._h, 64, None, None, hits.ctypes.data, None) == INVALID
        assert (buf == 0).all()
        # and the checks refuse nothing they should not
        Q.assert_hits_equal(s.world, ctx.query_closest(rays)["hits"], s.rec[:64], s.hit[:64], "scene2")
