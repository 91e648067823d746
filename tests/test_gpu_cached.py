"""Cached radiance queries on the MI355X (cached.hip): query_radiance_cached_kernel<TREE, VISIBLE> must give the host
form's answers (the same body, dev_cached.h) and those of the walk over the oracle (tests/cached_ref.py), tolerance 0 -- colours as
raw words (any NaN equals any NaN), final streams as all 48 bytes, the counts -- on scene 6 and a lit flat world with media (the
TREE kernels) and on scene 1 (the item loop over a reference BVH); at every batch size around a wave and a group; on torch tensors
and torch streams; and it must leave the render's state alone."""
import ctypes as C

import numpy as np
import pytest

from mort_amd import hip, host, structs as S
from tests import cached_ref as CR
from tests import oracle_lib as O
from tests import query_rays as Q
from tests import radiance_ref as R
from tests.test_gpu_radiance import SIZES, _mixed

pytestmark = pytest.mark.gpu

NO_WORLD, INVALID, CAPACITY = -4, -1, -7


def test_the_worlds_run_both_kernels():
    assert [bool(Q.reach(Q.build(n).world)["tree"]) for n in CR.WORLDS] == [True, False, True]


@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("depth", CR.DEPTHS)
@pytest.mark.parametrize("mask,samples", CR.CASES)
@pytest.mark.parametrize("name", CR.WORLDS)
def test_device_equals_host_equals_reference(gpu_ctx, name, mask, samples, depth, visible):
    ref = CR.reference(name, depth, samples, mask, visible)
    gpu_ctx.upload_world(ref.world)
    streams = ref.streams0.copy()
    got = gpu_ctx.query_radiance_cached(ref.params, ref.rays, streams, ref.records, ref.depth)
    CR.assert_equal(got, streams, ref, f"{name} {mask} samples={samples} K={depth} visible={visible} device")
    hs = ref.streams0.copy()
    h = hip.query_radiance_cached_host(ref.world, ref.params, ref.rays, hs, ref.records, ref.depth, tree=Q.reach(ref.world)["tree"], nthreads=16)
    assert (Q._words(h["rgb"]) == Q._words(got["rgb"])).all() and hs.tobytes() == streams.tobytes() and (h["ends"] == got["ends"]).all(), "device / host"


@pytest.mark.parametrize("visible", [False, True])
def test_baked_volume_on_scene_6(gpu_ctx, visible):
    ref = CR.reference("scene6", 1, 1, "baked", visible)
    gpu_ctx.upload_world(ref.world)
    streams = ref.streams0.copy()
    got = gpu_ctx.query_radiance_cached(ref.params, ref.rays, streams, ref.records, ref.depth)
    CR.assert_equal(got, streams, ref, f"scene6 baked visible={visible} device")


def _tensors(torch, dev, ref):
    rec = torch.from_numpy(np.array(ref.records)).to(dev)  # copies: the reference's arrays are read-only
    dep = torch.from_numpy(np.array(ref.depth)).to(dev) if ref.depth is not None else None
    return rec, dep


@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("name", ["scene6", "scene1"])
def test_partial_waves_and_groups(gpu_ctx, name, visible):
    """n around a wave (64) and a group (256), far, axis and ordinary rays in every wave, under the slab mask (paths that end in
    the volume and Lambertian hits that fall through side by side): the rays past n are not there, the bytes past n of the colours,
    the streams and the counts are not written"""
    import torch
    ref = CR.reference(name, 1, 3, "slab", visible)
    idx = _mixed(ref)
    assert len(idx) >= max(SIZES) + 64
    gpu_ctx.upload_world(ref.world)
    dev = torch.device("cuda:0")
    rays_t = torch.from_numpy(np.ascontiguousarray(ref.rays[idx[:max(SIZES) + 64]])).to(dev)
    rec_t, dep_t = _tensors(torch, dev, ref)
    for n in SIZES:
        sub = idx[:n]
        streams = np.ascontiguousarray(ref.streams0[sub])
        got = gpu_ctx.query_radiance_cached(ref.params, np.ascontiguousarray(ref.rays[sub]), streams, ref.records, ref.depth)
        CR.assert_equal(got, streams, ref, f"{name} n={n}", idx=sub)
        # the _device form into the head of larger tensors: the tails keep their bytes
        rgb_t = torch.full(((n + 64) * 12,), 0xa5, dtype=torch.uint8, device=dev)
        ends_t = torch.full(((n + 64) * 4,), 0xa5, dtype=torch.uint8, device=dev)
        st_t = torch.from_numpy(np.ascontiguousarray(ref.streams0[idx[:n + 64]]).view(np.uint8).reshape(-1).copy()).to(dev)
        gpu_ctx.query_radiance_cached_device(ref.params, rays_t[:n], st_t[:n * 48], rec_t, dep_t, rgb_t[:n * 12], ends_t[:n * 4], sync=True)
        out, st, en = rgb_t.cpu().numpy(), st_t.cpu().numpy(), ends_t.cpu().numpy()
        assert (out[n * 12:] == 0xa5).all(), f"n={n}: colours written past the batch"
        assert (en[n * 4:] == 0xa5).all(), f"n={n}: counts written past the batch"
        assert st[n * 48:].tobytes() == np.ascontiguousarray(ref.streams0[idx[n:n + 64]]).tobytes(), f"n={n}: streams written past the batch"
        dgot = dict(rgb=out[:n * 12].view(np.float32).reshape(n, 3), ends=en[:n * 4].view(np.uint32))
        CR.assert_equal(dgot, st[:n * 48], ref, f"{name} n={n} device form", idx=sub)


@pytest.mark.parametrize("visible", [False, True])
def test_device_form_on_a_torch_stream(gpu_ctx, visible):
    """on a stream other than the context's; one asynchronous call, then a timed one: equal results, the reference's"""
    import torch
    ref = CR.reference("scene6", 1, 3, "fractional", visible)
    gpu_ctx.upload_world(ref.world)
    dev = torch.device("cuda:0")
    n = len(ref.rays)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rays = torch.from_numpy(ref.rays.copy()).to(dev)
        rec_t, dep_t = _tensors(torch, dev, ref)
        out = [torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(2)]
        ends = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2)]
        st = [torch.from_numpy(ref.streams0.view(np.uint8).reshape(-1).copy()).to(dev) for _ in range(2)]
        assert gpu_ctx.query_radiance_cached_device(ref.params, rays, st[0], rec_t, dep_t, out[0], ends[0]) is None  # enqueued, not waited for
        sec = gpu_ctx.query_radiance_cached_device(ref.params, rays, st[1], rec_t, dep_t, out[1], ends[1], sync=True)
    stream.synchronize()
    assert sec > 0
    a, b = (o.cpu().numpy().reshape(n, 3) for o in out)
    assert a.tobytes() == b.tobytes() and (st[0] == st[1]).all() and (ends[0] == ends[1]).all()
    CR.assert_equal(dict(rgb=a, ends=ends[0].cpu().numpy().view(np.uint32)), st[0].cpu().numpy(), ref, "scene6 on a torch stream")
    # without the counts
    out2 = torch.zeros(n * 3, dtype=torch.float32, device=dev)
    st2 = torch.from_numpy(ref.streams0.view(np.uint8).reshape(-1).copy()).to(dev)
    gpu_ctx.query_radiance_cached_device(ref.params, rays, st2, rec_t, dep_t, out2, None, sync=True)
    assert out2.cpu().numpy().tobytes() == a.tobytes() and (st2 == st[0]).all()


@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("name", CR.WORLDS)
def test_depth_at_the_bounce_limit_is_the_radiance_query(gpu_ctx, name, visible):
    """K = bounce_limit on the device equals ctx.query_radiance on the device, to the bit, streams included"""
    g, rec, depth, vis = CR.volume(name, "ones")
    rays, streams0, _ = R.rays_of(name)
    s = Q.build(name)
    path = hip.radiance_params_from_camera(R.copy_camera(s.cam, None, R.world_light(name)), 2)
    p = CR.params(path, path.bounce_limit, g, vis if visible else None)
    gpu_ctx.upload_world(s.world)
    a_st, b_st = streams0.copy(), streams0.copy()
    a = gpu_ctx.query_radiance_cached(p, rays, a_st, rec, depth if visible else None)
    b = gpu_ctx.query_radiance(path, rays, b_st)
    assert (Q._words(a["rgb"]) == Q._words(b["rgb"])).all() and a_st.tobytes() == b_st.tobytes() and not a["ends"].any()
    assert (a_st.view(np.uint8).reshape(-1, 48) != streams0.view(np.uint8).reshape(-1, 48)).any(1).mean() > 0.25


def test_queries_leave_the_render_alone():
    """two frames with a cached query before and between them equal two frames on a fresh context: image, accumulators, segment
    counts, RNG states and statistics"""
    world, cam = host.build_scene(6, width=96, spp=4)
    W, H = cam.image_width, cam.image_height
    ref = CR.reference("scene6", 1, 1, "fractional", True)
    rays = np.ascontiguousarray(ref.rays[:2000])

    def frames(with_queries):
        out = []
        with hip.Context(0) as ctx:
            ctx.upload_world(world)
            if with_queries:  # before any rng_seed: a cached query needs no pixel RNG
                ctx.query_radiance_cached(ref.params, rays, ref.streams0[:2000].copy(), ref.records, ref.depth)
            ctx.rng_seed(69420, W, H)
            for f in range(2):
                if with_queries and f:
                    ctx.query_radiance_cached(ref.params, rays, ref.streams0[:2000].copy(), ref.records, ref.depth)
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


def test_argument_checks_on_the_device():
    import torch
    ref = CR.reference("scene6", 1, 1, "ones", True)
    L = hip.lib()
    n = 64
    dev = torch.device("cuda:0")
    probes = ref.grid.probes
    sizes = dict(rays=n * 32, streams=n * 48, rgb=n * 12, ends=n * 4, records=probes * 128, depth=probes * 800)

    def params(visible=True, **kw):
        p = CR.params(ref.path, 1, ref.grid, ref.vis if visible else None)
        for k, v in kw.items():
            obj, _, field = k.rpartition("__")
            setattr(getattr(p, obj) if obj else p, field, v)
        return p

    with hip.Context(0) as ctx:
        buf = torch.zeros(sum(sizes.values()) + 64, dtype=torch.uint8, device=dev)
        at, ptr = buf.data_ptr(), {}
        for k, v in sizes.items():
            ptr[k] = at
            at += v

        def call(p, visible=True, count=n, **kw):
            a = dict(ptr)
            a.update(kw)
            return L.mort_hip_query_radiance_cached_device(ctx._h, C.byref(p) if p is not None else None, count, a["rays"], a["streams"], a["records"],
                                                           a["depth"] if visible else None, a["rgb"], a["ends"], None, None)

        assert call(params()) == NO_WORLD
        with pytest.raises(hip.MortHipError) as e:
            ctx.query_radiance_cached(ref.params, ref.rays[:n], ref.streams0[:n].copy(), ref.records, ref.depth)
        assert e.value.status == NO_WORLD
        ctx.upload_world(ref.world)
        torch.cuda.synchronize()
        # an empty batch launches nothing and is fine; NULL buffers, overlapping and misaligned device buffers and bad parameters are not
        assert call(params(), count=0) == 0 and call(params(False), False, count=0) == 0
        assert call(None) == INVALID
        for k in ("rays", "streams", "records", "rgb"):
            assert call(params(), **{k: None}) == INVALID, k
        assert call(params(), False) == INVALID and call(params(False), True) == INVALID, "the maps go with the flag"
        assert call(params(flags=3)) == INVALID and call(params(False, flags=2), False) == INVALID
        assert call(params(cache_depth=-1)) == INVALID and call(params(cache_depth=65)) == INVALID
        assert call(params(), rgb=ptr["rays"] + n * 32 - 16) == INVALID      # colours over the rays' tail
        assert call(params(), ends=ptr["streams"] + 48) == INVALID           # counts over the streams
        assert call(params(), rgb=ptr["records"]) == INVALID                 # colours over the records
        assert call(params(), ends=ptr["depth"] + 800) == INVALID            # counts over the maps
        for k in ("rays", "streams", "records", "depth", "rgb", "ends"):       # not 16-byte aligned
            assert call(params(), **{k: ptr[k] + 4}) == INVALID, k
        for kw, status in ((dict(path__samples=0), INVALID), (dict(path__bounce_limit=-1), CAPACITY), (dict(path__bounce_limit=65), CAPACITY),
                           (dict(path__light_obj_type=S.OBJ_SPHERE, path__light_obj_idx=1 << 20), INVALID), (dict(vis__min_visibility=2.0), INVALID),
                           (dict(vis__normal_bias=-1.0), INVALID)):
            assert call(params(**kw)) == status, kw
        for bad in (0, hip.VOLUME_MAX_COUNT + 1):
            p = params()
            p.grid.count[0] = bad
            assert call(p) == INVALID, bad
        p = params()
        p.grid.spacing[1] = 0.0
        assert call(p) == INVALID
        assert (buf == 0).all(), "a refused call writes nothing"
        # and the checks refuse nothing they should not
        streams = ref.streams0[:n].copy()
        got = ctx.query_radiance_cached(ref.params, ref.rays[:n], streams, ref.records, ref.depth)
        CR.assert_equal(got, streams, ref, "scene6", idx=np.arange(n))
