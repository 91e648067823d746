"""Direct-light cached radiance queries on the MI355X (cached_direct.hip): query_radiance_cached_direct_kernel<TREE,
VISIBLE> must give the host form's answers (the same body, dev_cached_direct.h) and those of the walk over the oracle
(tests/cached_direct_ref.py), tolerance 0 -- colours as raw words (any NaN equals any NaN), final streams as all 48 bytes, both
counts -- on scene 6 and a lit flat world with media (the TREE kernels) and on scene 1 and a list of lights over a reference BVH
(the item loop); at every batch size around a wave and a group; on torch tensors and torch streams; with its identities against the
cached and the plain radiance queries; and the command line must print --mode host's line."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from mort_amd import hip, structs as S
from tests import cached_direct_ref as DR
from tests import cached_ref as CR
from tests import query_rays as Q
from tests import radiance_ref as R
from tests.test_gpu_radiance import _mixed

pytestmark = pytest.mark.gpu

NO_WORLD, INVALID, CAPACITY = -4, -1, -7
SIZES = (1, 63, 64, 65, 257, 1024)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORT = os.path.join(ROOT, "mort_amd", "bin", "mort")


def test_the_worlds_run_both_kernels():
    assert [bool(Q.reach(Q.build(n).world)["tree"]) for n in DR.WORLDS] == [True, False, True, False]
    assert [R.world_light(n) is not None for n in DR.WORLDS] == [True, False, True, True]


@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("depth", DR.DEPTHS)
@pytest.mark.parametrize("mask,samples", DR.CASES)
@pytest.mark.parametrize("name", DR.WORLDS)
def test_device_equals_host_equals_reference(gpu_ctx, name, mask, samples, depth, visible):
    ref = DR.reference(name, depth, samples, mask, visible)
    gpu_ctx.upload_world(ref.world)
    streams = ref.streams0.copy()
    got = gpu_ctx.query_radiance_cached_direct(ref.params, ref.rays, streams, ref.records, ref.depth)
    DR.assert_equal(got, streams, ref, f"{name} {mask} samples={samples} K={depth} visible={visible} device")
    hs = ref.streams0.copy()
    h = hip.query_radiance_cached_direct_host(ref.world, ref.params, ref.rays, hs, ref.records, ref.depth, tree=Q.reach(ref.world)["tree"], nthreads=16)
    assert (Q._words(h["rgb"]) == Q._words(got["rgb"])).all() and hs.tobytes() == streams.tobytes(), "device / host"
    assert (h["ends"] == got["ends"]).all() and (h["lit"] == got["lit"]).all(), "device / host"


def test_rule_a_at_the_last_iteration(gpu_ctx):
    ref = DR.reference("scene6", 2, 1, "ones", False, bounce_limit=3)
    gpu_ctx.upload_world(ref.world)
    streams = ref.streams0.copy()
    got = gpu_ctx.query_radiance_cached_direct(ref.params, ref.rays, streams, ref.records, None)
    DR.assert_equal(got, streams, ref, "scene6 K=2 limit=3 device")
    assert got["ends"].sum() >= 100 and not got["lit"].any()


def test_the_indirect_bake_on_the_device_is_the_hosts(gpu_ctx):
    """the composition over the device bakes: the three sets of coefficients and the final streams equal the host forms', and the
    emission-only bake sees the light"""
    from tests import oracle_lib as O
    s = Q.build("scene6")
    g = CR.grid_of("scene6")
    pp = hip.probe_params_from_camera(s.cam, 64)
    probes = hip.volume_probes(g)
    gpu_ctx.upload_world(s.world)
    d_st, h_st = (O.seed_states(S.DEFAULT_SEED, g.probes * 64, 1) for _ in range(2))
    d = gpu_ctx.probe_bake_indirect(pp, probes, d_st)
    h = hip.probe_bake_indirect_host(s.world, pp, probes, h_st, tree=True, nthreads=16)
    for k in ("sh_full", "sh_emit", "sh_ind"):
        assert (Q._words(d[k].reshape(-1, 3)) == Q._words(h[k].reshape(-1, 3))).all(), k
    assert d_st.tobytes() == h_st.tobytes()
    assert (d["sh_emit"][:, 0, :] > 0).any() and (d["sh_ind"].view(np.uint32) == (d["sh_full"] - d["sh_emit"]).astype(np.float32).view(np.uint32)).all()


def _tensors(torch, dev, ref):
    rec = torch.from_numpy(np.array(ref.records)).to(dev)  # copies: the reference's arrays are read-only
    dep = torch.from_numpy(np.array(ref.depth)).to(dev) if ref.depth is not None else None
    return rec, dep


@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("name", ["scene6", DR.BVH_LIGHT_WORLD])
def test_partial_waves_and_groups(gpu_ctx, name, visible):
    """n around a wave (64) and a group (256), far, axis and ordinary rays in every wave, under the slab mask (paths that end in
    the volume with and without a lit shadow segment and Lambertian hits that fall through side by side): the rays past n are not
    there, the bytes past n of the colours, the streams and both counts are not written"""
    import torch
    ref = DR.reference(name, 0, 3, "slab", visible)
    idx = _mixed(ref)
    assert len(idx) >= max(SIZES) + 64
    gpu_ctx.upload_world(ref.world)
    dev = torch.device("cuda:0")
    rays_t = torch.from_numpy(np.ascontiguousarray(ref.rays[idx[:max(SIZES) + 64]])).to(dev)
    rec_t, dep_t = _tensors(torch, dev, ref)
    for n in SIZES:
        sub = idx[:n]
        streams = np.ascontiguousarray(ref.streams0[sub])
        got = gpu_ctx.query_radiance_cached_direct(ref.params, np.ascontiguousarray(ref.rays[sub]), streams, ref.records, ref.depth)
        DR.assert_equal(got, streams, ref, f"{name} n={n}", idx=sub)
        # the _device form into the heads of larger tensors: the tails keep their fill
        rgb_t = torch.full(((n + 64) * 12,), 0xa5, dtype=torch.uint8, device=dev)
        ends_t = torch.full(((n + 64) * 4,), 0xa5, dtype=torch.uint8, device=dev)
        lit_t = torch.full(((n + 64) * 4,), 0xa5, dtype=torch.uint8, device=dev)
        st_t = torch.from_numpy(np.ascontiguousarray(ref.streams0[idx[:n + 64]]).view(np.uint8).reshape(-1).copy()).to(dev)
        gpu_ctx.query_radiance_cached_direct_device(ref.params, rays_t[:n], st_t[:n * 48], rec_t, dep_t, rgb_t[:n * 12], ends_t[:n * 4], lit_t[:n * 4],
                                                    sync=True)
        out, st, en, li = rgb_t.cpu().numpy(), st_t.cpu().numpy(), ends_t.cpu().numpy(), lit_t.cpu().numpy()
        assert (out[n * 12:] == 0xa5).all(), f"n={n}: colours written past the batch"
        assert (en[n * 4:] == 0xa5).all() and (li[n * 4:] == 0xa5).all(), f"n={n}: counts written past the batch"
        assert st[n * 48:].tobytes() == np.ascontiguousarray(ref.streams0[idx[n:n + 64]]).tobytes(), f"n={n}: streams written past the batch"
        dgot = dict(rgb=out[:n * 12].view(np.float32).reshape(n, 3), ends=en[:n * 4].view(np.uint32), lit=li[:n * 4].view(np.uint32))
        DR.assert_equal(dgot, st[:n * 48], ref, f"{name} n={n} device form", idx=sub)


@pytest.mark.parametrize("visible", [False, True])
def test_device_form_on_a_torch_stream(gpu_ctx, visible):
    """on a stream other than the context's; one asynchronous call, then a timed one: equal results, the reference's"""
    import torch
    ref = DR.reference("scene6", 1, 3, "fractional", visible)
    gpu_ctx.upload_world(ref.world)
    dev = torch.device("cuda:0")
    n = len(ref.rays)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rays = torch.from_numpy(ref.rays.copy()).to(dev)
        rec_t, dep_t = _tensors(torch, dev, ref)
        out = [torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(2)]
        ends = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2)]
        lit = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2)]
        st = [torch.from_numpy(ref.streams0.view(np.uint8).reshape(-1).copy()).to(dev) for _ in range(2)]
        assert gpu_ctx.query_radiance_cached_direct_device(ref.params, rays, st[0], rec_t, dep_t, out[0], ends[0], lit[0]) is None  # enqueued, not waited for
        sec = gpu_ctx.query_radiance_cached_direct_device(ref.params, rays, st[1], rec_t, dep_t, out[1], ends[1], lit[1], sync=True)
    stream.synchronize()
    assert sec > 0
    a, b = (o.cpu().numpy().reshape(n, 3) for o in out)
    assert a.tobytes() == b.tobytes() and (st[0] == st[1]).all() and (ends[0] == ends[1]).all() and (lit[0] == lit[1]).all()
    DR.assert_equal(dict(rgb=a, ends=ends[0].cpu().numpy().view(np.uint32), lit=lit[0].cpu().numpy().view(np.uint32)), st[0].cpu().numpy(), ref,
                    "scene6 on a torch stream")
    # without the counts
    out2 = torch.zeros(n * 3, dtype=torch.float32, device=dev)
    st2 = torch.from_numpy(ref.streams0.view(np.uint8).reshape(-1).copy()).to(dev)
    gpu_ctx.query_radiance_cached_direct_device(ref.params, rays, st2, rec_t, dep_t, out2, None, None, sync=True)
    assert out2.cpu().numpy().tobytes() == a.tobytes() and (st2 == st[0]).all()


@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("name", DR.WORLDS)
def test_without_a_light_object_it_is_the_cached_query(gpu_ctx, name, visible):
    """(i) on the device against ctx.query_radiance_cached on the device, to the bit, streams and ends included"""
    ref = DR.reference(name, 0, 3, "fractional", visible)
    p = hip.CACHED_PARAMS.from_buffer_copy(ref.params)
    p.path.light_obj_type, p.path.light_obj_idx = -1, 0
    gpu_ctx.upload_world(ref.world)
    a_st, b_st = ref.streams0.copy(), ref.streams0.copy()
    a = gpu_ctx.query_radiance_cached_direct(p, ref.rays, a_st, ref.records, ref.depth)
    b = gpu_ctx.query_radiance_cached(p, ref.rays, b_st, ref.records, ref.depth)
    assert (Q._words(a["rgb"]) == Q._words(b["rgb"])).all() and a_st.tobytes() == b_st.tobytes() and (a["ends"] == b["ends"]).all()
    assert a["ends"].sum() > 100 and not a["lit"].any()


@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("name", DR.WORLDS)
def test_depth_at_the_bounce_limit_and_an_empty_volume_are_the_radiance_query(gpu_ctx, name, visible):
    """(ii) on the device against ctx.query_radiance on the device, to the bit, streams included"""
    g, rec, depth, vis = CR.volume(name, "ones")
    zeros = CR.volume(name, "zeros")[1]
    rays, streams0, _ = R.rays_of(name)
    s = Q.build(name)
    path = hip.radiance_params_from_camera(R.copy_camera(s.cam, None, R.world_light(name)), 2)
    gpu_ctx.upload_world(s.world)
    b_st = streams0.copy()
    b = gpu_ctx.query_radiance(path, rays, b_st)
    for what, k, records in (("K = bounce_limit", path.bounce_limit, rec), ("every weight 0", 0, zeros)):
        a_st = streams0.copy()
        a = gpu_ctx.query_radiance_cached_direct(CR.params(path, k, g, vis if visible else None), rays, a_st, records, depth if visible else None)
        assert (Q._words(a["rgb"]) == Q._words(b["rgb"])).all() and a_st.tobytes() == b_st.tobytes(), what
        assert not a["ends"].any() and not a["lit"].any(), what
    assert (b_st.view(np.uint8).reshape(-1, 48) != streams0.view(np.uint8).reshape(-1, 48)).any(1).mean() > 0.25


def test_argument_checks_on_the_device():
    import torch
    ref = DR.reference("scene6", 1, 1, "ones", True)
    L = hip.lib()
    n = 64
    dev = torch.device("cuda:0")
    probes = ref.grid.probes
    sizes = dict(rays=n * 32, streams=n * 48, rgb=n * 12, ends=n * 4, lit=n * 4, records=probes * 128, depth=probes * 800)

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
            return L.mort_hip_query_radiance_cached_direct_device(ctx._h, C.byref(p) if p is not None else None, count, a["rays"], a["streams"],
                                                                  a["records"], a["depth"] if visible else None, a["rgb"], a["ends"], a["lit"], None,
                                                                  None)

        assert call(params()) == NO_WORLD
        with pytest.raises(hip.MortHipError) as e:
            ctx.query_radiance_cached_direct(ref.params, ref.rays[:n], ref.streams0[:n].copy(), ref.records, ref.depth)
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
        assert call(params(), lit=ptr["streams"] + 48) == INVALID            # lit counts over the streams
        assert call(params(), lit=ptr["ends"]) == INVALID                    # lit counts over the counts
        assert call(params(), lit=ptr["rgb"] + 16) == INVALID                # lit counts over the colours
        assert call(params(), rgb=ptr["records"]) == INVALID                 # colours over the records
        assert call(params(), ends=ptr["depth"] + 800) == INVALID            # counts over the maps
        assert call(params(), lit=ptr["depth"] + 800) == INVALID             # lit counts over the maps
        for k in ("rays", "streams", "records", "depth", "rgb", "ends", "lit"):  # not 16-byte aligned
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
        got = ctx.query_radiance_cached_direct(ref.params, ref.rays[:n], streams, ref.records, ref.depth)
        DR.assert_equal(got, streams, ref, "scene6", idx=np.arange(n))


def test_the_command_line_prints_the_host_modes_line():
    """`mort 6 ... --cache-direct --probe` on the GPU against --mode host: every field but the mode and the times"""
    args = ["6", "--width", "24", "--sh-volume", "100,100,100,455,455,455,3,3,2,64", "--visibility", "5", "--cache-depth", "0", "--cache-direct",
            "--probe", "12,4,8"]
    lines = []
    for mode in (["--mode", "host"], []):
        p = subprocess.run([MORT] + args + mode, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        j = json.loads(p.stdout.strip())
        lines.append({k: v for k, v in j.items() if k not in ("mode", "seconds", "bake_seconds")})
    assert lines[0] == lines[1] and lines[0]["cache_direct"] == 1 and lines[0]["lit"] >= 1 and lines[0]["ends"] == 8
    assert [json.dumps(v) for v in lines[0].values()] == [json.dumps(v) for v in lines[1].values()]
