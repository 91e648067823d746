"""Volume refresh on the MI355X (refresh.hip): probe_refresh_kernel<TREE, VISIBLE, BLOCK> must give the host form's
records (the same body, dev_refresh.h) and those of the reference of tests/refresh_ref.py, tolerance 0 -- records as raw words (any
NaN equals any NaN), all 48 bytes of every stream, the counts -- on scene 6 and a lit flat world with media (the TREE kernels) and on
scene 1 (the item loop over a reference BVH); at every group size; into the head of larger tensors; on torch streams; equal to the
bake where no path can end in the volume; it must leave the render's state alone; and a view takes refreshed records without
forgetting its history."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from mort_amd import hip, host, structs as S
from tests import cached_frame_ref as FR
from tests import cached_ref as CR
from tests import oracle_lib as O
from tests import query_rays as Q
from tests import refresh_ref as RR

pytestmark = pytest.mark.gpu

NO_WORLD, INVALID, CAPACITY = -4, -1, -7
P = 24


def test_the_worlds_run_both_kernels():
    assert [bool(Q.reach(Q.build(n).world)["tree"]) for n in RR.WORLDS] == [True, False, True]


def _device(ctx, ref, dirs="ref", want_ends=True):
    """the host-buffer form on the reference's inputs, the outputs pre-filled; (records, streams, ends)"""
    streams = ref.streams0.copy()
    rec, ends = RR.filled(P)
    ctx.volume_refresh(ref.params, streams, ref.records_in, ref.depth, records_out=rec, ends=ends if want_ends else None,
                       dirs=ref.dirs if dirs == "ref" else dirs, m=ref.m)
    return rec, streams, (ends if want_ends else None)


def _host(ref):
    streams = ref.streams0.copy()
    rec, ends = RR.filled(P)
    hip.volume_refresh_host(ref.world, ref.params, streams, ref.records_in, ref.depth, records_out=rec, ends=ends, dirs=ref.dirs, m=ref.m,
                            tree=Q.reach(ref.world)["tree"], nthreads=16)
    return rec, streams, ends


@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("h", [0.0, 0.75])
@pytest.mark.parametrize("K", [0, 1])
@pytest.mark.parametrize("mask", RR.MASKS)
@pytest.mark.parametrize("name", RR.WORLDS)
def test_device_equals_host_equals_reference(gpu_ctx, name, mask, K, h, samples, visible):
    ref = RR.reference(name, K, h, samples, mask, visible)
    gpu_ctx.upload_world(ref.world)
    rec, streams, ends = _device(gpu_ctx, ref)
    RR.assert_equal(rec, streams, ends, ref, f"{name} {mask} K={K} h={h} samples={samples} visible={visible} device")
    hrec, hst, hends = _host(ref)
    assert (Q._words(hrec) == Q._words(rec)).all() and hst.tobytes() == streams.tobytes() and (hends == ends).all(), "device / host"


@pytest.mark.parametrize("sel", RR.SELECTIONS[1:])
@pytest.mark.parametrize("name", RR.WORLDS)
def test_selections(gpu_ctx, name, sel):
    """a partial refresh: the unselected records and counts keep their fill, the unselected streams all 48 bytes"""
    ref = RR.reference(name, 1, 0.75, 1, "fractional", False, sel=sel)
    gpu_ctx.upload_world(ref.world)
    rec, streams, ends = _device(gpu_ctx, ref)
    RR.assert_equal(rec, streams, ends, ref, f"{name} selection {sel} device")


@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("D", [64, 128, 192, 256, 320, 576])
@pytest.mark.parametrize("name", ["scene6", "scene1"])
def test_every_group_size(gpu_ctx, name, D, visible):
    """every BLOCK instantiation; one batch per wave (64 .. 256), more than one (320: five batches, 576: nine)"""
    ref = RR.reference(name, 0, 0.75, 1, "fractional", visible, D=D)
    gpu_ctx.upload_world(ref.world)
    rec, streams, ends = _device(gpu_ctx, ref)
    RR.assert_equal(rec, streams, ends, ref, f"{name} D={D} visible={visible} device")


def _tensors(torch, dev, ref):
    rec = torch.from_numpy(np.array(ref.records_in)).to(dev)  # copies: the reference's arrays are read-only
    dep = torch.from_numpy(np.array(ref.depth)).to(dev) if ref.depth is not None else None
    return rec, dep


def _bytes(torch, dev, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


@pytest.mark.parametrize("name,visible", [("scene6", True), ("scene1", False)])
def test_device_form_into_larger_tensors(gpu_ctx, name, visible):
    """records, streams and counts go into the heads of larger tensors whose tails keep their fill"""
    import torch
    ref = RR.reference(name, 1, 0.75, 1, "fractional", visible, sel=(1, 5, 5))
    gpu_ctx.upload_world(ref.world)
    dev = torch.device("cuda:0")
    D = ref.params.directions
    rec_in, dep = _tensors(torch, dev, ref)
    tail = 4096
    out = torch.full((P * 128 + tail,), RR.FILL, dtype=torch.uint8, device=dev)
    ends = torch.full((P * 4 + tail,), RR.FILL, dtype=torch.uint8, device=dev)
    st = torch.full((P * D * 48 + tail,), RR.FILL, dtype=torch.uint8, device=dev)
    st[:P * D * 48] = _bytes(torch, dev, ref.streams0)
    dirs = torch.from_numpy(np.array(ref.dirs)).to(dev)
    gpu_ctx.volume_refresh_device(ref.params, st, rec_in, dep, out, ends, dirs=dirs, m=ref.m, sync=True)
    o, e, s = out.cpu().numpy(), ends.cpu().numpy(), st.cpu().numpy()
    assert (o[P * 128:] == RR.FILL).all() and (e[P * 4:] == RR.FILL).all() and (s[P * D * 48:] == RR.FILL).all()
    RR.assert_equal(o[:P * 128].view(np.float32).reshape(P, 32), s[:P * D * 48], e[:P * 4].view(np.uint32), ref, f"{name} device form")


def test_the_contexts_direction_set_follows_d(gpu_ctx):
    """a caller's direction tensor and NULL, with D 64, 128, then 64 again"""
    import torch
    dev = torch.device("cuda:0")
    for D in (64, 128, 64):
        ref = RR.reference("scene6", 0, 0.75, 1, "fractional", False, D=D)
        gpu_ctx.upload_world(ref.world)
        rec_in, _ = _tensors(torch, dev, ref)
        for dirs in (torch.from_numpy(np.array(ref.dirs)).to(dev), None):
            out, ends, st = _bytes(torch, dev, RR.filled(P)[0]), _bytes(torch, dev, RR.filled(P)[1]), _bytes(torch, dev, ref.streams0)
            gpu_ctx.volume_refresh_device(ref.params, st, rec_in, None, out, ends, dirs=dirs, sync=True)
            RR.assert_equal(out.cpu().numpy().view(np.float32).reshape(P, 32), st.cpu().numpy(), ends.cpu().numpy().view(np.uint32), ref,
                            f"D={D} dirs={'own' if dirs is not None else 'NULL'}")


@pytest.mark.parametrize("visible", [False, True])
def test_device_form_on_a_torch_stream(gpu_ctx, visible):
    """on a stream other than the context's; one asynchronous call, then a timed one: equal results, the reference's"""
    import torch
    ref = RR.reference("scene6", 1, 0.75, 3, "fractional", visible)
    gpu_ctx.upload_world(ref.world)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rec_in, dep = _tensors(torch, dev, ref)
        out = [_bytes(torch, dev, RR.filled(P)[0]) for _ in range(2)]
        ends = [_bytes(torch, dev, RR.filled(P)[1]) for _ in range(2)]
        st = [_bytes(torch, dev, ref.streams0) for _ in range(2)]
        assert gpu_ctx.volume_refresh_device(ref.params, st[0], rec_in, dep, out[0], ends[0]) is None  # enqueued, not waited for
        sec = gpu_ctx.volume_refresh_device(ref.params, st[1], rec_in, dep, out[1], ends[1], sync=True)
    stream.synchronize()
    assert sec > 0
    assert (out[0] == out[1]).all() and (st[0] == st[1]).all() and (ends[0] == ends[1]).all()
    RR.assert_equal(out[0].cpu().numpy().view(np.float32).reshape(P, 32), st[0].cpu().numpy(), ends[0].cpu().numpy().view(np.uint32), ref,
                    "scene6 on a torch stream")


@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("name", RR.WORLDS)
def test_bootstrap_is_a_bake(gpu_ctx, name, visible):
    """(a) on the device: h = 0, K >= bounce_limit, records_in = pack(zeros, weight > 0) gives ctx.volume_pack of ctx.probe_bake
    over volume_probes(grid), and the bake's streams"""
    g, _, depth, vis = CR.volume(name, "ones")
    D = 128
    path = RR.path_of(name, 2)
    world = Q.build(name).world
    gpu_ctx.upload_world(world)
    weight = np.random.default_rng(5).uniform(0.1, 2.0, size=P).astype(np.float32)
    zeros = gpu_ctx.volume_pack(np.zeros((P, 27), dtype=np.float32), weight)["records"]
    st_bake = RR.streams_of(P, D)
    sh = gpu_ctx.probe_bake(hip.PROBE_PARAMS(path, D), hip.volume_probes(g), st_bake)["sh"]
    want = gpu_ctx.volume_pack(sh, weight)["records"]
    params = RR.params_of(path, RR.LIMIT, g, vis if visible else None, D, 0.0, (0, 1, P))
    st = RR.streams_of(P, D)
    got = gpu_ctx.volume_refresh(params, st, zeros, depth if visible else None)
    assert (Q._words(got["records"]) == Q._words(want)).all()
    assert st.tobytes() == st_bake.tobytes() and not got["ends"].any()
    assert (st.view(np.uint8).reshape(-1, 48) != RR.streams_of(P, D).view(np.uint8).reshape(-1, 48)).any(1).mean() > 0.05


def test_refreshes_leave_the_render_alone():
    """two frames with a refresh before and between them equal two frames on a fresh context: image, accumulators, segment counts,
    RNG states and statistics"""
    world, cam = host.build_scene(6, width=96, spp=4)
    W, H = cam.image_width, cam.image_height
    ref = RR.reference("scene6", 1, 0.75, 1, "fractional", True)

    def frames(with_refresh):
        out = []
        with hip.Context(0) as ctx:
            ctx.upload_world(world)
            if with_refresh:  # before any rng_seed: a refresh needs no pixel RNG
                _device(ctx, ref)
            ctx.rng_seed(69420, W, H)
            for f in range(2):
                if with_refresh and f:
                    _device(ctx, ref, dirs=None)
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
    ref = RR.reference("scene6", 1, 0.75, 1, "ones", True)
    L = hip.lib()
    D = 64
    dev = torch.device("cuda:0")
    sizes = dict(dirs=D * 12, streams=P * D * 48, records_in=P * 128, depth=P * 800, records_out=P * 128, ends=P * 4)

    def params(visible=True, **kw):
        p = RR.params_of(ref.path, 1, ref.grid, ref.vis if visible else None, D, 0.75, (0, 1, P))
        for k, v in kw.items():
            obj, _, field = k.rpartition("__")
            o = p
            for part in obj.split("__") if obj else ():
                o = getattr(o, part)
            setattr(o, field, v)
        return p

    with hip.Context(0) as ctx:
        buf = torch.zeros(sum(sizes.values()) + 64, dtype=torch.uint8, device=dev)
        at, ptr = buf.data_ptr(), {}
        for k, v in sizes.items():
            ptr[k] = at
            at += v

        def call(p, visible=True, m=P, **kw):
            a = dict(ptr)
            a.update(kw)
            return L.mort_hip_volume_refresh_device(ctx._h, C.byref(p) if p is not None else None, m, a["dirs"], a["streams"], a["records_in"],
                                                    a["depth"] if visible else None, a["records_out"], a["ends"], None, None)

        assert call(params()) == NO_WORLD
        ctx.upload_world(ref.world)
        torch.cuda.synchronize()
        assert call(params(), m=0) == 0 and call(params(False), False, m=0) == 0
        assert call(None) == INVALID
        for k in ("streams", "records_in", "records_out"):
            assert call(params(), **{k: None}) == INVALID, k
        assert call(params(), False) == INVALID and call(params(False), True) == INVALID, "the maps go with the flag"
        for kw in (dict(directions=0), dict(directions=96), dict(directions=4160), dict(cached__path__samples=0), dict(cached__flags=3),
                   dict(cached__cache_depth=-1), dict(cached__cache_depth=65), dict(hysteresis=float("nan")), dict(hysteresis=-0.25),
                   dict(hysteresis=1.0), dict(step=0), dict(first=P), dict(first=1), dict(step=2), dict(first=0xffffffff, step=0xffffffff),
                   dict(cached__vis__min_visibility=2.0), dict(cached__path__light_obj_type=S.OBJ_SPHERE, cached__path__light_obj_idx=1 << 20)):
            assert call(params(**kw)) == INVALID, kw
        assert call(params(cached__path__bounce_limit=-1)) == CAPACITY and call(params(cached__path__bounce_limit=65)) == CAPACITY
        assert call(params(), records_out=ptr["records_in"]) == INVALID, "in place"
        assert call(params(), records_out=ptr["records_in"] + 128 * (P - 1)) == INVALID
        assert call(params(), ends=ptr["streams"] + 48) == INVALID and call(params(), ends=ptr["depth"] + 800) == INVALID
        assert call(params(), records_out=ptr["dirs"]) == INVALID and call(params(), streams=ptr["records_out"]) == INVALID
        for k in sizes:  # not 16-byte aligned
            assert call(params(), **{k: ptr[k] + 4}) == INVALID, k
        assert (buf == 0).all(), "a refused call writes nothing"
        rec, streams, ends = _device(ctx, RR.reference("scene6", 1, 0.75, 1, "ones", True))
        RR.assert_equal(rec, streams, ends, RR.reference("scene6", 1, 0.75, 1, "ones", True), "scene6 after the refusals")


def _cameras(cam0):
    c1 = host.camera_input(S.Camera.from_buffer_copy(cam0), "W")
    c2 = host.camera_input(S.Camera.from_buffer_copy(c1), None, (6, -3))
    c3 = host.camera_input(S.Camera.from_buffer_copy(c2), "D")
    return [cam0, c1, c2, c3]


def test_a_view_takes_refreshed_records_and_keeps_its_history(gpu_ctx):
    """four frames at 48 x 48, 4 spp, temporal accumulation, a cache attached, update_cache with refreshed records before frame 2:
    every frame's output and history equal render_cached_device and the stage calls chained by hand; frame 2 is not the frame a
    set_cache at that point gives (which would forget the history)"""
    import torch
    W = H = 48
    n = W * H
    g, rec0, depth, vis = CR.volume("scene6", "fractional")
    cam0 = FR.camera("scene6", (W, H), 4)
    cams = _cameras(cam0)
    world = Q.build("scene6").world
    fparams = FR.params(1, g, vis)
    streams0 = O.seed_states(FR.SEED, W, H)
    gpu_ctx.upload_world(world)
    dev = torch.device("cuda:0")
    # the refreshed records: one round on the device, h = 0.5, K = 0
    D = 64
    rparams = RR.params_of(RR.path_of("scene6"), 0, g, vis, D, 0.5, (0, 1, P))
    rec_t = [torch.from_numpy(np.array(rec0)).to(dev), torch.zeros(P * 32, dtype=torch.float32, device=dev)]
    dep_t = torch.from_numpy(np.array(depth)).to(dev)
    st_t = _bytes(torch, dev, RR.streams_of(P, D))
    gpu_ctx.volume_refresh_device(rparams, st_t, rec_t[0], dep_t, rec_t[1], None, sync=True)
    assert (rec_t[0].view(-1) != rec_t[1].view(-1)).any()

    def by_hand(reset_at=None):
        gpu_ctx.rng_load(np.ascontiguousarray(streams0), W, H)
        th = hip.TemporalHistory(W, H, backend=gpu_ctx)
        out = []
        for i, cam in enumerate(cams):
            if i == reset_at:
                th.reset()
            rgba = torch.zeros(n * 4, dtype=torch.uint8, device=dev)
            accum = torch.zeros(n * 3, dtype=torch.float32, device=dev)
            gpu_ctx.render_cached_device(cam, fparams, rec_t[0 if i < 2 else 1], dep_t, rgba, accum, None, sync=True)
            acc = accum.cpu().numpy().reshape(H, W, 3)
            f = gpu_ctx.render_features(cam)
            t = th.step(acc, f["normal"], f["depth"], cam)
            out.append(dict(raw_accum=acc, accum=t["accum"].copy(), rgba=t["rgba"].copy(), history=th.history.copy()))
        return out

    want, forgotten = by_hand(), by_hand(reset_at=2)
    assert (want[2]["accum"].view(np.uint32) != forgotten[2]["accum"].view(np.uint32)).any()
    gpu_ctx.rng_load(np.ascontiguousarray(streams0), W, H)
    with gpu_ctx.view(W, H, temporal=1, filter=hip.FILTER_NONE) as v:
        L = hip.lib()
        assert L.mort_hip_view_update_cache(v._h, rec_t[1].data_ptr(), dep_t.data_ptr()) == INVALID, "no cache attached"
        assert L.mort_hip_view_update_cache_host(v._h, rec0.ctypes.data, depth.ctypes.data) == INVALID, "no cache attached"
        v.set_cache(fparams, rec_t[0], dep_t)
        for i, cam in enumerate(cams):
            if i == 2:
                assert L.mort_hip_view_update_cache(v._h, rec_t[1].data_ptr(), None) == INVALID, "the maps go with the attached flag"
                assert L.mort_hip_view_update_cache(v._h, None, dep_t.data_ptr()) == INVALID
                assert L.mort_hip_view_update_cache(v._h, rec_t[1].data_ptr() + 4, dep_t.data_ptr()) == INVALID
                v.update_cache(rec_t[1], dep_t)
            out = v.frame(cam)
            assert out["stats"]["frame"] == i, "the history goes on"
            assert (out["rgba"] == want[i]["rgba"]).all(), f"frame {i}: rgba"
            for k in ("raw_accum", "accum", "history"):
                assert (v.read(k).view(np.uint32) == want[i][k].view(np.uint32)).all(), f"frame {i}: {k}"
            if i == 2:
                assert (v.read("accum").view(np.uint32) != forgotten[2]["accum"].view(np.uint32)).any()
        # the host-array form, from frame 2 on again
        gpu_ctx.rng_load(np.ascontiguousarray(streams0), W, H)
        v.set_cache(fparams, rec_t[0], dep_t)
        for i, cam in enumerate(cams):
            if i == 2:
                v.update_cache(rec_t[1].cpu().numpy(), np.array(depth))
            out = v.frame(cam)
            assert out["stats"]["frame"] == i and (out["rgba"] == want[i]["rgba"]).all(), f"host form, frame {i}"


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORT = os.path.join(ROOT, "mort_amd", "bin", "mort")


@pytest.mark.parametrize("args", [["--refresh", "2,0.5,1", "--irradiance-out"],
                                  ["--visibility", "5", "--cache-depth", "1", "--cache-render", "--refresh", "1,0.75,0,2", "--spp", "4", "--frames", "3", "--out"]])
def test_cli_refresh_on_the_gpu_is_the_host_mode(tmp_path, args):
    """`mort 6 --sh-volume ... --refresh ...` on the GPU writes the bytes `--mode host` writes and reports the same counts: the rounds
    after the bake, and with --cache-render the rounds between the frames of a view"""
    base = [MORT, "6", "--width", "24", "--sh-volume", "100,100,100,455,455,455,3,3,2,64"]
    got = {}
    for mode in ("gpu", "host"):
        out = tmp_path / f"{mode}.ppm"
        p = subprocess.run(base + (["--mode", "host", "--threads", "4"] if mode == "host" else []) + args + [str(out)], cwd=ROOT, capture_output=True,
                           text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        got[mode] = (out.read_bytes(), json.loads(p.stdout.strip().splitlines()[-1]))
    assert got["gpu"][0] == got["host"][0]
    for k in ("refresh_rounds", "hysteresis", "refresh_depth", "refresh_stride", "refresh_ends") + (("ends", "segments") if "--cache-render" in args else ()):
        assert got["gpu"][1][k] == got["host"][1][k], k
    assert got["gpu"][1]["refresh_ends"] > 0 and got["gpu"][1]["mode"] == "mega"
