"""Direct-light volume refresh on the MI355X (refresh_direct.hip): probe_refresh_direct_kernel<TREE, VISIBLE, BLOCK>
must give the host form's records (the same body, dev_refresh_direct.h) and those of the reference of tests/refresh_direct_ref.py,
tolerance 0 -- records as raw words (any NaN equals any NaN), all 48 bytes of every stream, both counts -- on scene 6 and the lit
flat world with media (the TREE kernels), on the BVH light world and scene 1 (the scan kernels); at every group size; for every
selection; into the heads of larger tensors; on a torch stream; without the counts; identities (A) and (B) against the device's own
plain refresh and direct query; the status codes; a view with a direct cache that takes direct-refreshed records and keeps its
history; and the command line on the GPU against --mode host."""
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
from tests import probe_ref as PR
from tests import query_rays as Q
from tests import refresh_direct_ref as XR
from tests import refresh_ref as RR

pytestmark = pytest.mark.gpu

NO_WORLD, INVALID, CAPACITY = -4, -1, -7


def test_the_worlds_run_both_kernels():
    assert [bool(Q.reach(Q.build(n).world)["tree"]) for n in XR.WORLDS] == [True, True, False, False]


def _device(ctx, ref, dirs="ref", want_ends=True, want_lit=True):
    """the host-buffer form on the reference's inputs, the outputs pre-filled; (records, streams, ends, lit)"""
    streams = ref.streams0.copy()
    rec, ends, lit = XR.filled(ref.grid.probes)
    ctx.volume_refresh_direct(ref.params, streams, ref.records_in, ref.depth, records_out=rec, ends=ends if want_ends else None,
                              lit=lit if want_lit else None, dirs=ref.dirs if dirs == "ref" else dirs, m=ref.m)
    return rec, streams, (ends if want_ends else None), (lit if want_lit else None)


def _host(ref):
    streams = ref.streams0.copy()
    rec, ends, lit = XR.filled(ref.grid.probes)
    hip.volume_refresh_direct_host(ref.world, ref.params, streams, ref.records_in, ref.depth, records_out=rec, ends=ends, lit=lit, dirs=ref.dirs,
                                   m=ref.m, tree=Q.reach(ref.world)["tree"], nthreads=16)
    return rec, streams, ends, lit


@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("h", [0.0, 0.75])
@pytest.mark.parametrize("K", [0, 1])
@pytest.mark.parametrize("mask", XR.MASKS)
@pytest.mark.parametrize("name", XR.WORLDS)
def test_device_equals_host_equals_reference(gpu_ctx, name, mask, K, h, samples, visible):
    ref = XR.reference(name, K, h, samples, mask, visible)
    gpu_ctx.upload_world(ref.world)
    rec, streams, ends, lit = _device(gpu_ctx, ref)
    XR.assert_equal(rec, streams, ends, lit, ref, f"{name} {mask} K={K} h={h} samples={samples} visible={visible} device")
    hrec, hst, hends, hlit = _host(ref)
    assert (Q._words(hrec) == Q._words(rec)).all() and hst.tobytes() == streams.tobytes() and (hends == ends).all() and (hlit == lit).all()


@pytest.mark.parametrize("which", [1, 2, 3])
@pytest.mark.parametrize("name", XR.WORLDS)
def test_selections(gpu_ctx, name, which):
    """a partial refresh: the unselected records and counts keep their fill, the unselected streams all 48 bytes"""
    sel = XR.selections(XR.grid_of(name).probes)[which]
    ref = XR.reference(name, 1, 0.75, 1, "fractional", False, sel=sel)
    gpu_ctx.upload_world(ref.world)
    rec, streams, ends, lit = _device(gpu_ctx, ref)
    XR.assert_equal(rec, streams, ends, lit, ref, f"{name} selection {sel} device")


@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("D", [64, 128, 192, 256, 320])
@pytest.mark.parametrize("name", ["scene6", XR.BVH_LIGHT_WORLD])
def test_every_group_size(gpu_ctx, name, D, visible):
    """every BLOCK instantiation of the tree and of the scan kernels; at 320 a wave takes two batches"""
    ref = XR.reference(name, 0, 0.75, 1, "fractional", visible, D=D)
    gpu_ctx.upload_world(ref.world)
    rec, streams, ends, lit = _device(gpu_ctx, ref)
    XR.assert_equal(rec, streams, ends, lit, ref, f"{name} D={D} visible={visible} device")
    assert lit.sum() > 0


def test_without_the_counts(gpu_ctx):
    ref = XR.reference("scene6", 1, 0.75, 3, "fractional", True)
    gpu_ctx.upload_world(ref.world)
    for want_ends, want_lit in ((True, False), (False, True), (False, False)):
        rec, streams, ends, lit = _device(gpu_ctx, ref, want_ends=want_ends, want_lit=want_lit)
        XR.assert_equal(rec, streams, ends, lit, ref, f"ends={want_ends} lit={want_lit} device")


def _tensors(torch, dev, ref):
    rec = torch.from_numpy(np.array(ref.records_in)).to(dev)  # copies: the reference's arrays are read-only
    dep = torch.from_numpy(np.array(ref.depth)).to(dev) if ref.depth is not None else None
    return rec, dep


def _bytes(torch, dev, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


@pytest.mark.parametrize("name,visible", [("scene6", True), (XR.BVH_LIGHT_WORLD, False)])
def test_device_form_into_larger_tensors(gpu_ctx, name, visible):
    """records, streams and both counts go into the heads of larger tensors whose tails keep their fill"""
    import torch
    P = XR.grid_of(name).probes
    ref = XR.reference(name, 1, 0.75, 1, "fractional", visible, sel=(1, 5, 3))
    gpu_ctx.upload_world(ref.world)
    dev = torch.device("cuda:0")
    D = ref.params.directions
    rec_in, dep = _tensors(torch, dev, ref)
    tail = 4096
    out = torch.full((P * 128 + tail,), XR.FILL, dtype=torch.uint8, device=dev)
    ends = torch.full((P * 4 + tail,), XR.FILL, dtype=torch.uint8, device=dev)
    lit = torch.full((P * 4 + tail,), XR.FILL, dtype=torch.uint8, device=dev)
    st = torch.full((P * D * 48 + tail,), XR.FILL, dtype=torch.uint8, device=dev)
    st[:P * D * 48] = _bytes(torch, dev, ref.streams0)
    dirs = torch.from_numpy(np.array(ref.dirs)).to(dev)
    gpu_ctx.volume_refresh_direct_device(ref.params, st, rec_in, dep, out, ends, lit, dirs=dirs, m=ref.m, sync=True)
    o, e, l, s = out.cpu().numpy(), ends.cpu().numpy(), lit.cpu().numpy(), st.cpu().numpy()
    assert (o[P * 128:] == XR.FILL).all() and (e[P * 4:] == XR.FILL).all() and (l[P * 4:] == XR.FILL).all() and (s[P * D * 48:] == XR.FILL).all()
    XR.assert_equal(o[:P * 128].view(np.float32).reshape(P, 32), s[:P * D * 48], e[:P * 4].view(np.uint32), l[:P * 4].view(np.uint32), ref,
                    f"{name} device form")


@pytest.mark.parametrize("visible", [False, True])
def test_device_form_on_a_torch_stream(gpu_ctx, visible):
    """on a stream other than the context's; one asynchronous call with NULL directions, then a timed one: equal results"""
    import torch
    ref = XR.reference("flat:lit_by_quad_with_media", 1, 0.75, 3, "fractional", visible)
    P = ref.grid.probes
    gpu_ctx.upload_world(ref.world)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rec_in, dep = _tensors(torch, dev, ref)
        out = [_bytes(torch, dev, XR.filled(P)[0]) for _ in range(2)]
        ends = [_bytes(torch, dev, XR.filled(P)[1]) for _ in range(2)]
        lit = [_bytes(torch, dev, XR.filled(P)[2]) for _ in range(2)]
        st = [_bytes(torch, dev, ref.streams0) for _ in range(2)]
        assert gpu_ctx.volume_refresh_direct_device(ref.params, st[0], rec_in, dep, out[0], ends[0], lit[0]) is None  # enqueued, not waited for
        sec = gpu_ctx.volume_refresh_direct_device(ref.params, st[1], rec_in, dep, out[1], ends[1], lit[1], sync=True)
    stream.synchronize()
    assert sec > 0
    assert (out[0] == out[1]).all() and (st[0] == st[1]).all() and (ends[0] == ends[1]).all() and (lit[0] == lit[1]).all()
    XR.assert_equal(out[0].cpu().numpy().view(np.float32).reshape(P, 32), st[0].cpu().numpy(), ends[0].cpu().numpy().view(np.uint32),
                    lit[0].cpu().numpy().view(np.uint32), ref, "on a torch stream")


@pytest.mark.parametrize("visible", [False, True])
def test_a_world_without_emitters_is_the_plain_refresh(gpu_ctx, visible):
    """(A) on the device: scene 1 against the device's own plain refresh"""
    ref = XR.reference("scene1", 1, 0.75, 3, "fractional", visible)
    gpu_ctx.upload_world(ref.world)
    rec, streams, ends, lit = _device(gpu_ctx, ref)
    st = ref.streams0.copy()
    prec, pends = RR.filled(ref.grid.probes)
    gpu_ctx.volume_refresh(ref.params, st, ref.records_in, ref.depth, records_out=prec, ends=pends, dirs=ref.dirs)
    assert (Q._words(rec) == Q._words(prec)).all() and streams.tobytes() == st.tobytes() and (ends == pends).all()
    assert ends.sum() > 100 and not lit.any()


@pytest.mark.parametrize("name", ["scene6", XR.BVH_LIGHT_WORLD])
def test_composed_from_the_devices_own_queries(gpu_ctx, name):
    """(B) on the device: the mask from ctx.query_radiance at bounce limit 1 and a black background, the values from
    ctx.query_radiance_cached_direct at one sample on the carried streams"""
    samples, D = 3, 64
    ref = XR.reference(name, 0, 0.75, samples, "fractional", True)
    gpu_ctx.upload_world(ref.world)
    live = ref.census["active"]
    rays = PR.rays_of(RR.positions(ref.grid)[live], ref.dirs)
    idx = (live[:, None] * D + np.arange(D)[None, :]).reshape(-1)
    st = np.ascontiguousarray(ref.streams0[idx]).copy()
    one = hip.CACHED_PARAMS.from_buffer_copy(ref.params.cached)
    one.path.samples = 1
    black = hip.RADIANCE_PARAMS.from_buffer_copy(ref.path)
    black.bounce_limit, black.samples = 1, 1
    for k in range(3):
        black.background[k] = 0.0
    total = np.zeros((len(rays), 3), dtype=np.float32)
    ends = np.zeros(len(rays), dtype=np.uint32)
    lit = np.zeros(len(rays), dtype=np.uint32)
    for _ in range(samples):
        emits = (gpu_ctx.query_radiance(black, rays, st.copy())["rgb"] != 0).any(1)
        got = gpu_ctx.query_radiance_cached_direct(one, rays, st, ref.records_in, ref.depth)
        with np.errstate(invalid="ignore", over="ignore"):
            total = (total + np.where(emits[:, None], np.float32(0), got["rgb"])).astype(np.float32)
        ends += got["ends"]; lit += got["lit"]
    new = PR.project(total.reshape(len(live), D, 3), ref.dirs, samples).reshape(len(live), 27)
    want = RR.blend(ref.records_in[live, :27], new, 0.75)
    rec, streams, got_ends, got_lit = _device(gpu_ctx, ref)
    assert (Q._words(rec[live, :27]) == Q._words(want)).all()
    assert np.ascontiguousarray(streams[idx]).tobytes() == st.tobytes()
    assert (got_ends[live] == ends.reshape(len(live), D).sum(1)).all() and (got_lit[live] == lit.reshape(len(live), D).sum(1)).all()


def test_argument_checks_on_the_device():
    import torch
    ref = XR.reference("scene6", 1, 0.75, 1, "ones", True)
    P = ref.grid.probes
    L = hip.lib()
    D = 64
    dev = torch.device("cuda:0")
    sizes = dict(dirs=D * 12, streams=P * D * 48, records_in=P * 128, depth=P * 800, records_out=P * 128, ends=P * 4, lit=P * 4)

    def params(visible=True, **kw):
        p = XR.params_of(ref.path, 1, ref.grid, ref.vis if visible else None, D, 0.75, (0, 1, P))
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
            assert v % 16 == 0
            ptr[k] = at
            at += v

        def call(p, visible=True, m=P, **kw):
            a = dict(ptr)
            a.update(kw)
            return L.mort_hip_volume_refresh_direct_device(ctx._h, C.byref(p) if p is not None else None, m, a["dirs"], a["streams"], a["records_in"],
                                                           a["depth"] if visible else None, a["records_out"], a["ends"], a["lit"], None, None)

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
        assert call(params(), lit=ptr["ends"]) == INVALID and call(params(), lit=ptr["streams"] + 48) == INVALID
        assert call(params(), lit=ptr["records_out"] + 128 * (P - 1)) == INVALID and call(params(), lit=ptr["depth"] + 800) == INVALID
        assert call(params(), ends=ptr["lit"]) == INVALID and call(params(), records_out=ptr["dirs"]) == INVALID
        for k in sizes:  # not 16-byte aligned
            assert call(params(), **{k: ptr[k] + 4}) == INVALID, k
        assert (buf == 0).all(), "a refused call writes nothing"
        rec, streams, ends, lit = _device(ctx, ref)
        XR.assert_equal(rec, streams, ends, lit, ref, "scene6 after the refusals")


def _cameras(cam0):
    c1 = host.camera_input(S.Camera.from_buffer_copy(cam0), "W")
    c2 = host.camera_input(S.Camera.from_buffer_copy(c1), None, (6, -3))
    c3 = host.camera_input(S.Camera.from_buffer_copy(c2), "D")
    return [cam0, c1, c2, c3]


def test_a_direct_view_takes_direct_refreshed_records_and_keeps_its_history(gpu_ctx):
    """four frames at 48 x 48, 4 spp, temporal accumulation, a direct cache attached, update_cache with direct-refreshed records
    before frame 2: every frame's output, counts and history equal render_cached_direct_device and the stage calls chained by hand;
    frame 2 is not the frame that a history reset at that point gives.  No view code knows of the direct refresh."""
    import torch
    W = H = 48
    n = W * H
    g, rec0, depth, vis = CR.volume("scene6", "fractional")  # the grid over the whole scene: the frames' paths end all over it
    P = g.probes
    cams = _cameras(FR.camera("scene6", (W, H), 4))
    world = Q.build("scene6").world
    fparams = FR.params(1, g, vis)
    streams0 = O.seed_states(FR.SEED, W, H)
    gpu_ctx.upload_world(world)
    dev = torch.device("cuda:0")
    D = 64
    rparams = XR.params_of(XR.path_of("scene6"), 0, g, vis, D, 0.5, (0, 1, P))
    rec_t = [torch.from_numpy(np.array(rec0)).to(dev), torch.zeros(P * 32, dtype=torch.float32, device=dev)]
    dep_t = torch.from_numpy(np.array(depth)).to(dev)
    st_t = _bytes(torch, dev, XR.streams_of(P, D))
    lit_t = torch.zeros(P, dtype=torch.int32, device=dev)
    gpu_ctx.volume_refresh_direct_device(rparams, st_t, rec_t[0], dep_t, rec_t[1], None, lit_t, sync=True)
    assert (rec_t[0].view(-1) != rec_t[1].view(-1)).any() and int(lit_t.sum()) > 0

    def by_hand(reset_at=None):
        gpu_ctx.rng_load(np.ascontiguousarray(streams0), W, H)
        th = hip.TemporalHistory(W, H, backend=gpu_ctx)
        out = []
        for i, cam in enumerate(cams):
            if i == reset_at:
                th.reset()
            rgba = torch.zeros(n * 4, dtype=torch.uint8, device=dev)
            accum = torch.zeros(n * 3, dtype=torch.float32, device=dev)
            ends = torch.zeros(n, dtype=torch.int32, device=dev)
            lit = torch.zeros(n, dtype=torch.int32, device=dev)
            gpu_ctx.render_cached_direct_device(cam, fparams, rec_t[0 if i < 2 else 1], dep_t, rgba, accum, ends, lit, sync=True)
            acc = accum.cpu().numpy().reshape(H, W, 3)
            f = gpu_ctx.render_features(cam)
            t = th.step(acc, f["normal"], f["depth"], cam)
            out.append(dict(raw_accum=acc, accum=t["accum"].copy(), rgba=t["rgba"].copy(), history=th.history.copy(),
                            ends=ends.cpu().numpy().astype(np.uint32).reshape(H, W), lit=lit.cpu().numpy().astype(np.uint32).reshape(H, W)))
        return out

    want, forgotten = by_hand(), by_hand(reset_at=2)
    assert (want[2]["accum"].view(np.uint32) != forgotten[2]["accum"].view(np.uint32)).any()
    gpu_ctx.rng_load(np.ascontiguousarray(streams0), W, H)
    with gpu_ctx.view(W, H, temporal=1, filter=hip.FILTER_NONE) as v:
        v.set_cache(fparams, rec_t[0], dep_t, direct=True)
        for i, cam in enumerate(cams):
            if i == 2:
                v.update_cache(rec_t[1], dep_t)
            out = v.frame(cam)
            assert out["stats"]["frame"] == i, "the history goes on"
            assert (out["rgba"] == want[i]["rgba"]).all(), f"frame {i}: rgba"
            for k in ("raw_accum", "accum", "history"):
                assert (v.read(k).view(np.uint32) == want[i][k].view(np.uint32)).all(), f"frame {i}: {k}"
            assert (v.read("ends").reshape(H, W) == want[i]["ends"]).all() and (v.read("lit").reshape(H, W) == want[i]["lit"]).all(), f"frame {i}: counts"
            if i == 2:
                assert (v.read("accum").view(np.uint32) != forgotten[2]["accum"].view(np.uint32)).any()
        assert want[3]["lit"].sum() > 0


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORT = os.path.join(ROOT, "mort_amd", "bin", "mort")


@pytest.mark.parametrize("args", [["--cache-depth", "0", "--cache-direct", "--refresh-direct", "2,0.5,0", "--radiance-out"],
                                  ["--visibility", "5", "--cache-depth", "1", "--cache-render-direct", "--refresh-direct", "1,0.75,0,2", "--spp", "4",
                                   "--frames", "3", "--out"]])
def test_cli_refresh_direct_on_the_gpu_is_the_host_mode(tmp_path, args):
    """`mort 6 --sh-volume ... --refresh-direct ...` on the GPU writes the bytes `--mode host` writes and reports the same counts: the
    rounds after the bakes, and with --cache-render-direct the rounds between the frames of a view"""
    base = [MORT, "6", "--width", "24", "--sh-volume", "100,100,100,455,455,455,3,3,2,64"]
    got = {}
    for mode in ("gpu", "host"):
        out = tmp_path / f"{mode}.ppm"
        p = subprocess.run(base + (["--mode", "host", "--threads", "4"] if mode == "host" else []) + args + [str(out)], cwd=ROOT, capture_output=True,
                           text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        got[mode] = (out.read_bytes(), json.loads(p.stdout.strip().splitlines()[-1]))
    assert got["gpu"][0] == got["host"][0]
    keys = ("refresh_rounds", "hysteresis", "refresh_depth", "refresh_stride", "refresh_ends", "refresh_direct", "refresh_lit", "ends", "lit")
    for k in keys + (("segments",) if "--cache-render-direct" in args else ()):
        assert got["gpu"][1][k] == got["host"][1][k], k
    assert got["gpu"][1]["refresh_ends"] > 0 and got["gpu"][1]["refresh_lit"] > 0 and got["gpu"][1]["mode"] == "mega"
