"""Cached frames on the MI355X (cached_frame.hip): cached_frame_kernel<TREE, VISIBLE> must give the host form's
frames (the same body, dev_cached_frame.h) and those of the walk over the oracle (tests/cached_frame_ref.py), tolerance 0 -- uchar4,
accumulators as raw words, per-pixel segments, counts, all 48 bytes of every final stream, the statistics' totals -- on scene 6 and
a lit flat world with media (the TREE kernels) and on scene 1 (the item loop over a reference BVH); at frame sizes around a wave
and a group; on torch tensors and torch streams; equal to the plain render where no path can end in the volume; inside a view; and
between plain renders, whose streams it continues."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from mort_amd import hip, host, structs as S
from tests import cached_frame_ref as FR
from tests import oracle_lib as O
from tests import query_rays as Q

pytestmark = pytest.mark.gpu

NO_RNG, NO_WORLD, INVALID, UNSUPPORTED, CAPACITY = -5, -4, -1, -6, -7
FILL = 0xa5


def _load(ctx, ref, states=None):
    W, H = ref.cam.image_width, ref.cam.image_height
    ctx.rng_load(np.ascontiguousarray(ref.streams0 if states is None else states), W, H)
    return W, H


def _device_frame(ctx, ref, states=None, **kw):
    W, H = _load(ctx, ref, states)
    got = ctx.render_cached(ref.cam, ref.params, ref.records, ref.depth, want_segments=True, **kw)
    return got, ctx.rng_store(W, H, O.STATE_DTYPE)


def _kernel(ref):
    return f"cached_frame_kernel<{'true' if Q.reach(ref.world)['tree'] else 'false'}, {'true' if ref.depth is not None else 'false'}>"


def test_the_worlds_run_both_kernels():
    assert [bool(Q.reach(Q.build(n).world)["tree"]) for n in FR.WORLDS] == [True, False, True]


@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("depth,mask,lens", [(0, "fractional", False), (1, "slab", False), (2, "fractional", True), (1, "poison", False), (1, "holes", True)])
@pytest.mark.parametrize("name", FR.WORLDS)
def test_device_equals_host_equals_reference(gpu_ctx, name, depth, mask, lens, visible):
    aside = mask == "slab" and FR.slab_aside(name)
    ref = FR.reference(name, depth, (40, 33) if aside else FR.SIZE, mask=mask, visible=visible, lens=lens, aside=aside)
    want = ref.frames[0]
    gpu_ctx.upload_world(ref.world)
    got, states = _device_frame(gpu_ctx, ref)
    what = f"{name} {mask} K={depth} visible={visible} lens={lens}"
    FR.assert_equal(got, states, want, what + " device")
    st = got["stats"]
    npx = want["ends_px"].size
    assert st["segments"] == want["segments"] and st["pixels"] == npx and st["eff_samples"] == 4 * npx and st["seconds"] > 0
    assert st["kernel_name"] == _kernel(ref) and st["scene_in_lds"] == 0 and st["reference_walks"] == 0 and st["kernel_vgprs"] > 0
    assert st["algorithmic_hbm_bytes"] == npx * (100 + 12 + 4)
    h = hip.render_cached_host(ref.world, ref.cam, ref.params, ref.records, ref.depth, states=ref.streams0, tree=Q.reach(ref.world)["tree"], nthreads=16)
    FR.assert_equal(h, h["states"], want, what + " host")
    assert h["stats"]["rng_draws"] == st["rng_draws"], "device / host draws"


def _tensors(torch, dev, ref):
    rec = torch.from_numpy(np.array(ref.records)).to(dev)  # copies: the reference's arrays are read-only
    dep = torch.from_numpy(np.array(ref.depth)).to(dev) if ref.depth is not None else None
    return rec, dep


@pytest.mark.parametrize("size", FR.SIZES)
@pytest.mark.parametrize("name,visible", [("scene6", True), ("scene1", False)])
def test_frame_sizes_round_a_wave_and_a_group(gpu_ctx, name, visible, size):
    """1, 63, 64, 65, 255, 256, 257 and 1320 pixels at K = 1, 4 spp, under the slab mask (paths that end in the volume and hits
    that fall through side by side); the _device form writes into the heads of larger tensors, whose tails keep their fill"""
    import torch
    ref = FR.reference(name, 1, size, mask="slab", visible=visible)
    want = ref.frames[0]
    gpu_ctx.upload_world(ref.world)
    got, states = _device_frame(gpu_ctx, ref)
    FR.assert_equal(got, states, want, f"{name} {size}")
    dev = torch.device("cuda:0")
    n = size[0] * size[1]
    rec_t, dep_t = _tensors(torch, dev, ref)
    rgba = torch.full(((n + 64) * 4,), FILL, dtype=torch.uint8, device=dev)
    accum = torch.full(((n + 64) * 12,), FILL, dtype=torch.uint8, device=dev)
    ends = torch.full(((n + 64) * 4,), FILL, dtype=torch.uint8, device=dev)
    W, H = _load(gpu_ctx, ref)
    st = gpu_ctx.render_cached_device(ref.cam, ref.params, rec_t, dep_t, rgba, accum, ends, sync=True)
    r, a, e = rgba.cpu().numpy(), accum.cpu().numpy(), ends.cpu().numpy()
    assert (r[n * 4:] == FILL).all() and (a[n * 12:] == FILL).all() and (e[n * 4:] == FILL).all(), f"{size}: written past the frame"
    dgot = dict(rgba=r[:n * 4].reshape(H, W, 4), accum=a[:n * 12].view(np.float32).reshape(H, W, 3), ends_px=e[:n * 4].view(np.uint32).reshape(H, W))
    FR.assert_equal(dgot, gpu_ctx.rng_store(W, H, O.STATE_DTYPE), want, f"{name} {size} device form")
    assert st["segments"] == want["segments"] and st["algorithmic_hbm_bytes"] == n * 116
    # without the optional buffers
    rgba2 = torch.zeros(n * 4, dtype=torch.uint8, device=dev)
    _load(gpu_ctx, ref)
    st = gpu_ctx.render_cached_device(ref.cam, ref.params, rec_t, dep_t, rgba2, sync=True)
    assert (rgba2.cpu().numpy() == r[:n * 4]).all() and st["algorithmic_hbm_bytes"] == n * 100
    assert gpu_ctx.rng_store(W, H, O.STATE_DTYPE).tobytes() == want["states"].tobytes()


@pytest.mark.parametrize("visible", [False, True])
def test_device_form_on_a_torch_stream(gpu_ctx, visible):
    """on a stream other than the context's; one asynchronous call, then a timed one: equal results, the reference's"""
    import torch
    ref = FR.reference("scene6", 1, (40, 33), mask="fractional", visible=visible)
    want = ref.frames[0]
    gpu_ctx.upload_world(ref.world)
    dev = torch.device("cuda:0")
    n = 40 * 33
    stream = torch.cuda.Stream(device=dev)
    outs = []
    with torch.cuda.stream(stream):
        rec_t, dep_t = _tensors(torch, dev, ref)
        for sync in (False, True):
            rgba = torch.zeros(n * 4, dtype=torch.uint8, device=dev)
            accum = torch.zeros(n * 3, dtype=torch.float32, device=dev)
            ends = torch.zeros(n, dtype=torch.int32, device=dev)
            W, H = _load(gpu_ctx, ref)
            st = gpu_ctx.render_cached_device(ref.cam, ref.params, rec_t, dep_t, rgba, accum, ends, sync=sync)
            assert (st is None) == (not sync)  # enqueued, not waited for / timed
            stream.synchronize()
            outs.append((dict(rgba=rgba.cpu().numpy().reshape(H, W, 4), accum=accum.cpu().numpy().reshape(H, W, 3),
                              ends_px=ends.cpu().numpy().view(np.uint32).reshape(H, W)), gpu_ctx.rng_store(W, H, O.STATE_DTYPE), st))
    assert outs[1][2]["seconds"] > 0 and outs[1][2]["segments"] == want["segments"]
    for got, states, _ in outs:
        FR.assert_equal(got, states, want, f"scene6 on a torch stream visible={visible}")


@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("name", FR.WORLDS)
def test_depth_at_the_bounce_limit_is_the_render(gpu_ctx, name, visible):
    """K = bounce_limit on the device equals ctx.render(cam, MODE_MEGA) on the device, to the bit, statistics included"""
    cam = FR.camera(name, (40, 33))
    ref = FR.reference(name, cam.bounce_limit, (40, 33), visible=visible)
    gpu_ctx.upload_world(ref.world)
    got, states = _device_frame(gpu_ctx, ref)
    W, H = _load(gpu_ctx, ref)
    plain = gpu_ctx.render(ref.cam, mode=hip.MODE_MEGA, want_accum=True, want_segments=True)
    pstates = gpu_ctx.rng_store(W, H, O.STATE_DTYPE)
    assert (got["rgba"] == plain["rgba"]).all() and (got["accum"].view(np.uint32) == plain["accum"].view(np.uint32)).all()
    assert (got["segments_px"] == plain["segments_px"]).all() and states.tobytes() == pstates.tobytes() and not got["ends_px"].any()
    assert got["stats"]["segments"] == plain["stats"]["segments"] and got["stats"]["rng_draws"] == plain["stats"]["rng_draws"]
    FR.assert_equal(got, states, ref.frames[0], f"{name} K=bounce_limit against the reference")
    # an empty volume likewise
    zeros = FR.reference(name, 0, (40, 33), mask="zeros", visible=visible)
    got, states = _device_frame(gpu_ctx, zeros)
    assert (got["rgba"] == plain["rgba"]).all() and (got["accum"].view(np.uint32) == plain["accum"].view(np.uint32)).all()
    assert states.tobytes() == pstates.tobytes() and got["stats"]["rng_draws"] == plain["stats"]["rng_draws"] and not got["ends_px"].any()


def _cameras(cam0):
    c1 = host.camera_input(S.Camera.from_buffer_copy(cam0), "W")
    c2 = host.camera_input(S.Camera.from_buffer_copy(c1), None, (6, -3))
    return [cam0, c1, c2]


@pytest.mark.parametrize("visible", [False, True])
def test_a_view_with_the_cache_attached_is_the_hand_chain(gpu_ctx, visible):
    """temporal + SVGF over 3 frames of a moving camera: the view's buffers equal render_cached_device followed by the stage calls
    chained by hand, bit for bit; attaching resets the frame count; detaching gives the plain view's frames again"""
    import torch
    ref = FR.reference("scene6", 1, (40, 33), mask="fractional", visible=visible)
    W, H = 40, 33
    n = W * H
    cams = _cameras(ref.cam)
    gpu_ctx.upload_world(ref.world)
    dev = torch.device("cuda:0")
    rec_t, dep_t = _tensors(torch, dev, ref)
    # by hand
    gpu_ctx.rng_load(np.ascontiguousarray(ref.streams0), W, H)
    th = hip.TemporalHistory(W, H, backend=gpu_ctx)
    want = []
    for cam in cams:
        rgba = torch.zeros(n * 4, dtype=torch.uint8, device=dev)
        accum = torch.zeros(n * 3, dtype=torch.float32, device=dev)
        ends = torch.zeros(n, dtype=torch.int32, device=dev)
        gpu_ctx.render_cached_device(cam, ref.params, rec_t, dep_t, rgba, accum, ends, sync=True)
        acc = accum.cpu().numpy().reshape(H, W, 3)
        f = gpu_ctx.render_features(cam)
        t = th.step(acc, f["normal"], f["depth"], cam)
        t = dict(accum=t["accum"].copy(), variance=t["variance"].copy())
        d = gpu_ctx.svgf(t["accum"], f["albedo"], f["normal"], f["depth"], t["variance"])
        want.append(dict(raw_accum=acc, accum=t["accum"], variance=t["variance"], filtered=d["accum"], rgba=d["rgba"],
                         ends=ends.cpu().numpy().view(np.uint32).reshape(H, W)))
    states_after = gpu_ctx.rng_store(W, H, O.STATE_DTYPE)
    assert (want[0]["raw_accum"].view(np.uint32) == ref.frames[0]["accum"].view(np.uint32)).all(), "the first frame is the reference's"
    # the view
    gpu_ctx.rng_load(np.ascontiguousarray(ref.streams0), W, H)
    with gpu_ctx.view(W, H, temporal=1, filter=hip.FILTER_SVGF) as v:
        with pytest.raises(hip.MortHipError) as err:
            v.read("ends")  # no cache attached
        assert err.value.status == INVALID
        v.set_cache(ref.params, rec_t, dep_t)
        for i, cam in enumerate(cams):
            out = v.frame(cam)
            assert out["stats"]["frame"] == i and out["stats"]["render"]["kernel_name"] == _kernel(ref)
            assert (out["rgba"] == want[i]["rgba"]).all(), f"frame {i}: rgba"
            for k in ("raw_accum", "accum", "variance", "filtered"):
                assert (v.read(k).view(np.uint32) == want[i][k].view(np.uint32)).all(), f"frame {i}: {k}"
            assert (v.read("ends") == want[i]["ends"]).all(), f"frame {i}: ends"
        assert gpu_ctx.rng_store(W, H, O.STATE_DTYPE).tobytes() == states_after.tobytes()
        with pytest.raises(hip.MortHipError) as err:
            v.frame(cams[0], mode=hip.MODE_WAVE)
        assert err.value.status == UNSUPPORTED
        # attaching again forgets the history, as reset() does
        v.set_cache(ref.params, rec_t, dep_t)
        gpu_ctx.rng_load(np.ascontiguousarray(ref.streams0), W, H)
        out = v.frame(cams[0])
        assert out["stats"]["frame"] == 0 and out["stats"]["history_reset"] == 1 and (out["rgba"] == want[0]["rgba"]).all()
        # the host-array form: the view's own copies of the volume, replaced by the next attach of either form
        for attach in ((np.array(ref.records), None if ref.depth is None else np.array(ref.depth)), (rec_t, dep_t)) * 2:
            v.set_cache(ref.params, *attach)
            gpu_ctx.rng_load(np.ascontiguousarray(ref.streams0), W, H)
            for i in range(2):
                out = v.frame(cams[i])
                assert out["stats"]["frame"] == i and (out["rgba"] == want[i]["rgba"]).all() and (v.read("ends") == want[i]["ends"]).all()
        v.set_cache(ref.params, np.array(ref.records), None if ref.depth is None else np.array(ref.depth))
        L = hip.lib()
        bad = FR.params(65, ref.grid, ref.vis)
        assert L.mort_hip_view_set_cache_host(v._h, C.byref(bad), ref.records.ctypes.data, ref.depth.ctypes.data if ref.depth is not None else None) == INVALID
        assert L.mort_hip_view_set_cache_host(v._h, None, ref.records.ctypes.data, None) == INVALID
        assert L.mort_hip_view_set_cache_host(v._h, C.byref(ref.params), None, None) == INVALID
        assert L.mort_hip_view_set_cache_host(v._h, C.byref(ref.params), ref.records.ctypes.data, None if ref.depth is not None else ref.records.ctypes.data) == INVALID
        gpu_ctx.rng_load(np.ascontiguousarray(ref.streams0), W, H)
        assert (v.frame(cams[0])["rgba"] == want[0]["rgba"]).all(), "a refused attach leaves the cache that was there"
        # detached: the plain view's frames
        v.set_cache(None)
        gpu_ctx.rng_load(np.ascontiguousarray(ref.streams0), W, H)
        out = v.frame(cams[0])
        assert out["stats"]["frame"] == 0 and out["stats"]["render"]["kernel_name"] != _kernel(ref)
        raw = v.read("raw_accum")
        rgba_plain = out["rgba"]
    gpu_ctx.rng_load(np.ascontiguousarray(ref.streams0), W, H)
    with gpu_ctx.view(W, H, temporal=1, filter=hip.FILTER_SVGF) as v:  # a view that never had a cache
        out = v.frame(cams[0])
        assert (out["rgba"] == rgba_plain).all() and (v.read("raw_accum").view(np.uint32) == raw.view(np.uint32)).all()
    plain = O.render(ref.world, ref.cam, states=ref.streams0.copy(), nthreads=4)
    assert (raw.view(np.uint32) == plain["accum"].view(np.uint32)).all()


@pytest.mark.parametrize("name", ["scene6", "scene1"])
def test_cached_frames_between_plain_renders_continue_the_streams(gpu_ctx, name):
    """cached, plain, cached, plain on one context: the oracle's frames continued over the same streams"""
    ref = FR.reference(name, 1, (40, 33), mask="fractional", visible=True)
    W, H = 40, 33
    gpu_ctx.upload_world(ref.world)
    gpu_ctx.rng_load(np.ascontiguousarray(ref.streams0), W, H)
    streams = ref.streams0.copy()
    for i in range(4):
        if i % 2 == 0:
            want = FR.frame(ref.world, ref.cam, 1, ref.grid, ref.records, ref.depth, ref.vis, streams)
            got = gpu_ctx.render_cached(ref.cam, ref.params, ref.records, ref.depth, want_segments=True)
            assert (got["ends_px"] == want["ends_px"]).all(), i
        else:
            want = O.render(ref.world, ref.cam, states=streams, nthreads=4)
            got = gpu_ctx.render(ref.cam, mode=hip.MODE_MEGA, want_accum=True, want_segments=True)
        assert (got["rgba"] == want["rgba"]).all() and (FR.words(got["accum"]) == FR.words(want["accum"])).all(), i
        assert (got["segments_px"] == want["segments_px"]).all() and got["stats"]["segments"] == want["segments"], i
        assert gpu_ctx.rng_store(W, H, O.STATE_DTYPE).tobytes() == streams.tobytes(), i


def test_argument_checks_on_the_device():
    import torch
    ref = FR.reference("scene6", 1, FR.SIZE, mask="ones", visible=True)
    W, H = FR.SIZE
    n = W * H
    L = hip.lib()
    dev = torch.device("cuda:0")
    probes = ref.grid.probes
    sizes = dict(rgba=n * 4, accum=n * 12, ends=n * 4, records=probes * 128, depth=probes * 800)

    def params(visible=True, **kw):
        p = FR.params(1, ref.grid, ref.vis if visible else None)
        for k, v in kw.items():
            obj, _, field = k.rpartition("__")
            setattr(getattr(p, obj) if obj else p, field, v)
        return p

    def camera(**kw):
        c = S.Camera.from_buffer_copy(ref.cam)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    with hip.Context(0) as ctx:
        buf = torch.zeros(sum(sizes.values()) + 128, dtype=torch.uint8, device=dev)
        at, ptr = buf.data_ptr(), {}
        for k, v in sizes.items():
            assert at % 16 == 0
            ptr[k] = at
            at += (v + 15) // 16 * 16

        def call(p, visible=True, cam=ref.cam, **kw):
            a = dict(ptr)
            a.update(kw)
            return L.mort_hip_render_cached_device(ctx._h, C.byref(cam) if cam is not None else None, C.byref(p) if p is not None else None, a["records"],
                                                   a["depth"] if visible else None, a["rgba"], a["accum"], a["ends"], None, None)

        assert call(params()) == NO_WORLD
        ctx.upload_world(ref.world)
        assert call(params()) == NO_RNG
        ctx.rng_seed(1, W + 1, H)
        assert call(params()) == NO_RNG, "streams of another frame size"
        ctx.rng_seed(1, W, H)
        torch.cuda.synchronize()
        assert call(None) == INVALID and call(params(), cam=None) == INVALID
        for k in ("records", "rgba"):
            assert call(params(), **{k: None}) == INVALID, k
        assert call(params(), False) == INVALID and call(params(False), True) == INVALID, "the maps go with the flag"
        assert call(params(flags=3)) == INVALID and call(params(False, flags=2), False) == INVALID
        assert call(params(cache_depth=-1)) == INVALID and call(params(cache_depth=65)) == INVALID
        assert call(params(), accum=ptr["rgba"] + 16) == INVALID            # accumulators over the image
        assert call(params(), ends=ptr["accum"] + 16) == INVALID           # counts over the accumulators
        assert call(params(), rgba=ptr["records"]) == INVALID              # the image over the records
        assert call(params(), ends=ptr["depth"] + 800) == INVALID          # counts over the maps
        for k in ("records", "depth", "rgba", "accum", "ends"):              # not 16-byte aligned
            assert call(params(), **{k: ptr[k] + 4}) == INVALID, k
        for kw, status in ((dict(image_width=0), INVALID), (dict(sqrt_spp=-1), INVALID), (dict(bounce_limit=-1), CAPACITY), (dict(bounce_limit=65), CAPACITY),
                           (dict(light_obj_type=S.OBJ_SPHERE, light_obj_idx=1 << 20), INVALID)):
            assert call(params(), cam=camera(**kw)) == status, kw
        for kw in (dict(vis__min_visibility=2.0), dict(vis__normal_bias=-1.0)):
            assert call(params(**kw)) == INVALID, kw
        for bad in (0, hip.VOLUME_MAX_COUNT + 1):
            p = params()
            p.grid.count[0] = bad
            assert call(p) == INVALID, bad
        p = params()
        p.grid.spacing[1] = 0.0
        assert call(p) == INVALID
        ctx.set_partition(0, 2)
        ctx.rng_seed(1, W, H)
        assert call(params()) == UNSUPPORTED
        ctx.set_partition(0, 1)
        ctx.rng_load(np.ascontiguousarray(ref.streams0), W, H)
        torch.cuda.synchronize()
        assert (buf == 0).all(), "a refused call writes nothing"
        # and the checks refuse nothing they should not
        for k, arr in (("records", ref.records), ("depth", ref.depth)):
            off = ptr[k] - buf.data_ptr()
            buf[off:off + sizes[k]] = torch.from_numpy(np.array(arr).view(np.uint8).reshape(-1)).to(dev)
        assert call(params()) == 0
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        off = ptr["rgba"] - buf.data_ptr()
        assert (got[off:off + n * 4].reshape(H, W, 4) == ref.frames[0]["rgba"]).all()
        # the view's attach checks what the frames will
        with ctx.view(W, H, temporal=0, filter=hip.FILTER_NONE) as v:
            for args in ((params(), ptr["records"], None), (params(False), ptr["records"], ptr["depth"]), (params(), None, ptr["depth"]),
                         (params(), ptr["records"] + 4, ptr["depth"]), (params(cache_depth=65), ptr["records"], ptr["depth"])):
                assert L.mort_hip_view_set_cache(v._h, C.byref(args[0]), args[1], args[2]) == INVALID
            assert L.mort_hip_view_set_cache(v._h, None, None, None) == 0


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORT = os.path.join(ROOT, "mort_amd", "bin", "mort")


@pytest.mark.parametrize("extra", [[], ["--visibility", "5", "--frames", "2", "--keys", "W", "--temporal", "--svgf"]])
def test_cli_cache_render_on_the_gpu_is_the_host_mode(tmp_path, extra):
    """`mort 6 ... --cache-render` through a view with the cache attached writes the bytes `--mode host` writes, and reports the same
    segments and ends"""
    def run(mode, name):
        out = tmp_path / name
        p = subprocess.run([MORT, "6", *mode, "--width", "40", "--spp", "4", "--sh-volume", "100,100,100,455,455,455,3,3,2,64", "--cache-depth", "1",
                            "--cache-render", "--out", str(out)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        return json.loads(p.stdout.strip().splitlines()[-1]), out.read_bytes()

    gj, gpu = run([], "gpu.ppm")
    hj, cpu = run(["--mode", "host", "--threads", "4"], "host.ppm")
    assert gpu == cpu
    for k in ("segments", "ends", "cache_depth", "probes", "directions", "probe_samples", "spp_effective"):
        assert gj[k] == hj[k], k
    assert gj["ends"] > 0 and gj["mode"] == "mega" and gj["kernel"].startswith("cached_frame_kernel<true, ") and ("normal_bias" in gj) == bool(extra)
