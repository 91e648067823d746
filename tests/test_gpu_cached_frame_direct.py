"""Direct-light cached frames on the MI355X (cached_frame_direct.hip): cached_frame_direct_kernel<TREE, VISIBLE>
must give the host form's frames (the same body, dev_cached_frame_direct.h) and those of the walk over the oracle
(tests/cached_frame_direct_ref.py), tolerance 0 -- uchar4, accumulators as raw words, per-pixel segments, both counts, all 48
bytes of every final stream, the statistics' totals -- on scene 6 and a lit flat world with media (the TREE kernels), on scene 1
and on a list of sphere lights over a reference BVH (the item loop); at frame sizes around a wave and a group; on torch tensors and
torch streams; equal to the cached frame and to the plain render where the contract says so; inside a view; and between cached
frames and plain renders, whose streams it continues."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from mort_amd import hip, host, structs as S
from tests import cached_frame_direct_ref as DR
from tests import cached_frame_ref as FR
from tests import oracle_lib as O
from tests import query_rays as Q

pytestmark = pytest.mark.gpu

NO_RNG, NO_WORLD, INVALID, UNSUPPORTED, CAPACITY = -5, -4, -1, -6, -7
FILL = 0xa5
BIG = (40, 33)


def _load(ctx, ref, states=None):
    W, H = ref.cam.image_width, ref.cam.image_height
    ctx.rng_load(np.ascontiguousarray(ref.streams0 if states is None else states), W, H)
    return W, H


def _device_frame(ctx, ref, states=None, **kw):
    W, H = _load(ctx, ref, states)
    got = ctx.render_cached_direct(ref.cam, ref.params, ref.records, ref.depth, want_segments=True, **kw)
    return got, ctx.rng_store(W, H, O.STATE_DTYPE)


def _tree(ref):
    return bool(Q.reach(ref.world)["tree"])


def _kernel(ref, direct=True):
    return f"cached_frame_{'direct_' if direct else ''}kernel<{'true' if _tree(ref) else 'false'}, {'true' if ref.depth is not None else 'false'}>"


def test_the_worlds_run_both_kernels():
    assert [bool(Q.reach(Q.build(n).world)["tree"]) for n in DR.WORLDS] == [n in DR.TREE_WORLDS for n in DR.WORLDS] == [True, False, True, False]


@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("depth,mask,lens", [(0, "fractional", False), (1, "slab", False), (2, "fractional", True), (1, "poison", False), (1, "holes", True)])
@pytest.mark.parametrize("name", DR.WORLDS)
def test_device_equals_host_equals_reference(gpu_ctx, name, depth, mask, lens, visible):
    ref = DR.reference(name, depth, mask=mask, visible=visible, lens=lens)
    want = ref.frames[0]
    gpu_ctx.upload_world(ref.world)
    got, states = _device_frame(gpu_ctx, ref)
    what = f"{name} {mask} K={depth} visible={visible} lens={lens}"
    DR.assert_equal(got, states, want, what + " device")
    st = got["stats"]
    npx = want["ends_px"].size
    assert st["segments"] == want["segments"] and st["pixels"] == npx and st["eff_samples"] == 4 * npx and st["seconds"] > 0
    assert st["kernel_name"] == _kernel(ref) and st["scene_in_lds"] == 0 and st["reference_walks"] == 0 and st["kernel_vgprs"] > 0
    assert st["algorithmic_hbm_bytes"] == npx * (100 + 12 + 4 + 4)
    h = hip.render_cached_direct_host(ref.world, ref.cam, ref.params, ref.records, ref.depth, states=ref.streams0, tree=_tree(ref), nthreads=16)
    DR.assert_equal(h, h["states"], want, what + " host")
    assert h["stats"]["rng_draws"] == st["rng_draws"], "device / host draws"
    assert (got["lit_px"] <= got["ends_px"]).all() and (got["ends_px"] <= 4).all()


def _tensors(torch, dev, ref):
    rec = torch.from_numpy(np.array(ref.records)).to(dev)  # copies: the reference's arrays are read-only
    dep = torch.from_numpy(np.array(ref.depth)).to(dev) if ref.depth is not None else None
    return rec, dep


@pytest.mark.parametrize("size", DR.SIZES)
@pytest.mark.parametrize("name,visible", [("scene6", True), (DR.CD.BVH_LIGHT_WORLD, False)])
def test_frame_sizes_round_a_wave_and_a_group(gpu_ctx, name, visible, size):
    """1, 63, 64, 65, 255, 256, 257 and 1320 pixels at K = 1, 4 spp, under the slab mask; the _device form writes into the heads of
    larger tensors, whose tails keep their fill; then without the optional buffers"""
    import torch
    ref = DR.reference(name, 1, size, mask="slab", visible=visible)
    want = ref.frames[0]
    gpu_ctx.upload_world(ref.world)
    got, states = _device_frame(gpu_ctx, ref)
    DR.assert_equal(got, states, want, f"{name} {size}")
    dev = torch.device("cuda:0")
    n = size[0] * size[1]
    rec_t, dep_t = _tensors(torch, dev, ref)
    rgba = torch.full(((n + 64) * 4,), FILL, dtype=torch.uint8, device=dev)
    accum = torch.full(((n + 64) * 12,), FILL, dtype=torch.uint8, device=dev)
    ends = torch.full(((n + 64) * 4,), FILL, dtype=torch.uint8, device=dev)
    lit = torch.full(((n + 64) * 4,), FILL, dtype=torch.uint8, device=dev)
    W, H = _load(gpu_ctx, ref)
    st = gpu_ctx.render_cached_direct_device(ref.cam, ref.params, rec_t, dep_t, rgba, accum, ends, lit, sync=True)
    r, a, e, l = rgba.cpu().numpy(), accum.cpu().numpy(), ends.cpu().numpy(), lit.cpu().numpy()
    assert (r[n * 4:] == FILL).all() and (a[n * 12:] == FILL).all() and (e[n * 4:] == FILL).all() and (l[n * 4:] == FILL).all(), f"{size}: written past the frame"
    dgot = dict(rgba=r[:n * 4].reshape(H, W, 4), accum=a[:n * 12].view(np.float32).reshape(H, W, 3), ends_px=e[:n * 4].view(np.uint32).reshape(H, W),
                lit_px=l[:n * 4].view(np.uint32).reshape(H, W))
    DR.assert_equal(dgot, gpu_ctx.rng_store(W, H, O.STATE_DTYPE), want, f"{name} {size} device form")
    assert st["segments"] == want["segments"] and st["algorithmic_hbm_bytes"] == n * 120
    # without the optional buffers
    rgba2 = torch.zeros(n * 4, dtype=torch.uint8, device=dev)
    _load(gpu_ctx, ref)
    st = gpu_ctx.render_cached_direct_device(ref.cam, ref.params, rec_t, dep_t, rgba2, sync=True)
    assert (rgba2.cpu().numpy() == r[:n * 4]).all() and st["algorithmic_hbm_bytes"] == n * 100 and st["segments"] == want["segments"]
    assert gpu_ctx.rng_store(W, H, O.STATE_DTYPE).tobytes() == want["states"].tobytes()


@pytest.mark.parametrize("visible", [False, True])
def test_device_form_on_a_torch_stream(gpu_ctx, visible):
    """on a stream other than the context's; one asynchronous call, then a timed one: equal results, the reference's"""
    import torch
    ref = DR.reference("scene6", 0, BIG, mask="fractional", visible=visible)
    want = ref.frames[0]
    gpu_ctx.upload_world(ref.world)
    dev = torch.device("cuda:0")
    n = BIG[0] * BIG[1]
    stream = torch.cuda.Stream(device=dev)
    outs = []
    with torch.cuda.stream(stream):
        rec_t, dep_t = _tensors(torch, dev, ref)
        for sync in (False, True):
            rgba = torch.zeros(n * 4, dtype=torch.uint8, device=dev)
            accum = torch.zeros(n * 3, dtype=torch.float32, device=dev)
            ends = torch.zeros(n, dtype=torch.int32, device=dev)
            lit = torch.zeros(n, dtype=torch.int32, device=dev)
            W, H = _load(gpu_ctx, ref)
            st = gpu_ctx.render_cached_direct_device(ref.cam, ref.params, rec_t, dep_t, rgba, accum, ends, lit, sync=sync)
            assert (st is None) == (not sync)  # enqueued, not waited for / timed
            stream.synchronize()
            outs.append((dict(rgba=rgba.cpu().numpy().reshape(H, W, 4), accum=accum.cpu().numpy().reshape(H, W, 3),
                              ends_px=ends.cpu().numpy().view(np.uint32).reshape(H, W), lit_px=lit.cpu().numpy().view(np.uint32).reshape(H, W)),
                         gpu_ctx.rng_store(W, H, O.STATE_DTYPE), st))
    assert outs[1][2]["seconds"] > 0 and outs[1][2]["segments"] == want["segments"]
    for got, states, _ in outs:
        DR.assert_equal(got, states, want, f"scene6 on a torch stream visible={visible}")


def _assert_same_frames(a, sa, b, sb, what):
    assert (a["rgba"] == b["rgba"]).all() and (a["accum"].view(np.uint32) == b["accum"].view(np.uint32)).all(), what
    assert (a["segments_px"] == b["segments_px"]).all() and sa.tobytes() == sb.tobytes(), what
    assert a["stats"]["segments"] == b["stats"]["segments"] and a["stats"]["rng_draws"] == b["stats"]["rng_draws"], what


@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("name", DR.WORLDS)
def test_the_identities_on_the_device(gpu_ctx, name, visible):
    """(i) no light object and (iii) bounce_limit == K + 1 against render_cached on the device, (ii) K = bounce_limit and an
    empty volume against render(MODE_MEGA) on the device, to the bit, statistics included"""
    gpu_ctx.upload_world(Q.build(name).world)
    for what, ref in (("(i)", DR.reference(name, 1, BIG, mask="fractional", visible=visible, light=False)),
                      ("(iii)", DR.reference(name, 1, BIG, mask="fractional", visible=visible, bounce_limit=2))):
        got, states = _device_frame(gpu_ctx, ref)
        W, H = _load(gpu_ctx, ref)
        plain = gpu_ctx.render_cached(ref.cam, ref.params, ref.records, ref.depth, want_segments=True)
        _assert_same_frames(got, states, plain, gpu_ctx.rng_store(W, H, O.STATE_DTYPE), f"{what} {name}")
        assert (got["ends_px"] == plain["ends_px"]).all() and got["ends_px"].any() and not got["lit_px"].any()
        assert plain["stats"]["kernel_name"] == _kernel(ref, False) and got["stats"]["kernel_name"] == _kernel(ref)
        DR.assert_equal(got, states, ref.frames[0], f"{what} {name} against the reference")
    cam = DR.camera(name, BIG)
    for ref in (DR.reference(name, cam.bounce_limit, BIG, visible=visible), DR.reference(name, 0, BIG, mask="zeros", visible=visible)):
        got, states = _device_frame(gpu_ctx, ref)
        W, H = _load(gpu_ctx, ref)
        plain = gpu_ctx.render(ref.cam, mode=hip.MODE_MEGA, want_accum=True, want_segments=True)
        _assert_same_frames(got, states, plain, gpu_ctx.rng_store(W, H, O.STATE_DTYPE), f"(ii) {name}")
        assert not got["ends_px"].any() and not got["lit_px"].any()
        DR.assert_equal(got, states, ref.frames[0], f"(ii) {name} against the reference")


def _cameras(cam0):
    c1 = host.camera_input(S.Camera.from_buffer_copy(cam0), "W")
    c2 = host.camera_input(S.Camera.from_buffer_copy(c1), None, (6, -3))
    return [cam0, c1, c2]


@pytest.mark.parametrize("visible", [False, True])
def test_a_view_with_the_direct_cache_attached_is_the_hand_chain(gpu_ctx, visible):
    """temporal + SVGF over 3 frames of a moving camera: the view's buffers equal render_cached_direct_device followed by the stage
    calls chained by hand, bit for bit, ends, lit and the final streams included; plain <-> direct <-> detached each reset the
    history; update_cache keeps the history and the direct-ness; MODE_WAVE is refused"""
    import torch
    ref = DR.reference("scene6", 0, BIG, mask="fractional", visible=visible)
    W, H = BIG
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
        lit = torch.zeros(n, dtype=torch.int32, device=dev)
        gpu_ctx.render_cached_direct_device(cam, ref.params, rec_t, dep_t, rgba, accum, ends, lit, sync=True)
        acc = accum.cpu().numpy().reshape(H, W, 3)
        f = gpu_ctx.render_features(cam)
        t = th.step(acc, f["normal"], f["depth"], cam)
        t = dict(accum=t["accum"].copy(), variance=t["variance"].copy())
        d = gpu_ctx.svgf(t["accum"], f["albedo"], f["normal"], f["depth"], t["variance"])
        want.append(dict(raw_accum=acc, accum=t["accum"], variance=t["variance"], filtered=d["accum"], rgba=d["rgba"],
                         ends=ends.cpu().numpy().view(np.uint32).reshape(H, W), lit=lit.cpu().numpy().view(np.uint32).reshape(H, W)))
    states_after = gpu_ctx.rng_store(W, H, O.STATE_DTYPE)
    assert (want[0]["raw_accum"].view(np.uint32) == ref.frames[0]["accum"].view(np.uint32)).all(), "the first frame is the reference's"
    assert (want[0]["lit"] == ref.frames[0]["lit_px"]).all() and want[0]["lit"].any()
    # the plain cached frame of the same volume, for the switches
    gpu_ctx.rng_load(np.ascontiguousarray(ref.streams0), W, H)
    with gpu_ctx.view(W, H, temporal=1, filter=hip.FILTER_SVGF) as v:
        v.set_cache(ref.params, rec_t, dep_t)
        plain_rgba = v.frame(cams[0])["rgba"]
        with pytest.raises(hip.MortHipError) as err:
            v.read("lit")  # a plain cache attached
        assert err.value.status == INVALID
        assert (plain_rgba != want[0]["rgba"]).any()
        # plain -> direct
        v.set_cache(ref.params, rec_t, dep_t, direct=True)
        gpu_ctx.rng_load(np.ascontiguousarray(ref.streams0), W, H)
        for i, cam in enumerate(cams):
            out = v.frame(cam)
            assert out["stats"]["frame"] == i and out["stats"]["render"]["kernel_name"] == _kernel(ref)
            assert (i > 0) or out["stats"]["history_reset"] == 1
            assert (out["rgba"] == want[i]["rgba"]).all(), f"frame {i}: rgba"
            for k in ("raw_accum", "accum", "variance", "filtered"):
                assert (v.read(k).view(np.uint32) == want[i][k].view(np.uint32)).all(), f"frame {i}: {k}"
            assert (v.read("ends") == want[i]["ends"]).all() and (v.read("lit") == want[i]["lit"]).all(), f"frame {i}: counts"
        assert gpu_ctx.rng_store(W, H, O.STATE_DTYPE).tobytes() == states_after.tobytes()
        with pytest.raises(hip.MortHipError) as err:
            v.frame(cams[0], mode=hip.MODE_WAVE)
        assert err.value.status == UNSUPPORTED
        # update_cache: the history goes on, the frames stay direct (host arrays, then tensors)
        gpu_ctx.rng_load(np.ascontiguousarray(ref.streams0), W, H)
        v.set_cache(ref.params, rec_t, dep_t, direct=True)
        assert v.frame(cams[0])["stats"]["frame"] == 0
        v.update_cache(np.array(ref.records), None if ref.depth is None else np.array(ref.depth))
        out = v.frame(cams[1])
        assert out["stats"]["frame"] == 1 and out["stats"]["render"]["kernel_name"] == _kernel(ref) and (out["rgba"] == want[1]["rgba"]).all()
        v.update_cache(rec_t, dep_t)
        out = v.frame(cams[2])
        assert out["stats"]["frame"] == 2 and (out["rgba"] == want[2]["rgba"]).all() and (v.read("lit") == want[2]["lit"]).all()
        # direct -> plain: the history is forgotten, lit is gone
        v.set_cache(ref.params, rec_t, dep_t)
        gpu_ctx.rng_load(np.ascontiguousarray(ref.streams0), W, H)
        out = v.frame(cams[0])
        assert out["stats"]["frame"] == 0 and out["stats"]["history_reset"] == 1 and (out["rgba"] == plain_rgba).all()
        assert out["stats"]["render"]["kernel_name"] == _kernel(ref, False)
        with pytest.raises(hip.MortHipError) as err:
            v.read("lit")
        assert err.value.status == INVALID
        # plain -> direct by the host-array form -> detached
        v.set_cache(ref.params, np.array(ref.records), None if ref.depth is None else np.array(ref.depth), direct=True)
        gpu_ctx.rng_load(np.ascontiguousarray(ref.streams0), W, H)
        for i in range(2):
            out = v.frame(cams[i])
            assert out["stats"]["frame"] == i and (out["rgba"] == want[i]["rgba"]).all() and (v.read("lit") == want[i]["lit"]).all()
        L = hip.lib()
        bad = DR.params(65, ref.grid, ref.vis)
        assert L.mort_hip_view_set_cache_direct_host(v._h, C.byref(bad), ref.records.ctypes.data, ref.depth.ctypes.data if ref.depth is not None else None) == INVALID
        assert L.mort_hip_view_set_cache_direct_host(v._h, None, ref.records.ctypes.data, None) == INVALID
        assert L.mort_hip_view_set_cache_direct(v._h, C.byref(ref.params), rec_t.data_ptr() + 4, dep_t.data_ptr() if dep_t is not None else None) == INVALID
        out = v.frame(cams[2])
        assert out["stats"]["frame"] == 2 and (out["rgba"] == want[2]["rgba"]).all(), "a refused attach leaves the cache and the history that were there"
        v.set_cache(None, direct=True)
        gpu_ctx.rng_load(np.ascontiguousarray(ref.streams0), W, H)
        out = v.frame(cams[0])
        assert out["stats"]["frame"] == 0 and not out["stats"]["render"]["kernel_name"].startswith("cached_frame")
        for k in ("ends", "lit"):
            with pytest.raises(hip.MortHipError) as err:
                v.read(k)
            assert err.value.status == INVALID
        plain = O.render(ref.world, ref.cam, states=ref.streams0.copy(), nthreads=4)
        assert (v.read("raw_accum").view(np.uint32) == plain["accum"].view(np.uint32)).all()


@pytest.mark.parametrize("name", ["scene6", DR.CD.BVH_LIGHT_WORLD])
def test_direct_cached_and_plain_frames_alternate_on_one_context(gpu_ctx, name):
    """direct, cached, plain, direct, ... on one context: the references' frames continued over the same streams"""
    ref = DR.reference(name, 1, BIG, mask="fractional", visible=True)
    W, H = BIG
    gpu_ctx.upload_world(ref.world)
    gpu_ctx.rng_load(np.ascontiguousarray(ref.streams0), W, H)
    streams = ref.streams0.copy()
    for i in range(6):
        if i % 3 == 0:
            want = DR.frame(ref.world, ref.cam, 1, ref.grid, ref.records, ref.depth, ref.vis, streams)
            got = gpu_ctx.render_cached_direct(ref.cam, ref.params, ref.records, ref.depth, want_segments=True)
            assert (got["ends_px"] == want["ends_px"]).all() and (got["lit_px"] == want["lit_px"]).all(), i
        elif i % 3 == 1:
            want = FR.frame(ref.world, ref.cam, 1, ref.grid, ref.records, ref.depth, ref.vis, streams)
            got = gpu_ctx.render_cached(ref.cam, ref.params, ref.records, ref.depth, want_segments=True)
            assert (got["ends_px"] == want["ends_px"]).all(), i
        else:
            want = O.render(ref.world, ref.cam, states=streams, nthreads=4)
            got = gpu_ctx.render(ref.cam, mode=hip.MODE_MEGA, want_accum=True, want_segments=True)
        assert (got["rgba"] == want["rgba"]).all() and (DR.words(got["accum"]) == DR.words(want["accum"])).all(), i
        assert (got["segments_px"] == want["segments_px"]).all() and got["stats"]["segments"] == want["segments"], i
        assert gpu_ctx.rng_store(W, H, O.STATE_DTYPE).tobytes() == streams.tobytes(), i


def test_argument_checks_on_the_device():
    import torch
    ref = DR.reference("scene6", 1, DR.SIZE, mask="ones", visible=True)
    W, H = DR.SIZE
    n = W * H
    L = hip.lib()
    dev = torch.device("cuda:0")
    probes = ref.grid.probes
    sizes = dict(rgba=n * 4, accum=n * 12, ends=n * 4, lit=n * 4, records=probes * 128, depth=probes * 800)

    def params(visible=True, **kw):
        p = DR.params(1, ref.grid, ref.vis if visible else None)
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
            return L.mort_hip_render_cached_direct_device(ctx._h, C.byref(cam) if cam is not None else None, C.byref(p) if p is not None else None,
                                                          a["records"], a["depth"] if visible else None, a["rgba"], a["accum"], a["ends"], a["lit"], None,
                                                          None)

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
        assert call(params(), accum=ptr["rgba"] + 16) == INVALID           # accumulators over the image
        assert call(params(), ends=ptr["accum"] + 16) == INVALID          # counts over the accumulators
        for k in ("rgba", "accum", "ends", "records", "depth"):            # lit over every other buffer
            assert call(params(), lit=ptr[k] + 16) == INVALID, k
        assert call(params(), ends=ptr["lit"]) == INVALID
        for k in ("records", "depth", "rgba", "accum", "ends", "lit"):     # not 16-byte aligned
            assert call(params(), **{k: ptr[k] + 4}) == INVALID, k
        for kw, status in ((dict(image_width=0), INVALID), (dict(sqrt_spp=-1), INVALID), (dict(bounce_limit=-1), CAPACITY), (dict(bounce_limit=65), CAPACITY),
                           (dict(light_obj_type=S.OBJ_SPHERE, light_obj_idx=1 << 20), INVALID)):
            assert call(params(), cam=camera(**kw)) == status, kw
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
        off = ptr["lit"] - buf.data_ptr()
        assert (got[off:off + n * 4].view(np.uint32).reshape(H, W) == ref.frames[0]["lit_px"]).all()
        assert call(params(), lit=None, accum=None, ends=None) == 0
        torch.cuda.synchronize()
        # the view's attach checks what the frames will
        with ctx.view(W, H, temporal=0, filter=hip.FILTER_NONE) as v:
            for args in ((params(), ptr["records"], None), (params(False), ptr["records"], ptr["depth"]), (params(), None, ptr["depth"]),
                         (params(), ptr["records"] + 4, ptr["depth"]), (params(cache_depth=65), ptr["records"], ptr["depth"])):
                assert L.mort_hip_view_set_cache_direct(v._h, C.byref(args[0]), args[1], args[2]) == INVALID
            assert L.mort_hip_view_set_cache_direct(v._h, None, None, None) == 0


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORT = os.path.join(ROOT, "mort_amd", "bin", "mort")


@pytest.mark.parametrize("extra", [[], ["--visibility", "5", "--frames", "2", "--keys", "W", "--temporal", "--svgf"]])
def test_cli_cache_render_direct_on_the_gpu_is_the_host_mode(tmp_path, extra):
    """`mort 6 ... --cache-render-direct` through a view with the direct cache attached writes the bytes `--mode host` writes, and
    reports the same segments, ends and lit"""
    def run(mode, name):
        out = tmp_path / name
        p = subprocess.run([MORT, "6", *mode, "--width", "40", "--spp", "4", "--sh-volume", "100,100,100,455,455,455,3,3,2,64", "--cache-depth", "1",
                            "--cache-render-direct", "--out", str(out)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        return json.loads(p.stdout.strip().splitlines()[-1]), out.read_bytes()

    gj, gpu = run([], "gpu.ppm")
    hj, cpu = run(["--mode", "host", "--threads", "4"], "host.ppm")
    assert gpu == cpu
    for k in ("segments", "ends", "lit", "cache_direct", "cache_depth", "probes", "directions", "probe_samples", "spp_effective"):
        assert gj[k] == hj[k], k
    assert 0 < gj["lit"] < gj["ends"] and gj["mode"] == "mega" and gj["kernel"].startswith("cached_frame_direct_kernel<true, ")
    assert ("normal_bias" in gj) == bool(extra)
