"""Radiance queries on the MI355X (radiance.hip): query_radiance_kernel must give the host form's answers (the same
body, dev_radiance.h) and the CPU oracle's ray_color sums, tolerance 0 -- colours as raw words (any NaN equals any NaN), final
streams as all 48 bytes -- on the primary, secondary, far and axis rays of tests/query_rays.py; at every batch size around a wave
and a group; with one and three samples; on torch tensors and torch streams; and it must leave the render's state alone."""
import ctypes as C

import numpy as np
import pytest

from mort_amd import hip, host, structs as S
from tests import oracle_lib as O
from tests import query_rays as Q
from tests import radiance_ref as R

pytestmark = pytest.mark.gpu

# (world, bounce limit or None = the camera's, samples): scene 1 the item loop over a reference BVH; 6 light, quads, deep paths; 7
# media and NaN; 9 the tree with its primitives in L2, shallow and deep (the deep one with one sample: the oracle's side of three
# takes several seconds); a lit flat world with media; a PLACED world (a solid inside a medium, seen from outside); and two of
# tests/query_rays.py GEN_RANDOM_PICK: 75 chain ids with the primitives in LDS, duplicates with the primitives in L2
GEN_RANDOM_CASES = ("genrandom:instances_150_s1", "genrandom:ties_360_s0")
CASES = [(n, None, k) for n in ("scene1", "scene6", "scene7", "flat:lit_by_quad_with_media", "placed:solid_inside_medium") for k in (1, 3)] + \
    [("scene9", 4, 1), ("scene9", 4, 3), ("scene9", 40, 1)] + [(n, 8, k) for n in GEN_RANDOM_CASES for k in (1, 3)]
SIZES = (1, 63, 64, 65, 255, 256, 257, 1300)
NO_WORLD, INVALID, CAPACITY = -4, -1, -7


def _ref(name, limit=None, samples=1):
    return R.reference(name, samples=samples, bounce_limit=limit, light=R.world_light(name))


@pytest.mark.parametrize("name,limit,samples", CASES)
def test_device_equals_host_equals_oracle(gpu_ctx, name, limit, samples):
    ref = _ref(name, limit, samples)
    gpu_ctx.upload_world(ref.world)
    streams = ref.streams0.copy()
    got = gpu_ctx.query_radiance(ref.params, ref.rays, streams)["rgb"]
    R.assert_equal(got, streams, ref, f"{name} limit={limit} samples={samples} device")
    hs = ref.streams0.copy()
    hrgb = hip.query_radiance_host(ref.world, ref.params, ref.rays, hs, tree=Q.reach(ref.world)["tree"], nthreads=16)["rgb"]
    assert (Q._words(hrgb) == Q._words(got)).all() and hs.tobytes() == streams.tobytes(), f"{name}: device / host"


def _mixed(ref, waves=22, seed=3):
    """far, axis and ordinary rays in every wave of 64: 6 + 6 + 52 of them, shuffled within the wave"""
    rng = np.random.default_rng(seed)
    pools = [np.arange(ref.slices[k].start, ref.slices[k].stop) for k in ("far", "axis")]
    pools.append(np.concatenate([np.arange(ref.slices[k].start, ref.slices[k].start + 600) for k in ("primary", "secondary")]))
    share = (6, 6, 52)
    idx = []
    for w in range(waves):
        lane = np.concatenate([np.take(pool, np.arange(w * m, (w + 1) * m), mode="wrap") for pool, m in zip(pools, share)])
        idx.append(rng.permutation(lane))
    return np.concatenate(idx)


@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("name", ["scene7", "scene1", "scene6"])
def test_partial_waves_and_groups(gpu_ctx, name, samples):
    """n around a wave (64) and a group (256), far, axis and ordinary rays in every wave: the rays past n are not there, the bytes
    past n are not written"""
    import torch
    ref = _ref(name, samples=samples)
    idx = _mixed(ref)
    assert len(idx) >= max(SIZES) + 64
    gpu_ctx.upload_world(ref.world)
    dev = torch.device("cuda:0")
    rays_t = torch.from_numpy(np.ascontiguousarray(ref.rays[idx[:max(SIZES) + 64]])).to(dev)
    for n in SIZES:
        sub = idx[:n]
        # the host-buffer form
        streams = np.ascontiguousarray(ref.streams0[sub])
        got = gpu_ctx.query_radiance(ref.params, np.ascontiguousarray(ref.rays[sub]), streams)["rgb"]
        R.assert_equal(got, streams, ref, f"{name} n={n}", idx=sub)
        # the _device form into the head of larger tensors: the tail keeps its bytes
        rgb_t = torch.full(((n + 64) * 12,), 0xa5, dtype=torch.uint8, device=dev)
        st_t = torch.from_numpy(np.ascontiguousarray(ref.streams0[idx[:n + 64]]).view(np.uint8).reshape(-1).copy()).to(dev)
        gpu_ctx.query_radiance_device(ref.params, rays_t[:n], st_t[:n * 48], rgb_t[:n * 12], sync=True)
        out, st = rgb_t.cpu().numpy(), st_t.cpu().numpy()
        assert (out[n * 12:] == 0xa5).all(), f"n={n}: colours written past the batch"
        assert st[n * 48:].tobytes() == np.ascontiguousarray(ref.streams0[idx[n:n + 64]]).tobytes(), f"n={n}: streams written past the batch"
        R.assert_equal(out[:n * 12].view(np.float32).reshape(n, 3), st[:n * 48], ref, f"{name} n={n} device form", idx=sub)


def test_device_form_on_a_torch_stream(gpu_ctx):
    """on a stream other than the context's; one asynchronous call, then a timed one: equal results, the oracle's"""
    import torch
    ref = _ref("scene9", 40)
    gpu_ctx.upload_world(ref.world)
    dev = torch.device("cuda:0")
    n = len(ref.rays)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rays = torch.from_numpy(ref.rays.copy()).to(dev)
        out = [torch.zeros(n * 3, dtype=torch.float32, device=dev) for _ in range(2)]
        st = [torch.from_numpy(ref.streams0.view(np.uint8).reshape(-1).copy()).to(dev) for _ in range(2)]
        assert gpu_ctx.query_radiance_device(ref.params, rays, st[0], out[0]) is None  # seconds == NULL: enqueued, not waited for
        sec = gpu_ctx.query_radiance_device(ref.params, rays, st[1], out[1], sync=True)
    stream.synchronize()
    assert sec > 0
    a, b = (o.cpu().numpy().reshape(n, 3) for o in out)
    assert a.tobytes() == b.tobytes() and (st[0] == st[1]).all()
    R.assert_equal(a, st[0].cpu().numpy(), ref, "scene9 on a torch stream")
    # the context's own stream (stream == NULL) gives the same
    out2 = torch.zeros(n * 3, dtype=torch.float32, device=dev)
    st2 = torch.from_numpy(ref.streams0.view(np.uint8).reshape(-1).copy()).to(dev)
    torch.cuda.synchronize()
    sec = C.c_double(0)
    assert hip.lib().mort_hip_query_radiance_device(gpu_ctx._h, C.byref(ref.params), n, rays.data_ptr(), st2.data_ptr(), out2.data_ptr(), None, C.byref(sec)) == 0
    R.assert_equal(out2.cpu().numpy().reshape(n, 3), st2.cpu().numpy(), ref, "scene9 on the context's stream")


@pytest.mark.parametrize("sid", [1, 9])
def test_queries_leave_the_render_alone(sid):
    """two frames with a radiance query before and between them equal two frames on a fresh context: image, accumulators, segment
    counts, RNG states, and the second frame's statistics (its tile order comes from the first frame's costs)"""
    world, cam = host.build_scene(sid, width=160, spp=4)
    W, H = cam.image_width, cam.image_height
    ref = _ref(f"scene{sid}", 4 if sid == 9 else None)
    rays = np.ascontiguousarray(ref.rays[:2000])

    def frames(with_queries):
        out = []
        with hip.Context(0) as ctx:
            ctx.upload_world(world)
            if with_queries:  # before any rng_seed: a radiance query needs no pixel RNG
                ctx.query_radiance(ref.params, rays, ref.streams0[:2000].copy())
            ctx.rng_seed(69420, W, H)
            for f in range(2):
                if with_queries and f:
                    ctx.query_radiance(ref.params, rays, ref.streams0[:2000].copy())
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
    ref = _ref("scene6")
    gpu_ctx.upload_world(ref.world)
    try:
        gpu_ctx.set_partition(1, 2)
        streams = ref.streams0.copy()
        got = gpu_ctx.query_radiance(ref.params, ref.rays, streams)["rgb"]
    finally:
        gpu_ctx.set_partition(0, 1)
    R.assert_equal(got, streams, ref, "scene6 under a partition")


def test_argument_checks_on_the_device():
    import torch
    ref = _ref("scene2")
    L = hip.lib()
    n = 64
    rays = np.ascontiguousarray(ref.rays[:n])
    dev = torch.device("cuda:0")
    p = C.byref(ref.params)
    with hip.Context(0) as ctx:
        with pytest.raises(hip.MortHipError) as e:
            ctx.query_radiance(ref.params, rays, ref.streams0[:n].copy())
        assert e.value.status == NO_WORLD
        buf = torch.zeros(n * 48 * 4, dtype=torch.uint8, device=dev)
        base = buf.data_ptr()
        d_rays, d_st, d_rgb = base, base + n * 32, base + n * 32 + n * 48
        assert L.mort_hip_query_radiance_device(ctx._h, p, n, d_rays, d_st, d_rgb, None, None) == NO_WORLD
        ctx.upload_world(ref.world)
        torch.cuda.synchronize()
        # an empty batch launches nothing and is fine; NULL buffers, overlapping buffers and misaligned device buffers are not
        assert L.mort_hip_query_radiance_device(ctx._h, p, 0, d_rays, d_st, d_rgb, None, None) == 0
        for a in ((None, d_st, d_rgb), (d_rays, None, d_rgb), (d_rays, d_st, None)):
            assert L.mort_hip_query_radiance_device(ctx._h, p, n, *a, None, None) == INVALID
        assert L.mort_hip_query_radiance_device(ctx._h, None, n, d_rays, d_st, d_rgb, None, None) == INVALID
        assert L.mort_hip_query_radiance_device(ctx._h, p, n, d_rays, d_st, d_rays + n * 32 - 16, None, None) == INVALID  # colours over the rays' tail
        assert L.mort_hip_query_radiance_device(ctx._h, p, n, d_rays, d_st, d_st + 48, None, None) == INVALID             # colours over the streams
        assert L.mort_hip_query_radiance_device(ctx._h, p, n, d_rays, d_rays + 16, d_rgb, None, None) == INVALID          # streams over the rays
        for a in ((d_rays + 4, d_st + 16, d_rgb + 16), (d_rays, d_st + 8, d_rgb + 16), (d_rays, d_st, d_rgb + 4)):  # not 16-byte aligned
            assert L.mort_hip_query_radiance_device(ctx._h, p, n, *a, None, None) == INVALID
        for field, value, status in (("samples", 0, INVALID), ("bounce_limit", -1, CAPACITY), ("bounce_limit", 65, CAPACITY),
                                     ("light_obj_idx", 1 << 20, INVALID)):
            q = hip.radiance_params_from_camera(ref.cam)
            q.light_obj_type = S.OBJ_SPHERE if field == "light_obj_idx" else q.light_obj_type
            setattr(q, field, value)
            assert L.mort_hip_query_radiance_device(ctx._h, C.byref(q), n, d_rays, d_st, d_rgb, None, None) == status, (field, value)
        assert (buf == 0).all()
        # and the checks refuse nothing they should not
        streams = ref.streams0[:n].copy()
        got = ctx.query_radiance(ref.params, rays, streams)["rgb"]
        R.assert_equal(got, streams, ref, "scene2", idx=np.arange(n))
