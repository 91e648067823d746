"""Light probes on the MI355X (probe.hip): probe_sh_kernel must give the host form's answers (the same body,
dev_probe.h) and the reference's of tests/probe_ref.py -- the oracle's ray_color and the contract restated in numpy -- at
tolerance 0: coefficients as raw words (any NaN equals any NaN), final streams as all 48 bytes; at every direction count at which
the group's shape or a wave's share of the batches changes; with one and three paths per direction; on torch tensors and torch
streams; and it must leave the render's state alone."""
import ctypes as C

import numpy as np
import pytest

from mort_amd import hip, host, structs as S
from tests import oracle_lib as O
from tests import probe_ref as P
from tests import query_rays as Q

pytestmark = pytest.mark.gpu

# (world, bounce limit or None = the camera's): scene 1 the item loop over a reference BVH; 6 light, quads, deep paths; 7 media and
# NaN; 9 the tree with its primitives in L2; a lit flat world with media
WORLDS = [("scene1", None), ("scene6", None), ("scene7", None), ("scene9", 4), ("flat:lit_by_quad_with_media", None)]
# directions -> batches per wave: 64 one wave of work; 128, 192, 256 one each for two, three, four waves; 320 wave 0 takes two;
# 576 the waves take 3 / 2 / 2 / 2
DIRECTIONS = (64, 128, 192, 256, 320, 576)
COUNTS = (1, 2, 5)
NO_WORLD, INVALID, CAPACITY = -4, -1, -7


def _ref(name, limit, D, samples=1, **kw):
    return P.reference(name, D, samples, limit, n=max(COUNTS), **kw)


@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("name,limit", WORLDS)
def test_device_equals_host_equals_reference(gpu_ctx, name, limit, samples):
    world = Q.build(name).world
    gpu_ctx.upload_world(world)
    tree = Q.reach(world)["tree"]
    for D in DIRECTIONS:
        ref = _ref(name, limit, D, samples)
        assert len(ref.probes) == max(COUNTS)
        for n in COUNTS:
            streams = ref.streams0[:n * D].copy()
            got = gpu_ctx.probe_bake(ref.params, ref.probes[:n], streams)["sh"]
            P.assert_equal(got, streams, ref, f"{name} limit={limit} samples={samples} D={D} n={n} device", n=n)
        hs = ref.streams0.copy()
        hsh = hip.probe_bake_host(ref.world, ref.params, ref.probes, hs, tree=tree, nthreads=16)["sh"]
        assert (Q._words(hsh) == Q._words(got)).all() and hs.tobytes() == streams.tobytes(), f"{name} D={D}: device / host"


@pytest.mark.parametrize("name,limit", [("scene7", None), ("scene1", None)])
def test_bytes_past_the_batch_are_untouched(gpu_ctx, name, limit):
    """the _device form into the head of larger tensors: the bytes past 27 n floats and past n D streams keep theirs"""
    import torch
    gpu_ctx.upload_world(Q.build(name).world)
    dev = torch.device("cuda:0")
    for D in (64, 320):
        ref = _ref(name, limit, D, 3)
        probes_t = torch.from_numpy(ref.probes.view(np.float32).copy()).to(dev)
        for n in (1, 2):
            sh_t = torch.full((n * 108 + 256,), 0xa5, dtype=torch.uint8, device=dev)
            st_t = torch.from_numpy(ref.streams0[:(n + 1) * D].view(np.uint8).reshape(-1).copy()).to(dev)
            gpu_ctx.probe_bake_device(ref.params, probes_t[:n * 4], st_t[:n * D * 48], sh_t[:n * 108], sync=True)
            out, st = sh_t.cpu().numpy(), st_t.cpu().numpy()
            assert (out[n * 108:] == 0xa5).all(), f"D={D} n={n}: coefficients written past the batch"
            assert st[n * D * 48:].tobytes() == np.ascontiguousarray(ref.streams0[n * D:(n + 1) * D]).tobytes(), f"D={D} n={n}: streams written past the batch"
            P.assert_equal(out[:n * 108].view(np.float32), st[:n * D * 48], ref, f"{name} D={D} n={n} device form", n=n)


def test_a_callers_direction_tensor_and_null(gpu_ctx):
    """the caller's own set (axis-parallel, zero-length, unnormalised entries; one with a NaN direction) as a tensor; NULL is the
    library's set, kept by the context per direction count: 64, then 128, then 64 again"""
    import torch
    gpu_ctx.upload_world(Q.build("scene1").world)
    dev = torch.device("cuda:0")
    n = max(COUNTS)

    def bake(ref, dirs):
        probes_t = torch.from_numpy(ref.probes.view(np.float32).copy()).to(dev)
        st_t = torch.from_numpy(ref.streams0.view(np.uint8).reshape(-1).copy()).to(dev)
        sh_t = torch.zeros(n * 27, dtype=torch.float32, device=dev)
        dirs_t = torch.from_numpy(np.ascontiguousarray(dirs).reshape(-1).copy()).to(dev) if dirs is not None else None
        gpu_ctx.probe_bake_device(ref.params, probes_t, st_t, sh_t, dirs=dirs_t, sync=True)
        return sh_t.cpu().numpy(), st_t.cpu().numpy()

    for kind in ("own", "nan"):
        ref = _ref("scene1", None, P.OWN_D, 3, dirs=kind)
        sh, st = bake(ref, ref.dirs)
        P.assert_equal(sh, st, ref, f"scene1 directions {kind}")
        got = gpu_ctx.probe_bake(ref.params, ref.probes, ref.streams0.copy(), dirs=ref.dirs)["sh"]
        assert (Q._words(got) == Q._words(ref.sh)).all(), "the host-buffer form with a set of the caller's"
    assert np.isnan(ref.sh).any()
    for D in (64, 128, 64):
        ref = _ref("scene1", None, D, 1)
        sh, st = bake(ref, None)
        P.assert_equal(sh, st, ref, f"scene1 D={D} the library's set")


def test_device_form_on_a_torch_stream(gpu_ctx):
    """on a stream other than the context's; one asynchronous call, then a timed one: equal results, the reference's"""
    import torch
    ref = _ref("scene9", 4, 320, 1)
    gpu_ctx.upload_world(ref.world)
    dev = torch.device("cuda:0")
    n = len(ref.probes)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        probes = torch.from_numpy(ref.probes.view(np.float32).copy()).to(dev)
        out = [torch.zeros(n * 27, dtype=torch.float32, device=dev) for _ in range(2)]
        st = [torch.from_numpy(ref.streams0.view(np.uint8).reshape(-1).copy()).to(dev) for _ in range(2)]
        assert gpu_ctx.probe_bake_device(ref.params, probes, st[0], out[0]) is None  # seconds == NULL: enqueued, not waited for
        sec = gpu_ctx.probe_bake_device(ref.params, probes, st[1], out[1], sync=True)
    stream.synchronize()
    assert sec > 0
    a, b = (o.cpu().numpy() for o in out)
    assert a.tobytes() == b.tobytes() and (st[0] == st[1]).all()
    P.assert_equal(a, st[0].cpu().numpy(), ref, "scene9 on a torch stream")
    # the context's own stream (stream == NULL) gives the same
    out2 = torch.zeros(n * 27, dtype=torch.float32, device=dev)
    st2 = torch.from_numpy(ref.streams0.view(np.uint8).reshape(-1).copy()).to(dev)
    torch.cuda.synchronize()
    sec = C.c_double(0)
    assert hip.lib().mort_hip_probe_bake_device(gpu_ctx._h, C.byref(ref.params), n, probes.data_ptr(), None, st2.data_ptr(), out2.data_ptr(), None, C.byref(sec)) == 0
    P.assert_equal(out2.cpu().numpy(), st2.cpu().numpy(), ref, "scene9 on the context's stream")


@pytest.mark.parametrize("sid", [1, 9])
def test_bakes_leave_the_render_alone(sid):
    """two frames with a bake before and between them equal two frames on a fresh context: image, accumulators, segment counts,
    RNG states, and the second frame's statistics (its tile order comes from the first frame's costs)"""
    world, cam = host.build_scene(sid, width=160, spp=4)
    W, H = cam.image_width, cam.image_height
    ref = _ref(f"scene{sid}", 4 if sid == 9 else None, 128, 1)

    def frames(with_bakes):
        out = []
        with hip.Context(0) as ctx:
            ctx.upload_world(world)
            if with_bakes:  # before any rng_seed: a bake needs no pixel RNG
                ctx.probe_bake(ref.params, ref.probes, ref.streams0.copy())
            ctx.rng_seed(69420, W, H)
            for f in range(2):
                if with_bakes and f:
                    ctx.probe_bake(ref.params, ref.probes, ref.streams0.copy())
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


def test_bakes_ignore_the_partition(gpu_ctx):
    ref = _ref("scene6", None, 128, 1)
    gpu_ctx.upload_world(ref.world)
    try:
        gpu_ctx.set_partition(1, 2)
        streams = ref.streams0.copy()
        got = gpu_ctx.probe_bake(ref.params, ref.probes, streams)["sh"]
    finally:
        gpu_ctx.set_partition(0, 1)
    P.assert_equal(got, streams, ref, "scene6 under a partition")


def test_argument_checks_on_the_device():
    import torch
    D, n = 64, 2
    ref = P.reference("scene2", D, 1, n=n)
    L = hip.lib()
    dev = torch.device("cuda:0")
    p = C.byref(ref.params)
    with hip.Context(0) as ctx:
        with pytest.raises(hip.MortHipError) as e:
            ctx.probe_bake(ref.params, ref.probes, ref.streams0.copy())
        assert e.value.status == NO_WORLD
        buf = torch.zeros(n * 16 + D * 12 + n * D * 48 + n * 108 + 8192, dtype=torch.uint8, device=dev)
        base = buf.data_ptr()
        d_pr, d_dirs, d_st = base, base + n * 16, base + n * 16 + D * 12
        d_sh = d_st + n * D * 48
        assert all(a % 16 == 0 for a in (d_pr, d_dirs, d_st, d_sh))
        call = lambda q, m, *a: L.mort_hip_probe_bake_device(ctx._h, q, m, *a, None, None)  # noqa: E731
        assert call(p, n, d_pr, d_dirs, d_st, d_sh) == NO_WORLD
        ctx.upload_world(ref.world)
        torch.cuda.synchronize()
        # an empty batch launches nothing and is fine; NULL buffers, overlapping buffers and misaligned device buffers are not
        assert call(p, 0, d_pr, d_dirs, d_st, d_sh) == 0
        for a in ((None, d_dirs, d_st, d_sh), (d_pr, d_dirs, None, d_sh), (d_pr, d_dirs, d_st, None)):
            assert call(p, n, *a) == INVALID
        assert call(None, n, d_pr, d_dirs, d_st, d_sh) == INVALID
        assert call(p, n, d_pr, d_dirs, d_st, d_dirs + D * 12 - 16) == INVALID   # coefficients over the directions' tail
        assert call(p, n, d_pr, d_dirs, d_st, d_st + 48) == INVALID              # coefficients over the streams
        assert call(p, n, d_pr, d_dirs, d_pr + 16, d_sh) == INVALID              # streams over the probes
        assert call(p, n, d_pr, d_dirs, d_sh - 16, d_sh) == INVALID              # streams over the coefficients
        for a in ((d_pr + 4, d_dirs, d_st, d_sh), (d_pr, d_dirs + 4, d_st, d_sh), (d_pr, d_dirs, d_st + 8, d_sh + n * D * 48), (d_pr, d_dirs, d_st, d_sh + 4)):
            assert call(p, n, *a) == INVALID, "not 16-byte aligned"
        for directions in (0, 63, 65, 4160):
            q = hip.probe_params_from_camera(ref.cam, directions)
            assert call(C.byref(q), n, d_pr, d_dirs, d_st, d_sh) == INVALID, directions
        for field, value, status in (("samples", 0, INVALID), ("bounce_limit", -1, CAPACITY), ("bounce_limit", 65, CAPACITY),
                                     ("light_obj_idx", 1 << 20, INVALID)):
            q = hip.probe_params_from_camera(ref.cam, D)
            q.rp.light_obj_type = S.OBJ_SPHERE if field == "light_obj_idx" else q.rp.light_obj_type
            setattr(q.rp, field, value)
            assert call(C.byref(q), n, d_pr, d_dirs, d_st, d_sh) == status, (field, value)
        assert (buf == 0).all()
        # and the checks refuse nothing they should not
        streams = ref.streams0.copy()
        got = ctx.probe_bake(ref.params, ref.probes, streams)["sh"]
        P.assert_equal(got, streams, ref, "scene2")
