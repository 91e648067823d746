"""The feature pass and the a-trous denoiser on the MI355X: feat_kernel and atrous_kernel must give the host
forms' bits (the same bodies, dev_features.h), with either traversal, under a row partition and on torch tensors; and they must
leave the render's state alone -- the next frame is bit-identical to a run without them.  feat_kernel is also held, word for
word, to tests/feature_ref.py: the contract restated from the CPU oracle's entry points, which shares no code with it."""
import ctypes as C

import numpy as np
import pytest

from mort_amd import hip, host
from tests.feature_ref import MEDIUM, SOLID, assert_same_words, oracle_features
from tests.worlds import FLAT_WORLDS, PLACED, flat_camera, flat_world, random_world, set_view

pytestmark = pytest.mark.gpu

KEYS = ("albedo", "normal", "depth")


def _same_features(a, b, what=""):
    for k in KEYS:
        assert (a[k].view(np.uint32) == b[k].view(np.uint32)).all(), f"{what} {k} differs"


def _gpu_features(ctx, world, cam, no_gen, monkeypatch):
    if no_gen:
        monkeypatch.setenv("MORT_NO_GEN", "1")
    else:
        monkeypatch.delenv("MORT_NO_GEN", raising=False)
    ctx.upload_world(world)
    monkeypatch.delenv("MORT_NO_GEN", raising=False)
    return ctx.render_features(cam)


@pytest.mark.parametrize("sid", range(1, 11))
def test_features_match_host_on_every_scene(gpu_ctx, monkeypatch, sid):
    world, cam = host.build_scene(sid, width=160, spp=4)
    ref = hip.render_features_host(world, cam, nthreads=16)
    for no_gen in (False, True):
        _same_features(_gpu_features(gpu_ctx, world, cam, no_gen, monkeypatch), ref, f"scene {sid} MORT_NO_GEN={int(no_gen)}")


@pytest.mark.parametrize("name", sorted(FLAT_WORLDS))
def test_features_match_host_on_awkward_worlds(gpu_ctx, monkeypatch, name):
    spec = FLAT_WORLDS[name]
    w, ids = flat_world(spec["prims"], media=spec.get("media", ()), late_list=spec.get("late_list", False))
    cam = flat_camera(light=ids[spec["light"][1]] if spec.get("light") else None)
    ref = hip.render_features_host(w, cam, nthreads=16, tree=True)
    for no_gen in (False, True):
        _same_features(_gpu_features(gpu_ctx, w, cam, no_gen, monkeypatch), ref, f"{name} MORT_NO_GEN={int(no_gen)}")


@pytest.mark.parametrize("sid", [1, 9])
def test_features_compose_under_a_partition(gpu_ctx, sid):
    world, cam = host.build_scene(sid, width=120, spp=1)
    ref = hip.render_features_host(world, cam, nthreads=16)
    gpu_ctx.upload_world(world)
    H, W = cam.image_height, cam.image_width
    parts = {k: np.full(ref[k].shape, np.nan, dtype=np.float32) for k in KEYS}
    try:
        for rank in range(2):
            gpu_ctx.set_partition(rank, 2, 8)
            out = {k: np.full(ref[k].shape, np.nan, dtype=np.float32) for k in KEYS}
            f = C.c_double(0)
            st = hip.lib().mort_hip_render_features(gpu_ctx._h, C.byref(cam), out["albedo"].ctypes.data, out["normal"].ctypes.data,
                                                    out["depth"].ctypes.data, C.byref(f))
            assert st == 0
            rows = [gpu_ctx.global_row(ly) for ly in range(gpu_ctx.local_rows(H))]
            others = sorted(set(range(H)) - set(rows))
            for k in KEYS:
                assert np.isnan(out[k][others]).all(), "rows not owned stay untouched"
                parts[k][rows] = out[k][rows]
    finally:
        gpu_ctx.set_partition(0, 1, 8)
    _same_features(parts, ref, f"scene {sid}, two ranks")


# ---- feat_kernel<false> (MORT_NO_GEN=1) and feat_kernel<true> against the oracle-made reference, tolerance 0 ----
def _gpu_equals_oracle(ctx, world, cam, monkeypatch, what):
    ref = oracle_features(world, cam, nthreads=16)
    for no_gen in (False, True):
        assert_same_words(_gpu_features(ctx, world, cam, no_gen, monkeypatch), ref, f"{what} MORT_NO_GEN={int(no_gen)}")
    return ref


def _sized(sid, width, height):
    """a built-in scene's camera at an arbitrary frame size"""
    world, cam = host.build_scene(sid, width=width, spp=1, aspect=width / (height + 0.5))
    assert (cam.image_width, cam.image_height) == (width, height)
    return world, cam


@pytest.mark.parametrize("sid", range(1, 11))
def test_features_equal_the_oracle_on_every_scene(gpu_ctx, monkeypatch, sid):
    world, cam = host.build_scene(sid, width=160, spp=1)
    ref = _gpu_equals_oracle(gpu_ctx, world, cam, monkeypatch, f"scene {sid}")
    assert (ref["kind"] == SOLID).sum() > (0.005 if sid == 10 else 0.3) * ref["kind"].size
    if sid == 7:
        assert (ref["kind"] == MEDIUM).sum() > 0.1 * ref["kind"].size
    if sid in (8, 9):
        assert (ref["started_inside"] >= 1).all() and (ref["depth"] > 1).all(), "geometry, not the fog shell around the camera"


@pytest.mark.parametrize("name", sorted(FLAT_WORLDS))
def test_features_equal_the_oracle_on_awkward_worlds(gpu_ctx, monkeypatch, name):
    spec = FLAT_WORLDS[name]
    w, ids = flat_world(spec["prims"], media=spec.get("media", ()), late_list=spec.get("late_list", False))
    cam = flat_camera(light=ids[spec["light"][1]] if spec.get("light") else None, spp=1)
    ref = _gpu_equals_oracle(gpu_ctx, w, cam, monkeypatch, name)
    assert name == "empty" or (ref["kind"] == SOLID).sum() > 0.02 * ref["kind"].size
    assert not spec.get("media") or (ref["kind"] == MEDIUM).sum() > 0.02 * ref["kind"].size


@pytest.mark.parametrize("seed", range(8))
def test_features_equal_the_oracle_on_random_worlds(gpu_ctx, monkeypatch, seed):
    """the first 8 random worlds of tests/test_host_mode.py from that test's four views"""
    rng = np.random.default_rng(1000 + seed)
    w, light = random_world(rng, n_spheres=int(rng.integers(1, 60)), n_quads=int(rng.integers(0, 12)), n_boxes=int(rng.integers(0, 3)),
                            n_media=int(rng.integers(0, 3)), with_light=bool(seed % 2))
    _, cam = host.build_scene(2, width=56, spp=1, depth=int(rng.integers(2, 20)))
    for i in range(3):
        cam.background.e[i] = float(rng.uniform(0.0, 0.8)) * (0 if light and seed % 4 == 1 else 1)
    views = [((0, 2, 9), (0, 1, 0)), ((0.3, 0.05, 0.2), (4, 0.3, 1)), ((40, 25, -60), (0, 0, 0)), (tuple(rng.uniform(-5, 5, 3) + (0, 6, 0)), tuple(rng.uniform(-2, 2, 3)))]
    solid = 0
    for k, (frm, at) in enumerate(views):
        set_view(cam, frm, at, vfov=int(rng.integers(20, 90)), defocus=float(rng.choice([0.0, 0.0, 0.8])))
        solid += (_gpu_equals_oracle(gpu_ctx, w, cam, monkeypatch, f"random world {seed} view {k}")["kind"] == SOLID).sum()
    assert solid > 0.3 * 4 * cam.image_width * cam.image_height


@pytest.mark.parametrize("name", sorted(PLACED))
def test_features_equal_the_oracle_from_placed_cameras(gpu_ctx, monkeypatch, name):
    """what each case must show is asserted on the reference in tests/test_features_oracle.py"""
    from tests import test_features_oracle as T
    w, cam = PLACED[name]()
    ref = _gpu_equals_oracle(gpu_ctx, w, cam, monkeypatch, name)
    getattr(T, "_placed_" + name)(w, cam, ref)


@pytest.mark.parametrize("nranks", [2, 3])
def test_partitioned_features_equal_the_oracle(gpu_ctx, nranks):
    world, cam = host.build_scene(9, width=120, spp=1)
    ref = oracle_features(world, cam, nthreads=16)
    gpu_ctx.upload_world(world)
    H = cam.image_height
    parts = {k: np.full(ref[k].shape, np.nan, dtype=np.float32) for k in KEYS}
    seen = []
    try:
        for rank in range(nranks):
            gpu_ctx.set_partition(rank, nranks, 8)
            out = {k: np.full(ref[k].shape, np.nan, dtype=np.float32) for k in KEYS}
            st = hip.lib().mort_hip_render_features(gpu_ctx._h, C.byref(cam), out["albedo"].ctypes.data, out["normal"].ctypes.data,
                                                    out["depth"].ctypes.data, None)
            assert st == 0
            rows = [gpu_ctx.global_row(ly) for ly in range(gpu_ctx.local_rows(H))]
            seen += rows
            for k in KEYS:
                parts[k][rows] = out[k][rows]
    finally:
        gpu_ctx.set_partition(0, 1, 8)
    assert sorted(seen) == list(range(H))
    assert_same_words(parts, ref, f"scene 9, {nranks} ranks")


@pytest.mark.parametrize("sid,width,height", [(9, 61, 35), (6, 61, 35), (9, 5, 3), (1, 5, 3), (9, 1, 1), (6, 1, 1)])
def test_ragged_frames_equal_the_oracle(gpu_ctx, monkeypatch, sid, width, height):
    world, cam = _sized(sid, width, height)
    ref = _gpu_equals_oracle(gpu_ctx, world, cam, monkeypatch, f"scene {sid} at {width}x{height}")
    assert (ref["kind"] == SOLID).any()


@pytest.mark.parametrize("sid,width,height", [(1, 1200, 675), (6, 800, 800), (9, 800, 800)])
def test_large_frames_equal_the_oracle(gpu_ctx, monkeypatch, sid, width, height):
    """sizes no other feature test reaches: many workgroups per row and per column, every pixel against the oracle"""
    world, cam = host.build_scene(sid, width=width, spp=1)
    assert (cam.image_width, cam.image_height) == (width, height)
    ref = _gpu_equals_oracle(gpu_ctx, world, cam, monkeypatch, f"scene {sid} at {width}x{height}")
    assert (ref["kind"] == SOLID).sum() > 0.5 * width * height


PARAMS = [dict(), dict(iterations=0), dict(iterations=1), dict(iterations=3, sigma_color=0.7, sigma_depth=0.5, sigma_albedo=0.3, normal_log2_power=1),
          dict(iterations=8, normal_log2_power=6)]


@pytest.mark.parametrize("W,H", [(97, 55), (5, 3), (400, 225)])
@pytest.mark.parametrize("pi", range(len(PARAMS)))
def test_denoise_matches_host(gpu_ctx, W, H, pi):
    from tests.test_denoise_host import random_inputs
    p = hip.DenoiseParams(**PARAMS[pi])
    C_, A, N, D = random_inputs(W, H, 3 * W + H)
    ref = hip.denoise_host(C_, A, N, D, params=p, nthreads=16)
    out = gpu_ctx.denoise(C_, A, N, D, params=p)
    assert (out["accum"].view(np.uint32) == ref["accum"].view(np.uint32)).all()
    assert (out["rgba"] == ref["rgba"]).all()


def test_device_paths_on_torch_tensors(gpu_ctx):
    import torch
    world, cam = host.build_scene(6, width=200, spp=4)
    W, H = cam.image_width, cam.image_height
    gpu_ctx.upload_world(world)
    gpu_ctx.rng_seed(69420, W, H)
    r = gpu_ctx.render(cam, want_accum=True)
    f = hip.render_features_host(world, cam, nthreads=16)
    dev = torch.device("cuda:0")
    alb, nrm, dep = (torch.zeros(W * H * c, dtype=torch.float32, device=dev) for c in (3, 3, 1))
    gpu_ctx.render_features_device(cam, alb, nrm, dep)
    acc = torch.from_numpy(r["accum"].reshape(-1).copy()).to(dev)
    acc_out = torch.zeros(W * H * 3, dtype=torch.float32, device=dev)
    rgba = torch.zeros(W * H * 4, dtype=torch.uint8, device=dev)
    for p in (hip.DenoiseParams(), hip.DenoiseParams(iterations=2)):
        gpu_ctx.denoise_device(W, H, acc, alb, nrm, dep, accum_out=acc_out, rgba_out=rgba, params=p)
        torch.cuda.synchronize()
        for k, t in zip(KEYS, (alb, nrm, dep)):
            assert (t.cpu().numpy().view(np.uint32) == f[k].reshape(-1).view(np.uint32)).all(), k
        ref = hip.denoise_host(r["accum"], f["albedo"], f["normal"], f["depth"], params=p, nthreads=16)
        assert (acc_out.cpu().numpy().view(np.uint32) == ref["accum"].reshape(-1).view(np.uint32)).all()
        assert (rgba.cpu().numpy() == ref["rgba"].reshape(-1)).all()


@pytest.mark.parametrize("sid,mode", [(1, hip.MODE_MEGA), (6, hip.MODE_MEGA), (6, hip.MODE_WAVE), (9, hip.MODE_WAVE)])
def test_features_and_denoise_leave_the_next_frame_alone(gpu_ctx, sid, mode):
    world, cam = host.build_scene(sid, width=128, spp=4)
    W, H = cam.image_width, cam.image_height
    gpu_ctx.upload_world(world)

    def two_frames(extra):
        gpu_ctx.rng_seed(69420, W, H)
        first = gpu_ctx.render(cam, mode=mode, want_accum=True)
        if extra:
            f = gpu_ctx.render_features(cam)
            gpu_ctx.denoise(first["accum"], f["albedo"], f["normal"], f["depth"])
        out = gpu_ctx.render(cam, mode=mode, want_accum=True, want_segments=mode == hip.MODE_MEGA)
        out["states"] = gpu_ctx.rng_store(W, H)
        return out

    a, b = two_frames(False), two_frames(True)
    assert (a["rgba"] == b["rgba"]).all()
    assert (a["accum"].view(np.uint32) == b["accum"].view(np.uint32)).all()
    assert (a["states"] == b["states"]).all()
    assert a["stats"]["segments"] == b["stats"]["segments"]
    if a["segments_px"] is not None:
        assert (a["segments_px"] == b["segments_px"]).all()


@pytest.mark.parametrize("sid,limit", [(1, 0.9), (3, 1.2), (6, 0.6)])
def test_denoise_quality_on_the_gpu(gpu_ctx, sid, limit):
    def g(a):
        return np.sqrt(np.clip(a, 0, 0.999 ** 2))
    world, cam = host.build_scene(sid, width=400, spp=4)
    w2, cam2 = host.build_scene(sid, width=400, spp=1024)
    gpu_ctx.upload_world(world)
    gpu_ctx.rng_seed(69420, cam.image_width, cam.image_height)
    noisy = gpu_ctx.render(cam, want_accum=True)["accum"]
    f = gpu_ctx.render_features(cam)
    den = gpu_ctx.denoise(noisy, f["albedo"], f["normal"], f["depth"])["accum"]
    gpu_ctx.upload_world(w2)
    gpu_ctx.rng_seed(69420, cam2.image_width, cam2.image_height)
    ref = gpu_ctx.render(cam2, want_accum=True)["accum"]
    e0 = np.sqrt(np.mean((g(noisy) - g(ref)) ** 2))
    e1 = np.sqrt(np.mean((g(den) - g(ref)) ** 2))
    print(f"scene {sid} 400 px, 4 spp vs 1024 spp: noisy RMSE {e0:.4f}, denoised {e1:.4f}, ratio {e1 / e0:.3f}")
    assert e1 <= limit * e0, f"ratio {e1 / e0:.3f}"


def test_features_need_a_world_but_no_rng():
    world, cam = host.build_scene(2, width=64, spp=1)
    with hip.Context(0) as ctx:
        with pytest.raises(hip.MortHipError) as e:
            ctx.render_features(cam)
        assert e.value.status == -4  # MORT_ERR_NO_WORLD
        ctx.upload_world(world)
        _same_features(ctx.render_features(cam), hip.render_features_host(world, cam, nthreads=16), "before any rng_seed")
