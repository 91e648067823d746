"""Parity tests proper: the HIP render path, called through the C ABI of libmort_hip.so, against
the CPU oracle on the same seeded inputs.  Bar: BIT-EXACT -- uchar4 image, fp32 accumulators
(compared as raw bits), per-pixel segment counts and final XORWOW words.  Every kernel is
compiled with -ffp-contract=off and uses include/mort_math.h, as the oracle does, so there is no
tolerance to state (the north_star's "stated ULP tolerance" is 0 ULP against the oracle; against
the CUDA reference: tests/test_gpu_reference_pin.py and DESIGN.md 2)."""
import os

import numpy as np
import pytest

from mort_amd import host, hip, structs as S
from tests.golden.make_golden import CASES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "oracle_golden.npz"))


def render_gpu(ctx, world, cam, seed=S.DEFAULT_SEED, states=None, oracle=None):
    ctx.set_partition(0, 1, 8)
    ctx.upload_world(world)
    W, H = cam.image_width, cam.image_height
    if states is None:
        ctx.rng_seed(seed, W, H)
    else:
        ctx.rng_load(states, W, H)
    out = ctx.render(cam, want_accum=True, want_segments=True)
    out["states"] = ctx.rng_store(W, H, oracle.STATE_DTYPE) if oracle else None
    return out


def assert_same(out, ref):
    assert (out["rgba"] == ref["rgba"]).all(), "uchar4 image differs"
    assert (out["accum"].view(np.uint32) == ref["accum"].view(np.uint32)).all(), "fp32 accumulators differ (bitwise)"
    assert (out["segments_px"] == ref["segments_px"]).all(), "per-pixel segment counts differ"
    assert out["stats"]["segments"] == ref["segments"] and out["stats"]["rng_draws"] == ref["rng_draws"]
    if out.get("states") is not None:
        assert (out["states"]["d"] == ref["states"]["d"]).all() and (out["states"]["v"] == ref["states"]["v"]).all(), "final RNG states differ"


def test_seeding_matches_oracle(gpu_ctx, oracle):
    for W, H in ((200, 112), (37, 11), (1200, 9)):
        gpu_ctx.set_partition(0, 1, 8)
        gpu_ctx.rng_seed(69420, W, H)
        got = gpu_ctx.rng_store(W, H, oracle.STATE_DTYPE)
        want = oracle.seed_states(69420, W, H)
        assert (got["d"] == want["d"]).all() and (got["v"] == want["v"]).all()
        assert (got["bf"] == 0).all() and (got["bed"] == 0).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_scene_matches_oracle_and_golden(gpu_ctx, oracle, name):
    """Every scene family of the reference's catalogue (BVH, brute force, instances, media,
    lights/MIS, checker / image / noise textures), HIP vs oracle vs the committed golden vectors."""
    sid, width, spp, depth = CASES[name]
    world, cam = host.build_scene(sid, width=width, spp=spp, depth=depth)
    ref = oracle.render(world, cam, nthreads=8)
    out = render_gpu(gpu_ctx, world, cam, oracle=oracle)
    assert_same(out, ref)
    assert (out["rgba"] == GOLD[name + "_rgba"]).all()
    assert (out["accum"].view(np.uint32) == GOLD[name + "_accum"].view(np.uint32)).all()
    # scenes 1 / 10: BVH megakernel; final scene: unified-tree megakernel (both stage the scene in LDS); small worlds: one lane per pixel
    want = "mega_bvh_kernel" if sid in (1, 10) else "mega_gen_kernel" if sid in (8, 9) else "mega_kernel"
    assert out["stats"]["kernel_name"].startswith(want)
    assert out["stats"]["scene_in_lds"] == (0 if want == "mega_kernel" else 1)


def test_generic_kernel_on_bvh_scene(gpu_ctx, oracle, monkeypatch):
    """Scene 1 through the general (non-LDS) kernel gives the same bits as the LDS state-machine kernel."""
    world, cam = host.build_scene(1, width=160, spp=9)
    ref = oracle.render(world, cam, nthreads=8)
    monkeypatch.setenv("MORT_FORCE_GENERIC", "1")
    out = render_gpu(gpu_ctx, world, cam, oracle=oracle)
    assert out["stats"]["scene_in_lds"] == 0
    assert_same(out, ref)


@pytest.mark.parametrize("sid,width,spp,depth", [(9, 120, 9, None), (8, 72, 4, None), (8, 64, 4, 6)])
def test_final_scene_tree_and_scan_equal_oracle(oracle, monkeypatch, sid, width, spp, depth):
    """final_scene scans 2401 quads + a 1000-sphere list per ray in the reference.  The unified-tree kernel and the
    one-lane-per-pixel kernel (which scans like the reference) must both give the oracle's bits.  (Round 1 walked
    per-run trees with fixed pads inside the scan; at 800x800x100 spp one ray in 3.6e8 went wrong -- a grazing hit on a
    small sphere seen from far away -- and that code is gone: scene_compile.h build_unified sizes its pads for it.)"""
    world, cam = host.build_scene(sid, width=width, spp=spp, depth=depth)
    ref = oracle.render(world, cam, nthreads=16)
    for no_gen in (False, True):
        if no_gen:
            monkeypatch.setenv("MORT_NO_GEN", "1")
        else:
            monkeypatch.delenv("MORT_NO_GEN", raising=False)
        ctx = hip.Context(0)
        try:
            out = render_gpu(ctx, world, cam, oracle=oracle)
            assert out["stats"]["kernel_name"].startswith("mega_kernel" if no_gen else "mega_gen_kernel")
            assert_same(out, ref)
        finally:
            ctx.close()


@pytest.mark.parametrize("depth", [0, 1, 2, 50])
def test_bounce_limits(gpu_ctx, oracle, depth):
    world, cam = host.build_scene(1, width=96, spp=4, depth=depth)
    assert_same(render_gpu(gpu_ctx, world, cam, oracle=oracle), oracle.render(world, cam, nthreads=8))


def test_ragged_sizes_and_odd_spp(gpu_ctx, oracle):
    """Widths/heights that are not multiples of the 8x8 tile, spp that is not a square (500 -> 484 logic)."""
    for width, aspect, spp in ((61, 1.7, 5), (8, 1.0, 1), (130, 3.3, 7), (9, 0.3, 2)):
        world, cam = host.build_scene(1, width=width, spp=spp, aspect=aspect)
        assert_same(render_gpu(gpu_ctx, world, cam, oracle=oracle), oracle.render(world, cam, nthreads=8))


def test_frames_continue_the_streams(gpu_ctx, oracle):
    """RNG states persist from frame to frame (mort.cu:93-120): frame 2 continues where frame 1 stopped."""
    world, cam = host.build_scene(1, width=96, spp=4)
    gpu_ctx.set_partition(0, 1, 8)
    gpu_ctx.upload_world(world)
    gpu_ctx.rng_seed(S.DEFAULT_SEED, cam.image_width, cam.image_height)
    f1 = gpu_ctx.render(cam)
    f2 = gpu_ctx.render(cam)
    r1 = oracle.render(world, cam, nthreads=8)
    r2 = oracle.render(world, cam, states=r1["states"], nthreads=8)
    assert (f1["rgba"] == r1["rgba"]).all() and (f2["rgba"] == r2["rgba"]).all()
    assert not (f1["rgba"] == f2["rgba"]).all()


def test_state_load_store_round_trip(gpu_ctx, oracle):
    """The 48-byte curandStateXORWOW array is an ABI input/output: a dump from another run pins the streams."""
    world, cam = host.build_scene(10, width=120, spp=1)
    W, H = cam.image_width, cam.image_height
    states = oracle.seed_states(12345, W, H)
    ref = oracle.render(world, cam, states=states.copy(), nthreads=8)
    out = render_gpu(gpu_ctx, world, cam, states=states, oracle=oracle)
    assert_same(out, ref)


@pytest.mark.parametrize("nranks,rpb", [(2, 8), (4, 8), (8, 8), (3, 16)])
def test_partition_invariance(gpu_ctx, oracle, nranks, rpb):
    """Image rows split over N ranks (run one after another on the one GPU) compose to exactly the
    single-rank image: per-pixel streams make the partition invisible."""
    world, cam = host.build_scene(1, width=120, spp=4)
    W, H = cam.image_width, cam.image_height
    ref = oracle.render(world, cam, nthreads=8)
    rgba = np.zeros((H, W, 4), np.uint8)
    accum = np.zeros((H, W, 3), np.float32)
    seg = 0
    owned = np.zeros(H, int)
    for r in range(nranks):
        gpu_ctx.set_partition(r, nranks, rpb)
        gpu_ctx.upload_world(world)
        gpu_ctx.rng_seed(S.DEFAULT_SEED, W, H)
        out = gpu_ctx.render(cam)
        lr = gpu_ctx.local_rows(H)
        rows = [gpu_ctx.global_row(l) for l in range(lr)]
        owned[rows] += 1
        rgba[rows] = out["rgba"][rows]
        accum[rows] = out["accum"][rows]
        seg += out["stats"]["segments"]
        others = np.setdiff1d(np.arange(H), rows)
        assert (out["rgba"][others] == 0).all()  # rows not owned are left untouched
    gpu_ctx.set_partition(0, 1, 8)
    assert (owned == 1).all() and seg == ref["segments"]
    assert (rgba == ref["rgba"]).all() and (accum.view(np.uint32) == ref["accum"].view(np.uint32)).all()


WAVE_CASES = [(1, 200, 4, None), (10, 160, 1, None), (1, 96, 9, 3), (1, 61, 5, 1), (1, 130, 16, 50)]


@pytest.mark.parametrize("sid,width,spp,depth", WAVE_CASES)
def test_wavefront_mode_matches_oracle(gpu_ctx, oracle, sid, width, spp, depth):
    """MORT_MODE_WAVE (queued pipeline, wave_bvh.h) produces the same bits as the oracle and the megakernel."""
    world, cam = host.build_scene(sid, width=width, spp=spp, depth=depth)
    ref = oracle.render(world, cam, nthreads=8)
    gpu_ctx.set_partition(0, 1, 8)
    gpu_ctx.upload_world(world)
    gpu_ctx.rng_seed(S.DEFAULT_SEED, cam.image_width, cam.image_height)
    out = gpu_ctx.render(cam, mode=hip.MODE_WAVE, want_accum=True, want_segments=True)
    out["states"] = gpu_ctx.rng_store(cam.image_width, cam.image_height, oracle.STATE_DTYPE)
    assert_same(out, ref)


def test_wavefront_mode_rejects_unsupported_worlds(gpu_ctx):
    """A world whose list is scanned after a medium has no unified tree (order matters): megakernel only."""
    from tests.worlds import FLAT_WORLDS, flat_world, flat_camera
    spec = FLAT_WORLDS["media_then_list"]
    w, _ = flat_world(spec["prims"], media=spec["media"], late_list=True)
    cam = flat_camera(spp=1, width=32)
    gpu_ctx.set_partition(0, 1, 8)
    gpu_ctx.upload_world(w)
    gpu_ctx.rng_seed(1, cam.image_width, cam.image_height)
    with pytest.raises(hip.MortHipError) as e:
        gpu_ctx.render(cam, mode=hip.MODE_WAVE)
    assert e.value.status == -6


@pytest.mark.parametrize("env", [
    {"MORT_CHAIN_BOUND": "0"}, {"MORT_CHAIN_BOUND": "1"},
    {"MORT_CHAIN_BOUND": "1", "MORT_SPREAD_SHIFT": "3"}, {"MORT_CHAIN_BOUND": "0", "MORT_SPREAD_SHIFT": "0"},
    {"MORT_NO_TILE_ORDER": "1"}, {"MORT_THRESHOLDS": "2,2,2"}, {"MORT_THRESHOLDS": "64,64,64"},
    {"MORT_FAST_BLOCK_SIZE": "256"}, {"MORT_FAST_BLOCK_SIZE": "512", "MORT_CHAIN_BOUND": "1"}, {"MORT_FAST_BLOCK_SIZE": "1024"},
    {"MORT_BVH_DRAIN": "0"}, {"MORT_BVH_DRAIN": "2", "MORT_CHAIN_BOUND": "1"},
])
def test_scheduling_choices_do_not_reach_the_pixels(gpu_ctx, oracle, monkeypatch, env):
    """Which lanes take which pixels, in which order, in which batch sizes and workgroup shapes (cost-ordered tiles,
    spread fetches, drain mode, thresholds) must not change a bit of the result: Scene 1 at 400x225, two frames
    (the second one ordered by the first one's costs), against the oracle."""
    world, cam = host.build_scene(1, width=400, spp=9)
    ref1 = oracle.render(world, cam, nthreads=8)
    ref2 = oracle.render(world, cam, nthreads=8, states=ref1["states"].copy())
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out1 = render_gpu(gpu_ctx, world, cam, oracle=oracle)
    assert_same(out1, ref1)
    out2 = gpu_ctx.render(cam, want_accum=True, want_segments=True)  # streams continue; tiles now ordered by frame 1
    out2["states"] = gpu_ctx.rng_store(cam.image_width, cam.image_height, oracle.STATE_DTYPE)
    assert_same(out2, ref2)


@pytest.mark.parametrize("sid", [1, 10])
def test_other_viewpoints(gpu_ctx, oracle, sid):
    """The built-in cameras look at the BVH scenes from one side only.  Other ray populations for the own-tree walk
    (DESIGN.md 4.2): cameras inside the sphere field, at ground level, under the ground, looking straight up / down /
    along an axis (direction components that are exactly zero take the reference walk), zoomed far out, with and
    without defocus -- each against the oracle, bit for bit."""
    from mort_amd.host import lib as host_lib
    import ctypes as C
    world, cam = host.build_scene(sid, width=120, spp=4)
    rng = np.random.default_rng(7 + sid)
    views = [((0.5, 0.3, 0.5), (3.0, 0.3, 0.2)), ((0.0, 0.21, 2.0), (0.0, 0.21, -5.0)), ((2.0, -3.0, 1.0), (0.0, 1.0, 0.0)),
             ((0.0, 30.0, 0.0), (0.0, 0.0, 0.001)), ((0.0, 0.5, 0.0), (0.0, 10.0, 0.0001)), ((5.0, 1.0, 0.0), (-5.0, 1.0, 0.0)),
             ((300.0, 120.0, 200.0), (0.0, 0.0, 0.0)), ((0.0, 1.0, 0.0), (4.0, 1.0, 0.0))]
    views += [(tuple(rng.uniform(-9, 9, 3) * (1, 0.2, 1) + (0, 0.5, 0)), tuple(rng.uniform(-6, 6, 3) * (1, 0.1, 1))) for _ in range(4)]
    for k, (frm, at) in enumerate(views):
        for i in range(3):
            cam.lookfrom.e[i] = frm[i]; cam.lookat.e[i] = at[i]
        cam.defocus_angle = 0.0 if k % 2 else 0.6
        cam.vfov = 20 if k % 3 else 70
        host_lib().mort_camera_initialize(C.byref(cam))
        ref = oracle.render(world, cam, nthreads=8)
        out = render_gpu(gpu_ctx, world, cam, oracle=oracle)
        assert_same(out, ref)


from tests.worlds import custom_bvh_world as _custom_bvh_world, BVH_WORLDS


@pytest.mark.parametrize("name", ["one", "two", "three", "coincident", "concentric_glass", "every_material"])
def test_small_and_awkward_bvh_worlds(gpu_ctx, oracle, name):
    """BVH-of-spheres worlds the built-in scenes do not contain: one to three spheres (no own tree below two leaf
    nodes: generic kernel), the same sphere several times (equal t: ties -> reference walk), concentric glass shells,
    and every material / texture kind on a sphere (isotropic, emissive, checker, Perlin noise, image)."""
    import ctypes as C
    worlds = BVH_WORLDS
    w = _custom_bvh_world(worlds[name])
    _, cam = host.build_scene(1, width=144, spp=9, depth=12)
    for i, v in enumerate((0.0, 0.6, 1.5)): cam.lookfrom.e[i] = v
    for i, v in enumerate((0.0, 0.0, -1.0)): cam.lookat.e[i] = v
    cam.vfov = 60; cam.defocus_angle = 0.0
    host.lib().mort_camera_initialize(C.byref(cam))
    ref = oracle.render(w, cam, nthreads=8)
    out = render_gpu(gpu_ctx, w, cam, oracle=oracle)
    assert_same(out, ref)
    if name == "coincident":
        assert out["stats"]["scene_in_lds"] == 1 and out["stats"]["reference_walks"] > 0


def test_reference_walk_is_rare_and_counted(gpu_ctx, oracle):
    """The BVH megakernel re-traces a ray with the reference's own walk when it cannot prove its winner
    (DESIGN.md 4.2): a handful per million segments, reported in the stats."""
    world, cam = host.build_scene(1, width=400, spp=16)
    out = render_gpu(gpu_ctx, world, cam, oracle=oracle)
    assert 0 <= out["stats"]["reference_walks"] < out["stats"]["segments"] // 10000
    assert_same(out, oracle.render(world, cam, nthreads=8))


def test_full_geometry_low_spp(gpu_ctx, oracle):
    """The headline geometry (Scene 1, 1200x675) at 4 spp against the oracle, bit for bit."""
    world, cam = host.build_scene(1, spp=4)
    assert (cam.image_width, cam.image_height) == (1200, 675)
    assert_same(render_gpu(gpu_ctx, world, cam, oracle=oracle), oracle.render(world, cam, nthreads=16))


def test_headline_config_matches_oracle_bit_for_bit(gpu_ctx, oracle):
    """BASELINE config 2 in full (Scene 1 1200x675, 500 spp nominal = 484 effective, depth 20): 392 M samples, 1.02 G
    segments, every byte of the image, every accumulator bit, every per-pixel segment count and final RNG word
    against the CPU oracle (about half a minute on the box's 16 host threads)."""
    world, cam = host.build_scene(1, spp=500)
    ref = oracle.render(world, cam, nthreads=min(len(os.sched_getaffinity(0)), 32))
    out = render_gpu(gpu_ctx, world, cam, oracle=oracle)
    assert out["stats"]["eff_samples"] == 1200 * 675 * 484
    assert_same(out, ref)


def test_headline_config_properties(gpu_ctx, oracle):
    """BASELINE config 2 in full (1200x675, 500 spp nominal = 484 effective): too big for the oracle in a
    test, so size-independent properties: run-to-run determinism, partition invariance of the segment
    count, alpha = 255, sky rows cost exactly 484 segments per pixel."""
    world, cam = host.build_scene(1, spp=500)
    assert host.effective_spp(cam) == 484
    a = render_gpu(gpu_ctx, world, cam, oracle=oracle)
    b = render_gpu(gpu_ctx, world, cam, oracle=oracle)
    assert (a["rgba"] == b["rgba"]).all() and (a["accum"].view(np.uint32) == b["accum"].view(np.uint32)).all()
    assert (a["states"]["v"] == b["states"]["v"]).all() and a["stats"]["segments"] == b["stats"]["segments"]
    assert (a["rgba"][..., 3] == 255).all()
    assert a["stats"]["eff_samples"] == 1200 * 675 * 484 and a["stats"]["segments"] == int(a["segments_px"].sum(dtype=np.uint64))
    assert a["segments_px"].min() == 484
    total = 0
    for r in range(2):
        gpu_ctx.set_partition(r, 2, 8)
        gpu_ctx.upload_world(world)
        gpu_ctx.rng_seed(S.DEFAULT_SEED, 1200, 675)
        total += gpu_ctx.render(cam, want_accum=False)["stats"]["segments"]
    gpu_ctx.set_partition(0, 1, 8)
    assert total == a["stats"]["segments"]


def test_error_paths(oracle):
    """Error behaviour of the ABI (the reference print-and-exits; here: status codes)."""
    ctx = hip.Context(0)
    try:
        world, cam = host.build_scene(1, width=32, spp=1)
        with pytest.raises(hip.MortHipError) as e:
            ctx.render(cam)
        assert e.value.status == -4  # MORT_ERR_NO_WORLD
        ctx.upload_world(world)
        with pytest.raises(hip.MortHipError) as e:
            ctx.render(cam)
        assert e.value.status == -5  # MORT_ERR_NO_RNG
        ctx.rng_seed(1, cam.image_width, cam.image_height)
        ctx.render(cam)
        with pytest.raises(hip.MortHipError) as e:
            ctx.render(cam, mode=7)
        assert e.value.status == -1  # unknown mode
        _, deep = host.build_scene(1, width=32, spp=1, depth=S.MAX_BOUNCE_LIMIT + 1)
        with pytest.raises(hip.MortHipError) as e:
            ctx.render(deep)
        assert e.value.status == -7  # MORT_ERR_CAPACITY
        _, other = host.build_scene(1, width=40, spp=1)
        with pytest.raises(hip.MortHipError) as e:
            ctx.render(other)  # states were seeded for another image size
        assert e.value.status == -5
        bad, cam6 = host.build_scene(6, width=32, spp=1)
        bad.c.objs.host_quad[1].mat_idx = 999  # a material index the tables do not have
        with pytest.raises(hip.MortHipError) as e:
            ctx.upload_world(bad)
        assert e.value.status == -1
        with pytest.raises(hip.MortHipError):
            ctx.set_partition(2, 2, 8)
        with pytest.raises(hip.MortHipError):
            ctx.set_partition(0, 1, 12)
    finally:
        ctx.close()


def test_empty_world_renders_background(gpu_ctx, oracle):
    world, cam = host.build_scene(11, width=64, spp=1)  # unknown id -> empty world (mort.cu:649-689 has no default)
    out = render_gpu(gpu_ctx, world, cam, oracle=oracle)
    assert_same(out, oracle.render(world, cam))
    assert out["stats"]["segments"] == cam.image_width * cam.image_height


def test_smoke_entry():
    import __graft_entry__ as g
    g.smoke()


def test_render_device_after_smaller_render_with_segments(gpu_ctx, oracle):
    """a per-pixel segment buffer left by an earlier, smaller mort_hip_render must not be written by a
    later mort_hip_render_device on a bigger frame (it is an internal argument now, never taken from the context)."""
    import torch
    world, cam_s = host.build_scene(1, width=64, spp=1)
    gpu_ctx.set_partition(0, 1, 8)
    gpu_ctx.upload_world(world)
    gpu_ctx.rng_seed(S.DEFAULT_SEED, cam_s.image_width, cam_s.image_height)
    gpu_ctx.render(cam_s, want_segments=True)
    world_b, cam_b = host.build_scene(1, width=400, spp=4)
    gpu_ctx.upload_world(world_b)
    W, H = cam_b.image_width, cam_b.image_height
    gpu_ctx.rng_seed(S.DEFAULT_SEED, W, H)
    tile = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    guard = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")  # neighbours in the caching allocator stay zero
    torch.cuda.synchronize()
    st = gpu_ctx.render_device(cam_b, tile.data_ptr(), 0, 0, sync=True)
    ref = oracle.render(world_b, cam_b, nthreads=8)
    assert (tile.cpu().numpy() == ref["rgba"]).all() and st["segments"] == ref["segments"]
    assert int(guard.sum().item()) == 0


def test_async_render_device_then_store(gpu_ctx, oracle):
    """render_device(stats=NULL) on a caller stream returns without waiting (the tile order is sorted on the device);
    rng_store afterwards waits for that stream (stream ownership) and sees the finished states."""
    import torch
    world, cam = host.build_scene(1, width=320, spp=9)
    W, H = cam.image_width, cam.image_height
    gpu_ctx.set_partition(0, 1, 8)
    gpu_ctx.upload_world(world)
    gpu_ctx.rng_seed(S.DEFAULT_SEED, W, H)
    stream = torch.cuda.Stream("cuda:0")
    tile = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    gpu_ctx.render_device(cam, tile.data_ptr(), 0, stream.cuda_stream, sync=False)
    got = gpu_ctx.rng_store(W, H, oracle.STATE_DTYPE)  # must wait for the caller's stream
    ref = oracle.render(world, cam, nthreads=8)
    assert (got["d"] == ref["states"]["d"]).all() and (got["v"] == ref["states"]["v"]).all()
    stream.synchronize()
    assert (tile.cpu().numpy() == ref["rgba"]).all()
    # second frame of the same view takes the cost-ordered path with history; a moved camera invalidates it
    gpu_ctx.render_device(cam, tile.data_ptr(), 0, stream.cuda_stream, sync=False)
    world2, cam2 = host.build_scene(10, width=320, spp=4)
    gpu_ctx.upload_world(world2)  # waits for the frame in flight, drops the cost history
    gpu_ctx.rng_seed(S.DEFAULT_SEED, cam2.image_width, cam2.image_height)
    tile2 = torch.zeros((cam2.image_height, cam2.image_width, 4), dtype=torch.uint8, device="cuda:0")
    gpu_ctx.render_device(cam2, tile2.data_ptr(), 0, stream.cuda_stream, sync=True)
    assert (tile2.cpu().numpy() == oracle.render(world2, cam2, nthreads=8)["rgba"]).all()


def test_right_to_left_host_profile(gpu_ctx, oracle):
    """The reference leaves the evaluation order of sibling random_float() arguments to the compiler (mort.cu:147,152,164;
    vec3.cuh:63-69): the host layer's right-to-left profile builds a different Scene 1 / final scene; the HIP path must
    match the oracle on those worlds too."""
    for sid, width, spp in ((1, 160, 4), (9, 64, 4)):
        world, cam = host.build_scene(sid, width=width, spp=spp, args_rtl=1)
        w0, _ = host.build_scene(sid, width=width, spp=spp)
        ref = oracle.render(world, cam, nthreads=8)
        assert not (ref["rgba"] == oracle.render(w0, cam, nthreads=8)["rgba"]).all()  # it IS a different world
        assert_same(render_gpu(gpu_ctx, world, cam, oracle=oracle), ref)
