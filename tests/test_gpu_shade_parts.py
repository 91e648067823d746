"""The parts of the BVH megakernel's shade step against the oracle, bit for bit -- image, accumulators, per-pixel segment counts, final
RNG words, and the totals `segments` and `rng_draws`:

 - Scenes 1 and 10 at 96x54, 16 spp, bounce limits 1, 2, 5 and 50, on 1024-, 768- and 256-thread workgroups: the bounce stack keeps
   between four and twelve levels in LDS and the rest in HBM (mega_bvh.h: LDS levels through ds_read / ds_write, HBM levels through
   a global-address pointer), so the deep paths of the limit-50 frames cross that boundary on the wide workgroups and the shallow
   limits never reach it.  Which frames cross is checked on the CPU, against the level count the 1024-thread launch really keeps in
   LDS (mort_hip_debug_bvh_lds_levels): Scene 1 (four levels) has pixels whose segment count changes when the limit drops from 50 to
   5, and to 13 -- deeper than ANY LDS part.  Scene 10 (eight levels) NEVER crosses, and no bounce limit makes it: its paths end by
   themselves within five segments (the limit-50 frame equals the limit-5 frame), which is asserted, so its cases cover the LDS
   levels alone.
 - Scene 2 (two checker spheres) and a world of nested checkers, checkers with a noise child and a checkered light, through the kernel
   the library picks and through the wavefront pipeline: every texture path of the lookup.
 - two frames of Scene 1 in a row: the second starts from stored states, not from the seed.
 - a two-way partition of Scene 1."""
import ctypes as C

import numpy as np
import pytest

from mort_amd import host, hip, structs as S
from tests.checker_worlds import nested_checker_world

pytestmark = pytest.mark.gpu

LDS_LEVELS_MAX = 12  # world_images.h state_lds_levels: the launch keeps at most twelve bounce-stack levels in LDS
_REF = {}


def _scene(sid, depth):
    return host.build_scene(sid, width=96, spp=16, depth=depth)


def _ref(oracle, sid, depth):
    """the oracle's frame, computed once per (scene, limit) and shared by the block sizes"""
    key = (sid, depth)
    if key not in _REF:
        world, cam = _scene(sid, depth)
        _REF[key] = oracle.render(world, cam, nthreads=8)
    return _REF[key]


def _same(out, ref):
    assert (out["rgba"] == ref["rgba"]).all(), "uchar4 image differs"
    assert (out["accum"].view(np.uint32) == ref["accum"].view(np.uint32)).all(), "fp32 accumulators differ (bitwise)"
    assert (out["segments_px"] == ref["segments_px"]).all(), "per-pixel segment counts differ"
    assert out["stats"]["segments"] == ref["segments"], (out["stats"]["segments"], ref["segments"])
    assert out["stats"]["rng_draws"] == ref["rng_draws"], (out["stats"]["rng_draws"], ref["rng_draws"])
    assert (out["states"]["d"] == ref["states"]["d"]).all() and (out["states"]["v"] == ref["states"]["v"]).all(), "final RNG states differ"


def _render(ctx, oracle, world, cam, mode=hip.MODE_MEGA, seed=True):
    W, H = cam.image_width, cam.image_height
    if seed:
        ctx.set_partition(0, 1, 8)
        ctx.upload_world(world)
        ctx.rng_seed(S.DEFAULT_SEED, W, H)
    out = ctx.render(cam, mode=mode, want_accum=True, want_segments=True)
    out["states"] = ctx.rng_store(W, H, oracle.STATE_DTYPE)
    return out


def _lds_levels_1024(world):
    """the bounce-stack levels a 1024-thread launch of mega_bvh_kernel keeps in LDS beside the world's image (host only)"""
    fn = hip.lib().mort_hip_debug_bvh_lds_levels
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    info = (C.c_int * 4)()
    assert fn(C.cast(world.ptr, C.c_void_p), info) == 0
    assert info[0] > 0
    return info[1]


def _pixels_cut_by_limit(oracle, sid, limit):
    """Pixels of the limit-50 frame holding a path that a bounce limit of `limit` cuts short: such a path has stored bounce level
    limit - 1, the first one past an LDS part of that many levels; the pixel's stream, and with it its segment count, then differs."""
    deep = _ref(oracle, sid, 50)
    cut = _ref(oracle, sid, limit)
    return int((deep["segments_px"] != cut["segments_px"]).sum())


def test_which_limit_50_frames_cross_the_lds_part_at_1024_threads(oracle):
    """Not a GPU check by itself: it makes the limit-50 cases below mean what the docstring says."""
    dl1, dl10 = _lds_levels_1024(_scene(1, 50)[0]), _lds_levels_1024(_scene(10, 50)[0])
    assert 1 <= dl1 <= LDS_LEVELS_MAX and 1 <= dl10 <= LDS_LEVELS_MAX
    at_dl, at_max = _pixels_cut_by_limit(oracle, 1, dl1 + 1), _pixels_cut_by_limit(oracle, 1, LDS_LEVELS_MAX + 1)
    print(f"Scene 1: {dl1} LDS levels at 1024 threads; {at_dl} pixels hold a path past them, {at_max} past {LDS_LEVELS_MAX} levels")
    assert at_dl > 0 and at_max > 0
    # Scene 10: no path is longer than five segments whatever the limit, so it cannot be made to cross; asserted, not assumed
    s10 = _pixels_cut_by_limit(oracle, 10, dl10 + 1)
    print(f"Scene 10: {dl10} LDS levels at 1024 threads; {s10} pixels hold a path past them; limit 5 against 50: {_pixels_cut_by_limit(oracle, 10, 5)}")
    assert dl10 >= 5 and s10 == 0 and _pixels_cut_by_limit(oracle, 10, 5) == 0
    assert (_ref(oracle, 10, 50)["segments_px"] != _ref(oracle, 10, 2)["segments_px"]).any()  # but its frames do bounce


@pytest.mark.parametrize("block", [1024, 768, 256])
@pytest.mark.parametrize("depth", [1, 2, 5, 50])
@pytest.mark.parametrize("sid", [1, 10])
def test_bvh_scenes_by_block_size_and_bounce_limit(gpu_ctx, oracle, monkeypatch, sid, depth, block):
    monkeypatch.setenv("MORT_FAST_BLOCK_SIZE", str(block))
    world, cam = _scene(sid, depth)
    out = _render(gpu_ctx, oracle, world, cam)
    assert out["stats"]["kernel_name"].startswith(f"mega_bvh_kernel<{block},"), out["stats"]["kernel_name"]
    _same(out, _ref(oracle, sid, depth))


@pytest.mark.parametrize("which", ["scene2", "nested"])
def test_checker_worlds_in_both_pipelines(gpu_ctx, oracle, which):
    world, cam = host.build_scene(2, width=64, spp=4) if which == "scene2" else nested_checker_world()
    assert (cam.image_width, cam.image_height) == (64, 36)
    ref = oracle.render(world, cam, nthreads=8)
    assert len(np.unique(ref["rgba"].reshape(-1, 4), axis=0)) > 50  # the frame shows something
    for mode in (hip.MODE_MEGA, hip.MODE_WAVE):
        _same(_render(gpu_ctx, oracle, world, cam, mode=mode), ref)


def test_second_frame_continues_from_stored_states(gpu_ctx, oracle):
    world, cam = _scene(1, 50)
    r1 = _ref(oracle, 1, 50)
    r2 = oracle.render(world, cam, states=r1["states"].copy(), nthreads=8)
    assert (r1["states"]["d"] != oracle.seed_states(S.DEFAULT_SEED, cam.image_width, cam.image_height)["d"]).all()
    _same(_render(gpu_ctx, oracle, world, cam), r1)
    _same(_render(gpu_ctx, oracle, world, cam, seed=False), r2)


def test_two_way_partition(gpu_ctx, oracle):
    world, cam = _scene(1, 50)
    ref = _ref(oracle, 1, 50)
    W, H = cam.image_width, cam.image_height
    rgba = np.zeros((H, W, 4), np.uint8); accum = np.zeros((H, W, 3), np.float32); segpx = np.zeros((H, W), np.uint32)
    d = np.zeros((H, W), np.uint32)
    seg = draws = 0
    try:
        for r in range(2):
            gpu_ctx.set_partition(r, 2, 8)
            gpu_ctx.upload_world(world)
            gpu_ctx.rng_seed(S.DEFAULT_SEED, W, H)
            out = gpu_ctx.render(cam, want_accum=True, want_segments=True)
            st = gpu_ctx.rng_store(W, H, oracle.STATE_DTYPE)
            rows = [gpu_ctx.global_row(l) for l in range(gpu_ctx.local_rows(H))]
            rgba[rows] = out["rgba"][rows]; accum[rows] = out["accum"][rows]; segpx[rows] = out["segments_px"].reshape(H, W)[rows]
            d[rows] = st["d"].reshape(H, W)[rows]
            seg += out["stats"]["segments"]; draws += out["stats"]["rng_draws"]
    finally:
        gpu_ctx.set_partition(0, 1, 8)
    assert (rgba == ref["rgba"]).all() and (accum.view(np.uint32) == ref["accum"].view(np.uint32)).all()
    assert (segpx == ref["segments_px"].reshape(H, W)).all() and (d == ref["states"]["d"].reshape(H, W)).all()
    assert seg == ref["segments"] and draws == ref["rng_draws"]
