"""The BVH megakernel's bounce stack as a ring (mega_bvh.h): entries are indexed by STORED levels (a dielectric level takes no
index), the newest DL of them live in LDS as a ring, and pushing entry n >= DL first moves entry n - DL to HBM; the unwind reads the
ring newest first while the HBM entries are already requested.  Everything here is compared with the oracle bit for bit -- image,
accumulators, per-pixel segment counts, final RNG words, and the totals `segments` and `rng_draws`:

 - ring boundaries: Scene 1 at 96x54, 16 spp, bounce limits 1 ... 14, 25, 26 and 50 (and 15 ... 23 by twos) on workgroups of 1024, 768, 512, 384 and 256
   threads.  A launch keeps between one and twelve entries in LDS; for every ring size DL from 2 to 12 the limits hold DL (the ring
   exactly full), DL + 1 (the first eviction), DL + 2 (the second) and 2 DL + 1 (the first wrap of the evicting cursor), which a host
   check below re-derives together with the fact that the frames really hold paths that reach each of those limits;
 - an enclosed world (a Lambertian shell around the camera, no glass): every path runs to the limit, so stored entries = bounce index =
   limit, at limits DL, DL + 1 and 2 DL + 1 -- once black (nothing emits) and once with a small light inside, so that the unwound
   values are not all zero;
 - a glass shell around Lambertian spheres: paths whose deepest level is an identity, at the limit too;
 - a second frame on one context, a two-way partition, and the first frame after an upload, which runs the one-sample cost probe (the
   kernel's PROBE variant) before it: the probe's tile costs order the frame and are read back through Context.tile_state(), and the
   frame after it is checked as every frame is;
 - MODE_THROUGHPUT (the SUB variant) against its own reference, the oracle's arithmetic on the sub-streams (test_gpu_throughput.py)."""
import ctypes as C

import numpy as np
import pytest

from mort_amd import host, hip, structs as S
from tests import tile_ref
from tests.test_gpu_throughput import expected_substream, render_tp
from tests.worlds import custom_bvh_world, set_view

pytestmark = pytest.mark.gpu

BLOCKS = [1024, 768, 512, 384, 256]
LIMITS = list(range(1, 15)) + [15, 17, 19, 21, 23] + [25, 26, 50]  # the odd ones: 2 DL + 1 for DL = 7 ... 11
RING_MAX = 12  # world_images.h state_lds_levels
_REF = {}


def _scene(depth):
    return host.build_scene(1, width=96, spp=16, depth=depth)


def _ref(oracle, key, make):
    """the oracle's frame of (world, camera) = make(), computed once per key and shared by the block sizes"""
    if key not in _REF:
        world, cam = make()
        _REF[key] = oracle.render(world, cam, nthreads=8)
    return _REF[key]


def _ref1(oracle, depth):
    return _ref(oracle, ("scene1", depth), lambda: _scene(depth))


def _same(out, ref):
    assert (out["rgba"] == ref["rgba"]).all(), "uchar4 image differs"
    assert (out["accum"].view(np.uint32) == ref["accum"].view(np.uint32)).all(), "fp32 accumulators differ (bitwise)"
    assert (out["segments_px"] == ref["segments_px"]).all(), "per-pixel segment counts differ"
    assert out["stats"]["segments"] == ref["segments"], (out["stats"]["segments"], ref["segments"])
    assert out["stats"]["rng_draws"] == ref["rng_draws"], (out["stats"]["rng_draws"], ref["rng_draws"])
    assert (out["states"]["d"] == ref["states"]["d"]).all() and (out["states"]["v"] == ref["states"]["v"]).all(), "final RNG states differ"


def _render(ctx, oracle, world, cam, seed=True):
    W, H = cam.image_width, cam.image_height
    if seed:
        ctx.set_partition(0, 1, 8)
        ctx.upload_world(world)
        ctx.rng_seed(S.DEFAULT_SEED, W, H)
    out = ctx.render(cam, want_accum=True, want_segments=True)
    out["states"] = ctx.rng_store(W, H, oracle.STATE_DTYPE)
    return out


def _lds_levels(world):
    """ring sizes of a launch of mega_bvh_kernel on 1024-, 768- and 256-thread workgroups for this world (host only)"""
    fn = hip.lib().mort_hip_debug_bvh_lds_levels
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    info = (C.c_int * 4)()
    assert fn(C.cast(world.ptr, C.c_void_p), info) == 0
    assert info[0] > 0, "the world is not served by mega_bvh_kernel"
    return {1024: info[1], 768: info[2], 256: info[3]}


def test_the_limits_cross_every_ring_size(oracle):
    """Not a GPU check by itself: it makes the ring-boundary cases mean what the docstring says."""
    for dl in range(2, RING_MAX + 1):
        for limit in (dl, dl + 1, dl + 2, 2 * dl + 1):
            assert limit in LIMITS, (dl, limit)
    sizes = _lds_levels(_scene(50)[0])
    print(f"Scene 1 ring sizes by workgroup: {sizes}")
    for block, dl in sizes.items():
        assert 1 <= dl <= RING_MAX, (block, dl)
    assert max(sizes.values()) < 13  # the limit-25, -26 and -50 frames wrap every launch's ring
    # a frame at limit k holds paths that reach k levels iff the limit-50 frame has paths that k cuts short: their pixels' streams,
    # and so their segment counts, then differ between the two frames
    deep = _ref1(oracle, 50)
    for limit in LIMITS[:-1]:
        cut = int((deep["segments_px"] != _ref1(oracle, limit)["segments_px"]).sum())
        print(f"limit {limit}: {cut} pixels hold a path that reaches it")
        assert cut > 0, limit
    # and paths stop by themselves below the limit too (entries stay in the ring while others of the same wave leave it)
    assert int((deep["segments_px"] == _ref1(oracle, 2)["segments_px"]).sum()) > 0


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("depth", LIMITS)
def test_ring_boundaries(gpu_ctx, oracle, monkeypatch, depth, block):
    monkeypatch.setenv("MORT_FAST_BLOCK_SIZE", str(block))
    world, cam = _scene(depth)
    out = _render(gpu_ctx, oracle, world, cam)
    assert out["stats"]["kernel_name"].startswith(f"mega_bvh_kernel<{block},"), out["stats"]["kernel_name"]
    _same(out, _ref1(oracle, depth))


# ---- worlds whose paths are all deep ----

def _inside_camera(depth, spp=4, background=(0.0, 0.0, 0.0)):
    _, cam = host.build_scene(1, width=64, spp=spp, depth=depth)
    set_view(cam, (0.0, 0.5, 1.5), (0.0, 0.2, -1.0), vfov=70, defocus=0.0)
    cam.background.e[0], cam.background.e[1], cam.background.e[2] = background
    return cam


_INNER = [((0.0, 0.0, -1.0), 0.5, ("lamb", (.7, .3, .3))), ((1.1, 0.1, -1.4), 0.4, ("lamb", (.2, .5, .8))), ((-1.2, 0.3, -0.6), 0.45, ("lamb", (.8, .8, .2))),
          ((0.0, -100.5, -1.0), 100.0, ("lamb", (.5, .5, .5)))]


def _enclosed_world(light):
    """the camera and a few Lambertian spheres inside a Lambertian shell: no path leaves, none meets glass"""
    spheres = [((0.0, 0.0, 0.0), 6.0, ("lamb", (.8, .8, .8)))] + _INNER
    if light:
        spheres.append(((0.3, 1.6, -0.4), 0.3, ("light", (6.0, 5.0, 4.0))))
    return custom_bvh_world(spheres)


def _glass_world():
    """the same spheres inside a glass shell, under a bright sky: a path leaves through the shell or is reflected back in by it"""
    return custom_bvh_world([((0.0, 0.0, 0.0), 6.0, ("glass", 1.5))] + _INNER + [((0.6, 0.4, 0.3), 0.25, ("glass", 1.5))])


def _world_case(oracle, name, depth):
    if name == "glass":
        make = lambda: (_glass_world(), _inside_camera(depth, background=(0.7, 0.8, 1.0)))
    else:
        make = lambda: (_enclosed_world(name == "enclosed_lit"), _inside_camera(depth))
    world, cam = make()
    return world, cam, _ref(oracle, (name, depth), lambda: (world, cam))


@pytest.mark.parametrize("block", [1024, 256])
@pytest.mark.parametrize("step", ["DL", "DL+1", "2DL+1"])
@pytest.mark.parametrize("name", ["enclosed", "enclosed_lit"])
def test_enclosed_world_runs_every_path_to_the_limit(gpu_ctx, oracle, monkeypatch, name, step, block):
    dl = _lds_levels(_enclosed_world(name == "enclosed_lit"))[block]
    depth = {"DL": dl, "DL+1": dl + 1, "2DL+1": 2 * dl + 1}[step]
    monkeypatch.setenv("MORT_FAST_BLOCK_SIZE", str(block))
    world, cam, ref = _world_case(oracle, name, depth)
    px = cam.image_width * cam.image_height
    if name == "enclosed":  # nothing ends a path but the limit (or, in a few pixels, the seam between shell and ground): a sample traces `depth` segments
        assert (ref["segments_px"] <= depth * 4).all() and int((ref["segments_px"] == depth * 4).sum()) > 0.99 * px
        assert not ref["accum"].any()
    else:
        assert ref["accum"].any() and (ref["segments_px"] <= depth * 4).all() and (ref["segments_px"] == depth * 4).any()
    out = _render(gpu_ctx, oracle, world, cam)
    assert out["stats"]["kernel_name"].startswith(f"mega_bvh_kernel<{block},"), out["stats"]["kernel_name"]
    _same(out, ref)


@pytest.mark.parametrize("block", [1024, 256])
@pytest.mark.parametrize("depth", [3, 13, 26])
def test_glass_shell_world(gpu_ctx, oracle, monkeypatch, depth, block):
    monkeypatch.setenv("MORT_FAST_BLOCK_SIZE", str(block))
    world, cam, ref = _world_case(oracle, "glass", depth)
    shallow = _world_case(oracle, "glass", 2)[2]
    assert (ref["segments_px"] != shallow["segments_px"]).any() and ref["accum"].any()
    out = _render(gpu_ctx, oracle, world, cam)
    assert out["stats"]["kernel_name"].startswith(f"mega_bvh_kernel<{block},"), out["stats"]["kernel_name"]
    _same(out, ref)


# ---- frames in a row, partitions, the other launches ----

@pytest.mark.parametrize("block", [1024, 256])
def test_first_frame_after_the_probe_and_second_frame(gpu_ctx, oracle, monkeypatch, block):
    """The first frame after upload_world is ordered by the cost probe, which runs the same limit-50 paths with one sample on the
    frame's HBM part before the frame does; the second frame starts from the stored states and from a ring left wherever the first ended."""
    monkeypatch.setenv("MORT_FAST_BLOCK_SIZE", str(block))
    world, cam = _scene(50)
    r1 = _ref1(oracle, 50)
    if "frame2" not in _REF:
        _REF["frame2"] = oracle.render(world, cam, states=r1["states"].copy(), nthreads=8)
    r2 = _REF["frame2"]
    _same(_render(gpu_ctx, oracle, world, cam), r1)
    # the PROBE variant's own result: the tile costs the first frame was ordered by (Context.tile_state) are the oracle's one-sample
    # frame's from the same streams
    if "probe" not in _REF:
        cam1 = type(cam).from_buffer_copy(cam)
        cam1.samples_per_pixel, cam1.sqrt_spp, cam1.recip_sqrt_spp, cam1.pixel_samples_scale = 1, 1, 1.0, 1.0
        _REF["probe"] = oracle.render(world, cam1, nthreads=8, want_accum=False)
    ts = gpu_ctx.tile_state()
    assert (ts["ordered"], ts["probed"], ts["block"]) == (1, 1, block)
    probe_cost = np.zeros(ts["tiles"], np.uint32)
    probe_cost[ts["order"]] = ts["keys"]
    assert (np.sort(ts["order"]) == np.arange(ts["tiles"])).all()
    assert (probe_cost == tile_ref.tile_costs(_REF["probe"]["segments_px"], cam.image_width)).all(), "the probe's tile costs"
    assert (ts["cost"] == tile_ref.tile_costs(r1["segments_px"], cam.image_width)).all(), "the first frame's tile costs"
    _same(_render(gpu_ctx, oracle, world, cam, seed=False), r2)
    assert gpu_ctx.tile_state()["probed"] == 0


@pytest.mark.parametrize("block", [1024, 256])
def test_two_way_partition(gpu_ctx, oracle, monkeypatch, block):
    monkeypatch.setenv("MORT_FAST_BLOCK_SIZE", str(block))
    world, cam = _scene(26)
    ref = _ref1(oracle, 26)
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


@pytest.mark.parametrize("block", [1024, 256])
def test_throughput_mode_past_the_ring(gpu_ctx, oracle, monkeypatch, block):
    """the SUB variant at a limit past twice the largest ring, against the mode's own definition"""
    monkeypatch.setenv("MORT_FAST_BLOCK_SIZE", str(block))
    world, cam = host.build_scene(1, width=24, spp=9, depth=26)
    out = render_tp(gpu_ctx, world, cam)
    assert out["stats"]["kernel_name"].startswith(f"mega_bvh_kernel<{block},") and out["stats"]["kernel_name"].endswith(", true>")
    acc, rgba = expected_substream(oracle, world, cam, S.DEFAULT_SEED)
    assert (out["accum"].view(np.uint32) == acc.view(np.uint32)).all()
    assert (out["rgba"] == rgba).all()
