"""Frames at the limits of the state-machine kernels' packed state.  mega_bvh_kernel and mega_gen_kernel keep a lane's pixel as
xy & 0xffff and (xy >> 16) & 0x7fff and its sample as s_ij (s_i | s_j << 16); choose_family (mort_hip.hip) guards the packing with
W < 65536, H < 32768 and sqrt_spp < 32768 and hands anything beyond to the one-lane kernel.  Every case here is compared with the oracle
through test_gpu_parity.assert_same -- uchar4 image, accumulator bits, per-pixel segment counts, totals and final stream words, so the
seeding of frames this wide and this tall is covered too -- and the kernel that rendered it is asserted in both directions:

  65535 x 1, 1 x 32767, 65535 x 2   the state-machine kernels, at their last width and height
  65536 x 1, 1 x 32768              mega_kernel, one past them

on a sphere-BVH world (mega_bvh_kernel), a flat world of more than 48 primitives (mega_gen_kernel), both again in wavefront mode, and
both with the one-lane kernel forced (MORT_FORCE_GENERIC=1); 1 spp, bounce limit 4.  A frame of aspect 65535 : 1 fans out to nearly 180
degrees, so the worlds hold a large sphere (and the flat one a wall) far off to the +u side and a sphere at the top of the view: the census (on the oracle) wants at least 256
pixels with x >= 65000, or y >= 32000, that trace two segments or more.  One 1 x 32767 frame is rendered as 3 ranks of 8-row blocks and
recomposed; one 2 x 2 frame at 181^2 = 32761 spp exercises s_ij and the tile key's sample index far beyond the ten scenes' 44.

Measured on the MI355X: 0.01 - 0.13 s per case for the wide frames, 0.46 - 0.49 s for the tall ones (the same on every kernel: 32767 rows
of one pixel), 0.95 s for the three ranks, 0.94 - 2.26 s at 181^2 spp; the oracle 0.02 - 0.2 s per frame, rendered once per world and size."""
import functools
import time

import numpy as np
import pytest

from mort_amd import host, hip, structs as S
from tests import oracle_lib as O
from tests.test_gpu_parity import assert_same
from tests.worlds import custom_bvh_world, flat_camera, flat_world, set_view

pytestmark = pytest.mark.gpu

FROM, AT = (0.0, 0.8, 2.5), (0.0, 0.0, -1.0)
# +u of this view is +x: the last columns of a 65535-wide frame look straight along it, with a direction some 3e5 long (ten units per pixel),
# so what they are to hit must lie beyond 0.001 of that: ray_color's t_min
SIDE = ((2000.0, 0.8, 2.5), 1200.0)
ABOVE = ((0.0, 2.79, -5.14), 1.0)      # around the direction of the 55-degree view's top rows
SIZES = ((65535, 1), (65536, 1), (1, 32767), (1, 32768), (65535, 2))
IDS = [f"{w}x{h}" for w, h in SIZES]


def _field(n):
    rng = np.random.default_rng(31)
    return [((float(rng.uniform(-4, 4)), float(rng.uniform(-0.3, 1.5)), float(rng.uniform(-6, 0))), float(rng.uniform(0.1, 0.45))) for _ in range(n)]


def _material(k):
    return (("lamb", (.7, .3, .3)), ("metal", (.8, .8, .8), 0.1), ("glass", 1.5), ("lamb", (.2, .4, .8)))[k % 4]


@functools.lru_cache(None)
def world(kind):
    """bvh: one reference BVH over 64 small spheres, the ground and the two large ones, built as worlds.random_bvh_world builds its own
    (a skip list, mort_add_bvh); flat: the same spheres and a wall quad at +x as a flat world of 60 primitives"""
    small = [(c, r, _material(k)) for k, (c, r) in enumerate(_field(64 if kind == "bvh" else 56))]
    big = [((0, -100.5, -1), 100, ("checker",)), (SIDE[0], SIDE[1], ("lamb", (.6, .6, .2))), (ABOVE[0], ABOVE[1], ("lamb", (.3, .7, .4)))]
    if kind == "bvh":
        return custom_bvh_world(big + small)
    prims = [("sphere", c, r, m) for c, r, m in big + small] + [("quad", (600.0, -3000.0, -3000.0), (0, 6000.0, 0), (0, 0, 6000.0), ("lamb", (.5, .5, .5)))]
    return flat_world(prims)[0]


def camera(width, height, spp=1, depth=4):
    """flat_camera's view at an arbitrary frame size (test_gpu_denoise._sized's idiom: the aspect that gives exactly this height)"""
    _, cam = host.build_scene(2, width=width, spp=spp, depth=depth, aspect=width / (height + 0.5))
    cam.background.e[0], cam.background.e[1], cam.background.e[2] = 0.30, 0.35, 0.45
    set_view(cam, FROM, AT, vfov=55, defocus=0.0)
    assert (cam.image_width, cam.image_height) == (width, height)
    return cam


@functools.lru_cache(None)
def reference(kind, width, height, spp=1, depth=4):
    t0 = time.perf_counter()
    ref = O.render(world(kind), camera(width, height, spp, depth), nthreads=16)
    print(f"oracle {kind} {width}x{height}x{spp}: {time.perf_counter() - t0:.2f} s, {ref['segments']} segments")
    return ref


def census(ref, width, height):
    """pixels at the far end of the frame that trace at least two segments"""
    seg = ref["segments_px"]
    return int((seg[:, 65000:] >= 2).sum()) if width > 65000 else int((seg[32000:, :] >= 2).sum())


def render(ctx, kind, cam, mode=hip.MODE_MEGA):
    ctx.set_partition(0, 1, 8)
    ctx.upload_world(world(kind))
    ctx.rng_seed(S.DEFAULT_SEED, cam.image_width, cam.image_height)
    t0 = time.perf_counter()
    out = ctx.render(cam, mode=mode, want_accum=True, want_segments=True)
    out["states"] = ctx.rng_store(cam.image_width, cam.image_height, O.STATE_DTYPE)
    print(f"{kind} {cam.image_width}x{cam.image_height}: {out['stats']['kernel_name']}, render + read back {time.perf_counter() - t0:.2f} s")
    return out


def within(width, height):
    return width < 65536 and height < 32768


@pytest.mark.parametrize("size", SIZES, ids=IDS)
@pytest.mark.parametrize("kind", ("bvh", "flat"))
def test_megakernels_up_to_the_limit_and_the_one_lane_kernel_past_it(gpu_ctx, kind, size):
    ref = reference(kind, *size)
    assert census(ref, *size) >= 256
    out = render(gpu_ctx, kind, camera(*size))
    want = ("mega_bvh_kernel" if kind == "bvh" else "mega_gen_kernel") if within(*size) else "mega_kernel"
    assert out["stats"]["kernel_name"].startswith(want) and (want != "mega_kernel" or out["stats"]["kernel_name"] == "mega_kernel"), out["stats"]["kernel_name"]
    assert_same(out, ref)


@pytest.mark.parametrize("size", SIZES, ids=IDS)
@pytest.mark.parametrize("kind", ("bvh", "flat"))
def test_wavefront_mode_at_the_limits(gpu_ctx, kind, size):
    ref = reference(kind, *size)
    out = render(gpu_ctx, kind, camera(*size), mode=hip.MODE_WAVE)
    assert out["stats"]["kernel_name"].startswith("wf_"), out["stats"]["kernel_name"]
    assert_same(out, ref)


@pytest.mark.parametrize("size", ((65535, 1), (1, 32767)), ids=("65535x1", "1x32767"))
@pytest.mark.parametrize("kind", ("bvh", "flat"))
def test_one_lane_kernel_forced_below_the_limit(gpu_ctx, monkeypatch, kind, size):
    ref = reference(kind, *size)
    monkeypatch.setenv("MORT_FORCE_GENERIC", "1")
    out = render(gpu_ctx, kind, camera(*size))
    assert out["stats"]["kernel_name"] == "mega_kernel"
    assert_same(out, ref)


def test_tall_frame_in_three_ranks(gpu_ctx):
    """1 x 32767 as 3 ranks of 8-row blocks, one after another on the one GPU, recomposed (test_gpu_parity.test_partition_invariance) and
    compared through assert_same like every other case: image, accumulators, per-pixel segment counts, totals and final stream words"""
    W, H = 1, 32767
    ref = reference("bvh", W, H)
    cam = camera(W, H)
    rgba, accum = np.zeros((H, W, 4), np.uint8), np.zeros((H, W, 3), np.float32)
    seg_px, states = np.zeros((H, W), np.uint32), np.zeros(W * H, O.STATE_DTYPE)
    seg = draws = 0
    owned = np.zeros(H, int)
    for r in range(3):
        gpu_ctx.set_partition(r, 3, 8)
        gpu_ctx.upload_world(world("bvh"))
        gpu_ctx.rng_seed(S.DEFAULT_SEED, W, H)
        out = gpu_ctx.render(cam, want_accum=True, want_segments=True)
        st = gpu_ctx.rng_store(W, H, O.STATE_DTYPE)
        assert out["stats"]["kernel_name"].startswith("mega_bvh_kernel")
        rows = [gpu_ctx.global_row(l) for l in range(gpu_ctx.local_rows(H))]
        owned[rows] += 1
        rgba[rows] = out["rgba"][rows]
        accum[rows] = out["accum"][rows]
        seg_px[rows] = out["segments_px"][rows]
        states[rows] = st[rows]                      # W = 1: a row is one stream
        seg += out["stats"]["segments"]
        draws += out["stats"]["rng_draws"]
        others = np.setdiff1d(np.arange(H), rows)
        assert (out["rgba"][others] == 0).all() and (out["segments_px"][others] == 0).all()
    gpu_ctx.set_partition(0, 1, 8)
    assert (owned == 1).all()
    assert_same(dict(rgba=rgba, accum=accum, segments_px=seg_px, states=states, stats=dict(segments=seg, rng_draws=draws)), ref)


@pytest.mark.parametrize("kind,mode", (("bvh", hip.MODE_MEGA), ("flat", hip.MODE_MEGA), ("bvh", hip.MODE_WAVE), ("flat", hip.MODE_WAVE)),
                         ids=("mega_bvh", "mega_gen", "wave_bvh", "wave_gen"))
def test_high_spp_on_a_tiny_frame(gpu_ctx, kind, mode):
    """2 x 2 pixels at 181 x 181 samples, bounce limit 3"""
    ref = reference(kind, 2, 2, 181 * 181, 3)
    cam = camera(2, 2, 181 * 181, 3)
    assert cam.sqrt_spp == 181
    out = render(gpu_ctx, kind, cam, mode=mode)
    if mode == hip.MODE_MEGA:
        assert out["stats"]["kernel_name"].startswith("mega_bvh_kernel" if kind == "bvh" else "mega_gen_kernel"), out["stats"]["kernel_name"]
    assert_same(out, ref)
