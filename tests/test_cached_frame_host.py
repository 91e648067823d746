"""Cached frames on the host (mort_hip_render_cached_host, dev_cached_frame.h): both host traversals against the
walk of tests/cached_frame_ref.py over the oracle, tolerance 0 -- the uchar4, the accumulators as raw 32-bit words (any NaN equals
any NaN), per-pixel segments, the counts of paths that ended in the volume, all 48 bytes of every final stream.  No GPU."""
import numpy as np
import pytest

from mort_amd import hip
from tests import cached_frame_ref as FR
from tests import oracle_lib as O
from tests import volume_ref as V
from tests import worlds as Wd

F = np.float32
TREES = [False, True]
BIG = (40, 33)


def _frame(ref, tree, states=None, **kw):
    return hip.render_cached_host(ref.world, ref.cam, ref.params, ref.records, ref.depth, states=ref.streams0 if states is None else states,
                                  tree=tree, nthreads=4, **kw)


def _check(ref, tree, what):
    got = _frame(ref, tree)
    want = ref.frames[0]
    FR.assert_equal(got, got["states"], want, what)
    assert got["stats"]["segments"] == want["segments"] == int(got["segments_px"].sum()), what
    spp = ref.cam.sqrt_spp ** 2
    assert got["stats"]["eff_samples"] == spp * got["rgba"].shape[0] * got["rgba"].shape[1]
    assert (got["ends_px"] <= spp).all()
    return got


# ------------------------------------------------------------------------------------------------------------------- census

@pytest.mark.parametrize("name", FR.WORLDS)
def test_frames_show_something(name):
    """The census of the issue, on the reference alone, 40 x 33 x 4 spp at K = 1.  Measured (scene 6 / scene 1 / the flat world):
    share of the paths ending in the volume 48.6 / 33.6 / 13.6 %; Lambertian hits at iter >= K that fall through under the slab
    mask 1353 / 636 / 43 (the flat world seen from cached_frame_ref.ASIDE: its own camera gives 1); pixels whose sum is NaN
    under the poison mask 612 / 498 / 528 of 1320; paths ending in the volume directly after a dielectric level on scene 1: 214."""
    f = FR.reference(name, 1, BIG).frames[0]
    share = FR.share_ended(f, 4)
    print(name, "share ended", round(share, 3))
    assert 0.10 <= share <= 0.90, share
    fell = FR.reference(name, 1, BIG, mask="slab", aside=FR.slab_aside(name)).frames[0]["census"]["fell_through"]
    print(name, "fall through under the slab mask", fell)
    assert fell >= 20, fell
    nan = FR.reference(name, 1, BIG, mask="poison").frames[0]["census"]["nan_pixels"]
    print(name, "NaN pixels under the poison mask", nan)
    assert nan >= 1
    if name == "scene1":
        after = f["census"]["after_dielectric"]
        print(name, "end in the volume after a dielectric level", after)
        assert after >= 1


# ---------------------------------------------------------------------------------------------------------- bit for bit

@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("depth", FR.DEPTHS)
@pytest.mark.parametrize("name", FR.WORLDS)
def test_equals_the_reference(name, depth, visible, tree):
    _check(FR.reference(name, depth, mask="fractional", visible=visible), tree, f"{name} K={depth} visible={visible} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("mask", FR.MASKS)
@pytest.mark.parametrize("name", FR.WORLDS)
def test_every_mask(name, mask, visible, tree):
    aside = mask == "slab" and FR.slab_aside(name)
    _check(FR.reference(name, 1, BIG if aside else FR.SIZE, mask=mask, visible=visible, aside=aside), tree, f"{name} {mask} visible={visible} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("spp,sqrt_spp", [(1, 1), (4, 2), (9, 3), (5, 2)])
@pytest.mark.parametrize("name", FR.WORLDS)
def test_samples_per_pixel(name, spp, sqrt_spp, tree):
    """spp = 5 runs its 4 strata"""
    ref = FR.reference(name, 1, spp=spp, mask="slab", visible=spp != 4)
    assert ref.cam.sqrt_spp == sqrt_spp
    _check(ref, tree, f"{name} spp={spp} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("depth", FR.DEPTHS)
@pytest.mark.parametrize("name", FR.WORLDS)
def test_through_a_lens(name, depth, tree):
    """defocus_angle > 0: get_ray draws a point of the lens per sample"""
    ref = FR.reference(name, depth, mask="holes", visible=True, lens=True)
    assert ref.cam.defocus_angle > 0
    _check(ref, tree, f"{name} lens K={depth} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("size", [(1, 1), (13, 5), BIG])
def test_other_frame_sizes(size, tree):
    _check(FR.reference("scene6", 1, size, mask="fractional", visible=True), tree, f"scene6 {size} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
def test_without_the_optional_outputs(tree):
    """ends_px_out, accum_out and segments_px_out = NULL change nothing else"""
    ref = FR.reference("scene6", 1, mask="fractional", visible=True)
    want = ref.frames[0]
    got = _frame(ref, tree, want_ends=False)
    assert got["ends_px"] is None
    FR.assert_equal(got, got["states"], want, f"no counts tree={tree}", ends=False)
    got = _frame(ref, tree, want_accum=False, want_segments=False)
    assert got["accum"] is None and got["segments_px"] is None
    assert (got["rgba"] == want["rgba"]).all() and (got["ends_px"] == want["ends_px"]).all()
    assert got["states"].tobytes() == want["states"].tobytes()


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("name", FR.WORLDS)
def test_two_frames_continue_the_streams(name, tree):
    ref = FR.reference(name, 1, mask="fractional", frames=2)
    assert ref.frames[0]["states"].tobytes() != ref.frames[1]["states"].tobytes()
    first = _frame(ref, tree)
    FR.assert_equal(first, first["states"], ref.frames[0], f"{name} first frame tree={tree}")
    second = _frame(ref, tree, states=first["states"])
    FR.assert_equal(second, second["states"], ref.frames[1], f"{name} second frame tree={tree}")
    assert (ref.frames[0]["accum"] != ref.frames[1]["accum"]).any(), "a restart would repeat the first frame"


# ------------------------------------------------------------------------------------------------ equal to a plain render

def _assert_is_the_render(ref, tree, what):
    plain = O.render(ref.world, ref.cam, states=ref.streams0.copy(), nthreads=4)
    want = ref.frames[0]
    assert not want["ends_px"].any()
    for k in ("rgba", "segments_px"):
        assert (want[k] == plain[k]).all(), f"{what}: the reference's {k} against the oracle's render"
    assert (FR.words(want["accum"]) == FR.words(plain["accum"])).all() and want["states"].tobytes() == plain["states"].tobytes(), what
    got = _frame(ref, tree)
    FR.assert_equal(got, got["states"], want, what)
    assert not got["ends_px"].any()
    host = hip.render_host(ref.world, ref.cam, states=ref.streams0, tree=tree, nthreads=4)
    for k in ("rgba", "segments_px", "states"):
        assert (got[k] == host[k]).all(), f"{what}: {k} against render_host"
    assert (got["accum"].view(np.uint32) == host["accum"].view(np.uint32)).all()
    assert got["stats"]["segments"] == host["stats"]["segments"] == plain["segments"]
    assert got["stats"]["rng_draws"] == host["stats"]["rng_draws"] == plain["rng_draws"]


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("name", FR.WORLDS)
def test_depth_at_the_bounce_limit_is_the_render(name, visible, tree):
    """K = bounce_limit: no iteration can take the shortcut"""
    limit = FR.camera(name).bounce_limit
    _assert_is_the_render(FR.reference(name, limit, visible=visible), tree, f"{name} K=bounce_limit visible={visible} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("name", FR.WORLDS)
def test_all_weights_zero_is_the_render(name, depth, visible, tree):
    ref = FR.reference(name, depth, mask="zeros", visible=visible)
    assert ref.frames[0]["census"]["fell_through"] > 100
    _assert_is_the_render(ref, tree, f"{name} zeros K={depth} visible={visible} tree={tree}")


# ------------------------------------------------------------------------------------------------------------------ furnace

@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("visible", [False, True])
def test_furnace(visible, tree):
    """tests/test_cached_host.py's furnace seen through a camera: one Lambertian sphere of solid colour a, every record the constant
    radiance b, K = 0.  A pixel whose samples all hit the sphere ends every path there with a * b, so its accumulator is a * b within
    1e-5 relative (that file's bound for the sample's arithmetic; the mean of spp equal values adds two roundings) and its count is spp."""
    a, b = np.array([0.7, 0.35, 0.2], dtype=F), np.array([0.25, 0.5, 2.0], dtype=F)
    world, _ = Wd.flat_world([("sphere", (0.0, 0.0, -1.0), 0.5, ("lamb", tuple(float(x) for x in a)))])
    sh = np.zeros((9, 3), dtype=F)
    sh[0] = (b.astype(np.float64) / float(V.C0)).astype(F)
    g = hip.VOLUME_GRID((-1.0, -1.0, -2.0), (0.7, 1.1, 0.9), (4, 3, 2), 0.5)
    records = V.pack(np.tile(sh.reshape(1, 27), (g.probes, 1)))
    depth = np.ones((g.probes, hip.DEPTH_FLOATS), dtype=F) if visible else None
    cam = Wd.flat_camera(spp=9, width=24)
    Wd.set_view(cam, (0.0, 0.3, 0.8), (0.0, 0.0, -1.0), vfov=40)  # the sphere fills the middle of the frame
    for k in range(3):
        cam.background.e[k] = 0.0
    spp = cam.sqrt_spp ** 2
    p = hip.CACHED_FRAME_PARAMS(0, g, hip.VOLUME_VIS_PARAMS(0.01, 0.05) if visible else None)
    got = hip.render_cached_host(world, cam, p, records, depth, tree=tree, nthreads=2)
    inside = got["ends_px"] == spp
    assert inside.sum() >= 20, "the camera sees the sphere"
    assert (got["segments_px"] == spp).all(), "every path is one segment: a hit that ends in the volume, or a miss"
    want = a.astype(np.float64) * b.astype(np.float64)
    assert np.abs(got["accum"][inside].astype(np.float64) / want - 1.0).max() <= 1e-5
    assert (got["accum"][got["ends_px"] == 0] == 0).all()
