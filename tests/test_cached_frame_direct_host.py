"""Direct-light cached frames on the host (mort_hip_render_cached_direct_host, dev_cached_frame_direct.h): both host
traversals against the walk of tests/cached_frame_direct_ref.py over the oracle, tolerance 0 -- the uchar4, the accumulators as raw
32-bit words (any NaN equals any NaN), per-pixel segments with the shadow searches in them, the counts of paths that ended in the
volume and of paths whose shadow segment saw light, all 48 bytes of every final stream -- the three identities of the contract, and
the sampled direct term of a frame against an area integral that is not the contract.  No GPU."""
import itertools

import numpy as np
import pytest

from mort_amd import hip
from tests import cached_frame_direct_ref as DR
from tests import oracle_lib as O
from tests import volume_ref as V
from tests import worlds as Wd

F = np.float32
TREES = [False, True]
BIG = (40, 33)
MATRIX_MASKS = ("ones", "fractional", "slab", "poison", "holes")
LIT_WORLDS = tuple(w for w in DR.WORLDS if w != "scene1")


def _frame(ref, tree, states=None, **kw):
    return hip.render_cached_direct_host(ref.world, ref.cam, ref.params, ref.records, ref.depth, states=ref.streams0 if states is None else states,
                                         tree=tree, nthreads=4, **kw)


def _check(ref, tree, what):
    got = _frame(ref, tree)
    want = ref.frames[0]
    DR.assert_equal(got, got["states"], want, what)
    assert got["stats"]["segments"] == want["segments"] == int(got["segments_px"].sum()), what
    spp = ref.cam.sqrt_spp ** 2
    assert got["stats"]["eff_samples"] == spp * got["rgba"].shape[0] * got["rgba"].shape[1]
    assert (got["lit_px"] <= got["ends_px"]).all() and (got["ends_px"] <= spp).all()
    assert "cached frame, direct" in got["stats"]["kernel_name"]
    return got


# ------------------------------------------------------------------------------------------------------------------- census

def test_scene_6_ends_lit_and_unlit():
    """The issue's conditions on the reference alone: scene 6, mask "ones", K = 0, 17 x 15 x 4 spp.  Measured: 815 of the 1 020 paths
    end in the volume (79.9 %); the shadow segment of 283 of them returns light (34.7 %).  Scene 6's light object is a list of the
    quad light and the glass sphere, so half of the samples aim at the sphere and return nothing."""
    f = DR.reference("scene6", 0).frames[0]
    c = f["census"]
    print("scene 6: paths", c["paths"], "ended", c["ended"], "lit", c["lit"])
    assert c["ended"] >= 0.50 * c["paths"]
    assert 0.10 * c["ended"] <= c["lit"] <= 0.90 * c["ended"]
    assert c["shadow_segments"] == c["ended"] and f["segments"] == int(f["segments_px"].sum())


def test_the_matrix_meets_every_rule():
    """Over the bit-for-bit matrix the terminal takes every branch of the contract.  Measured over K = 0, 1, 2 x the five masks x both
    flags x the four worlds at 17 x 15 x 4 spp: 43 106 paths of 122 400 end in the volume, 11 692 under rule (a) (scene 1: no light
    object; the BVH light world: 16 hits at iteration bounce_limit - 1), 31 414 shadow segments of which 14 994 are lit, 1 330 end in
    a medium (the flat world) and 14 044 are blocked by a solid that is no emitter.  No camera of the four worlds sees a point whose
    light sample has a pdf that is not > 0 or whose shadow segment misses, so two views of the BVH light world join the matrix
    (cached_frame_direct_ref.VIEWS): "below" has 23 pdfs that are not > 0 among its 1 020 paths, "far" at 96 x 80 x 16 spp has 2
    shadow segments that miss (and 2 such pdfs) among 70 125.  The BVH light world's own frames: lit 407 of 546 ended at K = 0."""
    tot = dict.fromkeys(DR.CENSUS_KEYS + ("ended", "lit"), 0)
    for name in DR.WORLDS:
        for k in DR.DEPTHS:
            for mask in MATRIX_MASKS:
                for visible in (False, True):
                    c = DR.reference(name, k, mask=mask, visible=visible).frames[0]["census"]
                    for key in tot:
                        tot[key] += c[key]
    below = DR.reference(DR.CD.BVH_LIGHT_WORLD, 0, view="below").frames[0]["census"]
    far = DR.reference(DR.CD.BVH_LIGHT_WORLD, 0, DR.FAR_SIZE, DR.FAR_SPP, view="far").frames[0]["census"]
    print(tot, "\nbelow", below, "\nfar", far)
    assert tot["rule_a"] >= 1 and tot["shadow_on_medium"] >= 1 and tot["shadow_blocked"] - tot["shadow_on_medium"] >= 1
    assert below["pdf_not_positive"] >= 1 and far["shadow_missed"] >= 1
    own = DR.reference(DR.CD.BVH_LIGHT_WORLD, 0).frames[0]["census"]
    assert own["lit"] > 0 and own["ended"] > own["lit"]
    forced = DR.reference("scene6", 2, bounce_limit=3).frames[0]["census"]
    assert forced["rule_a"] == forced["ended"] >= 100 and forced["shadow_segments"] == 0 and forced["lit"] == 0


def test_which_worlds_have_a_tree():
    """the host loop under MORT_HOST_TREE walks the unified tree where the GPU runs cached_frame_direct_kernel<true, *>"""
    for name in DR.WORLDS:
        got = _frame(DR.reference(name, 1), True)
        assert ("unified tree" in got["stats"]["kernel_name"]) == (name in DR.TREE_WORLDS), (name, got["stats"]["kernel_name"])
        assert "item scan" in _frame(DR.reference(name, 1), False)["stats"]["kernel_name"]


# ---------------------------------------------------------------------------------------------------------- bit for bit

@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("mask", MATRIX_MASKS)
@pytest.mark.parametrize("depth", DR.DEPTHS)
@pytest.mark.parametrize("name", DR.WORLDS)
def test_equals_the_reference(name, depth, mask, visible, tree):
    _check(DR.reference(name, depth, mask=mask, visible=visible), tree, f"{name} K={depth} {mask} visible={visible} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("depth,mask,visible", [(0, "fractional", False), (1, "holes", True), (2, "fractional", True), (1, "poison", False)])
@pytest.mark.parametrize("name", DR.WORLDS)
def test_through_a_lens(name, depth, mask, visible, tree):
    """defocus_angle > 0: get_ray draws a point of the lens per sample, before the path's and the terminal's draws"""
    ref = DR.reference(name, depth, mask=mask, visible=visible, lens=True)
    assert ref.cam.defocus_angle > 0
    _check(ref, tree, f"{name} lens K={depth} {mask} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
def test_the_rare_branches(tree):
    """the two views that show a pdf that is not > 0 (the quotient is what the division gives) and a shadow segment that misses"""
    _check(DR.reference(DR.CD.BVH_LIGHT_WORLD, 0, view="below"), tree, f"below tree={tree}")
    _check(DR.reference(DR.CD.BVH_LIGHT_WORLD, 0, DR.FAR_SIZE, DR.FAR_SPP, view="far"), tree, f"far tree={tree}")


@pytest.mark.parametrize("tree", TREES)
def test_the_slab_mask_from_aside(tree):
    """the flat world from cached_frame_ref.ASIDE, where hits fall through the slab mask's cells without a probe"""
    ref = DR.reference("flat:lit_by_quad_with_media", 1, BIG, mask="slab", visible=True, aside=True)
    assert ref.frames[0]["census"]["fell_through"] >= 20
    _check(ref, tree, f"flat aside tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("spp,sqrt_spp", [(1, 1), (9, 3), (5, 2)])
def test_samples_per_pixel(spp, sqrt_spp, tree):
    ref = DR.reference("scene6", 0, spp=spp, mask="fractional", visible=True)
    assert ref.cam.sqrt_spp == sqrt_spp
    _check(ref, tree, f"scene6 spp={spp} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("size", [(1, 1), (13, 5), BIG])
def test_other_frame_sizes(size, tree):
    _check(DR.reference("scene6", 1, size, mask="slab", visible=True), tree, f"scene6 {size} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
def test_without_the_optional_outputs(tree):
    """accum_out, segments_px_out, ends_px_out and lit_px_out = NULL in every combination change nothing else"""
    ref = DR.reference("scene6", 0, mask="fractional", visible=True)
    want = ref.frames[0]
    for accum, seg, ends, lit in itertools.product((False, True), repeat=4):
        got = _frame(ref, tree, want_accum=accum, want_segments=seg, want_ends=ends, want_lit=lit)
        what = f"accum={accum} segments={seg} ends={ends} lit={lit} tree={tree}"
        for key, on in (("accum", accum), ("segments_px", seg), ("ends_px", ends), ("lit_px", lit)):
            assert (got[key] is not None) == on, what
        assert (got["rgba"] == want["rgba"]).all() and got["states"].tobytes() == want["states"].tobytes(), what
        assert not accum or (DR.words(got["accum"]) == DR.words(want["accum"])).all(), what
        for key in ("segments_px", "ends_px", "lit_px"):
            assert got[key] is None or (got[key] == want[key]).all(), what
        assert got["stats"]["segments"] == want["segments"], what


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("name", DR.WORLDS)
def test_two_frames_continue_the_streams(name, tree):
    ref = DR.reference(name, 0, mask="fractional", frames=2)
    assert ref.frames[0]["states"].tobytes() != ref.frames[1]["states"].tobytes()
    first = _frame(ref, tree)
    DR.assert_equal(first, first["states"], ref.frames[0], f"{name} first frame tree={tree}")
    second = _frame(ref, tree, states=first["states"])
    DR.assert_equal(second, second["states"], ref.frames[1], f"{name} second frame tree={tree}")
    assert (ref.frames[0]["accum"] != ref.frames[1]["accum"]).any(), "a restart would repeat the first frame"


# ------------------------------------------------------------------------------------------------------- the identities

def _assert_is_the_cached_frame(ref, tree, what):
    """the direct frame against mort_hip_render_cached_host under the same camera, to the bit; lit all 0"""
    got = _check(ref, tree, what)
    plain = hip.render_cached_host(ref.world, ref.cam, ref.params, ref.records, ref.depth, states=ref.streams0, tree=tree, nthreads=4)
    for k in ("rgba", "segments_px", "ends_px", "states"):
        assert (got[k] == plain[k]).all(), f"{what}: {k} against render_cached_host"
    assert (got["accum"].view(np.uint32) == plain["accum"].view(np.uint32)).all(), what
    assert got["stats"]["segments"] == plain["stats"]["segments"] and got["stats"]["rng_draws"] == plain["stats"]["rng_draws"], what
    assert not got["lit_px"].any() and got["ends_px"].any(), what


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("name", DR.WORLDS)
def test_without_a_light_object_it_is_the_cached_frame(name, depth, visible, tree):
    """(i): scene 1 has none; the others lose theirs"""
    ref = DR.reference(name, depth, mask="fractional", visible=visible, light=False)
    assert ref.cam.light_obj_type == -1
    assert ref.frames[0]["census"]["rule_a"] == ref.frames[0]["census"]["ended"] and ref.frames[0]["census"]["shadow_segments"] == 0
    _assert_is_the_cached_frame(ref, tree, f"(i) {name} K={depth} visible={visible} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("depth", [0, 1, 2])
@pytest.mark.parametrize("name", LIT_WORLDS)
def test_no_segment_left_is_the_cached_frame(name, depth, tree):
    """(iii): bounce_limit == K + 1, so every terminal hit is at the last iteration and takes rule (a)"""
    ref = DR.reference(name, depth, mask="fractional", visible=depth == 1, bounce_limit=depth + 1)
    c = ref.frames[0]["census"]
    assert ref.cam.light_obj_type != -1 and c["rule_a"] == c["ended"] > 0 and c["shadow_segments"] == 0
    _assert_is_the_cached_frame(ref, tree, f"(iii) {name} K={depth} tree={tree}")


def _assert_is_the_render(ref, tree, what):
    plain = O.render(ref.world, ref.cam, states=ref.streams0.copy(), nthreads=4)
    want = ref.frames[0]
    assert not want["ends_px"].any() and not want["lit_px"].any()
    for k in ("rgba", "segments_px"):
        assert (want[k] == plain[k]).all(), f"{what}: the reference's {k} against the oracle's render"
    assert (DR.words(want["accum"]) == DR.words(plain["accum"])).all() and want["states"].tobytes() == plain["states"].tobytes(), what
    got = _check(ref, tree, what)
    assert not got["ends_px"].any() and not got["lit_px"].any()
    rh = hip.render_host(ref.world, ref.cam, states=ref.streams0, tree=tree, nthreads=4)
    for k in ("rgba", "segments_px", "states"):
        assert (got[k] == rh[k]).all(), f"{what}: {k} against render_host"
    assert (got["accum"].view(np.uint32) == rh["accum"].view(np.uint32)).all()
    assert got["stats"]["segments"] == rh["stats"]["segments"] == plain["segments"]
    assert got["stats"]["rng_draws"] == rh["stats"]["rng_draws"] == plain["rng_draws"]


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("name", DR.WORLDS)
def test_depth_at_the_bounce_limit_is_the_render(name, visible, tree):
    """(ii): K = bounce_limit, no iteration can end in the volume"""
    limit = DR.camera(name).bounce_limit
    _assert_is_the_render(DR.reference(name, limit, visible=visible), tree, f"(ii) {name} K=bounce_limit visible={visible} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("name", DR.WORLDS)
def test_all_weights_zero_is_the_render(name, depth, visible, tree):
    """(ii): no probe contributes anywhere"""
    ref = DR.reference(name, depth, mask="zeros", visible=visible)
    assert ref.frames[0]["census"]["fell_through"] > 100
    _assert_is_the_render(ref, tree, f"(ii) {name} zeros K={depth} visible={visible} tree={tree}")


# ------------------------------------------------------------------------------- against something that is not the contract

LE = (5.0, 3.0, 1.0)
LIGHT_Q, LIGHT_U, LIGHT_V = (-0.5, 2.0, -0.5), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)  # u x v = (0, -1, 0): the front face looks down
POINT = np.array([0.3, 0.0, -0.2])


def _light_integral(m):
    """the area integral of cos cos' / r^2 / pi over the light from POINT (normal +y), midpoint rule on m x m cells, float64"""
    s = (np.arange(m) + 0.5) / m
    a, b = np.meshgrid(s, s, indexing="ij")
    q = np.array(LIGHT_Q)[None, None, :] + a[..., None] * np.array(LIGHT_U) + b[..., None] * np.array(LIGHT_V)
    d = q - POINT
    r2 = (d * d).sum(-1)
    cos_p = d[..., 1] / np.sqrt(r2)  # at the point, against +y
    cos_l = d[..., 1] / np.sqrt(r2)  # at the light, against its normal -y, seen from below
    area = np.linalg.norm(np.cross(LIGHT_U, LIGHT_V))
    return float((cos_p * cos_l / r2 / np.pi).mean() * area)


@pytest.mark.parametrize("tree", TREES)
def test_the_sampled_term_is_the_area_integral(tree):
    """tests/test_cached_direct_host.py's white Lambertian floor under one quad light, nothing else, a black background, a volume of
    zeros with weight 1, K = 0, as a frame: one pixel of a pinhole camera half a unit above POINT looking straight down under a field
    of view of 1 degree (a footprint of 0.0087, 0.44 % of the light's distance of 2), 16 frames of 16 x 16 samples from
    independent seeds.  The mean of the 16 accumulators estimates albedo Le times the integral of cos cos' / r^2 / pi over the
    light, which a 64 x 64 midpoint rule gives in float64.  Allowed: 4 standard errors of that mean, from the spread of the 16
    frames, plus the quadrature's own error (the difference to the 32 x 32 rule).  Measured: the allowance is 0.62 % of the value in
    every channel, the mean is 0.27 % off."""
    world, ids = Wd.flat_world([("quad", (-5.0, 0.0, -5.0), (10.0, 0.0, 0.0), (0.0, 0.0, 10.0), ("lamb", (1.0, 1.0, 1.0))),
                                ("quad", LIGHT_Q, LIGHT_U, LIGHT_V, ("light", LE))])
    cam = Wd.flat_camera(light=ids[1], spp=256, width=1)
    cam.aspect_ratio = 1.0
    cam.vup.e[0], cam.vup.e[1], cam.vup.e[2] = 0.0, 0.0, -1.0
    for k in range(3):
        cam.background.e[k] = 0.0
    Wd.set_view(cam, tuple(float(x) for x in POINT + np.array([0.0, 0.5, 0.0])), tuple(float(x) for x in POINT), vfov=1, defocus=0.0)
    assert (cam.image_width, cam.image_height, cam.sqrt_spp) == (1, 1, 16)
    g = hip.VOLUME_GRID((-2.0, -1.0, -2.0), (2.0, 2.0, 2.0), (3, 3, 3), 0.5)
    records = V.pack(np.zeros((g.probes, 27), dtype=F))
    assert (records[:, 27] == 1).all()
    p = hip.CACHED_FRAME_PARAMS(0, g, None)
    frames = []
    for seed in range(16):
        got = hip.render_cached_direct_host(world, cam, p, records, None, seed=1000 + seed, tree=tree, nthreads=1)
        assert got["ends_px"][0, 0] == 256, "every path hits the floor and ends there"
        assert got["lit_px"][0, 0] == 256, "nothing stands between the point and the light"
        assert got["segments_px"][0, 0] == 512
        frames.append(got["accum"][0, 0].astype(np.float64))
    frames = np.array(frames)
    fine, coarse = _light_integral(64), _light_integral(32)
    for ch in range(3):
        want = LE[ch] * fine
        mean = frames[:, ch].mean()
        allowed = 4.0 * frames[:, ch].std(ddof=1) / np.sqrt(len(frames)) + LE[ch] * abs(fine - coarse)
        print(f"channel {ch}: mean {mean:.6f} integral {want:.6f} off {abs(mean - want) / want:.2%} allowed {allowed:.6f} ({allowed / want:.2%})")
        assert abs(mean - want) <= allowed, (ch, mean, want, allowed)
