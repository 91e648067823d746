"""Cached radiance queries on the host (mort_hip_query_radiance_cached_host, dev_cached.h): both host traversals
against the walk of tests/cached_ref.py over the oracle, tolerance 0 -- colours as raw 32-bit words (any NaN equals any NaN), final
streams as all 48 bytes, the counts of paths that ended in the volume.  No GPU."""
import numpy as np
import pytest

from mort_amd import hip
from tests import cached_ref as CR
from tests import query_rays as Q
from tests import radiance_ref as R
from tests import volume_ref as V
from tests import worlds as Wd

F = np.float32
TREES = [False, True]


def _query(ref, tree, **kw):
    streams = ref.streams0.copy()
    got = hip.query_radiance_cached_host(ref.world, ref.params, ref.rays, streams, ref.records, ref.depth, tree=tree, nthreads=4, **kw)
    return got, streams


# ------------------------------------------------------------------------------------------------------------------- census

@pytest.mark.parametrize("name", CR.WORLDS)
def test_sets_show_something(name):
    """The census of the issue, on the reference alone.  Measured (scene 6 / scene 1 / the flat world): share of the primary and
    secondary paths ending in the volume 44 / 39 / 31 % at K = 1, 36 / 28 / 23 % at K = 2, 67 / 66 / 56 % at K = 0; Lambertian hits
    at iter >= K that fall through under the slab mask 1077 / 3045 / 117 at K = 1; paths ending in the volume directly after a
    dielectric level on scene 1: 65."""
    share = {k: CR.share_ended(CR.reference(name, k)) for k in CR.DEPTHS}
    print(name, {k: round(v, 3) for k, v in share.items()})
    assert 0.25 <= share[1] <= 0.60, share
    assert share[2] >= 0.15, share
    assert share[0] >= 0.50, share
    for k in CR.DEPTHS:
        fell = CR.reference(name, k, mask="slab").census["fell_through"]
        print(name, "K", k, "fall through under the slab mask", fell)
        assert fell >= 50, (k, fell)
    if name == "scene1":
        after = CR.reference(name, 1).census["after_dielectric"]
        print(name, "end in the volume after a dielectric level", after)
        assert after >= 10


def test_nan_reaches_the_colour():
    """no NaN guard.  Under "holes" the NaN coefficients sit in probes of weight 0 and poison nothing, so the NaN colours of that
    mask are those of the rays that are NaN anyway (scene 1 and the flat world have such rays, scene 6 none): at least one over the
    worlds.  Under "poison" -- a NaN probe of weight 1 -- every world has paths that end with a NaN, and more than under "ones" """
    holes = sum(int(np.isnan(CR.reference(name, 1, mask="holes").rgb).any(1).sum()) for name in CR.WORLDS)
    assert holes >= 1
    for name in CR.WORLDS:
        bad = int(np.isnan(CR.reference(name, 1, mask="poison").rgb).any(1).sum())
        plain = int(np.isnan(CR.reference(name, 1, mask="ones").rgb).any(1).sum())
        print(name, "NaN colours under poison", bad, "under ones", plain)
        assert bad >= plain + 10, (name, bad, plain)


# ---------------------------------------------------------------------------------------------------------- bit for bit

@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("depth", CR.DEPTHS)
@pytest.mark.parametrize("mask,samples", CR.CASES)
@pytest.mark.parametrize("name", CR.WORLDS)
def test_equals_the_reference(name, mask, samples, depth, visible, tree):
    ref = CR.reference(name, depth, samples, mask, visible)
    got, streams = _query(ref, tree)
    CR.assert_equal(got, streams, ref, f"{name} {mask} samples={samples} K={depth} visible={visible} tree={tree}")
    assert (got["ends"] <= samples).all()


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("depth", CR.DEPTHS)
def test_baked_volume_on_scene_6(depth, visible, tree):
    """the 3 x 3 x 3 grid in the Cornell box as the host forms bake it, with its baked depth maps"""
    ref = CR.reference("scene6", depth, 1, "baked", visible)
    assert CR.share_ended(ref) > 0.2
    got, streams = _query(ref, tree)
    CR.assert_equal(got, streams, ref, f"scene6 baked K={depth} visible={visible} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
def test_without_the_counts(tree):
    """ends_out = NULL changes nothing else"""
    ref = CR.reference("scene6", 1, 3, "fractional", True)
    got, streams = _query(ref, tree, want_ends=False)
    assert got["ends"] is None
    R.assert_equal(got["rgb"], streams, ref, f"no counts tree={tree}")


# ------------------------------------------------------------------------------------------ equal to a plain radiance query

@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("name", CR.WORLDS)
def test_depth_at_the_bounce_limit_is_a_radiance_query(name, visible, tree):
    """K = bounce_limit: no iteration can take the shortcut"""
    plain = R.reference(name, light=R.world_light(name))
    ref = CR.reference(name, plain.params.bounce_limit, 1, "ones", visible)
    R.assert_equal(ref.rgb, ref.streams, plain, f"{name}: the walk at K = bounce_limit against the oracle's ray_color")
    assert not ref.ends.any()
    got, streams = _query(ref, tree)
    R.assert_equal(got["rgb"], streams, plain, f"{name} K=bounce_limit visible={visible} tree={tree} against the oracle")
    assert not got["ends"].any()
    st = plain.streams0.copy()
    rad = hip.query_radiance_host(plain.world, plain.params, plain.rays, st, tree=tree, nthreads=4)["rgb"]
    assert (Q._words(got["rgb"]) == Q._words(rad)).all() and streams.tobytes() == st.tobytes()


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("name", CR.WORLDS)
def test_all_weights_zero_is_a_radiance_query(name, depth, visible, tree):
    """every sample returns a weight sum of 0: every Lambertian hit falls through to the shade step"""
    plain = R.reference(name, light=R.world_light(name))
    ref = CR.reference(name, depth, 1, "zeros", visible)
    R.assert_equal(ref.rgb, ref.streams, plain, f"{name}: the walk over an empty volume against the oracle's ray_color")
    assert ref.census["fell_through"] > 100 and not ref.ends.any()
    got, streams = _query(ref, tree)
    R.assert_equal(got["rgb"], streams, plain, f"{name} zeros K={depth} visible={visible} tree={tree} against the oracle")
    assert not got["ends"].any()
    st = plain.streams0.copy()
    rad = hip.query_radiance_host(plain.world, plain.params, plain.rays, st, tree=tree, nthreads=4)["rgb"]
    assert (Q._words(got["rgb"]) == Q._words(rad)).all() and streams.tobytes() == st.tobytes()


# ------------------------------------------------------------------------------------------------------------------ furnace

@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("visible", [False, True])
def test_furnace(visible, tree):
    """One Lambertian sphere of solid colour a under a constant radiance b, no light, K = 0: every probe's record is the constant
    b (band 0 alone), so E = pi b everywhere and every path ends at its first hit with a * b.  Tolerance 1e-5 relative: the
    expression -- one basis product, eight corners' weights and sums, one division, two products -- has fewer than twenty
    float32 roundings of 6e-8 each.  ends == samples and no stream moves."""
    a, b = np.array([0.7, 0.35, 0.2], dtype=F), np.array([0.25, 0.5, 2.0], dtype=F)
    world, _ = Wd.flat_world([("sphere", (0.0, 0.0, -1.0), 0.5, ("lamb", tuple(float(x) for x in a)))])
    sh = np.zeros((9, 3), dtype=F)
    sh[0] = (b.astype(np.float64) / float(V.C0)).astype(F)
    E = hip.sh9_irradiance(sh, (0.0, 0.6, 0.8))
    assert np.allclose(E, np.pi * b.astype(np.float64), rtol=1e-6, atol=0)
    g = hip.VOLUME_GRID((-1.0, -1.0, -2.0), (0.7, 1.1, 0.9), (4, 3, 2), 0.5)
    records = V.pack(np.tile(sh.reshape(1, 27), (g.probes, 1)))
    depth = np.ones((g.probes, hip.DEPTH_FLOATS), dtype=F) if visible else None
    rng = np.random.default_rng(5)
    n, samples = 500, 3
    origin = (Q._unit_sphere(rng, n) * F(3.0) + np.array([0, 0, -1], dtype=F)).astype(F)
    target = (np.array([0, 0, -1], dtype=F) + Q._unit_sphere(rng, n) * F(0.3)).astype(F)
    rays = np.zeros((n, 8), dtype=F)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = origin, target - origin, 0.5, np.inf
    rp = hip.RADIANCE_PARAMS()
    rp.bounce_limit, rp.samples, rp.light_obj_type, rp.light_obj_idx = 12, samples, -1, 0
    for k in range(3):
        rp.background[k] = b[k]
    cp = hip.CACHED_PARAMS(rp, 0, g, hip.VOLUME_VIS_PARAMS(0.01, 0.05) if visible else None)
    streams = Q.some_streams(n)
    before = streams.copy()
    got = hip.query_radiance_cached_host(world, cp, rays, streams, records, depth, tree=tree, nthreads=2)
    assert (got["ends"] == samples).all(), "every path hits the sphere and ends there"
    assert streams.tobytes() == before.tobytes()
    want = (a.astype(np.float64) * b.astype(np.float64)) * samples
    assert np.abs(got["rgb"].astype(np.float64) / want - 1.0).max() <= 1e-5
