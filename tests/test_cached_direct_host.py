"""Direct-light cached radiance queries on the host (mort_hip_query_radiance_cached_direct_host, dev_cached_direct.h):
both host traversals against the walk of tests/cached_direct_ref.py over the oracle, tolerance 0 -- colours as raw 32-bit words (any
NaN equals any NaN), final streams as all 48 bytes, the counts of paths that ended in the volume and of paths whose shadow segment
saw light -- the identities with the cached and the plain radiance queries, and the sampled direct term against an area integral
that is not the contract.  No GPU."""
import numpy as np
import pytest

from mort_amd import hip, host
from tests import cached_direct_ref as DR
from tests import cached_ref as CR
from tests import query_rays as Q
from tests import radiance_ref as R
from tests import volume_ref as V
from tests import worlds as Wd
from tests.feature_ref import primary_rays

F = np.float32
# (tree, threads): the scan on one thread and the unified tree on three, as the matrix runs them; the other two in one test
FORMS = [(False, 1), (True, 3)]


def _query(ref, tree, nthreads=4, **kw):
    streams = ref.streams0.copy()
    got = hip.query_radiance_cached_direct_host(ref.world, ref.params, ref.rays, streams, ref.records, ref.depth, tree=tree, nthreads=nthreads, **kw)
    return got, streams


# ------------------------------------------------------------------------------------------------------------------- census

def _camera_walk(name, width=32):
    """the walk over the pixel-centre rays of a `width`-wide frame of the world's scene, one path, K = 0, mask "ones" """
    sid = int(name[5:])
    world, cam = host.build_scene(sid, width=width, spp=1)
    rays = Q.ray8(primary_rays(cam), Q.INF)
    g, rec, _, _ = CR.volume(name, "ones")
    path = hip.radiance_params_from_camera(cam, 1)
    streams = Q.some_streams(len(rays))
    return DR.walk(world, path, 0, g, rec, None, None, rays, streams), len(rays)


def test_scene_6_ends_lit_and_unlit():
    """The census of the issue on the reference alone: 32 x 32 camera rays of scene 6, one path, K = 0, mask "ones".  Measured: 889 of
    the 1024 paths end in the volume (86.8 %); the shadow segment of 313 of them returns light (35.2 %), that of 576 does not
    (64.8 %).  Scene 6's light object is a list of the quad light and the glass sphere, so half of the samples aim at the sphere and
    return nothing: uniform samples of the quad alone would be seen from about 70 % of these points."""
    (rgb, ends, lit, cen), n = _camera_walk("scene6")
    assert n == 32 * 32
    ended, seen = int(ends.sum()), int(lit.sum())
    print("scene 6: paths", n, "ended", ended, "lit", seen, "unlit", ended - seen)
    assert ended >= 0.50 * n
    assert seen >= 0.30 * ended
    assert ended - seen >= 0.05 * ended
    assert (lit <= ends).all()


def test_the_matrix_meets_every_rule():
    """Over the bit-for-bit matrix (K x CASES x the flag x the worlds) the terminal hits take every branch of the contract.  Measured
    over mask "ones", one path, both flags, K = 0, 1, 2: 7 990 terminal hits under rule (a) (scene 1: no light object; the BVH light
    world: four hits at iteration bounce_limit - 1), 32 with a pdf that is not > 0 (all of them in the BVH light world, whose lights
    are spheres), 1 302 shadow segments that end in a medium (the flat world).  K at
    bounce_limit - 1 forces rule (a) on a lit world: every terminal hit of scene 6 at bounce limit 3, K = 2, takes it."""
    tot = dict(rule_a=0, pdf_not_positive=0, shadow_on_medium=0, shadow_segments=0)
    for name in DR.WORLDS:
        for k in DR.DEPTHS:
            for visible in (False, True):
                c = DR.reference(name, k, 1, "ones", visible).census
                for key in tot:
                    tot[key] += c[key]
    print(tot)
    assert tot["rule_a"] >= 1 and tot["pdf_not_positive"] >= 1 and tot["shadow_on_medium"] >= 1 and tot["shadow_segments"] >= 1000
    assert DR.reference("flat:lit_by_quad_with_media", 0).census["shadow_on_medium"] >= 1
    forced = DR.reference("scene6", 2, 1, "ones", False, bounce_limit=3)
    assert forced.census["rule_a"] == int(forced.ends.sum()) >= 100 and forced.census["shadow_segments"] == 0 and not forced.lit.any()


# ---------------------------------------------------------------------------------------------------------- bit for bit

@pytest.mark.parametrize("tree,threads", FORMS)
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("depth", DR.DEPTHS)
@pytest.mark.parametrize("mask,samples", DR.CASES)
@pytest.mark.parametrize("name", DR.WORLDS)
def test_equals_the_reference(name, mask, samples, depth, visible, tree, threads):
    ref = DR.reference(name, depth, samples, mask, visible)
    got, streams = _query(ref, tree, threads)
    DR.assert_equal(got, streams, ref, f"{name} {mask} samples={samples} K={depth} visible={visible} tree={tree}")
    assert (got["ends"] <= samples).all() and (got["lit"] <= got["ends"]).all()


@pytest.mark.parametrize("tree,threads", [(False, 3), (True, 1)])
@pytest.mark.parametrize("name", DR.WORLDS)
def test_the_other_thread_counts(name, tree, threads):
    ref = DR.reference(name, 0, 3, "fractional", True)
    got, streams = _query(ref, tree, threads)
    DR.assert_equal(got, streams, ref, f"{name} tree={tree} threads={threads}")


@pytest.mark.parametrize("tree,threads", FORMS)
def test_rule_a_at_the_last_iteration(tree, threads):
    """K = bounce_limit - 1: a path that ends in the volume has no segment left for the light"""
    ref = DR.reference("scene6", 2, 1, "ones", False, bounce_limit=3)
    got, streams = _query(ref, tree, threads)
    DR.assert_equal(got, streams, ref, f"scene6 K=2 limit=3 tree={tree}")
    assert got["ends"].sum() >= 100 and not got["lit"].any()


@pytest.mark.parametrize("tree,threads", FORMS)
def test_without_the_counts(tree, threads):
    """lit_out = NULL, ends_out = NULL and both change nothing else"""
    ref = DR.reference("scene6", 1, 3, "fractional", True)
    for want_ends, want_lit in ((True, False), (False, True), (False, False)):
        got, streams = _query(ref, tree, threads, want_ends=want_ends, want_lit=want_lit)
        assert (got["ends"] is None) == (not want_ends) and (got["lit"] is None) == (not want_lit)
        DR.assert_equal(got, streams, ref, f"ends={want_ends} lit={want_lit} tree={tree}")


@pytest.mark.parametrize("tree,threads", FORMS)
@pytest.mark.parametrize("name", DR.WORLDS)
def test_a_stride_of_rays_with_degenerate_directions(name, tree, threads):
    """every third ray and the whole axis set (directions of zero length, with NaN components, along the axes): each ray is its own
    query, so the answers are the reference's for those rays"""
    ref = DR.reference(name, 0, 3, "slab", True)
    ax = ref.slices["axis"]
    idx = np.union1d(np.arange(0, len(ref.rays), 3), np.arange(ax.start, ax.stop))
    d = ref.rays[idx, 3:6]
    assert ((d == 0).all(1)).sum() >= 10 and np.isnan(d).any(1).sum() >= 10
    streams = np.ascontiguousarray(ref.streams0[idx]).copy()
    got = hip.query_radiance_cached_direct_host(ref.world, ref.params, np.ascontiguousarray(ref.rays[idx]), streams, ref.records, ref.depth,
                                                tree=tree, nthreads=threads)
    DR.assert_equal(got, streams, ref, f"{name} stride tree={tree}", idx=idx)


# ------------------------------------------------------------------------------------------------------------ identities

def _no_light(params):
    p = hip.CACHED_PARAMS.from_buffer_copy(params)
    p.path.light_obj_type, p.path.light_obj_idx = -1, 0
    return p


@pytest.mark.parametrize("tree,threads", FORMS)
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("name", DR.WORLDS)
def test_without_a_light_object_it_is_the_cached_query(name, depth, visible, tree, threads):
    """(i): to the bit, streams and ends included; nothing is lit.  Scene 1 names no light; the others have theirs taken away"""
    ref = DR.reference(name, depth, 3, "fractional", visible)
    p = _no_light(ref.params)
    a_st, b_st = ref.streams0.copy(), ref.streams0.copy()
    a = hip.query_radiance_cached_direct_host(ref.world, p, ref.rays, a_st, ref.records, ref.depth, tree=tree, nthreads=threads)
    b = hip.query_radiance_cached_host(ref.world, p, ref.rays, b_st, ref.records, ref.depth, tree=tree, nthreads=threads)
    assert (Q._words(a["rgb"]) == Q._words(b["rgb"])).all() and a_st.tobytes() == b_st.tobytes() and (a["ends"] == b["ends"]).all()
    assert a["ends"].sum() > 100 and not a["lit"].any()
    if name == "scene1":
        assert ref.params.path.light_obj_type == -1
        DR.assert_equal(a, a_st, ref, "scene 1 as it is")


@pytest.mark.parametrize("tree,threads", FORMS)
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("name", DR.WORLDS)
def test_depth_at_the_bounce_limit_is_a_radiance_query(name, visible, tree, threads):
    """(ii), K >= bounce_limit: no iteration can end in the volume"""
    plain = R.reference(name, light=R.world_light(name))
    ref = DR.reference(name, plain.params.bounce_limit, 1, "ones", visible)
    R.assert_equal(ref.rgb, ref.streams, plain, f"{name}: the walk at K = bounce_limit against the oracle's ray_color")
    got, streams = _query(ref, tree, threads)
    R.assert_equal(got["rgb"], streams, plain, f"{name} K=bounce_limit visible={visible} tree={tree} against the oracle")
    assert not got["ends"].any() and not got["lit"].any()
    st = plain.streams0.copy()
    rad = hip.query_radiance_host(plain.world, plain.params, plain.rays, st, tree=tree, nthreads=threads)["rgb"]
    assert (Q._words(got["rgb"]) == Q._words(rad)).all() and streams.tobytes() == st.tobytes()


@pytest.mark.parametrize("tree,threads", FORMS)
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("name", DR.WORLDS)
def test_all_weights_zero_is_a_radiance_query(name, depth, visible, tree, threads):
    """(ii), every weight 0: every Lambertian hit falls through to the shade step"""
    plain = R.reference(name, light=R.world_light(name))
    ref = DR.reference(name, depth, 1, "zeros", visible)
    R.assert_equal(ref.rgb, ref.streams, plain, f"{name}: the walk over an empty volume against the oracle's ray_color")
    assert ref.census["fell_through"] > 100 and not ref.ends.any()
    got, streams = _query(ref, tree, threads)
    R.assert_equal(got["rgb"], streams, plain, f"{name} zeros K={depth} visible={visible} tree={tree} against the oracle")
    assert not got["ends"].any() and not got["lit"].any()
    st = plain.streams0.copy()
    rad = hip.query_radiance_host(plain.world, plain.params, plain.rays, st, tree=tree, nthreads=threads)["rgb"]
    assert (Q._words(got["rgb"]) == Q._words(rad)).all() and streams.tobytes() == st.tobytes()


@pytest.mark.parametrize("name", ["scene6", "flat:lit_by_quad_with_media"])
def test_ends_are_the_cached_querys_on_the_first_path(name):
    """(iii): with one path per ray the streams have not parted before the terminal hit, so ends is the cached query's"""
    ref = DR.reference(name, 1, 1, "slab", False)
    st = ref.streams0.copy()
    b = hip.query_radiance_cached_host(ref.world, ref.params, ref.rays, st, ref.records, None, nthreads=4)
    assert (b["ends"] == ref.ends).all() and ref.ends.sum() > 100


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


@pytest.mark.parametrize("tree,threads", FORMS)
def test_the_sampled_term_is_the_area_integral(tree, threads):
    """One white Lambertian floor quad under one quad light, nothing else, a black background, a volume of zeros with weight 1,
    K = 0: 64 rays aimed at one floor point, N = 64 paths each.  rgb / N estimates Le times the integral of cos cos' / r^2 / pi over
    the light, which a 64 x 64 midpoint rule gives in float64.  Allowed: 4 standard errors of the mean over the 64 rays, computed
    here from their results, plus the quadrature's own error (the difference to the 32 x 32 rule); the test fails as vacuous should
    that allowance pass 5 % of the value."""
    world, ids = Wd.flat_world([("quad", (-5.0, 0.0, -5.0), (10.0, 0.0, 0.0), (0.0, 0.0, 10.0), ("lamb", (1.0, 1.0, 1.0))),
                                ("quad", LIGHT_Q, LIGHT_U, LIGHT_V, ("light", LE))])
    n, N = 64, 64
    rng = np.random.default_rng(22)
    up = Q._unit_sphere(rng, n).astype(np.float64)
    up[:, 1] = np.abs(up[:, 1]) * 0.5 + 0.3
    origin = POINT + up / np.linalg.norm(up, axis=1, keepdims=True) * rng.uniform(0.5, 1.5, (n, 1))
    rays = np.zeros((n, 8), dtype=F)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = origin, POINT - origin, 0.5, np.inf
    rp = hip.RADIANCE_PARAMS()
    rp.bounce_limit, rp.samples = 12, N
    rp.light_obj_type, rp.light_obj_idx = ids[1]
    g = hip.VOLUME_GRID((-2.0, -1.0, -2.0), (2.0, 2.0, 2.0), (3, 3, 3), 0.5)
    records = V.pack(np.zeros((g.probes, 27), dtype=F))
    assert (records[:, 27] == 1).all()
    streams = Q.some_streams(n)
    got = hip.query_radiance_cached_direct_host(world, hip.CACHED_PARAMS(rp, 0, g), rays, streams, records, None, tree=tree, nthreads=threads)
    assert (got["ends"] == N).all(), "every path hits the floor and ends there"
    assert (got["lit"] == N).all(), "nothing stands between the point and the light"
    per_ray = got["rgb"].astype(np.float64) / N
    fine, coarse = _light_integral(64), _light_integral(32)
    for ch in range(3):
        want = LE[ch] * fine
        mean = per_ray[:, ch].mean()
        allowed = 4.0 * per_ray[:, ch].std(ddof=1) / np.sqrt(n) + LE[ch] * abs(fine - coarse)
        print(f"channel {ch}: mean {mean:.6f} integral {want:.6f} allowed {allowed:.6f} ({allowed / want:.2%})")
        assert allowed <= 0.05 * want, "the allowance is too wide to show anything"
        assert abs(mean - want) <= allowed, (ch, mean, want, allowed)
