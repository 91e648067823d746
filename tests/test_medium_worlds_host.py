"""MEDIUM_WORLDS (tests/medium_worlds.py) on the CPU, so that tests/test_gpu_medium_worlds.py cannot pass for nothing:

  - the census, judged by the oracle alone: every medium that can be hit ends rays of the world's batch, the three that cannot (density 0,
    density 1e-30, a lone quad as boundary) end none, and the batch holds records with NaN t and with negative t, rays that drew and hit
    nothing, scatter points beyond the unified tree's reach, a ray that draws ten times in one segment, and medium normals other than
    (1, 0, 0).  Every test prints its figures;
  - the pin: each world's oracle render is the reference build's, live (pin_render of tests/test_reference_pin.py) and through the digests
    recorded in tests/golden/medium_pin.npz (tests/golden/make_golden.py), which hold where the reference is absent;
  - the host loops: render_host over the scan and over the tree, query_closest_host with and without streams, query_occluded_host,
    render_features_host, a radiance query and one probe, all bit for bit the oracle's;
  - what the compile step decides: which worlds get a unified tree, that a medium bounded by a medium is refused, that a medium bounded by
    a tag hitDispatch does not serve is never hit."""
import os

import numpy as np
import pytest

from mort_amd import hip, structs as S
from tests import material_worlds as M
from tests import medium_worlds as MW
from tests import oracle_lib as O
from tests import query_rays as Q
from tests.feature_ref import assert_same_words
from tests.golden.make_golden import MEDIUM_PIN_FRAMES, digest, state_words
from tests.test_reference_pin import pin_render, ref  # noqa: F401  (the fixture: skips where the reference is absent, as that module does)

NAMES = MW.NAMES
PIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "medium_pin.npz")
UNSUPPORTED = -6


def _has_tree(world):
    return bool(hip.debug_gen_tree(world)["tree"])


# ------------------------------------------------------------------------------------------------------------------ census

# media no ray of a batch ends on: hit_distance = -inf * log(u) = +inf and -1e30 * log(u) >= 5e22 for every u but exactly 1.0f (2^-25 of
# curand_uniform's draws, none of them here: the batches are fixed), and a boundary that is met once only
CANNOT_BE_HIT = {"density_edges": (MW.DENSITY_EDGES.index(0.0), MW.DENSITY_EDGES.index(1e-30)), "boundary_shapes": (MW.LONE_QUAD,)}
# a sphere of radius 0 has a discriminant <= 0 in exact arithmetic: two boundary roots 0.0001 apart take a rounding error no ray need have
NO_FLOOR = {"boundary_shapes": (MW.ZERO_RADIUS,)}


def _figures(name):
    w, r = MW.world(name), MW.rays(name)
    med = r.medium >= 0
    t = r.rec["t"]
    info = Q.reach(w)
    return dict(rays=len(r.rays), per_medium=[int((r.medium == i).sum()) for i in range(len(MW.media_of(w)))],
                nan_t=int((med & np.isnan(t)).sum()), negative_t=int((med & (t < 0)).sum()),
                drew_and_hit_nothing=int((~r.hit & r.advanced).sum()), most_draws=int(r.draws.max()),
                beyond_reach=int((med & ~Q.in_reach(info, r.rec["p"])).sum()) if info["tree"] else None,
                turned_normals=int((med & (r.rec["normal"] != np.array([1, 0, 0], np.float32)).any(1)).sum()),
                cut_inside=int((r.medium[r.slices["cut"]] >= 0).sum()))


@pytest.mark.parametrize("name", NAMES)
def test_census(name):
    w, r = MW.world(name), MW.rays(name)
    f = _figures(name)
    print(f"{name}: " + ", ".join(f"{k} {v}" for k, v in f.items()))
    assert len(r.rays) <= 6500 and len(set(MW.media_of(w))) == len(MW.media_of(w)), "every medium has a phase material of its own"
    solids = {(w.c.objs.host_sphere[i].mat_type, w.c.objs.host_sphere[i].mat_idx) for i in range(w.c.objs.num_spheres) if not w.c.objs.host_sphere[i].skip}
    solids |= {(w.c.objs.host_quad[i].mat_type, w.c.objs.host_quad[i].mat_idx) for i in range(w.c.objs.num_quads) if not w.c.objs.host_quad[i].skip}
    assert not solids & set(MW.media_of(w)), "a solid shares a medium's phase material"
    for i, n in enumerate(f["per_medium"]):
        if i in CANNOT_BE_HIT.get(name, ()):
            assert n == 0, f"{name}: medium {i} cannot be hit and ends {n} rays"
        elif i not in NO_FLOOR.get(name, ()):
            assert n >= 10, f"{name}: medium {i} ends {n} rays"
    assert f["cut_inside"] >= 10, "rays whose t_max ends them inside a medium"
    # a medium hit is a front-face record; a ray that drew nothing has its stream as it was
    med = r.medium >= 0
    assert r.rec["front_face"][med].all() and (r.draws[~r.advanced] == 0).all() and (r.draws[r.advanced] >= 1).all()
    if name == "density_edges":
        assert f["drew_and_hit_nothing"] >= 20 and f["nan_t"] >= 20 and f["negative_t"] >= 20
        nan_medium = MW.DENSITY_EDGES.index(next(d for d in MW.DENSITY_EDGES if d != d))
        assert (r.medium[np.isnan(r.rec["t"]) & med] == nan_medium).all() and np.isnan(r.rec["p"][r.medium == nan_medium]).all()
    if name == "negative_far":
        assert f["negative_t"] >= 20 and f["beyond_reach"] >= 100
    if name == "fifty_media":
        assert f["most_draws"] >= 10 and len(f["per_medium"]) == MW.MAX_MEDIA
    if name == "transformed_phase":
        assert f["turned_normals"] >= 10
    if name == "camera_inside":
        cam = MW.camera(name)
        c, rad = MW.probes(name)[0]
        assert np.linalg.norm(np.array([cam.center.e[k] for k in range(3)]) - c) < rad and f["negative_t"] >= 10


def test_the_table_holds_fifty_media():
    from tests import worlds as Wd
    b = MW._Builder()
    for k in range(MW.MAX_MEDIA):
        b.medium(MW._ball((0.4 * k, 0, 0), 0.1, 1.0, 0), False)
    with pytest.raises(RuntimeError):  # Wd._ok: mort_add_constant_medium returned -1
        b.medium(MW._ball((0.4 * MW.MAX_MEDIA, 0, 0), 0.1, 1.0, 0), False)
    assert b.w.c.objs.num_constant_medium == MW.MAX_MEDIA and Wd._ok(0, "") == 0


# --------------------------------------------------------------------------------------------------------------------- pin

@pytest.mark.parametrize("name", NAMES)
def test_oracle_renders_as_the_reference(ref, name):  # noqa: F811
    pin_render(MW.world(name), MW.camera(name))


def _render_digests(render, name):
    w, cam = MW.world(name), MW.camera(name)
    out, st = [], None
    for f in range(MEDIUM_PIN_FRAMES):
        r = render(w, cam, st)
        st = r["states"]
        out.append([digest(r["rgba"]), digest(r["accum"]), digest(state_words(st))])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_the_recorded_reference(name):
    """holds where the reference is absent: the oracle's frames hash to what the reference build rendered"""
    got = _render_digests(lambda w, c, st: O.render(w, c, states=st, nthreads=16, want_segments=False), name)
    for f, g in enumerate(got):
        assert g == np.load(PIN)[f"{name}_f{f}"].tolist(), f"frame {f}: [rgba, accum, states] digests differ"


@pytest.mark.parametrize("name", NAMES)
def test_reference_build_matches_its_record(ref, name):  # noqa: F811
    from tests import ref_lib as R
    got = _render_digests(lambda w, c, st: R.render(w, c, states=st), name)
    for f, g in enumerate(got):
        assert g == np.load(PIN)[f"{name}_f{f}"].tolist()


# -------------------------------------------------------------------------------------------------------------- host loops

@pytest.mark.parametrize("name", NAMES)
def test_host_loop_equals_the_oracle(name):
    w, cam, want = MW.world(name), MW.camera(name), MW.frame_reference(name)
    for tree in (False, True):
        out = hip.render_host(w, cam, nthreads=8, tree=tree)
        assert ("unified tree" in out["stats"]["kernel_name"]) == (tree and _has_tree(w)), out["stats"]["kernel_name"]
        M.assert_frame_same(out, want, f"{name} tree={tree}")


@pytest.mark.parametrize("name", NAMES)
def test_closest_hit_queries_equal_the_oracle(name):
    w, r = MW.world(name), MW.rays(name)
    for tree in (False, True):
        streams = r.streams0.copy()
        got = hip.query_closest_host(w, r.rays, streams, tree=tree, nthreads=8)["hits"]
        MW.assert_hits_equal(name, got, True, f"{name} with streams tree={tree}")
        assert streams.tobytes() == r.streams.tobytes(), f"{name} tree={tree}: final streams differ"
        got = hip.query_closest_host(w, r.rays, tree=tree, nthreads=8)["hits"]
        MW.assert_hits_equal(name, got, False, f"{name} without streams tree={tree}")
        occ = hip.query_occluded_host(w, r.rays, tree=tree, nthreads=8)["occluded"]
        assert (occ.astype(bool) == r.shit).all(), f"{name} tree={tree}: occlusion differs from the oracle's solid hits"


@pytest.mark.parametrize("name", NAMES)
def test_feature_pass_equals_the_oracle(name):
    w, cam, want = MW.world(name), MW.camera(name), MW.features_reference(name)
    assert (want["kind"] == 2).sum() >= 20, "pixels whose first hit is a medium"
    for tree in (False, True):
        assert_same_words(hip.render_features_host(w, cam, nthreads=8, tree=tree), want, f"{name} tree={tree}")


@pytest.mark.parametrize("name", NAMES)
def test_radiance_query_and_one_probe(name):
    from tests import probe_ref as P
    w = MW.world(name)
    r, p = MW.radiance_reference(name), MW.probe_reference(name)
    for tree in (False, True):
        streams = r.streams0.copy()
        got = hip.query_radiance_host(w, r.params, r.rays, streams, tree=tree, nthreads=8)["rgb"]
        bad = np.flatnonzero((Q._words(got) != Q._words(r.rgb)).any(1))
        assert bad.size == 0, f"{name}: colour differs for {bad.size} rays, first {bad[0]}: got {got[bad[0]]} oracle {r.rgb[bad[0]]}"
        assert streams.tobytes() == r.streams.tobytes(), f"{name}: final streams differ"
        streams = p.streams0.copy()
        sh = hip.probe_bake_host(w, p.params, p.probes, streams, tree=tree, nthreads=8)["sh"]
        P.assert_equal(sh, streams, p, f"{name} tree={tree}")


# -------------------------------------------------------------------------------------------------------------- tree facts

def test_which_worlds_get_a_unified_tree():
    assert [n for n in NAMES if not _has_tree(MW.world(n))] == list(MW.NO_TREE)
    for name in MW.TREE_NAMES:  # ... and the camera can use it
        cam = MW.camera(name)
        centre = np.array([[cam.center.e[k] for k in range(3)]], np.float32)
        assert hip.debug_gen_tree(MW.world(name))["fits"] and Q.in_reach(Q.reach(MW.world(name)), centre)[0], name


def test_a_medium_bounded_by_a_medium_is_refused():
    inner = MW._ball((0.9, 0.2, -0.8), 0.45, 2.0, 2)
    w = MW.odd_boundary_world(("medium", inner))
    for call in (lambda: hip.render_host(w, MW.camera("density_edges")), lambda: hip.debug_gen_tree(w),
                 lambda: hip.query_closest_host(w, MW.rays("density_edges").rays[:8])):
        with pytest.raises(hip.MortHipError) as e:
            call()
        assert e.value.status == UNSUPPORTED


@pytest.mark.parametrize("tag", [S.OBJ_BVH, 0, 99, -1])
def test_a_medium_bounded_by_a_tag_without_a_hit_test_is_never_hit(tag):
    """hitDispatch returns false for OBJ_BVH and for a tag it does not know: the world renders as the one without that medium"""
    cam = MW.camera("density_edges")
    w, without = MW.odd_boundary_world(("tag", tag, 0)), MW.odd_boundary_world(None)
    assert w.c.objs.num_constant_medium == 2 and without.c.objs.num_constant_medium == 1
    want = M._frozen(O.render(without, cam, nthreads=8))
    own = O.render(w, cam, nthreads=8)
    M.assert_frame_same(dict(own, stats=dict(segments=own["segments"], rng_draws=own["rng_draws"])), want, f"the oracle, tag {tag}")
    assert _has_tree(w)
    for tree in (False, True):
        M.assert_frame_same(hip.render_host(w, cam, nthreads=8, tree=tree), want, f"tag {tag} tree={tree}")
