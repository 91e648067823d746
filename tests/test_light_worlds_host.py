"""The light objects no built-in scene has, through the host forms of everything that shades (no GPU): LIGHT_WORLDS of
tests/light_cases.py -- lists of one, of seven (a moving sphere, a glass sphere that does not emit, a quad turned away) and with members
that sample nothing, a sky dome (every shading point inside the light), a light in the plane of the floor it lights, a tiny distant
sphere, a moving light, a quad without area, a list over spheres a BVH build has moved, and the seven-member list in a world large enough
for the unified-tree megakernel.  64 x 36, 4 spp, bounce limit 8.

  host loop (item scan and, where the world has one, the unified tree)  ==  oracle: image, accumulators, per-pixel segment counts,
  totals, final RNG words; a radiance query over the frame's own primary rays and one SH9 probe  ==  oracle's ray_color.

A NaN's sign and payload are not compared (tests/query_rays._words).  Census, on the oracle alone: the light object changes at least 10 %
of the pixels of every world (measured 57 - 59 %, the dome 20 %); in dome, coplanar and degenerate_quad at least 5 % of the pixels hold a
non-finite sample (measured 58.1 %, 23.1 %, 58.1 % of the frame's primary rays).  The frame itself zeroes a NaN pixel sum
(camera.cuh:197-199), so no accumulator is non-finite (measured 0 in every world): the share is counted on the per-ray radiance, where
the NaN is still there."""
import numpy as np
import pytest

from mort_amd import hip, structs as S
from tests import light_cases as LC
from tests import query_rays as Q

NAMES = sorted(LC.LIGHT_WORLDS)


def _has_tree(world):
    return bool(hip.debug_gen_tree(world)["tree"])


@pytest.mark.parametrize("name", NAMES)
def test_census(name):
    c = LC.frame_census(name)
    print(f"{name}: light on / off differ in {c['changed']:.1%} of the pixels; non-finite first sample in {c['non_finite_samples']:.1%}; "
          f"non-finite accumulator in {c['non_finite_accum']:.1%}")
    assert c["changed"] >= 0.10, c
    if name in LC.NON_FINITE_WORLDS:
        assert c["non_finite_samples"] >= 0.05, c


def test_the_worlds_are_what_they_claim():
    for name in NAMES:
        w, cam = LC.light_world(name)
        o = w.c.objs
        mats = {o.host_sphere[i].mat_type for i in range(o.num_spheres)}
        assert S.MAT_DIELECTRIC in mats, name
        assert S.MAT_ISOTROPIC in mats or any(not o.host_constant_medium[i].skip for i in range(o.num_constant_medium)), name
        assert cam.light_obj_type != -1 and (cam.image_width, cam.sqrt_spp ** 2, cam.bounce_limit) == (64, 4, 8)
        assert any(cam.background.e[k] != 0 for k in range(3)) == (name != "dome")
    tab = LC._tables(LC.light_world("list_of_seven")[0])
    lt, li = tab["lists"][0]
    assert list(lt) == [1, 1, 1, 2, 2, 2, 2]
    sph = tab["spheres"][li[:3]]
    assert sph["moves"].astype(bool).sum() == 1 and (sph["mat_type"] == S.MAT_DIELECTRIC).sum() == 1
    areas = tab["quads"]["area"][li[3:]]
    assert areas.max() / areas.min() >= 1e4
    assert tab["quads"]["normal"][li[6]][2] == -1.0  # turned away from the camera and the scene
    assert len(LC._tables(LC.light_world("list_of_one")[0])["lists"][0][0]) == 1
    lt, _ = LC._tables(LC.light_world("list_with_foreign")[0])["lists"][1]
    assert list(lt) == [S.OBJ_QUAD, S.OBJ_SPHERE, S.OBJ_TRANSLATE, S.OBJ_CONSTANT_MEDIUM]
    w, cam = LC.light_world("bvh_list")
    lt, li = LC._tables(w)["lists"][1]
    assert w.c.bvh_mode and list(lt) == [1, 1] and set(li).isdisjoint({0, 1})  # added first, moved by the build
    assert (LC._tables(w)["spheres"]["mat_type"][li] == S.MAT_DIFFUSE_LIGHT).all()
    big = LC.light_world("big_list")[0].c.objs
    assert big.num_spheres + big.num_quads >= 60


def test_a_quad_without_area_in_the_scan_is_accepted_and_swallows_the_frame(oracle):
    """why degenerate_quad keeps its quad out of the scan: the compile accepts u || v, and quad::hit's NaN t passes every test, so every
    ray ends on it -- in the oracle and in the host loop alike.  No box bounds such a quad, so the world gets no unified tree (it had one,
    and the tree walk missed the quad in 228 of these 576 pixels)"""
    assert not _has_tree(LC.Wd.flat_world(LC._BASE + [("quad", (-1, 2.2, -2), (2, 0, 0), (4, 0, 0), ("light", (9, 9, 9)))])[0])
    assert not _has_tree(LC.Wd.flat_world(LC._BASE + [("quad", (-1, 2.2, -2), (0, 0, 0), (4, 0, 0), ("light", (9, 9, 9)))])[0])
    assert _has_tree(LC.light_world("degenerate_quad")[0])  # skipped by the scan: not in the tree either
    w, ids = LC.Wd.flat_world(LC._BASE + [("quad", (-1, 2.2, -2), (2, 0, 0), (4, 0, 0), ("light", (9, 9, 9)))])
    cam = LC.Wd.flat_camera(light=ids[4], spp=4, width=32, depth=8)
    ref = oracle.render(w, cam, nthreads=4)
    assert ref["segments"] == cam.image_width * cam.image_height * 4 and not ref["accum"].any()
    for tree in (False, True):
        out = hip.render_host(w, cam, nthreads=4, tree=tree)
        LC.assert_frame_same(out, ref, f"tree={tree}")


@pytest.mark.parametrize("tree", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_host_loop_equals_the_oracle(name, tree):
    w, cam = LC.light_world(name)
    out = hip.render_host(w, cam, nthreads=8, tree=tree)
    assert ("unified tree" in out["stats"]["kernel_name"]) == (tree and _has_tree(w))
    LC.assert_frame_same(out, LC.frame_reference(name), f"{name} tree={tree}")


@pytest.mark.parametrize("tree", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_radiance_query_along_the_frames_primary_rays(name, tree):
    w, _ = LC.light_world(name)
    r = LC.radiance_reference(name)
    streams = r.streams0.copy()
    got = hip.query_radiance_host(w, r.params, r.rays, streams, tree=tree, nthreads=8)["rgb"]
    bad = np.flatnonzero((Q._words(got) != Q._words(r.rgb)).any(1))
    assert bad.size == 0, f"{name}: colour differs for {bad.size} rays, first {bad[0]}: got {got[bad[0]]} oracle {r.rgb[bad[0]]}"
    assert streams.tobytes() == r.streams.tobytes(), f"{name}: final streams differ"


@pytest.mark.parametrize("tree", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_one_probe(name, tree):
    from tests import probe_ref as P
    r = LC.probe_reference(name)
    streams = r.streams0.copy()
    sh = hip.probe_bake_host(r.world, r.params, r.probes, streams, tree=tree, nthreads=8)["sh"]
    P.assert_equal(sh, streams, r, f"{name} tree={tree}")
