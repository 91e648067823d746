"""MATERIAL_WORLDS (tests/material_worlds.py) through the host forms of everything that shades, against the oracle (no GPU): the host loop
over the item scan and, where the world has one, over the unified tree; a radiance query over the frame's own primary rays; one SH9 probe
at the camera.  Image, accumulators as raw words, per-pixel segment counts, totals and final RNG words are the oracle's
(material_worlds.assert_frame_same: light_cases.assert_frame_same plus the accumulators' raw words).

The tag rule (scene_compile.h mat_ref / tex_ref): every material or texture tag outside the known set compiles to ONE
reference, DREF_UNKNOWN, that no decode turns into a known tag.  Before the rule the compile step packed tag and index into 15 + 16 bits
unlooked-at, and four rows of TAG_ROWS aliased a known tag; measured on the commit before the rule, pixels of the 64 x 36 frame of
tag_row_world that differ from the oracle, item scan / unified tree / reference BVH alike: tex_zeroed 21, tex_high_bit 35,
mat_high_bits 36, mat_index_spill 36 of 2304, every other row 0; unknown_tags, which holds all the rows, 132.

Census, on the oracle alone: inside_glass holds primary rays that end in total internal reflection; in mirror_hall some pixel has every
sample at the bounce limit and some pixel is non-zero, at limits 64, 50 and 13 (measured in test_census_mirror_hall's output)."""
import numpy as np
import pytest

from mort_amd import hip, structs as S
from tests import material_worlds as M
from tests import query_rays as Q

KEYS = M.KEYS
IDS = [M.key_id(k) for k in KEYS]


def _has_tree(world):
    return bool(hip.debug_gen_tree(world)["tree"])


def test_the_catalogue_is_what_it_claims():
    assert S.MAX_BOUNCE_LIMIT == 64 and M.limits("mirror_hall") == (64, 50, 13)
    for name in M.MATERIAL_WORLDS:
        for form in M.forms(name):
            w = M.material_world(name, form)
            assert bool(w.c.bvh_mode) == (form == "bvh")
            if form == "bvh":  # the only way to the inline shade blocks: the world must be one the BVH kernels take
                im = hip.debug_bvh_images(w)
                assert im["sphere_bvh"] and im["four_wide"] and im["fits"] and im["wide_fits"], (name, im)
    m = M.material_world("ior_edges", "flat").c.mats
    iors = [m.host_dielectric[i].ior for i in range(m.num_dielectrics)]
    assert len(iors) == len(M.IORS) and sum(np.isnan(iors)) == 1 and sum(np.isinf(iors)) == 1
    o = M.material_world("ior_edges", "flat").c.objs
    radii = [o.host_sphere[i].radius for i in range(o.num_spheres)]
    assert radii.count(np.float32(0.3)) == radii.count(np.float32(-0.3)) == len(M.IORS)
    o = M.material_world("moving_mix", "bvh").c.objs
    moving = {o.host_sphere[i].mat_type for i in range(o.num_spheres) if o.host_sphere[i].moves}
    assert moving == {S.MAT_LAMBERTIAN, S.MAT_METAL, S.MAT_DIELECTRIC, S.MAT_DIFFUSE_LIGHT, S.MAT_ISOTROPIC}
    o = M.material_world("unknown_tags", "flat").c
    tags = {(o.objs.host_sphere[i].mat_type, o.objs.host_sphere[i].mat_idx) for i in range(o.objs.num_spheres)}
    assert {(t, i) for k, t, i in M.TAG_ROWS.values() if k == "mat"} <= tags
    texs = {(o.mats.host_lambertian[i].texType, o.mats.host_lambertian[i].texIdx) for i in range(o.mats.num_lambertians)}
    assert {(t, i) for k, t, i in M.TAG_ROWS.values() if k == "tex"} <= texs
    assert o.mats.num_metals == 1 and o.texs.num_solid_colors >= 1  # what the aliasing rows alias is in the tables
    o = M.material_world("surface_isotropic_and_phase", "flat").c.objs
    assert {o.host_constant_medium[i].mat_type for i in range(o.num_constant_medium)} == {S.MAT_LAMBERTIAN, S.MAT_METAL, S.MAT_DIELECTRIC, S.MAT_ISOTROPIC}
    assert S.MAT_ISOTROPIC in {o.host_quad[i].mat_type for i in range(o.num_quads)}


@pytest.mark.parametrize("form", ["flat", "bvh"])
def test_census_inside_glass(form):
    key = ("inside_glass", form, 12)
    n = M.total_internal_reflections(key)
    rays = len(M.primary_rays(M.camera("inside_glass", 12)))
    print(f"inside_glass {form}: {n} of {rays} primary rays end in total internal reflection")
    assert n >= rays // 20


@pytest.mark.parametrize("limit", M.limits("mirror_hall"))
@pytest.mark.parametrize("form", ["flat", "bvh"])
def test_census_mirror_hall(form, limit):
    ref = M.frame_reference(("mirror_hall", form, limit))
    seg = ref["segments_px"].reshape(-1)
    at_limit, lit = int((seg == 4 * limit).sum()), int(ref["accum"].reshape(-1, 3).any(1).sum())
    print(f"mirror_hall {form} limit {limit}: {at_limit} of {seg.size} pixels have every sample at the limit, {lit} are non-zero, max {seg.max()} segments")
    assert seg.max() == 4 * limit and at_limit >= 1 and lit >= 1


def _assert_host_loop(world, cam, ref, what):
    for tree in (False, True):
        out = hip.render_host(world, cam, nthreads=8, tree=tree)
        assert ("unified tree" in out["stats"]["kernel_name"]) == (tree and _has_tree(world)), out["stats"]["kernel_name"]
        M.assert_frame_same(out, ref, f"{what} tree={tree}")


@pytest.mark.parametrize("form", ["flat", "bvh"])
@pytest.mark.parametrize("row", sorted(M.TAG_ROWS))
def test_tag_rows_host_loop_equals_the_oracle(row, form):
    """one sphere with the row's tag over a ground sphere, one metal in the world: the four ALIASING_ROWS fail without the tag rule"""
    w = M.tag_row_world(row, form)
    assert form == "bvh" or _has_tree(w)
    _assert_host_loop(w, M._camera({}, 12), M.tag_row_reference(row, form), f"{row} {form}")


def test_unknown_tags_compile_to_one_reference():
    """the compiled spheres of unknown_tags, read back through a closest-hit query at each sphere's centre line: every unknown material
    tag is reported as the one unknown tag with index 0, and no sphere's moves bit is set (a moving sphere would report p off the ray)"""
    w = M.material_world("unknown_tags", "flat")
    o = w.c.objs
    rays = np.zeros(o.num_spheres, dtype=hip.RAY_DTYPE)
    for i in range(o.num_spheres):
        c = [o.host_sphere[i].center1.e[k] for k in range(3)]
        rays["origin"][i] = (c[0], c[1], c[2] + 50.0 if i else c[2] + 150.0)
    rays["dir"] = (0, 0, -1); rays["time"] = 0.5; rays["t_max"] = np.inf
    got = hip.query_closest_host(w, rays)["hits"]
    assert (got["flags"] & 1).all() and (got["p"][2:, :2] == rays["origin"][2:, :2]).all()
    unknown = 0
    for i in range(2, o.num_spheres):
        known = S.MAT_LAMBERTIAN <= o.host_sphere[i].mat_type <= S.MAT_ISOTROPIC
        want = (o.host_sphere[i].mat_type, o.host_sphere[i].mat_idx) if known else (0x7fff, 0)
        assert (int(got["mat_type"][i]), int(got["mat_idx"][i])) == want, (i, got[i])
        unknown += not known
    assert unknown == sum(1 for k, _, _ in M.TAG_ROWS.values() if k == "mat")


def test_an_index_outside_its_table_is_still_refused():
    """indices of known tags are validated as before the rule"""
    for bad in (("mat", S.MAT_METAL, 1), ("mat", S.MAT_METAL, -1), ("mat", S.MAT_METAL, 0x10000), ("tex", S.TEXTURE_SOLID, 999), ("tex", S.TEXTURE_CHECKER, -1)):
        w = M.build([M._GROUND, ((0, 1.1, -2.2), 0.5, ("metal", (.9, .6, .3), 0.0)), ((0, 0, -1), 0.3, bad)], "flat")
        with pytest.raises(hip.MortHipError) as e:
            hip.render_host(w, M._camera({}, 12))
        assert e.value.status == -1, bad  # MORT_ERR_INVALID


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_host_loop_equals_the_oracle(key):
    name, form, limit = key
    _assert_host_loop(M.material_world(name, form), M.camera(name, limit), M.frame_reference(key), M.key_id(key))


@pytest.mark.parametrize("tree", [False, True])
@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_radiance_query_along_the_frames_primary_rays(key, tree):
    w = M.material_world(key[0], key[1])
    r = M.radiance_reference(key)
    streams = r.streams0.copy()
    got = hip.query_radiance_host(w, r.params, r.rays, streams, tree=tree, nthreads=8)["rgb"]
    bad = np.flatnonzero((Q._words(got) != Q._words(r.rgb)).any(1))
    assert bad.size == 0, f"{key}: colour differs for {bad.size} rays, first {bad[0]}: got {got[bad[0]]} oracle {r.rgb[bad[0]]}"
    assert streams.tobytes() == r.streams.tobytes(), f"{key}: final streams differ"


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_one_probe(key):
    from tests import probe_ref as P
    r = M.probe_reference(key)
    for tree in (False, True):
        streams = r.streams0.copy()
        sh = hip.probe_bake_host(r.world, r.params, r.probes, streams, tree=tree, nthreads=8)["sh"]
        P.assert_equal(sh, streams, r, f"{key} tree={tree}")
