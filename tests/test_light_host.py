"""Light sampling, record by record, on the CPU: hipcc's host compile of light_pdf_value and light_random (dev_render.h over dev_trace.h's
wsphere_* / wquad_*, reading the compile's world-order tables and flattened lists; mort_hip_debug_light_host) against the oracle's
pdf_value_dispatch / random_dispatch (mort_oracle_light_batch), bit for bit.  2^20 records per function and world
(tests/light_cases.py): tolerance 0, signed zeros count, any NaN equals any NaN, the final stream words and draw counts are equal.
The census conditions are asserted on the oracle's answers alone, before anything is compared.

What the sweep found: random_int(0, n - 1) gives n once in 2^25 draws for lists of 33 members and more (curand_uniform is exactly 1.0f
there), and light_random then read the NEXT list's first member where the reference reads its own array's (0, 0) entry past the members:
334 of the 83907 records on the BVH world's 500-member list differed (direction, stream and draw count).  scene_compile.h now ends
every list with that entry.

Measured (flat / BVH world): "toward" records with a finite positive pdf from outside 99.97 % / 99.96 % (static spheres), 99.96 % / 99.96 %
(moving), 99.32 % / 99.34 % (quads, off plane); inside a sphere 100 % NaN; every in-plane record of the axis quads +0; every foreign
tag +0 and (1,0,0) with no draw; 20841 / 20746 infinite pdfs of far spheres; random_int one past the list 103 times in the 20000
records looked at of the 40-member list, 116 of the 30000 of the 500-member list, never for 1 and 3 members."""
import numpy as np
import pytest

from mort_amd import host, hip, structs as S
from tests import light_cases as LC
from tests import oracle_lib as O

CASES = [(w, fn) for w in sorted(LC.WORLDS) for fn in (0, 1)]
IDS = [f"{w}-{LC.NAMES[fn]}" for w, fn in CASES]


@pytest.mark.parametrize("world_name,fn", CASES, ids=IDS)
def test_host_compile_equals_the_oracle(world_name, fn):
    LC.assert_census(world_name, fn)
    world, _ = LC.WORLDS[world_name]()
    rec, _ = LC.build(world_name, fn)
    got = hip.debug_light_host(world, fn, rec).reshape(len(rec), -1)
    LC.assert_same(fn, rec, dict(oracle=LC.oracle(world_name, fn), hipcc_host=got))


def test_the_bvh_build_moves_the_spheres():
    """the BVH world's list names spheres by world index, and the build has put another sphere at nearly every index"""
    _, tab, moved = LC.bvh_light_world()
    assert moved >= LC.N_BVH_SPHERES * 9 // 10, moved
    lt, li = tab["lists"][0]
    assert len(lt) == LC.N_BVH_SPHERES and (lt == S.OBJ_SPHERE).all() and sorted(li) == list(range(LC.N_BVH_SPHERES))


def test_degenerate_primitives_are_accepted():
    """mort_add_sphere takes a zero and a negative radius and mort_add_quad a quad without area (u || v, u = 0: NaN normal); the compile
    refuses none of them, so they stay in the worlds of the sweep"""
    for name in LC.WORLDS:
        world, tab = LC.WORLDS[name]()
        assert hip.debug_light_host(world, 0, np.zeros((1, 8), np.uint32)).shape == (1,)
        assert np.isnan(tab["quads"]["normal"][LC.QUAD_PARALLEL]).all() and tab["quads"]["area"][LC.QUAD_PARALLEL] == 0
        assert np.isnan(tab["quads"]["normal"][LC.QUAD_ZERO_U]).all()
        assert (tab["spheres"]["r"] == 0).sum() == 1
    assert LC.flat_light_world()[1]["spheres"]["r"][LC.SPHERE_NEGATIVE_RADIUS] < 0


def _record(fn, typ, idx):
    rec = np.zeros((3, LC.O.LIGHT_SHAPES[fn][0]), np.uint32)
    at = 0 if fn == 0 else 6
    rec[:, at] = np.array([S.OBJ_SPHERE, typ, S.OBJ_SPHERE], np.int32).view(np.uint32)   # the refused record stands between two good ones
    rec[:, at + 1] = np.array([0, idx, 0], np.int32).view(np.uint32)
    return rec


def _nested_world():
    L = host.lib()
    w = host.World()
    mt, mi = S.MAT_DIELECTRIC, L.mort_add_dielectric(w.ptr, 1.5)
    L.mort_add_sphere(w.ptr, host.vec3(0, 0, 0), 1.0, mt, mi, False)
    inner = L.mort_add_hittable_list(w.ptr, True)
    L.mort_list_add(w.ptr, inner, S.OBJ_SPHERE, 0)
    outer = L.mort_add_hittable_list(w.ptr, True)
    L.mort_list_add(w.ptr, outer, S.OBJ_SPHERE, 0)
    L.mort_list_add(w.ptr, outer, S.OBJ_HITTABLE_LIST, inner)
    w.c.bvh_mode = False
    return w, outer


REFUSED = [("sphere_past_the_table", S.OBJ_SPHERE, 1090, -1), ("sphere_negative_index", S.OBJ_SPHERE, -1, -1), ("quad_past_the_table", S.OBJ_QUAD, 640, -1),
           ("list_past_the_lists", S.OBJ_HITTABLE_LIST, 2, -1), ("list_negative_index", S.OBJ_HITTABLE_LIST, -1, -1)]


@pytest.mark.parametrize("fn", (0, 1))
@pytest.mark.parametrize("what,typ,idx,status", REFUSED, ids=[r[0] for r in REFUSED])
def test_host_entry_refuses_what_check_light_object_refuses(what, typ, idx, status, fn):
    world, _ = LC.flat_light_world()
    with pytest.raises(hip.MortHipError) as e:
        hip.debug_light_host(world, fn, _record(fn, typ, idx))
    assert e.value.status == status


@pytest.mark.parametrize("fn", (0, 1))
def test_host_entry_refuses_nested_and_empty_lists(fn):
    w, outer = _nested_world()
    with pytest.raises(hip.MortHipError) as e:
        hip.debug_light_host(w, fn, _record(fn, S.OBJ_HITTABLE_LIST, outer))
    assert e.value.status == -6
    empty = host.World()
    L = host.lib()
    L.mort_add_sphere(empty.ptr, host.vec3(0, 0, 0), 1.0, S.MAT_DIELECTRIC, L.mort_add_dielectric(empty.ptr, 1.5), False)
    L.mort_add_hittable_list(empty.ptr, True)
    empty.c.bvh_mode = False
    with pytest.raises(hip.MortHipError) as e:
        hip.debug_light_host(empty, fn, _record(fn, S.OBJ_HITTABLE_LIST, 0))
    assert e.value.status == -1


def test_a_list_ends_with_the_entry_the_reference_reads_past_it():
    """a stream whose next curand_uniform is 1.0f makes random_int(0, 39) give 40: the oracle reads the (0, 0) mort_list_add left
    there, samples nothing and returns (1,0,0) after ONE draw; so must the library, for the list that is followed by another one (the BVH
    world's list 0) as for the last one (the flat world's list 1)"""
    for name, li in (("flat", 1), ("bvh", 0)):
        world, tab = LC.WORLDS[name]()
        n = len(tab["lists"][li][0])
        st = LC.MC._states(np.random.default_rng(1), 1 << 18)[0]
        st = st[LC.MC.xorwow_step(st.copy()) >= 0xffffff80][:64]
        assert len(st) == 64
        assert (LC._chosen_positions(st, n) == n).all()
        rec = LC.light_random_records(np.full(64, S.OBJ_HITTABLE_LIST, np.int32), np.full(64, li, np.int32), np.ones((64, 3), np.float32), st)
        want = O.light_batch(world, 1, rec)
        assert (want[:, :3] == np.array([0x3f800000, 0, 0], np.uint32)).all() and (want[:, 9] == 1).all()
        LC.assert_same(1, rec, dict(oracle=want, hipcc_host=hip.debug_light_host(world, 1, rec).reshape(64, -1)))
