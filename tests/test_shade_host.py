"""The shade step of the host compile, record by record (no GPU): debug.hip's shade table -- the closest-hit search of a radiance query's
segment and dev_shade.h's shade_hit, hipcc's host compile over a world compiled as the host loop compiles it (mort_hip_debug_shade_host),
over the item scan and over the unified tree -- against the oracle's loop body (mort_oracle_shade_batch, the function its ray_color runs).

  hipcc host, item scan  ==  hipcc host, unified tree  ==  oracle: 0 differing records of 2^18 per (world, light setting), of the ragged
  batch of 2^16 + 37 and of the batch of one; status, k, rp, final_value, the ray afterwards, the final stream words and the draw count,
  bit for bit (math_cases.canon: any NaN equals any NaN; signed zeros count).

The census (tests/shade_cases.py assert_census) is asserted on the oracle's branch words alone: every branch in at least 1000 records per
world, at most 5 % misses, at least 1 % of the records with a non-finite word.  Measured (flat / flat_zero / bvh, of 786 432 records each):
misses 16 491 / 16 085 / 27 510; a non-finite word 182 322 / 191 524 / 192 413; total internal reflection 71 643 / 69 665 / 78 300;
reflected by Schlick 28 633 / 28 474 / 32 090; refracted 118 487 / 118 229 / 128 514, with ratio exactly 1 36 323 / 35 082 / 41 971; emission
from the back face 21 901 / 21 673 / 21 286; mat_pdf == 0 32 116 / 36 658 / 44 828; rp == inf 0 / 1 541 / 4 145 and a non-finite normal 0 /
15 012 / 24 513 (flat cannot produce either, asserted); the unknown material tags 12 744 .. 18 684 each, the unknown texture tags
12 715 .. 16 104 each."""
import ctypes as C

import numpy as np
import pytest

from mort_amd import hip, structs as S
from tests import oracle_lib as O
from tests import shade_cases as SC

CASES = [(w, s) for w in SC.WORLDS for s in SC.LIGHT_SETTINGS]


def test_shape_and_tables():
    fn = hip.lib().mort_hip_debug_shade_shape
    fn.restype = C.c_int; fn.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    a, b = C.c_int(), C.c_int()
    assert fn(0, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == hip.SHADE_SHAPE == O.SHADE_SHAPE == (16, 22) and len(SC.OUT_KINDS) == 22
    assert fn(1, C.byref(a), C.byref(b)) == -1 and fn(-1, C.byref(a), C.byref(b)) == -1 and fn(0, None, C.byref(b)) == -1
    flat, zero, bvh = (SC.shade_world(n) for n in SC.WORLDS)
    assert not flat.world.c.bvh_mode and not zero.world.c.bvh_mode and bvh.world.c.bvh_mode
    assert hip.debug_gen_tree(flat.world)["tree"] and not hip.debug_gen_tree(zero.world)["tree"] and not hip.debug_gen_tree(bvh.world)["tree"]
    assert not any(flat.world.c.objs.host_sphere[i].radius == 0 for i in range(flat.world.c.objs.num_spheres))
    o = zero.world.c.objs
    assert o.num_quads >= 50 and o.num_translates >= 6 and o.num_rotate_y >= 6 and o.num_constant_medium == 2 and o.num_hittable_list == 2
    assert sum(1 for i in range(o.num_spheres) if o.host_sphere[i].moves) >= 50 and sum(1 for i in range(o.num_spheres) if o.host_sphere[i].radius < 0) >= 30
    assert sum(1 for i in range(o.num_spheres) if o.host_sphere[i].radius == 0) == 4
    assert bvh.world.c.objs.num_spheres >= 640 and bvh.world.c.objs.num_bvh == 1
    for s in (flat, zero, bvh):
        m, t = s.world.c.mats, s.world.c.texs
        assert {m.host_lambertian[i].texType for i in range(m.num_lambertians)} >= {-1, 0, 1, 2, 3, 4, 5}
        assert {m.host_diffuse_light[i].texType for i in range(m.num_diffuse_lights)} >= {1, 2, 3, 4}
        assert t.num_checker_textures >= 2 * len(SC.NESTED) and t.num_noise_textures == 1 and t.num_image_textures >= 3


def test_status_codes():
    fn = hip.lib().mort_hip_debug_shade_host
    fn.restype = C.c_int; fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    w = SC.shade_world("flat").world
    wp = C.cast(w.ptr, C.c_void_p)
    rec = np.array(SC.records("flat", "list")[0][:4])
    out = np.zeros((4, 22), np.uint32)
    assert fn(None, 0, 0, rec.ctypes.data, 4, out.ctypes.data) == -1            # NULL world
    assert fn(wp, 0, 0, None, 4, out.ctypes.data) == -1 and fn(wp, 0, 0, rec.ctypes.data, 4, None) == -1
    assert fn(wp, 1, 0, rec.ctypes.data, 4, out.ctypes.data) == -1 and fn(wp, -1, 0, rec.ctypes.data, 4, out.ctypes.data) == -1  # unknown fn
    assert fn(wp, 0, 0, None, 0, None) == 0 and fn(wp, 0, 0, rec.ctypes.data, 0, out.ctypes.data) == 0 and not out.any()       # an empty batch
    for bad in ((S.OBJ_SPHERE, 100000), (S.OBJ_QUAD, -1), (S.OBJ_HITTABLE_LIST, 2), (S.OBJ_HITTABLE_LIST, -1)):  # a bad light, in the last record
        r = rec.copy()
        r[3, 14:16] = np.array(bad, np.int32).view(np.uint32)
        assert fn(wp, 0, 0, r.ctypes.data, 4, out.ctypes.data) == -1 and not out.any(), bad
        with pytest.raises(O.OracleBatchError):
            O.shade_batch(w, r)
    nested = rec.copy()  # the first list holds the rotated box's quads: acceptable; a light tag nobody samples is accepted too
    nested[0, 14:16] = np.array((S.OBJ_TRANSLATE, 0), np.int32).view(np.uint32)
    assert fn(wp, 0, 0, nested.ctypes.data, 4, out.ctypes.data) == 0 and out.any()


@pytest.mark.parametrize("name", SC.WORLDS)
def test_census(name):
    c = SC.assert_census(name)
    print(name, c)


@pytest.mark.parametrize("name,setting", CASES)
def test_host_equals_the_oracle(name, setting):
    rec, fam = SC.records(name, setting)
    assert len(rec) == SC.N_RECORDS and all((fam == k).any() for k, f in enumerate(SC.FAMILIES) if (name != "bvh" or f not in ("quads", "boxes", "media")) and (name != "flat" or f != "zero_radius"))
    w = SC.shade_world(name).world
    SC.assert_same(rec, dict(oracle=SC.oracle(name, setting)[0], host_scan=hip.debug_shade_host(w, rec), host_tree=hip.debug_shade_host(w, rec, tree=True)))


@pytest.mark.parametrize("name", SC.WORLDS)
def test_ragged_and_single_batches(name):
    w = SC.shade_world(name).world
    rec = SC.ragged(name, "list")
    assert len(rec) == (1 << 16) + 37
    SC.assert_same(rec, dict(oracle=O.shade_batch(w, rec)[0], host_scan=hip.debug_shade_host(w, rec), host_tree=hip.debug_shade_host(w, rec, tree=True)))
    for i in (0, 12345):
        one = np.ascontiguousarray(rec[i:i + 1])
        got = hip.debug_shade_host(w, one, tree=True)
        assert got.shape == (22,)
        SC.assert_same(one, dict(oracle=O.shade_batch(w, one)[0], host=got))


def test_the_oracle_batch_is_ray_colors_own_step():
    """a two-segment path by hand from two batch calls equals mort_oracle_ray_color at bounce limit 2: the unwind over the batch's k and rp"""
    from tests import radiance_ref as R
    from mort_amd import host
    name = "flat"
    s = SC.shade_world(name)
    rec = np.array(SC.records(name, "none")[0][:4096])
    rec[:, 13] = rec[:, 12]  # ray_color scatters with the time of the ray it was given
    first, _ = O.shade_batch(s.world, rec)
    second_in = rec.copy()
    second_in[:, 0:6] = first[:, 15:21]; second_in[:, 6:13] = first[:, 8:15]
    second, _ = O.shade_batch(s.world, second_in)
    _, cam = host.build_scene(2, width=8, spp=1, depth=2)
    for k in range(3):
        cam.background.e[k] = 0.25 * (k + 1)
    cam.light_obj_type = -1
    rays = np.zeros((len(rec), 8), np.float32)
    rays[:, :7] = rec[:, 6:13].view(np.float32); rays[:, 7] = np.inf
    streams = np.zeros(len(rec), O.STATE_DTYPE)
    streams["d"] = rec[:, 0]; streams["v"] = rec[:, 1:6]
    want = R.oracle_radiance(s.world, cam, rays, streams, 1)
    bg = np.array([0.25, 0.5, 0.75], np.float32)
    f32 = lambda a: a.view(np.float32)
    with np.errstate(all="ignore"):
        def value(out, deeper):  # what a segment returns upward: background, emission, or emission 0 + (k * deeper) * rp
            st = out[:, 0:1]
            sc = np.float32(0) + f32(out[:, 4:5]) * (f32(out[:, 1:4]) * deeper)
            sc = np.where(st == SC.STATUS_IDENTITY, np.float32(0) + deeper, sc)
            return np.where(st == SC.STATUS_MISS, bg, np.where(st == SC.STATUS_END, f32(out[:, 5:8]), sc)).astype(np.float32)
        got = value(first, value(second, np.zeros((len(rec), 3), np.float32)))
    from tests.query_rays import _words
    assert (_words(got) == _words(want)).all(), int((_words(got) != _words(want)).any(1).sum())
    assert (streams["d"] == np.where(first[:, 0] >= 2, second[:, 15], first[:, 15])).all()
