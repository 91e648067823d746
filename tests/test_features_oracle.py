"""The first-hit feature pass in its host form -- the body the gfx950 feat_kernel runs (dev_features.h) --
against tests/feature_ref.py, a restatement of the contract made from the CPU oracle's entry points only.  Albedo, normal
and depth are compared as raw 32-bit words on every pixel, item scan and unified-tree walk alike: tolerance 0.  Every case
also asserts that the frame shows what the case is for, so none passes on background alone."""
import numpy as np
import pytest

from mort_amd import hip, host, structs as S
from tests import oracle_lib as O
from tests.feature_ref import MEDIUM, MISS, SOLID, assert_same_words, oracle_features, primary_rays
from tests.worlds import (BVH_WORLDS, FLAT_WORLDS, GEN_FAR_VIEW, PLACED, bvh_camera, bvh_scene_views, custom_bvh_world, flat_camera, flat_world,
                          gen_scene_views, random_world, set_view)

NT = 16


def check(world, cam, what, walks=None):
    """both traversals against the reference; walks: expected 'unified tree' in the render's kernel name for tree=True"""
    ref = oracle_features(world, cam, nthreads=NT)
    for tree in (False, True):
        assert_same_words(hip.render_features_host(world, cam, nthreads=NT, tree=tree), ref, f"{what}, tree={tree}")
    if walks is not None:
        assert tree_walks(world, cam) == walks, f"{what}: which walk ran"
    return ref


def tree_walks(world, cam):
    """the feature call does not report which walk ran; the render applies the same test (tree built, camera within its reach)"""
    small = type(cam).from_buffer_copy(cam)
    small.samples_per_pixel, small.sqrt_spp, small.recip_sqrt_spp, small.pixel_samples_scale, small.bounce_limit = 1, 1, 1.0, 1.0, 1
    name = hip.render_host(world, small, nthreads=NT, tree=True)["stats"]["kernel_name"]
    assert "unified tree" in name or "item scan" in name, name
    return "unified tree" in name


def count(ref, kind):
    return int((ref["kind"] == kind).sum())


# ---- the ten built-in scenes ----
@pytest.mark.parametrize("sid,width", [(s, 160) for s in range(1, 11)] + [(6, 400), (8, 400)])
def test_scene_features_equal_the_oracle(sid, width):
    world, cam = host.build_scene(sid, width=width, spp=1)
    ref = check(world, cam, f"scene {sid} at {width} px", walks=sid not in (1, 10))
    px = ref["kind"].size
    assert count(ref, SOLID) > (0.005 if sid == 10 else 0.3) * px
    o = world.c.objs
    if sid in (6, 8, 9):  # instanced geometry: pixels whose winner is a translate -> rotate_y chain
        assert o.num_translates >= 1 and on_object(world, cam, ref, S.OBJ_TRANSLATE, 0) > 0.01 * px
    if sid in (1, 8, 9):
        assert moving_sphere_pixels(world, cam, ref) > 20
    if sid == 7:
        assert count(ref, MEDIUM) > 0.1 * px, "the two smoke boxes under their chains"
    if sid in (8, 9):
        assert (ref["started_inside"] >= 1).all(), "the camera sits inside the fog shell"
        assert count(ref, MISS) == 0 and (ref["depth"] > 1).all(), "geometry, not the fog 1 cm before the lens"
    if sid in (3, 4):  # the earth image, Perlin noise
        assert len(np.unique(ref["albedo"][ref["kind"] == SOLID], axis=0)) > 100, "textured albedo"


def on_object(world, cam, ref, obj_type, obj_idx, time=None):
    """how many pixels' first hit is this object's own hit (same t as hitDispatch on it alone)"""
    rays = primary_rays(cam)
    if time is not None:
        rays[:, 6] = time
    rec, hit = O.object_hit_batch(world, obj_type, obj_idx, rays, 0.001, np.inf, nthreads=NT)
    return int((hit & (ref["kind"].reshape(-1) == SOLID) & (rec["t"] == ref["t"].reshape(-1))).sum())


def moving_sphere_pixels(world, cam, ref):
    o = world.c.objs
    movers = [i for i in range(o.num_spheres) if o.host_sphere[i].moves]
    assert movers
    at_half = sum(on_object(world, cam, ref, S.OBJ_SPHERE, i) for i in movers)
    at_zero = sum(on_object(world, cam, ref, S.OBJ_SPHERE, i, time=0.0) for i in movers)
    assert at_zero < at_half, "time 0 would put the moving spheres elsewhere"
    return at_half


# ---- the awkward hand-built worlds ----
@pytest.mark.parametrize("name", sorted(FLAT_WORLDS))
def test_flat_world_features_equal_the_oracle(name):
    spec = FLAT_WORLDS[name]
    w, ids = flat_world(spec["prims"], media=spec.get("media", ()), late_list=spec.get("late_list", False))
    cam = flat_camera(light=ids[spec["light"][1]] if spec.get("light") else None, spp=1)
    ref = check(w, cam, name, walks=name != "media_then_list")
    px = ref["kind"].size
    if name == "empty":
        assert count(ref, MISS) == px
    else:
        assert count(ref, SOLID) > 0.02 * px
    if spec.get("media"):
        assert count(ref, MEDIUM) > 0.02 * px
    if name == "coincident":  # equal t: the scan's last-wins rule picks the albedo
        alb = ref["albedo"].reshape(-1, 3)
        for rgb in ((.1 * 3, .2, .5), (.2 * 2, .5, .2)):
            assert (alb == np.array(rgb, dtype=np.float32)).all(-1).sum() > 0.01 * px, f"the last of the coincident primitives {rgb} wins"
        for rgb in ((.1 * 0, .2, .5), (.2 * 0, .5, .2)):
            assert not (alb == np.array(rgb, dtype=np.float32)).all(-1).any(), f"the first of the coincident primitives {rgb} never shows"
    if name == "every_material_lit_by_sphere":
        assert set(np.unique(ref["mat_type"])) == {0, S.MAT_LAMBERTIAN, S.MAT_METAL, S.MAT_DIELECTRIC, S.MAT_DIFFUSE_LIGHT, S.MAT_ISOTROPIC}
    if name == "boxes_and_instances":
        assert on_object(w, cam, ref, S.OBJ_TRANSLATE, 0) > 0.005 * px


@pytest.mark.parametrize("name", sorted(BVH_WORLDS))
def test_bvh_world_features_equal_the_oracle(name):
    w = custom_bvh_world(BVH_WORLDS[name])
    cam = bvh_camera(spp=1)
    ref = check(w, cam, name, walks=False)  # a reference BVH: run_bvh through the item scan
    px = ref["kind"].size
    assert count(ref, SOLID) > 0.03 * px
    if name == "every_material":
        assert set(np.unique(ref["mat_type"])) == {0, S.MAT_LAMBERTIAN, S.MAT_METAL, S.MAT_DIELECTRIC, S.MAT_DIFFUSE_LIGHT, S.MAT_ISOTROPIC}


# ---- other viewpoints ----
@pytest.mark.parametrize("sid", [1, 10])
def test_bvh_scene_viewpoints_equal_the_oracle(sid):
    world, cam = host.build_scene(sid, width=120, spp=1)
    hits = []
    for k, (frm, at, vfov, defocus) in enumerate(bvh_scene_views(sid)):
        set_view(cam, frm, at, vfov=vfov, defocus=defocus)
        ref = check(world, cam, f"scene {sid} view {k}", walks=False)
        hits.append(count(ref, SOLID))
    px = cam.image_width * cam.image_height
    if sid == 1:
        assert sum(h > 0 for h in hits) >= len(hits) - 2 and max(hits) > 0.5 * px, hits
    else:  # scene 10 is sparse
        assert sum(h > 0 for h in hits) >= 3 and sum(hits) > 0.02 * px, hits


@pytest.mark.parametrize("sid", [6, 7, 9])
def test_gen_scene_viewpoints_equal_the_oracle(sid):
    world, cam = host.build_scene(sid, width=72, spp=1)
    hits, media = [], 0
    for k, (frm, at, vfov, defocus) in enumerate(gen_scene_views(sid)):
        set_view(cam, frm, at, vfov=vfov, defocus=defocus)
        ref = check(world, cam, f"scene {sid} view {k}", walks=k != GEN_FAR_VIEW)  # beyond the tree's reach: the scan
        hits.append(count(ref, SOLID))
        media += count(ref, MEDIUM)
        if sid == 9 and k != GEN_FAR_VIEW:
            assert (ref["depth"][ref["kind"] != MISS] > 1).all()
    assert sum(h > 0 for h in hits) >= len(hits) - 1, hits
    if sid == 7:
        assert media > 500, "smoke boxes seen from the other viewpoints"


# ---- random worlds (the 40 of tests/test_host_mode.py, from that test's four views) ----
@pytest.mark.parametrize("seed", range(40))
def test_random_world_features_equal_the_oracle(seed):
    rng = np.random.default_rng(1000 + seed)
    w, light = random_world(rng, n_spheres=int(rng.integers(1, 60)), n_quads=int(rng.integers(0, 12)), n_boxes=int(rng.integers(0, 3)),
                            n_media=int(rng.integers(0, 3)), with_light=bool(seed % 2))
    _, cam = host.build_scene(2, width=56, spp=1, depth=int(rng.integers(2, 20)))
    for i in range(3):
        cam.background.e[i] = float(rng.uniform(0.0, 0.8)) * (0 if light and seed % 4 == 1 else 1)
    views = [((0, 2, 9), (0, 1, 0)), ((0.3, 0.05, 0.2), (4, 0.3, 1)), ((40, 25, -60), (0, 0, 0)), (tuple(rng.uniform(-5, 5, 3) + (0, 6, 0)), tuple(rng.uniform(-2, 2, 3)))]
    solid = 0
    for k, (frm, at) in enumerate(views):
        set_view(cam, frm, at, vfov=int(rng.integers(20, 90)), defocus=float(rng.choice([0.0, 0.0, 0.8])))
        solid += count(check(w, cam, f"random world {seed} view {k}", walks=True), SOLID)
    assert solid > 0.3 * 4 * cam.image_width * cam.image_height


# ---- cameras placed on purpose ----
def _centre(ref, key):
    H, W = ref["kind"].shape
    return ref[key][H // 2, W // 2]


def _placed_inside_small_medium(w, cam, ref):
    assert (ref["started_inside"] == 1).all() and count(ref, MEDIUM) == 0, "a ray that starts inside a medium does not enter it"
    assert count(ref, SOLID) > 1000 and count(ref, MISS) > 1000, "the sphere behind the smoke and the background around it"


def _placed_fog_cluster(w, cam, ref):
    assert (ref["started_inside"] >= 1).all() and (ref["depth"] > 1).all()
    assert on_object(w, cam, ref, S.OBJ_TRANSLATE, 0) > 1000, "the sphere cluster under rotate_y and translate"


def _placed_fog_moving_sphere(w, cam, ref):
    assert (ref["started_inside"] >= 1).all() and (ref["depth"] > 1).all()
    assert moving_sphere_pixels(w, cam, ref) > 300
    assert _centre(ref, "mat_type") == S.MAT_LAMBERTIAN


def _placed_solid_before_medium(w, cam, ref):
    assert _centre(ref, "kind") == SOLID and count(ref, SOLID) > 50 and count(ref, MEDIUM) > 200, "the solid hides the medium behind it, not around it"


def _placed_solid_inside_medium(w, cam, ref):
    assert _centre(ref, "kind") == MEDIUM and count(ref, SOLID) == 0 and count(ref, MEDIUM) > 200


def _placed_solid_behind_medium(w, cam, ref):
    assert _centre(ref, "kind") == MEDIUM and count(ref, MEDIUM) > 200 and count(ref, SOLID) > 50, "the solid shows around the medium only"


def _placed_grazed_medium(w, cam, ref):
    assert (ref["grazed"] > 0).sum() >= 1 and not ((ref["grazed"] > 0) & (ref["kind"] == MEDIUM)).any(), "a chord below 0.0001 is no hit"
    assert count(ref, MEDIUM) > 1000 and count(ref, MISS) > 1000
    assert not tree_walks(w, cam), "this far away the pass takes the scan"


def _placed_quad_from_behind(w, cam, ref):
    hit = ref["kind"] == SOLID
    assert hit.sum() > 300 and not ref["front_face"][hit].any()
    d = primary_rays(cam)[:, 3:6].reshape(ref["normal"].shape)
    assert ((ref["normal"] * d).sum(-1)[hit] < 0).all(), "the normal of a back face is turned towards the camera"


def _placed_inside_glass_sphere(w, cam, ref):
    assert count(ref, SOLID) == ref["kind"].size and (ref["mat_type"] == S.MAT_DIELECTRIC).all() and not ref["front_face"].any()
    assert (ref["albedo"] == 1).all()


def _placed_camera_on_surface(w, cam, ref):
    hit = ref["kind"] == SOLID
    assert hit.sum() > 1000 and count(ref, MISS) > 1000
    assert (ref["t"][hit] >= np.float32(0.001)).all() and not ref["front_face"][hit].any(), "the root at the lens is below t_min: the far side is hit from inside"


@pytest.mark.parametrize("name", sorted(PLACED))
def test_placed_camera_features_equal_the_oracle(name):
    w, cam = PLACED[name]()
    ref = check(w, cam, name)
    globals()["_placed_" + name](w, cam, ref)


# ---- the oracle's batched entry points against its single calls ----
def test_oracle_batches_equal_single_calls():
    import ctypes as C
    world, cam = host.build_scene(7, width=24, spp=1)
    rays = primary_rays(cam)[::2][:300].copy()
    rays[:, 6] = np.linspace(0, 1, len(rays), dtype=np.float32)
    n = len(rays)
    lo = np.where(np.arange(n) % 3 == 0, 0.001, 100.0).astype(np.float32)
    hi = np.where(np.arange(n) % 5 == 0, 900.0, np.inf).astype(np.float32)
    streams = O.seed_states(7, n, 1)
    single = streams.copy()
    rec, hit = O.world_hit_batch(world, rays, lo, hi, states=streams, nthreads=5)
    media = 0
    for i in range(n):
        h = O.Hit()
        got = O.lib().mort_oracle_world_hit(world.ptr, rays[i].ctypes.data_as(C.POINTER(C.c_float)), lo[i], hi[i],
                                            C.cast(single[i:i + 1].ctypes.data, C.POINTER(S.RngState)), C.byref(h))
        assert bool(got) == bool(hit[i])
        if got:
            assert (h.t, h.u, h.v, h.mat_type, h.mat_idx, bool(h.front_face)) == (rec["t"][i], rec["u"][i], rec["v"][i], rec["mat_type"][i],
                                                                                  rec["mat_idx"][i], bool(rec["front_face"][i]))
            assert list(h.p.e) == list(rec["p"][i]) and list(h.normal.e) == list(rec["normal"][i])
            media += h.mat_type == world.c.objs.host_constant_medium[0].mat_type and h.normal.e[0] == 1.0 and h.front_face
    assert streams.tobytes() == single.tobytes(), "the streams advance as in the single calls"
    assert hit.sum() > 100 and media > 5 and (streams != O.seed_states(7, n, 1)).any()
    # one object alone: the first smoke box's boundary (a list under rotate_y and translate)
    cm = world.c.objs.host_constant_medium[0]
    r1, h1 = O.object_hit_batch(world, cm.obj_type, cm.obj_idx, rays, -np.inf, np.inf, nthreads=3)
    r2, h2 = O.object_hit_batch(world, cm.obj_type, cm.obj_idx, rays, -np.inf, np.inf, nthreads=1)
    assert h1.sum() > 5 and (h1 == h2).all() and r1.tobytes() == r2.tobytes()
    # a call that would draw without a stream is refused, and so are objects that do not exist
    for call in (lambda: O.world_hit_batch(world, rays, 0.001, np.inf), lambda: O.object_hit_batch(world, S.OBJ_CONSTANT_MEDIUM, 0, rays, 0.001, np.inf)):
        with pytest.raises(O.OracleBatchError) as e:
            call()
        assert e.value.status == O.BATCH_NO_STREAM
    with pytest.raises(O.OracleBatchError) as e:
        O.object_hit_batch(world, S.OBJ_SPHERE, 0, rays, 0.001, np.inf)  # scene 7 has no sphere
    assert e.value.status == -1
    pts = rec["p"][hit][:50]
    one = np.zeros(3, dtype=np.float32)
    fp = C.POINTER(C.c_float)
    batch = O.texture_value_batch(world, S.TEXTURE_SOLID, 2, 0.25, 0.5, pts)
    for k in range(len(pts)):
        O.lib().mort_oracle_texture_value(world.ptr, S.TEXTURE_SOLID, 2, 0.25, 0.5, pts[k].ctypes.data_as(fp), one.ctypes.data_as(fp))
        assert (one == batch[k]).all()
