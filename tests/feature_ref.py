"""An independent reference for the first-hit feature pass (include/mort_hip.h): the contract restated with
the CPU oracle's entry points and numpy float32 arithmetic.  Nothing here calls libmort_hip.so, so a mistake in the pass's
body (dev_features.h and the traversal pieces it shares with the render) does not repeat itself on this side.

Every float operation below is a single IEEE float32 operation in the order the contract states it (numpy does not
contract a * b + c), so the result is meant to equal the pass's bit for bit."""
import numpy as np

from mort_amd import structs as S
from tests import oracle_lib as O

F = np.float32
T_MIN = F(0.001)
MISS, SOLID, MEDIUM = 0, 1, 2


def _v(v):
    return np.array([v.e[0], v.e[1], v.e[2]], dtype=F)


def primary_rays(cam):
    """(H * W, 7) float32: origin cam.center, direction ((pixel00 + float(x) * du) + float(y) * dv) - center, time 0.5."""
    W, H = cam.image_width, cam.image_height
    c, p00, du, dv = _v(cam.center), _v(cam.pixel00_loc), _v(cam.pixel_delta_u), _v(cam.pixel_delta_v)
    xs = np.arange(W, dtype=F)[None, :, None]
    ys = np.arange(H, dtype=F)[:, None, None]
    d = ((p00 + xs * du) + ys * dv) - c
    assert d.dtype == F
    rays = np.empty((H, W, 7), dtype=F)
    rays[..., 0:3] = c
    rays[..., 3:6] = d
    rays[..., 6] = F(0.5)
    return rays.reshape(-1, 7)


def _vlen(d):
    """sqrt(x * x + y * y + z * z), summed left to right in float32"""
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def _some_streams(n):
    """n arbitrary XORWOW streams: the solid pass must leave them as they are"""
    base = O.seed_states(S.DEFAULT_SEED, 64, 1)
    return np.ascontiguousarray(np.resize(base, n))


def media_in_scan_order(world):
    """[(medium, path)] for every constant medium world::hit reaches, in the order it reaches them (world.cuh:122-168: translates,
    rotate_ys, media, lists, each table's entries without `skip`); path: the (type, index) of the transforms around the medium,
    outermost first.  A medium bounded by a medium is not followed."""
    o = world.c.objs
    found = []
    if world.c.bvh_mode:  # world::hit returns after the BVHs
        return found

    def walk(t, i, path):
        if t == S.OBJ_TRANSLATE and 0 <= i < o.num_translates:
            walk(o.host_translate[i].obj_type, o.host_translate[i].obj_idx, path + [(t, i)])
        elif t == S.OBJ_ROTATE_Y and 0 <= i < o.num_rotate_y:
            walk(o.host_rotate_y[i].obj_type, o.host_rotate_y[i].obj_idx, path + [(t, i)])
        elif t == S.OBJ_CONSTANT_MEDIUM and 0 <= i < o.num_constant_medium:
            found.append((i, path))
        elif t == S.OBJ_HITTABLE_LIST and 0 <= i < o.num_hittable_list:
            lst = o.host_hittable_list[i]
            for k in range(lst.num_objs):
                walk(lst.obj_types[k], lst.obj_idxs[k], path)

    for i in range(o.num_translates):
        if not o.host_translate[i].skip:
            walk(S.OBJ_TRANSLATE, i, [])
    for i in range(o.num_rotate_y):
        if not o.host_rotate_y[i].skip:
            walk(S.OBJ_ROTATE_Y, i, [])
    found += [(i, []) for i in range(o.num_constant_medium) if not o.host_constant_medium[i].skip]
    for i in range(o.num_hittable_list):
        if not o.host_hittable_list[i].skip:
            walk(S.OBJ_HITTABLE_LIST, i, [])
    return found


def oracle_features(world, cam, nthreads=16):
    """dict(albedo (H, W, 3), normal (H, W, 3), depth (H, W)) float32 as the contract defines them, plus what the tests assert
    their cases on: kind (H, W) of MISS / SOLID / MEDIUM, mat_type, front_face, t, and started_inside (H, W) = the number of
    media the ray starts inside (passed over by the rule below), and grazed (H, W) = the number of media whose boundary the
    ray meets once only."""
    W, H = cam.image_width, cam.image_height
    o, m = world.c.objs, world.c.mats
    rays = primary_rays(cam)
    n = rays.shape[0]
    d = rays[:, 3:6]
    inf = F(np.inf)

    # solids: world::hit with every constant medium passed over, so no random number is drawn.  A medium the scan reaches through a
    # transform or a list has no skip flag that counts, so each medium's boundary reference is set to a tag hitDispatch does not
    # know for the call: constant_medium::hit then returns at its first boundary test, before it draws
    media = media_in_scan_order(world)
    streams = _some_streams(n)
    before = streams.copy()
    bounds = [(o.host_constant_medium[i].obj_type, o.host_constant_medium[i].obj_idx) for i in range(o.num_constant_medium)]
    try:
        for i in range(o.num_constant_medium):
            o.host_constant_medium[i].obj_type = 0
        rec, hit = O.world_hit_batch(world, rays, T_MIN, inf, states=streams, nthreads=nthreads)
    finally:
        for i, (bt, bi) in enumerate(bounds):
            o.host_constant_medium[i].obj_type = bt
    assert streams.tobytes() == before.tobytes(), "the solid pass drew a random number"

    kind = np.where(hit, SOLID, MISS).astype(np.int32)
    closest = np.where(hit, rec["t"], inf).astype(F)
    normal = np.where(hit[:, None], rec["normal"], F(0)).astype(F)
    p = rec["p"].copy()
    u, v = rec["u"].copy(), rec["v"].copy()
    mat_type, mat_idx = rec["mat_type"].copy(), rec["mat_idx"].copy()
    front = rec["front_face"].astype(bool) & hit
    started_inside = np.zeros(n, dtype=np.int32)
    grazed = np.zeros(n, dtype=np.int32)

    # media in scan order after the solids: constant_medium::hit's interval from the boundary object alone, no distance drawn
    if media:
        dlen = _vlen(d)
        inv = F(1) / dlen
        minus_unit = -(inv[:, None] * d)
        assert minus_unit.dtype == F
    for i, path in media:
        cm = o.host_constant_medium[i]
        # a medium under transforms: the outermost is dispatched on with the innermost holding the boundary in the medium's place, so
        # the ray reaches the boundary through the oracle's own translate::hit / rotate_y::hit (t is the same in every frame)
        entry = path[0] if path else (cm.obj_type, cm.obj_idx)
        holder = (o.host_translate if path[-1][0] == S.OBJ_TRANSLATE else o.host_rotate_y)[path[-1][1]] if path else None
        try:
            if holder is not None:
                holder.obj_type, holder.obj_idx = cm.obj_type, cm.obj_idx
            r1, h1 = O.object_hit_batch(world, entry[0], entry[1], rays, -inf, inf, nthreads=nthreads)
            t1 = r1["t"]
            lo2 = (t1.astype(np.float64) + 0.0001).astype(F)
            r2, h2 = O.object_hit_batch(world, entry[0], entry[1], rays, np.where(h1, lo2, inf), inf, nthreads=nthreads)
        finally:
            if holder is not None:
                holder.obj_type, holder.obj_idx = S.OBJ_CONSTANT_MEDIUM, i
        both = h1 & h2
        grazed += h1 & ~h2  # no second boundary hit beyond t1 + 0.0001
        inside = both & (t1 < T_MIN)  # the ray starts inside this medium: it does not enter it, so it is no first hit
        started_inside += inside
        t2 = np.where(r2["t"] > closest, closest, r2["t"])
        acc = both & ~inside & (t1 < t2)
        closest = np.where(acc, t1, closest).astype(F)
        kind[acc] = MEDIUM
        normal[acc] = minus_unit[acc]
        p[acc] = (rays[acc, 0:3] + t1[acc, None] * d[acc]).astype(F)
        u[acc] = 0; v[acc] = 0
        mat_type[acc] = cm.mat_type; mat_idx[acc] = cm.mat_idx
        front[acc] = True

    # albedo by material kind
    albedo = np.empty((n, 3), dtype=F)
    albedo[:] = _v(cam.background)
    any_hit = kind != MISS
    albedo[any_hit] = F(1)  # dielectric, diffuse_light
    tex_type = np.zeros(n, dtype=np.int32)
    tex_idx = np.zeros(n, dtype=np.int32)
    for mt, arr in ((S.MAT_LAMBERTIAN, m.host_lambertian), (S.MAT_ISOTROPIC, m.host_isotropic)):
        for k in np.unique(mat_idx[any_hit & (mat_type == mt)]):
            sel = any_hit & (mat_type == mt) & (mat_idx == k)
            tex_type[sel] = arr[int(k)].texType
            tex_idx[sel] = arr[int(k)].texIdx
    textured = any_hit & ((mat_type == S.MAT_LAMBERTIAN) | (mat_type == S.MAT_ISOTROPIC))
    if textured.any():
        albedo[textured] = O.texture_value_batch(world, tex_type[textured], tex_idx[textured], u[textured], v[textured], p[textured])
    metal = any_hit & (mat_type == S.MAT_METAL)
    if metal.any():
        for k in np.unique(mat_idx[metal]):
            albedo[metal & (mat_idx == k)] = _v(m.host_metal[int(k)].albedo)

    depth = np.where(any_hit, closest * _vlen(d), F(0)).astype(F)
    return dict(albedo=albedo.reshape(H, W, 3), normal=normal.reshape(H, W, 3), depth=depth.reshape(H, W),
                kind=kind.reshape(H, W), mat_type=np.where(any_hit, mat_type, 0).reshape(H, W), front_face=front.reshape(H, W),
                t=np.where(any_hit, closest, F(0)).reshape(H, W), started_inside=started_inside.reshape(H, W), grazed=grazed.reshape(H, W))


KEYS = ("albedo", "normal", "depth")


def differing_words(got, ref):
    """per buffer: how many float32 words differ as raw bits"""
    return {k: int((np.ascontiguousarray(got[k]).view(np.uint32) != np.ascontiguousarray(ref[k]).view(np.uint32)).sum()) for k in KEYS}


def assert_same_words(got, ref, what=""):
    diff = differing_words(got, ref)
    if any(diff.values()):
        k = next(k for k in KEYS if diff[k])
        bad = np.argwhere(np.ascontiguousarray(got[k]).view(np.uint32) != np.ascontiguousarray(ref[k]).view(np.uint32))[0]
        y, x = int(bad[0]), int(bad[1])
        raise AssertionError(f"{what}: differing words {diff}; first in {k} at pixel (x={x}, y={y}): got {got[k][y, x]!r}, "
                             f"reference {ref[k][y, x]!r} (kind {ref['kind'][y, x]}, material {ref['mat_type'][y, x]})")
