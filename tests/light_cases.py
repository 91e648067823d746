"""Worlds and records for the light-sampling sweep (tests/test_light_host.py, tests/test_gpu_light.py, tests/test_reference_pin.py):
light_pdf_value and light_random of dev_render.h, record by record, against the oracle's pdf_value_dispatch / random_dispatch.

Two seeded worlds whose tables are near their capacity: a flat one (every primitive skipped by the world scan: only the world-order
tables and the lists matter here) and one whose list 0 is the source of a reference BVH, built over spheres added in an order the build
changes (mort_add_bvh swaps the sphere records themselves, so a world index names another sphere afterwards).  Records are 2^20 per
function and world, in the layout of debug.hip's light table; every record carries its family labels, and the census conditions are
asserted on the oracle's answers alone, before anything is compared."""
import ctypes as C
import functools

import numpy as np

from mort_amd import hip, host, structs as S
from tests import math_cases as MC
from tests import oracle_lib as O

F, U = np.float32, np.uint32
N_RECORDS = 1 << 20
RAGGED = (1 << 16) + 37
NAMES = ("light_pdf_value", "light_random")
OUT_KINDS = ("f", "fff" + "i" * 7)

SPHERE_DTYPE = np.dtype(dict(names=["c", "r", "moves", "cv", "mat_type", "mat_idx", "idx", "skip", "bbox"],
                             formats=[("<f4", (3,)), "<f4", "u1", ("<f4", (3,)), "<i4", "<i4", "<i4", "u1", ("<f4", (6,))],
                             offsets=[0, 12, 16, 20, 32, 36, 40, 44, 48], itemsize=72))
QUAD_DTYPE = np.dtype(dict(names=["Q", "u", "v", "normal", "w", "bbox", "D", "area", "mat_type", "mat_idx", "idx", "skip"],
                           formats=[("<f4", (3,))] * 5 + [("<f4", (6,)), "<f4", "<f4", "<i4", "<i4", "<i4", "u1"],
                           offsets=[0, 12, 24, 36, 48, 60, 84, 88, 92, 96, 100, 104], itemsize=108))
assert SPHERE_DTYPE.itemsize == C.sizeof(S.Sphere) and QUAD_DTYPE.itemsize == C.sizeof(S.Quad)

# fixed places in the tables (flat world; the BVH world keeps its specials outside the tree, see bvh_light_world)
SPHERE_ZERO_RADIUS, SPHERE_NEGATIVE_RADIUS = 1, 2
QUAD_PARALLEL, QUAD_ZERO_U = 1, 2          # u || v (area 0, NaN normal); u = 0
N_AXIS_QUADS = 96                          # quads 8 .. 8 + N_AXIS_QUADS - 1 lie in a coordinate plane: an origin can be IN that plane exactly
AXIS_QUAD_FIRST = 8
FOREIGN_TAGS = (-1, 0, S.OBJ_TRANSLATE, S.OBJ_ROTATE_Y, S.OBJ_CONSTANT_MEDIUM, S.OBJ_BVH, 8)
BIG_LIST_MEMBERS = 40
SEEN_R = 2e-3                              # census: spheres whose far side is beyond t_min = 0.001 from any origin outside them


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _materials(w):
    L = host.lib()
    col = L.mort_add_solid_color(w.ptr, host.vec3(.6, .5, .4))
    hot = L.mort_add_solid_color(w.ptr, host.vec3(7, 7, 7))
    return [(S.MAT_LAMBERTIAN, L.mort_add_lambertian(w.ptr, S.TEXTURE_SOLID, col)),
            (S.MAT_DIFFUSE_LIGHT, L.mort_add_diffuse_light(w.ptr, S.TEXTURE_SOLID, hot)),
            (S.MAT_DIELECTRIC, L.mort_add_dielectric(w.ptr, 1.5)),          # a light object need not emit
            (S.MAT_METAL, L.mort_add_metal(w.ptr, host.vec3(.8, .8, .8), 0.1))]


def _add_spheres(w, rng, n, mats, special, skip=True):
    """n spheres, radii 1e-4 .. 1e4 (log-uniform), a quarter moving, centres within 30 radii of the world origin so that a float next to a
    surface is still a small fraction of the radius; special: {position: radius}"""
    L = host.lib()
    ids = []
    for i in range(n):
        r = float(F(special[i])) if i in special else float(F(10.0 ** rng.uniform(-4, 4)))
        scale = abs(r) if r else 1.0
        c = rng.uniform(-30, 30, 3) * scale
        mt, mi = mats[int(rng.integers(0, len(mats)))]
        if i not in special and rng.random() < 0.25:
            ids.append(L.mort_add_moving_sphere(w.ptr, host.vec3(*c), host.vec3(*(c + rng.uniform(-2, 2, 3) * scale)), r, mt, mi, skip))
        else:
            ids.append(L.mort_add_sphere(w.ptr, host.vec3(*c), r, mt, mi, skip))
    assert min(ids) >= 0
    return ids


def _add_quads(w, rng, n, mats):
    """n quads: one side 1e-4 .. 1e4, the other within a factor of five of it (areas 1e-8 .. 1e8; a thinner quad is missed by rays aimed at
    it, the hit point's rounding being wider than the quad), u and v 20 .. 160 degrees apart; QUAD_PARALLEL, QUAD_ZERO_U; the axis quads"""
    L = host.lib()
    for i in range(n):
        lu = 10.0 ** rng.uniform(-4, 4)
        lv = lu * 10.0 ** rng.uniform(-0.7, 0.7)
        size = max(lu, lv)
        mt, mi = mats[int(rng.integers(0, len(mats)))]
        if AXIS_QUAD_FIRST <= i < AXIS_QUAD_FIRST + N_AXIS_QUADS:
            k = i % 3
            u, v = np.zeros(3), np.zeros(3)
            u[(k + 1) % 3] = lu * rng.choice([-1, 1])
            v[(k + 2) % 3] = lv * rng.choice([-1, 1])
            v[(k + 1) % 3] = lv * rng.uniform(-0.8, 0.8)       # skewed within the plane
        else:
            u = _unit(rng, 1)[0] * lu
            t = _unit(rng, 1)[0]
            t -= t.dot(u) * u / (lu * lu)
            t /= np.linalg.norm(t)
            phi = np.radians(rng.uniform(20, 160))
            v = lv * (np.cos(phi) * u / lu + np.sin(phi) * t)
        if i == QUAD_PARALLEL:
            v = 2.0 * np.asarray(F(u), dtype=np.float64)      # exactly parallel in float32: the cross product is exactly 0
        if i == QUAD_ZERO_U:
            u = np.zeros(3)
        Q = rng.uniform(-30, 30, 3) * size
        assert L.mort_add_quad(w.ptr, host.vec3(*Q), host.vec3(*u), host.vec3(*v), mt, mi, True) == i


def _tables(w):
    o = w.c.objs
    sph = np.frombuffer(C.string_at(C.cast(o.host_sphere, C.c_void_p).value, o.num_spheres * 72), dtype=SPHERE_DTYPE).copy()
    qd = np.frombuffer(C.string_at(C.cast(o.host_quad, C.c_void_p).value, o.num_quads * 108), dtype=QUAD_DTYPE).copy()
    lists = []
    for i in range(o.num_hittable_list):
        l = o.host_hittable_list[i]
        lists.append((np.array(l.obj_types[: l.num_objs], np.int32), np.array(l.obj_idxs[: l.num_objs], np.int32)))
    return dict(spheres=sph, quads=qd, lists=lists)


@functools.lru_cache(maxsize=None)
def flat_light_world():
    """(world, tables): 1090 spheres and 640 quads, all skipped by the scan but one ground sphere; list 0 holds one quad; list 1 holds
    BIG_LIST_MEMBERS members of every kind a list may hold but a list: spheres (static, moving, non-emissive), quads (the degenerate ones
    among them), a translate, a rotate_y, a constant medium and a BVH tag"""
    L = host.lib()
    rng = np.random.default_rng(20260101)
    w = host.World()
    mats = _materials(w)
    _add_spheres(w, rng, 1, mats, {0: 100.0}, skip=False)                      # sphere 0: the one thing the scan sees
    _add_spheres(w, rng, 1089, mats, {0: 0.0, 1: -1.5, 2: 1e-3})               # positions 1, 2, 3 of the table
    _add_quads(w, rng, 640, mats)
    tr = L.mort_add_translate(w.ptr, S.OBJ_SPHERE, 5, host.vec3(1, 2, 3), True)
    ro = L.mort_add_rotate_y(w.ptr, S.OBJ_QUAD, 20, 30.0, True)
    med = L.mort_add_constant_medium(w.ptr, S.OBJ_SPHERE, 6, 0.5, mats[0][0], mats[0][1], True)
    one = L.mort_add_hittable_list(w.ptr, True)
    L.mort_list_add(w.ptr, one, S.OBJ_QUAD, 200)
    big = L.mort_add_hittable_list(w.ptr, True)
    sph = _tables(w)["spheres"]
    moving = [int(i) for i in np.flatnonzero(sph["moves"])[:4]]
    members = [(S.OBJ_SPHERE, 10), (S.OBJ_QUAD, 30), (S.OBJ_TRANSLATE, tr), (S.OBJ_SPHERE, moving[0]), (S.OBJ_QUAD, QUAD_PARALLEL), (S.OBJ_ROTATE_Y, ro),
               (S.OBJ_QUAD, AXIS_QUAD_FIRST), (S.OBJ_CONSTANT_MEDIUM, med), (S.OBJ_SPHERE, SPHERE_ZERO_RADIUS), (S.OBJ_BVH, 0), (S.OBJ_QUAD, QUAD_ZERO_U),
               (S.OBJ_SPHERE, moving[1])]
    while len(members) < BIG_LIST_MEMBERS:
        members.append((S.OBJ_SPHERE, int(rng.integers(4, 1090))) if rng.random() < 0.5 else (S.OBJ_QUAD, int(rng.integers(3, 640))))
    for t, i in members:
        assert L.mort_list_add(w.ptr, big, t, i) == 0
    w.c.bvh_mode = False
    return w, _tables(w)


N_BVH_SPHERES = 500


@functools.lru_cache(maxsize=None)
def bvh_light_world():
    """(world, tables, moved): list 0 is the source of one reference BVH over N_BVH_SPHERES spheres added in random order -- itself a light
    list with that many members; list 1 holds three of them, named by the world indices they have AFTER the build.  Spheres past the
    tree (radius 0, a tiny one, moving ones) and the quads are reached by index only.  moved = how many world indices hold another
    sphere after the build than before."""
    L = host.lib()
    rng = np.random.default_rng(20260102)
    w = host.World()
    mats = _materials(w)
    lst = L.mort_add_hittable_list(w.ptr, True)
    for i in range(N_BVH_SPHERES):  # static, positive radii: the tree's boxes are ordinary
        r = float(F(10.0 ** rng.uniform(-4, 4)))
        mt, mi = mats[int(rng.integers(0, len(mats)))]
        assert L.mort_add_sphere(w.ptr, host.vec3(*(rng.uniform(-30, 30, 3) * r)), r, mt, mi, True) == i
        L.mort_list_add(w.ptr, lst, S.OBJ_SPHERE, i)
    before = _tables(w)["spheres"]["c"][:N_BVH_SPHERES].copy()
    assert L.mort_add_bvh(w.ptr, lst, False) == 0
    after = _tables(w)["spheres"]["c"][:N_BVH_SPHERES]
    moved = int((before != after).any(1).sum())
    _add_spheres(w, rng, 590, mats, {0: 0.0, 1: 1e-3})                          # world indices 500, 501
    _add_quads(w, rng, 640, mats)
    few = L.mort_add_hittable_list(w.ptr, True)
    for i in (7, 123, 499):
        L.mort_list_add(w.ptr, few, S.OBJ_SPHERE, i)
    w.c.bvh_mode = True
    return w, _tables(w), moved


WORLDS = {"flat": lambda: flat_light_world()[:2], "bvh": lambda: bvh_light_world()[:2]}

# ---- records ----
# origin families, per anchor primitive
S_FAR, S_MID, S_NEAR, S_SURFACE, S_SURFACE_IN, S_SURFACE_OUT, S_INSIDE, S_CENTRE = range(8)
Q_FAR, Q_NEAR, Q_BEHIND, Q_IN_PLANE, Q_OFF_PLANE, Q_AT_Q = range(8, 14)
ORIGIN_NAMES = ("s_far", "s_mid", "s_near", "s_surface", "s_surface_in", "s_surface_out", "s_inside", "s_centre",
                "q_far", "q_near", "q_behind", "q_in_plane", "q_off_plane", "q_at_Q")
# direction families (fn 0)
D_TOWARD, D_NUDGED, D_RIM, D_RANDOM, D_ZERO, D_INF, D_NAN, D_AXIS = range(8)
DIR_NAMES = ("toward", "nudged", "rim", "random", "zero", "inf", "nan", "axis")


def _next(x, up):
    return np.nextafter(x, np.where(up, F(np.inf), F(-np.inf)).astype(F)).astype(F)


def _pick_lights(rng, tab, n):
    """(type, idx, anchor kind 1 sphere / 2 quad, anchor index) per record: spheres, quads, both lists (the anchor is the member the
    origin is placed around) and every foreign tag; the special primitives are drawn more often than their share"""
    ns, nq = len(tab["spheres"]), len(tab["quads"])
    typ = np.empty(n, np.int32); idx = np.empty(n, np.int32); ak = np.empty(n, np.int32); ai = np.empty(n, np.int32)
    what = rng.choice(5, n, p=[0.34, 0.34, 0.08, 0.14, 0.10])
    special_s = np.flatnonzero((tab["spheres"]["r"] <= 0) | (tab["spheres"]["r"] == F(1e-3)))
    special_q = np.array([QUAD_PARALLEL, QUAD_ZERO_U])
    s = rng.integers(0, ns, n); q = rng.integers(0, nq, n)
    boost = rng.random(n)
    s = np.where(boost < 0.03, special_s[rng.integers(0, len(special_s), n)], s)
    q = np.where(boost < 0.03, special_q[rng.integers(0, 2, n)], q)
    q = np.where((boost >= 0.03) & (boost < 0.30), AXIS_QUAD_FIRST + rng.integers(0, N_AXIS_QUADS, n), q)
    m = what == 0; typ[m] = S.OBJ_SPHERE; idx[m] = s[m]; ak[m] = 1; ai[m] = s[m]
    m = what == 1; typ[m] = S.OBJ_QUAD; idx[m] = q[m]; ak[m] = 2; ai[m] = q[m]
    for li, code in ((0, 2), (1, 3)):
        m = what == code
        lt, lidx = tab["lists"][li]
        pos = rng.integers(0, len(lt), n)
        mt, mi = lt[pos], lidx[pos]
        prim = (mt == S.OBJ_SPHERE) | (mt == S.OBJ_QUAD)
        typ[m] = S.OBJ_HITTABLE_LIST; idx[m] = li
        ak[m] = np.where(prim, mt, 1)[m]; ai[m] = np.where(prim, mi, s)[m]      # a foreign member: around some sphere
    m = what == 4
    typ[m] = np.array(FOREIGN_TAGS, np.int32)[rng.integers(0, len(FOREIGN_TAGS), n)][m]
    idx[m] = rng.integers(-3, 2000, n)[m]                                        # never dereferenced
    ak[m] = np.where(rng.random(n) < 0.5, 1, 2)[m]; ai[m] = np.where(ak == 1, s, q)[m]
    return typ, idx, ak, ai


def _origins(rng, tab, ak, ai):
    """(origin float32 (n, 3), family code (n,)) around the anchors"""
    n = len(ak)
    org = np.zeros((n, 3), F)
    fam = np.zeros(n, np.int32)
    # spheres: pdf_value ignores motion, so the geometry is that of center1
    m = np.flatnonzero(ak == 1)
    sp = tab["spheres"][ai[m]]
    c = sp["c"].astype(np.float64); r = np.abs(sp["r"].astype(np.float64))[:, None]
    f = rng.choice(8, len(m), p=[0.14, 0.14, 0.22, 0.08, 0.06, 0.06, 0.22, 0.08])
    d = _unit(rng, len(m))
    dist = np.select([f == S_FAR, f == S_MID, f == S_NEAR, f == S_INSIDE, f == S_CENTRE],
                     [10.0 ** rng.uniform(3, 6, len(m)), 10.0 ** rng.uniform(np.log10(5), np.log10(500), len(m)), rng.uniform(1.05, 5, len(m)),
                      rng.uniform(0, 0.98, len(m)), 0.0], 1.0)[:, None]
    o = (c + d * r * dist).astype(F)
    toward_centre = (sp["c"] > o)
    o = np.where((f == S_SURFACE_IN)[:, None], _next(o, toward_centre), o)
    o = np.where((f == S_SURFACE_OUT)[:, None], _next(o, ~toward_centre), o)
    o = np.where((f == S_CENTRE)[:, None], sp["c"], o)
    org[m] = o; fam[m] = f
    # quads
    m = np.flatnonzero(ak == 2)
    qd = tab["quads"][ai[m]]
    Q, u, v = (qd[k].astype(np.float64) for k in ("Q", "u", "v"))
    nrm = qd["normal"].astype(np.float64)
    bad = ~np.isfinite(nrm).all(1)
    nrm[bad] = _unit(rng, int(bad.sum()))                                        # a degenerate quad has no side: any direction serves
    size = np.maximum(np.maximum(np.linalg.norm(u, axis=1), np.linalg.norm(v, axis=1)), 1e-30)[:, None]
    f = 8 + rng.choice(6, len(m), p=[0.12, 0.30, 0.22, 0.18, 0.10, 0.08])
    a, b = rng.uniform(-0.5, 1.5, (2, len(m), 1))
    P = Q + a * u + b * v
    h = np.select([f == Q_FAR, f == Q_NEAR, f == Q_BEHIND], [10.0 ** rng.uniform(3, 6, len(m)), rng.uniform(0.2, 3, len(m)), -rng.uniform(0.2, 3, len(m))], 0.0)[:, None]
    o = (P + nrm * size * h).astype(F)
    far = f == Q_FAR
    o[far] = (Q[far] + 0.5 * (u[far] + v[far]) + _unit(rng, int(far.sum())) * size[far] * np.abs(h[far])).astype(F)
    # the axis quads: in the plane exactly (the normal's coordinate is Q's), and one float off it
    axis = (ai[m] >= AXIS_QUAD_FIRST) & (ai[m] < AXIS_QUAD_FIRST + N_AXIS_QUADS)
    k = ai[m] % 3
    rows = np.arange(len(m))
    flat = axis & ((f == Q_IN_PLANE) | (f == Q_OFF_PLANE))
    o[rows[flat], k[flat]] = qd["Q"][rows[flat], k[flat]]
    off = axis & (f == Q_OFF_PLANE)
    o[rows[off], k[off]] = _next(o[rows[off], k[off]], rng.random(int(off.sum())) < 0.5)
    o = np.where((f == Q_AT_Q)[:, None], qd["Q"], o)
    org[m] = o; fam[m] = f
    return org, fam


def _rim_directions(rng, tab, ak, ai, org):
    """aimed at a quad's corners and edges, and at a sphere's limb from either side of it"""
    n = len(ak)
    out = np.zeros((n, 3), np.float64)
    o = org.astype(np.float64)
    m = np.flatnonzero(ak == 2)
    qd = tab["quads"][ai[m]]
    ab = np.array([(0, 0), (1, 0), (0, 1), (1, 1), (0.5, 0), (0, 0.5), (1, 0.5), (0.5, 1)], np.float64)[rng.integers(0, 8, len(m))]
    out[m] = qd["Q"].astype(np.float64) + ab[:, :1] * qd["u"] + ab[:, 1:] * qd["v"] - o[m]
    m = np.flatnonzero(ak == 1)
    sp = tab["spheres"][ai[m]]
    wv = sp["c"].astype(np.float64) - o[m]
    dist = np.maximum(np.linalg.norm(wv, axis=1, keepdims=True), 1e-300)
    wv = wv / dist
    t = _unit(rng, len(m))
    t -= (t * wv).sum(1, keepdims=True) * wv
    t /= np.maximum(np.linalg.norm(t, axis=1, keepdims=True), 1e-300)
    sin = np.clip(np.abs(sp["r"].astype(np.float64))[:, None] / dist, 0, 1) * (1 + rng.choice([-1e-3, -1e-6, 0, 1e-6, 1e-3], (len(m), 1)))
    sin = np.clip(sin, 0, 1)
    out[m] = (np.sqrt(1 - sin * sin) * wv + sin * t) * dist * rng.uniform(0.1, 10, (len(m), 1))
    return np.nan_to_num(out, nan=0.0).astype(F)


def _streams(rng, n):
    """(n, 6) XORWOW words: math_cases' seeded, extreme-output and random states, shuffled"""
    m = max(n, 1 << 18)  # the seeded and extreme states alone are 155648
    st, _ = MC._states(rng, m)
    return np.ascontiguousarray(st[rng.permutation(m)[:n]])


def light_random_records(typ, idx, org, states):
    rec = np.empty((len(typ), 11), U)
    rec[:, :6] = states
    rec[:, 6] = typ.view(U); rec[:, 7] = idx.view(U); rec[:, 8:] = org.view(U)
    return rec


@functools.lru_cache(maxsize=None)
def build(world_name, fn, n=N_RECORDS):
    """(records (n, in_words) uint32, labels): labels = dict(type, idx, anchor_kind, anchor_idx, origin (family code), direction (family
    code, fn 0)).  Seeded; the "toward" directions are the oracle's own light_random from the record's origin."""
    world, tab = WORLDS[world_name]()
    rng = np.random.default_rng(4000 + 10 * sorted(WORLDS).index(world_name) + fn)
    typ, idx, ak, ai = _pick_lights(rng, tab, n)
    org, ofam = _origins(rng, tab, ak, ai)
    labels = dict(type=typ, idx=idx, anchor_kind=ak, anchor_idx=ai, origin=ofam)
    if fn == 1:
        rec = light_random_records(typ, idx, org, _streams(rng, n))
        return rec, labels
    toward = O.light_batch(world, 1, light_random_records(typ, idx, org, _streams(rng, n)))[:, :3].view(F)
    dfam = rng.choice(8, n, p=[0.40, 0.12, 0.14, 0.18, 0.03, 0.04, 0.04, 0.05])
    up = rng.random((n, 3)) < 0.5
    special = np.zeros((n, 3), F)
    col = rng.integers(0, 3, n); rows = np.arange(n)
    rnd = _unit(rng, n).astype(F)
    inf = rnd.copy(); inf[rows, col] = np.where(rng.random(n) < 0.5, F(np.inf), F(-np.inf))
    nan = rnd.copy(); nan[rows, col] = F(np.nan)
    nan[rng.random(n) < 0.3] = F(np.nan)
    axis = special.copy(); axis[rows, col] = np.where(rng.random(n) < 0.5, F(1), F(-1))
    zero = special.copy(); zero[rng.random(n) < 0.5, 0] = F(-0.0)
    d = np.select([(dfam == k)[:, None] for k in range(8)],
                  [toward, _next(toward, up), _rim_directions(rng, tab, ak, ai, org), rnd * F(10.0 ** rng.uniform(-3, 3, (n, 1))), zero, inf, nan, axis])
    rec = np.empty((n, 8), U)
    rec[:, 0] = typ.view(U); rec[:, 1] = idx.view(U); rec[:, 2:5] = org.view(U); rec[:, 5:] = np.ascontiguousarray(d, dtype=F).view(U)
    labels["direction"] = dfam
    return rec, labels


def ragged(world_name, fn):
    rec, _ = build(world_name, fn)
    pick = np.random.default_rng(90 + fn).choice(len(rec), RAGGED, replace=False)
    return np.ascontiguousarray(rec[np.sort(pick)])


@functools.lru_cache(maxsize=None)
def oracle(world_name, fn):
    """the oracle's answers over build(world_name, fn), computed once and shared (read-only)"""
    out = O.light_batch(WORLDS[world_name]()[0], fn, build(world_name, fn)[0], nthreads=16)
    out.setflags(write=False)
    return out


def _share(cond, of):
    return float(cond[of].mean()) if of.any() else -1.0


def census(world_name, fn):
    """{condition: (measured, required, comparison)} on the oracle's answers alone"""
    _, tab = WORLDS[world_name]()
    rec, lab = build(world_name, fn)
    out = oracle(world_name, fn)
    typ, idx, ofam = lab["type"], lab["idx"], lab["origin"]
    sph, qd = tab["spheres"], tab["quads"]
    res = {}
    for k, name in enumerate(ORIGIN_NAMES):
        res["origin " + name] = (int((ofam == k).sum()), 1000, ">=")
    for t in range(-1, 9):
        res[f"tag {t}"] = (int((typ == t).sum()), 1000, ">=")
    for li, (lt, _) in enumerate(tab["lists"]):
        res[f"list {li} ({len(lt)} members)"] = (int(((typ == S.OBJ_HITTABLE_LIST) & (idx == li)).sum()), 1000, ">=")
    foreign = ~np.isin(typ, (S.OBJ_SPHERE, S.OBJ_QUAD, S.OBJ_HITTABLE_LIST))
    is_s, is_q = typ == S.OBJ_SPHERE, typ == S.OBJ_QUAD
    r = np.where(is_s, sph["r"][np.where(is_s, idx, 0)], F(1))
    moving = is_s & (sph["moves"][np.where(is_s, idx, 0)] != 0)
    good_q = is_q & np.isfinite(qd["normal"][np.where(is_q, idx, 0)]).all(1) & (qd["area"][np.where(is_q, idx, 0)] > 0)
    if fn == 0:
        pdf = out[:, 0].view(F)
        dfam = lab["direction"]
        for k, name in enumerate(DIR_NAMES):
            res["direction " + name] = (int((dfam == k).sum()), 1000, ">=")
        fine = np.isfinite(pdf) & (pdf > 0)
        toward = dfam == D_TOWARD
        outside_s = np.isin(ofam, (S_MID, S_NEAR))
        # a sphere under 1e-3 across lies wholly within t_min = 0.001 of an origin next to it: no direction hits it.  SEEN_R keeps those out
        seen = r >= F(SEEN_R)
        res["toward, static sphere, outside: finite positive"] = (_share(fine, toward & is_s & ~moving & seen & outside_s), 0.99, ">=")
        res["toward, moving sphere, outside: finite positive"] = (_share(fine, toward & moving & seen & outside_s), 0.99, ">=")
        res["toward, sphere under 1e-3 across, near: zero"] = (int((pdf[toward & is_s & (r > 0) & (r < F(4e-4)) & (ofam == S_NEAR)] == 0).sum()), 100, ">=")
        res["toward, quad, off plane: finite positive"] = (_share(fine, toward & good_q & np.isin(ofam, (Q_NEAR, Q_BEHIND))), 0.99, ">=")
        res["toward, quad, behind: finite positive"] = (_share(fine, toward & good_q & (ofam == Q_BEHIND)), 0.99, ">=")
        res["toward, inside a sphere: NaN"] = (_share(np.isnan(pdf), toward & is_s & (r > 0) & (ofam == S_INSIDE)), 0.90, ">=")
        finite_dir = np.isfinite(rec[:, 5:].view(F)).all(1)
        axis_q = is_q & (idx >= AXIS_QUAD_FIRST) & (idx < AXIS_QUAD_FIRST + N_AXIS_QUADS)
        in_plane = axis_q & (ofam == Q_IN_PLANE) & finite_dir
        res["in-plane records"] = (int(in_plane.sum()), 1000, ">=")
        res["in-plane records that are not +0"] = (int((out[in_plane, 0] != 0).sum()), 0, "==")
        res["foreign tags that are not +0"] = (int((out[foreign, 0] != 0).sum()), 0, "==")
        res["far sphere (1e3 .. 1e6 radii away): infinite pdfs"] = (int(np.isinf(pdf[is_s & (r > 0) & (ofam == S_FAR)]).sum()), 1, ">=")
        par = is_q & (idx == QUAD_PARALLEL)
        res["u || v quad: NaN"] = (_share(np.isnan(pdf), par & finite_dir), 0.99, ">=")
        res["NaN pdfs"] = (int(np.isnan(pdf).sum()), 1000, ">=")
        res["infinite pdfs"] = (int(np.isinf(pdf).sum()), 100, ">=")
        res["zero pdfs"] = (int((pdf == 0).sum()), 1000, ">=")
    else:
        d, draws = out[:, :3].view(F), out[:, 9]
        plain = (d == np.array([1, 0, 0], F)).all(1) & (out[:, :3] == np.array([0x3f800000, 0, 0], U)).all(1)
        res["foreign tags not (1,0,0) or with a draw"] = (int((~plain[foreign] | (draws[foreign] != 0)).sum()), 0, "==")
        res["primitives with other than 2 draws"] = (int((draws[is_s | is_q] != 2).sum()), 0, "==")
        for li, (lt, lidx) in enumerate(tab["lists"]):
            m = np.flatnonzero((typ == S.OBJ_HITTABLE_LIST) & (idx == li))[: max(60 * len(lt), 20000)]
            pos = _chosen_positions(rec[m], len(lt))
            past = pos == len(lt)
            assert ((pos >= 0) & (pos <= len(lt))).all()
            res[f"list {li}: positions never chosen"] = (int(len(lt) - len(np.unique(pos[~past]))), 0, "==")
            # curand_uniform is exactly 1.0f for the highest generator outputs (2^-25 of all draws; math_cases' streams hold many), and
            # random_int(0, n - 1) = (int)(float)(u * (n - 1 + 0.999999)) is then n - 1e-6 rounded to float32: n itself from n = 33 on.  The
            # entry one past the list is read, which mort_list_add has left (0, 0), a foreign tag
            res[f"list {li}: random_int gives n, one past the list"] = (int(past.sum()), 10 if len(lt) >= 33 else 0, ">=" if len(lt) >= 33 else "==")
            # a list draws once, then its member draws twice or (a foreign tag) not at all
            prim = np.isin(np.append(lt, 0)[pos], (S.OBJ_SPHERE, S.OBJ_QUAD))
            res[f"list {li}: draw counts other than 1 + the member's"] = (int((draws[m] != np.where(prim, 3, 1)).sum()), 0, "==")
        res["non-finite directions"] = (int((~np.isfinite(d).all(1)).sum()), 100, ">=")
    return res


def _chosen_positions(rec, n_members):
    """the list position the oracle's random_int(0, n - 1) picks from each record's stream"""
    L = O.lib()
    pos = np.empty(len(rec), np.int64)
    st = S.RngState()
    for i, row in enumerate(rec):
        st.d = int(row[0])
        for k in range(5):
            st.v[k] = int(row[1 + k])
        pos[i] = L.mort_oracle_random_int(C.byref(st), 0, n_members - 1)
    return pos


def assert_census(world_name, fn):
    res = census(world_name, fn)
    lines = [f"  {k}: {v[0]:.4f} (required {v[2]} {v[1]})" if isinstance(v[0], float) else f"  {k}: {v[0]} (required {v[2]} {v[1]})" for k, v in res.items()]
    print(f"census, {world_name} world, {NAMES[fn]}:\n" + "\n".join(lines))
    bad = [k for k, (got, want, op) in res.items() if not (got >= want if op == ">=" else got == want)]
    assert not bad, f"{world_name} / {NAMES[fn]}: census conditions missed: {[(k, res[k]) for k in bad]}"


def assert_same(fn, rec, results):
    """results: {label: (n, out_words) uint32 words}: all equal bit for bit, any NaN equal to any NaN (MC.canon), signed zeros and the
    stream words and draw counts included; the failure names the first differing record"""
    labels = list(results)
    can = [MC.canon(np.asarray(results[k]).reshape(len(rec), -1), OUT_KINDS[fn]) for k in labels]
    bad = np.zeros(len(rec), bool)
    for c in can[1:]:
        bad |= (c != can[0]).any(1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        hexes = lambda w: " ".join(f"{int(v):08x}" for v in np.ascontiguousarray(w).reshape(-1).view(U))
        raise AssertionError(f"{NAMES[fn]}: {int(bad.sum())} of {len(rec)} records differ; first at record {i}: input {hexes(rec[i])}; " +
                             "; ".join(f"{k} {hexes(np.asarray(results[k]).reshape(len(rec), -1)[i])}" for k in labels))


PIN_RECORDS = 1 << 14


def pin_records(world_name, fn):
    """the records run against the reference's own code: the same builder at 2^14 records, so every family is in it whole"""
    return build(world_name, fn, PIN_RECORDS)


# ---- the same lights through every form that shades: small hand-built worlds over a diffuse checker ground, each with an isotropic
# sphere or medium and a glass sphere, each naming its light object (tests/test_light_worlds_host.py, tests/test_gpu_light_worlds.py) ----
from tests import worlds as Wd  # noqa: E402

_ISO = ("sphere", (-0.9, 0, -1), 0.5, ("iso", (.9, .4, .2)))
_GLASS = ("sphere", (0.9, 0, -1), 0.5, ("glass", 1.5))
_LAMB = ("sphere", (0, 0, -1.8), 0.5, ("lamb", (.2, .4, .9)))
_BASE = [Wd.GROUND, _ISO, _GLASS, _LAMB]
# list_of_seven's members: three spheres (one moving, one the glass sphere of _BASE, not emissive) and four quads of very different
# size, the last with its normal turned away from the scene
_SEVEN = [("sphere", (-1.6, 1.4, -1.2), 0.15, ("light", (20, 20, 20))),
          ("msphere", (1.5, 1.2, -1.5), (1.5, 1.6, -1.5), 0.25, ("light", (8, 8, 8))),
          ("quad", (-1, 2.5, -2.5), (0, 0, 2), (2, 0, 0), ("light", (5, 5, 5))),
          ("quad", (-0.1, 1.8, -0.6), (0, 0, 0.2), (0.2, 0, 0), ("light", (40, 40, 40))),
          ("quad", (0.5, 0.9, -0.2), (0.02, 0, 0), (0, 0.02, 0), ("light", (200, 200, 200))),
          ("quad", (-0.75, 1.8, -3.5), (1.5, 0, 0), (0, -1.5, 0), ("light", (6, 6, 6)))]
_SEVEN_MEMBERS = (4, 5, 2, 6, 7, 8, 9)  # positions in _BASE + _SEVEN


def _light_list(w, members):
    L = host.lib()
    lst = L.mort_add_hittable_list(w.ptr, True)
    for t, i in members:
        assert L.mort_list_add(w.ptr, lst, t, i) == 0
    return (S.OBJ_HITTABLE_LIST, lst)


def _lw_list_of_one():
    w, ids = Wd.flat_world(_BASE + [("quad", (-1, 2.2, -2), (0, 0, 2), (2, 0, 0), ("light", (9, 9, 9)))])
    return w, _light_list(w, [ids[4]])


def _lw_list_of_seven():
    w, ids = Wd.flat_world(_BASE + _SEVEN)
    return w, _light_list(w, [ids[k] for k in _SEVEN_MEMBERS])


def _lw_list_with_foreign():
    """a quad, a sphere, and the translate and the medium of a smoke box in one list"""
    L = host.lib()
    w, ids = Wd.flat_world([Wd.GROUND, _GLASS, _LAMB, ("quad", (-1, 2.2, -2), (0, 0, 2), (2, 0, 0), ("light", (9, 9, 9))),
                            ("sphere", (-1.7, 1.0, -0.8), 0.2, ("light", (15, 15, 15)))])
    col = L.mort_add_solid_color(w.ptr, host.vec3(.9, .9, .9))
    L.mort_rotated_smoke_box(w.ptr, host.vec3(0.8, 0.9, 0.8), host.vec3(-1.3, -0.5, -1.4), 20.0, 2.0, S.MAT_ISOTROPIC, L.mort_add_isotropic(w.ptr, S.TEXTURE_SOLID, col))
    o = w.c.objs
    return w, _light_list(w, [ids[3], ids[4], (S.OBJ_TRANSLATE, o.num_translates - 1), (S.OBJ_CONSTANT_MEDIUM, o.num_constant_medium - 1)])


def _lw_dome():
    w, ids = Wd.flat_world(_BASE + [("sphere", (0, 0, -1), 50.0, ("light", (1.2, 1.1, 1.0)))])
    return w, ids[4]


def _lw_coplanar():
    """a quad light lying in the plane of a diffuse floor quad: every shading point of the floor is in the light's plane"""
    w, ids = Wd.flat_world([Wd.GROUND, _ISO, _GLASS, ("quad", (-3, -0.45, -4), (0, 0, 6), (6, 0, 0), ("lamb", (.7, .7, .7))),
                            ("quad", (-0.6, -0.45, -1.9), (0, 0, 1.2), (1.2, 0, 0), ("light", (6, 6, 6)))])
    return w, ids[4]


def _lw_tiny_far():
    w, ids = Wd.flat_world(_BASE + [("sphere", (0, 800, -601), 1e-3, ("light", (1e6, 1e6, 1e6)))])
    return w, ids[4]


def _lw_moving_light():
    w, ids = Wd.flat_world(_BASE + [("msphere", (-0.5, 1.6, -1), (0.5, 1.6, -1), 0.3, ("light", (12, 12, 12)))])
    return w, ids[4]


def _lw_degenerate_quad():
    """u || v: area 0, NaN normal.  The compile accepts it.  In the scan it would swallow the frame -- its NaN t passes every test of
    quad::hit, so every ray "hits" it first and the oracle's frame is black -- so it is skipped there and only named as the light: every
    pdf_value toward it is NaN"""
    w, ids = Wd.flat_world(_BASE + [("quad", (-1, 2.2, -2), (2, 0, 0), (4, 0, 0), ("light", (9, 9, 9)))])
    w.c.objs.host_quad[ids[4][1]].skip = True
    return w, ids[4]


_BVH_SPHERES = [((1.6, 1.4, -1.2), 0.2, ("light", (20, 20, 20))), ((-1.6, 1.2, -1.6), 0.3, ("light", (8, 8, 8))), Wd._BVH_GROUND,
                ((-0.9, 0, -1), 0.5, ("iso", (.9, .4, .2))), ((0.9, 0, -1), 0.5, ("glass", 1.5)), ((0, 0, -1.8), 0.5, ("lamb", (.2, .4, .9))),
                ((0.1, -0.3, -0.2), 0.2, ("metal", (.8, .8, .8), 0.1)), ((-2.2, -0.2, -2.5), 0.3, ("lamb", (.7, .3, .3)))]


def _lw_bvh_list():
    w = Wd.custom_bvh_world(_BVH_SPHERES)
    sph = _tables(w)["spheres"]
    lights = [int(i) for i in np.flatnonzero(sph["mat_type"] == S.MAT_DIFFUSE_LIGHT)]
    assert len(lights) == 2 and set(lights).isdisjoint({0, 1}), lights  # added at 0 and 1, moved by the build
    return w, _light_list(w, [(S.OBJ_SPHERE, i) for i in lights])


def _lw_big_list():
    """list_of_seven among 56 more small spheres: 66 primitives, so the unified-tree megakernel is the library's own choice"""
    rng = np.random.default_rng(66)
    more = [("sphere", (float(-2.4 + 0.7 * (k % 8)), -0.38, float(-3.2 + 0.45 * (k // 8))), 0.12,
             ("lamb", tuple(rng.uniform(0.2, 0.9, 3))) if k % 3 else ("metal", tuple(rng.uniform(0.5, 0.9, 3)), 0.2)) for k in range(56)]
    w, ids = Wd.flat_world(_BASE + _SEVEN + more)
    return w, _light_list(w, [ids[k] for k in _SEVEN_MEMBERS])


LIGHT_WORLDS = {"list_of_one": _lw_list_of_one, "list_of_seven": _lw_list_of_seven, "list_with_foreign": _lw_list_with_foreign, "dome": _lw_dome,
                "coplanar": _lw_coplanar, "tiny_far": _lw_tiny_far, "moving_light": _lw_moving_light, "degenerate_quad": _lw_degenerate_quad,
                "bvh_list": _lw_bvh_list, "big_list": _lw_big_list}
NON_FINITE_WORLDS = ("dome", "coplanar", "degenerate_quad")  # census: at least 5 % of the pixels hold a non-finite sample


@functools.lru_cache(maxsize=None)
def light_world(name, lit=True):
    """(world, camera): 64 x 36, 4 spp, bounce limit 8, a non-zero background except under the dome; lit=False: the same without a light object"""
    w, light = LIGHT_WORLDS[name]()
    cam = Wd.flat_camera(light=light if lit else None, spp=4, width=64, depth=8)
    if name == "dome":
        for k in range(3):
            cam.background.e[k] = 0.0
    return w, cam


@functools.lru_cache(maxsize=None)
def frame_reference(name, lit=True):
    w, cam = light_world(name, lit)
    ref = O.render(w, cam, nthreads=8)
    for a in (ref["rgba"], ref["accum"], ref["segments_px"]):
        a.setflags(write=False)
    return ref


class RayRef:
    """rays (n, 8), streams0 / streams, rgb (n, 3): the oracle's ray_color along the frame's own primary rays (sample 0, 0 of every pixel)"""


@functools.lru_cache(maxsize=None)
def radiance_reference(name):
    from tests import query_rays as Q
    from tests import radiance_ref as R
    w, cam = light_world(name)
    W, H = cam.image_width, cam.image_height
    L = O.lib()
    r = RayRef()
    gen = O.seed_states(7, W, H)   # the streams get_ray draws the rays from
    r.rays = np.zeros((W * H, 8), F)
    r7, st = (C.c_float * 7)(), S.RngState()
    for i in range(W * H):
        st.d = int(gen["d"][i])
        for k in range(5):
            st.v[k] = int(gen["v"][i][k])
        L.mort_oracle_get_ray(C.byref(cam), i % W, i // W, 0, 0, C.byref(st), r7)
        r.rays[i, :7] = list(r7)
    r.rays[:, 7] = np.inf
    r.params = hip.radiance_params_from_camera(cam, 1)
    r.streams0 = Q.some_streams(W * H)
    r.streams = r.streams0.copy()
    r.rgb = R.oracle_radiance(w, cam, r.rays, r.streams, 1)
    for a in (r.rays, r.streams0, r.streams, r.rgb):
        a.setflags(write=False)
    return r


PROBE_D = 64


@functools.lru_cache(maxsize=None)
def probe_reference(name):
    """one SH9 probe above the scene's middle, 64 directions, one path each (tests/probe_ref.py's restatement of the contract)"""
    from tests import probe_ref as P
    from tests import query_rays as Q
    from tests import radiance_ref as R
    w, cam = light_world(name)
    r = P.Ref()
    r.world, r.cam = w, cam
    r.params = hip.probe_params_from_camera(cam, PROBE_D, 1)
    r.probes = np.zeros(1, dtype=hip.PROBE_DTYPE)
    r.probes["position"] = (0.0, 0.4, -0.6)
    r.probes["time"] = 0.5
    r.dirs = P.fibonacci(PROBE_D)
    r.streams0 = Q.some_streams(PROBE_D)
    r.streams = r.streams0.copy()
    r.s = R.oracle_radiance(w, cam, P.rays_of(r.probes, r.dirs), r.streams, 1).reshape(1, PROBE_D, 3)
    r.sh = P.project(r.s, r.dirs, 1)
    for a in (r.probes, r.dirs, r.streams0, r.streams, r.s, r.sh):
        a.setflags(write=False)
    return r


def frame_census(name):
    """on the oracle alone: the share of pixels the light object changes, the share whose first sample is non-finite along the frame's own
    primary rays, the share of non-finite accumulator components (the frame zeroes a NaN pixel sum, camera.cuh:197-199, so only an
    infinity survives there)"""
    on, off = frame_reference(name), frame_reference(name, lit=False)
    changed = float(((on["accum"].view(U) != off["accum"].view(U)).any(-1) | (on["segments_px"] != off["segments_px"]).reshape(on["accum"].shape[:2])).mean())
    rgb = radiance_reference(name).rgb
    return dict(changed=changed, non_finite_samples=float((~np.isfinite(rgb)).any(1).mean()), non_finite_accum=float((~np.isfinite(on["accum"])).any(-1).mean()))


def assert_frame_same(out, ref, what):
    """image, accumulators (raw words, any NaN equal to any NaN), per-pixel segment counts, totals and final RNG words"""
    from tests.query_rays import _words
    assert (out["rgba"] == ref["rgba"]).all(), f"{what}: uchar4 image differs in {int((out['rgba'] != ref['rgba']).any(-1).sum())} pixels"
    assert (_words(out["accum"]) == _words(ref["accum"])).all(), f"{what}: fp32 accumulators differ"
    assert (np.asarray(out["segments_px"]).reshape(-1) == ref["segments_px"].reshape(-1)).all(), f"{what}: per-pixel segment counts differ"
    assert out["stats"]["segments"] == ref["segments"] and out["stats"]["rng_draws"] == ref["rng_draws"], f"{what}: totals differ"
    st = np.asarray(out["states"]).view(O.STATE_DTYPE).reshape(-1)
    assert (st["d"] == ref["states"]["d"]).all() and (st["v"] == ref["states"]["v"]).all(), f"{what}: final RNG states differ"
