"""Worlds and records for the shade-step sweep (tests/test_shade_host.py, tests/test_gpu_shade.py, tests/test_reference_pin.py): one iteration
of ray_color's loop body -- the closest-hit search over [0.001, inf) and dev_shade.h's shade_hit -- record by record, against the oracle's
bounce_step (mort_oracle_shade_batch), in the layout of debug.hip's shade table.

Three seeded worlds inside an enclosing shell (a ray that leaves its target still ends on something: misses stay rare):
  flat       spheres on a lattice (a fifth of them moving, every seventh of negative radius), quads, boxes, a rotated and translated box,
             rotated and translated quads and spheres, two media, a quad light and a light list (the quad, a sphere, a moving sphere and a
             quad without area, which the scan skips: in the scan its NaN t passes every test of quad::hit and it would swallow every ray).
             It has a unified tree: the device searches it as a radiance query does;
  flat_zero  the same with four spheres of radius zero at exactly representable centres.  No box bounds their error band, so the world
             has no unified tree and the device runs the item scan: the only form that reaches a non-finite normal and, without a light,
             a zero pdf (rp = inf) on a flat world;
  bvh        one reference BVH over the spheres (the four of radius zero among them) and the shell; the quad light, the area-less quad and
             the light list stand beside it.
Their materials hold: every known tag; refraction indices
1, 0.1, 1e30, 1e-30, 0, -1.5, inf, NaN beside 1.5 and 1 / 1.5; fuzz 0, 5, -1, inf, NaN; albedos 0, above 1, negative, inf, NaN; checkers of
scale 0, inf, -0.32, 1e-30, 1e30, NaN and one nested to the depth validate_world allows; noise and image textures, on scattering and on
emissive materials; the unknown material tags -1, 0, 6, 9 and texture tags -1, 0, 5 with zero and in-range indices.

Rays are aimed: per primitive at normal, random and grazing incidence; from inside; at glass from inside (and at 1 / 1.5 glass from
outside) at and around the critical angle; at moving spheres with ray.tm != ray_time0; at the poles and the seam of image-textured
spheres; through the centre of the zero-radius spheres in exact arithmetic; rays that miss; and the legal ray classes of
tests/query_rays.py (origins with a NaN or infinite coordinate, directions with zero components, of zero length, with a NaN).  Each world is
run with no light, the quad light and the light list.  The census is asserted on the oracle's branch words alone, before anything is compared."""
import functools

import numpy as np

from mort_amd import host, structs as S
from tests import material_worlds as M
from tests import math_cases as MC
from tests import oracle_lib as O
from tests import query_rays as Q

F, U = np.float32, np.uint32
N_RECORDS = 1 << 18
RAGGED = (1 << 16) + 37
WORLDS = ("flat", "flat_zero", "bvh")
LIGHT_SETTINGS = ("none", "quad", "list")
OUT_KINDS = "i" + "f" * 14 + "i" * 7
STATUS_MISS, STATUS_END, STATUS_SCATTER, STATUS_IDENTITY = 0, 1, 2, 3
SHELL_R = 200.0
UNKNOWN_MAT_TAGS, UNKNOWN_TEX_TAGS = (-1, 0, 6, 9), (-1, 0, 5)
NESTED = (0.7, 0.4, 0.25, 0.15, 0.1, 0.07, 0.05)  # checker depths 0 .. 6: the deepest nesting tex_ok accepts


def _palette():
    lamb = [("lamb", (.7, .3, .3)), ("lamb", (.2, .4, .9))] + [("lamb", a) for a in M.ALBEDOS] + [("checker", s) for s in M.CHECKER_SCALES] + \
           [("checker", NESTED), ("noise",), ("image",)] + [("tex", t, i) for t in UNKNOWN_TEX_TAGS for i in (0, 3)]
    metal = [("metal", (.8, .7, .6), f) for f in M.FUZZES] + [("metal", a, 0.2) for a in M.ALBEDOS]
    glass = [("glass", i) for i in M.IORS] + [("glass", 1.5), ("glass", 1 / 1.5)]
    iso = [("iso", (.3, .6, .9)), ("iso", (M.NAN, .5, .5)), ("checker", 0.3, "iso"), ("noise", "iso"), ("image", "iso")]
    light = [("light", (4, 4, 4)), ("light", (M.INF, 1, 1)), ("light", (M.NAN, 1, 1)), ("light", (-1, -2, -3)), ("checker", 0.3, "light"),
             ("checker", NESTED, "light"), ("noise", "light"), ("image", "light")]
    unknown = [("mat", t, i) for t in UNKNOWN_MAT_TAGS for i in (0, 1)]
    return lamb, metal, glass, iso, light, unknown


def _kind(mat):
    """what a sphere of this material is to the ray generator"""
    k = mat[0]
    if k == "glass":
        return "glass"
    if k == "image":
        return "image"
    return k


class ShadeWorld:
    """world, name, sph (descriptors: c (n, 3) centre at time 0, cv (n, 3) centre_vec, r (n,), kind / ior lists), quads (Q, u, v), boxes
    (centres), media (centre, radius), lights {setting: (type, idx)}"""


def _lattice(n, spacing=3.0):
    side = int(np.ceil(n ** (1 / 3)))
    ijk = np.array([(i, j, k) for i in range(side) for j in range(side) for k in range(side)][:n], np.float64)
    return (ijk - (side - 1) / 2.0) * spacing


@functools.lru_cache(maxsize=None)
def shade_world(name):
    rng = np.random.default_rng({"flat": 11, "flat_zero": 11, "bvh": 12}[name])
    lamb, metal, glass, iso, light, unknown = _palette()
    pal = lamb + metal + glass + iso + light + unknown
    n_sph = 640 if name == "bvh" else 260
    pos = _lattice(n_sph + 50)
    rng.shuffle(pos)
    spheres, desc = [], []
    for i in range(n_sph):
        mat = pal[i % len(pal)]
        c = tuple(float(v) for v in pos[i])
        r = -0.4 if i % 7 == 3 else 0.4
        if i % 5 == 1:
            c2 = (c[0] + 0.5, c[1] + 0.25, c[2] - 0.5)
            spheres.append((c, c2, r, mat)); desc.append((c, (0.5, 0.25, -0.5), r, mat))
        else:
            spheres.append((c, r, mat)); desc.append((c, (0, 0, 0), r, mat))
    zero_mats = [("lamb", (.7, .3, .3)), ("metal", (.8, .7, .6), 0.0), ("glass", 1.5), ("iso", (.3, .6, .9))]
    for k, mat in enumerate(zero_mats if name != "flat" else []):  # radius zero: centres on the lattice, every coordinate a multiple of 0.5
        c = tuple(float(v) for v in pos[n_sph + k])
        spheres.append((c, 0.0, mat)); desc.append((c, (0, 0, 0), 0.0, mat))
    # the light list's spheres: one static, one moving
    lc = [tuple(float(v) for v in pos[n_sph + 10 + k]) for k in range(2)]
    spheres.append((lc[0], 0.4, ("light", (9, 9, 9)))); desc.append((lc[0], (0, 0, 0), 0.4, ("light", (9, 9, 9))))
    spheres.append((lc[1], (lc[1][0] + 0.5, lc[1][1], lc[1][2]), 0.4, ("light", (9, 9, 9)))); desc.append((lc[1], (0.5, 0, 0), 0.4, ("light", (9, 9, 9))))
    shell = ((0.0, 0.0, 0.0), SHELL_R, ("lamb", (.5, .5, .5)))
    spheres.append(shell)

    b = M._Builder()
    L, w = b.L, b.w
    s = ShadeWorld()
    s.name, s.quads, s.boxes, s.media = name, [], [], []
    free = pos[n_sph + 20:]
    if name == "bvh":
        lst = M.Wd._ok(L.mort_add_hittable_list(w.ptr, True), "list")
        for sp in spheres:
            assert L.mort_list_add(w.ptr, lst, S.OBJ_SPHERE, b.sphere(sp, True)) == 0
        M.Wd._ok(L.mort_add_bvh(w.ptr, lst, False), "mort_add_bvh")
        w.c.bvh_mode = True
    else:
        for sp in spheres:
            b.sphere(sp, False)
        qmats = lamb[:4] + metal[:2] + glass[-2:] + iso[:1] + light[:2] + unknown[:2] + [("image",), ("noise",)]
        for k in range(8):  # free-standing quads
            Qp = free[k] + rng.uniform(-0.3, 0.3, 3)
            u = rng.uniform(-1, 1, 3); v = np.cross(u, rng.uniform(-1, 1, 3)); v *= np.linalg.norm(u) / np.linalg.norm(v)
            mt, mi = b.material(qmats[k % len(qmats)])
            M.Wd._ok(L.mort_add_quad(w.ptr, host.vec3(*Qp), host.vec3(*u), host.vec3(*v), mt, mi, False), "mort_add_quad")
            s.quads.append((np.asarray(F(Qp), np.float64), np.asarray(F(u), np.float64), np.asarray(F(v), np.float64)))
        for k in range(6):  # axis-aligned boxes, then rotated and translated ones
            c = free[8 + k]
            mt, mi = b.material(qmats[(k + 3) % len(qmats)])
            L.mort_box(w.ptr, host.vec3(*(c - 0.4)), host.vec3(*(c + 0.4)), mt, mi)
            s.boxes.append(np.asarray(c, np.float64))
        c = free[14]  # one rotated and translated box (it takes one of the reference's two lists; the light list is the other) ...
        mt, mi = b.material(qmats[7])
        L.mort_rotated_box(w.ptr, host.vec3(0.8, 0.8, 0.8), host.vec3(*c), 35.0, mt, mi)
        s.boxes.append(np.asarray(c, np.float64) + (0.0, 0.4, 0.0))
        for k in range(1, 6):  # ... and single quads and spheres under a rotation and a translation
            c = free[14 + k]
            mt, mi = b.material(qmats[(k + 7) % len(qmats)])
            if k % 2:
                prim = (S.OBJ_QUAD, M.Wd._ok(L.mort_add_quad(w.ptr, host.vec3(-.4, -.4, 0), host.vec3(.8, 0, 0), host.vec3(0, .8, 0), mt, mi, True), "mort_add_quad"))
            else:
                prim = (S.OBJ_SPHERE, M.Wd._ok(L.mort_add_sphere(w.ptr, host.vec3(0, 0, 0), 0.4, mt, mi, True), "mort_add_sphere"))
            rot = M.Wd._ok(L.mort_add_rotate_y(w.ptr, prim[0], prim[1], float(rng.uniform(-60, 60)), True), "mort_add_rotate_y")
            M.Wd._ok(L.mort_add_translate(w.ptr, S.OBJ_ROTATE_Y, rot, host.vec3(*c), False), "mort_add_translate")
            s.boxes.append(np.asarray(c, np.float64))
        for k, phase in enumerate((("iso", (.9, .9, .9)), ("iso", (.2, .5, .9)))):  # two media
            c = free[20 + k]
            boundary = M.Wd._ok(L.mort_add_sphere(w.ptr, host.vec3(*c), 0.9, *b.material(("glass", 1.5)), True), "mort_add_sphere")
            mt, mi = b.material(phase)
            M.Wd._ok(L.mort_add_constant_medium(w.ptr, S.OBJ_SPHERE, boundary, 2.0, mt, mi, False), "mort_add_constant_medium")
            s.media.append((np.asarray(c, np.float64), 0.9))
        w.c.bvh_mode = False
    # the quad light faces the lattice from above; the area-less quad (u || v) is a light only
    mt, mi = b.material(("light", (7, 7, 7)))
    top = float(pos[:, 1].max()) + 4.0
    qlight = M.Wd._ok(L.mort_add_quad(w.ptr, host.vec3(-3, top, -3), host.vec3(6, 0, 0), host.vec3(0, 0, 6), mt, mi, name == "bvh"), "mort_add_quad")
    flatq = M.Wd._ok(L.mort_add_quad(w.ptr, host.vec3(-1, top + 2, -2), host.vec3(2, 0, 0), host.vec3(4, 0, 0), mt, mi, True), "mort_add_quad")
    if name != "bvh":
        s.quads.append((np.array([-3, top, -3.0]), np.array([6.0, 0, 0]), np.array([0, 0, 6.0])))
    o = w.c.objs
    found = []
    for c in lc:  # the BVH build moves the sphere records: find the list's spheres where they are now
        hits = [i for i in range(o.num_spheres) if tuple(o.host_sphere[i].center1.e[k] for k in range(3)) == tuple(float(F(v)) for v in c)]
        assert len(hits) == 1
        found.append(hits[0])
    llist = M.Wd._ok(L.mort_add_hittable_list(w.ptr, True), "list")
    for t, i in ((S.OBJ_QUAD, qlight), (S.OBJ_SPHERE, found[0]), (S.OBJ_SPHERE, found[1]), (S.OBJ_QUAD, flatq)):
        assert L.mort_list_add(w.ptr, llist, t, i) == 0
    s.world = w
    s.lights = {"none": (-1, 0), "quad": (S.OBJ_QUAD, qlight), "list": (S.OBJ_HITTABLE_LIST, llist)}
    s.c = np.array([d[0] for d in desc], np.float64)
    s.cv = np.array([d[1] for d in desc], np.float64)
    s.r = np.array([d[2] for d in desc], np.float64)
    s.kind = np.array([_kind(d[3]) for d in desc])
    s.ior = np.array([float(F(d[3][1])) if d[3][0] == "glass" else 0.0 for d in desc])
    s.image = np.array([d[3][0] == "image" for d in desc])
    return s


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _tangent(rng, nrm):
    t = np.cross(nrm, _unit(rng, len(nrm)))
    return t / np.linalg.norm(t, axis=1, keepdims=True)


FAMILIES = ("normal", "random", "grazing", "inside", "critical_inside", "critical_outside", "ratio_one", "poles_and_seam", "zero_radius", "quads",
            "boxes", "media", "miss", "classes")


@functools.lru_cache(maxsize=None)
def records(name, setting, n=N_RECORDS):
    """((n, 16) uint32 records, (n,) family index): seeded per (world, light setting)"""
    s = shade_world(name)
    rng = np.random.default_rng(1000 * WORLDS.index(name) + LIGHT_SETTINGS.index(setting) + 5)
    flat = name != "bvh"
    share = dict(normal=.10, random=.22, grazing=.08, inside=.14, critical_inside=.08, critical_outside=.04, ratio_one=.04, poles_and_seam=.04,
                 zero_radius=.03 if name != "flat" else 0, quads=.08 if flat else 0, boxes=.05 if flat else 0, media=.03 if flat else 0, miss=.02, classes=.03)
    tot = sum(share.values())
    fam = rng.choice(len(FAMILIES), n, p=[share[f] / tot for f in FAMILIES])
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    tm = rng.random(n)
    tm[rng.random(n) < 0.1] = 0.0
    time0 = np.where(rng.random(n) < 0.5, tm, rng.random(n))
    regular = np.flatnonzero(s.r != 0)

    def sphere_at(sel, pick):
        """centres at the rays' times, |radius|, a random outward unit normal, the surface point"""
        c = s.c[pick] + tm[sel, None] * s.cv[pick]
        r = np.abs(s.r[pick])[:, None]
        nrm = _unit(rng, len(sel))
        return c, r, nrm, c + r * nrm

    for k, f in enumerate(FAMILIES):
        sel = np.flatnonzero(fam == k)
        m = len(sel)
        if not m:
            continue
        L = 10.0 ** rng.uniform(-1, 1, (m, 1))  # direction lengths: shade_hit normalises where the reference does
        if f in ("normal", "random", "grazing", "inside"):
            c, r, nrm, P = sphere_at(sel, regular[rng.integers(0, len(regular), m)])
            if f == "normal":
                o[sel], d[sel] = P + nrm * rng.uniform(0.3, 1.2, (m, 1)), -nrm * L
            elif f == "random":
                wv = _unit(rng, m); wv *= np.sign((wv * nrm).sum(1))[:, None]
                o[sel], d[sel] = P + wv * rng.uniform(0.3, 1.2, (m, 1)), -wv * L
            elif f == "grazing":  # along a tangent, lifted off the tangent plane by a few ulp of the radius either way
                t = _tangent(rng, nrm)
                eps = rng.integers(-3, 4, (m, 1)) * 2.0 ** -22 * r
                o[sel], d[sel] = P + eps * nrm - t * rng.uniform(0.5, 1.0, (m, 1)), t * L
            else:
                o[sel], d[sel] = c + 0.6 * r * _unit(rng, m) * rng.random((m, 1)), _unit(rng, m) * L
        elif f in ("critical_inside", "critical_outside", "ratio_one"):
            want = 1.5 if f == "critical_inside" else float(F(1 / 1.5)) if f == "critical_outside" else 1.0
            cand = np.flatnonzero((s.kind == "glass") & (np.abs(s.ior - want) < 1e-6) & (s.r > 0))
            assert len(cand), (name, f)
            c, r, nrm, P = sphere_at(sel, cand[rng.integers(0, len(cand), m)])
            t = _tangent(rng, nrm)
            if f == "ratio_one":
                th = rng.uniform(0, 1.5, (m, 1))
            else:  # ratio x sin(theta) = 1 + delta, delta from 0 through a few ulp to 1e-2, either sign
                delta = rng.choice([-1, 1], (m, 1)) * np.where(rng.random((m, 1)) < 0.2, 0.0, 10.0 ** rng.uniform(-8, -2, (m, 1)))
                th = np.arcsin(np.clip((1.0 + delta) / 1.5, -1, 1))
            if f == "critical_outside":  # 1 / 1.5 glass: the front face's ratio is 1.5
                wv = np.cos(th) * nrm + np.sin(th) * t
                o[sel], d[sel] = P + wv * rng.uniform(0.3, 1.0, (m, 1)), -wv * L
            else:  # from the middle of the chord that ends at P
                inward = -(np.cos(th) * nrm + np.sin(th) * t)
                o[sel], d[sel] = P + inward * (r * np.cos(th)), -inward * L
                if f == "ratio_one":
                    half = rng.random(m) < 0.5  # and from outside
                    o[sel[half]] = (P + (np.cos(th) * nrm + np.sin(th) * t) * 0.8)[half]
                    d[sel[half]] = (-(np.cos(th) * nrm + np.sin(th) * t) * L)[half]
        elif f == "poles_and_seam":
            cand = np.flatnonzero(s.image & (s.r != 0))
            c, r, nrm, P = sphere_at(sel, cand[rng.integers(0, len(cand), m)])
            y = rng.uniform(-0.99, 0.99, m)
            which = rng.integers(0, 4, m)
            nrm = np.stack([-np.sqrt(1 - y * y), y, np.choose(which, [0.0, -0.0, 1e-7, -1e-7])], 1)
            pole = which >= 2
            nrm[pole & (y > 0)] = (0.0, 1.0, 0.0)
            nrm[pole & (y <= 0) & (which == 3)] = (0.0, -1.0, 0.0)
            P = c + r * nrm
            o[sel], d[sel] = P + nrm * rng.uniform(0.3, 1.0, (m, 1)), -nrm * L
        elif f == "zero_radius":  # o = c - k e, d = e with small-integer e: h, a and |oc|^2 are exact and the discriminant is exactly 0
            cand = np.flatnonzero(s.r == 0)
            pick = cand[rng.integers(0, len(cand), m)]
            e = rng.integers(-2, 3, (m, 3)).astype(np.float64)
            e[(e == 0).all(1)] = (1.0, 0.0, 0.0)
            kk = rng.integers(1, 5, (m, 1)).astype(np.float64)
            o[sel], d[sel] = s.c[pick] - kk * e, e
        elif f == "quads":
            q = [s.quads[i] for i in rng.integers(0, len(s.quads), m)]
            Qp, u, v = (np.array([x[j] for x in q]) for j in range(3))
            P = Qp + rng.uniform(0.02, 0.98, (m, 1)) * u + rng.uniform(0.02, 0.98, (m, 1)) * v
            nrm = np.cross(u, v); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
            nrm *= rng.choice([-1.0, 1.0], (m, 1))
            style = rng.integers(0, 3, m)[:, None]
            wv = _unit(rng, m); wv *= np.sign((wv * nrm).sum(1))[:, None]
            t = np.cross(nrm, _unit(rng, m)); t /= np.linalg.norm(t, axis=1, keepdims=True)
            graz = t + nrm * rng.integers(-3, 4, (m, 1)) * 2.0 ** -22
            wv = np.where(style == 0, nrm, np.where(style == 1, wv, graz))
            o[sel], d[sel] = P + wv * rng.uniform(0.3, 1.0, (m, 1)), -wv * L
        elif f in ("boxes", "media"):
            if f == "boxes":
                c = np.array([s.boxes[i] for i in rng.integers(0, len(s.boxes), m)])
            else:
                c = np.array([s.media[i][0] for i in rng.integers(0, len(s.media), m)])
            wv = _unit(rng, m)
            P = c + rng.uniform(-0.3, 0.3, (m, 3))
            start = rng.uniform(1.2, 2.0, (m, 1)) if f == "boxes" else rng.uniform(0.0, 1.6, (m, 1))  # media: from inside the boundary too
            o[sel], d[sel] = P + wv * start, -wv * L
        elif f == "miss":
            wv = _unit(rng, m)
            o[sel], d[sel] = wv * (SHELL_R * rng.uniform(1.2, 5.0, (m, 1))), (wv + 0.3 * _unit(rng, m)) * L
        else:  # the legal ray classes of tests/query_rays.py, restated on this world
            c, r, nrm, P = sphere_at(sel, regular[rng.integers(0, len(regular), m)])
            oo, dd = P + nrm * 0.5, -nrm + 0.2 * _unit(rng, m)
            cls = rng.integers(0, 7, m)
            ax = rng.integers(0, 3, m)
            rows = np.arange(m)
            for q, val in ((0, np.nan), (1, np.inf), (2, -np.inf)):  # an origin no reach holds
                hit = cls == q
                oo[rows[hit], ax[hit]] = val
            hit = cls == 3; dd[rows[hit], ax[hit]] = 0.0                       # one component exactly zero
            hit = cls == 4; dd[hit] = np.sign(dd[hit]) * (np.arange(3) == ax[hit, None])  # along an axis: two zero components (-0.0 among them)
            hit = cls == 5; dd[hit] = np.where(rng.random((int(hit.sum()), 1)) < 0.5, 0.0, -0.0)  # zero length
            hit = cls == 6; dd[rows[hit], ax[hit]] = np.nan
            o[sel], d[sel] = oo, dd
    st = Q.some_streams(n, seed=77 + LIGHT_SETTINGS.index(setting))
    rec = np.zeros((n, 16), U)
    rec[:, 0] = st["d"]; rec[:, 1:6] = st["v"]
    rec[:, 6:9] = o.astype(F).view(U); rec[:, 9:12] = d.astype(F).view(U)
    rec[:, 12] = tm.astype(F).view(U); rec[:, 13] = time0.astype(F).view(U)
    lt, li = s.lights[setting]
    rec[:, 14] = np.array(lt, np.int32).view(U); rec[:, 15] = np.array(li, np.int32).view(U)
    rec.setflags(write=False); fam.setflags(write=False)
    return rec, fam


def ragged(name, setting):
    rec, _ = records(name, setting)
    return np.ascontiguousarray(rec[np.sort(np.random.default_rng(3).choice(len(rec), RAGGED, replace=False))])


@functools.lru_cache(maxsize=None)
def oracle(name, setting):
    """((n, 22) results, (n,) branch words) of the oracle over records(name, setting)"""
    out, br = O.shade_batch(shade_world(name).world, records(name, setting)[0])
    out.setflags(write=False); br.setflags(write=False)
    return out, br


def census(name):
    """the branch counts of one world over its three light settings, from the oracle's answers alone"""
    c = {}

    def add(k, v):
        c[k] = c.get(k, 0) + int(v)
    for setting in LIGHT_SETTINGS:
        out, br = oracle(name, setting)
        status = out[:, 0]
        hit = status != STATUS_MISS
        tag, tex = O.br_tag(br), O.br_tex(br)
        add("records", len(out)); add("misses", (~hit).sum())
        fl = out[:, 1:15].view(F)
        add("non_finite", (~np.isfinite(fl)).any(1).sum())
        for t in (S.MAT_LAMBERTIAN, S.MAT_METAL, S.MAT_DIELECTRIC, S.MAT_DIFFUSE_LIGHT, S.MAT_ISOTROPIC) + UNKNOWN_MAT_TAGS:
            add(f"material tag {t}", (hit & (tag == t)).sum())
        for t in (S.TEXTURE_SOLID, S.TEXTURE_CHECKER, S.TEXTURE_IMAGE, S.TEXTURE_NOISE) + UNKNOWN_TEX_TAGS:
            add(f"texture tag {t}", (hit & (tex == t)).sum())
            add(f"texture tag {t} on a light", (hit & (tex == t) & (tag == S.MAT_DIFFUSE_LIGHT)).sum())
        glass = hit & (tag == S.MAT_DIELECTRIC)
        front = (br & O.BR_FRONT) != 0
        add("front face", (hit & front).sum()); add("back face", (hit & ~front).sum())
        add("total internal reflection", (glass & ((br & O.BR_CANT_REFRACT) != 0)).sum())
        add("reflected by Schlick", (glass & ((br & O.BR_REFLECTED) != 0) & ((br & O.BR_CANT_REFRACT) == 0)).sum())
        add("refracted", (glass & ((br & O.BR_REFRACTED) != 0)).sum())
        add("refracted with ratio exactly 1", (glass & ((br & O.BR_REFRACTED) != 0) & ((br & O.BR_RATIO_ONE) != 0)).sum())
        add("emission seen from the back face", (hit & (tag == S.MAT_DIFFUSE_LIGHT) & ~front).sum())
        add("emission seen from the front face", (hit & (tag == S.MAT_DIFFUSE_LIGHT) & front).sum())
        add("mat_pdf == 0", ((br & O.BR_MAT_PDF_ZERO) != 0).sum())
        add("rp == inf", (out[:, 4] == 0x7f800000).sum())
        add("non-finite normal", ((br & O.BR_NORMAL_NONFINITE) != 0).sum())
        add("identity scatter", (status == STATUS_IDENTITY).sum()); add("scatter", (status == STATUS_SCATTER).sum()); add("path ends", (status == STATUS_END).sum())
        if setting != "none":
            add("sampled from the light", ((br & O.BR_FROM_LIGHT) != 0).sum())
            add("sampled from the material", ((br & O.BR_FROM_MATERIAL) != 0).sum())
    return c


CENSUS_AT_LEAST_1000 = tuple(f"material tag {t}" for t in (1, 2, 3, 4, 5) + UNKNOWN_MAT_TAGS) + tuple(f"texture tag {t}" for t in (1, 2, 3, 4) + UNKNOWN_TEX_TAGS) + \
    tuple(f"texture tag {t} on a light" for t in (1, 2, 3, 4)) + \
    ("front face", "back face", "total internal reflection", "reflected by Schlick", "refracted", "refracted with ratio exactly 1",
     "emission seen from the back face", "emission seen from the front face", "mat_pdf == 0", "rp == inf", "non-finite normal", "identity scatter", "scatter",
     "path ends", "sampled from the light", "sampled from the material")


# what a world cannot produce: every normal of `flat` is finite, and with a finite normal a direction drawn from the material has a positive pdf
CENSUS_CANNOT = {"flat": ("rp == inf", "non-finite normal")}


def assert_census(name):
    c = census(name)
    few = {k: c[k] for k in CENSUS_AT_LEAST_1000 if c[k] < 1000 and k not in CENSUS_CANNOT.get(name, ())}
    assert all(c[k] == 0 for k in CENSUS_CANNOT.get(name, ())), (name, c)
    assert not few, f"{name}: branches in fewer than 1000 records: {few}"
    assert c["misses"] <= 0.05 * c["records"], (name, c["misses"], c["records"])
    assert c["non_finite"] >= 0.01 * c["records"], (name, c["non_finite"], c["records"])
    return c


def assert_same(rec, results):
    """results: {label: (n, 22) uint32 words} over rec -- all equal bit for bit (math_cases.canon's NaN rule, signed zeros count); the failure
    names the first differing record as hex words with every result"""
    labels = list(results)
    can = [MC.canon(np.asarray(results[k]).reshape(len(rec), -1), OUT_KINDS) for k in labels]
    bad = np.zeros(len(rec), bool)
    for c in can[1:]:
        bad |= (c != can[0]).any(1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        hexes = lambda w: " ".join(f"{int(v):08x}" for v in np.ascontiguousarray(w).reshape(-1).view(U))
        raise AssertionError(f"shade step: {int(bad.sum())} of {len(rec)} records differ; first at record {i}: input {hexes(rec[i])}; " +
                             "; ".join(f"{k} {hexes(np.asarray(results[k]).reshape(len(rec), -1)[i])}" for k in labels))
