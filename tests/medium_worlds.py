"""MEDIUM_WORLDS: small worlds whose constant media lie where no other catalogue goes (constant_medium::hit, objects.cuh:396-434, is the
only step of the closest-hit search that draws from the pixel's stream, and this build restates it in world_hit, gen_media, the query
scan and the feature pass).  Densities 0, negative, inf, NaN, 1e30 and 1e-30; boundaries that are a moving sphere, a list of two spheres,
a slab of two quads, a lone quad, a sphere of negative and of zero radius, a sphere behind rotate_y and translate; media that are
themselves under rotate_y / translate with a surface material as phase function; overlapping and nested media; fifty media in a row; a
medium inside a non-skip list; the camera inside a medium.

Every world stands on one base -- a ground sphere, a back quad, three small Lambertian spheres -- and is a brute-force world (no reference
BVH).  Every medium has a phase material of its own, so a hit record names its medium by (mat_type, mat_idx).  Frames are 96 x 54 or
smaller, 4 spp, bounce limit 12; one oracle render per world, shared by every test.  Each world also has one batch of query rays: the
frame's primary rays, every eighth of them again with t_max cut to the point nearest a medium's centre (the ray ends inside that medium
if it meets it), and rays that start inside each boundary.

tests/test_medium_worlds_host.py holds the census and runs the host forms, tests/test_gpu_medium_worlds.py every kernel form."""
import functools

import numpy as np

from mort_amd import hip, host, structs as S
from tests import material_worlds as M
from tests import oracle_lib as O
from tests import query_rays as Q
from tests import worlds as Wd
from tests.feature_ref import primary_rays

F = np.float32
INF, NAN = float("inf"), float("nan")

DENSITY_EDGES = (0.0, -0.5, INF, NAN, 1e30, 1e-30, -INF, -1e-3)
MAX_MEDIA = 50  # the reference's table (objects.cuh)


class _Builder(M._Builder):
    """material_worlds' materials, and boundaries by description: ("sphere", centre, radius) | ("msphere", c at time 0, c at time 1,
    radius) | ("quad", Q, u, v) | ("list", [boundaries]) | ("T", boundary, offset) | ("R", boundary, degrees) | ("medium", medium) |
    ("tag", obj_type, obj_idx): that reference as given.  Every object of a boundary is added with skip set."""

    def boundary(self, b):
        L, w, kind = self.L, self.w, b[0]
        if kind == "sphere":
            return S.OBJ_SPHERE, Wd._ok(L.mort_add_sphere(w.ptr, host.vec3(*b[1]), b[2], *self.material(("glass", 1.5)), True), "mort_add_sphere")
        if kind == "msphere":
            return S.OBJ_SPHERE, Wd._ok(L.mort_add_moving_sphere(w.ptr, host.vec3(*b[1]), host.vec3(*b[2]), b[3], *self.material(("glass", 1.5)), True), "mort_add_moving_sphere")
        if kind == "quad":
            return S.OBJ_QUAD, Wd._ok(L.mort_add_quad(w.ptr, host.vec3(*b[1]), host.vec3(*b[2]), host.vec3(*b[3]), *self.material(("glass", 1.5)), True), "mort_add_quad")
        if kind == "list":
            refs = [self.boundary(m) for m in b[1]]
            lst = Wd._ok(L.mort_add_hittable_list(w.ptr, True), "mort_add_hittable_list")
            for t, i in refs:
                assert L.mort_list_add(w.ptr, lst, t, i) == 0
            return S.OBJ_HITTABLE_LIST, lst
        if kind == "T":
            t, i = self.boundary(b[1])
            return S.OBJ_TRANSLATE, Wd._ok(L.mort_add_translate(w.ptr, t, i, host.vec3(*b[2]), True), "mort_add_translate")
        if kind == "R":
            t, i = self.boundary(b[1])
            return S.OBJ_ROTATE_Y, Wd._ok(L.mort_add_rotate_y(w.ptr, t, i, b[2], True), "mort_add_rotate_y")
        if kind == "medium":
            return S.OBJ_CONSTANT_MEDIUM, self.medium(b[1], True)
        assert kind == "tag", b
        return b[1], b[2]

    def medium(self, m, skip):
        """m: dict(b boundary, d density, phase material, [wraps: ("R", degrees) / ("T", offset) around the medium, innermost first]);
        returns the medium's index.  Under wraps the medium is skipped by the scan and the outermost wrap is not."""
        wraps = m.get("wraps", ())
        t, i = self.boundary(m["b"])
        mt, mi = self.material(m["phase"])
        idx = Wd._ok(self.L.mort_add_constant_medium(self.w.ptr, t, i, m["d"], mt, mi, skip or bool(wraps)), "mort_add_constant_medium")
        t, i = S.OBJ_CONSTANT_MEDIUM, idx
        for k, wr in enumerate(wraps):
            outer = skip or k + 1 < len(wraps)
            if wr[0] == "T":
                t, i = S.OBJ_TRANSLATE, Wd._ok(self.L.mort_add_translate(self.w.ptr, t, i, host.vec3(*wr[1]), outer), "mort_add_translate")
            else:
                t, i = S.OBJ_ROTATE_Y, Wd._ok(self.L.mort_add_rotate_y(self.w.ptr, t, i, wr[1], outer), "mort_add_rotate_y")
        return idx


_BASE_SPHERES = [((0, -100.5, -1), 100, ("checker", 0.32)), ((-1.9, -0.3, -0.2), 0.2, ("lamb", (.7, .3, .3))),
                 ((1.9, -0.3, -0.2), 0.2, ("lamb", (.3, .7, .3))), ((0.0, -0.35, 0.7), 0.15, ("lamb", (.3, .3, .7)))]
_BASE_QUADS = [((-3.0, -0.5, -5.0), (6.0, 0, 0), (0, 2.5, 0), ("lamb", (.6, .5, .3)))]


def build(spec, with_media=True):
    """the base, the world's own spheres and quads, its media in order, then a non-skip list of `in_list` = media and spheres.
    with_media False: the same world without its media -- their materials are added all the same, so every index is the same"""
    b = _Builder()
    for s in _BASE_SPHERES + list(spec.get("spheres", ())):
        b.sphere(s, False)
    for Qp, u, v, mat in _BASE_QUADS + list(spec.get("quads", ())):
        Wd._ok(b.L.mort_add_quad(b.w.ptr, host.vec3(*Qp), host.vec3(*u), host.vec3(*v), *b.material(mat), False), "mort_add_quad")
    if not with_media:
        medium = lambda m, skip: (b.material(("glass", 1.5)), b.material(m["phase"]))  # noqa: E731
    else:
        medium = b.medium
    for m in spec["media"]:
        medium(m, False)
    if "in_list" in spec:
        refs = [(S.OBJ_CONSTANT_MEDIUM, medium(e, True)) if isinstance(e, dict) else (S.OBJ_SPHERE, b.sphere(e, True)) for e in spec["in_list"]]
        refs = [ref for ref in refs if with_media or ref[0] == S.OBJ_SPHERE]
        lst = Wd._ok(b.L.mort_add_hittable_list(b.w.ptr, False), "mort_add_hittable_list")
        for t, i in refs:
            assert b.L.mort_list_add(b.w.ptr, lst, t, i) == 0
    b.w.c.bvh_mode = False
    return b.w


# ---------------------------------------------------------------------------------------------------------------- the worlds

def _iso(k):
    """an isotropic phase function of its own colour (the reference's table holds 20)"""
    return ("iso", (round(0.25 + 0.035 * k, 3), round(0.9 - 0.03 * k, 3), round(0.3 + 0.6 * ((k * 7) % 10) / 10, 3)))


def _ball(c, r, d, k, **kw):
    return {"b": ("sphere", c, r), "d": d, "phase": _iso(k), **kw}


def _negative_far():
    rng = np.random.default_rng(2024)
    pal = [("lamb", (.7, .3, .3)), ("lamb", (.3, .6, .7)), ("lamb", (.8, .8, .3)), ("lamb", (.5, .5, .5)), ("metal", (.8, .8, .7), 0.1), ("glass", 1.5)]
    pos = lambda: (float(rng.uniform(-2.6, 2.6)), float(rng.uniform(-0.3, 1.7)), float(rng.uniform(-4.0, 0.6)))  # noqa: E731
    quads = [(pos(), Wd._v(rng.uniform(-0.45, 0.45, 3)), Wd._v(rng.uniform(-0.45, 0.45, 3)), pal[int(rng.integers(0, len(pal)))]) for _ in range(60)]
    spheres = [(pos(), float(rng.uniform(0.07, 0.22)), pal[int(rng.integers(0, len(pal)))]) for _ in range(40)]
    media = [_ball((-1.1, 0.5, 0.2), 0.4, -1e-3, 0), _ball((0.0, 1.0, -0.4), 0.4, -1e-4, 1), _ball((1.1, 0.5, 0.2), 0.4, -1e-6, 2)]
    return dict(spheres=spheres, quads=quads, media=media)


_SHAPES = [
    dict(b=("msphere", (-1.7, -0.05, -0.6), (-1.45, 0.15, -0.6), 0.33), d=2.0, phase=_iso(0)),
    # two spheres that overlap: from inside the first the next surface is the second's, not the first's exit
    dict(b=("list", [("sphere", (-0.75, -0.05, -0.6), 0.28), ("sphere", (-0.35, -0.05, -0.6), 0.28)]), d=2.0, phase=_iso(1)),
    dict(b=("list", [("quad", (0.25, -0.4, -0.45), (0.7, 0, 0), (0, 0.7, 0)), ("quad", (0.25, -0.4, -0.85), (0.7, 0, 0), (0, 0.7, 0))]), d=2.0, phase=_iso(2),
         at=((0.6, -0.05, -0.65), 0.18)),
    dict(b=("quad", (1.3, -0.4, -0.6), (0.6, 0, 0), (0, 0.7, 0)), d=2.0, phase=_iso(3), at=((1.6, -0.05, -0.6), 0.15)),
    dict(b=("sphere", (-1.3, 0.95, -1.8), -0.38), d=2.0, phase=_iso(4)),
    dict(b=("sphere", (0.0, 0.95, -1.8), 0.0), d=2.0, phase=_iso(5)),
    dict(b=("T", ("R", ("sphere", (0.0, 0.0, 0.0), 0.38), 30.0), (1.3, 0.95, -1.8)), d=2.0, phase=_iso(6)),
]
LONE_QUAD, ZERO_RADIUS = 3, 5  # in boundary_shapes

_FIFTY = dict(
    # touching spheres along x, the far end first in the table: the scan evaluates far media first, so a ray down the row draws in
    # every medium it crosses, whichever of them ends it
    media=[_ball((-6.0 + 0.4 * k, 0.6, 1.0), 0.2, 8.0, 0, phase=(("iso", (.3 + .03 * k, .5, .6)) if k < 20 else ("lamb", (.2, .3 + .02 * (k - 20), .8))))
           for k in reversed(range(MAX_MEDIA))],
    view=dict(frm=(-8.0, 1.0, 1.5), at=(13.6, 0.6, 1.0), vfov=30), width=80)

# name -> dict(media, [spheres, quads, in_list], [view, width])
MEDIUM_WORLDS = {
    "density_edges": dict(media=[_ball((float(-1.5 + (k % 4)), -0.1 + (k // 4), -0.8 - (k // 4)), 0.35, d, k) for k, d in enumerate(DENSITY_EDGES)]),
    "negative_far": _negative_far(),
    "boundary_shapes": dict(media=_SHAPES),
    "transformed_phase": dict(media=[
        dict(b=("sphere", (0, 0, 0), 0.45), d=3.0, phase=("lamb", (.8, .8, .3)), wraps=(("R", 25.0), ("T", (-1.2, 0.1, -0.8)))),
        dict(b=("sphere", (0, 0, 0), 0.45), d=3.0, phase=("metal", (.9, .7, .7), 0.3), wraps=(("T", (0.0, 0.95, -1.8)),)),
        # a chain of three: translate (rotate_y (medium (translate (sphere))))
        dict(b=("T", ("sphere", (0.3, 0, 0), 0.45), (-0.2, 0, 0.1)), d=3.0, phase=("lamb", (.3, .7, .8)), wraps=(("R", -40.0), ("T", (1.2, 0.1, -0.8))))]),
    "overlap_nested": dict(
        media=[_ball((-1.4, 0.0, -0.8), 0.4, 2.0, 0), _ball((-0.95, 0.0, -0.8), 0.4, 2.0, 1),             # overlapping, equal density
               _ball((0.25, 0.15, -1.0), 0.6, 0.3, 2), _ball((0.25, 0.15, -1.0), 0.25, 8.0, 3),            # a dense medium inside a thin one
               _ball((1.5, 0.0, -0.6), 0.45, 4.0, 4)],                                                     # a dense medium around a solid sphere
        spheres=[((1.5, 0.0, -0.6), 0.2, ("lamb", (.9, .2, .6)))]),
    "fifty_media": _FIFTY,
    # the list is scanned after the top-level medium and holds a solid: order matters, no unified tree
    "medium_in_list": dict(media=[_ball((0.9, 0.3, -0.6), 0.45, 2.0, 0)],
                           in_list=[_ball((-0.8, 0.1, -0.8), 0.45, 2.0, 1), ((0.2, 0.0, -1.2), 0.35, ("lamb", (.4, .4, .9)))]),
    # the camera (0, 0.8, 2.5) inside a medium that reaches to z = -1; a medium of negative density behind it
    "camera_inside": dict(media=[_ball((0.0, 0.5, 1.5), 2.6, 0.7, 0), _ball((0.5, 0.3, -2.6), 0.8, -0.5, 1)]),
}
NAMES = sorted(MEDIUM_WORLDS)
NO_TREE = ("medium_in_list",)
TREE_NAMES = [n for n in NAMES if n not in NO_TREE]


@functools.lru_cache(maxsize=None)
def world(name):
    return build(MEDIUM_WORLDS[name])


@functools.lru_cache(maxsize=None)
def solids_world(name):
    return build(MEDIUM_WORLDS[name], with_media=False)


def camera(name):
    spec = MEDIUM_WORLDS[name]
    cam = Wd.flat_camera(spp=4, width=spec.get("width", 96), depth=12)
    if "view" in spec:
        Wd.set_view(cam, spec["view"]["frm"], spec["view"]["at"], vfov=spec["view"].get("vfov"))
    return cam


def media_of(w):
    """every medium of the world's table, skipped by the scan or not: [(mat_type, mat_idx) of its phase function]"""
    o = w.c.objs
    return [(o.host_constant_medium[i].mat_type, o.host_constant_medium[i].mat_idx) for i in range(o.num_constant_medium)]


@functools.lru_cache(maxsize=None)
def frame_reference(name):
    return M._frozen(O.render(world(name), camera(name), nthreads=8))


@functools.lru_cache(maxsize=None)
def features_reference(name):
    from tests.feature_ref import oracle_features
    return oracle_features(world(name), camera(name), nthreads=8)


# ---------------------------------------------------------------------------------------------------------------- the rays

def _to_world(p, wraps):
    """a point of an object's frame through ("R", degrees) / ("T", offset), innermost first (rotate_y::hit, translate::hit)"""
    p = np.asarray(p, np.float64)
    for wr in wraps:
        if wr[0] == "T":
            p = p + np.asarray(wr[1], np.float64)
        else:
            s, c = np.sin(np.radians(wr[1])), np.cos(np.radians(wr[1]))
            p = np.array([c * p[0] + s * p[2], p[1], -s * p[0] + c * p[2]])
    return p


def _inside_of(b):
    """(centre, radius) of a ball inside a boundary, in the boundary's own frame (a moving sphere: at time 0.5, half its radius)"""
    if b[0] == "sphere":
        return np.asarray(b[1], np.float64), abs(b[2])
    if b[0] == "msphere":
        return 0.5 * (np.asarray(b[1], np.float64) + np.asarray(b[2], np.float64)), 0.5 * abs(b[3])
    if b[0] == "list":
        return _inside_of(b[1][0])
    assert b[0] in ("T", "R"), b
    c, r = _inside_of(b[1])
    return _to_world(c, [("T", b[2])] if b[0] == "T" else [("R", b[2])]), r


def probes(name):
    """per medium of the world's table: (centre, radius) of a ball inside its boundary, in world space"""
    spec = MEDIUM_WORLDS[name]
    out = []
    for m in list(spec["media"]) + [e for e in spec.get("in_list", ()) if isinstance(e, dict)]:
        c, r = m["at"] if "at" in m else _inside_of(m["b"])
        out.append((_to_world(c, m.get("wraps", ())), float(r)))
    return out


INSIDE_PER_MEDIUM = 40


class Rays:
    """rays (n, 8); slices primary / cut / inside; streams0, streams: before and after the oracle's closest hits with media (rec, hit);
    srec, shit: the oracle's closest hits with every medium passed over; advanced (n,) and draws (n,): what each stream drew"""


@functools.lru_cache(maxsize=None)
def rays(name):
    w, cam = world(name), camera(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    r = Rays()
    prim = Q.ray8(primary_rays(cam), Q.INF)
    pr = probes(name)
    cen = np.array([c for c, _ in pr])
    # every eighth primary ray again, cut at the point nearest the centre of the medium it passes nearest
    cut = prim[3::8].copy()
    o, d = cut[:, 0:3].astype(np.float64), cut[:, 3:6].astype(np.float64)
    t = ((cen[None, :, :] - o[:, None, :]) * d[:, None, :]).sum(2) / (d * d).sum(1)[:, None]       # (rays, media)
    miss = np.linalg.norm(o[:, None, :] + t[:, :, None] * d[:, None, :] - cen[None, :, :], axis=2)
    miss[t <= 0] = np.inf
    cut[:, 7] = t[np.arange(len(cut)), miss.argmin(1)].astype(F)
    # rays that start inside each boundary, uniform directions, times over the shutter
    k = INSIDE_PER_MEDIUM
    org = np.concatenate([c + 0.9 * rad * Q._unit_sphere(rng, k) * rng.random((k, 1)) ** (1 / 3) for c, rad in pr])
    inside = Q.ray8(np.concatenate([org, Q._unit_sphere(rng, len(org)), rng.random((len(org), 1))], axis=1), Q.INF)
    r.rays = np.concatenate([prim, cut, inside])
    r.slices = dict(primary=slice(0, len(prim)), cut=slice(len(prim), len(prim) + len(cut)), inside=slice(len(prim) + len(cut), len(r.rays)))
    r.streams0 = Q.some_streams(len(r.rays))
    r.streams = r.streams0.copy()
    r.rec, r.hit = Q.oracle_closest(w, r.rays, states=r.streams)
    # media passed over: the world without them (setting `skip` would not reach a medium under a transform or in a list)
    same = r.streams0.copy()
    r.srec, r.shit = O.world_hit_batch(solids_world(name), r.rays[:, :7], Q.T_MIN, r.rays[:, 7], states=same)
    assert same.tobytes() == r.streams0.tobytes(), "the oracle drew a random number in a world without media"
    r.advanced = (r.streams.view(np.uint8).reshape(-1, 48) != r.streams0.view(np.uint8).reshape(-1, 48)).any(1)
    r.draws = (r.streams["d"] - r.streams0["d"]) // np.uint32(362437)  # XORWOW's Weyl word steps by 362437 per draw
    mats = media_of(w)
    r.medium = np.full(len(r.rays), -1)  # which medium of the table ends the ray
    for i, (mt, mi) in enumerate(mats):
        r.medium[r.hit & (r.rec["mat_type"] == mt) & (r.rec["mat_idx"] == mi)] = i
    for a in (r.rays, r.streams0, r.streams, r.rec, r.hit, r.srec, r.shit, r.advanced, r.draws, r.medium):
        a.setflags(write=False)
    return r


def assert_hits_equal(name, got, with_media, what):
    """Q.assert_hits_equal with the medium hits told by their phase material: the normal of a medium under rotate_y is not (1, 0, 0)"""
    r = rays(name)
    rec, hit = (r.rec, r.hit) if with_media else (r.srec, r.shit)
    Q.assert_hits_equal(world(name), got, rec, hit, what, with_media=with_media, medium_hits=(r.medium >= 0) if with_media else None)


# ------------------------------------------------------------------------------------------------- radiance along the frame's rays

@functools.lru_cache(maxsize=None)
def radiance_reference(name):
    from tests import radiance_ref as R
    w, cam = world(name), camera(name)
    r = M.RayRef()
    r.rays = M.primary_rays(cam)
    r.params = hip.radiance_params_from_camera(cam, 1)
    r.streams0 = Q.some_streams(len(r.rays))
    r.streams = r.streams0.copy()
    r.rgb = R.oracle_radiance(w, cam, r.rays, r.streams, 1)
    for a in (r.rays, r.streams0, r.streams, r.rgb):
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def probe_reference(name):
    """one SH9 probe at the camera's own position, 64 directions, one path each"""
    from tests import probe_ref as P
    from tests import radiance_ref as R
    w, cam = world(name), camera(name)
    r = P.Ref()
    r.world, r.cam = w, cam
    r.params = hip.probe_params_from_camera(cam, M.PROBE_D, 1)
    r.probes = np.zeros(1, dtype=hip.PROBE_DTYPE)
    r.probes["position"] = tuple(cam.center.e[k] for k in range(3))
    r.probes["time"] = 0.5
    r.dirs = P.fibonacci(M.PROBE_D)
    r.streams0 = Q.some_streams(M.PROBE_D)
    r.streams = r.streams0.copy()
    r.s = R.oracle_radiance(w, cam, P.rays_of(r.probes, r.dirs), r.streams, 1).reshape(1, M.PROBE_D, 3)
    r.sh = P.project(r.s, r.dirs, 1)
    for a in (r.probes, r.dirs, r.streams0, r.streams, r.s, r.sh):
        a.setflags(write=False)
    return r


# ------------------------------------------------------------------------------------- worlds the compile step refuses or trims

def odd_boundary_world(boundary):
    """the base and ONE medium (density 2) bounded by `boundary`, after a plain medium; boundary None: without that medium, its
    materials still in the tables"""
    b = _Builder()
    for s in _BASE_SPHERES:
        b.sphere(s, False)
    for Qp, u, v, mat in _BASE_QUADS:
        Wd._ok(b.L.mort_add_quad(b.w.ptr, host.vec3(*Qp), host.vec3(*u), host.vec3(*v), *b.material(mat), False), "mort_add_quad")
    b.medium(_ball((-0.9, 0.2, -0.8), 0.45, 2.0, 0), False)
    b.material(_iso(1))
    if boundary is not None:
        b.medium(dict(b=boundary, d=2.0, phase=_iso(1)), False)
    b.w.c.bvh_mode = False
    return b.w
