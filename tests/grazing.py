"""Cameras aimed at silhouettes and box faces ("margin audit"): the rays a tree walk's error-bound argument is
for.  A whole image of a scene holds about one such ray in 1e8; the "microscope" built here is a 65 x 65 viewport a few
millionths of the target's size wide, put around one chosen point of a primitive, so that every primary ray of the frame grazes.
A mort_camera is plain data: the kernels, the host loop, the oracle and tests/feature_ref.py read centre, pixel00_loc, the two
pixel deltas and the image size, so such a camera needs no vfov that an int of degrees could express.

Shared by tests/test_grazing_host.py (CPU) and tests/test_gpu_grazing.py: the case table CASES, the worlds, the oracle
references (computed once per case and left unchanged) and the conditions every case asserts on the oracle's result alone."""
import math

import numpy as np

from mort_amd import host, structs as S
from tests import oracle_lib as O
from tests.feature_ref import MEDIUM, oracle_features, primary_rays
from tests.worlds import PLACED, custom_bvh_world, flat_world

NT = 8
F = np.float32
# solid Lambertian colours that are exact in fp32 and that nothing else in a world uses: "this ray hit the target" is read off
# the oracle's albedo
TARGETS = ((0.125, 0.625, 0.875), (0.875, 0.125, 0.625), (0.625, 0.875, 0.125), (0.375, 0.0625, 0.75))
TARGET = TARGETS[0]
AXES = {"-x": (-1, 0, 0), "+x": (1, 0, 0), "-y": (0, -1, 0), "+y": (0, 1, 0), "-z": (0, 0, -1), "+z": (0, 0, 1)}


# ---- cameras ----
_TEMPLATE = []


def _blank_camera():
    if not _TEMPLATE:
        _, cam = host.build_scene(2, width=65, spp=1, depth=8)
        _TEMPLATE.append(cam)
    return S.Camera.from_buffer_copy(_TEMPLATE[0])


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / math.sqrt(float(v @ v))


def microscope(cam, origin, target, span, W=65, H=65):
    """Aims `cam` from `origin` at `target`: the viewport is centred on the target, perpendicular to target - origin, and the
    W pixel centres of a row span `span` world units.  The ray through pixel ((W-1)/2, (H-1)/2) passes through the target; with a
    power-of-two span and an aim along an axis plane its whole column (or row) has a direction component of exactly 0."""
    o, t = np.asarray(origin, dtype=np.float64), np.asarray(target, dtype=np.float64)
    w = _unit(t - o)
    up = np.eye(3)[int(np.argmin(np.abs(w)))]  # the axis most nearly perpendicular to the aim
    u = _unit(np.cross(up, w))
    v = np.cross(w, u)
    du, dv = u * (span / (W - 1)), v * (span / (H - 1))
    p00 = t - du * ((W - 1) / 2) - dv * ((H - 1) / 2)
    cam.image_width, cam.image_height = W, H
    cam.aspect_ratio = W / H
    cam.samples_per_pixel, cam.sqrt_spp, cam.recip_sqrt_spp, cam.pixel_samples_scale = 1, 1, 1.0, 1.0
    cam.defocus_angle = 0.0
    for k in range(3):
        cam.center.e[k] = cam.lookfrom.e[k] = o[k]
        cam.lookat.e[k] = t[k]
        cam.pixel00_loc.e[k] = p00[k]
        cam.pixel_delta_u.e[k] = du[k]
        cam.pixel_delta_v.e[k] = dv[k]
        cam.u.e[k], cam.v.e[k], cam.w.e[k] = u[k], v[k], -w[k]
    return cam


def limb(c, r, origin, side):
    """the point where a line from `origin` touches the sphere (c, r), on the side of the silhouette that faces `side`"""
    c, o = np.asarray(c, dtype=np.float64), np.asarray(origin, dtype=np.float64)
    L = math.sqrt(float((c - o) @ (c - o)))
    w = (c - o) / L
    s = np.asarray(side, dtype=np.float64)
    s = _unit(s - (s @ w) * w)
    sin_a = r / L
    return c + r * (-sin_a * w + math.sqrt(1.0 - sin_a * sin_a) * s)


# ---- worlds ----
def _crowd(rng, n, centre, scale, radius):
    """n small spheres of every material kind in the octant beyond `centre` (+x, +z): a target at `centre` defines the low
    corner of its tree nodes, and cameras on its -x / -z side see it unobstructed"""
    out = []
    for k in range(n):
        p = np.asarray(centre) + scale * np.array([rng.uniform(2.5, 9), rng.uniform(-0.5, 4), rng.uniform(2.5, 9)])
        mat = [("lamb", tuple(rng.uniform(0.1, 0.9, 3))), ("metal", tuple(rng.uniform(0.3, 0.9, 3)), float(rng.uniform(0, 0.5))),
               ("checker",), ("lamb", tuple(rng.uniform(0.1, 0.9, 3)))][k % 4]
        out.append(("sphere", tuple(float(x) for x in p), float(radius * rng.uniform(0.5, 1.0)), mat))
    return out


GROUND = ("sphere", (0, -1000, 0), 1000, ("lamb", (.5, .5, .5)))


def _sphere_world(r, ground=True, seed=0, centre=None):
    """the issue's recipe: 1000-radius ground, the target, a glass sphere, 50 small spheres"""
    c = (0.0, 2.0 * r, 0.0) if centre is None else centre
    rng = np.random.default_rng(77 + seed)
    prims = ([GROUND] if ground else []) + [("sphere", c, r, ("lamb", TARGET)),
                                            ("sphere", (c[0] + 4 * r, c[1] + r, c[2] + 3 * r), 1.5 * r, ("glass", 1.5))]
    prims += _crowd(rng, 50, c, r, 0.4 * r)
    return flat_world(prims)[0]


QUAD = ((-1.0, 1.5, -1.0), (2.0, 0.0, 0.0), (0.0, 0.25, 2.0))
AQUAD = ((-6.0, 3.0, -5.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0))  # axis-aligned, seen straight down y
RBOX = ((1.0, 1.5, 1.0), (-9.0, 0.0, -6.0), 25.0)
MOVER = ((-3.0, 4.0, -8.0), (-3.0, 4.5, -8.0), 0.5)


def _shapes_world():
    rng = np.random.default_rng(78)
    prims = [GROUND, ("quad",) + QUAD + (("lamb", TARGETS[0]),), ("quad",) + AQUAD + (("lamb", TARGETS[1]),),
             ("rbox",) + RBOX + (("lamb", TARGETS[2]),), ("msphere",) + MOVER + (("lamb", TARGETS[3]),),
             ("sphere", (4.0, 1.0, 5.0), 1.0, ("glass", 1.5))]
    prims += _crowd(rng, 50, (2.0, 0.5, 2.0), 1.0, 0.4)
    return flat_world(prims)[0]


def _medium_world():
    rng = np.random.default_rng(79)
    prims = [GROUND] + _crowd(rng, 50, (0.0, 0.5, 0.0), 1.0, 0.4)
    return flat_world(prims, media=[((-2.0, 1.0, -2.0), 0.5, 1.0, (.9, .4, .2))])[0]


def _tiny_beside_giant_world():
    """no ground; a radius-0.01 target at the low corner of a cloud 20 units wide, so that kmin = 20u / r_min and the sphere term
    of the static pad (20u M^2 / r, M = mnear) are large next to every fixed pad.  The target's -x, -y and -z box faces lie in the
    coordinate planes: a ray in such a face has a zero product o * inv on that axis and so the narrowest band"""
    rng = np.random.default_rng(80)
    prims = [("sphere", (0.01, 0.01, 0.01), 0.01, ("lamb", TARGET)), ("sphere", (14.0, 6.0, 12.0), 4.0, ("glass", 1.5))]
    prims += _crowd(rng, 50, (0.0, 0.0, 0.0), 2.0, 0.6)
    return flat_world(prims)[0]


def _tiny_in_wide_cloud_world():
    """the same target at the corner of a cloud 200 units wide: 130 units away a camera is still a near one (inside mnear, so no
    per-ray widening), where u L^2 is ten times r^2 -- sphere::hit accepts rays that pass three radii from the centre, outside
    every pad but the static sphere term"""
    rng = np.random.default_rng(83)
    prims = [("sphere", (0.01, 0.01, 0.01), 0.01, ("lamb", TARGET)), ("sphere", (140.0, 60.0, 120.0), 30.0, ("glass", 1.5))]
    prims += _crowd(rng, 50, (0.0, 0.0, 0.0), 20.0, 6.0)
    return flat_world(prims)[0]


def _bare_world(r, sign):
    """no ground: a target sphere whose box faces on the `sign` side lie in the coordinate planes, first (sign -1) or last (+1) in
    every axis of a small crowd"""
    rng = np.random.default_rng(81)
    c = (-sign * r,) * 3
    prims = [("sphere", c, r, ("lamb", TARGET)), ("sphere", (-sign * 5 * r, -sign * 4 * r, -sign * 6 * r), 1.5 * r, ("glass", 1.5))]
    for p in _crowd(rng, 50, (0, 0, 0), r, 0.4 * r):
        prims.append((p[0], tuple(-sign * x for x in p[1])) + p[2:])
    return flat_world(prims)[0]


BVH_R = 0.5
BVH_C = (0.0, 1.0, 0.0)
BVH_ALONE = (-40.0, 3.0, -40.0)  # far from every other sphere: alone in its reference leaf node


def _bvh_world():
    rng = np.random.default_rng(82)
    spheres = [((0, -1000, 0), 1000, ("lamb", (.5, .5, .5))), (BVH_C, BVH_R, ("lamb", TARGETS[0])), (BVH_ALONE, BVH_R, ("lamb", TARGETS[1]))]
    for k in range(120):
        p = (float(rng.uniform(1.5, 9)), float(rng.uniform(0.2, 3)), float(rng.uniform(1.5, 9)))
        spheres.append((p, 0.2, [("lamb", tuple(rng.uniform(0.1, 0.9, 3))), ("metal", (.7, .6, .5), 0.1), ("glass", 1.5)][k % 3]))
    return custom_bvh_world(spheres)


WORLDS = {"sphere_0.01": lambda: _sphere_world(0.01), "sphere_0.5": lambda: _sphere_world(0.5), "sphere_10": lambda: _sphere_world(10.0),
          "shapes": _shapes_world, "medium": _medium_world, "grazed_medium": lambda: PLACED["grazed_medium"]()[0],
          "tiny_beside_giant": _tiny_beside_giant_world, "tiny_in_wide_cloud": _tiny_in_wide_cloud_world,
          "bare_0.5_lo": lambda: _bare_world(0.5, -1), "bare_0.5_hi": lambda: _bare_world(0.5, +1),
          "bare_10_lo": lambda: _bare_world(10.0, -1), "bare_0.01_lo": lambda: _bare_world(0.01, -1),
          "bvh": _bvh_world}
_WORLD_CACHE = {}


def world(name):
    if name not in _WORLD_CACHE:
        _WORLD_CACHE[name] = WORLDS[name]()
    return _WORLD_CACHE[name]


# ---- cases ----
class Case:
    """One frame.  cond: "silhouette" (share of target pixels in [0.15, 0.85]), "zero" (>= 65 rays with a component of exactly 0),
    "face" (the same 65 rays in the feature pass; the render's jittered rays straddle the face instead of lying in it),
    "over" (>= 5 % of the rays hit the target by the oracle while the float64 discriminant of the same fp32 ray is negative),
    "medium" (share of medium pixels in [0.15, 0.85]).  walk: "tree" | "scan" (beyond reach) | "bvh"."""

    def __init__(self, group, name, world, origin, aim, span, cond=("silhouette",), colour=0, walk="tree", sphere=None, camera=None):
        self.group, self.name, self.world, self.origin, self.aim, self.span = group, name, world, origin, aim, span
        self.cond, self.colour, self.walk, self.sphere, self._camera = tuple(cond), colour, walk, sphere, camera

    def __repr__(self):
        return f"{self.group}/{self.name}"

    def camera(self):
        if self._camera is not None:
            return self._camera()
        aim = self.aim(self) if callable(self.aim) else self.aim
        return microscope(_blank_camera(), self.origin, aim, self.span)


CASES = []
DIAG = _unit((-0.48, 0.62, -0.62))  # where the limb cameras stand: above the ground, on the side the crowd leaves free
IN_PLANE = {"x": _unit((0.0, 0.6, -0.8)), "y": _unit((-0.6, 0.0, -0.8)), "z": _unit((-0.8, 0.6, 0.0))}
UP = _unit((-0.1, 0.99, -0.1))


def _add(*a, **kw):
    CASES.append(Case(*a, **kw))


def _sphere_cases():
    for r in (0.01, 0.5, 10.0):
        wname, c = f"sphere_{r:g}", np.array((0.0, 2.0 * r, 0.0))
        sph = (tuple(c), r)
        for L in (3, 40, 150, 2000):
            o = c + L * r * DIAG
            for side, s in AXES.items():
                spans = {3: (-6, -14), 40: (-6, -10), 150: (-5, -6), 2000: (-5, -7)}[L]
                if r == 0.01 and L == 2000:  # r^2 is 3 ulp of |oc|^2 here: the fp32 silhouette is ragged, finer spans show one side of it only
                    spans = (0, -1, -2)
                for e in spans:
                    _add(f"limb_r{r:g}", f"L{L}r{side}span2^{e}", wname, o, limb(c, r, o, s), r * 2.0 ** e, sphere=sph)
        # the ray in the tangent plane of an axis pole: the centre ray runs in the face of the primitive's box
        for side, s in AXES.items():
            pole = c + r * np.array(s, dtype=np.float64)
            for L in (3, 40):
                o = pole + L * r * IN_PLANE[side[1]]
                # coarse: a silhouette; fine (a pixel is a few ulp of the coordinates wide): the render's jittered rays, too, have
                # components of exactly 0 -- from 40 r the fp32 test accepts most of such a frame, so it is no silhouette any more
                fine = -10 if r == 0.01 else -14
                _add(f"pole_r{r:g}", f"L{L}r{side}span2^-6", wname, o, pole, r * 2.0 ** -6, sphere=sph)
                _add(f"pole_r{r:g}", f"L{L}r{side}span2^{fine}", wname, o, pole, r * 2.0 ** fine, cond=("zero",) + (("silhouette",) if L == 3 else ()), sphere=sph)
    # beyond the tree's reach: the host loop and the GPU launch fall back to the reference's scan
    c, r = np.array((0.0, 20.0, 0.0)), 10.0
    o = c + 20000.0 * UP
    for side in ("-x", "+z"):
        _add("beyond_reach", f"L20000{side}", "sphere_10", o, limb(c, r, o, AXES[side]), r * 2.0 ** -6, walk="scan", sphere=(tuple(c), r))
    # far origins, where fp32 accepts hits the exact line misses (the class of the round-1 regression)
    for L, span in ((300, 1e-2), (300, 1e-4), (1500, 1e-2), (1500, 1e-4)):
        o = c + L * DIAG
        for side in ("-x", "+y", "-z"):
            _add("over_accepted", f"L{L}{side}span{span:g}", "sphere_10", o, limb(c, r, o, AXES[side]), span, cond=("over",), sphere=(tuple(c), r))


def _shape_cases():
    Q, u, v = (np.array(x) for x in QUAD)
    for k, o in enumerate(((0.3, 8.0, 0.2), (40.0, 30.0, -20.0), (900.0, 700.0, 500.0))):
        for span in ((1e-2, 1e-5) if k < 2 else (1e-2,)):
            _add("quad", f"edge_from{k}_span{span:g}", "shapes", o, Q + 0.5 * u, span)
            _add("quad", f"corner_from{k}_span{span:g}", "shapes", o, Q, span)
    # rays nearly in the quad's plane: the origin a hair above the plane, aimed at the far edge
    n = _unit(np.cross(u, v))
    for lift in (2e-3, 1e-3):
        o = Q + 0.5 * u - 3.0 * v + lift * n * (1 if n[1] > 0 else -1)
        _add("quad", f"in_plane_lift{lift:g}", "shapes", o, Q + 0.5 * u, 2.0 ** -10)
    A, au, av = (np.array(x) for x in AQUAD)
    for e in (-10, -16):  # straight down y on an edge: a column of rays has d.x == 0 (or d.z), the scan decides them
        _add("quad", f"axis_quad_down_y_span2^{e}", "shapes", A + 0.5 * av + (0, 8.0, 0), A + 0.5 * av, 2.0 ** e, cond=("silhouette", "zero"), colour=1)
        _add("quad", f"axis_quad_down_y_corner_span2^{e}", "shapes", A + (0, 8.0, 0), A, 2.0 ** e, cond=("silhouette", "zero"), colour=1)
    # a rotated box's silhouette edge through its rotate_y / translate chain: found by bisection on the oracle's own frames
    for span in (2.0 ** -4, 2.0 ** -12):
        for k, o in enumerate(((-20.0, 6.0, -18.0), (-9.0, 12.0, -30.0))):
            _add("rbox", f"edge_from{k}_span{span:g}", "shapes", o, _search_silhouette(np.array(RBOX[1]) + (0.3, 0.75, 0.6), 2), span, colour=2)
    # the moving sphere: the feature pass sees it at time 0.5, the render at the time it draws
    c0, c1, r = np.array(MOVER[0]), np.array(MOVER[1]), MOVER[2]
    mid = 0.5 * (c0 + c1)
    for L in (3, 40):
        o = mid + L * r * DIAG
        for side in ("-x", "+x", "-y", "+y"):
            _add("moving", f"L{L}r{side}", "shapes", o, limb(mid, r, o, AXES[side]), r * 2.0 ** -6, colour=3)


def _medium_cases():
    _add("medium_far", "grazed_medium", "grazed_medium", None, None, None, cond=("grazed",), walk="scan", camera=lambda: PLACED["grazed_medium"]()[1])
    c, r = np.array((-2.0, 1.0, -2.0)), 0.5
    for L in (3, 40):
        o = c + L * r * DIAG
        for side in ("-x", "+y"):
            for e in (-6, -10):
                _add("medium", f"near_L{L}r{side}span2^{e}", "medium", o, limb(c, r, o, AXES[side]), r * 2.0 ** e, cond=("medium",))


def _margin_cases():
    """the rays the static pads and the per-ray band exist for: a ray in (or a hair off) a face of the target's box, with that
    face in a coordinate plane, so that o * inv is 0 on that axis and the band is as narrow as it gets"""
    # tiny sphere beside a giant: origins inside mnear (static pad's sphere term) and outside it (kmin widening)
    c, r = np.array((0.01, 0.01, 0.01)), 0.01
    for axis, (a, b) in (("x", (1, 2)), ("y", (0, 2)), ("z", (0, 1))):
        k = "xyz".index(axis)
        pole = c.copy(); pole[k] = 0.0
        for L in (4.0, 20.0, 45.0, 120.0):  # mnear is about 37 here, reach about 150
            d = np.zeros(3); d[a], d[b] = -0.6, -0.8
            o = pole + L * d
            for tilt in (0.0, 2e-4 * L, -2e-4 * L):  # the origin a hair off the face plane: every ray has a small nonzero component
                oo = o.copy(); oo[k] += tilt
                _add("margin_tiny", f"-{axis}_L{L:g}_tilt{tilt:g}", "tiny_beside_giant", oo, pole, r * 2.0 ** -2,
                     cond=("face",) if tilt == 0.0 else ("any",), sphere=(tuple(c), r))
    # the static sphere term alone: near cameras (no widening) 100 and 130 units from the tiny sphere in the wide cloud, aimed
    # 2 and 3 radii outside its box face, a ray's small component pointing away from the box; shares of 0.24 - 0.98 measured
    for axis, (a, b) in (("x", (1, 2)), ("y", (0, 2)), ("z", (0, 1))):
        k = "xyz".index(axis)
        pole = c.copy(); pole[k] = 0.0
        for L in (100.0, 130.0):
            d = np.zeros(3); d[a], d[b] = 0.6, -0.8
            for off in (0.02, 0.03):
                aim = pole.copy(); aim[k] -= off
                _add("margin_wide", f"-{axis}_L{L:g}_off{off:g}", "tiny_in_wide_cloud", pole + L * d, aim, 0.008, cond=("over",), sphere=(tuple(c), r))
    # the far-origin widening alone: diagonal rays (every |1 / d| moderate) from 5000 and 10000 units, where u L^2 is 6 - 24 and
    # r^2 is 0.25: sphere::hit accepts rays that pass 1.2 - 2 units from the centre, past the corner of every static pad
    cs, rs = np.array((0.0, 1.0, 0.0)), 0.5
    for L, q in ((5000.0, 1.2), (5000.0, 2.0), (10000.0, 0.6), (10000.0, 1.2), (10000.0, 2.0)):
        _add("far_diagonal", f"L{L:g}_q{q:g}", "sphere_0.5", cs + L * _unit((-1.0, 0.01, -1.0)), cs + q * _unit((1.0, 0.0, -1.0)), 1.0,
             cond=("over",), sphere=(tuple(cs), rs))
    for wname, r, sign in (("bare_0.5_lo", 0.5, -1), ("bare_0.5_hi", 0.5, 1), ("bare_10_lo", 10.0, -1), ("bare_0.01_lo", 0.01, -1)):
        c = np.full(3, -sign * r)
        for axis, (a, b) in (("x", (1, 2)), ("y", (0, 2)), ("z", (0, 1))):
            k = "xyz".index(axis)
            pole = c.copy(); pole[k] = 0.0
            for L in (10, 60):  # within reach (2 diag + 4 amag + 10) of these small worlds; mnear is about 20 r
                d = np.zeros(3); d[a], d[b] = sign * 0.6, sign * 0.8
                for tilt in (0.0, 3e-5, -3e-5):
                    o = pole + L * r * d
                    o[k] += tilt * L * r
                    _add("margin_" + wname, f"{'+' if sign > 0 else '-'}{axis}_L{L}r_tilt{tilt:g}", wname, o, pole, r * 2.0 ** -8,
                         cond=("face",) if tilt == 0.0 else ("any",), sphere=(tuple(c), r))


def _bvh_cases():
    c, r = np.array(BVH_C), BVH_R
    for side, s in AXES.items():
        pole = c + r * np.array(s, dtype=np.float64)
        o = pole + 6.0 * IN_PLANE[side[1]]
        for e in (-3, -10, -17):
            _add("bvh_pole", f"{side}span2^{e}", "bvh", o, pole, 2.0 ** e, cond=("zero",) + (("silhouette",) if e > -17 else ()), walk="bvh", sphere=(tuple(c), r))
    for L in (3, 40, 150):
        o = c + L * r * DIAG
        for side in ("-x", "+x", "-y", "+y", "-z", "+z"):
            _add("bvh_limb", f"L{L}r{side}", "bvh", o, limb(c, r, o, AXES[side]), r * 2.0 ** -6, walk="bvh", sphere=(tuple(c), r))
    ca = np.array(BVH_ALONE)
    for L in (3, 40):
        o = ca + L * r * DIAG
        for side in ("-x", "+y", "-z"):
            _add("bvh_alone", f"L{L}r{side}", "bvh", o, limb(ca, r, o, AXES[side]), r * 2.0 ** -6, colour=1, walk="bvh", sphere=(tuple(ca), r))


def _search_silhouette(start, colour, steps=4):
    """an aim for a case: from the case's origin, the boundary of the colour-`colour` target nearest to `start`, refined on the
    oracle's own feature frames (each step centres a 65-pixel frame on a boundary pixel of the one before and narrows it 16 times)"""
    def aim(case):
        p, span = np.asarray(start, dtype=np.float64), 4.0
        w = world(case.world)
        for _ in range(steps):
            cam = microscope(_blank_camera(), case.origin, p, span)
            ref = oracle_features(w, cam, nthreads=NT)
            m = (ref["albedo"] == np.array(TARGETS[colour], dtype=F)).all(-1)
            edge = np.argwhere(m[:, 1:] != m[:, :-1])
            assert len(edge), f"{case}: no boundary of the target in a frame {span} wide around {p}"
            y, x = edge[np.argmin(((edge - (32, 31.5)) ** 2).sum(-1))]
            p00, du, dv = (np.array([getattr(cam, n).e[k] for k in range(3)], dtype=np.float64) for n in ("pixel00_loc", "pixel_delta_u", "pixel_delta_v"))
            p = p00 + (x + 0.5) * du + y * dv
            span /= 16.0
        return p
    return aim


_sphere_cases()
_shape_cases()
_medium_cases()
_margin_cases()
_bvh_cases()
FLAT = [c for c in CASES if c.walk != "bvh"]
BVH = [c for c in CASES if c.walk == "bvh"]
GROUPS = sorted({c.group for c in CASES})
assert len({repr(c) for c in CASES}) == len(CASES)


# ---- references and conditions ----
_REF = {}


def reference(case):
    """(world, camera, oracle features, oracle render at 1 spp and bounce limit 8): made once per case, never changed"""
    key = repr(case)
    if key not in _REF:
        w, cam = world(case.world), case.camera()
        cam.bounce_limit = 8
        feat = oracle_features(w, cam, nthreads=NT)
        ren = O.render(w, cam, nthreads=NT)
        for a in list(feat.values()) + [ren["rgba"], ren["accum"], ren["segments_px"], ren["states"]]:
            a.setflags(write=False)
        _REF[key] = (w, cam, feat, ren)
    return _REF[key]


def shares(case, cam, feat):
    """what the conditions are judged on, from the oracle's frame alone"""
    rays = primary_rays(cam)
    on_target = (feat["albedo"].reshape(-1, 3) == np.array(TARGETS[case.colour], dtype=F)).all(-1)
    out = dict(target=float(on_target.mean()), zero=int((rays[:, 3:6] == 0).any(-1).sum()), medium=float((feat["kind"] == MEDIUM).mean()),
               grazed=int((feat["grazed"] > 0).sum()), over=0.0)
    if case.sphere is not None:  # h^2 - a c in float64 on the same fp32 ray
        c, r = np.asarray(case.sphere[0], dtype=np.float64), float(case.sphere[1])
        o, d = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
        oc = o - c
        h, a, cc = (oc * d).sum(-1), (d * d).sum(-1), (oc * oc).sum(-1) - r * r
        out["over"] = float((on_target & (h * h - a * cc < 0)).mean())
    return out


def check_conditions(case, cam, feat):
    s = shares(case, cam, feat)
    for cond in case.cond:
        if cond == "silhouette":
            assert 0.15 <= s["target"] <= 0.85, f"{case}: target share {s['target']:.3f} is no silhouette"
        elif cond in ("zero", "face"):
            assert s["zero"] >= 65, f"{case}: {s['zero']} rays with a zero direction component"
        elif cond == "over":
            assert s["over"] >= 0.05, f"{case}: {s['over']:.3f} of the rays are accepted by fp32 and missed by the exact line"
        elif cond == "medium":
            assert 0.15 <= s["medium"] <= 0.85, f"{case}: medium share {s['medium']:.3f}"
        elif cond == "grazed":
            assert s["grazed"] >= 1 and 0.05 <= s["medium"] <= 0.95, f"{case}: {s}"
        else:
            assert cond == "any" and s["target"] > 0, f"{case}: the target is not in the frame"
    return s
