"""MATERIAL_WORLDS: small worlds whose materials lie where no other catalogue goes -- refraction indices 1, 0.1, 1e30, 1e-30, 0, -1.5,
inf and NaN, fuzz 0, 5, -1, inf and NaN, albedos 0, above 1, negative, inf and NaN, checker scales 0, inf, negative, 1e-30, 1e30 and NaN,
each at radius +0.3 and -0.3; a camera inside glass; a closed hall of mirrors that runs every path to the bounce limit; moving spheres of
every material; material and texture tags outside the known set; an isotropic material on surfaces and surface materials as a medium's
phase function; textured emission seen from the front and from the back.

Most worlds come in two forms over the same spheres: "flat" (the scan and, where the world has one, the unified tree: shade_hit of
dev_shade.h) and "bvh" (one reference BVH: the inline shade blocks of mega_bvh.h and wave_bvh.h).  Frames are 64 x 36 (mirror_hall
48 x 27), 4 spp, bounce limit 12 unless the world says otherwise; one oracle render per (world, form), shared by every test.

tests/test_material_worlds_host.py runs them through the host loop, tests/test_gpu_material_worlds.py through every kernel form."""
import ctypes as C
import functools

import numpy as np

from mort_amd import hip, host, structs as S
from tests import oracle_lib as O
from tests import worlds as Wd

F = np.float32
INF, NAN = float("inf"), float("nan")

IORS = (1.0, 0.1, 1e30, 1e-30, 0.0, -1.5, INF, NAN)
FUZZES = (0.0, 5.0, -1.0, INF, NAN)
ALBEDOS = ((0.0, 0.0, 0.0), (1.5, 2.0, 4.0), (-0.5, -0.2, -1.0), (INF, 0.5, INF), (NAN, 0.5, 0.5))
CHECKER_SCALES = (0.0, INF, -0.32, 1e-30, 1e30, NAN)

# the rows of the tag table: name -> ("tex", texType, texIdx) on a Lambertian, or ("mat", mat_type, mat_idx) on the sphere.
# The first four alias a known tag when a compile step packs them into 15 + 16 bits without looking: a zeroed texture struct is the
# "colour inlined" value, 0x8001 loses its top bit and is SOLID, 0x10002 loses its top bit and is METAL, and index 0x20000 spills into
# the tag field as METAL.  Every aliased index is 0 and the world holds solid colour 0 and metal 0, so a wrong build reads valid memory
# and paints a wrong picture.
TAG_ROWS = {"tex_zeroed": ("tex", 0, 0), "tex_high_bit": ("tex", 0x8001, 0), "mat_high_bits": ("mat", 0x10002, 0), "mat_index_spill": ("mat", 0, 0x20000),
            "tex_0_3": ("tex", 0, 3), "tex_7_0": ("tex", 7, 0), "tex_5_0": ("tex", 5, 0), "tex_minus1_0": ("tex", -1, 0),
            "mat_0_0": ("mat", 0, 0), "mat_6_0": ("mat", 6, 0), "mat_9_0": ("mat", 9, 0), "mat_9_minus1": ("mat", 9, -1), "mat_minus1_0": ("mat", -1, 0)}
ALIASING_ROWS = ("tex_zeroed", "tex_high_bit", "mat_high_bits", "mat_index_spill")


class _Builder:
    """materials by description, each distinct description added once (the reference's tables are small).  Descriptions:
    ("lamb" | "light" | "iso", rgb), ("metal", rgb, fuzz), ("glass", ior), ("checker", scale[, kind]) -- nested to the allowed depth when
    scale is a tuple --, ("noise"[, kind]), ("image"[, kind]) with kind "lamb" (default), "light" or "iso", ("tex", texType, texIdx): a
    Lambertian over that texture reference as given, ("mat", mat_type, mat_idx): that material reference as given."""

    def __init__(self):
        self.L = host.lib()
        self.w = host.World()
        self.seen = {}
        self.noise = None

    def _textured(self, kind, tt, ti):
        add = {"lamb": self.L.mort_add_lambertian, "light": self.L.mort_add_diffuse_light, "iso": self.L.mort_add_isotropic}[kind]
        return {"lamb": S.MAT_LAMBERTIAN, "light": S.MAT_DIFFUSE_LIGHT, "iso": S.MAT_ISOTROPIC}[kind], Wd._ok(add(self.w.ptr, tt, ti), "material")

    def _solid(self, rgb):
        return Wd._ok(self.L.mort_add_solid_color(self.w.ptr, host.vec3(*rgb)), "mort_add_solid_color")

    def material(self, mat):
        key = repr(mat)
        if key not in self.seen:
            self.seen[key] = self._material(mat)
        return self.seen[key]

    def _material(self, mat):
        L, w, kind = self.L, self.w, mat[0]
        if kind in ("lamb", "light", "iso"):
            return self._textured(kind, S.TEXTURE_SOLID, self._solid(mat[1]))
        if kind == "checker":
            scales = mat[1] if isinstance(mat[1], tuple) else (mat[1],)
            bright = (4.0, 4.0, 4.0) if len(mat) > 2 and mat[2] == "light" else (.9, .9, .9)
            tt, ti = S.TEXTURE_SOLID, self._solid(bright)
            for s in reversed(scales):  # the last scale is the innermost checker
                tt, ti = S.TEXTURE_CHECKER, Wd._ok(L.mort_add_checker_texture(w.ptr, s, S.TEXTURE_SOLID, self._solid((.2, .3, .1)), tt, ti), "checker")
            return self._textured(mat[2] if len(mat) > 2 else "lamb", tt, ti)
        if kind == "noise":
            if self.noise is None:  # the reference's table holds one noise texture
                g = S.HostRng(); L.mort_host_rng_init(C.byref(g), 3, 0)
                self.noise = Wd._ok(L.mort_add_noise_texture(w.ptr, 4.0, C.byref(g)), "noise")
            return self._textured(mat[1] if len(mat) > 1 else "lamb", S.TEXTURE_NOISE, self.noise)
        if kind == "image":
            img = host.synthetic_earth(64, 32); w._keepalive.append(img)
            return self._textured(mat[1] if len(mat) > 1 else "lamb", S.TEXTURE_IMAGE, Wd._ok(L.mort_add_image_texture(w.ptr, img.ctypes.data, 64, 32), "image"))
        if kind == "metal":
            return S.MAT_METAL, Wd._ok(L.mort_add_metal(w.ptr, host.vec3(*mat[1]), mat[2]), "mort_add_metal")
        if kind == "glass":
            return S.MAT_DIELECTRIC, Wd._ok(L.mort_add_dielectric(w.ptr, mat[1]), "mort_add_dielectric")
        if kind == "tex":
            return S.MAT_LAMBERTIAN, Wd._ok(L.mort_add_lambertian(w.ptr, mat[1], mat[2]), "mort_add_lambertian")
        assert kind == "mat", mat
        return mat[1], mat[2]

    def sphere(self, sph, skip):
        mt, mi = self.material(sph[-1])
        if len(sph) == 4:
            return Wd._ok(self.L.mort_add_moving_sphere(self.w.ptr, host.vec3(*sph[0]), host.vec3(*sph[1]), sph[2], mt, mi, skip), "mort_add_moving_sphere")
        return Wd._ok(self.L.mort_add_sphere(self.w.ptr, host.vec3(*sph[0]), sph[1], mt, mi, skip), "mort_add_sphere")


def build(spheres, form, quads=(), media=()):
    """spheres: (centre, radius, material) or (centre at time 0, centre at time 1, radius, material).  form "flat": the spheres, then
    quads (Q, u, v, material) and media (centre, radius, density, material of the phase function) in the scan; form "bvh": one reference
    BVH over the spheres (no quads, no media)."""
    b = _Builder()
    if form == "bvh":
        assert not quads and not media
        lst = Wd._ok(b.L.mort_add_hittable_list(b.w.ptr, True), "mort_add_hittable_list")
        for s in spheres:
            assert b.L.mort_list_add(b.w.ptr, lst, S.OBJ_SPHERE, b.sphere(s, True)) == 0
        Wd._ok(b.L.mort_add_bvh(b.w.ptr, lst, False), "mort_add_bvh")
        b.w.c.bvh_mode = True
        return b.w
    for s in spheres:
        b.sphere(s, False)
    for Q, u, v, mat in quads:
        mt, mi = b.material(mat)
        Wd._ok(b.L.mort_add_quad(b.w.ptr, host.vec3(*Q), host.vec3(*u), host.vec3(*v), mt, mi, False), "mort_add_quad")
    for centre, radius, density, mat in media:
        boundary = Wd._ok(b.L.mort_add_sphere(b.w.ptr, host.vec3(*centre), radius, *b.material(("glass", 1.5)), True), "mort_add_sphere")
        mt, mi = b.material(mat)
        Wd._ok(b.L.mort_add_constant_medium(b.w.ptr, S.OBJ_SPHERE, boundary, density, mt, mi, False), "mort_add_constant_medium")
    b.w.c.bvh_mode = False
    return b.w


_GROUND = ((0, -100.5, -1), 100, ("checker", 0.32))
_BACK = ((0, 1.2, -4.5), 1.5, ("lamb", (.6, .5, .3)))


def _rows(mats, radii=(0.3, -0.3)):
    """one row of spheres per radius, a material per column, in front of the camera of Wd.flat_camera"""
    n = len(mats)
    return [((float(-0.35 * (n - 1) + 0.7 * k), -0.2 + 0.75 * j, -1.2 - 0.9 * j), r, m) for j, r in enumerate(radii) for k, m in enumerate(mats)]


def _tag_spheres(rows):
    """a metal sphere (metal 0; the ground's checker holds solid colours 0 and 1) and one sphere per row of TAG_ROWS"""
    return [_GROUND, ((0, 1.1, -2.2), 0.5, ("metal", (.9, .6, .3), 0.0))] + \
           [((float(-0.21 * (len(rows) - 1) + 0.42 * k), -0.3 + 0.45 * (k % 2), -0.8 - 0.5 * (k % 2)), 0.2, TAG_ROWS[r]) for k, r in enumerate(rows)]


_EVERY = [("lamb", (.7, .3, .3)), ("metal", (.8, .8, .6), 0.0), ("metal", (.6, .8, .8), 0.4), ("glass", 1.5), ("iso", (.3, .6, .9)),
          ("light", (3, 3, 3)), ("checker", 0.32), ("noise",), ("image",)]

# name -> dict(spheres, [quads, media: flat form only], [forms], [camera settings])
MATERIAL_WORLDS = {
    "ior_edges": dict(spheres=[_GROUND, _BACK] + _rows([("glass", i) for i in IORS])),
    "fuzz_edges": dict(spheres=[_GROUND, _BACK] + _rows([("metal", (.8, .7, .6), f) for f in FUZZES])),
    "albedo_edges": dict(spheres=[_GROUND, _BACK] + _rows([("lamb", a) for a in ALBEDOS] + [("metal", a, 0.2) for a in ALBEDOS])),
    "checker_scales": dict(spheres=[_GROUND, _BACK] + _rows([("checker", s) for s in CHECKER_SCALES])),
    # the camera off-centre inside a glass sphere of radius 2: rays reach its wall at up to asin(1.74 / 2) = 60 degrees, the critical
    # angle is asin(1 / 1.5) = 41.8 degrees.  Inside it a 1 / 1.5 sphere and a negative-radius bubble; outside the ground and a backdrop.
    "inside_glass": dict(spheres=[_GROUND, ((0, 0, 0), 2.0, ("glass", 1.5)), ((-0.3, 0.1, -0.5), 0.6, ("glass", 1 / 1.5)),
                                  ((0.6, -0.3, -0.7), -0.35, ("glass", 1.5)), ((0, 1.0, -5.0), 1.5, ("lamb", (.8, .3, .2))),
                                  ((-3.5, 0.5, -1.0), 1.0, ("metal", (.8, .8, .8), 0.1))],
                         view=dict(frm=(1.2, 0.6, 1.1), at=(0.0, 0.0, -1.0))),
    # a closed mirror (albedo 1, fuzz 0) around the camera: nothing leaves, a path ends on the light or at the bounce limit.  The mirror
    # inside is tinted: with every entry of the bounce stack equal to the identity, a level taken for an identity level by mistake
    # (ident_mask, mega_bvh.h) would change nothing but a zero's sign
    "mirror_hall": dict(spheres=[((0, 0.5, 0), 4.0, ("metal", (1, 1, 1), 0.0)), ((-0.9, 0, -1), 0.5, ("glass", 1.5)), ((0.9, 0, -1), 0.5, ("glass", 1 / 1.5)),
                                 ((0, 0.2, -2.2), 0.6, ("metal", (.95, .9, .85), 0.0)), ((0.2, 2.6, -0.5), 0.35, ("light", (5, 4, 3)))],
                        width=48, limits=(64, 50, 13)),
    "moving_mix": dict(spheres=[_GROUND, _BACK] + [((c[0], c[1], c[2]), (c[0] + 0.1, c[1] + 0.35, c[2] - 0.1), 0.3, m)
                                                   for (c, _, m) in _rows(_EVERY, radii=(0.3,))]),
    "unknown_tags": dict(spheres=_tag_spheres(sorted(TAG_ROWS))),
    "surface_isotropic_and_phase": dict(spheres=[_GROUND, ((-1.3, 0.0, -1.2), 0.5, ("iso", (.9, .4, .2))), ((1.9, 0.1, -2.0), 0.4, ("light", (4, 4, 4)))],
                                        quads=[((-0.6, -0.5, -2.6), (1.6, 0, 0), (0, 1.4, 0.3), ("iso", (.3, .7, .4)))],
                                        media=[((0.0, 0.0, -1.0), 0.45, 3.0, ("lamb", (.8, .8, .3))), ((1.1, 0.0, -1.0), 0.45, 3.0, ("metal", (.9, .7, .7), 0.3)),
                                               ((0.5, 0.8, -1.6), 0.4, 3.0, ("glass", 1.5)), ((-0.5, 0.8, -1.6), 0.4, 3.0, ("iso", (.5, .5, .9)))],
                                        forms=("flat",)),
    # emission is front-face only: a sphere of negative radius shows the camera its back face
    "textured_lights": dict(spheres=[_GROUND, _BACK] + _rows([("checker", 0.2, "light"), ("noise", "light"), ("image", "light"), ("checker", (0.4, 0.15), "light")])),
}


def forms(name):
    return MATERIAL_WORLDS[name].get("forms", ("flat", "bvh"))


def limits(name):
    return MATERIAL_WORLDS[name].get("limits", (12,))


KEYS = [(name, form, limit) for name in sorted(MATERIAL_WORLDS) for form in forms(name) for limit in limits(name)]


def key_id(key):
    return "-".join(str(k) for k in key)


def _camera(spec, limit):
    cam = Wd.flat_camera(spp=4, width=spec.get("width", 64), depth=limit)
    if "view" in spec:
        Wd.set_view(cam, spec["view"]["frm"], spec["view"]["at"])
    return cam


@functools.lru_cache(maxsize=None)
def material_world(name, form):
    spec = MATERIAL_WORLDS[name]
    if form == "bvh":
        return build(spec["spheres"], "bvh")
    return build(spec["spheres"], "flat", spec.get("quads", ()), spec.get("media", ()))


def camera(name, limit):
    return _camera(MATERIAL_WORLDS[name], limit)


@functools.lru_cache(maxsize=None)
def tag_row_world(row, form):
    """the ground, the metal sphere and ONE sphere that carries the row's tag"""
    return build(_tag_spheres([row]), form)


def _frozen(ref):
    for a in (ref["rgba"], ref["accum"], ref["segments_px"]):
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def frame_reference(key):
    name, form, limit = key
    return _frozen(O.render(material_world(name, form), camera(name, limit), nthreads=8))


@functools.lru_cache(maxsize=None)
def tag_row_reference(row, form):
    return _frozen(O.render(tag_row_world(row, form), _camera({}, 12), nthreads=8))


def primary_rays(cam):
    """(W * H, 8) rays of hip.RAY_DTYPE's layout: sample (0, 0) of every pixel as get_ray draws it from the streams of seed 7"""
    W, H = cam.image_width, cam.image_height
    L = O.lib()
    gen = O.seed_states(7, W, H)
    rays = np.zeros((W * H, 8), F)
    r7, st = (C.c_float * 7)(), S.RngState()
    for i in range(W * H):
        st.d = int(gen["d"][i])
        for k in range(5):
            st.v[k] = int(gen["v"][i][k])
        L.mort_oracle_get_ray(C.byref(cam), i % W, i // W, 0, 0, C.byref(st), r7)
        rays[i, :7] = list(r7)
    rays[:, 7] = np.inf
    return rays


class RayRef:
    """rays (n, 8), streams0 / streams, rgb (n, 3): the oracle's ray_color along the frame's own primary rays"""


@functools.lru_cache(maxsize=None)
def radiance_reference(key):
    from tests import query_rays as Q
    from tests import radiance_ref as R
    name, form, limit = key
    w, cam = material_world(name, form), camera(name, limit)
    r = RayRef()
    r.rays = primary_rays(cam)
    r.params = hip.radiance_params_from_camera(cam, 1)
    r.streams0 = Q.some_streams(len(r.rays))
    r.streams = r.streams0.copy()
    r.rgb = R.oracle_radiance(w, cam, r.rays, r.streams, 1)
    for a in (r.rays, r.streams0, r.streams, r.rgb):
        a.setflags(write=False)
    return r


PROBE_D = 64


@functools.lru_cache(maxsize=None)
def probe_reference(key):
    """one SH9 probe at the camera's own position (inside the glass sphere, inside the hall), 64 directions, one path each"""
    from tests import probe_ref as P
    from tests import query_rays as Q
    from tests import radiance_ref as R
    name, form, limit = key
    w, cam = material_world(name, form), camera(name, limit)
    r = P.Ref()
    r.world, r.cam = w, cam
    r.params = hip.probe_params_from_camera(cam, PROBE_D, 1)
    r.probes = np.zeros(1, dtype=hip.PROBE_DTYPE)
    r.probes["position"] = tuple(cam.center.e[k] for k in range(3))
    r.probes["time"] = 0.5
    r.dirs = P.fibonacci(PROBE_D)
    r.streams0 = Q.some_streams(PROBE_D)
    r.streams = r.streams0.copy()
    r.s = R.oracle_radiance(w, cam, P.rays_of(r.probes, r.dirs), r.streams, 1).reshape(1, PROBE_D, 3)
    r.sh = P.project(r.s, r.dirs, 1)
    for a in (r.probes, r.dirs, r.streams0, r.streams, r.s, r.sh):
        a.setflags(write=False)
    return r


def total_internal_reflections(key):
    """how many of the frame's own primary rays end on a dielectric from its back face beyond the critical angle, by a margin no rounding
    of the fp32 shade step can cross (ior x sin(theta) >= 1.01, in float64 from the oracle's own hit records)"""
    name, form, limit = key
    w, cam = material_world(name, form), camera(name, limit)
    rays = primary_rays(cam)
    rec, hit = O.world_hit_batch(w, rays[:, :7], 0.001, np.inf)
    d = rays[:, 3:6].astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    cos = np.minimum(-(d * rec["normal"].astype(np.float64)).sum(1), 1.0)
    sin = np.sqrt(np.maximum(0.0, 1.0 - cos * cos))
    iors = np.array([w.c.mats.host_dielectric[int(i)].ior if t == S.MAT_DIELECTRIC else 0.0 for t, i in zip(rec["mat_type"], rec["mat_idx"])])
    return int((hit & (rec["mat_type"] == S.MAT_DIELECTRIC) & (rec["front_face"] == 0) & (iors * sin >= 1.01)).sum())


def assert_frame_same(out, ref, what):
    """light_cases.assert_frame_same -- image, accumulators, per-pixel segment counts, totals, final RNG words -- with the accumulators
    compared as raw words, a NaN's sign and payload included: a frame zeroes a NaN pixel sum, so the oracle's accumulators hold none"""
    from tests import light_cases as LC
    assert not np.isnan(ref["accum"]).any()
    assert (np.asarray(out["accum"]).view(np.uint32) == ref["accum"].view(np.uint32)).all(), f"{what}: fp32 accumulators differ (raw words)"
    LC.assert_frame_same(out, ref, what)
