"""Hand-built brute-force worlds (no reference BVH) shared by the GPU parity tests (tests/test_gpu_gen.py) and the
CPU tests of the host loop (tests/test_host_mode.py): the awkward cases the built-in scenes do not contain."""
import ctypes as C

import numpy as np

from mort_amd import host, structs as S


def set_view(cam, frm, at, vfov=None, defocus=None):
    for i in range(3):
        cam.lookfrom.e[i] = frm[i]; cam.lookat.e[i] = at[i]
    if vfov is not None:
        cam.vfov = vfov
    if defocus is not None:
        cam.defocus_angle = defocus
    host.lib().mort_camera_initialize(C.byref(cam))


def flat_world(prims, media=(), light=None, late_list=False):
    """A brute-force world (no BVH).  prims: ("sphere", centre, radius, mat) | ("msphere", c1, c2, radius, mat) |
    ("quad", Q, u, v, mat) | ("box", a, b, mat) | ("rbox", size, translation, theta, mat); mat as in
    test_gpu_parity._custom_bvh_world.  media: (centre, radius, density, rgb).  Returns (world, ids of the prims)."""
    L = host.lib()
    w = host.World()

    def material(mat):
        kind = mat[0]
        if kind in ("lamb", "light", "iso"):
            col = L.mort_add_solid_color(w.ptr, host.vec3(*mat[1]))
            add = {"lamb": L.mort_add_lambertian, "light": L.mort_add_diffuse_light, "iso": L.mort_add_isotropic}[kind]
            return {"lamb": S.MAT_LAMBERTIAN, "light": S.MAT_DIFFUSE_LIGHT, "iso": S.MAT_ISOTROPIC}[kind], add(w.ptr, S.TEXTURE_SOLID, col)
        if kind == "checker":
            c1 = L.mort_add_solid_color(w.ptr, host.vec3(.2, .3, .1)); c2 = L.mort_add_solid_color(w.ptr, host.vec3(.9, .9, .9))
            return S.MAT_LAMBERTIAN, L.mort_add_lambertian(w.ptr, S.TEXTURE_CHECKER, L.mort_add_checker_texture(w.ptr, 0.32, S.TEXTURE_SOLID, c1, S.TEXTURE_SOLID, c2))
        if kind == "noise":
            g = S.HostRng(); L.mort_host_rng_init(C.byref(g), 3, 0)
            return S.MAT_LAMBERTIAN, L.mort_add_lambertian(w.ptr, S.TEXTURE_NOISE, L.mort_add_noise_texture(w.ptr, 4.0, C.byref(g)))
        if kind == "image":
            img = host.synthetic_earth(64, 32); w._keepalive.append(img)
            return S.MAT_LAMBERTIAN, L.mort_add_lambertian(w.ptr, S.TEXTURE_IMAGE, L.mort_add_image_texture(w.ptr, img.ctypes.data, 64, 32))
        if kind == "metal":
            return S.MAT_METAL, L.mort_add_metal(w.ptr, host.vec3(*mat[1]), mat[2])
        return S.MAT_DIELECTRIC, L.mort_add_dielectric(w.ptr, mat[1])

    ids = []
    for p in prims:
        mt, mi = material(p[-1])
        if p[0] == "sphere":
            ids.append((S.OBJ_SPHERE, L.mort_add_sphere(w.ptr, host.vec3(*p[1]), p[2], mt, mi, False)))
        elif p[0] == "msphere":
            ids.append((S.OBJ_SPHERE, L.mort_add_moving_sphere(w.ptr, host.vec3(*p[1]), host.vec3(*p[2]), p[3], mt, mi, False)))
        elif p[0] == "quad":
            ids.append((S.OBJ_QUAD, L.mort_add_quad(w.ptr, host.vec3(*p[1]), host.vec3(*p[2]), host.vec3(*p[3]), mt, mi, False)))
        elif p[0] == "box":
            L.mort_box(w.ptr, host.vec3(*p[1]), host.vec3(*p[2]), mt, mi); ids.append(None)
        else:
            L.mort_rotated_box(w.ptr, host.vec3(*p[1]), host.vec3(*p[2]), p[3], mt, mi); ids.append(None)
    for centre, radius, density, rgb in media:
        b = L.mort_add_sphere(w.ptr, host.vec3(*centre), radius, S.MAT_DIELECTRIC, L.mort_add_dielectric(w.ptr, 1.5), True)
        col = L.mort_add_solid_color(w.ptr, host.vec3(*rgb))
        L.mort_add_constant_medium(w.ptr, S.OBJ_SPHERE, b, density, S.MAT_ISOTROPIC, L.mort_add_isotropic(w.ptr, S.TEXTURE_SOLID, col), False)
    if late_list:  # a non-skip list is scanned AFTER the media (world.cuh:154-168): order matters, no unified tree
        lst = L.mort_add_hittable_list(w.ptr, False)
        mt, mi = material(("lamb", (.4, .4, .9)))
        L.mort_list_add(w.ptr, lst, S.OBJ_SPHERE, L.mort_add_sphere(w.ptr, host.vec3(0.2, 0.1, -1.2), 0.35, mt, mi, True))
    w.c.bvh_mode = False
    return w, ids


def flat_camera(light=None, spp=9, width=144, depth=12):
    _, cam = host.build_scene(2, width=width, spp=spp, depth=depth)
    cam.background.e[0], cam.background.e[1], cam.background.e[2] = 0.30, 0.35, 0.45
    if light is not None:
        cam.light_obj_type, cam.light_obj_idx = light
    set_view(cam, (0.0, 0.8, 2.5), (0.0, 0.0, -1.0), vfov=55, defocus=0.0)
    return cam


GROUND = ("sphere", (0, -100.5, -1), 100, ("checker",))
FLAT_WORLDS = {
    "empty": dict(prims=[]),
    "single_sphere": dict(prims=[("sphere", (0, 0, -1), 0.5, ("lamb", (.7, .3, .3)))]),
    "single_quad": dict(prims=[("quad", (-1, -0.5, -1.5), (2, 0, 0), (0, 1.5, 0.3), ("metal", (.8, .8, .8), 0.05))]),
    # equal t everywhere: the same sphere / quad several times, a quad lying in another one's plane -> the scan decides
    "coincident": dict(prims=[GROUND] + [("sphere", (0, 0, -1), 0.5, ("lamb", (.1 * k, .2, .5))) for k in range(4)] +
                       [("quad", (-2, -0.5, -2), (4, 0, 0), (0, 2, 0), ("lamb", (.2 * k, .5, .2))) for k in range(3)] +
                       [("quad", (-1, 0, -2), (1, 0, 0), (0, 1, 0), ("metal", (.9, .9, .2), 0.0))]),
    "concentric_glass": dict(prims=[GROUND, ("sphere", (0, 0, -1), 0.5, ("glass", 1.5)), ("sphere", (0, 0, -1), 0.4, ("glass", 1 / 1.5)),
                                    ("sphere", (0, 0, -1), 0.2, ("glass", 1.5)), ("msphere", (-1.2, 0, -1), (-1.2, 0.4, -1), 0.4, ("lamb", (.8, .8, 0))),
                                    ("sphere", (1.2, 0, -1), 0.5, ("metal", (.8, .6, .2), 1.0))]),
    "boxes_and_instances": dict(prims=[GROUND, ("box", (-1.5, -0.5, -2.0), (-0.7, 0.4, -1.2), ("lamb", (.7, .2, .2))),
                                       ("rbox", (0.8, 1.2, 0.8), (0.2, -0.5, -2.2), 25.0, ("metal", (.7, .7, .7), 0.1)),
                                       ("rbox", (0.5, 0.5, 0.5), (-0.3, -0.5, -0.8), -40.0, ("glass", 1.5))]),
    # isotropic and emissive spheres UNDER A LIGHT OBJECT (mixture pdf + sphere_pdf, pdf.cuh:29-37,91-103)
    "every_material_lit_by_sphere": dict(prims=[GROUND] + [("sphere", (-3 + 1.0 * k, 0.0, -1.5 - 0.2 * k), 0.45, m) for k, m in enumerate(
        [("lamb", (.7, .3, .3)), ("noise",), ("image",), ("metal", (.7, .6, .5), 0.2), ("glass", 1.5), ("light", (6, 6, 6)), ("iso", (.3, .6, .9))])],
        light=("prim", 6)),  # the emissive sphere (world sphere index 6) is the light object
    "lit_by_quad_with_media": dict(prims=[GROUND, ("quad", (-1, 2.2, -2), (2, 0, 0), (0, 0, 2), ("light", (9, 9, 9))),
                                          ("sphere", (-0.9, 0, -1), 0.5, ("iso", (.9, .4, .2))), ("sphere", (0.9, 0, -1), 0.5, ("lamb", (.2, .4, .9)))],
                                   media=[((0, 0.2, -1), 0.6, 1.5, (.9, .9, .9)), ((0, 0, 0), 30.0, 0.02, (1, 1, 1))], light=("prim", 1)),
    "media_then_list": dict(prims=[GROUND, ("sphere", (-0.9, 0, -1), 0.5, ("lamb", (.9, .4, .2)))],
                            media=[((0, 0.2, -1), 0.7, 2.0, (.9, .9, .9))], late_list=True),
}


def random_world(rng, n_spheres, n_quads, n_boxes, n_media, with_light):
    """A random brute-force world: spheres (some moving, some huge, some tiny), quads, rotated / translated boxes, media in
    sphere boundaries; every material kind.  Returns (world, light (type, idx) or None)."""
    L = host.lib()
    w = host.World()

    palette = []

    def material():
        # the reference's tables are small (20 isotropics, 50 dielectrics, ...): draw from a palette of at most 16
        if len(palette) >= 16:
            return palette[int(rng.integers(0, len(palette)))]
        m = new_material()
        palette.append(m)
        return m

    def new_material():
        k = rng.integers(0, 6)
        col = tuple(rng.uniform(0.1, 0.95, 3))
        if k == 0:
            return S.MAT_METAL, L.mort_add_metal(w.ptr, host.vec3(*col), float(rng.uniform(0, 1)))
        if k == 1:
            return S.MAT_DIELECTRIC, L.mort_add_dielectric(w.ptr, float(rng.uniform(1.1, 2.0)))
        if k == 2:
            c = L.mort_add_solid_color(w.ptr, host.vec3(*col))
            return S.MAT_ISOTROPIC, L.mort_add_isotropic(w.ptr, S.TEXTURE_SOLID, c)
        if k == 3:
            c1 = L.mort_add_solid_color(w.ptr, host.vec3(*col)); c2 = L.mort_add_solid_color(w.ptr, host.vec3(.9, .9, .9))
            ck = L.mort_add_checker_texture(w.ptr, float(rng.uniform(0.2, 2.0)), S.TEXTURE_SOLID, c1, S.TEXTURE_SOLID, c2)
            return S.MAT_LAMBERTIAN, L.mort_add_lambertian(w.ptr, S.TEXTURE_CHECKER, ck)
        c = L.mort_add_solid_color(w.ptr, host.vec3(*col))
        return S.MAT_LAMBERTIAN, L.mort_add_lambertian(w.ptr, S.TEXTURE_SOLID, c)

    light = None
    if with_light:
        c = L.mort_add_solid_color(w.ptr, host.vec3(7, 7, 7))
        lm = L.mort_add_diffuse_light(w.ptr, S.TEXTURE_SOLID, c)
        q = L.mort_add_quad(w.ptr, host.vec3(-2, 6, -2), host.vec3(4, 0, 0), host.vec3(0, 0, 4), S.MAT_DIFFUSE_LIGHT, lm, False)
        light = (S.OBJ_QUAD, q)
    mt, mi = material()
    L.mort_add_sphere(w.ptr, host.vec3(0, -1000, 0), 1000.0, mt, mi, False)  # ground: a huge sphere among small ones
    for _ in range(n_spheres):
        mt, mi = material()
        c = rng.uniform(-6, 6, 3) * (1, 0.3, 1) + (0, 1.2, 0)
        r = float(rng.choice([0.05, 0.2, 0.5, 1.0, 1.5]))
        if rng.random() < 0.3:
            L.mort_add_moving_sphere(w.ptr, host.vec3(*c), host.vec3(*(c + rng.uniform(-0.5, 0.5, 3))), r, mt, mi, False)
        else:
            L.mort_add_sphere(w.ptr, host.vec3(*c), r, mt, mi, False)
    for _ in range(n_quads):
        mt, mi = material()
        L.mort_add_quad(w.ptr, host.vec3(*rng.uniform(-5, 5, 3)), host.vec3(*rng.uniform(-2, 2, 3)), host.vec3(*rng.uniform(-2, 2, 3)), mt, mi, False)
    for _ in range(n_boxes):
        mt, mi = material()
        L.mort_rotated_box(w.ptr, host.vec3(*rng.uniform(0.3, 2.0, 3)), host.vec3(*(rng.uniform(-5, 5, 3) * (1, 0, 1))), float(rng.uniform(-60, 60)), mt, mi)
    for _ in range(n_media):
        b = L.mort_add_sphere(w.ptr, host.vec3(*(rng.uniform(-4, 4, 3) * (1, 0.2, 1) + (0, 1, 0))), float(rng.uniform(0.5, 2.5)), S.MAT_DIELECTRIC, L.mort_add_dielectric(w.ptr, 1.5), True)
        c = L.mort_add_solid_color(w.ptr, host.vec3(*rng.uniform(0.2, 1.0, 3)))
        L.mort_add_constant_medium(w.ptr, S.OBJ_SPHERE, b, float(rng.uniform(0.05, 3.0)), S.MAT_ISOTROPIC, L.mort_add_isotropic(w.ptr, S.TEXTURE_SOLID, c), False)
    w.c.bvh_mode = False
    return w, light


def custom_bvh_world(spheres, noise_seed=1):
    """A world that is one BVH over the given spheres: (centre, radius, material) with material one of
    ("lamb", rgb) ("checker",) ("noise",) ("image",) ("metal", rgb, fuzz) ("glass", ior) ("light", rgb) ("iso", rgb)."""
    import ctypes as C
    L = host.lib()
    w = host.World()
    lst = L.mort_add_hittable_list(w.ptr, True)
    LAMB, METAL, DIEL, LIGHT, ISO = S.MAT_LAMBERTIAN, S.MAT_METAL, S.MAT_DIELECTRIC, S.MAT_DIFFUSE_LIGHT, S.MAT_ISOTROPIC
    for centre, radius, mat in spheres:
        kind = mat[0]
        if kind in ("lamb", "light", "iso"):
            col = L.mort_add_solid_color(w.ptr, host.vec3(*mat[1]))
            add = {"lamb": L.mort_add_lambertian, "light": L.mort_add_diffuse_light, "iso": L.mort_add_isotropic}[kind]
            mt, mi = {"lamb": LAMB, "light": LIGHT, "iso": ISO}[kind], add(w.ptr, S.TEXTURE_SOLID, col)
        elif kind == "checker":
            c1 = L.mort_add_solid_color(w.ptr, host.vec3(.2, .3, .1)); c2 = L.mort_add_solid_color(w.ptr, host.vec3(.9, .9, .9))
            ck = L.mort_add_checker_texture(w.ptr, 0.32, S.TEXTURE_SOLID, c1, S.TEXTURE_SOLID, c2)
            mt, mi = LAMB, L.mort_add_lambertian(w.ptr, S.TEXTURE_CHECKER, ck)
        elif kind == "noise":
            g = S.HostRng(); L.mort_host_rng_init(C.byref(g), noise_seed, 0)
            nz = L.mort_add_noise_texture(w.ptr, 4.0, C.byref(g))
            mt, mi = LAMB, L.mort_add_lambertian(w.ptr, S.TEXTURE_NOISE, nz)
        elif kind == "image":
            img = host.synthetic_earth(64, 32); w._keepalive.append(img)
            im = L.mort_add_image_texture(w.ptr, img.ctypes.data, 64, 32)
            mt, mi = LAMB, L.mort_add_lambertian(w.ptr, S.TEXTURE_IMAGE, im)
        elif kind == "metal":
            mt, mi = METAL, L.mort_add_metal(w.ptr, host.vec3(*mat[1]), mat[2])
        else:
            mt, mi = DIEL, L.mort_add_dielectric(w.ptr, mat[1])
        L.mort_list_add(w.ptr, lst, S.OBJ_SPHERE, L.mort_add_sphere(w.ptr, host.vec3(*centre), radius, mt, mi, True))
    L.mort_add_bvh(w.ptr, lst, False)
    w.c.bvh_mode = True
    return w



_BVH_GROUND = ((0, -100.5, -1), 100, ("checker",))
BVH_WORLDS = {
    "one": [((0, 0, -1), 0.5, ("lamb", (.7, .3, .3)))],
    "two": [_BVH_GROUND, ((0, 0, -1), 0.5, ("glass", 1.5))],
    "three": [_BVH_GROUND, ((0, 0, -1), 0.5, ("lamb", (.1, .2, .5))), ((1, 0, -1), 0.5, ("metal", (.8, .6, .2), 0.3))],
    "coincident": [_BVH_GROUND] + [((0, 0, -1), 0.5, ("lamb", (.1 * k, .2, .5))) for k in range(5)] + [((0.3, 0, -1), 0.5, ("metal", (.8, .8, .8), 0.0))] * 3,
    "concentric_glass": [_BVH_GROUND, ((0, 0, -1), 0.5, ("glass", 1.5)), ((0, 0, -1), 0.4, ("glass", 1.0 / 1.5)), ((0, 0, -1), 0.2, ("glass", 1.5)),
                         ((-1.1, 0, -1), 0.5, ("lamb", (.8, .8, 0))), ((1.1, 0, -1), 0.5, ("metal", (.8, .6, .2), 1.0))],
    "every_material": [_BVH_GROUND] + [((-3 + 1.0 * k, 0.0, -1.5 - 0.2 * k), 0.45, m) for k, m in enumerate(
        [("lamb", (.7, .3, .3)), ("noise",), ("image",), ("metal", (.7, .6, .5), 0.2), ("glass", 1.5), ("light", (4, 4, 4)), ("iso", (.3, .6, .9))])],
}


# ---- pre-build worlds for the BVH builder (tests/test_reference_pin.py, tests/golden/make_golden.py) ----

def _raw(ptr, n, T):
    return C.string_at(C.cast(ptr, C.c_void_p).value, n * C.sizeof(T)) if n else b""


def world_object_bytes(w):
    """sphere / quad / translate / rotate_y / medium arrays and every BVH, byte for byte (the lists are left out: the
    reference's scenes sort a local copy, mort_add_bvh the world's own)"""
    o = w.c.objs
    return b"".join([_raw(o.host_sphere, o.num_spheres, S.Sphere), _raw(o.host_quad, o.num_quads, S.Quad),
                     _raw(o.host_translate, o.num_translates, S.Translate), _raw(o.host_rotate_y, o.num_rotate_y, S.RotateY),
                     _raw(o.host_constant_medium, o.num_constant_medium, S.ConstantMedium), _raw(o.host_bvh, o.num_bvh, S.Bvh),
                     bytes([o.num_bvh, int(w.c.bvh_mode)])])


def _list_world(items):
    """a pre-build world: one skip list over `items` = ("s", centre, radius) | ("q", Q, u, v) | ("t", item, offset) |
    ("r", item, degrees) | ("b", size, translation, degrees) (a rotated box: list -> rotate_y -> translate)"""
    L = host.lib()
    w = host.World()
    m = L.mort_add_lambertian(w.ptr, S.TEXTURE_SOLID, L.mort_add_solid_color(w.ptr, host.vec3(.5, .5, .5)))
    lam = S.MAT_LAMBERTIAN

    def add(it):
        if it[0] == "s":
            return S.OBJ_SPHERE, L.mort_add_sphere(w.ptr, host.vec3(*it[1]), it[2], lam, m, True)
        if it[0] == "q":
            return S.OBJ_QUAD, L.mort_add_quad(w.ptr, host.vec3(*it[1]), host.vec3(*it[2]), host.vec3(*it[3]), lam, m, True)
        if it[0] == "t":
            t, i = add(it[1])
            return S.OBJ_TRANSLATE, L.mort_add_translate(w.ptr, t, i, host.vec3(*it[2]), True)
        t, i = add(it[1])
        return S.OBJ_ROTATE_Y, L.mort_add_rotate_y(w.ptr, t, i, it[2], True)
    refs = [add(it) for it in items]
    assert all(i >= 0 for _, i in refs), "more objects than the reference's arrays hold"
    li = L.mort_add_hittable_list(w.ptr, True)
    for t, i in refs:
        assert L.mort_list_add(w.ptr, li, t, i) == 0
    return w, li


def _scene_list_world(sid, order):
    """scene `sid`'s objects in a new list order (`order` maps the permutation of its list entries)"""
    src, _ = host.build_scene(sid, width=16, spp=1)
    w = host.World()
    so, wo = src.c.objs, w.c.objs
    C.memmove(wo.host_sphere, so.host_sphere, so.num_spheres * C.sizeof(S.Sphere)); wo.num_spheres = so.num_spheres
    C.memmove(wo.host_quad, so.host_quad, so.num_quads * C.sizeof(S.Quad)); wo.num_quads = so.num_quads
    lst = so.host_hittable_list[0]
    entries = [(lst.obj_types[i], lst.obj_idxs[i]) for i in range(lst.num_objs)]
    li = host.lib().mort_add_hittable_list(w.ptr, True)
    for t, i in order(entries):
        host.lib().mort_list_add(w.ptr, li, t, i)
    return w, li


def _random_list(seed, n):
    rng = np.random.default_rng(seed)
    items = []
    for _ in range(n):
        k = rng.random()
        c = tuple(np.round(rng.uniform(-20, 20, 3), int(rng.integers(0, 3))))  # rounded: equal minima are common
        if k < 0.55:
            items.append(("s", c, float(rng.choice([0.2, 0.5, 1.0, 2.0]))))
        elif k < 0.8:
            items.append(("q", c, tuple(rng.uniform(-3, 3, 3)), tuple(rng.uniform(-3, 3, 3))))
        elif k < 0.9 and sum(it[0] == "t" for it in items) < 40:  # 50 translates / rotate_ys at most (objects.cuh)
            items.append(("t", ("s", c, 0.5), tuple(rng.uniform(-5, 5, 3))))
        elif sum(it[0] == "r" for it in items) < 40:
            items.append(("r", ("q", c, (1.0, 0, 0), (0, 1.0, 0)), float(rng.uniform(-90, 90))))
        else:
            items.append(("s", c, 0.75))
    return items


BVH_BUILDS = {
    "one_sphere": lambda: _list_world([("s", (0, 0, 0), 1.0)]),
    "two_spheres": lambda: _list_world([("s", (1, 0, 0), 1.0), ("s", (-1, 0, 0), 0.5)]),
    "two_spheres_tie": lambda: _list_world([("s", (0, 0, 0), 1.0), ("s", (0.5, 3, 0), 1.5)]),  # equal x minima
    "two_mixed_tie": lambda: _list_world([("q", (-1, 0, 0), (0, 1, 0), (0, 0, 1)), ("s", (0, 5, 0), 1.0)]),
    "three_spheres": lambda: _list_world([("s", (2, 0, 0), 0.5), ("s", (0, 0, 0), 0.5), ("s", (1, 0, 0), 0.5)]),
    "three_ties": lambda: _list_world([("s", (0, 0, 0), 1.0)] * 3),
    "equal_minima": lambda: _list_world([("s", (float(k % 3), float(k), 0), 1.0 + (k % 3)) for k in range(12)]),
    "mixed_instances": lambda: _list_world([("q", (3, 0, 0), (1, 0, 0), (0, 1, 0)), ("s", (1, 0, 0), 0.5),
                                            ("t", ("s", (0, 0, 0), 0.5), (-2, 0, 0)), ("r", ("q", (0, 0, 0), (1, 0, 0), (0, 1, 0)), 30.0),
                                            ("s", (-3, 0, 0), 0.5), ("q", (2, 1, 0), (1, 0, 0), (0, 0, 1)), ("s", (2, 0, 0), 0.25),
                                            ("t", ("q", (0, 0, 0), (0, 1, 0), (0, 0, 1)), (5, 0, 0))]),
    "scene1_reversed": lambda: _scene_list_world(1, lambda e: e[::-1]),
    "scene1_shuffled": lambda: _scene_list_world(1, lambda e: [e[i] for i in np.random.default_rng(1).permutation(len(e))]),
    "scene10_shuffled": lambda: _scene_list_world(10, lambda e: [e[i] for i in np.random.default_rng(10).permutation(len(e))]),
    **{f"random{n}": (lambda n=n: _list_world(_random_list(n, n))) for n in (4, 5, 17, 64, 200, 480)},
}


# ---- cameras shared by the feature tests (tests/test_features_oracle.py, tests/test_gpu_denoise.py) ----

def bvh_camera(width=144, spp=9):
    """the camera test_small_and_awkward_bvh_worlds (tests/test_gpu_parity.py) puts in front of the BVH_WORLDS"""
    _, cam = host.build_scene(1, width=width, spp=spp, depth=12)
    set_view(cam, (0.0, 0.6, 1.5), (0.0, 0.0, -1.0), vfov=60, defocus=0.0)
    return cam


def bvh_scene_views(sid):
    """test_other_viewpoints' list (tests/test_gpu_parity.py) for the reference-BVH scenes 1 and 10: (lookfrom, lookat, vfov,
    defocus) inside the sphere field, at and under the ground, straight up / down / along an axis, far out, 4 random ones"""
    rng = np.random.default_rng(7 + sid)
    views = [((0.5, 0.3, 0.5), (3.0, 0.3, 0.2)), ((0.0, 0.21, 2.0), (0.0, 0.21, -5.0)), ((2.0, -3.0, 1.0), (0.0, 1.0, 0.0)),
             ((0.0, 30.0, 0.0), (0.0, 0.0, 0.001)), ((0.0, 0.5, 0.0), (0.0, 10.0, 0.0001)), ((5.0, 1.0, 0.0), (-5.0, 1.0, 0.0)),
             ((300.0, 120.0, 200.0), (0.0, 0.0, 0.0)), ((0.0, 1.0, 0.0), (4.0, 1.0, 0.0))]
    views += [(tuple(rng.uniform(-9, 9, 3) * (1, 0.2, 1) + (0, 0.5, 0)), tuple(rng.uniform(-6, 6, 3) * (1, 0.1, 1))) for _ in range(4)]
    return [(frm, at, 20 if k % 3 else 70, 0.0 if k % 2 else 0.6) for k, (frm, at) in enumerate(views)]


def gen_scene_views(sid):
    """test_gen_other_viewpoints' list (tests/test_gpu_gen.py) for scenes 6, 7, 9: inside the box / the cluster, at floor
    level, along an axis, from outside, from beyond the unified tree's reach (the fifth), 4 random ones"""
    rng = np.random.default_rng(11 + sid)
    views = [((278, 278, 100), (278, 278, 555)), ((278, 1.0, 278), (300, 1.0, 0)), ((100, 300, 100), (100, 0, 100.001)),
             ((278, 278, -800), (278, 278, 0)), ((-3e5, 4e5, -9e5), (278, 278, 0)), ((130, 60, 200), (400, 200, 300))]
    views += [(tuple(rng.uniform(0, 555, 3)), tuple(rng.uniform(0, 555, 3))) for _ in range(4)]
    return [(frm, at, 40 if k % 3 else 80, 0.0 if k % 2 else 0.5) for k, (frm, at) in enumerate(views)]


GEN_FAR_VIEW = 4  # index into gen_scene_views: the camera beyond the tree's reach


def _placed_flat(prims, media, frm, at, vfov=55, width=96):
    w, _ = flat_world(prims, media=media)
    cam = flat_camera(spp=1, width=width)
    set_view(cam, frm, at, vfov=vfov, defocus=0.0)
    return w, cam


def _placed_scene(sid, frm, at, vfov, width=96):
    w, cam = host.build_scene(sid, width=width, spp=1)
    set_view(cam, frm, at, vfov=vfov, defocus=0.0)
    return w, cam


_BACK = ("sphere", (0, 0, -4), 1.5, ("checker",))
_MED = ((0, 0, -1), 0.5, 1.0, (.9, .4, .2))
# Cameras placed on purpose.  name -> () -> (world, camera); tests/test_features_oracle.py states what each must show.
PLACED = {
    # every ray starts inside the medium: it is no first hit, the checkered sphere behind it is
    "inside_small_medium": lambda: _placed_flat([_BACK], [_MED], (0.1, 0.05, -0.9), (0, 0, -4)),
    # the final scene's fog shell (radius 5000) holds the camera: the sphere cluster under rotate_y / translate ...
    "fog_cluster": lambda: _placed_scene(8, (100, 350, 0), (-20, 350, 480), 50),
    # ... and the moving sphere at time 0.5
    "fog_moving_sphere": lambda: _placed_scene(8, (400, 400, -150), (415, 400, 200), 40),
    # a solid in front of, inside and behind a medium along the centre ray
    "solid_before_medium": lambda: _placed_flat([("sphere", (0, 0, 0.5), 0.15, ("lamb", (.1, .2, .3)))], [_MED], (0, 0, 3), (0, 0, -1), vfov=30),
    "solid_inside_medium": lambda: _placed_flat([("sphere", (0, 0, -1), 0.2, ("lamb", (.1, .2, .3)))], [_MED], (0, 0, 3), (0, 0, -1), vfov=30),
    "solid_behind_medium": lambda: _placed_flat([("sphere", (0, 0, -3), 1.5, ("lamb", (.1, .2, .3)))], [_MED], (0, 0, 3), (0, 0, -1), vfov=30),
    # a medium seen from so far away that fp32 leaves some silhouette rays a chord below constant_medium::hit's 0.0001 step
    "grazed_medium": lambda: _placed_flat([], [((0, 0, 0), 100.0, 0.02, (1, 1, 1))], (3000, 1000, 7000), (0, 0, 0), vfov=2, width=160),
    "quad_from_behind": lambda: _placed_flat([("quad", (-1, -0.5, -1.5), (2, 0, 0), (0, 1.5, 0.3), ("lamb", (.2, .5, .8)))], [], (0.3, 0.4, -5), (0, 0, -1.5)),
    "inside_glass_sphere": lambda: _placed_flat(FLAT_WORLDS["concentric_glass"]["prims"], [], (0.05, 0.02, -1.0), (3, 0.5, -1)),
    # the lens centre lies on the sphere (0, 0, -1) r 0.5: the root at t = 0 is below t_min, rays into the ball leave by its far side
    "camera_on_surface": lambda: _placed_flat([("sphere", (0, 0, -1), 0.5, ("lamb", (.7, .3, .3)))], [], (0, 0, -0.5), (1, 0, -0.5), vfov=90),
}


# ---- random worlds that are one reference BVH over spheres (tests/test_bvh_random_host.py, tests/test_gpu_bvh_random.py) ----
# The BVH megakernel and wave_bvh.h walk a tree of this build's own over the reference's leaf nodes (scene_compile.h): these
# families give that builder tree shapes the built-in scenes do not have.

def _ok(v, what):
    if v < 0:
        raise RuntimeError(f"{what} failed: a table of the reference's capacities is full")
    return v


def _bvh_palette(w, rng, extras):
    """the materials every sphere of a random BVH world draws from: 12 solid Lambertians, metals of fuzz 0 / 0.3 / 1, glass
    1.5 and 1 / 1.5 (the last two entries); extras: a checker and a noise Lambertian as well"""
    L = host.lib()
    pal = []
    for _ in range(12):
        col = _ok(L.mort_add_solid_color(w.ptr, host.vec3(*rng.uniform(0.1, 0.95, 3))), "mort_add_solid_color")
        pal.append((S.MAT_LAMBERTIAN, _ok(L.mort_add_lambertian(w.ptr, S.TEXTURE_SOLID, col), "mort_add_lambertian")))
    if extras:
        c1 = _ok(L.mort_add_solid_color(w.ptr, host.vec3(.2, .3, .1)), "mort_add_solid_color")
        c2 = _ok(L.mort_add_solid_color(w.ptr, host.vec3(.9, .9, .9)), "mort_add_solid_color")
        ck = _ok(L.mort_add_checker_texture(w.ptr, 0.4, S.TEXTURE_SOLID, c1, S.TEXTURE_SOLID, c2), "mort_add_checker_texture")
        pal.append((S.MAT_LAMBERTIAN, _ok(L.mort_add_lambertian(w.ptr, S.TEXTURE_CHECKER, ck), "mort_add_lambertian")))
        g = S.HostRng(); L.mort_host_rng_init(C.byref(g), 5, 0)
        nz = _ok(L.mort_add_noise_texture(w.ptr, 3.0, C.byref(g)), "mort_add_noise_texture")
        pal.append((S.MAT_LAMBERTIAN, _ok(L.mort_add_lambertian(w.ptr, S.TEXTURE_NOISE, nz), "mort_add_lambertian")))
    for fuzz in (0.0, 0.3, 1.0):
        pal.append((S.MAT_METAL, _ok(L.mort_add_metal(w.ptr, host.vec3(*rng.uniform(0.5, 0.95, 3)), fuzz), "mort_add_metal")))
    for ior in (1.5, 1.0 / 1.5):
        pal.append((S.MAT_DIELECTRIC, _ok(L.mort_add_dielectric(w.ptr, ior), "mort_add_dielectric")))
    return pal


# Each family: (rng, n) -> (spheres, view requests).  A sphere is (centre, radius, material) with material None = drawn from the
# whole palette, "glass" / "glass_in" = the dielectrics 1.5 and 1 / 1.5, "solid" = anything but glass.  A view request is
# (target, direction towards the camera, vfov, defocus_angle, share of the frame the spheres should cover) -- _fit_view turns it
# into a camera -- or ("fixed", lookfrom, lookat, vfov, defocus_angle).  vfov is a whole number of degrees (the reference's camera
# keeps an int).

def _covered(frm, at, vfov, cen, rad, nx=24, ny=14):
    """share of an nx x ny grid of pinhole rays of a 16:9 camera that meet one of the spheres (centres cen (n, 3), radii rad)"""
    frm, at = np.asarray(frm, float), np.asarray(at, float)
    wv = frm - at; wv /= np.linalg.norm(wv)
    uv = np.cross((0.0, 1.0, 0.0), wv); uv /= np.linalg.norm(uv)
    vv = np.cross(wv, uv)
    h = np.tan(np.radians(vfov) / 2)
    xs = ((np.arange(nx) + 0.5) / nx * 2 - 1) * h * 16 / 9
    ys = ((np.arange(ny) + 0.5) / ny * 2 - 1) * h
    d = (xs[None, :, None] * uv + ys[:, None, None] * vv - wv).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    oc = cen - frm                                           # (n, 3)
    b = (d.astype(np.float32) @ oc.T.astype(np.float32))     # (rays, n); the camera is outside every sphere
    hit = (b > 0) & (b * b > ((oc * oc).sum(1) - rad * rad).astype(np.float32)[None, :])
    return float(hit.any(1).mean())


def _fit_view(sph, ends, target, direction, vfov, defocus, want):
    """the camera on the ray target + d * direction whose frame the spheres cover most nearly to the share `want`, among
    distances d from where the field's reach about the target fills a third of the frame's height downwards (ratio 0.64, then
    0.8 about the best of those), outside
    every sphere along its motion by a tenth of its radius and a lens' width.  target None: the centre of the sphere nearest the
    middle of the field -- a sphere's centre as target means that coming closer covers more of the frame."""
    cen = np.array([0.5 * (np.asarray(c) + np.asarray(e)) for (c, _, _), e in zip(sph, ends)], float)
    c1 = np.array([c for c, _, _ in sph], float)
    c2 = np.array(ends, float)
    rad = np.array([r for _, r, _ in sph], float)
    if target is None:
        target = cen[np.argmin(np.abs(cen - 0.5 * (cen.min(0) + cen.max(0))).sum(1))]
    target = np.asarray(target, float)
    dirn = np.asarray(direction, float); dirn = dirn / np.linalg.norm(dirn)
    reach = float((np.linalg.norm(cen - target, axis=1) + rad).max())
    best = None
    fine = (48, 27) if len(sph) <= 64 else (16, 9)
    ab = c2 - c1
    ab2 = np.maximum((ab * ab).sum(1), 1e-30)
    for k in list(range(0, 36, 2)) + [-1, 1]:
        if k in (-1, 1):                                    # the two distances next to the best of the even ones
            if best is None:
                continue
            k += best[2]
        d = 3.0 * reach / np.tan(np.radians(vfov) / 2) * 0.8 ** k
        frm = target + d * dirn
        lens = d * np.tan(np.radians(defocus) / 2) * 1.5
        t = np.clip(((frm - c1) * ab).sum(1) / ab2, 0, 1)     # distance from the camera to each sphere's path of centres
        if (np.linalg.norm(c1 + t[:, None] * ab - frm, axis=1) < 1.1 * rad + lens + 1e-3).any():
            continue
        cov = _covered(frm, target, vfov, cen, rad, *fine)
        if best is None or abs(cov - want) < abs(best[0] - want):
            best = (cov, frm, k if k % 2 == 0 else best[2])
    assert best is not None, "no camera position outside every sphere"
    return tuple(float(v) for v in best[1]), tuple(float(v) for v in target), vfov, defocus


def _slab_side(n):
    return max(1.5, 0.55 * float(np.sqrt(n)))


def _fam_uniform(rng, n):
    s = _slab_side(n)
    sph = [((float(rng.uniform(-s, s)), float(rng.uniform(0, 2)), float(rng.uniform(-s, s))), float(rng.uniform(0.05, 0.9)), None) for _ in range(n)]
    mid = min(range(n), key=lambda i: abs(sph[i][0][0]) + abs(sph[i][0][2]))
    views = [(None, (0.0, 0.45, 1.0), 40, 0.0, 0.45),          # the slab from above its edge
             (sph[mid][0], (1.0, 0.3, 0.35), 65, 0.4, 0.6),               # the sphere nearest the middle from among the others, with a lens
             (None, (-1.0, -0.03, 0.07), 30, 0.0, 0.5)]        # from outside, at ground level
    return sph, views


def _fam_cluster(rng, n):
    k = max(1, n // 24)
    g = max(1, int(np.ceil(np.sqrt(k))))
    cells = rng.permutation(g * g)[:k]
    cen = [(1.6 * (int(c) % g - 0.5 * (g - 1)), 0.8 + 0.9 * float(rng.integers(0, 2)), 1.6 * (int(c) // g - 0.5 * (g - 1))) for c in cells]
    sph = []
    for i in range(n):
        c = cen[i % k]
        p = rng.normal(0.0, 0.22, 3)
        sph.append(((c[0] + float(p[0]), c[1] + float(p[1]), c[2] + float(p[2])), float(rng.choice([0.02, 0.1, 0.4], p=[0.3, 0.4, 0.3])), None))
    views = [(None, (0.0, 0.7, 1.0), 38, 0.0, 0.45),           # every cluster
             (max(sph[0::k], key=lambda q: q[1])[0], (0.55, 0.25, 0.8), 40, 0.0, 0.55),                  # one cluster close up
             (None, (-1.0, 0.04, 0.12), 24, 0.3, 0.45)]        # along the grid's rows, with a lens
    return sph, views


def _fam_scales(rng, n):
    s = 2.0 + 1.5 * float(n) ** (1.0 / 3.0)
    sph = [(tuple(float(v) for v in rng.uniform(-s, s, 3)), float(10.0 ** rng.uniform(-2.5, 1.5)), None) for _ in range(n)]
    c, r, _ = max(sph, key=lambda q: q[1])
    views = [(c, (0.1, 0.35, 1.0), 40, 0.0, 0.5),              # the largest sphere and what sticks out of it, from outside every sphere
             (c, (1.0, 1.02, 1.04), 75, 0.0, 0.6),             # from a corner of the field
             ("fixed", (c[0] + 0.3 * r, c[1] - 0.2 * r, c[2] + 0.1 * r), (c[0] - r, c[1], c[2] + r), 70, 0.0)]  # INSIDE the largest sphere
    return sph, views


BVH_INTERIOR_VIEW = ("scales", 2)  # the one view that starts inside a sphere on purpose: no background to see


def _fam_line(rng, n):
    x0 = -0.3 * (n - 1)
    sph = [((x0 + 0.6 * i, 0.0, 0.0), 0.5, None) for i in range(n)]  # radius 0.5 every 0.6: each overlaps its neighbours
    views = [((x0 + 0.6 * (n // 2), 0.0, 0.0), (0.2, 0.28, 1.0), 40, 0.0, 0.4),   # across the line
             ((x0 + 0.6 * (n // 4), 0.0, 0.0), (-1.0, 0.012, 0.0015), 2, 0.0, 0.4)]  # along it from far away, a narrow field of view
    return sph, views


def _fam_shells(rng, n):
    k = max(1, (n + 9) // 10)
    g = max(1, int(np.ceil(np.sqrt(k))))
    cen = [(2.9 * (j % g - 0.5 * (g - 1)), 1.3, 2.9 * (j // g - 0.5 * (g - 1))) for j in range(k)]
    sph = []
    for i in range(n):
        j, lvl = i % k, i // k
        r = 1.25 * 0.8 ** lvl                       # a geometric series inwards from 1.25
        c = cen[j]
        if rng.random() < 0.5:                       # nearly concentric: off centre by a few 1e-4 of the radius
            c = tuple(float(v + d) for v, d in zip(c, rng.uniform(-3e-4, 3e-4, 3) * r))
        kind = ("glass", "glass_in", "glass", "solid")[lvl % 4] if rng.random() < 0.8 else None
        sph.append((c, r, kind))
    views = [(None, (0.0, 0.6, 1.0), 38, 0.0, 0.5),
             (cen[0], (0.35, 0.3, 0.9), 42, 0.0, 0.55),                   # one nest of shells close up
             (None, (-1.0, 0.05, 0.09), 26, 0.0, 0.45)]        # along the rows of nests
    return sph, views


def _fam_ties(rng, n):
    s = _slab_side(n)
    again = max(2, n // 6) if n >= 3 else 1          # every repeated sphere occurs three times or more: a reference leaf node holds two
    base = n - again
    sph = [((float(rng.uniform(-s, s)), float(rng.uniform(0, 2)), float(rng.uniform(-s, s))), float(rng.uniform(0.2, 0.9)), None) for _ in range(base)]
    few = sorted((int(i) for i in rng.choice(base, size=min(base, 3, max(1, again // 2)), replace=False)), key=lambda i: -sph[i][1])
    c0 = sph[few[0]][0]
    for d in range(again):                           # the few spheres that occur again and again:
        c, r, _ = sph[few[d % len(few)]]
        sph.append((c, r, None))                     # the same centre and radius, another material drawn
    sph = [sph[int(i)] for i in rng.permutation(n)]
    views = [(None, (0.0, 0.45, 1.0), 40, 0.0, 0.45),
             (c0, (0.4, 0.35, 0.85), 45, 0.0, 0.55),                      # the most repeated sphere close up
             (None, (1.0, 0.02, -0.4), 50, 0.0, 0.55)]
    return sph, views


_BVH_FAMILY = {"uniform": _fam_uniform, "cluster": _fam_cluster, "scales": _fam_scales, "line": _fam_line, "shells": _fam_shells,
               "ties": _fam_ties}
BVH_FAMILIES = tuple(_BVH_FAMILY)


def random_bvh_world(rng, n, family, extras=False, emissive=False):
    """A world that is one reference BVH over n spheres of `family` (see _fam_*), materials from a small shared palette so that
    1000 spheres stay within the reference's tables; about 15 % of the spheres move (none in `line`).  extras: checker and
    noise Lambertians in the palette; emissive: the LAST sphere of the n is a light above the field instead.
    Returns (world, views, light) -- views (lookfrom, lookat, vfov, defocus_angle) for set_view, light = (S.OBJ_SPHERE, index) of
    the emissive sphere after the BVH build has reordered the spheres (a camera's light_obj_type / light_obj_idx), or None."""
    L = host.lib()
    w = host.World()
    pal = _bvh_palette(w, rng, extras)
    sph, requests = _BVH_FAMILY[family](rng, n)
    assert len(sph) == n
    if emissive:
        top = max(c[1] + r for c, r, _ in sph[:-1]) if n > 1 else 2.0
        sph[-1] = ((0.0, top + 2.5, 0.0), 1.5, "light")
    lst = _ok(L.mort_add_hittable_list(w.ptr, True), "mort_add_hittable_list")
    ends, motion = [], {}
    for c, r, kind in sph:
        if kind == "light":
            col = _ok(L.mort_add_solid_color(w.ptr, host.vec3(6, 6, 6)), "mort_add_solid_color")
            mt, mi = S.MAT_DIFFUSE_LIGHT, _ok(L.mort_add_diffuse_light(w.ptr, S.TEXTURE_SOLID, col), "mort_add_diffuse_light")
        elif kind == "glass":
            mt, mi = pal[-2]
        elif kind == "glass_in":
            mt, mi = pal[-1]
        elif kind == "solid":
            mt, mi = pal[int(rng.integers(0, len(pal) - 2))]
        else:
            mt, mi = pal[int(rng.integers(0, len(pal)))]
        if (c, r) in motion:                         # a repeated sphere repeats its motion: an exact duplicate
            c2 = motion[c, r]
        elif family != "line" and kind != "light" and rng.random() < 0.15:
            c2 = tuple(float(a + d) for a, d in zip(c, rng.uniform(-1, 1, 3) * max(r, 0.3)))
        else:
            c2 = c
        motion[c, r] = c2
        if c2 != c:
            i = _ok(L.mort_add_moving_sphere(w.ptr, host.vec3(*c), host.vec3(*c2), r, mt, mi, True), "mort_add_moving_sphere")
        else:
            i = _ok(L.mort_add_sphere(w.ptr, host.vec3(*c), r, mt, mi, True), "mort_add_sphere")
        ends.append(c2)
        if L.mort_list_add(w.ptr, lst, S.OBJ_SPHERE, i) != 0:
            raise RuntimeError("mort_list_add failed: the list is full")
    _ok(L.mort_add_bvh(w.ptr, lst, False), "mort_add_bvh")
    w.c.bvh_mode = True
    views = [tuple(q[1:]) if q[0] == "fixed" else _fit_view(sph, ends, *q) for q in requests]
    light = None
    if emissive:
        o = w.c.objs
        idx = [i for i in range(o.num_spheres) if o.host_sphere[i].mat_type == S.MAT_DIFFUSE_LIGHT]
        assert len(idx) == 1
        light = (S.OBJ_SPHERE, idx[0])
    return w, views, light


# The catalogue: name -> (family, spheres, seed, extras, emissive).  Two seeds of every family at 2 .. 7 spheres (2: one leaf
# node, no own tree), 64, 300, the family's size just below and just above the 72 KB limit on the LDS images
# (world_images.h build_bvh_images; found on the CPU, tests/test_bvh_random_host.py holds the census) and 1000, the list's
# capacity; seed 1 of the 64s and 300s with checker and noise textures.
BVH_LIMIT_SIZES = {"uniform": (650, 660), "cluster": (640, 660), "scales": (640, 650), "line": (670, 680), "shells": (640, 660),
                   "ties": (650, 670)}
BVH_RANDOM = {f"{fam}_{n}_s{seed}": (fam, n, seed, seed == 1 and n in (64, 300), False)
              for fam in BVH_FAMILIES for n in (2, 3, 4, 5, 7, 64, 300) + BVH_LIMIT_SIZES[fam] + (1000,) for seed in (0, 1)}
# worlds whose own tree has no four-wide form (pending-children bound above MORT_OWN4_STACK) although their size is well within
# the image limit
BVH_RANDOM.update({f"{fam}_{n}_s{seed}": (fam, n, seed, False, False)
                   for fam, n, seed in (("ties", 460, 1), ("scales", 430, 1), ("scales", 620, 0), ("scales", 620, 1))})
# one emissive sphere above a uniform field: the light object of tests that name one
BVH_RANDOM["uniform_300_lit"] = ("uniform", 300, 2, True, True)
_bvh_random_built = {}


def bvh_random_case(name):
    """(world, views, light) of a catalogue entry, built once per process; nothing may change the world"""
    if name not in _bvh_random_built:
        fam, n, seed, extras, emissive = BVH_RANDOM[name]
        rng = np.random.default_rng([seed, n, BVH_FAMILIES.index(fam)])
        _bvh_random_built[name] = random_bvh_world(rng, n, fam, extras=extras, emissive=emissive)
    return _bvh_random_built[name]


def bvh_random_camera(name, k, light=None, width=96):
    """view k of a catalogue entry as a 96 x 54 camera: 4 spp (9 on every seventh (entry, view) pair), bounce limits from 2 to 20
    in turn.  light: (type, index) to name as the camera's light object; width: another image width, 16 : 9 as well."""
    _, views, _ = bvh_random_case(name)
    i = sorted(BVH_RANDOM).index(name) * 3 + k
    _, cam = host.build_scene(1, width=width, spp=9 if i % 7 == 0 else 4, depth=(2, 5, 8, 12, 20)[i % 5])
    if light is not None:
        cam.light_obj_type, cam.light_obj_idx = light
    frm, at, vfov, defocus = views[k]
    set_view(cam, frm, at, vfov=vfov, defocus=defocus)
    return cam


def bvh_random_prediction(name):
    """What the host will decide for a catalogue entry, from the two device-free debug entries of libmort_hip.so:
    dict(tree = the nine facts of mort_hip_debug_own_tree, image = those of mort_hip_debug_bvh_images, state = 1 no own tree /
    2 own tree without a four-wide form / 3 both, fits = mega_bvh_kernel and the wavefront pipeline serve the world,
    kernel = the family megakernel mode renders it with)"""
    from mort_amd import hip
    w, _, _ = bvh_random_case(name)
    t, im = hip.debug_own_tree(w), hip.debug_bvh_images(w)
    state = 1 if t["leaves"] < 2 else 2 if t["n4"] == 0 else 3
    fits = bool(im["fits"])
    return dict(tree=t, image=im, state=state, fits=fits, kernel="mega_bvh_kernel" if fits else "mega_kernel")


# ---- random worlds WITHOUT a reference BVH (tests/test_gen_random_host.py, tests/test_gpu_gen_random.py) ----
# mega_gen_kernel, wf_trav_gen and the tree forms of the feature and query kernels walk this build's unified tree
# (scene_compile.h build_unified).  Each family below is aimed at one part of that builder or of dev_gen.h; the cameras are placed
# with the tree's own constants (hip.debug_gen_tree): one where the static sphere pad applies (|o - G| <= 2 R + 1), one where the
# per-ray band widens (beyond mnear, within reach), and on some entries one beyond reach.
#
# A family: (rng, n, seed) -> dict(prims, media, light, shift, scale).  A primitive is ("s", centre, radius, end of its motion or None) |
# ("q", Q, u, v) | ("box", size, translation, degrees) (a rotated box: six quads under translate(rotate_y(list))) |
# ("inst", kind, primitive, a, b) with kind "TR" translate a (rotate_y b degrees (primitive)), "TT" translate a (translate b
# (primitive)), "T" translate a, "R" rotate_y b; followed by an optional material: "light", "glass", or None = drawn from the palette.
# n counts the entries of the unified tree: a box is six of them, a medium's boundary is none.

GEN_TRANSLATES = GEN_ROTATIONS = 50   # the reference's tables (objects.cuh)


def _v(a):
    return tuple(float(x) for x in a)


def _gen_mixed_prims(rng, n, s=None, boxes=True, radii=(0.05, 0.2, 0.5, 0.9)):
    """spheres (15 % moving, one ground sphere among them from 3 on), quads, up to two rotated boxes: n tree entries in a slab"""
    nb = 0 if not boxes else 2 if n >= 30 else 1 if n >= 14 else 0
    m = n - 6 * nb
    ns = max(1, int(round(0.3 * m))) if m > 1 else m
    nq = m - ns
    s = s or max(1.5, 0.4 * float(np.sqrt(n)))
    prims = []
    for i in range(ns):
        if i == 0 and ns >= 3:
            prims.append(("s", (0.0, -1000.0, 0.0), 1000.0, None))       # ground: a giant among ordinary spheres
            continue
        c = (float(rng.uniform(-s, s)), float(rng.uniform(0.1, 2.2)), float(rng.uniform(-s, s)))
        r = float(rng.choice(radii))
        end = _v(np.asarray(c) + rng.uniform(-0.5, 0.5, 3)) if rng.random() < 0.15 else None
        prims.append(("s", c, r, end))
    for _ in range(nq):
        q = (float(rng.uniform(-s, s)), float(rng.uniform(0.0, 2.5)), float(rng.uniform(-s, s)))
        prims.append(("q", q, _v(rng.uniform(-1.2, 1.2, 3)), _v(rng.uniform(-1.2, 1.2, 3))))
    for _ in range(nb):
        prims.append(("box", _v(rng.uniform(0.4, 1.6, 3)), (float(rng.uniform(-s, s)), 0.0, float(rng.uniform(-s, s))), float(rng.uniform(-60, 60))))
    return prims, s


def _gen_media(rng, s, k):
    return [((float(rng.uniform(-s, s)) * 0.6, 1.0, float(rng.uniform(-s, s)) * 0.6), float(rng.uniform(0.6, 1.8)), float(rng.uniform(0.1, 2.0))) for _ in range(k)]


def _gfam_mixed(rng, n, seed):
    prims, s = _gen_mixed_prims(rng, n)
    light = n >= 5 and seed == 1
    if light:
        i = max(j for j, p in enumerate(prims) if p[0] == "q")
        prims[i] = ("q", (-1.5, 5.0, -1.5), (3.0, 0.0, 0.0), (0.0, 0.0, 3.0), "light")
    return dict(prims=prims, media=_gen_media(rng, s, 1 + seed) if n >= 47 else [], light=light)


def _gfam_offset(rng, n, seed):
    """a mixed world far from the origin: seed 0 about 3e4 away and 5 times as large, seed 1 about 1e6 away and 300 times as
    large (one ulp of a coordinate is 0.06 there, and the tree's R carries 1e-3 of the distance from the origin)"""
    prims, s = _gen_mixed_prims(rng, n, radii=(0.3, 0.5, 0.9))
    return dict(prims=prims, media=_gen_media(rng, s, 1) if n >= 47 else [], light=False,
                shift=((3e4, -2e4, 2.5e4), (1e6, 0.0, -1e6))[seed], scale=(5.0, 300.0)[seed])


def _gfam_scales(rng, n, seed):
    """spheres only, radii log-uniform over four decades (1e-3 .. 10), centres in a box of half side 4 whatever n is; seed 1 of the
    sizes 2 and 3 draws every radius from the top of the range, so that all are giants"""
    lo, hi = (0.9, 1.0) if (seed == 1 and n in (2, 3)) else (-3.0, 1.0)
    return dict(prims=[("s", _v(rng.uniform(-4, 4, 3)), float(10.0 ** rng.uniform(lo, hi)), None) for _ in range(n)], media=[], light=False)


def _gfam_quads(rng, n, seed):
    """quads only: axis-aligned sheets on shared planes (zero extent on one axis), slivers with |u| / |v| about 1e3, and a floor and a
    back wall that span the world next to small quads"""
    s = max(2.0, 0.55 * float(n) ** (1.0 / 3.0) * 1.6)
    prims = []
    if n >= 3:
        prims.append(("q", (-2 * s, -s, -2 * s), (4 * s, 0.0, 0.0), (0.0, 0.0, 4 * s)))     # floor
    if n >= 5:
        prims.append(("q", (-2 * s, -s, -s), (4 * s, 0.0, 0.0), (0.0, 3 * s, 0.0)))        # back wall
    planes = [round(float(v), 1) for v in rng.uniform(-s, s, 4)]
    while len(prims) < n:
        k = rng.random()
        a, b = float(rng.uniform(-s, s)), float(rng.uniform(-s, s))
        if k < 0.5:                                  # a sheet in one of a few shared axis-aligned planes
            ax = int(rng.integers(0, 3)); p = planes[int(rng.integers(0, len(planes)))]
            e1, e2 = [j for j in range(3) if j != ax]
            q = [0.0, 0.0, 0.0]; u = [0.0, 0.0, 0.0]; v = [0.0, 0.0, 0.0]
            q[ax] = p; q[e1] = a; q[e2] = b; u[e1] = float(rng.uniform(0.3, 1.5)); v[e2] = float(rng.uniform(0.3, 1.5))
            prims.append(("q", tuple(q), tuple(u), tuple(v)))
        elif k < 0.7:                                # a sliver
            d = rng.normal(size=3); d /= np.linalg.norm(d)
            e = np.cross(d, rng.normal(size=3)); e /= np.linalg.norm(e)
            L = float(rng.uniform(1.0, 2.0) * s)
            prims.append(("q", (a, float(rng.uniform(-s, s)), b), _v(d * L), _v(e * L * 1e-3 * float(rng.uniform(0.5, 2.0)))))
        else:
            prims.append(("q", (a, float(rng.uniform(-s, s)), b), _v(rng.uniform(-1.0, 1.0, 3)), _v(rng.uniform(-1.0, 1.0, 3))))
    return dict(prims=prims[:n], media=[], light=False)


def _gfam_line(rng, n, seed):
    """spheres and quads along a slanted line, size and spacing growing geometrically over four decades: the surface-area split
    peels the large end off one primitive at a time until the depth cap takes over"""
    g = 10.0 ** (4.0 / max(n - 1, 1))
    d = np.array([1.0, 0.05, 0.3]); d /= np.linalg.norm(d)
    prims, x = [], 0.0
    for i in range(n):
        r = 0.01 * g ** i
        c = d * x + rng.uniform(-0.2, 0.2, 3) * r
        if i % 3 == 2:
            e1 = np.cross(d, (0.0, 1.0, 0.0)); e1 /= np.linalg.norm(e1)
            e2 = np.cross(d, e1)
            prims.append(("q", _v(c - r * (e1 + e2)), _v(2 * r * e1 + 0.3 * r * d), _v(2 * r * e2)))
        else:
            prims.append(("s", _v(c), float(r), None))
        x += 1.2 * r * (1.0 + g)
    return dict(prims=prims, media=[], light=False)


def _gfam_ties(rng, n, seed):
    """groups of two to five identical spheres (a moving one repeats its motion) and identical quads, and quads lying in another
    quad's plane: equal t, which the scan order decides"""
    s = max(1.5, 0.4 * float(np.sqrt(n)))
    prims = [("s", (0.0, -1000.0, 0.0), 1000.0, None)] if n >= 6 else []
    while len(prims) < n:
        k = min(int(rng.integers(2, 6)), n - len(prims))
        c = (float(rng.uniform(-s, s)), float(rng.uniform(0.2, 2.2)), float(rng.uniform(-s, s)))
        kind = rng.random()
        if kind < 0.5:
            r = float(rng.uniform(0.2, 0.8))
            end = _v(np.asarray(c) + rng.uniform(-0.5, 0.5, 3)) if rng.random() < 0.15 else None
            prims += [("s", c, r, end)] * k
        else:
            u, v = rng.uniform(-1.5, 1.5, 3), rng.uniform(-1.5, 1.5, 3)
            if kind < 0.8:
                prims += [("q", c, _v(u), _v(v))] * k
            else:                                    # smaller quads inside the first one's parallelogram
                prims.append(("q", c, _v(u), _v(v)))
                for j in range(1, k):
                    f = 0.5 ** j
                    prims.append(("q", _v(np.asarray(c) + 0.25 * u + 0.25 * v), _v(u * f), _v(v * f)))
    prims = prims[:1] + [prims[1:][int(i)] for i in rng.permutation(len(prims) - 1)] if len(prims) > 2 else prims
    return dict(prims=prims, media=_gen_media(rng, s, 1) if n >= 47 else [], light=False)


def _gfam_instances(rng, n, seed):
    """single spheres (some moving) and quads under translate(rotate_y()), translate(translate()), translate() and rotate_y() until
    the reference's 50 translates and 50 rotations are used up, two rotated boxes (six quads sharing one chain each) from 30
    primitives on, and plain primitives for the rest of n"""
    nb = 2 if n >= 30 else 1 if n >= 14 else 0
    T = GEN_TRANSLATES - nb; R = GEN_ROTATIONS - nb
    s = max(1.5, 0.4 * float(np.sqrt(n)))
    prims = []
    kinds = ("TR", "TT", "T", "R")
    i = 0
    while len(prims) < n - 6 * nb:
        kind = kinds[i % 4]; i += 1
        need = {"TR": (1, 1), "TT": (2, 0), "T": (1, 0), "R": (0, 1)}[kind]
        if need[0] > T or need[1] > R:
            if T == 0 and R == 0 or i > 400:
                break
            continue
        T -= need[0]; R -= need[1]
        if rng.random() < 0.6:
            c = _v(rng.uniform(-0.3, 0.3, 3))
            end = _v(np.asarray(c) + rng.uniform(-0.4, 0.4, 3)) if rng.random() < 0.25 else None
            base = ("s", c, float(rng.uniform(0.15, 0.7)), end)
        else:
            base = ("q", _v(rng.uniform(-0.5, 0.5, 3)), _v(rng.uniform(-1.2, 1.2, 3)), _v(rng.uniform(-1.2, 1.2, 3)))
        a = (float(rng.uniform(-s, s)), float(rng.uniform(0.3, 2.2)), float(rng.uniform(-s, s)))
        if kind == "R":                              # a rotation about the y axis keeps the distance from it: place the primitive itself
            base = (base[0], _v(np.asarray(base[1]) + a)) + base[2:]
            if base[0] == "s" and base[3] is not None:
                base = base[:3] + (_v(np.asarray(base[3]) + a),)
        b = float(rng.uniform(-80, 80)) if kind in ("TR", "R") else _v(rng.uniform(-0.5, 0.5, 3))
        prims.append(("inst", kind, base, a, b))
    rest = n - 6 * nb - len(prims)
    if rest > 0:
        prims += _gen_mixed_prims(rng, rest, s, boxes=False)[0]
    for _ in range(nb):
        prims.append(("box", _v(rng.uniform(0.4, 1.6, 3)), (float(rng.uniform(-s, s)), 0.0, float(rng.uniform(-s, s))), float(rng.uniform(-60, 60))))
    return dict(prims=prims, media=[], light=False)


_GEN_FAMILY = {"mixed": _gfam_mixed, "scales": _gfam_scales, "offset": _gfam_offset, "quads": _gfam_quads, "line": _gfam_line,
               "ties": _gfam_ties, "instances": _gfam_instances}
GEN_FAMILIES = tuple(_GEN_FAMILY)


def _rot_y(p, deg):
    st, ct = np.sin(np.radians(deg)), np.cos(np.radians(deg))
    p = np.asarray(p, float)
    return np.array([ct * p[0] + st * p[2], p[1], -st * p[0] + ct * p[2]])


def _covered_gen(frm, at, vfov, cen, rad, Q, U, V, nx=16, ny=9):
    """share of an nx x ny grid of pinhole rays of a 16:9 camera that meet a sphere (cen (n, 3), rad) or a quad (Q, U, V (m, 3))"""
    frm, at = np.asarray(frm, float), np.asarray(at, float)
    wv = frm - at; wv /= np.linalg.norm(wv)
    uv = np.cross((0.0, 1.0, 0.0), wv)
    if np.linalg.norm(uv) < 1e-9:
        uv = np.array([1.0, 0.0, 0.0])
    uv /= np.linalg.norm(uv)
    vv = np.cross(wv, uv)
    h = np.tan(np.radians(vfov) / 2)
    xs = ((np.arange(nx) + 0.5) / nx * 2 - 1) * h * 16 / 9
    ys = ((np.arange(ny) + 0.5) / ny * 2 - 1) * h
    d = (xs[None, :, None] * uv + ys[:, None, None] * vv - wv).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    hit = np.zeros(len(d), bool)
    if len(cen):
        oc = cen - frm
        b = d @ oc.T
        c = (oc * oc).sum(1) - rad * rad
        hit |= (((b > 0) & (b * b > c[None, :])) | (c[None, :] < 0)).any(1)
    if len(Q):
        n = np.cross(U, V)
        w = n / np.maximum((n * n).sum(1, keepdims=True), 1e-300)
        den = d @ n.T                                             # (rays, m)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((Q - frm) * n).sum(1)[None, :] / den
            p = frm[None, None, :] + t[:, :, None] * d[:, None, :] - Q[None, :, :]
            al = (w[None] * np.cross(p, V[None])).sum(2)
            be = (w[None] * np.cross(U[None], p)).sum(2)
            hit |= ((t > 1e-3) & (al >= 0) & (al <= 1) & (be >= 0) & (be <= 1)).any(1)
    return float(hit.mean())


_GEN_VFOVS = (1, 2, 3, 5, 8, 12, 18, 26, 36, 48, 62, 78)
_GEN_DIRS = ((0.25, 0.45, 1.0), (1.0, 0.3, 0.35), (-0.8, 0.6, 0.5), (-0.3, 0.2, -1.0), (0.6, 1.0, -0.4))


def _gen_far(pos, t):
    """gen_ray_setup's `far` for an origin, in float32 as the device computes it"""
    F = np.float32
    e = [F(F(pos[k]) - t["centre"][k]) for k in range(3)]
    return F(F(np.sqrt(F(F(F(e[0] * e[0]) + F(e[1] * e[1])) + F(e[2] * e[2])))) * F(1.000001)) + t["R"]


def gen_in_reach(pos, rad, reach):
    """camera_in_reach (mort_ctx.h) for a camera centre and lens radius, in float32"""
    F = np.float32
    return all(F(F(pos[k]) - F(rad)) >= F(reach["lo"][k] - reach["reach"]) and F(F(pos[k]) + F(rad)) <= F(reach["hi"][k] + reach["reach"]) for k in range(3))


def _gen_fit(proxy, cands, want):
    """the (lookfrom, lookat, vfov) among the candidates (lookfrom, lookat) and the whole-degree fields of view whose frame the
    primitives cover most nearly to the share `want`"""
    best = None
    for frm, at in cands:
        lo, hi = 0, len(_GEN_VFOVS) - 1
        tried = {}
        while lo <= hi:                                # coverage falls as the field of view widens about a target that is hit
            mid = (lo + hi) // 2
            tried[mid] = cov = _covered_gen(frm, at, _GEN_VFOVS[mid], *proxy)
            if cov > want:
                lo = mid + 1
            else:
                hi = mid - 1
        for i, cov in tried.items():
            if best is None or abs(cov - want) < abs(best[0] - want):
                best = (cov, frm, at, _GEN_VFOVS[i])
    return _v(best[1]), _v(best[2]), best[3]


def random_gen_world(rng, n, family, seed, far_view=False, tele_view=False):
    """A world without a reference BVH of n tree entries of `family`, materials from a small shared palette.
    Returns (world, views, light, info): views (lookfrom, lookat, vfov, defocus_angle) for set_view -- view 0 within 2 R + 1 of the
    tree's centre, view 1 beyond mnear within reach, then (far_view) one beyond reach and (tele_view) ("tele", origin, target, span):
    a telescope (tests/grazing.py microscope) four fifths of the reach away, whose square viewport frames the field of ordinary
    spheres -- there u |oc|^2 exceeds the small spheres' r^2, sphere::hit accepts rays that pass far outside every static pad, and
    only the per-ray band of gen_ray_setup keeps the walk from pruning them; light = (type, index) of the quad light or None;
    info = dict(spheres = world-space (centre, end, radius) of the tree's spheres, moving, instances, shift)."""
    from mort_amd import hip
    L = host.lib()
    w = host.World()
    pal = _bvh_palette(w, rng, True)
    spec = _GEN_FAMILY[family](rng, n, seed)
    shift = np.asarray(spec.get("shift", (0.0, 0.0, 0.0)), float); scale = float(spec.get("scale", 1.0))
    lightmat = None
    light = None
    sph, quads = [], []                                  # world-space proxies: (c1, c2, r), (Q, u, v)
    moving = instances = 0

    def mat(p, k):
        nonlocal lightmat
        if len(p) > k and p[k] == "light":
            if lightmat is None:
                col = _ok(L.mort_add_solid_color(w.ptr, host.vec3(7, 7, 7)), "mort_add_solid_color")
                lightmat = (S.MAT_DIFFUSE_LIGHT, _ok(L.mort_add_diffuse_light(w.ptr, S.TEXTURE_SOLID, col), "mort_add_diffuse_light"))
            return lightmat
        return pal[int(rng.integers(0, len(pal)))]

    def place(x):                                        # the family's coordinates -> the world's
        return np.asarray(x, float) * scale + shift

    def add(p, skip, to_world, top):
        """adds a sphere or a quad (coordinates already final, in its own frame); to_world maps a point of that frame to the world"""
        nonlocal moving, light
        if p[0] == "s":
            mt, mi = mat(p, 4)
            c, r, end = np.asarray(p[1], float), float(p[2]), p[3]
            if end is not None:
                moving += 1
                i = _ok(L.mort_add_moving_sphere(w.ptr, host.vec3(*c), host.vec3(*end), r, mt, mi, skip), "mort_add_moving_sphere")
            else:
                i = _ok(L.mort_add_sphere(w.ptr, host.vec3(*c), r, mt, mi, skip), "mort_add_sphere")
            sph.append((to_world(c), to_world(c if end is None else end), r))
            return S.OBJ_SPHERE, i
        mt, mi = mat(p, 4)
        q, u, v = (np.asarray(x, float) for x in p[1:4])
        i = _ok(L.mort_add_quad(w.ptr, host.vec3(*q), host.vec3(*u), host.vec3(*v), mt, mi, skip), "mort_add_quad")
        if mt == S.MAT_DIFFUSE_LIGHT and top:
            light = (S.OBJ_QUAD, i)
        o = to_world(q)
        quads.append((o, to_world(q + u) - o, to_world(q + v) - o))
        return S.OBJ_QUAD, i

    def scaled(p, with_shift):
        sh = shift if with_shift else 0.0
        if p[0] == "s":
            return ("s", _v(np.asarray(p[1], float) * scale + sh), p[2] * scale, None if p[3] is None else _v(np.asarray(p[3], float) * scale + sh)) + tuple(p[4:])
        return ("q", _v(np.asarray(p[1], float) * scale + sh), _v(np.asarray(p[2], float) * scale), _v(np.asarray(p[3], float) * scale)) + tuple(p[4:])

    for p in spec["prims"]:
        if p[0] in ("s", "q"):
            add(scaled(p, True), False, lambda x: np.asarray(x, float), True)
        elif p[0] == "box":
            size, tr, deg = np.asarray(p[1], float) * scale, place(p[2]), p[3]
            mt, mi = mat(p, 4)
            L.mort_rotated_box(w.ptr, host.vec3(*size), host.vec3(*tr), deg, mt, mi)
            f = lambda x, tr=tr, deg=deg: _rot_y(x, deg) + tr
            for q, u, v in (((0, 0, size[2]), (size[0], 0, 0), (0, size[1], 0)), ((size[0], 0, size[2]), (0, 0, -size[2]), (0, size[1], 0)),
                            ((size[0], 0, 0), (-size[0], 0, 0), (0, size[1], 0)), ((0, 0, 0), (0, 0, size[2]), (0, size[1], 0)),
                            ((0, size[1], size[2]), (size[0], 0, 0), (0, 0, -size[2])), ((0, 0, 0), (size[0], 0, 0), (0, 0, size[2]))):
                q, u, v = (np.asarray(x, float) for x in (q, u, v))
                quads.append((f(q), f(q + u) - f(q), f(q + v) - f(q)))
            instances += 1
        else:
            _, kind, base, a, b = p
            a = np.asarray(a, float)
            instances += 1
            if kind == "TR":
                f = lambda x, a=a, b=b: _rot_y(x, b) + a
                t, i = add(base, True, f, False)
                r = _ok(L.mort_add_rotate_y(w.ptr, t, i, b, True), "mort_add_rotate_y")
                _ok(L.mort_add_translate(w.ptr, S.OBJ_ROTATE_Y, r, host.vec3(*a), False), "mort_add_translate")
            elif kind == "TT":
                bb = np.asarray(b, float)
                f = lambda x, a=a, bb=bb: np.asarray(x, float) + bb + a
                t, i = add(base, True, f, False)
                r = _ok(L.mort_add_translate(w.ptr, t, i, host.vec3(*bb), True), "mort_add_translate")
                _ok(L.mort_add_translate(w.ptr, S.OBJ_TRANSLATE, r, host.vec3(*a), False), "mort_add_translate")
            elif kind == "T":
                f = lambda x, a=a: np.asarray(x, float) + a
                t, i = add(base, True, f, False)
                _ok(L.mort_add_translate(w.ptr, t, i, host.vec3(*a), False), "mort_add_translate")
            else:
                f = lambda x, b=b: _rot_y(x, b)
                t, i = add(base, True, f, False)
                _ok(L.mort_add_rotate_y(w.ptr, t, i, b, False), "mort_add_rotate_y")
    iso = None
    for centre, radius, density in spec["media"]:
        bnd = _ok(L.mort_add_sphere(w.ptr, host.vec3(*place(centre)), radius * scale, pal[-2][0], pal[-2][1], True), "mort_add_sphere")
        if iso is None:
            col = _ok(L.mort_add_solid_color(w.ptr, host.vec3(.8, .8, .9)), "mort_add_solid_color")
            iso = _ok(L.mort_add_isotropic(w.ptr, S.TEXTURE_SOLID, col), "mort_add_isotropic")
        _ok(L.mort_add_constant_medium(w.ptr, S.OBJ_SPHERE, bnd, density / scale, S.MAT_ISOTROPIC, iso, False), "mort_add_constant_medium")
    w.c.bvh_mode = False

    # ---- cameras, from the tree's own constants ----
    t = hip.debug_gen_tree(w); reach = hip.debug_gen_reach(w)
    assert t["tree"] and t["entries"] == n, (family, n, t)
    cen = np.array([0.5 * (a + b) for a, b, _ in sph], float).reshape(-1, 3)
    rad = np.array([r for _, _, r in sph], float)
    Q = np.array([q for q, _, _ in quads], float).reshape(-1, 3)
    U = np.array([u for _, u, _ in quads], float).reshape(-1, 3)
    V = np.array([v for _, _, v in quads], float).reshape(-1, 3)
    if len(Q) > 500:                                    # fitting only: every k-th quad behind the first eight is enough
        keep = np.r_[0:8, 8:len(Q):-(-len(Q) // 500)]
        Q, U, V = Q[keep], U[keep], V[keep]
    proxy = (cen, rad, Q, U, V)
    G = t["centre"].astype(float)
    near = 2.0 * float(t["R"]) + 1.0
    lo, hi = reach["lo"].astype(float), reach["hi"].astype(float)
    mid = 0.5 * (lo + hi)
    big = family == "line"                              # the line is seen at its large end
    aim = [G] if not big else [np.asarray(sph[-1][0] if spec["prims"][-1][0] == "s" else quads[-1][0], float)]
    if len(cen) == 0:
        aim = [mid * 0.3, np.array([0.0, -0.5 * (hi[1] - lo[1]), -0.4 * (hi[2] - lo[2])])]
    if not big:                                         # a few primitives leave the middle empty: aim at one of them as well
        pc = np.concatenate([cen, Q + 0.5 * (U + V)]) if len(Q) else cen
        ps = np.concatenate([rad, 0.5 * np.sqrt(np.linalg.norm(np.cross(U, V), axis=1))]) if len(Q) else rad
        ordinary = ps <= max(near, 0.25 * np.linalg.norm(hi - lo))
        if ordinary.any():
            idx = np.flatnonzero(ordinary)
            aim.append(pc[idx[np.argmax(ps[idx])]])
            aim.append(pc[idx[np.argmin(np.linalg.norm(pc[idx] - aim[0], axis=1))]])
    dirs = [np.asarray(d, float) / np.linalg.norm(d) for d in (_GEN_DIRS if n <= 600 else _GEN_DIRS[:3])]
    views = []
    cands = []
    for d in dirs:
        for f in (0.93, 0.6, 0.3) + ((0.1,) if n <= 150 else ()):
            pos = G + d * f * near
            if _gen_far(pos, t) > t["mnear"]:
                continue
            for at in aim:
                if np.linalg.norm(at - pos) > 1e-6 * (1 + np.abs(pos).max()):
                    cands.append((pos, at))
            if len(cen) == 0 or f == 0.3:
                cands.append((pos, pos - d + np.array([0.0, -0.4, 0.0])))          # outwards and down
    views.append(_gen_fit(proxy, cands, 0.6) + (0.0,))
    cands = []
    lens = 0.3 if (n % 2 == 1 and seed == 1) else 0.0
    outer = [np.linalg.norm(c - G) + r for c, r in zip(cen, rad) if r < 500.0 * scale]   # the ground aside, from outside every sphere too
    for d in dirs:
        for f in (1.08, 1.5, 2.5) + ((1.6 * max(outer) / near,) if outer and 1.6 * max(outer) > 1.08 * near else ()):
            if len(cen) == 0:                           # no sphere, no band to widen (mnear = 1e30, kmin = 0): a camera outside the solids' box
                pos = mid + d * (0.8 + 0.5 * f) * np.linalg.norm(hi - lo)
            else:
                pos = G + d * (f * near + 1e-3 * np.abs(G).max())
                if not (_gen_far(pos, t) > t["mnear"]):
                    continue
            if not gen_in_reach(pos, 0.2 * np.linalg.norm(pos - G), reach):
                continue
            for at in aim:
                cands.append((pos, at))
    views.append(_gen_fit(proxy, cands, 0.6) + (lens,))
    if far_view:
        d = dirs[0]
        k = 1.05
        while True:
            pos = mid + d * k * (float(reach["reach"]) + np.linalg.norm(hi - lo)) / np.abs(d).max()
            if not gen_in_reach(pos, 0.0, reach):
                break
            k *= 1.1
        views.append(_gen_fit(proxy, [(pos, a) for a in aim + [mid]], 0.6) + (0.0,))
    if tele_view:
        d = np.array([0.6, 0.02, 0.8]); d /= np.linalg.norm(d)
        dist = 0.8 * float(reach["reach"]) / np.abs(d).max()
        while not gen_in_reach(G + d * dist, 0.0, reach):
            dist *= 0.9
        span = 2.4 * max(float(t["R"]) - 1e-3 * (1.0 + np.abs(np.r_[lo, hi]).max()), 1.0)
        views.append(("tele", _v(G + d * dist), _v(G + np.array([0.0, 0.15 * span, 0.0])), span))
    info = dict(spheres=sph, moving=moving, instances=instances, shift=shift, scale=scale, n_spheres=len(sph), n_quads=len(quads))
    return w, views, light, info


# The catalogue: name -> (family, tree entries, seed).  Two seeds of every family at 1 (not `ties`: a tie takes two), 2, 3, 5, 47 and
# 48 (the two sides of the default MORT_GEN_MIN_PRIMS), 150, the family's sizes just below and just above the 48 KB rule that puts
# the primitives into the LDS image (world_images.h build_gen_image; found on the CPU with hip.debug_gen_tree,
# tests/test_gen_random_host.py holds the census) and 1000; `mixed` and `quads` once more near the capacity of the reference's
# sphere and quad tables.
GEN_LIMIT_SIZES = {"mixed": (300, 310), "scales": (540, 550), "offset": (300, 310), "quads": (260, 270), "line": (390, 410), "ties": (330, 360),
                   "instances": (290, 300)}
GEN_CAPACITY_SIZES = {"mixed": 3500, "quads": 2490}
GEN_SMALL_SIZES = (1, 2, 3, 5, 47, 48, 150)


def gen_random_sizes(fam):
    return tuple(n for n in GEN_SMALL_SIZES if not (fam == "ties" and n == 1)) + GEN_LIMIT_SIZES[fam] + (1000,) + \
        ((GEN_CAPACITY_SIZES[fam],) if fam in GEN_CAPACITY_SIZES else ())


GEN_RANDOM = {f"{fam}_{n}_s{seed}": (fam, n, seed) for fam in GEN_FAMILIES for n in gen_random_sizes(fam) for seed in (0, 1)}
# the entries with a third camera, beyond the tree's reach: the one-lane kernel renders it, wavefront mode refuses it
# the entries with a telescope as their last camera: the families with a ground sphere at the origin (so a reach of thousands of
# units), at the sizes from 150 on (smaller fields, and the far-away and all-sizes worlds, leave such a frame without sky)
GEN_TELE_FAMILIES = ("mixed", "ties", "instances")
GEN_FAR_VIEWS = tuple(f"{fam}_{n}_s0" for fam in ("mixed", "scales", "quads", "ties", "instances") for n in (5, 150))
_gen_random_built = {}


def gen_has_tele(name):
    fam, n, _ = GEN_RANDOM[name]
    return fam in GEN_TELE_FAMILIES and n >= 150


def gen_random_case(name):
    """(world, views, light, info) of a catalogue entry, built once per process; nothing may change the world"""
    if name not in _gen_random_built:
        fam, n, seed = GEN_RANDOM[name]
        rng = np.random.default_rng([seed, n, GEN_FAMILIES.index(fam)])
        _gen_random_built[name] = random_gen_world(rng, n, fam, seed, far_view=name in GEN_FAR_VIEWS, tele_view=gen_has_tele(name))
    return _gen_random_built[name]


def gen_random_camera(name, k, width=None):
    """view k of a catalogue entry as a 16 : 9 camera, 64 wide up to 150 primitives, 48 wide up to 1100, 32 beyond: 4 spp (9 on
    every seventh (entry, view) pair), bounce limits from 2 to 20 in turn; the world's quad light, if it has one, is the camera's
    light object."""
    _, views, light, _ = gen_random_case(name)
    n = GEN_RANDOM[name][1]
    i = sorted(GEN_RANDOM).index(name) * 3 + k
    cam = flat_camera(light=light, spp=9 if i % 7 == 0 else 4, width=width or (64 if n <= 150 else 48 if n <= 1100 else 32), depth=(2, 5, 8, 12, 20)[i % 5])
    if views[k][0] == "tele":
        from tests.grazing import microscope
        microscope(cam, views[k][1], views[k][2], views[k][3], W=cam.image_width, H=cam.image_height)
        cam.samples_per_pixel, cam.sqrt_spp, cam.recip_sqrt_spp, cam.pixel_samples_scale = 4, 2, 0.5, 0.25
        return cam
    frm, at, vfov, defocus = views[k]
    set_view(cam, frm, at, vfov=vfov, defocus=defocus)
    return cam


def gen_camera_lens(cam):
    """the lens radius choose_family widens camera_in_reach by, in float32"""
    F = np.float32
    r = F(0)
    for v in (cam.defocus_disk_u, cam.defocus_disk_v):
        for k in range(3):
            r = F(r + F(abs(F(v.e[k]))))
    return r


GEN_MIN_PRIMS = 48  # the default of MORT_GEN_MIN_PRIMS (mort_hip.hip choose_family)


def gen_random_prediction(name, min_prims=GEN_MIN_PRIMS):
    """What the host will decide for a catalogue entry, from the two device-free debug entries of libmort_hip.so:
    dict(tree = the facts of mort_hip_debug_gen_tree, has_tree, prims_in_lds, in_reach[k], near[k] (gen_ray_setup leaves the
    camera centre's band alone), kernel[k] = the family megakernel mode renders view k with: mega_gen_kernel where the camera
    is in reach and the tree has at least min_prims entries, else mega_kernel)"""
    from mort_amd import hip
    w, views, _, _ = gen_random_case(name)
    t, reach = hip.debug_gen_tree(w), hip.debug_gen_reach(w)
    ok = t["tree"] and t["fits"]
    inr, near, kern = [], [], []
    for k in range(len(views)):
        cam = gen_random_camera(name, k)
        pos = [cam.center.e[j] for j in range(3)]
        inr.append(bool(ok and gen_in_reach(pos, gen_camera_lens(cam), reach)))
        near.append(bool(not (_gen_far(pos, t) > t["mnear"])))
        kern.append("mega_gen_kernel" if inr[-1] and t["entries"] >= min_prims else "mega_kernel")
    return dict(tree=t, reach=reach, has_tree=bool(ok), prims_in_lds=bool(t["prims_in_lds"]), in_reach=inr, near=near, kernel=kern)


# the near views that stand inside a sphere: the ball |o - G| <= 2 R + 1 the first camera must lie in is inside a sphere that is the
# whole world, or a giant, or the large end of the line -- (almost) no background to see
GEN_INTERIOR_VIEWS = (("line_2_s0", 0), ("mixed_1_s1", 0), ("mixed_2_s0", 0), ("scales_1000_s1", 0), ("scales_1_s1", 0), ("scales_2_s1", 0),
                      ("scales_3_s1", 0), ("scales_550_s1", 0))
