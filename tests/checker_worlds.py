"""Worlds for the checker lookups (tests/test_gpu_shade_parts.py)."""
import ctypes as C

from mort_amd import host, structs as S


def nested_checker_world(width=64, spp=4):
    """One reference BVH over spheres whose Lambertians read: a checker of two checkers (ground), a checker of a checker and a solid, a
    checker of a noise texture and a solid, a plain checker of two solids, a solid; and a light whose emission is a checker.
    Checker records in order: 0 plain_a (solid, solid), 1 plain_b (solid, solid), 2 both (checker, checker), 3 one (checker, solid),
    4 noisy (noise, solid), 5 lit (solid, solid) -- NESTED_RECORDS below.  Returns (world, camera)."""
    L = host.lib()
    w = host.World()
    lst = L.mort_add_hittable_list(w.ptr, True)
    sol = lambda r, g, b: L.mort_add_solid_color(w.ptr, host.vec3(r, g, b))
    ck = lambda scale, te, ie, to, io: L.mort_add_checker_texture(w.ptr, scale, te, ie, to, io)
    SOL, CK, NZ = S.TEXTURE_SOLID, S.TEXTURE_CHECKER, S.TEXTURE_NOISE
    plain_a = ck(0.32, SOL, sol(.2, .3, .1), SOL, sol(.9, .9, .9))
    plain_b = ck(0.11, SOL, sol(.8, .1, .1), SOL, sol(.1, .1, .8))
    both = ck(1.3, CK, plain_a, CK, plain_b)
    one = ck(0.5, CK, plain_b, SOL, sol(.9, .8, .2))
    g = S.HostRng(); L.mort_host_rng_init(C.byref(g), 3, 0)
    noisy = ck(0.4, NZ, L.mort_add_noise_texture(w.ptr, 4.0, C.byref(g)), SOL, sol(.3, .7, .4))
    lit = ck(0.2, SOL, sol(4, 4, 4), SOL, sol(.5, 2, 4))
    lamb = lambda t, i: (S.MAT_LAMBERTIAN, L.mort_add_lambertian(w.ptr, t, i))
    mats = [((0, -100.5, -1), 100, lamb(CK, both)), ((-1.6, 0, -1.2), 0.5, lamb(CK, one)), ((-0.5, 0, -1.0), 0.5, lamb(CK, noisy)),
            ((0.6, 0, -1.0), 0.5, lamb(CK, plain_a)), ((1.7, 0, -1.3), 0.5, lamb(SOL, sol(.7, .3, .3))),
            ((0, 1.4, -1.5), 0.4, (S.MAT_DIFFUSE_LIGHT, L.mort_add_diffuse_light(w.ptr, CK, lit))),
            ((0.1, -0.2, -0.2), 0.25, (S.MAT_DIELECTRIC, L.mort_add_dielectric(w.ptr, 1.5))),
            ((-1.0, -0.25, -0.3), 0.2, (S.MAT_METAL, L.mort_add_metal(w.ptr, host.vec3(.8, .8, .8), 0.1)))]
    for centre, radius, (mt, mi) in mats:
        L.mort_list_add(w.ptr, lst, S.OBJ_SPHERE, L.mort_add_sphere(w.ptr, host.vec3(*centre), radius, mt, mi, True))
    L.mort_add_bvh(w.ptr, lst, False)
    w.c.bvh_mode = True
    _, cam = host.build_scene(1, width=width, spp=spp, depth=12)
    for i, v in enumerate((0.0, 0.6, 1.5)): cam.lookfrom.e[i] = v
    for i, v in enumerate((0.0, 0.0, -1.0)): cam.lookat.e[i] = v
    cam.vfov = 60; cam.defocus_angle = 0.0
    L.mort_camera_initialize(C.byref(cam))
    return w, cam


NESTED_RECORDS = [  # (by_value, even colour, odd colour) of nested_checker_world's records, in order
    (1, (.2, .3, .1), (.9, .9, .9)), (1, (.8, .1, .1), (.1, .1, .8)), (0, None, None), (0, None, None), (0, None, None), (1, (4, 4, 4), (.5, 2, 4))]
