"""The oracle pinned to the reference's own device code.  oracle/_ref/libmort_ref.so is the reference's .cuh headers
compiled for the CPU through the CUDA-on-host shim (oracle/refshim/, oracle/ref_render.cpp; "pinned" math: the non-IEEE
libm calls go through include/mort_math.h as the oracle and the kernels do).  Every comparison is bit for bit:

  a. renders: uchar4 image, fp32 accumulators and final XORWOW words, two frames per case
  b. per-ray known answers: world::hit's full hit_record, pdf_value, a light's random direction, texture values
  c. the host scene layer: the reference's BVH builder on the same pre-build world as mort_add_bvh
  d. recorded vectors (tests/golden/ref_pin.npz): SHA-256 of the reference build's outputs, so the pin also holds
     where the reference is absent

Where the reference tree exists and the library is missing, the module builds it; it skips only when both are absent.
What this cannot see: cuRAND's seed-scramble constants (restated in the shim), nvcc's contraction, CUDA
libm's last ULP, MSVC's host tan."""
import collections
import ctypes as C
import os

import numpy as np
import pytest

from mort_amd import host, structs as S
from tests import oracle_lib as O, ref_lib as R
from tests.golden.make_golden import REF_PIN_BVH, REF_PIN_CASES, REF_PIN_FRAMES, digest, state_words
from tests.worlds import BVH_BUILDS, BVH_WORLDS, FLAT_WORLDS, custom_bvh_world, flat_camera, flat_world, set_view, world_object_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
PIN_PATH = os.path.join(HERE, "golden", "ref_pin.npz")
COUNTS = collections.Counter()
INF = float("inf")


@pytest.fixture(scope="module")
def ref(request):
    if not R.ensure_built():
        pytest.skip("neither the reference tree nor oracle/_ref/libmort_ref.so is here")
    yield R.lib()
    tr = request.config.pluginmanager.get_plugin("terminalreporter")
    if tr is not None and COUNTS:
        tr.write_line("reference pin cases: " + ", ".join(f"{k} {v}" for k, v in sorted(COUNTS.items())))


# ---------------------------------------------------------------- a. renders

def pin_render(world, cam, frames=2):
    W, H = cam.image_width, cam.image_height
    so = O.seed_states(S.DEFAULT_SEED, W, H)
    sr = R.seed_states(S.DEFAULT_SEED, W, H)
    assert (so["d"] == sr["d"]).all() and (so["v"] == sr["v"]).all(), "setup_rng states differ"
    for f in range(frames):
        o = O.render(world, cam, states=so, nthreads=16, want_segments=False)
        r = R.render(world, cam, states=sr)
        bad = (o["rgba"] != r["rgba"]).any(-1)
        assert not bad.any(), f"frame {f}: uchar4 differs in {int(bad.sum())} pixels, first {np.argwhere(bad)[0]}"
        bad = (o["accum"].view(np.uint32) != r["accum"].view(np.uint32)).any(-1)
        assert not bad.any(), f"frame {f}: fp32 accumulators differ in {int(bad.sum())} pixels, first {np.argwhere(bad)[0]}"
        assert (so["d"] == sr["d"]).all() and (so["v"] == sr["v"]).all(), f"frame {f}: final XORWOW words differ"
    COUNTS["2a renders"] += 1


SCENES = [(1, 64, 4), (2, 48, 4), (3, 48, 4), (4, 48, 4), (5, 32, 9), (6, 32, 9), (7, 32, 9), (8, 24, 4), (9, 32, 4), (10, 64, 4)]


@pytest.mark.parametrize("sid,width,spp", SCENES)
def test_scenes_render_as_the_reference(ref, sid, width, spp):
    pin_render(*host.build_scene(sid, width=width, spp=spp))


@pytest.mark.parametrize("sid", [1, 2, 4])
def test_defocus_cameras_render_as_the_reference(ref, sid):
    """get_ray's defocus-disk branch (camera.cuh:215, vec3.cuh:163-169): no built-in scene opens the aperture."""
    world, cam = host.build_scene(sid, width=48, spp=4)
    cam.defocus_angle = 2.5
    host.lib().mort_camera_initialize(C.byref(cam))
    pin_render(world, cam)


@pytest.mark.parametrize("depth", [0, 1, 2, 50])
def test_bounce_limits_render_as_the_reference(ref, depth):
    pin_render(*host.build_scene(1, width=48, spp=4, depth=depth))


def test_ragged_sizes_and_odd_spp_render_as_the_reference(ref):
    for sid, width, aspect, spp in ((2, 61, 1.7, 5), (6, 37, 1.0, 7), (4, 9, 0.3, 2)):
        pin_render(*host.build_scene(sid, width=width, spp=spp, aspect=aspect))


@pytest.mark.parametrize("name", sorted(FLAT_WORLDS))
def test_flat_worlds_render_as_the_reference(ref, name):
    spec = FLAT_WORLDS[name]
    w, ids = flat_world(spec["prims"], media=spec.get("media", ()), late_list=spec.get("late_list", False))
    light = ids[spec["light"][1]] if spec.get("light") else None
    pin_render(w, flat_camera(light=light, spp=4, width=40))


@pytest.mark.parametrize("name", sorted(BVH_WORLDS))
def test_bvh_worlds_render_as_the_reference(ref, name):
    w = custom_bvh_world(BVH_WORLDS[name])
    _, cam = host.build_scene(1, width=40, spp=4, depth=12)
    set_view(cam, (0.0, 0.6, 1.5), (0.0, 0.0, -1.0), vfov=60, defocus=0.0)
    pin_render(w, cam)


@pytest.mark.parametrize("seed", range(10))
def test_random_worlds_render_as_the_reference(ref, seed):
    from tests.test_host_mode import _random_world
    rng = np.random.default_rng(5000 + seed)
    w, light = _random_world(rng, n_spheres=int(rng.integers(1, 40)), n_quads=int(rng.integers(0, 10)), n_boxes=int(rng.integers(0, 3)),
                             n_media=int(rng.integers(0, 3)), with_light=bool(seed % 2))
    _, cam = host.build_scene(2, width=24, spp=4, depth=int(rng.integers(2, 16)))
    if light:
        cam.light_obj_type, cam.light_obj_idx = light
    views = [((0, 2, 9), (0, 1, 0)), ((0.3, 0.05, 0.2), (4, 0.3, 1)), ((40, 25, -60), (0, 0, 0))]
    for frm, at in views:
        set_view(cam, frm, at, vfov=int(rng.integers(20, 90)), defocus=float(rng.choice([0.0, 0.8])))
        pin_render(w, cam, frames=1 if frm[0] == 40 else 2)


# ---------------------------------------------------------------- b. per-ray known answers

def _points(w):
    """centres of the finite spheres and corners of the quads: where the geometry is"""
    o = w.c.objs
    pts = [list(o.host_sphere[i].center1.e) for i in range(o.num_spheres) if o.host_sphere[i].radius < 500]
    pts += [list(o.host_quad[i].Q.e) for i in range(o.num_quads)]
    return np.array(pts or [[0.0, 0.0, 0.0]], dtype=np.float64)


def _rays(w, rng, n):
    """(origin, direction) rows: random, along the axes (zero components), grazing the spheres, and from far away"""
    pts = _points(w)
    c = np.median(pts, axis=0)
    s = float(np.clip(np.ptp(pts, axis=0).max(), 1.0, 600.0))
    out = []
    k = n // 4
    o = c + s * rng.uniform(-1, 1, (k, 3))
    out += list(zip(o, rng.normal(size=(k, 3))))
    o = c + s * rng.uniform(-1, 1, (k, 3))
    d = np.zeros((k, 3))
    ax = rng.integers(0, 3, k)
    d[np.arange(k), ax] = rng.choice([-1.0, 1.0, 0.37], k)
    two = rng.random(k) < 0.3  # one zero component only
    d[two, (ax[two] + 1) % 3] = rng.uniform(-1, 1, int(two.sum()))
    out += list(zip(o, d))
    sph = [w.c.objs.host_sphere[i] for i in range(w.c.objs.num_spheres)]
    for _ in range(k):
        if sph:
            sp = sph[int(rng.integers(0, len(sph)))]
            cen, r = np.array(sp.center1.e, np.float64), float(sp.radius)
            d = rng.normal(size=3); d /= np.linalg.norm(d)
            perp = np.cross(d, rng.normal(size=3)); perp /= np.linalg.norm(perp)
            dist = float(rng.choice([2.0, 20.0, 200.0])) * max(r, 1.0)
            o = cen - d * dist + perp * r * (1.0 + float(rng.choice([-1e-6, 0.0, 1e-6, -1e-3, 1e-3])))
            out.append((o, d))
        else:
            out.append((c + s * rng.uniform(-1, 1, 3), rng.normal(size=3)))
    for _ in range(n - 3 * k):
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        o = c + u * float(rng.choice([1e3, 1e4, 3e4]))
        tgt = pts[int(rng.integers(0, len(pts)))] + rng.normal(scale=0.5, size=3)
        out.append((o, tgt - o))
    return out


def _hit_fields(h):
    return (list(h.p.e), list(h.normal.e), h.mat_idx, h.mat_type, h.t, h.u, h.v, bool(h.front_face))


def _same_floats(a, b):
    return np.array(a, np.float32).view(np.uint32).tolist() == np.array(b, np.float32).view(np.uint32).tolist()


def _hit_worlds():
    ws = []
    for sid in (1, 2, 3, 4, 5, 6, 7, 9, 10):
        w, cam = host.build_scene(sid, width=16, spp=1)
        ws.append((f"scene{sid}", w, cam, 900 if sid == 9 else 6000))
    for name, spec in sorted(FLAT_WORLDS.items()):
        w, ids = flat_world(spec["prims"], media=spec.get("media", ()), late_list=spec.get("late_list", False))
        light = ids[spec["light"][1]] if spec.get("light") else None
        ws.append((name, w, flat_camera(light=light, spp=1, width=16), 5000))
    for name in sorted(BVH_WORLDS):
        w = custom_bvh_world(BVH_WORLDS[name])
        _, cam = host.build_scene(1, width=16, spp=1)
        ws.append(("bvh_" + name, w, cam, 5000))
    return ws


def _medium_only_materials(w):
    """(mat_type, mat_idx) of the constant media that no sphere or quad outside a medium boundary uses: a world-level
    hit with one of these comes from a medium"""
    o = w.c.objs
    media = {(o.host_constant_medium[i].mat_type, o.host_constant_medium[i].mat_idx) for i in range(o.num_constant_medium)}
    boundary = {(o.host_constant_medium[i].obj_type, o.host_constant_medium[i].obj_idx) for i in range(o.num_constant_medium)}
    # the boundaries of the media: their skip primitives, reached through lists / instances (rotated smoke boxes)
    stack, seen = list(boundary), set()
    while stack:
        t, i = stack.pop()
        if (t, i) in seen:
            continue
        seen.add((t, i))
        if t in (S.OBJ_TRANSLATE, S.OBJ_ROTATE_Y):
            x = o.host_translate[i] if t == S.OBJ_TRANSLATE else o.host_rotate_y[i]
            stack.append((x.obj_type, x.obj_idx))
        elif t == S.OBJ_HITTABLE_LIST:
            x = o.host_hittable_list[i]
            stack += [(x.obj_types[k], x.obj_idxs[k]) for k in range(x.num_objs)]
    used = {(x.mat_type, x.mat_idx) for k in range(o.num_spheres) for x in [o.host_sphere[k]] if (S.OBJ_SPHERE, k) not in seen}
    used |= {(x.mat_type, x.mat_idx) for k in range(o.num_quads) for x in [o.host_quad[k]] if (S.OBJ_QUAD, k) not in seen}
    return media - used


def test_world_hit_pdf_and_light_sampling_per_ray(ref):
    """world::hit for every field of the hit record (t p normal u v front_face mat) and the stream it leaves behind; then
    pdf_value and a light's random() (same draws) from the hit points and random origins."""
    OL = O.lib()
    rng = np.random.default_rng(77)
    r7 = (C.c_float * 7)()
    so, sr = S.RngState(), S.RngState()
    OL.mort_oracle_rng_init(so, 123, 0)
    ho, hr = O.Hit(), O.Hit()
    rays = hits = pdfs = media = 0
    for name, w, cam, n in _hit_worlds():
        R.load(w)
        media_mats = _medium_only_materials(w)
        for o, d in _rays(w, rng, n):
            r7[:] = [*np.float32(o), *np.float32(d), float(np.float32(rng.random()))]
            for tmax in (INF, float(np.float32(rng.uniform(0.5, 50.0)))):
                C.memmove(C.byref(sr), C.byref(so), C.sizeof(so))
                a = OL.mort_oracle_world_hit(w.ptr, r7, 0.001, tmax, so, ho)
                b = ref.mort_ref_world_hit(r7, 0.001, tmax, sr, hr)
                assert a == b, (name, list(r7), tmax)
                if a:
                    fa, fb = _hit_fields(ho), _hit_fields(hr)
                    # a constant_medium hit leaves u, v as the record held them (objects.cuh:425-431): indeterminate in
                    # the reference, 0 in the oracle and the kernels.  Told apart by its material, which
                    # nothing but media carries; every other field is compared, and the oracle's u, v must be 0.
                    medium = (fa[3], fa[2]) in media_mats
                    if medium:
                        assert fa[5:7] == (0.0, 0.0) and fb[1] == [1.0, 0.0, 0.0] and fb[7], (name, list(r7), fa, fb)
                    n_uv = 1 if medium else 3
                    assert _same_floats(fa[0] + fa[1] + list(fa[4:4 + n_uv]), fb[0] + fb[1] + list(fb[4:4 + n_uv])) and \
                        fa[2:4] == fb[2:4] and fa[7] == fb[7], (name, list(r7), tmax, fa, fb)
                    hits += 1
                    media += medium
                assert so.d == sr.d and list(so.v) == list(sr.v), (name, list(r7), "stream")
                rays += 1
        if cam.light_obj_type > 0:
            lt, li = cam.light_obj_type, cam.light_obj_idx
            for o, d in _rays(w, rng, 400):
                org = (C.c_float * 3)(*np.float32(o))
                dr = (C.c_float * 3)(*np.float32(d))
                assert _same_floats([OL.mort_oracle_pdf_value(w.ptr, lt, li, org, dr)], [ref.mort_ref_pdf_value(lt, li, org, dr)]), (name, list(org), list(dr))
                C.memmove(C.byref(sr), C.byref(so), C.sizeof(so))
                da, db = (C.c_float * 3)(), (C.c_float * 3)()
                OL.mort_oracle_light_random(w.ptr, lt, li, org, so, da)
                assert ref.mort_ref_light_random(lt, li, org, sr, db) == 0
                assert _same_floats(list(da), list(db)) and so.d == sr.d and list(so.v) == list(sr.v), (name, list(org))
                # the pdf of the direction the light sampled: a hit by construction
                assert _same_floats([OL.mort_oracle_pdf_value(w.ptr, lt, li, org, da)], [ref.mort_ref_pdf_value(lt, li, org, da)])
                pdfs += 2
    COUNTS["2b rays"] += rays
    COUNTS["2b hits"] += hits
    COUNTS["2b of them medium hits"] += media
    COUNTS["2b pdf / light samples"] += pdfs
    assert rays >= 100000 and hits > rays // 10


def test_texture_values(ref):
    """Every texture kind at the edges: u = 1 and v = 0 of the image (clamped texel reads), negative checker cells,
    Perlin noise at large |p|."""
    OL = O.lib()
    rng = np.random.default_rng(9)
    worlds = [host.build_scene(3)[0], host.build_scene(4)[0], custom_bvh_world(BVH_WORLDS["every_material"])]
    uv = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.5, 0.0), (1.0, 0.5), (-0.2, 1.3), (0.99999994, 1e-8)] + \
         [tuple(x) for x in rng.uniform(0, 1, (200, 2))]
    pts = [(0.0, 0.0, 0.0), (-0.1, -0.1, -0.1), (-3.3, 0.2, -7.9), (1e3, -1e3, 5e2), (-2e4, 3e4, 1e4), (3e4, 3e4, -3e4)] + \
          [tuple(x) for x in rng.uniform(-50, 50, (200, 3))] + [tuple(x) for x in rng.uniform(-3e4, 3e4, (100, 3))]
    out_o, out_r = (C.c_float * 3)(), (C.c_float * 3)()
    n = 0
    for w in worlds:
        R.load(w)
        t = w.c.texs
        kinds = [(S.TEXTURE_SOLID, t.num_solid_colors), (S.TEXTURE_CHECKER, t.num_checker_textures),
                 (S.TEXTURE_IMAGE, t.num_image_textures), (S.TEXTURE_NOISE, t.num_noise_textures)]
        for tt, count in kinds:
            for ti in range(count):
                for k, p in enumerate(pts):
                    u, v = uv[k % len(uv)]
                    pf = (C.c_float * 3)(*p)
                    OL.mort_oracle_texture_value(w.ptr, tt, ti, u, v, pf, out_o)
                    assert ref.mort_ref_texture_value(tt, ti, u, v, pf, out_r) == 0
                    assert _same_floats(list(out_o), list(out_r)), (tt, ti, u, v, p, list(out_o), list(out_r))
                    n += 1
                for u, v in uv:
                    pf = (C.c_float * 3)(*pts[2])
                    OL.mort_oracle_texture_value(w.ptr, tt, ti, u, v, pf, out_o)
                    assert ref.mort_ref_texture_value(tt, ti, u, v, pf, out_r) == 0
                    assert _same_floats(list(out_o), list(out_r)), (tt, ti, u, v)
                    n += 1
    COUNTS["2b texture values"] += n


def test_camera_rays_and_ray_color(ref):
    """get_ray (stratified offset, defocus disk, time) and ray_color one sample at a time from the same stream"""
    OL = O.lib()
    r7o, r7r, co, cr = (C.c_float * 7)(), (C.c_float * 7)(), (C.c_float * 3)(), (C.c_float * 3)()
    so, sr = S.RngState(), S.RngState()
    OL.mort_oracle_rng_init(so, 42, 0)
    n = 0
    for sid, defocus in ((1, 0.0), (2, 3.0), (6, 0.0), (7, 0.0)):
        w, cam = host.build_scene(sid, width=32, spp=9)
        cam.defocus_angle = defocus
        host.lib().mort_camera_initialize(C.byref(cam))
        R.load(w)
        for y in range(0, cam.image_height, 3):
            for x in range(0, cam.image_width, 3):
                C.memmove(C.byref(sr), C.byref(so), C.sizeof(so))
                OL.mort_oracle_get_ray(C.byref(cam), x, y, x % 3, y % 3, so, r7o)
                ref.mort_ref_get_ray(C.byref(cam), x, y, x % 3, y % 3, sr, r7r)
                assert _same_floats(list(r7o), list(r7r)), (sid, x, y)
                OL.mort_oracle_ray_color(w.ptr, C.byref(cam), r7o, so, co)
                assert ref.mort_ref_ray_color(C.byref(cam), r7r, sr, cr) == 0
                assert _same_floats(list(co), list(cr)) and so.d == sr.d and list(so.v) == list(sr.v), (sid, x, y)
                n += 1
    COUNTS["2b camera rays"] += n


def test_get_ray_records_as_the_reference(ref):
    """2^12 of the camera sweep's get_ray records (tests/camera_cases.py: offsets of exactly 0 and 1, disk points on the unit circle, pixels
    past 2^24, sqrt_spp of 0 and 32768, defocus angles of -0, inf and NaN, non-finite cameras) through the reference's own get_ray: the ray
    and the stream it leaves equal the oracle's, bit for bit"""
    from tests import camera_cases as CC
    rec = CC.pin_ray_records()
    want = O.camera_batch(0, rec)
    got = np.zeros_like(want)
    got[:, 13] = want[:, 13]  # the reference does not count its draws: the stream words tell
    cam, st, r7 = S.Camera(), S.RngState(), (C.c_float * 7)()
    f = rec[:, 10:].view(np.float32)
    for i in range(len(rec)):
        st.d = int(rec[i, 0])
        for k in range(5):
            st.v[k] = int(rec[i, 1 + k])
        cam.recip_sqrt_spp, cam.defocus_angle = f[i, 0], f[i, 1]
        for j, name in enumerate(("center", "pixel00_loc", "pixel_delta_u", "pixel_delta_v", "defocus_disk_u", "defocus_disk_v")):
            getattr(cam, name).e[:] = f[i, 2 + 3 * j: 5 + 3 * j].tolist()
        x, y, s_i, s_j = (int(v) for v in rec[i, 6:10].view(np.int32))
        ref.mort_ref_get_ray(C.byref(cam), x, y, s_i, s_j, st, r7)
        got[i, 0:7] = np.array(list(r7), np.float32).view(np.uint32)
        got[i, 7] = st.d
        got[i, 8:13] = list(st.v)
    cen = CC.ray_census(rec, want)
    assert min(cen["no_disk"], cen["accepted_first"], cen["rejected_once"], cen["rejected_more"]) >= 50 and cen["nonfinite"] >= 40, cen
    assert min(cen["px_zero"], cen["px_one"], cen["py_zero"], cen["py_one"]) >= 1, cen
    CC.assert_same(0, rec, dict(oracle=want, reference=got))
    COUNTS["2b get_ray records"] += len(rec)


def test_pixel_tail_records_as_the_reference(ref):
    """The end of Camera::render is not callable alone: 1 x 1 frames of an empty world, whose every sample returns the background, hand it
    sqrt_spp^2 x background.  2048 cases (tests/camera_cases.py pin_pixel_cases) with sqrt_spp in 1, 2, 3; a case is kept where the fp32
    additions of the background reproduce the intended sum exactly, which at least half must; the kept ones equal the oracle's tail over
    (pixel_samples_scale, sum): the uchar4 of the reference's own render, and the accumulator."""
    from tests import camera_cases as CC
    rows = CC.pin_pixel_cases()
    empty = host.World()
    R.load(empty)
    _, cam = host.build_scene(2, width=1, spp=1, aspect=1.0)
    assert cam.image_width == 1 and cam.image_height == 1
    rec = np.zeros((len(rows), 4), np.float32)
    got = np.zeros((len(rows), 4), np.uint32)
    keep = np.zeros(len(rows), bool)
    rgba, accum = np.zeros(4, np.uint8), np.zeros(3, np.float32)
    with np.errstate(all="ignore"):
        for i, (n, *b) in enumerate(rows):
            n = int(n)
            b = np.array(b, np.float32)
            total = np.zeros(3, np.float32)
            for _ in range(n * n):
                total = total + b
            intended = (b.astype(np.float64) * (n * n)).astype(np.float32)
            keep[i] = bool(((total.view(np.uint32) == intended.view(np.uint32)) & ((b.astype(np.float64) * (n * n)) == intended)).all())
            cam.samples_per_pixel = n * n
            host.lib().mort_camera_initialize(C.byref(cam))
            cam.background.e[:] = b.tolist()
            rec[i, 0] = cam.pixel_samples_scale
            rec[i, 1:4] = total
            st = O.seed_states(S.DEFAULT_SEED, 1, 1)
            assert ref.mort_ref_render(C.byref(cam), st.ctypes.data, 0, 1, rgba.ctypes.data, accum.ctypes.data, 1) == 0
            got[i, 0:3] = accum.view(np.uint32)
            got[i, 3] = rgba.view(np.uint32)[0]
    assert keep.sum() * 2 >= len(rows), int(keep.sum())
    rec, got = rec[keep], got[keep]
    want = O.camera_batch(2, rec.view(np.uint32))
    prod = rec[:, 0:1] * rec[:, 1:4]
    assert (prod < 0).any() and (prod == np.float32(-0.5)).any() and np.isinf(prod).any() and len(np.unique(want[:, 3] & 0xff)) >= 200
    CC.assert_same(2, rec.view(np.uint32), dict(oracle=want, reference=got))
    COUNTS["2b pixel tails"] += len(rec)


def _shade_cases():
    from tests import shade_cases as SC
    return [(w, s) for w in SC.WORLDS for s in SC.LIGHT_SETTINGS]


def _undefined_int_conversion(world, rays7, streams):
    """per ray: does the closest hit evaluate a texture whose (int)floorf(...) is out of int's range or a NaN?  The reference converts with a
    plain cast (textures.cuh:54-56,183-185,347), which the device defines (saturation, NaN -> 0: mort_f2i, the oracle's form) and C++ on
    the host leaves undefined: there the reference compiled for the CPU is not the reference.  True for a hit on a textured material at a
    non-finite point, or on a checker whose 1 / scale carries every finite point out of range (scale 0, 1e-30 or NaN)."""
    st = streams.copy()
    h, hit = O.world_hit_batch(world, rays7, 0.001, np.inf, states=st)
    m, t = world.c.mats, world.c.texs
    tables = {S.MAT_LAMBERTIAN: m.host_lambertian, S.MAT_DIFFUSE_LIGHT: m.host_diffuse_light, S.MAT_ISOTROPIC: m.host_isotropic}
    out = np.zeros(len(rays7), bool)
    for i in np.flatnonzero(hit):
        tab = tables.get(int(h["mat_type"][i]))
        if tab is None:
            continue
        tex = tab[int(h["mat_idx"][i])]
        wild = tex.texType == S.TEXTURE_CHECKER and not abs(t.host_checker_texture[tex.texIdx].inv_scale) < 1e6
        out[i] = wild or not np.isfinite(h["p"][i]).all() or (tex.texType not in (S.TEXTURE_SOLID, S.TEXTURE_CHECKER, S.TEXTURE_NOISE) and not np.isfinite((h["u"][i], h["v"][i])).all())
    return out


@pytest.mark.parametrize("world_name,setting", _shade_cases())
def test_shade_sweep_records_as_two_segment_paths(ref, world_name, setting):
    """the records of the shade-step sweep (tests/shade_cases.py: edge refraction indices, fuzz and albedos, unknown tags, zero and negative
    radii, rays at the critical angle, non-finite rays) as two-segment paths through the reference's own ray_color, bounce limit 2: colour
    and final stream words against the oracle's ray_color, whose loop body is the function mort_oracle_shade_batch runs.  2048 records
    of each of the nine (world, light setting) pairs, so that more than 2^14 are compared.  A path whose first or second hit converts a float outside int's range with a plain cast
    (_undefined_int_conversion) is left out of the comparison: at least 85 % of the records remain."""
    from tests import radiance_ref as RR
    from tests import shade_cases as SC
    from tests.query_rays import _words
    sw = SC.shade_world(world_name)
    rec, _ = SC.records(world_name, setting)
    n = 2048
    rec = np.array(rec[np.sort(np.random.default_rng(14).choice(len(rec), n, replace=False))])
    rec[:, 13] = rec[:, 12]  # ray_color scatters with the time of the ray it is given
    _, cam = host.build_scene(2, width=8, spp=1, depth=2)
    cam.background.e[0], cam.background.e[1], cam.background.e[2] = 0.30, 0.35, 0.45
    cam.light_obj_type, cam.light_obj_idx = sw.lights[setting]
    rays = np.zeros((n, 8), np.float32)
    rays[:, :7] = rec[:, 6:13].view(np.float32); rays[:, 7] = np.inf
    streams0 = np.zeros(n, O.STATE_DTYPE)
    streams0["d"] = rec[:, 0]; streams0["v"] = rec[:, 1:6]
    streams = streams0.copy()
    want = RR.oracle_radiance(sw.world, cam, rays, streams, 1)
    first, _ = O.shade_batch(sw.world, rec)
    mid = np.zeros(n, O.STATE_DTYPE)
    mid["d"] = first[:, 15]; mid["v"] = first[:, 16:21]
    left_out = _undefined_int_conversion(sw.world, rays[:, :7], streams0) | \
        ((first[:, 0] >= 2) & _undefined_int_conversion(sw.world, np.ascontiguousarray(first[:, 8:15].view(np.float32)), mid))
    assert left_out.mean() <= 0.15, float(left_out.mean())
    R.load(sw.world)
    r7, cr, sr = (C.c_float * 7)(), (C.c_float * 3)(), S.RngState()
    got = np.zeros((n, 3), np.float32)
    for i in np.flatnonzero(~left_out):
        r7[:] = rays[i, :7].tolist()
        sr.d = int(rec[i, 0])
        for k in range(5):
            sr.v[k] = int(rec[i, 1 + k])
        assert ref.mort_ref_ray_color(C.byref(cam), r7, sr, cr) == 0
        got[i] = list(cr)
        assert sr.d == streams["d"][i] and list(sr.v) == streams["v"][i].tolist(), (world_name, setting, i)
    bad = np.flatnonzero((_words(got) != _words(want)).any(1) & ~left_out)
    assert bad.size == 0, f"{world_name} {setting}: {bad.size} of {n} colours differ, first {bad[0]}: reference {got[bad[0]]} oracle {want[bad[0]]}"
    COUNTS["2b shade sweep records"] += int((~left_out).sum())
    COUNTS["2b of them left out: an int conversion C++ leaves undefined"] += int(left_out.sum())


MATERIAL_PINS = [("ior_edges", "flat", 12), ("unknown_tags", "bvh", 12), ("mirror_hall", "bvh", 64)]


@pytest.mark.parametrize("key", MATERIAL_PINS, ids=["-".join(map(str, k)) for k in MATERIAL_PINS])
def test_material_worlds_render_as_the_reference(ref, key):
    """three of MATERIAL_WORLDS (tests/material_worlds.py), small: the edge refraction indices, the tags outside the known set, and the
    closed hall of mirrors at the bounce limit's maximum"""
    from tests import material_worlds as M
    cam = M.camera(key[0], key[2])
    small = M._camera(dict(M.MATERIAL_WORLDS[key[0]], width=32), key[2])
    assert small.image_width < cam.image_width
    pin_render(M.material_world(key[0], key[1]), small, frames=1)


# ---------------------------------------------------------------- c. the host scene layer: BVH build

@pytest.mark.parametrize("hierarchy", [0, 1])
@pytest.mark.parametrize("name", sorted(BVH_BUILDS))
def test_bvh_build_leaves_the_reference_world(ref, name, hierarchy):
    """mort_add_bvh's stable insertion sort and leaf order against the reference's bubble sort (which swaps the objects
    themselves between same-type neighbours and the list entries otherwise) and two-object leaf rule, on the same
    pre-build world; with `hierarchy`, the reference's build_aabb_hierarchy recomputes the boxes afterwards."""
    wm, li = BVH_BUILDS[name]()
    wr, li2 = BVH_BUILDS[name]()
    assert world_object_bytes(wm) == world_object_bytes(wr)
    assert host.lib().mort_add_bvh(wm.ptr, li, False) == 0
    assert ref.mort_ref_add_bvh(wr.ptr, li2, False, hierarchy) == 0
    a, b = world_object_bytes(wm), world_object_bytes(wr)
    if a != b:
        i = next(k for k in range(min(len(a), len(b))) if a[k] != b[k])
        pytest.fail(f"world bytes differ from byte {i} of {len(a)}")
    COUNTS["2c BVH builds"] += 1


# ---------------------------------------------------------------- d. recorded vectors

def _render_digests(render, name):
    sid, width, spp, depth = REF_PIN_CASES[name]
    world, cam = host.build_scene(sid, width=width, spp=spp, depth=depth)
    out = []
    st = None
    for f in range(REF_PIN_FRAMES):
        r = render(world, cam, st)
        st = r["states"]
        out.append([digest(r["rgba"]), digest(r["accum"]), digest(state_words(st))])
    return out


@pytest.mark.parametrize("name", sorted(REF_PIN_CASES))
def test_oracle_matches_the_recorded_reference(name):
    """holds where the reference is absent: the oracle's frames hash to what the reference build rendered"""
    got = _render_digests(lambda w, c, st: O.render(w, c, states=st, nthreads=16, want_segments=False), name)
    for f, g in enumerate(got):
        assert g == np.load(PIN_PATH)[f"{name}_f{f}"].tolist(), f"frame {f}: [rgba, accum, states] digests differ"


@pytest.mark.parametrize("name", REF_PIN_BVH)
def test_bvh_build_matches_the_recorded_reference(name):
    w, li = BVH_BUILDS[name]()
    assert host.lib().mort_add_bvh(w.ptr, li, False) == 0
    assert digest(np.frombuffer(world_object_bytes(w), np.uint8)) == np.load(PIN_PATH)["bvh_" + name][0]


@pytest.mark.parametrize("name", sorted(REF_PIN_CASES))
def test_reference_build_matches_its_record(ref, name):
    """the live reference build still renders what was recorded (the record is not stale)"""
    got = _render_digests(lambda w, c, st: R.render(w, c, states=st), name)
    for f, g in enumerate(got):
        assert g == np.load(PIN_PATH)[f"{name}_f{f}"].tolist()
    COUNTS["2d recorded cases"] += 1


@pytest.mark.parametrize("world_name", ["bvh", "flat"])
def test_light_sampling_records(ref, world_name):
    """pdfValueDispatch / randomDispatch over the light sweep's worlds (tests/light_cases.py): 2^14 records per function from the same
    builder as the 2^20 the kernels run, so every family is there whole -- origins inside a sphere, in a quad's plane, at the centre, at
    Q; degenerate primitives; lists of 1, 3, 40 and 500 members with members that sample nothing; random_int one past the list -- where
    the oracle's restatement could have drifted from the reference unnoticed.  The pdf, the direction and the final stream words."""
    from tests import light_cases as LC
    world, _ = LC.WORLDS[world_name]()
    R.load(world)
    rec, lab = LC.pin_records(world_name, 0)
    want = O.light_batch(world, 0, rec)[:, 0]
    got = np.empty(len(rec), np.float32)
    f = rec[:, 2:].view(np.float32)
    for i in range(len(rec)):
        got[i] = ref.mort_ref_pdf_value(int(lab["type"][i]), int(lab["idx"][i]), (C.c_float * 3)(*f[i, :3]), (C.c_float * 3)(*f[i, 3:]))
    assert np.isnan(got).sum() > 1000 and np.isinf(got).sum() > 100 and (got == 0).sum() > 1000  # the edges are in the sample
    LC.assert_same(0, rec, dict(oracle=want.reshape(-1, 1), reference=got.view(np.uint32).reshape(-1, 1)))
    rec, lab = LC.pin_records(world_name, 1)
    want = O.light_batch(world, 1, rec)
    got = np.zeros((len(rec), 10), np.uint32)
    got[:, 9] = want[:, 9]  # the reference does not count its draws: the stream words tell
    st, d = S.RngState(), (C.c_float * 3)()
    f = rec[:, 8:].view(np.float32)
    for i in range(len(rec)):
        st.d = int(rec[i, 0])
        for k in range(5):
            st.v[k] = int(rec[i, 1 + k])
        assert ref.mort_ref_light_random(int(lab["type"][i]), int(lab["idx"][i]), (C.c_float * 3)(*f[i]), st, d) == 0
        got[i, :3] = np.array(list(d), np.float32).view(np.uint32)
        got[i, 3] = st.d
        got[i, 4:9] = list(st.v)
    past = [int((want[(lab["type"] == S.OBJ_HITTABLE_LIST) & (lab["idx"] == li), 9] == 1).sum()) for li in (0, 1)]
    LC.assert_same(1, rec, dict(oracle=want, reference=got))
    COUNTS["2b light sweep records"] += 2 * len(rec)
    COUNTS["2b of them random_int one past a list of primitives"] += past[0] if world_name == "bvh" else 0


def test_entry_points_refuse_without_a_loaded_world(ref):
    """a BVH build leaves the reference's host arrays unlike the uploaded world: until the next load the per-ray entry
    points answer with an error and touch nothing"""
    w, li = BVH_BUILDS["three_spheres"]()
    assert ref.mort_ref_add_bvh(w.ptr, li, False, 0) == 0
    r7, hit, st, out = (C.c_float * 7)(0, 0, 5, 0, 0, -1, 0), O.Hit(), S.RngState(), (C.c_float * 3)()
    p = (C.c_float * 3)(0, 0, 5)
    _, cam = host.build_scene(2, width=16, spp=1)
    assert not ref.mort_ref_world_hit(r7, 0.001, INF, st, hit)
    assert ref.mort_ref_ray_color(C.byref(cam), r7, st, out) == -1
    assert ref.mort_ref_texture_value(S.TEXTURE_SOLID, 0, 0.0, 0.0, p, out) == -1
    assert ref.mort_ref_light_random(S.OBJ_SPHERE, 0, p, st, out) == -1
    assert np.isnan(ref.mort_ref_pdf_value(S.OBJ_SPHERE, 0, p, p))
    assert ref.mort_ref_render(C.byref(cam), np.zeros(16 * 9, O.STATE_DTYPE).ctypes.data, 0, 9,
                               np.zeros(16 * 9 * 4, np.uint8).ctypes.data, None, 1) == -1
    R.load(w)
    assert ref.mort_ref_world_hit(r7, 0.001, INF, st, hit)


def test_ref_distance_script_output(ref):
    """scripts/ref_distance.py (native libm / nvcc-style contraction against the oracle) at a tiny size:
    the shape of its output only -- the numbers are measurements, not bounds"""
    import json
    import subprocess
    import sys
    assert R.ensure_built("native") and R.ensure_built("fma")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(HERE), "scripts", "ref_distance.py"), "--tiny"],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert sorted(out) == ["scene1_1200x675x4", "scene6_400x400x16"]
    for row in out.values():
        for mode in ("native", "fma"):
            assert sorted(row[mode]) == ["accum_rmse", "divergent_pixel_share", "max_byte_diff"]
            assert 0.0 <= row[mode]["divergent_pixel_share"] <= 1.0 and row[mode]["accum_rmse"] >= 0.0 and 0 <= row[mode]["max_byte_diff"] <= 255
