"""The oracle side of the radiance-query tests (tests/test_radiance_host.py, tests/test_gpu_radiance.py).

The reference is mort_oracle_ray_color alone: for each ray it is called `samples` times from the ray's stream and the colours
are summed in numpy float32 as the contract writes the sum, ((0 + c_1) + c_2) + ...  The camera carries the parameters (bounce
limit, background, light object).  The rays are the primary, secondary, far and axis sets of tests/query_rays.py (its interval
set re-issues rays of the first two with other t_max, which a radiance query ignores).  reference() caches one answer per
(world, parameters) per process, and nothing may change it."""
import ctypes as C
import functools

import numpy as np

from mort_amd import hip, structs as S
from tests import oracle_lib as O
from tests import query_rays as Q
from tests import worlds as Wd

F = np.float32
SETS = ("primary", "secondary", "far", "axis")


def copy_camera(cam, bounce_limit=None, light=None, background=None):
    """the camera with other radiance parameters; light: None = the camera's own, else (type, idx), (-1, 0) = none"""
    c = type(cam).from_buffer_copy(cam)
    if bounce_limit is not None:
        c.bounce_limit = bounce_limit
    if light is not None:
        c.light_obj_type, c.light_obj_idx = light
    if background is not None:
        for k in range(3):
            c.background.e[k] = background[k]
    return c


def world_light(name):
    """the light object of a lit world: the scene camera's own, or the primitive a FLAT_WORLDS entry names; None without one"""
    if name.startswith("flat:"):
        spec = Wd.FLAT_WORLDS[name[5:]]
        if "light" not in spec:
            return None
        _, ids = Wd.flat_world(spec["prims"], media=spec.get("media", ()), late_list=spec.get("late_list", False))
        return ids[spec["light"][1]]
    cam = Q.build(name).cam
    return (cam.light_obj_type, cam.light_obj_idx) if cam.light_obj_type != -1 else None


def oracle_radiance(world, cam, rays, states, samples=1):
    """rgb float32 (n, 3); states (O.STATE_DTYPE, n) are advanced in place"""
    L = O.lib()
    fp, sp = C.POINTER(C.c_float), C.POINTER(S.RngState)
    r7 = np.ascontiguousarray(np.asarray(rays, dtype=F).reshape(-1, 8)[:, :7])
    n = r7.shape[0]
    assert states.dtype == O.STATE_DTYPE and states.shape == (n,) and states.flags.c_contiguous
    out = np.zeros((n, 3), dtype=F)
    rgb = np.zeros(3, dtype=F)
    rgb_p, cam_p, r0, s0 = rgb.ctypes.data_as(fp), C.byref(cam), r7.ctypes.data, states.ctypes.data
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            acc = np.zeros(3, dtype=F)
            ray_p, st_p = C.cast(r0 + 28 * i, fp), C.cast(s0 + 48 * i, sp)
            for _ in range(samples):
                L.mort_oracle_ray_color(world.ptr, cam_p, ray_p, st_p, rgb_p)
                acc = acc + rgb
            out[i] = acc
    return out


class Ref:
    """rays (n, 8), streams0 / streams (before / after), rgb (n, 3), advanced bool (n,), slices per set, params"""


@functools.lru_cache(maxsize=None)
def rays_of(name):
    """(rays (n, 8), streams0 (n,), slices): the four sets of the world, one stream per ray"""
    s = Q.build(name)
    rays = np.concatenate([s.all[s.slices[k]] for k in SETS])
    slices, at = {}, 0
    for k in SETS:
        m = s.slices[k].stop - s.slices[k].start
        slices[k] = slice(at, at + m); at += m
    streams0 = Q.some_streams(len(rays))
    rays.setflags(write=False); streams0.setflags(write=False)
    return rays, streams0, slices


@functools.lru_cache(maxsize=None)
def reference(name, samples=1, bounce_limit=None, light=None, background=None, sets=SETS):
    """the oracle's answer for the world's rays (of `sets`) under the camera's parameters, or the ones given"""
    s = Q.build(name)
    rays, streams0, slices = rays_of(name)
    idx = np.concatenate([np.arange(slices[k].start, slices[k].stop) for k in sets])
    r = Ref()
    r.name, r.world = name, s.world
    r.cam = copy_camera(s.cam, bounce_limit, light, background)
    r.params = hip.radiance_params_from_camera(r.cam, samples)
    r.rays = np.ascontiguousarray(rays[idx])
    r.streams0 = np.ascontiguousarray(streams0[idx])
    r.streams = r.streams0.copy()
    r.rgb = oracle_radiance(s.world, r.cam, r.rays, r.streams, samples)
    r.advanced = (r.streams.view(np.uint8).reshape(-1, 48) != r.streams0.view(np.uint8).reshape(-1, 48)).any(1)
    r.slices, at = {}, 0
    for k in sets:
        m = slices[k].stop - slices[k].start
        r.slices[k] = slice(at, at + m); at += m
    for a in (r.rays, r.streams0, r.streams, r.rgb, r.advanced):
        a.setflags(write=False)
    return r


def assert_equal(rgb, streams, ref, what, idx=None):
    """a query's colours and final streams against the oracle's: raw 32-bit words with any NaN equal to any NaN (Q._words), and
    all 48 bytes of every stream"""
    want_rgb, want_st, rays = ref.rgb, ref.streams, ref.rays
    if idx is not None:
        want_rgb, want_st, rays = want_rgb[idx], np.ascontiguousarray(want_st[idx]), rays[idx]
    assert rgb.shape == want_rgb.shape, what
    bad = np.flatnonzero((Q._words(rgb) != Q._words(want_rgb)).any(1))
    assert bad.size == 0, f"{what}: colour differs for {bad.size} of {len(want_rgb)} rays, first {bad[0]}: ray {rays[bad[0]]} got {rgb[bad[0]]} oracle {want_rgb[bad[0]]}"
    a, b = streams.view(np.uint8).reshape(-1, 48), want_st.view(np.uint8).reshape(-1, 48)
    bad = np.flatnonzero((a != b).any(1))
    assert bad.size == 0, f"{what}: final stream differs for {bad.size} rays, first {bad[0]}: ray {rays[bad[0]]}"


def two_sets(ref):
    """the primary and secondary rays: what the census figures are shares of"""
    return slice(ref.slices["primary"].start, ref.slices["secondary"].stop)


def census(name):
    """The sets show something, asserted on the oracle's answers alone.  Returns the figures."""
    out = {}
    r = reference(name)
    ps = two_sets(r)
    rgb = r.rgb[ps]
    bg = np.array([r.cam.background.e[k] for k in range(3)], dtype=F)
    with np.errstate(invalid="ignore"):
        plain = (rgb == bg).all(1) | (rgb == 0).all(1)
    out["coloured"] = float((~plain).mean())
    out["advanced"] = float(r.advanced[ps].mean())
    out["advanced_rays"] = int(r.advanced[ps].sum())
    out["nan"] = float(np.isnan(rgb).any(1).mean())
    one, two = reference(name, bounce_limit=1), reference(name, bounce_limit=2)
    out["limit_1_vs_2"] = float((Q._words(one.rgb[ps]) != Q._words(two.rgb[ps])).any(1).mean())
    sid = int(name[5:]) if name.startswith("scene") else 0
    if 1 <= sid <= 9:
        assert out["coloured"] >= 0.08, f"{name}: {out['coloured']:.1%} of the rays return a colour other than the background or zero"
    if sid:
        assert out["limit_1_vs_2"] >= 0.04, f"{name}: {out['limit_1_vs_2']:.1%} of the rays differ between bounce limits 1 and 2"
        assert out["advanced"] >= 0.25, f"{name}: {out['advanced']:.1%} of the streams advance"
    if sid in (7, 9):
        assert out["advanced_rays"] >= 30, f"{name}: {out['advanced_rays']} rays advance their stream"
    return out


def deep_rays(name, levels):
    """primary rays whose path runs past `levels` segments: the final stream under bounce_limit = levels differs from the one under 50"""
    a = reference(name, bounce_limit=levels, sets=("primary",))
    b = reference(name, bounce_limit=50, sets=("primary",))
    return int((a.streams.view(np.uint8).reshape(-1, 48) != b.streams.view(np.uint8).reshape(-1, 48)).any(1).sum())
