"""The C ABI of the radiance queries (include/mort_hip.h) as far as it can be checked without a GPU: the layout of
mort_radiance_params, its defaults from a camera, every status code of the host form, the refusal of overlapping buffers and
the empty batch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mort_amd import hip, host, structs as S

OK, INVALID, UNSUPPORTED, CAPACITY = 0, -1, -6, -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_BOUNCE_LIMIT = 64


def test_layout_as_the_header_declares_it(tmp_path):
    """sizeof and offsetof from the header itself, compiled as C, against the ctypes structure of the binding"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mort_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(mort_radiance_params), offsetof(mort_radiance_params, bounce_limit), '
                   'offsetof(mort_radiance_params, samples), offsetof(mort_radiance_params, background), offsetof(mort_radiance_params, light_obj_type), '
                   'offsetof(mort_radiance_params, light_obj_idx), MORT_MAX_BOUNCE_LIMIT); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "cc"), "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    assert got == [28, 0, 4, 8, 20, 24, MAX_BOUNCE_LIMIT]
    P = hip.RADIANCE_PARAMS
    assert [C.sizeof(P)] + [getattr(P, k).offset for k in ("bounce_limit", "samples", "background", "light_obj_type", "light_obj_idx")] == got[:6]


def test_exports():
    L = C.CDLL(hip.LIB_PATH)
    for name in ("mort_hip_radiance_params_from_camera", "mort_hip_query_radiance", "mort_hip_query_radiance_device",
                 "mort_hip_query_radiance_host", "mort_hip_debug_radiance_lds_levels"):
        assert name in hip.EXPORTS or name.startswith("mort_hip_debug_")
        getattr(L, name)
    # 8 KB of traversal column beside the levels, four groups in a CU's 160 KB
    levels = hip.radiance_lds_levels()
    assert levels >= 1 and 4 * (16 * 256 * 2 + levels * 256 * 16) <= 160 * 1024


def test_defaults_from_a_camera():
    _, cam = host.build_scene(6, width=32, spp=4)
    p = hip.radiance_params_from_camera(cam)
    assert p.samples == 1 and p.bounce_limit == cam.bounce_limit
    assert (p.light_obj_type, p.light_obj_idx) == (cam.light_obj_type, cam.light_obj_idx) and cam.light_obj_type != -1
    _, cam = host.build_scene(2, width=32, spp=4)
    p = hip.radiance_params_from_camera(cam)
    assert [p.background[k] for k in range(3)] == [cam.background.e[k] for k in range(3)] and any(p.background)
    assert p.light_obj_type == -1
    L = hip.lib()
    assert L.mort_hip_radiance_params_from_camera(None, C.byref(p)) == INVALID
    assert L.mort_hip_radiance_params_from_camera(C.cast(C.byref(cam), C.c_void_p), None) == INVALID


@pytest.fixture(scope="module")
def scene():
    w, cam = host.build_scene(2, width=16, spp=1)
    return w, cam


def _rays(n):
    r = np.zeros(n, dtype=hip.RAY_DTYPE)
    r["origin"] = (0, 1, 5); r["dir"] = (0, -0.2, -1); r["time"] = 0.5; r["t_max"] = np.inf
    return r


def _call(world, p, n, rays, states, rgb, sec=None):
    return hip.lib().mort_hip_query_radiance_host(world.ptr if world is not None else None, C.byref(p) if p is not None else None, n, rays, states, 1, 0, rgb, sec)


def test_empty_batch_is_ok(scene):
    world, cam = scene
    p = hip.radiance_params_from_camera(cam)
    r, st, rgb = _rays(1), np.full(48, 7, dtype=np.uint8), np.full(3, 7, dtype=np.float32)
    sec = C.c_double(5)
    assert _call(world, p, 0, r.ctypes.data, st.ctypes.data, rgb.ctypes.data, C.byref(sec)) == OK
    assert (st == 7).all() and (rgb == 7).all() and sec.value == 0, "nothing is written"
    out = hip.query_radiance_host(world, p, np.zeros((0, 8), dtype=np.float32), np.zeros(0, dtype=np.uint8))
    assert out["rgb"].shape == (0, 3)


def test_null_arguments_are_invalid(scene):
    world, cam = scene
    L = hip.lib()
    p = hip.radiance_params_from_camera(cam)
    r, st, rgb = _rays(4), np.zeros(4 * 48, dtype=np.uint8), np.zeros(12, dtype=np.float32)
    a = (r.ctypes.data, st.ctypes.data, rgb.ctypes.data)
    assert _call(None, p, 4, *a) == INVALID
    assert _call(world, None, 4, *a) == INVALID
    assert _call(world, p, 4, None, a[1], a[2]) == INVALID
    assert _call(world, p, 4, a[0], None, a[2]) == INVALID, "the streams are required"
    assert _call(world, p, 4, a[0], a[1], None) == INVALID
    # the forms that take a context check it before anything touches a GPU
    assert L.mort_hip_query_radiance(None, C.byref(p), 4, *a, None) == INVALID
    assert L.mort_hip_query_radiance_device(None, C.byref(p), 4, *a, None, None) == INVALID
    # seconds may be NULL
    assert _call(world, p, 4, *a) == OK
    assert rgb.any() and st.any()


def test_parameter_checks(scene):
    world, cam = scene
    r, st, rgb = _rays(4), np.zeros(4 * 48, dtype=np.uint8), np.zeros(12, dtype=np.float32)
    a = (r.ctypes.data, st.ctypes.data, rgb.ctypes.data)

    def status(**kw):
        p = hip.radiance_params_from_camera(cam)
        for k, v in kw.items():
            setattr(p, k, v)
        return _call(world, p, 4, *a)

    assert status() == OK
    assert status(samples=0) == INVALID and status(samples=-3) == INVALID
    assert status(bounce_limit=-1) == CAPACITY and status(bounce_limit=MAX_BOUNCE_LIMIT + 1) == CAPACITY
    assert status(bounce_limit=0) == OK and status(bounce_limit=MAX_BOUNCE_LIMIT) == OK
    # the light object, as mort_hip_render_host checks the camera's: a primitive or list that is not there
    n_spheres = world.c.objs.num_spheres
    assert status(light_obj_type=S.OBJ_SPHERE, light_obj_idx=n_spheres) == INVALID
    assert status(light_obj_type=S.OBJ_SPHERE, light_obj_idx=-1) == INVALID
    assert status(light_obj_type=S.OBJ_QUAD, light_obj_idx=1 << 20) == INVALID
    assert status(light_obj_type=S.OBJ_HITTABLE_LIST, light_obj_idx=1 << 20) == INVALID
    assert status(light_obj_type=S.OBJ_SPHERE, light_obj_idx=0) == OK
    # ... and the render's own status for the same camera
    bad = type(cam).from_buffer_copy(cam)
    bad.light_obj_type, bad.light_obj_idx = S.OBJ_SPHERE, n_spheres
    with pytest.raises(hip.MortHipError) as e:
        hip.render_host(world, bad)
    assert e.value.status == INVALID
    bad = type(cam).from_buffer_copy(cam)
    bad.bounce_limit = MAX_BOUNCE_LIMIT + 1
    with pytest.raises(hip.MortHipError) as e:
        hip.render_host(world, bad)
    assert e.value.status == CAPACITY


def test_nested_light_lists_are_unsupported():
    """a light list that holds a list: MORT_ERR_UNSUPPORTED, as for the render"""
    w, cam = host.build_scene(2, width=16, spp=1)
    L = host.lib()
    inner = L.mort_add_hittable_list(w.ptr, True)
    outer = L.mort_add_hittable_list(w.ptr, True)
    assert inner >= 0 and outer >= 0
    L.mort_list_add(w.ptr, inner, S.OBJ_SPHERE, 0)
    L.mort_list_add(w.ptr, outer, S.OBJ_HITTABLE_LIST, inner)
    p = hip.radiance_params_from_camera(cam)
    p.light_obj_type, p.light_obj_idx = S.OBJ_HITTABLE_LIST, outer
    r, st, rgb = _rays(1), np.zeros(48, dtype=np.uint8), np.zeros(3, dtype=np.float32)
    assert _call(w, p, 1, r.ctypes.data, st.ctypes.data, rgb.ctypes.data) == UNSUPPORTED
    p.light_obj_idx = inner
    assert _call(w, p, 1, r.ctypes.data, st.ctypes.data, rgb.ctypes.data) == OK


def test_overlapping_buffers_are_refused(scene):
    world, cam = scene
    p = hip.radiance_params_from_camera(cam)
    n = 8
    buf = np.zeros(n * 48 * 4, dtype=np.uint8)
    base = buf.ctypes.data
    buf[:n * 32].view(hip.RAY_DTYPE)[:] = _rays(n)
    rays, streams, rgb = base, base + n * 32, base + n * 32 + n * 48  # side by side
    assert _call(world, p, n, rays, streams, rgb) == OK
    assert _call(world, p, n, rays, streams, rays) == INVALID                # colours over the rays
    assert _call(world, p, n, rays, streams, rays + n * 32 - 4) == INVALID   # colours over the rays' tail
    assert _call(world, p, n, rays, rays + 16, rgb) == INVALID               # streams over the rays
    assert _call(world, p, n, rays, streams, streams + n * 48 - 4) == INVALID  # colours over the streams' tail
    assert _call(world, p, n, rays, rgb + 8, rgb) == INVALID                 # streams over the colours
