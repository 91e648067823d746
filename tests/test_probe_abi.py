"""The C ABI of the light probes (include/mort_hip.h) as far as it can be checked without a GPU: the layout of
mort_probe and mort_probe_params, every status code of the host form, the refusal of overlapping buffers, the empty batch and the
direction counts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mort_amd import hip, host, structs as S

OK, INVALID, UNSUPPORTED, CAPACITY = 0, -1, -6, -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_BOUNCE_LIMIT = 64
D = 64


def test_layout_as_the_header_declares_it(tmp_path):
    """sizeof and offsetof from the header itself, compiled as C, against the ctypes structures and the dtype of the binding"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mort_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(mort_probe), offsetof(mort_probe, position), offsetof(mort_probe, time), '
                   'sizeof(mort_probe_params), sizeof(mort_radiance_params), offsetof(mort_probe_params, directions), MORT_SH9_FLOATS); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "cc"), "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    assert got == [16, 0, 12, 32, 28, 28, 27]
    assert got[3] == got[4] + 4
    assert C.sizeof(hip.PROBE_PARAMS) == 32 and hip.PROBE_PARAMS.rp.offset == 0 and hip.PROBE_PARAMS.directions.offset == 28
    assert hip.PROBE_DTYPE.itemsize == 16 and hip.PROBE_DTYPE.fields["position"][1] == 0 and hip.PROBE_DTYPE.fields["time"][1] == 12
    assert hip.SH9_FLOATS == 27


def test_exports():
    L = C.CDLL(hip.LIB_PATH)
    for name in ("mort_hip_probe_directions", "mort_hip_probe_bake", "mort_hip_probe_bake_device", "mort_hip_probe_bake_host",
                 "mort_hip_sh9_irradiance"):
        assert name in hip.EXPORTS
        getattr(L, name)


@pytest.fixture(scope="module")
def scene():
    return host.build_scene(2, width=16, spp=1)


def _probes(n):
    p = np.zeros(n, dtype=hip.PROBE_DTYPE)
    p["position"] = (0, 1, 5); p["time"] = 0.5
    return p


def _call(world, p, n, probes, dirs, states, sh, sec=None):
    return hip.lib().mort_hip_probe_bake_host(world.ptr if world is not None else None, C.byref(p) if p is not None else None, n, probes, dirs,
                                              states, 1, 0, sh, sec)


def _buffers(n):
    return _probes(n), np.zeros(n * D * 48, dtype=np.uint8), np.zeros(n * 27, dtype=np.float32)


def test_empty_batch_is_ok(scene):
    world, cam = scene
    p = hip.probe_params_from_camera(cam, D)
    pr, st, sh = _probes(1), np.full(D * 48, 7, dtype=np.uint8), np.full(27, 7, dtype=np.float32)
    sec = C.c_double(5)
    assert _call(world, p, 0, pr.ctypes.data, None, st.ctypes.data, sh.ctypes.data, C.byref(sec)) == OK
    assert (st == 7).all() and (sh == 7).all() and sec.value == 0, "nothing is written"
    out = hip.probe_bake_host(world, p, np.zeros((0, 4), dtype=np.float32), np.zeros(0, dtype=np.uint8))
    assert out["sh"].shape == (0, 9, 3)


def test_null_arguments_are_invalid(scene):
    world, cam = scene
    L = hip.lib()
    p = hip.probe_params_from_camera(cam, D)
    pr, st, sh = _buffers(2)
    a = (pr.ctypes.data, None, st.ctypes.data, sh.ctypes.data)
    assert _call(None, p, 2, *a) == INVALID
    assert _call(world, None, 2, *a) == INVALID
    assert _call(world, p, 2, None, None, a[2], a[3]) == INVALID
    assert _call(world, p, 2, a[0], None, None, a[3]) == INVALID, "the streams are required"
    assert _call(world, p, 2, a[0], None, a[2], None) == INVALID
    # the forms that take a context check it before anything touches a GPU
    assert L.mort_hip_probe_bake(None, C.byref(p), 2, *a, None) == INVALID
    assert L.mort_hip_probe_bake_device(None, C.byref(p), 2, *a, None, None) == INVALID
    # seconds and the directions may be NULL
    assert _call(world, p, 2, *a) == OK
    assert sh.any() and st.any()
    # the helpers
    d = np.zeros((D, 3), dtype=np.float32)
    assert L.mort_hip_probe_directions(D, None) == INVALID and L.mort_hip_probe_directions(D, d.ctypes.data) == OK
    rgb, nrm = np.zeros(3, dtype=np.float32), np.array([0, 0, 1], dtype=np.float32)
    assert L.mort_hip_sh9_irradiance(None, nrm.ctypes.data, rgb.ctypes.data) == INVALID
    assert L.mort_hip_sh9_irradiance(sh.ctypes.data, None, rgb.ctypes.data) == INVALID
    assert L.mort_hip_sh9_irradiance(sh.ctypes.data, nrm.ctypes.data, None) == INVALID
    assert L.mort_hip_sh9_irradiance(sh.ctypes.data, nrm.ctypes.data, rgb.ctypes.data) == OK


def test_parameter_checks(scene):
    world, cam = scene
    pr = _probes(1)
    st, sh = np.zeros(4160 * 48, dtype=np.uint8), np.zeros(27, dtype=np.float32)  # room for any direction count tried
    a = (pr.ctypes.data, None, st.ctypes.data, sh.ctypes.data)

    def status(directions=D, **kw):
        p = hip.probe_params_from_camera(cam, directions)
        for k, v in kw.items():
            setattr(p.rp, k, v)
        return _call(world, p, 1, *a)

    assert status() == OK
    for bad in (0, 63, 65, 4160, -64, 32):
        assert status(directions=bad) == INVALID, bad
    assert (st[D * 48:] == 0).all() and status(directions=128) == OK and status(directions=4096, bounce_limit=1) == OK
    assert status(samples=0) == INVALID and status(samples=-3) == INVALID
    assert status(bounce_limit=-1) == CAPACITY and status(bounce_limit=MAX_BOUNCE_LIMIT + 1) == CAPACITY
    assert status(bounce_limit=0) == OK and status(bounce_limit=MAX_BOUNCE_LIMIT) == OK
    assert status(directions=63, bounce_limit=-1) == INVALID, "the order of the checks: the counts before the bounce limit"
    # n D above the queries' ray limit, before any buffer is touched
    p = hip.probe_params_from_camera(cam, 4096)
    assert _call(world, p, (0x7fffffff * 256) // 4096 + 1, *a) == INVALID
    # the light object, as the radiance queries check it
    n_spheres = world.c.objs.num_spheres
    assert status(light_obj_type=S.OBJ_SPHERE, light_obj_idx=n_spheres) == INVALID
    assert status(light_obj_type=S.OBJ_SPHERE, light_obj_idx=-1) == INVALID
    assert status(light_obj_type=S.OBJ_QUAD, light_obj_idx=1 << 20) == INVALID
    assert status(light_obj_type=S.OBJ_HITTABLE_LIST, light_obj_idx=1 << 20) == INVALID
    assert status(light_obj_type=S.OBJ_SPHERE, light_obj_idx=0) == OK


def test_nested_light_lists_are_unsupported():
    """a light list that holds a list: MORT_ERR_UNSUPPORTED, as for the render and the radiance queries"""
    w, cam = host.build_scene(2, width=16, spp=1)
    L = host.lib()
    inner = L.mort_add_hittable_list(w.ptr, True)
    outer = L.mort_add_hittable_list(w.ptr, True)
    assert inner >= 0 and outer >= 0
    L.mort_list_add(w.ptr, inner, S.OBJ_SPHERE, 0)
    L.mort_list_add(w.ptr, outer, S.OBJ_HITTABLE_LIST, inner)
    p = hip.probe_params_from_camera(cam, D)
    p.rp.light_obj_type, p.rp.light_obj_idx = S.OBJ_HITTABLE_LIST, outer
    pr, st, sh = _buffers(1)
    assert _call(w, p, 1, pr.ctypes.data, None, st.ctypes.data, sh.ctypes.data) == UNSUPPORTED
    p.rp.light_obj_idx = inner
    assert _call(w, p, 1, pr.ctypes.data, None, st.ctypes.data, sh.ctypes.data) == OK


def test_overlapping_buffers_are_refused(scene):
    world, cam = scene
    p = hip.probe_params_from_camera(cam, D)
    n = 2
    buf = np.zeros(n * 16 + D * 12 + n * D * 48 + n * 108 + 64, dtype=np.uint8)
    base = buf.ctypes.data
    probes, dirs, streams, sh = base, base + n * 16, base + n * 16 + D * 12, base + n * 16 + D * 12 + n * D * 48  # side by side
    buf[:n * 16].view(hip.PROBE_DTYPE)[:] = _probes(n)
    buf[n * 16:n * 16 + D * 12].view(np.float32)[:] = hip.probe_directions(D).reshape(-1)
    assert _call(world, p, n, probes, dirs, streams, sh) == OK
    assert _call(world, p, n, probes, dirs, streams, probes) == INVALID               # coefficients over the probes
    assert _call(world, p, n, probes, dirs, streams, dirs + D * 12 - 4) == INVALID    # coefficients over the directions' tail
    assert _call(world, p, n, probes, dirs, probes + 16, sh) == INVALID               # streams over the probes
    assert _call(world, p, n, probes, dirs, dirs + 4, sh) == INVALID                  # streams over the directions
    assert _call(world, p, n, probes, dirs, streams, streams + n * D * 48 - 4) == INVALID  # coefficients over the streams' tail
    assert _call(world, p, n, probes, dirs, sh + 8, sh) == INVALID                    # streams over the coefficients
