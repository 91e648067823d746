"""The C ABI of the ray queries (include/mort_hip.h) as far as it can be checked without a GPU: the layouts of
mort_ray and mort_hit, the argument checks of the host forms, the empty batch, the refusal of overlapping buffers, and the
miss for an interval that is empty or not a number."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mort_amd import hip, host

OK, INVALID = 0, -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layouts_as_the_header_declares_them(tmp_path):
    """sizeof and offsetof from the header itself, compiled as C, against the numpy dtypes of the binding"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mort_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(mort_ray), offsetof(mort_ray, origin), offsetof(mort_ray, dir), '
                   'offsetof(mort_ray, time), offsetof(mort_ray, t_max));\n'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(mort_hit), offsetof(mort_hit, p), offsetof(mort_hit, normal), offsetof(mort_hit, t), '
                   'offsetof(mort_hit, u), offsetof(mort_hit, v), offsetof(mort_hit, mat_type), offsetof(mort_hit, mat_idx), offsetof(mort_hit, flags));\n'
                   'printf("%u %u %u\\n", MORT_HIT_HIT, MORT_HIT_FRONT_FACE, MORT_HIT_MEDIUM); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "cc"), "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    ray, hit, flags = [list(map(int, ln.split())) for ln in subprocess.check_output([str(exe)], text=True).strip().splitlines()]
    assert ray == [32, 0, 12, 24, 28]
    assert hit == [48, 0, 12, 24, 28, 32, 36, 40, 44]
    assert flags == [hip.HIT_HIT, hip.HIT_FRONT_FACE, hip.HIT_MEDIUM] == [1, 2, 4]
    R, Hd = hip.RAY_DTYPE, hip.HIT_DTYPE
    assert [R.itemsize] + [R.fields[k][1] for k in ("origin", "dir", "time", "t_max")] == ray
    assert [Hd.itemsize] + [Hd.fields[k][1] for k in ("p", "normal", "t", "u", "v", "mat_type", "mat_idx", "flags")] == hit


@pytest.fixture(scope="module")
def world():
    w, _ = host.build_scene(2, width=16, spp=1)
    return w


def _rays(n, t_max=np.inf):
    r = np.zeros(n, dtype=hip.RAY_DTYPE)
    r["origin"] = (0, 1, 5); r["dir"] = (0, -0.2, -1); r["time"] = 0.5; r["t_max"] = t_max
    return r


def test_empty_batch_is_ok(world):
    L = hip.lib()
    r, h, o = _rays(1), np.full(1, 7, dtype=np.uint8).repeat(48), np.full(1, 7, dtype=np.uint8)
    assert L.mort_hip_query_closest_host(world.ptr, 0, r.ctypes.data, None, 1, 0, h.ctypes.data, None) == OK
    assert L.mort_hip_query_occluded_host(world.ptr, 0, r.ctypes.data, 1, 0, o.ctypes.data, None) == OK
    assert (h == 7).all() and (o == 7).all(), "nothing is written"
    assert hip.query_closest_host(world, np.zeros((0, 8), dtype=np.float32))["hits"].shape == (0,)


def test_null_arguments_are_invalid(world):
    L = hip.lib()
    r, h, o = _rays(4), np.zeros(4, dtype=hip.HIT_DTYPE), np.zeros(4, dtype=np.uint8)
    sec = C.c_double(0)
    assert L.mort_hip_query_closest_host(None, 4, r.ctypes.data, None, 1, 0, h.ctypes.data, C.byref(sec)) == INVALID
    assert L.mort_hip_query_closest_host(world.ptr, 4, None, None, 1, 0, h.ctypes.data, C.byref(sec)) == INVALID
    assert L.mort_hip_query_closest_host(world.ptr, 4, r.ctypes.data, None, 1, 0, None, C.byref(sec)) == INVALID
    assert L.mort_hip_query_occluded_host(None, 4, r.ctypes.data, 1, 0, o.ctypes.data, None) == INVALID
    assert L.mort_hip_query_occluded_host(world.ptr, 4, None, 1, 0, o.ctypes.data, None) == INVALID
    assert L.mort_hip_query_occluded_host(world.ptr, 4, r.ctypes.data, 1, 0, None, None) == INVALID
    # the forms that take a context check it before anything touches a GPU
    assert L.mort_hip_query_closest(None, 4, r.ctypes.data, None, h.ctypes.data, None) == INVALID
    assert L.mort_hip_query_closest_device(None, 4, r.ctypes.data, None, h.ctypes.data, None, None) == INVALID
    assert L.mort_hip_query_occluded(None, 4, r.ctypes.data, o.ctypes.data, None) == INVALID
    assert L.mort_hip_query_occluded_device(None, 4, r.ctypes.data, o.ctypes.data, None, None) == INVALID
    # seconds and states may be NULL
    assert L.mort_hip_query_closest_host(world.ptr, 4, r.ctypes.data, None, 1, 0, h.ctypes.data, None) == OK


def test_overlapping_buffers_are_refused(world):
    L = hip.lib()
    n = 8
    buf = np.zeros(n * 48 * 3, dtype=np.uint8)
    base = buf.ctypes.data
    buf[:n * 32].view(hip.RAY_DTYPE)[:] = _rays(n)
    # records over the rays, records over the tail of the rays, streams over the rays, streams over the records, bytes over the rays
    assert L.mort_hip_query_closest_host(world.ptr, n, base, None, 1, 0, base, None) == INVALID
    assert L.mort_hip_query_closest_host(world.ptr, n, base, None, 1, 0, base + n * 32 - 16, None) == INVALID
    assert L.mort_hip_query_closest_host(world.ptr, n, base, base + 16, 1, 0, base + n * 48, None) == INVALID
    assert L.mort_hip_query_closest_host(world.ptr, n, base, base + n * 48 + 48, 1, 0, base + n * 48, None) == INVALID
    assert L.mort_hip_query_occluded_host(world.ptr, n, base, 1, 0, base + n * 32 - 1, None) == INVALID
    # side by side is fine
    assert L.mort_hip_query_closest_host(world.ptr, n, base, base + n * 32 + n * 48, 1, 0, base + n * 32, None) == OK
    assert L.mort_hip_query_occluded_host(world.ptr, n, base, 1, 0, base + n * 32, None) == OK


@pytest.mark.parametrize("tree", [False, True])
def test_an_empty_or_nan_interval_is_a_miss(world, tree):
    hit = hip.query_closest_host(world, _rays(3), tree=tree)["hits"]
    assert (hit["flags"] & 1).all(), "the ray of this test hits the ground"
    for t_max in (np.nan, 0.001, 0.0, -1.0, -np.inf):
        r = _rays(3, t_max)
        streams = np.arange(3 * 48, dtype=np.uint8)
        before = streams.copy()
        got = hip.query_closest_host(world, r, states=streams, tree=tree)["hits"]
        assert not got.view(np.uint8).any(), f"t_max {t_max}: not an all-zero record"
        assert (streams == before).all()
        assert not hip.query_occluded_host(world, r, tree=tree)["occluded"].any()
    assert hip.query_occluded_host(world, _rays(3, float(np.nextafter(np.float32(0.001), np.float32(1)))), tree=tree)["occluded"].sum() == 0
