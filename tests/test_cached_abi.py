"""The C ABI of the cached radiance queries (include/mort_hip.h) as far as it can be checked without a GPU: the
layout of mort_cached_params, every refusal the contract lists, the empty batch and the optional counts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mort_amd import hip, host, structs as S

OK, INVALID, CAPACITY = 0, -1, -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_BOUNCE_LIMIT = 64
FIELDS = ("path", "cache_depth", "flags", "grid", "vis")


def test_layout_as_the_header_declares_it(tmp_path):
    """sizeof and offsetof from the header itself, compiled as C, against the ctypes structure of the binding"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mort_hip.h"\n'
                   'int main(void) { printf("%zu ' + "%zu " * len(FIELDS) + '%u\\n", sizeof(mort_cached_params), ' +
                   "".join(f"offsetof(mort_cached_params, {k}), " for k in FIELDS) + 'MORT_CACHED_VISIBLE); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "cc"), "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    assert got == [84, 0, 28, 32, 36, 76, 1]
    P = hip.CACHED_PARAMS
    assert [C.sizeof(P)] + [getattr(P, k).offset for k in FIELDS] == got[:6] and hip.CACHED_VISIBLE == got[6]


def test_exports():
    L = C.CDLL(hip.LIB_PATH)
    for name in ("mort_hip_query_radiance_cached", "mort_hip_query_radiance_cached_device", "mort_hip_query_radiance_cached_host"):
        assert name in hip.EXPORTS
        getattr(L, name)


@pytest.fixture(scope="module")
def scene():
    return host.build_scene(2, width=16, spp=1)


N = 4
GRID = dict(origin=(-4.0, 0.0, -4.0), spacing=(4.0, 1.0, 2.0), count=(3, 2, 4))


class Buffers:
    """rays that look down on scene 2's ground, streams, a volume of constant records, maps, outputs"""

    def __init__(self, n=N):
        self.rays = np.zeros(n, dtype=hip.RAY_DTYPE)
        self.rays["origin"] = (0, 1, 5); self.rays["dir"] = (0, -0.2, -1); self.rays["time"] = 0.5; self.rays["t_max"] = np.inf
        self.streams = np.zeros(n * 48, dtype=np.uint8)
        g = hip.VOLUME_GRID(**GRID)
        self.records = np.zeros((g.probes, 32), dtype=np.float32)
        self.records[:, 0:3] = 1.0
        self.records[:, 27] = 1.0
        self.depth = np.ones((g.probes, 200), dtype=np.float32)
        self.rgb = np.zeros(3 * n, dtype=np.float32)
        self.ends = np.full(n, 99, dtype=np.uint32)

    def args(self, visible, **kw):
        a = dict(rays=self.rays.ctypes.data, streams=self.streams.ctypes.data, records=self.records.ctypes.data,
                 depth=self.depth.ctypes.data if visible else None, rgb=self.rgb.ctypes.data, ends=self.ends.ctypes.data)
        a.update(kw)
        return a


def _params(cam, visible=False, cache_depth=0, **kw):
    p = hip.CACHED_PARAMS(hip.radiance_params_from_camera(cam), cache_depth, hip.VOLUME_GRID(**GRID),
                          hip.VOLUME_VIS_PARAMS(0.01, 0.05) if visible else None)
    for k, v in kw.items():
        obj, _, field = k.rpartition("__")
        setattr(getattr(p, obj) if obj else p, field, v)
    return p


def _call(world, p, n, a, sec=None):
    return hip.lib().mort_hip_query_radiance_cached_host(world.ptr if world is not None else None, C.byref(p) if p is not None else None, n, a["rays"],
                                                         a["streams"], a["records"], a["depth"], 1, 0, a["rgb"], a["ends"], sec)


@pytest.mark.parametrize("visible", [False, True])
def test_a_valid_call_and_the_optional_counts(scene, visible):
    world, cam = scene
    b = Buffers()
    assert _call(world, _params(cam, visible), N, b.args(visible)) == OK
    assert (b.ends == 1).all() and b.rgb.all(), "every ray ends on the ground, in the volume"
    rgb = b.rgb.copy()
    b2 = Buffers()
    assert _call(world, _params(cam, visible), N, b2.args(visible, ends=None)) == OK, "ends_out may be NULL"
    assert (b2.rgb == rgb).all() and (b2.ends == 99).all()
    out = hip.query_radiance_cached_host(world, _params(cam, visible), b.rays, np.zeros(N * 48, dtype=np.uint8), b.records,
                                         b.depth if visible else None, want_ends=False)
    assert out["ends"] is None and (out["rgb"].reshape(-1) == rgb).all()


@pytest.mark.parametrize("visible", [False, True])
def test_empty_batch_is_ok(scene, visible):
    world, cam = scene
    b = Buffers(1)
    b.streams[:] = 7; b.rgb[:] = 7
    sec = C.c_double(5)
    assert _call(world, _params(cam, visible), 0, b.args(visible), C.byref(sec)) == OK
    assert (b.streams == 7).all() and (b.rgb == 7).all() and (b.ends == 99).all() and sec.value == 0, "nothing is written"
    out = hip.query_radiance_cached_host(world, _params(cam, visible), np.zeros((0, 8), dtype=np.float32), np.zeros(0, dtype=np.uint8), b.records,
                                         b.depth if visible else None)
    assert out["rgb"].shape == (0, 3) and out["ends"].shape == (0,)


def test_null_arguments_are_invalid(scene):
    world, cam = scene
    L = hip.lib()
    b = Buffers()
    p = _params(cam)
    assert _call(None, p, N, b.args(False)) == INVALID
    assert _call(world, None, N, b.args(False)) == INVALID
    for k in ("rays", "streams", "records", "rgb"):
        assert _call(world, p, N, b.args(False, **{k: None})) == INVALID, k
    a = b.args(False)
    # the forms that take a context check it before anything touches a GPU
    assert L.mort_hip_query_radiance_cached(None, C.byref(p), N, a["rays"], a["streams"], a["records"], None, a["rgb"], a["ends"], None) == INVALID
    assert L.mort_hip_query_radiance_cached_device(None, C.byref(p), N, a["rays"], a["streams"], a["records"], None, a["rgb"], a["ends"], None,
                                                   None) == INVALID


def test_depth_goes_with_the_flag(scene):
    world, cam = scene
    b = Buffers()
    assert _call(world, _params(cam, False), N, b.args(True)) == INVALID, "maps without MORT_CACHED_VISIBLE"
    assert _call(world, _params(cam, True), N, b.args(False)) == INVALID, "MORT_CACHED_VISIBLE without maps"
    assert _call(world, _params(cam, False, flags=2), N, b.args(False)) == INVALID, "an unknown flag bit"
    assert _call(world, _params(cam, True, flags=3), N, b.args(True)) == INVALID
    assert _call(world, _params(cam, True, flags=0x80000001), N, b.args(True)) == INVALID


def test_parameter_checks(scene):
    world, cam = scene
    b = Buffers()

    def status(visible=False, **kw):
        return _call(world, _params(cam, visible, **kw), N, b.args(visible))

    assert status() == OK and status(True) == OK
    # the new fields
    assert status(cache_depth=-1) == INVALID and status(cache_depth=MAX_BOUNCE_LIMIT + 1) == INVALID
    assert status(cache_depth=MAX_BOUNCE_LIMIT) == OK
    # the radiance calls' checks
    assert status(path__samples=0) == INVALID
    assert status(path__bounce_limit=-1) == CAPACITY and status(path__bounce_limit=MAX_BOUNCE_LIMIT + 1) == CAPACITY
    assert status(path__bounce_limit=0) == OK
    n_spheres = world.c.objs.num_spheres
    assert status(path__light_obj_type=S.OBJ_SPHERE, path__light_obj_idx=n_spheres) == INVALID
    assert status(path__light_obj_type=S.OBJ_QUAD, path__light_obj_idx=1 << 20) == INVALID
    assert status(path__light_obj_type=S.OBJ_SPHERE, path__light_obj_idx=0) == OK
    # the volume calls' checks: counts 1 .. MORT_VOLUME_MAX_COUNT, spacing and origin
    for bad in (0, -1, hip.VOLUME_MAX_COUNT + 1):
        p = _params(cam)
        p.grid.count[1] = bad
        assert _call(world, p, N, b.args(False)) == INVALID, bad
    for bad in (0.0, -1.0, np.inf, np.nan):
        p = _params(cam)
        p.grid.spacing[2] = bad
        assert _call(world, p, N, b.args(False)) == INVALID, bad
    p = _params(cam)
    p.grid.origin[0] = np.nan
    assert _call(world, p, N, b.args(False)) == INVALID
    # the visibility parameters, read only with the flag
    for k, bad in (("normal_bias", -0.5), ("normal_bias", np.nan), ("min_visibility", -0.1), ("min_visibility", 1.5), ("min_visibility", np.inf)):
        assert status(True, **{"vis__" + k: bad}) == INVALID, (k, bad)
        assert status(False, **{"vis__" + k: bad}) == OK, (k, bad)


def test_overlapping_buffers_are_refused(scene):
    world, cam = scene
    n = 8
    b = Buffers(n)
    g = hip.VOLUME_GRID(**GRID)
    buf = np.zeros(n * (32 + 48 + 12 + 4) + 64, dtype=np.uint8)
    base = buf.ctypes.data
    buf[:n * 32].view(hip.RAY_DTYPE)[:] = b.rays
    rays, streams, rgb, ends = base, base + n * 32, base + n * 80, base + n * 92  # side by side
    rec, dep = b.records.ctypes.data, b.depth.ctypes.data

    def status(visible=False, **kw):
        a = dict(rays=rays, streams=streams, records=rec, depth=dep if visible else None, rgb=rgb, ends=ends)
        a.update(kw)
        return _call(world, _params(cam, visible), n, a)

    assert status() == OK and status(True) == OK
    assert status(rgb=rays) == INVALID                      # colours over the rays
    assert status(streams=rays + 16) == INVALID             # streams over the rays
    assert status(rgb=streams + n * 48 - 4) == INVALID      # colours over the streams' tail
    assert status(ends=rgb + n * 12 - 4) == INVALID         # counts over the colours' tail
    assert status(ends=rays + n * 32 - 4) == INVALID        # counts over the rays' tail
    assert status(ends=streams) == INVALID                  # counts over the streams
    assert status(rgb=rec + g.probes * 128 - 4) == INVALID  # colours over the records' tail
    assert status(ends=rec) == INVALID                      # counts over the records
    assert status(streams=rec) == INVALID                   # streams over the records
    assert status(True, rgb=dep + g.probes * 800 - 4) == INVALID  # colours over the maps' tail
    assert status(True, ends=dep) == INVALID                # counts over the maps
