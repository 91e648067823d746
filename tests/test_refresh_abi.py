"""The C ABI of the volume refresh (include/mort_hip.h) as far as it can be checked without a GPU: the layout of
mort_refresh_params, every refusal the contract lists with the outputs still at their fill, the empty selection, every overlap
pair, and the view's update call without a view."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mort_amd import hip, host, structs as S

OK, INVALID, CAPACITY = 0, -1, -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_BOUNCE_LIMIT = 64
FIELDS = ("cached", "directions", "hysteresis", "first", "step")
GRID = dict(origin=(-4.0, 0.5, -4.0), spacing=(4.0, 1.0, 2.0), count=(3, 2, 4))
P, D = 24, 64
FILL = 0x5a


def test_layout_as_the_header_declares_it(tmp_path):
    """sizeof and offsetof from the header itself, compiled as C, against the ctypes structure of the binding"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mort_hip.h"\n'
                   'int main(void) { printf("%zu ' + "%zu " * len(FIELDS) + '\\n", sizeof(mort_refresh_params), ' +
                   ", ".join(f"offsetof(mort_refresh_params, {k})" for k in FIELDS) + '); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "cc"), "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    assert got == [100, 0, 84, 88, 92, 96]
    R = hip.REFRESH_PARAMS
    assert [C.sizeof(R)] + [getattr(R, k).offset for k in FIELDS] == got


def test_exports():
    L = C.CDLL(hip.LIB_PATH)
    for name in ("mort_hip_volume_refresh", "mort_hip_volume_refresh_device", "mort_hip_volume_refresh_host", "mort_hip_probe_directions_round",
                 "mort_hip_view_update_cache", "mort_hip_view_update_cache_host"):
        assert name in hip.EXPORTS
        getattr(L, name)


@pytest.fixture(scope="module")
def scene():
    return host.build_scene(2, width=16, spp=1)


class Buffers:
    """the library's directions, streams, a volume of constant records above scene 2's ground, maps, and the outputs at a fill"""

    def __init__(self):
        self.dirs = hip.probe_directions(D)
        self.streams = np.full(P * D * 48, FILL, dtype=np.uint8)
        self.records = np.zeros((P, 32), dtype=np.float32)
        self.records[:, 0:3] = 1.0
        self.records[:, 27] = 1.0
        self.depth = np.ones((P, 200), dtype=np.float32)
        self.out = np.full(P * 128, FILL, dtype=np.uint8)
        self.ends = np.full(P * 4, FILL, dtype=np.uint8)

    def args(self, visible, **kw):
        a = dict(dirs=self.dirs.ctypes.data, streams=self.streams.ctypes.data, records_in=self.records.ctypes.data,
                 depth=self.depth.ctypes.data if visible else None, records_out=self.out.ctypes.data, ends=self.ends.ctypes.data)
        a.update(kw)
        return a

    def untouched(self):
        return (self.streams == FILL).all() and (self.out == FILL).all() and (self.ends == FILL).all()


def _params(cam, visible=False, **kw):
    c = hip.CACHED_PARAMS(hip.radiance_params_from_camera(cam), 0, hip.VOLUME_GRID(**GRID), hip.VOLUME_VIS_PARAMS(0.01, 0.05) if visible else None)
    p = hip.REFRESH_PARAMS(c, D, 0.5, 0, 1)
    for k, v in kw.items():
        o = p
        *objs, field = k.split("__")
        for part in objs:
            o = getattr(o, part)
        setattr(o, field, v)
    return p


def _call(world, p, m, a, sec=None):
    return hip.lib().mort_hip_volume_refresh_host(world.ptr if world is not None else None, C.byref(p) if p is not None else None, m, a["dirs"],
                                                  a["streams"], a["records_in"], a["depth"], 1, 0, a["records_out"], a["ends"], sec)


@pytest.mark.parametrize("visible", [False, True])
def test_a_valid_call_and_the_optional_arguments(scene, visible):
    world, cam = scene
    b = Buffers()
    b.streams[:] = 0
    assert _call(world, _params(cam, visible), P, b.args(visible)) == OK
    rec = b.out.view(np.float32).reshape(P, 32)
    assert (rec[:, 27] == 1.0).all() and (rec[:, 28:] == 0.0).all() and rec[:, :3].all()
    assert (b.ends.view(np.uint32) > 0).all(), "every probe looks down on the ground, in the volume"
    b2 = Buffers()
    b2.streams[:] = 0
    assert _call(world, _params(cam, visible), P, b2.args(visible, ends=None, dirs=None)) == OK, "ends_out and dirs may be NULL"
    assert (b2.out == b.out).all() and (b2.ends == FILL).all()


@pytest.mark.parametrize("visible", [False, True])
def test_empty_selection_is_ok(scene, visible):
    world, cam = scene
    b = Buffers()
    sec = C.c_double(5)
    assert _call(world, _params(cam, visible), 0, b.args(visible), C.byref(sec)) == OK
    assert b.untouched() and sec.value == 0, "nothing is written"
    assert _call(world, _params(cam, visible, first=P + 7), 0, b.args(visible)) == OK, "no selected probe, no range to check"
    assert _call(world, _params(cam, visible, step=0), 0, b.args(visible)) == INVALID


def test_null_arguments_are_invalid(scene):
    world, cam = scene
    L = hip.lib()
    b = Buffers()
    p = _params(cam)
    assert _call(None, p, P, b.args(False)) == INVALID
    assert _call(world, None, P, b.args(False)) == INVALID
    for k in ("streams", "records_in", "records_out"):
        assert _call(world, p, P, b.args(False, **{k: None})) == INVALID, k
    a = b.args(False)
    # the forms that take a context check it before anything touches a GPU
    assert L.mort_hip_volume_refresh(None, C.byref(p), P, a["dirs"], a["streams"], a["records_in"], None, a["records_out"], a["ends"], None) == INVALID
    assert L.mort_hip_volume_refresh_device(None, C.byref(p), P, a["dirs"], a["streams"], a["records_in"], None, a["records_out"], a["ends"], None,
                                            None) == INVALID
    assert b.untouched()


def test_the_view_calls_without_a_view():
    L = hip.lib()
    rec = np.zeros((P, 32), dtype=np.float32)
    assert L.mort_hip_view_update_cache(None, rec.ctypes.data, None) == INVALID
    assert L.mort_hip_view_update_cache_host(None, rec.ctypes.data, None) == INVALID


def test_parameter_checks(scene):
    world, cam = scene
    b = Buffers()

    def status(visible=False, m=P, **kw):
        return _call(world, _params(cam, visible, **kw), m, b.args(visible))

    # the bake's checks of the directions and the samples
    for bad in (0, 63, 65, 96, 4160, -64):
        assert status(directions=bad) == INVALID, bad
    assert status(cached__path__samples=0) == INVALID
    # the cached calls' checks
    assert status(False, cached__flags=2) == INVALID and status(True, cached__flags=3) == INVALID
    assert _call(world, _params(cam, False), P, b.args(True)) == INVALID, "maps without MORT_CACHED_VISIBLE"
    assert _call(world, _params(cam, True), P, b.args(False)) == INVALID, "MORT_CACHED_VISIBLE without maps"
    assert status(cached__cache_depth=-1) == INVALID and status(cached__cache_depth=MAX_BOUNCE_LIMIT + 1) == INVALID
    for bad in (0, -1, hip.VOLUME_MAX_COUNT + 1):
        p = _params(cam)
        p.cached.grid.count[1] = bad
        assert _call(world, p, 1, b.args(False)) == INVALID, bad
    for bad in (0.0, -1.0, np.inf, np.nan):
        p = _params(cam)
        p.cached.grid.spacing[2] = bad
        assert _call(world, p, P, b.args(False)) == INVALID, bad
    for k, bad in (("normal_bias", -0.5), ("normal_bias", np.nan), ("min_visibility", -0.1), ("min_visibility", 1.5)):
        assert status(True, **{"cached__vis__" + k: bad}) == INVALID, (k, bad)
    # the hysteresis
    for bad in (np.nan, -0.25, -np.inf, 1.0, 1.5, np.inf):
        assert status(hysteresis=bad) == INVALID, bad
    # the selection, without overflow
    assert status(step=0) == INVALID
    assert status(first=P, m=1) == INVALID and status(first=1) == INVALID and status(step=2) == INVALID
    assert status(first=3, step=7, m=4) == INVALID
    assert status(first=0xffffffff, step=0xffffffff, m=2) == INVALID and status(first=0, step=0xffffffff, m=2) == INVALID
    assert status(first=0, step=1, m=(1 << 64) - 1) == INVALID and status(first=1, step=3, m=(1 << 63) + 5) == INVALID
    # the queries' ray limit: P D
    p = _params(cam, directions=4096)
    for a in range(3):
        p.cached.grid.count[a] = 1024
    assert _call(world, p, 1, b.args(False)) == INVALID
    # the bounce limit and the light object
    assert status(cached__path__bounce_limit=-1) == CAPACITY and status(cached__path__bounce_limit=MAX_BOUNCE_LIMIT + 1) == CAPACITY
    n_spheres = world.c.objs.num_spheres
    assert status(cached__path__light_obj_type=S.OBJ_SPHERE, cached__path__light_obj_idx=n_spheres) == INVALID
    assert status(cached__path__light_obj_type=S.OBJ_QUAD, cached__path__light_obj_idx=1 << 20) == INVALID
    assert b.untouched(), "a refused call writes nothing"
    # and the checks refuse nothing they should not
    b.streams[:] = 0
    assert status(hysteresis=0.0, first=3, step=7, m=3) == OK and status(True, cached__cache_depth=MAX_BOUNCE_LIMIT, first=P - 1, m=1) == OK


def test_overlapping_buffers_are_refused(scene):
    """every pair of an output with an input or another output; an in-place refresh among them"""
    world, cam = scene
    b = Buffers()
    a0 = b.args(True)
    sizes = dict(dirs=D * 12, streams=P * D * 48, records_in=P * 128, depth=P * 800, records_out=P * 128, ends=P * 4)
    big = np.full(sum(sizes.values()) + P * D * 48, FILL, dtype=np.uint8)  # room for any output laid over any other buffer
    p = _params(cam, True)
    for out in ("streams", "records_out", "ends"):
        for other in sizes:
            if other == out:
                continue
            for off in (0, sizes[other] - 4):  # the output's head on the other's head and on its last word
                assert _call(world, p, P, dict(a0, **{out: a0[other] + off})) == INVALID, (out, other, off)
            # the other's head on the output's last word
            if other not in ("dirs", "records_in", "depth"):
                continue
            base = big.ctypes.data
            assert _call(world, p, P, dict(a0, **{out: base, other: base + sizes[out] - 4})) == INVALID, (out, other, "tail")
    assert b.untouched() and (big == FILL).all()
    assert _call(world, _params(cam, False), P, dict(b.args(False), records_out=a0["records_in"])) == INVALID, "in place"
