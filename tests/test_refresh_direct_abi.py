"""The C ABI of the direct-light volume refresh (include/mort_hip.h) as far as it can be checked without a GPU:
the exports, every refusal of the plain refresh with the outputs still at their fill, lit_out against every other buffer, and the
empty selection.  Buffers, parameters and the fill are tests/test_refresh_abi.py's."""
import ctypes as C

import numpy as np
import pytest

from mort_amd import hip, host, structs as S
from tests import test_refresh_abi as RA

OK, INVALID, CAPACITY = RA.OK, RA.INVALID, RA.CAPACITY
P, D, FILL = RA.P, RA.D, RA.FILL
_params = RA._params


def test_exports():
    L = C.CDLL(hip.LIB_PATH)
    for name in ("mort_hip_volume_refresh_direct", "mort_hip_volume_refresh_direct_device", "mort_hip_volume_refresh_direct_host"):
        assert name in hip.EXPORTS
        getattr(L, name)


@pytest.fixture(scope="module")
def scene():
    return host.build_scene(2, width=16, spp=1)


class Buffers(RA.Buffers):
    """the plain refresh's buffers and the second count, at the fill"""

    def __init__(self):
        super().__init__()
        self.lit = np.full(P * 4, FILL, dtype=np.uint8)

    def args(self, visible, **kw):
        a = dict(lit=self.lit.ctypes.data)
        a.update(kw)
        return super().args(visible, **a)

    def untouched(self):
        return super().untouched() and (self.lit == FILL).all()


def _call(world, p, m, a, sec=None):
    return hip.lib().mort_hip_volume_refresh_direct_host(world.ptr if world is not None else None, C.byref(p) if p is not None else None, m,
                                                         a["dirs"], a["streams"], a["records_in"], a["depth"], 1, 0, a["records_out"], a["ends"],
                                                         a["lit"], sec)


@pytest.mark.parametrize("visible", [False, True])
def test_a_valid_call_and_the_optional_arguments(scene, visible):
    world, cam = scene
    b = Buffers()
    b.streams[:] = 0
    assert _call(world, _params(cam, visible), P, b.args(visible)) == OK
    rec = b.out.view(np.float32).reshape(P, 32)
    assert (rec[:, 27] == 1.0).all() and (rec[:, 28:] == 0.0).all() and rec[:, :3].all()
    assert (b.ends.view(np.uint32) > 0).all(), "every probe looks down on the ground, in the volume"
    assert (b.lit.view(np.uint32) == 0).all(), "scene 2 has no light"
    b2 = Buffers()
    b2.streams[:] = 0
    assert _call(world, _params(cam, visible), P, b2.args(visible, ends=None, lit=None, dirs=None)) == OK, "both counts and dirs may be NULL"
    assert (b2.out == b.out).all() and (b2.ends == FILL).all() and (b2.lit == FILL).all()


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
    assert L.mort_hip_volume_refresh_direct(None, C.byref(p), P, a["dirs"], a["streams"], a["records_in"], None, a["records_out"], a["ends"],
                                            a["lit"], None) == INVALID
    assert L.mort_hip_volume_refresh_direct_device(None, C.byref(p), P, a["dirs"], a["streams"], a["records_in"], None, a["records_out"], a["ends"],
                                                   a["lit"], None, None) == INVALID
    assert b.untouched()


def test_parameter_checks(scene):
    """the plain refresh's list, in its order"""
    world, cam = scene
    b = Buffers()

    def status(visible=False, m=P, **kw):
        return _call(world, _params(cam, visible, **kw), m, b.args(visible))

    for bad in (0, 63, 65, 96, 4160, -64):
        assert status(directions=bad) == INVALID, bad
    assert status(cached__path__samples=0) == INVALID
    assert status(False, cached__flags=2) == INVALID and status(True, cached__flags=3) == INVALID
    assert _call(world, _params(cam, False), P, b.args(True)) == INVALID, "maps without MORT_CACHED_VISIBLE"
    assert _call(world, _params(cam, True), P, b.args(False)) == INVALID, "MORT_CACHED_VISIBLE without maps"
    assert status(cached__cache_depth=-1) == INVALID and status(cached__cache_depth=RA.MAX_BOUNCE_LIMIT + 1) == INVALID
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
    for bad in (np.nan, -0.25, -np.inf, 1.0, 1.5, np.inf):
        assert status(hysteresis=bad) == INVALID, bad
    assert status(step=0) == INVALID
    assert status(first=P, m=1) == INVALID and status(first=1) == INVALID and status(step=2) == INVALID
    assert status(first=3, step=7, m=4) == INVALID
    assert status(first=0xffffffff, step=0xffffffff, m=2) == INVALID and status(first=0, step=0xffffffff, m=2) == INVALID
    assert status(first=0, step=1, m=(1 << 64) - 1) == INVALID and status(first=1, step=3, m=(1 << 63) + 5) == INVALID
    p = _params(cam, directions=4096)
    for a in range(3):
        p.cached.grid.count[a] = 1024
    assert _call(world, p, 1, b.args(False)) == INVALID
    assert status(cached__path__bounce_limit=-1) == CAPACITY and status(cached__path__bounce_limit=RA.MAX_BOUNCE_LIMIT + 1) == CAPACITY
    # an overlap is reported before the bounce limit, as the plain refresh orders them
    p = _params(cam, cached__path__bounce_limit=-1)
    assert _call(world, p, P, b.args(False, lit=b.ends.ctypes.data)) == INVALID
    n_spheres = world.c.objs.num_spheres
    assert status(cached__path__light_obj_type=S.OBJ_SPHERE, cached__path__light_obj_idx=n_spheres) == INVALID
    assert status(cached__path__light_obj_type=S.OBJ_QUAD, cached__path__light_obj_idx=1 << 20) == INVALID
    assert b.untouched(), "a refused call writes nothing"
    b.streams[:] = 0
    assert status(hysteresis=0.0, first=3, step=7, m=3) == OK and status(True, cached__cache_depth=RA.MAX_BOUNCE_LIMIT, first=P - 1, m=1) == OK


def test_overlapping_buffers_are_refused(scene):
    """every pair of an output with an input or another output, lit_out among the outputs; an in-place refresh among them"""
    world, cam = scene
    b = Buffers()
    a0 = b.args(True)
    sizes = dict(dirs=D * 12, streams=P * D * 48, records_in=P * 128, depth=P * 800, records_out=P * 128, ends=P * 4, lit=P * 4)
    big = np.full(sum(sizes.values()) + P * D * 48, FILL, dtype=np.uint8)  # room for any output laid over any other buffer
    p = _params(cam, True)
    for out in ("streams", "records_out", "ends", "lit"):
        for other in sizes:
            if other == out:
                continue
            for off in (0, sizes[other] - 4):  # the output's head on the other's head and on its last word
                assert _call(world, p, P, dict(a0, **{out: a0[other] + off})) == INVALID, (out, other, off)
            base = big.ctypes.data  # the other's head on the output's last word
            assert _call(world, p, P, dict(a0, **{out: base, other: base + sizes[out] - 4})) == INVALID, (out, other, "tail")
    assert b.untouched() and (big == FILL).all()
    assert _call(world, _params(cam, False), P, dict(b.args(False), records_out=a0["records_in"])) == INVALID, "in place"
    # lit_out beside the others, touching none, is fine
    b.streams[:] = 0
    assert _call(world, p, P, b.args(True)) == OK
