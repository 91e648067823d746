"""The C ABI of the direct-light cached radiance queries (include/mort_hip.h) as far as it can be checked without a
GPU: every refusal of the cached calls repeated on the new entry points with the outputs at their fill, lit_out against every other
buffer, the empty batch and the optional counts.  The parameters are mort_cached_params, whose layout tests/test_cached_abi.py pins;
the _device form's alignment of lit_out needs a context and is in tests/test_gpu_cached_direct.py."""
import ctypes as C

import numpy as np
import pytest

from mort_amd import hip, host, structs as S

OK, INVALID, CAPACITY = 0, -1, -7
MAX_BOUNCE_LIMIT = 64
NAMES = ("mort_hip_query_radiance_cached_direct", "mort_hip_query_radiance_cached_direct_device", "mort_hip_query_radiance_cached_direct_host")


def test_exports_and_declarations():
    import os
    L = C.CDLL(hip.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mort_hip.h")).read()
    for name in NAMES:
        assert name in hip.EXPORTS and name + "(" in header
        getattr(L, name)


@pytest.fixture(scope="module")
def scene():
    return host.build_scene(2, width=16, spp=1)


N = 4
GRID = dict(origin=(-4.0, 0.0, -4.0), spacing=(4.0, 1.0, 2.0), count=(3, 2, 4))
FILL = 99


class Buffers:
    """rays that look down on scene 2's ground, streams, a volume of constant records, maps, outputs at their fill"""

    def __init__(self, n=N):
        self.rays = np.zeros(n, dtype=hip.RAY_DTYPE)
        self.rays["origin"] = (0, 1, 5); self.rays["dir"] = (0, -0.2, -1); self.rays["time"] = 0.5; self.rays["t_max"] = np.inf
        self.streams = np.full(n * 48, 7, dtype=np.uint8)
        g = hip.VOLUME_GRID(**GRID)
        self.records = np.zeros((g.probes, 32), dtype=np.float32)
        self.records[:, 0:3] = 1.0
        self.records[:, 27] = 1.0
        self.depth = np.ones((g.probes, 200), dtype=np.float32)
        self.rgb = np.full(3 * n, 7, dtype=np.float32)
        self.ends = np.full(n, FILL, dtype=np.uint32)
        self.lit = np.full(n, FILL, dtype=np.uint32)

    def args(self, visible, **kw):
        a = dict(rays=self.rays.ctypes.data, streams=self.streams.ctypes.data, records=self.records.ctypes.data,
                 depth=self.depth.ctypes.data if visible else None, rgb=self.rgb.ctypes.data, ends=self.ends.ctypes.data, lit=self.lit.ctypes.data)
        a.update(kw)
        return a

    def untouched(self):
        return (self.streams == 7).all() and (self.rgb == 7).all() and (self.ends == FILL).all() and (self.lit == FILL).all()


def _params(cam, visible=False, cache_depth=0, **kw):
    p = hip.CACHED_PARAMS(hip.radiance_params_from_camera(cam), cache_depth, hip.VOLUME_GRID(**GRID),
                          hip.VOLUME_VIS_PARAMS(0.01, 0.05) if visible else None)
    for k, v in kw.items():
        obj, _, field = k.rpartition("__")
        setattr(getattr(p, obj) if obj else p, field, v)
    return p


def _call(world, p, n, a, sec=None):
    return hip.lib().mort_hip_query_radiance_cached_direct_host(world.ptr if world is not None else None, C.byref(p) if p is not None else None, n,
                                                                a["rays"], a["streams"], a["records"], a["depth"], 1, 0, a["rgb"], a["ends"], a["lit"],
                                                                sec)


def _refused(world, p, n, b, a, status=INVALID):
    """the call is refused with `status` and has written nothing"""
    return _call(world, p, n, a) == status and b.untouched()


@pytest.mark.parametrize("visible", [False, True])
def test_a_valid_call_and_the_optional_counts(scene, visible):
    """scene 2 names no light object: every ray ends on the ground, in the volume, and nothing is lit"""
    world, cam = scene
    b = Buffers()
    assert _call(world, _params(cam, visible), N, b.args(visible)) == OK
    assert (b.ends == 1).all() and (b.lit == 0).all() and b.rgb.all()
    rgb = b.rgb.copy()
    for missing in (("ends",), ("lit",), ("ends", "lit")):
        b2 = Buffers()
        assert _call(world, _params(cam, visible), N, b2.args(visible, **{k: None for k in missing})) == OK, f"{missing} may be NULL"
        assert (b2.rgb == rgb).all()
        assert (b2.ends == (FILL if "ends" in missing else 1)).all() and (b2.lit == (FILL if "lit" in missing else 0)).all()
    out = hip.query_radiance_cached_direct_host(world, _params(cam, visible), b.rays, np.zeros(N * 48, dtype=np.uint8), b.records,
                                                b.depth if visible else None, want_ends=False, want_lit=False)
    assert out["ends"] is None and out["lit"] is None and (out["rgb"].reshape(-1) == rgb).all()


@pytest.mark.parametrize("visible", [False, True])
def test_empty_batch_is_ok(scene, visible):
    world, cam = scene
    b = Buffers(1)
    sec = C.c_double(5)
    assert _call(world, _params(cam, visible), 0, b.args(visible), C.byref(sec)) == OK
    assert b.untouched() and sec.value == 0, "nothing is written"
    out = hip.query_radiance_cached_direct_host(world, _params(cam, visible), np.zeros((0, 8), dtype=np.float32), np.zeros(0, dtype=np.uint8),
                                                b.records, b.depth if visible else None)
    assert out["rgb"].shape == (0, 3) and out["ends"].shape == (0,) and out["lit"].shape == (0,)


def test_null_arguments_are_invalid(scene):
    world, cam = scene
    L = hip.lib()
    b = Buffers()
    p = _params(cam)
    assert _refused(None, p, N, b, b.args(False))
    assert _refused(world, None, N, b, b.args(False))
    for k in ("rays", "streams", "records", "rgb"):
        assert _refused(world, p, N, b, b.args(False, **{k: None})), k
    a = b.args(False)
    # the forms that take a context check it before anything touches a GPU
    assert L.mort_hip_query_radiance_cached_direct(None, C.byref(p), N, a["rays"], a["streams"], a["records"], None, a["rgb"], a["ends"], a["lit"],
                                                   None) == INVALID
    assert L.mort_hip_query_radiance_cached_direct_device(None, C.byref(p), N, a["rays"], a["streams"], a["records"], None, a["rgb"], a["ends"],
                                                          a["lit"], None, None) == INVALID
    assert b.untouched()


def test_depth_goes_with_the_flag_and_no_new_flag_bit(scene):
    world, cam = scene
    b = Buffers()
    assert _refused(world, _params(cam, False), N, b, b.args(True)), "maps without MORT_CACHED_VISIBLE"
    assert _refused(world, _params(cam, True), N, b, b.args(False)), "MORT_CACHED_VISIBLE without maps"
    assert _refused(world, _params(cam, False, flags=2), N, b, b.args(False)), "an unknown flag bit"
    assert _refused(world, _params(cam, True, flags=3), N, b, b.args(True))
    assert _refused(world, _params(cam, True, flags=0x80000001), N, b, b.args(True))


def test_parameter_checks(scene):
    world, cam = scene
    b = Buffers()

    def status(visible=False, **kw):
        return _call(world, _params(cam, visible, **kw), N, b.args(visible))

    def refused(code, visible=False, **kw):
        return _refused(world, _params(cam, visible, **kw), N, b, b.args(visible), code)

    # the new fields
    assert refused(INVALID, cache_depth=-1) and refused(INVALID, cache_depth=MAX_BOUNCE_LIMIT + 1)
    # the radiance calls' checks
    assert refused(INVALID, path__samples=0)
    assert refused(CAPACITY, path__bounce_limit=-1) and refused(CAPACITY, path__bounce_limit=MAX_BOUNCE_LIMIT + 1)
    n_spheres = world.c.objs.num_spheres
    assert refused(INVALID, path__light_obj_type=S.OBJ_SPHERE, path__light_obj_idx=n_spheres)
    assert refused(INVALID, path__light_obj_type=S.OBJ_QUAD, path__light_obj_idx=1 << 20)
    # the volume calls' checks: counts 1 .. MORT_VOLUME_MAX_COUNT, spacing and origin
    for bad in (0, -1, hip.VOLUME_MAX_COUNT + 1):
        p = _params(cam)
        p.grid.count[1] = bad
        assert _refused(world, p, N, b, b.args(False)), bad
    for bad in (0.0, -1.0, np.inf, np.nan):
        p = _params(cam)
        p.grid.spacing[2] = bad
        assert _refused(world, p, N, b, b.args(False)), bad
    p = _params(cam)
    p.grid.origin[0] = np.nan
    assert _refused(world, p, N, b, b.args(False))
    # the visibility parameters, read only with the flag
    for k, bad in (("normal_bias", -0.5), ("normal_bias", np.nan), ("min_visibility", -0.1), ("min_visibility", 1.5), ("min_visibility", np.inf)):
        assert refused(INVALID, True, **{"vis__" + k: bad}), (k, bad)
    # and what the checks must let through
    assert status() == OK and status(True) == OK
    assert status(cache_depth=MAX_BOUNCE_LIMIT) == OK and status(path__bounce_limit=0) == OK
    assert status(path__light_obj_type=S.OBJ_SPHERE, path__light_obj_idx=0) == OK
    for k, bad in (("normal_bias", -0.5), ("min_visibility", 1.5)):
        assert status(False, **{"vis__" + k: bad}) == OK, (k, bad)


def test_overlapping_buffers_are_refused(scene):
    world, cam = scene
    n = 8
    b = Buffers(n)
    g = hip.VOLUME_GRID(**GRID)
    buf = np.zeros(n * (32 + 48 + 12 + 4 + 4) + 64, dtype=np.uint8)
    base = buf.ctypes.data
    buf[:n * 32].view(hip.RAY_DTYPE)[:] = b.rays
    rays, streams, rgb, ends, lit = base, base + n * 32, base + n * 80, base + n * 92, base + n * 96  # side by side
    rec, dep = b.records.ctypes.data, b.depth.ctypes.data
    before = buf.copy()

    def status(visible=False, **kw):
        a = dict(rays=rays, streams=streams, records=rec, depth=dep if visible else None, rgb=rgb, ends=ends, lit=lit)
        a.update(kw)
        return _call(world, _params(cam, visible), n, a)

    # the cached calls' overlaps
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
    # lit_out over each input and each other output
    assert status(lit=rays) == INVALID and status(lit=rays + n * 32 - 4) == INVALID
    assert status(lit=rec) == INVALID and status(lit=rec + g.probes * 128 - 4) == INVALID
    assert status(True, lit=dep) == INVALID and status(True, lit=dep + g.probes * 800 - 4) == INVALID
    assert status(lit=streams) == INVALID and status(lit=streams + n * 48 - 4) == INVALID
    assert status(lit=rgb) == INVALID and status(lit=rgb + n * 12 - 4) == INVALID
    assert status(lit=ends) == INVALID and status(lit=ends + n * 4 - 4) == INVALID and status(lit=ends - 4) == INVALID
    assert status(ends=lit + n * 4 - 4) == INVALID
    assert (buf == before).all() and b.untouched(), "a refused call writes nothing"
    # maps that the call does not read may lie anywhere
    assert status() == OK and status(True) == OK
