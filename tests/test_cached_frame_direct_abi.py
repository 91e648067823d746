"""The C ABI of the direct-light cached frames (include/mort_hip.h): the exports, the cached frame's refusals
repeated through the host form with every output left at its fill, and `lit` overlapping every other buffer.  No GPU; the
partition's refusal needs a context and is marked gpu."""
import ctypes as C

import numpy as np
import pytest

from mort_amd import hip, host, structs as S

OK, INVALID, UNSUPPORTED, CAPACITY = 0, -1, -6, -7
MAX_BOUNCE_LIMIT = 64
FILL = 0xa5
NAMES = ("mort_hip_render_cached_direct", "mort_hip_render_cached_direct_device", "mort_hip_render_cached_direct_host",
         "mort_hip_view_set_cache_direct", "mort_hip_view_set_cache_direct_host")
GRID = dict(origin=(-4.0, 0.0, -4.0), spacing=(4.0, 1.0, 2.0), count=(3, 2, 4))


def test_exports():
    L = C.CDLL(hip.LIB_PATH)
    for name in NAMES:
        assert name in hip.EXPORTS
        getattr(L, name)
    assert hip.VIEW_BUFFERS["lit"] == (9, 1) and C.sizeof(hip.CACHED_FRAME_PARAMS) == 56, "no new flag bit, no new field"


@pytest.fixture(scope="module")
def scene():
    world, cam = host.build_scene(2, width=8, spp=4)
    cam = S.Camera.from_buffer_copy(cam)
    cam.light_obj_type, cam.light_obj_idx = S.OBJ_SPHERE, 0  # any primitive may be sampled; what it emits is the census' business
    return world, cam


class Buffers:
    """streams, a volume of constant records, maps, outputs (filled) for a W x H frame"""

    def __init__(self, cam):
        self.n = n = cam.image_width * cam.image_height
        self.streams = hip.seed_states_host(7, cam.image_width, cam.image_height)
        g = hip.VOLUME_GRID(**GRID)
        self.records = np.zeros((g.probes, 32), dtype=np.float32)
        self.records[:, 0:3] = 1.0
        self.records[:, 27] = 1.0
        self.depth = np.ones((g.probes, 200), dtype=np.float32)
        self.rgba = np.full(4 * n, FILL, dtype=np.uint8)
        self.accum = np.full(12 * n, FILL, dtype=np.uint8)
        self.seg = np.full(4 * n, FILL, dtype=np.uint8)
        self.ends = np.full(4 * n, FILL, dtype=np.uint8)
        self.lit = np.full(4 * n, FILL, dtype=np.uint8)
        self.streams0 = self.streams.copy()

    def args(self, visible, **kw):
        a = dict(streams=self.streams.ctypes.data, records=self.records.ctypes.data, depth=self.depth.ctypes.data if visible else None,
                 rgba=self.rgba.ctypes.data, accum=self.accum.ctypes.data, seg=self.seg.ctypes.data, ends=self.ends.ctypes.data,
                 lit=self.lit.ctypes.data)
        a.update(kw)
        return a

    def untouched(self):
        return all((x == FILL).all() for x in (self.rgba, self.accum, self.seg, self.ends, self.lit)) and (self.streams == self.streams0).all()


def _params(visible=False, cache_depth=0, **kw):
    p = hip.CACHED_FRAME_PARAMS(cache_depth, hip.VOLUME_GRID(**GRID), hip.VOLUME_VIS_PARAMS(0.01, 0.05) if visible else None)
    for k, v in kw.items():
        obj, _, field = k.rpartition("__")
        setattr(getattr(p, obj) if obj else p, field, v)
    return p


def _camera(cam, **kw):
    c = S.Camera.from_buffer_copy(cam)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _call(world, cam, p, a, stats=None):
    return hip.lib().mort_hip_render_cached_direct_host(world.ptr if world is not None else None, C.byref(cam) if cam is not None else None,
                                                        a["streams"], 1, 0, C.byref(p) if p is not None else None, a["records"], a["depth"], a["rgba"],
                                                        a["accum"], a["seg"], a["ends"], a["lit"], stats)


@pytest.mark.parametrize("visible", [False, True])
def test_a_valid_call_and_the_optional_outputs(scene, visible):
    world, cam = scene
    b = Buffers(cam)
    st = hip.Stats()
    assert _call(world, cam, _params(visible), b.args(visible), C.byref(st)) == OK
    ends, lit, seg = b.ends.view(np.uint32), b.lit.view(np.uint32), b.seg.view(np.uint32)
    assert (lit <= ends).all() and (ends <= 4).all() and ends.any() and b.rgba.reshape(-1, 4)[:, 3].all()
    assert st.segments == seg.sum() and st.pixels == b.n and st.eff_samples == 4 * b.n and st.scene_in_lds == 0 and st.reference_walks == 0
    assert b"cached frame, direct" in bytes(st.kernel_name)
    b2 = Buffers(cam)
    assert _call(world, cam, _params(visible), b2.args(visible, accum=None, seg=None, ends=None, lit=None)) == OK, "the optional outputs may be NULL"
    assert (b2.rgba == b.rgba).all() and (b2.streams == b.streams).all()
    assert all((x == FILL).all() for x in (b2.accum, b2.seg, b2.ends, b2.lit))


def test_null_arguments_are_invalid(scene):
    world, cam = scene
    L = hip.lib()
    b = Buffers(cam)
    p = _params()
    assert _call(None, cam, p, b.args(False)) == INVALID
    assert _call(world, None, p, b.args(False)) == INVALID
    assert _call(world, cam, None, b.args(False)) == INVALID
    for k in ("streams", "records", "rgba"):
        assert _call(world, cam, p, b.args(False, **{k: None})) == INVALID, k
    a = b.args(False)
    # the forms that take a context check it before anything touches a GPU
    assert L.mort_hip_render_cached_direct(None, C.byref(cam), C.byref(p), a["records"], None, a["rgba"], a["accum"], a["seg"], a["ends"], a["lit"],
                                           None) == INVALID
    assert L.mort_hip_render_cached_direct_device(None, C.byref(cam), C.byref(p), a["records"], None, a["rgba"], a["accum"], a["ends"], a["lit"], None,
                                                  None) == INVALID
    assert L.mort_hip_view_set_cache_direct(None, C.byref(p), a["records"], None) == INVALID
    assert L.mort_hip_view_set_cache_direct_host(None, C.byref(p), a["records"], None) == INVALID
    assert b.untouched()


def test_depth_goes_with_the_flag(scene):
    world, cam = scene
    b = Buffers(cam)
    assert _call(world, cam, _params(False), b.args(True)) == INVALID, "maps without MORT_CACHED_VISIBLE"
    assert _call(world, cam, _params(True), b.args(False)) == INVALID, "MORT_CACHED_VISIBLE without maps"
    assert _call(world, cam, _params(False, flags=2), b.args(False)) == INVALID, "an unknown flag bit: the direct frames have none of their own"
    assert _call(world, cam, _params(True, flags=3), b.args(True)) == INVALID
    assert _call(world, cam, _params(True, flags=0x80000001), b.args(True)) == INVALID
    assert b.untouched()


def test_parameter_checks(scene):
    world, cam = scene
    b = Buffers(cam)

    def status(visible=False, cam_kw=None, **kw):
        return _call(world, _camera(cam, **(cam_kw or {})), _params(visible, **kw), b.args(visible))

    assert status(cache_depth=-1) == INVALID and status(cache_depth=MAX_BOUNCE_LIMIT + 1) == INVALID
    assert status(cam_kw=dict(image_width=0)) == INVALID and status(cam_kw=dict(image_height=-1)) == INVALID
    assert status(cam_kw=dict(sqrt_spp=-1)) == INVALID
    assert status(cam_kw=dict(bounce_limit=-1)) == CAPACITY and status(cam_kw=dict(bounce_limit=MAX_BOUNCE_LIMIT + 1)) == CAPACITY
    n_spheres = world.c.objs.num_spheres
    assert status(cam_kw=dict(light_obj_type=S.OBJ_SPHERE, light_obj_idx=n_spheres)) == INVALID
    assert status(cam_kw=dict(light_obj_type=S.OBJ_QUAD, light_obj_idx=1 << 20)) == INVALID
    for bad in (0, -1, hip.VOLUME_MAX_COUNT + 1):
        p = _params()
        p.grid.count[1] = bad
        assert _call(world, cam, p, b.args(False)) == INVALID, bad
    for bad in (0.0, -1.0, np.inf, np.nan):
        p = _params()
        p.grid.spacing[2] = bad
        assert _call(world, cam, p, b.args(False)) == INVALID, bad
    p = _params()
    p.grid.origin[0] = np.nan
    assert _call(world, cam, p, b.args(False)) == INVALID
    for k, bad in (("normal_bias", -0.5), ("normal_bias", np.nan), ("min_visibility", -0.1), ("min_visibility", 1.5), ("min_visibility", np.inf)):
        assert status(True, **{"vis__" + k: bad}) == INVALID, (k, bad)
    assert b.untouched(), "a refused call writes nothing"
    # and the checks refuse nothing they should not
    assert status(cache_depth=MAX_BOUNCE_LIMIT) == OK and status(cam_kw=dict(bounce_limit=0)) == OK and status(True) == OK
    assert status(cam_kw=dict(light_obj_type=-1, light_obj_idx=0)) == OK
    assert status(False, vis__min_visibility=1.5) == OK, "read only with the flag"


def test_overlapping_buffers_are_refused(scene):
    world, cam = scene
    b = Buffers(cam)
    n = b.n
    g = hip.VOLUME_GRID(**GRID)
    buf = np.zeros(n * (48 + 4 + 12 + 4 + 4 + 4) + 64, dtype=np.uint8)
    base = buf.ctypes.data
    streams, rgba, accum, seg, ends, lit = base, base + n * 48, base + n * 52, base + n * 64, base + n * 68, base + n * 72  # side by side
    rec, dep = b.records.ctypes.data, b.depth.ctypes.data

    def status(visible=False, **kw):
        a = dict(streams=streams, records=rec, depth=dep if visible else None, rgba=rgba, accum=accum, seg=seg, ends=ends, lit=lit)
        a.update(kw)
        buf[:] = 0
        buf[:n * 48] = b.streams0
        st = _call(world, cam, _params(visible), a)
        assert st == OK or not buf[n * 48:].any(), "a refused call writes nothing"
        return st

    assert status() == OK and status(True) == OK
    # the cached frame's
    assert status(rgba=streams + n * 48 - 4) == INVALID and status(accum=rgba + n * 4 - 4) == INVALID
    assert status(seg=accum + n * 12 - 4) == INVALID and status(ends=seg + n * 4 - 4) == INVALID
    assert status(ends=streams) == INVALID and status(ends=rgba) == INVALID and status(rgba=rec + g.probes * 128 - 4) == INVALID
    # lit over every other buffer: the whole of it, its tail, its head
    for name, at, size in (("streams", streams, n * 48), ("rgba", rgba, n * 4), ("accum", accum, n * 12), ("seg", seg, n * 4), ("ends", ends, n * 4),
                           ("records", rec, g.probes * 128)):
        assert status(lit=at) == INVALID, name
        assert status(lit=at + size - 4) == INVALID, name + " tail"
        assert status(lit=at - n * 4 + 4) == INVALID, name + " head"
    for at in (dep, dep + g.probes * 800 - 4, dep - n * 4 + 4):
        assert status(True, lit=at) == INVALID
    assert status(False, lit=dep) == OK, "maps that the call does not read"
    assert status(lit=None) == OK


@pytest.mark.gpu
def test_only_the_whole_image_partition(scene):
    """a partition other than the whole image is MORT_ERR_UNSUPPORTED for both forms that take a context"""
    import torch
    world, cam = scene
    W, H = cam.image_width, cam.image_height
    b = Buffers(cam)
    p = _params()
    dev = torch.device("cuda:0")
    rec = torch.from_numpy(b.records).to(dev)
    rgba = torch.zeros(4 * b.n, dtype=torch.uint8, device=dev)
    lit = torch.zeros(4 * b.n, dtype=torch.uint8, device=dev)
    with hip.Context(0) as ctx:
        ctx.upload_world(world)
        ctx.set_partition(0, 2)
        ctx.rng_seed(7, W, H)
        with pytest.raises(hip.MortHipError) as e:
            ctx.render_cached_direct(cam, p, b.records)
        assert e.value.status == UNSUPPORTED
        with pytest.raises(hip.MortHipError) as e:
            ctx.render_cached_direct_device(cam, p, rec, None, rgba, lit=lit, sync=True)
        assert e.value.status == UNSUPPORTED
        assert not rgba.any().item() and not lit.any().item(), "a refused call writes nothing"
        ctx.set_partition(0, 1)
        ctx.rng_seed(7, W, H)
        got = ctx.render_cached_direct(cam, p, b.records)
    want = hip.render_cached_direct_host(world, cam, p, b.records, states=b.streams0)
    assert (got["rgba"] == want["rgba"]).all() and (got["ends_px"] == want["ends_px"]).all() and (got["lit_px"] == want["lit_px"]).all()
