"""The C ABI of the cached frames (include/mort_hip.h): the layout of mort_cached_frame_params, every refusal the
contract lists and the overlap refusals through the host form, which needs no GPU; the partition's refusal needs a context and is
marked gpu."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mort_amd import hip, host, structs as S

OK, INVALID, UNSUPPORTED, CAPACITY = 0, -1, -6, -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_BOUNCE_LIMIT = 64
FIELDS = ("cache_depth", "flags", "grid", "vis")
NAMES = ("mort_hip_render_cached", "mort_hip_render_cached_device", "mort_hip_render_cached_host", "mort_hip_view_set_cache",
         "mort_hip_view_set_cache_host")


def test_layout_as_the_header_declares_it(tmp_path):
    """sizeof and offsetof from the header itself, compiled as C, against the ctypes structure of the binding"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mort_hip.h"\n'
                   'int main(void) { printf("%zu ' + "%zu " * len(FIELDS) + '\\n", sizeof(mort_cached_frame_params), ' +
                   ", ".join(f"offsetof(mort_cached_frame_params, {k})" for k in FIELDS) + '); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "cc"), "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    assert got == [56, 0, 4, 8, 48]
    P = hip.CACHED_FRAME_PARAMS
    assert [C.sizeof(P)] + [getattr(P, k).offset for k in FIELDS] == got


def test_exports():
    L = C.CDLL(hip.LIB_PATH)
    for name in NAMES:
        assert name in hip.EXPORTS
        getattr(L, name)


@pytest.fixture(scope="module")
def scene():
    return host.build_scene(2, width=8, spp=4)


GRID = dict(origin=(-4.0, 0.0, -4.0), spacing=(4.0, 1.0, 2.0), count=(3, 2, 4))


class Buffers:
    """streams, a volume of constant records, maps, outputs for a W x H frame"""

    def __init__(self, cam):
        self.n = n = cam.image_width * cam.image_height
        self.streams = hip.seed_states_host(7, cam.image_width, cam.image_height)
        g = hip.VOLUME_GRID(**GRID)
        self.records = np.zeros((g.probes, 32), dtype=np.float32)
        self.records[:, 0:3] = 1.0
        self.records[:, 27] = 1.0
        self.depth = np.ones((g.probes, 200), dtype=np.float32)
        self.rgba = np.zeros(4 * n, dtype=np.uint8)
        self.accum = np.zeros(3 * n, dtype=np.float32)
        self.seg = np.zeros(n, dtype=np.uint32)
        self.ends = np.full(n, 99, dtype=np.uint32)

    def args(self, visible, **kw):
        a = dict(streams=self.streams.ctypes.data, records=self.records.ctypes.data, depth=self.depth.ctypes.data if visible else None,
                 rgba=self.rgba.ctypes.data, accum=self.accum.ctypes.data, seg=self.seg.ctypes.data, ends=self.ends.ctypes.data)
        a.update(kw)
        return a


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
    return hip.lib().mort_hip_render_cached_host(world.ptr if world is not None else None, C.byref(cam) if cam is not None else None, a["streams"], 1, 0,
                                                 C.byref(p) if p is not None else None, a["records"], a["depth"], a["rgba"], a["accum"], a["seg"],
                                                 a["ends"], stats)


@pytest.mark.parametrize("visible", [False, True])
def test_a_valid_call_and_the_optional_outputs(scene, visible):
    world, cam = scene
    b = Buffers(cam)
    st = hip.Stats()
    assert _call(world, cam, _params(visible), b.args(visible), C.byref(st)) == OK
    assert (b.ends <= 4).all() and b.ends.any() and b.rgba.reshape(-1, 4)[:, 3].all()
    assert st.segments == b.seg.sum() and st.pixels == b.n and st.eff_samples == 4 * b.n and st.scene_in_lds == 0 and st.reference_walks == 0
    b2 = Buffers(cam)
    assert _call(world, cam, _params(visible), b2.args(visible, accum=None, seg=None, ends=None)) == OK, "the optional outputs may be NULL"
    assert (b2.rgba == b.rgba).all() and (b2.ends == 99).all() and not b2.accum.any() and (b2.streams == b.streams).all()


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
    assert L.mort_hip_render_cached(None, C.byref(cam), C.byref(p), a["records"], None, a["rgba"], a["accum"], a["seg"], a["ends"], None) == INVALID
    assert L.mort_hip_render_cached_device(None, C.byref(cam), C.byref(p), a["records"], None, a["rgba"], a["accum"], a["ends"], None, None) == INVALID
    assert L.mort_hip_view_set_cache(None, C.byref(p), a["records"], None) == INVALID
    assert L.mort_hip_view_set_cache_host(None, C.byref(p), a["records"], None) == INVALID


def test_depth_goes_with_the_flag(scene):
    world, cam = scene
    b = Buffers(cam)
    assert _call(world, cam, _params(False), b.args(True)) == INVALID, "maps without MORT_CACHED_VISIBLE"
    assert _call(world, cam, _params(True), b.args(False)) == INVALID, "MORT_CACHED_VISIBLE without maps"
    assert _call(world, cam, _params(False, flags=2), b.args(False)) == INVALID, "an unknown flag bit"
    assert _call(world, cam, _params(True, flags=3), b.args(True)) == INVALID
    assert _call(world, cam, _params(True, flags=0x80000001), b.args(True)) == INVALID


def test_parameter_checks(scene):
    world, cam = scene
    b = Buffers(cam)

    def status(visible=False, cam_kw=None, **kw):
        return _call(world, _camera(cam, **(cam_kw or {})), _params(visible, **kw), b.args(visible))

    assert status() == OK and status(True) == OK
    # the new fields
    assert status(cache_depth=-1) == INVALID and status(cache_depth=MAX_BOUNCE_LIMIT + 1) == INVALID
    assert status(cache_depth=MAX_BOUNCE_LIMIT) == OK
    # the render's checks of the camera
    assert status(cam_kw=dict(image_width=0)) == INVALID and status(cam_kw=dict(image_height=-1)) == INVALID
    assert status(cam_kw=dict(sqrt_spp=-1)) == INVALID
    assert status(cam_kw=dict(bounce_limit=-1)) == CAPACITY and status(cam_kw=dict(bounce_limit=MAX_BOUNCE_LIMIT + 1)) == CAPACITY
    assert status(cam_kw=dict(bounce_limit=0)) == OK
    n_spheres = world.c.objs.num_spheres
    assert status(cam_kw=dict(light_obj_type=S.OBJ_SPHERE, light_obj_idx=n_spheres)) == INVALID
    assert status(cam_kw=dict(light_obj_type=S.OBJ_QUAD, light_obj_idx=1 << 20)) == INVALID
    assert status(cam_kw=dict(light_obj_type=S.OBJ_SPHERE, light_obj_idx=0)) == OK
    # the volume calls' checks: counts 1 .. MORT_VOLUME_MAX_COUNT, spacing and origin
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
    # the visibility parameters, read only with the flag
    for k, bad in (("normal_bias", -0.5), ("normal_bias", np.nan), ("min_visibility", -0.1), ("min_visibility", 1.5), ("min_visibility", np.inf)):
        assert status(True, **{"vis__" + k: bad}) == INVALID, (k, bad)
        assert status(False, **{"vis__" + k: bad}) == OK, (k, bad)


def test_overlapping_buffers_are_refused(scene):
    world, cam = scene
    b = Buffers(cam)
    n = b.n
    g = hip.VOLUME_GRID(**GRID)
    buf = np.zeros(n * (48 + 4 + 12 + 4 + 4) + 64, dtype=np.uint8)
    base = buf.ctypes.data
    buf[:n * 48] = b.streams
    streams, rgba, accum, seg, ends = base, base + n * 48, base + n * 52, base + n * 64, base + n * 68  # side by side
    rec, dep = b.records.ctypes.data, b.depth.ctypes.data

    def status(visible=False, **kw):
        a = dict(streams=streams, records=rec, depth=dep if visible else None, rgba=rgba, accum=accum, seg=seg, ends=ends)
        a.update(kw)
        buf[:n * 48] = b.streams
        return _call(world, cam, _params(visible), a)

    assert status() == OK and status(True) == OK
    assert status(rgba=streams + n * 48 - 4) == INVALID       # the image over the streams' tail
    assert status(accum=rgba + n * 4 - 4) == INVALID          # accumulators over the image's tail
    assert status(seg=accum + n * 12 - 4) == INVALID          # segments over the accumulators' tail
    assert status(ends=seg + n * 4 - 4) == INVALID            # counts over the segments' tail
    assert status(ends=streams) == INVALID                    # counts over the streams
    assert status(ends=rgba) == INVALID                       # counts over the image
    assert status(rgba=rec + g.probes * 128 - 4) == INVALID   # the image over the records' tail
    assert status(accum=rec) == INVALID and status(seg=rec) == INVALID and status(ends=rec) == INVALID and status(streams=rec) == INVALID
    assert status(True, rgba=dep + g.probes * 800 - 4) == INVALID  # the image over the maps' tail
    assert status(True, ends=dep) == INVALID and status(True, accum=dep + 800) == INVALID


@pytest.mark.gpu
def test_only_the_whole_image_partition(scene):
    """a partition other than the whole image is MORT_ERR_UNSUPPORTED, as for a view, for both forms that take a context"""
    import torch
    world, cam = scene
    W, H = cam.image_width, cam.image_height
    b = Buffers(cam)
    p = _params()
    dev = torch.device("cuda:0")
    rec = torch.from_numpy(b.records).to(dev)
    rgba = torch.zeros(4 * b.n, dtype=torch.uint8, device=dev)
    with hip.Context(0) as ctx:
        ctx.upload_world(world)
        ctx.set_partition(0, 2)
        ctx.rng_seed(7, W, H)
        with pytest.raises(hip.MortHipError) as e:
            ctx.render_cached(cam, p, b.records)
        assert e.value.status == UNSUPPORTED
        with pytest.raises(hip.MortHipError) as e:
            ctx.render_cached_device(cam, p, rec, None, rgba, sync=True)
        assert e.value.status == UNSUPPORTED
        assert not rgba.any().item(), "a refused call writes nothing"
        ctx.set_partition(0, 1)
        ctx.rng_seed(7, W, H)
        got = ctx.render_cached(cam, p, b.records)
    want = hip.render_cached_host(world, cam, p, b.records, states=b.streams)
    assert (got["rgba"] == want["rgba"]).all() and (got["ends_px"] == want["ends_px"]).all()
