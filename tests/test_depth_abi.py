"""The C ABI of the visibility-weighted irradiance volumes (include/mort_hip.h) as far as it can be checked without a
GPU: the layout of mort_depth_params, mort_volume_vis_params and a depth map, every status code of the host forms, the refusal of
overlapping buffers and the empty batch."""
import ctypes as C
import os
import subprocess

import numpy as np

from mort_amd import hip, host

OK, INVALID = 0, -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = ("mort_hip_probe_depth_bake", "mort_hip_probe_depth_bake_device", "mort_hip_probe_depth_bake_host",
         "mort_hip_volume_sample_visible", "mort_hip_volume_sample_visible_device", "mort_hip_volume_sample_visible_host")


def test_layout_as_the_header_declares_it(tmp_path):
    """sizeof and offsetof from the header itself, compiled as C, against the ctypes structures of the binding: 8, 8 and 800 bytes"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mort_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %d %zu\\n", sizeof(mort_depth_params), offsetof(mort_depth_params, subsamples), '
                   'offsetof(mort_depth_params, max_distance), sizeof(mort_volume_vis_params), offsetof(mort_volume_vis_params, normal_bias), '
                   'offsetof(mort_volume_vis_params, min_visibility), MORT_DEPTH_RES, MORT_DEPTH_FLOATS * sizeof(float)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "cc"), "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    assert got == [8, 0, 4, 8, 0, 4, 8, 800]
    P, V = hip.DEPTH_PARAMS, hip.VOLUME_VIS_PARAMS
    assert C.sizeof(P) == 8 and (P.subsamples.offset, P.max_distance.offset) == (0, 4)
    assert C.sizeof(V) == 8 and (V.normal_bias.offset, V.min_visibility.offset) == (0, 4)
    assert hip.DEPTH_FLOATS == 200 and hip.DEPTH_RES == 8 and hip.DEPTH_FLOATS == 2 * (hip.DEPTH_RES + 2) ** 2


def test_exports():
    L = C.CDLL(hip.LIB_PATH)
    for name in NAMES:
        assert name in hip.EXPORTS
        getattr(L, name)


# ---------------------------------------------------------------------------------------------------------------- the bake

def _world():
    return host.build_scene(6, width=16, spp=1)[0]


def _bake(world, params, n, probes, depth, sec=None, nthreads=1, flags=0):
    return hip.lib().mort_hip_probe_depth_bake_host(world.ptr if world is not None else None, C.byref(params) if params is not None else None, n,
                                                    probes, nthreads, flags, depth, sec)


def test_bake_status_codes():
    L = hip.lib()
    w = _world()
    n = 2
    probes = np.zeros(n, dtype=hip.PROBE_DTYPE)
    probes["position"] = (278, 278, 278)
    depth = np.zeros(n * 200, dtype=F)
    p, d = probes.ctypes.data, depth.ctypes.data
    good = hip.DEPTH_PARAMS(1, 100.0)
    assert _bake(w, good, n, p, d) == OK and depth.all()
    depth[:] = 0
    assert _bake(None, good, n, p, d) == INVALID
    assert _bake(w, None, n, p, d) == INVALID
    assert _bake(w, good, n, None, d) == INVALID
    assert _bake(w, good, n, p, None) == INVALID
    for s in (0, -1, 9, 1 << 30):
        assert _bake(w, hip.DEPTH_PARAMS(s, 100.0), n, p, d) == INVALID, s
    for s in (1, 8):
        assert _bake(w, hip.DEPTH_PARAMS(s, 100.0), 1, p, d) == OK, s
    depth[:] = 0
    for mx in (0.0, -0.0, -1.0, np.inf, -np.inf, np.nan):
        assert _bake(w, hip.DEPTH_PARAMS(1, mx), n, p, d) == INVALID, mx
    assert _bake(w, hip.DEPTH_PARAMS(1, 1e-45), 1, p, d) == OK, "the smallest denormal is finite and > 0"
    depth[:] = 0
    assert _bake(w, good, 0x7fffffff + 1, p, d) == INVALID
    assert not depth.any(), "a refused call writes nothing"
    # the forms that take a context check it before anything touches a GPU
    assert L.mort_hip_probe_depth_bake(None, C.byref(good), n, p, d, None) == INVALID
    assert L.mort_hip_probe_depth_bake_device(None, C.byref(good), n, p, d, None, None) == INVALID


def test_bake_empty_batch_and_overlap():
    w = _world()
    good = hip.DEPTH_PARAMS(2, 100.0)
    probes = np.zeros(1, dtype=hip.PROBE_DTYPE)
    depth = np.full(200, 7, dtype=F)
    sec = C.c_double(5)
    assert _bake(w, good, 0, probes.ctypes.data, depth.ctypes.data, C.byref(sec)) == OK
    assert (depth == 7).all() and sec.value == 0, "nothing is written"
    assert _bake(w, hip.DEPTH_PARAMS(0, 100.0), 0, probes.ctypes.data, depth.ctypes.data) == INVALID, "the parameters are checked first"
    assert hip.probe_depth_bake_host(w, good, np.zeros((0, 4), dtype=F))["depth"].shape == (0, 200)
    # probes and maps side by side
    n = 3
    buf = np.zeros(n * 16 + n * 800 + 64, dtype=np.uint8)
    base = buf.ctypes.data
    pr, dm = base, base + n * 16
    assert _bake(w, good, n, pr, dm) == OK
    assert _bake(w, good, n, pr, dm - 4) == INVALID    # the maps over the last probe's time
    assert _bake(w, good, n, pr, pr) == INVALID
    assert _bake(w, good, n, dm + n * 800 - 4, dm) == INVALID  # the probes over the maps' tail
    assert _bake(w, good, 1, pr, pr + 16) == OK, "one probe spans 16 bytes"


# ------------------------------------------------------------------------------------------------------------- the sampler

def _grid(count=(2, 2, 2)):
    return hip.VOLUME_GRID((0, 0, 0), (1, 1, 1), count, 0.5)


def _sample(g, rec, depth, vp, n, pts, stride, out, sec=None):
    return hip.lib().mort_hip_volume_sample_visible_host(C.byref(g) if g is not None else None, rec, depth, C.byref(vp) if vp is not None else None,
                                                         n, pts, stride, 1, out, sec)


def _buffers(n=3, probes=8):
    return np.ones(probes * 32, dtype=F), np.ones(probes * 200, dtype=F), np.zeros(n * 6, dtype=F), np.zeros(n * 4, dtype=F)


def test_sampler_status_codes():
    L = hip.lib()
    g = _grid()
    rec, dm, pts, out = _buffers()
    r, d, p, o = rec.ctypes.data, dm.ctypes.data, pts.ctypes.data, out.ctypes.data
    good = hip.VOLUME_VIS_PARAMS(0.5, 0.05)
    assert _sample(g, r, d, good, 3, p, 24, o) == OK and out.any()
    out[:] = 0
    assert _sample(None, r, d, good, 3, p, 24, o) == INVALID
    assert _sample(g, None, d, good, 3, p, 24, o) == INVALID
    assert _sample(g, r, None, good, 3, p, 24, o) == INVALID
    assert _sample(g, r, d, None, 3, p, 24, o) == INVALID
    assert _sample(g, r, d, good, 3, None, 24, o) == INVALID
    assert _sample(g, r, d, good, 3, p, 24, None) == INVALID
    for bias, minv in ((-1.0, 0.05), (np.nan, 0.05), (np.inf, 0.05), (-np.inf, 0.05), (0.5, -0.1), (0.5, 1.5), (0.5, np.nan), (0.5, np.inf),
                       (0.5, float(np.nextafter(F(1.0), F(2.0))))):
        assert _sample(g, r, d, hip.VOLUME_VIS_PARAMS(bias, minv), 3, p, 24, o) == INVALID, (bias, minv)
    for bias, minv in ((0.0, 0.0), (0.0, 1.0), (1e30, 0.5), (-0.0, -0.0)):
        assert _sample(g, r, d, hip.VOLUME_VIS_PARAMS(bias, minv), 1, p, 24, o) == OK, (bias, minv)
    out[:] = 0
    wide = np.zeros(3 * 12, dtype=F)
    for stride in (0, 4, 20, 23, 25, 42, 47):
        assert _sample(g, r, d, good, 3, wide.ctypes.data, stride, o) == INVALID, stride
    for kw in (dict(count=(0, 2, 2)), dict(count=(2, 2, 4097))):
        assert _sample(_grid(**kw), r, d, good, 3, p, 24, o) == INVALID, kw
    bad = _grid()
    bad.spacing[1] = 0.0
    assert _sample(bad, r, d, good, 3, p, 24, o) == INVALID
    assert _sample(g, r, d, good, 0x7fffffff * 256 + 1, p, 24, o) == INVALID
    assert not out.any(), "a refused call writes nothing"
    assert L.mort_hip_volume_sample_visible(None, C.byref(g), r, d, C.byref(good), 3, p, 24, o, None) == INVALID
    assert L.mort_hip_volume_sample_visible_device(None, C.byref(g), r, d, C.byref(good), 3, p, 24, o, None, None) == INVALID


def test_sampler_empty_batch_and_overlap():
    g = _grid()
    rec, dm, pts, out = _buffers()
    good = hip.VOLUME_VIS_PARAMS(0.5, 0.05)
    out[:] = 7
    sec = C.c_double(5)
    assert _sample(g, rec.ctypes.data, dm.ctypes.data, good, 0, pts.ctypes.data, 24, out.ctypes.data, C.byref(sec)) == OK
    assert (out == 7).all() and sec.value == 0, "nothing is written"
    assert _sample(g, rec.ctypes.data, dm.ctypes.data, hip.VOLUME_VIS_PARAMS(-1.0, 0.05), 0, pts.ctypes.data, 24, out.ctypes.data) == INVALID
    assert hip.volume_sample_visible_host(g, rec, dm, good, np.zeros((0, 6), dtype=F))["out"].shape == (0, 4)
    # records, maps, points, output side by side
    n, stride = 4, 40
    span = (n - 1) * stride + 24
    buf = np.zeros(8 * 128 + 8 * 800 + span + n * 16 + 256, dtype=np.uint8)
    base = buf.ctypes.data
    r, d = base, base + 8 * 128
    p = d + 8 * 800
    o = p + span
    assert _sample(g, r, d, good, n, p, stride, o) == OK
    assert _sample(g, r, d, good, n, p, stride, d + 8 * 800 - 4) == INVALID  # over the maps' tail
    assert _sample(g, r, d, good, n, p, stride, d) == INVALID
    assert _sample(g, r, d, good, n, p, stride, d + 400) == INVALID          # inside a map
    assert _sample(g, r, d, good, n, p, stride, r + 8 * 128 - 4) == INVALID  # over the records' tail
    assert _sample(g, r, d, good, n, p, stride, o - 4) == INVALID            # over the last point's normal
    assert _sample(g, r, d, good, n, p, stride, p + 24) == INVALID
    assert _sample(g, r, r, good, n, p, stride, o) == OK, "inputs may share memory"
