"""The C ABI of the irradiance volumes (include/mort_hip.h) as far as it can be checked without a GPU: the layout
of mort_volume_grid, mort_volume_point and a record, every status code of the host forms, the refusal of overlapping buffers and
the empty batch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mort_amd import hip

OK, INVALID = 0, -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_layout_as_the_header_declares_it(tmp_path):
    """sizeof and offsetof from the header itself, compiled as C, against the ctypes structure and the dtype of the binding"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mort_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %zu\\n", sizeof(mort_volume_grid), offsetof(mort_volume_grid, origin), '
                   'offsetof(mort_volume_grid, spacing), offsetof(mort_volume_grid, count), offsetof(mort_volume_grid, time), '
                   'sizeof(mort_volume_point), offsetof(mort_volume_point, p), offsetof(mort_volume_point, normal), MORT_VOLUME_RECORD_FLOATS, '
                   'MORT_VOLUME_MAX_COUNT, offsetof(mort_hit, normal)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "cc"), "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    assert got == [40, 0, 12, 24, 36, 24, 0, 12, 32, 4096, 12]
    G = hip.VOLUME_GRID
    assert C.sizeof(G) == 40 and (G.origin.offset, G.spacing.offset, G.count.offset, G.time.offset) == (0, 12, 24, 36)
    P = hip.VOLUME_POINT_DTYPE
    assert P.itemsize == 24 and P.fields["p"][1] == 0 and P.fields["normal"][1] == 12
    assert hip.HIT_DTYPE.fields["p"][1] == 0 and hip.HIT_DTYPE.fields["normal"][1] == 12, "a point is the head of a hit"
    assert hip.VOLUME_RECORD_FLOATS * 4 == 128 and hip.VOLUME_MAX_COUNT == 4096


def test_exports():
    L = C.CDLL(hip.LIB_PATH)
    for name in ("mort_hip_volume_probes", "mort_hip_volume_pack", "mort_hip_volume_pack_device", "mort_hip_volume_pack_host",
                 "mort_hip_volume_sample", "mort_hip_volume_sample_device", "mort_hip_volume_sample_host"):
        assert name in hip.EXPORTS
        getattr(L, name)


def _grid(origin=(0, 0, 0), spacing=(1, 1, 1), count=(2, 2, 2)):
    return hip.VOLUME_GRID(origin, spacing, count, 0.5)


def _sample(g, rec, n, pts, stride, out, sec=None):
    return hip.lib().mort_hip_volume_sample_host(C.byref(g) if g is not None else None, rec, n, pts, stride, 1, out, sec)


def _buffers(n=3, probes=8):
    return np.ones(probes * 32, dtype=F), np.zeros(n * 6, dtype=F), np.zeros(n * 4, dtype=F)


BAD_GRIDS = [dict(spacing=(0, 1, 1)), dict(spacing=(1, -1, 1)), dict(spacing=(1, 1, np.inf)), dict(spacing=(np.nan, 1, 1)),
             dict(spacing=(1, 0, 1), count=(2, 1, 2)),  # spacing > 0 also where count is 1
             dict(origin=(np.inf, 0, 0)), dict(origin=(0, np.nan, 0)), dict(origin=(0, 0, -np.inf)),
             dict(count=(0, 2, 2)), dict(count=(2, -1, 2)), dict(count=(2, 2, 4097)),
             dict(count=(2048, 2048, 512))]  # 2^31 probes


def test_grid_checks():
    rec, pts, out = _buffers()
    a = (rec.ctypes.data, 3, pts.ctypes.data, 24, out.ctypes.data)
    assert _sample(_grid(), *a) == OK
    probes = np.zeros(8, dtype=hip.PROBE_DTYPE)
    for kw in BAD_GRIDS:
        g = _grid(**kw)
        assert _sample(g, *a) == INVALID, kw
        assert hip.lib().mort_hip_volume_probes(C.byref(g), probes.ctypes.data) == INVALID, kw
        with pytest.raises(hip.MortHipError) as e:
            hip.volume_probes(g)
        assert e.value.status == INVALID
    assert (probes.view(np.uint8) == 0).all()
    # the limit of an axis is itself fine
    g = _grid(count=(4096, 1, 1))
    big = np.zeros(4096, dtype=hip.PROBE_DTYPE)
    assert hip.lib().mort_hip_volume_probes(C.byref(g), big.ctypes.data) == OK and big["position"][4095][0] == 4095
    assert hip.lib().mort_hip_volume_probes(None, big.ctypes.data) == INVALID
    assert hip.lib().mort_hip_volume_probes(C.byref(g), None) == INVALID


def test_null_arguments_and_strides():
    L = hip.lib()
    g = _grid()
    rec, pts, out = _buffers()
    r, p, o = rec.ctypes.data, pts.ctypes.data, out.ctypes.data
    assert _sample(None, r, 3, p, 24, o) == INVALID
    assert _sample(g, None, 3, p, 24, o) == INVALID
    assert _sample(g, r, 3, None, 24, o) == INVALID
    assert _sample(g, r, 3, p, 24, None) == INVALID
    wide = np.zeros(3 * 12, dtype=F)
    for stride in (0, 4, 20, 23, 25, 26, 27, 42, 47):
        assert _sample(g, r, 3, wide.ctypes.data, stride, o) == INVALID, stride
    for stride in (24, 28, 40, 48):
        assert _sample(g, r, 3, wide.ctypes.data, stride, o) == OK, stride
    assert _sample(g, r, 3, wide.ctypes.data, 2 ** 63, o) == INVALID, "(n - 1) * stride does not fit size_t"
    # the forms that take a context check it before anything touches a GPU
    assert L.mort_hip_volume_sample(None, C.byref(g), r, 3, p, 24, o, None) == INVALID
    assert L.mort_hip_volume_sample_device(None, C.byref(g), r, 3, p, 24, o, None, None) == INVALID
    assert L.mort_hip_volume_pack(None, 2, r, None, o, None) == INVALID
    assert L.mort_hip_volume_pack_device(None, 2, r, None, o, None, None) == INVALID
    # the pack
    sh, recs = np.zeros(2 * 27, dtype=F), np.zeros(2 * 32, dtype=F)
    assert L.mort_hip_volume_pack_host(2, None, None, 1, recs.ctypes.data, None) == INVALID
    assert L.mort_hip_volume_pack_host(2, sh.ctypes.data, None, 1, None, None) == INVALID
    assert L.mort_hip_volume_pack_host(2, sh.ctypes.data, None, 1, recs.ctypes.data, None) == OK
    assert L.mort_hip_volume_pack_host((0x7fffffff * 256) // 8 + 1, sh.ctypes.data, None, 1, recs.ctypes.data, None) == INVALID
    assert _sample(g, r, 0x7fffffff * 256 + 1, p, 24, o) == INVALID


def test_empty_batch_is_ok():
    L = hip.lib()
    g = _grid()
    rec, pts, out = _buffers()
    out[:] = 7
    sec = C.c_double(5)
    assert _sample(g, rec.ctypes.data, 0, pts.ctypes.data, 24, out.ctypes.data, C.byref(sec)) == OK
    assert (out == 7).all() and sec.value == 0, "nothing is written"
    assert _sample(_grid(count=(0, 1, 1)), rec.ctypes.data, 0, pts.ctypes.data, 24, out.ctypes.data) == INVALID, "the grid is checked first"
    recs = np.full(32, 7, dtype=F)
    sec = C.c_double(5)
    assert L.mort_hip_volume_pack_host(0, rec.ctypes.data, None, 1, recs.ctypes.data, C.byref(sec)) == OK
    assert (recs == 7).all() and sec.value == 0
    assert hip.volume_sample_host(g, rec, np.zeros((0, 6), dtype=F))["out"].shape == (0, 4)


def test_overlapping_buffers_are_refused():
    L = hip.lib()
    g = _grid()
    n, stride = 4, 40
    span = (n - 1) * stride + 24
    buf = np.zeros(8 * 128 + span + n * 16 + 256, dtype=np.uint8)
    base = buf.ctypes.data
    rec, pts, out = base, base + 8 * 128, base + 8 * 128 + span  # side by side: the output starts where the points' span ends
    assert _sample(g, rec, n, pts, stride, out) == OK
    assert _sample(g, rec, n, pts, stride, out - 4) == INVALID        # over the last point's normal
    assert _sample(g, rec, n, pts, stride, pts + 24) == INVALID       # between two points is inside the span
    assert _sample(g, rec, n, pts, stride, pts) == INVALID
    assert _sample(g, rec, n, pts, stride, rec + 8 * 128 - 4) == INVALID  # over the records' tail
    assert _sample(g, rec, n, pts, stride, rec) == INVALID
    assert _sample(g, rec, n, pts - n * 16, stride, rec) == INVALID
    assert _sample(g, rec, 1, pts, stride, pts + 24) == OK, "one point spans 24 bytes"
    buf[:] = 0
    # the pack: sh, weight, records side by side
    m = 3
    sh, wt, recs = base, base + m * 108, base + m * 108 + m * 4
    assert L.mort_hip_volume_pack_host(m, sh, wt, 1, recs, None) == OK
    assert L.mort_hip_volume_pack_host(m, sh, wt, 1, wt + m * 4 - 4, None) == INVALID   # records over the weights' tail
    assert L.mort_hip_volume_pack_host(m, sh, wt, 1, sh + m * 108 - 4, None) == INVALID  # records over the coefficients' tail
    assert L.mort_hip_volume_pack_host(m, sh, None, 1, wt, None) == OK, "no weights, no range"
    assert L.mort_hip_volume_pack_host(m, recs + 4, wt, 1, recs, None) == INVALID
