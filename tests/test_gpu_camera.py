"""The two ends of Camera::render, record by record, ON THE DEVICE: get_ray in both instantiations the kernels compile -- get_ray<RenderArgs>
(fn 0: the one-lane kernel, the wave mode's front) and get_ray<CamView> read from LDS as mega_bvh.h and mega_gen.hip read it (fn 1: every record's CamView is written by the neighbouring
lane and read after a barrier; the build checks that camera_kernel keeps its 256 x 80 B of static LDS) -- and
pixel_finish / pixel_rgba (fn 2), through mort_hip_debug_camera_device (one upload, one launch of camera_kernel, one download per function),
bit for bit against hipcc's host compile of the same body and against the oracle's get_ray and render_pixel's tail:

  device (hipcc, gfx950)  ==  hipcc's host compile (mort_hip_debug_camera_host)  ==  the oracle (mort_oracle_camera_batch)

2^18 records per function (tests/camera_cases.py; the families and the census are in tests/test_camera_host.py): streams whose first four
outputs are chosen (offsets of exactly 0 and 1, disk points on the unit circle), pixels past 2^16 and 2^24, sqrt_spp from 0 to 32768,
defocus angles of -0, denormal, inf and NaN, the sweep's own cameras with scaled, zero and non-finite vectors; sums whose scaled value lies
on and beside every byte boundary, negative, -0, denormal, infinite and NaN, inf x 0.  Tolerance 0; signed zeros count; any NaN equals any
NaN; the final stream words and the draw counts are equal.  One batch per function ends inside a wave (2^16 + 37 records) into an
over-allocated output filled with 0xa5, whose tail must stay untouched."""
import time

import numpy as np
import pytest

from mort_amd import hip
from tests import camera_cases as CC
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fn", (0, 1, 2), ids=CC.NAMES)
def test_device_equals_host_compile_and_oracle(gpu_ctx, fn):
    rec = CC.records(fn)
    want = CC.oracle(fn)
    if fn == 2:
        CC.assert_pixel_census(CC.pixel_census(rec, want))
    else:
        CC.assert_ray_census(CC.ray_census(rec, want), len(rec))
    t0 = time.perf_counter()
    dev = hip.debug_camera_device(fn, rec)
    seconds = time.perf_counter() - t0
    print(f"{CC.NAMES[fn]}: {len(rec)} records, upload + launch + download {seconds:.3f} s")
    CC.assert_same(fn, rec, dict(device=dev.reshape(len(rec), -1), hipcc_host=hip.debug_camera_host(fn, rec).reshape(len(rec), -1), oracle=want))
    if fn == 2:
        assert ((dev.reshape(len(rec), -1)[:, 3] >> np.uint32(24)) == 255).all()


@pytest.mark.parametrize("fn", (0, 1, 2), ids=CC.NAMES)
def test_ragged_batch_leaves_the_tail_untouched(gpu_ctx, fn):
    """2^16 + 37 records: the last wave is partial, and the words after record n keep their 0xa5 fill"""
    rec = CC.ragged(fn)
    ow = hip.CAMERA_SHAPES[fn][1]
    out = np.full(len(rec) * ow + 4096, 0xa5a5a5a5, dtype=np.uint32)
    hip.debug_camera_device(fn, rec, out=out)
    assert (out[len(rec) * ow:] == 0xa5a5a5a5).all()
    got = out[: len(rec) * ow].reshape(len(rec), ow)
    assert not (got == 0xa5a5a5a5).all(1).any()  # every record was written
    CC.assert_same(fn, rec, dict(device=got, oracle=O.camera_batch(fn, rec)))


@pytest.mark.parametrize("fn", (0, 1, 2), ids=CC.NAMES)
def test_small_batches(gpu_ctx, fn):
    """1, 2, 3, 255, 257 and 513 records: in fn 1 the last record's CamView comes from a lane that has no record of its own (odd sizes), or
    from the next workgroup's first trip (past a multiple of 256)"""
    rec = CC.ragged(fn)
    for n in (1, 2, 3, 255, 257, 513):
        part = np.ascontiguousarray(rec[1000: 1000 + n])
        got = hip.debug_camera_device(fn, part).reshape(n, -1)
        CC.assert_same(fn, part, dict(device=got, oracle=O.camera_batch(fn, part)))


def test_device_entry_refuses_before_it_launches(gpu_ctx):
    """no function 3 or -1, no empty batch, no null buffer: refused with nothing written"""
    import ctypes as C
    f = hip.lib().mort_hip_debug_camera_device
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    rec = np.zeros((2, 30), np.uint32)
    out = np.full(64, 0xa5a5a5a5, dtype=np.uint32)
    for fn, n, src, dst in ((3, 2, rec.ctypes.data, out.ctypes.data), (-1, 2, rec.ctypes.data, out.ctypes.data), (0, 0, rec.ctypes.data, out.ctypes.data),
                            (0, 2, None, out.ctypes.data), (0, 2, rec.ctypes.data, None)):
        assert f(0, fn, src, n, dst) == -1, (fn, n)
    assert (out == 0xa5a5a5a5).all()
