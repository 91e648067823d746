"""Light sampling, record by record, ON THE DEVICE: light_pdf_value and light_random (dev_render.h over dev_trace.h's wsphere_* / wquad_*) over
the scene of a context whose world has been uploaded (mort_hip_debug_light_device: one upload, one launch of light_kernel, one download
per function and world), bit for bit against hipcc's host compile of the same body and against the oracle's pdf_value_dispatch /
random_dispatch:

  device (hipcc, gfx950)  ==  hipcc's host compile (mort_hip_debug_light_host)  ==  the oracle (mort_oracle_light_batch)

2^20 records per function and world (tests/light_cases.py; the families and the census figures are in tests/test_light_host.py's
docstring): lists of 1, 3, 40 and 500 members, members that sample nothing, a list over spheres a BVH build has moved, moving and
non-emissive lights, quads from the back, origins inside a sphere, in a quad's plane, at the centre and at Q, degenerate primitives,
zero, infinite and NaN directions, every tag from -1 to 8.  Tolerance 0; signed zeros count; any NaN equals any NaN; the final stream
words and the draw counts are equal.  One batch per function ends inside a wave (2^16 + 37 records) into an over-allocated output
filled with 0xa5, whose tail must stay untouched.

Measured on the MI355X: 0 differing records; upload + launch + download 0.007 s (light_pdf_value) and 0.010 s (light_random) per 2^20
records.  What the sweep sees, from three scratch mutations of the device code alone: 3.1415926 -> 3.14159265 in wsphere_pdf_value
fails 38417 (BVH world) and 26066 (flat world) of the 2^20 light_pdf_value records and 1621 of the ragged batch; a one-member list that
skips its random_int draw fails all 83713 records of the flat world's list 0 (5393 of the ragged batch) and list_of_one in every form
of tests/test_gpu_light_worlds.py; the list weight formed as 1.0f / (float)n fails nothing and cannot: a quotient rounded to 53 bits
and then to 24 is the quotient rounded to 24, so it equals (float)(1.0 / (double)(float)n) for every n (checked for all n < 2^24)."""
import time

import numpy as np
import pytest

from mort_amd import hip, structs as S
from tests import light_cases as LC
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

CASES = [(w, fn) for w in sorted(LC.WORLDS) for fn in (0, 1)]
IDS = [f"{w}-{LC.NAMES[fn]}" for w, fn in CASES]


def _upload(ctx, world):
    ctx.set_partition(0, 1, 8)
    ctx.upload_world(world)


@pytest.mark.parametrize("world_name,fn", CASES, ids=IDS)
def test_device_equals_host_compile_and_oracle(gpu_ctx, world_name, fn):
    LC.assert_census(world_name, fn)
    world, _ = LC.WORLDS[world_name]()
    rec, _ = LC.build(world_name, fn)
    _upload(gpu_ctx, world)
    t0 = time.perf_counter()
    dev = hip.debug_light_device(gpu_ctx, fn, rec)
    seconds = time.perf_counter() - t0
    print(f"{world_name} world, {LC.NAMES[fn]}: {len(rec)} records, upload + launch + download {seconds:.3f} s")
    LC.assert_same(fn, rec, dict(device=dev.reshape(len(rec), -1), hipcc_host=hip.debug_light_host(world, fn, rec).reshape(len(rec), -1),
                                 oracle=LC.oracle(world_name, fn)))


@pytest.mark.parametrize("fn", (0, 1), ids=LC.NAMES)
def test_ragged_batch_leaves_the_tail_untouched(gpu_ctx, fn):
    """2^16 + 37 records: the last wave is partial, and the words after record n keep their 0xa5 fill"""
    world, _ = LC.WORLDS["flat"]()
    rec = LC.ragged("flat", fn)
    ow = hip.LIGHT_SHAPES[fn][1]
    out = np.full(len(rec) * ow + 4096, 0xa5a5a5a5, dtype=np.uint32)
    _upload(gpu_ctx, world)
    hip.debug_light_device(gpu_ctx, fn, rec, out=out)
    assert (out[len(rec) * ow:] == 0xa5a5a5a5).all()
    got = out[: len(rec) * ow].reshape(len(rec), ow)
    assert not (got == 0xa5a5a5a5).all(1).any()  # every record was written
    LC.assert_same(fn, rec, dict(device=got, oracle=O.light_batch(world, fn, rec)))


def test_device_entry_refuses_before_it_launches(gpu_ctx):
    """every record is checked on the host against the uploaded world's tables (check_light): one bad record among good ones fails the call"""
    world, _ = LC.WORLDS["flat"]()
    _upload(gpu_ctx, world)
    for fn in (0, 1):
        for typ, idx in ((S.OBJ_SPHERE, 1090), (S.OBJ_SPHERE, -1), (S.OBJ_QUAD, 640), (S.OBJ_HITTABLE_LIST, 2), (S.OBJ_HITTABLE_LIST, -1)):
            rec = np.zeros((3, hip.LIGHT_SHAPES[fn][0]), np.uint32)
            at = 0 if fn == 0 else 6
            rec[:, at] = np.array([S.OBJ_SPHERE, typ, S.OBJ_SPHERE], np.int32).view(np.uint32)
            rec[:, at + 1] = np.array([0, idx, 0], np.int32).view(np.uint32)
            out = np.full(3 * hip.LIGHT_SHAPES[fn][1], 0xa5a5a5a5, dtype=np.uint32)
            with pytest.raises(hip.MortHipError) as e:
                hip.debug_light_device(gpu_ctx, fn, rec, out=out)
            assert e.value.status == -1 and (out == 0xa5a5a5a5).all(), (fn, typ, idx)
