"""The math layer ON THE DEVICE against the two host compiles of the same source, bit for bit (mort_hip_debug_math_device: one upload, one
launch of math_kernel, one download per function).

include/mort_math.h promises that gcc (the oracle) and hipcc (the gfx950 kernels) give the same bits from the same definitions; the renders
only ever feed it the workload's own arguments.  Here every function of debug.hip's math table runs over its whole builder of
tests/math_cases.py -- every exponent, denormal arguments and results, signed zeros, infinities, NaNs, the floats next to k * pi/2 up to the
1e5 domain bound, next to +-1, next to atan's break points, next to 0.9 for onb_from_w, the sphere's poles and seam, texel boundaries --
2^22 records per function of mort_math.h (group A) and per plain operator the contract leans on (P: / in fp32 and fp64, the narrowing and
integer conversions, truncf), 2^20 per function of dev_math.h (B) and dev_trace.h (C), 2^18 for noise_value:

  device (hipcc, gfx950)  ==  hipcc's host compile (mort_hip_debug_math_host)  ==  gcc's compile (mort_oracle_math_batch; groups A and P)

Tolerance 0; signed zeros count; a NaN compares as one word (IEEE 754 leaves a produced NaN's sign and payload open; measured: no raw word
differs in groups A and P, and the sign alone in 54 records of reflectance and refract with infinite arguments).  One batch per group ends inside a wave (2^16 + 37 records) into an over-allocated output filled with 0xa5, whose tail must
stay untouched.  random_float is swept over all 2^32 generator outputs against the reference's (float)(1.0 - (double)u), on the device."""
import time

import numpy as np
import pytest

from mort_amd import hip
from tests import math_cases as MC
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tables():
    world, noise_raw = MC.noise_world()
    _, image_recs, texels = MC.image_world()
    return world, noise_raw, image_recs, texels


def _results(fn, rec, tables, out=None):
    kw = MC.tables_for(fn, *tables[1:])
    t0 = time.perf_counter()
    dev = hip.debug_math_device(fn, rec, out=out, **kw)
    seconds = time.perf_counter() - t0
    res = dict(device=dev[: len(rec) * hip.debug_math_shapes()[fn][1]].reshape(len(rec), -1), hipcc_host=hip.debug_math_host(fn, rec, **kw).reshape(len(rec), -1))
    if fn < len(O.MATH_SHAPES):
        res["gcc"] = O.math_batch(fn, rec)
    return res, seconds


@pytest.mark.parametrize("fn", range(len(MC.NAMES)), ids=MC.NAMES)
def test_device_equals_both_host_compiles(fn, tables):
    rec, census = MC.build(fn)
    MC.assert_census(fn, census)
    res, seconds = _results(fn, rec, tables)
    print(f"{MC.NAMES[fn]}: {len(rec)} records, upload + launch + download {seconds:.3f} s, compared with {', '.join(list(res)[1:])}")
    MC.assert_same(fn, rec, res)


@pytest.mark.parametrize("fn", MC.RAGGED_FNS, ids=[MC.NAMES[f] for f in MC.RAGGED_FNS])
def test_ragged_batch_leaves_the_tail_untouched(fn, tables):
    """2^16 + 37 records: the last wave is partial, and the words after record n keep their 0xa5 fill"""
    rec = MC.ragged(fn)
    ow = hip.debug_math_shapes()[fn][1]
    out = np.full(len(rec) * ow + 4096, 0xa5a5a5a5, dtype=np.uint32)
    res, _ = _results(fn, rec, tables, out=out)
    assert (out[len(rec) * ow:] == 0xa5a5a5a5).all()
    assert not (out[: len(rec) * ow].reshape(len(rec), ow) == 0xa5a5a5a5).all(1).any()  # every record was written
    MC.assert_same(fn, rec, res)


def test_random_float_over_all_generator_outputs():
    """dev_math.h: random_float's 1.0f - u equals the reference's (float)(1.0 - (double)u) for all 2^32 generator outputs -- the device half
    (tests/test_rng.py is the host's)"""
    r = hip.debug_random_float_device()
    assert r["visited"] == 1 << 32
    assert r["differ"] == 0 and r["lowest"] == 0xffffffff, r
