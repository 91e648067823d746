"""The shade step on the device, record by record: debug.hip's shade table -- the closest-hit search of a radiance query's segment (the
unified tree for the flat world, the threaded reference walk for the BVH world) and dev_shade.h's shade_hit, the gfx950 compile over the
scene of a context's uploaded world (mort_hip_debug_shade_device: one upload, one launch of shade_kernel, one download).

  device (hipcc, gfx950)  ==  hipcc's host compile (mort_hip_debug_shade_host)  ==  the oracle (mort_oracle_shade_batch)

0 differing records of 2^18 per (world, light setting), of the ragged batch of 2^16 + 37 and of the batch of one: status, k, rp,
final_value, the ray afterwards, the final stream words and the draw count, bit for bit (math_cases.canon's NaN rule; signed zeros count).
The worlds, the records and the census: tests/shade_cases.py, tests/test_shade_host.py."""
import numpy as np
import pytest

from mort_amd import hip, structs as S
from tests import oracle_lib as O
from tests import shade_cases as SC

pytestmark = pytest.mark.gpu

CASES = [(w, s) for w in SC.WORLDS for s in SC.LIGHT_SETTINGS]


@pytest.mark.parametrize("name,setting", CASES)
def test_device_equals_host_equals_the_oracle(gpu_ctx, name, setting):
    rec, _ = SC.records(name, setting)
    w = SC.shade_world(name).world
    gpu_ctx.upload_world(w)
    SC.assert_same(rec, dict(oracle=SC.oracle(name, setting)[0], host=hip.debug_shade_host(w, rec, tree=True), device=hip.debug_shade_device(gpu_ctx, rec)))


@pytest.mark.parametrize("name", SC.WORLDS)
def test_ragged_and_single_batches(gpu_ctx, name):
    w = SC.shade_world(name).world
    gpu_ctx.upload_world(w)
    rec = SC.ragged(name, "list")
    guard = np.full(len(rec) * 22 + 64, 0xdeadbeef, np.uint32)
    got = hip.debug_shade_device(gpu_ctx, rec, out=guard)
    assert (guard[len(rec) * 22:] == 0xdeadbeef).all()  # nothing written after the last record
    SC.assert_same(rec, dict(oracle=O.shade_batch(w, rec)[0], host=hip.debug_shade_host(w, rec, tree=True), device=got[: len(rec) * 22]))
    for i in (0, 12345):
        one = np.ascontiguousarray(rec[i:i + 1])
        SC.assert_same(one, dict(oracle=O.shade_batch(w, one)[0], device=hip.debug_shade_device(gpu_ctx, one)))


def test_status_codes(gpu_ctx):
    rec = np.array(SC.records("flat", "list")[0][:4])
    gpu_ctx.upload_world(SC.shade_world("flat").world)
    bad = rec.copy()
    bad[3, 14:16] = np.array((S.OBJ_SPHERE, 100000), np.int32).view(np.uint32)
    for r, kw in ((bad, {}), (rec, dict(fnum=1)), (rec[:0], {})):  # a bad light, an unknown fn, an empty batch: refused before any launch
        with pytest.raises(hip.MortHipError) as e:
            hip.debug_shade_device(gpu_ctx, r, **kw)
        assert e.value.status == -1
    with hip.Context(0) as fresh:
        with pytest.raises(hip.MortHipError) as e:
            hip.debug_shade_device(fresh, rec)
        assert e.value.status != 0  # no world uploaded
