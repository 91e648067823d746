"""The device side of mort_f2i (include/mort_math.h: one v_cvt_i32_f32) is CUDA's cvt.rzi.s32.f32 -- truncate, saturate, NaN -> 0 -- for
every float there is.

 (a) a kernel runs ALL 2^32 bit patterns through the device's mort_f2i and through mort_f2i_select (the same function as selects around
     a guarded (int)x, compiled beside it) and counts the patterns that convert differently: 0 (mort_hip_debug_f2i_device);
 (b) 2^20 chosen patterns are converted on the device, copied back and compared with the HOST's mort_f2i (the ifs, as gcc and the oracle
     have them) and with the definition written out in numpy: +-0, denormals, +-2^31 and +-(2^31 - 128) with their neighbours on both
     sides, +-infinity, quiet and signalling NaNs of both signs, every exponent with all-zero and all-one mantissas, integers, halves and
     their neighbours, and random patterns for the rest."""
import ctypes as C

import numpy as np
import pytest

from mort_amd import hip

pytestmark = pytest.mark.gpu

N_LIST = 1 << 20
INT_MAX, INT_MIN = 2147483647, -2147483648


def _chosen_patterns():
    u = np.uint32
    parts = []
    sign = np.array([0, 0x80000000], np.uint32)
    around = np.arange(-64, 65, dtype=np.int64)
    # +-0, the smallest and largest denormals and their neighbours, the smallest normal
    for centre in (0x00000000, 0x00000001, 0x007fffff, 0x00800000, 0x00400000):
        parts.append((centre + np.arange(0, 65, dtype=np.int64))[None, :] | sign[:, None].astype(np.int64))
    # 2^31 = 0x4f000000, 2^31 - 128 = 0x4effffff (the largest float below 2^31), 1.0, 2^24, 2^23: neighbours on both sides, both signs
    for centre in (0x4f000000, 0x4effffff, 0x3f800000, 0x4b800000, 0x4b000000, 0x4e800000):
        parts.append((centre + around)[None, :] | sign[:, None].astype(np.int64))
    # infinities, quiet and signalling NaNs of both signs: first, last and scattered payloads
    payload = np.concatenate([np.arange(1, 65), (1 << 22) - np.arange(1, 65), (1 << 22) + np.arange(0, 65), (1 << 23) - np.arange(1, 65)]).astype(np.int64)
    parts.append((0x7f800000 + np.concatenate([[0], payload]))[None, :] | sign[:, None].astype(np.int64))
    # every exponent with all-zero and all-one mantissas, both signs
    e = np.arange(256, dtype=np.int64) << 23
    parts.append(np.concatenate([e, e | 0x7fffff])[None, :] | sign[:, None].astype(np.int64))
    fixed = np.concatenate([p.ravel() for p in parts]).astype(np.uint32)
    rng = np.random.default_rng(2311)
    # integers, halves and their neighbours in the last place, up to 2^31 and beyond
    k = rng.integers(0, 1 << 33, 1 << 17).astype(np.float64) * rng.choice([0.5, 1.0, 1.0], 1 << 17) * rng.choice([-1.0, 1.0], 1 << 17)
    near = k.astype(np.float32)
    near = np.concatenate([near, np.nextafter(near, np.float32(0)), np.nextafter(near, np.float32(np.inf)), np.nextafter(near, np.float32(-np.inf))]).view(np.uint32)
    n_rand = N_LIST - len(fixed) - len(near)
    bits = np.concatenate([fixed, near, rng.integers(0, 1 << 32, n_rand, dtype=np.uint64).astype(u)])
    assert len(bits) == N_LIST
    return np.ascontiguousarray(bits, np.uint32)


def _definition(bits):
    """cvt.rzi.s32.f32 written out: NaN -> 0, saturate, else truncate (exact in fp64)."""
    with np.errstate(invalid="ignore"):  # signalling NaNs raise `invalid` when widened
        x = bits.view(np.float32).astype(np.float64)
        t = np.trunc(np.where(np.isnan(x), 0.0, np.clip(x, float(INT_MIN), float(INT_MAX))))
    return t.astype(np.int64).astype(np.int32)


@pytest.fixture(scope="module")
def converted():
    L = hip.lib()
    dev = L.mort_hip_debug_f2i_device
    dev.restype = C.c_int
    dev.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_ulonglong)]
    hst = L.mort_hip_debug_f2i_host
    hst.restype = C.c_int
    hst.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    bits = _chosen_patterns()
    got = np.empty(N_LIST, np.int32)
    want = np.empty(N_LIST, np.int32)
    out = (C.c_ulonglong * 3)()
    assert dev(0, bits.ctypes.data_as(C.c_void_p), N_LIST, got.ctypes.data_as(C.c_void_p), out) == 0
    assert hst(bits.ctypes.data_as(C.c_void_p), N_LIST, want.ctypes.data_as(C.c_void_p)) == 0
    return bits, got, want, list(out)


def test_every_bit_pattern_against_the_select_form(converted):
    differ, lowest, visited = converted[3]
    print(f"mort_f2i against mort_f2i_select on the device: {visited} patterns, {differ} differ, lowest 0x{lowest:08x}")
    assert visited == 1 << 32
    assert differ == 0, f"{differ} patterns differ, the lowest is 0x{lowest:08x}"


def test_chosen_patterns_against_the_host(converted):
    bits, got, want, _ = converted
    x = bits.view(np.float32)
    # the list holds what the docstring says it holds
    assert (bits == 0).any() and (bits == 0x80000000).any()
    for v in (0x4f000000, 0x4effffff, 0xcf000000, 0xceffffff, 0x4f000001, 0xcf000001, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001):
        assert (bits == v).any(), hex(v)
    denormal = ((bits & 0x7f800000) == 0) & ((bits & 0x7fffff) != 0)
    assert denormal.sum() > 100 and np.isnan(x).sum() > 500
    for e in range(256):
        assert (bits == (e << 23)).any() and (bits == ((e << 23) | 0x7fffff)).any() and (bits == (0x80000000 | (e << 23) | 0x7fffff)).any()
    model = _definition(bits)
    bad_host = np.flatnonzero(want != model)
    assert bad_host.size == 0, [(hex(int(bits[i])), int(want[i]), int(model[i])) for i in bad_host[:8]]
    bad = np.flatnonzero(got != want)
    print(f"device mort_f2i against the host's on {N_LIST} chosen patterns: {bad.size} differ; saturated high {int((got == INT_MAX).sum())}, "
          f"low {int((got == INT_MIN).sum())}, NaN inputs {int(np.isnan(x).sum())}")
    assert bad.size == 0, [(hex(int(bits[i])), int(got[i]), int(want[i])) for i in bad[:8]]
    assert (got[np.isnan(x)] == 0).all() and (got == INT_MAX).sum() > 100 and (got == INT_MIN).sum() > 100
