"""The short forms of x / a and sqrtf(x) that the BVH leaf step uses (dev_math.h div_by, sqrt_ord), as MODELS on the host: the same
fma sequences in plain C++ with the hardware's seed (v_rcp_f32, v_sqrt_f32) as a parameter, against the host's correctly rounded
operators (mort_hip_debug_exact_forms_model).  No tolerance anywhere: 0 differing bits.

 - root: every seed within one unit in the last place of sqrtf(x), over more than 10^7 inputs across the whole guarded range
   [2^-96, 2^100): random, all-ones, zero and near-power-of-two mantissas, exact squares and their neighbours;
 - division: the correctly rounded reciprocal as seed over the same kinds of inputs (denominators 2^-40 ... 2^40, numerators
   2^-85 ... 2^56 of either sign), and seeds one unit off over random mantissas.  (A seed one unit off is NOT exact for a denominator
   with an all-ones mantissa under a power-of-two numerator: that family depends on what v_rcp_f32 returns and is settled on the
   device, tests/test_gpu_exact_forms.py.)
 - the guards: the last value inside each bound passes and is exact, the first value outside is refused (and so takes the plain
   operators); NaN, infinities, zeros, denormals and negative values are outside where the comments in dev_math.h say so."""
import ctypes as C

import numpy as np

from mort_amd import hip

N = 10_500_000


def _hooks():
    L = hip.lib()
    model = L.mort_hip_debug_exact_forms_model
    model.restype = C.c_int
    model.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]
    guards = L.mort_hip_debug_exact_guards
    guards.restype = C.c_int
    guards.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    return model, guards


def _run(model, what, x, a, lo, hi):
    x = np.ascontiguousarray(x, np.float32)
    a = None if a is None else np.ascontiguousarray(a, np.float32)
    out = (C.c_ulonglong * 16)()
    assert model(what, x.ctypes.data_as(C.c_void_p), None if a is None else a.ctypes.data_as(C.c_void_p), len(x), lo, hi, out) == 0
    out = list(out)
    return out[0], out[1], out[2], out[8:8 + min(out[1], 8)]


def _pow2(e):
    return np.ldexp(np.float32(1.0), np.asarray(e)).astype(np.float32)


def _values(rng, n, e_lo, e_hi):
    """n positive float32 in [2^e_lo, 2^e_hi): a quarter each with random, all-ones, zero and near-power mantissas."""
    e = rng.integers(e_lo, e_hi, n)
    kind = np.arange(n) % 4
    mant = rng.integers(0, 1 << 23, n, dtype=np.uint32)
    near = rng.integers(0, 4, n, dtype=np.uint32)                              # a few units above a power of two ...
    near = np.where(rng.random(n) < 0.5, near, np.uint32((1 << 23) - 1) - near)  # ... or below the next one
    mant = np.select([kind == 0, kind == 1, kind == 2], [mant, np.uint32((1 << 23) - 1), np.uint32(0)], near).astype(np.uint32)
    bits = ((e + 127).astype(np.uint32) << np.uint32(23)) | mant
    return bits.view(np.float32)


def test_root_model_is_sqrtf_for_every_seed_within_one_ulp():
    model, _ = _hooks()
    rng = np.random.default_rng(5101)
    x = _values(rng, N, -96, 100)
    k = rng.integers(1, 4096, 200_000).astype(np.float32) * _pow2(rng.integers(-40, 37, 200_000))
    sq = k * k                                                                 # exact squares (24 bits suffice) and their neighbours
    x = np.concatenate([x, sq, np.nextafter(sq, np.float32(0)), np.nextafter(sq, np.float32(np.inf))])
    compared, differ, outside, first = _run(model, 0, x, None, -1, 1)
    print(f"root model: {compared} comparisons, {differ} differ, {outside} inputs outside the guard, first {first}")
    assert outside == 0 and compared == 3 * len(x) and compared >= 3 * 10_000_000
    assert differ == 0, [float(x[i]) for i in first]


def test_division_model_is_the_quotient():
    model, _ = _hooks()
    rng = np.random.default_rng(5102)
    a = _values(rng, N, -40, 40)
    x = _values(rng, N, -85, 56)[rng.permutation(N)] * np.where(rng.random(N) < 0.5, np.float32(-1), np.float32(1))
    compared, differ, outside, first = _run(model, 1, x, a, 0, 0)
    print(f"division model, correctly rounded seed: {compared} comparisons, {differ} differ, {outside} outside, first {first}")
    assert outside == 0 and compared == N
    assert differ == 0, [(float(x[i]), float(a[i])) for i in first]
    # seeds one unit off, random mantissas
    ea, ex = rng.integers(-40, 40, N), rng.integers(-85, 56, N)
    a = (((ea + 127).astype(np.uint32) << np.uint32(23)) | rng.integers(0, 1 << 23, N, dtype=np.uint32)).view(np.float32)
    x = (((ex + 127).astype(np.uint32) << np.uint32(23)) | rng.integers(0, 1 << 23, N, dtype=np.uint32) |
         (rng.integers(0, 2, N, dtype=np.uint32) << np.uint32(31))).view(np.float32)
    compared, differ, outside, first = _run(model, 1, x, a, -1, 1)
    print(f"division model, seeds within one unit: {compared} comparisons, {differ} differ, {outside} outside, first {first}")
    assert outside == 0 and compared == 3 * N
    assert differ == 0, [(float(x[i]), float(a[i])) for i in first]


def test_guards_at_their_boundaries():
    model, guards = _hooks()
    f = np.float32
    inf, nan = f(np.inf), f(np.nan)

    def flags(v):
        v = np.ascontiguousarray(v, np.float32)
        out = np.zeros(len(v), np.uint8)
        assert guards(v.ctypes.data_as(C.c_void_p), len(v), out.ctypes.data_as(C.c_void_p)) == 0
        return out

    def below(v):
        return np.nextafter(f(v), f(0))

    def above(v):
        return np.nextafter(f(v), inf)

    den, num, root = 1, 2, 4
    p = lambda e: _pow2(e)[()]
    # denominators: 2^-40 <= a <= 2^40
    assert (flags([p(-40), p(40), f(1)]) & den).all()
    assert not (flags([below(p(-40)), above(p(40)), -p(-40), -f(1), f(0), f(-0.0), f(1e-45), inf, -inf, nan]) & den).any()
    # numerators: |x| < 2^56, either sign, zeros and denormals included (they only have to end below t_min)
    assert (flags([below(p(56)), -below(p(56)), f(0), f(-0.0), f(1e-45), p(-85)]) & num).all()
    assert not (flags([p(56), -p(56), inf, -inf, nan]) & num).any()
    # roots: 2^-96 <= x < 2^100
    assert (flags([p(-96), below(p(100)), f(1)]) & root).all()
    assert not (flags([below(p(-96)), p(100), f(0), f(-0.0), f(1e-45), -p(-96), -f(1), inf, -inf, nan]) & root).any()
    # just inside every bound the forms are exact for every tested seed; just outside the entry refuses the input
    edge_a = np.array([p(-40), above(p(-40)), below(p(40)), p(40)], f)
    edge_x = np.array([p(-85), above(p(-85)), below(p(56)), below(below(p(56))), -p(-85), -below(p(56))], f)
    aa, xx = np.meshgrid(edge_a, edge_x)
    compared, differ, outside, _ = _run(model, 1, xx.ravel(), aa.ravel(), 0, 0)
    assert (compared, differ, outside) == (aa.size, 0, 0)
    compared, differ, outside, _ = _run(model, 1, [f(1), f(1), p(56), below(p(-85)), f(0)], [below(p(-40)), above(p(40)), f(1), f(1), f(1)], 0, 0)
    assert (compared, outside) == (0, 5)
    compared, differ, outside, _ = _run(model, 0, [p(-96), above(p(-96)), below(p(100)), below(p(-96)), p(100), f(0), inf], None, -1, 1)
    assert (compared, differ, outside) == (9, 0, 4)
