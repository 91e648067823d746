"""include/mort_math.h, and the layers that stand on it, on the CPU.

 (a) against glibc/numpy on the workload's ranges: every fp32 function within 1 ULP of the float64 result rounded once, specials follow IEEE
     (the tests this file began with);
 (b) against mpmath (120 bits) on a fixed sample of the builders of tests/math_cases.py -- their edge families whole (specials, denormals,
     both sides of +-1e5, the 4096 floats either side of +-1, the neighbours of atan's break points, one pass over every exponent) and a
     stride over the large ones (the floats next to k * pi/2, dense ranges): the header's own claim, at most 1 ULP from the correctly
     rounded result, with the measured figures beside each assertion;
 (c) gcc's compile (mort_oracle_math_batch) against hipcc's host compile (mort_hip_debug_math_host) of the same definitions, bit for bit,
     over the full builders of mort_math.h's functions and of the plain operators the numerical contract leans on;
 (d) hipcc's host compile of dev_math.h's primitives and dev_trace.h's sphere_uv against restatements in numpy from the reference's
     formulas (tests/math_restate.py), and of noise_value / image_value against the oracle's texture dispatch, tolerance 0.
tests/test_gpu_math.py runs the same builders through the gfx950 compile."""
import math

import mpmath
import numpy as np
import pytest

from mort_amd import hip
from mort_amd import structs as S
from tests import math_cases as MC
from tests import math_restate as R


def ulp_diff(a, b):
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def vec(fn, xs):
    return np.array([fn(float(x)) for x in xs], dtype=np.float32)


def test_sinf_cosf(oracle):
    L = oracle.lib()
    rng = np.random.default_rng(1)
    xs = np.concatenate([rng.uniform(0, 2 * math.pi, 20000), rng.uniform(-50, 50, 5000), [0.0, math.pi, 2 * math.pi]]).astype(np.float32)
    for name, ref in (("sinf", np.sin), ("cosf", np.cos)):
        got = vec(getattr(L, "mort_oracle_" + name), xs)
        want = ref(xs.astype(np.float64)).astype(np.float32)
        # near zeros of the function the relative error of the fp64 reference itself matters; use abs there
        ok = (ulp_diff(got, want) <= 1) | (np.abs(got.astype(np.float64) - ref(xs.astype(np.float64))) < 1e-9)
        assert ok.all(), (name, xs[~ok][:5], got[~ok][:5], want[~ok][:5])


def test_sincosf_is_sinf_and_cosf(oracle):
    """The kernels evaluate sin and cos of random_cosine_direction's angle together (mort_sincosf): bit-identical
    to the separate functions, including out-of-domain, inf and NaN arguments."""
    import ctypes as C
    L = oracle.lib()
    L.mort_oracle_sincosf.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.mort_oracle_sincosf.restype = None
    rng = np.random.default_rng(3)
    xs = np.concatenate([rng.uniform(0, 2 * math.pi, 20000), rng.uniform(-1000, 1000, 5000),
                         [0.0, -0.0, math.pi, 2 * math.pi, 1e5, -1e5, 99999.99, 3e38, np.inf, -np.inf, np.nan]]).astype(np.float32)
    s, c = C.c_float(), C.c_float()
    for x in xs:
        L.mort_oracle_sincosf(float(x), C.byref(s), C.byref(c))
        want_s = np.float32(L.mort_oracle_sinf(float(x))); want_c = np.float32(L.mort_oracle_cosf(float(x)))
        assert np.float32(s.value).view(np.uint32) == want_s.view(np.uint32) or (np.isnan(s.value) and np.isnan(want_s)), x
        assert np.float32(c.value).view(np.uint32) == want_c.view(np.uint32) or (np.isnan(c.value) and np.isnan(want_c)), x


def test_sin_f64(oracle):
    L = oracle.lib()
    rng = np.random.default_rng(2)
    xs = rng.uniform(-500, 500, 20000)
    got = np.array([L.mort_oracle_sin(float(x)) for x in xs])
    assert np.max(np.abs(got - np.sin(xs))) < 5e-14


def test_acosf(oracle):
    L = oracle.lib()
    rng = np.random.default_rng(3)
    xs = np.concatenate([rng.uniform(-1, 1, 20000), [-1.0, 1.0, 0.0, -0.99999994, 0.99999994]]).astype(np.float32)
    got = vec(L.mort_oracle_acosf, xs)
    want = np.arccos(xs.astype(np.float64)).astype(np.float32)
    assert (ulp_diff(got, want) <= 1).all()
    assert math.isnan(L.mort_oracle_acosf(1.0000001)) and math.isnan(L.mort_oracle_acosf(-1.5))


def test_atan2f(oracle):
    L = oracle.lib()
    rng = np.random.default_rng(4)
    ys = rng.uniform(-2, 2, 20000).astype(np.float32)
    xs = rng.uniform(-2, 2, 20000).astype(np.float32)
    got = np.array([L.mort_oracle_atan2f(float(y), float(x)) for y, x in zip(ys, xs)], dtype=np.float32)
    want = np.arctan2(ys.astype(np.float64), xs.astype(np.float64)).astype(np.float32)
    assert (ulp_diff(got, want) <= 1).all()
    for y, x in ((0.0, 1.0), (0.0, -1.0), (1.0, 0.0), (-1.0, 0.0), (-0.0, -1.0), (1.0, 1.0), (-1.0, -1.0)):
        assert L.mort_oracle_atan2f(y, x) == pytest.approx(math.atan2(y, x), abs=1e-7)


def test_logf(oracle):
    L = oracle.lib()
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.uniform(0, 1, 20000), rng.uniform(0, 1e-30, 100), [1.0, 0.5, 5.9604645e-08]]).astype(np.float32)
    xs = xs[xs > 0]
    got = vec(L.mort_oracle_logf, xs)
    want = np.log(xs.astype(np.float64)).astype(np.float32)
    assert (ulp_diff(got, want) <= 1).all()
    assert L.mort_oracle_logf(0.0) == -math.inf
    assert math.isnan(L.mort_oracle_logf(-1.0))


# ---- (b) accuracy against mpmath ----
mpmath.mp.prec = 120
_MP = {"sinf": mpmath.sin, "cosf": mpmath.cos, "acosf": mpmath.acos, "logf": mpmath.log, "atan2f": mpmath.atan2, "sin": mpmath.sin, "cos": mpmath.cos, "atan": mpmath.atan}
_NP = {"sinf": np.sin, "cosf": np.cos, "acosf": np.arccos, "logf": np.log, "atan2f": np.arctan2, "sin": np.sin, "cos": np.cos, "atan": np.arctan}


def _rounded(v, mant_bits, e_min):
    """an mpf v != 0 rounded to nearest (ties to even) in a binary format of mant_bits + 1 significant bits and least normal exponent e_min,
    denormals included: (the rounded value, the spacing of the format at v)"""
    _, e = mpmath.frexp(abs(v))
    ulp = mpmath.ldexp(mpmath.mpf(1), max(int(e) - 1, e_min) - mant_bits)
    r = mpmath.nint(abs(v) / ulp) * ulp
    return (r if v > 0 else -r), ulp


def measure(oracle, name):
    """gcc's compile of mort_<name> over the fixed sample of its builder (MC.subsample: every edge family whole, a stride over the large
    families, 2^16 records at the most) against mpmath: dict(points with a finite non-zero exact result,
    not_cr = how many are not the correctly rounded result, worst = the largest error in units of the result format's spacing at the exact
    value, steps = the largest distance from the correctly rounded result in representable values).  Inputs whose exact result is not an
    ordinary number (NaN, infinities, zero, out of domain) are checked for their class and sign against numpy's float64 function."""
    fn = MC.FN[name]
    wide = name in ("sin", "cos", "atan")
    rec, edge = MC.subsample(fn)
    got = oracle.math_batch(fn, rec).view(np.float64 if wide else np.float32)[:, 0]
    args = rec.astype(np.float64)
    with np.errstate(all="ignore"):
        want64 = _NP[name](*args.T)
    in_domain = np.abs(args[:, 0]) < 1.0e5 if name in ("sinf", "cosf", "sin", "cos") else np.ones(len(rec), bool)
    ordinary = np.isfinite(args).all(1) & np.isfinite(want64) & (want64 != 0) & in_domain
    if name == "atan2f":
        ordinary &= args[:, 0] != 0  # the sign of a zero y chooses between +pi and -pi, and mpmath has one zero
    # everything else: the class, and the sign of a zero or an infinity
    rest = ~ordinary & in_domain
    assert (np.isnan(got[rest]) == np.isnan(want64[rest])).all(), name
    fin = rest & ~np.isnan(want64)
    if name == "atan2f":  # a zero y or an infinite argument: 0, +-pi, +-pi/2, +-pi/4, +-3pi/4 -- numpy's fp64 value rounded once, and the sign of a zero
        assert (got[fin] == want64[fin].astype(np.float32)).all()
        assert (np.signbit(got[fin]) == np.signbit(want64[fin])).all()
    else:
        assert (got[fin] == want64[fin]).all(), name
        # mort_sin(-0.0) and mort_atan(-0.0) return +0 where IEEE 754 recommends -0, on every compiler alike.  No caller passes -0 (phi is
        # (float)(2 pi r1) >= +0, the Perlin phase enters 1 + sin, mort_acosf's argument is a square root >= +0): DESIGN.md 2.
        signed = fin & ~((args[:, 0] == 0) & np.signbit(args[:, 0]) & (name in ("sin", "sinf", "atan")))
        assert (np.signbit(got[signed]) == np.signbit(want64[signed])).all(), name
    out = got[~in_domain & np.isfinite(args[:, 0])]
    assert (out == 0).all(), name  # out of domain: x - x
    mant, e_min = (52, -1022) if wide else (23, -126)
    not_cr, worst, steps = 0, mpmath.mpf(0), 0
    for a, g in zip(args[ordinary], got[ordinary]):
        v = _MP[name](*[mpmath.mpf(float(t)) for t in a])
        cr, ulp = _rounded(v, mant, e_min)
        g = mpmath.mpf(float(g))
        if g != cr:
            not_cr += 1
            steps = max(steps, int(mpmath.nint(abs(g - cr) / ulp)))
        worst = max(worst, abs(g - v) / ulp)
    return dict(points=int(ordinary.sum()), edge_rows=edge, sampled=len(rec), not_cr=not_cr, worst=float(worst), steps=steps)


# measured on gcc's compile over the fixed samples (MC.subsample: a builder's edge families whole -- 9 425 rows for sinf and cosf, 30 485 for
# atan2f, 29 837 for acosf, 34 828 for logf -- and a stride over its large families up to 2^16 records), precision 120 bits: every fp32 result
# is the correctly rounded one
FP32_MEASURED = {"sinf": (0, 0.4999977), "cosf": (0, 0.4999999976), "atan2f": (0, 0.49999999999), "acosf": (0, 0.4999998), "logf": (0, 0.49999997)}


@pytest.mark.parametrize("name", sorted(FP32_MEASURED))
def test_fp32_functions_against_mpmath(oracle, name):
    """The header's claim: each fp32 function is at most 1 ULP from the correctly rounded result (denormal results counted in the denormal
    spacing).  Measured: 0 results that are not correctly rounded for every function; the largest errors are in FP32_MEASURED as
    (not correctly rounded, largest error in ULP) and the count is asserted to stay 0.  mort_sincosf is bit for bit mort_sinf and mort_cosf
    over its whole builder (test_sincosf_over_the_whole_builder), so their figures are its own."""
    r = measure(oracle, name)
    print(name, r)
    assert r["points"] > 1 << 15 and r["edge_rows"] > 9000  # of at most 2^16 sampled; the rest are NaN, infinite, zero or out-of-domain cases
    assert r["steps"] <= 1, r            # the header's claim
    assert r["not_cr"] == FP32_MEASURED[name][0], r
    assert r["worst"] <= 0.5, r


# largest error of the fp64 functions in units of the fp64 result's spacing, measured the same way.  mort_sin / mort_cos reduce with a
# 86-bit pi/2: at the doubles nearest k * pi/2 the result is ~1e-16 * k with an absolute error near 1e-21, which is what these figures are
# (on [0, 2 pi] away from the zeros they stay below 1 ULP); mort_atan is a short series in plain fp64.
FP64_MEASURED = {"sin": 657875901.1, "cos": 780288820.7, "atan": 2.5440275}


@pytest.mark.parametrize("name", sorted(FP64_MEASURED))
def test_fp64_functions_against_mpmath(oracle, name):
    """mort_sin, mort_cos, mort_atan: the largest error against mpmath in ULP of the fp64 result stays within twice the measured value
    (FP64_MEASURED, also in DESIGN.md 2); the function and the inputs are deterministic, the factor only leaves room to reseed a builder."""
    r = measure(oracle, name)
    print(name, r)
    assert r["points"] > 10000
    assert r["worst"] <= 2 * FP64_MEASURED[name], r


def test_sincosf_over_the_whole_builder(oracle):
    rec, _ = MC.build(MC.FN["sincosf"])
    both = oracle.math_batch(MC.FN["sincosf"], rec)
    MC.assert_same(MC.FN["sinf"], rec, dict(sincosf=both[:, 0:1], sinf=oracle.math_batch(MC.FN["sinf"], rec)))
    MC.assert_same(MC.FN["cosf"], rec, dict(sincosf=both[:, 1:2], cosf=oracle.math_batch(MC.FN["cosf"], rec)))


# ---- (c) gcc against hipcc's host compile ----
def test_math_table_is_walkable_and_private(oracle):
    shapes = hip.debug_math_shapes()
    assert len(shapes) == len(MC.NAMES) and tuple(shapes[: len(oracle.MATH_SHAPES)]) == oracle.MATH_SHAPES
    for name in ("mort_hip_debug_math_shape", "mort_hip_debug_math_host", "mort_hip_debug_math_device", "mort_hip_debug_random_float_device"):
        assert name not in hip.EXPORTS and getattr(hip.lib(), name) is not None
    # the oracle's own copy of the table (mort_oracle.c) ends where the Python copy does
    assert oracle.lib().mort_oracle_math_batch(len(oracle.MATH_SHAPES) - 1, None, 0, None) == 0
    assert oracle.lib().mort_oracle_math_batch(len(oracle.MATH_SHAPES), None, 0, None) != 0
    with pytest.raises(hip.MortHipError):
        hip.debug_math_host(len(shapes), np.zeros(4, np.float32))
    with pytest.raises(hip.MortHipError):  # a table function without its table
        hip.debug_math_host(MC.FN["noise_value"], np.zeros((1, 4), np.uint32))


@pytest.mark.parametrize("fn", list(MC.GROUP_A) + list(MC.GROUP_P), ids=[MC.NAMES[f] for f in list(MC.GROUP_A) + list(MC.GROUP_P)])
def test_gcc_and_hipcc_host_compiles_agree(oracle, fn):
    """Bit for bit over the full builder, signed zeros included, a NaN as one word (both compilers generate x86's 0xffc00000 here, and
    propagate an argument's NaN unchanged: no raw word differs either -- recorded in DESIGN.md 2)"""
    rec, census = MC.build(fn)
    MC.assert_census(fn, census)
    MC.assert_same(fn, rec, dict(gcc=oracle.math_batch(fn, rec), hipcc_host=hip.debug_math_host(fn, rec)))


def test_plain_operators_against_numpy(oracle):
    """gcc's compile of the plain operators against numpy's (IEEE 754 on the same CPU, another code path): the division families with
    denormal and huge denominators and denormal quotients, the narrowing conversions' ties, truncf"""
    f, d = np.float32, np.float64
    with np.errstate(all="ignore"):
        for name, op in (("divf", lambda r: r[:, 0] / r[:, 1]), ("rcpf", lambda r: f(1) / r[:, 0]), ("div", lambda r: r[:, 0] / r[:, 1]),
                         ("d2f", lambda r: r[:, 0].astype(f)), ("u2f", lambda r: r[:, 0].astype(f)), ("truncf", lambda r: np.trunc(r[:, 0]))):
            rec, _ = MC.build(MC.FN[name])
            want = np.ascontiguousarray(op(rec))
            assert want.dtype == (d if name == "div" else f)
            MC.assert_same(MC.FN[name], rec, dict(gcc=oracle.math_batch(MC.FN[name], rec), numpy=want.view(np.uint32).reshape(len(rec), -1)))


# ---- (d) dev_math.h and dev_trace.h on the host compile ----
_RESTATED = list(MC.GROUP_B) + [MC.FN["sphere_uv"]]


@pytest.mark.parametrize("fn", _RESTATED, ids=[MC.NAMES[f] for f in _RESTATED])
def test_host_compile_against_numpy_restatement(oracle, fn):
    rec, census = MC.build(fn)
    MC.assert_census(fn, census)
    MC.assert_same(fn, rec, dict(hipcc_host=hip.debug_math_host(fn, rec), numpy=R.evaluate(fn, rec)))


def test_noise_value_against_the_oracle(oracle):
    fn = MC.FN["noise_value"]
    rec, census = MC.build(fn)
    MC.assert_census(fn, census)
    world, raw = MC.noise_world()
    want = oracle.texture_value_batch(world, S.TEXTURE_NOISE, rec[:, 0].astype(np.int32), 0, 0, rec[:, 1:4].view(np.float32))
    MC.assert_same(fn, rec, dict(hipcc_host=hip.debug_math_host(fn, rec, noise=raw), oracle=want.view(np.uint32)))
    # sin's phase s.z + 10 * turb next to a multiple of pi: the builder's leading pairs are one step of z apart and their colours
    # 0.5 * (1 + sin) lie on either side of 0.5 (MC._phase_brackets) ...
    k = 2 * census["phase_brackets_multiple_of_pi"]
    pair = want[:k, 0].reshape(-1, 2) > 0.5
    assert k >= 4096 and (pair[:, 0] != pair[:, 1]).all()
    assert (rec[:k:2, 1:3] == rec[1:k:2, 1:3]).all() and (np.nextafter(rec[:k:2, 3].view(np.float32), np.float32(np.inf)) == rec[1:k:2, 3].view(np.float32)).all()
    # ... and next to an odd multiple of pi/2 the colour is at a flat extremum that brackets nothing: colours within 2^-20 of 0 and of 1
    # (the phase within 2^-9.5 of the multiple) are counted instead
    v = want[:, 0].astype(np.float64)
    assert all(np.count_nonzero(np.abs(v - t) < 2.0 ** -20) > 0 for t in (0.0, 1.0))


def test_image_value_against_the_oracle(oracle):
    fn = MC.FN["image_value"]
    rec, census = MC.build(fn)
    MC.assert_census(fn, census)
    world, images, texels = MC.image_world()
    want = oracle.texture_value_batch(world, S.TEXTURE_IMAGE, rec[:, 0].astype(np.int32), rec[:, 1].view(np.float32), rec[:, 2].view(np.float32),
                                      np.zeros((len(rec), 3), np.float32))
    got = hip.debug_math_host(fn, rec, images=images, texels=texels)
    MC.assert_same(fn, rec, dict(hipcc_host=got, oracle=want.view(np.uint32)))
    # every texel of the 3 x 2 image was read, and u = 1 clamps the byte index, not the texel (textures.cuh:139-143): the row's last byte thrice
    im = MC.image_tables()[0][1]
    seen = {tuple(int(t) for t in c) for c in np.round(want[rec[:, 0] == 1].astype(np.float64) * 255)}
    assert seen == {tuple(int(t) for t in c) for c in im.reshape(-1, 3)} | {(int(row[-1, 2]),) * 3 for row in im}
