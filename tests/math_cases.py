"""Inputs for the sweeps of the math layer (tests/test_math.py on the CPU, tests/test_gpu_math.py on the device): one seeded builder per
function number of debug.hip's math table.  build(fn) returns (records, census): records is a (n, k) float32, float64 or uint32 array, one
row per input record, and census a dict of counts per input family that the tests assert to be positive, so that no family goes missing.

Families follow tests/test_gpu_exact_forms.py _values -- for every exponent of a range a random, an all-ones, a zero and a near-power
mantissa -- plus the edges each function has (see the builders)."""
import math

import numpy as np

F, D, U = np.float32, np.float64, np.uint32

NAMES = ["sqrtf", "sqrt", "floorf", "fmaxf", "fmin", "d2i", "powi5f", "sin", "cos", "sinf", "cosf", "sincosf", "atan", "atan2f", "acosf", "logf",
         "divf", "rcpf", "div", "d2f", "u2f", "truncf",
         "vlen", "vdiv", "vunit", "vcross", "reflect", "refract", "reflectance", "onb", "random_float_range", "random_int",
         "random_in_unit_sphere", "random_unit_vector", "random_in_unit_disk", "random_cosine_direction",
         "sphere_uv", "noise_value", "image_value"]
FN = {name: i for i, name in enumerate(NAMES)}
GROUP_A, GROUP_P, GROUP_B, GROUP_C = range(0, 16), range(16, 22), range(22, 36), range(36, 39)
N_AP, N_BC, N_NOISE = 1 << 22, 1 << 20, 1 << 18
RAGGED = (1 << 16) + 37          # one batch per group that ends inside a wave
RAGGED_FNS = (FN["atan2f"], FN["div"], FN["onb"], FN["sphere_uv"])

TWO_OVER_PI = 0.6366197723675814
PIO2_HI, PIO2_LO = 1.5707963267948966, 6.123233995736766e-17  # pi/2 as a double-double


# ---- families ----
def f32_families(rng, n, e_lo=-126, e_hi=128, signed=True):
    """n float32 with exponents e_lo <= e < e_hi, every exponent in turn; a quarter each with random, all-ones, zero and near-power mantissas"""
    span = e_hi - e_lo
    i = np.arange(n)
    e = e_lo + i % span
    kind = (i // span) % 4
    mant = rng.integers(0, 1 << 23, n, dtype=np.uint32)
    near = rng.integers(0, 4, n, dtype=np.uint32)
    near = np.where(rng.random(n) < 0.5, near, U((1 << 23) - 1) - near)
    mant = np.select([kind == 0, kind == 1, kind == 2], [mant, U((1 << 23) - 1), U(0)], near).astype(U)
    bits = ((e + 127).astype(U) << U(23)) | mant
    if signed:
        bits = bits | (rng.integers(0, 2, n, dtype=np.uint32) << U(31))
    return bits.view(F)


def f64_families(rng, n, e_lo=-1022, e_hi=1024, signed=True):
    span = e_hi - e_lo
    i = np.arange(n)
    e = e_lo + i % span
    kind = (i // span) % 4
    ones = np.uint64((1 << 52) - 1)
    mant = rng.integers(0, 1 << 52, n, dtype=np.uint64)
    near = rng.integers(0, 4, n, dtype=np.uint64)
    near = np.where(rng.random(n) < 0.5, near, ones - near)
    mant = np.select([kind == 0, kind == 1, kind == 2], [mant, ones, np.uint64(0)], near).astype(np.uint64)
    bits = ((e + 1023).astype(np.uint64) << np.uint64(52)) | mant
    if signed:
        bits = bits | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
    return bits.view(D)


def f32_denormals(rng, n):
    """the lowest 4096 patterns (zero included), the highest 64 denormals, random ones; both signs"""
    low = np.arange(4096, dtype=U)
    high = U(0x007fffff) - np.arange(64, dtype=U)
    rest = rng.integers(1, 1 << 23, max(n - 2 * (4096 + 64), 0), dtype=np.uint32)
    bits = np.concatenate([low, high, low | U(0x80000000), high | U(0x80000000), rest | (rng.integers(0, 2, len(rest), dtype=np.uint32) << U(31))])
    return bits.view(F)


def f64_denormals(rng, n):
    low = np.arange(1024, dtype=np.uint64)
    high = np.uint64((1 << 52) - 1) - np.arange(64, dtype=np.uint64)
    rest = rng.integers(1, 1 << 52, max(n - 2 * (1024 + 64), 0), dtype=np.uint64)
    s = np.uint64(1 << 63)
    return np.concatenate([low, high, low | s, high | s, rest | (rng.integers(0, 2, len(rest), dtype=np.uint64) << np.uint64(63))]).view(D)


def around32(v, k):
    """the 2k + 1 float32 patterns around v"""
    b = np.atleast_1d(np.asarray(v, F)).view(np.int32).astype(np.int64)
    key = np.where(b < 0, -(b & 0x7fffffff), b)[:, None] + np.arange(-k, k + 1)[None, :]  # ordered integers: -0 and +0 share 0
    out = np.where(key < 0, (-key) | 0x80000000, key).astype(np.uint32)
    return out.ravel().view(F)


def around64(v, k):
    b = np.atleast_1d(np.asarray(v, D)).view(np.int64)
    key = np.where(b < 0, -(b & np.int64(0x7fffffffffffffff)), b)[:, None] + np.arange(-k, k + 1, dtype=np.int64)[None, :]
    out = np.where(key < 0, ((-key).astype(np.uint64)) | np.uint64(1 << 63), key.astype(np.uint64))
    return out.ravel().view(D)


SPECIAL32 = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.17549435e-38, -1.17549435e-38, 1.0, -1.0, 0.5, -0.5, 2.0, -2.0,
                      3.4028235e38, -3.4028235e38, np.inf, -np.inf, np.nan], F)
SPECIAL64 = np.array([0.0, -0.0, 5e-324, -5e-324, 2.225073858507201e-308, -2.225073858507201e-308, 2.2250738585072014e-308, -2.2250738585072014e-308,
                      1.0, -1.0, 0.5, -0.5, 2.0, -2.0, 1.7976931348623157e308, -1.7976931348623157e308, np.inf, -np.inf, np.nan], D)


def _pairs(a, b):
    """every pair (a[i], b[j]) as two flat arrays"""
    x, y = np.meshgrid(a, b, indexing="ij")
    return x.ravel(), y.ravel()


def _finish(parts, n, filler, width, dtype):
    """the parts, then filler(n - their length) -- n rows of `width` columns exactly"""
    parts = [np.asarray(p, dtype).reshape(-1, width) for p in parts]
    have = sum(len(p) for p in parts)
    assert have <= n, (have, n)
    if have < n:
        parts.append(np.asarray(filler(n - have), dtype).reshape(-1, width))
    out = np.ascontiguousarray(np.concatenate(parts))
    assert out.shape == (n, width)
    return out


def _finish_edges(edges, big, n, filler, width, dtype):
    """_finish with the small edge families leading and the large ones next: (the rows, (how many rows from the top are edge rows, how many
    after them belong to the large families)); the filler comes last.  tests/test_math.py's mpmath sample takes the edge rows whole and a
    stride of the large families (subsample); the filler's kind of value is in the edge rows as one pass over every exponent."""
    edges = [np.asarray(p, dtype).reshape(-1, width) for p in edges]
    big = [np.asarray(p, dtype).reshape(-1, width) for p in big]
    return _finish(edges + big, n, filler, width, dtype), (sum(len(p) for p in edges), sum(len(p) for p in big))


def _count(cond):
    return int(np.count_nonzero(cond))


# ---- group A ----
def _sqrtf(rng, n):
    k = rng.integers(1, 4096, 1 << 16).astype(F) * np.ldexp(F(1), rng.integers(-60, 50, 1 << 16)).astype(F)
    sq = k * k
    x = _finish([SPECIAL32, f32_denormals(rng, 1 << 15), sq, np.nextafter(sq, F(0)), np.nextafter(sq, F(np.inf))], n, lambda m: f32_families(rng, m), 1, F)
    return x, dict(denormal=_count((x != 0) & (np.abs(x) < F(1.17549435e-38))), negative=_count(x < 0), nan=_count(np.isnan(x)), inf=_count(np.isinf(x)),
                   square=len(sq), zero=_count(x == 0))


def _sqrt(rng, n):
    k = rng.integers(1, 1 << 26, 1 << 16).astype(D) * np.ldexp(1.0, rng.integers(-500, 480, 1 << 16))
    sq = k * k
    x = _finish([SPECIAL64, f64_denormals(rng, 1 << 15), sq, np.nextafter(sq, 0.0), np.nextafter(sq, np.inf)], n, lambda m: f64_families(rng, m), 1, D)
    return x, dict(denormal=_count((x != 0) & (np.abs(x) < 2.2250738585072014e-308)), negative=_count(x < 0), nan=_count(np.isnan(x)), zero=_count(x == 0))


def _floorf(rng, n):
    ints = np.arange(-4096, 4097).astype(F)
    half = np.array([s * (8388608.0 + d) for s in (1, -1) for d in (-0.5, 0.5, 0.0, -1.0, 1.0)], F)  # 2^23 - 0.5 is a float, 2^23 + 0.5 rounds to 2^23
    big = (np.ldexp(F(1), np.arange(20, 33)).astype(F)[:, None] * np.array([1, -1], F)[None, :]).ravel()
    edges = np.concatenate([SPECIAL32, ints, around32(ints, 1), half, around32(half, 2), around32(big, 2), f32_denormals(rng, 1 << 14)])
    x = _finish([edges], n, lambda m: f32_families(rng, m, -30, 34), 1, F)
    return x, dict(negative_integer=_count((x < 0) & (x == np.floor(x)) & np.isfinite(x)), negative_zero=_count((x == 0) & np.signbit(x)),
                   just_below_integer=_count((x != np.floor(x)) & (np.nextafter(x, F(np.inf)) == np.ceil(x))),
                   two23=_count(np.abs(np.abs(x) - F(8388608)) <= 1), fraction=_count(x != np.floor(x)), nan=_count(np.isnan(x)))


def _minmax32(rng, n):
    a, b = _pairs(SPECIAL32, SPECIAL32)
    fam = f32_families(rng, 1 << 18)
    parts = [np.stack([a, b], 1), np.stack([fam, fam], 1), np.stack([fam, -fam], 1), np.stack([fam, np.nextafter(fam, F(0))], 1)]
    x = _finish(parts, n, lambda m: np.stack([f32_families(rng, m), rng.permutation(f32_families(rng, m))], 1), 2, F)
    return x, dict(nan_first=_count(np.isnan(x[:, 0]) & ~np.isnan(x[:, 1])), nan_second=_count(~np.isnan(x[:, 0]) & np.isnan(x[:, 1])),
                   both_nan=_count(np.isnan(x).all(1)), equal=_count(x[:, 0] == x[:, 1]),
                   zeros_of_two_signs=_count((x[:, 0] == 0) & (x[:, 1] == 0) & (np.signbit(x[:, 0]) != np.signbit(x[:, 1]))),
                   less=_count(x[:, 0] < x[:, 1]), greater=_count(x[:, 0] > x[:, 1]))


def _minmax64(rng, n):
    a, b = _pairs(SPECIAL64, SPECIAL64)
    fam = f64_families(rng, 1 << 18)
    one = np.stack([around64(1.0, 2048), np.ones(4097)], 1)  # refract's fmin(cos, 1.0)
    parts = [np.stack([a, b], 1), np.stack([fam, fam], 1), np.stack([fam, -fam], 1), np.stack([fam, np.nextafter(fam, 0.0)], 1), one]
    x = _finish(parts, n, lambda m: np.stack([f64_families(rng, m), rng.permutation(f64_families(rng, m))], 1), 2, D)
    return x, dict(nan_first=_count(np.isnan(x[:, 0]) & ~np.isnan(x[:, 1])), nan_second=_count(~np.isnan(x[:, 0]) & np.isnan(x[:, 1])),
                   both_nan=_count(np.isnan(x).all(1)), equal=_count(x[:, 0] == x[:, 1]),
                   zeros_of_two_signs=_count((x[:, 0] == 0) & (x[:, 1] == 0) & (np.signbit(x[:, 0]) != np.signbit(x[:, 1]))),
                   less=_count(x[:, 0] < x[:, 1]), greater=_count(x[:, 0] > x[:, 1]))


def _d2i(rng, n):
    edge = around64(np.array([2147483648.0, -2147483648.0, 2147483647.0, -2147483647.0, 2147483649.0, -2147483649.0]), 64)
    ties = (np.arange(-4096, 4096).astype(D) + 0.5)
    ties = np.concatenate([ties, around64(ties, 1), np.array([0.5, -0.5, 2147483647.5, -2147483648.5, 2147483646.5])])
    x = _finish([SPECIAL64, edge, ties, f64_denormals(rng, 1 << 12), f64_families(rng, 1 << 16)], n, lambda m: f64_families(rng, m, -8, 40), 1, D)
    return x, dict(saturates_high=_count(x >= 2147483648.0), saturates_low=_count(x <= -2147483648.0), last_in_range=_count((x > 2147483647.0) & (x < 2147483648.0)),
                   tie=_count((np.abs(x) < 1e9) & (x - np.trunc(x) == 0.5)) + _count((np.abs(x) < 1e9) & (x - np.trunc(x) == -0.5)), nan=_count(np.isnan(x)), inf=_count(np.isinf(x)),
                   in_range=_count(np.abs(x) < 2147483648.0))


def _powi5f(rng, n):
    x = _finish([SPECIAL32, f32_denormals(rng, 1 << 12), f32_families(rng, 1 << 18, -40, -20), f32_families(rng, 1 << 18, 20, 30),
                 (F(1) - rng.random(1 << 18, dtype=F))], n, lambda m: f32_families(rng, m), 1, F)
    with np.errstate(all="ignore"):
        p = x.astype(D) ** 5
    return x, dict(denormal_result=_count((p != 0) & (np.abs(p) < 1.17549435e-38) & (np.abs(p) > 1e-45)), overflow=_count(np.abs(p) > 3.5e38) ,
                   underflow=_count((x != 0) & (np.abs(p) < 1e-46)), unit_range=_count((x >= 0) & (x <= 1)), nan=_count(np.isnan(x)))


def _kpio2_64():
    """the doubles nearest k * pi/2 for every k with |x| < 1e5, and nearest (k + 1/2) * pi/2 (the quadrant ties of mort_rem_pio2)"""
    k = np.arange(-63661, 63662).astype(np.longdouble)
    k = np.concatenate([k, k + np.longdouble(0.5)])
    return (k * np.longdouble(PIO2_HI) + k * np.longdouble(PIO2_LO)).astype(D)


def _trig_census(x):
    xd = x.astype(D)
    ok = np.abs(xd) < 1.0e5
    kd = xd[ok] * TWO_OVER_PI
    k = np.trunc(np.where(kd < 0.0, kd - 0.5, kd + 0.5)).astype(np.int64)
    c = {f"quadrant{q}": _count((k & 3) == q) for q in range(4)}
    c.update(out_of_domain=_count(~ok & np.isfinite(xd)), inf=_count(np.isinf(xd)), nan=_count(np.isnan(xd)), zero=_count(xd == 0), negative=_count(xd < 0),
             workload=_count((xd >= 0) & (xd <= 2 * math.pi)), large=_count(ok & (np.abs(xd) > 5.0e4)),
             at_domain_bound=_count(np.abs(np.abs(xd) - 1.0e5) < 0.02), near_quadrant_tie=_count(np.abs(np.abs(kd - np.trunc(kd)) - 0.5) < 1e-6))
    return c


def _trig32(rng, n):
    near = _kpio2_64().astype(F)
    bound = around32(np.array([1e5, -1e5], F), 2)
    dense = np.concatenate([np.linspace(0, 2 * math.pi, 1 << 18).astype(F), (rng.random(1 << 19) * 2 * math.pi).astype(F)])
    ties = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5]) / TWO_OVER_PI  # kd on or next to a half
    x, k = _finish_edges([SPECIAL32, bound, f32_denormals(rng, 1 << 12), around32(ties.astype(F), 4),
                          np.array([0.78539816, 2.3561945, 3.9269908, 5.497787, 3.1415927, 6.2831855], F), f32_families(rng, 4 * 254)],
                         [near, np.nextafter(near, F(-np.inf)), np.nextafter(near, F(np.inf)), dense, f32_families(rng, 1 << 16)],
                         n, lambda m: f32_families(rng, m, -126, 17), 1, F)
    return x, k, _trig_census(x)


def _trig64(rng, n):
    near = _kpio2_64()
    bound = around64(np.array([1e5, -1e5]), 2)
    dense = np.concatenate([np.linspace(0, 2 * math.pi, 1 << 18), rng.random(1 << 19) * 2 * math.pi])
    ties = (np.arange(-2048, 2048) + 0.5) / TWO_OVER_PI
    x, k = _finish_edges([SPECIAL64, SPECIAL32.astype(D), bound, f64_denormals(rng, 1 << 12), around64(ties[1792:2304], 2), f64_families(rng, 4 * 2046)],
                         [near, np.nextafter(near, -np.inf), np.nextafter(near, np.inf), dense, around64(ties, 2), f64_families(rng, 1 << 16)],
                         n, lambda m: f64_families(rng, m, -1022, 17), 1, D)
    return x, k, _trig_census(x)


ATAN_BREAKS = np.array([0.125, 0.375, 0.625, 0.875, 1.0])


def _atan(rng, n):
    brk = around64(np.concatenate([ATAN_BREAKS, -ATAN_BREAKS]), 1024)
    with np.errstate(all="ignore"):
        inv = 1.0 / brk
    x, k = _finish_edges([SPECIAL64, brk, inv, f64_denormals(rng, 1 << 12), f64_families(rng, 4 * 2046)], [f32_families(rng, 1 << 18).astype(D)], n, lambda m: f64_families(rng, m), 1, D)
    a = np.abs(x)
    c = {f"below_break{i}": _count((a < b) & (a > b - 1e-12)) for i, b in enumerate(ATAN_BREAKS)}
    c.update({f"segment{i}": _count((a <= 1) & (a >= lo) & (a < hi)) for i, (lo, hi) in enumerate(zip([0, .125, .375, .625, .875], [.125, .375, .625, .875, 1.5]))})
    c.update(reciprocal=_count(a > 1), one=_count(a == 1), nan=_count(np.isnan(x)), inf=_count(np.isinf(x)), negative=_count(x < 0), denormal=_count((a > 0) & (a < 2.2250738585072014e-308)))
    return x, k, c


def _atan2f(rng, n):
    f = F
    mags = np.array([0.0, 1e-45, 1e-40, 1.0, 3e38, np.inf], f)
    vals = np.concatenate([mags, -mags, [f(np.nan)]])
    sy, sx = _pairs(vals, vals)
    m = 1 << 18
    fam = f32_families(rng, m)
    sgn = lambda k: np.where(rng.random(k) < 0.5, f(-1), f(1))
    equal = np.stack([fam, fam * sgn(m)], 1)                                      # |y| == |x|
    # ratios next to the break points: x a family value, y = fl(x * b) moved by up to 2 places, both ways round
    xs = f32_families(rng, 5 * m, -100, 100)
    b = np.tile(ATAN_BREAKS.astype(f), m)
    ys = (np.abs(xs) * b).view(np.int32) + rng.integers(-2, 3, 5 * m).astype(np.int32)
    ys = ys.view(f) * sgn(5 * m)
    swap = (np.arange(5 * m) % 2 == 1)[:, None]
    ratio = np.where(swap, np.stack([xs, ys], 1), np.stack([ys, xs], 1))
    # exponent differences from -250 to 250
    d = np.arange(-250, 251)
    ey = rng.integers(-126, 128, (64, len(d)))
    ex = ey - d[None, :]
    ok = (ex >= -149) & (ex < 128) & (ey >= -126)
    mk = lambda e: (np.ldexp(1.0 + rng.random(e.shape), e)).astype(f) * sgn(e.size).reshape(e.shape)
    with np.errstate(all="ignore"):
        diff = np.stack([mk(ey)[ok], mk(ex)[ok]], 1)
    far = np.abs(np.broadcast_to(d[None, :], ok.shape)[ok]) >= 240                # the extremes of the exponent difference, whole
    # the break points on a few exact scales, the quotient moved by up to 2 places, both ways round and every pair of signs
    bx, bb, bs, b1, b2 = (a.ravel() for a in np.meshgrid(np.ldexp(f(1), np.arange(-120, 121, 8)).astype(f), ATAN_BREAKS.astype(f), np.arange(-2, 3), [1, -1], [1, -1], indexing="ij"))
    by = ((bx * bb).view(np.int32) + bs.astype(np.int32)).view(f)
    brk = np.concatenate([np.stack([by * b1.astype(f), bx * b2.astype(f)], 1), np.stack([bx * b1.astype(f), by * b2.astype(f)], 1)])
    den = f32_denormals(rng, 1 << 12)[:8000]
    x, n_edge = _finish_edges([np.stack([sy, sx], 1), diff[far], brk, np.stack([den, f32_families(rng, 8000)], 1), np.stack([f32_families(rng, 8000), den], 1), np.stack([den, rng.permutation(den)], 1)],
                              [equal, ratio, diff[~far]], n, lambda k: np.stack([f32_families(rng, k), rng.permutation(f32_families(rng, k, -126, 128))], 1), 2, f)
    y64, x64 = x[:, 0].astype(D), x[:, 1].astype(D)
    ay, ax = np.abs(y64), np.abs(x64)
    fin = np.isfinite(ay) & np.isfinite(ax) & (ay > 0) & (ax > 0)
    with np.errstate(all="ignore"):
        r = np.where(ax >= ay, ay / ax, ax / ay)
        ed = np.where(fin, np.log2(ay) - np.log2(ax), 0)
    c = {f"near_break{i}": _count(fin & (np.abs(r - bb) < 1e-6 * bb)) for i, bb in enumerate(ATAN_BREAKS)}
    c.update({f"below_break{i}": _count(fin & (r < bb) & (bb - r < 1e-6 * bb)) for i, bb in enumerate(ATAN_BREAKS)})
    c.update(ax_ge_ay=_count(fin & (ax >= ay)), ax_lt_ay=_count(fin & (ax < ay)), equal=_count(fin & (ax == ay)), y_zero=_count(ay == 0), x_zero=_count((ax == 0) & (ay != 0)),
             inf_inf=_count(np.isinf(ay) & np.isinf(ax)), nan=_count(np.isnan(y64) | np.isnan(x64)), far_apart_low=_count(ed < -240), far_apart_high=_count(ed > 240),
             **{f"signs{int(a)}{int(bq)}": _count((np.signbit(y64) == a) & (np.signbit(x64) == bq)) for a in (0, 1) for bq in (0, 1)})
    return x, n_edge, c


def _acosf(rng, n):
    one = np.concatenate([around32(F(1), 4096), around32(F(-1), 4096)])
    outside = f32_families(rng, 1 << 16, 0, 128)
    dense = (rng.random(1 << 20) * 2 - 1).astype(F)
    x, k = _finish_edges([SPECIAL32, one, f32_denormals(rng, 1 << 13), f32_families(rng, 4 * 254), outside[:4096]], [outside, dense], n, lambda m: f32_families(rng, m, -126, 0), 1, F)
    a = np.abs(x.astype(D))
    return x, k, dict(just_inside_plus=_count((x < 1) & (x > F(0.9995))), just_outside_plus=_count((x > 1) & (x < F(1.0005))), just_inside_minus=_count((x > -1) & (x < F(-0.9995))),
                   just_outside_minus=_count((x < -1) & (x > F(-1.0005))), plus_one=_count(x == 1), minus_one=_count(x == -1), zero=_count(x == 0), denormal=_count((a > 0) & (a < 1.17549435e-38)),
                   outside=_count(a > 1), tiny=_count((a > 0) & (a < 1e-30)), nan=_count(np.isnan(x)))


def _logf(rng, n):
    low = np.arange(4096, dtype=U).view(F)
    one = around32(F(1), 2048)
    g = np.concatenate([np.arange(2048, dtype=U), U(0xffffffff) - np.arange(0, 1 << 19, 256, dtype=U), rng.integers(0, 1 << 32, 1 << 19, dtype=np.uint64).astype(U)])
    u = g.astype(F) * F(2.3283064e-10) + F(2.3283064e-10) / F(2.0)   # curand_uniform: (0, 1], down to 2^-33
    rf = F(1) - u                                                      # random_float: [0, 1), up to 1 - 2^-24
    neg = -f32_families(rng, 1 << 10, signed=False)
    x, k = _finish_edges([SPECIAL32, low, one, u[:4096], rf[:4096], neg, f32_denormals(rng, 1 << 14), f32_families(rng, 4 * 254, signed=False)], [u[4096:], rf[4096:]],
                         n, lambda m: f32_families(rng, m, signed=False), 1, F)
    return x, k, dict(denormal=_count((x > 0) & (x < F(1.17549435e-38))), near_one=_count((x != 1) & (np.abs(x - F(1)) < F(1e-4))), one=_count(x == 1), largest_below_one=_count(x == F(1 - 2.0 ** -24)),
                   scale_2_33=_count((x > 0) & (x < F(2.0 ** -32))), zero=_count((x == 0) & ~np.signbit(x)), negative_zero=_count((x == 0) & np.signbit(x)), negative=_count(x < 0),
                   inf=_count(x == np.inf), nan=_count(np.isnan(x)), unit_range=_count((x > 0) & (x <= 1)), above_sqrt2_mantissa=_count(np.frexp(x.astype(D))[0] * 2 > 1.4142135623730951))


# ---- group P ----
def _divf(rng, n):
    f = F
    sx, sa = _pairs(SPECIAL32, SPECIAL32)
    ea, ex = _pairs(np.arange(-126, 128), np.arange(-126, 128))
    ones = (((ea + 127).astype(U) << U(23)) | U((1 << 23) - 1)).view(f)       # all-ones mantissa under a power-of-two numerator
    pw = np.ldexp(f(1), ex).astype(f)
    m = 1 << 18
    den_a = f32_denormals(rng, m)[:m]                                          # denormal denominators
    huge_a = f32_families(rng, m, 100, 128)
    # quotients that are denormal: exponent(x) - exponent(a) in [-150, -125]
    qa = f32_families(rng, m, -20, 128)
    with np.errstate(all="ignore"):
        qx = (qa.astype(D) * np.ldexp(1.0 + rng.random(m), rng.integers(-150, -124, m))).astype(f)
    fx = f32_families(rng, m)
    parts = [np.stack([sx, sa], 1), np.stack([pw, ones], 1), np.stack([-pw, ones], 1), np.stack([f32_families(rng, m), den_a], 1), np.stack([f32_families(rng, m), huge_a], 1),
             np.stack([qx, qa], 1), np.stack([fx, np.zeros(m, f)], 1), np.stack([fx, -np.zeros(m, f)], 1)]
    x = _finish(parts, n, lambda k: np.stack([f32_families(rng, k), rng.permutation(f32_families(rng, k))], 1), 2, f)
    with np.errstate(all="ignore"):
        q = np.abs(x[:, 0].astype(D) / x[:, 1].astype(D))
    a = np.abs(x[:, 1])
    return x, dict(denormal_denominator=_count((a > 0) & (a < f(1.17549435e-38))), huge_denominator=_count((a > f(1e30)) & np.isfinite(a)), denormal_quotient=_count((q > 1e-45) & (q < 1.17549435e-38)),
                   zero_over_zero=_count((x[:, 0] == 0) & (a == 0)), over_plus_zero=_count((x[:, 0] != 0) & (a == 0) & ~np.signbit(x[:, 1])), over_minus_zero=_count((x[:, 0] != 0) & (a == 0) & np.signbit(x[:, 1])),
                   all_ones_under_power=2 * len(ones), overflow=_count((q >= 3.4028235677973366e38) & np.isfinite(x).all(1) & (a > 0)), underflow=_count((q < 1e-46) & (x[:, 0] != 0) & np.isfinite(a)), nan=_count(np.isnan(x).any(1)))


def _rcpf(rng, n):
    pw = np.ldexp(F(1), np.arange(-149, 128)).astype(F)
    x = _finish([SPECIAL32, pw, -pw, around32(pw, 2), f32_denormals(rng, 1 << 16), f32_families(rng, 1 << 18, 120, 128)], n, lambda m: f32_families(rng, m), 1, F)
    a = np.abs(x.astype(D))
    return x, dict(denormal=_count((a > 0) & (a < 1.17549435e-38)), denormal_result=_count(a > 2.0 ** 126) - _count(np.isinf(a)), overflow=_count((a > 0) & (a < 2.0 ** -128)), zero=_count(a == 0),
                   inf=_count(np.isinf(a)), nan=_count(np.isnan(a)), power_of_two=_count(np.frexp(a)[0] == 0.5))


def _div(rng, n):
    sx, sa = _pairs(SPECIAL64, SPECIAL64)
    m = 1 << 18
    ea, ex = rng.integers(-1022, 1024, m), rng.integers(-1022, 1024, m)
    ones = (((ea + 1023).astype(np.uint64) << np.uint64(52)) | np.uint64((1 << 52) - 1)).view(D)
    pw = np.ldexp(1.0, ex)
    qa = f64_families(rng, m, -50, 1024)
    with np.errstate(all="ignore"):
        qx = qa * np.ldexp(1.0 + rng.random(m), rng.integers(-1074, -1020, m).astype(np.int64) - np.frexp(qa)[1] + 1)  # |x / a| in the denormal range
    fx = f64_families(rng, m)
    parts = [np.stack([sx, sa], 1), np.stack([pw, ones], 1), np.stack([-pw, ones], 1), np.stack([f64_families(rng, m), f64_denormals(rng, m)[:m]], 1),
             np.stack([f64_families(rng, m), f64_families(rng, m, 900, 1024)], 1), np.stack([qx, qa], 1), np.stack([fx, np.zeros(m)], 1), np.stack([fx, -np.zeros(m)], 1),
             np.stack([f32_families(rng, m).astype(D), f32_families(rng, m).astype(D)], 1)]
    x = _finish(parts, n, lambda k: np.stack([f64_families(rng, k), rng.permutation(f64_families(rng, k))], 1), 2, D)
    a = np.abs(x[:, 1])
    with np.errstate(all="ignore"):
        q = np.abs(x[:, 0] / x[:, 1])
    return x, dict(denormal_denominator=_count((a > 0) & (a < 2.2250738585072014e-308)), huge_denominator=_count((a > 1e300) & np.isfinite(a)), denormal_quotient=_count((q > 0) & (q < 2.2250738585072014e-308)),
                   zero_over_zero=_count((x[:, 0] == 0) & (a == 0)), over_plus_zero=_count((x[:, 0] != 0) & (a == 0) & ~np.signbit(x[:, 1])), over_minus_zero=_count((x[:, 0] != 0) & (a == 0) & np.signbit(x[:, 1])),
                   all_ones_under_power=2 * m, nan=_count(np.isnan(x).any(1)))


def _d2f(rng, n):
    m = 1 << 18
    fl = f32_families(rng, m)
    up = np.nextafter(fl, F(np.inf))
    with np.errstate(all="ignore"):
        mid = (fl.astype(D) + up.astype(D)) / 2                                  # exactly between two floats: ties to even
    den = f32_denormals(rng, m)[:m]
    dmid = (den.astype(D) + np.nextafter(den, F(np.inf)).astype(D)) / 2
    small = f64_families(rng, m, -160, -120)                                    # narrows to a denormal, to the least normal, or to zero
    top = around64(np.array([3.4028234663852886e38, 3.4028235677973366e38, -3.4028235677973366e38]), 64)  # FLT_MAX and the overflow threshold
    x = _finish([SPECIAL64, SPECIAL32.astype(D), mid, around64(mid[: 1 << 15], 1), dmid, around64(dmid[: 1 << 15], 1), small, top, fl.astype(D)], n, lambda k: f64_families(rng, k), 1, D)
    a = np.abs(x)
    return x, dict(denormal_result=_count((a >= 2.0 ** -149) & (a < 2.0 ** -126)), underflow_to_zero=_count((a > 0) & (a < 2.0 ** -150)), half_of_least=_count(a == 2.0 ** -150),
                   tie=len(mid) + len(dmid), overflow=_count((a >= 3.4028235677973366e38) & np.isfinite(a)), inf=_count(np.isinf(a)), nan=_count(np.isnan(a)), exact=_count(a.astype(F).astype(D) == a))


def _u2f(rng, n):
    k = rng.integers(0, 1 << 24, 1 << 18, dtype=np.uint64)
    sh = rng.integers(1, 9, 1 << 18).astype(np.uint64)
    tie = (((k | np.uint64(1 << 23)) << sh) | (np.uint64(1) << (sh - np.uint64(1)))) & np.uint64(0xffffffff)  # a half of the last place kept
    edges = np.array([0, 1, 2, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 2, (1 << 24) + 3, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 31) + 128, (1 << 31) + 129,
                      0xffffff7f, 0xffffff80, 0xffffff81, 0xfffffffe, 0xffffffff], np.uint64)
    low = np.arange(1 << 16, dtype=np.uint64)
    high = np.uint64(0xffffffff) - low
    x = _finish([edges, tie, tie + np.uint64(1), tie - np.uint64(1), low, high], n, lambda m: rng.integers(0, 1 << 32, m, dtype=np.uint64), 1, np.uint64).astype(U)
    xl = x.astype(np.uint64)
    return np.ascontiguousarray(x), dict(exact=_count(xl < (1 << 24)), inexact=_count(xl.astype(F).astype(np.float64) != xl.astype(np.float64)), rounds_to_2_32=_count(xl >= 0xffffff80), zero=_count(xl == 0),
                                         top_bit=_count(xl >= (1 << 31)))


# ---- group B ----
def _vec_scales(rng, n, e_lo, e_hi):
    """n float32 3-vectors: random directions at lengths 2^e_lo .. 2^e_hi"""
    v = rng.standard_normal((n, 3))
    v /= np.sqrt((v * v).sum(1, keepdims=True))
    with np.errstate(all="ignore"):
        return (v * np.ldexp(1.0 + rng.random((n, 1)), rng.integers(e_lo, e_hi, (n, 1)))).astype(F)


def _axis_vectors():
    """axis-aligned vectors with +0 / -0 in the other components, at several lengths, and the zero vectors"""
    out = []
    for axis in range(3):
        for s in (1.0, -1.0):
            for length in (1.0, 0.5, 3.0, 1e-45, 1e-40, 2.0 ** 60, 2.0 ** 63, 3e38):
                for z1 in (0.0, -0.0):
                    for z2 in (0.0, -0.0):
                        v = [z1, z2]
                        v.insert(axis, s * length)
                        out.append(v)
    for z in ((0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (0.0, -0.0, 0.0), (-0.0, 0.0, -0.0)):
        out.append(list(z))
    return np.array(out, F)


def _near_09(rng, n):
    """vectors whose unit vector has |x| within a few places of 0.9 (onb_from_w's branch): (t, sqrt(1 - t^2) split over y and z) * scale"""
    t = around32(F(0.9), 8)[rng.integers(0, 17, n)].astype(D)
    rest = np.sqrt(1 - t * t)
    phi = rng.random(n) * 2 * math.pi
    split = rng.integers(0, 3, n)
    y = np.where(split == 0, rest, np.where(split == 1, 0.0, rest * np.cos(phi)))
    z = np.where(split == 0, 0.0, np.where(split == 1, rest, rest * np.sin(phi)))
    scale = np.ldexp(1.0, rng.integers(-20, 21, n)) * np.where(rng.random(n) < 0.3, 1.0, 1.0 + rng.random(n))
    sgn = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return (np.stack([sgn * t, y, z], 1) * scale[:, None]).astype(F)


def _w_vectors(rng, n):
    """vunit / onb_from_w inputs"""
    m = n // 8
    return _finish([_axis_vectors(), _vec_scales(rng, m, -149, -120), _vec_scales(rng, m, 58, 64), _vec_scales(rng, m, -75, -55), _near_09(rng, 2 * m),
                    f32_families(rng, 3 * m).reshape(-1, 3), np.array([[np.nan, 1, 0], [np.inf, 1, 1], [1, -np.inf, 0], [3e38, 3e38, 3e38]], F)], n,
                   lambda k: _vec_scales(rng, k, -10, 10), 3, F)


def _w_census(w):
    from tests import math_restate as R
    with np.errstate(all="ignore"):
        ux = np.abs(R.vunit(w)[:, 0])
        ln = R.vlen(w)
    b = ux.view(np.int32).astype(np.int64) - int(F(0.9).view(np.int32))
    nz = (w != 0).sum(1)
    with np.errstate(all="ignore"):
        l2 = R.vlen2(w)
    return dict(zero=_count(nz == 0), denormal_squared_length=_count((l2 > 0) & (l2 < F(1.17549435e-38))), denormal_length=_count((nz > 0) & (np.abs(w).max(1) < F(1.17549435e-38))), length_2_60=_count((ln >= F(2.0 ** 60)) & np.isfinite(ln)), length_overflows=_count(np.isinf(ln) & np.isfinite(w).all(1)),
                axis_aligned=_count(nz == 1), negative_zero_component=_count(((w == 0) & np.signbit(w)).any(1)), branch_x_above_09=_count(ux.astype(D) > 0.9), branch_x_not_above_09=_count(ux.astype(D) <= 0.9),
                within_4_above_09=_count((b > 0) & (b <= 4)), within_4_up_to_09=_count((b <= 0) & (b >= -4)), unit_is_nan=_count(np.isnan(ux)))


def _vlen(rng, n):
    w = _w_vectors(rng, n)
    c = _w_census(w)
    return w, {k: c[k] for k in ("zero", "denormal_length", "length_2_60", "length_overflows", "axis_aligned", "negative_zero_component")}


def _vunit(rng, n):
    w = _w_vectors(rng, n)
    return w, _w_census(w)


def _onb(rng, n):
    w = _w_vectors(rng, n)
    a = _vec_scales(rng, n, -2, 2)
    a[: 1 << 16] = f32_families(rng, 3 << 16, -20, 20).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([w, a], 1)), _w_census(w)


def _vdiv(rng, n):
    m = 1 << 16
    ts = np.concatenate([SPECIAL32, f32_denormals(rng, m), f32_families(rng, m, 100, 128), f32_families(rng, m, -126, -100)])
    t = _finish([ts], n, lambda k: f32_families(rng, k), 1, F)
    v = _finish([_axis_vectors()], n, lambda k: f32_families(rng, 3 * k).reshape(-1, 3), 3, F)
    v = v[rng.permutation(n)]
    x = np.ascontiguousarray(np.concatenate([v, t], 1))
    a = np.abs(t[:, 0].astype(D))
    return x, dict(denormal_t=_count((a > 0) & (a < 1.17549435e-38)), huge_t=_count((a > 1e30) & np.isfinite(a)), reciprocal_denormal=_count((a > 2.0 ** 126) & np.isfinite(a)), reciprocal_overflows=_count((a > 0) & (a < 2.0 ** -128)),
                   zero_t=_count(a == 0), inf_t=_count(np.isinf(a)), nan_t=_count(np.isnan(a)), zero_component=_count((v == 0).any(1)))


def _two_vectors(rng, n):
    m = n // 4
    u = _finish([_axis_vectors()], n, lambda k: np.concatenate([_vec_scales(rng, k - k // 2, -3, 3), f32_families(rng, 3 * (k // 2)).reshape(-1, 3)]), 3, F)
    v = _finish([_axis_vectors()[::-1]], n, lambda k: np.concatenate([_vec_scales(rng, k - k // 2, -3, 3), f32_families(rng, 3 * (k // 2), -60, 60).reshape(-1, 3)]), 3, F)
    v[m: 2 * m] = u[m: 2 * m]                                                    # parallel: the cross product cancels
    v[2 * m: 2 * m + 1000] = -u[2 * m: 2 * m + 1000]
    x = np.ascontiguousarray(np.concatenate([u, v], 1))
    return x, dict(parallel=_count((u == v).all(1)), opposite=_count((u == -v).all(1) & (u != 0).any(1)), zero_component=_count((x == 0).any(1)), negative_zero=_count(((x == 0) & np.signbit(x)).any(1)),
                   wide_range=_count(np.abs(x).max(1) > F(1e20)), unit_scale=_count((np.abs(x).max(1) < 16) & (np.abs(x).max(1) > F(0.01))))


ETAS = (F(1.5), F(1.0) / F(1.5))


def _refract(rng, n):
    m = n // 8
    unit = lambda k: _unit64(rng, k)
    nrm = unit(n)
    # (a) uv = -n up to rounding: cos_theta lands on either side of 1
    uv_a = -nrm[:m]
    # (b) near the critical angle of eta = 1.5: sin(theta) = (2 / 3)(1 + d), d of either sign and down to the last place
    t = _tangent(rng, nrm[m: 3 * m])
    d = np.where(rng.random(2 * m) < 0.5, -1.0, 1.0) * np.ldexp(1.0, rng.integers(-26, -8, 2 * m)) * rng.random(2 * m)
    s = (2.0 / 3.0) * (1 + d)
    uv_b = s[:, None] * t - np.sqrt(1 - s * s)[:, None] * nrm[m: 3 * m]
    # (c) grazing and random incidence, (d) lengths off 1, (e) wild values
    ct = rng.random(m) ** 4
    t2 = _tangent(rng, nrm[3 * m: 4 * m])
    uv_c = np.sqrt(1 - ct * ct)[:, None] * t2 - ct[:, None] * nrm[3 * m: 4 * m]
    uv_d = unit(m) * (1 + (rng.random((m, 1)) - 0.5) * 1e-3)
    uv = _finish([uv_a, uv_b, uv_c, uv_d, f32_families(rng, 3 * m).reshape(-1, 3)], n, lambda k: unit(k), 3, F)
    nf = nrm.astype(F)
    nf[4 * m + 7: 5 * m: 13] = _axis_vectors()[0]
    eta = np.where(np.arange(n) % 2 == 0, ETAS[0], ETAS[1]).astype(F)
    eta[2 * m: 3 * m] = ETAS[0]
    eta[5 * m: 5 * m + 64] = f32_families(rng, 64)
    uv[5 * m + 64: 5 * m + 70] = np.array([[np.nan, 0, 0], [np.inf, 0, 0], [0, -np.inf, 0], [3e38, 3e38, 0], [0, 0, 0], [-0.0, -0.0, -0.0]], F)
    x = np.ascontiguousarray(np.concatenate([uv, nf, eta[:, None]], 1))
    from tests import math_restate as R
    with np.errstate(all="ignore"):
        dot = R.vdot(-x[:, 0:3], x[:, 3:6]).astype(D)
        cos = np.fmin(dot, 1.0)
        perp = x[:, 6:7] * (x[:, 0:3] + cos.astype(F)[:, None] * x[:, 3:6])
        left = 1.0 - R.vlen2(perp).astype(D)
    return x, dict(cos_above_one=_count(dot > 1), cos_is_one=_count(dot == 1), cos_just_below_one=_count((dot < 1) & (dot > 1 - 1e-6)), total_reflection=_count(left < 0), refracted=_count(left > 0),
                   crossing_above=_count((left > 0) & (left < 4e-7)), crossing_below=_count((left < 0) & (left > -4e-7)), crossing_zero=_count(left == 0), eta_15=_count(x[:, 6] == ETAS[0]), eta_inv=_count(x[:, 6] == ETAS[1]),
                   nan=_count(np.isnan(left)))


def _unit64(rng, k):
    v = rng.standard_normal((k, 3))
    return v / np.sqrt((v * v).sum(1, keepdims=True))


def _tangent(rng, nrm):
    r = _unit64(rng, len(nrm))
    t = r - (r * nrm).sum(1, keepdims=True) * nrm
    return t / np.sqrt((t * t).sum(1, keepdims=True))


def _reflectance(rng, n):
    m = 1 << 16
    cos = np.concatenate([SPECIAL32, around32(np.array([0, 1], F), 64), rng.random(m, dtype=F), F(1) - rng.random(m, dtype=F) * F(1e-3), f32_families(rng, m)])
    idx = np.concatenate([ETAS[0] * np.ones(m // 2, F), ETAS[1] * np.ones(m // 2, F), SPECIAL32, around32(F(-1), 16), around32(F(1), 16), f32_families(rng, m)])
    c, i = cos[rng.integers(0, len(cos), n)], idx[rng.integers(0, len(idx), n)]
    pc, pi_ = _pairs(SPECIAL32, SPECIAL32)
    c[: len(pc)], i[: len(pc)] = pc, pi_
    x = np.ascontiguousarray(np.stack([c, i], 1))
    return x, dict(workload=_count((c >= 0) & (c <= 1) & ((i == ETAS[0]) | (i == ETAS[1]))), idx_minus_one=_count(i == -1), idx_one=_count(i == 1), cos_one=_count(c == 1), cos_zero=_count(c == 0), cos_above_one=_count(c > 1),
                   nan=_count(np.isnan(x).any(1)), inf=_count(np.isinf(x).any(1)))


# ---- stream functions: six XORWOW words lead the record ----
def xorwow_step(st):
    """one step of XORWOW on a (n, 6) uint32 array [d, v0..v4] in place; returns the output word"""
    t = st[:, 1] ^ (st[:, 1] >> U(2))
    st[:, 1], st[:, 2], st[:, 3], st[:, 4] = st[:, 2].copy(), st[:, 3].copy(), st[:, 4].copy(), st[:, 5].copy()
    st[:, 5] = (st[:, 5] ^ (st[:, 5] << U(4))) ^ (t ^ (t << U(1)))
    st[:, 0] = st[:, 0] + U(362437)
    return st[:, 5] + st[:, 0]


def _states(rng, n):
    """(n, 6) uint32: the streams of a seeded 512 x 256 image (oracle.seed_states), states whose next output is the smallest / largest / a chosen
    word (so the next curand_uniform is 2^-33, 1.0, ...), and random states"""
    from tests import oracle_lib as O
    seeded = O.seed_states(69420, 512, 256)
    st = rng.integers(0, 1 << 32, (n, 6), dtype=np.uint64).astype(U)
    k = len(seeded)
    st[:k, 0] = seeded["d"]; st[:k, 1:6] = seeded["v"]
    m = 1 << 12
    want = np.concatenate([np.zeros(m, U), np.full(m, 0xffffffff, U), np.arange(m, dtype=U), U(0xffffffff) - np.arange(m, dtype=U), np.full(m, 0x80000000, U), np.full(m, 0x7fffffff, U)])
    c = st[k: k + len(want)].copy()
    out = xorwow_step(c)                      # what these states would give; move d so that they give `want`
    st[k: k + len(want), 0] += want - out
    check = st[k: k + len(want)].copy()
    assert (xorwow_step(check) == want).all()
    first = xorwow_step(st.copy())
    return st, dict(seeded=k, smallest_uniform=_count(first == 0), largest_uniform=_count(first == 0xffffffff), uniform_rounds_to_one=_count(first >= 0xffffff80), random_state=n - k - len(want))


def _stream(rng, n):
    st, c = _states(rng, n)
    return np.ascontiguousarray(st), c


def _sphere_stream(rng, n):
    from tests import math_restate as R
    st, c = _states(rng, n)
    _, _, draws = R.random_in_unit_sphere(st.copy())
    c.update(rejected_once=_count(draws > 3), rejected_twice=_count(draws > 6), accepted_first=_count(draws == 3))
    return np.ascontiguousarray(st), c


def _disk_stream(rng, n):
    from tests import math_restate as R
    st, c = _states(rng, n)
    _, _, draws = R.random_in_unit_disk(st.copy())
    c.update(rejected_once=_count(draws > 2), rejected_twice=_count(draws > 4), accepted_first=_count(draws == 2))
    return np.ascontiguousarray(st), c


def _float_range(rng, n):
    st, c = _states(rng, n)
    rngs = np.array([[-1, 1], [0, 1], [0.5, 1], [-0.5, 0.5], [0, 0], [1, -1], [-1e30, 1e30], [0, 1e-40], [3e38, -3e38], [165, 555], [0, np.inf], [np.nan, 1]], F)
    mm = rngs[np.arange(n) % len(rngs)]
    x = np.ascontiguousarray(np.concatenate([st, mm.view(U)], 1))
    c.update(unit=_count((mm[:, 0] == -1) & (mm[:, 1] == 1)), empty=_count(mm[:, 0] == mm[:, 1]), overflow=_count(mm[:, 0] == F(3e38)), denormal=_count(mm[:, 1] == F(1e-40)))
    return x, c


INT_RANGES = np.array([[0, 0], [0, 1], [-3, 3], [0, 255], [0, 1 << 24]], np.int32)


def _int_range(rng, n):
    st, c = _states(rng, n)
    mm = INT_RANGES[np.arange(n) % len(INT_RANGES)]
    x = np.ascontiguousarray(np.concatenate([st, mm.view(U)], 1))
    c.update({f"range{i}": _count((mm == r).all(1)) for i, r in enumerate(INT_RANGES)})
    return x, c


# ---- group C ----
def _sphere_uv(rng, n):
    f = F
    z = (f(0.0), f(-0.0))
    poles = np.array([[a, s, b] for s in (1, -1) for a in z for b in z], f)
    seam = np.array([[-x, y, b] for x in (1.0, 0.5, 1e-3, 1e-30, 1e-45) for y in (0.0, -0.0, 0.5, -0.8) for b in z], f)
    base = np.concatenate([poles, seam, np.array([[1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1], [1, -0.0, -0.0], [-1, -0.0, 0.0]], f)])
    # every component of those moved by one place either way
    steps = np.array(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1])).reshape(3, -1).T
    near = np.stack([around32(base[:, k], 1).reshape(len(base), 3)[:, steps[:, k] + 1] for k in range(3)], 2).reshape(-1, 3)
    m = 1 << 17
    unit = _unit64(rng, 4 * m)
    above = (unit[:m] * (1 + np.ldexp(1.0, rng.integers(-24, -18, (m, 1))))).astype(f)      # a hit on a small sphere: |p| a little over 1
    polar = unit[m: 2 * m].copy()
    polar[:, [0, 2]] *= np.ldexp(1.0, rng.integers(-60, -2, (m, 1)))                         # close to a pole
    polar[:, 1] = np.sign(polar[:, 1]) * np.sqrt(np.maximum(1 - polar[:, 0] ** 2 - polar[:, 2] ** 2, 0))
    seamy = unit[2 * m: 3 * m].copy()
    seamy[:, 0] = -np.abs(seamy[:, 0])
    seamy[:, 2] *= np.ldexp(1.0, rng.integers(-160, -2, m))                             # close to the seam, denormal z included
    axis = unit[3 * m:].copy()
    axis[np.arange(m), rng.integers(0, 3, m)] = np.where(rng.random(m) < 0.5, 0.0, -0.0)
    with np.errstate(all="ignore"):
        parts = [base, near, above, polar.astype(f), seamy.astype(f), axis.astype(f), np.array([[np.nan, 0, 1], [0, 2, 0], [0, -2, 0], [np.inf, 0, 0], [1, 0, np.inf], [-np.inf, 0, -np.inf]], f),
                 f32_families(rng, 3 << 12, -8, 4).reshape(-1, 3)]
    x = _finish(parts, n, lambda k: _unit64(rng, k), 3, f)
    return x, dict(pole=_count((np.abs(x[:, 1]) == 1) & (x[:, 0] == 0) & (x[:, 2] == 0)), seam_plus_zero=_count((x[:, 0] < 0) & (x[:, 2] == 0) & ~np.signbit(x[:, 2])),
                   seam_minus_zero=_count((x[:, 0] < 0) & (x[:, 2] == 0) & np.signbit(x[:, 2])), y_outside=_count(np.abs(x[:, 1]) > 1), y_just_outside=_count((np.abs(x[:, 1]) > 1) & (np.abs(x[:, 1]) < f(1.00001))),
                   y_just_inside=_count((np.abs(x[:, 1]) < 1) & (np.abs(x[:, 1]) > f(0.99999))), x_zero=_count(x[:, 0] == 0), z_denormal=_count((x[:, 2] != 0) & (np.abs(x[:, 2]) < f(1.17549435e-38))),
                   nan=_count(np.isnan(x).any(1)), **{f"quadrant{int(a)}{int(b)}": _count((np.signbit(x[:, 0]) == a) & (np.signbit(x[:, 2]) == b)) for a in (0, 1) for b in (0, 1)})


IMAGE_SHAPES = ((1, 1), (3, 2), (257, 129))  # width, height


def image_tables(seed=4107):
    """the synthetic images: (list of (height, width, 3) uint8 arrays, DImage records as (offset, width, height, 0) rows, the texels end to end)"""
    rng = np.random.default_rng(seed)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in IMAGE_SHAPES]
    recs, off = [], 0
    for im in imgs:
        recs.append((off, im.shape[1], im.shape[0], 0))
        off += im.size
    return imgs, recs, np.concatenate([im.ravel() for im in imgs])


def _coords(size):
    f = F
    k = (np.arange(size + 1).astype(f) / f(size)).astype(f)
    base = np.concatenate([around32(np.array([0.0, -0.0, 1.0], f), 1), k, np.nextafter(k, f(-np.inf)), np.nextafter(k, f(np.inf)), np.array([-0.0, 2, -1, np.nan, np.inf, -np.inf, 0.5, 1e-45, 3e38], f)])
    return base


def _image_value(rng, n):
    parts = []
    for idx, (w, h) in enumerate(IMAGE_SHAPES):
        u, v = _pairs(_coords(w), _coords(h))
        parts.append(np.stack([np.full(len(u), idx, U), u.view(U), v.view(U)], 1))

    def fill(k):
        uv = np.where(rng.random((k, 2)) < 0.9, rng.random((k, 2)) * 1.2 - 0.1, f32_families(rng, 2 * k, -30, 3).reshape(-1, 2)).astype(F)
        return np.concatenate([rng.integers(0, len(IMAGE_SHAPES), (k, 1)).astype(U), uv.view(U)], 1)
    x = _finish(parts, n, fill, 3, U)
    u, v = x[:, 1].view(F), x[:, 2].view(F)
    c = dict(u_below=_count(u < 0), u_above=_count(u > 1), v_below=_count(v < 0), v_above=_count(v > 1), u_one=_count(u == 1), v_zero=_count(v == 0), negative_zero=_count((u == 0) & np.signbit(u)), nan=_count(np.isnan(u) | np.isnan(v)),
             inside=_count((u > 0) & (u < 1) & (v > 0) & (v < 1)))
    c.update({f"image{i}": _count(x[:, 0] == i) for i in range(len(IMAGE_SHAPES))})
    return np.ascontiguousarray(x), c


NOISE_SCENE = 4          # two_perlin_spheres: one mort_noise_texture, scale 4
NOISE_SCALE = 4.0


def _phase_brackets(rng, m):
    """2 m points in m pairs that differ by one step of z and whose colours 0.5 * (1 + sin(s.z + 10 * turb)) lie on either side of 0.5: the
    sine changes sign between the two, so mort_sin's argument sits within one step of a multiple of pi (its even multiples of pi/2; at the
    odd ones the colour is at a flat extremum and brackets nothing).  Found by bisection on z with the oracle's texture dispatch -- the
    oracle chooses inputs here, it is not what the device is compared with on them alone."""
    from mort_amd import structs as S
    from tests import oracle_lib as O
    world, _ = noise_world()
    above = lambda p: O.texture_value_batch(world, S.TEXTURE_NOISE, 0, 0, 0, p)[:, 0] > F(0.5)
    p = rng.uniform(-8, 8, (16 * m, 3)).astype(F)
    q = p.copy()
    q[:, 2] += F(0.25)
    a = above(p)
    keep = np.flatnonzero(a != above(q))[:m]
    assert len(keep) == m
    p, a = p[keep], a[keep]
    lo, hi = p[:, 2].copy(), q[keep, 2].copy()
    for _ in range(64):
        mid = ((lo.astype(D) + hi.astype(D)) / 2).astype(F)
        live = (mid != lo) & (mid != hi)
        if not live.any():
            break
        pm = p.copy()
        pm[:, 2] = mid
        same = above(pm) == a
        lo, hi = np.where(live & same, mid, lo), np.where(live & ~same, mid, hi)
    assert (np.nextafter(lo, F(np.inf)) == hi).all()
    left, right = p.copy(), p.copy()
    left[:, 2], right[:, 2] = lo, hi
    return np.stack([left, right], 1).reshape(-1, 3)


def _noise_value(rng, n):
    """Every |scale * p * 64| stays below 2^31 (perlin_noise doubles the point six times): past that the lattice index saturates and the host's
    i + 1 is a signed overflow with nothing defined to compare.  With scale 4 that allows |p| < 2^23; the builder stops at 1e6."""
    f = F
    m = n // 8
    lat = rng.integers(-64, 65, (m, 3)).astype(f) / f(NOISE_SCALE)                           # scale * p on the integer lattice
    below = np.nextafter(lat, f(-np.inf))
    zero = np.where(rng.random((m, 3)) < 0.5, f(0.0), f(-0.0))
    zero[rng.random((m, 3)) < 0.5] = f(0.37)
    scene = _unit64(rng, m).astype(f) * f(2) + np.array([0, 2, 0], f)                         # on the scene's own sphere
    ground = np.stack([rng.uniform(-30, 30, m), np.zeros(m), rng.uniform(-30, 30, m)], 1).astype(f)
    far = (_unit64(rng, m) * 10.0 ** rng.uniform(1, 6, (m, 1))).astype(f)
    tiny = f32_families(rng, 3 * m, -149 + 23, -20).reshape(-1, 3)
    brackets = _phase_brackets(rng, 2048)
    pts = _finish([brackets, lat, below, zero, scene, ground, far, tiny], n, lambda k: rng.uniform(-8, 8, (k, 3)), 3, f)
    assert np.abs(pts.astype(D) * NOISE_SCALE * 64).max() < 2.0 ** 31
    x = np.ascontiguousarray(np.concatenate([np.zeros((n, 1), U), pts.view(U)], 1))
    s = pts * f(NOISE_SCALE)
    return x, dict(phase_brackets_multiple_of_pi=len(brackets) // 2, lattice=_count((s == np.floor(s)).all(1)), just_below_lattice=_count((np.nextafter(s, f(np.inf)) == np.ceil(s)).any(1) & (s != np.floor(s)).any(1)), negative=_count((pts < 0).any(1)),
                   negative_zero=_count(((pts == 0) & np.signbit(pts)).any(1)), far=_count(np.abs(pts).max(1) > 1e5), tiny=_count(np.abs(pts).max(1) < 1e-6))


_BUILDERS = {
    "sqrtf": _sqrtf, "sqrt": _sqrt, "floorf": _floorf, "fmaxf": _minmax32, "fmin": _minmax64, "d2i": _d2i, "powi5f": _powi5f, "sin": _trig64, "cos": _trig64, "sinf": _trig32, "cosf": _trig32,
    "sincosf": _trig32, "atan": _atan, "atan2f": _atan2f, "acosf": _acosf, "logf": _logf, "divf": _divf, "rcpf": _rcpf, "div": _div, "d2f": _d2f, "u2f": _u2f, "truncf": _floorf,
    "vlen": _vlen, "vdiv": _vdiv, "vunit": _vunit, "vcross": _two_vectors, "reflect": _two_vectors, "refract": _refract, "reflectance": _reflectance, "onb": _onb,
    "random_float_range": _float_range, "random_int": _int_range, "random_in_unit_sphere": _sphere_stream, "random_unit_vector": _sphere_stream, "random_in_unit_disk": _disk_stream,
    "random_cosine_direction": _stream, "sphere_uv": _sphere_uv, "noise_value": _noise_value, "image_value": _image_value,
}


def noise_world():
    """(the built-in scene with a Perlin texture, the bytes of its mort_noise_texture records)"""
    import ctypes as C
    from mort_amd import host, structs as S
    w, _ = host.build_scene(NOISE_SCENE, width=16, spp=1)
    count = w.c.texs.num_noise_textures
    assert count == 1 and w.c.texs.host_noise_texture[0].scale == NOISE_SCALE
    raw = np.ctypeslib.as_array(C.cast(w.c.texs.host_noise_texture, C.POINTER(C.c_ubyte)), shape=(count * C.sizeof(S.NoiseTexture),)).copy()
    return w, raw


def image_world():
    """(a world holding the synthetic images as image textures 0, 1, 2, their DImage records, the texels end to end)"""
    from mort_amd import hip, host
    imgs, recs, texels = image_tables()
    w = host.World()
    for k, im in enumerate(imgs):
        w._keepalive.append(im)
        assert host.lib().mort_add_image_texture(w.ptr, im.ctypes.data, im.shape[1], im.shape[0]) == k
    return w, np.array(recs, dtype=hip.DIMAGE_DTYPE), texels


def tables_for(fn, noise_raw, image_recs, texels):
    """the keyword arguments hip.debug_math_host / debug_math_device need for function fn"""
    if NAMES[fn] == "noise_value":
        return dict(noise=noise_raw)
    if NAMES[fn] == "image_value":
        return dict(images=image_recs, texels=texels)
    return {}


def size_of(fn):
    return N_NOISE if NAMES[fn] == "noise_value" else (N_AP if fn < GROUP_B[0] else N_BC)


def build(fn, n=None):
    """(records (n, k), census) of function number fn; n defaults to the function's full size"""
    n = size_of(fn) if n is None else n
    rng = np.random.default_rng(9000 + fn)
    rec, census, _ = _build(fn, n)
    return rec, census


def _build(fn, n=None):
    """(records, census, edge rows): the builders of the functions that tests/test_math.py measures against mpmath lead with their small
    edge families and say how many rows those are (0 for the others)"""
    n = size_of(fn) if n is None else n
    rng = np.random.default_rng(9000 + fn)
    with np.errstate(all="ignore"):
        res = _BUILDERS[NAMES[fn]](rng, n)
    rec, census = res[0], res[-1]
    edge = res[1] if len(res) == 3 else (0, 0)
    assert len(rec) == n and rec.flags.c_contiguous
    return rec, census, edge


def ragged(fn):
    """RAGGED records of function fn, a seeded choice among its full builder's"""
    rec, _ = build(fn)
    pick = np.random.default_rng(77 + fn).choice(len(rec), RAGGED, replace=False)
    return np.ascontiguousarray(rec[np.sort(pick)])


def canon(out_words, kinds):
    """(n, out_words) uint32 results -> the same with every NaN replaced by one pattern (tests/query_rays.py _words: a generated NaN's sign and
    payload are the compiler's and the machine's choice; every other value is compared bit for bit).  kinds: per output column 'f' (float32),
    'd' (low and high word of a float64: two columns) or 'i' (integer word, compared as it is)."""
    w = np.array(out_words, dtype=U, copy=True)
    k = 0
    for kind in kinds:
        if kind == "f":
            nan = np.isnan(w[:, k].view(F))
            w[nan, k] = 0x7fc00000
            k += 1
        elif kind == "d":
            v = (w[:, k].astype(np.uint64) | (w[:, k + 1].astype(np.uint64) << np.uint64(32))).view(D)
            nan = np.isnan(v)
            w[nan, k] = 0
            w[nan, k + 1] = 0x7ff80000
            k += 2
        else:
            k += 1
    assert k == w.shape[1]
    return w


def assert_same(fn, rec, results):
    """results: {label: (n, out_words) uint32 words} of function fn over rec -- all equal bit for bit (canon's NaN rule, signed zeros count);
    the failure names the first differing input as hex words with every result"""
    kinds = OUT_KINDS[NAMES[fn]]
    labels = list(results)
    can = [canon(np.asarray(results[k]).reshape(len(rec), -1), kinds) for k in labels]
    bad = np.zeros(len(rec), bool)
    for c in can[1:]:
        bad |= (c != can[0]).any(1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        hexes = lambda w: " ".join(f"{int(v):08x}" for v in np.ascontiguousarray(w).reshape(-1).view(U))
        raise AssertionError(f"{NAMES[fn]}: {int(bad.sum())} of {len(rec)} records differ; first at record {i}: input {hexes(rec[i])} ({rec[i].tolist()}); " +
                             "; ".join(f"{k} {hexes(np.asarray(results[k]).reshape(len(rec), -1)[i])}" for k in labels))


def assert_census(fn, census):
    missing = [k for k, v in census.items() if v <= 0]
    assert not missing, f"{NAMES[fn]}: input families missing from the builder: {missing} ({census})"


def subsample(fn, most=1 << 16):
    """the fixed sample of function fn's builder that is measured against mpmath: every edge family whole (specials, the lowest and highest
    denormals, the neighbours of +-1, of +-1e5, of the break points and of 1.0, the quadrant ties, the sign x magnitude pairs, the extreme
    exponent differences, one pass over every exponent), then a stride over the large families (the values next to k * pi/2, dense ranges,
    equal magnitudes, break-point ratios at every scale) up to `most` records.  Returns (records, how many of them are edge rows)."""
    rec, _, (edge, big) = _build(fn)
    assert 0 < edge < most and big > 0, (NAMES[fn], edge, big)
    step = -(-big // (most - edge))
    return np.concatenate([rec[:edge], rec[edge: edge + big: step]]), edge


# what each function's output columns hold (canon)
OUT_KINDS = {"sqrtf": "f", "sqrt": "d", "floorf": "f", "fmaxf": "f", "fmin": "d", "d2i": "i", "powi5f": "f", "sin": "d", "cos": "d", "sinf": "f", "cosf": "f", "sincosf": "ff", "atan": "d",
             "atan2f": "f", "acosf": "f", "logf": "f", "divf": "f", "rcpf": "f", "div": "d", "d2f": "f", "u2f": "f", "truncf": "f", "vlen": "f", "vdiv": "fff", "vunit": "fff", "vcross": "fff",
             "reflect": "fff", "refract": "fff", "reflectance": "f", "onb": "f" * 12, "random_float_range": "f" + "i" * 7, "random_int": "i" * 8, "random_in_unit_sphere": "fff" + "i" * 7,
             "random_unit_vector": "fff" + "i" * 7, "random_in_unit_disk": "fff" + "i" * 7, "random_cosine_direction": "fff" + "i" * 7, "sphere_uv": "ff", "noise_value": "fff", "image_value": "fff"}
