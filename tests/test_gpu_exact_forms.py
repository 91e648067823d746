"""The short forms of the BVH leaf step ON THE DEVICE, against the device's own plain operators, bit for bit, 0 mismatches
(mort_hip_debug_exact_forms_device: one launch per part, the kernel returns the count and the first failing elements).

 (a) dev_math.h div_by against / and sqrt_ord against sqrtf, 2^24 inputs each: random, all-ones, zero and near-power mantissas over the
     whole guarded range, the family the algebra alone does not settle (a denominator with an all-ones mantissa under a power-of-two
     numerator, every exponent pair inside the guards, both signs), the guards' boundary values and their neighbours outside
     (which must be refused), and numerators below 2^-85 (zeros and denormals included), whose quotients only have to end below
     2^-44 in both forms.
 (b) mega_bvh.h sphere_hit_root_fast against sphere_hit_root on 2^22 (ray, sphere, t_max) records: moving and static spheres,
     zero and negative-zero coordinates, rays that start on and inside the sphere, t_max = +infinity, and scales from 2^-40 to
     2^40 with direction lengths from 2^-22 to 2^22, so that both the short and the generic branch are taken and both accept
     roots (asserted)."""
import ctypes as C

import numpy as np
import pytest

from mort_amd import hip

pytestmark = pytest.mark.gpu

N_A = 1 << 24
N_B = 1 << 22


def _device(what, arr, n):
    fn = hip.lib().mort_hip_debug_exact_forms_device
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_ulonglong)]
    arr = np.ascontiguousarray(arr, np.float32)
    out = (C.c_ulonglong * 16)()
    assert fn(0, what, arr.ctypes.data_as(C.c_void_p), n, out) == 0
    out = list(out)
    return out, out[8:8 + min(out[1], 8)]


def _pow2(e):
    return np.ldexp(np.float32(1.0), np.asarray(e)).astype(np.float32)


def _values(rng, n, e_lo, e_hi):
    """n positive float32 in [2^e_lo, 2^e_hi): a quarter each with random, all-ones, zero and near-power mantissas."""
    e = rng.integers(e_lo, e_hi, n)
    kind = np.arange(n) % 4
    mant = rng.integers(0, 1 << 23, n, dtype=np.uint32)
    near = rng.integers(0, 4, n, dtype=np.uint32)
    near = np.where(rng.random(n) < 0.5, near, np.uint32((1 << 23) - 1) - near)
    mant = np.select([kind == 0, kind == 1, kind == 2], [mant, np.uint32((1 << 23) - 1), np.uint32(0)], near).astype(np.uint32)
    return (((e + 127).astype(np.uint32) << np.uint32(23)) | mant).view(np.float32)


def _edges(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(np.inf))]


def test_division_by_a_prepared_denominator():
    rng = np.random.default_rng(7301)
    f = np.float32
    # all-ones denominators x power-of-two numerators, every exponent pair inside the guards, both signs
    ea, ex = np.meshgrid(np.arange(-40, 40), np.arange(-85, 56))
    ones = (((ea.ravel() + 127).astype(np.uint32) << np.uint32(23)) | np.uint32((1 << 23) - 1)).view(np.float32)
    pw = _pow2(ex.ravel())
    fam_a, fam_x = np.concatenate([ones, ones]), np.concatenate([pw, -pw])
    # boundaries: every edge value of the denominator against every edge value of the numerator, neighbours outside included
    ba = np.array(_edges(_pow2(-40)[()]) + _edges(_pow2(40)[()]) + [f(0), f(-0.0), f(1e-45), f(np.inf), f(np.nan), f(-1)], f)
    bx = np.array(_edges(_pow2(-85)[()]) + _edges(_pow2(56)[()]) + [f(0), f(-0.0), f(1e-45), f(-1e-45), _pow2(-126)[()], f(np.inf), f(np.nan)], f)
    bx = np.concatenate([bx, -bx])
    gx, ga = np.meshgrid(bx, ba)
    # small numerators under every kind of denominator
    ns = 1 << 16
    small_x = _values(rng, ns, -126, -85) * np.where(rng.random(ns) < 0.5, f(-1), f(1))
    small_a = _values(rng, ns, -40, 40)
    n_rand = N_A - len(fam_a) - gx.size - ns
    a = np.concatenate([_values(rng, n_rand, -40, 40), fam_a, ga.ravel(), small_a])
    x = np.concatenate([_values(rng, n_rand, -85, 56)[rng.permutation(n_rand)] * np.where(rng.random(n_rand) < 0.5, f(-1), f(1)), fam_x, gx.ravel(), small_x])
    assert len(a) == len(x) == N_A
    out, first = _device(1, np.stack([x, a], axis=1), N_A)
    compared, fail, outside, small = out[0], out[1], out[2], out[3]
    print(f"div_by against /: {compared} compared bit for bit, {small} small numerators, {outside} refused by the guards, {fail} fail, first {first}")
    assert fail == 0, [(float(x[i]), float(a[i])) for i in first]
    assert compared + small + outside == N_A
    assert compared >= n_rand + len(fam_a) and small >= ns and outside > 0


def test_square_root():
    rng = np.random.default_rng(7302)
    f = np.float32
    k = rng.integers(1, 4096, 1 << 18).astype(np.float32) * _pow2(rng.integers(-40, 37, 1 << 18))
    sq = k * k
    edge = np.array(_edges(_pow2(-96)[()]) + _edges(_pow2(100)[()]) + [f(0), f(-0.0), f(1e-45), f(np.inf), f(np.nan), f(-1), f(1), f(2), f(4)], f)
    n_rand = N_A - 3 * len(sq) - len(edge)
    x = np.concatenate([_values(rng, n_rand, -96, 100), sq, np.nextafter(sq, f(0)), np.nextafter(sq, f(np.inf)), edge])
    assert len(x) == N_A
    out, first = _device(0, x, N_A)
    compared, fail, outside = out[0], out[1], out[2]
    print(f"sqrt_ord against sqrtf: {compared} compared bit for bit, {outside} refused by the guard, {fail} fail, first {first}")
    assert fail == 0, [float(x[i]) for i in first]
    assert compared + outside == N_A and outside == 9 and compared >= N_A - len(edge)


def _records(rng, n):
    """n x 16 float32: ray origin, direction, time, t_max; sphere centre, radius, velocity, moves."""
    f = np.float32
    uni = lambda lo, hi, shape: rng.random(shape, dtype=f) * f(hi - lo) + f(lo)
    scale = _pow2(rng.integers(-40, 41, n))[:, None]                           # the scene's length scale
    dlen = _pow2(rng.integers(-22, 23, n))[:, None]                            # the direction's length: a = |d|^2 from 2^-44 to 2^44
    rec = np.empty((n, 16), f)
    centre = uni(-4, 4, (n, 3)) * scale
    radius = uni(0.05, 2.0, (n, 1)) * scale
    moves = rng.random(n, dtype=f) < 0.5
    vel = np.where(moves[:, None], uni(-1, 1, (n, 3)) * scale, f(0))
    tm = rng.random((n, 1), dtype=f)
    now = centre + tm * vel                                                    # about where the sphere is at the ray's time
    u = uni(-1, 1, (n, 3)); u /= np.sqrt((u * u).sum(axis=1, keepdims=True)) + f(1e-30)
    where = rng.integers(0, 5, n)[:, None]
    # outside; on the sphere (up to rounding); inside; at the centre; within rounding of the surface
    factor = np.select([where == 0, where == 1, where == 2, where == 3],
                       [uni(1.5, 20, (n, 1)), f(1), rng.random((n, 1), dtype=f), f(0)], f(1) + uni(-1e-6, 1e-6, (n, 1)))
    origin = now + u * (radius * factor)
    aim = now + uni(-1, 1, (n, 3)) * radius * rng.choice(np.array([0.3, 1.0, 1.5], f), (n, 1)) - origin
    far = np.sqrt((aim * aim).sum(axis=1, keepdims=True))
    d = np.where(far > 0, aim / np.where(far > 0, far, f(1)), u) * dlen
    # zero and negative-zero coordinates: a tenth of the records get some of their nine coordinates replaced
    for arr in (origin, d, centre):
        z = (rng.random((n, 3), dtype=f) < 0.3) & (rng.random((n, 1), dtype=f) < 0.1)
        arr[z] = np.where(rng.random((n, 3), dtype=f) < 0.5, f(0.0), f(-0.0))[z]
    gap = now - origin
    dist = np.sqrt((gap * gap).sum(axis=1, keepdims=True)) / dlen
    t_max = np.where(rng.random((n, 1), dtype=f) < 0.5, f(np.inf), (dist + f(1e-3)) * uni(0.3, 3.0, (n, 1)))
    rec[:, 0:3] = origin; rec[:, 3:6] = d; rec[:, 6:7] = tm; rec[:, 7:8] = t_max
    rec[:, 8:11] = centre; rec[:, 11:12] = radius; rec[:, 12:15] = vel; rec[:, 15] = moves
    return rec


def test_leaf_step_sphere_test_against_the_generic_one():
    rec = _records(np.random.default_rng(7303), N_B)
    out, first = _device(2, rec, N_B)
    compared, fail, short, generic, short_hits, generic_hits = out[0], out[1], out[4], out[5], out[6], out[7]
    print(f"sphere_hit_root_fast against sphere_hit_root: {compared} records, short branch {short} ({short_hits} accepted roots), "
          f"generic branch past its miss test {generic} ({generic_hits} accepted roots), {fail} fail, first {first}")
    assert fail == 0, [rec[i].tolist() for i in first]
    assert compared == N_B
    assert short > 0 and generic > 0 and short_hits > 0 and generic_hits > 0
