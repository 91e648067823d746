"""dev_math.h's shading primitives and dev_trace.h's sphere_uv restated in numpy from the reference's formulas (vec3.cuh:99-112,143-212,
onb.cuh:41-51, rng.cuh:17-42, objects.cuh:101-108): float32 and float64 arrays, one IEEE operation per numpy operation, in the reference's
order.  Transcendentals come from the oracle's mort_oracle_math_batch (gcc's compile of mort_math.h); XORWOW is restated on uint32 arrays
(tests/math_cases.py xorwow_step).  tests/test_math.py compares hipcc's host compile of the headers with these, tolerance 0."""
import numpy as np

from tests import oracle_lib as O
from tests.math_cases import FN, xorwow_step

F, D, U = np.float32, np.float64, np.uint32
ONE, TWO = F(1), F(2)


def _col(t):
    return np.asarray(t, F)[:, None]


def vdot(u, v):
    return u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1] + u[:, 2] * v[:, 2]


def vlen2(a):
    return a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2]


def vlen(a):
    return np.sqrt(vlen2(a))


def vscale(t, v):
    return _col(t) * v


def vdiv(v, t):  # vec3.cuh:109-112: (1 / t) * v
    return vscale(ONE / np.asarray(t, F), v)


def vunit(a):
    return vdiv(a, vlen(a))


def vcross(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)


def reflect(v, n):  # vec3.cuh:192-194
    return v - vscale(TWO * vdot(v, n), n)


def refract(uv, n, eta):  # vec3.cuh:197-203
    cos_theta = np.fmin(vdot(-uv, n).astype(D), 1.0)
    perp = vscale(eta, uv + vscale(cos_theta.astype(F), n))
    par = vscale((-np.sqrt(np.abs(1.0 - vlen2(perp).astype(D)))).astype(F), n)
    return perp + par


def reflectance(cosine, ref_idx):  # vec3.cuh:206-212; pow(float, 5) by squaring
    r0 = (ONE - ref_idx) / (ONE + ref_idx)
    r0 = r0 * r0
    a = ONE - cosine
    a2 = a * a
    a4 = a2 * a2
    return r0 + (ONE - r0) * (a * a4)


def onb(w, a):  # onb.cuh:41-51, then local()
    uw = vunit(w)
    pick = (np.abs(uw[:, 0]).astype(D) > 0.9)[:, None]
    axis = np.where(pick, np.array([0, 1, 0], F), np.array([1, 0, 0], F)).astype(F)
    v = vunit(vcross(uw, axis))
    u = vcross(uw, v)
    local = (vscale(a[:, 0], u) + vscale(a[:, 1], v)) + vscale(a[:, 2], uw)
    return np.concatenate([u, v, uw, local], 1)


# ---- streams: st is a (n, 6) uint32 array [d, v0..v4], advanced in place ----
def curand_uniform(st):
    return xorwow_step(st).astype(F) * F(2.3283064e-10) + F(2.3283064e-10) / F(2.0)


def random_float(st):  # rng.cuh:17-23: (float)(1.0 - (double)u)
    return (1.0 - curand_uniform(st).astype(D)).astype(F)


def random_float_range(st, mn, mx):
    return random_float(st) * (mx - mn) + mn


def random_int(st, mn, mx):  # rng.cuh:31-42
    r = curand_uniform(st)
    r = (r.astype(D) * ((mx - mn).astype(D) + 0.999999)).astype(F)
    r = r + mn.astype(F)
    return np.trunc(r).astype(np.int64).astype(np.int32)


def _rejection(st, dims, accept):
    n = len(st)
    out = np.zeros((n, 3), F)
    draws = np.zeros(n, U)
    active = np.arange(n)
    lo, hi = F(-1), F(1)
    while len(active):
        s = st[active]
        p = np.zeros((len(active), 3), F)
        for k in range(dims):
            p[:, k] = random_float_range(s, lo, hi)
        st[active] = s
        draws[active] += U(dims)
        ok = accept(vlen2(p))
        out[active[ok]] = p[ok]
        active = active[~ok]
    return out, st, draws


def random_in_unit_sphere(st):  # vec3.cuh:143-155: again while |p|^2 >= 1
    return _rejection(st, 3, lambda l2: ~(l2 >= 1))


def random_in_unit_disk(st):  # vec3.cuh:162-169: until |p|^2 < 1
    return _rejection(st, 2, lambda l2: l2 < 1)


def random_unit_vector(st):
    p, st, draws = random_in_unit_sphere(st)
    return vunit(p), st, draws


def random_cosine_direction(st):  # vec3.cuh:180-189
    r1 = random_float(st)
    r2 = random_float(st)
    phi = (2 * 3.1415926 * r1.astype(D)).astype(F)
    sq = np.sqrt(r2)
    sc = O.math_batch(FN["sincosf"], phi).view(F)
    x = sc[:, 1] * sq
    y = sc[:, 0] * sq
    z = np.sqrt(ONE - r2)
    return np.stack([x, y, z], 1), st, np.full(len(st), 2, U)


def sphere_uv(p):  # objects.cuh:101-108
    theta = O.math_batch(FN["acosf"], np.ascontiguousarray(-p[:, 1])).view(F)[:, 0]
    at = O.math_batch(FN["atan2f"], np.ascontiguousarray(np.stack([-p[:, 2], p[:, 0]], 1))).view(F)[:, 0]
    phi = (at.astype(D) + 3.141592565).astype(F)
    u = (phi.astype(D) / (2.0 * 3.141592565)).astype(F)
    v = (theta.astype(D) / 3.141592565).astype(F)
    return np.stack([u, v], 1)


def _stream_result(value, st, draws):
    value = np.asarray(value)
    value = value.reshape(len(st), -1)
    return np.concatenate([value.view(U), st, draws[:, None].astype(U)], 1)


def evaluate(fn, rec):
    """function number fn (group B, or sphere_uv) over its builder's records -> (n, out_words) uint32 words"""
    name = [k for k, v in FN.items() if v == fn][0]
    with np.errstate(all="ignore"):
        if name == "vlen": return vlen(rec).view(U)[:, None]
        if name == "vdiv": return vdiv(rec[:, 0:3], rec[:, 3]).view(U)
        if name == "vunit": return vunit(rec).view(U)
        if name == "vcross": return vcross(rec[:, 0:3], rec[:, 3:6]).view(U)
        if name == "reflect": return reflect(rec[:, 0:3], rec[:, 3:6]).view(U)
        if name == "refract": return refract(rec[:, 0:3], rec[:, 3:6], rec[:, 6]).view(U)
        if name == "reflectance": return reflectance(rec[:, 0], rec[:, 1]).view(U)[:, None]
        if name == "onb": return onb(rec[:, 0:3], rec[:, 3:6]).view(U)
        if name == "sphere_uv": return sphere_uv(rec).view(U)
        st = np.array(rec[:, 0:6], dtype=U, copy=True)
        if name == "random_float_range":
            v = random_float_range(st, rec[:, 6].view(F), rec[:, 7].view(F))
            return _stream_result(v, st, np.ones(len(st), U))
        if name == "random_int":
            v = random_int(st, rec[:, 6].view(np.int32), rec[:, 7].view(np.int32))
            return _stream_result(v.view(U), st, np.ones(len(st), U))
        f = dict(random_in_unit_sphere=random_in_unit_sphere, random_unit_vector=random_unit_vector, random_in_unit_disk=random_in_unit_disk,
                 random_cosine_direction=random_cosine_direction)[name]
        return _stream_result(*f(st))
