/*
 * dev_math.h -- device-side vec3 / ray / XORWOW primitives for the gfx950
 * kernels.  Same operator semantics as the reference's vec3.cuh / ray.cuh /
 * rng.cuh (division = multiply by the fp32 reciprocal, dot sums left to
 * right, random_float = (float)(1.0 - curand_uniform)); compiled with
 * -ffp-contract=off so that nothing is fused (DESIGN.md "Numerical contract").
 */
#ifndef MORT_DEV_MATH_H
#define MORT_DEV_MATH_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mort_math.h"

#pragma clang fp contract(off)

#define DEV __host__ __device__ __forceinline__ /* the host loop (host_render.hip) runs the same bodies */

struct V3 { float x, y, z; };
DEV V3 mk(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
DEV V3 vadd(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
DEV V3 vsub(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
DEV V3 vmul(V3 a, V3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
DEV V3 vneg(V3 a) { return mk(-a.x, -a.y, -a.z); }
DEV V3 vscale(float t, V3 v) { return mk(t * v.x, t * v.y, t * v.z); } /* vec3.cuh:99-101 */
DEV V3 vdiv(V3 v, float t) { return vscale(1 / t, v); }                /* vec3.cuh:109-112 */
DEV float vdot(V3 u, V3 v) { return u.x * v.x + u.y * v.y + u.z * v.z; }
DEV float vlen2(V3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
DEV float vlen(V3 a) { return mort_sqrtf(vlen2(a)); }
DEV V3 vunit(V3 a) { return vdiv(a, vlen(a)); }
DEV V3 vcross(V3 u, V3 v) { return mk(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x); }

struct Ray { V3 o, d; float tm; };
DEV V3 ray_at(const Ray &r, float t) { return vadd(r.o, vscale(t, r.d)); } /* ray.cuh:17-19 (t narrowed to fp32) */

/* ---- XORWOW in registers: the reference reloads and stores the 48-byte
 * state around every draw (rng.cuh:18-22); here a pixel's d, v[5] live in six
 * VGPRs from its first sample to its last. ---- */
struct Rng { uint32_t d, v0, v1, v2, v3, v4; uint32_t draws; };

DEV uint32_t xorwow_next(Rng &s) {
    uint32_t t = s.v0 ^ (s.v0 >> 2);
    s.v0 = s.v1; s.v1 = s.v2; s.v2 = s.v3; s.v3 = s.v4;
    s.v4 = (s.v4 ^ (s.v4 << 4)) ^ (t ^ (t << 1));
    s.d += 362437u;
    return s.v4 + s.d;
}
/* curand_uniform: x * 2^-32 + 2^-33 (the product is exact) */
DEV float curand_uniform_of(uint32_t x) { return (float)x * 2.3283064e-10f + (2.3283064e-10f / 2.0f); }
DEV float curand_uniform_f(Rng &s) {
    s.draws++;
    return curand_uniform_of(xorwow_next(s));
}
/* rng.cuh:17-23 computes (float)(1.0 - (double)u).  u >= 2^-33 has 24 significant bits, so 1 - u is exact in fp64
 * unless u < 2^-29 (where both roundings give 1.0f); the fp32 subtraction rounds the same exact value once.
 * Checked for all 2^32 generator outputs, on the host (tests/test_rng.py) and on the device (tests/test_gpu_math.py,
 * random_float_all_kernel in debug.hip, which calls curand_uniform_of and random_float_of). */
DEV float random_float_of(float u) { return 1.0f - u; }
DEV float random_float(Rng &s) { return random_float_of(curand_uniform_f(s)); }
DEV float random_float_range(Rng &s, float mn, float mx) { float b = random_float(s); return b * (mx - mn) + mn; }
DEV int random_int(Rng &s, int mn, int mx) { /* rng.cuh:31-42 */
    float random = curand_uniform_f(s);
    random = (float)((double)random * (mx - mn + 0.999999));
    random += (float)mn;
    return mort_f2i(__builtin_truncf(random));
}

DEV V3 random_in_unit_sphere(Rng &s) { /* vec3.cuh:143-155 */
    for (;;) {
        float a = random_float_range(s, -1, 1);
        float b = random_float_range(s, -1, 1);
        float c = random_float_range(s, -1, 1);
        V3 p = mk(a, b, c);
        if (vlen2(p) >= 1) continue;
        return p;
    }
}
DEV V3 random_unit_vector(Rng &s) { return vunit(random_in_unit_sphere(s)); }
DEV V3 random_in_unit_disk(Rng &s) { /* vec3.cuh:162-169 */
    for (;;) {
        float a = random_float_range(s, -1, 1);
        float b = random_float_range(s, -1, 1);
        V3 p = mk(a, b, 0);
        if (vlen2(p) < 1) return p;
    }
}
DEV V3 random_cosine_direction(Rng &s) { /* vec3.cuh:180-189 */
    float r1 = random_float(s);
    float r2 = random_float(s);
    float phi = (float)(2 * 3.1415926 * (double)r1);
    float sq = mort_sqrtf(r2);
    float sn, cs;
    mort_sincosf(phi, &sn, &cs); /* == mort_sinf(phi), mort_cosf(phi) */
    float x = cs * sq;
    float y = sn * sq;
    float z = mort_sqrtf(1 - r2);
    return mk(x, y, z);
}
DEV V3 reflect(V3 v, V3 n) { return vsub(v, vscale(2 * vdot(v, n), n)); } /* vec3.cuh:192-194 */
DEV V3 refract(V3 uv, V3 n, float etai_over_etat) { /* vec3.cuh:197-203 */
    double cos_theta = mort_fmin((double)vdot(vneg(uv), n), 1.0);
    V3 r_out_perp = vscale(etai_over_etat, vadd(uv, vscale((float)cos_theta, n)));
    V3 r_out_parallel = vscale((float)(-mort_sqrt(mort_fabs(1.0 - (double)vlen2(r_out_perp)))), n);
    return vadd(r_out_perp, r_out_parallel);
}
DEV float reflectance(float cosine, float ref_idx) { /* vec3.cuh:206-212 */
    float r0 = (1 - ref_idx) / (1 + ref_idx);
    r0 = r0 * r0;
    return r0 + (1 - r0) * mort_powi5f(1 - cosine);
}

struct Onb { V3 u, v, w; };
DEV Onb onb_from_w(V3 w) { /* onb.cuh:41-51 */
    Onb o;
    V3 unit_w = vunit(w);
    V3 a = ((double)mort_fabsf(unit_w.x) > 0.9) ? mk(0, 1, 0) : mk(1, 0, 0);
    V3 v = vunit(vcross(unit_w, a));
    V3 u = vcross(unit_w, v);
    o.u = u; o.v = v; o.w = unit_w;
    return o;
}
DEV V3 onb_local(const Onb &o, V3 a) { return vadd(vadd(vscale(a.x, o.u), vscale(a.y, o.v)), vscale(a.z, o.w)); }

/* ---- short forms of x / a and sqrtf(x): exact by construction, on a guarded range only ----
 *
 * hipcc expands an fp32 division (denormals on) into
 *     a' = v_div_scale(a), x' = v_div_scale(x), r0 = v_rcp_f32(a'), e = fma(-a', r0, 1), r = fma(e, r0, r0),
 *     q0 = x' * r, e1 = fma(-a', q0, x'), q1 = fma(e1, r, q0), e2 = fma(-a', q1, x'), q = v_div_fmas(e2, r, q1), v_div_fixup(q, a, x)
 * and sqrtf into
 *     x' = x < 2^-96 ? x * 2^32 : x, s = v_sqrt_f32(x'), dn / up = s with the integer pattern - 1 / + 1,
 *     s = dn if fma(-dn, s, x') <= 0, s = up if fma(-up, s, x') > 0, the unscale by 2^-16, x itself for a zero or +infinity.
 * The short forms are these sequences without the steps that are identities on the guarded range:
 *   - v_div_scale returns its operand and leaves VCC clear (v_div_fmas is then a plain fma) unless an operand is zero, the denominator
 *     is denormal, 1 / a or x / a is denormal, exponent(x) - exponent(a) >= 96 or the numerator's biased exponent is <= 23;
 *     v_div_fixup returns the quotient it is given unless an operand is zero, infinite or NaN or the quotient leaves the normal range.
 *     With 2^-40 <= a <= 2^40 (div_den_ok) and 2^-85 <= |x| < 2^56 (div_num_ok bounds |x| from above) the exponent difference lies in
 *     [-125, 95] and none of these holds: the quotient is the compiler's, bit for bit, r prepared once per denominator;
 *   - a numerator below 2^-85 (zero and denormals included) is NOT exact here (a zero may lose its sign), but its quotient is finite
 *     and below 2^-44 in magnitude in both forms: a caller that rejects everything below a threshold such as t_min = 0.001 needs no guard;
 *   - 2^-96 <= x < 2^100 (sqrt_arg_ok) is neither scaled nor a zero or an infinity.
 * The compare forms are integer range checks of the bit pattern: NaN, infinities, negative values and both zeros fall outside.
 * Everything outside the guards takes the plain operators.  The host side of DEV is the plain operators throughout.
 * (div_num_ok states the numerator's bound for the tests of div_by alone; the leaf step bounds its numerators through half_b^2 < 2^110 and the
 * discriminant's range instead, mega_bvh.h sphere_short_ok, which the device test of sphere_hit_root_fast covers.)
 * tests/test_exact_forms_host.py runs the *_model functions (the same fma sequences with the hardware's seed as a parameter) against
 * gcc's / and sqrtf; tests/test_gpu_exact_forms.py runs the device forms against the device's / and sqrtf, boundaries included. */
#define MORT_DIV_DEN_LO 0x2b800000u /* 2^-40 */
#define MORT_DIV_DEN_HI 0x53800000u /* 2^40 */
#define MORT_DIV_NUM_HI 0x5b800000u /* 2^56 */
#define MORT_SQRT_LO 0x0f800000u    /* 2^-96 */
#define MORT_SQRT_HI 0x71800000u    /* 2^100 */
DEV bool div_den_ok(float a) { return __builtin_bit_cast(uint32_t, a) - MORT_DIV_DEN_LO <= MORT_DIV_DEN_HI - MORT_DIV_DEN_LO; }
DEV bool div_num_ok(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7fffffffu) < MORT_DIV_NUM_HI; }
DEV bool sqrt_arg_ok(float x) { return __builtin_bit_cast(uint32_t, x) - MORT_SQRT_LO < MORT_SQRT_HI - MORT_SQRT_LO; }

/* the models: seed r0 = the hardware's v_rcp_f32(a), s = v_sqrt_f32(x) */
DEV float div_by_model_prepare(float a, float r0) { const float e = __builtin_fmaf(-a, r0, 1.0f); return __builtin_fmaf(e, r0, r0); }
DEV float div_by_model(float x, float a, float r) {
    const float q0 = x * r;
    const float e1 = __builtin_fmaf(-a, q0, x);
    const float q1 = __builtin_fmaf(e1, r, q0);
    const float e2 = __builtin_fmaf(-a, q1, x);
    return __builtin_fmaf(e2, r, q1);
}
DEV float sqrt_ord_model(float x, float s) {
    const float dn = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, s) - 1u);
    const float up = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, s) + 1u);
    const float vp = __builtin_fmaf(-dn, s, x), vs = __builtin_fmaf(-up, s, x);
    float t = (vp <= 0.0f) ? dn : s;
    t = (vs > 0.0f) ? up : t;
    return t;
}

/* a denominator prepared once: ok = div_den_ok(a); r is meaningful only then */
struct DivBy { float a, r; bool ok; };
DEV DivBy div_prepare(float a) {
    DivBy d; d.a = a; d.ok = div_den_ok(a);
#if defined(__HIP_DEVICE_COMPILE__)
    d.r = div_by_model_prepare(a, __builtin_amdgcn_rcpf(a));
#else
    d.r = 0.0f;
#endif
    return d;
}
/* x / d.a for d.ok and div_num_ok(x) (see above for numerators below 2^-85) */
DEV float div_by(float x, const DivBy &d) {
#if defined(__HIP_DEVICE_COMPILE__)
    return div_by_model(x, d.a, d.r);
#else
    return x / d.a;
#endif
}
/* sqrtf(x) for sqrt_arg_ok(x) */
DEV float sqrt_ord(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return sqrt_ord_model(x, __builtin_amdgcn_sqrtf(x));
#else
    return mort_sqrtf(x);
#endif
}

#endif
