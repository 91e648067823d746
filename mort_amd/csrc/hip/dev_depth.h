/*
 * dev_depth.h -- visibility-weighted irradiance volumes: ONE interior texel of a probe's octahedral depth map
 * (the first two moments of the distance to the nearest solid over the texel's s x s sub-samples) and ONE sample of the volume
 * with every corner's weight multiplied by the Chebyshev visibility read from that corner's map; compiled for the gfx950 kernels
 * of depth.hip / volume.hip AND run by the host loops there, -ffp-contract=off on both sides, so host and device agree bit for bit.
 *
 * Everything below is the contract of include/mort_hip.h, written once.  The search is the ray queries' (dev_query.h), unchanged:
 * media passed over, nothing drawn.  The sample is dev_volume.h's but for the corner weight: its axes, basis, record quarters
 * and final division are used as they are.
 */
#ifndef MORT_DEV_DEPTH_H
#define MORT_DEV_DEPTH_H

#include <cstring>

#include "mort_hip.h"
#include "dev_query.h"
#include "dev_volume.h"

#pragma clang fp contract(off)

constexpr int DEPTH_SIDE = MORT_DEPTH_RES + 2; /* texels per row, border included */

struct DepthArgs {
    QueryArgs q;              /* the scene and, for TREE, the walk and its reach; rays, states, hits and occluded stay null */
    const mort_probe *probes; /* n */
    size_t n;
    float *depth;             /* MORT_DEPTH_FLOATS n */
    int s;                    /* sub-samples per texel side */
    float step, inv;          /* 2.0f / (float)(8 s) and 1.0f / (float)(s s), rounded once on the host */
    float max_distance;
};

struct VolumeVisArgs {
    VolumeArgs v;
    const float *depth; /* MORT_DEPTH_FLOATS per probe, grid index order */
    float normal_bias, min_visibility;
};

/* the octahedral direction of (u, v) in [-1, 1]^2, not normalised */
DEV V3 depth_direction(float u, float v) {
    const float au = mort_fabsf(u), av = mort_fabsf(v);
    const float z = (1.0f - au) - av;
    float x = u, y = v;
    if (z < 0.0f) {
        x = (1.0f - av) * (u >= 0.0f ? 1.0f : -1.0f);
        y = (1.0f - au) * (v >= 0.0f ? 1.0f : -1.0f);
    }
    return mk(x, y, z);
}

/* interior texel (i + 1, j + 1), i, j in 0..7: its s x s rays one after the other, b ascending, a ascending within b */
template <bool TREE>
DEV void depth_texel(const DepthArgs &a, V3 origin, float time, int i, int j, unsigned short *stack, int stride, float &m1, float &m2) {
    m1 = 0.0f; m2 = 0.0f;
    for (int sb = 0; sb < a.s; sb++) {
        const float v = ((float)(j * a.s + sb) + 0.5f) * a.step - 1.0f;
        for (int sa = 0; sa < a.s; sa++) {
            const float u = ((float)(i * a.s + sa) + 0.5f) * a.step - 1.0f;
            Ray ray;
            ray.o = origin; ray.d = depth_direction(u, v); ray.tm = time;
            float t;
            bool hit;
            if (TREE) {
                uint32_t e;
                query_tree_solids<false>(a.q, ray, __builtin_inff(), stack, stride, t, e);
                hit = e != GBEST_NONE;
            } else {
                Rng none;
                none.d = none.v0 = none.v1 = none.v2 = none.v3 = none.v4 = 0; none.draws = 0;
                Best best;
                query_items<false, false>(a.q.sc, ray, __builtin_inff(), none, best);
                hit = best.kind != HIT_NONE;
                t = best.t;
            }
            const float len = mort_sqrtf((ray.d.x * ray.d.x + ray.d.y * ray.d.y) + ray.d.z * ray.d.z);
            float d = hit ? t * len : a.max_distance;
            d = (d < a.max_distance) ? d : a.max_distance; /* a NaN goes to the cap */
            m1 = m1 + d;
            m2 = m2 + d * d;
        }
    }
    m1 = m1 * a.inv;
    m2 = m2 * a.inv;
}

DEV void depth_put(float *map, int I, int J, float m1, float m2) {
    float *t = map + 2 * (J * DEPTH_SIDE + I);
#if defined(__HIP_DEVICE_COMPILE__)
    *(float2 *)t = make_float2(m1, m2); /* a map is 800 bytes from a 16-byte aligned base: every texel is 8-byte aligned */
#else
    const float m[2] = {m1, m2};
    std::memcpy(t, m, sizeof m);
#endif
}

/* interior texel (I, J), I, J in 1..8, and the border texels that copy it: one or two on an edge, the diagonal one at a corner */
DEV void depth_store(float *map, int I, int J, float m1, float m2) {
    const int R = MORT_DEPTH_RES;
    depth_put(map, I, J, m1, m2);
    if (I == 1) depth_put(map, 0, R + 1 - J, m1, m2);
    if (I == R) depth_put(map, R + 1, R + 1 - J, m1, m2);
    if (J == 1) depth_put(map, R + 1 - I, 0, m1, m2);
    if (J == R) depth_put(map, R + 1 - I, R + 1, m1, m2);
    if ((I == 1 || I == R) && (J == 1 || J == R)) depth_put(map, I == 1 ? R + 1 : 0, J == 1 ? R + 1 : 0, m1, m2); /* the opposite corner */
}

/* 8 bytes of a map: texel (i, j) */
DEV float2 depth_tap(const float *map, int i, int j) {
    const float *t = map + 2 * (j * DEPTH_SIDE + i);
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const float2 *)t;
#else
    float2 m;
    std::memcpy(&m, t, sizeof m);
    return m;
#endif
}

struct DepthCoord { int i0; float f; };
DEV DepthCoord depth_coord(float o) {
    DepthCoord c;
    const float t = (o * 0.5f + 0.5f) * (float)MORT_DEPTH_RES + 0.5f;
    int i0 = (int)__builtin_floorf(t);
    if (i0 > MORT_DEPTH_RES) i0 = MORT_DEPTH_RES;
    if (i0 < 0) i0 = 0;
    c.i0 = i0;
    c.f = t - (float)i0;
    return c;
}

/* acc and wsum take the corner at probe p = (ix, iy, iz) with trilinear weight T under its visibility from q.  Its map and its
 * coefficients are loaded only when T * weight > 0, then together: the taps need nothing of the record */
DEV void volume_vis_corner(const VolumeVisArgs &a, const VolumeCorner &c, size_t p, int ix, int iy, int iz, const float q[3], const float B[9],
                           float acc[3], float &wsum) {
    if (!(c.W > 0.0f)) return;
    const mort_volume_grid &g = a.v.g;
    const int idx[3] = {ix, iy, iz};
    float v[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float step = (float)idx[k] * g.spacing[k]; /* rounded, then the sum */
        const float pos = g.origin[k] + step;
        v[k] = q[k] - pos;
    }
    const float s1 = (mort_fabsf(v[0]) + mort_fabsf(v[1])) + mort_fabsf(v[2]);
    const bool dir = (s1 > 0.0f) && (s1 < __builtin_inff());
    /* Everything from here to W is straight-line code with selects, on purpose: the four taps must be whole 8-byte loads issued in
     * one block with the six coefficient loads.  With `if (dir)` / `if (r > m1)` as branches the compiler split every tap into its
     * two dwords and sank the m2 halves under the comparison, a third dependent round trip.  No direction: ox = oy = 0, the taps
     * read the map's centre and V below is 1 whatever they hold */
    const float qx = v[0] / s1, qy = v[1] / s1;
    const float fx = (1.0f - mort_fabsf(qy)) * (qx >= 0.0f ? 1.0f : -1.0f);
    const float fy = (1.0f - mort_fabsf(qx)) * (qy >= 0.0f ? 1.0f : -1.0f);
    const bool fold = v[2] < 0.0f;
    const float ox = dir ? (fold ? fx : qx) : 0.0f;
    const float oy = dir ? (fold ? fy : qy) : 0.0f;
    const DepthCoord cx = depth_coord(ox), cy = depth_coord(oy);
    const float *map = a.depth + p * MORT_DEPTH_FLOATS;
    const float2 t00 = depth_tap(map, cx.i0, cy.i0), t10 = depth_tap(map, cx.i0 + 1, cy.i0);
    const float2 t01 = depth_tap(map, cx.i0, cy.i0 + 1), t11 = depth_tap(map, cx.i0 + 1, cy.i0 + 1);
    float sh[MORT_SH9_FLOATS];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const float4 w = volume_quad(c.rec + 4 * k);
        sh[4 * k + 0] = w.x; sh[4 * k + 1] = w.y; sh[4 * k + 2] = w.z; sh[4 * k + 3] = w.w;
    }
    sh[24] = c.tail.x; sh[25] = c.tail.y; sh[26] = c.tail.z;

    const float r = mort_sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const float gx = 1.0f - cx.f, gy = 1.0f - cy.f;
    const float top1 = t00.x * gx + t10.x * cx.f, bot1 = t01.x * gx + t11.x * cx.f;
    const float top2 = t00.y * gx + t10.y * cx.f, bot2 = t01.y * gx + t11.y * cx.f;
    const float m1 = top1 * gy + bot1 * cy.f;
    const float m2 = top2 * gy + bot2 * cy.f;
    const float var = mort_fabsf(m2 - m1 * m1);
    const float dl = r - m1;
    const float den = var + dl * dl;
    const float k = (den > 0.0f) ? var / den : 0.0f;
    float Vc = (k * k) * k;
    Vc = (Vc > a.min_visibility) ? Vc : a.min_visibility;
    const float V = (dir && r > m1) ? Vc : 1.0f; /* r > m1 is false for a NaN on either side */
    const float W = c.W * V;
    const bool on = W > 0.0f; /* a select, not a branch: a branch here lets the compiler sink the coefficient loads below the taps' wait */
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        float e = B[0] * sh[ch]; /* the k = 0 product: no leading 0 + */
#pragma unroll
        for (int k = 1; k < 9; k++) e = e + B[k] * sh[k * 3 + ch];
        const float sum = acc[ch] + W * e;
        acc[ch] = on ? sum : acc[ch];
    }
    const float ws = wsum + W;
    wsum = on ? ws : wsum;
}

/* one sample: position (px, py, pz), normal (nx, ny, nz) -> {E_r, E_g, E_b, wsum} */
DEV float4 volume_vis_sample_point(const VolumeVisArgs &a, float px, float py, float pz, float nx, float ny, float nz) {
    const VolumeArgs &va = a.v;
    const VolumeAxis ax = volume_axis(px, va.g.origin[0], va.inv[0], va.g.count[0]);
    const VolumeAxis ay = volume_axis(py, va.g.origin[1], va.inv[1], va.g.count[1]);
    const VolumeAxis az = volume_axis(pz, va.g.origin[2], va.inv[2], va.g.count[2]);
    float B[9];
    volume_basis(nx, ny, nz, B);
    const float bx = a.normal_bias * nx, by = a.normal_bias * ny, bz = a.normal_bias * nz;
    const float q[3] = {px + bx, py + by, pz + bz};
    float acc[3] = {0.0f, 0.0f, 0.0f};
    float wsum = 0.0f;
    /* as volume_sample_point: corners 2 j and 2 j + 1 per step, not unrolled */
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
        const int iy = (j & 1) ? ay.i1 : ay.i0, iz = (j & 2) ? az.i1 : az.i0;
        const float wy = (j & 1) ? ay.w1 : ay.w0, wz = (j & 2) ? az.w1 : az.w0;
        const size_t row = ((size_t)iz * (size_t)va.g.count[1] + (size_t)iy) * (size_t)va.g.count[0];
        VolumeCorner c0, c1;
        volume_corner_begin(c0, va.records, row + (size_t)ax.i0, (ax.w0 * wy) * wz);
        volume_corner_begin(c1, va.records, row + (size_t)ax.i1, (ax.w1 * wy) * wz);
        volume_vis_corner(a, c0, row + (size_t)ax.i0, ax.i0, iy, iz, q, B, acc, wsum);
        volume_vis_corner(a, c1, row + (size_t)ax.i1, ax.i1, iy, iz, q, B, acc, wsum);
    }
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (wsum > 0.0f) {
        const DivBy d = div_prepare(wsum);
        const float r = d.ok ? div_by(1.0f, d) : 1.0f / wsum;
        o = make_float4(acc[0] * r, acc[1] * r, acc[2] * r, wsum);
    }
    return o;
}

/* point i of the batch: its 24 bytes in, its 16 bytes out (dev_volume.h's loads and store) */
DEV void volume_vis_sample_one(const VolumeVisArgs &a, size_t i) {
    const VolumePointIn r = volume_load_point(a.v, i);
    volume_store_sample(a.v, i, volume_vis_sample_point(a, r.p[0], r.p[1], r.p[2], r.p[3], r.p[4], r.p[5]));
}

#endif
