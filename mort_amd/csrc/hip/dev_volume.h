/*
 * dev_volume.h -- irradiance volumes: the irradiance at ONE (position, normal) from a regular grid of packed
 * SH9 probe records, trilinearly blended between the eight surrounding probes under the records' weights; compiled for the
 * gfx950 kernels of volume.hip AND run by the host loop there (mort_hip_volume_sample_host), -ffp-contract=off on both sides,
 * so host and device agree bit for bit.
 *
 * Everything below is the contract of include/mort_hip.h, written once: the cell and the fractions per axis, the nine basis
 * products B_k = A_l(k) Y_k(n), the corners in ascending c = cx + 2 cy + 4 cz, the 9-term sum per channel from the k = 0 product,
 * the accumulation from 0.0f and the division by the weights' sum.  The basis expressions are the bake's (probe_basis,
 * dev_probe.h).
 */
#ifndef MORT_DEV_VOLUME_H
#define MORT_DEV_VOLUME_H

#include <cstring>

#include "mort_hip.h"
#include "dev_math.h"
#include "dev_probe.h"

#pragma clang fp contract(off)

struct VolumeArgs {
    mort_volume_grid g;          /* passed by value: wave-uniform, held in scalar registers */
    float inv[3];                /* 1.0f / spacing, correctly rounded on the host, once per call */
    const float *records;        /* 32 floats per probe */
    const unsigned char *points; /* n records of `stride` bytes, the first 24 of each are read */
    size_t stride;
    size_t n;
    float *out;                  /* 4 n */
};

typedef uint32_t __attribute__((may_alias)) volume_word; /* a float's bits, moved as a word: NaN payloads survive */
struct VolumePackArgs {
    const volume_word *sh;     /* 27 n words, copied bit for bit */
    const volume_word *weight; /* n words or null = 1.0f */
    volume_word *records;      /* 32 n */
    size_t n;
};

struct VolumeAxis { int i0, i1; float w0, w1; };

/* the cell and the two weights along one axis; a coordinate outside the grid takes the boundary, a NaN the first probe */
DEV VolumeAxis volume_axis(float x, float origin, float inv, int count) {
    VolumeAxis r;
    float u = (x - origin) * inv;
    u = (u > 0.0f) ? u : 0.0f;
    const float m = (float)(count - 1);
    u = (u < m) ? u : m;
    int i0 = (int)__builtin_floorf(u);
    if (i0 > count - 2) i0 = count - 2;
    if (i0 < 0) i0 = 0;
    const float f = u - (float)i0;
    r.i0 = i0;
    r.i1 = (i0 + 1 < count) ? i0 + 1 : i0;
    r.w0 = 1.0f - f;
    r.w1 = f;
    return r;
}

/* B_k = A_l(k) * Y_k(n), the normal as given */
DEV void volume_basis(float nx, float ny, float nz, float B[9]) {
    const float A0 = (float)M_PI, A1 = (float)(2.0 * M_PI / 3.0), A2 = (float)(M_PI / 4.0);
    float Y[9];
    probe_basis(nx, ny, nz, Y);
    B[0] = A0 * Y[0];
    for (int k = 1; k < 4; k++) B[k] = A1 * Y[k];
    for (int k = 4; k < 9; k++) B[k] = A2 * Y[k];
}

/* 16 bytes of a record: four floats from r */
DEV float4 volume_quad(const float *r) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const float4 *)r; /* the _device form asks for 16-byte aligned records */
#else
    float4 q;
    std::memcpy(&q, r, sizeof q);
    return q;
#endif
}

/* the record's last quarter that is read: sh[24..26] and the weight */
struct VolumeCorner { const float *rec; float T, W; float4 tail; };

DEV void volume_corner_begin(VolumeCorner &c, const float *records, size_t p, float T) {
    c.rec = records + p * MORT_VOLUME_RECORD_FLOATS;
    c.T = T;
    c.W = 0.0f;
    if (T > 0.0f) { /* T == 0: W is 0 or NaN whatever the weight, the corner cannot contribute: nothing of it is loaded */
        c.tail = volume_quad(c.rec + 24);
        c.W = T * c.tail.w;
    }
}

/* acc and wsum take corner c if it contributes; its first 96 bytes are loaded only then */
DEV void volume_corner_add(const VolumeCorner &c, const float B[9], float acc[3], float &wsum) {
    if (!(c.W > 0.0f)) return;
    float sh[MORT_SH9_FLOATS];
#pragma unroll
    for (int q = 0; q < 6; q++) {
        const float4 v = volume_quad(c.rec + 4 * q);
        sh[4 * q + 0] = v.x; sh[4 * q + 1] = v.y; sh[4 * q + 2] = v.z; sh[4 * q + 3] = v.w;
    }
    sh[24] = c.tail.x; sh[25] = c.tail.y; sh[26] = c.tail.z;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        float e = B[0] * sh[ch]; /* the k = 0 product: no leading 0 + */
#pragma unroll
        for (int k = 1; k < 9; k++) e = e + B[k] * sh[k * 3 + ch];
        acc[ch] = acc[ch] + c.W * e;
    }
    wsum = wsum + c.W;
}

/* one sample: position (px, py, pz), normal (nx, ny, nz) -> {E_r, E_g, E_b, wsum} */
DEV float4 volume_sample_point(const VolumeArgs &a, float px, float py, float pz, float nx, float ny, float nz) {
    const VolumeAxis ax = volume_axis(px, a.g.origin[0], a.inv[0], a.g.count[0]);
    const VolumeAxis ay = volume_axis(py, a.g.origin[1], a.inv[1], a.g.count[1]);
    const VolumeAxis az = volume_axis(pz, a.g.origin[2], a.inv[2], a.g.count[2]);
    float B[9];
    volume_basis(nx, ny, nz, B);
    float acc[3] = {0.0f, 0.0f, 0.0f};
    float wsum = 0.0f;
    /* corners c = 2 j and 2 j + 1 (the x neighbours of row cy = j & 1, cz = j >> 1) per step, not unrolled: two records in flight */
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
        const int iy = (j & 1) ? ay.i1 : ay.i0, iz = (j & 2) ? az.i1 : az.i0;
        const float wy = (j & 1) ? ay.w1 : ay.w0, wz = (j & 2) ? az.w1 : az.w0;
        const size_t row = ((size_t)iz * (size_t)a.g.count[1] + (size_t)iy) * (size_t)a.g.count[0];
        VolumeCorner c0, c1;
        volume_corner_begin(c0, a.records, row + (size_t)ax.i0, (ax.w0 * wy) * wz);
        volume_corner_begin(c1, a.records, row + (size_t)ax.i1, (ax.w1 * wy) * wz);
        volume_corner_add(c0, B, acc, wsum);
        volume_corner_add(c1, B, acc, wsum);
    }
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (wsum > 0.0f) {
        /* 1.0f / wsum, correctly rounded: the short form where the denominator allows it (dev_math.h), else the plain operator */
        const DivBy d = div_prepare(wsum);
        const float r = d.ok ? div_by(1.0f, d) : 1.0f / wsum;
        o = make_float4(acc[0] * r, acc[1] * r, acc[2] * r, wsum);
    }
    return o;
}

/* point i of the batch: its 24 bytes in ... */
struct VolumePointIn { float p[6]; };
DEV VolumePointIn volume_load_point(const VolumeArgs &a, size_t i) {
    const unsigned char *src = a.points + i * a.stride;
    VolumePointIn r;
#if defined(__HIP_DEVICE_COMPILE__)
    if ((a.stride & 15u) == 0) { /* wave-uniform; the points' base is 16-byte aligned: 16 + 8 bytes */
        const float4 lo = *(const float4 *)src;
        const float2 hi = *(const float2 *)(src + 16);
        r.p[0] = lo.x; r.p[1] = lo.y; r.p[2] = lo.z; r.p[3] = lo.w; r.p[4] = hi.x; r.p[5] = hi.y;
    } else {
#pragma unroll
        for (int k = 0; k < 6; k++) r.p[k] = ((const float *)src)[k];
    }
#else
    std::memcpy(r.p, src, sizeof r.p);
#endif
    return r;
}

/* ... and its 16 bytes out */
DEV void volume_store_sample(const VolumeArgs &a, size_t i, float4 o) {
#if defined(__HIP_DEVICE_COMPILE__)
    *(float4 *)(a.out + 4 * i) = o;
#else
    std::memcpy(a.out + 4 * i, &o, sizeof o);
#endif
}

DEV void volume_sample_one(const VolumeArgs &a, size_t i) {
    const VolumePointIn r = volume_load_point(a, i);
    volume_store_sample(a, i, volume_sample_point(a, r.p[0], r.p[1], r.p[2], r.p[3], r.p[4], r.p[5]));
}

/* 16 bytes t of the packed records: quarter t & 7 of record t >> 3 */
DEV void volume_pack_quad(const VolumePackArgs &a, size_t t) {
    const size_t p = t >> 3;
    const int q = (int)(t & 7);
    const volume_word *s = a.sh + p * MORT_SH9_FLOATS + 4 * q;
    uint32_t v[4] = {0u, 0u, 0u, 0u}; /* quarter 7: four 0.0f */
    if (q < 6) {
        v[0] = s[0]; v[1] = s[1]; v[2] = s[2]; v[3] = s[3];
    } else if (q == 6) {
        v[0] = s[0]; v[1] = s[1]; v[2] = s[2];
        v[3] = a.weight ? a.weight[p] : 0x3f800000u;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    uint4 o; o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
    *(uint4 *)(a.records + 4 * t) = o;
#else
    std::memcpy(a.records + 4 * t, v, sizeof v);
#endif
}

#endif
