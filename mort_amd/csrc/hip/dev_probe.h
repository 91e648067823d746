/*
 * dev_probe.h -- light probes: the path-traced radiance arriving at ONE probe along ONE direction of its set and
 * that direction's 27 SH9 terms, compiled for the gfx950 kernels of probe.hip AND run by the host loop there
 * (mort_hip_probe_bake_host), -ffp-contract=off on both sides, so host and device agree bit for bit.
 *
 * The paths are the radiance query's own (radiance_paths, dev_radiance.h): the ray is built in registers from the probe record
 * and the direction, nothing of it is stored.  What follows the paths is the contract of include/mort_hip.h, written once here:
 * the NaN guard, the nine basis expressions, the terms, and the balanced tree over the 64 terms of a batch (probe_tree64: the
 * host's form of the kernel's xor-butterfly).
 */
#ifndef MORT_DEV_PROBE_H
#define MORT_DEV_PROBE_H

#include "mort_hip.h"
#include "dev_radiance.h"

#pragma clang fp contract(off)

#define MORT_PROBE_BATCH 64                 /* directions per batch: one per lane of a wave */
#define MORT_PROBE_MAX_DIRECTIONS 4096
#define MORT_PROBE_MAX_BATCHES (MORT_PROBE_MAX_DIRECTIONS / MORT_PROBE_BATCH)

struct ProbeArgs {
    RadianceArgs r;            /* scene, tree, parameters; r.q.states: the n D streams, r.q.n: the probes (rays, rgb unused) */
    const mort_probe *probes;  /* n */
    const float *dirs;         /* 3 D */
    float *sh;                 /* 27 n */
    int directions;            /* D */
    float scale;               /* (float)(4 pi / (D samples)) */
};

/* the real SH basis of bands 0..2 at (x, y, z), as the contract writes it */
DEV void probe_basis(float x, float y, float z, float Y[9]) {
    const float c0 = 0.2820948f, c1 = 0.4886025f, c2 = 1.0925484f, c3 = 0.31539157f, c4 = 0.5462742f;
    Y[0] = c0;
    Y[1] = c1 * y;
    Y[2] = c1 * z;
    Y[3] = c1 * x;
    Y[4] = (c2 * x) * y;
    Y[5] = (c2 * y) * z;
    Y[6] = c3 * ((3.0f * z) * z - 1.0f);
    Y[7] = (c2 * x) * z;
    Y[8] = c4 * (x * x - y * y);
}

/* direction j of probe p: the paths from stream p D + j (advanced in place, d and v[] only), the render's NaN guard on their
 * sum, and term[k * 3 + ch] = Y_k * g[ch] */
template <bool TREE>
DEV void probe_direction(const ProbeArgs &a, size_t p, V3 origin, float time, int j, unsigned short *walk, int walk_stride, float4 *lds_stack,
                         int lds_levels, int lds_stride, float term[MORT_SH9_FLOATS]) {
    mort_rng_state *st = a.r.q.states + (p * (size_t)a.directions + (size_t)j);
    Rng rng;
    rng.draws = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    { /* the 24 bytes the paths read, as dwordx4 + dwordx2 (the _device form asks for 16-byte aligned streams) */
        const uint4 lo = *(const uint4 *)st;
        const uint2 hi = *(const uint2 *)((const unsigned char *)st + 16);
        rng.d = lo.x; rng.v0 = lo.y; rng.v1 = lo.z; rng.v2 = lo.w; rng.v3 = hi.x; rng.v4 = hi.y;
    }
#else
    rng.d = st->d; rng.v0 = st->v[0]; rng.v1 = st->v[1]; rng.v2 = st->v[2]; rng.v3 = st->v[3]; rng.v4 = st->v[4];
#endif
    const float *dj = a.dirs + 3 * (size_t)j;
    Ray ray0;
    ray0.o = origin; ray0.d = mk(dj[0], dj[1], dj[2]); ray0.tm = time; /* the direction exactly as given */

    const V3 s = radiance_paths<TREE>(a.r, ray0, rng, walk, walk_stride, lds_stack, lds_levels, lds_stride);

#if defined(__HIP_DEVICE_COMPILE__)
    {
        uint4 lo; uint2 hi;
        lo.x = rng.d; lo.y = rng.v0; lo.z = rng.v1; lo.w = rng.v2; hi.x = rng.v3; hi.y = rng.v4;
        *(uint4 *)st = lo;
        *(uint2 *)((unsigned char *)st + 16) = hi;
    }
#else
    st->d = rng.d; st->v[0] = rng.v0; st->v[1] = rng.v1; st->v[2] = rng.v2; st->v[3] = rng.v3; st->v[4] = rng.v4;
#endif

    float g[3] = {s.x, s.y, s.z};
    for (int ch = 0; ch < 3; ch++) if (g[ch] != g[ch]) g[ch] = 0.0f; /* the render's NaN guard: one NaN path must not poison the probe */
    float Y[9];
    probe_basis(ray0.d.x, ray0.d.y, ray0.d.z, Y);
    for (int k = 0; k < 9; k++)
        for (int ch = 0; ch < 3; ch++) term[k * 3 + ch] = Y[k] * g[ch];
}

/* the batch's sum: a balanced binary tree over neighbouring indices, x = x[0::2] + x[1::2] six times (destroys x) */
static inline float probe_tree64(float x[MORT_PROBE_BATCH]) {
    for (int m = MORT_PROBE_BATCH / 2; m >= 1; m >>= 1)
        for (int i = 0; i < m; i++) x[i] = x[2 * i] + x[2 * i + 1];
    return x[0];
}

#endif
