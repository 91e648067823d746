/*
 * dev_refresh.h -- volume refresh: ONE direction of ONE probe of an irradiance volume re-baked through the volume
 * as it stands, and the blend of the probe's new coefficients into its record; compiled for the gfx950 kernels of refresh.hip
 * AND run by the host loop there (mort_hip_volume_refresh_host), -ffp-contract=off on both sides, so host and device agree bit
 * for bit.
 *
 * The pieces are the tree's own: the probe's position is mort_hip_volume_probes' arithmetic, the stream is loaded and stored as
 * probe_direction (dev_probe.h) does it, the paths are cached_paths (dev_cached.h) over the records the call reads, and the guard,
 * the basis and the terms are the bake's.  What is new is written once here: the probe's place in the grid, the blend under the
 * hysteresis, and the copy of a masked probe.
 */
#ifndef MORT_DEV_REFRESH_H
#define MORT_DEV_REFRESH_H

#include "mort_hip.h"
#include "dev_probe.h"
#include "dev_cached.h"

#pragma clang fp contract(off)

template <bool VISIBLE>
struct RefreshArgs {
    CachedArgs<VISIBLE> c;  /* scene, tree, path parameters, K, the volume by value over records_in (and the maps);
                               c.r.q.states: the P D streams of the whole grid; c.r.q.rays, c.r.rgb and c.ends stay null */
    const float *dirs;      /* 3 D */
    volume_word *out;       /* records_out: 32 P words, the selected records are written */
    uint32_t *ends;         /* P or null */
    int directions;         /* D */
    float scale;            /* (float)(4 pi / (D samples)) */
    float h, om;            /* the hysteresis and 1.0f - h, rounded once per call */
    uint32_t first, step;   /* selected probe i: first + i step */
};

DEV const float *refresh_records(const VolumeArgs &v) { return v.records; }
DEV const float *refresh_records(const VolumeVisArgs &v) { return v.v.records; }
DEV const mort_volume_grid &refresh_grid(const VolumeArgs &v) { return v.g; }
DEV const mort_volume_grid &refresh_grid(const VolumeVisArgs &v) { return v.v.g; }

/* probe p = (iz ny + iy) nx + ix of the grid: its position, as mort_hip_volume_probes writes it (the product rounded, then the sum) */
DEV V3 refresh_position(const mort_volume_grid &g, size_t p) {
    const size_t nx = (size_t)g.count[0], ny = (size_t)g.count[1];
    const int ix = (int)(p % nx), iy = (int)((p / nx) % ny), iz = (int)(p / (nx * ny));
    const float sx = (float)ix * g.spacing[0], sy = (float)iy * g.spacing[1], sz = (float)iz * g.spacing[2];
    return mk(g.origin[0] + sx, g.origin[1] + sy, g.origin[2] + sz);
}

/* a record's weight: > 0 or the probe is masked and its record copied */
DEV bool refresh_masked(const float *records_in, size_t p) { return !(records_in[p * MORT_VOLUME_RECORD_FLOATS + MORT_SH9_FLOATS] > 0.0f); }

/* direction j of probe p: probe_direction with the cached paths -- the stream p D + j loaded and stored the same way, the guard on
 * the paths' sum, term[k * 3 + ch] = Y_k * g[ch]; ends: how many of the paths ended in the volume */
template <bool TREE, bool VISIBLE>
DEV void refresh_direction(const RefreshArgs<VISIBLE> &a, size_t p, V3 origin, float time, int j, unsigned short *walk, int walk_stride,
                           float4 *lds_stack, int lds_levels, int lds_stride, float term[MORT_SH9_FLOATS], uint32_t &ends) {
    mort_rng_state *st = a.c.r.q.states + (p * (size_t)a.directions + (size_t)j);
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

    const V3 s = cached_paths<TREE, VISIBLE>(a.c, ray0, rng, walk, walk_stride, lds_stack, lds_levels, lds_stride, ends);

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
    for (int ch = 0; ch < 3; ch++) if (g[ch] != g[ch]) g[ch] = 0.0f; /* the bake's NaN guard: a poisoned record reaches one direction, not the probe */
    float Y[9];
    probe_basis(ray0.d.x, ray0.d.y, ray0.d.z, Y);
    for (int k = 0; k < 9; k++)
        for (int ch = 0; ch < 3; ch++) term[k * 3 + ch] = Y[k] * g[ch];
}

/* word i of the probe's new record: floats 0..26 blended (acc: the fixed-order sum of that float's terms), the weight copied, zeros */
DEV uint32_t refresh_word(int i, const volume_word *old_record, float acc, float scale, float h, float om) {
    if (i > MORT_SH9_FLOATS) return 0u;
    const uint32_t old_word = old_record[i];
    if (i == MORT_SH9_FLOATS) return old_word;
    const float fresh = scale * acc;
    if (h == 0.0f) return __builtin_bit_cast(uint32_t, fresh); /* no 0 * old: an old NaN or infinity is gone */
    const float keep = h * __builtin_bit_cast(float, old_word), take = om * fresh;
    return __builtin_bit_cast(uint32_t, keep + take);
}

#endif
