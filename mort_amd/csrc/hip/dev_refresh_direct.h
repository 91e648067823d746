/*
 * dev_refresh_direct.h -- direct-light volume refresh: ONE direction of ONE probe of an irradiance volume of
 * INDIRECT light re-baked through that volume; compiled for the gfx950 kernels of refresh_direct.hip AND run by the host loop there
 * (mort_hip_volume_refresh_direct_host), -ffp-contract=off on both sides, so host and device agree bit for bit.
 *
 * refresh_direction (dev_refresh.h) with the direct cached query's paths (cached_direct_paths, dev_cached_direct.h) under rule E:
 * a path whose primary segment ends on an emitter, or on a material the shade step does not know, has the value 0, so the light a
 * probe sees directly stays out of a record that holds indirect light.  The probe's place in the grid, the blend and the copy of a
 * masked probe are dev_refresh.h's.
 */
#ifndef MORT_DEV_REFRESH_DIRECT_H
#define MORT_DEV_REFRESH_DIRECT_H

#include "mort_hip.h"
#include "dev_refresh.h"
#include "dev_cached_direct.h"

#pragma clang fp contract(off)

template <bool VISIBLE>
struct RefreshDirectArgs {
    RefreshArgs<VISIBLE> r;
    uint32_t *lit; /* P or null: the probe's paths whose shadow segment returned a non-zero emission */
};

/* direction j of probe p: refresh_direction's loads, stores, guard and terms around the direct paths; lit: how many of the paths
 * that ended in the volume had a shadow segment that saw light */
template <bool TREE, bool VISIBLE>
DEV void refresh_direct_direction(const RefreshArgs<VISIBLE> &a, size_t p, V3 origin, float time, int j, unsigned short *walk, int walk_stride,
                                  float4 *lds_stack, int lds_levels, int lds_stride, float term[MORT_SH9_FLOATS], uint32_t &ends, uint32_t &lit) {
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

    const V3 s = cached_direct_paths<TREE, VISIBLE, true>(a.c, ray0, rng, walk, walk_stride, lds_stack, lds_levels, lds_stride, ends, lit);

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
    for (int ch = 0; ch < 3; ch++) if (g[ch] != g[ch]) g[ch] = 0.0f; /* the bake's NaN guard */
    float Y[9];
    probe_basis(ray0.d.x, ray0.d.y, ray0.d.z, Y);
    for (int k = 0; k < 9; k++)
        for (int ch = 0; ch < 3; ch++) term[k * 3 + ch] = Y[k] * g[ch];
}

#endif
