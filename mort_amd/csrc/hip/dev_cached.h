/*
 * dev_cached.h -- cached radiance queries: the colour along ONE caller ray by paths that end in an irradiance
 * volume, compiled for the gfx950 kernels of cached.hip AND run by the host loop there (mort_hip_query_radiance_cached_host),
 * -ffp-contract=off on both sides, so host and device agree bit for bit.
 *
 * radiance_paths (dev_radiance.h) with one addition: a segment that has found a Lambertian hit at iteration >= cache_depth asks the
 * volume for the irradiance there (volume_sample_point / volume_vis_sample_point as they stand, dev_volume.h / dev_depth.h) and,
 * if a probe contributes, ends with (albedo * E) * INV_PI without a draw.  Everything else -- the search per segment, the media,
 * shade_hit for every other hit, the identity mask, the bounce stack with its LDS levels and the unwind -- is the radiance queries',
 * word for word, so a cache_depth at the bounce limit or a volume without a contributing probe gives a plain radiance query.
 */
#ifndef MORT_DEV_CACHED_H
#define MORT_DEV_CACHED_H

#include "mort_hip.h"
#include "dev_radiance.h"
#include "dev_volume.h"
#include "dev_depth.h"

#pragma clang fp contract(off)

/* the volume rides by value, as VolumeArgs has it (its points, stride, n and out stay null); the plain form carries no depth maps */
template <bool VISIBLE> struct CachedVolume { VolumeArgs v; };
template <> struct CachedVolume<true> { VolumeVisArgs v; };

template <bool VISIBLE>
struct CachedArgs {
    RadianceArgs r;
    int cache_depth;  /* K: the first iteration that may end in the volume */
    uint32_t *ends;   /* n or null: the paths of a ray that ended in the volume */
    CachedVolume<VISIBLE> vol;
};

DEV float4 cached_sample(const VolumeArgs &v, V3 p, V3 n) { return volume_sample_point(v, p.x, p.y, p.z, n.x, n.y, n.z); }
DEV float4 cached_sample(const VolumeVisArgs &v, V3 p, V3 n) { return volume_vis_sample_point(v, p.x, p.y, p.z, n.x, n.y, n.z); }

/* the hit `best` of `ray` at an iteration >= cache_depth: true if the path ends in the volume, final_value its radiance.  The albedo
 * is looked up before the sample, so that only the point and its normal are live across the corners' loop */
template <bool VISIBLE>
DEV bool cached_end(const DScene &sc, const CachedVolume<VISIBLE> &vol, const Ray &ray, const Best &best, V3 &final_value) {
    const float INV_PI = (float)(1.0 / 3.14159265358979323846);
    HitRec rec;
    resolve_hit(sc, ray, best, rec);
    if (DREF_TYPE(rec.mat) != MORT_MAT_LAMBERTIAN) return false;
    const DLambert m = sc.lambert[DREF_IDX(rec.mat)];
    const V3 albedo = lambert_color_rec(sc, m, rec);
    const float4 E = cached_sample(vol.v, rec.p, rec.normal);
    if (!(E.w > 0.0f)) return false; /* no probe contributes (a weight sum of 0 or NaN): the hit is shaded as any other */
    final_value = mk((albedo.x * E.x) * INV_PI, (albedo.y * E.y) * INV_PI, (albedo.z * E.z) * INV_PI);
    return true;
}

/* radiance_paths with the shortcut; ends: how many of the paths took it */
template <bool TREE, bool VISIBLE>
DEV V3 cached_paths(const CachedArgs<VISIBLE> &c, const Ray ray0, Rng &rng, unsigned short *walk, int walk_stride, float4 *lds_stack, int lds_levels,
                    int lds_stride, uint32_t &ends) {
    const RadianceArgs &a = c.r;
    const DScene &sc = a.q.sc;
    StackEntry stack[MORT_MAX_BOUNCE_LIMIT];
    unsigned long long ident_mask = 0ull; /* levels whose entry is the identity (dielectric): not stored */
    V3 color = mk(0, 0, 0);
    int s = 0, iter = 0;
    Ray ray = ray0;
    const float ray_time0 = ray0.tm;
    ends = 0;

    while (s < a.samples) {
        V3 final_value;
        bool done = false;
        if (iter >= a.bounce_limit) {
            final_value = mk(0, 0, 0);
            done = true;
        } else {
            Best best;
            if (!radiance_world_hit<TREE>(a.q, ray, rng, best, walk, walk_stride)) {
                final_value = a.background;
                done = true;
            } else if (iter >= c.cache_depth && cached_end<VISIBLE>(sc, c.vol, ray, best, final_value)) {
                ends++;
                done = true;
            } else {
                const ShadeOut so = shade_hit(sc, a.light_type, a.light_idx, ray, ray_time0, best, rng);
                if (so.done) { final_value = so.final_value; done = true; }
                else {
                    if (so.ident) ident_mask |= (1ull << iter);
                    else if (iter < lds_levels) { float4 e4; e4.x = so.e.kx; e4.y = so.e.ky; e4.z = so.e.kz; e4.w = so.e.rp; lds_stack[iter * lds_stride] = e4; }
                    else stack[iter] = so.e;
                    iter++;
                }
            }
        }
        if (done) { /* the radiance queries' unwind and sum */
            while (iter > 0) {
                iter--;
                if ((ident_mask >> iter) & 1ull) { final_value = vadd(mk(0, 0, 0), final_value); continue; }
                StackEntry e;
                if (iter < lds_levels) { const float4 e4 = lds_stack[iter * lds_stride]; e.kx = e4.x; e.ky = e4.y; e.kz = e4.z; e.rp = e4.w; }
                else e = stack[iter];
                const V3 t = vmul(mk(e.kx, e.ky, e.kz), final_value);
                final_value = vadd(mk(0, 0, 0), vscale(e.rp, t));
            }
            ident_mask = 0ull;
            color = vadd(color, final_value);
            s++;
            ray = ray0;
        }
    }
    return color;
}

/* one cached query: radiance_ray's loads and stores, and the ray's count where the caller asked for it */
template <bool TREE, bool VISIBLE>
DEV void cached_ray(const CachedArgs<VISIBLE> &c, size_t i, unsigned short *walk, int walk_stride, float4 *lds_stack, int lds_levels, int lds_stride) {
    const RadianceArgs &a = c.r;
    Ray ray0;
    float t_max_ignored;
    query_load_ray(a.q.rays, i, ray0, t_max_ignored);

    Rng rng;
    {
        const mort_rng_state *st = a.q.states + i;
        rng.d = st->d; rng.v0 = st->v[0]; rng.v1 = st->v[1]; rng.v2 = st->v[2]; rng.v3 = st->v[3]; rng.v4 = st->v[4];
        rng.draws = 0;
    }

    uint32_t ends;
    const V3 color = cached_paths<TREE, VISIBLE>(c, ray0, rng, walk, walk_stride, lds_stack, lds_levels, lds_stride, ends);

    {
        mort_rng_state *st = a.q.states + i;
        st->d = rng.d; st->v[0] = rng.v0; st->v[1] = rng.v1; st->v[2] = rng.v2; st->v[3] = rng.v3; st->v[4] = rng.v4;
    }
    struct Rgb { float r, g, b; };
    Rgb out; out.r = color.x; out.g = color.y; out.b = color.z;
    *(Rgb *)(a.rgb + 3 * i) = out;
    if (c.ends) c.ends[i] = ends;
}

#endif
