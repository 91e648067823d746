/*
 * dev_cached_direct.h -- direct-light cached radiance queries: the colour along ONE caller ray by paths that end in
 * an irradiance volume of INDIRECT light and add one sampled shadow segment toward the light object there, compiled for the gfx950
 * kernels of cached_direct.hip AND run by the host loop there (mort_hip_query_radiance_cached_direct_host), -ffp-contract=off on
 * both sides, so host and device agree bit for bit.
 *
 * cached_paths (dev_cached.h) with one change, at the hit where a path ends in the volume: unless the call names no light object or
 * the bounce limit leaves no segment, the path draws a direction toward the light (light_random, dev_render.h), searches that
 * shadow segment as any other segment is searched, and adds (albedo * scattering_pdf) * Le / pdf to (albedo * E) * INV_PI, Le the
 * emission of a diffuse light the segment ends on and 0 otherwise.  The shadow segment goes through the loop's ONE search call: the
 * path keeps what it needs of the terminal hit (DirectPending, seven floats) and takes one more turn of the loop, so the kernel
 * holds one copy of the tree walk, as query_radiance_cached_kernel does.
 */
#ifndef MORT_DEV_CACHED_DIRECT_H
#define MORT_DEV_CACHED_DIRECT_H

#include "mort_hip.h"
#include "dev_cached.h"

#pragma clang fp contract(off)

template <bool VISIBLE>
struct CachedDirectArgs {
    CachedArgs<VISIBLE> c;
    uint32_t *lit; /* n or null: the paths of a ray whose shadow segment returned a non-zero emission */
};

/* what a path that has ended in the volume carries across its shadow segment */
struct DirectPending {
    V3 base;   /* (albedo * E) * INV_PI: the cached query's final value */
    V3 k;      /* albedo * scattering_pdf */
    float pdf; /* light_pdf_value of the drawn direction */
};

/* cached_end (dev_cached.h) that also hands out the hit's point, facing normal and albedo: the light sample starts there */
template <bool VISIBLE>
DEV bool cached_direct_end(const DScene &sc, const CachedVolume<VISIBLE> &vol, const Ray &ray, const Best &best, V3 &base, V3 &albedo, V3 &p, V3 &normal) {
    const float INV_PI = (float)(1.0 / 3.14159265358979323846);
    HitRec rec;
    resolve_hit(sc, ray, best, rec);
    if (DREF_TYPE(rec.mat) != MORT_MAT_LAMBERTIAN) return false;
    const DLambert m = sc.lambert[DREF_IDX(rec.mat)];
    albedo = lambert_color_rec(sc, m, rec);
    const float4 E = cached_sample(vol.v, rec.p, rec.normal);
    if (!(E.w > 0.0f)) return false; /* no probe contributes (a weight sum of 0 or NaN): the hit is shaded as any other */
    base = mk((albedo.x * E.x) * INV_PI, (albedo.y * E.y) * INV_PI, (albedo.z * E.z) * INV_PI);
    p = rec.p; normal = rec.normal;
    return true;
}

/* the light sample at a terminal hit: the direction from the ray's stream as hittable_pdf::generate draws it, its pdf_value, and
 * lambertian::scattering_pdf's face rule over INV_PI.  `ray` becomes the shadow segment (p, dir, time) */
DEV void direct_sample(const DScene &sc, int light_type, int light_idx, V3 albedo, V3 p, V3 normal, float ray_time0, Rng &rng, Ray &ray, DirectPending &d) {
    const float INV_PI = (float)(1.0 / 3.14159265358979323846);
    const V3 dir = light_random(sc, light_type, light_idx, p, rng);
    d.pdf = light_pdf_value(sc, light_type, light_idx, p, dir);
    const float cosine = vdot(normal, vunit(dir));
    const float spdf = (cosine < 0) ? 0.0f : cosine * INV_PI;
    d.k = mk(albedo.x * spdf, albedo.y * spdf, albedo.z * spdf);
    ray.o = p; ray.d = dir; ray.tm = ray_time0;
}

/* what the shadow segment's hit sends back: emitted() of a diffuse light with its face rule and its texture, as shade_hit's
 * emissive branch (dev_shade.h); 0 for every other material -- no scatter is evaluated and nothing is drawn */
DEV V3 direct_emission(const DScene &sc, const Ray &ray, const Best &best) {
    HitRec rec;
    resolve_hit(sc, ray, best, rec);
    if (DREF_TYPE(rec.mat) != MORT_MAT_DIFFUSE_LIGHT || !rec.front_face) return mk(0, 0, 0);
    return lambert_color_rec(sc, sc.dlight[DREF_IDX(rec.mat)], rec);
}

/* cached_paths with the direct terminal; ends: the paths that ended in the volume, lit: those of them whose shadow segment saw light.
 * PRIMARY_DARK (the direct refresh's rule E): a path whose primary segment ends in the shade step's non-scattering
 * branch has the value 0 -- the search, the shade step and every draw are made as without it */
template <bool TREE, bool VISIBLE, bool PRIMARY_DARK = false>
DEV V3 cached_direct_paths(const CachedArgs<VISIBLE> &c, const Ray ray0, Rng &rng, unsigned short *walk, int walk_stride, float4 *lds_stack,
                           int lds_levels, int lds_stride, uint32_t &ends, uint32_t &lit) {
    const RadianceArgs &a = c.r;
    const DScene &sc = a.q.sc;
    StackEntry stack[MORT_MAX_BOUNCE_LIMIT];
    unsigned long long ident_mask = 0ull; /* levels whose entry is the identity (dielectric): not stored */
    V3 color = mk(0, 0, 0);
    int s = 0, iter = 0;
    Ray ray = ray0;
    const float ray_time0 = ray0.tm;
    bool shadow = false; /* `ray` is the shadow segment of a path that has ended in the volume; `pend` is that path's */
    DirectPending pend;
    pend.base = mk(0, 0, 0); pend.k = mk(0, 0, 0); pend.pdf = 0.0f;
    ends = 0; lit = 0;

    while (s < a.samples) {
        V3 final_value;
        bool done = false;
        if (!shadow && iter >= a.bounce_limit) {
            final_value = mk(0, 0, 0);
            done = true;
        } else {
            Best best;
            const bool hit = radiance_world_hit<TREE>(a.q, ray, rng, best, walk, walk_stride); /* the one search: path and shadow segments */
            if (shadow) { /* a miss is 0, not the background: the background is in the probes */
                const V3 Le = hit ? direct_emission(sc, ray, best) : mk(0, 0, 0);
                if (Le.x != 0.0f || Le.y != 0.0f || Le.z != 0.0f) lit++;
                final_value = mk(pend.base.x + ((pend.k.x * Le.x) / pend.pdf), pend.base.y + ((pend.k.y * Le.y) / pend.pdf),
                                 pend.base.z + ((pend.k.z * Le.z) / pend.pdf));
                shadow = false;
                done = true;
            } else if (!hit) {
                final_value = a.background;
                done = true;
            } else {
                V3 albedo, p, normal;
                if (iter >= c.cache_depth && cached_direct_end<VISIBLE>(sc, c.vol, ray, best, pend.base, albedo, p, normal)) {
                    ends++;
                    if (a.light_type == -1 || iter + 1 >= a.bounce_limit) { /* no direct term: the cached query's value, nothing drawn */
                        final_value = pend.base;
                        done = true;
                    } else {
                        direct_sample(sc, a.light_type, a.light_idx, albedo, p, normal, ray_time0, rng, ray, pend);
                        shadow = true;
                    }
                } else {
                    const ShadeOut so = shade_hit(sc, a.light_type, a.light_idx, ray, ray_time0, best, rng);
                    if (so.done) {
                        final_value = so.final_value;
                        if constexpr (PRIMARY_DARK) { if (iter == 0) final_value = mk(0, 0, 0); }
                        done = true;
                    } else {
                        if (so.ident) ident_mask |= (1ull << iter);
                        else if (iter < lds_levels) { float4 e4; e4.x = so.e.kx; e4.y = so.e.ky; e4.z = so.e.kz; e4.w = so.e.rp; lds_stack[iter * lds_stride] = e4; }
                        else stack[iter] = so.e;
                        iter++;
                    }
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

/* one query: cached_ray's loads and stores, and the second count where the caller asked for it */
template <bool TREE, bool VISIBLE>
DEV void cached_direct_ray(const CachedDirectArgs<VISIBLE> &d, size_t i, unsigned short *walk, int walk_stride, float4 *lds_stack, int lds_levels,
                           int lds_stride) {
    const RadianceArgs &a = d.c.r;
    Ray ray0;
    float t_max_ignored;
    query_load_ray(a.q.rays, i, ray0, t_max_ignored);

    Rng rng;
    {
        const mort_rng_state *st = a.q.states + i;
        rng.d = st->d; rng.v0 = st->v[0]; rng.v1 = st->v[1]; rng.v2 = st->v[2]; rng.v3 = st->v[3]; rng.v4 = st->v[4];
        rng.draws = 0;
    }

    uint32_t ends, lit;
    const V3 color = cached_direct_paths<TREE, VISIBLE>(d.c, ray0, rng, walk, walk_stride, lds_stack, lds_levels, lds_stride, ends, lit);

    {
        mort_rng_state *st = a.q.states + i;
        st->d = rng.d; st->v[0] = rng.v0; st->v[1] = rng.v1; st->v[2] = rng.v2; st->v[3] = rng.v3; st->v[4] = rng.v4;
    }
    struct Rgb { float r, g, b; };
    Rgb out; out.r = color.x; out.g = color.y; out.b = color.z;
    *(Rgb *)(a.rgb + 3 * i) = out;
    if (d.c.ends) d.c.ends[i] = ends;
    if (d.lit) d.lit[i] = lit;
}

#endif
