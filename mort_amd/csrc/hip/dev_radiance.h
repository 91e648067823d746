/*
 * dev_radiance.h -- radiance queries: the path-traced colour along ONE caller ray, compiled for the gfx950
 * kernels of radiance.hip AND run by the host loop there (mort_hip_query_radiance_host), -ffp-contract=off on both sides, so
 * host and device agree bit for bit.
 *
 * render_pixel (dev_pixel.h) without its camera and its pixel: the flat sample x bounce loop of Camera::render / ray_color
 * (camera.cuh:86-190) over shade_hit, the identity-level mask, the StackEntry bounce stack and the unwind expressions are
 * the render's; there is no get_ray, no pixel tail (scale, NaN guard, gamma) and no segment counter.  The search of a segment
 * is the ray queries' (dev_query.h): every segment's origin takes the reach test, since a caller's ray -- and so every ray
 * scattered from where it lands -- may start anywhere.
 */
#ifndef MORT_DEV_RADIANCE_H
#define MORT_DEV_RADIANCE_H

#include "mort_hip.h"
#include "dev_query.h"
#include "dev_shade.h"

#pragma clang fp contract(off)

#define MORT_RADIANCE_LDS_LEVELS 8 /* bounce-stack levels kept in LDS: 8 x 256 x 16 B beside the 8 KB walk column = 40 KB, four groups per CU */

struct RadianceArgs {
    QueryArgs q;               /* scene, tree, reach, n, rays, states (hits and occluded unused) */
    float *rgb;                /* 3 n floats */
    int bounce_limit, samples;
    V3 background;
    int light_type, light_idx;
};

/* world::hit(ray, interval(0.001, inf), rec) for one segment.  TREE: the unified tree as a closest-hit query searches it
 * (reach test, walk with its pending children at walk[k * walk_stride], scan for a ray the walk does not decide), then the
 * media; else world::hit's item loop as mega_kernel runs it (world_hit, dev_trace.h, in the ray queries' form: query_items) */
template <bool TREE>
DEV bool radiance_world_hit(const QueryArgs &q, const Ray &ray, Rng &rng, Best &best, unsigned short *walk, int walk_stride) {
    if (!TREE) { /* a caller's zero-length or NaN direction can make closest_so_far a NaN, which the render's walk never meets */
        query_items<true, false>(q.sc, ray, __builtin_inff(), rng, best);
        return best.kind != HIT_NONE;
    }
    float closest;
    uint32_t e;
    query_tree_solids<false>(q, ray, __builtin_inff(), walk, walk_stride, closest, e);
    gen_media(q.sc, q.gw.first_medium, q.sc.n_items, ray, rng, closest, e);
    if (e == GBEST_NONE) return false;
    best = gen_decode_best(q.sc, q.gw.chains, e, closest);
    return true;
}

/* the paths of one ray: ((0 + c_1) + c_2) + ... + c_samples, c_k the k-th ray_color of ray0 drawn from rng, both in the
 * caller's registers (a radiance query loads them, a light probe builds the ray: dev_probe.h).
 * The first lds_levels bounce-stack levels of this ray live at lds_stack[level * lds_stride] (the kernel: the lane's column of
 * an LDS array; the host loop: a local array), the rest in the private array, as in render_pixel */
template <bool TREE>
DEV V3 radiance_paths(const RadianceArgs &a, const Ray ray0, Rng &rng, unsigned short *walk, int walk_stride, float4 *lds_stack, int lds_levels, int lds_stride) {
    const DScene &sc = a.q.sc;
    StackEntry stack[MORT_MAX_BOUNCE_LIMIT];
    unsigned long long ident_mask = 0ull; /* levels whose entry is the identity (dielectric): not stored */
    V3 color = mk(0, 0, 0);
    int s = 0, iter = 0;
    Ray ray = ray0;
    const float ray_time0 = ray0.tm;

    while (s < a.samples) {
        /* ---- one iteration of ray_color's bounce loop (camera.cuh:96-159) ---- */
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
        if (done) { /* unwind (camera.cuh:165-173) and accumulate (camera.cuh:190) */
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
            ray = ray0; /* the next path of the same ray */
        }
    }
    return color;
}

/* one radiance query: rgb[i] = the paths' sum for ray i drawn from stream i */
template <bool TREE>
DEV void radiance_ray(const RadianceArgs &a, size_t i, unsigned short *walk, int walk_stride, float4 *lds_stack, int lds_levels, int lds_stride) {
    Ray ray0;
    float t_max_ignored; /* ray_color always searches [0.001, inf) */
    query_load_ray(a.q.rays, i, ray0, t_max_ignored);

    Rng rng;
    {
        const mort_rng_state *st = a.q.states + i;
        rng.d = st->d; rng.v0 = st->v[0]; rng.v1 = st->v[1]; rng.v2 = st->v[2]; rng.v3 = st->v[3]; rng.v4 = st->v[4];
        rng.draws = 0;
    }

    const V3 color = radiance_paths<TREE>(a, ray0, rng, walk, walk_stride, lds_stack, lds_levels, lds_stride);

    { /* d and v[] only: the words this path never reads keep the caller's bits */
        mort_rng_state *st = a.q.states + i;
        st->d = rng.d; st->v[0] = rng.v0; st->v[1] = rng.v1; st->v[2] = rng.v2; st->v[3] = rng.v3; st->v[4] = rng.v4;
    }
    struct Rgb { float r, g, b; }; /* one 12-byte store */
    Rgb out; out.r = color.x; out.g = color.y; out.b = color.z;
    *(Rgb *)(a.rgb + 3 * i) = out;
}

#endif
