/*
 * dev_query.h -- ray queries: closest hit and occlusion for ONE caller ray, compiled for the gfx950 kernels
 * of query.hip AND run by the host loops there (mort_hip_query_*_host), -ffp-contract=off on both sides, so host and device
 * agree bit for bit.
 *
 * No traversal of its own: the unified-tree walk and its scan (dev_gen.h), world::hit's item loop (the body of world_hit,
 * dev_trace.h, started at closest = t_max), the media and resolve_hit are the render's, used unchanged.  What is new here is
 * the interval's far end per ray, the reach test per ray (the render checks its one camera on the host) and the record.
 */
#ifndef MORT_DEV_QUERY_H
#define MORT_DEV_QUERY_H

#include "mort_hip.h"
#include "dev_gen.h"

#pragma clang fp contract(off)

struct QueryArgs {
    DScene sc;
    GenWalk gw;                /* valid when the launch walks the unified tree */
    float lo[3], hi[3], reach; /* the box of the tree's solids and how far from it an origin may lie (build_unified) */
    size_t n;
    const mort_ray *rays;
    mort_rng_state *states;    /* closest hit with media: one stream per ray */
    mort_hit *hits;            /* closest hit */
    uint8_t *occluded;         /* occlusion */
};

/* a ray as two 16-byte loads, a record as three 16-byte stores (the _device forms ask for 16-byte aligned buffers; the host
 * forms take the caller's pointers as they are) */
DEV void query_load_ray(const mort_ray *rays, size_t i, Ray &ray, float &t_max) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float4 *p = (const float4 *)(rays + i);
    const float4 a = p[0], b = p[1];
    ray.o = mk(a.x, a.y, a.z); ray.d = mk(a.w, b.x, b.y); ray.tm = b.z; t_max = b.w;
#else
    const mort_ray r = rays[i];
    ray.o = mk(r.origin[0], r.origin[1], r.origin[2]); ray.d = mk(r.dir[0], r.dir[1], r.dir[2]); ray.tm = r.time; t_max = r.t_max;
#endif
}
DEV void query_store_hit(mort_hit *hits, size_t i, const mort_hit &h) {
#if defined(__HIP_DEVICE_COMPILE__)
    float4 *p = (float4 *)(hits + i);
    float4 a, b, c;
    a.x = h.p[0]; a.y = h.p[1]; a.z = h.p[2]; a.w = h.normal[0];
    b.x = h.normal[1]; b.y = h.normal[2]; b.z = h.t; b.w = h.u;
    c.x = h.v; c.y = __int_as_float(h.mat_type); c.z = __int_as_float(h.mat_idx); c.w = __uint_as_float(h.flags);
    p[0] = a; p[1] = b; p[2] = c;
#else
    hits[i] = h;
#endif
}

/* camera_in_reach (mort_ctx.h) for one origin, rad = 0: the tree's pads are sized for origins within `reach` of the solids'
 * box.  A NaN or infinite coordinate fails every comparison it takes part in */
DEV bool query_in_reach(const QueryArgs &a, V3 o) {
    const float v[3] = {o.x, o.y, o.z};
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; k++)
        if (!(v[k] >= a.lo[k] - a.reach && v[k] <= a.hi[k] + a.reach)) in = false;
    return in;
}

DEV Best query_no_hit() { Best b; b.kind = HIT_NONE; b.t = 0; b.prim = 0; b.chain_first = 0; b.chain_count = 0; return b; }

/* world::hit (world.cuh:104-171) over [0.001, t_max]: the body of world_hit (dev_trace.h) started at closest = t_max.
 * MEDIA false: every constant medium is passed over and rng is not touched.  ANY: stop after the first item that was hit */
template <bool MEDIA, bool ANY>
DEV void query_items(const DScene &sc, const Ray &r, float t_max, Rng &rng, Best &best) {
    const float t_min = 0.001f;
    float closest = t_max;
    best = query_no_hit();
    for (int i = 0; i < sc.n_items; i++) {
        const DItem it = sc.items[i];
        const int kind = it.kind;
        if (kind == ITEM_BVH) run_bvh_t<true>(sc, r, it.first, it.count, t_min, closest, best); /* a NaN closest_so_far as aabb::hit reads it */
        if (kind == ITEM_SPHERES) run_spheres(sc, r, it.first, it.count, it.chain_first, it.chain_count, t_min, closest, best);
        if (kind == ITEM_QUADS) run_quads(sc, r, it.first, it.count, it.chain_first, it.chain_count, t_min, closest, best);
        if (ANY && best.kind != HIT_NONE) break;
        if (MEDIA && kind != ITEM_BVH && kind != ITEM_SPHERES && kind != ITEM_QUADS) { /* constant_medium::hit, objects.cuh:396-434 */
            const Ray rm = apply_chain(sc, r, it.chain_first, it.chain_count);
            float t1, t2;
            if (!boundary_t(sc, r, it.first, it.count, -__builtin_inff(), __builtin_inff(), t1)) continue;
            if (!boundary_t(sc, r, it.first, it.count, (float)((double)t1 + 0.0001), __builtin_inff(), t2)) continue;
            if (t1 < t_min) t1 = t_min;
            if (t2 > closest) t2 = closest;
            if (t1 >= t2) continue;
            if (t1 < 0) t1 = 0;
            const float ray_length = vlen(rm.d);
            const float distance_inside_boundary = (t2 - t1) * ray_length;
            const double hit_distance = sc.neg_inv_density[it.medium] * (double)mort_logf(random_float(rng));
            if (hit_distance > (double)distance_inside_boundary) continue;
            const float t = (float)((double)t1 + hit_distance / (double)ray_length);
            closest = t;
            best.t = t; best.kind = HIT_MEDIUM; best.prim = i; best.chain_first = it.chain_first; best.chain_count = it.chain_count;
        }
    }
}

/* the solids through the unified tree over [0.001, t_max]: the single-lane walk for an origin within reach, then the scan for
 * the rays the walk does not decide -- an origin out of reach, a reciprocal that is not ordinary (a zero, denormal, huge or
 * NaN direction component), a NaN root.  ANY: the walk returns at its first accepted root; a flagged ray is still re-decided */
template <bool ANY>
DEV void query_tree_solids(const QueryArgs &a, const Ray &ray, float t_max, unsigned short *stack, int stride, float &closest, uint32_t &e) {
    int flags = GFL_REF;
    closest = t_max; e = GBEST_NONE;
    if (query_in_reach(a, ray.o)) gen_walk_solids_from<ANY>(a.sc, a.gw, ray, stack, stride, t_max, closest, e, flags);
    if (flags) gen_scan_solids_from(a.sc, a.gw.first_medium, a.gw.chains, a.gw.n_chains, ray, t_max, closest, e);
}

/* one closest-hit query.  TREE: the unified tree (stack as in feat_tree_solids, dev_features.h), else the item loop.
 * MEDIA: a.states is given */
template <bool TREE, bool MEDIA>
DEV void query_closest_ray(const QueryArgs &a, size_t i, unsigned short *stack, int stride) {
    const DScene &sc = a.sc;
    Ray ray;
    float t_max;
    query_load_ray(a.rays, i, ray, t_max);
    mort_hit h;
    h.p[0] = h.p[1] = h.p[2] = 0.0f; h.normal[0] = h.normal[1] = h.normal[2] = 0.0f;
    h.t = 0.0f; h.u = 0.0f; h.v = 0.0f; h.mat_type = 0; h.mat_idx = 0; h.flags = 0;
    if (t_max > 0.001f) {
        Rng rng;
        rng.d = rng.v0 = rng.v1 = rng.v2 = rng.v3 = rng.v4 = 0; rng.draws = 0;
        if (MEDIA) {
            const mort_rng_state *st = a.states + i;
            rng.d = st->d; rng.v0 = st->v[0]; rng.v1 = st->v[1]; rng.v2 = st->v[2]; rng.v3 = st->v[3]; rng.v4 = st->v[4];
        }
        Best best = query_no_hit();
        if (TREE) {
            float closest;
            uint32_t e;
            query_tree_solids<false>(a, ray, t_max, stack, stride, closest, e);
            if (MEDIA) gen_media(sc, a.gw.first_medium, sc.n_items, ray, rng, closest, e);
            if (e != GBEST_NONE) best = gen_decode_best(sc, a.gw.chains, e, closest);
        } else {
            query_items<MEDIA, false>(sc, ray, t_max, rng, best);
        }
        if (MEDIA) { /* d and v[] only: the words this path never reads keep the caller's bits */
            mort_rng_state *st = a.states + i;
            st->d = rng.d; st->v[0] = rng.v0; st->v[1] = rng.v1; st->v[2] = rng.v2; st->v[3] = rng.v3; st->v[4] = rng.v4;
        }
        if (best.kind != HIT_NONE) {
            HitRec rec;
            resolve_hit(sc, ray, best, rec);
            if (rec.uv_sphere) sphere_uv(rec.on, rec.u, rec.v); /* resolve_hit leaves a sphere's (u, v) to whoever reads them */
            h.p[0] = rec.p.x; h.p[1] = rec.p.y; h.p[2] = rec.p.z;
            h.normal[0] = rec.normal.x; h.normal[1] = rec.normal.y; h.normal[2] = rec.normal.z;
            h.t = rec.t; h.u = rec.u; h.v = rec.v;
            h.mat_type = DREF_TYPE(rec.mat); h.mat_idx = DREF_IDX(rec.mat);
            h.flags = MORT_HIT_HIT | (rec.front_face ? MORT_HIT_FRONT_FACE : 0u) | (best.kind == HIT_MEDIUM ? MORT_HIT_MEDIUM : 0u);
        }
    }
    query_store_hit(a.hits, i, h);
}

/* one occlusion query: is a solid hit in [0.001, t_max] */
template <bool TREE>
DEV void query_occluded_ray(const QueryArgs &a, size_t i, unsigned short *stack, int stride) {
    Ray ray;
    float t_max;
    query_load_ray(a.rays, i, ray, t_max);
    bool hit = false;
    if (t_max > 0.001f) {
        if (TREE) {
            float closest;
            uint32_t e;
            query_tree_solids<true>(a, ray, t_max, stack, stride, closest, e);
            hit = e != GBEST_NONE;
        } else {
            Rng none;
            none.d = none.v0 = none.v1 = none.v2 = none.v3 = none.v4 = 0; none.draws = 0;
            Best best;
            query_items<false, true>(a.sc, ray, t_max, none, best);
            hit = best.kind != HIT_NONE;
        }
    }
    a.occluded[i] = hit ? 1 : 0;
}

#endif
