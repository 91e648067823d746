/*
 * dev_cached_frame_direct.h -- direct-light cached frames: Camera::render for ONE pixel whose paths may end in an
 * irradiance volume of INDIRECT light and add one sampled shadow segment toward the camera's light object there, compiled for the
 * gfx950 kernels of cached_frame_direct.hip AND run by the host loop there (mort_hip_render_cached_direct_host),
 * -ffp-contract=off on both sides, so host and device agree bit for bit.
 *
 * cached_frame_pixel (dev_cached_frame.h) with the terminal of cached_direct_paths (dev_cached_direct.h): the pixel's stream,
 * get_ray per stratum, the flat sample x bounce loop, the identity mask, the bounce stack with its LDS levels, the unwind,
 * pixel_finish, pixel_rgba and the stream stored back are the cached frame's, word for word.  The shadow segment goes through the
 * loop's ONE search call: the path keeps its DirectPending, replaces its ray and takes one more turn of the loop under `shadow`,
 * so the kernel holds one copy of the tree walk, as cached_frame_kernel does.  That search is counted as a segment.
 */
#ifndef MORT_DEV_CACHED_FRAME_DIRECT_H
#define MORT_DEV_CACHED_FRAME_DIRECT_H

#include "mort_hip.h"
#include "dev_cached_direct.h"
#include "dev_cached_frame.h"

#pragma clang fp contract(off)

template <bool VISIBLE>
struct CachedFrameDirectArgs {
    CachedFrameArgs<VISIBLE> f;
    uint32_t *lit; /* W H or null: the paths of a pixel whose shadow segment returned a non-zero emission */
};

/* pixel lofs = x + y W of the whole image */
template <bool TREE, bool VISIBLE>
DEV PixelTotals cached_frame_direct_pixel(const CachedFrameDirectArgs<VISIBLE> &d, int x, int y, unsigned short *walk, int walk_stride,
                                          float4 *lds_stack, int lds_levels, int lds_stride) {
    const CachedFrameArgs<VISIBLE> &c = d.f;
    const DScene &sc = c.q.sc;
    const size_t lofs = (size_t)x + (size_t)y * (size_t)c.width;

    Rng rng = rng_load(c.states[lofs]);

    StackEntry stack[MORT_MAX_BOUNCE_LIMIT];
    unsigned long long ident_mask = 0ull; /* levels whose entry is the identity (dielectric): not stored */
    V3 pixel_color = mk(0, 0, 0);
    const int spp = c.sqrt_spp * c.sqrt_spp;
    int s = 0, s_i = 0, s_j = 0;
    int iter = 0;
    bool fresh = true;
    bool shadow = false; /* `ray` is the shadow segment of a path that has ended in the volume; `pend` is that path's */
    DirectPending pend;
    pend.base = mk(0, 0, 0); pend.k = mk(0, 0, 0); pend.pdf = 0.0f;
    uint32_t segments = 0, ends = 0, lit = 0;
    Ray ray;
    ray.o = mk(0, 0, 0); ray.d = mk(0, 0, 1); ray.tm = 0;
    float ray_time0 = 0.f;

    while (s < spp) {
        if (fresh) { /* camera.cuh:187-190 */
            ray = get_ray(c.cam, x, y, rng, s_i, s_j);
            ray_time0 = ray.tm;
            iter = 0;
            fresh = false;
        }
        /* ---- one iteration of ray_color's bounce loop (camera.cuh:96-159), or the shadow segment of a path that has ended ---- */
        V3 final_value;
        bool done = false;
        if (!shadow && iter >= c.bounce_limit) {
            final_value = mk(0, 0, 0);
            done = true;
        } else {
            Best best;
            segments++;
            const bool hit = radiance_world_hit<TREE>(c.q, ray, rng, best, walk, walk_stride); /* the one search: path and shadow segments */
            if (shadow) { /* a miss is 0, not the background: the background is in the probes */
                const V3 Le = hit ? direct_emission(sc, ray, best) : mk(0, 0, 0);
                if (Le.x != 0.0f || Le.y != 0.0f || Le.z != 0.0f) lit++;
                final_value = mk(pend.base.x + ((pend.k.x * Le.x) / pend.pdf), pend.base.y + ((pend.k.y * Le.y) / pend.pdf),
                                 pend.base.z + ((pend.k.z * Le.z) / pend.pdf));
                shadow = false;
                done = true;
            } else if (!hit) {
                final_value = c.background;
                done = true;
            } else {
                V3 albedo, p, normal;
                if (iter >= c.cache_depth && cached_direct_end<VISIBLE>(sc, c.vol, ray, best, pend.base, albedo, p, normal)) {
                    ends++;
                    if (c.light_type == -1 || iter + 1 >= c.bounce_limit) { /* no direct term: the cached frame's value, nothing drawn */
                        final_value = pend.base;
                        done = true;
                    } else {
                        direct_sample(sc, c.light_type, c.light_idx, albedo, p, normal, ray_time0, rng, ray, pend);
                        shadow = true;
                    }
                } else {
                    const ShadeOut so = shade_hit(sc, c.light_type, c.light_idx, ray, ray_time0, best, rng);
                    if (so.done) { final_value = so.final_value; done = true; }
                    else {
                        if (so.ident) ident_mask |= (1ull << iter);
                        else if (iter < lds_levels) { float4 e4; e4.x = so.e.kx; e4.y = so.e.ky; e4.z = so.e.kz; e4.w = so.e.rp; lds_stack[iter * lds_stride] = e4; }
                        else stack[iter] = so.e;
                        iter++;
                    }
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
            pixel_color = vadd(pixel_color, final_value);
            s++;
            s_i++;
            if (s_i == c.sqrt_spp) { s_i = 0; s_j++; }
            fresh = true;
        }
    }

    /* camera.cuh:194-207 */
    pixel_color = pixel_finish(c.pixel_samples_scale, pixel_color);
    if (c.accum) { c.accum[3 * lofs] = pixel_color.x; c.accum[3 * lofs + 1] = pixel_color.y; c.accum[3 * lofs + 2] = pixel_color.z; }
    pixel_rgba(c.rgba[lofs], pixel_color);
    if (c.seg_px) c.seg_px[lofs] = segments;
    if (c.ends) c.ends[lofs] = ends;
    if (d.lit) d.lit[lofs] = lit;
    c.states[lofs] = rng_state(rng.d, rng.v0, rng.v1, rng.v2, rng.v3, rng.v4);
    PixelTotals t; t.segments = segments; t.draws = rng.draws;
    return t;
}

#endif
