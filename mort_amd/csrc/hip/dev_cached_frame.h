/*
 * dev_cached_frame.h -- cached frames: Camera::render for ONE pixel whose paths may end in an irradiance volume,
 * compiled for the gfx950 kernels of cached_frame.hip AND run by the host loop there (mort_hip_render_cached_host),
 * -ffp-contract=off on both sides, so host and device agree bit for bit.
 *
 * render_pixel (dev_pixel.h) restated once with the cached radiance queries' shortcut (cached_end, dev_cached.h) in its bounce
 * loop: the pixel's stream, get_ray per stratum, the flat sample x bounce loop with a segment counted per search, the identity
 * mask, the bounce stack with its LDS levels, the unwind, pixel_finish, pixel_rgba and the stream stored back are the render's,
 * word for word.  The search of a segment is the radiance queries' (radiance_world_hit: the reach test per origin, the walk
 * column), since the frame shares its kernel shape and LDS with them.  With cache_depth at the bounce limit, or a volume without a
 * contributing probe, the pixel is render_pixel's.
 */
#ifndef MORT_DEV_CACHED_FRAME_H
#define MORT_DEV_CACHED_FRAME_H

#include "mort_hip.h"
#include "dev_cached.h"
#include "dev_pixel.h"

#pragma clang fp contract(off)

/* the camera and the volume ride by value (scalar registers on the device); q.n, q.rays and q.states stay null */
template <bool VISIBLE>
struct CachedFrameArgs {
    QueryArgs q;               /* scene, tree, reach */
    CamView cam;               /* what get_ray reads */
    int width, height;
    int sqrt_spp, bounce_limit;
    float pixel_samples_scale;
    V3 background;
    int light_type, light_idx;
    int cache_depth;           /* K: the first iteration that may end in the volume */
    mort_rng_state *states;    /* W H: the pixels' streams */
    uchar4 *rgba;
    float *accum;              /* may be null */
    uint32_t *seg_px;          /* may be null */
    uint32_t *ends;            /* may be null: the paths of a pixel that ended in the volume */
    unsigned long long *counters; /* device: [0] segments, [1] rng draws */
    CachedVolume<VISIBLE> vol;
};

/* pixel lofs = x + y W of the whole image */
template <bool TREE, bool VISIBLE>
DEV PixelTotals cached_frame_pixel(const CachedFrameArgs<VISIBLE> &c, int x, int y, unsigned short *walk, int walk_stride, float4 *lds_stack,
                                   int lds_levels, int lds_stride) {
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
    uint32_t segments = 0, ends = 0;
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
        /* ---- one iteration of ray_color's bounce loop (camera.cuh:96-159) ---- */
        V3 final_value;
        bool done = false;
        if (iter >= c.bounce_limit) {
            final_value = mk(0, 0, 0);
            done = true;
        } else {
            Best best;
            segments++;
            if (!radiance_world_hit<TREE>(c.q, ray, rng, best, walk, walk_stride)) {
                final_value = c.background;
                done = true;
            } else if (iter >= c.cache_depth && cached_end<VISIBLE>(sc, c.vol, ray, best, final_value)) {
                ends++;
                done = true;
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
    c.states[lofs] = rng_state(rng.d, rng.v0, rng.v1, rng.v2, rng.v3, rng.v4);
    PixelTotals t; t.segments = segments; t.draws = rng.draws;
    return t;
}

#endif
