/*
 * cached_frame_direct.hip -- direct-light cached frames: cached frames (cached_frame.hip) over a volume of INDIRECT
 * light whose paths, where they end in the volume, add one sampled shadow segment toward the camera's light object, the terminal
 * of the direct-light cached queries (cached_direct.hip).  The render's outputs (uchar4, accumulators, per-pixel segments,
 * streams, statistics), the cached frame's `ends` and one more count per pixel, `lit`.
 *
 * Kernel (gfx950, wave64, 256-thread groups, one lane per pixel, an 8x8 pixel tile per wave as mega_kernel, 1-D grid):
 *   cached_frame_direct_kernel<TREE, VISIBLE>   cached_frame_kernel's shape and LDS (the walk column where the world has a tree and
 *                                 MORT_RADIANCE_LDS_LEVELS bounce-stack levels) around cached_frame_direct_pixel
 *                                 (dev_cached_frame_direct.h), which searches path and shadow segments at ONE call site.  Held to
 *                                 the cached frames' resource rule by the build (scripts/kernel_resources.py); the waves per SIMD
 *                                 each instantiation is compiled for are DESIGN.md 4.23's table.
 *
 * The host form (mort_hip_render_cached_direct_host) runs the same per-pixel body on host threads and makes no HIP runtime call.
 * The checks, the arguments and the statistics restate cached_frame.hip's with `lit` as one more output; that file and its
 * kernels stay as they are.
 */
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstring>

#include "mort_hip.h"
#include "dev_cached_frame_direct.h"
#include "scene_blob.h"
#include "mort_ctx.h"
#include "mort_internal.h"
#include "stage_common.h"
#include "query_common.h"

#pragma clang fp contract(off)

/* ====================================================================== device */

/* waves per SIMD the kernel is compiled for: the highest that does not spill.  MORT_CFD_WAVES compiles all four
 * at one value, for that table */
#ifdef MORT_CFD_WAVES
#define CFD_WAVES(TREE, VISIBLE) (MORT_CFD_WAVES)
#else
#define CFD_WAVES(TREE, VISIBLE) ((TREE) ? 2 : 3)
#endif

template <bool TREE, bool VISIBLE>
__global__ void __launch_bounds__(QUERY_BLOCK, CFD_WAVES(TREE, VISIBLE)) cached_frame_direct_kernel(const CachedFrameDirectArgs<VISIBLE> d) {
    __shared__ unsigned short walk_stack[TREE ? MORT_OWN_STACK * QUERY_BLOCK : 1];
    __shared__ float4 bounce_stack[MORT_RADIANCE_LDS_LEVELS * QUERY_BLOCK];
    /* an 8x8 pixel tile per wave, as cached_frame_kernel */
    const int lane = threadIdx.x & 63, tiles_x = (d.f.width + 7) >> 3;
    const size_t wave = (size_t)blockIdx.x * (QUERY_BLOCK / 64) + (threadIdx.x >> 6);
    const int x = (int)(wave % (size_t)tiles_x) * 8 + (lane & 7);
    const size_t row = (wave / (size_t)tiles_x) * 8 + (size_t)(lane >> 3);
    if (x >= d.f.width || row >= (size_t)d.f.height) return;
    const int y = (int)row;
    const PixelTotals t = cached_frame_direct_pixel<TREE, VISIBLE>(d, x, y, &walk_stack[TREE ? threadIdx.x : 0], QUERY_BLOCK, bounce_stack + threadIdx.x,
                                                                   MORT_RADIANCE_LDS_LEVELS, QUERY_BLOCK);
    atomicAdd(&d.f.counters[0], (unsigned long long)t.segments);
    atomicAdd(&d.f.counters[1], (unsigned long long)t.draws);
}

/* ====================================================================== host */

namespace {

constexpr size_t kRecordBytes = MORT_VOLUME_RECORD_FLOATS * sizeof(float);
constexpr size_t kDepthBytes = MORT_DEPTH_FLOATS * sizeof(float);

/* 256-thread groups of a frame: four 8x8 pixel tiles each */
size_t frame_groups(int W, int H) { return ((size_t)((W + 7) / 8) * (size_t)((H + 7) / 8) + 3) / 4; }

/* the cached frame's checks (cached_frame.hip frame_check) with `lit` among the outputs */
int frame_check(const mort_camera *cam, const mort_cached_frame_params *p, const void *records, const void *depth, void *states, void *rgba,
                void *accum, void *segpx, void *ends, void *lit) {
    if (!cam || !p || !rgba) return MORT_ERR_INVALID;
    const int W = cam->image_width, H = cam->image_height;
    if (W <= 0 || H <= 0 || cam->sqrt_spp < 0) return MORT_ERR_INVALID;
    if (cam->bounce_limit < 0 || cam->bounce_limit > MORT_MAX_BOUNCE_LIMIT) return MORT_ERR_CAPACITY;
    if (!mort_cached_volume_ok(p->cache_depth, p->flags, &p->grid, &p->vis, records, depth)) return MORT_ERR_INVALID;
    const size_t npx = (size_t)W * (size_t)H;
    if (npx > kMaxRays || frame_groups(W, H) > (size_t)0x7fffffff) return MORT_ERR_CAPACITY; /* a 1-D grid of 256-thread groups */
    const size_t probes = (size_t)p->grid.count[0] * (size_t)p->grid.count[1] * (size_t)p->grid.count[2];
    const void *ins[2] = {records, depth};
    const size_t in_bytes[2] = {probes * kRecordBytes, probes * kDepthBytes};
    void *outs[6] = {states, rgba, accum, segpx, ends, lit};
    const size_t out_bytes[6] = {npx * sizeof(mort_rng_state), npx * 4, npx * 12, npx * 4, npx * 4, npx * 4};
    return buffers_disjoint(ins, in_bytes, 2, outs, out_bytes, 6) ? MORT_OK : MORT_ERR_INVALID;
}

/* everything of the arguments but the scene (d.f.q: query_args_device / query_args_host come first, they clear it) */
template <bool VISIBLE>
void frame_args(CachedFrameDirectArgs<VISIBLE> &d, const mort_camera *cam, const mort_cached_frame_params *p, const void *records, const void *depth,
                mort_rng_state *states, void *rgba, void *accum, void *segpx, void *ends, void *lit, unsigned long long *counters) {
    CachedFrameArgs<VISIBLE> &c = d.f;
    RenderArgs a; /* the camera as every render kernel takes it */
    std::memset(&a, 0, sizeof a);
    render_args_camera(a, cam);
    cam_view_fill(c.cam, a);
    c.width = a.width; c.height = a.height; c.sqrt_spp = a.sqrt_spp; c.bounce_limit = a.bounce_limit;
    c.pixel_samples_scale = a.pixel_samples_scale; c.background = a.background;
    c.light_type = a.light_type; c.light_idx = a.light_idx;
    c.cache_depth = p->cache_depth;
    c.states = states; c.rgba = (uchar4 *)rgba; c.accum = (float *)accum; c.seg_px = (uint32_t *)segpx; c.ends = (uint32_t *)ends;
    c.counters = counters;
    d.lit = (uint32_t *)lit;
    if constexpr (VISIBLE) mort_cached_volume(c.vol.v, p->grid, p->vis, records, depth);
    else mort_cached_volume(c.vol.v, p->grid, records);
}

typedef const void *kernel_ptr;
template <bool VISIBLE>
kernel_ptr frame_launch(const mort_ctx *ctx, const CachedFrameDirectArgs<VISIBLE> &d, hipStream_t s) {
    const dim3 grid((unsigned)frame_groups(d.f.width, d.f.height)), block(QUERY_BLOCK);
    if (ctx->gen_ok) {
        hipLaunchKernelGGL((cached_frame_direct_kernel<true, VISIBLE>), grid, block, 0, s, d);
        return (kernel_ptr)cached_frame_direct_kernel<true, VISIBLE>;
    }
    hipLaunchKernelGGL((cached_frame_direct_kernel<false, VISIBLE>), grid, block, 0, s, d);
    return (kernel_ptr)cached_frame_direct_kernel<false, VISIBLE>;
}

/* the statistics of a direct cached frame, once its stop event has been recorded: the cached frame's, and 4 B per pixel for lit */
int frame_stats(mort_ctx *c, kernel_ptr kernel, bool tree, bool visible, int W, int H, int sqrt_spp, bool has_accum, bool has_ends, bool has_lit,
                mort_stats *stats) {
    HIPCHK(c, hipEventSynchronize(c->ev1));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    unsigned long long cnt[2] = {0, 0};
    HIPCHK(c, hipMemcpy(cnt, c->d_counters, sizeof cnt, hipMemcpyDeviceToHost));
    std::memset(stats, 0, sizeof *stats);
    stats->seconds = ms * 1e-3;
    stats->segments = cnt[0];
    stats->rng_draws = cnt[1];
    stats->pixels = (uint64_t)W * (uint64_t)H;
    stats->eff_samples = stats->pixels * (uint64_t)(sqrt_spp * sqrt_spp);
    stats->algorithmic_hbm_bytes = stats->pixels * (uint64_t)(100 + (has_accum ? 12 : 0) + (has_ends ? 4 : 0) + (has_lit ? 4 : 0));
    stats->local_rows = H;
    std::snprintf(stats->kernel_name, sizeof stats->kernel_name, "cached_frame_direct_kernel<%s, %s>", tree ? "true" : "false", visible ? "true" : "false");
    hipFuncAttributes fattr;
    if (hipFuncGetAttributes(&fattr, kernel) == hipSuccess) { stats->kernel_vgprs = fattr.numRegs; stats->kernel_lds_bytes = (int)fattr.sharedSizeBytes; }
    return MORT_OK;
}

/* d_segpx: as render_device_impl's, only the host-buffer form passes one */
int frame_device_impl(mort_ctx *c, const mort_camera *cam, const mort_cached_frame_params *p, const void *d_records, const void *d_depth, void *d_rgba,
                      void *d_accum, void *d_segpx, void *d_ends, void *d_lit, void *stream, mort_stats *stats) {
    if (!c) return MORT_ERR_INVALID;
    int st = frame_check(cam, p, d_records, d_depth, c->d_states, d_rgba, d_accum, d_segpx, d_ends, d_lit);
    if (st != MORT_OK) return st;
    if (!aligned16(d_records) || !aligned16(d_depth) || !aligned16(d_rgba) || !aligned16(d_accum) || !aligned16(d_segpx) || !aligned16(d_ends) ||
        !aligned16(d_lit))
        return MORT_ERR_INVALID;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    if (c->part.nranks != 1) return MORT_ERR_UNSUPPORTED;
    const int W = cam->image_width, H = cam->image_height;
    if (!c->d_states || c->rng_w != W || c->rng_h != H) return MORT_ERR_NO_RNG;
    if ((st = check_light(c, cam->light_obj_type, cam->light_obj_idx)) != MORT_OK) return st;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    /* a render still running on another stream uses the same states and counters */
    if (c->last_stream && c->last_stream != s) HIPCHK(c, hipStreamSynchronize(c->last_stream));
    c->last_stream = s;

    HIPCHK(c, hipMemsetAsync(c->d_counters, 0, 96 * sizeof(unsigned long long), s));
    if (stats) HIPCHK(c, hipEventRecord(c->ev0, s));
    const bool visible = (p->flags & MORT_CACHED_VISIBLE) != 0;
    kernel_ptr kernel;
    if (visible) {
        CachedFrameDirectArgs<true> a;
        query_args_device(c, a.f.q);
        frame_args(a, cam, p, d_records, d_depth, c->d_states, d_rgba, d_accum, d_segpx, d_ends, d_lit, c->d_counters);
        kernel = frame_launch(c, a, s);
    } else {
        CachedFrameDirectArgs<false> a;
        query_args_device(c, a.f.q);
        frame_args(a, cam, p, d_records, d_depth, c->d_states, d_rgba, d_accum, d_segpx, d_ends, d_lit, c->d_counters);
        kernel = frame_launch(c, a, s);
    }
    HIPCHK(c, hipGetLastError());
    if (!stats) return MORT_OK;
    HIPCHK(c, hipEventRecord(c->ev1, s));
    /* by value: a view collects them after its frame's one wait (c->defer_stats), as it does a render's */
    const bool tree = c->gen_ok, has_accum = d_accum != nullptr, has_ends = d_ends != nullptr, has_lit = d_lit != nullptr;
    const int sqrt_spp = cam->sqrt_spp;
    auto fill = [=](mort_stats *out) { return frame_stats(c, kernel, tree, visible, W, H, sqrt_spp, has_accum, has_ends, has_lit, out); };
    if (c->defer_stats) { c->pending_stats = fill; return MORT_OK; }
    return fill(stats);
}

template <bool VISIBLE>
struct FrameHostJob {
    CachedFrameDirectArgs<VISIBLE> d;
    bool tree;
    std::atomic<unsigned long long> segments{0}, draws{0};
};
template <bool VISIBLE>
void frame_host_row(void *p, int y) {
    FrameHostJob<VISIBLE> *j = (FrameHostJob<VISIBLE> *)p;
    unsigned short walk[MORT_OWN_STACK];
    float4 first_levels[MORT_RADIANCE_LDS_LEVELS]; /* the kernel's LDS levels: the host runs the same seam */
    unsigned long long seg = 0, drw = 0;
    for (int x = 0; x < j->d.f.width; x++) {
        const PixelTotals t = j->tree ? cached_frame_direct_pixel<true, VISIBLE>(j->d, x, y, walk, 1, first_levels, MORT_RADIANCE_LDS_LEVELS, 1)
                                      : cached_frame_direct_pixel<false, VISIBLE>(j->d, x, y, walk, 1, first_levels, MORT_RADIANCE_LDS_LEVELS, 1);
        seg += t.segments; drw += t.draws;
    }
    j->segments += seg; j->draws += drw;
}

template <bool VISIBLE>
void frame_host_run(const SceneBlob &sb, bool tree, const mort_camera *cam, const mort_cached_frame_params *p, const float *records, const float *depth,
                    mort_rng_state *states, int nthreads, uint8_t *rgba, float *accum, uint32_t *segpx, uint32_t *ends, uint32_t *lit,
                    unsigned long long *totals) {
    FrameHostJob<VISIBLE> job;
    job.tree = tree;
    query_args_host(sb, tree, job.d.f.q);
    frame_args(job.d, cam, p, records, depth, states, rgba, accum, segpx, ends, lit, nullptr);
    run_rows(cam->image_height, nthreads, frame_host_row<VISIBLE>, &job);
    totals[0] = job.segments; totals[1] = job.draws;
}

} // namespace

extern "C" int mort_hip_render_cached_direct_device(mort_ctx *c, const mort_camera *cam, const mort_cached_frame_params *p, const void *d_records,
                                                    const void *d_depth, void *d_rgba, void *d_accum, void *d_ends, void *d_lit, void *stream,
                                                    mort_stats *stats) {
    return frame_device_impl(c, cam, p, d_records, d_depth, d_rgba, d_accum, nullptr, d_ends, d_lit, stream, stats);
}

/* the host-buffer form: records and maps up, the frame on the context's stream, the image, accumulators and counts down */
extern "C" int mort_hip_render_cached_direct(mort_ctx *c, const mort_camera *cam, const mort_cached_frame_params *p, const float *records,
                                             const float *depth, uint8_t *rgba_out, float *accum_out, uint32_t *segments_px_out, uint32_t *ends_px_out,
                                             uint32_t *lit_px_out, mort_stats *stats) {
    if (!c) return MORT_ERR_INVALID;
    int st = frame_check(cam, p, records, depth, nullptr, rgba_out, accum_out, segments_px_out, ends_px_out, lit_px_out);
    if (st != MORT_OK) return st;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    if (c->part.nranks != 1) return MORT_ERR_UNSUPPORTED;
    const int W = cam->image_width, H = cam->image_height;
    if (!c->d_states || c->rng_w != W || c->rng_h != H) return MORT_ERR_NO_RNG;
    if ((st = check_light(c, cam->light_obj_type, cam->light_obj_idx)) != MORT_OK) return st;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, switch_stream(c, c->stream)); /* the staging buffer is the stages' */
    const size_t npx = (size_t)W * (size_t)H, probes = (size_t)p->grid.count[0] * (size_t)p->grid.count[1] * (size_t)p->grid.count[2];
    StagePlane pl[7] = {{records, nullptr, probes * kRecordBytes}, {depth, nullptr, probes * kDepthBytes}, {nullptr, rgba_out, npx * 4},
                        {nullptr, accum_out, npx * 12}, {nullptr, segments_px_out, npx * 4}, {nullptr, ends_px_out, npx * 4},
                        {nullptr, lit_px_out, npx * 4}};
    if ((st = stage_upload(c, pl, 7)) != MORT_OK) return st;
    mort_stats local;
    if ((st = frame_device_impl(c, cam, p, pl[0].dev, pl[1].dev, pl[2].dev, pl[3].dev, pl[4].dev, pl[5].dev, pl[6].dev, c->stream, &local)) != MORT_OK)
        return st;
    if (stats) *stats = local;
    return stage_download(c, pl, 7);
}

extern "C" int mort_hip_render_cached_direct_host(const mort_world *world, const mort_camera *cam, mort_rng_state *states, int nthreads, int flags,
                                                  const mort_cached_frame_params *p, const float *records, const float *depth, uint8_t *rgba_out,
                                                  float *accum_out, uint32_t *segments_px_out, uint32_t *ends_px_out, uint32_t *lit_px_out,
                                                  mort_stats *stats) {
    if (!world || !states) return MORT_ERR_INVALID;
    int st = frame_check(cam, p, records, depth, states, rgba_out, accum_out, segments_px_out, ends_px_out, lit_px_out);
    if (st != MORT_OK) return st;
    SceneBlob sb;
    if ((st = build_scene_blob(world, sb)) != MORT_OK) return st;
    if ((st = check_light_object(sb.comp, world->objs.num_hittable_list, cam->light_obj_type, cam->light_obj_idx)) != MORT_OK) return st;
    const bool tree = (flags & MORT_HOST_TREE) && sb.comp.g_ok;
    const bool visible = (p->flags & MORT_CACHED_VISIBLE) != 0;
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 256) nthreads = 256;
    unsigned long long totals[2] = {0, 0};
    const double t0 = now_s();
    if (visible)
        frame_host_run<true>(sb, tree, cam, p, records, depth, states, nthreads, rgba_out, accum_out, segments_px_out, ends_px_out, lit_px_out, totals);
    else
        frame_host_run<false>(sb, tree, cam, p, records, depth, states, nthreads, rgba_out, accum_out, segments_px_out, ends_px_out, lit_px_out, totals);
    const double dt = now_s() - t0;
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->seconds = dt;
        stats->segments = totals[0]; stats->rng_draws = totals[1];
        stats->pixels = (uint64_t)cam->image_width * (uint64_t)cam->image_height;
        stats->eff_samples = stats->pixels * (uint64_t)(cam->sqrt_spp * cam->sqrt_spp);
        stats->local_rows = cam->image_height;
        std::snprintf(stats->kernel_name, sizeof stats->kernel_name, "host loop, cached frame, direct, %d thread(s), %s", nthreads,
                      tree ? "unified tree" : "item scan");
    }
    return MORT_OK;
}
