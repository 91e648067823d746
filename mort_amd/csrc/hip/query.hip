/*
 * query.hip -- ray queries: closest hit and occlusion for batches of the caller's rays, answered by the
 * render's own traversal.
 *
 * Kernels (gfx950, wave64, 256-thread groups, one lane per ray, 1-D grid):
 *   query_closest_kernel<TREE, MEDIA>   world::hit(ray, interval(0.001, t_max), rec): a ray as two 16-byte loads, the record
 *                                       as three 16-byte stores.  TREE: the unified-tree walk with its pending children in LDS
 *                                       (16 x 256 x 2 B) for origins within the tree's reach, the scan for the others and for
 *                                       the rays the walk flags; else world::hit's item loop (the threaded reference walk for
 *                                       BVH worlds).  MEDIA: the caller gave streams -- media are evaluated and the lane's
 *                                       stream is loaded and stored; without it they are passed over.
 *   query_occluded_kernel<TREE>         is a solid hit in [0.001, t_max]: one byte per ray, the walk stops at its first hit
 *
 * The host forms (mort_hip_query_*_host) run the same per-ray bodies (dev_query.h) on host threads and make no HIP runtime
 * call.  Nothing here reads or writes the render's pixel states, tile-cost cache or counters, or looks at the partition.  The
 * _device entry points' prologue and timed epilogue and the staging of the host-buffer forms are stage_common.h's.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "mort_hip.h"
#include "dev_query.h"
#include "scene_blob.h"
#include "mort_ctx.h"
#include "mort_internal.h"
#include "stage_common.h"
#include "query_common.h"

#pragma clang fp contract(off)

/* ====================================================================== device */

template <bool TREE, bool MEDIA>
__global__ void __launch_bounds__(QUERY_BLOCK) query_closest_kernel(const QueryArgs a) {
    __shared__ unsigned short query_stack[MORT_OWN_STACK * QUERY_BLOCK];
    const size_t i = (size_t)blockIdx.x * QUERY_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    query_closest_ray<TREE, MEDIA>(a, i, &query_stack[threadIdx.x], QUERY_BLOCK);
}

template <bool TREE>
__global__ void __launch_bounds__(QUERY_BLOCK) query_occluded_kernel(const QueryArgs a) {
    __shared__ unsigned short query_stack[MORT_OWN_STACK * QUERY_BLOCK];
    const size_t i = (size_t)blockIdx.x * QUERY_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    query_occluded_ray<TREE>(a, i, &query_stack[threadIdx.x], QUERY_BLOCK);
}

/* ====================================================================== host */

namespace {

/* no output (the streams are one: they are written in place) overlaps the rays or another output */
bool query_buffers_ok(size_t n, const void *rays, void *states, void *hits, void *occ) {
    const void *ins[1] = {rays};
    const size_t in_bytes[1] = {n * sizeof(mort_ray)};
    void *outs[3] = {states, hits, occ};
    const size_t out_bytes[3] = {n * sizeof(mort_rng_state), n * sizeof(mort_hit), n};
    return buffers_disjoint(ins, in_bytes, 1, outs, out_bytes, 3);
}

struct QueryHostJob { QueryArgs a; bool tree, closest; };
void query_host_chunk(void *p, int chunk) {
    const QueryHostJob *j = (const QueryHostJob *)p;
    unsigned short stack[MORT_OWN_STACK];
    const size_t i0 = (size_t)chunk * kHostChunk, i1 = i0 + kHostChunk < j->a.n ? i0 + kHostChunk : j->a.n;
    const bool media = j->a.states != nullptr;
    for (size_t i = i0; i < i1; i++) {
        if (!j->closest) {
            if (j->tree) query_occluded_ray<true>(j->a, i, stack, 1);
            else query_occluded_ray<false>(j->a, i, stack, 1);
        } else if (j->tree) {
            if (media) query_closest_ray<true, true>(j->a, i, stack, 1);
            else query_closest_ray<true, false>(j->a, i, stack, 1);
        } else {
            if (media) query_closest_ray<false, true>(j->a, i, stack, 1);
            else query_closest_ray<false, false>(j->a, i, stack, 1);
        }
    }
}

int query_host(const mort_world *world, size_t n, const mort_ray *rays, mort_rng_state *states, int nthreads, int flags, mort_hit *hits,
               uint8_t *occ, double *seconds) {
    if (n > kMaxRays || !query_buffers_ok(n, rays, states, hits, occ)) return MORT_ERR_INVALID;
    if (seconds) *seconds = 0;
    if (n == 0) return MORT_OK;
    SceneBlob sb;
    const int st = build_scene_blob(world, sb);
    if (st != MORT_OK) return st;
    QueryHostJob job;
    job.tree = (flags & MORT_HOST_TREE) && sb.comp.g_ok;
    job.closest = hits != nullptr;
    query_args_host(sb, job.tree, job.a);
    job.a.n = n; job.a.rays = rays; job.a.states = states; job.a.hits = hits; job.a.occluded = occ;
    const double t0 = now_s();
    run_rows((int)((n + kHostChunk - 1) / kHostChunk), nthreads, query_host_chunk, &job);
    if (seconds) *seconds = now_s() - t0;
    return MORT_OK;
}

/* a _device entry point after its own null checks */
int query_device(mort_ctx *c, size_t n, const void *d_rays, void *d_states, void *d_hits, void *d_occ, void *stream, double *seconds) {
    if (n > kMaxRays || !aligned16(d_rays) || !aligned16(d_states) || !aligned16(d_hits)) return MORT_ERR_INVALID;
    if (!query_buffers_ok(n, d_rays, d_states, d_hits, d_occ)) return MORT_ERR_INVALID;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    if (n == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    QueryArgs a;
    query_args_device(c, a);
    a.n = n; a.rays = (const mort_ray *)d_rays; a.states = (mort_rng_state *)d_states; a.hits = (mort_hit *)d_hits; a.occluded = (uint8_t *)d_occ;
    hipStream_t s;
    const int st = stage_begin(c, stream, 0, seconds, &s);
    if (st != MORT_OK) return st;
    const dim3 grid((unsigned)((n + QUERY_BLOCK - 1) / QUERY_BLOCK)), block(QUERY_BLOCK);
    const bool tree = c->gen_ok, media = d_states != nullptr;
    if (!d_hits) {
        if (tree) hipLaunchKernelGGL(query_occluded_kernel<true>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(query_occluded_kernel<false>, grid, block, 0, s, a);
    } else if (tree) {
        if (media) hipLaunchKernelGGL((query_closest_kernel<true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((query_closest_kernel<true, false>), grid, block, 0, s, a);
    } else {
        if (media) hipLaunchKernelGGL((query_closest_kernel<false, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((query_closest_kernel<false, false>), grid, block, 0, s, a);
    }
    HIPCHK(c, hipGetLastError());
    return stage_end(c, s, seconds);
}

/* a host-buffer form: rays (and streams) up, the _device call on the context's stream, records or bytes (and streams) down */
int query_staged(mort_ctx *c, size_t n, const mort_ray *rays, mort_rng_state *states, mort_hit *hits, uint8_t *occ, double *seconds) {
    if (n > kMaxRays || !query_buffers_ok(n, rays, states, hits, occ)) return MORT_ERR_INVALID;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    if (n == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, switch_stream(c, c->stream));
    StagePlane pl[4] = {{rays, nullptr, n * sizeof(mort_ray)}, {states, states, n * sizeof(mort_rng_state)},
                        {nullptr, hits, n * sizeof(mort_hit)}, {nullptr, occ, n}};
    int st = stage_upload(c, pl, 4);
    if (st != MORT_OK) return st;
    double sec = 0;
    if ((st = query_device(c, n, pl[0].dev, pl[1].dev, pl[2].dev, pl[3].dev, c->stream, &sec)) != MORT_OK) return st;
    if (seconds) *seconds = sec;
    return stage_download(c, pl, 4);
}

} // namespace

extern "C" int mort_hip_query_closest_device(mort_ctx *c, size_t n, const void *d_rays, void *d_states, void *d_out, void *stream,
                                             double *seconds) {
    if (!c || !d_rays || !d_out) return MORT_ERR_INVALID;
    return query_device(c, n, d_rays, d_states, d_out, nullptr, stream, seconds);
}

extern "C" int mort_hip_query_occluded_device(mort_ctx *c, size_t n, const void *d_rays, void *d_out, void *stream, double *seconds) {
    if (!c || !d_rays || !d_out) return MORT_ERR_INVALID;
    return query_device(c, n, d_rays, nullptr, nullptr, d_out, stream, seconds);
}

extern "C" int mort_hip_query_closest(mort_ctx *c, size_t n, const mort_ray *rays, mort_rng_state *states, mort_hit *out, double *seconds) {
    if (!c || !rays || !out) return MORT_ERR_INVALID;
    return query_staged(c, n, rays, states, out, nullptr, seconds);
}

extern "C" int mort_hip_query_occluded(mort_ctx *c, size_t n, const mort_ray *rays, uint8_t *out, double *seconds) {
    if (!c || !rays || !out) return MORT_ERR_INVALID;
    return query_staged(c, n, rays, nullptr, nullptr, out, seconds);
}

extern "C" int mort_hip_query_closest_host(const mort_world *world, size_t n, const mort_ray *rays, mort_rng_state *states, int nthreads,
                                           int flags, mort_hit *out, double *seconds) {
    if (!world || !rays || !out) return MORT_ERR_INVALID;
    return query_host(world, n, rays, states, nthreads, flags, out, nullptr, seconds);
}

extern "C" int mort_hip_query_occluded_host(const mort_world *world, size_t n, const mort_ray *rays, int nthreads, int flags, uint8_t *out,
                                            double *seconds) {
    if (!world || !rays || !out) return MORT_ERR_INVALID;
    return query_host(world, n, rays, nullptr, nthreads, flags, nullptr, out, seconds);
}
