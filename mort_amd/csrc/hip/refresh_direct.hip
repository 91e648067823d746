/*
 * refresh_direct.hip -- direct-light volume refresh: the volume refresh (refresh.hip) for a volume that holds
 * INDIRECT light only.  A probe's paths are the direct cached query's (cached_direct.hip): a path that ends in the volume adds one
 * sampled shadow segment toward the light object, so the surfaces a probe sees are lit as the frames light them; and a path whose
 * primary segment ends on an emitter counts as 0 (rule E), so the light a probe sees directly stays out of its record.
 *
 * Kernel (gfx950, wave64, one workgroup per selected probe, 1-D grid):
 *   probe_refresh_direct_kernel<TREE, VISIBLE, BLOCK>   probe_refresh_kernel's shape: the masked-probe exit before any barrier, wave w
 *                                 takes batches w, w + waves, ..., the 27 terms and BOTH counts go through the xor-butterfly and
 *                                 lane 0 writes the batch's sums to LDS; 32 lanes add the batches and write the 128-byte row
 *                                 through refresh_word, lane 0 the two counts.  The shadow segment is one more turn of the path
 *                                 loop, so the kernel holds one copy of the tree walk.  The scan forms are compiled for three waves
 *                                 per SIMD, the tree forms for two, as the direct cached queries (held to three they spill).
 *
 * The host form (mort_hip_volume_refresh_direct_host) runs the same per-direction body (dev_refresh_direct.h) on host threads, one
 * probe per work item; it makes no HIP runtime call.  Nothing here reads or writes the render's pixel states, tile-cost cache or
 * counters, or looks at the partition.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "mort_hip.h"
#include "dev_refresh_direct.h"
#include "scene_blob.h"
#include "mort_ctx.h"
#include "mort_internal.h"
#include "stage_common.h"
#include "query_common.h"

#pragma clang fp contract(off)

/* ====================================================================== device */

/* waves per SIMD: the light sample and the pending terminal do not fit the tree forms' 168 registers (DESIGN.md 4.24 has the table) */
#ifdef MORT_REFRESH_DIRECT_WAVES
#define REFRESH_DIRECT_WAVES(TREE) MORT_REFRESH_DIRECT_WAVES
#else
#define REFRESH_DIRECT_WAVES(TREE) ((TREE) ? 2 : 3)
#endif
template <bool TREE, bool VISIBLE, int BLOCK>
__global__ void __launch_bounds__(BLOCK, REFRESH_DIRECT_WAVES(TREE)) probe_refresh_direct_kernel(const RefreshDirectArgs<VISIBLE> da) {
    constexpr int WAVES = BLOCK / MORT_PROBE_BATCH;
    constexpr int MAX_BATCHES = BLOCK == QUERY_BLOCK ? MORT_PROBE_MAX_BATCHES : WAVES; /* a smaller group is launched for D == BLOCK only */
    __shared__ unsigned short walk_stack[TREE ? MORT_OWN_STACK * BLOCK : 1];
    __shared__ float4 bounce_stack[MORT_RADIANCE_LDS_LEVELS * BLOCK];
    __shared__ float batch_sum[MAX_BATCHES * MORT_SH9_FLOATS];
    __shared__ uint32_t batch_ends[MAX_BATCHES];
    __shared__ uint32_t batch_lit[MAX_BATCHES];
    const RefreshArgs<VISIBLE> &a = da.r;
    const size_t p = (size_t)a.first + (size_t)blockIdx.x * (size_t)a.step; /* group-uniform */
    const float *records_in = refresh_records(a.c.vol.v);
    const volume_word *old_record = (const volume_word *)records_in + p * MORT_VOLUME_RECORD_FLOATS;
    volume_word *new_record = a.out + p * MORT_VOLUME_RECORD_FLOATS;

    if (refresh_masked(records_in, p)) { /* the whole group leaves: no barrier is waited for */
        if (threadIdx.x < MORT_VOLUME_RECORD_FLOATS) new_record[threadIdx.x] = old_record[threadIdx.x];
        if (threadIdx.x == 0 && a.ends) a.ends[p] = 0u;
        if (threadIdx.x == 0 && da.lit) da.lit[p] = 0u;
        return;
    }

    const int lane = threadIdx.x & (MORT_PROBE_BATCH - 1), wave = threadIdx.x / MORT_PROBE_BATCH;
    const int batches = a.directions / MORT_PROBE_BATCH;
    const mort_volume_grid &g = refresh_grid(a.c.vol.v);
    const V3 origin = refresh_position(g, p);

    for (int b = wave; b < batches; b += WAVES) {
        float term[MORT_SH9_FLOATS];
        uint32_t ends, lit;
        refresh_direct_direction<TREE, VISIBLE>(a, p, origin, g.time, b * MORT_PROBE_BATCH + lane, &walk_stack[TREE ? threadIdx.x : 0], BLOCK,
                                                bounce_stack + threadIdx.x, MORT_RADIANCE_LDS_LEVELS, BLOCK, term, ends, lit);
        /* every lane of the wave is here: b is wave-uniform and the batch is full */
#pragma unroll
        for (int m = 1; m < MORT_PROBE_BATCH; m <<= 1) {
            ends = ends + (uint32_t)__shfl_xor((int)ends, m, MORT_PROBE_BATCH);
            lit = lit + (uint32_t)__shfl_xor((int)lit, m, MORT_PROBE_BATCH);
        }
        if (lane == 0) { batch_ends[b] = ends; batch_lit[b] = lit; }
#pragma unroll
        for (int k = 0; k < MORT_SH9_FLOATS; k++) {
            float v = term[k];
#pragma unroll
            for (int m = 1; m < MORT_PROBE_BATCH; m <<= 1) v = v + __shfl_xor(v, m, MORT_PROBE_BATCH);
            if (lane == 0) batch_sum[b * MORT_SH9_FLOATS + k] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x < MORT_VOLUME_RECORD_FLOATS) {
        const int i = threadIdx.x;
        float acc = 0.0f;
        if (i < MORT_SH9_FLOATS) {
            acc = batch_sum[i]; /* batch 0's sum: no leading 0 + */
            for (int b = 1; b < batches; b++) acc = acc + batch_sum[b * MORT_SH9_FLOATS + i];
        }
        new_record[i] = refresh_word(i, old_record, acc, a.scale, a.h, a.om);
        if (i == 0) {
            uint32_t e = 0u, l = 0u;
            for (int b = 0; b < batches; b++) { e += batch_ends[b]; l += batch_lit[b]; }
            if (a.ends) a.ends[p] = e;
            if (da.lit) da.lit[p] = l;
        }
    }
}

/* ====================================================================== host */

namespace {

constexpr size_t kRecordBytes = MORT_VOLUME_RECORD_FLOATS * sizeof(float);
constexpr size_t kDepthBytes = MORT_DEPTH_FLOATS * sizeof(float);

bool directions_ok(int d) { return d >= MORT_PROBE_BATCH && d <= MORT_PROBE_MAX_DIRECTIONS && d % MORT_PROBE_BATCH == 0; }

size_t refresh_probes(const mort_refresh_params *p) {
    return (size_t)p->cached.grid.count[0] * (size_t)p->cached.grid.count[1] * (size_t)p->cached.grid.count[2];
}

/* the plain refresh's checks in its order, with lit as one more output */
int refresh_direct_check(const mort_refresh_params *p, size_t m, const void *dirs, void *states, const void *records_in, const void *depth,
                         void *records_out, void *ends, void *lit) {
    if (!p || !states || !records_in || !records_out) return MORT_ERR_INVALID;
    if (!directions_ok(p->directions) || p->cached.path.samples < 1) return MORT_ERR_INVALID;
    if (!mort_cached_volume_ok(p->cached.cache_depth, p->cached.flags, &p->cached.grid, &p->cached.vis, records_in, depth)) return MORT_ERR_INVALID;
    if (!(p->hysteresis >= 0.0f) || !(p->hysteresis < 1.0f)) return MORT_ERR_INVALID; /* a NaN fails the first test */
    const size_t P = refresh_probes(p), D = (size_t)p->directions;
    if (p->step == 0) return MORT_ERR_INVALID;
    if (m > 0 && ((size_t)p->first >= P || m - 1 > (P - 1 - (size_t)p->first) / (size_t)p->step)) return MORT_ERR_INVALID;
    if (P > kMaxRays / D) return MORT_ERR_INVALID;
    const void *ins[3] = {dirs, records_in, depth};
    const size_t in_bytes[3] = {3 * D * sizeof(float), P * kRecordBytes, P * kDepthBytes};
    void *outs[4] = {states, records_out, ends, lit};
    const size_t out_bytes[4] = {P * D * sizeof(mort_rng_state), P * kRecordBytes, P * sizeof(uint32_t), P * sizeof(uint32_t)};
    if (!buffers_disjoint(ins, in_bytes, 3, outs, out_bytes, 4)) return MORT_ERR_INVALID;
    if (p->cached.path.bounce_limit < 0 || p->cached.path.bounce_limit > MORT_MAX_BOUNCE_LIMIT) return MORT_ERR_CAPACITY;
    return MORT_OK;
}

/* everything of the arguments but the scene (a.c.r.q: query_args_device / query_args_host come first, they clear it) */
template <bool VISIBLE>
void refresh_direct_args(RefreshDirectArgs<VISIBLE> &da, const mort_refresh_params *p, const void *dirs, void *states, const void *records_in,
                         const void *depth, void *records_out, void *ends, void *lit) {
    RefreshArgs<VISIBLE> &a = da.r;
    mort_radiance_args_params(a.c.r, &p->cached.path);
    a.c.r.q.n = refresh_probes(p); a.c.r.q.states = (mort_rng_state *)states; a.c.r.rgb = nullptr;
    a.c.cache_depth = p->cached.cache_depth; a.c.ends = nullptr;
    if constexpr (VISIBLE) mort_cached_volume(a.c.vol.v, p->cached.grid, p->cached.vis, records_in, depth);
    else mort_cached_volume(a.c.vol.v, p->cached.grid, records_in);
    a.dirs = (const float *)dirs; a.out = (volume_word *)records_out; a.ends = (uint32_t *)ends;
    a.directions = p->directions;
    a.scale = (float)(4.0 * M_PI / ((double)p->directions * (double)p->cached.path.samples));
    a.h = p->hysteresis; a.om = 1.0f - p->hysteresis;
    a.first = p->first; a.step = p->step;
    da.lit = (uint32_t *)lit;
}

template <bool TREE, bool VISIBLE>
void refresh_direct_launch_tree(const RefreshDirectArgs<VISIBLE> &a, size_t m, hipStream_t s) {
    const dim3 grid((unsigned)m);
    switch (a.r.directions < QUERY_BLOCK ? a.r.directions : QUERY_BLOCK) {
    case 64: hipLaunchKernelGGL((probe_refresh_direct_kernel<TREE, VISIBLE, 64>), grid, dim3(64), 0, s, a); break;
    case 128: hipLaunchKernelGGL((probe_refresh_direct_kernel<TREE, VISIBLE, 128>), grid, dim3(128), 0, s, a); break;
    case 192: hipLaunchKernelGGL((probe_refresh_direct_kernel<TREE, VISIBLE, 192>), grid, dim3(192), 0, s, a); break;
    default: hipLaunchKernelGGL((probe_refresh_direct_kernel<TREE, VISIBLE, QUERY_BLOCK>), grid, dim3(QUERY_BLOCK), 0, s, a); break;
    }
}

template <bool VISIBLE>
void refresh_direct_launch(const mort_ctx *c, const mort_refresh_params *p, size_t m, const void *dirs, void *states, const void *records_in,
                           const void *depth, void *records_out, void *ends, void *lit, hipStream_t s) {
    RefreshDirectArgs<VISIBLE> a;
    query_args_device(c, a.r.c.r.q);
    refresh_direct_args(a, p, dirs, states, records_in, depth, records_out, ends, lit);
    if (c->gen_ok) refresh_direct_launch_tree<true, VISIBLE>(a, m, s);
    else refresh_direct_launch_tree<false, VISIBLE>(a, m, s);
}

template <bool VISIBLE> struct RefreshDirectHostJob { RefreshDirectArgs<VISIBLE> a; bool tree; };
template <bool VISIBLE>
void refresh_direct_host_probe(void *arg, int item) {
    const RefreshDirectHostJob<VISIBLE> *j = (const RefreshDirectHostJob<VISIBLE> *)arg;
    const RefreshArgs<VISIBLE> &a = j->a.r;
    uint32_t *lit_out = j->a.lit;
    const size_t p = (size_t)a.first + (size_t)item * (size_t)a.step;
    const float *records_in = refresh_records(a.c.vol.v);
    const volume_word *old_record = (const volume_word *)records_in + p * MORT_VOLUME_RECORD_FLOATS;
    volume_word *new_record = a.out + p * MORT_VOLUME_RECORD_FLOATS;
    if (refresh_masked(records_in, p)) {
        for (int i = 0; i < MORT_VOLUME_RECORD_FLOATS; i++) new_record[i] = old_record[i];
        if (a.ends) a.ends[p] = 0u;
        if (lit_out) lit_out[p] = 0u;
        return;
    }
    unsigned short walk[MORT_OWN_STACK];
    float4 first_levels[MORT_RADIANCE_LDS_LEVELS]; /* the kernel's LDS levels: the host runs the same seam */
    const mort_volume_grid &g = refresh_grid(a.c.vol.v);
    const V3 origin = refresh_position(g, p);
    float acc[MORT_SH9_FLOATS];
    float terms[MORT_SH9_FLOATS][MORT_PROBE_BATCH];
    uint32_t total = 0u, total_lit = 0u;
    for (int b = 0; b < a.directions / MORT_PROBE_BATCH; b++) {
        for (int lane = 0; lane < MORT_PROBE_BATCH; lane++) {
            float term[MORT_SH9_FLOATS];
            uint32_t ends, lit;
            const int d = b * MORT_PROBE_BATCH + lane;
            if (j->tree) refresh_direct_direction<true, VISIBLE>(a, p, origin, g.time, d, walk, 1, first_levels, MORT_RADIANCE_LDS_LEVELS, 1, term, ends, lit);
            else refresh_direct_direction<false, VISIBLE>(a, p, origin, g.time, d, walk, 1, first_levels, MORT_RADIANCE_LDS_LEVELS, 1, term, ends, lit);
            for (int k = 0; k < MORT_SH9_FLOATS; k++) terms[k][lane] = term[k];
            total += ends; total_lit += lit;
        }
        for (int k = 0; k < MORT_SH9_FLOATS; k++) {
            const float sum = probe_tree64(terms[k]);
            acc[k] = b ? acc[k] + sum : sum; /* batch 0's sum: no leading 0 + */
        }
    }
    for (int i = 0; i < MORT_VOLUME_RECORD_FLOATS; i++)
        new_record[i] = refresh_word(i, old_record, i < MORT_SH9_FLOATS ? acc[i] : 0.0f, a.scale, a.h, a.om);
    if (a.ends) a.ends[p] = total;
    if (lit_out) lit_out[p] = total_lit;
}

template <bool VISIBLE>
void refresh_direct_host_run(const SceneBlob &sb, bool tree, const mort_refresh_params *p, size_t m, const float *dirs, mort_rng_state *states,
                             const float *records_in, const float *depth, int nthreads, float *records_out, uint32_t *ends, uint32_t *lit) {
    RefreshDirectHostJob<VISIBLE> job;
    job.tree = tree;
    query_args_host(sb, tree, job.a.r.c.r.q);
    refresh_direct_args(job.a, p, dirs, states, records_in, depth, records_out, ends, lit);
    run_rows((int)m, nthreads, refresh_direct_host_probe<VISIBLE>, &job);
}

} // namespace

extern "C" int mort_hip_volume_refresh_direct_device(mort_ctx *c, const mort_refresh_params *p, size_t m, const void *d_dirs, void *d_states,
                                                     const void *d_records_in, const void *d_depth, void *d_records_out, void *d_ends_out,
                                                     void *d_lit_out, void *stream, double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    int st = refresh_direct_check(p, m, d_dirs, d_states, d_records_in, d_depth, d_records_out, d_ends_out, d_lit_out);
    if (st != MORT_OK) return st;
    if (!aligned16(d_dirs) || !aligned16(d_states) || !aligned16(d_records_in) || !aligned16(d_depth) || !aligned16(d_records_out) ||
        !aligned16(d_ends_out) || !aligned16(d_lit_out))
        return MORT_ERR_INVALID;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    if ((st = check_light(c, p->cached.path.light_obj_type, p->cached.path.light_obj_idx)) != MORT_OK) return st;
    if (m == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    if (!d_dirs) { /* the library's set, before the clock starts */
        HIPCHK(c, hipSetDevice(c->device));
        const hipStream_t s0 = stream ? (hipStream_t)stream : c->stream;
        HIPCHK(c, switch_stream(c, s0));
        const float *own = nullptr;
        if ((st = mort_probe_own_directions(c, p->directions, s0, &own)) != MORT_OK) return st;
        d_dirs = own;
    }
    hipStream_t s;
    if ((st = stage_begin(c, stream, 0, seconds, &s)) != MORT_OK) return st;
    if (p->cached.flags & MORT_CACHED_VISIBLE)
        refresh_direct_launch<true>(c, p, m, d_dirs, d_states, d_records_in, d_depth, d_records_out, d_ends_out, d_lit_out, s);
    else refresh_direct_launch<false>(c, p, m, d_dirs, d_states, d_records_in, d_depth, d_records_out, d_ends_out, d_lit_out, s);
    HIPCHK(c, hipGetLastError());
    return stage_end(c, s, seconds);
}

/* the host-buffer form: the plain refresh's planes (records_out goes up as well) and lit as one more */
extern "C" int mort_hip_volume_refresh_direct(mort_ctx *c, const mort_refresh_params *p, size_t m, const float *dirs, mort_rng_state *states,
                                              const float *records_in, const float *depth, float *records_out, uint32_t *ends_out,
                                              uint32_t *lit_out, double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    int st = refresh_direct_check(p, m, dirs, states, records_in, depth, records_out, ends_out, lit_out);
    if (st != MORT_OK) return st;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    if ((st = check_light(c, p->cached.path.light_obj_type, p->cached.path.light_obj_idx)) != MORT_OK) return st;
    if (m == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, switch_stream(c, c->stream));
    const size_t P = refresh_probes(p), D = (size_t)p->directions;
    StagePlane pl[7] = {{dirs, nullptr, 3 * D * sizeof(float)}, {states, states, P * D * sizeof(mort_rng_state)}, {records_in, nullptr, P * kRecordBytes},
                        {depth, nullptr, P * kDepthBytes}, {records_out, records_out, P * kRecordBytes}, {ends_out, ends_out, P * sizeof(uint32_t)},
                        {lit_out, lit_out, P * sizeof(uint32_t)}};
    if ((st = stage_upload(c, pl, 7)) != MORT_OK) return st;
    double sec = 0;
    if ((st = mort_hip_volume_refresh_direct_device(c, p, m, pl[0].dev, pl[1].dev, pl[2].dev, pl[3].dev, pl[4].dev, pl[5].dev, pl[6].dev, c->stream,
                                                    &sec)) != MORT_OK)
        return st;
    if (seconds) *seconds = sec;
    return stage_download(c, pl, 7);
}

extern "C" int mort_hip_volume_refresh_direct_host(const mort_world *world, const mort_refresh_params *p, size_t m, const float *dirs,
                                                   mort_rng_state *states, const float *records_in, const float *depth, int nthreads, int flags,
                                                   float *records_out, uint32_t *ends_out, uint32_t *lit_out, double *seconds) {
    if (!world) return MORT_ERR_INVALID;
    int st = refresh_direct_check(p, m, dirs, states, records_in, depth, records_out, ends_out, lit_out);
    if (st != MORT_OK) return st;
    SceneBlob sb;
    if ((st = build_scene_blob(world, sb)) != MORT_OK) return st;
    if ((st = check_light_object(sb.comp, world->objs.num_hittable_list, p->cached.path.light_obj_type, p->cached.path.light_obj_idx)) != MORT_OK) return st;
    if (seconds) *seconds = 0;
    if (m == 0) return MORT_OK;
    std::vector<float> own;
    if (!dirs) { own.resize(3 * (size_t)p->directions); mort_hip_probe_directions(p->directions, own.data()); dirs = own.data(); }
    const bool tree = (flags & MORT_HOST_TREE) && sb.comp.g_ok;
    const double t0 = now_s();
    if (p->cached.flags & MORT_CACHED_VISIBLE)
        refresh_direct_host_run<true>(sb, tree, p, m, dirs, states, records_in, depth, nthreads, records_out, ends_out, lit_out);
    else refresh_direct_host_run<false>(sb, tree, p, m, dirs, states, records_in, depth, nthreads, records_out, ends_out, lit_out);
    if (seconds) *seconds = now_s() - t0;
    return MORT_OK;
}
