/*
 * refresh.hip -- volume refresh: selected probes of an irradiance volume re-baked through the volume as it stands
 * and blended into their records under a hysteresis.  A probe's rays are the bake's (probe.hip), its paths the cached queries'
 * (cached.hip) over the records the call reads, its projection the bake's fixed sum, and the result goes into a second set of
 * records: light is carried one bounce further per round, at the price of a cached query per direction.
 *
 * Kernel (gfx950, wave64, one workgroup per selected probe, 1-D grid):
 *   probe_refresh_kernel<TREE, VISIBLE, BLOCK>   probe_sh_kernel's shape with cached_paths as the body.  The group's probe is
 *                                 first + blockIdx.x * step; its weight is one scalar load, and a masked probe (weight not > 0)
 *                                 is copied by 32 lanes and the group returns -- the test is group-uniform and comes before any
 *                                 barrier.  The position is computed from the index in scalar registers; the volume rides by value
 *                                 in the arguments.  One lane per direction of a batch of 64, wave w takes batches w, w + waves,
 *                                 ...; the 27 terms and the lane's count of paths that ended in the volume go through the
 *                                 xor-butterfly (the count as an integer) and lane 0 writes the batch's sums to LDS.  After the
 *                                 barrier 32 lanes add the batches in ascending order and write the record as one 128-byte row:
 *                                 27 blended floats, the weight, four zeros; lane 0 also writes the probe's count.
 *                                 BLOCK = min(D, 256), as the bake.  Every form keeps the three waves per SIMD of the cached
 *                                 queries without a spill; the <true, true, *> forms do so at exactly 168 registers, the last
 *                                 count that allows three (left to itself the compiler takes 169).
 *
 * The host form (mort_hip_volume_refresh_host) runs the same per-direction body and blend (dev_refresh.h) on host threads, one probe
 * per work item, with the bake's tree over a local array; it makes no HIP runtime call.  Nothing here reads or writes the render's
 * pixel states, tile-cost cache or counters, or looks at the partition.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "mort_hip.h"
#include "dev_refresh.h"
#include "scene_blob.h"
#include "mort_ctx.h"
#include "mort_internal.h"
#include "stage_common.h"
#include "query_common.h"

#pragma clang fp contract(off)

/* ====================================================================== device */

/* 3 waves per SIMD, as the cached queries and the bake: the resource check of the build holds these kernels to the radiance rule */
template <bool TREE, bool VISIBLE, int BLOCK>
__global__ void __launch_bounds__(BLOCK, 3) probe_refresh_kernel(const RefreshArgs<VISIBLE> a) {
    constexpr int WAVES = BLOCK / MORT_PROBE_BATCH;
    constexpr int MAX_BATCHES = BLOCK == QUERY_BLOCK ? MORT_PROBE_MAX_BATCHES : WAVES; /* a smaller group is launched for D == BLOCK only */
    __shared__ unsigned short walk_stack[TREE ? MORT_OWN_STACK * BLOCK : 1];
    __shared__ float4 bounce_stack[MORT_RADIANCE_LDS_LEVELS * BLOCK];
    __shared__ float batch_sum[MAX_BATCHES * MORT_SH9_FLOATS];
    __shared__ uint32_t batch_ends[MAX_BATCHES];
    const size_t p = (size_t)a.first + (size_t)blockIdx.x * (size_t)a.step; /* group-uniform */
    const float *records_in = refresh_records(a.c.vol.v);
    const volume_word *old_record = (const volume_word *)records_in + p * MORT_VOLUME_RECORD_FLOATS;
    volume_word *new_record = a.out + p * MORT_VOLUME_RECORD_FLOATS;

    if (refresh_masked(records_in, p)) { /* the whole group leaves: no barrier is waited for */
        if (threadIdx.x < MORT_VOLUME_RECORD_FLOATS) new_record[threadIdx.x] = old_record[threadIdx.x];
        if (threadIdx.x == 0 && a.ends) a.ends[p] = 0u;
        return;
    }

    const int lane = threadIdx.x & (MORT_PROBE_BATCH - 1), wave = threadIdx.x / MORT_PROBE_BATCH;
    const int batches = a.directions / MORT_PROBE_BATCH;
    const mort_volume_grid &g = refresh_grid(a.c.vol.v);
    const V3 origin = refresh_position(g, p);

    for (int b = wave; b < batches; b += WAVES) {
        float term[MORT_SH9_FLOATS];
        uint32_t ends;
        refresh_direction<TREE, VISIBLE>(a, p, origin, g.time, b * MORT_PROBE_BATCH + lane, &walk_stack[TREE ? threadIdx.x : 0], BLOCK,
                                         bounce_stack + threadIdx.x, MORT_RADIANCE_LDS_LEVELS, BLOCK, term, ends);
        /* every lane of the wave is here: b is wave-uniform and the batch is full */
#pragma unroll
        for (int m = 1; m < MORT_PROBE_BATCH; m <<= 1) ends = ends + (uint32_t)__shfl_xor((int)ends, m, MORT_PROBE_BATCH);
        if (lane == 0) batch_ends[b] = ends;
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
        if (i == 0 && a.ends) {
            uint32_t e = 0u;
            for (int b = 0; b < batches; b++) e += batch_ends[b];
            a.ends[p] = e;
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

/* what the three forms check before they look at a world: the bake's checks of D and the samples, the cached calls' of their fields,
 * then the new fields, the sizes and the overlaps */
int refresh_check(const mort_refresh_params *p, size_t m, const void *dirs, void *states, const void *records_in, const void *depth, void *records_out,
                  void *ends) {
    if (!p || !states || !records_in || !records_out) return MORT_ERR_INVALID;
    if (!directions_ok(p->directions) || p->cached.path.samples < 1) return MORT_ERR_INVALID;
    if (!mort_cached_volume_ok(p->cached.cache_depth, p->cached.flags, &p->cached.grid, &p->cached.vis, records_in, depth)) return MORT_ERR_INVALID;
    if (!(p->hysteresis >= 0.0f) || !(p->hysteresis < 1.0f)) return MORT_ERR_INVALID; /* a NaN fails the first test */
    const size_t P = refresh_probes(p), D = (size_t)p->directions;
    if (p->step == 0) return MORT_ERR_INVALID;
    if (m > 0 && ((size_t)p->first >= P || m - 1 > (P - 1 - (size_t)p->first) / (size_t)p->step)) return MORT_ERR_INVALID;
    if (P > kMaxRays / D) return MORT_ERR_INVALID;
    /* an in-place refresh is refused: the paths of one probe would read records that another group is writing */
    const void *ins[3] = {dirs, records_in, depth};
    const size_t in_bytes[3] = {3 * D * sizeof(float), P * kRecordBytes, P * kDepthBytes};
    void *outs[3] = {states, records_out, ends};
    const size_t out_bytes[3] = {P * D * sizeof(mort_rng_state), P * kRecordBytes, P * sizeof(uint32_t)};
    if (!buffers_disjoint(ins, in_bytes, 3, outs, out_bytes, 3)) return MORT_ERR_INVALID;
    if (p->cached.path.bounce_limit < 0 || p->cached.path.bounce_limit > MORT_MAX_BOUNCE_LIMIT) return MORT_ERR_CAPACITY;
    return MORT_OK;
}

/* everything of the arguments but the scene (a.c.r.q: query_args_device / query_args_host come first, they clear it) */
template <bool VISIBLE>
void refresh_args(RefreshArgs<VISIBLE> &a, const mort_refresh_params *p, const void *dirs, void *states, const void *records_in, const void *depth,
                  void *records_out, void *ends) {
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
}

template <bool TREE, bool VISIBLE>
void refresh_launch_tree(const RefreshArgs<VISIBLE> &a, size_t m, hipStream_t s) {
    const dim3 grid((unsigned)m);
    switch (a.directions < QUERY_BLOCK ? a.directions : QUERY_BLOCK) {
    case 64: hipLaunchKernelGGL((probe_refresh_kernel<TREE, VISIBLE, 64>), grid, dim3(64), 0, s, a); break;
    case 128: hipLaunchKernelGGL((probe_refresh_kernel<TREE, VISIBLE, 128>), grid, dim3(128), 0, s, a); break;
    case 192: hipLaunchKernelGGL((probe_refresh_kernel<TREE, VISIBLE, 192>), grid, dim3(192), 0, s, a); break;
    default: hipLaunchKernelGGL((probe_refresh_kernel<TREE, VISIBLE, QUERY_BLOCK>), grid, dim3(QUERY_BLOCK), 0, s, a); break;
    }
}

template <bool VISIBLE>
void refresh_launch(const mort_ctx *c, const mort_refresh_params *p, size_t m, const void *dirs, void *states, const void *records_in, const void *depth,
                    void *records_out, void *ends, hipStream_t s) {
    RefreshArgs<VISIBLE> a;
    query_args_device(c, a.c.r.q);
    refresh_args(a, p, dirs, states, records_in, depth, records_out, ends);
    if (c->gen_ok) refresh_launch_tree<true, VISIBLE>(a, m, s);
    else refresh_launch_tree<false, VISIBLE>(a, m, s);
}

template <bool VISIBLE> struct RefreshHostJob { RefreshArgs<VISIBLE> a; bool tree; };
template <bool VISIBLE>
void refresh_host_probe(void *arg, int item) {
    const RefreshHostJob<VISIBLE> *j = (const RefreshHostJob<VISIBLE> *)arg;
    const RefreshArgs<VISIBLE> &a = j->a;
    const size_t p = (size_t)a.first + (size_t)item * (size_t)a.step;
    const float *records_in = refresh_records(a.c.vol.v);
    const volume_word *old_record = (const volume_word *)records_in + p * MORT_VOLUME_RECORD_FLOATS;
    volume_word *new_record = a.out + p * MORT_VOLUME_RECORD_FLOATS;
    if (refresh_masked(records_in, p)) {
        for (int i = 0; i < MORT_VOLUME_RECORD_FLOATS; i++) new_record[i] = old_record[i];
        if (a.ends) a.ends[p] = 0u;
        return;
    }
    unsigned short walk[MORT_OWN_STACK];
    float4 first_levels[MORT_RADIANCE_LDS_LEVELS]; /* the kernel's LDS levels: the host runs the same seam */
    const mort_volume_grid &g = refresh_grid(a.c.vol.v);
    const V3 origin = refresh_position(g, p);
    float acc[MORT_SH9_FLOATS];
    float terms[MORT_SH9_FLOATS][MORT_PROBE_BATCH];
    uint32_t total = 0u;
    for (int b = 0; b < a.directions / MORT_PROBE_BATCH; b++) {
        for (int lane = 0; lane < MORT_PROBE_BATCH; lane++) {
            float term[MORT_SH9_FLOATS];
            uint32_t ends;
            const int d = b * MORT_PROBE_BATCH + lane;
            if (j->tree) refresh_direction<true, VISIBLE>(a, p, origin, g.time, d, walk, 1, first_levels, MORT_RADIANCE_LDS_LEVELS, 1, term, ends);
            else refresh_direction<false, VISIBLE>(a, p, origin, g.time, d, walk, 1, first_levels, MORT_RADIANCE_LDS_LEVELS, 1, term, ends);
            for (int k = 0; k < MORT_SH9_FLOATS; k++) terms[k][lane] = term[k];
            total += ends;
        }
        for (int k = 0; k < MORT_SH9_FLOATS; k++) {
            const float sum = probe_tree64(terms[k]);
            acc[k] = b ? acc[k] + sum : sum; /* batch 0's sum: no leading 0 + */
        }
    }
    for (int i = 0; i < MORT_VOLUME_RECORD_FLOATS; i++)
        new_record[i] = refresh_word(i, old_record, i < MORT_SH9_FLOATS ? acc[i] : 0.0f, a.scale, a.h, a.om);
    if (a.ends) a.ends[p] = total;
}

template <bool VISIBLE>
void refresh_host_run(const SceneBlob &sb, bool tree, const mort_refresh_params *p, size_t m, const float *dirs, mort_rng_state *states,
                      const float *records_in, const float *depth, int nthreads, float *records_out, uint32_t *ends) {
    RefreshHostJob<VISIBLE> job;
    job.tree = tree;
    query_args_host(sb, tree, job.a.c.r.q);
    refresh_args(job.a, p, dirs, states, records_in, depth, records_out, ends);
    run_rows((int)m, nthreads, refresh_host_probe<VISIBLE>, &job);
}

/* direction j of the library's D-point set in double, before it is rounded (mort_hip_probe_directions rounds exactly these) */
void fibonacci_double(int D, int j, double v[3]) {
    const double golden = M_PI * (3.0 - std::sqrt(5.0));
    const double z = 1.0 - (2.0 * (double)j + 1.0) / (double)D;
    const double r = std::sqrt(1.0 - z * z);
    const double phi = (double)j * golden;
    v[0] = r * std::cos(phi); v[1] = r * std::sin(phi); v[2] = z;
}

} // namespace

extern "C" int mort_hip_probe_directions_round(int directions, uint32_t round, float *dirs_out) {
    if (!dirs_out || !directions_ok(directions)) return MORT_ERR_INVALID;
    if (round == 0) return mort_hip_probe_directions(directions, dirs_out);
    double k[3];
    fibonacci_double(MORT_PROBE_BATCH, (int)(round % MORT_PROBE_BATCH), k);
    const double theta = (double)round * (M_PI * (3.0 - std::sqrt(5.0)));
    const double c = std::cos(theta), s = std::sin(theta), t = 1.0 - c;
    const double R[3][3] = {{c + (t * k[0]) * k[0], (t * k[0]) * k[1] - s * k[2], (t * k[0]) * k[2] + s * k[1]},
                            {(t * k[0]) * k[1] + s * k[2], c + (t * k[1]) * k[1], (t * k[1]) * k[2] - s * k[0]},
                            {(t * k[0]) * k[2] - s * k[1], (t * k[1]) * k[2] + s * k[0], c + (t * k[2]) * k[2]}};
    for (int j = 0; j < directions; j++) {
        double v[3];
        fibonacci_double(directions, j, v);
        for (int a = 0; a < 3; a++) dirs_out[3 * j + a] = (float)((R[a][0] * v[0] + R[a][1] * v[1]) + R[a][2] * v[2]);
    }
    return MORT_OK;
}

extern "C" int mort_hip_volume_refresh_device(mort_ctx *c, const mort_refresh_params *p, size_t m, const void *d_dirs, void *d_states,
                                              const void *d_records_in, const void *d_depth, void *d_records_out, void *d_ends_out, void *stream,
                                              double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    int st = refresh_check(p, m, d_dirs, d_states, d_records_in, d_depth, d_records_out, d_ends_out);
    if (st != MORT_OK) return st;
    if (!aligned16(d_dirs) || !aligned16(d_states) || !aligned16(d_records_in) || !aligned16(d_depth) || !aligned16(d_records_out) ||
        !aligned16(d_ends_out))
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
    if (p->cached.flags & MORT_CACHED_VISIBLE) refresh_launch<true>(c, p, m, d_dirs, d_states, d_records_in, d_depth, d_records_out, d_ends_out, s);
    else refresh_launch<false>(c, p, m, d_dirs, d_states, d_records_in, d_depth, d_records_out, d_ends_out, s);
    HIPCHK(c, hipGetLastError());
    return stage_end(c, s, seconds);
}

/* the host-buffer form: directions, streams, both sets of records and the maps up (records_out too: the call writes the selected
 * records only, the others go back as they came), the _device call on the context's stream, records, streams and counts down */
extern "C" int mort_hip_volume_refresh(mort_ctx *c, const mort_refresh_params *p, size_t m, const float *dirs, mort_rng_state *states,
                                       const float *records_in, const float *depth, float *records_out, uint32_t *ends_out, double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    int st = refresh_check(p, m, dirs, states, records_in, depth, records_out, ends_out);
    if (st != MORT_OK) return st;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    if ((st = check_light(c, p->cached.path.light_obj_type, p->cached.path.light_obj_idx)) != MORT_OK) return st;
    if (m == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, switch_stream(c, c->stream));
    const size_t P = refresh_probes(p), D = (size_t)p->directions;
    StagePlane pl[6] = {{dirs, nullptr, 3 * D * sizeof(float)}, {states, states, P * D * sizeof(mort_rng_state)}, {records_in, nullptr, P * kRecordBytes},
                        {depth, nullptr, P * kDepthBytes}, {records_out, records_out, P * kRecordBytes}, {ends_out, ends_out, P * sizeof(uint32_t)}};
    if ((st = stage_upload(c, pl, 6)) != MORT_OK) return st;
    double sec = 0;
    if ((st = mort_hip_volume_refresh_device(c, p, m, pl[0].dev, pl[1].dev, pl[2].dev, pl[3].dev, pl[4].dev, pl[5].dev, c->stream, &sec)) != MORT_OK)
        return st;
    if (seconds) *seconds = sec;
    return stage_download(c, pl, 6);
}

extern "C" int mort_hip_volume_refresh_host(const mort_world *world, const mort_refresh_params *p, size_t m, const float *dirs, mort_rng_state *states,
                                            const float *records_in, const float *depth, int nthreads, int flags, float *records_out,
                                            uint32_t *ends_out, double *seconds) {
    if (!world) return MORT_ERR_INVALID;
    int st = refresh_check(p, m, dirs, states, records_in, depth, records_out, ends_out);
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
    if (p->cached.flags & MORT_CACHED_VISIBLE) refresh_host_run<true>(sb, tree, p, m, dirs, states, records_in, depth, nthreads, records_out, ends_out);
    else refresh_host_run<false>(sb, tree, p, m, dirs, states, records_in, depth, nthreads, records_out, ends_out);
    if (seconds) *seconds = now_s() - t0;
    return MORT_OK;
}
