/*
 * depth.hip -- depth maps of light probes: for each probe an octahedral map, 8 x 8 texels and a one-texel border,
 * of the first two moments of the distance to the nearest solid, by the ray queries' own closest-hit search and the fixed
 * arithmetic of include/mort_hip.h.  The visibility-weighted sampler that reads the maps is in volume.hip.
 *
 * Kernel (gfx950, wave64, 256-thread groups, 1-D grid):
 *   probe_depth_kernel<TREE>  one wave per probe, four probes per group; a wave whose probe index is >= n returns as a whole.  One
 *                             lane per interior texel, lane = j * 8 + i.  The probe record is one wave-uniform 16-byte load.  A
 *                             lane runs its s x s rays one after the other (query_tree_solids<false> with its pending children in
 *                             LDS, 16 x 256 x 2 B, or query_items<false, false>; only t is needed, so nothing is resolved), keeps
 *                             m1 and m2 in two registers -- no cross-lane reduction, no barrier -- and stores its texel as one
 *                             8-byte store; the 28 lanes on an edge also store their one or two border copies, the four corner
 *                             lanes the diagonal one.
 *
 * The host form (mort_hip_probe_depth_bake_host) runs the same per-texel body (dev_depth.h) on host threads, one probe per work
 * item, and makes no HIP runtime call.  Nothing here reads or writes the render's pixel states, tile-cost cache or counters,
 * looks at the partition, or draws a random number.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "mort_hip.h"
#include "dev_depth.h"
#include "scene_blob.h"
#include "mort_ctx.h"
#include "mort_internal.h"
#include "stage_common.h"
#include "query_common.h"

#pragma clang fp contract(off)

/* ====================================================================== device */

constexpr int DEPTH_LANES = MORT_DEPTH_RES * MORT_DEPTH_RES; /* one wave */
constexpr int DEPTH_PROBES_PER_GROUP = QUERY_BLOCK / DEPTH_LANES;
static_assert(DEPTH_LANES == 64, "one wave64 per probe");

template <bool TREE>
__global__ void __launch_bounds__(QUERY_BLOCK) probe_depth_kernel(const DepthArgs a) {
    __shared__ unsigned short walk_stack[TREE ? MORT_OWN_STACK * QUERY_BLOCK : 1];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / DEPTH_LANES));
    const size_t p = (size_t)blockIdx.x * DEPTH_PROBES_PER_GROUP + (size_t)wave;
    if (p >= a.n) return; /* wave-uniform */
    const int lane = threadIdx.x & (DEPTH_LANES - 1);
    const int i = lane & (MORT_DEPTH_RES - 1), j = lane / MORT_DEPTH_RES;
    const mort_probe pr = a.probes[p]; /* wave-uniform: one 16-byte load */
    float m1, m2;
    depth_texel<TREE>(a, mk(pr.position[0], pr.position[1], pr.position[2]), pr.time, i, j, &walk_stack[TREE ? threadIdx.x : 0], QUERY_BLOCK, m1, m2);
    depth_store(a.depth + p * MORT_DEPTH_FLOATS, i + 1, j + 1, m1, m2);
}

/* ====================================================================== host */

namespace {

constexpr size_t kMaxDepthProbes = 0x7fffffff; /* a 1-D grid of groups of four probes stays far below the limit; the maps' bytes fit a size_t */

/* what the three forms check before they look at a world */
int depth_check(const mort_depth_params *p, size_t n, const void *probes, void *depth) {
    if (!p || !probes || !depth) return MORT_ERR_INVALID;
    if (p->subsamples < 1 || p->subsamples > MORT_DEPTH_RES) return MORT_ERR_INVALID;
    if (!std::isfinite(p->max_distance) || !(p->max_distance > 0.0f)) return MORT_ERR_INVALID;
    if (n > kMaxDepthProbes) return MORT_ERR_INVALID;
    const void *ins[1] = {probes};
    const size_t in_bytes[1] = {n * sizeof(mort_probe)};
    void *outs[1] = {depth};
    const size_t out_bytes[1] = {n * MORT_DEPTH_FLOATS * sizeof(float)};
    return buffers_disjoint(ins, in_bytes, 1, outs, out_bytes, 1) ? MORT_OK : MORT_ERR_INVALID;
}

void depth_args_params(DepthArgs &a, const mort_depth_params *p, size_t n, const void *probes, void *depth) {
    a.probes = (const mort_probe *)probes; a.n = n; a.depth = (float *)depth;
    a.s = p->subsamples;
    a.step = 2.0f / (float)(MORT_DEPTH_RES * p->subsamples);
    a.inv = 1.0f / (float)(p->subsamples * p->subsamples);
    a.max_distance = p->max_distance;
}

struct DepthHostJob { DepthArgs a; bool tree; };
void depth_host_probe(void *arg, int item) {
    const DepthHostJob *job = (const DepthHostJob *)arg;
    const DepthArgs &a = job->a;
    unsigned short walk[MORT_OWN_STACK];
    const size_t p = (size_t)item;
    const mort_probe pr = a.probes[p];
    const V3 origin = mk(pr.position[0], pr.position[1], pr.position[2]);
    for (int j = 0; j < MORT_DEPTH_RES; j++)
        for (int i = 0; i < MORT_DEPTH_RES; i++) {
            float m1, m2;
            if (job->tree) depth_texel<true>(a, origin, pr.time, i, j, walk, 1, m1, m2);
            else depth_texel<false>(a, origin, pr.time, i, j, walk, 1, m1, m2);
            depth_store(a.depth + p * MORT_DEPTH_FLOATS, i + 1, j + 1, m1, m2);
        }
}

} // namespace

extern "C" int mort_hip_probe_depth_bake_device(mort_ctx *c, const mort_depth_params *p, size_t n, const void *d_probes, void *d_depth_out,
                                                void *stream, double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    int st = depth_check(p, n, d_probes, d_depth_out);
    if (st != MORT_OK) return st;
    if (!aligned16(d_probes) || !aligned16(d_depth_out)) return MORT_ERR_INVALID;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    if (n == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    DepthArgs a;
    query_args_device(c, a.q);
    depth_args_params(a, p, n, d_probes, d_depth_out);
    hipStream_t s;
    if ((st = stage_begin(c, stream, 0, seconds, &s)) != MORT_OK) return st;
    const dim3 grid((unsigned)((n + DEPTH_PROBES_PER_GROUP - 1) / DEPTH_PROBES_PER_GROUP)), block(QUERY_BLOCK);
    if (c->gen_ok) hipLaunchKernelGGL(probe_depth_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(probe_depth_kernel<false>, grid, block, 0, s, a);
    HIPCHK(c, hipGetLastError());
    return stage_end(c, s, seconds);
}

/* the host-buffer form: probes up, the _device call on the context's stream, maps down */
extern "C" int mort_hip_probe_depth_bake(mort_ctx *c, const mort_depth_params *p, size_t n, const mort_probe *probes, float *depth_out,
                                         double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    int st = depth_check(p, n, probes, depth_out);
    if (st != MORT_OK) return st;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    if (n == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, switch_stream(c, c->stream));
    StagePlane pl[2] = {{probes, nullptr, n * sizeof(mort_probe)}, {nullptr, depth_out, n * MORT_DEPTH_FLOATS * sizeof(float)}};
    if ((st = stage_upload(c, pl, 2)) != MORT_OK) return st;
    double sec = 0;
    if ((st = mort_hip_probe_depth_bake_device(c, p, n, pl[0].dev, pl[1].dev, c->stream, &sec)) != MORT_OK) return st;
    if (seconds) *seconds = sec;
    return stage_download(c, pl, 2);
}

extern "C" int mort_hip_probe_depth_bake_host(const mort_world *world, const mort_depth_params *p, size_t n, const mort_probe *probes, int nthreads,
                                              int flags, float *depth_out, double *seconds) {
    if (!world) return MORT_ERR_INVALID;
    int st = depth_check(p, n, probes, depth_out);
    if (st != MORT_OK) return st;
    SceneBlob sb;
    if ((st = build_scene_blob(world, sb)) != MORT_OK) return st;
    if (seconds) *seconds = 0;
    if (n == 0) return MORT_OK;
    DepthHostJob job;
    job.tree = (flags & MORT_HOST_TREE) && sb.comp.g_ok;
    query_args_host(sb, job.tree, job.a.q);
    depth_args_params(job.a, p, n, probes, depth_out);
    const double t0 = now_s();
    run_rows((int)n, nthreads, depth_host_probe, &job);
    if (seconds) *seconds = now_s() - t0;
    return MORT_OK;
}
