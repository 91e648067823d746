/*
 * probe.hip -- light probes: for each probe position the SH9 coefficients per colour channel of the path-traced
 * radiance arriving there, by the radiance queries' own path body (dev_radiance.h) and the fixed summation order of
 * include/mort_hip.h.
 *
 * Kernel (gfx950, wave64, one workgroup per probe, 1-D grid):
 *   probe_sh_kernel<TREE, BLOCK>  one lane per direction of a batch of 64; wave w of the group takes batches w, w + waves, ...
 *                                 Per batch a lane loads its stream (dwordx4 + dwordx2), builds its ray from the probe record
 *                                 and its direction, runs radiance_paths<TREE>, stores the stream, guards the sum and forms its
 *                                 27 terms; then the wave, all 64 lanes reconverged (every batch is full: D is a multiple of
 *                                 64, and no lane returns early), adds them with an xor-butterfly over lanes 1, 2, ... 32 --
 *                                 the contract's balanced tree, since fp32 addition commutes -- and lane 0 writes the batch's
 *                                 27 sums to LDS.  After the group's barrier 27 lanes add the batches in ascending order, scale
 *                                 and store the probe's 108 bytes.
 *                                 BLOCK = min(D, 256): a group has as many waves as the probe has batches, four at the most,
 *                                 and its LDS (the walk column for TREE, the first MORT_RADIANCE_LDS_LEVELS bounce-stack
 *                                 levels, the batch sums) is sized for them, so that probes of fewer than 256 directions still
 *                                 fill the three waves per SIMD the path body's registers allow (a 256-thread group of which
 *                                 one wave works would hold 47 KB of LDS and three register slots for it).
 *
 * The host form (mort_hip_probe_bake_host) runs the same per-direction body (dev_probe.h) on host threads, one probe per work
 * item, and the same tree over a local array; it makes no HIP runtime call.  Nothing here reads or writes the render's pixel
 * states, tile-cost cache or counters, or looks at the partition.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "mort_hip.h"
#include "dev_probe.h"
#include "scene_blob.h"
#include "mort_ctx.h"
#include "mort_internal.h"
#include "stage_common.h"
#include "query_common.h"

#pragma clang fp contract(off)

/* ====================================================================== device */

/* the radiance kernels' occupancy (radiance.hip): the path body takes 145 / 158 registers */
#ifndef MORT_RADIANCE_WAVES
#define MORT_RADIANCE_WAVES 3
#endif
template <bool TREE, int BLOCK>
__global__ void __launch_bounds__(BLOCK, MORT_RADIANCE_WAVES) probe_sh_kernel(const ProbeArgs a) {
    constexpr int WAVES = BLOCK / MORT_PROBE_BATCH;
    constexpr int MAX_BATCHES = BLOCK == QUERY_BLOCK ? MORT_PROBE_MAX_BATCHES : WAVES; /* a smaller group is launched for D == BLOCK only */
    __shared__ unsigned short walk_stack[TREE ? MORT_OWN_STACK * BLOCK : 1];
    __shared__ float4 bounce_stack[MORT_RADIANCE_LDS_LEVELS * BLOCK];
    __shared__ float batch_sum[MAX_BATCHES * MORT_SH9_FLOATS];
    const size_t p = blockIdx.x;
    const int lane = threadIdx.x & (MORT_PROBE_BATCH - 1), wave = threadIdx.x / MORT_PROBE_BATCH;
    const int batches = a.directions / MORT_PROBE_BATCH;
    const mort_probe pr = a.probes[p]; /* wave-uniform: one 16-byte load */
    const V3 origin = mk(pr.position[0], pr.position[1], pr.position[2]);

    for (int b = wave; b < batches; b += WAVES) {
        float term[MORT_SH9_FLOATS];
        probe_direction<TREE>(a, p, origin, pr.time, b * MORT_PROBE_BATCH + lane, &walk_stack[TREE ? threadIdx.x : 0], BLOCK, bounce_stack + threadIdx.x,
                              MORT_RADIANCE_LDS_LEVELS, BLOCK, term);
        /* every lane of the wave is here: b is wave-uniform and the batch is full */
#pragma unroll
        for (int k = 0; k < MORT_SH9_FLOATS; k++) {
            float v = term[k];
#pragma unroll
            for (int m = 1; m < MORT_PROBE_BATCH; m <<= 1) v = v + __shfl_xor(v, m, MORT_PROBE_BATCH);
            if (lane == 0) batch_sum[b * MORT_SH9_FLOATS + k] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x < MORT_SH9_FLOATS) {
        float acc = batch_sum[threadIdx.x]; /* batch 0's sum: no leading 0 + */
        for (int b = 1; b < batches; b++) acc = acc + batch_sum[b * MORT_SH9_FLOATS + threadIdx.x];
        a.sh[p * MORT_SH9_FLOATS + threadIdx.x] = a.scale * acc;
    }
}

/* ====================================================================== host */

namespace {

constexpr size_t kMaxProbes = 0x7fffffff; /* a 1-D grid of one group per probe */

bool directions_ok(int d) { return d >= MORT_PROBE_BATCH && d <= MORT_PROBE_MAX_DIRECTIONS && d % MORT_PROBE_BATCH == 0; }

/* the library's own set: the spherical Fibonacci points, in double, rounded once */
void fibonacci_directions(int D, float *out) {
    const double golden = M_PI * (3.0 - std::sqrt(5.0));
    for (int j = 0; j < D; j++) {
        const double z = 1.0 - (2.0 * (double)j + 1.0) / (double)D;
        const double r = std::sqrt(1.0 - z * z);
        const double phi = (double)j * golden;
        out[3 * j + 0] = (float)(r * std::cos(phi));
        out[3 * j + 1] = (float)(r * std::sin(phi));
        out[3 * j + 2] = (float)z;
    }
}

/* what the three forms check before they look at a world */
int probe_check(const mort_probe_params *p, size_t n, const void *probes, const void *dirs, void *states, void *sh) {
    if (!p || !probes || !states || !sh) return MORT_ERR_INVALID;
    if (!directions_ok(p->directions) || p->rp.samples < 1) return MORT_ERR_INVALID;
    const size_t D = (size_t)p->directions;
    if (n > kMaxRays / D || n > kMaxProbes) return MORT_ERR_INVALID;
    /* no output (the streams are one: they are advanced in place) overlaps an input or the other output */
    const void *ins[2] = {probes, dirs};
    const size_t in_bytes[2] = {n * sizeof(mort_probe), 3 * D * sizeof(float)};
    void *outs[2] = {states, sh};
    const size_t out_bytes[2] = {n * D * sizeof(mort_rng_state), n * MORT_SH9_FLOATS * sizeof(float)};
    if (!buffers_disjoint(ins, in_bytes, 2, outs, out_bytes, 2)) return MORT_ERR_INVALID;
    if (p->rp.bounce_limit < 0 || p->rp.bounce_limit > MORT_MAX_BOUNCE_LIMIT) return MORT_ERR_CAPACITY;
    return MORT_OK;
}

void probe_args_params(ProbeArgs &a, const mort_probe_params *p) {
    a.r.bounce_limit = p->rp.bounce_limit; a.r.samples = p->rp.samples;
    a.r.background = mk(p->rp.background[0], p->rp.background[1], p->rp.background[2]);
    a.r.light_type = p->rp.light_obj_type; a.r.light_idx = p->rp.light_obj_idx;
    a.r.rgb = nullptr;
    a.directions = p->directions;
    a.scale = (float)(4.0 * M_PI / ((double)p->directions * (double)p->rp.samples));
}

struct ProbeHostJob { ProbeArgs a; bool tree; };
void probe_host_probe(void *arg, int item) {
    const ProbeHostJob *j = (const ProbeHostJob *)arg;
    const ProbeArgs &a = j->a;
    unsigned short walk[MORT_OWN_STACK];
    float4 first_levels[MORT_RADIANCE_LDS_LEVELS]; /* the kernel's LDS levels: the host runs the same seam */
    const size_t p = (size_t)item;
    const mort_probe pr = a.probes[p];
    const V3 origin = mk(pr.position[0], pr.position[1], pr.position[2]);
    float acc[MORT_SH9_FLOATS];
    float terms[MORT_SH9_FLOATS][MORT_PROBE_BATCH];
    for (int b = 0; b < a.directions / MORT_PROBE_BATCH; b++) {
        for (int lane = 0; lane < MORT_PROBE_BATCH; lane++) {
            float term[MORT_SH9_FLOATS];
            const int d = b * MORT_PROBE_BATCH + lane;
            if (j->tree) probe_direction<true>(a, p, origin, pr.time, d, walk, 1, first_levels, MORT_RADIANCE_LDS_LEVELS, 1, term);
            else probe_direction<false>(a, p, origin, pr.time, d, walk, 1, first_levels, MORT_RADIANCE_LDS_LEVELS, 1, term);
            for (int k = 0; k < MORT_SH9_FLOATS; k++) terms[k][lane] = term[k];
        }
        for (int k = 0; k < MORT_SH9_FLOATS; k++) {
            const float sum = probe_tree64(terms[k]);
            acc[k] = b ? acc[k] + sum : sum; /* batch 0's sum: no leading 0 + */
        }
    }
    for (int k = 0; k < MORT_SH9_FLOATS; k++) a.sh[p * MORT_SH9_FLOATS + k] = a.scale * acc[k];
}

/* the context's copy of the library's own set for D directions, made when D changes */
int own_directions(mort_ctx *c, int D, hipStream_t s, const float **d_dirs) {
    if (c->probe_dirs_d != D) {
        int st = MORT_OK;
        HIPCHK(c, hipStreamSynchronize(s)); /* an earlier bake on this stream may still read the set it replaces */
        c->probe_dirs_d = 0;
        if ((st = ensure_buf(c, c->probe_dirs, (size_t)3 * D * sizeof(float))) != MORT_OK) return st;
        std::vector<float> h((size_t)3 * D);
        fibonacci_directions(D, h.data());
        HIPCHK(c, hipMemcpy(c->probe_dirs.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
        c->probe_dirs_d = D;
    }
    *d_dirs = (const float *)c->probe_dirs.p;
    return MORT_OK;
}

template <bool TREE>
void launch_probes(const ProbeArgs &a, hipStream_t s) {
    const dim3 grid((unsigned)a.r.q.n);
    switch (a.directions < QUERY_BLOCK ? a.directions : QUERY_BLOCK) {
    case 64: hipLaunchKernelGGL((probe_sh_kernel<TREE, 64>), grid, dim3(64), 0, s, a); break;
    case 128: hipLaunchKernelGGL((probe_sh_kernel<TREE, 128>), grid, dim3(128), 0, s, a); break;
    case 192: hipLaunchKernelGGL((probe_sh_kernel<TREE, 192>), grid, dim3(192), 0, s, a); break;
    default: hipLaunchKernelGGL((probe_sh_kernel<TREE, QUERY_BLOCK>), grid, dim3(QUERY_BLOCK), 0, s, a); break;
    }
}

} // namespace

int mort_probe_own_directions(mort_ctx *c, int D, hipStream_t s, const float **d_dirs) { return own_directions(c, D, s, d_dirs); }

extern "C" int mort_hip_probe_directions(int directions, float *dirs_out) {
    if (!dirs_out || !directions_ok(directions)) return MORT_ERR_INVALID;
    fibonacci_directions(directions, dirs_out);
    return MORT_OK;
}

extern "C" int mort_hip_sh9_irradiance(const float *sh, const float *normal, float *rgb_out) {
    if (!sh || !normal || !rgb_out) return MORT_ERR_INVALID;
    const double c0 = 0.2820948f, c1 = 0.4886025f, c2 = 1.0925484f, c3 = 0.31539157f, c4 = 0.5462742f; /* the basis' own constants */
    const double x = normal[0], y = normal[1], z = normal[2];
    const double A0 = M_PI, A1 = 2.0 * M_PI / 3.0, A2 = M_PI / 4.0;
    const double w[9] = {A0 * c0, A1 * (c1 * y), A1 * (c1 * z), A1 * (c1 * x), A2 * ((c2 * x) * y), A2 * ((c2 * y) * z),
                         A2 * (c3 * ((3.0 * z) * z - 1.0)), A2 * ((c2 * x) * z), A2 * (c4 * (x * x - y * y))};
    for (int ch = 0; ch < 3; ch++) {
        double e = 0.0;
        for (int k = 0; k < 9; k++) e += w[k] * (double)sh[k * 3 + ch];
        rgb_out[ch] = (float)e;
    }
    return MORT_OK;
}

extern "C" int mort_hip_probe_bake_device(mort_ctx *c, const mort_probe_params *p, size_t n, const void *d_probes, const void *d_dirs,
                                          void *d_states, void *d_sh_out, void *stream, double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    int st = probe_check(p, n, d_probes, d_dirs, d_states, d_sh_out);
    if (st != MORT_OK) return st;
    if (!aligned16(d_probes) || !aligned16(d_dirs) || !aligned16(d_states) || !aligned16(d_sh_out)) return MORT_ERR_INVALID;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    if ((st = check_light(c, p->rp.light_obj_type, p->rp.light_obj_idx)) != MORT_OK) return st;
    if (n == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    ProbeArgs a;
    query_args_device(c, a.r.q);
    probe_args_params(a, p);
    a.r.q.n = n; a.r.q.states = (mort_rng_state *)d_states;
    a.probes = (const mort_probe *)d_probes; a.dirs = (const float *)d_dirs; a.sh = (float *)d_sh_out;
    if (!a.dirs) { /* the library's set, before the clock starts */
        HIPCHK(c, hipSetDevice(c->device));
        const hipStream_t s0 = stream ? (hipStream_t)stream : c->stream;
        HIPCHK(c, switch_stream(c, s0));
        if ((st = own_directions(c, p->directions, s0, &a.dirs)) != MORT_OK) return st;
    }
    hipStream_t s;
    if ((st = stage_begin(c, stream, 0, seconds, &s)) != MORT_OK) return st;
    if (c->gen_ok) launch_probes<true>(a, s);
    else launch_probes<false>(a, s);
    HIPCHK(c, hipGetLastError());
    return stage_end(c, s, seconds);
}

/* the host-buffer form: probes, directions and streams up, the _device call on the context's stream, coefficients and streams down */
extern "C" int mort_hip_probe_bake(mort_ctx *c, const mort_probe_params *p, size_t n, const mort_probe *probes, const float *dirs,
                                   mort_rng_state *states, float *sh_out, double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    int st = probe_check(p, n, probes, dirs, states, sh_out);
    if (st != MORT_OK) return st;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    if ((st = check_light(c, p->rp.light_obj_type, p->rp.light_obj_idx)) != MORT_OK) return st;
    if (n == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, switch_stream(c, c->stream));
    const size_t D = (size_t)p->directions;
    StagePlane pl[4] = {{probes, nullptr, n * sizeof(mort_probe)}, {dirs, nullptr, 3 * D * sizeof(float)},
                        {states, states, n * D * sizeof(mort_rng_state)}, {nullptr, sh_out, n * MORT_SH9_FLOATS * sizeof(float)}};
    if ((st = stage_upload(c, pl, 4)) != MORT_OK) return st;
    double sec = 0;
    if ((st = mort_hip_probe_bake_device(c, p, n, pl[0].dev, pl[1].dev, pl[2].dev, pl[3].dev, c->stream, &sec)) != MORT_OK) return st;
    if (seconds) *seconds = sec;
    return stage_download(c, pl, 4);
}

extern "C" int mort_hip_probe_bake_host(const mort_world *world, const mort_probe_params *p, size_t n, const mort_probe *probes, const float *dirs,
                                        mort_rng_state *states, int nthreads, int flags, float *sh_out, double *seconds) {
    if (!world) return MORT_ERR_INVALID;
    int st = probe_check(p, n, probes, dirs, states, sh_out);
    if (st != MORT_OK) return st;
    SceneBlob sb;
    if ((st = build_scene_blob(world, sb)) != MORT_OK) return st;
    if ((st = check_light_object(sb.comp, world->objs.num_hittable_list, p->rp.light_obj_type, p->rp.light_obj_idx)) != MORT_OK) return st;
    if (seconds) *seconds = 0;
    if (n == 0) return MORT_OK;
    std::vector<float> own;
    if (!dirs) { own.resize(3 * (size_t)p->directions); fibonacci_directions(p->directions, own.data()); dirs = own.data(); }
    ProbeHostJob job;
    job.tree = (flags & MORT_HOST_TREE) && sb.comp.g_ok;
    query_args_host(sb, job.tree, job.a.r.q);
    probe_args_params(job.a, p);
    job.a.r.q.n = n; job.a.r.q.states = states;
    job.a.probes = probes; job.a.dirs = dirs; job.a.sh = sh_out;
    const double t0 = now_s();
    run_rows((int)n, nthreads, probe_host_probe, &job);
    if (seconds) *seconds = now_s() - t0;
    return MORT_OK;
}
