/*
 * volume.hip -- irradiance volumes: a regular grid of SH9 light probes, packed into one 128-byte record per
 * probe, and the irradiance at batches of the caller's (position, normal) points, trilinearly blended between the eight
 * surrounding probes under the records' weights, in the fixed arithmetic of include/mort_hip.h.
 *
 * Kernels (gfx950, wave64, 256-thread groups, 1-D grid, no LDS):
 *   volume_sample_kernel   one lane per point.  The grid descriptor and 1 / spacing are kernel arguments (scalar registers).  A
 *                          point is read as 16 + 8 bytes where the stride is a multiple of 16, else as six dwords; the eight
 *                          corners are taken two at a time (the x neighbours of one grid row) in a loop that is not unrolled, so
 *                          at most two records are in registers; of a corner first the quarter with the weight is loaded, the
 *                          other six only if the corner contributes, none if its trilinear weight is 0; one 16-byte store.
 *   volume_sample_visible_kernel   the same with every corner's weight multiplied by the Chebyshev visibility read from the
 *                          probe's depth map (dev_depth.h): normal_bias and min_visibility ride in the argument
 *                          struct; once a corner's T * weight is known to be > 0 the corner is straight-line code (selects, no
 *                          branch), so that its four map taps (8-byte loads in the source, merged pairwise into two 16-byte
 *                          loads by the compiler) are issued in one block with its six coefficient loads and nothing is
 *                          loaded after that block's first wait (checked in the disassembly).
 *   volume_pack_kernel     one lane per 16 bytes of the records: dword loads (a probe's 108 bytes are only 4-byte aligned), one
 *                          16-byte store.
 *
 * The host forms (mort_hip_volume_*_host) run the same bodies (dev_volume.h) on host threads and make no HIP runtime call.
 * Nothing here needs an uploaded world or an RNG, looks at the partition, or touches what the render keeps.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "mort_hip.h"
#include "dev_volume.h"
#include "dev_depth.h"
#include "mort_ctx.h"
#include "mort_internal.h"
#include "stage_common.h"
#include "query_common.h"

#pragma clang fp contract(off)

/* ====================================================================== device */

__global__ void __launch_bounds__(QUERY_BLOCK) volume_sample_kernel(const VolumeArgs a) {
    const size_t i = (size_t)blockIdx.x * QUERY_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    volume_sample_one(a, i);
}

__global__ void __launch_bounds__(QUERY_BLOCK) volume_sample_visible_kernel(const VolumeVisArgs a) {
    const size_t i = (size_t)blockIdx.x * QUERY_BLOCK + threadIdx.x;
    if (i >= a.v.n) return;
    volume_vis_sample_one(a, i);
}

__global__ void __launch_bounds__(QUERY_BLOCK) volume_pack_kernel(const VolumePackArgs a) {
    const size_t t = (size_t)blockIdx.x * QUERY_BLOCK + threadIdx.x;
    if (t >= 8 * a.n) return;
    volume_pack_quad(a, t);
}

/* ====================================================================== host */

namespace {

constexpr size_t kPointBytes = sizeof(mort_volume_point);
constexpr size_t kRecordBytes = MORT_VOLUME_RECORD_FLOATS * sizeof(float);
constexpr size_t kMaxPack = kMaxRays / 8; /* a lane per 16 bytes */

bool grid_ok(const mort_volume_grid *g) {
    uint64_t probes = 1;
    for (int a = 0; a < 3; a++) {
        if (!std::isfinite(g->origin[a]) || !std::isfinite(g->spacing[a]) || !(g->spacing[a] > 0.0f)) return false;
        if (g->count[a] < 1 || g->count[a] > MORT_VOLUME_MAX_COUNT) return false;
        probes *= (uint64_t)g->count[a];
    }
    return probes <= 0x7fffffffu;
}
size_t grid_probes(const mort_volume_grid *g) { return (size_t)g->count[0] * (size_t)g->count[1] * (size_t)g->count[2]; }

/* what the three sample forms check; *span: the bytes of the points that are read */
int sample_check(const mort_volume_grid *g, const void *records, size_t n, const void *points, size_t stride, void *out, size_t *span) {
    if (!g || !records || !points || !out) return MORT_ERR_INVALID;
    if (!grid_ok(g)) return MORT_ERR_INVALID;
    if (stride < kPointBytes || stride % 4 != 0) return MORT_ERR_INVALID;
    if (n > kMaxRays || (n > 1 && stride > (SIZE_MAX - kPointBytes) / (n - 1))) return MORT_ERR_INVALID;
    *span = n ? (n - 1) * stride + kPointBytes : 0;
    const void *ins[2] = {records, points};
    const size_t in_bytes[2] = {grid_probes(g) * kRecordBytes, *span};
    void *outs[1] = {out};
    const size_t out_bytes[1] = {n * 4 * sizeof(float)};
    return buffers_disjoint(ins, in_bytes, 2, outs, out_bytes, 1) ? MORT_OK : MORT_ERR_INVALID;
}

bool vis_params_ok(const mort_volume_vis_params *vp) {
    if (!std::isfinite(vp->normal_bias) || !(vp->normal_bias >= 0.0f)) return false;
    return std::isfinite(vp->min_visibility) && vp->min_visibility >= 0.0f && vp->min_visibility <= 1.0f;
}

/* what the three visible forms check on top of that */
int visible_check(const mort_volume_grid *g, const void *records, const void *depth, const mort_volume_vis_params *vp, size_t n, const void *points,
                  size_t stride, void *out, size_t *span) {
    if (!depth || !vp) return MORT_ERR_INVALID;
    const int st = sample_check(g, records, n, points, stride, out, span);
    if (st != MORT_OK) return st;
    if (!vis_params_ok(vp)) return MORT_ERR_INVALID;
    return overlap(out, n * 4 * sizeof(float), depth, grid_probes(g) * MORT_DEPTH_FLOATS * sizeof(float)) ? MORT_ERR_INVALID : MORT_OK;
}

int pack_check(size_t n, const void *sh, const void *weight, void *records) {
    if (!sh || !records || n > kMaxPack) return MORT_ERR_INVALID;
    const void *ins[2] = {sh, weight};
    const size_t in_bytes[2] = {n * MORT_SH9_FLOATS * sizeof(float), n * sizeof(float)};
    void *outs[1] = {records};
    const size_t out_bytes[1] = {n * kRecordBytes};
    return buffers_disjoint(ins, in_bytes, 2, outs, out_bytes, 1) ? MORT_OK : MORT_ERR_INVALID;
}

void sample_args(VolumeArgs &a, const mort_volume_grid *g, const void *records, size_t n, const void *points, size_t stride, void *out) {
    a.g = *g;
    for (int k = 0; k < 3; k++) a.inv[k] = 1.0f / g->spacing[k];
    a.records = (const float *)records; a.points = (const unsigned char *)points; a.stride = stride; a.n = n; a.out = (float *)out;
}

void pack_args(VolumePackArgs &a, size_t n, const void *sh, const void *weight, void *records) {
    a.sh = (const volume_word *)sh; a.weight = (const volume_word *)weight; a.records = (volume_word *)records; a.n = n;
}

void sample_host_chunk(void *p, int chunk) {
    const VolumeArgs *a = (const VolumeArgs *)p;
    const size_t i0 = (size_t)chunk * kHostChunk, i1 = i0 + kHostChunk < a->n ? i0 + kHostChunk : a->n;
    for (size_t i = i0; i < i1; i++) volume_sample_one(*a, i);
}

void pack_host_chunk(void *p, int chunk) {
    const VolumePackArgs *a = (const VolumePackArgs *)p;
    const size_t i0 = (size_t)chunk * kHostChunk, i1 = i0 + kHostChunk < a->n ? i0 + kHostChunk : a->n;
    for (size_t t = 8 * i0; t < 8 * i1; t++) volume_pack_quad(*a, t);
}

void visible_args(VolumeVisArgs &a, const mort_volume_grid *g, const void *records, const void *depth, const mort_volume_vis_params *vp, size_t n,
                  const void *points, size_t stride, void *out) {
    sample_args(a.v, g, records, n, points, stride, out);
    a.depth = (const float *)depth; a.normal_bias = vp->normal_bias; a.min_visibility = vp->min_visibility;
}

void visible_host_chunk(void *p, int chunk) {
    const VolumeVisArgs *a = (const VolumeVisArgs *)p;
    const size_t i0 = (size_t)chunk * kHostChunk, i1 = i0 + kHostChunk < a->v.n ? i0 + kHostChunk : a->v.n;
    for (size_t i = i0; i < i1; i++) volume_vis_sample_one(*a, i);
}

} // namespace

bool mort_volume_grid_ok(const mort_volume_grid *g) { return grid_ok(g); }
bool mort_volume_vis_params_ok(const mort_volume_vis_params *p) { return vis_params_ok(p); }

extern "C" int mort_hip_volume_probes(const mort_volume_grid *g, mort_probe *probes_out) {
    if (!g || !probes_out || !grid_ok(g)) return MORT_ERR_INVALID;
    mort_probe *o = probes_out;
    for (int iz = 0; iz < g->count[2]; iz++)
        for (int iy = 0; iy < g->count[1]; iy++)
            for (int ix = 0; ix < g->count[0]; ix++, o++) {
                const int i[3] = {ix, iy, iz};
                for (int a = 0; a < 3; a++) {
                    const float step = (float)i[a] * g->spacing[a]; /* rounded, then the sum: nothing contracted */
                    o->position[a] = g->origin[a] + step;
                }
                o->time = g->time;
            }
    return MORT_OK;
}

extern "C" int mort_hip_volume_pack_host(size_t n, const float *sh, const float *weight, int nthreads, float *records_out, double *seconds) {
    const int st = pack_check(n, sh, weight, records_out);
    if (st != MORT_OK) return st;
    if (seconds) *seconds = 0;
    if (n == 0) return MORT_OK;
    VolumePackArgs a;
    pack_args(a, n, sh, weight, records_out);
    const double t0 = now_s();
    run_rows((int)((n + kHostChunk - 1) / kHostChunk), nthreads, pack_host_chunk, &a);
    if (seconds) *seconds = now_s() - t0;
    return MORT_OK;
}

extern "C" int mort_hip_volume_pack_device(mort_ctx *c, size_t n, const void *d_sh, const void *d_weight, void *d_records_out, void *stream,
                                           double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    int st = pack_check(n, d_sh, d_weight, d_records_out);
    if (st != MORT_OK) return st;
    if (!aligned16(d_sh) || !aligned16(d_weight) || !aligned16(d_records_out)) return MORT_ERR_INVALID;
    if (n == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    VolumePackArgs a;
    pack_args(a, n, d_sh, d_weight, d_records_out);
    hipStream_t s;
    if ((st = stage_begin(c, stream, 0, seconds, &s)) != MORT_OK) return st;
    const dim3 grid((unsigned)((8 * n + QUERY_BLOCK - 1) / QUERY_BLOCK)), block(QUERY_BLOCK);
    hipLaunchKernelGGL(volume_pack_kernel, grid, block, 0, s, a);
    HIPCHK(c, hipGetLastError());
    return stage_end(c, s, seconds);
}

extern "C" int mort_hip_volume_pack(mort_ctx *c, size_t n, const float *sh, const float *weight, float *records_out, double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    int st = pack_check(n, sh, weight, records_out);
    if (st != MORT_OK) return st;
    if (n == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, switch_stream(c, c->stream));
    StagePlane pl[3] = {{sh, nullptr, n * MORT_SH9_FLOATS * sizeof(float)}, {weight, nullptr, n * sizeof(float)}, {nullptr, records_out, n * kRecordBytes}};
    if ((st = stage_upload(c, pl, 3)) != MORT_OK) return st;
    double sec = 0;
    if ((st = mort_hip_volume_pack_device(c, n, pl[0].dev, pl[1].dev, pl[2].dev, c->stream, &sec)) != MORT_OK) return st;
    if (seconds) *seconds = sec;
    return stage_download(c, pl, 3);
}

extern "C" int mort_hip_volume_sample_host(const mort_volume_grid *g, const float *records, size_t n, const void *points, size_t stride,
                                           int nthreads, float *out, double *seconds) {
    size_t span = 0;
    const int st = sample_check(g, records, n, points, stride, out, &span);
    if (st != MORT_OK) return st;
    if (seconds) *seconds = 0;
    if (n == 0) return MORT_OK;
    VolumeArgs a;
    sample_args(a, g, records, n, points, stride, out);
    const double t0 = now_s();
    run_rows((int)((n + kHostChunk - 1) / kHostChunk), nthreads, sample_host_chunk, &a);
    if (seconds) *seconds = now_s() - t0;
    return MORT_OK;
}

extern "C" int mort_hip_volume_sample_device(mort_ctx *c, const mort_volume_grid *g, const void *d_records, size_t n, const void *d_points,
                                             size_t stride, void *d_out, void *stream, double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    size_t span = 0;
    int st = sample_check(g, d_records, n, d_points, stride, d_out, &span);
    if (st != MORT_OK) return st;
    if (!aligned16(d_records) || !aligned16(d_points) || !aligned16(d_out)) return MORT_ERR_INVALID;
    if (n == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    VolumeArgs a;
    sample_args(a, g, d_records, n, d_points, stride, d_out);
    hipStream_t s;
    if ((st = stage_begin(c, stream, 0, seconds, &s)) != MORT_OK) return st;
    const dim3 grid((unsigned)((n + QUERY_BLOCK - 1) / QUERY_BLOCK)), block(QUERY_BLOCK);
    hipLaunchKernelGGL(volume_sample_kernel, grid, block, 0, s, a);
    HIPCHK(c, hipGetLastError());
    return stage_end(c, s, seconds);
}

extern "C" int mort_hip_volume_sample(mort_ctx *c, const mort_volume_grid *g, const float *records, size_t n, const void *points, size_t stride,
                                      float *out, double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    size_t span = 0;
    int st = sample_check(g, records, n, points, stride, out, &span);
    if (st != MORT_OK) return st;
    if (n == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, switch_stream(c, c->stream));
    StagePlane pl[3] = {{records, nullptr, grid_probes(g) * kRecordBytes}, {points, nullptr, span}, {nullptr, out, n * 4 * sizeof(float)}};
    if ((st = stage_upload(c, pl, 3)) != MORT_OK) return st;
    double sec = 0;
    if ((st = mort_hip_volume_sample_device(c, g, pl[0].dev, n, pl[1].dev, stride, pl[2].dev, c->stream, &sec)) != MORT_OK) return st;
    if (seconds) *seconds = sec;
    return stage_download(c, pl, 3);
}

extern "C" int mort_hip_volume_sample_visible_host(const mort_volume_grid *g, const float *records, const float *depth,
                                                   const mort_volume_vis_params *vp, size_t n, const void *points, size_t stride, int nthreads,
                                                   float *out, double *seconds) {
    size_t span = 0;
    const int st = visible_check(g, records, depth, vp, n, points, stride, out, &span);
    if (st != MORT_OK) return st;
    if (seconds) *seconds = 0;
    if (n == 0) return MORT_OK;
    VolumeVisArgs a;
    visible_args(a, g, records, depth, vp, n, points, stride, out);
    const double t0 = now_s();
    run_rows((int)((n + kHostChunk - 1) / kHostChunk), nthreads, visible_host_chunk, &a);
    if (seconds) *seconds = now_s() - t0;
    return MORT_OK;
}

extern "C" int mort_hip_volume_sample_visible_device(mort_ctx *c, const mort_volume_grid *g, const void *d_records, const void *d_depth,
                                                     const mort_volume_vis_params *vp, size_t n, const void *d_points, size_t stride, void *d_out,
                                                     void *stream, double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    size_t span = 0;
    int st = visible_check(g, d_records, d_depth, vp, n, d_points, stride, d_out, &span);
    if (st != MORT_OK) return st;
    if (!aligned16(d_records) || !aligned16(d_depth) || !aligned16(d_points) || !aligned16(d_out)) return MORT_ERR_INVALID;
    if (n == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    VolumeVisArgs a;
    visible_args(a, g, d_records, d_depth, vp, n, d_points, stride, d_out);
    hipStream_t s;
    if ((st = stage_begin(c, stream, 0, seconds, &s)) != MORT_OK) return st;
    const dim3 grid((unsigned)((n + QUERY_BLOCK - 1) / QUERY_BLOCK)), block(QUERY_BLOCK);
    hipLaunchKernelGGL(volume_sample_visible_kernel, grid, block, 0, s, a);
    HIPCHK(c, hipGetLastError());
    return stage_end(c, s, seconds);
}

extern "C" int mort_hip_volume_sample_visible(mort_ctx *c, const mort_volume_grid *g, const float *records, const float *depth,
                                              const mort_volume_vis_params *vp, size_t n, const void *points, size_t stride, float *out,
                                              double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    size_t span = 0;
    int st = visible_check(g, records, depth, vp, n, points, stride, out, &span);
    if (st != MORT_OK) return st;
    if (n == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, switch_stream(c, c->stream));
    StagePlane pl[4] = {{records, nullptr, grid_probes(g) * kRecordBytes}, {depth, nullptr, grid_probes(g) * MORT_DEPTH_FLOATS * sizeof(float)},
                        {points, nullptr, span}, {nullptr, out, n * 4 * sizeof(float)}};
    if ((st = stage_upload(c, pl, 4)) != MORT_OK) return st;
    double sec = 0;
    if ((st = mort_hip_volume_sample_visible_device(c, g, pl[0].dev, pl[1].dev, vp, n, pl[2].dev, stride, pl[3].dev, c->stream, &sec)) != MORT_OK) return st;
    if (seconds) *seconds = sec;
    return stage_download(c, pl, 4);
}
