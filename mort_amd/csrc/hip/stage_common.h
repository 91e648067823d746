/*
 * stage_common.h -- the host scaffolding that the feature pass, the denoiser, the temporal step and the SVGF filter share
 * (denoise.hip, temporal.hip, svgf.hip; view.hip for the size limit): the one workgroup shape and its grid, the prologue and
 * timed epilogue of a _device entry point, the overlap checks, and the staging of the host-buffer forms.  Written once here so
 * that a new stage has nothing to copy.  The per-pixel bodies are in dev_features.h, dev_temporal.h and dev_svgf.h.
 */
#ifndef MORT_STAGE_COMMON_H
#define MORT_STAGE_COMMON_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "mort_hip.h"
#include "mort_ctx.h"

/* ---- the workgroup of every stage kernel: 64x4 pixels, so each wave covers 64 contiguous pixels of one row.  A grid of at
 * most 65535 of them per axis bounds the image the stages and a view take ---- */
constexpr int STAGE_BX = 64, STAGE_BY = 4;

static inline dim3 stage_block() { return dim3(STAGE_BX, STAGE_BY); }
static inline dim3 stage_grid(int W, int rows) { return dim3((W + STAGE_BX - 1) / STAGE_BX, (rows + STAGE_BY - 1) / STAGE_BY); }
static inline bool stage_size_ok(int W, int H) { return W > 0 && H > 0 && W < 65536 * STAGE_BX && H < 65536 * STAGE_BY; }

/* ---- a _device entry point, after its argument checks: set the device, resolve the stream (null = the context's own), wait for
 * the stage that ran on another stream (switch_stream), grow the shared float4 planes to `planes_bytes` if the stage wants them
 * (0 = not), and with `seconds` start the clock.  Without `seconds` neither function records or waits for an event ---- */
static inline int stage_begin(mort_ctx *c, void *stream, size_t planes_bytes, const double *seconds, hipStream_t *s) {
    HIPCHK(c, hipSetDevice(c->device));
    *s = stream ? (hipStream_t)stream : c->stream;
    HIPCHK(c, switch_stream(c, *s));
    if (planes_bytes) {
        const int st = ensure_buf(c, c->stage_planes, planes_bytes);
        if (st != MORT_OK) return st;
    }
    if (seconds) HIPCHK(c, hipEventRecord(c->ev0, *s));
    return MORT_OK;
}

/* ... and after its last launch: with `seconds`, wait for the stage and report its device time */
static inline int stage_end(mort_ctx *c, hipStream_t s, double *seconds) {
    if (!seconds) return MORT_OK;
    HIPCHK(c, hipEventRecord(c->ev1, s));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *seconds = ms * 1e-3;
    return MORT_OK;
}

/* ---- argument checks ---- */

static inline bool same_vec(const mort_vec3 &a, const mort_vec3 &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

/* two byte ranges share a byte (a null pointer is no range) */
static inline bool overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

/* no output overlaps an input or another output */
static inline bool buffers_disjoint(const void *const *ins, const size_t *in_bytes, int n_in, void *const *outs, const size_t *out_bytes, int n_out) {
    for (int o = 0; o < n_out; o++) {
        for (int i = 0; i < n_in; i++) if (overlap(outs[o], out_bytes[o], ins[i], in_bytes[i])) return false;
        for (int j = 0; j < o; j++) if (overlap(outs[o], out_bytes[o], outs[j], out_bytes[j])) return false;
    }
    return true;
}

/* ---- the host-buffer forms: the caller's buffers staged through one device allocation around the _device call.  A plane is
 * uploaded from `in` before the call, downloaded to `out` after it, or both; one with neither host pointer (an optional
 * buffer the caller left out) takes no memory and its `dev` is null, which is what the _device call wants for it ---- */
struct StagePlane {
    const void *in;
    void *out;
    size_t bytes;
    void *dev; /* set by stage_upload */
};

/* sizes the context's staging buffer for the planes, carves it with every plane at a multiple of 16 bytes (the history and
 * whatever else a kernel reads as float4) and uploads the inputs */
static inline int stage_upload(mort_ctx *c, StagePlane *pl, int n) {
    size_t total = 0;
    for (int i = 0; i < n; i++) if (pl[i].in || pl[i].out) total += (pl[i].bytes + 15) & ~(size_t)15;
    const int st = ensure_buf(c, c->stage_io, total);
    if (st != MORT_OK) return st;
    unsigned char *d = (unsigned char *)c->stage_io.p;
    for (int i = 0; i < n; i++) {
        pl[i].dev = nullptr;
        if (!pl[i].in && !pl[i].out) continue;
        pl[i].dev = d;
        d += (pl[i].bytes + 15) & ~(size_t)15;
        if (pl[i].in) HIPCHK(c, hipMemcpy(pl[i].dev, pl[i].in, pl[i].bytes, hipMemcpyHostToDevice));
    }
    return MORT_OK;
}

/* the outputs back to the caller; blocking, so the staging buffer is idle when the form returns */
static inline int stage_download(mort_ctx *c, const StagePlane *pl, int n) {
    for (int i = 0; i < n; i++)
        if (pl[i].out) HIPCHK(c, hipMemcpy(pl[i].out, pl[i].dev, pl[i].bytes, hipMemcpyDeviceToHost));
    return MORT_OK;
}

#endif
