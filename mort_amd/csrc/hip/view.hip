/*
 * view.hip -- the view: a frame's whole chain kept on the device across frames.
 *
 *   render (or cached frame, mort_hip_view_set_cache) -> first-hit features -> [temporal step] -> [a-trous denoiser | SVGF filter] -> uchar4
 *
 * No kernel lives here and no arithmetic: a frame is the existing _device entry points (mort_hip.hip, denoise.hip, temporal.hip,
 * svgf.hip) called back to back on one stream with their `seconds` / `stats` waits left out, so its bits are those of the calls
 * chained by hand.  What this file adds is the residency (the view owns every buffer the chain passes on, the ping-ponged
 * history and the previous camera), the single host wait per frame (the render's statistics are deferred as
 * mort_hip_render_gather defers them; the stage times come from the view's own events, read after that wait), the skipped
 * feature pass under a still camera, and the invalidation rules.  The size limit is the stages' (stage_common.h).
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>

#include "mort_hip.h"
#include "mort_ctx.h"
#include "mort_internal.h"
#include "stage_common.h"

/* the view's events of a frame: after the features, after the temporal step, after the filter.  The render is bracketed by the
 * context's own pair (ev0, ev1: what mort_stats.seconds is), which nothing records again before the frame's statistics are read */
enum { EV_FEAT, EV_TEMPORAL, EV_FILTER, EV_COUNT };

struct mort_view {
    mort_ctx *ctx = nullptr;
    mort_view_params p{};
    size_t npx = 0;
    /* device buffers, whole image */
    void *d_rgba = nullptr;     /* the render's uchar4 */
    float *d_accum = nullptr;   /* the render's accumulators */
    float *d_feat = nullptr;    /* albedo (3), normal (3), depth (1) */
    float *d_hist[2] = {nullptr, nullptr};
    float *d_tacc = nullptr;    /* accumulated colour */
    float *d_var = nullptr;     /* the temporal step's variance */
    float *d_facc = nullptr;    /* filtered colour */
    void *d_out = nullptr;      /* mort_hip_view_frame: the last stage's uchar4 before it leaves the device */
    uint8_t *h_out = nullptr;   /* ... and the pinned buffer it is copied to (allocated on first use) */
    hipEvent_t ev[EV_COUNT] = {};
    hipStream_t last_stream = nullptr; /* stream of the last frame: what read / destroy wait for */
    /* frame-to-frame state */
    int frame = 0;              /* frames since the last reset */
    int hist_cur = 0;           /* the history the last frame wrote */
    bool have_frame = false;    /* the buffers hold a frame (mort_hip_view_read) */
    bool have_feat = false;     /* d_feat belongs to feat_cam and world feat_serial */
    mort_camera prev_cam{}, feat_cam{};
    unsigned feat_serial = 0, hist_serial = 0;
    /* mort_hip_view_set_cache: the frames are cached frames over the caller's device buffers */
    bool cached = false;
    mort_cached_frame_params cache{};
    const void *d_records = nullptr, *d_cache_depth = nullptr;
    uint32_t *d_ends = nullptr; /* per pixel, the last frame's paths that ended in the volume (allocated when a cache is first attached) */
    /* mort_hip_view_set_cache_direct: the frames are direct cached frames */
    bool direct = false;
    uint32_t *d_lit = nullptr; /* per pixel, the last frame's ended paths whose shadow segment saw light (allocated with the first direct cache) */
    void *own_records = nullptr, *own_depth = nullptr; /* mort_hip_view_set_cache_host: the view's own copies of the caller's host arrays */

    float *albedo() const { return d_feat; }
    float *normal() const { return d_feat + 3 * npx; }
    float *depth() const { return d_feat + 6 * npx; }
};

namespace {

/* bit-identical in every field the feature pass reads (denoise.hip feat_camera) */
bool same_feature_camera(const mort_camera &a, const mort_camera &b) {
    return a.image_width == b.image_width && a.image_height == b.image_height && same_vec(a.background, b.background) &&
           same_vec(a.center, b.center) && same_vec(a.pixel00_loc, b.pixel00_loc) && same_vec(a.pixel_delta_u, b.pixel_delta_u) &&
           same_vec(a.pixel_delta_v, b.pixel_delta_v);
}

void free_buffers(mort_view *v) {
    (void)hipFree(v->d_rgba); (void)hipFree(v->d_accum); (void)hipFree(v->d_feat); (void)hipFree(v->d_hist[0]); (void)hipFree(v->d_hist[1]);
    (void)hipFree(v->d_tacc); (void)hipFree(v->d_var); (void)hipFree(v->d_facc); (void)hipFree(v->d_out); (void)hipFree(v->d_ends);
    (void)hipFree(v->d_lit);
    (void)hipFree(v->own_records); (void)hipFree(v->own_depth);
    if (v->h_out) (void)hipHostFree(v->h_out);
    for (hipEvent_t e : v->ev) if (e) (void)hipEventDestroy(e);
}

/* a frame that failed half way leaves nothing to build on, and its render's deferred statistics are not collected */
int frame_failed(mort_view *v, int st) {
    v->ctx->pending_stats = nullptr;
    v->have_frame = v->have_feat = false;
    v->frame = 0;
    return st;
}

/* One frame.  d_dst: where the frame's uchar4 goes on the device (the caller's buffer, or the view's d_out); h_dst: the host
 * buffer of mort_hip_view_frame, or null.  wait: one host wait at the end (always with stats or h_dst). */
int view_frame(mort_view *v, const mort_camera *cam, int mode, void *d_dst, uint8_t *h_dst, void *stream, mort_view_stats *stats) {
    mort_ctx *c = v->ctx;
    const int W = v->p.width, H = v->p.height;
    if (cam->image_width != W || cam->image_height != H) return MORT_ERR_INVALID;
    if (c->part.nranks != 1) return MORT_ERR_UNSUPPORTED;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    /* the previous frame went to another stream: it still reads and writes what this one does */
    if (v->last_stream && v->last_stream != s) HIPCHK(c, hipStreamSynchronize(v->last_stream));
    const bool timed = stats != nullptr;
    const bool wait = timed || h_dst != nullptr;
    const size_t npx = v->npx;

    /* a new world: neither the features nor the history describe it */
    if (v->frame > 0 && v->hist_serial != c->world_serial) v->frame = 0;
    const bool fresh = v->frame == 0;
    const bool reuse = v->have_feat && v->feat_serial == c->world_serial && same_feature_camera(v->feat_cam, *cam);
    const bool filter = v->p.filter != MORT_VIEW_FILTER_NONE;

    /* ---- render: into the view's own buffers; with statistics, those are collected after the frame's one wait ---- */
    mort_stats local;
    std::memset(&local, 0, sizeof local);
    c->defer_stats = timed; c->pending_stats = nullptr;
    int st;
    if (!v->cached) st = mort_hip_render_device(c, cam, mode, v->d_rgba, v->d_accum, s, timed ? &local : nullptr);
    else if (mode != MORT_MODE_MEGA) st = MORT_ERR_UNSUPPORTED;
    else if (v->direct)
        st = mort_hip_render_cached_direct_device(c, cam, &v->cache, v->d_records, v->d_cache_depth, v->d_rgba, v->d_accum, v->d_ends, v->d_lit, s,
                                                  timed ? &local : nullptr);
    else st = mort_hip_render_cached_device(c, cam, &v->cache, v->d_records, v->d_cache_depth, v->d_rgba, v->d_accum, v->d_ends, s, timed ? &local : nullptr);
    c->defer_stats = false;
    if (st != MORT_OK) {
        c->pending_stats = nullptr;
        /* a refusal (argument, world, RNG states, capacity, mode) comes before anything is launched and leaves the view as it
         * was; a runtime failure may come after the render has begun to overwrite the accumulators */
        return (st == MORT_ERR_HIP || st == MORT_ERR_NOMEM) ? frame_failed(v, st) : st;
    }
    v->last_stream = s;
    v->have_frame = false;

    /* ---- features: skipped under a still camera ---- */
    if (!reuse) {
        v->have_feat = false;
        st = mort_hip_render_features_device(c, cam, v->albedo(), v->normal(), v->depth(), s, nullptr);
        if (st != MORT_OK) return frame_failed(v, st);
        v->feat_cam = *cam; v->feat_serial = c->world_serial; v->have_feat = true;
    }
    if (timed && hipEventRecord(v->ev[EV_FEAT], s) != hipSuccess) return frame_failed(v, MORT_ERR_HIP);

    /* ---- temporal step, filter: the last stage that runs writes the frame's uchar4 ---- */
    const void *colour = v->d_accum, *variance = nullptr;
    const void *d_src = v->d_rgba; /* where the frame's uchar4 is, if no stage wrote it to d_dst */
    if (v->p.temporal) {
        const int out = fresh ? 0 : 1 - v->hist_cur;
        st = mort_hip_temporal_device(c, &v->p.tp, fresh ? nullptr : &v->prev_cam, cam, W, H, v->d_accum, v->normal(), v->depth(),
                                      fresh ? nullptr : v->d_hist[v->hist_cur], v->d_hist[out], v->d_tacc, v->d_var, filter ? nullptr : d_dst,
                                      s, nullptr);
        if (st != MORT_OK) return frame_failed(v, st);
        v->hist_cur = out;
        colour = v->d_tacc; variance = v->d_var;
        if (!filter) d_src = nullptr;
        if (timed && hipEventRecord(v->ev[EV_TEMPORAL], s) != hipSuccess) return frame_failed(v, MORT_ERR_HIP);
    }
    if (filter) {
        if (v->p.filter == MORT_VIEW_FILTER_DENOISE)
            st = mort_hip_denoise_device(c, &v->p.dp, W, H, colour, v->albedo(), v->normal(), v->depth(), v->d_facc, d_dst, s, nullptr);
        else
            st = mort_hip_svgf_device(c, &v->p.sp, W, H, colour, v->albedo(), v->normal(), v->depth(), variance, v->d_facc, nullptr, d_dst, s, nullptr);
        if (st != MORT_OK) return frame_failed(v, st);
        d_src = nullptr;
        if (timed && hipEventRecord(v->ev[EV_FILTER], s) != hipSuccess) return frame_failed(v, MORT_ERR_HIP);
    }

    /* ---- the frame leaves: only the uchar4 moves ---- */
    hipError_t e = hipSuccess;
    if (h_dst) e = hipMemcpyAsync(v->h_out, d_src ? d_src : d_dst, npx * 4, hipMemcpyDeviceToHost, s);
    else if (d_src) e = hipMemcpyAsync(d_dst, d_src, npx * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && wait) e = hipStreamSynchronize(s); /* the one host wait */
    if (e != hipSuccess) { hip_fail(c, e, "view frame"); return frame_failed(v, MORT_ERR_HIP); }
    if (h_dst) std::memcpy(h_dst, v->h_out, npx * 4);

    const int index = v->frame;
    v->prev_cam = *cam;
    v->hist_serial = c->world_serial;
    v->frame++;
    v->have_frame = true;
    if (!timed) return MORT_OK;

    std::memset(stats, 0, sizeof *stats);
    if (c->pending_stats) {
        st = c->pending_stats(&local);
        c->pending_stats = nullptr;
        if (st != MORT_OK) return st;
    }
    stats->render = local;
    auto span = [](hipEvent_t a, hipEvent_t b, double *out) {
        float ms = 0;
        const hipError_t ee = hipEventElapsedTime(&ms, a, b);
        *out = ms * 1e-3;
        return ee;
    };
    hipEvent_t last = v->ev[EV_FEAT];
    if (!reuse) HIPCHK(c, span(c->ev1, v->ev[EV_FEAT], &stats->features_seconds));
    if (v->p.temporal) { HIPCHK(c, span(last, v->ev[EV_TEMPORAL], &stats->temporal_seconds)); last = v->ev[EV_TEMPORAL]; }
    if (filter) { HIPCHK(c, span(last, v->ev[EV_FILTER], &stats->filter_seconds)); last = v->ev[EV_FILTER]; }
    /* from where the render's own time starts (its upkeep before that -- tile ordering, a moved camera's probe -- is in
     * neither) to the last event: the stages and whatever idles between them */
    double tail = 0;
    HIPCHK(c, span(c->ev1, last, &tail));
    stats->device_seconds = local.seconds + tail;
    stats->frame = index;
    stats->features_reused = reuse ? 1 : 0;
    stats->history_reset = fresh ? 1 : 0;
    return MORT_OK;
}

} // namespace

extern "C" int mort_hip_view_defaults(mort_view_params *p) {
    if (!p) return MORT_ERR_INVALID;
    std::memset(p, 0, sizeof *p);
    p->temporal = 1;
    p->filter = MORT_VIEW_FILTER_SVGF;
    mort_hip_temporal_defaults(&p->tp);
    mort_hip_denoise_defaults(&p->dp);
    mort_hip_svgf_defaults(&p->sp);
    return MORT_OK;
}

extern "C" int mort_hip_view_check_params(const mort_view_params *p) {
    if (!p) return MORT_ERR_INVALID;
    if (!stage_size_ok(p->width, p->height)) return MORT_ERR_INVALID; /* the stages' grid limits */
    if (p->temporal != 0 && p->temporal != 1) return MORT_ERR_INVALID;
    if (p->filter != MORT_VIEW_FILTER_NONE && p->filter != MORT_VIEW_FILTER_DENOISE && p->filter != MORT_VIEW_FILTER_SVGF) return MORT_ERR_INVALID;
    if (p->temporal && !mort_temporal_params_ok(&p->tp)) return MORT_ERR_INVALID;
    if (p->filter == MORT_VIEW_FILTER_DENOISE && !mort_denoise_params_ok(&p->dp)) return MORT_ERR_INVALID;
    if (p->filter == MORT_VIEW_FILTER_SVGF && !mort_svgf_params_ok(&p->sp)) return MORT_ERR_INVALID;
    return MORT_OK;
}

extern "C" int mort_hip_view_create(mort_ctx *c, const mort_view_params *p, mort_view **out) {
    if (out) *out = nullptr;
    if (!c || !p || !out) return MORT_ERR_INVALID;
    int st = mort_hip_view_check_params(p);
    if (st != MORT_OK) return st;
    HIPCHK(c, hipSetDevice(c->device));
    mort_view *v = new (std::nothrow) mort_view;
    if (!v) return MORT_ERR_NOMEM;
    v->ctx = c; v->p = *p;
    const size_t npx = v->npx = (size_t)p->width * (size_t)p->height, hb = npx * MORT_TEMPORAL_HISTORY_FLOATS * sizeof(float);
    hipError_t e = hipMalloc(&v->d_rgba, npx * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&v->d_accum, npx * 12);
    if (e == hipSuccess) e = hipMalloc((void **)&v->d_feat, npx * 28);
    if (e == hipSuccess) e = hipMalloc(&v->d_out, npx * 4);
    if (p->temporal) {
        for (int k = 0; k < 2 && e == hipSuccess; k++) e = hipMalloc((void **)&v->d_hist[k], hb);
        if (e == hipSuccess) e = hipMalloc((void **)&v->d_tacc, npx * 12);
        if (e == hipSuccess) e = hipMalloc((void **)&v->d_var, npx * 4);
    }
    if (p->filter != MORT_VIEW_FILTER_NONE && e == hipSuccess) e = hipMalloc((void **)&v->d_facc, npx * 12);
    for (int k = 0; k < EV_COUNT && e == hipSuccess; k++) e = hipEventCreate(&v->ev[k]);
    if (e != hipSuccess) {
        free_buffers(v);
        delete v;
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return MORT_ERR_NOMEM; }
        return hip_fail(c, e, "mort_hip_view_create");
    }
    c->views.push_back(v);
    *out = v;
    return MORT_OK;
}

extern "C" void mort_hip_view_destroy(mort_view *v) {
    if (!v) return;
    mort_ctx *c = v->ctx;
    (void)hipSetDevice(c->device);
    if (v->last_stream) (void)hipStreamSynchronize(v->last_stream);
    c->views.erase(std::remove(c->views.begin(), c->views.end(), v), c->views.end());
    free_buffers(v);
    delete v;
}

/* mort_hip_shutdown, after it has waited for every stream the context used */
void mort_views_free(mort_ctx *c) {
    for (mort_view *v : c->views) { free_buffers(v); delete v; }
    c->views.clear();
}

extern "C" int mort_hip_view_reset(mort_view *v) {
    if (!v) return MORT_ERR_INVALID;
    v->frame = 0;
    return MORT_OK;
}

namespace {
/* the volume copies of an earlier mort_hip_view_set_cache_host, once no frame in flight reads them */
int free_own_cache(mort_view *v) {
    if (!v->own_records && !v->own_depth) return MORT_OK;
    mort_ctx *c = v->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    if (v->last_stream) HIPCHK(c, hipStreamSynchronize(v->last_stream));
    (void)hipFree(v->own_records); (void)hipFree(v->own_depth);
    v->own_records = v->own_depth = nullptr;
    return MORT_OK;
}
} // namespace

namespace {
/* device copies of a caller's host records and maps (depth may be null), for the _host forms of set_cache and update_cache */
int upload_cache(mort_view *v, const mort_volume_grid &grid, const float *records, const float *depth, void **d_rec, void **d_dep, const char *what) {
    mort_ctx *c = v->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t probes = (size_t)grid.count[0] * (size_t)grid.count[1] * (size_t)grid.count[2];
    const size_t rb = probes * MORT_VOLUME_RECORD_FLOATS * sizeof(float), db = probes * MORT_DEPTH_FLOATS * sizeof(float);
    *d_rec = *d_dep = nullptr;
    hipError_t e = hipMalloc(d_rec, rb);
    if (e == hipSuccess) e = hipMemcpy(*d_rec, records, rb, hipMemcpyHostToDevice);
    if (e == hipSuccess && depth) e = hipMalloc(d_dep, db);
    if (e == hipSuccess && depth) e = hipMemcpy(*d_dep, depth, db, hipMemcpyHostToDevice);
    return e == hipSuccess ? MORT_OK : e == hipErrorOutOfMemory ? ((void)hipGetLastError(), MORT_ERR_NOMEM) : hip_fail(c, e, what);
}
} // namespace

namespace {
int set_cache_impl(mort_view *v, const mort_cached_frame_params *p, const void *d_records, const void *d_depth, bool direct);

int set_cache_host_impl(mort_view *v, const mort_cached_frame_params *p, const float *records, const float *depth, bool direct, const char *what) {
    if (!v || !p) return MORT_ERR_INVALID;
    if (!mort_cached_volume_ok(p->cache_depth, p->flags, &p->grid, &p->vis, records, depth)) return MORT_ERR_INVALID;
    void *d_rec = nullptr, *d_dep = nullptr;
    int st = upload_cache(v, p->grid, records, depth, &d_rec, &d_dep, what);
    if (st == MORT_OK) st = set_cache_impl(v, p, d_rec, d_dep, direct); /* frees the copies of an earlier call */
    if (st != MORT_OK) { (void)hipFree(d_rec); (void)hipFree(d_dep); return st; }
    v->own_records = d_rec; v->own_depth = d_dep;
    return MORT_OK;
}
} // namespace

extern "C" int mort_hip_view_set_cache_host(mort_view *v, const mort_cached_frame_params *p, const float *records, const float *depth) {
    return set_cache_host_impl(v, p, records, depth, false, "mort_hip_view_set_cache_host");
}

extern "C" int mort_hip_view_set_cache_direct_host(mort_view *v, const mort_cached_frame_params *p, const float *records, const float *depth) {
    return set_cache_host_impl(v, p, records, depth, true, "mort_hip_view_set_cache_direct_host");
}

/* new records and maps under the attached params; the history goes on */
extern "C" int mort_hip_view_update_cache(mort_view *v, const void *d_records, const void *d_depth) {
    if (!v || !v->cached) return MORT_ERR_INVALID;
    const mort_cached_frame_params *p = &v->cache;
    if (!mort_cached_volume_ok(p->cache_depth, p->flags, &p->grid, &p->vis, d_records, d_depth)) return MORT_ERR_INVALID;
    if (((uintptr_t)d_records & 15u) || ((uintptr_t)d_depth & 15u)) return MORT_ERR_INVALID;
    const int st = free_own_cache(v); /* whatever is attached now replaces them */
    if (st != MORT_OK) return st;
    v->d_records = d_records; v->d_cache_depth = d_depth;
    return MORT_OK;
}

extern "C" int mort_hip_view_update_cache_host(mort_view *v, const float *records, const float *depth) {
    if (!v || !v->cached) return MORT_ERR_INVALID;
    const mort_cached_frame_params *p = &v->cache;
    if (!mort_cached_volume_ok(p->cache_depth, p->flags, &p->grid, &p->vis, records, depth)) return MORT_ERR_INVALID;
    void *d_rec = nullptr, *d_dep = nullptr;
    int st = upload_cache(v, p->grid, records, depth, &d_rec, &d_dep, "mort_hip_view_update_cache_host");
    if (st == MORT_OK) st = mort_hip_view_update_cache(v, d_rec, d_dep); /* frees the copies of an earlier call */
    if (st != MORT_OK) { (void)hipFree(d_rec); (void)hipFree(d_dep); return st; }
    v->own_records = d_rec; v->own_depth = d_dep;
    return MORT_OK;
}

namespace {
/* one more per-pixel count of the view's, allocated when first wanted */
int ensure_counts(mort_view *v, uint32_t **d) {
    if (*d) return MORT_OK;
    mort_ctx *c = v->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    const hipError_t e = hipMalloc((void **)d, v->npx * sizeof(uint32_t));
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return MORT_ERR_NOMEM; }
    HIPCHK(c, e);
    return MORT_OK;
}

int set_cache_impl(mort_view *v, const mort_cached_frame_params *p, const void *d_records, const void *d_depth, bool direct) {
    if (!v) return MORT_ERR_INVALID;
    if (p) { /* what mort_hip_render_cached[_direct]_device will ask of them at every frame */
        if (!mort_cached_volume_ok(p->cache_depth, p->flags, &p->grid, &p->vis, d_records, d_depth)) return MORT_ERR_INVALID;
        if (((uintptr_t)d_records & 15u) || ((uintptr_t)d_depth & 15u)) return MORT_ERR_INVALID;
        int st = ensure_counts(v, &v->d_ends);
        if (st == MORT_OK && direct) st = ensure_counts(v, &v->d_lit);
        if (st != MORT_OK) return st;
    }
    const int st = free_own_cache(v); /* whatever is attached now replaces them */
    if (st != MORT_OK) return st;
    if (p) v->cache = *p;
    v->cached = p != nullptr;
    v->direct = v->cached && direct;
    v->d_records = p ? d_records : nullptr; v->d_cache_depth = p ? d_depth : nullptr;
    v->frame = 0; /* another estimator: its history does not continue */
    return MORT_OK;
}
} // namespace

extern "C" int mort_hip_view_set_cache(mort_view *v, const mort_cached_frame_params *p, const void *d_records, const void *d_depth) {
    return set_cache_impl(v, p, d_records, d_depth, false);
}

extern "C" int mort_hip_view_set_cache_direct(mort_view *v, const mort_cached_frame_params *p, const void *d_records, const void *d_depth) {
    return set_cache_impl(v, p, d_records, d_depth, true);
}

extern "C" int mort_hip_view_frame_device(mort_view *v, const mort_camera *cam, int mode, void *d_rgba_out, void *stream, mort_view_stats *stats) {
    if (!v || !cam || !d_rgba_out) return MORT_ERR_INVALID;
    return view_frame(v, cam, mode, d_rgba_out, nullptr, stream, stats);
}

extern "C" int mort_hip_view_frame(mort_view *v, const mort_camera *cam, int mode, uint8_t *rgba_out, mort_view_stats *stats) {
    if (!v || !cam || !rgba_out) return MORT_ERR_INVALID;
    mort_ctx *c = v->ctx;
    if (!v->h_out) {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipHostMalloc((void **)&v->h_out, v->npx * 4, hipHostMallocDefault));
    }
    return view_frame(v, cam, mode, v->d_out, rgba_out, nullptr, stats);
}

extern "C" int mort_hip_view_read(mort_view *v, int what, void *host_out) {
    if (!v || !host_out || !v->have_frame) return MORT_ERR_INVALID;
    mort_ctx *c = v->ctx;
    const size_t npx = v->npx;
    const void *src = nullptr; /* 32-bit words: floats, but for MORT_VIEW_ENDS and MORT_VIEW_LIT */
    size_t floats = 0;
    switch (what) {
    case MORT_VIEW_RAW_ACCUM: src = v->d_accum; floats = 3 * npx; break;
    case MORT_VIEW_ACCUM: src = v->d_tacc; floats = 3 * npx; break;
    case MORT_VIEW_FILTERED: src = v->d_facc; floats = 3 * npx; break;
    case MORT_VIEW_VARIANCE: src = v->d_var; floats = npx; break;
    case MORT_VIEW_ALBEDO: src = v->albedo(); floats = 3 * npx; break;
    case MORT_VIEW_NORMAL: src = v->normal(); floats = 3 * npx; break;
    case MORT_VIEW_DEPTH: src = v->depth(); floats = npx; break;
    case MORT_VIEW_ENDS: src = v->cached ? v->d_ends : nullptr; floats = npx; break;
    case MORT_VIEW_LIT: src = v->direct ? v->d_lit : nullptr; floats = npx; break;
    case MORT_VIEW_HISTORY: src = v->p.temporal ? v->d_hist[v->hist_cur] : (const void *)nullptr; floats = MORT_TEMPORAL_HISTORY_FLOATS * npx; break;
    default: return MORT_ERR_INVALID;
    }
    if (!src) return MORT_ERR_INVALID; /* a buffer this configuration does not produce */
    HIPCHK(c, hipSetDevice(c->device));
    if (v->last_stream) HIPCHK(c, hipStreamSynchronize(v->last_stream));
    HIPCHK(c, hipMemcpy(host_out, src, floats * sizeof(float), hipMemcpyDeviceToHost));
    return MORT_OK;
}
