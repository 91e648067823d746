/*
 * mort_ctx.h -- the opaque mort_ctx of include/mort_hip.h, shared by the translation units of libmort_hip.so.
 */
#ifndef MORT_CTX_H
#define MORT_CTX_H

#include <hip/hip_runtime.h>

#include <pthread.h>
#include <time.h>

#include <atomic>
#include <functional>
#include <string>
#include <vector>

#include "mort_hip.h"
#include "mega_gen.h"
#include "world_images.h"

/* the kernel families of a render (mort_hip.hip choose_family) */
enum RenderFamily { FAM_MEGA, FAM_BVH, FAM_GEN, FAM_WAVE, FAM_WAVE_GEN };

/* what a render launched: filled by its family's launcher, read by its statistics */
struct LaunchPlan {
    RenderFamily fam;
    const void *kernel; /* the main kernel that ran: its registers (and static LDS) are reported */
    int block;
    int lds_bytes;      /* LDS reported: the launch's own figure, or -1 for the kernel's static LDS */
    char name[64];      /* as rocprofv3 prints it */
};

struct mort_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string last_error;
    /* scene */
    void *d_scene = nullptr;
    DScene sc{};
    bool have_world = false;
    std::vector<int> list_types, list_idxs;        /* host copy, to validate the light object at render */
    int list_first[MORT_NUM_HITTABLE_LIST]{}, list_count[MORT_NUM_HITTABLE_LIST]{};
    int n_wspheres = 0, n_wquads = 0, n_lists = 0;
    /* partition */
    mort_partition part{0, 1, 8};
    /* rng */
    mort_rng_state *d_states = nullptr;
    int rng_w = 0, rng_h = 0, rng_local_rows = 0;
    uint32_t *d_seqmats = nullptr;
    /* MORT_MODE_THROUGHPUT: one stream per (pixel, stratum row), seeded on first use from the seed of mort_hip_rng_seed */
    uint64_t seed = 0;
    bool seed_known = false; /* false after rng_load: those states have no seed to derive sub-streams from */
    mort_rng_state *d_substates = nullptr;
    float *d_vaccum = nullptr;
    size_t substates_cap = 0, vaccum_cap = 0;
    int sub_w = 0, sub_h = 0, sub_lr = 0, sub_s = 0; /* what d_substates is seeded for (0 = nothing) */
    /* scratch */
    void *d_rgba = nullptr, *d_accum = nullptr, *d_segpx = nullptr;
    size_t rgba_cap = 0, accum_cap = 0, segpx_cap = 0;
    void *d_deep = nullptr; /* state-machine megakernels: bounce-stack levels below the LDS part, [level][lane of the launch] */
    size_t deep_cap = 0;
    void *d_wave_log = nullptr; /* profile builds, MORT_WAVE_LINES=1: 16 words per wave of the last state-machine launch */
    size_t wave_log_cap = 0, wave_log_waves = 0;
    unsigned long long *d_counters = nullptr; /* [0] segments, [1] rng draws, [2] work counter */
    bool wave_ok = false; /* wavefront mode: one BVH over spheres as the whole world, hot blob fits LDS */
    /* BVH megakernel: its own LDS image (four-wide own tree, leaf records with their spheres, leaf boxes, material / texture tables) */
    void *d_fast = nullptr;
    void *d_trav = nullptr; /* wf_trav's LDS image */
    uint32_t fast_bytes = 0, trav_bytes = 0;
    BvhOffsets bvh{}; /* where the parts of the two images lie (world_images.h build_bvh_images) */
    int own_nodes = 0, own_leaves = 0, own4_stack = 1;
    bool fast_ok = false;
    /* unified-tree megakernel (mega_gen.hip): its LDS image and launch constants */
    void *d_gen = nullptr;
    unsigned *d_prio_count = nullptr; int heavy_percent = 50; /* heavy waves: device word with the number of head tiles; its threshold */
    /* d_prio_count: head word (16 bytes) | the 96 counters heavy_count_kernel reads | a copy of them as it read them (mort_hip_debug_tile_state) */
    static constexpr size_t prio_count_bytes = 16 + 2 * 96 * sizeof(unsigned long long);
    uint32_t gen_bytes = 0;
    GenArgs gen{};
    bool gen_ok = false;
    int gen_prims = 0; /* solid primitives in the unified tree */
    float gen_lo[3] = {0, 0, 0}, gen_hi[3] = {0, 0, 0}, gen_reach = 0;
    int num_cus = 256;
    /* pixel-tile ordering of the BVH megakernel: most expensive tiles first (cost = segments of the previous
     * frame with this geometry, or of a 1-sample probe) so the frame does not end on its longest pixel chains */
    unsigned *d_tile_cost = nullptr, *d_tile_order = nullptr;
    mort_rng_state *d_probe_states = nullptr;
    size_t tile_cap = 0, probe_cap = 0;
    unsigned long long cost_key = 0; /* hash of the (world, geometry, partition, camera basis) the costs in d_tile_cost belong to; 0 = none */
    unsigned world_serial = 0;       /* bumped by upload_world: part of cost_key */
    unsigned *d_tile_keys = nullptr, *d_tile_iota = nullptr; /* device argsort scratch (tile_sort.hip) */
    void *d_sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0;
    /* what the last render launch decided about its tile order, for mort_hip_debug_tile_state (debug.hip): host stores of
     * render_device_impl (reset, tiles), launch_bvh / launch_gen (grid, block, heavy) and prepare_tile_order (the rest) */
    struct TileLaunch {
        int ordered = 0, probed = 0, tiles = 0, tiles_x = 0, grid = 0, block = 0, key_sum = 0, spread_shift = 0, gen_tiles = 0;
        int heavy[4] = {0, 0, 0, 0}; /* mod, num, cap, percent */
        int has_head = 0;            /* heavy_count_kernel ran for this launch: d_prio_count[0] and the saved counters are its */
    } tile_launch;
    hipStream_t last_stream = nullptr; /* stream of the most recent render launch (may be the caller's) */
    /* wavefront mode work buffers */
    void *d_wf = nullptr;
    size_t wf_bytes = 0;
    unsigned *h_live = nullptr; /* pinned */
    int wf_fronts = 0;          /* fronts of the last wavefront render (reported) */
    /* multi-GPU frame gather over RCCL (comm_rccl.hip): one communicator per context, rank = part.rank */
    void *comm = nullptr;            /* ncclComm_t */
    void *d_gather = nullptr;        /* rank 0: nranks x max tile bytes */
    void *d_frame = nullptr;         /* rank 0: the de-interleaved W x H x 4 frame */
    size_t gather_cap = 0, frame_cap = 0;
    hipEvent_t ev_g0 = nullptr, ev_g1 = nullptr; /* brackets of the gather step (created on first use) */
    /* mort_hip_render_gather: the render's statistics are collected after the gather's one host wait */
    bool defer_stats = false;
    std::function<int(mort_stats *)> pending_stats;
    /* the stages (feature pass, denoiser, temporal step, SVGF filter; stage_common.h): scratch that frees itself when
     * mort_hip_shutdown deletes the context, nothing the render keeps across frames */
    struct Scratch {
        void *p = nullptr;
        size_t cap = 0;
        ~Scratch() { if (p) (void)hipFree(p); }
    };
    /* Both are shared by every stage, whatever the image size; each call sizes and carves them anew and expects nothing of
     * their contents.  That is safe because every user passes through switch_stream first: a call on another stream than
     * the previous stage's waits for that stream, and calls on one stream run in order, so no two stages are in flight over
     * the same bytes; a call that has to grow a buffer frees it with hipFree, which waits for the device's outstanding work
     * as it did when one stage ran twice at growing sizes.  The host-buffer forms, stage_io's only users, are blocking:
     * they return after their downloads, with the buffer idle */
    Scratch stage_planes; /* the filters' four float4 planes: colour (+ variance) ping-pong, (normal, depth), albedo */
    Scratch stage_io;     /* the host-buffer forms' device copies of the caller's buffers (stage_upload) */
    Scratch probe_dirs;   /* light probes (probe.hip): the library's own direction set for the last D asked for, 3 D floats */
    int probe_dirs_d = 0; /* that D; 0 = none yet */
    hipStream_t dn_stream = nullptr; /* stream of the last stage launch */
    /* views (view.hip): the ones alive on this context, freed by mort_hip_shutdown */
    std::vector<struct mort_view *> views;
};

static inline int hip_fail(mort_ctx *c, hipError_t e, const char *what) {
    if (c) c->last_error = std::string(what) + ": " + hipGetErrorString(e);
    return MORT_ERR_HIP;
}
#define HIPCHK(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return hip_fail(ctx, e_, #call); } while (0)

/* ---- host helpers of the translation units ---- */

/* a device buffer of at least `need` bytes in *p (capacity *cap); a smaller one is freed first */
static inline int ensure_buf(mort_ctx *c, void **p, size_t *cap, size_t need) {
    if (*p && *cap >= need) return MORT_OK;
    if (*p) { HIPCHK(c, hipFree(*p)); *p = nullptr; *cap = 0; }
    HIPCHK(c, hipMalloc(p, need ? need : 16));
    *cap = need;
    return MORT_OK;
}
static inline int ensure_buf(mort_ctx *c, mort_ctx::Scratch &b, size_t need) { return ensure_buf(c, &b.p, &b.cap, need); }

/* a stage call (feature pass, denoiser, temporal step, SVGF filter) on another stream than the previous one: that one may still
 * use the shared stage scratch */
static inline hipError_t switch_stream(mort_ctx *c, hipStream_t s) {
    hipError_t e = hipSuccess;
    if (c->dn_stream && c->dn_stream != s) e = hipStreamSynchronize(c->dn_stream);
    c->dn_stream = s;
    return e;
}

/* Wait for everything this context has launched: its own stream and, if a render went to a caller's stream, that one
 * too -- before any call that reads, overwrites or frees what a render kernel uses (states, scene, counters). */
static inline hipError_t quiesce(mort_ctx *c) {
    hipError_t e = hipSuccess;
    if (c->stream) e = hipStreamSynchronize(c->stream);
    if (c->last_stream && c->last_stream != c->stream) { hipError_t e2 = hipStreamSynchronize(c->last_stream); if (e == hipSuccess) e = e2; }
    c->last_stream = nullptr;
    if (c->dn_stream && c->dn_stream != c->stream) { hipError_t e2 = hipStreamSynchronize(c->dn_stream); if (e == hipSuccess) e = e2; } /* the stages */
    c->dn_stream = nullptr;
    return e;
}

/* rows of `height` that partition p owns: blocks rank, rank + nranks, ... of rows_per_block rows */
static inline int local_rows_for(const mort_partition &p, int height) {
    int n = 0;
    const int rpb = p.rows_per_block;
    const int nblocks = (height + rpb - 1) / rpb;
    for (int b = p.rank; b < nblocks; b += p.nranks) {
        int r0 = b * rpb, r1 = r0 + rpb;
        if (r1 > height) r1 = height;
        n += r1 - r0;
    }
    return n;
}

/* the image row of partition p's packed row ly */
static inline int global_row_host(const mort_partition &p, int ly) {
    const int lb = ly / p.rows_per_block, within = ly % p.rows_per_block;
    return (lb * p.nranks + p.rank) * p.rows_per_block + within;
}

/* the camera must lie where the unified tree's pads were sized for (scene_compile.h build_unified): its centre, widened by
 * the lens radius `rad` for rays that start on the lens */
static inline bool camera_in_reach(const mort_camera *cam, const float lo[3], const float hi[3], float reach, float rad) {
    for (int k = 0; k < 3; k++) {
        const float v = cam->center.e[k];
        if (!(v - rad >= lo[k] - reach && v + rad <= hi[k] + reach)) return false;
    }
    return true;
}

/* the light object a camera or a radiance query names must be primitives the light-sampling code can index (pdf.cuh:60-80),
 * checked against the host copy of the uploaded world's lists */
static inline int check_light(const mort_ctx *c, int type, int idx) {
    if (type == -1) return MORT_OK;
    if (type == MORT_OBJ_SPHERE) return (idx >= 0 && idx < c->n_wspheres) ? MORT_OK : MORT_ERR_INVALID;
    if (type == MORT_OBJ_QUAD) return (idx >= 0 && idx < c->n_wquads) ? MORT_OK : MORT_ERR_INVALID;
    if (type == MORT_OBJ_HITTABLE_LIST) {
        if (idx < 0 || idx >= c->n_lists || idx >= MORT_NUM_HITTABLE_LIST) return MORT_ERR_INVALID;
        if (c->list_count[idx] <= 0) return MORT_ERR_INVALID;
        for (int i = 0; i <= c->list_count[idx]; i++) { /* the entry past the members too: random_int(0, n - 1) can give n (scene_compile.h) */
            const int t = c->list_types[c->list_first[idx] + i], k = c->list_idxs[c->list_first[idx] + i];
            if (t == MORT_OBJ_SPHERE) { if (k < 0 || k >= c->n_wspheres) return MORT_ERR_INVALID; }
            else if (t == MORT_OBJ_QUAD) { if (k < 0 || k >= c->n_wquads) return MORT_ERR_INVALID; }
            else if (t == MORT_OBJ_HITTABLE_LIST) return MORT_ERR_UNSUPPORTED; /* nested light lists */
        }
        return MORT_OK;
    }
    return MORT_OK; /* any other tag samples nothing: pdf 0, direction (1,0,0) (objects.cuh:961,978) */
}

static inline double now_s() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }

/* run `fn(arg, row)` for rows [0, rows) on `nthreads` host threads (1..256), rows handed out one at a time */
struct RowJob {
    std::atomic<int> next{0};
    int rows = 0;
    void (*fn)(void *, int) = nullptr;
    void *arg = nullptr;
};
static inline void *row_worker(void *p) {
    RowJob *j = (RowJob *)p;
    for (;;) {
        const int r = j->next.fetch_add(1);
        if (r >= j->rows) break;
        j->fn(j->arg, r);
    }
    return nullptr;
}
static inline void run_rows(int rows, int nthreads, void (*fn)(void *, int), void *arg) {
    RowJob job;
    job.rows = rows; job.fn = fn; job.arg = arg;
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 256) nthreads = 256;
    std::vector<pthread_t> th((size_t)nthreads - 1);
    size_t started = 0;
    for (; started < th.size(); started++)
        if (pthread_create(&th[started], nullptr, row_worker, &job) != 0) break;
    row_worker(&job);
    for (size_t i = 0; i < started; i++) pthread_join(th[i], nullptr);
}


#endif
