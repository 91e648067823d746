/*
 * context.hip -- the life of a mort_ctx and its RNG state: init / shutdown, the partition, the upload of a world with the
 * LDS images the kernels read (world_images.h decides, this file copies), and the per-pixel XORWOW streams.
 *
 * Kernel:
 *   seed_kernel   per-pixel XORWOW init with the 2^67-step sequence skip (replaces setup_rng, rng.cuh:8-15); also seeds
 *                 the (pixel, stratum row) streams of MORT_MODE_THROUGHPUT for the render (mort_ensure_substates)
 */
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "mort_hip.h"
#include "dev_render.h"
#include "scene_blob.h"
#include "seed_host.h"
#include "mort_internal.h"
#include "mort_ctx.h"
#include "world_images.h"

/* ---- seeding: curand_init(seed, subsequence, 0) ---- */
struct SeedArgs {
    mort_rng_state *states;
    const uint32_t *mats; /* [levels][160][5]: A^(2^67 * 4^k), row i = image of state bit i */
    int levels;
    int width, local_rows, rank, nranks, rows_per_block;
    uint32_t d0, v0, v1, v2, v3, v4; /* scrambled seed */
    int sub; /* 0: the reference's keying, subsequence x + y*W.  S > 0 (MORT_MODE_THROUGHPUT): states[x + (ly*S + j)*W] gets subsequence x + (y*S + j)*W */
};

extern "C" __global__ void __launch_bounds__(256)
seed_kernel(const SeedArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int sub = a.sub > 0 ? a.sub : 1;
    const long long n = (long long)a.width * a.local_rows * sub;
    if (i >= n) return;
    const int vly = i / a.width, x = i - vly * a.width;
    const int ly = vly / sub, j = vly - ly * sub;
    const int y = global_row(ly, a.rank, a.nranks, a.rows_per_block);
    unsigned long long p = (unsigned long long)x + ((unsigned long long)y * (unsigned long long)sub + (unsigned long long)j) * (unsigned long long)a.width;
    uint32_t v[5] = {a.v0, a.v1, a.v2, a.v3, a.v4};
    for (int k = 0; p != 0 && k < a.levels; k++, p >>= 2) {
        const uint32_t *m = a.mats + (size_t)k * 160 * 5;
        const int reps = (int)(p & 3ull);
        for (int t = 0; t < reps; t++) {
            uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0;
            for (int wv = 0; wv < 5; wv++) {
                const uint32_t word = v[wv];
                for (int b = 0; b < 32; b++) {
                    const uint32_t mask = 0u - ((word >> b) & 1u);
                    const uint32_t *row = m + (wv * 32 + b) * 5;
                    r0 ^= row[0] & mask; r1 ^= row[1] & mask; r2 ^= row[2] & mask; r3 ^= row[3] & mask; r4 ^= row[4] & mask;
                }
            }
            v[0] = r0; v[1] = r1; v[2] = r2; v[3] = r3; v[4] = r4;
        }
    }
    a.states[i] = rng_state(a.d0, v[0], v[1], v[2], v[3], v[4]);
}

extern "C" const char *mort_hip_strerror(int st) {
    switch (st) {
    case MORT_OK: return "ok";
    case MORT_ERR_INVALID: return "invalid argument";
    case MORT_ERR_NO_DEVICE: return "no usable HIP device (gfx950 required)";
    case MORT_ERR_HIP: return "HIP runtime error";
    case MORT_ERR_NO_WORLD: return "no world uploaded";
    case MORT_ERR_NO_RNG: return "RNG states not seeded/loaded for this image size";
    case MORT_ERR_UNSUPPORTED: return "scene graph / mode not supported by the kernels";
    case MORT_ERR_CAPACITY: return "capacity exceeded";
    case MORT_ERR_NOMEM: return "out of memory";
    }
    return "unknown status";
}
extern "C" const char *mort_hip_last_error(const mort_ctx *c) { return c ? c->last_error.c_str() : ""; }

extern "C" int mort_hip_local_rows(const mort_ctx *c, int height) { return c ? local_rows_for(c->part, height) : 0; }
extern "C" int mort_hip_global_row(const mort_ctx *c, int ly) { return c ? global_row_host(c->part, ly) : 0; }

extern "C" int mort_hip_init(int device, mort_ctx **out) {
    if (!out) return MORT_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return MORT_ERR_NO_DEVICE;
    mort_ctx *c = new (std::nothrow) mort_ctx;
    if (!c) return MORT_ERR_NOMEM;
    c->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete c; return MORT_ERR_NO_DEVICE; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { delete c; return MORT_ERR_NO_DEVICE; }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) { delete c; return MORT_ERR_NO_DEVICE; }
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipMalloc(&c->d_counters, 96 * sizeof(unsigned long long)) != hipSuccess) {
        mort_hip_shutdown(c);
        return MORT_ERR_HIP;
    }
    *out = c;
    return MORT_OK;
}

extern "C" void mort_hip_shutdown(mort_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    quiesce(c);
    mort_views_free(c);
    mort_hip_comm_destroy(c);
    hipFree(c->d_tile_keys); hipFree(c->d_tile_iota); hipFree(c->d_sort_tmp);
    hipFree(c->d_prio_count); hipFree(c->d_scene); hipFree(c->d_fast); hipFree(c->d_trav); hipFree(c->d_gen); hipFree(c->d_states); hipFree(c->d_seqmats);
    hipFree(c->d_substates); hipFree(c->d_vaccum);
    hipFree(c->d_rgba); hipFree(c->d_accum); hipFree(c->d_segpx); hipFree(c->d_counters); hipFree(c->d_wf);
    hipFree(c->d_tile_cost); hipFree(c->d_tile_order); hipFree(c->d_probe_states); hipFree(c->d_deep); hipFree(c->d_wave_log);
    if (c->h_live) hipHostFree(c->h_live);
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

extern "C" int mort_hip_set_partition(mort_ctx *c, const mort_partition *p) {
    if (!c || !p) return MORT_ERR_INVALID;
    if (p->nranks < 1 || p->rank < 0 || p->rank >= p->nranks || p->rows_per_block < 8 || (p->rows_per_block % 8) != 0)
        return MORT_ERR_INVALID;
    hipSetDevice(c->device);
    quiesce(c);
    c->part = *p;
    c->cost_key = 0;
    /* RNG states are laid out per partition: force a re-seed */
    c->rng_w = c->rng_h = c->rng_local_rows = 0;
    c->sub_w = c->sub_h = c->sub_lr = c->sub_s = 0;
    return MORT_OK;
}

extern "C" int mort_hip_upload_world(mort_ctx *c, const mort_world *w) {
    if (!c || !w) return MORT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, quiesce(c));
    c->cost_key = 0; c->world_serial++;
    /* nothing of the previous world survives a failed upload: a later render must see MORT_ERR_NO_WORLD, not the old world's
     * trees walked against the new scene tables */
    c->have_world = c->fast_ok = c->gen_ok = c->wave_ok = false;
    if (c->d_fast) { hipFree(c->d_fast); c->d_fast = nullptr; }
    if (c->d_trav) { hipFree(c->d_trav); c->d_trav = nullptr; }
    if (c->d_gen) { hipFree(c->d_gen); c->d_gen = nullptr; }
    int st;
    SceneBlob sb;
    st = build_scene_blob(w, sb);
    if (st != MORT_OK) return st;
    const mortc::Compiled &o = sb.comp;
    void *d = nullptr;
    HIPCHK(c, hipMalloc(&d, sb.bytes.size()));
    hipError_t e = hipMemcpy(d, sb.bytes.data(), sb.bytes.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { hipFree(d); return hip_fail(c, e, "hipMemcpy(scene)"); }
    if (c->d_scene) hipFree(c->d_scene);
    c->d_scene = d;
    scene_view(sb, (const unsigned char *)d, c->sc);
    c->list_types = o.list_types; c->list_idxs = o.list_idxs;
    for (int i = 0; i < MORT_NUM_HITTABLE_LIST; i++) { c->list_first[i] = o.list_first[i]; c->list_count[i] = o.list_count[i]; }
    c->n_wspheres = (int)o.wspheres.size(); c->n_wquads = (int)o.wquads.size(); c->n_lists = w->objs.num_hittable_list;
    c->wave_ok = one_sphere_bvh(o);
    if (c->wave_ok && !o.own_nodes.empty() && !o.own_nodes4.empty()) {
        BvhImages im;
        build_bvh_images(o, im);
        const std::vector<unsigned char> &fb = im.fb, &tb = im.tb;
        c->bvh = im.off;
        if (im.fits) {
            HIPCHK(c, hipMalloc(&c->d_fast, fb.size()));
            HIPCHK(c, hipMemcpy(c->d_fast, fb.data(), fb.size(), hipMemcpyHostToDevice));
            HIPCHK(c, hipMalloc(&c->d_trav, tb.size()));
            HIPCHK(c, hipMemcpy(c->d_trav, tb.data(), tb.size(), hipMemcpyHostToDevice));
            c->fast_bytes = (uint32_t)fb.size(); c->trav_bytes = (uint32_t)tb.size();
            c->own_nodes = (int)o.own_nodes.size(); c->own_leaves = (int)o.own_leaves.size(); c->own4_stack = o.own4_stack > 1 ? o.own4_stack : 1;
            c->fast_ok = true;
        }
    }
    /* unified-tree megakernel: LDS image = tree + every small table (+ the primitives when they fit) */
    if (o.g_ok && !std::getenv("MORT_NO_GEN")) {
        GenImage gi;
        build_gen_image(o, gi);
        if (gi.fits) {
            const std::vector<unsigned char> &gb = gi.gb;
            GenArgs g = gi.g;
            HIPCHK(c, hipMalloc(&c->d_gen, gb.size()));
            HIPCHK(c, hipMemcpy(c->d_gen, gb.data(), gb.size(), hipMemcpyHostToDevice));
            c->gen_bytes = (uint32_t)gi.lds_part;
            g.ranks = (const uint32_t *)((const unsigned char *)c->d_gen + gi.o_ranks);
            c->gen = g;
            for (int k = 0; k < 3; k++) { c->gen_lo[k] = o.g_lo[k]; c->gen_hi[k] = o.g_hi[k]; }
            c->gen_reach = o.g_reach;
            c->gen_prims = (int)o.g_entries.size();
            c->gen_ok = true;
        }
    }
    c->have_world = true;
    return MORT_OK;
}

static int ensure_states(mort_ctx *c, int width, int height) {
    const int lr = local_rows_for(c->part, height);
    if (c->d_states && c->rng_w == width && c->rng_h == height && c->rng_local_rows == lr) return MORT_OK;
    if (c->d_states) { hipFree(c->d_states); c->d_states = nullptr; }
    c->rng_w = c->rng_h = c->rng_local_rows = 0;
    size_t n = (size_t)width * (size_t)(lr > 0 ? lr : 1);
    HIPCHK(c, hipMalloc((void **)&c->d_states, n * sizeof(mort_rng_state)));
    c->rng_w = width; c->rng_h = height; c->rng_local_rows = lr;
    return MORT_OK;
}

extern "C" int mort_hip_rng_seed(mort_ctx *c, uint64_t seed, int width, int height) {
    if (!c || width <= 0 || height <= 0) return MORT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_seqmats) {
        std::vector<XMat> seq;
        build_seq_matrices(seq);
        HIPCHK(c, hipMalloc((void **)&c->d_seqmats, seq.size() * sizeof(XMat)));
        HIPCHK(c, hipMemcpy(c->d_seqmats, seq.data(), seq.size() * sizeof(XMat), hipMemcpyHostToDevice));
    }
    HIPCHK(c, quiesce(c));
    int st = ensure_states(c, width, height);
    if (st != MORT_OK) return st;
    SeedArgs a;
    a.states = c->d_states; a.mats = c->d_seqmats; a.levels = SEQ_LEVELS;
    a.width = width; a.local_rows = c->rng_local_rows;
    a.rank = c->part.rank; a.nranks = c->part.nranks; a.rows_per_block = c->part.rows_per_block;
    const SeedWords sw = seed_scramble(seed);
    a.d0 = sw.d; a.v0 = sw.v[0]; a.v1 = sw.v[1]; a.v2 = sw.v[2]; a.v3 = sw.v[3]; a.v4 = sw.v[4];
    a.sub = 0;
    c->seed = seed; c->seed_known = true;
    c->sub_w = c->sub_h = c->sub_lr = c->sub_s = 0; /* a re-seed restarts the sub-streams too */
    const int n = width * c->rng_local_rows;
    if (n > 0) {
        hipLaunchKernelGGL(seed_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, a);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return MORT_OK;
}

extern "C" int mort_hip_rng_load(mort_ctx *c, const mort_rng_state *states, int width, int height) {
    if (!c || !states || width <= 0 || height <= 0) return MORT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, quiesce(c));
    int st = ensure_states(c, width, height);
    if (st != MORT_OK) return st;
    c->seed_known = false;
    c->sub_w = c->sub_h = c->sub_lr = c->sub_s = 0;
    for (int ly = 0; ly < c->rng_local_rows; ly++) {
        const int y = global_row_host(c->part, ly);
        HIPCHK(c, hipMemcpy(c->d_states + (size_t)ly * width, states + (size_t)y * width, (size_t)width * sizeof(mort_rng_state), hipMemcpyHostToDevice));
    }
    return MORT_OK;
}

extern "C" int mort_hip_rng_store(mort_ctx *c, mort_rng_state *states, int width, int height) {
    if (!c || !states || width <= 0 || height <= 0) return MORT_ERR_INVALID;
    if (!c->d_states || c->rng_w != width || c->rng_h != height) return MORT_ERR_NO_RNG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, quiesce(c));
    for (int ly = 0; ly < c->rng_local_rows; ly++) {
        const int y = global_row_host(c->part, ly);
        HIPCHK(c, hipMemcpy(states + (size_t)y * width, c->d_states + (size_t)ly * width, (size_t)width * sizeof(mort_rng_state), hipMemcpyDeviceToHost));
    }
    return MORT_OK;
}

/* MORT_MODE_THROUGHPUT: the (pixel, stratum row) streams for this image, partition and sqrt_spp; seeded once, then carried from
 * frame to frame like the per-pixel states */
int mort_ensure_substates(mort_ctx *c, int W, int H, int S, hipStream_t s) {
    const int lr = c->rng_local_rows;
    const size_t n = (size_t)W * (size_t)lr * (size_t)S;
    if (n >= (1ull << 31)) return MORT_ERR_CAPACITY;
    if (c->substates_cap < n) {
        if (c->d_substates) { hipFree(c->d_substates); c->d_substates = nullptr; }
        c->substates_cap = 0; c->sub_s = 0;
        HIPCHK(c, hipMalloc((void **)&c->d_substates, (n ? n : 1) * sizeof(mort_rng_state)));
        c->substates_cap = n;
    }
    if (c->vaccum_cap < n) {
        if (c->d_vaccum) { hipFree(c->d_vaccum); c->d_vaccum = nullptr; }
        c->vaccum_cap = 0;
        HIPCHK(c, hipMalloc((void **)&c->d_vaccum, (n ? n : 1) * 3 * sizeof(float)));
        c->vaccum_cap = n;
    }
    if (c->sub_w == W && c->sub_h == H && c->sub_lr == lr && c->sub_s == S) return MORT_OK;
    SeedArgs a;
    a.states = c->d_substates; a.mats = c->d_seqmats; a.levels = SEQ_LEVELS;
    a.width = W; a.local_rows = lr;
    a.rank = c->part.rank; a.nranks = c->part.nranks; a.rows_per_block = c->part.rows_per_block;
    const SeedWords sw = seed_scramble(c->seed);
    a.d0 = sw.d; a.v0 = sw.v[0]; a.v1 = sw.v[1]; a.v2 = sw.v[2]; a.v3 = sw.v[3]; a.v4 = sw.v[4];
    a.sub = S;
    if (n > 0) {
        hipLaunchKernelGGL(seed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
        HIPCHK(c, hipGetLastError());
    }
    c->sub_w = W; c->sub_h = H; c->sub_lr = lr; c->sub_s = S;
    return MORT_OK;
}
