/*
 * mort_hip.hip -- the render: mort_hip_render / mort_hip_render_device, the choice of the kernel family for a call, the
 * launches and their statistics.  The context, the world upload and the RNG streams are context.hip's, the diagnostics
 * debug.hip's, and what the launches decide from a world alone (images, LDS budgets) is world_images.h's.
 *
 * Kernels (hand-written for CDNA4, wave64):
 *   mega_kernel       one lane per pixel, 8x8 pixel tile per wave; the whole sample x bounce nest of Camera::render /
 *                     ray_color (camera.cuh:86-208) runs as ONE flat per-lane loop so that a lane whose path ends starts
 *                     its next sample immediately instead of idling until the longest path of the wave ends.  RNG state in
 *                     6 VGPRs for the pixel's lifetime; the first bounce-stack levels in LDS, the rest private; no global
 *                     scratch arrays (mort.cu:712-725).
 *   mega_bvh_kernel   (mega_bvh.h) the state-machine megakernel of worlds that are one reference BVH over spheres: lanes
 *                     take pixels from a pool and are scheduled by state (box step, leaf step, shade step); launch_bvh.
 *   wf_init, wf_trav, wf_shade   (wave_bvh.h) the wavefront pipeline of the same worlds, one launch pair per front; launch_wave.
 *   substream_resolve_kernel     sums the stratum rows of a MORT_MODE_THROUGHPUT launch into pixels.
 * The unified-tree kernels live in mega_gen.hip and wave_gen.hip: launch_gen takes its kernel from mort_gen_kernel,
 * FAM_WAVE_GEN goes through mort_wave_gen_render.
 */
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mort_hip.h"
#include "dev_pixel.h"
#include "scene_blob.h"
#include "mort_internal.h"
#include "mort_ctx.h"
#include "world_images.h"
#include "mega_gen.h"
#include "wave_gen.h"

#pragma clang fp contract(off)

/* ====================================================================== device */

/* 4 waves per SIMD: 128 registers and 9 bounce-stack levels in LDS (36 KB per workgroup, four workgroups per CU).  Without a bound the
 * compiler takes 172 registers (two waves); at three (148 registers, 12 levels) the Cornell box 800x800x1000 took 360 ms, at four 326 ms,
 * Cornell smoke 52.9 -> 47.2 ms -- a wave issues a dependent vector instruction only every ~8 cycles, so the fourth
 * wave outweighs the extra spills (this kernel keeps its deep stack levels in private memory either way) */
#ifndef MORT_GENERIC_WAVES
#define MORT_GENERIC_WAVES 4
#endif
#ifndef MORT_MEGA_LDS_LEVELS
#define MORT_MEGA_LDS_LEVELS 9
#endif
extern "C" __global__ void __launch_bounds__(256, MORT_GENERIC_WAVES)
mega_kernel(const RenderArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    const int tiles_x = (a.width + 7) >> 3;
    const int tx = wave % tiles_x, ty = wave / tiles_x;
    const int x = tx * 8 + (lane & 7);
    const int ly = ty * 8 + (lane >> 3);
    const bool active = (x < a.width) && (ly < a.local_rows);
    if (!active) return;

    __shared__ float4 s_stack[MORT_MEGA_LDS_LEVELS * 256]; /* the first bounce-stack levels of the block's 256 lanes: 36 KB, four blocks per CU */
    const PixelTotals t = render_pixel<false>(a, nullptr, x, ly, nullptr, s_stack + threadIdx.x, MORT_MEGA_LDS_LEVELS, 256); /* dev_pixel.h: the body the host loop runs too */
    atomicAdd(&a.counters[0], (unsigned long long)t.segments);
    atomicAdd(&a.counters[1], (unsigned long long)t.draws);
}

#include "mega_bvh.h"
#include "wave_bvh.h"

/* finishes the pixels of a sub-stream launch: stratum rows summed in order, then Camera::render's tail (camera.cuh:194-207) */
static __global__ void __launch_bounds__(256) substream_resolve_kernel(const float *vaccum, int width, int local_rows, int sub, float scale, uchar4 *rgba, float *accum) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= width * local_rows) return;
    const int ly = i / width, x = i - ly * width;
    V3 c = mk(0, 0, 0);
    for (int j = 0; j < sub; j++) {
        const size_t v = 3 * ((size_t)(ly * sub + j) * (size_t)width + (size_t)x);
        c = vadd(c, mk(vaccum[v], vaccum[v + 1], vaccum[v + 2]));
    }
    c = pixel_finish(scale, c);
    if (accum) { accum[3 * i] = c.x; accum[3 * i + 1] = c.y; accum[3 * i + 2] = c.z; }
    pixel_rgba(rgba[i], c);
}

/* ====================================================================== host */

/* ---- wavefront mode over one reference BVH of spheres: one wf_trav + one wf_shade launch per front (wave_common.h wf_render) ---- */
static int launch_wave(mort_ctx *c, const mort_camera *cam, const RenderArgs &a, hipStream_t s, LaunchPlan &plan) {
    WfArgs w;
    std::memset(&w, 0, sizeof w);
    w.r = a;
    w.node_first = 0; w.node_count = c->sc.n_nodes;
    auto trav = wf_trav<MORT_WF_BLOCK>;
    const size_t stage_bytes = (size_t)(MORT_WF_BLOCK / 64) * 3 * MORT_WF_STAGE * sizeof(unsigned);
    /* wf_trav's LDS: its image (binary own tree, leaf nodes, spheres) | traversal stacks | class staging | prefetch rings */
    w.trav_src = (const unsigned char *)c->d_trav; w.trav_bytes = c->trav_bytes;
    w.t_nodes2 = c->bvh.t_nodes2; w.t_leaves = c->bvh.t_leaves; w.t_spheres = c->bvh.t_spheres;
    w.t_tstack = (c->trav_bytes + 15u) & ~15u;
    w.t_stage = w.t_tstack + (uint32_t)MORT_OWN_STACK * (uint32_t)MORT_WF_BLOCK * 2u;
    const size_t ring_off = (((size_t)w.t_stage + stage_bytes) + 1023) & ~(size_t)1023;
    const size_t trav_lds = ring_off + (size_t)(MORT_WF_BLOCK / 64) * 4096;
    w.off_ring = (uint32_t)ring_off;
    int wf_share = 1; /* 64-record batches per wave at least (MORT_WAVE_SHARE; 2 was 4 % slower: a front's time is its slowest wave's) */
    knob_int_in(std::getenv("MORT_WAVE_SHARE"), 1, INT_MAX, wf_share);
    plan.kernel = (const void *)trav; plan.block = MORT_WF_BLOCK; plan.lds_bytes = (int)c->trav_bytes;
    std::snprintf(plan.name, sizeof plan.name, "wf_trav<%d>", MORT_WF_BLOCK);
    return wf_render(c, cam, (size_t)a.width * (size_t)a.local_rows, w, wf_init, trav, wf_shade, MORT_WF_BLOCK, trav_lds,
                     (size_t)(MORT_WF_BLOCK / 64) * 64 * (size_t)wf_share, s);
}

/* ---- tile order of the state-machine megakernels: most expensive 8x8 tiles first (cost = segments per tile in the
 * previous frame of this world / view / partition, or in a one-sample probe on a scratch copy of the streams), so a frame
 * does not end on its longest pixel chains.  Sub-stream launches are not ordered: their work items are a stratum row,
 * 1/sqrt_spp of a pixel -- no long tail to order away.  Everything is queued on `s`; nothing waits on the host.  Leaves
 * fa.tile_order null when it orders nothing. ---- */
template <typename ProbeFn>
static int prepare_tile_order(mort_ctx *c, const mort_camera *cam, const RenderArgs &a, FastArgs &fa, int tiles, int grid, int FB,
                              bool chain_bound, bool sub, bool timed, hipStream_t s, ProbeFn launch_probe) {
    if (sub || std::getenv("MORT_NO_TILE_ORDER") || tiles < 4 * grid) return MORT_OK;
    const int W = a.width, H = a.height;
    if (c->tile_cap < (size_t)tiles) {
        hipFree(c->d_tile_cost); hipFree(c->d_tile_order); hipFree(c->d_tile_keys); hipFree(c->d_tile_iota); hipFree(c->d_sort_tmp);
        c->d_tile_cost = c->d_tile_order = c->d_tile_keys = c->d_tile_iota = nullptr; c->d_sort_tmp = nullptr;
        c->tile_cap = 0; c->sort_tmp_bytes = 0;
        HIPCHK(c, hipMalloc((void **)&c->d_tile_cost, (size_t)tiles * sizeof(unsigned)));
        HIPCHK(c, hipMalloc((void **)&c->d_tile_order, (size_t)tiles * sizeof(unsigned)));
        HIPCHK(c, hipMalloc((void **)&c->d_tile_keys, (size_t)tiles * sizeof(unsigned)));
        HIPCHK(c, hipMalloc((void **)&c->d_tile_iota, (size_t)tiles * sizeof(unsigned)));
        c->sort_tmp_bytes = mort_tile_sort_temp_bytes(tiles);
        HIPCHK(c, hipMalloc(&c->d_sort_tmp, c->sort_tmp_bytes ? c->sort_tmp_bytes : 16));
        c->tile_cap = (size_t)tiles;
        c->cost_key = 0;
    }
    if (fa.heavy_mod > 0 && !c->d_prio_count) {
        HIPCHK(c, hipMalloc((void **)&c->d_prio_count, mort_ctx::prio_count_bytes));
        HIPCHK(c, hipMemsetAsync(c->d_prio_count, 0, mort_ctx::prio_count_bytes, s));
    }
    const char *tk = std::getenv("MORT_TILE_KEY");
    const int key_sum = (tk && std::strcmp(tk, "sum") == 0) ? 1 : 0;
    /* the costs belong to one (world, image geometry, partition, view): FNV-1a over all of it */
    unsigned long long key = 1469598103934665603ull;
    auto mix = [&key](const void *p, size_t n) { const unsigned char *b = (const unsigned char *)p; for (size_t i = 0; i < n; i++) { key ^= b[i]; key *= 1099511628211ull; } };
    { const int g[9] = {W, H, a.local_rows, a.rank, a.nranks, a.rows_per_block, cam->bounce_limit, (int)c->world_serial, a.light_type * 65536 + a.light_idx}; mix(g, sizeof g); }
    mix(&a.center, sizeof a.center); mix(&a.pixel00, sizeof a.pixel00); mix(&a.du, sizeof a.du); mix(&a.dv, sizeof a.dv);
    mix(&a.defocus_angle, sizeof a.defocus_angle);
    if (key == 0) key = 1;
    if (c->cost_key != key) { /* no history for this view: one-sample probe on a scratch copy of the streams */
        const size_t npx = (size_t)W * (size_t)a.local_rows;
        if (c->probe_cap < npx) {
            if (c->d_probe_states) { hipFree(c->d_probe_states); c->d_probe_states = nullptr; c->probe_cap = 0; }
            HIPCHK(c, hipMalloc((void **)&c->d_probe_states, npx * sizeof(mort_rng_state)));
            c->probe_cap = npx;
        }
        HIPCHK(c, hipMemcpyAsync(c->d_probe_states, c->d_states, npx * sizeof(mort_rng_state), hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemsetAsync(c->d_tile_cost, 0, (size_t)tiles * sizeof(unsigned), s));
        FastArgs pa = fa;
        pa.r.states = c->d_probe_states; pa.r.sqrt_spp = 1; pa.r.recip_sqrt_spp = 1.0f; pa.r.pixel_samples_scale = 1.0f;
        pa.r.accum = nullptr; pa.r.seg_px = nullptr;
        pa.tile_order = nullptr; pa.tile_cost = c->d_tile_cost;
        pa.tile_key_sum = key_sum;
        HIPCHK(c, launch_probe(pa));
        if (c->d_prio_count) HIPCHK(c, hipMemcpyAsync(c->d_prio_count + 4, c->d_counters, 96 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s)); /* the probe's counters (pixel_write<true> adds its segments to the per-workgroup slots), beside its tile costs */
        HIPCHK(c, hipMemsetAsync(c->d_counters, 0, 96 * sizeof(unsigned long long), s)); /* probe totals and work cursor */
        c->cost_key = key;
        c->tile_launch.probed = 1;
    }
    /* order = argsort(cost, descending, equal costs by index), on the device and on this stream */
    HIPCHK(c, mort_tile_sort_desc(c->d_tile_cost, c->d_tile_keys, c->d_tile_iota, c->d_tile_order, c->d_sort_tmp, c->sort_tmp_bytes, tiles, s));
    /* the head of the order: tiles whose longest pixel reaches heavy_percent % of the frame's longest (unified-tree kernel's heavy waves) */
    fa.prio_dev = nullptr;
    if (fa.heavy_mod > 0) {
        /* d_prio_count: [0] the head's size for this launch (u32); from byte 16: the 96 counters of the frame (or probe) the tile costs come from */
        HIPCHK(c, mort_tile_heavy_count(c->d_tile_keys, tiles, (unsigned)c->heavy_percent, (unsigned)(tiles / 2 > 0 ? tiles / 2 : 1),
                                        (const unsigned long long *)(c->d_prio_count + 4), (unsigned long long)grid * (unsigned long long)FB, c->d_prio_count, s));
        fa.prio_dev = c->d_prio_count;
        /* diagnostic: the counters as the kernel above read them (launch_gen overwrites them after the frame) */
        HIPCHK(c, hipMemcpyAsync(c->d_prio_count + 4 + 192, c->d_prio_count + 4, 96 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
        c->tile_launch.has_head = 1;
    }
    HIPCHK(c, hipMemsetAsync(c->d_tile_cost, 0, (size_t)tiles * sizeof(unsigned), s));
    fa.tile_order = c->d_tile_order; fa.tile_cost = c->d_tile_cost;
    fa.tile_key_sum = key_sum;
    fa.gen_tiles = grid * (FB / 64); /* one tile's worth of slots per wave in flight */
    fa.spread_shift = chain_bound ? 0 : 6; /* measured: whole tiles while lanes refill several times, single pixels otherwise */
    knob_int(std::getenv("MORT_SPREAD_SHIFT"), fa.spread_shift);
    if (fa.spread_shift >= 6 || fa.spread_shift < 0) fa.gen_tiles = 0;
    c->tile_launch.ordered = 1; c->tile_launch.key_sum = key_sum; c->tile_launch.spread_shift = fa.spread_shift; c->tile_launch.gen_tiles = fa.gen_tiles;
    if (timed) HIPCHK(c, hipEventRecord(c->ev0, s)); /* time the frame itself; ordering upkeep is reported by wall-clock benches */
    return MORT_OK;
}

/* ---- the two state-machine megakernels (mega_bvh_kernel, mega_gen_kernel): what their launches share ---- */

/* the FastArgs fields both fill alike: camera / buffers, LDS image source, work cursor, tiles, sub-streams, lane cap */
static void fast_args_base(const mort_ctx *c, const mort_camera *cam, const RenderArgs &a, FastArgs &fa, const void *image, uint32_t image_bytes,
                           int tiles, bool sub) {
    fa.r = a;
    fa.hot_src = (const unsigned char *)image; fa.hot_bytes = image_bytes;
    fa.next_q = (unsigned int *)(c->d_counters + 2);
    fa.tiles_x = (a.width + 7) / 8; fa.tiles_total = tiles;
    if (sub) { fa.sub = cam->sqrt_spp; fa.vaccum = c->d_vaccum; fa.r.states = c->d_substates; }
    fa.lane_cap = 64;
    knob_int_in(std::getenv("MORT_LANE_CAP"), 1, 64, fa.lane_cap);
}

/* LDS, grid and HBM scratch of a launch of `kern` in FB-thread groups.  LDS: the image (fa.hot_bytes) | traversal stacks
 * [tstack_levels][FB] u16 | as many bounce-stack levels [dl][FB] float4 as fit next to them (world_images.h state_lds_levels), at least dl_min, at most 12 and dl_cap, with as many
 * groups per CU as keep 12 waves per CU (fewer when their LDS does not fit 160 KB) and at most per_cu_cap.  The levels below dl
 * go to c->d_deep; MORT_WAVE_LINES (profile builds) sizes the per-wave log. */
static int state_setup(mort_ctx *c, const mort_camera *cam, FastArgs &fa, const void *kern, int FB, uint32_t tstack_levels, int dl_min, int dl_cap,
                       int per_cu_cap, const char *too_big, hipStream_t s, size_t &lds_bytes, int &grid) {
    uint32_t static_lds = 1024; /* the kernel's own __shared__ objects come out of the same 160 KB */
    { hipFuncAttributes fattr; if (hipFuncGetAttributes(&fattr, kern) == hipSuccess) static_lds = (uint32_t)((fattr.sharedSizeBytes + 1023) & ~(size_t)1023); }
    uint32_t tstack_off = 0, stack_off = 0;
    int dl = state_lds_levels(fa.hot_bytes, FB, tstack_levels, static_lds, dl_min, tstack_off, stack_off);
    fa.off_tstack = tstack_off;
    if (dl < 0) { c->last_error = too_big; return MORT_ERR_CAPACITY; }
    if (dl > dl_cap) dl = dl_cap;
    fa.off_stack = stack_off; fa.stack_lds_depth = dl;
    lds_bytes = (size_t)stack_off + (size_t)dl * FB * 16;
    HIPCHK(c, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, FB, lds_bytes) != hipSuccess || per_cu < 1) per_cu = 1;
    if (per_cu > per_cu_cap) per_cu = per_cu_cap;
    grid = c->num_cus * per_cu;
    const int want_blocks = (int)(((long long)fa.tiles_total * 64 + FB - 1) / FB);
    if (grid > want_blocks) grid = want_blocks;
    if (grid < 1) grid = 1;
    /* bounce-stack levels that do not fit in LDS: [level - dl][lane of the launch] in HBM */
    const int deep_levels = cam->bounce_limit > dl ? cam->bounce_limit - dl : 0;
    const int st = ensure_buf(c, &c->d_deep, &c->deep_cap, (size_t)(deep_levels > 0 ? deep_levels : 1) * (size_t)grid * (size_t)FB * sizeof(float4));
    if (st != MORT_OK) return st;
    fa.deep = (float4 *)c->d_deep;
    fa.wave_log = nullptr;
    if (std::getenv("MORT_WAVE_LINES")) { /* profile builds: 16 words per wave, read back by mort_hip_debug_wave_log */
        c->wave_log_waves = (size_t)grid * (size_t)(FB / 64);
        if (ensure_buf(c, &c->d_wave_log, &c->wave_log_cap, c->wave_log_waves * 16 * sizeof(unsigned long long)) == MORT_OK) {
            hipMemsetAsync(c->d_wave_log, 0, c->wave_log_waves * 16 * sizeof(unsigned long long), s);
            fa.wave_log = (unsigned long long *)c->d_wave_log;
        }
    }
    return MORT_OK;
}

/* mega_bvh_kernel<BLOCK, PROBE, DRAIN, SUB> for a launch shape (1024-thread groups have no DRAIN variant; a probe is neither DRAIN
 * nor SUB).  Written so that the device code object lists the variants in the order it always has. */
typedef void (*bvh_kernel_t)(const FastArgs);
static bvh_kernel_t bvh_kernel(int FB, bool probe, bool drain, bool sub) {
    if (!sub) switch (FB) {
        case 1024: return !probe ? mega_bvh_kernel<1024, false, false> : mega_bvh_kernel<1024, true, false>;
        case 768: return probe ? mega_bvh_kernel<768, true, false> : drain ? mega_bvh_kernel<768, false, true> : mega_bvh_kernel<768, false, false>;
        case 512: return probe ? mega_bvh_kernel<512, true, false> : drain ? mega_bvh_kernel<512, false, true> : mega_bvh_kernel<512, false, false>;
        case 384: return probe ? mega_bvh_kernel<384, true, false> : drain ? mega_bvh_kernel<384, false, true> : mega_bvh_kernel<384, false, false>;
        default: return probe ? mega_bvh_kernel<256, true, false> : drain ? mega_bvh_kernel<256, false, true> : mega_bvh_kernel<256, false, false>;
    }
    return FB == 1024 ? mega_bvh_kernel<1024, false, false, true> : FB == 768 ? mega_bvh_kernel<768, false, false, true> : FB == 512 ? mega_bvh_kernel<512, false, false, true>
           : FB == 384 ? mega_bvh_kernel<384, false, false, true> : mega_bvh_kernel<256, false, false, true>;
}

/* ---- the BVH megakernel (mega_bvh.h): one reference BVH as the world, its own four-wide tree in LDS ---- */
static int launch_bvh(mort_ctx *c, const mort_camera *cam, const RenderArgs &a, int tiles, bool sub, bool timed, hipStream_t s, LaunchPlan &plan) {
    FastArgs fa;
    std::memset(&fa, 0, sizeof fa);
    fast_args_base(c, cam, a, fa, c->d_fast, c->fast_bytes, tiles, sub);
    const BvhOffsets &o = c->bvh;
    fa.off_nodes4 = o.f_nodes4; fa.off_leafrecs = o.f_leafrecs; fa.off_lambert = o.f_lambert; fa.off_metal = o.f_metal;
    fa.off_diel = o.f_diel; fa.off_dlight = o.f_dlight; fa.off_iso = o.f_iso; fa.off_solid = o.f_solid; fa.off_checker = o.f_checker;
    fa.node_first = 0; fa.node_count = c->sc.n_nodes; /* the reference's threaded nodes (HBM): fallback walk */
    const long long lanes_wanted = (long long)tiles * 64;
    const double px_per_lane = (double)lanes_wanted / ((double)c->num_cus * 768.0);
    /* workgroup size.  Two pixels per lane or more: 1024 threads, compiled for 128 registers = 16 waves per CU.  A wave issues a
     * dependent vector instruction every ~8 cycles and an independent one every ~5 (calibration), a SIMD can issue one
     * every ~1.2: a fourth wave per SIMD is worth more than the 24 registers the 1024-thread build keeps in private memory, all of
     * them touched in the shade step only (Scene 1: 103.7 ms against 111.9 ms with 768 threads at 153 registers).
     * Otherwise the largest of {768, 512, 384, 256} that still gives every CU a workgroup
     * (a rank of an 8-way partition owns ~100 k pixels: 768-thread groups would leave half the CUs idle) */
    int FB = MORT_FAST_BLOCK;
    if (!knob_int(std::getenv("MORT_FAST_BLOCK_SIZE"), FB)) {
        const int cand[4] = {768, 512, 384, 256};
        FB = 256;
        const bool wide_ok = lanes_wanted >= 2ll * 1024 * c->num_cus;
        /* about one pixel per lane or fewer: the frame is as long as its longest pixel chain, so take the drain kernels that are
         * compiled without spills (<= 512 threads; one rank of 4 at 1200x675: 81 ms vs 90 ms with 768) */
        for (int k = (px_per_lane < 1.5 && !sub) ? 1 : 0; k < 4; k++) if (lanes_wanted >= (long long)cand[k] * c->num_cus) { FB = cand[k]; break; }
        if (wide_ok) FB = 1024;
    }
    /* 1024 threads: image + traversal stacks + one bounce-stack level per lane must fit one CU's LDS, else the widest shape that does */
    if (FB == 1024 && !bvh_wide_block_fits(fa.hot_bytes, c->own4_stack)) FB = 768;
    if (FB != 1024 && FB != 768 && FB != 512 && FB != 384) FB = 256;
    fa.drain_rounds = 3; /* batch thresholds as shares of the wave's LIVE lanes (they differ from fixed counts only once lanes have run out of pixels: the tail of a frame;
                          * three runs each, one box: N = 1 100.1-100.5 vs 100.3-102.9 ms, a rank of 2 75.6-78.6 vs 77.6-82.2 ms, ranks of 4 / 8 unchanged); DRAIN kernels
                          * also follow the lane furthest behind (round 2).  MORT_BVH_DRAIN: 0 / 1 = fixed counts, 2 = rounds, 3 = this */
    { int dm = 0; if (knob_int(std::getenv("MORT_BVH_DRAIN"), dm)) fa.drain_rounds = dm == 2 ? 1 : dm == 3 ? 3 : 0; }
    /* chain-bound partition (about one pixel per lane or fewer): drain mode + spread fetches (mega_bvh.h); no drain variant at 1024
     * threads: chain-bound partitions take <= 512 */
    bool chain_bound = px_per_lane < 1.5 && !sub;
    if (!sub) knob_flag(std::getenv("MORT_CHAIN_BOUND"), chain_bound);
    if (FB == 1024) chain_bound = false;
    const bvh_kernel_t kern = bvh_kernel(FB, false, chain_bound, sub), kern_probe = bvh_kernel(FB, true, false, false);
    /* scheduling thresholds (mega_bvh.h).  Smaller batches do not help a chain-bound partition: measured on
     * one rank of 8, (32,24,16) 100 ms, (12,12,8) 126 ms, (2,2,2) 192 ms -- a lane waits through every step
     * its wave runs for other lanes, and small batches mean more of those */
    fa.th_s = MORT_TH_S; fa.th_l = MORT_TH_L; fa.t_keep = MORT_T_KEEP;
    { int th[3]; if (knob_ints(std::getenv("MORT_THRESHOLDS"), 3, 1, th)) { fa.th_s = th[0]; fa.th_l = th[1]; fa.t_keep = th[2]; } } /* "s,l,k" */
    int per_cu_cap = INT_MAX;
    knob_int_in(std::getenv("MORT_FAST_BLOCKS_PER_CU"), 1, INT_MAX, per_cu_cap);
    /* traversal stacks: the world's own four-wide bound (at most MORT_OWN4_STACK) */
    size_t lds_bytes = 0;
    int grid = 0;
    int st = state_setup(c, cam, fa, (const void *)kern, FB, (uint32_t)c->own4_stack + MORT_BVH_TSTACK_SPARE, 1, 12, per_cu_cap, "BVH image does not fit one CU's LDS", s, lds_bytes, grid);
    if (st != MORT_OK) return st;
    c->tile_launch.grid = grid; c->tile_launch.block = FB;
    st = prepare_tile_order(c, cam, a, fa, tiles, grid, FB, chain_bound, sub, timed, s, [&](const FastArgs &pa) {
        hipError_t e_ = hipFuncSetAttribute((const void *)kern_probe, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e_ != hipSuccess) return e_;
        hipLaunchKernelGGL(kern_probe, dim3(grid), dim3(FB), lds_bytes, s, pa);
        return hipGetLastError();
    });
    if (st != MORT_OK) return st;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(FB), lds_bytes, s, fa);
    HIPCHK(c, hipGetLastError());
    plan.kernel = (const void *)kern; plan.block = FB; plan.lds_bytes = (int)lds_bytes;
    std::snprintf(plan.name, sizeof plan.name, "mega_bvh_kernel<%d, false, %s, %s>", FB, chain_bound ? "true" : "false", sub ? "true" : "false");
    return MORT_OK;
}

/* ---- the unified-tree megakernel (mega_gen.hip): every world without reference BVHs ---- */
static int launch_gen(mort_ctx *c, const mort_camera *cam, const RenderArgs &a, int tiles, bool sub, bool timed, hipStream_t s, LaunchPlan &plan) {
    GenArgs ga = c->gen; /* LDS image offsets, root, far-ray constants (upload_world) */
    FastArgs &fa = ga.f;
    fast_args_base(c, cam, a, fa, c->d_gen, c->gen_bytes, tiles, sub);
    const long long lanes_wanted = (long long)tiles * 64;
    int FB = 768;
    bool heavy_default = false;
    if (sub || !knob_int(std::getenv("MORT_GEN_BLOCK_SIZE"), FB)) {
        /* many pixels per lane: 1024 threads compiled for 128 registers = four waves per SIMD, which pays for its spills as in the BVH
         * kernel (4096 x 4096 x 4: 126.6 ms, 768 threads at 160 registers 137.5 ms, 512 threads 181 ms; 1920 x 1080 x 49: 173 vs 175 ms).
         * With a handful of pixels per lane the frame ends with its longest pixel chains, whose rounds are faster with two waves per
         * SIMD and no spills (final scene 800 x 800 x 961: 3.07 s with 512 threads, 3.21 s with 1024); fewer pixels than lanes:
         * 256-thread groups so every CU has work */
        const double ppl = (double)lanes_wanted / ((double)c->num_cus * 768.0);
        FB = ppl >= 8.0 ? 1024 : (lanes_wanted >= 512ll * c->num_cus) ? 512 : 256;
        /* fewer pixels per lane: the frame may be bound by its longest pixel chains, and then HEAVY WAVES pay (below): 1024 threads, the launch decides on the device */
        if (ppl < 8.0 && lanes_wanted >= 32ll * 1024 && !std::getenv("MORT_GEN_NO_HEAVY")) { FB = 1024; heavy_default = true; }
    }
    if (FB != 1024 && FB != 768 && FB != 512 && FB != 256) FB = 256;
    if (FB == 1024 && (size_t)c->gen_bytes + 16u + (size_t)MORT_OWN_STACK * 1024u * 2u + 2048u > 160u * 1024u) FB = 768; /* image + traversal stacks of 1024 threads must fit */
    if (sub && FB > 512) FB = 512; /* the non-parity launch is instantiated for 512- and 256-thread workgroups */
    /* swept on the final scene, 800x800x100 (scripts/th_sweep.py, 180 settings): 373 ms here vs 449 ms with the BVH kernel's (40,24,12) and m = 24 */
    fa.th_s = 28; fa.th_l = 20; fa.t_keep = 4; ga.th_m = 56;
    /* heavy waves (mega_bvh.h FastArgs.heavy_*): "mod,num,cap,percent" */
    fa.heavy_mod = 0; fa.heavy_num = 0; fa.heavy_cap = 64; c->heavy_percent = 50;
    /* default where the frame has fewer than 8 pixels per lane: two waves of three take 12 lanes each from the tiles whose longest pixel reaches half of the frame's
     * longest -- IF the device finds the frame chain-bound (tile_sort.hip heavy_count_kernel); final scene 800x800x961: 3.04 -> 2.55 s, x100: 318 -> 270 ms */
    if (heavy_default && FB == 1024 && !sub) { fa.heavy_mod = 3; fa.heavy_num = 2; fa.heavy_cap = 12; }
    { int hv[4];
      if (!sub && knob_ints(std::getenv("MORT_GEN_HEAVY"), 4, 1, hv) && hv[1] <= hv[0] && hv[2] <= 64 && hv[3] <= 100) {
          fa.heavy_mod = hv[0]; fa.heavy_num = hv[1]; fa.heavy_cap = hv[2]; c->heavy_percent = hv[3]; } }
    ga.drain_mode = 3; /* thresholds as shares of the live lanes; measured alternatives: 0 = fixed counts, 1 = follow one lane, 2 = rounds */
    knob_int_in(std::getenv("MORT_GEN_DRAIN"), 0, 3, ga.drain_mode); /* other values: the default */
    /* thresholds below 1 are refused: with t_keep < 1 a box-step loop whose lanes have all left the tree would never end */
    { int th[4]; if (knob_ints(std::getenv("MORT_GEN_THRESHOLDS"), 4, 1, th)) { fa.th_s = th[0]; fa.th_l = th[1]; fa.t_keep = th[2]; ga.th_m = th[3]; } } /* "s,l,k,m" */
    const gen_kernel_t kern = mort_gen_kernel(FB, ga.prims_in_lds != 0, sub);
    int dl_cap = 12;
    if (knob_int(std::getenv("MORT_GEN_DL"), dl_cap) && dl_cap < 0) dl_cap = 0; /* a negative count would shrink the LDS below the traversal stacks */
    size_t lds_bytes = 0;
    int grid = 0;
    int st = state_setup(c, cam, fa, (const void *)kern, FB, MORT_OWN_STACK, 0, dl_cap, INT_MAX, "unified-tree image does not fit one CU's LDS", s, lds_bytes, grid);
    if (st != MORT_OK) return st;
    c->tile_launch.grid = grid; c->tile_launch.block = FB;
    c->tile_launch.heavy[0] = fa.heavy_mod; c->tile_launch.heavy[1] = fa.heavy_num; c->tile_launch.heavy[2] = fa.heavy_cap; c->tile_launch.heavy[3] = c->heavy_percent;
    st = prepare_tile_order(c, cam, a, fa, tiles, grid, FB, false, sub, timed, s, [&](const FastArgs &pa) {
        GenArgs pg = ga;
        pg.f = pa;
        pg.probe = 1;
        hipError_t e_ = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e_ != hipSuccess) return e_;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(FB), lds_bytes, s, pg);
        return hipGetLastError();
    });
    if (st != MORT_OK) return st;
    /* priority pixels (mega_bvh.h FastArgs), with a tile order only: the head of the cost order, a few per wave.  A frame with a handful
     * of pixels per lane ends when its longest pixel chain does (final scene 800x800: the fog ball's pixels run 8 x the mean), and a chain
     * advances one segment per round of its wave: such a pixel must not share its wave with 63 others of its kind, and its wave must follow it */
    if (fa.tile_order) {
        int k_prio = 0; /* measured, not the default: following one lane starves the other 63 of a tile whose pixels are all long */
        knob_int(std::getenv("MORT_GEN_PRIO_LANES"), k_prio);
        if (k_prio > 0 && ga.drain_mode == 1) {
            const long long waves = (long long)grid * (FB / 64);
            long long pt = (waves * k_prio + 63) / 64;
            if (pt > tiles / 4) pt = tiles / 4;
            fa.prio_tiles = (int)pt; fa.prio_lanes = k_prio;
        }
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(FB), lds_bytes, s, ga);
    HIPCHK(c, hipGetLastError());
    if (fa.heavy_mod > 0 && c->d_prio_count && std::getenv("MORT_GEN_HEAVY_DEBUG")) { /* diagnostic: what the device decided for this launch */
        unsigned h[4] = {0, 0, 0, 0};
        HIPCHK(c, hipStreamSynchronize(s));
        HIPCHK(c, hipMemcpy(h, c->d_prio_count, 16, hipMemcpyDeviceToHost));
        std::fprintf(stderr, "[heavy] head tiles %u of %d, lanes %d\n", h[0], tiles, grid * FB);
    }
    if (fa.heavy_mod > 0 && c->d_prio_count) /* this frame's segment total, beside the tile costs it leaves for the next frame's order */
        HIPCHK(c, hipMemcpyAsync(c->d_prio_count + 4, c->d_counters, 96 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
    plan.kernel = (const void *)kern; plan.block = FB; plan.lds_bytes = (int)lds_bytes;
    std::snprintf(plan.name, sizeof plan.name, "mega_gen_kernel<%d, %s, %s>", FB, ga.prims_in_lds ? "true" : "false", sub ? "true" : "false"); /* as rocprofv3 prints it: <BLOCK, PRIMS_LDS, SUB> */
    return MORT_OK;
}

/* the kernel family that renders this call, or the status the call fails with (arguments, world and RNG already checked) */
static int choose_family(const mort_ctx *c, const mort_camera *cam, int mode, bool seg_px, RenderFamily &fam) {
    const int W = cam->image_width, H = cam->image_height;
    bool force = false;
    knob_flag(std::getenv("MORT_FORCE_GENERIC"), force);
    const bool state_ok = cam->sqrt_spp >= 1 && cam->sqrt_spp < 32768 && cam->bounce_limit >= 1 && W < 65536 && H < 32768 && !force;
    /* rays start on the lens: the unified tree serves cameras within its reach widened by the lens radius */
    const float rad = std::fabs(cam->defocus_disk_u.e[0]) + std::fabs(cam->defocus_disk_u.e[1]) + std::fabs(cam->defocus_disk_u.e[2]) +
                      std::fabs(cam->defocus_disk_v.e[0]) + std::fabs(cam->defocus_disk_v.e[1]) + std::fabs(cam->defocus_disk_v.e[2]);
    const bool gen_reach = c->gen_ok && camera_in_reach(cam, c->gen_lo, c->gen_hi, c->gen_reach, rad);
    if (mode == MORT_MODE_WAVE) {
        /* the wavefront pipeline: wave_bvh.h for one reference BVH of spheres as the world (no light object), wave_gen.hip for
         * every world with a unified tree (lights, quads, instances, media); anything else is not supported in this mode */
        if (!(cam->sqrt_spp >= 1 && cam->sqrt_spp < 4096 && cam->bounce_limit >= 1)) return MORT_ERR_UNSUPPORTED;
        if (c->wave_ok && c->fast_ok && cam->light_obj_type == -1) fam = FAM_WAVE;
        else if (gen_reach) fam = FAM_WAVE_GEN;
        else return MORT_ERR_UNSUPPORTED;
        return MORT_OK;
    }
    const bool use_fast = c->fast_ok && cam->light_obj_type == -1 && state_ok;
    /* the unified-tree megakernel: worlds without reference BVHs.  Small worlds stay on the one-lane-per-pixel kernel: scanning a
     * dozen primitives in lockstep keeps every lane busy, a tree walk scheduled by state does not (Cornell box 800x800x100: 53 ms
     * vs 83 ms) */
    bool use_gen = !use_fast && state_ok && gen_reach;
    if (use_gen) {
        int min_prims = 48;
        knob_int(std::getenv("MORT_GEN_MIN_PRIMS"), min_prims);
        if (c->gen_prims < min_prims) use_gen = false;
    }
    if (mode == MORT_MODE_THROUGHPUT) {
        if (!(use_fast || use_gen) || seg_px) return MORT_ERR_UNSUPPORTED; /* the two LDS state-machine kernels only */
        if (!c->seed_known) return MORT_ERR_NO_RNG;
        if ((long long)c->rng_local_rows * cam->sqrt_spp >= 32768ll * 64) return MORT_ERR_CAPACITY;
    }
    fam = use_fast ? FAM_BVH : use_gen ? FAM_GEN : FAM_MEGA;
    return MORT_OK;
}

#ifdef MORT_PROFILE_STATES
/* profile builds: the state counters of the launch (mega_bvh.h, mega_gen.hip, wave_bvh.h PROF_*) */
static void print_profile(const mort_ctx *c, RenderFamily fam, const unsigned long long *cnt) {
    if (fam == FAM_WAVE || fam == FAM_WAVE_GEN) {
        const char *nm[3] = {"T", "L", "F"};
        const double tot = (double)(cnt[12] + cnt[13] + cnt[14] + cnt[15]);
        for (int k = 0; k < 3; k++)
            std::fprintf(stderr, "[wf_trav %s] %10llu wave-steps  util %5.1f%%  cycles %5.1f%% (%.0f/step)\n", nm[k], cnt[4 + k],
                         cnt[4 + k] ? 100.0 * (double)cnt[8 + k] / (64.0 * (double)cnt[4 + k]) : 0.0, 100.0 * (double)cnt[12 + k] / tot,
                         cnt[4 + k] ? (double)cnt[12 + k] / (double)cnt[4 + k] : 0.0);
        std::fprintf(stderr, "[wf_trav sched] cycles %5.1f%%   fronts %d\n", 100.0 * (double)cnt[15] / tot, c->wf_fronts);
        std::fprintf(stderr, "[wf_trav waves] %llu waves, mean lifetime %.1f us, in-loop cycles per wave %.0f\n", cnt[21],
                     cnt[21] ? (double)cnt[20] / (double)cnt[21] * 0.01 : 0.0, cnt[21] ? tot / (double)cnt[21] : 0.0);
    } else if (fam == FAM_GEN) {
        const char *nm[4] = {"T", "L", "M", "S"};
        unsigned long long segs = cnt[0];
        for (int k = 0; k < 32; k++) segs += cnt[32 + 2 * k];
        const double tot = (double)(cnt[12] + cnt[13] + cnt[14] + cnt[15] + cnt[16]);
        for (int k = 0; k < 4; k++)
            std::fprintf(stderr, "[gen %s] %12llu wave-steps  lanes %5.1f%%  cycles %5.1f%% (%.0f/step)\n", nm[k], cnt[4 + 2 * k],
                         cnt[4 + 2 * k] ? 100.0 * (double)cnt[5 + 2 * k] / (64.0 * (double)cnt[4 + 2 * k]) : 0.0, 100.0 * (double)cnt[12 + k] / tot,
                         cnt[4 + 2 * k] ? (double)cnt[12 + k] / (double)cnt[4 + 2 * k] : 0.0);
        std::fprintf(stderr, "[gen S parts, cycles per S step] scan+decode %.0f  shade call %.0f  stack store %.0f  finish %.0f  newpix %.0f  newray %.0f\n", (double)cnt[24] / (double)cnt[10],
                     (double)cnt[25] / (double)cnt[10], (double)cnt[20] / (double)cnt[10], (double)cnt[21] / (double)cnt[10], (double)cnt[22] / (double)cnt[10], (double)cnt[23] / (double)cnt[10]);
        std::fprintf(stderr, "[gen sched] cycles %5.1f%%; leaf loop: %.2f iterations per L step, %.1f lanes per iteration; scans %llu; steps per segment: T %.2f L %.2f M %.2f S %.2f\n",
                     100.0 * (double)cnt[16] / tot, cnt[6] ? (double)cnt[17] / (double)cnt[6] : 0.0, cnt[17] ? (double)cnt[18] / (double)cnt[17] : 0.0, cnt[3],
                     (double)cnt[5] / (double)(segs + 1), (double)cnt[7] / (double)(segs + 1), (double)cnt[9] / (double)(segs + 1), (double)cnt[11] / (double)(segs + 1));
    } else if (fam == FAM_BVH) {
        const char *nm[3] = {"T", "L", "S"};
        for (int k = 0; k < 3; k++)
            std::fprintf(stderr, "[states] %s: %llu wave-steps, %llu lane-steps, utilisation %.1f%%\n", nm[k], cnt[4 + 2 * k], cnt[5 + 2 * k],
                         cnt[4 + 2 * k] ? 100.0 * (double)cnt[5 + 2 * k] / (64.0 * (double)cnt[4 + 2 * k]) : 0.0);
        std::fprintf(stderr, "[states] box-step runs: %llu (%.1f steps per run)\n", cnt[30], cnt[30] ? (double)cnt[4] / (double)cnt[30] : 0.0);
        const double tot = (double)(cnt[10] + cnt[11] + cnt[12] + cnt[13]);
        std::fprintf(stderr, "[cycles] T %.1f%% (%.0f/step)  L %.1f%% (%.0f/step)  S %.1f%% (%.0f/step)  sched %.1f%%  total wave-cycles %.3g\n",
                     100.0 * cnt[10] / tot, (double)cnt[10] / (double)cnt[4], 100.0 * cnt[11] / tot, (double)cnt[11] / (double)cnt[6],
                     100.0 * cnt[12] / tot, (double)cnt[12] / (double)cnt[8], 100.0 * cnt[13] / tot, tot);
#ifdef MORT_PROFILE_FINE
        std::fprintf(stderr, "[S shade parts, cycles/step] verify %.0f  hit record %.0f  metal %.0f  dielectric %.0f  lambert texture %.0f  lambert scatter %.0f  light %.0f  (rest of 'shade' below: stack store)\n",
                     (double)cnt[18] / (double)cnt[8], (double)cnt[19] / (double)cnt[8], (double)cnt[20] / (double)cnt[8], (double)cnt[21] / (double)cnt[8],
                     (double)cnt[22] / (double)cnt[8], (double)cnt[23] / (double)cnt[8], (double)cnt[24] / (double)cnt[8]);
#else
        const char *bn[5] = {"metal", "dielectric", "lambertian", "finish", "get_ray"};
        for (int k = 0; k < 5; k++)
            std::fprintf(stderr, "[S branch] %-16s entered in %5.1f%% of S steps (x%.2f), %4.1f lanes when entered\n", bn[k],
                         100.0 * (double)cnt[18 + 2 * k] / (double)cnt[8], (double)cnt[18 + 2 * k] / (double)cnt[8],
                         cnt[18 + 2 * k] ? (double)cnt[19 + 2 * k] / (double)cnt[18 + 2 * k] : 0.0);
        /* mega_bvh_kernel: cnt[28 / 29] unwind levels read from LDS / from HBM (lane-levels), cnt[31] the deepest lane's levels summed over the S steps */
        std::fprintf(stderr, "[S branch] unwind iteration: %.2f levels from LDS + %.2f from HBM per S step (%.1f %% from HBM), the step's deepest lane unwinds %.2f\n",
                     (double)cnt[28] / (double)cnt[8], (double)cnt[29] / (double)cnt[8], cnt[28] + cnt[29] ? 100.0 * (double)cnt[29] / (double)(cnt[28] + cnt[29]) : 0.0,
                     (double)cnt[31] / (double)cnt[8]);
#endif
        std::fprintf(stderr, "[S parts, cycles/step] shade %.0f  finish %.0f  newpix %.0f  newsample+setup %.0f\n", (double)cnt[14] / (double)cnt[8],
                     (double)cnt[15] / (double)cnt[8], (double)cnt[16] / (double)cnt[8], (double)cnt[17] / (double)cnt[8]);
    }
}
#endif

/* the statistics of a render, once its stop event has been recorded */
static int collect_stats(mort_ctx *c, const LaunchPlan &plan, int W, int local_rows, int sqrt_spp, bool has_accum, mort_stats *stats) {
    HIPCHK(c, hipEventSynchronize(c->ev1));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    unsigned long long cnt[96] = {0};
    HIPCHK(c, hipMemcpy(cnt, c->d_counters, sizeof cnt, hipMemcpyDeviceToHost));
#ifdef MORT_PROFILE_STATES
    print_profile(c, plan.fam, cnt);
#endif
    const bool wave = plan.fam == FAM_WAVE || plan.fam == FAM_WAVE_GEN;
    std::memset(stats, 0, sizeof *stats);
    stats->seconds = ms * 1e-3;
    for (int k = 0; k < 32; k++) { cnt[0] += cnt[32 + 2 * k]; cnt[1] += cnt[33 + 2 * k]; } /* BVH megakernel: per-workgroup slots */
    stats->segments = cnt[0];
    stats->rng_draws = cnt[1];
    stats->reference_walks = (plan.fam == FAM_BVH || plan.fam == FAM_GEN) ? cnt[3] : 0;
    stats->pixels = (uint64_t)W * (uint64_t)local_rows;
    stats->eff_samples = stats->pixels * (uint64_t)(sqrt_spp * sqrt_spp);
    stats->algorithmic_hbm_bytes = stats->pixels * (uint64_t)(100 + (has_accum ? 12 : 0));
    stats->scene_in_lds = plan.fam != FAM_MEGA ? 1 : 0;
    if (wave) stats->algorithmic_hbm_bytes += 240ull * stats->segments; /* wave_bvh.h: per-segment record traffic */
    stats->local_rows = local_rows;
    std::snprintf(stats->kernel_name, sizeof stats->kernel_name, "%s", plan.name);
    hipFuncAttributes fattr;
    if (hipFuncGetAttributes(&fattr, plan.kernel) == hipSuccess) {
        stats->kernel_vgprs = fattr.numRegs;
        stats->kernel_lds_bytes = plan.lds_bytes >= 0 ? plan.lds_bytes : (int)fattr.sharedSizeBytes;
    }
    return MORT_OK;
}

/* d_segpx: per-pixel segment counts for the packed owned rows, or null.  Only mort_hip_render passes one (sized for
 * THIS image and partition); the public device entry never does, so a buffer left over from an earlier, smaller
 * render can not be written past its end. */
static int render_device_impl(mort_ctx *c, const mort_camera *cam, int mode, void *d_rgba, void *d_accum, uint32_t *d_segpx,
                              void *stream, mort_stats *stats) {
    if (!c || !cam || !d_rgba) return MORT_ERR_INVALID;
    if (mode != MORT_MODE_MEGA && mode != MORT_MODE_WAVE && mode != MORT_MODE_THROUGHPUT) return MORT_ERR_INVALID;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    const int W = cam->image_width, H = cam->image_height;
    if (W <= 0 || H <= 0 || cam->sqrt_spp < 0) return MORT_ERR_INVALID;
    if (cam->bounce_limit < 0 || cam->bounce_limit > MORT_MAX_BOUNCE_LIMIT) return MORT_ERR_CAPACITY;
    if (!c->d_states || c->rng_w != W || c->rng_h != H) return MORT_ERR_NO_RNG;
    int st = check_light(c, cam->light_obj_type, cam->light_obj_idx);
    if (st != MORT_OK) return st;
    LaunchPlan plan = {FAM_MEGA, (const void *)mega_kernel, 256, -1, "mega_kernel"};
    if ((st = choose_family(c, cam, mode, d_segpx != nullptr, plan.fam)) != MORT_OK) return st;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    /* a render still running on another stream uses the same states and counters */
    if (c->last_stream && c->last_stream != s) HIPCHK(c, hipStreamSynchronize(c->last_stream));
    c->last_stream = s;

    RenderArgs a;
    std::memset(&a, 0, sizeof a);
    a.sc = c->sc;
    render_args_camera(a, cam);
    a.rank = c->part.rank; a.nranks = c->part.nranks; a.rows_per_block = c->part.rows_per_block;
    a.local_rows = c->rng_local_rows;
    a.states = c->d_states;
    a.rgba = (uchar4 *)d_rgba; a.accum = (float *)d_accum; a.seg_px = d_segpx;
    a.counters = c->d_counters;
    a.debug_lofs = -1;
    knob_int(std::getenv("MORT_DEBUG_PIXEL"), a.debug_lofs);

    HIPCHK(c, hipMemsetAsync(c->d_counters, 0, 96 * sizeof(unsigned long long), s));
    /* MORT_MODE_THROUGHPUT: the launch covers a virtual image of local_rows * sqrt_spp rows (mega_bvh.h FastArgs.sub) */
    const bool sub = mode == MORT_MODE_THROUGHPUT;
    const int tiles = ((W + 7) / 8) * (((sub ? a.local_rows * cam->sqrt_spp : a.local_rows) + 7) / 8);
    if (sub && (st = mort_ensure_substates(c, W, H, cam->sqrt_spp, s)) != MORT_OK) return st;
    c->tile_launch = mort_ctx::TileLaunch(); /* this launch's, whatever family renders it (mort_hip_debug_tile_state) */
    c->tile_launch.tiles = tiles; c->tile_launch.tiles_x = (W + 7) / 8;
    if (stats) HIPCHK(c, hipEventRecord(c->ev0, s));
    /* a rank that owns no rows launches nothing (and reports mega_kernel) */
    if (tiles > 0) {
        switch (plan.fam) {
        case FAM_MEGA: hipLaunchKernelGGL(mega_kernel, dim3((tiles + 3) / 4), dim3(256), 0, s, a); HIPCHK(c, hipGetLastError()); break; /* four 8x8 tiles per group */
        case FAM_BVH: st = launch_bvh(c, cam, a, tiles, sub, stats != nullptr, s, plan); break;
        case FAM_GEN: st = launch_gen(c, cam, a, tiles, sub, stats != nullptr, s, plan); break;
        case FAM_WAVE: st = launch_wave(c, cam, a, s, plan); break;
        case FAM_WAVE_GEN: st = mort_wave_gen_render(c, cam, a, s, plan); break;
        }
        if (st != MORT_OK) return st;
        if (sub) { /* the stratum rows of each pixel summed in order, then Camera::render's tail */
            hipLaunchKernelGGL(substream_resolve_kernel, dim3((W * a.local_rows + 255) / 256), dim3(256), 0, s, (const float *)c->d_vaccum, W, a.local_rows,
                               cam->sqrt_spp, a.pixel_samples_scale, a.rgba, a.accum);
            HIPCHK(c, hipGetLastError());
        }
    }
    if (!stats) return MORT_OK;
    HIPCHK(c, hipEventRecord(c->ev1, s));
    /* what the statistics need, by value: mort_hip_render_gather lets the frame gather follow the render on the stream
     * and collects them after its one wait (c->defer_stats) */
    const int local_rows = a.local_rows, sqrt_spp = cam->sqrt_spp;
    const bool has_accum = d_accum != nullptr;
    auto fill = [=](mort_stats *out) { return collect_stats(c, plan, W, local_rows, sqrt_spp, has_accum, out); };
    if (c->defer_stats) { c->pending_stats = fill; return MORT_OK; }
    return fill(stats);
}

extern "C" int mort_hip_render_device(mort_ctx *c, const mort_camera *cam, int mode, void *d_rgba, void *d_accum,
                                      void *stream, mort_stats *stats) {
    return render_device_impl(c, cam, mode, d_rgba, d_accum, nullptr, stream, stats);
}

extern "C" int mort_hip_render(mort_ctx *c, const mort_camera *cam, int mode, uint8_t *rgba_out, float *accum_out,
                               uint32_t *segments_px_out, mort_stats *stats) {
    if (!c || !cam || !rgba_out) return MORT_ERR_INVALID;
    const int W = cam->image_width, H = cam->image_height;
    if (W <= 0 || H <= 0) return MORT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const int lr = local_rows_for(c->part, H);
    const size_t npx = (size_t)W * (size_t)lr;
    int st;
    if ((st = ensure_buf(c, &c->d_rgba, &c->rgba_cap, npx * 4)) != MORT_OK) return st;
    if (accum_out && (st = ensure_buf(c, &c->d_accum, &c->accum_cap, npx * 12)) != MORT_OK) return st;
    if (segments_px_out) { if ((st = ensure_buf(c, &c->d_segpx, &c->segpx_cap, npx * 4)) != MORT_OK) return st; }
    else if (c->d_segpx) { hipFree(c->d_segpx); c->d_segpx = nullptr; c->segpx_cap = 0; }
    mort_stats local;
    st = render_device_impl(c, cam, mode, c->d_rgba, accum_out ? c->d_accum : nullptr,
                            segments_px_out ? (uint32_t *)c->d_segpx : nullptr, nullptr, &local);
    if (st != MORT_OK) return st;
    if (stats) *stats = local;
    if (c->part.nranks == 1) { /* packed rows are the whole image: three copies instead of one per row */
        HIPCHK(c, hipMemcpy(rgba_out, c->d_rgba, npx * 4, hipMemcpyDeviceToHost));
        if (accum_out) HIPCHK(c, hipMemcpy(accum_out, c->d_accum, npx * 12, hipMemcpyDeviceToHost));
        if (segments_px_out) HIPCHK(c, hipMemcpy(segments_px_out, c->d_segpx, npx * 4, hipMemcpyDeviceToHost));
        return MORT_OK;
    }
    for (int ly = 0; ly < lr; ly++) {
        const int y = global_row_host(c->part, ly);
        HIPCHK(c, hipMemcpy(rgba_out + (size_t)y * W * 4, (uint8_t *)c->d_rgba + (size_t)ly * W * 4, (size_t)W * 4, hipMemcpyDeviceToHost));
        if (accum_out) HIPCHK(c, hipMemcpy(accum_out + (size_t)y * W * 3, (float *)c->d_accum + (size_t)ly * W * 3, (size_t)W * 12, hipMemcpyDeviceToHost));
        if (segments_px_out) HIPCHK(c, hipMemcpy(segments_px_out + (size_t)y * W, (uint32_t *)c->d_segpx + (size_t)ly * W, (size_t)W * 4, hipMemcpyDeviceToHost));
    }
    return MORT_OK;
}
