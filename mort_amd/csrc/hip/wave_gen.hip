/*
 * wave_gen.hip -- MORT_MODE_WAVE for worlds without reference BVHs (reference scenes 2..9; BASELINE config 5 is the
 * book-2 final scene through this form): the render path as a queue of path segments instead of one lane per pixel.
 *
 * One path per pixel, all pixels of the rank in flight.  A pixel's samples stay chained through its own XORWOW state
 * (the reference's streams are pixel-serial, rng.cuh:17-23), so a FRONT is one segment of every live pixel: a compact
 * array of (path id, ray) records in HBM.  Per front, two launches:
 *
 *   wf_trav_gen   closest solid hit of every record: the unified tree (scene_compile.h build_unified) in LDS, walked by
 *                 the same per-lane state machine as mega_gen_kernel (T both child boxes of a node / L the primitives of
 *                 a leaf / F retire + refill).  Each wave owns 64-record batches of the front, strided over the front; a
 *                 lane whose ray is done takes the next record by rank among the waiting lanes (ballot + mbcnt), so the
 *                 box-test loop stays full.  Retiring writes an 8-byte hit record at the ray's position and appends the
 *                 position to the queue of its shade class, staged per wave in LDS (one global atomic per ~128 entries).
 *   wf_shade_gen  one workgroup = 256 positions of ONE class (diffuse / specular+emissive / miss): the constant media
 *                 after the solids (they draw from the pixel's stream, which lives here: constant_medium::hit,
 *                 objects.cuh:396-434), then dev_shade.h's shade_hit -- every material, texture and the light mixture --
 *                 then either the next segment's record (appended to the next front: one atomic per workgroup,
 *                 coalesced 32-byte writes) or the unwind, the next sample's camera ray, or the finished pixel.
 *
 * What the two forms of the mode share is wave_common.h's: the records, front 0 (wf_init_gen is one call), the shade kernel's
 * head, push, tail and append around the middle written here, and the traversal kernel's pick / stage / flush.
 *
 * Same streams, same operations, same order per pixel as the megakernels: bit-identical output (tests/test_gpu_gen.py).
 * Algorithmic HBM traffic per segment: trav 32 r + 8 w + 4 q; shade 4 q + 4 + 32 + 8 + 48 r, 4 + 32 + 48 + 16 w = 240 B.
 */
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mort_internal.h"
#include "wave_gen.h"
#include "wave_common.h"
#include "dev_gen.h"
#include "dev_shade_call.h"

#pragma clang fp contract(off)

struct WfGenArgs {
    GenArgs g;                /* g.f.r: camera / partition / buffers; g.f.hot_src / hot_bytes / off_tstack: LDS image */
    uint32_t t_stage;         /* LDS offset of the per-wave class staging */
    int n_paths;
    unsigned *q_id[2];        /* front[parity]: path id of each record */
    WfRay *q_ray[2];          /* front[parity]: its ray */
    WfHit *hits;              /* by position in the current front */
    WfPix *pix;               /* by path id */
    float4 *stack;            /* [bounce_limit][n_paths] */
    unsigned *q_cls[3];       /* positions, per shade class */
    WfCounters *cnt;
    int parity;               /* front & 1 */
};

/* ---- front 0: load streams, first camera ray of every pixel ---- */
__global__ void __launch_bounds__(256) wf_init_gen(const WfGenArgs w) { wf_front0(w, w.g.f.r); }

/* the scan for rays the walk does not decide: out of line, HBM copy of the scene */
struct WScanHit { uint32_t best; float closest; };
__device__ __attribute__((noinline)) WScanHit wf_scan_solids(const DScene *scp, int first_medium, const int *chains, int n_chains,
                                                             float ox, float oy, float oz, float dx, float dy, float dz, float tm) {
    Ray r; r.o = mk(ox, oy, oz); r.d = mk(dx, dy, dz); r.tm = tm;
    WScanHit h;
    gen_scan_solids(*scp, first_medium, chains, n_chains, r, h.closest, h.best);
    return h;
}

template <int BLOCK, bool PRIMS_LDS>
__global__ void __launch_bounds__(BLOCK) wf_trav_gen(const WfGenArgs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    /* launch arguments without private memory (mega_gen.hip): the by-value parameter is never named; the kernarg segment is copied into
     * LDS, the loop's wave-uniform values are pinned in SGPRs, the out-of-line scan gets the segment's own address */
    __shared__ WfGenArgs s_w;
    const WfGenArgs *const wp = (const WfGenArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    {
        const uint32_t *src = (const uint32_t *)wp;
        uint32_t *dst = (uint32_t *)&s_w;
        for (uint32_t i = threadIdx.x; i < (uint32_t)(sizeof(WfGenArgs) / 4); i += BLOCK) dst[i] = src[i];
    }
    {
        const uint4 *src = (const uint4 *)wp->g.f.hot_src;
        uint4 *dst = (uint4 *)lds;
        const uint32_t n16 = wp->g.f.hot_bytes >> 4;
        for (uint32_t i = threadIdx.x; i < n16; i += BLOCK) dst[i] = src[i];
    }
    const int par = wp->parity;
    WfCounters *const wcnt = wp->cnt;
    if (blockIdx.x == 0 && threadIdx.x == 0) wcnt->front_count[par ^ 1] = 0; /* next front: its last reader was the previous wf_trav_gen */
    __syncthreads();
    const WfGenArgs &W = s_w;
    const GenArgs &L = W.g;
    const DNodeQ *nodes2 = (const DNodeQ *)(lds + uni_u(L.o_nodes));
    const uint32_t *entries = (const uint32_t *)(lds + uni_u(L.o_entries));
    const int *chains = (const int *)(lds + uni_u(L.o_chains));
    unsigned short *tstack = (unsigned short *)(lds + uni_u(L.f.off_tstack)) + threadIdx.x; /* [level * BLOCK] */
    unsigned *stage = (unsigned *)(lds + uni_u(W.t_stage)) + (threadIdx.x >> 6) * (3 * MORT_WF_STAGE);
    DScene lsc; /* only what the leaf test reads: transform chains and primitives */
    lsc.xforms = (const DXform *)(lds + uni_u(L.o_xforms));
    if (PRIMS_LDS) { lsc.spheres = (const DSphere *)(lds + uni_u(L.o_spheres)); lsc.quads = (const DQuad *)(lds + uni_u(L.o_quads)); }
    else { lsc.spheres = uni_p(L.f.r.sc.spheres); lsc.quads = uni_p(L.f.r.sc.quads); }
    const DSphere *spheres = lsc.spheres;
    const DQuad *quads = lsc.quads;
    const uint32_t *ranks = uni_p(L.ranks);
    const int n_spheres = uni_i(L.n_spheres);
    const uint32_t root = uni_u(L.root);
    const float g_x = uni_f(L.gx), g_y = uni_f(L.gy), g_z = uni_f(L.gz), g_R = uni_f(L.gR), g_mnear = uni_f(L.mnear), g_kmin = uni_f(L.kmin);
    WfHit *const hits = uni_p(W.hits);
    unsigned *const q_cls0 = uni_p(W.q_cls[0]), *const q_cls1 = uni_p(W.q_cls[1]), *const q_cls2 = uni_p(W.q_cls[2]);
    int staged[3] = {0, 0, 0};
    const int lane = threadIdx.x & 63;
    const unsigned n_items = wcnt->front_count[par];
    const WfRay *front = par ? uni_p(W.q_ray[1]) : uni_p(W.q_ray[0]);

    /* this wave's share of the front: 64-record batches wave_id, wave_id + n_waves, ... (strided, so every wave samples
     * the whole image: fronts are in pixel order and cost varies by region) */
    const unsigned n_waves = gridDim.x * (BLOCK / 64), wave_id = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    unsigned next_batch = wave_id, b_base = 0;
    int b_cnt = 0, b_off = 0;

    const int th_f = uni_i(L.f.th_s), th_l = uni_i(L.f.th_l), t_keep = uni_i(L.f.t_keep); /* scheduling thresholds (lanes), as in mega_gen.hip; F plays S's part */
    int state = W_F;
    bool have = false;
    unsigned pos = 0;
    Ray ray; ray.o = mk(0, 0, 0); ray.d = mk(0, 0, 1); ray.tm = 0;
    GenRay gr; gr.ix = gr.iy = gr.iz = 1; gr.mx = gr.my = gr.mz = 0; gr.band = 0;
    float ray_a = 1, closest = 0;
    uint32_t best = GBEST_NONE, node = 0;
    int sp = 0, flags = 0;

    WPROF_BEGIN;
    WPROF_T0;
    for (;;) {
        const int nT = __popcll(__ballot(state == W_T));
        const int nL = __popcll(__ballot(state == W_L));
        const int nF = __popcll(__ballot(state == W_F));
        if (nT + nL + nF == 0) break;
        int pick;
        WF_PICK(pick, nT, nL, nF, th_f, th_l);
        WPROFC(3);

        if (pick == W_T) {
            int keep;
            do {
                WPROF(0, __popcll(__ballot(state == W_T)));
                if (state == W_T) { /* both child boxes of one node (dev_gen.h gen_prune) */
                    const uint4 *np = (const uint4 *)(nodes2 + node); /* two ds_read_b128: corner + steps, 12 plane offsets + children */
                    const uint4 na = np[0], nb = np[1];
                    const GenBoxes nd = gen_node_decode(__uint_as_float(na.x), __uint_as_float(na.y), __uint_as_float(na.z), na.w, nb.x, nb.y, nb.z, nb.w);
                    float te0, te1;
                    const bool m0 = gen_prune(nd.x0min, nd.x0max, nd.y0min, nd.y0max, nd.z0min, nd.z0max, gr, closest, te0);
                    const bool m1 = gen_prune(nd.x1min, nd.x1max, nd.y1min, nd.y1max, nd.z1min, nd.z1max, gr, closest, te1);
                    const uint32_t c0 = nd.c0, c1 = nd.c1;
                    const bool both = !m0 && !m1, none = m0 && m1;
                    const bool first0 = te0 <= te1;
                    uint32_t next = both ? (first0 ? c0 : c1) : (m0 ? c1 : c0);
                    if (both) tstack[sp * BLOCK] = (unsigned short)(first0 ? c1 : c0);
                    sp += both ? 1 : 0;
                    const bool more = !none || sp > 0;
                    if (none && sp > 0) { sp--; next = tstack[sp * BLOCK]; }
                    if (!more) state = W_F;
                    else { node = next & 0x7fffu; if (next & 0x8000u) state = W_L; }
                }
                keep = __popcll(__ballot(state == W_T));
            } while (keep >= t_keep);
            WPROFC(0);
        }
        if (pick == W_L) { /* sequential ifs, not a chain: no register copies at a common join (mega_bvh.h) */
            WPROF(1, nL);
            uint32_t lpos = 0;
            int cnt = 0;
            if (state == W_L) { lpos = GLEAF_FIRST(node); cnt = (int)GLEAF_COUNT(node); } /* a leaf reference is a run of entries */
            uint32_t e0 = 0, e1 = 0; /* two primitives per trip through two register sets, the next record requested before this one is tested (mega_gen.hip) */
            PrimRec r0, r1;
            { const v4f_t z = {0.f, 0.f, 0.f, 0.f}; r0.a = r0.b = r0.c = r0.d = r0.e = z; r1 = r0; }
            if (cnt > 0) { e0 = entries[lpos]; r0 = load_prim<PRIMS_LDS>(spheres, quads, e0); }
            while (__ballot(cnt > 0) != 0ull) {
                if (cnt > 0) {
                    if (cnt > 1) { e1 = entries[lpos + 1]; r1 = load_prim<PRIMS_LDS>(spheres, quads, e1); }
                    /* both own roots against the same closest_so_far (independent chains), then applied in entry order: dev_gen.h gen_prim_t */
                    const uint32_t ea = e0, eb = e1;
                    const float ta = gen_prim_t(lsc, chains, rec_sphere(r0), rec_quad(r0), ea, ray, ray_a, closest);
                    float tb = -1.0f;
                    if (cnt > 1) tb = gen_prim_t(lsc, chains, rec_sphere(r1), rec_quad(r1), eb, ray, ray_a, closest);
                    if (cnt > 2) { e0 = entries[lpos + 2]; r0 = load_prim<PRIMS_LDS>(spheres, quads, e0); }
                    gen_apply_t(ranks, n_spheres, ta, ea, closest, best, flags);
                    gen_apply_t(ranks, n_spheres, tb, eb, closest, best, flags);
                    lpos += 2; cnt -= 2;
                }
            }
            if (state == W_L) {
                if (sp > 0) {
                    sp--;
                    const uint32_t next = tstack[sp * BLOCK];
                    node = next & 0x7fffu;
                    state = (next & 0x8000u) ? W_L : W_T;
                } else state = W_F;
            }
            WPROFC(1);
        }
        if (pick == W_F) {
            WPROF(2, nF);
            /* wave-uniform control flow: every lane runs this block */
            const bool inF = (state == W_F);
            const bool fin = inF && have;
            if (fin && flags) { /* non-ordinary reciprocal / NaN root: the scan decides */
                const WScanHit h = wf_scan_solids(&wp->g.f.r.sc, wp->g.first_medium, (const int *)(wp->g.f.hot_src + wp->g.o_chains), wp->g.n_chains,
                                                  ray.o.x, ray.o.y, ray.o.z, ray.d.x, ray.d.y, ray.d.z, ray.tm);
                best = h.best; closest = h.closest;
            }
            /* ---- retire: hit record at the ray's position, position into its class queue ---- */
            int cls = -1;
            if (fin) {
                WfHit h; h.t = closest; h.best = (int)best;
                hits[pos] = h;
                if (best == GBEST_NONE) cls = WC_FIN;
                else {
                    const uint32_t mat = GENT_QUAD(best) ? quads[GENT_IDX(best)].mat : spheres[GENT_IDX(best)].mat;
                    const int mt = DREF_TYPE(mat);
                    cls = (mt == MORT_MAT_LAMBERTIAN || mt == MORT_MAT_ISOTROPIC) ? WC_LAMB : WC_SPEC;
                }
            }
            const unsigned f_pos = pos;
            if (inF) have = false;
#pragma unroll
            for (int k = 0; k < 3; k++) WF_STAGE(wcnt, par, k, k == 0 ? q_cls0 : k == 1 ? q_cls1 : q_cls2, stage, staged, cls, f_pos);
            /* ---- hand the waiting lanes the next records of this wave's batches ---- */
            const unsigned long long need = __ballot(inF);
            const int want = __popcll(need);
            const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(need >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)need, 0));
            int served = 0;
            while (served < want) {
                if (b_off == b_cnt) { /* batch used up: the next one of this wave */
                    b_base = next_batch * 64u;
                    b_cnt = (b_base < n_items) ? (int)((n_items - b_base < 64u) ? (n_items - b_base) : 64u) : 0;
                    b_off = 0;
                    next_batch += n_waves;
                    if (b_cnt == 0) break;
                }
                int take = b_cnt - b_off;
                if (take > want - served) take = want - served;
                if (inF && rank >= served && rank < served + take) {
                    pos = b_base + (unsigned)(b_off + (rank - served));
                    const WfRay rr = front[pos];
                    ray.o = mk(rr.ox, rr.oy, rr.oz); ray.d = mk(rr.dx, rr.dy, rr.dz); ray.tm = rr.tm;
                    ray_a = vlen2(ray.d);
                    const bool ordinary = gen_ray_setup(ray, g_x, g_y, g_z, g_R, g_mnear, g_kmin, gr);
                    closest = __builtin_inff(); best = GBEST_NONE; sp = 0;
                    flags = ordinary ? 0 : GFL_REF;
                    have = true;
                    if (!ordinary || root == 0xffffu) state = W_F; /* retired at the next F step (the scan decides) */
                    else { node = root & 0x7fffu; state = (root & 0x8000u) ? W_L : W_T; }
                }
                b_off += take; served += take;
            }
            if (inF && !have) state = W_DONE; /* this wave's batches are exhausted */
            WPROFC(2);
        }
    }
    WF_FLUSH(wcnt, par, 0, q_cls0, stage, staged); WF_FLUSH(wcnt, par, 1, q_cls1, stage, staged); WF_FLUSH(wcnt, par, 2, q_cls2, stage, staged);
    WPROF_END(wp->g.f.r.counters);
}

/* ---- shading of one front ---- */
__global__ void __launch_bounds__(256, MORT_WF_SHADE_WAVES) wf_shade_gen(const WfGenArgs w) {
    const GenArgs &ga = w.g;
    const RenderArgs &a = ga.f.r;
    const DScene &sc = a.sc;
    const int *chains = (const int *)(ga.f.hot_src + ga.o_chains);
    WfLane l;
    if (!wf_shade_begin(w, l)) return;
    if (l.valid) {
        wf_shade_load(w, l);
        Ray &ray = l.ray;
        Rng &rng = l.rng;
        const float time0 = l.time0;
        /* the constant media come after every solid, with the solids' closest_so_far (world.cuh:154-160) */
        float closest = l.h.t;
        uint32_t best = (uint32_t)l.h.best;
        gen_media(sc, ga.first_medium, sc.n_items, ray, rng, closest, best);
        V3 final_value = a.background; /* a miss (camera.cuh:154-158) */
        bool terminated = (best == GBEST_NONE);
        if (!terminated) { /* what the ray hit and what the material does: a bounce entry and the scattered ray, or a final value */
            const Best bb = gen_decode_best(sc, chains, best, closest);
            /* inlined: this kernel waits on memory (71 % of its wave cycles), and the out-of-line call's frame -- callee-saved registers and
             * the 22-dword result through scratch -- was half of its memory instructions: 2048x2048x4 spp 223 -> 112 ms.  (The call was a
             * workaround for the SLP vectorizer's miscompile, dev_shade_call.h; the library is built without that pass now.  -DMORT_SHADE_CALL
             * brings the call back; mega_gen.hip keeps it, where it costs nothing.) */
#ifdef MORT_SHADE_CALL
            const ShadeOut so = shade_hit_outlined(&a.sc, a.light_type, a.light_idx, ray, time0, bb, rng);
#else
            const ShadeOut so = shade_hit(a.sc, a.light_type, a.light_idx, ray, time0, bb, rng);
#endif
            if (so.done) { final_value = so.final_value; terminated = true; }
            else {
                float4 e; e.x = so.e.kx; e.y = so.e.ky; e.z = so.e.kz; e.w = so.e.rp; /* dielectric: (1, 1, 1, 1) */
                if (so.ident) e.x = e.y = e.z = e.w = 1.0f;
                wf_shade_push(w, a, l, e, terminated, final_value);
            }
        }
        wf_shade_tail(w, a, l, terminated, final_value);
    }
    wf_append(w, l);
}

/* ---- host side ---- */
typedef void (*trav_kernel_t)(const WfGenArgs);
static trav_kernel_t pick_trav(int block, bool prims_in_lds) {
    if (block == 1024) return prims_in_lds ? wf_trav_gen<1024, true> : wf_trav_gen<1024, false>;
    if (block == 512) return prims_in_lds ? wf_trav_gen<512, true> : wf_trav_gen<512, false>;
    return prims_in_lds ? wf_trav_gen<256, true> : wf_trav_gen<256, false>;
}
static int trav_block_for(const GenArgs &ga) { /* the LDS image + per-wave staging must fit one CU's LDS */
    const size_t fixed = (size_t)ga.f.hot_bytes + 32;
    const size_t need512 = fixed + (size_t)MORT_OWN_STACK * 512 * 2 + (size_t)(512 / 64) * 3 * MORT_WF_STAGE * 4;
    const size_t need1024 = fixed + (size_t)MORT_OWN_STACK * 1024 * 2 + (size_t)(1024 / 64) * 3 * MORT_WF_STAGE * 4;
    int tb = need512 <= 150 * 1024 ? 512 : 256;
    /* a big image (the final scene's 98 KB) admits one workgroup per CU: the kernel needs under 128 VGPRs, so that workgroup can bring four waves per SIMD */
    if (need512 > 75 * 1024 && need1024 <= 158 * 1024) tb = 1024;
    { int v = 0; if (knob_int(std::getenv("MORT_WAVE_TRAV_BLOCK"), v) && (v == 256 || v == 512 || (v == 1024 && need1024 <= 158 * 1024))) tb = v; }
    return tb;
}
int mort_wave_gen_render(mort_ctx *c, const mort_camera *cam, const RenderArgs &a, hipStream_t s, LaunchPlan &plan) {
    WfGenArgs w;
    std::memset(&w, 0, sizeof w);
    GenArgs &ga = w.g;
    ga = c->gen; /* LDS image offsets, root, far-ray constants (upload_world) */
    ga.f.r = a;
    ga.f.hot_src = (const unsigned char *)c->d_gen; ga.f.hot_bytes = c->gen_bytes;
    ga.f.th_s = 32; ga.f.th_l = 24; ga.f.t_keep = 16; /* wf_trav_gen's retire+refill / leaf / box-run thresholds */
    { int th[3]; if (knob_ints(std::getenv("MORT_WAVE_THRESHOLDS"), 3, 1, th)) { ga.f.th_s = th[0]; ga.f.th_l = th[1]; ga.f.t_keep = th[2]; } } /* "f,l,k" */
    const int TB = trav_block_for(ga);
    trav_kernel_t trav = pick_trav(TB, ga.prims_in_lds != 0);
    /* LDS of wf_trav_gen: image | traversal stacks | class staging */
    ga.f.off_tstack = (ga.f.hot_bytes + 15u) & ~15u;
    w.t_stage = ga.f.off_tstack + (uint32_t)MORT_OWN_STACK * (uint32_t)TB * 2u;
    const size_t trav_lds = (size_t)w.t_stage + (size_t)(TB / 64) * 3 * MORT_WF_STAGE * sizeof(unsigned);
    { /* dynamic + the kernel's own __shared__ objects must fit the CU's 160 KB: refuse here rather than fail at the first launch */
        hipFuncAttributes fattr;
        HIPCHK(c, hipFuncGetAttributes(&fattr, (const void *)trav));
        if (trav_lds + fattr.sharedSizeBytes > (size_t)160 * 1024) return hip_fail(c, hipErrorInvalidValue, "wf_trav_gen LDS");
    }
    plan.kernel = (const void *)trav; plan.block = TB; plan.lds_bytes = -1;
    std::snprintf(plan.name, sizeof plan.name, "wf_trav_gen<%d, %s>", TB, ga.prims_in_lds ? "true" : "false"); /* <BLOCK, PRIMS_LDS> */
    /* a wave's share of a front: one 64-record batch at least (two were 4 % slower on small fronts: the front's time is its slowest wave's) */
    return wf_render(c, cam, (size_t)a.width * (size_t)a.local_rows, w, wf_init_gen, trav, wf_shade_gen, TB, trav_lds, (size_t)(TB / 64) * 64, s);
}
