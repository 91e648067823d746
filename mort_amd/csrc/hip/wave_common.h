/*
 * wave_common.h -- everything the two forms of MORT_MODE_WAVE share (wave_bvh.h: reference-BVH worlds, wave_gen.hip: every
 * other world).  What is left in the forms is their argument struct, their traversal kernel and the middle of their shade
 * kernel: what the ray hit and what the material does.
 *
 *   HBM records   front ray 32 B + id 4 B (two parities), hit 8 B (by position), pixel 48 B (by id: XORWOW words, colour
 *                 sum, packed counters), bounce stack [depth][id] 16 B.  Counters are double-buffered by front parity and
 *                 zeroed by the kernel that runs between their last reader and next writer, so a front needs no memset.
 *   device        templates over the argument struct WA (WfArgs or WfGenArgs: the queue fields have the same names), the
 *                 RenderArgs passed beside it.  wf_front0: front 0 for one path id.  wf_shade_begin / wf_shade_load /
 *                 wf_shade_push / wf_shade_tail / wf_append: a shade kernel around its middle.  WF_PICK, WF_STAGE, WF_FLUSH and the WPROF macros: the
 *                 traversal kernels' state pick, class staging and profile counters.
 *   host          wf_render: the loop over the fronts.
 */
#ifndef MORT_WAVE_COMMON_H
#define MORT_WAVE_COMMON_H


#ifndef MORT_WF_SHADE_WAVES
#define MORT_WF_SHADE_WAVES 4 /* waves per SIMD the two shade kernels (wf_shade, wf_shade_gen) are compiled for: measured 4 / 5 / 6 / 8, DESIGN.md 4.5 */
#endif
#ifndef MORT_WF_STAGE
#define MORT_WF_STAGE 128 /* positions per class staged in LDS per wave before a flush, in both traversal kernels */
#endif
#include "dev_render.h"
#include "mort_ctx.h"

struct __attribute__((aligned(16))) WfRay { float ox, oy, oz, tm; float dx, dy, dz, time0; };
struct __attribute__((aligned(8))) WfHit { float t; int best; };
struct __attribute__((aligned(16))) WfPix {
    uint32_t d, v0, v1, v2;
    uint32_t v3, v4; float cr, cg;
    float cb; uint32_t packed; /* s_i | s_j << 12 | iter << 24 */ uint32_t segments, draws;
};

enum { WC_LAMB = 0, WC_SPEC = 1, WC_FIN = 2 };

struct WfCounters {
    unsigned front_count[2];  /* records in front[parity] */
    unsigned cls_count[2][3]; /* positions in the class queues of front parity */
    unsigned live;            /* pixels not finished yet */
    unsigned pad[7];
};

DEV Rng wf_rng_load(const WfPix &p) { Rng r; r.d = p.d; r.v0 = p.v0; r.v1 = p.v1; r.v2 = p.v2; r.v3 = p.v3; r.v4 = p.v4; r.draws = p.draws; return r; }
DEV void wf_rng_store(WfPix &p, const Rng &r) { p.d = r.d; p.v0 = r.v0; p.v1 = r.v1; p.v2 = r.v2; p.v3 = r.v3; p.v4 = r.v4; p.draws = r.draws; }
DEV WfRay wf_ray(const Ray &r, float time0) { WfRay o; o.ox = r.o.x; o.oy = r.o.y; o.oz = r.o.z; o.tm = r.tm; o.dx = r.d.x; o.dy = r.d.y; o.dz = r.d.z; o.time0 = time0; return o; }

/* ---- front 0 for one path id: load its stream, the first camera ray of its pixel ---- */
template <typename WA>
__device__ __forceinline__ void wf_front0(const WA &w, const RenderArgs &a) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id == 0) {
        w.cnt->front_count[0] = (unsigned)w.n_paths; w.cnt->front_count[1] = 0;
        for (int p = 0; p < 2; p++) for (int k = 0; k < 3; k++) w.cnt->cls_count[p][k] = 0;
        w.cnt->live = (unsigned)w.n_paths;
    }
    if (id >= w.n_paths) return;
    const int ly = id / a.width, x = id - ly * a.width;
    const int y = global_row(ly, a.rank, a.nranks, a.rows_per_block);
    Rng rng = rng_load(a.states[id]);
    const Ray ray = get_ray(a, x, y, rng, 0, 0);
    w.q_ray[0][id] = wf_ray(ray, ray.tm);
    w.q_id[0][id] = (unsigned)id;
    WfPix p; wf_rng_store(p, rng); p.cr = p.cg = p.cb = 0; p.packed = 0; p.segments = 1; /* the segment this ray is about to trace */
    w.pix[id] = p;
}

/* ---- a shade kernel: one workgroup = 256 positions of ONE class.
 *     WfLane l;
 *     if (!wf_shade_begin(w, l)) return;           counter reset, class and index of this lane
 *     if (l.valid) {
 *         wf_shade_load(w, l);                      id, ray, hit, pixel record, packed counters
 *         ...the kernel's own middle: the hit becomes a bounce entry and the scattered ray (wf_shade_push), or a final value...
 *         wf_shade_tail(w, a, l, terminated, final_value);      unwind, accumulate, next sample or finished pixel; the stored WfPix
 *     }
 *     wf_append(w, l);                              the next front
 * The loads and the tail sit in ONE `if (l.valid)` with the middle, and the push where the middle knows its entry: behind a join
 * of their own, every value of the lane crosses that join (wf_shade_gen was 0.3 % slower on the final scene that way). ---- */
struct WfLane {
    bool valid, cont;   /* holds a record of this front; its path continues into the next one */
    int cls;            /* of the whole workgroup */
    unsigned i, id;     /* index in the class queue; path id */
    WfHit h;
    WfPix P;
    Rng rng;
    int s_i, s_j, iter; /* P.packed */
    Ray ray;            /* in: this segment's; out: the next front's */
    float time0;        /* the sample's camera-ray time */
};

/* false: this workgroup has no positions (the grid is sized from the live count, not from the class counts) */
template <typename WA>
__device__ __forceinline__ bool wf_shade_begin(const WA &w, WfLane &l) {
    const int par = w.parity;
    const unsigned n0 = w.cnt->cls_count[par][0], n1 = w.cnt->cls_count[par][1], n2 = w.cnt->cls_count[par][2];
    const unsigned b0 = (n0 + 255u) >> 8, b1 = (n1 + 255u) >> 8, b2 = (n2 + 255u) >> 8;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        /* the other parity's class counters were last read by the previous shade launch; this front's traversal is done */
        w.cnt->cls_count[par ^ 1][0] = 0; w.cnt->cls_count[par ^ 1][1] = 0; w.cnt->cls_count[par ^ 1][2] = 0;
    }
    unsigned b = blockIdx.x, n;
    if (b < b0) { l.cls = WC_LAMB; n = n0; }
    else if (b < b0 + b1) { l.cls = WC_SPEC; n = n1; b -= b0; }
    else if (b < b0 + b1 + b2) { l.cls = WC_FIN; n = n2; b -= b0 + b1; }
    else return false;
    l.i = b * 256u + threadIdx.x;
    l.valid = l.i < n;
    l.cont = false;
    l.id = 0;
    l.ray.o = mk(0, 0, 0); l.ray.d = mk(0, 0, 1); l.ray.tm = 0;
    l.time0 = 0;
    return true;
}
template <typename WA>
__device__ __forceinline__ void wf_shade_load(const WA &w, WfLane &l) {
    const int par = w.parity;
    const unsigned pos = w.q_cls[l.cls][l.i];
    l.id = w.q_id[par][pos];
    const WfRay rr = w.q_ray[par][pos];
    l.h = w.hits[pos];
    l.P = w.pix[l.id];
    l.rng = wf_rng_load(l.P);
    l.s_i = (int)(l.P.packed & 0xfffu); l.s_j = (int)((l.P.packed >> 12) & 0xfffu); l.iter = (int)(l.P.packed >> 24);
    l.ray.o = mk(rr.ox, rr.oy, rr.oz); l.ray.d = mk(rr.dx, rr.dy, rr.dz); l.ray.tm = rr.tm;
    l.time0 = rr.time0;
}

/* a valid lane whose hit scatters: the bounce entry `e` goes on the stack; at the bounce limit the path ends black
 * (camera.cuh:161-163), else it continues with l.ray, which the middle has set to the scattered ray */
template <typename WA>
__device__ __forceinline__ void wf_shade_push(const WA &w, const RenderArgs &a, WfLane &l, float4 e, bool &terminated, V3 &final_value) {
    w.stack[(size_t)l.iter * (size_t)w.n_paths + l.id] = e;
    l.iter++;
    if (l.iter >= a.bounce_limit) { final_value = mk(0, 0, 0); terminated = true; }
    else { l.P.segments++; l.cont = true; }
}

/* a valid lane after the middle: terminated = final_value is the path's end (a miss, an emitter, the bounce limit) */
template <typename WA>
__device__ __forceinline__ void wf_shade_tail(const WA &w, const RenderArgs &a, WfLane &l, bool terminated, V3 final_value) {
    WfPix &P = l.P;
    const unsigned id = l.id;
    if (terminated) { /* unwind + accumulate (camera.cuh:165-173,190), then the next sample or the finished pixel */
        while (l.iter > 0) {
            l.iter--;
            const float4 se = w.stack[(size_t)l.iter * (size_t)w.n_paths + id];
            const V3 t = vmul(mk(se.x, se.y, se.z), final_value);
            final_value = vadd(mk(0, 0, 0), vscale(se.w, t));
        }
        P.cr += final_value.x; P.cg += final_value.y; P.cb += final_value.z;
        l.s_i++;
        if (l.s_i >= a.sqrt_spp) { l.s_i = 0; l.s_j++; }
        const int ly = (int)id / a.width, x = (int)id - ly * a.width;
        if (l.s_j < a.sqrt_spp) {
            const int y = global_row(ly, a.rank, a.nranks, a.rows_per_block);
            l.ray = get_ray(a, x, y, l.rng, l.s_i, l.s_j);
            l.time0 = l.ray.tm;
            P.segments++;
            l.cont = true;
        } else { /* camera.cuh:194-207 */
            const V3 col = pixel_finish(a.pixel_samples_scale, mk(P.cr, P.cg, P.cb));
            if (a.accum) { a.accum[3 * id] = col.x; a.accum[3 * id + 1] = col.y; a.accum[3 * id + 2] = col.z; }
            pixel_rgba(a.rgba[id], col);
            if (a.seg_px) a.seg_px[id] = P.segments;
            a.states[id] = rng_state(l.rng.d, l.rng.v0, l.rng.v1, l.rng.v2, l.rng.v3, l.rng.v4);
            atomicAdd(&a.counters[0], (unsigned long long)P.segments);
            atomicAdd(&a.counters[1], (unsigned long long)l.rng.draws);
            l.cont = false;
        }
    }
    if (l.cont) {
        wf_rng_store(P, l.rng);
        P.packed = (uint32_t)l.s_i | ((uint32_t)l.s_j << 12) | ((uint32_t)l.iter << 24);
        w.pix[id] = P;
    }
}

/* append the survivors to the next front: one global atomicAdd per workgroup, coalesced record writes.  Every lane of the
 * workgroup calls this. */
template <typename WA>
__device__ __forceinline__ void wf_append(const WA &w, const WfLane &l) {
    __shared__ unsigned s_cnt[4], s_fin[4], s_base;
    const int par = w.parity;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(l.cont);
    const unsigned long long mf = __ballot(l.valid && !l.cont);
    if (lane == 0) { s_cnt[wv] = (unsigned)__popcll(m); s_fin[wv] = (unsigned)__popcll(mf); }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned tot = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        const unsigned fin = s_fin[0] + s_fin[1] + s_fin[2] + s_fin[3];
        s_base = tot ? atomicAdd(&w.cnt->front_count[par ^ 1], tot) : 0u;
        if (fin) atomicSub(&w.cnt->live, fin); /* only finished pixels change the live count */
    }
    __syncthreads();
    unsigned off = s_base;
    for (int k = 0; k < wv; k++) off += s_cnt[k];
    const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
    if (l.cont) {
        const unsigned np = off + (unsigned)rank;
        w.q_ray[par ^ 1][np] = wf_ray(l.ray, l.time0);
        w.q_id[par ^ 1][np] = l.id;
    }
}

/* ---- the traversal kernels: per-lane states, the state a wave runs next, class staging ---- */
enum { W_T = 0, W_L = 1, W_F = 2, W_DONE = 3 };

/* The three pieces below are macros, not functions: inlined functions reach the code generator with other branches (a select
 * for the pick, another join after the flush), and the traversal kernels' instruction streams are kept exactly as they were. */

/* pick = the state a wave runs next; nT / nL / nF lanes wait in T (box step) / L (leaf step) / F (retire + refill): a full
 * enough F or L batch first, else the boxes */
#define WF_PICK(pick, nT, nL, nF, th_f, th_l) do { \
        if ((nF) >= (th_f)) pick = W_F; \
        else if ((nL) >= (th_l)) pick = W_L; \
        else if ((nT) > 0) pick = W_T; \
        else pick = ((nL) >= (nF)) ? W_L : W_F; \
    } while (0)

/* the wave's staged[k] positions of class k (at stage[k * MORT_WF_STAGE]) into the class queue q: one global atomicAdd on
 * cnt->cls_count[par][k].  Reads `lane` */
#define WF_FLUSH(cnt, par, k, q, stage, staged) do { \
        if (staged[k] > 0) { \
            unsigned base_ = 0; \
            if (lane == 0) base_ = atomicAdd(&(cnt)->cls_count[par][k], (unsigned)staged[k]); \
            base_ = __shfl(base_, 0); \
            for (int i_ = lane; i_ < staged[k]; i_ += 64) (q)[base_ + (unsigned)i_] = stage[(k) * MORT_WF_STAGE + i_]; \
            staged[k] = 0; \
        } } while (0)

/* the lanes with cls == k stage f_pos, after a flush if they would not fit */
#define WF_STAGE(cnt, par, k, q, stage, staged, cls, f_pos) do { \
        const unsigned long long m_ = __ballot((cls) == (k)); \
        const int n_ = __popcll(m_); \
        if (n_ > 0) { \
            if (staged[k] + n_ > MORT_WF_STAGE) WF_FLUSH(cnt, par, k, q, stage, staged); \
            const int rk_ = __builtin_amdgcn_mbcnt_hi((unsigned)(m_ >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m_, 0)); \
            if ((cls) == (k)) stage[(k) * MORT_WF_STAGE + staged[k] + rk_] = (f_pos); \
            staged[k] += n_; \
        } } while (0)

/* -DMORT_PROFILE_STATES: per-state wave-steps, lanes and cycles of a traversal kernel (scripts/wave_profile.py; printed by
 * mort_hip_render).  WPROF_T0 where the wave's lifetime starts, WPROF_BEGIN before the loop, WPROF_END(counters) after it. */
#ifdef MORT_PROFILE_STATES
#define WPROF_T0 const unsigned long long rt0 = __builtin_amdgcn_s_memrealtime()
#define WPROF_BEGIN unsigned long long pr_steps[3] = {0, 0, 0}, pr_lanes[3] = {0, 0, 0}, pr_cyc[4] = {0, 0, 0, 0}; \
    unsigned long long pt0 = __builtin_readcyclecounter(), pt1
#define WPROF(i, lanes) do { pr_steps[i] += 1; pr_lanes[i] += (unsigned long long)(lanes); } while (0)
#define WPROFC(i) do { pt1 = __builtin_readcyclecounter(); pr_cyc[i] += pt1 - pt0; pt0 = pt1; } while (0)
#define WPROF_END(counters) do { if (lane == 0) { \
        for (int k = 0; k < 3; k++) { atomicAdd(&(counters)[4 + k], pr_steps[k]); atomicAdd(&(counters)[8 + k], pr_lanes[k]); } \
        for (int k = 0; k < 4; k++) atomicAdd(&(counters)[12 + k], pr_cyc[k]); \
        atomicAdd(&(counters)[20], __builtin_amdgcn_s_memrealtime() - rt0); /* sum of wave lifetimes, 10 ns ticks */ \
        atomicAdd(&(counters)[21], 1ull);                                   /* waves */ \
    } } while (0)
#else
#define WPROF_T0 do { } while (0)
#define WPROF_BEGIN do { } while (0)
#define WPROF(i, lanes) do { } while (0)
#define WPROFC(i) do { } while (0)
#define WPROF_END(counters) do { } while (0)
#endif

/* ---- host: the front loop of both forms.  Carves the records of the N owned pixels out of c->d_wf into the queue fields of
 * `w` (WfArgs or WfGenArgs), launches `init`, then one trav + shade launch pair per front until no pixel is live.  trav runs
 * TB-thread groups with trav_lds bytes of dynamic LDS, a group taking per_group records of a front at least. ---- */
template <typename WA>
static int wf_render(mort_ctx *c, const mort_camera *cam, size_t N, WA &w, void (*init)(const WA), void (*trav)(const WA),
                     void (*shade)(const WA), int TB, size_t trav_lds, size_t per_group, hipStream_t s) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += al(bytes); return o; };
    const size_t o_ray0 = take(N * sizeof(WfRay)), o_ray1 = take(N * sizeof(WfRay));
    const size_t o_id0 = take(N * sizeof(unsigned)), o_id1 = take(N * sizeof(unsigned));
    const size_t o_hits = take(N * sizeof(WfHit)), o_pix = take(N * sizeof(WfPix));
    const size_t o_stack = take(N * (size_t)cam->bounce_limit * sizeof(float4));
    const size_t o_c0 = take(N * sizeof(unsigned)), o_c1 = take(N * sizeof(unsigned)), o_c2 = take(N * sizeof(unsigned));
    const size_t o_cnt = take(sizeof(WfCounters));
    const int st = ensure_buf(c, &c->d_wf, &c->wf_bytes, off);
    if (st != MORT_OK) return st;
    if (!c->h_live) HIPCHK(c, hipHostMalloc((void **)&c->h_live, 64));
    unsigned char *base = (unsigned char *)c->d_wf;
    w.n_paths = (int)N;
    w.q_ray[0] = (WfRay *)(base + o_ray0); w.q_ray[1] = (WfRay *)(base + o_ray1);
    w.q_id[0] = (unsigned *)(base + o_id0); w.q_id[1] = (unsigned *)(base + o_id1);
    w.hits = (WfHit *)(base + o_hits); w.pix = (WfPix *)(base + o_pix);
    w.stack = (float4 *)(base + o_stack);
    w.q_cls[0] = (unsigned *)(base + o_c0); w.q_cls[1] = (unsigned *)(base + o_c1); w.q_cls[2] = (unsigned *)(base + o_c2);
    w.cnt = (WfCounters *)(base + o_cnt);

    HIPCHK(c, hipFuncSetAttribute((const void *)trav, hipFuncAttributeMaxDynamicSharedMemorySize, (int)trav_lds));
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, trav, TB, trav_lds) != hipSuccess || per_cu < 1) per_cu = 1;
    const int max_trav_grid = c->num_cus * per_cu;
    hipLaunchKernelGGL(init, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, w);
    HIPCHK(c, hipGetLastError());
    const long long max_fronts = (long long)cam->sqrt_spp * cam->sqrt_spp * ((long long)cam->bounce_limit + 1) + 8;
    size_t live = N;
    long long front = 0;
    const int chunk = 32; /* fronts per host round trip (the live count is read back in between) */
    while (live > 0 && front < max_fronts) {
        int tg = (int)((live + per_group - 1) / per_group);
        if (tg > max_trav_grid) tg = max_trav_grid;
        if (tg < 1) tg = 1;
        const int sg = (int)((live + 255) / 256) + 3;
        for (int k = 0; k < chunk; k++, front++) {
            w.parity = (int)(front & 1);
            hipLaunchKernelGGL(trav, dim3(tg), dim3(TB), trav_lds, s, w);
            hipLaunchKernelGGL(shade, dim3(sg), dim3(256), 0, s, w);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(c->h_live, &w.cnt->live, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        live = *c->h_live;
    }
    c->wf_fronts = (int)front;
    if (live != 0) { c->last_error = "wavefront: front limit reached with live pixels"; return MORT_ERR_HIP; }
    return MORT_OK;
}


#endif
