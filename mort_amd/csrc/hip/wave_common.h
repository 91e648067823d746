/*
 * wave_common.h -- HBM records of MORT_MODE_WAVE, shared by its two forms (wave_bvh.h: reference-BVH worlds,
 * wave_gen.hip: every other world).  Front ray 32 B + id 4 B (two parities), hit 8 B (by position), pixel 48 B (by id:
 * XORWOW words, colour sum, packed counters), bounce stack [depth][id] 16 B; and the host loop over the fronts.
 */
#ifndef MORT_WAVE_COMMON_H
#define MORT_WAVE_COMMON_H


#ifndef MORT_WF_SHADE_WAVES
#define MORT_WF_SHADE_WAVES 4 /* waves per SIMD the two shade kernels (wf_shade, wf_shade_gen) are compiled for: measured 4 / 5 / 6 / 8, DESIGN.md 4.5 */
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
