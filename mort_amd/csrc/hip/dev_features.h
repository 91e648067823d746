/*
 * dev_features.h -- the first-hit feature pass and the edge-aware a-trous denoiser (Dammertz et al., HPG 2010): one body per
 * pixel, compiled for the gfx950 kernels of denoise.hip AND run by the host loops there (mort_hip_render_features_host,
 * mort_hip_denoise_host), -ffp-contract=off on both sides, so host and device agree bit for bit.
 *
 * Not part of the parity path: nothing here draws a random number, reads or writes a pixel's XORWOW state, or is inlined
 * into a render kernel.  The traversal pieces are the render's own (dev_trace.h, dev_gen.h), used unchanged; what differs
 * (solids only, a deterministic medium entry, an explicit traversal stack) lives in the new functions below.
 */
#ifndef MORT_DEV_FEATURES_H
#define MORT_DEV_FEATURES_H

#include "mort_hip.h"
#include "dev_gen.h"

#pragma clang fp contract(off)

/* ---------------------------------------------------------------------------------------------------------------------
 * Feature pass: one primary ray per pixel through the pixel centre from the lens centre, tm = 0.5
 * ------------------------------------------------------------------------------------------------------------------ */
struct FeatArgs {
    DScene sc;
    GenWalk gw;            /* valid when the launch walks the unified tree */
    int width, height;
    V3 background, center, pixel00, du, dv;
    int rank, nranks, rows_per_block, local_rows;
    float *albedo, *normal, *depth; /* packed owned rows: 3, 3, 1 floats per pixel */
};

/* the single-lane tree walk over the solids (dev_gen.h) with the pending far children at stack[k * stride] (an LDS column on
 * the device, a local array on the host), and the scan for the rays the walk does not decide.  No media. */
DEV void feat_tree_solids(const DScene &sc, const GenWalk &gw, const Ray &ray, unsigned short *stack, int stride, float &closest, uint32_t &best) {
    int flags;
    gen_walk_solids(sc, gw, ray, stack, stride, closest, best, flags);
    if (flags) gen_scan_solids(sc, gw.first_medium, gw.chains, gw.n_chains, ray, closest, best);
}

/* world::hit's scan over every solid item (reference BVHs included), t_min = 0.001 */
DEV void feat_scan_solids(const DScene &sc, const Ray &r, float &closest, Best &best) {
    closest = __builtin_inff();
    best.kind = HIT_NONE; best.t = 0; best.prim = 0; best.chain_first = 0; best.chain_count = 0;
    for (int i = 0; i < sc.n_items; i++) {
        const DItem it = sc.items[i];
        const int kind = it.kind;
        if (kind == ITEM_BVH) run_bvh(sc, r, it.first, it.count, 0.001f, closest, best);
        if (kind == ITEM_SPHERES) run_spheres(sc, r, it.first, it.count, it.chain_first, it.chain_count, 0.001f, closest, best);
        if (kind == ITEM_QUADS) run_quads(sc, r, it.first, it.count, it.chain_first, it.chain_count, 0.001f, closest, best);
    }
}

/* the constant media in scan order after the solids: world::hit's two boundary_t calls and its clamp of the exit to closest,
 * no random distance -- a medium the ray enters before the closest solid is hit at its entry t1.  A ray that starts inside a
 * medium (entry below t_min) does not enter it: that medium is no first hit, and the pixel shows what lies behind it */
DEV void feat_media(const DScene &sc, const Ray &ray, float &closest, Best &best) {
    for (int i = 0; i < sc.n_items; i++) {
        const DItem it = sc.items[i];
        if (it.kind != ITEM_MEDIUM) continue;
        float t1, t2;
        if (!boundary_t(sc, ray, it.first, it.count, -__builtin_inff(), __builtin_inff(), t1)) continue;
        if (!boundary_t(sc, ray, it.first, it.count, (float)((double)t1 + 0.0001), __builtin_inff(), t2)) continue;
        if (t1 < 0.001f) continue;
        if (t2 > closest) t2 = closest;
        if (t1 >= t2) continue;
        closest = t1;
        best.t = t1; best.kind = HIT_MEDIUM; best.prim = i; best.chain_first = it.chain_first; best.chain_count = it.chain_count;
    }
}

/* one pixel: TREE = the unified-tree walk (stack as in feat_tree_solids), else the item scan */
template <bool TREE>
DEV void feat_pixel(const FeatArgs &a, int x, int ly, unsigned short *stack, int stride) {
    const DScene &sc = a.sc;
    const int y = global_row(ly, a.rank, a.nranks, a.rows_per_block);
    const size_t lofs = (size_t)x + (size_t)ly * (size_t)a.width;
    /* get_ray (dev_render.h) with both sub-pixel offsets 0 and no defocus sample */
    const V3 pixel_sample = vadd(vadd(a.pixel00, vscale((float)((double)x + 0.0), a.du)), vscale((float)((double)y + 0.0), a.dv));
    Ray ray;
    ray.o = a.center;
    ray.d = vsub(pixel_sample, a.center);
    ray.tm = 0.5f;

    float closest;
    Best best;
    if (TREE) {
        uint32_t e;
        feat_tree_solids(sc, a.gw, ray, stack, stride, closest, e);
        if (e != GBEST_NONE) best = gen_decode_best(sc, a.gw.chains, e, closest);
        else { best.kind = HIT_NONE; best.t = 0; best.prim = 0; best.chain_first = 0; best.chain_count = 0; }
    } else {
        feat_scan_solids(sc, ray, closest, best);
    }
    feat_media(sc, ray, closest, best);

    V3 alb = a.background, nrm = mk(0, 0, 0);
    float dep = 0.0f;
    if (best.kind != HIT_NONE) {
        HitRec rec;
        resolve_hit(sc, ray, best, rec);
        const int mtype = DREF_TYPE(rec.mat), midx = DREF_IDX(rec.mat);
        if (mtype == MORT_MAT_LAMBERTIAN) alb = lambert_color_rec(sc, sc.lambert[midx], rec);
        else if (mtype == MORT_MAT_ISOTROPIC) alb = lambert_color_rec(sc, sc.isotropic[midx], rec);
        else if (mtype == MORT_MAT_METAL) { const DMetal m = sc.metal[midx]; alb = mk(m.r, m.g, m.b); }
        else alb = mk(1, 1, 1); /* dielectric, diffuse_light (and an unknown tag) */
        nrm = best.kind == HIT_MEDIUM ? vneg(vunit(ray.d)) : rec.normal;
        dep = best.t * vlen(ray.d);
    }
    a.albedo[3 * lofs] = alb.x; a.albedo[3 * lofs + 1] = alb.y; a.albedo[3 * lofs + 2] = alb.z;
    a.normal[3 * lofs] = nrm.x; a.normal[3 * lofs + 1] = nrm.y; a.normal[3 * lofs + 2] = nrm.z;
    a.depth[lofs] = dep;
}

/* ---------------------------------------------------------------------------------------------------------------------
 * Denoiser: edge-avoiding a-trous wavelet filter on the demodulated colour E = C / max(A, 1e-3)
 * ------------------------------------------------------------------------------------------------------------------ */

/* e^x without libm, in the style of mort_logf: x = n ln2 + r, |r| <= ln2 / 2 (Cody-Waite split of ln2), a degree-7
 * Taylor polynomial for e^r, 2^n built from its exponent bits.  Only + - * / and conversions, so host and device round
 * every step alike.  0 below -87 (and for NaN); arguments here are <= 0. */
DEV float dn_expf(float x) {
    if (!(x >= -87.0f)) return 0.0f;
    if (x > 88.0f) x = 88.0f;
    const float tn = x * 1.44269504f;
    const int n = mort_f2i(tn >= 0.0f ? tn + 0.5f : tn - 0.5f);
    const float fn = (float)n;
    float r = x - fn * 0.693359375f;   /* ln2 high part: 9 significant bits, fn * hi is exact */
    r = r - fn * -2.12194440e-4f;      /* ln2 low part */
    float p = 1.0f / 5040.0f;
    p = p * r + 1.0f / 720.0f;
    p = p * r + 1.0f / 120.0f;
    p = p * r + 1.0f / 24.0f;
    p = p * r + 1.0f / 6.0f;
    p = p * r + 0.5f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    return p * gen_bits_float((uint32_t)(n + 127) << 23); /* n in [-126, 127] */
}

/* a filtered colour as the render would have written it (dev_render.h pixel_rgba) */
DEV uchar4 dn_rgba(float r, float g, float b) { uchar4 out; pixel_rgba(out, mk(r, g, b)); return out; }

/* B3-spline taps (1/16, 1/4, 3/8, 1/4, 1/16) */
DEV float dn_kernel(int i) { return (i == 0 || i == 4) ? 0.0625f : (i == 2 ? 0.375f : 0.25f); }

/* w_n of DESIGN.md 4.9: max(0, Np.Nq)^(2^npow) */
DEV float dn_wn(float ax, float ay, float az, float bx, float by, float bz, int npow) {
    const float nd = ax * bx + ay * by + az * bz;
    float wn = nd > 0.0f ? nd : 0.0f;
    for (int k = 0; k < npow; k++) wn = wn * wn;
    return wn;
}

/* iterations == 0, for the denoiser and the SVGF filter (Args: AtrousArgs or SvgfArgs): the accumulators unchanged and the
 * render's own rgba; either output may be null */
template <class Args>
DEV void dn_pass(const Args &a, size_t p) {
    const float r = a.C[3 * p], g = a.C[3 * p + 1], b = a.C[3 * p + 2];
    if (a.accum_out) { a.accum_out[3 * p] = r; a.accum_out[3 * p + 1] = g; a.accum_out[3 * p + 2] = b; }
    if (a.rgba_out) a.rgba_out[p] = dn_rgba(r, g, b);
}

/* One iteration of the filter over the whole image.  Internal layout, float4 per pixel:
 *   e[]  = (E.r, E.g, E.b, 0)   ping-pong between iterations
 *   g0[] = (N.x, N.y, N.z, D)   written by iteration 0
 *   g1[] = (A.r, A.g, A.b, 0)   written by iteration 0
 * Iteration 0 (FIRST) reads the caller's C / A / N / D and demodulates on the fly; the last (LAST) remodulates, applies the
 * render's NaN guard and writes accum_out / rgba_out (either may be null) instead of e_out. */
struct AtrousArgs {
    int width, height, step, npow;
    float inv_c;           /* 4^i / sigma_color^2 */
    float sd;              /* sigma_depth * step */
    float inv_a;           /* 1 / sigma_albedo^2 */
    const float *C, *A, *N, *D;
    const float4 *e_in;
    float4 *e_out, *g0, *g1;
    float *accum_out;
    uchar4 *rgba_out;
};

struct DnTap { float er, eg, eb, nx, ny, nz, d, ar, ag, ab; };

template <bool FIRST>
DEV DnTap dn_load(const AtrousArgs &a, size_t q) {
    DnTap t;
    if (FIRST) {
        t.ar = a.A[3 * q]; t.ag = a.A[3 * q + 1]; t.ab = a.A[3 * q + 2];
        t.er = a.C[3 * q] / mort_fmaxf(t.ar, 1e-3f); t.eg = a.C[3 * q + 1] / mort_fmaxf(t.ag, 1e-3f); t.eb = a.C[3 * q + 2] / mort_fmaxf(t.ab, 1e-3f);
        t.nx = a.N[3 * q]; t.ny = a.N[3 * q + 1]; t.nz = a.N[3 * q + 2];
        t.d = a.D[q];
    } else {
        const float4 e = a.e_in[q], g = a.g0[q], h = a.g1[q];
        t.er = e.x; t.eg = e.y; t.eb = e.z;
        t.nx = g.x; t.ny = g.y; t.nz = g.z; t.d = g.w;
        t.ar = h.x; t.ag = h.y; t.ab = h.z;
    }
    return t;
}

template <bool FIRST, bool LAST>
DEV void dn_pixel(const AtrousArgs &a, int x, int y) {
    const size_t p = (size_t)x + (size_t)y * (size_t)a.width;
    const DnTap c = dn_load<FIRST>(a, p);
    if (FIRST && !LAST) {
        float4 g, h;
        g.x = c.nx; g.y = c.ny; g.z = c.nz; g.w = c.d;
        h.x = c.ar; h.y = c.ag; h.z = c.ab; h.w = 0.0f;
        a.g0[p] = g; a.g1[p] = h;
    }
    const bool miss_p = c.d == 0.0f;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * a.step;
        if (qy < 0 || qy >= a.height) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * a.step;
            if (qx < 0 || qx >= a.width) continue;
            const DnTap q = dn_load<FIRST>(a, (size_t)qx + (size_t)qy * (size_t)a.width);
            const bool miss_q = q.d == 0.0f;
            if (miss_p != miss_q) continue; /* weight 0 */
            float wn = 1.0f, xd = 0.0f;
            if (!miss_p) {
                wn = dn_wn(c.nx, c.ny, c.nz, q.nx, q.ny, q.nz, a.npow);
                xd = mort_fabsf(c.d - q.d) / (a.sd * c.d);
            }
            const float der = c.er - q.er, deg = c.eg - q.eg, deb = c.eb - q.eb;
            const float xc = (der * der + deg * deg + deb * deb) * a.inv_c;
            const float dar = c.ar - q.ar, dag = c.ag - q.ag, dab = c.ab - q.ab;
            const float xa = (dar * dar + dag * dag + dab * dab) * a.inv_a;
            const float w = (dn_kernel(dx + 2) * dn_kernel(dy + 2)) * wn * dn_expf(-(xc + xd + xa));
            sr = sr + w * q.er; sg = sg + w * q.eg; sb = sb + w * q.eb;
            sw = sw + w;
        }
    }
    float er = c.er, eg = c.eg, eb = c.eb;
    if (sw > 0.0f) { er = sr / sw; eg = sg / sw; eb = sb / sw; }
    if (!LAST) {
        float4 e;
        e.x = er; e.y = eg; e.z = eb; e.w = 0.0f;
        a.e_out[p] = e;
    } else {
        /* svgf_pixel (dev_svgf.h) ends on the same tail; it is written out in both, because moving it into a function of its own
         * changes the register allocation of atrous_kernel<true, true> */
        float r = er * mort_fmaxf(c.ar, 1e-3f), g = eg * mort_fmaxf(c.ag, 1e-3f), b = eb * mort_fmaxf(c.ab, 1e-3f);
        if (r != r) r = 0.0f;
        if (g != g) g = 0.0f;
        if (b != b) b = 0.0f;
        if (a.accum_out) { a.accum_out[3 * p] = r; a.accum_out[3 * p + 1] = g; a.accum_out[3 * p + 2] = b; }
        if (a.rgba_out) a.rgba_out[p] = dn_rgba(r, g, b);
    }
}

/* iterations == 0 */
DEV void dn_passthrough(const AtrousArgs &a, int x, int y) {
    dn_pass(a, (size_t)x + (size_t)y * (size_t)a.width);
}

#endif
