/*
 * dev_svgf.h -- the SVGF filter stage (Schied et al., HPG 2017): a variance-guided a-trous filter over the
 * accumulated colour.  One body per pixel, compiled for the gfx950 kernels of svgf.hip AND run by its host loop
 * (mort_hip_svgf_host), -ffp-contract=off on both sides and only + - * / sqrt, conversions and dn_expf, sums in the order
 * written here, so host and device agree bit for bit.
 *
 * Not part of the parity path: nothing here draws a random number, touches a pixel's XORWOW state or is inlined into a render
 * kernel.  dn_expf, dn_kernel, dn_rgba, the normal weight dn_wn and the pass-through body dn_pass come from dev_features.h, shared
 * with the denoiser.
 *
 * A body reads its taps through a source object (tap(qx, qy), var(qx, qy)): the buffers in memory (the host loop, and the
 * kernels that load every tap from global memory) or a workgroup's tile staged in LDS.  The arithmetic and its order do not
 * depend on the source, so the choice cannot change a bit of the result.
 */
#ifndef MORT_DEV_SVGF_H
#define MORT_DEV_SVGF_H

#include "dev_features.h"

#pragma clang fp contract(off)

/* Internal layout, float4 per pixel:
 *   e[]  = (E.r, E.g, E.b, Var)  demodulated colour and the variance of its luminance; ping-pong between iterations
 *   g0[] = (N.x, N.y, N.z, D)    written by the prepare pass
 *   g1[] = (A.r, A.g, A.b, 0)    written by the prepare pass */
struct SvgfArgs {
    int width, height, step, npow;
    float sl;              /* sigma_luminance */
    float sd1;             /* sigma_depth (the prepare pass scales it by the tap's ring) */
    float sd;              /* sigma_depth * step */
    float inv_a;           /* 1 / sigma_albedo^2 */
    const float *C, *A, *N, *D, *V; /* the caller's buffers; V may be null */
    const float4 *e_in;
    float4 *e_out, *g0, *g1;
    float *accum_out, *variance_out;
    uchar4 *rgba_out;
};

DEV float sv_lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

/* ---------------------------------------------------------------------------------------------------------------------
 * Prepare: demodulate, pack the features, set the variance of l(E) (from the temporal variance, or the spatial estimate)
 * ------------------------------------------------------------------------------------------------------------------ */
struct SvPrepTap { float l, nx, ny, nz, d; };

/* what the prepare pass needs of pixel q from the caller's buffers */
DEV SvPrepTap sv_prep_load(const SvgfArgs &a, size_t q) {
    SvPrepTap t;
    const float er = a.C[3 * q] / mort_fmaxf(a.A[3 * q], 1e-3f), eg = a.C[3 * q + 1] / mort_fmaxf(a.A[3 * q + 1], 1e-3f),
                eb = a.C[3 * q + 2] / mort_fmaxf(a.A[3 * q + 2], 1e-3f);
    t.l = sv_lum(er, eg, eb);
    t.nx = a.N[3 * q]; t.ny = a.N[3 * q + 1]; t.nz = a.N[3 * q + 2];
    t.d = a.D[q];
    return t;
}

struct SvPrepGlobal {
    const SvgfArgs *a;
    DEV SvPrepTap tap(int qx, int qy) const { return sv_prep_load(*a, (size_t)qx + (size_t)qy * (size_t)a->width); }
};

/* a workgroup's tile: pixel (x0 + i, y0 + j) at [i + j * pitch], nd = (N, D), l = l(E) */
struct SvPrepTile {
    const float4 *nd;
    const float *l;
    int x0, y0, pitch;
    DEV SvPrepTap tap(int qx, int qy) const {
        const int i = (qx - x0) + (qy - y0) * pitch;
        const float4 g = nd[i];
        SvPrepTap t;
        t.l = l[i]; t.nx = g.x; t.ny = g.y; t.nz = g.z; t.d = g.w;
        return t;
    }
};

template <bool HAVE_VAR, class Src>
DEV void svgf_prep_pixel(const SvgfArgs &a, const Src &src, int x, int y) {
    const size_t p = (size_t)x + (size_t)y * (size_t)a.width;
    const float ar = a.A[3 * p], ag = a.A[3 * p + 1], ab = a.A[3 * p + 2];
    const float mr = mort_fmaxf(ar, 1e-3f), mg = mort_fmaxf(ag, 1e-3f), mb = mort_fmaxf(ab, 1e-3f);
    const float nx = a.N[3 * p], ny = a.N[3 * p + 1], nz = a.N[3 * p + 2], dp = a.D[p];
    float4 e, g, h;
    e.x = a.C[3 * p] / mr; e.y = a.C[3 * p + 1] / mg; e.z = a.C[3 * p + 2] / mb;
    g.x = nx; g.y = ny; g.z = nz; g.w = dp;
    h.x = ar; h.y = ag; h.z = ab; h.w = 0.0f;

    float var = 0.0f;
    bool known = false;
    if (HAVE_VAR) {
        const float v = a.V[p];
        if (v >= 0.0f) { /* a negative value (and NaN): unknown */
            const float k = sv_lum(mr, mg, mb);
            var = v / (k * k);
            known = true;
        }
    }
    if (!known) { /* the spatial estimate: weighted moments of l over the 5x5 window at step 1 */
        const bool miss_p = dp == 0.0f;
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
            const int qy = y + dy;
            if (qy < 0 || qy >= a.height) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int qx = x + dx;
                if (qx < 0 || qx >= a.width) continue;
                const SvPrepTap q = src.tap(qx, qy);
                const bool miss_q = q.d == 0.0f;
                if (miss_p != miss_q) continue;
                float wn = 1.0f, xd = 0.0f;
                if (!miss_p) {
                    wn = dn_wn(nx, ny, nz, q.nx, q.ny, q.nz, a.npow);
                    const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, ring = ax > ay ? ax : ay;
                    if (ring > 0) xd = mort_fabsf(dp - q.d) / ((a.sd1 * (float)ring) * dp);
                }
                const float w = wn * dn_expf(-xd);
                s0 = s0 + w; s1 = s1 + w * q.l; s2 = s2 + w * (q.l * q.l);
            }
        }
        if (s0 > 0.0f) {
            const float m1 = s1 / s0, m2 = s2 / s0;
            var = m2 - m1 * m1;
            if (!(var > 0.0f)) var = 0.0f;
        }
    }
    e.w = var;
    a.e_out[p] = e; a.g0[p] = g; a.g1[p] = h;
}

/* ---------------------------------------------------------------------------------------------------------------------
 * One iteration at step 2^i
 * ------------------------------------------------------------------------------------------------------------------ */
struct SvTap { float er, eg, eb, var, nx, ny, nz, d, ar, ag, ab; };

DEV SvTap sv_tap(float4 e, float4 g, float4 h) {
    SvTap t;
    t.er = e.x; t.eg = e.y; t.eb = e.z; t.var = e.w;
    t.nx = g.x; t.ny = g.y; t.nz = g.z; t.d = g.w;
    t.ar = h.x; t.ag = h.y; t.ab = h.z;
    return t;
}

struct SvGlobal {
    const float4 *e, *g0, *g1;
    int width;
    DEV SvTap tap(int qx, int qy) const {
        const size_t q = (size_t)qx + (size_t)qy * (size_t)width;
        return sv_tap(e[q], g0[q], g1[q]);
    }
    DEV float var(int qx, int qy) const { return e[(size_t)qx + (size_t)qy * (size_t)width].w; }
};

/* a workgroup's tile, three float4 planes: pixel (x0 + i, y0 + j) at [i + j * pitch] */
struct SvTile {
    const float4 *e, *g0, *g1;
    int x0, y0, pitch;
    DEV SvTap tap(int qx, int qy) const {
        const int i = (qx - x0) + (qy - y0) * pitch;
        return sv_tap(e[i], g0[i], g1[i]);
    }
    DEV float var(int qx, int qy) const { return e[(qx - x0) + (qy - y0) * pitch].w; }
};

template <bool LAST, class Src>
DEV void svgf_pixel(const SvgfArgs &a, const Src &src, int x, int y) {
    const size_t p = (size_t)x + (size_t)y * (size_t)a.width;
    const SvTap c = src.tap(x, y);
    /* g_p: the 3x3 Gaussian (1/4, 1/2, 1/4)^2 of Var around p at step 1, renormalised by the in-image weight */
    float gs = 0.0f, gw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= a.height) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= a.width) continue;
            const float wt = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
            gs = gs + wt * src.var(qx, qy);
            gw = gw + wt;
        }
    }
    /* g_p = 0 leaves 1e-6: any luminance difference then gives an argument below -87, where dn_expf is exactly 0, and an
     * equal luminance gives x_l = 0.  A NaN variance makes every weight 0 (dn_expf(NaN) = 0): the pixel stays as it is */
    const float lden = a.sl * mort_sqrtf(gs / gw) + 1e-6f;
    const float lp = sv_lum(c.er, c.eg, c.eb);
    const bool miss_p = c.d == 0.0f;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f, sw = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * a.step;
        if (qy < 0 || qy >= a.height) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * a.step;
            if (qx < 0 || qx >= a.width) continue;
            const SvTap q = src.tap(qx, qy);
            const bool miss_q = q.d == 0.0f;
            if (miss_p != miss_q) continue; /* weight 0 */
            float wn = 1.0f, xd = 0.0f;
            if (!miss_p) {
                wn = dn_wn(c.nx, c.ny, c.nz, q.nx, q.ny, q.nz, a.npow);
                xd = mort_fabsf(c.d - q.d) / (a.sd * c.d);
            }
            const float xl = mort_fabsf(lp - sv_lum(q.er, q.eg, q.eb)) / lden;
            const float dar = c.ar - q.ar, dag = c.ag - q.ag, dab = c.ab - q.ab;
            const float xa = (dar * dar + dag * dag + dab * dab) * a.inv_a;
            const float w = (dn_kernel(dx + 2) * dn_kernel(dy + 2)) * wn * dn_expf(-(xl + xd + xa));
            sr = sr + w * q.er; sg = sg + w * q.eg; sb = sb + w * q.eb;
            sv = sv + (w * w) * q.var;
            sw = sw + w;
        }
    }
    float er = c.er, eg = c.eg, eb = c.eb, var = c.var;
    if (sw > 0.0f) { er = sr / sw; eg = sg / sw; eb = sb / sw; var = sv / (sw * sw); }
    if (!LAST) {
        float4 e;
        e.x = er; e.y = eg; e.z = eb; e.w = var;
        a.e_out[p] = e;
    } else {
        const float mr = mort_fmaxf(c.ar, 1e-3f), mg = mort_fmaxf(c.ag, 1e-3f), mb = mort_fmaxf(c.ab, 1e-3f);
        float r = er * mr, g = eg * mg, b = eb * mb;
        if (r != r) r = 0.0f;
        if (g != g) g = 0.0f;
        if (b != b) b = 0.0f;
        if (a.accum_out) { a.accum_out[3 * p] = r; a.accum_out[3 * p + 1] = g; a.accum_out[3 * p + 2] = b; }
        if (a.rgba_out) a.rgba_out[p] = dn_rgba(r, g, b);
        if (a.variance_out) { const float k = sv_lum(mr, mg, mb); a.variance_out[p] = var * (k * k); }
    }
}

/* iterations == 0: the accumulators unchanged, the render's own rgba and the prepared variance */
DEV void svgf_passthrough(const SvgfArgs &a, int x, int y) {
    const size_t p = (size_t)x + (size_t)y * (size_t)a.width;
    dn_pass(a, p);
    if (a.variance_out) {
        const float4 h = a.g1[p];
        const float k = sv_lum(mort_fmaxf(h.x, 1e-3f), mort_fmaxf(h.y, 1e-3f), mort_fmaxf(h.z, 1e-3f));
        a.variance_out[p] = a.e_in[p].w * (k * k);
    }
}

#endif
