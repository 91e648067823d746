/*
 * dev_temporal.h -- temporal accumulation with camera reprojection (the reprojection / accumulation half of SVGF, Schied et al.,
 * HPG 2017): one body per pixel, compiled for the gfx950 kernels of temporal.hip AND run by its host loop
 * (mort_hip_temporal_host), -ffp-contract=off on both sides and only + - * / sqrt, floor and conversions, so host and device
 * agree bit for bit.
 *
 * Not part of the parity path: nothing here draws a random number, touches a pixel's XORWOW state or is inlined into a render
 * kernel.  The feature pass's primary ray and the render's gamma tail come from dev_features.h, unchanged.
 */
#ifndef MORT_DEV_TEMPORAL_H
#define MORT_DEV_TEMPORAL_H

#include "dev_features.h"

#pragma clang fp contract(off)

/* History, caller-owned, three float4 planes of W*H pixels (plane k at k*W*H float4s, row 0 = bottom row):
 *   h0 = (mu.r, mu.g, mu.b, n)   accumulated linear colour, effective sample count
 *   h1 = (m1, m2, f, D)          sample-weighted means of the frame luminance and its square, frame count, this frame's depth
 *   h2 = (N.x, N.y, N.z, 0)      this frame's normal */
struct TaccArgs {
    int width, height;
    int reset;                 /* no history at all (prev_cam == NULL) */
    float n_c;                 /* this frame's effective samples, sqrt_spp^2 */
    float cap;                 /* max_samples (still) or motion_max_samples (moved); 0 = unbounded */
    float tol, nmin;           /* depth_tolerance, normal_min */
    V3 center, pixel00, du, dv; /* this frame's camera */
    /* the previous camera, moved launches only: centre c', viewport plane P00' + a du' + b dv' with normal nrm = du' x dv' at
     * signed offset k = nrm . (P00' - c'), Gram matrix of (du', dv') and its determinant */
    V3 pc, po, pdu, pdv, nrm;  /* po = P00' - c' */
    float k, g11, g12, g22, det;
    const float *C, *N, *D;    /* this frame: accumulators (3), normal (3), depth (1) */
    const float4 *hin;         /* 3 planes, null when reset */
    float4 *hout;              /* 3 planes */
    float *accum_out, *variance_out;
    uchar4 *rgba_out;
};

/* the history a pixel blends with: n == 0 = none */
struct TaccHist { float r, g, b, n, m1, m2, f; };

DEV float tacc_lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

/* STILL: the previous camera is bit-identical (the host decides once per call); the pixel's own history, no resampling */
template <bool STILL>
DEV void tacc_pixel(const TaccArgs &a, int x, int y) {
    const size_t npx = (size_t)a.width * (size_t)a.height;
    const size_t p = (size_t)x + (size_t)y * (size_t)a.width;
    float cr = a.C[3 * p], cg = a.C[3 * p + 1], cb = a.C[3 * p + 2];
    if (cr != cr) cr = 0.0f; /* the render's NaN guard */
    if (cg != cg) cg = 0.0f;
    if (cb != cb) cb = 0.0f;
    const float nx = a.N[3 * p], ny = a.N[3 * p + 1], nz = a.N[3 * p + 2];
    const float dp = a.D[p];
    const bool hit = dp > 0.0f;

    TaccHist h;
    h.r = 0.0f; h.g = 0.0f; h.b = 0.0f; h.n = 0.0f; h.m1 = 0.0f; h.m2 = 0.0f; h.f = 0.0f;
    if (!a.reset) {
        if (STILL) {
            const float4 q0 = a.hin[p], q1 = a.hin[npx + p], q2 = a.hin[2 * npx + p];
            bool ok = (q1.w > 0.0f) == hit;
            if (ok && hit) ok = mort_fabsf(q1.w - dp) <= a.tol * dp && nx * q2.x + ny * q2.y + nz * q2.z >= a.nmin;
            if (ok) { h.r = q0.x; h.g = q0.y; h.b = q0.z; h.n = q0.w; h.m1 = q1.x; h.m2 = q1.y; h.f = q1.z; }
        } else if (hit) {
            /* the feature pass's primary ray (feat_pixel), the hit point at depth dp along it */
            const V3 ps = vadd(vadd(a.pixel00, vscale((float)((double)x + 0.0), a.du)), vscale((float)((double)y + 0.0), a.dv));
            const V3 X = vadd(a.center, vscale(dp, vunit(vsub(ps, a.center))));
            /* through c' onto the previous viewport plane: c' + t r, t = k / (nrm . r) > 0; then (a, b) from the Gram system */
            const V3 r = vsub(X, a.pc);
            const float dist = vlen(r), nr = vdot(a.nrm, r);
            const float t = a.k / nr;
            if (t > 0.0f && t < 1e30f) {
                const V3 e = vsub(vscale(t, r), a.po);
                const float eu = vdot(e, a.pdu), ev = vdot(e, a.pdv);
                const float fa = (a.g22 * eu - a.g12 * ev) / a.det, fb = (a.g11 * ev - a.g12 * eu) / a.det;
                if (fa > -1.0f && fa < (float)a.width && fb > -1.0f && fb < (float)a.height) {
                    const float x0f = mort_floorf(fa), y0f = mort_floorf(fb);
                    const float fx = fa - x0f, fy = fb - y0f;
                    const int x0 = (int)x0f, y0 = (int)y0f;
                    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sn = 0.0f, s1 = 0.0f, s2 = 0.0f, sf = 0.0f, sw = 0.0f;
#pragma unroll
                    for (int j = 0; j < 2; j++) {
#pragma unroll
                        for (int i = 0; i < 2; i++) {
                            const int qx = x0 + i, qy = y0 + j;
                            if (qx < 0 || qx >= a.width || qy < 0 || qy >= a.height) continue;
                            const size_t q = (size_t)qx + (size_t)qy * (size_t)a.width;
                            const float4 q1 = a.hin[npx + q];
                            if (!(q1.w > 0.0f) || !(mort_fabsf(q1.w - dist) <= a.tol * dist)) continue;
                            const float4 q2 = a.hin[2 * npx + q];
                            if (!(nx * q2.x + ny * q2.y + nz * q2.z >= a.nmin)) continue;
                            const float4 q0 = a.hin[q];
                            const float w = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
                            sr = sr + w * q0.x; sg = sg + w * q0.y; sb = sb + w * q0.z; sn = sn + w * q0.w;
                            s1 = s1 + w * q1.x; s2 = s2 + w * q1.y; sf = sf + w * q1.z;
                            sw = sw + w;
                        }
                    }
                    if (sw > 1e-3f) {
                        h.r = sr / sw; h.g = sg / sw; h.b = sb / sw; h.n = sn / sw; h.m1 = s1 / sw; h.m2 = s2 / sw; h.f = sf / sw;
                    }
                }
            }
        }
    }
    /* the cap: at most `cap` effective samples after the blend */
    if (a.cap > 0.0f && h.n > 0.0f && h.n + a.n_c > a.cap) {
        const float s = mort_fmaxf(0.0f, a.cap - a.n_c) / h.n;
        h.n = h.n * s; h.f = h.f * s;
    }
    const float L = tacc_lum(cr, cg, cb);
    const float n1 = h.n + a.n_c;
    const float mr = (h.n * h.r + a.n_c * cr) / n1, mg = (h.n * h.g + a.n_c * cg) / n1, mb = (h.n * h.b + a.n_c * cb) / n1;
    const float m1 = (h.n * h.m1 + a.n_c * L) / n1, m2 = (h.n * h.m2 + a.n_c * (L * L)) / n1;
    const float f1 = h.f + 1.0f;
    float4 o0, o1, o2;
    o0.x = mr; o0.y = mg; o0.z = mb; o0.w = n1;
    o1.x = m1; o1.y = m2; o1.z = f1; o1.w = dp;
    o2.x = nx; o2.y = ny; o2.z = nz; o2.w = 0.0f;
    a.hout[p] = o0; a.hout[npx + p] = o1; a.hout[2 * npx + p] = o2;
    if (a.accum_out) { a.accum_out[3 * p] = mr; a.accum_out[3 * p + 1] = mg; a.accum_out[3 * p + 2] = mb; }
    if (a.rgba_out) a.rgba_out[p] = dn_rgba(mr, mg, mb);
    if (a.variance_out) a.variance_out[p] = f1 >= 2.0f ? mort_fmaxf(0.0f, m2 - m1 * m1) / (f1 - 1.0f) : -1.0f;
}

#endif
