/*
 * temporal.hip -- temporal accumulation across frames with camera reprojection: a non-parity extra between the
 * render and the denoiser, so that a still camera converges and a moving one keeps what it can of the frames before.
 *
 * Kernel (gfx950, wave64, 64x4-pixel workgroups: every wave covers 64 contiguous pixels of one row):
 *   tacc_kernel<STILL>   one lane per pixel, tacc_pixel (dev_temporal.h).  STILL: the previous camera is bit-identical to this
 *                        one (decided once per call on the host) and every pixel reads its own history; else the hit point is
 *                        reprojected into the previous frame and the history is a bilinear gather of up to four pixels.
 *                        History is three float4 planes in, three out; no LDS.
 *
 * The host form (mort_hip_temporal_host) runs the same body on host threads and makes no HIP runtime call.  Nothing here touches
 * the render's RNG states, tile-cost cache or counters.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "mort_hip.h"
#include "dev_temporal.h"
#include "mort_ctx.h"
#include "mort_internal.h"

#pragma clang fp contract(off)

#define FEAT_BX 64
#define FEAT_BY 4

/* ====================================================================== device */

template <bool STILL>
__global__ void __launch_bounds__(FEAT_BX * FEAT_BY) tacc_kernel(const TaccArgs a) {
    const int x = blockIdx.x * FEAT_BX + threadIdx.x, y = blockIdx.y * FEAT_BY + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    tacc_pixel<STILL>(a, x, y);
}

/* ====================================================================== host */

namespace {

/* tuned on scenes 1, 3 and 6, still and moving cameras */
const mort_temporal_params kDefaults = {0, 32, 0.02f, 0.8f};

bool params_ok(const mort_temporal_params *p) {
    if (!p) return false;
    if (p->max_samples < 0 || p->motion_max_samples < 0 || p->max_samples > (1 << 24) || p->motion_max_samples > (1 << 24)) return false;
    if (!(p->depth_tolerance >= 0.0f && p->depth_tolerance <= 1.0f)) return false;
    if (!(p->normal_min >= -1.0f && p->normal_min <= 1.0f)) return false;
    return true;
}

V3 v3_of(const mort_vec3 &v) { return mk(v.e[0], v.e[1], v.e[2]); }

bool same_vec(const mort_vec3 &a, const mort_vec3 &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

/* the previous camera is bit-identical where the reprojection looks: centre, viewport, image size */
bool camera_still(const mort_camera *prev, const mort_camera *cam) {
    return same_vec(prev->center, cam->center) && same_vec(prev->pixel00_loc, cam->pixel00_loc) && same_vec(prev->pixel_delta_u, cam->pixel_delta_u) &&
           same_vec(prev->pixel_delta_v, cam->pixel_delta_v) && prev->image_width == cam->image_width && prev->image_height == cam->image_height;
}

bool overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

/* the checks every form makes on the parameters, the cameras and the size */
int check_call(const mort_temporal_params *p, const mort_camera *prev, const mort_camera *cam, int W, int H) {
    if (!params_ok(p) || !cam) return MORT_ERR_INVALID;
    if (W <= 0 || H <= 0 || W >= 65536 * FEAT_BX || H >= 65536 * FEAT_BY) return MORT_ERR_INVALID;
    if (cam->image_width != W || cam->image_height != H || cam->sqrt_spp < 1) return MORT_ERR_INVALID;
    if (prev && (prev->image_width != W || prev->image_height != H)) return MORT_ERR_INVALID;
    return MORT_OK;
}

/* inputs present, history in iff a previous camera, no output overlapping an input or another output */
bool buffers_ok(const mort_camera *prev, int W, int H, const void *accum, const void *normal, const void *depth, const void *hin, void *hout,
                void *accum_out, void *variance_out, void *rgba_out) {
    if (!accum || !normal || !depth || !hout || (prev == nullptr) != (hin == nullptr)) return false;
    const size_t npx = (size_t)W * (size_t)H, hb = npx * MORT_TEMPORAL_HISTORY_FLOATS * sizeof(float);
    const void *ins[4] = {accum, normal, depth, hin};
    const size_t in_b[4] = {npx * 12, npx * 12, npx * 4, hb};
    void *outs[4] = {hout, accum_out, variance_out, rgba_out};
    const size_t out_b[4] = {hb, npx * 12, npx * 4, npx * 4};
    for (int o = 0; o < 4; o++) {
        for (int i = 0; i < 4; i++) if (overlap(outs[o], out_b[o], ins[i], in_b[i])) return false;
        for (int j = 0; j < o; j++) if (overlap(outs[o], out_b[o], outs[j], out_b[j])) return false;
    }
    return true;
}

/* the kernel arguments of a checked call (the same bits for the kernel and the host loop) */
int temporal_args(const mort_temporal_params *p, const mort_camera *prev, const mort_camera *cam, int W, int H, const void *accum,
                  const void *normal, const void *depth, const void *hin, void *hout, void *accum_out, void *variance_out, void *rgba_out,
                  TaccArgs &a, bool &still) {
    int st = check_call(p, prev, cam, W, H);
    if (st != MORT_OK) return st;
    if (!buffers_ok(prev, W, H, accum, normal, depth, hin, hout, accum_out, variance_out, rgba_out)) return MORT_ERR_INVALID;
    if (((uintptr_t)hout & 15u) || ((uintptr_t)hin & 15u)) return MORT_ERR_INVALID; /* float4 planes */

    std::memset(&a, 0, sizeof a);
    a.width = W; a.height = H;
    a.reset = prev == nullptr;
    still = prev == nullptr || camera_still(prev, cam);
    a.n_c = (float)(cam->sqrt_spp * cam->sqrt_spp);
    a.cap = (float)(still ? p->max_samples : p->motion_max_samples);
    a.tol = p->depth_tolerance; a.nmin = p->normal_min;
    a.center = v3_of(cam->center); a.pixel00 = v3_of(cam->pixel00_loc); a.du = v3_of(cam->pixel_delta_u); a.dv = v3_of(cam->pixel_delta_v);
    if (!still) {
        a.pc = v3_of(prev->center); a.pdu = v3_of(prev->pixel_delta_u); a.pdv = v3_of(prev->pixel_delta_v);
        a.po = vsub(v3_of(prev->pixel00_loc), a.pc);
        a.nrm = vcross(a.pdu, a.pdv);
        a.k = vdot(a.nrm, a.po);
        a.g11 = vdot(a.pdu, a.pdu); a.g12 = vdot(a.pdu, a.pdv); a.g22 = vdot(a.pdv, a.pdv);
        a.det = a.g11 * a.g22 - a.g12 * a.g12;
    }
    a.C = (const float *)accum; a.N = (const float *)normal; a.D = (const float *)depth;
    a.hin = (const float4 *)hin; a.hout = (float4 *)hout;
    a.accum_out = (float *)accum_out; a.variance_out = (float *)variance_out; a.rgba_out = (uchar4 *)rgba_out;
    return MORT_OK;
}

/* the host loop: one row of tacc_pixel (run_rows) */
struct TaccHostJob { const TaccArgs *a; bool still; };
void tacc_host_row(void *p, int y) {
    const TaccHostJob *j = (const TaccHostJob *)p;
    for (int x = 0; x < j->a->width; x++) {
        if (j->still) tacc_pixel<true>(*j->a, x, y);
        else tacc_pixel<false>(*j->a, x, y);
    }
}

} // namespace

static_assert(FEAT_BX == MORT_FEAT_BX && FEAT_BY == MORT_FEAT_BY, "mort_internal.h states the workgroup shape for view.hip");
bool mort_temporal_params_ok(const mort_temporal_params *p) { return params_ok(p); }

extern "C" int mort_hip_temporal_defaults(mort_temporal_params *p) {
    if (!p) return MORT_ERR_INVALID;
    *p = kDefaults;
    return MORT_OK;
}

extern "C" int mort_hip_temporal_device(mort_ctx *c, const mort_temporal_params *p, const mort_camera *prev_cam, const mort_camera *cam, int W,
                                        int H, const void *d_accum, const void *d_normal, const void *d_depth, const void *d_hist_in,
                                        void *d_hist_out, void *d_accum_out, void *d_variance_out, void *d_rgba_out, void *stream,
                                        double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    TaccArgs a;
    bool still;
    const int st = temporal_args(p, prev_cam, cam, W, H, d_accum, d_normal, d_depth, d_hist_in, d_hist_out, d_accum_out, d_variance_out,
                                 d_rgba_out, a, still);
    if (st != MORT_OK) return st;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    HIPCHK(c, switch_stream(c, s));
    const dim3 grid((W + FEAT_BX - 1) / FEAT_BX, (H + FEAT_BY - 1) / FEAT_BY), block(FEAT_BX, FEAT_BY);
    if (seconds) HIPCHK(c, hipEventRecord(c->ev0, s));
    if (still) hipLaunchKernelGGL(tacc_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(tacc_kernel<false>, grid, block, 0, s, a);
    HIPCHK(c, hipGetLastError());
    if (seconds) {
        HIPCHK(c, hipEventRecord(c->ev1, s));
        HIPCHK(c, hipEventSynchronize(c->ev1));
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        *seconds = ms * 1e-3;
    }
    return MORT_OK;
}

extern "C" int mort_hip_temporal(mort_ctx *c, const mort_temporal_params *p, const mort_camera *prev_cam, const mort_camera *cam, int W, int H,
                                 const float *accum, const float *normal, const float *depth, const float *hist_in, float *hist_out,
                                 float *accum_out, float *variance_out, uint8_t *rgba_out, double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    int st = check_call(p, prev_cam, cam, W, H);
    if (st != MORT_OK) return st;
    if (!buffers_ok(prev_cam, W, H, accum, normal, depth, hist_in, hist_out, accum_out, variance_out, rgba_out)) return MORT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, switch_stream(c, c->stream));
    const size_t npx = (size_t)W * (size_t)H, hf = npx * MORT_TEMPORAL_HISTORY_FLOATS;
    /* history in, history out (float4 planes first), C, N (3 floats each), D, accum_out (3 floats), variance, rgba (4 bytes) */
    st = ensure_buf(c, &c->d_tio, &c->tio_cap, (2 * hf + 12 * npx) * sizeof(float));
    if (st != MORT_OK) return st;
    float *dHi = (float *)c->d_tio, *dHo = dHi + hf, *dC = dHo + hf, *dN = dC + 3 * npx, *dD = dN + 3 * npx, *dO = dD + npx, *dV = dO + 3 * npx;
    uint8_t *dR = (uint8_t *)(dV + npx);
    HIPCHK(c, hipMemcpy(dC, accum, npx * 12, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dN, normal, npx * 12, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dD, depth, npx * 4, hipMemcpyHostToDevice));
    if (hist_in) HIPCHK(c, hipMemcpy(dHi, hist_in, hf * 4, hipMemcpyHostToDevice));
    double sec = 0;
    if ((st = mort_hip_temporal_device(c, p, prev_cam, cam, W, H, dC, dN, dD, hist_in ? dHi : nullptr, dHo, accum_out ? dO : nullptr,
                                       variance_out ? dV : nullptr, rgba_out ? dR : nullptr, c->stream, &sec)) != MORT_OK)
        return st;
    if (seconds) *seconds = sec;
    HIPCHK(c, hipMemcpy(hist_out, dHo, hf * 4, hipMemcpyDeviceToHost));
    if (accum_out) HIPCHK(c, hipMemcpy(accum_out, dO, npx * 12, hipMemcpyDeviceToHost));
    if (variance_out) HIPCHK(c, hipMemcpy(variance_out, dV, npx * 4, hipMemcpyDeviceToHost));
    if (rgba_out) HIPCHK(c, hipMemcpy(rgba_out, dR, npx * 4, hipMemcpyDeviceToHost));
    return MORT_OK;
}

extern "C" int mort_hip_temporal_host(const mort_temporal_params *p, const mort_camera *prev_cam, const mort_camera *cam, int W, int H,
                                      int nthreads, const float *accum, const float *normal, const float *depth, const float *hist_in,
                                      float *hist_out, float *accum_out, float *variance_out, uint8_t *rgba_out, double *seconds) {
    TaccArgs a;
    bool still;
    const int st = temporal_args(p, prev_cam, cam, W, H, accum, normal, depth, hist_in, hist_out, accum_out, variance_out, rgba_out, a, still);
    if (st != MORT_OK) return st;
    const double t0 = now_s();
    TaccHostJob job = {&a, still};
    run_rows(H, nthreads, tacc_host_row, &job);
    if (seconds) *seconds = now_s() - t0;
    return MORT_OK;
}
