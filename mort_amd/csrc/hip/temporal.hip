/*
 * temporal.hip -- temporal accumulation across frames with camera reprojection: a non-parity extra between the
 * render and the denoiser, so that a still camera converges and a moving one keeps what it can of the frames before.
 *
 * Kernel (gfx950, wave64, the stages' 64x4-pixel workgroups of stage_common.h: every wave covers 64 contiguous pixels of one row):
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
#include "stage_common.h"

#pragma clang fp contract(off)

/* ====================================================================== device */

template <bool STILL>
__global__ void __launch_bounds__(STAGE_BX * STAGE_BY) tacc_kernel(const TaccArgs a) {
    const int x = blockIdx.x * STAGE_BX + threadIdx.x, y = blockIdx.y * STAGE_BY + threadIdx.y;
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

/* the previous camera is bit-identical where the reprojection looks: centre, viewport, image size */
bool camera_still(const mort_camera *prev, const mort_camera *cam) {
    return same_vec(prev->center, cam->center) && same_vec(prev->pixel00_loc, cam->pixel00_loc) && same_vec(prev->pixel_delta_u, cam->pixel_delta_u) &&
           same_vec(prev->pixel_delta_v, cam->pixel_delta_v) && prev->image_width == cam->image_width && prev->image_height == cam->image_height;
}

/* the checks every form makes on the parameters, the cameras and the size */
int check_call(const mort_temporal_params *p, const mort_camera *prev, const mort_camera *cam, int W, int H) {
    if (!params_ok(p) || !cam) return MORT_ERR_INVALID;
    if (!stage_size_ok(W, H)) return MORT_ERR_INVALID;
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
    return buffers_disjoint(ins, in_b, 4, outs, out_b, 4);
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
    a.center = to_v3(cam->center); a.pixel00 = to_v3(cam->pixel00_loc); a.du = to_v3(cam->pixel_delta_u); a.dv = to_v3(cam->pixel_delta_v);
    if (!still) {
        a.pc = to_v3(prev->center); a.pdu = to_v3(prev->pixel_delta_u); a.pdv = to_v3(prev->pixel_delta_v);
        a.po = vsub(to_v3(prev->pixel00_loc), a.pc);
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
    int st = temporal_args(p, prev_cam, cam, W, H, d_accum, d_normal, d_depth, d_hist_in, d_hist_out, d_accum_out, d_variance_out,
                           d_rgba_out, a, still);
    if (st != MORT_OK) return st;
    hipStream_t s;
    if ((st = stage_begin(c, stream, 0, seconds, &s)) != MORT_OK) return st;
    if (still) hipLaunchKernelGGL(tacc_kernel<true>, stage_grid(W, H), stage_block(), 0, s, a);
    else hipLaunchKernelGGL(tacc_kernel<false>, stage_grid(W, H), stage_block(), 0, s, a);
    HIPCHK(c, hipGetLastError());
    return stage_end(c, s, seconds);
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
    const size_t npx = (size_t)W * (size_t)H, hb = npx * MORT_TEMPORAL_HISTORY_FLOATS * sizeof(float);
    StagePlane pl[8] = {{accum, nullptr, npx * 12}, {normal, nullptr, npx * 12}, {depth, nullptr, npx * 4}, {hist_in, nullptr, hb},
                        {nullptr, hist_out, hb}, {nullptr, accum_out, npx * 12}, {nullptr, variance_out, npx * 4}, {nullptr, rgba_out, npx * 4}};
    if ((st = stage_upload(c, pl, 8)) != MORT_OK) return st;
    double sec = 0;
    if ((st = mort_hip_temporal_device(c, p, prev_cam, cam, W, H, pl[0].dev, pl[1].dev, pl[2].dev, pl[3].dev, pl[4].dev, pl[5].dev, pl[6].dev,
                                       pl[7].dev, c->stream, &sec)) != MORT_OK)
        return st;
    if (seconds) *seconds = sec;
    return stage_download(c, pl, 8);
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
