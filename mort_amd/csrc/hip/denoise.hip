/*
 * denoise.hip -- first-hit feature buffers and the edge-aware a-trous denoiser: a non-parity extra on top
 * of the untouched render path, for a viewable image at the sample counts an interactive frame can afford.
 *
 * Kernels (gfx950, wave64, the stages' 64x4-pixel workgroups of stage_common.h: every wave covers 64 contiguous pixels of one row):
 *   feat_kernel<TREE>             one primary ray per pixel (lens centre -> pixel centre, tm = 0.5), no random numbers:
 *                                 albedo, normal, depth of the first hit.  TREE: the unified-tree walk with its pending
 *                                 children in LDS (16 x 256 x 2 B), else the item scan.  Reads the scene in HBM.
 *   atrous_kernel<FIRST, LAST>    one a-trous iteration, 5x5 taps at step 2^i; iteration 0 demodulates the caller's buffers,
 *                                 the last remodulates and writes the accumulators and the rgba: n launches for n iterations
 *   atrous_passthrough_kernel     iterations == 0: the accumulators and the render's own rgba
 *
 * The host forms (mort_hip_render_features_host, mort_hip_denoise_host) run the same per-pixel bodies (dev_features.h)
 * on host threads and make no HIP runtime call.  Nothing here touches the render's RNG states, tile-cost cache or counters.
 * The _device entry points' prologue and timed epilogue, the staging of the host-buffer forms and the shared scratch are
 * stage_common.h's, as in temporal.hip and svgf.hip.
 */
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "mort_hip.h"
#include "dev_features.h"
#include "scene_blob.h"
#include "mort_ctx.h"
#include "mort_internal.h"
#include "stage_common.h"

#pragma clang fp contract(off)

/* ====================================================================== device */

template <bool TREE>
__global__ void __launch_bounds__(STAGE_BX * STAGE_BY) feat_kernel(const FeatArgs a) {
    __shared__ unsigned short feat_stack[MORT_OWN_STACK * STAGE_BX * STAGE_BY];
    const int tid = threadIdx.x + threadIdx.y * STAGE_BX;
    const int x = blockIdx.x * STAGE_BX + threadIdx.x, ly = blockIdx.y * STAGE_BY + threadIdx.y;
    if (x >= a.width || ly >= a.local_rows) return;
    feat_pixel<TREE>(a, x, ly, &feat_stack[tid], STAGE_BX * STAGE_BY);
}

template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(STAGE_BX * STAGE_BY) atrous_kernel(const AtrousArgs a) {
    const int x = blockIdx.x * STAGE_BX + threadIdx.x, y = blockIdx.y * STAGE_BY + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    dn_pixel<FIRST, LAST>(a, x, y);
}

__global__ void __launch_bounds__(STAGE_BX * STAGE_BY) atrous_passthrough_kernel(const AtrousArgs a) {
    const int x = blockIdx.x * STAGE_BX + threadIdx.x, y = blockIdx.y * STAGE_BY + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    dn_passthrough(a, x, y);
}

/* ====================================================================== host */

namespace {

/* tuned on scenes 1, 3 and 6 at 4 spp */
const mort_denoise_params kDefaults = {5, 2.0f, 0.1f, 0.05f, 3};

bool params_ok(const mort_denoise_params *p) {
    if (!p) return false;
    if (p->iterations < 0 || p->iterations > 8) return false;
    if (p->normal_log2_power < 0 || p->normal_log2_power > 16) return false;
    const float s[3] = {p->sigma_color, p->sigma_depth, p->sigma_albedo};
    for (float v : s) if (!(v > 0.0f && v < 1e30f)) return false;
    return true;
}

/* the arguments of iteration i of n (buffers filled in by the caller) */
AtrousArgs atrous_args(const mort_denoise_params *p, int W, int H, int i) {
    AtrousArgs a;
    std::memset(&a, 0, sizeof a);
    a.width = W; a.height = H;
    a.step = 1 << i;
    a.npow = p->normal_log2_power;
    a.inv_c = (float)(1 << (2 * i)) / (p->sigma_color * p->sigma_color); /* the colour sigma halves every iteration */
    a.sd = p->sigma_depth * (float)a.step;
    a.inv_a = 1.0f / (p->sigma_albedo * p->sigma_albedo);
    return a;
}

struct FeatHostJob { FeatArgs a; bool tree; };
void feat_host_row(void *p, int ly) {
    const FeatHostJob *j = (const FeatHostJob *)p;
    unsigned short stack[MORT_OWN_STACK];
    for (int x = 0; x < j->a.width; x++) {
        if (j->tree) feat_pixel<true>(j->a, x, ly, stack, 1);
        else feat_pixel<false>(j->a, x, ly, stack, 1);
    }
}

struct DnHostJob { AtrousArgs a; int first, last, pass; };
void dn_host_row(void *p, int y) {
    const DnHostJob *j = (const DnHostJob *)p;
    for (int x = 0; x < j->a.width; x++) {
        if (j->pass) dn_passthrough(j->a, x, y);
        else if (j->first && j->last) dn_pixel<true, true>(j->a, x, y);
        else if (j->first) dn_pixel<true, false>(j->a, x, y);
        else if (j->last) dn_pixel<false, true>(j->a, x, y);
        else dn_pixel<false, false>(j->a, x, y);
    }
}

void feat_camera(FeatArgs &a, const mort_camera *cam) {
    a.width = cam->image_width; a.height = cam->image_height;
    a.background = to_v3(cam->background); a.center = to_v3(cam->center); a.pixel00 = to_v3(cam->pixel00_loc);
    a.du = to_v3(cam->pixel_delta_u); a.dv = to_v3(cam->pixel_delta_v);
}

} // namespace

bool mort_denoise_params_ok(const mort_denoise_params *p) { return params_ok(p); }

extern "C" int mort_hip_denoise_defaults(mort_denoise_params *p) {
    if (!p) return MORT_ERR_INVALID;
    *p = kDefaults;
    return MORT_OK;
}

/* ---------------------------------------------------------------------------------------------- feature pass */

extern "C" int mort_hip_render_features_device(mort_ctx *c, const mort_camera *cam, void *d_albedo, void *d_normal, void *d_depth,
                                               void *stream, double *seconds) {
    if (!c || !cam || !d_albedo || !d_normal || !d_depth) return MORT_ERR_INVALID;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    const int W = cam->image_width, H = cam->image_height;
    if (!stage_size_ok(W, H)) return MORT_ERR_INVALID;

    FeatArgs a;
    std::memset(&a, 0, sizeof a);
    a.sc = c->sc;
    feat_camera(a, cam);
    a.rank = c->part.rank; a.nranks = c->part.nranks; a.rows_per_block = c->part.rows_per_block;
    a.local_rows = mort_hip_local_rows(c, H);
    a.albedo = (float *)d_albedo; a.normal = (float *)d_normal; a.depth = (float *)d_depth;
    const bool tree = c->gen_ok && camera_in_reach(cam, c->gen_lo, c->gen_hi, c->gen_reach, 0.0f);
    if (tree) {
        const unsigned char *g = (const unsigned char *)c->d_gen;
        a.gw.nodes = (const DNodeQ *)(g + c->gen.o_nodes); a.gw.entries = (const uint32_t *)(g + c->gen.o_entries);
        a.gw.chains = (const int *)(g + c->gen.o_chains); a.gw.ranks = c->gen.ranks; a.gw.n_spheres = c->gen.n_spheres;
        a.gw.n_chains = c->gen.n_chains; a.gw.root = c->gen.root; a.gw.first_medium = c->gen.first_medium;
        a.gw.gx = c->gen.gx; a.gw.gy = c->gen.gy; a.gw.gz = c->gen.gz; a.gw.gR = c->gen.gR; a.gw.mnear = c->gen.mnear; a.gw.kmin = c->gen.kmin;
    }
    hipStream_t s;
    const int st = stage_begin(c, stream, 0, seconds, &s);
    if (st != MORT_OK) return st;
    if (a.local_rows > 0) {
        const dim3 grid = stage_grid(W, a.local_rows), block = stage_block();
        if (tree) hipLaunchKernelGGL(feat_kernel<true>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(feat_kernel<false>, grid, block, 0, s, a);
        HIPCHK(c, hipGetLastError());
    }
    return stage_end(c, s, seconds);
}

extern "C" int mort_hip_render_features(mort_ctx *c, const mort_camera *cam, float *albedo_out, float *normal_out, float *depth_out,
                                        double *seconds) {
    if (!c || !cam || !albedo_out || !normal_out || !depth_out) return MORT_ERR_INVALID;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    const int W = cam->image_width, H = cam->image_height;
    if (W <= 0 || H <= 0) return MORT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const int lr = mort_hip_local_rows(c, H);
    const size_t npx = (size_t)W * (size_t)lr;
    HIPCHK(c, switch_stream(c, c->stream));
    /* the packed owned rows: the whole image without a partition */
    StagePlane pl[3] = {{nullptr, albedo_out, npx * 12}, {nullptr, normal_out, npx * 12}, {nullptr, depth_out, npx * 4}};
    int st = stage_upload(c, pl, 3);
    if (st != MORT_OK) return st;
    float *d_alb = (float *)pl[0].dev, *d_nrm = (float *)pl[1].dev, *d_dep = (float *)pl[2].dev;
    double sec = 0;
    if ((st = mort_hip_render_features_device(c, cam, d_alb, d_nrm, d_dep, c->stream, &sec)) != MORT_OK) return st;
    if (seconds) *seconds = sec;
    if (c->part.nranks == 1) return stage_download(c, pl, 3);
    for (int ly = 0; ly < lr; ly++) {
        const size_t y = (size_t)mort_hip_global_row(c, ly), W3 = (size_t)W * 3;
        HIPCHK(c, hipMemcpy(albedo_out + y * W3, d_alb + (size_t)ly * W3, W3 * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(normal_out + y * W3, d_nrm + (size_t)ly * W3, W3 * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(depth_out + y * W, d_dep + (size_t)ly * W, (size_t)W * 4, hipMemcpyDeviceToHost));
    }
    return MORT_OK;
}

extern "C" int mort_hip_render_features_host(const mort_world *world, const mort_camera *cam, int nthreads, int flags, float *albedo_out,
                                             float *normal_out, float *depth_out, double *seconds) {
    if (!world || !cam || !albedo_out || !normal_out || !depth_out) return MORT_ERR_INVALID;
    const int W = cam->image_width, H = cam->image_height;
    if (W <= 0 || H <= 0) return MORT_ERR_INVALID;
    SceneBlob sb;
    const int st = build_scene_blob(world, sb);
    if (st != MORT_OK) return st;
    FeatHostJob job;
    std::memset(&job.a, 0, sizeof job.a);
    scene_view(sb, sb.bytes.data(), job.a.sc);
    feat_camera(job.a, cam);
    job.a.rank = 0; job.a.nranks = 1; job.a.rows_per_block = 8; job.a.local_rows = H;
    job.a.albedo = albedo_out; job.a.normal = normal_out; job.a.depth = depth_out;
    const mortc::Compiled &o = sb.comp;
    job.tree = (flags & MORT_HOST_TREE) && o.g_ok && camera_in_reach(cam, o.g_lo, o.g_hi, o.g_reach, 0.0f);
    if (job.tree) job.a.gw = gen_walk_of(o);
    const double t0 = now_s();
    run_rows(H, nthreads, feat_host_row, &job);
    if (seconds) *seconds = now_s() - t0;
    return MORT_OK;
}

/* ---------------------------------------------------------------------------------------------- denoiser */

extern "C" int mort_hip_denoise_device(mort_ctx *c, const mort_denoise_params *p, int W, int H, const void *d_accum, const void *d_albedo,
                                       const void *d_normal, const void *d_depth, void *d_accum_out, void *d_rgba_out, void *stream,
                                       double *seconds) {
    if (!c || !params_ok(p) || !d_accum || !d_albedo || !d_normal || !d_depth) return MORT_ERR_INVALID;
    if (!stage_size_ok(W, H)) return MORT_ERR_INVALID;
    const size_t npx = (size_t)W * (size_t)H;
    const int n = p->iterations;
    hipStream_t s;
    const int st = stage_begin(c, stream, n > 1 ? npx * 4 * sizeof(float4) : 0, seconds, &s); /* e ping-pong, g0, g1 */
    if (st != MORT_OK) return st;
    float4 *e0 = (float4 *)c->stage_planes.p, *e1 = e0 + npx, *g0 = e1 + npx, *g1 = g0 + npx; /* not dereferenced where n <= 1 */
    const dim3 grid = stage_grid(W, H), block = stage_block();
    for (int i = 0; i < (n > 0 ? n : 1); i++) {
        AtrousArgs a = atrous_args(p, W, H, i);
        a.C = (const float *)d_accum; a.A = (const float *)d_albedo; a.N = (const float *)d_normal; a.D = (const float *)d_depth;
        a.e_in = (i & 1) ? e1 : e0; a.e_out = (i & 1) ? e0 : e1; a.g0 = g0; a.g1 = g1;
        a.accum_out = (float *)d_accum_out; a.rgba_out = (uchar4 *)d_rgba_out;
        const bool first = i == 0, last = i == n - 1;
        if (n == 0) hipLaunchKernelGGL(atrous_passthrough_kernel, grid, block, 0, s, a);
        else if (first && last) hipLaunchKernelGGL((atrous_kernel<true, true>), grid, block, 0, s, a);
        else if (first) hipLaunchKernelGGL((atrous_kernel<true, false>), grid, block, 0, s, a);
        else if (last) hipLaunchKernelGGL((atrous_kernel<false, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((atrous_kernel<false, false>), grid, block, 0, s, a);
        HIPCHK(c, hipGetLastError());
    }
    return stage_end(c, s, seconds);
}

extern "C" int mort_hip_denoise(mort_ctx *c, const mort_denoise_params *p, int W, int H, const float *accum, const float *albedo,
                                const float *normal, const float *depth, float *accum_out, uint8_t *rgba_out, double *seconds) {
    if (!c || !params_ok(p) || !accum || !albedo || !normal || !depth) return MORT_ERR_INVALID;
    if (W <= 0 || H <= 0) return MORT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, switch_stream(c, c->stream));
    const size_t npx = (size_t)W * (size_t)H;
    StagePlane pl[6] = {{accum, nullptr, npx * 12}, {albedo, nullptr, npx * 12}, {normal, nullptr, npx * 12}, {depth, nullptr, npx * 4},
                        {nullptr, accum_out, npx * 12}, {nullptr, rgba_out, npx * 4}};
    int st = stage_upload(c, pl, 6);
    if (st != MORT_OK) return st;
    double sec = 0;
    if ((st = mort_hip_denoise_device(c, p, W, H, pl[0].dev, pl[1].dev, pl[2].dev, pl[3].dev, pl[4].dev, pl[5].dev, c->stream, &sec)) != MORT_OK)
        return st;
    if (seconds) *seconds = sec;
    return stage_download(c, pl, 6);
}

extern "C" int mort_hip_denoise_host(const mort_denoise_params *p, int W, int H, int nthreads, const float *accum, const float *albedo,
                                     const float *normal, const float *depth, float *accum_out, uint8_t *rgba_out, double *seconds) {
    if (!params_ok(p) || !accum || !albedo || !normal || !depth) return MORT_ERR_INVALID;
    if (W <= 0 || H <= 0) return MORT_ERR_INVALID;
    const size_t npx = (size_t)W * (size_t)H;
    const int n = p->iterations;
    std::vector<float4> buf(n > 1 ? npx * 4 : 0);
    float4 *e0 = buf.data(), *e1 = e0 ? e0 + npx : nullptr, *g0 = e1 ? e1 + npx : nullptr, *g1 = g0 ? g0 + npx : nullptr;
    const double t0 = now_s();
    for (int i = 0; i < (n > 0 ? n : 1); i++) {
        DnHostJob job;
        job.a = atrous_args(p, W, H, i);
        job.a.C = accum; job.a.A = albedo; job.a.N = normal; job.a.D = depth;
        job.a.e_in = (i & 1) ? e1 : e0; job.a.e_out = (i & 1) ? e0 : e1; job.a.g0 = g0; job.a.g1 = g1;
        job.a.accum_out = accum_out; job.a.rgba_out = (uchar4 *)rgba_out;
        job.pass = n == 0; job.first = i == 0; job.last = i == n - 1;
        run_rows(H, nthreads, dn_host_row, &job);
    }
    if (seconds) *seconds = now_s() - t0;
    return MORT_OK;
}
