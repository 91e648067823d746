/*
 * svgf.hip -- the SVGF filter stage: a variance-guided a-trous filter over the accumulated colour, fed by the
 * variance that temporal accumulation writes (temporal.hip) or, where that is unknown, by a spatial estimate.  A non-parity
 * extra like the denoiser (denoise.hip) and the temporal step.
 *
 * Kernels (gfx950, wave64, the stages' 64x4-pixel workgroups of stage_common.h: every wave covers 64 contiguous pixels of one row):
 *   svgf_prep_kernel<HAVE_VAR, TILE>   demodulates, packs (N, D) and A as float4, sets the variance of the demodulated
 *                                      luminance: V / k^2 where the caller's variance is known, else the 5x5 spatial estimate.
 *                                      TILE: the workgroup's 68x8 neighbourhood (l, N, D) staged in LDS (10.6 KB); with
 *                                      HAVE_VAR only in workgroups that hold a pixel of unknown variance.
 *   svgf_iter_kernel<LAST, TILE>       one iteration, 5x5 taps at step 2^i plus the 3x3 variance prefilter; the last one
 *                                      remodulates and writes accum / rgba / variance.  TILE = 1, 2: iterations 0 / 1 with
 *                                      the (64 + 4s) x (4 + 4s) neighbourhood staged in LDS as three float4 planes (25.5 KB,
 *                                      40.5 KB); TILE = 0: every tap from global memory (any step).
 *   svgf_passthrough_kernel            iterations == 0
 * Every wave reads 64 contiguous float4 of one tile row per tap, so each 16-lane group of a ds_read_b128 covers 16 distinct
 * 16-byte slots of the 256-byte bank row whatever the row pitch: no bank conflicts at 68 or 72 pixels per row.
 *
 * By default the prepare pass and iteration 0 read the tile and iteration 1 global memory (the fastest of each);
 * MORT_SVGF_TAPS=lds stages iteration 1 too, =global stages nothing.  The arithmetic is the same body (dev_svgf.h) wherever a
 * tap comes from, so the bits are too.  The host form (mort_hip_svgf_host) runs that body on host threads and makes no
 * HIP runtime call.  Nothing here touches the render's RNG states, tile-cost cache or counters.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mort_hip.h"
#include "dev_svgf.h"
#include "mort_ctx.h"
#include "mort_internal.h"
#include "stage_common.h"

#pragma clang fp contract(off)

/* ====================================================================== device */

template <bool HAVE_VAR, bool TILE>
__global__ void __launch_bounds__(STAGE_BX * STAGE_BY) svgf_prep_kernel(const SvgfArgs a) {
    const int x = blockIdx.x * STAGE_BX + threadIdx.x, y = blockIdx.y * STAGE_BY + threadIdx.y;
    if constexpr (TILE) {
        constexpr int TW = STAGE_BX + 4, TH = STAGE_BY + 4;
        __shared__ float4 t_nd[TW * TH];
        __shared__ float t_l[TW * TH];
        const int x0 = blockIdx.x * STAGE_BX - 2, y0 = blockIdx.y * STAGE_BY - 2;
        bool stage = true;
        if constexpr (HAVE_VAR) { /* the tile serves the spatial estimate only: skip it where the whole workgroup knows its variance */
            const bool unknown = x < a.width && y < a.height && !(a.V[(size_t)x + (size_t)y * (size_t)a.width] >= 0.0f);
            stage = __syncthreads_or(unknown) != 0;
        }
        for (int i = threadIdx.x + threadIdx.y * STAGE_BX; stage && i < TW * TH; i += STAGE_BX * STAGE_BY) {
            const int qx = x0 + i % TW, qy = y0 + i / TW;
            float4 g;
            g.x = 0.0f; g.y = 0.0f; g.z = 0.0f; g.w = 0.0f;
            float l = 0.0f;
            if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) { /* taps outside the image are never read */
                const SvPrepTap t = sv_prep_load(a, (size_t)qx + (size_t)qy * (size_t)a.width);
                g.x = t.nx; g.y = t.ny; g.z = t.nz; g.w = t.d;
                l = t.l;
            }
            t_nd[i] = g; t_l[i] = l;
        }
        __syncthreads();
        if (x >= a.width || y >= a.height) return;
        const SvPrepTile src = {t_nd, t_l, x0, y0, TW};
        svgf_prep_pixel<HAVE_VAR>(a, src, x, y);
    } else {
        if (x >= a.width || y >= a.height) return;
        const SvPrepGlobal src = {&a};
        svgf_prep_pixel<HAVE_VAR>(a, src, x, y);
    }
}

template <bool LAST, int TILE>
__global__ void __launch_bounds__(STAGE_BX * STAGE_BY) svgf_iter_kernel(const SvgfArgs a) {
    const int x = blockIdx.x * STAGE_BX + threadIdx.x, y = blockIdx.y * STAGE_BY + threadIdx.y;
    if constexpr (TILE > 0) { /* a.step == TILE */
        constexpr int TW = STAGE_BX + 4 * TILE, TH = STAGE_BY + 4 * TILE;
        __shared__ float4 t_e[TW * TH], t_g0[TW * TH], t_g1[TW * TH];
        const int x0 = blockIdx.x * STAGE_BX - 2 * TILE, y0 = blockIdx.y * STAGE_BY - 2 * TILE;
        for (int i = threadIdx.x + threadIdx.y * STAGE_BX; i < TW * TH; i += STAGE_BX * STAGE_BY) {
            const int qx = x0 + i % TW, qy = y0 + i / TW;
            float4 e, g, h;
            e.x = 0.0f; e.y = 0.0f; e.z = 0.0f; e.w = 0.0f;
            g = e; h = e;
            if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
                const size_t q = (size_t)qx + (size_t)qy * (size_t)a.width;
                e = a.e_in[q]; g = a.g0[q]; h = a.g1[q];
            }
            t_e[i] = e; t_g0[i] = g; t_g1[i] = h;
        }
        __syncthreads();
        if (x >= a.width || y >= a.height) return;
        const SvTile src = {t_e, t_g0, t_g1, x0, y0, TW};
        svgf_pixel<LAST>(a, src, x, y);
    } else {
        if (x >= a.width || y >= a.height) return;
        const SvGlobal src = {a.e_in, a.g0, a.g1, a.width};
        svgf_pixel<LAST>(a, src, x, y);
    }
}

__global__ void __launch_bounds__(STAGE_BX * STAGE_BY) svgf_passthrough_kernel(const SvgfArgs a) {
    const int x = blockIdx.x * STAGE_BX + threadIdx.x, y = blockIdx.y * STAGE_BY + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    svgf_passthrough(a, x, y);
}

/* ====================================================================== host */

namespace {

/* iterations and sigma_luminance tuned on scenes 1, 3, 6, 8; the rest are mort_hip_denoise_defaults' */
const mort_svgf_params kDefaults = {3, 3.0f, 0.1f, 0.05f, 3};

bool params_ok(const mort_svgf_params *p) {
    if (!p) return false;
    if (p->iterations < 0 || p->iterations > 8) return false;
    if (p->normal_log2_power < 0 || p->normal_log2_power > 16) return false;
    const float s[3] = {p->sigma_luminance, p->sigma_depth, p->sigma_albedo};
    for (float v : s) if (!(v > 0.0f && v < 1e30f)) return false;
    return true;
}

/* required inputs present, no output overlapping an input or another output */
bool buffers_ok(int W, int H, const void *accum, const void *albedo, const void *normal, const void *depth, const void *variance,
                void *accum_out, void *variance_out, void *rgba_out) {
    if (!accum || !albedo || !normal || !depth) return false;
    const size_t npx = (size_t)W * (size_t)H;
    const void *ins[5] = {accum, albedo, normal, depth, variance};
    const size_t in_b[5] = {npx * 12, npx * 12, npx * 12, npx * 4, npx * 4};
    void *outs[3] = {accum_out, variance_out, rgba_out};
    const size_t out_b[3] = {npx * 12, npx * 4, npx * 4};
    return buffers_disjoint(ins, in_b, 5, outs, out_b, 3);
}

/* the checks every form makes */
int check_call(const mort_svgf_params *p, int W, int H, const void *accum, const void *albedo, const void *normal, const void *depth,
               const void *variance, void *accum_out, void *variance_out, void *rgba_out) {
    if (!params_ok(p)) return MORT_ERR_INVALID;
    if (!stage_size_ok(W, H)) return MORT_ERR_INVALID;
    if (!buffers_ok(W, H, accum, albedo, normal, depth, variance, accum_out, variance_out, rgba_out)) return MORT_ERR_INVALID;
    return MORT_OK;
}

/* the arguments of the prepare pass (i < 0) or of iteration i; the scratch is four float4 planes: e ping-pong, g0, g1 */
SvgfArgs svgf_args(const mort_svgf_params *p, int W, int H, int i, const void *accum, const void *albedo, const void *normal,
                   const void *depth, const void *variance, float4 *scratch, void *accum_out, void *variance_out, void *rgba_out) {
    SvgfArgs a;
    std::memset(&a, 0, sizeof a);
    const size_t npx = (size_t)W * (size_t)H;
    float4 *e0 = scratch, *e1 = e0 + npx;
    a.width = W; a.height = H;
    a.step = 1 << (i < 0 ? 0 : i);
    a.npow = p->normal_log2_power;
    a.sl = p->sigma_luminance;
    a.sd1 = p->sigma_depth;
    a.sd = p->sigma_depth * (float)a.step;
    a.inv_a = 1.0f / (p->sigma_albedo * p->sigma_albedo);
    a.C = (const float *)accum; a.A = (const float *)albedo; a.N = (const float *)normal; a.D = (const float *)depth;
    a.V = (const float *)variance;
    a.g0 = e1 + npx; a.g1 = a.g0 + npx;
    if (i < 0) { a.e_out = e0; a.e_in = e0; } /* e_in: what the pass-through reads after the prepare pass */
    else { a.e_in = (i & 1) ? e1 : e0; a.e_out = (i & 1) ? e0 : e1; }
    a.accum_out = (float *)accum_out; a.variance_out = (float *)variance_out; a.rgba_out = (uchar4 *)rgba_out;
    return a;
}

struct SvHostJob { SvgfArgs a; int kind; /* 0 prepare, 1 iteration, 2 last iteration, 3 pass-through */ };
void sv_host_row(void *p, int y) {
    const SvHostJob *j = (const SvHostJob *)p;
    const SvgfArgs &a = j->a;
    const SvPrepGlobal ps = {&a};
    const SvGlobal src = {a.e_in, a.g0, a.g1, a.width};
    for (int x = 0; x < a.width; x++) {
        if (j->kind == 0) { if (a.V) svgf_prep_pixel<true>(a, ps, x, y); else svgf_prep_pixel<false>(a, ps, x, y); }
        else if (j->kind == 1) svgf_pixel<false>(a, src, x, y);
        else if (j->kind == 2) svgf_pixel<true>(a, src, x, y);
        else svgf_passthrough(a, x, y);
    }
}

/* MORT_SVGF_TAPS: the largest step whose neighbourhood is staged in LDS.  Unset: 1 -- the prepare pass and iteration 0 from
 * the tile, iteration 1 from global memory, which is what measures fastest.  "lds": 2, iteration 1 staged as
 * well; "global": 0, no tile anywhere.  The same bits either way */
int lds_steps() {
    const char *e = getenv("MORT_SVGF_TAPS");
    if (e && std::strcmp(e, "global") == 0) return 0;
    if (e && std::strcmp(e, "lds") == 0) return 2;
    return 1;
}

template <bool LAST>
void launch_iter(const SvgfArgs &a, int lds, dim3 grid, dim3 block, hipStream_t s) {
    if (lds >= 1 && a.step == 1) hipLaunchKernelGGL((svgf_iter_kernel<LAST, 1>), grid, block, 0, s, a);
    else if (lds >= 2 && a.step == 2) hipLaunchKernelGGL((svgf_iter_kernel<LAST, 2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((svgf_iter_kernel<LAST, 0>), grid, block, 0, s, a);
}

} // namespace

bool mort_svgf_params_ok(const mort_svgf_params *p) { return params_ok(p); }

extern "C" int mort_hip_svgf_defaults(mort_svgf_params *p) {
    if (!p) return MORT_ERR_INVALID;
    *p = kDefaults;
    return MORT_OK;
}

extern "C" int mort_hip_svgf_device(mort_ctx *c, const mort_svgf_params *p, int W, int H, const void *d_accum, const void *d_albedo,
                                    const void *d_normal, const void *d_depth, const void *d_variance, void *d_accum_out,
                                    void *d_variance_out, void *d_rgba_out, void *stream, double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    int st = check_call(p, W, H, d_accum, d_albedo, d_normal, d_depth, d_variance, d_accum_out, d_variance_out, d_rgba_out);
    if (st != MORT_OK) return st;
    const int lds = lds_steps();
    const int n = p->iterations;
    const dim3 grid = stage_grid(W, H), block = stage_block();
    hipStream_t s;
    if ((st = stage_begin(c, stream, (size_t)W * (size_t)H * 4 * sizeof(float4), seconds, &s)) != MORT_OK) return st;
    float4 *scratch = (float4 *)c->stage_planes.p;
    const SvgfArgs pa = svgf_args(p, W, H, -1, d_accum, d_albedo, d_normal, d_depth, d_variance, scratch, d_accum_out, d_variance_out, d_rgba_out);
    if (d_variance) {
        if (lds) hipLaunchKernelGGL((svgf_prep_kernel<true, true>), grid, block, 0, s, pa);
        else hipLaunchKernelGGL((svgf_prep_kernel<true, false>), grid, block, 0, s, pa);
    } else {
        if (lds) hipLaunchKernelGGL((svgf_prep_kernel<false, true>), grid, block, 0, s, pa);
        else hipLaunchKernelGGL((svgf_prep_kernel<false, false>), grid, block, 0, s, pa);
    }
    HIPCHK(c, hipGetLastError());
    if (n == 0) {
        hipLaunchKernelGGL(svgf_passthrough_kernel, grid, block, 0, s, pa);
        HIPCHK(c, hipGetLastError());
    }
    for (int i = 0; i < n; i++) {
        const SvgfArgs a = svgf_args(p, W, H, i, d_accum, d_albedo, d_normal, d_depth, d_variance, scratch, d_accum_out, d_variance_out, d_rgba_out);
        if (i == n - 1) launch_iter<true>(a, lds, grid, block, s);
        else launch_iter<false>(a, lds, grid, block, s);
        HIPCHK(c, hipGetLastError());
    }
    return stage_end(c, s, seconds);
}

extern "C" int mort_hip_svgf(mort_ctx *c, const mort_svgf_params *p, int W, int H, const float *accum, const float *albedo, const float *normal,
                             const float *depth, const float *variance, float *accum_out, float *variance_out, uint8_t *rgba_out,
                             double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    int st = check_call(p, W, H, accum, albedo, normal, depth, variance, accum_out, variance_out, rgba_out);
    if (st != MORT_OK) return st;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, switch_stream(c, c->stream));
    const size_t npx = (size_t)W * (size_t)H;
    StagePlane pl[8] = {{accum, nullptr, npx * 12}, {albedo, nullptr, npx * 12}, {normal, nullptr, npx * 12}, {depth, nullptr, npx * 4},
                        {variance, nullptr, npx * 4}, {nullptr, accum_out, npx * 12}, {nullptr, variance_out, npx * 4}, {nullptr, rgba_out, npx * 4}};
    if ((st = stage_upload(c, pl, 8)) != MORT_OK) return st;
    double sec = 0;
    if ((st = mort_hip_svgf_device(c, p, W, H, pl[0].dev, pl[1].dev, pl[2].dev, pl[3].dev, pl[4].dev, pl[5].dev, pl[6].dev, pl[7].dev, c->stream,
                                   &sec)) != MORT_OK)
        return st;
    if (seconds) *seconds = sec;
    return stage_download(c, pl, 8);
}

extern "C" int mort_hip_svgf_host(const mort_svgf_params *p, int W, int H, int nthreads, const float *accum, const float *albedo,
                                  const float *normal, const float *depth, const float *variance, float *accum_out, float *variance_out,
                                  uint8_t *rgba_out, double *seconds) {
    const int st = check_call(p, W, H, accum, albedo, normal, depth, variance, accum_out, variance_out, rgba_out);
    if (st != MORT_OK) return st;
    const size_t npx = (size_t)W * (size_t)H;
    std::vector<float4> scratch(npx * 4);
    const int n = p->iterations;
    const double t0 = now_s();
    for (int i = -1; i < (n > 0 ? n : 1); i++) {
        SvHostJob job;
        job.a = svgf_args(p, W, H, n == 0 ? -1 : i, accum, albedo, normal, depth, variance, scratch.data(), accum_out, variance_out, rgba_out);
        job.kind = i < 0 ? 0 : (n == 0 ? 3 : (i == n - 1 ? 2 : 1));
        run_rows(H, nthreads, sv_host_row, &job);
    }
    if (seconds) *seconds = now_s() - t0;
    return MORT_OK;
}
