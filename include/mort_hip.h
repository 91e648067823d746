/*
 * mort_hip.h -- C ABI of libmort_hip.so, the MI355X (gfx950) render path.
 *
 * The reference has no plugin / FFI interface: host and device share one
 * translation unit and the boundary is a kernel launch with by-value structs.
 * The entry points below are what a binding for that boundary has to replace:
 *
 *   mort_hip_upload_world   <- world::toDevice()            world.cuh:98-102
 *                              (16x cudaMemcpyToSymbol:     objects.cuh:848-856,
 *                               materials.cuh:264-270, textures.cuh:320-325,
 *                               image upload textures.cuh:89-127)
 *   mort_hip_rng_seed       <- setup_rng<<<>>>              rng.cuh:8-15, mort.cu:706-709
 *   mort_hip_rng_load/store <- (dev_states array itself)    mort.cu:706-708
 *   mort_hip_render[_device]<- renderKernel<<<>>> + the four per-bounce scratch
 *                              allocations                  mort.cu:44-47,106,712-725
 *   mort_hip_init/shutdown  <- implicit device 0 context    textures.cuh:91
 *
 * Conventions: plain C, no C++ types or exceptions cross the boundary.  The
 * caller owns every host buffer; the library owns all device memory behind
 * the opaque mort_ctx (except buffers passed to mort_hip_render_device).
 * Calls are blocking unless stated; one context per process per device; a
 * context is not re-entrant.  Every function returns MORT_OK (0) or a
 * negative mort_status; the reference's convention is print-and-exit
 * (HANDLE_ERROR, include/book.h:21-30), which the `mort` CLI reproduces on
 * top of these codes.
 */
#ifndef MORT_HIP_H
#define MORT_HIP_H

#include "mort_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mort_ctx mort_ctx;

typedef enum mort_status {
    MORT_OK = 0,
    MORT_ERR_INVALID = -1,      /* NULL / out-of-range argument */
    MORT_ERR_NO_DEVICE = -2,    /* no HIP device, or not gfx950 */
    MORT_ERR_HIP = -3,          /* a HIP runtime call failed (see mort_hip_last_error) */
    MORT_ERR_NO_WORLD = -4,     /* render before upload_world */
    MORT_ERR_NO_RNG = -5,       /* render before rng_seed / rng_load */
    MORT_ERR_UNSUPPORTED = -6,  /* scene graph outside what the kernels flatten */
    MORT_ERR_CAPACITY = -7,     /* bounce_limit > MORT_MAX_BOUNCE_LIMIT, nesting too deep, ... */
    MORT_ERR_NOMEM = -8
} mort_status;

/* render modes */
#define MORT_MODE_MEGA 0 /* one lane per pixel, whole path on chip */
#define MORT_MODE_THROUGHPUT 2 /* NOT a drop-in, NOT bit-compatible with the reference: the reference keys one cuRAND stream per pixel (mort.cu:23-24), which
                                 * makes a pixel's samples one serial chain; this mode keys one stream per (pixel, stratum row) -- subsequence x + (y*sqrt_spp + s_j)*W of
                                 * the same seed -- so a pixel's sqrt_spp rows run as independent work items, and a resolve kernel sums them in order.  Same estimator,
                                 * same per-sample arithmetic, deterministic and partition-invariant, but different random numbers: images agree with MORT_MODE_MEGA only
                                 * statistically.  Needs mort_hip_rng_seed (the seed is reused; rng_load'ed states are not); worlds the two LDS state-machine
                                 * kernels take (scenes 1, 10; the final scenes 8, 9), else MORT_ERR_UNSUPPORTED; the per-pixel states of the other modes are left untouched.  bench.py reports it only
                                 * as a separately labelled line */
#define MORT_MODE_WAVE 1 /* wavefront (queued) pipeline: every world the megakernels stage in LDS (all ten built-in scenes), else MORT_ERR_UNSUPPORTED; blocking */

/* Which rows of the image this context renders: rows are grouped into blocks
 * of `rows_per_block` and this context owns blocks rank, rank+nranks, ...
 * (image-space partition across GPUs).  {0,1,8} = whole image. */
typedef struct mort_partition {
    int rank;
    int nranks;
    int rows_per_block; /* multiple of 8 */
} mort_partition;

typedef struct mort_stats {
    double seconds;          /* device time of the render kernel(s), HIP events */
    uint64_t segments;       /* world::hit calls == path segments traced */
    uint64_t pixels;         /* pixels rendered by this context */
    uint64_t eff_samples;    /* pixels * floor(sqrt(spp))^2 */
    uint64_t rng_draws;      /* curand_uniform calls */
    uint64_t algorithmic_hbm_bytes; /* 100 B/pixel (+12 with accum) */
    int scene_in_lds;        /* 1 if the kernel staged the scene in LDS */
    int local_rows;          /* rows owned under the partition */
    int kernel_vgprs, kernel_lds_bytes; /* launch facts, for reports */
    uint64_t reference_walks; /* BVH megakernel: segments re-traced with the reference's own walk */
    char kernel_name[64];    /* dominant kernel of this render as rocprofv3 names it (template arguments included) */
    double gather_seconds;   /* mort_hip_render_gather: device time of the frame gather (RCCL + de-interleave + copy out) */
} mort_stats;

const char *mort_hip_strerror(int status);
/* Text of the last HIP error seen by this context ("" if none). */
const char *mort_hip_last_error(const mort_ctx *ctx);

/* device = HIP ordinal (one process per GPU uses LOCAL_RANK). */
int mort_hip_init(int device, mort_ctx **out);
void mort_hip_shutdown(mort_ctx *ctx);

/* Copies and re-lays-out the world for the kernels; the caller keeps ownership
 * of every host array (including image texels) and may free them afterwards. */
int mort_hip_upload_world(mort_ctx *ctx, const mort_world *world);

int mort_hip_set_partition(mort_ctx *ctx, const mort_partition *part);

/* states[x + y*W] = curand_init(seed, subsequence = x + y*W, offset = 0) for
 * every pixel this context owns (unlike rng.cuh:8-15, bounds-guarded). */
int mort_hip_rng_seed(mort_ctx *ctx, uint64_t seed, int width, int height);
/* Full-image arrays of W*H 48-byte curandStateXORWOW records, row-major from
 * the bottom row (the reference's layout); only owned rows are read/written. */
int mort_hip_rng_load(mort_ctx *ctx, const mort_rng_state *states, int width, int height);
int mort_hip_rng_store(mort_ctx *ctx, mort_rng_state *states, int width, int height);

/* Renders the owned rows into full-size host buffers: rgba_out W*H*4 bytes
 * (uchar4, row 0 = bottom row, as the reference's GL buffer), accum_out W*H*3
 * floats (linear pixel mean before gamma) or NULL, segments_px_out W*H
 * uint32 or NULL.  Rows not owned are left untouched. */
int mort_hip_render(mort_ctx *ctx, const mort_camera *cam, int mode, uint8_t *rgba_out, float *accum_out,
                    uint32_t *segments_px_out, mort_stats *stats);

/* Same render into caller-provided DEVICE buffers holding only the owned rows,
 * packed (local_rows * W pixels): d_rgba local_rows*W*4 bytes, d_accum
 * local_rows*W*3 floats or NULL.  Launched on `stream` (a hipStream_t, NULL =
 * the context's stream); asynchronous when stats is NULL, otherwise waits and
 * fills stats.  This is the entry bench.py and the multi-GPU gather use. */
int mort_hip_render_device(mort_ctx *ctx, const mort_camera *cam, int mode, void *d_rgba, void *d_accum,
                           void *stream, mort_stats *stats);

/* ---- `mort --mode host` (BASELINE config 1; the CPU figure timed beside the GPU): the render path as a straight host
 * loop of the SAME kernel body the GPU runs (camera.cuh:86-242 and everything below it), on `nthreads` host threads.
 * An explicit mode, never a fallback; needs no GPU and makes no HIP runtime call.  `states`: W*H records, read and
 * written in place (full image, row 0 = bottom row).  flags: MORT_HOST_TREE = walk this build's unified tree where the
 * world has one (what one GPU lane does) instead of the reference's scan over every primitive. ---- */
#define MORT_HOST_TREE 1
int mort_hip_rng_seed_host(uint64_t seed, int width, int height, mort_rng_state *states);
int mort_hip_render_host(const mort_world *world, const mort_camera *cam, mort_rng_state *states, int nthreads, int flags,
                         uint8_t *rgba_out, float *accum_out, uint32_t *segments_px_out, mort_stats *stats);

/* ---- multi-GPU: one process (one context) per GPU, image rows partitioned with mort_hip_set_partition, ONE exchange step:
 * the packed uchar4 rows of every rank are gathered to rank 0 over RCCL and de-interleaved there (the reference is
 * single-GPU).  Rank 0 obtains an id (mort_hip_comm_id) and hands its MORT_COMM_ID_BYTES bytes to the other ranks by any
 * means (the CLI uses pipes to the ranks it forked); every rank then calls mort_hip_comm_init (collective) after
 * mort_hip_set_partition(rank, nranks, rows_per_block).  mort_hip_render_gather = render + gather, collective, blocking;
 * rank 0 receives the full W*H*4 frame in rgba_out (other ranks may pass NULL).  With nranks == 1 no communicator is needed. */
#define MORT_COMM_ID_BYTES 128
int mort_hip_comm_id(void *id);
int mort_hip_comm_init(mort_ctx *ctx, const void *id, int rank, int nranks);
void mort_hip_comm_destroy(mort_ctx *ctx);
int mort_hip_render_gather(mort_ctx *ctx, const mort_camera *cam, int mode, uint8_t *rgba_out, mort_stats *stats);
/* One-rank rehearsal of the RCCL path (library load, communicator, grouped send / recv to self, de-interleave): MORT_OK when the bytes come back. */
int mort_hip_comm_selftest(mort_ctx *ctx);

/* ---- roofline calibration (measurement only; bench.py prints the results beside the render kernels' counters).
 * mort_hip_calib_valu: shader cycles one SIMD needs per wave64 VALU instruction with exactly `waves_per_simd` (1..8) waves
 * resident on every SIMD; kind 0 = independent v_fma_f32, 1 = one dependent v_fma_f32 chain, 2 = independent v_fma_f64,
 * 3 = three v_fma_f32 per scalar instruction, 4 = independent v_pk_fma_f32 (two fma per lane and instruction).  mort_hip_calib_hbm_copy: GB/s (read + write) of a float4 copy of `bytes`
 * per buffer (use > 256 MB, the Infinity Cache), best of `reps`. ---- */
typedef struct mort_calib_valu {
    int waves_per_simd, kind;
    double seconds;                  /* HIP-event time of the launch */
    double cycles_per_wave;          /* s_memtime ticks around the loop, median over waves */
    double clock_ghz;                /* s_memtime ticks per s_memrealtime tick (100 MHz), median over waves */
    double valu_per_wave;            /* VALU instructions each wave issued */
    int simds_seen;                  /* distinct (XCC, SE, SH, CU, SIMD) the waves reported (HW_REG_HW_ID / HW_REG_XCC_ID) */
    double resident_waves_per_simd;  /* waves of this launch that really overlapped on a SIMD (median over SIMDs) */
    double cycles_per_valu_per_wave; /* what ONE wave sustains: cycles_per_wave / valu_per_wave */
    double cycles_per_valu_per_simd; /* what a SIMD sustains: (first start .. last end of its waves) x clock / instructions issued on it, median over SIMDs */
} mort_calib_valu;
int mort_hip_calib_valu(mort_ctx *ctx, int waves_per_simd, int kind, mort_calib_valu *out);
int mort_hip_calib_hbm_copy(mort_ctx *ctx, size_t bytes, int reps, double *gbs_out);

/* ---- first-hit feature buffers and an edge-aware a-trous denoiser (Dammertz et al., HPG 2010).  NOT parity: an extra on
 * top of the render for a viewable image at low sample counts.  None of these calls draws a random number or touches what the render keeps
 * across frames (RNG states, tile-cost cache).  All buffers are full-image f32, row 0 = bottom row.  `seconds` may be NULL; when given it
 * receives the HIP-event device time of the kernels (host forms: wall time of the loop).
 *
 * Features: one ray per pixel from the lens centre through the pixel centre (time 0.5), closest solid hit (t_min = 0.001), then the
 * constant media in scan order entered before it (no random distance).  A ray that starts inside a medium (boundary entry below t_min)
 * does not enter it: that medium is passed over, so a camera inside smoke or fog sees the solids behind it.  albedo W*H*3: lambertian / isotropic = texture at the hit,
 * metal = its colour, dielectric / diffuse_light = 1; normal W*H*3: world space, front-face oriented (medium: -unit(dir)); depth W*H:
 * t * |dir|.  A miss: albedo = camera background, normal = 0, depth = 0 (the "no hit" sentinel).
 *
 * Denoise: C' = remodulate(a-trous^n(C / max(A, 1e-3))) with the weights of DESIGN.md 4.9, then the render's NaN guard and gamma tail
 * for rgba (uchar4 W*H).  iterations == 0 returns C unchanged and the render's own rgba.  accum_out (W*H*3) or rgba_out may be NULL;
 * outputs must not alias inputs.  Whole image, whatever the context's partition. ---- */
typedef struct mort_denoise_params {
    int iterations;          /* 0..8; iteration i filters at step 2^i */
    float sigma_color;       /* demodulated colour; halves every iteration */
    float sigma_depth;       /* relative depth difference per step */
    float sigma_albedo;      /* albedo difference */
    int normal_log2_power;   /* normal weight max(0, Np.Nq)^(2^k), k squarings; 0..16 */
} mort_denoise_params;
int mort_hip_denoise_defaults(mort_denoise_params *params);
/* full-size host buffers; under a partition only the owned rows are written.  Needs an uploaded world, no RNG. */
int mort_hip_render_features(mort_ctx *ctx, const mort_camera *cam, float *albedo_out, float *normal_out, float *depth_out, double *seconds);
/* packed owned rows in DEVICE buffers (local_rows * W pixels), on `stream` (NULL = the context's); asynchronous when seconds is NULL */
int mort_hip_render_features_device(mort_ctx *ctx, const mort_camera *cam, void *d_albedo, void *d_normal, void *d_depth, void *stream,
                                    double *seconds);
int mort_hip_denoise(mort_ctx *ctx, const mort_denoise_params *params, int width, int height, const float *accum, const float *albedo,
                     const float *normal, const float *depth, float *accum_out, uint8_t *rgba_out, double *seconds);
/* the same on DEVICE buffers of the whole image, on `stream` (NULL = the context's); asynchronous when seconds is NULL */
int mort_hip_denoise_device(mort_ctx *ctx, const mort_denoise_params *params, int width, int height, const void *d_accum, const void *d_albedo,
                            const void *d_normal, const void *d_depth, void *d_accum_out, void *d_rgba_out, void *stream, double *seconds);
/* host loops of the same bodies: no GPU, no HIP runtime call.  flags: MORT_HOST_TREE as for mort_hip_render_host */
int mort_hip_render_features_host(const mort_world *world, const mort_camera *cam, int nthreads, int flags, float *albedo_out, float *normal_out,
                                  float *depth_out, double *seconds);
int mort_hip_denoise_host(const mort_denoise_params *params, int width, int height, int nthreads, const float *accum, const float *albedo,
                          const float *normal, const float *depth, float *accum_out, uint8_t *rgba_out, double *seconds);

/* ---- temporal accumulation across frames with camera reprojection (the reprojection / accumulation half of SVGF, Schied et al.,
 * HPG 2017).  NOT parity.  Between the render and the denoiser: the frame's accumulators (W*H*3) and its features
 * (normal W*H*3, depth W*H from mort_hip_render_features*) are blended with a caller-owned history of the frames before, seen from
 * prev_cam (NULL = no history: a reset).  The frame weighs cam->sqrt_spp^2 effective samples.  A still camera (centre, viewport and
 * size bit-identical to prev_cam's) reads each pixel's own history, misses included; a moved one reprojects the hit point into the
 * previous frame and gathers the accepted bilinear taps (hit, depth within depth_tolerance, normal dot >= normal_min); a miss under
 * motion starts over.  History: MORT_TEMPORAL_HISTORY_FLOATS floats per pixel as three float4 planes (16-byte aligned) of W*H,
 * plane k at k*W*H*4 floats, row 0 = bottom: (mu.rgb, n), (mean L, mean L^2, frames, depth), (normal, 0).  hist_in and hist_out
 * must not alias.  Outputs: accum_out = the accumulated colour (what mort_hip_denoise* takes as accum), rgba_out = its gamma tail,
 * variance_out (W*H) = the estimated variance of the accumulated luminance mean, -1 with fewer than 2 frames.  accum_out,
 * variance_out and rgba_out may be NULL; outputs must not alias inputs.  Whole image, whatever the context's partition.  None of
 * these calls draws a random number or touches what the render keeps across frames. ---- */
#define MORT_TEMPORAL_HISTORY_FLOATS 12
typedef struct mort_temporal_params {
    int max_samples;         /* cap on the accumulated effective samples, still camera; 0 = unbounded */
    int motion_max_samples;  /* the same after a reprojection; 0 = unbounded */
    float depth_tolerance;   /* a history tap counts if |D_q - |X - c'|| <= depth_tolerance * |X - c'|; 0..1 */
    float normal_min;        /* ... and N_p . N_q >= normal_min; -1..1 */
} mort_temporal_params;
int mort_hip_temporal_defaults(mort_temporal_params *params);
/* host buffers; the kernel's HIP-event time in *seconds */
int mort_hip_temporal(mort_ctx *ctx, const mort_temporal_params *params, const mort_camera *prev_cam, const mort_camera *cam, int width,
                      int height, const float *accum, const float *normal, const float *depth, const float *hist_in, float *hist_out,
                      float *accum_out, float *variance_out, uint8_t *rgba_out, double *seconds);
/* the same on DEVICE buffers, on `stream` (NULL = the context's); asynchronous when seconds is NULL */
int mort_hip_temporal_device(mort_ctx *ctx, const mort_temporal_params *params, const mort_camera *prev_cam, const mort_camera *cam,
                             int width, int height, const void *d_accum, const void *d_normal, const void *d_depth, const void *d_hist_in,
                             void *d_hist_out, void *d_accum_out, void *d_variance_out, void *d_rgba_out, void *stream, double *seconds);
/* host loop of the same body: no GPU, no HIP runtime call */
int mort_hip_temporal_host(const mort_temporal_params *params, const mort_camera *prev_cam, const mort_camera *cam, int width, int height,
                           int nthreads, const float *accum, const float *normal, const float *depth, const float *hist_in, float *hist_out,
                           float *accum_out, float *variance_out, uint8_t *rgba_out, double *seconds);

/* ---- the SVGF filter stage: a variance-guided a-trous filter over the accumulated colour (Schied et al., HPG 2017).
 * NOT parity.  After the temporal step (or on a single frame): accum (W*H*3) and the features (albedo, normal W*H*3, depth W*H) as
 * for mort_hip_denoise*, plus variance (W*H) = what mort_hip_temporal* writes as variance_out, the estimated variance of the
 * accumulated luminance mean.  A negative value, or variance == NULL, means unknown: that pixel's variance is then estimated from
 * the luminance of its 5x5 neighbourhood.  The filter works on E = C / max(A, 1e-3) and carries the variance of E's luminance with
 * it; iteration i at step 2^i stops at luminance differences of sigma_luminance standard deviations (the 3x3 Gaussian of the
 * variance), at depth, normal and albedo edges as the denoiser does, and never mixes hits with misses.  Outputs: accum_out (W*H*3),
 * rgba_out (uchar4 W*H: the render's NaN guard and gamma tail) and variance_out (W*H: the filtered variance, in the units of the
 * input); each may be NULL, none may alias an input or another output.  iterations == 0 returns accum unchanged, the render's own
 * rgba and the prepared variance.  Whole image, whatever the context's partition.  None of these calls draws a random number or
 * touches what the render keeps across frames. ---- */
typedef struct mort_svgf_params {
    int iterations;          /* 0..8; iteration i filters at step 2^i */
    float sigma_luminance;   /* luminance difference in standard deviations of the (prefiltered) variance */
    float sigma_depth;       /* relative depth difference per step */
    float sigma_albedo;      /* albedo difference */
    int normal_log2_power;   /* normal weight max(0, Np.Nq)^(2^k), k squarings; 0..16 */
} mort_svgf_params;
int mort_hip_svgf_defaults(mort_svgf_params *params);
/* host buffers; the kernels' HIP-event time in *seconds */
int mort_hip_svgf(mort_ctx *ctx, const mort_svgf_params *params, int width, int height, const float *accum, const float *albedo,
                  const float *normal, const float *depth, const float *variance, float *accum_out, float *variance_out, uint8_t *rgba_out,
                  double *seconds);
/* the same on DEVICE buffers of the whole image, on `stream` (NULL = the context's); asynchronous when seconds is NULL */
int mort_hip_svgf_device(mort_ctx *ctx, const mort_svgf_params *params, int width, int height, const void *d_accum, const void *d_albedo,
                         const void *d_normal, const void *d_depth, const void *d_variance, void *d_accum_out, void *d_variance_out,
                         void *d_rgba_out, void *stream, double *seconds);
/* host loop of the same bodies: no GPU, no HIP runtime call */
int mort_hip_svgf_host(const mort_svgf_params *params, int width, int height, int nthreads, const float *accum, const float *albedo,
                       const float *normal, const float *depth, const float *variance, float *accum_out, float *variance_out,
                       uint8_t *rgba_out, double *seconds);

/* ---- the view: a frame's whole chain kept on the device across frames.  NOT parity beyond its render.  A view
 * belongs to a context and owns what the chain keeps between frames: the render's rgba and accumulators, the feature buffers, the
 * ping-ponged temporal history with the previous camera, the accumulated and filtered colour, the variance.  One frame is
 *   mort_hip_render_device -> mort_hip_render_features_device -> [mort_hip_temporal_device] -> [mort_hip_denoise_device |
 *   mort_hip_svgf_device] -> uchar4
 * on ONE stream with at most one host wait, and equals bit for bit what those calls give when chained by hand: the filter takes the
 * accumulated colour (the raw accumulators without `temporal`), SVGF also the temporal variance (none without `temporal`), and the
 * uchar4 of the last stage that ran is the frame.  Pixel RNG states continue from frame to frame exactly as under plain renders.
 *
 * Still camera: when the camera fields the feature pass reads (image size, background, centre, viewport) are bit-identical to the
 * previous frame's and no world has been uploaded since, the pass is skipped and the previous buffers are kept (features_reused).
 * mort_hip_upload_world makes the next frame recompute the features and start without history, as mort_hip_view_reset does for
 * the history alone.  Several views may live on one context, of any sizes and parameters; their histories are independent and
 * they share the context's stage scratch.  A view needs the whole-image partition (else MORT_ERR_UNSUPPORTED), a camera of its
 * own width and height (else MORT_ERR_INVALID), and an uploaded world and seeded RNG states as the render does.
 * mort_hip_shutdown frees the views still alive on its context; destroying a view after that is an error of the caller.
 * A context and its views are not re-entrant. ---- */
typedef struct mort_view mort_view;
#define MORT_VIEW_FILTER_NONE 0
#define MORT_VIEW_FILTER_DENOISE 1
#define MORT_VIEW_FILTER_SVGF 2
typedef struct mort_view_params {
    int width, height;
    int temporal;                 /* 0 / 1 */
    int filter;                   /* MORT_VIEW_FILTER_* */
    mort_temporal_params tp;      /* read when temporal */
    mort_denoise_params dp;       /* read when filter == MORT_VIEW_FILTER_DENOISE */
    mort_svgf_params sp;          /* read when filter == MORT_VIEW_FILTER_SVGF */
} mort_view_params;
typedef struct mort_view_stats {
    mort_stats render;            /* as mort_hip_render_device fills it */
    double features_seconds, temporal_seconds, filter_seconds; /* HIP events of the view; 0 for a stage that did not run */
    double device_seconds;        /* first to last event of the frame: from where render.seconds starts to the end of the last stage */
    int frame;                    /* frames before this one since the last reset (0 = the first) */
    int features_reused;          /* 1: still camera, the previous frame's features were kept */
    int history_reset;            /* 1: this frame started without history (frame == 0) */
} mort_view_stats;
/* what mort_hip_view_read copies out: floats per pixel in brackets, row 0 = bottom row */
#define MORT_VIEW_RAW_ACCUM 0 /* [3] the render's accumulators */
#define MORT_VIEW_ACCUM 1     /* [3] the accumulated colour; needs temporal */
#define MORT_VIEW_FILTERED 2  /* [3] the filtered colour; needs a filter */
#define MORT_VIEW_VARIANCE 3  /* [1] the temporal step's variance; needs temporal */
#define MORT_VIEW_ALBEDO 4    /* [3] */
#define MORT_VIEW_NORMAL 5    /* [3] */
#define MORT_VIEW_DEPTH 6     /* [1] */
#define MORT_VIEW_HISTORY 7   /* [MORT_TEMPORAL_HISTORY_FLOATS] the history the last frame wrote, three float4 planes; needs temporal */
#define MORT_VIEW_ENDS 8      /* [1, uint32] the last cached frame's paths per pixel that ended in the volume; needs a cache attached */
#define MORT_VIEW_LIT 9       /* [1, uint32] of those, the paths whose shadow segment saw light; needs a DIRECT cache attached (4.23) */
/* the three stages' own defaults; temporal 1, filter SVGF; width = height = 0 */
int mort_hip_view_defaults(mort_view_params *p);
/* MORT_OK or MORT_ERR_INVALID: sizes > 0, temporal 0 / 1, a known filter, and the stages' own checks of the parameters in use
 * (what mort_hip_view_create applies; needs no GPU) */
int mort_hip_view_check_params(const mort_view_params *p);
int mort_hip_view_create(mort_ctx *ctx, const mort_view_params *p, mort_view **out);
/* waits for the view's work in flight, then frees its buffers */
void mort_hip_view_destroy(mort_view *v);
/* forget the history: the next frame starts over (frame 0).  RNG states and feature buffers are not touched */
int mort_hip_view_reset(mort_view *v);
/* one frame into a host buffer (W*H*4 bytes, uchar4, row 0 = bottom row): one host wait, at the end.  `mode` as for
 * mort_hip_render_device; stats may be NULL */
int mort_hip_view_frame(mort_view *v, const mort_camera *cam, int mode, uint8_t *rgba_out, mort_view_stats *stats);
/* the same into a DEVICE buffer on `stream` (a hipStream_t, NULL = the context's).  The view remembers the stream of its last
 * frame and waits for it in its next call (a frame on another stream, mort_hip_view_read, mort_hip_view_destroy): a caller's
 * stream must outlive that call.  stats == NULL: everything is enqueued and the
 * call returns without waiting (MORT_MODE_WAVE stays blocking); otherwise one wait at the end, then the statistics */
int mort_hip_view_frame_device(mort_view *v, const mort_camera *cam, int mode, void *d_rgba_out, void *stream, mort_view_stats *stats);
/* copies one buffer of the last frame (MORT_VIEW_*) to the host, after waiting for that frame; MORT_ERR_INVALID for a buffer the
 * view's configuration does not produce, or before the first frame */
int mort_hip_view_read(mort_view *v, int what, void *host_out);

/* ---- ray queries: closest hit and occlusion for batches of the caller's own rays.  The render's own traversal
 * (world::hit over the flattened items, the unified-tree walk with its scan for the rays it does not decide, the transform chains,
 * the media, the hit record) behind an entry point: picking, line of sight, shadow rays and probes agree with the renderer bit for bit.
 *
 * A closest-hit query is the reference's world::hit(ray, interval(0.001, t_max), rec).  t_min is the render's 0.001 -- the only
 * value world::hit is ever given, built into the box tests -- and NOT a parameter.  t_max is per ray and may be +inf; a root equal to
 * t_max is accepted (both primitive tests accept it).  !(t_max > 0.001f), NaN included, is a miss and nothing is traced.
 * Zero-length, non-finite and axis-parallel directions and origins anywhere are legal: the answer is world::hit's.
 *
 * states == NULL: every constant medium is passed over, as if its `skip` were set, and no random number is drawn.
 * states != NULL: one 48-byte XORWOW stream per ray; media are evaluated exactly as world::hit does, drawing from that ray's
 * stream, which is advanced in place (only d and v[] are written; a ray that draws nothing leaves its stream's bits as they were).
 *
 * The record: a miss is all zero.  mat_type / mat_idx are the hit's material reference as the world was compiled: a tag outside
 * MORT_MAT_LAMBERTIAN .. MORT_MAT_ISOTROPIC is reported as (0x7fff, 0), whatever its index.  A sphere's (u, v) are sphere_uv of its outward normal; a medium hit has normal (1, 0, 0),
 * MORT_HIT_FRONT_FACE and u = v = 0 (the reference leaves u, v indeterminate there).
 * Occlusion: out[i] = 1 iff a solid is hit in [0.001, t_max]; media never occlude and nothing is drawn: the MORT_HIT_HIT flag of
 * the closest-hit query with states == NULL.
 *
 * Forms as for the stages: the host-buffer form is blocking and stages its data through the context; the _device form takes DEVICE
 * buffers (16-byte aligned), runs on `stream` (NULL = the context's) and is asynchronous when seconds is NULL; the _host form is
 * the same per-ray body on `nthreads` host threads and makes no HIP call (flags: MORT_HOST_TREE as for
 * mort_hip_render_features_host).  `seconds`: HIP-event time of the kernel (host form: wall time of the loop), may be NULL.
 * n == 0 is MORT_OK and launches nothing.  Outputs must not overlap inputs.  Queries need an uploaded world (else
 * MORT_ERR_NO_WORLD) but no seeded pixel RNG, ignore the partition, and touch nothing the render keeps across frames (pixel
 * states, tile-cost cache, counters). ---- */
typedef struct mort_ray { float origin[3], dir[3], time, t_max; } mort_ray; /* 32 B; the first seven floats are the oracle's ray7 */
typedef struct mort_hit { float p[3], normal[3], t, u, v; int32_t mat_type, mat_idx; uint32_t flags; } mort_hit; /* 48 B */
#define MORT_HIT_HIT 1u
#define MORT_HIT_FRONT_FACE 2u
#define MORT_HIT_MEDIUM 4u
MORT_SA(sizeof(mort_ray) == 32 && sizeof(mort_hit) == 48, "ray query layout");
int mort_hip_query_closest(mort_ctx *ctx, size_t n, const mort_ray *rays, mort_rng_state *states, mort_hit *out, double *seconds);
int mort_hip_query_closest_device(mort_ctx *ctx, size_t n, const void *d_rays, void *d_states, void *d_out, void *stream, double *seconds);
int mort_hip_query_closest_host(const mort_world *world, size_t n, const mort_ray *rays, mort_rng_state *states, int nthreads, int flags,
                                mort_hit *out, double *seconds);
int mort_hip_query_occluded(mort_ctx *ctx, size_t n, const mort_ray *rays, uint8_t *out, double *seconds);
int mort_hip_query_occluded_device(mort_ctx *ctx, size_t n, const void *d_rays, void *d_out, void *stream, double *seconds);
int mort_hip_query_occluded_host(const mort_world *world, size_t n, const mort_ray *rays, int nthreads, int flags, uint8_t *out,
                                 double *seconds);

/* ---- radiance queries: the path-traced colour arriving along batches of the caller's own rays.  The render's
 * path above the traversal -- ray_color's bounce loop, the material scatter, the mixture pdf towards the light, the media, the
 * unwind -- behind an entry point: light and reflection probes, panorama / fisheye / stereo cameras and lightmap texels get the
 * renderer's own answer, bit for bit the reference's ray_color.
 *
 * The ray is the ray queries' mort_ray.  Its `time` is ray_color's r.time(): every scattered ray carries it.  Its t_max is
 * IGNORED: ray_color always searches [0.001, inf).  Zero-length, non-finite and axis-parallel directions and origins anywhere are
 * legal: the answer is ray_color's.
 *
 * states is required: one 48-byte XORWOW stream per ray, advanced in place (only d and v[] are written; a ray that draws nothing
 * leaves its stream's bits as they were).
 *
 * rgb_out is 3 n floats: rgb_out[i] = ((0 + c_1) + c_2) + ... + c_samples in fp32, c_k the k-th ray_color of ray i, the paths
 * drawing from stream i one after the other (Camera::render's pixel_color = pixel_color + ray_color(...)).  No scale, no NaN guard,
 * no gamma: a NaN stays a NaN and the caller scales.  bounce_limit == 0 returns 0 and draws nothing; a path that reaches the
 * limit contributes 0, as in the reference.
 *
 * Forms, `seconds`, n == 0, alignment and overlap as for the ray queries; the streams count as an output.  NULL params, rays,
 * states or rgb_out and samples < 1 are MORT_ERR_INVALID; bounce_limit and the light object are checked as mort_hip_render
 * checks the camera's (MORT_ERR_CAPACITY; MORT_ERR_INVALID / MORT_ERR_UNSUPPORTED).  The calls need an uploaded world (else
 * MORT_ERR_NO_WORLD) but no seeded pixel RNG, ignore the partition, and touch nothing the render keeps across frames. ---- */
typedef struct mort_radiance_params {
    int bounce_limit;                  /* 0..MORT_MAX_BOUNCE_LIMIT; ray_color's cam->bounce_limit */
    int samples;                       /* >= 1: paths per ray, drawn one after the other from the ray's stream */
    float background[3];               /* what a miss returns (cam->background) */
    int light_obj_type, light_obj_idx; /* -1 = no light sampling; else as mort_camera's */
} mort_radiance_params;
MORT_SA(sizeof(mort_radiance_params) == 28, "radiance query layout");
int mort_hip_radiance_params_from_camera(const mort_camera *cam, mort_radiance_params *out); /* samples = 1 */
int mort_hip_query_radiance(mort_ctx *ctx, const mort_radiance_params *params, size_t n, const mort_ray *rays, mort_rng_state *states,
                            float *rgb_out, double *seconds);
int mort_hip_query_radiance_device(mort_ctx *ctx, const mort_radiance_params *params, size_t n, const void *d_rays, void *d_states,
                                   void *d_rgb_out, void *stream, double *seconds);
int mort_hip_query_radiance_host(const mort_world *world, const mort_radiance_params *params, size_t n, const mort_ray *rays,
                                 mort_rng_state *states, int nthreads, int flags, float *rgb_out, double *seconds);

/* ---- light probes: path-traced radiance projected onto SH9 on the device.  For each probe position the nine
 * real spherical-harmonics coefficients (bands 0..2) per colour channel of the incoming radiance: one fused kernel builds the
 * rays in registers, runs the radiance queries' own path body and reduces in the wave, so 108 bytes per probe leave the device.
 * The summation order below is part of the contract: GPU kernel, host loop and any restatement of it agree to the bit.
 *
 * For probe p and direction j < D (D = params->directions), everything fp32 and nothing contracted:
 *   ray      origin position_p, direction dirs[j] exactly as given (NOT normalised), time time_p; searched as a radiance query
 *            searches, [0.001, inf).
 *   stream   states[p D + j], advanced in place (only d and v[] are written; a direction that draws nothing keeps its bits).
 *   s_j      ((0 + c_1) + c_2) + ... + c_samples, the radiance query's sum of rp.samples paths.
 *   g_j      s_j with every component c != c replaced by 0 (the render's NaN guard).
 *   Y_k      with (x, y, z) = dirs[j], c0 = 0.2820948f, c1 = 0.4886025f, c2 = 1.0925484f, c3 = 0.31539157f, c4 = 0.5462742f:
 *            Y0 = c0, Y1 = c1*y, Y2 = c1*z, Y3 = c1*x, Y4 = (c2*x)*y, Y5 = (c2*y)*z, Y6 = c3*((3.0f*z)*z - 1.0f), Y7 = (c2*x)*z,
 *            Y8 = c4*(x*x - y*y).
 *   term     term[j][k][ch] = Y_k * g_j[ch].
 *   sum      directions in batches of 64; within a batch the 64 terms are summed by a balanced binary tree over neighbouring
 *            indices (x = x[0::2] + x[1::2], six times); the batch sums are added in ascending batch order starting from batch
 *            0's sum (no leading 0 +); sh_out[p][k][ch] = scale * acc, scale = (float)(4 pi / (double)(D samples)).
 *
 * dirs == NULL is the library's own set, the spherical Fibonacci points, computed in double and rounded once to float:
 * z = 1.0 - (2.0 j + 1.0) / D, r = sqrt(1.0 - z z), phi = j * (pi * (3.0 - sqrt(5.0))), the point (r cos phi, r sin phi, z);
 * mort_hip_probe_directions writes it and needs no GPU.  The _device form keeps the set of the last D in a buffer the context
 * owns.  A caller's own set must be equal-weight; that is not checked.  Zero-length, non-finite and unnormalised directions are
 * legal: the answer is the formulas'.
 *
 * mort_hip_sh9_irradiance (plain host code): E(n) = sum_k A_l(k) sh[k] Y_k(n) per channel, A_0 = pi, A_1 = 2 pi / 3, A_2 = pi / 4
 * (Ramamoorthi-Hanrahan), Y_k the expressions above with the same constants, evaluated in double and rounded once; `normal`
 * is used as given and should be of unit length.
 *
 * Forms, `seconds`, alignment and overlap as for the queries; the streams count as an output.  NULL params, probes, states or
 * sh_out, directions outside 64..4096 or not a multiple of 64, samples < 1, n D above the queries' ray limit (or n above
 * 2^31 - 1: one workgroup per probe) and overlapping buffers are MORT_ERR_INVALID; bounce_limit and the light object are checked
 * as the radiance queries check them.  n == 0 is MORT_OK and launches nothing.  The calls need an uploaded world (else
 * MORT_ERR_NO_WORLD) but no seeded pixel RNG, ignore the partition, and touch nothing the render keeps across frames. ---- */
typedef struct mort_probe { float position[3]; float time; } mort_probe; /* 16 B */
typedef struct mort_probe_params {
    mort_radiance_params rp; /* bounce_limit, samples (paths per direction), background, light object: as for the radiance queries */
    int directions;          /* D: 64..4096, a multiple of 64 */
} mort_probe_params;
#define MORT_SH9_FLOATS 27 /* [9 coefficients][3 channels] per probe */
MORT_SA(sizeof(mort_probe) == 16 && sizeof(mort_probe_params) == sizeof(mort_radiance_params) + 4, "light probe layout");
int mort_hip_probe_directions(int directions, float *dirs_out /* 3 D */);
int mort_hip_probe_bake(mort_ctx *ctx, const mort_probe_params *params, size_t n, const mort_probe *probes, const float *dirs /* 3 D or NULL */,
                        mort_rng_state *states /* n D */, float *sh_out /* 27 n */, double *seconds);
int mort_hip_probe_bake_device(mort_ctx *ctx, const mort_probe_params *params, size_t n, const void *d_probes, const void *d_dirs /* or NULL */,
                               void *d_states, void *d_sh_out, void *stream, double *seconds);
int mort_hip_probe_bake_host(const mort_world *world, const mort_probe_params *params, size_t n, const mort_probe *probes, const float *dirs,
                             mort_rng_state *states, int nthreads, int flags, float *sh_out, double *seconds);
int mort_hip_sh9_irradiance(const float sh[MORT_SH9_FLOATS], const float normal[3], float rgb_out[3]);

/* ---- irradiance volumes: a regular grid of light probes sampled trilinearly on the device.  The probes of a
 * grid are baked with mort_hip_probe_bake*, packed into one 128-byte record each, and a kernel gives the irradiance at every
 * (position, normal) of a batch, blended between the eight surrounding probes under a per-probe weight.  The arithmetic and the
 * order of the blend below are part of the contract: GPU kernel, host loop and any restatement of it agree to the bit.
 *
 * The grid.  Probe (ix, iy, iz) has index p = (iz count[1] + iy) count[0] + ix, position origin[a] + (float)i_a * spacing[a] per
 * axis (fp32: the product is rounded, then the sum) and time grid.time.  A valid grid has a finite origin, spacing finite and > 0
 * on every axis (also where count is 1), every count in 1..MORT_VOLUME_MAX_COUNT and at most 2^31 - 1 probes; anything else is
 * MORT_ERR_INVALID.  mort_hip_volume_probes (plain host code) writes the mort_probe records in index order, ready for the bake.
 *
 * A record is MORT_VOLUME_RECORD_FLOATS floats: the probe's 27 SH9 floats as the bake writes them, the weight, four 0.0f.
 * 128 bytes are one cache line of the device: with records aligned to 128 bytes each corner costs exactly one line (advice; the
 * _device forms ask for 16 bytes as every other call does).  A record is read as seven 16-byte loads, its last 16 bytes never.
 * mort_hip_volume_pack* copies the 27 floats bit for bit (NaN payloads included), then the weight as given (weight == NULL:
 * 1.0f), then the zeros.  The weight is the caller's: 0 masks a probe, no validity rule is built in.
 *
 * A point is the first 24 bytes of a record of `stride` bytes: position, then normal -- the head of a mort_hit, so the output of
 * mort_hip_query_closest_device is sampled with stride 48 and no copy.  stride >= 24 and a multiple of 4, else MORT_ERR_INVALID;
 * the bytes between the points are not read.
 *
 * One sample, everything fp32, nothing contracted, nothing reordered.  Per axis a, with inv[a] = 1.0f / spacing[a] (correctly
 * rounded, once per call):
 *   u  = (x[a] - origin[a]) * inv[a];  u = (u > 0) ? u : 0 (NaN goes to 0);  m = (float)(count[a] - 1);  u = (u < m) ? u : m
 *   i0 = (int)floorf(u);  if (i0 > count[a] - 2) i0 = count[a] - 2;  if (i0 < 0) i0 = 0
 *   f  = u - (float)i0;  i1 = (i0 + 1 < count[a]) ? i0 + 1 : i0;  w[a][0] = 1.0f - f;  w[a][1] = f
 * so a point outside the grid takes the boundary's value and an axis with one probe has f = 0.
 *   B_k  = A_l(k) * Y_k(n): Y_k the nine expressions of the light probes above at the normal AS GIVEN (not normalised),
 *          A_0 = (float)M_PI, A_1 = (float)(2.0 * M_PI / 3.0), A_2 = (float)(M_PI / 4.0).
 *   For corner c = cx + 2 cy + 4 cz in ascending c, the probe (i_cx, i_cy, i_cz):
 *          T_c = (w[0][cx] * w[1][cy]) * w[2][cz],  W_c = T_c * weight_c.
 *          A corner contributes only if W_c > 0; otherwise its coefficients are not used (a masked probe that holds NaN poisons
 *          nothing).  For a contributing corner e_c[ch] = ((B_0 sh_c[0][ch] + B_1 sh_c[1][ch]) + ...) + B_8 sh_c[8][ch] (from
 *          the k = 0 product, no leading 0 +), acc[ch] = acc[ch] + W_c * e_c[ch], wsum = wsum + W_c, both from 0.0f.
 *   out  = {acc[0] * r, acc[1] * r, acc[2] * r, wsum} with r = 1.0f / wsum correctly rounded where wsum > 0, else {0, 0, 0, 0}:
 *          the fourth float shows a point that no valid probe covers.
 *
 * Forms, `seconds`, streams, n == 0 and alignment as for the queries; the _host forms take `nthreads` and make no HIP call.
 * Outputs must not overlap inputs (the points count with their span (n - 1) stride + 24).  NULL grid, records, points, sh or
 * outputs are MORT_ERR_INVALID.  None of these calls needs an uploaded world or an RNG; they ignore the partition and touch
 * nothing the render keeps. ---- */
typedef struct mort_volume_grid { float origin[3]; float spacing[3]; int32_t count[3]; float time; } mort_volume_grid; /* 40 B */
typedef struct mort_volume_point { float p[3], normal[3]; } mort_volume_point; /* 24 B: the head of a mort_hit */
#define MORT_VOLUME_RECORD_FLOATS 32 /* 128 B per probe: [27 SH9 floats as the bake writes them][weight][4 x 0.0f] */
#define MORT_VOLUME_MAX_COUNT 4096   /* probes per axis */
MORT_SA(sizeof(mort_volume_grid) == 40 && sizeof(mort_volume_point) == 24, "irradiance volume layout");
int mort_hip_volume_probes(const mort_volume_grid *grid, mort_probe *probes_out /* count[0] count[1] count[2] */);
int mort_hip_volume_pack(mort_ctx *ctx, size_t n, const float *sh /* 27 n */, const float *weight /* n or NULL = 1.0f */,
                         float *records_out /* 32 n */, double *seconds);
int mort_hip_volume_pack_device(mort_ctx *ctx, size_t n, const void *d_sh, const void *d_weight /* or NULL */, void *d_records_out,
                                void *stream, double *seconds);
int mort_hip_volume_pack_host(size_t n, const float *sh, const float *weight, int nthreads, float *records_out, double *seconds);
int mort_hip_volume_sample(mort_ctx *ctx, const mort_volume_grid *grid, const float *records, size_t n, const void *points, size_t stride,
                           float *out /* 4 n */, double *seconds);
int mort_hip_volume_sample_device(mort_ctx *ctx, const mort_volume_grid *grid, const void *d_records, size_t n, const void *d_points,
                                  size_t stride, void *d_out, void *stream, double *seconds);
int mort_hip_volume_sample_host(const mort_volume_grid *grid, const float *records, size_t n, const void *points, size_t stride, int nthreads,
                                float *out, double *seconds);

/* ---- visibility-weighted irradiance volumes: per-probe depth maps and a Chebyshev test in the sampler.  The
 * blend above weighs the eight probes round a point by trilinear weight alone, so a probe behind a wall lights a surface it
 * cannot see.  Here every probe also gets an octahedral map of the first two moments of the distance to the nearest solid, baked
 * on the device, and the sampler multiplies each corner's weight by the Chebyshev bound on the probability that the probe sees the
 * point.  Everything is fp32, nothing contracted or reordered, every / and square root correctly rounded: GPU kernel, host loop
 * and any restatement agree to the bit.
 *
 * A depth map is MORT_DEPTH_FLOATS floats: (R + 2) x (R + 2) texels of two floats (m1, m2), R = MORT_DEPTH_RES = 8, row-major;
 * texel (i, j) sits at float 2 (j 10 + i): 800 bytes per probe.  Interior texels are i, j in 1..8; the one-texel border holds
 * copies so that the sampler's bilinear taps never wrap, in bordered coordinates:
 *   (0, j) <- (1, 9 - j), (9, j) <- (8, 9 - j) for j in 1..8;  (i, 0) <- (9 - i, 1), (i, 9) <- (9 - i, 8) for i in 1..8;
 *   (0, 0) <- (8, 8), (9, 9) <- (1, 1), (0, 9) <- (8, 1), (9, 0) <- (1, 8).
 *
 * The bake.  params->subsamples = s in 1..8, params->max_distance finite and > 0, else MORT_ERR_INVALID.  For probe p and interior
 * texel (i + 1, j + 1), i, j in 0..7, the sub-samples (a, b) in ascending b and within b in ascending a, with
 * step = 2.0f / (float)(8 s) and inv = 1.0f / (float)(s s), each rounded once on the host:
 *   u = ((float)(i s + a) + 0.5f) * step - 1.0f, v the same from (j, b);  z = (1.0f - |u|) - |v|;
 *   z < 0: x = (1.0f - |v|) * (u >= 0 ? 1.0f : -1.0f), y = (1.0f - |u|) * (v >= 0 ? 1.0f : -1.0f);  else x = u, y = v.
 *   ray    origin position_p, direction (x, y, z) as computed (NOT normalised), time time_p, t_max = +inf; searched as
 *          mort_hip_query_closest searches with states == NULL: media are passed over and nothing is drawn.
 *   len = sqrt((x x + y y) + z z);  d = hit ? t * len : max_distance;  d = (d < max_distance) ? d : max_distance (a NaN goes to
 *   the cap);  m1 = m1 + d, m2 = m2 + d * d, both from 0.0f.
 * The texel is (m1 * inv, m2 * inv); the border copies follow the table above.
 * Forms, alignment, overlap, `seconds`, n == 0 (MORT_OK, nothing launched), MORT_ERR_NO_WORLD and MORT_HOST_TREE as for
 * mort_hip_probe_bake*; there is no RNG and no light object.  NULL params, probes or depth_out are MORT_ERR_INVALID.
 *
 * The sampler takes mort_hip_volume_sample*'s arguments, the maps (`depth`, MORT_DEPTH_FLOATS per probe in grid index order) and
 * mort_volume_vis_params: normal_bias and min_visibility finite and >= 0, min_visibility <= 1, else MORT_ERR_INVALID (as are a
 * NULL depth or params, and maps that overlap the output).  One sample is the plain sampler's, word for word, but for the corner
 * weight.  For corner c with W0_c = T_c * weight_c: if !(W0_c > 0) the corner is skipped as there -- neither its map nor its
 * coefficients influence the result.  Otherwise, per axis a,
 *   q[a] = x[a] + normal_bias * n[a];  pos[a] = origin[a] + (float)i_a * spacing[a] (product rounded, then the sum);
 *   v[a] = q[a] - pos[a];  r = sqrt((v0 v0 + v1 v1) + v2 v2);  s1 = (|v0| + |v1|) + |v2|.
 *   !(s1 > 0) || !(s1 < +inf): V = 1.0f.  Otherwise
 *   ox = v0 / s1, oy = v1 / s1;  v2 < 0: (ox, oy) = ((1.0f - |oy|) * (ox >= 0 ? 1 : -1), (1.0f - |ox|) * (oy >= 0 ? 1 : -1)), both
 *   from the old values;
 *   tx = (ox * 0.5f + 0.5f) * 8.0f + 0.5f, i0 = (int)floorf(tx) clamped to 0..8, fx = tx - (float)i0; ty, j0, fy the same;
 *   per moment, with t(i, j) the map's texel:  top = t(i0, j0) * (1.0f - fx) + t(i0 + 1, j0) * fx,
 *   bot = t(i0, j0 + 1) * (1.0f - fx) + t(i0 + 1, j0 + 1) * fx,  m = top * (1.0f - fy) + bot * fy;
 *   r > m1: var = |m2 - m1 m1|, dl = r - m1, den = var + dl dl, k = (den > 0) ? var / den : 0.0f, V = (k k) k,
 *   V = (V > min_visibility) ? V : min_visibility;  else (also for a NaN on either side) V = 1.0f.
 *   W_c = W0_c * V; the corner contributes only if W_c > 0, and from there the nine-term sums, the accumulation from 0.0f, wsum
 *   and 1.0f / wsum are the plain sampler's.
 * So with V = 1 at every corner the output equals mort_hip_volume_sample's bit for bit, and with min_visibility = 0 a fully
 * occluded probe drops out of the blend and cannot poison the sum.  None of the sampler's forms needs an uploaded world. ---- */
#define MORT_DEPTH_RES 8
#define MORT_DEPTH_FLOATS 200 /* (8 + 2) x (8 + 2) texels x (m1, m2): 800 B per probe */
typedef struct mort_depth_params { int subsamples; float max_distance; } mort_depth_params;
typedef struct mort_volume_vis_params { float normal_bias; float min_visibility; } mort_volume_vis_params;
MORT_SA(sizeof(mort_depth_params) == 8 && sizeof(mort_volume_vis_params) == 8 && MORT_DEPTH_FLOATS * sizeof(float) == 800,
        "depth map layout");
int mort_hip_probe_depth_bake(mort_ctx *ctx, const mort_depth_params *params, size_t n, const mort_probe *probes, float *depth_out /* 200 n */,
                              double *seconds);
int mort_hip_probe_depth_bake_device(mort_ctx *ctx, const mort_depth_params *params, size_t n, const void *d_probes, void *d_depth_out,
                                     void *stream, double *seconds);
int mort_hip_probe_depth_bake_host(const mort_world *world, const mort_depth_params *params, size_t n, const mort_probe *probes, int nthreads,
                                   int flags, float *depth_out, double *seconds);
int mort_hip_volume_sample_visible(mort_ctx *ctx, const mort_volume_grid *grid, const float *records, const float *depth,
                                   const mort_volume_vis_params *params, size_t n, const void *points, size_t stride, float *out /* 4 n */,
                                   double *seconds);
int mort_hip_volume_sample_visible_device(mort_ctx *ctx, const mort_volume_grid *grid, const void *d_records, const void *d_depth,
                                          const mort_volume_vis_params *params, size_t n, const void *d_points, size_t stride, void *d_out,
                                          void *stream, double *seconds);
int mort_hip_volume_sample_visible_host(const mort_volume_grid *grid, const float *records, const float *depth,
                                        const mort_volume_vis_params *params, size_t n, const void *points, size_t stride, int nthreads,
                                        float *out, double *seconds);

/* ---- cached radiance queries: paths that end in an irradiance volume.  The final-gather use of a probe grid: a
 * path runs its first K = cache_depth bounces as a radiance query runs them, and at the first Lambertian surface after that it
 * returns albedo * E(p, n) / pi from the volume instead of tracing on.
 *
 * The calls take the radiance queries' arguments (rays, streams advanced in place, rgb_out 3 n), and in addition `records`
 * (MORT_VOLUME_RECORD_FLOATS per probe of params->grid, as mort_hip_volume_pack* writes them), `depth` (MORT_DEPTH_FLOATS per
 * probe: required with MORT_CACHED_VISIBLE, NULL without) and an optional ends_out (n words or NULL): per ray, how many of its
 * `samples` paths ended in the volume.
 *
 * The path is the radiance query's with one addition.  At iteration `iter` of a path (0 = the caller's ray's own hit), when the
 * segment's search has found a hit and before its emission or scatter is evaluated:
 *   1. if iter >= K and the hit's material tag is MORT_MAT_LAMBERTIAN (isotropic, metal, dielectric, lights and unknown tags
 *      never), the volume is sampled at the hit's point and its facing normal, by mort_hip_volume_sample*'s arithmetic, or with
 *      MORT_CACHED_VISIBLE by mort_hip_volume_sample_visible*'s under params->vis, word for word;
 *   2. if the returned weight sum is > 0 the path ends here: its final value per channel is (albedo_c * E_c) * INV_PI, albedo the
 *      material's texture value at the hit, INV_PI = (float)(1.0 / 3.14159265358979323846); no random number is drawn for this hit
 *      and the ray's count goes up by one; the unwind and the sum over the samples are the radiance query's;
 *   3. otherwise (a weight sum of 0 or NaN: no probe contributes) the iteration goes on exactly as in a radiance query.
 * Everything else is the radiance queries': the reach test per origin, the media after the solids with their draws, the bounce
 * limit, no NaN guard (a NaN coefficient reaches the colour).  So with K >= bounce_limit, or with every weight 0, the call is a
 * radiance query to the bit, streams included.
 *
 * Forms, `seconds`, n == 0, alignment (the _device form: every buffer 16 bytes) and overlap as for the radiance queries; the
 * streams and the counts are outputs, the records and maps inputs.  The radiance calls' checks apply to params->path and the
 * volume calls' to params->grid and, with the flag, params->vis.  cache_depth outside 0..MORT_MAX_BOUNCE_LIMIT, an unknown flag
 * bit, a NULL records, and depth present without MORT_CACHED_VISIBLE or absent with it are MORT_ERR_INVALID. ---- */
#define MORT_CACHED_VISIBLE 1u
typedef struct mort_cached_params {
    mort_radiance_params path;  /* bounce limit, samples, background, light object: as a radiance query */
    int32_t cache_depth;        /* K, 0 .. MORT_MAX_BOUNCE_LIMIT */
    uint32_t flags;             /* 0 or MORT_CACHED_VISIBLE */
    mort_volume_grid grid;
    mort_volume_vis_params vis; /* read only with MORT_CACHED_VISIBLE */
} mort_cached_params;
MORT_SA(sizeof(mort_cached_params) == 84, "cached radiance query layout");
int mort_hip_query_radiance_cached(mort_ctx *ctx, const mort_cached_params *params, size_t n, const mort_ray *rays, mort_rng_state *states,
                                   const float *records, const float *depth /* or NULL */, float *rgb_out, uint32_t *ends_out /* n or NULL */,
                                   double *seconds);
int mort_hip_query_radiance_cached_device(mort_ctx *ctx, const mort_cached_params *params, size_t n, const void *d_rays, void *d_states,
                                          const void *d_records, const void *d_depth, void *d_rgb_out, void *d_ends_out, void *stream,
                                          double *seconds);
int mort_hip_query_radiance_cached_host(const mort_world *world, const mort_cached_params *params, size_t n, const mort_ray *rays,
                                        mort_rng_state *states, const float *records, const float *depth, int nthreads, int flags,
                                        float *rgb_out, uint32_t *ends_out, double *seconds);

/* ---- direct-light cached radiance queries: a sampled light plus a volume of indirect light.  A 128-byte SH9
 * record cannot hold the emitters' own light -- its shadows and the fall-off under a small emitter are lost -- so the volume keeps
 * indirect light only and a path that ends in it adds one sampled shadow segment toward the light object.
 *
 * The indirect volume is a composition of two bakes, not a call of its own.  "Indirect" is the radiance arriving at a probe with
 * the emission of directly seen emitters taken out; the background and every reflected bounce stay in.
 *   sh_full  mort_hip_probe_bake* under the caller's mort_probe_params;
 *   sh_emit  mort_hip_probe_bake* over the same probes and directions, from a COPY of the streams sh_full started from, under the
 *            same params changed in three fields: rp.bounce_limit = 1, rp.background = 0, rp.samples = 1 (at limit 1 a path
 *            returns its first hit's emission or 0);
 *   sh_ind[i] = sh_full[i] - sh_emit[i], one fp32 subtraction per float; mort_hip_volume_pack* makes the records of it.
 *
 * The calls take mort_hip_query_radiance_cached*'s arguments under the same mort_cached_params -- no new flag bit -- and one more
 * optional output, lit_out (n words or NULL): per ray, how many of its paths' shadow segments returned a non-zero emission.
 * Everything is fp32, nothing contracted, every / correctly rounded.  The path is the cached query's, word for word, but for its
 * step 2: the hit is Lambertian, iter >= K, the weight sum is > 0 and the path ends, with the final value per channel
 *   final_c = ((albedo_c * E_c) * INV_PI) + direct_c,    direct formed in this order:
 *   a. if params->path.light_obj_type == -1, or iter + 1 >= bounce_limit, there is no direct term: nothing is drawn, nothing is
 *      added, and final_c is the cached query's to the bit;
 *   b. dir = the light object's random direction from p, drawn from the ray's stream as the render's light sampling draws it;
 *      pdf = the light object's pdf_value(p, dir);  cosine = dot(n, unit(dir)), n the hit's facing normal;
 *      spdf = cosine < 0 ? 0 : cosine * INV_PI;
 *   c. the shadow segment (p, dir, the ray's time) is searched as every path segment is: [0.001, inf), the solids, then the media
 *      with their draws from the stream.  If it ends on a hit whose material tag is MORT_MAT_DIFFUSE_LIGHT, Le is the emission a
 *      radiance query returns at that hit (front face only, the light's texture); otherwise -- a miss, a medium's scatter point,
 *      any other material -- Le = 0.  No scatter is evaluated and nothing further is drawn; a miss does not return the
 *      background, which is in the probes;
 *   d. direct_c = ((albedo_c * spdf) * Le_c) / pdf, without a guard: a zero, infinite or NaN pdf gives what the division gives.
 *      The ray's count in lit_out goes up by one when any Le_c != 0.
 * The unwind, the sum over the samples and ends_out are the cached query's.  So
 *   (i)   with no light object the call is mort_hip_query_radiance_cached* to the bit, streams included;
 *   (ii)  with K >= bounce_limit, or with every weight 0, it is mort_hip_query_radiance* to the bit;
 *   (iii) ends_out is the cached query's for the same inputs wherever the streams have not yet parted: the terminal hit ends the
 *         path, and the streams differ only by the draws of (b) and (c).
 * Checks, forms, `seconds`, n == 0, alignment and overlap as for the cached queries; lit_out is one more output. ---- */
int mort_hip_query_radiance_cached_direct(mort_ctx *ctx, const mort_cached_params *params, size_t n, const mort_ray *rays, mort_rng_state *states,
                                          const float *records, const float *depth /* or NULL */, float *rgb_out, uint32_t *ends_out /* n or NULL */,
                                          uint32_t *lit_out /* n or NULL */, double *seconds);
int mort_hip_query_radiance_cached_direct_device(mort_ctx *ctx, const mort_cached_params *params, size_t n, const void *d_rays, void *d_states,
                                                 const void *d_records, const void *d_depth, void *d_rgb_out, void *d_ends_out, void *d_lit_out,
                                                 void *stream, double *seconds);
int mort_hip_query_radiance_cached_direct_host(const mort_world *world, const mort_cached_params *params, size_t n, const mort_ray *rays,
                                               mort_rng_state *states, const float *records, const float *depth, int nthreads, int flags,
                                               float *rgb_out, uint32_t *ends_out, uint32_t *lit_out, double *seconds);

/* ---- cached frames: renders whose paths end in an irradiance volume.  Camera::render for every pixel, as
 * mort_hip_render runs it -- the pixel's stream from the context (or `states`), get_ray per stratum drawn from that stream, the flat
 * sample x bounce loop with one segment counted per search, the unwind, the pixel's finish and its uchar4, the stream stored back
 * -- with the cached radiance queries' one shortcut inside the bounce loop: after a search that found a hit and before that hit is
 * shaded, at iteration iter >= K = cache_depth, steps 1-3 above; a path that ends so makes no draw for that hit, its segment is
 * counted as any other, and the pixel's count in ends_px_out goes up by one.  The bounce limit, the background, the light object
 * and the samples are the camera's.  So with K >= cam->bounce_limit, or with every weight 0, a cached frame is
 * mort_hip_render(..., MORT_MODE_MEGA, ...) to the bit: uchar4, accumulators, per-pixel segments, final streams, stats.segments
 * and stats.rng_draws.
 *
 * `records`, `depth` and the flag as for the cached queries.  ends_px_out (one uint32 per pixel, or NULL): how many of the pixel's
 * sqrt_spp^2 paths ended in the volume.  The three forms mirror mort_hip_render / _render_device / _render_host: host buffers
 * (records and maps go up, results come down); caller's DEVICE buffers, every one 16-byte aligned, on `stream`, asynchronous
 * when stats is NULL; and the host loop of the same body, which needs no GPU (MORT_HOST_TREE as elsewhere).
 *
 * Checks: the render's (camera, world, seeded states of the frame's size) and the cached queries' (cache_depth, flags, grid, vis,
 * records, depth with and without the flag); an output that overlaps an input or another output is MORT_ERR_INVALID.  Only the
 * whole-image partition is supported, else MORT_ERR_UNSUPPORTED, as for a view.  mort_stats as the render fills it: kernel_name
 * the kernel with its template arguments, scene_in_lds 0, reference_walks 0, algorithmic_hbm_bytes the render's plus 4 B per
 * pixel when ends is written. ---- */
typedef struct mort_cached_frame_params {
    int32_t cache_depth;        /* K, 0 .. MORT_MAX_BOUNCE_LIMIT */
    uint32_t flags;             /* 0 or MORT_CACHED_VISIBLE */
    mort_volume_grid grid;
    mort_volume_vis_params vis; /* read only with MORT_CACHED_VISIBLE */
} mort_cached_frame_params;
MORT_SA(sizeof(mort_cached_frame_params) == 56, "cached frame layout");
int mort_hip_render_cached(mort_ctx *ctx, const mort_camera *cam, const mort_cached_frame_params *params, const float *records,
                           const float *depth /* or NULL */, uint8_t *rgba_out, float *accum_out /* or NULL */,
                           uint32_t *segments_px_out /* or NULL */, uint32_t *ends_px_out /* or NULL */, mort_stats *stats);
int mort_hip_render_cached_device(mort_ctx *ctx, const mort_camera *cam, const mort_cached_frame_params *params, const void *d_records,
                                  const void *d_depth, void *d_rgba, void *d_accum /* or NULL */, void *d_ends /* or NULL */, void *stream,
                                  mort_stats *stats);
int mort_hip_render_cached_host(const mort_world *world, const mort_camera *cam, mort_rng_state *states, int nthreads, int flags,
                                const mort_cached_frame_params *params, const float *records, const float *depth, uint8_t *rgba_out,
                                float *accum_out, uint32_t *segments_px_out, uint32_t *ends_px_out, mort_stats *stats);
/* a view's frames as cached frames (NULL params: plain renders again).  The caller owns d_records and d_depth, which must outlive
 * the view's frames; the checks are mort_hip_render_cached_device's for them.  Attaching or detaching forgets the history, as
 * mort_hip_view_reset does: the estimator changes and its variance with it.  With a cache attached a frame must use
 * MORT_MODE_MEGA, any other mode is MORT_ERR_UNSUPPORTED.  mort_hip_view_read(MORT_VIEW_ENDS) gives the last frame's counts of
 * paths that ended in the volume, which the view keeps in a buffer of its own. */
int mort_hip_view_set_cache(mort_view *v, const mort_cached_frame_params *params, const void *d_records, const void *d_depth);
/* the same for a caller without device buffers (the CLI): records and depth (or NULL) are host arrays, which the view copies into
 * device buffers of its own; those live until the next attach or detach by either form, or the view's end */
int mort_hip_view_set_cache_host(mort_view *v, const mort_cached_frame_params *params, const float *records, const float *depth);

/* ---- direct-light cached frames: cached frames over a volume of INDIRECT light whose paths add one sampled shadow segment toward
 * the light object where they end.  The calls take mort_hip_render_cached*'s arguments under the same
 * mort_cached_frame_params -- no new flag bit -- and one more optional output, lit_px_out / d_lit (one uint32 per pixel, or NULL):
 * how many of the pixel's paths had a shadow segment that returned a non-zero emission.  The volume is composed as for the
 * direct-light cached queries above (sh_full - sh_emit).
 *
 * A direct cached frame is a cached frame word for word, except at the hit where a path ends in the volume.  There steps (a)-(d)
 * of the direct-light cached queries apply, bound to the frame so:
 *   - the light object is cam->light_obj_type / cam->light_obj_idx, the bounce limit and the background are the camera's;
 *   - the shadow segment's time is the sample's ray time, the time get_ray gave that sample's ray;
 *   - the draws of (b) and (c) come from the pixel's stream, after the path's own draws and before the next sample's get_ray;
 *   - rule (a): with no light object, or when iter + 1 >= bounce_limit, nothing is drawn and nothing is added;
 *   - the shadow segment's search counts as a segment ("one segment counted per search"): in segments_px_out, in stats.segments
 *     and, through its draws, in stats.rng_draws;
 *   - ends counts a path once, however its terminal went; per pixel lit <= ends <= sqrt_spp^2.
 * So
 *   (i)   with cam->light_obj_type == -1 the call is mort_hip_render_cached* to the bit: uchar4, accumulators, per-pixel segments,
 *         ends, final streams, stats.segments and stats.rng_draws; lit is all 0;
 *   (ii)  with K >= cam->bounce_limit, or with every weight 0, it is mort_hip_render(..., MORT_MODE_MEGA, ...) to the bit;
 *   (iii) with cam->bounce_limit == K + 1 every terminal takes rule (a) and the frame is the cached frame to the bit.
 * Checks, forms, alignment, overlap, the partition's refusal (MORT_ERR_UNSUPPORTED), the asynchronous form and the deferred stats
 * are the cached frame's; lit is one more output among those that must not overlap, 16-byte aligned in the _device form.
 * mort_stats as the cached frame fills it: algorithmic_hbm_bytes the cached frame's plus 4 B per pixel when lit is written,
 * kernel_name cached_frame_direct_kernel<TREE, VISIBLE>; the host loop's name says "cached frame, direct". ---- */
int mort_hip_render_cached_direct(mort_ctx *ctx, const mort_camera *cam, const mort_cached_frame_params *params, const float *records,
                                  const float *depth /* or NULL */, uint8_t *rgba_out, float *accum_out /* or NULL */,
                                  uint32_t *segments_px_out /* or NULL */, uint32_t *ends_px_out /* or NULL */, uint32_t *lit_px_out /* or NULL */,
                                  mort_stats *stats);
int mort_hip_render_cached_direct_device(mort_ctx *ctx, const mort_camera *cam, const mort_cached_frame_params *params, const void *d_records,
                                         const void *d_depth, void *d_rgba, void *d_accum /* or NULL */, void *d_ends /* or NULL */,
                                         void *d_lit /* or NULL */, void *stream, mort_stats *stats);
int mort_hip_render_cached_direct_host(const mort_world *world, const mort_camera *cam, mort_rng_state *states, int nthreads, int flags,
                                       const mort_cached_frame_params *params, const float *records, const float *depth, uint8_t *rgba_out,
                                       float *accum_out, uint32_t *segments_px_out, uint32_t *ends_px_out, uint32_t *lit_px_out,
                                       mort_stats *stats);
/* mort_hip_view_set_cache* with the view's frames run as direct cached frames: the same checks, the history forgotten the same
 * way.  Attaching by either family replaces what the other attached; NULL params detaches.  mort_hip_view_update_cache* works
 * unchanged on such a view: the params and the direct-ness stay, the history is kept.  mort_hip_view_read(MORT_VIEW_LIT) gives
 * the last frame's lit counts, kept beside the ends; it is MORT_ERR_INVALID unless a direct cache is attached. */
int mort_hip_view_set_cache_direct(mort_view *v, const mort_cached_frame_params *params, const void *d_records, const void *d_depth);
int mort_hip_view_set_cache_direct_host(mort_view *v, const mort_cached_frame_params *params, const float *records, const float *depth);

/* ---- volume refresh: probes re-baked through the volume and blended into their records.  The producer that uses
 * the cache: a probe's rays are traced as cached paths that end in the volume as it stands, projected as the bake projects them,
 * and blended into the probe's record under a hysteresis, so each round carries light one bounce further at the cost of a cached
 * query per direction, and any subset of the probes can be refreshed between two frames.  Kernel, host loop and any restatement
 * agree to the bit.
 *
 * Let P be the probes of params->cached.grid, D = params->directions, m the call's number of selected probes
 * p_i = first + i step, i = 0 .. m - 1.
 *   states       P D streams for the WHOLE grid, probe p direction j uses states[p D + j]; only the selected probes' streams move,
 *                so a partial refresh leaves every other probe's streams where its last refresh left them.
 *   records_in, records_out   P records each (MORT_VOLUME_RECORD_FLOATS floats); the call writes the m selected records of
 *                records_out and no other byte of it.
 *   depth        the maps, P x MORT_DEPTH_FLOATS: required with MORT_CACHED_VISIBLE in cached.flags, NULL without.
 *   ends_out     P words or NULL, written for the selected probes only: how many of the probe's D samples paths ended in the volume.
 *   dirs         3 D floats or NULL = mort_hip_probe_directions' set, as for the bake.
 *
 * For a selected probe p = (iz ny + iy) nx + ix, everything fp32 and nothing contracted:
 *   1. if the weight records_in[p][27] is not > 0 (0, negative, NaN) the record is copied to records_out[p] bit for bit; no path
 *      runs, no stream moves, ends_out[p] = 0.  Masking is the caller's rule, and a masked probe is usually one inside geometry.
 *   2. position origin[a] + (float)i_a * spacing[a] per axis (the product rounded, then the sum), time grid.time:
 *      mort_hip_volume_probes' arithmetic, computed where the probe is refreshed.
 *   3. for direction j the ray is (position, dirs[j] exactly as given, time) and the stream states[p D + j] is advanced in place as
 *      the bake advances it; the paths are the cached query's over records_in and depth under params->cached, word for word (its
 *      steps 1-3 with K = cached.cache_depth, samples = cached.path.samples paths per direction, MORT_CACHED_VISIBLE honoured).
 *   4. the projection is the light probes': the NaN guard on the direction's sum, the nine basis expressions,
 *      term[k][ch] = Y_k * g[ch], batches of 64 summed by the balanced tree, the batch sums added in ascending order from batch 0's
 *      sum, new[k][ch] = scale * acc with scale = (float)(4 pi / (double)(D samples)).
 *   5. the blend, for each of the 27 floats with old = records_in[p][i]: if hysteresis == 0.0f, out = new bit for bit; otherwise
 *      out = (h * old) + (om * new) with om = 1.0f - h rounded once per call.  Nothing is guarded: a NaN in old stays NaN for
 *      h > 0.  Float 27, the weight, is copied bit for bit; floats 28..31 are 0.0f.
 *   6. ends_out[p] is the sum of the directions' counts.
 * So with hysteresis 0, K >= bounce_limit and records_in = mort_hip_volume_pack(zeros, weight) with every weight > 0, the first 27
 * floats of every selected record and all streams equal mort_hip_probe_bake* over mort_hip_volume_probes(grid) to the bit, and
 * the record equals mort_hip_volume_pack* of that bake; and the selected records never depend on the unselected bytes of
 * records_out.
 *
 * mort_hip_probe_directions_round (plain host code) gives a direction set per refresh round: with K = 0 in a diffuse world a
 * refresh draws no random number, so the set is the only sampling and an unrotated set would repeat its aliasing every round.
 * Round 0 is mort_hip_probe_directions bit for bit.  Round r >= 1 is that set rotated, in double, rounded once: with v_j the
 * library's D-point direction j in double before rounding, k = (k0, k1, k2) direction r mod 64 of the 64-point set in double before
 * rounding, theta = (double)r * (pi * (3.0 - sqrt(5.0))), c = cos theta, s = sin theta, t = 1.0 - c, the Rodrigues matrix
 *   R = { c + (t k0) k0,      (t k0) k1 - s k2,   (t k0) k2 + s k1 }
 *       { (t k0) k1 + s k2,   c + (t k1) k1,      (t k1) k2 - s k0 }
 *       { (t k0) k2 - s k1,   (t k1) k2 + s k0,   c + (t k2) k2    }
 * and out[j][a] = (float)((R[a][0] v_j[0] + R[a][1] v_j[1]) + R[a][2] v_j[2]).
 *
 * Checks, in this order: NULL params, states, records_in or records_out; directions outside 64..4096 or not a multiple of 64,
 * samples < 1; the cached calls' checks of cache_depth, flags, grid, vis and depth against the flag; hysteresis NaN, < 0 or >= 1;
 * step == 0, or (m > 0) first + (m - 1) step >= P computed without overflow; P D above the queries' ray limit -- all
 * MORT_ERR_INVALID.  records_out, states and ends_out are outputs, dirs, records_in and depth inputs: an output that overlaps an
 * input or another output is MORT_ERR_INVALID -- an in-place refresh is refused on purpose, the paths of one probe would read
 * records another workgroup is writing.  Then the bounce limit (MORT_ERR_CAPACITY), for the _device form every buffer 16-byte
 * aligned, an uploaded world (MORT_ERR_NO_WORLD) and the light object, as for the bake.  m == 0 is MORT_OK and touches nothing.
 * Forms, `seconds` and MORT_HOST_TREE as for the bake; the host-buffer form sends records_out up as well, so its unselected records
 * come back as they went.  The calls ignore the partition, need no pixel RNG and touch nothing the render keeps. ---- */
typedef struct mort_refresh_params {
    mort_cached_params cached; /* path (samples = paths per direction), cache_depth K, flags, grid, vis: as a cached query */
    int32_t directions;        /* D: a multiple of 64 in 64..4096, as a probe bake */
    float hysteresis;          /* h, finite, 0 <= h < 1 */
    uint32_t first, step;      /* the selected probes: p_i = first + i * step, i = 0 .. m - 1 */
} mort_refresh_params;
MORT_SA(sizeof(mort_refresh_params) == 100, "volume refresh layout");
int mort_hip_volume_refresh(mort_ctx *ctx, const mort_refresh_params *params, size_t m, const float *dirs /* 3 D or NULL */,
                            mort_rng_state *states /* P D */, const float *records_in, const float *depth /* or NULL */, float *records_out,
                            uint32_t *ends_out /* P or NULL */, double *seconds);
int mort_hip_volume_refresh_device(mort_ctx *ctx, const mort_refresh_params *params, size_t m, const void *d_dirs /* or NULL */, void *d_states,
                                   const void *d_records_in, const void *d_depth, void *d_records_out, void *d_ends_out, void *stream,
                                   double *seconds);
int mort_hip_volume_refresh_host(const mort_world *world, const mort_refresh_params *params, size_t m, const float *dirs, mort_rng_state *states,
                                 const float *records_in, const float *depth, int nthreads, int flags, float *records_out, uint32_t *ends_out,
                                 double *seconds);
int mort_hip_probe_directions_round(int directions, uint32_t round, float *dirs_out /* 3 D */);

/* ---- direct-light volume refresh: the volume refresh for a volume of INDIRECT light.  "Indirect" is the
 * direct-light cached queries' definition: the radiance arriving at a probe with the emission of directly seen emitters taken out;
 * the background and every reflected bounce stay in.  The calls take mort_hip_volume_refresh*'s arguments under the same
 * mort_refresh_params -- no new flag bit -- and one more optional output after ends_out, lit_out / d_lit_out (P words or NULL,
 * written for the selected probes only): how many of the probe's D samples paths had a shadow segment that returned a non-zero
 * emission.  A copied (masked) probe writes 0.
 *
 * A direct refresh is the volume refresh above with two changes to its step 3; steps 1, 2, 4, 5 and 6, the checks and their order,
 * the forms, `seconds`, MORT_HOST_TREE, the stream layout, the selection and the copy rule are unchanged:
 *   3'. the paths are the direct-light cached query's (its rules (a)-(d)) over records_in and depth, word for word: a path that
 *       ends in the volume has the value ((albedo E) INV_PI) + ((albedo spdf) Le) / pdf, and the shadow segment counts and draws as
 *       it does there;
 *   E.  a path whose PRIMARY segment ends in the shade step's non-scattering branch (iteration 0, not a shadow segment, the hit a
 *       diffuse light or a material the shade step does not know) has the value (0, 0, 0) instead of what the shade step returned.
 *       Nothing else changes: the search, the shade step and every draw are made as before, so the streams equal those of the
 *       direct-light cached query on the same rays.  Emission met after a path-traced bounce stays in: it is reflected light.
 * So
 *   (A) in a world without an emitter, or called with light_obj_type == -1 where no primary ray meets an emitter, records, streams
 *       and ends equal mort_hip_volume_refresh* to the bit and lit is 0;
 *   (B) per path, with "the primary hit emits" read from mort_hip_query_radiance* at bounce limit 1 and a black background on a
 *       copy of the streams, and the path's value v from mort_hip_query_radiance_cached_direct* at one sample on the carried
 *       streams, the direction's sum is the sum of (emits ? 0 : v) in path order; projection and blend as above give the records
 *       to the bit, and the streams and both counts are the query's;
 *   (C) with hysteresis 0, K >= bounce_limit, one sample and records_in = mort_hip_volume_pack(zeros, weight > 0), the 27 floats
 *       equal mort_hip_probe_bake_indirect*'s sh_ind on the same probes, directions and streams up to the rounding of two fp32
 *       summations (the bake subtracts two sums, the refresh sums the differences), and the streams equal the full bake's to the bit;
 *   (D) a masked probe is copied, none of its streams moves, and both of its counts are 0;
 *   (E) the selected records never depend on the unselected bytes of records_out.
 * Per probe lit <= ends <= D samples.  lit_out is an output for the overlap checks: it must not overlap an input or another
 * output, and the _device form wants it 16-byte aligned.  The host-buffer form sends records_out up as well. ---- */
int mort_hip_volume_refresh_direct(mort_ctx *ctx, const mort_refresh_params *params, size_t m, const float *dirs /* 3 D or NULL */,
                                   mort_rng_state *states /* P D */, const float *records_in, const float *depth /* or NULL */,
                                   float *records_out, uint32_t *ends_out /* P or NULL */, uint32_t *lit_out /* P or NULL */, double *seconds);
int mort_hip_volume_refresh_direct_device(mort_ctx *ctx, const mort_refresh_params *params, size_t m, const void *d_dirs /* or NULL */,
                                          void *d_states, const void *d_records_in, const void *d_depth, void *d_records_out, void *d_ends_out,
                                          void *d_lit_out, void *stream, double *seconds);
int mort_hip_volume_refresh_direct_host(const mort_world *world, const mort_refresh_params *params, size_t m, const float *dirs,
                                        mort_rng_state *states, const float *records_in, const float *depth, int nthreads, int flags,
                                        float *records_out, uint32_t *ends_out, uint32_t *lit_out, double *seconds);

/* new records (and maps) for a view that has a cache attached: the params stay, the checks are mort_hip_view_set_cache's, the
 * presence of depth must match the attached flag, and a view without a cache is MORT_ERR_INVALID.  The history is KEPT: set_cache
 * forgets it because the estimator changes; a refreshed volume is the same estimator with a better cache.  The caller runs the
 * refresh on the frames' stream into a back buffer of its own and hands the view the pointer; the _host form copies the arrays
 * into device buffers of the view's own, as mort_hip_view_set_cache_host does. */
int mort_hip_view_update_cache(mort_view *v, const void *d_records, const void *d_depth);
int mort_hip_view_update_cache_host(mort_view *v, const float *records, const float *depth);

/* Number of rows owned for an image of `height` rows under the current partition. */
int mort_hip_local_rows(const mort_ctx *ctx, int height);
/* Global row index of local row `local_row`. */
int mort_hip_global_row(const mort_ctx *ctx, int local_row);

/* ---- diagnostics of the tile scheduler (DESIGN.md 5 "Reading the scheduler back"): what decides when and where a pixel is
 * rendered never reaches the pixel, so the tests read it here.  Nothing in this section launches or changes a render kernel. */
#define MORT_TILE_COUNTERS 96
typedef struct mort_tile_state {
    int32_t ordered;      /* 1: the launch was ordered by the cost order (0: sub-stream launch, MORT_NO_TILE_ORDER, tiles < 4 * grid, a family without one) */
    int32_t probed;       /* 1: the launch ran the one-sample cost probe first */
    int32_t tiles, tiles_x, grid, block;
    int32_t key_sum;      /* 1: MORT_TILE_KEY=sum */
    int32_t spread_shift, gen_tiles;
    int32_t heavy[4];     /* heavy waves of the launch: mod, num, cap, percent */
    int32_t has_head;     /* 1: heavy waves were on, `head` and `frame_total` are the launch's */
    uint32_t head;        /* tiles in the head of the order (tile_sort.hip heavy_count_kernel) */
    uint32_t pad_;
    uint64_t frame_total[MORT_TILE_COUNTERS]; /* the saved counters as heavy_count_kernel read them */
} mort_tile_state;
MORT_SA(sizeof(mort_tile_state) == 64 + 8 * MORT_TILE_COUNTERS, "tile state layout");
/* The last render launch of ctx, after waiting for its stream.  keys / order (what the launch was ordered by) and cost (what it left
 * for the next one) receive out->tiles words each when the launch was ordered and cap >= out->tiles; any of them may be NULL. */
int mort_hip_debug_tile_state(mort_ctx *ctx, mort_tile_state *out, uint32_t *keys, uint32_t *order, uint32_t *cost, size_t cap);
/* The scheduler's helper kernels on a caller's arrays, through the functions the render calls (host arrays in and out):
 * the descending stable argsort of n costs, */
int mort_hip_debug_tile_sort(int device, const uint32_t *cost, size_t n, uint32_t *keys_out, uint32_t *order_out);
/* the size of the heavy-wave head for n sorted keys (counters: MORT_TILE_COUNTERS words or NULL), */
int mort_hip_debug_heavy_count(int device, const uint32_t *keys, size_t n, uint32_t percent, uint32_t max_r, const uint64_t *counters,
                               uint64_t lanes, uint32_t *head_out);
/* and the frame gather's de-interleave of nranks tiles of packed rows, *tile_px pixels apart (the stride mort_hip_render_gather uses;
 * written whenever tile_px is not NULL, and alone when gathered and frame are NULL), into the W x H frame.  No RCCL is involved. */
int mort_hip_debug_deinterleave(int device, const uint8_t *gathered, int width, int height, int nranks, int rows_per_block,
                                uint8_t *frame_out, size_t *tile_px);

#ifdef __cplusplus
}
#endif
#endif /* MORT_HIP_H */
