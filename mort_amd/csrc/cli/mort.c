/*
 * mort -- command line of the renderer: `mort <scene_id>` as in the reference (mort.cu:633-689), plus overrides, file
 * output (the reference only draws into a GLUT window) and the multi-GPU / host modes the north_star names.  Host code
 * is C; every render goes through the C ABI of libmort_hip.so.  Errors print and exit like HANDLE_ERROR
 * (include/book.h:21-30).
 *
 *   mort <scene_id> [--width W] [--aspect A] [--spp N] [--depth D] [--seed S] [--frames N]
 *                   [--mode mega|wave|host|throughput] [--threads T] [--tree]       host: the kernel body as a host loop (no GPU)
 *                   [--gpus N] [--devices a,b,..] [--gather rccl|shm]     one process per GPU, rows partitioned, one gather
 *                   [--out f.ppm] [--dump-f32 f.raw] [--states-in f] [--states-out f] [--earth img] [--rtl] [--device K]
 *                   [--keys WASD..] [--mouse dx,dy]        the reference's interactive loop, scripted: one idle tick per frame
 *                   [--denoise] [--features-out PREFIX]   first-hit features + a-trous denoiser on the last frame (single GPU / host)
 *                   [--temporal] [--variance-out F]       temporal accumulation across frames with reprojection (single GPU / host)
 *                   [--svgf]                              variance-guided a-trous filter (SVGF) on the last frame (single GPU / host)
 *                   [--pick X,Y]                          no render: the closest-hit record under pixel (X, Y) as one JSON line
 *                   [--probe X,Y[,N]]                     no render: the path-traced colour along the ray through pixel (X, Y) as one JSON line
 *                   [--sh-probe X,Y,Z[,D[,N]]]            no render: the SH9 light probe at world position (X, Y, Z) as one JSON line
 *                   [--sh-volume X0,Y0,Z0,X1,Y1,Z1,NX,NY,NZ[,D[,N]]]   no render: an irradiance volume over the box, sampled at
 *                                                          --pick X,Y (one JSON line) or at every pixel (--irradiance-out FILE)
 *                   [--visibility BIAS[,MINVIS[,S]]]      with --sh-volume: depth maps per probe and the visibility-weighted sampler
 *                   [--cache-depth K]                     with --sh-volume: paths that end in the volume from bounce K on, along
 *                                                          --probe X,Y[,N] (one JSON line) or every pixel's ray (--radiance-out FILE)
 *                   [--cache-render]                      with --sh-volume and --cache-depth: the frames are cached frames, renders
 *                                                          whose paths end in the volume (single GPU / host)
 *                   [--refresh R[,H[,KR[,S]]]]            with --sh-volume: R rounds re-bake every probe through the volume and blend;
 *                                                          with --cache-render and S > 0 every S-th probe again before each frame
 *
 * --frames N re-renders like the reference's idle loop (mort.cu:93-120): RNG streams continue from frame to frame; before each
 * frame after the first, input() runs (mort.cu:49-91) with the frame's character of --keys held down ('.' = none) and the
 * --mouse delta dragged with the left button.  --out / --dump-f32 hold the last frame.
 * --denoise: after the last frame, the feature pass for its camera and the a-trous denoiser (default parameters) over its
 * accumulators; --out then holds the denoised image (--dump-f32 stays the raw render) and the JSON line gains "denoise_seconds".
 * --features-out P writes P.albedo.f32, P.normal.f32, P.depth.f32 (W*H*3 / *3 / *1 floats, row 0 = bottom row).
 * --temporal: after every frame, the feature pass for its camera and one temporal step (default parameters; the previous frame's
 * camera, none for frame 0); --out then holds the accumulated image of the last frame, --denoise filters the accumulated colour
 * with the last frame's features, --dump-f32 stays the raw render, and the JSON line gains "temporal_seconds" (features + temporal,
 * summed over frames).  --variance-out F writes the last step's variance estimate (W*H floats, -1 = unknown).
 * --svgf (not with --denoise): after the last frame, the feature pass for its camera and the SVGF filter stage (default parameters)
 * over its accumulators, the variance from the spatial estimate; with --temporal, over the accumulated colour with the last step's
 * features and its variance.  --out then holds the filtered image (--dump-f32 stays the raw render, --variance-out the temporal
 * step's variance) and the JSON line gains "svgf_seconds" (features + filter).
 * On a single GPU any of --temporal / --denoise / --svgf / --features-out / --variance-out / --dump-f32 sends every frame through a
 * view (mort_hip_view_frame): the chain stays on the device, one host wait per frame, only the uchar4 frame and the
 * files asked for come back.  With --temporal every frame goes through the view (and is filtered, as a viewer would; nothing of the
 * filter is fed back, so the files are the same); without it only the last frame does, the ones before are plain renders.  The
 * files and the JSON keys are those of the last frame as above, the seconds the device times of the stages (a still camera skips
 * the feature pass: "temporal_seconds" counts the passes that ran).
 *
 * --pick X,Y (single GPU / host; row 0 = bottom row, as every buffer): renders nothing; one closest-hit query (mort_hip_query_closest,
 * or mort_hip_query_closest_host under --mode host, which needs no GPU) for the feature pass's primary ray of that pixel -- lens
 * centre through the pixel centre, time 0.5, t_max = inf, no streams, so media are passed over -- printed as one JSON line:
 * pick, hit, t, p, normal, u, v, mat_type, mat_idx, front_face, medium, mode, seconds.  Floats are printed with nine significant
 * digits, which identify a float32; a non-finite one as NaN / Infinity / -Infinity.
 *
 * --probe X,Y[,N] (single GPU / host): renders nothing; one radiance query (mort_hip_query_radiance, or mort_hip_query_radiance_host
 * under --mode host) for the same ray as --pick: N paths (default 1) with the scene camera's bounce limit (--depth), background and
 * light object, drawn from subsequence X + Y * W of --seed, which is that pixel's stream at the start of a render.  One JSON line:
 * probe, samples, origin, dir, time, rgb (the unscaled sum of the N colours), mode, seconds.
 *
 * --sh-probe X,Y,Z[,D[,N]] (single GPU / host; excludes --pick and --probe): renders nothing; bakes one light probe
 * (mort_hip_probe_bake, or mort_hip_probe_bake_host under --mode host) at world position (X, Y, Z), time 0.5: D directions of the
 * library's own set (default 256), N paths per direction (default 1), the scene camera's bounce limit (--depth), background and
 * light object, the streams subsequences 0 .. D - 1 of --seed.  One JSON line: sh (9 x 3), directions, samples, position, mode,
 * seconds.
 *
 * --sh-volume X0,Y0,Z0,X1,Y1,Z1,NX,NY,NZ[,D[,N]] (single GPU / host; with --pick or --irradiance-out, excludes --probe and
 * --sh-probe): renders nothing; an irradiance volume of NX x NY x NZ probes that spans the box inclusively --
 * spacing (X1 - X0) / (NX - 1), an axis with one probe sits at X0 with spacing 1 -- baked at time 0.5 as --sh-probe bakes (D
 * directions, N paths, the scene camera's parameters; the streams are subsequences 0 .. probes D - 1 of --seed, probe-major),
 * packed with all weights 1.  With --pick X,Y: that pixel's closest-hit query, then the volume sampled at the hit's position and
 * normal; one JSON line, --pick's fields plus irradiance (3) and weight_sum, zeros for a miss.  With --irradiance-out FILE (and
 * without --pick): the same chain for every pixel's --pick ray, sqrt(clamp(E / pi, 0, 1)) as an 8-bit PPM, misses black.
 *
 * --visibility BIAS[,MINVIS[,S]] (with --sh-volume only): after the SH bake, one depth map per probe (DESIGN.md 4.18;
 * mort_hip_probe_depth_bake, or its _host form) with S x S rays per texel (default 2, 1..8) and
 * max_distance = (float)(1.5 sqrt(sx^2 + sy^2 + sz^2)) over the grid's spacing, computed in double; the volume is then sampled with
 * mort_hip_volume_sample_visible: normal_bias = BIAS (finite, >= 0), min_visibility = MINVIS (default 0.05, in 0..1).  --pick's JSON
 * line gains normal_bias, min_visibility, depth_subsamples and max_distance, --irradiance-out's the same.  Without the
 * option every byte of the output is what it was.
 *
 * --cache-depth K (with --sh-volume only, and then with --probe or --radiance-out instead of --pick / --irradiance-out): the
 * volume is baked as above (with --visibility its depth maps too) and used inside the path: a cached radiance
 * query (mort_hip_query_radiance_cached, or its _host form) with cache_depth = K in 0..MORT_MAX_BOUNCE_LIMIT and the scene
 * camera's parameters.  With --probe X,Y[,N]: --probe's ray, stream and N paths; one JSON line, --probe's fields plus
 * cache_depth, ends (how many of the N paths ended in the volume) and the volume's parameters.  With --radiance-out FILE: every
 * pixel's --pick ray gets N = --spp paths (default 1) from that pixel's stream (subsequence X + Y * W of --seed), and
 * sqrt(clamp(sum / N, 0, 1)), NaN as 0, is written as an 8-bit PPM.  That is a PREVIEW from pixel-centre rays (no jitter, no lens,
 * time 0.5), not a render.  Without --cache-depth every accepted and refused combination and every output byte is what it was.
 *
 * --cache-render (with --sh-volume ... --cache-depth K, --visibility optional; excludes --probe, --radiance-out, --pick and
 * --irradiance-out; one GPU in the default mode, or --mode host): the volume is baked as above, then the ordinary frame loop runs
 * -- --spp, --frames, --keys / --mouse, --out, --temporal, --denoise, --svgf, --features-out, --variance-out, --dump-f32 and the
 * states files as for a render -- with cached frames in the renders' place: on a GPU every frame goes through a
 * view with the cache attached (mort_hip_view_set_cache_host), under --mode host through mort_hip_render_cached_host.  The JSON line is
 * the render's own plus cache_depth, ends (the paths of the last frame that ended in the volume) and the volume's parameters.
 * Without --cache-render every accepted and refused combination and every output byte is what it was.
 *
 * --refresh R[,H[,KR[,S]]] (with --sh-volume only, under every use it has): after the bake (and the maps), R rounds of
 * mort_hip_volume_refresh (or its _host form) follow.  Round r = 1 .. R refreshes every probe (first 0, step 1)
 * with hysteresis H (default 0.9, 0 <= H < 1), refresh depth KR (default 0, in 0..MORT_MAX_BOUNCE_LIMIT), --sh-volume's D and N, and
 * the direction set mort_hip_probe_directions_round(D, r); the bake's streams are carried on and the records ping-pong between two
 * buffers.  With --cache-render and S > 0 (default 0; S > 0 needs --cache-render), before every frame f >= 1 one more round runs
 * over the probes first = f mod S, step = S with the set of round R + f, and the view takes the records by
 * mort_hip_view_update_cache_host (its history goes on).  The JSON line gains refresh_rounds, hysteresis, refresh_depth,
 * refresh_stride and refresh_ends (the paths of the last full round that ended in the volume; 0 for R = 0).  Without --refresh
 * every accepted and refused combination and every output byte is what it was.
 *
 * --cache-direct (with --sh-volume ... --cache-depth K and --probe or --radiance-out; excludes --cache-render and --refresh, whose
 * paths do not have the direct terminal: --refresh-direct is the refresh for this volume): the volume holds indirect light only and a path that ends in it adds one sampled shadow
 * segment toward the scene's light object.  After the bake a second, emission-only bake runs over the same probes
 * and directions from a copy of the streams the first one started from (bounce limit 1, black background, one path per direction),
 * the coefficients are subtracted float by float, packed, and the query is mort_hip_query_radiance_cached_direct (or its _host
 * form).  The JSON line gains cache_direct: 1 and lit (the paths whose shadow segment returned a non-zero emission), after ends.
 * Without --cache-direct every accepted and refused combination and every output byte is what it was.
 *
 * --cache-render-direct (with --sh-volume ... --cache-depth K, --visibility optional; excludes --cache-render, --cache-direct,
 * --refresh, --probe, --radiance-out, --pick and --irradiance-out; one GPU in the default mode, or --mode host): --cache-render with
 * direct cached frames in the cached frames' place.  The volume is composed as --cache-direct composes it (the bake
 * minus an emission-only bake from a copy of its streams), then the frame loop runs as under --cache-render: on a GPU through a view
 * with the direct cache attached (mort_hip_view_set_cache_direct_host), under --mode host through mort_hip_render_cached_direct_host.
 * The JSON line is --cache-render's plus cache_direct: 1 and lit (the last frame's paths whose shadow segment returned a non-zero
 * emission), after ends.  --refresh is refused: a refresh through plain cached paths would put the emitters' light back into a
 * volume that is to hold indirect light only; --refresh-direct is the refresh for this volume.  Without --cache-render-direct every accepted and refused combination and every
 * output byte is what it was.
 *
 * --refresh-direct R[,H[,KR[,S]]] (with --cache-direct or --cache-render-direct only; --refresh's grammar and defaults): --refresh
 * for the indirect-only volume of those two options, through mort_hip_volume_refresh_direct (or its _host form).
 * The rounds run over the indirect records (the full bake minus the emission-only bake); the full bake's streams are carried on, the
 * direction sets are rotated and the records ping-pong as under --refresh.  With --cache-direct S must be 0; with
 * --cache-render-direct and S > 0 every S-th probe is refreshed before each frame f >= 1 with the set of round R + f, and the view
 * takes the records by mort_hip_view_update_cache_host.  It is refused with --refresh, with --cache-render and without a direct
 * option; --refresh beside the direct options stays refused.  The JSON line gains --refresh's fields, then refresh_direct: 1 and
 * refresh_lit (the paths of the last full round whose shadow segment returned a non-zero emission).  Without --refresh-direct every
 * accepted and refused combination and every output byte is what it was.
 *
 * --gpus N: N - 1 ranks are forked BEFORE any HIP call (a process that has initialised the GPU must not fork or exec);
 * rank r renders row blocks r, r + N, ... on device r (or --devices) and the packed rows are gathered to rank 0 -- over
 * RCCL (`--gather rccl`, the default: xGMI inside a node), or through a shared host mapping (`--gather shm`: for ranks
 * that share one GPU, where RCCL refuses a communicator; used by the tests on a one-GPU box).
 */
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/prctl.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>

#include "mort_hip.h"
#include "mort_host.h"

/* ---- `--gpus N`: no rank may outlive a failed peer.  The frame gather is collective (rank 0 blocks in ncclRecv + a stream wait, the
 * peers in ncclSend), so a rank that fails takes the others down instead of leaving them waiting: a forked rank signals rank 0
 * (SIGUSR1), whose handler kills every rank and exits non-zero; rank 0 kills its ranks before it exits itself; and every forked rank
 * asks the kernel for SIGKILL when rank 0 dies for any other reason (PR_SET_PDEATHSIG). ---- */
static pid_t g_kids[64];
static int g_nkids = 0, g_rank = 0;
static void kill_ranks(void) { for (int r = 1; r <= g_nkids; r++) if (g_kids[r] > 0) kill(g_kids[r], SIGKILL); }
static void on_rank_failed(int sig) { (void)sig; kill_ranks(); static const char m[] = "a rank failed\n"; if (write(2, m, sizeof m - 1) < 0) { } _exit(EXIT_FAILURE); }
static void fail_exit(void) {
    if (g_rank == 0) kill_ranks();
    else kill(getppid(), SIGUSR1);
    exit(EXIT_FAILURE);
}
static void die(mort_ctx *ctx, int st, const char *what) {
    fprintf(stderr, "%s: %s %s\n", what, mort_hip_strerror(st), ctx ? mort_hip_last_error(ctx) : "");
    fail_exit();
}
static double now_s(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }

static int usage(void) {
    printf("Usage: mort <number_between_1_and_10> [--width W] [--aspect A] [--spp N] [--depth D] [--seed S] [--frames N] "
           "[--mode mega|wave|host|throughput] [--threads T] [--tree] [--gpus N] [--devices a,b,..] [--gather rccl|shm] "
           "[--out f.ppm] [--dump-f32 f.raw] [--states-in f] [--states-out f] [--earth image.jpg|.ppm] [--rtl] [--device K] [--keys WASD..] [--mouse dx,dy] "
           "[--denoise] [--features-out PREFIX] [--temporal] [--variance-out F] [--svgf] [--pick X,Y] [--probe X,Y[,N]] [--sh-probe X,Y,Z[,D[,N]]] "
           "[--sh-volume X0,Y0,Z0,X1,Y1,Z1,NX,NY,NZ[,D[,N]]] [--irradiance-out FILE] [--visibility BIAS[,MINVIS[,S]]] "
           "[--cache-depth K] [--radiance-out FILE] [--cache-render] [--refresh R[,H[,KR[,S]]]] [--cache-direct]\n"
           "            [--cache-render-direct] [--refresh-direct R[,H[,KR[,S]]]]\n"
           "  --cache-depth K with --sh-volume: paths end in the volume from bounce K on; --probe X,Y[,N] prints one pixel's colour,\n"
           "  --radiance-out FILE writes a preview from pixel-centre rays (--spp paths each; no jitter, no lens), not a render,\n"
           "  --cache-render renders: the ordinary frame loop (--frames, --out, --temporal, --svgf, ...) over cached frames\n"
           "  --refresh R[,H[,KR[,S]]] with --sh-volume: R rounds re-bake every probe through the volume (hysteresis H, refresh depth KR);\n"
           "  with --cache-render and S > 0 every S-th probe is refreshed again before each frame\n"
           "  --cache-direct with --cache-depth and --probe or --radiance-out: the volume keeps indirect light only and a path that\n"
           "  ends in it adds one sampled shadow ray toward the scene's light\n"
           "  --cache-render-direct with --sh-volume and --cache-depth: --cache-render over that indirect-only volume, the frames'\n"
           "  paths adding the sampled shadow ray where they end; excludes --cache-render, --cache-direct and --refresh\n"
           "  --refresh-direct R[,H[,KR[,S]]] with --cache-direct or --cache-render-direct: --refresh for their indirect-only volume,\n"
           "  the probes' paths adding the shadow ray and leaving out the emitters a probe sees directly; S > 0 only with\n"
           "  --cache-render-direct\n");
    return -1;
}

/* the reference loads "imgs/earthmap.jpg" relative to the working directory (mort.cu:296,599) */
static unsigned char *load_earth(const char *path, const char *argv0, int *w, int *h, char *used, size_t used_len) {
    if (path) { snprintf(used, used_len, "%s", path); return mort_read_image(path, w, h); }
    const char *cands[3] = {"imgs/earthmap.jpg", "tests/golden/earthmap.jpg", NULL};
    char rel[4096];
    for (int i = 0; i < 3; i++) {
        const char *p = cands[i];
        if (!p) { /* next to the binary: <repo>/mort_amd/bin/mort -> <repo>/tests/golden/earthmap.jpg */
            const char *slash = strrchr(argv0, '/');
            if (!slash) break;
            snprintf(rel, sizeof rel, "%.*s/../../tests/golden/earthmap.jpg", (int)(slash - argv0), argv0);
            p = rel;
        }
        unsigned char *t = mort_read_image(p, w, h);
        if (t) { snprintf(used, used_len, "%s", p); return t; }
    }
    snprintf(used, used_len, "imgs/earthmap.jpg");
    return NULL;
}

/* a float32 as JSON: nine significant digits, which identify it; NaN / Infinity / -Infinity as Python's json module reads and writes them */
static void print_f32(float v) {
    if (v != v) printf("NaN");
    else if (v - v != 0.0f) printf(v > 0 ? "Infinity" : "-Infinity");
    else { /* always with a fraction or an exponent, so that a reader keeps it a float: -0.0 stays negative */
        char b[32];
        snprintf(b, sizeof b, "%.9g", (double)v);
        printf("%s%s", b, strpbrk(b, ".e") ? "" : ".0");
    }
}
static void print_v3(const char *key, const float *v) {
    printf(", \"%s\": [", key);
    for (int k = 0; k < 3; k++) { if (k) printf(", "); print_f32(v[k]); }
    printf("]");
}

/* --pick: the feature pass's primary ray of pixel (x, y) (dev_features.h feat_pixel: lens centre through the pixel centre, time 0.5) */
static mort_ray pick_ray(const mort_camera *cam, int x, int y) {
    mort_ray r;
    for (int k = 0; k < 3; k++) {
        const float sample = (cam->pixel00_loc.e[k] + (float)x * cam->pixel_delta_u.e[k]) + (float)y * cam->pixel_delta_v.e[k];
        r.origin[k] = cam->center.e[k];
        r.dir[k] = sample - cam->center.e[k];
    }
    r.time = 0.5f;
    r.t_max = 1.0f / 0.0f;
    return r;
}

/* --sh-volume's grid: NX x NY x NZ probes that span the box inclusively, at time 0.5; -1 (and a message) where the library's own
 * conditions fail, before anything is sized by the counts */
static int volume_grid(const float box[6], const int n[3], mort_volume_grid *grid) {
    for (int k = 0; k < 3; k++) {
        grid->origin[k] = box[k];
        grid->count[k] = n[k];
        grid->spacing[k] = n[k] > 1 ? (box[3 + k] - box[k]) / (float)(n[k] - 1) : 1.0f;
    }
    grid->time = 0.5f;
    for (int k = 0; k < 3; k++)
        if (grid->count[k] < 1 || grid->count[k] > MORT_VOLUME_MAX_COUNT || !(grid->spacing[k] > 0.0f) || grid->spacing[k] - grid->spacing[k] != 0.0f ||
            grid->origin[k] - grid->origin[k] != 0.0f) { fprintf(stderr, "--sh-volume: a box with X1 > X0 (or one probe) per axis and 1..%d probes per axis\n", MORT_VOLUME_MAX_COUNT); return -1; }
    return 0;
}

/* --refresh R[,H[,KR[,S]]]: rounds of the volume refresh over a baked volume */
typedef struct {
    int on, rounds, depth, stride;
    float h;
    unsigned long long ends; /* the paths of the last full round that ended in the volume */
    int direct;              /* --refresh-direct: the direct refresh in the refresh's place */
    unsigned long long lit;  /* direct: of those paths, the ones whose shadow segment returned a non-zero emission */
} refresh_opts;

/* one round over the probes first, first + step, ... with the direction set of round `round`: from `in` into `out`, the streams
 * carried on; ctx NULL: the host form.  *ends_sum, *lit_sum (or NULL): the selected probes' counts (lit: of a direct refresh) */
static void refresh_round(mort_ctx *ctx, const mort_world *world, const mort_camera *cam, const refresh_opts *ro, const mort_volume_grid *grid,
                          uint32_t flags, const mort_volume_vis_params *vis, int sh_d, int sh_n, uint32_t round, uint32_t first, uint32_t step,
                          mort_rng_state *states, const float *in, const float *depth, float *out, int threads, int host_flags,
                          unsigned long long *ends_sum, unsigned long long *lit_sum) {
    const size_t n = (size_t)grid->count[0] * (size_t)grid->count[1] * (size_t)grid->count[2];
    const size_t m = first < n ? (n - 1 - first) / step + 1 : 0;
    mort_refresh_params rp;
    memset(&rp, 0, sizeof rp);
    mort_hip_radiance_params_from_camera(cam, &rp.cached.path);
    rp.cached.path.samples = sh_n;
    rp.cached.cache_depth = ro->depth; rp.cached.flags = flags; rp.cached.grid = *grid; rp.cached.vis = *vis;
    rp.directions = sh_d; rp.hysteresis = ro->h; rp.first = first; rp.step = step;
    float *dirs = (float *)malloc(3 * (size_t)sh_d * sizeof *dirs);
    uint32_t *ends = (uint32_t *)calloc(n, sizeof *ends);
    uint32_t *lit = ro->direct ? (uint32_t *)calloc(n, sizeof *lit) : NULL;
    if (!dirs || !ends || (ro->direct && !lit)) { fprintf(stderr, "out of memory\n"); fail_exit(); }
    int st;
    if ((st = mort_hip_probe_directions_round(sh_d, round, dirs)) != MORT_OK) die(NULL, st, "mort_hip_probe_directions_round");
    if (ro->direct) {
        if (!ctx) {
            if ((st = mort_hip_volume_refresh_direct_host(world, &rp, m, dirs, states, in, depth, threads, host_flags, out, ends, lit, NULL)) != MORT_OK) die(NULL, st, "mort_hip_volume_refresh_direct_host");
        } else if ((st = mort_hip_volume_refresh_direct(ctx, &rp, m, dirs, states, in, depth, out, ends, lit, NULL)) != MORT_OK) die(ctx, st, "mort_hip_volume_refresh_direct");
        if (lit_sum) { *lit_sum = 0; for (size_t i = 0; i < m; i++) *lit_sum += lit[first + i * step]; }
    } else if (!ctx) {
        if ((st = mort_hip_volume_refresh_host(world, &rp, m, dirs, states, in, depth, threads, host_flags, out, ends, NULL)) != MORT_OK) die(NULL, st, "mort_hip_volume_refresh_host");
    } else if ((st = mort_hip_volume_refresh(ctx, &rp, m, dirs, states, in, depth, out, ends, NULL)) != MORT_OK) die(ctx, st, "mort_hip_volume_refresh");
    if (ends_sum) { *ends_sum = 0; for (size_t i = 0; i < m; i++) *ends_sum += ends[first + i * step]; }
    free(dirs); free(ends); free(lit);
}

/* rounds 1 .. R over every probe; the records ping-pong between `a` (the bake's) and `b`: returns the one that holds the last round's */
static float *refresh_all(mort_ctx *ctx, const mort_world *world, const mort_camera *cam, refresh_opts *ro, const mort_volume_grid *grid, uint32_t flags,
                          const mort_volume_vis_params *vis, int sh_d, int sh_n, mort_rng_state *states, float *a, float *b, const float *depth,
                          int threads, int host_flags) {
    for (int r = 1; r <= ro->rounds; r++) {
        refresh_round(ctx, world, cam, ro, grid, flags, vis, sh_d, sh_n, (uint32_t)r, 0, 1, states, a, depth, b, threads, host_flags, &ro->ends, &ro->lit);
        float *t = a; a = b; b = t;
    }
    return a;
}

static void print_refresh(const refresh_opts *ro) {
    if (!ro->on) return;
    printf(", \"refresh_rounds\": %d, \"hysteresis\": ", ro->rounds); print_f32(ro->h);
    printf(", \"refresh_depth\": %d, \"refresh_stride\": %d, \"refresh_ends\": %llu", ro->depth, ro->stride, ro->ends);
    if (ro->direct) printf(", \"refresh_direct\": 1, \"refresh_lit\": %llu", ro->lit);
}

/* --cache-render: the volume a cached frame ends its paths in, baked as the no-render uses of --sh-volume bake it (D directions, N
 * paths, the scene camera's parameters, the streams subsequences 0 .. probes D - 1 of the seed; all weights 1; with --visibility
 * the depth maps, S x S rays per texel, max_distance 1.5 cell diagonals) */
typedef struct {
    mort_cached_frame_params p;
    mort_depth_params dp;
    float *records, *depth; /* host; depth NULL without --visibility */
    size_t probes;
    double bake_sec;
    float *back;            /* --refresh: the buffer the next round writes, and the bake's streams carried on; else NULL */
    mort_rng_state *states;
} cache_volume;
static void bake_cache_volume(cache_volume *v, mort_ctx *ctx /* NULL: the host forms */, const mort_world *world, const mort_camera *cam,
                              unsigned long long seed, int sh_d, int sh_n, int vis_s, int threads, int host_flags, refresh_opts *ro,
                              int direct /* --cache-render-direct: indirect light only, as --cache-direct composes it */) {
    const mort_volume_grid *g = &v->p.grid;
    const int visible = (v->p.flags & MORT_CACHED_VISIBLE) != 0;
    const size_t n = v->probes = (size_t)g->count[0] * (size_t)g->count[1] * (size_t)g->count[2];
    mort_probe_params pp;
    mort_hip_radiance_params_from_camera(cam, &pp.rp);
    pp.rp.samples = sh_n;
    pp.directions = sh_d;
    v->dp.subsamples = vis_s;
    v->dp.max_distance = (float)(1.5 * sqrt((double)g->spacing[0] * (double)g->spacing[0] + (double)g->spacing[1] * (double)g->spacing[1] +
                                            (double)g->spacing[2] * (double)g->spacing[2]));
    mort_probe *probes = (mort_probe *)malloc(n * sizeof *probes);
    mort_rng_state *states = (mort_rng_state *)malloc(n * (size_t)sh_d * sizeof *states);
    float *sh = (float *)malloc(n * MORT_SH9_FLOATS * sizeof *sh);
    v->records = (float *)malloc(n * MORT_VOLUME_RECORD_FLOATS * sizeof(float));
    v->depth = visible ? (float *)malloc(n * MORT_DEPTH_FLOATS * sizeof(float)) : NULL;
    if (!probes || !states || !sh || !v->records || (visible && !v->depth) || n * (size_t)sh_d > 0x7fffffffu) { fprintf(stderr, "out of memory\n"); fail_exit(); }
    int st;
    if ((st = mort_hip_volume_probes(g, probes)) != MORT_OK) die(NULL, st, "mort_hip_volume_probes");
    if ((st = mort_hip_rng_seed_host(seed, (int)(n * (size_t)sh_d), 1, states)) != MORT_OK) die(NULL, st, "mort_hip_rng_seed_host");
    if (direct) { /* the full bake minus the emission-only bake (bounce limit 1, black background, one path) from a copy of the streams */
        mort_probe_params pe = pp;
        pe.rp.bounce_limit = 1; pe.rp.samples = 1;
        pe.rp.background[0] = pe.rp.background[1] = pe.rp.background[2] = 0.0f;
        mort_rng_state *states_e = (mort_rng_state *)malloc(n * (size_t)sh_d * sizeof *states_e);
        float *sh_e = (float *)malloc(n * MORT_SH9_FLOATS * sizeof *sh_e);
        if (!states_e || !sh_e) { fprintf(stderr, "out of memory\n"); fail_exit(); }
        memcpy(states_e, states, n * (size_t)sh_d * sizeof *states_e);
        double emit_sec = 0;
        if (!ctx) {
            if ((st = mort_hip_probe_bake_host(world, &pp, n, probes, NULL, states, threads, host_flags, sh, &v->bake_sec)) != MORT_OK) die(NULL, st, "mort_hip_probe_bake_host");
            if ((st = mort_hip_probe_bake_host(world, &pe, n, probes, NULL, states_e, threads, host_flags, sh_e, &emit_sec)) != MORT_OK) die(NULL, st, "mort_hip_probe_bake_host");
        } else {
            if ((st = mort_hip_probe_bake(ctx, &pp, n, probes, NULL, states, sh, &v->bake_sec)) != MORT_OK) die(ctx, st, "mort_hip_probe_bake");
            if ((st = mort_hip_probe_bake(ctx, &pe, n, probes, NULL, states_e, sh_e, &emit_sec)) != MORT_OK) die(ctx, st, "mort_hip_probe_bake");
        }
        for (size_t i = 0; i < n * MORT_SH9_FLOATS; i++) sh[i] = sh[i] - sh_e[i];
        v->bake_sec += emit_sec;
        free(states_e); free(sh_e);
    }
    if (!ctx) {
        if (!direct && (st = mort_hip_probe_bake_host(world, &pp, n, probes, NULL, states, threads, host_flags, sh, &v->bake_sec)) != MORT_OK) die(NULL, st, "mort_hip_probe_bake_host");
        if ((st = mort_hip_volume_pack_host(n, sh, NULL, threads, v->records, NULL)) != MORT_OK) die(NULL, st, "mort_hip_volume_pack_host");
        if (visible && (st = mort_hip_probe_depth_bake_host(world, &v->dp, n, probes, threads, host_flags, v->depth, NULL)) != MORT_OK) die(NULL, st, "mort_hip_probe_depth_bake_host");
    } else {
        if (!direct && (st = mort_hip_probe_bake(ctx, &pp, n, probes, NULL, states, sh, &v->bake_sec)) != MORT_OK) die(ctx, st, "mort_hip_probe_bake");
        if ((st = mort_hip_volume_pack(ctx, n, sh, NULL, v->records, NULL)) != MORT_OK) die(ctx, st, "mort_hip_volume_pack");
        if (visible && (st = mort_hip_probe_depth_bake(ctx, &v->dp, n, probes, v->depth, NULL)) != MORT_OK) die(ctx, st, "mort_hip_probe_depth_bake");
    }
    free(probes); free(sh);
    if (!ro->on) { free(states); return; }
    v->states = states;
    float *second = (float *)malloc(n * MORT_VOLUME_RECORD_FLOATS * sizeof(float));
    if (!second) { fprintf(stderr, "out of memory\n"); fail_exit(); }
    float *now = refresh_all(ctx, world, cam, ro, g, v->p.flags, &v->p.vis, sh_d, sh_n, states, v->records, second, v->depth, threads, host_flags);
    v->back = now == v->records ? second : v->records;
    v->records = now;
}

/* --refresh ...,S with --cache-render, before frame f >= 1: the probes f mod S, f mod S + S, ... once more, into the back buffer (which
 * first takes the other records as they stand), and the buffers change places */
static void refresh_before_frame(cache_volume *v, mort_ctx *ctx, const mort_world *world, const mort_camera *cam, const refresh_opts *ro, int sh_d,
                                 int sh_n, int f, int threads, int host_flags) {
    memcpy(v->back, v->records, v->probes * MORT_VOLUME_RECORD_FLOATS * sizeof(float));
    refresh_round(ctx, world, cam, ro, &v->p.grid, v->p.flags, &v->p.vis, sh_d, sh_n, (uint32_t)(ro->rounds + f), (uint32_t)(f % ro->stride),
                  (uint32_t)ro->stride, v->states, v->records, v->depth, v->back, threads, host_flags, NULL, NULL);
    float *t = v->records; v->records = v->back; v->back = t;
}

/* input() before frame f (mort.cu:49-91,94): the f-th character of --keys held down, the --mouse delta dragged */
static void frame_input(mort_camera *cam, const char *keys, int f, int mdx, int mdy) {
    int k = 0;
    if (keys && (size_t)(f - 1) < strlen(keys)) {
        const char ch = keys[f - 1];
        k = (ch == 'W' || ch == 'w') ? MORT_KEY_W : (ch == 'S' || ch == 's') ? MORT_KEY_S : (ch == 'A' || ch == 'a') ? MORT_KEY_A : (ch == 'D' || ch == 'd') ? MORT_KEY_D : 0;
    }
    if (k || mdx || mdy) mort_camera_input(cam, k, mdx, mdy, (mdx || mdy) ? 1 : 0);
}

int main(int argc, char **argv) {
    if (argc < 2) return usage();
    int scene = atoi(argv[1]);
    int width = 0, spp = 0, depth = -1, frames = 1, device = 0, rtl = 0, mode = MORT_MODE_MEGA, host_mode = 0, threads = 1, tree = 0;
    int gpus = 1, gather_shm = 0, devices[64], n_devices = 0;
    double aspect = 0;
    unsigned long long seed = MORT_DEFAULT_SEED;
    const char *out = NULL, *dump = NULL, *sin = NULL, *sout = NULL, *earth = NULL, *keys = NULL, *feat_out = NULL, *var_out = NULL;
    int denoise = 0, temporal = 0, svgf = 0;
    int mouse_dx = 0, mouse_dy = 0;
    int pick = 0, pick_x = 0, pick_y = 0;
    int probe = 0, probe_x = 0, probe_y = 0, probe_n = 1;
    int sh_probe = 0, sh_d = 256, sh_n = 1;
    float sh_pos[3] = {0, 0, 0};
    int sh_volume = 0, vol_n[3] = {0, 0, 0};
    float vol_box[6] = {0, 0, 0, 0, 0, 0};
    const char *irr_out = NULL;
    int visibility = 0, vis_s = 2;
    float vis_bias = 0.0f, vis_min = 0.05f;
    int cached = 0, cache_depth = 0;
    const char *rad_out = NULL;
    int cache_render = 0;
    int cache_direct = 0;
    int cache_render_direct = 0; /* --cache-render-direct: sets cache_render too, once its own refusals are through */
    refresh_opts refresh, refresh_direct; /* --refresh-direct: takes --refresh's place once both options' refusals are through */
    memset(&refresh, 0, sizeof refresh);
    refresh.h = 0.9f;
    refresh_direct = refresh;
    for (int i = 2; i < argc; i++) {
#define ARG(name) (strcmp(argv[i], name) == 0 && i + 1 < argc)
        if (ARG("--width")) width = atoi(argv[++i]);
        else if (ARG("--aspect")) aspect = atof(argv[++i]);
        else if (ARG("--spp")) spp = atoi(argv[++i]);
        else if (ARG("--depth")) depth = atoi(argv[++i]);
        else if (ARG("--seed")) seed = strtoull(argv[++i], NULL, 10);
        else if (ARG("--out")) out = argv[++i];
        else if (ARG("--dump-f32")) dump = argv[++i];
        else if (ARG("--states-in")) sin = argv[++i];
        else if (ARG("--states-out")) sout = argv[++i];
        else if (ARG("--earth")) earth = argv[++i];
        else if (ARG("--frames")) frames = atoi(argv[++i]);
        else if (ARG("--keys")) keys = argv[++i];
        else if (ARG("--mouse")) { if (sscanf(argv[++i], "%d,%d", &mouse_dx, &mouse_dy) != 2) { fprintf(stderr, "--mouse dx,dy\n"); return -1; } }
        else if (ARG("--device")) device = atoi(argv[++i]);
        else if (ARG("--threads")) threads = atoi(argv[++i]);
        else if (ARG("--gpus")) gpus = atoi(argv[++i]);
        else if (ARG("--devices")) {
            char *s = argv[++i];
            for (char *tok = strtok(s, ","); tok && n_devices < 64; tok = strtok(NULL, ",")) devices[n_devices++] = atoi(tok);
        }
        else if (ARG("--gather")) { const char *g = argv[++i]; if (strcmp(g, "shm") == 0) gather_shm = 1; else if (strcmp(g, "rccl") != 0) { fprintf(stderr, "unknown gather %s\n", g); return -1; } }
        else if (ARG("--mode")) {
            const char *m = argv[++i];
            if (strcmp(m, "wave") == 0) mode = MORT_MODE_WAVE;
            else if (strcmp(m, "throughput") == 0) mode = MORT_MODE_THROUGHPUT; /* non-parity: own streams per (pixel, stratum row) */
            else if (strcmp(m, "host") == 0) host_mode = 1;
            else if (strcmp(m, "mega") != 0) { fprintf(stderr, "unknown mode %s\n", m); return -1; }
        }
        else if (strcmp(argv[i], "--rtl") == 0) rtl = 1;
        else if (strcmp(argv[i], "--tree") == 0) tree = 1;
        else if (strcmp(argv[i], "--denoise") == 0) denoise = 1;
        else if (ARG("--features-out")) feat_out = argv[++i];
        else if (strcmp(argv[i], "--temporal") == 0) temporal = 1;
        else if (ARG("--variance-out")) var_out = argv[++i];
        else if (strcmp(argv[i], "--svgf") == 0) svgf = 1;
        else if (ARG("--pick")) { pick = 1; if (sscanf(argv[++i], "%d,%d", &pick_x, &pick_y) != 2) { fprintf(stderr, "--pick X,Y\n"); return -1; } }
        else if (ARG("--probe")) { probe = 1; if (sscanf(argv[++i], "%d,%d,%d", &probe_x, &probe_y, &probe_n) < 2 || probe_n < 1) { fprintf(stderr, "--probe X,Y[,N]\n"); return -1; } }
        else if (ARG("--sh-probe")) {
            sh_probe = 1;
            if (sscanf(argv[++i], "%f,%f,%f,%d,%d", &sh_pos[0], &sh_pos[1], &sh_pos[2], &sh_d, &sh_n) < 3 || sh_n < 1) { fprintf(stderr, "--sh-probe X,Y,Z[,D[,N]]\n"); return -1; }
        }
        else if (ARG("--sh-volume")) {
            sh_volume = 1;
            if (sscanf(argv[++i], "%f,%f,%f,%f,%f,%f,%d,%d,%d,%d,%d", &vol_box[0], &vol_box[1], &vol_box[2], &vol_box[3], &vol_box[4], &vol_box[5],
                       &vol_n[0], &vol_n[1], &vol_n[2], &sh_d, &sh_n) < 9 || sh_n < 1) { fprintf(stderr, "--sh-volume X0,Y0,Z0,X1,Y1,Z1,NX,NY,NZ[,D[,N]]\n"); return -1; }
        }
        else if (ARG("--irradiance-out")) irr_out = argv[++i];
        else if (ARG("--visibility")) {
            visibility = 1;
            if (sscanf(argv[++i], "%f,%f,%d", &vis_bias, &vis_min, &vis_s) < 1) { fprintf(stderr, "--visibility BIAS[,MINVIS[,S]]\n"); return -1; }
        }
        else if (ARG("--cache-depth")) { cached = 1; if (sscanf(argv[++i], "%d", &cache_depth) != 1) { fprintf(stderr, "--cache-depth K\n"); return -1; } }
        else if (ARG("--radiance-out")) rad_out = argv[++i];
        else if (strcmp(argv[i], "--cache-render") == 0) cache_render = 1;
        else if (strcmp(argv[i], "--cache-direct") == 0) cache_direct = 1;
        else if (strcmp(argv[i], "--cache-render-direct") == 0) cache_render_direct = 1;
        else if (ARG("--refresh-direct")) {
            refresh_direct.on = refresh_direct.direct = 1;
            if (sscanf(argv[++i], "%d,%f,%d,%d", &refresh_direct.rounds, &refresh_direct.h, &refresh_direct.depth, &refresh_direct.stride) < 1) { fprintf(stderr, "--refresh-direct R[,H[,KR[,S]]]\n"); return -1; }
        }
        else if (ARG("--refresh")) {
            refresh.on = 1;
            if (sscanf(argv[++i], "%d,%f,%d,%d", &refresh.rounds, &refresh.h, &refresh.depth, &refresh.stride) < 1) { fprintf(stderr, "--refresh R[,H[,KR[,S]]]\n"); return -1; }
        }
        else { fprintf(stderr, "unknown option %s\n", argv[i]); return usage(); }
    }
    if (gpus < 1 || gpus > 64 || frames < 1 || threads < 1) { fprintf(stderr, "bad --gpus / --frames / --threads\n"); return -1; }
    if (host_mode && gpus != 1) { fprintf(stderr, "--mode host runs on the host: --gpus does not apply\n"); return -1; }
    if (gpus > 1 && (dump || sin || sout)) { fprintf(stderr, "--dump-f32 / --states-in / --states-out are single-GPU options\n"); return -1; }
    if (gpus > 1 && (denoise || feat_out)) { fprintf(stderr, "--denoise / --features-out are single-GPU options\n"); return -1; }
    if (gpus > 1 && (temporal || var_out)) { fprintf(stderr, "--temporal / --variance-out are single-GPU options\n"); return -1; }
    if (gpus > 1 && svgf) { fprintf(stderr, "--svgf is a single-GPU option\n"); return -1; }
    if (svgf && denoise) { fprintf(stderr, "--svgf and --denoise exclude each other\n"); return -1; }
    if (var_out && !temporal) { fprintf(stderr, "--variance-out needs --temporal\n"); return -1; }
    if (pick && gpus > 1) { fprintf(stderr, "--pick is a single-GPU option\n"); return -1; }
    if (probe && (gpus > 1 || pick)) { fprintf(stderr, "--probe is a single-GPU option and excludes --pick\n"); return -1; }
    if (sh_probe && (gpus > 1 || pick || probe)) { fprintf(stderr, "--sh-probe is a single-GPU option and excludes --pick and --probe\n"); return -1; }
    if (sh_probe && (sh_d < 64 || sh_d > 4096 || sh_d % 64)) { fprintf(stderr, "--sh-probe: D is a multiple of 64 in 64..4096\n"); return -1; }
    if (cached && !sh_volume) { fprintf(stderr, "--cache-depth needs --sh-volume\n"); return -1; }
    if (rad_out && !cached) { fprintf(stderr, "--radiance-out needs --cache-depth\n"); return -1; }
    if (cached && (cache_depth < 0 || cache_depth > MORT_MAX_BOUNCE_LIMIT)) { fprintf(stderr, "--cache-depth: K in 0..%d\n", MORT_MAX_BOUNCE_LIMIT); return -1; }
    if (refresh_direct.on) {
        if (refresh.on) { fprintf(stderr, "--refresh-direct excludes --refresh: the one is for an indirect-only volume, the other for a full one\n"); return -1; }
        if (cache_render) { fprintf(stderr, "--refresh-direct excludes --cache-render: its volume holds the emitters' light, --refresh is the option for it\n"); return -1; }
        if (!cache_direct && !cache_render_direct) { fprintf(stderr, "--refresh-direct needs --cache-direct or --cache-render-direct\n"); return -1; }
        if (refresh_direct.rounds < 0 || refresh_direct.rounds > 65535 || !(refresh_direct.h >= 0.0f) || !(refresh_direct.h < 1.0f) || refresh_direct.depth < 0 ||
            refresh_direct.depth > MORT_MAX_BOUNCE_LIMIT || refresh_direct.stride < 0 || (refresh_direct.stride > 0 && !cache_render_direct)) {
            fprintf(stderr, "--refresh-direct: R in 0..65535, H in [0, 1), KR in 0..%d, S >= 0 and S > 0 only with --cache-render-direct\n", MORT_MAX_BOUNCE_LIMIT); return -1;
        }
    }
    if (cache_render_direct) {
        if (cache_render || cache_direct) { fprintf(stderr, "--cache-render-direct excludes --cache-render and --cache-direct\n"); return -1; }
        if (!sh_volume || !cached) { fprintf(stderr, "--cache-render-direct needs --sh-volume and --cache-depth\n"); return -1; }
        if (probe || rad_out || pick || irr_out) { fprintf(stderr, "--cache-render-direct excludes --probe, --radiance-out, --pick and --irradiance-out\n"); return -1; }
        if (gpus > 1 || mode != MORT_MODE_MEGA) { fprintf(stderr, "--cache-render-direct is a single-GPU option of the default mode and of --mode host\n"); return -1; }
        if (refresh.on) {
            fprintf(stderr, "--cache-render-direct excludes --refresh: a refresh through plain cached paths would put the emitters' light back into the indirect volume\n");
            return -1;
        }
        cache_render = 1; /* from here on: --cache-render with another volume and another frame call */
    }
    if (cache_direct && !cached) { fprintf(stderr, "--cache-direct needs --cache-depth\n"); return -1; }
    if (cache_direct && (cache_render || refresh.on)) { fprintf(stderr, "--cache-direct excludes --cache-render and --refresh\n"); return -1; }
    if (cache_render && (!sh_volume || !cached)) { fprintf(stderr, "--cache-render needs --sh-volume and --cache-depth\n"); return -1; }
    if (cache_render && (probe || rad_out || pick || irr_out)) { fprintf(stderr, "--cache-render excludes --probe, --radiance-out, --pick and --irradiance-out\n"); return -1; }
    if (cache_render && (gpus > 1 || mode != MORT_MODE_MEGA)) { fprintf(stderr, "--cache-render is a single-GPU option of the default mode and of --mode host\n"); return -1; }
    if (cached && !cache_render && (pick || irr_out || !probe == !rad_out)) {
        fprintf(stderr, "--cache-depth needs --probe X,Y[,N] or --radiance-out FILE, not both, and excludes --pick and --irradiance-out\n"); return -1;
    }
    if (sh_volume && (gpus > 1 || (probe && !cached) || sh_probe)) { fprintf(stderr, "--sh-volume is a single-GPU option and excludes --probe and --sh-probe\n"); return -1; }
    if (sh_volume && (sh_d < 64 || sh_d > 4096 || sh_d % 64)) { fprintf(stderr, "--sh-volume: D is a multiple of 64 in 64..4096\n"); return -1; }
    if (sh_volume && !cached && !pick == !irr_out) { fprintf(stderr, "--sh-volume needs --pick X,Y or --irradiance-out FILE, not both\n"); return -1; }
    if (visibility && !sh_volume) { fprintf(stderr, "--visibility needs --sh-volume\n"); return -1; }
    if (visibility && (!(vis_bias >= 0.0f) || vis_bias - vis_bias != 0.0f || !(vis_min >= 0.0f) || !(vis_min <= 1.0f) || vis_s < 1 || vis_s > MORT_DEPTH_RES)) {
        fprintf(stderr, "--visibility: BIAS finite and >= 0, MINVIS in 0..1, S in 1..%d\n", MORT_DEPTH_RES); return -1;
    }
    if (irr_out && !sh_volume) { fprintf(stderr, "--irradiance-out needs --sh-volume\n"); return -1; }
    if (refresh.on && !sh_volume) { fprintf(stderr, "--refresh needs --sh-volume\n"); return -1; }
    if (refresh.on && (refresh.rounds < 0 || refresh.rounds > 65535 || !(refresh.h >= 0.0f) || !(refresh.h < 1.0f) || refresh.depth < 0 ||
                       refresh.depth > MORT_MAX_BOUNCE_LIMIT || refresh.stride < 0 || (refresh.stride > 0 && !cache_render))) {
        fprintf(stderr, "--refresh: R in 0..65535, H in [0, 1), KR in 0..%d, S >= 0 and S > 0 only with --cache-render\n", MORT_MAX_BOUNCE_LIMIT); return -1;
    }
    if (refresh_direct.on) refresh = refresh_direct; /* from here on: --refresh with another refresh call */
    if (n_devices && n_devices != gpus) { fprintf(stderr, "--devices needs %d entries\n", gpus); return -1; }

    mort_world world;
    mort_camera cam;
    if (mort_world_init(&world) != 0) { fprintf(stderr, "out of memory\n"); return EXIT_FAILURE; }
    mort_scene_opts opts;
    memset(&opts, 0, sizeof opts);
    opts.args_rtl = rtl;
    unsigned char *texels = NULL;
    if (scene == 3 || scene == 8 || scene == 9) {
        char used[4096];
        texels = load_earth(earth, argv[0], &opts.earth_width, &opts.earth_height, used, sizeof used);
        if (!texels) { /* img_loader.h:33 prints this and renders the missing-texture colour; a batch render of the wrong picture helps nobody */
            fprintf(stderr, "ERROR: Could not load image file '%s'.\n", used);
            return EXIT_FAILURE;
        }
        opts.earth_texels = texels;
    }
    mort_scene_build(scene, &world, &cam, &opts);
    if (width > 0) cam.image_width = width;
    if (aspect > 0) cam.aspect_ratio = (float)aspect;
    if (spp > 0) cam.samples_per_pixel = spp;
    if (depth >= 0) cam.bounce_limit = depth;
    mort_camera_initialize(&cam);
    const int W = cam.image_width, H = cam.image_height;
    const size_t npx = (size_t)W * H;
    const int eff = mort_camera_effective_spp(&cam);

    if (sh_volume && !cache_render) { /* ---- no render: bake a grid of probes, pack it, sample it at the hits of --pick's rays ---- */
        if (pick && (pick_x < 0 || pick_x >= W || pick_y < 0 || pick_y >= H)) { fprintf(stderr, "--pick %d,%d is outside the %dx%d image\n", pick_x, pick_y, W, H); return -1; }
        if (probe && (probe_x < 0 || probe_x >= W || probe_y < 0 || probe_y >= H)) { fprintf(stderr, "--probe %d,%d is outside the %dx%d image\n", probe_x, probe_y, W, H); return -1; }
        mort_volume_grid grid;
        int pst;
        if (volume_grid(vol_box, vol_n, &grid) != 0) return -1;
        const size_t probes_n = (size_t)grid.count[0] * (size_t)grid.count[1] * (size_t)grid.count[2];
        const size_t nq = (pick || probe) ? 1 : npx;
        mort_probe_params pp;
        mort_hip_radiance_params_from_camera(&cam, &pp.rp);
        pp.rp.samples = sh_n;
        pp.directions = sh_d;
        mort_probe *probes = (mort_probe *)malloc(probes_n * sizeof *probes);
        mort_rng_state *states = (mort_rng_state *)malloc(probes_n * (size_t)sh_d * sizeof *states); /* subsequences 0 .. probes D - 1, probe-major */
        float *sh = (float *)malloc(probes_n * MORT_SH9_FLOATS * sizeof *sh);
        float *records = (float *)malloc(probes_n * MORT_VOLUME_RECORD_FLOATS * sizeof *records);
        float *records2 = refresh.on ? (float *)malloc(probes_n * MORT_VOLUME_RECORD_FLOATS * sizeof *records2) : NULL; /* --refresh: the other buffer */
        float *volume = records; /* the records that are sampled: the bake's, or the last round's */
        mort_ray *rays = (mort_ray *)malloc(nq * sizeof *rays);
        mort_hit *hits = (mort_hit *)malloc(nq * sizeof *hits);
        float *irr = (float *)malloc(nq * 4 * sizeof *irr);
        float *depth = visibility ? (float *)malloc(probes_n * MORT_DEPTH_FLOATS * sizeof *depth) : NULL;
        mort_depth_params dp;
        dp.subsamples = vis_s;
        dp.max_distance = (float)(1.5 * sqrt((double)grid.spacing[0] * (double)grid.spacing[0] + (double)grid.spacing[1] * (double)grid.spacing[1] +
                                             (double)grid.spacing[2] * (double)grid.spacing[2]));
        mort_volume_vis_params vp;
        vp.normal_bias = vis_bias; vp.min_visibility = vis_min;
        if ((visibility && !depth) || (refresh.on && !records2)) { fprintf(stderr, "out of memory\n"); return EXIT_FAILURE; }
        if (!probes || !states || !sh || !records || !rays || !hits || !irr || probes_n * (size_t)sh_d > 0x7fffffffu) { fprintf(stderr, "out of memory\n"); return EXIT_FAILURE; }
        if ((pst = mort_hip_volume_probes(&grid, probes)) != MORT_OK) die(NULL, pst, "mort_hip_volume_probes");
        if ((pst = mort_hip_rng_seed_host(seed, (int)(probes_n * (size_t)sh_d), 1, states)) != MORT_OK) die(NULL, pst, "mort_hip_rng_seed_host");
        /* --cache-depth: the volume inside the path.  The query's parameters, one pixel stream per ray, the colours and the counts */
        mort_cached_params cp;
        memset(&cp, 0, sizeof cp);
        mort_hip_radiance_params_from_camera(&cam, &cp.path);
        cp.path.samples = probe ? probe_n : (spp > 0 ? spp : 1);
        cp.cache_depth = cache_depth; cp.flags = visibility ? MORT_CACHED_VISIBLE : 0u; cp.grid = grid; cp.vis = vp;
        mort_rng_state *qstates = NULL;
        float *rgb = NULL;
        uint32_t *ends = NULL;
        /* --cache-direct: the emission-only bake's parameters, the streams the bake starts from, its coefficients, the lit counts */
        mort_probe_params pe = pp;
        pe.rp.bounce_limit = 1; pe.rp.samples = 1;
        pe.rp.background[0] = pe.rp.background[1] = pe.rp.background[2] = 0.0f;
        mort_rng_state *states_e = NULL;
        float *sh_e = NULL;
        uint32_t *lit = NULL;
        double emit_sec = 0;
        if (cache_direct) {
            states_e = (mort_rng_state *)malloc(probes_n * (size_t)sh_d * sizeof *states_e);
            sh_e = (float *)malloc(probes_n * MORT_SH9_FLOATS * sizeof *sh_e);
            lit = (uint32_t *)malloc(nq * sizeof *lit);
            if (!states_e || !sh_e || !lit) { fprintf(stderr, "out of memory\n"); return EXIT_FAILURE; }
            memcpy(states_e, states, probes_n * (size_t)sh_d * sizeof *states_e);
        }
        if (cached) {
            mort_rng_state *pixels = (mort_rng_state *)malloc(npx * sizeof *pixels); /* the run's pixel streams */
            qstates = (mort_rng_state *)malloc(nq * sizeof *qstates);
            rgb = (float *)malloc(nq * 3 * sizeof *rgb);
            ends = (uint32_t *)malloc(nq * sizeof *ends);
            if (!pixels || !qstates || !rgb || !ends) { fprintf(stderr, "out of memory\n"); return EXIT_FAILURE; }
            if ((pst = mort_hip_rng_seed_host(seed, W, H, pixels)) != MORT_OK) die(NULL, pst, "mort_hip_rng_seed_host");
            if (probe) qstates[0] = pixels[(size_t)probe_x + (size_t)probe_y * W];
            else memcpy(qstates, pixels, npx * sizeof *pixels);
            free(pixels);
        }
        if (pick) rays[0] = pick_ray(&cam, pick_x, pick_y);
        else if (probe) rays[0] = pick_ray(&cam, probe_x, probe_y);
        else for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) rays[(size_t)y * W + x] = pick_ray(&cam, x, y);
        double sec = 0, bake_sec = 0, sample_sec = 0;
        if (host_mode) {
            const int fl = tree ? MORT_HOST_TREE : 0;
            if ((pst = mort_hip_probe_bake_host(&world, &pp, probes_n, probes, NULL, states, threads, fl, sh, &bake_sec)) != MORT_OK) die(NULL, pst, "mort_hip_probe_bake_host");
            if (cache_direct) { /* the volume keeps indirect light: the full bake minus the emission-only bake, float by float */
                if ((pst = mort_hip_probe_bake_host(&world, &pe, probes_n, probes, NULL, states_e, threads, fl, sh_e, &emit_sec)) != MORT_OK) die(NULL, pst, "mort_hip_probe_bake_host");
                for (size_t i = 0; i < probes_n * MORT_SH9_FLOATS; i++) sh[i] = sh[i] - sh_e[i];
                bake_sec += emit_sec;
            }
            if ((pst = mort_hip_volume_pack_host(probes_n, sh, NULL, threads, records, NULL)) != MORT_OK) die(NULL, pst, "mort_hip_volume_pack_host");
            if (!cached && (pst = mort_hip_query_closest_host(&world, nq, rays, NULL, threads, fl, hits, &sec)) != MORT_OK) die(NULL, pst, "mort_hip_query_closest_host");
            if (visibility && (pst = mort_hip_probe_depth_bake_host(&world, &dp, probes_n, probes, threads, fl, depth, NULL)) != MORT_OK) die(NULL, pst, "mort_hip_probe_depth_bake_host");
            if (refresh.on) volume = refresh_all(NULL, &world, &cam, &refresh, &grid, cp.flags, &vp, sh_d, sh_n, states, records, records2, depth, threads, fl);
            if (cache_direct) {
                if ((pst = mort_hip_query_radiance_cached_direct_host(&world, &cp, nq, rays, qstates, volume, depth, threads, fl, rgb, ends, lit, &sec)) != MORT_OK) die(NULL, pst, "mort_hip_query_radiance_cached_direct_host");
            } else if (cached) {
                if ((pst = mort_hip_query_radiance_cached_host(&world, &cp, nq, rays, qstates, volume, depth, threads, fl, rgb, ends, &sec)) != MORT_OK) die(NULL, pst, "mort_hip_query_radiance_cached_host");
            } else if (visibility) {
                if ((pst = mort_hip_volume_sample_visible_host(&grid, volume, depth, &vp, nq, hits, sizeof *hits, threads, irr, &sample_sec)) != MORT_OK) die(NULL, pst, "mort_hip_volume_sample_visible_host");
            } else
            if ((pst = mort_hip_volume_sample_host(&grid, volume, nq, hits, sizeof *hits, threads, irr, &sample_sec)) != MORT_OK) die(NULL, pst, "mort_hip_volume_sample_host");
        } else {
            mort_ctx *pctx = NULL;
            if ((pst = mort_hip_init(device, &pctx)) != MORT_OK) die(NULL, pst, "mort_hip_init");
            if ((pst = mort_hip_upload_world(pctx, &world)) != MORT_OK) die(pctx, pst, "mort_hip_upload_world");
            if ((pst = mort_hip_probe_bake(pctx, &pp, probes_n, probes, NULL, states, sh, &bake_sec)) != MORT_OK) die(pctx, pst, "mort_hip_probe_bake");
            if (cache_direct) {
                if ((pst = mort_hip_probe_bake(pctx, &pe, probes_n, probes, NULL, states_e, sh_e, &emit_sec)) != MORT_OK) die(pctx, pst, "mort_hip_probe_bake");
                for (size_t i = 0; i < probes_n * MORT_SH9_FLOATS; i++) sh[i] = sh[i] - sh_e[i];
                bake_sec += emit_sec;
            }
            if ((pst = mort_hip_volume_pack(pctx, probes_n, sh, NULL, records, NULL)) != MORT_OK) die(pctx, pst, "mort_hip_volume_pack");
            if (!cached && (pst = mort_hip_query_closest(pctx, nq, rays, NULL, hits, &sec)) != MORT_OK) die(pctx, pst, "mort_hip_query_closest");
            if (visibility && (pst = mort_hip_probe_depth_bake(pctx, &dp, probes_n, probes, depth, NULL)) != MORT_OK) die(pctx, pst, "mort_hip_probe_depth_bake");
            if (refresh.on) volume = refresh_all(pctx, &world, &cam, &refresh, &grid, cp.flags, &vp, sh_d, sh_n, states, records, records2, depth, threads, 0);
            if (cache_direct) {
                if ((pst = mort_hip_query_radiance_cached_direct(pctx, &cp, nq, rays, qstates, volume, depth, rgb, ends, lit, &sec)) != MORT_OK) die(pctx, pst, "mort_hip_query_radiance_cached_direct");
            } else if (cached) {
                if ((pst = mort_hip_query_radiance_cached(pctx, &cp, nq, rays, qstates, volume, depth, rgb, ends, &sec)) != MORT_OK) die(pctx, pst, "mort_hip_query_radiance_cached");
            } else if (visibility) {
                if ((pst = mort_hip_volume_sample_visible(pctx, &grid, volume, depth, &vp, nq, hits, sizeof *hits, irr, &sample_sec)) != MORT_OK) die(pctx, pst, "mort_hip_volume_sample_visible");
            } else
            if ((pst = mort_hip_volume_sample(pctx, &grid, volume, nq, hits, sizeof *hits, irr, &sample_sec)) != MORT_OK) die(pctx, pst, "mort_hip_volume_sample");
            mort_hip_shutdown(pctx);
        }
        if (cached) {
            if (probe) {
                printf("{\"scene\": %d, \"width\": %d, \"height\": %d, \"probe\": [%d, %d], \"samples\": %d", scene, W, H, probe_x, probe_y, probe_n);
                print_v3("origin", rays[0].origin); print_v3("dir", rays[0].dir);
                printf(", \"time\": "); print_f32(rays[0].time);
                print_v3("rgb", rgb);
                printf(", \"cache_depth\": %d, \"ends\": %u", cache_depth, (unsigned)ends[0]);
                if (cache_direct) printf(", \"cache_direct\": 1, \"lit\": %u", (unsigned)lit[0]);
            } else {
                uint8_t *img = (uint8_t *)malloc(npx * 4);
                if (!img) { fprintf(stderr, "out of memory\n"); return EXIT_FAILURE; }
                const float paths = (float)cp.path.samples;
                unsigned long long ended = 0;
                for (size_t i = 0; i < npx; i++) {
                    for (int ch = 0; ch < 3; ch++) {
                        float v = rgb[3 * i + ch] / paths;
                        v = (v > 0.0f) ? v : 0.0f; /* NaN goes to 0 */
                        v = (v < 1.0f) ? v : 1.0f;
                        img[4 * i + ch] = (uint8_t)(255.0f * sqrtf(v) + 0.5f);
                    }
                    img[4 * i + 3] = 255;
                    ended += ends[i];
                }
                if (mort_write_ppm(rad_out, img, W, H) != 0) { fprintf(stderr, "cannot write %s\n", rad_out); return EXIT_FAILURE; }
                free(img);
                printf("{\"scene\": %d, \"width\": %d, \"height\": %d, \"radiance_out\": \"%s\", \"samples\": %d, \"cache_depth\": %d, \"ends\": %llu", scene, W, H,
                       rad_out, cp.path.samples, cache_depth, ended);
                if (cache_direct) {
                    unsigned long long lit_paths = 0;
                    for (size_t i = 0; i < npx; i++) lit_paths += lit[i];
                    printf(", \"cache_direct\": 1, \"lit\": %llu", lit_paths);
                }
            }
            if (visibility) {
                printf(", \"normal_bias\": "); print_f32(vp.normal_bias);
                printf(", \"min_visibility\": "); print_f32(vp.min_visibility);
                printf(", \"depth_subsamples\": %d, \"max_distance\": ", dp.subsamples); print_f32(dp.max_distance);
            }
            print_refresh(&refresh);
            printf(", \"probes\": [%d, %d, %d], \"directions\": %d, \"probe_samples\": %d, \"mode\": \"%s\", \"seconds\": %.6f, \"bake_seconds\": %.6f}\n",
                   (int)grid.count[0], (int)grid.count[1], (int)grid.count[2], sh_d, sh_n, host_mode ? "host" : "mega", sec, bake_sec);
            free(qstates); free(rgb); free(ends); free(states_e); free(sh_e); free(lit);
        } else {
        for (size_t i = 0; i < nq; i++) /* a miss is an all-zero record: its sample means nothing */
            if (!(hits[i].flags & MORT_HIT_HIT)) irr[4 * i] = irr[4 * i + 1] = irr[4 * i + 2] = irr[4 * i + 3] = 0.0f;
        if (pick) {
            const mort_hit h = hits[0];
            printf("{\"scene\": %d, \"width\": %d, \"height\": %d, \"pick\": [%d, %d], \"hit\": %d, \"t\": ", scene, W, H, pick_x, pick_y, (h.flags & MORT_HIT_HIT) ? 1 : 0);
            print_f32(h.t);
            print_v3("p", h.p); print_v3("normal", h.normal);
            printf(", \"u\": "); print_f32(h.u);
            printf(", \"v\": "); print_f32(h.v);
            printf(", \"mat_type\": %d, \"mat_idx\": %d, \"front_face\": %d, \"medium\": %d", (int)h.mat_type, (int)h.mat_idx,
                   (h.flags & MORT_HIT_FRONT_FACE) ? 1 : 0, (h.flags & MORT_HIT_MEDIUM) ? 1 : 0);
            print_v3("irradiance", irr);
            printf(", \"weight_sum\": "); print_f32(irr[3]);
            if (visibility) {
                printf(", \"normal_bias\": "); print_f32(vp.normal_bias);
                printf(", \"min_visibility\": "); print_f32(vp.min_visibility);
                printf(", \"depth_subsamples\": %d, \"max_distance\": ", dp.subsamples); print_f32(dp.max_distance);
            }
            print_refresh(&refresh);
            printf(", \"probes\": [%d, %d, %d], \"directions\": %d, \"samples\": %d, \"mode\": \"%s\", \"seconds\": %.6f, \"bake_seconds\": %.6f, \"sample_seconds\": %.6f}\n",
                   (int)grid.count[0], (int)grid.count[1], (int)grid.count[2], sh_d, sh_n, host_mode ? "host" : "mega", sec, bake_sec, sample_sec);
        } else {
            uint8_t *img = (uint8_t *)malloc(npx * 4);
            if (!img) { fprintf(stderr, "out of memory\n"); return EXIT_FAILURE; }
            const float inv_pi = 0.318309886f;
            for (size_t i = 0; i < npx; i++) {
                for (int ch = 0; ch < 3; ch++) {
                    float v = irr[4 * i + ch] * inv_pi;
                    v = (v > 0.0f) ? v : 0.0f; /* NaN goes to 0 */
                    v = (v < 1.0f) ? v : 1.0f;
                    img[4 * i + ch] = (uint8_t)(255.0f * sqrtf(v) + 0.5f);
                }
                img[4 * i + 3] = 255;
            }
            if (mort_write_ppm(irr_out, img, W, H) != 0) { fprintf(stderr, "cannot write %s\n", irr_out); return EXIT_FAILURE; }
            free(img);
            printf("{\"scene\": %d, \"width\": %d, \"height\": %d, \"irradiance_out\": \"%s\", \"probes\": [%d, %d, %d], \"directions\": %d, \"samples\": %d, "
                   "\"mode\": \"%s\", \"seconds\": %.6f, \"bake_seconds\": %.6f, \"sample_seconds\": %.6f", scene, W, H, irr_out, (int)grid.count[0], (int)grid.count[1],
                   (int)grid.count[2], sh_d, sh_n, host_mode ? "host" : "mega", sec, bake_sec, sample_sec);
            if (visibility) {
                printf(", \"normal_bias\": "); print_f32(vp.normal_bias);
                printf(", \"min_visibility\": "); print_f32(vp.min_visibility);
                printf(", \"depth_subsamples\": %d, \"max_distance\": ", dp.subsamples); print_f32(dp.max_distance);
            }
            print_refresh(&refresh);
            printf("}\n");
        }
        }
        free(probes); free(states); free(sh); free(records); free(records2); free(rays); free(hits); free(irr); free(depth);
        mort_world_free(&world);
        free(texels);
        return 0;
    }

    if (pick) { /* ---- no render: one closest-hit query ---- */
        if (pick_x < 0 || pick_x >= W || pick_y < 0 || pick_y >= H) { fprintf(stderr, "--pick %d,%d is outside the %dx%d image\n", pick_x, pick_y, W, H); return -1; }
        const mort_ray ray = pick_ray(&cam, pick_x, pick_y);
        mort_hit h;
        double sec = 0;
        int pst;
        if (host_mode) {
            if ((pst = mort_hip_query_closest_host(&world, 1, &ray, NULL, 1, tree ? MORT_HOST_TREE : 0, &h, &sec)) != MORT_OK) die(NULL, pst, "mort_hip_query_closest_host");
        } else {
            mort_ctx *pctx = NULL;
            if ((pst = mort_hip_init(device, &pctx)) != MORT_OK) die(NULL, pst, "mort_hip_init");
            if ((pst = mort_hip_upload_world(pctx, &world)) != MORT_OK) die(pctx, pst, "mort_hip_upload_world");
            if ((pst = mort_hip_query_closest(pctx, 1, &ray, NULL, &h, &sec)) != MORT_OK) die(pctx, pst, "mort_hip_query_closest");
            mort_hip_shutdown(pctx);
        }
        printf("{\"scene\": %d, \"width\": %d, \"height\": %d, \"pick\": [%d, %d], \"hit\": %d, \"t\": ", scene, W, H, pick_x, pick_y, (h.flags & MORT_HIT_HIT) ? 1 : 0);
        print_f32(h.t);
        print_v3("p", h.p); print_v3("normal", h.normal);
        printf(", \"u\": "); print_f32(h.u);
        printf(", \"v\": "); print_f32(h.v);
        printf(", \"mat_type\": %d, \"mat_idx\": %d, \"front_face\": %d, \"medium\": %d, \"mode\": \"%s\", \"seconds\": %.6f}\n", (int)h.mat_type, (int)h.mat_idx,
               (h.flags & MORT_HIT_FRONT_FACE) ? 1 : 0, (h.flags & MORT_HIT_MEDIUM) ? 1 : 0, host_mode ? "host" : "mega", sec);
        mort_world_free(&world);
        free(texels);
        return 0;
    }

    if (probe) { /* ---- no render: one radiance query ---- */
        if (probe_x < 0 || probe_x >= W || probe_y < 0 || probe_y >= H) { fprintf(stderr, "--probe %d,%d is outside the %dx%d image\n", probe_x, probe_y, W, H); return -1; }
        const mort_ray ray = pick_ray(&cam, probe_x, probe_y);
        mort_radiance_params rp;
        mort_hip_radiance_params_from_camera(&cam, &rp);
        rp.samples = probe_n;
        mort_rng_state *states = (mort_rng_state *)malloc(npx * sizeof *states); /* the run's pixel streams; the probe takes its pixel's */
        if (!states) { fprintf(stderr, "out of memory\n"); return EXIT_FAILURE; }
        int pst;
        if ((pst = mort_hip_rng_seed_host(seed, W, H, states)) != MORT_OK) die(NULL, pst, "mort_hip_rng_seed_host");
        mort_rng_state stream = states[(size_t)probe_x + (size_t)probe_y * W];
        free(states);
        float rgb[3] = {0, 0, 0};
        double sec = 0;
        if (host_mode) {
            if ((pst = mort_hip_query_radiance_host(&world, &rp, 1, &ray, &stream, 1, tree ? MORT_HOST_TREE : 0, rgb, &sec)) != MORT_OK) die(NULL, pst, "mort_hip_query_radiance_host");
        } else {
            mort_ctx *pctx = NULL;
            if ((pst = mort_hip_init(device, &pctx)) != MORT_OK) die(NULL, pst, "mort_hip_init");
            if ((pst = mort_hip_upload_world(pctx, &world)) != MORT_OK) die(pctx, pst, "mort_hip_upload_world");
            if ((pst = mort_hip_query_radiance(pctx, &rp, 1, &ray, &stream, rgb, &sec)) != MORT_OK) die(pctx, pst, "mort_hip_query_radiance");
            mort_hip_shutdown(pctx);
        }
        printf("{\"scene\": %d, \"width\": %d, \"height\": %d, \"probe\": [%d, %d], \"samples\": %d", scene, W, H, probe_x, probe_y, probe_n);
        print_v3("origin", ray.origin); print_v3("dir", ray.dir);
        printf(", \"time\": "); print_f32(ray.time);
        print_v3("rgb", rgb);
        printf(", \"mode\": \"%s\", \"seconds\": %.6f}\n", host_mode ? "host" : "mega", sec);
        mort_world_free(&world);
        free(texels);
        return 0;
    }

    if (sh_probe) { /* ---- no render: one light probe ---- */
        mort_probe_params pp;
        mort_hip_radiance_params_from_camera(&cam, &pp.rp);
        pp.rp.samples = sh_n;
        pp.directions = sh_d;
        mort_probe pr;
        for (int k = 0; k < 3; k++) pr.position[k] = sh_pos[k];
        pr.time = 0.5f;
        mort_rng_state *states = (mort_rng_state *)malloc((size_t)sh_d * sizeof *states); /* subsequences 0 .. D - 1 of the seed */
        if (!states) { fprintf(stderr, "out of memory\n"); return EXIT_FAILURE; }
        int pst;
        if ((pst = mort_hip_rng_seed_host(seed, sh_d, 1, states)) != MORT_OK) die(NULL, pst, "mort_hip_rng_seed_host");
        float sh[MORT_SH9_FLOATS];
        double sec = 0;
        if (host_mode) {
            if ((pst = mort_hip_probe_bake_host(&world, &pp, 1, &pr, NULL, states, threads, tree ? MORT_HOST_TREE : 0, sh, &sec)) != MORT_OK) die(NULL, pst, "mort_hip_probe_bake_host");
        } else {
            mort_ctx *pctx = NULL;
            if ((pst = mort_hip_init(device, &pctx)) != MORT_OK) die(NULL, pst, "mort_hip_init");
            if ((pst = mort_hip_upload_world(pctx, &world)) != MORT_OK) die(pctx, pst, "mort_hip_upload_world");
            if ((pst = mort_hip_probe_bake(pctx, &pp, 1, &pr, NULL, states, sh, &sec)) != MORT_OK) die(pctx, pst, "mort_hip_probe_bake");
            mort_hip_shutdown(pctx);
        }
        free(states);
        printf("{\"scene\": %d, \"sh\": [", scene);
        for (int k = 0; k < 9; k++) {
            printf("%s[", k ? ", " : "");
            for (int ch = 0; ch < 3; ch++) { if (ch) printf(", "); print_f32(sh[k * 3 + ch]); }
            printf("]");
        }
        printf("], \"directions\": %d, \"samples\": %d", sh_d, sh_n);
        print_v3("position", pr.position);
        printf(", \"mode\": \"%s\", \"seconds\": %.6f}\n", host_mode ? "host" : "mega", sec);
        mort_world_free(&world);
        free(texels);
        return 0;
    }

    /* ---- ranks: fork before anything touches the GPU ---- */
    int rank = 0;
    int id_pipe[64][2];
    pid_t kids[64];
    uint8_t *shm = NULL; /* --gather shm: rank r writes its rows of the full frame here */
    if (gpus > 1) {
        if (gather_shm) {
            shm = mmap(NULL, npx * 4, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
            if (shm == MAP_FAILED) { perror("mmap"); return EXIT_FAILURE; }
        }
        for (int r = 1; r < gpus; r++) if (pipe(id_pipe[r]) != 0) { perror("pipe"); return EXIT_FAILURE; }
        signal(SIGUSR1, on_rank_failed);
        const pid_t parent = getpid();
        for (int r = 1; r < gpus; r++) {
            pid_t p = fork();
            if (p < 0) { perror("fork"); kill_ranks(); return EXIT_FAILURE; }
            if (p == 0) {
                rank = g_rank = r; g_nkids = 0;
                signal(SIGUSR1, SIG_DFL);
                prctl(PR_SET_PDEATHSIG, SIGKILL);
                if (getppid() != parent) _exit(EXIT_FAILURE); /* rank 0 died before the request took effect */
                break;
            }
            kids[r] = g_kids[r] = p; g_nkids = r;
        }
        device = n_devices ? devices[rank] : rank;
        /* test hooks for the failure path (tests/test_cli.py; no GPU needed): MORT_TEST_FAIL_RANK=r makes rank r fail here,
         * MORT_TEST_BLOCK_RANK0=1 makes rank 0 wait as it would inside the gather */
        const char *tf = getenv("MORT_TEST_FAIL_RANK");
        if (tf && atoi(tf) == rank) { if (rank > 0) usleep(200000); fprintf(stderr, "rank %d: MORT_TEST_FAIL_RANK\n", rank); fail_exit(); }
        if (tf && rank == 0 && getenv("MORT_TEST_BLOCK_RANK0")) { sleep(60); fprintf(stderr, "rank 0 was not taken down by the failed rank\n"); kill_ranks(); return 3; }
        if (tf && rank != 0) { sleep(60); _exit(3); } /* a healthy peer that would wait in ncclSend: must be killed, not waited for */
    }

    cache_volume cv; /* --cache-render */
    memset(&cv, 0, sizeof cv);
    uint32_t *ends_px = NULL, *lit_px = NULL;
    if (cache_render) {
        cv.p.cache_depth = cache_depth; cv.p.flags = visibility ? MORT_CACHED_VISIBLE : 0u;
        cv.p.vis.normal_bias = vis_bias; cv.p.vis.min_visibility = vis_min;
        if (volume_grid(vol_box, vol_n, &cv.p.grid) != 0) return -1;
        ends_px = calloc(npx, sizeof *ends_px);
        lit_px = cache_render_direct ? calloc(npx, sizeof *lit_px) : NULL;
        if (!ends_px || (cache_render_direct && !lit_px)) { fprintf(stderr, "out of memory\n"); return EXIT_FAILURE; }
    }

    uint8_t *rgba = calloc(npx, 4);
    /* a single GPU keeps the chain on the device (a view): only --dump-f32 brings the accumulators back */
    const int use_view = !host_mode && gpus == 1 && (temporal || denoise || svgf || feat_out || dump || cache_render);
    const int want_accum = dump || (host_mode && (denoise || temporal || svgf));
    float *accum = want_accum ? calloc(npx * 3, sizeof(float)) : NULL;
    if (!rgba || (want_accum && !accum)) { fprintf(stderr, "out of memory\n"); fail_exit(); }
    /* --temporal: this frame's features (albedo unused), the ping-ponged history, the accumulated colour and the variance */
    float *alb = NULL, *nrm = NULL, *dep = NULL, *hist[2] = {NULL, NULL}, *tacc = NULL, *tvar = NULL;
    mort_camera prev_cam;
    mort_temporal_params tp;
    mort_hip_temporal_defaults(&tp);
    double temporal_sec = 0;
    if (temporal && host_mode) {
        alb = malloc(npx * 3 * sizeof(float)); nrm = malloc(npx * 3 * sizeof(float)); dep = malloc(npx * sizeof(float));
        tacc = malloc(npx * 3 * sizeof(float)); tvar = malloc(npx * sizeof(float));
        for (int k = 0; k < 2; k++) hist[k] = aligned_alloc(16, npx * MORT_TEMPORAL_HISTORY_FLOATS * sizeof(float));
        if (!alb || !nrm || !dep || !tacc || !tvar || !hist[0] || !hist[1]) { fprintf(stderr, "out of memory\n"); fail_exit(); }
    }
    mort_stats stats;
    memset(&stats, 0, sizeof stats);
    double total_ms = 0, frame_wall = 0;
    mort_ctx *ctx = NULL;
    mort_view *view = NULL;
    mort_rng_state *hstates = NULL;
    double denoise_sec = 0, svgf_sec = 0, view_feat_sec = 0;
    int st;

    if (host_mode) { /* ---- the kernel body as a host loop: no GPU ---- */
        hstates = malloc(npx * sizeof *hstates);
        if (!hstates) { fprintf(stderr, "out of memory\n"); return EXIT_FAILURE; }
        if (sin) {
            FILE *f = fopen(sin, "rb");
            if (!f || fread(hstates, sizeof *hstates, npx, f) != npx) { fprintf(stderr, "cannot read %zu states from %s\n", npx, sin); return EXIT_FAILURE; }
            fclose(f);
        } else if ((st = mort_hip_rng_seed_host(seed, W, H, hstates)) != MORT_OK) die(NULL, st, "mort_hip_rng_seed_host");
        if (cache_render) bake_cache_volume(&cv, NULL, &world, &cam, seed, sh_d, sh_n, vis_s, threads, tree ? MORT_HOST_TREE : 0, &refresh, cache_render_direct);
        for (int f = 0; f < frames; f++) {
            if (f > 0) frame_input(&cam, keys, f, mouse_dx, mouse_dy);
            if (f > 0 && cache_render && refresh.stride > 0) refresh_before_frame(&cv, NULL, &world, &cam, &refresh, sh_d, sh_n, f, threads, tree ? MORT_HOST_TREE : 0);
            if (cache_render_direct) {
                if ((st = mort_hip_render_cached_direct_host(&world, &cam, hstates, threads, tree ? MORT_HOST_TREE : 0, &cv.p, cv.records, cv.depth, rgba, accum,
                                                             NULL, ends_px, lit_px, &stats)) != MORT_OK) die(NULL, st, "mort_hip_render_cached_direct_host");
            } else if (cache_render) {
                if ((st = mort_hip_render_cached_host(&world, &cam, hstates, threads, tree ? MORT_HOST_TREE : 0, &cv.p, cv.records, cv.depth, rgba, accum, NULL,
                                                      ends_px, &stats)) != MORT_OK) die(NULL, st, "mort_hip_render_cached_host");
            } else
            if ((st = mort_hip_render_host(&world, &cam, hstates, threads, tree ? MORT_HOST_TREE : 0, rgba, accum, NULL, &stats)) != MORT_OK) die(NULL, st, "mort_hip_render_host");
            total_ms += stats.seconds * 1e3;
            printf("Avg. time per frame: %3.1f ms\n", total_ms / (f + 1)); /* mort.cu:119 */
            if (temporal) {
                double fs = 0, ts = 0;
                if ((st = mort_hip_render_features_host(&world, &cam, threads, tree ? MORT_HOST_TREE : 0, alb, nrm, dep, &fs)) != MORT_OK) die(NULL, st, "mort_hip_render_features_host");
                if ((st = mort_hip_temporal_host(&tp, f ? &prev_cam : NULL, &cam, W, H, threads, accum, nrm, dep, f ? hist[(f + 1) & 1] : NULL, hist[f & 1],
                                                 tacc, tvar, rgba, &ts)) != MORT_OK) die(NULL, st, "mort_hip_temporal_host");
                temporal_sec += fs + ts;
                prev_cam = cam;
            }
        }
        frame_wall = stats.seconds;
    } else {
        st = mort_hip_init(device, &ctx);
        if (st != MORT_OK) die(NULL, st, "mort_hip_init");
        if (gpus > 1) {
            mort_partition part = {rank, gpus, 8};
            if ((st = mort_hip_set_partition(ctx, &part)) != MORT_OK) die(ctx, st, "mort_hip_set_partition");
            if (!gather_shm) { /* rank 0 makes the RCCL id, the others read it from their pipe */
                unsigned char id[MORT_COMM_ID_BYTES];
                if (rank == 0) {
                    if ((st = mort_hip_comm_id(id)) != MORT_OK) die(ctx, st, "mort_hip_comm_id");
                    for (int r = 1; r < gpus; r++) if (write(id_pipe[r][1], id, sizeof id) != (ssize_t)sizeof id) { perror("write"); fail_exit(); }
                } else if (read(id_pipe[rank][0], id, sizeof id) != (ssize_t)sizeof id) { perror("read"); fail_exit(); }
                if ((st = mort_hip_comm_init(ctx, id, rank, gpus)) != MORT_OK) die(ctx, st, "mort_hip_comm_init");
            }
        }
        if ((st = mort_hip_upload_world(ctx, &world)) != MORT_OK) die(ctx, st, "mort_hip_upload_world");
        if (sin) {
            mort_rng_state *s = malloc(npx * sizeof *s);
            FILE *f = fopen(sin, "rb");
            if (!s || !f || fread(s, sizeof *s, npx, f) != npx) { fprintf(stderr, "cannot read %zu states from %s\n", npx, sin); fail_exit(); }
            fclose(f);
            if ((st = mort_hip_rng_load(ctx, s, W, H)) != MORT_OK) die(ctx, st, "mort_hip_rng_load");
            free(s);
        } else if ((st = mort_hip_rng_seed(ctx, seed, W, H)) != MORT_OK) die(ctx, st, "mort_hip_rng_seed");

        if (use_view) {
            mort_view_params vp;
            mort_hip_view_defaults(&vp);
            vp.width = W; vp.height = H;
            vp.temporal = temporal;
            vp.filter = denoise ? MORT_VIEW_FILTER_DENOISE : svgf ? MORT_VIEW_FILTER_SVGF : MORT_VIEW_FILTER_NONE;
            if ((st = mort_hip_view_create(ctx, &vp, &view)) != MORT_OK) die(ctx, st, "mort_hip_view_create");
        }
        if (cache_render) { /* the volume baked on this context; the view keeps its own device copies of the records and maps */
            bake_cache_volume(&cv, ctx, &world, &cam, seed, sh_d, sh_n, vis_s, threads, 0, &refresh, cache_render_direct);
            if (cache_render_direct) {
                if ((st = mort_hip_view_set_cache_direct_host(view, &cv.p, cv.records, cv.depth)) != MORT_OK) die(ctx, st, "mort_hip_view_set_cache_direct_host");
            } else
            if ((st = mort_hip_view_set_cache_host(view, &cv.p, cv.records, cv.depth)) != MORT_OK) die(ctx, st, "mort_hip_view_set_cache_host");
        }
        for (int f = 0; f < frames; f++) {
            if (f > 0) frame_input(&cam, keys, f, mouse_dx, mouse_dy);
            if (f > 0 && cache_render && refresh.stride > 0) { /* some probes once more; the view takes the records and keeps its history */
                refresh_before_frame(&cv, ctx, &world, &cam, &refresh, sh_d, sh_n, f, threads, 0);
                if ((st = mort_hip_view_update_cache_host(view, cv.records, cv.depth)) != MORT_OK) die(ctx, st, "mort_hip_view_update_cache_host");
            }
            const double t0 = now_s();
            if (view && (temporal || cache_render || f == frames - 1)) { /* render, features, temporal step and filter on the device; the frame's uchar4
                                                          * comes back.  Without --temporal only the last frame is filtered or written:
                                                          * the frames before it are plain renders, as they always were */
                mort_view_stats vs;
                if ((st = mort_hip_view_frame(view, &cam, mode, rgba, &vs)) != MORT_OK) die(ctx, st, "mort_hip_view_frame");
                stats = vs.render;
                if (temporal) temporal_sec += vs.features_seconds + vs.temporal_seconds;
                /* feature pass + filter of the last frame, as before: under a still camera the pass that made the features in use
                 * is an earlier frame's; with --temporal it is counted there */
                if (!vs.features_reused) view_feat_sec = vs.features_seconds;
                denoise_sec = svgf_sec = (temporal ? 0 : view_feat_sec) + vs.filter_seconds;
            } else if (view) {
                if ((st = mort_hip_render(ctx, &cam, mode, rgba, NULL, NULL, &stats)) != MORT_OK) die(ctx, st, "mort_hip_render");
            } else if (gpus > 1 && !gather_shm) {
                if ((st = mort_hip_render_gather(ctx, &cam, mode, rank == 0 ? rgba : NULL, &stats)) != MORT_OK) die(ctx, st, "mort_hip_render_gather");
            } else {
                if ((st = mort_hip_render(ctx, &cam, mode, rgba, accum, NULL, &stats)) != MORT_OK) die(ctx, st, "mort_hip_render");
                if (gpus > 1) { /* --gather shm: owned rows into the shared frame */
                    const int lr = mort_hip_local_rows(ctx, H);
                    for (int ly = 0; ly < lr; ly++) { const int y = mort_hip_global_row(ctx, ly); memcpy(shm + (size_t)y * W * 4, rgba + (size_t)y * W * 4, (size_t)W * 4); }
                }
            }
            frame_wall = now_s() - t0;
            total_ms += stats.seconds * 1e3;
            if (rank == 0) printf("Avg. time per frame: %3.1f ms\n", total_ms / (f + 1)); /* mort.cu:119 */
        }
        if (view) { /* what the files need of the last frame */
            if (cache_render && (st = mort_hip_view_read(view, MORT_VIEW_ENDS, ends_px)) != MORT_OK) die(ctx, st, "mort_hip_view_read");
            if (cache_render_direct && (st = mort_hip_view_read(view, MORT_VIEW_LIT, lit_px)) != MORT_OK) die(ctx, st, "mort_hip_view_read");
            if (dump && (st = mort_hip_view_read(view, MORT_VIEW_RAW_ACCUM, accum)) != MORT_OK) die(ctx, st, "mort_hip_view_read");
            if (feat_out) {
                alb = malloc(npx * 3 * sizeof(float)); nrm = malloc(npx * 3 * sizeof(float)); dep = malloc(npx * sizeof(float));
                if (!alb || !nrm || !dep) { fprintf(stderr, "out of memory\n"); fail_exit(); }
                if ((st = mort_hip_view_read(view, MORT_VIEW_ALBEDO, alb)) != MORT_OK || (st = mort_hip_view_read(view, MORT_VIEW_NORMAL, nrm)) != MORT_OK ||
                    (st = mort_hip_view_read(view, MORT_VIEW_DEPTH, dep)) != MORT_OK) die(ctx, st, "mort_hip_view_read");
            }
            if (var_out) {
                tvar = malloc(npx * sizeof(float));
                if (!tvar) { fprintf(stderr, "out of memory\n"); fail_exit(); }
                if ((st = mort_hip_view_read(view, MORT_VIEW_VARIANCE, tvar)) != MORT_OK) die(ctx, st, "mort_hip_view_read");
            }
            mort_hip_view_destroy(view);
        }
    }

    /* ---- --denoise / --svgf / --features-out: the last frame's camera; the PPM becomes the filtered image.  With --temporal the
     * features are the last step's and the filter takes the accumulated colour (--svgf: and its variance).  On the GPU the view
     * has done all of this; what follows computes for --mode host only ---- */
    if (denoise || svgf || feat_out) {
        if (host_mode && !temporal) {
            alb = malloc(npx * 3 * sizeof(float)); nrm = malloc(npx * 3 * sizeof(float)); dep = malloc(npx * sizeof(float));
            if (!alb || !nrm || !dep) { fprintf(stderr, "out of memory\n"); fail_exit(); }
        }
        double fs = 0, ds = 0;
        if (host_mode && !temporal) { /* with --temporal: the last step's */
            if ((st = mort_hip_render_features_host(&world, &cam, threads, tree ? MORT_HOST_TREE : 0, alb, nrm, dep, &fs)) != MORT_OK) die(NULL, st, "mort_hip_render_features_host");
        }
        if (host_mode && denoise) {
            const float *col = temporal ? tacc : accum;
            mort_denoise_params dp;
            mort_hip_denoise_defaults(&dp);
            if ((st = mort_hip_denoise_host(&dp, W, H, threads, col, alb, nrm, dep, NULL, rgba, &ds)) != MORT_OK) die(NULL, st, "mort_hip_denoise_host");
            denoise_sec = fs + ds;
        }
        if (host_mode && svgf) {
            const float *col = temporal ? tacc : accum;
            mort_svgf_params sp;
            mort_hip_svgf_defaults(&sp);
            if ((st = mort_hip_svgf_host(&sp, W, H, threads, col, alb, nrm, dep, tvar, NULL, NULL, rgba, &ds)) != MORT_OK) die(NULL, st, "mort_hip_svgf_host");
            svgf_sec = fs + ds;
        }
        if (feat_out) {
            const char *suffix[3] = {"albedo", "normal", "depth"};
            const float *buf[3] = {alb, nrm, dep};
            const size_t cnt[3] = {npx * 3, npx * 3, npx};
            for (int k = 0; k < 3; k++) {
                char path[4096];
                snprintf(path, sizeof path, "%s.%s.f32", feat_out, suffix[k]);
                FILE *f = fopen(path, "wb");
                if (!f || fwrite(buf[k], sizeof(float), cnt[k], f) != cnt[k]) { fprintf(stderr, "cannot write %s\n", path); return EXIT_FAILURE; }
                fclose(f);
            }
        }
    }
    if (var_out) {
        FILE *f = fopen(var_out, "wb");
        if (!f || fwrite(tvar, sizeof(float), npx, f) != npx) { fprintf(stderr, "cannot write %s\n", var_out); return EXIT_FAILURE; }
        fclose(f);
    }
    free(alb); free(nrm); free(dep); free(tacc); free(tvar); free(hist[0]); free(hist[1]);

    /* ---- ranks other than 0 are done; rank 0 waits for them (their rows are in shm / were gathered) ---- */
    if (rank != 0) {
        if (ctx) mort_hip_shutdown(ctx);
        _exit(0);
    }
    int failed = 0;
    for (int r = 1; r < gpus; r++) { int ws = 0; if (waitpid(kids[r], &ws, 0) < 0 || !WIFEXITED(ws) || WEXITSTATUS(ws) != 0) failed = 1; }
    if (failed) { fprintf(stderr, "a rank failed\n"); kill_ranks(); return EXIT_FAILURE; }
    if (gpus > 1 && gather_shm) {
        const int lr = mort_hip_local_rows(ctx, H); /* rank 0's own rows are already in rgba; take the others from the mapping */
        uint8_t *own = malloc(npx * 4);
        memcpy(own, rgba, npx * 4);
        memcpy(rgba, shm, npx * 4);
        for (int ly = 0; ly < lr; ly++) { const int y = mort_hip_global_row(ctx, ly); memcpy(rgba + (size_t)y * W * 4, own + (size_t)y * W * 4, (size_t)W * 4); }
        free(own);
    }

    const double sec = (gpus > 1) ? frame_wall : stats.seconds; /* multi-GPU: wall clock of the frame on rank 0, gather included */
    printf("{\"scene\": %d, \"width\": %d, \"height\": %d, \"spp_nominal\": %d, \"spp_effective\": %d, \"depth\": %d, \"mode\": \"%s\", \"gpus\": %d, "
           "\"seconds\": %.6f, \"msamples_per_s\": %.3f, \"kernel_seconds\": %.6f, \"gather_seconds\": %.6f, \"segments\": %llu, "
           "\"algorithmic_hbm_bytes\": %llu, \"hbm_GBps\": %.4g, \"hbm_frac_of_8TBps\": %.3g, \"reference_walks\": %llu, \"kernel\": \"%s\"",
           scene, W, H, cam.samples_per_pixel, eff, cam.bounce_limit, host_mode ? "host" : mode == MORT_MODE_WAVE ? "wave" : mode == MORT_MODE_THROUGHPUT ? "throughput (non-parity)" : "mega", gpus, sec,
           (double)npx * eff / sec / 1e6, stats.seconds, stats.gather_seconds, (unsigned long long)stats.segments,
           (unsigned long long)stats.algorithmic_hbm_bytes, stats.algorithmic_hbm_bytes / stats.seconds / 1e9,
           stats.algorithmic_hbm_bytes / stats.seconds / 8e12, (unsigned long long)stats.reference_walks, stats.kernel_name);
    if (denoise) printf(", \"denoise_seconds\": %.6f", denoise_sec); /* feature pass + denoise, device time (host loops: wall time) */
    if (svgf) printf(", \"svgf_seconds\": %.6f", svgf_sec); /* feature pass + SVGF filter, likewise */
    if (temporal) printf(", \"temporal_seconds\": %.6f", temporal_sec); /* feature passes + temporal steps over all frames, likewise */
    if (cache_render) { /* the last frame's paths that ended in the volume, and the volume as the no-render uses report it */
        unsigned long long ended = 0;
        for (size_t i = 0; i < npx; i++) ended += ends_px[i];
        printf(", \"cache_depth\": %d, \"ends\": %llu", cache_depth, ended);
        if (cache_render_direct) { /* of those, the paths whose shadow segment returned a non-zero emission */
            unsigned long long lit_paths = 0;
            for (size_t i = 0; i < npx; i++) lit_paths += lit_px[i];
            printf(", \"cache_direct\": 1, \"lit\": %llu", lit_paths);
        }
        if (visibility) {
            printf(", \"normal_bias\": "); print_f32(cv.p.vis.normal_bias);
            printf(", \"min_visibility\": "); print_f32(cv.p.vis.min_visibility);
            printf(", \"depth_subsamples\": %d, \"max_distance\": ", cv.dp.subsamples); print_f32(cv.dp.max_distance);
        }
        print_refresh(&refresh);
        printf(", \"probes\": [%d, %d, %d], \"directions\": %d, \"probe_samples\": %d, \"bake_seconds\": %.6f", (int)cv.p.grid.count[0], (int)cv.p.grid.count[1],
               (int)cv.p.grid.count[2], sh_d, sh_n, cv.bake_sec);
    }
    printf("}\n");
    if (out && mort_write_ppm(out, rgba, W, H) != 0) { fprintf(stderr, "cannot write %s\n", out); return EXIT_FAILURE; }
    if (dump) {
        FILE *f = fopen(dump, "wb");
        if (!f || fwrite(accum, sizeof(float), npx * 3, f) != npx * 3) { fprintf(stderr, "cannot write %s\n", dump); return EXIT_FAILURE; }
        fclose(f);
    }
    if (sout) {
        mort_rng_state *s = hstates ? hstates : malloc(npx * sizeof *s);
        if (!hstates && (st = mort_hip_rng_store(ctx, s, W, H)) != MORT_OK) die(ctx, st, "mort_hip_rng_store");
        FILE *f = fopen(sout, "wb");
        if (!f || fwrite(s, sizeof *s, npx, f) != npx) { fprintf(stderr, "cannot write %s\n", sout); return EXIT_FAILURE; }
        fclose(f);
        if (!hstates) free(s);
    }
    if (ctx) mort_hip_shutdown(ctx);
    mort_world_free(&world);
    free(texels); free(rgba); free(accum); free(hstates); free(ends_px); free(cv.records); free(cv.depth); free(cv.back); free(cv.states);
    return 0;
}
