/*
 * cached_direct_asan.cpp -- the host form of the direct-light cached radiance queries as a stand-alone program for
 * AddressSanitizer and UndefinedBehaviorSanitizer: CPU only, no GPU and no HIP call.  scripts/cached_direct_asan.sh compiles the
 * library's host side and this file with -Xarch_host -fsanitize=address,undefined into one executable and runs it.
 *
 * Over scenes 6 and 1 at 32 x 32 pixel-centre rays, 3 paths each: a 3 x 3 x 2 volume of indirect light (the full bake minus the
 * emission-only bake, D = 64) with its depth maps, then mort_hip_query_radiance_cached_direct_host at K = 0 and 1, with and without
 * MORT_CACHED_VISIBLE, lit_out present and NULL, the scan and MORT_HOST_TREE, one and three threads -- every buffer a heap block of
 * exactly the size the contract names, so that a byte past any of them is a report -- and the refusals, which must write nothing.
 * Prints one line per scene; exit status 0 when every call answered as expected.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" {
#include "mort_host.h"
}
#include "mort_hip.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

template <typename T> struct Block { /* a heap block of exactly n elements */
    T *p; size_t n;
    explicit Block(size_t n_) : p((T *)std::malloc(n_ ? n_ * sizeof(T) : 1)), n(n_) { CHECK(p); std::memset(p, 0, n_ * sizeof(T)); }
    ~Block() { std::free(p); }
    Block(const Block &) = delete;
};

static mort_ray pixel_ray(const mort_camera *cam, int x, int y) {
    mort_ray r;
    for (int k = 0; k < 3; k++) {
        const float sample = (cam->pixel00_loc.e[k] + (float)x * cam->pixel_delta_u.e[k]) + (float)y * cam->pixel_delta_v.e[k];
        r.origin[k] = cam->center.e[k];
        r.dir[k] = sample - cam->center.e[k];
    }
    r.time = 0.5f;
    r.t_max = INFINITY;
    return r;
}

static void run_scene(int scene, const float lo[3], const float hi[3]) {
    mort_world world;
    mort_camera cam;
    mort_scene_opts opts;
    std::memset(&opts, 0, sizeof opts);
    CHECK(mort_world_init(&world) == 0);
    mort_camera_defaults(&cam);
    CHECK(mort_scene_build(scene, &world, &cam, &opts) == 0);
    cam.image_width = 32; cam.aspect_ratio = 1.0f; cam.samples_per_pixel = 1;
    mort_camera_initialize(&cam);
    const int W = cam.image_width, H = cam.image_height;
    const size_t n = (size_t)W * (size_t)H;

    mort_volume_grid grid;
    const int count[3] = {3, 3, 2};
    for (int k = 0; k < 3; k++) { grid.origin[k] = lo[k]; grid.count[k] = count[k]; grid.spacing[k] = (hi[k] - lo[k]) / (float)(count[k] - 1); }
    grid.time = 0.5f;
    const size_t probes_n = 18, D = 64;

    /* the indirect volume: the full bake, the emission-only bake from a copy of its streams, the difference, the pack, the maps */
    mort_probe_params pp, pe;
    CHECK(mort_hip_radiance_params_from_camera(&cam, &pp.rp) == MORT_OK);
    pp.directions = (int)D;
    pe = pp;
    pe.rp.bounce_limit = 1; pe.rp.samples = 1; pe.rp.background[0] = pe.rp.background[1] = pe.rp.background[2] = 0.0f;
    Block<mort_probe> probes(probes_n);
    Block<mort_rng_state> bake_states(probes_n * D), emit_states(probes_n * D);
    Block<float> sh(probes_n * MORT_SH9_FLOATS), sh_e(probes_n * MORT_SH9_FLOATS), records(probes_n * MORT_VOLUME_RECORD_FLOATS),
        depth(probes_n * MORT_DEPTH_FLOATS);
    CHECK(mort_hip_volume_probes(&grid, probes.p) == MORT_OK);
    CHECK(mort_hip_rng_seed_host(MORT_DEFAULT_SEED, (int)(probes_n * D), 1, bake_states.p) == MORT_OK);
    std::memcpy(emit_states.p, bake_states.p, probes_n * D * sizeof(mort_rng_state));
    CHECK(mort_hip_probe_bake_host(&world, &pp, probes_n, probes.p, NULL, bake_states.p, 3, MORT_HOST_TREE, sh.p, NULL) == MORT_OK);
    CHECK(mort_hip_probe_bake_host(&world, &pe, probes_n, probes.p, NULL, emit_states.p, 3, MORT_HOST_TREE, sh_e.p, NULL) == MORT_OK);
    for (size_t i = 0; i < sh.n; i++) sh.p[i] = sh.p[i] - sh_e.p[i];
    CHECK(mort_hip_volume_pack_host(probes_n, sh.p, NULL, 1, records.p, NULL) == MORT_OK);
    mort_depth_params dp;
    dp.subsamples = 2;
    dp.max_distance = 1.5f * std::sqrt(grid.spacing[0] * grid.spacing[0] + grid.spacing[1] * grid.spacing[1] + grid.spacing[2] * grid.spacing[2]);
    CHECK(mort_hip_probe_depth_bake_host(&world, &dp, probes_n, probes.p, 3, MORT_HOST_TREE, depth.p, NULL) == MORT_OK);

    Block<mort_ray> rays(n);
    Block<mort_rng_state> seeded(n);
    for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) rays.p[(size_t)y * W + x] = pixel_ray(&cam, x, y);
    CHECK(mort_hip_rng_seed_host(MORT_DEFAULT_SEED, W, H, seeded.p) == MORT_OK);

    mort_cached_params cp;
    std::memset(&cp, 0, sizeof cp);
    CHECK(mort_hip_radiance_params_from_camera(&cam, &cp.path) == MORT_OK);
    cp.path.samples = 3;
    cp.grid = grid;
    cp.vis.normal_bias = 0.01f * grid.spacing[0]; cp.vis.min_visibility = 0.05f;

    unsigned long long calls = 0, ended = 0, lit_paths = 0;
    for (int K = 0; K <= 1; K++) for (int visible = 0; visible <= 1; visible++) for (int with_lit = 0; with_lit <= 1; with_lit++)
        for (int tree = 0; tree <= 1; tree++) {
            cp.cache_depth = K; cp.flags = visible ? MORT_CACHED_VISIBLE : 0u;
            Block<mort_rng_state> states(n);
            Block<float> rgb(3 * n);
            Block<uint32_t> ends(n), lit(with_lit ? n : 0);
            std::memcpy(states.p, seeded.p, n * sizeof(mort_rng_state));
            double sec = -1;
            CHECK(mort_hip_query_radiance_cached_direct_host(&world, &cp, n, rays.p, states.p, records.p, visible ? depth.p : NULL, tree ? 3 : 1,
                                                             tree ? MORT_HOST_TREE : 0, rgb.p, ends.p, with_lit ? lit.p : NULL, &sec) == MORT_OK);
            CHECK(sec >= 0);
            for (size_t i = 0; i < n; i++) {
                CHECK(ends.p[i] <= 3u);
                ended += ends.p[i];
                if (with_lit) { CHECK(lit.p[i] <= ends.p[i]); lit_paths += lit.p[i]; }
            }
            calls++;
        }

    /* the refusals: the outputs keep their fill */
    {
        Block<mort_rng_state> states(n);
        Block<float> rgb(3 * n);
        Block<uint32_t> ends(n), lit(n);
        std::memset(states.p, 7, n * sizeof(mort_rng_state)); std::memset(rgb.p, 7, 3 * n * sizeof(float));
        std::memset(ends.p, 7, n * sizeof(uint32_t)); std::memset(lit.p, 7, n * sizeof(uint32_t));
        cp.cache_depth = 0; cp.flags = 0;
        mort_cached_params bad;
#define REFUSED(status, P, N, RAYS, STATES, RECORDS, DEPTH, RGB, ENDS, LIT) \
        CHECK(mort_hip_query_radiance_cached_direct_host(&world, P, N, RAYS, STATES, RECORDS, DEPTH, 1, 0, RGB, ENDS, LIT, NULL) == status)
        REFUSED(MORT_ERR_INVALID, NULL, n, rays.p, states.p, records.p, NULL, rgb.p, ends.p, lit.p);
        REFUSED(MORT_ERR_INVALID, &cp, n, NULL, states.p, records.p, NULL, rgb.p, ends.p, lit.p);
        REFUSED(MORT_ERR_INVALID, &cp, n, rays.p, NULL, records.p, NULL, rgb.p, ends.p, lit.p);
        REFUSED(MORT_ERR_INVALID, &cp, n, rays.p, states.p, NULL, NULL, rgb.p, ends.p, lit.p);
        REFUSED(MORT_ERR_INVALID, &cp, n, rays.p, states.p, records.p, NULL, NULL, ends.p, lit.p);
        REFUSED(MORT_ERR_INVALID, &cp, n, rays.p, states.p, records.p, depth.p, rgb.p, ends.p, lit.p); /* maps without the flag */
        bad = cp; bad.flags = MORT_CACHED_VISIBLE;
        REFUSED(MORT_ERR_INVALID, &bad, n, rays.p, states.p, records.p, NULL, rgb.p, ends.p, lit.p);   /* the flag without maps */
        bad = cp; bad.flags = 2u;
        REFUSED(MORT_ERR_INVALID, &bad, n, rays.p, states.p, records.p, NULL, rgb.p, ends.p, lit.p);
        bad = cp; bad.cache_depth = -1;
        REFUSED(MORT_ERR_INVALID, &bad, n, rays.p, states.p, records.p, NULL, rgb.p, ends.p, lit.p);
        bad = cp; bad.cache_depth = MORT_MAX_BOUNCE_LIMIT + 1;
        REFUSED(MORT_ERR_INVALID, &bad, n, rays.p, states.p, records.p, NULL, rgb.p, ends.p, lit.p);
        bad = cp; bad.path.samples = 0;
        REFUSED(MORT_ERR_INVALID, &bad, n, rays.p, states.p, records.p, NULL, rgb.p, ends.p, lit.p);
        bad = cp; bad.path.bounce_limit = MORT_MAX_BOUNCE_LIMIT + 1;
        REFUSED(MORT_ERR_CAPACITY, &bad, n, rays.p, states.p, records.p, NULL, rgb.p, ends.p, lit.p);
        bad = cp; bad.path.light_obj_type = MORT_OBJ_QUAD; bad.path.light_obj_idx = 1 << 20;
        REFUSED(MORT_ERR_INVALID, &bad, n, rays.p, states.p, records.p, NULL, rgb.p, ends.p, lit.p);
        bad = cp; bad.grid.count[1] = 0;
        REFUSED(MORT_ERR_INVALID, &bad, n, rays.p, states.p, records.p, NULL, rgb.p, ends.p, lit.p);
        bad = cp; bad.grid.spacing[2] = 0.0f;
        REFUSED(MORT_ERR_INVALID, &bad, n, rays.p, states.p, records.p, NULL, rgb.p, ends.p, lit.p);
        REFUSED(MORT_ERR_INVALID, &cp, n, rays.p, states.p, records.p, NULL, rgb.p, ends.p, ends.p);             /* lit over ends */
        REFUSED(MORT_ERR_INVALID, &cp, n, rays.p, states.p, records.p, NULL, rgb.p, ends.p, (uint32_t *)rgb.p);  /* lit over the colours */
        REFUSED(MORT_ERR_INVALID, &cp, n, rays.p, states.p, records.p, NULL, rgb.p, ends.p, (uint32_t *)rays.p); /* lit over the rays */
        REFUSED(MORT_ERR_INVALID, &cp, n, rays.p, states.p, records.p, NULL, rgb.p, ends.p, (uint32_t *)records.p);
        REFUSED(MORT_ERR_INVALID, &cp, n, rays.p, states.p, records.p, NULL, rgb.p, ends.p, (uint32_t *)states.p);
#undef REFUSED
        CHECK(mort_hip_query_radiance_cached_direct_host(NULL, &cp, n, rays.p, states.p, records.p, NULL, 1, 0, rgb.p, ends.p, lit.p, NULL) == MORT_ERR_INVALID);
        CHECK(mort_hip_query_radiance_cached_direct_host(&world, &cp, 0, rays.p, states.p, records.p, NULL, 1, 0, rgb.p, ends.p, lit.p, NULL) == MORT_OK);
        const unsigned char *b[4] = {(const unsigned char *)states.p, (const unsigned char *)rgb.p, (const unsigned char *)ends.p, (const unsigned char *)lit.p};
        const size_t nb[4] = {n * sizeof(mort_rng_state), 3 * n * sizeof(float), n * sizeof(uint32_t), n * sizeof(uint32_t)};
        for (int k = 0; k < 4; k++) for (size_t i = 0; i < nb[k]; i++) CHECK(b[k][i] == 7);
    }
    std::printf("scene %d: %llu calls over %zu rays x 3 paths, %llu paths ended in the volume, %llu lit; the refusals wrote nothing\n", scene, calls, n, ended,
                lit_paths);
    mort_world_free(&world);
}

int main() {
    const float lo6[3] = {100, 100, 100}, hi6[3] = {455, 455, 455};
    const float lo1[3] = {-6, 0.2f, -6}, hi1[3] = {6, 2, 6};
    run_scene(6, lo6, hi6);
    run_scene(1, lo1, hi1);
    return 0;
}
