/*
 * refresh_direct_asan.cpp -- the host form of the direct-light volume refresh as a stand-alone program for
 * AddressSanitizer and UndefinedBehaviorSanitizer: CPU only, no GPU and no HIP call.  scripts/refresh_direct_asan.sh compiles the
 * library's host side and this file with -Xarch_host -fsanitize=address,undefined into one executable and runs it.
 *
 * Over scenes 6 and 1: a 3 x 3 x 2 volume of indirect light (the full bake minus the emission-only bake) with its depth maps, then
 * mort_hip_volume_refresh_direct_host with D = 64 and 320, a full and a partial selection, with and without MORT_CACHED_VISIBLE,
 * lit_out present and NULL, the scan and MORT_HOST_TREE, one and three threads; two rounds chained through two buffers with rotated
 * sets and the bake's streams carried on -- every buffer a heap block of exactly the size the contract names, so that a byte past
 * any of them is a report -- and the refusals, which must write nothing.  Prints one line per scene; exit status 0 when every call
 * answered as expected.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

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

static void run_scene(int scene, const float lo[3], const float hi[3]) {
    mort_world world;
    mort_camera cam;
    mort_scene_opts opts;
    std::memset(&opts, 0, sizeof opts);
    CHECK(mort_world_init(&world) == 0);
    mort_camera_defaults(&cam);
    CHECK(mort_scene_build(scene, &world, &cam, &opts) == 0);
    cam.image_width = 32; cam.aspect_ratio = 1.0f; cam.samples_per_pixel = 1;
    cam.bounce_limit = 6;
    mort_camera_initialize(&cam);

    mort_volume_grid grid;
    const int count[3] = {3, 3, 2};
    for (int k = 0; k < 3; k++) { grid.origin[k] = lo[k]; grid.count[k] = count[k]; grid.spacing[k] = (hi[k] - lo[k]) / (float)(count[k] - 1); }
    grid.time = 0.5f;
    const size_t P = 18;

    unsigned long long calls = 0, ended = 0, lit_paths = 0;
    const size_t Ds[2] = {64, 320};
    for (int di = 0; di < 2; di++) {
        const size_t D = Ds[di];
        /* the indirect volume: the full bake, the emission-only bake from a copy of its streams, the difference, the pack, the maps */
        mort_probe_params pp, pe;
        CHECK(mort_hip_radiance_params_from_camera(&cam, &pp.rp) == MORT_OK);
        pp.directions = (int)D;
        pe = pp;
        pe.rp.bounce_limit = 1; pe.rp.samples = 1; pe.rp.background[0] = pe.rp.background[1] = pe.rp.background[2] = 0.0f;
        Block<mort_probe> probes(P);
        Block<mort_rng_state> bake_states(P * D), emit_states(P * D);
        Block<float> sh(P * MORT_SH9_FLOATS), sh_e(P * MORT_SH9_FLOATS), records(P * MORT_VOLUME_RECORD_FLOATS), depth(P * MORT_DEPTH_FLOATS);
        Block<float> weight(P);
        for (size_t i = 0; i < P; i++) weight.p[i] = (i % 5 == 2) ? 0.0f : 1.0f; /* some probes take the copy rule */
        CHECK(mort_hip_volume_probes(&grid, probes.p) == MORT_OK);
        CHECK(mort_hip_rng_seed_host(MORT_DEFAULT_SEED, (int)(P * D), 1, bake_states.p) == MORT_OK);
        std::memcpy(emit_states.p, bake_states.p, P * D * sizeof(mort_rng_state));
        CHECK(mort_hip_probe_bake_host(&world, &pp, P, probes.p, NULL, bake_states.p, 3, MORT_HOST_TREE, sh.p, NULL) == MORT_OK);
        CHECK(mort_hip_probe_bake_host(&world, &pe, P, probes.p, NULL, emit_states.p, 3, MORT_HOST_TREE, sh_e.p, NULL) == MORT_OK);
        for (size_t i = 0; i < sh.n; i++) sh.p[i] = sh.p[i] - sh_e.p[i];
        CHECK(mort_hip_volume_pack_host(P, sh.p, weight.p, 1, records.p, NULL) == MORT_OK);
        mort_depth_params dp;
        dp.subsamples = 2;
        dp.max_distance = 1.5f * std::sqrt(grid.spacing[0] * grid.spacing[0] + grid.spacing[1] * grid.spacing[1] + grid.spacing[2] * grid.spacing[2]);
        CHECK(mort_hip_probe_depth_bake_host(&world, &dp, P, probes.p, 3, MORT_HOST_TREE, depth.p, NULL) == MORT_OK);

        mort_refresh_params rp;
        std::memset(&rp, 0, sizeof rp);
        CHECK(mort_hip_radiance_params_from_camera(&cam, &rp.cached.path) == MORT_OK);
        rp.cached.path.samples = 2;
        rp.cached.grid = grid;
        rp.cached.vis.normal_bias = 0.01f * grid.spacing[0]; rp.cached.vis.min_visibility = 0.05f;
        rp.directions = (int)D; rp.hysteresis = 0.75f;

        const uint32_t sel[2][3] = {{0, 1, (uint32_t)P}, {3, 7, 3}}; /* first, step, m */
        for (int K = 0; K <= 1; K++) for (int visible = 0; visible <= 1; visible++) for (int with_lit = 0; with_lit <= 1; with_lit++)
            for (int tree = 0; tree <= 1; tree++) for (int s = 0; s < 2; s++) {
                if (di == 1 && (K == 1 || s == 1)) continue; /* D = 320: the full selection at K = 0 */
                rp.cached.cache_depth = K; rp.cached.flags = visible ? MORT_CACHED_VISIBLE : 0u;
                rp.first = sel[s][0]; rp.step = sel[s][1];
                Block<mort_rng_state> states(P * D);
                Block<float> out(P * MORT_VOLUME_RECORD_FLOATS);
                Block<uint32_t> ends(P), lit(with_lit ? P : 0);
                std::memcpy(states.p, bake_states.p, P * D * sizeof(mort_rng_state));
                double sec = -1;
                CHECK(mort_hip_volume_refresh_direct_host(&world, &rp, sel[s][2], NULL, states.p, records.p, visible ? depth.p : NULL, tree ? 3 : 1,
                                                          tree ? MORT_HOST_TREE : 0, out.p, ends.p, with_lit ? lit.p : NULL, &sec) == MORT_OK);
                CHECK(sec >= 0);
                for (size_t i = 0; i < sel[s][2]; i++) {
                    const size_t p = sel[s][0] + i * sel[s][1];
                    CHECK(ends.p[p] <= 2u * D);
                    if (weight.p[p] == 0.0f) CHECK(ends.p[p] == 0u && std::memcmp(out.p + 32 * p, records.p + 32 * p, 128) == 0);
                    ended += ends.p[p];
                    if (with_lit) { CHECK(lit.p[p] <= ends.p[p]); lit_paths += lit.p[p]; }
                }
                calls++;
            }

        /* two rounds chained: rotated sets, the bake's streams carried on, the records ping-pong */
        {
            Block<float> a(P * MORT_VOLUME_RECORD_FLOATS), b(P * MORT_VOLUME_RECORD_FLOATS), dirs(3 * D);
            Block<uint32_t> ends(P), lit(P);
            std::memcpy(a.p, records.p, a.n * sizeof(float));
            rp.cached.cache_depth = 0; rp.cached.flags = MORT_CACHED_VISIBLE; rp.first = 0; rp.step = 1;
            float *in = a.p, *out = b.p;
            for (uint32_t r = 1; r <= 2; r++) {
                CHECK(mort_hip_probe_directions_round((int)D, r, dirs.p) == MORT_OK);
                CHECK(mort_hip_volume_refresh_direct_host(&world, &rp, P, dirs.p, bake_states.p, in, depth.p, 3, MORT_HOST_TREE, out, ends.p, lit.p, NULL) == MORT_OK);
                float *t = in; in = out; out = t;
                calls++;
            }
            for (size_t i = 0; i < P; i++) { ended += ends.p[i]; lit_paths += lit.p[i]; }
        }

        if (di == 1) continue;
        /* the refusals: the outputs keep their fill */
        Block<mort_rng_state> states(P * D);
        Block<float> out(P * MORT_VOLUME_RECORD_FLOATS), dirs(3 * D);
        Block<uint32_t> ends(P), lit(P);
        std::memset(states.p, 7, P * D * sizeof(mort_rng_state)); std::memset(out.p, 7, out.n * sizeof(float));
        std::memset(ends.p, 7, P * sizeof(uint32_t)); std::memset(lit.p, 7, P * sizeof(uint32_t));
        CHECK(mort_hip_probe_directions((int)D, dirs.p) == MORT_OK);
        rp.cached.cache_depth = 0; rp.cached.flags = 0; rp.first = 0; rp.step = 1;
        mort_refresh_params bad;
#define REFUSED(status, PARAMS, M, DIRS, STATES, IN, DEPTH, OUT, ENDS, LIT) \
        CHECK(mort_hip_volume_refresh_direct_host(&world, PARAMS, M, DIRS, STATES, IN, DEPTH, 1, 0, OUT, ENDS, LIT, NULL) == status)
        REFUSED(MORT_ERR_INVALID, NULL, P, dirs.p, states.p, records.p, NULL, out.p, ends.p, lit.p);
        REFUSED(MORT_ERR_INVALID, &rp, P, dirs.p, NULL, records.p, NULL, out.p, ends.p, lit.p);
        REFUSED(MORT_ERR_INVALID, &rp, P, dirs.p, states.p, NULL, NULL, out.p, ends.p, lit.p);
        REFUSED(MORT_ERR_INVALID, &rp, P, dirs.p, states.p, records.p, NULL, NULL, ends.p, lit.p);
        REFUSED(MORT_ERR_INVALID, &rp, P, dirs.p, states.p, records.p, depth.p, out.p, ends.p, lit.p); /* maps without the flag */
        bad = rp; bad.cached.flags = MORT_CACHED_VISIBLE;
        REFUSED(MORT_ERR_INVALID, &bad, P, dirs.p, states.p, records.p, NULL, out.p, ends.p, lit.p);   /* the flag without maps */
        bad = rp; bad.directions = 96;
        REFUSED(MORT_ERR_INVALID, &bad, P, dirs.p, states.p, records.p, NULL, out.p, ends.p, lit.p);
        bad = rp; bad.cached.path.samples = 0;
        REFUSED(MORT_ERR_INVALID, &bad, P, dirs.p, states.p, records.p, NULL, out.p, ends.p, lit.p);
        bad = rp; bad.cached.cache_depth = MORT_MAX_BOUNCE_LIMIT + 1;
        REFUSED(MORT_ERR_INVALID, &bad, P, dirs.p, states.p, records.p, NULL, out.p, ends.p, lit.p);
        bad = rp; bad.hysteresis = 1.0f;
        REFUSED(MORT_ERR_INVALID, &bad, P, dirs.p, states.p, records.p, NULL, out.p, ends.p, lit.p);
        bad = rp; bad.hysteresis = NAN;
        REFUSED(MORT_ERR_INVALID, &bad, P, dirs.p, states.p, records.p, NULL, out.p, ends.p, lit.p);
        bad = rp; bad.step = 0;
        REFUSED(MORT_ERR_INVALID, &bad, P, dirs.p, states.p, records.p, NULL, out.p, ends.p, lit.p);
        bad = rp; bad.first = 1;
        REFUSED(MORT_ERR_INVALID, &bad, P, dirs.p, states.p, records.p, NULL, out.p, ends.p, lit.p);
        bad = rp; bad.first = 0xffffffffu; bad.step = 0xffffffffu;
        REFUSED(MORT_ERR_INVALID, &bad, 2, dirs.p, states.p, records.p, NULL, out.p, ends.p, lit.p);
        bad = rp; bad.cached.path.bounce_limit = MORT_MAX_BOUNCE_LIMIT + 1;
        REFUSED(MORT_ERR_CAPACITY, &bad, P, dirs.p, states.p, records.p, NULL, out.p, ends.p, lit.p);
        bad = rp; bad.cached.path.light_obj_type = MORT_OBJ_QUAD; bad.cached.path.light_obj_idx = 1 << 20;
        REFUSED(MORT_ERR_INVALID, &bad, P, dirs.p, states.p, records.p, NULL, out.p, ends.p, lit.p);
        REFUSED(MORT_ERR_INVALID, &rp, P, dirs.p, states.p, records.p, NULL, records.p, ends.p, lit.p);             /* in place */
        REFUSED(MORT_ERR_INVALID, &rp, P, dirs.p, states.p, records.p, NULL, out.p, ends.p, ends.p);                /* lit over ends */
        REFUSED(MORT_ERR_INVALID, &rp, P, dirs.p, states.p, records.p, NULL, out.p, ends.p, (uint32_t *)out.p);     /* lit over the records */
        REFUSED(MORT_ERR_INVALID, &rp, P, dirs.p, states.p, records.p, NULL, out.p, ends.p, (uint32_t *)records.p);
        REFUSED(MORT_ERR_INVALID, &rp, P, dirs.p, states.p, records.p, NULL, out.p, ends.p, (uint32_t *)states.p);
        REFUSED(MORT_ERR_INVALID, &rp, P, dirs.p, states.p, records.p, NULL, out.p, ends.p, (uint32_t *)dirs.p);
#undef REFUSED
        CHECK(mort_hip_volume_refresh_direct_host(NULL, &rp, P, dirs.p, states.p, records.p, NULL, 1, 0, out.p, ends.p, lit.p, NULL) == MORT_ERR_INVALID);
        CHECK(mort_hip_volume_refresh_direct_host(&world, &rp, 0, dirs.p, states.p, records.p, NULL, 1, 0, out.p, ends.p, lit.p, NULL) == MORT_OK);
        const unsigned char *bl[4] = {(const unsigned char *)states.p, (const unsigned char *)out.p, (const unsigned char *)ends.p, (const unsigned char *)lit.p};
        const size_t nb[4] = {P * D * sizeof(mort_rng_state), out.n * sizeof(float), P * sizeof(uint32_t), P * sizeof(uint32_t)};
        for (int k = 0; k < 4; k++) for (size_t i = 0; i < nb[k]; i++) CHECK(bl[k][i] == 7);
    }
    std::printf("scene %d: %llu calls, %llu paths ended in the volume, %llu lit; the refusals wrote nothing\n", scene, calls, ended, lit_paths);
    mort_world_free(&world);
}

int main() {
    const float lo6[3] = {100, 100, 100}, hi6[3] = {455, 455, 455};
    const float lo1[3] = {-6, 0.2f, -6}, hi1[3] = {6, 2, 6};
    run_scene(6, lo6, hi6);
    run_scene(1, lo1, hi1);
    return 0;
}
