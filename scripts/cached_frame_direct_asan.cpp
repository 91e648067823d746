/*
 * cached_frame_direct_asan.cpp -- the host form of the direct-light cached frames as a stand-alone program for
 * AddressSanitizer and UndefinedBehaviorSanitizer: CPU only, no GPU and no HIP call.  scripts/cached_frame_direct_asan.sh compiles
 * the library's host side and this file with -Xarch_host -fsanitize=address,undefined into one executable and runs it.
 *
 * Over scenes 6 and 1 at 33 x 29 pixels, 4 samples each (an odd size, so that a row or a pixel too many is a report): a 3 x 3 x 2
 * volume of indirect light (the full bake minus the emission-only bake, D = 64) with its depth maps, then
 * mort_hip_render_cached_direct_host at K = 0 and 1, with and without MORT_CACHED_VISIBLE, lit_px_out present and NULL (and with
 * it the other optional outputs), the scan and MORT_HOST_TREE, one and three threads -- every buffer a heap block of exactly the
 * size the contract names, so that a byte past any of them is a report -- and the refusals, which must write nothing.  Prints one
 * line per scene; exit status 0 when every call answered as expected.
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
    cam.image_width = 33; cam.aspect_ratio = 33.0f / 29.5f; cam.samples_per_pixel = 4;
    mort_camera_initialize(&cam);
    const int W = cam.image_width, H = cam.image_height;
    CHECK(W == 33 && H == 29 && cam.sqrt_spp == 2);
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

    Block<mort_rng_state> seeded(n);
    CHECK(mort_hip_rng_seed_host(MORT_DEFAULT_SEED, W, H, seeded.p) == MORT_OK);

    mort_cached_frame_params fp;
    std::memset(&fp, 0, sizeof fp);
    fp.grid = grid;
    fp.vis.normal_bias = 0.01f * grid.spacing[0]; fp.vis.min_visibility = 0.05f;

    unsigned long long calls = 0, ended = 0, lit_paths = 0, segments = 0;
    for (int K = 0; K <= 1; K++) for (int visible = 0; visible <= 1; visible++) for (int with_lit = 0; with_lit <= 1; with_lit++)
        for (int tree = 0; tree <= 1; tree++) {
            fp.cache_depth = K; fp.flags = visible ? MORT_CACHED_VISIBLE : 0u;
            Block<mort_rng_state> states(n);
            Block<uint8_t> rgba(4 * n);
            /* with lit: every optional output; without: none of them */
            Block<float> accum(with_lit ? 3 * n : 0);
            Block<uint32_t> seg(with_lit ? n : 0), ends(with_lit ? n : 0), lit(with_lit ? n : 0);
            std::memcpy(states.p, seeded.p, n * sizeof(mort_rng_state));
            mort_stats st;
            CHECK(mort_hip_render_cached_direct_host(&world, &cam, states.p, tree ? 3 : 1, tree ? MORT_HOST_TREE : 0, &fp, records.p, visible ? depth.p : NULL,
                                                     rgba.p, with_lit ? accum.p : NULL, with_lit ? seg.p : NULL, with_lit ? ends.p : NULL,
                                                     with_lit ? lit.p : NULL, &st) == MORT_OK);
            CHECK(st.pixels == n && st.eff_samples == 4 * n && std::strstr(st.kernel_name, "cached frame, direct"));
            unsigned long long s = 0;
            for (size_t i = 0; with_lit && i < n; i++) {
                CHECK(lit.p[i] <= ends.p[i] && ends.p[i] <= 4u);
                ended += ends.p[i]; lit_paths += lit.p[i]; s += seg.p[i];
            }
            CHECK(!with_lit || s == st.segments);
            segments += st.segments;
            calls++;
        }

    /* the refusals: the outputs keep their fill */
    {
        Block<mort_rng_state> states(n);
        Block<uint8_t> rgba(4 * n);
        Block<float> accum(3 * n);
        Block<uint32_t> seg(n), ends(n), lit(n);
        std::memset(states.p, 7, n * sizeof(mort_rng_state)); std::memset(rgba.p, 7, 4 * n); std::memset(accum.p, 7, 3 * n * sizeof(float));
        std::memset(seg.p, 7, n * sizeof(uint32_t)); std::memset(ends.p, 7, n * sizeof(uint32_t)); std::memset(lit.p, 7, n * sizeof(uint32_t));
        fp.cache_depth = 0; fp.flags = 0;
        mort_cached_frame_params bad;
        mort_camera bc;
#define REFUSED(status, CAM, STATES, P, RECORDS, DEPTH, RGBA, ACCUM, SEG, ENDS, LIT) \
        CHECK(mort_hip_render_cached_direct_host(&world, CAM, STATES, 1, 0, P, RECORDS, DEPTH, RGBA, ACCUM, SEG, ENDS, LIT, NULL) == status)
        REFUSED(MORT_ERR_INVALID, NULL, states.p, &fp, records.p, NULL, rgba.p, accum.p, seg.p, ends.p, lit.p);
        REFUSED(MORT_ERR_INVALID, &cam, NULL, &fp, records.p, NULL, rgba.p, accum.p, seg.p, ends.p, lit.p);
        REFUSED(MORT_ERR_INVALID, &cam, states.p, NULL, records.p, NULL, rgba.p, accum.p, seg.p, ends.p, lit.p);
        REFUSED(MORT_ERR_INVALID, &cam, states.p, &fp, NULL, NULL, rgba.p, accum.p, seg.p, ends.p, lit.p);
        REFUSED(MORT_ERR_INVALID, &cam, states.p, &fp, records.p, NULL, NULL, accum.p, seg.p, ends.p, lit.p);
        REFUSED(MORT_ERR_INVALID, &cam, states.p, &fp, records.p, depth.p, rgba.p, accum.p, seg.p, ends.p, lit.p); /* maps without the flag */
        bad = fp; bad.flags = MORT_CACHED_VISIBLE;
        REFUSED(MORT_ERR_INVALID, &cam, states.p, &bad, records.p, NULL, rgba.p, accum.p, seg.p, ends.p, lit.p);   /* the flag without maps */
        bad = fp; bad.flags = 2u;
        REFUSED(MORT_ERR_INVALID, &cam, states.p, &bad, records.p, NULL, rgba.p, accum.p, seg.p, ends.p, lit.p);
        bad = fp; bad.flags = 3u;
        REFUSED(MORT_ERR_INVALID, &cam, states.p, &bad, records.p, depth.p, rgba.p, accum.p, seg.p, ends.p, lit.p);
        bad = fp; bad.cache_depth = -1;
        REFUSED(MORT_ERR_INVALID, &cam, states.p, &bad, records.p, NULL, rgba.p, accum.p, seg.p, ends.p, lit.p);
        bad = fp; bad.cache_depth = MORT_MAX_BOUNCE_LIMIT + 1;
        REFUSED(MORT_ERR_INVALID, &cam, states.p, &bad, records.p, NULL, rgba.p, accum.p, seg.p, ends.p, lit.p);
        bad = fp; bad.grid.count[1] = 0;
        REFUSED(MORT_ERR_INVALID, &cam, states.p, &bad, records.p, NULL, rgba.p, accum.p, seg.p, ends.p, lit.p);
        bad = fp; bad.grid.spacing[2] = 0.0f;
        REFUSED(MORT_ERR_INVALID, &cam, states.p, &bad, records.p, NULL, rgba.p, accum.p, seg.p, ends.p, lit.p);
        bc = cam; bc.image_width = 0;
        REFUSED(MORT_ERR_INVALID, &bc, states.p, &fp, records.p, NULL, rgba.p, accum.p, seg.p, ends.p, lit.p);
        bc = cam; bc.bounce_limit = MORT_MAX_BOUNCE_LIMIT + 1;
        REFUSED(MORT_ERR_CAPACITY, &bc, states.p, &fp, records.p, NULL, rgba.p, accum.p, seg.p, ends.p, lit.p);
        bc = cam; bc.light_obj_type = MORT_OBJ_QUAD; bc.light_obj_idx = 1 << 20;
        REFUSED(MORT_ERR_INVALID, &bc, states.p, &fp, records.p, NULL, rgba.p, accum.p, seg.p, ends.p, lit.p);
        REFUSED(MORT_ERR_INVALID, &cam, states.p, &fp, records.p, NULL, rgba.p, accum.p, seg.p, ends.p, ends.p);               /* lit over ends */
        REFUSED(MORT_ERR_INVALID, &cam, states.p, &fp, records.p, NULL, rgba.p, accum.p, seg.p, ends.p, seg.p);                /* lit over the segments */
        REFUSED(MORT_ERR_INVALID, &cam, states.p, &fp, records.p, NULL, rgba.p, accum.p, seg.p, ends.p, (uint32_t *)accum.p);  /* lit over the accumulators */
        REFUSED(MORT_ERR_INVALID, &cam, states.p, &fp, records.p, NULL, rgba.p, accum.p, seg.p, ends.p, (uint32_t *)rgba.p);   /* lit over the image */
        REFUSED(MORT_ERR_INVALID, &cam, states.p, &fp, records.p, NULL, rgba.p, accum.p, seg.p, ends.p, (uint32_t *)records.p);
        REFUSED(MORT_ERR_INVALID, &cam, states.p, &fp, records.p, NULL, rgba.p, accum.p, seg.p, ends.p, (uint32_t *)states.p);
#undef REFUSED
        CHECK(mort_hip_render_cached_direct_host(NULL, &cam, states.p, 1, 0, &fp, records.p, NULL, rgba.p, accum.p, seg.p, ends.p, lit.p, NULL) == MORT_ERR_INVALID);
        const unsigned char *b[6] = {(const unsigned char *)states.p, rgba.p, (const unsigned char *)accum.p, (const unsigned char *)seg.p,
                                     (const unsigned char *)ends.p, (const unsigned char *)lit.p};
        const size_t nb[6] = {n * sizeof(mort_rng_state), 4 * n, 3 * n * sizeof(float), n * sizeof(uint32_t), n * sizeof(uint32_t), n * sizeof(uint32_t)};
        for (int k = 0; k < 6; k++) for (size_t i = 0; i < nb[k]; i++) CHECK(b[k][i] == 7);
    }
    std::printf("scene %d: %llu frames of %zu pixels x 4 paths, %llu segments, %llu paths ended in the volume, %llu lit; the refusals wrote nothing\n", scene,
                calls, n, segments, ended, lit_paths);
    mort_world_free(&world);
}

int main() {
    const float lo6[3] = {100, 100, 100}, hi6[3] = {455, 455, 455};
    const float lo1[3] = {-6, 0.2f, -6}, hi1[3] = {6, 2, 6};
    run_scene(6, lo6, hi6);
    run_scene(1, lo1, hi1);
    return 0;
}
