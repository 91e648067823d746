/*
 * depth_host_sanitize.cpp -- the host forms of the visibility-weighted irradiance volumes as a stand-alone
 * program for AddressSanitizer / UBSan on the CPU: its own main over the library's host side, every buffer a heap block of
 * exactly its size, so that a read or a write one byte outside is a report.  No GPU is touched: only *_host entry points run.
 *
 *   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -fno-fast-math -fno-gpu-rdc -Iinclude -Imort_amd/csrc/hip \
 *         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
 *         scripts/depth_host_sanitize.cpp mort_amd/csrc/hip/*.hip -Lmort_amd/lib -lmort_host -Wl,-rpath,$PWD/mort_amd/lib -lpthread -ldl \
 *         -o depth_host_sanitize      (after `make host`: the C scene layer builds the worlds)
 *   ./depth_host_sanitize        (prints "ok" and exits 0; a finding aborts with the sanitizer's report)
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mort_hip.h"
#include "mort_host.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

template <class T> static T *block(size_t n) { return (T *)std::malloc(n ? n * sizeof(T) : 1); }

static float frand(unsigned &s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.0f / 16777216.0f); }

static int bake(const mort_world *w, int scene, int threads, int flags) {
    const mort_volume_grid g = {{100.0f, 100.0f, 100.0f}, {177.5f, 177.5f, 177.5f}, {3, 2, 2}, 0.5f};
    const size_t n = 12;
    mort_probe *probes = block<mort_probe>(n);
    CHECK(mort_hip_volume_probes(&g, probes) == MORT_OK);
    probes[5].position[1] = NAN;
    probes[7].position[0] = 1e6f;
    for (int s = 1; s <= 3; s++) {
        const mort_depth_params p = {s, 400.0f};
        float *a = block<float>(n * MORT_DEPTH_FLOATS), *b = block<float>(n * MORT_DEPTH_FLOATS);
        CHECK(mort_hip_probe_depth_bake_host(w, &p, n, probes, 1, flags, a, nullptr) == MORT_OK);
        CHECK(mort_hip_probe_depth_bake_host(w, &p, n, probes, threads, flags, b, nullptr) == MORT_OK);
        CHECK(std::memcmp(a, b, n * MORT_DEPTH_FLOATS * sizeof(float)) == 0);
        CHECK(mort_hip_probe_depth_bake_host(w, &p, 0, probes, threads, flags, b, nullptr) == MORT_OK);
        std::free(a); std::free(b);
    }
    const mort_depth_params bad = {9, 400.0f};
    float *d = block<float>(n * MORT_DEPTH_FLOATS);
    CHECK(mort_hip_probe_depth_bake_host(w, &bad, n, probes, 1, flags, d, nullptr) == MORT_ERR_INVALID);
    CHECK(mort_hip_probe_depth_bake_host(w, nullptr, n, probes, 1, flags, d, nullptr) == MORT_ERR_INVALID);
    std::free(d); std::free(probes);
    (void)scene;
    return 0;
}

static int sample(const int count[3], size_t stride, int mask, int threads) {
    mort_volume_grid g = {{-1.5f, 0.25f, 3.0f}, {0.7f, 1.3f, 0.45f}, {count[0], count[1], count[2]}, 0.5f};
    const size_t probes = (size_t)count[0] * count[1] * count[2], n = 1500;
    unsigned seed = 12345u + (unsigned)stride + (unsigned)mask;
    float *rec = block<float>(probes * MORT_VOLUME_RECORD_FLOATS), *maps = block<float>(probes * MORT_DEPTH_FLOATS);
    for (size_t p = 0; p < probes; p++) {
        for (int k = 0; k < MORT_VOLUME_RECORD_FLOATS; k++) rec[p * MORT_VOLUME_RECORD_FLOATS + k] = k < 27 ? 3.0f * frand(seed) - 1.0f : 0.0f;
        float wt = 1.0f;
        if (mask == 1 && p % 3 == 1) wt = 0.0f;
        if (mask == 2) wt = 2.0f * frand(seed);
        rec[p * MORT_VOLUME_RECORD_FLOATS + 27] = wt;
        for (int k = 0; k < MORT_DEPTH_FLOATS; k += 2) {
            const float m1 = 2.0f * frand(seed);
            maps[p * MORT_DEPTH_FLOATS + k] = wt == 0.0f ? NAN : m1;
            maps[p * MORT_DEPTH_FLOATS + k + 1] = m1 * m1 + 0.5f * frand(seed);
        }
    }
    const size_t span = (n - 1) * stride + sizeof(mort_volume_point); /* the points' block ends where the last point does */
    unsigned char *pts = block<unsigned char>(span);
    std::memset(pts, 0xa5, span);
    for (size_t i = 0; i < n; i++) {
        float v[6];
        for (int k = 0; k < 3; k++) v[k] = g.origin[k] + (4.0f * frand(seed) - 1.0f) * g.spacing[k] * (float)(count[k] > 1 ? count[k] - 1 : 1);
        for (int k = 3; k < 6; k++) v[k] = 2.0f * frand(seed) - 1.0f;
        if (i % 50 == 7) v[i % 3] = NAN;
        if (i % 50 == 9) v[i % 3] = INFINITY;
        if (i % 50 == 11) v[i % 3] = 1e36f;
        if (i % 50 == 13) for (int k = 0; k < 3; k++) v[k] = g.origin[k]; /* exactly at a probe */
        std::memcpy(pts + i * stride, v, sizeof v);
    }
    const mort_volume_vis_params vp = {0.25f, mask == 2 ? 0.0f : 0.05f};
    float *a = block<float>(4 * n), *b = block<float>(4 * n);
    CHECK(mort_hip_volume_sample_visible_host(&g, rec, maps, &vp, n, pts, stride, 1, a, nullptr) == MORT_OK);
    CHECK(mort_hip_volume_sample_visible_host(&g, rec, maps, &vp, n, pts, stride, threads, b, nullptr) == MORT_OK);
    CHECK(std::memcmp(a, b, 4 * n * sizeof(float)) == 0);
    const mort_volume_vis_params bad = {-1.0f, 0.05f};
    CHECK(mort_hip_volume_sample_visible_host(&g, rec, maps, &bad, n, pts, stride, 1, a, nullptr) == MORT_ERR_INVALID);
    CHECK(mort_hip_volume_sample_visible_host(&g, rec, maps, &vp, n, pts, stride, 1, maps + 4, nullptr) == MORT_ERR_INVALID);
    std::free(a); std::free(b); std::free(pts); std::free(rec); std::free(maps);
    return 0;
}

int main() {
    for (int scene : {6, 1, 7}) {
        mort_world world;
        mort_camera cam;
        CHECK(mort_world_init(&world) == 0);
        mort_scene_opts opts;
        std::memset(&opts, 0, sizeof opts);
        mort_scene_build(scene, &world, &cam, &opts);
        if (bake(&world, scene, 3, 0)) return 1;
        if (bake(&world, scene, 3, MORT_HOST_TREE)) return 1;
        mort_world_free(&world);
    }
    const int grids[2][3] = {{4, 3, 2}, {1, 1, 1}};
    for (const auto &c : grids)
        for (size_t stride : {(size_t)24, (size_t)40, (size_t)48})
            for (int mask = 0; mask < 3; mask++)
                if (sample(c, stride, mask, 3)) return 1;
    std::puts("ok");
    return 0;
}
