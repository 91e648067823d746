/*
 * oracle/_ref driver (test infrastructure): the reference's own device code --
 * its .cuh headers, included from where they lie (REF, oracle/Makefile `ref`) --
 * compiled for the CPU through the CUDA-on-host shim in refshim/, behind C
 * entry points that mirror mort_oracle.h.  No reference source is copied into
 * this repository.  Tests compare these entry points with the oracle bit for
 * bit, so the oracle (and through it every kernel) is pinned to the
 * reference's own arithmetic rather than to a restatement of it.
 *
 * The reference keeps the scene in process globals (the dev_* arrays and the
 * global_idx statics), so there is one loaded world per process:
 * mort_ref_load_world() copies a mort_world (whose layout mort_scene.h
 * asserts) into the reference's host arrays and calls its toDevice(); the
 * other entry points use that world.  Callers serialise loads.
 */
#include <atomic>
#include <functional>
#include <mutex>
#include <new>
#include <thread>

#include <cuda_runtime.h>

#include "world.cuh"
#include "camera.cuh"

#include "mort_oracle.h"

static_assert(sizeof(sphere) == sizeof(mort_sphere) && sizeof(quad) == sizeof(mort_quad) &&
              sizeof(translate) == sizeof(mort_translate) && sizeof(rotate_y) == sizeof(mort_rotate_y) &&
              sizeof(constant_medium) == sizeof(mort_constant_medium) &&
              sizeof(hittable_list) == sizeof(mort_hittable_list) && sizeof(bvh) == sizeof(mort_bvh),
              "object layouts");
static_assert(sizeof(lambertian) == sizeof(mort_lambertian) && sizeof(metal) == sizeof(mort_metal) &&
              sizeof(dielectric) == sizeof(mort_dielectric) && sizeof(diffuse_light) == sizeof(mort_diffuse_light) &&
              sizeof(isotropic) == sizeof(mort_isotropic), "material layouts");
static_assert(sizeof(solid_color) == sizeof(mort_solid_color) && sizeof(checker_texture) == sizeof(mort_checker_texture) &&
              sizeof(image_texture) == sizeof(mort_image_texture) && sizeof(noise_texture) == sizeof(mort_noise_texture),
              "texture layouts");
static_assert(sizeof(Camera) == sizeof(mort_camera) && sizeof(curandState) == sizeof(mort_rng_state) &&
              sizeof(vec3) == sizeof(mort_vec3) && sizeof(aabb) == sizeof(mort_aabb), "camera / rng / math layouts");

namespace {

std::mutex g_mu;
world *g_world;                                 /* the reference's host arrays, allocated by its constructor */
bool g_loaded;                                  /* a world is loaded and uploaded (mort_ref_load_world) */
std::vector<cudaTextureObject_t> g_textures;    /* texture objects of the loaded image textures */
const int kMaxThreads = 16;

template <class T>
bool copy_in(T *dst, int &count, const void *src, int n, int cap) {
    if (n < 0 || n > cap || (n > 0 && !src)) return false;
    if (n) memcpy(static_cast<void *>(dst), src, size_t(n) * sizeof(T));
    count = n;
    return true;
}

void set_global_indices(const world &d) { /* as if the loaded objects had just been constructed (the textures' are private) */
    sphere::global_idx = d.objs.num_spheres;
    quad::global_idx = d.objs.num_quads;
    translate::global_idx = d.objs.num_translates;
    rotate_y::global_idx = d.objs.num_rotate_y;
    constant_medium::global_idx = d.objs.num_constant_medium;
    hittable_list::global_idx = d.objs.num_hittable_list;
    bvh::global_idx = d.objs.num_bvh;
    lambertian::global_idx = d.mats.num_lambertians;
    metal::global_idx = d.mats.num_metals;
    dielectric::global_idx = d.mats.num_dielectrics;
    diffuse_light::global_idx = d.mats.num_diffuse_lights;
    isotropic::global_idx = d.mats.num_isotropics;
}

/* the mort_world's objects into the reference's host arrays (no textures, no upload) */
int load_objects(const mort_world *w) {
    if (!g_world) g_world = new world();
    world &d = *g_world;
    const mort_world_objects &o = w->objs;
    if (!copy_in(d.objs.host_sphere, d.objs.num_spheres, o.host_sphere, o.num_spheres, NUM_SPHERES) ||
        !copy_in(d.objs.host_quad, d.objs.num_quads, o.host_quad, o.num_quads, NUM_QUADS) ||
        !copy_in(d.objs.host_translate, d.objs.num_translates, o.host_translate, o.num_translates, NUM_TRANSLATE) ||
        !copy_in(d.objs.host_rotate_y, d.objs.num_rotate_y, o.host_rotate_y, o.num_rotate_y, NUM_ROTATE_Y) ||
        !copy_in(d.objs.host_constant_medium, d.objs.num_constant_medium, o.host_constant_medium, o.num_constant_medium,
                 NUM_CONSTANT_MEDIUM) ||
        !copy_in(d.objs.host_hittable_list, d.objs.num_hittable_list, o.host_hittable_list, o.num_hittable_list,
                 NUM_HITTABLE_LIST) ||
        !copy_in(d.objs.host_bvh, d.objs.num_bvh, o.host_bvh, o.num_bvh, NUM_BVH))
        return -1;
    d.bvh_mode = w->bvh_mode;
    return 0;
}

/* Per-bounce scratch of Camera::ray_color for one pixel: it indexes
 * [x * bounce_limit + y * image_width * bounce_limit + iter], so the pointers
 * are biased by that pixel's base (as integers: the buffers are per thread). */
struct Scratch {
    std::vector<color> att, emi;
    std::vector<float> spdf, pdf;
    explicit Scratch(int bounce_limit)
        : att(size_t(bounce_limit) + 1), emi(size_t(bounce_limit) + 1), spdf(size_t(bounce_limit) + 1),
          pdf(size_t(bounce_limit) + 1) {}
    template <class T>
    static T *bias(T *p, long base) { return reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(p) - uintptr_t(base) * sizeof(T)); }
    void point(Camera &c, int x, int y) {
        const long base = long(x) * c.bounce_limit + long(y) * c.image_width * c.bounce_limit;
        c.recursionAttenuation = bias(att.data(), base);
        c.recursionEmission = bias(emi.data(), base);
        c.recursionScatteringPdf = bias(spdf.data(), base);
        c.recursionPdf = bias(pdf.data(), base);
    }
};

bool camera_ok(const mort_camera *mc) {
    return mc && mc->image_width > 0 && mc->image_height > 0 && mc->bounce_limit >= 0 &&
           mc->bounce_limit <= MORT_MAX_BOUNCE_LIMIT && mc->sqrt_spp >= 0;
}

Camera camera_from(const mort_camera *mc) {
    Camera c;
    memcpy(static_cast<void *>(&c), mc, sizeof c);
    return c;
}

ray ray_from(const float r7[7]) { return ray(point3(r7[0], r7[1], r7[2]), vec3(r7[3], r7[4], r7[5]), r7[6]); }

void ray_to(const ray &r, float r7[7]) {
    const point3 o = r.origin();
    const vec3 d = r.direction();
    const float v[7] = {o.x(), o.y(), o.z(), d.x(), d.y(), d.z(), r.time()};
    memcpy(r7, v, sizeof v);
}

void run_threads(int nthreads, const std::function<void(int)> &f) {
    if (nthreads < 1) nthreads = 1;
    if (nthreads > kMaxThreads) nthreads = kMaxThreads;
    std::vector<std::thread> th;
    for (int t = 1; t < nthreads; t++) th.emplace_back(f, t);
    f(0);
    for (auto &x : th) x.join();
}

}  // namespace

extern "C" {

/* 0, or -1 (a count beyond the reference's capacity), -2 (an image texture
 * whose scanline is not a multiple of the 32-byte pitch alignment: the
 * reference's own upload overruns its buffer there, textures.cuh:95-111). */
int mort_ref_load_world(const mort_world *w) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_loaded = false;
    if (!w) return -1;
    if (load_objects(w) != 0) return -1;
    world &d = *g_world;
    const mort_world_materials &m = w->mats;
    const mort_world_textures &t = w->texs;
    if (!copy_in(d.mats.host_lambertian, d.mats.num_lambertians, m.host_lambertian, m.num_lambertians, NUM_LAMBERTIANS) ||
        !copy_in(d.mats.host_metal, d.mats.num_metals, m.host_metal, m.num_metals, NUM_METALS) ||
        !copy_in(d.mats.host_dielectric, d.mats.num_dielectrics, m.host_dielectric, m.num_dielectrics, NUM_DIELECTRICS) ||
        !copy_in(d.mats.host_diffuse_light, d.mats.num_diffuse_lights, m.host_diffuse_light, m.num_diffuse_lights,
                 NUM_DIFFUSE_LIGHTS) ||
        !copy_in(d.mats.host_isotropic, d.mats.num_isotropics, m.host_isotropic, m.num_isotropics, NUM_ISOTROPICS) ||
        !copy_in(d.texs.host_solid_color, d.texs.num_solid_colors, t.host_solid_color, t.num_solid_colors, NUM_SOLID_COLOR) ||
        !copy_in(d.texs.host_checker_texture, d.texs.num_checker_textures, t.host_checker_texture, t.num_checker_textures,
                 NUM_CHECKER_TEXTURE) ||
        !copy_in(d.texs.host_image_texture, d.texs.num_image_textures, t.host_image_texture, t.num_image_textures,
                 NUM_IMAGE_TEXTURE) ||
        !copy_in(d.texs.host_noise_texture, d.texs.num_noise_textures, t.host_noise_texture, t.num_noise_textures,
                 NUM_NOISE_TEXTURE))
        return -1;
    for (cudaTextureObject_t o : g_textures) cudaDestroyTextureObject(o);
    g_textures.clear();
    /* image_texture holds its cudaTextureObject_t where mort_image_texture holds
     * the texel pointer (first member of both): a pitch-2D texture over the
     * tightly packed texels, whose pitch is what the reference's upload makes
     * when the scanline is a multiple of the alignment */
    for (int i = 0; i < t.num_image_textures; i++) {
        const mort_image_texture &src = t.host_image_texture[i];
        if (src.height <= 0) continue; /* the reference returns its missing-image colour before sampling */
        const size_t scanline = size_t(src.width) * 3;
        if (src.width <= 0 || !src.texels || scanline % 32 != 0) return -2;
        cudaResourceDesc res;
        memset(&res, 0, sizeof res);
        res.resType = cudaResourceTypePitch2D;
        res.res.pitch2D.devPtr = const_cast<unsigned char *>(src.texels);
        res.res.pitch2D.width = scanline;
        res.res.pitch2D.height = size_t(src.height);
        res.res.pitch2D.desc = cudaCreateChannelDesc<unsigned char>();
        res.res.pitch2D.pitchInBytes = scanline;
        cudaTextureDesc tex;
        memset(&tex, 0, sizeof tex);
        cudaTextureObject_t obj = 0;
        if (cudaCreateTextureObject(&obj, &res, &tex, nullptr) != cudaSuccess) return -2;
        g_textures.push_back(obj);
        memcpy(static_cast<void *>(&d.texs.host_image_texture[i]), &obj, sizeof obj);
    }
    d.toDevice();
    set_global_indices(d);
    g_loaded = true;
    return 0;
}

/* setup_rng (rng.cuh) for every pixel of a W x H frame */
void mort_ref_rng_seed(mort_rng_state *states, uint64_t seed, int width, int height, int nthreads) {
    run_threads(nthreads, [&](int tid) {
        int n = nthreads < 1 ? 1 : (nthreads > kMaxThreads ? kMaxThreads : nthreads);
        blockDim = dim3{1, 1, 1};
        threadIdx = dim3{0, 0, 0};
        for (int y = tid; y < height; y += n)
            for (int x = 0; x < width; x++) {
                blockIdx = dim3{unsigned(x), unsigned(y), 0};
                setup_rng(reinterpret_cast<curandState *>(states), (unsigned long)seed, width);
            }
    });
}

/* Rows [row0, row1) of a frame.  rgba (W*H*4) through the reference's own
 * Camera::render, advancing `states` in place; accum (W*H*3 floats, or NULL):
 * the pixel mean after the NaN scrub, before gamma, through its get_ray /
 * ray_color from the same start states.  0, -1 (arguments), or -3 when the two
 * passes leave different final states. */
int mort_ref_render(const mort_camera *mc, mort_rng_state *states, int row0, int row1, uint8_t *rgba, float *accum,
                    int nthreads) {
    if (!g_loaded || !camera_ok(mc) || !states || !rgba) return -1;
    const int W = mc->image_width, H = mc->image_height;
    if (row0 < 0) row0 = 0;
    if (row1 > H) row1 = H;
    const Camera cam = camera_from(mc);
    std::vector<mort_rng_state> second;
    if (accum) second.assign(states, states + size_t(W) * H);
    int n = nthreads < 1 ? 1 : (nthreads > kMaxThreads ? kMaxThreads : nthreads);
    std::atomic<int> mismatch{0};
    run_threads(n, [&](int tid) {
        Camera c = cam;
        Scratch s(c.bounce_limit);
        curandState *st = reinterpret_cast<curandState *>(states);
        curandState *st2 = reinterpret_cast<curandState *>(second.data());
        blockDim = dim3{1, 1, 1};
        threadIdx = dim3{0, 0, 0};
        for (int y = row0 + tid; y < row1; y += n)
            for (int x = 0; x < W; x++) {
                const int offset = x + y * W;
                s.point(c, x, y);
                blockIdx = dim3{unsigned(x), unsigned(y), 0};
                c.render(reinterpret_cast<uchar4 *>(rgba), st, *g_world);
                if (!accum) continue;
                color pixel_color(0, 0, 0);
                for (int s_j = 0; s_j < c.sqrt_spp; s_j++)
                    for (int s_i = 0; s_i < c.sqrt_spp; s_i++) {
                        ray r = c.get_ray(x, y, st2, offset, s_i, s_j);
                        pixel_color += c.ray_color(r, st2, offset, x, y, *g_world);
                    }
                pixel_color *= c.pixel_samples_scale;
                for (int k = 0; k < 3; k++) {
                    float v = pixel_color[k];
                    accum[3 * size_t(offset) + k] = (v != v) ? 0.0f : v;
                }
                if (st2[offset].d != st[offset].d || memcmp(st2[offset].v, st[offset].v, sizeof st[offset].v) != 0)
                    mismatch.store(1);
            }
    });
    return mismatch.load() ? -3 : 0;
}

/* The per-ray entry points below use the loaded world: before the first
 * mort_ref_load_world they return false / -1 / NaN and touch nothing. */

/* world::hit (world.cuh) on one ray; the full hit_record */
bool mort_ref_world_hit(const float ray7[7], float t_min, float t_max, mort_rng_state *state, mort_oracle_hit *out) {
    if (!g_loaded) return false;
    hit_record rec;
    memset(static_cast<void *>(&rec), 0, sizeof rec);
    const bool h = g_world->hit(ray_from(ray7), t_min, t_max, rec, reinterpret_cast<curandState *>(state), 0);
    memset(out, 0, sizeof *out);
    memcpy(out->p.e, &rec.p, sizeof out->p.e);
    memcpy(out->normal.e, &rec.normal, sizeof out->normal.e);
    out->mat_idx = rec.mat_idx;
    out->mat_type = rec.mat_type;
    out->t = rec.t;
    out->u = rec.u;
    out->v = rec.v;
    out->front_face = rec.front_face;
    return h;
}

void mort_ref_get_ray(const mort_camera *mc, int x, int y, int s_i, int s_j, mort_rng_state *state, float ray7[7]) {
    const Camera c = camera_from(mc);
    ray_to(c.get_ray(x, y, reinterpret_cast<curandState *>(state), 0, s_i, s_j), ray7);
}

/* Camera::initialize (camera.cuh:47-84) on the camera's input fields; every field comes back */
void mort_ref_camera_initialize(mort_camera *mc) {
    Camera c = camera_from(mc);
    c.initialize();
    memcpy(mc, static_cast<const void *>(&c), sizeof c);
}

/* rotate_around (vec3.cuh:215-227) */
void mort_ref_rotate_around(const float vec[3], const float axis[3], float theta, float out[3]) {
    const vec3 r = rotate_around(vec3(vec[0], vec[1], vec[2]), vec3(axis[0], axis[1], axis[2]), theta);
    memcpy(out, &r, 3 * sizeof(float));
}

/* One tick of mort.cu's input() (lines 51-90), which polls Win32 and cannot be compiled: its statements restated over the reference's
 * own vec3 operators, rotate_around and initialize(), with the polls replaced by their results (keys: 1 W, 2 S, 4 A, 8 D). */
void mort_ref_camera_input(mort_camera *mc, int keys, int mouseDeltaX, int mouseDeltaY, int left) {
    Camera cam = camera_from(mc);
    if (keys & 1) { cam.lookat += -(cam.w); cam.lookfrom += -(cam.w); }
    if (keys & 2) { cam.lookat += cam.w; cam.lookfrom += cam.w; }
    if (keys & 4) { cam.lookat += -(cam.u); cam.lookfrom += -(cam.u); }
    if (keys & 8) { cam.lookat += cam.u; cam.lookfrom += cam.u; }
    if (left) {
        if (mouseDeltaX != 0) {
            vec3 cam_direction = cam.lookat - cam.lookfrom;
            vec3 rotated = rotate_around(cam_direction, cam.vup, -mouseDeltaX / 500.0);
            cam.lookat = cam.lookfrom + rotated;
        }
        if (mouseDeltaY != 0) {
            vec3 cam_direction = cam.lookat - cam.lookfrom;
            vec3 rotated = rotate_around(cam_direction, cam.u, -mouseDeltaY / 500.0);
            cam.lookat = cam.lookfrom + rotated;
        }
    }
    cam.initialize();
    memcpy(mc, static_cast<const void *>(&cam), sizeof cam);
}

/* the tan (fn 0), cos (1) and sin (2) of a float as this translation unit resolves them: the overloads initialize() and rotate_around call */
float mort_ref_libm(int fn, float x) {
    return fn == 0 ? tan(x) : fn == 1 ? cos(x) : sin(x);
}

/* Camera::ray_color for one ray of pixel (0, 0) */
int mort_ref_ray_color(const mort_camera *mc, const float ray7[7], mort_rng_state *state, float rgb[3]) {
    if (!g_loaded || !camera_ok(mc)) return -1;
    Camera c = camera_from(mc);
    Scratch s(c.bounce_limit);
    s.point(c, 0, 0);
    const color col = c.ray_color(ray_from(ray7), reinterpret_cast<curandState *>(state), 0, 0, 0, *g_world);
    memcpy(rgb, &col, 3 * sizeof(float));
    return 0;
}

int mort_ref_texture_value(int tex_type, int tex_idx, float u, float v, const float p[3], float rgb[3]) {
    if (!g_loaded) return -1;
    const color col = valueDispatch(tex_type, tex_idx, u, v, point3(p[0], p[1], p[2]));
    memcpy(rgb, &col, 3 * sizeof(float));
    return 0;
}

float mort_ref_pdf_value(int type, int idx, const float origin[3], const float dir[3]) {
    if (!g_loaded) return std::numeric_limits<float>::quiet_NaN();
    return pdfValueDispatch(type, idx, point3(origin[0], origin[1], origin[2]), vec3(dir[0], dir[1], dir[2]));
}

int mort_ref_light_random(int type, int idx, const float origin[3], mort_rng_state *state, float dir[3]) {
    if (!g_loaded) return -1;
    const vec3 d = randomDispatch(type, idx, point3(origin[0], origin[1], origin[2]), reinterpret_cast<curandState *>(state), 0);
    memcpy(dir, &d, 3 * sizeof(float));
    return 0;
}

/* The reference's host BVH build (objects.cuh bvh::bvh) over a copy of list
 * `li` of a pre-build world -- its scenes sort a local copy of the list --
 * then, if `hierarchy`, bvh::build_aabb_hierarchy(0).  Like mort_add_bvh it
 * appends the BVH to `w` and sets bvh_mode; the sort's same-type swaps land in
 * w's object arrays.  Returns the BVH's index, or -1. */
int mort_ref_add_bvh(mort_world *w, int li, bool skip, int hierarchy) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_loaded = false; /* the host arrays below are no longer the uploaded world's */
    if (!w || load_objects(w) != 0) return -1;
    world &d = *g_world;
    if (li < 0 || li >= d.objs.num_hittable_list || d.objs.num_bvh >= NUM_BVH) return -1;
    if (d.objs.host_hittable_list[li].num_objs < 1) return -1; /* the reference's loop never ends on an empty list */
    set_global_indices(d);
    hittable_list *list = new hittable_list(d.objs.host_hittable_list[li]);
    void *mem = calloc(1, sizeof(bvh)); /* zeroed like mort_add_bvh's node arrays */
    bvh *b = new (mem) bvh(*list, d.objs, skip);
    if (hierarchy) b->build_aabb_hierarchy(0, d.objs);
    d.add(*b);
    const int bi = d.objs.num_bvh - 1;
    free(mem);
    delete list;
    mort_world_objects &o = w->objs;
    memcpy(o.host_sphere, d.objs.host_sphere, size_t(d.objs.num_spheres) * sizeof(sphere));
    memcpy(o.host_quad, d.objs.host_quad, size_t(d.objs.num_quads) * sizeof(quad));
    memcpy(o.host_translate, d.objs.host_translate, size_t(d.objs.num_translates) * sizeof(translate));
    memcpy(o.host_rotate_y, d.objs.host_rotate_y, size_t(d.objs.num_rotate_y) * sizeof(rotate_y));
    memcpy(o.host_constant_medium, d.objs.host_constant_medium, size_t(d.objs.num_constant_medium) * sizeof(constant_medium));
    memcpy(static_cast<void *>(&o.host_bvh[bi]), &d.objs.host_bvh[bi], sizeof(bvh));
    o.num_bvh = d.objs.num_bvh;
    w->bvh_mode = d.bvh_mode;
    return bi;
}

}  // extern "C"
