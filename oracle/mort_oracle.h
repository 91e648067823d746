/*
 * mort_oracle.h -- CPU oracle for the render path.  TEST INFRASTRUCTURE ONLY
 * (see the header of mort_oracle.c): never linked into the product.
 */
#ifndef MORT_ORACLE_H
#define MORT_ORACLE_H

#include "mort_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hit_record.cuh:10-19 */
typedef struct mort_oracle_hit {
    mort_vec3 p;
    mort_vec3 normal;
    int mat_idx;
    int mat_type;
    float t;
    float u, v;
    bool front_face;
} mort_oracle_hit;

typedef struct mort_oracle_stats {
    uint64_t segments;  /* world::hit calls */
    uint64_t rng_draws; /* curand_uniform calls */
} mort_oracle_stats;

/* curand_init(seed, subsequence, 0) */
void mort_oracle_rng_init(mort_rng_state *s, uint64_t seed, uint64_t subsequence);
/* setup_rng (rng.cuh:8-15): states[x + y*W] = curand_init(seed, x + y*W, 0) */
void mort_oracle_rng_seed(mort_rng_state *states, uint64_t seed, int width, int height);
unsigned mort_oracle_rng_next(mort_rng_state *s);
float mort_oracle_rng_uniform(mort_rng_state *s);          /* curand_uniform */
float mort_oracle_random_float(mort_rng_state *s);         /* rng.cuh:17-23 */
int mort_oracle_random_int(mort_rng_state *s, int mn, int mx); /* rng.cuh:31-42 */
void mort_oracle_rng_step_matrix_2p67(unsigned out[160 * 5]);

/* Camera::render (camera.cuh:178-208) over rows [row0,row1) with `nthreads`
 * host threads (rows interleaved).  rgba: W*H*4, accum: W*H*3 floats (linear
 * pixel mean after NaN scrub, before gamma) or NULL, segments_per_pixel: W*H
 * or NULL.  states advance exactly as the reference's would. */
int mort_oracle_render(const mort_world *w, const mort_camera *cam, mort_rng_state *states, int row0, int row1,
                       uint8_t *rgba, float *accum, uint32_t *segments_per_pixel, int nthreads,
                       mort_oracle_stats *stats);

/* known-answer entry points (ray7 = origin xyz, direction xyz, time) */
bool mort_oracle_world_hit(const mort_world *w, const float ray7[7], float t_min, float t_max,
                           mort_rng_state *state, mort_oracle_hit *out);
bool mort_oracle_aabb_hit(const mort_aabb *b, const float ray7[7], float t_min, float t_max);
void mort_oracle_get_ray(const mort_camera *cam, int x, int y, int s_i, int s_j, mort_rng_state *state, float ray7[7]);
void mort_oracle_ray_color(const mort_world *w, const mort_camera *cam, const float ray7[7], mort_rng_state *state, float rgb[3]);
void mort_oracle_texture_value(const mort_world *w, int tex_type, int tex_idx, float u, float v, const float p[3], float rgb[3]);
float mort_oracle_pdf_value(const mort_world *w, int type, int idx, const float origin[3], const float dir[3]);
void mort_oracle_light_random(const mort_world *w, int type, int idx, const float origin[3], mort_rng_state *state, float dir[3]);

/* Batched forms for tests that need a hit per pixel: n rays (ray7 as above, 7 floats each), per-ray t_min / t_max, the records
 * and hit flags out, over `nthreads` host threads.  object_hit_batch runs the reference's hitDispatch (objects.cuh:858-887) on
 * one object of the world alone.  `states` holds one stream per ray, or is NULL for a call that draws nothing: a call that
 * would draw (a constant medium that is reached and not skipped) without streams returns -3 and computes nothing.
 * Returns 0, or -1 for bad arguments. */
int mort_oracle_world_hit_batch(const mort_world *w, int n, const float *ray7, const float *t_min, const float *t_max,
                                mort_rng_state *states, mort_oracle_hit *out, uint8_t *hit, int nthreads);
int mort_oracle_object_hit_batch(const mort_world *w, int type, int idx, int n, const float *ray7, const float *t_min, const float *t_max,
                                 mort_rng_state *states, mort_oracle_hit *out, uint8_t *hit, int nthreads);
int mort_oracle_texture_value_batch(const mort_world *w, int n, const int *tex_type, const int *tex_idx, const float *u, const float *v,
                                    const float *p, float *rgb);

float mort_oracle_sinf(float x);
float mort_oracle_cosf(float x);
void mort_oracle_sincosf(float x, float *s, float *c);
float mort_oracle_acosf(float x);
float mort_oracle_atan2f(float y, float x);
float mort_oracle_logf(float x);
double mort_oracle_sin(double x);
/* mort_math.h over n records of 32-bit words: fn 0 mort_sqrtf, 1 mort_sqrt, 2 mort_floorf, 3 mort_fmaxf, 4 mort_fmin, 5 mort_d2i,
 * 6 mort_powi5f, 7 mort_sin, 8 mort_cos, 9 mort_sinf, 10 mort_cosf, 11 mort_sincosf, 12 mort_atan, 13 mort_atan2f, 14 mort_acosf,
 * 15 mort_logf; and the plain operators 16 fp32 x / a, 17 fp32 1 / a, 18 fp64 x / a, 19 (float) of a double, 20 (float) of a uint32_t,
 * 21 __builtin_truncf; a double is two words.  MORT_ORACLE_BATCH_OK or MORT_ORACLE_BATCH_BAD_ARGS. */
int mort_oracle_math_batch(int fn, const uint32_t *in, size_t n, uint32_t *out);
/* pdf_value_dispatch (fn 0) and random_dispatch (fn 1) over n records of 32-bit words against `w`, over `nthreads` host threads:
 * fn 0 type, idx, origin[3], direction[3] -> the pdf; fn 1 the six stream words (d, v[0..4]), type, idx, origin[3] -> the direction,
 * the six final stream words, the draw count.  A sphere, quad or list index outside the world's tables gives MORT_ORACLE_BATCH_BAD_ARGS
 * and computes nothing. */
int mort_oracle_light_batch(const mort_world *w, int fn, const uint32_t *in, size_t n, uint32_t *out, int nthreads);

/* one iteration of ray_color's loop body -- world::hit over [0.001, inf), then emission, scatter and the pdf mixture -- over n records of
 * 32-bit words, the layout of mort_hip_debug_shade_shape (debug.hip): 16 words in, 22 out (mort_oracle.c has the fields).  ray_color runs
 * the same function.  branch: NULL, or n words that name the branches each record took (material and texture tag, front face, the
 * dielectric's decisions, which half of the mixture was sampled, a zero material pdf, a non-finite normal), for a census.  A light
 * object outside the world's tables gives MORT_ORACLE_BATCH_BAD_ARGS and computes nothing. */
int mort_oracle_shade_batch(const mort_world *w, const uint32_t *in, size_t n, uint32_t *out, uint32_t *branch, int nthreads);

/* the two ends of Camera::render over n records of 32-bit words, the layouts of mort_hip_debug_camera_shape (debug.hip): fn 0 and fn 1
 * get_ray (30 words in: the six stream words, x, y, s_i, s_j, recip_sqrt_spp, defocus_angle and the six camera vectors; 14 out: the ray,
 * the six final words, the draw count), fn 2 the pixel's tail (scale, sum[3] -> accumulator[3], the pixel's four bytes as one word). */
int mort_oracle_camera_batch(int fn, const uint32_t *in, size_t n, uint32_t *out, int nthreads);

#ifdef __cplusplus
}
#endif
#endif
