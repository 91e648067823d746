/*
 * mort_oracle.c -- CPU ORACLE for the render path.  TEST INFRASTRUCTURE ONLY.
 *
 * A plain-C restatement of the reference's device code, function by function,
 * in the reference's own structure (tagged dispatch, recursive instances,
 * explicit BVH traversal, per-bounce stack + backward unwind), operating
 * directly on the mort_world / mort_camera structs.  Only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this; the
 * product (libmort_hip.so, the CLI) never links or calls it.
 *
 * PARITY STATUS: pinned to the reference's own device code.  The reference's
 * .cuh headers, compiled for the CPU through the shim in refshim/ (ref_render.cpp,
 * oracle/_ref/libmort_ref.so), agree with this file bit for bit on renders,
 * per-ray known answers and the BVH build (tests/test_reference_pin.py); the
 * recorded digests (tests/golden/ref_pin.npz) hold that where the reference is
 * absent.  Shared with that build and so not pinned by it: cuRAND's seed-scramble
 * constants, mort_math.h in place of CUDA's libm, no FMA contraction, MSVC's
 * host tan and the host scene builders.  Also pinned: the XORWOW recurrence and
 * 2^67 skip against rocRAND's engine, closed-form known answers, goldens.
 * Third-party pieces restated from their published definitions:
 *   cuRAND XORWOW (CUDA 11.3/13.2, curand_kernel.h: curand_init, curand,
 *   curand_uniform) -- call sites rng.cuh:14,20,34.
 *
 * Numerical contract: expressions are evaluated in the
 * precision C++ gives them in the reference (unsuffixed literals are double),
 * compiled with -ffp-contract=off; libm calls go through include/mort_math.h.
 * Unspecified sibling-argument evaluation order in device code
 * (vec3.cuh:139-146,164; objects.cuh:233) is taken left to right.
 */
#include "mort_oracle.h"
#include "mort_math.h"

#include <math.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

/* ------------------------------------------------------------------ vec3 (vec3.cuh) */
typedef mort_vec3 vec3;
static inline vec3 V(float x, float y, float z) { vec3 r = {{x, y, z}}; return r; }
static inline vec3 vadd(vec3 a, vec3 b) { return V(a.e[0] + b.e[0], a.e[1] + b.e[1], a.e[2] + b.e[2]); }
static inline vec3 vsub(vec3 a, vec3 b) { return V(a.e[0] - b.e[0], a.e[1] - b.e[1], a.e[2] - b.e[2]); }
static inline vec3 vmul(vec3 a, vec3 b) { return V(a.e[0] * b.e[0], a.e[1] * b.e[1], a.e[2] * b.e[2]); }
static inline vec3 vneg(vec3 a) { return V(-a.e[0], -a.e[1], -a.e[2]); }
static inline vec3 vscale(float t, vec3 v) { return V(t * v.e[0], t * v.e[1], t * v.e[2]); } /* vec3.cuh:99-101 */
static inline vec3 vdiv(vec3 v, float t) { return vscale(1 / t, v); }                         /* vec3.cuh:109-112 */
static inline float vdot(vec3 u, vec3 v) { return u.e[0] * v.e[0] + u.e[1] * v.e[1] + u.e[2] * v.e[2]; }
static inline float vlen2(vec3 a) { return a.e[0] * a.e[0] + a.e[1] * a.e[1] + a.e[2] * a.e[2]; }
static inline float vlen(vec3 a) { return mort_sqrtf(vlen2(a)); }
static inline vec3 vunit(vec3 a) { return vdiv(a, vlen(a)); }
static inline vec3 vcross(vec3 u, vec3 v) {
    return V(u.e[1] * v.e[2] - u.e[2] * v.e[1], u.e[2] * v.e[0] - u.e[0] * v.e[2], u.e[0] * v.e[1] - u.e[1] * v.e[0]);
}

typedef struct { vec3 orig, dir; float t; } ray; /* ray.cuh */
static inline vec3 ray_at(const ray *r, double t) { return vadd(r->orig, vscale((float)t, r->dir)); } /* ray.cuh:17-19 */

typedef mort_oracle_hit hit_record; /* hit_record.cuh:10-19 */

static inline void set_face_normal(hit_record *rec, const ray *r, vec3 outward) { /* hit_record.cuh:20-23 */
    rec->front_face = vdot(r->dir, outward) < 0;
    rec->normal = rec->front_face ? outward : vneg(outward);
}

/* ------------------------------------------------------------------ XORWOW (rng.cuh + cuRAND) */

static inline unsigned xorwow_next(mort_rng_state *s) {
    unsigned t = s->v[0] ^ (s->v[0] >> 2);
    s->v[0] = s->v[1]; s->v[1] = s->v[2]; s->v[2] = s->v[3]; s->v[3] = s->v[4];
    s->v[4] = (s->v[4] ^ (s->v[4] << 4)) ^ (t ^ (t << 1));
    s->d += 362437u;
    return s->v[4] + s->d;
}

/* curand_uniform: x * 2^-32 + 2^-33 in fp32, in (0, 1].  The literal
 * 2.3283064e-10f is exactly 2^-32, so the product is exact and the result does
 * not depend on whether the compiler fuses the multiply-add. */
static inline float curand_uniform_f(mort_rng_state *s) {
    unsigned x = xorwow_next(s);
    return (float)x * 2.3283064e-10f + (2.3283064e-10f / 2.0f);
}

typedef struct { mort_rng_state *st; uint64_t draws; } rng_t;

static inline float random_float(rng_t *g) { /* rng.cuh:17-23 */
    g->draws++;
    return (float)(1.0 - curand_uniform_f(g->st));
}
static inline float random_float_range(rng_t *g, float mn, float mx) { /* rng.cuh:25-29 */
    float base = random_float(g);
    return base * (mx - mn) + mn;
}
static inline int random_int(rng_t *g, int mn, int mx) { /* rng.cuh:31-42 */
    g->draws++;
    float random = curand_uniform_f(g->st);
    random = (float)(random * (mx - mn + 0.999999));
    random += mn;
    return mort_f2i(truncf(random));
}

/* 160x160 GF(2) step matrix powers; row i = image of state bit i. */
typedef struct { unsigned row[160][5]; } xmat;
static void xmat_apply(const xmat *m, const unsigned v[5], unsigned out[5]) {
    unsigned r[5] = {0, 0, 0, 0, 0};
    for (int w = 0; w < 5; w++)
        for (int b = 0; b < 32; b++)
            if (v[w] >> b & 1u) {
                const unsigned *row = m->row[w * 32 + b];
                r[0] ^= row[0]; r[1] ^= row[1]; r[2] ^= row[2]; r[3] ^= row[3]; r[4] ^= row[4];
            }
    memcpy(out, r, sizeof r);
}
static void xmat_square(const xmat *a, xmat *out) {
    for (int i = 0; i < 160; i++) xmat_apply(a, a->row[i], out->row[i]);
}

#define XORWOW_SEQ_LEVELS 32
static xmat g_seq[XORWOW_SEQ_LEVELS]; /* A^(2^67 * 4^k) */
static pthread_once_t g_seq_once = PTHREAD_ONCE_INIT;
static void build_seq_matrices(void) {
    xmat *a = malloc(sizeof *a), *b = malloc(sizeof *b);
    for (int i = 0; i < 160; i++) { /* one step applied to each basis vector */
        mort_rng_state s;
        memset(&s, 0, sizeof s);
        s.v[i / 32] = 1u << (i % 32);
        xorwow_next(&s);
        memcpy(a->row[i], s.v, sizeof s.v);
    }
    for (int k = 0; k < 67; k++) { xmat_square(a, b); xmat *t = a; a = b; b = t; }
    g_seq[0] = *a;
    for (int k = 1; k < XORWOW_SEQ_LEVELS; k++) {
        xmat_square(&g_seq[k - 1], b);
        xmat_square(b, &g_seq[k]);
    }
    free(a); free(b);
}

void mort_oracle_rng_init(mort_rng_state *s, uint64_t seed, uint64_t subsequence) { /* curand_init, offset 0 */
    pthread_once(&g_seq_once, build_seq_matrices);
    memset(s, 0, sizeof *s);
    unsigned s0 = (unsigned)seed ^ 0xaad26b49u;
    unsigned s1 = (unsigned)(seed >> 32) ^ 0xf7dcefddu;
    unsigned t0 = 1099087573u * s0;
    unsigned t1 = 2591861531u * s1;
    s->d = 6615241u + t1 + t0;
    s->v[0] = 123456789u + t0;
    s->v[1] = 362436069u ^ t0;
    s->v[2] = 521288629u + t1;
    s->v[3] = 88675123u ^ t1;
    s->v[4] = 5783321u + t0;
    uint64_t p = subsequence;
    for (int k = 0; p && k < XORWOW_SEQ_LEVELS; k++, p >>= 2)
        for (unsigned t = 0; t < (p & 3u); t++) xmat_apply(&g_seq[k], s->v, s->v);
    /* d is unchanged: 2^67 steps advance it by a multiple of 2^32 */
}

void mort_oracle_rng_seed(mort_rng_state *states, uint64_t seed, int width, int height) {
    /* rng.cuh:8-15: states[x + y*W] = curand_init(seed, x + y*W, 0); consecutive
     * subsequences differ by one application of A^(2^67). */
    size_t n = (size_t)width * height;
    if (n == 0) return;
    mort_oracle_rng_init(&states[0], seed, 0);
    for (size_t i = 1; i < n; i++) {
        states[i] = states[i - 1];
        xmat_apply(&g_seq[0], states[i - 1].v, states[i].v);
    }
}

unsigned mort_oracle_rng_next(mort_rng_state *s) { return xorwow_next(s); }
float mort_oracle_rng_uniform(mort_rng_state *s) { return curand_uniform_f(s); }
float mort_oracle_random_float(mort_rng_state *s) { rng_t g = {s, 0}; return random_float(&g); }
int mort_oracle_random_int(mort_rng_state *s, int mn, int mx) { rng_t g = {s, 0}; return random_int(&g, mn, mx); }
void mort_oracle_rng_step_matrix_2p67(unsigned out[160 * 5]) {
    pthread_once(&g_seq_once, build_seq_matrices);
    memcpy(out, g_seq[0].row, sizeof g_seq[0].row);
}

/* ------------------------------------------------------------------ random directions (vec3.cuh:138-189) */

static vec3 random_vec_range(rng_t *g, float mn, float mx) { /* vec3.cuh:143-146, left to right */
    float a = random_float_range(g, mn, mx);
    float b = random_float_range(g, mn, mx);
    float c = random_float_range(g, mn, mx);
    return V(a, b, c);
}
static vec3 random_in_unit_sphere(rng_t *g) {
    for (;;) {
        vec3 p = random_vec_range(g, -1, 1);
        if (vlen2(p) >= 1) continue;
        return p;
    }
}
static vec3 random_unit_vector(rng_t *g) { return vunit(random_in_unit_sphere(g)); }
static vec3 random_in_unit_disk(rng_t *g) {
    for (;;) {
        float a = random_float_range(g, -1, 1);
        float b = random_float_range(g, -1, 1);
        vec3 p = V(a, b, 0);
        if (vlen2(p) < 1) return p;
    }
}
static vec3 random_cosine_direction(rng_t *g) { /* vec3.cuh:180-189 */
    float r1 = random_float(g);
    float r2 = random_float(g);
    float phi = (float)(2 * 3.1415926 * r1);
    float x = mort_cosf(phi) * mort_sqrtf(r2);
    float y = mort_sinf(phi) * mort_sqrtf(r2);
    float z = mort_sqrtf(1 - r2);
    return V(x, y, z);
}
static vec3 reflect(vec3 v, vec3 n) { return vsub(v, vscale(2 * vdot(v, n), n)); } /* vec3.cuh:192-194 */
static vec3 refract(vec3 uv, vec3 n, float etai_over_etat) { /* vec3.cuh:197-203 */
    double cos_theta = mort_fmin((double)vdot(vneg(uv), n), 1.0);
    vec3 r_out_perp = vscale(etai_over_etat, vadd(uv, vscale((float)cos_theta, n)));
    vec3 r_out_parallel = vscale((float)(-mort_sqrt(mort_fabs(1.0 - vlen2(r_out_perp)))), n);
    return vadd(r_out_perp, r_out_parallel);
}
static float reflectance(float cosine, float ref_idx) { /* vec3.cuh:206-212 */
    float r0 = (1 - ref_idx) / (1 + ref_idx);
    r0 = r0 * r0;
    return r0 + (1 - r0) * mort_powi5f(1 - cosine);
}

/* ------------------------------------------------------------------ onb (onb.cuh) */
typedef struct { vec3 axis[3]; } onb;
static void onb_build_from_w(onb *o, vec3 w) {
    vec3 unit_w = vunit(w);
    vec3 a = (mort_fabsf(unit_w.e[0]) > 0.9) ? V(0, 1, 0) : V(1, 0, 0);
    vec3 v = vunit(vcross(unit_w, a));
    vec3 u = vcross(unit_w, v);
    o->axis[0] = u; o->axis[1] = v; o->axis[2] = unit_w;
}
static vec3 onb_local(const onb *o, vec3 a) {
    return vadd(vadd(vscale(a.e[0], o->axis[0]), vscale(a.e[1], o->axis[1])), vscale(a.e[2], o->axis[2]));
}

/* ------------------------------------------------------------------ objects (objects.cuh, aabb.cuh) */

typedef struct { const mort_world *w; rng_t *g; uint64_t segments; } ctx_t;

static bool hit_dispatch(ctx_t *c, int type, int idx, const ray *r, float t_min, float t_max, hit_record *rec);

static bool aabb_hit(const mort_aabb *b, const ray *r, float t_min, float t_max) { /* aabb.cuh:37-59 */
    const mort_interval ax[3] = {b->x, b->y, b->z};
    for (int a = 0; a < 3; a++) {
        double invD = 1.0 / r->dir.e[a];
        float orig = r->orig.e[a];
        double t0 = (ax[a].imin - orig) * invD;
        double t1 = (ax[a].imax - orig) * invD;
        if (invD < 0) { double aux = t0; t0 = t1; t1 = aux; }
        if (t0 > t_min) t_min = (float)t0;
        if (t1 < t_max) t_max = (float)t1;
        if (t_max <= t_min) return false;
    }
    return true;
}

static vec3 sphere_center(const mort_sphere *s, float time) { /* objects.cuh:90-97 */
    if (!s->moves) return s->center1;
    return vadd(s->center1, vscale(time, s->center_vec));
}
static void sphere_compute_uv(vec3 p, float *u, float *v) { /* objects.cuh:101-108 */
    float theta = mort_acosf(-p.e[1]);
    float phi = (float)(mort_atan2f(-p.e[2], p.e[0]) + 3.141592565);
    *u = (float)(phi / (2.0 * 3.141592565));
    *v = (float)(theta / 3.141592565);
}
static bool sphere_hit(const mort_sphere *s, const ray *r, float t_min, float t_max, hit_record *rec) { /* objects.cuh:60-88 */
    const vec3 oc = vsub(r->orig, sphere_center(s, r->t));
    const float a = vlen2(r->dir);
    const float half_b = vdot(oc, r->dir);
    const float c = vlen2(oc) - s->radius * s->radius;
    const float discriminant = half_b * half_b - a * c;
    if (discriminant < 0) return false;
    const float sqrtd = mort_sqrtf(discriminant);
    float root = (-half_b - sqrtd) / a;
    if (root < t_min || t_max < root) {
        root = (-half_b + sqrtd) / a;
        if (root < t_min || t_max < root) return false;
    }
    rec->t = root;
    rec->p = ray_at(r, rec->t);
    const vec3 outward_normal = vdiv(vsub(rec->p, sphere_center(s, r->t)), s->radius);
    set_face_normal(rec, r, outward_normal);
    sphere_compute_uv(outward_normal, &rec->u, &rec->v);
    rec->mat_type = s->mat_type;
    rec->mat_idx = s->mat_idx;
    return true;
}
static bool quad_hit(const mort_quad *q, const ray *r, float t_min, float t_max, hit_record *rec) { /* objects.cuh:190-215 */
    float denom = vdot(q->normal, r->dir);
    if (mort_fabsf(denom) < 1e-8) return false;
    float t = (q->D - vdot(q->normal, r->orig)) / denom;
    if (t < t_min || t > t_max) return false;
    vec3 intersection = ray_at(r, t);
    vec3 planar = vsub(intersection, q->Q);
    float alpha = vdot(q->w, vcross(planar, q->v));
    float beta = vdot(q->w, vcross(q->u, planar));
    if ((alpha < 0) || (alpha > 1) || (beta < 0) || (beta > 1)) return false;
    rec->t = t;
    rec->p = intersection;
    rec->mat_type = q->mat_type;
    rec->mat_idx = q->mat_idx;
    rec->u = alpha;
    rec->v = beta;
    set_face_normal(rec, r, q->normal);
    return true;
}
static bool translate_hit(ctx_t *c, const mort_translate *t, const ray *r, float t_min, float t_max, hit_record *rec) {
    ray offset_r = {vsub(r->orig, t->offset), r->dir, r->t}; /* objects.cuh:268-278 */
    if (!hit_dispatch(c, t->obj_type, t->obj_idx, &offset_r, t_min, t_max, rec)) return false;
    rec->p = vadd(rec->p, t->offset);
    return true;
}
static bool rotate_y_hit(ctx_t *c, const mort_rotate_y *ro, const ray *r, float t_min, float t_max, hit_record *rec) {
    vec3 origin = r->orig, direction = r->dir; /* objects.cuh:334-366 */
    const float ct = ro->cos_theta, st = ro->sin_theta;
    origin.e[0] = ct * r->orig.e[0] - st * r->orig.e[2];
    origin.e[2] = st * r->orig.e[0] + ct * r->orig.e[2];
    direction.e[0] = ct * r->dir.e[0] - st * r->dir.e[2];
    direction.e[2] = st * r->dir.e[0] + ct * r->dir.e[2];
    ray rotated = {origin, direction, r->t};
    if (!hit_dispatch(c, ro->obj_type, ro->obj_idx, &rotated, t_min, t_max, rec)) return false;
    vec3 p = rec->p;
    p.e[0] = ct * rec->p.e[0] + st * rec->p.e[2];
    p.e[2] = -st * rec->p.e[0] + ct * rec->p.e[2];
    vec3 n = rec->normal;
    n.e[0] = ct * rec->normal.e[0] + st * rec->normal.e[2];
    n.e[2] = -st * rec->normal.e[0] + ct * rec->normal.e[2];
    rec->p = p;
    rec->normal = n;
    return true;
}
static bool constant_medium_hit(ctx_t *c, const mort_constant_medium *m, const ray *r, float t_min, float t_max, hit_record *rec) {
    hit_record rec1, rec2; /* objects.cuh:396-434 */
    memset(&rec1, 0, sizeof rec1); memset(&rec2, 0, sizeof rec2);
    if (!hit_dispatch(c, m->obj_type, m->obj_idx, r, -INFINITY, INFINITY, &rec1)) return false;
    if (!hit_dispatch(c, m->obj_type, m->obj_idx, r, (float)(rec1.t + 0.0001), INFINITY, &rec2)) return false;
    if (rec1.t < t_min) rec1.t = t_min;
    if (rec2.t > t_max) rec2.t = t_max;
    if (rec1.t >= rec2.t) return false;
    if (rec1.t < 0) rec1.t = 0;
    float ray_length = vlen(r->dir);
    float distance_inside_boundary = (rec2.t - rec1.t) * ray_length;
    double hit_distance = m->neg_inv_density * mort_logf(random_float(c->g));
    if (hit_distance > distance_inside_boundary) return false;
    rec->t = (float)(rec1.t + hit_distance / ray_length);
    rec->p = ray_at(r, rec->t);
    rec->normal = V(1, 0, 0);
    rec->front_face = true;
    rec->mat_type = m->mat_type;
    rec->mat_idx = m->mat_idx;
    /* u, v are left as they were in the caller's record (indeterminate in the
     * reference); defined as 0 here and in the kernels. */
    rec->u = 0; rec->v = 0;
    return true;
}
static bool list_hit(ctx_t *c, const mort_hittable_list *l, const ray *r, float t_min, float t_max, hit_record *rec) {
    hit_record temp; /* objects.cuh:471-486 */
    memset(&temp, 0, sizeof temp);
    bool hit_anything = false;
    float closest = t_max;
    for (int i = 0; i < l->num_objs; i++) {
        if (hit_dispatch(c, l->obj_types[i], l->obj_idxs[i], r, t_min, closest, &temp)) {
            hit_anything = true;
            closest = temp.t;
            *rec = temp;
        }
    }
    return hit_anything;
}
static bool bvh_hit(ctx_t *c, const mort_bvh *b, const ray *r, float t_min, float t_max, hit_record *rec) {
    /* objects.cuh:664-723: explicit frames {node, child_evaluated, left_result, t_max} */
    struct frame { int node, child_evaluated; bool left_result; float t_max; } stack[64], cur;
    bool retval = false;
    int sp = 0;
    stack[0] = (struct frame){0, 0, true, t_max};
    while (sp >= 0) {
        cur = stack[sp];
        if (cur.child_evaluated == 0) {
            if (!aabb_hit(&b->bounding_boxes[cur.node], r, t_min, cur.t_max)) { retval = false; sp--; continue; }
            if (!b->is_internal_node[cur.node]) {
                bool hl = hit_dispatch(c, b->left_children_types[cur.node], b->left_children_idxs[cur.node], r, t_min, cur.t_max, rec);
                bool hr = hit_dispatch(c, b->right_children_types[cur.node], b->right_children_idxs[cur.node], r, t_min, hl ? rec->t : cur.t_max, rec);
                retval = hl || hr;
                sp--;
                continue;
            }
            stack[sp].child_evaluated += 1;
            sp++;
            stack[sp] = (struct frame){b->left_children_idxs[cur.node], 0, true, cur.t_max};
            continue;
        } else if (cur.child_evaluated == 1) {
            stack[sp].left_result = retval;
            stack[sp].child_evaluated += 1;
            sp++;
            stack[sp] = (struct frame){b->right_children_idxs[cur.node], 0, true, retval ? rec->t : cur.t_max};
            continue;
        } else {
            retval = cur.left_result || retval;
            sp--;
            continue;
        }
    }
    return retval;
}

static bool hit_dispatch(ctx_t *c, int type, int idx, const ray *r, float t_min, float t_max, hit_record *rec) {
    const mort_world_objects *o = &c->w->objs; /* objects.cuh:858-887 (no OBJ_BVH case) */
    switch (type) {
    case MORT_OBJ_SPHERE: return sphere_hit(&o->host_sphere[idx], r, t_min, t_max, rec);
    case MORT_OBJ_QUAD: return quad_hit(&o->host_quad[idx], r, t_min, t_max, rec);
    case MORT_OBJ_TRANSLATE: return translate_hit(c, &o->host_translate[idx], r, t_min, t_max, rec);
    case MORT_OBJ_ROTATE_Y: return rotate_y_hit(c, &o->host_rotate_y[idx], r, t_min, t_max, rec);
    case MORT_OBJ_CONSTANT_MEDIUM: return constant_medium_hit(c, &o->host_constant_medium[idx], r, t_min, t_max, rec);
    case MORT_OBJ_HITTABLE_LIST: return list_hit(c, &o->host_hittable_list[idx], r, t_min, t_max, rec);
    }
    return false;
}

static bool world_hit(ctx_t *c, const ray *r, float t_min, float t_max, hit_record *rec) { /* world.cuh:104-171 */
    const mort_world_objects *o = &c->w->objs;
    hit_record temp;
    memset(&temp, 0, sizeof temp);
    bool hit_anything = false;
    float closest = t_max;
    c->segments++;
#ifdef MORT_ORACLE_SEGMENT_HOOK /* scripts/ experiments that #include this file: observe each segment's ray */
    MORT_ORACLE_SEGMENT_HOOK(c->w, r, t_min);
#endif
#define WORLD_LOOP(N, ARR, CALL)                                              \
    for (int i = 0; i < (N); i++) {                                           \
        if (!o->ARR[i].skip && (CALL)) { hit_anything = true; closest = temp.t; *rec = temp; } \
    }
    WORLD_LOOP(o->num_bvh, host_bvh, bvh_hit(c, &o->host_bvh[i], r, t_min, closest, &temp))
    if (c->w->bvh_mode) return hit_anything;
    WORLD_LOOP(o->num_spheres, host_sphere, sphere_hit(&o->host_sphere[i], r, t_min, closest, &temp))
    WORLD_LOOP(o->num_quads, host_quad, quad_hit(&o->host_quad[i], r, t_min, closest, &temp))
    WORLD_LOOP(o->num_translates, host_translate, translate_hit(c, &o->host_translate[i], r, t_min, closest, &temp))
    WORLD_LOOP(o->num_rotate_y, host_rotate_y, rotate_y_hit(c, &o->host_rotate_y[i], r, t_min, closest, &temp))
    WORLD_LOOP(o->num_constant_medium, host_constant_medium, constant_medium_hit(c, &o->host_constant_medium[i], r, t_min, closest, &temp))
    WORLD_LOOP(o->num_hittable_list, host_hittable_list, list_hit(c, &o->host_hittable_list[i], r, t_min, closest, &temp))
#undef WORLD_LOOP
    return hit_anything;
}

/* ---- light sampling on objects (objects.cuh:110-145,217-235,488-504,947-979) ---- */

static float pdf_value_dispatch(ctx_t *c, int type, int idx, vec3 origin, vec3 direction);
static vec3 random_dispatch(ctx_t *c, int type, int idx, vec3 origin);

static float sphere_pdf_value(const mort_sphere *s, vec3 origin, vec3 direction) {
    hit_record rec;
    ray r = {origin, direction, 0};
    if (!sphere_hit(s, &r, 0.001f, HUGE_VALF, &rec)) return 0.0f; /* `return false` */
    float cos_theta_max = mort_sqrtf(1 - s->radius * s->radius / vlen2(vsub(s->center1, origin)));
    float solid_angle = (float)(2 * 3.1415926 * (1 - cos_theta_max));
    return (float)(1.0 / solid_angle);
}
static vec3 random_to_sphere(float radius, float distance_squared, rng_t *g) {
    float r1 = random_float(g);
    float r2 = random_float(g);
    float z = 1 + r2 * (mort_sqrtf(1 - radius * radius / distance_squared) - 1);
    float phi = (float)(2 * 3.141592 * r1);
    float x = mort_cosf(phi) * mort_sqrtf(1 - z * z);
    float y = mort_sinf(phi) * mort_sqrtf(1 - z * z);
    return V(x, y, z);
}
static vec3 sphere_random(const mort_sphere *s, vec3 origin, rng_t *g) {
    vec3 direction = vsub(s->center1, origin);
    float distance_squared = vlen2(direction);
    onb uvw;
    onb_build_from_w(&uvw, direction);
    return onb_local(&uvw, random_to_sphere(s->radius, distance_squared, g));
}
static float quad_pdf_value(const mort_quad *q, vec3 origin, vec3 direction) {
    hit_record rec;
    ray r = {origin, direction, 0};
    if (!quad_hit(q, &r, 0.001f, HUGE_VALF, &rec)) return 0;
    float distance_squared = rec.t * rec.t * vlen2(direction);
    float cosine = mort_fabsf(vdot(direction, rec.normal) / vlen(direction));
    return distance_squared / (cosine * q->area);
}
static vec3 quad_random(const mort_quad *q, vec3 origin, rng_t *g) {
    float a = random_float(g);
    float b = random_float(g);
    vec3 p = vadd(vadd(q->Q, vscale(a, q->u)), vscale(b, q->v));
    return vsub(p, origin);
}
static float list_pdf_value(ctx_t *c, const mort_hittable_list *l, vec3 origin, vec3 direction) {
    float weight = (float)(1.0 / (float)(l->num_objs));
    float sum = 0.0f;
    for (int i = 0; i < l->num_objs; i++)
        sum += weight * pdf_value_dispatch(c, l->obj_types[i], l->obj_idxs[i], origin, direction);
    return sum;
}
static vec3 list_random(ctx_t *c, const mort_hittable_list *l, vec3 origin) {
    int k = random_int(c->g, 0, l->num_objs - 1);
    return random_dispatch(c, l->obj_types[k], l->obj_idxs[k], origin);
}
static float pdf_value_dispatch(ctx_t *c, int type, int idx, vec3 origin, vec3 direction) {
    const mort_world_objects *o = &c->w->objs;
    switch (type) {
    case MORT_OBJ_SPHERE: return sphere_pdf_value(&o->host_sphere[idx], origin, direction);
    case MORT_OBJ_QUAD: return quad_pdf_value(&o->host_quad[idx], origin, direction);
    case MORT_OBJ_HITTABLE_LIST: return list_pdf_value(c, &o->host_hittable_list[idx], origin, direction);
    }
    return 0.0f;
}
static vec3 random_dispatch(ctx_t *c, int type, int idx, vec3 origin) {
    const mort_world_objects *o = &c->w->objs;
    switch (type) {
    case MORT_OBJ_SPHERE: return sphere_random(&o->host_sphere[idx], origin, c->g);
    case MORT_OBJ_QUAD: return quad_random(&o->host_quad[idx], origin, c->g);
    case MORT_OBJ_HITTABLE_LIST: return list_random(c, &o->host_hittable_list[idx], origin);
    }
    return V(1, 0, 0);
}

/* ------------------------------------------------------------------ textures (textures.cuh) */

static vec3 value_dispatch(const mort_world *w, int type, int idx, float u, float v, vec3 p);

static vec3 checker_value(const mort_world *w, const mort_checker_texture *t, float u, float v, vec3 p) { /* :52-60 */
    int xi = mort_f2i(mort_floorf(t->inv_scale * p.e[0]));
    int yi = mort_f2i(mort_floorf(t->inv_scale * p.e[1]));
    int zi = mort_f2i(mort_floorf(t->inv_scale * p.e[2]));
    bool is_even = (xi + yi + zi) % 2 == 0;
    return is_even ? value_dispatch(w, t->evenTextureType, t->evenTextureIdx, u, v, p)
                   : value_dispatch(w, t->oddTextureType, t->oddTextureIdx, u, v, p);
}
static float clamp01(float x) { if (x < 0) return 0; if (x > 1) return 1; return x; } /* interval.cuh:34-38 */
static vec3 image_value(const mort_image_texture *t, float u, float v) { /* textures.cuh:129-146 */
    if (t->height <= 0) return V(0, 1, 1);
    u = clamp01(u);
    v = (float)(1.0 - clamp01(v));
    int i = mort_f2i(u * t->width);
    int j = mort_f2i(v * t->height);
    /* tex2D<uchar> on an unnormalised pitch-2D resource: point sampling with
     * clamp-to-edge over the byte grid (row pitch = 3*width, rounded up to the
     * texture pitch alignment, which 3*1024 already satisfies) */
    int row_bytes = t->width * 3;
    if (j < 0) j = 0;
    if (j > t->height - 1) j = t->height - 1;
    int rgb[3];
    for (int k = 0; k < 3; k++) {
        int x = i * 3 + k;
        if (x < 0) x = 0;
        if (x > row_bytes - 1) x = row_bytes - 1;
        rgb[k] = t->texels[(size_t)j * row_bytes + x];
    }
    float color_scale = (float)(1.0 / 255.0);
    return V(color_scale * rgb[0], color_scale * rgb[1], color_scale * rgb[2]);
}
static float perlin_interp(vec3 c[2][2][2], double u, double v, double w) { /* textures.cuh:232-250 */
    double uu = u * u * (3 - 2 * u);
    double vv = v * v * (3 - 2 * v);
    double ww = w * w * (3 - 2 * w);
    double accum = 0.0;
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++)
            for (int k = 0; k < 2; k++) {
                vec3 weight_v = V((float)(u - i), (float)(v - j), (float)(w - k));
                accum += (i * uu + (1 - i) * (1 - uu)) * (j * vv + (1 - j) * (1 - vv)) *
                         (k * ww + (1 - k) * (1 - ww)) * vdot(c[i][j][k], weight_v);
            }
    return (float)accum;
}
static float noise_noise(const mort_noise_texture *t, vec3 p) { /* textures.cuh:174-196 */
    float u = p.e[0] - mort_floorf(p.e[0]);
    float v = p.e[1] - mort_floorf(p.e[1]);
    float w = p.e[2] - mort_floorf(p.e[2]);
    u = u * u * (3 - 2 * u);
    v = v * v * (3 - 2 * v);
    w = w * w * (3 - 2 * w);
    int i = mort_f2i(mort_floorf(p.e[0]));
    int j = mort_f2i(mort_floorf(p.e[1]));
    int k = mort_f2i(mort_floorf(p.e[2]));
    vec3 c[2][2][2];
    for (int di = 0; di < 2; di++)
        for (int dj = 0; dj < 2; dj++)
            for (int dk = 0; dk < 2; dk++) {
                int idx = t->perm_x[(i + di) & 255] ^ t->perm_y[(j + dj) & 255] ^ t->perm_z[(k + dk) & 255];
                c[di][dj][dk] = t->ranvec[idx];
            }
    return perlin_interp(c, u, v, w);
}
static float noise_turb(const mort_noise_texture *t, vec3 p) { /* textures.cuh:252-265, depth 7 */
    double accum = 0.0;
    vec3 temp_p = p;
    double weight = 1.0;
    for (int i = 0; i < 7; i++) {
        accum += weight * noise_noise(t, temp_p);
        weight *= 0.5;
        temp_p = vscale(2, temp_p);
    }
    return mort_fabsf((float)accum);
}
static vec3 noise_value(const mort_noise_texture *t, vec3 p) { /* textures.cuh:198-202 */
    vec3 s = vscale(t->scale, p);
    vec3 half = vscale(0.5f, V(1, 1, 1));
    return vscale((float)(1 + mort_sin(s.e[2] + 10.0 * noise_turb(t, s))), half);
}
static vec3 value_dispatch(const mort_world *w, int type, int idx, float u, float v, vec3 p) { /* textures.cuh:327-349 */
    switch (type) {
    case MORT_TEXTURE_SOLID: return w->texs.host_solid_color[idx].color_value;
    case MORT_TEXTURE_CHECKER: return checker_value(w, &w->texs.host_checker_texture[idx], u, v, p);
    case MORT_TEXTURE_IMAGE: return image_value(&w->texs.host_image_texture[idx], u, v);
    case MORT_TEXTURE_NOISE: return noise_value(&w->texs.host_noise_texture[idx], p);
    }
    float error = (float)((mort_f2i(mort_floorf((float)(u * 1000.0))) % 2) == (mort_f2i(mort_floorf((float)(v * 1000.0))) % 2));
    return V(error, 0.0f, error);
}

/* ------------------------------------------------------------------ materials + pdfs (materials.cuh, pdf.cuh) */

enum { PDF_NONE = 0, PDF_COSINE = 1, PDF_SPHERE = 2 };
typedef struct { vec3 attenuation; int pdf_kind; onb uvw; bool skip_pdf; ray skip_pdf_ray; bool cant_refract, reflected; /* census only */ } scatter_record;

static bool scatter_dispatch(ctx_t *c, const ray *r_in, const hit_record *rec, scatter_record *srec) {
    const mort_world *w = c->w; /* materials.cuh:272-296 */
    switch (rec->mat_type) {
    case MORT_MAT_LAMBERTIAN: { /* :38-44 */
        const mort_lambertian *m = &w->mats.host_lambertian[rec->mat_idx];
        srec->attenuation = value_dispatch(w, m->texType, m->texIdx, rec->u, rec->v, rec->p);
        srec->pdf_kind = PDF_COSINE;
        onb_build_from_w(&srec->uvw, rec->normal);
        srec->skip_pdf = false;
        return true;
    }
    case MORT_MAT_METAL: { /* :73-84 */
        const mort_metal *m = &w->mats.host_metal[rec->mat_idx];
        vec3 reflected = reflect(r_in->dir, rec->normal);
        reflected = vadd(vunit(reflected), vscale(m->fuzz, random_unit_vector(c->g)));
        srec->attenuation = m->albedo;
        srec->pdf_kind = PDF_NONE;
        srec->skip_pdf = true;
        srec->skip_pdf_ray = (ray){rec->p, reflected, r_in->t};
        return true;
    }
    case MORT_MAT_DIELECTRIC: { /* :107-130 */
        const mort_dielectric *m = &w->mats.host_dielectric[rec->mat_idx];
        srec->attenuation = V(1.0f, 1.0f, 1.0f);
        srec->pdf_kind = PDF_NONE;
        srec->skip_pdf = true;
        float refraction_ratio = rec->front_face ? m->inv_ior : m->ior;
        vec3 unit_direction = vunit(r_in->dir);
        float cos_theta = (float)mort_fmin((double)vdot(vneg(unit_direction), rec->normal), 1.0);
        float sin_theta = (float)mort_sqrt(1.0 - cos_theta * cos_theta);
        bool cant_refract = (refraction_ratio * sin_theta) > 1.0;
        vec3 direction;
        srec->cant_refract = cant_refract;
        if (cant_refract || reflectance(cos_theta, refraction_ratio) > random_float(c->g)) {
            direction = reflect(unit_direction, rec->normal);
            srec->reflected = true;
        } else {
            direction = refract(unit_direction, rec->normal, refraction_ratio);
            srec->reflected = false;
        }
        srec->skip_pdf_ray = (ray){rec->p, direction, r_in->t};
        return true;
    }
    case MORT_MAT_DIFFUSE_LIGHT: return false;
    case MORT_MAT_ISOTROPIC: { /* :182-188 */
        const mort_isotropic *m = &w->mats.host_isotropic[rec->mat_idx];
        srec->attenuation = value_dispatch(w, m->texType, m->texIdx, rec->u, rec->v, rec->p);
        srec->pdf_kind = PDF_SPHERE;
        srec->skip_pdf = false;
        return true;
    }
    }
    return false;
}
static vec3 emit_dispatch(const mort_world *w, const hit_record *rec) { /* materials.cuh:298-322 */
    if (rec->mat_type == MORT_MAT_DIFFUSE_LIGHT) { /* :156-163 */
        const mort_diffuse_light *m = &w->mats.host_diffuse_light[rec->mat_idx];
        if (!rec->front_face) return V(0, 0, 0);
        return value_dispatch(w, m->texType, m->texIdx, rec->u, rec->v, rec->p);
    }
    return V(0.0f, 0.0f, 0.0f);
}
static float scatter_pdf_dispatch(const hit_record *rec, const ray *scattered) { /* materials.cuh:324-349 */
    switch (rec->mat_type) {
    case MORT_MAT_LAMBERTIAN: { /* :51-55 */
        float cos_theta = vdot(rec->normal, vunit(scattered->dir));
        return (float)((cos_theta < 0) ? 0 : cos_theta / 3.141592565);
    }
    case MORT_MAT_ISOTROPIC: return (float)(1 / (4 * 3.1415926));
    }
    return 0;
}
static float srec_pdf_value(const scatter_record *s, vec3 direction) {
    if (s->pdf_kind == PDF_COSINE) { /* pdf.cuh:45-49 */
        float cosine_theta = vdot(vunit(direction), s->uvw.axis[2]);
        return mort_fmaxf(0, (float)(cosine_theta / 3.1415926));
    }
    return (float)(1 / (4 * 3.1415926)); /* sphere_pdf, pdf.cuh:29-32 */
}
static vec3 srec_pdf_generate(const scatter_record *s, rng_t *g) {
    if (s->pdf_kind == PDF_COSINE) return onb_local(&s->uvw, random_cosine_direction(g)); /* pdf.cuh:51-54 */
    return random_unit_vector(g);                                                          /* pdf.cuh:34-37 */
}

/* ------------------------------------------------------------------ camera (camera.cuh) */

/* one iteration of ray_color's loop body (camera.cuh:96-159): the closest hit of *current_ray and what its material does.  ray_color
 * and mort_oracle_shade_batch both call it, so the batch cannot drift from the loop the goldens and the reference pin hold in place.
 * time0 is r.time() of the ray ray_color was called with (camera.cuh:119).  STEP_SCATTER: *current_ray is the scattered ray and
 * att / emi / spdf / pdf are what the loop pushes.  STEP_END: emi is the emission the path ends with.  `branch`: see SHADE_BR_*. */
enum { STEP_MISS = 0, STEP_END = 1, STEP_SCATTER = 2 };
enum { SHADE_BR_TAG = 0 /* 8 bits: mat_type + 2, 0xff = outside -1 .. 252 */, SHADE_BR_TEX = 8 /* 8 bits: the material's texType + 2 likewise, 0 = no texture */,
       SHADE_BR_FRONT = 1 << 16, SHADE_BR_CANT_REFRACT = 1 << 17, SHADE_BR_REFLECTED = 1 << 18, SHADE_BR_REFRACTED = 1 << 19,
       SHADE_BR_FROM_LIGHT = 1 << 20, SHADE_BR_FROM_MATERIAL = 1 << 21, SHADE_BR_MAT_PDF_ZERO = 1 << 22, SHADE_BR_NORMAL_NONFINITE = 1 << 23,
       SHADE_BR_RATIO_ONE = 1 << 24, SHADE_BR_SKIP_PDF = 1 << 25 };
typedef struct { vec3 att, emi; float spdf, pdf; unsigned branch; } step_out;

static unsigned branch_tag(int tag) { return (tag >= -1 && tag <= 252) ? (unsigned)(tag + 2) : 0xffu; }

static int bounce_step(ctx_t *c, int light_obj_type, int light_obj_idx, float time0, ray *current_ray, hit_record *rec, step_out *o) {
    o->att = V(0, 0, 0); o->emi = V(0, 0, 0); o->spdf = 0; o->pdf = 0; o->branch = 0;
    if (!world_hit(c, current_ray, 0.001f, INFINITY, rec)) return STEP_MISS;
    {
        const mort_world_materials *m = &c->w->mats;
        int tex = -2; /* the material's own texture tag, for the census */
        if (rec->mat_type == MORT_MAT_LAMBERTIAN) tex = m->host_lambertian[rec->mat_idx].texType;
        else if (rec->mat_type == MORT_MAT_DIFFUSE_LIGHT) tex = m->host_diffuse_light[rec->mat_idx].texType;
        else if (rec->mat_type == MORT_MAT_ISOTROPIC) tex = m->host_isotropic[rec->mat_idx].texType;
        o->branch = branch_tag(rec->mat_type) << SHADE_BR_TAG | (tex == -2 ? 0u : branch_tag(tex) << SHADE_BR_TEX) | (rec->front_face ? SHADE_BR_FRONT : 0);
        if (!isfinite(rec->normal.e[0]) || !isfinite(rec->normal.e[1]) || !isfinite(rec->normal.e[2])) o->branch |= SHADE_BR_NORMAL_NONFINITE;
        if (rec->mat_type == MORT_MAT_DIELECTRIC) { /* the decisions scatter_dispatch is about to take, restated for the census only */
            const mort_dielectric *d = &m->host_dielectric[rec->mat_idx];
            const float ratio = rec->front_face ? d->inv_ior : d->ior;
            if (ratio == 1.0f) o->branch |= SHADE_BR_RATIO_ONE;
        }
    }
    ray scattered;
    vec3 emission = emit_dispatch(c->w, rec);
    float pdf, scattering_pdf;
    scatter_record srec;
    srec.cant_refract = false; srec.reflected = false;
    if (!scatter_dispatch(c, current_ray, rec, &srec)) {
        o->emi = emission;
        return STEP_END;
    }
    if (srec.skip_pdf) {
        *current_ray = srec.skip_pdf_ray;
        o->att = srec.attenuation; o->emi = V(0, 0, 0); o->spdf = 1.0f; o->pdf = 1.0f;
        o->branch |= SHADE_BR_SKIP_PDF;
        if (rec->mat_type == MORT_MAT_DIELECTRIC)
            o->branch |= (srec.cant_refract ? SHADE_BR_CANT_REFRACT : 0) | (srec.reflected ? SHADE_BR_REFLECTED : SHADE_BR_REFRACTED);
        return STEP_SCATTER;
    }
    if (light_obj_type == -1) {
        scattered = (ray){rec->p, srec_pdf_generate(&srec, c->g), time0};
        pdf = srec_pdf_value(&srec, scattered.dir);
        scattering_pdf = scatter_pdf_dispatch(rec, &scattered);
    } else {
        /* mixture_pdf(hittable_pdf(light), srec.pdf), pdf.cuh:60-107 */
        vec3 dir;
        if (random_float(c->g) < 0.5) {
            dir = random_dispatch(c, light_obj_type, light_obj_idx, rec->p);
            o->branch |= SHADE_BR_FROM_LIGHT;
        } else {
            dir = srec_pdf_generate(&srec, c->g);
            o->branch |= SHADE_BR_FROM_MATERIAL;
        }
        scattered = (ray){rec->p, dir, time0};
        pdf = (float)(0.5 * pdf_value_dispatch(c, light_obj_type, light_obj_idx, rec->p, scattered.dir) +
                      0.5 * srec_pdf_value(&srec, scattered.dir));
        scattering_pdf = scatter_pdf_dispatch(rec, &scattered);
    }
    if (srec_pdf_value(&srec, scattered.dir) == 0.0f) o->branch |= SHADE_BR_MAT_PDF_ZERO; /* census only: pure, draws nothing */
    *current_ray = scattered;
    o->att = srec.attenuation; o->emi = emission; o->spdf = scattering_pdf; o->pdf = pdf;
    return STEP_SCATTER;
}

static vec3 ray_color(ctx_t *c, const mort_camera *cam, const ray *r) { /* camera.cuh:86-176 */
    hit_record rec;
    memset(&rec, 0, sizeof rec);
    int iter = 0;
    ray current_ray = *r;
    vec3 st_att[MORT_MAX_BOUNCE_LIMIT], st_emi[MORT_MAX_BOUNCE_LIMIT];
    float st_spdf[MORT_MAX_BOUNCE_LIMIT], st_pdf[MORT_MAX_BOUNCE_LIMIT];
    vec3 final_value = V(0, 0, 0);

    while (iter < cam->bounce_limit) {
        step_out so;
        const int what = bounce_step(c, cam->light_obj_type, cam->light_obj_idx, r->t, &current_ray, &rec, &so);
        if (what == STEP_SCATTER) {
            st_att[iter] = so.att;
            st_emi[iter] = so.emi;
            st_spdf[iter] = so.spdf;
            st_pdf[iter] = so.pdf;
            iter++;
        } else if (what == STEP_END) {
            final_value = so.emi;
            break;
        } else {
            final_value = cam->background;
            break;
        }
    }
    if (iter == cam->bounce_limit) final_value = V(0, 0, 0);
    while (iter > 0) { /* camera.cuh:165-173 */
        iter--;
        final_value = vadd(st_emi[iter], vdiv(vmul(vscale(st_spdf[iter], st_att[iter]), final_value), st_pdf[iter]));
    }
    return final_value;
}

static ray get_ray(const mort_camera *cam, double u, double v, rng_t *g, int s_i, int s_j) { /* camera.cuh:210-242 */
    double px = ((s_i + random_float(g)) * cam->recip_sqrt_spp) - 0.5;
    double py = ((s_j + random_float(g)) * cam->recip_sqrt_spp) - 0.5;
    vec3 offset = V((float)px, (float)py, 0);
    vec3 pixel_sample = vadd(vadd(cam->pixel00_loc, vscale((float)(u + offset.e[0]), cam->pixel_delta_u)),
                             vscale((float)(v + offset.e[1]), cam->pixel_delta_v));
    vec3 ray_origin;
    if (cam->defocus_angle <= 0) {
        ray_origin = cam->center;
    } else {
        vec3 p = random_in_unit_disk(g);
        ray_origin = vadd(vadd(cam->center, vscale(p.e[0], cam->defocus_disk_u)), vscale(p.e[1], cam->defocus_disk_v));
    }
    vec3 ray_direction = vsub(pixel_sample, ray_origin);
    float ray_time = random_float(g);
    return (ray){ray_origin, ray_direction, ray_time};
}

static float clampf(float x, float mn, float mx) { if (x < mn) return mn; if (x > mx) return mx; return x; } /* utils.h:35-39 */

/* the end of Camera::render (camera.cuh:194-207) on a pixel's sum: the mean with each NaN component 0 (returned: the accumulator), and
 * its gamma-2, clamped, truncated bytes with alpha 255 into rgba4 */
static vec3 pixel_tail(float pixel_samples_scale, vec3 pixel_color, uint8_t *rgba4) {
    pixel_color = vscale(pixel_samples_scale, pixel_color);
    for (int k = 0; k < 3; k++)
        if (pixel_color.e[k] != pixel_color.e[k]) pixel_color.e[k] = 0.0f;
    for (int k = 0; k < 3; k++) {
        float gch = mort_sqrtf(pixel_color.e[k]);
        rgba4[k] = (uint8_t)mort_f2i(256 * clampf(gch, 0.0f, 0.999f));
    }
    rgba4[3] = 255;
    return pixel_color;
}

static void render_pixel(const mort_world *w, const mort_camera *cam, mort_rng_state *states, int x, int y,
                         uint8_t *rgba, float *accum, uint32_t *seg_px, uint64_t *segs, uint64_t *draws) {
    int offset = x + y * cam->image_width; /* camera.cuh:178-208 */
    rng_t g = {&states[offset], 0};
    ctx_t c = {w, &g, 0};
    vec3 pixel_color = V(0, 0, 0);
    for (int s_j = 0; s_j < cam->sqrt_spp; s_j++)
        for (int s_i = 0; s_i < cam->sqrt_spp; s_i++) {
            ray r = get_ray(cam, x, y, &g, s_i, s_j);
            pixel_color = vadd(pixel_color, ray_color(&c, cam, &r));
        }
    pixel_color = pixel_tail(cam->pixel_samples_scale, pixel_color, rgba + 4 * (size_t)offset);
    if (accum) { accum[3 * offset] = pixel_color.e[0]; accum[3 * offset + 1] = pixel_color.e[1]; accum[3 * offset + 2] = pixel_color.e[2]; }
    if (seg_px) seg_px[offset] = (uint32_t)c.segments;
    *segs += c.segments;
    *draws += g.draws;
}

typedef struct {
    const mort_world *w; const mort_camera *cam; mort_rng_state *states;
    int row0, row1, tid, nthreads;
    uint8_t *rgba; float *accum; uint32_t *seg_px; uint64_t segs, draws;
} job_t;

static void *render_job(void *arg) {
    job_t *j = arg;
    /* rows interleaved over threads: neighbouring rows cost about the same */
    for (int y = j->row0 + j->tid; y < j->row1; y += j->nthreads)
        for (int x = 0; x < j->cam->image_width; x++)
            render_pixel(j->w, j->cam, j->states, x, y, j->rgba, j->accum, j->seg_px, &j->segs, &j->draws);
    return NULL;
}

int mort_oracle_render(const mort_world *w, const mort_camera *cam, mort_rng_state *states, int row0, int row1,
                       uint8_t *rgba, float *accum, uint32_t *segments_per_pixel, int nthreads,
                       mort_oracle_stats *stats) {
    if (!w || !cam || !states || !rgba) return -1;
    if (cam->bounce_limit > MORT_MAX_BOUNCE_LIMIT || cam->bounce_limit < 0) return -2;
    if (row0 < 0) row0 = 0;
    if (row1 > cam->image_height) row1 = cam->image_height;
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 256) nthreads = 256;
    job_t jobs[256];
    pthread_t th[256];
    for (int t = 0; t < nthreads; t++) {
        jobs[t] = (job_t){w, cam, states, row0, row1, t, nthreads, rgba, accum, segments_per_pixel, 0, 0};
        if (t > 0) pthread_create(&th[t], NULL, render_job, &jobs[t]);
    }
    render_job(&jobs[0]);
    uint64_t segs = jobs[0].segs, draws = jobs[0].draws;
    for (int t = 1; t < nthreads; t++) { pthread_join(th[t], NULL); segs += jobs[t].segs; draws += jobs[t].draws; }
    if (stats) { stats->segments = segs; stats->rng_draws = draws; }
    return 0;
}

/* ------------------------------------------------------------------ known-answer entry points */

bool mort_oracle_world_hit(const mort_world *w, const float ray7[7], float t_min, float t_max,
                           mort_rng_state *state, mort_oracle_hit *out) {
    rng_t g = {state, 0};
    ctx_t c = {w, &g, 0};
    ray r = {V(ray7[0], ray7[1], ray7[2]), V(ray7[3], ray7[4], ray7[5]), ray7[6]};
    memset(out, 0, sizeof *out);
    return world_hit(&c, &r, t_min, t_max, out);
}

bool mort_oracle_aabb_hit(const mort_aabb *b, const float ray7[7], float t_min, float t_max) {
    ray r = {V(ray7[0], ray7[1], ray7[2]), V(ray7[3], ray7[4], ray7[5]), ray7[6]};
    return aabb_hit(b, &r, t_min, t_max);
}

void mort_oracle_get_ray(const mort_camera *cam, int x, int y, int s_i, int s_j, mort_rng_state *state, float ray7[7]) {
    rng_t g = {state, 0};
    ray r = get_ray(cam, x, y, &g, s_i, s_j);
    memcpy(ray7, &r, 7 * sizeof(float));
}

void mort_oracle_ray_color(const mort_world *w, const mort_camera *cam, const float ray7[7], mort_rng_state *state, float rgb[3]) {
    rng_t g = {state, 0};
    ctx_t c = {w, &g, 0};
    ray r = {V(ray7[0], ray7[1], ray7[2]), V(ray7[3], ray7[4], ray7[5]), ray7[6]};
    vec3 col = ray_color(&c, cam, &r);
    memcpy(rgb, col.e, sizeof col.e);
}

void mort_oracle_texture_value(const mort_world *w, int tex_type, int tex_idx, float u, float v, const float p[3], float rgb[3]) {
    vec3 col = value_dispatch(w, tex_type, tex_idx, u, v, V(p[0], p[1], p[2]));
    memcpy(rgb, col.e, sizeof col.e);
}

float mort_oracle_pdf_value(const mort_world *w, int type, int idx, const float origin[3], const float dir[3]) {
    ctx_t c = {w, NULL, 0};
    return pdf_value_dispatch(&c, type, idx, V(origin[0], origin[1], origin[2]), V(dir[0], dir[1], dir[2]));
}

void mort_oracle_light_random(const mort_world *w, int type, int idx, const float origin[3], mort_rng_state *state, float dir[3]) {
    rng_t g = {state, 0};
    ctx_t c = {w, &g, 0};
    vec3 d = random_dispatch(&c, type, idx, V(origin[0], origin[1], origin[2]));
    memcpy(dir, d.e, sizeof d.e);
}

/* ---- batched, threaded forms of the entry points above (tests/feature_ref.py): loops, no arithmetic of their own ---- */
enum { MORT_ORACLE_BATCH_OK = 0, MORT_ORACLE_BATCH_BAD_ARGS = -1, MORT_ORACLE_BATCH_NO_STREAM = -3 };

/* pdf_value_dispatch (fn 0) and random_dispatch (fn 1) over n records of 32-bit words, function numbers and record shapes as
 * mort_hip_debug_light_shape (mort_amd/csrc/hip/debug.hip): fn 0 type, idx, origin[3], direction[3] -> the pdf; fn 1 the six stream words
 * (d, v[0..4]), type, idx, origin[3] -> the direction, the six final words, the draw count.  A sphere, quad or list index outside the
 * world's tables is refused for the whole batch; what a list holds is the caller's business, as it is pdf_value_dispatch's */
typedef struct { const mort_world *w; int fn, tid, nthreads; size_t n; const uint32_t *in; uint32_t *out; } light_job_t;
static void *light_job(void *arg) {
    light_job_t *j = arg;
    const size_t iw = j->fn == 0 ? 8 : 11, ow = j->fn == 0 ? 1 : 10;
    for (size_t i = j->n * (size_t)j->tid / (size_t)j->nthreads, end = j->n * ((size_t)j->tid + 1) / (size_t)j->nthreads; i < end; i++) {
        const uint32_t *a = j->in + i * iw;
        uint32_t *o = j->out + i * ow;
        float f[6];
        if (j->fn == 0) {
            memcpy(f, a + 2, sizeof f);
            ctx_t c = {j->w, NULL, 0};
            float pdf = pdf_value_dispatch(&c, (int)a[0], (int)a[1], V(f[0], f[1], f[2]), V(f[3], f[4], f[5]));
            memcpy(o, &pdf, 4);
        } else {
            mort_rng_state st;
            memset(&st, 0, sizeof st);
            st.d = a[0];
            for (int k = 0; k < 5; k++) st.v[k] = a[1 + k];
            memcpy(f, a + 8, 3 * sizeof(float));
            rng_t g = {&st, 0};
            ctx_t c = {j->w, &g, 0};
            vec3 d = random_dispatch(&c, (int)a[6], (int)a[7], V(f[0], f[1], f[2]));
            memcpy(o, d.e, 3 * sizeof(float));
            o[3] = st.d;
            for (int k = 0; k < 5; k++) o[4 + k] = st.v[k];
            o[9] = (uint32_t)g.draws;
        }
    }
    return NULL;
}
int mort_oracle_light_batch(const mort_world *w, int fn, const uint32_t *in, size_t n, uint32_t *out, int nthreads) {
    if (!w || (fn != 0 && fn != 1) || ((!in || !out) && n)) return MORT_ORACLE_BATCH_BAD_ARGS;
    const mort_world_objects *o = &w->objs;
    const size_t iw = fn == 0 ? 8 : 11, at = fn == 0 ? 0 : 6;
    for (size_t i = 0; i < n; i++) {
        const int type = (int)in[i * iw + at], idx = (int)in[i * iw + at + 1];
        const int count = type == MORT_OBJ_SPHERE ? o->num_spheres : type == MORT_OBJ_QUAD ? o->num_quads :
                          type == MORT_OBJ_HITTABLE_LIST ? o->num_hittable_list : -1;
        if (count >= 0 && (idx < 0 || idx >= count)) return MORT_ORACLE_BATCH_BAD_ARGS;
    }
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 64) nthreads = 64;
    if (n < 4096) nthreads = 1;
    light_job_t jobs[64];
    pthread_t th[64];
    for (int t = 0; t < nthreads; t++) {
        jobs[t] = (light_job_t){w, fn, t, nthreads, n, in, out};
        if (t > 0) pthread_create(&th[t], NULL, light_job, &jobs[t]);
    }
    light_job(&jobs[0]);
    for (int t = 1; t < nthreads; t++) pthread_join(th[t], NULL);
    return MORT_ORACLE_BATCH_OK;
}

/* one iteration of ray_color's loop body (bounce_step) over n records of 32-bit words, the layout of mort_hip_debug_shade_shape
 * (mort_amd/csrc/hip/debug.hip): in (16) the six stream words (d, v[0..4]), ray origin[3], direction[3], time, the time of the ray
 * ray_color was called with, the camera's light object (type, idx); out (22) status (0 miss, 1 the path ends, 2 scatter, 3 a dielectric's
 * scatter), k[3] = scattering_pdf x attenuation, rp = the fp32 1 / pdf (1 for a skip-pdf scatter), final_value[3] (the emission a path
 * ends with), the ray afterwards (7), the six final words, the draw count.  branch (may be NULL): one SHADE_BR_* word per record, for a
 * census; no kernel produces it.  A light object whose sphere, quad or list index lies outside the world's tables is refused for the
 * whole batch. */
typedef struct { const mort_world *w; int tid, nthreads; size_t n; const uint32_t *in; uint32_t *out, *branch; } shade_job_t;
static void *shade_job(void *arg) {
    shade_job_t *j = arg;
    for (size_t i = j->n * (size_t)j->tid / (size_t)j->nthreads, end = j->n * ((size_t)j->tid + 1) / (size_t)j->nthreads; i < end; i++) {
        const uint32_t *a = j->in + i * 16;
        uint32_t *o = j->out + i * 22;
        float f[8];
        mort_rng_state st;
        memset(&st, 0, sizeof st);
        st.d = a[0];
        for (int k = 0; k < 5; k++) st.v[k] = a[1 + k];
        memcpy(f, a + 6, sizeof f);
        rng_t g = {&st, 0};
        ctx_t c = {j->w, &g, 0};
        ray r = {V(f[0], f[1], f[2]), V(f[3], f[4], f[5]), f[6]};
        hit_record rec;
        memset(&rec, 0, sizeof rec);
        step_out so;
        const int what = bounce_step(&c, (int)a[14], (int)a[15], f[7], &r, &rec, &so);
        vec3 kk = V(0, 0, 0), fin = V(0, 0, 0);
        float rp = 0;
        if (what == STEP_SCATTER) {
            kk = vscale(so.spdf, so.att);
            rp = (so.branch & SHADE_BR_SKIP_PDF) ? 1.0f : 1 / so.pdf;
        } else if (what == STEP_END) fin = so.emi;
        o[0] = what == STEP_SCATTER && rec.mat_type == MORT_MAT_DIELECTRIC ? 3u : (uint32_t)what;
        memcpy(o + 1, kk.e, 12); memcpy(o + 4, &rp, 4); memcpy(o + 5, fin.e, 12);
        memcpy(o + 8, r.orig.e, 12); memcpy(o + 11, r.dir.e, 12); memcpy(o + 14, &r.t, 4);
        o[15] = st.d;
        for (int k = 0; k < 5; k++) o[16 + k] = st.v[k];
        o[21] = (uint32_t)g.draws;
        if (j->branch) j->branch[i] = so.branch;
    }
    return NULL;
}
int mort_oracle_shade_batch(const mort_world *w, const uint32_t *in, size_t n, uint32_t *out, uint32_t *branch, int nthreads) {
    if (!w || ((!in || !out) && n)) return MORT_ORACLE_BATCH_BAD_ARGS;
    const mort_world_objects *ob = &w->objs;
    for (size_t i = 0; i < n; i++) {
        const int type = (int)in[i * 16 + 14], idx = (int)in[i * 16 + 15];
        const int count = type == MORT_OBJ_SPHERE ? ob->num_spheres : type == MORT_OBJ_QUAD ? ob->num_quads :
                          type == MORT_OBJ_HITTABLE_LIST ? ob->num_hittable_list : -1;
        if (count >= 0 && (idx < 0 || idx >= count)) return MORT_ORACLE_BATCH_BAD_ARGS;
    }
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 64) nthreads = 64;
    if (n < 4096) nthreads = 1;
    shade_job_t jobs[64];
    pthread_t th[64];
    for (int t = 0; t < nthreads; t++) {
        jobs[t] = (shade_job_t){w, t, nthreads, n, in, out, branch};
        if (t > 0) pthread_create(&th[t], NULL, shade_job, &jobs[t]);
    }
    shade_job(&jobs[0]);
    for (int t = 1; t < nthreads; t++) pthread_join(th[t], NULL);
    return MORT_ORACLE_BATCH_OK;
}

/* the two ends of Camera::render over n records of 32-bit words, function numbers and record shapes as mort_hip_debug_camera_shape
 * (mort_amd/csrc/hip/debug.hip).  fn 0 and fn 1 (one function here; the kernels have two instantiations), get_ray: in (30) the six stream
 * words (d, v[0..4]), x, y, s_i, s_j, recip_sqrt_spp, defocus_angle, center, pixel00_loc, pixel_delta_u, pixel_delta_v, defocus_disk_u,
 * defocus_disk_v; out (14) origin[3], direction[3], time, the six final words, the draw count.  fn 2, render_pixel's tail: in (4)
 * pixel_samples_scale, the pixel's sum[3]; out (4) the accumulator[3] and the four bytes of the pixel as one word (red lowest). */
typedef struct { int fn, tid, nthreads; size_t n; const uint32_t *in; uint32_t *out; } camera_job_t;
static void *camera_job(void *arg) {
    camera_job_t *j = arg;
    const size_t iw = j->fn == 2 ? 4 : 30, ow = j->fn == 2 ? 4 : 14;
    for (size_t i = j->n * (size_t)j->tid / (size_t)j->nthreads, end = j->n * ((size_t)j->tid + 1) / (size_t)j->nthreads; i < end; i++) {
        const uint32_t *a = j->in + i * iw;
        uint32_t *o = j->out + i * ow;
        if (j->fn == 2) {
            float f[4];
            uint8_t px[4];
            memcpy(f, a, sizeof f);
            vec3 acc = pixel_tail(f[0], V(f[1], f[2], f[3]), px);
            memcpy(o, acc.e, sizeof acc.e);
            o[3] = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16) | ((uint32_t)px[3] << 24);
        } else {
            mort_rng_state st;
            memset(&st, 0, sizeof st);
            st.d = a[0];
            for (int k = 0; k < 5; k++) st.v[k] = a[1 + k];
            mort_camera cam;
            memset(&cam, 0, sizeof cam);
            float f[20];
            memcpy(f, a + 10, sizeof f);
            cam.recip_sqrt_spp = f[0];
            cam.defocus_angle = f[1];
            cam.center = V(f[2], f[3], f[4]);
            cam.pixel00_loc = V(f[5], f[6], f[7]);
            cam.pixel_delta_u = V(f[8], f[9], f[10]);
            cam.pixel_delta_v = V(f[11], f[12], f[13]);
            cam.defocus_disk_u = V(f[14], f[15], f[16]);
            cam.defocus_disk_v = V(f[17], f[18], f[19]);
            rng_t g = {&st, 0};
            ray r = get_ray(&cam, (int)a[6], (int)a[7], &g, (int)a[8], (int)a[9]);
            memcpy(o, &r, 7 * sizeof(float));
            o[7] = st.d;
            for (int k = 0; k < 5; k++) o[8 + k] = st.v[k];
            o[13] = (uint32_t)g.draws;
        }
    }
    return NULL;
}
int mort_oracle_camera_batch(int fn, const uint32_t *in, size_t n, uint32_t *out, int nthreads) {
    if (fn < 0 || fn > 2 || ((!in || !out) && n)) return MORT_ORACLE_BATCH_BAD_ARGS;
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 64) nthreads = 64;
    if (n < 4096) nthreads = 1;
    camera_job_t jobs[64];
    pthread_t th[64];
    for (int t = 0; t < nthreads; t++) {
        jobs[t] = (camera_job_t){fn, t, nthreads, n, in, out};
        if (t > 0) pthread_create(&th[t], NULL, camera_job, &jobs[t]);
    }
    camera_job(&jobs[0]);
    for (int t = 1; t < nthreads; t++) pthread_join(th[t], NULL);
    return MORT_ORACLE_BATCH_OK;
}

/* would hit_dispatch on this object reach constant_medium_hit's random_float()? */
static bool object_draws(const mort_world *w, int type, int idx, int depth) {
    const mort_world_objects *o = &w->objs;
    if (depth > 16) return true; /* a cyclic reference: refuse rather than recurse */
    switch (type) {
    case MORT_OBJ_CONSTANT_MEDIUM: return true;
    case MORT_OBJ_TRANSLATE: return object_draws(w, o->host_translate[idx].obj_type, o->host_translate[idx].obj_idx, depth + 1);
    case MORT_OBJ_ROTATE_Y: return object_draws(w, o->host_rotate_y[idx].obj_type, o->host_rotate_y[idx].obj_idx, depth + 1);
    case MORT_OBJ_HITTABLE_LIST:
        for (int i = 0; i < o->host_hittable_list[idx].num_objs; i++)
            if (object_draws(w, o->host_hittable_list[idx].obj_types[i], o->host_hittable_list[idx].obj_idxs[i], depth + 1)) return true;
        return false;
    }
    return false;
}
/* the same for world_hit: the objects its loops do not pass over */
static bool world_draws(const mort_world *w) {
    const mort_world_objects *o = &w->objs;
    for (int b = 0; b < o->num_bvh; b++) {
        if (o->host_bvh[b].skip) continue;
        for (int n = 0; n < MORT_MAX_BVH_NODES; n++) {
            const mort_bvh *v = &o->host_bvh[b];
            if (v->is_internal_node[n]) continue;
            if (object_draws(w, v->left_children_types[n], v->left_children_idxs[n], 0)) return true;
            if (object_draws(w, v->right_children_types[n], v->right_children_idxs[n], 0)) return true;
        }
    }
    if (w->bvh_mode) return false;
    for (int i = 0; i < o->num_translates; i++) if (!o->host_translate[i].skip && object_draws(w, MORT_OBJ_TRANSLATE, i, 0)) return true;
    for (int i = 0; i < o->num_rotate_y; i++) if (!o->host_rotate_y[i].skip && object_draws(w, MORT_OBJ_ROTATE_Y, i, 0)) return true;
    for (int i = 0; i < o->num_constant_medium; i++) if (!o->host_constant_medium[i].skip) return true;
    for (int i = 0; i < o->num_hittable_list; i++) if (!o->host_hittable_list[i].skip && object_draws(w, MORT_OBJ_HITTABLE_LIST, i, 0)) return true;
    return false;
}

typedef struct {
    const mort_world *w; int type, idx; /* type 0: world_hit */
    int n, tid, nthreads;
    const float *ray7, *t_min, *t_max; mort_rng_state *states; mort_oracle_hit *out; uint8_t *hit;
} batch_job_t;

#define BATCH_BLOCK 256
static void *batch_job(void *arg) {
    batch_job_t *j = arg;
    for (int b = j->tid * BATCH_BLOCK; b < j->n; b += j->nthreads * BATCH_BLOCK)
        for (int i = b; i < j->n && i < b + BATCH_BLOCK; i++) {
            rng_t g = {j->states ? &j->states[i] : NULL, 0};
            ctx_t c = {j->w, &g, 0};
            const float *q = j->ray7 + 7 * (size_t)i;
            ray r = {V(q[0], q[1], q[2]), V(q[3], q[4], q[5]), q[6]};
            memset(&j->out[i], 0, sizeof j->out[i]);
            j->hit[i] = j->type ? hit_dispatch(&c, j->type, j->idx, &r, j->t_min[i], j->t_max[i], &j->out[i])
                                : world_hit(&c, &r, j->t_min[i], j->t_max[i], &j->out[i]);
        }
    return NULL;
}

static int batch_run(batch_job_t proto, int nthreads) {
    if (!proto.w || proto.n < 0 || !proto.ray7 || !proto.t_min || !proto.t_max || !proto.out || !proto.hit) return MORT_ORACLE_BATCH_BAD_ARGS;
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 256) nthreads = 256;
    batch_job_t jobs[256];
    pthread_t th[256];
    for (int t = 0; t < nthreads; t++) {
        jobs[t] = proto; jobs[t].tid = t; jobs[t].nthreads = nthreads;
        if (t > 0) pthread_create(&th[t], NULL, batch_job, &jobs[t]);
    }
    batch_job(&jobs[0]);
    for (int t = 1; t < nthreads; t++) pthread_join(th[t], NULL);
    return MORT_ORACLE_BATCH_OK;
}

int mort_oracle_world_hit_batch(const mort_world *w, int n, const float *ray7, const float *t_min, const float *t_max,
                                mort_rng_state *states, mort_oracle_hit *out, uint8_t *hit, int nthreads) {
    if (!w) return MORT_ORACLE_BATCH_BAD_ARGS;
    if (!states && world_draws(w)) return MORT_ORACLE_BATCH_NO_STREAM;
    return batch_run((batch_job_t){w, 0, 0, n, 0, 0, ray7, t_min, t_max, states, out, hit}, nthreads);
}

int mort_oracle_object_hit_batch(const mort_world *w, int type, int idx, int n, const float *ray7, const float *t_min, const float *t_max,
                                 mort_rng_state *states, mort_oracle_hit *out, uint8_t *hit, int nthreads) {
    if (!w || idx < 0) return MORT_ORACLE_BATCH_BAD_ARGS;
    const mort_world_objects *o = &w->objs;
    const int counts[] = {0, o->num_spheres, o->num_quads, o->num_translates, o->num_rotate_y, o->num_constant_medium, o->num_hittable_list};
    if (type < MORT_OBJ_SPHERE || type > MORT_OBJ_HITTABLE_LIST || idx >= counts[type]) return MORT_ORACLE_BATCH_BAD_ARGS;
    if (!states && object_draws(w, type, idx, 0)) return MORT_ORACLE_BATCH_NO_STREAM;
    return batch_run((batch_job_t){w, type, idx, n, 0, 0, ray7, t_min, t_max, states, out, hit}, nthreads);
}

int mort_oracle_texture_value_batch(const mort_world *w, int n, const int *tex_type, const int *tex_idx, const float *u, const float *v,
                                    const float *p, float *rgb) {
    if (!w || n < 0 || !tex_type || !tex_idx || !u || !v || !p || !rgb) return MORT_ORACLE_BATCH_BAD_ARGS;
    for (int i = 0; i < n; i++) mort_oracle_texture_value(w, tex_type[i], tex_idx[i], u[i], v[i], p + 3 * (size_t)i, rgb + 3 * (size_t)i);
    return MORT_ORACLE_BATCH_OK;
}

/* mort_math.h entry points so tests can measure them against glibc */
float mort_oracle_sinf(float x) { return mort_sinf(x); }
float mort_oracle_cosf(float x) { return mort_cosf(x); }
void mort_oracle_sincosf(float x, float *s, float *c) { mort_sincosf(x, s, c); } /* the kernels' shared evaluation */
float mort_oracle_acosf(float x) { return mort_acosf(x); }
float mort_oracle_atan2f(float y, float x) { return mort_atan2f(y, x); }
float mort_oracle_logf(float x) { return mort_logf(x); }
double mort_oracle_sin(double x) { return mort_sin(x); }

/* mort_math.h (0..15) and the plain operators the numerical contract leans on (16..21) over n records of 32-bit words (a double is two,
 * low word first), function numbers and record shapes as mort_hip_debug_math_shape's groups A and P (mort_amd/csrc/hip/debug.hip):
 * gcc's compile beside hipcc's two */
static float mb_f(const uint32_t *w) { float x; memcpy(&x, w, 4); return x; }
static double mb_d(const uint32_t *w) { double x; memcpy(&x, w, 8); return x; }
static void mb_pf(uint32_t *w, float x) { memcpy(w, &x, 4); }
static void mb_pd(uint32_t *w, double x) { memcpy(w, &x, 8); }
int mort_oracle_math_batch(int fn, const uint32_t *in, size_t n, uint32_t *out) {
    static const unsigned char shape[22][2] = {{1, 1}, {2, 2}, {1, 1}, {2, 1}, {4, 2}, {2, 1}, {1, 1}, {2, 2},
                                               {2, 2}, {1, 1}, {1, 1}, {1, 2}, {2, 2}, {2, 1}, {1, 1}, {1, 1},
                                               {2, 1}, {1, 1}, {4, 2}, {2, 1}, {1, 1}, {1, 1}};
    if (fn < 0 || fn >= 22 || ((!in || !out) && n)) return MORT_ORACLE_BATCH_BAD_ARGS;
    const size_t iw = shape[fn][0], ow = shape[fn][1];
    for (size_t i = 0; i < n; i++) {
        const uint32_t *a = in + i * iw;
        uint32_t *o = out + i * ow;
        switch (fn) {
        case 0: mb_pf(o, mort_sqrtf(mb_f(a))); break;
        case 1: mb_pd(o, mort_sqrt(mb_d(a))); break;
        case 2: mb_pf(o, mort_floorf(mb_f(a))); break;
        case 3: mb_pf(o, mort_fmaxf(mb_f(a), mb_f(a + 1))); break;
        case 4: mb_pd(o, mort_fmin(mb_d(a), mb_d(a + 2))); break;
        case 5: o[0] = (uint32_t)mort_d2i(mb_d(a)); break;
        case 6: mb_pf(o, mort_powi5f(mb_f(a))); break;
        case 7: mb_pd(o, mort_sin(mb_d(a))); break;
        case 8: mb_pd(o, mort_cos(mb_d(a))); break;
        case 9: mb_pf(o, mort_sinf(mb_f(a))); break;
        case 10: mb_pf(o, mort_cosf(mb_f(a))); break;
        case 11: { float s, c; mort_sincosf(mb_f(a), &s, &c); mb_pf(o, s); mb_pf(o + 1, c); break; }
        case 12: mb_pd(o, mort_atan(mb_d(a))); break;
        case 13: mb_pf(o, mort_atan2f(mb_f(a), mb_f(a + 1))); break;
        case 14: mb_pf(o, mort_acosf(mb_f(a))); break;
        case 15: mb_pf(o, mort_logf(mb_f(a))); break;
        case 16: mb_pf(o, mb_f(a) / mb_f(a + 1)); break;
        case 17: mb_pf(o, 1 / mb_f(a)); break;
        case 18: mb_pd(o, mb_d(a) / mb_d(a + 2)); break;
        case 19: mb_pf(o, (float)mb_d(a)); break;
        case 20: mb_pf(o, (float)a[0]); break;
        default: mb_pf(o, __builtin_truncf(mb_f(a))); break;
        }
    }
    return MORT_ORACLE_BATCH_OK;
}
