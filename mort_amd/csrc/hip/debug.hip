/*
 * debug.hip -- the diagnostics behind mort_amd/hip.py's debug_* calls (only the tile scheduler's, at the end, are in
 * include/mort_hip.h: they read a context's last launch back and drive tile_sort.hip's kernels, and add no kernel).  Most are host only:
 * they compile a world and report what world_images.h decides from it, or run the kernels' DEV bodies on the CPU.  Seven
 * launch small kernels of their own: exact_forms_kernel, f2i_all_kernel and f2i_list_kernel put the device's short forms
 * beside its plain operators, math_kernel runs the math layer on a caller's inputs, light_kernel the light sampling on a caller's
 * records over an uploaded world, shade_kernel the shade step (search + shade_hit) on a caller's records over an uploaded world, random_float_all_kernel sweeps random_float.  mega_bvh.h is included for those bodies; its kernels are templates and none is instantiated here.
 */
#include <hip/hip_runtime.h>

#include <array>
#include <cstring>
#include <thread>
#include <vector>

#include "mort_hip.h"
#include "mega_bvh.h"
#include "scene_blob.h"
#include "mort_ctx.h"
#include "mort_internal.h"
#include "world_images.h"
#include "dev_radiance.h"
#include "query_common.h"

#pragma clang fp contract(off)

/* diagnostic (not in include/mort_hip.h): the per-wave records of the last frame of a profile build run with MORT_WAVE_LINES=1 */
extern "C" int mort_hip_debug_wave_log(mort_ctx *c, unsigned long long *out, size_t max_waves) {
    if (!c || !out || !c->d_wave_log) return 0;
    hipSetDevice(c->device);
    quiesce(c);
    const size_t n = c->wave_log_waves < max_waves ? c->wave_log_waves : max_waves;
    if (hipMemcpy(out, c->d_wave_log, n * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return (int)n;
}

/* diagnostic (not in include/mort_hip.h; host only, no HIP call): facts of this build's own trees over a world -- out[0] binary
 * nodes, [1] leaves, [2] binary depth, [3] four-wide nodes, [4] its pending-children bound, [5] leaf references reached from the
 * four-wide root, [6] leaves reached more than once or out of range, [7] child slots in use, [8] 1 if every four-wide box and margin
 * is bit for bit one of the binary tree's for the same child. */
extern "C" int mort_hip_debug_own_tree(const mort_world *w, int *out) {
    if (!w || !out) return MORT_ERR_INVALID;
    SceneBlob sb;
    const int st = build_scene_blob(w, sb);
    if (st != MORT_OK) return st;
    const mortc::Compiled &o = sb.comp;
    for (int i = 0; i < 9; i++) out[i] = 0;
    out[0] = (int)o.own_nodes.size(); out[1] = (int)o.own_leaves.size(); out[2] = o.own_depth;
    out[3] = (int)o.own_nodes4.size(); out[4] = o.own4_stack;
    if (o.own_nodes4.empty()) return MORT_OK;
    /* child reference -> (box, margin) in the binary tree */
    struct Rec { float v[7]; };
    std::vector<Rec> of_inner(o.own_nodes.size()), of_leaf(o.own_leaves.size());
    for (const DNode2 &nd : o.own_nodes)
        for (int k = 0; k < 2; k++) {
            const uint32_t ref = k ? nd.child1 : nd.child0;
            Rec r = k ? Rec{{nd.x1min, nd.x1max, nd.y1min, nd.y1max, nd.z1min, nd.z1max, nd.e1}} : Rec{{nd.x0min, nd.x0max, nd.y0min, nd.y0max, nd.z0min, nd.z0max, nd.e0}};
            if (ref & 0x8000u) of_leaf[ref & 0x7fffu] = r; else of_inner[ref] = r;
        }
    std::vector<int> seen(o.own_leaves.size(), 0);
    std::vector<uint32_t> todo(1, 0u);
    bool same = true;
    /* every inner child of a four-wide node stands for one binary node: find which by its box, via the leaves below it */
    while (!todo.empty()) {
        const uint32_t n = todo.back(); todo.pop_back();
        const DNode4 &nd = o.own_nodes4[n];
        for (int k = 0; k < 4; k++) {
            const uint32_t ref = nd.child[k];
            if (ref == 0xffffu) continue;
            out[7]++;
            const Rec r{{nd.x[0][k], nd.x[1][k], nd.y[0][k], nd.y[1][k], nd.z[0][k], nd.z[1][k], nd.e[k]}};
            /* the third piece of each axis repeats the first (dev_scene.h) */
            if (std::memcmp(&nd.x[2][k], &nd.x[0][k], 4) || std::memcmp(&nd.y[2][k], &nd.y[0][k], 4) || std::memcmp(&nd.z[2][k], &nd.z[0][k], 4)) same = false;
            if (ref & 0x8000u) {
                const uint32_t l = (ref & 0x7fffu) / MORT_LEAF2_PIECES;
                if ((ref & 0x7fffu) % MORT_LEAF2_PIECES || l >= seen.size() || seen[l]++) { out[6]++; continue; }
                out[5]++;
                if (std::memcmp(&r, &of_leaf[l], sizeof r) != 0) same = false;
            } else {
                if (ref % MORT_NODE4_PIECES || ref / MORT_NODE4_PIECES >= o.own_nodes4.size()) { out[6]++; continue; }
                bool found = false;
                for (const Rec &b : of_inner) if (std::memcmp(&r, &b, sizeof r) == 0) { found = true; break; }
                if (!found) same = false;
                todo.push_back(ref / MORT_NODE4_PIECES);
            }
        }
    }
    out[8] = same ? 1 : 0;
    return MORT_OK;
}

/* diagnostic (not in include/mort_hip.h; host only, no HIP call): what mort_hip_upload_world and the launch of mega_bvh_kernel decide from
 * a world's own trees -- out[0] 1 if the world is one reference BVH over spheres, [1] 1 if it has a four-wide tree, [2] bytes of the BVH
 * megakernel's LDS image (0 without a four-wide tree), [3] bytes of the wavefront traversal kernel's, [4] the limit on either, [5] 1 if mega_bvh_kernel and the wavefront
 * pipeline serve the world (both images within the limit), [6] the traversal stack levels the launch sizes for, [7] 1 if 1024-thread
 * groups fit one CU's LDS with that image and stack. */
extern "C" int mort_hip_debug_bvh_images(const mort_world *w, int *out) {
    if (!w || !out) return MORT_ERR_INVALID;
    SceneBlob sb;
    const int st = build_scene_blob(w, sb);
    if (st != MORT_OK) return st;
    const mortc::Compiled &o = sb.comp;
    for (int i = 0; i < 8; i++) out[i] = 0;
    out[0] = one_sphere_bvh(o) ? 1 : 0; out[1] = (!o.own_nodes.empty() && !o.own_nodes4.empty()) ? 1 : 0; out[4] = MORT_BVH_IMAGE_MAX;
    if (!out[0] || o.own_nodes.empty()) return MORT_OK;
    BvhImages im;
    build_bvh_images(o, im);
    out[3] = (int)im.tb.size(); /* the binary tree's image exists without a four-wide tree, and tells how big the world is */
    if (!out[1]) return MORT_OK;
    out[2] = (int)im.fb.size(); out[5] = im.fits ? 1 : 0;
    out[6] = o.own4_stack > 1 ? o.own4_stack : 1;
    out[7] = (im.fits && bvh_wide_block_fits((uint32_t)im.fb.size(), out[6])) ? 1 : 0;
    return MORT_OK;
}

/* diagnostic (not in include/mort_hip.h; host only, no HIP call): where the unified tree of a world may be walked from -- out[0] 1 if
 * the world has a unified tree (else the rest is 0), [1..3] the low corner of its solids' box, [4..6] the high corner, [7] the reach:
 * a ray origin o is walked iff lo[k] - reach <= o[k] <= hi[k] + reach on every axis (camera_in_reach; per ray in dev_query.h). */
extern "C" int mort_hip_debug_gen_reach(const mort_world *w, float *out) {
    if (!w || !out) return MORT_ERR_INVALID;
    SceneBlob sb;
    const int st = build_scene_blob(w, sb);
    if (st != MORT_OK) return st;
    const mortc::Compiled &o = sb.comp;
    for (int i = 0; i < 8; i++) out[i] = 0;
    if (!o.g_ok) return MORT_OK;
    out[0] = 1;
    for (int k = 0; k < 3; k++) { out[1 + k] = o.g_lo[k]; out[4 + k] = o.g_hi[k]; }
    out[7] = o.g_reach;
    return MORT_OK;
}

/* diagnostic (not in include/mort_hip.h; host only, no HIP call): the unified tree of a world and what mort_hip_upload_world decides
 * from it (build_gen_image, MORT_NO_GEN aside) -- iout[0] 1 if the world has a unified tree (else the rest is 0), [1] nodes, [2] entries,
 * [3] depth, [4] chain ids (id 0, no transform, included), [5] bytes of the LDS image before the primitives, [6] bytes of the primitives,
 * [7] 1 if the primitives are in the image, [8] bytes of the LDS part of the image, [9] 1 if that is within MORT_GEN_IMAGE_MAX (the
 * unified-tree kernels serve the world), [10] MORT_GEN_IMAGE_MAX, [11] the limit on image + primitives for the primitives to be in LDS,
 * [12] nodes whose split the depth cap chose over the best surface-area split (gen_emit);
 * fout[0] g_R, [1] g_mnear, [2] g_kmin, [3] g_reach, [4..6] g_c (gen_ray_setup's arguments). */
extern "C" int mort_hip_debug_gen_tree(const mort_world *w, int *iout, float *fout) {
    if (!w || !iout || !fout) return MORT_ERR_INVALID;
    SceneBlob sb;
    const int st = build_scene_blob(w, sb);
    if (st != MORT_OK) return st;
    const mortc::Compiled &o = sb.comp;
    for (int i = 0; i < 13; i++) iout[i] = 0;
    for (int i = 0; i < 7; i++) fout[i] = 0;
    if (!o.g_ok) return MORT_OK;
    GenImage gi;
    build_gen_image(o, gi);
    iout[0] = 1; iout[1] = (int)o.g_nodes.size(); iout[2] = (int)o.g_entries.size(); iout[3] = o.g_depth; iout[4] = gi.g.n_chains;
    iout[5] = (int)gi.table_bytes; iout[6] = (int)gi.prim_bytes; iout[7] = gi.g.prims_in_lds; iout[8] = (int)gi.lds_part;
    iout[9] = gi.fits ? 1 : 0; iout[10] = MORT_GEN_IMAGE_MAX; iout[11] = MORT_GEN_PRIMS_LDS_MAX; iout[12] = o.g_capped;
    fout[0] = gi.g.gR; fout[1] = gi.g.mnear; fout[2] = gi.g.kmin; fout[3] = o.g_reach; fout[4] = gi.g.gx; fout[5] = gi.g.gy; fout[6] = gi.g.gz;
    return MORT_OK;
}

/* diagnostic (not in include/mort_hip.h; host only, no HIP call): the boxes of the occupied children of the world's four-wide tree, six
 * floats each (xmin, xmax, ymin, ymax, zmin, zmax), at most max_boxes of them.  Returns how many there are, or a negative status. */
extern "C" int mort_hip_debug_own_tree4_boxes(const mort_world *w, float *out, size_t max_boxes) {
    if (!w || (!out && max_boxes)) return MORT_ERR_INVALID;
    SceneBlob sb;
    const int st = build_scene_blob(w, sb);
    if (st != MORT_OK) return st;
    size_t n = 0;
    for (const DNode4 &nd : sb.comp.own_nodes4)
        for (int k = 0; k < 4; k++) {
            if (nd.child[k] == 0xffffu) continue;
            if (n < max_boxes) { float *o = out + 6 * n; o[0] = nd.x[0][k]; o[1] = nd.x[1][k]; o[2] = nd.y[0][k]; o[3] = nd.y[1][k]; o[4] = nd.z[0][k]; o[5] = nd.z[1][k]; }
            n++;
        }
    return (int)n;
}

/* diagnostic (not in include/mort_hip.h; host only, no HIP call): the box step's two forms of the slab test, own_prune on (min, max) and
 * own_prune_ordered on the sign-chosen (near, far) pieces, over the world's four-wide tree, the pieces chosen by own_sign_offset as in the kernel.
 * rays: n x 7 floats (origin, direction, closest); ray r meets the nodes r % stride, r % stride + stride, ...  A ray whose reciprocals
 * are not ordinary never reaches the box step and is only counted.  out[0] (occupied child, ray) pairs compared, [1] pairs whose te differs
 * in any bit, [2] pairs whose skip decision differs, [3] rays left out, [4] four-wide nodes, [5] unused child slots with a non-zero plane
 * or margin, [6] pairs skipped by both forms, [8..15] rays compared per sign octant (bit 0: x reciprocal negative, 1: y, 2: z). */
extern "C" int mort_hip_debug_prune_forms(const mort_world *w, const float *rays, size_t n, int stride, unsigned long long *out) {
    if (!w || !rays || !out || stride < 1) return MORT_ERR_INVALID;
    SceneBlob sb;
    const int st = build_scene_blob(w, sb);
    if (st != MORT_OK) return st;
    const std::vector<DNode4> &nodes = sb.comp.own_nodes4;
    for (int i = 0; i < 16; i++) out[i] = 0;
    out[4] = nodes.size();
    if (nodes.empty()) return MORT_OK;
    for (const DNode4 &nd : nodes)
        for (int k = 0; k < 4; k++) {
            if (nd.child[k] != 0xffffu) continue;
            const float v[10] = {nd.x[0][k], nd.x[1][k], nd.x[2][k], nd.y[0][k], nd.y[1][k], nd.y[2][k], nd.z[0][k], nd.z[1][k], nd.z[2][k], nd.e[k]};
            for (float f : v) { uint32_t b; std::memcpy(&b, &f, 4); if (b) { out[5]++; break; } }
        }
    unsigned nthreads = std::thread::hardware_concurrency();
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 16) nthreads = 16;
    std::vector<std::array<unsigned long long, 16>> part(nthreads);
    auto work = [&](unsigned t) {
        std::array<unsigned long long, 16> &o = part[t];
        o.fill(0);
        for (size_t r = t; r < n; r += nthreads) {
            const float *q = rays + 7 * r;
            OwnRay orr; /* as the kernel's segment setup (mega_bvh.h) */
            orr.ix = 1.0f / q[3]; orr.iy = 1.0f / q[4]; orr.iz = 1.0f / q[5];
            orr.mx = q[0] * orr.ix; orr.my = q[1] * orr.iy; orr.mz = q[2] * orr.iz;
            const float mm = __builtin_fmaxf(__builtin_fmaxf(mort_fabsf(orr.mx), mort_fabsf(orr.my)), mort_fabsf(orr.mz));
            orr.band = mm * 4.76837158203125e-07f;
            orr.invlen = 1.01f / mort_sqrtf(q[3] * q[3] + q[4] * q[4] + q[5] * q[5]);
            if (!(own_inv_ok(orr.ix) && own_inv_ok(orr.iy) && own_inv_ok(orr.iz) && (mm < 1e30f))) { o[3]++; continue; }
            const uint32_t sx = own_sign_offset(orr.ix) / 16u, sy = own_sign_offset(orr.iy) / 16u, sz = own_sign_offset(orr.iz) / 16u;
            o[8 + (sx | sy << 1 | sz << 2)]++;
            const float closest = q[6];
            for (size_t ni = r % (size_t)stride; ni < nodes.size(); ni += (size_t)stride) {
                const DNode4 &nd = nodes[ni];
                for (int k = 0; k < 4; k++) {
                    if (nd.child[k] == 0xffffu) continue;
                    float te_a, te_b;
                    const bool skip_a = own_prune(nd.x[0][k], nd.x[1][k], nd.y[0][k], nd.y[1][k], nd.z[0][k], nd.z[1][k], nd.e[k], orr, closest, te_a);
                    const bool skip_b = own_prune_ordered(nd.x[sx][k], nd.x[sx + 1][k], nd.y[sy][k], nd.y[sy + 1][k], nd.z[sz][k], nd.z[sz + 1][k], nd.e[k], orr, closest, te_b);
                    o[0]++;
                    if (std::memcmp(&te_a, &te_b, 4) != 0) o[1]++;
                    if (skip_a != skip_b) o[2]++;
                    if (skip_a && skip_b) o[6]++;
                }
            }
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nthreads; t++) pool.emplace_back(work, t);
    work(0);
    for (std::thread &th : pool) th.join();
    for (const auto &o : part) for (int i = 0; i < 16; i++) if (i != 4 && i != 5) out[i] += o[i];
    return MORT_OK;
}

/* diagnostic (not in include/mort_hip.h; host only, no HIP call): dev_math.h's guards of the short forms, per value: bit 0 div_den_ok,
 * bit 1 div_num_ok, bit 2 sqrt_arg_ok */
extern "C" int mort_hip_debug_exact_guards(const float *v, size_t n, unsigned char *flags) {
    if ((!v || !flags) && n) return MORT_ERR_INVALID;
    for (size_t i = 0; i < n; i++) flags[i] = (unsigned char)((div_den_ok(v[i]) ? 1 : 0) | (div_num_ok(v[i]) ? 2 : 0) | (sqrt_arg_ok(v[i]) ? 4 : 0));
    return MORT_OK;
}

/* diagnostic (not in include/mort_hip.h; host only, no HIP call): the MODELS of the short forms (dev_math.h: the fma sequences as plain
 * C++, the hardware's seed a parameter) against the host's correctly rounded operators.
 *   what 0: sqrt_ord_model(x[i], seed) against sqrtf(x[i]), seed = sqrtf(x[i]) moved by every offset in [seed_lo, seed_hi] units of its
 *           last place; `a` is not read;
 *   what 1: div_by_model(x[i], a[i], div_by_model_prepare(a[i], seed)) against x[i] / a[i], seed = fl(1 / a[i]) moved likewise.
 * Inputs outside the guards (sqrt_arg_ok; div_den_ok and 2^-85 <= |x| < 2^56) are only counted.  out[0] comparisons, [1] those that
 * differ in any bit, [2] inputs outside the guards, [8..15] the indices of the first inputs that differ. */
extern "C" int mort_hip_debug_exact_forms_model(int what, const float *x, const float *a, size_t n, int seed_lo, int seed_hi, unsigned long long *out) {
    if (!x || !out || (what != 0 && what != 1) || (what == 1 && !a) || seed_lo > seed_hi) return MORT_ERR_INVALID;
    for (int i = 0; i < 16; i++) out[i] = 0;
    for (size_t i = 0; i < n; i++) {
        const bool inside = what == 0 ? sqrt_arg_ok(x[i]) : (div_den_ok(a[i]) && div_num_ok(x[i]) && mort_fabsf(x[i]) >= 0x1p-85f);
        if (!inside) { out[2]++; continue; }
        const float want = what == 0 ? mort_sqrtf(x[i]) : x[i] / a[i];
        const float seed0 = what == 0 ? want : 1.0f / a[i];
        for (int k = seed_lo; k <= seed_hi; k++) {
            const float seed = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, seed0) + (uint32_t)k);
            const float got = what == 0 ? sqrt_ord_model(x[i], seed) : div_by_model(x[i], a[i], div_by_model_prepare(a[i], seed));
            out[0]++;
            if (std::memcmp(&got, &want, 4) != 0) { if (out[1] < 8) out[8 + out[1]] = i; out[1]++; }
        }
    }
    return MORT_OK;
}

/* the device forms against the device's own operators, one element per lane and round (mort_hip_debug_exact_forms_device) */
__device__ __forceinline__ void exact_forms_count(unsigned long long *slot, bool cond) {
    const unsigned long long m = __ballot(cond);
    if (m != 0ull && (int)(threadIdx.x & 63u) == __ffsll((long long)m) - 1) atomicAdd(slot, (unsigned long long)__popcll(m));
}
static __global__ void __launch_bounds__(256) exact_forms_kernel(int what, const float *in, size_t n, unsigned long long *out) {
    const size_t stride = (size_t)gridDim.x * 256;
    const size_t rounds = (n + stride - 1) / stride; /* every lane runs every round: the ballots see whole waves */
    for (size_t k = 0; k < rounds; k++) {
        const size_t i = k * stride + (size_t)blockIdx.x * 256 + threadIdx.x;
        const bool live = i < n;
        bool compared = false, differs = false, outside = false, small = false, short_path = false, generic_path = false, short_hit = false, generic_hit = false;
        if (live && what == 0) {
            const float x = in[i];
            if (sqrt_arg_ok(x)) {
                compared = true;
                differs = __float_as_uint(sqrt_ord(x)) != __float_as_uint(mort_sqrtf(x));
            } else outside = true;
        } else if (live && what == 1) {
            const float x = in[2 * i], a = in[2 * i + 1];
            const DivBy dv = div_prepare(a);
            if (dv.ok && div_num_ok(x)) {
                const float got = div_by(x, dv), want = x / a;
                if (mort_fabsf(x) >= 0x1p-85f) { compared = true; differs = __float_as_uint(got) != __float_as_uint(want); }
                else { small = true; differs = !(mort_fabsf(got) < 0x1p-44f && mort_fabsf(want) < 0x1p-44f); } /* both finite and below any t_min >= 2^-44 */
            } else outside = true;
        } else if (live) {
            const float *q = in + 16 * i;
            Ray ray; ray.o = mk(q[0], q[1], q[2]); ray.d = mk(q[3], q[4], q[5]); ray.tm = q[6];
            const float t_max = q[7];
            DSphere s;
            s.cx = q[8]; s.cy = q[9]; s.cz = q[10]; s.radius = q[11]; s.vx = q[12]; s.vy = q[13]; s.vz = q[14];
            s.mat = q[15] != 0.0f ? 0x80000000u : 0u; /* bit 31: the sphere moves (dev_scene.h) */
            const float a = vlen2(ray.d);
            const DivBy dv = div_prepare(a);
            const float got = sphere_hit_root_fast(s, ray, dv, 0.001f, t_max), want = sphere_hit_root(s, ray, a, 0.001f, t_max);
            compared = true;
            differs = __float_as_uint(got) != __float_as_uint(want);
            const SphereQuad sq = sphere_quadratic(s, ray, a);
            short_path = sphere_short_ok(sq.discriminant, sq.hb2, dv);
            generic_path = !short_path && !(sq.discriminant < 0);
            short_hit = short_path && want != -1.0f;
            generic_hit = generic_path && want != -1.0f;
        }
        exact_forms_count(&out[0], compared);
        exact_forms_count(&out[2], outside);
        exact_forms_count(&out[3], small);
        exact_forms_count(&out[4], short_path);
        exact_forms_count(&out[5], generic_path);
        exact_forms_count(&out[6], short_hit);
        exact_forms_count(&out[7], generic_hit);
        if (differs) { const unsigned long long at = atomicAdd(&out[1], 1ull); if (at < 8ull) out[8 + at] = (unsigned long long)i; }
    }
}

/* diagnostic (not in include/mort_hip.h): one launch of the kernel above on `device`, the short forms against the plain operators ON THE DEVICE.
 *   what 0: in = n values x: sqrt_ord(x) against sqrtf(x) where sqrt_arg_ok(x);
 *   what 1: in = n pairs (x, a): div_by(x, div_prepare(a)) against x / a where div_den_ok(a) and div_num_ok(x); a numerator below 2^-85 is
 *           checked for what dev_math.h promises instead: both quotients below 2^-44 in magnitude;
 *   what 2: in = n records of 16 floats (ray origin, direction, time, t_max; sphere centre, radius, velocity, moves != 0):
 *           sphere_hit_root_fast against sphere_hit_root with t_min = 0.001, a = the direction's squared length.
 * out[0] elements compared bit for bit, [1] elements that fail, [2] outside the guards (what 0, 1), [3] small numerators (what 1), what 2:
 * [4] records on the short branch, [5] on the generic branch past its miss test, [6] / [7] accepted roots of either, [8..15] first failing elements. */
extern "C" int mort_hip_debug_exact_forms_device(int device, int what, const float *in, size_t n, unsigned long long *out) {
    if (!in || !out || what < 0 || what > 2 || n == 0) return MORT_ERR_INVALID;
    const size_t per = what == 0 ? 1 : what == 1 ? 2 : 16;
    int caller_device = -1;
    if (hipGetDevice(&caller_device) != hipSuccess) caller_device = -1;
    if (hipSetDevice(device) != hipSuccess) return MORT_ERR_NO_DEVICE;
    float *d_in = nullptr;
    unsigned long long *d_out = nullptr;
    int st = MORT_OK;
    if (hipMalloc((void **)&d_in, n * per * sizeof(float)) != hipSuccess || hipMalloc((void **)&d_out, 16 * sizeof(unsigned long long)) != hipSuccess) st = MORT_ERR_NOMEM;
    if (st == MORT_OK && (hipMemcpy(d_in, in, n * per * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
                          hipMemset(d_out, 0, 16 * sizeof(unsigned long long)) != hipSuccess)) st = MORT_ERR_HIP;
    if (st == MORT_OK) {
        const size_t blocks = (n + 255) / 256;
        exact_forms_kernel<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256)>>>(what, d_in, n, d_out);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(out, d_out, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) st = MORT_ERR_HIP;
    }
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    if (caller_device >= 0 && caller_device != device) (void)hipSetDevice(caller_device); /* the caller's current device, as it was */
    return st;
}

/* diagnostic (not in include/mort_hip.h; host only, no HIP call): the bounce-stack levels a launch of mega_bvh_kernel keeps in LDS beside
 * the world's image -- out[0] the image's bytes (0: the world is not served by that kernel, the rest is 0 too), out[1..3] the levels on
 * 1024-, 768- and 256-thread workgroups (state_lds_levels with the kernel's 1 KB of static LDS); deeper levels go to HBM. */
extern "C" int mort_hip_debug_bvh_lds_levels(const mort_world *w, int *out) {
    if (!w || !out) return MORT_ERR_INVALID;
    SceneBlob sb;
    const int st = build_scene_blob(w, sb);
    if (st != MORT_OK) return st;
    const mortc::Compiled &o = sb.comp;
    for (int i = 0; i < 4; i++) out[i] = 0;
    if (!one_sphere_bvh(o) || o.own_nodes.empty() || o.own_nodes4.empty()) return MORT_OK;
    BvhImages im;
    build_bvh_images(o, im);
    if (!im.fits) return MORT_OK;
    const uint32_t levels = (uint32_t)(o.own4_stack > 1 ? o.own4_stack : 1) + MORT_BVH_TSTACK_SPARE;
    const int shapes[3] = {1024, 768, 256};
    out[0] = (int)im.fb.size();
    for (int k = 0; k < 3; k++) { uint32_t a = 0, b = 0; out[1 + k] = state_lds_levels((uint32_t)im.fb.size(), shapes[k], levels, 1024u, 1, a, b); }
    return MORT_OK;
}

/* the device side of mort_f2i (mort_math.h: one v_cvt_i32_f32) against mort_f2i_select compiled beside it, over ALL 2^32 bit patterns
 * (every lane takes every 2^20-th pattern), and its results for a list of patterns (mort_hip_debug_f2i_device) */

/* mort_f2i without a branch or an instruction by name: (int)x of an in-range value, guarded by selects */
__device__ __forceinline__ int mort_f2i_select(float x) {
    const bool in_range = (x > -2147483648.0f) && (x < 2147483648.0f);
    const int t = (int)(in_range ? x : 0.0f);
    return (x != x) ? 0 : (x >= 2147483648.0f) ? 2147483647 : (x <= -2147483648.0f) ? (-2147483647 - 1) : t;
}
static __global__ void __launch_bounds__(256) f2i_all_kernel(unsigned long long *out) {
    const uint32_t first = blockIdx.x * 256u + threadIdx.x; /* 4096 blocks: 2^20 lanes, 2^12 patterns each */
    uint32_t differ = 0, lowest = 0xffffffffu;
    for (uint32_t k = 0; k < 4096u; k++) {
        const uint32_t bits = first + (k << 20);
        const float x = __uint_as_float(bits);
        if (mort_f2i(x) != mort_f2i_select(x)) { differ++; lowest = bits < lowest ? bits : lowest; }
    }
    atomicAdd(&out[2], 4096ull);
    if (differ) { atomicAdd(&out[0], (unsigned long long)differ); atomicMin(&out[1], (unsigned long long)lowest); }
}
static __global__ void __launch_bounds__(256) f2i_list_kernel(const uint32_t *bits, size_t n, int *res) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) res[i] = mort_f2i(__uint_as_float(bits[i]));
}

/* diagnostic (not in include/mort_hip.h): on `device`, out[0] = how many of the 2^32 float bit patterns the device's mort_f2i and
 * mort_f2i_select convert differently, out[1] = the lowest such pattern (2^32 - 1 if none), out[2] = patterns visited; res[i] = the device's
 * mort_f2i of bits[i] for the n listed patterns (n may be 0). */
extern "C" int mort_hip_debug_f2i_device(int device, const uint32_t *bits, size_t n, int *res, unsigned long long *out) {
    if (!out || (n && (!bits || !res)) || n > ((size_t)1 << 28)) return MORT_ERR_INVALID;
    int caller_device = -1;
    if (hipGetDevice(&caller_device) != hipSuccess) caller_device = -1;
    if (hipSetDevice(device) != hipSuccess) return MORT_ERR_NO_DEVICE;
    uint32_t *d_bits = nullptr;
    int *d_res = nullptr;
    unsigned long long *d_out = nullptr;
    const unsigned long long init[3] = {0ull, 0xffffffffull, 0ull};
    int st = MORT_OK;
    if (hipMalloc((void **)&d_out, sizeof init) != hipSuccess) st = MORT_ERR_NOMEM;
    if (st == MORT_OK && n && (hipMalloc((void **)&d_bits, n * 4) != hipSuccess || hipMalloc((void **)&d_res, n * 4) != hipSuccess)) st = MORT_ERR_NOMEM;
    if (st == MORT_OK && (hipMemcpy(d_out, init, sizeof init, hipMemcpyHostToDevice) != hipSuccess ||
                          (n && hipMemcpy(d_bits, bits, n * 4, hipMemcpyHostToDevice) != hipSuccess))) st = MORT_ERR_HIP;
    if (st == MORT_OK) {
        f2i_all_kernel<<<dim3(4096), dim3(256)>>>(d_out);
        if (n) f2i_list_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(d_bits, n, d_res);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(out, d_out, sizeof init, hipMemcpyDeviceToHost) != hipSuccess ||
            (n && hipMemcpy(res, d_res, n * 4, hipMemcpyDeviceToHost) != hipSuccess)) st = MORT_ERR_HIP;
    }
    if (d_bits) (void)hipFree(d_bits);
    if (d_res) (void)hipFree(d_res);
    if (d_out) (void)hipFree(d_out);
    if (caller_device >= 0 && caller_device != device) (void)hipSetDevice(caller_device); /* the caller's current device, as it was */
    return st;
}
/* host only, no HIP call: the host's mort_f2i of the same patterns (what gcc makes of the same source is tests/test_math.py's business) */
extern "C" int mort_hip_debug_f2i_host(const uint32_t *bits, size_t n, int *res) {
    if ((!bits || !res) && n) return MORT_ERR_INVALID;
    for (size_t i = 0; i < n; i++) res[i] = mort_f2i(__builtin_bit_cast(float, bits[i]));
    return MORT_OK;
}

/* ---- the math layer on a caller's inputs: mort_math.h (group A), the plain operators the contract leans on (P), dev_math.h (B) and
 * dev_trace.h's uv / texture functions (C), one function number each.  Records are 32-bit words, a double is two (low word first).
 * math_eval is the one body behind mort_hip_debug_math_host (hipcc's host compile) and math_kernel (the gfx950 compile);
 * oracle/mort_oracle.c's mort_oracle_math_batch is gcc's compile of group A under the same numbers (tests/test_math.py,
 * tests/test_gpu_math.py). ---- */
struct MathShape { unsigned char in, out; };
static const MathShape MATH_SHAPES[] = {
    /* A  0 mort_sqrtf x -> f            */ {1, 1},  /*  1 mort_sqrt x -> d               */ {2, 2},
    /*    2 mort_floorf x -> f           */ {1, 1},  /*  3 mort_fmaxf a b -> f            */ {2, 1},
    /*    4 mort_fmin a b -> d           */ {4, 2},  /*  5 mort_d2i x -> int              */ {2, 1},
    /*    6 mort_powi5f a -> f           */ {1, 1},  /*  7 mort_sin x -> d                */ {2, 2},
    /*    8 mort_cos x -> d              */ {2, 2},  /*  9 mort_sinf x -> f               */ {1, 1},
    /*   10 mort_cosf x -> f             */ {1, 1},  /* 11 mort_sincosf x -> sin, cos     */ {1, 2},
    /*   12 mort_atan x -> d             */ {2, 2},  /* 13 mort_atan2f y x -> f           */ {2, 1},
    /*   14 mort_acosf x -> f            */ {1, 1},  /* 15 mort_logf x -> f               */ {1, 1},
    /* P 16 fp32 x / a                   */ {2, 1},  /* 17 fp32 1 / a                     */ {1, 1},
    /*   18 fp64 x / a                   */ {4, 2},  /* 19 (float) of a double            */ {2, 1},
    /*   20 (float) of a uint32_t        */ {1, 1},  /* 21 __builtin_truncf               */ {1, 1},
    /* B 22 vlen v -> f                  */ {3, 1},  /* 23 vdiv v t -> v                  */ {4, 3},
    /*   24 vunit v -> v                 */ {3, 3},  /* 25 vcross u v -> v                */ {6, 3},
    /*   26 reflect v n -> v             */ {6, 3},  /* 27 refract uv n eta -> v          */ {7, 3},
    /*   28 reflectance cos idx -> f     */ {2, 1},  /* 29 onb_from_w w, onb_local a -> u v w local */ {6, 12},
    /*   stream functions: the six XORWOW words (d, v0..v4) lead the record; the value, the six final words and the draw count come back */
    /*   30 random_float_range mn mx     */ {8, 8},  /* 31 random_int mn mx               */ {8, 8},
    /*   32 random_in_unit_sphere        */ {6, 10}, /* 33 random_unit_vector             */ {6, 10},
    /*   34 random_in_unit_disk          */ {6, 10}, /* 35 random_cosine_direction        */ {6, 10},
    /* C 36 sphere_uv p -> u v           */ {3, 2},  /* 37 noise_value idx p -> rgb       */ {4, 3},
    /*   38 image_value idx u v -> rgb   */ {3, 3},
};
#define MATH_FUNCTIONS ((int)(sizeof MATH_SHAPES / sizeof MATH_SHAPES[0]))
#define MATH_FN_NOISE 37
#define MATH_FN_IMAGE 38
struct MathTables { const float *noise; const DImage *images; const unsigned char *texels; };

DEV float math_f(const uint32_t *w, int k) { return __builtin_bit_cast(float, w[k]); }
DEV double math_d(const uint32_t *w, int k) { return __builtin_bit_cast(double, (uint64_t)w[k] | ((uint64_t)w[k + 1] << 32)); }
DEV V3 math_v(const uint32_t *w, int k) { return mk(math_f(w, k), math_f(w, k + 1), math_f(w, k + 2)); }
DEV void math_pf(uint32_t *w, int k, float x) { w[k] = __builtin_bit_cast(uint32_t, x); }
DEV void math_pd(uint32_t *w, int k, double x) { const uint64_t u = __builtin_bit_cast(uint64_t, x); w[k] = (uint32_t)u; w[k + 1] = (uint32_t)(u >> 32); }
DEV void math_pv(uint32_t *w, int k, V3 v) { math_pf(w, k, v.x); math_pf(w, k + 1, v.y); math_pf(w, k + 2, v.z); }
DEV Rng math_rng(const uint32_t *w) { Rng s; s.d = w[0]; s.v0 = w[1]; s.v1 = w[2]; s.v2 = w[3]; s.v3 = w[4]; s.v4 = w[5]; s.draws = 0; return s; }
DEV void math_prng(uint32_t *w, int k, const Rng &s) { w[k] = s.d; w[k + 1] = s.v0; w[k + 2] = s.v1; w[k + 3] = s.v2; w[k + 4] = s.v3; w[k + 5] = s.v4; w[k + 6] = s.draws; }

static __host__ __device__ void math_eval(int fn, const uint32_t *in, uint32_t *out, const MathTables &t) {
    switch (fn) {
    case 0: math_pf(out, 0, mort_sqrtf(math_f(in, 0))); break;
    case 1: math_pd(out, 0, mort_sqrt(math_d(in, 0))); break;
    case 2: math_pf(out, 0, mort_floorf(math_f(in, 0))); break;
    case 3: math_pf(out, 0, mort_fmaxf(math_f(in, 0), math_f(in, 1))); break;
    case 4: math_pd(out, 0, mort_fmin(math_d(in, 0), math_d(in, 2))); break;
    case 5: out[0] = (uint32_t)mort_d2i(math_d(in, 0)); break;
    case 6: math_pf(out, 0, mort_powi5f(math_f(in, 0))); break;
    case 7: math_pd(out, 0, mort_sin(math_d(in, 0))); break;
    case 8: math_pd(out, 0, mort_cos(math_d(in, 0))); break;
    case 9: math_pf(out, 0, mort_sinf(math_f(in, 0))); break;
    case 10: math_pf(out, 0, mort_cosf(math_f(in, 0))); break;
    case 11: { float s, c; mort_sincosf(math_f(in, 0), &s, &c); math_pf(out, 0, s); math_pf(out, 1, c); break; }
    case 12: math_pd(out, 0, mort_atan(math_d(in, 0))); break;
    case 13: math_pf(out, 0, mort_atan2f(math_f(in, 0), math_f(in, 1))); break;
    case 14: math_pf(out, 0, mort_acosf(math_f(in, 0))); break;
    case 15: math_pf(out, 0, mort_logf(math_f(in, 0))); break;
    case 16: math_pf(out, 0, math_f(in, 0) / math_f(in, 1)); break;
    case 17: math_pf(out, 0, 1 / math_f(in, 0)); break;
    case 18: math_pd(out, 0, math_d(in, 0) / math_d(in, 2)); break;
    case 19: math_pf(out, 0, (float)math_d(in, 0)); break;
    case 20: math_pf(out, 0, (float)in[0]); break;
    case 21: math_pf(out, 0, __builtin_truncf(math_f(in, 0))); break;
    case 22: math_pf(out, 0, vlen(math_v(in, 0))); break;
    case 23: math_pv(out, 0, vdiv(math_v(in, 0), math_f(in, 3))); break;
    case 24: math_pv(out, 0, vunit(math_v(in, 0))); break;
    case 25: math_pv(out, 0, vcross(math_v(in, 0), math_v(in, 3))); break;
    case 26: math_pv(out, 0, reflect(math_v(in, 0), math_v(in, 3))); break;
    case 27: math_pv(out, 0, refract(math_v(in, 0), math_v(in, 3), math_f(in, 6))); break;
    case 28: math_pf(out, 0, reflectance(math_f(in, 0), math_f(in, 1))); break;
    case 29: { const Onb o = onb_from_w(math_v(in, 0)); math_pv(out, 0, o.u); math_pv(out, 3, o.v); math_pv(out, 6, o.w); math_pv(out, 9, onb_local(o, math_v(in, 3))); break; }
    case 30: { Rng s = math_rng(in); math_pf(out, 0, random_float_range(s, math_f(in, 6), math_f(in, 7))); math_prng(out, 1, s); break; }
    case 31: { Rng s = math_rng(in); out[0] = (uint32_t)random_int(s, (int)in[6], (int)in[7]); math_prng(out, 1, s); break; }
    case 32: { Rng s = math_rng(in); math_pv(out, 0, random_in_unit_sphere(s)); math_prng(out, 3, s); break; }
    case 33: { Rng s = math_rng(in); math_pv(out, 0, random_unit_vector(s)); math_prng(out, 3, s); break; }
    case 34: { Rng s = math_rng(in); math_pv(out, 0, random_in_unit_disk(s)); math_prng(out, 3, s); break; }
    case 35: { Rng s = math_rng(in); math_pv(out, 0, random_cosine_direction(s)); math_prng(out, 3, s); break; }
    case 36: { float u, v; sphere_uv(math_v(in, 0), u, v); math_pf(out, 0, u); math_pf(out, 1, v); break; }
    case MATH_FN_NOISE: math_pv(out, 0, noise_value(t.noise, (int)in[0], math_v(in, 1))); break;
    case MATH_FN_IMAGE: math_pv(out, 0, image_value(t.images, t.texels, (int)in[0], math_f(in, 1), math_f(in, 2))); break;
    default: break;
    }
}

/* what the table functions may read: every record's index inside its table, every image inside the texels */
static int math_check_tables(int fn, const uint32_t *in, size_t n, const void *noise, size_t noise_bytes, const DImage *images, size_t n_images,
                             const void *texels, size_t texel_bytes) {
    if (fn == MATH_FN_NOISE) {
        const size_t count = noise_bytes / sizeof(mort_noise_texture);
        if (!noise || count == 0 || noise_bytes % sizeof(mort_noise_texture)) return MORT_ERR_INVALID;
        for (size_t k = 0; k < count; k++) { /* the permutations index ranvec */
            const mort_noise_texture &nt = ((const mort_noise_texture *)noise)[k];
            for (int j = 0; j < MORT_POINT_COUNT; j++)
                if ((unsigned)nt.perm_x[j] > 255u || (unsigned)nt.perm_y[j] > 255u || (unsigned)nt.perm_z[j] > 255u) return MORT_ERR_INVALID;
        }
        for (size_t i = 0; i < n; i++) if (in[4 * i] >= count) return MORT_ERR_INVALID;
    } else if (fn == MATH_FN_IMAGE) {
        if (!images || n_images == 0 || (!texels && texel_bytes)) return MORT_ERR_INVALID;
        for (size_t k = 0; k < n_images; k++) {
            const DImage &im = images[k];
            if (im.height <= 0) continue; /* image_value returns before it reads a texel */
            if (im.width <= 0 || im.width > 65536 || im.height > 65536) return MORT_ERR_INVALID;
            if ((size_t)im.offset + (size_t)im.width * 3 * (size_t)im.height > texel_bytes) return MORT_ERR_INVALID;
        }
        for (size_t i = 0; i < n; i++) if (in[3 * i] >= n_images) return MORT_ERR_INVALID;
    }
    return MORT_OK;
}

/* diagnostic (not in include/mort_hip.h; host only, no HIP call): the record shape of function fn in 32-bit words; MORT_ERR_INVALID
 * past the last function */
extern "C" int mort_hip_debug_math_shape(int fn, int *in_words, int *out_words) {
    if (fn < 0 || fn >= MATH_FUNCTIONS || !in_words || !out_words) return MORT_ERR_INVALID;
    *in_words = MATH_SHAPES[fn].in; *out_words = MATH_SHAPES[fn].out;
    return MORT_OK;
}

/* diagnostic (not in include/mort_hip.h; host only, no HIP call): function fn over n records, hipcc's host compile of math_eval.
 * noise: mort_noise_texture records (fn 37); images / texels: DImage records {offset, width, height, 0} and the bytes they index (fn 38);
 * NULL / 0 for every other function. */
extern "C" int mort_hip_debug_math_host(int fn, const uint32_t *in, size_t n, uint32_t *out, const void *noise, size_t noise_bytes,
                                        const void *images, size_t n_images, const void *texels, size_t texel_bytes) {
    if (fn < 0 || fn >= MATH_FUNCTIONS || ((!in || !out) && n)) return MORT_ERR_INVALID;
    const int st = math_check_tables(fn, in, n, noise, noise_bytes, (const DImage *)images, n_images, texels, texel_bytes);
    if (st != MORT_OK) return st;
    const MathTables t{(const float *)noise, (const DImage *)images, (const unsigned char *)texels};
    const size_t iw = MATH_SHAPES[fn].in, ow = MATH_SHAPES[fn].out;
    unsigned nthreads = std::thread::hardware_concurrency();
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 16) nthreads = 16;
    if (n < 4096) nthreads = 1;
    auto work = [&](unsigned k) {
        for (size_t i = n * k / nthreads, end = n * (k + 1) / nthreads; i < end; i++) math_eval(fn, in + i * iw, out + i * ow, t);
    };
    std::vector<std::thread> pool;
    for (unsigned k = 1; k < nthreads; k++) pool.emplace_back(work, k);
    work(0);
    for (std::thread &th : pool) th.join();
    return MORT_OK;
}

/* one lane per record, grid-stride; results leave as raw words */
static __global__ void __launch_bounds__(256) math_kernel(int fn, int iw, int ow, const uint32_t *in, size_t n, uint32_t *out, MathTables t) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) math_eval(fn, in + i * (size_t)iw, out + i * (size_t)ow, t);
}

/* diagnostic (not in include/mort_hip.h): one launch of math_kernel on `device`: function fn over n records, arguments as
 * mort_hip_debug_math_host; the tables are uploaded beside the records.  Writes n records to `out` and nothing after them. */
extern "C" int mort_hip_debug_math_device(int device, int fn, const uint32_t *in, size_t n, uint32_t *out, const void *noise, size_t noise_bytes,
                                          const void *images, size_t n_images, const void *texels, size_t texel_bytes) {
    if (fn < 0 || fn >= MATH_FUNCTIONS || !in || !out || n == 0 || n > ((size_t)1 << 28)) return MORT_ERR_INVALID;
    int st = math_check_tables(fn, in, n, noise, noise_bytes, (const DImage *)images, n_images, texels, texel_bytes);
    if (st != MORT_OK) return st;
    const size_t iw = MATH_SHAPES[fn].in, ow = MATH_SHAPES[fn].out;
    int caller_device = -1;
    if (hipGetDevice(&caller_device) != hipSuccess) caller_device = -1;
    if (hipSetDevice(device) != hipSuccess) return MORT_ERR_NO_DEVICE;
    uint32_t *d_in = nullptr, *d_out = nullptr;
    void *d_noise = nullptr, *d_images = nullptr, *d_texels = nullptr;
    const size_t image_bytes = n_images * sizeof(DImage);
    const bool want_noise = fn == MATH_FN_NOISE, want_image = fn == MATH_FN_IMAGE;
    if (hipMalloc((void **)&d_in, n * iw * 4) != hipSuccess || hipMalloc((void **)&d_out, n * ow * 4) != hipSuccess ||
        (want_noise && hipMalloc(&d_noise, noise_bytes) != hipSuccess) ||
        (want_image && (hipMalloc(&d_images, image_bytes) != hipSuccess || hipMalloc(&d_texels, texel_bytes ? texel_bytes : 1) != hipSuccess))) st = MORT_ERR_NOMEM;
    if (st == MORT_OK && (hipMemcpy(d_in, in, n * iw * 4, hipMemcpyHostToDevice) != hipSuccess ||
                          (want_noise && hipMemcpy(d_noise, noise, noise_bytes, hipMemcpyHostToDevice) != hipSuccess) ||
                          (want_image && (hipMemcpy(d_images, images, image_bytes, hipMemcpyHostToDevice) != hipSuccess ||
                                          (texel_bytes && hipMemcpy(d_texels, texels, texel_bytes, hipMemcpyHostToDevice) != hipSuccess))))) st = MORT_ERR_HIP;
    if (st == MORT_OK) {
        const size_t blocks = (n + 255) / 256;
        const MathTables t{(const float *)d_noise, (const DImage *)d_images, (const unsigned char *)d_texels};
        math_kernel<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256)>>>(fn, (int)iw, (int)ow, d_in, n, d_out, t);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(out, d_out, n * ow * 4, hipMemcpyDeviceToHost) != hipSuccess) st = MORT_ERR_HIP;
    }
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    if (d_noise) (void)hipFree(d_noise);
    if (d_images) (void)hipFree(d_images);
    if (d_texels) (void)hipFree(d_texels);
    if (caller_device >= 0 && caller_device != device) (void)hipSetDevice(caller_device); /* the caller's current device, as it was */
    return st;
}

/* ---- light sampling on a caller's records against a caller's world: dev_render.h's light_pdf_value and light_random over dev_trace.h's
 * wsphere_* / wquad_*, reading the world-order tables and the flattened lists of scene_compile.h.  Records are 32-bit words:
 *   fn 0 light_pdf_value: type, idx, origin[3], direction[3] -> the pdf;
 *   fn 1 light_random: the six XORWOW words (d, v0..v4), type, idx, origin[3] -> the direction, the six final words, the draw count
 *        (the math table's stream layout).
 * light_eval is the one body behind mort_hip_debug_light_host (hipcc's host compile over a world compiled as host_render.hip compiles it)
 * and light_kernel (the gfx950 compile over a context's uploaded scene); oracle/mort_oracle.c's mort_oracle_light_batch is the oracle's
 * pdf_value_dispatch / random_dispatch under the same numbers (tests/test_light_host.py, tests/test_gpu_light.py). ---- */
static const MathShape LIGHT_SHAPES[] = {/* 0 light_pdf_value */ {8, 1}, /* 1 light_random */ {11, 10}};
#define LIGHT_FUNCTIONS ((int)(sizeof LIGHT_SHAPES / sizeof LIGHT_SHAPES[0]))

static __host__ __device__ void light_eval(int fn, const DScene &sc, const uint32_t *in, uint32_t *out) {
    if (fn == 0) {
        math_pf(out, 0, light_pdf_value(sc, (int)in[0], (int)in[1], math_v(in, 2), math_v(in, 5)));
    } else {
        Rng s = math_rng(in);
        math_pv(out, 0, light_random(sc, (int)in[6], (int)in[7], math_v(in, 8), s));
        math_prng(out, 3, s);
    }
}

/* every record names a light object the render would accept: `check` is check_light or check_light_object on (type, idx).  A list's answer
 * is formed once (it walks the list), a primitive's per record */
template <typename Check>
static int light_check_records(size_t iw, size_t at, const uint32_t *in, size_t n, Check check) { /* (type, idx) at words at, at + 1 of iw */
    int list_status[MORT_NUM_HITTABLE_LIST];
    bool list_known[MORT_NUM_HITTABLE_LIST] = {};
    for (size_t i = 0; i < n; i++) {
        const int type = (int)in[i * iw + at], idx = (int)in[i * iw + at + 1];
        int st;
        if (type == MORT_OBJ_HITTABLE_LIST && idx >= 0 && idx < MORT_NUM_HITTABLE_LIST) {
            if (!list_known[idx]) { list_status[idx] = check(type, idx); list_known[idx] = true; }
            st = list_status[idx];
        } else st = check(type, idx);
        if (st != MORT_OK) return st;
    }
    return MORT_OK;
}

/* diagnostic (not in include/mort_hip.h; host only, no HIP call): the record shape of light function fn in 32-bit words; MORT_ERR_INVALID
 * past the last function */
extern "C" int mort_hip_debug_light_shape(int fn, int *in_words, int *out_words) {
    if (fn < 0 || fn >= LIGHT_FUNCTIONS || !in_words || !out_words) return MORT_ERR_INVALID;
    *in_words = LIGHT_SHAPES[fn].in; *out_words = LIGHT_SHAPES[fn].out;
    return MORT_OK;
}

/* diagnostic (not in include/mort_hip.h; host only, no HIP call): light function fn over n records against `w`, hipcc's host compile of
 * light_eval.  The world is compiled as mort_hip_render_host compiles it; a record whose (type, idx) check_light_object refuses as a camera's
 * light object (index out of range, empty or nested list) fails the whole call with that status, before anything is evaluated. */
extern "C" int mort_hip_debug_light_host(const mort_world *w, int fn, const uint32_t *in, size_t n, uint32_t *out) {
    if (!w || fn < 0 || fn >= LIGHT_FUNCTIONS || ((!in || !out) && n)) return MORT_ERR_INVALID;
    SceneBlob sb;
    int st = build_scene_blob(w, sb);
    if (st != MORT_OK) return st;
    const int n_lists = w->objs.num_hittable_list;
    st = light_check_records(LIGHT_SHAPES[fn].in, fn == 0 ? 0 : 6, in, n, [&](int type, int idx) { return check_light_object(sb.comp, n_lists, type, idx); });
    if (st != MORT_OK) return st;
    DScene sc;
    scene_view(sb, sb.bytes.data(), sc);
    const size_t iw = LIGHT_SHAPES[fn].in, ow = LIGHT_SHAPES[fn].out;
    unsigned nthreads = std::thread::hardware_concurrency();
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 16) nthreads = 16;
    if (n < 4096) nthreads = 1;
    auto work = [&](unsigned k) {
        for (size_t i = n * k / nthreads, end = n * (k + 1) / nthreads; i < end; i++) light_eval(fn, sc, in + i * iw, out + i * ow);
    };
    std::vector<std::thread> pool;
    for (unsigned k = 1; k < nthreads; k++) pool.emplace_back(work, k);
    work(0);
    for (std::thread &th : pool) th.join();
    return MORT_OK;
}

/* one lane per record, grid-stride; results leave as raw words */
static __global__ void __launch_bounds__(256) light_kernel(int fn, int iw, int ow, DScene sc, const uint32_t *in, size_t n, uint32_t *out) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) light_eval(fn, sc, in + i * (size_t)iw, out + i * (size_t)ow);
}

/* diagnostic (not in include/mort_hip.h): one launch of light_kernel over the scene of a context whose world has been uploaded: light
 * function fn over n records.  Every record is checked on the host first, by check_light against the context's copy of the uploaded
 * world's lists, so every index a lane forms lies inside the uploaded tables; a refused record fails the whole call before the launch.
 * Writes n records to `out` and nothing after them. */
extern "C" int mort_hip_debug_light_device(mort_ctx *c, int fn, const uint32_t *in, size_t n, uint32_t *out) {
    if (!c || fn < 0 || fn >= LIGHT_FUNCTIONS || !in || !out || n == 0 || n > ((size_t)1 << 28)) return MORT_ERR_INVALID;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    int st = light_check_records(LIGHT_SHAPES[fn].in, fn == 0 ? 0 : 6, in, n, [&](int type, int idx) { return check_light(c, type, idx); });
    if (st != MORT_OK) return st;
    const size_t iw = LIGHT_SHAPES[fn].in, ow = LIGHT_SHAPES[fn].out;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, quiesce(c));
    uint32_t *d_in = nullptr, *d_out = nullptr;
    if (hipMalloc((void **)&d_in, n * iw * 4) != hipSuccess || hipMalloc((void **)&d_out, n * ow * 4) != hipSuccess) st = MORT_ERR_NOMEM;
    if (st == MORT_OK && hipMemcpy(d_in, in, n * iw * 4, hipMemcpyHostToDevice) != hipSuccess) st = MORT_ERR_HIP;
    if (st == MORT_OK) {
        const size_t blocks = (n + 255) / 256;
        light_kernel<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, c->stream>>>(fn, (int)iw, (int)ow, c->sc, d_in, n, d_out);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(out, d_out, n * ow * 4, hipMemcpyDeviceToHost) != hipSuccess) st = MORT_ERR_HIP;
    }
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    return st;
}

/* ---- the shade step on a caller's records against a caller's world: one iteration of ray_color's loop body (camera.cuh:96-159) -- the
 * closest-hit search of a radiance query's segment (dev_radiance.h radiance_world_hit: [0.001, inf), the unified tree where the world has
 * one, else the item scan) and dev_shade.h's shade_hit on what it finds.  One record, in 32-bit words:
 *   in  (16): the six XORWOW words (d, v0..v4), ray origin[3], direction[3], time, ray_time0 (the time a Lambertian or isotropic scatter
 *             gives its ray), light_type, light_idx (the camera's light object; -1 = none);
 *   out (22): status (0 miss, 1 the path ends, 2 scatter, 3 scatter whose stack entry is the identity), k[3] = scattering_pdf x attenuation,
 *             rp = 1 / pdf, final_value[3], the ray afterwards (7; the scattered ray of a scatter, else the ray as given), the six final
 *             stream words, the draw count.  k and rp are 0 where nothing scatters, (1, 1, 1) and 1 for status 3; final_value is 0 for a
 *             miss (the background is the caller's) and for a scatter.
 * shade_eval is the one body behind mort_hip_debug_shade_host (hipcc's host compile over a world compiled as host_render.hip compiles it)
 * and shade_kernel (the gfx950 compile over a context's uploaded scene); oracle/mort_oracle.c's mort_oracle_shade_batch is the oracle's
 * loop body under the same layout (tests/test_shade_host.py, tests/test_gpu_shade.py). ---- */
#define SHADE_IN_WORDS 16
#define SHADE_OUT_WORDS 22

template <bool TREE>
static __host__ __device__ void shade_eval(const QueryArgs &q, const uint32_t *in, uint32_t *out, unsigned short *walk, int walk_stride) {
    Rng s = math_rng(in);
    Ray ray;
    ray.o = math_v(in, 6); ray.d = math_v(in, 9); ray.tm = math_f(in, 12);
    const float ray_time0 = math_f(in, 13);
    uint32_t status = 0;
    StackEntry e;
    e.kx = e.ky = e.kz = e.rp = 0.0f;
    V3 final_value = mk(0, 0, 0);
    Best best;
    if (radiance_world_hit<TREE>(q, ray, s, best, walk, walk_stride)) {
        const ShadeOut so = shade_hit(q.sc, (int)in[14], (int)in[15], ray, ray_time0, best, s);
        if (so.done) { status = 1; final_value = so.final_value; }
        else if (so.ident) { status = 3; e.kx = e.ky = e.kz = e.rp = 1.0f; }
        else { status = 2; e = so.e; }
    }
    out[0] = status;
    math_pf(out, 1, e.kx); math_pf(out, 2, e.ky); math_pf(out, 3, e.kz); math_pf(out, 4, e.rp);
    math_pv(out, 5, final_value);
    math_pv(out, 8, ray.o); math_pv(out, 11, ray.d); math_pf(out, 14, ray.tm);
    math_prng(out, 15, s);
}

/* diagnostic (not in include/mort_hip.h; host only, no HIP call): the record shape of shade function fn in 32-bit words (fn 0, the shade
 * step, is the only one); MORT_ERR_INVALID past the last function */
#define SHADE_FUNCTIONS 1
extern "C" int mort_hip_debug_shade_shape(int fn, int *in_words, int *out_words) {
    if (fn < 0 || fn >= SHADE_FUNCTIONS || !in_words || !out_words) return MORT_ERR_INVALID;
    *in_words = SHADE_IN_WORDS; *out_words = SHADE_OUT_WORDS;
    return MORT_OK;
}

/* diagnostic (not in include/mort_hip.h; host only, no HIP call): the shade step over n records against `w`, hipcc's host compile of
 * shade_eval.  The world is compiled as mort_hip_render_host compiles it; flags: MORT_HOST_TREE searches the unified tree where the world
 * has one.  A record whose light object check_light_object refuses fails the whole call with that status, before anything is evaluated. */
extern "C" int mort_hip_debug_shade_host(const mort_world *w, int fn, int flags, const uint32_t *in, size_t n, uint32_t *out) {
    if (!w || fn < 0 || fn >= SHADE_FUNCTIONS || ((!in || !out) && n)) return MORT_ERR_INVALID;
    SceneBlob sb;
    int st = build_scene_blob(w, sb);
    if (st != MORT_OK) return st;
    const int n_lists = w->objs.num_hittable_list;
    st = light_check_records(SHADE_IN_WORDS, 14, in, n, [&](int type, int idx) { return check_light_object(sb.comp, n_lists, type, idx); });
    if (st != MORT_OK) return st;
    const bool tree = (flags & MORT_HOST_TREE) && sb.comp.g_ok;
    QueryArgs q;
    query_args_host(sb, tree, q);
    unsigned nthreads = std::thread::hardware_concurrency();
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 16) nthreads = 16;
    if (n < 4096) nthreads = 1;
    auto work = [&](unsigned k) {
        unsigned short walk[MORT_OWN_STACK];
        for (size_t i = n * k / nthreads, end = n * (k + 1) / nthreads; i < end; i++) {
            if (tree) shade_eval<true>(q, in + i * SHADE_IN_WORDS, out + i * SHADE_OUT_WORDS, walk, 1);
            else shade_eval<false>(q, in + i * SHADE_IN_WORDS, out + i * SHADE_OUT_WORDS, walk, 1);
        }
    };
    std::vector<std::thread> pool;
    for (unsigned k = 1; k < nthreads; k++) pool.emplace_back(work, k);
    work(0);
    for (std::thread &th : pool) th.join();
    return MORT_OK;
}

/* one lane per record, grid-stride; the walk's pending children in LDS as query_radiance_kernel keeps them; results leave as raw words */
template <bool TREE>
static __global__ void __launch_bounds__(QUERY_BLOCK) shade_kernel(QueryArgs q, const uint32_t *in, size_t n, uint32_t *out) {
    __shared__ unsigned short walk_stack[TREE ? MORT_OWN_STACK * QUERY_BLOCK : 1];
    const size_t stride = (size_t)gridDim.x * QUERY_BLOCK;
    for (size_t i = (size_t)blockIdx.x * QUERY_BLOCK + threadIdx.x; i < n; i += stride)
        shade_eval<TREE>(q, in + i * SHADE_IN_WORDS, out + i * SHADE_OUT_WORDS, &walk_stack[TREE ? threadIdx.x : 0], QUERY_BLOCK);
}

/* diagnostic (not in include/mort_hip.h): one launch of shade_kernel over the scene of a context whose world has been uploaded, the
 * search a radiance query makes there (the unified tree where the world has one).  Every record's light object is checked on the host
 * first, by check_light against the context's copy of the uploaded world's lists; a refused record fails the whole call before the
 * launch.  Writes n records to `out` and nothing after them. */
extern "C" int mort_hip_debug_shade_device(mort_ctx *c, int fn, const uint32_t *in, size_t n, uint32_t *out) {
    if (!c || fn < 0 || fn >= SHADE_FUNCTIONS || !in || !out || n == 0 || n > ((size_t)1 << 26)) return MORT_ERR_INVALID;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    int st = light_check_records(SHADE_IN_WORDS, 14, in, n, [&](int type, int idx) { return check_light(c, type, idx); });
    if (st != MORT_OK) return st;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, quiesce(c));
    QueryArgs q;
    query_args_device(c, q);
    uint32_t *d_in = nullptr, *d_out = nullptr;
    if (hipMalloc((void **)&d_in, n * SHADE_IN_WORDS * 4) != hipSuccess || hipMalloc((void **)&d_out, n * SHADE_OUT_WORDS * 4) != hipSuccess) st = MORT_ERR_NOMEM;
    if (st == MORT_OK && hipMemcpy(d_in, in, n * SHADE_IN_WORDS * 4, hipMemcpyHostToDevice) != hipSuccess) st = MORT_ERR_HIP;
    if (st == MORT_OK) {
        const size_t blocks = (n + QUERY_BLOCK - 1) / QUERY_BLOCK;
        const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096)), block(QUERY_BLOCK);
        if (c->gen_ok) shade_kernel<true><<<grid, block, 0, c->stream>>>(q, d_in, n, d_out);
        else shade_kernel<false><<<grid, block, 0, c->stream>>>(q, d_in, n, d_out);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(out, d_out, n * SHADE_OUT_WORDS * 4, hipMemcpyDeviceToHost) != hipSuccess) st = MORT_ERR_HIP;
    }
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    return st;
}

/* ---- the two ends of Camera::render on a caller's records: dev_render.h's get_ray in both of its instantiations, and the pixel's finish.
 * Records are 32-bit words:
 *   fn 0 get_ray<RenderArgs> (the one-lane kernel, the wave mode's front, the host loop): in (30) the six XORWOW words (d, v0..v4), x, y,
 *        s_i, s_j, recip_sqrt_spp, defocus_angle, center, pixel00, du, dv, defocus_u, defocus_v; out (14) origin[3], direction[3], time, the
 *        six final words, the draw count;
 *   fn 1 get_ray<CamView>, the same records: on the device a record's CamView is written into the workgroup's LDS (256 x 80 B) by the
 *        NEIGHBOURING lane, and after a barrier get_ray reads the LDS copy, as mega_bvh.h and mega_gen.hip read theirs after theirs (the
 *        build checks camera_kernel's 20480 B of static LDS: scripts/kernel_resources.py);
 *   fn 2 pixel_finish and pixel_rgba: in (4) scale, sum[3]; out (4) the accumulator[3] and the uchar4, written as the pixel itself.
 * camera_eval is the one body behind mort_hip_debug_camera_host (hipcc's host compile) and camera_kernel (the gfx950 compile);
 * oracle/mort_oracle.c's mort_oracle_camera_batch is the oracle's get_ray and render_pixel's tail under the same numbers
 * (tests/test_camera_host.py, tests/test_gpu_camera.py). ---- */
static const MathShape CAMERA_SHAPES[] = {/* 0 get_ray<RenderArgs> */ {30, 14}, /* 1 get_ray<CamView> */ {30, 14}, /* 2 pixel finish */ {4, 4}};
#define CAMERA_FUNCTIONS ((int)(sizeof CAMERA_SHAPES / sizeof CAMERA_SHAPES[0]))
static_assert(sizeof(CamView) == 80, "CamView: 20 words");

DEV void camera_put_ray(uint32_t *out, const Ray &r, const Rng &s) {
    math_pv(out, 0, r.o); math_pv(out, 3, r.d); math_pf(out, 6, r.tm);
    math_prng(out, 7, s);
}

/* the CamView of a record, for fn 1 */
DEV void camera_view_fill(CamView &view, const uint32_t *in) {
    view.recip_sqrt_spp = math_f(in, 10); view.defocus_angle = math_f(in, 11);
    view.center = math_v(in, 12); view.pixel00 = math_v(in, 15); view.du = math_v(in, 18); view.dv = math_v(in, 21);
    view.defocus_u = math_v(in, 24); view.defocus_v = math_v(in, 27);
}

/* `view` (fn 1 only): the record's CamView, filled before the call (camera_view_fill): in LDS on the device */
static __host__ __device__ void camera_eval(int fn, const uint32_t *in, uint32_t *out, const CamView *view) {
    if (fn == 2) {
        const V3 c = pixel_finish(math_f(in, 0), math_v(in, 1));
        math_pv(out, 0, c);
        pixel_rgba(*reinterpret_cast<uchar4 *>(out + 3), c);
        return;
    }
    Rng s = math_rng(in);
    const int x = (int)in[6], y = (int)in[7], s_i = (int)in[8], s_j = (int)in[9];
    if (fn == 0) {
        RenderArgs a;
        a.recip_sqrt_spp = math_f(in, 10); a.defocus_angle = math_f(in, 11);
        a.center = math_v(in, 12); a.pixel00 = math_v(in, 15); a.du = math_v(in, 18); a.dv = math_v(in, 21);
        a.defocus_u = math_v(in, 24); a.defocus_v = math_v(in, 27);
        camera_put_ray(out, get_ray(a, x, y, s, s_i, s_j), s);
    } else {
        camera_put_ray(out, get_ray(*view, x, y, s, s_i, s_j), s);
    }
}

/* diagnostic (not in include/mort_hip.h; host only, no HIP call): the record shape of camera function fn in 32-bit words; MORT_ERR_INVALID
 * past the last function */
extern "C" int mort_hip_debug_camera_shape(int fn, int *in_words, int *out_words) {
    if (fn < 0 || fn >= CAMERA_FUNCTIONS || !in_words || !out_words) return MORT_ERR_INVALID;
    *in_words = CAMERA_SHAPES[fn].in; *out_words = CAMERA_SHAPES[fn].out;
    return MORT_OK;
}

/* diagnostic (not in include/mort_hip.h; host only, no HIP call): camera function fn over n records, hipcc's host compile of camera_eval */
extern "C" int mort_hip_debug_camera_host(int fn, const uint32_t *in, size_t n, uint32_t *out) {
    if (fn < 0 || fn >= CAMERA_FUNCTIONS || ((!in || !out) && n)) return MORT_ERR_INVALID;
    const size_t iw = CAMERA_SHAPES[fn].in, ow = CAMERA_SHAPES[fn].out;
    unsigned nthreads = std::thread::hardware_concurrency();
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 16) nthreads = 16;
    if (n < 4096) nthreads = 1;
    auto work = [&](unsigned k) {
        CamView view;
        for (size_t i = n * k / nthreads, end = n * (k + 1) / nthreads; i < end; i++) {
            if (fn == 1) camera_view_fill(view, in + i * iw);
            camera_eval(fn, in + i * iw, out + i * ow, &view);
        }
    };
    std::vector<std::thread> pool;
    for (unsigned k = 1; k < nthreads; k++) pool.emplace_back(work, k);
    work(0);
    for (std::thread &th : pool) th.join();
    return MORT_OK;
}

/* one lane per record, grid-stride with the same trip count in every lane, so that the barriers are reached by all.  fn 1: lane t writes the
 * CamView of its neighbour's record (lane t ^ 1 of the same workgroup: record i ^ 1) into slot t ^ 1 of the workgroup's LDS; after the
 * barrier every lane hands get_ray the slot of its own record, which another lane wrote; the second barrier keeps the next trip's writes
 * behind this trip's reads.  Results leave as raw words */
static __global__ void __launch_bounds__(256) camera_kernel(int fn, int iw, int ow, const uint32_t *in, size_t n, uint32_t *out) {
    __shared__ CamView s_view[256];
    const size_t stride = (size_t)gridDim.x * 256;
    const size_t trips = (n + stride - 1) / stride;
    for (size_t k = 0; k < trips; k++) {
        const size_t i = k * stride + (size_t)blockIdx.x * 256 + threadIdx.x, j = i ^ 1;
        if (fn == 1 && j < n) camera_view_fill(s_view[threadIdx.x ^ 1], in + j * (size_t)iw);
        __syncthreads();
        if (i < n) camera_eval(fn, in + i * (size_t)iw, out + i * (size_t)ow, &s_view[threadIdx.x]);
        __syncthreads();
    }
}

/* diagnostic (not in include/mort_hip.h): one launch of camera_kernel on `device`: camera function fn over n records.  Writes n records
 * to `out` and nothing after them. */
extern "C" int mort_hip_debug_camera_device(int device, int fn, const uint32_t *in, size_t n, uint32_t *out) {
    if (fn < 0 || fn >= CAMERA_FUNCTIONS || !in || !out || n == 0 || n > ((size_t)1 << 26)) return MORT_ERR_INVALID;
    const size_t iw = CAMERA_SHAPES[fn].in, ow = CAMERA_SHAPES[fn].out;
    int caller_device = -1;
    if (hipGetDevice(&caller_device) != hipSuccess) caller_device = -1;
    if (hipSetDevice(device) != hipSuccess) return MORT_ERR_NO_DEVICE;
    int st = MORT_OK;
    uint32_t *d_in = nullptr, *d_out = nullptr;
    if (hipMalloc((void **)&d_in, n * iw * 4) != hipSuccess || hipMalloc((void **)&d_out, n * ow * 4) != hipSuccess) st = MORT_ERR_NOMEM;
    if (st == MORT_OK && hipMemcpy(d_in, in, n * iw * 4, hipMemcpyHostToDevice) != hipSuccess) st = MORT_ERR_HIP;
    if (st == MORT_OK) {
        const size_t blocks = (n + 255) / 256;
        camera_kernel<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256)>>>(fn, (int)iw, (int)ow, d_in, n, d_out);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(out, d_out, n * ow * 4, hipMemcpyDeviceToHost) != hipSuccess) st = MORT_ERR_HIP;
    }
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    if (caller_device >= 0 && caller_device != device) (void)hipSetDevice(caller_device); /* the caller's current device, as it was */
    return st;
}

/* the device half of dev_math.h's sentence on random_float: random_float_of(curand_uniform_of(x)), dev_math.h's own two steps, against the
 * reference's (float)(1.0 - (double)u), for ALL 2^32 generator outputs x (every lane takes every 2^20-th) */
static __global__ void __launch_bounds__(256) random_float_all_kernel(unsigned long long *out) {
    const uint32_t first = blockIdx.x * 256u + threadIdx.x; /* 4096 blocks: 2^20 lanes, 2^12 outputs each */
    uint32_t differ = 0, lowest = 0xffffffffu;
    for (uint32_t k = 0; k < 4096u; k++) {
        const uint32_t x = first + (k << 20);
        const float u = curand_uniform_of(x);
        double wide = (double)u;
        __asm__ volatile("" : "+v"(wide)); /* opaque: the compiler would otherwise narrow the fp64 subtraction to the fp32 one and compare nothing */
        const float got = random_float_of(u), want = (float)(1.0 - wide);
        if (__float_as_uint(got) != __float_as_uint(want)) { differ++; lowest = x < lowest ? x : lowest; }
    }
    atomicAdd(&out[2], 4096ull);
    if (differ) { atomicAdd(&out[0], (unsigned long long)differ); atomicMin(&out[1], (unsigned long long)lowest); }
}

/* diagnostic (not in include/mort_hip.h): on `device`, out[0] = how many of the 2^32 generator outputs give a random_float that differs
 * from the reference's form, out[1] = the lowest such output (2^32 - 1 if none), out[2] = outputs visited */
extern "C" int mort_hip_debug_random_float_device(int device, unsigned long long *out) {
    if (!out) return MORT_ERR_INVALID;
    int caller_device = -1;
    if (hipGetDevice(&caller_device) != hipSuccess) caller_device = -1;
    if (hipSetDevice(device) != hipSuccess) return MORT_ERR_NO_DEVICE;
    unsigned long long *d_out = nullptr;
    const unsigned long long init[3] = {0ull, 0xffffffffull, 0ull};
    int st = MORT_OK;
    if (hipMalloc((void **)&d_out, sizeof init) != hipSuccess) st = MORT_ERR_NOMEM;
    if (st == MORT_OK && hipMemcpy(d_out, init, sizeof init, hipMemcpyHostToDevice) != hipSuccess) st = MORT_ERR_HIP;
    if (st == MORT_OK) {
        random_float_all_kernel<<<dim3(4096), dim3(256)>>>(d_out);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(out, d_out, sizeof init, hipMemcpyDeviceToHost) != hipSuccess) st = MORT_ERR_HIP;
    }
    if (d_out) (void)hipFree(d_out);
    if (caller_device >= 0 && caller_device != device) (void)hipSetDevice(caller_device); /* the caller's current device, as it was */
    return st;
}

/* ---- the tile scheduler read back (include/mort_hip.h; DESIGN.md 5 "Reading the scheduler back") ---- */

/* the last render launch's tile order as the host recorded it (mort_ctx::TileLaunch) and as the device holds it: the keys and the
 * order stay in their buffers until the next ordered launch sorts again, the costs are what the frame's pixel_write left */
extern "C" int mort_hip_debug_tile_state(mort_ctx *c, mort_tile_state *out, uint32_t *keys, uint32_t *order, uint32_t *cost, size_t cap) {
    if (!c || !out) return MORT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, quiesce(c));
    const mort_ctx::TileLaunch &t = c->tile_launch;
    std::memset(out, 0, sizeof *out);
    out->ordered = t.ordered; out->probed = t.probed;
    out->tiles = t.tiles; out->tiles_x = t.tiles_x; out->grid = t.grid; out->block = t.block;
    out->key_sum = t.key_sum; out->spread_shift = t.spread_shift; out->gen_tiles = t.gen_tiles;
    for (int k = 0; k < 4; k++) out->heavy[k] = t.heavy[k];
    out->has_head = t.has_head;
    if (t.has_head && c->d_prio_count) {
        HIPCHK(c, hipMemcpy(&out->head, c->d_prio_count, sizeof out->head, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(out->frame_total, c->d_prio_count + 4 + 2 * MORT_TILE_COUNTERS, sizeof out->frame_total, hipMemcpyDeviceToHost));
    }
    if (!t.ordered || t.tiles <= 0 || cap < (size_t)t.tiles || c->tile_cap < (size_t)t.tiles) return MORT_OK;
    const size_t bytes = (size_t)t.tiles * sizeof(uint32_t);
    if (keys) HIPCHK(c, hipMemcpy(keys, c->d_tile_keys, bytes, hipMemcpyDeviceToHost));
    if (order) HIPCHK(c, hipMemcpy(order, c->d_tile_order, bytes, hipMemcpyDeviceToHost));
    if (cost) HIPCHK(c, hipMemcpy(cost, c->d_tile_cost, bytes, hipMemcpyDeviceToHost));
    return MORT_OK;
}

/* device buffers of a helper-kernel driver: freed when it returns */
namespace {
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    bool alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16) == hipSuccess; }
    bool up(const void *src, size_t bytes) { return hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) == hipSuccess; }
    bool down(void *dst, size_t bytes) const { return hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost) == hipSuccess; }
};
struct OnDevice { /* the caller's current device, as it was */
    int caller = -1, device;
    bool ok;
    explicit OnDevice(int d) : device(d) { if (hipGetDevice(&caller) != hipSuccess) caller = -1; ok = hipSetDevice(d) == hipSuccess; }
    ~OnDevice() { if (caller >= 0 && caller != device) (void)hipSetDevice(caller); }
};
}

/* mort_tile_sort_desc (tile_sort.hip) as prepare_tile_order calls it, on a caller's costs */
extern "C" int mort_hip_debug_tile_sort(int device, const uint32_t *cost, size_t n, uint32_t *keys_out, uint32_t *order_out) {
    if (!cost || !keys_out || !order_out || n < 1 || n > ((size_t)1 << 24)) return MORT_ERR_INVALID;
    OnDevice dev(device);
    if (!dev.ok) return MORT_ERR_NO_DEVICE;
    DevBuf d_cost, d_keys, d_iota, d_order, d_tmp;
    const size_t bytes = n * sizeof(uint32_t), tmp_bytes = mort_tile_sort_temp_bytes((int)n);
    if (!d_cost.alloc(bytes) || !d_keys.alloc(bytes) || !d_iota.alloc(bytes) || !d_order.alloc(bytes) || !d_tmp.alloc(tmp_bytes)) return MORT_ERR_NOMEM;
    if (!d_cost.up(cost, bytes)) return MORT_ERR_HIP;
    if (mort_tile_sort_desc((const unsigned *)d_cost.p, (unsigned *)d_keys.p, (unsigned *)d_iota.p, (unsigned *)d_order.p, d_tmp.p, tmp_bytes, (int)n, nullptr) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess || !d_keys.down(keys_out, bytes) || !d_order.down(order_out, bytes)) return MORT_ERR_HIP;
    return MORT_OK;
}

/* mort_tile_heavy_count (tile_sort.hip) as prepare_tile_order calls it, on a caller's sorted keys and saved counters */
extern "C" int mort_hip_debug_heavy_count(int device, const uint32_t *keys, size_t n, uint32_t percent, uint32_t max_r, const uint64_t *counters,
                                          uint64_t lanes, uint32_t *head_out) {
    if (!keys || !head_out || n < 1 || n > ((size_t)1 << 24)) return MORT_ERR_INVALID;
    OnDevice dev(device);
    if (!dev.ok) return MORT_ERR_NO_DEVICE;
    DevBuf d_keys, d_cnt, d_out;
    const size_t bytes = n * sizeof(uint32_t), cnt_bytes = MORT_TILE_COUNTERS * sizeof(uint64_t);
    const uint32_t unwritten = 0xffffffffu; /* the kernel always writes the word: this value never comes back */
    if (!d_keys.alloc(bytes) || !d_out.alloc(sizeof(uint32_t)) || (counters && !d_cnt.alloc(cnt_bytes))) return MORT_ERR_NOMEM;
    if (!d_keys.up(keys, bytes) || !d_out.up(&unwritten, sizeof unwritten) || (counters && !d_cnt.up(counters, cnt_bytes))) return MORT_ERR_HIP;
    if (mort_tile_heavy_count((const unsigned *)d_keys.p, (int)n, percent, max_r, (const unsigned long long *)d_cnt.p, (unsigned long long)lanes, (unsigned *)d_out.p, nullptr) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess || !d_out.down(head_out, sizeof(uint32_t))) return MORT_ERR_HIP;
    return MORT_OK;
}
