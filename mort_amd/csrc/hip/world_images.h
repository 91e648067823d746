/*
 * world_images.h -- what the host decides from a compiled world before anything reaches the GPU: which kernels serve it, the
 * LDS images they read and the LDS budget of their launches.  Host only: no HIP runtime call and no runtime header of its
 * own, so mort_hip_upload_world (context.hip), the launches (mort_hip.hip) and the host diagnostics (debug.hip) take the
 * same decisions from the same code.
 */
#ifndef MORT_WORLD_IMAGES_H
#define MORT_WORLD_IMAGES_H

#include <cstring>
#include <vector>

#include "scene_blob.h"
#include "mega_gen.h" /* GenArgs, MORT_BVH_TSTACK_SPARE */

/* the LDS kernels handle: one BVH over spheres as the whole world */
static inline bool one_sphere_bvh(const mortc::Compiled &o) { return o.items.size() == 1 && o.items[0].kind == ITEM_BVH && o.quads.empty(); }

/* The two LDS images of such a world: the BVH megakernel's (four-wide nodes, leaf records with their spheres by value, every small
 * table) and the wavefront traversal kernel's (binary nodes, leaf nodes, spheres), with the offsets of their parts.  fits: both
 * within MORT_BVH_IMAGE_MAX, the condition of mega_bvh_kernel and wave_bvh.h. */
#define MORT_BVH_IMAGE_MAX (72 * 1024)
struct BvhOffsets { /* f_: into the megakernel's image (FastArgs.off_*), t_: into the traversal kernel's (WfArgs.t_*) */
    uint32_t f_nodes4, f_leafrecs, f_lambert, f_metal, f_diel, f_dlight, f_iso, f_solid, f_checker, t_nodes2, t_leaves, t_spheres;
};
struct BvhImages {
    std::vector<unsigned char> fb, tb;
    BvhOffsets off;
    bool fits;
};
static inline void build_bvh_images(const mortc::Compiled &o, BvhImages &im) {
    std::vector<unsigned char> &fb = im.fb, &tb = im.tb;
    BvhOffsets &f = im.off;
    f.f_nodes4 = (uint32_t)place(fb, o.own_nodes4); f.f_leafrecs = (uint32_t)place(fb, o.own_leafrecs);
    f.f_lambert = (uint32_t)place(fb, o.lambert); f.f_metal = (uint32_t)place(fb, o.metal); f.f_diel = (uint32_t)place(fb, o.dielectric);
    f.f_dlight = (uint32_t)place(fb, o.dlight); f.f_iso = (uint32_t)place(fb, o.isotropic);
    f.f_solid = (uint32_t)place(fb, o.solid); f.f_checker = (uint32_t)place(fb, o.checker);
    fb.resize((fb.size() + 15) & ~(size_t)15, 0);
    f.t_nodes2 = (uint32_t)place(tb, o.own_nodes); f.t_leaves = (uint32_t)place(tb, o.own_leaves); f.t_spheres = (uint32_t)place(tb, o.spheres);
    tb.resize((tb.size() + 15) & ~(size_t)15, 0);
    im.fits = fb.size() <= MORT_BVH_IMAGE_MAX && tb.size() <= MORT_BVH_IMAGE_MAX;
}

/* 1024-thread groups of mega_bvh_kernel: image + traversal stacks + one bounce-stack level per lane must fit one CU's LDS */
static inline bool bvh_wide_block_fits(uint32_t image_bytes, int own4_stack) {
    return (size_t)((image_bytes + 15u) & ~15u) + ((size_t)own4_stack + MORT_BVH_TSTACK_SPARE) * 1024u * 2u + 2048u + 1024u * 16u <= 160u * 1024u;
}

/* The LDS image of a world with a unified tree (o.g_ok): the tree, every small table and, when image + primitives stay within
 * MORT_GEN_PRIMS_LDS_MAX, the primitives; behind the LDS part the scan ranks, which stay in HBM.  g: the table offsets and the tree's
 * constants as the kernels take them (g.ranks is left null: it points into the device copy).  fits: the LDS part is within
 * MORT_GEN_IMAGE_MAX, the condition of mega_gen_kernel and wave_gen.hip. */
#define MORT_GEN_PRIMS_LDS_MAX (48 * 1024)
#ifndef MORT_GEN_IMAGE_MAX
#define MORT_GEN_IMAGE_MAX (124 * 1024) /* + traversal stacks of 768 threads (24 KB) + the launch arguments: one workgroup per CU */
#endif
struct GenImage {
    std::vector<unsigned char> gb;
    GenArgs g;
    size_t table_bytes, prim_bytes, lds_part, o_ranks; /* the image before the primitives, the primitives, the whole LDS part */
    bool fits;
};
static inline void build_gen_image(const mortc::Compiled &o, GenImage &gi) {
    std::vector<unsigned char> &gb = gi.gb;
    GenArgs &g = gi.g;
    std::memset(&g, 0, sizeof g);
    g.o_nodes = (uint32_t)place(gb, o.g_nodes); g.o_leaves = g.o_nodes; g.o_entries = (uint32_t)place(gb, o.g_entries);
    g.o_chains = (uint32_t)place(gb, o.g_chains); g.o_xforms = (uint32_t)place(gb, o.xforms);
    g.o_items = (uint32_t)place(gb, o.items); g.o_subitems = (uint32_t)place(gb, o.subitems); g.o_media = (uint32_t)place(gb, o.media);
    g.o_lambert = (uint32_t)place(gb, o.lambert); g.o_metal = (uint32_t)place(gb, o.metal); g.o_diel = (uint32_t)place(gb, o.dielectric);
    g.o_dlight = (uint32_t)place(gb, o.dlight); g.o_iso = (uint32_t)place(gb, o.isotropic);
    g.o_solid = (uint32_t)place(gb, o.solid); g.o_checker = (uint32_t)place(gb, o.checker); g.o_image = (uint32_t)place(gb, o.image);
    g.o_lfirst = (uint32_t)place(gb, std::vector<int>(o.list_first, o.list_first + MORT_NUM_HITTABLE_LIST));
    g.o_lcount = (uint32_t)place(gb, std::vector<int>(o.list_count, o.list_count + MORT_NUM_HITTABLE_LIST));
    gi.table_bytes = gb.size();
    gi.prim_bytes = o.spheres.size() * sizeof(DSphere) + o.quads.size() * sizeof(DQuad) + o.wspheres.size() * sizeof(DSphere) +
                    o.wquads.size() * sizeof(DQuad) + (o.list_types.size() + o.list_idxs.size()) * sizeof(int) + 6 * 32;
    if (gi.table_bytes + gi.prim_bytes <= MORT_GEN_PRIMS_LDS_MAX) {
        g.prims_in_lds = 1;
        g.o_spheres = (uint32_t)place(gb, o.spheres); g.o_quads = (uint32_t)place(gb, o.quads);
        g.o_wspheres = (uint32_t)place(gb, o.wspheres); g.o_wquads = (uint32_t)place(gb, o.wquads);
        g.o_ltypes = (uint32_t)place(gb, o.list_types); g.o_lidxs = (uint32_t)place(gb, o.list_idxs);
    }
    gb.resize((gb.size() + 15) & ~(size_t)15, 0);
    gi.lds_part = gb.size();
    gi.o_ranks = place(gb, o.g_ranks); /* HBM only: read when two hits have equal t */
    g.n_spheres = (int)o.spheres.size();
    g.root = o.g_root; g.first_medium = o.g_first_medium; g.n_chains = (int)(o.g_chains.size() / 2);
    g.gx = o.g_c[0]; g.gy = o.g_c[1]; g.gz = o.g_c[2]; g.gR = o.g_R; g.mnear = o.g_mnear; g.kmin = o.g_kmin;
    gi.fits = gi.lds_part <= MORT_GEN_IMAGE_MAX;
}

/* the bounce-stack levels (at most 12) that fit in LDS beside an image of hot_bytes and the traversal stacks, in FB-thread groups, with
 * as many groups per CU as keep 12 waves per CU (fewer when their LDS does not fit 160 KB, or leaves fewer than min_levels levels:
 * mega_bvh_kernel's ring needs one); -1: the image and stacks alone, with min_levels levels, do not fit */
static inline int state_lds_levels(uint32_t hot_bytes, int FB, uint32_t tstack_levels, uint32_t static_lds, int min_levels, uint32_t &tstack_off, uint32_t &stack_off) {
    tstack_off = (hot_bytes + 15u) & ~15u;
    stack_off = tstack_off + tstack_levels * (uint32_t)FB * 2u;
    int groups_per_cu = FB >= 768 ? 1 : 768 / FB;
    while (groups_per_cu > 1 && (long long)(stack_off + static_lds + (uint32_t)min_levels * (uint32_t)FB * 16u) * groups_per_cu > 160ll * 1024) groups_per_cu--;
    const long long room = (160ll * 1024 - (long long)static_lds * groups_per_cu) / groups_per_cu - (long long)stack_off;
    if (room < 0) return -1;
    const int dl = (int)(room / ((long long)FB * 16));
    if (dl < min_levels) return -1;
    return dl > 12 ? 12 : dl;
}

#endif
