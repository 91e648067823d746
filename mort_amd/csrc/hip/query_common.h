/*
 * query_common.h -- host scaffolding that the ray queries (query.hip), the radiance queries (radiance.hip) and the cached radiance
 * queries (cached.hip, cached_direct.hip) share: the one workgroup shape and its limits, the alignment the _device forms ask for, and
 * the launch arguments over the context's scene.  The per-ray bodies are in dev_query.h, dev_radiance.h, dev_cached.h and
 * dev_cached_direct.h.
 */
#ifndef MORT_QUERY_COMMON_H
#define MORT_QUERY_COMMON_H

#include <cstring>

#include "dev_query.h"
#include "scene_blob.h"
#include "mort_ctx.h"

constexpr int QUERY_BLOCK = 256;

constexpr size_t kHostChunk = 1024;                                  /* rays a host thread takes at a time */
constexpr size_t kMaxRays = (size_t)0x7fffffff * (size_t)QUERY_BLOCK; /* a 1-D grid of 256-thread groups */

static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

/* the launch arguments over the context's scene in HBM; the unified tree where the world has one */
static inline void query_args_device(const mort_ctx *c, QueryArgs &a) {
    std::memset(&a, 0, sizeof a);
    a.sc = c->sc;
    if (!c->gen_ok) return;
    const unsigned char *g = (const unsigned char *)c->d_gen;
    a.gw.nodes = (const DNodeQ *)(g + c->gen.o_nodes); a.gw.entries = (const uint32_t *)(g + c->gen.o_entries);
    a.gw.chains = (const int *)(g + c->gen.o_chains); a.gw.ranks = c->gen.ranks; a.gw.n_spheres = c->gen.n_spheres;
    a.gw.n_chains = c->gen.n_chains; a.gw.root = c->gen.root; a.gw.first_medium = c->gen.first_medium;
    a.gw.gx = c->gen.gx; a.gw.gy = c->gen.gy; a.gw.gz = c->gen.gz; a.gw.gR = c->gen.gR; a.gw.mnear = c->gen.mnear; a.gw.kmin = c->gen.kmin;
    for (int k = 0; k < 3; k++) { a.lo[k] = c->gen_lo[k]; a.hi[k] = c->gen_hi[k]; }
    a.reach = c->gen_reach;
}

/* the same over a compiled world in host memory (the _host forms); tree: walk its unified tree */
static inline void query_args_host(const SceneBlob &sb, bool tree, QueryArgs &a) {
    std::memset(&a, 0, sizeof a);
    scene_view(sb, sb.bytes.data(), a.sc);
    if (!tree) return;
    const mortc::Compiled &o = sb.comp;
    a.gw = gen_walk_of(o);
    for (int k = 0; k < 3; k++) { a.lo[k] = o.g_lo[k]; a.hi[k] = o.g_hi[k]; }
    a.reach = o.g_reach;
}

#endif
