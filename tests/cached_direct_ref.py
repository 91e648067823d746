"""The reference side of the direct-light cached-query tests (tests/test_cached_direct_host.py, tests/test_gpu_cached_direct.py;
DESIGN.md 4.22), made from the oracle and the numpy restatements alone, never the library.

walk() is cached_ref.walk with the new terminal.  Where a path ends in the volume and the call names a light object and the bounce
limit leaves a segment, the direction and its pdf come from O.light_batch (fn 1 on the path's stream, fn 0), the shadow segment's
search from O.world_hit_batch on a COPY of the stream, and -- for a segment that ends on a hit whose tag is the diffuse light -- the
emission from O.shade_batch on that same ray and the ORIGINAL stream, which must answer "ended with a colour".  The scattering pdf,
the product, the quotient and the sum are float32 numpy in the contract's order.  The worlds, grids, masks and maps are
cached_ref's, the coefficients taken as they are: the reference does not care whether they are indirect-only.  One more world,
"light:bvh_list", is tests/light_cases.py's list of two sphere lights over a reference BVH, so that the kernel without the unified
tree meets a light; scene 1 has no light object and shows identity (i).  reference() caches one answer per case per process, and
nothing may change it."""
import functools

import numpy as np

from mort_amd import hip, host, structs as S
from tests import cached_ref as CR
from tests import depth_ref as D
from tests import light_cases as LC
from tests import math_restate as M
from tests import oracle_lib as O
from tests import query_rays as Q
from tests import radiance_ref as R
from tests import volume_ref as V

F = np.float32
INV_PI = CR.INV_PI
BVH_LIGHT_WORLD = "light:bvh_list"
WORLDS = CR.WORLDS + (BVH_LIGHT_WORLD,)
TREE_WORLDS = ("scene6", "flat:lit_by_quad_with_media")  # worlds with a unified tree: the TREE kernel on the GPU
CASES, DEPTHS, MASKS = CR.CASES, CR.DEPTHS, CR.MASKS


def _bvh_light_world():
    w, cam = LC.light_world("bvh_list")
    cam = R.copy_camera(cam)  # light_world's camera is shared: the copy takes the width of the other worlds' query rays
    cam.image_width = 48
    host.lib().mort_camera_initialize(cam)
    return w, cam


def _build_bvh_light_world():
    """Q.build's ray sets and oracle answers for the new world, under its name: the maker stands in Q.WORLDS only while Q.build
    runs -- Q.build keeps its answer per name from then on -- so the tests that walk over Q.WORLDS see the worlds they always saw"""
    assert BVH_LIGHT_WORLD not in Q.WORLDS
    Q.WORLDS[BVH_LIGHT_WORLD] = _bvh_light_world
    try:
        Q.build(BVH_LIGHT_WORLD)
    finally:
        del Q.WORLDS[BVH_LIGHT_WORLD]


_build_bvh_light_world()


def walk(world, rp, cache_depth, g, records, depth, vis, rays, streams):
    """(rgb (n, 3), ends uint32 (n,), lit uint32 (n,), census dict); streams (O.STATE_DTYPE, n) are advanced in place.
    rp: RADIANCE_PARAMS; depth / vis None: the plain sampler"""
    rays = np.asarray(rays, dtype=F).reshape(-1, 8)
    n = len(rays)
    assert streams.dtype == O.STATE_DTYPE and streams.shape == (n,)
    tex_type, tex_idx = CR._lambert_textures(world)
    background = np.array(list(rp.background), dtype=F)
    light = np.array([rp.light_obj_type, rp.light_obj_idx], dtype=np.int32).view(np.uint32)
    has_light = rp.light_obj_type != -1
    rgb = np.zeros((n, 3), dtype=F)
    ends = np.zeros(n, dtype=np.uint32)
    lit = np.zeros(n, dtype=np.uint32)
    cen = dict(paths=0, ended=np.zeros(n, dtype=np.int64), lit=np.zeros(n, dtype=np.int64), segments=0, fell_through=0, rule_a=0,
               pdf_not_positive=0, shadow_segments=0, shadow_on_medium=0, shadow_missed=0, shadow_blocked=0)
    medium_mats = Q.medium_materials(world)
    zero = F(0.0)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for _ in range(rp.samples):
            cur = np.ascontiguousarray(rays[:, :7]).copy()
            final = np.zeros((n, 3), dtype=F)
            levels = []  # per level: (path indices, k (m, 3), rp (m,), ident (m,))
            active = np.arange(n)
            it = 0
            while active.size:
                if it >= rp.bounce_limit:
                    final[active] = zero
                    break
                cen["segments"] += active.size
                probe = np.ascontiguousarray(streams[active]).copy()
                rec, hit = O.world_hit_batch(world, cur[active], Q.T_MIN, Q.INF, states=probe)
                take = np.zeros(active.size, dtype=bool)
                cand = hit & (rec["mat_type"] == S.MAT_LAMBERTIAN) if it >= cache_depth else take
                if cand.any():
                    c = np.flatnonzero(cand)
                    r = rec[c]
                    albedo = O.texture_value_batch(world, tex_type[r["mat_idx"]], tex_idx[r["mat_idx"]], r["u"], r["v"], r["p"])
                    if depth is None:
                        E = V.sample(g, records, r["p"], r["normal"])
                    else:
                        E = D.sample_visible(g, records, depth, vis[0], vis[1], r["p"], r["normal"])
                    ok = E[:, 3] > 0
                    take[c[ok]] = True
                    who = active[c[ok]]
                    base = ((albedo[ok] * E[ok, :3]).astype(F) * INV_PI).astype(F)
                    streams[who] = probe[c[ok]]
                    ends[who] += 1
                    cen["ended"][who] += 1
                    cen["fell_through"] += int((~ok).sum())
                    if not has_light or it + 1 >= rp.bounce_limit:  # rule (a): the cached query's value, nothing drawn
                        final[who] = base
                        cen["rule_a"] += who.size
                    elif who.size:
                        final[who] = _direct(world, light, who, base, albedo[ok], np.ascontiguousarray(r["p"][ok]), np.ascontiguousarray(r["normal"][ok]),
                                             rays, streams, lit, cen, medium_mats)
                go = np.flatnonzero(~take)
                who = active[go]
                inp = np.zeros((who.size, 16), dtype=np.uint32)
                inp[:, 0] = streams["d"][who]
                inp[:, 1:6] = streams["v"][who]
                inp[:, 6:13] = cur[who].view(np.uint32)
                inp[:, 13] = rays[who, 6].view(np.uint32)
                inp[:, 14:16] = light
                out, _ = O.shade_batch(world, inp)
                status = out[:, 0]
                assert ((status != 0) == hit[go]).all(), "the shade step's search and the hit batch disagree"
                streams["d"][who] = out[:, 15]
                streams["v"][who] = out[:, 16:21]
                final[who[status == 0]] = background
                final[who[status == 1]] = out[status == 1, 5:8].view(F)
                on = status >= 2
                nxt = who[on]
                cur[nxt] = out[on, 8:15].view(F)
                levels.append((nxt, out[on, 1:4].view(F), out[on, 4].view(F), status[on] == 3))
                active = nxt
                it += 1
            for who, k, rpdf, ident in reversed(levels):
                f = final[who]
                t = (k * f).astype(F)
                f = np.where(ident[:, None], zero + f, zero + (rpdf[:, None] * t).astype(F)).astype(F)
                final[who] = f
            rgb = (rgb + final).astype(F)
            cen["paths"] += n
    return rgb, ends, lit, cen


def _direct(world, light, who, base, albedo, p, normal, rays, streams, lit, cen, medium_mats):
    """rules (b)-(d) for the paths `who` that have just ended at (p, normal) with `base`: their final values; their streams and lit
    counts are advanced in place"""
    m = who.size
    # (b) the light sample from the path's stream, its pdf, the scattering pdf
    lr = np.zeros((m, 11), dtype=np.uint32)
    lr[:, 0] = streams["d"][who]
    lr[:, 1:6] = streams["v"][who]
    lr[:, 6:8] = light
    lr[:, 8:11] = p.view(np.uint32)
    out = O.light_batch(world, 1, lr)
    direction = np.ascontiguousarray(out[:, 0:3]).view(F)
    streams["d"][who] = out[:, 3]
    streams["v"][who] = out[:, 4:9]
    pr = np.zeros((m, 8), dtype=np.uint32)
    pr[:, 0:2] = light
    pr[:, 2:5] = p.view(np.uint32)
    pr[:, 5:8] = direction.view(np.uint32)
    pdf = np.ascontiguousarray(O.light_batch(world, 0, pr)[:, 0]).view(F)
    cosine = M.vdot(normal, M.vunit(direction)).astype(F)
    spdf = np.where(cosine < 0, F(0), (cosine * INV_PI).astype(F)).astype(F)
    cen["pdf_not_positive"] += int((~(pdf > 0)).sum())
    # (c) the shadow segment: the search on a copy of the stream; the emission of a light from the shade step on the original
    seg = np.ascontiguousarray(np.concatenate([p, direction, rays[who, 6:7]], axis=1), dtype=F)
    copy = np.ascontiguousarray(streams[who]).copy()
    rec, hit = O.world_hit_batch(world, seg, Q.T_MIN, Q.INF, states=copy)
    Le = np.zeros((m, 3), dtype=F)
    on_light = hit & (rec["mat_type"] == S.MAT_DIFFUSE_LIGHT)
    if on_light.any():
        k = np.flatnonzero(on_light)
        inp = np.zeros((k.size, 16), dtype=np.uint32)
        inp[:, 0] = streams["d"][who[k]]
        inp[:, 1:6] = streams["v"][who[k]]
        inp[:, 6:13] = seg[k].view(np.uint32)
        inp[:, 13] = rays[who[k], 6].view(np.uint32)
        inp[:, 14:16] = light
        sh, _ = O.shade_batch(world, inp)
        assert (sh[:, 0] == 1).all(), "a shadow segment that ends on a light must end with a colour"
        assert (sh[:, 15] == copy["d"][k]).all() and (sh[:, 16:21] == copy["v"][k]).all(), "the shade step's search and the hit batch disagree"
        Le[k] = sh[:, 5:8].view(F)
    streams[who] = copy
    cen["shadow_segments"] += m
    cen["shadow_missed"] += int((~hit).sum())
    cen["shadow_on_medium"] += int(Q.on_medium(world, rec, hit).sum()) if medium_mats else 0
    cen["shadow_blocked"] += int((hit & ~on_light).sum())
    seen = (Le != 0).any(1)
    lit[who[seen]] += 1
    cen["lit"][who[seen]] += 1
    # (d) ((albedo * spdf) * Le) / pdf, added to the cached value
    k3 = (albedo * spdf[:, None]).astype(F)
    direct = ((k3 * Le).astype(F) / pdf[:, None]).astype(F)
    return (base + direct).astype(F)


class Ref:
    """rays (n, 8), streams0 / streams (before / after), rgb (n, 3), ends (n,), lit (n,), census, params (CACHED_PARAMS), records, depth"""


@functools.lru_cache(maxsize=None)
def reference(name, cache_depth, samples=1, mask="ones", visible=False, bounce_limit=None):
    """the walk's answer for the world's rays (R.rays_of) under the world's camera, its own light object included"""
    s = Q.build(name)
    g, rec, depth, vis = CR.volume(name, mask)
    r = Ref()
    r.name, r.world = name, s.world
    r.rays, r.streams0, r.slices = R.rays_of(name)
    r.path = hip.radiance_params_from_camera(R.copy_camera(s.cam, bounce_limit, R.world_light(name)), samples)
    r.grid, r.records = g, rec
    r.depth, r.vis = (depth, vis) if visible else (None, None)
    r.params = CR.params(r.path, cache_depth, g, r.vis)
    r.streams = r.streams0.copy()
    r.rgb, r.ends, r.lit, r.census = walk(s.world, r.path, cache_depth, g, rec, r.depth, r.vis, r.rays, r.streams)
    for a in (r.rgb, r.ends, r.lit, r.streams):
        a.setflags(write=False)
    return r


def assert_equal(got, streams, ref, what, idx=None):
    """a query's colours (raw words, NaN = NaN), all 48 bytes of every final stream and both counts against the walk's (idx: for
    those of its rays); a count the call did not return (None) is not compared"""
    R.assert_equal(got["rgb"], streams, ref, what, idx=idx)
    for key in ("ends", "lit"):
        if got.get(key) is None:
            continue
        want = getattr(ref, key) if idx is None else getattr(ref, key)[idx]
        bad = np.flatnonzero(np.asarray(got[key]) != want)
        assert bad.size == 0, f"{what}: {key} differ for {bad.size} rays, first {bad[0]}: got {got[key][bad[0]]} want {want[bad[0]]}"
