"""The reference side of the cached-radiance-query tests (tests/test_cached_host.py, tests/test_gpu_cached.py),
made from the oracle and the numpy restatements alone.

All rays are walked level by level in batches.  At a level, O.world_hit_batch on a COPY of the streams gives every path's hit
record and the streams after the media's draws; a Lambertian hit at iteration >= K takes its albedo from O.texture_value_batch and
its irradiance from volume_ref.sample / depth_ref.sample_visible, and where the weight sum is > 0 the path ends with
(albedo * E) * INV_PI and keeps the copy's stream.  Every other path goes through O.shade_batch on its ORIGINAL stream -- ray_color's
own loop body: the search again, emission, scatter, the mixture pdf -- which gives the stack entry, the next ray and the stream.
The unwind and the sum over the samples are numpy float32 in the contract's order.  reference() caches one answer per case per
process, and nothing may change it."""
import functools

import numpy as np

from mort_amd import hip
from tests import depth_cases as DC
from tests import depth_ref as D
from tests import oracle_lib as O
from tests import query_rays as Q
from tests import radiance_ref as R
from tests import volume_cases as K
from tests import volume_ref as V

F = np.float32
INV_PI = F(1.0 / 3.14159265358979323846)
MAT_LAMBERTIAN, MAT_DIELECTRIC = 1, 3
WORLDS = ("scene6", "scene1", "flat:lit_by_quad_with_media")
COUNT = (4, 3, 2)
VIS = (0.05, 0.05)  # normal_bias as a share of the smallest spacing, min_visibility
MASKS = ("ones", "fractional", "holes", "slab", "poison", "zeros")
# (mask, samples) of the bit-for-bit cases; each runs at K = 0, 1, 2, with and without MORT_CACHED_VISIBLE
CASES = (("ones", 1), ("fractional", 1), ("holes", 1), ("slab", 1), ("poison", 1), ("fractional", 3), ("slab", 3))
DEPTHS = (0, 1, 2)


# ------------------------------------------------------------------------------------------------------------------ volumes

@functools.lru_cache(maxsize=None)
def grid_of(name):
    """a COUNT grid over the world's reach box (the unified tree's); a world without a tree (scene 1: the reference BVH) takes
    the box of the middle 80 % per axis of the oracle's hit points of its primary rays instead"""
    s = Q.build(name)
    info = Q.reach(s.world)
    if info["tree"]:
        lo, hi = info["lo"].astype(np.float64), info["hi"].astype(np.float64)
    else:
        rays, streams0, slices = R.rays_of(name)
        pr = rays[slices["primary"]]
        rec, hit = O.world_hit_batch(s.world, pr[:, :7], Q.T_MIN, Q.INF, states=np.ascontiguousarray(streams0[slices["primary"]]).copy())
        p = rec["p"][hit & np.isfinite(rec["p"]).all(1)].astype(np.float64)
        lo, hi = np.percentile(p, 10, axis=0), np.percentile(p, 90, axis=0)
    spacing = (hi - lo) / (np.array(COUNT) - 1)
    return hip.VOLUME_GRID(tuple(float(F(x)) for x in lo), tuple(float(F(x)) for x in spacing), COUNT, 0.5)


def slab_records(g, seed=1):
    """K.records' "fractional" coefficients under a mask of its own: weight 0 for every probe with ix <= 1, 1 elsewhere, so the
    cells of the grid's first slab hold no contributing probe and their hits fall through to the shade step"""
    sh = K.coefficients(g, seed)
    ix = np.arange(g.probes) % g.count[0]
    return V.pack(sh, np.where(ix <= 1, F(0), F(1)).astype(F))


def poison_records(g, seed=1):
    """K.records' "ones" with NaN coefficients in one probe of weight 1, in the middle of the grid: no NaN guard, so every
    hit in the cells round it ends with a NaN colour"""
    rec = K.records(g, "ones", seed)
    mid = ((g.count[2] // 2) * g.count[1] + g.count[1] // 2) * g.count[0] + g.count[0] // 2
    rec[mid, :27] = np.nan
    return rec


@functools.lru_cache(maxsize=None)
def volume(name, mask):
    """(grid, records (probes, 32), depth (probes, 200), (normal_bias, min_visibility)) of a world: mask one of MASKS, or "baked"
    (scene 6 only: K.scene6_grid baked by the host form at D = 64, bounce limit 4, with DC.scene6_maps)"""
    if mask == "baked":
        assert name == "scene6"
        import mort_amd.structs as S
        world, cam = K.scene6()[:2]
        g, maps = DC.scene6_maps()
        pp = hip.probe_params_from_camera(cam, 64)
        pp.rp.bounce_limit = 4
        sh = hip.probe_bake_host(world, pp, hip.volume_probes(g), O.seed_states(S.DEFAULT_SEED, g.probes * 64, 1), nthreads=4)["sh"]
        rec, depth = V.pack(sh), np.array(maps)
    else:
        g = grid_of(name)
        rec = slab_records(g) if mask == "slab" else poison_records(g) if mask == "poison" else K.records(g, mask)
        # K.grid's cells are 0.45 .. 1.3 wide and DC.random_maps' distances lie in (0, 2): scaled to this grid's cells
        depth = DC.random_maps(g).reshape(g.probes, D.SIDE, D.SIDE, 2).copy()
        scale = F(min(g.spacing))
        depth[..., 0] *= scale
        depth[..., 1] *= scale * scale
        depth = depth.reshape(g.probes, D.DEPTH_FLOATS)
    vis = (float(F(VIS[0] * min(g.spacing))), VIS[1])
    rec.setflags(write=False); depth.setflags(write=False)
    return g, rec, depth, vis


def params(ref_params, cache_depth, g, vis=None):
    """hip.CACHED_PARAMS over a radiance query's parameters; vis (normal_bias, min_visibility) sets MORT_CACHED_VISIBLE"""
    return hip.CACHED_PARAMS(ref_params, cache_depth, g, hip.VOLUME_VIS_PARAMS(*vis) if vis is not None else None)


# ------------------------------------------------------------------------------------------------------------------ the walk

def _lambert_textures(world):
    m = world.c.mats
    return (np.array([m.host_lambertian[i].texType for i in range(m.num_lambertians)], dtype=np.int32),
            np.array([m.host_lambertian[i].texIdx for i in range(m.num_lambertians)], dtype=np.int32))


def walk(world, rp, cache_depth, g, records, depth, vis, rays, streams):
    """(rgb (n, 3), ends uint32 (n,), census dict); streams (O.STATE_DTYPE, n) are advanced in place.  rp: RADIANCE_PARAMS;
    depth / vis None: the plain sampler"""
    rays = np.asarray(rays, dtype=F).reshape(-1, 8)
    n = len(rays)
    assert streams.dtype == O.STATE_DTYPE and streams.shape == (n,)
    tex_type, tex_idx = _lambert_textures(world)
    background = np.array(list(rp.background), dtype=F)
    light = np.array([rp.light_obj_type, rp.light_obj_idx], dtype=np.int32).view(np.uint32)
    rgb = np.zeros((n, 3), dtype=F)
    ends = np.zeros(n, dtype=np.uint32)
    cen = dict(paths=0, ended=np.zeros(n, dtype=np.int64), segments=0, fell_through=0, after_dielectric=0)
    zero = F(0.0)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for _ in range(rp.samples):
            cur = np.ascontiguousarray(rays[:, :7]).copy()
            final = np.zeros((n, 3), dtype=F)
            levels = []  # per level: (path indices, k (m, 3), rp (m,), ident (m,))
            active = np.arange(n)
            last_dielectric = np.zeros(n, dtype=bool)
            it = 0
            while active.size:
                if it >= rp.bounce_limit:
                    final[active] = zero
                    break
                cen["segments"] += active.size
                probe = np.ascontiguousarray(streams[active]).copy()
                rec, hit = O.world_hit_batch(world, cur[active], Q.T_MIN, Q.INF, states=probe)
                take = np.zeros(active.size, dtype=bool)
                cand = hit & (rec["mat_type"] == MAT_LAMBERTIAN) if it >= cache_depth else take
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
                    final[who] = ((albedo[ok] * E[ok, :3]).astype(F) * INV_PI).astype(F)
                    streams[who] = probe[c[ok]]
                    ends[who] += 1
                    cen["ended"][who] += 1
                    cen["fell_through"] += int((~ok).sum())
                    cen["after_dielectric"] += int(last_dielectric[who].sum())
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
                last_dielectric[:] = False
                last_dielectric[nxt] = status[on] == 3
                active = nxt
                it += 1
            for who, k, rpdf, ident in reversed(levels):
                f = final[who]
                t = (k * f).astype(F)
                f = np.where(ident[:, None], zero + f, zero + (rpdf[:, None] * t).astype(F)).astype(F)
                final[who] = f
            rgb = (rgb + final).astype(F)
            cen["paths"] += n
    return rgb, ends, cen


class Ref:
    """rays (n, 8), streams0 / streams (before / after), rgb (n, 3), ends (n,), census, params (CACHED_PARAMS), records, depth"""


@functools.lru_cache(maxsize=None)
def reference(name, cache_depth, samples=1, mask="ones", visible=False, bounce_limit=None):
    """the walk's answer for the world's rays (R.rays_of) under the world's camera, its own light object included (the parameters
    of R.reference(name, samples, bounce_limit, light=R.world_light(name)))"""
    s = Q.build(name)
    g, rec, depth, vis = volume(name, mask)
    r = Ref()
    r.name, r.world = name, s.world
    r.rays, r.streams0, r.slices = R.rays_of(name)
    r.path = hip.radiance_params_from_camera(R.copy_camera(s.cam, bounce_limit, R.world_light(name)), samples)
    r.grid, r.records = g, rec
    r.depth, r.vis = (depth, vis) if visible else (None, None)
    r.params = params(r.path, cache_depth, g, r.vis)
    r.streams = r.streams0.copy()
    r.rgb, r.ends, r.census = walk(s.world, r.path, cache_depth, g, rec, r.depth, r.vis, r.rays, r.streams)
    for a in (r.rgb, r.ends, r.streams):
        a.setflags(write=False)
    return r


def assert_equal(got, streams, ref, what, idx=None):
    """a cached query's colours (raw words, NaN = NaN), all 48 bytes of every final stream and the counts against the walk's
    (idx: for those of its rays)"""
    R.assert_equal(got["rgb"], streams, ref, what, idx=idx)
    want = ref.ends if idx is None else ref.ends[idx]
    bad = np.flatnonzero(np.asarray(got["ends"]) != want)
    assert bad.size == 0, f"{what}: ends differ for {bad.size} rays, first {bad[0]}: got {got['ends'][bad[0]]} want {want[bad[0]]}"


def share_ended(ref):
    """the share of the primary and secondary paths that ended in the volume"""
    ps = R.two_sets(ref)
    return float(ref.census["ended"][ps].sum()) / (ref.params.path.samples * (ps.stop - ps.start))


def mean_segments(ref):
    return ref.census["segments"] / ref.census["paths"]
