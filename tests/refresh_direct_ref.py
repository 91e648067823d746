"""The reference side of the direct-light volume-refresh tests (tests/test_refresh_direct_host.py, tests/test_gpu_refresh_direct.py;
DESIGN.md 4.24), made from the oracle and numpy alone.

Positions, selection, blend and the copy rule are tests/refresh_ref's, the projection tests/probe_ref.project.  walk() is
tests/cached_direct_ref.walk restated with rule E: at iteration 0 a path the shade step ends with a colour (status 1: a diffuse
light or a material it does not know) gets 0 in place of that colour; the search, the shade step and the streams stay as they
were.  The terminal (rules (b)-(d)) is cached_direct_ref._direct itself.

The lit worlds take NEAR-LIGHT grids, placed so that every probe (scene 6, the flat world) or most probes (the BVH light world,
where one probe lies inside a sphere light) see an emitter along some of the library's 64 directions; scene 1 has no emitter and
keeps cached_ref's grid.  Records and maps are volume_cases.records and depth_cases.random_maps, scaled as cached_ref.volume
scales them.  reference() caches one answer per case per process, and nothing may change it."""
import functools

import numpy as np

import mort_amd.structs as S
from mort_amd import hip
from tests import cached_direct_ref as DR
from tests import cached_ref as CR
from tests import depth_cases as DC
from tests import depth_ref as D
from tests import oracle_lib as O
from tests import probe_ref as PR
from tests import query_rays as Q
from tests import refresh_ref as RR
from tests import volume_cases as K
from tests import volume_ref as V

F = np.float32
INV_PI = CR.INV_PI
BVH_LIGHT_WORLD = DR.BVH_LIGHT_WORLD
LIT_WORLDS = ("scene6", "flat:lit_by_quad_with_media", BVH_LIGHT_WORLD)
WORLDS = LIT_WORLDS + ("scene1",)
TREE_WORLDS = DR.TREE_WORLDS
MASKS = ("ones", "fractional", "holes", "poison")
LIMIT = RR.LIMIT
FILL = RR.FILL
# origin, spacing, count of the near-light grids
NEAR = {
    "scene6": ((178.0, 400.0, 180.0), (100.0, 75.0, 100.0), (3, 2, 2)),
    "flat:lit_by_quad_with_media": ((-1.2, 0.8, -2.2), (0.8, 0.6, 1.2), (4, 2, 2)),
    BVH_LIGHT_WORLD: ((-2.0, 0.9, -1.9), (1.2, 0.4, 0.7), (4, 2, 2)),
}


@functools.lru_cache(maxsize=None)
def grid_of(name):
    if name in NEAR:
        origin, spacing, count = NEAR[name]
        return hip.VOLUME_GRID(origin, spacing, count, 0.5)
    return CR.grid_of(name)


def selections(P):
    """(first, step, m): everything, a stride, the last probe alone, a stride that stops short"""
    return ((0, 1, P), (1, 5, 3), (P - 1, 1, 1), (3, 7, 2))


@functools.lru_cache(maxsize=None)
def volume(name, mask):
    """(grid, records (P, 32), depth (P, 200), (normal_bias, min_visibility)): cached_ref.volume's rule on this module's grids"""
    g = grid_of(name)
    rec = CR.poison_records(g) if mask == "poison" else K.records(g, mask)
    depth = DC.random_maps(g).reshape(g.probes, D.SIDE, D.SIDE, 2).copy()
    scale = F(min(g.spacing))
    depth[..., 0] *= scale
    depth[..., 1] *= scale * scale
    depth = depth.reshape(g.probes, D.DEPTH_FLOATS)
    vis = (float(F(CR.VIS[0] * min(g.spacing))), CR.VIS[1])
    rec.setflags(write=False); depth.setflags(write=False)
    return g, rec, depth, vis


def walk(world, rp, cache_depth, g, records, depth, vis, rays, streams):
    """(rgb (n, 3), ends uint32 (n,), lit uint32 (n,), census dict); streams (O.STATE_DTYPE, n) are advanced in place.
    cached_direct_ref.walk with rule E; census: that walk's keys, plus rule_e (n,) bool: the ray's primary segment fell under the
    rule in some path, rule_e_emits (n,) bool: with a non-zero colour, and value (n, samples, 3): each path's value"""
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
               pdf_not_positive=0, shadow_segments=0, shadow_on_medium=0, shadow_missed=0, shadow_blocked=0,
               rule_e=np.zeros(n, dtype=bool), rule_e_emits=np.zeros(n, dtype=bool), value=np.zeros((n, rp.samples, 3), dtype=F))
    medium_mats = Q.medium_materials(world)
    zero = F(0.0)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for sample in range(rp.samples):
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
                        final[who] = DR._direct(world, light, who, base, albedo[ok], np.ascontiguousarray(r["p"][ok]),
                                                np.ascontiguousarray(r["normal"][ok]), rays, streams, lit, cen, medium_mats)
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
                colour = out[status == 1, 5:8].view(F)
                if it == 0:  # rule E: what the probe sees directly is not indirect light
                    cen["rule_e"][who[status == 1]] = True
                    cen["rule_e_emits"][who[status == 1]] |= (colour != 0).any(1)
                    colour = np.zeros_like(colour)
                final[who[status == 1]] = colour
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
            cen["value"][:, sample] = final
            rgb = (rgb + final).astype(F)
            cen["paths"] += n
    return rgb, ends, lit, cen


def refresh(world, path, cache_depth, g, records_in, depth, vis, dirs, h, sel, streams, records_out, ends_out=None, lit_out=None):
    """one call, as refresh_ref.refresh: streams, records_out, ends_out and lit_out (or None) are written in place for the selected
    probes.  Returns the census: s (the active probes' direction sums), active, masked, ends / lit (n, D), walk (the walk's)"""
    first, step, m = sel
    Dn = len(dirs)
    P = g.probes
    assert streams.shape == (P * Dn,) and records_in.shape == (P, 32) and records_out.shape == (P, 32)
    probes = RR.positions(g)
    sel_p = RR.selected(first, step, m)
    assert m == 0 or sel_p[-1] < P
    with np.errstate(invalid="ignore"):
        live = records_in[sel_p, 27] > 0
    active, masked = sel_p[live], sel_p[~live]
    win, wout = records_in.view(np.uint32), records_out.view(np.uint32)
    wout[masked] = win[masked]
    for counts in (ends_out, lit_out):
        if counts is not None:
            counts[masked] = 0
    cen = dict(active=active, masked=masked, s=np.zeros((0, Dn, 3), dtype=F), walk=None)
    if active.size == 0:
        return cen
    idx = (active[:, None] * Dn + np.arange(Dn)[None, :]).reshape(-1)
    sub = np.ascontiguousarray(streams[idx])
    rays = PR.rays_of(probes[active], dirs)
    rgb, ends, lit, wc = walk(world, path, cache_depth, g, records_in, depth, vis, rays, sub)
    streams[idx] = sub
    s = rgb.reshape(active.size, Dn, 3)
    new = PR.project(s, dirs, path.samples).reshape(active.size, 27)
    out = np.zeros((active.size, 32), dtype=F)
    out[:, :27] = RR.blend(records_in[active, :27], new, h)
    ow = out.view(np.uint32)
    ow[:, 27] = win[active, 27]
    wout[active] = ow
    if ends_out is not None:
        ends_out[active] = ends.reshape(active.size, Dn).sum(1)
    if lit_out is not None:
        lit_out[active] = lit.reshape(active.size, Dn).sum(1)
    cen.update(s=s, walk=wc, ends=ends.reshape(active.size, Dn), lit=lit.reshape(active.size, Dn))
    return cen


def path_of(name, samples=1, limit=LIMIT, light=True):
    """the world's radiance parameters; light False: without its light object"""
    p = RR.path_of(name, samples, limit)
    if not light:
        p.light_obj_type, p.light_obj_idx = -1, 0
    return p


streams_of = RR.streams_of
params_of = RR.params_of


def filled(P, fill=FILL):
    """(records (P, 32) float32, ends (P,), lit (P,) uint32) of the fill byte"""
    rec, ends = RR.filled(P, fill)
    return rec, ends, ends.copy()


class Ref:
    """world, grid, params (REFRESH_PARAMS), m, dirs, records_in, depth, streams0 / streams, records (P, 32; unselected FILL), ends
    and lit (P,; unselected FILL words), census"""


@functools.lru_cache(maxsize=None)
def reference(name, cache_depth=0, h=0.0, samples=1, mask="ones", visible=False, D=64, sel=None, limit=LIMIT, dirs=None, light=True):
    """sel None: every probe; dirs: None = the library's set (restated), an int r = round r's set (restated), else a kind of
    PR.own_directions"""
    s = Q.build(name)
    g, rec, depth, vis = volume(name, mask)
    sel = (0, 1, g.probes) if sel is None else sel
    r = Ref()
    r.name, r.world, r.grid = name, s.world, g
    r.path = path_of(name, samples, limit, light)
    r.dirs = PR.fibonacci(D) if dirs is None else RR.directions_round(D, dirs) if isinstance(dirs, int) else PR.own_directions(dirs)
    assert len(r.dirs) == D
    r.records_in = rec
    r.depth, r.vis = (depth, vis) if visible else (None, None)
    r.sel, r.m = sel, sel[2]
    r.params = params_of(r.path, cache_depth, g, r.vis, D, h, sel)
    r.streams0 = streams_of(g.probes, D)
    r.streams = r.streams0.copy()
    r.records, r.ends, r.lit = filled(g.probes)
    r.census = refresh(s.world, r.path, cache_depth, g, rec, r.depth, r.vis, r.dirs, h, sel, r.streams, r.records, r.ends, r.lit)
    for a in (r.dirs, r.streams0, r.streams, r.records, r.ends, r.lit):
        a.setflags(write=False)
    return r


def assert_equal(records, streams, ends, lit, ref, what):
    """refresh_ref.assert_equal (records as raw words with NaN = NaN, all 48 bytes of every stream, ends) and lit, the unselected
    words against the fill they were given"""
    RR.assert_equal(records, streams, ends, ref, what)
    if lit is not None:
        bad = np.flatnonzero(np.asarray(lit) != ref.lit)
        assert bad.size == 0, f"{what}: lit differs for {bad.size} probes, first {bad[0]}: got {lit[bad[0]]} want {ref.lit[bad[0]]}"
