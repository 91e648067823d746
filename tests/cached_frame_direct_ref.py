"""The reference side of the direct-light cached-frame tests (tests/test_cached_frame_direct_host.py,
tests/test_gpu_cached_frame_direct.py), made from the oracle and the numpy restatements alone, never the library.

cached_frame_ref's walk (get_rays, the level loop of walk_once, frame) with cached_direct_ref's terminal: where a path ends in the
volume, the camera names a light object and the bounce limit leaves a segment, the direction and its pdf come from O.light_batch,
the shadow segment's search from O.world_hit_batch on a COPY of the stream and the emission from O.shade_batch
(cached_direct_ref._direct, with the sample's ray time).  The shadow search is counted as a segment of its pixel, and the frame
gives lit_px beside ends_px.  The worlds are cached_frame_ref's and cached_direct_ref.BVH_LIGHT_WORLD: scene 1 has no light object
and shows identity (i), the list of sphere lights over a reference BVH makes the kernel without the unified tree meet a light.
reference() caches one answer per case per process, and nothing may change it."""
import ctypes as C
import functools

import numpy as np

from mort_amd import host
from tests import cached_direct_ref as CD
from tests import cached_frame_ref as FR
from tests import cached_ref as CR
from tests import depth_ref as D
from tests import oracle_lib as O
from tests import query_rays as Q
from tests import radiance_ref as R
from tests import volume_ref as V

F = np.float32
U = np.uint32
WORLDS = FR.WORLDS + (CD.BVH_LIGHT_WORLD,)
TREE_WORLDS = CD.TREE_WORLDS  # worlds with a unified tree: cached_frame_direct_kernel<true, *> on the GPU; the others <false, *>
MASKS = FR.MASKS
DEPTHS = FR.DEPTHS
SIZE = FR.SIZE
SIZES = FR.SIZES
SEED = FR.SEED
CENSUS_KEYS = ("paths", "fell_through", "rule_a", "pdf_not_positive", "shadow_segments", "shadow_on_medium", "shadow_missed", "shadow_blocked")

# two more views of the BVH light world, for the terminal's rare branches (lookfrom, lookat, vfov).  "below": from inside the ground
# sphere down onto its far inside, 100-200 away, where the fp32 hit test of a 0.2-wide light fails and its pdf_value is 0.  "far":
# from z = 17 along the ground, whose points see the lights under a ratio radius^2 / distance^2 near 1e-4: a direction drawn at the
# cone's rim then passes the light by a rounding and leaves the world, a shadow segment that misses (about 3 in 100 000)
VIEWS = {"below": ((0.0, -0.52, 0.6), (0.3, -3.0, 0.5), 60), "far": ((0.0, 0.3, 17.0), (0.0, -0.5, 3.0), 20)}
FAR_SIZE, FAR_SPP = (96, 80), 16

params = FR.params
words = FR.words


@functools.lru_cache(maxsize=None)
def camera(name, size=SIZE, spp=4, lens=False, bounce_limit=None, aside=False, view=None, light=True):
    """cached_frame_ref.camera; view: from VIEWS instead; light=False: without its light object"""
    cam = FR.camera(name, size, spp, lens, bounce_limit, aside)
    if view is None and light:
        return cam
    cam = R.copy_camera(cam, light=None if light else (-1, 0))
    if view is not None:
        frm, at, vfov = VIEWS[view]
        for k in range(3):
            cam.lookfrom.e[k], cam.lookat.e[k] = frm[k], at[k]
        cam.vfov = vfov
        host.lib().mort_camera_initialize(C.byref(cam))
        assert (cam.image_width, cam.image_height) == tuple(size)
    return cam


def walk_once(world, cam, cache_depth, g, records, depth, vis, rays, streams, tex, cen, medium_mats):
    """one path per ray (n, 7) of one sample: final (n, 3), ended bool (n,), lit bool (n,), segments (n,); streams advanced in
    place.  cached_frame_ref.walk_once with the terminal of cached_direct_ref.walk"""
    n = len(rays)
    tex_type, tex_idx = tex
    background = np.array([cam.background.e[k] for k in range(3)], dtype=F)
    light = np.array([cam.light_obj_type, cam.light_obj_idx], dtype=np.int32).view(U)
    has_light = cam.light_obj_type != -1
    zero = F(0.0)
    cur = np.ascontiguousarray(rays).copy()
    final = np.zeros((n, 3), dtype=F)
    ended = np.zeros(n, dtype=bool)
    lit = np.zeros(n, dtype=U)
    segments = np.zeros(n, dtype=np.int64)
    dcen = dict(lit=np.zeros(n, dtype=np.int64), pdf_not_positive=0, shadow_segments=0, shadow_on_medium=0, shadow_missed=0, shadow_blocked=0)
    levels = []  # per level: (path indices, k (m, 3), rp (m,), ident (m,))
    active = np.arange(n)
    it = 0
    while active.size:
        if it >= cam.bounce_limit:
            final[active] = zero
            break
        segments[active] += 1
        probe = np.ascontiguousarray(streams[active]).copy()
        rec, hit = O.world_hit_batch(world, cur[active], Q.T_MIN, Q.INF, states=probe)
        take = np.zeros(active.size, dtype=bool)
        cand = hit & (rec["mat_type"] == CR.MAT_LAMBERTIAN) if it >= cache_depth else take
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
            base = ((albedo[ok] * E[ok, :3]).astype(F) * CR.INV_PI).astype(F)
            streams[who] = probe[c[ok]]
            ended[who] = True
            cen["fell_through"] += int((~ok).sum())
            if not has_light or it + 1 >= cam.bounce_limit:  # rule (a): the cached frame's value, nothing drawn, no segment
                final[who] = base
                cen["rule_a"] += who.size
            elif who.size:
                final[who] = CD._direct(world, light, who, base, albedo[ok], np.ascontiguousarray(r["p"][ok]), np.ascontiguousarray(r["normal"][ok]),
                                        rays, streams, lit, dcen, medium_mats)
                segments[who] += 1  # one segment counted per search
        go = np.flatnonzero(~take)
        who = active[go]
        inp = np.zeros((who.size, 16), dtype=U)
        inp[:, 0] = streams["d"][who]
        inp[:, 1:6] = streams["v"][who]
        inp[:, 6:13] = cur[who].view(U)
        inp[:, 13] = rays[who, 6].view(U)
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
        final[who] = np.where(ident[:, None], zero + f, zero + (rpdf[:, None] * t).astype(F)).astype(F)
    for key in ("pdf_not_positive", "shadow_segments", "shadow_on_medium", "shadow_missed", "shadow_blocked"):
        cen[key] += dcen[key]
    assert (lit <= 1).all() and not (lit.astype(bool) & ~ended).any()
    return final, ended, lit.astype(bool), segments


def frame(world, cam, cache_depth, g, records, depth, vis, streams):
    """one direct cached frame over streams (O.STATE_DTYPE, W H), advanced in place: dict(rgba (H, W, 4), accum (H, W, 3),
    segments_px, ends_px, lit_px (H, W), segments, census)"""
    W, H = cam.image_width, cam.image_height
    n = W * H
    assert streams.dtype == O.STATE_DTYPE and streams.shape == (n,)
    tex = CR._lambert_textures(world)
    medium_mats = Q.medium_materials(world)
    color = np.zeros((n, 3), dtype=F)
    ends = np.zeros(n, dtype=U)
    lit = np.zeros(n, dtype=U)
    segments = np.zeros(n, dtype=np.int64)
    cen = dict.fromkeys(CENSUS_KEYS, 0)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for s_j in range(cam.sqrt_spp):
            for s_i in range(cam.sqrt_spp):
                rays, _ = FR.get_rays(cam, streams, s_i, s_j)
                final, ended, seen, seg = walk_once(world, cam, cache_depth, g, records, depth, vis, rays, streams, tex, cen, medium_mats)
                color = (color + final).astype(F)
                ends += ended.astype(U)
                lit += seen.astype(U)
                segments += seg
                cen["paths"] += n
        rec = np.concatenate([np.full((n, 1), cam.pixel_samples_scale, dtype=F), color], 1)
        tail = O.camera_batch(2, np.ascontiguousarray(rec).view(U))
    cen["ended"], cen["lit"] = int(ends.sum()), int(lit.sum())
    return dict(rgba=np.ascontiguousarray(tail[:, 3]).view(np.uint8).reshape(H, W, 4), accum=np.ascontiguousarray(tail[:, 0:3]).view(F).reshape(H, W, 3),
                segments_px=segments.astype(U).reshape(H, W), ends_px=ends.reshape(H, W), lit_px=lit.reshape(H, W), segments=int(segments.sum()),
                census=cen)


class Ref:
    """world, cam, params (CACHED_FRAME_PARAMS), records, depth, streams0, frames: a list of frame() dicts, each with the streams
    after it"""


@functools.lru_cache(maxsize=None)
def reference(name, cache_depth, size=SIZE, spp=4, mask="ones", visible=False, lens=False, bounce_limit=None, frames=1, aside=False, view=None,
              light=True):
    """light=False: the world's camera without its light object (identity (i) on a world that has one)"""
    s = Q.build(name)
    g, rec, depth, vis = CR.volume(name, mask)
    r = Ref()
    r.name, r.world = name, s.world
    r.cam = camera(name, size, spp, lens, bounce_limit, aside, view, light)
    r.grid, r.records = g, rec
    r.depth, r.vis = (depth, vis) if visible else (None, None)
    r.params = params(cache_depth, g, r.vis)
    r.streams0 = O.seed_states(SEED, size[0], size[1])
    r.streams0.setflags(write=False)
    streams = r.streams0.copy()
    r.frames = []
    for _ in range(frames):
        f = frame(s.world, r.cam, cache_depth, g, rec, r.depth, r.vis, streams)
        f["states"] = streams.copy()
        for a in f.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        r.frames.append(f)
    return r


def assert_equal(got, states, want, what, ends=True, lit=True):
    """cached_frame_ref.assert_equal and the lit counts"""
    FR.assert_equal(got, states, want, what, ends=ends)
    if lit:
        assert (got["lit_px"] == want["lit_px"]).all(), f"{what}: lit differ in {int((got['lit_px'] != want['lit_px']).sum())} pixels"
