"""The reference side of the cached-frame tests (tests/test_cached_frame_host.py, tests/test_gpu_cached_frame.py),
made from the oracle and the numpy restatements alone.

A frame is walked sample by sample, (s_i, s_j) in the render's order.  For a sample, O.camera_batch's get_ray draws every pixel's
ray from the pixel's stream; then all those paths are walked level by level as tests/cached_ref.py walks a query's: O.world_hit_batch
on a COPY of the streams, a Lambertian hit at iteration >= K sampled through volume_ref.sample / depth_ref.sample_visible with its
albedo from O.texture_value_batch, every other path through O.shade_batch on its ORIGINAL stream.  The level loop is restated here
because a frame wants the segments of every pixel, which cached_ref.walk only totals.  The unwind and the float32 sum over the samples
are in the contract's order; the oracle's pixel finish (O.camera_batch fn 2) makes the accumulators and the uchar4.  reference()
caches one answer per case per process, and nothing may change it."""
import ctypes as C
import functools

import numpy as np

from mort_amd import hip, host
from tests import cached_ref as CR
from tests import depth_ref as D
from tests import oracle_lib as O
from tests import query_rays as Q
from tests import radiance_ref as R
from tests import volume_ref as V

F = np.float32
U = np.uint32
WORLDS = CR.WORLDS
MASKS = CR.MASKS
DEPTHS = CR.DEPTHS
SIZE = (17, 15)  # the CPU tests' frame: 255 pixels
# frame sizes whose pixel counts straddle a wave and a group
SIZES = ((1, 1), (9, 7), (8, 8), (13, 5), (17, 15), (16, 16), (257, 1), (40, 33))
SEED = 69420
# the flat world's second view: from above, down onto the ground at x < -33, which its own camera never sees and where the slab
# mask's cells without a contributing probe lie (the grid spans the ground sphere, cells of 66.7 x 115 x 200)
ASIDE = ((-25.0, 25.0, 2.5), (-45.0, -12.0, -1.0), 55)


# ------------------------------------------------------------------------------------------------------------------ cameras

@functools.lru_cache(maxsize=None)
def camera(name, size=SIZE, spp=4, lens=False, bounce_limit=None, aside=False):
    """the world's own camera (tests/query_rays.py) with its light object, shrunk to `size`; lens: defocus_angle > 0 (scene 1's
    camera has a lens of its own, the others get 0.6 degrees at their own focus distance); aside: from ASIDE instead"""
    s = Q.build(name)
    cam = R.copy_camera(s.cam, bounce_limit, R.world_light(name))
    W, H = size
    cam.image_width = W
    cam.aspect_ratio = W / (H + 0.5)  # image_height = int(W / aspect_ratio)
    cam.samples_per_pixel = spp
    if lens and not cam.defocus_angle > 0:
        cam.defocus_angle = 0.6
    if aside:
        for k in range(3):
            cam.lookfrom.e[k], cam.lookat.e[k] = ASIDE[0][k], ASIDE[1][k]
        cam.vfov = ASIDE[2]
    host.lib().mort_camera_initialize(C.byref(cam))
    assert (cam.image_width, cam.image_height) == (W, H), (cam.image_width, cam.image_height)
    assert not lens or cam.defocus_angle > 0
    return cam


def slab_aside(name):
    """the slab mask's cases of the flat world look from ASIDE: its own camera sees one hit in a cell without a contributing probe"""
    return name.startswith("flat:")


def params(cache_depth, g, vis=None):
    """hip.CACHED_FRAME_PARAMS; vis (normal_bias, min_visibility) sets MORT_CACHED_VISIBLE"""
    return hip.CACHED_FRAME_PARAMS(cache_depth, g, hip.VOLUME_VIS_PARAMS(*vis) if vis is not None else None)


# ------------------------------------------------------------------------------------------------------------------ the walk

def get_rays(cam, streams, s_i, s_j):
    """get_ray for every pixel, from the pixel's stream (advanced in place): rays (n, 7), draws (n,)"""
    W, H = cam.image_width, cam.image_height
    n = W * H
    rec = np.zeros((n, 30), dtype=U)
    rec[:, 0] = streams["d"]
    rec[:, 1:6] = streams["v"]
    lofs = np.arange(n)
    rec[:, 6], rec[:, 7] = (lofs % W).astype(U), (lofs // W).astype(U)
    rec[:, 8], rec[:, 9] = s_i, s_j
    rec[:, 10] = np.array([cam.recip_sqrt_spp], dtype=F).view(U)[0]
    rec[:, 11] = np.array([cam.defocus_angle], dtype=F).view(U)[0]
    vec = np.array([[v.e[k] for k in range(3)] for v in (cam.center, cam.pixel00_loc, cam.pixel_delta_u, cam.pixel_delta_v, cam.defocus_disk_u,
                                                          cam.defocus_disk_v)], dtype=F).reshape(18)
    rec[:, 12:30] = vec.view(U)
    out = O.camera_batch(0, rec)
    streams["d"] = out[:, 7]
    streams["v"] = out[:, 8:13]
    return np.ascontiguousarray(out[:, 0:7]).view(F), out[:, 13].astype(np.int64)


def walk_once(world, cam, cache_depth, g, records, depth, vis, rays, streams, tex, cen):
    """one path per ray (n, 7) of one sample: final (n, 3), ended bool (n,), segments (n,); streams advanced in place.  The level
    loop of cached_ref.walk, with the searches counted per path"""
    n = len(rays)
    tex_type, tex_idx = tex
    background = np.array([cam.background.e[k] for k in range(3)], dtype=F)
    light = np.array([cam.light_obj_type, cam.light_obj_idx], dtype=np.int32).view(U)
    zero = F(0.0)
    cur = np.ascontiguousarray(rays).copy()
    final = np.zeros((n, 3), dtype=F)
    ended = np.zeros(n, dtype=bool)
    segments = np.zeros(n, dtype=np.int64)
    levels = []  # per level: (path indices, k (m, 3), rp (m,), ident (m,))
    active = np.arange(n)
    last_dielectric = np.zeros(n, dtype=bool)
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
            final[who] = ((albedo[ok] * E[ok, :3]).astype(F) * CR.INV_PI).astype(F)
            streams[who] = probe[c[ok]]
            ended[who] = True
            cen["fell_through"] += int((~ok).sum())
            cen["after_dielectric"] += int(last_dielectric[who].sum())
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
        last_dielectric[:] = False
        last_dielectric[nxt] = status[on] == 3
        active = nxt
        it += 1
    for who, k, rpdf, ident in reversed(levels):
        f = final[who]
        t = (k * f).astype(F)
        final[who] = np.where(ident[:, None], zero + f, zero + (rpdf[:, None] * t).astype(F)).astype(F)
    return final, ended, segments


def frame(world, cam, cache_depth, g, records, depth, vis, streams):
    """one cached frame over streams (O.STATE_DTYPE, W H), advanced in place: dict(rgba (H, W, 4), accum (H, W, 3), segments_px,
    ends_px (H, W), segments, census)"""
    W, H = cam.image_width, cam.image_height
    n = W * H
    assert streams.dtype == O.STATE_DTYPE and streams.shape == (n,)
    tex = CR._lambert_textures(world)
    color = np.zeros((n, 3), dtype=F)
    ends = np.zeros(n, dtype=U)
    segments = np.zeros(n, dtype=np.int64)
    cen = dict(paths=0, fell_through=0, after_dielectric=0)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for s_j in range(cam.sqrt_spp):
            for s_i in range(cam.sqrt_spp):
                rays, _ = get_rays(cam, streams, s_i, s_j)
                final, ended, seg = walk_once(world, cam, cache_depth, g, records, depth, vis, rays, streams, tex, cen)
                color = (color + final).astype(F)
                ends += ended.astype(U)
                segments += seg
                cen["paths"] += n
        rec = np.concatenate([np.full((n, 1), cam.pixel_samples_scale, dtype=F), color], 1)
        tail = O.camera_batch(2, np.ascontiguousarray(rec).view(U))
    cen["nan_pixels"] = int(np.isnan(color).any(1).sum())
    return dict(rgba=np.ascontiguousarray(tail[:, 3]).view(np.uint8).reshape(H, W, 4), accum=np.ascontiguousarray(tail[:, 0:3]).view(F).reshape(H, W, 3),
                segments_px=segments.astype(U).reshape(H, W), ends_px=ends.reshape(H, W), segments=int(segments.sum()), census=cen)


class Ref:
    """world, cam, params (CACHED_FRAME_PARAMS), records, depth, streams0, frames: a list of frame() dicts, each with the streams
    after it"""


@functools.lru_cache(maxsize=None)
def reference(name, cache_depth, size=SIZE, spp=4, mask="ones", visible=False, lens=False, bounce_limit=None, frames=1, aside=False):
    s = Q.build(name)
    g, rec, depth, vis = CR.volume(name, mask)
    r = Ref()
    r.name, r.world = name, s.world
    r.cam = camera(name, size, spp, lens, bounce_limit, aside)
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


def words(a):
    """float32 as raw words, every NaN the same word"""
    a = np.ascontiguousarray(a, dtype=F)
    return np.where(np.isnan(a), U(0x7fc00000), a.view(U))


def assert_equal(got, states, want, what, ends=True):
    """a frame's uchar4, accumulator words (NaN = NaN), per-pixel segments, counts and all 48 bytes of every final stream against
    a frame() dict of the reference"""
    assert (got["rgba"] == want["rgba"]).all(), f"{what}: uchar4 differs in {int((got['rgba'] != want['rgba']).any(-1).sum())} pixels"
    bad = np.flatnonzero((words(got["accum"]) != words(want["accum"])).any(-1).reshape(-1))
    assert bad.size == 0, f"{what}: accumulators differ in {bad.size} pixels, first {bad[0]}"
    if got.get("segments_px") is not None:
        assert (got["segments_px"] == want["segments_px"]).all(), f"{what}: per-pixel segments differ"
    if ends:
        assert (got["ends_px"] == want["ends_px"]).all(), f"{what}: ends differ in {int((got['ends_px'] != want['ends_px']).sum())} pixels"
    a = np.ascontiguousarray(states).view(np.uint8).reshape(-1, 48)
    b = np.ascontiguousarray(want["states"]).view(np.uint8).reshape(-1, 48)
    bad = np.flatnonzero((a != b).any(1))
    assert bad.size == 0, f"{what}: final stream differs for {bad.size} pixels, first {bad[0]}"


def share_ended(f, spp):
    return float(f["ends_px"].sum()) / (spp * f["ends_px"].size)
