#!/usr/bin/env python3
"""cached_time.py -- what a cached radiance query costs beside the plain radiance query on the same rays, and what
its picture is worth.  HIP-event times from the calls' own `seconds`, warm, the median of --reps runs after --warmup; the streams
are put back before every run, so each run does the same work.  Nothing is gated.

  time      the Cornell box (scene 6), --width^2 primary rays (default 1024: 2^20; lens centre through every pixel centre, time
            0.5), --samples paths each (default 4), one stream per ray seeded as the pixel's.  A grid of --grid^3 probes (default 8)
            inside the box, baked on the device (D = 256, one path per direction, depth maps with 2 x 2 rays per texel).  Cases: the
            plain radiance query; the cached query at K = 0, 1 and 2; the cached query with visibility at K = 1.
  segments  the mean number of segments per path for the same rays, from the walk of tests/cached_ref.py over the oracle (needs no
            GPU; K = bounce limit is the plain query): the ratio plain / cached is what a kernel whose time went with its segments
            would reach.  --segment-rays N walks every (rays / N)-th ray; 0 leaves the walk out.
  rmse      at --rmse-width (default 256): the preview of `mort --radiance-out` -- sqrt(clamp(sum / N, 0, 1)), NaN as 0 -- of the
            cached query at K = 1 and 4 paths, and of the plain query at 4 paths, each against the plain query at 1024 paths;
            root mean square over pixels and channels on the picture's 0..1 scale.

One JSON line.   --no-gpu: the segments alone."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SEED = 69420
BOX = (20.0, 535.0)


def grid_of(hip, count):
    sp = (BOX[1] - BOX[0]) / (count - 1)
    return hip.VOLUME_GRID((BOX[0],) * 3, (sp,) * 3, (count,) * 3, 0.5)


def cap_of(g):
    return float(np.float32(1.5 * np.sqrt(sum(float(s) ** 2 for s in g.spacing))))


def segments(a, out):
    """the walk over the oracle, on the host alone: the volume baked by the host forms (bit for bit the device's)"""
    from mort_amd import hip, host
    from tests import cached_ref as CR
    from tests import oracle_lib as O
    from tests import query_rays as Q
    from tests.feature_ref import primary_rays
    world, cam = host.build_scene(6, width=a.width, spp=1, aspect=1.0)
    W, H = cam.image_width, cam.image_height
    step = max(1, (W * H) // a.segment_rays)
    idx = np.arange(0, W * H, step)
    rays = Q.ray8(primary_rays(cam), Q.INF)[idx]
    streams0 = np.ascontiguousarray(O.seed_states(SEED, W, H)[idx])
    g = grid_of(hip, a.grid)
    probes = hip.volume_probes(g)
    sh = hip.probe_bake_host(world, hip.probe_params_from_camera(cam, 64), probes, O.seed_states(SEED, g.probes * 64, 1), tree=True, nthreads=16)["sh"]
    rec = hip.volume_pack_host(sh)["records"]
    maps = hip.probe_depth_bake_host(world, hip.DEPTH_PARAMS(2, cap_of(g)), probes, tree=True, nthreads=16)["depth"]
    path = hip.radiance_params_from_camera(cam, a.samples)
    seg = {}
    for key, depth, vis in (("plain", path.bounce_limit, None), ("k0", 0, None), ("k1", 1, None), ("k2", 2, None), ("k1_visible", 1, (a.bias, 0.05))):
        _, ends, cen = CR.walk(world, path, depth, g, rec, maps if vis else None, vis, rays, streams0.copy())
        seg[key] = dict(mean_segments=cen["segments"] / cen["paths"], share_ended=float(ends.sum()) / cen["paths"])
    out["segments"] = dict(rays=len(idx), directions=64, **seg)


def gpu(a, out):
    import torch
    torch.cuda.init()  # torch's HIP runtime first, as in tests/conftest.py
    from mort_amd import hip, host
    from scripts.query_time import primary_rays
    dev = torch.device("cuda", 0)

    def med(f):
        t = [f() for _ in range(a.warmup + a.reps)][a.warmup:]
        return dict(ms=float(np.median(t)) * 1e3, ms_min=min(t) * 1e3, ms_max=max(t) * 1e3)

    with hip.Context(0) as ctx:
        def setup(width):
            world, cam = host.build_scene(6, width=width, spp=1, aspect=1.0)
            W, H = cam.image_width, cam.image_height
            ctx.upload_world(world)
            ctx.rng_seed(SEED, W, H)
            seeded = torch.from_numpy(ctx.rng_store(W, H)).to(dev)
            return world, cam, W * H, seeded, primary_rays(cam, dev)

        world, cam, n, seeded, rays = setup(a.width)
        g = grid_of(hip, a.grid)
        probes = hip.volume_probes(g)
        D = 256
        bake = ctx.probe_bake(hip.probe_params_from_camera(cam, D), probes, hip.seed_states_host(SEED, g.probes * D, 1))
        rec = torch.from_numpy(ctx.volume_pack(bake["sh"])["records"]).to(dev)
        dbake = ctx.probe_depth_bake(hip.DEPTH_PARAMS(2, cap_of(g)), probes)
        maps = torch.from_numpy(dbake["depth"]).to(dev)
        out["volume"] = dict(probes=g.probes, directions=D, bake_ms=bake["seconds"] * 1e3, depth_bake_ms=dbake["seconds"] * 1e3)

        def run(n, rays, seeded, samples, depth=None, vis=None):
            """(median times, rgb (n, 3), ends or None): depth None = the plain radiance query"""
            path = hip.radiance_params_from_camera(cam, samples)
            streams = torch.empty_like(seeded)
            rgb = torch.zeros(n * 3, dtype=torch.float32, device=dev)
            ends = torch.zeros(n, dtype=torch.int32, device=dev)
            p = hip.CACHED_PARAMS(path, depth, g, hip.VOLUME_VIS_PARAMS(*vis) if vis else None) if depth is not None else None

            def once():
                streams.copy_(seeded)
                torch.cuda.synchronize()
                if p is None:
                    return ctx.query_radiance_device(path, rays, streams, rgb, sync=True)
                return ctx.query_radiance_cached_device(p, rays, streams, rec, maps if vis else None, rgb, ends, sync=True)

            return med(once), rgb.view(n, 3), (ends if p is not None else None)

        out.update(width=cam.image_width, rays=n, samples=a.samples, bounce_limit=cam.bounce_limit, reps=a.reps, warmup=a.warmup)
        times = {}
        for key, depth, vis in (("plain", None, None), ("k0", 0, None), ("k1", 1, None), ("k2", 2, None), ("k1_visible", 1, (a.bias, 0.05))):
            t, rgb, ends = run(n, rays, seeded, a.samples, depth, vis)
            t["mpaths_per_s"] = n * a.samples / t["ms"] / 1e3
            if ends is not None:
                t["share_ended"] = float(ends.sum()) / (n * a.samples)
            times[key] = t
        for key in ("k0", "k1", "k2", "k1_visible"):
            times[key]["plain_over_cached"] = times["plain"]["ms"] / times[key]["ms"]
        out["times"] = times

        # the preview's worth
        def picture(rgb, samples):
            v = torch.nan_to_num(rgb / samples, nan=0.0).clamp(0, 1)
            return torch.sqrt(v)

        saved = (a.reps, a.warmup)
        a.reps, a.warmup = 1, 0
        world, cam, n, seeded, rays = setup(a.rmse_width)
        truth = picture(run(n, rays, seeded, 1024)[1], 1024)
        plain4 = picture(run(n, rays, seeded, 4)[1], 4)
        rm = dict(width=cam.image_width, truth_paths=1024, paths=4, plain=float(((plain4 - truth) ** 2).mean().sqrt()))
        for key, vis in (("k1", None), ("k1_visible", (a.bias, 0.05))):
            rm[key] = float(((picture(run(n, rays, seeded, 4, 1, vis)[1], 4) - truth) ** 2).mean().sqrt())
        a.reps, a.warmup = saved
        out["rmse"] = rm


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--bias", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rmse-width", type=int, default=256)
    ap.add_argument("--segment-rays", type=int, default=1 << 20)
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    out = {}
    if a.segment_rays > 0:
        segments(a, out)
    if not a.no_gpu:
        gpu(a, out)
    print(json.dumps(out), flush=True)
