#!/usr/bin/env python3
"""cached_direct_time.py -- what the direct terminal costs beside the cached and the plain radiance query on the same rays, and what
the split of the volume into sampled direct and cached indirect light is worth.  Nothing is gated.

  time      (GPU) the Cornell box (scene 6), --width^2 pixel-centre rays (default 1024: 2^20), --samples paths each (default 4), one
            stream per ray seeded as the pixel's; --grid^3 probes (default 8) over [20, 535]^3 baked on the device (D = 256, one path
            per direction; the full and the indirect volume, depth maps with 2 x 2 rays per texel).  One call per run, HIP-event
            times from the calls' own `seconds`, warm, the median of --reps after --warmup with min and max, the streams put back
            before every run.  The yardsticks first -- query_radiance_cached_device at K = 0 and K = 1 on the full volume and
            query_radiance_device -- then the new call on the indirect volume at K = 0 and K = 1, with and without visibility:
            ms, the ratio to each yardstick, the shares of paths that ended in the volume and of those that were lit.
  segments  (CPU) the mean number of segments per path -- shadow segments included -- for every (rays / --segment-rays)-th of those
            rays from the walks of tests/cached_ref.py and tests/cached_direct_ref.py over the oracle; 0 leaves the walks out.
  worth     (CPU, host forms; --worth) scene 6 at --worth-width^2 (default 96), pixel-centre rays, 16 paths: the relative RMSE of
            rgb / 16 against query_radiance_host at 1024 paths on the same rays -- sqrt(sum (x - t)^2 / sum t^2) over pixels and
            channels -- for the cached query at K = 0 and K = 1 on the full volume, the new query at K = 0 and K = 1 on the indirect
            volume and, as a control that counts direct light twice, the new query at K = 0 on the full volume.

One JSON line.   --no-gpu: without the times."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SEED = 69420
BOX = (20.0, 535.0)
THREADS = 16


def grid_of(hip, count):
    sp = (BOX[1] - BOX[0]) / (count - 1)
    return hip.VOLUME_GRID((BOX[0],) * 3, (sp,) * 3, (count,) * 3, 0.5)


def cap_of(g):
    return float(np.float32(1.5 * np.sqrt(sum(float(s) ** 2 for s in g.spacing))))


def host_volumes(world, cam, g, D):
    """the records of the full and of the indirect volume and the depth maps, by the host forms (bit for bit the device's)"""
    from mort_amd import hip
    from tests import oracle_lib as O
    probes = hip.volume_probes(g)
    bake = hip.probe_bake_indirect_host(world, hip.probe_params_from_camera(cam, D), probes, O.seed_states(SEED, g.probes * D, 1), tree=True,
                                        nthreads=THREADS)
    rec = {k: hip.volume_pack_host(bake["sh_" + k])["records"] for k in ("full", "ind")}
    maps = hip.probe_depth_bake_host(world, hip.DEPTH_PARAMS(2, cap_of(g)), probes, tree=True, nthreads=THREADS)["depth"]
    return rec, maps


def host_rays(cam):
    from tests import oracle_lib as O
    from tests import query_rays as Q
    from tests.feature_ref import primary_rays
    return Q.ray8(primary_rays(cam), Q.INF), O.seed_states(SEED, cam.image_width, cam.image_height)


def segments(a, out):
    from mort_amd import hip, host
    from tests import cached_direct_ref as DR
    from tests import cached_ref as CR
    world, cam = host.build_scene(6, width=a.width, spp=1, aspect=1.0)
    rays, streams0 = host_rays(cam)
    idx = np.arange(0, len(rays), max(1, len(rays) // a.segment_rays))
    rays, streams0 = rays[idx], np.ascontiguousarray(streams0[idx])
    g = grid_of(hip, a.grid)
    rec, maps = host_volumes(world, cam, g, 64)
    path = hip.radiance_params_from_camera(cam, a.samples)
    seg = {}
    for key, depth in (("plain", path.bounce_limit), ("cached_k0", 0), ("cached_k1", 1)):
        _, ends, cen = CR.walk(world, path, depth, g, rec["full"], None, None, rays, streams0.copy())
        seg[key] = dict(mean_segments=cen["segments"] / cen["paths"], share_ended=float(ends.sum()) / cen["paths"])
    for key, depth, vis in (("direct_k0", 0, None), ("direct_k1", 1, None), ("direct_k0_visible", 0, (a.bias, 0.05)), ("direct_k1_visible", 1, (a.bias, 0.05))):
        _, ends, lit, cen = DR.walk(world, path, depth, g, rec["ind"], maps if vis else None, vis, rays, streams0.copy())
        seg[key] = dict(mean_segments=(cen["segments"] + cen["shadow_segments"]) / cen["paths"], share_ended=float(ends.sum()) / cen["paths"],
                        share_lit=float(lit.sum()) / max(1, int(ends.sum())))
    out["segments"] = dict(rays=len(idx), directions=64, **seg)


def worth(a, out):
    from mort_amd import hip, host
    world, cam = host.build_scene(6, width=a.worth_width, spp=1, aspect=1.0)
    rays, streams0 = host_rays(cam)
    g = grid_of(hip, a.grid)
    rec, _ = host_volumes(world, cam, g, 256)
    truth_paths, paths = 1024, 16
    truth = hip.query_radiance_host(world, hip.radiance_params_from_camera(cam, truth_paths), rays, streams0.copy(), tree=True,
                                    nthreads=THREADS)["rgb"].astype(np.float64) / truth_paths
    path = hip.radiance_params_from_camera(cam, paths)

    def err(rgb):
        x = np.nan_to_num(rgb.astype(np.float64) / paths)
        return float(np.sqrt(((x - truth) ** 2).sum() / (truth ** 2).sum()))

    res = dict(width=cam.image_width, truth_paths=truth_paths, paths=paths, probes=g.probes, directions=256)
    res["plain"] = err(hip.query_radiance_host(world, path, rays, streams0.copy(), tree=True, nthreads=THREADS)["rgb"])
    for k in (0, 1):
        p = hip.CACHED_PARAMS(path, k, g)
        res[f"cached_k{k}_full"] = err(hip.query_radiance_cached_host(world, p, rays, streams0.copy(), rec["full"], tree=True, nthreads=THREADS)["rgb"])
        d = hip.query_radiance_cached_direct_host(world, p, rays, streams0.copy(), rec["ind"], tree=True, nthreads=THREADS)
        res[f"direct_k{k}_indirect"] = err(d["rgb"])
        res[f"direct_k{k}_share_lit"] = float(d["lit"].sum()) / max(1, int(d["ends"].sum()))
    p = hip.CACHED_PARAMS(path, 0, g)
    res["direct_k0_full_control"] = err(hip.query_radiance_cached_direct_host(world, p, rays, streams0.copy(), rec["full"], tree=True, nthreads=THREADS)["rgb"])
    out["worth"] = res


def gpu(a, out):
    import torch
    from mort_amd import hip, host
    from scripts.query_time import primary_rays
    dev = torch.device("cuda", 0)

    def med(f):
        t = [f() for _ in range(a.warmup + a.reps)][a.warmup:]
        return dict(ms=float(np.median(t)) * 1e3, ms_min=min(t) * 1e3, ms_max=max(t) * 1e3)

    with hip.Context(0) as ctx:
        world, cam = host.build_scene(6, width=a.width, spp=1, aspect=1.0)
        W, H = cam.image_width, cam.image_height
        n = W * H
        ctx.upload_world(world)
        ctx.rng_seed(SEED, W, H)
        seeded = torch.from_numpy(ctx.rng_store(W, H)).to(dev)
        rays = primary_rays(cam, dev)
        g = grid_of(hip, a.grid)
        probes = hip.volume_probes(g)
        D = 256
        bake = ctx.probe_bake_indirect(hip.probe_params_from_camera(cam, D), probes, hip.seed_states_host(SEED, g.probes * D, 1))
        rec = {k: torch.from_numpy(ctx.volume_pack(bake["sh_" + k])["records"]).to(dev) for k in ("full", "ind")}
        dbake = ctx.probe_depth_bake(hip.DEPTH_PARAMS(2, cap_of(g)), probes)
        maps = torch.from_numpy(dbake["depth"]).to(dev)
        out["volume"] = dict(probes=g.probes, directions=D, both_bakes_ms=bake["seconds"] * 1e3, depth_bake_ms=dbake["seconds"] * 1e3)
        path = hip.radiance_params_from_camera(cam, a.samples)
        streams = torch.empty_like(seeded)
        rgb = torch.zeros(n * 3, dtype=torch.float32, device=dev)
        ends = torch.zeros(n, dtype=torch.int32, device=dev)
        lit = torch.zeros(n, dtype=torch.int32, device=dev)

        def run(kind, depth=None, vis=None):
            p = hip.CACHED_PARAMS(path, depth, g, hip.VOLUME_VIS_PARAMS(*vis) if vis else None) if depth is not None else None

            def once():
                streams.copy_(seeded)
                torch.cuda.synchronize()
                if kind == "plain":
                    return ctx.query_radiance_device(path, rays, streams, rgb, sync=True)
                if kind == "cached":
                    return ctx.query_radiance_cached_device(p, rays, streams, rec["full"], maps if vis else None, rgb, ends, sync=True)
                return ctx.query_radiance_cached_direct_device(p, rays, streams, rec["ind"], maps if vis else None, rgb, ends, lit, sync=True)

            t = med(once)
            t["mpaths_per_s"] = n * a.samples / t["ms"] / 1e3
            if kind != "plain":
                t["share_ended"] = float(ends.sum()) / (n * a.samples)
            if kind == "direct":
                t["share_lit"] = float(lit.sum()) / max(1.0, float(ends.sum()))
            return t

        out.update(width=W, rays=n, samples=a.samples, bounce_limit=cam.bounce_limit, reps=a.reps, warmup=a.warmup)
        times = {}
        for key, kind, depth, vis in (("cached_k0", "cached", 0, None), ("cached_k1", "cached", 1, None), ("plain", "plain", None, None),
                                      ("direct_k0", "direct", 0, None), ("direct_k1", "direct", 1, None),
                                      ("direct_k0_visible", "direct", 0, (a.bias, 0.05)), ("direct_k1_visible", "direct", 1, (a.bias, 0.05))):
            times[key] = run(kind, depth, vis)
        for key in times:
            if key.startswith("direct"):
                for y in ("cached_k0", "cached_k1", "plain"):
                    times[key]["over_" + y] = times[key]["ms"] / times[y]["ms"]
        out["times"] = times


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--bias", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--segment-rays", type=int, default=4096)
    ap.add_argument("--worth", action="store_true")
    ap.add_argument("--worth-width", type=int, default=96)
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    out = {}
    if not a.no_gpu:
        import torch
        torch.cuda.init()  # torch's HIP runtime before the library's, as in tests/conftest.py, whatever runs first below
    if a.segment_rays > 0:
        segments(a, out)
    if a.worth:
        worth(a, out)
    if not a.no_gpu:
        gpu(a, out)
    print(json.dumps(out))
