#!/usr/bin/env python3
"""cached_frame_time.py -- what a cached frame costs beside the plain render of the same frame and beside the cached
radiance query on the same number of rays, and what its picture is worth.  HIP-event times from the calls' own statistics, warm,
the median of --reps runs after --warmup; the pixel streams are seeded anew before every run, so each run does the same work.
Nothing is gated.

  time   the Cornell box (scene 6), --width^2 pixels (default 1024), --spp samples (default 4).  A grid of --grid^3 probes (default
         8) over [20, 535]^3, baked on the device (D = 256, one path per direction, depth maps with 2 x 2 rays per texel): section
         4.19's setup.  Yardsticks: (a) mort_hip_render_device, MORT_MODE_MEGA, of the same frame; (b) the cached radiance query
         (mort_hip_query_radiance_cached_device) on the pixel-centre rays, as many rays and paths, at the same K.  Cases: the cached
         frame at K = 0, 1, 2, and at K = 1 with visibility; per case the time, its ratios to (a) and (b), the mean segments per path
         and the share of the paths that ended in the volume.
  rmse   at --rmse-width (default 256), 4 spp: the gamma-encoded frame (the uchar4 / 256) of a cached frame at K = 1 and of a plain
         render, each against a plain render at 1024 spp; alone, and as the 8th frame of a view's temporal + SVGF chain under a still
         camera.  Root mean square over pixels and channels on the picture's 0..1 scale.

One JSON line, also appended to --out (default profiles/cached_frame/cached_frame_time.jsonl)."""
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


def main(a):
    import torch
    torch.cuda.init()  # torch's HIP runtime first, as in tests/conftest.py
    from mort_amd import hip, host
    from scripts.query_time import primary_rays
    dev = torch.device("cuda", 0)
    out = {}

    def med(f):
        r = [f() for _ in range(a.warmup + a.reps)][a.warmup:]
        t = [x["seconds"] if isinstance(x, dict) else x for x in r]
        return dict(ms=float(np.median(t)) * 1e3, ms_min=min(t) * 1e3, ms_max=max(t) * 1e3), r[-1]

    with hip.Context(0) as ctx:
        world, cam = host.build_scene(6, width=a.width, spp=a.spp, aspect=1.0)
        W, H = cam.image_width, cam.image_height
        n, spp = W * H, cam.sqrt_spp ** 2
        ctx.upload_world(world)
        g = grid_of(hip, a.grid)
        probes = hip.volume_probes(g)
        D = 256
        bake = ctx.probe_bake(hip.probe_params_from_camera(cam, D), probes, hip.seed_states_host(SEED, g.probes * D, 1))
        rec = torch.from_numpy(ctx.volume_pack(bake["sh"])["records"]).to(dev)
        dbake = ctx.probe_depth_bake(hip.DEPTH_PARAMS(2, cap_of(g)), probes)
        maps = torch.from_numpy(dbake["depth"]).to(dev)
        out["volume"] = dict(probes=g.probes, directions=D, bake_ms=bake["seconds"] * 1e3, depth_bake_ms=dbake["seconds"] * 1e3)
        out.update(width=W, height=H, spp=spp, bounce_limit=cam.bounce_limit, reps=a.reps, warmup=a.warmup)

        rgba = torch.zeros(n * 4, dtype=torch.uint8, device=dev)
        accum = torch.zeros(n * 3, dtype=torch.float32, device=dev)
        ends = torch.zeros(n, dtype=torch.int32, device=dev)
        vis = hip.VOLUME_VIS_PARAMS(a.bias, 0.05)

        def frame(depth, visible):
            p = hip.CACHED_FRAME_PARAMS(depth, g, vis if visible else None)

            def once():
                ctx.rng_seed(SEED, W, H)
                return ctx.render_cached_device(cam, p, rec, maps if visible else None, rgba, accum, ends, sync=True)
            return once

        def plain():
            ctx.rng_seed(SEED, W, H)
            return ctx.render_device(cam, rgba.data_ptr(), accum.data_ptr(), mode=hip.MODE_MEGA, sync=True)

        # (b): the cached query on the pixel-centre rays, one stream per ray seeded as the pixel's
        ctx.rng_seed(SEED, W, H)
        seeded = torch.from_numpy(ctx.rng_store(W, H)).to(dev)
        rays = primary_rays(cam, dev)
        streams = torch.empty_like(seeded)
        rgb = torch.zeros(n * 3, dtype=torch.float32, device=dev)
        path = hip.radiance_params_from_camera(cam, spp)

        def query(depth, visible):
            p = hip.CACHED_PARAMS(path, depth, g, vis if visible else None)

            def once():
                streams.copy_(seeded)
                torch.cuda.synchronize()
                return ctx.query_radiance_cached_device(p, rays, streams, rec, maps if visible else None, rgb, ends, sync=True)
            return once

        times = {}
        t, st = med(plain)
        times["render_mega"] = dict(t, kernel=st["kernel_name"], mean_segments=st["segments"] / (n * spp))
        for key, depth, visible in (("k0", 0, False), ("k1", 1, False), ("k2", 2, False), ("k1_visible", 1, True)):
            t, st = med(frame(depth, visible))
            t.update(kernel=st["kernel_name"], vgprs=st["kernel_vgprs"], lds_bytes=st["kernel_lds_bytes"], mean_segments=st["segments"] / (n * spp),
                     share_ended=float(ends.sum()) / (n * spp), render_over_frame=times["render_mega"]["ms"] / t["ms"])
            q, _ = med(query(depth, visible))
            t.update(query_ms=q["ms"], query_over_frame=q["ms"] / t["ms"])
            times[key] = t
        out["times"] = times

        # ---- what the picture is worth
        world, cam = host.build_scene(6, width=a.rmse_width, spp=4, aspect=1.0)
        _, truth_cam = host.build_scene(6, width=a.rmse_width, spp=1024, aspect=1.0)
        W, H = cam.image_width, cam.image_height
        pic = lambda r: r[..., :3].astype(np.float64) / 256.0  # noqa: E731
        rmse = lambda x, y: float(np.sqrt(((x - y) ** 2).mean()))  # noqa: E731
        ctx.rng_seed(SEED + 1, W, H)
        truth = pic(ctx.render(truth_cam, mode=hip.MODE_MEGA, want_accum=False)["rgba"])
        p = hip.CACHED_FRAME_PARAMS(1, g, None)
        pv = hip.CACHED_FRAME_PARAMS(1, g, vis)
        rm = dict(width=W, truth_spp=1024, spp=4, frames=8)
        ctx.rng_seed(SEED, W, H)
        rm["plain"] = rmse(pic(ctx.render(cam, mode=hip.MODE_MEGA, want_accum=False)["rgba"]), truth)
        for key, params, depth_maps in (("k1", p, None), ("k1_visible", pv, maps)):
            ctx.rng_seed(SEED, W, H)
            rm[key] = rmse(pic(ctx.render_cached(cam, params, rec.cpu().numpy(), depth_maps.cpu().numpy() if depth_maps is not None else None,
                                                 want_accum=False, want_ends=False)["rgba"]), truth)
        for key, params, depth_maps in (("plain_view", None, None), ("k1_view", p, None), ("k1_visible_view", pv, maps)):
            ctx.rng_seed(SEED, W, H)
            with ctx.view(W, H, temporal=1, filter=hip.FILTER_SVGF) as v:
                if params is not None:
                    v.set_cache(params, rec, depth_maps)
                for _ in range(rm["frames"]):
                    last = v.frame(cam)["rgba"]
            rm[key] = rmse(pic(last), truth)
        out["rmse"] = rm
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--bias", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rmse-width", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cached_frame", "cached_frame_time.jsonl"))
    main(ap.parse_args())
