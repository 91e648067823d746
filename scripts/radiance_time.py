#!/usr/bin/env python3
"""radiance_time.py -- what a batch of radiance queries costs beside the render of the same camera, all through the
same library in one call, HIP-event times of the kernels, the median of --reps runs after --warmup:

  query     mort_hip_query_radiance_device on the feature pass's primary rays (lens centre through every pixel centre, time 0.5),
            one stream per ray seeded as the pixel's, samples = 1 and samples = 16; the streams are put back before every run,
            so each run does the same work
  generic   mort_hip_render_device of the same camera at 1 spp and 16 spp with MORT_FORCE_GENERIC=1: mega_kernel, one lane per
            pixel -- the same loop plus get_ray and the pixel tail (its rays are jittered inside the pixel and start on the lens, so
            the work is alike, not identical).  It searches with the scan over the flattened lists: like for like on the Cornell
            box, where it is the default kernel; on the final scene the query walks the tree and the scan is far slower
  default   the same render as the library chooses its kernel

Cases: the book-2 final scene (9) at 1920x1080 (the unified tree) and the Cornell box (6) at 800x800 (light sampling, deep
paths).  One JSON line per case; nothing is gated.

  --case final|cornell|all   --reps N   --warmup N"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.cuda.init()  # torch's HIP runtime first, as in tests/conftest.py

from mort_amd import hip, host  # noqa: E402
from scripts.query_time import primary_rays  # noqa: E402

CASES = {"final": (9, 1920, 1920 / 1080), "cornell": (6, 800, 1.0)}
SEED = 69420


def med(f, reps, warmup):
    t = [f() for _ in range(warmup + reps)][warmup:]
    return dict(ms=float(np.median(t)) * 1e3, ms_min=min(t) * 1e3, ms_max=max(t) * 1e3)


def case(ctx, name, reps, warmup):
    sid, width, aspect = CASES[name]
    dev = torch.device("cuda", 0)
    out = dict(case=name, scene=sid, reps=reps, warmup=warmup)
    for spp in (1, 16):
        world, cam = host.build_scene(sid, width=width, spp=spp, aspect=aspect)
        W, H = cam.image_width, cam.image_height
        n = W * H
        out.update(width=W, height=H, rays=n, bounce_limit=cam.bounce_limit)
        ctx.upload_world(world)
        # the query: the pixels' own streams, restored before every run
        ctx.rng_seed(SEED, W, H)
        seeded = torch.from_numpy(ctx.rng_store(W, H)).to(dev)
        streams = torch.empty_like(seeded)
        rays = primary_rays(cam, dev)
        rgb = torch.zeros(n * 3, dtype=torch.float32, device=dev)
        params = hip.radiance_params_from_camera(cam, samples=spp)

        def query():
            streams.copy_(seeded)
            torch.cuda.synchronize()
            return ctx.query_radiance_device(params, rays, streams, rgb, sync=True)

        q = med(query, reps, warmup)
        # the renders: reseeded before every run
        rgba = torch.zeros(n * 4, dtype=torch.uint8, device=dev)
        accum = torch.zeros(n * 3, dtype=torch.float32, device=dev)
        names = {}

        def render(key):
            ctx.rng_seed(SEED, W, H)
            torch.cuda.synchronize()
            st = ctx.render_device(cam, rgba.data_ptr(), accum.data_ptr())
            names[key] = st["kernel_name"].decode() if isinstance(st["kernel_name"], bytes) else st["kernel_name"]
            return st["seconds"]

        os.environ["MORT_FORCE_GENERIC"] = "1"
        try:
            g = med(lambda: render("generic"), reps, warmup)
        finally:
            del os.environ["MORT_FORCE_GENERIC"]
        d = med(lambda: render("default"), reps, warmup)
        out[f"spp{spp}"] = dict(query=q, generic=g, default=d, generic_kernel=names["generic"], default_kernel=names["default"],
                                query_over_generic=q["ms"] / g["ms"], query_over_default=q["ms"] / d["ms"],
                                mpaths_per_s=n * spp / q["ms"] / 1e3,
                                nan_share=float(torch.isnan(rgb).view(n, 3).any(1).float().mean()),
                                mean_rgb=[float(v) for v in torch.nan_to_num(rgb.view(n, 3)).mean(0) / spp])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=list(CASES) + ["all"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    with hip.Context(0) as ctx:
        for name in (CASES if a.case == "all" else [a.case]):
            case(ctx, name, a.reps, a.warmup)
