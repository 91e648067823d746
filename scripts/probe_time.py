#!/usr/bin/env python3
"""probe_time.py -- what a bake of light probes costs beside the radiance query of the same paths, through the same
library in one run, HIP-event times of the kernels, the median of --reps runs after --warmup with their minimum and maximum:

  bake    mort_hip_probe_bake_device: 4096 probes on a regular 16 x 16 x 16 grid (cell centres) inside the solids' box, time 0.5,
          D = 256 directions of the library's set, samples = 1 and samples = 4; the streams are put back before every run, so
          each run does the same work
  query   mort_hip_query_radiance_device on the identical n D rays in probe-major order with identical streams: the way to the
          same paths without this feature.  Its figure leaves out what that way needs besides: building the rays on the host,
          the 12 bytes per ray copied back and the caller's projection

Frames: the book-2 final scene (9) at bounce limit 4 and the Cornell box (6) at its own limit.  One JSON line per frame with the
two medians, the spreads (max - min) / median, the ratio bake / query and the margin the ratio is held against: the query's own
spread with a floor of 3 %.  Nothing is gated; the final streams of the two ways are compared as a check that they ran the same paths.

  --case final|cornell|all   --reps N   --warmup N   --probes-per-axis K"""
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

CASES = {"final": (9, 4), "cornell": (6, None)}
SEED = 69420
D = 256


def med(f, reps, warmup):
    t = [f() for _ in range(warmup + reps)][warmup:]
    m = float(np.median(t))
    return dict(ms=m * 1e3, ms_min=min(t) * 1e3, ms_max=max(t) * 1e3, spread=(max(t) - min(t)) / m)


def grid_probes(world, k):
    info = hip.debug_gen_reach(world)
    lo, hi = info["lo"].astype(np.float64), info["hi"].astype(np.float64)
    t = (np.arange(k) + 0.5) / k
    x, y, z = np.meshgrid(*(lo[a] + t * (hi[a] - lo[a]) for a in range(3)), indexing="ij")
    p = np.zeros(k ** 3, dtype=hip.PROBE_DTYPE)
    p["position"] = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float32)
    p["time"] = 0.5
    return p, bool(info["tree"])


def case(ctx, name, reps, warmup, k):
    sid, limit = CASES[name]
    dev = torch.device("cuda", 0)
    world, cam = host.build_scene(sid, width=64, spp=1)
    if limit is not None:
        cam.bounce_limit = limit
    ctx.upload_world(world)
    probes, tree = grid_probes(world, k)
    n = len(probes)
    dirs = hip.probe_directions(D)
    rays = np.zeros((n, D, 8), dtype=np.float32)
    rays[:, :, 0:3] = probes["position"][:, None, :]
    rays[:, :, 3:6] = dirs[None, :, :]
    rays[:, :, 6] = 0.5
    rays[:, :, 7] = np.inf
    seeded = torch.from_numpy(hip.seed_states_host(SEED, D, n).view(np.uint8).reshape(-1)).to(dev)  # stream p D + j: subsequence p D + j
    streams = torch.empty_like(seeded)
    rays_t = torch.from_numpy(rays.reshape(-1)).to(dev)
    probes_t = torch.from_numpy(probes.view(np.float32).copy()).to(dev)
    rgb = torch.zeros(n * D * 3, dtype=torch.float32, device=dev)
    sh = torch.zeros(n * 27, dtype=torch.float32, device=dev)
    out = dict(case=name, scene=sid, bounce_limit=cam.bounce_limit, probes=n, directions=D, rays=n * D, unified_tree=tree, reps=reps, warmup=warmup)
    for samples in (1, 4):
        pp = hip.probe_params_from_camera(cam, D, samples)
        rp = hip.radiance_params_from_camera(cam, samples)

        def bake():
            streams.copy_(seeded)
            torch.cuda.synchronize()
            return ctx.probe_bake_device(pp, probes_t, streams, sh, sync=True)

        def query():
            streams.copy_(seeded)
            torch.cuda.synchronize()
            return ctx.query_radiance_device(rp, rays_t, streams, rgb, sync=True)

        q = med(query, reps, warmup)
        after_query = streams.clone()
        b = med(bake, reps, warmup)
        same = bool((streams == after_query).all())
        margin = max(q["spread"], 0.03)
        ratio = b["ms"] / q["ms"]
        out[f"samples{samples}"] = dict(bake=b, query=q, ratio=ratio, margin=margin, within_margin=bool(ratio <= 1.0 + margin), same_final_streams=same,
                                        mpaths_per_s=n * D * samples / b["ms"] / 1e3, nan_coefficients=int(torch.isnan(sh).sum()),
                                        mean_c0=[float(v) for v in sh.view(n, 9, 3)[:, 0].nanmean(0)])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=list(CASES) + ["all"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--probes-per-axis", type=int, default=16)
    a = ap.parse_args()
    with hip.Context(0) as ctx:
        for name in (CASES if a.case == "all" else [a.case]):
            case(ctx, name, a.reps, a.warmup, a.probes_per_axis)
