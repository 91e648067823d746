#!/usr/bin/env python3
"""query_time.py -- what a batch of ray queries costs beside the feature pass, all through the same library in one
call, HIP-event times of the kernels, the median of --reps runs after --warmup:

  closest   mort_hip_query_closest_device without streams on the feature pass's own primary rays (lens centre through every
            pixel centre, time 0.5, t_max = inf), built on the device with the pass's float32 operations
  features  mort_hip_render_features_device for the same camera: on a tree world the same walk plus a texture fetch, 28 B written
            per pixel against the query's 32 B read and 48 B written
  secondary closest hit and occlusion on the secondary rays: from the hit points of `closest` into directions uniform on the
            sphere, t_max = inf -- what the occlusion kernel's early exit buys

Cases: the book-2 final scene (9) at 4096x4096 (the unified tree) and scene 1 at 1200x675 (a reference BVH: the threaded
reference walk, the known slow path).  One JSON line per case.  For scene 9 the query is expected within 1.5x of the feature
pass; the line says whether it is, and that makes the exit status.

  --case final|scene1|all   --reps N   --warmup N"""
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

CASES = {"final": (9, 4096, 1.5), "scene1": (1, 1200, None)}


def primary_rays(cam, dev):
    """(H * W, 8) float32 on the device: the feature pass's rays, as tests/feature_ref.py primary_rays states them"""
    W, H = cam.image_width, cam.image_height
    v = lambda a: torch.tensor([a.e[0], a.e[1], a.e[2]], dtype=torch.float32, device=dev)  # noqa: E731
    c, p00, du, dv = v(cam.center), v(cam.pixel00_loc), v(cam.pixel_delta_u), v(cam.pixel_delta_v)
    xs = torch.arange(W, dtype=torch.float32, device=dev)[None, :, None]
    ys = torch.arange(H, dtype=torch.float32, device=dev)[:, None, None]
    rays = torch.empty((H, W, 8), dtype=torch.float32, device=dev)
    rays[..., 0:3] = c
    rays[..., 3:6] = ((p00 + xs * du) + ys * dv) - c
    rays[..., 6] = 0.5
    rays[..., 7] = float("inf")
    return rays.reshape(-1, 8)


def med(f, reps, warmup):
    t = [f() for _ in range(warmup + reps)][warmup:]
    return float(np.median(t)) * 1e3, min(t) * 1e3, max(t) * 1e3


def case(ctx, name, reps, warmup):
    sid, width, bar = CASES[name]
    world, cam = host.build_scene(sid, width=width, spp=1)
    W, H = cam.image_width, cam.image_height
    n = W * H
    dev = torch.device("cuda", 0)
    ctx.upload_world(world)
    rays = primary_rays(cam, dev)
    hits = torch.zeros(n * 12, dtype=torch.float32, device=dev)
    occ = torch.zeros(n, dtype=torch.uint8, device=dev)
    alb, nrm, dep = (torch.zeros(n * k, dtype=torch.float32, device=dev) for k in (3, 3, 1))
    torch.cuda.synchronize()
    out = dict(case=name, scene=sid, width=W, height=H, rays=n, reps=reps, warmup=warmup)
    q = med(lambda: ctx.query_closest_device(rays, hits, sync=True), reps, warmup)
    f = med(lambda: ctx.render_features_device(cam, alb, nrm, dep, sync=True), reps, warmup)
    o = med(lambda: ctx.query_occluded_device(rays, occ, sync=True), reps, warmup)
    out.update(closest_ms=q[0], closest_ms_min=q[1], closest_ms_max=q[2], features_ms=f[0], features_ms_min=f[1], features_ms_max=f[2],
               occluded_primary_ms=o[0], closest_over_features=q[0] / f[0], mrays_per_s=n / q[0] / 1e3)
    # the query and the pass must have seen the same thing: depth > 0 where the query hit a solid (the pass also enters media)
    rec = hits.view(n, 12)
    flags = rec[:, 11].view(torch.int32)
    hit = (flags & 1) != 0
    out["hit_share"] = float(hit.float().mean())
    out["solid_hits_without_depth"] = int((hit & (dep == 0)).sum())
    # secondary: from the hit points (a missed ray's from the camera), directions uniform on the sphere
    g = torch.Generator(device=dev).manual_seed(1)
    d = torch.randn((n, 3), generator=g, device=dev)
    sec = torch.empty((n, 8), dtype=torch.float32, device=dev)
    sec[:, 0:3] = torch.where(hit[:, None], rec[:, 0:3], rays[:, 0:3])
    sec[:, 3:6] = d / d.norm(dim=1, keepdim=True)
    sec[:, 6] = 0.5
    sec[:, 7] = float("inf")
    torch.cuda.synchronize()
    q2 = med(lambda: ctx.query_closest_device(sec, hits, sync=True), reps, warmup)
    o2 = med(lambda: ctx.query_occluded_device(sec, occ, sync=True), reps, warmup)
    hit2 = (hits.view(n, 12)[:, 11].view(torch.int32) & 1) != 0
    out.update(secondary_closest_ms=q2[0], secondary_occluded_ms=o2[0], secondary_closest_over_occluded=q2[0] / o2[0],
               secondary_hit_share=float(hit2.float().mean()), secondary_occluded_agrees=bool((hit2 == (occ != 0)).all()))
    ok = out["secondary_occluded_agrees"]
    if bar is not None:
        out["bar"] = bar
        out["within_bar"] = out["closest_over_features"] <= bar
        ok = ok and out["within_bar"]
    print(json.dumps(out), flush=True)
    return ok


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=list(CASES) + ["all"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    good = True
    with hip.Context(0) as ctx:
        for name in (CASES if a.case == "all" else [a.case]):
            good = case(ctx, name, a.reps, a.warmup) and good
    sys.exit(0 if good else 1)
