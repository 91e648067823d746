#!/usr/bin/env python3
"""volume_time.py -- what sampling an irradiance volume costs, HIP-event times of volume_sample_kernel, the
median of --reps runs after --warmup with their minimum and maximum.

The volume: a 16 x 16 x 16 grid over the Cornell box (scene 6), baked on the GPU (D = 64, bounce limit 4), packed with all weights
1: 4096 records, 512 KB.  Two batches of 2^20 points:

  coherent     the first hits of a 1024 x 1024 frame of the scene's --pick rays (lens centre through the pixel centre), at stride
               48 straight from mort_hip_query_closest_device's output tensor: neighbouring lanes share their eight probes
  incoherent   uniform random points in the grid's box with random unit normals, at stride 24: every lane its own eight probes

There is nothing in the parent to compare with, so each batch's time is reported with its minimum traffic -- n (stride + 16) +
128 probes bytes: every point record read once (whole records at stride 48: the lines are fetched whole), every output written
once, every probe record read once -- and that traffic's rate as a share of Context.calib_hbm_copy measured in the same process.
Nothing is gated.  One JSON line per batch.

The visibility-weighted sampler is timed beside the plain one in the same process, on the same two batches: the
depth maps of the same grid are baked first (s = 2, max_distance 1.5 cell diagonals, reported in rays per second: 64 s^2 per
probe), then volume_sample_visible_kernel runs with normal_bias 5 and min_visibility 0.05.  Each batch's line gains the visible
sampler's times under "visible", its ratio to the plain sampler and its extra minimum traffic, 800 bytes per probe.

  --reps N   --warmup N   --probes-per-axis K   --width W"""
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

SEED = 69420
D = 64
F = np.float32


def med(f, reps, warmup):
    t = [f() for _ in range(warmup + reps)][warmup:]
    m = float(np.median(t))
    return dict(ms=m * 1e3, ms_min=min(t) * 1e3, ms_max=max(t) * 1e3, spread=(max(t) - min(t)) / m, runs_ms=[v * 1e3 for v in t])


def pick_rays(cam):
    """the feature pass's primary rays, float32 (H W, 8): origin the lens centre, direction through the pixel centre, time 0.5, t_max inf"""
    W, H = cam.image_width, cam.image_height
    v = lambda e: np.array([e.e[0], e.e[1], e.e[2]], dtype=F)  # noqa: E731
    c, p00, du, dv = v(cam.center), v(cam.pixel00_loc), v(cam.pixel_delta_u), v(cam.pixel_delta_v)
    xs = np.arange(W, dtype=F)[None, :, None]
    ys = np.arange(H, dtype=F)[:, None, None]
    rays = np.empty((H, W, 8), dtype=F)
    rays[..., 0:3] = c
    rays[..., 3:6] = ((p00 + xs * du) + ys * dv) - c
    rays[..., 6] = 0.5
    rays[..., 7] = np.inf
    return rays.reshape(-1, 8)


def main(a):
    dev = torch.device("cuda", 0)
    k = a.probes_per_axis
    world, cam = host.build_scene(6, width=a.width, spp=1)
    cam.bounce_limit = 4
    lo, hi = 5.0, 550.0  # inside the walls of the 555-unit box
    grid = hip.VOLUME_GRID((lo, lo, lo), ((hi - lo) / (k - 1),) * 3, (k, k, k), 0.5)
    with hip.Context(0) as ctx:
        ctx.upload_world(world)
        copy_gbs = ctx.calib_hbm_copy()
        # bake and pack on the device
        probes_t = torch.from_numpy(hip.volume_probes(grid).view(F).copy()).to(dev)
        streams = torch.from_numpy(hip.seed_states_host(SEED, D, grid.probes).view(np.uint8).reshape(-1)).to(dev)
        sh = torch.zeros(grid.probes * 27, dtype=torch.float32, device=dev)
        records = torch.zeros(grid.probes * 32, dtype=torch.float32, device=dev)
        bake_s = ctx.probe_bake_device(hip.probe_params_from_camera(cam, D), probes_t, streams, sh, sync=True)
        pack_s = ctx.volume_pack_device(sh, records, sync=True)
        # the depth maps of the same probes
        dparams = hip.DEPTH_PARAMS(2, float(F(1.5 * np.sqrt(3.0) * float(grid.spacing[0]))))
        depth = torch.zeros(grid.probes * hip.DEPTH_FLOATS, dtype=torch.float32, device=dev)
        db = med(lambda: ctx.probe_depth_bake_device(dparams, probes_t, depth, sync=True), a.reps, a.warmup)
        depth_rays = grid.probes * 64 * dparams.subsamples ** 2
        vparams = hip.VOLUME_VIS_PARAMS(5.0, 0.05)
        # coherent: the frame's hits, never copied
        rays = pick_rays(cam)
        n = len(rays)
        rays_t = torch.from_numpy(rays.reshape(-1)).to(dev)
        hits_t = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
        query_s = ctx.query_closest_device(rays_t, hits_t, sync=True)
        # incoherent: random points in the box
        rng = np.random.default_rng(5)
        pts = np.empty((n, 6), dtype=F)
        pts[:, :3] = rng.uniform(lo, hi, size=(n, 3))
        d = rng.normal(size=(n, 3))
        pts[:, 3:] = d / np.linalg.norm(d, axis=1, keepdims=True)
        pts_t = torch.from_numpy(pts.reshape(-1)).to(dev)
        out = torch.zeros(n * 4, dtype=torch.float32, device=dev)
        base = dict(probes=grid.probes, record_bytes=grid.probes * 128, points=n, reps=a.reps, warmup=a.warmup, calib_hbm_copy_gbs=copy_gbs,
                    bake_ms=bake_s * 1e3, pack_ms=pack_s * 1e3, query_closest_ms=query_s * 1e3,
                    depth_bake=dict(subsamples=dparams.subsamples, max_distance=dparams.max_distance, rays=depth_rays, ms=db["ms"], ms_min=db["ms_min"],
                                    ms_max=db["ms_max"], mrays_per_s=depth_rays / db["ms"] / 1e3, map_bytes=grid.probes * 800))
        for name, t, stride in (("coherent", hits_t, 48), ("incoherent", pts_t, 24)):
            r = med(lambda: ctx.volume_sample_device(grid, records, t, out, stride=stride, sync=True), a.reps, a.warmup)
            o = out.view(n, 4)
            plain_out = out.clone()
            v = med(lambda: ctx.volume_sample_visible_device(grid, records, depth, vparams, t, out, stride=stride, sync=True), a.reps, a.warmup)
            changed = float((out.view(n, 4) != plain_out.view(n, 4)).any(1).float().mean())
            visible = dict(ms=v["ms"], ms_min=v["ms_min"], ms_max=v["ms_max"], spread=v["spread"], runs_ms=v["runs_ms"], ratio_to_plain=v["ms"] / r["ms"],
                           extra_min_traffic_bytes=800 * grid.probes, points_changed=changed, normal_bias=vparams.normal_bias,
                           min_visibility=vparams.min_visibility)
            o = plain_out.view(n, 4)
            traffic = n * (stride + 16) + 128 * grid.probes
            gbs = traffic / (r["ms"] * 1e-3) / 1e9
            print(json.dumps(dict(base, batch=name, stride=stride, **r, min_traffic_bytes=traffic, min_traffic_gbs=gbs, share_of_copy=gbs / copy_gbs, visible=visible,
                                  mpoints_per_s=n / r["ms"] / 1e3, covered=float((o[:, 3] > 0).float().mean()),
                                  mean_irradiance=[float(v) for v in o[:, :3].nanmean(0)])), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--probes-per-axis", type=int, default=16)
    ap.add_argument("--width", type=int, default=1024)
    main(ap.parse_args())
