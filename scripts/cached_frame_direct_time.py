#!/usr/bin/env python3
"""cached_frame_direct_time.py -- what a direct-light cached frame costs beside the cached frame and the plain render
of the same frame, and what its picture is worth.  Nothing is gated.

  time      (GPU) the Cornell box (scene 6), --width^2 pixels (default 1024), --spp samples (default 4): section 4.20's frame.
            --grid^3 probes (default 8) over [20, 535]^3 baked on the device (D = 256, one path per direction; the full and the
            indirect volume, depth maps with 2 x 2 rays per texel).  HIP-event times from the calls' own statistics, warm, the
            median of --reps after --warmup with min and max; the pixel streams are seeded anew before every run.  The yardsticks
            first -- render_cached_device at K = 0 and K = 1 on the full volume and render_device in MODE_MEGA -- then
            render_cached_direct_device on the indirect volume at K = 0 and K = 1, with and without visibility: ms, the ratio to each
            yardstick, mean segments per path (shadow segments included), the shares of paths that ended in the volume and of those
            that were lit, from the frame's own counts (which the tests hold to the reference's).
  census    (CPU; --census) the same three columns from the walk of tests/cached_frame_direct_ref.py over the oracle, at
            --census-width^2 pixels (default 64) of that frame and D = 64.
  worth     (CPU, host forms; --worth) scene 6 at --worth-width^2 (default 96), 16 spp: the relative RMSE of the accumulators
            against render_host at 1024 spp -- sqrt(sum (x - t)^2 / sum t^2) over pixels and channels -- for the plain render, the
            cached frame at K = 0 and K = 1 on the full volume, the direct frame at K = 0 and K = 1 on the indirect volume and, as
            a control that counts direct light twice, the direct frame at K = 0 on the full volume.

One JSON line, also appended to --out.   --no-gpu: without the times."""
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


def census(a, out):
    from mort_amd import hip, host
    from tests import cached_frame_direct_ref as DR
    from tests import oracle_lib as O
    world, cam = host.build_scene(6, width=a.census_width, spp=a.spp, aspect=1.0)
    W, H = cam.image_width, cam.image_height
    g = grid_of(hip, a.grid)
    rec, maps = host_volumes(world, cam, g, 64)
    res = dict(width=W, spp=cam.sqrt_spp ** 2, directions=64)
    for key, depth, vis in (("direct_k0", 0, None), ("direct_k1", 1, None), ("direct_k0_visible", 0, (a.bias, 0.05)), ("direct_k1_visible", 1, (a.bias, 0.05))):
        f = DR.frame(world, cam, depth, g, rec["ind"], maps if vis else None, vis, O.seed_states(SEED, W, H))
        c = f["census"]
        res[key] = dict(mean_segments=f["segments"] / c["paths"], share_ended=c["ended"] / c["paths"], share_lit=c["lit"] / max(1, c["ended"]))
    out["census"] = res


def worth(a, out):
    from mort_amd import hip, host
    world, cam = host.build_scene(6, width=a.worth_width, spp=16, aspect=1.0)
    _, truth_cam = host.build_scene(6, width=a.worth_width, spp=1024, aspect=1.0)
    g = grid_of(hip, a.grid)
    rec, _ = host_volumes(world, cam, g, 256)
    truth = hip.render_host(world, truth_cam, seed=SEED + 1, tree=True, nthreads=THREADS)["accum"].astype(np.float64)

    def err(r):
        x = np.nan_to_num(r["accum"].astype(np.float64))
        return float(np.sqrt(((x - truth) ** 2).sum() / (truth ** 2).sum()))

    res = dict(width=cam.image_width, truth_spp=1024, spp=cam.sqrt_spp ** 2, probes=g.probes, directions=256)
    res["plain"] = err(hip.render_host(world, cam, seed=SEED, tree=True, nthreads=THREADS))
    for k in (0, 1):
        p = hip.CACHED_FRAME_PARAMS(k, g, None)
        res[f"cached_k{k}_full"] = err(hip.render_cached_host(world, cam, p, rec["full"], seed=SEED, tree=True, nthreads=THREADS))
        d = hip.render_cached_direct_host(world, cam, p, rec["ind"], seed=SEED, tree=True, nthreads=THREADS)
        res[f"direct_k{k}_indirect"] = err(d)
        res[f"direct_k{k}_share_lit"] = float(d["lit_px"].sum()) / max(1, int(d["ends_px"].sum()))
    p = hip.CACHED_FRAME_PARAMS(0, g, None)
    res["direct_k0_full_control"] = err(hip.render_cached_direct_host(world, cam, p, rec["full"], seed=SEED, tree=True, nthreads=THREADS))
    out["worth"] = res


def gpu(a, out):
    import torch
    torch.cuda.init()  # torch's HIP runtime first, as in tests/conftest.py
    from mort_amd import hip, host
    dev = torch.device("cuda", 0)

    def med(f):
        r = [f() for _ in range(a.warmup + a.reps)][a.warmup:]
        t = [x["seconds"] for x in r]
        return dict(ms=float(np.median(t)) * 1e3, ms_min=min(t) * 1e3, ms_max=max(t) * 1e3), r[-1]

    with hip.Context(0) as ctx:
        world, cam = host.build_scene(6, width=a.width, spp=a.spp, aspect=1.0)
        W, H = cam.image_width, cam.image_height
        n, spp = W * H, cam.sqrt_spp ** 2
        ctx.upload_world(world)
        g = grid_of(hip, a.grid)
        probes = hip.volume_probes(g)
        D = 256
        bake = ctx.probe_bake_indirect(hip.probe_params_from_camera(cam, D), probes, hip.seed_states_host(SEED, g.probes * D, 1))
        rec = {k: torch.from_numpy(ctx.volume_pack(bake["sh_" + k])["records"]).to(dev) for k in ("full", "ind")}
        maps = torch.from_numpy(ctx.probe_depth_bake(hip.DEPTH_PARAMS(2, cap_of(g)), probes)["depth"]).to(dev)
        out.update(width=W, height=H, spp=spp, bounce_limit=cam.bounce_limit, reps=a.reps, warmup=a.warmup, probes=g.probes, directions=D,
                   bake_ms=bake["seconds"] * 1e3)
        rgba = torch.zeros(n * 4, dtype=torch.uint8, device=dev)
        accum = torch.zeros(n * 3, dtype=torch.float32, device=dev)
        ends = torch.zeros(n, dtype=torch.int32, device=dev)
        lit = torch.zeros(n, dtype=torch.int32, device=dev)
        vis = hip.VOLUME_VIS_PARAMS(a.bias, 0.05)

        def plain():
            ctx.rng_seed(SEED, W, H)
            return ctx.render_device(cam, rgba.data_ptr(), accum.data_ptr(), mode=hip.MODE_MEGA, sync=True)

        def cached(depth):
            p = hip.CACHED_FRAME_PARAMS(depth, g, None)

            def once():
                ctx.rng_seed(SEED, W, H)
                return ctx.render_cached_device(cam, p, rec["full"], None, rgba, accum, ends, sync=True)
            return once

        def direct(depth, visible):
            p = hip.CACHED_FRAME_PARAMS(depth, g, vis if visible else None)

            def once():
                ctx.rng_seed(SEED, W, H)
                return ctx.render_cached_direct_device(cam, p, rec["ind"], maps if visible else None, rgba, accum, ends, lit, sync=True)
            return once

        times = {}
        # the yardsticks first, in the same run
        for key, f in (("cached_k0", cached(0)), ("cached_k1", cached(1)), ("render_mega", plain)):
            t, st = med(f)
            t.update(kernel=st["kernel_name"], mean_segments=st["segments"] / (n * spp))
            if key != "render_mega":
                t.update(share_ended=float(ends.sum()) / (n * spp))
            times[key] = t
        for key, depth, visible in (("direct_k0", 0, False), ("direct_k1", 1, False), ("direct_k0_visible", 0, True), ("direct_k1_visible", 1, True)):
            t, st = med(direct(depth, visible))
            ended = float(ends.sum())
            t.update(kernel=st["kernel_name"], vgprs=st["kernel_vgprs"], lds_bytes=st["kernel_lds_bytes"], mean_segments=st["segments"] / (n * spp),
                     share_ended=ended / (n * spp), share_lit=float(lit.sum()) / max(1.0, ended))
            for y in ("cached_k0", "cached_k1", "render_mega"):
                t["over_" + y] = t["ms"] / times[y]["ms"]
            times[key] = t
        out["times"] = times


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--bias", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--census", action="store_true")
    ap.add_argument("--census-width", type=int, default=64)
    ap.add_argument("--worth", action="store_true")
    ap.add_argument("--worth-width", type=int, default=96)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cached_frame_direct", "cached_frame_direct_time.jsonl"))
    a = ap.parse_args()
    out = {}
    if not a.no_gpu:
        gpu(a, out)
    if a.census:
        census(a, out)
    if a.worth:
        worth(a, out)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
