#!/usr/bin/env python3
"""view_time.py -- what a frame of the whole chain costs, two arms through the same library:

  view    mort_hip_view_frame, temporal + SVGF defaults: the chain stays on the device, one host wait, the uchar4 frame comes back
  chain   the host-buffer stage calls chained as the CLI chained them before the view: mort_hip_render -> mort_hip_render_features
          -> mort_hip_temporal -> mort_hip_svgf, every buffer through host memory, every call blocking

Cases: scene 1 at 1200x675x4 spp with a still camera and with two cameras one `D` apart alternating; the book-2 final scene (9) at
4096x4096x4 spp, still.  Per case and arm: the median over --frames frames after --warmup of the wall time per frame and of the
device time (view: device_seconds; chain: the sum of the four calls' device times), one JSON line per case.  The conditions
printed with it -- every measured view frame faster on the wall clock than the chain's frame of the same index, and no view
frame's device time above the chain's by more than the chain's own spread in this run -- make the exit status.

  --case still|moving|final|all   --arm view|chain|both   --frames N   --warmup N
Run under `rocprofv3 --kernel-trace --stats -- python3 scripts/view_time.py --case still --arm view` (and `--case moving`) for the
kernel table of a view's frames: to check there are the chain's kernels and no others, and one feat_kernel launch per camera
move -- one in all for the still case (profiles/view/)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from mort_amd import hip, host  # noqa: E402
from mort_amd import structs as S  # noqa: E402

CASES = {"still": (1, 1200, False), "moving": (1, 1200, True), "final": (9, 4096, False)}


def cameras(cam, moving, n):
    if not moving:
        return [cam] * n
    other = host.camera_input(S.Camera.from_buffer_copy(cam), "D")
    return [cam if i % 2 == 0 else other for i in range(n)]


def run_view(ctx, cams, W, H):
    wall, dev, parts = [], [], []
    ctx.rng_seed(69420, W, H)
    with ctx.view(W, H) as v:
        for cam in cams:
            t0 = time.perf_counter()
            s = v.frame(cam)["stats"]
            wall.append(time.perf_counter() - t0)
            dev.append(s["device_seconds"])
            parts.append((s["render"]["seconds"], s["features_seconds"], s["temporal_seconds"], s["filter_seconds"]))
    return wall, dev, parts


def run_chain(ctx, cams, W, H):
    """mort.c's frame loop before the view, with the filter on every frame: caller-owned host buffers, reused."""
    L = hip.lib()
    n = W * H
    f32 = lambda k: np.zeros(k, dtype=np.float32)  # noqa: E731
    rgba, accum = np.zeros(n * 4, dtype=np.uint8), f32(n * 3)
    alb, nrm, dep, tacc, tvar = f32(n * 3), f32(n * 3), f32(n), f32(n * 3), f32(n)
    hist = [hip.history_array(W, H), hip.history_array(W, H)]
    tp, sp = hip.TemporalParams(), hip.SvgfParams()
    st, fs, ts, ds = hip.Stats(), C.c_double(0), C.c_double(0), C.c_double(0)
    p = lambda a: a.ctypes.data  # noqa: E731
    wall, dev, parts = [], [], []
    ctx.rng_seed(69420, W, H)
    prev = None
    for f, cam in enumerate(cams):
        t0 = time.perf_counter()
        ctx._chk(L.mort_hip_render(ctx._h, C.byref(cam), hip.MODE_MEGA, p(rgba), p(accum), None, C.byref(st)), "mort_hip_render")
        ctx._chk(L.mort_hip_render_features(ctx._h, C.byref(cam), p(alb), p(nrm), p(dep), C.byref(fs)), "mort_hip_render_features")
        ctx._chk(L.mort_hip_temporal(ctx._h, C.byref(tp), C.byref(prev) if f else None, C.byref(cam), W, H, p(accum), p(nrm), p(dep),
                                     p(hist[(f + 1) & 1]) if f else None, p(hist[f & 1]), p(tacc), p(tvar), p(rgba), C.byref(ts)), "mort_hip_temporal")
        ctx._chk(L.mort_hip_svgf(ctx._h, C.byref(sp), W, H, p(tacc), p(alb), p(nrm), p(dep), p(tvar), None, None, p(rgba), C.byref(ds)), "mort_hip_svgf")
        wall.append(time.perf_counter() - t0)
        dev.append(st.seconds + fs.value + ts.value + ds.value)
        parts.append((st.seconds, fs.value, ts.value, ds.value))
        prev = S.Camera.from_buffer_copy(cam)
    return wall, dev, parts, rgba.copy()


def med(a):
    return float(np.median(a))


def case(ctx, name, arms, frames, warmup):
    sid, width, moving = CASES[name]
    world, cam = host.build_scene(sid, width=width, spp=4)
    W, H = cam.image_width, cam.image_height
    ctx.upload_world(world)
    cams = cameras(cam, moving, warmup + frames)
    out = dict(case=name, scene=sid, width=W, height=H, spp=4, frames=frames, warmup=warmup)
    res = {}
    if "chain" in arms:
        res["chain"] = run_chain(ctx, cams, W, H)[:3]
    if "view" in arms:
        res["view"] = run_view(ctx, cams, W, H)
    for arm, (wall, dev, parts) in res.items():
        wall, dev, parts = wall[warmup:], dev[warmup:], np.array(parts[warmup:])
        res[arm] = (wall, dev)
        out[arm] = dict(wall_ms_median=med(wall) * 1e3, wall_ms_min=min(wall) * 1e3, wall_ms_max=max(wall) * 1e3,
                        device_ms_median=med(dev) * 1e3, device_ms_min=min(dev) * 1e3, device_ms_max=max(dev) * 1e3,
                        render_ms_median=med(parts[:, 0]) * 1e3, features_ms_median=med(parts[:, 1]) * 1e3,
                        temporal_ms_median=med(parts[:, 2]) * 1e3, filter_ms_median=med(parts[:, 3]) * 1e3)
    ok = True
    if len(res) == 2:
        (vw, vd), (cw, cd) = res["view"], res["chain"]
        spread = max(cd) - min(cd)
        out["wall_ratio_chain_over_view"] = med(cw) / med(vw)
        out["device_ratio_view_over_chain"] = med(vd) / med(cd)
        out["chain_device_spread_ms"] = spread * 1e3
        out["every_view_frame_faster_on_the_wall"] = all(a < b for a, b in zip(vw, cw))
        out["no_view_frame_above_chain_device_plus_spread"] = all(a <= b + spread for a, b in zip(vd, cd))
        ok = out["every_view_frame_faster_on_the_wall"] and out["no_view_frame_above_chain_device_plus_spread"]
    print(json.dumps(out), flush=True)
    return ok


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=list(CASES) + ["all"])
    ap.add_argument("--arm", default="both", choices=["view", "chain", "both"])
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    arms = ("view", "chain") if a.arm == "both" else (a.arm,)
    good = True
    with hip.Context(0) as ctx:
        for name in (CASES if a.case == "all" else [a.case]):
            good = case(ctx, name, arms, a.frames, a.warmup) and good
    sys.exit(0 if good else 1)
