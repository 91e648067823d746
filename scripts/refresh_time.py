#!/usr/bin/env python3
"""refresh_time.py -- what a volume refresh costs beside the bake of the same probes and directions, and what its rounds are worth
(DESIGN.md 4.21).  HIP-event times from the calls' own `seconds`, warm, the median of --reps runs after --warmup with min-max; the
streams are put back before every run, so each run does the same work.  Nothing is gated.

  time      two setups: the Cornell box (scene 6) with a --grid^3 (default 8) volume over [20, 535]^3, and the book-2 final scene (9)
            at bounce limit 4 with a 16^3 grid of cell centres in the solids' box; D = 256, N = 1 and 4 paths per direction.  The
            yardstick is mort_hip_probe_bake_device + mort_hip_volume_pack_device on the same probes, directions and streams.  Cases:
            the refresh at K = bounce limit (the bake's own paths plus the blend; expected within the bake's run-to-run spread, floor
            3 %), and at K = 0, 1, 2 with and without visibility, each with the share of its paths that ended in the volume (the
            kernel's own counts).
  segments  the mean segments per path of the same cases from the walk of tests/cached_ref.py over the oracle, on the host alone,
            for every (probes / --segment-probes)-th probe of the Cornell setup (0 leaves the walk out).
  worth     scene 6 at --worth-width^2 (default 256): the picture of `mort --irradiance-out` -- sqrt(clamp(E / pi, 0, 1)) at every
            pixel-centre ray's hit -- from the 8^3 volume baked at D = 4096, N = 16 as the reference; RMSE against it of (a) the plain
            D = 256, N = 1 bake and (b) that bake followed by R = 1, 2, 4, 8 rounds at K = 0, H = 0.9 with the rotated sets, with the
            total device milliseconds of each.

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
D = 256
CASES = (("k0", 0, False), ("k1", 1, False), ("k2", 2, False), ("k0_visible", 0, True), ("k1_visible", 1, True), ("k2_visible", 2, True))


def cornell_grid(hip, count):
    sp = (BOX[1] - BOX[0]) / (count - 1)
    return hip.VOLUME_GRID((BOX[0],) * 3, (sp,) * 3, (count,) * 3, 0.5)


def final_grid(hip, world, k=16):
    info = hip.debug_gen_reach(world)
    lo, hi = info["lo"].astype(np.float64), info["hi"].astype(np.float64)
    sp = (hi - lo) / k
    return hip.VOLUME_GRID(tuple(lo + 0.5 * sp), tuple(sp), (k,) * 3, 0.5)


def cap_of(g):
    return float(np.float32(1.5 * np.sqrt(sum(float(s) ** 2 for s in g.spacing))))


def segments(a, out):
    """the walk over the oracle, on the host alone: the volume baked by the host forms (bit for bit the device's)"""
    from mort_amd import hip, host
    from tests import cached_ref as CR
    from tests import oracle_lib as O
    from tests import probe_ref as PR
    from tests import refresh_ref as RR
    world, cam = host.build_scene(6, width=64, spp=1)
    g = cornell_grid(hip, a.grid)
    probes = hip.volume_probes(g)
    path = hip.radiance_params_from_camera(cam, 1)
    sh = hip.probe_bake_host(world, hip.PROBE_PARAMS(path, D), probes, O.seed_states(SEED, g.probes * D, 1), tree=True, nthreads=16)["sh"]
    rec = hip.volume_pack_host(sh)["records"]
    maps = hip.probe_depth_bake_host(world, hip.DEPTH_PARAMS(2, cap_of(g)), probes, tree=True, nthreads=16)["depth"]
    step = max(1, g.probes // a.segment_probes)
    sel = np.arange(0, g.probes, step)
    rays = PR.rays_of(RR.positions(g)[sel], hip.probe_directions(D))
    seg = {}
    for key, depth, vis in (("bake", path.bounce_limit, False),) + CASES:
        v = (a.bias, 0.05) if vis else None
        _, ends, cen = CR.walk(world, path, depth, g, rec, maps if vis else None, v, rays, O.seed_states(SEED, len(rays), 1))
        seg[key] = dict(mean_segments=cen["segments"] / cen["paths"], share_ended=float(ends.sum()) / cen["paths"])
    out["segments"] = dict(probes=len(sel), directions=D, samples=1, **seg)


def gpu(a, out):
    import torch
    torch.cuda.init()  # torch's HIP runtime first, as in tests/conftest.py
    from mort_amd import hip, host
    from tests import query_rays as Q
    from tests.feature_ref import primary_rays
    dev = torch.device("cuda", 0)

    def med(f, reps=None, warmup=None):
        reps, warmup = a.reps if reps is None else reps, a.warmup if warmup is None else warmup
        t = [f() for _ in range(warmup + reps)][warmup:]
        m = float(np.median(t))
        return dict(ms=m * 1e3, ms_min=min(t) * 1e3, ms_max=max(t) * 1e3, spread=(max(t) - min(t)) / m)

    def t32(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)

    with hip.Context(0) as ctx:
        def setup(name):
            sid, limit = (6, None) if name == "cornell" else (9, 4)
            world, cam = host.build_scene(sid, width=64, spp=1)
            if limit is not None:
                cam.bounce_limit = limit
            ctx.upload_world(world)
            g = cornell_grid(hip, a.grid) if name == "cornell" else final_grid(hip, world)
            return world, cam, g

        def time_setup(name):
            world, cam, g = setup(name)
            P = g.probes
            probes = hip.volume_probes(g)
            probes_t = torch.from_numpy(probes.view(np.float32).copy()).to(dev)
            seeded = t32(hip.seed_states_host(SEED, P * D, 1))
            streams = torch.empty_like(seeded)
            sh = torch.zeros(P * 27, dtype=torch.float32, device=dev)
            rec = torch.zeros(P * 32, dtype=torch.float32, device=dev)
            back = torch.zeros(P * 32, dtype=torch.float32, device=dev)
            ends = torch.zeros(P, dtype=torch.int32, device=dev)
            maps = t32(ctx.probe_depth_bake(hip.DEPTH_PARAMS(2, cap_of(g)), probes)["depth"])
            vis = hip.VOLUME_VIS_PARAMS(a.bias if name == "cornell" else 0.05 * min(g.spacing), 0.05)
            res = dict(setup=name, probes=P, directions=D, bounce_limit=cam.bounce_limit, by_samples={})
            for samples in (1, 4):
                path = hip.radiance_params_from_camera(cam, samples)
                pp = hip.PROBE_PARAMS(path, D)

                def bake():
                    streams.copy_(seeded)
                    torch.cuda.synchronize()
                    return ctx.probe_bake_device(pp, probes_t, streams, sh, sync=True) + ctx.volume_pack_device(sh, rec, sync=True)

                r = dict(bake=med(bake))  # leaves the baked volume in rec
                margin = max(r["bake"]["spread"], 0.03)

                def refresh_case(depth, visible):
                    p = hip.REFRESH_PARAMS(hip.CACHED_PARAMS(path, depth, g, vis if visible else None), D, 0.9, 0, 1)

                    def once():
                        streams.copy_(seeded)
                        torch.cuda.synchronize()
                        return ctx.volume_refresh_device(p, streams, rec, maps if visible else None, back, ends, sync=True)

                    t = med(once)
                    t["over_bake"] = t["ms"] / r["bake"]["ms"]
                    t["share_ended"] = float(ends.sum()) / (P * D * samples)
                    return t

                r["k_limit"] = refresh_case(cam.bounce_limit, False)
                r["k_limit"]["margin"] = margin
                r["k_limit"]["within_margin"] = bool(r["k_limit"]["over_bake"] <= 1.0 + margin)
                for key, depth, visible in CASES:
                    r[key] = refresh_case(depth, visible)
                res["by_samples"][str(samples)] = r
            return res

        out.update(reps=a.reps, warmup=a.warmup)
        out["time"] = [time_setup(n) for n in a.setups.split(",") if n]

        # ---- worth
        if a.worth_width > 0:
            world, _, g = setup("cornell")
            _, cam = host.build_scene(6, width=a.worth_width, spp=1, aspect=1.0)
            P = g.probes
            probes = hip.volume_probes(g)
            hits = ctx.query_closest(Q.ray8(primary_rays(cam), Q.INF))["hits"]
            hit = ((hits["flags"] & hip.HIT_HIT) != 0)[:, None]

            def picture(records):
                e = ctx.volume_sample(g, records, hits)["out"][:, :3]
                v = np.where(hit, e, 0.0).astype(np.float64) / np.pi
                return np.sqrt(np.clip(np.nan_to_num(v), 0.0, 1.0))

            def baked(directions, samples):
                path = hip.radiance_params_from_camera(cam, samples)
                st = hip.seed_states_host(SEED, P * directions, 1)
                b = ctx.probe_bake(hip.PROBE_PARAMS(path, directions), probes, st)
                k = ctx.volume_pack(b["sh"])
                return k["records"], st, (b["seconds"] + k["seconds"]) * 1e3

            truth = picture(baked(4096, 16)[0])
            rec, st, ms = baked(D, 1)
            rmse = lambda r: float(np.sqrt(((picture(r) - truth) ** 2).mean()))  # noqa: E731
            worth = dict(width=cam.image_width, reference=dict(directions=4096, samples=16), hysteresis=0.9, refresh_depth=0,
                         rounds={"0": dict(rmse=rmse(rec), device_ms=ms)})
            path = hip.radiance_params_from_camera(cam, 1)
            p = hip.REFRESH_PARAMS(hip.CACHED_PARAMS(path, 0, g, None), D, 0.9, 0, 1)
            for r in range(1, 9):
                got = ctx.volume_refresh(p, st, rec, dirs=hip.probe_directions_round(D, r))
                rec, ms = got["records"], ms + got["seconds"] * 1e3
                if r in (1, 2, 4, 8):
                    worth["rounds"][str(r)] = dict(rmse=rmse(rec), device_ms=ms, share_ended=float(got["ends"].sum()) / (P * D))
            out["worth"] = worth


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--bias", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--setups", default="cornell,final")
    ap.add_argument("--worth-width", type=int, default=256)
    ap.add_argument("--segment-probes", type=int, default=64)
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    out = {}
    if a.segment_probes > 0:
        segments(a, out)
    if not a.no_gpu:
        gpu(a, out)
    print(json.dumps(out), flush=True)
