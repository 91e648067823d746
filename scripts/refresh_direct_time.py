#!/usr/bin/env python3
"""refresh_direct_time.py -- what a direct-light volume refresh costs beside the plain refresh and the bake of the same probes and
directions, and what its rounds are worth.  The method is refresh_time.py's: one call, HIP-event times from the
calls' own `seconds`, warm, the median of --reps runs after --warmup with min-max; the streams are put back before every run, so each
run does the same work.  Nothing is gated.

  time   two setups: the Cornell box (scene 6) with a --grid^3 (default 8) volume over [20, 535]^3, and the book-2 final scene (9)
         at bounce limit 4 with a 16^3 grid; D = 256, N = 1 and 4 paths per direction.  The yardsticks are measured first, in the
         same run, on code the direct refresh does not touch: mort_hip_volume_refresh_device at K = 0 and K = 1 over the full
         volume, and mort_hip_probe_bake_device + mort_hip_volume_pack_device.  Then mort_hip_volume_refresh_direct_device at K = 0
         and K = 1 over the indirect volume (the full bake minus the emission-only bake), with the shares of its paths that ended in
         the volume and that were lit, and its ratios to the yardsticks with the yardsticks' own spread beside them.
  worth  (--worth; on the host forms alone with --no-gpu) scene 6 at --worth-width^2 (default 96): the direct cached query at K = 0,
         16 paths per pixel-centre ray, against query_radiance_host at --worth-reference (default 1024) paths; relative RMSE
         (the RMSE over the reference's RMS) of the indirect bake alone (D = 256) and of the bake followed by R = 1, 2, 4, 8 direct
         rounds at H = 0.9, K = 0 with the rotated sets; as a control the same rounds through the PLAIN refresh, which puts the
         emitters back.

One JSON line, appended by the caller to profiles/refresh_direct/refresh_direct_time.jsonl."""
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


def cornell_grid(hip, count):
    sp = (BOX[1] - BOX[0]) / (count - 1)
    return hip.VOLUME_GRID((BOX[0],) * 3, (sp,) * 3, (count,) * 3, 0.5)


def final_grid(hip, world, k=16):
    info = hip.debug_gen_reach(world)
    lo, hi = info["lo"].astype(np.float64), info["hi"].astype(np.float64)
    sp = (hi - lo) / k
    return hip.VOLUME_GRID(tuple(lo + 0.5 * sp), tuple(sp), (k,) * 3, 0.5)


def gpu(a, out):
    import torch
    torch.cuda.init()  # torch's HIP runtime first, as in tests/conftest.py
    from mort_amd import hip, host
    dev = torch.device("cuda", 0)

    def med(f):
        t = [f() for _ in range(a.warmup + a.reps)][a.warmup:]
        m = float(np.median(t))
        return dict(ms=m * 1e3, ms_min=min(t) * 1e3, ms_max=max(t) * 1e3, spread=(max(t) - min(t)) / m)

    def t32(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)

    with hip.Context(0) as ctx:
        def time_setup(name):
            sid, limit = (6, None) if name == "cornell" else (9, 4)
            world, cam = host.build_scene(sid, width=64, spp=1)
            if limit is not None:
                cam.bounce_limit = limit
            ctx.upload_world(world)
            g = cornell_grid(hip, a.grid) if name == "cornell" else final_grid(hip, world)
            P = g.probes
            probes_t = torch.from_numpy(hip.volume_probes(g).view(np.float32).copy()).to(dev)
            seeded = t32(hip.seed_states_host(SEED, P * D, 1))
            streams = torch.empty_like(seeded)
            sh = torch.zeros(P * 27, dtype=torch.float32, device=dev)
            sh_e = torch.zeros(P * 27, dtype=torch.float32, device=dev)
            rec = torch.zeros(P * 32, dtype=torch.float32, device=dev)
            rec_ind = torch.zeros(P * 32, dtype=torch.float32, device=dev)
            back = torch.zeros(P * 32, dtype=torch.float32, device=dev)
            ends = torch.zeros(P, dtype=torch.int32, device=dev)
            lit = torch.zeros(P, dtype=torch.int32, device=dev)
            res = dict(setup=name, probes=P, directions=D, bounce_limit=cam.bounce_limit, light=[cam.light_obj_type, cam.light_obj_idx], by_samples={})
            for samples in (1, 4):
                path = hip.radiance_params_from_camera(cam, samples)
                pp = hip.PROBE_PARAMS(path, D)

                def bake():
                    streams.copy_(seeded)
                    torch.cuda.synchronize()
                    return ctx.probe_bake_device(pp, probes_t, streams, sh, sync=True) + ctx.volume_pack_device(sh, rec, sync=True)

                def refresh_case(depth, direct):
                    p = hip.REFRESH_PARAMS(hip.CACHED_PARAMS(path, depth, g, None), D, 0.9, 0, 1)

                    def once():
                        streams.copy_(seeded)
                        torch.cuda.synchronize()
                        if direct:
                            return ctx.volume_refresh_direct_device(p, streams, rec_ind, None, back, ends, lit, sync=True)
                        return ctx.volume_refresh_device(p, streams, rec, None, back, ends, sync=True)

                    t = med(once)
                    t["share_ended"] = float(ends.sum()) / (P * D * samples)
                    if direct:
                        t["share_lit"] = float(lit.sum()) / (P * D * samples)
                    return t

                r = dict(bake=med(bake))  # leaves the baked volume in rec; the yardsticks come first
                r["plain_k0"], r["plain_k1"] = refresh_case(0, False), refresh_case(1, False)
                # the indirect volume: the emission-only bake from the seeded streams, the difference, the pack
                streams.copy_(seeded)
                ctx.probe_bake_device(hip.emission_probe_params(pp), probes_t, streams, sh_e, sync=True)
                ctx.volume_pack_device(sh - sh_e, rec_ind, sync=True)
                for key, depth in (("direct_k0", 0), ("direct_k1", 1)):
                    t = refresh_case(depth, True)
                    t["over_plain"] = t["ms"] / r["plain_" + key[-2:]]["ms"]
                    t["over_bake"] = t["ms"] / r["bake"]["ms"]
                    r[key] = t
                res["by_samples"][str(samples)] = r
            return res

        out.update(reps=a.reps, warmup=a.warmup)
        out["time"] = [time_setup(n) for n in a.setups.split(",") if n]


def worth(a, out):
    """on the host forms alone"""
    from mort_amd import hip, host
    from tests import query_rays as Q
    from tests.feature_ref import primary_rays
    world, cam = host.build_scene(6, width=a.worth_width, spp=1, aspect=1.0)
    g = cornell_grid(hip, a.grid)
    P = g.probes
    probes = hip.volume_probes(g)
    rays = Q.ray8(primary_rays(cam), Q.INF)
    n = len(rays)
    nt = a.threads
    truth = hip.query_radiance_host(world, hip.radiance_params_from_camera(cam, a.worth_reference), rays, hip.seed_states_host(SEED + 1, n, 1), tree=True,
                                    nthreads=nt)["rgb"].astype(np.float64) / a.worth_reference
    rms = float(np.sqrt((truth ** 2).mean()))
    paths = 16
    cp = hip.CACHED_PARAMS(hip.radiance_params_from_camera(cam, paths), 0, g, None)

    def rel_rmse(records):
        got = hip.query_radiance_cached_direct_host(world, cp, rays, hip.seed_states_host(SEED, n, 1), records, None, tree=True, nthreads=nt)
        return float(np.sqrt(((np.nan_to_num(got["rgb"].astype(np.float64)) / paths - truth) ** 2).mean())) / rms

    path = hip.radiance_params_from_camera(cam, 1)
    rp = hip.REFRESH_PARAMS(hip.CACHED_PARAMS(path, 0, g, None), D, 0.9, 0, 1)
    res = dict(width=cam.image_width, paths=paths, reference_paths=a.worth_reference, reference_rms=rms, hysteresis=0.9, refresh_depth=0, directions=D,
               probes=P)
    for kind in ("direct", "plain"):
        st = hip.seed_states_host(SEED, P * D, 1)
        rec = hip.volume_pack_host(hip.probe_bake_indirect_host(world, hip.PROBE_PARAMS(path, D), probes, st, tree=True, nthreads=nt)["sh_ind"])["records"]
        rounds = {"0": dict(rel_rmse=rel_rmse(rec))}
        for r in range(1, 9):
            if kind == "direct":
                got = hip.volume_refresh_direct_host(world, rp, st, rec, dirs=hip.probe_directions_round(D, r), tree=True, nthreads=nt)
            else:
                got = hip.volume_refresh_host(world, rp, st, rec, dirs=hip.probe_directions_round(D, r), tree=True, nthreads=nt)
            rec = got["records"]
            if r in (1, 2, 4, 8):
                rounds[str(r)] = dict(rel_rmse=rel_rmse(rec), share_ended=float(got["ends"].sum()) / (P * D))
                if kind == "direct":
                    rounds[str(r)]["share_lit"] = float(got["lit"].sum()) / (P * D)
        res[kind] = rounds
    out["worth"] = res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--setups", default="cornell,final")
    ap.add_argument("--worth", action="store_true")
    ap.add_argument("--worth-width", type=int, default=96)
    ap.add_argument("--worth-reference", type=int, default=1024)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    out = {}
    if not a.no_gpu:
        gpu(a, out)
    if a.worth:
        worth(a, out)
    print(json.dumps(out), flush=True)
