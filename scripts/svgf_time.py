#!/usr/bin/env python3
"""svgf_time.py -- device time of the feature pass + the SVGF filter stage (default parameters) on torch tensors, after warm-up:
scene 1 at 1200x675 (the headline geometry) and the book-2 final scene (9) at 4096x4096, with the taps of the prepare pass and of
iterations 0 / 1 read as the library does by default, all from LDS tiles and all from global memory (MORT_SVGF_TAPS), with and without a temporal variance, beside the
a-trous denoiser (5 iterations) on the same buffers.  Prints one JSON line per case with HIP-event times (median of 20); run under
`rocprofv3 --kernel-trace --stats -- python3 scripts/svgf_time.py` for per-kernel figures (svgf_prep_kernel, svgf_iter_kernel,
atrous_kernel).  `--five` adds the five-iteration chain.  DESIGN.md 4.11 records the results."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (torch's HIP runtime first, as tests/conftest.py does)

torch.cuda.init()
from mort_amd import hip, host  # noqa: E402


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def case(ctx, sid, width, reps=20, warmup=3, five=False):
    world, cam = host.build_scene(sid, width=width, spp=4)
    W, H = cam.image_width, cam.image_height
    ctx.upload_world(world)
    ctx.rng_seed(69420, W, H)
    n = W * H
    alb, nrm, dep = (torch.zeros(n * c, dtype=torch.float32, device="cuda") for c in (3, 3, 1))
    hist = [torch.zeros(n * hip.TEMPORAL_HISTORY_FLOATS, dtype=torch.float32, device="cuda") for _ in range(2)]
    acc, var = torch.zeros(n * 3, dtype=torch.float32, device="cuda"), torch.zeros(n, dtype=torch.float32, device="cuda")
    ctx.render_features_device(cam, alb, nrm, dep, sync=True)
    for f in range(2):  # two still frames: the second step knows a variance everywhere
        fr = torch.from_numpy(ctx.render(cam, want_accum=True)["accum"].reshape(-1).copy()).cuda()
        ctx.temporal_device(cam if f else None, cam, fr, nrm, dep, hist[1 - f] if f else None, hist[f], accum_out=acc, variance_out=var, sync=True)
    out = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
    vout = torch.zeros(n, dtype=torch.float32, device="cuda")
    rgba = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
    row = dict(scene=sid, width=W, height=H)
    tf = []
    for i in range(warmup + reps):
        t = ctx.render_features_device(cam, alb, nrm, dep, sync=True)
        if i >= warmup:
            tf.append(t)
    row["features_ms"] = median(tf) * 1e3
    dp = hip.DenoiseParams()
    td = []
    for i in range(warmup + reps):
        t = ctx.denoise_device(W, H, acc, alb, nrm, dep, accum_out=out, rgba_out=rgba, params=dp, sync=True)
        if i >= warmup:
            td.append(t)
    row[f"denoise_{dp.iterations}it_ms"] = median(td) * 1e3
    for its in ([hip.SvgfParams().iterations] + ([5] if five else [])):
        p = hip.SvgfParams(iterations=its)
        for taps in ("default", "lds", "global"):
            os.environ.pop("MORT_SVGF_TAPS", None)
            if taps != "default":
                os.environ["MORT_SVGF_TAPS"] = taps
            for name, v in (("var", var), ("novar", None)):
                ts = []
                for i in range(warmup + reps):
                    t = ctx.svgf_device(W, H, acc, alb, nrm, dep, variance=v, accum_out=out, variance_out=vout, rgba_out=rgba, params=p, sync=True)
                    if i >= warmup:
                        ts.append(t)
                row[f"svgf_{its}it_{taps}_{name}_ms"] = median(ts) * 1e3
    os.environ.pop("MORT_SVGF_TAPS", None)
    its = hip.SvgfParams().iterations
    row["features_plus_svgf_ms"] = row["features_ms"] + row[f"svgf_{its}it_default_var_ms"]
    row["features_plus_svgf_novar_ms"] = row["features_ms"] + row[f"svgf_{its}it_default_novar_ms"]
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    with hip.Context(0) as ctx:
        case(ctx, 1, 1200, five="--five" in sys.argv)
        case(ctx, 9, 4096, five="--five" in sys.argv)
