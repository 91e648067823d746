#!/usr/bin/env python3
"""denoise_time.py -- device time of the feature pass + the a-trous denoiser (default parameters, 5 iterations) on torch tensors,
after warm-up: scene 1 at 1200x675 (the headline geometry) and the book-2 final scene (9) at 4096x4096.  Prints one JSON line per
case with HIP-event times; run under `rocprofv3 --kernel-trace --stats -- python3 scripts/denoise_time.py` for per-kernel figures
(feat_kernel, atrous_kernel).  DESIGN.md 4.9 records the results."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (torch's HIP runtime first, as tests/conftest.py does)

torch.cuda.init()
from mort_amd import hip, host  # noqa: E402


def case(ctx, sid, width, reps=20, warmup=3):
    world, cam = host.build_scene(sid, width=width, spp=4)
    W, H = cam.image_width, cam.image_height
    ctx.upload_world(world)
    ctx.rng_seed(69420, W, H)
    acc = torch.from_numpy(ctx.render(cam, want_accum=True)["accum"].reshape(-1).copy()).cuda()
    alb, nrm, dep = (torch.zeros(W * H * c, dtype=torch.float32, device="cuda") for c in (3, 3, 1))
    out = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
    rgba = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    p = hip.DenoiseParams()
    tf, td = [], []
    for i in range(warmup + reps):
        a = ctx.render_features_device(cam, alb, nrm, dep, sync=True)
        b = ctx.denoise_device(W, H, acc, alb, nrm, dep, accum_out=out, rgba_out=rgba, params=p, sync=True)
        if i >= warmup:
            tf.append(a); td.append(b)
    tf.sort(); td.sort()
    print(json.dumps(dict(scene=sid, width=W, height=H, iterations=p.iterations, features_ms_median=tf[len(tf) // 2] * 1e3,
                          denoise_ms_median=td[len(td) // 2] * 1e3, total_ms_median=(tf[len(tf) // 2] + td[len(td) // 2]) * 1e3,
                          features_ms_min=tf[0] * 1e3, denoise_ms_min=td[0] * 1e3)), flush=True)


if __name__ == "__main__":
    with hip.Context(0) as ctx:
        case(ctx, 1, 1200)
        case(ctx, 9, 4096)
