#!/usr/bin/env python3
"""temporal_time.py -- device time of the feature pass + one temporal step (default parameters) on torch tensors, after warm-up:
scene 1 at 1200x675 (the headline geometry) with a still camera and a moving one ('D' held down), and the book-2 final scene (9) at
4096x4096.  Prints one JSON line per case with median HIP-event times over 20 repetitions; run under
`rocprofv3 --kernel-trace --stats -- python3 scripts/temporal_time.py` for per-kernel figures (feat_kernel, tacc_kernel).
DESIGN.md 4.10 records the results."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (torch's HIP runtime first, as tests/conftest.py does)

torch.cuda.init()
from mort_amd import hip, host  # noqa: E402
from mort_amd import structs as S  # noqa: E402


def case(ctx, sid, width, moving, reps=20, warmup=3):
    world, cam = host.build_scene(sid, width=width, spp=4)
    W, H = cam.image_width, cam.image_height
    ctx.upload_world(world)
    ctx.rng_seed(69420, W, H)
    acc = torch.from_numpy(ctx.render(cam, want_accum=True)["accum"].reshape(-1).copy()).cuda()
    alb, nrm, dep = (torch.zeros(W * H * c, dtype=torch.float32, device="cuda") for c in (3, 3, 1))
    th = hip.TemporalHistory(W, H, backend=("device", ctx))
    cams = [cam, host.camera_input(S.Camera.from_buffer_copy(cam), "D")] if moving else [cam]
    tf, tt = [], []
    for i in range(warmup + reps):
        c = cams[i % len(cams)]
        a = ctx.render_features_device(c, alb, nrm, dep, sync=True)
        b = th.step(acc, nrm, dep, c, sync=True)["seconds"]
        if i >= warmup:
            tf.append(a); tt.append(b)
    tf.sort(); tt.sort()
    print(json.dumps(dict(scene=sid, width=W, height=H, camera="moving" if moving else "still", features_ms_median=tf[len(tf) // 2] * 1e3,
                          temporal_ms_median=tt[len(tt) // 2] * 1e3, total_ms_median=(tf[len(tf) // 2] + tt[len(tt) // 2]) * 1e3,
                          temporal_ms_min=tt[0] * 1e3)), flush=True)


if __name__ == "__main__":
    with hip.Context(0) as ctx:
        case(ctx, 1, 1200, False)
        case(ctx, 1, 1200, True)
        case(ctx, 9, 4096, False)
        case(ctx, 9, 4096, True)
