#!/usr/bin/env python3
"""How far the two things DESIGN.md 2 calls unknowable move a frame, measured on the reference's own device code
compiled for the CPU (oracle/_ref, tests/ref_lib.py) against the oracle, on the same seeded inputs:

  native  glibc's sinf cosf acosf atan2f logf and fp64 sin in place of include/mort_math.h (a libm whose last ULP
          differs: CUDA's differs from both, by amounts nothing here can know)
  fma     the native build with -ffp-contract=fast -mfma (nvcc contracts a*b+c by default)

For each frame and build: the share of pixels whose uchar4 differs, the RMSE of the fp32 accumulators and the largest
byte difference.  CPU only; prints one JSON object.  Needs the reference tree or the built libraries.
usage: ref_distance.py [--tiny]   (--tiny: small frames, for the test of the output's shape)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mort_amd import host  # noqa: E402
from tests import oracle_lib as O, ref_lib as R  # noqa: E402

FRAMES = {"scene1_1200x675x4": (1, 1200, 4), "scene6_400x400x16": (6, 400, 16)}
TINY = {"scene1_1200x675x4": (1, 48, 4), "scene6_400x400x16": (6, 24, 4)}


def distance(ref, out):
    d = np.abs(ref["rgba"].astype(np.int16) - out["rgba"].astype(np.int16))
    diff = (ref["accum"].astype(np.float64) - out["accum"].astype(np.float64))
    return dict(divergent_pixel_share=float(d.any(-1).mean()), accum_rmse=float(np.sqrt(np.mean(diff * diff))),
                max_byte_diff=int(d.max()))


def main():
    frames = TINY if "--tiny" in sys.argv[1:] else FRAMES
    result = {}
    for name, (sid, width, spp) in frames.items():
        world, cam = host.build_scene(sid, width=width, spp=spp)
        W, H = cam.image_width, cam.image_height
        oracle = O.render(world, cam, nthreads=16, want_segments=False)
        row = dict(width=W, height=H, spp=spp)
        for mode in ("native", "fma"):
            out = R.render(world, cam, states=O.seed_states(69420, W, H), mode=mode)
            row[mode] = distance(oracle, out)
        result[name] = row
        print(name, json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
