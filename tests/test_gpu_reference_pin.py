"""The GPU kernels against the reference's own device code, through the recorded digests of tests/golden/ref_pin.npz
(what the reference build in oracle/_ref renders on the CPU, tests/test_reference_pin.py): uchar4 image, fp32
accumulators and XORWOW words of two consecutive frames, for every kernel family -- mega_bvh_kernel, mega_gen_kernel,
mega_kernel -- and the wavefront mode.  Reads only the recorded digests, never the reference tree."""
import os

import numpy as np
import pytest

from mort_amd import hip, host
from tests import oracle_lib as O
from tests.golden.make_golden import REF_PIN_CASES, REF_PIN_FRAMES, digest, state_words

pytestmark = pytest.mark.gpu

PIN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pin.npz"))
KERNEL = {"s1": "mega_bvh_kernel", "s10": "mega_bvh_kernel", "s9": "mega_gen_kernel", "s6": "mega_kernel", "s3": "mega_kernel"}


@pytest.mark.parametrize("mode", [hip.MODE_MEGA, hip.MODE_WAVE])
@pytest.mark.parametrize("name", sorted(REF_PIN_CASES))
def test_kernels_render_what_the_reference_rendered(gpu_ctx, name, mode):
    sid, width, spp, depth = REF_PIN_CASES[name]
    world, cam = host.build_scene(sid, width=width, spp=spp, depth=depth)
    gpu_ctx.set_partition(0, 1, 8)
    gpu_ctx.upload_world(world)
    gpu_ctx.rng_seed(69420, cam.image_width, cam.image_height)
    for f in range(REF_PIN_FRAMES):
        out = gpu_ctx.render(cam, mode=mode, want_accum=True)
        st = gpu_ctx.rng_store(cam.image_width, cam.image_height, O.STATE_DTYPE)
        if mode == hip.MODE_MEGA:
            assert out["stats"]["kernel_name"].startswith(KERNEL[name]), out["stats"]["kernel_name"]
        got = [digest(out["rgba"]), digest(out["accum"]), digest(state_words(st))]
        assert got == PIN[f"{name}_f{f}"].tolist(), f"frame {f} ({out['stats']['kernel_name']}): [rgba, accum, states] digests differ"
