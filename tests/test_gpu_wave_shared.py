"""The parts the two forms of MORT_MODE_WAVE share (wave_common.h: front 0, the shade kernels' head and tail, the append
to the next front), at the corners of their index arithmetic in one place: a width that is no multiple of 64, so the last
wave of every class queue and of every front is partial; a spp that is not a square; depth 2, so most paths end at the bounce
limit and unwind a full stack; a two-way row partition whose ranks own different numbers of rows, so a path id is not a
pixel offset of the frame and global_row decides every camera ray; and the accumulator and segment buffers present or
null.  Bar: the oracle's render of the whole frame, bit for bit."""
import functools

import numpy as np
import pytest

from mort_amd import host, hip, structs as S

pytestmark = pytest.mark.gpu

WIDTH, SPP, DEPTH, NRANKS, RPB = 61, 5, 2, 2, 8


@functools.lru_cache(maxsize=None)
def _reference(sid):
    from tests import oracle_lib
    world, cam = host.build_scene(sid, width=WIDTH, spp=SPP, depth=DEPTH)
    ref = oracle_lib.render(world, cam, nthreads=8)
    for a in (ref["rgba"], ref["accum"], ref["segments_px"], ref["states"]):
        a.setflags(write=False)
    return world, cam, ref


# scene 1: one reference BVH of spheres (wave_bvh.h); scene 6: the Cornell box, a unified-tree world with a light (wave_gen.hip)
@pytest.mark.parametrize("buffers", [True, False], ids=["buffers", "null_buffers"])
@pytest.mark.parametrize("sid,kernel", [(1, "wf_trav<"), (6, "wf_trav_gen<")])
def test_partitioned_wave_render_equals_oracle(gpu_ctx, oracle, sid, kernel, buffers):
    world, cam, ref = _reference(sid)
    W, H = cam.image_width, cam.image_height
    rgba = np.zeros((H, W, 4), np.uint8)
    accum = np.zeros((H, W, 3), np.float32)
    seg = np.zeros((H, W), np.uint32)
    states = np.zeros((H, W), oracle.STATE_DTYPE)
    total = draws = 0
    owned = []
    try:
        for r in range(NRANKS):
            gpu_ctx.set_partition(r, NRANKS, RPB)
            gpu_ctx.upload_world(world)
            gpu_ctx.rng_seed(S.DEFAULT_SEED, W, H)
            out = gpu_ctx.render(cam, mode=hip.MODE_WAVE, want_accum=buffers, want_segments=buffers)
            assert out["stats"]["kernel_name"].startswith(kernel), out["stats"]["kernel_name"]
            rows = [gpu_ctx.global_row(l) for l in range(gpu_ctx.local_rows(H))]
            owned.append(len(rows))
            rgba[rows] = out["rgba"][rows]
            if buffers:
                accum[rows] = out["accum"][rows]
                seg[rows] = out["segments_px"][rows]
            else:
                assert out["accum"] is None and out["segments_px"] is None
            states[rows] = gpu_ctx.rng_store(W, H, oracle.STATE_DTYPE).reshape(H, W)[rows]
            total += out["stats"]["segments"]
            draws += out["stats"]["rng_draws"]
    finally:
        gpu_ctx.set_partition(0, 1, 8)
    assert sum(owned) == H and owned[0] != owned[1], owned
    assert (rgba == ref["rgba"]).all(), "uchar4 image differs"
    if buffers:
        assert (accum.view(np.uint32) == ref["accum"].view(np.uint32)).all(), "fp32 accumulators differ (bitwise)"
        assert (seg == ref["segments_px"]).all(), "per-pixel segment counts differ"
    want = ref["states"].reshape(H, W)
    assert (states["d"] == want["d"]).all() and (states["v"] == want["v"]).all(), "final stream words differ"
    assert total == ref["segments"] and draws == ref["rng_draws"]
