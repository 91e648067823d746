"""MATERIAL_WORLDS (tests/material_worlds.py: the worlds; tests/test_material_worlds_host.py: the census and the tag rows' figures)
through every kernel form that shades, against the oracle.  The step after the closest hit exists in three hand-written copies, and
each form below is named for the copy it runs:

  - the kernel the library picks: mega_kernel (shade_hit) for the flat forms, mega_bvh_kernel (its inline shade block) for the BVH forms;
  - the one-lane-per-pixel kernel forced (MORT_FORCE_GENERIC=1): shade_hit over the BVH forms too;
  - the unified-tree megakernel forced onto the flat forms (MORT_GEN_MIN_PRIMS=0): shade_hit;
  - mega_bvh_kernel at 1024, 768 and 256 threads for the BVH forms: the HBM part of the bounce stack differs with the block size, and
    mirror_hall fills it to the bounce limits 64, 50 and 13;
  - wavefront mode: wf_shade / wf_texture for the BVH forms, wf_shade_gen for the flat forms;
  - a radiance query over the frame's own primary rays and one SH9 probe at the camera.

Image, accumulators as raw words, per-pixel segment counts, totals and final RNG words are the oracle's, bit for bit; the kernel's name
is asserted, so a world meant for one copy ran on it.  No world carries an index outside a table."""
import numpy as np
import pytest

from mort_amd import hip, structs as S
from tests import material_worlds as M
from tests import oracle_lib as O
from tests import query_rays as Q

pytestmark = pytest.mark.gpu

KEYS = M.KEYS
IDS = [M.key_id(k) for k in KEYS]
BVH_KEYS = [k for k in KEYS if k[1] == "bvh"]
FLAT_KEYS = [k for k in KEYS if k[1] == "flat"]


def _tree_serves(world, cam):
    """choose_family's gen_reach: the world has a unified tree within the image limit and the camera lies within its reach"""
    t = hip.debug_gen_tree(world)
    if not (t["tree"] and t["fits"]):
        return False
    centre = np.array([[cam.center.e[k] for k in range(3)]], np.float32)
    return bool(Q.in_reach(Q.reach(world), centre)[0])


def _render(ctx, key, mode=hip.MODE_MEGA):
    world, cam = M.material_world(key[0], key[1]), M.camera(key[0], key[2])
    W, H = cam.image_width, cam.image_height
    ctx.set_partition(0, 1, 8)
    ctx.upload_world(world)
    ctx.rng_seed(S.DEFAULT_SEED, W, H)
    out = ctx.render(cam, mode=mode, want_accum=True, want_segments=True)
    out["states"] = ctx.rng_store(W, H, O.STATE_DTYPE)
    return out


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_the_kernel_the_library_picks(gpu_ctx, key):
    out = _render(gpu_ctx, key)
    want = "mega_bvh_kernel<" if key[1] == "bvh" else "mega_kernel"
    assert out["stats"]["kernel_name"].startswith(want), out["stats"]["kernel_name"]
    M.assert_frame_same(out, M.frame_reference(key), M.key_id(key))


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_one_lane_per_pixel_kernel(gpu_ctx, monkeypatch, key):
    monkeypatch.setenv("MORT_FORCE_GENERIC", "1")
    out = _render(gpu_ctx, key)
    assert out["stats"]["kernel_name"] == "mega_kernel", out["stats"]["kernel_name"]
    M.assert_frame_same(out, M.frame_reference(key), M.key_id(key))


@pytest.mark.parametrize("key", FLAT_KEYS, ids=[M.key_id(k) for k in FLAT_KEYS])
def test_unified_tree_megakernel_forced(gpu_ctx, monkeypatch, key):
    monkeypatch.setenv("MORT_GEN_MIN_PRIMS", "0")
    assert _tree_serves(M.material_world(key[0], key[1]), M.camera(key[0], key[2]))  # every flat form has a tree the camera can use
    out = _render(gpu_ctx, key)
    assert out["stats"]["kernel_name"].startswith("mega_gen_kernel<"), out["stats"]["kernel_name"]
    M.assert_frame_same(out, M.frame_reference(key), M.key_id(key))


@pytest.mark.parametrize("block", [1024, 768, 256])
@pytest.mark.parametrize("key", BVH_KEYS, ids=[M.key_id(k) for k in BVH_KEYS])
def test_bvh_megakernel_block_sizes(gpu_ctx, monkeypatch, key, block):
    monkeypatch.setenv("MORT_FAST_BLOCK_SIZE", str(block))
    out = _render(gpu_ctx, key)
    assert out["stats"]["kernel_name"].startswith(f"mega_bvh_kernel<{block},"), out["stats"]["kernel_name"]
    M.assert_frame_same(out, M.frame_reference(key), f"{M.key_id(key)} block {block}")


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_wavefront_mode(gpu_ctx, key):
    out = _render(gpu_ctx, key, mode=hip.MODE_WAVE)
    want = "wf_trav<" if key[1] == "bvh" else "wf_trav_gen<"
    assert out["stats"]["kernel_name"].startswith(want), out["stats"]["kernel_name"]
    M.assert_frame_same(out, M.frame_reference(key), M.key_id(key))


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_radiance_query_along_the_frames_primary_rays(gpu_ctx, key):
    r = M.radiance_reference(key)
    gpu_ctx.upload_world(M.material_world(key[0], key[1]))
    streams = r.streams0.copy()
    got = gpu_ctx.query_radiance(r.params, r.rays, streams)["rgb"]
    bad = np.flatnonzero((Q._words(got) != Q._words(r.rgb)).any(1))
    assert bad.size == 0, f"{key}: colour differs for {bad.size} rays, first {bad[0]}: got {got[bad[0]]} oracle {r.rgb[bad[0]]}"
    assert streams.tobytes() == r.streams.tobytes(), f"{key}: final streams differ"


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_one_probe(gpu_ctx, key):
    from tests import probe_ref as P
    r = M.probe_reference(key)
    gpu_ctx.upload_world(r.world)
    streams = r.streams0.copy()
    sh = gpu_ctx.probe_bake(r.params, r.probes, streams)["sh"]
    P.assert_equal(sh, streams, r, M.key_id(key))
