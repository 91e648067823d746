"""The light objects no built-in scene has, through every kernel form that shades, against the oracle: LIGHT_WORLDS of
tests/light_cases.py (the worlds, the census and its measured figures: tests/test_light_worlds_host.py) at 64 x 36, 4 spp, bounce limit 8.

  - the kernel the library picks (mega_kernel for the small worlds and for the BVH world, whose light object keeps it off the BVH
    megakernel; mega_gen_kernel for big_list);
  - the one-lane-per-pixel kernel forced (MORT_FORCE_GENERIC=1);
  - the unified-tree megakernel forced onto the small worlds (MORT_GEN_MIN_PRIMS=0);
  - wavefront mode, where choose_family accepts the world (a unified tree with the camera in its reach), refused with
    MORT_ERR_UNSUPPORTED for the BVH world;
  - a radiance query over the frame's own primary rays;
  - one SH9 probe.

Image, accumulators, per-pixel segment counts, totals and final RNG words are the oracle's, bit for bit; where a NaN can appear (the
per-ray colours of dome, coplanar and degenerate_quad; the frames zero theirs) its sign and payload are not compared
(tests/query_rays._words)."""
import numpy as np
import pytest

from mort_amd import hip, structs as S
from tests import light_cases as LC
from tests import oracle_lib as O
from tests import query_rays as Q

pytestmark = pytest.mark.gpu

NAMES = sorted(LC.LIGHT_WORLDS)


def _tree_serves(world, cam):
    """choose_family's gen_reach: the world has a unified tree within the image limit and the camera lies within its reach"""
    t = hip.debug_gen_tree(world)
    if not (t["tree"] and t["fits"]):
        return False
    centre = np.array([[cam.center.e[k] for k in range(3)]], np.float32)
    return bool(Q.in_reach(Q.reach(world), centre)[0])


def _render(ctx, name, mode=hip.MODE_MEGA):
    world, cam = LC.light_world(name)
    W, H = cam.image_width, cam.image_height
    ctx.set_partition(0, 1, 8)
    ctx.upload_world(world)
    ctx.rng_seed(S.DEFAULT_SEED, W, H)
    out = ctx.render(cam, mode=mode, want_accum=True, want_segments=True)
    out["states"] = ctx.rng_store(W, H, O.STATE_DTYPE)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_the_kernel_the_library_picks(gpu_ctx, name):
    out = _render(gpu_ctx, name)
    want = "mega_gen_kernel" if name == "big_list" else "mega_kernel"
    assert out["stats"]["kernel_name"].startswith(want), out["stats"]["kernel_name"]
    LC.assert_frame_same(out, LC.frame_reference(name), name)


@pytest.mark.parametrize("name", NAMES)
def test_one_lane_per_pixel_kernel(gpu_ctx, monkeypatch, name):
    monkeypatch.setenv("MORT_FORCE_GENERIC", "1")
    out = _render(gpu_ctx, name)
    assert out["stats"]["kernel_name"] == "mega_kernel", out["stats"]["kernel_name"]
    LC.assert_frame_same(out, LC.frame_reference(name), name)


@pytest.mark.parametrize("name", NAMES)
def test_unified_tree_megakernel_forced(gpu_ctx, monkeypatch, name):
    monkeypatch.setenv("MORT_GEN_MIN_PRIMS", "0")
    world, cam = LC.light_world(name)
    out = _render(gpu_ctx, name)
    serves = _tree_serves(world, cam)
    assert serves == (name != "bvh_list")
    assert out["stats"]["kernel_name"].startswith("mega_gen_kernel" if serves else "mega_kernel"), out["stats"]["kernel_name"]
    LC.assert_frame_same(out, LC.frame_reference(name), name)


@pytest.mark.parametrize("name", NAMES)
def test_wavefront_mode(gpu_ctx, name):
    world, cam = LC.light_world(name)
    if not _tree_serves(world, cam):
        assert name == "bvh_list"
        with pytest.raises(hip.MortHipError) as e:
            _render(gpu_ctx, name, mode=hip.MODE_WAVE)
        assert e.value.status == -6
        return
    out = _render(gpu_ctx, name, mode=hip.MODE_WAVE)
    assert not out["stats"]["kernel_name"].startswith("mega_"), out["stats"]["kernel_name"]
    LC.assert_frame_same(out, LC.frame_reference(name), name)


@pytest.mark.parametrize("name", NAMES)
def test_radiance_query_along_the_frames_primary_rays(gpu_ctx, name):
    world, _ = LC.light_world(name)
    r = LC.radiance_reference(name)
    gpu_ctx.upload_world(world)
    streams = r.streams0.copy()
    got = gpu_ctx.query_radiance(r.params, r.rays, streams)["rgb"]
    bad = np.flatnonzero((Q._words(got) != Q._words(r.rgb)).any(1))
    assert bad.size == 0, f"{name}: colour differs for {bad.size} rays, first {bad[0]}: got {got[bad[0]]} oracle {r.rgb[bad[0]]}"
    assert streams.tobytes() == r.streams.tobytes(), f"{name}: final streams differ"


@pytest.mark.parametrize("name", NAMES)
def test_one_probe(gpu_ctx, name):
    from tests import probe_ref as P
    r = LC.probe_reference(name)
    gpu_ctx.upload_world(r.world)
    streams = r.streams0.copy()
    sh = gpu_ctx.probe_bake(r.params, r.probes, streams)["sh"]
    P.assert_equal(sh, streams, r, name)
