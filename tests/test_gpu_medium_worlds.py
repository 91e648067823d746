"""MEDIUM_WORLDS (tests/medium_worlds.py: the worlds and their rays; tests/test_medium_worlds_host.py: the census, the pin and the host
forms) through every hand-written copy of constant_medium::hit on the device, each bit for bit against the cached oracle frame or the
oracle's hit records.  Each test is named for the copy it runs and, where the call reports one, asserts the kernel's name:

  - the kernel the library picks (mega_gen_kernel from 48 solids on, else mega_kernel);
  - mega_kernel forced (MORT_FORCE_GENERIC=1): world_hit of dev_trace.h;
  - mega_gen_kernel forced (MORT_GEN_MIN_PRIMS=0) at 256 and at 1024 threads: gen_media of dev_gen.h and the has_media path of mega_gen.hip;
  - wavefront mode: wf_trav_gen;
  - query_closest with streams (hits and final streams) and without (media passed over, streams untouched), and query_occluded, with the
    world uploaded as it is (gen_world_hit) and under MORT_NO_GEN=1 (the MEDIA branch of the scan in dev_query.h);
  - query_radiance over the frame's primary rays and one SH9 probe at the camera;
  - render_cached with a cache depth above the bounce limit, which is then the plain frame, on density_edges and transformed_phase: the
    cached kernel's own walk;
  - render_features with and without the tree: the deterministic entry of dev_features.h."""
import numpy as np
import pytest

from mort_amd import hip, structs as S
from tests import cached_frame_ref as FR
from tests import material_worlds as M
from tests import medium_worlds as MW
from tests import oracle_lib as O
from tests import query_rays as Q
from tests.feature_ref import assert_same_words

pytestmark = pytest.mark.gpu

NAMES, TREE_NAMES = MW.NAMES, MW.TREE_NAMES
GEN_MIN_PRIMS = 48  # choose_family's default (mort_hip.hip)
UNSUPPORTED = -6


def _render(ctx, name, mode=hip.MODE_MEGA):
    world, cam = MW.world(name), MW.camera(name)
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
    t = hip.debug_gen_tree(MW.world(name))
    want = "mega_gen_kernel<" if t["tree"] and t["entries"] >= GEN_MIN_PRIMS else "mega_kernel"
    assert (name == "negative_far") == (want == "mega_gen_kernel<")
    assert out["stats"]["kernel_name"].startswith(want), out["stats"]["kernel_name"]
    M.assert_frame_same(out, MW.frame_reference(name), name)


@pytest.mark.parametrize("name", NAMES)
def test_one_lane_per_pixel_kernel(gpu_ctx, monkeypatch, name):
    monkeypatch.setenv("MORT_FORCE_GENERIC", "1")
    out = _render(gpu_ctx, name)
    assert out["stats"]["kernel_name"] == "mega_kernel", out["stats"]["kernel_name"]
    M.assert_frame_same(out, MW.frame_reference(name), name)


@pytest.mark.parametrize("block", [256, 1024])
@pytest.mark.parametrize("name", NAMES)
def test_unified_tree_megakernel_forced(gpu_ctx, monkeypatch, name, block):
    monkeypatch.setenv("MORT_GEN_MIN_PRIMS", "0")
    monkeypatch.setenv("MORT_GEN_BLOCK_SIZE", str(block))
    out = _render(gpu_ctx, name)
    want = f"mega_gen_kernel<{block}," if name in TREE_NAMES else "mega_kernel"  # a world without a tree keeps the scan
    assert out["stats"]["kernel_name"].startswith(want), out["stats"]["kernel_name"]
    M.assert_frame_same(out, MW.frame_reference(name), f"{name} block {block}")


@pytest.mark.parametrize("name", NAMES)
def test_wavefront_mode(gpu_ctx, name):
    if name not in TREE_NAMES:  # the wavefront pipeline walks the tree only
        with pytest.raises(hip.MortHipError) as e:
            _render(gpu_ctx, name, mode=hip.MODE_WAVE)
        assert e.value.status == UNSUPPORTED
        return
    out = _render(gpu_ctx, name, mode=hip.MODE_WAVE)
    assert out["stats"]["kernel_name"].startswith("wf_trav_gen<"), out["stats"]["kernel_name"]
    M.assert_frame_same(out, MW.frame_reference(name), name)


@pytest.mark.parametrize("no_gen", [False, True], ids=["tree", "scan"])
@pytest.mark.parametrize("name", NAMES)
def test_closest_hit_and_occlusion_queries(gpu_ctx, monkeypatch, name, no_gen):
    if no_gen:
        monkeypatch.setenv("MORT_NO_GEN", "1")  # read when the world is uploaded
    r = MW.rays(name)
    gpu_ctx.upload_world(MW.world(name))
    streams = r.streams0.copy()
    got = gpu_ctx.query_closest(r.rays, streams)["hits"]
    MW.assert_hits_equal(name, got, True, f"{name} with streams")
    assert streams.tobytes() == r.streams.tobytes(), f"{name}: final streams differ"
    got = gpu_ctx.query_closest(r.rays)["hits"]
    MW.assert_hits_equal(name, got, False, f"{name} without streams")
    occ = gpu_ctx.query_occluded(r.rays)["occluded"]
    assert (occ.astype(bool) == r.shit).all(), f"{name}: occlusion differs from the oracle's solid hits"


@pytest.mark.parametrize("name", NAMES)
def test_radiance_query_along_the_frames_primary_rays(gpu_ctx, name):
    r = MW.radiance_reference(name)
    gpu_ctx.upload_world(MW.world(name))
    streams = r.streams0.copy()
    got = gpu_ctx.query_radiance(r.params, r.rays, streams)["rgb"]
    bad = np.flatnonzero((Q._words(got) != Q._words(r.rgb)).any(1))
    assert bad.size == 0, f"{name}: colour differs for {bad.size} rays, first {bad[0]}: got {got[bad[0]]} oracle {r.rgb[bad[0]]}"
    assert streams.tobytes() == r.streams.tobytes(), f"{name}: final streams differ"


@pytest.mark.parametrize("name", NAMES)
def test_one_probe(gpu_ctx, name):
    from tests import probe_ref as P
    r = MW.probe_reference(name)
    gpu_ctx.upload_world(r.world)
    streams = r.streams0.copy()
    sh = gpu_ctx.probe_bake(r.params, r.probes, streams)["sh"]
    P.assert_equal(sh, streams, r, name)


@pytest.mark.parametrize("name", ["density_edges", "transformed_phase"])
def test_cached_frame_that_never_reaches_its_volume(gpu_ctx, name):
    """one probe of zeros and a cache depth above the bounce limit: no path ends in the volume, the frame is the plain one"""
    world, cam, want = MW.world(name), MW.camera(name), MW.frame_reference(name)
    W, H = cam.image_width, cam.image_height
    params = FR.params(cam.bounce_limit + 1, hip.VOLUME_GRID(origin=(0, 0.5, -1), spacing=(1, 1, 1), count=(1, 1, 1), time=0.5))
    gpu_ctx.set_partition(0, 1, 8)
    gpu_ctx.upload_world(world)
    gpu_ctx.rng_seed(S.DEFAULT_SEED, W, H)
    out = gpu_ctx.render_cached(cam, params, np.zeros((1, hip.VOLUME_RECORD_FLOATS), np.float32), want_segments=True)
    out["states"] = gpu_ctx.rng_store(W, H, O.STATE_DTYPE)
    assert out["stats"]["kernel_name"] == "cached_frame_kernel<true, false>", out["stats"]["kernel_name"]
    assert not out["ends_px"].any()
    M.assert_frame_same(out, want, name)


def test_a_medium_bounded_by_a_medium_is_refused_at_upload(gpu_ctx):
    w = MW.odd_boundary_world(("medium", MW._ball((0.9, 0.2, -0.8), 0.45, 2.0, 2)))
    with pytest.raises(hip.MortHipError) as e:
        gpu_ctx.upload_world(w)
    assert e.value.status == UNSUPPORTED
    gpu_ctx.upload_world(MW.world("density_edges"))  # the context serves the next world


@pytest.mark.parametrize("gen", [False, True], ids=["mega_kernel", "mega_gen_kernel"])
@pytest.mark.parametrize("tag", [S.OBJ_BVH, 99])
def test_a_medium_bounded_by_a_tag_without_a_hit_test_is_never_hit(gpu_ctx, monkeypatch, tag, gen):
    """the oracle's frame of the world WITHOUT that medium (tests/test_medium_worlds_host.py shows the oracle renders both alike)"""
    if gen:
        monkeypatch.setenv("MORT_GEN_MIN_PRIMS", "0")
    cam = MW.camera("density_edges")
    W, H = cam.image_width, cam.image_height
    want = O.render(MW.odd_boundary_world(None), cam, nthreads=8)
    gpu_ctx.set_partition(0, 1, 8)
    gpu_ctx.upload_world(MW.odd_boundary_world(("tag", tag, 0)))
    gpu_ctx.rng_seed(S.DEFAULT_SEED, W, H)
    out = gpu_ctx.render(cam, want_accum=True, want_segments=True)
    out["states"] = gpu_ctx.rng_store(W, H, O.STATE_DTYPE)
    assert out["stats"]["kernel_name"].startswith("mega_gen_kernel<" if gen else "mega_kernel"), out["stats"]["kernel_name"]
    M.assert_frame_same(out, want, f"tag {tag}")


@pytest.mark.parametrize("no_gen", [False, True], ids=["tree", "scan"])
@pytest.mark.parametrize("name", NAMES)
def test_feature_pass(gpu_ctx, monkeypatch, name, no_gen):
    if no_gen:
        monkeypatch.setenv("MORT_NO_GEN", "1")
    gpu_ctx.set_partition(0, 1, 8)
    gpu_ctx.upload_world(MW.world(name))
    assert_same_words(gpu_ctx.render_features(MW.camera(name)), MW.features_reference(name), f"{name} MORT_NO_GEN={int(no_gen)}")
