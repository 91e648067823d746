"""Radiance queries on the host (mort_hip_query_radiance_host, dev_radiance.h): both host traversals -- world::hit's
item loop and the unified tree with its per-segment reach test -- against the CPU oracle's ray_color, tolerance 0: colours as raw
32-bit words (any NaN equals any NaN), final streams as all 48 bytes.  No GPU.  The oracle side is tests/radiance_ref.py."""
import json
import os
import subprocess

import numpy as np
import pytest

from mort_amd import hip, host
from tests import oracle_lib as O
from tests import query_rays as Q
from tests import radiance_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORT = os.path.join(ROOT, "mort_amd", "bin", "mort")
F = np.float32

SCENES = tuple(f"scene{k}" for k in range(1, 11))
WORLDS = SCENES + tuple(n for n in Q.WORLDS if n.startswith(("flat:", "bvh:", "placed:"))) + \
    ("bvhrandom:uniform_64_s1", "bvhrandom:ties_64_s0", "bvhrandom:ties_670_s1", "bvhrandom:uniform_2_s0") + \
    ("genrandom:instances_150_s1", "genrandom:ties_360_s0")
# the worlds every parameter is varied on: reference BVH, light + quads + deep paths, media + NaN, the final scene, a lit flat world
VARIED = ("scene1", "scene6", "scene7", "scene9", "flat:lit_by_quad_with_media")
TREES = [False, True]


def _query(ref, tree, rays=None):
    streams = ref.streams0.copy()
    got = hip.query_radiance_host(ref.world, ref.params, ref.rays if rays is None else rays, streams, tree=tree, nthreads=4)
    return got["rgb"], streams


@pytest.mark.parametrize("name", SCENES)
def test_sets_show_something(name):
    """the census of tests/radiance_ref.py, on the oracle's answers alone"""
    R.census(name)


@pytest.mark.parametrize("name", ["scene6", "scene8"])
def test_paths_run_past_the_lds_levels(name):
    """the bounce-stack levels behind the LDS part are exercised (on the oracle's answers alone)"""
    L = hip.radiance_lds_levels()
    assert 1 <= L < 50
    assert R.deep_rays(name, L) >= 16


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("name", WORLDS)
def test_one_sample_equals_the_oracle(name, tree):
    """primary, secondary, far and axis rays (zero-length and NaN directions among them) under the world's own camera"""
    ref = R.reference(name)
    rgb, streams = _query(ref, tree)
    R.assert_equal(rgb, streams, ref, f"{name} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("name", VARIED)
def test_three_samples_equal_the_oracle(name, tree):
    ref = R.reference(name, samples=3, light=R.world_light(name))
    rgb, streams = _query(ref, tree)
    R.assert_equal(rgb, streams, ref, f"{name} samples=3 tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("limit", [0, 1, 2])
@pytest.mark.parametrize("name", VARIED)
def test_bounce_limits_equal_the_oracle(name, limit, tree):
    ref = R.reference(name, bounce_limit=limit, light=R.world_light(name))
    rgb, streams = _query(ref, tree)
    R.assert_equal(rgb, streams, ref, f"{name} bounce_limit={limit} tree={tree}")
    if limit == 0:  # returns 0 and draws nothing
        assert not rgb.view(np.uint32).any() and streams.tobytes() == ref.streams0.tobytes()


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("name", ["scene6", "flat:lit_by_quad_with_media", "flat:every_material_lit_by_sphere"])
def test_light_on_and_off(name, tree):
    light = R.world_light(name)
    assert light is not None
    on, off = R.reference(name, light=light), R.reference(name, light=(-1, 0))
    assert (Q._words(on.rgb) != Q._words(off.rgb)).any(1).mean() > 0.05, "sampling the light changes nothing"
    for ref in (on, off):
        rgb, streams = _query(ref, tree)
        R.assert_equal(rgb, streams, ref, f"{name} light={ref.cam.light_obj_type} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
def test_a_background_on_a_dark_scene(tree):
    dark = R.reference("scene6")
    assert all(dark.cam.background.e[k] == 0 for k in range(3))
    ref = R.reference("scene6", background=(0.25, 0.5, 2.0))
    assert (Q._words(ref.rgb) != Q._words(dark.rgb)).any(1).mean() > 0.05
    rgb, streams = _query(ref, tree)
    R.assert_equal(rgb, streams, ref, f"scene6 with a background tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("t_max", [0.0, -1.0, np.nan])
def test_t_max_is_ignored(t_max, tree):
    ref = R.reference("scene7")
    rays = ref.rays.copy()
    rays[:, 7] = t_max
    rgb, streams = _query(ref, tree, rays)
    R.assert_equal(rgb, streams, ref, f"scene7 t_max={t_max} tree={tree}")


def test_streams_untouched_words_keep_their_bits():
    """only d and v[] of a stream are written: the Box-Muller words keep the caller's bits, drawn from or not"""
    ref = R.reference("scene7")
    streams = ref.streams0.copy()
    for k, v in (("bf", 0x11111111), ("bfd", 0x22222222), ("pad", 0x44444444)):
        streams[k] = v
    streams["be"] = 3.25; streams["bed"] = -7.5
    before = streams.copy()
    rgb = hip.query_radiance_host(ref.world, ref.params, ref.rays, streams, tree=True)["rgb"]
    assert (Q._words(rgb) == Q._words(ref.rgb)).all()
    for k in ("bf", "bfd", "be", "pad", "bed"):
        assert (streams[k] == before[k]).all(), k
    assert (streams["d"] == ref.streams["d"]).all() and (streams["v"] == ref.streams["v"]).all()
    quiet = ~ref.advanced
    assert quiet.any() and streams[quiet].tobytes() == before[quiet].tobytes(), "a ray that draws nothing keeps its bits"


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("sid", [1, 6])
def test_render_equivalence(sid, tree):
    """Camera::render at one sample per pixel is get_ray followed by ray_color on the pixel's stream: the oracle's get_ray on the
    seeded pixel streams, then the query on the advanced streams, gives mort_hip_render_host's accumulators (its NaN guard
    applied; its `0 +` is the query's own) and its final states"""
    import ctypes as C
    from mort_amd import structs as S
    world, cam = host.build_scene(sid, width=24, spp=1)
    W, H = cam.image_width, cam.image_height
    assert cam.sqrt_spp == 1 and cam.pixel_samples_scale == 1.0
    states = O.seed_states(S.DEFAULT_SEED, W, H)
    render = hip.render_host(world, cam, states=states, tree=tree, nthreads=4)
    rays = np.zeros((W * H, 8), dtype=F)
    r7 = np.zeros(7, dtype=F)
    L = O.lib()
    for y in range(H):
        for x in range(W):
            i = x + y * W
            L.mort_oracle_get_ray(C.byref(cam), x, y, 0, 0, C.cast(states.ctypes.data + 48 * i, C.POINTER(S.RngState)), r7.ctypes.data_as(C.POINTER(C.c_float)))
            rays[i, :7] = r7
    rays[:, 7] = np.inf
    got = hip.query_radiance_host(world, hip.radiance_params_from_camera(cam), rays, states, tree=tree, nthreads=4)["rgb"]
    guarded = np.where(np.isnan(got), F(0), got)
    assert (guarded.view(np.uint32) == render["accum"].reshape(-1, 3).view(np.uint32)).all()
    final = render["states"].view(O.STATE_DTYPE)
    assert (states["d"] == final["d"]).all() and (states["v"] == final["v"]).all()
    assert (got != 0).any(1).mean() > 0.2


@pytest.mark.parametrize("sid,tree", [(6, True), (1, False), (7, False)])
def test_probe_prints_the_colour_along_the_pixel_ray(sid, tree):
    """`mort <scene> --mode host --probe X,Y[,N]`: the feature pass's primary ray of the pixel, N paths from subsequence X + Y * W of
    the seed, the scene camera's parameters: the oracle's sum"""
    from mort_amd import structs as S
    from tests.feature_ref import primary_rays
    if not os.path.exists(MORT):
        subprocess.check_call(["make", "-C", ROOT, "host", "hip", "cli"])
    world, cam = host.build_scene(sid, width=48, spp=1)
    W, H = cam.image_width, cam.image_height
    prim = primary_rays(cam)
    seeded = O.seed_states(S.DEFAULT_SEED, W, H)
    for x, y, n in ((W // 2, H // 2, None), (5, H - 3, 4), (W - 1, 0, 1)):
        i = x + y * W
        args = [MORT, str(sid), "--mode", "host", "--width", "48", "--probe", f"{x},{y}" + (f",{n}" if n else "")] + (["--tree"] if tree else [])
        p = subprocess.run(args, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        lines = p.stdout.strip().splitlines()
        assert len(lines) == 1, "one JSON line"
        j = json.loads(lines[0])
        assert j["probe"] == [x, y] and j["samples"] == (n or 1) and j["mode"] == "host"
        ray = np.array(j["origin"] + j["dir"] + [j["time"]], dtype=F)
        assert (ray.view(np.uint32) == prim[i].view(np.uint32)).all()
        want = R.oracle_radiance(world, cam, np.append(prim[i], F(np.inf))[None, :], seeded[i:i + 1].copy(), n or 1)
        assert (Q._words(np.array(j["rgb"], dtype=F)) == Q._words(want[0])).all(), (j, want)
    p = subprocess.run([MORT, str(sid), "--mode", "host", "--width", "48", "--probe", f"0,{H}"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "outside" in p.stderr
