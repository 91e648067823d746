"""The catalogue of random sphere-BVH worlds (tests/worlds.py BVH_RANDOM) checked on the CPU, so that the GPU battery over it
(tests/test_gpu_bvh_random.py) cannot pass vacuously: which state this build's own trees are in for every entry, which kernel
family the host will pick, that the entries reach both sides of the 72 KB image limit and the upper end of the four-wide stack
bound, that every camera sees spheres and paths that bounce, and that the host loop over the reference BVH agrees with the
oracle on these worlds bit for bit."""
import numpy as np
import pytest

from mort_amd import hip
from tests import oracle_lib as O
from tests.feature_ref import oracle_features, MISS
from tests.worlds import BVH_RANDOM, BVH_FAMILIES, BVH_LIMIT_SIZES, BVH_INTERIOR_VIEW, bvh_random_case, bvh_random_camera, bvh_random_prediction

NAMES = sorted(BVH_RANDOM)
OWN4_STACK = 24  # MORT_OWN4_STACK (scene_compile.h)


def test_catalogue_shape():
    """two seeds of every family at every size the battery asks for, named one by one"""
    for fam in BVH_FAMILIES:
        for n in (2, 3, 4, 5, 7, 64, 300) + BVH_LIMIT_SIZES[fam] + (1000,):
            for seed in (0, 1):
                assert BVH_RANDOM[f"{fam}_{n}_s{seed}"][:3] == (fam, n, seed)
    for name in NAMES:
        w, views, light = bvh_random_case(name)
        fam, n, _, _, emissive = BVH_RANDOM[name]
        o = w.c.objs
        assert o.num_spheres == n and o.num_bvh == 1 and o.host_hittable_list[0].num_objs == n and w.c.bvh_mode
        moving = sum(o.host_sphere[i].moves for i in range(n))
        assert (moving == 0) if fam == "line" else (n < 64 or moving >= 1) and (n < 300 or fam == "ties" or 0.08 * n <= moving <= 0.22 * n), (name, moving)  # a repeated sphere repeats its motion
        assert len(views) == (2 if fam == "line" else 3) and (light is not None) == emissive


@pytest.mark.parametrize("name", NAMES)
def test_own_tree_state(name):
    """mort_hip_debug_own_tree succeeds; with a four-wide tree its numbers satisfy what tests/test_abi.py states for one, and the
    entry is in one of three states: 1 fewer than two leaf nodes, no own tree; 2 an own tree whose pending-children bound exceeds
    the kernel's LDS stack, so no four-wide form; 3 both trees"""
    p = bvh_random_prediction(name)
    t, im = p["tree"], p["image"]
    assert im["sphere_bvh"] == 1
    if p["state"] == 1:
        assert BVH_RANDOM[name][1] <= 2 and t["n2"] == 0 and t["n4"] == 0 and not p["fits"]
        return
    assert t["n2"] == t["leaves"] - 1 and t["depth2"] <= 15, t
    if p["state"] == 2:
        assert t["stack4"] > OWN4_STACK and im["four_wide"] == 0 and not p["fits"], t
        return
    assert 1 <= t["n4"] <= max(1, t["n2"] // 2 + 1) and t["reached"] == t["leaves"] and t["bad"] == 0 and t["same"] == 1, t
    assert t["slots"] == t["n4"] - 1 + t["leaves"] and 1 <= t["stack4"] <= OWN4_STACK, t
    assert im["four_wide"] == 1 and im["stack_levels"] == t["stack4"]
    assert p["fits"] == (im["fast_bytes"] <= im["limit"] and im["trav_bytes"] <= im["limit"]) and im["limit"] == 72 * 1024
    # 1024-thread groups: the 72 KB image, 25 traversal levels and one bounce level of 1024 lanes come to 140 KB of a CU's 160
    assert im["wide_fits"] == int(p["fits"])


def test_catalogue_reaches_the_limits():
    """the census the GPU battery relies on: entries just inside the image limit, entries beyond it, entries that fit with a
    stack bound near MORT_OWN4_STACK, all three tree states, and the second state at sizes whose images would fit"""
    P = {name: bvh_random_prediction(name) for name in NAMES}
    spare = {n: p["image"]["limit"] - max(p["image"]["fast_bytes"], p["image"]["trav_bytes"]) for n, p in P.items() if p["fits"]}
    assert sum(0 <= s < 4096 for s in spare.values()) >= 4, spare
    too_big = [n for n, p in P.items() if p["state"] == 3 and not p["fits"]]
    assert len(too_big) >= 4, too_big
    assert sum(p["fits"] and p["tree"]["stack4"] >= 20 for p in P.values()) >= 3
    assert {p["state"] for p in P.values()} == {1, 2, 3}
    # every family: its size below the limit fits with both seeds or is without a four-wide tree, its size above does not fit
    for fam, (below, above) in BVH_LIMIT_SIZES.items():
        assert all(P[f"{fam}_{below}_s{s}"]["fits"] for s in (0, 1)), fam
        assert not all(P[f"{fam}_{above}_s{s}"]["fits"] for s in (0, 1)), fam
    # state 2 below the image limit: the binary tree's image is no larger than that of entries of the same family that fit
    fitting_trav = max(p["image"]["trav_bytes"] for p in P.values() if p["fits"])
    small2 = [n for n, p in P.items() if p["state"] == 2 and p["image"]["trav_bytes"] <= fitting_trav and BVH_RANDOM[n][1] < 640]
    assert len(small2) >= 3, small2
    assert all(P[n]["kernel"] == "mega_kernel" for n in small2 + too_big)


_seen = {}


def _what_the_camera_sees(name, k):
    if (name, k) not in _seen:
        w, _, _ = bvh_random_case(name)
        cam = bvh_random_camera(name, k)
        f = oracle_features(w, cam, nthreads=8)
        r = O.render(w, cam, nthreads=8, want_accum=False, want_segments=False)
        _seen[name, k] = (float((f["kind"] != MISS).mean()), r["segments"], cam.image_width * cam.image_height * cam.sqrt_spp ** 2)
    return _seen[name, k]


@pytest.mark.parametrize("name", NAMES)
def test_cameras_see_spheres_and_sky(name):
    """a condition on the catalogue, judged by the oracle alone: at least a fifth of every frame's pixels first meet a sphere,
    and all views but the one placed inside a sphere on purpose keep at least 5 % background"""
    fam = BVH_RANDOM[name][0]
    for k in range(len(bvh_random_case(name)[1])):
        hit, _, _ = _what_the_camera_sees(name, k)
        assert hit >= 0.20, (name, k, hit)
        if (fam, k) != BVH_INTERIOR_VIEW:
            assert hit <= 0.95, (name, k, hit)
    cam = bvh_random_camera(name, 0)
    assert (cam.image_width, cam.image_height) == (96, 54) and cam.sqrt_spp in (2, 3) and 2 <= cam.bounce_limit <= 20


def test_paths_bounce():
    """over the whole catalogue the oracle traces at least 1.5 segments per sample: the cameras do not look at sky"""
    seg = n = 0
    for name in NAMES:
        for k in range(len(bvh_random_case(name)[1])):
            _, s, m = _what_the_camera_sees(name, k)
            seg += s; n += m
    assert seg >= 1.5 * n, seg / n


HOST_LOOP_CASES = ["uniform_1000_s0", "cluster_1000_s1", "scales_1000_s0", "line_1000_s0", "shells_1000_s1", "ties_1000_s0",
                   "uniform_650_s1", "scales_640_s0", "ties_460_s1", "shells_300_s1", "cluster_64_s1", "ties_7_s0", "scales_2_s0"]


@pytest.mark.parametrize("name", HOST_LOOP_CASES)
def test_host_loop_equals_oracle(name):
    """hip.render_host (the item scan over the reference BVH) against oracle.render, bit for bit, on worlds with moving spheres
    and up to 1000 list entries: the reference side of the GPU comparison"""
    w, views, _ = bvh_random_case(name)
    k = len(views) - 1 if BVH_RANDOM[name][0] != "scales" else 1
    cam = bvh_random_camera(name, k)
    ref = O.render(w, cam, nthreads=8)
    out = hip.render_host(w, cam, nthreads=8)
    assert (out["rgba"] == ref["rgba"]).all() and (out["accum"].view(np.uint32) == ref["accum"].view(np.uint32)).all()
    assert (out["segments_px"] == ref["segments_px"]).all()
    assert out["stats"]["segments"] == ref["segments"] and out["stats"]["rng_draws"] == ref["rng_draws"]
    st = out["states"].view(O.STATE_DTYPE)
    assert (st["d"] == ref["states"]["d"]).all() and (st["v"] == ref["states"]["v"]).all()
