"""Ray queries on the host (mort_hip_query_closest_host / mort_hip_query_occluded_host) against the CPU oracle's
world::hit, tolerance 0: every record field of every ray as raw 32-bit words (tests/query_rays.py says what is compared and how
NaNs are read), the final 48-byte stream states byte for byte.  The item loop (tree=False) and the unified tree with its per-ray
reach test (tree=True) must both give the oracle's answer on every set: primary, secondary, interval, far, axis.  No GPU."""
import json
import os
import subprocess

import numpy as np
import pytest

from mort_amd import hip
from tests import query_rays as Q

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MORT = os.path.join(ROOT, "mort_amd", "bin", "mort")


@pytest.mark.parametrize("name", sorted(Q.WORLDS))
def test_sets_show_something(name):
    """the census of tests/query_rays.py, on the oracle's answers alone"""
    Q.census(Q.build(name))


@pytest.mark.parametrize("tree", [False, True], ids=["items", "tree"])
@pytest.mark.parametrize("name", sorted(Q.WORLDS))
def test_closest_without_streams_equals_the_oracle(name, tree):
    s = Q.build(name)
    got = hip.query_closest_host(s.world, s.all, tree=tree, nthreads=4)["hits"]
    Q.assert_hits_equal(s.world, got, s.rec, s.hit, f"{name} tree={tree}")


@pytest.mark.parametrize("tree", [False, True], ids=["items", "tree"])
@pytest.mark.parametrize("name", sorted(Q.WORLDS))
def test_closest_with_streams_equals_the_oracle(name, tree):
    s = Q.build(name)
    streams = s.streams0.copy()
    got = hip.query_closest_host(s.world, s.all, states=streams, tree=tree, nthreads=4)["hits"]
    Q.assert_hits_equal(s.world, got, s.mrec, s.mhit, f"{name} tree={tree} with streams", with_media=True)
    assert streams.tobytes() == s.streams.tobytes(), f"{name} tree={tree}: final stream states differ from the oracle's"
    still = ~s.advanced  # a ray that draws nothing: identical bits
    assert (streams.view(np.uint8).reshape(-1, 48)[still] == s.streams0.view(np.uint8).reshape(-1, 48)[still]).all()


@pytest.mark.parametrize("tree", [False, True], ids=["items", "tree"])
@pytest.mark.parametrize("name", sorted(Q.WORLDS))
def test_occluded_equals_the_oracle(name, tree):
    s = Q.build(name)
    got = hip.query_occluded_host(s.world, s.all, tree=tree, nthreads=4)["occluded"]
    bad = np.flatnonzero(got != s.hit.astype(np.uint8))
    assert bad.size == 0, f"{name} tree={tree}: {bad.size} rays differ, first {bad[0]}: {s.all[bad[0]]} got {got[bad[0]]}"


def test_streams_untouched_words_keep_their_bits():
    """only d and v[] of a stream are written: the Box-Muller words keep the caller's bits, drawn from or not"""
    s = Q.build("scene7")
    streams = s.streams0.copy()
    raw = streams.view(np.uint8).reshape(-1, 48)
    raw[:, 24:] = 0xa5
    hip.query_closest_host(s.world, s.all, states=streams, tree=True)
    assert (raw[:, 24:] == 0xa5).all()
    assert (raw[:, :24] == s.streams.view(np.uint8).reshape(-1, 48)[:, :24]).all()


@pytest.mark.parametrize("sid,tree", [(1, False), (7, True), (9, True), (3, False)])
def test_pick_prints_the_record_under_the_pixel(sid, tree):
    """`mort <scene> --mode host --pick X,Y`: the feature pass's primary ray of the pixel, the same record as the oracle's"""
    if not os.path.exists(MORT):
        subprocess.check_call(["make", "-C", ROOT, "host", "hip", "cli"])
    s = Q.build(f"scene{sid}")
    # the scene as the CLI builds it at this width; Q.build may have turned its own camera, so the reference ray is rebuilt here
    from mort_amd import host
    from tests.feature_ref import primary_rays
    world, cam = host.build_scene(sid, width=48, spp=1)
    W, H = cam.image_width, cam.image_height
    rays = Q.ray8(primary_rays(cam), Q.INF)
    rec, hit = Q.oracle_closest(world, rays)
    picks = [(W // 2, H // 2), (3, H - 2), (W - 5, 1)] + ([(int(np.flatnonzero(hit)[0]) % W, int(np.flatnonzero(hit)[0]) // W)] if hit.any() else [])
    assert hit[[x + y * W for x, y in picks]].any(), "every picked pixel misses"
    for x, y in picks:
        args = [MORT, str(sid), "--mode", "host", "--width", "48", "--pick", f"{x},{y}"] + (["--tree"] if tree else [])
        p = subprocess.run(args, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        lines = p.stdout.strip().splitlines()
        assert len(lines) == 1, "one JSON line"
        j = json.loads(lines[0])
        i = x + y * W
        assert j["pick"] == [x, y] and j["hit"] == int(hit[i]) and j["mode"] == "host" and j["medium"] == 0
        got = np.zeros(1, dtype=hip.HIT_DTYPE)
        if j["hit"]:
            got["p"], got["normal"], got["t"], got["u"], got["v"] = j["p"], j["normal"], j["t"], j["u"], j["v"]
            got["mat_type"], got["mat_idx"] = j["mat_type"], j["mat_idx"]
            got["flags"] = 1 | (2 if j["front_face"] else 0)
        else:
            assert j["t"] == 0 and j["p"] == [0, 0, 0] and j["mat_type"] == 0
        Q.assert_hits_equal(world, got, rec[i:i + 1], hit[i:i + 1], f"scene {sid} --pick {x},{y}")
    p = subprocess.run([MORT, str(sid), "--mode", "host", "--width", "48", "--pick", f"{W},0"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "outside" in p.stderr
