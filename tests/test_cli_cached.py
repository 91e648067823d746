"""`mort <scene> --mode host --sh-volume ... --cache-depth K`: the JSON line of --probe and the PPM of
--radiance-out equal what the Python calls compose for the same pixels on scene 6, and the option's refusals.  No GPU."""
import json
import os
import subprocess

import numpy as np
import pytest

from mort_amd import hip, host, structs as S
from tests import oracle_lib as O
from tests import query_rays as Q
from tests.feature_ref import primary_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORT = os.path.join(ROOT, "mort_amd", "bin", "mort")
F = np.float32
WIDTH, SPEC, DN = 24, "100,100,100,455,455,455,3,3,2", 64
BASE = ["--sh-volume", SPEC + f",{DN}"]


def _run(args):
    if not os.path.exists(MORT):
        subprocess.check_call(["make", "-C", ROOT, "host", "hip", "cli"])
    return subprocess.run([MORT, "6", "--mode", "host", "--width", str(WIDTH)] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def composed():
    """the command line's chain in Python: the grid, the baked and packed records, the depth maps for --visibility 5, the pixel
    rays and the pixel streams"""
    world, cam = host.build_scene(6, width=WIDTH, spp=1)
    sp = F(355) / F(2)
    g = hip.VOLUME_GRID((100, 100, 100), (sp, sp, F(355)), (3, 3, 2), 0.5)
    probes = hip.volume_probes(g)
    sh = hip.probe_bake_host(world, hip.probe_params_from_camera(cam, DN), probes, O.seed_states(S.DEFAULT_SEED, g.probes * DN, 1))["sh"]
    rec = hip.volume_pack_host(sh)["records"]
    cap = F(1.5 * np.sqrt(float(sp) ** 2 + float(sp) ** 2 + 355.0 ** 2))
    maps = hip.probe_depth_bake_host(world, hip.DEPTH_PARAMS(2, float(cap)), probes)["depth"]
    rays = Q.ray8(primary_rays(cam), Q.INF)
    streams = O.seed_states(S.DEFAULT_SEED, cam.image_width, cam.image_height)
    return world, cam, g, rec, maps, cap, rays, streams


def _cached(c, depth, samples, visible, idx=None):
    world, cam, g, rec, maps, cap, rays, streams = c
    p = hip.CACHED_PARAMS(hip.radiance_params_from_camera(cam, samples), depth, g, hip.VOLUME_VIS_PARAMS(5.0, 0.05) if visible else None)
    idx = np.arange(len(rays)) if idx is None else np.asarray(idx)
    return hip.query_radiance_cached_host(world, p, rays[idx], np.ascontiguousarray(streams[idx]).copy(), rec, maps if visible else None, nthreads=4)


@pytest.mark.parametrize("visible", [False, True])
def test_probe_prints_the_cached_colour(composed, visible):
    cam = composed[1]
    W, H = cam.image_width, cam.image_height
    vis = ["--visibility", "5"] if visible else []
    for (x, y, n), depth in (((W // 2, H // 2, None), 1), ((5, H - 3, 4), 0), ((W - 2, 1, 3), 2)):
        p = _run(BASE + vis + ["--cache-depth", str(depth), "--probe", f"{x},{y}" + (f",{n}" if n else "")])
        assert p.returncode == 0, p.stdout + p.stderr
        lines = p.stdout.strip().splitlines()
        assert len(lines) == 1, "one JSON line"
        j = json.loads(lines[0])
        i = x + y * W
        want = _cached(composed, depth, n or 1, visible, [i])
        assert j["probe"] == [x, y] and j["samples"] == (n or 1) and j["mode"] == "host" and j["cache_depth"] == depth
        assert j["probes"] == [3, 3, 2] and j["directions"] == DN and j["probe_samples"] == 1
        ray = np.array(j["origin"] + j["dir"] + [j["time"]], dtype=F)
        assert (ray.view(np.uint32) == composed[6][i, :7].view(np.uint32)).all()
        assert (Q._words(np.array(j["rgb"], dtype=F)) == Q._words(want["rgb"][0])).all(), (j, want)
        assert j["ends"] == int(want["ends"][0])
        assert ("normal_bias" in j) == visible
        if visible:
            assert F(j["normal_bias"]) == F(5.0) and F(j["min_visibility"]) == F(0.05) and j["depth_subsamples"] == 2 and F(j["max_distance"]) == composed[5]


@pytest.mark.parametrize("visible,spp", [(False, None), (True, 3)])
def test_radiance_out_is_the_composed_preview(composed, visible, spp, tmp_path):
    cam = composed[1]
    W, H = cam.image_width, cam.image_height
    out = tmp_path / "cached.ppm"
    args = BASE + (["--visibility", "5"] if visible else []) + ["--cache-depth", "1", "--radiance-out", str(out)] + (["--spp", str(spp)] if spp else [])
    p = _run(args)
    assert p.returncode == 0, p.stdout + p.stderr
    j = json.loads(p.stdout.strip())
    n = spp or 1
    want = _cached(composed, 1, n, visible)
    assert j["samples"] == n and j["cache_depth"] == 1 and j["ends"] == int(want["ends"].sum()) and j["ends"] > W * H * n // 4
    head = f"P6\n{W} {H}\n255\n".encode()
    data = out.read_bytes()
    assert data.startswith(head) and len(data) == len(head) + 3 * W * H
    img = np.frombuffer(data[len(head):], dtype=np.uint8).reshape(H, W, 3)[::-1].reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        v = (want["rgb"] / F(n)).astype(F)
        v = np.where(v > 0, v, F(0)).astype(F)  # NaN goes to 0
        v = np.where(v < 1, v, F(1)).astype(F)
        ref8 = (F(255.0) * np.sqrt(v) + F(0.5)).astype(F).astype(np.uint8)
    assert (img == ref8).all() and img.max() > 32


def test_refusals():
    """--cache-depth is valid only with --sh-volume and one of --probe / --radiance-out; without it --sh-volume refuses --probe
    as before"""
    r = _run(["--cache-depth", "1", "--probe", "1,1"])
    assert r.returncode != 0 and "--cache-depth needs --sh-volume" in r.stderr
    r = _run(BASE + ["--probe", "1,1"])
    assert r.returncode != 0 and "excludes --probe" in r.stderr
    for bad in (BASE + ["--cache-depth", "1"], BASE + ["--cache-depth", "1", "--pick", "1,1"],
                BASE + ["--cache-depth", "1", "--probe", "1,1", "--pick", "1,1"],
                BASE + ["--cache-depth", "1", "--irradiance-out", "x.ppm"],
                BASE + ["--cache-depth", "1", "--probe", "1,1", "--radiance-out", "x.ppm"],
                BASE + ["--cache-depth", "-1", "--probe", "1,1"], BASE + ["--cache-depth", "65", "--probe", "1,1"],
                BASE + ["--cache-depth", "x", "--probe", "1,1"], BASE + ["--cache-depth", "1", "--probe", f"0,{WIDTH}"],
                BASE + ["--radiance-out", "x.ppm"], ["--radiance-out", "x.ppm"]):
        r = _run(bad)
        assert r.returncode != 0 and not r.stdout.strip(), bad
