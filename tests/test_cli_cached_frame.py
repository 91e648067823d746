"""`mort <scene> --mode host --sh-volume ... --cache-depth K --cache-render`: the PPM and the JSON line equal what
the Python calls compose for the same frames on scene 6 -- alone, and with --temporal --svgf over two frames of a moving camera --
the new refusals, and --cache-depth without --cache-render refused as before.  No GPU."""
import json
import os
import subprocess

import numpy as np
import pytest

from mort_amd import hip, host, structs as S
from tests import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORT = os.path.join(ROOT, "mort_amd", "bin", "mort")
F = np.float32
WIDTH, SPP, SPEC, DN = 24, 4, "100,100,100,455,455,455,3,3,2", 64
BASE = ["--sh-volume", SPEC + f",{DN}"]


def _run(args, mode=("--mode", "host")):
    if not os.path.exists(MORT):
        subprocess.check_call(["make", "-C", ROOT, "host", "hip", "cli"])
    return subprocess.run([MORT, "6", *mode, "--width", str(WIDTH), "--spp", str(SPP)] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def composed():
    """the command line's bake in Python: the grid, the baked and packed records, the depth maps of --visibility 5"""
    world, cam = host.build_scene(6, width=WIDTH, spp=SPP)
    sp = F(355) / F(2)
    g = hip.VOLUME_GRID((100, 100, 100), (sp, sp, F(355)), (3, 3, 2), 0.5)
    probes = hip.volume_probes(g)
    sh = hip.probe_bake_host(world, hip.probe_params_from_camera(cam, DN), probes, O.seed_states(S.DEFAULT_SEED, g.probes * DN, 1))["sh"]
    rec = hip.volume_pack_host(sh)["records"]
    cap = F(1.5 * np.sqrt(float(sp) ** 2 + float(sp) ** 2 + 355.0 ** 2))
    maps = hip.probe_depth_bake_host(world, hip.DEPTH_PARAMS(2, float(cap)), probes)["depth"]
    return world, cam, g, rec, maps, cap


def _frames(c, depth, visible, frames, key=None):
    """the frames the command line renders: cached frames over continuing streams, input() between them"""
    world, cam0, g, rec, maps, _ = c
    cam = S.Camera.from_buffer_copy(cam0)
    p = hip.CACHED_FRAME_PARAMS(depth, g, hip.VOLUME_VIS_PARAMS(5.0, 0.05) if visible else None)
    states, out = None, []
    for f in range(frames):
        if f and key:
            host.camera_input(cam, key)
        r = hip.render_cached_host(world, cam, p, rec, maps if visible else None, states=states, nthreads=2)
        states = r["states"]
        r["cam"] = S.Camera.from_buffer_copy(cam)
        out.append(r)
    return out


def _ppm(path, W, H):
    head = f"P6\n{W} {H}\n255\n".encode()
    data = path.read_bytes()
    assert data.startswith(head) and len(data) == len(head) + 3 * W * H
    return np.frombuffer(data[len(head):], dtype=np.uint8).reshape(H, W, 3)[::-1]


def _report(p):
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert [ln.startswith("Avg. time per frame") for ln in lines[:-1]] == [True] * (len(lines) - 1)
    return json.loads(lines[-1]), len(lines) - 1


@pytest.mark.parametrize("visible,depth", [(False, 1), (True, 0), (True, 2)])
def test_a_cached_render_is_the_composed_frame(composed, visible, depth, tmp_path):
    cam = composed[1]
    W, H = cam.image_width, cam.image_height
    out, dump, sout = tmp_path / "frame.ppm", tmp_path / "frame.f32", tmp_path / "states.bin"
    args = BASE + (["--visibility", "5"] if visible else []) + ["--cache-depth", str(depth), "--cache-render", "--out", str(out), "--dump-f32", str(dump),
                                                                "--states-out", str(sout), "--threads", "2"]
    j, n_frames = _report(_run(args))
    want = _frames(composed, depth, visible, 1)[0]
    assert n_frames == 1
    assert (_ppm(out, W, H) == want["rgba"][..., :3]).all()
    assert dump.read_bytes() == want["accum"].tobytes() and sout.read_bytes() == want["states"].tobytes()
    # the render's own report ...
    assert (j["scene"], j["width"], j["height"], j["spp_nominal"], j["spp_effective"], j["depth"], j["mode"], j["gpus"]) == (6, W, H, SPP, SPP, cam.bounce_limit, "host", 1)
    assert j["segments"] == want["stats"]["segments"] == int(want["segments_px"].sum()) and j["kernel"] == want["stats"]["kernel_name"]
    # ... plus the cache's
    assert j["cache_depth"] == depth and j["ends"] == int(want["ends_px"].sum()) and j["ends"] > W * H * SPP // 4
    assert j["probes"] == [3, 3, 2] and j["directions"] == DN and j["probe_samples"] == 1 and j["bake_seconds"] > 0
    assert ("normal_bias" in j) == visible
    if visible:
        assert F(j["normal_bias"]) == F(5.0) and F(j["min_visibility"]) == F(0.05) and j["depth_subsamples"] == 2 and F(j["max_distance"]) == composed[5]
    plain = hip.render_host(composed[0], cam, nthreads=4)
    assert (plain["rgba"] != want["rgba"]).any(), "the cache changes the picture"


@pytest.mark.parametrize("visible", [False, True])
def test_two_frames_through_temporal_and_svgf(composed, visible, tmp_path):
    """--frames 2 --keys W --temporal --svgf: cached frames stand in for the renders, everything after them is the chain's"""
    world, cam = composed[0], composed[1]
    W, H = cam.image_width, cam.image_height
    out, var = tmp_path / "frame.ppm", tmp_path / "var.f32"
    args = BASE + (["--visibility", "5"] if visible else []) + ["--cache-depth", "1", "--cache-render", "--frames", "2", "--keys", "W", "--temporal", "--svgf",
                                                                "--out", str(out), "--variance-out", str(var), "--threads", "2"]
    j, n_frames = _report(_run(args))
    frames = _frames(composed, 1, visible, 2, key="W")
    assert n_frames == 2 and (frames[0]["cam"].center.e[2] != frames[1]["cam"].center.e[2] or frames[0]["cam"].center.e[0] != frames[1]["cam"].center.e[0])
    hist, prev, t = None, None, None
    for fr in frames:
        feat = hip.render_features_host(world, fr["cam"])
        t = hip.temporal_host(prev, fr["cam"], fr["accum"], feat["normal"], feat["depth"], hist)
        hist, prev = t["history"].copy(), fr["cam"]
    filt = hip.svgf_host(t["accum"], feat["albedo"], feat["normal"], feat["depth"], t["variance"])
    assert (_ppm(out, W, H) == filt["rgba"][..., :3]).all()
    assert var.read_bytes() == np.ascontiguousarray(t["variance"], dtype=F).tobytes()
    assert j["segments"] == frames[1]["stats"]["segments"] and j["ends"] == int(frames[1]["ends_px"].sum()) and j["cache_depth"] == 1
    assert "temporal_seconds" in j and "svgf_seconds" in j


def test_refusals():
    """--cache-render is valid only with --sh-volume and --cache-depth, on one GPU in the default mode or under --mode host, and
    excludes the no-render uses of the volume"""
    cr = BASE + ["--cache-depth", "1", "--cache-render"]
    r = _run(["--cache-render"])
    assert r.returncode != 0 and "--cache-render needs --sh-volume and --cache-depth" in r.stderr
    r = _run(BASE + ["--cache-render"])
    assert r.returncode != 0 and "--cache-render needs --sh-volume and --cache-depth" in r.stderr
    for extra in (["--probe", "1,1"], ["--radiance-out", "x.ppm"], ["--pick", "1,1"], ["--irradiance-out", "x.ppm"]):
        r = _run(cr + extra)
        assert r.returncode != 0 and "--cache-render excludes" in r.stderr and not r.stdout.strip(), extra
    for mode in (("--mode", "wave"), ("--mode", "throughput"), ("--gpus", "2")):
        r = _run(cr, mode=mode)
        assert r.returncode != 0 and "--cache-render is a single-GPU option" in r.stderr and not r.stdout.strip(), mode
    for bad in (BASE + ["--cache-depth", "-1", "--cache-render"], BASE + ["--cache-depth", "65", "--cache-render"],
                ["--sh-volume", "100,100,100,455,455,455,0,3,2", "--cache-depth", "1", "--cache-render"],
                ["--sh-volume", SPEC + ",63", "--cache-depth", "1", "--cache-render"], cr + ["--visibility", "-1"],
                cr + ["--svgf", "--denoise"], cr + ["--variance-out", "v.f32"]):
        r = _run(bad)
        assert r.returncode != 0 and not r.stdout.strip(), bad


def test_cache_depth_without_cache_render_is_refused_as_before():
    r = _run(BASE + ["--cache-depth", "1"])
    assert r.returncode != 0 and not r.stdout.strip()
    assert "--cache-depth needs --probe X,Y[,N] or --radiance-out FILE, not both, and excludes --pick and --irradiance-out" in r.stderr
    r = _run(BASE + ["--cache-depth", "1", "--pick", "1,1"])
    assert r.returncode != 0 and "--cache-depth needs --probe" in r.stderr
