"""`mort <scene> --mode host --sh-volume ... --cache-depth K --cache-render-direct`: the PPM and the JSON line equal
what the Python calls compose for the same frames on scene 6 -- the full and the emission-only bake, the subtraction, the pack, the
direct cached frames over continuing streams -- alone, and with --temporal --svgf over two frames of a moving camera; the option's
refusals; and --cache-render and --cache-direct lines that print what they printed.  No GPU."""
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
WIDTH, SPP, SPEC, DN = 24, 4, "100,100,100,455,455,455,3,3,2", 64
BASE = ["--sh-volume", SPEC + f",{DN}"]


def _run(args, mode=("--mode", "host"), spp=SPP):
    if not os.path.exists(MORT):
        subprocess.check_call(["make", "-C", ROOT, "host", "hip", "cli"])
    return subprocess.run([MORT, "6", *mode, "--width", str(WIDTH)] + (["--spp", str(spp)] if spp else []) + args, cwd=ROOT, capture_output=True, text=True,
                          timeout=300)


@pytest.fixture(scope="module")
def composed():
    """the command line's bakes in Python: the grid, the records of the full and of the indirect volume, the depth maps of
    --visibility 5"""
    world, cam = host.build_scene(6, width=WIDTH, spp=SPP)
    sp = F(355) / F(2)
    g = hip.VOLUME_GRID((100, 100, 100), (sp, sp, F(355)), (3, 3, 2), 0.5)
    probes = hip.volume_probes(g)
    bake = hip.probe_bake_indirect_host(world, hip.probe_params_from_camera(cam, DN), probes, O.seed_states(S.DEFAULT_SEED, g.probes * DN, 1))
    rec = {k: hip.volume_pack_host(bake[k])["records"] for k in ("sh_full", "sh_ind")}
    cap = F(1.5 * np.sqrt(float(sp) ** 2 + float(sp) ** 2 + 355.0 ** 2))
    maps = hip.probe_depth_bake_host(world, hip.DEPTH_PARAMS(2, float(cap)), probes)["depth"]
    return world, cam, g, rec, maps, cap


def _frames(c, depth, visible, frames, key=None, direct=True):
    """the frames the command line renders: (direct) cached frames over continuing streams, input() between them"""
    world, cam0, g, rec, maps, _ = c
    cam = S.Camera.from_buffer_copy(cam0)
    p = hip.CACHED_FRAME_PARAMS(depth, g, hip.VOLUME_VIS_PARAMS(5.0, 0.05) if visible else None)
    states, out = None, []
    for f in range(frames):
        if f and key:
            host.camera_input(cam, key)
        if direct:
            r = hip.render_cached_direct_host(world, cam, p, rec["sh_ind"], maps if visible else None, states=states, nthreads=2)
        else:
            r = hip.render_cached_host(world, cam, p, rec["sh_full"], maps if visible else None, states=states, nthreads=2)
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
def test_a_direct_cached_render_is_the_composed_frame(composed, visible, depth, tmp_path):
    cam = composed[1]
    W, H = cam.image_width, cam.image_height
    out, dump, sout = tmp_path / "frame.ppm", tmp_path / "frame.f32", tmp_path / "states.bin"
    tail = ["--out", str(out), "--dump-f32", str(dump), "--states-out", str(sout), "--threads", "2"]
    args = BASE + (["--visibility", "5"] if visible else []) + ["--cache-depth", str(depth)]
    j, n_frames = _report(_run(args + ["--cache-render-direct"] + tail))
    want = _frames(composed, depth, visible, 1)[0]
    assert n_frames == 1
    assert (_ppm(out, W, H) == want["rgba"][..., :3]).all()
    assert dump.read_bytes() == want["accum"].tobytes() and sout.read_bytes() == want["states"].tobytes()
    assert (j["scene"], j["width"], j["height"], j["spp_nominal"], j["spp_effective"], j["depth"], j["mode"], j["gpus"]) == (6, W, H, SPP, SPP, cam.bounce_limit, "host", 1)
    assert j["segments"] == want["stats"]["segments"] == int(want["segments_px"].sum()) and j["kernel"] == want["stats"]["kernel_name"]
    assert "cached frame, direct" in j["kernel"]
    assert j["cache_depth"] == depth and j["ends"] == int(want["ends_px"].sum()) and j["ends"] > W * H * SPP // 4
    assert j["cache_direct"] == 1 and j["lit"] == int(want["lit_px"].sum()) and 0 < j["lit"] < j["ends"]
    assert j["probes"] == [3, 3, 2] and j["directions"] == DN and j["probe_samples"] == 1 and j["bake_seconds"] > 0
    assert ("normal_bias" in j) == visible
    # the same line with --cache-render: the cached frame over the full volume, no new field, nothing else moves
    ppm_direct = out.read_bytes()
    k, _ = _report(_run(args + ["--cache-render"] + tail))
    plain = _frames(composed, depth, visible, 1, direct=False)[0]
    assert "cache_direct" not in k and "lit" not in k
    assert [key for key in j if key not in ("cache_direct", "lit")] == list(k), "the new fields come after ends"
    assert (_ppm(out, W, H) == plain["rgba"][..., :3]).all() and dump.read_bytes() == plain["accum"].tobytes() and sout.read_bytes() == plain["states"].tobytes()
    assert k["segments"] == plain["stats"]["segments"] and k["ends"] == int(plain["ends_px"].sum()) and k["kernel"] == plain["stats"]["kernel_name"]
    assert out.read_bytes() != ppm_direct, "the two estimators differ"


@pytest.mark.parametrize("visible", [False, True])
def test_two_frames_through_temporal_and_svgf(composed, visible, tmp_path):
    """--frames 2 --keys W --temporal --svgf: direct cached frames stand in for the renders, everything after them is the chain's"""
    world, cam = composed[0], composed[1]
    W, H = cam.image_width, cam.image_height
    out, var = tmp_path / "frame.ppm", tmp_path / "var.f32"
    args = BASE + (["--visibility", "5"] if visible else []) + ["--cache-depth", "0", "--cache-render-direct", "--frames", "2", "--keys", "W", "--temporal",
                                                                "--svgf", "--out", str(out), "--variance-out", str(var), "--threads", "2"]
    j, n_frames = _report(_run(args))
    frames = _frames(composed, 0, visible, 2, key="W")
    assert n_frames == 2
    hist, prev, t = None, None, None
    for fr in frames:
        feat = hip.render_features_host(world, fr["cam"])
        t = hip.temporal_host(prev, fr["cam"], fr["accum"], feat["normal"], feat["depth"], hist)
        hist, prev = t["history"].copy(), fr["cam"]
    filt = hip.svgf_host(t["accum"], feat["albedo"], feat["normal"], feat["depth"], t["variance"])
    assert (_ppm(out, W, H) == filt["rgba"][..., :3]).all()
    assert var.read_bytes() == np.ascontiguousarray(t["variance"], dtype=F).tobytes()
    assert j["segments"] == frames[1]["stats"]["segments"] and j["ends"] == int(frames[1]["ends_px"].sum()) and j["lit"] == int(frames[1]["lit_px"].sum())
    assert j["cache_depth"] == 0 and j["cache_direct"] == 1 and "temporal_seconds" in j and "svgf_seconds" in j


def test_a_denoised_frame(composed, tmp_path):
    """--denoise over a direct cached frame"""
    world, cam = composed[0], composed[1]
    W, H = cam.image_width, cam.image_height
    out = tmp_path / "frame.ppm"
    j, _ = _report(_run(BASE + ["--cache-depth", "1", "--cache-render-direct", "--denoise", "--out", str(out), "--threads", "2"]))
    fr = _frames(composed, 1, False, 1)[0]
    feat = hip.render_features_host(world, fr["cam"])
    assert (_ppm(out, W, H) == hip.denoise_host(fr["accum"], feat["albedo"], feat["normal"], feat["depth"])["rgba"][..., :3]).all()
    assert j["lit"] == int(fr["lit_px"].sum()) and "denoise_seconds" in j


def test_refusals():
    """--cache-render-direct needs --sh-volume and --cache-depth, one GPU in the default mode or --mode host, and excludes
    --cache-render, --cache-direct, the no-render uses of the volume and --refresh; every refusal has a message and no stdout"""
    crd = BASE + ["--cache-depth", "1", "--cache-render-direct"]
    for args in (["--cache-render-direct"], BASE + ["--cache-render-direct"]):
        r = _run(args)
        assert r.returncode != 0 and not r.stdout.strip() and "--cache-render-direct needs --sh-volume and --cache-depth" in r.stderr, args
    r = _run(["--cache-depth", "1", "--cache-render-direct"])
    assert r.returncode != 0 and not r.stdout.strip() and r.stderr.strip()
    for extra in (["--cache-render"], ["--cache-direct"], ["--cache-direct", "--probe", "1,1"]):
        r = _run(crd + extra)
        assert r.returncode != 0 and not r.stdout.strip() and "--cache-render-direct excludes --cache-render and --cache-direct" in r.stderr, extra
    for extra in (["--probe", "1,1"], ["--radiance-out", "x.ppm"], ["--pick", "1,1"], ["--irradiance-out", "x.ppm"]):
        r = _run(crd + extra)
        assert r.returncode != 0 and not r.stdout.strip() and "--cache-render-direct excludes --probe, --radiance-out" in r.stderr, extra
    for mode in (("--mode", "wave"), ("--mode", "throughput"), ("--gpus", "2")):
        r = _run(crd, mode=mode)
        assert r.returncode != 0 and not r.stdout.strip() and "--cache-render-direct is a single-GPU option" in r.stderr, mode
    for extra in (["--refresh", "1"], ["--refresh", "0,0.9,0,2"]):
        r = _run(crd + extra)
        assert r.returncode != 0 and not r.stdout.strip() and "--cache-render-direct excludes --refresh" in r.stderr and "emitters' light back" in r.stderr, extra
    for bad in (BASE + ["--cache-depth", "-1", "--cache-render-direct"], BASE + ["--cache-depth", "65", "--cache-render-direct"],
                ["--sh-volume", SPEC + ",63", "--cache-depth", "1", "--cache-render-direct"], crd + ["--visibility", "-1"], crd + ["--svgf", "--denoise"]):
        r = _run(bad)
        assert r.returncode != 0 and not r.stdout.strip() and r.stderr.strip(), bad


def test_the_older_lines_print_what_they_printed(composed):
    """--cache-direct --probe prints the direct-light cached query's colour, as it did; --cache-direct --cache-render is refused with
    the words it was refused with; --cache-depth alone is refused as before"""
    world, cam, g, rec = composed[:4]
    W, H = cam.image_width, cam.image_height
    x, y, n = W // 2, H - 3, 4
    p = _run(BASE + ["--cache-depth", "0", "--probe", f"{x},{y},{n}", "--cache-direct"], spp=None)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    j = json.loads(lines[0])
    cam1 = host.build_scene(6, width=WIDTH, spp=1)[1]
    rays = Q.ray8(primary_rays(cam1), Q.INF)
    i = x + y * W
    st = np.ascontiguousarray(O.seed_states(S.DEFAULT_SEED, W, H)[[i]]).copy()
    want = hip.query_radiance_cached_direct_host(world, hip.CACHED_PARAMS(hip.radiance_params_from_camera(cam1, n), 0, g, None), rays[[i]], st, rec["sh_ind"],
                                                 None, nthreads=2)
    assert (Q._words(np.array(j["rgb"], dtype=F)) == Q._words(want["rgb"][0])).all()
    assert j["ends"] == int(want["ends"][0]) and j["cache_direct"] == 1 and j["lit"] == int(want["lit"][0])
    r = _run(BASE + ["--cache-depth", "1", "--cache-direct", "--cache-render"])
    assert r.returncode != 0 and not r.stdout.strip() and r.stderr == "--cache-direct excludes --cache-render and --refresh\n"
    r = _run(BASE + ["--cache-depth", "1"])
    assert r.returncode != 0 and not r.stdout.strip()
    assert "--cache-depth needs --probe X,Y[,N] or --radiance-out FILE, not both, and excludes --pick and --irradiance-out" in r.stderr
