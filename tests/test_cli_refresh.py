"""`mort <scene> --mode host --sh-volume ... --refresh R[,H[,KR[,S]]]`: the PPM of --irradiance-out, the JSON line
of --cache-depth K --probe X,Y and the frames of --cache-render equal what the Python host calls compose for scene 6, byte for byte,
and the option's refusals.  No GPU."""
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


def _run(args, width=WIDTH):
    if not os.path.exists(MORT):
        subprocess.check_call(["make", "-C", ROOT, "host", "hip", "cli"])
    return subprocess.run([MORT, "6", "--mode", "host", "--width", str(width)] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)


class Chain:
    """the command line's chain in Python: the grid, the bake, the maps for --visibility 5, then the rounds"""

    def __init__(self, visible, spp=1):
        self.world, self.cam = host.build_scene(6, width=WIDTH, spp=spp)
        sp = F(355) / F(2)
        self.g = g = hip.VOLUME_GRID((100, 100, 100), (sp, sp, F(355)), (3, 3, 2), 0.5)
        probes = hip.volume_probes(g)
        self.streams = O.seed_states(S.DEFAULT_SEED, g.probes * DN, 1)
        sh = hip.probe_bake_host(self.world, hip.probe_params_from_camera(self.cam, DN), probes, self.streams)["sh"]
        self.records = hip.volume_pack_host(sh)["records"]
        cap = F(1.5 * np.sqrt(float(sp) ** 2 + float(sp) ** 2 + 355.0 ** 2))
        self.maps = hip.probe_depth_bake_host(self.world, hip.DEPTH_PARAMS(2, float(cap)), probes)["depth"] if visible else None
        self.vis = hip.VOLUME_VIS_PARAMS(5.0, 0.05) if visible else None
        self.ends = 0

    def round(self, r, h, depth, first=0, step=1):
        """one round with the set of round r; the unselected records are carried over"""
        c = hip.CACHED_PARAMS(hip.radiance_params_from_camera(self.cam, 1), depth, self.g, self.vis)
        p = hip.REFRESH_PARAMS(c, DN, h, first, step)
        got = hip.volume_refresh_host(self.world, p, self.streams, self.records, self.maps, records_out=self.records.copy(),
                                      dirs=hip.probe_directions_round(DN, r), nthreads=4)
        self.records = got["records"]
        return int(got["ends"][first::step].sum())

    def rounds(self, R, h, depth):
        for r in range(1, R + 1):
            self.ends = self.round(r, h, depth)
        return self


@pytest.mark.parametrize("visible", [False, True])
def test_irradiance_out_after_two_rounds(visible, tmp_path):
    c = Chain(visible).rounds(2, 0.5, 0)
    W, H = c.cam.image_width, c.cam.image_height
    out = tmp_path / "irr.ppm"
    p = _run(BASE + (["--visibility", "5"] if visible else []) + ["--refresh", "2,0.5,0", "--irradiance-out", str(out)])
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, "one JSON line"
    j = json.loads(lines[0])
    assert (j["refresh_rounds"], j["refresh_depth"], j["refresh_stride"], j["refresh_ends"]) == (2, 0, 0, c.ends) and F(j["hysteresis"]) == F(0.5)
    assert c.ends > 0 and j["probes"] == [3, 3, 2] and j["directions"] == DN and j["samples"] == 1 and j["mode"] == "host"
    plain = _run(BASE + (["--visibility", "5"] if visible else []) + ["--irradiance-out", str(tmp_path / "plain.ppm")])
    jp = json.loads(plain.stdout.strip())
    assert [k for k in j if k not in jp] == ["refresh_rounds", "hysteresis", "refresh_depth", "refresh_stride", "refresh_ends"]
    assert all(j[k] == jp[k] for k in jp if not k.endswith("seconds") and k != "irradiance_out")
    rays = Q.ray8(primary_rays(c.cam), Q.INF)
    hits = hip.query_closest_host(c.world, rays)["hits"]
    if visible:
        irr = hip.volume_sample_visible_host(c.g, c.records, c.maps, c.vis, hits)["out"]
    else:
        irr = hip.volume_sample_host(c.g, c.records, hits)["out"]
    irr = np.where(((hits["flags"] & hip.HIT_HIT) != 0)[:, None], irr, F(0)).astype(F)
    with np.errstate(invalid="ignore"):
        v = (irr[:, :3] * F(0.318309886)).astype(F)
        v = np.where(v > 0, v, F(0)).astype(F)  # NaN goes to 0
        v = np.where(v < 1, v, F(1)).astype(F)
        ref8 = (F(255.0) * np.sqrt(v) + F(0.5)).astype(F).astype(np.uint8)
    head = f"P6\n{W} {H}\n255\n".encode()
    want = head + ref8.reshape(H, W, 3)[::-1].tobytes()  # the file's first row is the top row
    assert out.read_bytes() == want
    assert out.read_bytes() != (tmp_path / "plain.ppm").read_bytes(), "the rounds show"


@pytest.mark.parametrize("visible", [False, True])
def test_probe_after_the_rounds(visible):
    c = Chain(visible).rounds(3, 0.9, 1)
    W, H = c.cam.image_width, c.cam.image_height
    rays = Q.ray8(primary_rays(c.cam), Q.INF)
    streams = O.seed_states(S.DEFAULT_SEED, W, H)
    for (x, y, n) in ((W // 2, H // 2, 1), (5, H - 3, 4)):
        p = _run(BASE + (["--visibility", "5"] if visible else []) + ["--cache-depth", "1", "--refresh", "3,0.9,1", "--probe", f"{x},{y},{n}"])
        assert p.returncode == 0, p.stdout + p.stderr
        j = json.loads(p.stdout.strip())
        i = x + y * W
        q = hip.CACHED_PARAMS(hip.radiance_params_from_camera(c.cam, n), 1, c.g, c.vis)
        want = hip.query_radiance_cached_host(c.world, q, rays[[i]], np.ascontiguousarray(streams[[i]]).copy(), c.records, c.maps)
        assert (Q._words(np.array(j["rgb"], dtype=F)) == Q._words(want["rgb"][0])).all(), (j, want)
        assert j["ends"] == int(want["ends"][0]) and j["cache_depth"] == 1
        assert (j["refresh_rounds"], j["refresh_depth"], j["refresh_stride"], j["refresh_ends"]) == (3, 1, 0, c.ends)
        assert F(j["hysteresis"]) == F(0.9)
    # H and KR default to 0.9 and 0
    d = json.loads(_run(BASE + ["--cache-depth", "1", "--refresh", "1", "--probe", "3,3"]).stdout.strip())
    assert F(d["hysteresis"]) == F(0.9) and d["refresh_depth"] == 0 and d["refresh_stride"] == 0 and d["refresh_rounds"] == 1


def test_cache_render_with_a_round_before_every_frame(tmp_path):
    """--cache-render --refresh 1,0.75,0,2 over three frames: one full round, then before frames 1 and 2 every second probe once more
    with the sets of rounds 2 and 3; the last frame is the host form's cached frame over those records"""
    c = Chain(True, spp=4).rounds(1, 0.75, 0)
    full = c.ends
    W, H = c.cam.image_width, c.cam.image_height
    fp = hip.CACHED_FRAME_PARAMS(1, c.g, c.vis)
    states = hip.seed_states_host(S.DEFAULT_SEED, W, H)
    for f in range(3):
        if f:
            c.round(1 + f, 0.75, 0, first=f % 2, step=2)
        r = hip.render_cached_host(c.world, c.cam, fp, c.records, c.maps, states=states, nthreads=4)
        states = r["states"]
    out = tmp_path / "frame.ppm"
    p = _run(BASE + ["--visibility", "5", "--cache-depth", "1", "--cache-render", "--refresh", "1,0.75,0,2", "--spp", "4", "--frames", "3", "--threads", "4",
                     "--out", str(out)])
    assert p.returncode == 0, p.stdout + p.stderr
    j = json.loads(p.stdout.strip().splitlines()[-1])
    assert (j["refresh_rounds"], j["refresh_depth"], j["refresh_stride"], j["refresh_ends"]) == (1, 0, 2, full) and F(j["hysteresis"]) == F(0.75)
    assert j["ends"] == int(r["ends_px"].sum()) and j["segments"] == r["stats"]["segments"]
    head = f"P6\n{W} {H}\n255\n".encode()
    assert out.read_bytes() == head + r["rgba"][::-1, :, :3].tobytes()
    still = _run(BASE + ["--visibility", "5", "--cache-depth", "1", "--cache-render", "--refresh", "1,0.75,0", "--spp", "4", "--frames", "3", "--threads", "4",
                         "--out", str(tmp_path / "still.ppm")])
    assert still.returncode == 0 and (tmp_path / "still.ppm").read_bytes() != out.read_bytes(), "the rounds between the frames show"


def test_refusals():
    """--refresh is valid only with --sh-volume; R, H, KR and S are checked; S > 0 needs --cache-render"""
    r = _run(["--refresh", "2"])
    assert r.returncode != 0 and "--refresh needs --sh-volume" in r.stderr
    r = _run(["--refresh", "2", "--pick", "1,1"])
    assert r.returncode != 0 and "--refresh needs --sh-volume" in r.stderr
    for bad in ("x", "-1", "65536", "2,1.0", "2,-0.1", "2,nan", "2,inf", "2,0.5,-1", "2,0.5,65", "2,0.5,0,-1", "2,0.5,0,2"):
        r = _run(BASE + ["--pick", "1,1", "--refresh", bad])
        assert r.returncode != 0 and not r.stdout.strip(), bad
    r = _run(BASE + ["--cache-depth", "1", "--probe", "1,1", "--refresh", "2,0.5,0,3"])
    assert r.returncode != 0 and "only with --cache-render" in r.stderr
    # --refresh does not stand in for what --sh-volume needs
    assert _run(BASE + ["--refresh", "2"]).returncode != 0
    ok = _run(BASE + ["--pick", "1,1", "--refresh", "0"])
    assert ok.returncode == 0 and json.loads(ok.stdout.strip())["refresh_ends"] == 0
