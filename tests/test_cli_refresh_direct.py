"""`mort <scene> --mode host --sh-volume ... --cache-depth K --cache-direct | --cache-render-direct --refresh-direct R[,H[,KR[,S]]]`
(DESIGN.md 4.24): the JSON line and the frame equal what the Python host calls compose on scene 6 -- the full and the emission-only
bake, the subtraction, the pack, the direct rounds over rotated sets with the full bake's streams carried on, then the direct
cached query or the direct cached frames with every S-th probe refreshed between them; the option's refusals; and the older
refusals of --refresh beside the direct options, word for word.  No GPU."""
import json
import os
import subprocess

import numpy as np

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


class Composed:
    """the command line's volume in Python: the indirect records after R full direct rounds, the streams carried on"""

    def __init__(self, rounds, h, K):
        self.world, self.cam = host.build_scene(6, width=WIDTH, spp=SPP)
        sp = F(355) / F(2)
        self.g = g = hip.VOLUME_GRID((100, 100, 100), (sp, sp, F(355)), (3, 3, 2), 0.5)
        self.states = O.seed_states(S.DEFAULT_SEED, g.probes * DN, 1)
        bake = hip.probe_bake_indirect_host(self.world, hip.probe_params_from_camera(self.cam, DN), hip.volume_probes(g), self.states)
        self.records = hip.volume_pack_host(bake["sh_ind"])["records"]
        self.baked = self.records.copy()
        self.back = np.zeros_like(self.records)
        self.rounds, self.h, self.K = rounds, h, K
        self.ends = self.lit = 0
        for r in range(1, rounds + 1):
            got = self.round(r, 0, 1)
            self.ends, self.lit = int(got["ends"].sum()), int(got["lit"].sum())

    def round(self, r, first, step):
        """one round into the back buffer, which then becomes the records"""
        p = hip.REFRESH_PARAMS(hip.CACHED_PARAMS(hip.radiance_params_from_camera(self.cam, 1), self.K, self.g, None), DN, self.h, first, step)
        got = hip.volume_refresh_direct_host(self.world, p, self.states, self.records, None, records_out=self.back,
                                             dirs=hip.probe_directions_round(DN, r), nthreads=2)
        self.records, self.back = self.back, self.records
        return got

    def before_frame(self, f, stride):
        self.back[:] = self.records
        self.round(self.rounds + f, f % stride, stride)


def test_a_refreshed_probe_query_is_the_composed_one():
    c = Composed(2, 0.5, 0)
    assert (Q._words(c.records) != Q._words(c.baked)).any(), "the rounds changed nothing"
    W, H = c.cam.image_width, c.cam.image_height
    x, y, n = W // 2, H - 3, 4
    p = _run(BASE + ["--cache-depth", "0", "--cache-direct", "--refresh-direct", "2,0.5,0", "--probe", f"{x},{y},{n}", "--threads", "2"], spp=None)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    j = json.loads(lines[0])
    cam1 = host.build_scene(6, width=WIDTH, spp=1)[1]
    rays = Q.ray8(primary_rays(cam1), Q.INF)
    i = x + y * W
    st = np.ascontiguousarray(O.seed_states(S.DEFAULT_SEED, W, H)[[i]]).copy()
    cp = hip.CACHED_PARAMS(hip.radiance_params_from_camera(cam1, n), 0, c.g, None)
    want = hip.query_radiance_cached_direct_host(c.world, cp, rays[[i]], st, c.records, None, nthreads=2)
    assert (Q._words(np.array(j["rgb"], dtype=F)) == Q._words(want["rgb"][0])).all()
    assert j["ends"] == int(want["ends"][0]) and j["cache_direct"] == 1 and j["lit"] == int(want["lit"][0])
    assert (j["refresh_rounds"], j["hysteresis"], j["refresh_depth"], j["refresh_stride"]) == (2, 0.5, 0, 0)
    assert j["refresh_ends"] == c.ends > 0 and j["refresh_direct"] == 1 and j["refresh_lit"] == c.lit > 0
    keys = list(j)
    assert keys.index("refresh_ends") + 1 == keys.index("refresh_direct") == keys.index("refresh_lit") - 1
    # without the rounds the bake's records answer, and they answer differently
    unrefreshed = hip.query_radiance_cached_direct_host(c.world, cp, rays[[i]], np.ascontiguousarray(O.seed_states(S.DEFAULT_SEED, W, H)[[i]]).copy(),
                                                        c.baked, None, nthreads=2)
    assert (Q._words(unrefreshed["rgb"]) != Q._words(want["rgb"])).any()
    k = json.loads(_run(BASE + ["--cache-depth", "0", "--cache-direct", "--probe", f"{x},{y},{n}", "--threads", "2"], spp=None).stdout)
    assert (Q._words(np.array(k["rgb"], dtype=F)) == Q._words(unrefreshed["rgb"][0])).all() and "refresh_direct" not in k and "refresh_rounds" not in k


def _ppm(path, W, H):
    head = f"P6\n{W} {H}\n255\n".encode()
    data = path.read_bytes()
    assert data.startswith(head) and len(data) == len(head) + 3 * W * H
    return np.frombuffer(data[len(head):], dtype=np.uint8).reshape(H, W, 3)[::-1]


def test_the_last_of_three_refreshed_frames_is_the_composed_one(tmp_path):
    """--cache-render-direct --refresh-direct 1,0.75,0,2 --frames 3: one full round, then the probes 1, 3, ... before frame 1 and
    0, 2, ... before frame 2, with the sets of rounds 2 and 3"""
    c = Composed(1, 0.75, 0)
    W, H = c.cam.image_width, c.cam.image_height
    out, dump, sout = tmp_path / "frame.ppm", tmp_path / "frame.f32", tmp_path / "states.bin"
    p = _run(BASE + ["--cache-depth", "0", "--cache-render-direct", "--refresh-direct", "1,0.75,0,2", "--frames", "3", "--out", str(out), "--dump-f32",
                     str(dump), "--states-out", str(sout), "--threads", "2"])
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 4
    j = json.loads(lines[-1])
    fp = hip.CACHED_FRAME_PARAMS(0, c.g, None)
    states, frames, volumes = None, [], []
    for f in range(3):
        if f:
            c.before_frame(f, 2)
        volumes.append(c.records.copy())
        r = hip.render_cached_direct_host(c.world, c.cam, fp, c.records, None, states=states, nthreads=2)
        states = r["states"]
        frames.append(r)
    assert (Q._words(volumes[1]) != Q._words(volumes[0])).any() and (Q._words(volumes[2]) != Q._words(volumes[1])).any()
    assert (Q._words(volumes[1][0::2]) == Q._words(volumes[0][0::2])).all(), "frame 1 refreshes the odd probes alone"
    want = frames[2]
    assert (_ppm(out, W, H) == want["rgba"][..., :3]).all()
    assert dump.read_bytes() == want["accum"].tobytes() and sout.read_bytes() == want["states"].tobytes()
    assert j["segments"] == want["stats"]["segments"] and j["ends"] == int(want["ends_px"].sum()) and j["lit"] == int(want["lit_px"].sum())
    assert (j["refresh_rounds"], j["hysteresis"], j["refresh_depth"], j["refresh_stride"]) == (1, 0.75, 0, 2)
    assert j["refresh_ends"] == c.ends > 0 and j["refresh_direct"] == 1 and j["refresh_lit"] == c.lit > 0 and j["cache_direct"] == 1


def test_refusals():
    """every refusal has its own message and no stdout; --refresh beside the direct options is refused with the words it was"""
    cd = BASE + ["--cache-depth", "0", "--cache-direct", "--probe", "1,1"]
    crd = BASE + ["--cache-depth", "0", "--cache-render-direct"]

    def refused(args, words):
        r = _run(args)
        assert r.returncode != 0 and not r.stdout.strip() and words in r.stderr, (args, r.stderr)
        return r

    for base in (cd, crd):
        refused(base + ["--refresh-direct", "1", "--refresh", "1"], "--refresh-direct excludes --refresh")
    refused(BASE + ["--cache-depth", "0", "--cache-render", "--refresh-direct", "1"], "--refresh-direct excludes --cache-render:")
    for args in (BASE + ["--cache-depth", "0", "--probe", "1,1", "--refresh-direct", "1"], BASE + ["--pick", "1,1", "--refresh-direct", "1"],
                 ["--refresh-direct", "1"]):
        refused(args, "--refresh-direct needs --cache-direct or --cache-render-direct")
    refused(cd + ["--refresh-direct", "1,0.9,0,2"], "S > 0 only with --cache-render-direct")
    for bad in ("-1", "65536", "1,1.0", "1,-0.1", "1,nan", "1,0.5,-1", "1,0.5,65", "1,0.5,0,-1"):
        refused(crd + ["--refresh-direct", bad], "--refresh-direct: R in 0..65535")
    refused(crd + ["--refresh-direct", "x"], "--refresh-direct R[,H[,KR[,S]]]")
    r = _run(cd + ["--refresh", "1"])
    assert r.returncode != 0 and not r.stdout.strip() and r.stderr == "--cache-direct excludes --cache-render and --refresh\n"
    r = _run(crd + ["--refresh", "1"])
    assert r.returncode != 0 and not r.stdout.strip()
    assert r.stderr == ("--cache-render-direct excludes --refresh: a refresh through plain cached paths would put the emitters' light back into the "
                        "indirect volume\n")
