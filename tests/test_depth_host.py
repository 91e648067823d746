"""Visibility-weighted irradiance volumes on the host (mort_hip_probe_depth_bake_host, mort_hip_volume_sample_visible_host,
dev_depth.h) against the contract restated in numpy over the oracle's distances (tests/depth_ref.py) at tolerance
0 -- outputs as raw 32-bit words, any NaN equal to any NaN -- and against things that are not the contract: the distance inside a
lone sphere, the plain sampler where nothing is occluded, a wall between two probes.  The command line.  No GPU."""
import json
import os
import subprocess

import numpy as np
import pytest

from mort_amd import hip, host, structs as S
from tests import depth_cases as DC
from tests import depth_ref as D
from tests import oracle_lib as O
from tests import volume_cases as K
from tests import volume_ref as V
from tests import worlds as Wd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORT = os.path.join(ROOT, "mort_amd", "bin", "mort")
F = np.float32
U = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- the bake

@pytest.mark.parametrize("s", DC.SUBSAMPLES)
@pytest.mark.parametrize("name", DC.WORLDS)
def test_bake_equals_the_restatement_over_the_oracle(name, s):
    w = DC.world(name)[0]
    want = DC.maps(name, s)
    trees = (False, True) if DC.has_tree(name) else (False,)
    for tree in trees:
        for nthreads in (1, 3):
            got = hip.probe_depth_bake_host(w, DC.params(name, s), DC.probes(name), tree=tree, nthreads=nthreads)["depth"]
            assert got.shape == (DC.N_PROBES, hip.DEPTH_FLOATS) and got.dtype == F
            DC.same(got, want, f"{name} s {s} tree {tree} threads {nthreads}")


def test_the_inputs_of_the_bake_tests_show_something():
    """A check of the fixtures, not of the library (it calls nothing of the feature): on the restatement over the oracle alone,
    both tree choices are exercised, rays end below and at the cap, the probe inside the tall box sees nothing beyond the box, the
    far and the NaN probe see nothing at all"""
    assert DC.has_tree("genrandom:scales_150_s0") and not DC.has_tree("scene1")
    for name in DC.WORLDS:
        cap = DC.world(name)[2]
        m1 = DC.maps(name, 1).reshape(DC.N_PROBES, D.SIDE, D.SIDE, 2)[:, 1:9, 1:9, 0]
        assert np.isfinite(DC.maps(name, 3)).all()
        assert 0.1 < float((m1 < cap).mean()) < 0.9, name
        assert (m1[3] == cap).all() and (m1[4] == cap).all(), "nothing within the cap a million away; a NaN origin hits nothing"
        assert np.isnan(DC.probes(name)["position"][4]).any() and np.abs(DC.probes(name)["position"][3]).max() >= 1e6
    inside6, inside7 = (DC.maps(name, 2).reshape(DC.N_PROBES, D.SIDE, D.SIDE, 2)[2, 1:9, 1:9, 0] for name in ("scene6", "scene7"))
    assert inside6.max() < 400 and DC.world("scene6")[2] > 500, "330 tall, 165 wide: every wall of the box is nearer than the cap"
    # scene 7's boxes are constant media, which the bake passes over: the same probe sees the room's walls through the box
    assert len(DC.Q._media(DC.world("scene7")[0])) == 2 and inside7.mean() > 2 * inside6.mean() and (inside7 > 400).any()


@pytest.mark.parametrize("name", DC.WORLDS)
def test_border_texels_equal_their_sources(name):
    w = DC.world(name)[0]
    m = hip.probe_depth_bake_host(w, DC.params(name, 2), DC.probes(name), nthreads=2)["depth"].view(np.uint32).reshape(DC.N_PROBES, 10, 10, 2)
    t = lambda i, j: m[:, j, i]  # noqa: E731  texel (i, j) sits at float 2 (j 10 + i)
    for k in range(1, 9):
        assert (t(0, k) == t(1, 9 - k)).all() and (t(9, k) == t(8, 9 - k)).all()
        assert (t(k, 0) == t(9 - k, 1)).all() and (t(k, 9) == t(9 - k, 8)).all()
    assert (t(0, 0) == t(8, 8)).all() and (t(9, 9) == t(1, 1)).all() and (t(0, 9) == t(8, 1)).all() and (t(9, 0) == t(1, 8)).all()


def test_inside_a_lone_sphere_every_texel_is_the_radius():
    """Not the contract: a probe exactly at the centre of a sphere of radius rho sees rho in every direction, so every interior
    texel is (rho, rho^2).  The bound, first order in u = 2^-24 (relative), from the operation count of one ray with oc = 0:
    a = (x x + y y) + z z carries 3 (a product and two sums above it, all terms positive); c = 0 - rho rho 1; the discriminant
    0 - a c 3 + 1 + 1 = 5; its square root 5 / 2 + 1 = 3.5; the far root (0 + sqrtd) / a 3.5 + 3 + 1 = 7.5; len = sqrt(a) 3 / 2 + 1
    = 2.5; d = t len 7.5 + 2.5 + 1 = 11.  m1: s^2 - 1 additions of positive terms and the product with inv (itself rounded) add
    s^2 - 1 + 2, and 1 for the second order: (13 + s^2) u rho.  m2: d d 2 x 11 + 1 = 23, the same sum and scale, 1 for the second
    order: (25 + s^2) u rho^2."""
    rho, centre = 1.7, (0.3, -1.2, 2.5)
    w, _ = Wd.flat_world([("sphere", centre, rho, ("lamb", (.5, .5, .5)))])
    pr = np.zeros(1, dtype=hip.PROBE_DTYPE)
    pr["position"][0], pr["time"] = centre, 0.5
    rho32 = float(F(rho))
    worst = [0.0, 0.0]
    for s in (1, 2, 3):
        m = hip.probe_depth_bake_host(w, hip.DEPTH_PARAMS(s, 10.0), pr)["depth"].reshape(10, 10, 2)[1:9, 1:9].astype(np.float64)
        e1 = np.abs(m[..., 0] - rho32).max() / (U * rho32)
        e2 = np.abs(m[..., 1] - rho32 * rho32).max() / (U * rho32 * rho32)
        print(f"s {s}: worst m1 {e1:.2f} u rho (bound {13 + s * s}), worst m2 {e2:.2f} u rho^2 (bound {25 + s * s})")
        worst = [max(worst[0], e1), max(worst[1], e2)]
        assert e1 <= 13 + s * s and e2 <= 25 + s * s
    print(f"lone sphere: worst m1 {worst[0]:.2f} u rho, worst m2 {worst[1]:.2f} u rho^2")


# ------------------------------------------------------------------------------------------------------------- the sampler

def _visible(g, rec, maps, bias, minv, pts, stride=None, nthreads=1):
    return hip.volume_sample_visible_host(g, rec, maps, hip.VOLUME_VIS_PARAMS(bias, minv), pts, stride=stride, nthreads=nthreads)["out"]


@pytest.mark.parametrize("count", K.COUNTS)
def test_sampler_equals_the_restatement(count):
    g = K.grid(count)
    maps = DC.random_maps(g)
    pts = DC.sampler_points(g)
    assert not np.isfinite(pts).all() and np.abs(pts[np.isfinite(pts).all(1), :3]).max() > 1e30
    for mask in ("ones", "holes", "fractional"):
        rec = K.records(g, mask)
        m = maps.copy()
        if mask == "holes":  # NaN behind a zero weight, in the map as well: neither may influence the result
            m[rec[:, 27] == 0] = np.nan
        for bias, minv in ((0.0, 0.0), (0.25, 0.05), (0.0, 0.05), (0.25, 0.0)):
            census = {}
            want = D.sample_visible(g, rec, m, bias, minv, pts[:, :3], pts[:, 3:], census=census)
            DC.same(_visible(g, rec, m, bias, minv, pts, nthreads=3 if bias else 1), want, f"grid {count} {mask} bias {bias} min {minv}")
            if min(count) > 1:
                assert 0.1 < census["beyond"] / census["evaluated"] < 0.9, census
        if mask == "holes":
            filled = m.copy()
            filled[rec[:, 27] == 0] = 0.5
            frec = rec.copy()
            frec[rec[:, 27] == 0, :27] = 7.5
            DC.same(_visible(g, frec, filled, 0.25, 0.05, pts), _visible(g, rec, m, 0.25, 0.05, pts), "NaN behind a zero weight")


def test_sampler_strides():
    g = K.grid((4, 3, 2))
    rec, maps = K.records(g, "fractional"), DC.random_maps(g)
    pts = DC.sampler_points(g, 300)
    want = D.sample_visible(g, rec, maps, 0.1, 0.05, pts[:, :3], pts[:, 3:])
    DC.same(_visible(g, rec, maps, 0.1, 0.05, pts), want, "stride 24")
    DC.same(_visible(g, rec, maps, 0.1, 0.05, K.strided(pts, 40, 0xff), stride=40), want, "stride 40, NaN words between the points")
    DC.same(_visible(g, rec, maps, 0.1, 0.05, K.strided(pts, 48), stride=48, nthreads=2), want, "stride 48")


def test_a_point_exactly_at_a_probe():
    """s1 = 0: that corner's V is 1 whatever its map holds"""
    g = K.grid((4, 3, 2))
    rec = K.records(g)
    pts = DC.exact_points(g)
    zero = np.zeros((g.probes, hip.DEPTH_FLOATS), dtype=F)  # m1 = 0 everywhere: every other corner is beyond its map
    got = _visible(g, rec, zero, 0.0, 0.0, pts)
    DC.same(got, D.sample_visible(g, rec, zero, 0.0, 0.0, pts[:, :3], pts[:, 3:]), "at the probes")
    assert (got[:, 3] > 0).all(), "the probe the point sits on still counts"


@pytest.mark.parametrize("count", K.COUNTS)
def test_with_every_m1_flt_max_it_is_the_plain_sampler(count):
    """r > FLT_MAX needs r = +inf: the points whose squared offset overflows (coordinates beyond 1.8e19) are compared with the
    restatement alone, every other point with mort_hip_volume_sample_host, as words"""
    g = K.grid(count)
    pts = DC.sampler_points(g)
    maps = DC.flt_max_maps(g)
    for mask in ("ones", "fractional", "holes"):
        rec = K.records(g, mask)
        got = _visible(g, rec, maps, 0.25, 0.05, pts)
        DC.same(got, D.sample_visible(g, rec, maps, 0.25, 0.05, pts[:, :3], pts[:, 3:]), "the restatement")
        plain = hip.volume_sample_host(g, rec, pts)["out"]
        with np.errstate(invalid="ignore", over="ignore"):
            near = ~(np.abs(pts[:, :3]) > 1e18).any(1)
        assert near.sum() >= 600 and np.isnan(pts[near, :3]).any()
        DC.same(got[near], plain[near], f"identity, grid {count} {mask}")


def test_scene_6_maps_and_census():
    """maps baked in scene 6 by the host form, sampled at the scene's hits (stride 48: the hit records as they are).  The census,
    on the restatement alone: of the corner evaluations (T weight > 0) both sides of r > m1 hold at least a tenth"""
    world, cam, rays, hits = K.scene6()
    g, want_maps = DC.scene6_maps()
    maps = hip.probe_depth_bake_host(world, hip.DEPTH_PARAMS(2, float(DC.SCENE6_CAP)), hip.volume_probes(g), nthreads=4)["depth"]
    DC.same(maps, want_maps, "scene 6 grid maps")
    rec = K.records(g, "ones", seed=9)
    for bias, minv in ((5.0, 0.05), (0.0, 0.0)):
        want = D.sample_visible(g, rec, maps, bias, minv, hits["p"], hits["normal"])
        DC.same(_visible(g, rec, maps, bias, minv, hits, nthreads=4), want, f"scene 6 hits bias {bias}")
        census, hit = {}, (hits["flags"] & hip.HIT_HIT) != 0  # the census over the hit points alone: a miss is a zero record
        D.sample_visible(g, rec, maps, bias, minv, hits["p"][hit], hits["normal"][hit], census=census)
        beyond, dimmed = census["beyond"] / census["evaluated"], census["dimmed"] / census["evaluated"]
        print(f"scene 6 census, bias {bias} min {minv}: {census['evaluated']} corner evaluations, r > m1 in {beyond:.4f}, V < 1 in {dimmed:.4f}")
        assert 0.1 <= beyond <= 0.9 and dimmed > 0.05, census
    plain = hip.volume_sample_host(g, rec, hits)["out"]
    assert (K.words(plain) != K.words(want)).any(1).mean() > 0.1, "the visibility changes the picture"


def test_a_wall_between_two_probes_stops_the_leak():
    """Not the contract: grid (2, 1, 1), probe 0 bright, probe 1 dark behind a wall at 0.6 of the cell, points at 0.3.  The plain
    sampler gives probe 1 a share of 0.3 of the weights' sum; with min_visibility = 0 the share measured on the restatement
    is 2.1e-3 at the worst, and the library's must stay below ten times that (the factor covers moving the wall by a texel)."""
    w, g, rec, pts = DC.leak()
    maps = hip.probe_depth_bake_host(w, hip.DEPTH_PARAMS(2, float(F(1.5 * np.sqrt(3.0)))), hip.volume_probes(g))["depth"]
    plain = DC.leak_share(hip.volume_sample_host(g, rec, pts)["out"])
    assert np.abs(plain - 0.3).max() < 1e-6
    shares = []
    D.sample_visible(g, rec, maps, 0.0, 0.0, pts[:, :3], pts[:, 3:], shares=shares)
    W = shares[0].astype(np.float64)
    restated = float((W[1] / (W[0] + W[1])).max())
    got = float(DC.leak_share(_visible(g, rec, maps, 0.0, 0.0, pts)).max())
    print(f"leak: plain share {plain.max():.4f}, restated share {restated:.3e}, library share {got:.3e}")
    assert 0 < restated < 0.03, "a tenth of the plain share at the most, and not exactly 0 (then the factor would mean nothing)"
    assert got < 10 * restated


# -------------------------------------------------------------------------------------------------------- the command line

def _run(args, **kw):
    return subprocess.run([MORT, "6", "--mode", "host", "--width", "48"] + args, cwd=ROOT, capture_output=True, text=True, timeout=300, **kw)


def test_visibility_on_the_command_line(tmp_path):
    if not os.path.exists(MORT):
        subprocess.check_call(["make", "-C", ROOT, "host", "hip", "cli"])
    spec, Dn = "100,100,100,455,455,455,3,3,1", 64
    world, cam = host.build_scene(6, width=48, spp=1)
    W, H = cam.image_width, cam.image_height
    sp = F(355) / F(2)
    g = hip.VOLUME_GRID((100, 100, 100), (sp, sp, 1.0), (3, 3, 1), 0.5)
    cap = F(1.5 * np.sqrt(float(sp) ** 2 + float(sp) ** 2 + 1.0))
    sh = hip.probe_bake_host(world, hip.probe_params_from_camera(cam, Dn), hip.volume_probes(g), O.seed_states(S.DEFAULT_SEED, g.probes * Dn, 1))["sh"]
    rec = V.pack(sh)
    rays = K.Q.ray8(K.primary_rays(cam), K.Q.INF)
    hits = hip.query_closest_host(world, rays)["hits"]
    miss = np.flatnonzero((hits["flags"] & hip.HIT_HIT) == 0)
    picks = [(W // 2, H // 2), (3, H - 2), (W - 5, 1)] + ([(int(miss[0]) % W, int(miss[0]) // W)] if miss.size else [])
    assert miss.size, "the Cornell box's open side: some pixels miss"
    base = ["--sh-volume", spec + f",{Dn}"]
    for vis, bias, minv, s in (("5", 5.0, 0.05, 2), ("2.5,0,3", 2.5, 0.0, 3), ("0,0.5", 0.0, 0.5, 2)):
        pr = np.zeros(g.probes, dtype=hip.PROBE_DTYPE)
        pr["position"], pr["time"] = D.positions(g), 0.5
        maps = D.bake(world, pr, s, cap)
        want = D.sample_visible(g, rec, maps, bias, minv, hits["p"], hits["normal"])
        for x, y in picks:
            p = _run(base + ["--visibility", vis, "--pick", f"{x},{y}"])
            assert p.returncode == 0, p.stdout + p.stderr
            lines = p.stdout.strip().splitlines()
            assert len(lines) == 1, "one JSON line"
            j = json.loads(lines[0])
            i = x + y * W
            hit = int(hits["flags"][i] & hip.HIT_HIT)
            assert j["pick"] == [x, y] and j["hit"] == hit and j["mode"] == "host" and j["depth_subsamples"] == s
            assert F(j["normal_bias"]) == F(bias) and F(j["min_visibility"]) == F(minv) and F(j["max_distance"]) == cap
            got = np.array(j["irradiance"] + [j["weight_sum"]], dtype=F)
            assert (K.words(got) == (K.words(want[i]) if hit else 0)).all(), (vis, x, y, j, want[i])
    # --irradiance-out with and without the flag; without it every byte of the output is what it was
    out_v, out_p = tmp_path / "vis.ppm", tmp_path / "plain.ppm"
    p = _run(base + ["--visibility", "5", "--irradiance-out", str(out_v)])
    assert p.returncode == 0, p.stdout + p.stderr
    j = json.loads(p.stdout.strip())
    assert j["depth_subsamples"] == 2 and F(j["max_distance"]) == cap
    q = _run(base + ["--irradiance-out", str(out_p)])
    assert q.returncode == 0
    jq = json.loads(q.stdout.strip())
    assert list(jq) == ["scene", "width", "height", "irradiance_out", "probes", "directions", "samples", "mode", "seconds", "bake_seconds", "sample_seconds"]
    head = f"P6\n{W} {H}\n255\n".encode()
    plain = V.sample(g, rec, hits["p"], hits["normal"])
    pr = np.zeros(g.probes, dtype=hip.PROBE_DTYPE)
    pr["position"], pr["time"] = D.positions(g), 0.5
    vis = D.sample_visible(g, rec, D.bake(world, pr, 2, cap), 5.0, 0.05, hits["p"], hits["normal"])
    for path, want in ((out_p, plain), (out_v, vis)):
        data = path.read_bytes()
        assert data.startswith(head) and len(data) == len(head) + 3 * W * H
        img = np.frombuffer(data[len(head):], dtype=np.uint8).reshape(H, W, 3)[::-1].reshape(-1, 3)
        e = np.where(((hits["flags"] & hip.HIT_HIT) != 0)[:, None], want[:, :3], 0).astype(np.float64)
        ref8 = 255.0 * np.sqrt(np.clip(np.nan_to_num(e / np.pi), 0, 1))
        assert np.abs(img.astype(np.float64) - ref8).max() <= 0.51 and (img[miss] == 0).all() and img.max() > 32
    assert out_v.read_bytes() != out_p.read_bytes(), "the two images differ"
    x, y = picks[0]
    jp = json.loads(_run(base + ["--pick", f"{x},{y}"]).stdout)
    assert not {"normal_bias", "min_visibility", "depth_subsamples", "max_distance"} & set(jp), "without the flag: today's fields"
    for bad in (["--visibility", "5", "--pick", "1,1"], ["--visibility", "5"], base + ["--visibility", "-1", "--pick", "1,1"],
                base + ["--visibility", "5,2", "--pick", "1,1"], base + ["--visibility", "5,0.05,0", "--pick", "1,1"],
                base + ["--visibility", "5,0.05,9", "--pick", "1,1"], base + ["--visibility", "nan", "--pick", "1,1"],
                base + ["--visibility", "x", "--pick", "1,1"], base + ["--visibility", "inf", "--pick", "1,1"]):
        r = _run(bad)
        assert r.returncode != 0, bad
