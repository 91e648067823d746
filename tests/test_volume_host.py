"""Irradiance volumes on the host (mort_hip_volume_*_host, dev_volume.h) against the contract restated in numpy
(tests/volume_ref.py) at tolerance 0 -- outputs as raw 32-bit words, any NaN equal to any NaN -- and against two things that are
not the contract: mort_hip_sh9_irradiance at the probes, and the float64 irradiance of an affine field between them.  The record
layout, the strides, the masks, the chain from a bake on scene 6, and the command line.  No GPU."""
import json
import os
import subprocess

import numpy as np
import pytest

from mort_amd import hip, host, structs as S
from tests import oracle_lib as O
from tests import volume_cases as K
from tests import volume_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORT = os.path.join(ROOT, "mort_amd", "bin", "mort")
F = np.float32


def _same(got, want, what):
    bad = np.flatnonzero((K.words(got) != K.words(want)).reshape(len(want), -1).any(1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} differ, first {bad[0]}: {got[bad[0]]} / {want[bad[0]]}"


@pytest.mark.parametrize("count", K.COUNTS)
def test_host_form_equals_the_restatement(count):
    g = K.grid(count)
    rec = K.records(g)
    pts = K.points(g)
    assert not np.isfinite(pts).all() and len(pts) >= 2000 + g.probes
    want = V.sample(g, rec, pts[:, :3], pts[:, 3:])
    for nthreads in (1, 3):
        got = hip.volume_sample_host(g, rec, pts, nthreads=nthreads)["out"]
        _same(got, want, f"grid {count} threads {nthreads}")
    assert np.isnan(want).any() and (want[:, 3] > 0).all(), "NaN normals give NaN colours; every point is covered"


@pytest.mark.parametrize("count", K.COUNTS + [(4096, 1, 2)])
def test_probe_positions(count):
    g = K.grid(count)
    pr = hip.volume_probes(g)
    assert pr.shape == (g.probes,) and pr.dtype == hip.PROBE_DTYPE
    assert (pr["position"].view(np.uint32) == V.positions(g).view(np.uint32)).all() and (pr["time"] == F(0.5)).all()
    assert (pr["position"][0] == np.array(K.ORIGIN, dtype=F)).all()
    # index order: x fastest
    if count[0] > 1:
        assert pr["position"][1][0] > pr["position"][0][0] and (pr["position"][1][1:] == pr["position"][0][1:]).all()


def test_pack_layout():
    """27 words bit for bit (a NaN with a payload, a signalling one, -0.0), the weight as given, four zeros; NULL weight is 1.0f"""
    n = 5
    sh = np.random.default_rng(4).uniform(-3, 3, size=(n, 27)).astype(F)
    w32 = sh.view(np.uint32)
    w32[1, 4], w32[2, 26], w32[3, 0], w32[4, 13] = 0x7fc12345, 0xffa00001, 0x80000000, 0x7f800000
    weight = np.array([0.0, 0.25, -1.0, np.inf, 3.5], dtype=F)
    weight.view(np.uint32)[2] = 0x7fc00abc
    for wt in (weight, None):
        rec = hip.volume_pack_host(sh, wt, nthreads=2)["records"]
        assert rec.shape == (n, 32) and rec.dtype == F
        r32 = rec.view(np.uint32)
        assert (r32[:, :27] == w32).all(), "coefficients are copied as words"
        assert (r32[:, 27] == (weight.view(np.uint32) if wt is not None else 0x3f800000)).all()
        assert (r32[:, 28:] == 0).all()
        assert (r32 == V.pack(sh, wt).view(np.uint32)).all(), "the restated layout"
    assert hip.volume_pack_host(np.zeros((0, 27), dtype=F))["records"].shape == (0, 32)


def test_strides():
    g = K.grid((4, 3, 2))
    rec = K.records(g, "fractional")
    pts = K.points(g, 300)
    want = V.sample(g, rec, pts[:, :3], pts[:, 3:])
    _same(hip.volume_sample_host(g, rec, pts)["out"], want, "stride 24")
    _same(hip.volume_sample_host(g, rec, pts.view(hip.VOLUME_POINT_DTYPE).reshape(-1))["out"], want, "VOLUME_POINT_DTYPE")
    for fill in (0xa5, 0xff, 0x00):  # 0xff: NaN words between the points
        _same(hip.volume_sample_host(g, rec, K.strided(pts, 40, fill), stride=40)["out"], want, f"stride 40, {fill:#x} between the points")
    _same(hip.volume_sample_host(g, rec, K.strided(pts, 48), stride=48, nthreads=2)["out"], want, "stride 48")


def test_stride_48_is_a_hit_array():
    """the records of query_closest_host go in as they are"""
    world, cam, rays, hits = K.scene6()
    g = K.scene6_grid()
    rec = K.records(g, "ones", seed=9)
    assert hits.dtype == hip.HIT_DTYPE and hits.dtype.itemsize == 48
    got = hip.volume_sample_host(g, rec, hits)["out"]
    want = V.sample(g, rec, hits["p"], hits["normal"])
    _same(got, want, "scene 6 hits")
    hit = (hits["flags"] & hip.HIT_HIT) != 0
    assert np.abs(got[hit, :3]).max() > 0 and (got[:, 3] > 0).all()


def test_census():
    """on the restatement alone: with every weight 1 an interior point's weights sum to 1 within 2^-22, and where every axis has
    more than one probe at least half the points blend eight probes"""
    for count in K.COUNTS:
        g = K.grid(count)
        pts = K.uniform_points(g, 2000)
        used = []
        out = V.sample(g, K.records(g), pts, K.normals(len(pts)), census=used)
        wsum = out[:, 3].astype(np.float64)
        eight = float((used[0] == 8).mean())
        print(f"grid {count}: wsum {wsum.min():.9f} .. {wsum.max():.9f}, eight corners at {eight:.3f} of the points")
        assert np.abs(wsum - 1.0).max() <= 2.0 ** -22, count
        if min(count) > 1:
            assert eight >= 0.5, count
        assert used[0].max() <= 2 ** sum(c > 1 for c in count), "an axis with one probe has f = 0: its upper corners never contribute"


def _basis64(n):
    """A_l(k) Y_k(n) in float64 with the contract's constants: what mort_hip_sh9_irradiance sums"""
    x, y, z = (n[:, i].astype(np.float64) for i in range(3))
    c0, c1, c2, c3, c4 = (float(c) for c in (V.C0, V.C1, V.C2, V.C3, V.C4))
    Y = np.stack([np.full(len(n), c0), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c3 * (3.0 * z * z - 1.0), c2 * x * z, c4 * (x * x - y * y)], axis=1)
    A = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)
    return A[None, :] * Y


def test_at_the_probes_it_is_the_probes_irradiance():
    """origin and spacing are powers of two, so at a probe position f is exactly 0 (or 1 at the upper boundary), one corner has
    T = 1 and the others T = 0: the output is that probe's fp32 e.  Against mort_hip_sh9_irradiance (float64, rounded once) within
    16 * 2^-24 * sum_k |B_k sh_k|: the 9-term fp32 dot product (9 roundings of partial sums bounded by the absolute sum, 9 of the
    products) and the basis roundings (at most 5 per B_k), first order, fall well inside 16 half-ulps of the absolute sum."""
    g = hip.VOLUME_GRID((-2.0, 0.5, 4.0), (0.5, 2.0, 0.25), (4, 3, 2), 0.0)
    sh = K.coefficients(g, 6)
    rec = V.pack(sh)
    pos = V.positions(g)
    rng = np.random.default_rng(8)
    worst = 0.0
    for rep in range(4):
        nrm = K.Q._unit_sphere(rng, g.probes)
        got = hip.volume_sample_host(g, rec, np.concatenate([pos, nrm], axis=1))["out"]
        assert (got[:, 3] == 1).all()
        B = _basis64(nrm)
        for p in range(g.probes):
            want = hip.sh9_irradiance(sh[p], nrm[p]).astype(np.float64)
            bound = 16 * 2.0 ** -24 * (np.abs(B[p])[:, None] * np.abs(sh[p].reshape(9, 3).astype(np.float64))).sum(0)
            err = np.abs(got[p, :3].astype(np.float64) - want)
            worst = max(worst, float((err / (bound / 16)).max()))
            assert (err <= bound).all(), (p, got[p], want, bound)
    print(f"at the probes: worst {worst:.2f} units of 2^-24 sum|B sh| (bound 16)")


def test_affine_fields_are_reproduced():
    """records sh_p = a + b . pos_p: trilinear interpolation reproduces an affine field, so at interior points the output is the
    float64 irradiance of a + b . x within 64 * 2^-24 * M, M = sum_k |B_k| max_p |sh_p[k]| per channel.  In units of 2^-24 M, first
    order: the basis B_k 5 (the constants' products and A_l); the 9-term dot product 9; the three-factor corner weights T_c and
    W_c 5; the sum over eight corners 8; the division (1 / wsum and the product) 2; wsum itself, eight additions and the T_c in
    them, 12; the coordinate: u carries 3 roundings relative to u <= count - 1 <= 3, the fraction f moves by that absolute amount
    and the field across a cell by at most twice M over (count - 1) cells' worth, 3 u (count - 1) 2 = 18: 59, with 5 to spare for
    the float32 rounding of the records and of the probe positions themselves."""
    rng = np.random.default_rng(12)
    worst = 0.0
    for count in ((4, 3, 2), (2, 4, 3), (4, 4, 4)):
        g = hip.VOLUME_GRID((-0.4, 0.3, 0.2), (0.7, 1.3, 0.45), count, 0.0)
        pos = V.positions(g).astype(np.float64)
        a = rng.uniform(-1, 1, size=27)
        b = rng.uniform(-1, 1, size=(27, 3))
        sh64 = a[None, :] + pos @ b.T
        rec = V.pack(sh64.astype(F))
        x = K.uniform_points(g, 2000, seed=int(sum(count)))
        nrm = K.Q._unit_sphere(rng, len(x))
        got = hip.volume_sample_host(g, rec, np.concatenate([x, nrm], axis=1))["out"]
        B = _basis64(nrm)                                            # (n, 9)
        field = (a[None, :] + x.astype(np.float64) @ b.T).reshape(-1, 9, 3)
        want = (B[:, :, None] * field).sum(1)
        M = (np.abs(B)[:, :, None] * np.abs(sh64).max(0).reshape(9, 3)[None]).sum(1)
        err = np.abs(got[:, :3].astype(np.float64) - want)
        units = float((err / (2.0 ** -24 * M)).max())
        worst = max(worst, units)
        print(f"affine field on {count}: worst {units:.2f} units of 2^-24 M (bound 64)")
        assert (err <= 64 * 2.0 ** -24 * M).all(), (count, units)
        assert np.abs(got[:, 3].astype(np.float64) - 1).max() <= 2.0 ** -22


def test_masks():
    g = K.grid((5, 4, 3))
    pts = K.points(g, 500)
    # a zero-weight corner with NaN coefficients changes nothing: the same points over records whose masked probes hold numbers
    holes = K.records(g, "holes")
    off = holes[:, 27] == 0
    assert off.any() and (~off).any() and np.isnan(holes[off, :27]).all()
    filled = holes.copy()
    filled[off, :27] = 7.5
    got = hip.volume_sample_host(g, holes, pts)["out"]
    _same(got, hip.volume_sample_host(g, filled, pts)["out"], "NaN behind a zero weight")
    _same(got, V.sample(g, holes, pts[:, :3], pts[:, 3:]), "holes")
    fin = np.isfinite(pts).all(1)
    assert np.isfinite(got[fin]).all() and (got[fin, 3] < 1 - 1e-3).any(), "some points lose corners"
    # every weight 0: four zeros, as words
    zero = hip.volume_sample_host(g, K.records(g, "zeros"), pts)["out"]
    assert (zero.view(np.uint32) == 0).all()
    # negative and NaN weights mask as well
    neg = K.records(g, "ones")
    neg[::2, 27] = -1.0
    neg[1::4, 27] = np.nan
    _same(hip.volume_sample_host(g, neg, pts)["out"], V.sample(g, neg, pts[:, :3], pts[:, 3:]), "negative and NaN weights")
    # fractional weights
    frac = K.records(g, "fractional")
    _same(hip.volume_sample_host(g, frac, pts, nthreads=3)["out"], V.sample(g, frac, pts[:, :3], pts[:, 3:]), "fractional weights")


def test_bake_pack_sample_on_scene_6():
    """a 3 x 3 x 3 grid in the Cornell box baked by the host form (D = 64, limit 4), packed, sampled at the scene's hits: the
    restatement over the same records"""
    world, cam, rays, hits = K.scene6()
    g = K.scene6_grid()
    params = hip.probe_params_from_camera(cam, 64)
    params.rp.bounce_limit = 4
    probes = hip.volume_probes(g)
    sh = hip.probe_bake_host(world, params, probes, O.seed_states(S.DEFAULT_SEED, g.probes * 64, 1), nthreads=4)["sh"]
    assert sh.shape == (27, 9, 3) and np.abs(sh[:, 0]).min() > 0, "every probe sees light"
    rec = hip.volume_pack_host(sh)["records"]
    assert (rec.view(np.uint32) == V.pack(sh).view(np.uint32)).all()
    got = hip.volume_sample_host(g, rec, hits, nthreads=4)["out"]
    _same(got, V.sample(g, rec, hits["p"], hits["normal"]), "scene 6 chain")
    hit = (hits["flags"] & hip.HIT_HIT) != 0
    assert (got[hit, :3] > 0).mean() > 0.9, "irradiance is positive almost everywhere on the walls"


@pytest.mark.parametrize("tree", [False, True])
def test_sh_volume_on_the_command_line(tree, tmp_path):
    """`mort 6 --mode host --sh-volume ... --pick X,Y`: --pick's fields plus the chain's irradiance, zeros for a miss"""
    if not os.path.exists(MORT):
        subprocess.check_call(["make", "-C", ROOT, "host", "hip", "cli"])
    spec, D = "100,100,100,455,455,455,3,3,1", 64
    world, cam = host.build_scene(6, width=48, spp=1)
    W, H = cam.image_width, cam.image_height
    g = hip.VOLUME_GRID((100, 100, 100), (F(355) / F(2), F(355) / F(2), 1.0), (3, 3, 1), 0.5)
    sh = hip.probe_bake_host(world, hip.probe_params_from_camera(cam, D), hip.volume_probes(g), O.seed_states(S.DEFAULT_SEED, g.probes * D, 1), tree=tree)["sh"]
    rec = V.pack(sh)
    rays = K.Q.ray8(K.primary_rays(cam), K.Q.INF)
    hits = hip.query_closest_host(world, rays, tree=tree)["hits"]
    want = V.sample(g, rec, hits["p"], hits["normal"])
    miss = np.flatnonzero((hits["flags"] & hip.HIT_HIT) == 0)
    picks = [(W // 2, H // 2), (3, H - 2), (W - 5, 1)] + ([(int(miss[0]) % W, int(miss[0]) // W)] if miss.size else [])
    base = [MORT, "6", "--mode", "host", "--width", "48", "--sh-volume", spec + f",{D}"] + (["--tree"] if tree else [])
    for x, y in picks:
        p = subprocess.run(base + ["--pick", f"{x},{y}"], cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        lines = p.stdout.strip().splitlines()
        assert len(lines) == 1, "one JSON line"
        j = json.loads(lines[0])
        i = x + y * W
        hit = int(hits["flags"][i] & hip.HIT_HIT)
        assert j["pick"] == [x, y] and j["hit"] == hit and j["mode"] == "host" and j["directions"] == D and j["probes"] == [3, 3, 1]
        assert (K.words(np.array(j["p"], dtype=F)) == K.words(hits["p"][i])).all()
        got = np.array(j["irradiance"] + [j["weight_sum"]], dtype=F)
        assert (K.words(got) == (K.words(want[i]) if hit else 0)).all(), (x, y, j, want[i])
    if tree:
        return
    out = tmp_path / "irr.ppm"
    p = subprocess.run(base + ["--irradiance-out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    data = out.read_bytes()
    head = f"P6\n{W} {H}\n255\n".encode()
    assert data.startswith(head) and len(data) == len(head) + 3 * W * H
    img = np.frombuffer(data[len(head):], dtype=np.uint8).reshape(H, W, 3)[::-1].reshape(-1, 3)  # the file's first row is the top row
    e = np.where(((hits["flags"] & hip.HIT_HIT) != 0)[:, None], want[:, :3], 0).astype(np.float64)
    ref8 = 255.0 * np.sqrt(np.clip(np.nan_to_num(e / np.pi), 0, 1))
    assert np.abs(img.astype(np.float64) - ref8).max() <= 0.51 and (img[miss] == 0).all() and img.max() > 32
    for bad in (["--sh-volume", "0,0,0,1,1,1,2,2"], ["--sh-volume", "0,0,0,1,1,1,2,2,2,100", "--pick", "1,1"], ["--sh-volume", "0,0,0,0,1,1,2,2,2", "--pick", "1,1"],
                ["--sh-volume", spec], ["--sh-volume", spec, "--pick", "1,1", "--irradiance-out", str(out)], ["--irradiance-out", str(out)],
                ["--sh-volume", spec, "--pick", "1,1", "--probe", "1,1"], ["--sh-volume", "0,0,0,1,1,1,0,2,2", "--pick", "1,1"]):
        q = subprocess.run([MORT, "6", "--mode", "host", "--width", "48"] + bad, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert q.returncode != 0, bad
