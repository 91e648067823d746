"""First-hit feature buffers and the a-trous denoiser through their host forms -- the same per-pixel bodies
the gfx950 kernels run (dev_features.h) -- on the CPU: closed-form features on hand-built worlds, invariants on the ten
built-in scenes, the denoiser against an independent float64 numpy restatement of its contract, the pass-through case,
the quality it reaches at 4 spp, the CLI flags and the new kernels' resources."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mort_amd import hip, host
from tests.worlds import flat_camera, flat_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORT = os.path.join(ROOT, "mort_amd", "bin", "mort")
NT = min(16, os.cpu_count() or 1)


def _v(v):
    return np.array([v.e[0], v.e[1], v.e[2]], dtype=np.float64)


def _primary_ray(cam, x, y):
    o = _v(cam.center)
    return o, _v(cam.pixel00_loc) + x * _v(cam.pixel_delta_u) + y * _v(cam.pixel_delta_v) - o


def _sphere_t(o, d, c, r):
    oc = o - c
    a, hb, cc = d @ d, oc @ d, oc @ oc - r * r
    disc = hb * hb - a * cc
    if disc < 0:
        return None
    for t in ((-hb - np.sqrt(disc)) / a, (-hb + np.sqrt(disc)) / a):
        if t >= 0.001:
            return t
    return None


def _pixels(cam):
    W, H = cam.image_width, cam.image_height
    return [(x, y) for y in range(0, H, 2) for x in range(0, W, 2)]


def _check_pixel(f, x, y, alb, nrm, dep):
    np.testing.assert_allclose(f["depth"][y, x], dep, rtol=1e-5)
    np.testing.assert_allclose(f["albedo"][y, x], alb, rtol=1e-5)
    # a normal component is a difference of nearly equal fp32 values near the silhouette: absolute tolerance
    np.testing.assert_allclose(f["normal"][y, x], nrm, rtol=1e-5, atol=1e-4)


def _check_miss(f, cam, x, y):
    assert f["depth"][y, x] == 0.0
    assert (f["normal"][y, x] == 0.0).all()
    assert (f["albedo"][y, x] == np.array([cam.background.e[k] for k in range(3)], dtype=np.float32)).all()


@pytest.mark.parametrize("kind", ["lamb", "metal"])
@pytest.mark.parametrize("tree", [False, True])
def test_sphere_features_closed_form(kind, tree):
    c, r = np.array([0.0, 0.0, -1.0]), 0.5
    mat = ("lamb", (.7, .3, .3)) if kind == "lamb" else ("metal", (.8, .6, .2), 0.3)
    world, _ = flat_world([("sphere", tuple(c), r, mat)])
    cam = flat_camera(width=64)
    f = hip.render_features_host(world, cam, nthreads=NT, tree=tree)
    hits = 0
    for x, y in _pixels(cam):
        o, d = _primary_ray(cam, x, y)
        t = _sphere_t(o, d, c, r)
        if t is None:
            _check_miss(f, cam, x, y)
            continue
        hits += 1
        n = (o + t * d - c) / r
        n = n if n @ d < 0 else -n
        _check_pixel(f, x, y, mat[1], n, t * np.linalg.norm(d))
    assert hits > 10


def test_quad_features_closed_form():
    Q, u, v = np.array([-1.0, -0.5, -1.5]), np.array([2.0, 0, 0]), np.array([0, 1.5, 0.3])
    world, _ = flat_world([("quad", tuple(Q), tuple(u), tuple(v), ("lamb", (.2, .5, .8)))])
    cam = flat_camera(width=64)
    f = hip.render_features_host(world, cam, nthreads=NT)
    nvec = np.cross(u, v)
    nunit = nvec / np.linalg.norm(nvec)
    w = nvec / (nvec @ nvec)
    hits = 0
    for x, y in _pixels(cam):
        o, d = _primary_ray(cam, x, y)
        t = (nunit @ Q - nunit @ o) / (nunit @ d)
        p = o + t * d - Q
        al, be = w @ np.cross(p, v), w @ np.cross(u, p)
        if not (t >= 0.001 and 0 <= al <= 1 and 0 <= be <= 1):
            _check_miss(f, cam, x, y)
            continue
        hits += 1
        _check_pixel(f, x, y, (.2, .5, .8), nunit if nunit @ d < 0 else -nunit, t * np.linalg.norm(d))
    assert hits > 10


def test_constant_medium_features_closed_form():
    c, r = np.array([0.0, 0.0, -1.0]), 0.5
    world, _ = flat_world([], media=[(tuple(c), r, 1.0, (.9, .4, .2))])
    cam = flat_camera(width=64)
    f = hip.render_features_host(world, cam, nthreads=NT)
    hits = 0
    for x, y in _pixels(cam):
        o, d = _primary_ray(cam, x, y)
        oc = o - c
        a, hb, cc = d @ d, oc @ d, oc @ oc - r * r
        disc = hb * hb - a * cc
        if disc <= 1e-9:
            if disc < -1e-6:
                _check_miss(f, cam, x, y)
            continue
        hits += 1
        t1 = (-hb - np.sqrt(disc)) / a  # the camera is outside: the entry point, no random distance
        _check_pixel(f, x, y, (.9, .4, .2), -d / np.linalg.norm(d), t1 * np.linalg.norm(d))
    assert hits > 10


def test_features_before_a_solid_medium_and_behind_it():
    """A medium in front of a solid is hit at its entry; a solid in front of the medium hides it."""
    world, _ = flat_world([("sphere", (0, 0, -3), 0.5, ("lamb", (.1, .2, .3)))], media=[((0, 0, -1), 0.3, 1.0, (.5, .5, .5))])
    cam = flat_camera(width=48)
    f = hip.render_features_host(world, cam, nthreads=NT)
    x, y = cam.image_width // 2, cam.image_height // 2
    o, d = _primary_ray(cam, x, y)
    assert np.allclose(f["albedo"][y, x], .5) or np.allclose(f["albedo"][y, x], (.1, .2, .3))
    tm = _sphere_t(o, d, np.array([0, 0, -1.0]), 0.3)
    ts = _sphere_t(o, d, np.array([0, 0, -3.0]), 0.5)
    if tm is not None:
        assert ts is None or tm < ts
        np.testing.assert_allclose(f["depth"][y, x], tm * np.linalg.norm(d), rtol=1e-5)


@pytest.mark.parametrize("sid", range(1, 11))
def test_scene_features_invariants(sid):
    world, cam = host.build_scene(sid, width=48, spp=4)
    a = hip.render_features_host(world, cam, nthreads=NT)
    b = hip.render_features_host(world, cam, nthreads=3)
    t = hip.render_features_host(world, cam, nthreads=NT, tree=True)
    for k in ("albedo", "normal", "depth"):
        assert (a[k].view(np.uint32) == b[k].view(np.uint32)).all(), f"{k}: two calls differ"
        assert (a[k].view(np.uint32) == t[k].view(np.uint32)).all(), f"{k}: tree walk and item scan differ"
    hit = a["depth"] > 0
    assert (a["depth"] >= 0).all()
    H, W = a["depth"].shape
    ys, xs = np.mgrid[0:H, 0:W]
    o = _v(cam.center)
    d = _v(cam.pixel00_loc)[None, None] + xs[..., None] * _v(cam.pixel_delta_u) + ys[..., None] * _v(cam.pixel_delta_v) - o
    n = a["normal"].astype(np.float64)
    assert np.abs(np.linalg.norm(n[hit], axis=-1) - 1).max(initial=0) < 5e-3
    du = d / np.linalg.norm(d, axis=-1, keepdims=True)
    assert ((n * du).sum(-1)[hit] <= 1e-6).all(), "normals face the camera"
    bg = np.array([cam.background.e[k] for k in range(3)], dtype=np.float32)
    assert (a["albedo"][~hit] == bg).all() and (a["normal"][~hit] == 0).all()


# ---- the denoiser against an independent float64 restatement of its contract (include/mort_hip.h) ----
K5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])


def ref_denoise(C, A, N, D, p):
    C, A, N, D = (np.asarray(a, dtype=np.float64) for a in (C, A, N, D))
    if p.iterations == 0:
        return C
    H, W = D.shape
    m = np.maximum(A, 1e-3)
    E = C / m
    miss = D == 0
    ys, xs = np.mgrid[0:H, 0:W]
    for i in range(p.iterations):
        s = 2 ** i
        num = np.zeros_like(E)
        den = np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + dy * s, xs + dx * s
                ok = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                Eq, Nq, Dq, Aq, mq = E[qy, qx], N[qy, qx], D[qy, qx], A[qy, qx], miss[qy, qx]
                both = miss & mq
                wn = np.where(both, 1.0, np.maximum(0.0, (N * Nq).sum(-1)) ** (2 ** p.normal_log2_power))
                xc = ((E - Eq) ** 2).sum(-1) * 4 ** i / p.sigma_color ** 2
                with np.errstate(divide="ignore", invalid="ignore"):
                    xd = np.where(both, 0.0, np.abs(D - Dq) / (p.sigma_depth * s * D))
                xa = ((A - Aq) ** 2).sum(-1) / p.sigma_albedo ** 2
                with np.errstate(invalid="ignore"):
                    w = K5[dx + 2] * K5[dy + 2] * wn * np.exp(-(xc + xd + xa))
                w = np.where(ok & (miss == mq), w, 0.0)
                num += w[..., None] * Eq
                den += w
        E = np.where(den[..., None] > 0, num / np.where(den > 0, den, 1)[..., None], E)
    out = E * m
    return np.where(np.isnan(out), 0.0, out)


def gamma_tail(acc):
    v = np.clip(np.sqrt(acc.astype(np.float32)), np.float32(0), np.float32(0.999))
    return (np.float32(256) * v).astype(np.int32).astype(np.uint8)


def random_inputs(W, H, seed):
    g = np.random.default_rng(seed)
    C = g.uniform(0, 2, (H, W, 3)).astype(np.float32)
    A = g.uniform(0, 1, (H, W, 3)).astype(np.float32)
    A[g.random((H, W)) < 0.05] = 0.0  # clamped to 1e-3 by the demodulation
    N = g.normal(size=(H, W, 3))
    N /= np.linalg.norm(N, axis=-1, keepdims=True)
    N = (0.3 * N + np.array([0, 0, 1.0])) / np.linalg.norm(0.3 * N + np.array([0, 0, 1.0]), axis=-1, keepdims=True)
    D = g.uniform(1, 10, (H, W)).astype(np.float32)
    miss = g.random((H, W)) < 0.2
    D[miss] = 0
    N[miss] = 0
    return C, A, N.astype(np.float32), D


def _compare(C, A, N, D, p):
    out = hip.denoise_host(C, A, N, D, params=p, nthreads=NT)
    ref = ref_denoise(C, A, N, D, p)
    np.testing.assert_allclose(out["accum"], ref, rtol=1e-4, atol=1e-6 * max(1.0, float(np.abs(ref).max())))
    assert (out["rgba"][..., :3] == gamma_tail(out["accum"])).all()
    assert (out["rgba"][..., 3] == 255).all()
    return out


@pytest.mark.parametrize("W,H", [(97, 55), (5, 3), (1, 1), (40, 7)])
@pytest.mark.parametrize("pset", [dict(), dict(iterations=1), dict(iterations=3, sigma_color=0.7, sigma_depth=0.5, sigma_albedo=0.3, normal_log2_power=1),
                                  dict(iterations=8, normal_log2_power=6)])
def test_denoise_matches_numpy_on_random_images(W, H, pset):
    _compare(*random_inputs(W, H, W * 1000 + H), hip.DenoiseParams(**pset))


@pytest.mark.parametrize("sid", [1, 6, 8])
def test_denoise_matches_numpy_on_real_features(sid):
    world, cam = host.build_scene(sid, width=64, spp=4)
    r = hip.render_host(world, cam, nthreads=NT)
    f = hip.render_features_host(world, cam, nthreads=NT)
    for p in (hip.DenoiseParams(), hip.DenoiseParams(iterations=2, sigma_color=8.0)):
        _compare(r["accum"], f["albedo"], f["normal"], f["depth"], p)


def test_denoise_is_deterministic_across_thread_counts():
    C, A, N, D = random_inputs(61, 33, 7)
    a = hip.denoise_host(C, A, N, D, nthreads=1)
    b = hip.denoise_host(C, A, N, D, nthreads=NT)
    assert (a["accum"].view(np.uint32) == b["accum"].view(np.uint32)).all() and (a["rgba"] == b["rgba"]).all()


def test_zero_iterations_pass_the_render_through():
    world, cam = host.build_scene(2, width=64, spp=4)
    r = hip.render_host(world, cam, nthreads=NT)
    f = hip.render_features_host(world, cam, nthreads=NT)
    out = hip.denoise_host(r["accum"], f["albedo"], f["normal"], f["depth"], params=hip.DenoiseParams(iterations=0), nthreads=NT)
    assert (out["accum"].view(np.uint32) == r["accum"].view(np.uint32)).all()
    assert (out["rgba"] == r["rgba"]).all()


def test_defaults_and_parameter_checks():
    p = hip.DenoiseParams()
    assert p.iterations == 5 and p.sigma_color > 0 and p.sigma_depth > 0 and p.sigma_albedo > 0 and 0 <= p.normal_log2_power <= 16
    C, A, N, D = random_inputs(8, 8, 1)
    for bad in (dict(iterations=9), dict(iterations=-1), dict(sigma_color=0.0), dict(sigma_depth=float("nan")), dict(normal_log2_power=17)):
        with pytest.raises(hip.MortHipError):
            hip.denoise_host(C, A, N, D, params=hip.DenoiseParams(**bad))


# ---- quality at 4 spp (DESIGN.md 4.9 records the measured ratios; the thresholds sit just above them) ----
def _g(a):
    return np.sqrt(np.clip(a, 0, 0.999 ** 2))


# scene 8: the camera sits inside the final scene's fog shell.  Its limit is the ratio measured with the medium entry clamped to
# t_min, when every pixel of the feature buffers was the fog 1 cm before the lens (0.6521); passing the fog over gives 0.535.
@pytest.mark.parametrize("sid,limit", [(1, 0.85), (3, 1.15), (6, 0.6), (8, 0.6522)])
def test_denoise_quality_at_4spp(sid, limit):
    world, cam = host.build_scene(sid, width=96, spp=4)
    noisy = hip.render_host(world, cam, nthreads=NT)["accum"]
    w2, cam2 = host.build_scene(sid, width=96, spp=400)
    ref = hip.render_host(w2, cam2, nthreads=NT)["accum"]
    f = hip.render_features_host(world, cam, nthreads=NT)
    den = hip.denoise_host(noisy, f["albedo"], f["normal"], f["depth"], nthreads=NT)["accum"]
    e0 = np.sqrt(np.mean((_g(noisy) - _g(ref)) ** 2))
    e1 = np.sqrt(np.mean((_g(den) - _g(ref)) ** 2))
    assert e1 <= limit * e0, f"scene {sid}: denoised RMSE {e1:.4f} vs noisy {e0:.4f} (ratio {e1 / e0:.3f})"


# ---- CLI ----
def _run(*args, cwd):
    return subprocess.run([MORT, *map(str, args)], cwd=cwd, capture_output=True, text=True, timeout=600)


def test_cli_denoise_and_features_out(tmp_path):
    p = _run(1, "--mode", "host", "--width", 64, "--spp", 4, "--denoise", "--features-out", "P", "--out", "x.ppm", "--dump-f32", "raw.f32",
             "--threads", NT, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["denoise_seconds"] > 0
    W, H = line["width"], line["height"]
    world, cam = host.build_scene(1, width=64, spp=4)
    f = hip.render_features_host(world, cam, nthreads=NT)
    for k, ch in (("albedo", 3), ("normal", 3), ("depth", 1)):
        got = np.fromfile(tmp_path / f"P.{k}.f32", dtype=np.float32)
        assert got.size == W * H * ch and (got.view(np.uint32) == f[k].reshape(-1).view(np.uint32)).all()
    r = hip.render_host(world, cam, nthreads=NT)
    assert (np.fromfile(tmp_path / "raw.f32", dtype=np.float32).view(np.uint32) == r["accum"].reshape(-1).view(np.uint32)).all(), "--dump-f32 is the raw render"
    den = hip.denoise_host(r["accum"], f["albedo"], f["normal"], f["depth"], nthreads=NT)
    data = open(tmp_path / "x.ppm", "rb").read()
    img = np.frombuffer(data[len(data) - W * H * 3:], dtype=np.uint8).reshape(H, W, 3)
    assert (img[::-1] == den["rgba"][..., :3]).all() or (img == den["rgba"][..., :3]).all()


def test_cli_without_new_flags_keeps_its_json_keys(tmp_path):
    p = _run(2, "--mode", "host", "--width", 32, "--spp", 1, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    keys = set(json.loads(p.stdout.strip().splitlines()[-1]))
    assert "denoise_seconds" not in keys
    assert keys == {"scene", "width", "height", "spp_nominal", "spp_effective", "depth", "mode", "gpus", "seconds", "msamples_per_s",
                    "kernel_seconds", "gather_seconds", "segments", "algorithmic_hbm_bytes", "hbm_GBps", "hbm_frac_of_8TBps",
                    "reference_walks", "kernel"}


@pytest.mark.parametrize("flag", [["--denoise"], ["--features-out", "P"]])
def test_cli_rejects_denoise_with_several_gpus(tmp_path, flag):
    p = _run(1, "--gpus", 2, "--gather", "shm", *flag, cwd=tmp_path)
    assert p.returncode != 0 and "single-GPU" in p.stderr
    assert not list(tmp_path.iterdir())


def test_new_kernels_use_no_private_memory():
    lib = os.path.join(ROOT, "mort_amd", "lib", "libmort_hip.so")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"), lib], capture_output=True, text=True, check=True).stdout
    rows = [l.split() for l in out.splitlines() if l.startswith(("feat_kernel", "atrous_"))]
    names = {" ".join(r[:-7]) for r in rows}
    assert names == {"feat_kernel<false>", "feat_kernel<true>", "atrous_kernel<false, false>", "atrous_kernel<false, true>",
                     "atrous_kernel<true, false>", "atrous_kernel<true, true>", "atrous_passthrough_kernel"}, names
    for r in rows:
        vspill, sspill, private = int(r[-4]), int(r[-3]), int(r[-2])
        assert vspill == 0 and sspill == 0 and private == 0, r
