"""The SVGF filter stage through its host form -- the same per-pixel bodies the gfx950 kernels run (dev_svgf.h) --
on the CPU: an independent numpy restatement of the contract (float64, and float32 to measure the contract's own sensitivity),
closed forms, determinism and parameter checks, the quality it reaches against the a-trous denoiser on the accumulated colour,
the CLI flag and the new kernels' resources."""
import ctypes as C_
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mort_amd import hip, host
from tests.test_denoise_host import _g, gamma_tail, random_inputs
from tests.test_temporal_host import _frames, _moved, _sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORT = os.path.join(ROOT, "mort_amd", "bin", "mort")
NT = min(16, os.cpu_count() or 1)

K5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
K3 = (1 / 4, 1 / 2, 1 / 4)
LW = (0.2126, 0.7152, 0.0722)


# ---- the contract, restated (include/mort_hip.h); f = the dtype every operation runs in ----
def _shift(a, dy, dx):
    """(a[y + dy, x + dx] with clamped indices, in-image mask)"""
    H, W = a.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    qy, qx = ys + dy, xs + dx
    ok = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
    return a[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)], ok


def _lum(X, f):
    return f(LW[0]) * X[..., 0] + f(LW[1]) * X[..., 1] + f(LW[2]) * X[..., 2]


def ref_svgf(C, A, N, D, V, p, f=np.float64):
    """(accum (H, W, 3), variance (H, W)) in dtype f"""
    C, A, N, D = (np.asarray(a).astype(f) for a in (C, A, N, D))
    H, W = D.shape
    m = np.maximum(A, f(1e-3))
    E = C / m
    k = _lum(m, f)
    miss = D == 0
    sl, sd, sa = f(p.sigma_luminance), f(p.sigma_depth), f(p.sigma_albedo)
    npow = 2 ** p.normal_log2_power

    def geometry(dy, dx, depth_scale):
        """(w_n, x_d, tap counts) between p and q = p + (dy, dx)"""
        Nq, ok = _shift(N, dy, dx)
        Dq, _ = _shift(D, dy, dx)
        mq, _ = _shift(miss, dy, dx)
        both = miss & mq
        wn = np.where(both, f(1), np.maximum(f(0), (N * Nq).sum(-1)) ** npow).astype(f)
        with np.errstate(divide="ignore", invalid="ignore"):
            xd = np.where(both | (depth_scale == 0), f(0), np.abs(D - Dq) / (sd * f(depth_scale) * D)).astype(f)
        return wn, xd, ok & (miss == mq)

    # prepare: the variance of l(E)
    l = _lum(E, f)
    s0, s1, s2 = (np.zeros((H, W), dtype=f) for _ in range(3))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            wn, xd, ok = geometry(dy, dx, max(abs(dx), abs(dy)))
            lq, _ = _shift(l, dy, dx)
            with np.errstate(invalid="ignore", over="ignore"):
                w = np.where(ok, wn * np.exp(-xd), f(0)).astype(f)
                s0 += w
                s1 += w * lq
                s2 += w * (lq * lq)
    with np.errstate(divide="ignore", invalid="ignore"):
        m1, m2 = s1 / s0, s2 / s0
        var = np.where(s0 > 0, np.maximum(f(0), m2 - m1 * m1), f(0)).astype(f)
        if V is not None:
            V = np.asarray(V).astype(f)
            var = np.where(V >= 0, V / (k * k), var).astype(f)
    if p.iterations == 0:
        return C, var * (k * k)

    for i in range(p.iterations):
        s = 2 ** i
        gs, gw = np.zeros((H, W), dtype=f), np.zeros((H, W), dtype=f)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                vq, ok = _shift(var, dy, dx)
                wt = f(K3[dx + 1] * K3[dy + 1])
                gs += np.where(ok, wt * vq, f(0))
                gw += np.where(ok, wt, f(0))
        with np.errstate(invalid="ignore"):
            lden = sl * np.sqrt(gs / gw) + f(1e-6)
        l = _lum(E, f)
        num, nv, den = np.zeros_like(E), np.zeros((H, W), dtype=f), np.zeros((H, W), dtype=f)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                wn, xd, ok = geometry(dy * s, dx * s, s)
                Eq, _ = _shift(E, dy * s, dx * s)
                Aq, _ = _shift(A, dy * s, dx * s)
                vq, _ = _shift(var, dy * s, dx * s)
                lq, _ = _shift(l, dy * s, dx * s)
                with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                    xl = np.abs(l - lq) / lden
                    xa = ((A - Aq) ** 2).sum(-1) / (sa * sa)
                    w = f(K5[dx + 2] * K5[dy + 2]) * wn * np.exp(-(xl + xd + xa))
                w = np.where(ok & ~np.isnan(w), w, f(0)).astype(f)
                num += w[..., None] * Eq
                nv += (w * w) * vq
                den += w
        good = den > 0
        sden = np.where(good, den, f(1))
        E = np.where(good[..., None], num / sden[..., None], E).astype(f)
        var = np.where(good, nv / (sden * sden), var).astype(f)
    out = E * m
    return np.where(np.isnan(out), f(0), out), var * (k * k)


def svgf_inputs(W, H, seed):
    """test_denoise_host's random images (20 % misses) plus V in [0.01, 1] with 10 % of the pixels unknown (-1)"""
    C, A, N, D = random_inputs(W, H, seed)
    g = np.random.default_rng(seed + 77)
    V = g.uniform(0.01, 1, (H, W)).astype(np.float32)
    V[g.random((H, W)) < 0.1] = -1.0
    return C, A, N, D, V


def _second_moment(C, A):
    """max over the image of l(E)^2 k^2: the magnitude of the two moments whose difference the spatial variance estimate is"""
    m = np.maximum(np.asarray(A, dtype=np.float64), 1e-3)
    return float((_lum(np.asarray(C, dtype=np.float64) / m, np.float64) ** 2).max() * (_lum(m, np.float64) ** 2).max())


def _compare(C, A, N, D, V, p):
    out = hip.svgf_host(C, A, N, D, V, params=p, nthreads=NT)
    ref, rvar = ref_svgf(C, A, N, D, V, p)
    np.testing.assert_allclose(out["accum"], ref, rtol=1e-4, atol=1e-6 * max(1.0, float(np.abs(ref).max())))
    # the variance: the same tolerance, its "max" being the largest magnitude that enters it -- where it comes from the spatial
    # estimate that is the second moment (Var = m2 - m1^2 cancels: both moments carry 6e-8 relative rounding)
    np.testing.assert_allclose(out["variance"], rvar, rtol=1e-4, atol=1e-6 * max(1.0, float(np.abs(rvar).max()), _second_moment(C, A)))
    assert (out["rgba"][..., :3] == gamma_tail(out["accum"])).all()
    assert (out["rgba"][..., 3] == 255).all()
    assert not np.isnan(out["accum"]).any() and not np.isnan(out["variance"]).any() and (out["variance"] >= 0).all()
    return out


PSETS = [dict(), dict(iterations=0), dict(iterations=1), dict(iterations=3, sigma_luminance=0.7, sigma_depth=0.5, sigma_albedo=0.3, normal_log2_power=1),
         dict(iterations=8, normal_log2_power=6), dict(iterations=5, sigma_luminance=10.0)]


@pytest.mark.parametrize("W,H", [(97, 55), (5, 3), (1, 1), (40, 7)])
@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("have_var", [True, False])
def test_svgf_matches_numpy_on_random_images(W, H, pset, have_var):
    C, A, N, D, V = svgf_inputs(W, H, W * 1000 + H)
    _compare(C, A, N, D, V if have_var else None, hip.SvgfParams(**pset))


def _accumulated(sid, width=64, frames=4):
    """scene sid accumulated over `frames` still frames at 4 spp: (accum, features, variance)"""
    _, cam = host.build_scene(sid, width=width, spp=4)
    _, fr = _frames(sid, [cam] * frames, width=width)
    th = hip.TemporalHistory(cam.image_width, cam.image_height, nthreads=NT)
    for acc, f in fr:
        out = th.step(acc, f["normal"], f["depth"], cam)
    return out["accum"], fr[-1][1], out["variance"]


@pytest.mark.parametrize("sid", [1, 6, 8])
def test_svgf_matches_numpy_on_real_inputs(sid):
    """Real variances can be tiny and x_l = |dl| / (sigma sqrt(g) + 1e-6) ill-conditioned, so the yardstick is the contract's own
    fp32 sensitivity: the restatement run in float32 against the same in float64, largest deviation over the image, relative to
    the largest value.  The implementation may deviate from the float64 restatement by 4x that (summation order).
    Measured, default parameters (float32 restatement vs float64 / host form vs float64), accum; variance:
    scene 1, known variance: 3.2e-7 / 3.0e-7; 5.9e-7 / 5.9e-7    spatial estimate: 4.4e-7 / 5.6e-7; 2.3e-7 / 5.2e-7
    scene 6, known variance: 1.9e-7 / 1.3e-7; 5.6e-7 / 6.8e-7    spatial estimate: 1.5e-7 / 2.0e-7; 3.9e-7 / 3.1e-7
    scene 8, known variance: 3.6e-7 / 3.9e-7; 1.6e-7 / 1.5e-7    spatial estimate: 6.4e-7 / 4.4e-7; 3.5e-7 / 2.6e-7
    -- a few float32 roundings: on these inputs the contract is well conditioned; the largest host / sensitivity ratio seen is
    2.6 (scene 1, spatial estimate, 5 iterations at sigma_luminance 1, variance: 1.8e-7 / 4.7e-7)."""
    acc, f, var = _accumulated(sid)
    for V in (var, None):
        for p in (hip.SvgfParams(), hip.SvgfParams(iterations=5, sigma_luminance=1.0)):
            out = hip.svgf_host(acc, f["albedo"], f["normal"], f["depth"], V, params=p, nthreads=NT)
            r64 = ref_svgf(acc, f["albedo"], f["normal"], f["depth"], V, p)
            r32 = ref_svgf(acc, f["albedo"], f["normal"], f["depth"], V, p, f=np.float32)
            for name, got, a64, a32 in (("accum", out["accum"], r64[0], r32[0]), ("variance", out["variance"], r64[1], r32[1])):
                scale = float(np.abs(a64).max())
                sens = float(np.abs(a32.astype(np.float64) - a64).max()) / scale
                dev = float(np.abs(got.astype(np.float64) - a64).max()) / scale
                print(f"scene {sid} V={'known' if V is not None else 'none'} it={p.iterations} {name}: sensitivity {sens:.3e}, host form {dev:.3e}")
                assert dev <= 4 * sens, (sid, name, dev, sens)
            assert not np.isnan(out["accum"]).any() and not np.isnan(out["variance"]).any()


# ---- closed forms ----
def _flat(W, H, colour=1.0, albedo=0.5, depth=3.0):
    C = np.full((H, W, 3), colour, dtype=np.float32)
    A = np.full((H, W, 3), albedo, dtype=np.float32)
    N = np.zeros((H, W, 3), dtype=np.float32)
    N[..., 2] = 1.0
    D = np.full((H, W), depth, dtype=np.float32)
    return C, A, N, D


def _kernel_sums(W, H, s):
    """per pixel, over the in-image 5x5 taps at step s of the B3 kernel: (sum of weights, sum of squared weights)"""
    one = np.ones((H, W))
    sw, sw2 = np.zeros((H, W)), np.zeros((H, W))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            _, ok = _shift(one, dy * s, dx * s)
            w = K5[dx + 2] * K5[dy + 2]
            sw += ok * w
            sw2 += ok * w * w
    return sw, sw2


def test_constant_image_returns_itself_and_scales_the_variance():
    W, H = 64, 48
    C, A, N, D = _flat(W, H, colour=0.7)
    V = np.full((H, W), 0.04, dtype=np.float32)
    out = hip.svgf_host(C, A, N, D, V, params=hip.SvgfParams(iterations=1), nthreads=NT)
    np.testing.assert_allclose(out["accum"], C, rtol=1e-6)
    sw, sw2 = _kernel_sums(W, H, 1)
    np.testing.assert_allclose(out["variance"], 0.04 * sw2 / sw ** 2, rtol=1e-5)
    # away from the border: the 5x5 kernel's factor, sum over the taps of (h_i h_j)^2 = (sum h_i^2)^2 = (70 / 256)^2
    np.testing.assert_allclose(out["variance"][2:-2, 2:-2], 0.04 * (70 / 256) ** 2, rtol=1e-5)
    # every iteration multiplies by its own step's sums
    out = hip.svgf_host(C, A, N, D, V, params=hip.SvgfParams(iterations=3), nthreads=NT)
    # uniform only where no tap of this or an earlier step left the image (2 * (1 + 2 + 4) = 14 pixels from the border)
    np.testing.assert_allclose(out["variance"][14:-14, 14:-14], 0.04 * (70 / 256) ** 6, rtol=1e-5)
    np.testing.assert_allclose(out["accum"], C, rtol=1e-6)


def test_zero_variance_returns_the_input():
    C, A, N, D, _ = svgf_inputs(53, 31, 3)
    V = np.zeros((31, 53), dtype=np.float32)
    out = hip.svgf_host(C, A, N, D, V, nthreads=NT)
    # a zero-variance pixel filters with equal-luminance neighbours only: on a random image, itself.  What is left is the rounding
    # of the demodulation, the weighted mean of one tap and the remodulation
    np.testing.assert_allclose(out["accum"], C, rtol=4e-7, atol=1e-30)
    assert not np.isnan(out["accum"]).any() and (out["variance"] == 0).all()


def test_step_edge_stays_with_small_variance_and_blurs_with_large():
    W, H = 40, 16
    C, A, N, D = _flat(W, H, colour=0.5, albedo=1.0)
    C[:, W // 2:] = 1.0
    p = hip.SvgfParams()
    sharp = hip.svgf_host(C, A, N, D, np.full((H, W), 1e-8, dtype=np.float32), params=p, nthreads=NT)["accum"]
    np.testing.assert_allclose(sharp, C, rtol=1e-6)
    blurred = hip.svgf_host(C, A, N, D, np.full((H, W), 4.0, dtype=np.float32), params=p, nthreads=NT)["accum"]
    assert blurred[H // 2, W // 2 - 1, 0] > 0.6 and blurred[H // 2, W // 2, 0] < 0.9
    assert abs(float(blurred.astype(np.float64).mean()) - float(C.astype(np.float64).mean())) < 0.02


def test_hits_and_misses_never_mix():
    W, H = 36, 20
    C, A, N, D = _flat(W, H, colour=1.0, albedo=1.0)
    miss = np.zeros((H, W), dtype=bool)
    miss[:, :11] = True
    miss[5:9, 20:27] = True
    C[miss] = 5.0
    D[miss] = 0.0
    N[miss] = 0.0
    for V in (np.full((H, W), 100.0, dtype=np.float32), None):
        out = hip.svgf_host(C, A, N, D, V, params=hip.SvgfParams(iterations=5, sigma_luminance=1e6), nthreads=NT)["accum"]
        np.testing.assert_allclose(out[miss], 5.0, rtol=1e-6)
        np.testing.assert_allclose(out[~miss], 1.0, rtol=1e-6)


# ---- determinism and checks ----
def test_svgf_is_deterministic_across_thread_counts():
    C, A, N, D, V = svgf_inputs(61, 33, 7)
    a = hip.svgf_host(C, A, N, D, V, nthreads=1)
    b = hip.svgf_host(C, A, N, D, V, nthreads=NT)
    for k in ("accum", "variance", "rgba"):
        assert (np.ascontiguousarray(a[k]).view(np.uint8) == np.ascontiguousarray(b[k]).view(np.uint8)).all(), k


def test_zero_iterations_pass_the_render_through():
    world, cam = host.build_scene(2, width=64, spp=4)
    r = hip.render_host(world, cam, nthreads=NT)
    f = hip.render_features_host(world, cam, nthreads=NT)
    V = np.full(f["depth"].shape, 0.01, dtype=np.float32)
    out = hip.svgf_host(r["accum"], f["albedo"], f["normal"], f["depth"], V, params=hip.SvgfParams(iterations=0), nthreads=NT)
    assert (out["accum"].view(np.uint32) == r["accum"].view(np.uint32)).all()
    assert (out["rgba"] == r["rgba"]).all()
    np.testing.assert_allclose(out["variance"], V, rtol=4e-7)  # V / k^2 * k^2


def test_defaults_and_parameter_checks():
    p = hip.SvgfParams()
    d = hip.DenoiseParams()
    assert p.iterations == 3 and abs(p.sigma_luminance - 3.0) < 1e-7
    assert (p.sigma_depth, p.sigma_albedo, p.normal_log2_power) == (d.sigma_depth, d.sigma_albedo, d.normal_log2_power)
    C, A, N, D, V = svgf_inputs(8, 8, 1)
    for bad in (dict(iterations=9), dict(iterations=-1), dict(sigma_luminance=0.0), dict(sigma_luminance=-1.0), dict(sigma_luminance=float("nan")),
                dict(sigma_depth=0.0), dict(sigma_depth=float("nan")), dict(sigma_albedo=-2.0), dict(sigma_albedo=float("nan")),
                dict(normal_log2_power=17), dict(normal_log2_power=-1)):
        with pytest.raises(hip.MortHipError) as e:
            hip.svgf_host(C, A, N, D, V, params=hip.SvgfParams(**bad))
        assert e.value.status == -1
    L = hip.lib()
    out, vout, rgba = np.zeros((8, 8, 3), np.float32), np.zeros((8, 8), np.float32), np.zeros((8, 8, 4), np.uint8)
    ptr = lambda x: x.ctypes.data if x is not None else None  # noqa: E731
    call = lambda c, a, n, d, v, o, vo, r, w=8, h=8: L.mort_hip_svgf_host(C_.byref(p), w, h, 2, ptr(c), ptr(a), ptr(n), ptr(d), ptr(v), ptr(o),  # noqa: E731
                                                                          ptr(vo), ptr(r), None)
    assert call(C, A, N, D, V, out, vout, rgba) == 0
    assert call(C, A, N, D, None, None, None, None) == 0, "the variance and every output may be NULL"
    assert call(None, A, N, D, V, out, vout, rgba) == -1 and call(C, None, N, D, V, out, vout, rgba) == -1
    assert call(C, A, None, D, V, out, vout, rgba) == -1 and call(C, A, N, None, V, out, vout, rgba) == -1
    assert call(C, A, N, D, V, out, vout, rgba, w=0) == -1 and call(C, A, N, D, V, out, vout, rgba, h=-3) == -1
    assert call(C, A, N, D, V, C, vout, rgba) == -1, "accum_out aliases accum"
    assert call(C, A, N, D, V, A, vout, rgba) == -1, "accum_out aliases albedo"
    assert call(C, A, N, D, V, out, V, rgba) == -1, "variance_out aliases variance"
    assert call(C, A, N, D, V, out, D, rgba) == -1, "variance_out aliases depth"
    assert call(C, A, N, D, V, out, out, rgba) == -1, "two outputs alias"
    assert L.mort_hip_svgf_host(None, 8, 8, 1, ptr(C), ptr(A), ptr(N), ptr(D), None, ptr(out), None, None, None) == -1
    assert L.mort_hip_svgf_defaults(None) == -1


# ---- quality: 96 px, 8 frames x 4 spp against 400 spp at the last camera, as tests/test_temporal_host.py ----
_CASES = {}


def _case(sid, kind):
    """(accumulated colour, its variance, the last frame's features, the last frame alone, the 400 spp reference)"""
    if (sid, kind) not in _CASES:
        _, cams, frames, ref = _sequence(sid, kind)
        th = hip.TemporalHistory(cams[0].image_width, cams[0].image_height, nthreads=NT)
        for (acc, f), c in zip(frames, cams):
            out = th.step(acc, f["normal"], f["depth"], c)
        _CASES[(sid, kind)] = (out["accum"], out["variance"], frames[-1][1], frames[-1][0], ref)
    return _CASES[(sid, kind)]


def _rmse(a, ref):
    return float(np.sqrt(np.mean((_g(a) - _g(ref)) ** 2)))


def _svgf(col, f, var):
    return hip.svgf_host(col, f["albedo"], f["normal"], f["depth"], var, nthreads=NT)["accum"]


# (scene, camera, limit on svgf / denoise(accumulated), limit on svgf with the temporal variance / svgf with the spatial estimate):
# measured 0.612, 0.614, 0.744, 0.832, 0.941, 0.808 and 0.818, 0.814, 0.784, 0.876, 0.542, 0.910
QUALITY = [(6, "still", 0.64, 0.85), (6, "keys", 0.64, 0.85), (1, "still", 0.77, 0.81), (1, "mouse", 0.86, 0.90), (3, "still", 0.97, 0.57),
           (8, "still", 0.83, 0.93)]


@pytest.mark.parametrize("sid,kind,limit_parent,limit_spatial", QUALITY)
def test_svgf_beats_the_denoiser_on_the_accumulated_colour_and_the_variance_guides(sid, kind, limit_parent, limit_spatial):
    acc, var, f, _, ref = _case(sid, kind)
    e_svgf = _rmse(_svgf(acc, f, var), ref)
    e_parent = _rmse(hip.denoise_host(acc, f["albedo"], f["normal"], f["depth"], nthreads=NT)["accum"], ref)
    e_spatial = _rmse(_svgf(acc, f, None), ref)
    print(f"scene {sid} {kind}: svgf {e_svgf:.4f}, denoise(accumulated) {e_parent:.4f} (ratio {e_svgf / e_parent:.3f}), "
          f"svgf with the spatial estimate {e_spatial:.4f} (ratio {e_svgf / e_spatial:.3f})")
    if sid == 3:
        assert e_svgf <= e_parent
    else:
        assert e_svgf < e_parent
    assert e_svgf < e_spatial, "the temporal variance must guide better than the spatial estimate"
    assert e_svgf <= limit_parent * e_parent and e_svgf <= limit_spatial * e_spatial


# a single 4 spp frame, no history: measured 0.811, 0.839
@pytest.mark.parametrize("sid,limit", [(1, 0.84), (6, 0.87)])
def test_svgf_beats_the_denoiser_on_a_single_frame(sid, limit):
    _, _, f, frame, ref = _case(sid, "still")
    e_svgf = _rmse(_svgf(frame, f, None), ref)
    e_parent = _rmse(hip.denoise_host(frame, f["albedo"], f["normal"], f["depth"], nthreads=NT)["accum"], ref)
    print(f"scene {sid} single frame: svgf {e_svgf:.4f}, denoise {e_parent:.4f} (ratio {e_svgf / e_parent:.3f})")
    assert e_svgf < e_parent and e_svgf <= limit * e_parent


# ---- CLI ----
def _run(*args, cwd):
    return subprocess.run([MORT, *map(str, args)], cwd=cwd, capture_output=True, text=True, timeout=600)


def _ppm(path, W, H):
    data = open(path, "rb").read()
    return np.frombuffer(data[len(data) - W * H * 3:], dtype=np.uint8).reshape(H, W, 3)


def test_cli_svgf_matches_the_python_chain(tmp_path):
    p = _run(1, "--mode", "host", "--width", 64, "--spp", 4, "--svgf", "--out", "x.ppm", "--dump-f32", "raw.f32", "--threads", NT, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["svgf_seconds"] > 0 and "denoise_seconds" not in line and "temporal_seconds" not in line
    W, H = line["width"], line["height"]
    world, cam = host.build_scene(1, width=64, spp=4)
    r = hip.render_host(world, cam, nthreads=NT)
    f = hip.render_features_host(world, cam, nthreads=NT)
    want = hip.svgf_host(r["accum"], f["albedo"], f["normal"], f["depth"], None, nthreads=NT)
    img = _ppm(tmp_path / "x.ppm", W, H)
    assert (img[::-1] == want["rgba"][..., :3]).all() or (img == want["rgba"][..., :3]).all()
    assert not (want["rgba"] == r["rgba"]).all(), "the filter changed the image"
    raw = np.fromfile(tmp_path / "raw.f32", dtype=np.float32)
    assert (raw.view(np.uint32) == r["accum"].reshape(-1).view(np.uint32)).all(), "--dump-f32 is the raw render"


def test_cli_temporal_svgf_matches_the_python_chain(tmp_path):
    p = _run(6, "--mode", "host", "--width", 64, "--spp", 4, "--frames", 4, "--keys", ".D.D", "--temporal", "--svgf", "--variance-out", "V",
             "--out", "x.ppm", "--dump-f32", "raw.f32", "--threads", NT, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["svgf_seconds"] > 0 and line["temporal_seconds"] > 0 and "denoise_seconds" not in line
    _, cam = host.build_scene(6, width=64, spp=4)
    cams = [cam]
    for k in ".D.":
        cams.append(_moved(cams[-1], None if k == "." else k))
    _, frames = _frames(6, cams)
    th = hip.TemporalHistory(cam.image_width, cam.image_height, nthreads=NT)
    for (acc, f), c in zip(frames, cams):
        out = th.step(acc, f["normal"], f["depth"], c)
    f = frames[-1][1]
    want = hip.svgf_host(out["accum"], f["albedo"], f["normal"], f["depth"], out["variance"], nthreads=NT)
    W, H = line["width"], line["height"]
    img = _ppm(tmp_path / "x.ppm", W, H)
    assert (img[::-1] == want["rgba"][..., :3]).all() or (img == want["rgba"][..., :3]).all()
    assert (np.fromfile(tmp_path / "V", dtype=np.float32).view(np.uint32) == out["variance"].reshape(-1).view(np.uint32)).all(), \
        "--variance-out stays the temporal step's variance"
    raw = np.fromfile(tmp_path / "raw.f32", dtype=np.float32)
    assert (raw.view(np.uint32) == frames[-1][0].reshape(-1).view(np.uint32)).all(), "--dump-f32 is the raw render"


@pytest.mark.parametrize("flags,word", [(["--svgf", "--denoise", "--mode", "host"], "exclude"), (["--svgf", "--gpus", 2, "--gather", "shm"], "single-GPU")])
def test_cli_rejects_svgf_with_denoise_or_several_gpus(tmp_path, flags, word):
    p = _run(1, "--width", 32, "--spp", 1, "--out", "x.ppm", *flags, cwd=tmp_path)
    assert p.returncode != 0 and word in p.stderr
    assert not list(tmp_path.iterdir())


def test_cli_without_the_flag_keeps_its_json_keys(tmp_path):
    p = _run(2, "--mode", "host", "--width", 32, "--spp", 1, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    keys = set(json.loads(p.stdout.strip().splitlines()[-1]))
    assert keys == {"scene", "width", "height", "spp_nominal", "spp_effective", "depth", "mode", "gpus", "seconds", "msamples_per_s",
                    "kernel_seconds", "gather_seconds", "segments", "algorithmic_hbm_bytes", "hbm_GBps", "hbm_frac_of_8TBps",
                    "reference_walks", "kernel"}
    p = _run(2, "--mode", "host", "--width", 32, "--spp", 1, "--svgf", cwd=tmp_path)
    assert set(json.loads(p.stdout.strip().splitlines()[-1])) == keys | {"svgf_seconds"}


# ---- kernel resources ----
def test_new_kernels_use_no_private_memory():
    lib = os.path.join(ROOT, "mort_amd", "lib", "libmort_hip.so")
    script = os.path.join(ROOT, "scripts", "kernel_resources.py")
    out = subprocess.run([sys.executable, script, lib], capture_output=True, text=True, check=True).stdout
    rows = [l.split() for l in out.splitlines() if l.startswith("svgf_")]
    names = {" ".join(r[:-7]) for r in rows}
    assert names == {f"svgf_prep_kernel<{v}, {t}>" for v in ("false", "true") for t in ("false", "true")} | \
        {f"svgf_iter_kernel<{l}, {t}>" for l in ("false", "true") for t in (0, 1, 2)} | {"svgf_passthrough_kernel"}, names
    for r in rows:
        vspill, sspill, private = int(r[-4]), int(r[-3]), int(r[-2])
        assert vspill == 0 and sspill == 0 and private == 0, r
    assert subprocess.run([sys.executable, script, lib, "--check"], capture_output=True, text=True).returncode == 0, "make hip's --check"
