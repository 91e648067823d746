"""The view's C ABI without a GPU (include/mort_hip.h): the exported symbols, the ctypes structures against the
C ones, the defaults, the argument and parameter checks, and the CLI's `--mode host` path, which the view must leave alone."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from mort_amd import hip, host
from mort_amd import structs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORT = os.path.join(ROOT, "mort_amd", "bin", "mort")
NT = min(16, os.cpu_count() or 1)
INVALID = -1

VIEW_SYMBOLS = ["mort_hip_view_defaults", "mort_hip_view_check_params", "mort_hip_view_create", "mort_hip_view_destroy", "mort_hip_view_reset",
                "mort_hip_view_frame", "mort_hip_view_frame_device", "mort_hip_view_read"]


def test_library_exports_the_view():
    L = C.CDLL(hip.LIB_PATH)
    for n in VIEW_SYMBOLS:
        assert n in hip.EXPORTS
        assert getattr(L, n) is not None


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "mort_hip.h"
#define F(s, f) printf("%s.%s %zu\n", #s, #f, offsetof(s, f))
int main(void) {
    printf("mort_view_params %zu\nmort_view_stats %zu\nmort_stats %zu\n", sizeof(mort_view_params), sizeof(mort_view_stats), sizeof(mort_stats));
    F(mort_view_params, width); F(mort_view_params, height); F(mort_view_params, temporal); F(mort_view_params, filter);
    F(mort_view_params, tp); F(mort_view_params, dp); F(mort_view_params, sp);
    F(mort_view_stats, render); F(mort_view_stats, features_seconds); F(mort_view_stats, temporal_seconds); F(mort_view_stats, filter_seconds);
    F(mort_view_stats, device_seconds); F(mort_view_stats, frame); F(mort_view_stats, features_reused); F(mort_view_stats, history_reset);
    printf("codes %d %d %d %d %d %d %d %d %d %d %d\n", MORT_VIEW_FILTER_NONE, MORT_VIEW_FILTER_DENOISE, MORT_VIEW_FILTER_SVGF, MORT_VIEW_RAW_ACCUM,
           MORT_VIEW_ACCUM, MORT_VIEW_FILTERED, MORT_VIEW_VARIANCE, MORT_VIEW_ALBEDO, MORT_VIEW_NORMAL, MORT_VIEW_DEPTH, MORT_VIEW_HISTORY);
    return 0;
}
"""


def test_ctypes_structures_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler builds the library; the probe needs the same one"
    (tmp_path / "probe.c").write_text(PROBE)
    subprocess.run([cc, "-std=gnu11", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "probe"), str(tmp_path / "probe.c")], check=True)
    out = subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout
    got = {l.rsplit(" ", 1)[0]: int(l.rsplit(" ", 1)[1]) for l in out.splitlines() if not l.startswith("codes")}
    want = {"mort_view_params": C.sizeof(hip.ViewParams), "mort_view_stats": C.sizeof(hip.ViewStats), "mort_stats": C.sizeof(hip.Stats)}
    for name, cls in (("mort_view_params", hip.ViewParams), ("mort_view_stats", hip.ViewStats)):
        for f, _ in cls._fields_:
            want[f"{name}.{f}"] = getattr(cls, f).offset
    assert got == want
    codes = [int(x) for x in [l for l in out.splitlines() if l.startswith("codes")][0].split()[1:]]
    assert codes[:3] == [hip.FILTER_NONE, hip.FILTER_DENOISE, hip.FILTER_SVGF]
    assert codes[3:] == [hip.VIEW_BUFFERS[k][0] for k in ("raw_accum", "accum", "filtered", "variance", "albedo", "normal", "depth", "history")]


def _bytes(s):
    return bytes(memoryview(s))


def test_defaults_are_the_three_stages_defaults():
    L = hip.lib()
    p = hip.ViewParams.__new__(hip.ViewParams)
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    assert L.mort_hip_view_defaults(C.byref(p)) == 0
    assert (p.width, p.height, p.temporal, p.filter) == (0, 0, 1, hip.FILTER_SVGF)
    assert _bytes(p.tp) == _bytes(hip.TemporalParams())
    assert _bytes(p.dp) == _bytes(hip.DenoiseParams())
    assert _bytes(p.sp) == _bytes(hip.SvgfParams())
    assert L.mort_hip_view_defaults(None) == INVALID
    q = hip.ViewParams(96, 54, temporal=0)
    assert (q.width, q.height, q.temporal, q.filter) == (96, 54, 0, hip.FILTER_SVGF)


def test_null_arguments_are_invalid():
    L = hip.lib()
    p = hip.ViewParams(32, 32)
    out = C.c_void_p()
    cam = S.Camera()
    buf = (C.c_uint8 * 16)()
    fake = C.c_void_p(1)  # never dereferenced: every call below must fail on its NULL argument first
    assert L.mort_hip_view_create(None, C.byref(p), C.byref(out)) == INVALID and not out.value
    assert L.mort_hip_view_create(fake, None, C.byref(out)) == INVALID
    assert L.mort_hip_view_create(fake, C.byref(p), None) == INVALID
    assert L.mort_hip_view_frame(None, C.byref(cam), 0, buf, None) == INVALID
    assert L.mort_hip_view_frame(fake, None, 0, buf, None) == INVALID
    assert L.mort_hip_view_frame(fake, C.byref(cam), 0, None, None) == INVALID
    assert L.mort_hip_view_frame_device(None, C.byref(cam), 0, buf, None, None) == INVALID
    assert L.mort_hip_view_frame_device(fake, None, 0, buf, None, None) == INVALID
    assert L.mort_hip_view_frame_device(fake, C.byref(cam), 0, None, None, None) == INVALID
    assert L.mort_hip_view_read(None, 0, buf) == INVALID
    assert L.mort_hip_view_reset(None) == INVALID
    assert L.mort_hip_view_check_params(None) == INVALID
    L.mort_hip_view_destroy(None)  # a no-op, like free(NULL)


def _check(**kw):
    nested = {k: kw.pop(k) for k in list(kw) if "." in k}
    p = hip.ViewParams(kw.pop("width", 96), kw.pop("height", 54), **kw)
    for k, v in nested.items():
        s, f = k.split(".")
        setattr(getattr(p, s), f, v)
    return hip.lib().mort_hip_view_check_params(C.byref(p))


def test_parameter_validation_is_the_stages_own():
    assert _check() == 0
    for filt in (hip.FILTER_NONE, hip.FILTER_DENOISE, hip.FILTER_SVGF):
        for t in (0, 1):
            assert _check(temporal=t, filter=filt) == 0
    # sizes, switches
    for bad in (dict(width=0), dict(width=-4), dict(height=0), dict(height=-1), dict(filter=3), dict(filter=-1), dict(temporal=2), dict(temporal=-1)):
        assert _check(**bad) == INVALID, bad
    # the stage in use refuses what its own call refuses ...
    for bad in ({"sp.iterations": 9}, {"sp.iterations": -1}, {"sp.sigma_luminance": 0.0}, {"sp.sigma_depth": -1.0}, {"sp.sigma_albedo": float("nan")},
                {"sp.normal_log2_power": 17}):
        assert _check(filter=hip.FILTER_SVGF, **bad) == INVALID, bad
    for bad in ({"dp.iterations": 9}, {"dp.iterations": -1}, {"dp.sigma_color": 0.0}, {"dp.sigma_depth": -0.5}, {"dp.normal_log2_power": -1}):
        assert _check(filter=hip.FILTER_DENOISE, **bad) == INVALID, bad
    for bad in ({"tp.max_samples": -1}, {"tp.motion_max_samples": -1}, {"tp.depth_tolerance": 1.5}, {"tp.normal_min": -2.0}):
        assert _check(temporal=1, **bad) == INVALID, bad
    # ... and the same values are what the stage calls themselves refuse
    z3, z1 = np.zeros((2, 2, 3), np.float32), np.zeros((2, 2), np.float32)
    with pytest.raises(hip.MortHipError):
        hip.svgf_host(z3, z3, z3, z1, None, params=hip.SvgfParams(iterations=9))
    with pytest.raises(hip.MortHipError):
        hip.denoise_host(z3, z3, z3, z1, params=hip.DenoiseParams(sigma_color=0.0))
    # a stage that is switched off is not read
    assert _check(filter=hip.FILTER_DENOISE, **{"sp.iterations": 9}) == 0
    assert _check(filter=hip.FILTER_NONE, **{"dp.iterations": 9, "sp.iterations": 9}) == 0
    assert _check(temporal=0, **{"tp.depth_tolerance": 1.5}) == 0


# ---- the CLI's host mode goes no way near a view: the files are those of the host stage chain ----
def _run(*args, cwd):
    return subprocess.run([MORT, *map(str, args)], cwd=cwd, capture_output=True, text=True, timeout=600)


def _ppm(path, W, H):
    data = open(path, "rb").read()
    return np.frombuffer(data[len(data) - W * H * 3:], dtype=np.uint8).reshape(H, W, 3)


def _same_image(img, rgba):
    return (img[::-1] == rgba[..., :3]).all() or (img == rgba[..., :3]).all()


def _host_chain(sid, width, keys):
    """The host stage chain over the CLI's scripted frames: (last accum, last features, temporal out, cams)."""
    world, cam = host.build_scene(sid, width=width, spp=4)
    cams = [cam]
    for k in keys:
        cams.append(host.camera_input(S.Camera.from_buffer_copy(cams[-1]), None if k == "." else k))
    th = hip.TemporalHistory(cam.image_width, cam.image_height, nthreads=NT)
    states = None
    for c in cams:
        r = hip.render_host(world, c, states=states, nthreads=NT, want_segments=False)
        states = r["states"]
        f = hip.render_features_host(world, c, nthreads=NT)
        out = th.step(r["accum"], f["normal"], f["depth"], c)
    return r, f, out


def test_cli_host_mode_temporal_svgf_files_are_unchanged(tmp_path):
    p = _run(6, "--mode", "host", "--width", 64, "--spp", 4, "--frames", 4, "--keys", ".D.D", "--temporal", "--svgf", "--variance-out", "V",
             "--out", "x.ppm", "--dump-f32", "raw.f32", "--features-out", "P", "--threads", NT, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["mode"] == "host" and line["svgf_seconds"] > 0 and line["temporal_seconds"] > 0 and "denoise_seconds" not in line
    r, f, out = _host_chain(6, 64, ".D.")
    want = hip.svgf_host(out["accum"], f["albedo"], f["normal"], f["depth"], out["variance"], nthreads=NT)
    W, H = line["width"], line["height"]
    assert _same_image(_ppm(tmp_path / "x.ppm", W, H), want["rgba"])
    assert (np.fromfile(tmp_path / "V", dtype=np.float32).view(np.uint32) == out["variance"].reshape(-1).view(np.uint32)).all()
    assert (np.fromfile(tmp_path / "raw.f32", dtype=np.float32).view(np.uint32) == r["accum"].reshape(-1).view(np.uint32)).all()
    for k in ("albedo", "normal", "depth"):
        assert (np.fromfile(tmp_path / f"P.{k}.f32", dtype=np.float32).view(np.uint32) == f[k].reshape(-1).view(np.uint32)).all(), k


def test_cli_host_mode_denoise_files_are_unchanged(tmp_path):
    p = _run(1, "--mode", "host", "--width", 64, "--spp", 4, "--denoise", "--features-out", "P", "--out", "x.ppm", "--dump-f32", "raw.f32",
             "--threads", NT, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["denoise_seconds"] > 0 and "svgf_seconds" not in line and "temporal_seconds" not in line
    world, cam = host.build_scene(1, width=64, spp=4)
    r = hip.render_host(world, cam, nthreads=NT)
    f = hip.render_features_host(world, cam, nthreads=NT)
    den = hip.denoise_host(r["accum"], f["albedo"], f["normal"], f["depth"], nthreads=NT)
    assert _same_image(_ppm(tmp_path / "x.ppm", line["width"], line["height"]), den["rgba"])
    assert (np.fromfile(tmp_path / "raw.f32", dtype=np.float32).view(np.uint32) == r["accum"].reshape(-1).view(np.uint32)).all()
    for k in ("albedo", "normal", "depth"):
        assert (np.fromfile(tmp_path / f"P.{k}.f32", dtype=np.float32).view(np.uint32) == f[k].reshape(-1).view(np.uint32)).all(), k
