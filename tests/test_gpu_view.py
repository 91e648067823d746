"""The view on the MI355X: a frame of mort_hip_view_frame* must be, as raw 32-bit words, what the stage calls
give when chained by hand -- render -> features -> [temporal] -> [denoise | SVGF] -- in every configuration; it must leave the
render alone, run asynchronously on a caller's stream, skip the feature pass under a still camera and no longer, forget its
history when told to or when the world changes, share a context with other views, and carry the CLI's post chain."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mort_amd import hip, host
from mort_amd import structs as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORT = os.path.join(ROOT, "mort_amd", "bin", "mort")
SEED = 69420
CONFIGS = [(t, f) for t in (0, 1) for f in (hip.FILTER_NONE, hip.FILTER_DENOISE, hip.FILTER_SVGF)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _eq(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _sequence(cam0):
    """tests/test_gpu_temporal.py::_sequence: frame 0, the same camera (still), then W, then a mouse drag."""
    c1 = S.Camera.from_buffer_copy(cam0)
    c2 = host.camera_input(S.Camera.from_buffer_copy(c1), "W")
    c3 = host.camera_input(S.Camera.from_buffer_copy(c2), None, (6, -3))
    return [cam0, c1, c2, c3]


def _hand_chain(ctx, cams, mode=hip.MODE_MEGA, seed=SEED, configs=CONFIGS):
    """The stage calls chained by hand over `cams`, one render sequence from `seed`: per frame a dict config -> the buffers a view
    of that configuration holds after the frame."""
    W, H = cams[0].image_width, cams[0].image_height
    ctx.rng_seed(seed, W, H)
    th = hip.TemporalHistory(W, H, backend=ctx)
    frames = []
    for cam in cams:
        r = ctx.render(cam, mode=mode, want_accum=True)
        f = ctx.render_features(cam)
        t = th.step(r["accum"], f["normal"], f["depth"], cam)
        t = dict(accum=t["accum"].copy(), variance=t["variance"].copy(), rgba=t["rgba"].copy(), history=th.history.copy())
        per = {}
        for temporal, filt in configs:
            e = dict(raw_accum=r["accum"], albedo=f["albedo"], normal=f["normal"], depth=f["depth"], rgba=r["rgba"])
            col, var = r["accum"], None
            if temporal:
                e.update(accum=t["accum"], variance=t["variance"], history=t["history"], rgba=t["rgba"])
                col, var = t["accum"], t["variance"]
            if filt == hip.FILTER_DENOISE:
                d = ctx.denoise(col, f["albedo"], f["normal"], f["depth"])
                e.update(filtered=d["accum"], rgba=d["rgba"])
            elif filt == hip.FILTER_SVGF:
                d = ctx.svgf(col, f["albedo"], f["normal"], f["depth"], var)
                e.update(filtered=d["accum"], rgba=d["rgba"])
            per[(temporal, filt)] = e
        frames.append(per)
    return frames


def _check_view(ctx, cams, want, config, mode=hip.MODE_MEGA, seed=SEED, what=""):
    """A view of `config` over `cams` from `seed` against the hand chain's frames; returns the stats of every frame."""
    W, H = cams[0].image_width, cams[0].image_height
    temporal, filt = config
    ctx.rng_seed(seed, W, H)
    stats = []
    with ctx.view(W, H, temporal=temporal, filter=filt) as v:
        for i, cam in enumerate(cams):
            out = v.frame(cam, mode=mode)
            e = want[i][config]
            assert _eq(out["rgba"], e["rgba"]), f"{what} config {config} frame {i}: rgba differs"
            for name in hip.VIEW_BUFFERS:
                if name in e:
                    assert _eq(v.read(name), e[name]), f"{what} config {config} frame {i}: {name} differs"
                else:  # a buffer this configuration does not produce
                    with pytest.raises(hip.MortHipError) as err:
                        v.read(name)
                    assert err.value.status == -1
            stats.append(out["stats"])
    return stats


# ---- 1. bits against the chain ----
@pytest.mark.parametrize("sid", range(1, 11))
def test_view_frames_are_the_hand_chain_on_every_scene(gpu_ctx, sid):
    world, cam0 = host.build_scene(sid, width=96, spp=4)
    gpu_ctx.upload_world(world)
    cams = _sequence(cam0)
    want = _hand_chain(gpu_ctx, cams)
    for config in CONFIGS:
        stats = _check_view(gpu_ctx, cams, want, config, what=f"scene {sid}")
        assert [s["frame"] for s in stats] == [0, 1, 2, 3]
        assert [s["features_reused"] for s in stats] == [0, 1, 0, 0]
        assert [s["history_reset"] for s in stats] == [1, 0, 0, 0]
        for s in stats:
            assert s["render"]["seconds"] > 0 and s["render"]["segments"] > 0 and s["device_seconds"] >= s["render"]["seconds"]
            assert (s["temporal_seconds"] > 0) == bool(config[0]) and (s["filter_seconds"] > 0) == (config[1] != hip.FILTER_NONE)
            assert (s["features_seconds"] > 0) == (not s["features_reused"])


@pytest.mark.parametrize("sid", [1, 9])
def test_view_frames_are_the_hand_chain_in_wavefront_mode(gpu_ctx, sid):
    world, cam0 = host.build_scene(sid, width=96, spp=4)
    gpu_ctx.upload_world(world)
    cams = _sequence(cam0)
    want = _hand_chain(gpu_ctx, cams, mode=hip.MODE_WAVE)
    for config in CONFIGS:
        _check_view(gpu_ctx, cams, want, config, mode=hip.MODE_WAVE, what=f"scene {sid} wave")


@pytest.mark.parametrize("sid,width,aspect", [(6, 101, 1.37), (1, 1200, None)])
def test_view_frames_are_the_hand_chain_on_ragged_and_full_frames(gpu_ctx, sid, width, aspect):
    world, cam0 = host.build_scene(sid, width=width, spp=4, aspect=aspect)
    W, H = cam0.image_width, cam0.image_height
    assert (W % 64 != 0 and H % 4 != 0) if aspect else (W, H) == (1200, 675)
    gpu_ctx.upload_world(world)
    cams = _sequence(cam0)
    configs = CONFIGS if aspect else [(1, hip.FILTER_SVGF), (0, hip.FILTER_DENOISE)]
    want = _hand_chain(gpu_ctx, cams, configs=configs)
    for config in configs:
        _check_view(gpu_ctx, cams, want, config, what=f"{W}x{H}")


# ---- 2. the render is untouched ----
@pytest.mark.parametrize("sid,mode", [(1, hip.MODE_MEGA), (9, hip.MODE_MEGA), (6, hip.MODE_WAVE)])
def test_view_leaves_the_render_alone(gpu_ctx, sid, mode):
    world, cam0 = host.build_scene(sid, width=128, spp=4)
    W, H = cam0.image_width, cam0.image_height
    gpu_ctx.upload_world(world)
    cams = _sequence(cam0)

    gpu_ctx.rng_seed(SEED, W, H)
    plain = [gpu_ctx.render(c, mode=mode, want_accum=True) for c in cams]
    plain_states = gpu_ctx.rng_store(W, H)
    after_plain = gpu_ctx.render(cam0, mode=mode, want_accum=True)

    gpu_ctx.rng_seed(SEED, W, H)
    with gpu_ctx.view(W, H) as v:
        for i, c in enumerate(cams):
            out = v.frame(c, mode=mode)
            assert _eq(v.read("raw_accum"), plain[i]["accum"]), f"frame {i}: raw accumulators"
            assert out["stats"]["render"]["segments"] == plain[i]["stats"]["segments"]
            assert out["stats"]["render"]["kernel_name"] == plain[i]["stats"]["kernel_name"]
        assert (gpu_ctx.rng_store(W, H) == plain_states).all(), "RNG states after the view's frames"
        after_view = gpu_ctx.render(cam0, mode=mode, want_accum=True)
    assert _eq(after_view["rgba"], after_plain["rgba"]) and _eq(after_view["accum"], after_plain["accum"])
    assert after_view["stats"]["segments"] == after_plain["stats"]["segments"]


# ---- 3. asynchrony ----
def test_frames_enqueued_on_a_torch_stream_match_blocking_frames(gpu_ctx):
    import torch
    world, cam0 = host.build_scene(6, width=160, spp=4)
    W, H = cam0.image_width, cam0.image_height
    gpu_ctx.upload_world(world)
    cams = _sequence(cam0)[1:]
    dev = torch.device("cuda:0")

    gpu_ctx.rng_seed(SEED, W, H)
    with gpu_ctx.view(W, H) as v:
        blocking = [v.frame(c)["rgba"] for c in cams]
        last = {k: v.read(k) for k in ("filtered", "accum", "variance", "history")}

    stream = torch.cuda.Stream(device=dev)
    outs = [torch.zeros(W * H * 4, dtype=torch.uint8, device=dev) for _ in cams]
    gpu_ctx.rng_seed(SEED, W, H)
    with gpu_ctx.view(W, H) as v:
        with torch.cuda.stream(stream):
            for c, o in zip(cams, outs):
                assert v.frame_device(c, o) is None  # stats == NULL: enqueued, not waited for
        stream.synchronize()
        for i, (o, b) in enumerate(zip(outs, blocking)):
            assert (o.cpu().numpy().reshape(H, W, 4) == b).all(), f"frame {i}"
        for k, a in last.items():
            assert _eq(v.read(k), a), k
        # with statistics the same call waits once and reports
        with torch.cuda.stream(stream):
            st = v.frame_device(cams[-1], outs[0], sync=True)
        assert st["frame"] == 3 and st["features_reused"] == 1 and st["device_seconds"] > 0

    # the host-buffer form without statistics
    gpu_ctx.rng_seed(SEED, W, H)
    L = hip.lib()
    with gpu_ctx.view(W, H) as v:
        for i, c in enumerate(cams):
            rgba = np.zeros((H, W, 4), dtype=np.uint8)
            assert L.mort_hip_view_frame(v._h, C.byref(c), hip.MODE_MEGA, rgba.ctypes.data, None) == 0
            assert (rgba == blocking[i]).all(), f"mort_hip_view_frame, frame {i}"


# ---- 4. still-camera reuse and invalidation ----
def test_feature_reuse_and_invalidation(gpu_ctx):
    world6, cam0 = host.build_scene(6, width=96, spp=4)
    world1, cam1 = host.build_scene(1, width=96, spp=4, aspect=1.0)  # square, as scene 6
    W, H = cam0.image_width, cam0.image_height
    assert (cam1.image_width, cam1.image_height) == (W, H)
    gpu_ctx.upload_world(world6)
    gpu_ctx.rng_seed(SEED, W, H)
    moved = host.camera_input(S.Camera.from_buffer_copy(cam0), "D")
    with gpu_ctx.view(W, H) as v:
        with pytest.raises(hip.MortHipError):
            v.read("albedo")  # no frame yet
        first = v.frame(cam0)
        first_bufs = {k: v.read(k) for k in ("filtered", "accum", "variance", "history")}
        fresh = gpu_ctx.render_features(cam0)
        seen = [first["stats"]]
        for _ in range(2):
            seen.append(v.frame(S.Camera.from_buffer_copy(cam0))["stats"])
            for k in ("albedo", "normal", "depth"):
                assert _eq(v.read(k), fresh[k]), f"reused {k}"
        assert [s["features_reused"] for s in seen] == [0, 1, 1]
        assert [s["history_reset"] for s in seen] == [1, 0, 0] and [s["frame"] for s in seen] == [0, 1, 2]
        assert seen[1]["features_seconds"] == 0 and seen[0]["features_seconds"] > 0
        s = v.frame(moved)["stats"]
        assert s["features_reused"] == 0 and s["history_reset"] == 0
        fm = gpu_ctx.render_features(moved)
        assert all(_eq(v.read(k), fm[k]) for k in ("albedo", "normal", "depth"))

        # reset: the history goes, the features stay; the frame is a first frame of the same render sequence
        gpu_ctx.rng_seed(SEED, W, H)
        v.frame(moved)
        v.reset()
        gpu_ctx.rng_seed(SEED, W, H)
        r = v.frame(cam0)
        assert r["stats"]["history_reset"] == 1 and r["stats"]["frame"] == 0 and r["stats"]["features_reused"] == 0
        assert _eq(r["rgba"], first["rgba"])
        for k, a in first_bufs.items():
            assert _eq(v.read(k), a), f"after reset: {k}"
        v.reset()
        gpu_ctx.rng_seed(SEED, W, H)
        r = v.frame(cam0)
        assert r["stats"]["history_reset"] == 1 and r["stats"]["features_reused"] == 1 and _eq(r["rgba"], first["rgba"])

        # another scene: features recomputed, history gone -- a first-frame result
        assert v.frame(cam0)["stats"]["frame"] == 1
        gpu_ctx.upload_world(world1)
        gpu_ctx.rng_seed(SEED, W, H)
        r = v.frame(cam1)
        assert r["stats"]["features_reused"] == 0 and r["stats"]["history_reset"] == 1 and r["stats"]["frame"] == 0
        want = _hand_chain(gpu_ctx, [cam1], configs=[(1, hip.FILTER_SVGF)])[0][(1, hip.FILTER_SVGF)]
        assert _eq(r["rgba"], want["rgba"])
        for k in ("albedo", "normal", "depth", "accum", "variance", "history", "filtered"):
            assert _eq(v.read(k), want[k]), f"after upload_world: {k}"
        s = v.frame(S.Camera.from_buffer_copy(cam1))["stats"]
        assert s["features_reused"] == 1 and s["history_reset"] == 0 and s["frame"] == 1
        # the same world uploaded again counts as a new one, although the camera is bit-identical
        gpu_ctx.upload_world(world1)
        gpu_ctx.rng_seed(SEED, W, H)
        r = v.frame(S.Camera.from_buffer_copy(cam1))
        assert r["stats"]["features_reused"] == 0 and r["stats"]["history_reset"] == 1 and r["stats"]["frame"] == 0
        assert _eq(r["rgba"], want["rgba"])


# ---- 5. several views, errors ----
def test_two_views_of_different_sizes_share_a_context(gpu_ctx):
    world, cam_a0 = host.build_scene(6, width=96, spp=4)
    _, cam_b0 = host.build_scene(6, width=144, spp=4)
    gpu_ctx.upload_world(world)
    seqs = {"a": _sequence(cam_a0), "b": _sequence(cam_b0)}
    cfg = {"a": (1, hip.FILTER_SVGF), "b": (1, hip.FILTER_DENOISE)}
    size = {k: (s[0].image_width, s[0].image_height) for k, s in seqs.items()}
    alone = {}
    for k in "ab":
        gpu_ctx.rng_seed(SEED, *size[k])
        with gpu_ctx.view(*size[k], temporal=cfg[k][0], filter=cfg[k][1]) as v:
            alone[k] = []
            for c in seqs[k]:
                rgba = v.frame(c)["rgba"]
                alone[k].append(dict(rgba=rgba, filtered=v.read("filtered"), history=v.read("history")))
    # alternately: the context holds one set of pixel states, so each view's are stored and loaded around its frames
    states = {k: hip.seed_states_host(SEED, *size[k]) for k in "ab"}
    views = {k: gpu_ctx.view(*size[k], temporal=cfg[k][0], filter=cfg[k][1]) for k in "ab"}
    try:
        for i in range(4):
            for k in "ab":
                gpu_ctx.rng_load(states[k], *size[k])
                rgba = views[k].frame(seqs[k][i])["rgba"]
                states[k] = gpu_ctx.rng_store(*size[k])
                assert _eq(rgba, alone[k][i]["rgba"]), f"view {k} frame {i}"
            for k in "ab":  # the other view's frame left this one's buffers alone
                assert _eq(views[k].read("filtered"), alone[k][i]["filtered"]) and _eq(views[k].read("history"), alone[k][i]["history"])
    finally:
        for v in views.values():
            v.close()


def test_error_codes(gpu_ctx):
    world, cam = host.build_scene(6, width=96, spp=4)
    _, other = host.build_scene(6, width=64, spp=4)
    W, H = cam.image_width, cam.image_height
    gpu_ctx.upload_world(world)
    gpu_ctx.rng_seed(SEED, W, H)
    for bad in (dict(filter=7), dict(temporal=3), dict(sp=hip.SvgfParams(iterations=9)), dict(filter=hip.FILTER_DENOISE, dp=hip.DenoiseParams(sigma_color=0.0))):
        with pytest.raises(hip.MortHipError) as e:
            gpu_ctx.view(W, H, **bad)
        assert e.value.status == -1, bad
    for w, h in ((0, H), (W, -1)):
        with pytest.raises(hip.MortHipError) as e:
            gpu_ctx.view(w, h)
        assert e.value.status == -1
    with gpu_ctx.view(W, H) as v:
        with pytest.raises(hip.MortHipError) as e:
            v.frame(other)
        assert e.value.status == -1  # MORT_ERR_INVALID: not the view's size
        with pytest.raises(hip.MortHipError) as e:
            v.frame(cam, mode=17)
        assert e.value.status == -1
        gpu_ctx.rng_seed(SEED, 64, other.image_height)
        with pytest.raises(hip.MortHipError) as e:
            v.frame(cam)
        assert e.value.status == -5  # MORT_ERR_NO_RNG: states of another size
        try:
            gpu_ctx.set_partition(0, 2)
            gpu_ctx.rng_seed(SEED, W, H)
            with pytest.raises(hip.MortHipError) as e:
                v.frame(cam)
            assert e.value.status == -6  # MORT_ERR_UNSUPPORTED: not the whole image
        finally:
            gpu_ctx.set_partition(0, 1)
        gpu_ctx.rng_seed(SEED, W, H)
        first = v.frame(cam)  # none of the refused calls left anything behind
        assert first["stats"]["frame"] == 0
        want = _hand_chain(gpu_ctx, [cam], configs=[(1, hip.FILTER_SVGF)])[0][(1, hip.FILTER_SVGF)]
        assert _eq(first["rgba"], want["rgba"])
        with pytest.raises(hip.MortHipError) as e:
            gpu_ctx._chk(hip.lib().mort_hip_view_read(v._h, 99, first["rgba"].ctypes.data), "mort_hip_view_read")
        assert e.value.status == -1


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from mort_amd import hip, host
world, cam = host.build_scene(6, width=64, spp=4)
W, H = cam.image_width, cam.image_height
ctx = hip.Context(0)
v = ctx.view(W, H)
w = ctx.view(W, H, temporal=0, filter=hip.FILTER_DENOISE)
def status(fn):
    try:
        fn()
    except hip.MortHipError as e:
        return e.status
    return 0
assert status(lambda: v.frame(cam)) == -4, "MORT_ERR_NO_WORLD"
ctx.upload_world(world)
assert status(lambda: v.frame(cam)) == -5, "MORT_ERR_NO_RNG"
ctx.rng_seed(69420, W, H)
a = v.frame(cam)
b = w.frame(cam)
assert a["stats"]["frame"] == 0 and a["rgba"].any() and b["rgba"].any()
ctx.close()  # two views alive: mort_hip_shutdown frees them
try:
    v.frame(cam)
except RuntimeError as e:
    assert "closed" in str(e)
else:
    raise AssertionError("a view of a closed context must not be usable")
v.close(); w.close()  # no-ops
print("child ok")
"""


def test_closing_the_context_frees_live_views(tmp_path):
    """Once, in a child process: the errors a view passes on from the render before a world and RNG states exist, then
    mort_hip_shutdown with two views alive."""
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    p = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


# ---- 6. CLI ----
def _ppm(path, W, H):
    data = open(path, "rb").read()
    return np.frombuffer(data[len(data) - W * H * 3:], dtype=np.uint8).reshape(H, W, 3)


@pytest.mark.parametrize("flags", [["--temporal", "--svgf"], ["--temporal", "--denoise"], ["--svgf"], ["--denoise"], ["--temporal"], []])
def test_cli_post_chain_goes_through_a_view(gpu_ctx, tmp_path, flags):
    temporal = "--temporal" in flags
    filt = hip.FILTER_SVGF if "--svgf" in flags else hip.FILTER_DENOISE if "--denoise" in flags else hip.FILTER_NONE
    args = [MORT, "6", "--width", "96", "--spp", "4", "--frames", "4", "--keys", ".DW", *flags, "--out", "x.ppm", "--features-out", "P",
            "--dump-f32", "raw.f32"] + (["--variance-out", "V"] if temporal else [])
    p = subprocess.run(args, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    base = {"scene", "width", "height", "spp_nominal", "spp_effective", "depth", "mode", "gpus", "seconds", "msamples_per_s", "kernel_seconds",
            "gather_seconds", "segments", "algorithmic_hbm_bytes", "hbm_GBps", "hbm_frac_of_8TBps", "reference_walks", "kernel"}
    extra = ({"temporal_seconds"} if temporal else set()) | ({"svgf_seconds"} if filt == hip.FILTER_SVGF else set()) | \
        ({"denoise_seconds"} if filt == hip.FILTER_DENOISE else set())
    assert set(line) == base | extra
    assert all(line[k] > 0 for k in extra) and line["kernel_seconds"] > 0 and line["segments"] > 0

    world, cam = host.build_scene(6, width=96, spp=4)
    cams = [cam]
    for k in ".DW":
        cams.append(host.camera_input(S.Camera.from_buffer_copy(cams[-1]), None if k == "." else k))
    gpu_ctx.upload_world(world)
    want = _hand_chain(gpu_ctx, cams, configs=[(int(temporal), filt)])[-1][(int(temporal), filt)]
    W, H = line["width"], line["height"]
    img = _ppm(tmp_path / "x.ppm", W, H)
    assert (img[::-1] == want["rgba"][..., :3]).all() or (img == want["rgba"][..., :3]).all()
    files = {"raw.f32": "raw_accum", "P.albedo.f32": "albedo", "P.normal.f32": "normal", "P.depth.f32": "depth"}
    if temporal:
        files["V"] = "variance"
    for name, key in files.items():
        got = np.fromfile(tmp_path / name, dtype=np.float32)
        assert got.size == want[key].size and (got.view(np.uint32) == want[key].reshape(-1).view(np.uint32)).all(), name


def test_cli_without_the_flags_adds_no_key_and_no_view(tmp_path):
    p = subprocess.run([MORT, "2", "--width", "64", "--spp", "4", "--out", "x.ppm"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert set(json.loads(p.stdout.strip().splitlines()[-1])) == {
        "scene", "width", "height", "spp_nominal", "spp_effective", "depth", "mode", "gpus", "seconds", "msamples_per_s", "kernel_seconds",
        "gather_seconds", "segments", "algorithmic_hbm_bytes", "hbm_GBps", "hbm_frac_of_8TBps", "reference_walks", "kernel"}
