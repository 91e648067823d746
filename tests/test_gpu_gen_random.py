"""The unified-tree kernels (mega_gen_kernel and its throughput variant, wf_trav_gen, the tree form of feat_kernel) and the host's
choice between them and mega_kernel on the catalogue of random worlds without a reference BVH (tests/worlds.py GEN_RANDOM): LDS
images up to 82 KB, primitives in LDS and read from L2 on both sides of the 48 KB rule, trees at the depth cap, 75 chain ids,
worlds 1e6 away from the origin, radii over four decades, sheets and slivers, exact duplicates, cameras on both sides of mnear and
beyond reach, every workgroup shape.  Every comparison is bit for bit against the CPU oracle (tests/test_gpu_parity.py
assert_same); what the host is expected to pick comes from tests/worlds.py gen_random_prediction, which
tests/test_gen_random_host.py checks on the CPU."""
import numpy as np
import pytest

from mort_amd import hip, structs as S
from tests.feature_ref import assert_same_words, oracle_features
from tests.test_gpu_parity import assert_same, render_gpu
from tests.test_gpu_throughput import expected_substream
from tests.worlds import (GEN_RANDOM, GEN_FAMILIES, GEN_LIMIT_SIZES, GEN_MIN_PRIMS, gen_random_case, gen_random_camera,
                          gen_random_prediction)

pytestmark = pytest.mark.gpu

NAMES = sorted(GEN_RANDOM)
UNSUPPORTED = -6  # MORT_ERR_UNSUPPORTED (include/mort_hip.h)
_refs = {}
_walks = {}


def _views(name):
    return range(len(gen_random_case(name)[1]))


def _oracle_frames(oracle, name, k):
    """the oracle's first and second frame of a view, computed once and shared"""
    if (name, k) not in _refs:
        w = gen_random_case(name)[0]
        cam = gen_random_camera(name, k)
        r1 = oracle.render(w, cam, nthreads=8)
        r2 = oracle.render(w, cam, states=r1["states"].copy(), nthreads=8)
        _refs[name, k] = (r1, r2)
    return _refs[name, k]


def _status_of(fn):
    with pytest.raises(hip.MortHipError) as e:
        fn()
    return e.value.status


def _mega_name(p, k, block=None):
    """what the kernel's name starts with: mega_gen_kernel<BLOCK, PRIMS_LDS, or mega_kernel"""
    if p["kernel"][k] != "mega_gen_kernel":
        return "mega_kernel"
    return f"mega_gen_kernel<{block}, {'true' if p['prims_in_lds'] else 'false'}, false>" if block else "mega_gen_kernel<"


def _check_mega(out, p, k, block=None):
    kn = out["stats"]["kernel_name"]
    gen = p["kernel"][k] == "mega_gen_kernel"
    assert kn.startswith(_mega_name(p, k, block)) and (gen or kn == "mega_kernel"), (k, kn)
    if gen:
        assert f", {'true' if p['prims_in_lds'] else 'false'}, false>" in kn, (k, kn)
    assert out["stats"]["scene_in_lds"] == int(gen)


def _two_frames(ctx, oracle, name, p):
    """both frames of every view against the oracle; returns (reference walks, segments)"""
    w = gen_random_case(name)[0]
    walks = segs = 0
    for k in _views(name):
        cam = gen_random_camera(name, k)
        r1, r2 = _oracle_frames(oracle, name, k)
        out = render_gpu(ctx, w, cam, oracle=oracle)
        _check_mega(out, p, k)
        assert_same(out, r1)
        out2 = ctx.render(cam, want_accum=True, want_segments=True)   # its tiles ordered by the first frame's costs
        out2["states"] = ctx.rng_store(cam.image_width, cam.image_height, oracle.STATE_DTYPE)
        _check_mega(out2, p, k)
        assert_same(out2, r2)
        for o in (out, out2):
            assert 0 <= o["stats"]["reference_walks"] <= o["stats"]["segments"]
            walks += o["stats"]["reference_walks"]; segs += o["stats"]["segments"]
    return walks, segs


@pytest.mark.parametrize("name", NAMES)
def test_megakernel_mode(gpu_ctx, oracle, monkeypatch, name):
    """every entry from every one of its cameras with MORT_GEN_MIN_PRIMS=0: the oracle's bits, the kernel the CPU test predicts
    (mega_gen_kernel with the predicted PRIMS_LDS within reach, mega_kernel beyond), and a second frame that continues the
    streams.  The referral counter stays within the segment count; it is printed per family for DESIGN.md (-s)."""
    monkeypatch.setenv("MORT_GEN_MIN_PRIMS", "0")
    p = gen_random_prediction(name, min_prims=0)
    walks, segs = _two_frames(gpu_ctx, oracle, name, p)
    fam = GEN_RANDOM[name][0]
    a = _walks.setdefault(fam, [0, 0])
    a[0] += walks; a[1] += segs
    print(f"{name}: reference walks {walks} of {segs} segments; {fam} so far {a[0]} of {a[1]} ({a[0] / a[1]:.2e})")


@pytest.mark.parametrize("name", [n for n in NAMES if GEN_RANDOM[n][1] in (GEN_MIN_PRIMS - 1, GEN_MIN_PRIMS)])
def test_default_kernel_choice_at_47_and_48(gpu_ctx, oracle, monkeypatch, name):
    """without MORT_GEN_MIN_PRIMS the entries of 47 primitives stay on mega_kernel and those of 48 take mega_gen_kernel"""
    monkeypatch.delenv("MORT_GEN_MIN_PRIMS", raising=False)
    p = gen_random_prediction(name)
    assert set(p["kernel"]) == {"mega_gen_kernel" if GEN_RANDOM[name][1] >= GEN_MIN_PRIMS else "mega_kernel"}
    _two_frames(gpu_ctx, oracle, name, p)


# two entries per family, one on each side of the 48 KB rule
SHAPE_CASES = [f"{fam}_{GEN_LIMIT_SIZES[fam][side]}_s{side}" for fam in GEN_FAMILIES for side in (0, 1)]
DRAIN_CASES = ["mixed_300_s0", "ties_360_s1", "instances_300_s1", "line_390_s0"]


def test_shape_cases_cover_both_sides():
    for fam in GEN_FAMILIES:
        assert {gen_random_prediction(n)["prims_in_lds"] for n in SHAPE_CASES if GEN_RANDOM[n][0] == fam} == {True, False}
    assert set(DRAIN_CASES) <= set(SHAPE_CASES) and {gen_random_prediction(n)["prims_in_lds"] for n in DRAIN_CASES} == {True, False}


@pytest.mark.parametrize("name", SHAPE_CASES)
def test_every_workgroup_shape(gpu_ctx, oracle, monkeypatch, name):
    """MORT_GEN_BLOCK_SIZE 1024, 768, 512 and 256 (four stack strides): the named kernel, the oracle's bits"""
    monkeypatch.setenv("MORT_GEN_MIN_PRIMS", "0")
    w = gen_random_case(name)[0]
    p = gen_random_prediction(name, min_prims=0)
    assert p["tree"]["lds_bytes"] + 16 + 16 * 1024 * 2 + 2048 <= 160 * 1024      # 1024 threads are not lowered to 768 (mort_hip.hip)
    for block in (1024, 768, 512, 256):
        monkeypatch.setenv("MORT_GEN_BLOCK_SIZE", str(block))
        for k in _views(name):
            out = render_gpu(gpu_ctx, w, gen_random_camera(name, k), oracle=oracle)
            _check_mega(out, p, k, block)
            assert_same(out, _oracle_frames(oracle, name, k)[0])


@pytest.mark.parametrize("env", [{"MORT_GEN_DRAIN": "0"}, {"MORT_GEN_DRAIN": "1"}, {"MORT_GEN_DRAIN": "2"}, {"MORT_GEN_THRESHOLDS": "2,2,2,2"}],
                         ids=["drain0", "drain1", "drain2", "thresholds2"])
@pytest.mark.parametrize("name", DRAIN_CASES)
def test_drain_modes_and_thresholds(gpu_ctx, oracle, monkeypatch, name, env):
    monkeypatch.setenv("MORT_GEN_MIN_PRIMS", "0")
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    w = gen_random_case(name)[0]
    p = gen_random_prediction(name, min_prims=0)
    for k in _views(name):
        out = render_gpu(gpu_ctx, w, gen_random_camera(name, k), oracle=oracle)
        _check_mega(out, p, k)
        assert_same(out, _oracle_frames(oracle, name, k)[0])


def _wave(ctx, oracle, cam):
    W, H = cam.image_width, cam.image_height
    ctx.rng_seed(S.DEFAULT_SEED, W, H)
    out = ctx.render(cam, mode=hip.MODE_WAVE, want_accum=True, want_segments=True)
    out["states"] = ctx.rng_store(W, H, oracle.STATE_DTYPE)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_wavefront_mode(gpu_ctx, oracle, name):
    """the wavefront pipeline on every camera within reach: wf_trav_gen with the predicted PRIMS_LDS, the oracle's bits; a camera
    beyond reach has no kernel in this mode: MORT_ERR_UNSUPPORTED"""
    w = gen_random_case(name)[0]
    p = gen_random_prediction(name)
    gpu_ctx.set_partition(0, 1, 8)
    gpu_ctx.upload_world(w)
    for k in _views(name):
        cam = gen_random_camera(name, k)
        if not p["in_reach"][k]:
            gpu_ctx.rng_seed(S.DEFAULT_SEED, cam.image_width, cam.image_height)
            assert _status_of(lambda: gpu_ctx.render(cam, mode=hip.MODE_WAVE)) == UNSUPPORTED
            continue
        out = _wave(gpu_ctx, oracle, cam)
        kn = out["stats"]["kernel_name"]
        assert kn.startswith("wf_trav_gen<") and kn.endswith(f", {'true' if p['prims_in_lds'] else 'false'}>"), kn
        assert_same(out, _oracle_frames(oracle, name, k)[0])


@pytest.mark.parametrize("name", SHAPE_CASES)
def test_wavefront_traversal_blocks(gpu_ctx, oracle, monkeypatch, name):
    """MORT_WAVE_TRAV_BLOCK 256, 512 and 1024: the named kernel, the oracle's bits"""
    w = gen_random_case(name)[0]
    p = gen_random_prediction(name)
    gpu_ctx.set_partition(0, 1, 8)
    gpu_ctx.upload_world(w)
    for block in (256, 512, 1024):
        monkeypatch.setenv("MORT_WAVE_TRAV_BLOCK", str(block))
        for k in _views(name):
            out = _wave(gpu_ctx, oracle, gen_random_camera(name, k))
            assert out["stats"]["kernel_name"] == f"wf_trav_gen<{block}, {'true' if p['prims_in_lds'] else 'false'}>", out["stats"]["kernel_name"]
            assert_same(out, _oracle_frames(oracle, name, k)[0])


@pytest.mark.parametrize("name", NAMES)
def test_feature_pass(gpu_ctx, monkeypatch, name):
    """render_features from the first camera against the oracle's first hits, word for word: with the tree, and with the world
    uploaded under MORT_NO_GEN=1 (the item scan)"""
    w = gen_random_case(name)[0]
    cam = gen_random_camera(name, 0)
    ref = oracle_features(w, cam, nthreads=8)
    gpu_ctx.set_partition(0, 1, 8)
    gpu_ctx.upload_world(w)
    assert_same_words(gpu_ctx.render_features(cam), ref, f"{name} with the tree")
    monkeypatch.setenv("MORT_NO_GEN", "1")
    gpu_ctx.upload_world(w)
    assert_same_words(gpu_ctx.render_features(cam), ref, f"{name} without the tree")


@pytest.mark.parametrize("name", [n for n in NAMES if GEN_RANDOM[n][1] <= 150])
def test_throughput_mode_is_its_definition(gpu_ctx, oracle, monkeypatch, name):
    """MORT_MODE_THROUGHPUT on the entries of at most 150 primitives, a frame 16 to 20 wide from the second camera: the
    <..., true> kernel computes the oracle's arithmetic on the sub-streams, as tests/test_gpu_throughput.py defines it"""
    monkeypatch.setenv("MORT_GEN_MIN_PRIMS", "0")
    w = gen_random_case(name)[0]
    p = gen_random_prediction(name, min_prims=0)
    cam = gen_random_camera(name, 1, width=16 + NAMES.index(name) % 5)
    gpu_ctx.set_partition(0, 1, 8)
    gpu_ctx.upload_world(w)
    gpu_ctx.rng_seed(S.DEFAULT_SEED, cam.image_width, cam.image_height)
    out = gpu_ctx.render(cam, mode=hip.MODE_THROUGHPUT, want_accum=True)
    kn = out["stats"]["kernel_name"]
    assert kn.startswith("mega_gen_kernel<") and kn.endswith(f", {'true' if p['prims_in_lds'] else 'false'}, true>"), kn
    acc, rgba = expected_substream(oracle, w, cam, S.DEFAULT_SEED)
    assert (out["accum"].view(np.uint32) == acc.view(np.uint32)).all()
    assert (out["rgba"] == rgba).all()


@pytest.mark.parametrize("name", SHAPE_CASES)
def test_one_lane_kernel(oracle, monkeypatch, name):
    """MORT_NO_GEN=1: mega_kernel, the reference side of every comparison above, gives the oracle's bits on worlds of this size"""
    monkeypatch.setenv("MORT_NO_GEN", "1")
    w = gen_random_case(name)[0]
    with hip.Context(0) as ctx:
        for k in _views(name):
            out = render_gpu(ctx, w, gen_random_camera(name, k), oracle=oracle)
            assert out["stats"]["kernel_name"] == "mega_kernel" and out["stats"]["scene_in_lds"] == 0
            assert_same(out, _oracle_frames(oracle, name, k)[0])
