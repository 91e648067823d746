"""The BVH kernels (mega_bvh_kernel, its throughput variant, wave_bvh.h) and the host's choice between them and mega_kernel on
the catalogue of random sphere-BVH worlds (tests/worlds.py BVH_RANDOM): tree shapes the built-in scenes do not have -- deep and
unbalanced trees, radii over four decades, moving spheres, chains of overlapping boxes, nested and duplicated spheres, worlds on
both sides of the 72 KB image limit and of the four-wide stack bound.  Every comparison is bit for bit against the CPU oracle
(tests/test_gpu_parity.py assert_same); what the host is expected to pick comes from tests/worlds.py bvh_random_prediction,
which tests/test_bvh_random_host.py checks on the CPU."""
import numpy as np
import pytest

from mort_amd import hip, structs as S
from tests.feature_ref import assert_same_words, oracle_features
from tests.test_gpu_parity import assert_same, render_gpu
from tests.test_gpu_throughput import expected_substream
from tests.worlds import BVH_RANDOM, bvh_random_case, bvh_random_camera, bvh_random_prediction

pytestmark = pytest.mark.gpu

NAMES = sorted(BVH_RANDOM)
_refs = {}


def _views(name):
    return range(len(bvh_random_case(name)[1]))


def _oracle_frames(oracle, name, k, light=None):
    """the oracle's first and second frame of a view, computed once and shared"""
    key = (name, k, light)
    if key not in _refs:
        w, _, _ = bvh_random_case(name)
        cam = bvh_random_camera(name, k, light=light)
        r1 = oracle.render(w, cam, nthreads=8)
        r2 = oracle.render(w, cam, states=r1["states"].copy(), nthreads=8)
        _refs[key] = (r1, r2)
    return _refs[key]


def _status_of(fn):
    with pytest.raises(hip.MortHipError) as e:
        fn()
    return e.value.status


@pytest.mark.parametrize("name", NAMES)
def test_megakernel_mode(gpu_ctx, oracle, name):
    """every entry from every one of its cameras: the oracle's bits, the kernel family the CPU test predicts, and a second frame
    that continues the streams (its tiles ordered by the first frame's costs).  The referral counter stays within the segment
    count and is positive where the same sphere occurs several times; it is printed for DESIGN.md 4.2 (-s)."""
    w, _, _ = bvh_random_case(name)
    p = bvh_random_prediction(name)
    walks = segs = 0
    for k in _views(name):
        cam = bvh_random_camera(name, k)
        r1, r2 = _oracle_frames(oracle, name, k)
        out = render_gpu(gpu_ctx, w, cam, oracle=oracle)
        assert out["stats"]["kernel_name"].startswith(p["kernel"] + "<" if p["fits"] else p["kernel"]), (k, out["stats"]["kernel_name"])
        assert out["stats"]["scene_in_lds"] == int(p["fits"])
        assert_same(out, r1)
        out2 = gpu_ctx.render(cam, want_accum=True, want_segments=True)
        out2["states"] = gpu_ctx.rng_store(cam.image_width, cam.image_height, oracle.STATE_DTYPE)
        assert_same(out2, r2)
        for o in (out, out2):
            assert 0 <= o["stats"]["reference_walks"] <= o["stats"]["segments"]
            walks += o["stats"]["reference_walks"]; segs += o["stats"]["segments"]
    print(f"{name}: {out['stats']['kernel_name']}, reference walks {walks} of {segs} segments ({walks / segs:.2e})")
    if BVH_RANDOM[name][0] == "ties" and p["fits"]:
        assert walks > 0


@pytest.mark.parametrize("name", NAMES)
def test_wavefront_mode(gpu_ctx, oracle, monkeypatch, name):
    """the wavefront pipeline walks the binary own tree: the oracle's bits where the images fit (the large entries with two
    batches per wave as well), MORT_ERR_UNSUPPORTED where they do not"""
    w, _, _ = bvh_random_case(name)
    p = bvh_random_prediction(name)
    gpu_ctx.set_partition(0, 1, 8)
    gpu_ctx.upload_world(w)
    for k in _views(name):
        cam = bvh_random_camera(name, k)
        W, H = cam.image_width, cam.image_height
        for share in ((None, "2") if BVH_RANDOM[name][1] >= 600 else (None,)):
            if share:
                monkeypatch.setenv("MORT_WAVE_SHARE", share)
            else:
                monkeypatch.delenv("MORT_WAVE_SHARE", raising=False)
            gpu_ctx.rng_seed(S.DEFAULT_SEED, W, H)
            if not p["fits"]:
                assert _status_of(lambda: gpu_ctx.render(cam, mode=hip.MODE_WAVE)) == -6
                continue
            out = gpu_ctx.render(cam, mode=hip.MODE_WAVE, want_accum=True, want_segments=True)
            out["states"] = gpu_ctx.rng_store(W, H, oracle.STATE_DTYPE)
            assert out["stats"]["kernel_name"].startswith("wf_trav<"), out["stats"]["kernel_name"]
            assert_same(out, _oracle_frames(oracle, name, k)[0])


@pytest.mark.parametrize("name,k,width", [("uniform_650_s1", 1, 16), ("ties_64_s0", 1, 24), ("cluster_300_s0", 2, 20), ("scales_64_s1", 0, 17),
                                          ("shells_7_s0", 1, 24), ("line_300_s1", 1, 21)])
def test_throughput_mode_is_its_definition(gpu_ctx, oracle, name, k, width):
    """MORT_MODE_THROUGHPUT on entries that fit (one of them within 1 KB of the image limit, one with repeated spheres): the oracle's
    arithmetic on the sub-streams, as tests/test_gpu_throughput.py defines it"""
    w, _, _ = bvh_random_case(name)
    assert bvh_random_prediction(name)["fits"]
    cam = bvh_random_camera(name, k, width=width)
    gpu_ctx.set_partition(0, 1, 8)
    gpu_ctx.upload_world(w)
    gpu_ctx.rng_seed(S.DEFAULT_SEED, cam.image_width, cam.image_height)
    out = gpu_ctx.render(cam, mode=hip.MODE_THROUGHPUT, want_accum=True)
    name_ = out["stats"]["kernel_name"]
    assert name_.startswith("mega_bvh_kernel<") and name_.endswith(", true>"), name_
    acc, rgba = expected_substream(oracle, w, cam, S.DEFAULT_SEED)
    assert (out["accum"].view(np.uint32) == acc.view(np.uint32)).all()
    assert (out["rgba"] == rgba).all()


def test_throughput_mode_rejects_what_does_not_fit(gpu_ctx):
    """worlds beyond the image limit and worlds without a four-wide tree have no state-machine kernel: MORT_ERR_UNSUPPORTED"""
    tried = 0
    for name in NAMES:
        p = bvh_random_prediction(name)
        if p["fits"] or p["state"] == 1:
            continue
        w, _, _ = bvh_random_case(name)
        cam = bvh_random_camera(name, 0)
        gpu_ctx.set_partition(0, 1, 8)
        gpu_ctx.upload_world(w)
        gpu_ctx.rng_seed(S.DEFAULT_SEED, cam.image_width, cam.image_height)
        assert _status_of(lambda: gpu_ctx.render(cam, mode=hip.MODE_THROUGHPUT)) == -6, name
        tried += 1
    assert tried >= 8


def _shape_cases():
    """the three largest entries that fit and the three with the largest stack bound among the others that fit"""
    P = {n: bvh_random_prediction(n) for n in NAMES}
    fit = [n for n in NAMES if P[n]["fits"]]
    big = sorted(fit, key=lambda n: -P[n]["image"]["fast_bytes"])[:3]
    deep = sorted((n for n in fit if n not in big), key=lambda n: -P[n]["tree"]["stack4"])[:3]
    assert min(P[n]["image"]["fast_bytes"] for n in big) > 68 * 1024 and min(P[n]["tree"]["stack4"] for n in deep) >= 22
    return big + deep


def _recomposed(ctx, w, cam, nranks, rpb):
    W, H = cam.image_width, cam.image_height
    got = dict(rgba=np.zeros((H, W, 4), np.uint8), accum=np.zeros((H, W, 3), np.float32), segments_px=np.zeros((H, W), np.uint32),
               stats=dict(segments=0, rng_draws=0))
    owned = np.zeros(H, int)
    names = set()
    try:
        for r in range(nranks):
            ctx.set_partition(r, nranks, rpb)
            ctx.upload_world(w)
            ctx.rng_seed(S.DEFAULT_SEED, W, H)
            out = ctx.render(cam, want_accum=True, want_segments=True)
            rows = [ctx.global_row(l) for l in range(ctx.local_rows(H))]
            owned[rows] += 1
            for key in ("rgba", "accum", "segments_px"):
                got[key][rows] = out[key][rows]
            for key in ("segments", "rng_draws"):
                got["stats"][key] += out["stats"][key]
            names.add(out["stats"]["kernel_name"].split("<")[0])
    finally:
        ctx.set_partition(0, 1, 8)
    assert (owned == 1).all()
    return got, names


@pytest.mark.parametrize("env,block", [({"MORT_FAST_BLOCK_SIZE": "1024"}, 1024), ({"MORT_FAST_BLOCK_SIZE": "768"}, 768),
                                       ({"MORT_FAST_BLOCK_SIZE": "256"}, 256), ({"MORT_LANE_CAP": "7"}, None), ({"MORT_BVH_DRAIN": "2"}, None),
                                       ("partition", None)],
                         ids=["block1024", "block768", "block256", "lane_cap7", "drain2", "three_ranks_of_16_rows"])
def test_launch_shapes(gpu_ctx, oracle, monkeypatch, env, block):
    """workgroup sizes, a lane cap, the drain mode and a row partition on the entries with the largest LDS images and the deepest
    traversal stacks: none of it reaches the pixels.  A request for 1024 threads is honoured or lowered to 768 as the LDS sum of
    world_images.h (bvh_wide_block_fits) says for the entry's image and stack bound."""
    for name in _shape_cases():
        w, _, _ = bvh_random_case(name)
        p = bvh_random_prediction(name)
        k = 1
        cam = bvh_random_camera(name, k)
        ref = _oracle_frames(oracle, name, k)[0]
        if env == "partition":
            got, names = _recomposed(gpu_ctx, w, cam, 3, 16)
            assert names == {"mega_bvh_kernel"}
            assert_same(got, ref)
            continue
        for key, v in env.items():
            monkeypatch.setenv(key, v)
        out = render_gpu(gpu_ctx, w, cam, oracle=oracle)
        kn = out["stats"]["kernel_name"]
        if block:
            want = block if block != 1024 or p["image"]["wide_fits"] else 768
            assert kn.startswith(f"mega_bvh_kernel<{want},"), (name, kn)
        else:
            assert kn.startswith("mega_bvh_kernel<"), (name, kn)
        assert_same(out, ref)


def test_light_object_on_a_bvh_world(gpu_ctx, oracle):
    """a camera that names a light object takes a BVH world off the BVH kernels: megakernel mode renders it with mega_kernel, to
    the oracle's bits; wavefront mode refuses; the same world without the light named runs mega_bvh_kernel"""
    name = "uniform_300_lit"
    w, _, light = bvh_random_case(name)
    assert light is not None and bvh_random_prediction(name)["fits"]
    for k in _views(name):
        cam = bvh_random_camera(name, k, light=light)
        assert (cam.light_obj_type, cam.light_obj_idx) == light
        r1, _ = _oracle_frames(oracle, name, k, light=light)
        out = render_gpu(gpu_ctx, w, cam, oracle=oracle)
        assert out["stats"]["kernel_name"].startswith("mega_kernel") and out["stats"]["scene_in_lds"] == 0
        assert_same(out, r1)
        gpu_ctx.rng_seed(S.DEFAULT_SEED, cam.image_width, cam.image_height)
        assert _status_of(lambda: gpu_ctx.render(cam, mode=hip.MODE_WAVE)) == -6
        plain = bvh_random_camera(name, k)
        out = render_gpu(gpu_ctx, w, plain, oracle=oracle)
        assert out["stats"]["kernel_name"].startswith("mega_bvh_kernel<")
        assert_same(out, _oracle_frames(oracle, name, k)[0])
        assert not (out["accum"] == r1["accum"]).all()  # sampling the light changes the estimate


@pytest.mark.parametrize("name,k", [("uniform_2_s0", 0), ("scales_2_s1", 1), ("line_3_s0", 1), ("ties_7_s1", 1), ("shells_64_s1", 1),
                                    ("cluster_300_s1", 2), ("scales_640_s1", 2), ("line_670_s0", 1), ("uniform_660_s0", 2),
                                    ("ties_460_s1", 1), ("scales_620_s0", 0), ("ties_1000_s1", 2), ("shells_1000_s0", 0)])
def test_feature_pass(gpu_ctx, name, k):
    """render_features against the oracle's first hits, word for word, on entries in all three tree states"""
    w, _, _ = bvh_random_case(name)
    cam = bvh_random_camera(name, k)
    gpu_ctx.set_partition(0, 1, 8)
    gpu_ctx.upload_world(w)
    assert_same_words(gpu_ctx.render_features(cam), oracle_features(w, cam, nthreads=8), f"{name} view {k}")


def test_feature_pass_cases_cover_the_tree_states():
    states = {bvh_random_prediction(n)["state"] for n, _ in test_feature_pass.pytestmark[0].args[1]}
    assert states == {1, 2, 3}
