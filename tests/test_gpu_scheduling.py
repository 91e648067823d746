"""Scheduling never reaches the pixels: heavy waves, spread fetches, partitions and every tuning variable of the megakernels and the
wavefront pipeline, each against the CPU oracle, bit for bit (image, fp32 accumulators, per-pixel segment counts, final XORWOW words).

Every case renders TWO frames on one context: the first one is ordered by the one-sample cost probe, the second one by the first
frame's costs (and its heavy-wave head comes from them).  Frame 1 is compared with the oracle's frame 1, frame 2 with the oracle's
frame 2 from frame 1's streams.  The oracle does not see the variables, so each reference is rendered once per module.

Heavy waves (mega_bvh.h FastArgs.heavy_*) are asserted to have run: with MORT_GEN_HEAVY_DEBUG=1 the host prints the head the device
chose for each launch ("[heavy] head tiles N of T"), and N must be > 0 on both frames."""
import re

import numpy as np
import pytest

from mort_amd import host, hip, structs as S
from tests.test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

_REFS = {}
_HEAVY_LINE = re.compile(r"\[heavy\] head tiles (\d+) of (\d+), lanes (\d+)")


def _scene(key):
    """(world, cam) for a case key; worlds are rebuilt per call (upload_world drops the cost history, so every case starts cold)."""
    if key == "s8":  # the book-2 final scene: 36 864 pixels (above 32 k), 0.19 pixels per lane -> heavy waves by default
        world, cam = host.build_scene(8, width=192, spp=4)
        assert (cam.image_width, cam.image_height, cam.bounce_limit) == (192, 192, 40)
        return world, cam
    if key == "flat":
        return _flat_world_with_fog()
    if key == "s1":
        return host.build_scene(1, width=400, spp=9)
    if key == "s6":  # Cornell box, depth 50, through the unified-tree kernel (MORT_GEN_MIN_PRIMS=0)
        world, cam = host.build_scene(6, width=96, spp=4)
        assert cam.bounce_limit == 50
        return world, cam
    raise KeyError(key)


def _flat_world_with_fog():
    """A random brute-force world as in test_host_mode._random_world, plus a dense constant medium in view (like scene 8's fog ball):
    its pixels run to the bounce limit, so the frame's longest chains are long enough for heavy_count_kernel's chain-bound test."""
    from tests.test_host_mode import _random_world
    from tests.worlds import set_view
    rng = np.random.default_rng(4242)
    w, _ = _random_world(rng, n_spheres=24, n_quads=6, n_boxes=2, n_media=1, with_light=False)
    L = host.lib()
    b = L.mort_add_sphere(w.ptr, host.vec3(0.0, 1.2, 0.0), 1.6, S.MAT_DIELECTRIC, L.mort_add_dielectric(w.ptr, 1.5), True)
    col = L.mort_add_solid_color(w.ptr, host.vec3(0.9, 0.9, 0.9))
    L.mort_add_constant_medium(w.ptr, S.OBJ_SPHERE, b, 8.0, S.MAT_ISOTROPIC, L.mort_add_isotropic(w.ptr, S.TEXTURE_SOLID, col), False)
    w.c.bvh_mode = False
    _, cam = host.build_scene(2, width=192, spp=4, depth=40, aspect=1.0)
    for i, v in enumerate((0.5, 0.6, 0.7)):
        cam.background.e[i] = v
    set_view(cam, (0.0, 2.0, 9.0), (0.0, 1.2, 0.0), vfov=40, defocus=0.0)
    assert (cam.image_width, cam.image_height) == (192, 192)
    return w, cam


def _refs(oracle, key):
    if key not in _REFS:
        world, cam = _scene(key)
        r1 = oracle.render(world, cam, nthreads=16)
        r2 = oracle.render(world, cam, states=r1["states"].copy(), nthreads=16)
        _REFS[key] = (r1, r2)
    return _REFS[key]


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _frame(ctx, cam, oracle, mode=hip.MODE_MEGA):
    out = ctx.render(cam, mode=mode, want_accum=True, want_segments=True)
    out["states"] = ctx.rng_store(cam.image_width, cam.image_height, oracle.STATE_DTYPE)
    return out


def _heads(capfd):
    return [int(m.group(1)) for m in _HEAVY_LINE.finditer(capfd.readouterr().err)]


def _two_frames(ctx, oracle, key, capfd=None, mode=hip.MODE_MEGA):
    """Frame 1 and frame 2 of `key` on ctx, each against the oracle; returns (out1, out2, heads1, heads2) (heads: [heavy] lines)."""
    world, cam = _scene(key)
    ref1, ref2 = _refs(oracle, key)
    ctx.set_partition(0, 1, 8)
    ctx.upload_world(world)
    ctx.rng_seed(S.DEFAULT_SEED, cam.image_width, cam.image_height)
    if capfd is not None:
        capfd.readouterr()
    out1 = _frame(ctx, cam, oracle, mode)
    h1 = _heads(capfd) if capfd is not None else None
    assert_same(out1, ref1)
    out2 = _frame(ctx, cam, oracle, mode)
    h2 = _heads(capfd) if capfd is not None else None
    assert_same(out2, ref2)
    return out1, out2, h1, h2


def _assert_heavy_ran(h1, h2):
    # frame 1's head comes from the cost probe's totals (pixel_write<true> adds them up), frame 2's from frame 1's
    assert len(h1) == 1 and h1[0] > 0, f"frame 1: heavy-wave head {h1}"
    assert len(h2) == 1 and h2[0] > 0, f"frame 2: heavy-wave head {h2}"


HEAVY_SHAPES = [None, "3,2,12,50", "1,1,4,100", "4,1,8,75", "2,1,1,30",
                "1,1,1,1",      # every wave heavy with one lane, head as large as it can be (percent 1)
                "3,3,64,100"]   # no ordinary waves: the heavy ones take the head, then what is left


@pytest.mark.parametrize("heavy", HEAVY_SHAPES, ids=lambda h: "default" if h is None else h)
@pytest.mark.parametrize("key", ["s8", "flat"])
def test_heavy_waves_against_the_oracle(gpu_ctx, oracle, monkeypatch, capfd, key, heavy):
    """Frames under 8 pixels per lane with >= 32 k pixels run heavy waves by default (1024-thread workgroups, the device decides the
    head); forced shapes too.  Both frames equal the oracle's and both ran heavy waves."""
    env = {"MORT_GEN_MIN_PRIMS": "0", "MORT_GEN_HEAVY_DEBUG": "1"}
    if heavy is not None:
        env["MORT_GEN_HEAVY"] = heavy
    _setenv(monkeypatch, env)
    out1, out2, h1, h2 = _two_frames(gpu_ctx, oracle, key, capfd)
    assert out1["stats"]["kernel_name"].startswith("mega_gen_kernel<1024"), out1["stats"]["kernel_name"]
    _assert_heavy_ran(h1, h2)


@pytest.mark.parametrize("key", ["s8", "flat"])
def test_no_heavy_launch_has_no_head(gpu_ctx, oracle, monkeypatch, capfd, key):
    _setenv(monkeypatch, {"MORT_GEN_MIN_PRIMS": "0", "MORT_GEN_HEAVY_DEBUG": "1", "MORT_GEN_NO_HEAVY": "1"})
    out1, _, h1, h2 = _two_frames(gpu_ctx, oracle, key, capfd)
    assert out1["stats"]["kernel_name"].startswith("mega_gen_kernel")
    assert h1 == [] and h2 == []


@pytest.mark.parametrize("shift", ["0", "3"])
@pytest.mark.parametrize("heavy", [None, "3,2,12,50", "1,1,4,100"], ids=lambda h: "default" if h is None else h)
def test_heavy_waves_with_spread_fetches(gpu_ctx, oracle, monkeypatch, capfd, heavy, shift):
    """MORT_SPREAD_SHIFT < 6 makes the ordinary fetch spread a wave's slots over a generation of the cost order (gen_tiles > 0); heavy-role
    fetches hand out whole tiles in order (pixel_fetch's !by_role).  Both kinds in one launch."""
    env = {"MORT_GEN_HEAVY_DEBUG": "1", "MORT_SPREAD_SHIFT": shift}
    if heavy is not None:
        env["MORT_GEN_HEAVY"] = heavy
    _setenv(monkeypatch, env)
    out1, _, h1, h2 = _two_frames(gpu_ctx, oracle, "s8", capfd)
    assert out1["stats"]["kernel_name"].startswith("mega_gen_kernel<1024")
    _assert_heavy_ran(h1, h2)


@pytest.mark.parametrize("env", [
    {"MORT_GEN_HEAVY": "3,2,12,50", "MORT_GEN_BLOCK_SIZE": "1024"},
    {"MORT_GEN_HEAVY": "3,2,12,50", "MORT_GEN_BLOCK_SIZE": "1024", "MORT_SPREAD_SHIFT": "3"},
    {"MORT_GEN_HEAVY": "1,1,4,100", "MORT_GEN_BLOCK_SIZE": "1024", "MORT_SPREAD_SHIFT": "3"},
    {"MORT_GEN_HEAVY": "3,2,12,50"},  # the workgroup size the launch picks itself (256 threads for a rank of 8)
    {"MORT_GEN_HEAVY": "3,2,12,50", "MORT_SPREAD_SHIFT": "3"},
], ids=lambda e: ",".join(f"{k[5:]}={v}" for k, v in e.items()))
@pytest.mark.parametrize("nranks,rpb", [(2, 8), (8, 8), (3, 16)])
def test_heavy_waves_on_row_partitions(gpu_ctx, oracle, monkeypatch, capfd, nranks, rpb, env):
    """Each rank of a row partition renders frame 1 and frame 2 back to back (the cost key includes rank and partition) with forced heavy
    waves (a rank has fewer than 32 k pixels: not the default); the owned rows compose to the oracle's two frames, rows not owned stay
    untouched, and every rank's launches ran heavy waves."""
    _setenv(monkeypatch, dict(env, MORT_GEN_HEAVY_DEBUG="1"))
    world, cam = _scene("s8")
    W, H = cam.image_width, cam.image_height
    refs = _refs(oracle, "s8")
    got = [dict(rgba=np.zeros((H, W, 4), np.uint8), accum=np.zeros((H, W, 3), np.float32), seg=np.zeros((H, W), np.uint32),
                states=np.zeros(W * H, oracle.STATE_DTYPE).reshape(H, W), total=0) for _ in range(2)]
    owned = np.zeros(H, int)
    try:
        for r in range(nranks):
            gpu_ctx.set_partition(r, nranks, rpb)
            gpu_ctx.upload_world(world)
            gpu_ctx.rng_seed(S.DEFAULT_SEED, W, H)
            rows = [gpu_ctx.global_row(l) for l in range(gpu_ctx.local_rows(H))]
            others = np.setdiff1d(np.arange(H), rows)
            owned[rows] += 1
            capfd.readouterr()
            for f in range(2):
                out = _frame(gpu_ctx, cam, oracle)
                heads = _heads(capfd)
                name = out["stats"]["kernel_name"]
                assert name.startswith("mega_gen_kernel<" + env.get("MORT_GEN_BLOCK_SIZE", "256") + ","), name  # a rank here: < 32 k pixels, 256 threads
                assert len(heads) == 1 and heads[0] > 0, f"rank {r} frame {f + 1}: heavy-wave head {heads}"
                assert (out["rgba"][others] == 0).all() and (out["segments_px"][others] == 0).all()  # rows not owned are left untouched
                g = got[f]
                g["rgba"][rows] = out["rgba"][rows]
                g["accum"][rows] = out["accum"][rows]
                g["seg"][rows] = out["segments_px"][rows]
                g["states"][rows] = out["states"].reshape(H, W)[rows]
                g["total"] += out["stats"]["segments"]
    finally:
        gpu_ctx.set_partition(0, 1, 8)
    assert (owned == 1).all()
    for f in range(2):
        g, ref = got[f], refs[f]
        assert (g["rgba"] == ref["rgba"]).all(), f"frame {f + 1}: uchar4 image differs"
        assert (g["accum"].view(np.uint32) == ref["accum"].view(np.uint32)).all(), f"frame {f + 1}: fp32 accumulators differ"
        assert (g["seg"] == ref["segments_px"]).all() and g["total"] == ref["segments"], f"frame {f + 1}: segment counts differ"
        st = ref["states"].reshape(H, W)
        assert (g["states"]["d"] == st["d"]).all() and (g["states"]["v"] == st["v"]).all(), f"frame {f + 1}: final RNG states differ"


# ---- the tuning variables, each on the kernel that reads it ----

@pytest.mark.parametrize("env,want", [
    ({"MORT_LANE_CAP": "1"}, None), ({"MORT_LANE_CAP": "7"}, None), ({"MORT_LANE_CAP": "63"}, None),
    ({"MORT_TILE_KEY": "sum"}, None), ({"MORT_TILE_KEY": "sum", "MORT_CHAIN_BOUND": "1"}, "mega_bvh_kernel<256, false, true, false>"),
    ({"MORT_TILE_KEY": "sum", "MORT_CHAIN_BOUND": "0"}, "mega_bvh_kernel<256, false, false, false>"),
    ({"MORT_FAST_BLOCKS_PER_CU": "1"}, None), ({"MORT_FAST_BLOCKS_PER_CU": "1", "MORT_FAST_BLOCK_SIZE": "1024"}, "mega_bvh_kernel<1024,"),
    ({"MORT_LANE_CAP": "7", "MORT_FAST_BLOCK_SIZE": "1024"}, "mega_bvh_kernel<1024,"),
    ({"MORT_WAVE_LINES": "1"}, None),  # a non-profile build: the per-wave log is allocated, the kernel writes nothing
], ids=lambda e: ",".join(f"{k[5:]}={v}" for k, v in e.items()) if isinstance(e, dict) else str(e))
def test_bvh_megakernel_knobs(gpu_ctx, oracle, monkeypatch, env, want):
    """Scene 1 at 400x225x9 (0.47 pixels per lane: 256-thread drain kernels, spread fetches) as in
    test_gpu_parity.test_scheduling_choices_do_not_reach_the_pixels."""
    _setenv(monkeypatch, env)
    out1, out2, _, _ = _two_frames(gpu_ctx, oracle, "s1")
    name = out1["stats"]["kernel_name"]
    assert name.startswith(want or "mega_bvh_kernel<"), name
    assert out2["stats"]["kernel_name"] == name


GEN_KNOBS = [
    {"MORT_LANE_CAP": "1"}, {"MORT_LANE_CAP": "33"},
    {"MORT_TILE_KEY": "sum"}, {"MORT_TILE_KEY": "sum", "MORT_GEN_HEAVY": "3,2,12,50"},
    {"MORT_GEN_DRAIN": "0"}, {"MORT_GEN_DRAIN": "1"}, {"MORT_GEN_DRAIN": "2"}, {"MORT_GEN_DRAIN": "3"},
    {"MORT_GEN_DRAIN": "1", "MORT_GEN_PRIO_LANES": "1"}, {"MORT_GEN_DRAIN": "1", "MORT_GEN_PRIO_LANES": "4"},
    {"MORT_GEN_DRAIN": "7"}, {"MORT_GEN_DRAIN": "-1"},  # outside 0..3: the host keeps the default (3)
    {"MORT_WAVE_LINES": "1"},
]


@pytest.mark.parametrize("env", GEN_KNOBS, ids=lambda e: ",".join(f"{k[5:]}={v}" for k, v in e.items()))
@pytest.mark.parametrize("key", ["s8", "s6"])
def test_unified_tree_megakernel_knobs(gpu_ctx, oracle, monkeypatch, capfd, key, env):
    _setenv(monkeypatch, dict(env, MORT_GEN_MIN_PRIMS="0", MORT_GEN_HEAVY_DEBUG="1"))
    out1, out2, h1, h2 = _two_frames(gpu_ctx, oracle, key, capfd)
    name = out1["stats"]["kernel_name"]
    assert name.startswith("mega_gen_kernel<"), name
    if "MORT_GEN_HEAVY" in env or key == "s8":  # forced, or scene 8's default: heavy waves ran (a tile-sum key makes any frame's head non-empty)
        _assert_heavy_ran(h1, h2)


@pytest.mark.parametrize("block", ["256", "1024"])
@pytest.mark.parametrize("key", ["s8", "s6"])
def test_unified_tree_lds_stack_levels(gpu_ctx, oracle, monkeypatch, key, block):
    """MORT_GEN_DL: bounce-stack levels kept in LDS; the others live in the HBM `deep` buffer at [level - DL][lane].  0, 1 and 2 at depth
    40 / 50 send almost every level there.  The LDS size the launch reports shows the setting arrived (FB * 16 bytes per level), and a
    negative value is clamped to 0."""
    _setenv(monkeypatch, {"MORT_GEN_MIN_PRIMS": "0", "MORT_GEN_BLOCK_SIZE": block})
    lds = {}
    for dl in ("0", "1", "2", "-3"):
        monkeypatch.setenv("MORT_GEN_DL", dl)
        out1, out2, _, _ = _two_frames(gpu_ctx, oracle, key)
        assert out1["stats"]["kernel_name"].startswith(f"mega_gen_kernel<{block},"), out1["stats"]["kernel_name"]
        lds[dl] = out1["stats"]["kernel_lds_bytes"]
        assert out2["stats"]["kernel_lds_bytes"] == lds[dl]
    assert lds["1"] - lds["0"] == lds["2"] - lds["1"] == int(block) * 16
    assert lds["-3"] == lds["0"]


@pytest.mark.parametrize("env,block", [
    ({"MORT_WAVE_THRESHOLDS": "2,2,2"}, None), ({"MORT_WAVE_THRESHOLDS": "64,64,64"}, None),
    ({"MORT_WAVE_TRAV_BLOCK": "256"}, 256), ({"MORT_WAVE_TRAV_BLOCK": "512"}, 512),
    ({"MORT_WAVE_TRAV_BLOCK": "1024"}, 1024),  # the final scene's image admits 1024 threads (its default): wave_gen.hip trav_block_for
    ({"MORT_WAVE_TRAV_BLOCK": "512", "MORT_WAVE_THRESHOLDS": "2,2,2"}, 512),
], ids=lambda e: ",".join(f"{k[5:]}={v}" for k, v in e.items()) if isinstance(e, dict) else str(e))
def test_wavefront_unified_tree_knobs(gpu_ctx, oracle, monkeypatch, env, block):
    """Scene 8 through the wavefront pipeline of unified-tree worlds (wave_gen.hip), which reads MORT_WAVE_THRESHOLDS and
    MORT_WAVE_TRAV_BLOCK; the kernel name shows the traversal's workgroup size."""
    _setenv(monkeypatch, env)
    out1, out2, _, _ = _two_frames(gpu_ctx, oracle, "s8", mode=hip.MODE_WAVE)
    name = out1["stats"]["kernel_name"]
    assert name.startswith("wf_trav_gen<" + (f"{block}," if block else "")), name


@pytest.mark.parametrize("env", [{"MORT_WAVE_SHARE": "2"}, {"MORT_WAVE_SHARE": "8"}],
                         ids=lambda e: ",".join(f"{k[5:]}={v}" for k, v in e.items()))
def test_wavefront_bvh_knobs(gpu_ctx, oracle, monkeypatch, env):
    """Scene 1 through the wavefront pipeline of BVH worlds (mort_hip.hip launch_wave), which reads MORT_WAVE_SHARE: the 64-record
    batches per wave of a traversal front."""
    _setenv(monkeypatch, env)
    out1, _, _, _ = _two_frames(gpu_ctx, oracle, "s1", mode=hip.MODE_WAVE)
    assert out1["stats"]["kernel_name"].startswith("wf_trav<"), out1["stats"]["kernel_name"]
