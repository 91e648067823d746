"""The tile scheduler, read back: device code that decides only WHEN or WHERE a pixel is rendered leaves a correct pixel correct, so
the parity tests cannot see it.  Here the per-tile costs pixel_write leaves, the one-sample cost probe, the device argsort, the
heavy-wave head and the cost-key cache are read through Context.tile_state() (mort_hip_debug_tile_state) and compared with
tests/tile_ref.py over the ORACLE's per-pixel segment counts; the three helper kernels (sort, heavy count, the frame gather's
de-interleave) are also driven directly on synthetic input.  Every comparison is exact integer equality.

Rendered cases follow test_gpu_scheduling.py: two frames per context, the first ordered by the probe, the second by the first one's
costs.  Each asserts `ordered` and `probed` first, so none passes on a launch that ordered nothing.  Whether a launch orders at all is
`tiles >= 4 * grid` (mort_hip.hip prepare_tile_order); with the 256-thread workgroups small frames get, grid = ceil(tiles / 4), so the
frame sizes here have tile counts that are multiples of 4 (24 tiles across), and the one that must NOT order has 350."""
import numpy as np
import pytest

from mort_amd import host, hip, partition, structs as S
from tests import tile_ref as T
from tests.test_gpu_scheduling import _HEAVY_LINE, _refs as _sched_refs, _scene as _sched_scene
from tests.worlds import set_view

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 255, 256, 257, 1450, 65536]
_REFS = {}


# ---------------------------------------------------------------- helper kernels on synthetic input

def _cost_patterns(n):
    rng = np.random.default_rng(1000 + n)
    hi = rng.integers(0, 4, n, dtype=np.uint32) * np.uint32(0x40000000) + rng.integers(0, 3, n, dtype=np.uint32)  # bits 30 / 31, many ties
    hi[rng.integers(0, n, max(1, n // 7))] = 0xffffffff
    hi[rng.integers(0, n, max(1, n // 7))] = 0x80000000
    return {
        "equal": np.full(n, 77, np.uint32),
        "zero": np.zeros(n, np.uint32),
        "increasing": np.arange(n, dtype=np.uint32) * np.uint32(3) + np.uint32(1),
        "ties": rng.integers(0, max(2, n // 8), n, dtype=np.uint32),
        "high_bits": hi,
    }


@pytest.mark.parametrize("n", SIZES)
def test_tile_sort_kernel(n):
    """mort_tile_sort_desc as the render calls it: keys = cost[order], order is a permutation and IS the stable descending argsort."""
    for name, cost in _cost_patterns(n).items():
        keys, order = hip.debug_tile_sort(cost)
        want_keys, want_order = T.order_desc(cost)
        assert (np.sort(order) == np.arange(n, dtype=np.uint32)).all(), f"{name}: order is no permutation"
        assert (keys == cost[order]).all(), f"{name}: keys != cost[order]"
        assert (order == want_order).all() and (keys == want_keys).all(), f"{name}: not the stable descending argsort"
    if n > 1:
        assert T.order_desc(_cost_patterns(n)["increasing"])[1][0] == n - 1  # the patterns are not all the identity


def _counters(total, rng, junk=True):
    """96 counters whose segment total is `total`, spread over word 0 and the 32 per-workgroup slots; every other word junk"""
    c = rng.integers(1, 1 << 62, T.COUNTERS, dtype=np.uint64) if junk else np.zeros(T.COUNTERS, np.uint64)
    parts = [int(v) for v in rng.integers(0, max(1, total // 40 + 1), 32)]
    rest = total - sum(parts)
    if rest < 0:
        parts, rest = [0] * 32, total
    c[0] = rest
    for k in range(32):
        c[32 + 2 * k] = parts[k]
    assert T.counters_total(c) == total
    return c


def _heavy_keys(n, percent, top):
    """n descending keys: `top` first, then keys AT the threshold ceil(top * percent / 100), one below, one above, random ones, zeros"""
    rng = np.random.default_rng(7 * n + percent)
    thr = -((-top * percent) // 100)
    pool = [thr, thr, max(thr - 1, 0), min(thr + 1, top), 0, 0] + [int(v) for v in rng.integers(0, top + 1, max(0, n - 7), dtype=np.uint64)]
    keys = np.array(sorted(pool[: n - 1], reverse=True), dtype=np.uint32)
    return np.concatenate([np.array([top], np.uint32), keys])[:n]


@pytest.mark.parametrize("percent", [1, 30, 50, 100])
@pytest.mark.parametrize("n", SIZES)
def test_heavy_count_kernel(n, percent):
    """heavy_count_kernel against tile_ref.heavy_head: the threshold (keys equal to it exactly count), zero keys, the cap on both sides
    of the count, no counters / an all-zero total, the chain-bound boundary top * lanes == 2 * total and one segment either side of
    it, the total spread over word 0 and the 32 slots with junk in the words between, and products past 32 bits."""
    rng = np.random.default_rng(31 * n + percent)
    top, lanes = 1000, 36 * 1024
    keys = _heavy_keys(n, percent, top)
    assert int(keys[0]) == top and (np.diff(keys.astype(np.int64)) <= 0).all()
    edge = top * lanes // 2  # top * lanes == 2 * edge
    full = T.heavy_head(keys, percent, n + 5, edge, lanes)
    assert full >= 1
    if n >= 7:
        thr = -((-top * percent) // 100)
        assert int((keys == thr).sum()) >= 2 and full < n  # keys at the threshold are there, and so are keys that do not count
    cases = [(n + 5, None, lanes), (n + 5, np.zeros(T.COUNTERS, np.uint64), lanes)]
    zero_total = _counters(0, rng)  # junk in every word that is not a segment slot: still no total
    cases.append((n + 5, zero_total, lanes))
    for total in (edge - 1, edge, edge + 1):
        cases.append((n + 5, _counters(total, rng), lanes))           # max_r above the count
        cases.append((max(full - 1, 0), _counters(total, rng), lanes))  # max_r below it
        cases.append((full, _counters(total, rng, junk=False), lanes))  # max_r the count itself
    want = [T.heavy_head(keys, percent, m, 0 if c is None else T.counters_total(c), l) for m, c, l in cases]
    assert want[:3] == [0, 0, 0] and full in want and 0 in want[3:]
    for (m, c, l), w in zip(cases, want):
        got = hip.debug_heavy_count(keys, percent, m, c, l)
        assert got == w, (n, percent, m, None if c is None else T.counters_total(c), l, got, w)
    # top = 2^32 - 1 and lanes = 2^21: a 32-bit product would wrap to a small number and call the frame not chain-bound
    big = np.concatenate([np.array([0xffffffff], np.uint32), (keys[1:].astype(np.uint64) * 4000000 % (1 << 32)).astype(np.uint32)])
    big[1:] = np.sort(big[1:])[::-1]
    lanes_big = 1 << 21
    edge_big = 0xffffffff * lanes_big // 2
    for total in (edge_big, edge_big + 1, 1):
        c = _counters(total, rng)
        w = T.heavy_head(big, percent, n + 5, total, lanes_big)
        got = hip.debug_heavy_count(big, percent, n + 5, c, lanes_big)
        assert got == w, (n, percent, total, got, w)
    assert T.heavy_head(big, percent, n + 5, edge_big, lanes_big) >= 1 and T.heavy_head(big, percent, n + 5, edge_big + 1, lanes_big) == 0


POISON = 0xffffffff


@pytest.mark.parametrize("W,H,N,rpb", [(7, 5, 1, 8), (64, 64, 2, 8), (97, 55, 3, 8), (97, 37, 3, 8), (33, 100, 8, 8), (16, 9, 4, 16),
                                        (300, 77, 2, 16)])
def test_deinterleave_kernel(W, H, N, rpb):
    """The frame gather's de-interleave for N ranks on one GPU, at the stride the exchange uses.  Every pixel of `gathered` names its
    (rank, packed row, x); padding is poison.  (97, 55, 3, 8): 7 blocks, the last one partial and rank 0's THIRD (ranks 1 and 2 own two
    whole blocks); (97, 37, 3, 8): 5 blocks, the last one partial and the MIDDLE rank's; (16, 9, 4, 16): one block, ranks 1 to 3 own
    nothing."""
    stride = hip.debug_gather_stride(W, H, N, rpb)
    assert stride == partition.max_local_rows(H, N, rpb) * W
    g = np.full((N, stride), POISON, dtype=np.uint32)
    for r in range(N):
        n = partition.local_rows(H, r, N, rpb)
        ly, x = np.divmod(np.arange(n * W, dtype=np.uint32), np.uint32(W))
        g[r, : n * W] = (np.uint32(r) << np.uint32(24)) | (ly << np.uint32(12)) | x
    if (W, H, N, rpb) == (16, 9, 4, 16):
        assert [partition.local_rows(H, r, N, rpb) for r in range(N)] == [9, 0, 0, 0]
    if (W, H, N, rpb) == (97, 55, 3, 8):
        assert [partition.local_rows(H, r, N, rpb) for r in range(N)] == [23, 16, 16]
    if (W, H, N, rpb) == (97, 37, 3, 8):
        assert [partition.local_rows(H, r, N, rpb) for r in range(N)] == [16, 13, 8]
    frame = hip.debug_deinterleave(g.view(np.uint8), W, H, N, rpb).view(np.uint32).reshape(H, W)
    assert not (frame == POISON).any(), "a padding pixel reached the frame"
    assert (frame == T.deinterleave(g, W, H, N, rpb, stride)).all()
    # and straight from the encoding: pixel (y, x) comes from rank (y // rpb) % N, packed row (y // rpb // N) * rpb + y % rpb
    y = np.arange(H)[:, None]
    assert ((frame >> 24) == (y // rpb) % N).all() and (((frame >> 12) & 0xfff) == (y // rpb // N) * rpb + y % rpb).all()
    assert ((frame & 0xfff) == np.arange(W)[None, :]).all()


# ---------------------------------------------------------------- rendered frames

def _cam1(cam):
    """the camera the cost probe renders with: this one at one sample per pixel (prepare_tile_order sets exactly these fields)"""
    c1 = type(cam).from_buffer_copy(cam)
    c1.samples_per_pixel, c1.sqrt_spp, c1.recip_sqrt_spp, c1.pixel_samples_scale = 1, 1, 1.0, 1.0
    return c1


def _oracle_frames(oracle, key, world, cam, r12=None):
    """the oracle's one-sample frame, frame 1 and frame 2 (from frame 1's streams) of a case, computed once per module"""
    if key not in _REFS:
        if r12 is None:
            r1 = oracle.render(world, cam, nthreads=16)
            r12 = (r1, oracle.render(world, cam, states=r1["states"].copy(), nthreads=16))
        rp = oracle.render(world, _cam1(cam), nthreads=16, want_accum=False)
        _REFS[key] = dict(r1=r12[0], r2=r12[1], rp=rp)
    return _REFS[key]


def _bvh_scene(W=192, H=108, depth=None, spp=4):
    world, cam = host.build_scene(1, width=W, spp=spp, depth=depth, aspect=W / (H + 0.5))
    assert (cam.image_width, cam.image_height) == (W, H)
    return world, cam


def _gen_scene():
    world, cam = _sched_scene("s6")  # Cornell box through the unified-tree kernel (MORT_GEN_MIN_PRIMS=0): 96 x 96, 144 tiles
    assert (cam.image_width, cam.image_height) == (96, 96)
    return world, cam


def _owned_rows(ctx, H):
    return [ctx.global_row(l) for l in range(ctx.local_rows(H))]


def _probe_costs(ts):
    """the costs the launch's order was sorted from: cost[order[i]] = keys[i]"""
    assert (np.sort(ts["order"]) == np.arange(ts["tiles"], dtype=np.uint32)).all(), "order is no permutation"
    cost = np.zeros(ts["tiles"], np.uint32)
    cost[ts["order"]] = ts["keys"]
    return cost


def _same_order(ts, cost, what):
    keys, order = T.order_desc(cost)
    assert (ts["keys"] == keys).all(), f"{what}: keys differ from the costs sorted"
    assert (ts["order"] == order).all(), f"{what}: order is not the stable descending argsort of the costs"


def _frame(ctx, oracle, cam, ref, rows, mode=hip.MODE_MEGA):
    out = ctx.render(cam, mode=mode, want_accum=True, want_segments=True)
    assert (out["rgba"][rows] == ref["rgba"][rows]).all(), "uchar4 image differs from the oracle"
    assert (out["segments_px"][rows] == ref["segments_px"][rows]).all(), "per-pixel segment counts differ from the oracle"
    return out


def _two_frames(ctx, oracle, world, cam, refs, kernel, part=(0, 1, 8), key="max"):
    """Frame 1 (probed) and frame 2 (from frame 1's costs) of one rank; returns the two tile states.  All costs are of the ORACLE's
    segment counts of the rank's rows, packed."""
    W, H = cam.image_width, cam.image_height
    ctx.set_partition(*part)
    ctx.upload_world(world)
    ctx.rng_seed(S.DEFAULT_SEED, W, H)
    rows = _owned_rows(ctx, H)
    tiles_x, tiles = (W + 7) // 8, ((W + 7) // 8) * ((len(rows) + 7) // 8)
    cost_p, cost_1, cost_2 = (T.tile_costs(refs[k]["segments_px"][rows], W, key) for k in ("rp", "r1", "r2"))
    assert cost_1.size == tiles and (cost_1 != cost_2).any() and (cost_1 != cost_p).any() and len(set(cost_1.tolist())) > 4
    states = []
    for f, (ref, before, after) in enumerate([(refs["r1"], cost_p, cost_1), (refs["r2"], cost_1, cost_2)]):
        out = _frame(ctx, oracle, cam, ref, rows)
        assert out["stats"]["kernel_name"].startswith(kernel), out["stats"]["kernel_name"]
        ts = ctx.tile_state()
        what = f"rank {part[0]} of {part[1]}, frame {f + 1}"
        assert ts["ordered"] == 1, (what, ts["tiles"], ts["grid"], ts["block"])
        assert ts["probed"] == (1 if f == 0 else 0), what
        assert (ts["tiles"], ts["tiles_x"], ts["key_sum"]) == (tiles, tiles_x, 1 if key == "sum" else 0), what
        assert ts["tiles"] >= 4 * ts["grid"] and f"<{ts['block']}," in out["stats"]["kernel_name"]
        # what the launch was ordered by: the probe's costs on frame 1 (the one-sample frame from the same streams), frame 1's on frame 2
        assert (_probe_costs(ts) == before).all(), f"{what}: the launch was ordered by other costs than the oracle's " + \
            ("one-sample frame gives" if f == 0 else "frame 1 gives")
        _same_order(ts, before, what)
        # what it left for the next launch
        assert (ts["cost"] == after).all(), f"{what}: tile costs differ from the oracle's segment counts of the packed rows"
        states.append(ts)
    return states


def _bvh_refs(oracle, W=192, H=108, depth=None):
    world, cam = _bvh_scene(W, H, depth)
    return world, cam, _oracle_frames(oracle, ("bvh", W, H, depth), world, cam)


@pytest.mark.parametrize("key", ["max", "sum"])
@pytest.mark.parametrize("kernel", ["mega_bvh_kernel", "mega_gen_kernel"])
def test_tile_costs_and_order(gpu_ctx, oracle, monkeypatch, kernel, key):
    """Both state-machine megakernels, both tile keys: the costs each frame leaves, the probe's costs, and the order made of them."""
    if key == "sum":
        monkeypatch.setenv("MORT_TILE_KEY", "sum")
    if kernel == "mega_gen_kernel":
        monkeypatch.setenv("MORT_GEN_MIN_PRIMS", "0")
        world, cam = _gen_scene()
        refs = _oracle_frames(oracle, "s6", world, cam, _sched_refs(oracle, "s6"))
    else:
        world, cam, refs = _bvh_refs(oracle)
    _two_frames(gpu_ctx, oracle, world, cam, refs, kernel + "<256,", key=key)


def test_tile_costs_of_a_ragged_frame(gpu_ctx, oracle):
    """188 x 105: the last tile column is 4 pixels wide, the last tile row 1 pixel high"""
    world, cam, refs = _bvh_refs(oracle, 188, 105)
    ts = _two_frames(gpu_ctx, oracle, world, cam, refs, "mega_bvh_kernel<256,")
    assert ts[0]["tiles"] == 24 * 14


@pytest.mark.parametrize("nranks,rpb", [(2, 8), (2, 16), (3, 8), (3, 16)])
def test_tile_costs_on_row_partitions(gpu_ctx, oracle, nranks, rpb):
    """Every rank of a partition of the ragged frame: its tiles are tiles of its PACKED rows (a tile of rank 1's holds image rows that are
    not neighbours of rank 0's), so a cost written at the image row's tile lands elsewhere -- or past the array."""
    world, cam, refs = _bvh_refs(oracle, 188, 105)
    try:
        for r in range(nranks):
            _two_frames(gpu_ctx, oracle, world, cam, refs, "mega_bvh_kernel<256,", part=(r, nranks, rpb))
    finally:
        gpu_ctx.set_partition(0, 1, 8)


@pytest.mark.parametrize("shift", [0, 3, 6])
def test_tile_costs_with_spread_fetches(gpu_ctx, oracle, monkeypatch, shift):
    monkeypatch.setenv("MORT_SPREAD_SHIFT", str(shift))
    world, cam, refs = _bvh_refs(oracle)
    for ts in _two_frames(gpu_ctx, oracle, world, cam, refs, "mega_bvh_kernel<256,"):
        assert ts["spread_shift"] == shift
        assert ts["gen_tiles"] == (0 if shift == 6 else ts["grid"] * (ts["block"] // 64))


@pytest.mark.parametrize("block", [384, 1024])
def test_tile_costs_by_workgroup_shape(gpu_ctx, oracle, monkeypatch, block):
    monkeypatch.setenv("MORT_FAST_BLOCK_SIZE", str(block))
    world, cam, refs = _bvh_refs(oracle)
    for ts in _two_frames(gpu_ctx, oracle, world, cam, refs, f"mega_bvh_kernel<{block},"):
        assert ts["block"] == block and ts["grid"] == -(-ts["tiles"] * 64 // block) and ts["head"] is None


# ---------------------------------------------------------------- heavy waves

@pytest.mark.parametrize("heavy", [None, "3,2,12,50", "1,1,4,100"], ids=lambda h: "default" if h is None else h)
@pytest.mark.parametrize("key", ["s8", "flat"])
def test_heavy_wave_head(gpu_ctx, oracle, monkeypatch, capfd, key, heavy):
    """The head of both frames is tile_ref.heavy_head of the launch's keys and of the segment total of the frame the keys came from (the
    one-sample frame on frame 1, frame 1 on frame 2), which the saved counters hold; and it is not empty."""
    monkeypatch.setenv("MORT_GEN_MIN_PRIMS", "0")
    monkeypatch.setenv("MORT_GEN_HEAVY_DEBUG", "1")
    if heavy is not None:
        monkeypatch.setenv("MORT_GEN_HEAVY", heavy)
    shape = tuple(int(v) for v in (heavy or "3,2,12,50").split(","))
    world, cam = _sched_scene(key)
    refs = _oracle_frames(oracle, key, world, cam, _sched_refs(oracle, key))
    capfd.readouterr()
    states = _two_frames(gpu_ctx, oracle, world, cam, refs, "mega_gen_kernel<1024,")
    printed = [int(m.group(1)) for m in _HEAVY_LINE.finditer(capfd.readouterr().err)]
    for f, (ts, came_from) in enumerate(zip(states, (refs["rp"], refs["r1"]))):
        assert ts["heavy"] == shape and ts["head"] is not None, ts["heavy"]
        total = T.counters_total(ts["frame_total"])
        assert total == came_from["segments"] == int(came_from["segments_px"].sum()), f"frame {f + 1}: saved segment total"
        want = T.heavy_head(ts["keys"], shape[3], ts["tiles"] // 2 or 1, total, ts["grid"] * ts["block"])
        assert ts["head"] == want, f"frame {f + 1}: head {ts['head']}, the rule gives {want}"
        assert ts["head"] > 0, f"frame {f + 1}"
    assert printed == [states[0]["head"], states[1]["head"]]


# ---------------------------------------------------------------- the cost-key cache

def test_cost_key_cache(gpu_ctx, oracle):
    """A launch probes when the costs it holds are of another (world, image, partition, view) and only then."""
    world, cam = _bvh_scene()
    W, H = cam.image_width, cam.image_height
    ctx = gpu_ctx

    def launch(c, want, what):
        ctx.render(c, want_accum=False)
        ts = ctx.tile_state()
        assert ts["ordered"] == 1, what
        assert ts["probed"] == want, what

    try:
        ctx.set_partition(0, 1, 8)
        ctx.upload_world(world)
        ctx.rng_seed(S.DEFAULT_SEED, W, H)
        launch(cam, 1, "first frame")
        launch(cam, 0, "second frame")
        launch(cam, 0, "third frame, same view")
        launch(_bvh_scene(spp=9)[1], 0, "sqrt_spp alone")
        ctx.rng_seed(S.DEFAULT_SEED + 1, W, H)
        launch(cam, 0, "seed alone")
        moved = _bvh_scene()[1]
        set_view(moved, (12.0, 2.0, 3.0), (0.0, 0.0, 0.0))
        launch(moved, 1, "moved camera")
        launch(moved, 0, "moved camera, second frame")
        launch(cam, 1, "back to the first view: one key is kept, not a table")
        launch(_bvh_scene(depth=7)[1], 1, "bounce limit")
        launch(cam, 1, "bounce limit back")
        ctx.upload_world(world)
        launch(cam, 1, "upload_world of the same world")
        launch(cam, 0, "frame after it")
        ctx.set_partition(0, 2, 8)
        ctx.rng_seed(S.DEFAULT_SEED, W, H)
        launch(cam, 1, "partition")
        ctx.set_partition(0, 1, 8)
        ctx.rng_seed(S.DEFAULT_SEED, W, H)
        launch(cam, 1, "partition back")
        launch(cam, 0, "frame after it")
        other = _bvh_scene(188, 105)[1]  # the same 336 tiles: no buffer grows, the key alone tells the sizes apart
        ctx.rng_seed(S.DEFAULT_SEED, 188, 105)
        launch(other, 1, "image size")
    finally:
        ctx.set_partition(0, 1, 8)


# ---------------------------------------------------------------- launches that do not order

def test_launches_that_do_not_order(gpu_ctx, oracle, monkeypatch):
    world, cam = _bvh_scene()
    W, H = cam.image_width, cam.image_height
    ctx = gpu_ctx
    ctx.set_partition(0, 1, 8)
    ctx.upload_world(world)
    ctx.rng_seed(S.DEFAULT_SEED, W, H)
    ctx.render(cam, want_accum=False)
    assert ctx.tile_state()["ordered"] == 1  # the frame orders when nothing forbids it
    ctx.render(cam, mode=hip.MODE_THROUGHPUT, want_accum=False)
    ts = ctx.tile_state()
    assert (ts["ordered"], ts["probed"]) == (0, 0) and ts["keys"] is None and ts["tiles"] == 24 * ((H * cam.sqrt_spp + 7) // 8)
    ctx.render(cam, mode=hip.MODE_WAVE, want_accum=False)  # the wavefront pipeline has no tile order
    ts = ctx.tile_state()
    assert (ts["ordered"], ts["probed"], ts["grid"]) == (0, 0, 0)
    monkeypatch.setenv("MORT_NO_TILE_ORDER", "1")
    ctx.render(cam, want_accum=False)
    ts = ctx.tile_state()
    assert (ts["ordered"], ts["probed"]) == (0, 0) and ts["tiles"] == 336 and ts["grid"] > 0
    monkeypatch.delenv("MORT_NO_TILE_ORDER")
    ctx.render(cam, want_accum=False)
    assert ctx.tile_state()["ordered"] == 1
    # 200 x 112: 25 x 14 = 350 tiles on 256-thread workgroups of four waves, one tile per wave: grid = ceil(350 / 4) = 88 (far below the
    # device's CU count, which caps it otherwise), and 350 < 4 * 88 = 352
    world, cam = _bvh_scene(200, 112)
    ctx.upload_world(world)
    ctx.rng_seed(S.DEFAULT_SEED, 200, 112)
    out = ctx.render(cam, want_accum=False)
    ts = ctx.tile_state()
    assert out["stats"]["kernel_name"].startswith("mega_bvh_kernel<256,")
    assert (ts["tiles"], ts["grid"], ts["block"]) == (350, 88, 256) and ts["tiles"] < 4 * ts["grid"]
    assert (ts["ordered"], ts["probed"]) == (0, 0) and ts["cost"] is None
