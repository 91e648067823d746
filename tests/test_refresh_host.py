"""Volume refresh on the host (mort_hip_volume_refresh_host, dev_refresh.h): both host traversals against the
reference of tests/refresh_ref.py -- tests/cached_ref.walk over the oracle, the bake's projection and the blend restated in numpy
-- at tolerance 0: records as raw 32-bit words (any NaN equals any NaN), all 48 bytes of every stream, the counts.  The census of
the inputs, the identities the contract promises, the fixed point, and the rotated direction sets.  No GPU."""
import math

import numpy as np
import pytest

from mort_amd import hip
from tests import cached_ref as CR
from tests import oracle_lib as O
from tests import probe_ref as PR
from tests import query_rays as Q
from tests import refresh_ref as RR
from tests import volume_ref as V
from tests import worlds as Wd

F = np.float32
TREES = [False, True]


def _refresh(ref, tree, fill=RR.FILL, want_ends=True, dirs="ref", records_in=None, streams=None):
    """the host form on the reference's inputs, the outputs pre-filled; (records, streams, ends)"""
    streams = ref.streams0.copy() if streams is None else streams
    rec, ends = RR.filled(ref.grid.probes, fill)
    got = hip.volume_refresh_host(ref.world, ref.params, streams, ref.records_in if records_in is None else records_in, ref.depth, records_out=rec,
                                  ends=ends if want_ends else None, dirs=ref.dirs if dirs == "ref" else dirs, m=ref.m, tree=tree, nthreads=4)
    assert got["records"] is rec
    return rec, streams, (ends if want_ends else None)


# ------------------------------------------------------------------------------------------------------------------- census

@pytest.mark.parametrize("name", RR.WORLDS)
def test_inputs_show_something(name):
    """The census of the inputs, on the reference alone, D = 64, samples 1, bounce limit 4.  Measured (scene 6 / scene 1 / the flat
    world): share of the paths ending in the volume at K = 0 under "ones" 22.9 / 64.9 / 14.5 %, at K = 1 (bounce limit 8 on scene 6)
    14.4 / 40.2 / 7.6 %, every probe with at least one such path; Lambertian hits that fall through under "slab" at K = 0 with the
    visible sampler 171 / 666 / 63 over the rays of every probe of the grid (the figure is of the volume and the rays: in the refresh
    itself the slab's own 12 probes are copied and run nothing, which leaves 67 / 77 / 2 of those hits); directions with a NaN colour under "poison" 184 / 229 / 161."""
    P, D = 24, 64
    for K, limit, least in ((0, RR.LIMIT, 0.10), (1, 8 if name == "scene6" else RR.LIMIT, 0.05)):
        r = RR.reference(name, K, limit=limit)
        ended = r.census["ends"]
        share = float(ended.sum()) / (P * D)
        print(name, "K", K, "share of the paths that end in the volume", round(share, 3))
        assert share >= least, (K, share)
        assert (ended.sum(1) >= 1).all() and len(ended) == P, (K, ended.sum(1))
        assert (r.ends == ended.sum(1)).all()
    fell = RR.census_of_the_rays(name, 0, "slab", True)["fell_through"]
    run = RR.reference(name, 0, mask="slab", visible=True).census["walk"]["fell_through"]
    print(name, "fall through under slab over every probe's rays", fell, "of them in the refresh, where half the probes are copied", run)
    assert fell >= 50, fell
    assert run >= 1, run
    r = RR.reference(name, 0, mask="poison")
    nan = np.isnan(r.census["s"]).any(2)
    print(name, "NaN directions under poison", int(nan.sum()), "over", int(nan.any(1).sum()), "probes")
    assert nan.sum() >= 100, nan.sum()
    for mask in ("holes", "slab", "fractional"):
        copied = len(RR.reference(name, 0, mask=mask).census["masked"])
        print(name, mask, "probes that take the copy rule", copied)
        assert 8 <= copied <= 16, (mask, copied)


def test_positions_are_the_grids():
    for name in RR.WORLDS:
        g = CR.grid_of(name)
        assert RR.positions(g).tobytes() == hip.volume_probes(g).tobytes()


# ---------------------------------------------------------------------------------------------------------- bit for bit

@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("h", [0.0, 0.75])
@pytest.mark.parametrize("K", [0, 1])
@pytest.mark.parametrize("mask", RR.MASKS)
@pytest.mark.parametrize("name", RR.WORLDS)
def test_equals_the_reference(name, mask, K, h, samples, visible, tree):
    ref = RR.reference(name, K, h, samples, mask, visible)
    rec, streams, ends = _refresh(ref, tree)
    RR.assert_equal(rec, streams, ends, ref, f"{name} {mask} K={K} h={h} samples={samples} visible={visible} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("D", [64, 128, 320])
@pytest.mark.parametrize("name", RR.WORLDS)
def test_direction_counts(name, D, tree):
    """320 directions are five batches: a wave of the kernel takes more than one, and their number is odd"""
    ref = RR.reference(name, 0, 0.75, 1, "fractional", True, D=D)
    rec, streams, ends = _refresh(ref, tree)
    RR.assert_equal(rec, streams, ends, ref, f"{name} D={D} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("sel", RR.SELECTIONS[1:])
@pytest.mark.parametrize("name", RR.WORLDS)
def test_selections(name, sel, tree):
    """a partial refresh: the unselected records and counts keep their fill, the unselected streams all 48 bytes"""
    ref = RR.reference(name, 1, 0.75, 1, "fractional", False, sel=sel)
    rec, streams, ends = _refresh(ref, tree)
    RR.assert_equal(rec, streams, ends, ref, f"{name} selection {sel} tree={tree}")
    others = np.setdiff1d(np.arange(24), RR.selected(*sel))
    assert (rec.view(np.uint8).reshape(24, 128)[others] == RR.FILL).all()
    assert (ends.view(np.uint8).reshape(24, 4)[others] == RR.FILL).all()
    a, b = streams.view(np.uint8).reshape(24, -1), ref.streams0.view(np.uint8).reshape(24, -1)
    assert (a[others] == b[others]).all()


@pytest.mark.parametrize("tree", TREES)
def test_without_the_counts(tree):
    ref = RR.reference("scene6", 1, 0.75, 3, "fractional", True)
    rec, streams, ends = _refresh(ref, tree, want_ends=False)
    assert ends is None
    RR.assert_equal(rec, streams, None, ref, f"no counts tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("kind", ["plain", "nan"])
@pytest.mark.parametrize("name", RR.WORLDS)
def test_a_callers_direction_set(name, kind, tree):
    """axis-parallel, zero-length, unnormalised and NaN directions, used as given"""
    ref = RR.reference(name, 0, 0.75, 1, "ones", False, dirs=kind)
    rec, streams, ends = _refresh(ref, tree)
    RR.assert_equal(rec, streams, ends, ref, f"{name} own directions {kind} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
def test_null_directions_are_the_librarys(tree):
    ref = RR.reference("scene6", 0, 0.75, 1, "fractional", False)
    rec, streams, ends = _refresh(ref, tree, dirs=None)
    RR.assert_equal(rec, streams, ends, ref, f"dirs=NULL tree={tree}")


# ---------------------------------------------------------------------------------------------------------- the identities

@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("name", RR.WORLDS)
def test_bootstrap_is_a_bake(name, samples, tree):
    """(a): h = 0, K >= bounce_limit, records_in = pack(zeros, weight > 0): the records are volume_pack of probe_bake over
    volume_probes(grid), the streams the bake's"""
    g = CR.grid_of(name)
    P, D = g.probes, 64
    path = RR.path_of(name, samples)
    weight = np.random.default_rng(5).uniform(0.1, 2.0, size=P).astype(F)
    zeros = hip.volume_pack_host(np.zeros((P, 27), dtype=F), weight)["records"]
    st_bake = RR.streams_of(P, D)
    sh = hip.probe_bake_host(Q.build(name).world, hip.PROBE_PARAMS(path, D), hip.volume_probes(g), st_bake, tree=tree, nthreads=4)["sh"]
    want = hip.volume_pack_host(sh, weight)["records"]
    for K in (RR.LIMIT, RR.LIMIT + 3):
        for visible in (False, True):
            _, _, depth, vis = CR.volume(name, "ones")
            params = RR.params_of(path, K, g, vis if visible else None, D, 0.0, (0, 1, P))
            st = RR.streams_of(P, D)
            got = hip.volume_refresh_host(Q.build(name).world, params, st, zeros, depth if visible else None, tree=tree, nthreads=4)
            assert (Q._words(got["records"]) == Q._words(want)).all(), (K, visible)
            assert st.tobytes() == st_bake.tobytes(), (K, visible)
            assert not got["ends"].any()


@pytest.mark.parametrize("tree", TREES)
def test_unselected_bytes_do_not_matter(tree):
    """(b): two fills of records_out give the same selected records"""
    ref = RR.reference("scene1", 1, 0.75, 1, "fractional", False, sel=(1, 5, 5))
    a, _, _ = _refresh(ref, tree, fill=0x00)
    b, _, _ = _refresh(ref, tree, fill=0xff)
    sel = RR.selected(*ref.sel)
    assert a[sel].tobytes() == b[sel].tobytes() == ref.records[sel].tobytes()


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("D", [64, 256])
def test_fixed_point_of_a_white_world(D, tree):
    """(c): K = 0, h = 0, every record the constant radiance b (band 0 = 4 pi c0 b = sqrt(4 pi) b, bands 1-2 zero), a probe that
    sees the background b and one white Lambertian sphere: the surface returns (1 * E) / pi = b, so every direction returns b and
    the record stays, within the set's quadrature error sqrt(4 pi) b |G_0k - delta_0k| (G the restated set's Gram matrix, as
    tests/test_probe_host.py derives it) plus 1e-5 relative for the fp32 sums.  (The issue writes the band-0 value as
    "sqrt(4 pi) b c0", which is b; the coefficient of a constant radiance b is 4 pi c0 b.)"""
    b = np.array([0.25, 0.5, 2.0], dtype=F)
    world, _ = Wd.flat_world([("sphere", (0, 0, -1), 0.5, ("lamb", (1.0, 1.0, 1.0)))])
    path = hip.RADIANCE_PARAMS(4, 1, (C_float3(b)), -1, 0)
    g = hip.VOLUME_GRID((-1.5, -1.0, -2.5), (1.0, 1.0, 1.0), (4, 3, 2), 0.0)
    band0 = (F(4.0 * math.pi) * PR.C0 * b).astype(F)
    sh = np.zeros((g.probes, 9, 3), dtype=F)
    sh[:, 0] = band0
    rec_in = V.pack(sh.reshape(g.probes, 27))
    params = RR.params_of(path, 0, g, None, D, 0.0, (0, 1, g.probes))
    st = RR.streams_of(g.probes, D)
    got = hip.volume_refresh_host(world, params, st, rec_in, tree=tree, nthreads=4)
    assert got["ends"].sum() > 0, "no probe sees the sphere"
    Y = PR.basis64(PR.fibonacci(D))
    G = (4.0 * math.pi / D) * (Y.T @ Y)
    new = got["records"][:, :27].reshape(g.probes, 9, 3).astype(np.float64)
    scale = math.sqrt(4.0 * math.pi) * b.astype(np.float64)
    for k in range(9):
        bound = scale * (abs(G[0, k] - (1.0 if k == 0 else 0.0)) + 1e-5)
        want = band0.astype(np.float64) if k == 0 else 0.0
        err = np.abs(new[:, k] - want).max(0)
        print("D", D, "band", k, "error", err, "bound", bound)
        assert (err <= bound).all(), (k, err, bound)


def C_float3(v):
    import ctypes
    return (ctypes.c_float * 3)(*[float(x) for x in v])


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("name", RR.WORLDS)
def test_two_rounds_chained(name, tree):
    """round 1 (the library's set) into a second buffer, round 2 (the rotated set) back into the first, the streams carried on:
    the reference chained the same way"""
    g, rec0, depth, vis = CR.volume(name, "fractional")
    P, D, h, K = g.probes, 64, 0.75, 0
    path = RR.path_of(name)
    params = RR.params_of(path, K, g, vis, D, h, (0, 1, P))
    world = Q.build(name).world
    sets = [hip.probe_directions_round(D, r) for r in (1, 2)]
    want = [rec0.copy(), np.zeros((P, 32), dtype=F)]
    want_st, want_ends = RR.streams_of(P, D), np.zeros(P, dtype=np.uint32)
    got = [rec0.copy(), np.zeros((P, 32), dtype=F)]
    got_st, got_ends = RR.streams_of(P, D), np.zeros(P, dtype=np.uint32)
    for r in range(2):
        RR.refresh(world, path, K, g, want[r % 2], depth, vis, sets[r], h, (0, 1, P), want_st, want[1 - r % 2], want_ends)
        hip.volume_refresh_host(world, params, got_st, got[r % 2], depth, records_out=got[1 - r % 2], ends=got_ends, dirs=sets[r], tree=tree,
                                nthreads=4)
        assert (Q._words(got[1 - r % 2]) == Q._words(want[1 - r % 2])).all(), r
        assert got_st.tobytes() == want_st.tobytes() and (got_ends == want_ends).all(), r
    assert (Q._words(got[0]) != Q._words(rec0)).any()


# ------------------------------------------------------------------------------------------------------ the rotated sets

def test_round_zero_is_the_librarys_set():
    for D in (64, 256, 4096):
        assert hip.probe_directions_round(D, 0).tobytes() == hip.probe_directions(D).tobytes()


@pytest.mark.parametrize("r", [1, 2, 63, 64, 65])
@pytest.mark.parametrize("D", [64, 320])
def test_rotated_sets(D, r):
    got = hip.probe_directions_round(D, r)
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max() <= 2.0 ** -22
    want = RR.directions_round(D, r)
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -23
    assert (got != hip.probe_directions(D)).any(1).sum() >= D - 2, "a rotation keeps at most its two poles"
    for other in (1, 2, 63, 64, 65):
        if other != r:
            assert (got != hip.probe_directions_round(D, other)).any()


def test_rotated_sets_refuse_what_the_set_refuses():
    out = np.zeros((64, 3), dtype=F)
    L = hip.lib()
    for bad in (0, 63, 65, 4160, -64):
        assert L.mort_hip_probe_directions_round(bad, 1, out.ctypes.data) == -1
    assert L.mort_hip_probe_directions_round(64, 1, None) == -1
