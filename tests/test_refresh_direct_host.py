"""Direct-light volume refresh on the host (mort_hip_volume_refresh_direct_host, dev_refresh_direct.h): both host
traversals against the reference of tests/refresh_direct_ref.py -- cached_direct_ref's walk restated with rule E over the oracle, the
bake's projection and the blend in numpy -- at tolerance 0: records as raw 32-bit words (any NaN equals any NaN), all 48 bytes of
every stream, both counts.  The census of the inputs, the identities (A)-(E) of include/mort_hip.h, and the estimator against the
indirect bake on independent seeds, which is not the contract.  No GPU."""
import numpy as np
import pytest

from mort_amd import hip
from tests import oracle_lib as O
from tests import probe_ref as PR
from tests import query_rays as Q
from tests import refresh_direct_ref as XR
from tests import refresh_ref as RR
from tests import volume_ref as V
from tests import worlds as Wd

F = np.float32
TREES = [False, True]


def _refresh(ref, tree, fill=XR.FILL, want_ends=True, want_lit=True, dirs="ref", streams=None):
    """the host form on the reference's inputs, the outputs pre-filled; (records, streams, ends, lit)"""
    streams = ref.streams0.copy() if streams is None else streams
    rec, ends, lit = XR.filled(ref.grid.probes, fill)
    got = hip.volume_refresh_direct_host(ref.world, ref.params, streams, ref.records_in, ref.depth, records_out=rec, ends=ends if want_ends else None,
                                         lit=lit if want_lit else None, dirs=ref.dirs if dirs == "ref" else dirs, m=ref.m, tree=tree, nthreads=4)
    assert got["records"] is rec
    return rec, streams, (ends if want_ends else None), (lit if want_lit else None)


# ------------------------------------------------------------------------------------------------------------------- census

@pytest.mark.parametrize("name", XR.LIT_WORLDS)
def test_inputs_show_something(name):
    """The census of the near-light grids on the reference alone, D = 64, one path, bounce limit 4, K = 0, mask "ones".  Counted
    (scene 6 / the flat world / the BVH light world): primary rays on an emitter 27 / 97 / 38, paths that end in the volume
    607 / 392 / 367, lit 173 / 317 / 281, shadow segments that end in a medium 51 in the flat world, rule-E rays with zero emission
    64 in the BVH light world (the probe inside a sphere light).  The thresholds are conditions, set below the counts."""
    r = XR.reference(name, 0)
    w = r.census["walk"]
    emits, dark = int(w["rule_e_emits"].sum()), int((w["rule_e"] & ~w["rule_e_emits"]).sum())
    ended, lit = int(r.census["ends"].sum()), int(r.census["lit"].sum())
    print(name, "rule E with emission", emits, "without", dark, "ended", ended, "lit", lit, "shadow segments in a medium", w["shadow_on_medium"])
    assert emits >= 20 and ended >= 300 and lit >= 150
    assert (r.census["lit"] <= r.census["ends"]).all()
    if name == XR.BVH_LIGHT_WORLD:
        assert dark >= 60
    if name.startswith("flat:"):
        assert w["shadow_on_medium"] >= 30
    for mask in XR.MASKS:
        m = XR.reference(name, 0, mask=mask)
        assert len(m.census["active"]) >= 1 and (m.census["lit"].sum(1) >= 1).any(), mask
        assert (m.lit[m.census["masked"]] == 0).all() and (m.ends[m.census["masked"]] == 0).all()


def test_the_matrix_meets_rule_a():
    """K = 1 at bounce limit 4 leaves rule (a) to the paths that end at iteration 3, and scene 1 has no light object: over the matrix
    at least 100 terminal hits take the rule (counted at K = 1: 125 / 6 / 3 in the lit worlds)"""
    total = 0
    for name in XR.WORLDS:
        for K in (0, 1):
            total += XR.reference(name, K).census["walk"]["rule_a"]
    print("terminal hits under rule (a)", total)
    assert total >= 100


def test_positions_are_the_grids():
    for name in XR.WORLDS:
        g = XR.grid_of(name)
        assert RR.positions(g).tobytes() == hip.volume_probes(g).tobytes()


# ---------------------------------------------------------------------------------------------------------- bit for bit

@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("h", [0.0, 0.75])
@pytest.mark.parametrize("K", [0, 1])
@pytest.mark.parametrize("mask", XR.MASKS)
@pytest.mark.parametrize("name", XR.WORLDS)
def test_equals_the_reference(name, mask, K, h, samples, visible, tree):
    ref = XR.reference(name, K, h, samples, mask, visible)
    rec, streams, ends, lit = _refresh(ref, tree)
    XR.assert_equal(rec, streams, ends, lit, ref, f"{name} {mask} K={K} h={h} samples={samples} visible={visible} tree={tree}")
    live = ref.census["active"]
    assert (lit[live] <= ends[live]).all() and (ends[live] <= 64 * samples).all()


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("D", [64, 128, 320])
@pytest.mark.parametrize("name", XR.WORLDS)
def test_direction_counts(name, D, tree):
    """320 directions are five batches: a wave of the kernel takes more than one, and their number is odd"""
    ref = XR.reference(name, 0, 0.75, 1, "fractional", True, D=D)
    rec, streams, ends, lit = _refresh(ref, tree)
    XR.assert_equal(rec, streams, ends, lit, ref, f"{name} D={D} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("which", [1, 2, 3])
@pytest.mark.parametrize("name", XR.WORLDS)
def test_selections(name, which, tree):
    """a partial refresh: the unselected records and counts keep their fill, the unselected streams all 48 bytes"""
    P = XR.grid_of(name).probes
    sel = XR.selections(P)[which]
    ref = XR.reference(name, 1, 0.75, 1, "fractional", False, sel=sel)
    rec, streams, ends, lit = _refresh(ref, tree)
    XR.assert_equal(rec, streams, ends, lit, ref, f"{name} selection {sel} tree={tree}")
    others = np.setdiff1d(np.arange(P), RR.selected(*sel))
    assert (rec.view(np.uint8).reshape(P, 128)[others] == XR.FILL).all()
    assert (ends.view(np.uint8).reshape(P, 4)[others] == XR.FILL).all()
    assert (lit.view(np.uint8).reshape(P, 4)[others] == XR.FILL).all()
    a, b = streams.view(np.uint8).reshape(P, -1), ref.streams0.view(np.uint8).reshape(P, -1)
    assert (a[others] == b[others]).all()


@pytest.mark.parametrize("tree", TREES)
def test_without_the_counts(tree):
    """ends_out = NULL, lit_out = NULL and both change nothing else"""
    ref = XR.reference("scene6", 1, 0.75, 3, "fractional", True)
    for want_ends, want_lit in ((True, False), (False, True), (False, False)):
        rec, streams, ends, lit = _refresh(ref, tree, want_ends=want_ends, want_lit=want_lit)
        assert (ends is None) == (not want_ends) and (lit is None) == (not want_lit)
        XR.assert_equal(rec, streams, ends, lit, ref, f"ends={want_ends} lit={want_lit} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("kind", ["plain", "nan"])
@pytest.mark.parametrize("name", XR.WORLDS)
def test_a_callers_direction_set(name, kind, tree):
    """axis-parallel, zero-length, unnormalised and NaN directions, used as given"""
    ref = XR.reference(name, 0, 0.75, 1, "ones", False, dirs=kind)
    rec, streams, ends, lit = _refresh(ref, tree)
    XR.assert_equal(rec, streams, ends, lit, ref, f"{name} own directions {kind} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
def test_null_directions_are_the_librarys(tree):
    ref = XR.reference("scene6", 0, 0.75, 1, "fractional", False)
    rec, streams, ends, lit = _refresh(ref, tree, dirs=None)
    XR.assert_equal(rec, streams, ends, lit, ref, f"dirs=NULL tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("name", XR.WORLDS)
def test_two_rounds_chained(name, tree):
    """round 1 into a second buffer, round 2 (another rotated set) back into the first, the streams carried on: the reference
    chained the same way"""
    g, rec0, depth, vis = XR.volume(name, "fractional")
    P, D, h, K = g.probes, 64, 0.75, 0
    path = XR.path_of(name)
    params = XR.params_of(path, K, g, vis, D, h, (0, 1, P))
    world = Q.build(name).world
    sets = [hip.probe_directions_round(D, r) for r in (1, 2)]
    want = [rec0.copy(), np.zeros((P, 32), dtype=F)]
    want_st, want_ends, want_lit = XR.streams_of(P, D), np.zeros(P, dtype=np.uint32), np.zeros(P, dtype=np.uint32)
    got = [rec0.copy(), np.zeros((P, 32), dtype=F)]
    got_st, got_ends, got_lit = XR.streams_of(P, D), np.zeros(P, dtype=np.uint32), np.zeros(P, dtype=np.uint32)
    for r in range(2):
        XR.refresh(world, path, K, g, want[r % 2], depth, vis, sets[r], h, (0, 1, P), want_st, want[1 - r % 2], want_ends, want_lit)
        hip.volume_refresh_direct_host(world, params, got_st, got[r % 2], depth, records_out=got[1 - r % 2], ends=got_ends, lit=got_lit,
                                       dirs=sets[r], tree=tree, nthreads=4)
        assert (Q._words(got[1 - r % 2]) == Q._words(want[1 - r % 2])).all(), r
        assert got_st.tobytes() == want_st.tobytes() and (got_ends == want_ends).all() and (got_lit == want_lit).all(), r
    assert (Q._words(got[0]) != Q._words(rec0)).any()


# ---------------------------------------------------------------------------------------------------------- the identities

@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("visible", [False, True])
@pytest.mark.parametrize("K", [0, 1])
def test_a_world_without_emitters_is_the_plain_refresh(K, visible, tree):
    """(A) on scene 1: no emitter, no light object"""
    ref = XR.reference("scene1", K, 0.75, 3, "fractional", visible)
    assert ref.params.cached.path.light_obj_type == -1 and not ref.census["walk"]["rule_e"].any()
    rec, streams, ends, lit = _refresh(ref, tree)
    st = ref.streams0.copy()
    prec, pends = RR.filled(ref.grid.probes)
    hip.volume_refresh_host(ref.world, ref.params, st, ref.records_in, ref.depth, records_out=prec, ends=pends, dirs=ref.dirs, tree=tree, nthreads=4)
    assert (Q._words(rec) == Q._words(prec)).all() and streams.tobytes() == st.tobytes() and (ends == pends).all()
    assert ends.sum() > 100 and not lit.any()


@pytest.mark.parametrize("tree", TREES)
def test_without_a_light_object_and_no_emitter_in_sight_it_is_the_plain_refresh(tree):
    """(A) on a lit world: the probes of scene 6's near grid whose primary rays meet no emitter along a caller's set that looks
    down, called without the light object"""
    name = "scene6"
    g, rec_in, depth, vis = XR.volume(name, "fractional")
    P, D = g.probes, 64
    dirs = PR.fibonacci(D).copy()
    dirs[:, 1] = -np.abs(dirs[:, 1])  # the light is above every probe
    path = XR.path_of(name, 3, light=False)
    world = Q.build(name).world
    want_st = XR.streams_of(P, D)
    wrec, wends, wlit = XR.filled(P)
    cen = XR.refresh(world, path, 0, g, rec_in, None, None, dirs, 0.75, (0, 1, P), want_st, wrec, wends, wlit)
    assert not cen["walk"]["rule_e_emits"].any() and cen["ends"].sum() > 100
    params = XR.params_of(path, 0, g, None, D, 0.75, (0, 1, P))
    a_st, b_st = XR.streams_of(P, D), XR.streams_of(P, D)
    a = hip.volume_refresh_direct_host(world, params, a_st, rec_in, dirs=dirs, tree=tree, nthreads=4)
    b = hip.volume_refresh_host(world, params, b_st, rec_in, dirs=dirs, tree=tree, nthreads=4)
    assert (Q._words(a["records"]) == Q._words(b["records"])).all() and a_st.tobytes() == b_st.tobytes() and (a["ends"] == b["ends"]).all()
    assert (Q._words(a["records"]) == Q._words(wrec)).all() and not a["lit"].any()


def _black_limit_one(path):
    p = hip.RADIANCE_PARAMS.from_buffer_copy(path)
    p.bounce_limit, p.samples = 1, 1
    for k in range(3):
        p.background[k] = 0.0
    return p


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("K", [0, 1])
@pytest.mark.parametrize("name", XR.LIT_WORLDS)
def test_composed_from_the_existing_calls(name, K, samples, tree):
    """(B): per path the mask "the primary hit emits" from query_radiance_host at bounce limit 1 and a black background on a copy
    of the streams as they stand, the value from query_radiance_cached_direct_host at one sample on the carried streams; the
    sum of where(mask, 0, value), the projection and the blend give the records to the bit, and the streams and counts too.
    A primary hit that ends the path with a colour of zero is 0 either way."""
    ref = XR.reference(name, K, 0.75, samples, "fractional", True)
    g, D = ref.grid, 64
    live = ref.census["active"]
    rays = PR.rays_of(RR.positions(g)[live], ref.dirs)
    idx = (live[:, None] * D + np.arange(D)[None, :]).reshape(-1)
    st = np.ascontiguousarray(ref.streams0[idx]).copy()
    one = hip.CACHED_PARAMS.from_buffer_copy(ref.params.cached)
    one.path.samples = 1
    total = np.zeros((len(rays), 3), dtype=F)
    ends = np.zeros(len(rays), dtype=np.uint32)
    lit = np.zeros(len(rays), dtype=np.uint32)
    dropped = 0
    for _ in range(samples):
        emits = (hip.query_radiance_host(ref.world, _black_limit_one(ref.path), rays, st.copy(), tree=tree, nthreads=4)["rgb"] != 0).any(1)
        got = hip.query_radiance_cached_direct_host(ref.world, one, rays, st, ref.records_in, ref.depth, tree=tree, nthreads=4)
        with np.errstate(invalid="ignore", over="ignore"):
            total = (total + np.where(emits[:, None], F(0), got["rgb"])).astype(F)
        ends += got["ends"]; lit += got["lit"]
        dropped += int(emits.sum())
    assert dropped >= 10, "no primary ray meets an emitter"
    new = PR.project(total.reshape(len(live), D, 3), ref.dirs, samples).reshape(len(live), 27)
    want = RR.blend(ref.records_in[live, :27], new, 0.75)
    rec, streams, got_ends, got_lit = _refresh(ref, tree)
    assert (Q._words(rec[live, :27]) == Q._words(want)).all()
    assert np.ascontiguousarray(streams[idx]).tobytes() == st.tobytes()
    assert (got_ends[live] == ends.reshape(len(live), D).sum(1)).all() and (got_lit[live] == lit.reshape(len(live), D).sum(1)).all()


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("D", [64, 320])
def test_bootstrap_is_the_indirect_bake(D, tree):
    """(C): scene 6's near grid, one path, h = 0, K at the bounce limit, records_in = pack(zeros, weight 1).  No path ends in the
    volume, so a direction's value is the full bake's g_j with the emission e_j of a directly seen emitter taken out: the refresh
    sums Y_k (g_j - e_j) where the indirect bake subtracts the sum of Y_k e_j from the sum of Y_k g_j.  Each of the three is a
    balanced tree over 64 terms (6 additions) and D / 64 - 1 batch additions; with the products, the scale and the final subtraction
    the two results differ by at most (6 + D / 64 + 2) 2^-23 scale sum_j |Y_k(d_j)| (|g_j| + |e_j|) per coefficient, computed here
    in float64 from the reference's per-direction values.  The streams are the full bake's to the bit."""
    name = "scene6"
    g = XR.grid_of(name)
    P = g.probes
    world = Q.build(name).world
    path = XR.path_of(name, 1)
    zeros = V.pack(np.zeros((P, 27), dtype=F))
    assert (zeros[:, 27] == 1).all()
    st_bake = XR.streams_of(P, D)
    bake = hip.probe_bake_indirect_host(world, hip.PROBE_PARAMS(path, D), hip.volume_probes(g), st_bake, tree=tree, nthreads=4)
    st = XR.streams_of(P, D)
    got = hip.volume_refresh_direct_host(world, XR.params_of(path, XR.LIMIT, g, None, D, 0.0, (0, 1, P)), st, zeros, tree=tree, nthreads=4)
    assert st.tobytes() == st_bake.tobytes()
    assert not got["ends"].any() and not got["lit"].any()
    # |g_j| and |e_j| from the reference: the walk without the rule is the full bake's, its rule-E paths' colours are e_j
    dirs = PR.fibonacci(D)
    rays = PR.rays_of(RR.positions(g), dirs)
    full = hip.query_radiance_host(world, path, rays, XR.streams_of(P, D), tree=False, nthreads=4)["rgb"].astype(np.float64).reshape(P, D, 3)
    emit = hip.query_radiance_host(world, _black_limit_one(path), rays, XR.streams_of(P, D), tree=False, nthreads=4)["rgb"].astype(np.float64).reshape(P, D, 3)
    assert (emit != 0).any(2).sum() >= 20
    Y = np.abs(PR.basis(dirs).astype(np.float64))  # (D, 9)
    scale = float(PR.scale_of(D, 1))
    bound = (6 + D / 64 + 2) * 2.0 ** -23 * scale * np.einsum("dk,pdc->pkc", Y, np.abs(full) + np.abs(emit))
    err = np.abs(got["records"][:, :27].reshape(P, 9, 3).astype(np.float64) - bake["sh_ind"].astype(np.float64))
    print("D", D, "largest error over its bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    assert (got["records"][:, :27].reshape(P, 9, 3) != bake["sh_full"]).any(), "rule E changed nothing"


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("mask", ["fractional", "holes"])
def test_masked_probes_are_copied(mask, tree):
    """(D): the record bit for bit, no stream moved, both counts 0"""
    ref = XR.reference("flat:lit_by_quad_with_media", 0, 0.75, 1, mask, False)
    masked = ref.census["masked"]
    assert len(masked) >= 2
    rec, streams, ends, lit = _refresh(ref, tree)
    assert rec.view(np.uint32)[masked].tobytes() == ref.records_in.view(np.uint32)[masked].tobytes()
    a, b = streams.view(np.uint8).reshape(ref.grid.probes, -1), ref.streams0.view(np.uint8).reshape(ref.grid.probes, -1)
    assert (a[masked] == b[masked]).all() and not ends[masked].any() and not lit[masked].any()


@pytest.mark.parametrize("tree", TREES)
def test_unselected_bytes_do_not_matter(tree):
    """(E): two fills of records_out give the same selected records"""
    ref = XR.reference("scene6", 1, 0.75, 1, "fractional", False, sel=(1, 5, 3))
    a = _refresh(ref, tree, fill=0x00)[0]
    b = _refresh(ref, tree, fill=0xff)[0]
    sel = RR.selected(*ref.sel)
    assert a[sel].tobytes() == b[sel].tobytes() == ref.records[sel].tobytes()


# ------------------------------------------------------------------------------- against something that is not the contract

def _floor_under_a_light():
    world, ids = Wd.flat_world([("quad", (-5.0, 0.0, -5.0), (10.0, 0.0, 0.0), (0.0, 0.0, 10.0), ("lamb", (1.0, 1.0, 1.0))),
                                ("quad", (-0.5, 2.0, -0.5), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), ("light", (5.0, 3.0, 1.0)))])
    return world, ids[1]


def test_one_round_is_the_indirect_bake_at_two_bounces():
    """A white floor under a quad light, a black background, a 2 x 2 x 2 grid between them, a volume of zeros with weight 1, K = 0,
    h = 0, D = 1024, N = 4: one direct round estimates what the indirect bake at bounce limit 2 estimates -- the floor's reflected
    direct light, and nothing of the light seen directly.  16 seeds each, other seeds for the bake.  For coefficients 0 and 1, per
    channel, at two probes the means must agree within 4 standard errors of the difference, computed from the repeats; the test
    fails as vacuous if that allowance passes 5 % of the value."""
    world, light = _floor_under_a_light()
    g = hip.VOLUME_GRID((-0.6, 0.5, -0.6), (1.2, 0.8, 1.2), (2, 2, 2), 0.5)
    P, D, N, R = g.probes, 1024, 4, 16
    rp = hip.RADIANCE_PARAMS()
    rp.bounce_limit, rp.samples = 12, N
    rp.light_obj_type, rp.light_obj_idx = light
    zeros = V.pack(np.zeros((P, 27), dtype=F))
    params = XR.params_of(rp, 0, g, None, D, 0.0, (0, 1, P))
    bp = hip.RADIANCE_PARAMS.from_buffer_copy(rp)
    bp.bounce_limit = 2
    a, b = np.zeros((R, P, 9, 3)), np.zeros((R, P, 9, 3))
    for i in range(R):
        got = hip.volume_refresh_direct_host(world, params, O.seed_states(1000 + i, P * D, 1), zeros, tree=True, nthreads=4)
        assert (got["ends"] > 0).all() and (got["lit"] > 0).all()
        a[i] = got["records"][:, :27].reshape(P, 9, 3)
        b[i] = hip.probe_bake_indirect_host(world, hip.PROBE_PARAMS(bp, D), hip.volume_probes(g), O.seed_states(5000 + i, P * D, 1), tree=True,
                                            nthreads=4)["sh_ind"]
    for p in (0, 5):  # two probes of the lower layer, in opposite corners
        for k in (0, 1):
            for ch in range(3):
                x, y = a[:, p, k, ch], b[:, p, k, ch]
                allowed = 4.0 * np.sqrt(x.var(ddof=1) / R + y.var(ddof=1) / R)
                print(f"probe {p} coefficient {k} channel {ch}: refresh {x.mean():.5f} bake {y.mean():.5f} allowed {allowed:.5f} "
                      f"({allowed / abs(y.mean()):.2%})")
                assert allowed <= 0.05 * abs(y.mean()), "the allowance is too wide to show anything"
                assert abs(x.mean() - y.mean()) <= allowed, (p, k, ch, x.mean(), y.mean(), allowed)
