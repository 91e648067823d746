"""The catalogue of random worlds without a reference BVH (tests/worlds.py GEN_RANDOM) checked on the CPU, so that the GPU battery
over it (tests/test_gpu_gen_random.py) cannot pass vacuously: what the unified tree of every entry looks like
(mort_hip_debug_gen_tree, which reads the upload's own decision), which kernel family the host will pick for every camera, that the
entries reach both sides of the 48 KB rule for primitives in LDS, the depth cap, many chain ids, far-away origins and the giant
rule, that every camera sees solids, sky and paths that bounce, that every entry has a camera on each side of mnear, and that the
host's tree walk and item scan agree with the oracle on these worlds bit for bit."""
import numpy as np
import pytest

from mort_amd import hip
from tests import oracle_lib as O
from tests.feature_ref import oracle_features, MISS, SOLID
from tests.worlds import (GEN_RANDOM, GEN_FAMILIES, GEN_LIMIT_SIZES, GEN_CAPACITY_SIZES, GEN_SMALL_SIZES, GEN_FAR_VIEWS, GEN_INTERIOR_VIEWS,
                          GEN_MIN_PRIMS, GEN_TRANSLATES, gen_random_case, gen_random_camera, gen_random_prediction, gen_random_sizes,
                          gen_in_reach, gen_camera_lens, gen_has_tele)

NAMES = sorted(GEN_RANDOM)
F = np.float32


def test_catalogue_shape():
    """two seeds of every family at every size the battery asks for, named one by one; primitive counts, moving spheres and
    chains as the families state them"""
    for fam in GEN_FAMILIES:
        sizes = GEN_SMALL_SIZES + GEN_LIMIT_SIZES[fam] + (1000,) + ((GEN_CAPACITY_SIZES[fam],) if fam in GEN_CAPACITY_SIZES else ())
        assert set(GEN_CAPACITY_SIZES) == {"mixed", "quads"}
        for n in sizes:
            for seed in (0, 1):
                if fam == "ties" and n == 1:
                    assert f"{fam}_{n}_s{seed}" not in GEN_RANDOM     # a tie takes two
                else:
                    assert GEN_RANDOM[f"{fam}_{n}_s{seed}"] == (fam, n, seed)
        assert len(gen_random_sizes(fam)) == len(sizes) - (fam == "ties")
    assert len(GEN_RANDOM) == sum(2 * len(gen_random_sizes(f)) for f in GEN_FAMILIES)
    for name in NAMES:
        w, views, light, info = gen_random_case(name)
        fam, n, seed = GEN_RANDOM[name]
        o = w.c.objs
        t = hip.debug_gen_tree(w)
        assert not w.c.bvh_mode and o.num_bvh == 0
        assert t["tree"] and t["entries"] == n == info["n_spheres"] + info["n_quads"], name
        assert len(views) == 2 + (name in GEN_FAR_VIEWS) + gen_has_tele(name)
        assert o.num_hittable_list <= 2
        moving = info["moving"]
        if fam in ("mixed", "offset") and n >= 1000:
            ns = info["n_spheres"]
            assert 0.08 * ns <= moving <= 0.22 * ns, (name, moving, ns)      # 15 % of the spheres
        if fam in ("scales", "quads", "line"):
            assert moving == 0
        if fam == "ties" and n >= 150:
            assert moving >= 5
        if fam == "quads":
            assert info["n_spheres"] == 0 and o.num_spheres == 0
        if fam == "scales":
            assert info["n_quads"] == 0
            if n >= 150:
                r = np.array([s[2] for s in info["spheres"]])
                assert r.max() / r.min() >= 1e3 and np.log10(r.max() / r.min()) <= 4.0   # drawn over four decades
        if fam == "instances":
            boxes = 2 if n >= 30 else 1 if n >= 14 else 0
            assert o.num_translates <= GEN_TRANSLATES and o.num_rotate_y <= GEN_TRANSLATES
            assert t["chains"] == 1 + info["instances"] and info["instances"] >= min(n - 6 * boxes, 40) + boxes
            if n >= 150:
                assert o.num_translates == GEN_TRANSLATES and o.num_rotate_y == GEN_TRANSLATES and moving >= 3
        elif fam in ("mixed", "offset"):
            assert t["chains"] == 1 + (2 if n >= 30 else 1 if n >= 14 else 0)
        else:
            assert t["chains"] == 1
        assert (light is not None) == (fam == "mixed" and seed == 1 and n >= 5)


@pytest.mark.parametrize("name", NAMES)
def test_prediction(name):
    """the tree's invariants, and the kernel family of every camera: in reach and at least MORT_GEN_MIN_PRIMS entries gives
    mega_gen_kernel, anything else mega_kernel"""
    p = gen_random_prediction(name)
    t = p["tree"]
    assert t["tree"] and p["has_tree"]
    assert t["nodes"] <= 0x7fff and t["entries"] <= 0x2000 and t["depth"] <= 15 and 1 <= t["chains"] <= 128   # ids 0 .. 127
    assert t["image_max"] == 124 * 1024 and t["prims_lds_max"] == 48 * 1024
    assert t["lds_bytes"] <= t["image_max"] and t["fits"]
    assert p["prims_in_lds"] == (t["image_bytes"] + t["prim_bytes"] <= 48 * 1024)
    if p["prims_in_lds"]:                                    # the primitives follow the tables, each table aligned
        assert t["image_bytes"] + t["prim_bytes"] - 6 * 32 <= t["lds_bytes"] <= t["image_bytes"] + t["prim_bytes"] + 16
    else:
        assert t["lds_bytes"] == (t["image_bytes"] + 15) & ~15
    n = GEN_RANDOM[name][1]
    views = gen_random_case(name)[1]
    for k in range(len(views)):
        far_view = name in GEN_FAR_VIEWS and k == 2
        if views[k][0] == "tele":                            # four fifths of the reach away: the band widens a great deal
            assert k == len(views) - 1 and p["in_reach"][k] and not p["near"][k]
            cam = gen_random_camera(name, k)
            d = np.linalg.norm([cam.center.e[j] - t["centre"][j] for j in range(3)])
            assert d >= 0.75 * t["reach"] and F(2.0 ** -24) * d * d > 1.0
        assert p["in_reach"][k] == (not far_view), (name, k)
        assert p["kernel"][k] == ("mega_gen_kernel" if n >= GEN_MIN_PRIMS and not far_view else "mega_kernel")
    p0 = gen_random_prediction(name, min_prims=0)
    assert all(kn == ("mega_gen_kernel" if r else "mega_kernel") for kn, r in zip(p0["kernel"], p0["in_reach"]))


def test_catalogue_reaches_the_limits():
    """the census the GPU battery relies on"""
    P = {name: gen_random_prediction(name) for name in NAMES}
    T = {name: p["tree"] for name, p in P.items()}
    room = {n: t["prims_lds_max"] - (t["image_bytes"] + t["prim_bytes"]) for n, t in T.items()}
    assert sum(P[n]["prims_in_lds"] and 0 <= room[n] < 4096 for n in NAMES) >= 4
    assert sum(not P[n]["prims_in_lds"] and 0 < -room[n] < 8192 for n in NAMES) >= 4
    for fam, (below, above) in GEN_LIMIT_SIZES.items():
        assert all(P[f"{fam}_{below}_s{s}"]["prims_in_lds"] for s in (0, 1)), fam
        assert not any(P[f"{fam}_{above}_s{s}"]["prims_in_lds"] for s in (0, 1)), fam
    deep = [n for n in NAMES if T[n]["depth"] >= 14]
    assert len(deep) >= 3 and any(n.startswith("line_") for n in deep), deep
    assert any(T[n]["capped"] >= 1 for n in NAMES if n.startswith("line_")), "the depth cap never overrode the surface-area split"
    assert max(t["chains"] for t in T.values()) > 64
    amag = {n: float(np.abs(np.concatenate([P[n]["reach"]["lo"], P[n]["reach"]["hi"]])).max()) for n in NAMES}
    assert sum(a >= 1e4 for a in amag.values()) >= 2 and sum(a >= 5e5 for a in amag.values()) >= 2
    # the giant rule (scene_compile.h pad_prims): radius above half the extent of all centres; giants are left out of (G, R)
    some = every = 0
    for name in NAMES:
        if GEN_RANDOM[name][0] != "scales" or GEN_RANDOM[name][1] < 2:
            continue
        sph = gen_random_case(name)[3]["spheres"]
        c = np.array([s[0] for s in sph]); r = np.array([s[2] for s in sph])
        giant = r > 0.5 * np.linalg.norm(c.max(0) - c.min(0))
        half = 0.5 * np.linalg.norm(c.max(0) - c.min(0))
        if giant.all():
            every += 1
            assert T[name]["R"] >= half                      # nothing ordinary to centre on: all alike
        elif giant.any():
            some += 1
            rest = c[~giant]
            assert T[name]["R"] <= 0.5 * np.linalg.norm(rest.max(0) - rest.min(0)) * 1.001 + 2e-3 * (1 + np.abs(c).max() + r.max())
    assert some >= 1 and every >= 1, (some, every)
    print("largest LDS image of the catalogue:", max((t["lds_bytes"], n) for n, t in T.items()))
    assert max(t["lds_bytes"] for t in T.values()) < 124 * 1024


_seen = {}


def _what_the_camera_sees(name, k):
    if (name, k) not in _seen:
        w = gen_random_case(name)[0]
        cam = gen_random_camera(name, k)
        f = oracle_features(w, cam, nthreads=8)
        r = O.render(w, cam, nthreads=8, want_accum=False, want_segments=False)
        _seen[name, k] = (float((f["kind"] == SOLID).mean()), float((f["kind"] == MISS).mean()), r["segments"],
                          cam.image_width * cam.image_height * cam.sqrt_spp ** 2)
    return _seen[name, k]


@pytest.mark.parametrize("name", NAMES)
def test_cameras_see_solids_and_sky(name):
    """a condition on the catalogue, judged by the oracle alone: at least a fifth of every frame's pixels first meet a solid, and
    all views but those inside a sphere on purpose (GEN_INTERIOR_VIEWS) keep at least 5 % background"""
    n = GEN_RANDOM[name][1]
    for k in range(len(gen_random_case(name)[1])):
        solid, sky, _, _ = _what_the_camera_sees(name, k)
        assert solid >= 0.20, (name, k, solid)
        if (name, k) not in GEN_INTERIOR_VIEWS:
            assert sky >= 0.05, (name, k, sky)
        cam = gen_random_camera(name, k)
        assert cam.image_width == (64 if n <= 150 else 48 if n <= 1100 else 32) and cam.image_width * 9 == cam.image_height * 16
        assert cam.sqrt_spp in (2, 3) and 2 <= cam.bounce_limit <= 20
    assert all(nm in GEN_RANDOM and k < len(gen_random_case(nm)[1]) for nm, k in GEN_INTERIOR_VIEWS)


def test_paths_bounce():
    """over the whole catalogue the oracle traces at least 1.5 segments per sample: the cameras do not look at sky"""
    seg = n = 0
    for name in NAMES:
        for k in range(len(gen_random_case(name)[1])):
            _, _, s, m = _what_the_camera_sees(name, k)
            seg += s; n += m
    assert seg >= 1.5 * n, seg / n


def test_cameras_on_both_sides_of_mnear():
    """gen_ray_setup in float32: every entry has a camera whose own rays keep the static pad (far <= mnear) and, where the world
    has a sphere at all, one whose band widens (far > mnear) within reach; a world without spheres has mnear = 1e30 and kmin = 0 (rounded up),
    and its second camera stands outside the solids' box.  At least six entries have a camera beyond reach."""
    beyond = 0
    for name in NAMES:
        p = gen_random_prediction(name)
        t, reach = p["tree"], p["reach"]
        w, views, _, info = gen_random_case(name)
        cams = [gen_random_camera(name, k) for k in range(len(views))]
        pos = [[F(c.center.e[j]) for j in range(3)] for c in cams]
        far = []
        for q in pos:
            e = [F(q[j] - t["centre"][j]) for j in range(3)]
            far.append(F(F(np.sqrt(F(F(F(e[0] * e[0]) + F(e[1] * e[1])) + F(e[2] * e[2])))) * F(1.000001)) + t["R"])
        inr = [gen_in_reach(q, gen_camera_lens(c), reach) for q, c in zip(pos, cams)]
        assert inr[0] and not far[0] > t["mnear"], name
        assert np.linalg.norm(np.array(pos[0], float) - t["centre"]) <= 2.0 * t["R"] + 1.0
        assert inr[1], name
        if info["n_spheres"]:
            assert far[1] > t["mnear"] and t["kmin"] > 0, name
        else:
            assert t["mnear"] >= F(1e30) and t["kmin"] <= F(1.5e-45), name       # kmin: 0 rounded up, one denormal
            assert any(pos[1][j] < reach["lo"][j] or pos[1][j] > reach["hi"][j] for j in range(3)), name
        if name in GEN_FAR_VIEWS:
            assert not inr[2], name
            beyond += 1
    assert beyond >= 6


HOST_LOOP_CASES = ["mixed_3500_s0", "quads_2490_s1", "mixed_300_s1", "mixed_310_s0", "scales_1000_s0", "scales_540_s1", "scales_3_s1",
                   "offset_1000_s1", "offset_150_s0", "quads_270_s0", "line_1000_s0", "line_390_s1", "ties_360_s0", "ties_330_s1",
                   "instances_1000_s1", "instances_150_s0", "mixed_5_s0"]


def test_host_loop_cases_cover_the_catalogue():
    fams = {GEN_RANDOM[n][0] for n in HOST_LOOP_CASES}
    assert fams == set(GEN_FAMILIES)
    lds = {gen_random_prediction(n)["prims_in_lds"] for n in HOST_LOOP_CASES}
    assert lds == {True, False}
    assert max(GEN_RANDOM, key=lambda n: GEN_RANDOM[n][1]) in HOST_LOOP_CASES or "mixed_3500_s0" in HOST_LOOP_CASES


def _same(out, ref):
    assert (out["rgba"] == ref["rgba"]).all() and (out["accum"].view(np.uint32) == ref["accum"].view(np.uint32)).all()
    assert (out["segments_px"] == ref["segments_px"]).all()
    assert out["stats"]["segments"] == ref["segments"] and out["stats"]["rng_draws"] == ref["rng_draws"]
    st = out["states"].view(O.STATE_DTYPE)
    assert (st["d"] == ref["states"]["d"]).all() and (st["v"] == ref["states"]["v"]).all()


@pytest.mark.parametrize("name", HOST_LOOP_CASES)
def test_host_loops_equal_oracle(name):
    """hip.render_host with the unified tree (the CPU form of the kernels' walk) and without (the item scan) against
    oracle.render, bit for bit, from every camera of the entry"""
    w, views, _, _ = gen_random_case(name)
    p = gen_random_prediction(name)
    for k in range(len(views)):
        cam = gen_random_camera(name, k)
        ref = O.render(w, cam, nthreads=8)
        for tree in (True, False):
            out = hip.render_host(w, cam, nthreads=8, tree=tree)
            _same(out, ref)
            if tree:
                assert ("unified tree" in out["stats"]["kernel_name"]) == p["in_reach"][k], (k, out["stats"]["kernel_name"])
