"""Ray sets, worlds and the oracle side of the ray-query tests (tests/test_query_host.py, tests/test_gpu_query.py; DESIGN.md
4.14).  Everything here is built from the CPU oracle and numpy alone -- nothing calls libmort_hip.so except the device-free
debug entry that reports where a world's unified tree may be walked from (reach()), which the far set is censused against.

A ray is 8 float32: origin, direction, time, t_max (hip.RAY_DTYPE).  Every set is a function of the world and its camera and
is deterministic; build(name) caches the world, its sets and the oracle's answers once per process, and nothing may change
them."""
import functools

import numpy as np

from mort_amd import host, hip, structs as S
from tests import oracle_lib as O
from tests import worlds as Wd
from tests.feature_ref import primary_rays

F = np.float32
T_MIN = F(0.001)
INF = F(np.inf)


# ---------------------------------------------------------------------------------------------------------------- worlds

def _scene(sid):
    return lambda: host.build_scene(sid, width=48, spp=1)


def _flat(name):
    def make():
        spec = Wd.FLAT_WORLDS[name]
        w, _ = Wd.flat_world(spec["prims"], media=spec.get("media", ()), late_list=spec.get("late_list", False))
        return w, Wd.flat_camera(spp=1, width=48)
    return make


def _bvh(name):
    return lambda: (Wd.custom_bvh_world(Wd.BVH_WORLDS[name]), Wd.bvh_camera(width=48, spp=1))


def _placed(name):
    def make():
        w, cam = Wd.PLACED[name]()
        cam.image_width = 48
        host.lib().mort_camera_initialize(cam)
        return w, cam
    return make


def _bvh_random(name):
    return lambda: (Wd.bvh_random_case(name)[0], Wd.bvh_random_camera(name, 0, width=48))


def _gen_random(name):
    return lambda: (Wd.gen_random_case(name)[0], Wd.gen_random_camera(name, 0, width=48))


def _random(seed):
    def make():  # the worlds of tests/test_features_oracle.py's random test, from its first view
        rng = np.random.default_rng(1000 + seed)
        w, _ = Wd.random_world(rng, n_spheres=int(rng.integers(1, 60)), n_quads=int(rng.integers(0, 12)), n_boxes=int(rng.integers(0, 3)),
                               n_media=int(rng.integers(0, 3)), with_light=bool(seed % 2))
        _, cam = host.build_scene(2, width=48, spp=1)
        Wd.set_view(cam, (0, 2, 9), (0, 1, 0), vfov=50, defocus=0.0)
        return w, cam
    return make


# eight of BVH_RANDOM: every family, one `ties` world, one above the limit on the LDS images (ties_670: BVH_LIMIT_SIZES)
BVH_RANDOM_PICK = ("uniform_64_s1", "cluster_300_s0", "scales_7_s0", "line_64_s0", "shells_300_s1", "ties_64_s0", "ties_670_s1", "uniform_2_s0")

# six of GEN_RANDOM (worlds without a reference BVH, from their first camera): radii over four decades, a world 1e6 from
# the origin, duplicates with the primitives outside the LDS image (ties_360: GEN_LIMIT_SIZES), 75 chain ids, the line at the
# depth the catalogue's cap entries have below them, and the largest world the reference's tables hold
GEN_RANDOM_PICK = ("scales_150_s0", "offset_150_s1", "ties_360_s0", "instances_150_s1", "line_150_s1", "mixed_3500_s0")

WORLDS = {}
WORLDS.update({f"scene{sid}": _scene(sid) for sid in range(1, 11)})
WORLDS.update({f"flat:{n}": _flat(n) for n in Wd.FLAT_WORLDS})
WORLDS.update({f"bvh:{n}": _bvh(n) for n in Wd.BVH_WORLDS})
WORLDS.update({f"placed:{n}": _placed(n) for n in Wd.PLACED})
WORLDS.update({f"bvhrandom:{n}": _bvh_random(n) for n in BVH_RANDOM_PICK})
WORLDS.update({f"genrandom:{n}": _gen_random(n) for n in GEN_RANDOM_PICK})
WORLDS.update({f"random:{k}": _random(k) for k in range(10)})

# worlds without a solid primitive: no ray can hit a solid, so the hit-rate and occlusion censuses do not apply to them
NO_SOLIDS = ("flat:empty", "placed:grazed_medium")
# worlds whose streams must advance and end on a medium for at least 30 rays ("media under a quad light" = lit_by_quad_with_media)
MEDIA_CENSUS = ("scene7", "scene9", "flat:lit_by_quad_with_media")


# -------------------------------------------------------------------------------------------------------------- the oracle

def _media(world):
    o = world.c.objs
    return [i for i in range(o.num_constant_medium) if not o.host_constant_medium[i].skip]


def some_streams(n, seed=S.DEFAULT_SEED):
    """n distinct XORWOW streams (subsequences 0 .. n-1 of `seed`)"""
    return O.seed_states(seed, n, 1)


def oracle_closest(world, rays, states=None):
    """world::hit(ray, interval(0.001, t_max), rec) for every ray.  states None: the reference side sets `skip` on the media
    around the call (as feature_ref.oracle_features does) and it is asserted that nothing was drawn; else the streams are
    advanced in place.  Returns (records O.HIT_DTYPE (n,), hit bool (n,))."""
    rays = np.ascontiguousarray(rays, dtype=F).reshape(-1, 8)
    n = rays.shape[0]
    if states is not None:
        return O.world_hit_batch(world, rays[:, :7], T_MIN, rays[:, 7], states=states)
    o = world.c.objs
    media = _media(world)
    streams = np.ascontiguousarray(np.resize(some_streams(64), n))
    before = streams.copy()
    try:
        for i in media:
            o.host_constant_medium[i].skip = True
        rec, hit = O.world_hit_batch(world, rays[:, :7], T_MIN, rays[:, 7], states=streams)
    finally:
        for i in media:
            o.host_constant_medium[i].skip = False
    assert streams.tobytes() == before.tobytes(), "the oracle drew a random number with every medium passed over"
    return rec, hit


def medium_materials(world):
    o = world.c.objs
    return {(o.host_constant_medium[i].mat_type, o.host_constant_medium[i].mat_idx) for i in _media(world)}


def on_medium(world, rec, hit):
    """which of the oracle's hits are medium hits: constant_medium::hit's record -- normal (1, 0, 0), front face, the medium's
    phase function as material.  (A solid with that material AND that normal would count too; its u, v are then left out of the
    comparison for no reason, which the tests' census of medium hits bounds: it counts only rays whose stream advanced.)"""
    mats = medium_materials(world)
    is_mat = np.zeros(len(rec), dtype=bool)
    for mt, mi in mats:
        is_mat |= (rec["mat_type"] == mt) & (rec["mat_idx"] == mi)
    return hit & is_mat & (rec["normal"] == np.array([1, 0, 0], dtype=F)).all(1) & rec["front_face"].astype(bool)


# ------------------------------------------------------------------------------------------------------------ comparison

def _words(a):
    """float32 array as raw 32-bit words with every NaN mapped to one word: IEEE 754 leaves a generated NaN's sign and payload
    open, and x86 and gfx950 generate different ones (0xffc00000 / 0x7fc00000).  Every other value is compared bit for bit."""
    a = np.ascontiguousarray(a, dtype=F)
    w = a.view(np.uint32).copy()
    w[np.isnan(a)] = 0x7fc00000
    return w


FIELDS = ("hit", "t", "p", "normal", "mat_type", "mat_idx", "front_face", "u", "v")


def assert_hits_equal(world, got, rec, hit, what, with_media=False, medium_hits=None):
    """got: hip.HIT_DTYPE (n,) from a query; rec, hit: the oracle's.  Tolerance 0: every field of every ray, u and v on medium
    hits alone left out; a miss must be an all-zero record.  medium_hits: which of the oracle's hits are medium hits, where the
    caller knows better than on_medium (a medium under rotate_y: its normal is (1, 0, 0) turned, and compared like any other)."""
    n = len(rec)
    assert got.shape == (n,)
    ghit = (got["flags"] & hip.HIT_HIT) != 0
    bad = np.flatnonzero(ghit != hit)
    assert bad.size == 0, f"{what}: hit flag differs for {bad.size} of {n} rays, first {bad[0]}: got {got[bad[0]]}, oracle hit {hit[bad[0]]} {rec[bad[0]]}"
    miss = ~hit
    assert not got[miss].view(np.uint8).any(), f"{what}: a miss is not an all-zero record"
    med = np.zeros(n, dtype=bool) if not with_media else on_medium(world, rec, hit) if medium_hits is None else np.asarray(medium_hits, dtype=bool) & hit
    gmed = (got["flags"] & hip.HIT_MEDIUM) != 0
    assert (gmed[hit] == med[hit]).all() if with_media else not gmed.any(), f"{what}: medium flags differ"
    h = hit
    diffs = {
        "t": _words(got["t"][h]) != _words(rec["t"][h]),
        "p": (_words(got["p"][h]) != _words(rec["p"][h])).any(1),
        "normal": (_words(got["normal"][h]) != _words(rec["normal"][h])).any(1),
        "mat_type": got["mat_type"][h] != rec["mat_type"][h],
        "mat_idx": got["mat_idx"][h] != rec["mat_idx"][h],
        "front_face": ((got["flags"][h] & hip.HIT_FRONT_FACE) != 0) != rec["front_face"][h].astype(bool),
        "u": (_words(got["u"][h]) != _words(rec["u"][h])) & ~med[h],
        "v": (_words(got["v"][h]) != _words(rec["v"][h])) & ~med[h],
    }
    for k, d in diffs.items():
        if d.any():
            i = np.flatnonzero(h)[np.flatnonzero(d)[0]]
            raise AssertionError(f"{what}: {k} differs for {int(d.sum())} of {int(h.sum())} hits; first ray {i}: got {got[i]}, oracle {rec[i]}")
    if with_media:  # a medium hit's own contract
        m = got[gmed]
        assert (m["u"] == 0).all() and (m["v"] == 0).all() and (medium_hits is not None or (m["normal"] == np.array([1, 0, 0], dtype=F)).all())


# -------------------------------------------------------------------------------------------------------------- ray sets

def ray8(r7, t_max):
    r7 = np.ascontiguousarray(r7, dtype=F).reshape(-1, 7)
    out = np.empty((r7.shape[0], 8), dtype=F)
    out[:, :7] = r7
    out[:, 7] = t_max
    return out


def _unit_sphere(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


def reach(world):
    """dict(tree, lo, hi, reach) of the world's unified tree (hip.debug_gen_reach), float32 as the kernels compare them"""
    return hip.debug_gen_reach(world)


def in_reach(info, origins):
    """the reach test restated: camera_in_reach with rad = 0, per origin, in float32"""
    o = np.ascontiguousarray(origins, dtype=F)
    lo = (info["lo"] - info["reach"]).astype(F)
    hi = (info["hi"] + info["reach"]).astype(F)
    with np.errstate(invalid="ignore"):
        return ((o >= lo) & (o <= hi)).all(1)


def _extent(world, prim, rec, hit):
    """(centre, radius) of what the rays should be aimed at: the tree's box where the world has one, else the primary hits"""
    info = reach(world)
    if info["tree"]:
        lo, hi = info["lo"].astype(np.float64), info["hi"].astype(np.float64)
        return 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo)), float(info["reach"])
    pts = rec["p"][hit].astype(np.float64) if hit.any() else prim[:, 0:3].astype(np.float64)
    pts = pts[np.isfinite(pts).all(1)]
    c = np.median(pts, axis=0)
    return c, float(np.percentile(np.linalg.norm(pts - c, axis=1), 90)) + 1.0, 0.0


class Sets:
    """the ray sets of one world and the oracle's answers to them"""


@functools.lru_cache(maxsize=None)
def build(name):
    world, cam = WORLDS[name]()
    rng = np.random.default_rng(sum(map(ord, name)))
    s = Sets()
    s.name, s.world, s.cam = name, world, cam

    # primary: the feature pass's rays.  Where the world's own camera sees a solid in fewer than half of them (one small sphere in
    # a wide frame, the sparse scene 10) the camera keeps its place and turns to the hit point nearest the median of the hit
    # points with a narrower field of view: the first of these whole degrees that reaches a half, else the best of them
    prim7 = primary_rays(cam)
    primary = ray8(prim7, INF)
    rec, hit = oracle_closest(world, primary)
    if name not in NO_SOLIDS and hit.mean() < 0.5 and hit.any():
        frm = tuple(cam.lookfrom.e[i] for i in range(3))
        pts = rec["p"][hit].astype(np.float64)
        at = tuple(float(v) for v in pts[np.argmin(np.linalg.norm(pts - np.median(pts, axis=0), axis=1))])
        tried = []
        for vfov in (40, 30, 20, 14, 10, 7, 5, 3, 2, 1):
            if vfov >= cam.vfov:
                continue
            Wd.set_view(cam, frm, at, vfov=vfov)
            rate = float(oracle_closest(world, ray8(primary_rays(cam), INF))[1].mean())
            tried.append((rate >= 0.5, rate if rate < 0.5 else 0.0, -len(tried), vfov))
            if rate >= 0.5:
                break
        Wd.set_view(cam, frm, at, vfov=max(tried)[3])
        prim7 = primary_rays(cam)
        primary = ray8(prim7, INF)
        rec, hit = oracle_closest(world, primary)

    # secondary: from the oracle's hit points of the primary set (a missed ray's from the hit point of another ray, from the
    # camera where nothing was hit), directions uniform on the sphere, times 0, 0.5, 1 and random in turn
    n = primary.shape[0]
    good = np.flatnonzero(hit & np.isfinite(rec["p"]).all(1))
    src = np.arange(n)
    if good.size:
        src = np.where(np.isin(src, good), src, good[rng.integers(0, good.size, n)])
    org = (rec["p"][src] if good.size else prim7[:, 0:3]).astype(F)
    tm = np.choose(np.arange(n) % 4, [np.zeros(n), np.full(n, 0.5), np.ones(n), rng.random(n)]).astype(F)
    # t_max: every fourth ray unbounded, the others a length up to twice the median distance of the primary hits (directions
    # are of unit length): lines of sight that end before and behind what they meet
    dist = rec["t"][hit].astype(np.float64) * np.linalg.norm(prim7[hit, 3:6].astype(np.float64), axis=1)
    scale = float(np.median(dist[np.isfinite(dist)])) if np.isfinite(dist).any() else 1.0
    tmx = np.where(np.arange(n) % 4 == 3, np.inf, rng.uniform(0.0, 2.0 * scale, n)).astype(F)
    secondary = ray8(np.concatenate([org, _unit_sphere(rng, n), tm[:, None]], axis=1), tmx)

    # interval: up to 96 rays of the two sets that hit, re-issued with t_max at and around the oracle's t
    both = np.concatenate([primary, secondary])
    brec, bhit = oracle_closest(world, both)
    pick = np.flatnonzero(bhit & np.isfinite(brec["t"]))
    pick = pick[np.linspace(0, len(pick) - 1, min(96, len(pick))).astype(int)] if len(pick) else pick
    t = brec["t"][pick]
    s.interval_kinds = ("exact", "below", "half", "double", "inf", "t_min", "zero", "negative")
    tmaxes = [t, np.nextafter(t, F(0)), F(0.5) * t, F(2) * t, np.full_like(t, INF), np.full_like(t, T_MIN), np.zeros_like(t), np.full_like(t, -1)]
    s.interval_n = len(pick)
    s.interval_t = t
    interval = np.concatenate([ray8(both[pick, :7], tm_) for tm_ in tmaxes]) if len(pick) else np.zeros((0, 8), dtype=F)

    # far: origins 3x and 100x beyond the tree's reach (beyond the scene's own size where the world has no tree), aimed into it ...
    c, rad, rch = _extent(world, prim7, rec, hit)
    far = []
    for k, mult in enumerate((3.0, 100.0)):
        m = 64
        out = _unit_sphere(rng, m).astype(np.float64)
        o = c + out * (rad + mult * max(rch, rad))
        target = c + rng.uniform(-0.5, 0.5, (m, 3)) * rad
        if hit.any():  # half of them at points the primary rays hit
            pts = rec["p"][hit][rng.integers(0, int(hit.sum()), m // 2)].astype(np.float64)
            target[: m // 2] = np.where(np.isfinite(pts), pts, target[: m // 2])
        d = target - o
        tm_ = rng.random(m)
        far.append(ray8(np.concatenate([o, d, tm_[:, None]], axis=1), INF))
    # ... and origins no reach holds: one coordinate NaN, +inf or -inf, directions uniform on the sphere
    m = 48
    o = org[np.linspace(0, n - 1, m).astype(int)].copy()
    o[np.arange(m), rng.integers(0, 3, m)] = np.resize(np.array([np.nan, np.nan, np.inf, -np.inf], dtype=F), m)
    d = _unit_sphere(rng, m)
    back = np.arange(0, m, 4)  # every other NaN origin: the camera looking away from the scene, so that no box lies ahead on the other two axes
    o[back] = prim7[back * (n // m), 0:3]
    d[back] = -prim7[back * (n // m), 3:6]
    o[back, rng.integers(0, 3, back.size)] = np.nan
    far.append(ray8(np.concatenate([o, d, np.full((m, 1), 0.5, dtype=F)], axis=1), INF))
    far = np.concatenate(far)
    s.far_origins = far[:, 0:3].copy()

    # axis: directions with one and with two components exactly 0, zero-length directions, a NaN component -- from the camera
    # and from the primary hit points
    m = 48
    o = np.concatenate([prim7[:m // 2, 0:3], org[np.linspace(0, n - 1, m - m // 2).astype(int)]])
    ax = []
    for kind in range(4):
        d = _unit_sphere(rng, m)
        k = rng.integers(0, 3, m)
        if kind == 0:
            d[np.arange(m), k] = 0
        elif kind == 1:
            d[np.arange(m), k] = 0; d[np.arange(m), (k + 1) % 3] = 0
            d[::5, :] = np.where(d[::5, :] != 0, np.sign(d[::5, :]), 0)  # some of unit length along the axis
            d[1::7, :] = -np.abs(d[1::7, :]) * (d[1::7, :] != 0)        # and -0.0 in the zero components
        elif kind == 2:
            d[:] = 0
            d[::2] = -0.0
        else:
            d[np.arange(m), k] = np.nan
        ax.append(ray8(np.concatenate([o, d.astype(F), np.full((m, 1), 0.5, dtype=F)], axis=1), INF))
    axis = np.concatenate(ax)

    s.sets = dict(primary=primary, secondary=secondary, interval=interval, far=far, axis=axis)
    s.all = np.concatenate(list(s.sets.values()))
    s.slices, at = {}, 0
    for k, v in s.sets.items():
        s.slices[k] = slice(at, at + len(v)); at += len(v)
    s.rec, s.hit = oracle_closest(world, s.all)           # media passed over
    s.streams0 = some_streams(len(s.all))
    s.streams = s.streams0.copy()
    s.mrec, s.mhit = oracle_closest(world, s.all, states=s.streams)  # media evaluated; s.streams = the final states
    s.advanced = (s.streams.view(np.uint8).reshape(len(s.all), 48) != s.streams0.view(np.uint8).reshape(len(s.all), 48)).any(1)
    for a in (s.all, s.rec, s.hit, s.mrec, s.mhit, s.streams0, s.streams, s.advanced):
        a.setflags(write=False)
    return s


def census(s):
    """The sets show something, asserted on the oracle's answers alone.  Returns the figures."""
    name, out = s.name, {}
    ps = slice(s.slices["primary"].start, s.slices["secondary"].stop)
    rate = float(s.hit[ps].mean())
    out["hit_rate"] = rate
    if name not in NO_SOLIDS:
        assert 0.20 <= rate <= 0.95, f"{name}: the primary and secondary sets hit in {rate:.1%} of rays"
        # occlusion: the same two sets; each outcome in at least 10 %
        assert 0.10 <= rate <= 0.90, f"{name}: occlusion outcomes {rate:.1%} / {1 - rate:.1%}"
    # interval
    iv, k = s.slices["interval"], s.interval_n
    out["interval_rays"] = k
    if name not in NO_SOLIDS:
        assert k >= 16, f"{name}: {k} rays in the interval set"
    if k:
        part = lambda j: slice(iv.start + j * k, iv.start + (j + 1) * k)  # noqa: E731
        exact, below = part(0), part(1)
        assert s.hit[exact].all() and (s.rec["t"][exact] == s.interval_t).all(), f"{name}: a root equal to t_max is accepted"
        same = s.hit[below] & (s.rec["t"][below] == s.rec["t"][exact]) & (s.rec["mat_idx"][below] == s.rec["mat_idx"][exact]) & \
            (s.rec["p"][below] == s.rec["p"][exact]).all(1)
        assert not same.any(), f"{name}: t_max one ulp below the root still returns the same record"
        out["below_misses"] = int((~s.hit[below]).sum())
        for j in (5, 6, 7):  # t_max = 0.001, 0, -1: nothing is hit
            assert not s.hit[part(j)].any() and not s.mhit[part(j)].any(), f"{name}: a hit in an empty interval"
    # far
    info = reach(s.world)
    if info["tree"]:
        assert not in_reach(info, s.far_origins).any(), f"{name}: a far origin within the tree's reach"
        if name not in NO_SOLIDS:  # (placed:grazed_medium looks at its medium from out of reach on purpose)
            assert in_reach(info, s.all[s.slices["primary"], 0:3]).all(), f"{name}: the camera out of the tree's reach"
    out["far_hits"] = int(s.hit[s.slices["far"]][:128].sum())  # of the 128 finite ones
    if name not in NO_SOLIDS:
        assert out["far_hits"] >= 8, f"{name}: only {out['far_hits']} far rays hit anything"
    # media
    ends_on_medium = on_medium(s.world, s.mrec, s.mhit) & s.advanced
    out["medium_hits"] = int(ends_on_medium.sum())
    out["advanced"] = int(s.advanced.sum())
    if name in MEDIA_CENSUS:
        assert out["medium_hits"] >= 30, f"{name}: {out['medium_hits']} rays advance their stream and end on a medium"
    if not _media(s.world):
        assert not s.advanced.any()
    return out
