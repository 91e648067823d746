"""Inputs the depth-map tests share (tests/test_depth_host.py, tests/test_gpu_depth.py): the four worlds and their
nine probes, the restated maps over the oracle (computed once per process and never changed), random maps, the scene-6 grid with
its baked maps, the leak-check scene.  The expected answers are tests/depth_ref.py's."""
import functools

import numpy as np

from mort_amd import hip
from tests import depth_ref as D
from tests import query_rays as Q
from tests import volume_cases as K
from tests import worlds as Wd
from tests.feature_ref import primary_rays

F = np.float32
SUBSAMPLES = (1, 2, 3)
# scene 6: rotated boxes behind transform chains; scene 1: a reference-BVH world, the item loop; a GEN_RANDOM world (a unified
# tree, so both tree choices); scene 7: the Cornell box with two media, which the bake passes over
WORLDS = ("scene6", "scene1", "genrandom:scales_150_s0", "scene7")
N_PROBES = 9


@functools.lru_cache(maxsize=None)
def world(name):
    """(world, cam, max_distance, rec, hit): rec and hit are the oracle's answers to the camera's primary rays; the cap is half the
    median distance of those hits, so that rays end on both sides of it"""
    w, cam = Q.WORLDS[name]()
    rays = Q.ray8(primary_rays(cam), Q.INF)
    rec, hit = Q.oracle_closest(w, rays)
    dist = rec["t"][hit].astype(np.float64) * np.linalg.norm(rays[hit, 3:6].astype(np.float64), axis=1)
    return w, cam, F(0.5 * np.median(dist[np.isfinite(dist)])), rec, hit


@functools.lru_cache(maxsize=None)
def probes(name):
    """PROBE_DTYPE (9,): 0 the camera (free space), 1 exactly on a surface (an oracle hit point; in the Cornell scenes exactly
    on the x = 555 wall's plane), 2 between the two (in the Cornell scenes inside the tall box), 3 a million away (out of the
    tree's reach: the scan), 4 a NaN coordinate, 5..8 further oracle hit points pulled halfway to the camera, time 0 and 1 among
    them"""
    w, cam, _, rec, hit = world(name)
    eye = np.array([cam.center.e[k] for k in range(3)], dtype=F)
    pts = rec["p"][hit & np.isfinite(rec["p"]).all(1)]
    pick = pts[np.linspace(0, len(pts) - 1, 6).astype(int)]
    pr = np.zeros(N_PROBES, dtype=hip.PROBE_DTYPE)
    pr["time"] = 0.5
    pr["position"][0] = eye
    pr["position"][1] = pick[0]
    pr["position"][2] = (F(0.5) * (eye + pick[1])).astype(F)
    if name in ("scene6", "scene7"):
        pr["position"][1] = (555.0, 278.0, 278.0)
        pr["position"][2] = (350.0, 150.0, 375.0)
    pr["position"][3] = (eye + F(1e6)).astype(F)
    pr["position"][4] = eye
    pr["position"][4][1] = np.nan
    for k in range(5, N_PROBES):
        pr["position"][k] = (F(0.5) * (eye + pick[k - 4])).astype(F)
    pr["time"][6], pr["time"][7] = 0.0, 1.0
    pr.setflags(write=False)
    return pr


@functools.lru_cache(maxsize=None)
def maps(name, s):
    """float32 (9, 200): the restatement over the oracle"""
    w, _, cap, _, _ = world(name)
    m = D.bake(w, probes(name), s, cap)
    m.setflags(write=False)
    return m


def params(name, s):
    return hip.DEPTH_PARAMS(s, float(world(name)[2]))


def has_tree(name):
    return bool(Q.reach(world(name)[0])["tree"])


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.flatnonzero((K.words(got) != K.words(want)).reshape(len(want), -1).any(1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} differ, first {bad[0]}: {got[bad[0]]} / {want[bad[0]]}"


# ------------------------------------------------------------------------------------------------------------- the sampler

def random_maps(g, seed=4):
    """float32 (probes, 200): m1 in (0, 2) (K.grid's cells are 0.45 .. 1.3 wide, so points lie on both sides of it), m2 = m1^2
    plus a variance in (0, 0.5); every texel its own, borders included -- the sampler must read what is there"""
    rng = np.random.default_rng(seed)
    m1 = rng.uniform(0.0, 2.0, size=(g.probes, D.SIDE, D.SIDE)).astype(F)
    m2 = (m1 * m1 + rng.uniform(0.0, 0.5, size=m1.shape).astype(F)).astype(F)
    return np.stack([m1, m2], axis=3).reshape(g.probes, D.DEPTH_FLOATS)


def flt_max_maps(g):
    m = np.zeros((g.probes, D.SIDE, D.SIDE, 2), dtype=F)
    m[..., 0] = np.finfo(F).max
    m[..., 1] = 1.0
    return m.reshape(g.probes, D.DEPTH_FLOATS)


def exact_points(g, n=6):
    """float32 (n, 6): points exactly at probes (s1 = 0 with bias 0), unit normals"""
    pos = D.positions(g)
    pick = pos[np.linspace(0, len(pos) - 1, min(n, len(pos))).astype(int)]
    return np.concatenate([pick, Q._unit_sphere(np.random.default_rng(31), len(pick))], axis=1).astype(F)


def sampler_points(g, n_uniform=600):
    """K.points (uniform, every probe position, cell faces, far outside, infinite and NaN coordinates) and exact_points"""
    return np.concatenate([K.points(g, n_uniform), exact_points(g)]).astype(F)


SCENE6_CAP = F(1.5 * np.sqrt(3.0 * 177.5 ** 2))  # the command line's rule for K.scene6_grid's spacing


@functools.lru_cache(maxsize=None)
def scene6_maps(s=2):
    """(grid, float32 (27, 200)): K.scene6_grid's probes baked by the restatement over the oracle"""
    g = K.scene6_grid()
    w = K.scene6()[0]
    pr = np.zeros(g.probes, dtype=hip.PROBE_DTYPE)
    pr["position"], pr["time"] = D.positions(g), g.time
    m = D.bake(w, pr, s, SCENE6_CAP)
    m.setflags(write=False)
    return g, m


# -------------------------------------------------------------------------------------------------------------- leak check

LEAK_BRIGHT = F(3.0)


@functools.lru_cache(maxsize=None)
def leak():
    """(world, grid, records, points (n, 6)): two probes a cell apart on x, probe 0 a constant bright record and probe 1 zeros, a
    quad wall across the cell at 0.6, points at 0.3 of the cell facing probe 0"""
    w, _ = Wd.flat_world([("quad", (0.6, -40.0, -40.0), (0, 80.0, 0), (0, 0, 80.0), ("lamb", (.7, .7, .7)))])
    g = hip.VOLUME_GRID((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 1, 1), 0.5)
    sh = np.zeros((2, 27), dtype=F)
    sh[0, 0:3] = LEAK_BRIGHT
    rng = np.random.default_rng(77)
    n = 200
    pts = np.zeros((n, 6), dtype=F)
    pts[:, 0] = 0.3
    pts[:, 1:3] = rng.uniform(-0.3, 0.3, size=(n, 2))
    pts[:, 3] = -1.0
    return w, g, K.V.pack(sh), pts


def leak_share(out):
    """probe 1's share of the weights' sum from a sampler's output: probe 0 alone carries light, E = B_0 bright W_0 / wsum"""
    b0 = float(K.V.A[0]) * float(K.V.C0)
    return 1.0 - out[:, 0].astype(np.float64) / (b0 * float(LEAK_BRIGHT))
