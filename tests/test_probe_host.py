"""Light probes on the host (mort_hip_probe_bake_host, dev_probe.h): both host traversals against the reference of
tests/probe_ref.py -- the oracle's ray_color and the contract restated in numpy -- at tolerance 0: coefficients as raw 32-bit
words (any NaN equals any NaN), final streams as all 48 bytes.  The direction set, the quadrature, the summation order and the
command line.  No GPU."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

from mort_amd import hip, host, structs as S
from tests import oracle_lib as O
from tests import probe_ref as P
from tests import query_rays as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MORT = os.path.join(ROOT, "mort_amd", "bin", "mort")
F = np.float32

# (world, bounce limit or None = the camera's): the ten scenes (the final scenes at limit 4), a lit flat world with media, a placed
# world, one BVH_RANDOM and one GEN_RANDOM world
WORLDS = [(f"scene{k}", 4 if k in (8, 9) else None) for k in range(1, 11)] + \
    [("flat:lit_by_quad_with_media", None), ("placed:solid_inside_medium", None), ("bvhrandom:ties_64_s0", None), ("genrandom:instances_150_s1", 8)]
CENSUS = [("scene1", None), ("scene6", None), ("scene7", None), ("scene9", 4), ("flat:lit_by_quad_with_media", None)]
TREES = [False, True]


def _bake(ref, tree, **kw):
    streams = ref.streams0.copy()
    got = hip.probe_bake_host(ref.world, ref.params, ref.probes, streams, tree=tree, nthreads=4, **kw)
    return got["sh"], streams


@pytest.mark.parametrize("name,limit", CENSUS)
def test_probes_show_something(name, limit):
    """the census of tests/probe_ref.py, on the oracle's answers alone: the worlds the GPU tests use"""
    out = P.census(name, limit)
    print(name, {k: np.round(v, 3).tolist() for k, v in out.items()})


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("D", [64, 128, 320])
@pytest.mark.parametrize("name,limit", WORLDS)
def test_both_traversals_equal_the_reference(name, limit, D, samples, tree):
    ref = P.reference(name, D, samples, limit)
    sh, streams = _bake(ref, tree)
    P.assert_equal(sh, streams, ref, f"{name} D={D} samples={samples} tree={tree}")


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("name", ["scene1", "scene6", "flat:lit_by_quad_with_media"])
def test_a_callers_own_direction_set(name, tree):
    """axis-parallel directions, two zero components, a zero-length entry and unnormalised entries, used exactly as given"""
    ref = P.reference(name, P.OWN_D, 3, dirs="own")
    assert np.isfinite(ref.dirs).all() and (ref.dirs[6] == 0).all() and np.abs(np.linalg.norm(ref.dirs[7:20], axis=1) - 1).max() > 0.5
    sh, streams = _bake(ref, tree, dirs=ref.dirs)
    P.assert_equal(sh, streams, ref, f"{name} own directions tree={tree}")
    lib = P.reference(name, P.OWN_D, 3)
    assert (Q._words(lib.sh) != Q._words(ref.sh)).any(), "the set given is not the set used"


@pytest.mark.parametrize("tree", TREES)
def test_a_nan_direction(tree):
    """the guard is on the colour, not on the basis: a NaN direction gives NaN coefficients where the restatement has them"""
    ref = P.reference("scene1", P.OWN_D, 1, dirs="nan")
    nan = np.isnan(ref.sh)
    assert nan.any() and not nan.all(), "x = NaN, y and z finite: Y0, Y1, Y2, Y5, Y6 stay finite where the colour is"
    sh, streams = _bake(ref, tree, dirs=ref.dirs)
    assert (np.isnan(sh) == nan).all()
    P.assert_equal(sh, streams, ref, f"scene1 NaN direction tree={tree}")


@pytest.mark.parametrize("D", [64, 256, 320, 1024, 4096])
def test_the_librarys_direction_set(D):
    """both sides round a double whose libm error is below a float's half-ulp to the nearest float, so they differ by at most one
    float spacing at magnitude <= 1: 2^-23 per component; unit length to 2^-22"""
    got = hip.probe_directions(D)
    want = P.fibonacci(D)
    assert got.shape == (D, 3) and got.dtype == F
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -23
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max() <= 2.0 ** -22
    for bad in (0, 63, 65, 4160, -64):
        with pytest.raises(hip.MortHipError) as e:
            hip.probe_directions(bad)
        assert e.value.status == -1


NORMALS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)] + \
    [tuple(np.array(v) / math.sqrt(3.0)) for v in ((1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1))]


@pytest.mark.parametrize("D", [64, 256, 1024])
def test_quadrature_of_a_constant_sky(D):
    """the empty world under a background b: the irradiance is pi b for every normal, within the bound the restated set's Gram
    matrix G = (4 pi / D) sum Y Y^T gives: b sqrt(4 pi) sum_k A_k |Y_k(n)| |G_0k - delta_0k|, plus 1e-5 pi b for the fp32 sums"""
    b = np.array([0.25, 0.5, 2.0], dtype=F)
    ref = P.reference("flat:empty", D, 1, background=(0.25, 0.5, 2.0))
    assert (ref.s == b).all(), "every direction returns the background"
    Y = P.basis64(P.fibonacci(D))
    G = (4.0 * math.pi / D) * (Y.T @ Y)
    A = np.array([math.pi] + [2.0 * math.pi / 3.0] * 3 + [math.pi / 4.0] * 5)
    sh, _ = _bake(ref, False)
    for n in NORMALS:
        Yn = P.basis64(np.array([n]))[0]
        bound = math.sqrt(4.0 * math.pi) * float((A * np.abs(Yn) * np.abs(G[0] - np.eye(9)[0])).sum())
        got = hip.sh9_irradiance(sh[0], n).astype(np.float64)
        want = math.pi * b.astype(np.float64)
        assert (np.abs(got - want) <= b * bound + 1e-5 * want).all(), (n, got, want, bound)
        # the library's evaluation is the formula's
        e = (A[:, None] * sh[0].astype(np.float64) * Yn[:, None]).sum(0)
        assert np.allclose(got, e.astype(F), rtol=1e-6, atol=0)


def test_the_sum_order_is_noticed():
    """on numpy alone: the batches added in descending order, or a sequential sum inside a batch, differ from the contract's"""
    ref = P.reference("scene1", 320, 1)
    contract = Q._words(P.project(ref.s, ref.dirs, 1))
    assert (contract == Q._words(ref.sh)).all()
    for order in ("descending", "sequential"):
        other = Q._words(P.project(ref.s, ref.dirs, 1, order=order))
        assert (other != contract).any(), order
        assert (other[0] != contract[0]).any(), f"{order}: the first probe alone shows it"


def test_streams_untouched_words_keep_their_bits():
    """only d and v[] of a stream are written: the Box-Muller words keep the caller's bits, drawn from or not"""
    ref = P.reference("scene7", 64, 1)
    streams = ref.streams0.copy()
    for k, v in (("bf", 0x11111111), ("bfd", 0x22222222), ("pad", 0x44444444)):
        streams[k] = v
    streams["be"] = 3.25; streams["bed"] = -7.5
    before = streams.copy()
    sh = hip.probe_bake_host(ref.world, ref.params, ref.probes, streams, tree=True)["sh"]
    assert (Q._words(sh) == Q._words(ref.sh)).all()
    for k in ("bf", "bfd", "be", "pad", "bed"):
        assert (streams[k] == before[k]).all(), k
    assert (streams["d"] == ref.streams["d"]).all() and (streams["v"] == ref.streams["v"]).all()
    quiet = (ref.streams.view(np.uint8).reshape(-1, 48) == ref.streams0.view(np.uint8).reshape(-1, 48)).all(1)
    assert quiet.any() and (~quiet).any() and streams[quiet].tobytes() == before[quiet].tobytes(), "a direction that draws nothing keeps its bits"


@pytest.mark.parametrize("sid,tree,spec", [(1, False, "0.5,1.25,2,64,2"), (6, True, "278,278,-300"), (7, False, "278,278,100,128")])
def test_sh_probe_on_the_command_line(sid, tree, spec):
    """`mort <scene> --mode host --sh-probe X,Y,Z[,D[,N]]`: one probe at time 0.5, the library's set, the scene camera's
    parameters, subsequences 0 .. D - 1 of the seed: the host form's answer"""
    if not os.path.exists(MORT):
        subprocess.check_call(["make", "-C", ROOT, "host", "hip", "cli"])
    parts = spec.split(",")
    pos = [float(v) for v in parts[:3]]
    D = int(parts[3]) if len(parts) > 3 else 256
    N = int(parts[4]) if len(parts) > 4 else 1
    args = [MORT, str(sid), "--mode", "host", "--width", "48", "--sh-probe", spec] + (["--tree"] if tree else [])
    p = subprocess.run(args, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, "one JSON line"
    j = json.loads(lines[0])
    assert j["directions"] == D and j["samples"] == N and j["position"] == pos and j["mode"] == "host"
    world, cam = host.build_scene(sid, width=48, spp=1)
    probes = np.zeros(1, dtype=hip.PROBE_DTYPE)
    probes["position"] = pos; probes["time"] = 0.5
    want = hip.probe_bake_host(world, hip.probe_params_from_camera(cam, D, N), probes, O.seed_states(S.DEFAULT_SEED, D, 1), tree=tree)["sh"][0]
    got = np.array(j["sh"], dtype=F)
    assert got.shape == (9, 3) and (Q._words(got) == Q._words(want)).all(), (j, want)
    assert np.abs(want[0]).max() > 0
    for bad in ("1,2", "0,0,0,100", "0,0,0,64,0"):
        q = subprocess.run([MORT, str(sid), "--mode", "host", "--sh-probe", bad], cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert q.returncode != 0, bad
    q = subprocess.run([MORT, str(sid), "--mode", "host", "--sh-probe", spec, "--probe", "1,1"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert q.returncode != 0 and "excludes" in q.stderr
