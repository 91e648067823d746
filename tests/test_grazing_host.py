"""The grazing battery on the CPU (tests/grazing.py): 65 x 65 frames a few millionths of a primitive wide, aimed at
sphere limbs, axis poles, quad edges and corners, a rotated box's silhouette and medium boundaries, so that every primary ray
needs one of the tree walk's margins.  The host loop's unified-tree walk and its item scan -- the bodies the gfx950 kernels
run -- against the CPU oracle: the feature pass word for word, the render at 1 spp and bounce limit 8 (its scattered rays start
on the limb) on accumulator bits, per-pixel segment counts and final stream words.  Tolerance 0.  Every case first asserts, on
the oracle's frame alone, that it shows what it is for."""
import numpy as np
import pytest

from mort_amd import hip
from tests import grazing as G
from tests.feature_ref import assert_same_words
from tests.test_host_mode import same

NT = G.NT


def _run(case, oracle):
    w, cam, feat, ren = G.reference(case)
    s = G.check_conditions(case, cam, feat)
    print(f"{case}: target {s['target']:.3f} over {s['over']:.3f} zero {s['zero']} medium {s['medium']:.3f}")
    for tree in (True, False):
        assert_same_words(hip.render_features_host(w, cam, nthreads=NT, tree=tree), feat, f"{case}, features, tree={tree}")
        out = hip.render_host(w, cam, nthreads=NT, tree=tree)
        name = out["stats"]["kernel_name"]
        want = "unified tree" if tree and case.walk == "tree" else "item scan"
        assert want in name, f"{case}: {name}"
        same(out, ren, oracle)
        if tree and case.walk == "tree" and "zero" in case.cond:
            assert out["stats"]["reference_walks"] > 0, f"{case}: rays with a zero component go to the reference's scan"


@pytest.mark.parametrize("group", [g for g in G.GROUPS if not g.startswith("bvh")])
def test_flat_grazing_cases_equal_the_oracle(oracle, group):
    cases = [c for c in G.FLAT if c.group == group]
    assert cases
    for case in cases:
        _run(case, oracle)


@pytest.mark.parametrize("group", [g for g in G.GROUPS if g.startswith("bvh")])
def test_bvh_grazing_cases_equal_the_oracle(oracle, group):
    """the host loop walks the reference's BVH (the own four-wide tree has no host form: tests/test_gpu_grazing.py)"""
    for case in [c for c in G.BVH if c.group == group]:
        _run(case, oracle)


def test_the_table_is_as_large_as_promised():
    assert len(G.FLAT) >= 100 and len(G.BVH) >= 30
    assert sum("over" in c.cond for c in G.CASES) >= 8
    for r in (0.01, 0.5, 10):
        sides = {c.name.split("r", 1)[1][:2] for c in G.FLAT if c.group in (f"limb_r{r:g}", f"pole_r{r:g}")}
        assert sides == set(G.AXES), (r, sides)
    assert any(c.walk == "scan" and c.group == "beyond_reach" for c in G.FLAT)
