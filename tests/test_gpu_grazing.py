"""The grazing battery (tests/grazing.py) on the MI355X: the same cases and the same oracle references as
tests/test_grazing_host.py, tolerance 0, through every kernel family that walks a tree -- mega_gen_kernel, wf_trav_gen,
mega_kernel (MORT_NO_GEN=1 and beyond the tree's reach), feat_kernel in both forms, and for the reference-BVH world
mega_bvh_kernel at both workgroup sizes, wf_trav, the general kernel and feat_kernel.  Frames are 65 x 65 at 1 spp: every lane of
every wave holds a grazing ray.  A group of cases shares one world, uploaded once per kernel choice."""
import pytest

from mort_amd import hip, structs as S
from tests import grazing as G
from tests.feature_ref import assert_same_words
from tests.test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _tree_kernel_for_every_world(monkeypatch):
    monkeypatch.setenv("MORT_GEN_MIN_PRIMS", "0")  # as tests/test_gpu_gen.py: the medium-only world has no 48 solids


def _frame(ctx, cam, oracle, mode=hip.MODE_MEGA):
    """one frame of the world the context holds, from freshly seeded streams (render_gpu of tests/test_gpu_parity.py without its upload)"""
    ctx.rng_seed(S.DEFAULT_SEED, cam.image_width, cam.image_height)
    out = ctx.render(cam, mode=mode, want_accum=True, want_segments=True)
    out["states"] = ctx.rng_store(cam.image_width, cam.image_height, oracle.STATE_DTYPE)
    return out


def _refs(cases):
    refs = [G.reference(c) for c in cases]
    for case, (_, cam, feat, _) in zip(cases, refs):
        G.check_conditions(case, cam, feat)
    return refs


@pytest.mark.parametrize("group", [g for g in G.GROUPS if not g.startswith("bvh")])
def test_flat_grazing_cases_on_the_gpu(gpu_ctx, oracle, monkeypatch, group):
    cases = [c for c in G.FLAT if c.group == group]
    refs = _refs(cases)
    world = refs[0][0]
    assert all(r[0] is world for r in refs)
    gpu_ctx.set_partition(0, 1, 8)
    gpu_ctx.upload_world(world)
    for case, (_, cam, feat, ren) in zip(cases, refs):
        out = _frame(gpu_ctx, cam, oracle)
        name = out["stats"]["kernel_name"]
        assert name.startswith("mega_gen_kernel<" if case.walk == "tree" else "mega_kernel"), f"{case}: {name}"
        assert_same(out, ren)
        if "zero" in case.cond and case.walk == "tree":
            assert out["stats"]["reference_walks"] > 0, f"{case}: rays with a zero component go to the reference's scan"
        if case.walk == "tree":  # beyond the tree's reach the wavefront mode has no kernel
            out = _frame(gpu_ctx, cam, oracle, mode=hip.MODE_WAVE)
            assert out["stats"]["kernel_name"].startswith("wf_trav_gen"), f"{case}: {out['stats']['kernel_name']}"
            assert_same(out, ren)
        assert_same_words(gpu_ctx.render_features(cam), feat, f"{case}, feat_kernel over the unified tree")
    monkeypatch.setenv("MORT_NO_GEN", "1")  # read when the world is uploaded
    gpu_ctx.upload_world(world)
    monkeypatch.delenv("MORT_NO_GEN")
    for case, (_, cam, feat, ren) in zip(cases, refs):
        out = _frame(gpu_ctx, cam, oracle)
        assert out["stats"]["kernel_name"] == "mega_kernel", f"{case}: {out['stats']['kernel_name']}"
        assert_same(out, ren)
        assert_same_words(gpu_ctx.render_features(cam), feat, f"{case}, feat_kernel over the item scan")


@pytest.mark.parametrize("group", [g for g in G.GROUPS if g.startswith("bvh")])
def test_bvh_grazing_cases_on_the_gpu(gpu_ctx, oracle, monkeypatch, group):
    cases = [c for c in G.BVH if c.group == group]
    refs = _refs(cases)
    world = refs[0][0]
    gpu_ctx.set_partition(0, 1, 8)
    gpu_ctx.upload_world(world)
    for case, (_, cam, feat, ren) in zip(cases, refs):
        out = _frame(gpu_ctx, cam, oracle)
        name = out["stats"]["kernel_name"]
        assert name.startswith("mega_bvh_kernel<") and not name.startswith("mega_bvh_kernel<1024"), f"{case}: {name}"
        assert_same(out, ren)
        out = _frame(gpu_ctx, cam, oracle, mode=hip.MODE_WAVE)
        assert out["stats"]["kernel_name"].startswith("wf_trav<"), f"{case}: {out['stats']['kernel_name']}"
        assert_same(out, ren)
        assert_same_words(gpu_ctx.render_features(cam), feat, f"{case}, feat_kernel")
    for env, want in (("MORT_FAST_BLOCK_SIZE", "mega_bvh_kernel<1024,"), ("MORT_FORCE_GENERIC", "mega_kernel")):
        monkeypatch.setenv(env, "1024" if env == "MORT_FAST_BLOCK_SIZE" else "1")
        for case, (_, cam, feat, ren) in zip(cases, refs):
            out = _frame(gpu_ctx, cam, oracle)
            assert out["stats"]["kernel_name"].startswith(want), f"{case}: {out['stats']['kernel_name']}"
            assert_same(out, ren)
        monkeypatch.delenv(env)
