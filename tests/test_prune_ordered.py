"""The box step's sign-ordered slab test (mega_bvh.h own_prune_ordered on DNode4's [min, max, min] pieces) against the
unordered one it replaces (own_prune), on the host: both are __host__ __device__, and the hook addresses the pieces as
the kernel does.  Over the real four-wide trees of Scenes 1 and 10 and more than 10^6 rays -- all eight sign octants,
directions with one or two tiny components, origins inside, on and far outside the boxes, finite and infinite
`closest` -- every occupied child must get the same entry distance, bit for bit, and the same skip decision.
No tolerance: the walk has to be the same walk step for step."""
import ctypes as C

import numpy as np
import pytest

from mort_amd import hip, host

RAYS = 1_048_576


def _hooks():
    L = hip.lib()
    boxes = L.mort_hip_debug_own_tree4_boxes
    boxes.restype = C.c_int
    boxes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    forms = L.mort_hip_debug_prune_forms
    forms.restype = C.c_int
    forms.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_ulonglong)]
    return boxes, forms


def _rays(boxes, n, seed):
    """n x 7 float32: origin, direction, closest."""
    rng = np.random.default_rng(seed)
    b = boxes[rng.integers(0, len(boxes), n)].astype(np.float64)
    lo, hi = b[:, 0::2], b[:, 1::2]
    ext = np.maximum(hi - lo, 1e-3)
    u = rng.random((n, 3))
    where = rng.integers(0, 4, n)
    inside = lo + u * (hi - lo)
    # on the box: one to three coordinates exactly on a plane (the float32 value the node stores)
    on = inside.copy()
    snap = rng.random((n, 3)) < 0.5
    snap[np.arange(n), rng.integers(0, 3, n)] = True
    on[snap] = np.where(rng.random((n, 3)) < 0.5, lo, hi)[snap]
    near = lo + (u * 3.0 - 1.0) * ext                                         # around the box, within one extent
    far = (lo + hi) * 0.5 + rng.standard_normal((n, 3)) * ext * 10.0 ** rng.uniform(1, 4, (n, 1))
    o = np.select([where[:, None] == 0, where[:, None] == 1, where[:, None] == 2], [inside, on, near], far)
    # directions: every octant equally often; a third of them with one tiny component, a third with two
    d = rng.uniform(0.05, 1.0, (n, 3)) * np.where((np.arange(n)[:, None] >> np.arange(3)) & 1, -1.0, 1.0)
    tiny = 10.0 ** rng.uniform(-14.5, -4, (n, 3))
    kind = rng.integers(0, 3, n)
    order = np.argsort(rng.random((n, 3)), axis=1)
    ntiny = np.where(kind == 0, 0, kind)[:, None]                              # 0, 1 or 2 tiny components
    mask = np.zeros((n, 3), bool)
    np.put_along_axis(mask, order[:, :1], ntiny >= 1, axis=1)
    np.put_along_axis(mask, order[:, 1:2], ntiny >= 2, axis=1)
    d = np.where(mask, np.sign(d) * tiny, d)
    d *= 10.0 ** rng.uniform(-2, 2, (n, 1))                                  # scattered rays are not unit vectors
    # closest: infinite for half the rays, else somewhere around the box's distance (so that `key > closest` decides both ways)
    dist = np.linalg.norm((lo + hi) * 0.5 - o, axis=1) / np.linalg.norm(d, axis=1)
    closest = np.where(rng.random(n) < 0.5, np.inf, (dist + 1e-3) * 10.0 ** rng.uniform(-1, 1, n))
    return np.ascontiguousarray(np.concatenate([o, d, closest[:, None]], axis=1), dtype=np.float32)


@pytest.mark.parametrize("scene", [1, 10])
def test_ordered_planes_give_the_same_walk(scene):
    boxes_fn, forms_fn = _hooks()
    world, _ = host.build_scene(scene, width=64, spp=1)
    wp = C.cast(world.ptr, C.c_void_p)
    nb = boxes_fn(wp, None, 0)
    assert nb >= 8, nb
    boxes = np.zeros((nb, 6), np.float32)
    assert boxes_fn(wp, boxes.ctypes.data_as(C.c_void_p), nb) == nb
    assert (boxes[:, 0::2] <= boxes[:, 1::2]).all()                            # the builder's min <= max
    rays = _rays(boxes, RAYS, 1000 + scene)
    out = (C.c_ulonglong * 16)()
    stride = 1                                                                 # every ray meets every node
    assert forms_fn(wp, rays.ctypes.data_as(C.c_void_p), len(rays), stride, out) == 0
    pairs, te_diff, skip_diff, left_out, n4, dirty_slots, both_skip = list(out)[:7]
    octants = list(out)[8:16]
    print(f"scene {scene}: {n4} four-wide nodes, {nb} boxes, stride {stride}, rays compared {sum(octants)} (left out {left_out}), "
          f"pairs {pairs}, skipped by both {both_skip}, te mismatches {te_diff}, skip mismatches {skip_diff}, per octant {octants}")
    assert dirty_slots == 0                                                    # unused child slots are all zero, third piece included
    assert sum(octants) >= 1_000_000 and min(octants) >= 100_000
    assert left_out < RAYS // 20                                               # (tiny components below 1e-15 never reach the box step)
    assert pairs == nb * sum(octants)
    assert both_skip >= 1_000_000 and pairs - both_skip >= 1_000_000           # the rays do both: miss boxes and enter them
    assert te_diff == 0 and skip_diff == 0
