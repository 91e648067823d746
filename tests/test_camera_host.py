"""The camera layer on the CPU: the two ends of Camera::render, each against its own reference.

1. mort_camera_initialize and mort_camera_input (mort_host.c) against the reference's own Camera::initialize, rotate_around and a
   restatement of input() over its operators (oracle/ref_render.cpp: mort_ref_camera_initialize / _rotate_around / _camera_input), word for
   word over every float and int field of mort_camera, on tests/camera_cases.py's cameras() and inputs().  The one thing that cannot be
   compared is libm: the host forms tan as (float)(mort_sin / mort_cos) in double, the reference calls tan(float).  Every case
   is classified by whether the libm values it uses agree (mort_ref_libm against the host's expression, restated over mort_sin / mort_cos
   through mort_oracle_math_batch): where they agree every word is equal; where one tan differs, every field that this tan does not reach
   is still equal to the bit, with no tolerance set for the rest.  At most 15 % of the cameras and of the ticks may be of the second kind.
2. get_ray: hipcc's host compile of both instantiations (mort_hip_debug_camera_host fn 0, fn 1) == the oracle (mort_oracle_camera_batch)
   == a numpy restatement over tests/math_restate.py, 2^18 records, tolerance 0; the branch census is asserted on the oracle's answers.
3. The pixel's finish (fn 2): host compile == oracle == the definition (NaN -> 0, correctly rounded root, clamp, x256, truncate; alpha 255).

Measured with glibc's tanf: tan(theta / 2) differs from the host's form in 160 of the 3037 cameras, the defocus tangent in 168 (every one
a defocus_angle of 180), either in 321 (10.57 %); 93 of the 1440 input ticks (6.46 %); none of the ten scenes' cameras.  What the sweep
found: mort_sin(-0.0) is +0, so a defocus_angle of -0 gave the disk vectors the opposite zero signs to the reference's tan(-0) = -0;
host_tanf now returns +-0 for +-0.  Slips tried in a scratch copy: a float add of y and the offset in get_ray fails 7079 records, < for <=
in the defocus test 74097, a rounded byte 183151 pixel records, viewport_width kept in float 126 cameras; 0.999f widened to double fails
nothing and cannot (no float lies between 0.999 and 0.999f; 256 v is exact in either width)."""
import ctypes as C

import numpy as np
import pytest

from mort_amd import host, hip
from tests import camera_cases as CC
from tests import math_cases as MC
from tests import oracle_lib as O
from tests import ref_lib as RL

F, D, U = np.float32, np.float64, np.uint32


@pytest.fixture(scope="module")
def ref():
    if not RL.ensure_built():
        pytest.skip("neither the reference tree nor oracle/_ref/libmort_ref.so is here")
    return RL.lib()


# ---------------------------------------------------------------- libm: what the host computes and what the reference calls
def _host_trig(x):
    """(tan, cos, sin) of float32 x as mort_host.c forms them: (float)(mort_sin / mort_cos) with tan(+-0) = +-0, (float)mort_cos,
    (float)mort_sin of the double"""
    x32 = np.ascontiguousarray(x, F)
    x = x32.astype(D)
    s = O.math_batch(MC.FN["sin"], x).view(D)[:, 0]
    c = O.math_batch(MC.FN["cos"], x).view(D)[:, 0]
    with np.errstate(all="ignore"):
        return np.where(x32 == 0, x32, (s / c).astype(F)).astype(F), c.astype(F), s.astype(F)


def _agree(ref, fn, x):
    """per element of float32 x: does the reference's libm value equal the host's expression (any NaN equals any NaN)"""
    x = np.ascontiguousarray(x, F)
    mine = _host_trig(x)[fn]
    theirs = np.array([ref.mort_ref_libm(fn, float(v)) for v in x], F)
    return (mine.view(U) == theirs.view(U)) | (np.isnan(mine) & np.isnan(theirs))


def _radians(deg):
    """degrees_to_radians (utils.h:21,25-27): float pi, the division in double"""
    return (np.asarray(deg, F) * F(3.1415926535897932385)).astype(D) / 180.0


def _tan_args(cams):
    theta = _radians(cams["vfov"].astype(F)).astype(F)
    return theta / F(2), _radians(cams["defocus_angle"] / F(2)).astype(F)


def _canon_words(cams, fields):
    """the words of `fields`, every float NaN as one pattern"""
    cols = []
    for name in fields:
        a = np.ascontiguousarray(cams[name]).reshape(len(cams), -1)
        if name in CC.FLOAT_FIELDS:
            w = a.view(U).copy()
            w[np.isnan(a)] = 0x7fc00000
        else:
            w = a.view(U)
        cols.append(w)
    return np.concatenate(cols, 1)


def _differing(a, b, fields):
    return np.flatnonzero((_canon_words(a, fields) != _canon_words(b, fields)).any(1))


ALL_FIELDS = CC.FLOAT_FIELDS + CC.INT_FIELDS


def _comparable(vfov_ok, defocus_ok):
    return CC.LIBM_FREE + (CC.VFOV_TAN if vfov_ok else ()) + (CC.DEFOCUS_TAN if defocus_ok else ())


def _assert_equal_where_comparable(mine, theirs, vfov_ok, defocus_ok, what):
    assert set(_comparable(True, True)) == set(ALL_FIELDS)
    for vo in (True, False):
        for do in (True, False):
            rows = np.flatnonzero((vfov_ok == vo) & (defocus_ok == do))
            if not len(rows):
                continue
            bad = _differing(mine[rows], theirs[rows], _comparable(vo, do))
            if len(bad):
                i = rows[bad[0]]
                names = [n for n in _comparable(vo, do) if len(_differing(mine[i: i + 1], theirs[i: i + 1], (n,)))]
                raise AssertionError(f"{what}: {len(bad)} cameras differ from the reference (tan agrees: vfov {vo}, defocus {do}); first {i}: fields {names}; "
                                     f"input {[(n, mine[n][i].tolist()) for n in CC.INPUT_FIELDS]}; ours {[mine[n][i].tolist() for n in names]}; reference {[theirs[n][i].tolist() for n in names]}")


def test_camera_initialize_equals_the_reference(ref):
    cams, fam = CC.cameras()
    mine = CC.initialized()
    theirs = CC.apply(ref.mort_ref_camera_initialize, cams.copy())
    a_v, a_d = _tan_args(cams)
    vfov_ok, defocus_ok = _agree(ref, 0, a_v), _agree(ref, 0, a_d)
    other = ~(vfov_ok & defocus_ok)
    print(f"cameras {len(cams)}: tan(theta / 2) differs from the host's form in {int((~vfov_ok).sum())}, tan(radians(defocus_angle / 2)) in {int((~defocus_ok).sum())}, "
          f"either in {int(other.sum())} ({100.0 * other.mean():.2f} %)")
    scenes = np.flatnonzero(other[fam["scenes"]])
    print("scene cameras whose tan differs:", [int(k) + 1 for k in scenes] or "none")
    _assert_equal_where_comparable(mine, theirs, vfov_ok, defocus_ok, "mort_camera_initialize")
    assert other.mean() <= 0.15
    nan_w = np.isnan(mine["w"]).any(1)
    assert nan_w[fam["w_nan"]].all() and np.isnan(mine["u"][fam["u_nan"]]).any(1).all() and not nan_w[fam["scenes"]].any()
    assert np.isinf(mine["recip_sqrt_spp"][cams["samples_per_pixel"] == 0]).all() and (cams["samples_per_pixel"] == 0).sum() >= 3
    assert {1, 65536} <= set(mine["image_height"].tolist()) and (mine["image_height"] == mine["image_width"]).any()


def test_rotate_around_equals_the_reference(ref):
    """the host's rotate_around is static: it is reached through mort_camera_input with one mouse axis, which turns lookat - lookfrom about
    vup (dx) or u (dy); the reference's own function on the same vectors must give the same lookat.  Angles: -d / 500 for every mouse delta
    of the chains (+-1 ... +-1571, 2^20) and two more, on 256 cameras; a turn whose cos or sin libm gives differently is left out (at
    most 15 %: none where the reference's cos and sin go through mort_math.h)"""
    cams, fam = CC.cameras()
    init = CC.initialized()
    rows = np.arange(fam["random"].start, fam["random"].start + 256)
    DELTAS = tuple(d for d in CC.MOUSE if d) + (7, -311)          # every delta of the input chains, about either axis in turn
    fp = C.POINTER(C.c_float)
    differ = compared = 0
    for i in rows:
        for k, d in enumerate(DELTAS):
            axis, (dx, dy) = ("vup", (d, 0)) if (i + k) % 2 == 0 else ("u", (0, d))
            cam = init[i: i + 1].copy()
            theta = F(-(dx or dy) / 500.0)
            if not (_agree(ref, 1, [theta])[0] and _agree(ref, 2, [theta])[0]):
                continue
            vec = (cam["lookat"][0] - cam["lookfrom"][0]).astype(F)
            ax = np.ascontiguousarray(cam[axis][0], F)
            out = np.zeros(3, F)
            ref.mort_ref_rotate_around(vec.ctypes.data_as(fp), ax.ctypes.data_as(fp), float(theta), out.ctypes.data_as(fp))
            want = (cam["lookfrom"][0] + out).astype(F)
            CC.apply(host.lib().mort_camera_input, cam, 0, dx, dy, 1)
            compared += 1
            same = (cam["lookat"][0].view(U) == want.view(U)) | (np.isnan(cam["lookat"][0]) & np.isnan(want))
            differ += int(not same.all())
    print(f"rotate_around: {compared} turns compared of {len(rows) * len(DELTAS)}")
    assert compared >= len(rows) * len(DELTAS) * 85 // 100 and differ == 0


def test_camera_input_equals_the_reference(ref):
    cams, _ = CC.cameras()
    init = CC.initialized()
    chains = CC.inputs()
    ticks = other = 0
    keys_seen, dx_seen, dy_seen, left_seen, lengths = set(), set(), set(), set(), set()
    for ci, chain in chains:
        mine, theirs = init[ci: ci + 1].copy(), init[ci: ci + 1].copy()
        CC.apply(ref.mort_ref_camera_initialize, theirs)
        a_v, a_d = _tan_args(mine)
        vfov_ok, defocus_ok = _agree(ref, 0, a_v), _agree(ref, 0, a_d)
        diverged = False
        lengths.add(len(chain))
        for t, (keys, dx, dy, left) in enumerate(chain):
            keys_seen.add(keys); dx_seen.add(dx); dy_seen.add(dy); left_seen.add(left)
            ticks += 1
            angles = [F(-d / 500.0) for d in (dx, dy) if left and d]
            trig_ok = all(_agree(ref, 1, [a])[0] and _agree(ref, 2, [a])[0] for a in angles)
            if diverged or not trig_ok:              # the mouse angle's cos or sin differs: lookat differs from here on
                diverged = True
                other += 1
                continue
            CC.apply(host.lib().mort_camera_input, mine, keys, dx, dy, left)
            CC.apply(ref.mort_ref_camera_input, theirs, keys, dx, dy, left)
            other += int(not (vfov_ok[0] and defocus_ok[0]))
            _assert_equal_where_comparable(mine, theirs, vfov_ok, defocus_ok, f"mort_camera_input, camera {ci}, tick {t} of {chain}")
    print(f"input chains {len(chains)}, ticks {ticks}: libm differs in {other} ({100.0 * other / ticks:.2f} %)")
    assert other <= 0.15 * ticks
    assert keys_seen == set(range(16)) and dx_seen == set(CC.MOUSE) and dy_seen == set(CC.MOUSE) and left_seen == {0, 1} and lengths == set(range(1, 9))


# ---------------------------------------------------------------- get_ray and the pixel's finish, record by record
def test_get_ray_host_compile_equals_the_oracle_and_the_restatement():
    rec, census = CC.ray_records()
    MC.assert_census(0, census)
    want = CC.oracle(0)
    cen = CC.ray_census(rec, want)
    print("get_ray census:", cen)
    CC.assert_ray_census(cen, len(rec))
    CC.assert_same(0, rec, dict(oracle=want, hipcc_host_args=hip.debug_camera_host(0, rec).reshape(len(rec), -1),
                                hipcc_host_view=hip.debug_camera_host(1, rec).reshape(len(rec), -1), numpy=CC.restate_get_ray(rec)))


def test_pixel_finish_host_compile_equals_the_oracle_and_the_definition():
    rec, census = CC.pixel_records()
    want = CC.oracle(2)
    cen = CC.pixel_census(rec, want)
    print("pixel census:", census, cen)
    CC.assert_pixel_census(cen)
    CC.assert_same(2, rec, dict(oracle=want, hipcc_host=hip.debug_camera_host(2, rec).reshape(len(rec), -1), definition=CC.define_pixel(rec)))
    assert ((want[:, 3] >> U(24)) == 255).all()


def test_camera_shapes_and_refusals():
    assert hip.CAMERA_SHAPES == O.CAMERA_SHAPES
    fn = hip.lib().mort_hip_debug_camera_shape
    fn.restype = C.c_int; fn.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    a, b = C.c_int(), C.c_int()
    for k, shape in enumerate(hip.CAMERA_SHAPES):
        assert fn(k, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == shape
    assert fn(3, C.byref(a), C.byref(b)) != 0 and fn(-1, C.byref(a), C.byref(b)) != 0
    with pytest.raises(hip.MortHipError):
        hip.debug_camera_host(3, np.zeros((1, 30), U))
    with pytest.raises(O.OracleBatchError):
        _bad_oracle_fn()


def _bad_oracle_fn():
    f = O.lib().mort_oracle_camera_batch
    f.restype = C.c_int; f.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
    buf = np.zeros(30, U)
    rc = f(3, buf.ctypes.data, 1, buf.ctypes.data, 1)
    if rc != 0:
        raise O.OracleBatchError(rc, "mort_oracle_camera_batch")
