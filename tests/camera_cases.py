"""Inputs of the camera sweep, seeded and deterministic:

  cameras() / inputs()  the CAMERAS as their input fields, and the INPUTS: chains of input() ticks on some of them, for
                     mort_camera_initialize and mort_camera_input against the reference's own functions (tests/test_camera_host.py);
  ray_records()      2^18 records of get_ray in the layout of debug.hip's camera table (fn 0 and 1), with streams whose first four outputs
                     are chosen: each step's new v4 is an invertible xorshift of the old first word, so v0..v3 can be solved for;
  pixel_records()    2^18 records of the pixel's finish (fn 2): sums whose scaled value lands on and beside every byte boundary.

A camera travels as CAM_WORDS 32-bit words, the bytes of mort_camera."""
import ctypes as C
import functools

import numpy as np

from mort_amd import host, structs as S
from tests import math_cases as MC
from tests import math_restate as R
from tests import oracle_lib as O

F, D, U = np.float32, np.float64, np.uint32
N_RAY = 1 << 18
N_PIXEL = 1 << 18
RAGGED = MC.RAGGED
NAMES = ("get_ray", "get_ray_lds", "pixel_finish")


def _cam_dtype():
    names, formats, offsets = [], [], []
    for name, typ in S.Camera._fields_:
        names.append(name)
        formats.append({C.c_float: "<f4", C.c_int: "<i4", C.c_void_p: "<u8", S.Vec3: ("<f4", (3,))}[typ])
        offsets.append(getattr(S.Camera, name).offset)
    return np.dtype(dict(names=names, formats=formats, offsets=offsets, itemsize=C.sizeof(S.Camera)))


CAM_DTYPE = _cam_dtype()
CAM_WORDS = CAM_DTYPE.itemsize // 4
INPUT_FIELDS = ("aspect_ratio", "image_width", "samples_per_pixel", "vfov", "lookfrom", "lookat", "vup", "defocus_angle", "focus_dist")
FLOAT_FIELDS = tuple(n for n in CAM_DTYPE.names if CAM_DTYPE[n].base == np.dtype("<f4"))
INT_FIELDS = tuple(n for n in CAM_DTYPE.names if CAM_DTYPE[n] == np.dtype("<i4"))
# what neither tan nor the mouse angles' cos and sin reach (camera.cuh:48-55, 64-66)
LIBM_FREE = ("aspect_ratio", "image_width", "image_height", "samples_per_pixel", "pixel_samples_scale", "sqrt_spp", "recip_sqrt_spp", "bounce_limit",
             "vfov", "background", "light_obj_type", "light_obj_idx", "center", "lookfrom", "lookat", "vup", "v", "u", "w", "defocus_angle", "focus_dist")
VFOV_TAN = ("pixel00_loc", "pixel_delta_u", "pixel_delta_v")     # reached by tan(theta / 2) alone
DEFOCUS_TAN = ("defocus_disk_u", "defocus_disk_v")               # reached by tan(radians(defocus_angle / 2)) alone

WIDTHS = (1, 2, 7, 1200, 4096, 65535, 65536)
SPPS = (1, 2, 3, 4, 5, 99, 100, 101, 500, 1 << 30, 0)
DEFOCUS = (0.0, -0.0, -1.0, 1e-3, 0.6, 2.5, 90.0, 179.0, 180.0)
MOUSE = (0, 1, -1, 6, -6, 500, -500, 1571, -1571, 1 << 20)


def _blank(n):
    c = np.zeros(n, CAM_DTYPE)
    c["aspect_ratio"] = 1.0; c["image_width"] = 100; c["samples_per_pixel"] = 100; c["bounce_limit"] = 10; c["vfov"] = 90
    c["background"] = (0.7, 0.8, 1.0); c["light_obj_type"] = -1
    c["lookfrom"] = (0, 0, 1); c["vup"] = (0, 1, 0); c["focus_dist"] = 10
    return c


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


@functools.lru_cache(None)
def scene_cameras():
    """the ten scenes' cameras as the scenes leave them (input fields; the rest is recomputed by whoever initialises)"""
    out = np.zeros(10, CAM_DTYPE)
    for k in range(10):
        _, cam = host.build_scene(k + 1)
        out[k] = np.frombuffer(bytes(cam), CAM_DTYPE)[0]
    return out


@functools.lru_cache(None)
def cameras():
    """(cameras as a CAM_DTYPE array with the input fields set, {family: slice})"""
    rng = np.random.default_rng(20261)
    parts, fam = [], {}

    def add(name, c):
        at = sum(len(p) for p in parts)
        fam[name] = slice(at, at + len(c))
        parts.append(c)

    sc = scene_cameras().copy()
    add("scenes", sc)
    for name, base in (("vfov_axis", _blank(1)[0]), ("vfov_scene1", sc[0]), ("vfov_scene9", sc[8])):
        c = np.repeat(np.array([base]), 179)
        c["vfov"] = np.arange(1, 180)
        add(name, c)
    c = np.repeat(_blank(1), 3 * len(WIDTHS))
    for i, w in enumerate(WIDTHS):
        c["image_width"][3 * i: 3 * i + 3] = w
        c["aspect_ratio"][3 * i: 3 * i + 3] = (F(w), 1.0, F(2.0) * F(w))     # height 1 exactly, height = width, height clamped up to 1
    add("aspect", c)
    c = np.repeat(_blank(1), 6)
    c["image_width"] = 1
    c["aspect_ratio"] = (1.0, 0.5, 1.0 / 7, 1.0 / 1200, 1.0 / 4096, 1.0 / 65536)       # width 1, heights 1 .. 65536
    add("width_one", c)
    c = np.repeat(sc[:3], len(SPPS))
    c["samples_per_pixel"] = np.tile(SPPS, 3)
    add("spp", c)
    c = np.repeat(sc[:2], 49)
    c["focus_dist"] = np.tile(np.logspace(-6, 6, 49), 2)
    c["defocus_angle"] = 0.6
    add("focus", c)
    c = np.repeat(sc[:4], len(DEFOCUS))
    c["defocus_angle"] = np.tile(DEFOCUS, 4)
    add("defocus", c)
    n = 200
    c = _blank(n)
    c["lookfrom"] = (_unit(rng, n) * 1e6 + rng.uniform(-50, 50, (n, 3)))
    c["lookat"] = c["lookfrom"].astype(D) + _unit(rng, n) * np.where(np.arange(n) % 2 == 0, 1.0, 1e6)[:, None]
    c["vfov"] = rng.integers(1, 180, n)
    add("far", c)
    n = 24
    c = _blank(n)
    c["lookfrom"] = rng.uniform(-20, 20, (n, 3))
    c["lookat"] = c["lookfrom"]
    add("w_nan", c)
    c = _blank(n)
    c["lookfrom"] = rng.uniform(-20, 20, (n, 3))
    d = np.array([(0, 1, 0), (0, -1, 0), (1, 0, 0), (0, 0, -3)], D)[np.arange(n) % 4]
    c["lookat"] = c["lookfrom"].astype(D) - d * 4            # w is d's direction, exactly
    c["vup"] = d * np.array([1, -1, 2.5, 1e-3, 1e10, -7])[np.arange(n) % 6][:, None]
    add("u_nan", c)
    n = 2048
    c = _blank(n)
    c["lookfrom"] = rng.uniform(-20, 20, (n, 3))
    c["lookat"] = rng.uniform(-20, 20, (n, 3))
    c["vup"] = _unit(rng, n) * np.array([1, -1, 2.5, 1e-3, 1e10, -7])[np.arange(n) % 6][:, None]
    c["vup"][::5] = (0, 1, 0)
    c["vfov"] = rng.integers(1, 180, n)
    c["image_width"] = np.array(WIDTHS)[rng.integers(0, len(WIDTHS), n)]
    c["aspect_ratio"] = np.array([1.0, 16.0 / 9.0, 0.5, 2.39], F)[rng.integers(0, 4, n)]
    c["samples_per_pixel"] = np.array(SPPS)[rng.integers(0, len(SPPS), n)]
    c["defocus_angle"] = np.array(DEFOCUS + (0.0, 0.6, 2.5), F)[rng.integers(0, len(DEFOCUS) + 3, n)]
    c["focus_dist"] = 10.0 ** rng.uniform(-6, 6, n)
    add("random", c)
    return np.concatenate(parts), fam


def words(cams):
    return np.ascontiguousarray(cams).view(U).reshape(len(cams), CAM_WORDS)


def apply(fn, cams, *args):
    """fn(mort_camera *, *args) on every camera of a CAM_DTYPE array, in place; returns the array"""
    w = words(cams)
    for i in range(len(w)):
        fn(C.byref(S.Camera.from_buffer(w[i])), *args)
    return cams


@functools.lru_cache(None)
def initialized():
    """CAMERAS through the library's mort_camera_initialize"""
    cams = cameras()[0].copy()
    fn = host.lib().mort_camera_initialize
    return apply(fn, cams)


@functools.lru_cache(None)
def inputs():
    """chains of input() ticks: [(camera index, [(keys, dx, dy, left), ...])] over 320 of the random cameras; every subset of W/A/S/D, every
    delta of MOUSE on either axis, the button up and down, 1 to 8 ticks"""
    rng = np.random.default_rng(20262)
    cams, fam = cameras()
    pool = np.arange(fam["random"].start, fam["random"].stop)
    ok = np.isfinite(initialized()["pixel00_loc"][pool]).all(1) & (cams["defocus_angle"][pool] != 180)    # tan at pi / 2: libm's least comparable value, left to cameras()
    pool = pool[ok][:320]
    chains = []
    for i, ci in enumerate(pool):
        ticks = []
        for t in range(1 + i % 8):
            keys = (i + 5 * t) % 16
            dx = MOUSE[(i + 3 * t) % len(MOUSE)]
            dy = MOUSE[(i // len(MOUSE) + 7 * t) % len(MOUSE)]
            left = 0 if (i + t) % 5 == 0 else 1
            ticks.append((keys, dx, dy, left))
        chains.append((int(ci), ticks))
    return chains


# ---- streams with chosen outputs ----
def _inv_f(y):
    """x with f(x) == y for XORWOW's f(x) = t ^ (t << 1), t = x ^ (x >> 2)"""
    t = y.astype(U).copy()
    for s in (1, 2, 4, 8, 16):
        t ^= t << U(s)
    x = t
    for s in (2, 4, 8, 16):
        x = x ^ (x >> U(s))
    return x


def _g(x):
    return x ^ (x << U(4))


def forced_states(rng, want):
    """(n, 6) states whose first four outputs are want (n, 4)"""
    n = len(want)
    st = rng.integers(0, 1 << 32, (n, 6), dtype=np.uint64).astype(U)
    want = want.astype(U)
    prev = st[:, 5]
    for k in range(4):
        target = want[:, k] - st[:, 0] - U(362437 * (k + 1))          # the new v4 this output needs
        st[:, 1 + k] = _inv_f(target ^ _g(prev))
        prev = target
    chk = st.copy()
    for k in range(4):
        assert (MC.xorwow_step(chk) == want[:, k]).all()
    return st


def _word_of(rf):
    """the generator output whose random_float is nearest rf in [0, 1]: random_float = 1 - (x * 2^-32 + 2^-33)"""
    x = np.rint((1.0 - np.asarray(rf, D)) * 4294967296.0 - 0.5)
    return np.clip(x, 0, 4294967295).astype(np.uint64).astype(U)


def _circle_words(rng, n):
    """outputs three and four (the disk's first point) on and just outside or inside the unit circle: p = 2 * random_float - 1 per axis"""
    ang = rng.uniform(0, 2 * np.pi, n)
    ang[: n // 8] = (np.arange(n // 8) % 8) * (np.pi / 4)              # the axes and diagonals: (1, 0) itself is on the circle
    wx = _word_of((np.cos(ang) + 1) / 2)
    px = (1.0 - (wx.astype(F) * F(2.3283064e-10) + F(2.3283064e-10) / F(2.0)).astype(D)).astype(F) * F(2) + F(-1)     # px as random_float_range(-1, 1) forms it from that word
    py = np.sqrt(np.maximum(0.0, 1.0 - px.astype(D) ** 2)) * np.where(np.sin(ang) < 0, -1.0, 1.0)
    wy = _word_of((py + 1) / 2).astype(np.int64) + rng.integers(-4, 5, n) * 128          # a few float steps either way
    return wx, np.clip(wy, 0, 4294967295).astype(np.uint64).astype(U)


def _with_nonfinite(rng, v, share):
    """one component of some rows +inf, -inf or NaN"""
    v = v.copy()
    rows = np.flatnonzero(rng.random(len(v)) < share)
    v[rows, rng.integers(0, v.shape[1], len(rows))] = np.array([np.inf, -np.inf, np.nan], F)[rng.integers(0, 3, len(rows))]
    return v


@functools.lru_cache(None)
def ray_records():
    """((N_RAY, 30) uint32 records, census of the inputs)"""
    rng = np.random.default_rng(20263)
    n = N_RAY
    st, census = MC._states(rng, n)
    m = 1 << 11
    lo, hi = np.zeros(m, U), np.full(m, 0xffffffff, U)                   # random_float 1 and 0
    rnd = lambda: rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(U)
    fams = [np.stack([lo, rnd(), rnd(), rnd()], 1), np.stack([hi, rnd(), rnd(), rnd()], 1), np.stack([rnd(), lo, rnd(), rnd()], 1),
            np.stack([rnd(), hi, rnd(), rnd()], 1), np.stack([lo, hi, rnd(), rnd()], 1), np.stack([hi, lo, rnd(), rnd()], 1),
            np.stack([lo, lo, lo, lo], 1), np.stack([hi, hi, hi, hi], 1)]
    n_circle = 1 << 14
    wx, wy = _circle_words(rng, n_circle)
    fams.append(np.stack([rng.integers(0, 1 << 32, n_circle, dtype=np.uint64).astype(U), rng.integers(0, 1 << 32, n_circle, dtype=np.uint64).astype(U), wx, wy], 1))
    want = np.concatenate(fams)
    forced = slice(n - len(want), n)
    circle = slice(n - n_circle, n)
    st[forced] = forced_states(rng, want)

    rec = np.zeros((n, 30), U)
    rec[:, 0:6] = st
    edge_xy = np.array([0, 1, (1 << 16) - 1, 1 << 16, (1 << 24) - 1, (1 << 24) + 1, (1 << 31) - 1], np.int64)
    for col in (6, 7):
        small = rng.integers(0, 4096, n)
        rec[:, col] = np.where(rng.random(n) < 0.5, small, edge_xy[rng.integers(0, len(edge_xy), n)]).astype(np.int32).view(U)
    sq = np.array([1, 2, 22, 181, 32767, 32768, 0, 10], np.int64)[rng.integers(0, 8, n)]
    sq[rng.random(n) < 0.25] = 10
    with np.errstate(divide="ignore"):
        rec[:, 10] = (1.0 / sq.astype(D)).astype(F).view(U)              # (float)(1.0 / sqrt_spp): inf for 0
    top = np.maximum(sq - 1, 0)
    for col in (8, 9):
        pick = rng.integers(0, 3, n)
        rec[:, col] = np.select([pick == 0, pick == 1], [0, top], rng.integers(0, 1 << 30, n) % np.maximum(sq, 1)).astype(np.int32).view(U)
    angles = np.array([0.0, -0.0, -1.0, 1e-40, 1e-30, 0.6, np.inf, np.nan, 0.0, 0.6], F)
    da = angles[rng.integers(0, len(angles), n)]
    da[circle] = F(0.6)
    rec[:, 11] = da.view(U)

    cams = initialized()
    pick = rng.integers(0, len(cams), n)
    vec = np.concatenate([cams[k][pick] for k in ("center", "pixel00_loc", "pixel_delta_u", "pixel_delta_v", "defocus_disk_u", "defocus_disk_v")], 1).astype(F)
    unit_disk = rng.random(n) < 0.3                                     # a disk of the camera's own size where the camera has none
    vec[unit_disk, 12:15] = cams["u"][pick][unit_disk] * F(0.25)
    vec[unit_disk, 15:18] = cams["v"][pick][unit_disk] * F(0.25)
    scale = np.select([rng.random(n) < 0.04, rng.random(n) < 0.04], [F(1e-30), F(1e30)], F(1)).astype(F)
    with np.errstate(all="ignore"):
        vec = vec * scale[:, None]
    vec = _with_nonfinite(rng, vec, 0.03)
    vec[rng.random(n) < 0.02, 6:9] = 0                                  # du = 0
    rec[:, 12:30] = vec.view(U)
    census.update(forced_four=len(want), circle=n_circle, x_past_2_16=MC._count(rec[:, 6].view(np.int32) >= (1 << 16)), recip_inf=MC._count(np.isinf(rec[:, 10].view(F))),
                  recip_one=MC._count(rec[:, 10].view(F) == 1), recip_2_15=MC._count(rec[:, 10].view(F) == F(2.0 ** -15)), du_zero=MC._count((vec[:, 6:9] == 0).all(1)),
                  angle_nan=MC._count(np.isnan(da)), angle_negative_zero=MC._count((da == 0) & np.signbit(da)), angle_denormal=MC._count(da == F(1e-40)))
    return np.ascontiguousarray(rec), census


def restate_get_ray(rec):
    """camera.cuh:210-242 over tests/math_restate.py: (n, 14) uint32 words"""
    rec = np.asarray(rec).reshape(-1, 30)
    st = np.array(rec[:, 0:6], dtype=U, copy=True)
    x, y, s_i, s_j = (rec[:, k].view(np.int32) for k in (6, 7, 8, 9))
    recip, angle = rec[:, 10].view(F), rec[:, 11].view(F)
    center, p00, du, dv, ddu, ddv = (rec[:, k: k + 3].view(F) for k in (12, 15, 18, 21, 24, 27))
    with np.errstate(all="ignore"):
        px = ((s_i.astype(F) + R.random_float(st)) * recip).astype(D) - 0.5
        py = ((s_j.astype(F) + R.random_float(st)) * recip).astype(D) - 0.5
        ox, oy = px.astype(F), py.astype(F)
        sample = (p00 + R.vscale((x.astype(D) + ox.astype(D)).astype(F), du)) + R.vscale((y.astype(D) + oy.astype(D)).astype(F), dv)
        disk = ~(angle <= 0)
        origin = center.copy()
        draws = np.full(len(rec), 3, U)
        sd = st[disk]
        p, sd, dd = R.random_in_unit_disk(sd)
        st[disk] = sd
        draws[disk] += dd
        origin[disk] = (center[disk] + R.vscale(p[:, 0], ddu[disk])) + R.vscale(p[:, 1], ddv[disk])
        direction = sample - origin
        tm = R.random_float(st)
    return np.concatenate([origin.view(U), direction.view(U), tm.view(U)[:, None], st, draws[:, None]], 1)


def offsets_of(rec):
    """the two random_float values get_ray's offsets are formed from (the first two draws)"""
    st = np.array(np.asarray(rec).reshape(-1, 30)[:, 0:6], dtype=U, copy=True)
    return R.random_float(st), R.random_float(st)


def ray_census(rec, out):
    """the branch census, from the oracle's answers (draw counts: 3 no disk, 5 accepted first, 7 rejected once, more: at least twice)"""
    draws = out[:, 13]
    a, b = offsets_of(rec)
    finite = np.isfinite(out[:, 0:7].view(F)).all(1)
    return dict(no_disk=int((draws == 3).sum()), accepted_first=int((draws == 5).sum()), rejected_once=int((draws == 7).sum()), rejected_more=int((draws >= 9).sum()),
                nonfinite=int((~finite).sum()), px_zero=int((a == 0).sum()), px_one=int((a == 1).sum()), py_zero=int((b == 0).sum()), py_one=int((b == 1).sum()))


def assert_ray_census(c, n):
    for k in ("no_disk", "accepted_first", "rejected_once", "rejected_more"):
        assert c[k] >= 1000, (k, c)
    assert c["nonfinite"] * 100 >= n, c
    for k in ("px_zero", "px_one", "py_zero", "py_one"):
        assert c[k] >= 1, (k, c)


# ---- the pixel's finish ----
@functools.lru_cache(None)
def pixel_records():
    """((N_PIXEL, 4) float32 records as uint32 words: scale, sum[3]; census)"""
    rng = np.random.default_rng(20264)
    ns = np.concatenate([np.arange(1, 33), [181]])
    scales = (1.0 / (ns * ns).astype(D)).astype(F)
    k = np.arange(257, dtype=D)
    edges = MC.around32(((k / 256.0) ** 2).astype(F), 1)                          # (k / 256)^2 and both neighbours
    top = MC.around32(F(0.999) * F(0.999), 3)
    specials = np.array([0.0, -0.0, 1e-45, 1e-40, 1.1754942e-38, -1e-45, -1e-40, 1.0, -0.5, -1.0, -1e-30, -1e30, 0.25, 0.5, 2.0, 1e30, np.inf, -np.inf], F)
    nans = np.array([0x7fc00000, 0xffc00000, 0x7fa00000, 0xffa00000, 0x7f800001, 0xffffffff], U).view(F)
    targets = np.concatenate([edges, top, specials, MC.around32(F(1.0), 2), nans])
    rows = []
    for s in scales:                                                               # the sums whose product with this scale is each target, and their neighbours
        with np.errstate(all="ignore"):
            s0 = (targets.astype(D) / D(s)).astype(F)
        cand = MC.around32(s0[np.isfinite(s0)], 2)
        cand = np.concatenate([cand, s0[~np.isfinite(s0)]])
        rows.append(np.stack([np.full(len(cand), s, F), cand], 1))
    tv = np.concatenate(rows)
    n_t = len(tv)
    n_mul = 4096
    rec = np.zeros((N_PIXEL, 4), F)
    rec[:n_t, 0] = tv[:, 0]
    rec[:n_t, 1] = tv[:, 1]
    rec[:n_t, 2] = np.roll(tv[:, 1], 1)
    rec[:n_t, 3] = np.roll(tv[:, 1], 7)
    mul = slice(n_t, n_t + n_mul)                                                  # inf * 0 and 0 * inf through the scale
    rec[mul, 0] = np.array([np.inf, 0.0, -0.0, np.inf], F)[np.arange(n_mul) % 4]
    rec[mul, 1:4] = np.array([0.0, np.inf, -np.inf, -0.0, 1.0, np.nan], F)[rng.integers(0, 6, (n_mul, 3))]
    rest = slice(n_t + n_mul, N_PIXEL)
    m = N_PIXEL - n_t - n_mul
    assert m > N_PIXEL // 4
    rec[rest, 0] = scales[rng.integers(0, len(scales), m)]
    rec[rest, 1:4] = MC.f32_families(rng, 3 * m).reshape(m, 3)                     # every exponent, both signs
    half = n_t + n_mul + m // 2                                                    # and products spread over [0, 1.1): every byte value
    dense = slice(half, N_PIXEL)
    with np.errstate(all="ignore"):
        rec[dense, 1:4] = (rng.uniform(0, 1.1, (N_PIXEL - half, 3)) ** 2 / rec[dense, 0].astype(D)[:, None]).astype(F)
    census = dict(targets=n_t, through_scale=n_mul, every_exponent=half - n_t - n_mul, dense=N_PIXEL - half)
    return np.ascontiguousarray(rec).view(U), census


def define_pixel(rec):
    """the definition: scale * sum in fp32, NaN -> 0 (the accumulator); then the correctly rounded square root (through float64), clamped to
    [0, 0.999], times 256, truncated; what is not a number after the root (a negative mean) gives 0; alpha 255.  (n, 4) uint32 words"""
    rec = np.asarray(rec).reshape(-1, 4).view(F)
    with np.errstate(all="ignore"):
        c = rec[:, 0:1] * rec[:, 1:4]
        c = np.where(np.isnan(c), F(0), c).astype(F)
        g = np.sqrt(c.astype(D)).astype(F)
        g = np.where(g < 0, F(0), g)
        g = np.where(g > F(0.999), F(0.999), g).astype(F)
        b = np.where(np.isnan(g), 0, np.trunc(F(256) * np.where(np.isnan(g), F(0), g))).astype(np.int64).astype(U)
    px = b[:, 0] | (b[:, 1] << U(8)) | (b[:, 2] << U(16)) | U(0xff000000)
    return np.concatenate([c.view(U), px[:, None].astype(U)], 1)


def pixel_census(rec, out):
    f = np.asarray(rec).reshape(-1, 4).view(F)
    with np.errstate(all="ignore"):
        prod = f[:, 0:1] * f[:, 1:4]
    b = np.stack([(out[:, 3] >> U(8 * k)) & U(0xff) for k in range(3)], 1)
    return dict(byte_values=len(np.unique(b)), nan_products=int(np.isnan(prod).sum()), negative=int((prod < 0).sum()), negative_zero=int(((prod == 0) & np.signbit(prod)).sum()),
                denormal=int(((np.abs(prod) > 0) & (np.abs(prod) < F(1.1754944e-38))).sum()), infinite=int(np.isinf(prod).sum()),
                minus_half=int((prod == F(-0.5)).sum()), minus_half_bytes=np.unique(b[prod == F(-0.5)]).tolist(),
                exact_squares=len(np.unique(prod[np.isin(prod, ((np.arange(257) / 256.0) ** 2).astype(F))])))


def assert_pixel_census(c):
    assert c["byte_values"] == 256 and c["exact_squares"] == 257, c
    for k in ("nan_products", "negative", "negative_zero", "denormal", "infinite", "minus_half"):
        assert c[k] >= 1, (k, c)
    assert c["minus_half_bytes"] == [0], c


# ---- comparison ----
RAY_KINDS = "f" * 7 + "i" * 7
PIXEL_KINDS = "fffi"


def assert_same(fn, rec, results):
    """results: {label: (n, out_words) uint32 words} -- all equal bit for bit (math_cases.canon's NaN rule; signed zeros count)"""
    kinds = PIXEL_KINDS if fn == 2 else RAY_KINDS
    rec = np.asarray(rec).reshape(len(rec), -1)
    labels = list(results)
    can = [MC.canon(np.asarray(results[k]).reshape(len(rec), -1), kinds) for k in labels]
    bad = np.zeros(len(rec), bool)
    for c in can[1:]:
        bad |= (c != can[0]).any(1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        hexes = lambda w: " ".join(f"{int(v):08x}" for v in np.ascontiguousarray(w).reshape(-1).view(U))
        raise AssertionError(f"{NAMES[fn]}: {int(bad.sum())} of {len(rec)} records differ; first at record {i}: input {hexes(rec[i])}; " +
                             "; ".join(f"{k} {hexes(np.asarray(results[k]).reshape(len(rec), -1)[i])}" for k in labels))


def records(fn):
    return pixel_records()[0] if fn == 2 else ray_records()[0]


@functools.lru_cache(None)
def oracle(fn):
    """the oracle's answers over the full record set of function fn (fn 0 and 1 share one)"""
    fn = 2 if fn == 2 else 0
    return O.camera_batch(fn, records(fn))


def pin_ray_records(n=1 << 12):
    """n of the get_ray records for the reference pin: half from the streams with four chosen outputs, half from the rest"""
    rec, census = ray_records()
    rng = np.random.default_rng(771)
    forced = len(rec) - census["forced_four"]
    pick = np.concatenate([rng.choice(forced, n // 2, replace=False), forced + rng.choice(census["forced_four"], n - n // 2, replace=False)])
    return np.ascontiguousarray(rec[np.sort(pick)])


def pin_pixel_cases(n=2048):
    """(n, 4) float32 rows for the reference pin of the pixel's tail: sqrt_spp in 1, 2, 3 and a background per channel; the reference adds the
    background sqrt_spp^2 times and scales, so backgrounds are squares (k / 256)^2 (16 significant bits: every partial sum is exact), their
    float neighbours, small integers times powers of two, and the negative, zero and infinite edges"""
    rng = np.random.default_rng(772)
    k = np.arange(257, dtype=D)
    squares = ((k / 256.0) ** 2).astype(F)
    pool = np.concatenate([squares, squares, MC.around32(squares, 1), (rng.integers(1, 64, 256) * 2.0 ** rng.integers(-40, 8, 256)).astype(F),
                           MC.around32(F(0.999) * F(0.999), 2), np.array([0.0, 1.0, -0.5, -1.0, -0.0, 1e-40, 1e-45, np.inf, 2.0, 1e30, -1e-30], F)])
    rows = np.zeros((n, 4), F)
    rows[:, 0] = 1 + np.arange(n) % 3
    rows[:, 1:4] = pool[rng.integers(0, len(pool), (n, 3))]
    rows[: len(pool), 1] = pool[: n]                                     # every pool value at least once
    return rows


def ragged(fn):
    rec = records(fn)
    pick = np.random.default_rng(770 + fn).choice(len(rec), RAGGED, replace=False)
    return np.ascontiguousarray(rec[np.sort(pick)])
