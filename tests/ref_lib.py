"""Loader for oracle/_ref/libmort_ref*.so: the reference's own device code compiled for the CPU through the CUDA-on-host
shim (oracle/ref_render.cpp, oracle/refshim/).  Built by `make -C oracle ref` where the reference tree exists; test
infrastructure only (tests/test_reference_pin.py, tests/golden/make_golden.py, scripts/ref_distance.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

from mort_amd import structs as S
from tests import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
REF = os.environ.get("MORT_REFERENCE", "/root/reference")  # the same default as oracle/Makefile's REF
LIBS = {"pinned": "libmort_ref.so", "native": "libmort_ref_native.so", "fma": "libmort_ref_fma.so"}
_libs = {}


def path(mode="pinned"):
    return os.path.join(ORACLE_DIR, "_ref", LIBS[mode])


def reference_present():
    return os.path.isfile(os.path.join(REF, "world.cuh"))


def ensure_built(mode="pinned"):
    """Where the reference exists, brings the library up to date (an incremental make: an edit of the shim or the
    driver is never tested against a stale build) and returns True; a failed build raises.  Where it is absent, True
    when a built library is there, False when both are absent."""
    if not reference_present():
        return os.path.exists(path(mode))
    target = "ref-fma" if mode == "fma" else "ref"
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, f"REF={REF}", target], check=True)
    if not os.path.exists(path(mode)):
        raise RuntimeError(f"make {target} did not produce {path(mode)}")
    return True


def lib(mode="pinned"):
    if mode not in _libs:
        if not ensure_built(mode):
            raise RuntimeError(f"{path(mode)} is missing and the reference tree is absent")
        L = C.CDLL(path(mode))
        W, Cam, St = C.POINTER(S.World), C.POINTER(S.Camera), C.POINTER(S.RngState)
        fp = C.POINTER(C.c_float)
        L.mort_ref_load_world.argtypes = [W]; L.mort_ref_load_world.restype = C.c_int
        L.mort_ref_rng_seed.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int]; L.mort_ref_rng_seed.restype = None
        L.mort_ref_render.argtypes = [Cam, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.mort_ref_render.restype = C.c_int
        L.mort_ref_world_hit.argtypes = [fp, C.c_float, C.c_float, St, C.POINTER(O.Hit)]; L.mort_ref_world_hit.restype = C.c_bool
        L.mort_ref_get_ray.argtypes = [Cam, C.c_int, C.c_int, C.c_int, C.c_int, St, fp]; L.mort_ref_get_ray.restype = None
        L.mort_ref_ray_color.argtypes = [Cam, fp, St, fp]; L.mort_ref_ray_color.restype = C.c_int
        L.mort_ref_texture_value.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, fp, fp]; L.mort_ref_texture_value.restype = C.c_int
        L.mort_ref_pdf_value.argtypes = [C.c_int, C.c_int, fp, fp]; L.mort_ref_pdf_value.restype = C.c_float
        L.mort_ref_light_random.argtypes = [C.c_int, C.c_int, fp, St, fp]; L.mort_ref_light_random.restype = C.c_int
        L.mort_ref_add_bvh.argtypes = [W, C.c_int, C.c_bool, C.c_int]; L.mort_ref_add_bvh.restype = C.c_int
        L.mort_ref_camera_initialize.argtypes = [Cam]; L.mort_ref_camera_initialize.restype = None
        L.mort_ref_rotate_around.argtypes = [fp, fp, C.c_float, fp]; L.mort_ref_rotate_around.restype = None
        L.mort_ref_camera_input.argtypes = [Cam, C.c_int, C.c_int, C.c_int, C.c_int]; L.mort_ref_camera_input.restype = None
        L.mort_ref_libm.argtypes = [C.c_int, C.c_float]; L.mort_ref_libm.restype = C.c_float
        _libs[mode] = L
    return _libs[mode]


def load(world, mode="pinned"):
    rc = lib(mode).mort_ref_load_world(world.ptr)
    if rc != 0:
        raise RuntimeError(f"mort_ref_load_world failed: {rc}")


def seed_states(seed, width, height, mode="pinned", nthreads=16):
    st = np.zeros(width * height, dtype=O.STATE_DTYPE)
    lib(mode).mort_ref_rng_seed(st.ctypes.data, seed, width, height, nthreads)
    return st


def render(world, cam, states=None, seed=S.DEFAULT_SEED, mode="pinned", nthreads=16, want_accum=True):
    """The reference's Camera::render over the whole frame: dict(rgba, accum, states); `states` advance in place."""
    W, H = cam.image_width, cam.image_height
    if states is None:
        states = seed_states(seed, W, H, mode)
    load(world, mode)
    rgba = np.zeros((H, W, 4), dtype=np.uint8)
    accum = np.zeros((H, W, 3), dtype=np.float32) if want_accum else None
    rc = lib(mode).mort_ref_render(C.byref(cam), states.ctypes.data, 0, H, rgba.ctypes.data,
                                   accum.ctypes.data if accum is not None else None, nthreads)
    if rc != 0:
        raise RuntimeError(f"mort_ref_render failed: {rc}")
    return dict(rgba=rgba, accum=accum, states=states)
