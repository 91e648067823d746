#!/usr/bin/env python3
"""Generates the committed golden fixtures.  Run from the repo root in the build container:

    python tests/golden/make_golden.py

1. earthmap_rgb.npz -- texels of the reference's imgs/earthmap.jpg decoded with the reference's
   vendored stb_image.h (oracle/_ref/stb_decode, compiled from /root/reference where it lies).
   Needs /root/reference; skipped (existing file kept) when it is absent.
2. earthmap_damaged.npz -- damaged copies of earthmap.jpg (truncations, bytes changed inside the scan: the recipe) and what
   the same stb_decode makes of each (SHA-256 and shape of the RGB bytes, or "" where it refuses the file).  Needs
   oracle/_ref like (1); skipped (existing file kept) when it is absent.
3. oracle_golden.npz -- outputs of the CPU oracle (oracle/mort_oracle.c) for small configurations
   of every scene family: uchar4 image, fp32 accumulators, per-pixel segment counts, and the final
   RNG words of a few pixels.  BASELINE config 1 (Scene 1, 200x112, 4 spp) is case "s1_c1".
4. ref_pin.npz -- SHA-256 of what the reference's own device code, compiled for the CPU (oracle/_ref/libmort_ref.so,
   tests/ref_lib.py), renders for REF_PIN_CASES (two frames each: uchar4 image, fp32 accumulators, XORWOW words), and of
   the world bytes the reference's BVH builder leaves for REF_PIN_BVH.  Needs the reference; skipped (existing file
   kept) when it is absent.  The GPU kernels and the oracle are compared with these where the reference is absent.
5. medium_pin.npz -- the same digests for the constant-medium worlds of tests/medium_worlds.py (density and boundary edges), two
   frames each.  Needs the reference like (4).

The reference ships no golden data of its own.  (3) pins the oracle against its own regressions; (4) records
the reference's own arithmetic, so the oracle and the kernels stay pinned to it where the reference is absent (what
that cannot see: DESIGN.md 2).
"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))

CASES = {  # name: (scene, width, spp, depth)
    "s1_c1": (1, 200, 4, None),
    "s2": (2, 96, 4, None),
    "s3": (3, 96, 4, None),
    "s4": (4, 96, 4, None),
    "s5": (5, 64, 9, None),
    "s6": (6, 64, 9, None),
    "s7": (7, 48, 9, None),
    "s9": (9, 48, 4, None),
    "s10": (10, 160, 1, None),
    "s1_depth3": (1, 96, 4, 3),
}


# name: (scene, width, spp, depth); each kernel family renders at least one (tests/test_gpu_reference_pin.py)
REF_PIN_CASES = {
    "s1": (1, 64, 4, None),     # reference BVH: mega_bvh_kernel
    "s10": (10, 48, 4, 3),      # reference BVH: mega_bvh_kernel
    "s9": (9, 32, 4, None),     # final scene: mega_gen_kernel
    "s6": (6, 32, 4, None),     # Cornell box: mega_kernel
    "s3": (3, 48, 4, None),     # the earth image texture: mega_kernel
}
REF_PIN_FRAMES = 2
REF_PIN_BVH = ("scene1_reversed", "scene10_shuffled", "mixed_instances")


def digest(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def state_words(states):
    """d and v[5] of 48-byte XORWOW records (a structured STATE_DTYPE array or raw bytes) as uint32 (N, 6)"""
    from tests import oracle_lib as O
    st = np.ascontiguousarray(states).view(O.STATE_DTYPE).reshape(-1)
    return np.concatenate([st["d"][:, None], st["v"]], axis=1).astype("<u4")


def make_ref_pin():
    from mort_amd import host
    from tests import ref_lib as R
    from tests.worlds import BVH_BUILDS, world_object_bytes
    if not R.ensure_built():
        print("reference absent: keeping existing ref_pin fixture")
        return
    out = {}
    for name, (sid, width, spp, depth) in REF_PIN_CASES.items():
        world, cam = host.build_scene(sid, width=width, spp=spp, depth=depth)
        st = R.seed_states(69420, cam.image_width, cam.image_height)
        for f in range(REF_PIN_FRAMES):
            r = R.render(world, cam, states=st)
            out[f"{name}_f{f}"] = np.array([digest(r["rgba"]), digest(r["accum"]), digest(state_words(r["states"]))])
        print(name, cam.image_width, cam.image_height)
    for name in REF_PIN_BVH:
        w, li = BVH_BUILDS[name]()
        assert R.lib().mort_ref_add_bvh(w.ptr, li, False, 0) == 0
        out["bvh_" + name] = np.array([digest(np.frombuffer(world_object_bytes(w), np.uint8))])
    np.savez_compressed(os.path.join(HERE, "ref_pin.npz"), **out)


MEDIUM_PIN_FRAMES = 2


def make_medium_pin():
    """5. medium_pin.npz -- as (4), for the worlds of tests/medium_worlds.py from their own cameras"""
    from tests import medium_worlds as MW
    from tests import ref_lib as R
    if not R.ensure_built():
        print("reference absent: keeping existing medium_pin fixture")
        return
    out = {}
    for name in MW.NAMES:
        world, cam = MW.world(name), MW.camera(name)
        st = R.seed_states(69420, cam.image_width, cam.image_height)
        for f in range(MEDIUM_PIN_FRAMES):
            r = R.render(world, cam, states=st)
            out[f"{name}_f{f}"] = np.array([digest(r["rgba"]), digest(r["accum"]), digest(state_words(r["states"]))])
        print(name, cam.image_width, cam.image_height)
    np.savez_compressed(os.path.join(HERE, "medium_pin.npz"), **out)


def make_earth():
    ref = "/root/reference/imgs/earthmap.jpg"
    if not os.path.exists(ref):
        print("reference absent: keeping existing earthmap fixture")
        return
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"])
    tmp = "/tmp/mort_earthmap.ppm"
    subprocess.check_call([os.path.join(ROOT, "oracle", "_ref", "stb_decode"), ref, tmp])
    data = open(tmp, "rb").read()
    hdr, rest = data.split(b"255\n", 1)
    w, h = [int(t) for t in hdr.split()[1:3]]
    rgb = np.frombuffer(rest, dtype=np.uint8).reshape(h, w, 3)
    np.savez_compressed(os.path.join(HERE, "earthmap_rgb.npz"), rgb=rgb)
    print("earthmap", w, h)


def damaged_cases(data, recipe):
    """The damaged files of earthmap_damaged.npz's recipe, in order."""
    cases = [data[:int(n)] for n in recipe["trunc"]]
    for n, pos, val in zip(recipe["flip_n"], recipe["flip_pos"], recipe["flip_val"]):
        d = bytearray(data)
        for i, v in zip(pos[:n], val[:n]):
            d[int(i)] = int(v)
        cases.append(bytes(d))
    return cases


def make_damaged():
    import hashlib
    import tempfile
    exe = os.path.join(ROOT, "oracle", "_ref", "stb_decode")
    if not os.path.exists(exe):
        print("oracle/_ref/stb_decode absent: keeping existing damaged-file fixture")
        return
    data = open(os.path.join(HERE, "earthmap.jpg"), "rb").read()
    rng = np.random.default_rng(11)
    trunc = [600, 2000, 20000, len(data) - 1000, len(data) - 3]
    flip_n = np.zeros(60, np.int64)
    flip_pos = np.zeros((60, 5), np.int64)
    flip_val = np.zeros((60, 5), np.uint8)
    for k in range(60):  # damage inside the entropy-coded scan (headers stay valid)
        pos = rng.integers(1000, len(data) - 2, size=int(rng.integers(1, 6)))
        flip_n[k] = len(pos)
        for j, i in enumerate(pos):
            flip_pos[k, j], flip_val[k, j] = i, rng.integers(0, 255)  # never 0xff: no new markers
    recipe = dict(trunc=np.array(trunc, np.int64), flip_n=flip_n, flip_pos=flip_pos, flip_val=flip_val)
    digests, shapes = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for k, blob in enumerate(damaged_cases(data, recipe)):
            jpg, ppm = os.path.join(tmp, f"case{k}.jpg"), os.path.join(tmp, f"case{k}.ppm")
            open(jpg, "wb").write(blob)
            p = subprocess.run([exe, jpg, ppm], capture_output=True)
            if p.returncode != 0 or not os.path.exists(ppm):
                digests.append(""); shapes.append((0, 0, 0))
                continue
            raw = open(ppm, "rb").read()
            hdr = raw[:32].split()
            w, h = int(hdr[1]), int(hdr[2])
            off = raw.index(b"255") + 4
            digests.append(hashlib.sha256(raw[off:off + w * h * 3]).hexdigest()); shapes.append((h, w, 3))
    np.savez_compressed(os.path.join(HERE, "earthmap_damaged.npz"), sha256=np.array(digests), shape=np.array(shapes, np.int64), **recipe)
    print("damaged", len(digests), "cases,", sum(1 for d in digests if d), "decoded")


def make_oracle():
    from mort_amd import host
    from tests import oracle_lib as O
    out = {}
    for name, (sid, width, spp, depth) in CASES.items():
        world, cam = host.build_scene(sid, width=width, spp=spp, depth=depth)
        r = O.render(world, cam, nthreads=8)
        out[name + "_rgba"] = r["rgba"]
        out[name + "_accum"] = r["accum"]
        out[name + "_segpx"] = r["segments_px"].astype(np.uint16)
        out[name + "_states"] = np.stack([r["states"]["d"][:64], *[r["states"]["v"][:64, k] for k in range(5)]], axis=1)
        out[name + "_meta"] = np.array([sid, cam.image_width, cam.image_height, spp, cam.bounce_limit, r["segments"], r["rng_draws"]], dtype=np.int64)
        print(name, cam.image_width, cam.image_height, r["segments"])
    np.savez_compressed(os.path.join(HERE, "oracle_golden.npz"), **out)


if __name__ == "__main__":
    make_earth()
    make_damaged()
    make_oracle()
    make_ref_pin()
    make_medium_pin()
