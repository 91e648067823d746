#!/usr/bin/env python3
"""The margin audit of DESIGN.md 4.3: which of the unified tree's stacked error margins does a test notice when it is gone?

For every mutant below the working tree is copied to a temporary directory, the named edits are applied to the copy, the CPU
pieces are built there, and two sets of CPU tests run in the copy: the grazing battery (tests/test_grazing_host.py) and the
tree-versus-oracle group the suite had before it (tests/test_host_mode.py -k "random_worlds or random_views or awkward or
grazing").  Prints the table mutant x caught-by.  CPU only: the copies run tests that are not marked gpu and nothing else (a
mutant is never to be launched on a GPU), nothing is written to the working tree, and pytest does not collect this file.  A
mutant takes one build of libmort_hip.so plus about two minutes of tests.

    python3 scripts/margin_audit.py              # every mutant
    python3 scripts/margin_audit.py a b h        # some
    python3 scripts/margin_audit.py --keep ...   # leave the copies in place and print where they are
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SC = "mort_amd/csrc/hip/scene_compile.h"
DG = "mort_amd/csrc/hip/dev_gen.h"

# (file, text to find exactly once, replacement)
_SPHERE_TERM = (SC, "delta += (e.r > 0) ? 20.0 * u * M * M / e.r : INFINITY;", "delta += 0.0 * M;")
_PADS = [(SC, "double delta = 64.0 * u * Mq + 1e-4;", "double delta = 0.0 * Mq;"),
         (SC, "g.wb.lo[k] -= (float)(64.0 * u * Mq); g.wb.hi[k] += (float)(64.0 * u * Mq);", "")]
_BOX_PAD = [(SC, "g.wb = box_pad(raw_box(g, delta));", "g.wb = raw_box(g, delta);"),
            (SC, "w.lo[k] = std::fmin(w.lo[k], std::nextafter((float)p[k], -INFINITY));", "w.lo[k] = std::fmin(w.lo[k], (float)p[k]);"),
            (SC, "w.hi[k] = std::fmax(w.hi[k], std::nextafter((float)p[k], INFINITY));", "w.hi[k] = std::fmax(w.hi[k], (float)p[k]);")]
_NEAREST = [(SC, "long long ql = (long long)std::floor(((double)b.lo[a] - (double)org[a]) / (double)step);",
             "long long ql = std::llround(((double)b.lo[a] - (double)org[a]) / (double)step);"),
            (SC, "while (ql > 0 && std::fmaf((float)ql, step, org[a]) > b.lo[a]) ql--;", ""),
            (SC, "long long qh = (long long)std::ceil(((double)b.hi[a] - (double)org[a]) / (double)step);",
             "long long qh = std::llround(((double)b.hi[a] - (double)org[a]) / (double)step);"),
            (SC, "while (qh <= 255 && std::fmaf((float)qh, step, org[a]) < b.hi[a]) qh++;", ""),
            (SC, "if (qh > 255 || std::fmaf((float)ql, step, org[a]) > b.lo[a]) { ok = false; break; }", "if (qh > 255) { ok = false; break; }")]
_BAND = (DG, "gr.band = mm * 4.76837158203125e-07f; /* 2^-21 */", "gr.band = 0.0f;")
_FAR = (DG, "if (far > mnear) gr.band =", "if (false && far > mnear) gr.band =")
_TAU = (DG, "mort_fabsf(tx)), 9.5367431640625e-07f, r.band);", "mort_fabsf(tx)), 0.0f, r.band);")
_NO_TOL = (DG, "return (tx - te < -tau) || (te - tau > closest);", "return (tx - te < -tau) || (te > closest);")
_NO_SCAN = (DG, "return gen_inv_ok(gr.ix) && gen_inv_ok(gr.iy) && gen_inv_ok(gr.iz) && (mm < 1e30f);", "return true;")

MUTANTS = {
    "a": ("sphere term of delta = 0", [_SPHERE_TERM]),
    "b": ("delta = 0 and both 64u*Mq pads gone", [_SPHERE_TERM] + _PADS),
    "c": ("(b) and box_pad, raw_box's nextafter gone", [_SPHERE_TERM] + _PADS + _BOX_PAD),
    "d": ("quantize_node rounds to nearest, fmaf check off", _NEAREST),
    "e": ("band = 0 in gen_ray_setup", [_BAND]),
    "f": ("far-origin widening off (kmin = 0)", [_FAR]),
    "g": ("tau's 2^-20 term = 0", [_TAU]),
    "h": ("(e) and (g)", [_BAND, _TAU]),
    "i": ("prune compares te > closest, no tolerance", [_NO_TOL]),
    "j": ("zero / denormal / huge reciprocals not sent to the scan", [_NO_SCAN]),
}
OLD = ["tests/test_host_mode.py", "-k", "random_worlds or random_views or awkward or grazing"]
NEW = ["tests/test_grazing_host.py"]
COPY = ["Makefile", "include", "mort_amd", "oracle", "scripts", "tests"]


def _copy_tree(dst):
    ignore = shutil.ignore_patterns("__pycache__", "*.pyc", "*.so", "*.o", "_ref", "bin", "lib")
    for name in COPY:
        src = os.path.join(ROOT, name)
        if os.path.isdir(src):
            shutil.copytree(src, os.path.join(dst, name), ignore=ignore)
        else:
            shutil.copy2(src, os.path.join(dst, name))


def _apply(dst, edits):
    for rel, old, new in edits:
        path = os.path.join(dst, rel)
        with open(path) as f:
            text = f.read()
        if text.count(old) != 1:
            raise SystemExit(f"{rel}: expected exactly one occurrence of {old!r}, found {text.count(old)}: the audit's edits are out of date")
        with open(path, "w") as f:
            f.write(text.replace(old, new))


def _build(dst):
    jobs = str(min(16, os.cpu_count() or 1))
    subprocess.check_call(["make", "-s", "-j" + jobs, "-C", dst, "host"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-s", "-C", os.path.join(dst, "oracle"), "all"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-s", "-j" + jobs, "-C", dst, "hip"], stdout=subprocess.DEVNULL)


def _run_tests(dst, args):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-rf", "--no-header", "-p", "no:cacheprovider", "-m", "not gpu"] + args,
                       cwd=dst, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    failed = re.findall(r"^FAILED (\S+)", p.stdout, flags=re.M)
    tail = p.stdout.strip().splitlines()[-1] if p.stdout.strip() else ""
    if p.returncode not in (0, 1):
        raise SystemExit(f"pytest could not run in {dst}:\n{p.stdout[-3000:]}")
    return failed, tail


def main(argv):
    keep = "--keep" in argv
    names = [a for a in argv if not a.startswith("--")] or (["none"] + sorted(MUTANTS))
    rows = []
    for name in names:
        what, edits = ("the build as it is", []) if name == "none" else MUTANTS[name]
        dst = tempfile.mkdtemp(prefix=f"margin_audit_{name}_")
        try:
            _copy_tree(dst)
            _apply(dst, edits)
            _build(dst)
            old_failed, old_tail = _run_tests(dst, OLD)
            new_failed, new_tail = _run_tests(dst, NEW)
        finally:
            if keep:
                print(f"# {name}: {dst}")
            else:
                shutil.rmtree(dst, ignore_errors=True)
        groups = sorted({re.sub(r".*\[(.*)\]", r"\1", t) for t in new_failed})
        rows.append((name, what, len(old_failed), len(new_failed), groups))
        print(f"# {name}: old [{old_tail}]  new [{new_tail}]", flush=True)
    print()
    print("| mutant | margin switched off | old tree-vs-oracle group | grazing battery | failing groups |")
    print("|---|---|---|---|---|")
    for name, what, old_n, new_n, groups in rows:
        print(f"| ({name}) | {what} | {'caught (%d)' % old_n if old_n else 'passes'} | {'caught (%d)' % new_n if new_n else 'passes'} | {', '.join(groups)} |")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
