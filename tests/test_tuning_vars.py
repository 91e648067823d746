"""The README says of the library's tuning variables: "none changes a result bit; the GPU tests check that".  This keeps the claim
honest without a GPU: every MORT_* variable the HIP library reads is either a diagnostic (it changes what is printed or which rows a
debug run renders, never a scheduling choice) or named in some tests/test_gpu_*.py, and the README lists every one that is not a
diagnostic."""
import glob
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

DIAGNOSTICS = {"MORT_DEBUG_PIXEL", "MORT_HOST_DEBUG", "MORT_HOST_ROWS", "MORT_GEN_HEAVY_DEBUG"}
DIAGNOSTIC_PREFIXES = ("MORT_TEST_",)


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _library_vars():
    names = set()
    for path in sorted(glob.glob(os.path.join(ROOT, "mort_amd", "csrc", "hip", "*"))):
        names.update(re.findall(r'getenv\(\s*"(MORT_[A-Z0-9_]+)"\s*\)', _read(path)))
    return names


def _named(name, text):
    return re.search(r"(?<![A-Z0-9_])" + re.escape(name) + r"(?![A-Z0-9_])", text) is not None


def _is_diagnostic(name):
    return name in DIAGNOSTICS or name.startswith(DIAGNOSTIC_PREFIXES)


def test_the_parser_finds_the_variables():
    names = _library_vars()
    # a few that certainly exist, so an empty or broken scan cannot pass the tests below
    assert {"MORT_LANE_CAP", "MORT_GEN_DL", "MORT_WAVE_SHARE", "MORT_GEN_HEAVY", "MORT_GEN_HEAVY_DEBUG"} <= names
    assert len(names) >= 25


def test_every_tuning_variable_is_set_by_a_gpu_test():
    gpu_tests = "\n".join(_read(p) for p in sorted(glob.glob(os.path.join(HERE, "test_gpu_*.py"))))
    missing = sorted(n for n in _library_vars() if not _is_diagnostic(n) and not _named(n, gpu_tests))
    assert not missing, f"read by libmort_hip but set by no tests/test_gpu_*.py: {missing}"


def test_readme_lists_every_tuning_variable():
    readme = _read(os.path.join(ROOT, "README.md"))
    missing = sorted(n for n in _library_vars() if not _is_diagnostic(n) and not _named(n, readme))
    assert not missing, f"read by libmort_hip but missing from README.md's list of tuning variables: {missing}"


def test_diagnostics_are_read_by_the_library():
    """The explicit list stays short and current: each diagnostic it names is still read somewhere."""
    names = _library_vars()
    assert DIAGNOSTICS <= names, sorted(DIAGNOSTICS - names)
