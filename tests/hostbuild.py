"""How the tests build host code of their own: the stand-alone check programs of tests/hostcheck/ (each with its own
main, under ASan and UBSan) and the shared objects that the ctypes fixtures load. One recipe for each kind, one rule for
what is stale, one table of the programs. A plain module: the tests import it."""
import functools
import glob
import os
import subprocess

ROOT  = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE  = os.path.join(ROOT, "tests", "hostcheck")
CSRC  = os.path.join(ROOT, "mrcal_amd", "csrc")
BUILD = os.path.join(HERE, "_build")
HIPCC = "/opt/rocm/bin/hipcc"

# host code only: -x c++ (the HIP headers are there for the sake of __host__ __device__), and no sanitizer for any GPU code
PROGRAM_FLAGS = ["-std=c++17", "-O1", "-g", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                 "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined"]
# (-ffp-contract=on: as the product is built)
LIBRARY_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=on", "-Wno-unused-function"]

# Every tests/hostcheck/*.cpp with a main (test_hostchecks.py holds the table to that): name -> (sources of the product
# compiled with it, whether it runs without arguments and prints "ok" and nothing else). Those that do are run by
# test_hostchecks.py; the others by the test that feeds them or reads what they print
PROGRAMS = {
    "analysis_plan_check":           ((), True),
    "chessboard_grid_check":         (("chessboard_grid.cpp",), True),
    "chessboard_pyramid_plan_check": ((), True),
    "damped_newton_check":           ((), True),
    "equalize_plan_check":           ((), True),
    "gram_banks_check":              ((), False),       # prints its table first: test_gram_banks.py
    "gram_packing_check":            ((), True),
    "image_prepare_check":           ((), True),
    "lensfit_plan_check":            ((), True),
    "match_plan_check":              ((), True),
    "point_cloud_plan_check":        ((), True),
    "problem_plan_check":            (("problem_plan.cpp",), True),
    "regional_stats_plan_check":     ((), True),
    "sgm_plan_check":                ((), True),
    "smooth_plan_check":             ((), True),
    "speckle_plan_check":            ((), True),
    "valid_region_check":            (("region_outline.cpp",), False),      # takes a file of masks: test_valid_region_host.py
}


def _build(out, sources, flags):
    """Coarse on purpose: anything of the product's sources makes every output stale"""
    deps = list(sources) + [os.path.join(ROOT, "include", "mrcal_amd.h"), os.path.abspath(__file__)]
    for pattern in ("*.hpp", "*.cpp", "*.hip"):
        deps += glob.glob(os.path.join(CSRC, pattern))
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(BUILD, exist_ok=True)
        # (under a name of its own, then moved into place: another test process never loads a half-written file)
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.check_call([HIPCC, *flags, *sources, "-o", tmp])
        os.replace(tmp, out)
    return out


def build_program(name):
    """the path of tests/hostcheck/<name>.cpp built as a stand-alone program, with ASan and UBSan"""
    extra, _ = PROGRAMS[name]
    sources = [os.path.join(HERE, name + ".cpp")] + [os.path.join(CSRC, s) for s in extra]
    return _build(os.path.join(BUILD, name), sources, PROGRAM_FLAGS)


def build_library(name):
    """the path of tests/hostcheck/<name>.cpp built as a shared object, for ctypes. No sanitizer flag, ever: a
    sanitized library needs the sanitizer's runtime preloaded into python, and that is not done in this project. What
    is to run under the sanitizers gets a main and a row in PROGRAMS"""
    return _build(os.path.join(BUILD, f"lib{name}.so"), [os.path.join(HERE, name + ".cpp")], LIBRARY_FLAGS)


@functools.lru_cache(maxsize=None)
def run_program(name):
    """an argument-less program built and run, once a test process"""
    return subprocess.run([build_program(name)], capture_output=True, text=True)


def assert_prints_ok(name):
    r = run_program(name)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
