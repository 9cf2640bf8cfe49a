"""The board kernel's Gram packings (csrc/problem.hpp, gram_packing()): which column blocks each operand of a k-step
holds, which pairs of operands are multiplied, and where every entry of the Gram ends up in the stored accumulators.
Checked on the host by a stand-alone program with its own main (tests/hostcheck/gram_packing_check.cpp), built with
ASan and UBSan: no GPU needed. What the kernel makes of the packings is tests/test_gram_packing_gpu.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gram_packing_under_the_host_sanitizers():
    here = os.path.join(ROOT, "tests", "hostcheck")
    csrc = os.path.join(ROOT, "mrcal_amd", "csrc")
    exe, src = os.path.join(here, "gram_packing_check"), os.path.join(here, "gram_packing_check.cpp")
    deps = [src] + [os.path.join(csrc, h) for h in ("problem.hpp", "layout.hpp", "lens_models.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        # (host code only: -x c++, the HIP headers for problem.hpp's sake, and no sanitizer for any GPU code)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-g", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                               "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
