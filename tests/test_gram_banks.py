"""The LDS bank conflicts of the board kernel's Gram operand reads (csrc/problem.hpp, gram_packing() and
gram_read_extra_cycles()): at 6 and 7 column blocks no read of a full half-tile conflicts. Counted on the host by the
DS instructions' bank rules in a stand-alone program with its own main (tests/hostcheck/gram_banks_check.cpp), built
with ASan and UBSan: no GPU needed. The program also prints the per-source conflict table of a 10x10 OPENCV8
observation that DESIGN.md 5.2 and profiles/LEDGER.md quote."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gram_reads_of_full_halves_are_conflict_free_under_the_host_sanitizers():
    here = os.path.join(ROOT, "tests", "hostcheck")
    csrc = os.path.join(ROOT, "mrcal_amd", "csrc")
    exe, src = os.path.join(here, "gram_banks_check"), os.path.join(here, "gram_banks_check.cpp")
    deps = [src] + [os.path.join(csrc, h) for h in ("problem.hpp", "layout.hpp", "lens_models.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        # (host code only: -x c++, the HIP headers for problem.hpp's sake, and no sanitizer for any GPU code)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-g", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                               "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "ok", r.stdout + r.stderr
    # the 6- and 7-block lines are there and say 0
    full = [l for l in lines if l.startswith(("blocks 6", "blocks 7")) and "full" in l]
    assert len(full) == 6 + 8 and all(l.endswith(": 0 extra cycles") for l in full), full
