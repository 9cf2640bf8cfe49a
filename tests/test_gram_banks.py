"""The LDS bank conflicts of the board kernel's Gram operand reads (csrc/problem.hpp, gram_packing() and
gram_read_extra_cycles()): at 6 and 7 column blocks no read of a full half-tile conflicts. Counted on the host by the
DS instructions' bank rules in a stand-alone program with its own main (tests/hostcheck/gram_banks_check.cpp), built
with ASan and UBSan: no GPU needed. The program also prints the per-source conflict table of a 10x10 OPENCV8
observation that DESIGN.md 5.2 and profiles/LEDGER.md quote."""
import hostbuild


def test_gram_reads_of_full_halves_are_conflict_free_under_the_host_sanitizers():
    r = hostbuild.run_program("gram_banks_check")
    print(r.stdout)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "ok", r.stdout + r.stderr
    # the 6- and 7-block lines are there and say 0
    full = [l for l in lines if l.startswith(("blocks 6", "blocks 7")) and "full" in l]
    assert len(full) == 6 + 8 and all(l.endswith(": 0 extra cycles") for l in full), full
