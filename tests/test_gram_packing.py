"""The board kernel's Gram packings (csrc/problem.hpp, gram_packing()): which column blocks each operand of a k-step
holds, which pairs of operands are multiplied, and where every entry of the Gram ends up in the stored accumulators.
Checked on the host by a stand-alone program with its own main (tests/hostcheck/gram_packing_check.cpp), built with
ASan and UBSan: no GPU needed. What the kernel makes of the packings is tests/test_gram_packing_gpu.py."""
import hostbuild


def test_gram_packing_under_the_host_sanitizers():
    hostbuild.assert_prints_ok("gram_packing_check")
