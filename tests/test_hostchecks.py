"""Every stand-alone check program of tests/hostcheck/ (host units of the product, each driven by a main of its own)
built with ASan and UBSan and run, without a GPU; and the table of them (hostbuild.PROGRAMS) held to the directory, so
that a program added later cannot be left unrun."""
import glob
import os

import pytest

import hostbuild


@pytest.mark.parametrize("name", [name for name, (_, prints_ok) in hostbuild.PROGRAMS.items() if prints_ok])
def test_under_the_host_sanitizers(name):
    hostbuild.assert_prints_ok(name)


def test_every_program_is_in_the_table():
    with_main = set()
    for path in glob.glob(os.path.join(hostbuild.HERE, "*.cpp")):
        with open(path) as f:
            if "main(" in f.read():
                with_main.add(os.path.splitext(os.path.basename(path))[0])
    assert with_main == set(hostbuild.PROGRAMS)
