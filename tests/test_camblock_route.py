"""camblock_route() (csrc/camblock_route.hpp) - the one function that decides by which route a trial step's camera block
is factored: the one-workgroup LDS Cholesky with or without the packed copy of S, or the launch-per-panel Cholesky
plain, compacted (with its tail kernel), compacted and dissected, or with the backward sweep. The launchers only read
what it returns. Checked on the CPU through its dev export against the table restated here: no GPU needed."""
import ctypes as C
import itertools
import os
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 64
LDS_LIMIT = 180          # the largest camera block the one-workgroup Cholesky holds (cholesky_lds.hip)
FIELDS = ("in_lds", "finish_rides", "S_packed", "compact", "nd_plans", "nd_launches", "sweep", "with_tail",
          "likely_panels", "l_last")


@pytest.fixture(scope="module")
def route():
    lib = C.CDLL(os.path.join(ROOT, "mrcal_amd", "libmrcal_amd.so"))
    f = lib.mrcal_amd_debug_camblock_route
    f.restype, f.argtypes = C.c_int, [C.c_int]*7 + [C.POINTER(C.c_int)]
    def call(Nc, sharded, compact, dissect, sweep, rounds, lchol_likely, nd_likely):
        out = (C.c_int*10)(*([-1]*10))
        ok = f(Nc, int(sharded), int(compact) | int(dissect) << 1 | int(sweep) << 2, rounds, 290, lchol_likely, nd_likely, out)
        if not ok: return None
        r = dict(zip(FIELDS, [int(v) for v in out]))
        return {k: (v if k in ("likely_panels", "l_last") else bool(v)) for k, v in r.items()}
    return call


def expected(Nc, sharded, compact, dissect, sweep, rounds, lchol_likely, nd_likely):
    """the table, literally"""
    if compact and sweep: return None
    if compact and sharded: return None
    if dissect and not compact: return None
    npanels = (Nc + NB - 1)//NB
    r = {}
    r["in_lds"] = Nc <= LDS_LIMIT
    r["finish_rides"] = not sharded and not sweep
    r["S_packed"] = r["finish_rides"] and r["in_lds"]
    r["compact"] = compact
    r["nd_plans"] = compact and dissect
    r["nd_launches"] = r["finish_rides"] and r["nd_plans"] and rounds > 0
    r["sweep"] = sweep
    r["likely_panels"] = nd_likely if r["nd_launches"] else lchol_likely
    r["with_tail"] = compact and not sweep and 0 < r["likely_panels"] < npanels
    r["l_last"] = r["likely_panels"] if r["with_tail"] else npanels
    if sharded and r["nd_plans"]: return None
    return r


@pytest.mark.parametrize("Nc", (1, 180, 181, 194, 652, 1206, 4096))
def test_the_route_is_the_table(route, Nc):
    npanels = (Nc + NB - 1)//NB
    likelies = sorted({0, 1, npanels - 1, npanels})
    refused = accepted = 0
    for sharded, compact, dissect, sweep in itertools.product((False, True), repeat=4):
        for rounds in (0, 4):
            # (the two counts the host learns are swept independently: which of them the route takes is part of the table)
            for lchol_likely, nd_likely in itertools.product(likelies, repeat=2):
                args = (Nc, sharded, compact, dissect, sweep, rounds, lchol_likely, nd_likely)
                r, e = route(*args), expected(*args)
                assert r == e, (args, r, e)
                if r is None:
                    refused += 1
                    continue
                accepted += 1
                # what the comments of the launchers used to state
                assert not r["nd_launches"] or (r["compact"] and r["finish_rides"]), (args, r)
                assert not r["S_packed"] or r["in_lds"], (args, r)
                assert not r["with_tail"] or (r["compact"] and not r["sweep"]), (args, r)
                assert not r["sweep"] or not r["finish_rides"], (args, r)
                assert 0 <= r["l_last"] <= npanels and (r["with_tail"] or r["l_last"] == npanels), (args, r)
    # of the 16 combinations of (sharded, mode): compact with sweep (4), compact sharded without sweep (2), dissect
    # without compact (4) do not exist
    per = 2*len(likelies)**2
    assert refused == 10*per and accepted == 6*per


def test_the_lds_limit_is_where_the_kernel_says(route):
    assert route(LDS_LIMIT, False, False, False, False, 0, 0, 0)["in_lds"]
    assert not route(LDS_LIMIT + 1, False, False, False, False, 0, 0, 0)["in_lds"]
    # the lchol_sweep hook on a small problem: the LDS kernel with the end of the trial in front, no packed copy
    r = route(LDS_LIMIT, False, False, False, True, 0, 0, 0)
    assert r["in_lds"] and not r["finish_rides"] and not r["S_packed"]
