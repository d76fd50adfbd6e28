"""The predicate of the full-shape form of k_resident's composed instantiation (resident_takes_full,
csrc/ipd_resident_plan.h) on the CPU: tests/resident_plan_full_driver.cpp is built with the system g++ against the
header and run on three-level shapes.  The predicate holds for exactly one shape -- F block, C block and level 2 of
1024 rows, 128 workgroups, the composed level 2, transfers from the mask with P = [W; I], isnsp, local first
sweeps, at least one sweep, a one-row tail, the V cycle -- and fails for each single violated condition.  CPU only."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "codes_of_ipd_ssn_amg_method_amd", "csrc")

FULL = dict(nf=1024, nc=1024, N2=1024, Nt=1, cycle="v", smoth=5, G=0, poly2=1, xm=1, wident=1, isnsp=1, lfirst=1,
            no_full=0)
ORDER = "nf nc N2 Nt cycle smoth G poly2 xm wident isnsp lfirst no_full".split()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resident_plan_full") / "resident_plan_full_driver")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC,
                          os.path.join(HERE, "resident_plan_full_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def run(driver, cases):
    """Per case: dict(kind, ke, ke3, poly2, G, wident, full)."""
    text = "\n".join(" ".join(str(dict(FULL, **c)[k]) for k in ORDER) for c in cases) + "\n"
    res = subprocess.run([driver], input=text, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = []
    for ln in res.stdout.splitlines():
        f = ln.split()
        assert f[0] == "plan" and f[7] == "full" and len(f) == 9, ln
        out.append(dict(kind=f[1], ke=int(f[2]), ke3=int(f[3]), poly2=int(f[4]), G=int(f[5]), wident=int(f[6]),
                        full=int(f[8])))
    assert len(out) == len(cases)
    return out


def test_the_full_shape_is_taken(driver):
    for smoth in (1, 2, 5):
        (p,) = run(driver, [dict(smoth=smoth)])
        assert p == dict(kind="k", ke=16, ke3=0, poly2=1, G=128, wident=1, full=1), (smoth, p)


VIOLATIONS = {
    "F rows": dict(nf=1000),                       # the (1024, 1000) system: n = nf = 1000
    "F rows, one short": dict(nf=1023),
    "C rows": dict(nc=1000, N2=1000),              # the (1000, 1024) system
    "C rows, one short": dict(nc=1023, N2=1023),
    "level 2 is not the C block": dict(N2=1000),
    "G": dict(G=256),                              # IPD_RESIDENT_G=256: four rows of a block per workgroup
    "G, one more": dict(G=129),
    "wident 0": dict(wident=0),
    "wident -1": dict(wident=-1),
    "no mask transfers": dict(xm=0),
    "W cycle": dict(cycle="w"),
    "smoth 0": dict(smoth=0),
    "no composed level 2": dict(poly2=0),
    "isnsp 0": dict(isnsp=0),
    "first sweeps handed off": dict(lfirst=0),
    "tail of two rows": dict(Nt=2),
    "IPD_RES_NO_FULL": dict(no_full=1),
}


@pytest.mark.parametrize("name", sorted(VIOLATIONS))
def test_each_violated_condition_keeps_the_general_form(driver, name):
    (p,) = run(driver, [VIOLATIONS[name]])
    assert p["full"] == 0, (name, p)
    # ... and where the condition is not one of the plan's own, the plan is the full shape's in everything else
    if name in ("wident 0", "wident -1", "no mask transfers", "isnsp 0", "first sweeps handed off", "IPD_RES_NO_FULL"):
        assert (p["kind"], p["ke"], p["poly2"], p["G"]) == ("k", 16, 1, 128), (name, p)

