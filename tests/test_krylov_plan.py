"""The host rules and the scalar step of AMG-PCG, its multi-right-hand-side form and the block solve
(csrc/ipd_krylov_plan.h, csrc/ipd_pcg_step.h) on the CPU: a small C++ driver (tests/krylov_plan_driver.cpp) is
built with the system g++ (-ffp-contract=off, as the library is) against the two headers; each rule is run at its
edges, and the step is fed the inner products of the numpy restatement tests/amg_pcg_ref.py and must return its
alpha, beta, res, it and stop flag bit for bit.  CPU only, no library."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests import amg_pcg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "codes_of_ipd_ssn_amg_method_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
LIMITS = open(os.path.join(CSRC, "ipd_limits.h")).read()


def _const(name):
    return int(re.search(r"static constexpr int %s = (\d+);" % name, LIMITS).group(1))


BT = _const("BT")
STAGE_MAX = _const("STAGE_MAX")
BLK_WMAX = _const("BLK_WMAX")
PCG_SMALL_MAXIT = _const("PCG_SMALL_MAXIT")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("krylov_plan") / "krylov_plan_driver")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC,
                          "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "krylov_plan_driver.cpp"),
                          "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def ask(driver, lines):
    """the driver's answer lines (token lists) to the given command lines"""
    res = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    out = res.stdout.splitlines()
    assert out[0].split() == ["limits"] + [str(v) for v in (BT, STAGE_MAX, BLK_WMAX, PCG_SMALL_MAXIT)]
    assert len(out) == len(lines) + 1
    return [o.split() for o in out[1:]]


def ints(driver, lines):
    return [[int(t) for t in toks] for toks in ask(driver, lines)]


# ---- the plan ------------------------------------------------------------------------------------
def test_block_width(driver):
    ns = [1, 2, 3, 4, 5, 8]
    assert [w for (w,) in ints(driver, ["width %d" % n for n in ns])] == [1, 2, 4, 4, 8, 8]


def test_chunks(driver):
    want = {1: [(0, 1, 1)], 2: [(0, 2, 2)], 3: [(0, 3, 4)], 8: [(0, 8, 8)], 9: [(0, 8, 8), (8, 1, 1)],
            16: [(0, 8, 8), (8, 8, 8)], 17: [(0, 8, 8), (8, 8, 8), (16, 1, 1)]}
    got = ask(driver, ["chunks %d" % n for n in want])
    for n, toks in zip(want, got):
        assert [tuple(int(v) for v in t.split(",")) for t in toks] == want[n], n


def test_staging(driver):
    assert STAGE_MAX % 8 == 0
    n8 = STAGE_MAX // 8   # 960
    cases = [(n8, 8), (n8 + 1, 8), (STAGE_MAX, 1), (STAGE_MAX + 1, 1), (STAGE_MAX // 2, 2), (STAGE_MAX // 2 + 1, 2),
             (2 * (STAGE_MAX // 8), 4), (2 * (STAGE_MAX // 8) + 1, 4)]
    got = ints(driver, ["stage %d %d" % c for c in cases])
    for (n, w), (staged, dyn) in zip(cases, got):
        assert staged == int(n * w <= STAGE_MAX), (n, w)
        assert dyn == (8 * n * w if staged else 0), (n, w)
    assert [g[0] for g in got] == [1, 0] * 4


def test_g3(driver):
    cu = 256
    ns = [0, 1, BT, BT + 1, BT * cu, BT * cu + 1, 10 * BT * cu]
    got = [g for (g,) in ints(driver, ["g3 %d %d" % (n, cu) for n in ns])]
    assert got == [1, 1, 1, 2, cu, cu, cu]
    assert got == [max(1, min(cu, -(-n // BT))) for n in ns]


def test_io_grid(driver):
    cases = [(1, 1), (256, 1), (257, 1), (256 * 1024 // 8, 8), (256 * 1024 // 8 + 1, 8), (10 ** 7, 8), (0, 1)]
    got = ints(driver, ["io %d %d" % c for c in cases])
    assert [g for g, _ in got] == [1, 1, 2, 1024, 1024, 1024, 1]
    assert all(t == 256 for _, t in got)


def test_route(driver):
    cases = [(1, 0), (1, PCG_SMALL_MAXIT), (1, PCG_SMALL_MAXIT + 1), (0, 0), (0, PCG_SMALL_MAXIT), (1, -1)]
    assert [r for (r,) in ints(driver, ["route %d %d" % c for c in cases])] == [1, 1, 0, 0, 0, 0]


def test_pcg_options(driver):
    h = float.hex
    got = ask(driver, ["opts null", "opts %s 0 -1" % h(0.0), "opts %s -1 -1" % h(-1.0), "opts %s 7 -1" % h(1e-6),
                       "opts %s -5 -1" % h(-0.5), "opts %s 7 2" % h(1e-6), "opts %s -1 1" % h(-1.0)])
    val = [(int(ok), float.fromhex(tol), int(mi)) for ok, tol, mi in got]
    assert val[0] == (1, 1e-11, 10000)          # NULL: the defaults
    assert val[1] == (1, 0.0, 0)                # retol = 0 and maxit = 0 are taken
    assert val[2] == (1, 1e-11, 10000)          # unset fields
    assert val[3] == (1, 1e-6, 7)
    assert val[4] == (1, 1e-11, 10000)          # negative fields are unset ones
    assert val[5][0] == 0 and val[6][0] == 0    # precd set: the caller's IPD_E_ARG


def test_history_indexing(driver):
    got = ints(driver, ["resk 0 10 1", "resk 0 10 10", "resk 3 10 1", "resk 3 10 4", "resk 8 1000 1",
                        "stride 0", "stride 50"])
    assert [g for (g,) in got] == [0, 9, 30, 33, 8000, 1, 51]


# ---- the step ------------------------------------------------------------------------------------
def run_step(driver, maxit, tol, d0, triples):
    """-> (it, res, stop) of the first form, then (alpha, beta, res, it, stop) per triple (pq, rw, rwo)"""
    h = float.hex
    line = "step %d %s %s " % (maxit, h(tol), h(d0)) + " ".join("%s %s %s" % (h(a), h(b), h(c)) for a, b, c in triples)
    (toks,) = ask(driver, [line])
    groups = " ".join(toks).split(" | ")
    f = groups[0].split()
    first = (int(f[1]), float.fromhex(f[2]), int(f[3]))
    rest = []
    for g in groups[1:]:
        a, b, r, it, stop = g.split()
        rest.append((float.fromhex(a), float.fromhex(b), float.fromhex(r), int(it), int(stop)))
    return first, rest


def bits(x):
    return np.float64(x).tobytes()


def spd_system(N=150, seed=3):
    rs = np.random.RandomState(seed)
    B = sp.random(N, N, density=0.05, random_state=rs, format="csr")
    A = (B @ B.T + sp.diags(0.5 + rs.random_sample(N))).tocsr()
    return A, rs.standard_normal(N)


@pytest.mark.parametrize("maxit,retol", [(10000, 2.0 ** -30), (5, 2.0 ** -30), (10000, 2.0 ** -8)])
def test_step_against_restatement(driver, maxit, retol):
    """retol is a power of two, so that its square is the same number however it is formed"""
    A, e = spd_system()
    dinv = 1.0 / A.diagonal()
    trace = []
    _, it, res, resk = R.amg_pcg(A, e, lambda r: dinv * r, retol=retol, maxit=maxit, trace=trace)
    assert it == len(trace) - 1 and it >= 3 and (it == maxit) == (maxit == 5)
    d0 = trace[0]
    first, rest = run_step(driver, maxit, retol, d0, [(t["pq"], t["rw"], t["rwo"]) for t in trace[1:]])
    assert first == (0, 1.0, 0)
    assert len(rest) == it
    for k, (t, (alpha, beta, r, itk, stop)) in enumerate(zip(trace[1:], rest)):
        assert bits(alpha) == bits(t["alpha"]) and bits(beta) == bits(t["beta"]), k
        assert bits(r) == bits(resk[k]) and itk == k + 1, k
        assert stop == int(k + 1 == it), k       # the restatement's loop ends exactly where the flag is set
    assert bits(rest[-1][2]) == bits(res)


def test_step_edges(driver):
    # delta_0 = 0 (a padding column): stops at the first test, res is NaN -- as the restatement reports it
    first, _ = run_step(driver, 100, 1e-11, 0.0, [])
    assert first[0] == 0 and math.isnan(first[1]) and first[2] == 1
    _, it, res, _ = R.amg_pcg(sp.identity(4, format="csr"), np.zeros(4), lambda r: r)
    assert it == 0 and math.isnan(res)
    # maxit = 0: stops at the first test with res = 1
    assert run_step(driver, 0, 1e-11, 3.0, [])[0] == (0, 1.0, 1)
    # tol = 0 runs to maxit, also when delta_new falls to the smallest positive number; an exact zero stops
    tiny = 5e-324
    first, rest = run_step(driver, 3, 0.0, 2.0, [(1.0, 1.0, 0.0), (1.0, tiny, 0.0), (1.0, tiny, 0.0)])
    assert first == (0, 1.0, 0) and [(r[3], r[4]) for r in rest] == [(1, 0), (2, 0), (3, 1)]
    _, rest = run_step(driver, 3, 0.0, 2.0, [(1.0, 0.0, 0.0)])
    assert (rest[0][3], rest[0][4]) == (1, 1)
    # a negative delta_new: res is the root of |delta_new / delta_0|, the loop stops, beta keeps its sign
    _, rest = run_step(driver, 10, 1e-3, 4.0, [(2.0, -1.0, 0.5)])
    alpha, beta, r, it, stop = rest[0]
    assert (alpha, beta, r, it, stop) == (2.0, -0.375, 0.5, 1, 1)
