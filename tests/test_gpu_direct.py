"""The dense direct solves where their block loops wrap: the blocked Cholesky of csrc/ipd_dense.hip behind
`ipd_spd_solve`, behind inner_solver 1 and 2 of the drivers and behind the ideal interpolation, and the LDS
Cholesky `k_small_blocks` of csrc/ipd_hybrid.hip on systems made of small components only.

The bar is the backward-error bound of a Cholesky solve, bar(n) = (3 n^2 + 4) u per right-hand side
(tests/direct_cases.py derives it; tests/test_direct_cases.py proves on the CPU that every case sits on the side
of each edge it is named for and that LAPACK and the oracle stay under a tenth of the bar).  Every test prints its
worst eta / bar."""
import time

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ipd_oracle as O
from tests import direct_cases as C

pytestmark = pytest.mark.gpu

OPTS = dict(retol=1e-11, bigph=1, maxit=30, theta=0.25, smoth=5, cycle="w", isnsp=1, inter=1, guess=None)


@pytest.fixture(scope="module")
def ipd():
    import codes_of_ipd_ssn_amg_method_amd as m
    return m


def assert_spd_solve(ipd, n, nrhs, what):
    A, nrm = C.spd_matrix(n)
    B = C.spd_rhs(n, nrhs)
    t0 = time.perf_counter()
    X = ipd.spd_solve(A, B)
    dt = time.perf_counter() - t0
    assert X.shape == (n, nrhs)
    assert np.all(np.isfinite(X))
    e = C.eta(A, X, B, nrm)
    print("%s n = %d, nrhs = %d: worst eta / bar = %.3g (solve %.3f s)" % (what, n, nrhs, e.max() / C.bar(n), dt))
    assert e.shape == (nrhs,) and np.all(e <= C.bar(n)), (what, int(np.argmax(e)), e.max() / C.bar(n))


# ---------------------------------------------------------------------------------------------------------
# A. ipd_spd_solve at its geometry edges
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nrhs", C.SPD_CASES)
def test_spd_solve_meets_the_backward_error_bound(ipd, n, nrhs):
    assert_spd_solve(ipd, n, nrhs, "A")


# ---------------------------------------------------------------------------------------------------------
# B. failure rules
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["pivot100", "pivot129", "nan"])
def test_a_failing_pivot_past_the_first_block_raises_and_leaves_the_context_usable(ipd, case):
    A = C.nan_entry() if case == "nan" else C.bad_pivot(int(case[5:]))
    with pytest.raises(ipd.IpdError, match="not symmetric positive definite"):
        ipd.spd_solve(A, C.spd_rhs(C.FAIL_N, 65))
    assert_spd_solve(ipd, 129, 65, "B after %s," % case)          # the same context, a valid solve


def test_the_two_limits_are_refused(ipd):
    """both IPD_E_LIMIT rules of ipd_spd_solve; test_direct_cases.py checks that they precede the dense allocation"""
    with pytest.raises(ipd.IpdError, match="dense scratch above 2 GiB"):
        ipd.spd_solve(sp.identity(C.LIMIT_ORDER, format="csc"), np.ones((C.LIMIT_ORDER, 1)))
    with pytest.raises(ipd.IpdError, match="too many right-hand sides"):
        ipd.spd_solve(sp.csc_matrix(np.array([[2.0]])), np.ones((1, C.LIMIT_NRHS)))
    assert_spd_solve(ipd, 65, 64, "B after the limits,")


# ---------------------------------------------------------------------------------------------------------
# C. k_small_blocks alone
# ---------------------------------------------------------------------------------------------------------
def assert_small_system(ipd, name):
    pd = C.small_system(name)[0]
    z_ref, it_ref, res_ref, info_ref, used_ref = C.small_reference(name)
    rng = ipd.MatlabRand()
    z, it, res, info = ipd.Hybrid_AMG(pd, O.amg_options_class2("v"), rng)
    assert (it, res, list(info), rng.consumed) == (it_ref, res_ref, list(info_ref), used_ref) == \
        (0, 0.0, [len(C.small_system(name)[4]), 0], 0)
    assert np.all(np.isfinite(z))
    es = C.small_etas(name, z)
    ratio, nb = max((e / C.bar(nb), nb) for nb, e in es)
    print("C %s: worst eta / bar = %.3g (on a block of %d); |z - oracle| = %.3g" %
          (name, ratio, nb, np.linalg.norm(z - z_ref)))
    bad = [(k, nb, e / C.bar(nb)) for k, (nb, e) in enumerate(es) if not e <= C.bar(nb)]
    assert not bad, bad[:5]


@pytest.mark.parametrize("name", list(C.SMALL_SYSTEMS))
def test_small_blocks_meet_the_backward_error_bound_block_by_block(ipd, name):
    assert_small_system(ipd, name)


def test_an_indefinite_small_block_raises_and_leaves_the_context_usable(ipd):
    pd = C.indefinite_system()[0]
    with pytest.raises(ipd.IpdError, match="small diagonal block is not positive definite"):
        ipd.Hybrid_AMG(pd, O.amg_options_class2("v"), ipd.MatlabRand())
    assert_small_system(ipd, "n0_only")


# ---------------------------------------------------------------------------------------------------------
# D. the dense routes inside the drivers
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,solver", C.DRIVER_RUNS, ids=["class%d-s%d" % r for r in C.DRIVER_RUNS])
def test_driver_iterations_through_the_dense_routes_match_the_oracle(ipd, cls, solver):
    """M = 271: five blocks; class 2 factors the bordered Jacobian of order 272 (inner_solver 1) or runs
    Jacobi-PCG on its compacted copy (inner_solver 2).  K iterations from the oracle's warm start against the
    oracle's K iterations with SciPy's sparse direct solve; neither converges within K."""
    from tests.test_gpu_driver import ws_of
    pr = C.driver_problem(cls)
    start, ref = C.driver_reference(cls)
    ws = ws_of(cls, pr)
    ws.set_state(start[0], start[0], start[1], 1.0)
    opts = OPTS if solver == 1 else dict(OPTS, smoth=10, maxit=40)
    out = ws.run(opts, ipd.MatlabRand(5489), iters=C.DRIVER_K, inner_solver=solver)
    hist = ws.history()
    recs = ws.records()
    ws.close()
    assert not ref["converged"] and ref["k"] == C.DRIVER_K
    assert out["converged"] == ref["converged"] and out["k"] == ref["k"]
    worst = {key: float(np.max(np.abs(hist[key] - np.asarray(ref[key])) / (1 + np.abs(np.asarray(ref[key])))))
             for key in ("KKT_xk", "KKT_lk") if hist[key].shape == np.asarray(ref[key]).shape}
    print("D class %d, inner_solver %d: |fval - ref| = %.3g, histories off by %s (relative to 1 + |ref|)" %
          (cls, solver, abs(out["fval"] - ref["fval"]), worst))
    if solver == 1:
        assert abs(out["fval"] - ref["fval"]) <= 1e-9 * (1 + abs(ref["fval"]))
        assert recs and all(r["itamg"] == 1 and r["resamg"] == 0.0 and r["info0"] == 0 for r in recs)
        for key in ("KKT_xk", "KKT_lk"):
            a, b = hist[key], np.asarray(ref[key])
            assert a.shape == b.shape and np.all(np.abs(a - b) <= 1e-8 * (1 + np.abs(b))), key
        ssn, ssn_ref = hist["SsN_itnum"].astype(int), np.asarray(ref["SsN_itnum"]).astype(int)
        half = len(ssn_ref) // 2
        assert np.array_equal(ssn[:half], ssn_ref[:half]) and np.abs(ssn - ssn_ref).max() <= 1
    else:
        assert abs(out["fval"] - ref["fval"]) <= 1e-7


# ---------------------------------------------------------------------------------------------------------
# E. ideal interpolation with Nf and Nc past 256
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("isnsp", [0, 1])
def test_ideal_interpolation_beyond_one_workgroup_of_columns(ipd, isnsp):
    A = C.ideal_matrix()
    Ac, Pro, isC = C.ideal_reference(isnsp)
    gAc, gPro, gC = ipd.transfer(A, C.ideal_options(isnsp), 2, ipd.MatlabRand())
    assert np.array_equal(gC, isC)
    assert isC.sum() > 256 and (~isC).sum() > 256
    assert gPro.shape == Pro.shape and gAc.shape == Ac.shape
    print("E isnsp %d: Pro off by %.3g of its bar, Ac by %.3g" %
          (isnsp, abs(gPro - Pro).max() / (1e-11 * abs(Pro).max()), abs(gAc - Ac).max() / (1e-10 * abs(Ac).max())))
    assert abs(gPro - Pro).max() <= 1e-11 * abs(Pro).max()
    assert abs(gAc - Ac).max() <= 1e-10 * abs(Ac).max()
    if isnsp == 0:      # the defining equation of the ideal interpolation, on the device result
        F, Cn = np.flatnonzero(~isC), np.flatnonzero(isC)
        Ad = A.toarray()
        W = gPro.toarray()[F, :]
        assert np.abs(Ad[np.ix_(F, F)] @ W + Ad[np.ix_(F, Cn)]).max() <= 1e-12 * np.abs(Ad).max() * max(1.0, np.abs(W).max())
        nf, es = C.ideal_etas(gPro, isC)                              # ... and column by column, at the derived bar
        print("E isnsp 0: worst eta / bar = %.3g" % (es.max() / C.bar(nf)))
        assert es.shape == (len(Cn),) and np.all(es <= C.bar(nf))
    else:
        assert np.allclose(gPro.toarray().sum(axis=1), 1.0, atol=1e-12)
