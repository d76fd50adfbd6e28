"""`ipd_pcg` (k_pcg / pcg_block for precd 1, 2; k_pcg_gen for precd 3, 4, 5), `aug_PCG` and `PCG4POT` where their
loops wrap: more rows than the one workgroup has threads (every `row += BT` loop takes 2 to 14 passes), rows of
more than 64 entries (the `t += 64` / `u += 64` walks of the triangular solves, of IC(0) and of k_aug_fill), every
lanes-per-row value of the Jacobi kernel from 1 to PCG_LANES_MAX, the 7000-row bound of the LDS-resident solve,
and IC(0) breaking down past the first pass.

A converged solve hides a preconditioner that is applied slightly wrong (it still converges to the same d), so
the probes are SHORT runs of fixed length against the oracle: one iteration from zero (d = alpha M^-1 e: a wrong
factor entry, a skipped row, a wrong triangular solve shows in d itself) and eight iterations from a nonzero
guess (the recurrence).  tests/test_pcg_cases.py proves on the CPU that the oracle's answers to exactly these
runs are stable to a thousandth of the bars used here.  References: oracle/ipd_oracle.py and numpy / scipy direct
solves only; bars: those of test_gpu_cycle.py and test_gpu_altsolvers.py."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ipd_oracle as O
from tests import pcg_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ipd():
    import codes_of_ipd_ssn_amg_method_amd as m
    return m


def run(ipd, kind, name, precd):
    return ipd.PCG(C.matrix(name), C.rhs(name), C.options(kind, name, precd))


def assert_d(d, d_ref, what):
    err = np.max(np.abs(d - d_ref) / (1e-10 + 1e-8 * np.abs(d_ref)))
    print("%s: d at %.3g of its bar" % (what, err))
    assert np.allclose(d, d_ref, rtol=1e-8, atol=1e-10), (what, err)


def assert_history(resk, resk_ref, k, what):
    err = np.max(np.abs(resk[:k] - resk_ref[:k]) / (1e-8 + 1e-6 * np.abs(resk_ref[:k])))
    print("%s: resk[:%d] at %.3g of its bar" % (what, k, err))
    assert np.allclose(resk[:k], resk_ref[:k], rtol=1e-6), (what, err)


def _ids(runs):
    return ["%s-p%d" % r for r in runs]


# ---------------------------------------------------------------------------------------------------------
# A. preconditioner probe
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precd", C.PROBE_A, ids=_ids(C.PROBE_A))
def test_one_iteration_applies_the_preconditioner_like_the_oracle(ipd, name, precd):
    d_ref, it_ref, res_ref, resk_ref = C.reference("A", name, precd)
    d, it, res, resk = run(ipd, "A", name, precd)
    assert it == 1 and it_ref == 1
    assert_d(d, d_ref, "A %s precd %d" % (name, precd))
    assert_history(resk, resk_ref, 1, "A %s precd %d" % (name, precd))
    assert res == resk[0]


# ---------------------------------------------------------------------------------------------------------
# B. recurrence probe
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precd", C.PROBE_B, ids=_ids(C.PROBE_B))
def test_eight_iterations_from_a_guess_match_the_oracle(ipd, name, precd):
    d_ref, it_ref, res_ref, resk_ref = C.reference("B", name, precd)
    d, it, res, resk = run(ipd, "B", name, precd)
    assert it == 8 and it_ref == 8
    assert_d(d, d_ref, "B %s precd %d" % (name, precd))
    assert_history(resk, resk_ref, 8, "B %s precd %d" % (name, precd))
    assert res == resk[7]


@pytest.mark.parametrize("name,precd", [("lap513", 1), ("lap2049", 2), ("hub513", 3), ("hub513", 4), ("big5", 5)])
def test_no_iteration_returns_the_guess(ipd, name, precd):
    o = dict(C.options("B", name, precd), maxit=0)
    d, it, res, resk = ipd.PCG(C.matrix(name), C.rhs(name), o)
    assert it == 0 and res == 1.0 and resk.size == 0
    assert np.array_equal(d, o["guess"])


# ---------------------------------------------------------------------------------------------------------
# C. converged solves: count, residual and d; no history
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precd", C.CONVERGED, ids=_ids(C.CONVERGED))
def test_converged_solve_matches_the_oracle(ipd, name, precd):
    d_ref, it_ref, res_ref, _ = C.reference("C", name, precd)
    A, b = C.matrix(name), C.rhs(name)
    d, it, res, _ = run(ipd, "C", name, precd)
    rel = np.linalg.norm(A @ d - b) / np.linalg.norm(b)
    print("C %s precd %d: it %d (oracle %d), res %.3g (oracle %.3g), residual %.3g" %
          (name, precd, it, it_ref, res, res_ref, rel))
    assert abs(it - it_ref) <= 1
    assert rel <= 1e-9
    assert_d(d, d_ref, "C %s precd %d" % (name, precd))


# ---------------------------------------------------------------------------------------------------------
# D. small ends
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precd,kind", C.SMALL, ids=["%s-p%d-%s" % r for r in C.SMALL])
def test_one_and_two_rows(ipd, name, precd, kind):
    d_ref = C.reference(kind, name, precd)[0]
    d, it, res, _ = run(ipd, kind, name, precd)
    assert_d(d, d_ref, "D %s precd %d" % (name, precd))
    assert_d(d, np.linalg.solve(C.matrix(name).toarray(), C.rhs(name)), "D %s precd %d, direct" % (name, precd))
    assert 1 <= it <= 3


# ---------------------------------------------------------------------------------------------------------
# E. the LDS bound of k_pcg_gen
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precd", C.LDS_BOUND, ids=_ids(C.LDS_BOUND))
def test_seven_thousand_rows_fit_the_lds_resident_solve(ipd, name, precd):
    d_ref, it_ref, _, resk_ref = C.reference("A", name, precd)
    d, it, res, resk = run(ipd, "A", name, precd)
    assert it == 1 and it_ref == 1
    assert_d(d, d_ref, "E %s precd %d" % (name, precd))
    assert_history(resk, resk_ref, 1, "E %s precd %d" % (name, precd))


def test_one_row_more_is_rejected_for_the_lds_resident_solve_only(ipd):
    A, b = C.matrix("tri7001"), C.rhs("tri7001")
    with pytest.raises(ipd.IpdError, match="at most 7000 rows"):
        ipd.PCG(A, b, C.options("A", "tri7001", 3))
    o = dict(guess=None, retol=1e-11, maxit=1000, precd=2)
    d, it, res, _ = ipd.PCG(A, b, o)
    d_ref, it_ref, _, _ = O.PCG(A, b, o)
    assert abs(it - it_ref) <= 1 and it < 100
    assert np.linalg.norm(A @ d - b) <= 1e-9 * np.linalg.norm(b)
    assert_d(d, d_ref, "E tri7001 precd 2")
    assert_d(d, sp.linalg.spsolve(sp.csc_matrix(A), b), "E tri7001 precd 2, direct")


# ---------------------------------------------------------------------------------------------------------
# F. breakdown of IC(0) past the first pass
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["pivot", "missing"])
def test_ichol_breakdown_raises_and_leaves_the_context_usable(ipd, case):
    H = C.pivot_breakdown() if case == "pivot" else C.missing_diagonal()
    b = np.random.RandomState(11).randn(H.shape[0])
    with pytest.raises(ipd.IpdError, match="nonpositive pivot"):
        ipd.PCG(H, b, dict(guess=None, retol=1e-11, maxit=50, precd=4))
    d, it, res, resk = run(ipd, "A", "lap513", 4)                 # the same context, a valid call
    assert it == 1
    assert_d(d, C.reference("A", "lap513", 4)[0], "F after %s" % case)


# ---------------------------------------------------------------------------------------------------------
# G. aug_PCG and PCG4POT on augmented systems of more than BT rows
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pot", [False, True], ids=["aug_PCG", "PCG4POT"])
@pytest.mark.parametrize("mask,seed", C.AUG_MASKS, ids=[m for m, _ in C.AUG_MASKS])
def test_aug_family_matches_the_oracle_and_a_direct_solve(ipd, mask, seed, pot):
    pd = C.aug_problem(mask, seed, pot)
    z_ref, it_ref, res_ref, info_ref = C.aug_reference(mask, seed, pot)
    direct = C.pot_direct(pd)[0] if pot else C.aug_direct(pd)
    z, it, res, info = (ipd.PCG4POT if pot else ipd.aug_PCG)(pd, C.AUG_OPTS)
    e_ref = np.linalg.norm(z - z_ref) / np.linalg.norm(z_ref)
    e_dir = np.linalg.norm(z - direct) / np.linalg.norm(direct)
    print("G %s pot=%d: it %d (oracle %d), info %s, zeta %.3g off the oracle, %.3g off the direct solve" %
          (mask, pot, it, it_ref, list(info), e_ref, e_dir))
    assert list(info) == list(info_ref)
    assert abs(it - it_ref) <= 2
    assert e_ref <= 1e-7
    assert e_dir <= 1e-7
