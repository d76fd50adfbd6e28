"""The column-slice resident kernel with its level 1 <-> 2 transfers from the bit mask (csrc/ipd_resident.h,
k_resident<16,16,0> and <16,16,0,true>): the hand-offs between the level-1 half sweeps -- the residual, the
restriction, level 2, the prolongation -- and the composed level-2 pass that is fed from the polls of r_2
(poly2_fed: the received r_2 meets the column slices of B in registers, one barrier, e_2 published from registers).
What changes there is summation order only, so one and two cycles are compared with the oracle on ragged systems
whose first cycle contracts slowly: a dropped term, a wrong column or a stale entry then shows orders above the
rounding floor.  Runs repeat bit for bit, the timed hook is Class_AMG's kernel, and the stamped hook (stamps by
class of hand-off) returns the unstamped iterate.

The three systems (Bernoulli masks with holes, seed 5, random p and q) coarsen to levels [m + n, m, 1] with rows
above 512 entries, the smallest that reach the 16-slice kernel: a wide F block over a narrow C block (1000 x 530),
the reverse (530 x 1000), and 515 F rows over 128 workgroups (1024 x 515: about four rows per workgroup, unevenly,
and waves without a row).  Every hierarchy attaches the mask transfers with the system's own p, q, tk, and every
test checks that they are in use and which kernel runs: the paths under test would otherwise silently not run."""
from ctypes import byref, c_double, c_int, c_int32, c_int64, create_string_buffer

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ipd_oracle as O
from tests import problems as PR

pytestmark = pytest.mark.gpu

SYSTEMS = [(1000, 530, 0.9), (530, 1000, 0.9), (1024, 515, 0.75)]
KERNELS = {False: "k_resident<16,16,0>", True: "k_resident<16,16,0,true>"}


@pytest.fixture(scope="module")
def ipd():
    import codes_of_ipd_ssn_amg_method_amd as m
    return m


def options(n, smoth=1, cycle="v", isnsp=1, maxit=30, retol=1e-11):
    return dict(retol=retol, bigph=1, maxit=maxit, theta=0.25, smoth=smoth, cycle=cycle, isnsp=isnsp, inter=1,
                fnode=n)


def resident_kernel(h):
    """(name, hand-offs of the last launch, transfers from the bit mask)"""
    from codes_of_ipd_ssn_amg_method_amd import _lib
    buf = create_string_buffer(64)
    handoffs, xm = c_int64(), c_int32()
    _lib.check(_lib.lib.ipd_amg_resident_kernel(h.handle, buf, c_int32(64), byref(handoffs), None, byref(xm)))
    return buf.value.decode(), handoffs.value, xm.value


def run_cycles(h, f, x0, cycles):
    from codes_of_ipd_ssn_amg_method_amd import _lib
    db = _lib.DeviceBuffer.from_array(f)
    dx = _lib.DeviceBuffer.from_array(x0)
    ms, bpc = c_double(), c_double()
    _lib.check(_lib.lib.ipd_amg_bench_cycles(h.handle, db.ptr, dx.ptr, c_int(cycles), byref(ms), byref(bpc)))
    return dx.to_array(np.float64, f.size)


def run_cycles_stamped(h, f, x0, cycles):
    """(iterate, the 32 stamp words) of ipd_amg_bench_resident_classes"""
    from codes_of_ipd_ssn_amg_method_amd import _lib
    db = _lib.DeviceBuffer.from_array(f)
    dx = _lib.DeviceBuffer.from_array(x0)
    ms = c_double()
    st = (c_int64 * 32)()
    _lib.check(_lib.lib.ipd_amg_bench_resident_classes(h.handle, db.ptr, dx.ptr, c_int(cycles), byref(ms), st))
    return dx.to_array(np.float64, f.size), [int(v) for v in st]


_systems, _oracle = {}, {}


def system(m, n, rho):
    """(Ae, f, guess, p, q, tk) of one system, built once."""
    key = (m, n, rho)
    if key not in _systems:
        s = PR.mask_bernoulli(m, n, rho, seed=5)
        pd = PR.make_prob(m, n, s, pq_random=True)
        H0 = O.ASAt(s, pd["p"], pd["q"])
        Ae = sp.csr_matrix(O.build_Ae(H0, pd["T"], pd["p"], pd["q"], pd["bk1"], pd["tk"])[0])
        f = np.concatenate([pd["q"], -pd["p"]]) * pd["z"]
        guess = pd["bk1"] * pd["tk"] * np.random.RandomState(4).random_sample(m + n)
        _systems[key] = (Ae, f, guess, pd["p"], pd["q"], pd["tk"])
    return _systems[key]


def oracle_cycles(m, n, rho, opts, cycles=2):
    """The oracle's iterates and residual norms over `cycles` cycles, computed once per system and options."""
    key = (m, n, rho, opts["smoth"], opts["isnsp"], opts["cycle"])
    if key not in _oracle:
        Ae, f, x0 = system(m, n, rho)[:3]
        o = dict(opts)
        o.update(guess=x0)
        h = O.amg_setup(Ae, o, O.matlab_rng())
        assert [a.shape[0] for a in h.Ack[1:]] == [m + n, m, 1], [a.shape[0] for a in h.Ack[1:]]
        A = h.Ack[1]
        mg = O.MG_Wcycle if opts["cycle"] == "w" else O.MG_Vcycle
        x = x0.copy()
        xs, res = [], [np.linalg.norm(A @ x - f)]
        for _ in range(cycles):
            x = x + mg(h, f - A @ x, opts["isnsp"])
            xs.append(x.copy())
            res.append(np.linalg.norm(A @ x - f))
        _oracle[key] = (xs, np.array(res))
    return _oracle[key]


def hierarchy(ipd, m, n, rho, opts, poly2):
    """A hierarchy of the system with the mask transfers attached (and level 2 composed), checked to run them."""
    Ae, f, guess, p, q, tk = system(m, n, rho)
    h = ipd.AMGHierarchy(Ae, opts, ipd.MatlabRand())
    assert h.attach_mask_transfers(p, q, tk)
    if poly2:
        assert h.attach_level2_poly()
    name, _, xm = resident_kernel(h)
    assert name == KERNELS[poly2] and xm == 1, (h.level_sizes(), name, xm)
    return h


def check_against_oracle(h, m, n, rho, opts, Ks, res_tol=1e-3, x_tol=1e-9):
    Ae, f, guess = system(m, n, rho)[:3]
    xo, reso = oracle_cycles(m, n, rho, opts)
    for K in Ks:
        x = run_cycles(h, f, guess, K)
        assert np.array_equal(x, run_cycles(h, f, guess, K)), K          # run to run
        r = np.linalg.norm(Ae @ x - f)
        dx = np.linalg.norm(Ae @ (x - xo[K - 1]))
        print("K=%d r=%.6e oracle=%.6e |r-ro|/ro=%.3e |A(x-xo)|/r0=%.3e" % (
            K, r, reso[K], abs(r - reso[K]) / reso[K], dx / reso[0]))
        if res_tol is not None:
            assert abs(r - reso[K]) <= res_tol * reso[K], (K, r, reso[K])
        if x_tol is not None:
            assert dx <= x_tol * reso[0], (K, dx, reso[0])


@pytest.mark.parametrize("m,n,rho", SYSTEMS)
@pytest.mark.parametrize("poly2", [False, True])
def test_one_sweep_cycles_against_oracle(ipd, m, n, rho, poly2):
    """smoth 1: the residual after one and two cycles to 1e-3 of the oracle's, the iterate through A to 1e-9 of
    the start, bit-equal reruns.  The oracle's first cycle contracts only to 1.9e-4 / 2.5e-4 / 5.5e-4 of the start
    (checked, not assumed), so a dropped term shows orders above the rounding floor."""
    opts = options(n)
    _, reso = oracle_cycles(m, n, rho, opts)
    assert reso[1] > 1e-4 * reso[0]
    h = hierarchy(ipd, m, n, rho, opts, poly2)
    check_against_oracle(h, m, n, rho, opts, (1, 2))
    h.close()


@pytest.mark.parametrize("poly2", [False, True])
def test_no_kernel_space_scalar(ipd, poly2):
    """isnsp 0: the c = 0 path (no 1'r_2 term in the composed pass either)."""
    m, n, rho = SYSTEMS[0]
    opts = options(n, isnsp=0)
    _, reso = oracle_cycles(m, n, rho, opts)
    assert reso[1] > 1e-4 * reso[0]
    h = hierarchy(ipd, m, n, rho, opts, poly2)
    check_against_oracle(h, m, n, rho, opts, (1, 2))
    h.close()


def test_two_sweeps_mid_sweep_halves(ipd):
    """smoth 2 on the (1024, 515) system: first halves in mid-run with a non-zero iterate.  The oracle's first cycle
    ends at 1.96e-9 of the start and the rounding floor lies at 3 % of it: the residual must agree to 10 %."""
    m, n, rho = SYSTEMS[2]
    opts = options(n, smoth=2)
    h = hierarchy(ipd, m, n, rho, opts, False)
    check_against_oracle(h, m, n, rho, opts, (1,), res_tol=0.1, x_tol=None)
    h.close()


def test_w_cycle_sweep_form_with_mask_transfers(ipd):
    """smoth 5, W cycle, level 2 as sweeps (two visits, the second from a non-zero iterate), mask transfers: the
    iterate through A to 1e-9 of the start against MG_Wcycle."""
    m, n, rho = SYSTEMS[0]
    opts = options(n, smoth=5, cycle="w")
    h = hierarchy(ipd, m, n, rho, opts, False)
    check_against_oracle(h, m, n, rho, opts, (1, 2), res_tol=None)
    h.close()


@pytest.mark.parametrize("poly2", [False, True])
def test_bench_hook_is_class_amg_bit_for_bit(ipd, poly2):
    """K timed loop bodies == K iterations of Class_AMG (maxit = K, retol = 0), and == themselves on a rerun."""
    m, n, rho = SYSTEMS[1]
    Ae, f, guess = system(m, n, rho)[:3]
    for K in (1, 2):
        h = hierarchy(ipd, m, n, rho, options(n), poly2)
        h2 = hierarchy(ipd, m, n, rho, options(n, maxit=K, retol=0.0), poly2)
        a = run_cycles(h, f, guess, K)
        assert np.array_equal(a, run_cycles(h, f, guess, K))
        x2, it2 = h2.solve(f, guess)[:2]
        assert it2 == K and np.array_equal(x2, a)
        assert np.array_equal(h2.solve(f, guess)[0], x2)
        h.close()
        h2.close()


@pytest.mark.parametrize("poly2", [False, True])
def test_stamped_hook_same_iterate_and_counts(ipd, poly2):
    """The hook with stamps by class returns the unstamped hook's bits for K = 2; its per-class hand-off counts add
    up to the hand-offs the library reports for the launch, one of them per cycle starts a run of half sweeps behind
    a barrier of its own (the post run is fed by the prolongation), and every class took time."""
    m, n, rho = SYSTEMS[2]
    Ae, f, guess = system(m, n, rho)[:3]
    h = hierarchy(ipd, m, n, rho, options(n), poly2)
    K = 2
    a = run_cycles(h, f, guess, K)
    x, st = run_cycles_stamped(h, f, guess, K)
    assert np.array_equal(x, a)
    total = resident_kernel(h)[1]
    clocks, counts = st[16:24], st[24:32]
    print("hand-offs %d, stamps[2] %d, per class %s, clocks %s" % (total, st[2], counts, clocks))
    assert sum(counts) == total == st[2]
    # one top per loop body and one ahead of the loop; smoth 1: the pre run is one half sweep (its first half is
    # formed locally) that starts the run, the post run two that are fed
    assert counts[6] == K + 1 and counts[1] == K and counts[0] == 2 * K
    assert counts[2] == counts[3] == counts[5] == K
    assert counts[4] == total - 6 * K - (K + 1) and (counts[4] == K or not poly2)
    assert all(c > 0 for c, k in zip(clocks, counts) if k) and all(c == 0 for c, k in zip(clocks, counts) if not k)
    assert sum(clocks) <= st[1]
    h.close()
