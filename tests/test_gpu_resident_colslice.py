"""Level 1 of the level-resident kernel in column slices (csrc/ipd_resident.h, res_cs_rows / half1_cs): thread t
holds columns t and t + 512 of the workgroup's rows, a received value is multiplied in the register it arrived
in, and a half sweep is one barrier.  The change is rounding only, so one and two cycles are compared with the
oracle on ragged systems whose first cycle contracts slowly (far above the rounding floor a dropped entry, a
wrong kernel-space scalar or a stale own entry would show), runs must repeat bit for bit, and the timed hook
must still be Class_AMG's kernel.

The three systems (Bernoulli masks with holes, random p and q) coarsen to levels [m + n, m, 1] with rows above
512 entries -- the planner's 16-slice kernel, which also takes the composed level 2 -- and cover a wide F block
over a narrow C block (1000 x 530), the reverse (530 x 1000), and 515 F rows over 128 workgroups (1024 x 515:
about four rows per workgroup, unevenly, and waves without a row).  First-cycle residual of the oracle at
smoth 1, isnsp 1, relative to the start: 1.9e-4, 2.5e-4, 5.5e-4."""
from ctypes import byref, c_int32, create_string_buffer

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ipd_oracle as O
from tests import problems as PR

pytestmark = pytest.mark.gpu

SYSTEMS = [(1000, 530, 0.9), (530, 1000, 0.9), (1024, 515, 0.75)]


@pytest.fixture(scope="module")
def ipd():
    import codes_of_ipd_ssn_amg_method_amd as m
    return m


def options(n, smoth=1, cycle="v", isnsp=1, maxit=30, retol=1e-11):
    return dict(retol=retol, bigph=1, maxit=maxit, theta=0.25, smoth=smoth, cycle=cycle, isnsp=isnsp, inter=1,
                fnode=n)


def kernel_name(h):
    from codes_of_ipd_ssn_amg_method_amd import _lib
    buf = create_string_buffer(64)
    _lib.check(_lib.lib.ipd_amg_resident_kernel(h.handle, buf, c_int32(64), None, None, None))
    return buf.value.decode()


def bench_cycles(h, f, x0, cycles):
    from ctypes import c_double, c_int
    from codes_of_ipd_ssn_amg_method_amd import _lib
    db = _lib.DeviceBuffer.from_array(f)
    dx = _lib.DeviceBuffer.from_array(x0)
    ms, bpc = c_double(), c_double()
    _lib.check(_lib.lib.ipd_amg_bench_cycles(h.handle, db.ptr, dx.ptr, c_int(cycles), byref(ms), byref(bpc)))
    return dx.to_array(np.float64, f.size)


_systems, _oracle = {}, {}


def system(m, n, rho):
    """(Ae, f, guess) of one system, built once."""
    key = (m, n, rho)
    if key not in _systems:
        s = PR.mask_bernoulli(m, n, rho, seed=5)
        pd = PR.make_prob(m, n, s, pq_random=True)
        H0 = O.ASAt(s, pd["p"], pd["q"])
        Ae = sp.csr_matrix(O.build_Ae(H0, pd["T"], pd["p"], pd["q"], pd["bk1"], pd["tk"])[0])
        f = np.concatenate([pd["q"], -pd["p"]]) * pd["z"]
        guess = pd["bk1"] * pd["tk"] * np.random.RandomState(4).random_sample(m + n)
        _systems[key] = (Ae, f, guess)
    return _systems[key]


def oracle_cycles(m, n, rho, opts, cycles=2):
    """The oracle's iterates and residual norms over `cycles` cycles, computed once per system and options."""
    key = (m, n, rho, opts["smoth"], opts["isnsp"], opts["cycle"])
    if key not in _oracle:
        Ae, f, x0 = system(m, n, rho)
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
    Ae, f, guess = system(m, n, rho)
    h = ipd.AMGHierarchy(Ae, opts, ipd.MatlabRand())
    assert kernel_name(h) == "k_resident<16,16,0>", (h.level_sizes(), kernel_name(h))
    if poly2:
        assert h.attach_level2_poly()
        assert kernel_name(h) == "k_resident<16,16,0,true>"
    return h


def check_against_oracle(h, m, n, rho, opts, Ks, res_tol=1e-3, x_tol=1e-9):
    Ae, f, guess = system(m, n, rho)
    xo, reso = oracle_cycles(m, n, rho, opts)
    for K in Ks:
        x = bench_cycles(h, f, guess, K)
        assert np.array_equal(x, bench_cycles(h, f, guess, K)), K          # run to run
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
    the start (the bounds of tests/test_gpu_resident_handoff.py), bit-equal reruns."""
    opts = options(n)
    _, reso = oracle_cycles(m, n, rho, opts)
    assert reso[1] > 1e-4 * reso[0]
    h = hierarchy(ipd, m, n, rho, opts, poly2)
    check_against_oracle(h, m, n, rho, opts, (1, 2))
    h.close()


def test_no_kernel_space_scalar(ipd):
    """isnsp 0: the c = 0 path (the oracle stagnates near 1.2e-2 of the start)."""
    m, n, rho = SYSTEMS[0]
    opts = options(n, isnsp=0)
    h = hierarchy(ipd, m, n, rho, opts, False)
    check_against_oracle(h, m, n, rho, opts, (1, 2))
    h.close()


def test_two_sweeps_mid_sweep_halves(ipd):
    """smoth 2: first halves in mid-run with a non-zero iterate, and the chain of scalars from sweep to sweep.
    The oracle's first cycle ends at 1.96e-9 of the start and the rounding floor lies at 5.8e-11, 3 % of it: the
    residual must agree to 10 % (a wrong scalar or a dropped entry lands orders above)."""
    m, n, rho = SYSTEMS[2]
    opts = options(n, smoth=2)
    h = hierarchy(ipd, m, n, rho, opts, False)
    check_against_oracle(h, m, n, rho, opts, (1,), res_tol=0.1, x_tol=None)
    h.close()


def test_product_path_w_cycle(ipd):
    """smoth 5, W cycle, level 2 as sweeps (two visits): at the rounding floor, so this pins protocol and order
    -- the iterate through A to 1e-9 of the start against MG_Wcycle."""
    m, n, rho = SYSTEMS[0]
    opts = options(n, smoth=5, cycle="w")
    h = hierarchy(ipd, m, n, rho, opts, False)
    check_against_oracle(h, m, n, rho, opts, (1, 2), res_tol=None)
    h.close()


@pytest.mark.parametrize("poly2", [False, True])
def test_bench_hook_is_class_amg_bit_for_bit(ipd, poly2):
    """K timed loop bodies == K iterations of Class_AMG (maxit = K, retol = 0), and == themselves on a rerun."""
    m, n, rho = SYSTEMS[1]
    Ae, f, guess = system(m, n, rho)
    for K in (1, 2):
        h = hierarchy(ipd, m, n, rho, options(n), poly2)
        h2 = hierarchy(ipd, m, n, rho, options(n, maxit=K, retol=0.0), poly2)
        a = bench_cycles(h, f, guess, K)
        assert np.array_equal(a, bench_cycles(h, f, guess, K))
        x2, it2 = h2.solve(f, guess)[:2]
        assert it2 == K and np.array_equal(x2, a)
        assert np.array_equal(h2.solve(f, guess)[0], x2)
        h.close()
        h2.close()


def solve_mode(h):
    """(mode, time-outs counted): mode 2 is the level-resident kernel, 0 the launches."""
    from codes_of_ipd_ssn_amg_method_amd import _lib
    mode, grid, tmo = c_int32(), c_int32(), c_int32()
    _lib.check(_lib.lib.ipd_amg_solve_mode(h.handle, byref(mode), byref(grid), byref(tmo)))
    return mode.value, tmo.value


def test_entry_the_slices_cannot_hold_runs_as_launches(ipd, monkeypatch):
    """A C row with an entry in a C column: the column slices have no slot for it.  The kernel reports it, the
    hierarchy loses its resident plan and solves as launches -- the same iterate as a hierarchy set up without
    the resident kernel (through A to 1e-9 of the start, same iteration count) -- no time-out is counted, and
    the context is not penalised: the next hierarchy still runs resident."""
    m, n, rho = SYSTEMS[1]
    Ae, f, guess = system(m, n, rho)
    B = sp.lil_matrix(Ae)
    i, j = n + 3, n + 7
    assert Ae[i, j] == 0.0
    B[i, j] = B[j, i] = 1e-3 * min(Ae[i, i], Ae[j, j])
    B = sp.csr_matrix(B)
    opts = options(n)
    h = ipd.AMGHierarchy(B, opts, ipd.MatlabRand())
    assert kernel_name(h) == "k_resident<16,16,0>" and solve_mode(h) == (2, 0)
    x, it = h.solve(f, guess)[:2]
    assert solve_mode(h) == (0, 0)
    monkeypatch.setenv("IPD_NO_RESIDENT", "1")
    h0 = ipd.AMGHierarchy(B, opts, ipd.MatlabRand())
    monkeypatch.delenv("IPD_NO_RESIDENT")
    assert solve_mode(h0)[0] == 0
    x0, it0 = h0.solve(f, guess)[:2]
    r0 = np.linalg.norm(B @ guess - f)
    print("it %d / %d, |B(x - x0)|/r0 = %.3e, |Bx - f|/r0 = %.3e, bit-equal %s" % (
        it, it0, np.linalg.norm(B @ (x - x0)) / r0, np.linalg.norm(B @ x - f) / r0, np.array_equal(x, x0)))
    assert it == it0 and np.linalg.norm(B @ (x - x0)) <= 1e-9 * r0
    assert np.linalg.norm(B @ x - f) <= 1e-9 * r0
    h1 = hierarchy(ipd, m, n, rho, opts, False)
    h1.solve(f, guess)
    assert solve_mode(h1) == (2, 0)
    from ctypes import c_int64
    from codes_of_ipd_ssn_amg_method_amd import _lib
    handoffs = c_int64()
    _lib.check(_lib.lib.ipd_amg_resident_kernel(h1.handle, create_string_buffer(64), c_int32(64), byref(handoffs),
                                                None, None))
    assert handoffs.value > 0          # ... and that solve did run in the kernel (a penalised context skips it)
    for hh in (h, h0, h1):
        hh.close()
