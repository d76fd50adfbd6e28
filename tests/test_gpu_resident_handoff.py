"""The level-resident kernel's hand-off (csrc/ipd_resident.h, RES_HANDOFF_P): work that does not need the
received values runs before the wait, and the level-1/2 row dots use fused multiply-adds.  Both change
rounding only, so the checks are: the timed hook and Class_AMG still run the same kernel (bit for bit),
runs repeat bit for bit, and one and two cycles agree with the oracle on a system whose first cycle
contracts by less than 1e-4 -- far above the rounding floor, where a wrong kernel-space scalar would
show (the dense metric system reaches the floor after one cycle)."""
from ctypes import byref, c_int32, create_string_buffer

import numpy as np
import pytest
import scipy.sparse as sp

import bench
from oracle import ipd_oracle as O
from tests import problems as PR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ipd():
    import codes_of_ipd_ssn_amg_method_amd as m
    return m


def options(n, smoth=5, maxit=30, retol=1e-11):
    return dict(retol=retol, bigph=1, maxit=maxit, theta=0.25, smoth=smoth, cycle="v", isnsp=1, inter=1,
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


def oracle_cycles(Ae, f, x0, opts, cycles):
    o = dict(opts)
    o.update(guess=x0)
    h = O.amg_setup(Ae, o, O.matlab_rng())
    A = h.Ack[1]
    x = x0.copy()
    xs, res = [], [np.linalg.norm(A @ x - f)]
    for _ in range(cycles):
        x = x + O.MG_Vcycle(h, f - A @ x, opts["isnsp"])
        xs.append(x.copy())
        res.append(np.linalg.norm(A @ x - f))
    return xs, np.array(res)


@pytest.fixture(scope="module")
def metric_system(ipd):
    m = n = 1024
    s = bench.build_mask(m, n, "bernoulli", 1.0)
    Ae, f, guess, H0 = bench.build_newton_system(ipd, m, n, s)
    return m, n, Ae, f, guess


@pytest.mark.parametrize("poly2", [True, False])
def test_metric_bench_hook_is_class_amg_bit_for_bit(ipd, metric_system, poly2):
    """K timed loop bodies (ipd_amg_bench_cycles) == K iterations of Class_AMG, and == themselves on a rerun.
    (K <= 2: the system reaches the rounding floor after one cycle, and from there Class_AMG stops at the
    first cycle whose residual rises -- Class_AMG.m:106 -- even with retol = 0.)"""
    m, n, Ae, f, guess = metric_system
    want = "k_resident<16,16,0,true>" if poly2 else "k_resident<16,16,0>"
    for K in (1, 2):
        h = ipd.AMGHierarchy(Ae, options(n), ipd.MatlabRand())
        h2 = ipd.AMGHierarchy(Ae, options(n, maxit=K, retol=0.0), ipd.MatlabRand())
        for hh in (h, h2):
            assert hh.attach_mask_transfers(np.ones(m), np.ones(n), bench.TK)
            if poly2:
                assert hh.attach_level2_poly()
            assert kernel_name(hh) == want
        a = bench_cycles(h, f, guess, K)
        assert np.array_equal(a, bench_cycles(h, f, guess, K))          # run to run
        x2, it2, rel2, relk2, rho2 = h2.solve(f, guess)
        assert it2 == K and np.array_equal(x2, a)
        x3 = h2.solve(f, guess)[0]
        assert np.array_equal(x3, x2)
        A = sp.csr_matrix(Ae)
        assert np.linalg.norm(A @ a - f) < np.linalg.norm(A @ guess - f)
        h.close()
        h2.close()


@pytest.mark.parametrize("m,n,rho", [(700, 900, 0.9), (600, 760, 0.7)])
@pytest.mark.parametrize("poly2", [False, True])
def test_slow_first_cycle_against_oracle(ipd, m, n, rho, poly2):
    """Ragged dense systems with a mask that has holes and one pre-/post-sweep (smoth 1): the first cycle only
    contracts the residual to 2e-4 / 1e-3 of its start, so the iterate after one and after two cycles is
    compared with the oracle's far above the rounding floor.

    Only smoth 1: no system the composed form takes (three levels, a one-row tail, rows above 512 entries)
    was found whose first cycle contracts by no more than 1e-4 at smoth >= 2.  Measured with the oracle over
    19 Bernoulli systems (m, n from 600 x 760 to 1000 x 1000, rho 0.6-1.0, random p and q): the slowest first
    cycle contracts to 2.6e-8 at smoth 2 (600 x 760, rho 0.6) and to 5.4e-10 at smoth 5 (1000 x 1000,
    rho 1), while the two systems of this test contract to 2.1e-4 / 9.7e-4 at smoth 1.  Masks of two weakly coupled
    dense blocks contract slowly (1e-3 - 1e-5 at any smoth) but coarsen to a two-row tail.  The composed
    operator at smoth 5 is pinned entrywise instead (tests/test_gpu_poly_operators.py)."""
    s = PR.mask_bernoulli(m, n, rho, seed=5)
    pd = PR.make_prob(m, n, s, pq_random=True)
    H0 = O.ASAt(s, pd["p"], pd["q"])
    Ae = sp.csr_matrix(O.build_Ae(H0, pd["T"], pd["p"], pd["q"], pd["bk1"], pd["tk"])[0])
    f = np.concatenate([pd["q"], -pd["p"]]) * pd["z"]
    guess = pd["bk1"] * pd["tk"] * np.random.RandomState(4).random_sample(m + n)
    opts = options(n, smoth=1)
    h = ipd.AMGHierarchy(Ae, opts, ipd.MatlabRand())
    assert kernel_name(h).startswith("k_resident<16,16,0"), (h.level_sizes(), kernel_name(h))
    if poly2:
        assert h.attach_level2_poly()
        assert kernel_name(h) == "k_resident<16,16,0,true>"
    xo, reso = oracle_cycles(Ae, f, guess, opts, 2)
    assert reso[1] > 1e-4 * reso[0]
    A = sp.csr_matrix(Ae)
    for K in (1, 2):
        x = bench_cycles(h, f, guess, K)
        assert np.array_equal(x, bench_cycles(h, f, guess, K))
        r = np.linalg.norm(A @ x - f)
        # the residual to 1e-3 of itself (the floor of any summation order lies near 4e-11 of the start, still
        # below 1e-3 of the second cycle's), the iterate through A to 1e-9 of the start
        assert abs(r - reso[K]) <= 1e-3 * reso[K], (K, r, reso[K])
        assert np.linalg.norm(A @ (x - xo[K - 1])) <= 1e-9 * reso[0], K
    h.close()
