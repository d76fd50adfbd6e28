"""AMG-preconditioned CG as ONE single-workgroup launch (ipd_amg_pcg_planned / AMGHierarchy.pcg(planned=True)).

1. it is the one launch where the hierarchy is planned for the single-workgroup solve (pcg_mode), and
   ipd_amg_pcg bit for bit elsewhere and beyond the maxit cap;
2. parity with the numpy restatement on the oracle hierarchy (tests/amg_pcg_ref.py) at
   test_gpu_amg_pcg.py::check_parity's bar;
3. agreement with the launch path on the same hierarchy at the same bar;
4. the operator: one and two iterations against the loop run on the host with the device's launch-path
   cycle, ||A (d - d_host)|| <= 1e-9 ||e|| (the per-cycle bar of tests/test_gpu_cycle.py: the two
   cycles are the same operator summed in different orders);
5. the system on which the stationary iteration stalls;
6. hygiene and edges."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import ipd_oracle as O
from tests import amg_pcg_ref as R
from tests import problems as PR
from tests.test_gpu_amg_pcg import _pin_cases, driver_opts, golden_system, laplacian, opts
from tests.test_gpu_setup import newton_matrix

pytestmark = pytest.mark.gpu

GOLDEN = ["class1_500_k08.npz", "class1_500_k20.npz", "class1_500_k40.npz"]


@pytest.fixture(scope="module")
def ipd():
    import codes_of_ipd_ssn_amg_method_amd as m
    return m


def v1_opts(n):
    """V cycle, one smoothing sweep, otherwise the drivers' options"""
    o = O.amg_options_class1("v")
    o.update(fnode=n, smoth=1)
    return o


def check_parity_planned(ipd, A, e, o, pcg_opts, expect_mode=1):
    """test_gpu_amg_pcg.py::check_parity with pcg(planned=True), and (3) the launch path on the same
    hierarchy at the same bar"""
    ho = O.amg_setup(A, o, O.matlab_rng())
    h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    try:
        d, it, res, resk = h.pcg(e, pcg_opts, planned=True)
        mode = h.pcg_mode
        dl, itl, resl, reskl = h.pcg(e, pcg_opts)
        assert h.pcg_mode == 0
    finally:
        h.close()
    assert mode == expect_mode, mode
    retol = pcg_opts.get("retol", 1e-11)
    dr, itr, resr, reskr = R.amg_pcg(A, e, R.cycle_operator(ho, o), retol=retol,
                                     maxit=pcg_opts.get("maxit", 10000), guess=pcg_opts.get("guess"))
    k = min(it, itr) - 2
    dev = np.max(np.abs(resk[:k] / reskr[:k] - 1)) if k > 0 else 0.0
    kl = min(it, itl) - 2
    devl = np.max(np.abs(resk[:kl] / reskl[:kl] - 1)) if kl > 0 else 0.0
    print("planned it=%d oracle it=%d launched it=%d res=%.3e resk dev oracle %.3e launched %.3e |Ad-e|/|e| %.3e"
          % (it, itr, itl, res, dev, devl, np.linalg.norm(A @ d - e) / np.linalg.norm(e)))
    assert abs(it - itr) <= 1, (it, itr)
    assert np.allclose(resk[:k], reskr[:k], rtol=1e-6), (resk[:k], reskr[:k])
    assert res <= retol, res
    assert np.linalg.norm(A @ d - e) <= 1e-8 * np.linalg.norm(e)
    # (3) against the launch path
    assert abs(it - itl) <= 1, (it, itl)
    assert np.allclose(resk[:kl], reskl[:kl], rtol=1e-6), (resk[:kl], reskl[:kl])
    assert resl <= retol
    return d, it, res, resk


# ---- 1. it is the one launch --------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN)
def test_one_launch_on_golden_systems(ipd, name):
    Ae, f, n = golden_system(name)
    h = ipd.AMGHierarchy(Ae, driver_opts(n), ipd.MatlabRand())
    assert h.pcg_mode == -1
    d, it, res, resk = h.pcg(f, dict(retol=1e-11, maxit=500), planned=True)
    assert h.pcg_mode == 1
    assert it >= 1 and res <= 1e-11
    h.pcg(f, dict(retol=1e-11, maxit=500))
    assert h.pcg_mode == 0
    h.close()


def test_one_launch_on_graph_laplacian_and_maxit_cap(ipd):
    A = laplacian(777, 3)
    e = np.random.RandomState(3).randn(777)
    h = ipd.AMGHierarchy(A, opts("v", isnsp=1), ipd.MatlabRand())
    a = h.pcg(e, dict(retol=1e-11, maxit=1000), planned=True)
    assert h.pcg_mode == 1
    # above the cap the call takes the launch path: ipd_amg_pcg bit for bit
    b = h.pcg(e, dict(retol=1e-11, maxit=1001), planned=True)
    assert h.pcg_mode == 0
    c = h.pcg(e, dict(retol=1e-11, maxit=1001))
    assert b[1] == c[1] and b[2] == c[2] and np.array_equal(b[0], c[0]) and np.array_equal(b[3], c[3])
    assert abs(a[1] - b[1]) <= 1
    h.close()


def test_launch_path_hierarchy_is_bit_identical(ipd):
    A = laplacian(3000, 3)     # levels 3000 / 608 / 61 / ...: not the single-workgroup solve
    e = np.random.RandomState(3).randn(3000)
    po = dict(retol=1e-11, maxit=500)
    h = ipd.AMGHierarchy(A, opts("v", isnsp=1), ipd.MatlabRand())
    a = h.pcg(e, po)
    b = h.pcg(e, po, planned=True)
    assert h.pcg_mode == 0
    assert a[1] == b[1] and a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3])
    h.close()


# ---- 2. / 3. oracle parity, and the launch path on the same hierarchy ----------------------------
@pytest.mark.parametrize("cycle", ["v", "w"])
@pytest.mark.parametrize("isnsp", [0, 1])
@pytest.mark.parametrize("N,seed", [(200, 1), (777, 3)])
def test_parity_graph_laplacian(ipd, N, seed, isnsp, cycle):
    A = laplacian(N, seed)
    e = np.random.RandomState(seed).randn(N)
    check_parity_planned(ipd, A, e, opts(cycle, isnsp=isnsp), dict(retol=1e-11, maxit=500))


@pytest.mark.parametrize("mask", ["tree", "bernoulli"])
def test_parity_newton(ipd, mask):
    if mask == "tree":
        m, n, s = 120, 100, PR.mask_tree(120, 100, seed=4)
    else:
        m, n, s = 60, 40, PR.mask_bernoulli(60, 40, 0.3, seed=5)
    Ae, pd = newton_matrix(m, n, s)
    e = np.random.RandomState(9).randn(m + n)
    check_parity_planned(ipd, Ae, e, driver_opts(n), dict(retol=1e-11, maxit=500))


@pytest.mark.parametrize("variant", ["driver", "v_smoth1"])
@pytest.mark.parametrize("name", GOLDEN)
def test_parity_golden(ipd, name, variant):
    Ae, f, n = golden_system(name)
    o = driver_opts(n) if variant == "driver" else v1_opts(n)
    d, it, res, resk = check_parity_planned(ipd, Ae, f, o, dict(retol=1e-11, maxit=500))
    assert it >= 1


# ---- 4. operator pin -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(5))
def test_operator_pin(ipd, case):
    name, A, o = _pin_cases()[case]
    A = sp.csr_matrix(A)
    N = A.shape[0]
    e = np.random.RandomState(7).randn(N)
    h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    isnsp = int(o["isnsp"])
    if o["cycle"] == "v":
        M = lambda r: ipd.MG_Vcycle(h, r, isnsp, 1)
    else:
        M = lambda r: ipd.MG_Wcycle(h, r, isnsp, 1)
    ne = np.linalg.norm(e)
    for guess in (None, 0.3 * np.random.RandomState(8).randn(N)):
        for maxit in (1, 2):
            po = dict(maxit=maxit, retol=1e-11, guess=guess)
            d, it, res, resk = h.pcg(e, po, planned=True)
            assert h.pcg_mode == 1, name
            de, ite, rese, reske = R.amg_pcg(A, e, M, retol=1e-11, maxit=maxit, guess=guess)
            err = np.linalg.norm(A @ (d - de)) / ne
            print("%s guess=%s maxit=%d ||A(d - d_host)||/||e|| = %.3e" % (name, guess is not None, maxit, err))
            assert it == ite == maxit, (name, it, ite)
            assert err <= 1e-9, (name, guess is None, maxit, err)
    h.close()


# ---- 5. where the stationary iteration stalls ----------------------------------------------------
def test_converges_where_stationary_amg_stalls(ipd):
    N = 500
    A = laplacian(N, 7, eps=1e-3)
    b = np.random.RandomState(2).randn(N)
    o = opts("v", smoth=1, isnsp=0, maxit=50)
    _, it, rel_res, _, rhok = O.Class_AMG(A, b, dict(o), O.matlab_rng())
    assert rel_res > o["retol"] and (it == o["maxit"] or rhok[-1] > 1), (it, rel_res)
    d, itp, res, _ = check_parity_planned(ipd, A, b, o, dict(retol=1e-11, maxit=50))
    assert itp < 50 and res <= 1e-11


# ---- 6. hygiene and edges ------------------------------------------------------------------------
def same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


def test_bits_repeat_and_no_side_effects(ipd):
    Ae, pd = newton_matrix(80, 60, PR.mask_tree(80, 60, seed=3))
    o = driver_opts(60)
    N = Ae.shape[0]
    b = np.random.RandomState(4).randn(N)
    e = np.random.RandomState(5).randn(N)
    B = np.random.RandomState(6).randn(N, 3)
    h = ipd.AMGHierarchy(Ae, o, ipd.MatlabRand())
    po = dict(maxit=300)   # the default maxit (1e4) is beyond the one-launch cap
    before = (h.solve(b), h.pcg(e, po), h.solve_multi(B), h.pcg_multi(B, po))
    r1 = h.pcg(e, po, planned=True)
    assert h.pcg_mode == 1
    r2 = h.pcg(e, po, planned=True)
    after = (h.solve(b), h.pcg(e, po), h.solve_multi(B), h.pcg_multi(B, po))
    assert r1[1] == r2[1] and same(r1, r2)
    for x, y in zip(before, after):
        flat_x = [v for part in x for v in (part if isinstance(part, list) else [part])]
        flat_y = [v for part in y for v in (part if isinstance(part, list) else [part])]
        assert same(flat_x, flat_y)
    h.close()


def test_device_entry_point_equals_host_entry_point(ipd):
    from codes_of_ipd_ssn_amg_method_amd import _lib as L
    Ae, pd = newton_matrix(70, 50, PR.mask_bernoulli(70, 50, 0.25, seed=6))
    o = driver_opts(50)
    N = Ae.shape[0]
    e = np.random.RandomState(6).randn(N)
    g = 0.1 * np.random.RandomState(7).randn(N)
    h = ipd.AMGHierarchy(Ae, o, ipd.MatlabRand())
    d_host, it_host, res_host, resk_host = h.pcg(e, dict(guess=g, maxit=300), planned=True)
    assert h.pcg_mode == 1
    de = L.DeviceBuffer.from_array(e, h.ctx)
    dg = L.DeviceBuffer.from_array(g, h.ctx)
    dd = L.DeviceBuffer(8 * N, h.ctx)
    po = L.ipd_pcg_opts()
    L.lib.ipd_pcg_opts_init(ctypes.byref(po))
    po.maxit = 300
    it = ctypes.c_int64()
    res = ctypes.c_double()
    resk = np.zeros(300)
    L.check(L.lib.ipd_amg_pcg_planned_dev(h.handle, de.ptr, dg.ptr, ctypes.byref(po), dd.ptr, ctypes.byref(it),
                                          ctypes.byref(res), resk.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    d_dev = dd.to_array(np.float64, N)
    assert h.pcg_mode == 1
    assert it.value == it_host and res.value == res_host
    assert np.array_equal(d_dev, d_host) and np.array_equal(resk, resk_host)
    h.close()


def test_edges(ipd):
    A = laplacian(200, 5)
    o = opts("v", isnsp=1)
    h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    d, it, res, _ = h.pcg(np.zeros(200), planned=True)      # default maxit 1e4: as launches
    assert h.pcg_mode == 0
    assert it == 0 and np.isnan(res) and not d.any()
    d, it, res, _ = h.pcg(np.zeros(200), dict(maxit=100), planned=True)
    assert h.pcg_mode == 1
    assert it == 0 and np.isnan(res) and not d.any()
    e = np.random.RandomState(1).randn(200)
    x = spla.spsolve(sp.csc_matrix(A), e)
    d, it, res, _ = h.pcg(e, dict(guess=x, maxit=50), planned=True)
    assert np.all(np.isfinite(d)) and np.linalg.norm(A @ d - e) <= 1e-8 * np.linalg.norm(e)
    with pytest.raises(ipd.IpdError):
        h.pcg(e, dict(precd=2), planned=True)
    h.close()
    for cyc in (1, "x"):
        h = ipd.AMGHierarchy(A, dict(o, cycle=cyc), ipd.MatlabRand())
        with pytest.raises(ipd.IpdError):
            h.pcg(e, dict(maxit=100), planned=True)
        h.close()
    # one-level hierarchy: M is its coarse PCG solve
    A1 = laplacian(2, 0)
    h = ipd.AMGHierarchy(A1, o, ipd.MatlabRand())
    assert h.J == 1
    d, it, res, _ = h.pcg(np.array([1.0, -2.0]), dict(maxit=100), planned=True)
    assert h.pcg_mode == 1
    assert it <= 2 and np.linalg.norm(A1 @ d - [1.0, -2.0]) <= 1e-10
    h.close()
    d, it, res, resk = ipd.AMG_PCG(A, e, o, dict(retol=1e-11, maxit=200), planned=True)
    assert res <= 1e-11 and np.linalg.norm(A @ d - e) <= 1e-8 * np.linalg.norm(e)
