"""AMG-preconditioned conjugate gradients on the device (ipd_amg_pcg / AMGHierarchy.pcg / AMG_PCG).

1. the operator: one and two iterations equal the loop run on the host with the device's own cycle
   (ipd_amg_vcycle / ipd_amg_wcycle) and exact host dots, to 1e-12;
2. parity with the numpy restatement on the oracle hierarchy (tests/amg_pcg_ref.py);
3. a system on which the stationary iteration stalls;
4. the plan modes of the launch path;
5. edges and hygiene."""
import re

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import ipd_oracle as O
from tests import amg_pcg_ref as R
from tests import problems as PR
from tests.test_golden_oracle import load, problem_from
from tests.test_gpu_setup import newton_matrix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ipd():
    import codes_of_ipd_ssn_amg_method_amd as m
    return m


def opts(cycle, smoth=3, isnsp=0, bigph=0, fnode=None, maxit=50):
    return dict(retol=1e-12, bigph=bigph, maxit=maxit, theta=0.25, smoth=smoth, cycle=cycle,
                isnsp=isnsp, inter=1, guess=None, fnode=fnode)


def driver_opts(n):
    o = O.amg_options_class1("w")
    o.update(fnode=n)
    return o


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def laplacian(N, seed, eps=0.5):
    return PR.random_sym_graph_laplacian(N, deg=4, seed=seed, eps=eps)


def check_parity(ipd, A, e, o, pcg_opts, h=None):
    """device vs restatement on the oracle hierarchy: the bar of test_pcg"""
    ho = O.amg_setup(A, o, O.matlab_rng())
    own = h is None
    if own:
        h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    try:
        d, it, res, resk = h.pcg(e, pcg_opts)
    finally:
        if own:
            h.close()
    retol = pcg_opts.get("retol", 1e-11)
    dr, itr, resr, reskr = R.amg_pcg(A, e, R.cycle_operator(ho, o), retol=retol,
                                     maxit=pcg_opts.get("maxit", 10000), guess=pcg_opts.get("guess"))
    assert abs(it - itr) <= 1, (it, itr)
    k = min(it, itr) - 2
    assert np.allclose(resk[:k], reskr[:k], rtol=1e-6), (resk[:k], reskr[:k])
    assert res <= retol, res
    assert np.linalg.norm(A @ d - e) <= 1e-8 * np.linalg.norm(e)
    return d, it, res, resk


# ---- 1. operator pin ------------------------------------------------------------------------
def _pin_cases():
    A1 = laplacian(300, 3)
    Ae, pd = newton_matrix(60, 50, PR.mask_tree(60, 50, seed=2))
    return [("lap_v_nsp0", A1, opts("v", isnsp=0)),
            ("lap_w_nsp1", A1, opts("w", isnsp=1)),
            ("newton_v_nsp1_bigph", Ae, opts("v", smoth=5, isnsp=1, bigph=1, fnode=50)),
            ("newton_w_nsp0_bigph", Ae, opts("w", smoth=5, isnsp=0, bigph=1, fnode=50)),
            ("newton_w_nsp1_bigph", Ae, driver_opts(50))]


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
    for guess in (None, 0.3 * np.random.RandomState(8).randn(N)):
        for maxit in (1, 2):
            po = dict(maxit=maxit, retol=1e-11, guess=guess)
            d, it, res, resk = h.pcg(e, po)
            de, ite, rese, reske = R.amg_pcg(A, e, M, retol=1e-11, maxit=maxit, guess=guess)
            assert it == ite == maxit, (name, it, ite)
            assert rel(d, de) <= 1e-12, (name, guess is None, maxit, rel(d, de))
            # res is a ratio of dots of a residual reduced by orders of magnitude (cancellation)
            assert abs(res - rese) <= 1e-9 * rese, (name, res, rese)
            assert np.allclose(resk[:it], reske, rtol=1e-9, atol=0)
    h.close()


# ---- 2. oracle parity -----------------------------------------------------------------------
@pytest.mark.parametrize("N,seed,cycle", [(200, 1, "v"), (200, 2, "w"), (777, 3, "v"), (777, 4, "w")])
def test_parity_graph_laplacian(ipd, N, seed, cycle):
    A = laplacian(N, seed)
    e = np.random.RandomState(seed).randn(N)
    check_parity(ipd, A, e, opts(cycle, isnsp=seed % 2), dict(retol=1e-11, maxit=500))


@pytest.mark.parametrize("mask", ["tree", "bernoulli"])
def test_parity_newton(ipd, mask):
    if mask == "tree":
        m, n, s = 120, 100, PR.mask_tree(120, 100, seed=4)
    else:
        m, n, s = 60, 40, PR.mask_bernoulli(60, 40, 0.3, seed=5)
    Ae, pd = newton_matrix(m, n, s)
    e = np.random.RandomState(9).randn(m + n)
    check_parity(ipd, Ae, e, driver_opts(n), dict(retol=1e-11, maxit=500))


def golden_system(name="class1_500_k08.npz"):
    g = load(name)
    pd = problem_from(g)
    H0 = O.ASAt(pd["s"], pd["p"], pd["q"])
    Ae = O.build_Ae(H0, pd["T"], pd["p"], pd["q"], pd["bk1"], pd["tk"])[0]
    f = np.concatenate([pd["q"], -pd["p"]]) * pd["z"]
    return sp.csr_matrix(Ae), f, pd["n"]


def test_parity_golden_driver_system(ipd):
    Ae, f, n = golden_system()
    d, it, res, resk = check_parity(ipd, Ae, f, driver_opts(n), dict(retol=1e-11, maxit=500))
    assert it >= 1


# ---- 3. where the stationary iteration stalls -------------------------------------------------
def test_converges_where_stationary_amg_stalls(ipd):
    N = 500
    A = laplacian(N, 7, eps=1e-3)
    b = np.random.RandomState(2).randn(N)
    o = opts("v", smoth=1, isnsp=0, maxit=50)
    _, it, rel_res, _, rhok = O.Class_AMG(A, b, dict(o), O.matlab_rng())
    assert rel_res > o["retol"] and (it == o["maxit"] or rhok[-1] > 1), (it, rel_res)
    d, itp, res, _ = check_parity(ipd, A, b, o, dict(retol=1e-11, maxit=50))
    assert itp < 50 and res <= 1e-11


# ---- 4. plan modes ----------------------------------------------------------------------------
def _k_sub(capfd, ipd, A, o, monkeypatch):
    monkeypatch.setenv("IPD_DEBUG_LEVELS", "1")
    capfd.readouterr()
    h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    err = capfd.readouterr().err
    monkeypatch.delenv("IPD_DEBUG_LEVELS")
    m = re.findall(r"k_sub=(\d+)", err)
    return h, int(m[-1]) if m else -1


def test_plan_modes(ipd, monkeypatch, capfd):
    A = laplacian(3000, 3)     # levels 3000 / 608 / 61 / ...: levels >= 3 run as the sub-cycle
    e = np.random.RandomState(3).randn(3000)
    o = opts("v", isnsp=1)
    po = dict(retol=1e-11, maxit=500)
    h, ks = _k_sub(capfd, ipd, A, o, monkeypatch)
    assert ks >= 1, "expected the lower levels to run as the single-workgroup sub-cycle"
    d0, it0, _, _ = check_parity(ipd, A, e, o, po, h)
    h.close()
    monkeypatch.setenv("IPD_NO_SUBCYCLE", "1")
    h, ks = _k_sub(capfd, ipd, A, o, monkeypatch)
    assert ks == 0
    d1, it1, _, _ = check_parity(ipd, A, e, o, po, h)
    h.close()
    monkeypatch.delenv("IPD_NO_SUBCYCLE")
    # padded rows of level 1 (the Newton systems' default) against the CSR walk
    Ae, f, n = golden_system()
    do = driver_opts(n)
    dp, itp, _, _ = check_parity(ipd, Ae, f, do, po)
    monkeypatch.setenv("IPD_NO_PAD", "1")
    dc, itc, _, _ = check_parity(ipd, Ae, f, do, po)
    monkeypatch.delenv("IPD_NO_PAD")
    assert abs(itp - itc) <= 1 and abs(it0 - it1) <= 1


# ---- 5. edges and hygiene -----------------------------------------------------------------------
def test_edges(ipd):
    A = laplacian(200, 5)
    o = opts("v", isnsp=1)
    h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    d, it, res, _ = h.pcg(np.zeros(200))
    assert it == 0 and np.isnan(res) and not d.any()
    e = np.random.RandomState(1).randn(200)
    x = spla.spsolve(sp.csc_matrix(A), e)
    d, it, res, _ = h.pcg(e, dict(guess=x, maxit=50))
    assert np.all(np.isfinite(d)) and np.linalg.norm(A @ d - e) <= 1e-8 * np.linalg.norm(e)
    with pytest.raises(ipd.IpdError):
        h.pcg(e, dict(precd=2))
    h.close()
    for cyc in (1, "x"):
        h = ipd.AMGHierarchy(A, dict(o, cycle=cyc), ipd.MatlabRand())
        with pytest.raises(ipd.IpdError):
            h.pcg(e)
        h.close()
    # one-level hierarchy: M is its coarse PCG solve
    A1 = laplacian(2, 0)
    h = ipd.AMGHierarchy(A1, o, ipd.MatlabRand())
    assert h.J == 1
    d, it, res, _ = h.pcg(np.array([1.0, -2.0]))
    assert it <= 2 and np.linalg.norm(A1 @ d - [1.0, -2.0]) <= 1e-10
    h.close()
    d, it, res, resk = ipd.AMG_PCG(A, e, o, dict(retol=1e-11, maxit=200))
    assert res <= 1e-11 and np.linalg.norm(A @ d - e) <= 1e-8 * np.linalg.norm(e)


def test_bits_repeat_and_no_side_effect_on_solve(ipd):
    Ae, pd = newton_matrix(80, 60, PR.mask_tree(80, 60, seed=3))
    o = driver_opts(60)
    N = Ae.shape[0]
    b = np.random.RandomState(4).randn(N)
    e = np.random.RandomState(5).randn(N)
    h = ipd.AMGHierarchy(Ae, o, ipd.MatlabRand())
    x0 = h.solve(b)
    r1 = h.pcg(e)
    r2 = h.pcg(e)
    x1 = h.solve(b)
    assert r1[1] == r2[1] and np.array_equal(r1[0], r2[0]) and np.array_equal(r1[3], r2[3])
    assert x0[1] == x1[1] and np.array_equal(x0[0], x1[0]) and np.array_equal(x0[3], x1[3])
    h.close()


def test_device_entry_point_equals_host_entry_point(ipd):
    import ctypes
    from codes_of_ipd_ssn_amg_method_amd import _lib as L
    Ae, pd = newton_matrix(70, 50, PR.mask_bernoulli(70, 50, 0.25, seed=6))
    o = driver_opts(50)
    N = Ae.shape[0]
    e = np.random.RandomState(6).randn(N)
    g = 0.1 * np.random.RandomState(7).randn(N)
    h = ipd.AMGHierarchy(Ae, o, ipd.MatlabRand())
    d_host, it_host, res_host, resk_host = h.pcg(e, dict(guess=g, maxit=300))
    de = L.DeviceBuffer.from_array(e, h.ctx)
    dg = L.DeviceBuffer.from_array(g, h.ctx)
    dd = L.DeviceBuffer(8 * N, h.ctx)
    po = L.ipd_pcg_opts()
    L.lib.ipd_pcg_opts_init(ctypes.byref(po))
    po.maxit = 300
    it = ctypes.c_int64()
    res = ctypes.c_double()
    resk = np.zeros(300)
    L.check(L.lib.ipd_amg_pcg_dev(h.handle, de.ptr, dg.ptr, ctypes.byref(po), dd.ptr, ctypes.byref(it),
                                  ctypes.byref(res), resk.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    d_dev = dd.to_array(np.float64, N)
    assert it.value == it_host and res.value == res_host
    assert np.array_equal(d_dev, d_host) and np.array_equal(resk, resk_host)
    h.close()
