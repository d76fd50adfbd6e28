"""AMG-preconditioned CG for several right-hand sides on the device (ipd_amg_pcg_multi /
AMGHierarchy.pcg_multi / AMG_PCG_multi): every column as if solved alone.

1. the operator: one and two iterations equal the loop run on the host with the device's own
   single-vector cycle, per column;
2. per-column parity with the numpy restatement on the oracle hierarchy (tests/amg_pcg_ref.py);
3. agreement with ipd_amg_pcg on the same hierarchy in every plan mode (0, 1, 2);
4. mixed stopping inside one block (frozen columns);
5. independence of the other columns and run-to-run determinism;
6. chunking (nrhs > 8) and lde > N;
7. hierarchy shapes: 1, 2, >= 4 levels, smoth = 0, Jacobi and bigraph smoothers, a mask operator;
8. edges and side effects.
Not covered: the IPD_E_ARG case of a hierarchy sharded over ranks (no call of the public interface
reaches it on one GPU; see tests/test_gpu_amg_multi.py)."""
import ctypes
import os
from contextlib import contextmanager

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ipd_oracle as O
from tests import amg_pcg_ref as R
from tests import problems as PR
from tests.test_gpu_amg_pcg import _pin_cases, driver_opts, golden_system, laplacian, opts, rel
from tests.test_gpu_setup import newton_matrix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ipd():
    import codes_of_ipd_ssn_amg_method_amd as m
    return m


@contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def solve_mode(h):
    from codes_of_ipd_ssn_amg_method_amd import _lib
    mode, grid, tmo = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _lib.check(_lib.lib.ipd_amg_solve_mode(h.handle, ctypes.byref(mode), ctypes.byref(grid), ctypes.byref(tmo)))
    return mode.value


def rhs(N, k, seed):
    return np.random.RandomState(seed).randn(N, k)


def newton_system(m, n, s, k, seed=7):
    Ae, pd = newton_matrix(m, n, s)
    rs = np.random.RandomState(seed)
    f = np.concatenate([pd["q"], -pd["p"]]) * pd["z"]
    E = np.column_stack([f * (1.0 + 0.1 * j) + 0.05 * rs.standard_normal(m + n) for j in range(k)])
    return sp.csr_matrix(Ae), E, pd


def same_bits(a, b):
    """two pcg_multi results (D, it, res, resk) are the same bits"""
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            and np.array_equal(a[2], b[2], equal_nan=True) and np.array_equal(a[3], b[3]))


def agree_with_singles(h, A, E, po, same_it=True):
    """every column of pcg_multi agrees with ipd_amg_pcg on the same hierarchy to rounding"""
    out = h.pcg_multi(E, po)
    D, it, res, resk = out
    for j in range(E.shape[1]):
        g = None if po.get("guess") is None else po["guess"][:, j]
        d, its, ress, resks = h.pcg(E[:, j], dict(po, guess=g))
        if same_it:
            assert it[j] == its, (j, it[j], its)
        else:
            assert abs(it[j] - its) <= 1, (j, it[j], its)
        k = max(0, min(it[j], its) - 2)
        assert np.allclose(resk[:k, j], resks[:k], rtol=1e-6, atol=0), (j, resk[:k, j], resks[:k])
        assert not resk[it[j]:, j].any()
        ne = np.linalg.norm(E[:, j])
        assert np.linalg.norm(A @ (D[:, j] - d)) <= 1e-8 * ne, j
        assert np.linalg.norm(A @ D[:, j] - E[:, j]) <= 1e-8 * ne, j
    return out


# ---- 1. operator pin ------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(5))
def test_operator_pin(ipd, case):
    name, A, o = _pin_cases()[case]
    A = sp.csr_matrix(A)
    N = A.shape[0]
    E = rhs(N, 3, 7)
    h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    isnsp = int(o["isnsp"])
    if o["cycle"] == "v":
        M = lambda r: ipd.MG_Vcycle(h, r, isnsp, 1)
    else:
        M = lambda r: ipd.MG_Wcycle(h, r, isnsp, 1)
    for G in (None, 0.3 * rhs(N, 3, 8)):
        for maxit in (1, 2):
            D, it, res, resk = h.pcg_multi(E, dict(maxit=maxit, retol=1e-11, guess=G))
            for j in range(3):
                de, ite, rese, reske = R.amg_pcg(A, E[:, j], M, retol=1e-11, maxit=maxit,
                                                 guess=None if G is None else G[:, j])
                assert it[j] == ite == maxit, (name, j, it[j], ite)
                assert rel(D[:, j], de) <= 1e-10, (name, j, G is None, maxit, rel(D[:, j], de))
                assert np.allclose(resk[:maxit, j], reske, rtol=1e-8, atol=0), (name, j, resk[:, j], reske)
    h.close()


# ---- 2. oracle parity per column -------------------------------------------------------------
def check_parity_multi(ipd, A, E, o, po):
    """the bar of test_gpu_amg_pcg.check_parity, column by column"""
    ho = O.amg_setup(A, o, O.matlab_rng())
    h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    try:
        D, it, res, resk = h.pcg_multi(E, po)
    finally:
        h.close()
    retol = po.get("retol", 1e-11)
    M = R.cycle_operator(ho, o)
    for j in range(E.shape[1]):
        e = E[:, j]
        dr, itr, resr, reskr = R.amg_pcg(A, e, M, retol=retol, maxit=po.get("maxit", 10000))
        assert abs(it[j] - itr) <= 1, (j, it[j], itr)
        k = max(0, min(it[j], itr) - 2)
        assert np.allclose(resk[:k, j], reskr[:k], rtol=1e-6), (j, resk[:k, j], reskr[:k])
        assert res[j] <= retol, (j, res[j])
        assert np.linalg.norm(A @ D[:, j] - e) <= 1e-8 * np.linalg.norm(e), j
    return D, it, res, resk


@pytest.mark.parametrize("N,seed,cycle,isnsp", [(200, 1, "v", 0), (200, 2, "w", 1), (300, 3, "v", 1),
                                                (300, 4, "w", 0)])
def test_parity_graph_laplacian(ipd, N, seed, cycle, isnsp):
    A = laplacian(N, seed)
    check_parity_multi(ipd, A, rhs(N, 3, seed), opts(cycle, isnsp=isnsp), dict(retol=1e-11, maxit=500))


@pytest.mark.parametrize("mask", ["tree", "bernoulli"])
def test_parity_newton(ipd, mask):
    if mask == "tree":
        m, n, s = 120, 100, PR.mask_tree(120, 100, seed=4)
    else:
        m, n, s = 60, 40, PR.mask_bernoulli(60, 40, 0.3, seed=5)
    A, E, _ = newton_system(m, n, s, 3)
    check_parity_multi(ipd, A, E, driver_opts(n), dict(retol=1e-11, maxit=500))


def test_parity_golden_driver_system(ipd):
    Ae, f, n = golden_system()
    E = np.column_stack([f, f + 0.01 * np.linalg.norm(f) / np.sqrt(f.size) * rhs(f.size, 1, 3)[:, 0]])
    D, it, res, resk = check_parity_multi(ipd, Ae, E, driver_opts(n), dict(retol=1e-11, maxit=500))
    assert it.min() >= 1


# ---- 3. agreement with the single call in every plan mode ----------------------------------------
def test_plan_modes(ipd):
    o = lambda n: dict(retol=1e-10, bigph=1, maxit=40, theta=0.25, smoth=5, cycle="v", isnsp=1, inter=1, fnode=n)
    seen = set()
    for m, n, sw in [(64, 64, {}), (64, 64, dict(IPD_NO_SMALL=1)), (1024, 1024, {}),
                     (1024, 1024, dict(IPD_NO_RESIDENT=1, IPD_NO_SMALL=1))]:
        A, E, pd = newton_system(m, n, PR.mask_tree(m, n, seed=4), 4)
        G = pd["bk1"] * pd["tk"] * np.random.RandomState(5).random_sample((m + n, 4))
        with env(**sw):
            h = ipd.AMGHierarchy(A, o(n), ipd.MatlabRand())
        seen.add(solve_mode(h))
        agree_with_singles(h, A, E, dict(retol=1e-11, maxit=300, guess=G))
        h.close()
    assert {0, 1, 2} <= seen, seen


# ---- 4. mixed stopping ---------------------------------------------------------------------------
def test_mixed_stopping(ipd):
    N = 500
    A = laplacian(N, 7, eps=1e-3)   # smoth 1: the stationary loop stalls, PCG needs ~24 iterations
    o = opts("v", smoth=1, isnsp=0, maxit=50)
    h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    rs = np.random.RandomState(2)
    b, g0 = rs.standard_normal(N), 0.1 * rs.standard_normal(N)
    x = np.zeros(N)
    x[7] = 0.5   # every entry of A x is ONE product: e - A x is exactly zero in any summation order
    t = np.linspace(0.0, 1.0, N)
    E = np.column_stack([b, 1e-3 * b, np.zeros(N), A @ x, np.sin(np.pi * t), A @ np.ones(N) + 1e-6 * b,
                         rs.standard_normal(N), np.cos(3 * np.pi * t)])
    G = np.column_stack([g0, 1e-3 * g0, np.zeros(N), x, np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N)])
    # the counts each column needs; then maxit one below the largest, so that the slowest columns are
    # capped while the others stop on the residual test at their own counts
    need = h.pcg_multi(E, dict(retol=1e-11, maxit=500, guess=G))[1]
    assert need.max() < 500 and len(set(need[need > 0])) >= 2, need
    maxit = int(need.max()) - 1
    po = dict(retol=1e-11, maxit=maxit, guess=G)
    out = h.pcg_multi(E, po)
    D, it, res, resk = out
    assert it[2] == 0 and it[3] == 0 and np.isnan(res[2]) and np.isnan(res[3])
    assert np.array_equal(D[:, 2], np.zeros(N)) and np.array_equal(D[:, 3], x)
    capped = [j for j in range(8) if need[j] > maxit]
    stopped = [j for j in range(8) if 0 < need[j] <= maxit]
    assert capped and stopped, need
    assert all(it[j] == maxit and res[j] > 1e-11 for j in capped), (it, res)
    assert all(it[j] == need[j] and res[j] <= 1e-11 for j in stopped), (it, need, res)
    # each column alone in a block of the same width (the other columns zero: frozen from the start)
    # gives the same bits: a frozen column's D is what it was when it stopped
    for j in range(8):
        Ea = np.zeros_like(E)
        Ga = np.zeros_like(G)
        Ea[:, 5], Ga[:, 5] = E[:, j], G[:, j]
        Da, ita, resa, reska = h.pcg_multi(Ea, dict(po, guess=Ga))
        assert np.array_equal(Da[:, 5], D[:, j]) and ita[5] == it[j], j
        assert np.array_equal(resa[5], res[j], equal_nan=True) and np.array_equal(reska[:, 5], resk[:, j]), j
        assert not resk[it[j]:, j].any()
    h.close()


# ---- 5. independence and determinism -------------------------------------------------------------
def test_independence_and_determinism(ipd):
    m = n = 256
    A, E, _ = newton_system(m, n, PR.mask_tree(m, n, seed=3), 7)
    o = driver_opts(n)
    h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    po = dict(retol=1e-11, maxit=300)
    out = h.pcg_multi(E, po)
    assert same_bits(out, h.pcg_multi(E, po))
    p = np.random.RandomState(0).permutation(7)
    Dp, itp, resp, reskp = h.pcg_multi(E[:, p], po)
    D, it, res, resk = out
    assert np.array_equal(Dp, D[:, p]) and np.array_equal(itp, it[p]) and np.array_equal(resp, res[p])
    assert np.array_equal(reskp, resk[:, p])
    h.close()


# ---- 6. chunking and lde > N ---------------------------------------------------------------------
def test_chunks_and_leading_dimension(ipd):
    from codes_of_ipd_ssn_amg_method_amd import _lib as L
    m = n = 64
    A, E, _ = newton_system(m, n, PR.mask_tree(m, n, seed=1), 17)
    o = driver_opts(n)
    h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    po = dict(retol=1e-11, maxit=200)
    for k in (11, 17):
        D, it, res, resk = h.pcg_multi(E[:, :k], po)
        for j0 in range(0, k, 8):
            j1 = min(k, j0 + 8)
            Dc, itc, resc, reskc = h.pcg_multi(E[:, j0:j1], po)
            assert np.array_equal(Dc, D[:, j0:j1]) and np.array_equal(itc, it[j0:j1])
            assert np.array_equal(resc, res[j0:j1]) and np.array_equal(reskc, resk[:, j0:j1])
    # lde > N through the C ABI: the caller's rows of D are carried through untouched
    N, k, lde, maxit = m + n, 5, m + n + 3, 200
    Ep = np.full((lde, k), 7.0, order="F")
    Ep[:N] = E[:, :k]
    Gp = np.full((lde, k), -3.0, order="F")
    Gp[:N] = 0.0
    Dp = np.full((lde, k), 11.0, order="F")
    it = np.zeros(k, np.int64)
    res = np.zeros(k)
    resk = np.full((maxit, k), -1.0, order="F")
    po_s = L.ipd_pcg_opts()
    L.lib.ipd_pcg_opts_init(ctypes.byref(po_s))
    po_s.maxit = maxit
    po_s.retol = 1e-11
    L.check(L.lib.ipd_amg_pcg_multi(h.handle, L.dptr(Ep), lde, k, L.dptr(Gp), ctypes.byref(po_s), L.dptr(Dp),
                                    it.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), L.dptr(res), L.dptr(resk)))
    D, itr, resr, reskr = h.pcg_multi(E[:, :k], po)
    assert np.array_equal(Dp[:N], D) and np.all(Dp[N:] == 11.0) and np.array_equal(it, itr)
    assert np.array_equal(res, resr)
    for j in range(k):   # slots past it[j] are left untouched
        assert np.array_equal(resk[:it[j], j], reskr[:it[j], j]) and np.all(resk[it[j]:, j] == -1.0)
    h.close()


# ---- 7. hierarchy shapes -------------------------------------------------------------------------
@pytest.mark.parametrize("cycle", ["v", "w"])
def test_hierarchy_shapes(ipd, cycle):
    base = dict(retol=1e-10, bigph=0, maxit=60, theta=0.25, smoth=3, cycle=cycle, isnsp=0, inter=1)
    po = dict(retol=1e-11, maxit=200)
    levels = set()
    # levels (oracle setups): 2 -> [2], 10 -> [10, 2], 3000 -> 4 levels
    for N, seed, extra in [(2, 0, {}), (10, 1, {}), (3000, 4, dict(isnsp=1)), (600, 5, dict(smoth=1, isnsp=1))]:
        A = laplacian(N, seed)
        h = ipd.AMGHierarchy(A, dict(base, **extra), ipd.MatlabRand())
        levels.add(h.J)
        agree_with_singles(h, A, rhs(N, 3, seed), po, same_it=h.J > 1)
        h.close()
    assert 1 in levels and 2 in levels and max(levels) >= 4, levels
    # smoth = 0: M is the coarse correction alone; two iterations against the device's own cycle
    A = laplacian(600, 5)
    h = ipd.AMGHierarchy(A, dict(base, smoth=0), ipd.MatlabRand())
    M = (lambda r: ipd.MG_Vcycle(h, r, 0, 1)) if cycle == "v" else (lambda r: ipd.MG_Wcycle(h, r, 0, 1))
    E = rhs(600, 3, 6)
    D, it, res, resk = h.pcg_multi(E, dict(retol=1e-11, maxit=2))
    for j in range(3):
        de, ite, _, reske = R.amg_pcg(A, E[:, j], M, retol=1e-11, maxit=2)
        assert it[j] == ite and rel(D[:, j], de) <= 1e-10 and np.allclose(resk[:ite, j], reske, rtol=1e-8)
    h.close()
    # bigraph Gauss-Seidel smoother, with and without a mask operator attached: the block path keeps the
    # CSR sweeps either way
    m, n = 100, 70
    A, E, pd = newton_system(m, n, PR.mask_bernoulli(m, n, 0.5), 3)
    o = dict(base, bigph=1, fnode=n, isnsp=1, smoth=5)
    with env(IPD_NO_SMALL=1):
        h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    out0 = agree_with_singles(h, A, E, po)
    assert h.attach_mask_operator(pd["p"], pd["q"], pd["tk"])
    assert same_bits(h.pcg_multi(E, po), out0)
    h.close()


# ---- 8. edges and side effects -------------------------------------------------------------------
def test_edges_and_side_effects(ipd):
    from codes_of_ipd_ssn_amg_method_amd import _lib as L
    m = n = 64
    A, E, pd = newton_system(m, n, PR.mask_tree(m, n, seed=1), 3)
    o = driver_opts(n)
    N = m + n
    G = 0.1 * rhs(N, 3, 4)
    po = dict(retol=1e-11, maxit=300, guess=G)
    h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    s0 = h.solve(E[:, 0], G[:, 0])
    sm0 = h.solve_multi(E, G)
    p0 = h.pcg(E[:, 1], dict(po, guess=G[:, 1]))
    out = h.pcg_multi(E, po)
    s1 = h.solve(E[:, 0], G[:, 0])
    sm1 = h.solve_multi(E, G)
    p1 = h.pcg(E[:, 1], dict(po, guess=G[:, 1]))
    assert np.array_equal(s0[0], s1[0]) and s0[1] == s1[1] and np.array_equal(s0[3], s1[3])
    assert np.array_equal(sm0[0], sm1[0]) and np.array_equal(sm0[1], sm1[1])
    assert all(np.array_equal(a, b) for a, b in zip(sm0[3], sm1[3]))
    assert np.array_equal(p0[0], p1[0]) and p0[1] == p1[1] and np.array_equal(p0[3], p1[3])
    # the two calls share the hierarchy's work blocks, which are made for the widest block met so far: on a
    # fresh hierarchy (same stream, so the same hierarchy) a call whose blocks were made for a narrower width
    # by the other entry, and a call narrower than the blocks it finds, give the bits of the calls above
    same_multi = lambda a, b: (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and
                               all(np.array_equal(u, v) for u, v in zip(a[3], b[3])))
    E9, G9 = np.column_stack([E, 0.5 * E, -E]), np.column_stack([G, G, G])
    h3 = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    sm_w1 = h3.solve_multi(E[:, :1], G[:, :1])                     # blocks made for width 1
    assert same_bits(h3.pcg_multi(E, po), out)                     # width 4 on blocks made for 1
    assert same_multi(h3.solve_multi(E[:, :1], G[:, :1]), sm_w1)   # width 1 on blocks made for 4
    pm_w2 = h3.pcg_multi(E[:, :2], dict(po, guess=G[:, :2]))       # width 2 on blocks (both kinds) made for 4
    sm9 = h3.solve_multi(E9, G9)                                   # chunks of width 8 then 1: blocks grow to 8
    pm9 = h3.pcg_multi(E9, dict(po, guess=G9))                     # the PCG's own vectors grow from 4 to 8
    assert same_bits(h3.pcg_multi(E, po), out) and same_multi(h3.solve_multi(E, G), sm0)   # 4 on 8
    h3.close()
    h4 = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    assert same_bits(h4.pcg_multi(E[:, :2], dict(po, guess=G[:, :2])), pm_w2)   # first call: made for width 2
    assert same_multi(h4.solve_multi(E, G), sm0)                   # width 4 on blocks the PCG made for 2
    assert same_bits(h4.pcg_multi(E9, dict(po, guess=G9)), pm9)    # 8 then 1 on blocks made for 4
    assert same_multi(h4.solve_multi(E9, G9), sm9)                 # ... and on blocks the PCG made for 8
    h4.close()
    # IPD_E_ARG cases
    Ef = np.asfortranarray(E)
    Df = np.empty((N, 3), order="F")
    itv = np.zeros(3, np.int64)
    ip = itv.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    pos = L.ipd_pcg_opts()
    L.lib.ipd_pcg_opts_init(ctypes.byref(pos))
    bad = L.ipd_pcg_opts()
    L.lib.ipd_pcg_opts_init(ctypes.byref(bad))
    bad.precd = 2
    P = ctypes.byref(pos)
    for args in [(None, L.dptr(Ef), N, 3, None, P, L.dptr(Df), ip, None, None),
                 (h.handle, None, N, 3, None, P, L.dptr(Df), ip, None, None),
                 (h.handle, L.dptr(Ef), N, 3, None, P, None, ip, None, None),
                 (h.handle, L.dptr(Ef), N, 3, None, P, L.dptr(Df), None, None, None),
                 (h.handle, L.dptr(Ef), N, 0, None, P, L.dptr(Df), ip, None, None),
                 (h.handle, L.dptr(Ef), N - 1, 3, None, P, L.dptr(Df), ip, None, None),
                 (h.handle, L.dptr(Ef), N, 3, None, ctypes.byref(bad), L.dptr(Df), ip, None, None)]:
        assert L.lib.ipd_amg_pcg_multi(*args) == L.IPD_E_ARG
    for cyc in (1, "x"):
        hc = ipd.AMGHierarchy(A, dict(o, cycle=cyc), ipd.MatlabRand())
        assert L.lib.ipd_amg_pcg_multi(hc.handle, L.dptr(Ef), N, 3, None, P, L.dptr(Df), ip, None, None) == L.IPD_E_ARG
        with pytest.raises(ipd.IpdError):
            hc.pcg_multi(E)
        hc.close()
    # NULL guess, res and resk are fine (defaults: retol 1e-11, maxit 1e4)
    assert L.lib.ipd_amg_pcg_multi(h.handle, L.dptr(Ef), N, 3, None, None, L.dptr(Df), ip, None, None) == 0
    Dn, itn, _, _ = h.pcg_multi(E)
    assert np.array_equal(Df, Dn) and np.array_equal(itv, itn)
    # the device entry point equals the host one
    maxit = 300
    dE = L.DeviceBuffer.from_array(Ef.T.copy().reshape(-1), h.ctx)
    dG = L.DeviceBuffer.from_array(np.asfortranarray(G).T.copy().reshape(-1), h.ctx)
    dD = L.DeviceBuffer(8 * N * 3, h.ctx)
    itd = np.zeros(3, np.int64)
    resd = np.zeros(3)
    reskd = np.zeros((maxit, 3), order="F")
    pos.maxit = maxit
    pos.retol = 1e-11
    L.check(L.lib.ipd_amg_pcg_multi_dev(h.handle, dE.ptr, N, 3, dG.ptr, ctypes.byref(pos), dD.ptr,
                                        itd.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), L.dptr(resd),
                                        L.dptr(reskd)))
    Dd = dD.to_array(np.float64, N * 3).reshape(3, N).T
    assert same_bits((Dd, itd, resd, reskd), out)
    h.close()
    # AMG_PCG_multi == AMGHierarchy.pcg_multi (fresh hierarchy, same stream)
    Dc = ipd.AMG_PCG_multi(A, E, o, po, ipd.MatlabRand())
    h2 = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    assert same_bits(Dc, h2.pcg_multi(E, po))
    h2.close()
    # where the stationary iteration stalls, every column converges
    Nl = 500
    Al = laplacian(Nl, 7, eps=1e-3)
    ol = opts("v", smoth=1, isnsp=0, maxit=50)
    El = rhs(Nl, 4, 2)
    _, it_st, rel_st, _, _ = O.Class_AMG(Al, El[:, 0], dict(ol), O.matlab_rng())
    assert rel_st > ol["retol"]
    D, it, res, _ = ipd.AMG_PCG_multi(Al, El, ol, dict(retol=1e-11, maxit=50), ipd.MatlabRand())
    assert np.all(it < 50) and np.all(res <= 1e-11)
    for j in range(4):
        assert np.linalg.norm(Al @ D[:, j] - El[:, j]) <= 1e-8 * np.linalg.norm(El[:, j])
