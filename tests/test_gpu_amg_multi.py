"""Several right-hand sides through one hierarchy (ipd_amg_solve_multi / AMGHierarchy.solve_multi /
Class_AMG_multi): every column as if solved alone.

1. per-column parity with the oracle's solve phase on the oracle hierarchy;
2. equality with the single solve on the same hierarchy in every plan mode (0, 1, 2);
3. mixed stopping inside one block (frozen columns);
4. independence of the other columns and run-to-run determinism;
5. chunking (nrhs > 8) and ldb > N;
6. hierarchy shapes: 1, 2, >= 4 levels, smoth = 0, Jacobi and bigraph smoothers, a mask operator;
7. edges and side effects.
Not covered: the IPD_E_ARG case of a hierarchy sharded over ranks.  A hierarchy is sharded only
inside ipd_amg_bench_cycles_sharded (emulated or over RCCL ranks; it restores shard_ranks = 1 before
returning), so no call of the public interface reaches solve_multi with a sharded hierarchy on one
GPU; the check guards against that state all the same."""
import ctypes
import os
from contextlib import contextmanager

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ipd_oracle as O
from tests import problems as PR
from tests.test_gpu_setup import newton_matrix

pytestmark = pytest.mark.gpu

RES_TOL = 1e-10


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


CASES = [
    ("tree64", 64, 64, lambda: PR.mask_tree(64, 64, seed=1)),
    ("tree_rect", 150, 90, lambda: PR.mask_tree(150, 90, seed=2)),
    ("tree256", 256, 256, lambda: PR.mask_tree(256, 256, seed=3)),
    ("dense96", 96, 96, lambda: PR.mask_bernoulli(96, 96, 1.0)),
    ("bern128", 128, 128, lambda: PR.mask_bernoulli(128, 128, 0.2)),
]


def system(m, n, s, k, seed=7):
    Ae, pd = newton_matrix(m, n, s)
    rs = np.random.RandomState(seed)
    f = np.concatenate([pd["q"], -pd["p"]]) * pd["z"]
    B = np.column_stack([f * (1.0 + 0.1 * j) + 0.05 * rs.standard_normal(m + n) for j in range(k)])
    G = pd["bk1"] * pd["tk"] * rs.random_sample((m + n, k))
    return sp.csr_matrix(Ae), B, G, pd


def laplacian(N, seed):
    return sp.csr_matrix(PR.random_sym_graph_laplacian(N, deg=4, seed=seed, eps=0.5))


def singles(h, B, G=None):
    out = []
    for j in range(B.shape[1]):
        out.append(h.solve(B[:, j], None if G is None else G[:, j]))
    return out


def close_ratios(rho, rhos, rk, rks):
    """rhok agrees where both residuals it divides are above the rounding floor (1e-8 relative); below it
    the ratio of two rounding-noise residuals is noise itself"""
    fin = np.isfinite(rhos)
    assert np.array_equal(fin, np.isfinite(rho))
    ok = fin.copy()
    ok[1:] &= (rks[1:] > 1e-8) & (rks[:-1] > 1e-8)
    assert np.allclose(rho[ok], rhos[ok], rtol=1e-6, atol=0), (rho, rhos)


def same_as_singles(h, B, G=None, X=None, it=None, rk=None, rho=None, A=None, tol=1e-12):
    if X is None:
        X, it, _, rk, rho = h.solve_multi(B, G)
    for j, (x, its, _, rks, rhos) in enumerate(singles(h, B, G)):
        assert it[j] == its, (j, it[j], its)
        assert len(rk[j]) == its + 1 and np.max(np.abs(rk[j] - rks)) <= tol, (j, rk[j], rks)
        close_ratios(rho[j], rhos, rk[j], rks)
        if A is not None:
            assert np.linalg.norm(A @ (X[:, j] - x)) <= 1e-11 * max(np.linalg.norm(B[:, j]), 1e-300)
    return X, it, rk, rho


# ---- 1. oracle parity per column -------------------------------------------------------------
@pytest.mark.parametrize("name,m,n,mk", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("isnsp", [0, 1])
@pytest.mark.parametrize("cycle", ["v", "w"])
def test_oracle_parity_per_column(ipd, name, m, n, mk, isnsp, cycle):
    A, B, G, _ = system(m, n, mk(), 5)
    o = O.amg_options_class1(cycle)
    o.update(fnode=n, isnsp=isnsp)
    ho = O.amg_setup(A, o, O.matlab_rng())
    h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    X, it, rel, rk, rho = h.solve_multi(B, G)
    for j in range(5):
        xo, ito, relo, rko, rhoo = O.amg_solve(ho, B[:, j], dict(o, guess=G[:, j]))
        # test_class_amg_residual_history's bar; the dense system reaches the rounding floor (1e-9 of
        # the initial residual) and then stops on the first rise of the residual (rhok > 1): which cycle
        # that is, is rounding noise (tests/test_gpu_bench_workload.py, same_history)
        k = min(len(rk[j]), len(rko))
        a, b = rk[j][:k], rko[:k]
        floor = (a <= 1e-9) & (b <= 1e-9)
        assert np.all((np.abs(a - b) <= RES_TOL) | floor), (j, a, b)
        if it[j] != ito:
            at_floor = max(a[-1], b[-1]) <= 1e-9
            assert (abs(it[j] - ito) == 1 and abs(rko[k - 1] - o["retol"]) <= RES_TOL) or \
                (at_floor and abs(it[j] - ito) <= 4), (j, it[j], ito, a, b)
        assert np.linalg.norm(A @ X[:, j] - B[:, j]) <= max(10 * relo, 1e-10) * np.linalg.norm(A @ G[:, j] - B[:, j])
    h.close()


# ---- 2. equality with the single solve in every plan mode --------------------------------------
def test_plan_modes(ipd):
    o = lambda n: dict(retol=1e-10, bigph=1, maxit=40, theta=0.25, smoth=5, cycle="v", isnsp=1, inter=1, fnode=n)
    seen = set()
    for m, n, sw in [(64, 64, {}), (64, 64, dict(IPD_NO_SMALL=1)), (1024, 1024, {}),
                     (1024, 1024, dict(IPD_NO_RESIDENT=1, IPD_NO_SMALL=1))]:
        A, B, G, _ = system(m, n, PR.mask_tree(m, n, seed=4), 4)
        with env(**sw):
            h = ipd.AMGHierarchy(A, o(n), ipd.MatlabRand())
        seen.add(solve_mode(h))
        same_as_singles(h, B, G, A=A)
        h.close()
    assert {0, 1, 2} <= seen, seen


# ---- 3. mixed stopping ---------------------------------------------------------------------------
@pytest.mark.parametrize("cycle", ["v", "w"])
def test_mixed_stopping(ipd, cycle):
    N = 600
    A = laplacian(N, 5)   # smoth 1: a slow, steady contraction (many cycles)
    o = dict(retol=1e-10, bigph=0, maxit=60, theta=0.25, smoth=1, cycle=cycle, isnsp=1, inter=1)
    h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    rs = np.random.RandomState(2)
    b, g0 = rs.standard_normal(N), 0.1 * rs.standard_normal(N)
    g = np.zeros(N)
    g[7] = 0.5   # every entry of A g is ONE product: b - A g is exactly zero in any summation order
    # column 4: A*1 (the kernel-space correction removes it in one cycle) plus a small rough part --
    # the oracle needs 13 cycles for it against 32 for column 0, so it stops while column 0 goes on
    Bm = np.column_stack([b, 1e-3 * b, np.zeros(N), A @ g, A @ np.ones(N) + 1e-6 * b])
    Gm = np.column_stack([g0, 1e-3 * g0, np.zeros(N), g, np.zeros(N)])
    X, it, rel, rk, rho = h.solve_multi(Bm, Gm)
    assert it[0] >= 8 and it[2] == 0 and it[3] == 0 and rk[2][0] == 0 and rho[3][0] == np.inf
    assert 1 <= it[4] and it[4] + 5 <= it[0], it   # frozen mid-run: column 0 cycles on after it
    assert np.array_equal(X[:, 2], np.zeros(N)) and np.array_equal(X[:, 3], g)
    same_as_singles(h, Bm, Gm, X, it, rk, rho, A=A)
    # a frozen column keeps the bits it stopped with: alone in a block of the same width (W = 8, the
    # other columns zero and inactive from the start) it gives the same x, count and history
    for j in (0, 4):
        Ba = np.zeros_like(Bm)
        Ga = np.zeros_like(Gm)
        Ba[:, 0], Ga[:, 0] = Bm[:, j], Gm[:, j]
        Xa, ita, rela, rka, rhoa = h.solve_multi(Ba, Ga)
        assert np.array_equal(Xa[:, 0], X[:, j]) and ita[0] == it[j] and rela[0] == rel[j], j
        assert np.array_equal(rka[0], rk[j]) and np.array_equal(rhoa[0], rho[j], equal_nan=True), j
    h.close()


# ---- 4. independence and determinism -------------------------------------------------------------
def test_independence_and_determinism(ipd):
    m = n = 256
    A, B, G, _ = system(m, n, PR.mask_tree(m, n, seed=3), 7)
    o = O.amg_options_class1("w")
    o.update(fnode=n, isnsp=1)
    h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    X, it, rel, rk, rho = h.solve_multi(B, G)
    X2, it2, rel2, rk2, rho2 = h.solve_multi(B, G)
    assert np.array_equal(X, X2) and np.array_equal(it, it2) and np.array_equal(rel, rel2)
    assert all(np.array_equal(a, b) for a, b in zip(rk, rk2))
    p = np.random.RandomState(0).permutation(7)
    Xp, itp, relp, rkp, rhop = h.solve_multi(B[:, p], G[:, p])
    assert np.array_equal(Xp, X[:, p]) and np.array_equal(itp, it[p]) and np.array_equal(relp, rel[p])
    assert all(np.array_equal(rkp[i], rk[p[i]]) for i in range(7))
    x1, it1, rel1, rk1, rho1 = h.solve_multi(B[:, 2], G[:, 2])
    assert it1[0] == it[2] and np.max(np.abs(rk1[0] - rk[2])) <= 1e-13
    assert np.linalg.norm(A @ (x1[:, 0] - X[:, 2])) <= 1e-13 * np.linalg.norm(B[:, 2]) * 100
    h.close()


# ---- 5. chunking and ldb > N --------------------------------------------------------------------
def test_chunks_and_leading_dimension(ipd):
    from codes_of_ipd_ssn_amg_method_amd import _lib as L
    m = n = 64
    A, B, G, _ = system(m, n, PR.mask_tree(m, n, seed=1), 33)
    o = O.amg_options_class1("v")
    o.update(fnode=n, isnsp=1)
    h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    for k in (17, 33):
        X, it, rel, rk, rho = h.solve_multi(B[:, :k], G[:, :k])
        for j0 in range(0, k, 8):
            j1 = min(k, j0 + 8)
            Xc, itc, relc, rkc, _ = h.solve_multi(B[:, j0:j1], G[:, j0:j1])
            assert np.array_equal(Xc, X[:, j0:j1]) and np.array_equal(itc, it[j0:j1])
            assert all(np.array_equal(a, b) for a, b in zip(rkc, rk[j0:j1]))
    # ldb > N through the C ABI: padding rows are carried through untouched
    N, k, ldb = m + n, 5, m + n + 3
    Bp = np.full((ldb, k), 7.0, order="F")
    Bp[:N] = B[:, :k]
    Gp = np.full((ldb, k), -3.0, order="F")
    Gp[:N] = G[:, :k]
    Xp = np.full((ldb, k), 11.0, order="F")
    it = np.zeros(k, np.int32)
    rel = np.zeros(k)
    hs = h.maxit + 1
    rk = np.full((hs, k), np.nan, order="F")
    rho = np.full((hs, k), np.nan, order="F")
    I32 = ctypes.POINTER(ctypes.c_int32)
    L.check(L.lib.ipd_amg_solve_multi(h.handle, L.dptr(Bp), ldb, k, L.dptr(Gp), L.dptr(Xp), it.ctypes.data_as(I32),
                                      L.dptr(rel), L.dptr(rk), L.dptr(rho)))
    X, itr, relr, rkr, _ = h.solve_multi(B[:, :k], G[:, :k])
    assert np.array_equal(Xp[:N], X) and np.all(Xp[N:] == 11.0) and np.array_equal(it, itr)
    for j in range(k):
        assert np.array_equal(rk[:it[j] + 1, j], rkr[j]) and np.all(np.isnan(rk[it[j] + 1:, j]))
    h.close()


# ---- 6. hierarchy shapes -------------------------------------------------------------------------
@pytest.mark.parametrize("cycle", ["v", "w"])
def test_hierarchy_shapes(ipd, cycle):
    rs = np.random.RandomState(5)
    base = dict(retol=1e-10, bigph=0, maxit=60, theta=0.25, smoth=3, cycle=cycle, isnsp=0, inter=1)
    levels = set()
    # levels (oracle setups): 2 -> [2], 10 -> [10, 2], 600 -> 4 levels, 3000 -> 4 levels
    for N, seed, extra in [(2, 0, {}), (10, 1, {}), (3000, 4, {}), (3000, 4, dict(isnsp=1)),
                           (600, 5, dict(smoth=0, maxit=8)), (600, 5, dict(smoth=1, isnsp=1))]:
        A = laplacian(N, seed)
        o = dict(base, **extra)
        h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
        levels.add(h.J)
        B = rs.standard_normal((N, 3))
        same_as_singles(h, B, A=A)
        h.close()
    assert 1 in levels and 2 in levels and max(levels) >= 4, levels
    # bigraph Gauss-Seidel smoother (with and without a mask operator attached: the block path
    # keeps the CSR sweeps either way)
    m, n = 100, 70
    A, B, G, pd = system(m, n, PR.mask_bernoulli(m, n, 0.5), 3)
    o = dict(base, bigph=1, fnode=n, isnsp=1, smoth=5)
    with env(IPD_NO_SMALL=1):
        h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    X0, it0, rk0, _ = same_as_singles(h, B, G, A=A, tol=1e-12)
    assert h.attach_mask_operator(pd["p"], pd["q"], pd["tk"])
    X1, it1, _, rk1, _ = h.solve_multi(B, G)
    assert np.array_equal(X1, X0) and np.array_equal(it1, it0)
    for j in range(3):   # single solves now use the mask operator: rounding differs
        x, its, _, rks, _ = h.solve(B[:, j], G[:, j])
        assert its == it1[j] and np.max(np.abs(rks - rk1[j])) <= 1e-12
    h.close()


# ---- 7. edges and side effects -------------------------------------------------------------------
def test_edges_and_side_effects(ipd):
    from codes_of_ipd_ssn_amg_method_amd import _lib as L
    m = n = 64
    A, B, G, _ = system(m, n, PR.mask_tree(m, n, seed=1), 3)
    o = O.amg_options_class1("v")
    o.update(fnode=n, isnsp=1)
    h = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    N = m + n
    x0, it0, rel0, rk0, rho0 = h.solve(B[:, 0], G[:, 0])
    X, it, rel, rk, rho = h.solve_multi(B, G)
    x1, it1, rel1, rk1, rho1 = h.solve(B[:, 0], G[:, 0])
    assert np.array_equal(x0, x1) and it0 == it1 and rel0 == rel1 and np.array_equal(rk0, rk1)
    # IPD_E_ARG cases
    Bf = np.asfortranarray(B)
    Xf = np.empty((N, 3), order="F")
    itv = np.zeros(3, np.int32)
    I32 = ctypes.POINTER(ctypes.c_int32)
    ip = itv.ctypes.data_as(I32)
    for args in [(None, L.dptr(Bf), N, 3, None, L.dptr(Xf), ip, None, None, None),
                 (h.handle, None, N, 3, None, L.dptr(Xf), ip, None, None, None),
                 (h.handle, L.dptr(Bf), N, 3, None, None, ip, None, None, None),
                 (h.handle, L.dptr(Bf), N, 3, None, L.dptr(Xf), None, None, None, None),
                 (h.handle, L.dptr(Bf), N, 0, None, L.dptr(Xf), ip, None, None, None),
                 (h.handle, L.dptr(Bf), N - 1, 3, None, L.dptr(Xf), ip, None, None, None)]:
        assert L.lib.ipd_amg_solve_multi(*args) == L.IPD_E_ARG
    # NULL histories and rel_res are fine
    assert L.lib.ipd_amg_solve_multi(h.handle, L.dptr(Bf), N, 3, None, L.dptr(Xf), ip, None, None, None) == 0
    # the device entry point equals the host one
    dB = L.DeviceBuffer.from_array(Bf.T.copy().reshape(-1), h.ctx)
    dG = L.DeviceBuffer.from_array(np.asfortranarray(G).T.copy().reshape(-1), h.ctx)
    dX = L.DeviceBuffer(8 * N * 3, h.ctx)
    itd = np.zeros(3, np.int32)
    reld = np.zeros(3)
    hs = h.maxit + 1
    rkd = np.full((hs, 3), np.nan, order="F")
    rhod = np.full((hs, 3), np.nan, order="F")
    L.check(L.lib.ipd_amg_solve_multi_dev(h.handle, dB.ptr, N, 3, dG.ptr, dX.ptr, itd.ctypes.data_as(I32),
                                          L.dptr(reld), L.dptr(rkd), L.dptr(rhod)))
    Xd = dX.to_array(np.float64, N * 3).reshape(3, N).T
    assert np.array_equal(Xd, X) and np.array_equal(itd, it) and np.array_equal(reld, rel)
    for j in range(3):
        assert np.array_equal(rkd[:it[j] + 1, j], rk[j]) and np.array_equal(rhod[:it[j] + 1, j], rho[j], equal_nan=True)
    h.close()
    # Class_AMG_multi == AMGHierarchy.solve_multi (fresh hierarchy, same stream)
    Xc, itc, relc, rkc, rhoc = ipd.Class_AMG_multi(A, B, dict(o, guess=G), ipd.MatlabRand())
    h2 = ipd.AMGHierarchy(A, o, ipd.MatlabRand())
    Xh, ith, relh, rkh, rhoh = h2.solve_multi(B, G)
    assert np.array_equal(Xc, Xh) and np.array_equal(itc, ith) and np.array_equal(relc, relh)
    h2.close()
    with pytest.raises(ValueError):
        ipd.AMGHierarchy(A, o, ipd.MatlabRand()).solve_multi(np.zeros((N + 1, 2)))
