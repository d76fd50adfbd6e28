"""The device-pointer ABI (include/ipd_amg.h, "device-resident path") called as a PyTorch-ROCm caller calls it:
through ctypes on raw device pointers, which need not have the 256-byte alignment of the library's own arena.

  1. ipd_ax_dev / ipd_aty_dev     at the tile edges, outputs at +0 and +8 bytes (k_aty_v2 / k_aty_v1)
  2. ipd_asat_dev, ipd_dmat_dims, ipd_dmat_download   mask at byte offsets 0, 8 (8-byte loads) and 1, 4 (byte
                                  loads + ballot), mask bytes other than 0 / 1, handle lifetimes
  3. ipd_spmv_dev                 the three row-group widths, the row lengths around them, the grid-stride loop
  4. ipd_amg_setup_dev / ipd_amg_solve_dev   the three solve modes, bit for bit against the host entries
  5. ipd_asat_dev -> ipd_hybrid_amg_dev      against ipd.Hybrid_AMG bit for bit, against the oracle, refusals
  6. ipd_h2d / ipd_d2h

Every output lies in a buffer prefilled with -7.0 and its surroundings are checked afterwards; every input is
downloaded again and compared bit for bit (tests/dev_abi.py).  Tolerances of sums are derived from the number
format (dev_abi.ax_ref, dev_abi.spmv_ref), not measured; tests/test_dev_abi_refs.py checks the references.

Mutation power (made by hand on a scratch copy, never committed; arithmetic only, no memory access changed; the
suite as it was before this file ran against each as well):
  (a) k_asat_masks<false> tests b == 1 instead of b != 0: test_asat_dev fails in the 28 "mixed" and "bit0clear"
      cases that have an entry (offsets 1 and 4, and every offset for m = 65), with
      test_asat_dev_handles_outlive_each_other and test_spmv_dev_of_asat_dev_is_ax_of_aty.  Suite before: green.
  (b) k_spmv<64> stops its shuffle reduction at d > 1: test_spmv_dev[L64], [one_row] and [cap_L64] fail, with
      test_spmv_dev_of_asat_dev_is_ax_of_aty (its H has about 35 entries a row: the <64> branch).  Suite before: green
      (csr_spmv is reached through ipd_spmv_dev only).
  (c) k_aty_v1 uses q[j0] for q[j]: test_aty_dev fails for the seven shapes with n > 1 (even m: only with z at
      +8) and test_spmv_dev_of_asat_dev_is_ax_of_aty.  Suite before: its three odd-m cases fail
      (test_gpu_kkt.py::test_ax_aty[3-5], [65-63], test_gpu_setup_at_scale.py::test_ax_aty_at_scale[2047x2049]);
      no case of it has an even m with z off a 16-byte boundary.
The file runs in under 2 s on one MI355X; no test takes more than 0.4 s."""
import os
from contextlib import contextmanager
from ctypes import byref, c_double, c_int, c_int32, c_int64, c_size_t, c_void_p

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ipd_oracle as O
from tests import dev_abi as D
from tests import problems as PR
from tests.dev_abi import DevArray, bits, free_all

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ipd():
    import codes_of_ipd_ssn_amg_method_amd as m
    return m


@pytest.fixture(scope="module")
def L():
    from codes_of_ipd_ssn_amg_method_amd import _lib
    return _lib


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


def csc_bits_equal(A, B):
    A, B = sp.csc_matrix(A), sp.csc_matrix(B)
    A.sort_indices()
    B.sort_indices()
    return (A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and np.array_equal(bits(A.data), bits(B.data)))


# ---------------------------------------------------------------------------------------------------------------
# 1. ipd_ax_dev / ipd_aty_dev
# ---------------------------------------------------------------------------------------------------------------
PLACEMENTS = [("out+0", 0, 0), ("out+8", 8, 0), ("all+8", 8, 8)]        # (name, output offset, input offset)


def kkt_inputs(m, n):
    rs = np.random.RandomState(m * 1000 + n)
    return 0.5 + rs.random_sample(m), 0.5 + rs.random_sample(n), rs.standard_normal(m * n), rs.standard_normal(m + n)


@pytest.mark.parametrize("m,n", D.AX_SHAPES)
def test_aty_dev(L, m, n):
    """Bit-equal to the oracle in every placement.  An even m with z at +8 takes k_aty_v1 (8-byte stores), at +0
    k_aty_v2 (16-byte stores, two rows per lane); an odd m always k_aty_v1."""
    p, q, _, y = kkt_inputs(m, n)
    ref = bits(O.Aty(y, p, q))
    ctx = L.get_ctx().handle
    for name, oo, io in PLACEMENTS:
        dy, dp, dq = DevArray(y, io), DevArray(p, io), DevArray(q, io)
        dz = DevArray.empty(m * n, off=oo)
        assert (dz.ptr.value % 16 == 0) == (oo == 0)
        got = []
        for _ in range(2):
            L.check(L.lib.ipd_aty_dev(ctx, dy.ptr, dp.ptr, dq.ptr, c_int64(m), c_int64(n), dz.ptr))
            got.append(bits(dz.read()))
        assert np.array_equal(got[0], ref), (name, int(np.sum(got[0] != ref)))
        assert np.array_equal(got[1], got[0]), name
        for d in (dy, dp, dq):
            d.assert_unchanged(name)
        free_all(dy, dp, dq, dz)


@pytest.mark.parametrize("m,n", D.AX_SHAPES)
def test_ax_dev(L, m, n):
    """Within the derived bound of a longdouble reference (dev_abi.ax_ref) in every placement, and two calls give
    the same bits."""
    p, q, x, _ = kkt_inputs(m, n)
    ref, bound = D.ax_ref(x, p, q)
    ctx = L.get_ctx().handle
    for name, oo, io in PLACEMENTS:
        dx, dp, dq = DevArray(x, io), DevArray(p, io), DevArray(q, io)
        dy = DevArray.empty(m + n, off=oo)
        got = []
        for _ in range(2):
            L.check(L.lib.ipd_ax_dev(ctx, dx.ptr, dp.ptr, dq.ptr, c_int64(m), c_int64(n), dy.ptr))
            got.append(dy.read())
        ok, worst = D.within(got[0], ref, bound)
        print("ax %dx%d %s: worst |y - ref| / bound = %.3f" % (m, n, name, worst))
        assert ok, (name, worst)
        assert np.array_equal(bits(got[1]), bits(got[0])), name
        for d in (dx, dp, dq):
            d.assert_unchanged(name)
        free_all(dx, dp, dq, dy)


# ---------------------------------------------------------------------------------------------------------------
# 2. ipd_asat_dev, ipd_dmat_dims, ipd_dmat_download
# ---------------------------------------------------------------------------------------------------------------
def asat_pq(m, n):
    rs = np.random.RandomState(7)
    return 0.5 + rs.random_sample(m), 0.5 + rs.random_sample(n)


def asat_dev(L, ds, dp, dq, m, n):
    H = c_void_p()
    L.check(L.lib.ipd_asat_dev(L.get_ctx().handle, ds.ptr, dp.ptr, dq.ptr, c_int64(m), c_int64(n), byref(H)))
    return H


def dmat_dims(L, H):
    r, c, z = c_int64(-1), c_int64(-1), c_int64(-1)
    L.check(L.lib.ipd_dmat_dims(H, byref(r), byref(c), byref(z)))
    return r.value, c.value, z.value


def dmat_download(L, H):
    out = L.ipd_csc_out()
    L.check(L.lib.ipd_dmat_download(L.get_ctx().handle, H, byref(out)))
    return L.csc_out_to_scipy(out)


@pytest.mark.parametrize("flavour", ["01", "mixed", "bit0clear"])
@pytest.mark.parametrize("rho", D.ASAT_DENSITIES)
@pytest.mark.parametrize("m,n", list(D.ASAT_SHAPES))
def test_asat_dev(L, m, n, rho, flavour):
    """The mask is "m*n logical": a byte counts when it is not 0.  k_asat_masks<true> (m % 8 == 0 and s 8-byte
    aligned: offsets 0, 8) packs 8-byte words with a multiply, k_asat_masks<false> (offsets 1, 4, and m = 65)
    tests each byte; m = 72 has tile 0 in the wide path and tile 1 in the byte path of the same launch."""
    p, q = asat_pq(m, n)
    s = D.mask_bytes(m, n, rho, flavour)
    Ho = sp.csc_matrix(O.ASAt(s != 0, p, q))
    M = m + n
    if rho == 0.0:
        assert Ho.nnz == 0
    dp, dq = DevArray(p), DevArray(q)
    for off in D.ASAT_OFFSETS:
        ds = DevArray(s, off)
        assert ds.ptr.value % 8 == off % 8
        H = asat_dev(L, ds, dp, dq, m, n)
        try:
            assert dmat_dims(L, H) == (M, M, Ho.nnz), (off, dmat_dims(L, H), Ho.nnz)
            assert csc_bits_equal(dmat_download(L, H), Ho), off
        finally:
            L.lib.ipd_dmat_destroy(H)
        ds.assert_unchanged("s at +%d" % off)
        ds.free()
    dp.assert_unchanged("p")
    dq.assert_unchanged("q")
    free_all(dp, dq)


def test_asat_dev_handles_outlive_each_other(L):
    """H1 and H2 from different masks, H1 destroyed, H3 built (the pool hands H1's memory out again): H2 is intact."""
    m, n = 72, 65
    p, q = asat_pq(m, n)
    masks = [D.mask_bytes(m, n, rho, "mixed", seed=k) for k, rho in enumerate((0.5, 0.3, 0.6))]
    dp, dq = DevArray(p), DevArray(q)
    ds = [DevArray(s, 8) for s in masks]
    H1 = asat_dev(L, ds[0], dp, dq, m, n)
    H2 = asat_dev(L, ds[1], dp, dq, m, n)
    L.lib.ipd_dmat_destroy(H1)
    H3 = asat_dev(L, ds[2], dp, dq, m, n)
    try:
        assert csc_bits_equal(dmat_download(L, H2), O.ASAt(masks[1] != 0, p, q))
        assert csc_bits_equal(dmat_download(L, H3), O.ASAt(masks[2] != 0, p, q))
        assert dmat_dims(L, H2)[2] != dmat_dims(L, H3)[2]
    finally:
        L.lib.ipd_dmat_destroy(H2)
        L.lib.ipd_dmat_destroy(H3)
    free_all(dp, dq, *ds)
    assert L.lib.ipd_dmat_dims(None, None, None, None) == L.IPD_E_ARG


# ---------------------------------------------------------------------------------------------------------------
# 3. ipd_spmv_dev
# ---------------------------------------------------------------------------------------------------------------
def dmat_upload(L, A, symmetric=0):
    a = L.CscIn(A)
    d = c_void_p()
    L.check(L.lib.ipd_dmat_upload(L.get_ctx().handle, a.ref(), c_int32(symmetric), byref(d)))
    return d


@pytest.mark.parametrize("name", list(D.SPMV_MATRICES))
def test_spmv_dev(L, name):
    """k_spmv<4>, <16>, <64> by average row length (<= 6, <= 24, above), rows shorter than, equal to and longer
    than the group, and the grid-stride loop behind the cap of 8192 workgroups: within the derived bound of a
    longdouble reference, x and y at +0 and +8."""
    make, width = D.SPMV_MATRICES[name]
    A = make()
    assert D.spmv_branch(A) == width
    nr, nc = A.shape
    x = np.random.RandomState(nr % 1000 + nc).standard_normal(nc)
    ref, bound = D.spmv_ref(A, x)
    dA = dmat_upload(L, A)
    try:
        assert dmat_dims(L, dA) == (nr, nc, A.nnz)
        for off in (0, 8):
            dx, dy = DevArray(x, off), DevArray.empty(nr, off=off)
            L.check(L.lib.ipd_spmv_dev(L.get_ctx().handle, dA, dx.ptr, dy.ptr))
            y = dy.read()
            ok, worst = D.within(y, ref, bound)
            print("spmv %s +%d: worst |y - ref| / bound = %.3f" % (name, off, worst))
            assert ok, (off, worst)
            dx.assert_unchanged("x")
            free_all(dx, dy)
    finally:
        L.lib.ipd_dmat_destroy(dA)


def test_spmv_dev_of_asat_dev_is_ax_of_aty(L):
    """H*y == Ax(s .* Aty(y)) with H = ASAt(s, p, q), every step a _dev entry (the product with s on the host).
    Bound: the sum of the two routes' bounds.  Route 2 sums exactly the terms p_i (p_i y_j + y_{n+i} q_j) of route
    1, regrouped; the rounding of z's two products and one add is at most 2u of sum |h| |y|, the stored values of
    H carry one rounding (off the diagonal) or cnt roundings (the diagonal's sum of cnt squares): with the len =
    cnt + 1 of the row walk that is (2 cnt + 3) u sum |h| |y|, inside spmv_ref's 2 (len + 1) u; the sum over s .* z
    is inside ax_ref's bound."""
    m, n = 72, 65
    p, q = asat_pq(m, n)
    s = D.mask_bytes(m, n, 0.5, "mixed")
    y = np.random.RandomState(5).standard_normal(m + n)
    ctx = L.get_ctx().handle
    ds, dp, dq, dy = DevArray(s, 1), DevArray(p, 8), DevArray(q, 8), DevArray(y, 8)
    H = asat_dev(L, ds, dp, dq, m, n)
    try:
        Hy = DevArray.empty(m + n, off=8)
        L.check(L.lib.ipd_spmv_dev(ctx, H, dy.ptr, Hy.ptr))
        route1 = Hy.read()
        dz = DevArray.empty(m * n, off=8)
        L.check(L.lib.ipd_aty_dev(ctx, dy.ptr, dp.ptr, dq.ptr, c_int64(m), c_int64(n), dz.ptr))
        sz = np.where(s != 0, dz.read(), 0.0)
        dsz, out = DevArray(sz, 8), DevArray.empty(m + n)
        L.check(L.lib.ipd_ax_dev(ctx, dsz.ptr, dp.ptr, dq.ptr, c_int64(m), c_int64(n), out.ptr))
        route2 = out.read()
    finally:
        L.lib.ipd_dmat_destroy(H)
    _, b1 = D.spmv_ref(sp.csr_matrix(O.ASAt(s != 0, p, q)), y)
    _, b2 = D.ax_ref(sz, p, q)
    ok, worst = D.within(route1, route2.astype(D.LD), b1 + b2)
    print("H*y against Ax(s .* Aty(y)): worst difference / bound = %.3f" % worst)
    assert ok, worst
    assert np.linalg.norm(route1) > 1.0
    for d in (ds, dp, dq, dy):
        d.assert_unchanged()
    free_all(ds, dp, dq, dy, Hy, dz, dsz, out)


# ---------------------------------------------------------------------------------------------------------------
# 4. ipd_amg_setup_dev / ipd_amg_solve_dev
# ---------------------------------------------------------------------------------------------------------------
RES_TOL = 1e-10          # tests/test_gpu_cycle.py


def solve_mode(L, handle):
    mode, grid, tmo = c_int32(), c_int32(), c_int32()
    L.check(L.lib.ipd_amg_solve_mode(handle, byref(mode), byref(grid), byref(tmo)))
    return mode.value, tmo.value


def tree64():
    """tests/test_gpu_cycle.py's tree64 system and solve"""
    from tests.test_gpu_setup import newton_matrix
    m = n = 64
    Ae, pd = newton_matrix(m, n, PR.mask_tree(m, n, seed=1))
    f = np.concatenate([pd["q"], -pd["p"]]) * pd["z"]
    o = O.amg_options_class1("v")
    o.update(fnode=n, isnsp=1)
    return sp.csr_matrix(Ae), f, o, pd


def bern256():
    """tests/test_gpu_resident_instantiations.py's smallest resident system (k_resident<4,4,0>, 512 / 256 / 1)"""
    from tests.test_gpu_bench_workload import options
    from tests.test_gpu_resident_instantiations import BERN256, synthetic
    Ae, f, n = synthetic(*BERN256)[:3]
    o = options("v", n)
    o["smoth"] = 1
    return sp.csr_matrix(Ae), f, o, dict(bk1=PR.BK1, tk=PR.TK)


# tree64 is the smallest system of the suite in each mode: IPD_NO_SMALL alone hands it to the resident kernel, the
# launches need both switches.  These three meet the oracle at test_class_amg_residual_history's bar.  bern256 is the
# smallest system the planner itself takes resident; it is compared with the host entries bit for bit like the others,
# and with the oracle by the suite's rule for the dense resident systems (test_gpu_bench_workload.same_history: its
# history reaches the rounding floor, 4e-11 against retol = 1e-11, and stops where the residual first rises -- 6
# cycles here, 8 in the oracle -- which the other bar's "counts differ by one" does not allow for).
MODE_CASES = [("launches", tree64, dict(IPD_NO_SMALL=1, IPD_NO_RESIDENT=1), 0, "cycle"),
              ("one_workgroup", tree64, {}, 1, "cycle"),
              ("resident", tree64, dict(IPD_NO_SMALL=1), 2, "cycle"),
              ("resident_as_planned", bern256, {}, 2, "floor")]


class DevSolve:
    def __init__(self, L, handle, N, maxit):
        self.L, self.handle, self.N, self.maxit = L, handle, N, maxit

    def __call__(self, db, dg, off=0):
        L = self.L
        dx = DevArray.empty(self.N, off=off)
        it, rel = c_int32(-1), c_double(-1.0)
        rk, rho = np.full(self.maxit + 2, np.nan), np.full(self.maxit + 2, np.nan)
        L.check(L.lib.ipd_amg_solve_dev(self.handle, db.ptr, dg.ptr if dg is not None else None, dx.ptr, byref(it),
                                        byref(rel), L.dptr(rk), L.dptr(rho)))
        x = dx.read()
        dx.free()
        k = it.value + 1
        return x, it.value, rel.value, rk[:k].copy(), rho[:k].copy()


def same_solve(a, b):
    return (np.array_equal(bits(a[0]), bits(b[0])) and a[1] == b[1] and bits([a[2]])[0] == bits([b[2]])[0]
            and np.array_equal(bits(a[3]), bits(b[3])) and np.array_equal(bits(a[4]), bits(b[4])))


@pytest.mark.parametrize("name,make,kv,mode,bar", MODE_CASES, ids=[c[0] for c in MODE_CASES])
def test_amg_setup_and_solve_dev(ipd, L, name, make, kv, mode, bar):
    """ipd_dmat_upload -> ipd_amg_setup_dev -> ipd_amg_solve_dev in each solve mode against ipd_amg_setup +
    ipd_amg_solve on the same matrix with the same replayed rand stream: bit for bit; against the oracle at
    test_class_amg_residual_history's bar.  The hierarchy holds a copy of A: the ipd_dmat is destroyed after the
    setup and its memory taken by another matrix (same pattern, other values) before the last solve."""
    A, f, o, pd = make()
    N = A.shape[0]
    guess = pd["bk1"] * pd["tk"] * np.random.RandomState(4).random_sample(N)
    replay = O.matlab_rng().random_sample(50000)
    ctx = L.get_ctx().handle
    with env(**kv):
        rng_h = ipd.MatlabRand(replay=replay)
        hh = ipd.AMGHierarchy(A, o, rng_h)
        dA = dmat_upload(L, A)
        rng_d = ipd.MatlabRand(replay=replay)
        opts = ipd.api._opts_struct(o)
        hd = c_void_p()
        L.check(L.lib.ipd_amg_setup_dev(ctx, dA, byref(opts), rng_d.handle, byref(hd)))
    try:
        assert solve_mode(L, hd) == (mode, 0) and solve_mode(L, hh.handle) == (mode, 0)
        assert rng_d.consumed == rng_h.consumed
        J = int(L.lib.ipd_amg_num_levels(hd))
        assert J == hh.J
        for k in range(1, J + 1):
            rows, nnz = c_int64(), c_int64()
            L.check(L.lib.ipd_amg_level_dims(hd, c_int(k), byref(rows), byref(nnz)))
            assert (rows.value, nnz.value) == hh.level_dims(k), k
        host = hh.solve(f, guess)
        host0 = hh.solve(f, None)
        solve = DevSolve(L, hd, N, int(o["maxit"]))
        db, dg, dzero = DevArray(f, 8), DevArray(guess, 8), DevArray(np.zeros(N))
        dev = solve(db, dg)
        assert same_solve(dev, host), (dev[1:], host[1:])
        assert same_solve(solve(db, dg, off=8), host)                      # x_dev at +8
        assert same_solve(solve(db, None), host0)                          # guess_dev = NULL ...
        assert same_solve(solve(db, dzero), host0)                         # ... is an all-zero guess
        assert host[1] >= 2 and not np.array_equal(host[0], host0[0])
        # the oracle, at tests/test_gpu_cycle.py::test_class_amg_residual_history's bar
        xo, ito, relo, rko, rhoo = O.Class_AMG(A, f, dict(o, guess=guess), O.matlab_rng())
        x, it, rel, rk, rho = dev
        k = min(len(rk), len(rko))
        print("%s: it %d / %d, max |rk - rko| = %.3e" % (name, it, ito, np.max(np.abs(rk[:k] - rko[:k]))))
        assert np.max(np.abs(rk[:k] - rko[:k])) <= RES_TOL, (rk, rko)
        if bar == "floor":
            from tests.test_gpu_bench_workload import same_history
            same_history(it, rk, ito, rko, tol=RES_TOL)
        elif it != ito:
            assert abs(it - ito) == 1 and abs(rko[k - 1] - o["retol"]) <= RES_TOL, (it, ito, rk, rko)
        big = rko[:k] > 1e-8
        assert np.allclose(rk[:k][big], rko[:k][big], rtol=1e-6)
        assert np.linalg.norm(A @ x - f) <= max(10 * relo, 1e-10) * np.linalg.norm(A @ guess - f)
        # lifetime: the hierarchy does not read the caller's matrix after the setup
        L.lib.ipd_dmat_destroy(dA)
        dA = dmat_upload(L, 2.0 * A)
        assert same_solve(solve(db, dg), host)
        assert solve_mode(L, hd) == (mode, 0)
        for d in (db, dg, dzero):
            d.assert_unchanged()
        free_all(db, dg, dzero)
    finally:
        L.lib.ipd_dmat_destroy(dA)
        L.lib.ipd_amg_destroy(hd)
        hh.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. ipd_asat_dev -> ipd_hybrid_amg_dev
# ---------------------------------------------------------------------------------------------------------------
HYBRID_CASES = [
    ("tree_connected", 96, 96, lambda: PR.mask_tree(96, 96, seed=1), None),
    ("tree_multi", 200, 200, lambda: PR.mask_tree(200, 200, seed=2, connect=False), None),
    ("class2_T", 150, 150, lambda: PR.mask_tree(150, 150, seed=5, connect=False), 0.7),
    ("empty", 40, 40, lambda: np.zeros(1600, np.uint8), None),
]


class HybridDev:
    """A problem on the device: s, p, q, z, t uploaded at +8 (s at +1), H0 from ipd_asat_dev."""

    def __init__(self, L, pd, t, build_h0=True):
        self.L, self.m, self.n, self.pd = L, pd["m"], pd["n"], pd
        self.ds, self.dp, self.dq = DevArray(pd["s"], 1), DevArray(pd["p"], 8), DevArray(pd["q"], 8)
        self.dz = DevArray(pd["z"], 8)
        self.dt = DevArray(t, 8) if t is not None else None
        self.H0 = asat_dev(L, self.ds, self.dp, self.dq, self.m, self.n) if build_h0 else None

    def call(self, opts, rng, off=0, H0=None, null=(), dq=None):
        L, M = self.L, self.m + self.n
        dzeta = DevArray.empty(M, off=off)
        it, res, info = c_int32(-1), c_double(-1.0), np.full(2, -1, np.int64)
        from codes_of_ipd_ssn_amg_method_amd import api
        o = api._opts_struct(opts)
        arg = dict(p=self.dp.ptr, q=(dq or self.dq).ptr, z=self.dz.ptr, zeta=dzeta.ptr)
        for k in null:
            arg[k] = None
        rc = L.lib.ipd_hybrid_amg_dev(L.get_ctx().handle, H0 or self.H0, self.dt.ptr if self.dt is not None else None,
                                      arg["p"], arg["q"], c_int64(self.m), c_int64(self.n), c_double(self.pd["bk1"]),
                                      c_double(self.pd["tk"]), arg["z"], byref(o), rng.handle, arg["zeta"], byref(it),
                                      byref(res), L.iptr(info))
        zeta = dzeta.read()
        dzeta.free()
        return rc, zeta, it.value, res.value, info

    def assert_inputs_unchanged(self):
        for d in (self.ds, self.dp, self.dq, self.dz, self.dt):
            if d is not None:
                d.assert_unchanged()

    def close(self):
        if self.H0:
            self.L.lib.ipd_dmat_destroy(self.H0)
        free_all(self.ds, self.dp, self.dq, self.dz, self.dt)


def hybrid_problem(m, n, mk, tfrac):
    s = mk()
    t = None
    if tfrac is not None:
        t = (np.random.RandomState(9).random_sample(m + n) < tfrac).astype(float)
    pd = PR.make_prob(m, n, s, t=t, pq_random=True)
    pd["H0"] = O.ASAt(s, pd["p"], pd["q"])
    opts = O.amg_options_class1("v") if tfrac is None else O.amg_options_class2("w")
    return pd, t, opts


@pytest.mark.parametrize("name,m,n,mk,tfrac", HYBRID_CASES, ids=[c[0] for c in HYBRID_CASES])
def test_hybrid_amg_dev(ipd, L, name, m, n, mk, tfrac):
    """H0 built on the device by ipd_asat_dev (nnz = 0 for the empty active set), t_dev given for class2_T and NULL
    otherwise: equal to ipd.Hybrid_AMG on the same problem -- info, itamg, resamg, rand numbers consumed, zeta bit
    for bit -- and to the oracle at tests/test_gpu_hybrid.py's bars; zeta_dev at +8."""
    pd, t, opts = hybrid_problem(m, n, mk, tfrac)
    rng_h = ipd.MatlabRand()
    zh, ith, resh, infoh = ipd.Hybrid_AMG(pd, opts, rng_h)
    hd = HybridDev(L, pd, t)
    try:
        assert dmat_dims(L, hd.H0) == (m + n, m + n, pd["H0"].nnz)
        for off in (0, 8):
            rng = ipd.MatlabRand()
            rc, z, it, res, info = hd.call(opts, rng, off=off)
            L.check(rc)
            assert np.array_equal(info, infoh) and it == ith and rng.consumed == rng_h.consumed, off
            assert bits([res])[0] == bits([resh])[0] and np.array_equal(bits(z), bits(zh)), off
        hd.assert_inputs_unchanged()
    finally:
        hd.close()
    tr = []
    zo, ito, reso, infoo = O.Hybrid_AMG(pd, opts, O.matlab_rng(), trace=tr)
    assert np.array_equal(info, infoo)
    noise_floor = res <= 1e-10 and reso <= 1e-10
    assert abs(it - ito) <= 1 or (noise_floor and abs(it - ito) <= 3), (it, ito, res, reso)
    M = m + n
    He = pd["bk1"] * sp.identity(M) + (pd["T"] + pd["H0"]) / pd["tk"]
    nz = np.linalg.norm(pd["z"])
    assert np.linalg.norm(He @ z - pd["z"]) <= max(1e-9, 20 * np.linalg.norm(He @ zo - pd["z"]) / nz) * nz
    assert np.linalg.norm(z - zo) <= 1e-5 * max(1.0, np.linalg.norm(zo))
    used = sum(len(t_["guess"]) + sum(len(i["mis"]["rand"]) for i in t_["h"].info[2:] if i and i.get("mis"))
               for t_ in tr)
    assert rng.consumed == used


def test_hybrid_amg_dev_refusals(ipd, L):
    """Each refusal is IPD_E_ARG, writes no zeta, and leaves the context able to give the right bits."""
    m = n = 96
    pd, t, opts = hybrid_problem(m, n, lambda: PR.mask_tree(96, 96, seed=1), None)
    hd = HybridDev(L, pd, None)
    other = hybrid_problem(m + 8, n, lambda: PR.mask_tree(m + 8, n, seed=1), None)[0]
    ho = HybridDev(L, other, None)
    qz = pd["q"].copy()
    qz[3] = 0.0
    dqz = DevArray(qz, 8)
    try:
        rc, good, it0, res0, info0 = hd.call(opts, ipd.MatlabRand())
        L.check(rc)
        assert it0 >= 1 and not np.any(good == D.SENTINEL)
        refusals = [("zero in q", dict(dq=dqz), "p or q contains 0"),
                    ("H0 of another (m, n)", dict(H0=ho.H0), "H0 must be"),
                    ("p NULL", dict(null=("p",)), "NULL"), ("q NULL", dict(null=("q",)), "NULL"),
                    ("z NULL", dict(null=("z",)), "NULL"), ("zeta NULL", dict(null=("zeta",)), "NULL")]
        for what, kw, msg in refusals:
            rc, z, it, res, info = hd.call(opts, ipd.MatlabRand(), **kw)
            assert rc == L.IPD_E_ARG, (what, rc)
            assert msg in L.lib.ipd_last_error().decode(), (what, L.lib.ipd_last_error())
            assert np.all(z == D.SENTINEL), what                           # nothing was delivered
            rc, z, it, res, info = hd.call(opts, ipd.MatlabRand())
            L.check(rc)
            assert np.array_equal(bits(z), bits(good)) and it == it0 and np.array_equal(info, info0), what
        hd.assert_inputs_unchanged()
    finally:
        hd.close()
        ho.close()
        dqz.free()


# ---------------------------------------------------------------------------------------------------------------
# 6. raw memory
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [1, 7, 8, 4097])
def test_h2d_d2h_round_trip(L, nbytes):
    ctx = L.get_ctx().handle
    src = np.random.RandomState(nbytes).randint(0, 256, nbytes).astype(np.uint8)
    buf = L.DeviceBuffer(nbytes + 16)
    fill = np.full(nbytes + 16, 0xA5, np.uint8)
    L.check(L.lib.ipd_h2d(ctx, buf.ptr, fill.ctypes.data_as(c_void_p), c_size_t(nbytes + 16)))
    for off in (0, 1, 8):
        L.check(L.lib.ipd_h2d(ctx, c_void_p(buf.ptr.value + off), src.ctypes.data_as(c_void_p), c_size_t(nbytes)))
        back = np.zeros(nbytes + 2, np.uint8)                              # one guard byte on either side
        L.check(L.lib.ipd_d2h(ctx, c_void_p(back.ctypes.data + 1), c_void_p(buf.ptr.value + off), c_size_t(nbytes)))
        assert np.array_equal(back[1:-1], src) and back[0] == 0 and back[-1] == 0, off
        whole = buf.to_array(np.uint8, nbytes + 16)
        assert np.all(whole[:off] == 0xA5) and np.all(whole[off + nbytes:] == 0xA5), off
        L.check(L.lib.ipd_h2d(ctx, buf.ptr, fill.ctypes.data_as(c_void_p), c_size_t(nbytes + 16)))
    assert L.lib.ipd_h2d(None, buf.ptr, src.ctypes.data_as(c_void_p), c_size_t(nbytes)) == L.IPD_E_ARG
    assert L.lib.ipd_d2h(None, src.ctypes.data_as(c_void_p), buf.ptr, c_size_t(nbytes)) == L.IPD_E_ARG
    assert np.all(buf.to_array(np.uint8, nbytes + 16) == 0xA5)
    buf.free()
