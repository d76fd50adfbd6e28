"""The transport plan as a sparse matrix out of and into the drivers' device workspace
(csrc/ipd_plan.hip: ipd_apd_plan, ipd_apd_plan_dev, ipd_apd_set_plan).

Reference: Xd = u[:mn].reshape((m, n), order="F"), K = ~(abs(Xd) <= tol); the plan is
scipy.sparse.csc_matrix(np.where(K, Xd, 0)) -- or the same arrays built by hand where NaNs are
present.  Bars: jc, ir, nnz, max_dropped equal, pr bit-equal; the sums to 1e-12 relative to
sum|x| resp. sum|c.*x| (the bar for reductions of tests/test_gpu_driver.py); ax against O.Ax of the
thresholded dense vector at the bar of tests/test_gpu_kkt.py (1e-13 * max(1,|ref|) * max(m,n)).
States are injected with set_state; only the last two groups run the drivers."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

from oracle import ipd_oracle as O       # noqa: E402


def ipd():
    import codes_of_ipd_ssn_amg_method_amd as pkg
    return pkg


def lib_mod():
    from codes_of_ipd_ssn_amg_method_amd import _lib
    return _lib


def problem(cls, m, n, seed=1, pq_random=False):
    """tests/test_gpu_driver.py's synthetic inputs, re-stated: c,r,l ~ U(0,1) (draw order c,r,l),
    p=q=1, phi=1 unless pq_random."""
    rs = np.random.RandomState(seed)
    c = rs.random_sample(m * n)
    r = rs.random_sample(n)
    l = rs.random_sample(m)
    p, q = np.ones(m), np.ones(n)
    if pq_random:
        p, q = 0.5 + rs.random_sample(m), 0.5 + rs.random_sample(n)
    if cls == 1:
        l = l * (r @ q) / (l @ p)      # <r,q> = <l,p>
        return dict(c=c, r=r, l=l, p=p, q=q)
    phi = np.ones(m * n) if not pq_random else 0.5 + rs.random_sample(m * n)
    mu = 0.65 * min(r.sum(), l.sum())
    return dict(c=c, r=r, l=l, p=p, q=q, mu=mu, phi=phi)


def ws_of(cls, pr):
    if cls == 1:
        return ipd().APDWorkspace(1, pr["c"], pr["r"], pr["l"], pr["p"], pr["q"], gama=np.inf)
    return ipd().APDWorkspace(2, pr["c"], pr["r"], pr["l"], pr["p"], pr["q"], mu=pr["mu"],
                              phi=pr["phi"])


def ref_plan(Xd, tol):
    """(jc, ir, pr, K) of the thresholded plan, built by hand (works with NaNs)."""
    K = ~(np.abs(Xd) <= tol)
    jc = np.concatenate([[0], np.cumsum(K.sum(axis=0))]).astype(np.int64)
    cols, rows = np.nonzero(K.T)          # column-major order: columns outer, rows ascending
    return jc, rows.astype(np.int64), Xd[rows, cols], K


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def inject(ws, Xd, rs):
    """state with the x block of u = Xd(:), everything else random; returns (u, v, lam)."""
    u = rs.standard_normal(ws.U)
    u[:ws.m * ws.n] = Xd.reshape(-1, order="F")
    v = rs.standard_normal(ws.U)
    lam = rs.standard_normal(ws.L)
    ws.set_state(u, v, lam, 0.37)
    return u, v, lam


def patterns(m, n, rs):
    val = lambda: 0.25 + rs.random_sample((m, n))
    sign = np.where(rs.random_sample((m, n)) < 0.3, -1.0, 1.0)
    out = {"zero": np.zeros((m, n)), "dense": val() * sign,
           "bernoulli": val() * sign * (rs.random_sample((m, n)) < 0.05)}
    gaps = val()
    gaps[:, 1::3] = 0.0
    gaps[:, 2::3] = 0.0
    out["empty_columns"] = gaps              # columns 0, 3, 6, ... full, the others empty
    last = np.zeros((m, n))
    last[m - 1, :] = val()[m - 1, :]
    last[:, n - 1] = val()[:, n - 1]
    out["last_row_and_column"] = last
    return out


def check_extraction(ws, pr, Xd, tol):
    m, n = Xd.shape
    jc, ir, prv, K = ref_plan(Xd, tol)
    X, st, ax = ws.plan(tol, stats=True)
    assert X.shape == (m, n)
    assert np.array_equal(X.indptr, jc), "jc differs"
    assert np.array_equal(X.indices, ir), "ir differs"
    assert np.array_equal(bits(X.data), bits(prv)), "pr differs"
    Xt = np.where(K, Xd, 0.0)
    if not np.isnan(Xd).any():
        R = sp.csc_matrix(Xt)
        R.sort_indices()
        assert np.array_equal(X.indptr, R.indptr) and np.array_equal(X.indices, R.indices)
        assert np.array_equal(bits(X.data), bits(R.data))
    dropped = np.abs(Xd[~K])
    assert st["nnz"] == int(K.sum())
    assert st["max_dropped"] == (dropped.max() if dropped.size else 0.0)
    C = pr["c"].reshape((m, n), order="F")
    sx = np.abs(Xd).sum()
    scx = np.abs(C * Xd).sum()
    print("sum_kept err %.3e  sum_dropped err %.3e  fval_kept err %.3e  (scales %.3e %.3e)" % (
        abs(st["sum_kept"] - Xd[K].sum()), abs(st["sum_dropped"] - dropped.sum()),
        abs(st["fval_kept"] - (C * Xd)[K].sum()), sx, scx))
    assert abs(st["sum_kept"] - Xd[K].sum()) <= 1e-12 * sx
    assert abs(st["sum_dropped"] - dropped.sum()) <= 1e-12 * sx
    assert abs(st["fval_kept"] - (C * Xd)[K].sum()) <= 1e-12 * scx
    ref_ax = O.Ax(Xt.reshape(-1, order="F"), pr["p"], pr["q"])
    print("ax err %.3e" % np.max(np.abs(ax - ref_ax)))
    assert np.max(np.abs(ax - ref_ax)) <= 1e-13 * max(1.0, np.max(np.abs(ref_ax))) * max(m, n)
    return X, st, ax


# the smallest shapes at which the walk can go wrong: degenerate dimensions, a wave boundary in the
# rows and a chunk boundary in the columns, one row past a 256-row workgroup, three row blocks
SHAPES = [(1, 1), (1, 37), (37, 1), (63, 17), (64, 16), (65, 33), (257, 19), (600, 45)]


@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", SHAPES)
def test_extraction(cls, m, n):
    pr = problem(cls, m, n, seed=3, pq_random=True)
    ws = ws_of(cls, pr)
    rs = np.random.RandomState(100 * m + n)
    for name, Xd in patterns(m, n, rs).items():
        inject(ws, Xd, rs)
        X, st, _ = check_extraction(ws, pr, Xd, 0.0)
        if name == "zero":
            assert st["nnz"] == 0 and not X.indptr.any()
        # a threshold inside the value range as well: part of the entries is dropped
        check_extraction(ws, pr, Xd, 0.5)
    ws.close()


@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("tol", [0.0, 0.375, 1e-9])
def test_threshold_edge(cls, tol):
    """Kept means exactly !(|x| <= tol): tol itself goes, its successor stays, a NaN stays."""
    m, n = 65, 33
    pr = problem(cls, m, n, seed=4, pq_random=True)
    ws = ws_of(cls, pr)
    rs = np.random.RandomState(5)
    up = np.nextafter(tol, np.inf)
    vals = np.array([0.0, -0.0, tol, up, -tol, -up])
    Xd = vals[rs.randint(0, vals.size, size=(m, n))]
    Xd[40, 20] = np.nan
    inject(ws, Xd, rs)
    jc, ir, prv, K = ref_plan(Xd, tol)
    assert K[40, 20] and np.array_equal(K, np.isnan(Xd) | (np.abs(Xd) == up))
    X, st, _ = ws.plan(tol, stats=True)
    assert np.array_equal(X.indptr, jc) and np.array_equal(X.indices, ir)
    assert np.array_equal(bits(X.data), bits(prv))
    assert st["nnz"] == int(K.sum())
    assert st["max_dropped"] == tol
    if tol == 0.0:
        # scipy's nonzero pattern (NaN != 0 counts as a nonzero there as well)
        R = sp.csc_matrix(Xd)
        R.eliminate_zeros()
        R.sort_indices()
        assert np.isnan(R[40, 20])
        assert np.array_equal(X.indptr, R.indptr) and np.array_equal(X.indices, R.indices)
        assert np.array_equal(bits(X.data), bits(R.data))
    ws.close()


SENT_I, SENT_F = -7777, -1234.5


@pytest.mark.parametrize("cls", [1, 2])
def test_device_variant(cls):
    L = lib_mod()
    m, n = 257, 19
    pr = problem(cls, m, n, seed=6, pq_random=True)
    ws = ws_of(cls, pr)
    rs = np.random.RandomState(8)
    Xd = patterns(m, n, rs)["bernoulli"]
    inject(ws, Xd, rs)
    Xh, sth, axh = ws.plan(0.0, stats=True)
    nnz = Xh.nnz
    assert nnz > 1

    def attempt(cap):
        jc = L.DeviceBuffer.from_array(np.full(n + 1, SENT_I, np.int64))
        ir = L.DeviceBuffer.from_array(np.full(max(cap, 1), SENT_I, np.int64))
        prb = L.DeviceBuffer.from_array(np.full(max(cap, 1), SENT_F, np.float64))
        ax = L.DeviceBuffer.from_array(np.full(m + n, SENT_F, np.float64))
        code, st = 0, None
        try:
            st = ws.plan_dev(0.0, jc, (ir.ptr.value, cap), (prb.ptr.value, cap), ax)
        except L.IpdError as e:
            code, st = e.code, e.stats
        res = (code, st, jc.to_array(np.int64, n + 1), ir.to_array(np.int64, max(cap, 1)),
               prb.to_array(np.float64, max(cap, 1)), ax.to_array(np.float64, m + n))
        for b in (jc, ir, prb, ax):
            b.free()
        return res

    code, st, jc, ir, prv, ax = attempt(0)                 # the size query
    assert code == L.IPD_E_LIMIT and st["nnz"] == nnz
    assert np.array_equal(jc, Xh.indptr)
    assert ir[0] == SENT_I and prv[0] == SENT_F
    code, st, jc, ir, prv, ax = attempt(nnz)
    assert code == 0 and st == sth
    assert np.array_equal(jc, Xh.indptr) and np.array_equal(ir, Xh.indices)
    assert np.array_equal(bits(prv), bits(Xh.data))
    assert np.array_equal(bits(ax), bits(axh))
    code, st, jc, ir, prv, ax = attempt(nnz - 1)
    assert code == L.IPD_E_LIMIT and st["nnz"] == nnz
    assert np.array_equal(jc, Xh.indptr)
    assert (ir == SENT_I).all() and (prv == SENT_F).all()
    # anything with torch's tensor interface is taken as it is (a stand-in over library memory:
    # the suite keeps a second HIP runtime out of this process)
    class Tensor:
        def __init__(self, count, dtype):
            self.buf, self.count, self.dtype = L.DeviceBuffer.from_array(np.zeros(count, dtype)), count, dtype

        def data_ptr(self):
            return self.buf.ptr.value

        def element_size(self):
            return 8

        def is_contiguous(self):
            return True

        def numel(self):
            return self.count

        def numpy(self):
            return self.buf.to_array(self.dtype, self.count)

    tjc, tir = Tensor(n + 1, np.int64), Tensor(nnz + 3, np.int64)
    tpr, tax = Tensor(nnz + 3, np.float64), Tensor(m + n, np.float64)
    st = ws.plan_dev(0.0, tjc, tir, tpr, tax)
    assert st == sth
    assert np.array_equal(tjc.numpy(), Xh.indptr)
    assert np.array_equal(tir.numpy()[:nnz], Xh.indices)
    assert np.array_equal(bits(tpr.numpy()[:nnz]), bits(Xh.data))
    assert np.array_equal(bits(tax.numpy()), bits(axh))
    ws.close()


@pytest.mark.parametrize("cls", [1, 2])
def test_two_calls_give_the_same_bits(cls):
    m, n = 600, 45
    pr = problem(cls, m, n, seed=7, pq_random=True)
    ws = ws_of(cls, pr)
    rs = np.random.RandomState(9)
    Xd = patterns(m, n, rs)["dense"] * (rs.random_sample((m, n)) < 0.4)
    inject(ws, Xd, rs)
    for tol in (0.0, 0.6):
        X1, st1, ax1 = ws.plan(tol, stats=True)
        X2, st2, ax2 = ws.plan(tol, stats=True)
        assert np.array_equal(X1.indptr, X2.indptr) and np.array_equal(X1.indices, X2.indices)
        assert np.array_equal(bits(X1.data), bits(X2.data))
        assert np.array_equal(bits(ax1), bits(ax2))
        assert st1["nnz"] == st2["nnz"]
        for k in ("sum_kept", "sum_dropped", "max_dropped", "fval_kept"):
            assert bits([st1[k]])[0] == bits([st2[k]])[0], k
    ws.close()


# ---------------------------------------------------------------------------
# set_plan
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", [(1, 1), (65, 33), (257, 19)])
def test_set_plan_round_trip(cls, m, n):
    pr = problem(cls, m, n, seed=10, pq_random=True)
    ws = ws_of(cls, pr)
    rs = np.random.RandomState(11)
    Xd = np.abs(patterns(m, n, rs)["bernoulli"])      # non-negative: no -0.0
    if m * n == 1:
        Xd[0, 0] = 0.75
    u, v, lam, = inject(ws, Xd, rs)
    X = ws.plan(0.0)
    ws.set_state(rs.standard_normal(ws.U), None, None, 0.37)      # something else in u
    ws.set_plan(X)
    u2, v2, lam2, bk2 = ws.state()
    mn = m * n
    assert np.array_equal(bits(u2[:mn]), bits(u[:mn]))
    assert np.array_equal(bits(v2[:mn]), bits(u[:mn]))
    assert np.array_equal(bits(lam2), bits(lam)) and bk2 == 0.37
    if cls == 2:
        ws.set_state(u, v, lam, 0.37)
        ws.set_plan(X)
        u3, v3, lam3, bk3 = ws.state()
        assert np.array_equal(bits(u3[mn:]), bits(u[mn:])), "y, z blocks of uk"
        assert np.array_equal(bits(v3[mn:]), bits(v[mn:])), "y, z blocks of vk"
        assert np.array_equal(bits(v3[:mn]), bits(u[:mn]))
        assert np.array_equal(bits(lam3), bits(lam)) and bk3 == 0.37
    ws.set_plan(sp.csc_matrix((m, n)))                 # the empty plan
    u4, v4, _, _ = ws.state()
    assert not u4[:mn].any() and not v4[:mn].any()
    ws.close()


AMG1 = dict(retol=1e-11, bigph=1, maxit=30, theta=1 / 4, smoth=5, cycle="w", isnsp=1, inter=1, guess=None)
AMG2 = dict(retol=1e-11, bigph=1, maxit=40, theta=1 / 4, smoth=10, cycle="w", isnsp=1, inter=1, guess=None)


@pytest.mark.parametrize("cls", [1, 2])
def test_set_plan_then_run_equals_set_state_then_run(cls):
    m = n = 24
    pr = problem(cls, m, n, seed=12)
    w0 = ws_of(cls, pr)
    w0.warmup(0.0, 40)
    u, _, lam, bk = w0.state()
    w0.close()
    mn = m * n
    full = u.copy()
    full[:mn] = np.where(np.abs(u[:mn]) <= 1e-3, 0.0, u[:mn])       # a thresholded warm start
    X = sp.csc_matrix(full[:mn].reshape((m, n), order="F"))
    outs = []
    for via_plan in (False, True):
        ws = ws_of(cls, pr)
        if via_plan:
            ws.set_state(full, full, lam, bk)     # y, z blocks, lk, bk; the x blocks go in sparse
            ws.set_state(np.where(np.arange(ws.U) < mn, 7.0, full), None, None, bk)
            vv = full.copy()
            vv[:mn] = -3.0
            ws.set_state(None, vv, None, bk)
            ws.set_plan(X)
        else:
            ws.set_state(full, full, lam, bk)
            ws.set_state(full, full, None, bk)
        res = ws.run(AMG1 if cls == 1 else AMG2, ipd().MatlabRand(), iters=2)
        outs.append((res, ws.history(), ws.records(), ws.state()))
        ws.close()
    (ra, ha, ca, sa), (rb, hb, cb, sb) = outs
    assert ra["k"] == rb["k"] == 2
    assert ra == rb
    assert ha.keys() == hb.keys()
    for k in ha:
        assert np.array_equal(bits(ha[k]), bits(hb[k])), k
    assert ca == cb
    for a, b in zip(sa[:3], sb[:3]):
        assert np.array_equal(bits(a), bits(b))
    assert sa[3] == sb[3]


# ---------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------
def test_plan_argument_errors():
    L = lib_mod()
    lib = L.lib
    m, n = 37, 5
    pr = problem(1, m, n, seed=13)
    ws = ws_of(1, pr)
    out, st = L.ipd_csc_out(), L.ipd_plan_stats()
    h, E = ws.handle, L.IPD_E_ARG
    t0 = ctypes.c_double(0.0)
    jc = L.DeviceBuffer(8 * (n + 1))
    assert lib.ipd_apd_plan(None, t0, ctypes.byref(out), ctypes.byref(st), None) == E
    assert lib.ipd_apd_plan(h, t0, None, ctypes.byref(st), None) == E
    assert lib.ipd_apd_plan(h, t0, ctypes.byref(out), None, None) == E
    for bad in (-1e-300, -1.0, float("nan")):
        assert lib.ipd_apd_plan(h, ctypes.c_double(bad), ctypes.byref(out), ctypes.byref(st), None) == E
        assert lib.ipd_apd_plan_dev(h, ctypes.c_double(bad), ctypes.c_int64(0), jc.ptr, None, None,
                                    ctypes.byref(st), None) == E
    assert lib.ipd_apd_plan_dev(None, t0, ctypes.c_int64(0), jc.ptr, None, None, ctypes.byref(st), None) == E
    assert lib.ipd_apd_plan_dev(h, t0, ctypes.c_int64(0), jc.ptr, None, None, None, None) == E
    assert lib.ipd_apd_plan_dev(h, t0, ctypes.c_int64(-1), jc.ptr, None, None, ctypes.byref(st), None) == E
    assert lib.ipd_apd_set_plan(None, L.CscIn(sp.csc_matrix((m, n))).ref()) == E
    assert lib.ipd_apd_set_plan(h, None) == E
    jc.free()
    ws.close()


def test_set_plan_argument_errors_leave_the_state_alone():
    L = lib_mod()
    lib = L.lib
    m, n = 37, 5
    pr = problem(2, m, n, seed=14)
    ws = ws_of(2, pr)
    rs = np.random.RandomState(15)
    Xd = np.abs(patterns(m, n, rs)["dense"]) * (rs.random_sample((m, n)) < 0.3)
    inject(ws, Xd, rs)
    before = ws.state()
    good = sp.csc_matrix(0.5 * Xd)
    good.sort_indices()
    gjc, gir, gpr = good.indptr.astype(np.int64), good.indices.astype(np.int64), good.data.copy()
    assert gjc[2] - gjc[1] >= 2 and gjc[1] >= 1, "the cases below edit columns 0 and 1"

    def call(nrows, ncols, nnz, jc, ir, prv):
        jc, ir, prv = (np.ascontiguousarray(jc, np.int64), np.ascontiguousarray(ir, np.int64),
                       np.ascontiguousarray(prv, np.float64))
        s = L.ipd_csc(nrows, ncols, nnz, L.iptr(jc), L.iptr(ir), L.dptr(prv))
        return lib.ipd_apd_set_plan(ws.handle, ctypes.byref(s))

    def edited(a, idx, val):
        b = a.copy()
        b[idx] = val
        return b

    nnz = int(gjc[n])
    swapped = gir.copy()
    swapped[gjc[1]], swapped[gjc[1] + 1] = gir[gjc[1] + 1], gir[gjc[1]]
    cases = {
        "m+1 rows": (m + 1, n, nnz, gjc, gir, gpr),
        "n+1 columns": (m, n + 1, nnz, np.append(gjc, nnz), gir, gpr),
        "jc[0] != 0": (m, n, nnz, edited(gjc, 0, 1), gir, gpr),
        "jc decreasing": (m, n, nnz, edited(gjc, 2, gjc[1] - 1), gir, gpr),
        "jc[n] != nnz": (m, n, nnz - 1, gjc, gir, gpr),
        "row = m": (m, n, nnz, gjc, edited(gir, gjc[1] - 1, m), gpr),
        "row = -1": (m, n, nnz, gjc, edited(gir, 0, -1), gpr),
        "row repeated": (m, n, nnz, gjc, edited(gir, gjc[1] + 1, gir[gjc[1]]), gpr),
        "rows descending": (m, n, nnz, gjc, swapped, gpr),
    }
    for name, args in cases.items():
        assert call(*args) == L.IPD_E_ARG, name
        after = ws.state()
        for a, b in zip(before[:3], after[:3]):
            assert np.array_equal(bits(a), bits(b)), name
        assert before[3] == after[3]
    assert call(m, n, nnz, gjc, gir, gpr) == 0        # the unedited arrays are fine
    assert np.array_equal(ws.state()[0][:m * n], (0.5 * Xd).reshape(-1, order="F"))
    ws.close()


# ---------------------------------------------------------------------------
# after a real run
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [1, 2])
def test_plan_of_a_real_run(cls):
    pr = problem(cls, 32, 32, seed=2)
    if cls == 1:
        run = lambda **kw: ipd().APD_SsN_Class1(pr["c"], pr["r"], pr["l"], pr["p"], pr["q"], np.inf, **kw)
    else:
        run = lambda **kw: ipd().APD_SsN_Class2(pr["c"], pr["r"], pr["l"], pr["p"], pr["q"], pr["mu"],
                                                pr["phi"], **kw)
    out = run(plan_tol=0.0)
    base = run()
    assert out["converged"]
    x = out["xk"]
    R = sp.csc_matrix(x.reshape((32, 32), order="F"))
    R.sort_indices()
    X = out["plan"]
    assert X.shape == (32, 32) and out["plan_stats"]["nnz"] == R.nnz
    assert np.array_equal(X.indptr, R.indptr) and np.array_equal(X.indices, R.indices)
    assert np.array_equal(bits(X.data), bits(R.data))
    scx = np.abs(pr["c"] * x).sum()
    print("fval_kept - fval = %.3e (scale %.3e)" % (out["plan_stats"]["fval_kept"] - out["fval"], scx))
    assert abs(out["plan_stats"]["fval_kept"] - out["fval"]) <= 1e-12 * scx
    ref_ax = O.Ax(x, pr["p"], pr["q"])
    assert np.max(np.abs(out["plan_ax"] - ref_ax)) <= 1e-13 * max(1.0, np.max(np.abs(ref_ax))) * 32
    # without plan_tol: the same keys and bits as ever
    assert set(out) - set(base) == {"plan", "plan_stats", "plan_ax"} and set(base) <= set(out)
    for k, b in base.items():
        a = out[k]
        if isinstance(b, np.ndarray):
            assert np.array_equal(bits(a), bits(b)), k
        elif isinstance(b, float):
            assert bits([a])[0] == bits([b])[0], k
        else:
            assert a == b, k
