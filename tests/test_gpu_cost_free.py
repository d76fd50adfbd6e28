"""Matrix-free cost (ipd_apd_create_points_free, ipd_apd_cost_info): a workspace that keeps
the coordinates and no c, against the stored point-cloud workspace (ipd_apd_create_points), which is the code that
was there before.  An entry recomputed in a pass is folded by the code k_cost_build stores it with, and every
reduction runs in the stored pass's order, so everything is compared bit for bit (view(np.int64)): no tolerance
anywhere in this file.  For cost() the yardstick is the numpy definition (the `cost_ref` of tests/test_gpu_cost.py,
restated here)."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

METRICS = {"sqeuclidean": 1, "euclidean": 2, "cityblock": 3, "chebyshev": 4}
# the tile walker's edges: one entry, one row, one column, a wave not full, one row / column past a wave / chunk,
# more than one workgroup of rows, one column past two chunks
SHAPES = [(1, 1), (1, 70), (70, 1), (63, 5), (65, 17), (129, 31), (257, 33)]
TWO = [(65, 17), (129, 31)]
# (m, n, d, metric, scale)
CASES = [(m, n, 2, "sqeuclidean", False) for m, n in SHAPES] + \
        [(m, n, d, "sqeuclidean", False) for m, n in TWO for d in (1, 3)] + \
        [(m, n, 2, metric, False) for m, n in TWO for metric in ("euclidean", "cityblock", "chebyshev")] + \
        [(m, n, 2, "sqeuclidean", True) for m, n in TWO]
IDS = ["%dx%d-d%d-%s-%s" % (m, n, d, metric, "scaled" if scale else "plain") for m, n, d, metric, scale in CASES]
AMG1 = dict(retol=1e-11, bigph=1, maxit=30, theta=1 / 4, smoth=5, cycle="w", isnsp=1, inter=1, guess=None)
AMG2 = dict(retol=1e-11, bigph=1, maxit=40, theta=1 / 4, smoth=10, cycle="w", isnsp=1, inter=1, guess=None)


def ipd():
    import codes_of_ipd_ssn_amg_method_amd as pkg
    return pkg


def lib_mod():
    from codes_of_ipd_ssn_amg_method_amd import _lib
    return _lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def cost_ref(xs, ys, metric, scale=False):
    """The definition, in numpy: (m, d) and (n, d) points -> (m, n)."""
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    xs = xs[:, None] if xs.ndim == 1 else xs
    ys = ys[:, None] if ys.ndim == 1 else ys
    acc = np.zeros((xs.shape[0], ys.shape[0]))
    for k in range(xs.shape[1]):
        t = xs[:, k][:, None] - ys[:, k][None, :]
        if metric in ("sqeuclidean", "euclidean"):
            acc = acc + t * t
        elif metric == "cityblock":
            acc = acc + np.abs(t)
        else:
            acc = np.maximum(acc, np.abs(t))
    if metric == "euclidean":
        acc = np.sqrt(acc)
    if scale:
        acc = acc / acc.max()
    return acc


@functools.lru_cache(maxsize=None)
def problem(m, n, d, seed=0):
    """Points, marginals and one random state per class; read-only, shared by the tests."""
    rs = np.random.RandomState(1000 * seed + 7 * m + 3 * n + d)
    pr = dict(xs=rs.standard_normal((m, d)), ys=rs.standard_normal((n, d)), r=rs.random_sample(n),
              l=rs.random_sample(m), p=0.5 + rs.random_sample(m), q=0.5 + rs.random_sample(n),
              gvec=0.3 + rs.random_sample(m * n))
    pr["l1"] = pr["l"] * (pr["r"] @ pr["q"]) / (pr["l"] @ pr["p"])      # class 1: <r,q> = <l,p>
    pr["mu"] = 0.65 * min(pr["r"].sum(), pr["l"].sum())
    for cls, U, L in ((1, m * n, m + n), (2, m * n + m + n, m + n + 1)):
        pr["state", cls] = (rs.random_sample(U), rs.random_sample(U), rs.standard_normal(L))
        pr["other_u", cls] = rs.random_sample(U)
    for v in pr.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return pr


VARIANTS = ("class1-scalar-gama", "class1-vector-gama", "class2-phi-none")


def make(variant, pr, metric, scale, matrix_free):
    P = ipd()
    if variant.startswith("class1"):
        gama = 0.7 if variant == "class1-scalar-gama" else pr["gvec"]
        return P.APDWorkspace.from_points(1, pr["xs"], pr["ys"], pr["r"], pr["l1"], pr["p"], pr["q"], metric=metric,
                                          scale=scale, gama=gama, matrix_free=matrix_free)
    return P.APDWorkspace.from_points(2, pr["xs"], pr["ys"], pr["r"], pr["l"], pr["p"], pr["q"], metric=metric,
                                      scale=scale, mu=pr["mu"], phi=None, matrix_free=matrix_free)


def pair(variant, pr, metric="sqeuclidean", scale=False):
    """(matrix-free, stored) from the same points"""
    return make(variant, pr, metric, scale, True), make(variant, pr, metric, scale, False)


def same_plan(a, b):
    (Xa, sa, axa), (Xb, sb, axb) = a, b
    assert Xa.shape == Xb.shape and np.array_equal(Xa.indptr, Xb.indptr) and np.array_equal(Xa.indices, Xb.indices)
    assert same_bits(Xa.data, Xb.data) and same_bits(axa, axb)
    assert sa["nnz"] == sb["nnz"] and set(sa) == set(sb)
    for k in sa:
        assert same_bits([sa[k]], [sb[k]]), (k, sa[k], sb[k])
    return sa


def same_state(wa, wb):
    sa, sb = wa.state(), wb.state()
    for name, a, b in zip(("u", "v", "lam"), sa[:3], sb[:3]):
        assert same_bits(a, b), name
    assert sa[3] == sb[3]


def check_passes(variant, pr, metric, scale):
    """Every pass that reads c, one at a time, on both workspaces in the same state."""
    cls = 1 if variant.startswith("class1") else 2
    wa, wb = pair(variant, pr, metric, scale)
    try:
        m, n = wa.m, wa.n
        u, v, lam = pr["state", cls]
        for w in (wa, wb):
            w.set_state(u, v, lam, bk=0.8)
        # the plan of the random iterate: u is uniform in [0, 1), so tol = 0.5 drops about half of it
        st = same_plan(wa.plan(0.5, stats=True), wb.plan(0.5, stats=True))
        if m * n >= 60:        # (a single entry is kept or dropped)
            assert 0 < st["nnz"] < m * n and st["fval_kept"] != 0.0
        # begin
        assert wa.begin(3) == wb.begin(3)
        for a, b in zip(wa.get_w(), wb.get_w()):
            assert same_bits(a, b)
        # end, measuring another iterate
        ea, eb = wa.end(lam, from_w=False, u=pr["other_u", cls]), wb.end(lam, from_w=False, u=pr["other_u", cls])
        assert same_bits(ea["kkt"], eb["kkt"]) and same_bits([ea["fx"]], [eb["fx"]])
        assert ea["fx"] != 0.0
        # end, forming the next iterate from wk
        ea, eb = wa.end(lam, from_w=True), wb.end(lam, from_w=True)
        assert same_bits(ea["kkt"], eb["kkt"]) and same_bits([ea["fx"]], [eb["fx"]])
        same_state(wa, wb)
        # and the plan of that iterate, with MATLAB's sparse() rule
        same_plan(wa.plan(0.0, stats=True), wb.plan(0.0, stats=True))
    finally:
        wa.close()
        wb.close()


# ---------------------------------------------------------------------------
# cost_info, cost and its statistics
# ---------------------------------------------------------------------------
def test_cost_info_of_the_three_forms():
    m, n, d = 65, 17, 3
    pr = problem(m, n, d)
    wa, wb = pair("class1-scalar-gama", pr, "cityblock", True)
    wc = ipd().APDWorkspace(1, np.ones(m * n), pr["r"], pr["l1"], pr["p"], pr["q"])
    try:
        assert wa.cost_info() == dict(form=1, dim=d, metric=3, scale=1, device_bytes=8 * (m + n) * d)
        assert wb.cost_info() == dict(form=0, dim=d, metric=3, scale=1, device_bytes=8 * m * n)
        assert wc.cost_info() == dict(form=0, dim=0, metric=0, scale=0, device_bytes=8 * m * n)
    finally:
        for w in (wa, wb, wc):
            w.close()
    L = lib_mod()
    assert L.lib.ipd_apd_cost_info(None, None) == L.IPD_E_ARG


@pytest.mark.parametrize("m,n,d,metric,scale", CASES, ids=IDS)
def test_cost_and_statistics(m, n, d, metric, scale):
    pr = problem(m, n, d)
    wa, wb = pair("class1-scalar-gama", pr, metric, scale)
    try:
        info = wa.cost_info()
        assert info["form"] == 1 and info["device_bytes"] == 8 * (m + n) * d
        assert wb.cost_info()["form"] == 0 and wb.cost_info()["device_bytes"] == 8 * m * n
        want = cost_ref(pr["xs"], pr["ys"], metric, scale)
        ca, sa = wa.cost(stats=True)
        cb, sb = wb.cost(stats=True)
        assert ca.shape == (m, n) and same_bits(ca, want) and same_bits(cb, want)
        for k in ("min", "max", "sum"):
            assert same_bits([sa[k]], [sb[k]]), (k, sa[k], sb[k])
        assert sa["min"] == want.min() and sa["max"] == want.max()
        # the statistics alone (c == NULL), and a second read
        st = lib_mod().ipd_cost_stats()
        lib_mod().check(lib_mod().lib.ipd_apd_get_cost(wa.handle, None, ctypes.byref(st)))
        assert same_bits([st.min, st.max, st.sum], [sa["min"], sa["max"], sa["sum"]])
        assert same_bits(wa.cost(), want)
    finally:
        wa.close()
        wb.close()


# ---------------------------------------------------------------------------
# the passes, one at a time
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,d,metric,scale", CASES, ids=IDS)
def test_every_pass_equals_the_stored_workspace(m, n, d, metric, scale, monkeypatch):
    monkeypatch.delenv("IPD_APD_REPS", raising=False)
    for variant in VARIANTS:
        check_passes(variant, problem(m, n, d), metric, scale)


def test_passes_with_two_repetitions_and_a_partly_filled_last_group(monkeypatch):
    """65 x 70 under IPD_APD_REPS=2: five column chunks in groups of two, so the rep loop runs twice and the last
    group ends after one chunk of six columns."""
    monkeypatch.setenv("IPD_APD_REPS", "2")        # read when a workspace is created
    for variant in VARIANTS:
        check_passes(variant, problem(65, 70, 2), "sqeuclidean", False)
    check_passes(VARIANTS[0], problem(65, 70, 3), "euclidean", True)


# ---------------------------------------------------------------------------
# whole runs
# ---------------------------------------------------------------------------
def run_both(cls, wa, wb):
    P = ipd()
    wa.warmup(0.0, 20)
    wb.warmup(0.0, 20)
    same_state(wa, wb)
    amg = AMG1 if cls == 1 else AMG2
    ra = wa.run(amg, P.MatlabRand(), iters=10)
    rb = wb.run(amg, P.MatlabRand(), iters=10)
    assert ra["k"] == rb["k"] and ra["k"] >= 1
    ha, hb = wa.history(), wb.history()
    assert set(ha) == set(hb) and ha["fxk"].size == ra["k"] + 1
    for k in ha:
        assert same_bits(ha[k], hb[k]), k
    same_state(wa, wb)
    return wa.state(), ha


@pytest.mark.parametrize("cls,m,n", [(1, 48, 40), (2, 40, 30)])
def test_warm_start_and_run_equal_the_stored_workspace(cls, m, n):
    pr = problem(m, n, 2, seed=21 + cls)
    variant = "class1-scalar-gama" if cls == 1 else "class2-phi-none"
    wa, wb = pair(variant, pr, "sqeuclidean", True)
    try:
        run_both(cls, wa, wb)
    finally:
        wa.close()
        wb.close()


def test_two_matrix_free_creates_and_runs_give_the_same_bits():
    pr = problem(48, 40, 2, seed=22)
    wa = make("class1-scalar-gama", pr, "sqeuclidean", True, True)
    wb = make("class1-scalar-gama", pr, "sqeuclidean", True, True)
    try:
        sa, sb = wa.cost(stats=True)[1], wb.cost(stats=True)[1]
        assert [bits([sa[k]])[0] for k in ("min", "max", "sum")] == [bits([sb[k]])[0] for k in ("min", "max", "sum")]
        run_both(1, wa, wb)
    finally:
        wa.close()
        wb.close()


# ---------------------------------------------------------------------------
# script wrappers
# ---------------------------------------------------------------------------
def same_value(a, b, where):
    import scipy.sparse as sp
    if sp.issparse(a):
        assert sp.issparse(b) and a.shape == b.shape, where
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices), where
        assert same_bits(a.data, b.data), where
    elif isinstance(a, dict):
        assert set(a) == set(b), where
        for k in a:
            same_value(a[k], b[k], where + "." + str(k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same_value(x, y, "%s[%d]" % (where, i))
    elif isinstance(a, np.ndarray) and a.dtype.names:
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), where
    elif isinstance(a, (np.ndarray, float, np.floating)):
        assert same_bits(a, b), where
    else:
        assert a == b, where


def test_script_wrapper_gives_the_same_result_dictionary():
    pr = problem(48, 40, 2, seed=22)
    args = (pr["xs"], pr["ys"], pr["r"], pr["l1"], pr["p"], pr["q"])
    free = ipd().APD_SsN_Class1_points(*args, metric="sqeuclidean", scale=True, plan_tol=0.0, matrix_free=True)
    stored = ipd().APD_SsN_Class1_points(*args, metric="sqeuclidean", scale=True, plan_tol=0.0, matrix_free=False)
    assert set(free) == set(stored) and free["k"] >= 1 and free["plan"].shape == (48, 40)
    same_value(free, stored, "out")


def test_script_wrapper_class2_takes_the_keyword():
    pr = problem(40, 30, 2, seed=23)
    args = (pr["xs"], pr["ys"], pr["r"], pr["l"], pr["p"], pr["q"], pr["mu"])
    free = ipd().APD_SsN_Class2_points(*args, scale=True, maxit=3, plan_tol=0.0, matrix_free=True)
    stored = ipd().APD_SsN_Class2_points(*args, scale=True, maxit=3, plan_tol=0.0)
    same_value(free, stored, "out")


# ---------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------
def raw_spec(L, metric=1, dim=2, m=5, n=4, scale=0, xs=None, ys=None, null=()):
    keep = [np.ascontiguousarray(np.arange(1.0, m * max(dim, 1) + 1) if xs is None else xs, dtype=np.float64),
            np.ascontiguousarray(np.arange(2.0, n * max(dim, 1) + 2) if ys is None else ys, dtype=np.float64)]
    s = L.ipd_cost_spec()
    s.metric, s.dim, s.m, s.n, s.scale = metric, dim, m, n, scale
    if "xs" not in null:
        s.xs = L.dptr(keep[0])
    if "ys" not in null:
        s.ys = L.dptr(keep[1])
    return s, keep


def apd_data(L, cls, m, n, keep, c=None):
    r, l, p, q = np.full(n, float(m)), np.full(m, float(n)), np.ones(m), np.ones(n)
    keep += [r, l, p, q]
    d = L.ipd_apd_data()
    d.cls, d.m, d.n = cls, m, n
    d.r, d.l, d.p, d.q = L.dptr(r), L.dptr(l), L.dptr(p), L.dptr(q)
    d.gama_scalar = np.inf
    d.mu = 1.0
    if c is not None:
        keep.append(c)
        d.c = L.dptr(c)
    return d


def test_argument_errors_are_those_of_create_points_and_leave_out_alone():
    L = lib_mod()
    ctx = L.get_ctx().handle
    m, n = 5, 4
    keep = []
    UNTOUCHED = 0x5A5A5A5A

    def create(fn, d, s):
        out = ctypes.c_void_p(UNTOUCHED)
        rc = fn(ctx, ctypes.byref(d) if d is not None else None, ctypes.byref(s) if s is not None else None,
                ctypes.byref(out))
        if rc != 0:
            assert out.value == UNTOUCHED
        else:
            L.lib.ipd_apd_destroy(out)
        return rc

    def spec(**kw):                       # the arrays a specification points to live as long as `keep`
        s, arrays = raw_spec(L, **kw)
        keep.extend(arrays)
        return s

    free, stored = L.lib.ipd_apd_create_points_free, L.lib.ipd_apd_create_points
    good = spec()
    assert create(free, apd_data(L, 1, m, n, keep), good) == 0
    # the limit of its own: dim 1..3 pass, 4 and 16 are a limit (and pass the storing create)
    for dim, code in ((1, 0), (3, 0), (4, L.IPD_E_LIMIT), (16, L.IPD_E_LIMIT)):
        s = spec(dim=dim)
        assert create(free, apd_data(L, 1, m, n, keep), s) == code, dim
        assert create(stored, apd_data(L, 1, m, n, keep), s) == 0, dim
    s4 = spec(dim=4)
    out = ctypes.c_void_p(UNTOUCHED)
    assert free(ctx, ctypes.byref(apd_data(L, 1, m, n, keep)), ctypes.byref(s4), ctypes.byref(out)) == L.IPD_E_LIMIT
    assert b"[1, 3]" in L.lib.ipd_last_error() and out.value == UNTOUCHED
    # everything ipd_apd_create_points refuses, with its code
    nan, inf = np.full(10, 1.0), np.full(8, 1.0)
    nan[-1], inf[-1] = np.nan, np.inf
    refusals = [
        ("d NULL", None, good),
        ("s NULL", apd_data(L, 1, m, n, keep), None),
        ("xs NULL", apd_data(L, 1, m, n, keep), spec(null=("xs",))),
        ("ys NULL", apd_data(L, 1, m, n, keep), spec(null=("ys",))),
        ("metric 0", apd_data(L, 1, m, n, keep), spec(metric=0)),
        ("metric 5", apd_data(L, 1, m, n, keep), spec(metric=5)),
        ("dim 0", apd_data(L, 1, m, n, keep), spec(dim=0)),
        ("dim 17", apd_data(L, 1, m, n, keep), spec(dim=17)),
        ("scale 2", apd_data(L, 1, m, n, keep), spec(scale=2)),
        ("c given", apd_data(L, 1, m, n, keep, c=np.ones(m * n)), good),
        ("m differs", apd_data(L, 1, m + 1, n, keep), good),
        ("n differs", apd_data(L, 1, m, n - 1, keep), good),
        ("cls 3", apd_data(L, 3, m, n, keep), good),
    ]
    for name, xs, ys in (("xs NaN", nan, None), ("ys inf", None, inf)):
        s = spec(xs=xs, ys=ys)
        refusals.append((name, apd_data(L, 1, m, n, keep), s))
    for name, xs, ys in (("all points equal", np.ones(10), np.ones(8)),
                         ("largest entry inf", np.full(10, 1e200), np.full(8, -1e200))):
        s = spec(scale=1, xs=xs, ys=ys)
        refusals.append((name, apd_data(L, 1, m, n, keep), s))
    s = spec(n=0, ys=np.ones(2))
    refusals.append(("n 0", apd_data(L, 1, m, 0, keep), s))
    for name, d, s in refusals:
        want = create(stored, d, s)
        assert want != 0, name
        assert create(free, d, s) == want, name
    assert create(free, apd_data(L, 1, m, n, keep), spec(metric=0)) == L.IPD_E_ARG
    out = ctypes.c_void_p(UNTOUCHED)
    assert free(ctx, ctypes.byref(apd_data(L, 1, m, n, keep)), ctypes.byref(good), None) == L.IPD_E_ARG
    assert free(None, ctypes.byref(apd_data(L, 1, m, n, keep)), ctypes.byref(good), ctypes.byref(out)) == L.IPD_E_ARG
    assert out.value == UNTOUCHED
    with pytest.raises(ipd().IpdError):
        ipd().APDWorkspace.from_points(1, np.ones((m, 4)), np.zeros((n, 4)), np.ones(n), np.ones(m), np.ones(m),
                                       np.ones(n), matrix_free=True)
