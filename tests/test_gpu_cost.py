"""The cost matrix built on the device from point clouds (ipd_cost_points_dev, ipd_apd_create_points,
ipd_apd_get_cost) against the numpy restatement of its definition.

The reference folds t_k = xs[:, k] - ys[:, k] in ascending k with separate operations, which numpy does not
contract, and the library is built with -ffp-contract=off: the bar for every entry is bit equality.  min and max
are exact too; the sum is a reduction in another order and is held to 1e-12 of sum|c|, the bar of
tests/test_gpu_plan.py for reductions.

Two workspaces built from the same host c reproduce each other bit for bit through run() (checked before these
tests were written, and asserted again in test_runs_from_one_host_c_reproduce), so a workspace made from points
is compared bitwise with one made from the reference matrix, through warm start and run."""
import ctypes
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

METRICS = {"sqeuclidean": 1, "euclidean": 2, "cityblock": 3, "chebyshev": 4}
SHAPES = [(1, 1), (1, 70), (70, 1), (63, 5), (64, 64), (65, 17), (127, 33), (129, 31), (200, 37), (257, 3)]
# every shape with d in {2, 5}; every d with two shapes (an odd and an even m, more than one workgroup of columns)
CASES = [(m, n, d) for (m, n) in SHAPES for d in (2, 5)] + \
        [(m, n, d) for d in (1, 3, 16) for (m, n) in ((65, 17), (200, 37))]
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
def points(m, n, d, seed=0):
    rs = np.random.RandomState(1000 * seed + 7 * m + 3 * n + d)
    xs, ys = rs.standard_normal((m, d)), rs.standard_normal((n, d))
    xs.setflags(write=False)
    ys.setflags(write=False)
    return xs, ys


@functools.lru_cache(maxsize=None)
def ref_of(m, n, d, metric, scale):
    c = cost_ref(*points(m, n, d), metric, scale)
    c.setflags(write=False)
    return c


class store_form:
    """IPD_COST_STORE for the calls inside (the library reads it at every call)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("IPD_COST_STORE")
        if self.value is None:
            os.environ.pop("IPD_COST_STORE", None)
        else:
            os.environ["IPD_COST_STORE"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("IPD_COST_STORE", None)
        else:
            os.environ["IPD_COST_STORE"] = self.old


def check_stats(st, c):
    assert st["min"] == c.min() and st["max"] == c.max()
    tot = np.abs(c).sum()
    print("sum - numpy's = %.3e (sum|c| %.3e)" % (st["sum"] - c.sum(), tot))
    assert abs(st["sum"] - c.sum()) <= 1e-12 * tot


# ---------------------------------------------------------------------------
# entry values and statistics
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,d", CASES)
def test_entries_are_bit_equal(m, n, d):
    xs, ys = points(m, n, d)
    # both store forms where the 16-byte one is possible (an even m, d in registers), the default otherwise
    forms = ("8", "16") if m % 2 == 0 and d <= 3 else (None,)
    for form in forms:
        with store_form(form):
            for metric in METRICS:
                for scale in (False, True):
                    want = ref_of(m, n, d, metric, scale)
                    got, st = ipd().point_cost(xs, ys, metric=metric, scale=scale, stats=True)
                    assert got.shape == (m, n)
                    bad = np.flatnonzero(bits(got) != bits(want))
                    assert bad.size == 0, (form, metric, scale, bad[:5], got.ravel()[bad[:5]], want.ravel()[bad[:5]])
                    check_stats(st, want)
                    if scale:
                        assert st["max"] == 1.0


def test_one_dimensional_points_may_be_vectors():
    xs, ys = points(65, 17, 1)
    got = ipd().point_cost(xs[:, 0], ys[:, 0], metric="cityblock")
    assert np.array_equal(bits(got), bits(ref_of(65, 17, 1, "cityblock", False)))


def test_duplicated_points_give_exact_zeros():
    xs, ys = (a.copy() for a in points(129, 31, 3))
    ys[4] = xs[70]
    ys[30] = xs[128]
    for metric in METRICS:
        for scale in (False, True):
            want = cost_ref(xs, ys, metric, scale)
            got, st = ipd().point_cost(xs, ys, metric=metric, scale=scale, stats=True)
            assert np.array_equal(bits(got), bits(want))
            assert got[70, 4] == 0.0 and got[128, 30] == 0.0 and not np.signbit(got[70, 4])
            assert st["min"] == 0.0


def test_city_block_of_huge_coordinates_does_not_overflow():
    rs = np.random.RandomState(5)
    xs, ys = 1e150 * rs.standard_normal((70, 5)), 1e150 * rs.standard_normal((33, 5))
    for scale in (False, True):
        want = cost_ref(xs, ys, "cityblock", scale)
        got, st = ipd().point_cost(xs, ys, metric="cityblock", scale=scale, stats=True)
        assert np.all(np.isfinite(got)) and np.array_equal(bits(got), bits(want))
        check_stats(st, want)


def test_two_calls_give_the_same_bits():
    xs, ys = points(600, 45, 2, seed=1)
    for metric, scale in (("euclidean", True), ("sqeuclidean", False)):
        a, sa = ipd().point_cost(xs, ys, metric=metric, scale=scale, stats=True)
        b, sb = ipd().point_cost(xs, ys, metric=metric, scale=scale, stats=True)
        assert np.array_equal(bits(a), bits(b))
        assert [bits([sa[k]])[0] for k in ("min", "max", "sum")] == [bits([sb[k]])[0] for k in ("min", "max", "sum")]
        check_stats(sa, cost_ref(xs, ys, metric, scale))


def test_an_array_that_is_not_16_byte_aligned_takes_8_byte_stores():
    L = lib_mod()
    m, n, d = 64, 64, 2
    xs, ys = points(m, n, d)
    spec, keep = ipd().api._cost_spec(xs, ys, "sqeuclidean", False)
    buf = L.DeviceBuffer(8 * (m * n + 2))
    L.check(L.lib.ipd_h2d(buf.ctx.handle, buf.ptr, np.full(m * n + 2, -7.0).ctypes.data_as(ctypes.c_void_p),
                          ctypes.c_size_t(8 * (m * n + 2))))
    with store_form("16"):
        L.check(L.lib.ipd_cost_points_dev(L.get_ctx().handle, ctypes.byref(spec), ctypes.c_void_p(buf.ptr.value + 8),
                                          None))
    out = buf.to_array(np.float64, m * n + 2)
    buf.free()
    assert out[0] == -7.0 and out[-1] == -7.0          # nothing outside the mn entries
    assert np.array_equal(bits(out[1:-1].reshape(n, m).T), bits(ref_of(m, n, d, "sqeuclidean", False)))


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


def bad_specs(L):
    """(name, spec, code) of every refusal of the cost specification itself."""
    nan, inf = np.full(10, 1.0), np.full(8, 1.0)
    nan[-1], inf[-1] = np.nan, np.inf
    S = 16384
    return [
        ("xs NULL", raw_spec(L, null=("xs",)), L.IPD_E_ARG),
        ("ys NULL", raw_spec(L, null=("ys",)), L.IPD_E_ARG),
        ("metric 0", raw_spec(L, metric=0), L.IPD_E_ARG),
        ("metric 5", raw_spec(L, metric=5), L.IPD_E_ARG),
        ("dim 0", raw_spec(L, dim=0), L.IPD_E_ARG),
        ("dim 17", raw_spec(L, dim=17), L.IPD_E_ARG),
        ("xs NaN", raw_spec(L, xs=nan), L.IPD_E_ARG),
        ("ys inf", raw_spec(L, ys=inf), L.IPD_E_ARG),
        ("scale 2", raw_spec(L, scale=2), L.IPD_E_ARG),
        ("largest entry 0", raw_spec(L, scale=1, xs=np.ones(10), ys=np.ones(8)), L.IPD_E_ARG),
        ("largest entry inf", raw_spec(L, scale=1, xs=np.full(10, 1e200), ys=np.full(8, -1e200)), L.IPD_E_ARG),
        ("m over the limit", raw_spec(L, m=S + 1, dim=1, xs=np.ones(S + 1)), L.IPD_E_LIMIT),
        ("n 0", raw_spec(L, n=0, ys=np.ones(2)), L.IPD_E_LIMIT),
    ]


def test_cost_argument_errors():
    L = lib_mod()
    ctx = L.get_ctx().handle
    buf = L.DeviceBuffer(8 * 5 * 4)
    good, keep = raw_spec(L)
    assert L.lib.ipd_cost_points_dev(ctx, ctypes.byref(good), buf.ptr, None) == 0
    assert L.lib.ipd_cost_points_dev(None, ctypes.byref(good), buf.ptr, None) == L.IPD_E_ARG
    assert L.lib.ipd_cost_points_dev(ctx, None, buf.ptr, None) == L.IPD_E_ARG
    assert L.lib.ipd_cost_points_dev(ctx, ctypes.byref(good), None, None) == L.IPD_E_ARG
    for name, (s, keep), code in bad_specs(L):
        big = L.DeviceBuffer(8 * 16385) if s.m > 5 else None
        assert L.lib.ipd_cost_points_dev(ctx, ctypes.byref(s), (big or buf).ptr, None) == code, name
        if big:
            big.free()
    # the limits themselves pass
    s, keep = raw_spec(L, dim=16, metric=4, scale=1)
    assert L.lib.ipd_cost_points_dev(ctx, ctypes.byref(s), buf.ptr, None) == 0
    buf.free()
    with pytest.raises(ValueError):
        ipd().point_cost(np.ones((3, 2)), np.ones((4, 2)), metric="minkowski")
    with pytest.raises(ValueError):
        ipd().point_cost(np.ones((3, 2)), np.ones((4, 3)))


def apd_data(L, cls, m, n, keep, c=None, phi=None):
    r, l, p, q = np.full(n, float(m)), np.full(m, float(n)), np.ones(m), np.ones(n)
    keep += [r, l, p, q]
    d = L.ipd_apd_data()
    d.cls, d.m, d.n = cls, m, n
    d.r, d.l, d.p, d.q = L.dptr(r), L.dptr(l), L.dptr(p), L.dptr(q)
    d.gama_scalar = np.inf
    d.mu = 1.0
    for name, a in (("c", c), ("phi", phi)):
        if a is not None:
            keep.append(a)
            setattr(d, name, L.dptr(a))
    return d


def test_create_points_argument_errors_leave_out_alone():
    L = lib_mod()
    ctx = L.get_ctx().handle
    m, n = 5, 4
    keep = []
    UNTOUCHED = 0x5A5A5A5A
    def create(d, s):
        out = ctypes.c_void_p(UNTOUCHED)
        rc = L.lib.ipd_apd_create_points(ctx, ctypes.byref(d) if d is not None else None,
                                         ctypes.byref(s) if s is not None else None, ctypes.byref(out))
        if rc != 0:
            assert out.value == UNTOUCHED
        return rc, out
    good, k0 = raw_spec(L)
    rc, out = create(apd_data(L, 1, m, n, keep), good)
    assert rc == 0 and out.value != UNTOUCHED
    L.lib.ipd_apd_destroy(out)
    assert create(None, good)[0] == L.IPD_E_ARG and create(apd_data(L, 1, m, n, keep), None)[0] == L.IPD_E_ARG
    assert L.lib.ipd_apd_create_points(ctx, ctypes.byref(apd_data(L, 1, m, n, keep)), ctypes.byref(good), None) == \
        L.IPD_E_ARG
    # c given although the points make it; sizes that disagree
    assert create(apd_data(L, 1, m, n, keep, c=np.ones(m * n)), good)[0] == L.IPD_E_ARG
    assert create(apd_data(L, 1, m + 1, n, keep), good)[0] == L.IPD_E_ARG
    assert create(apd_data(L, 1, m, n - 1, keep), good)[0] == L.IPD_E_ARG
    # every refusal of the specification
    for name, (s, k1), code in bad_specs(L):
        assert create(apd_data(L, 1, int(s.m), int(s.n), keep), s)[0] == code, name
    # everything else as ipd_apd_create
    assert create(apd_data(L, 3, m, n, keep), good)[0] == L.IPD_E_ARG
    d = apd_data(L, 1, m, n, keep)
    d.r = None
    assert create(d, good)[0] == L.IPD_E_ARG
    # ... whose own refusal of a NULL c or phi stands
    out = ctypes.c_void_p(UNTOUCHED)
    assert L.lib.ipd_apd_create(ctx, ctypes.byref(apd_data(L, 1, m, n, keep)), ctypes.byref(out)) == L.IPD_E_ARG
    assert L.lib.ipd_apd_create(ctx, ctypes.byref(apd_data(L, 2, m, n, keep, c=np.ones(m * n))),
                                ctypes.byref(out)) == L.IPD_E_ARG
    assert out.value == UNTOUCHED
    assert L.lib.ipd_apd_get_cost(None, None, None) == L.IPD_E_ARG
    with pytest.raises(ValueError):
        ipd().APDWorkspace.from_points(1, np.ones((m + 1, 2)), np.ones((n, 2)), np.ones(n), np.ones(m), np.ones(m),
                                       np.ones(n))


# ---------------------------------------------------------------------------
# workspaces
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ot_problem(cls, m, n, seed):
    """Points in the plane, p and q random in [0.5, 1.5], r and l as tests/test_gpu_plan.py::problem makes them."""
    rs = np.random.RandomState(seed)
    xs, ys = rs.standard_normal((m, 2)), rs.standard_normal((n, 2))
    r, l = rs.random_sample(n), rs.random_sample(m)
    p, q = 0.5 + rs.random_sample(m), 0.5 + rs.random_sample(n)
    pr = dict(xs=xs, ys=ys, r=r, l=l, p=p, q=q, c_ref=cost_ref(xs, ys, "sqeuclidean", True))
    if cls == 1:
        pr["l"] = l * (r @ q) / (l @ p)      # <r,q> = <l,p>
    else:
        pr["mu"] = 0.65 * min(r.sum(), l.sum())
    return pr


def pair_of(cls, pr):
    """(a workspace from the points, one from the reference matrix)"""
    P = ipd()
    common = (pr["r"], pr["l"], pr["p"], pr["q"])
    if cls == 1:
        return (P.APDWorkspace.from_points(1, pr["xs"], pr["ys"], *common, metric="sqeuclidean", scale=True),
                P.APDWorkspace(1, pr["c_ref"].reshape(-1, order="F"), *common, gama=np.inf))
    mn = pr["p"].size * pr["q"].size
    return (P.APDWorkspace.from_points(2, pr["xs"], pr["ys"], *common, metric="sqeuclidean", scale=True,
                                       mu=pr["mu"], phi=None),
            P.APDWorkspace(2, pr["c_ref"].reshape(-1, order="F"), *common, mu=pr["mu"], phi=np.ones(mn)))


def run_both(cls, wa, wb):
    """Warm start and ten iterations on both; everything they leave is compared bit for bit."""
    P = ipd()
    wa.warmup(0.0, 20)
    wb.warmup(0.0, 20)
    sa, sb = wa.state(), wb.state()
    for a, b in zip(sa[:3], sb[:3]):
        assert np.array_equal(bits(a), bits(b))
    assert sa[3] == sb[3]
    amg = AMG1 if cls == 1 else AMG2
    ra = wa.run(amg, P.MatlabRand(), iters=10)
    rb = wb.run(amg, P.MatlabRand(), iters=10)
    assert ra["k"] == rb["k"]
    ha, hb = wa.history(), wb.history()
    assert ha["fxk"].size == ra["k"] + 1
    assert np.array_equal(bits(ha["fxk"]), bits(hb["fxk"]))


def test_runs_from_one_host_c_reproduce():
    """The premise of the bitwise comparisons below: two workspaces from the same host c, one process."""
    pr = ot_problem(1, 48, 40, 21)
    common = (pr["r"], pr["l"], pr["p"], pr["q"])
    c = pr["c_ref"].reshape(-1, order="F")
    wa, wb = ipd().APDWorkspace(1, c, *common), ipd().APDWorkspace(1, c, *common)
    run_both(1, wa, wb)
    wa.close()
    wb.close()


@pytest.mark.parametrize("cls,m,n", [(1, 48, 40), (2, 40, 30)])
def test_workspace_from_points_equals_workspace_from_the_matrix(cls, m, n):
    pr = ot_problem(cls, m, n, 21 + cls)
    wa, wb = pair_of(cls, pr)
    ca, st = wa.cost(stats=True)
    assert ca.shape == (m, n) and np.array_equal(bits(ca), bits(pr["c_ref"]))
    assert np.array_equal(bits(wb.cost()), bits(pr["c_ref"]))
    check_stats(st, pr["c_ref"])
    run_both(cls, wa, wb)
    wa.close()
    wb.close()


def test_class2_phi_is_kept_when_given():
    """phi given with points: the workspace equals the one from the matrix and the same phi."""
    pr = ot_problem(2, 40, 30, 23)
    rs = np.random.RandomState(3)
    phi = 0.5 + rs.random_sample(40 * 30)
    common = (pr["r"], pr["l"], pr["p"], pr["q"])
    wa = ipd().APDWorkspace.from_points(2, pr["xs"], pr["ys"], *common, scale=True, mu=pr["mu"], phi=phi)
    wb = ipd().APDWorkspace(2, pr["c_ref"].reshape(-1, order="F"), *common, mu=pr["mu"], phi=phi)
    ua, la = wa.warmup(0.0, 20)
    ub, lb = wb.warmup(0.0, 20)
    assert np.array_equal(bits(ua), bits(ub)) and np.array_equal(bits(la), bits(lb))
    wa.close()
    wb.close()


def test_script_wrapper():
    pr = ot_problem(1, 48, 40, 21)
    common = (pr["r"], pr["l"], pr["p"], pr["q"])
    out = ipd().APD_SsN_Class1_points(pr["xs"], pr["ys"], *common, metric="sqeuclidean", scale=True, plan_tol=0.0)
    ref = ipd().APD_SsN_Class1(pr["c_ref"].reshape(-1, order="F"), *common, plan_tol=0.0)
    assert set(out) == set(ref)
    assert out["k"] == ref["k"] and out["converged"] == ref["converged"]
    X, R = out["plan"], ref["plan"]
    assert X.shape == (48, 40)
    assert np.array_equal(X.indptr, R.indptr) and np.array_equal(X.indices, R.indices)
    assert np.array_equal(bits(X.data), bits(R.data))


def test_script_wrapper_class2_keys():
    pr = ot_problem(2, 40, 30, 23)
    common = (pr["r"], pr["l"], pr["p"], pr["q"])
    out = ipd().APD_SsN_Class2_points(pr["xs"], pr["ys"], *common, pr["mu"], scale=True, maxit=3, plan_tol=0.0)
    ref = ipd().APD_SsN_Class2(pr["c_ref"].reshape(-1, order="F"), *common, pr["mu"], np.ones(40 * 30), maxit=3,
                               plan_tol=0.0)
    assert set(out) == set(ref) and out["k"] == ref["k"]
    assert np.array_equal(bits(out["fxk"]), bits(ref["fxk"]))


@pytest.mark.parametrize("m,n", [(129, 31), (600, 45)])
def test_get_cost_on_a_workspace_from_a_host_matrix(m, n):
    rs = np.random.RandomState(11)
    c = rs.standard_normal(m * n)                       # any matrix, negative entries too
    ws = ipd().APDWorkspace(1, c, np.ones(n), np.ones(m), np.ones(m), np.ones(n))
    got, st = ws.cost(stats=True)
    assert np.array_equal(bits(got), bits(c.reshape(n, m).T))
    check_stats(st, c)
    again, st2 = ws.cost(stats=True)
    assert st == st2 and np.array_equal(bits(again), bits(got))
    assert np.array_equal(bits(ws.cost()), bits(got))
    ws.close()
