"""The gradient of the transport cost in the point positions on the device (csrc/ipd_point_grad.hip:
ipd_apd_point_grad, ipd_apd_point_grad_dev; APDWorkspace.point_gradient, point_gradient_dev, transport_gradients; the
`gradient` keyword of the point-cloud drivers).

Reference: tests/point_grad_ref.py, the numpy restatement of csrc/ipd_point_grad_geo.h (tests/test_point_grad_geo.py
holds the header's scalar code to its bits, tests/test_point_grad_ref.py holds it to central differences).  One weight
and side 0 are compared bit for bit (a -0.0 counting as +0.0), side 1 and the mass within the any-order bar of DESIGN.md
section 4h, |G - ref| <= gamma(N + 4) * sum |x| |h_k| with the reference summed in longdouble from the float64 weights,
and exactly where every product and partial sum is exact.  States are injected with set_state as in
tests/test_gpu_plan_apply.py; only the last test runs the drivers."""
import ctypes

import numpy as np
import pytest

from tests import point_grad_ref as R

pytestmark = pytest.mark.gpu

NAMES = {1: "sqeuclidean", 2: "euclidean", 3: "cityblock", 4: "chebyshev"}
# tests/test_gpu_plan_apply.py's shapes: one lane, one column, 63 / 64 / 65 rows of a wave, the second row block, and
# 65 x 150: three column groups with a partly filled last one
SHAPES = [(1, 1), (1, 37), (37, 1), (63, 17), (64, 16), (65, 33), (257, 19), (600, 45), (65, 150)]
ALL_DIMS = [(65, 33), (257, 19), (65, 150)]
DIMS = [1, 2, 3, 4, 5, 16]    # registers (1, 2, 3); LDS: exactly one pass, one pass plus a tail, the limit


def dims_of(m, n):
    return DIMS if (m, n) in ALL_DIMS else [2, 5]


def ipd():
    import codes_of_ipd_ssn_amg_method_amd as pkg
    return pkg


def lib_mod():
    from codes_of_ipd_ssn_amg_method_amd import _lib
    return _lib


def data(cls, m, n, seed=1):
    rs = np.random.RandomState(seed)
    r, l = rs.random_sample(n) + 0.1, rs.random_sample(m) + 0.1
    l = l * r.sum() / l.sum()
    return dict(r=r, l=l, p=np.ones(m), q=np.ones(n), mu=0.65 * min(r.sum(), l.sum()))


def ws_host(cls, m, n, seed=1):
    """a workspace from a host matrix: it has no points of its own, every call gives them"""
    pr = data(cls, m, n, seed)
    c = np.random.RandomState(seed + 1).random_sample(m * n)
    if cls == 1:
        return ipd().APDWorkspace(1, c, pr["r"], pr["l"], pr["p"], pr["q"])
    return ipd().APDWorkspace(2, c, pr["r"], pr["l"], pr["p"], pr["q"], mu=pr["mu"], phi=np.ones(m * n))


def ws_points(cls, xs, ys, metric, scale, free=False, seed=1):
    m, n = len(xs), len(ys)
    pr = data(cls, m, n, seed)
    return ipd().APDWorkspace.from_points(cls, xs, ys, pr["r"], pr["l"], pr["p"], pr["q"], metric=NAMES[metric],
                                          scale=scale, mu=pr["mu"], matrix_free=free)


def inject(ws, Xd, rs):
    """state with the x block of u = Xd(:), everything else random (class 2: the y and z blocks too, so a leak shows)"""
    u = rs.standard_normal(ws.U)
    u[:ws.m * ws.n] = Xd.reshape(-1, order="F")
    ws.set_state(u, rs.standard_normal(ws.U), rs.standard_normal(ws.L), 0.37)


def clouds(m, n, d, seed):
    """tests/point_grad_ref.py's tie clouds (coincident points, zero differences, equal |t_k|, generic points in
    between) with a largest cost entry above 0, so that scale = 1 has a divider"""
    xs, ys = R.tie_points(m, n, d, seed)
    if not (xs[:, None, :] != ys[None, :, :]).any():
        ys[-1, 0] = xs[0, 0] + 0.75
    return xs, ys


def patterns(m, n, rs):
    val = lambda: 0.25 + rs.random_sample((m, n))
    sign = np.where(rs.random_sample((m, n)) < 0.3, -1.0, 1.0)
    out = {"dense": val() * sign, "bernoulli": val() * sign * (rs.random_sample((m, n)) < 0.05)}
    gaps = val()
    gaps[:, 1::3] = 0.0
    gaps[:, 2::3] = 0.0
    out["empty_columns"] = gaps
    last = np.zeros((m, n))
    last[m - 1, :] = val()[m - 1, :]
    last[:, n - 1] = val()[:, n - 1]
    out["last_row_and_column"] = last
    return out


def denom_of(xs, ys, metric, scale):
    return float(R.cost(xs, ys, metric).max()) if scale else None


def grad(ws, side, tol, xs, ys, metric, scale):
    return ws.point_gradient(side, tol, points=(xs, ys), metric=NAMES[metric], scale=scale, mass=True, stats=True)


@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", SHAPES)
def test_one_weight_bit_for_bit(cls, m, n):
    """A plan with one kept entry per row (side 0) or per column (side 1) at a random place: G is fl(x * h_k) of the
    restatement in every bit -- four metrics, scale on and off, every d, coordinates with exact ties."""
    ws = ws_host(cls, m, n)
    rs = np.random.RandomState(100 * m + n)
    for d in dims_of(m, n):
        xs, ys = clouds(m, n, d, 7 * d + m)
        plans = []
        for side in (0, 1):
            Xd = np.zeros((m, n))
            if side == 0:
                Xd[np.arange(m), rs.randint(0, n, m)] = rs.standard_normal(m)
            else:
                Xd[rs.randint(0, m, n), np.arange(n)] = rs.standard_normal(n)
            plans.append(Xd)
        for side in (0, 1):
            inject(ws, plans[side], rs)
            for metric in NAMES:
                for scale in (False, True):
                    den = denom_of(xs, ys, metric, scale)
                    H, kink = R.weights(xs, ys, metric, den)
                    P, K = R.terms(plans[side], H, side, 0.0)
                    want = P.sum(axis=0 if side else 1)      # one term per sum: exact
                    G, w, st = grad(ws, side, 0.0, xs, ys, metric, scale)
                    assert G.shape == want.shape == ((n if side else m), d)
                    assert R.bits_equal(G, want), (d, side, metric, scale)
                    assert R.bits_equal(w, plans[side].sum(axis=0 if side else 1))
                    assert st == dict(kept=int(K.sum()), kinks=int((K & kink).sum()), denom=den if scale else 1.0)
    ws.close()


@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", SHAPES)
def test_sums_side0_bits_side1_bar(cls, m, n):
    """Dense, Bernoulli (5 %), empty-columns and last-row-and-column plans at tol in {0, 0.375, 1e-9}: side 0 and its
    mass have the bits of the restatement's summation shape; side 1 and its mass lie within the any-order bar, exactly
    0 where the bar is 0; kept and kinks are the restatement's counts and the same on both sides."""
    ws = ws_host(cls, m, n)
    rs = np.random.RandomState(200 * m + n)
    pats = patterns(m, n, rs)
    worst = -np.inf
    for d in dims_of(m, n):
        xs, ys = clouds(m, n, d, 11 * d + n)
        for metric in NAMES:
            scale = (metric + d) % 2 == 1
            den = denom_of(xs, ys, metric, scale)
            H, kink = R.weights(xs, ys, metric, den)
            for name, Xd in pats.items():
                inject(ws, Xd, rs)
                for tol in (0.0, 0.375, 1e-9):
                    P, K = R.terms(Xd, H, 0, tol)
                    counts = dict(kept=int(K.sum()), kinks=int((K & kink).sum()), denom=den if scale else 1.0)
                    G0, w0, st0 = grad(ws, 0, tol, xs, ys, metric, scale)
                    assert R.bits_equal(G0, R.rows_sum(P)), (d, metric, name, tol)
                    assert R.bits_equal(w0, R.rows_sum(np.where(K, Xd, 0.0))), (d, metric, name, tol)
                    G1, w1, st1 = grad(ws, 1, tol, xs, ys, metric, scale)
                    ref, bar, wref, wbar, _, _ = R.reference(Xd, xs, ys, metric, 1, tol, den)
                    ok, over = R.within(G1, ref, bar)
                    okw, overw = R.within(w1, wref, wbar)
                    worst = max(worst, over, overw)
                    assert ok and okw, (d, metric, name, tol, over, overw)
                    assert st0 == counts and st1 == counts, (d, metric, name, tol, st0, st1, counts)
    print("side 1: largest err - bar over the cases: %.3e" % worst)
    ws.close()


@pytest.mark.parametrize("m,n", [(65, 33), (600, 45), (65, 150)])
def test_dyadic_inputs_are_exact(m, n):
    """Coordinates that are multiples of 2^-4 in [-4, 4], x multiples of 2^-10 in [0, 1], metrics 1, 3 and 4 without
    scale: every product and every partial sum is exact (at most 600 terms of magnitude <= 16 on a 2^-13 grid), so both
    sides equal numpy's sum in every bit, whatever the order."""
    ws = ws_host(1, m, n)
    rs = np.random.RandomState(300 * m + n)
    Xd = rs.randint(0, 1025, size=(m, n)) / 1024.0 * (rs.random_sample((m, n)) < 0.6)
    inject(ws, Xd, rs)
    for d in dims_of(m, n):
        xs = rs.randint(-64, 65, size=(m, d)) / 16.0
        ys = rs.randint(-64, 65, size=(n, d)) / 16.0
        for metric in (1, 3, 4):
            H, _ = R.weights(xs, ys, metric)
            for side in (0, 1):
                for tol in (0.0, 0.375):
                    P, K = R.terms(Xd, H, side, tol)
                    G, w, _ = grad(ws, side, tol, xs, ys, metric, False)
                    assert R.bits_equal(G, P.sum(axis=0 if side else 1)), (d, metric, side, tol)
                    assert R.bits_equal(w, np.where(K, Xd, 0.0).sum(axis=0 if side else 1))
    ws.close()


@pytest.mark.parametrize("metric", [1, 2, 3, 4])
def test_denom_is_the_cost_builds_divider(metric):
    m, n, d = 65, 33, 3
    xs, ys = clouds(m, n, d, 5)
    ws = ws_host(1, m, n)
    inject(ws, np.ones((m, n)), np.random.RandomState(1))
    _, st = ipd().point_cost(xs, ys, metric=NAMES[metric], scale=False, stats=True)
    for side in (0, 1):
        got = ws.point_gradient(side, points=(xs, ys), metric=NAMES[metric], scale=True, stats=True)[1]
        assert got["denom"] == st["max"] and got["kept"] == m * n
        assert ws.point_gradient(side, points=(xs, ys), metric=NAMES[metric], stats=True)[1]["denom"] == 1.0
    ws.close()


@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("d", [2, 3, 5])
def test_forms_and_entries_agree(cls, d):
    """The same bits from a stored and a matrix-free from_points workspace (d <= 3) with their own points, from a
    workspace made of a host matrix with points= given, from the host and the device entry (device arrays at offsets 0
    and +8 inside guarded buffers, sentinels intact) and from two calls in a row."""
    from tests import dev_abi as DA
    m, n = 257, 150
    rs = np.random.RandomState(40 + d)
    xs, ys = clouds(m, n, d, 3 * d)
    Xd = patterns(m, n, rs)["dense"] * (rs.random_sample((m, n)) < 0.4)
    for metric, scale in ((1, False), (2, True), (3, False), (4, True)):
        forms = [ws_points(cls, xs, ys, metric, scale)]
        if d <= 3:
            forms.append(ws_points(cls, xs, ys, metric, scale, free=True))
        host = ws_host(cls, m, n)
        before = [w.cost_info() for w in forms]
        for w in forms + [host]:
            inject(w, Xd, np.random.RandomState(9))
        for side in (0, 1):
            R_ = n if side else m
            for tol in (0.0, 0.5):
                want = grad(host, side, tol, xs, ys, metric, scale)
                again = grad(host, side, tol, xs, ys, metric, scale)
                assert all(R.bits_equal(a, b) for a, b in zip(want[:2], again[:2])) and want[2] == again[2]
                assert R.bits_equal(host.point_gradient(side, tol, points=(xs, ys), metric=NAMES[metric], scale=scale),
                                    want[0]), "mass=True changed G"
                for w in forms:
                    own = w.point_gradient(side, tol, mass=True, stats=True)
                    assert R.bits_equal(own[0], want[0]) and R.bits_equal(own[1], want[1]) and own[2] == want[2]
                for off in (0, 8):
                    Gd, wd = DA.DevArray.empty(R_ * d, off=off), DA.DevArray.empty(R_, off=off)
                    xd = DA.DevArray(np.ascontiguousarray(xs.T).reshape(-1), off=off)
                    yd = DA.DevArray(np.ascontiguousarray(ys.T).reshape(-1), off=off)
                    st = host.point_gradient_dev((Gd.ptr.value, R_ * d), (wd.ptr.value, R_), side=side, tol=tol,
                                                 xs=(xd.ptr.value, m * d), ys=(yd.ptr.value, n * d),
                                                 metric=NAMES[metric], scale=scale)
                    assert R.bits_equal(Gd.read().reshape((R_, d), order="F"), want[0]) and st == want[2]
                    assert R.bits_equal(wd.read(), want[1])
                    xd.assert_unchanged("xs")
                    yd.assert_unchanged("ys")
                    # the workspace's own points, no w
                    Ge = DA.DevArray.empty(R_ * d, off=off)
                    st = forms[0].point_gradient_dev((Ge.ptr.value, R_ * d), side=side, tol=tol)
                    assert R.bits_equal(Ge.read().reshape((R_, d), order="F"), want[0]) and st == want[2]
                    DA.free_all(Gd, wd, xd, yd, Ge)
        g = forms[0].transport_gradients(0.5)
        assert R.bits_equal(g["xs"], forms[0].point_gradient(0, 0.5)) and R.bits_equal(g["ys"], forms[0].point_gradient(1, 0.5))
        assert [w.cost_info() for w in forms] == before          # and 8*mn stored, 8*(m+n)*d matrix-free as before
        assert before[0]["device_bytes"] == 8 * m * n and before[0]["form"] == 0
        for w in forms + [host]:
            w.close()


@pytest.mark.parametrize("cls", [1, 2])
def test_sq_euclidean_against_apply_plan(cls):
    """Metric 1 without scale: G0 = 2 (w o xs - X ys) with apply_plan's product, within the sum of the two bars."""
    m, n, d = 257, 150, 3
    rs = np.random.RandomState(50)
    xs, ys = rs.standard_normal((m, d)), rs.standard_normal((n, d))
    Xd = patterns(m, n, rs)["dense"] * (rs.random_sample((m, n)) < 0.3)
    ws = ws_host(cls, m, n)
    inject(ws, Xd, rs)
    for tol in (0.0, 0.5):
        G, w, _ = grad(ws, 0, tol, xs, ys, 1, False)
        Y, wa = ws.apply_plan(ys, side=0, tol=tol, mass=True)
        assert R.bits_equal(w, wa)                            # the mass in 4j's bits
        Xt = np.where(R.kept(Xd, tol), Xd, 0.0)
        ld = np.longdouble
        other = 2 * (w.astype(ld)[:, None] * xs.astype(ld) - Y.astype(ld))
        _, bar, _, _, _, _ = R.reference(Xd, xs, ys, 1, 0, tol)
        bar2 = 2 * (R.gamma(n + 4) * (np.abs(Xt) @ np.abs(ys)) + (R.gamma(n + 4) + 2 * R.U) * np.abs(Xt).sum(axis=1)[:, None] * np.abs(xs))
        assert np.all(np.abs(G.astype(ld) - other) <= bar + bar2), tol
    ws.close()


def test_hygiene():
    """An inf or NaN coordinate is refused; an inf in a dropped entry of x never reaches G (|inf| <= tol holds for
    tol = inf only, which drops every entry but a NaN); a NaN x is kept and shows exactly in its row (side 0) or column
    (side 1)."""
    L = lib_mod()
    m, n, d = 65, 33, 3
    rs = np.random.RandomState(60)
    xs, ys = clouds(m, n, d, 6)
    ws = ws_host(1, m, n)
    Xd = patterns(m, n, rs)["dense"]
    inject(ws, Xd, rs)
    for bad in (np.inf, -np.inf, np.nan):
        for which in (0, 1):
            pts = [xs.copy(), ys.copy()]
            pts[which][3, 1] = bad
            with pytest.raises(L.IpdError) as ei:
                ws.point_gradient(0, points=tuple(pts))
            assert ei.value.code == L.IPD_E_ARG
    # tol = inf drops every finite entry and every inf; only a NaN stays
    Xn = Xd.copy()
    Xn[::7, ::5] = np.inf
    Xn[40, 20] = np.nan
    inject(ws, Xn, rs)
    for side in (0, 1):
        for metric in NAMES:
            G, w, st = grad(ws, side, np.inf, xs, ys, metric, False)
            hit = 20 if side else 40
            rest = np.arange(G.shape[0]) != hit
            assert not G[rest].any() and not w[rest].any() and st["kept"] == 1, (side, metric)
            assert np.isnan(w[hit]) and np.isnan(G[hit]).all()
    ws.close()


SENT = -1234.5


def test_argument_errors_write_nothing():
    L = lib_mod()
    lib = L.lib
    m, n, d = 37, 5, 3
    rs = np.random.RandomState(70)
    xs, ys = clouds(m, n, d, 8)
    own = ws_points(1, xs, ys, 2, True)
    host = ws_host(1, m, n)
    for w in (own, host):
        inject(w, patterns(m, n, rs)["dense"], rs)
    info = own.cost_info()
    X, Y = np.ascontiguousarray(xs.T).reshape(-1), np.ascontiguousarray(ys.T).reshape(-1)
    xd, yd = L.DeviceBuffer.from_array(X), L.DeviceBuffer.from_array(Y)
    E, EL, nan = L.IPD_E_ARG, L.IPD_E_LIMIT, float("nan")

    def spec(metric=2, dim=d, mm=m, nn=n, x=X, y=Y, scale=0):
        s = L.ipd_cost_spec()
        s.metric, s.dim, s.m, s.n, s.scale = metric, dim, mm, nn, scale
        s.xs = x.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if x is not None else None
        s.ys = y.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if y is not None else None
        return s
    same = np.zeros(m * d)        # all points equal: the largest entry is 0
    bad = X.copy()
    bad[5] = np.inf
    #          name, handle, spec, tol, side, G?, code
    host_cases = [("NULL h", None, spec(), 0.0, 0, True, E),
                  ("NULL G", own.handle, None, 0.0, 0, False, E),
                  ("side -1", own.handle, None, 0.0, -1, True, E),
                  ("side 2", own.handle, spec(), 0.0, 2, True, E),
                  ("tol -1", own.handle, None, -1.0, 0, True, E),
                  ("tol -tiny", own.handle, None, -1e-300, 1, True, E),
                  ("tol NaN", own.handle, spec(), nan, 0, True, E),
                  ("no points", host.handle, None, 0.0, 0, True, E),
                  ("metric 0", host.handle, spec(metric=0), 0.0, 0, True, E),
                  ("metric 5", own.handle, spec(metric=5), 0.0, 1, True, E),
                  ("dim 0", host.handle, spec(dim=0), 0.0, 0, True, E),
                  ("dim 17", host.handle, spec(dim=17), 0.0, 0, True, E),
                  ("scale 2", host.handle, spec(scale=2), 0.0, 0, True, E),
                  ("NULL xs", host.handle, spec(x=None), 0.0, 0, True, E),
                  ("NULL ys", host.handle, spec(y=None), 0.0, 0, True, E),
                  ("inf coordinate", host.handle, spec(x=bad), 0.0, 0, True, E),
                  ("m differs", host.handle, spec(mm=m - 1), 0.0, 0, True, E),
                  ("n differs", host.handle, spec(nn=n - 1), 0.0, 1, True, E),
                  ("m above the limit", host.handle, spec(mm=16385), 0.0, 0, True, EL),
                  ("largest entry 0", host.handle, spec(x=same, y=np.zeros(n * d), scale=1), 0.0, 0, True, E)]
    cnt = max(m, n) * d
    for name, hh, s, tol, side, hasG, code in host_cases:
        G, w, st = np.full(cnt, SENT), np.full(max(m, n), SENT), L.ipd_grad_stats(-7, -7, SENT)
        rc = lib.ipd_apd_point_grad(hh, ctypes.byref(s) if s is not None else None, ctypes.c_double(tol), side,
                                    G.ctypes.data if hasG else None, w.ctypes.data, ctypes.byref(st))
        assert rc == code, (name, rc)
        assert (G == SENT).all() and (w == SENT).all() and (st.kept, st.kinks, st.denom) == (-7, -7, SENT), name
    zx, zy = L.DeviceBuffer.from_array(np.zeros(m * d)), L.DeviceBuffer.from_array(np.zeros(n * d))
    bx, by = L.DeviceBuffer.from_array(np.full(m * d, 1e200)), L.DeviceBuffer.from_array(np.full(n * d, -1e200))
    #          name, handle, metric, dim, scale, xs? (or a buffer), ys?, tol, side, G?, code
    dev_cases = [("NULL h", None, 2, d, 0, True, True, 0.0, 0, True, E),
                 ("NULL G", own.handle, 2, d, 0, False, False, 0.0, 0, False, E),
                 ("side 2", own.handle, 2, d, 0, False, False, 0.0, 2, True, E),
                 ("tol NaN", own.handle, 2, d, 0, True, True, nan, 0, True, E),
                 ("tol -1", own.handle, 2, d, 0, False, False, -1.0, 1, True, E),
                 ("only xs", own.handle, 2, d, 0, True, False, 0.0, 0, True, E),
                 ("only ys", host.handle, 2, d, 0, False, True, 0.0, 0, True, E),
                 ("no points", host.handle, 2, d, 0, False, False, 0.0, 0, True, E),
                 ("metric 0", host.handle, 0, d, 0, True, True, 0.0, 0, True, E),
                 ("dim 0", host.handle, 2, 0, 0, True, True, 0.0, 0, True, E),
                 ("dim 17", host.handle, 2, 17, 0, True, True, 0.0, 0, True, E),
                 ("scale -1", host.handle, 2, d, -1, True, True, 0.0, 0, True, E),
                 # scale = 1 and a divider that is 0 (all points equal) or inf (the squares overflow): refused after
                 # the divider's pass, before anything of G is written
                 ("largest entry 0", host.handle, 2, d, 1, zx, zy, 0.0, 0, True, E),
                 ("largest entry 0, side 1", own.handle, 4, d, 1, zx, zy, 0.0, 1, True, E),
                 ("largest entry inf", host.handle, 1, d, 1, bx, by, 0.0, 0, True, E)]
    for name, hh, metric, dim, scale, hasx, hasy, tol, side, hasG, code in dev_cases:
        Gd, wd = L.DeviceBuffer.from_array(np.full(cnt, SENT)), L.DeviceBuffer.from_array(np.full(max(m, n), SENT))
        st = L.ipd_grad_stats(-7, -7, SENT)
        xp = hasx.ptr if isinstance(hasx, L.DeviceBuffer) else (xd.ptr if hasx else None)
        yp = hasy.ptr if isinstance(hasy, L.DeviceBuffer) else (yd.ptr if hasy else None)
        rc = lib.ipd_apd_point_grad_dev(hh, metric, dim, scale, xp, yp,
                                        ctypes.c_double(tol), side, Gd.ptr if hasG else None, wd.ptr, ctypes.byref(st))
        assert rc == code, (name + " (dev)", rc)
        assert (Gd.to_array(np.float64, cnt) == SENT).all() and (wd.to_array(np.float64, max(m, n)) == SENT).all(), name
        assert (st.kept, st.kinks, st.denom) == (-7, -7, SENT), name
        Gd.free()
        wd.free()
    # metric, dim and scale are ignored with the workspace's own points
    Gd = L.DeviceBuffer.from_array(np.full(m * d, SENT))
    assert lib.ipd_apd_point_grad_dev(own.handle, 99, -3, 7, None, None, ctypes.c_double(0.0), 0, Gd.ptr, None, None) == 0
    assert R.bits_equal(Gd.to_array(np.float64, m * d).reshape((m, d), order="F"), own.point_gradient(0))
    Gd.free()
    # the API reports them as IpdError or ValueError
    with pytest.raises(L.IpdError) as ei:
        own.point_gradient(0, tol=-1.0)
    assert ei.value.code == E
    with pytest.raises(ValueError):
        host.point_gradient(0)
    with pytest.raises(ValueError):
        own.point_gradient(2)
    with pytest.raises(ValueError):
        own.point_gradient(0, metric="euclidean")
    with pytest.raises(ValueError):
        host.point_gradient(0, points=(xs[:-1], ys))
    with pytest.raises(ValueError):
        host.point_gradient_dev((xd.ptr.value, m * d), xs=(xd.ptr.value, m * d))
    assert own.cost_info() == info
    for b in (xd, yd, zx, zy, bx, by):
        b.free()
    own.close()
    host.close()


def check_run(out, xs, ys, metric, scale, m, n):
    Xd = out["xk"].reshape((m, n), order="F")
    den = denom_of(xs, ys, metric, scale)
    G0, w0, kept, kinks = R.gradient_rows(Xd, xs, ys, metric, 0.0, den)
    assert R.bits_equal(out["grad_xs"], G0)
    ref, bar, _, _, _, _ = R.reference(Xd, xs, ys, metric, 1, 0.0, den)
    assert R.within(out["grad_ys"], ref, bar)[0]
    assert out["grad_stats"] == dict(kept=kept, kinks=kinks, denom=den if scale else 1.0)
    assert out["grad_xs"].shape == (m, 2) and out["grad_ys"].shape == (n, 2)


def test_drivers_take_the_keyword():
    """One run of each point-cloud driver at 40 x 28, d = 2 with gradient=0.0: grad_xs / grad_ys meet the checks above
    on the returned xk; without the keyword the result has the keys and bits it has today (a second run)."""
    m, n = 40, 28
    rs = np.random.RandomState(80)
    xs, ys = rs.random_sample((m, 2)), rs.random_sample((n, 2))
    pr = data(1, m, n, seed=81)
    a1 = (xs, ys, pr["r"], pr["l"], pr["p"], pr["q"])
    runs = {1: lambda **kw: ipd().APD_SsN_Class1_points(*a1, metric="euclidean", scale=True, maxit=2, **kw),
            2: lambda **kw: ipd().APD_SsN_Class2_points(*a1, pr["mu"], metric="sqeuclidean", maxit=1, **kw)}
    for cls, run in runs.items():
        with_grad, plain, again = run(gradient=0.0), run(), run()
        check_run(with_grad, xs, ys, 2 if cls == 1 else 1, cls == 1, m, n)
        assert set(with_grad) - set(plain) == {"grad_xs", "grad_ys", "grad_stats"} and set(plain) == set(again)
        for key in ("xk", "uk", "vk", "lk", "fxk", "KKT_xk", "KKT_lk"):
            assert R.bits_equal(plain[key], again[key]) and R.bits_equal(plain[key], with_grad[key]), key
        assert plain["bk"] == again["bk"] == with_grad["bk"] and plain["k"] == again["k"]
    # after gap_install the installed feasible plan is the one differentiated
    inst = runs[1](gradient=0.0, gap_rel=1e-9, gap_install=True)
    check_run(inst, xs, ys, 2, True, m, n)
