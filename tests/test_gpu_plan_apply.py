"""The transport plan applied on the device (csrc/ipd_plan_apply.hip: ipd_apd_plan_apply, ipd_apd_plan_apply_dev;
APDWorkspace.apply_plan, apply_plan_dev, barycentric_map).

Reference: Xd = u[:mn].reshape((m, n), order="F"), K = ~(abs(Xd) <= tol), Xt = where(K, Xd, 0) and
ref = Xt.astype(longdouble) @ B.astype(longdouble) (side 1: Xt.T).  Bar: the any-order summation bound of DESIGN.md
section 4h, entrywise |Y - ref| <= gamma(N + 4) * (|Xt| @ |B|) with gamma(s) = s*u / (1 - s*u), u = 2^-53 and N the
summed dimension; the same for the mass w against |Xt| summed.  Where the bar is 0 (nothing kept) the result is
exactly 0.  States are injected with set_state; only the last test runs the drivers."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
KS = [1, 3, 4, 5, 16]     # single, a partial pass, exactly one pass, one pass plus a tail, the limit


def ipd():
    import codes_of_ipd_ssn_amg_method_amd as pkg
    return pkg


def lib_mod():
    from codes_of_ipd_ssn_amg_method_amd import _lib
    return _lib


def gamma(s):
    return s * U / (1.0 - s * U)


def problem(cls, m, n, seed=1, pq_random=False):
    """tests/test_gpu_plan.py's synthetic inputs, re-stated: c,r,l ~ U(0,1) (draw order c,r,l), p=q=1, phi=1
    unless pq_random."""
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
    return ipd().APDWorkspace(2, pr["c"], pr["r"], pr["l"], pr["p"], pr["q"], mu=pr["mu"], phi=pr["phi"])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    """bit for bit, a NaN matching any NaN (the payload of 0/0 is the divider's own)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def inject(ws, Xd, rs):
    """state with the x block of u = Xd(:), everything else random (class 2: the y and z blocks too, so a leak
    shows); returns (u, v, lam)."""
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


def reference(Xt, B, side):
    """(ref, bar, wref, wbar) for the thresholded dense plan Xt (no NaNs) and B with all its columns"""
    A = Xt.T if side else Xt
    N = A.shape[1]
    ref = A.astype(np.longdouble) @ B.astype(np.longdouble)
    bar = gamma(N + 4) * (np.abs(A) @ np.abs(B))
    wref = A.astype(np.longdouble).sum(axis=1)
    wbar = gamma(N + 4) * np.abs(A).sum(axis=1)
    return ref, bar, wref, wbar


def within(Y, ref, bar):
    err = np.abs(Y.astype(np.longdouble) - ref)
    return bool(np.all(err <= bar)), float(np.max(err - bar)) if err.size else 0.0


def check_apply(ws, Xd, tol, Bfull, side, ks=KS, what=""):
    K = ~(np.abs(Xd) <= tol)
    Xt = np.where(K, Xd, 0.0)
    ref, bar, wref, wbar = reference(Xt, Bfull, side)
    worst = -np.inf
    for k in ks:
        Y, w = ws.apply_plan(Bfull[:, :k], side=side, tol=tol, mass=True)
        assert Y.shape == (ref.shape[0], k) and w.shape == (ref.shape[0],)
        ok, over = within(Y, ref[:, :k], bar[:, :k])
        okw, overw = within(w, wref, wbar)
        worst = max(worst, over, overw)
        assert ok, "%s side %d k %d tol %g: Y misses the bar by %.3e" % (what, side, k, tol, over)
        assert okw, "%s side %d k %d tol %g: w misses the bar by %.3e" % (what, side, k, tol, overw)
    return worst


# tests/test_gpu_plan.py's shapes (degenerate dimensions, the wave, chunk and workgroup boundaries) and 65 x 150:
# three column groups of 4, 4 and 2 chunks, the last chunk with 6 columns (tests/test_plan_apply_geo.py pins it)
SHAPES = [(1, 1), (1, 37), (37, 1), (63, 17), (64, 16), (65, 33), (257, 19), (600, 45), (65, 150)]


@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", SHAPES)
def test_products(cls, m, n):
    pr = problem(cls, m, n, seed=3, pq_random=True)
    ws = ws_of(cls, pr)
    rs = np.random.RandomState(100 * m + n)
    B = {0: rs.standard_normal((n, 16)), 1: rs.standard_normal((m, 16))}
    worst = -np.inf
    for name, Xd in patterns(m, n, rs).items():
        inject(ws, Xd, rs)
        for tol in (0.0, 0.5):
            for side in (0, 1):
                worst = max(worst, check_apply(ws, Xd, tol, B[side], side, what=name))
        if name == "zero":
            Y, w = ws.apply_plan(B[0], mass=True)
            assert not Y.any() and not w.any() and not np.signbit(Y).any()
    print("largest err - bar over the cases: %.3e" % worst)
    # a 1-D B is one column
    Y1 = ws.apply_plan(B[0][:, 0])
    assert Y1.shape == (m, 1) and same_bits(Y1, ws.apply_plan(B[0][:, :1]))
    ws.close()


@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("tol", [0.0, 0.375, 1e-9])
def test_threshold_edge(cls, tol):
    """Kept means exactly !(|x| <= tol): tol itself goes, its successor stays, a NaN stays -- and shows exactly in
    the rows (side 0) or columns (side 1) that hold it."""
    m, n = 65, 33
    pr = problem(cls, m, n, seed=4, pq_random=True)
    ws = ws_of(cls, pr)
    rs = np.random.RandomState(5)
    up = np.nextafter(tol, np.inf)
    vals = np.array([0.0, -0.0, tol, up, -tol, -up])
    Xd = vals[rs.randint(0, vals.size, size=(m, n))]
    Xd[40, 20] = np.nan
    inject(ws, Xd, rs)
    K = np.isnan(Xd) | (np.abs(Xd) == up)            # built by hand
    assert np.array_equal(K, ~(np.abs(Xd) <= tol)) and K[40, 20]
    Xt = np.where(K & ~np.isnan(Xd), Xd, 0.0)          # the NaN apart
    for side in (0, 1):
        B = rs.standard_normal((m if side else n, 16))
        if tol == 0.0:
            # the successor of 0 is the smallest subnormal: a product with it is rounded to a multiple of 2^-1074, an
            # absolute error the bar's relative model (no underflow) does not cover.  Small integers in B keep every
            # product and sum exact there, and the bar as it is.
            B = rs.randint(-4, 5, size=B.shape).astype(np.float64)
        ref, bar, wref, wbar = reference(Xt, B, side)
        hit = 20 if side else 40
        clean = np.arange(ref.shape[0]) != hit
        for k in KS:
            Y, w = ws.apply_plan(B[:, :k], side=side, tol=tol, mass=True)
            assert np.isnan(Y[hit]).all() and np.isnan(w[hit])
            assert not np.isnan(Y[clean]).any() and not np.isnan(w[clean]).any()
            ok, over = within(Y[clean], ref[clean, :k], bar[clean, :k])
            assert ok, (side, k, over)
            okw, overw = within(w[clean], wref[clean], wbar[clean])
            assert okw, (side, k, overw)
    ws.close()


@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", [(65, 33), (257, 19), (65, 150)])
def test_dropped_entries_are_inert(cls, m, n):
    """inf and NaN in the rows of B that meet only dropped or zero entries: Y is finite and within the bar of the
    reference with those rows of B zeroed."""
    pr = problem(cls, m, n, seed=5, pq_random=True)
    ws = ws_of(cls, pr)
    rs = np.random.RandomState(17 * m + n)
    tol = 0.5
    Xd = patterns(m, n, rs)["dense"]
    dead_cols = np.arange(n) % 3 == 1 if n > 1 else np.zeros(n, bool)
    dead_rows = np.arange(m) % 5 == 2
    dead_cols[n - 1] = True
    dead_rows[m - 1] = True
    # dead: zeros, signed zeros and entries at or below tol, alternating
    filler = np.array([0.0, -0.0, 0.3, -0.5, 0.5])[rs.randint(0, 5, size=(m, n))]
    Xd = np.where(dead_cols[None, :] | dead_rows[:, None], filler, Xd)
    inject(ws, Xd, rs)
    K = ~(np.abs(Xd) <= tol)
    assert not K[:, dead_cols].any() and not K[dead_rows, :].any() and K.any()
    Xt = np.where(K, Xd, 0.0)
    poison = np.array([np.inf, -np.inf, np.nan])
    for side in (0, 1):
        dead = dead_rows if side else dead_cols
        B = rs.standard_normal((dead.size, 16))
        Bz = B.copy()
        Bz[dead] = 0.0
        B[dead] = poison[rs.randint(0, 3, size=(int(dead.sum()), 16))]
        ref, bar, wref, wbar = reference(Xt, Bz, side)
        for k in KS:
            Y, w = ws.apply_plan(B[:, :k], side=side, tol=tol, mass=True)
            assert np.isfinite(Y).all() and np.isfinite(w).all(), (side, k)
            ok, over = within(Y, ref[:, :k], bar[:, :k])
            assert ok, (side, k, over)
            assert within(w, wref, wbar)[0]
            Yn = ws.apply_plan(B[:, :k], side=side, tol=tol, normalize=True)
            assert not np.isinf(Yn).any()
    ws.close()


@pytest.mark.parametrize("cls", [1, 2])
def test_normalize(cls):
    """normalize = 1 is one IEEE division by the mass: the bits of Y / w[:, None]; a row without kept mass is NaN."""
    m, n = 257, 150
    pr = problem(cls, m, n, seed=6, pq_random=True)
    ws = ws_of(cls, pr)
    rs = np.random.RandomState(21)
    Xd = patterns(m, n, rs)["dense"] * (rs.random_sample((m, n)) < 0.3)
    Xd[m - 1, :] = 0.2        # dropped at tol = 0.5
    Xd[:, 11] = 0.0
    Xd[:, n - 1] = -0.2
    Xd[7, :] = 0.0            # row 7 and column 11: no mass at any tol; the last row and column: none at 0.5
    inject(ws, Xd, rs)
    for side in (0, 1):
        B = rs.standard_normal((m if side else n, 16))
        for tol in (0.0, 0.5):
            for k in KS:
                Y, w = ws.apply_plan(B[:, :k], side=side, tol=tol, mass=True)
                Yn, wn = ws.apply_plan(B[:, :k], side=side, tol=tol, normalize=True, mass=True)
                with np.errstate(invalid="ignore", divide="ignore"):
                    want = Y / w[:, None]
                assert same_bits(Yn, want), (side, tol, k)
                assert same_bits(wn, w)
                # without w the mass is still computed
                assert same_bits(ws.apply_plan(B[:, :k], side=side, tol=tol, normalize=True), Yn)
                zero = w == 0.0
                assert zero[11 if side else 7] and (tol == 0.0 or zero[-1])
                assert np.isnan(Yn[zero]).all() and not np.isnan(Yn[~zero]).any()
    ws.close()


class Tensor:
    """anything with torch's tensor interface is taken as it is (a stand-in over library memory: the suite keeps a
    second HIP runtime out of this process)"""

    def __init__(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        self.buf, self.count = lib_mod().DeviceBuffer.from_array(a), a.size

    def data_ptr(self):
        return self.buf.ptr.value

    def element_size(self):
        return 8

    def is_contiguous(self):
        return True

    def numel(self):
        return self.count

    def numpy(self):
        return self.buf.to_array(np.float64, self.count)


SENT = -1234.5


@pytest.mark.parametrize("cls", [1, 2])
def test_calls_agree(cls):
    """Two calls, the host and the device entry, with and without the mass: the same bits."""
    L = lib_mod()
    m, n = 600, 150
    pr = problem(cls, m, n, seed=7, pq_random=True)
    ws = ws_of(cls, pr)
    rs = np.random.RandomState(9)
    Xd = patterns(m, n, rs)["dense"] * (rs.random_sample((m, n)) < 0.4)
    inject(ws, Xd, rs)
    for side in (0, 1):
        rin, rout = (m, n) if side else (n, m)
        for k in (3, 5, 16):
            B = rs.standard_normal((rin, k))
            for tol, norm in ((0.0, False), (0.6, False), (0.6, True)):
                Y1, w1 = ws.apply_plan(B, side=side, tol=tol, normalize=norm, mass=True)
                Y2, w2 = ws.apply_plan(B, side=side, tol=tol, normalize=norm, mass=True)
                assert same_bits(Y1, Y2) and same_bits(w1, w2)
                assert same_bits(ws.apply_plan(B, side=side, tol=tol, normalize=norm), Y1), "mass=True changed Y"
                Bd = L.DeviceBuffer.from_array(np.asfortranarray(B).reshape(-1, order="F"))
                Yd = L.DeviceBuffer.from_array(np.full(rout * k, SENT))
                wd = L.DeviceBuffer.from_array(np.full(rout, SENT))
                ws.apply_plan_dev(Bd, Yd, wd, side=side, tol=tol, normalize=norm)
                assert same_bits(Yd.to_array(np.float64, rout * k).reshape((rout, k), order="F"), Y1)
                assert same_bits(wd.to_array(np.float64, rout), w1)
                # (pointer, entries) pairs and no w
                Ye = L.DeviceBuffer.from_array(np.full(rout * k, SENT))
                ws.apply_plan_dev((Bd.ptr.value, rin * k), (Ye.ptr.value, rout * k), None, side=side, tol=tol,
                                  normalize=norm)
                assert same_bits(Ye.to_array(np.float64, rout * k).reshape((rout, k), order="F"), Y1)
                for b in (Bd, Yd, wd, Ye):
                    b.free()
    # tensors
    B = rs.standard_normal((n, 4))
    tB, tY, tw = Tensor(B.reshape(-1, order="F")), Tensor(np.full(m * 4, SENT)), Tensor(np.full(m, SENT))
    ws.apply_plan_dev(tB, tY, tw, side=0, tol=0.1)
    Y, w = ws.apply_plan(B, side=0, tol=0.1, mass=True)
    assert same_bits(tY.numpy().reshape((m, 4), order="F"), Y) and same_bits(tw.numpy(), w)
    with pytest.raises(ValueError):
        ws.apply_plan_dev((tB.data_ptr(), n * 4 - 1), tY)       # not k columns of n
    with pytest.raises(ValueError):
        ws.apply_plan_dev(tB, (tY.data_ptr(), m * 4 - 1))       # Y too small
    with pytest.raises(ValueError):
        ws.apply_plan(np.zeros((n + 1, 2)))
    with pytest.raises(ValueError):
        ws.apply_plan(B, side=2)
    ws.close()


@pytest.mark.parametrize("cls", [1, 2])
def test_workspace_untouched(cls):
    """state(), and a following plan(stats=True) and end(...), give the bits they give without the calls in between."""
    m, n = 257, 150
    pr = problem(cls, m, n, seed=8, pq_random=True)
    rs = np.random.RandomState(10)
    Xd = patterns(m, n, rs)["dense"] * (rs.random_sample((m, n)) < 0.4)
    B0, B1 = rs.standard_normal((n, 16)), rs.standard_normal((m, 5))
    seen = []
    for with_calls in (False, True):
        ws = ws_of(cls, pr)
        u, v, lam = inject(ws, Xd, np.random.RandomState(11))
        if with_calls:
            ws.apply_plan(B0, side=0, tol=0.3, mass=True)
            ws.apply_plan(B1, side=1, tol=0.0, normalize=True)
            ws.barycentric_map(B0[:, :3])
        st = ws.state()
        X, stats, ax = ws.plan(0.3, stats=True)
        if with_calls:
            ws.apply_plan(B0[:, :1], side=0)
        e = ws.end(lam, from_w=False)
        seen.append((st, X, stats, ax, e, ws.state()))
        ws.close()
    (sa, Xa, pa, axa, ea, ta), (sb, Xb, pb, axb, eb, tb) = seen
    for a, b in zip(sa[:3] + ta[:3], sb[:3] + tb[:3]):
        assert np.array_equal(bits(a), bits(b))
    assert sa[3] == sb[3] and ta[3] == tb[3]
    assert np.array_equal(Xa.indptr, Xb.indptr) and np.array_equal(Xa.indices, Xb.indices)
    assert np.array_equal(bits(Xa.data), bits(Xb.data)) and np.array_equal(bits(axa), bits(axb))
    assert pa["nnz"] == pb["nnz"]
    for key in ("sum_kept", "sum_dropped", "max_dropped", "fval_kept"):
        assert bits([pa[key]])[0] == bits([pb[key]])[0], key
    assert np.array_equal(bits(ea["kkt"]), bits(eb["kkt"])) and bits([ea["fx"]])[0] == bits([eb["fx"]])[0]


def test_barycentric_map_on_a_matrix_free_workspace():
    m, n = 65, 150
    rs = np.random.RandomState(12)
    xs, ys = rs.random_sample((m, 3)), rs.random_sample((n, 3))
    r, l = rs.random_sample(n), rs.random_sample(m)
    l = l * r.sum() / l.sum()
    ws = ipd().APDWorkspace.from_points(1, xs, ys, r, l, np.ones(m), np.ones(n), matrix_free=True)
    assert ws.cost_info()["form"] == 1
    Xd = np.abs(patterns(m, n, rs)["dense"]) * (rs.random_sample((m, n)) < 0.2)
    Xd[:, 0] += 0.5
    Xd[0, :] += 0.5          # no empty row or column
    inject(ws, Xd, rs)
    for side, pts in ((0, ys), (1, xs)):
        for tol in (0.0, 0.4):
            T = ws.barycentric_map(pts, side=side, tol=tol)
            assert T.shape == ((n if side else m), 3)
            assert same_bits(T, ws.apply_plan(pts, side=side, tol=tol, normalize=True))
            check_apply(ws, Xd, tol, pts, side, ks=[3])
            # a convex combination of the points: inside their bounding box (up to the rounding of the bar)
            assert np.all(T >= pts.min(axis=0) - 1e-12) and np.all(T <= pts.max(axis=0) + 1e-12)
    ws.close()


AMG1 = dict(retol=1e-11, bigph=1, maxit=30, theta=1 / 4, smoth=5, cycle="w", isnsp=1, inter=1, guess=None)
AMG2 = dict(retol=1e-11, bigph=1, maxit=40, theta=1 / 4, smoth=10, cycle="w", isnsp=1, inter=1, guess=None)


@pytest.mark.parametrize("cls", [1, 2])
def test_after_a_real_run(cls):
    """After warm start and two driver iterations (tests/test_gpu_plan.py's run-based size): apply_plan(B, tol) is
    within the bar of plan(tol) @ B."""
    m = n = 24
    pr = problem(cls, m, n, seed=12)
    ws = ws_of(cls, pr)
    ws.warmup(0.0, 40)
    ws.run(AMG1 if cls == 1 else AMG2, ipd().MatlabRand(), iters=2)
    rs = np.random.RandomState(13)
    xmax = float(np.abs(ws.state()[0][:m * n]).max())
    for tol in (0.0, 1e-3 * xmax):
        X = ws.plan(tol)
        Xt = X.toarray()
        for side in (0, 1):
            B = rs.standard_normal((m if side else n, 16))
            ref, bar, wref, wbar = reference(Xt, B, side)
            for k in KS:
                Y, w = ws.apply_plan(B[:, :k], side=side, tol=tol, mass=True)
                ok, over = within(Y, ref[:, :k], bar[:, :k])
                assert ok, (side, k, tol, over)
                assert within(w, wref, wbar)[0]
    ws.close()


def test_argument_errors_write_nothing():
    L = lib_mod()
    lib = L.lib
    m, n, k = 37, 5, 3
    pr = problem(1, m, n, seed=13)
    ws = ws_of(1, pr)
    rs = np.random.RandomState(14)
    inject(ws, patterns(m, n, rs)["dense"], rs)
    h, E, EL = ws.handle, L.IPD_E_ARG, L.IPD_E_LIMIT
    B = np.asfortranarray(rs.standard_normal((max(m, n), 17)))
    Bd = L.DeviceBuffer.from_array(B.reshape(-1, order="F"))
    t0, nan = 0.0, float("nan")
    #        h,  tol, side, k, normalize, B?, Y?
    cases = [("NULL h", None, t0, 0, k, 0, True, True, E),
             ("NULL B", h, t0, 0, k, 0, False, True, E),
             ("NULL Y", h, t0, 0, k, 0, True, False, E),
             ("side -1", h, t0, -1, k, 0, True, True, E),
             ("side 2", h, t0, 2, k, 0, True, True, E),
             ("normalize -1", h, t0, 0, k, -1, True, True, E),
             ("normalize 2", h, t0, 1, k, 2, True, True, E),
             ("tol -1", h, -1.0, 0, k, 0, True, True, E),
             ("tol -tiny", h, -1e-300, 1, k, 1, True, True, E),
             ("tol NaN", h, nan, 0, k, 0, True, True, E),
             ("k 0", h, t0, 0, 0, 0, True, True, EL),
             ("k -1", h, t0, 1, -1, 0, True, True, EL),
             ("k 17", h, t0, 0, 17, 1, True, True, EL)]
    cnt = max(m, n) * 17
    for name, hh, tol, side, kk, norm, hasB, hasY, code in cases:
        Y, w = np.full(cnt, SENT), np.full(max(m, n), SENT)
        rc = lib.ipd_apd_plan_apply(hh, ctypes.c_double(tol), side, kk, norm, B.ctypes.data if hasB else None,
                                    Y.ctypes.data if hasY else None, w.ctypes.data)
        assert rc == code, name
        assert (Y == SENT).all() and (w == SENT).all(), name
        Yd, wd = L.DeviceBuffer.from_array(Y), L.DeviceBuffer.from_array(w)
        rc = lib.ipd_apd_plan_apply_dev(hh, ctypes.c_double(tol), side, kk, norm, Bd.ptr if hasB else None,
                                        Yd.ptr if hasY else None, wd.ptr)
        assert rc == code, name + " (dev)"
        assert (Yd.to_array(np.float64, cnt) == SENT).all() and (wd.to_array(np.float64, max(m, n)) == SENT).all(), name
        Yd.free()
        wd.free()
    # the API reports them as IpdError
    with pytest.raises(L.IpdError) as ei:
        ws.apply_plan(B[:n, :17])
    assert ei.value.code == EL
    with pytest.raises(L.IpdError) as ei:
        ws.apply_plan(B[:n, :2], tol=-1.0)
    assert ei.value.code == E
    # and the unedited call is fine
    Y = np.full(m * k, SENT)
    assert lib.ipd_apd_plan_apply(h, ctypes.c_double(0.0), 0, k, 0, B.ctypes.data, Y.ctypes.data, None) == 0
    assert not (Y == SENT).any()
    Bd.free()
    ws.close()
