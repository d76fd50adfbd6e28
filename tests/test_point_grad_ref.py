"""The numpy restatement of the point-position gradient (tests/point_grad_ref.py) against what it
claims to be: the derivative of <c(xs, ys), X> in the coordinates at fixed X, and -- the envelope theorem -- of the
optimal transport cost at the LP optimum.  Central differences with step 1e-6 on generic Gaussian points (7 x 5, d = 3,
all four metrics) to 1e-8 absolute: the truncation error is h^2/6 * |c'''| ~ 1e-12, the rounding error u * f / h ~ 1e-10
for a plan of unit mass (f is a few units); the eight comparisons give 1.1e-10 to 4.0e-10 (the test prints them), a
margin of 25.  Also: the kink counts on constructed ties, and metric 1 against 2 (w o xs - X ys).  CPU only."""
import numpy as np
import pytest
from scipy.optimize import linprog

from tests import point_grad_ref as R

M, N, D, STEP, TOL = 7, 5, 3, 1e-6, 1e-8
METRICS = [1, 2, 3, 4]


def clouds(seed):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((M, D)), rs.standard_normal((N, D)), rs


def lp(xs, ys, metric, l, r):
    """min <c, X>, X 1 = l, X' 1 = r, X >= 0 (HiGHS): (value, X)"""
    c = R.cost(xs, ys, metric)
    A = np.zeros((M + N, M * N))
    for i in range(M):
        A[i, i * N:(i + 1) * N] = 1.0
    for j in range(N):
        A[M + j, j::N] = 1.0
    res = linprog(c.reshape(-1), A_eq=A[:-1], b_eq=np.concatenate([l, r])[:-1], bounds=(0, None), method="highs")
    assert res.status == 0
    return res.fun, res.x.reshape(M, N)


def central(f, xs, ys):
    """central differences of f(xs, ys) in every coordinate of both clouds"""
    gx, gy = np.zeros_like(xs), np.zeros_like(ys)
    for P, g, which in ((xs, gx, 0), (ys, gy, 1)):
        for idx in np.ndindex(*P.shape):
            vals = []
            for s in (STEP, -STEP):
                Q = P.copy()
                Q[idx] += s
                vals.append(f(Q, ys) if which == 0 else f(xs, Q))
            g[idx] = (vals[0] - vals[1]) / (2 * STEP)
    return gx, gy


def both_sides(X, xs, ys, metric):
    H, _ = R.weights(xs, ys, metric)
    return (X[:, :, None] * H).sum(axis=1), (X[:, :, None] * -H).sum(axis=0)


@pytest.mark.parametrize("metric", METRICS)
def test_fixed_plan_central_differences(metric):
    xs, ys, rs = clouds(10 + metric)
    X = rs.random_sample((M, N))
    X /= X.sum()                                    # a plan of unit mass: f is a few units, u * f / h ~ 1e-10
    gx, gy = both_sides(X, xs, ys, metric)
    cx, cy = central(lambda a, b: float((R.cost(a, b, metric) * X).sum()), xs, ys)
    err = max(np.abs(gx - cx).max(), np.abs(gy - cy).max())
    print("metric %d: fixed X, max |G - central| = %.3e" % (metric, err))
    assert err <= TOL
    # the device's summation shape gives the same numbers up to rounding
    G0, w, kept, kinks = R.gradient_rows(X, xs, ys, metric)
    assert np.abs(G0 - gx).max() <= 1e-14 * np.abs(gx).max() * N and kept == M * N and kinks == 0
    assert np.allclose(w, X.sum(axis=1), rtol=1e-15 * N, atol=0)


@pytest.mark.parametrize("metric", METRICS)
def test_lp_optimum_central_differences(metric):
    """the envelope theorem: the derivative of the LP optimum is the derivative at the fixed optimal plan"""
    xs, ys, rs = clouds(20 + metric)
    l, r = rs.random_sample(M) + 0.5, rs.random_sample(N) + 0.5
    r /= r.sum()
    l /= l.sum()                                    # unit mass on both sides
    _, X = lp(xs, ys, metric, l, r)
    gx, gy = both_sides(X, xs, ys, metric)
    cx, cy = central(lambda a, b: lp(a, b, metric, l, r)[0], xs, ys)
    err = max(np.abs(gx - cx).max(), np.abs(gy - cy).max())
    print("metric %d: LP optimum, max |G - central| = %.3e" % (metric, err))
    assert err <= TOL


def test_kinks_count_the_constructed_ties():
    rs = np.random.RandomState(3)
    xs, ys = rs.standard_normal((M, D)), rs.standard_normal((N, D))
    xs[2:5] = np.round(xs[2:5] * 8) / 8             # dyadic: the differences below are exact
    ys[0] = xs[0]                                   # coincident: a kink of 2, 3 and 4
    ys[1, 1] = xs[1, 1]                             # one zero difference: a kink of 3 only
    ys[2] = xs[2] - np.array([0.5, -0.5, 0.25])     # |t_0| == |t_1| the maximum: a kink of 4 only
    ys[3] = xs[3] - np.array([0.25, 0.5, -0.5])     # the maximum at k = 1 and 2: k* is the first of them
    ys[4] = xs[4] - np.array([0.5, 0.25, 0.25])     # a tie below the maximum: no kink
    want = {1: set(), 2: {(0, 0)}, 3: {(0, 0), (1, 1)}, 4: {(0, 0), (2, 2), (3, 3)}}
    for metric in METRICS:
        H, kink = R.weights(xs, ys, metric)
        assert set(zip(*np.nonzero(kink))) == want[metric], metric
        X = np.ones((M, N))
        X[1, 1] = 0.0                               # a dropped entry is not counted
        _, _, kept, kinks = R.gradient_rows(X, xs, ys, metric)
        assert kept == M * N - 1 and kinks == len(want[metric] - {(1, 1)}), metric
    H2, H3, H4 = (R.weights(xs, ys, k)[0] for k in (2, 3, 4))
    assert not H2[0, 0].any() and not np.signbit(H2[0, 0]).any()          # a == 0: +0.0, no NaN
    assert np.array_equal(H3[1, 1], [np.sign(xs[1, 0] - ys[1, 0]), 0.0, np.sign(xs[1, 2] - ys[1, 2])])
    assert np.array_equal(H4[2, 2], [1.0, 0.0, 0.0]) and np.array_equal(H4[3, 3], [0.0, 1.0, 0.0])
    assert np.array_equal(H4[4, 4], [1.0, 0.0, 0.0]) and not H4[0, 0].any()
    # scale: one division, applied last
    Hs, _ = R.weights(xs, ys, 2, denom=3.0)
    assert R.bits_equal(Hs, H2 / 3.0)


def test_sq_euclidean_is_the_plan_product():
    """metric 1: G0 = 2 (w o xs - X ys), within the sum of the two any-order bars"""
    rs = np.random.RandomState(4)
    m, n, d = 65, 150, 3
    xs, ys = rs.standard_normal((m, d)), rs.standard_normal((n, d))
    X = rs.random_sample((m, n)) * (rs.random_sample((m, n)) < 0.3)
    G0, w, _, _ = R.gradient_rows(X, xs, ys, 1)
    ld = np.longdouble
    want = 2 * (X.sum(axis=1).astype(ld)[:, None] * xs.astype(ld) - X.astype(ld) @ ys.astype(ld))
    ref, bar, _, _, _, _ = R.reference(X, xs, ys, 1, 0)
    bar2 = 2 * R.gamma(n + 4) * (X.sum(axis=1)[:, None] * np.abs(xs) + X @ np.abs(ys))
    assert np.all(np.abs(G0.astype(ld) - want) <= bar + bar2)
    assert R.within(G0, ref, bar)[0]


def test_summation_shape_is_the_groups():
    """the restatement's side 0 is cumsum inside the groups of 64 columns, then over the groups"""
    rs = np.random.RandomState(5)
    P = rs.standard_normal((3, 150))
    want = np.zeros(3)
    for i in range(3):
        tot = 0.0
        for g0 in range(0, 150, 64):
            s = 0.0
            for j in range(g0, min(g0 + 64, 150)):
                s = s + P[i, j]
            tot = tot + s
        want[i] = tot
    assert R.bits_equal(R.rows_sum(P), want)
