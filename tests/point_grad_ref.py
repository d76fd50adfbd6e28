"""The gradient of the transport cost in the point positions (csrc/ipd_point_grad_geo.h, csrc/ipd_point_grad.hip;
DESIGN.md section 4o) restated in numpy, operation by operation: every step below is one IEEE float64 operation on
arrays, in the order the header states it.  No GPU needed; tests/test_point_grad_ref.py checks the restatement against
central differences, tests/test_point_grad_geo.py checks the header's scalar code against it bit for bit, and
tests/test_gpu_point_grad.py checks the device against it.

xs is (m, d), ys (n, d), one point per row; X is (m, n).  metric: 1 sq. Euclidean, 2 Euclidean, 3 city block,
4 Chebyshev."""
import numpy as np

U = 2.0 ** -53
GROUP = 64          # WK_CPG * TC columns of a column group
WAVE = 64           # rows of a segment


def gamma(s):
    return s * U / (1.0 - s * U)


def diffs(xs, ys):
    """t[i, j, k] = xs(i,k) - ys(j,k), the subtraction of cost_fold"""
    xs, ys = np.asarray(xs, np.float64), np.asarray(ys, np.float64)
    return xs[:, None, :] - ys[None, :, :]


def sign(T):
    return np.where(T > 0.0, 1.0, np.where(T < 0.0, -1.0, 0.0))


def cost(xs, ys, metric):
    """the unscaled cost, folded in ascending k from +0.0 as cost_fold / cost_finish"""
    T = diffs(xs, ys)
    acc = np.zeros(T.shape[:2])
    for k in range(T.shape[2]):
        t = T[:, :, k]
        if metric == 3:
            acc = acc + np.abs(t)
        elif metric == 4:
            acc = np.maximum(acc, np.abs(t))
        else:
            sq = t * t
            acc = acc + sq
    return np.sqrt(acc) if metric == 2 else acc


def weights(xs, ys, metric, denom=None):
    """(H, kink): H[i, j, k] = h_k of the pair (i, j), divided by denom last when one is given; kink[i, j]: c is not
    differentiable at the pair."""
    T = diffs(xs, ys)
    m, n, d = T.shape
    if metric == 1:
        H = T + T
        kink = np.zeros((m, n), bool)
    elif metric == 2:
        acc = np.zeros((m, n))
        for k in range(d):
            sq = T[:, :, k] * T[:, :, k]
            acc = acc + sq
        a = np.sqrt(acc)
        pos = a > 0.0
        q = T / np.where(pos, a, 1.0)[:, :, None]          # a select: no 0/0 is formed
        H = np.where(pos[:, :, None], q, 0.0)
        kink = a == 0.0
    elif metric == 3:
        H = sign(T)
        kink = (T == 0.0).any(axis=2)
    elif metric == 4:
        acc = np.zeros((m, n))
        kstar = np.zeros((m, n), np.int64)
        tie = np.zeros((m, n), bool)
        for k in range(d):
            at = np.abs(T[:, :, k])
            up = at > acc                                   # strict: the first maximum stays
            tie = np.where(up, False, np.where(at == acc, True, tie))
            kstar = np.where(up, k, kstar)
            acc = np.where(up, at, acc)
        H = np.where(np.arange(d)[None, None, :] == kstar[:, :, None], sign(T), 0.0)
        kink = tie | (acc == 0.0)
    else:
        raise ValueError("metric")
    if denom is not None:
        H = H / denom
    return H, kink


def kept(X, tol):
    return ~(np.abs(X) <= tol)                               # walk_keep: a NaN is kept


def terms(X, H, side, tol):
    """what every entry adds: x*h_k (side 0) or x*(-h_k) (side 1) when it is kept, else +0.0"""
    K = kept(X, tol)
    Hs = -H if side else H
    with np.errstate(invalid="ignore", over="ignore"):
        P = X[:, :, None] * Hs
    return np.where(K[:, :, None], P, 0.0), K


def seq_sum(A, axis):
    """the sum along `axis` taken sequentially from +0.0 in ascending index"""
    A = np.moveaxis(A, axis, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.cumsum(np.concatenate([np.zeros((1,) + A.shape[1:]), A]), axis=0)[-1]


def rows_sum(P):
    """side 0's shape for P[i, j, ...]: within a group of GROUP columns sequentially from +0.0 in ascending j, then the
    groups' partials sequentially from +0.0 in ascending group"""
    n = P.shape[1]
    parts = [seq_sum(P[:, g0:g0 + GROUP], 1) for g0 in range(0, n, GROUP)]
    return seq_sum(np.stack(parts, axis=1), 1)


def gradient_rows(X, xs, ys, metric, tol=0.0, denom=None):
    """side 0 in the device's summation shape: (G (m, d), w (m), kept, kinks)"""
    H, kink = weights(xs, ys, metric, denom)
    P, K = terms(X, H, 0, tol)
    with np.errstate(invalid="ignore"):
        w = rows_sum(np.where(K, X, 0.0))
    return rows_sum(P), w, int(K.sum()), int((K & kink).sum())


def reference(X, xs, ys, metric, side, tol=0.0, denom=None):
    """either side with the sums in longdouble from the float64 weights, and the any-order bar of DESIGN.md section 4h:
    (ref, bar, wref, wbar, kept, kinks); |G - ref| <= bar = gamma(N + 4) * sum |x| |h_k| entrywise, N the summed
    dimension.  X must hold no NaN."""
    H, kink = weights(xs, ys, metric, denom)
    K = kept(X, tol)
    Xt = np.where(K, X, 0.0)
    Hs = -H if side else H
    ax = 0 if side else 1
    N = X.shape[ax]
    ld = np.longdouble
    ref = (Xt.astype(ld)[:, :, None] * Hs.astype(ld)).sum(axis=ax)
    bar = gamma(N + 4) * (np.abs(Xt)[:, :, None] * np.abs(Hs)).sum(axis=ax)
    wref = Xt.astype(ld).sum(axis=ax)
    wbar = gamma(N + 4) * np.abs(Xt).sum(axis=ax)
    return ref, bar, wref, wbar, int(K.sum()), int((K & kink).sum())


def within(G, ref, bar):
    """entrywise |G - ref| <= bar, exactly 0 where the bar is 0; also the worst excess"""
    err = np.abs(np.asarray(G, np.float64).astype(np.longdouble) - ref)
    return bool(np.all(err <= bar)), float(np.max(err - bar)) if err.size else 0.0


def bits_equal(a, b):
    """bit for bit, a -0.0 counting as +0.0 and a NaN matching any NaN"""
    a, b = np.asarray(a, np.float64) + 0.0, np.asarray(b, np.float64) + 0.0
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(
        np.ascontiguousarray(a[~na]).view(np.int64), np.ascontiguousarray(b[~nb]).view(np.int64))


def tie_points(m, n, d, seed):
    """point clouds on a coarse grid, so that exact ties are frequent: coincident points, zero differences in single
    coordinates and equal |t_k| -- with generic points in between"""
    rs = np.random.RandomState(seed)
    xs = rs.randint(-2, 3, size=(m, d)) * 0.5
    ys = rs.randint(-2, 3, size=(n, d)) * 0.5
    gx, gy = rs.random_sample(m) < 0.4, rs.random_sample(n) < 0.4
    xs[gx] = rs.standard_normal((int(gx.sum()), d))
    ys[gy] = rs.standard_normal((int(gy.sum()), d))
    return xs, ys
