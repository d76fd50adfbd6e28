"""The dual certificate on the device (csrc/ipd_dual.hip: ipd_apd_dual, ipd_apd_dual_dev; APDWorkspace.dual, dual_dev,
c_transform, certificate).

Reference: numpy restatements of the header's definitions, operation by operation.  With C = c.reshape((m, n),
order="F"), lam = [alpha (n); beta (m)(; tau)]:
  transform  T = ((-C [- tau*PHI]) - p_i*alpha_j) / q_j   (side 1: ... - q_j*beta_i) / p_i), NaN -> -inf, then .max and
             .argmax along the axis -- maxima are order-independent, so lam_out and arg are compared bit for bit;
  evaluate   D = ((C + p_i*alpha_j) + q_j*beta_i) [+ tau*PHI]: dmin, its first column-major place and the count of
             D < 0 exactly; the sums (cap, bterm, dual, fval) against longdouble within gamma(N + 4) * sum|terms|,
             gamma(s) = s*u / (1 - s*u), u = 2^-53, N the number of terms (DESIGN.md section 4h's any-order bound).
States are injected with set_state; only the feasibility and the driver tests run the solver."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
INF = np.inf

# tests/test_gpu_plan.py's shapes (degenerate dimensions, the wave, chunk and workgroup boundaries), 65 x 150 (three
# column groups, the last chunk partly filled) and 300 x 16 (a second row block with a partly filled wave):
# tests/test_dual_geo.py pins the last two
SHAPES = [(1, 1), (1, 37), (37, 1), (63, 17), (64, 16), (65, 33), (257, 19), (600, 45), (65, 150), (300, 16)]


def ipd():
    import codes_of_ipd_ssn_amg_method_amd as pkg
    return pkg


def lib_mod():
    from codes_of_ipd_ssn_amg_method_amd import _lib
    return _lib


def gamma(s):
    return s * U / (1.0 - s * U)


def problem(cls, m, n, seed=1, pq_random=False):
    """tests/test_gpu_plan_apply.py's synthetic inputs, re-stated: c,r,l ~ U(0,1) (draw order c,r,l), p=q=1, phi=1
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


def ws_of(cls, pr, gama=INF):
    if cls == 1:
        return ipd().APDWorkspace(1, pr["c"], pr["r"], pr["l"], pr["p"], pr["q"], gama=gama)
    return ipd().APDWorkspace(2, pr["c"], pr["r"], pr["l"], pr["p"], pr["q"], mu=pr["mu"], phi=pr["phi"])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def inject(ws, Xd, rs, lam=None):
    """state with the x block of u = Xd(:), everything else random; returns (u, v, lam)."""
    u = rs.standard_normal(ws.U)
    u[:ws.m * ws.n] = Xd.reshape(-1, order="F")
    v = rs.standard_normal(ws.U)
    lam = rs.standard_normal(ws.L) if lam is None else lam
    ws.set_state(u, v, lam, 0.37)
    return u, v, lam


def clamp0(a):
    return np.where(a > 0, a, 0.0)


def mats(cls, pr, m, n):
    C = pr["c"].reshape((m, n), order="F")
    PHI = pr["phi"].reshape((m, n), order="F") if cls == 2 else None
    return C, PHI


def transform_ref(cls, pr, m, n, lam, side):
    """(lam_out, arg) of the header's definition"""
    C, PHI = mats(cls, pr, m, n)
    p, q = pr["p"], pr["q"]
    alpha, beta = lam[:n].copy(), lam[n:n + m].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        base = -C
        if cls == 2:
            base = base - lam[n + m] * PHI
        if side == 0:
            if cls == 2:
                alpha = clamp0(alpha)
            T = (base - p[:, None] * alpha[None, :]) / q[None, :]
        else:
            if cls == 2:
                beta = clamp0(beta)
            T = (base - q[None, :] * beta[:, None]) / p[:, None]
    T = np.where(np.isnan(T), -INF, T)
    axis = 1 if side == 0 else 0
    new, arg = T.max(axis=axis), T.argmax(axis=axis)
    if cls == 2:
        new = clamp0(new)
    out = np.concatenate([alpha, new] if side == 0 else [new, beta])
    if cls == 2:
        out = np.append(out, lam[n + m])
    return out, arg.astype(np.int32)


def eval_ref(cls, pr, m, n, lam, gama=INF, x=None):
    """dict of what ipd_apd_dual reports for lam (side = -1), the sums as (longdouble value, bar)"""
    C, PHI = mats(cls, pr, m, n)
    p, q = pr["p"], pr["q"]
    alpha, beta = lam[:n], lam[n:n + m]
    with np.errstate(invalid="ignore", over="ignore"):
        D = (C + p[:, None] * alpha[None, :]) + q[None, :] * beta[:, None]
        if cls == 2:
            D = D + lam[n + m] * PHI
    Dv = D.reshape(-1, order="F")
    full = np.concatenate([Dv, alpha, beta]) if cls == 2 else Dv
    k = int(np.argmin(np.where(np.isnan(full), INF, full)))
    out = dict(dmin=full[k], imin=k % m if k < m * n else -1, jmin=k // m if k < m * n else -1,
               nneg=int((full < 0).sum()))
    ld = np.longdouble
    b = np.concatenate([pr["r"], pr["l"]] + ([[pr["mu"]]] if cls == 2 else []))
    tb = b.astype(ld) * lam.astype(ld)
    out["bterm"] = (-tb.sum(), gamma(b.size + 4) * float(np.abs(tb).sum()))
    finite = cls == 1 and (np.ndim(gama) > 0 or np.isfinite(gama))
    if finite:
        G = np.broadcast_to(np.asarray(gama, dtype=np.float64).reshape(-1), (m * n,)) if np.ndim(gama) == 0 \
            else np.asarray(gama, dtype=np.float64).reshape(-1)
        tc = np.where(Dv < 0, G.astype(ld) * (-Dv).astype(ld), ld(0))
        out["cap"] = (tc.sum(), gamma(m * n + 4) * float(np.abs(tc).sum()))
    else:
        out["cap"] = (ld(0), 0.0)
    out["dual"] = (out["bterm"][0] - out["cap"][0],
                   gamma(b.size + m * n + 4) * float(np.abs(tb).sum() + (np.abs(tc).sum() if finite else 0)))
    if x is not None:
        tf = pr["c"].astype(ld) * x[:m * n].astype(ld)
        out["fval"] = (tf.sum(), gamma(m * n + 4) * float(np.abs(tf).sum()))
    return out


def check_eval(res, ref, what=""):
    assert bits([res["dmin"]])[0] == bits([ref["dmin"]])[0], (what, res["dmin"], ref["dmin"])
    assert (res["imin"], res["jmin"], res["nneg"]) == (ref["imin"], ref["jmin"], ref["nneg"]), (what, res, ref)
    for key in ("bterm", "cap", "dual") + (("fval",) if "fval" in ref else ()):
        want, bar = ref[key]
        err = abs(np.longdouble(res[key]) - want)
        print("%s %s: err %.3e bar %.3e" % (what, key, float(err), bar))
        assert err <= bar, (what, key, res[key], float(want), float(err), bar)
    if "fval" in ref:
        assert bits([res["gap"]])[0] == bits([res["fval"] - res["dual"]])[0], what
    else:
        assert np.isnan(res["fval"]) and np.isnan(res["gap"]), what


def random_lam(cls, ws, rs):
    lam = rs.standard_normal(ws.L)
    if cls == 2:
        lam[0] = -0.5 - abs(lam[0])           # an alpha and a beta that are negative for certain: class 2 clamps them
        lam[ws.n] = -0.5 - abs(lam[ws.n])
        lam[-1] = -0.25 - rs.random_sample()  # tau < 0
    return lam


# ---------------------------------------------------------------------------
# 1. transform, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pq_random", [False, True])
@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", SHAPES)
def test_transform_bit_for_bit(cls, m, n, pq_random):
    pr = problem(cls, m, n, seed=3, pq_random=pq_random)
    ws = ws_of(cls, pr)
    rs = np.random.RandomState(100 * m + n)
    lam = random_lam(cls, ws, rs)
    inject(ws, rs.random_sample((m, n)), rs, lam=lam)
    other = random_lam(cls, ws, rs)
    for side in (0, 1):
        for given, L in ((None, lam), (other, other)):      # the workspace's lk, and an explicit one
            want, warg = transform_ref(cls, pr, m, n, L, side)
            res = ws.dual(given, side=side, arg=True)
            assert same_bits(res["lam"], want), (side, given is None, np.flatnonzero(bits(res["lam"]) != bits(want)))
            assert res["arg"].dtype == np.int32 and np.array_equal(res["arg"], warg), (side, given is None)
            assert same_bits(ws.c_transform(given, side=side), want)
            assert "arg" not in ws.dual(given, side=side)
            # and the evaluation that follows is the evaluation of the result
            check_eval(res, eval_ref(cls, pr, m, n, want), "side %d" % side)
    ws.close()


# ---------------------------------------------------------------------------
# 2. index plumbing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(65, 33), (64, 16)])
def test_arg_finds_a_planted_winner_everywhere(m, n):
    """c is 1 except for one tiny entry per row (side 0) or per column (side 1); over the shifts the winner stands at
    every column of every row and at every row of every column."""
    rs = np.random.RandomState(7)
    p, q = np.ones(m), np.ones(n)
    r, l = rs.random_sample(n), rs.random_sample(m)
    lam = 0.125 * rs.random_sample(m + n)       # differences below the planted gap of 9
    seen0, seen1 = np.zeros((m, n), bool), np.zeros((m, n), bool)
    for shift in range(max(m, n)):
        if shift < n:
            C = np.ones((m, n))
            win = (np.arange(m) + shift) % n
            C[np.arange(m), win] = -8.0
            ws = ipd().APDWorkspace(1, C.reshape(-1, order="F"), r, l, p, q)
            res = ws.dual(lam, side=0, arg=True)
            assert np.array_equal(res["arg"], win), shift
            seen0[np.arange(m), win] = True
            ws.close()
        if shift < m:
            C = np.ones((m, n))
            win = (np.arange(n) + shift) % m
            C[win, np.arange(n)] = -8.0
            ws = ipd().APDWorkspace(1, C.reshape(-1, order="F"), r, l, p, q)
            res = ws.dual(lam, side=1, arg=True)
            assert np.array_equal(res["arg"], win), shift
            seen1[win, np.arange(n)] = True
            ws.close()
    assert seen0.all() and seen1.all()


@pytest.mark.parametrize("m,n", [(65, 33), (64, 16), (65, 150), (300, 16)])
def test_ties_go_to_the_smallest_index(m, n):
    rs = np.random.RandomState(8)
    p, q = np.ones(m), np.ones(n)
    r, l = rs.random_sample(n), rs.random_sample(m)
    zero = np.zeros(m + n)
    ws = ipd().APDWorkspace(1, np.full(m * n, 0.75), r, l, p, q)       # every candidate ties
    for side in (0, 1):
        res = ws.dual(zero, side=side, arg=True)
        assert not res["arg"].any(), side
        assert np.array_equal(res["lam"][n:] if side == 0 else res["lam"][:n], np.full(m if side == 0 else n, -0.75))
    ws.close()
    C = rs.randint(0, 3, size=(m, n)).astype(np.float64)               # repeated maxima
    pr = dict(c=C.reshape(-1, order="F"), p=p, q=q)
    ws = ipd().APDWorkspace(1, pr["c"], r, l, p, q)
    for side in (0, 1):
        want, warg = transform_ref(1, pr, m, n, zero, side)
        res = ws.dual(zero, side=side, arg=True)
        assert np.array_equal(res["arg"], warg) and same_bits(res["lam"], want), side
        ties = (C == C.min(axis=1 if side == 0 else 0, keepdims=True)).sum(axis=1 if side == 0 else 0)
        assert (ties > 1).any()
    ws.close()


def test_an_infinite_held_entry_is_never_chosen_unless_alone():
    m, n = 65, 33
    pr = problem(1, m, n, seed=9, pq_random=True)
    ws = ws_of(1, pr)
    rs = np.random.RandomState(10)
    lam = rs.standard_normal(m + n)
    lam[[0, 5, n - 1]] = INF                # alpha
    lam[[n + 0, n + 64]] = INF              # beta
    for side, dead in ((0, [0, 5, n - 1]), (1, [0, 64])):
        res = ws.dual(lam, side=side, arg=True)
        want, warg = transform_ref(1, pr, m, n, lam, side)
        assert not np.isin(res["arg"], dead).any() and np.array_equal(res["arg"], warg)
        assert same_bits(res["lam"], want) and np.isfinite(res["lam"][n:] if side == 0 else res["lam"][:n]).all()
    ws.close()
    for mm, nn, side in ((37, 1, 0), (1, 37, 1)):        # the only column / row
        pr = problem(1, mm, nn, seed=11)
        ws = ws_of(1, pr)
        lam = np.full(mm + nn, INF)
        res = ws.dual(lam, side=side, arg=True)
        assert not res["arg"].any()
        new = res["lam"][nn:] if side == 0 else res["lam"][:nn]
        assert np.array_equal(new, np.full(new.size, -INF))
        ws.close()


# ---------------------------------------------------------------------------
# 3. evaluate
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["inf", "scalar", "vector", "class2"])
@pytest.mark.parametrize("m,n", SHAPES)
def test_evaluate(kind, m, n):
    cls = 2 if kind == "class2" else 1
    pr = problem(cls, m, n, seed=4, pq_random=True)
    rs = np.random.RandomState(31 * m + n)
    gama = {"inf": INF, "scalar": 0.625, "vector": 0.25 + rs.random_sample(m * n), "class2": INF}[kind]
    ws = ws_of(cls, pr, gama=gama)
    lam = random_lam(cls, ws, rs)
    u, _, _ = inject(ws, rs.standard_normal((m, n)), rs, lam=lam)
    other = random_lam(cls, ws, rs)
    for given, L in ((None, lam), (other, other)):
        res = ws.dual(given, primal=True)
        assert "lam" not in res and "arg" not in res
        ref = eval_ref(cls, pr, m, n, L, gama=gama, x=u)
        assert ref["nneg"] > 0 or min(m, n) == 1      # (a single beta or alpha can lift a whole row)
        check_eval(res, ref, kind)
        if kind in ("inf", "class2"):
            assert res["cap"] == 0.0 and bits([res["dual"]])[0] == bits([res["bterm"]])[0]
        res0 = ws.dual(given)                     # primal = 0: NaN for both, everything else the same bits
        check_eval(res0, eval_ref(cls, pr, m, n, L, gama=gama), kind)
        for key in ("dual", "bterm", "cap", "dmin"):
            assert bits([res0[key]])[0] == bits([res[key]])[0], key
    ws.close()


def test_evaluate_finds_the_minimum_in_the_y_and_z_blocks():
    m, n = 65, 33
    pr = problem(2, m, n, seed=5, pq_random=True)
    ws = ws_of(2, pr)
    rs = np.random.RandomState(12)
    lam = np.abs(rs.standard_normal(ws.L)) + 0.5
    lam[-1] = 0.25                                 # d > 0 everywhere
    for k in (3, n + 40):                          # an alpha, a beta
        L = lam.copy()
        L[k] = 1e-3
        res = ws.dual(L)
        assert (res["dmin"], res["imin"], res["jmin"], res["nneg"]) == (1e-3, -1, -1, 0)
        L[k] = -2.0
        ref = eval_ref(2, pr, m, n, L)
        check_eval(ws.dual(L), ref)
    ws.close()


# ---------------------------------------------------------------------------
# 4. cost sources agree
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_cost_sources_agree(cls, d):
    m, n = 65, 150
    rs = np.random.RandomState(40 + d)
    xs, ys = rs.random_sample((m, d)), rs.random_sample((n, d))
    r, l = rs.random_sample(n), rs.random_sample(m)
    p, q = 0.5 + rs.random_sample(m), 0.5 + rs.random_sample(n)
    kw = dict(mu=0.65 * min(r.sum(), l.sum()), phi=0.5 + rs.random_sample(m * n)) if cls == 2 else {}
    for metric in ("sqeuclidean", "cityblock"):
        for scale in (False, True):
            stored = ipd().APDWorkspace.from_points(cls, xs, ys, r, l, p, q, metric=metric, scale=scale, **kw)
            free = ipd().APDWorkspace.from_points(cls, xs, ys, r, l, p, q, metric=metric, scale=scale,
                                                  matrix_free=True, **kw)
            assert (stored.cost_info()["form"], free.cost_info()["form"]) == (0, 1)
            host = ipd().APDWorkspace(cls, stored.cost().reshape(-1, order="F"), r, l, p, q, **kw)
            lam = random_lam(cls, host, rs)
            Xd = rs.standard_normal((m, n))
            for ws in (host, stored, free):
                inject(ws, Xd, np.random.RandomState(5), lam=lam)
            for side in (-1, 0, 1):
                got = [ws.dual(side=side, primal=True, arg=side >= 0) for ws in (host, stored, free)]
                for other in got[1:]:
                    assert got[0].keys() == other.keys()
                    for key, val in got[0].items():
                        if key == "arg":
                            assert np.array_equal(val, other[key]), (metric, scale, side, key)
                        elif key in ("imin", "jmin", "nneg"):
                            assert val == other[key], (metric, scale, side, key)
                        else:
                            assert same_bits(val, other[key]), (metric, scale, side, key)
            for ws in (host, stored, free):
                ws.close()


# ---------------------------------------------------------------------------
# 5. feasibility and weak duality
# ---------------------------------------------------------------------------
AMG1 = dict(retol=1e-11, bigph=1, maxit=30, theta=1 / 4, smoth=5, cycle="w", isnsp=1, inter=1, guess=None)
AMG2 = dict(retol=1e-11, bigph=1, maxit=40, theta=1 / 4, smoth=10, cycle="w", isnsp=1, inter=1, guess=None)


def optimum(cls, pr, m, n):
    """f* of the linear program, by HiGHS on the CPU: min <c,x>, [X'p; Xq] (+ [y; z]) = [r; l], (<phi,x> = mu,)
    x (, y, z) >= 0"""
    import scipy.sparse as sp
    from scipy.optimize import linprog
    A = sp.vstack([sp.kron(sp.identity(n), pr["p"][None, :]), sp.kron(pr["q"][None, :], sp.identity(m))])
    b = np.concatenate([pr["r"], pr["l"]])
    c = pr["c"]
    if cls == 2:
        A = sp.vstack([sp.hstack([A, sp.identity(m + n)]), sp.hstack([sp.csr_matrix(pr["phi"][None, :]),
                                                                       sp.csr_matrix((1, m + n))])])
        b = np.append(b, pr["mu"])
        c = np.concatenate([c, np.zeros(m + n)])
    res = linprog(c, A_eq=sp.csr_matrix(A), b_eq=b, bounds=(0, None), method="highs")
    assert res.status == 0, res.message
    return float(res.fun)


@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", [(24, 24), (37, 29)])
def test_feasibility_and_weak_duality(cls, m, n):
    pr = problem(cls, m, n, seed=12)
    fstar = optimum(cls, pr, m, n)
    ws = ws_of(cls, pr)
    ws.warmup(0.0, 40)
    ws.run(AMG1 if cls == 1 else AMG2, ipd().MatlabRand(), iters=2)
    C, PHI = mats(cls, pr, m, n)
    p, q, r, l = pr["p"], pr["q"], pr["r"], pr["l"]
    duals = []
    for side in (0, 1):
        res = ws.dual(side=side, primal=True, arg=True)
        lam = res["lam"]
        alpha, beta = lam[:n], lam[n:n + m]
        size = np.abs(C) + np.abs(p[:, None] * alpha[None, :]) + np.abs(q[None, :] * beta[:, None])
        slack = gamma(m + n + 4) * (np.abs(r) @ np.abs(alpha) + np.abs(l) @ np.abs(beta))
        if cls == 2:
            size = size + np.abs(lam[n + m] * PHI)
            slack += gamma(m + n + 4) * pr["mu"] * abs(lam[n + m])
            assert (alpha >= 0).all() and (beta >= 0).all()
        floor = -4 * U * float(size.max())       # three roundings and the division
        print("cls %d %dx%d side %d: dmin %.3e (floor %.3e) dual %.12g f* %.12g gap %.3e"
              % (cls, m, n, side, res["dmin"], floor, res["dual"], fstar, res["gap"]))
        assert res["dmin"] >= floor, (side, res["dmin"], floor)
        assert res["dual"] <= fstar + abs(min(res["dmin"], 0.0)) * l.sum() / q.min() + slack, (side, res["dual"], fstar)
        duals.append(res)
    cert = ws.certificate()
    best = 1 if duals[1]["dual"] > duals[0]["dual"] else 0
    assert cert["side"] == best and cert["dual"] == max(duals[0]["dual"], duals[1]["dual"])
    for key, val in duals[best].items():
        assert np.array_equal(val, cert[key]) if key in ("arg",) else same_bits(val, cert[key]), key
    ws.close()


# ---------------------------------------------------------------------------
# 6. read-only
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [1, 2])
def test_workspace_untouched(cls):
    """state(), history(), and a following plan(stats=True) and end(...), give the bits they give without the calls
    in between."""
    m, n = 257, 150
    pr = problem(cls, m, n, seed=8, pq_random=True)
    rs = np.random.RandomState(10)
    Xd = rs.standard_normal((m, n)) * (rs.random_sample((m, n)) < 0.4)
    seen = []
    for with_calls in (False, True):
        ws = ws_of(cls, pr)
        u, v, lam = inject(ws, Xd, np.random.RandomState(11))
        if with_calls:
            ws.dual(primal=True)
            ws.dual(side=0, primal=True, arg=True)
            ws.dual(rs.standard_normal(ws.L), side=1)
            ws.certificate()
        st = ws.state()
        hist = ws.history()
        X, stats, ax = ws.plan(0.3, stats=True)
        if with_calls:
            ws.c_transform(side=1)
        e = ws.end(lam, from_w=False)
        seen.append((st, X, stats, ax, e, ws.state(), hist, ws.history()))
        ws.close()
    (sa, Xa, pa, axa, ea, ta, ha, ga), (sb, Xb, pb, axb, eb, tb, hb, gb) = seen
    for a, b in zip(sa[:3] + ta[:3], sb[:3] + tb[:3]):
        assert np.array_equal(bits(a), bits(b))
    assert sa[3] == sb[3] and ta[3] == tb[3]
    for x, y in ((ha, hb), (ga, gb)):
        assert x.keys() == y.keys() and all(same_bits(x[k], y[k]) for k in x)
    assert np.array_equal(Xa.indptr, Xb.indptr) and np.array_equal(Xa.indices, Xb.indices)
    assert np.array_equal(bits(Xa.data), bits(Xb.data)) and np.array_equal(bits(axa), bits(axb))
    assert pa["nnz"] == pb["nnz"]
    for key in ("sum_kept", "sum_dropped", "max_dropped", "fval_kept"):
        assert bits([pa[key]])[0] == bits([pb[key]])[0], key
    assert np.array_equal(bits(ea["kkt"]), bits(eb["kkt"])) and bits([ea["fx"]])[0] == bits([eb["fx"]])[0]


# ---------------------------------------------------------------------------
# 7. entries
# ---------------------------------------------------------------------------
class Tensor:
    """anything with torch's tensor interface is taken as it is (a stand-in over library memory: the suite keeps a
    second HIP runtime out of this process)"""

    def __init__(self, a, dtype=np.float64):
        a = np.ascontiguousarray(a, dtype=dtype)
        self.buf, self.count, self.dtype = lib_mod().DeviceBuffer.from_array(a), a.size, dtype

    def data_ptr(self):
        return self.buf.ptr.value

    def element_size(self):
        return np.dtype(self.dtype).itemsize

    def is_contiguous(self):
        return True

    def numel(self):
        return self.count

    def numpy(self):
        return self.buf.to_array(self.dtype, self.count)


SENT = -1234.5
STAT_KEYS = ("dual", "bterm", "cap", "dmin", "imin", "jmin", "nneg", "fval", "gap")


def same_stats(a, b):
    return all(same_bits(a[k], b[k]) for k in STAT_KEYS)


@pytest.mark.parametrize("cls", [1, 2])
def test_calls_agree(cls):
    """Two calls, and the host and the device entry: the same bits."""
    L = lib_mod()
    m, n = 600, 150
    pr = problem(cls, m, n, seed=7, pq_random=True)
    ws = ws_of(cls, pr)
    rs = np.random.RandomState(9)
    inject(ws, rs.standard_normal((m, n)), rs, lam=random_lam(cls, ws, rs))
    other = random_lam(cls, ws, rs)
    for given in (None, other):
        for side in (-1, 0, 1):
            for primal in (False, True):
                a = ws.dual(given, side=side, primal=primal, arg=True)
                b = ws.dual(given, side=side, primal=primal, arg=True)
                assert same_stats(a, b)
                rows = (m, n)[side] if side >= 0 else 1
                lam_d = L.DeviceBuffer.from_array(given) if given is not None else None
                out_d = L.DeviceBuffer.from_array(np.full(ws.L, SENT))
                arg_d = L.DeviceBuffer.from_array(np.full(rows, -77, np.int32))
                c = ws.dual_dev(lam_d, side=side, primal=primal, lam_out=out_d, arg=arg_d)
                assert same_stats(a, c)
                got_out, got_arg = out_d.to_array(np.float64, ws.L), arg_d.to_array(np.int32, rows)
                if side >= 0:
                    assert same_bits(a["lam"], b["lam"]) and np.array_equal(a["arg"], b["arg"])
                    assert same_bits(got_out, a["lam"]) and np.array_equal(got_arg, a["arg"])
                else:
                    assert (got_out == SENT).all() and (got_arg == -77).all()     # ignored for side = -1
                # without lam_out and arg: the same statistics
                assert same_stats(ws.dual_dev(lam_d, side=side, primal=primal), a)
                for buf in (lam_d, out_d, arg_d):
                    if buf is not None:
                        buf.free()
    # tensors, (pointer, entries) pairs, and in place
    t_lam, t_out, t_arg = Tensor(other), Tensor(np.full(ws.L, SENT)), Tensor(np.full(m, -77), np.int32)
    a = ws.dual(other, side=0, arg=True)
    assert same_stats(ws.dual_dev(t_lam, side=0, lam_out=t_out, arg=(t_arg.data_ptr(), m)), a)
    assert same_bits(t_out.numpy(), a["lam"]) and np.array_equal(t_arg.numpy(), a["arg"])
    assert same_stats(ws.dual_dev(t_lam, side=0, lam_out=t_lam), a) and same_bits(t_lam.numpy(), a["lam"])
    with pytest.raises(ValueError):
        ws.dual_dev((t_out.data_ptr(), ws.L - 1))
    with pytest.raises(ValueError):
        ws.dual_dev(t_out, side=1, arg=(t_arg.data_ptr(), n - 1))
    with pytest.raises(ValueError):
        ws.dual_dev(t_arg)                      # int32 is not a multiplier
    with pytest.raises(ValueError):
        ws.dual(other[:-1])
    with pytest.raises(ValueError):
        ws.dual(side=2)
    with pytest.raises(ValueError):
        ws.c_transform(side=-1)
    ws.close()


# ---------------------------------------------------------------------------
# 8. errors
# ---------------------------------------------------------------------------
def raw_calls(L, ws, h, lam, side, primal, with_st=True):
    """both entries on pre-filled outputs -> [(rc, lam_out, arg, stats bytes)]"""
    lib = L.lib
    rows = max(ws.m, ws.n)
    out = []
    st = (ctypes.c_double * 9)(*([SENT] * 9))
    lo, ar = np.full(ws.L, SENT), np.full(rows, -77, np.int32)
    rc = lib.ipd_apd_dual(h, lam.ctypes.data, side, primal, lo.ctypes.data, ar.ctypes.data,
                          ctypes.addressof(st) if with_st else None)
    out.append((rc, lo, ar, np.array(st)))
    st = (ctypes.c_double * 9)(*([SENT] * 9))
    lam_d, lo_d, ar_d = L.DeviceBuffer.from_array(lam), L.DeviceBuffer.from_array(lo), L.DeviceBuffer.from_array(ar)
    rc = lib.ipd_apd_dual_dev(h, lam_d.ptr, side, primal, lo_d.ptr, ar_d.ptr, ctypes.addressof(st) if with_st else None)
    out.append((rc, lo_d.to_array(np.float64, ws.L), ar_d.to_array(np.int32, rows), np.array(st)))
    for b in (lam_d, lo_d, ar_d):
        b.free()
    return out


def untouched(call):
    rc, lo, ar, st = call
    return (lo == SENT).all() and (ar == -77).all() and (st == SENT).all()


def test_argument_errors_write_nothing():
    L = lib_mod()
    m, n = 37, 5
    pr = problem(1, m, n, seed=13)
    ws = ws_of(1, pr)
    rs = np.random.RandomState(14)
    inject(ws, rs.standard_normal((m, n)), rs)
    lam = rs.standard_normal(ws.L)
    h, E = ws.handle, L.IPD_E_ARG
    cases = [("NULL h", None, 0, 0, True), ("NULL st", h, 0, 0, False), ("side -2", h, -2, 0, True),
             ("side 2", h, 2, 1, True), ("primal -1", h, -1, -1, True), ("primal 2", h, 0, 2, True)]
    for name, hh, side, primal, with_st in cases:
        for call in raw_calls(L, ws, hh, lam, side, primal, with_st):
            assert call[0] == E and untouched(call), name
    # finite gama: every multiplier is feasible, a transform is refused
    for gama in (0.625, 0.25 + rs.random_sample(m * n)):
        wg = ws_of(1, pr, gama=gama)
        for side in (0, 1):
            for call in raw_calls(L, wg, wg.handle, lam, side, 0):
                assert call[0] == L.IPD_E_UNSUPPORTED and untouched(call), side
        assert raw_calls(L, wg, wg.handle, lam, -1, 1)[0][0] == 0
        with pytest.raises(L.IpdError) as ei:
            wg.c_transform()
        assert ei.value.code == L.IPD_E_UNSUPPORTED
        assert wg.certificate()["side"] == -1
        wg.close()
    # a divider that is zero, negative or not finite: the side that divides by it is refused, at the first call and
    # at the next (the check is remembered), the other side and the evaluation are fine
    for bad in (0.0, -1.0, INF, np.nan):
        for side in (0, 1):
            pb = dict(pr)
            key = "q" if side == 0 else "p"
            pb[key] = pr[key].copy()
            pb[key][-2 if side else 3] = bad
            wb = ws_of(1, pb)
            for _ in range(2):
                for call in raw_calls(L, wb, wb.handle, lam, side, 0):
                    assert call[0] == E and untouched(call), (bad, side)
            assert raw_calls(L, wb, wb.handle, lam, -1, 0)[0][0] == 0
            if bad > 0 or bad < 0 or bad == 0:      # not NaN: the other side divides by good numbers
                assert raw_calls(L, wb, wb.handle, lam, 1 - side, 0)[0][0] == 0
            with pytest.raises(L.IpdError) as ei:
                wb.dual(lam, side=side)
            assert ei.value.code == E
            wb.close()
    # and the unedited call is fine
    for call in raw_calls(L, ws, h, lam, 0, 1):
        assert call[0] == 0 and not (call[1] == SENT).any() and not (call[2][:m] == -77).any()
        assert not (call[3] == SENT).any()
    ws.close()


# ---------------------------------------------------------------------------
# 9. driver keyword
# ---------------------------------------------------------------------------
def test_driver_keyword():
    m = n = 24
    pr = problem(1, m, n, seed=12)
    args = (pr["c"], pr["r"], pr["l"], pr["p"], pr["q"])
    plain = ipd().APD_SsN_Class1(*args, maxit=2)
    with_cert = ipd().APD_SsN_Class1(*args, maxit=2, certificate=True)
    assert set(with_cert) - set(plain) == {"certificate"} and "certificate" not in plain
    assert same_bits(plain["lk"], with_cert["lk"]) and same_bits(plain["xk"], with_cert["xk"])
    # an equal run, asked directly
    ws = ws_of(1, pr)
    ws.warmup(0.0, 100)
    ws.run(AMG1, ipd().MatlabRand(), prob=2, maxit=2)
    assert same_bits(ws.state()[2], plain["lk"])
    want = ws.certificate()
    ws.close()
    got = with_cert["certificate"]
    assert got.keys() == want.keys() and got["side"] in (0, 1)
    for key, val in want.items():
        assert np.array_equal(val, got[key]) if key in ("arg", "side") else same_bits(val, got[key]), key
    # finite gama: the evaluation of lk itself
    fin = ipd().APD_SsN_Class1(*args, gama=2.0, maxit=2, certificate=True)["certificate"]
    assert fin["side"] == -1 and "lam" not in fin and not np.isnan(fin["gap"])
    # the point-cloud drivers take the keyword too, stored and matrix-free alike
    rs = np.random.RandomState(15)
    xs, ys = rs.random_sample((m, 2)), rs.random_sample((n, 2))
    certs, mu = [], 0.65 * min(pr["r"].sum(), pr["l"].sum())
    for free in (False, True):
        out = ipd().APD_SsN_Class2_points(xs, ys, pr["r"], pr["l"], pr["p"], pr["q"], mu, maxit=1, matrix_free=free,
                                          certificate=True)
        certs.append(out["certificate"])
        assert certs[-1]["side"] in (0, 1) and certs[-1]["lam"].shape == (m + n + 1,)
    assert certs[0].keys() == certs[1].keys() and all(same_bits(certs[0][k], certs[1][k]) for k in certs[0])
    one = ipd().APD_SsN_Class1_points(xs, ys, pr["r"], pr["l"], pr["p"], pr["q"], maxit=1, certificate=True)
    assert one["certificate"]["side"] in (0, 1)
    assert "certificate" not in ipd().APD_SsN_Class1_points(xs, ys, pr["r"], pr["l"], pr["p"], pr["q"], maxit=1)
