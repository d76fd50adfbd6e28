"""The primal certificate on the device (csrc/ipd_round.hip: ipd_apd_round, ipd_apd_round_dev; APDWorkspace.round_plan,
round_plan_dev, bracket).

Reference: tests/round_ref.py, the header's twelve steps re-stated in numpy, operation by operation, in float64 and in
longdouble.  Where every sum is exact (pass A on dyadic inputs) the device is compared bit for bit; the rounded plan
is rebuilt in longdouble from the factors and scalars the device returned and the injected x, and its feasibility is
held to gamma(m+n+16)*(l_i + T/p_i) resp. (r_j + T/q_j), T = <p,l> + <q,r>, gamma(s) = s*u/(1 - s*u), u = 2^-53: the
any-order summation error of a2, b2, Se, Sf (DESIGN.md section 4h's argument).  States are injected with set_state;
only the bracket and the driver tests run the solver."""
import ctypes

import numpy as np
import pytest

from tests import round_ref as R

pytestmark = pytest.mark.gpu

INF = np.inf
LD = np.longdouble

# tests/test_gpu_dual.py's shapes
SHAPES = [(1, 1), (1, 37), (37, 1), (63, 17), (64, 16), (65, 33), (257, 19), (600, 45), (65, 150), (300, 16)]
STAT_KEYS = ("fval", "fs", "cc", "theta", "t", "se", "sf", "ms", "cp", "viol_in", "dropped", "ndropped", "ok")
VEC_KEYS = ("rho", "kappa", "e", "f")
SENT = -1234.5


def ipd():
    import codes_of_ipd_ssn_amg_method_amd as pkg
    return pkg


def lib_mod():
    from codes_of_ipd_ssn_amg_method_amd import _lib
    return _lib


def problem(cls, m, n, seed=1, pq_random=False):
    """tests/test_gpu_dual.py's problem(), re-stated: c,r,l ~ U(0,1) (draw order c,r,l), p=q=1, phi=1 unless
    pq_random."""
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


def same_result(a, b, keys=STAT_KEYS + VEC_KEYS):
    return all(same_bits(a[k], b[k]) for k in keys if k in a or k in b)


def inject(ws, Xd, rs, lam=None):
    """state with the x block of u = Xd(:), everything else random; returns (u, v, lam)."""
    u = rs.standard_normal(ws.U)
    u[:ws.m * ws.n] = Xd.reshape(-1, order="F")
    v = rs.standard_normal(ws.U)
    lam = rs.standard_normal(ws.L) if lam is None else lam
    ws.set_state(u, v, lam, 0.37)
    return u, v, lam


def base_plan(cls, pr, m, n):
    """outer(l, r) scaled to the right mass: class 1 its marginals are l and r, class 2 <phi, X> = mu"""
    X = np.outer(pr["l"], pr["r"])
    if cls == 1:
        return X / (pr["q"] @ pr["r"])
    return X * (pr["mu"] / (pr["phi"].reshape((m, n), order="F") * X).sum())


def noisy_plan(cls, pr, m, n, noise, rs, factor=1.0):
    """the base plan times 1 + noise*N(0,1), 10 % of the entries sign-flipped"""
    X = factor * base_plan(cls, pr, m, n) * (1.0 + noise * rs.standard_normal((m, n)))
    return np.where(rs.random_sample((m, n)) < 0.1, -X, X)


def x_out_of(ws, **kw):
    """(statistics, X^ (mn, column-major)) of round_plan_dev with an x_out buffer"""
    L = lib_mod()
    buf = L.DeviceBuffer.from_array(np.full(ws.m * ws.n, SENT))
    try:
        st = ws.round_plan_dev(x_out=buf, **kw)
        return st, buf.to_array(np.float64, ws.m * ws.n)
    finally:
        buf.free()


# ---------------------------------------------------------------------------
# 1. exact where exact
# ---------------------------------------------------------------------------
def dyadic_case(cls, m, n, seed):
    """x in multiples of 2^-10 below 4 (a third zero, NaNs planted), p, q in {0.5, 1, 2}; the callers choose l and r in
    multiples of 2^-11 around the first marginals: every sum of pass A is exact in any order"""
    rs = np.random.RandomState(seed)
    X = rs.randint(-4095, 4096, size=(m, n)) / 1024.0
    X[rs.random_sample((m, n)) < 0.33] = 0.0
    p, q = rs.choice([0.5, 1.0, 2.0], m), rs.choice([0.5, 1.0, 2.0], n)
    pr = dict(c=rs.random_sample(m * n), p=p, q=q)
    Xn = X.copy()
    Xn[rs.random_sample((m, n)) < 0.05] = np.nan
    Xn[m // 2, n // 2] = np.nan
    if cls == 2:
        pr.update(phi=0.5 + rs.random_sample(m * n))
    return pr, Xn, rs


@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", SHAPES)
def test_pass_a_bit_for_bit(cls, m, n):
    pr, X, rs = dyadic_case(cls, m, n, 17 * m + n + cls)
    for tol in (0.0, 0.375, 1e-9):
        Xp = R.clamp(X, tol)[0]
        a0, b0 = (pr["q"][None, :] * Xp).sum(axis=1), (pr["p"][:, None] * Xp).sum(axis=0)
        dl, dr = rs.randint(-64, 65, m) / 2048.0, rs.randint(-64, 65, n) / 2048.0
        dl[::2] = dr[::2] = 0.0                                         # every other one: a0_i == l_i, b0_j == r_j
        pr["l"], pr["r"] = np.maximum(a0 + dl, 0.0), np.maximum(b0 + dr, 0.0)
        if cls == 2:
            pr["mu"] = 0.5 * float((pr["phi"].reshape((m, n), order="F") * Xp).sum()) + 1.0
        ws = ws_of(cls, pr)
        u, _, _ = inject(ws, X, rs)
        assert np.isnan(u[:m * n]).any()
        for side in (0, 1):
            ref = R.round_ref(cls, pr, m, n, u, tol, side)
            assert same_bits(ref["a0"], a0) and same_bits(ref["b0"], b0)
            got = ws.round_plan(tol, side=side)
            what = (cls, m, n, tol, side)
            for key in ("viol_in", "dropped"):
                assert same_bits(got[key], ref[key]), (what, key, got[key], ref[key])
            assert (got["ndropped"], got["ok"]) == (ref["ndropped"], ref["ok"]), what
            first = "rho" if side == 0 else "kappa"
            assert same_bits(got[first], ref[first]), (what, first)
            marg, bound = (a0, pr["l"]) if side == 0 else (b0, pr["r"])
            assert (got[first][marg == bound] == 1.0).all() and (marg == bound).any()
            assert (got[first][marg > bound] < 1.0).all() and (got[first][marg < bound] == 1.0).all()
        ws.close()


@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", SHAPES)
def test_first_marginals_bit_for_bit(cls, m, n):
    """With l and r above every marginal both scale vectors are 1, X2 = x+, and the deficits e = l - a0, f = r - b0
    show a0 and b0 themselves: exact sums, so bit for bit in any order."""
    pr, X, rs = dyadic_case(cls, m, n, 19 * m + n + cls)
    Xp = R.clamp(X, 0.0)[0]
    a0, b0 = (pr["q"][None, :] * Xp).sum(axis=1), (pr["p"][:, None] * Xp).sum(axis=0)
    pr["l"], pr["r"] = a0 + rs.randint(0, 65, m) / 2048.0, b0 + rs.randint(0, 65, n) / 2048.0
    if cls == 2:
        pr["mu"] = float((pr["phi"].reshape((m, n), order="F") * Xp).sum()) + 1.0
    ws = ws_of(cls, pr)
    inject(ws, X, rs)
    for side in (0, 1):
        got = ws.round_plan(0.0, side=side)
        assert (got["rho"] == 1.0).all() and (got["kappa"] == 1.0).all()
        assert same_bits(got["e"], pr["l"] - a0) and same_bits(got["f"], pr["r"] - b0), (cls, m, n, side)
        want = 0.0 if cls == 2 else (pr["p"] * (pr["l"] - a0)).sum() + (pr["q"] * (pr["r"] - b0)).sum()   # exact sums
        assert got["viol_in"] == want, (cls, m, n, side)
    ws.close()


# ---------------------------------------------------------------------------
# 2. feasibility and value
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", SHAPES)
def test_rounded_plan_is_feasible(cls, m, n):
    worst = 0.0
    for pq_random in (False, True):
        pr = problem(cls, m, n, seed=3, pq_random=pq_random)
        ws = ws_of(cls, pr)
        for noise in (1e-6, 0.3):
            rs = np.random.RandomState(1000 * m + 10 * n + cls)
            u, _, _ = inject(ws, noisy_plan(cls, pr, m, n, noise, rs), rs)
            for side in (0, 1):
                what = "cls %d %dx%d pq %d noise %g side %d" % (cls, m, n, pq_random, noise, side)
                res = ws.round_plan(0.0, side=side)
                assert res["ok"] == 1, (what, res)
                Xh = R.rebuild(u, m, n, 0.0, res)
                used = R.check_feasible(cls, pr, m, n, Xh, what)
                print("%s: %.3f of the bound, viol_in %.3e" % (what, used, res["viol_in"]))
                worst = max(worst, used)
                R.check_values(cls, pr, m, n, u, 0.0, res, what)
                # the statistics are those of the restatement to the same kind of bound
                ref = R.round_ref(cls, pr, m, n, u, 0.0, side, ld=True)
                # (a marginal errs by gamma * its sum of |terms|, the weighted sum of the violations by gamma * itself)
                weight = float(pr["p"] @ ref["xp"] @ pr["q"])
                viol_bar = 2 * R.gamma(m + n + 16) * (2 * weight + float(pr["p"] @ pr["l"] + pr["q"] @ pr["r"]))
                assert abs(LD(res["viol_in"]) - ref["viol_in"]) <= viol_bar, (what, res["viol_in"], viol_bar)
                assert res["ndropped"] == ref["ndropped"]
                assert abs(LD(res["dropped"]) - ref["dropped"]) <= R.gamma(m * n + 16) * float(ref["dropped"])
        ws.close()
    print("worst fraction of the feasibility bound: %.3f" % worst)


@pytest.mark.parametrize("m,n", SHAPES)
def test_movement_bound(m, n):
    """Class 1, p = q = 1 (Altschuler, Weed, Rigollet, Lemma 7): |X^ - x+|_1 <= 2 viol_in and
    fval - <c, x+> <= 2 max(c) viol_in."""
    pr = problem(1, m, n, seed=5)
    ws = ws_of(1, pr)
    for noise in (1e-6, 0.3, 2.0):
        rs = np.random.RandomState(7 * m + n)
        u, _, _ = inject(ws, noisy_plan(1, pr, m, n, noise, rs), rs)
        xp = R.clamp(u[:m * n], 0.0)[0]
        for side in (0, 1):
            st, xh = x_out_of(ws, side=side)
            assert st["ok"] == 1
            moved = float(np.abs(xh.astype(LD) - xp.astype(LD)).sum())
            print("%dx%d noise %g side %d: moved %.3e of %.3e" % (m, n, noise, side, moved, 2 * st["viol_in"]))
            assert moved <= 2 * st["viol_in"] * (1 + 1e-12), (noise, side, moved, st["viol_in"])
            assert st["fval"] - float(pr["c"].astype(LD) @ xp.astype(LD)) <= 2 * pr["c"].max() * st["viol_in"]
            # x_out is the X^ of the factors
            res = ws.round_plan(0.0, side=side)
            Xh = R.rebuild(u, m, n, 0.0, res)
            assert np.abs(xh.reshape((m, n), order="F").astype(LD) - Xh).max() <= 4 * R.U * float(Xh.max())
    ws.close()


# ---------------------------------------------------------------------------
# 3. class 2: both branches, and no repair
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pq_random", [False, True])
@pytest.mark.parametrize("m,n", [(65, 33), (257, 19), (65, 150)])
def test_class2_branches(m, n, pq_random):
    pr = problem(2, m, n, seed=6, pq_random=pq_random)
    ws = ws_of(2, pr)
    rs = np.random.RandomState(m + n)
    for factor, shrink in ((1.5, True), (0.5, False)):
        u, _, _ = inject(ws, noisy_plan(2, pr, m, n, 1e-6, rs, factor=factor), rs)
        for side in (0, 1):
            res = ws.round_plan(0.0, side=side)
            what = "%dx%d factor %g side %d" % (m, n, factor, side)
            print(what, {k: res[k] for k in ("theta", "t", "ms", "cp", "se", "sf", "ok")})
            assert res["ok"] == 1, what
            if shrink:
                assert res["theta"] < 1.0 and res["t"] == 0.0 and res["ms"] >= pr["mu"], what
                assert bits([res["fval"]])[0] == bits([res["theta"] * res["fs"] + 0.0 * res["cc"]])[0]
            else:
                assert res["theta"] == 1.0 and res["t"] > 0.0 and res["ms"] < pr["mu"], what
                assert res["t"] * res["se"] <= 1.0 and res["t"] * res["sf"] <= 1.0
            R.check_feasible(2, pr, m, n, R.rebuild(u, m, n, 0.0, res), what)
            R.check_values(2, pr, m, n, u, 0.0, res, what)
    ws.close()


@pytest.mark.parametrize("m,n", [(65, 33), (300, 16)])
def test_class2_without_a_repair(m, n):
    """mu above what the slacks admit: t*Se > 1, ok = 0.  install = 0 reports it; install = 1 is refused with
    IPD_E_NUMERIC and the state keeps its bits."""
    L = lib_mod()
    pr = problem(2, m, n, seed=6, pq_random=True)
    pr["mu"] = 4.0 * float((pr["phi"].reshape((m, n), order="F") * np.outer(pr["l"], pr["r"])).sum()) + 10.0
    ws = ws_of(2, pr)
    rs = np.random.RandomState(3)
    X = 0.5 * np.outer(pr["l"], pr["r"]) / max(pr["q"] @ pr["r"], pr["p"] @ pr["l"])
    inject(ws, np.where(rs.random_sample((m, n)) < 0.1, -X, X), rs)
    before = ws.state()
    for side in (0, 1):
        res = ws.round_plan(0.0, side=side)
        assert res["ok"] == 0 and res["theta"] == 1.0 and res["t"] * min(res["se"], res["sf"]) > 1.0, res
        with pytest.raises(L.IpdError) as ei:
            ws.round_plan(0.0, side=side, install=True)
        assert ei.value.code == L.IPD_E_NUMERIC
        buf = L.DeviceBuffer.from_array(np.full(m * n, SENT))
        with pytest.raises(L.IpdError) as ei:
            ws.round_plan_dev(0.0, side=side, install=True, x_out=buf)
        assert ei.value.code == L.IPD_E_NUMERIC and (buf.to_array(np.float64, m * n) == SENT).all()
        buf.free()
        after = ws.state()
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before[:3], after[:3])) and before[3] == after[3]
    ws.close()


# ---------------------------------------------------------------------------
# 4. against the linear program
# ---------------------------------------------------------------------------
AMG1 = dict(retol=1e-11, bigph=1, maxit=30, theta=1 / 4, smoth=5, cycle="w", isnsp=1, inter=1, guess=None)
AMG2 = dict(retol=1e-11, bigph=1, maxit=40, theta=1 / 4, smoth=10, cycle="w", isnsp=1, inter=1, guess=None)


def optimum(cls, pr, m, n):
    """(f*, x*) of the linear program, by HiGHS on the CPU: min <c,x>, [X'p; Xq] (+ [y; z]) = [r; l], (<phi,x> = mu,)
    x (, y, z) >= 0 -- tests/test_gpu_dual.py's, re-stated"""
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
    return float(res.fun), np.asarray(res.x[:m * n])


@pytest.mark.parametrize("pq_random", [False, True])
@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", [(24, 24), (37, 29)])
def test_against_the_linear_program(cls, m, n, pq_random):
    pr = problem(cls, m, n, seed=12, pq_random=pq_random)
    fstar, xstar = optimum(cls, pr, m, n)
    ws = ws_of(cls, pr)
    rs = np.random.RandomState(21)
    for factor in (1.0, 1.001, 0.999):
        X = factor * xstar.reshape((m, n), order="F") + 1e-6 * rs.standard_normal((m, n))
        inject(ws, X, rs)
        for side in (0, 1):
            res = ws.round_plan(0.0, side=side, vectors=False)
            print("cls %d %dx%d pq %d factor %g side %d: fval - f* %.3e viol_in %.3e"
                  % (cls, m, n, pq_random, factor, side, res["fval"] - fstar, res["viol_in"]))
            assert res["ok"] == 1
            assert res["fval"] >= fstar - 1e-12 * abs(fstar), (factor, side, res["fval"], fstar)
            if cls == 1:
                assert res["fval"] - fstar <= 2 * pr["c"].max() * res["viol_in"], (factor, side, res, fstar)
    # the bracket of a short run
    ws.warmup(0.0, 40)
    ws.run(AMG1 if cls == 1 else AMG2, ipd().MatlabRand(), iters=2)
    br = ws.bracket()
    print("cls %d %dx%d pq %d: lower %.12g f* %.12g upper %.12g gap %.3e"
          % (cls, m, n, pq_random, br["lower"]["dual"], fstar, br["upper"]["fval"], br["gap"]))
    assert br["gap"] >= -1e-12 and br["gap"] == br["upper"]["fval"] - br["lower"]["dual"]
    assert br["lower"]["dual"] <= fstar <= br["upper"]["fval"], (br["lower"]["dual"], fstar, br["upper"]["fval"])
    both = [ws.round_plan(0.0, side=s) for s in (0, 1)]
    best = min((0, 1), key=lambda s: (not both[s]["ok"], both[s]["fval"]))
    assert br["upper"]["side"] == best and same_result(br["upper"], both[best])
    assert same_bits(br["lower"]["dual"], ws.certificate()["dual"])
    ws.close()


# ---------------------------------------------------------------------------
# 5. install
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pq_random", [False, True])
@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", [(65, 150), (300, 16), (257, 19)])
def test_install(cls, m, n, pq_random):
    pr = problem(cls, m, n, seed=9, pq_random=pq_random)
    ws = ws_of(cls, pr)
    rs = np.random.RandomState(m * n + cls)
    mn = m * n
    for side in (0, 1):
        u, v, lam = inject(ws, noisy_plan(cls, pr, m, n, 0.3, rs), rs)
        hist, recs = ws.history(), ws.records()
        st0, xh = x_out_of(ws, side=side)
        st, xo = x_out_of(ws, side=side, install=True)
        assert same_result(st0, st) and same_bits(xh, xo) and st["ok"] == 1
        u1, v1, lam1, bk1 = ws.state()
        assert same_bits(u1[:mn], xh) and same_bits(v1[:mn], xh)
        assert same_bits(lam1, lam) and bk1 == 0.37
        h1 = ws.history()
        assert h1.keys() == hist.keys() and all(same_bits(h1[k], hist[k]) for k in hist)
        assert len(ws.records()) == len(recs)
        Xh = xh.reshape((m, n), order="F").astype(LD)
        rb, cb = R.feasibility_bounds(pr, m, n)
        if cls == 2:
            y, z = u1[mn:mn + n], u1[mn + n:]
            assert same_bits(v1[mn:mn + n], y) and same_bits(v1[mn + n:], z)
            R.check_feasible(2, pr, m, n, Xh, "installed", yz=(y, z))
            # y^, z^ of the header: the slacks of the marginals of X^, to the bounds
            wy, wz = R.slacks(2, pr, m, n, Xh, st)
            assert (np.abs(y - wy) <= cb).all() and (np.abs(z - wz) <= rb).all()
        else:
            assert same_bits(u1[mn:], u[mn:]) and same_bits(v1[mn:], v[mn:])       # (nothing behind the x block)
            R.check_feasible(1, pr, m, n, Xh, "installed")
        # KKT_lk = |A u - b| / (1 + |b|) of the installed state is within the norm of the feasibility bound
        e = ws.end(lam, from_w=False)
        b = np.concatenate([pr["r"], pr["l"]] + ([[pr["mu"]]] if cls == 2 else []))
        bound = np.concatenate([cb, rb] + ([[4 * R.gamma(m + n + 16) * pr["mu"]]] if cls == 2 else []))
        print("cls %d %dx%d side %d: KKT_lk %.3e, bound %.3e" % (cls, m, n, side, e["kkt"][1], np.linalg.norm(bound)))
        assert e["kkt"][1] <= np.linalg.norm(bound)
        _, _, ax = ws.plan(0.0, stats=True)
        cols, rows = ax[:n] - pr["r"], ax[n:] - pr["l"]
        if cls == 1:
            assert (np.abs(cols) <= cb).all() and (np.abs(rows) <= rb).all()
        else:
            assert (cols <= cb).all() and (rows <= rb).all()
        # a second rounding finds nothing to do: viol_in is the weighted sum of marginal errors, each within its
        # bound, and the rank-one term is at rounding level.  Class 2: t*Se <= 1e-12.  Class 1 has t = 1/Se by
        # definition, so t*Se is 1 whenever Se > 0; there the term's mass t*Se*Sf = Sf (and Se) is held to 1e-12*T.
        again = ws.round_plan(0.0, side=side)
        total = float(pr["p"] @ pr["l"] + pr["q"] @ pr["r"])
        print("again: viol_in %.3e t %.3e Se %.3e Sf %.3e" % (again["viol_in"], again["t"], again["se"], again["sf"]))
        assert again["ok"] == 1 and again["viol_in"] <= float(pr["p"] @ rb + pr["q"] @ cb)
        if cls == 2:
            assert again["t"] * again["se"] <= 1e-12
        else:
            assert again["se"] <= 1e-12 * total and again["sf"] <= 1e-12 * total
    ws.close()


@pytest.mark.parametrize("cls", [1, 2])
def test_install_after_a_run_keeps_the_script(cls):
    """After a short run (histories and records are not empty) install changes the iterate only."""
    m, n = 24, 24
    pr = problem(cls, m, n, seed=12)
    ws = ws_of(cls, pr)
    ws.warmup(0.0, 40)
    ws.run(AMG1 if cls == 1 else AMG2, ipd().MatlabRand(), iters=2)
    u, v, lam, bk = ws.state()
    hist, recs = ws.history(), ws.records()
    assert len(recs) > 0 and all(len(h) > 0 for h in hist.values())
    st, xh = x_out_of(ws, side=0, install=True)
    u1, v1, lam1, bk1 = ws.state()
    assert st["ok"] == 1 and same_bits(u1[:m * n], xh) and same_bits(v1[:m * n], xh) and not same_bits(u[:m * n], xh)
    assert same_bits(lam1, lam) and bk1 == bk and repr(ws.records()) == repr(recs)
    h1 = ws.history()
    assert h1.keys() == hist.keys() and all(same_bits(h1[k], hist[k]) for k in hist)
    ws.close()


# ---------------------------------------------------------------------------
# 6. same bits
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


@pytest.mark.parametrize("cls", [1, 2])
def test_calls_agree(cls):
    """Two calls, the host and the device entry, vectors NULL and given: the same bits; install = 0 leaves the whole
    state as it was."""
    L = lib_mod()
    m, n = 600, 150
    pr = problem(cls, m, n, seed=7, pq_random=True)
    ws = ws_of(cls, pr)
    rs = np.random.RandomState(9)
    inject(ws, noisy_plan(cls, pr, m, n, 0.3, rs), rs)
    before = ws.state()
    for side in (0, 1):
        for tol in (0.0, 1e-4):
            a = ws.round_plan(tol, side=side)
            b = ws.round_plan(tol, side=side)
            assert same_result(a, b)
            assert same_result(a, ws.round_plan(tol, side=side, vectors=False), STAT_KEYS)
            sizes = dict(rho=m, kappa=n, e=m, f=n)
            bufs = {k: L.DeviceBuffer.from_array(np.full(sizes[k], SENT)) for k in VEC_KEYS}
            xo = L.DeviceBuffer.from_array(np.full(m * n, SENT))
            c = ws.round_plan_dev(tol, side=side, x_out=xo, **bufs)
            assert same_result(a, c, STAT_KEYS)
            for k in VEC_KEYS:
                assert same_bits(bufs[k].to_array(np.float64, sizes[k]), a[k]), k
            assert same_result(a, ws.round_plan_dev(tol, side=side), STAT_KEYS)          # every pointer NULL
            assert same_result(a, ws.round_plan_dev(tol, side=side, e=bufs["e"]), STAT_KEYS)
            x1 = xo.to_array(np.float64, m * n)
            assert not (x1 == SENT).any()
            assert same_bits(x1, x_out_of(ws, tol=tol, side=side)[1])
            for buf in list(bufs.values()) + [xo]:
                buf.free()
    after = ws.state()
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(before[:3], after[:3])) and before[3] == after[3]
    # tensors and (pointer, entries) pairs
    t_rho, t_f = Tensor(np.full(m, SENT)), Tensor(np.full(n, SENT))
    a = ws.round_plan(0.0, side=0)
    assert same_result(a, ws.round_plan_dev(0.0, side=0, rho=t_rho, f=(t_f.data_ptr(), n)), STAT_KEYS)
    assert same_bits(t_rho.numpy(), a["rho"]) and same_bits(t_f.numpy(), a["f"])
    with pytest.raises(ValueError):
        ws.round_plan_dev(rho=(t_rho.data_ptr(), m - 1))
    with pytest.raises(ValueError):
        ws.round_plan_dev(x_out=t_rho)
    with pytest.raises(ValueError):
        ws.round_plan_dev(kappa=Tensor(np.zeros(n), np.float32))
    with pytest.raises(ValueError):
        ws.round_plan(side=2)
    with pytest.raises(ValueError):
        ws.round_plan(tol=-1.0)
    ws.close()


@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_cost_sources_agree(cls, d):
    m, n = 65, 150
    rs = np.random.RandomState(40 + d)
    xs, ys = rs.random_sample((m, d)), rs.random_sample((n, d))
    r, l = rs.random_sample(n), rs.random_sample(m)
    p, q = 0.5 + rs.random_sample(m), 0.5 + rs.random_sample(n)
    kw = dict(mu=0.65 * min(r.sum(), l.sum()), phi=0.5 + rs.random_sample(m * n)) if cls == 2 else {}
    pr = dict(r=r, l=l, p=p, q=q, **kw)
    if cls == 1:
        pr["l"] = l = l * (r @ q) / (l @ p)
    Xd = noisy_plan(cls, pr, m, n, 0.3, rs)
    for metric in ("sqeuclidean", "cityblock"):
        for scale in (False, True):
            stored = ipd().APDWorkspace.from_points(cls, xs, ys, r, l, p, q, metric=metric, scale=scale, **kw)
            free = ipd().APDWorkspace.from_points(cls, xs, ys, r, l, p, q, metric=metric, scale=scale,
                                                  matrix_free=True, **kw)
            assert (stored.cost_info()["form"], free.cost_info()["form"]) == (0, 1)
            host = ipd().APDWorkspace(cls, stored.cost().reshape(-1, order="F"), r, l, p, q, **kw)
            for ws in (host, stored, free):
                inject(ws, Xd, np.random.RandomState(5))
            for side in (0, 1):
                got = [ws.round_plan(0.0, side=side) for ws in (host, stored, free)]
                outs = [x_out_of(ws, side=side)[1] for ws in (host, stored, free)]
                for other, xo in zip(got[1:], outs[1:]):
                    assert same_result(got[0], other), (metric, scale, side)
                    assert same_bits(outs[0], xo)
                assert got[0]["ok"] == 1 and got[0]["cc"] > 0
            for ws in (host, stored, free):
                ws.close()


# ---------------------------------------------------------------------------
# 7. errors
# ---------------------------------------------------------------------------
def raw_calls(L, ws, h, tol, side, install, with_st=True):
    """both entries on pre-filled outputs -> [(rc, [rho, kappa, e, f(, x_out)], stats bytes)]"""
    lib = L.lib
    m, n = ws.m, ws.n
    sizes = (m, n, m, n)
    out = []
    st = (ctypes.c_double * 13)(*([SENT] * 13))
    vec = [np.full(k, SENT) for k in sizes]
    rc = lib.ipd_apd_round(h, tol, side, install, *[v.ctypes.data for v in vec],
                           ctypes.addressof(st) if with_st else None)
    out.append((rc, vec, np.array(st)))
    st = (ctypes.c_double * 13)(*([SENT] * 13))
    dev = [L.DeviceBuffer.from_array(np.full(k, SENT)) for k in sizes + (m * n,)]
    rc = lib.ipd_apd_round_dev(h, tol, side, install, *[d.ptr for d in dev], ctypes.addressof(st) if with_st else None)
    out.append((rc, [d.to_array(np.float64, k) for d, k in zip(dev, sizes + (m * n,))], np.array(st)))
    for d in dev:
        d.free()
    return out


def untouched(call):
    rc, vec, st = call
    return all((v == SENT).all() for v in vec) and (st == SENT).all()


def test_argument_errors_write_nothing():
    L = lib_mod()
    assert ctypes.sizeof(L.ipd_round_stats) == 13 * 8
    m, n = 37, 5
    pr = problem(1, m, n, seed=13)
    ws = ws_of(1, pr)
    rs = np.random.RandomState(14)
    inject(ws, noisy_plan(1, pr, m, n, 0.3, rs), rs)
    before = ws.state()
    h, E = ws.handle, L.IPD_E_ARG
    cases = [("NULL h", None, 0.0, 0, 0, True), ("NULL st", h, 0.0, 0, 0, False), ("side -1", h, 0.0, -1, 0, True),
             ("side 2", h, 0.0, 2, 1, True), ("install -1", h, 0.0, 0, -1, True), ("install 2", h, 0.0, 1, 2, True),
             ("tol < 0", h, -1e-300, 0, 1, True), ("tol NaN", h, np.nan, 1, 0, True)]
    for name, hh, tol, side, install, with_st in cases:
        for call in raw_calls(L, ws, hh, tol, side, install, with_st):
            assert call[0] == E and untouched(call), name
    after = ws.state()
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before[:3], after[:3]))
    # finite gama, scalar and vector: the rank-one term does not keep x <= gama
    for gama in (0.625, 0.25 + rs.random_sample(m * n)):
        wg = ws_of(1, pr, gama=gama)
        inject(wg, noisy_plan(1, pr, m, n, 0.3, rs), rs)
        for side in (0, 1):
            for install in (0, 1):
                for call in raw_calls(L, wg, wg.handle, 0.0, side, install):
                    assert call[0] == L.IPD_E_UNSUPPORTED and untouched(call), (side, install)
        with pytest.raises(L.IpdError) as ei:
            wg.round_plan()
        assert ei.value.code == L.IPD_E_UNSUPPORTED
        with pytest.raises(ValueError):
            wg.bracket()
        wg.close()
    # and the unedited call is fine
    for call in raw_calls(L, ws, h, 0.0, 0, 0):
        assert call[0] == 0 and not any((v == SENT).any() for v in call[1]) and not (call[2] == SENT).any()
    ws.close()


# ---------------------------------------------------------------------------
# 8. driver keyword
# ---------------------------------------------------------------------------
def test_driver_keyword():
    m = n = 24
    pr = problem(1, m, n, seed=12)
    args = (pr["c"], pr["r"], pr["l"], pr["p"], pr["q"])
    plain = ipd().APD_SsN_Class1(*args, maxit=2)
    with_br = ipd().APD_SsN_Class1(*args, maxit=2, bracket=True)
    assert set(with_br) - set(plain) == {"bracket"} and "bracket" not in plain
    assert same_bits(plain["lk"], with_br["lk"]) and same_bits(plain["xk"], with_br["xk"])
    # an equal run, asked directly
    ws = ws_of(1, pr)
    ws.warmup(0.0, 100)
    ws.run(AMG1, ipd().MatlabRand(), prob=2, maxit=2)
    assert same_bits(ws.state()[2], plain["lk"])
    want = ws.bracket()
    ws.close()
    got = with_br["bracket"]
    assert got.keys() == want.keys() == {"lower", "upper", "gap"} and same_bits(got["gap"], want["gap"])
    assert same_result(got["upper"], want["upper"]) and got["upper"]["side"] == want["upper"]["side"]
    assert same_bits(got["lower"]["dual"], want["lower"]["dual"]) and got["gap"] >= -1e-12
    with pytest.raises(ValueError):
        ipd().APD_SsN_Class1(*args, gama=2.0, maxit=1, bracket=True)
    pr2 = problem(2, m, n, seed=12)
    two = ipd().APD_SsN_Class2(pr2["c"], pr2["r"], pr2["l"], pr2["p"], pr2["q"], pr2["mu"], pr2["phi"], maxit=1,
                               bracket=True)
    assert two["bracket"]["upper"]["ok"] == 1 and two["bracket"]["gap"] >= -1e-12
    # the point-cloud drivers take the keyword too, stored and matrix-free alike
    rs = np.random.RandomState(15)
    xs, ys = rs.random_sample((m, 2)), rs.random_sample((n, 2))
    mu = 0.65 * min(pr["r"].sum(), pr["l"].sum())
    outs = []
    for free in (False, True):
        out = ipd().APD_SsN_Class2_points(xs, ys, pr["r"], pr["l"], pr["p"], pr["q"], mu, maxit=1, matrix_free=free,
                                          bracket=True)
        outs.append(out["bracket"])
        assert outs[-1]["upper"]["ok"] == 1 and outs[-1]["gap"] >= -1e-12
    assert same_result(outs[0]["upper"], outs[1]["upper"]) and same_bits(outs[0]["gap"], outs[1]["gap"])
    one = ipd().APD_SsN_Class1_points(xs, ys, pr["r"], pr["l"], pr["p"], pr["q"], maxit=1, bracket=True)
    assert one["bracket"]["upper"]["ok"] == 1 and one["bracket"]["gap"] >= -1e-12
    assert "bracket" not in ipd().APD_SsN_Class1_points(xs, ys, pr["r"], pr["l"], pr["p"], pr["q"], maxit=1)
