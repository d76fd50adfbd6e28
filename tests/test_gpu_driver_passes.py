"""Every mn-sized pass of the APD / semismooth-Newton drivers (csrc/ipd_driver.hip: the tile walker k_tiles with
OpBegin, OpEvalT, OpMerit, OpEnd and their epilogues) at the geometry edges of the walker, through the
building-block entries ipd_apd_begin / get_w / eval / eval_trial / merit / end.

Reference rule.  Every elementwise quantity (wk, zk, prox, the mask, uk1, vk1, each product that enters a sum) is
computed in fp64 numpy in the kernel's written operation order: the unit is built without contraction, so these are
bit-equal and wk, s, t, uk1, vk1, lam_out and the count E are compared with array_equal.  Every reduction over
those values is computed in np.longdouble (64-bit significand).  A reduction of N terms t_i may differ from the
exact sum by at most gamma(N+4)*sum|t_i| with gamma(k) = k*u/(1-k*u), u = 2^-53: the bound of summation in ANY order
plus slack for the fixed combines.  A derived value (Fk, wlk, cFk, the merit, the KKT norms) gets the sum of its
inputs' bounds times their coefficients plus 4u times the sum of the absolute values of its addends; the square
root of a sum of squares carries the bound through sqrt.  Nothing here is measured.

Shapes (what each group reaches is in GROUPS below): a = wave / tile / column-chunk boundaries, b = row-side
sum_strided counts 32, 44, 48, c = column-side sum_strided, d = more than 512 workgroups, e = k_eval_fin's
global-memory fallback and its singled-out block, f = `reps` forced to 2, 4, 8 (IPD_APD_REPS; tests/test_apd_geo.py
ties that geometry to the natural rule), ties = comparisons that hold with equality."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import drivers as D          # noqa: E402

U53 = 2.0 ** -53
LD = np.longdouble
KB = ((1, 1.0), (7, 0.013))
STEPS = 0.9 ** np.arange(1, 9)
STEPS_ZERO = STEPS.copy()
STEPS_ZERO[3] = 0.0


def test_longdouble_is_wider_than_double():
    """The references' reductions are only 'exact' against fp64 if longdouble has the 64-bit significand."""
    assert np.finfo(LD).eps <= 2.0 ** -63


def ipd():
    import codes_of_ipd_ssn_amg_method_amd as pkg
    return pkg


def gam(k):
    return k * U53 / (1.0 - k * U53)


def red(terms, axis=None):
    """(exact sum, bound of a summation of these terms in any order)"""
    t = np.asarray(terms, dtype=LD)
    N = t.size if axis is None else t.shape[axis]
    return np.sum(t, axis=axis), gam(N + 4) * np.sum(np.abs(t), axis=axis)


def within(got, ref, tol, what):
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.max(np.where(err > 0, err / tol, 0))) if np.size(err) else 0.0
    print("%-12s %.3g of its bound" % (what, worst))
    assert np.all(err <= tol), "%s: %.3g times its bound" % (what, worst)


def within_sqrt(got, ref2, tol2, what):
    """got against sqrt(ref2), ref2 known to tol2"""
    r = np.sqrt(LD(ref2))
    tol = max(np.sqrt(LD(ref2) + tol2) - r, r - np.sqrt(max(LD(ref2) - tol2, LD(0)))) + 4 * U53 * r
    within(got, r, tol, what)


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
GROUPS = {
    "a": [(1, 1), (1, 17), (63, 16), (64, 15), (65, 33), (255, 31), (256, 32), (257, 1)],
    "b": [(1793, 17), (2561, 17), (2817, 17)],                       # 4*nib = 32, 44 = 32+8+4, 48 = 32+8+8
    "c": [(65, 16 * g - 5) for g in (7, 8, 9, 31, 32, 33, 43)],      # njg partials of a row
    "d": [(70, 8211), (300, 4099)],                                  # nib*njg = 514 > 512
}
VARIANTS = [(1, "scalar"), (1, "vector"), (1, "inf"), (2, None)]


class Case:
    def __init__(self, group, m, n, cls, gkind, reps=None, tie=None):
        self.group, self.m, self.n, self.cls, self.gkind, self.reps, self.tie = group, m, n, cls, gkind, reps, tie
        self.kb = KB[1:] if tie == "gama" else KB
        self.id = "%s-%dx%d-c%d%s%s%s" % (group, m, n, cls, gkind or "", "-r%d" % reps if reps else "",
                                           "-" + tie if tie else "")

    def __hash__(self):
        return hash(self.id)

    def __eq__(self, o):
        return self.id == o.id


def _cases():
    out = []
    for grp, shapes in GROUPS.items():
        out += [Case(grp, m, n, cls, gk) for m, n in shapes for cls, gk in VARIANTS]
    # e: 86 epilogue blocks (516 partials: the LDS copy holds 512), 4*nib = 172; M % 128 = 127, 0, 1
    out += [Case("e", 10900, 17, cls, gk) for cls, gk in VARIANTS]
    out += [Case("e", 100, n, 2, None) for n in (27, 28, 29)]
    # f: the last column group partly filled, chunks after the end of the columns
    out += [Case("f", m, n, cls, gk, reps=r) for m, n in [(300, 147), (65, 40), (257, 500)] for r in (2, 4, 8)
            for cls, gk in VARIANTS]
    out += [Case("ties", 65, 33, 1, "scalar", tie="zero"), Case("ties", 65, 33, 2, None, tie="zero"),
            Case("ties", 65, 33, 1, "vector", tie="gama"), Case("ties", 300, 147, 1, "vector", reps=4, tie="gama")]
    return out


CASES = _cases()
all_cases = pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])


class Inputs:
    pass


@functools.lru_cache(maxsize=None)
def inputs(case):
    """p, q in [0.5, 1.5]; u with about 70 % exact zeros, v = u + noise; lam, zeta random."""
    m, n, cls = case.m, case.n, case.cls
    rs = np.random.RandomState(10007 * m + 17 * n + cls)
    I = Inputs()
    I.m, I.n, I.cls, I.M, I.mn = m, n, cls, m + n, m * n
    I.L = I.M + (cls == 2)
    I.U = I.mn + (I.M if cls == 2 else 0)
    I.p, I.q = 0.5 + rs.random_sample(m), 0.5 + rs.random_sample(n)
    I.c, I.r, I.l = rs.random_sample(I.mn), rs.random_sample(n), rs.random_sample(m)
    I.phi = 0.5 + rs.random_sample(I.mn) if cls == 2 else None
    I.mu = 0.65 * min(I.r.sum(), I.l.sum()) if cls == 2 else 0.0
    I.b = np.concatenate([I.r, I.l] + ([[I.mu]] if cls == 2 else []))
    I.gama = {"scalar": 0.7, "vector": 0.2 + rs.random_sample(I.mn), "inf": np.inf, None: np.inf}[case.gkind]
    I.u = rs.random_sample(I.U) * (rs.random_sample(I.U) < 0.3)
    I.v = I.u + 0.1 * rs.standard_normal(I.U)
    I.lam = rs.standard_normal(I.L)
    I.lam_try = I.lam + 0.05 * rs.standard_normal(I.L)
    I.zeta = rs.standard_normal(I.L)
    I.Fold = rs.standard_normal(I.L)
    I.u_other = rs.random_sample(I.U) * (rs.random_sample(I.U) < 0.5)
    if case.tie == "zero":        # c = 0, u = v = 0, lam = 0: z = +0 everywhere, every entry is active
        I.c, I.u, I.v = np.zeros(I.mn), np.zeros(I.U), np.zeros(I.U)
        I.lam = I.lam_try = np.zeros(I.L)
    if case.tie == "gama":        # on a tenth of the entries gama is the reference's own zk: z <= g with equality
        (k, bk), = case.kb
        z = ref_eval(I, ref_begin(I, k, bk), None, I.lam_try)["z"].reshape(-1)
        hit = rs.random_sample(I.mn) < 0.1
        I.gama = np.where(hit, z, I.gama)
        I.tied = hit
    for a in vars(I).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return I


def workspace(case, monkeypatch, reps="case"):
    I = inputs(case)
    reps = case.reps if reps == "case" else reps
    if reps:
        monkeypatch.setenv("IPD_APD_REPS", str(reps))
    else:
        monkeypatch.delenv("IPD_APD_REPS", raising=False)
    if I.cls == 1:
        ws = ipd().APDWorkspace(1, I.c, I.r, I.l, I.p, I.q, gama=I.gama)
    else:
        ws = ipd().APDWorkspace(2, I.c, I.r, I.l, I.p, I.q, mu=I.mu, phi=I.phi)
    monkeypatch.delenv("IPD_APD_REPS", raising=False)      # read when the workspace is created
    return ws, I


# ---------------------------------------------------------------------------------------------------------------
# the references: x(i,j) = x[i + j*m] is X[j, i] below
# ---------------------------------------------------------------------------------------------------------------
def mat(I, x):
    return x[:I.mn].reshape(I.n, I.m)


def ax_red(I, X):
    """Ax = [sum_i p_i x_ij (n entries); sum_j q_j x_ij (m entries)]: exact sums and their bounds.  The kernel
    forms x*p_i and x*q_j (k_tiles: `x * pi`, `x * cc.q`)."""
    Sc, Bc = red(X * I.p[None, :], axis=1)
    Sr, Br = red(X * I.q[:, None], axis=0)
    return np.concatenate([Sc, Sr]), np.concatenate([Bc, Br])


def prox(I, x):
    t = np.where(x > 0.0, x, 0.0)
    if I.cls == 2:
        return t
    g = I.gama if np.ndim(I.gama) == 0 else mat(I, I.gama)
    return np.where(t < g, t, g)


def aty_of(I, lt):
    """`rc.pi * cc.y1 + rc.y2 * cc.q`, class 2: `aty + lamL * phi`"""
    aty = I.p[None, :] * lt[:I.n, None] + lt[None, I.n:I.M] * I.q[:, None]
    if I.cls == 2:
        aty = aty + lt[I.M] * mat(I, I.phi)
    return aty


@functools.lru_cache(maxsize=None)
def _ref_begin_cached(case, k, bk):
    return ref_begin(inputs(case), k, bk)


def ref_begin(I, k, bk):
    """OpBegin / k_begin_fin: wk (bit-equal), wlk (exact, with its bound)."""
    R = Inputs()
    R.ak = math.sqrt(k * k * bk)
    R.bk, R.bk1, R.tk = bk, bk / (1.0 + R.ak), bk * (1.0 + R.ak) / (R.ak * R.ak)
    ak, ak2, ibk, bk1, mn, M = R.ak, R.ak * R.ak, 1.0 / bk, R.bk1, I.mn, I.M
    R.w = np.empty(I.U)
    R.w[:mn] = -I.c + bk * (I.u[:mn] + ak * I.v[:mn]) / ak2
    if I.cls == 2:
        R.w[mn:] = -0.0 + bk * (I.u[mn:] + ak * I.v[mn:]) / ak2
    S, B = ax_red(I, mat(I, I.u))
    add = np.abs(S)
    if I.cls == 2:
        S = S + I.u[mn:]
        add = add + np.abs(I.u[mn:])
        Sp, Bp = red(I.phi * I.u[:mn])
        S, B, add = np.append(S, Sp), np.append(B, Bp), np.append(add, np.abs(Sp))
    R.wlk = bk1 * (I.lam - ibk * (S - I.b)) - I.b
    R.wlk_tol = bk1 * ibk * B + 4 * U53 * (np.abs(bk1 * I.lam) + bk1 * ibk * (add + np.abs(I.b)) + np.abs(I.b))
    return R


def ref_eval(I, R, wlk_dev, lam, zeta=None, step=0.0, Fold=None, m3=False, merit_only=False):
    """OpEvalT / k_eval_fin at lam + step*zeta.  wlk_dev = None: only z; merit_only: without Fk (OpMerit /
    k_merit_fin form the same sums operation for operation)."""
    mn, M, cls2 = I.mn, I.M, I.cls == 2
    bk1, tk, itk = R.bk1, R.tk, 1.0 / R.tk
    lt = lam + step * zeta if zeta is not None else lam
    z = itk * (mat(I, R.w) - aty_of(I, lt))
    if wlk_dev is None:
        return dict(z=z)
    px = prox(I, z)
    g = I.gama if np.ndim(I.gama) == 0 else mat(I, I.gama)
    act = (z >= 0.0) if cls2 else ((z >= 0.0) & (z <= g))
    out = dict(lam_out=lt, s=act.reshape(-1), E=int(act.sum()), t=None)
    tails = np.zeros(0)
    if cls2:
        zt = itk * (R.w[mn:] - lt[:M])
        pz = np.where(zt > 0.0, zt, 0.0)
        out["t"] = zt >= 0.0
        tails = pz * pz
        out["z2"] = red(zt * zt)
    if not merit_only:
        S, B = ax_red(I, px)
        add = np.abs(S)
        if cls2:
            Sp, Bp = red(mat(I, I.phi) * px)
            S, B, add = np.append(S + pz, Sp), np.append(B, Bp), np.append(add + pz, np.abs(Sp))
        out["F"] = bk1 * lt - S - wlk_dev
        out["F_tol"] = B + 4 * U53 * (np.abs(bk1 * lt) + add + np.abs(wlk_dev))
    out["lam2"] = red(lt * lt)
    out["wlk_lam"] = red(wlk_dev * lt)
    out["fold_zeta"] = red(Fold * zeta) if (zeta is not None and Fold is not None) else (LD(0), LD(0))
    out["prox2"] = red(np.concatenate([(px * px).reshape(-1), tails]))
    if m3:
        out["z2"] = red(z * z)
        out["zmp2"] = red((z - px) * (z - px))
    out.setdefault("z2", (LD(0), LD(0)))
    out.setdefault("zmp2", (LD(0), LD(0)))
    h = bk1 / 2.0
    (l2, bl2), (wl, bwl) = out["lam2"], out["wlk_lam"]
    if m3:      # :183-187  f0 + tk/2*(|zk|^2 - |zk - prox(zk)|^2)
        (a, ba), (c, bc) = out["z2"], out["zmp2"]
        out["cF"] = h * l2 - wl + 0.5 * tk * (a - c)
        out["cF_tol"] = h * bl2 + bwl + 0.5 * tk * (ba + bc) + 4 * U53 * (h * l2 + abs(wl) + 0.5 * tk * (a + c))
    else:
        a, ba = out["prox2"]
        out["cF"] = h * l2 - wl + 0.5 * tk * a
        out["cF_tol"] = h * bl2 + bwl + 0.5 * tk * ba + 4 * U53 * (h * l2 + abs(wl) + 0.5 * tk * a)
    return out


def check_eval(I, got, ref, what):
    assert np.array_equal(got["s"], ref["s"]), what + ": active-set mask"
    if I.cls == 2:
        assert np.array_equal(got["t"], ref["t"]), what + ": t"
    assert got["E"] == ref["E"]
    within(got["Fk"], ref["F"], ref["F_tol"], what + " Fk")
    f2, b2 = red(got["Fk"] * got["Fk"])
    within_sqrt(got["Fk_norm"], f2, b2, what + " |Fk|")
    within(got["cFk"], ref["cF"], ref["cF_tol"], what + " cFk")


def ref_end(I, R, lam, from_w, u):
    """OpEnd<from_w> / k_end_fin at the multiplier lam: uk1, vk1 (bit-equal), the KKT sums and fx."""
    mn, M, n, cls2 = I.mn, I.M, I.n, I.cls == 2
    itk, ak = 1.0 / R.tk, R.ak
    aty = aty_of(I, lam)
    C, Uo = mat(I, I.c), mat(I, u)
    out = {}
    if from_w:
        u1 = prox(I, itk * (mat(I, R.w) - aty))
        v1 = u1 + (u1 - Uo) / ak
    else:
        u1 = Uo
    d = u1 - prox(I, u1 - C - aty)
    out["kx2"] = red(d * d)
    out["fx"] = red(C * u1)
    S, B = ax_red(I, u1)
    add = np.abs(S)
    out["ky2"] = out["kz2"] = (LD(0), LD(0))
    unew, vnew = u1.reshape(-1), (v1.reshape(-1) if from_w else None)
    if cls2:
        lt, ut = lam[:M], u[mn:]
        if from_w:
            zt = itk * (R.w[mn:] - lt)
            pz = np.where(zt > 0.0, zt, 0.0)
            vnew = np.concatenate([vnew, pz + (pz - ut) / ak])
            ut = pz
        unew = np.concatenate([unew, ut])
        sh = ut - lt
        dd = ut - np.where(sh > 0.0, sh, 0.0)
        out["ky2"], out["kz2"] = red(dd[:n] * dd[:n]), red(dd[n:] * dd[n:])
        Sp, Bp = red(mat(I, I.phi) * u1)
        S, B, add = np.append(S + ut, Sp), np.append(B, Bp), np.append(add + np.abs(ut), np.abs(Sp))
    # kl2 = sum e_t^2 with e_t = Hu_t - b_t formed from the device's own (inexact) Hu
    e = S - I.b
    e_tol = B + 4 * U53 * (add + np.abs(I.b))
    s2, b2 = red(e * e)
    hi = np.abs(e) + e_tol
    out["kl2"] = (s2, np.sum(2 * np.abs(e) * e_tol + e_tol * e_tol) + gam(e.size + 4) * np.sum(hi * hi) + 4 * U53 * s2)
    out["u"], out["v"] = unew, vnew
    return out


def check_end(got, ref, what):
    for k, name in enumerate(("kx2", "kl2", "ky2", "kz2")):
        within_sqrt(got["kkt"][k], ref[name][0], ref[name][1], what + " sqrt(%s)" % name)
    within(got["fx"], ref["fx"][0], ref["fx"][1], what + " fx")


def begin_checked(ws, case, I, k, bk):
    """set_state + begin; wk bit-equal, wlk within its bound; returns the reference and the device's wlk"""
    R = _ref_begin_cached(case, k, bk)
    ws.set_state(I.u, I.v, I.lam, bk)
    got = ws.begin(k)
    assert (got["ak"], got["bk1"], got["tk"]) == (R.ak, R.bk1, R.tk)
    w, wlk = ws.get_w()
    assert np.array_equal(w, R.w) and np.array_equal(np.signbit(w), np.signbit(R.w)), "wk"
    within(wlk, R.wlk, R.wlk_tol, "wlk")
    return R, wlk


# ---------------------------------------------------------------------------------------------------------------
# the passes
# ---------------------------------------------------------------------------------------------------------------
@all_cases
def test_begin_and_eval(case, monkeypatch):
    ws, I = workspace(case, monkeypatch)
    try:
        for k, bk in case.kb:
            R, wlk = begin_checked(ws, case, I, k, bk)
            ref = ref_eval(I, R, wlk, I.lam_try)
            check_eval(I, ws.eval(I.lam_try), ref, "eval")
            if case.tie == "zero":
                assert ref["E"] == I.mn and (I.cls == 1 or ref["t"].all())
            if case.tie == "gama":
                z, g = ref_eval(I, R, None, I.lam_try)["z"].reshape(-1), I.gama
                assert np.array_equal(z[I.tied], g[I.tied]) and ref["s"][I.tied & (z >= 0)].all()
    finally:
        ws.close()


@all_cases
def test_eval_at_a_trial_point(case, monkeypatch):
    """Lam with zeta and step, the fold_zeta reduction, lam_out, the raw sums, and (class 1) the M3 instantiations."""
    ws, I = workspace(case, monkeypatch)
    try:
        for k, bk in case.kb:
            R, wlk = begin_checked(ws, case, I, k, bk)
            trials = [(False, 0.81, I.Fold), (False, 0.0, None)] + ([(True, 0.81, I.Fold)] if I.cls == 1 else [])
            for m3, step, Fold in trials:
                what = "trial m3=%d step=%g" % (m3, step)
                ref = ref_eval(I, R, wlk, I.lam, I.zeta, step, Fold, m3)
                got = ws.eval_trial(I.lam, I.zeta, step, Fold, merit3=m3)
                assert np.array_equal(got["lam_out"], ref["lam_out"]), what + ": lam_out"
                check_eval(I, got, ref, what)
                for name in ("lam2", "wlk_lam", "prox2", "z2", "zmp2", "fold_zeta"):
                    within(got[name], ref[name][0], ref[name][1], what + " " + name)
            # without a direction it is `eval`
            a, b = ws.eval_trial(I.lam_try), ws.eval(I.lam_try)
            assert np.array_equal(a["s"], b["s"]) and np.array_equal(a["Fk"], b["Fk"]) and a["cFk"] == b["cFk"]
            assert np.array_equal(a["lam_out"], I.lam_try)
    finally:
        ws.close()


@all_cases
def test_merit_pass(case, monkeypatch):
    """OpMerit / k_merit_fin: eight Armijo trial points per pass, each against the reference and against the
    trial-point eval's own cFk at that step; no slot repeats its neighbour unless the reference does."""
    ws, I = workspace(case, monkeypatch)
    try:
        for (k, bk), steps in zip(case.kb, (STEPS, STEPS_ZERO)[-len(case.kb):]):
            R, wlk = begin_checked(ws, case, I, k, bk)
            got = ws.merit(I.lam, I.zeta, steps)
            refs = [ref_eval(I, R, wlk, I.lam, I.zeta, st, merit_only=True) for st in steps]
            for j, st in enumerate(steps):
                within(got[j], refs[j]["cF"], refs[j]["cF_tol"], "merit[%d]" % j)
                ev = ws.eval_trial(I.lam, I.zeta, st)
                within(got[j], LD(ev["cFk"]), 2 * refs[j]["cF_tol"], "merit[%d] against eval" % j)
            for j in range(7):
                if refs[j]["cF"] != refs[j + 1]["cF"]:
                    assert got[j] != got[j + 1], "slots %d and %d repeat" % (j, j + 1)
    finally:
        ws.close()


@all_cases
def test_end_pass(case, monkeypatch):
    """OpEnd<true> (uk1, vk1 readable through state()), OpEnd<false> on a given iterate and on the state."""
    ws, I = workspace(case, monkeypatch)
    try:
        for k, bk in case.kb:
            R, _ = begin_checked(ws, case, I, k, bk)
            ref = ref_end(I, R, I.lam_try, True, I.u)
            check_end(ws.end(I.lam_try, from_w=True), ref, "end from_w")
            u, v, lam, _ = ws.state()
            assert np.array_equal(u, ref["u"]) and np.array_equal(v, ref["v"]) and np.array_equal(lam, I.lam_try)
            check_end(ws.end(I.lam_try, from_w=False), ref, "end of the state")          # measures (uk1, lam) again
            check_end(ws.end(I.lam, from_w=False, u=I.u_other), ref_end(I, R, I.lam, False, I.u_other), "end of u")
            assert np.array_equal(ws.state()[0], ref["u"]), "from_w = 0 changes nothing"
    finally:
        ws.close()


# ---------------------------------------------------------------------------------------------------------------
# the forced geometry against the natural one
# ---------------------------------------------------------------------------------------------------------------
F_CASES = [c for c in CASES if c.group == "f"]


def elementwise_outputs(ws, I, k, bk):
    ws.set_state(I.u, I.v, I.lam, bk)
    ws.begin(k)
    out = [ws.get_w()[0]]
    ev = ws.eval_trial(I.lam, I.zeta, 0.81, I.Fold, merit3=I.cls == 1)
    out += [ev["s"], ev["lam_out"], np.array([ev["E"]])] + ([ev["t"]] if I.cls == 2 else [])
    ws.end(I.lam_try, from_w=True)
    out += list(ws.state()[:2])
    return out


@pytest.mark.parametrize("case", F_CASES, ids=[c.id for c in F_CASES])
def test_forced_reps_against_the_natural_geometry(case, monkeypatch):
    """IPD_APD_REPS took effect (the byte count of a pass names njg), and the masks and elementwise outputs are
    those of the natural geometry; the reductions are held to the same exact reference by the tests above."""
    ws_f, I = workspace(case, monkeypatch)
    ws_n, _ = workspace(case, monkeypatch, reps=None)
    try:
        k, bk = KB[1]
        a, b = elementwise_outputs(ws_f, I, k, bk), elementwise_outputs(ws_n, I, k, bk)
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
        njg = {}
        for name, ws in (("forced", ws_f), ("natural", ws_n)):
            by = ws.bench_eval(1)[1]     # 8*mn + mn + 16*M (+ 8*mn for phi or a vector gama) + 8*(njg*m + 4*nib*n)
            vec = I.cls == 2 or np.ndim(I.gama) > 0
            njg[name] = (by - 9.0 * I.mn - 16.0 * I.M - (8.0 * I.mn if vec else 0.0)) / 8.0 - 4 * -(-I.m // 256) * I.n
            njg[name] /= I.m
        chunks = -(-I.n // 16)
        assert njg == dict(forced=-(-chunks // case.reps), natural=chunks)
    finally:
        ws_f.close()
        ws_n.close()


# ---------------------------------------------------------------------------------------------------------------
# warm starts: OpWarmA / OpWarmB and their epilogues through the same walker and partial sums
# ---------------------------------------------------------------------------------------------------------------
WARM = [Case("b", 1793, 17, 0, None), Case("c", 65, 139, 0, None), Case("d", 70, 8211, 0, None),
        Case("f", 300, 147, 0, None, reps=4), Case("f", 65, 40, 0, None, reps=8), Case("f", 257, 500, 0, None, reps=2)]
warm_cases = pytest.mark.parametrize("case", WARM, ids=["%s-%dx%d%s" % (c.group, c.m, c.n, "-r%d" % c.reps if c.reps else "")
                                                        for c in WARM])


def warm_problem(case, cls):
    rs = np.random.RandomState(77 + case.m + case.n)
    m, n = case.m, case.n
    pr = dict(c=rs.random_sample(m * n), r=rs.random_sample(n), l=rs.random_sample(m),
              p=0.5 + rs.random_sample(m), q=0.5 + rs.random_sample(n))
    if cls == 2:
        pr.update(phi=0.5 + rs.random_sample(m * n), mu=0.65 * min(pr["r"].sum(), pr["l"].sum()))
    return pr


@warm_cases
@pytest.mark.parametrize("gama", [np.inf, 0.05])
def test_warmup_class1_two_iterations(case, gama, monkeypatch):
    pr = warm_problem(case, 1)
    if case.reps:
        monkeypatch.setenv("IPD_APD_REPS", str(case.reps))
    xk, lk = ipd().warmup_class1(pr["c"], pr["r"], pr["l"], pr["p"], pr["q"], gama, 0, 2)
    xr, lr = D.warmup_class1(pr["c"], pr["r"], pr["l"], pr["p"], pr["q"], gama, 2)
    assert np.linalg.norm(xk - xr) <= 1e-10 * (1 + np.linalg.norm(xr))
    assert np.linalg.norm(lk - lr) <= 1e-10 * (1 + np.linalg.norm(lr))


@warm_cases
def test_warmup_class2_two_iterations(case, monkeypatch):
    pr = warm_problem(case, 2)
    if case.reps:
        monkeypatch.setenv("IPD_APD_REPS", str(case.reps))
    uk, lk = ipd().warmup_class2(pr["c"], pr["r"], pr["l"], pr["p"], pr["q"], pr["mu"], pr["phi"], 0, 2)
    ur, lr = D.warmup_class2(pr["c"], pr["r"], pr["l"], pr["p"], pr["q"], pr["mu"], pr["phi"], 2)
    assert np.linalg.norm(uk - ur) <= 1e-10 * (1 + np.linalg.norm(ur))
    # p, q, phi are not constant: 1e-7 for lk, for the reason recorded in tests/test_gpu_driver.py
    assert np.linalg.norm(lk - lr) <= 1e-7 * (1 + np.linalg.norm(lr))


def test_the_switch_refuses_other_values(monkeypatch):
    I = inputs(CASES[0])
    monkeypatch.setenv("IPD_APD_REPS", "3")
    with pytest.raises(ipd().IpdError, match="IPD_APD_REPS must be 1, 2, 4 or 8"):
        ipd().APDWorkspace(1, I.c, I.r, I.l, I.p, I.q)
