"""The primal certificate (include/ipd_amg.h) re-stated in numpy, operation by operation, in
float64 or in longdouble, and the checks tests/test_gpu_round.py applies to what the device returns.  numpy's sums
have their own order: what the header fixes beyond the order of the operations of one entry is compared within the
any-order bound gamma(s) = s*u / (1 - s*u), u = 2^-53, or bit for bit where every sum is
exact.  No GPU here: tools/bench_round.py uses the restatement as the host route."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def gamma(s):
    return s * U / (1.0 - s * U)


def clamp(X, tol):
    """step 1: plan()'s threshold, then the clamp at 0; a NaN becomes 0"""
    with np.errstate(invalid="ignore"):
        keep = ~(np.abs(X) <= tol) & (X > 0)
    return np.where(keep, X, 0.0), keep


def scale(s, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > bound, bound / s, 1.0).astype(s.dtype)


def pos(d):
    return np.where(d > 0, d, 0.0).astype(d.dtype)


def round_ref(cls, pr, m, n, x, tol=0.0, side=0, ld=False):
    """every quantity of the header's twelve steps for the x block x (mn entries, column-major)"""
    T = LD if ld else np.float64
    X = np.asarray(x, dtype=np.float64)[:m * n].reshape((m, n), order="F")
    Xp64, keep = clamp(X, tol)
    Xp = Xp64.astype(T)
    p, q, r, l = (pr[k].astype(T) for k in ("p", "q", "r", "l"))
    C = pr["c"].reshape((m, n), order="F").astype(T)
    out = dict(xp=Xp64)
    a0 = (q[None, :] * Xp).sum(axis=1)
    b0 = (p[:, None] * Xp).sum(axis=0)
    if side == 0:
        rho = scale(a0, l)
        b1 = (p[:, None] * (rho[:, None] * Xp)).sum(axis=0)
        kappa = scale(b1, r)
    else:
        kappa = scale(b0, r)
        a1 = (q[None, :] * (Xp * kappa[None, :])).sum(axis=1)
        rho = scale(a1, l)
    X2 = (rho[:, None] * Xp) * kappa[None, :]
    a2 = (q[None, :] * X2).sum(axis=1)
    b2 = (p[:, None] * X2).sum(axis=0)
    fs = (C * X2).sum()
    e, f = pos(l - a2), pos(r - b2)
    se, sf = (p * e).sum(), (q * f).sum()
    EF = e[:, None] * f[None, :]
    cc = (C * EF).sum()
    nan = T(np.nan)
    ms = cp = nan
    with np.errstate(divide="ignore", invalid="ignore"):
        if cls == 1:
            theta, t = T(1), (T(1) / se if se > 0 else T(0))
            viol = (p * np.abs(a0 - l)).sum() + (q * np.abs(b0 - r)).sum()
        else:
            PHI = pr["phi"].reshape((m, n), order="F").astype(T)
            mu = T(pr["mu"])
            ms, cp = (PHI * X2).sum(), (PHI * EF).sum()
            if ms >= mu:
                theta, t = mu / ms, T(0)
            else:
                theta, t = T(1), (mu - ms) / cp
            viol = (p * pos(a0 - l)).sum() + (q * pos(b0 - r)).sum()
        fval = theta * fs + t * cc
        ok = bool(np.isfinite(theta) and np.isfinite(t) and np.isfinite(fval))
        if cls == 2:
            ok = ok and bool(t * se <= 1) and bool(t * sf <= 1)
        xhat = theta * X2 + t * EF
    gone = (X != 0) & ~keep
    out.update(a0=a0, b0=b0, rho=rho, kappa=kappa, x2=X2, a2=a2, b2=b2, e=e, f=f, fs=fs, ms=ms, se=se, sf=sf, cc=cc,
               cp=cp, theta=theta, t=t, fval=fval, ok=int(ok), viol_in=viol, xhat=xhat,
               dropped=np.abs(X[gone & ~np.isnan(X)]).sum(), ndropped=int(gone.sum()))
    if cls == 2:
        with np.errstate(invalid="ignore"):
            out["yhat"] = pos(r - (theta * b2 + t * (se * f)))
            out["zhat"] = pos(l - (theta * a2 + t * (e * sf)))
    return out


def rebuild(x, m, n, tol, res):
    """X^ (m, n) in longdouble from the injected x and the factors and scalars a call returned"""
    Xp = clamp(np.asarray(x, dtype=np.float64)[:m * n].reshape((m, n), order="F"), tol)[0].astype(LD)
    rho, kappa, e, f = (res[k].astype(LD) for k in ("rho", "kappa", "e", "f"))
    return LD(res["theta"]) * ((rho[:, None] * Xp) * kappa[None, :]) + LD(res["t"]) * (e[:, None] * f[None, :])


def slacks(cls, pr, m, n, Xh, res):
    """class 2's y^, z^ in longdouble from the marginals of the rebuilt X^ -- what the header's step 11 is in exact
    arithmetic: theta*b2_j + t*(Se*f_j) is the column marginal of X^"""
    p, q, r, l = (pr[k].astype(LD) for k in ("p", "q", "r", "l"))
    return pos(r - (p[:, None] * Xh).sum(axis=0)), pos(l - (q[None, :] * Xh).sum(axis=1))


def feasibility_bounds(pr, m, n):
    """(row bound, column bound): gamma(m+n+16)*(l_i + T/p_i) and gamma(m+n+16)*(r_j + T/q_j), T = <p,l> + <q,r>"""
    p, q, r, l = pr["p"], pr["q"], pr["r"], pr["l"]
    T = float(p @ l + q @ r)
    g = gamma(m + n + 16)
    return g * (l + T / p), g * (r + T / q)


def check_feasible(cls, pr, m, n, Xh, what="", yz=None):
    """the feasibility assertions of the rounded plan Xh (longdouble); yz = (y^, z^) of class 2 when given.  Returns
    the largest used fraction of the bounds."""
    p, q, r, l = (pr[k].astype(LD) for k in ("p", "q", "r", "l"))
    rb, cb = feasibility_bounds(pr, m, n)
    assert (Xh >= 0).all(), (what, float(Xh.min()))
    rows = (q[None, :] * Xh).sum(axis=1) - l
    cols = (p[:, None] * Xh).sum(axis=0) - r
    if cls == 1:
        worst = max(float((np.abs(rows) / rb).max()), float((np.abs(cols) / cb).max()))
        assert (np.abs(rows) <= rb).all() and (np.abs(cols) <= cb).all(), (what, worst)
        return worst
    worst = max(float((rows / rb).max()), float((cols / cb).max()))
    assert (rows <= rb).all() and (cols <= cb).all(), (what, worst)
    mu = LD(pr["mu"])
    mass = (pr["phi"].reshape((m, n), order="F").astype(LD) * Xh).sum()
    mb = 4 * gamma(m + n + 16) * float(mu)
    worst = max(worst, float(abs(mass - mu)) / mb)
    assert abs(mass - mu) <= mb, (what, float(mass), float(mu), mb)
    if yz is not None:
        y, z = (np.asarray(v).astype(LD) for v in yz)
        assert (y >= 0).all() and (z >= 0).all(), what
        ry, rz = np.abs(cols + y), np.abs(rows + z)
        worst = max(worst, float((ry / cb).max()), float((rz / rb).max()))
        assert (ry <= cb).all() and (rz <= rb).all(), (what, worst)
    return worst


def check_values(cls, pr, m, n, x, tol, res, what=""):
    """fval against <c, X^> of the rebuilt plan, fs, cc, ms, cp against their sums over the rebuilt factors, se and sf
    against theirs: each within gamma(terms + 16) * sum |terms|, 2mn terms for the mn-sized sums"""
    Xp = clamp(np.asarray(x, dtype=np.float64)[:m * n].reshape((m, n), order="F"), tol)[0].astype(LD)
    rho, kappa, e, f = (res[k].astype(LD) for k in ("rho", "kappa", "e", "f"))
    X2 = (rho[:, None] * Xp) * kappa[None, :]
    EF = e[:, None] * f[None, :]
    C = pr["c"].reshape((m, n), order="F").astype(LD)
    Xh = LD(res["theta"]) * X2 + LD(res["t"]) * EF
    g2 = gamma(2 * m * n + 16)
    pairs = [("fval", (C * Xh).sum(), g2 * float((np.abs(C) * np.abs(Xh)).sum())),
             ("fs", (C * X2).sum(), g2 * float((np.abs(C) * X2).sum())),
             ("cc", (C * EF).sum(), g2 * float((np.abs(C) * EF).sum())),
             ("se", (pr["p"].astype(LD) * e).sum(), gamma(m + 16) * float((np.abs(pr["p"]) * e).sum())),
             ("sf", (pr["q"].astype(LD) * f).sum(), gamma(n + 16) * float((np.abs(pr["q"]) * f).sum()))]
    if cls == 2:
        PHI = pr["phi"].reshape((m, n), order="F").astype(LD)
        pairs += [("ms", (PHI * X2).sum(), g2 * float((np.abs(PHI) * X2).sum())),
                  ("cp", (PHI * EF).sum(), g2 * float((np.abs(PHI) * EF).sum()))]
    else:
        assert np.isnan(res["ms"]) and np.isnan(res["cp"]), what
    for key, want, bar in pairs:
        err = float(abs(LD(res[key]) - want))
        print("%s %s: err %.3e bar %.3e" % (what, key, err, bar))
        assert err <= bar, (what, key, float(res[key]), float(want), err, bar)
