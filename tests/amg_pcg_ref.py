"""Numpy restatement of AMG-preconditioned conjugate gradients (include/ipd_amg.h, ipd_amg_pcg): the
loop of PCG.m:68-87 with a preconditioner M and the flexible (Polak-Ribiere) beta
(r'w - r'w_old)/delta_old.  With the oracle's hierarchy M is O.MG_Vcycle / O.MG_Wcycle(h, r, isnsp, 1)."""
import math

import numpy as np

from oracle import ipd_oracle as O


def cycle_operator(h, amg_options):
    """M(r): one cycle of the oracle hierarchy `h` from a zero guess, the hierarchy's own options."""
    cyc, isnsp = amg_options["cycle"], int(amg_options.get("isnsp") or 0)
    if cyc == "v":
        return lambda r: O.MG_Vcycle(h, r, isnsp, 1)
    if cyc == "w":
        return lambda r: O.MG_Wcycle(h, r, isnsp, 1)
    raise ValueError("AMG-PCG needs cycle 'v' or 'w'")


def amg_pcg(A, e, M, retol=1e-11, maxit=10000, guess=None, trace=None):
    """Returns d, it, res, resk (resk has `it` entries).  trace: a list that receives delta_0 and then, per
    iteration, the inner products and scalars (pq, rw, rwo, alpha, beta) as Python floats."""
    e = np.asarray(e, float)
    d = np.zeros_like(e) if guess is None else np.array(guess, float)
    r = e - A @ d
    w = M(r)
    delta_new = float(r @ w)
    delta_0 = delta_new
    if trace is not None:
        trace.append(delta_0)
    p = w
    it = 0
    resk = []
    with np.errstate(invalid="ignore", divide="ignore"):
        while it < maxit and delta_new > retol ** 2 * delta_0:
            delta_old = delta_new
            q = A @ p
            pq = float(q @ p)
            alpha = delta_old / pq
            d = d + alpha * p
            r = r - alpha * q
            w_old = w
            w = M(r)
            delta_new = float(r @ w)
            rwo = float(r @ w_old)
            beta = (delta_new - rwo) / delta_old
            if trace is not None:
                trace.append(dict(pq=pq, rw=delta_new, rwo=rwo, alpha=alpha, beta=beta))
            p = w + beta * p
            it += 1
            resk.append(math.sqrt(abs(delta_new / delta_0)))
        res = math.sqrt(abs(delta_new / delta_0)) if delta_0 != 0 else float("nan")
    return d, it, res, np.array(resk)
