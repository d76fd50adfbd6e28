"""Reference side of Hybrid_AMG_PCG / AMG4POT(..., 'amg_pcg'): oracle/ipd_oracle.py's Hybrid_AMG with its
`solver=` hook set to the oracle's setup followed by the numpy AMG-PCG of tests/amg_pcg_ref.py on the
given random guess, and AMG4POT restated around it (Class2/AMG4POT.m:27-55)."""
import numpy as np

from oracle import ipd_oracle as O
from tests import amg_pcg_ref as R


class CountingRng:
    """the rand stream with a count of the numbers drawn (ipd.MatlabRand.consumed's counterpart)"""

    def __init__(self, rng=None):
        self.rng = rng if rng is not None else O.matlab_rng()
        self.consumed = 0

    def random_sample(self, n):
        out = self.rng.random_sample(n)
        self.consumed += int(np.size(out))
        return out


def pcg_solver(rng, log=None):
    """solver(A, f, o) for O.Hybrid_AMG: amg_setup (draws mis_set's numbers from `rng`) + AMG-PCG from
    o['guess'] with amg_options' retol / maxit (Class_AMG's defaults when unset)."""
    def solver(A, f, o):
        retol = 1e-12 if o.get("retol") is None else o["retol"]
        maxit = 50 if o.get("maxit") is None else int(o["maxit"])
        h = O.amg_setup(A, o, rng)
        d, it, res, resk = R.amg_pcg(A, f, R.cycle_operator(h, o), retol=retol, maxit=maxit, guess=o["guess"])
        if log is not None:
            log.append(dict(N=A.shape[0], it=it, res=res))
        return d, it, res, resk, None
    return solver


def Hybrid_AMG_PCG(prob_data, amg_options, rng, log=None):
    return O.Hybrid_AMG(prob_data, amg_options, rng, solver=pcg_solver(rng, log))


def AMG4POT_PCG(prob_data, amg_options, rng):
    p, q = prob_data["p"], prob_data["q"]
    bk1, tk = prob_data["bk1"], prob_data["tk"]
    phi = np.asarray(prob_data["phi"], float)
    z = np.asarray(prob_data["z"], float)
    s = np.asarray(prob_data["s"], float)
    z1, z2 = z[:-1], z[-1]
    epss, sg = bk1, 1 / tk
    phi_e = epss + sg * (phi @ (s * phi))
    v = O.Ax(s * phi, p, q)
    w = z1 - sg / phi_e * z2 * v
    pd = dict(prob_data)
    pd["z"] = v
    vv, it1, res1, info1 = Hybrid_AMG_PCG(pd, amg_options, rng)
    pd["z"] = w
    ww, it2, res2, info2 = Hybrid_AMG_PCG(pd, amg_options, rng)
    tt = sg ** 2 / (phi_e - sg ** 2 * (v @ vv))
    zeta1 = ww + tt * vv * (v @ ww)
    zeta2 = (z2 - sg * (v @ zeta1)) / phi_e
    return np.concatenate([zeta1, [zeta2]]), max(it1, it2), max(res1, res2), np.maximum(info1, info2)
