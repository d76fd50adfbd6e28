"""The reference side of the Hybrid_AMG_PCG tests (tests/hybrid_pcg_ref.py) against the oracle's own
Hybrid_AMG where there is no GPU: same routing and rand stream, a solution of the original system, and
convergence where the stationary iteration runs into maxit."""
import numpy as np
import scipy.sparse as sp

from oracle import ipd_oracle as O
from tests import hybrid_pcg_ref as HR
from tests import problems as PR
from tests.test_golden_oracle import load, problem_from


def _he(pd):
    M = pd["m"] + pd["n"]
    return pd["bk1"] * sp.identity(M) + (pd["T"] + pd["H0"]) / pd["tk"]


def v1_opts():
    o = O.amg_options_class1("v")
    o.update(smoth=1)
    return o


def test_reference_on_tree_rect_multi():
    m, n = 260, 150
    s = PR.mask_tree(m, n, extra=0.0, seed=3, connect=False)
    pd = PR.make_prob(m, n, s, pq_random=True)
    pd["H0"] = O.ASAt(s, pd["p"], pd["q"])
    opts = v1_opts()
    r0 = HR.CountingRng()
    zo, ito, reso, infoo = O.Hybrid_AMG(pd, opts, r0)
    r1 = HR.CountingRng()
    log = []
    z, it, res, info = HR.Hybrid_AMG_PCG(pd, opts, r1, log)
    assert np.array_equal(info, infoo)
    assert r0.consumed == r1.consumed and r0.random_sample(1)[0] == r1.random_sample(1)[0]
    assert ito == opts["maxit"] and reso > 1e-10          # the stationary iteration stalls here
    assert it < opts["maxit"] and res <= opts["retol"] and len(log) >= 1
    He, nz = _he(pd), np.linalg.norm(pd["z"])
    assert np.linalg.norm(He @ z - pd["z"]) <= 1e-9 * nz


def test_reference_on_a_golden_system():
    pd = problem_from(load("class1_500_k08.npz"))
    pd["H0"] = O.ASAt(pd["s"], pd["p"], pd["q"])
    opts = O.amg_options_class1("w")
    r0 = HR.CountingRng()
    zo, ito, reso, infoo = O.Hybrid_AMG(pd, opts, r0)
    r1 = HR.CountingRng()
    z, it, res, info = HR.Hybrid_AMG_PCG(pd, opts, r1)
    assert np.array_equal(info, infoo) and r0.consumed == r1.consumed
    assert it <= ito and res <= opts["retol"]
    assert np.linalg.norm(z - zo) <= 1e-6 * max(1.0, np.linalg.norm(zo))
