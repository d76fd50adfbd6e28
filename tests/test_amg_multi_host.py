"""The block solve's loop restated in numpy (CPU): every column of B runs Class_AMG's solve phase
(Class_AMG.m:86-109) in lockstep with the others, a column that has stopped is frozen (its x, its
history and its count stay as they are while later cycles run for the rest) -- the rule
ipd_amg_solve_multi implements with its active mask.  Checked against O.Class_AMG per column.
Also the Python wrapper's shape checks, which need no device."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ipd_oracle as O
from tests import problems as PR
from tests.test_gpu_setup import newton_matrix


def block_solve(h, B, G, o):
    """numpy restatement of the block loop: per-column records, active mask, frozen columns"""
    A = h.Ack[1]
    N, k = B.shape
    cyc = {"v": O.MG_Vcycle, "w": O.MG_Wcycle}.get(o["cycle"])
    col = lambda M: np.column_stack([M(j) for j in range(k)])
    norms = lambda X: np.array([np.linalg.norm(A @ X[:, j] - B[:, j]) for j in range(k)])
    X = G.copy()
    R = col(lambda j: B[:, j] - A @ X[:, j])                               # first loop top
    res0 = norms(X)
    res = res0.copy()
    cnt = np.zeros(k, int)
    rel = np.zeros(k)
    rk = [[0.0] if r == 0 else [1.0] for r in res0]
    rho = [[np.inf] if r == 0 else [np.nan] for r in res0]
    act = (res0 != 0) & (1.0 > o["retol"]) & (1 <= o["maxit"])
    while act.any():
        E = np.zeros_like(X)
        for j in np.flatnonzero(act):                                     # one block cycle
            if cyc is not None:
                E[:, j] = cyc(h, R[:, j], o["isnsp"])
        X = np.where(act, X + E, X)                                        # frozen columns keep x
        R = np.where(act, col(lambda j: B[:, j] - A @ X[:, j]), 0.0)       # ... and get r = 0
        rn = norms(X)
        for j in np.flatnonzero(act):
            prev, res[j] = res[j], rn[j]
            rel[j] = rn[j] / res0[j]
            r_ = rn[j] / prev
            cnt[j] += 1
            rk[j].append(rel[j])
            rho[j].append(r_)
            act[j] = not (r_ > 1.0) and rel[j] > o["retol"] and cnt[j] + 1 <= o["maxit"]
    return X, cnt, rel, [np.array(v) for v in rk], [np.array(v) for v in rho]


@pytest.mark.parametrize("cycle", ["v", "w"])
@pytest.mark.parametrize("isnsp", [0, 1])
def test_restatement_equals_class_amg_per_column(cycle, isnsp):
    m = n = 48
    s = PR.mask_tree(m, n, seed=2)
    Ae, pd = newton_matrix(m, n, s)
    A = sp.csr_matrix(Ae)
    rs = np.random.RandomState(3)
    f = np.concatenate([pd["q"], -pd["p"]]) * pd["z"]
    g = pd["bk1"] * pd["tk"] * rs.random_sample(m + n)
    # a column needing many cycles, a scaled copy, a zero column, a column that is A*guess
    B = np.column_stack([f, 1e-3 * f, np.zeros(m + n), A @ g, f + 0.1 * rs.standard_normal(m + n)])
    G = np.column_stack([g, 1e-3 * g, np.zeros(m + n), g, g])
    o = O.amg_options_class1(cycle)
    o.update(fnode=n, isnsp=isnsp)
    h = O.amg_setup(A, o, O.matlab_rng())
    X, it, rel, rk, rho = block_solve(h, B, G, o)
    assert it[2] == 0 and it[3] == 0 and it[0] >= 3
    for j in range(B.shape[1]):
        xo, ito, relo, rko, rhoo, _ = O.Class_AMG(A, B[:, j], dict(o, guess=G[:, j]), O.matlab_rng(),
                                                  return_hierarchy=True)
        assert it[j] == ito and rel[j] == relo
        assert np.array_equal(rk[j], rko) and np.array_equal(rho[j], rhoo, equal_nan=True)
        assert np.array_equal(X[:, j], xo)


def test_wrapper_shape_checks():
    from codes_of_ipd_ssn_amg_method_amd.api import multi_args
    B = np.arange(12.0).reshape(4, 3)
    Bf, gf, k = multi_args(4, B)
    assert k == 3 and gf is None and Bf.flags.f_contiguous and np.array_equal(Bf, B)
    Bf, gf, k = multi_args(4, np.ones(4), np.zeros(4))
    assert k == 1 and Bf.shape == (4, 1) and gf.shape == (4, 1) and gf.flags.f_contiguous
    for bad in (np.ones((5, 2)), np.ones((4, 0)), np.ones((2, 2, 1))):
        with pytest.raises(ValueError):
            multi_args(4, bad)
    with pytest.raises(ValueError):
        multi_args(4, B, np.zeros((4, 2)))
