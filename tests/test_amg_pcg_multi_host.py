"""AMG-preconditioned CG for several right-hand sides without a GPU: the entry points exist through the C ABI,
Python and the MEX gateway, and the block loop restated in numpy -- every column in lockstep, a column that
has stopped frozen (its d, r and record stay as they are while later iterations run for the rest) -- is the
single restatement (tests/amg_pcg_ref.py) run column by column, bit for bit."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ipd_oracle as O
from tests import amg_pcg_ref as R
from tests import problems as PR
from tests.test_gpu_setup import newton_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ipd_amg_pcg_multi", "ipd_amg_pcg_multi_dev")


def block_pcg(A, E, M, retol=1e-11, maxit=10000, G=None):
    """numpy restatement of the block loop: per-column scalars, an active mask, frozen columns (their cycle
    input is zero, so their w is M(0) = 0, and nothing of theirs is updated).  Columns are kept as separate
    contiguous vectors so that every dot is the one the single restatement takes."""
    N, k = E.shape
    cols = range(k)
    d = [np.zeros(N) if G is None else np.array(G[:, j], float) for j in cols]
    r = [E[:, j] - A @ d[j] for j in cols]                            # PCG.m:68
    w = [M(r[j]) for j in cols]
    dnew = [float(r[j] @ w[j]) for j in cols]
    d0 = list(dnew)
    p = [None] * k
    beta = [0.0] * k
    it = np.zeros(k, int)
    resk = [[] for _ in cols]
    act = [it[j] < maxit and dnew[j] > retol ** 2 * d0[j] for j in cols]
    with np.errstate(invalid="ignore", divide="ignore"):
        while any(act):
            for j in cols:                                            # K1, K2
                if not act[j]:
                    continue
                p[j] = w[j] if p[j] is None else w[j] + beta[j] * p[j]
                q = A @ p[j]
                alpha = dnew[j] / float(q @ p[j])
                d[j] = d[j] + alpha * p[j]
                r[j] = r[j] - alpha * q
            w_old = list(w)
            w = [M(r[j] if act[j] else np.zeros(N)) for j in cols]    # the block cycle
            for j in cols:                                            # K3
                if not act[j]:
                    continue
                dn = float(r[j] @ w[j])
                beta[j] = (dn - float(r[j] @ w_old[j])) / dnew[j]
                dnew[j] = dn
                it[j] += 1
                resk[j].append(math.sqrt(abs(dn / d0[j])))
                act[j] = it[j] < maxit and dn > retol ** 2 * d0[j]
        res = np.array([math.sqrt(abs(dnew[j] / d0[j])) if d0[j] != 0 else float("nan") for j in cols])
    return np.column_stack(d), it, res, [np.array(v) for v in resk]


def test_header_declares_both_entry_points():
    txt = open(os.path.join(ROOT, "include", "ipd_amg.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*ipd_amg\s*\*" % name, txt), name


def test_library_exports_both_entry_points():
    import __graft_entry__ as g
    g.build()
    from codes_of_ipd_ssn_amg_method_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name


def test_python_api_and_shape_checks():
    import codes_of_ipd_ssn_amg_method_amd as ipd
    assert callable(getattr(ipd.AMGHierarchy, "pcg_multi", None))
    assert callable(ipd.AMG_PCG_multi) and "AMG_PCG_multi" in ipd.__all__

    class Fake:   # the shape checks run before anything reaches the library
        N = 4
        handle = None
    for E, g in [(np.ones((5, 2)), None), (np.ones((4, 0)), None), (np.ones((2, 2, 1)), None),
                 (np.ones((4, 3)), np.zeros((4, 2))), (np.ones((4, 3)), np.zeros(4))]:
        with pytest.raises(ValueError):
            ipd.AMGHierarchy.pcg_multi(Fake(), E, None if g is None else dict(guess=g))


def test_mex_gateway_and_shim():
    mex = os.path.join(ROOT, "codes_of_ipd_ssn_amg_method_amd", "mex")
    assert '"AMG_PCG_multi"' in open(os.path.join(mex, "ipd_mex.cpp")).read()
    shim = open(os.path.join(mex, "AMG_PCG_multi.m")).read()
    assert "function [D,it,res,resk] = AMG_PCG_multi(varargin)" in shim and "ipd_mex('AMG_PCG_multi'" in shim


@pytest.mark.parametrize("cycle", ["v", "w"])
def test_block_restatement_equals_single_per_column(cycle):
    m = n = 40
    Ae, pd = newton_matrix(m, n, PR.mask_tree(m, n, seed=2))
    A = sp.csr_matrix(Ae)
    N = m + n
    o = O.amg_options_class1(cycle)
    o.update(fnode=n, isnsp=1)
    h = O.amg_setup(A, o, O.matlab_rng())
    M = R.cycle_operator(h, o)
    assert not M(np.zeros(N)).any()   # a frozen column's cycle input gives e = 0
    rs = np.random.RandomState(3)
    f = np.concatenate([pd["q"], -pd["p"]]) * pd["z"]
    g = 0.1 * rs.standard_normal(N)
    x = np.zeros(N)
    x[5] = 0.5
    # a column needing many iterations, a scaled copy, a zero column, a column whose guess is the solution,
    # a smooth right-hand side
    E = np.column_stack([f, 1e-3 * f, np.zeros(N), A @ x, A @ np.ones(N) + 1e-3 * f])
    G = np.column_stack([g, 1e-3 * g, np.zeros(N), x, np.zeros(N)])
    for maxit in (3, 500):
        D, it, res, resk = block_pcg(A, E, M, retol=1e-11, maxit=maxit, G=G)
        assert it[2] == 0 and it[3] == 0 and np.isnan(res[2]) and np.isnan(res[3])
        assert np.array_equal(D[:, 3], x) and not D[:, 2].any()
        for j in range(E.shape[1]):
            dj, itj, resj, reskj = R.amg_pcg(A, E[:, j], M, retol=1e-11, maxit=maxit, guess=G[:, j])
            assert it[j] == itj and np.array_equal(D[:, j], dj), (maxit, j)
            assert np.array_equal(resk[j], reskj) and np.array_equal(res[j], resj, equal_nan=True), (maxit, j)
        if maxit == 3:
            assert it[0] == 3
        else:
            assert it[0] > 3 and res[0] <= 1e-11
