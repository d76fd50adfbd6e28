"""The polynomial form of a level visit (csrc/ipd_cycle.hip: k_pack_poly, k_bpoly_*)
restated in numpy and checked against the oracle's own smoothing loops (oracle/ipd_oracle.py:_smooth,
i.e. AMG/MG_Vcycle.m:14-41): the nu sweeps, the residual and the transfers of a visit are two dense
maps.  This pins the ALGEBRA the kernels implement; their arithmetic is checked on the GPU against the
oracle's solves (tests/test_gpu_resident_remote.py, tests/test_gpu_cycle.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ipd_oracle as O


def level(N, Nc, seed):
    rs = np.random.RandomState(seed)
    B = sp.random(N, N, density=0.3, random_state=rs, format="csr")
    A = (B + B.T).toarray()
    A = A + np.diag(np.abs(A).sum(axis=1) + 0.05)          # symmetric, diagonally dominant
    P = sp.random(N, Nc, density=0.25, random_state=rs, format="csr").toarray()
    P[:Nc, :] += np.eye(Nc)
    dinv = 0.5 / np.diag(A)                                 # Jacobi level: Class_AMG.m:60-62
    return A, P, dinv, rs


def stacked_operators(A, P, dinv, isnsp, nu):
    """What pack_bpoly / k_pack_poly produce: M2a, M1, w and the rows stacked below them."""
    N = A.shape[0]
    one = np.ones(N)
    Axi = A @ one
    xx = float(one @ Axi)
    u = (1.0 - dinv * Axi) / xx if isnsp else np.zeros(N)
    cs = one @ A                                            # column sums 1'A
    S = np.eye(N) - (dinv[:, None] * A + np.outer(u, cs))   # I - Rg A
    powers = [np.eye(N)]
    for _ in range(nu):
        powers.append(S @ powers[-1])
    M1 = powers[nu]
    ssum = sum(powers[:nu])                                 # I + S + ... + S^(nu-1)
    M2a = ssum * dinv[None, :]
    w = ssum @ u
    T1 = P.T @ A
    return dict(M1=M1, M2a=M2a, w=w, Mr_low=P.T - T1 @ M2a, Me_low=-T1 @ M1, W_low=-T1 @ w, Mc=M1 @ P)


@pytest.mark.parametrize("isnsp", [0, 1])
@pytest.mark.parametrize("N,Nc", [(14, 3), (40, 11), (66, 11), (100, 34)])
def test_a_visit_is_two_dense_maps(N, Nc, isnsp):
    nu = 5
    A, P, dinv, rs = level(N, Nc, 7 * N + isnsp)
    R = sp.diags(dinv).tocsr()
    As = sp.csr_matrix(A)
    r = rs.standard_normal(N)
    e0 = rs.standard_normal(N)
    ec = rs.standard_normal(Nc)
    M = stacked_operators(A, P, dinv, isnsp, nu)
    sumr = float(np.ones(N) @ r)
    for e in (np.zeros(N), e0):                             # first visit (zero start) and MG_Wcycle.m:30's
        pre = O._smooth(As, R, r, e.copy(), isnsp, nu)      # :14-25
        rc = P.T @ (r - A @ pre)                            # :27
        post = O._smooth(As, R, r, pre + P @ ec, isnsp, nu)  # :31-41
        pre_poly = M["M2a"] @ r + M["M1"] @ e + M["w"] * sumr
        rc_poly = M["Mr_low"] @ r + M["Me_low"] @ e + M["W_low"] * sumr
        post_poly = M["M2a"] @ r + M["M1"] @ pre + M["Mc"] @ ec + M["w"] * sumr
        scale = 1.0 + np.abs(pre).max() + np.abs(post).max()
        assert np.abs(pre - pre_poly).max() <= 1e-11 * scale
        assert np.abs(rc - rc_poly).max() <= 1e-11 * (scale + np.abs(rc).max())
        assert np.abs(post - post_poly).max() <= 1e-11 * scale


def composed_operators(A, P, dinv, isnsp, nu):
    """What amg_attach_poly2 / k_bpoly_compose produce for a level whose coarse level has ONE row (the
    metric's level 2): the whole visit of MG_Vcycle.m:14-41 as e = B r + wB (1'r) + mp ec, where the coarse
    correction is ec = (s r + ws (1'r)) / Ac (PCG.m on one row) -- pre-smoothing from zero, the restriction
    and post-smoothing folded into one dense map."""
    M = stacked_operators(A, P, dinv, isnsp, nu)
    I1 = np.eye(A.shape[0]) + M["M1"]
    return dict(B=I1 @ M["M2a"], wB=I1 @ M["w"], mp=M["Mc"][:, 0], s=M["Mr_low"][0], ws=float(M["W_low"][0]))


@pytest.mark.parametrize("nu", [1, 2, 5])
@pytest.mark.parametrize("isnsp", [0, 1])
@pytest.mark.parametrize("N", [14, 40, 100])
def test_composed_visit_is_one_dense_map(N, isnsp, nu):
    """Level 2 of a three-level hierarchy whose coarsest level has one row: the composed operator of the
    resident kernel's POLY2 form (ResDesc::p2rows) against the oracle's visit -- pre-smoothing from zero
    (O._smooth, MG_Vcycle.m:14-25), restriction (:27), the one-row coarse solve (:43, PCG.m), prolongation
    and post-smoothing (:31-41)."""
    A, P, dinv, rs = level(N, 1, 11 * N + 3 * nu + isnsp)
    As = sp.csr_matrix(A)
    R = sp.diags(dinv).tocsr()
    Ac = sp.csr_matrix(P.T @ A @ P)
    C = composed_operators(A, P, dinv, isnsp, nu)
    for _ in range(3):
        r = rs.standard_normal(N)
        pre = O._smooth(As, R, r, np.zeros(N), isnsp, nu)
        rc = P.T @ (r - A @ pre)
        ec = O.PCG(Ac, rc)[0]
        e = O._smooth(As, R, r, pre + P @ ec, isnsp, nu)
        sumr = float(np.ones(N) @ r)
        rc_poly = float(C["s"] @ r) + C["ws"] * sumr
        e_poly = C["B"] @ r + C["wB"] * sumr + C["mp"] * (rc_poly / Ac[0, 0])
        assert abs(rc[0] - rc_poly) <= 1e-11 * (1.0 + abs(rc[0]) + np.abs(r).max())
        assert np.abs(e - e_poly).max() <= 1e-11 * (1.0 + np.abs(e).max())
