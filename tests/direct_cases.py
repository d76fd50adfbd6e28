"""Inputs of the dense direct-solve tests where the block loops wrap (tests/test_direct_cases.py proves them on the
CPU, tests/test_gpu_direct.py runs them on the device).  No GPU use.

The blocked Cholesky of csrc/ipd_dense.hip works on DNB x DNB blocks; its panel and diagonal-block solves give one
thread to a row / a right-hand side in workgroups of 256, its transposes stride over a grid capped at 4096
workgroups.  `k_small_blocks` (csrc/ipd_hybrid.hip) factors every component of at most HYBRID_N0 nodes in LDS, one
workgroup each.  The cases put every one of these loops past its first pass or its first workgroup.

The bar is derived, not measured.  For A x = b of order n the normwise backward error is

    eta = ||b - A x||_2 / (||A||_2 ||x||_2 + ||b||_2),

and a Cholesky solve has eta <= n * gamma_{3n+1} ~ 3 n^2 u, u = 2^-53 (Higham, Accuracy and Stability of Numerical
Algorithms, Theorem 10.4 with || |R'| |R| ||_2 <= n ||A||_2), in any summation order, hence for the blocked and
tiled forms.  bar(n) = (3 n^2 + 4) u per right-hand side; the + 4 covers the two scalings by [q; -p] on the
Hybrid_AMG path.  Residuals are computed in numpy.longdouble (80-bit)."""
import functools
import os
import re

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

from oracle import drivers as D
from oracle import ipd_oracle as O
from tests import problems as PR

LD = np.longdouble
U = 2.0 ** -53
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "codes_of_ipd_ssn_amg_method_amd",
                    "csrc")


def bar(n):
    return (3.0 * n * n + 4.0) * U


def norm2(A):
    """||A||_2 of a symmetric matrix (dense or sparse)"""
    Ad = A.toarray() if sp.issparse(A) else np.asarray(A, float)
    return float(np.abs(np.linalg.eigvalsh(Ad)).max()) if Ad.shape[0] > 1 else float(abs(Ad[0, 0]))


def eta(A, X, B, nrm=None):
    """The backward error of every column of X as a solution of A X = B; residuals in longdouble."""
    X2 = np.asarray(X, float).reshape(A.shape[0], -1).astype(LD)
    B2 = np.asarray(B).reshape(A.shape[0], -1).astype(LD)
    Al = sp.csr_matrix(A).astype(LD) if sp.issparse(A) else np.asarray(A).astype(LD)
    R = B2 - Al @ X2
    assert R.dtype == LD
    nrm = norm2(A) if nrm is None else nrm
    col = lambda M: np.sqrt((M * M).sum(axis=0))
    return (col(R) / (LD(nrm) * col(X2) + col(B2))).astype(float)


# ---------------------------------------------------------------------------------------------------------
# the constants of ipd_dense.hip, read from the source
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_rules():
    """DNB, the rows a k_trsm_panel workgroup takes, the right-hand sides a k_trsm_diag workgroup takes, the
    transposes' workgroup width and their grid cap, as ipd_dense.hip states them."""
    with open(os.path.join(CSRC, "ipd_dense.hip")) as fh:
        src = fh.read()
    dnb = int(re.search(r"constexpr int DNB = (\d+);", src).group(1))
    panel = int(re.search(r"k_trsm_panel, dim3\(cdiv\(below, (\d+)\)\), dim3\((\d+)\)", src).group(1))
    diag = {int(a) for a in re.findall(r"k_trsm_diag, dim3\(cdiv\(nrhs, (\d+)\)\), dim3\(\d+\)", src)}
    assert len(diag) == 1
    diag = diag.pop()
    body = src[src.index("void k_trsm_panel("):src.index("constexpr int DKH")]
    assert "blockIdx.x * %d + threadIdx.x" % panel in body
    body = src[src.index("void k_trsm_diag("):src.index("void k_subst_tiles(")]
    assert "blockIdx.x * %d + threadIdx.x" % diag in body
    width, cap = map(int, re.search(r"std::min<size_t>\(\(len \+ \d+\) / (\d+), (\d+)\)", src).groups())
    assert len(re.findall(r"k_transpose_to_(?:rows|cols), dim3\(g\), dim3\(%d\)" % width, src)) == 2
    return dict(DNB=dnb, panel=panel, diag=diag, width=width, cap=cap)


@functools.lru_cache(maxsize=None)
def hybrid_n0():
    with open(os.path.join(CSRC, "ipd_limits.h")) as fh:
        return int(re.search(r"constexpr int HYBRID_N0 = (\d+);", fh.read()).group(1))


def cdiv(a, b):
    return -(-a // b)


def geometry(n, nrhs, rules=None):
    """Where a solve of order n with nrhs right-hand sides lands: the number of blocks, the last block's rows,
    the workgroups of the first k_trsm_panel launch (0: none) and of k_trsm_diag, the tile columns of
    k_subst_tiles, and whether the transposes take a second trip through their grid-stride loop."""
    r = rules or dense_rules()
    blocks = cdiv(n, r["DNB"])
    below = n - min(r["DNB"], n)
    return dict(blocks=blocks, last_nb=n - (blocks - 1) * r["DNB"], panel_wgs=cdiv(below, r["panel"]),
                diag_wgs=cdiv(nrhs, r["diag"]), tile_cols=cdiv(nrhs, r["DNB"]),
                strides=n * nrhs > r["cap"] * r["width"])


# ---------------------------------------------------------------------------------------------------------
# A. ipd_spd_solve at its geometry edges
# ---------------------------------------------------------------------------------------------------------
SMALL_N = (63, 64, 65, 128, 129)
LARGE_N = (192, 320, 321, 577)
ALL_NRHS = (1, 64, 65, 255, 256, 257, 300)
STRIDE_CASE = (1025, 1030)
SPD_CASES = ([(n, k) for n in SMALL_N for k in ALL_NRHS] + [(n, k) for n in LARGE_N for k in (1, 257)] +
             [STRIDE_CASE])

# what each n and each nrhs is there for: (blocks, rows of the last block, workgroups of the first panel launch)
N_EDGES = {63: (1, 63, 0), 64: (1, 64, 0), 65: (2, 1, 1), 128: (2, 64, 1), 129: (3, 1, 1), 192: (3, 64, 1),
           320: (5, 64, 1), 321: (6, 1, 2), 577: (10, 1, 3), 1025: (17, 1, 4)}
# (workgroups of k_trsm_diag, tile columns of k_subst_tiles)
NRHS_EDGES = {1: (1, 1), 64: (1, 1), 65: (1, 2), 255: (1, 4), 256: (1, 4), 257: (2, 5), 300: (2, 5), 1030: (5, 17)}


@functools.lru_cache(maxsize=None)
def spd_matrix(n):
    """A = G G' + sigma I with about 6 entries a row in G, sigma in [0.5, 1.5): the matrix of
    test_spd_mldivide_matches_numpy.  Returns (A as CSC, ||A||_2)."""
    rs = np.random.RandomState(n)
    G = sp.random(n, n, density=min(1.0, 6.0 / n), random_state=rs, format="csr")
    A = sp.csc_matrix(G @ G.T + sp.identity(n) * (0.5 + rs.random_sample()))
    A.sort_indices()
    return A, norm2(A)


@functools.lru_cache(maxsize=None)
def spd_rhs(n, nrhs):
    B = np.random.RandomState(1000 * n + nrhs).standard_normal((n, nrhs))
    B.setflags(write=False)
    return B


def lapack_solve(A, B):
    """LAPACK's Cholesky solve (potrf / potrs) of the dense copy"""
    Ad = A.toarray() if sp.issparse(A) else np.asarray(A, float)
    return sla.cho_solve(sla.cho_factor(Ad, lower=True), np.asarray(B, float))


# ---------------------------------------------------------------------------------------------------------
# B. failure rules
# ---------------------------------------------------------------------------------------------------------
FAIL_N = 130
FAIL_AT = (100, 129)      # a pivot of the second block; the last pivot of the nb = 2 tail block


@functools.lru_cache(maxsize=None)
def bad_pivot(at):
    """spd_matrix(130) with A[at, at] = -1: the leading `at` rows factor as before, the pivot of row `at` is
    A[at, at] - sum_j L(at, j)^2 <= -1 in any summation order."""
    A = spd_matrix(FAIL_N)[0].tolil()
    A[at, at] = -1.0
    A = sp.csc_matrix(A)
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def nan_entry():
    """spd_matrix(130) with NaN at (100, 70) and (70, 100): the panel solve carries it into row 100, the
    trailing update into the pivot of row 100."""
    A = spd_matrix(FAIL_N)[0].tolil()
    A[100, 70] = A[70, 100] = np.nan
    A = sp.csc_matrix(A)
    A.sort_indices()
    return A


LIMIT_ORDER = 16385               # 16385^2 doubles exceed 2 GiB
LIMIT_NRHS = (1 << 20) + 1


# ---------------------------------------------------------------------------------------------------------
# C. k_small_blocks alone: systems made of small components only
# ---------------------------------------------------------------------------------------------------------
def system(blocks, t_on=()):
    """tests/test_hybrid_plan.py's `_system` with a COMPLETE bipartite mask in every block: eliminating the
    columns of a block fills its row-row Schur complement, so the trailing update of the factorisation works on
    nonzeros.  blocks: (rows, columns) in label order ((1, 0) / (0, 1): a row / a column with no active entry);
    t_on: the blocks on whose nodes T is one."""
    m, n = sum(b[0] for b in blocks), sum(b[1] for b in blocks)
    Y = np.zeros((m, n), np.uint8)
    t = np.zeros(m + n)
    r0 = c0 = 0
    for k, (nr, nc) in enumerate(blocks):
        if k in t_on:
            t[c0:c0 + nc] = 1.0
            t[n + r0:n + r0 + nr] = 1.0
        Y[r0:r0 + nr, c0:c0 + nc] = 1
        r0, c0 = r0 + nr, c0 + nc
    s = Y.reshape(-1, order="F").copy()
    pd = PR.make_prob(m, n, s, t=t, pq_random=True)
    pd["H0"] = O.ASAt(s, pd["p"], pd["q"])
    return pd


SMALL_BLOCKS = ((1, 1), (1, 2), (32, 31), (32, 32), (33, 32), (50, 49), (50, 50), (1, 0), (0, 1)) + ((1, 1),) * 300
SMALL_T_ON = (3, 5)
SMALL_SIZES = {1, 2, 3, 63, 64, 65, 99, 100}
SMALL_SYSTEMS = {
    # every size class, 309 components: more workgroups than the chip has compute units
    "all_sizes": (SMALL_BLOCKS, SMALL_T_ON),
    # one block of exactly HYBRID_N0 nodes as the only component that is not a singleton
    "n0_only": (((1, 0), (50, 50), (0, 1), (1, 0)), ()),
}


@functools.lru_cache(maxsize=None)
def small_system(name):
    """(prob_data, Ae, qp, f in longdouble, [nodes of component k, ascending])"""
    blocks, t_on = SMALL_SYSTEMS[name]
    pd = system(blocks, t_on)
    out = O.build_Ae(pd["H0"], pd["T"], pd["p"], pd["q"], pd["bk1"], pd["tk"])
    Ae, qp = sp.csr_matrix(out[0]), out[5]
    _, sizes, ps, rs = O.components(out[1])
    comps = [np.sort(ps[rs[k]:rs[k + 1]]) for k in range(len(sizes))]
    return pd, Ae, qp, qp.astype(LD) * pd["z"].astype(LD), comps


@functools.lru_cache(maxsize=None)
def small_reference(name):
    """(zeta, it, res, info, rand numbers consumed) of the oracle's Hybrid_AMG"""
    pd = small_system(name)[0]
    rng = O.matlab_rng()
    z, it, res, info = O.Hybrid_AMG(pd, O.amg_options_class2("v"), rng, N0=hybrid_n0())
    used = 0 if rng.random_sample() == O.matlab_rng().random_sample() else -1
    z.setflags(write=False)
    return z, it, res, info, used


def small_etas(name, zeta):
    """[(nb, eta)] per component: u_k = zeta(pk) / qp(pk) as a solution of Ae(pk, pk) u_k = f(pk)"""
    _, Ae, qp, f, comps = small_system(name)
    u = np.asarray(zeta, float).astype(LD) / qp.astype(LD)
    out = []
    for pk in comps:
        Ak = Ae[pk, :][:, pk].toarray()
        out.append((len(pk), float(_eta_ld(Ak, u[pk], f[pk]))))
    return out


def _eta_ld(Ak, u, f):
    r = f - Ak.astype(LD) @ u
    nrm = lambda v: np.sqrt((v * v).sum())
    return nrm(r) / (LD(norm2(Ak)) * nrm(u) + nrm(f))


INDEF_BLOCKS = ((1, 1), (32, 32), (32, 32), (1, 0))


@functools.lru_cache(maxsize=None)
def indefinite_system():
    """Two 64-node blocks; the H0 diagonal entry of one row node of the SECOND is lowered until Ae's entry is
    -1: the first workgroups factor clean blocks, the third meets a pivot <= -1 at local index 32 + 7.
    Returns (prob_data, the node, its block's nodes)."""
    pd = dict(system(INDEF_BLOCKS))
    n = pd["n"]
    node = n + (1 + 32 + 7)                     # row 7 of the second 64-node block; rows follow the n columns
    qp = np.concatenate([pd["q"], -pd["p"]])
    H0 = sp.lil_matrix(pd["H0"])
    H0[node, node] = pd["tk"] * (-1.0 / qp[node] ** 2 - pd["bk1"])       # Ae(i,i) = q^2 (bk1 + H0(i,i)/tk) = -1
    pd["H0"] = sp.csr_matrix(H0)
    rows = n + 1 + 32 + np.arange(32)
    cols = 1 + 32 + np.arange(32)
    return pd, node, np.concatenate([cols, rows])


# ---------------------------------------------------------------------------------------------------------
# D. the dense routes inside the drivers: M = 271 (five blocks), class 2's bordered N = 272
# ---------------------------------------------------------------------------------------------------------
DRIVER_M, DRIVER_N, DRIVER_K = 150, 121, 4
DRIVER_SEED = 2
DRIVER_RUNS = [(1, 1), (2, 1), (2, 2)]        # (class, inner_solver)


@functools.lru_cache(maxsize=None)
def driver_problem(cls):
    from tests.test_gpu_driver import problem
    return problem(cls, DRIVER_M, DRIVER_N, seed=DRIVER_SEED)


@functools.lru_cache(maxsize=None)
def driver_reference(cls):
    """(warm start, the oracle's K iterations with the direct inner solve from it)"""
    pr = driver_problem(cls)
    if cls == 1:
        start = D.warmup_class1(pr["c"], pr["r"], pr["l"], pr["p"], pr["q"], np.inf, 100)
        ref = D.apd_ssn_class1(pr["c"], pr["r"], pr["l"], pr["p"], pr["q"], np.inf, inner="direct", start=start,
                               maxit=DRIVER_K)
    else:
        start = D.warmup_class2(pr["c"], pr["r"], pr["l"], pr["p"], pr["q"], pr["mu"], pr["phi"], 100)
        ref = D.apd_ssn_class2(pr["c"], pr["r"], pr["l"], pr["p"], pr["q"], pr["mu"], pr["phi"], inner="direct",
                               start=start, maxit=DRIVER_K)
    return start, ref


# ---------------------------------------------------------------------------------------------------------
# E. ideal interpolation with Nf and Nc past 256
# ---------------------------------------------------------------------------------------------------------
IDEAL_N, IDEAL_DEG, IDEAL_SEED, IDEAL_SHIFT = 1200, 3, 7, 0.05


@functools.lru_cache(maxsize=None)
def ideal_matrix():
    A = PR.random_sym_graph_laplacian(IDEAL_N, deg=IDEAL_DEG, seed=IDEAL_SEED) + sp.identity(IDEAL_N) * IDEAL_SHIFT
    return sp.csr_matrix(A)


def ideal_options(isnsp):
    o = O.amg_options_class1("v")
    o.update(bigph=0, isnsp=isnsp, inter=2)
    return o


@functools.lru_cache(maxsize=None)
def ideal_reference(isnsp):
    """(Ac, Pro, isC) of the oracle's transfer"""
    Ac, Pro, info = O.transfer(ideal_matrix(), ideal_options(isnsp), 2, O.matlab_rng())
    return Ac, Pro, info["isC"]


def ideal_etas(Pro, isC):
    """eta of every column of W = Pro(F, :) as a solution of Aff W = -Afc; (Nf, etas)"""
    A = ideal_matrix()
    F, C = np.flatnonzero(~isC), np.flatnonzero(isC)
    Aff = sp.csr_matrix(A[F, :][:, F])
    Afc = A[F, :][:, C].toarray()
    W = sp.csr_matrix(Pro)[F, :].toarray()
    return len(F), eta(Aff, W, -Afc)
