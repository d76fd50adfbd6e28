"""Inputs of the PCG tests beyond one workgroup pass and beyond 64-entry rows (tests/test_pcg_cases.py proves them
fit on the CPU, tests/test_gpu_pcg_wrap.py runs them on the device).  No GPU use.

`ipd_pcg` runs as ONE workgroup of BT = 512 threads: every vector loop is `row += BT`, the triangular solves and
the IC(0) factorisation walk a row with the 64 lanes of a wave (`t += 64`, `u += 64`), and the Jacobi kernel
spreads a row over L = min(pick_lanes(nnz, N, 1), PCG_LANES_MAX) lanes.  The cases put N past one pass, rows past
64 entries, and L at 1, 2, 4, 8, 16 and 64.

Every matrix is symmetric positive definite (the two breakdown cases apart) and stored as sorted CSR.  The runs
compared with the oracle entry by entry are SHORT and of fixed length (`maxit` 1 or 8, `retol` 0): the late part
of a converged history amplifies a 1e-15 perturbation of the input past any useful bar, a fixed-length one keeps
it four orders of magnitude inside (test_pcg_cases.py measures every compared run).  Converged runs are compared
by iteration count, residual and d only."""
import functools

import numpy as np
import scipy.sparse as sp

from oracle import ipd_oracle as O
from tests import problems as PR


def _sorted(A):
    A = sp.csr_matrix(A, dtype=float)
    A.sum_duplicates()
    A.sort_indices()
    return A


# ---------------------------------------------------------------------------------------------------------
# matrices
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lap(N):
    """0.5 I + the weighted Laplacian of a random connected degree-3 graph; condition number about 40 (with
    hubs: 430-640) at N = 513 (one wave past one pass), 1100 (a ragged third pass), 2049 (a fifth pass of one
    row).  Mean row 8.9: L = 8."""
    return _sorted(PR.random_sym_graph_laplacian(N, deg=3, seed=10, eps=0.5))


@functools.lru_cache(maxsize=None)
def hubbed(N, hubs):
    """lap(N) plus the weighted Laplacian of a hub graph: each hub h is joined to cnt distinct random nodes
    j < h, consecutive hubs are joined to each other, weights 0.5 + U(0,1).  `hubs` is a tuple of (h, cnt).
    Row h then has more than cnt > 64 entries left of the diagonal, and the next hub's row references it."""
    rs = np.random.RandomState(7)
    rows, cols = [], []
    for h, cnt in hubs:
        rows += [h] * cnt
        cols += list(rs.choice(h, size=cnt, replace=False))
    for (h0, _), (h1, _) in zip(hubs, hubs[1:]):
        rows.append(h1)
        cols.append(h0)
    w = 0.5 + rs.random_sample(len(rows))
    W = sp.csr_matrix((w, (rows, cols)), shape=(N, N))
    W = W + W.T
    return _sorted(lap(N) + sp.diags(np.asarray(W.sum(axis=1)).ravel()) - W)


HUBS_513 = ((300, 150), (512, 200))
HUBS_1100 = ((400, 150), (700, 300), (1099, 200))


@functools.lru_cache(maxsize=None)
def diagonal(N=600):
    """L = 1 (mean row 1): distinct entries 1 .. 2."""
    return _sorted(sp.diags(1.0 + np.arange(N) / N))


@functools.lru_cache(maxsize=None)
def tridiagonal(N, shift=0.5):
    """L = 2 (mean row 3 - 2/N): the 1-D Laplacian plus a shift in [shift, shift + 0.5) on the diagonal (not
    constant, so that Jacobi differs from no preconditioner)."""
    dg = 2.0 + shift + 0.5 * ((7 * np.arange(N)) % 11) / 11.0
    return _sorted(sp.diags([-np.ones(N - 1), dg, -np.ones(N - 1)], [-1, 0, 1]))


@functools.lru_cache(maxsize=None)
def wide(N=600):
    """L = 16 (mean row about 130): a random degree-70 graph Laplacian plus 0.5 I."""
    return _sorted(PR.random_sym_graph_laplacian(N, deg=70, seed=3, eps=0.5))


@functools.lru_cache(maxsize=None)
def dense(N=600):
    """L = 64 = PCG_LANES_MAX (row N): G G'/N + 2 I, condition number about 3."""
    G = np.random.RandomState(2).randn(N, N)
    return _sorted(G @ G.T / N + 2.0 * np.eye(N))


@functools.lru_cache(maxsize=None)
def lanes4(N=700):
    """L = 4 (mean row in (4, 8]): a random degree-2 graph Laplacian plus 0.5 I."""
    return _sorted(PR.random_sym_graph_laplacian(N, deg=2, seed=10, eps=0.5))


@functools.lru_cache(maxsize=None)
def bigraph(m, n, mask, seed):
    """(Ae, nf): the rescaled Newton operator of a mask, F block = the n columns (Hybrid_AMG.m:17-24)."""
    s = mask_of(m, n, mask, seed)
    pd = PR.make_prob(m, n, s, pq_random=True)
    Ae = O.build_Ae(O.ASAt(s, pd["p"], pd["q"]), pd["T"], pd["p"], pd["q"], PR.BK1, PR.TK)[0]
    return _sorted(Ae), n


def mask_of(m, n, mask, seed):
    if mask == "tree":
        return PR.mask_tree(m, n, seed=seed)
    if mask == "tree_split":
        return PR.mask_tree(m, n, seed=seed, connect=False)
    if mask == "bernoulli":
        return PR.mask_bernoulli(m, n, 0.004, seed=seed)
    if mask == "hub":
        return PR.mask_hub(m, n, seed=seed)
    raise KeyError(mask)


BIG_M, BIG_N = 540, 530          # precd 5: nf = 530 and N - nf = 540 both exceed BT

# name -> (builder, expected lanes per row of k_pcg).  The oracle's and the device's PCG take the same matrix.
MATRICES = {
    "lap513": (lambda: lap(513), 8),
    "lap1100": (lambda: lap(1100), 8),
    "lap2049": (lambda: lap(2049), 8),
    "hub513": (lambda: hubbed(513, HUBS_513), 8),
    "hub1100": (lambda: hubbed(1100, HUBS_1100), 8),
    "diag600": (lambda: diagonal(600), 1),
    "tri777": (lambda: tridiagonal(777), 2),
    "lanes4_700": (lambda: lanes4(700), 4),
    "wide600": (lambda: wide(600), 16),
    "dense600": (lambda: dense(600), 64),
    "big5": (lambda: bigraph(BIG_M, BIG_N, "tree", 1)[0], 4),
    "tri7000": (lambda: tridiagonal(7000), 2),
    "tri7001": (lambda: tridiagonal(7001), 2),
    "one": (lambda: _sorted(np.array([[2.5]])), 1),                       # pcg_single
    "two": (lambda: _sorted(np.array([[2.0, -1.0], [-1.0, 3.0]])), 2),    # precd 5 with nf = 1
}
LANE_CASES = ("diag600", "tri777", "lanes4_700", "lap513", "wide600", "dense600")
LAP_CASES = ("lap513", "lap1100", "lap2049")
HUB_CASES = ("hub513", "hub1100")


def matrix(name):
    return MATRICES[name][0]()


def rhs(name):
    N = matrix(name).shape[0]
    return np.random.RandomState(11).randn(N)


def guess(name):
    N = matrix(name).shape[0]
    return 0.1 * np.random.RandomState(3).randn(N)


# ---------------------------------------------------------------------------------------------------------
# the runs compared with O.PCG: (matrix, precd) per probe
# ---------------------------------------------------------------------------------------------------------
# A: one iteration from a zero guess, d = alpha * M^-1 e
PROBE_A = ([(c, p) for c in HUB_CASES + ("lap2049",) for p in (3, 4)] + [("big5", 5)] +
           [(c, p) for c in LANE_CASES for p in (1, 2)])
# B: eight iterations from a nonzero guess.  precd 1 on the hub matrices is not a case: under the perturbation of
# test_pcg_cases.py its d moves to within 1.5-1.7x of the bar (every run below keeps a margin of 5e4 or more).
# Jacobi solves the diagonal matrix in one step.
PROBE_B = ([(c, p) for c in dict.fromkeys(LAP_CASES + LANE_CASES) for p in (1, 2) if (c, p) != ("diag600", 2)] +
           [(c, p) for c in HUB_CASES for p in (2, 3, 4)] + [("big5", 5)])
# C: converged; precd 3, 4 and 5 (one wave walks the rows) at no more than about 1100 rows
CONVERGED = [("lap2049", 1), ("lap2049", 2), ("dense600", 1), ("dense600", 2), ("hub1100", 3), ("hub1100", 4),
             ("big5", 5)]
# E: the largest system the LDS-resident solve takes
LDS_BOUND = [("tri7000", 3), ("tri7000", 4)]
# D: the small ends, (matrix, precd, kind): 'D' from a zero guess, 'Dg' from a nonzero one
SMALL = [("one", 1, "D"), ("one", 1, "Dg"), ("one", 2, "D"), ("one", 2, "Dg"), ("one", 3, "D"), ("one", 4, "D"),
         ("two", 5, "D")]


def options(kind, name, precd):
    """pcg_options of a run: kind 'A' (preconditioner probe), 'B' (recurrence probe), 'C' (converged),
    'D' / 'Dg' (small ends, without / with a guess)."""
    o = dict(precd=precd)
    if kind == "A":
        o.update(guess=None, retol=0.0, maxit=1)
    elif kind == "B":
        o.update(guess=guess(name), retol=0.0, maxit=8)
    elif kind == "C":
        o.update(guess=None, retol=1e-11, maxit=3000)
    elif kind in ("D", "Dg"):
        o.update(guess=guess(name) if kind == "Dg" else None, retol=1e-11, maxit=10)
    else:
        raise KeyError(kind)
    if precd == 5:
        o["nf"] = BIG_N if name == "big5" else 1
    return o


@functools.lru_cache(maxsize=None)
def reference(kind, name, precd):
    """(d, it, res, resk) of the oracle; computed once, shared, never written to."""
    d, it, res, resk = O.PCG(matrix(name), rhs(name), options(kind, name, precd))
    d.setflags(write=False)
    resk.setflags(write=False)
    return d, it, res, resk


# ---------------------------------------------------------------------------------------------------------
# breakdown: IC(0) meets a nonpositive or a structurally missing pivot
# ---------------------------------------------------------------------------------------------------------
PIVOT_ROW = 800


@functools.lru_cache(maxsize=None)
def pivot_breakdown():
    """hubbed(1100) with H[800, 800] lowered to half of sum_j L(800, j)^2: the pivot of row 800 is
    -0.5 * that sum, negative in any summation order; the rows before it factor as before."""
    H = hubbed(1100, HUBS_1100).tolil()
    Lc = O.ichol0(hubbed(1100, HUBS_1100)).tocsr()
    row = Lc[PIVOT_ROW].toarray().ravel()
    H[PIVOT_ROW, PIVOT_ROW] = 0.5 * float(np.sum(row[:PIVOT_ROW] ** 2))
    return _sorted(H)


MISSING_ROW = 550


@functools.lru_cache(maxsize=None)
def missing_diagonal():
    """lap(600) without the stored diagonal entry of row 550."""
    H = lap(600).tocoo()
    keep = ~((H.row == MISSING_ROW) & (H.col == MISSING_ROW))
    A = sp.csr_matrix((H.data[keep], (H.row[keep], H.col[keep])), shape=H.shape)
    A.sort_indices()
    return A


# ---------------------------------------------------------------------------------------------------------
# aug_PCG / PCG4POT: the four 330 x 300 masks
# ---------------------------------------------------------------------------------------------------------
AUG_M, AUG_N = 330, 300
AUG_MASKS = [("tree", 1), ("tree_split", 2), ("bernoulli", 4), ("hub", 4)]
AUG_OPTS = dict(retol=1e-11, maxit=10000, precd=2, guess=None)


@functools.lru_cache(maxsize=None)
def aug_problem(mask, seed, pot=False):
    """prob_data of aug_PCG (pot: of PCG4POT, with t ~ Bernoulli(0.7), phi = 0.5 + U and a bordered z)."""
    m, n = AUG_M, AUG_N
    s = mask_of(m, n, mask, seed)
    t = (np.random.RandomState(9).random_sample(m + n) < 0.7).astype(float) if pot else None
    pd = PR.make_prob(m, n, s, t=t, pq_random=True)
    pd["H0"] = O.ASAt(s, pd["p"], pd["q"])
    if pot:
        pd["z"] = np.random.RandomState(5).randn(m + n + 1)
        pd["phi"] = 0.5 + np.random.RandomState(6).random_sample(m * n)
    return pd


def aug_direct(pd):
    """zeta of aug_PCG by a sparse direct solve of bk1 I + (T + H0)/tk."""
    M = pd["m"] + pd["n"]
    J = pd["bk1"] * sp.identity(M) + (pd["T"] + pd["H0"]) / pd["tk"]
    return sp.linalg.spsolve(sp.csc_matrix(J), pd["z"][:M])


def pot_direct(pd):
    """zeta of PCG4POT by a dense solve of the bordered Jacobian (APD_SsN_Class2.m:152-156):
    J = bk1 I + ([T 0; 0 0] + [H0 ss; ss' phi'(s.*phi)])/tk with ss = Ax(s.*phi)."""
    M = pd["m"] + pd["n"]
    sphi = np.asarray(pd["s"], float) * pd["phi"]
    ss = O.Ax(sphi, pd["p"], pd["q"])
    B = np.zeros((M + 1, M + 1))
    B[:M, :M] = (pd["T"] + pd["H0"]).toarray()
    B[:M, M] = ss
    B[M, :M] = ss
    B[M, M] = pd["phi"] @ sphi
    J = pd["bk1"] * np.eye(M + 1) + B / pd["tk"]
    return np.linalg.solve(J, pd["z"]), J


@functools.lru_cache(maxsize=None)
def aug_reference(mask, seed, pot=False):
    pd = aug_problem(mask, seed, pot)
    return (O.PCG4POT if pot else O.aug_PCG)(pd, AUG_OPTS)
