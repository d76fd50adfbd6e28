"""The inputs of tests/test_gpu_pcg_wrap.py (tests/pcg_cases.py) are fit for the bars applied there.  CPU only.

a. structure: every size sits on the intended side of the workgroup's BT threads and of its multiples, the hub
   rows have more than 64 entries left of the diagonal and are referenced by a later row, the lanes per row are
   the ones written next to the builders (`pick_lanes` itself, compiled from csrc/ipd_launch_plan.h);
b. stability: the oracle's answer to every compared run moves, under a 1e-15 relative perturbation of H and e,
   by less than a thousandth of the bar the device is held to -- a run that fails this cannot tell a wrong
   kernel from a rounding order, and is then not a case;
c. independence: the converged references of aug_PCG and PCG4POT agree with direct solves assembled in numpy;
d. breakdown: the oracle's IC(0) raises on both breakdown cases, on the pivot case exactly at row 800."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ipd_oracle as O
from tests import pcg_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "codes_of_ipd_ssn_amg_method_amd", "csrc")
LIMITS = open(os.path.join(CSRC, "ipd_limits.h")).read()


def _const(name):
    return int(re.search(r"static constexpr int %s = (\d+);" % name, LIMITS).group(1))


BT = _const("BT")
PCG_LANES_MAX = _const("PCG_LANES_MAX")
WAVE = 64
GEN_ROWS_MAX = 7000     # pcg_dev: rows of the LDS-resident solve (precd 3, 4, 5)

# the bars of test_gpu_pcg_wrap.py (test_gpu_cycle.py's), and the margin a reference must keep inside them
D_RTOL, D_ATOL, RESK_RTOL, RESK_ATOL, MARGIN = 1e-8, 1e-10, 1e-6, 1e-8, 1000.0

LANES_SRC = r"""
#include <cstdio>
#include <cstdlib>
#include "ipd_launch_plan.h"
int main(int argc, char** argv) {
    for (int i = 1; i + 1 < argc; i += 2)
        std::printf("%d\n", std::min(pick_lanes(std::atoll(argv[i]), std::atoi(argv[i + 1]), 1), PCG_LANES_MAX));
    return 0;
}
"""


@pytest.fixture(scope="module")
def lanes(tmp_path_factory):
    """name -> L as pcg_dev computes it."""
    d = tmp_path_factory.mktemp("pcg_lanes")
    src, exe = str(d / "lanes.cpp"), str(d / "lanes")
    open(src, "w").write(LANES_SRC)
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-I" + CSRC, src, "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    names = list(C.MATRICES)
    args = [str(v) for n in names for v in (C.matrix(n).nnz, C.matrix(n).shape[0])]
    out = subprocess.run([exe] + args, capture_output=True, text=True, check=True).stdout.split()
    return dict(zip(names, (int(v) for v in out)))


# ---------------------------------------------------------------------------------------------------------
# a. structure
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.MATRICES))
def test_matrix_is_sorted_symmetric_positive_definite(name):
    A = C.matrix(name)
    assert sp.isspmatrix_csr(A) and A.has_sorted_indices and A.shape[0] == A.shape[1]
    key = np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.indptr)) * A.shape[0] + A.indices
    assert np.all(np.diff(key) > 0)                               # strictly ascending columns, no duplicates
    # build_Ae scales rows and columns in two products: symmetric up to the last bit
    assert abs(A - A.T).max() <= 4 * np.finfo(float).eps * abs(A).max()
    assert np.all(A.diagonal() > 0)
    if A.shape[0] <= 2100:
        assert np.linalg.eigvalsh(A.toarray())[0] > 0
    else:                     # the tridiagonal matrices: strictly diagonally dominant
        assert np.all(2 * A.diagonal() > np.asarray(abs(A).sum(axis=1)).ravel())


def test_lanes_per_row_are_the_intended_ones(lanes):
    for name, (_, L) in C.MATRICES.items():
        assert lanes[name] == L, (name, lanes[name], L)
    got = {lanes[n] for n in C.LANE_CASES}
    assert got == {1, 2, 4, 8, 16, PCG_LANES_MAX}                 # both ends and everything between but 32
    for n in C.LANE_CASES:                                        # ... each with more than one row pass
        assert C.matrix(n).shape[0] > BT // lanes[n] and C.matrix(n).shape[0] > BT


def test_sizes_sit_past_the_intended_passes():
    N = {n: C.matrix(n).shape[0] for n in C.MATRICES}
    assert N["lap513"] == BT + 1                                  # a second pass of one row
    assert 2 * BT < N["lap1100"] < 3 * BT and (N["lap1100"] - 2 * BT) % WAVE != 0     # a ragged third pass
    assert N["lap2049"] == 4 * BT + 1                             # a fifth pass of one row
    assert N["hub513"] == BT + 1 and 2 * BT < N["hub1100"] < 3 * BT
    assert N["tri7000"] == GEN_ROWS_MAX and N["tri7001"] == GEN_ROWS_MAX + 1
    assert 8 * GEN_ROWS_MAX + 8 * 16 + 4 <= 60 * 1024              # k_pcg_gen's LDS: unknowns, reduction slots, fail word
    assert N["one"] == 1 and N["two"] == 2
    Ae, nf = C.bigraph(C.BIG_M, C.BIG_N, "tree", 1)               # precd 5: both blocks take a second pass
    assert nf > BT and Ae.shape[0] - nf > BT and Ae.shape[0] <= GEN_ROWS_MAX
    assert abs(Ae[:nf, :nf] - sp.diags(Ae.diagonal()[:nf])).max() == 0        # bipartite: the blocks are diagonal
    assert abs(Ae[nf:, nf:] - sp.diags(Ae.diagonal()[nf:])).max() == 0


@pytest.mark.parametrize("name,hubs", [("hub513", C.HUBS_513), ("hub1100", C.HUBS_1100)])
def test_hub_rows_wrap_the_wave_and_are_referenced_later(name, hubs):
    A = C.matrix(name)
    lower = np.diff(sp.tril(A, -1, format="csr").indptr)
    wrapped = 0
    for h, cnt in hubs:
        assert WAVE < cnt <= lower[h] and 130 <= lower[h] <= 310
        later = A[h].indices[A[h].indices > h]
        if later.size:                 # pcg_ichol0 walks row h (u += 64) for every later row that references it
            wrapped += 1
    assert wrapped >= len(hubs) - 1 and wrapped >= 1
    # and rows of more than 64 entries in all, for the t += 64 loops of the triangular solves
    assert (np.diff(A.indptr) > WAVE).sum() >= len(hubs)


@pytest.mark.parametrize("mask,seed", C.AUG_MASKS)
def test_augmented_systems_take_a_second_pass(mask, seed):
    pd = C.aug_problem(mask, seed)
    nc = len(O.components(O.build_Ae(pd["H0"], pd["T"], pd["p"], pd["q"], pd["bk1"], pd["tk"])[1])[1])
    assert C.AUG_M + C.AUG_N + nc > BT
    assert C.aug_reference(mask, seed)[3][0] == nc
    if mask == "hub":                  # k_aug_fill: a row of more than 64 entries (t += 64 wraps)
        assert np.diff(sp.csr_matrix(pd["H0"]).indptr).max() > 4 * WAVE
    if mask == "bernoulli":            # a component row of more than 64 members
        assert O.components(pd["H0"])[1].max() > WAVE


# ---------------------------------------------------------------------------------------------------------
# b. stability of the references
# ---------------------------------------------------------------------------------------------------------
def perturbed(H, e, seed):
    """H .* (1 + 1e-15 G) with G symmetric standard normal, e .* (1 + 1e-15 g)."""
    rs = np.random.RandomState(1000 + seed)
    Hc = sp.coo_matrix(H)
    lo, hi = np.minimum(Hc.row, Hc.col), np.maximum(Hc.row, Hc.col)
    _, inv = np.unique(lo.astype(np.int64) * H.shape[0] + hi, return_inverse=True)
    g = rs.randn(inv.max() + 1)[inv]
    Hp = sp.csr_matrix((Hc.data * (1.0 + 1e-15 * g), (Hc.row, Hc.col)), shape=H.shape)
    Hp.sort_indices()
    return Hp, e * (1.0 + 1e-15 * rs.randn(e.size))


RUNS = ([("A", c, p) for c, p in C.PROBE_A] + [("B", c, p) for c, p in C.PROBE_B] +
        [("C", c, p) for c, p in C.CONVERGED] + [("A", c, p) for c, p in C.LDS_BOUND] +
        [(k, c, p) for c, p, k in C.SMALL])


@pytest.mark.parametrize("kind,name,precd", RUNS, ids=["%s-%s-p%d" % r for r in RUNS])
def test_reference_is_stable(kind, name, precd):
    d0, it0, _, resk0 = C.reference(kind, name, precd)
    o = C.options(kind, name, precd)
    k = it0 if kind in ("A", "B") else 0            # the compared part of the history: all of a probe's
    if kind in ("A", "B"):
        assert it0 == o["maxit"]
    else:
        assert it0 < o["maxit"]
    worst_d = worst_r = 0.0
    for seed in range(5):
        Hp, ep = perturbed(C.matrix(name), C.rhs(name), seed)
        d, it, _, resk = O.PCG(Hp, ep, o)
        assert it == it0, (seed, it, it0)
        worst_d = max(worst_d, np.max(np.abs(d - d0) / (D_ATOL + D_RTOL * np.abs(d0))))
        if k:
            worst_r = max(worst_r, np.max(np.abs(resk[:k] - resk0[:k]) / (RESK_ATOL + RESK_RTOL * np.abs(resk0[:k]))))
    print("%s %s precd %d: d at 1/%.3g of its bar, resk at 1/%.3g" %
          (kind, name, precd, 1 / max(worst_d, 1e-300), 1 / max(worst_r, 1e-300)))
    assert worst_d * MARGIN <= 1.0 and worst_r * MARGIN <= 1.0, (worst_d, worst_r)


# ---------------------------------------------------------------------------------------------------------
# c. independence of the converged references
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask,seed", C.AUG_MASKS)
def test_aug_pcg_reference_matches_a_direct_solve(mask, seed):
    pd = C.aug_problem(mask, seed)
    z, it, res, info = C.aug_reference(mask, seed)
    ref = C.aug_direct(pd)
    assert it < C.AUG_OPTS["maxit"] and info[1] == 1
    assert np.linalg.norm(z - ref) <= 1e-9 * np.linalg.norm(ref)


@pytest.mark.parametrize("mask,seed", C.AUG_MASKS)
def test_pcg4pot_reference_matches_a_dense_solve(mask, seed):
    pd = C.aug_problem(mask, seed, pot=True)
    z, it, res, info = C.aug_reference(mask, seed, pot=True)
    ref, J = C.pot_direct(pd)
    assert abs(J - J.T).max() == 0 and it < C.AUG_OPTS["maxit"]
    assert np.linalg.norm(z - ref) <= 1e-9 * np.linalg.norm(ref)
    assert np.linalg.norm(J @ ref - pd["z"]) <= 1e-12 * np.linalg.cond(J) * np.linalg.norm(pd["z"])


# ---------------------------------------------------------------------------------------------------------
# d. breakdown
# ---------------------------------------------------------------------------------------------------------
def test_pivot_breakdown_is_at_row_800():
    H = C.pivot_breakdown()
    r = C.PIVOT_ROW
    assert r > BT and abs(H - H.T).max() == 0 and H.has_sorted_indices
    O.ichol0(H[:r, :r])                                           # the rows before factor
    with pytest.raises(ValueError, match="nonpositive pivot"):
        O.ichol0(H[:r + 1, :r + 1])
    with pytest.raises(ValueError, match="nonpositive pivot"):
        O.ichol0(H)
    # far from the edge: the pivot is -(half the row's squares), not a rounding accident
    Lc = O.ichol0(C.hubbed(1100, C.HUBS_1100)).tocsr()
    sq = float(np.sum(Lc[r].toarray().ravel()[:r] ** 2))
    assert H[r, r] - sq <= -0.4 * sq < 0


def test_missing_diagonal_breaks_down_past_one_pass():
    H = C.missing_diagonal()
    r = C.MISSING_ROW
    assert r > BT and H.shape[0] > r and H.has_sorted_indices and abs(H - H.T).max() == 0
    assert r not in H[r].indices and H.nnz == C.lap(600).nnz - 1
    O.ichol0(H[:r, :r])
    with pytest.raises(ValueError, match="nonpositive pivot"):
        O.ichol0(H[:r + 1, :r + 1])
