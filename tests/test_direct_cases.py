"""The cases of tests/direct_cases.py, proven on the CPU: every case lands on the side of each geometry edge it
is named for (the constants come out of csrc/ipd_dense.hip, not from a copy here), LAPACK's or the oracle's own
backward error stays under a tenth of the bar the device has to meet, and the failure inputs fail where they are
meant to.  CPU only."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ipd_oracle as O
from tests import direct_cases as C


def test_longdouble_is_the_80_bit_format():
    assert np.finfo(C.LD).eps < 2e-19


def test_bar():
    assert C.bar(1) == 7 * C.U and C.bar(64) == (3 * 4096 + 4) * 2.0 ** -53
    assert 1.3e-12 < C.bar(63) < 1.4e-12 and 3.3e-12 < C.bar(100) < 3.4e-12


# ---------------------------------------------------------------------------------------------------------
# A
# ---------------------------------------------------------------------------------------------------------
def test_constants_read_from_the_source():
    r = C.dense_rules()
    assert set(r) == {"DNB", "panel", "diag", "width", "cap"} and all(v > 0 for v in r.values())
    assert C.hybrid_n0() > 0


def test_the_case_list_is_the_one_the_edges_are_named_for():
    assert len(C.SPD_CASES) == len(set(C.SPD_CASES)) == 5 * 7 + 4 * 2 + 1
    assert {n for n, _ in C.SPD_CASES} == set(C.N_EDGES)
    assert {k for _, k in C.SPD_CASES} == set(C.NRHS_EDGES)
    for n in C.SMALL_N:
        assert {k for m, k in C.SPD_CASES if m == n} == set(C.ALL_NRHS)


@pytest.mark.parametrize("n,nrhs", C.SPD_CASES)
def test_every_case_lands_on_its_side_of_each_edge(n, nrhs):
    g = C.geometry(n, nrhs)
    assert (g["blocks"], g["last_nb"], g["panel_wgs"]) == C.N_EDGES[n]
    assert (g["diag_wgs"], g["tile_cols"]) == C.NRHS_EDGES[nrhs]
    assert g["strides"] == ((n, nrhs) == C.STRIDE_CASE)


def test_the_edges_are_all_there():
    r = C.dense_rules()
    g = {c: C.geometry(*c) for c in C.SPD_CASES}
    ns = {n for n, _ in C.SPD_CASES}
    # an exact multiple of the block, one short of it and one past it
    assert {r["DNB"] - 1, r["DNB"], r["DNB"] + 1, 2 * r["DNB"], 2 * r["DNB"] + 1} <= ns
    # exactly one panel workgroup's worth of rows below the first block, and one row more
    assert {r["DNB"] + r["panel"], r["DNB"] + r["panel"] + 1} <= ns
    assert g[(320, 1)]["panel_wgs"] == 1 and g[(321, 1)]["panel_wgs"] == 2
    # the last right-hand side of the first k_trsm_diag workgroup and the first of the second, on every small n
    ks = {k for _, k in C.SPD_CASES}
    assert {r["diag"] - 1, r["diag"], r["diag"] + 1} <= ks and {1, r["DNB"], r["DNB"] + 1} <= ks
    assert all(g[(n, 257)]["diag_wgs"] == 2 for n in ns - {C.STRIDE_CASE[0]})
    # only the last case strides, and it does so with a ragged second trip
    n, k = C.STRIDE_CASE
    total, grid = n * k, r["cap"] * r["width"]
    assert grid < total < 2 * grid and [c for c in g if g[c]["strides"]] == [C.STRIDE_CASE]


@pytest.mark.parametrize("n", sorted(C.N_EDGES))
def test_lapack_meets_a_tenth_of_the_bar(n):
    A, nrm = C.spd_matrix(n)
    assert abs(A - A.T).max() == 0.0
    worst = 0.0
    for m, k in C.SPD_CASES:
        if m == n:
            B = C.spd_rhs(n, k)
            e = C.eta(A, C.lapack_solve(A, B), B, nrm)
            assert e.shape == (k,)
            worst = max(worst, e.max() / C.bar(n))
    print("n = %d: LAPACK's worst eta / bar = %.3g" % (n, worst))
    assert worst <= 0.1


def test_eta_sees_a_wrong_column():
    """one entry of one column off by 1e-9 relative: that column, and only that, leaves the bar"""
    n, k = 65, 64
    A, nrm = C.spd_matrix(n)
    B = C.spd_rhs(n, k)
    X = C.lapack_solve(A, B)
    X[64, 17] *= 1.0 + 1e-9
    e = C.eta(A, X, B, nrm)
    assert e[17] > C.bar(n) and np.all(np.delete(e, 17) <= 0.1 * C.bar(n))


# ---------------------------------------------------------------------------------------------------------
# B
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", C.FAIL_AT)
def test_the_bad_pivot_is_the_first_to_fail(at):
    r = C.dense_rules()
    A = C.bad_pivot(at).toarray()
    assert A.shape == (C.FAIL_N, C.FAIL_N) and np.array_equal(A, A.T)
    np.linalg.cholesky(A[:at, :at])                              # every pivot before it is positive
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(A[:at + 1, :at + 1])
    L = np.linalg.cholesky(C.spd_matrix(C.FAIL_N)[0].toarray()[:at, :at])
    l = np.linalg.solve(L, A[:at, at])
    assert A[at, at] - l @ l <= -1.0
    g = C.geometry(C.FAIL_N, 1)
    assert g["blocks"] == 3 and g["last_nb"] == 2
    assert at // r["DNB"] == {100: 1, 129: 2}[at] and (at != 129 or at == C.FAIL_N - 1)


def test_the_nan_sits_below_the_first_block():
    r = C.dense_rules()
    A = C.nan_entry().toarray()
    bad = np.argwhere(np.isnan(A))
    assert sorted(map(tuple, bad)) == [(70, 100), (100, 70)]
    assert 70 // r["DNB"] == 1 and 100 // r["DNB"] == 1 and 70 % r["DNB"] > 0


def test_the_limit_cases_sit_one_past_the_limits():
    two_gib = 2 << 30
    assert (C.LIMIT_ORDER - 1) ** 2 * 8 <= two_gib < C.LIMIT_ORDER ** 2 * 8
    assert C.LIMIT_NRHS == (1 << 20) + 1
    # ipd_spd_solve states both rules before it allocates the dense array
    import os
    with open(os.path.join(C.CSRC, "ipd_dense.hip")) as fh:
        body = fh.read()
    body = body[body.index('extern "C" int ipd_spd_solve('):]
    assert "nrhs <= (1 << 20)" in body and "(size_t(2) << 30)" in body
    alloc = body.index("tmp.alloc<double>")
    assert body.index("mldivide: too many right-hand sides") < body.index("mldivide: dense scratch above 2 GiB") < alloc


# ---------------------------------------------------------------------------------------------------------
# C
# ---------------------------------------------------------------------------------------------------------
def test_system_is_hybrid_plans_builder_with_full_blocks():
    """the same p, q, z, T and layout as tests/test_hybrid_plan.py's `_system`; the mask of each block complete"""
    from tests.test_hybrid_plan import _system
    blocks, t_on = ((3, 3), (1, 0), (4, 2), (0, 1)), (2,)
    a, b = C.system(blocks, t_on), _system(blocks, t_on)
    for key in ("p", "q", "z"):
        assert np.array_equal(a[key], b[key])
    assert abs(a["T"] - b["T"]).nnz == 0 and (a["m"], a["n"]) == (b["m"], b["n"])
    Ya, Yb = a["s"].reshape(a["m"], a["n"], order="F"), b["s"].reshape(a["m"], a["n"], order="F")
    assert np.all(Ya >= Yb) and Ya.sum() == 3 * 3 + 4 * 2
    assert np.array_equal(O.components(a["H0"])[0], O.components(b["H0"])[0])


@pytest.mark.parametrize("name", list(C.SMALL_SYSTEMS))
def test_small_systems_are_small_components_only(name):
    N0 = C.hybrid_n0()
    pd, Ae, qp, f, comps = C.small_system(name)
    sizes = np.array([len(pk) for pk in comps])
    assert sizes.sum() == pd["m"] + pd["n"] and sizes.max() == N0 and len(sizes) > 1
    if name == "all_sizes":
        assert set(sizes) == C.SMALL_SIZES and len(sizes) == 309 > 256
        assert N0 - 1 in sizes and {63, 64, 65} <= set(sizes)
        dT = pd["T"].diagonal()
        assert sorted(len(pk) for pk in comps if dT[pk].all()) == [64, 99] and dT.sum() == 64 + 99
    else:
        assert sorted(sizes) == [1, 1, 1, N0]
    # every block of more than two nodes fills: its factor has entries where Ae has none
    for pk in comps:
        if len(pk) > 3:
            Ak = Ae[pk, :][:, pk].toarray()
            assert np.count_nonzero(np.linalg.cholesky(Ak)) > np.count_nonzero(np.tril(Ak))


@pytest.mark.parametrize("name", list(C.SMALL_SYSTEMS))
def test_the_oracle_meets_a_tenth_of_the_bar_on_every_small_block(name):
    z, it, res, info, used = C.small_reference(name)
    comps = C.small_system(name)[4]
    assert (it, res, list(info), used) == (0, 0.0, [len(comps), 0], 0)
    es = C.small_etas(name, z)
    worst = max(e / C.bar(nb) for nb, e in es)
    print("%s: the oracle's worst eta / bar = %.3g" % (name, worst))
    assert len(es) == len(comps) and worst <= 0.1


def test_the_indefinite_block_is_the_second_of_64_nodes():
    pd, node, blk = C.indefinite_system()
    out = O.build_Ae(pd["H0"], pd["T"], pd["p"], pd["q"], pd["bk1"], pd["tk"])
    Ae = sp.csr_matrix(out[0])
    lab, sizes, ps, rs = O.components(out[1])
    assert list(sizes) == [2, 64, 64, 1] and lab[node] == 2
    assert np.array_equal(np.sort(ps[rs[2]:rs[3]]), np.sort(blk)) and list(np.sort(blk)).index(node) == 32 + 7
    assert Ae[node, node] <= -0.999
    for k, want in ((1, True), (2, False)):
        pk = np.sort(ps[rs[k]:rs[k + 1]])
        assert (np.linalg.eigvalsh(Ae[pk, :][:, pk].toarray())[0] > 0) == want


# ---------------------------------------------------------------------------------------------------------
# D
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [1, 2])
def test_the_driver_references_take_all_their_iterations(cls):
    r = C.dense_rules()
    M = C.DRIVER_M + C.DRIVER_N
    assert C.cdiv(M, r["DNB"]) == 5 and M + 1 == 272 > 256           # five blocks; k_border's second workgroup
    start, ref = C.driver_reference(cls)
    assert not ref["converged"] and ref["k"] == C.DRIVER_K
    assert len(ref["KKT_xk"]) == C.DRIVER_K + 1 and min(ref["SsN_itnum"]) >= 1


# ---------------------------------------------------------------------------------------------------------
# E
# ---------------------------------------------------------------------------------------------------------
def test_the_ideal_interpolation_case_has_both_sides_past_256():
    r = C.dense_rules()
    isC = C.ideal_reference(0)[2]
    Nc, Nf = int(isC.sum()), int((~isC).sum())
    assert Nc > r["diag"] and Nf > r["DNB"] + r["panel"]             # k_trsm_diag's and k_trsm_panel's second workgroup
    assert np.array_equal(isC, C.ideal_reference(1)[2])
    nf, es = C.ideal_etas(C.ideal_reference(0)[1], isC)
    print("ideal interpolation: the oracle's worst eta / bar = %.3g" % (es.max() / C.bar(nf)))
    assert nf == Nf and es.shape == (Nc,) and es.max() <= 0.1 * C.bar(nf)
