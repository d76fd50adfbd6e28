"""The AMG setup, ASAt, Ax and Aty at the DRIVER sizes (m = n = 1024 to 4096) against the oracle.

tests/test_gpu_setup.py holds every setup kernel to the oracle bit for bit, but on systems of at most ~560
unknowns: below the sizes where the setup's size-gated paths switch on.  Here the same bar -- level sizes, J,
A(k), P(k), cmask(k) with the same indptr, indices and data bits, and the same number of random numbers
consumed -- is applied to systems that reach each gate:

  lazy counts        N*Nc <= SPGEMM_LAZY_MAX and a previous hierarchy's hints (plan_transfer, csrc/ipd_setup_plan.h)
  head scans         N <= SCAN_HEAD_MAX (the consumers scan plain counts themselves: plan_row_count)
  ScanTail products  N > SCAN_HEAD_MAX (the last workgroup scans the counts)
  large mis_set      N > MIS_SMALL_ROWS or nnz > MIS_SMALL_NNZ (amg_mis_set instead of mis_set_small: plan_mis_small)
  split interpolation  nnz / N >= 256

Every system asserts, from the ORACLE's hierarchy, that it reaches the gates it is listed for (`GATES`), so a
moved threshold or a changed generator fails here instead of silently testing something else.  The thresholds
and the three gate helpers below are the planner's own: tests/setup_plan_driver.cpp, built against the header the
library compiles, reports its limits and the plan of a level shape, and test_planner_reports_the_gates holds the
planner's decisions to what `GATES` asserts (CPU only, like test_oracle_systems_reach_their_gates).

Oracle CPU time per call measured for this file (one x86 core): amg_setup 0.02 s (5 components) / 0.05-0.1 s
(trees 1024-2048) / 0.36 s (tree 4096) / 0.45 s (Bernoulli 1024 and 2048) / 1.4 s (hub 1024, level 2 fully
dense); Hybrid_AMG 0.07-0.75 s on the same systems; ASAt up to ~1 s at 4096 x 4096.  The GPU tests of the
file (76) ran in 13 s on one MI355X, the two driver captures included."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ipd_oracle as O
from tests import problems as PR
from tests import test_setup_plan as SP

gpu = pytest.mark.gpu

# the thresholds, from the planner (the `limits` line of tests/setup_plan_driver.cpp)
SPGEMM_LAZY_MAX = SP.limits()["SPGEMM_LAZY_MAX"]
SCAN_HEAD_MAX = SP.limits()["SCAN_HEAD_MAX"]
MIS_SMALL_ROWS = SP.limits()["MIS_SMALL_ROWS"]
MIS_SMALL_NNZ = SP.limits()["MIS_SMALL_NNZ"]


@pytest.fixture(scope="module")
def ipd():
    import codes_of_ipd_ssn_amg_method_amd as m
    return m


def csc_equal(A, B):
    A = sp.csc_matrix(A); B = sp.csc_matrix(B)
    A.sort_indices(); B.sort_indices()
    return (A.shape == B.shape and np.array_equal(A.indptr, B.indptr)
            and np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data))


# ---------------------------------------------------------------------------------------------------------------
# the systems: the largest component of build_Ae(ASAt(s, p, q), ...) with random p and q, fnode as Hybrid_AMG
# sets it (Hybrid_AMG.m:55-68: pk ascending, the F side first)
# ---------------------------------------------------------------------------------------------------------------
SYSTEMS = {
    "tree1024": (1024, 1024, lambda: PR.mask_tree(1024, 1024, seed=6)),
    "tree1024x1025": (1024, 1025, lambda: PR.mask_tree(1024, 1025, seed=6)),
    "hub1024": (1024, 1024, lambda: PR.mask_hub(1024, 1024, seed=6)),
    "bern1024": (1024, 1024, lambda: PR.mask_bernoulli(1024, 1024, 0.04, seed=6)),
    "tree2048": (2048, 2048, lambda: PR.mask_tree(2048, 2048, seed=6)),
    "tree2048x2049": (2048, 2049, lambda: PR.mask_tree(2048, 2049, seed=6)),
    "bern2048": (2048, 2048, lambda: PR.mask_bernoulli(2048, 2048, 0.01, seed=6)),
    "tree4096": (4096, 4096, lambda: PR.mask_tree(4096, 4096, seed=6)),
    "comp2048": (2048, 2048, lambda: PR.mask_tree(2048, 2048, extra=0.0, seed=3, connect=False)),
}
NEWTON = {"newton2048_k13": 12, "newton2048_k25": 24}   # capture(ipd, 2048, kcap) of test_gpu_resident_deep.py


@functools.lru_cache(maxsize=None)
def problem(name):
    m, n, mk = SYSTEMS[name]
    s = mk()
    pd = PR.make_prob(m, n, s, pq_random=True)
    pd["H0"] = O.ASAt(s, pd["p"], pd["q"])
    return pd


def largest_component(Ae, n):
    ncomp, lab = sp.csgraph.connected_components(Ae)
    pk = np.flatnonzero(lab == np.argmax(np.bincount(lab)))
    return sp.csr_matrix(Ae[pk, :][:, pk]), int((pk < n).sum()), ncomp


@functools.lru_cache(maxsize=None)
def system(name):
    """(Ae of the largest component, fnode, number of components of the whole system)."""
    pd = problem(name)
    Ae = O.build_Ae(pd["H0"], pd["T"], pd["p"], pd["q"], pd["bk1"], pd["tk"])[0]
    return largest_component(Ae, pd["n"])


_newton = {}


def newton_system(ipd, name):
    if name not in _newton:
        from tests.newton_capture import capture
        Ae, f, tk = capture(ipd, 2048, NEWTON[name])
        _newton[name] = largest_component(Ae, 2048)
    return _newton[name]


def get_system(ipd, name):
    return newton_system(ipd, name) if name in NEWTON else system(name)


def setup_options(fnode, isnsp):
    o = O.amg_options_class1("v")
    o.update(fnode=fnode, isnsp=isnsp)
    return o


_oracle = {}


def oracle_hierarchy(ipd, name, isnsp):
    key = (name, isnsp)
    if key not in _oracle:
        Ae, fnode, _ = get_system(ipd, name)
        _oracle[key] = O.amg_setup(Ae, setup_options(fnode, isnsp), O.matlab_rng())
    return _oracle[key]


def rand_used(ho):
    return sum(len(i["mis"]["rand"]) for i in ho.info[2:] if i and i.get("mis"))


def assert_same_hierarchy(h, ho, rng, tag):
    assert h.J == ho.J, tag
    assert h.level_sizes() == ho.level_sizes(), tag
    for k in range(1, ho.J + 1):
        assert csc_equal(h.A(k), ho.Ack[k]), f"{tag}: Ack{{{k}}} differs"
    for k in range(2, ho.J + 1):
        assert csc_equal(h.P(k), ho.Prok[k]), f"{tag}: Prok{{{k}}} differs"
        assert np.array_equal(h.cmask(k), ho.info[k]["isC"]), f"{tag}: cmask{{{k}}} differs"
    assert rng.consumed == rand_used(ho), tag


# ---------------------------------------------------------------------------------------------------------------
# the gates each system is listed for, read off the oracle's hierarchy.  Level k (1-based) has N = sizes[k-1]
# rows and nnz[k-1] entries; its transfer builds a P of N x Nc with Nc = sizes[k].
# ---------------------------------------------------------------------------------------------------------------
ANY_HINTS = (1, 1, 1, 1)   # the size part of a gate: what the planner says once a previous hierarchy left counts


def level_plan(sizes, nnz, k, hints=ANY_HINTS):
    """The planner's record of the transfer out of level k (level 1 is the bigraph level, as in every hierarchy
    of this file)."""
    z = nnz[k - 1] if nnz is not None else sizes[k - 1]
    return SP.transfer(k, sizes[k - 1], z, sizes[k], hints, bigph=1, fnode=sizes[0] - sizes[1])


def lazy_bounds_ok(sizes, k):
    """The size part of the lazy-count choice for the transfer out of level k (the hints are the other part)."""
    return level_plan(sizes, None, k)["lazy"] == 1


def large_mis(sizes, nnz, k):
    return level_plan(sizes, nnz, k)["mis_small"] == 0


def split_interp(sizes, nnz, k):
    return level_plan(sizes, nnz, k)["form"] == "SPLIT"


def _g_tree1024(s, z, nc):      # level 1 lazy with N*Nc = 2^21 exactly
    assert s[0] * s[1] == SPGEMM_LAZY_MAX and lazy_bounds_ok(s, 1)


def _g_tree1024x1025(s, z, nc):   # level 1 just over the lazy bound, head scan still on
    assert s[0] * s[1] > SPGEMM_LAZY_MAX and s[0] * s[1] - SPGEMM_LAZY_MAX <= s[1] and s[0] <= SCAN_HEAD_MAX
    assert not lazy_bounds_ok(s, 1)


def _g_hub1024(s, z, nc):       # level 2 fully dense: split interpolation, large mis_set by entry count
    assert z[1] == s[1] * s[1] and split_interp(s, z, 2)
    assert s[1] <= MIS_SMALL_ROWS and z[1] > MIS_SMALL_NNZ


def _g_bern1024(s, z, nc):      # level 2 with ~847 k entries and a tiny coarse level: split, large mis, lazy
    assert z[1] > 800_000 and split_interp(s, z, 2) and s[2] <= 16
    assert s[1] <= MIS_SMALL_ROWS and z[1] > MIS_SMALL_NNZ and lazy_bounds_ok(s, 2)


def _g_tree2048(s, z, nc):      # level 1 N = SCAN_HEAD_MAX; level 2 large mis_set by row count
    assert s[0] == SCAN_HEAD_MAX
    assert s[1] > MIS_SMALL_ROWS and z[1] <= MIS_SMALL_NNZ


def _g_tree2048x2049(s, z, nc):   # level 1 one row past the head scans
    assert s[0] == SCAN_HEAD_MAX + 1


def _g_bern2048(s, z, nc):      # dense level 2 at N = 2048
    assert s[1] == 2048 and split_interp(s, z, 2) and large_mis(s, z, 2)


def _g_tree4096(s, z, nc):      # level 1 counted through ScanTail; level 2 head scan but not lazy
    assert s[0] == 2 * SCAN_HEAD_MAX
    assert s[1] <= SCAN_HEAD_MAX and SPGEMM_LAZY_MAX < s[1] * s[2] < 1.5 * SPGEMM_LAZY_MAX
    assert not lazy_bounds_ok(s, 2) and large_mis(s, z, 2)


def _g_comp2048(s, z, nc):      # five components, the largest with seven levels
    assert nc == 5 and len(s) == 7


def _g_newton(s, z, nc):        # the driver's regime: ~4096 / 2048 / 640 / 190 / 55 / 15
    assert len(s) >= 5 and s[1] > MIS_SMALL_ROWS and s[0] > SCAN_HEAD_MAX // 2


GATES = {"tree1024": _g_tree1024, "tree1024x1025": _g_tree1024x1025, "hub1024": _g_hub1024,
         "bern1024": _g_bern1024, "tree2048": _g_tree2048, "tree2048x2049": _g_tree2048x2049,
         "bern2048": _g_bern2048, "tree4096": _g_tree4096, "comp2048": _g_comp2048,
         "newton2048_k13": _g_newton, "newton2048_k25": _g_newton}


def assert_gates(name, ho, ncomp):
    GATES[name](ho.level_sizes(), ho.level_nnz(), ncomp)


@functools.lru_cache(maxsize=None)
def oracle_hierarchy_cpu(name):
    """The oracle's hierarchy of a system of SYSTEMS with isnsp = 1 (no device: the captured Newton systems
    are not for this)."""
    Ae, fnode, _ = system(name)
    return O.amg_setup(Ae, setup_options(fnode, 1), O.matlab_rng())


# what GATES asserts of each system, as the planner's decisions: per level (form, mis_set in one launch, lazy
# with hints, P's row-count mode with hints and without); None: the gate does not speak of that level
PLANNED_GATES = {
    "tree1024": {1: ("BIGRAPH", None, 1, "HEAD", "TAIL_WAIT")},              # lazy at N*Nc = 2^21 exactly
    "tree1024x1025": {1: ("BIGRAPH", None, 0, "TAIL_WAIT", "TAIL_WAIT")},    # just over: counted, hints or not
    "hub1024": {2: ("SPLIT", 0, 1, "HEAD", "TAIL_WAIT")},                    # split, large mis_set by entries
    "bern1024": {2: ("SPLIT", 0, 1, "HEAD", "TAIL_WAIT")},                   # split, large mis_set, lazy
    "tree2048": {1: ("BIGRAPH", None, 0, "TAIL_WAIT", "TAIL_WAIT"),          # N = SCAN_HEAD_MAX, but 2^23 dense
                 2: ("WAVE", 0, 1, "HEAD", "SCAN_TOTAL")},                   # large mis_set by rows
    "tree2048x2049": {1: ("BIGRAPH", None, 0, "TAIL_WAIT", "TAIL_WAIT")},
    "bern2048": {2: ("SPLIT", 0, 1, "HEAD", "TAIL_WAIT")},
    "tree4096": {1: ("BIGRAPH", None, 0, "TAIL_WAIT", "TAIL_WAIT"),          # counted through ScanTail
                 2: ("WAVE", 0, 0, "SCAN_TOTAL", "SCAN_TOTAL")},             # head-scan size, but not lazy
    "comp2048": {k: ("WAVE", 1, 1, "HEAD", "SCAN_TOTAL") for k in range(3, 7)},   # the small levels of seven
}


def test_planner_reports_the_gates():
    """The rule behind every gate is run, not read: on the oracle's level shapes of every system the planner
    takes the paths `GATES` lists the system for, with hints (the second and third build of
    test_setup_at_the_gates) and without (the first)."""
    assert set(PLANNED_GATES) == set(SYSTEMS)
    for name in SYSTEMS:
        ho = oracle_hierarchy_cpu(name)
        sizes, nnz = ho.level_sizes(), ho.level_nnz()
        assert_gates(name, ho, system(name)[2])
        for k, (form, small, lazy, rows_hinted, rows_counted) in PLANNED_GATES[name].items():
            h, c = level_plan(sizes, nnz, k), level_plan(sizes, nnz, k, (0, 0, 0, 0))
            assert (h["form"], h["lazy"], h["lazy_prod"], h["rows"]) == (form, lazy, lazy, rows_hinted), (name, k, h)
            assert (c["form"], c["lazy"], c["lazy_prod"], c["rows"]) == (form, 0, 0, rows_counted), (name, k, c)
            if small is not None:
                assert h["mis_small"] == c["mis_small"] == small, (name, k, h)
    # the thresholds the gates were written against
    assert (SPGEMM_LAZY_MAX, SCAN_HEAD_MAX, MIS_SMALL_ROWS, MIS_SMALL_NNZ) == (1 << 21, 4096, 1024, 40000)
    assert SP.limits()["SPLIT_ROW_MIN"] == 256


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_oracle_systems_reach_their_gates(name):
    """The gate half of test_setup_at_the_gates, oracle only (the captured Newton systems need the device)."""
    assert_gates(name, oracle_hierarchy_cpu(name), system(name)[2])


# ---------------------------------------------------------------------------------------------------------------
# (a) hierarchies at the size gates: three builds on one fresh context (the first counted, the later ones lazy
#     wherever the bounds allow), each bit for bit against the oracle
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("isnsp", [0, 1])
@pytest.mark.parametrize("name", list(SYSTEMS) + list(NEWTON))
def test_setup_at_the_gates(ipd, name, isnsp):
    from codes_of_ipd_ssn_amg_method_amd import _lib
    Ae, fnode, ncomp = get_system(ipd, name)
    ho = oracle_hierarchy(ipd, name, isnsp)
    assert_gates(name, ho, ncomp)
    ctx = _lib.Context(0)
    try:
        for build in range(3):
            rng = ipd.MatlabRand()
            h = ipd.AMGHierarchy(Ae, setup_options(fnode, isnsp), rng, ctx=ctx)
            try:
                assert_same_hierarchy(h, ho, rng, (name, isnsp, build))
            finally:
                h.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# (b) hints left by a DIFFERENT system (the Newton loop and Hybrid_AMG's situation): one context, one ordered
#     sequence of builds, then the reverse order on another context
# ---------------------------------------------------------------------------------------------------------------
def component_systems(name):
    """Every component Hybrid_AMG solves with AMG (more than N0 = 100 nodes), in its visiting order."""
    pd = problem(name)
    Ae, A0 = O.build_Ae(pd["H0"], pd["T"], pd["p"], pd["q"], pd["bk1"], pd["tk"])[:2]
    blocks, sizes, ps, rs = O.components(A0)
    out = []
    for k in np.flatnonzero(sizes > 100):
        pk = np.sort(ps[rs[k]:rs[k + 1]])
        out.append((sp.csr_matrix(Ae[pk, :][:, pk]), int((pk < pd["n"]).sum())))
    return out


HINT_SEQUENCE = ["tree4096", "tree1024", "hub1024", "tree1024x1025", "comp2048*", "tree2048", "bern1024"]


@gpu
@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_setup_with_hints_from_other_systems(ipd, order):
    from codes_of_ipd_ssn_amg_method_amd import _lib
    seq = HINT_SEQUENCE if order == "forward" else HINT_SEQUENCE[::-1]
    builds = []
    for name in seq:
        if name.endswith("*"):
            comps = component_systems(name[:-1])
            assert len(comps) >= 3
            builds += [("%s[%d]" % (name[:-1], i), A, fn) for i, (A, fn) in enumerate(comps)]
        else:
            Ae, fnode, _ = system(name)
            builds.append((name, Ae, fnode))
    ctx = _lib.Context(0)
    try:
        for tag, Ae, fnode in builds:
            o = setup_options(fnode, 1)
            ho = O.amg_setup(Ae, o, O.matlab_rng()) if "[" in tag else oracle_hierarchy(ipd, tag, 1)
            rng = ipd.MatlabRand()
            h = ipd.AMGHierarchy(Ae, o, rng, ctx=ctx)
            try:
                assert_same_hierarchy(h, ho, rng, (order, tag))
            finally:
                h.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# (c) ASAt, Aty bit for bit and Ax to an entrywise forward-error bar at full size
# ---------------------------------------------------------------------------------------------------------------
KKT_SHAPES = [(1024, 1024), (1024, 1025), (2047, 2049), (2048, 2048), (4096, 4096)]
MASKS = {"tree": lambda m, n: PR.mask_tree(m, n, seed=6), "hub": lambda m, n: PR.mask_hub(m, n, seed=6),
         "bern": lambda m, n: PR.mask_bernoulli(m, n, 0.04, seed=6)}


def pq_of(m, n, random):
    if not random:
        return np.ones(m), np.ones(n)
    rs = np.random.RandomState(m + 7 * n)
    return 0.5 + rs.random_sample(m), 0.5 + rs.random_sample(n)


@gpu
@pytest.mark.parametrize("pq_random", [False, True], ids=["pq1", "pqrand"])
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("m,n", KKT_SHAPES, ids=["%dx%d" % s for s in KKT_SHAPES])
def test_asat_bit_exact_at_scale(ipd, m, n, mask, pq_random):
    s = MASKS[mask](m, n)
    p, q = pq_of(m, n, pq_random)
    assert csc_equal(ipd.ASAt(s, p, q), O.ASAt(s, p, q))


def ax_reference(x, p, q):
    """y = [X'p; Xq] in extended precision (numpy longdouble, pairwise sums along contiguous rows), and the
    entrywise magnitudes [|X|'|p|; |X||q|] that bound any order's rounding error."""
    m, n = len(p), len(q)
    Xc = x.reshape(n, m)                       # row j = column j of X (x is column-major)
    pl, ql = p.astype(np.longdouble), q.astype(np.longdouble)
    y1 = np.empty(n, np.longdouble)
    y2 = np.zeros(m, np.longdouble)
    step = 256
    for j0 in range(0, n, step):
        blk = Xc[j0:j0 + step].astype(np.longdouble)
        y1[j0:j0 + step] = (blk * pl).sum(axis=1)
        y2 += (np.ascontiguousarray(blk.T) * ql[j0:j0 + step]).sum(axis=1)
    mag = np.concatenate([np.abs(Xc) @ np.abs(p), np.abs(Xc).T @ np.abs(q)])
    return np.concatenate([y1, y2]), mag


AX_C = 4   # forward-error bar |y - y_ref| <= AX_C * eps * (|X|'|p|, |X||q|) entrywise


@gpu
@pytest.mark.parametrize("m,n", KKT_SHAPES, ids=["%dx%d" % s for s in KKT_SHAPES])
def test_ax_aty_at_scale(ipd, m, n):
    """Aty bit for bit (k_aty_v2 for even m, k_aty_v1 for odd m); Ax entrywise within AX_C ulps of the
    magnitude sums.  The worst case of the kernel's summation order is ~(16 + n/16) eps of them, but on Gaussian
    x even a plain left-to-right float64 sum of 4096 terms stays near 2; one lost or doubled term costs ~1/n of
    them (~10^12 eps)."""
    rs = np.random.RandomState(m * 7 + n)
    p, q = 0.5 + rs.random_sample(m), 0.5 + rs.random_sample(n)
    x = rs.randn(m * n)
    y = rs.randn(m + n)
    z = ipd.Aty(y, p, q)
    assert np.array_equal(z, O.Aty(y, p, q))
    got = ipd.Ax(x, p, q)
    ref, mag = ax_reference(x, p, q)
    err = np.abs(got.astype(np.longdouble) - ref).astype(float)
    bar = AX_C * np.finfo(float).eps * mag
    worst = int(np.argmax(err / bar))
    assert np.all(err <= bar), (worst, err[worst], bar[worst], float(np.max(err / bar * AX_C)))


# ---------------------------------------------------------------------------------------------------------------
# (d) setup pieces at their gates
# ---------------------------------------------------------------------------------------------------------------
def laplacian_with_nnz(N, nnz, seed=1, eps=1e-3):
    """eps*I + weighted Laplacian of a connected random graph with EXACTLY nnz stored entries (a path, then
    random extra edges, each adding two entries)."""
    k = (nnz - N) // 2
    assert N + 2 * k == nnz and k >= N - 1
    rs = np.random.RandomState(seed)
    edges = {(i, i + 1) for i in range(N - 1)}
    while len(edges) < k:
        a, b = rs.randint(0, N, 2)
        if a != b:
            edges.add((min(a, b), max(a, b)))
    e = np.array(sorted(edges))
    w = 0.5 + rs.random_sample(len(e))
    W = sp.csr_matrix((np.concatenate([w, w]), (np.concatenate([e[:, 0], e[:, 1]]),
                                                  np.concatenate([e[:, 1], e[:, 0]]))), shape=(N, N))
    Lp = sp.csr_matrix(sp.diags(np.asarray(W.sum(axis=1)).ravel()) - W + eps * sp.identity(N))
    assert Lp.nnz == nnz
    return Lp


MIS_CASES = [(1024, 40000), (1024, 40002), (1025, 39999), (1025, 40001)]


@gpu
@pytest.mark.parametrize("isnsp", [0, 1])
@pytest.mark.parametrize("N,nnz", MIS_CASES, ids=["N%d-nnz%d" % c for c in MIS_CASES])
def test_mis_set_and_transfer_at_the_small_gate(ipd, N, nnz, isnsp):
    """mis_set against the oracle (C, F, As, random numbers consumed), and a non-bigraph transfer, which takes
    the one-launch mis_set_small exactly when N <= MIS_SMALL_ROWS and nnz <= MIS_SMALL_NNZ
    (plan_mis_small, csrc/ipd_setup_plan.h): one case inside, three just outside."""
    A = laplacian_with_nnz(N, nnz)
    assert (N > MIS_SMALL_ROWS or nnz > MIS_SMALL_NNZ) == ((N, nnz) != (1024, 40000))
    assert SP.transfer(2, N, nnz, N // 2)["mis_small"] == ((N, nnz) == (1024, 40000))
    refC, refF, refAs, info = O.mis_set(A, 0.25, O.matlab_rng())
    rng = ipd.MatlabRand()
    gotC, gotF, gotAs = ipd.mis_set(A, 0.25, rng)
    assert np.array_equal(gotC, refC) and np.array_equal(gotF, refF)
    assert csc_equal(gotAs, refAs)
    assert rng.consumed == len(info["rand"])
    o = O.amg_options_class1("v"); o.update(bigph=0, isnsp=isnsp)
    Ac, Pro, tinfo = O.transfer(A, o, 2, O.matlab_rng())
    rng = ipd.MatlabRand()
    gAc, gPro, gC = ipd.transfer(A, o, 2, rng)
    assert csc_equal(gAc, Ac) and csc_equal(gPro, Pro) and np.array_equal(gC, tinfo["isC"])
    assert rng.consumed == len(tinfo["mis"]["rand"])


@gpu
@pytest.mark.parametrize("which", [1, 2])
def test_strength_and_cf_split_at_8192(ipd, which):
    A = PR.random_sym_graph_laplacian(8192, deg=4, seed=21)
    assert csc_equal(ipd.strength(A, which), O.strength(A, which))
    As = O.strength_mask(A, 0.25)
    S = sp.csr_matrix(((As + As.T) > 0).astype(float))
    refC, refF = O.cf_split(S)
    gotC, gotF = ipd.cf_split(S)
    assert np.array_equal(gotC, refC) and np.array_equal(gotF, refF)


@gpu
def test_components_at_8192(ipd):
    N = 8192
    rs = np.random.RandomState(22)
    G = sp.random(N, N, 0.6 / N, random_state=rs, format="csr")
    G = sp.csr_matrix(G + G.T + sp.identity(N))
    blocks, sizes, p, r = ipd.components(G)
    ob, osz, op, orr = O.components(G)
    assert len(osz) > 1000          # many components, many of one node and a few large ones
    assert np.array_equal(blocks, ob) and np.array_equal(sizes, osz)
    assert np.array_equal(p, op) and np.array_equal(r, orr)


# ---------------------------------------------------------------------------------------------------------------
# (e) Hybrid_AMG at the driver sizes against the oracle, with the bars of test_gpu_hybrid.py::test_hybrid_amg,
#     and every traced component's hierarchy bit for bit
# ---------------------------------------------------------------------------------------------------------------
HYBRID_CASES = [("tree1024", "w"), ("hub1024", "w"), ("bern1024", "v"), ("tree2048", "v"), ("comp2048", "w"),
                ("tree4096", "v")]


@gpu
@pytest.mark.parametrize("name,cycle", HYBRID_CASES, ids=["%s-%s" % c for c in HYBRID_CASES])
def test_hybrid_amg_at_driver_sizes(ipd, name, cycle):
    pd = problem(name)
    opts = O.amg_options_class1(cycle)
    tr = []
    zo, ito, reso, infoo = O.Hybrid_AMG(pd, opts, O.matlab_rng(), trace=tr)
    rng = ipd.MatlabRand()
    z, it, res, info = ipd.Hybrid_AMG(pd, opts, rng)
    assert np.array_equal(info, infoo)
    noise_floor = res <= 1e-10 and reso <= 1e-10
    assert abs(it - ito) <= 1 or (noise_floor and abs(it - ito) <= 3), (it, ito, res, reso)
    M = pd["m"] + pd["n"]
    He = pd["bk1"] * sp.identity(M) + (pd["T"] + pd["H0"]) / pd["tk"]
    nz = np.linalg.norm(pd["z"])
    assert np.linalg.norm(He @ z - pd["z"]) <= max(1e-9, 20 * np.linalg.norm(He @ zo - pd["z"]) / nz) * nz
    assert np.linalg.norm(z - zo) <= 1e-5 * max(1.0, np.linalg.norm(zo))
    used = sum(len(t_["guess"]) + rand_used(t_["h"]) for t_ in tr)
    assert rng.consumed == used
    # each traced component's hierarchy, from the random numbers the oracle's setup drew for it
    Ae = O.build_Ae(pd["H0"], pd["T"], pd["p"], pd["q"], pd["bk1"], pd["tk"])[0]
    assert len(tr) >= (3 if name == "comp2048" else 1)
    for i, t in enumerate(tr):
        Aek = sp.csr_matrix(Ae[t["pk"], :][:, t["pk"]])
        o = dict(opts, isnsp=t["isnsp"], fnode=t["fnode"])
        vals = np.concatenate([np.asarray(inf["mis"]["rand"], float) for inf in t["h"].info[2:]
                               if inf and inf.get("mis")] or [np.zeros(0)])
        krng = ipd.MatlabRand(replay=vals)
        h = ipd.AMGHierarchy(Aek, o, krng)
        try:
            assert_same_hierarchy(h, t["h"], krng, (name, "component", i))
        finally:
            h.close()
