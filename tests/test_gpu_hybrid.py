"""GPU parity of the problem-level solvers: components, Hybrid_AMG, AMG4POT.
Bar: component labels / routing info / iteration counts identical; zeta agrees with
the oracle through the residual of the ORIGINAL system He*zeta = z to 1e-9 (the
systems are nearly singular, so solution vectors are only compared loosely)."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ipd_oracle as O
from tests import problems as PR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ipd():
    import codes_of_ipd_ssn_amg_method_amd as m
    return m


@pytest.mark.parametrize("N,dens,seed", [(1, 0.0, 0), (60, 0.01, 1), (400, 0.002, 2), (2048, 0.0006, 3)])
def test_components(ipd, N, dens, seed):
    rs = np.random.RandomState(seed)
    G = sp.random(N, N, dens, random_state=rs, format="csr")
    G = sp.csr_matrix(G + G.T + sp.identity(N))
    blocks, sizes, p, r = ipd.components(G)
    ob, osz, op, orr = O.components(G)
    assert np.array_equal(blocks, ob) and np.array_equal(sizes, osz)
    assert np.array_equal(p, op) and np.array_equal(r, orr)


def test_components_path_graph(ipd):
    N = 3000   # worst case diameter
    G = sp.diags([np.ones(N - 1), np.ones(N), np.ones(N - 1)], [-1, 0, 1], format="csr")
    blocks, sizes, p, r = ipd.components(G)
    assert len(sizes) == 1 and sizes[0] == N and not blocks.any()


def _he(pd):
    M = pd["m"] + pd["n"]
    return pd["bk1"] * sp.identity(M) + (pd["T"] + pd["H0"]) / pd["tk"]


CASES = [
    ("tree_connected", 96, 96, lambda: PR.mask_tree(96, 96, seed=1), None),
    ("tree_multi", 200, 200, lambda: PR.mask_tree(200, 200, seed=2, connect=False), None),
    ("tree_rect_multi", 260, 150, lambda: PR.mask_tree(260, 150, extra=0.0, seed=3, connect=False), None),
    ("bern_sparse", 128, 128, lambda: PR.mask_bernoulli(128, 128, 0.006, seed=4), None),
    ("empty", 40, 40, lambda: np.zeros(1600, np.uint8), None),
    ("dense", 64, 64, lambda: PR.mask_bernoulli(64, 64, 1.0), None),
    ("class2_T", 150, 150, lambda: PR.mask_tree(150, 150, seed=5, connect=False), 0.7),
]


@pytest.mark.parametrize("name,m,n,mk,tfrac", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("cycle", ["v", "w"])
@pytest.mark.parametrize("pq_random", [False, True])
def test_hybrid_amg(ipd, name, m, n, mk, tfrac, cycle, pq_random):
    s = mk()
    t = None
    if tfrac is not None:
        t = (np.random.RandomState(9).random_sample(m + n) < tfrac).astype(float)
    pd = PR.make_prob(m, n, s, t=t, pq_random=pq_random)
    pd["H0"] = O.ASAt(s, pd["p"], pd["q"])
    opts = O.amg_options_class1(cycle) if tfrac is None else O.amg_options_class2(cycle)
    tr = []
    zo, ito, reso, infoo = O.Hybrid_AMG(pd, opts, O.matlab_rng(), trace=tr)
    rng = ipd.MatlabRand()
    z, it, res, info = ipd.Hybrid_AMG(pd, opts, rng)
    assert np.array_equal(info, infoo)
    # cycle counts agree unless the history stagnates at the rounding floor (rel_res within
    # the 1e-10 comparison bar of retol = 1e-11): there the count is decided by noise
    noise_floor = res <= 1e-10 and reso <= 1e-10
    assert abs(it - ito) <= 1 or (noise_floor and abs(it - ito) <= 3), (it, ito, res, reso)
    He = _he(pd)
    nz = np.linalg.norm(pd["z"])
    assert np.linalg.norm(He @ z - pd["z"]) <= max(1e-9, 20 * np.linalg.norm(He @ zo - pd["z"]) / nz) * nz
    assert np.linalg.norm(z - zo) <= 1e-5 * max(1.0, np.linalg.norm(zo))
    # the rand stream advanced exactly as in the oracle (guesses + mis_set tie-breaks)
    used = sum(len(t_["guess"]) + sum(len(i["mis"]["rand"]) for i in t_["h"].info[2:] if i and i.get("mis"))
               for t_ in tr)
    assert rng.consumed == used        # (the rand stream does not depend on the cycle count)


def test_hybrid_amg_at_the_n0_boundary(ipd):
    """The system of tests/test_hybrid_plan.py whose route is checked on the CPU: a component of exactly HYBRID_N0
    nodes (solved with the small blocks) next to one of HYBRID_N0 + 1 (its own AMG solve, T != 0: isnsp = 0),
    singletons, and a second large component with T = 0 behind them (Hybrid_AMG.m:53/85)."""
    from tests.test_hybrid_plan import limits, mixed_system
    N0 = limits()["HYBRID_N0"]
    pd = mixed_system()
    opts = O.amg_options_class2("v")
    tr = []
    zo, ito, reso, infoo = O.Hybrid_AMG(pd, opts, O.matlab_rng(), N0=N0, trace=tr)
    assert [len(t_["pk"]) for t_ in tr] == [N0 + 1, 130] and [t_["isnsp"] for t_ in tr] == [0, 1]
    rng = ipd.MatlabRand()
    z, it, res, info = ipd.Hybrid_AMG(pd, opts, rng)
    assert np.array_equal(info, infoo)
    noise_floor = res <= 1e-10 and reso <= 1e-10
    assert abs(it - ito) <= 1 or (noise_floor and abs(it - ito) <= 3), (it, ito, res, reso)
    He = _he(pd)
    nz = np.linalg.norm(pd["z"])
    assert np.linalg.norm(He @ z - pd["z"]) <= max(1e-9, 20 * np.linalg.norm(He @ zo - pd["z"]) / nz) * nz
    assert np.linalg.norm(z - zo) <= 1e-5 * max(1.0, np.linalg.norm(zo))
    used = sum(len(t_["guess"]) + sum(len(i["mis"]["rand"]) for i in t_["h"].info[2:] if i and i.get("mis"))
               for t_ in tr)
    assert rng.consumed == used


def test_hybrid_amg_zero_in_pq(ipd):
    m = n = 16
    s = PR.mask_tree(m, n, seed=1)
    pd = PR.make_prob(m, n, s)
    pd["H0"] = O.ASAt(s, pd["p"], pd["q"])
    pd["q"] = pd["q"].copy()
    pd["q"][3] = 0.0
    with pytest.raises(ipd.IpdError) as ei:
        ipd.Hybrid_AMG(pd, O.amg_options_class1("v"))
    assert "p or q contains 0" in str(ei.value)          # Hybrid_AMG.m:18-19


@pytest.mark.parametrize("m,n,rho", [(48, 48, 0.1), (120, 90, 0.02)])
def test_amg4pot(ipd, m, n, rho):
    rs = np.random.RandomState(13)
    s = PR.mask_bernoulli(m, n, rho, seed=14)
    t = (rs.random_sample(m + n) < 0.7).astype(float)
    pd = PR.make_prob(m, n, s, t=t)
    pd["z"] = rs.randn(m + n + 1)
    pd["phi"] = np.ones(m * n)
    pd["H0"] = O.ASAt(s, pd["p"], pd["q"])
    zo, ito, reso, infoo = O.AMG4POT(pd, O.amg_options_class2("w"), O.matlab_rng())
    z, it, res, info = ipd.AMG4POT(pd, O.amg_options_class2("w"), "amg", ipd.MatlabRand())
    assert np.array_equal(info, infoo) and abs(it - ito) <= 1
    assert np.linalg.norm(z - zo) <= 1e-6 * np.linalg.norm(zo)
    with pytest.raises(ValueError):
        ipd.AMG4POT(pd, O.amg_options_class2("w"), "direct")   # str is 'amg' or 'twogrid' (:44-51)


@pytest.mark.parametrize("connect", [True, False], ids=["connected", "as-drawn"])
def test_amg4pot_at_config3_size_against_the_oracle(ipd, connect):
    """BASELINE config 3's size (Class 2, m = n = 512) against the oracle DIRECTLY (VERDICT r3 #1;
    Class2/AMG4POT.m:31-55 with the driver's options, APD_SsN_Class2.m:80-81: W cycle, smoth 10,
    maxit 40): tree-like active set, t ~ Bernoulli(0.7), so T != 0 and the large component takes the
    isnsp = 0 branch (Hybrid_AMG.m:32-38)."""
    m = n = 512
    rs = np.random.RandomState(2)
    s = PR.mask_tree(m, n, seed=7, connect=connect)
    t = (rs.random_sample(m + n) < 0.7).astype(float)
    pd = PR.make_prob(m, n, s, t=t)
    pd["z"] = rs.randn(m + n + 1)
    pd["phi"] = np.ones(m * n)
    pd["H0"] = O.ASAt(s, pd["p"], pd["q"])
    opts = O.amg_options_class2("w")
    assert opts["smoth"] == 10 and opts["maxit"] == 40 and opts["cycle"] == "w"
    zo, ito, reso, infoo = O.AMG4POT(pd, opts, O.matlab_rng())
    rng = ipd.MatlabRand()
    z, it, res, info = ipd.AMG4POT(pd, opts, "amg", rng)
    assert np.array_equal(info, infoo), (info, infoo)
    assert abs(it - ito) <= 1, (it, ito)
    assert np.linalg.norm(z - zo) <= 1e-6 * np.linalg.norm(zo)
    assert res <= 1e-10 and reso <= 1e-10


def test_system_dump_roundtrip(ipd, monkeypatch, tmp_path):
    """IPD_DUMP_SYSTEM writes the rescaled Newton system a Hybrid_AMG call solves; the dump equals
    the oracle's Ae and f = Q0*z (Hybrid_AMG.m:17-24) bit for bit."""
    import glob
    from tests.read_system_dump import read
    m, n = 90, 70
    s = PR.mask_tree(m, n, seed=8, connect=False)
    pd = PR.make_prob(m, n, s, pq_random=True)
    pd["H0"] = O.ASAt(s, pd["p"], pd["q"])
    monkeypatch.setenv("IPD_DUMP_SYSTEM", str(tmp_path / "sys_"))
    monkeypatch.setenv("IPD_DUMP_CALLS", "0-100000000")
    ipd.Hybrid_AMG(pd, O.amg_options_class1("v"), ipd.MatlabRand())
    files = glob.glob(str(tmp_path / "sys_*.bin"))
    assert len(files) == 1
    Ae, f, nf = read(files[0])
    out = O.build_Ae(pd["H0"], pd["T"], pd["p"], pd["q"], pd["bk1"], pd["tk"])
    ref, qp = sp.csr_matrix(out[0]), out[5]
    ref.sort_indices()
    assert nf == n and Ae.shape == ref.shape
    assert np.array_equal(Ae.indptr, ref.indptr) and np.array_equal(Ae.indices, ref.indices)
    assert np.array_equal(Ae.data, ref.data)
    assert np.array_equal(f, qp * pd["z"])


def test_component_order_injection(ipd, monkeypatch):
    """SURVEY A-9: MATLAB's dmperm order of the components is undocumented; a recorded order can be
    replayed (ipd_ctx_set_component_order).  The order moves info(2) and the order in which the
    large components draw their random numbers -- checked against the oracle visiting the
    components in the same (here: reversed) order."""
    from ctypes import c_int64
    from codes_of_ipd_ssn_amg_method_amd import _lib
    m, n = 260, 250
    rs = np.random.RandomState(3)
    Y = np.zeros((m, n), np.uint8)     # two large components (>100 nodes) and a few small ones
    Y[:120, :110] = PR.mask_tree(120, 110, seed=1).reshape(120, 110, order="F")
    Y[120:250, 110:240] = PR.mask_tree(130, 130, seed=2).reshape(130, 130, order="F")
    Y[250:255, 240:245] = 1
    s = Y.reshape(-1, order="F").copy()
    pd = PR.make_prob(m, n, s, pq_random=True)
    pd["H0"] = O.ASAt(s, pd["p"], pd["q"])
    opts = O.amg_options_class1("v")
    blocks, sizes, ps, rs_ = O.components(pd["H0"])
    ncomp = len(sizes)
    assert (sizes > 100).sum() == 2
    order = np.arange(ncomp)[::-1]                       # visit in reverse
    smallest = np.array([ps[rs_[k]:rs_[k + 1]].min() for k in order], np.int64)

    def permuted(A):
        b, sz, p_, r_ = orig(A)
        newid = np.empty(ncomp, np.int64)
        newid[order] = np.arange(ncomp)
        b2 = newid[b]
        sz2 = sz[order]
        p2 = np.argsort(b2, kind="stable")
        return b2, sz2, p2, np.concatenate([[0], np.cumsum(sz2)])

    orig = O.components
    tr0, tr1 = [], []
    z0, it0, res0, info0 = O.Hybrid_AMG(pd, opts, O.matlab_rng(), trace=tr0)
    monkeypatch.setattr(O, "components", permuted)
    z1, it1, res1, info1 = O.Hybrid_AMG(pd, opts, O.matlab_rng(), trace=tr1)
    monkeypatch.setattr(O, "components", orig)
    assert info0[1] != info1[1]                          # the oracle itself sees the order
    ctx = _lib.get_ctx()
    _lib.check(_lib.lib.ipd_ctx_set_component_order(ctx.handle, smallest.ctypes.data_as(_lib.c_void_p),
                                                    c_int64(ncomp)))
    rng = ipd.MatlabRand()
    z, it, res, info = ipd.Hybrid_AMG(pd, opts, rng)
    assert np.array_equal(info, info1)
    assert np.linalg.norm(z - z1) <= 1e-6 * max(1.0, np.linalg.norm(z1))
    # one-shot: the next call is back to the default order
    z_, it_, res_, info_ = ipd.Hybrid_AMG(pd, opts, ipd.MatlabRand())
    assert np.array_equal(info_, info0)
    with pytest.raises(ipd.IpdError):
        _lib.check(_lib.lib.ipd_ctx_set_component_order(ctx.handle, smallest[:-1].ctypes.data_as(_lib.c_void_p),
                                                        c_int64(ncomp - 1)))
        ipd.Hybrid_AMG(pd, opts, ipd.MatlabRand())
