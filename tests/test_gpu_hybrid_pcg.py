"""Hybrid_AMG_PCG / AMG4POT(..., 'amg_pcg'): Hybrid_AMG.m's routing with AMG-preconditioned CG as the
inner solver, against tests/hybrid_pcg_ref.py (the oracle's Hybrid_AMG with the numpy AMG-PCG on the
oracle hierarchy behind its solver hook).

7. the seven cases of tests/test_gpu_hybrid.py x V / W x pq_random, with the drivers' smoothing and with
   one sweep: routing info, rand stream, iteration count +-1, the residual of the ORIGINAL system;
8. the golden Newton systems with V, one sweep, maxit 30: the stationary iteration runs into maxit,
   AMG-PCG converges, same routing and rand stream;
9. AMG4POT(..., 'amg_pcg') at test_gpu_hybrid.py::test_amg4pot's bar."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ipd_oracle as O
from tests import hybrid_pcg_ref as HR
from tests import problems as PR
from tests.test_golden_oracle import load, problem_from
from tests.test_gpu_hybrid import CASES, _he

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ipd():
    import codes_of_ipd_ssn_amg_method_amd as m
    return m


@pytest.mark.parametrize("name,m,n,mk,tfrac", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("cycle", ["v", "w"])
@pytest.mark.parametrize("pq_random", [False, True])
@pytest.mark.parametrize("smoth1", [False, True], ids=["smoth_driver", "smoth1"])
def test_hybrid_amg_pcg(ipd, name, m, n, mk, tfrac, cycle, pq_random, smoth1):
    s = mk()
    t = None
    if tfrac is not None:
        t = (np.random.RandomState(9).random_sample(m + n) < tfrac).astype(float)
    pd = PR.make_prob(m, n, s, t=t, pq_random=pq_random)
    pd["H0"] = O.ASAt(s, pd["p"], pd["q"])
    opts = O.amg_options_class1(cycle) if tfrac is None else O.amg_options_class2(cycle)
    if smoth1:
        opts["smoth"] = 1
    ref_rng = HR.CountingRng()
    log = []
    zo, ito, reso, infoo = HR.Hybrid_AMG_PCG(pd, opts, ref_rng, log)
    assert all(e["it"] < opts["maxit"] for e in log), log     # the reference converges on every case
    rng = ipd.MatlabRand()
    z, it, res, info = ipd.Hybrid_AMG_PCG(pd, opts, rng)
    He = _he(pd)
    nz = np.linalg.norm(pd["z"])
    own = np.linalg.norm(He @ z - pd["z"]) / nz
    ref = np.linalg.norm(He @ zo - pd["z"]) / nz
    print("%s %s pq_random=%d smoth=%d: it %d ref %d, res %.3e ref %.3e, |He z - z|/|z| %.3e ref %.3e"
          % (name, cycle, pq_random, opts["smoth"], it, ito, res, reso, own, ref))
    assert np.array_equal(info, infoo)
    assert rng.consumed == ref_rng.consumed
    assert abs(it - ito) <= 1, (it, ito, res, reso)
    assert own <= max(1e-9, 20 * ref)


@pytest.mark.parametrize("name", ["class1_500_k08.npz", "class1_500_k20.npz", "class1_500_k40.npz"])
def test_converges_where_hybrid_amg_hits_maxit(ipd, name):
    pd = problem_from(load(name))
    pd["H0"] = O.ASAt(pd["s"], pd["p"], pd["q"])
    opts = O.amg_options_class1("v")
    opts.update(smoth=1, maxit=30)
    r0 = ipd.MatlabRand()
    z0, it0, res0, info0 = ipd.Hybrid_AMG(pd, opts, r0)
    r1 = ipd.MatlabRand()
    z1, it1, res1, info1 = ipd.Hybrid_AMG_PCG(pd, opts, r1)
    ref_rng = HR.CountingRng()
    zo, ito, reso, infoo = HR.Hybrid_AMG_PCG(pd, opts, ref_rng)
    print("%s: Hybrid_AMG it %d res %.3e; Hybrid_AMG_PCG it %d res %.3e (reference it %d res %.3e)"
          % (name, it0, res0, it1, res1, ito, reso))
    assert it0 == 30 and res0 > 1e-10
    assert it1 < 30 and abs(it1 - ito) <= 1 and res1 <= 1e-11
    assert np.array_equal(info0, info1) and np.array_equal(info1, infoo)
    assert r0.consumed == r1.consumed == ref_rng.consumed
    assert r0.rand(1)[0] == r1.rand(1)[0]          # the next number drawn is the same


@pytest.mark.parametrize("m,n,rho", [(48, 48, 0.1), (120, 90, 0.02)])
def test_amg4pot_pcg(ipd, m, n, rho):
    rs = np.random.RandomState(13)
    s = PR.mask_bernoulli(m, n, rho, seed=14)
    t = (rs.random_sample(m + n) < 0.7).astype(float)
    pd = PR.make_prob(m, n, s, t=t)
    pd["z"] = rs.randn(m + n + 1)
    pd["phi"] = np.ones(m * n)
    pd["H0"] = O.ASAt(s, pd["p"], pd["q"])
    opts = O.amg_options_class2("w")
    ref_rng = HR.CountingRng()
    zo, ito, reso, infoo = HR.AMG4POT_PCG(pd, opts, ref_rng)
    rng = ipd.MatlabRand()
    z, it, res, info = ipd.AMG4POT(pd, opts, "amg_pcg", rng)
    print("AMG4POT amg_pcg %dx%d: it %d ref %d, |z - zo|/|zo| %.3e" % (m, n, it, ito, np.linalg.norm(z - zo) / np.linalg.norm(zo)))
    assert np.array_equal(info, infoo) and abs(it - ito) <= 1
    assert rng.consumed == ref_rng.consumed
    assert np.linalg.norm(z - zo) <= 1e-6 * np.linalg.norm(zo)
    with pytest.raises(ValueError):
        ipd.AMG4POT(pd, opts, "direct")
