"""The Newton systems the Class 1 device driver meets at m = n = N, shared by the GPU tests that need realistic
hierarchies (tests/test_gpu_resident_deep.py, tests/test_gpu_setup_at_scale.py).  Needs a GPU: the driver runs
on the device up to the captured iteration."""
import numpy as np
import scipy.sparse as sp


def capture(ipd, N, kcap):
    """Ae, f, tk of the first Newton system of APD iteration kcap + 1 of the Class 1 device driver on the
    synthetic m = n = N problem of SURVEY 8d (Hybrid_AMG.m:17-24 with p = q = 1, T = 0)."""
    rs = np.random.RandomState(1)
    c, r, l = rs.random_sample(N * N), rs.random_sample(N), rs.random_sample(N)
    l = l * r.sum() / l.sum()
    one = np.ones(N)
    ws = ipd.APDWorkspace(1, c, r, l, one, one, gama=np.inf)
    ws.warmup(0.0, 100)
    amg = dict(retol=1e-11, bigph=1, maxit=30, theta=1 / 4, smoth=5, cycle="w", isnsp=1, inter=1)
    ws.run(amg, ipd.MatlabRand(5489), iters=kcap)
    lam = ws.state()[2]
    sc = ws.begin(kcap + 1)
    ev = ws.eval(lam)
    ws.close()
    H0 = ipd.ASAt(ev["s"], one, one)
    Q0 = sp.diags(np.concatenate([one, -one]))
    Ae = sp.csr_matrix(sc["bk1"] * (Q0 @ Q0) + (1.0 / sc["tk"]) * ((Q0 @ H0) @ Q0))
    f = Q0 @ np.random.RandomState(3).standard_normal(2 * N)
    return Ae, f, sc["tk"]
