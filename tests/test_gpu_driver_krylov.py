"""The APD / semismooth-Newton drivers with AMG-preconditioned CG as the inner solver
(APDWorkspace.run(..., krylov=True), ipd_apd_set_krylov).

10. the drivers' options on Class 1 120x100 and Class 2 100x120 at test_gpu_altsolvers.py's bar for
    alternate inner solvers, against the direct-solve reference (oracle/drivers.py); krylov set and
    cleared again gives the default run bit for bit;
11. Class 1 120x100 with V, one sweep, maxit 30: the stationary inner solve fails (FailAMG > 0), AMG-PCG
    does not, both converge with the reference's k."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import drivers as D                      # noqa: E402
from tests.test_gpu_altsolvers import OPTS           # noqa: E402
from tests.test_gpu_driver import problem, ws_of     # noqa: E402


def ipd():
    import codes_of_ipd_ssn_amg_method_amd as pkg
    return pkg


def reference(cls, pr):
    if cls == 1:
        start = D.warmup_class1(pr["c"], pr["r"], pr["l"], pr["p"], pr["q"], np.inf, 100)
        ref = D.apd_ssn_class1(pr["c"], pr["r"], pr["l"], pr["p"], pr["q"], np.inf, inner="direct", start=start)
    else:
        start = D.warmup_class2(pr["c"], pr["r"], pr["l"], pr["p"], pr["q"], pr["mu"], pr["phi"], 100)
        ref = D.apd_ssn_class2(pr["c"], pr["r"], pr["l"], pr["p"], pr["q"], pr["mu"], pr["phi"],
                               inner="direct", start=start)
    return start, ref


def run(cls, pr, start, opts, krylov, toggle=False):
    ws = ws_of(cls, pr)
    ws.set_state(start[0], start[0], start[1], 1.0)
    rng = ipd().MatlabRand(5489)
    if toggle:      # set and cleared again before the run
        from codes_of_ipd_ssn_amg_method_amd import _lib as L
        L.check(L.lib.ipd_apd_set_krylov(ws.handle, 1))
        L.check(L.lib.ipd_apd_set_krylov(ws.handle, 0))
    out = ws.run(opts, rng, krylov=krylov)
    hist, recs = ws.history(), ws.records()
    ws.close()
    return out, hist, recs, rng.consumed


@pytest.mark.parametrize("cls,m,n,kref", [(1, 120, 100, 57), (2, 100, 120, 47)])
def test_driver_with_amg_pcg_inner_solver(cls, m, n, kref):
    pr = problem(cls, m, n, seed=1)
    start, ref = reference(cls, pr)
    assert ref["k"] == kref
    opts = OPTS if cls == 1 else dict(OPTS, smoth=10, maxit=40)
    out, hist, recs, used = run(cls, pr, start, opts, True)
    kx = np.asarray(ref["KKT_xk"])
    print("class %d: k %d ref %d, |fval - ref| %.3e, KKT_xk dev %.3e, SumAMG %d FailAMG %d"
          % (cls, out["k"], ref["k"], abs(out["fval"] - ref["fval"]),
             np.max(np.abs(hist["KKT_xk"][:len(kx)] - kx[:len(hist["KKT_xk"])]) / (1 + kx[:len(hist["KKT_xk"])])),
             out["SumAMG"], out["FailAMG"]))
    assert out["converged"] and out["k"] == ref["k"]
    assert abs(out["fval"] - ref["fval"]) <= 1e-7
    assert np.all(np.abs(hist["KKT_xk"] - kx) <= 1e-6 * (1 + kx))
    # krylov set and cleared again: the default run bit for bit
    a = run(cls, pr, start, opts, False)
    b = run(cls, pr, start, opts, False, toggle=True)
    assert a[0] == b[0] and a[2] == b[2] and a[3] == b[3]
    assert all(np.array_equal(a[1][k], b[1][k]) for k in a[1])
    assert a[2] != recs or a[0]["SumAMG"] != out["SumAMG"]     # ... and krylov did change the inner solver


def test_class1_driver_where_the_stationary_inner_solve_fails():
    pr = problem(1, 120, 100, seed=1)
    start, ref = reference(1, pr)
    opts = dict(OPTS, cycle="v", smoth=1, maxit=30)
    off = run(1, pr, start, opts, False)[0]
    on = run(1, pr, start, opts, True)[0]
    print("krylov off: k %d FailAMG %d SumAMG %d; on: k %d FailAMG %d SumAMG %d"
          % (off["k"], off["FailAMG"], off["SumAMG"], on["k"], on["FailAMG"], on["SumAMG"]))
    assert off["FailAMG"] > 0 and on["FailAMG"] == 0
    assert off["converged"] and on["converged"]
    assert off["k"] == ref["k"] and on["k"] == ref["k"]
