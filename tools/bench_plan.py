#!/usr/bin/env python3
"""The sparse transport plan out of the device workspace (csrc/ipd_plan.hip) against the dense
route it replaces, on a workspace after `warmup`.

  python tools/bench_plan.py [--sizes 1024,4096] [--reps 2] [--out FILE] [--bundled]

Per size and tol in {0, 1e-9 * max x}, timed with a host clock around calls that end in a device
synchronise, the variants alternating `--reps` times:
  (a) plan_dev   ipd_apd_plan_dev into device arrays sized by a first cap = 0 query
  (b) plan       ipd_apd_plan: the kept entries and the column pointers cross to the host
  (c) dense      state() + scipy.sparse.csc_matrix: 16*mn bytes cross, the host compacts
(a) is also given as bytes per second over 24*mn bytes (x twice, c once), next to the rate of the
drivers' evaluation pass (ipd_apd_bench_eval) on the same workspace.  The iterate after `warmup`
is dense (every entry is kept, the fill pass writes 16 bytes per entry on top of the 24 counted);
a converged plan has about m+n entries, so the same is measured once more at tol = 0 on a
staircase plan of m+n-1 entries that set_plan puts into the workspace (state "staircase").
--bundled: for the record, nnz of the plan after the Class 1 run on the bundled 500 x 500 input at
tol in {0, 1e-12, 1e-9, 1e-6} * max x, next to m+n-1.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import codes_of_ipd_ssn_amg_method_amd as ipd   # noqa: E402
from codes_of_ipd_ssn_amg_method_amd import _lib as L   # noqa: E402


def problem(N, seed=1):
    rs = np.random.RandomState(seed)
    c, r, l = rs.random_sample(N * N), rs.random_sample(N), rs.random_sample(N)
    return dict(c=c, r=r, l=l * r.sum() / l.sum())


def timed(fn, inner):
    ipd.get_ctx().sync()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    ipd.get_ctx().sync()
    return (time.perf_counter() - t0) / inner


def bench_size(N, reps, emit):
    pr = problem(N)
    one = np.ones(N)
    ws = ipd.APDWorkspace(1, pr["c"], pr["r"], pr["l"], one, one, gama=np.inf)
    x, _ = ws.warmup(0.0, 100)
    mn = N * N
    xmax = float(np.abs(x[:mn]).max())
    ws.begin(8)
    ws.bench_eval(20)
    ms, by = ws.bench_eval(200)
    eval_GBps = by * 200 / (ms * 1e-3) / 1e9
    for state, tol in (("warmup", 0.0), ("warmup", 1e-9 * xmax), ("staircase", 0.0)):
        if state == "staircase":
            rs = np.random.RandomState(2)
            i = np.arange(N)
            rows, cols = np.concatenate([i, i[1:]]), np.concatenate([i, i[:-1]])
            ws.set_plan(sp.csc_matrix((0.5 + rs.random_sample(2 * N - 1), (rows, cols)), shape=(N, N)))
        nnz = ws.plan(tol, stats=True)[1]["nnz"]
        jc, ax = L.DeviceBuffer(8 * (N + 1)), L.DeviceBuffer(8 * 2 * N)
        ir, prb = L.DeviceBuffer(8 * max(nnz, 1)), L.DeviceBuffer(8 * max(nnz, 1))

        def a_dev():
            ws.plan_dev(tol, jc, (ir.ptr.value, nnz), (prb.ptr.value, nnz), None)

        def a_dev_ax():
            ws.plan_dev(tol, jc, (ir.ptr.value, nnz), (prb.ptr.value, nnz), ax)

        def b_host():
            ws.plan(tol)

        def c_dense():
            u = ws.state()[0]
            X = u[:mn].reshape((N, N), order="F")
            if tol > 0.0:
                X = np.where(np.abs(X) <= tol, 0.0, X)
            return sp.csc_matrix(X)

        variants = [("plan_dev", a_dev, 50), ("plan_dev_ax", a_dev_ax, 50), ("plan", b_host, 20),
                    ("dense", c_dense, 2)]
        assert c_dense().nnz == nnz
        for _, fn, _ in variants:     # every variant once before the clock runs
            fn()
        times = {name: [] for name, _, _ in variants}
        for _ in range(reps):
            for name, fn, inner in variants:
                times[name].append(timed(fn, inner))
        best = {k: min(v) for k, v in times.items()}
        emit(dict(bench="plan", N=N, state=state, tol=tol, xmax=xmax, nnz=nnz, m_plus_n_minus_1=2 * N - 1,
                  seconds={k: [round(t, 7) for t in v] for k, v in times.items()},
                  plan_dev_GBps=24.0 * mn / best["plan_dev"] / 1e9,
                  plan_dev_ax_GBps=24.0 * mn / best["plan_dev_ax"] / 1e9, eval_GBps=eval_GBps,
                  eval_bytes=by, dense_over_plan_dev=best["dense"] / best["plan_dev"],
                  dense_over_plan=best["dense"] / best["plan"],
                  faster_than_dense=bool(max(times["plan_dev"]) < min(times["dense"]) and
                                         max(times["plan"]) < min(times["dense"]))))
        for b in (jc, ax, ir, prb):
            b.free()
    ws.close()


def bundled(emit):
    d = np.load(os.path.join(ROOT, "tests", "golden", "data1_500.npz"))
    m, n = d["l"].size, d["r"].size
    ws = ipd.APDWorkspace(1, d["c"], d["r"], d["l"], np.ones(m), np.ones(n), gama=np.inf)
    ws.warmup(0.0, 100)
    amg = dict(retol=1e-11, bigph=1, maxit=30, theta=1 / 4, smoth=5, cycle="w", isnsp=1, inter=1)
    out = ws.run(amg, ipd.MatlabRand(5489))
    xmax = float(ws.plan(0.0).data.max())
    nnz = {}
    for f in (0.0, 1e-12, 1e-9, 1e-6):
        st = ws.plan(f * xmax, stats=True)[1]
        nnz["%g" % f] = dict(nnz=st["nnz"], sum_dropped=st["sum_dropped"], max_dropped=st["max_dropped"])
    emit(dict(bench="plan_nnz_bundled_500", converged=out["converged"], k=out["k"], xmax=xmax,
              m_plus_n_minus_1=m + n - 1, by_tol_over_xmax=nnz))
    ws.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--reps", type=int, default=2, help="alternating repetitions of the variants")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--bundled", action="store_true")
    a = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for N in [int(s) for s in a.sizes.split(",") if s]:
        bench_size(N, a.reps, emit)
    if a.bundled:
        bundled(emit)


if __name__ == "__main__":
    main()
