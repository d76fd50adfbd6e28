#!/usr/bin/env python3
"""The plan applied on the device (csrc/ipd_plan_apply.hip) against the host route it replaces.

  python tools/bench_plan_apply.py [--sizes 1024,4096] [--reps 2] [--out FILE]

Per size, state, side in {0, 1} and k in {1, 3, 16}, timed with a host clock around calls that end in a device
synchronise, every variant warmed, the variants alternating `--reps` times (every repetition is in the row):
  (a) apply_dev   ipd_apd_plan_apply_dev on device arrays
  (b) apply       ipd_apd_plan_apply: B goes up, Y comes back
  (c) plan_matmul plan(tol) followed by X @ B (X.T @ B) with scipy: the only route before
States: "warmup", the dense iterate after warmup(0, 100) (every entry kept, so (c) moves 16*mn bytes to the host),
and "staircase", m+n-1 entries put in with set_plan -- what a converged plan looks like.  tol = 0.
The row says whether (a) and (b) beat (c), slowest repetition against fastest.  (a) is also given as bytes per
second over 8*mn*ceil(k/4) bytes (x once per pass of four columns), next to the rate of the drivers' evaluation
pass (ipd_apd_bench_eval) on the same workspace: half of it is the bar for m = n = 4096, k = 3.
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
    fn()     # warmed before every clocked block: the first device call after plan()'s large read-back takes milliseconds
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
    ws.warmup(0.0, 100)
    mn = N * N
    ws.begin(8)
    ws.bench_eval(20)
    ms, by = ws.bench_eval(200)
    eval_GBps = by * 200 / (ms * 1e-3) / 1e9
    rs = np.random.RandomState(3)
    for state in ("warmup", "staircase"):
        if state == "staircase":
            i = np.arange(N)
            rows, cols = np.concatenate([i, i[1:]]), np.concatenate([i, i[:-1]])
            ws.set_plan(sp.csc_matrix((0.5 + rs.random_sample(2 * N - 1), (rows, cols)), shape=(N, N)))
        nnz = ws.plan(0.0, stats=True)[1]["nnz"]
        for side in (0, 1):
            for k in (1, 3, 16):
                B = rs.standard_normal((N, k))
                Bd = L.DeviceBuffer.from_array(B.reshape(-1, order="F"))
                Yd = L.DeviceBuffer(8 * N * k)

                def a_dev():
                    ws.apply_plan_dev(Bd, Yd, None, side=side)

                def b_host():
                    return ws.apply_plan(B, side=side)

                def c_plan():
                    X = ws.plan(0.0)
                    return (X.T @ B) if side else (X @ B)

                scale = np.abs(c_plan()).max()
                assert np.abs(b_host() - c_plan()).max() <= 1e-12 * max(scale, 1.0)
                dense = state == "warmup"
                variants = [("apply_dev", a_dev, 50), ("apply", b_host, 20),
                            ("plan_matmul", c_plan, 1 if dense and N > 2048 else 3)]
                for _, fn, _ in variants:     # every variant once before the clock runs
                    fn()
                times = {name: [] for name, _, _ in variants}
                for _ in range(reps):
                    for name, fn, inner in variants:
                        times[name].append(timed(fn, inner))
                best = {key: min(v) for key, v in times.items()}
                passes = -(-k // 4)
                emit(dict(bench="plan_apply", N=N, state=state, side=side, k=k, nnz=nnz,
                          seconds={key: [round(t, 7) for t in v] for key, v in times.items()},
                          apply_dev_GBps=8.0 * mn * passes / best["apply_dev"] / 1e9, eval_GBps=eval_GBps,
                          eval_bytes=by, plan_matmul_over_apply_dev=best["plan_matmul"] / best["apply_dev"],
                          plan_matmul_over_apply=best["plan_matmul"] / best["apply"],
                          apply_dev_beats_plan_matmul=bool(max(times["apply_dev"]) < min(times["plan_matmul"])),
                          apply_beats_plan_matmul=bool(max(times["apply"]) < min(times["plan_matmul"]))))
                Bd.free()
                Yd.free()
    ws.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--reps", type=int, default=2, help="alternating repetitions of the variants")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for N in [int(s) for s in a.sizes.split(",") if s]:
        bench_size(N, a.reps, emit)


if __name__ == "__main__":
    main()
