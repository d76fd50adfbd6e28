#!/usr/bin/env python3
"""The dual certificate on the device (csrc/ipd_dual.hip) against the host route it replaces.

  python tools/bench_dual.py [--sizes 1024,4096] [--reps 2] [--out FILE]

Per size, class 1 (gama = inf), cost stored and matrix-free (both from the same d = 2 point clouds) and side in
{-1, 0, 1}, timed with a host clock around calls that end in a device synchronise, every clocked block preceded by an
unclocked call, the variants alternating `--reps` times (every repetition is in the row):
  (a) dual_dev   ipd_apd_dual_dev on device arrays
  (b) dual       ipd_apd_dual: lam_out and arg come back
  (c) host       cost() + state() and the numpy expressions of the header: the only route before
side = -1 runs with primal = 1 (the pass reads c and x: 16*mn bytes stored, 8*mn matrix-free), the transforms with
primal = 0 (the transform and the evaluation that follows read c once each: 8*mn bytes per pass, nothing mn-sized
matrix-free).  (a) is also given as bytes per second -- whole call, host clock: the launches of a call, the read-back
of the statistics and the synchronise are in it -- next to the rate of the drivers' evaluation pass
(ipd_apd_bench_eval, device events) on the same workspace in the same process; half of that is the bar for the
stored rows.  A transform call is two passes over c, so its rate counts 16*mn bytes.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import codes_of_ipd_ssn_amg_method_amd as ipd   # noqa: E402
from codes_of_ipd_ssn_amg_method_amd import _lib as L   # noqa: E402


def timed(fn, inner):
    fn()     # unclocked: the first device call after a large read-back takes milliseconds
    ipd.get_ctx().sync()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    ipd.get_ctx().sync()
    return (time.perf_counter() - t0) / inner


def host_route(ws, side, primal):
    """what a caller of the parent library does: c and the state to the host, then numpy"""
    m, n = ws.m, ws.n
    C = ws.cost()
    u, _, lam, _ = ws.state()
    alpha, beta = lam[:n], lam[n:]
    out = {}
    if side == 0:
        T = -C - alpha[None, :]            # p = q = 1
        beta = np.where(np.isnan(T), -np.inf, T).max(axis=1)
        out["arg"] = T.argmax(axis=1)
    elif side == 1:
        T = -C - beta[:, None]
        alpha = np.where(np.isnan(T), -np.inf, T).max(axis=0)
        out["arg"] = T.argmax(axis=0)
    D = C + alpha[None, :] + beta[:, None]
    out["dmin"] = D.min()
    out["nneg"] = int((D < 0).sum())
    out["dual"] = -(ws._keep[0] @ alpha + ws._keep[1] @ beta)
    if primal:
        out["fval"] = float(C.reshape(-1, order="F") @ u[:m * n])
    return out


def bench_size(N, reps, emit):
    rs = np.random.RandomState(1)
    xs, ys = rs.random_sample((N, 2)), rs.random_sample((N, 2))
    r, l = rs.random_sample(N), rs.random_sample(N)
    l = l * r.sum() / l.sum()
    one = np.ones(N)
    mn = N * N
    for cost in ("stored", "free"):
        ws = ipd.APDWorkspace.from_points(1, xs, ys, r, l, one, one, scale=True, matrix_free=cost == "free")
        ws.warmup(0.0, 100)
        ws.begin(8)
        ws.bench_eval(20)
        ms, by = ws.bench_eval(200)
        eval_GBps = by * 200 / (ms * 1e-3) / 1e9
        out_d, arg_d = L.DeviceBuffer(8 * ws.L), L.DeviceBuffer(4 * N)
        for side in (-1, 0, 1):
            primal = side < 0

            def a_dev():
                return ws.dual_dev(None, side=side, primal=primal, lam_out=out_d, arg=arg_d)

            def b_host():
                return ws.dual(None, side=side, primal=primal, arg=True)

            def c_numpy():
                return host_route(ws, side, primal)

            got, want = b_host(), c_numpy()
            assert abs(got["dual"] - want["dual"]) <= 1e-9 * max(1.0, abs(want["dual"])), (got["dual"], want["dual"])
            assert got["nneg"] == want["nneg"] or side < 0
            if side >= 0:
                assert np.array_equal(got["arg"], want["arg"])
            variants = [("dual_dev", a_dev, 50), ("dual", b_host, 20), ("host", c_numpy, 1 if N > 2048 else 3)]
            times = {name: [] for name, _, _ in variants}
            for _ in range(reps):
                for name, fn, inner in variants:
                    times[name].append(timed(fn, inner))
            best = {key: min(v) for key, v in times.items()}
            stored_bytes = 16.0 * mn if cost == "stored" else (8.0 * mn if primal else 0.0)
            emit(dict(bench="dual", N=N, cost=cost, side=side, primal=int(primal),
                      seconds={key: [round(t, 7) for t in v] for key, v in times.items()},
                      bytes=stored_bytes, dual_dev_GBps=stored_bytes / best["dual_dev"] / 1e9, eval_GBps=eval_GBps,
                      eval_bytes=by, meets_half_of_eval=bool(stored_bytes / best["dual_dev"] / 1e9 >= 0.5 * eval_GBps)
                      if cost == "stored" else None,
                      host_over_dual_dev=best["host"] / best["dual_dev"], host_over_dual=best["host"] / best["dual"],
                      dual_dev_beats_host=bool(max(times["dual_dev"]) < min(times["host"])),
                      dual_beats_host=bool(max(times["dual"]) < min(times["host"]))))
        out_d.free()
        arg_d.free()
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
