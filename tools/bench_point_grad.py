#!/usr/bin/env python3
"""The gradient of the transport cost in the point positions (csrc/ipd_point_grad.hip) against the routes it replaces.

  python tools/bench_point_grad.py [--sizes 1024,4096] [--reps 3] [--out FILE]

Per size, in one process, on the dense iterate after warmup(0, 100) (every entry kept), d = 3, tol = 0, both sides,
timed with a host clock around calls that end in a device synchronise, every variant warmed, the variants alternating
`--reps` times (every repetition is in the row; the row gives medians and the spread max - min):
  metric 1   (a) grad_dev    ipd_apd_point_grad_dev on device arrays, with the mass
             (b) apply_dev   yardstick 1, the parent's route: ipd_apd_plan_apply_dev(ys, mass) on the same state, from
                             which 2 (w o xs - X ys) follows; it reads x as often
             "no_slower" says whether median(a) <= median(b) + spread(b)
  metric 2,4 (a) grad_dev and (c) state_numpy, yardstick 2: state() and numpy over the mn entries
Also d = 16, metric 2 (four passes over x, the row coordinates in LDS), device entry only.  (a) is given as bytes per
second over 8*mn*ceil(d/4) bytes (x once per pass), beside the rate of the drivers' evaluation pass
(ipd_apd_bench_eval) on the same workspace and apply_dev's rate.  A measurement path that finds no GPU fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import codes_of_ipd_ssn_amg_method_amd as ipd   # noqa: E402
from codes_of_ipd_ssn_amg_method_amd import _lib as L   # noqa: E402

NAMES = {1: "sqeuclidean", 2: "euclidean", 3: "cityblock", 4: "chebyshev"}


def timed(fn, inner):
    fn()
    ipd.get_ctx().sync()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    ipd.get_ctx().sync()
    return (time.perf_counter() - t0) / inner


def host_route(ws, xs, ys, metric, side):
    """state() and numpy over the mn entries: the only route for a pair-dependent weight before"""
    N = ws.m
    X = ws.state()[0][:N * N].reshape((N, N), order="F")
    T = xs[:, None, :] - ys[None, :, :]
    if metric == 2:
        a = np.sqrt((T * T).sum(axis=2))
        H = T / np.where(a > 0, a, 1.0)[:, :, None]
    else:
        A = np.abs(T)
        H = np.where(A == A.max(axis=2, keepdims=True), np.sign(T), 0.0)
    P = X[:, :, None] * H
    return -P.sum(axis=0) if side else P.sum(axis=1)


def alternate(variants, reps):
    for _, fn, _ in variants:     # every variant once before the clock runs
        fn()
    times = {name: [] for name, _, _ in variants}
    for _ in range(reps):
        for name, fn, inner in variants:
            times[name].append(timed(fn, inner))
    return times


def med(v):
    return statistics.median(v)


def bench_size(N, reps, emit):
    rs = np.random.RandomState(1)
    r, l = rs.random_sample(N), rs.random_sample(N)
    l *= r.sum() / l.sum()
    one = np.ones(N)
    mn = N * N
    for d, metrics in ((3, (1, 2, 4)), (16, (2,))):
        xs, ys = rs.random_sample((N, d)), rs.random_sample((N, d))
        ws = ipd.APDWorkspace(1, rs.random_sample(mn), r, l, one, one, gama=np.inf)
        ws.warmup(0.0, 100)
        ws.begin(8)
        ws.bench_eval(20)
        ms, by = ws.bench_eval(200)
        eval_GBps = by * 200 / (ms * 1e-3) / 1e9
        xd = L.DeviceBuffer.from_array(np.ascontiguousarray(xs.T).reshape(-1))
        yd = L.DeviceBuffer.from_array(np.ascontiguousarray(ys.T).reshape(-1))
        Gd, Yd, wd = L.DeviceBuffer(8 * N * d), L.DeviceBuffer(8 * N * d), L.DeviceBuffer(8 * N)
        passes = -(-d // 4)
        for metric in metrics:
            for side in (0, 1):
                def grad_dev():
                    ws.point_gradient_dev(Gd, wd, side=side, xs=xd, ys=yd, metric=NAMES[metric])

                def apply_dev():
                    ws.apply_plan_dev(xd if side else yd, Yd, wd, side=side)

                variants = [("grad_dev", grad_dev, 50)]
                if metric == 1:
                    variants.append(("apply_dev", apply_dev, 50))
                elif d == 3:
                    G = ws.point_gradient(side, points=(xs, ys), metric=NAMES[metric])
                    want = host_route(ws, xs, ys, metric, side)
                    assert np.abs(G - want).max() <= 1e-10 * max(np.abs(want).max(), 1.0)
                    variants.append(("state_numpy", lambda: host_route(ws, xs, ys, metric, side), 1))
                times = alternate(variants, reps)
                rec = dict(bench="point_grad", N=N, d=d, metric=metric, side=side, passes=passes,
                           seconds={key: [round(t, 7) for t in v] for key, v in times.items()},
                           median={key: med(v) for key, v in times.items()},
                           spread={key: max(v) - min(v) for key, v in times.items()},
                           grad_dev_GBps=8.0 * mn * passes / med(times["grad_dev"]) / 1e9, eval_GBps=eval_GBps)
                if metric == 1:
                    rec["apply_dev_GBps"] = 8.0 * mn * passes / med(times["apply_dev"]) / 1e9
                    rec["no_slower"] = bool(med(times["grad_dev"]) <= med(times["apply_dev"])
                                            + (max(times["apply_dev"]) - min(times["apply_dev"])))
                elif d == 3:
                    rec["state_numpy_over_grad_dev"] = med(times["state_numpy"]) / med(times["grad_dev"])
                emit(rec)
        for b in (xd, yd, Gd, Yd, wd):
            b.free()
        ws.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--reps", type=int, default=3, help="alternating repetitions of the variants")
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
