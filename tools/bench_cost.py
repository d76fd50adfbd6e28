#!/usr/bin/env python3
"""The cost matrix built on the device from point clouds (csrc/ipd_cost.hip) against the route it replaces: the
host builds c and the workspace uploads it.

  python tools/bench_cost.py [--sizes 1024,4096,8192] [--reps 2] [--out FILE]

d = 2, squared Euclidean, scale on and off, m = n.  Timed with a host clock around calls that end in a device
synchronise, the variants alternating `--reps` times.  Per size:
  (a) numpy_c        the host builds c with numpy (the reference of tests/test_gpu_cost.py)
      from_matrix    APDWorkspace(1, c, ...): 8*mn bytes cross to the device
  (b) from_points    APDWorkspace.from_points: (m+n)*d coordinates cross, c is made in HBM
  (c) the kernel alone: ipd_cost_points_dev into a preallocated device array, 20 calls after a warm-up, for the
      8-byte and the 16-byte store form (IPD_COST_STORE) and scale off and on, as bytes per second over the
      8*mn bytes written (with scale the entries are computed twice and written once; a call also uploads the
      coordinates, reduces the statistics and reads them back).  COPY_TBPS is the guide's measured rate of a
      float4 copy on MI355X -- a read plus a write, named here for orientation; it is not a write ceiling.
The condition of DESIGN.md section 4g: in every repetition (b) is faster than from_matrix alone.

  python tools/bench_cost.py --passes [--sizes ...] [--reps 2] [--out FILE]
DESIGN.md section 4i: a stored and a matrix-free workspace from the same points, in one process, the two forms
alternating `--reps` times after a warm-up of both.  Per form and repetition: the create, `begin`, `end(from_w=True)`
(200 calls each, the mean), one warm-start iteration (warmup(0, 105) minus warmup(0, 5), over 100) and
`plan(tol, stats=True)` of the iterate the warm start leaves (20 calls; that iterate is dense, so tol is its 99th
percentile of |x|: one entry in a hundred is kept and crosses to the host, in both forms alike).  Host clock around
calls that end in a device synchronise, so a call carries its launch and read-back overhead in both forms alike.
Per pass the line gives min(stored) / min(free) and the spread between the stored form's own repetitions, the
margin a difference has to clear.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import codes_of_ipd_ssn_amg_method_amd as ipd   # noqa: E402
from codes_of_ipd_ssn_amg_method_amd import _lib as L   # noqa: E402
from codes_of_ipd_ssn_amg_method_amd.api import _cost_spec   # noqa: E402

COPY_TBPS = 6.29


def numpy_cost(xs, ys, scale):
    acc = np.zeros((xs.shape[0], ys.shape[0]))
    for k in range(xs.shape[1]):
        t = xs[:, k][:, None] - ys[:, k][None, :]
        acc = acc + t * t
    return acc / acc.max() if scale else acc


def clock(fn, inner=1):
    ipd.get_ctx().sync()
    t0 = time.perf_counter()
    for _ in range(inner):
        out = fn()
    ipd.get_ctx().sync()
    return (time.perf_counter() - t0) / inner, out


def bench_size(N, reps, emit):
    rs = np.random.RandomState(1)
    xs, ys = rs.standard_normal((N, 2)), rs.standard_normal((N, 2))
    r, l = rs.random_sample(N), rs.random_sample(N)
    l = l * r.sum() / l.sum()
    one = np.ones(N)
    mn = N * N
    for scale in (False, True):
        t_np, c = clock(lambda: numpy_cost(xs, ys, scale))
        c = np.asfortranarray(c).reshape(-1, order="F")

        def from_matrix():
            ipd.APDWorkspace(1, c, r, l, one, one, gama=np.inf).close()

        def from_points():
            ipd.APDWorkspace.from_points(1, xs, ys, r, l, one, one, metric="sqeuclidean", scale=scale).close()

        variants = [("from_matrix", from_matrix), ("from_points", from_points)]
        for _, fn in variants:       # every variant once before the clock runs
            fn()
        times = {name: [] for name, _ in variants}
        for _ in range(reps):
            for name, fn in variants:
                times[name].append(clock(fn)[0])
        # the results agree bit for bit
        ws = ipd.APDWorkspace.from_points(1, xs, ys, r, l, one, one, metric="sqeuclidean", scale=scale)
        same = bool(np.array_equal(ws.cost().reshape(-1, order="F").view(np.int64), c.view(np.int64)))
        ws.close()
        emit(dict(bench="cost_workspace", N=N, d=2, metric="sqeuclidean", scale=scale, numpy_c_seconds=round(t_np, 6),
                  seconds={k: [round(t, 6) for t in v] for k, v in times.items()}, bit_equal_to_numpy=same,
                  matrix_over_points=min(times["from_matrix"]) / min(times["from_points"]),
                  points_faster_in_every_rep=bool(all(p < m for p, m in zip(times["from_points"], times["from_matrix"])))))
        del c

    # (c) the kernel alone
    buf = L.DeviceBuffer(8 * mn)
    ctx = ipd.get_ctx().handle
    for scale in (False, True):
        spec, keep = _cost_spec(xs, ys, "sqeuclidean", scale)
        st = L.ipd_cost_stats()

        def call():
            L.check(L.lib.ipd_cost_points_dev(ctx, ctypes.byref(spec), buf.ptr, ctypes.byref(st)))

        times = {"8": [], "16": []}
        for form in times:           # warm-up of both forms
            os.environ["IPD_COST_STORE"] = form
            call()
        for _ in range(reps):
            for form in times:
                os.environ["IPD_COST_STORE"] = form
                times[form].append(clock(call, 20)[0])
        os.environ.pop("IPD_COST_STORE", None)
        emit(dict(bench="cost_kernel", N=N, d=2, metric="sqeuclidean", scale=scale, calls=20,
                  seconds_per_call={k: [round(t, 8) for t in v] for k, v in times.items()},
                  store8_TBps=8.0 * mn / min(times["8"]) / 1e12, store16_TBps=8.0 * mn / min(times["16"]) / 1e12,
                  copy_read_plus_write_TBps=COPY_TBPS))
    buf.free()


def bench_passes(N, reps, emit):
    rs = np.random.RandomState(1)
    xs, ys = rs.standard_normal((N, 2)), rs.standard_normal((N, 2))
    r, l = rs.random_sample(N), rs.random_sample(N)
    l = l * r.sum() / l.sum()
    one = np.ones(N)
    K0, K1, CALLS, PLAN_CALLS = 5, 105, 200, 20
    for scale in (False, True):
        def one_form(free):
            t = {}
            t["create"], ws = clock(lambda: ipd.APDWorkspace.from_points(1, xs, ys, r, l, one, one, metric="sqeuclidean",
                                                                         scale=scale, matrix_free=free))
            t_k0 = clock(lambda: ws.warmup(0.0, K0))[0]
            t_k1 = clock(lambda: ws.warmup(0.0, K1))[0]
            t["warm_iteration"] = (t_k1 - t_k0) / (K1 - K0)
            u, _, lam, _ = ws.state()
            tol = float(np.partition(np.abs(u), int(0.99 * u.size))[int(0.99 * u.size)])
            del u
            t["plan"], (X, st, ax) = clock(lambda: ws.plan(tol, stats=True), PLAN_CALLS)
            t["begin"] = clock(lambda: ws.begin(1), CALLS)[0]
            t["end_from_w"] = clock(lambda: ws.end(lam, from_w=True), CALLS)[0]
            info = ws.cost_info()
            ws.close()
            return t, info, (int(st["nnz"]), st["fval_kept"])
        forms = [("stored", False), ("free", True)]
        for _, free in forms:                # both forms once before the clock counts
            one_form(free)
        times = {name: [] for name, _ in forms}
        infos, plans = {}, {}
        for _ in range(reps):
            for name, free in forms:
                t, infos[name], plans[name] = one_form(free)
                times[name].append(t)
        passes = {}
        for key in ("create", "begin", "end_from_w", "warm_iteration", "plan"):
            st_, fr_ = [t[key] for t in times["stored"]], [t[key] for t in times["free"]]
            passes[key] = dict(stored=[round(v, 7) for v in st_], free=[round(v, 7) for v in fr_],
                               stored_over_free=min(st_) / min(fr_),
                               stored_spread=(max(st_) - min(st_)) / min(st_))
        emit(dict(bench="cost_free_passes", N=N, d=2, metric="sqeuclidean", scale=scale, reps=reps,
                  calls=dict(begin=CALLS, end_from_w=CALLS, plan=PLAN_CALLS, warm_iterations=K1 - K0),
                  seconds=passes, device_bytes={k: v["device_bytes"] for k, v in infos.items()},
                  plan_nnz=plans["stored"][0], same_plan_statistics=bool(plans["stored"] == plans["free"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--reps", type=int, default=2, help="alternating repetitions of the variants")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--passes", action="store_true", help="stored against matrix-free workspaces, pass by pass")
    a = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for N in [int(s) for s in a.sizes.split(",") if s]:
        (bench_passes if a.passes else bench_size)(N, a.reps, emit)


if __name__ == "__main__":
    main()
