#!/usr/bin/env python3
"""The primal certificate on the device (csrc/ipd_round.hip) against the host route it replaces.

  python tools/bench_round.py [--sizes 1024,4096] [--reps 2] [--out FILE]
  python tools/bench_round.py --converged [--out FILE]
  python tools/bench_round.py --correction [--sizes 1024,4096] [--reps 3] [--out FILE]

Per size, class 1 (gama = inf, p = q = 1), cost stored and matrix-free (both from the same d = 2 point clouds), state
after warmup(0, 100), side in {0, 1}, timed with a host clock around calls that end in a device synchronise, every
clocked block preceded by an unclocked call, the variants alternating `--reps` times (every repetition is in the row):
  (a)  round_dev        ipd_apd_round_dev on device arrays, the four factors out: passes A, B, C, D
  (a') round_dev_xout   the same with x_out: pass W as well
  (b)  round            ipd_apd_round: the four factors come back to the host
  (c)  host             state() + cost() and the numpy restatement of the header (tests/round_ref.py): the only route
                        before
Next to them the rate of the drivers' evaluation pass (ipd_apd_bench_eval, device events) on the same workspace in the
same process: half of that is the bar for each of the passes A, B, C, D and W, taken per kernel from a
`rocprofv3 --kernel-trace --stats` run of this benchmark (`--sizes 4096 --reps 1`).  Bytes per pass on a stored cost:
A, B and D 8*mn, C 16*mn, W 8*mn read and 8*mn written per destination.

--converged: the four cases of tests/test_gpu_dual.py::test_feasibility_and_weak_duality run to convergence with the
drivers' defaults and `bracket=True`; prints the certified bracket next to f* from HiGHS.

--correction: per size and cost source, ipd_apd_round_dev (the four factors out, no x_out) under
the rank-one term (mode 0: 8 launches), the north-west list (mode 1: 9 launches, none of them pass D) and the cheaper of
the two (mode 2: 10 launches), the modes alternating `--reps` times in one process with the protocol above; mode 0 is
the parent's path, the spread of its repetitions the bar for mode 1.  Next to the times the correction's cost t*cc of
the state after warmup(0, 100) under mode 0, mode 1 along the identity, mode 1 along projection_order, and mode 2.
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
from tests import round_ref as R   # noqa: E402


def timed(fn, inner):
    fn()     # unclocked: the first device call after a large read-back takes milliseconds
    ipd.get_ctx().sync()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    ipd.get_ctx().sync()
    return (time.perf_counter() - t0) / inner


def host_route(ws, pr, side):
    """what a caller of the parent library does: c and the state to the host, then numpy"""
    m, n = ws.m, ws.n
    pr = dict(pr, c=ws.cost().reshape(-1, order="F"))
    u = ws.state()[0]
    return R.round_ref(1, pr, m, n, u, 0.0, side)


def bench_size(N, reps, emit):
    rs = np.random.RandomState(1)
    xs, ys = rs.random_sample((N, 2)), rs.random_sample((N, 2))
    r, l = rs.random_sample(N), rs.random_sample(N)
    l = l * r.sum() / l.sum()
    one = np.ones(N)
    pr = dict(r=r, l=l, p=one, q=one)
    mn = N * N
    for cost in ("stored", "free"):
        ws = ipd.APDWorkspace.from_points(1, xs, ys, r, l, one, one, scale=True, matrix_free=cost == "free")
        ws.warmup(0.0, 100)
        ws.begin(8)
        ws.bench_eval(20)
        ms, by = ws.bench_eval(200)
        eval_GBps = by * 200 / (ms * 1e-3) / 1e9
        bufs = [L.DeviceBuffer(8 * N) for _ in range(4)]
        xo = L.DeviceBuffer(8 * mn)
        for side in (0, 1):
            def a_dev():
                return ws.round_plan_dev(0.0, side=side, rho=bufs[0], kappa=bufs[1], e=bufs[2], f=bufs[3])

            def a_xout():
                return ws.round_plan_dev(0.0, side=side, rho=bufs[0], kappa=bufs[1], e=bufs[2], f=bufs[3], x_out=xo)

            def b_host():
                return ws.round_plan(0.0, side=side)

            def c_numpy():
                return host_route(ws, pr, side)

            got, want = b_host(), c_numpy()
            assert got["ok"] == want["ok"] == 1
            assert abs(got["fval"] - want["fval"]) <= 1e-9 * max(1.0, abs(want["fval"])), (got["fval"], want["fval"])
            variants = [("round_dev", a_dev, 50), ("round_dev_xout", a_xout, 50), ("round", b_host, 20),
                        ("host", c_numpy, 1 if N > 2048 else 3)]
            times = {name: [] for name, _, _ in variants}
            for _ in range(reps):
                for name, fn, inner in variants:
                    times[name].append(timed(fn, inner))
            best = {key: min(v) for key, v in times.items()}
            emit(dict(bench="round", N=N, cost=cost, side=side,
                      seconds={key: [round(t, 7) for t in v] for key, v in times.items()},
                      fval=got["fval"], viol_in=got["viol_in"], t=got["t"], se=got["se"],
                      eval_GBps=eval_GBps, eval_bytes=by,
                      host_over_round_dev=best["host"] / best["round_dev"],
                      host_over_round=best["host"] / best["round"],
                      round_dev_beats_host=bool(max(times["round_dev"]) < min(times["host"])),
                      round_dev_xout_beats_host=bool(max(times["round_dev_xout"]) < min(times["host"])),
                      round_beats_host=bool(max(times["round"]) < min(times["host"]))))
        for b in bufs + [xo]:
            b.free()
        ws.close()


def bench_correction(N, reps, emit):
    rs = np.random.RandomState(1)
    xs, ys = rs.random_sample((N, 2)), rs.random_sample((N, 2))
    r, l = rs.random_sample(N), rs.random_sample(N)
    l = l * r.sum() / l.sum()
    one = np.ones(N)
    proj = ipd.projection_order(xs, ys)
    for cost in ("stored", "free"):
        ws = ipd.APDWorkspace.from_points(1, xs, ys, r, l, one, one, scale=True, matrix_free=cost == "free")
        ws.warmup(0.0, 100)
        bufs = [L.DeviceBuffer(8 * N) for _ in range(4)]
        for side in (0, 1):
            def call():
                return ws.round_plan_dev(0.0, side=side, rho=bufs[0], kappa=bufs[1], e=bufs[2], f=bufs[3])

            settings = [("rank_one", "rank_one", (None, None)), ("north_west_identity", "north_west", (None, None)),
                        ("north_west", "north_west", proj), ("cheaper", "cheaper", proj)]
            tcc, info = {}, {}
            for name, mode, order in settings:
                ws.set_correction(mode, *order)
                st = call()
                assert st["ok"] == 1
                tcc[name] = st["t"] * st["cc"]
                info[name] = ws.correction_info()
            times = {name: [] for name, _, _ in settings if name != "north_west_identity"}
            for _ in range(reps):
                for name, mode, order in settings:
                    if name in times:
                        ws.set_correction(mode, *order)
                        times[name].append(timed(call, 50))
            r1 = times["rank_one"]
            emit(dict(bench="round_correction", N=N, cost=cost, side=side,
                      seconds={key: [round(t, 7) for t in v] for key, v in times.items()},
                      launches=dict(rank_one=8, north_west=9, cheaper=10), t_cc=tcc,
                      count=info["north_west"]["count"], cheaper_form=info["cheaper"]["form"],
                      rank_one_spread=max(r1) - min(r1),
                      north_west_minus_rank_one=min(times["north_west"]) - min(r1),
                      north_west_within_spread=bool(min(times["north_west"]) <= max(r1))))
        ws.set_correction("rank_one")
        for b in bufs:
            b.free()
        ws.close()


def converged(emit):
    """tests/test_gpu_dual.py's four cases to convergence, with the bracket"""
    import scipy.sparse as sp
    from scipy.optimize import linprog
    for cls in (1, 2):
        for m, n in ((24, 24), (37, 29)):
            rs = np.random.RandomState(12)
            c, r, l = rs.random_sample(m * n), rs.random_sample(n), rs.random_sample(m)
            p, q = np.ones(m), np.ones(n)
            A = sp.vstack([sp.kron(sp.identity(n), p[None, :]), sp.kron(q[None, :], sp.identity(m))])
            if cls == 1:
                l = l * (r @ q) / (l @ p)
                out = ipd.APD_SsN_Class1(c, r, l, p, q, certificate=True, bracket=True)
                lp = linprog(c, A_eq=sp.csr_matrix(A), b_eq=np.concatenate([r, l]), bounds=(0, None), method="highs")
            else:
                phi, mu = np.ones(m * n), 0.65 * min(r.sum(), l.sum())
                out = ipd.APD_SsN_Class2(c, r, l, p, q, mu, phi, certificate=True, bracket=True)
                A = sp.vstack([sp.hstack([A, sp.identity(m + n)]),
                               sp.hstack([sp.csr_matrix(phi[None, :]), sp.csr_matrix((1, m + n))])])
                lp = linprog(np.concatenate([c, np.zeros(m + n)]), A_eq=sp.csr_matrix(A),
                             b_eq=np.concatenate([r, l, [mu]]), bounds=(0, None), method="highs")
            assert lp.status == 0, lp.message
            fstar = float(lp.fun)
            br, up = out["bracket"], out["bracket"]["upper"]
            emit(dict(bench="round_converged", cls=cls, m=m, n=n, k=int(out["k"]), kkt_lk=float(out["kkt"][1]),
                      fstar=fstar, fval_xk_minus_fstar=out["certificate"]["fval"] - fstar,
                      upper_minus_fstar=up["fval"] - fstar, fstar_minus_lower=fstar - br["lower"]["dual"],
                      gap=br["gap"], dual_gap=out["certificate"]["gap"], side=up["side"], ok=up["ok"],
                      viol_in=up["viol_in"], theta=up["theta"], t=up["t"], se=up["se"], sf=up["sf"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--reps", type=int, default=2, help="alternating repetitions of the variants")
    ap.add_argument("--converged", action="store_true", help="the bracket of four converged runs instead")
    ap.add_argument("--correction", action="store_true", help="the three correction modes of section 4n instead")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.converged:
        converged(emit)
        return
    for N in [int(s) for s in a.sizes.split(",") if s]:
        (bench_correction if a.correction else bench_size)(N, a.reps, emit)


if __name__ == "__main__":
    main()
