#!/usr/bin/env python3
"""The bracket as one device call (csrc/ipd_bracket.hip) against the calls it replaces, and the drivers' stopping rule
on the certified gap.

  python tools/bench_gap.py [--sizes 1024,4096] [--reps 2] [--out FILE]      the probe
  python tools/bench_gap.py --run [--size 1024] [--reps 2] [--out FILE]      whole runs

The probe.  Per size, class 1 (gama = inf, p = q = 1), cost stored and matrix-free (both from the same d = 2 point
clouds), state after warmup(0, 100), timed with a host clock around calls that end in a device synchronise, every
clocked block preceded by an unclocked call, the variants alternating `--reps` times (every repetition is in the row):
  fused     ipd_apd_bracket_dev, every pointer NULL
  four      ipd_apd_dual_dev (side 0, side 1, primal = 1) and ipd_apd_round_dev (side 0, side 1, no vectors)
  python    APDWorkspace.bracket(): the same four through the host entries, with the arg map and the vectors
`fused_not_slower` is the condition of section 4m: the fused call's slower repetition against the four calls' faster
one.  Next to them the rate of the drivers' evaluation pass (ipd_apd_bench_eval, device events) on the same workspace in
the same process: half of that is the bar for k_du_both and k_du_eval2 on the bytes they move, taken per kernel from a
`rocprofv3 --kernel-trace --stats` run of this benchmark (`--sizes 4096 --reps 1`).  Bytes on a stored cost: k_du_both
8*mn (c), k_du_eval2 16*mn (c and x); matrix-free: 0 and 8*mn.

Whole runs (--run).  Class 1 from 2-D points at `--size`, the drivers' warm start and defaults: no rule against a
record-only rule (every = 1) in alternation, then gap_rel 1e-3 and 1e-4 against the KKT run: iterations and seconds.
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

AMG1 = dict(retol=1e-11, bigph=1, maxit=30, theta=1 / 4, smoth=5, cycle="w", isnsp=1, inter=1, guess=None)


def timed(fn, inner):
    fn()     # unclocked: the first device call after a large read-back takes milliseconds
    ipd.get_ctx().sync()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    ipd.get_ctx().sync()
    return (time.perf_counter() - t0) / inner


def points(N):
    rs = np.random.RandomState(1)
    xs, ys = rs.random_sample((N, 2)), rs.random_sample((N, 2))
    r, l = rs.random_sample(N), rs.random_sample(N)
    return xs, ys, r, l * r.sum() / l.sum(), np.ones(N)


def bench_probe(N, reps, emit):
    xs, ys, r, l, one = points(N)
    for cost in ("stored", "free"):
        ws = ipd.APDWorkspace.from_points(1, xs, ys, r, l, one, one, scale=True, matrix_free=cost == "free")
        ws.warmup(0.0, 100)
        ws.begin(8)
        ws.bench_eval(20)
        ms, by = ws.bench_eval(200)
        eval_GBps = by * 200 / (ms * 1e-3) / 1e9

        def fused():
            return ws.gap_probe_dev(0.0)

        def four():
            d = [ws.dual_dev(side=s, primal=True) for s in (0, 1)]
            u = [ws.round_plan_dev(0.0, side=s) for s in (0, 1)]
            return d, u

        def python():
            return ws.bracket()

        got, (d, u), br = fused(), four(), python()
        ls = 1 if d[1]["dual"] > d[0]["dual"] else 0
        us = min((0, 1), key=lambda s: (not u[s]["ok"], u[s]["fval"]))
        assert (got["lower"]["side"], got["upper"]["side"]) == (ls, us)
        assert got["lower"]["dual"] == d[ls]["dual"] and got["upper"]["fval"] == u[us]["fval"]
        assert got["gap"] == br["gap"]
        variants = [("fused", fused, 50), ("four", four, 50), ("python", python, 20)]
        times = {name: [] for name, _, _ in variants}
        for _ in range(reps):
            for name, fn, inner in variants:
                times[name].append(timed(fn, inner))
        emit(dict(bench="gap_probe", N=N, cost=cost,
                  seconds={key: [round(t, 7) for t in v] for key, v in times.items()},
                  lower=got["lower"]["dual"], upper=got["upper"]["fval"], gap=got["gap"],
                  lower_side=ls, upper_side=us, eval_GBps=eval_GBps, eval_bytes=by,
                  four_over_fused=min(times["four"]) / min(times["fused"]),
                  python_over_fused=min(times["python"]) / min(times["fused"]),
                  fused_not_slower=bool(max(times["fused"]) <= min(times["four"]))))
        ws.close()


def bench_run(N, reps, emit):
    xs, ys, r, l, one = points(N)

    def run(**rule):
        ws = ipd.APDWorkspace.from_points(1, xs, ys, r, l, one, one, scale=True)
        ws.warmup(0.0, 100)
        if rule:
            ws.set_gap_rule(**rule)
        ipd.get_ctx().sync()
        t0 = time.perf_counter()
        res = ws.run(AMG1, ipd.MatlabRand())
        sec = time.perf_counter() - t0
        recs = ws.gap_records()
        ws.close()
        return dict(seconds=round(sec, 4), k=int(res["k"]), converged=bool(res["converged"]),
                    gap_stop=bool(res.get("gap_stop", False)), probes=len(recs),
                    gap=recs[-1]["gap"] if recs else None, upper=recs[-1]["upper"] if recs else None,
                    best=recs[-1]["best"] if recs else None)

    run()     # unclocked
    plain, record = [], []
    for _ in range(reps):
        plain.append(run())
        record.append(run(every=1))
    emit(dict(bench="gap_run_record_only", N=N, plain=plain, record_only=record,
              record_over_plain=min(x["seconds"] for x in record) / min(x["seconds"] for x in plain)))
    for rel in (1e-3, 1e-4):
        emit(dict(bench="gap_run_stop", N=N, gap_rel=rel, kkt=plain[-1], rule=[run(gap_rel=rel) for _ in range(reps)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--size", type=int, default=1024, help="of the whole runs")
    ap.add_argument("--reps", type=int, default=2, help="alternating repetitions of the variants")
    ap.add_argument("--run", action="store_true", help="whole runs with and without a rule instead")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.run:
        bench_run(a.size, a.reps, emit)
        return
    for N in [int(s) for s in a.sizes.split(",") if s]:
        bench_probe(N, a.reps, emit)


if __name__ == "__main__":
    main()
