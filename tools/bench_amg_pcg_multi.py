#!/usr/bin/env python3
"""AMG-preconditioned CG for several right-hand sides: one ipd_amg_pcg_multi_dev call of k columns against
k ipd_amg_pcg_dev calls and against one ipd_amg_solve_multi_dev call (the stationary loop) on the same
columns and the same hierarchy.

Cases (those of tools/bench_amg_pcg.py and tools/bench_amg_multi.py): the captured driver systems
tests/golden/class1_500_k08/k20/k40, Newton systems of the tree and hub masks at m = n = 1024 and 2048 and
the regime-D system of bench.py (m = n = 1024); drivers' options (W cycle, smoth 5, isnsp 1, bigph 1,
fnode n).  k in {1, 2, 4, 8, 16} seeded right-hand sides: column j = f (1 + 0.1 j) + 0.01 |f|_inf N(0,1),
zero guess; PCG with retol 1e-11, maxit 500.  One JSON line per case, k and repetition, with
device-synchronised wall clocks (every entry point ends in a stream sync):
  pcg_multi    ms of ONE pcg_multi call, its iterations (max and sum over the columns), ms per column,
               the largest final res of the columns
  pcg_singles  k ipd_amg_pcg_dev calls, summed ms, iterations, ms per column, largest res
  solve_multi  one ipd_amg_solve_multi_dev call (cycles instead of iterations), its largest rel_res
  speedup_vs_singles   pcg_singles ms over pcg_multi ms
Every case is warmed up first; --reps repetitions alternate the order of the three, and a last line per
case and k gives the spread of the repetitions (max/min - 1 of each timing).

  python tools/bench_amg_pcg_multi.py [--reps 2] [--ks 1,2,4,8,16] [--cases golden,newton,regimeD]
                                      [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_amg_multi import Dev, rhs_block  # noqa: E402
from bench_amg_pcg import cases  # noqa: E402

RETOL, MAXIT = 1e-11, 500
I64 = ctypes.POINTER(ctypes.c_int64)
I32 = ctypes.POINTER(ctypes.c_int32)


def pcg_opts(L):
    o = L.ipd_pcg_opts()
    L.lib.ipd_pcg_opts_init(ctypes.byref(o))
    o.retol = RETOL
    o.maxit = MAXIT
    return o


def run_pcg_multi(L, h, d, o):
    it = np.zeros(d.k, np.int64)
    res = np.zeros(d.k)
    t0 = time.perf_counter()
    L.check(L.lib.ipd_amg_pcg_multi_dev(h.handle, d.B.ptr, d.N, d.k, None, ctypes.byref(o), d.X.ptr,
                                        it.ctypes.data_as(I64), L.dptr(res), None))
    return 1e3 * (time.perf_counter() - t0), it, res


def run_pcg_singles(L, h, d, o):
    its, ress = [], []
    it = ctypes.c_int64()
    res = ctypes.c_double()
    t0 = time.perf_counter()
    for j in range(d.k):
        L.check(L.lib.ipd_amg_pcg_dev(h.handle, d.col(j), None, ctypes.byref(o), d.xcol(j), ctypes.byref(it),
                                      ctypes.byref(res), None))
        its.append(int(it.value))
        ress.append(float(res.value))
    return 1e3 * (time.perf_counter() - t0), np.array(its), np.array(ress)


def run_solve_multi(L, h, d):
    it = np.zeros(d.k, np.int32)
    rel = np.zeros(d.k)
    t0 = time.perf_counter()
    L.check(L.lib.ipd_amg_solve_multi_dev(h.handle, d.B.ptr, d.N, d.k, None, d.X.ptr, it.ctypes.data_as(I32),
                                          L.dptr(rel), None, None))
    return 1e3 * (time.perf_counter() - t0), it, rel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--cases", default="golden,newton,regimeD")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import codes_of_ipd_ssn_amg_method_amd as ipd
    from codes_of_ipd_ssn_amg_method_amd import _lib as L
    from oracle import ipd_oracle as O
    ks = [int(v) for v in args.ks.split(",")]
    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    o_pcg = pcg_opts(L)
    for name, mk in cases(ipd, args.cases.split(",")):
        Ae, f, n = mk()
        o = O.amg_options_class1("w")
        o.update(fnode=n, isnsp=1)
        h = ipd.AMGHierarchy(Ae, o, ipd.MatlabRand())
        Bmax = rhs_block(f, max(ks))
        devs = {k: Dev(L, h, Bmax[:, :k]) for k in ks}
        for k in ks:   # warm-up (first use makes the block work vectors)
            run_pcg_multi(L, h, devs[k], o_pcg), run_pcg_singles(L, h, devs[k], o_pcg), run_solve_multi(L, h, devs[k])
        times = {k: {"pcg_multi": [], "pcg_singles": [], "solve_multi": []} for k in ks}
        for rep in range(args.reps):
            for k in ks:
                d = devs[k]
                rec = {"case": name, "k": k, "rep": rep, "rows": int(Ae.shape[0]), "nnz": int(Ae.nnz),
                       "levels": h.level_sizes()}
                order = ["pcg_multi", "pcg_singles", "solve_multi"]
                if rep % 2:
                    order.reverse()
                for which in order:
                    if which == "pcg_multi":
                        ms, it, res = run_pcg_multi(L, h, d, o_pcg)
                    elif which == "pcg_singles":
                        ms, it, res = run_pcg_singles(L, h, d, o_pcg)
                    else:
                        ms, it, res = run_solve_multi(L, h, d)
                    key = "cycles" if which == "solve_multi" else "iterations"
                    rec[which] = {"ms": ms, "ms_per_column": ms / k, key + "_max": int(it.max()),
                                  key + "_sum": int(it.sum()), "res_max": float(np.max(res))}
                    times[k][which].append(ms)
                rec["speedup_vs_singles"] = rec["pcg_singles"]["ms"] / rec["pcg_multi"]["ms"]
                emit(rec)
        for k in ks:
            emit({"case": name, "k": k, "spread": {w: max(v) / min(v) - 1.0 for w, v in times[k].items()}})
        for d in devs.values():
            d.B.free()
            d.X.free()
        h.close()


if __name__ == "__main__":
    main()
