#!/usr/bin/env python3
"""Several right-hand sides on one hierarchy: one ipd_amg_solve_multi_dev call of k columns against k
ipd_amg_solve_dev calls, on the hierarchy as planned and on a launch-path one.

Cases (those of tools/bench_amg_pcg.py): the captured driver systems tests/golden/class1_500_k08/k20/k40,
Newton systems of the tree and hub masks at m = n = 1024 and 2048 and the regime-D system of bench.py
(m = n = 1024); drivers' options (W cycle, smoth 5, isnsp 1, bigph 1, fnode n).  k in {1, 2, 4, 8, 16}
seeded right-hand sides: column j = f (1 + 0.1 j) + 0.01 |f|_inf N(0,1), zero guess.  One JSON line per
case, k and repetition, with device-synchronised wall clocks (every entry point ends in a stream sync):
  multi     ms of ONE solve_multi call, its cycles (max and sum over the columns), ms per column, the
            smallest and largest final rel_res of the columns (likewise for the two below)
  planned   k ipd_amg_solve_dev calls on the planned hierarchy (solve mode: 0 launches, 1 single-workgroup
            solve, 2 resident kernel), summed ms, cycles, ms per column
  launched  the same on a hierarchy set up with IPD_NO_RESIDENT=1 IPD_NO_SMALL=1 (solve mode 0)
  speedup_planned / speedup_launched   their ms over the multi ms
Every case is warmed up first; --reps repetitions alternate the order of the three.

  python tools/bench_amg_multi.py [--reps 2] [--ks 1,2,4,8,16] [--cases golden,newton,regimeD] [--isnsp 1]
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

from bench_amg_pcg import cases, solve_mode  # noqa: E402


def rhs_block(f, k, seed=11):
    rs = np.random.RandomState(seed)
    s = 0.01 * np.max(np.abs(f))
    return np.column_stack([f * (1.0 + 0.1 * j) + s * rs.standard_normal(f.size) for j in range(k)])


class Dev:
    """device copies of the right-hand sides (column-major) and an output block"""

    def __init__(self, L, h, B):
        self.N, self.k = B.shape
        self.B = L.DeviceBuffer.from_array(np.asfortranarray(B).T.copy().reshape(-1), h.ctx)
        self.X = L.DeviceBuffer(8 * B.size, h.ctx)
        self.L = L

    def col(self, j):
        return ctypes.c_void_p(self.B.ptr.value + 8 * self.N * j)

    def xcol(self, j):
        return ctypes.c_void_p(self.X.ptr.value + 8 * self.N * j)


def run_multi(L, h, d):
    it = np.zeros(d.k, np.int32)
    rel = np.zeros(d.k)
    t0 = time.perf_counter()
    L.check(L.lib.ipd_amg_solve_multi_dev(h.handle, d.B.ptr, d.N, d.k, None, d.X.ptr,
                                          it.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), L.dptr(rel),
                                          None, None))
    return 1e3 * (time.perf_counter() - t0), it, rel


def run_singles(L, h, d):
    its, rels = [], []
    it = ctypes.c_int32()
    rel = ctypes.c_double()
    t0 = time.perf_counter()
    for j in range(d.k):
        L.check(L.lib.ipd_amg_solve_dev(h.handle, d.col(j), None, d.xcol(j), ctypes.byref(it), ctypes.byref(rel),
                                        None, None))
        its.append(int(it.value))
        rels.append(float(rel.value))
    return 1e3 * (time.perf_counter() - t0), np.array(its), np.array(rels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--cases", default="golden,newton,regimeD")
    ap.add_argument("--out", default=None)
    ap.add_argument("--isnsp", type=int, default=1, help="the drivers' 1; 0 to time the sweeps without the "
                    "kernel-space scalars")
    args = ap.parse_args()
    import codes_of_ipd_ssn_amg_method_amd as ipd
    from codes_of_ipd_ssn_amg_method_amd import _lib as L
    from oracle import ipd_oracle as O
    ks = [int(v) for v in args.ks.split(",")]
    sink = open(args.out, "w") if args.out else None
    for name, mk in cases(ipd, args.cases.split(",")):
        Ae, f, n = mk()
        o = O.amg_options_class1("w")
        o.update(fnode=n, isnsp=args.isnsp)
        h = ipd.AMGHierarchy(Ae, o, ipd.MatlabRand())
        os.environ["IPD_NO_RESIDENT"] = "1"
        os.environ["IPD_NO_SMALL"] = "1"
        try:
            hl = ipd.AMGHierarchy(Ae, o, ipd.MatlabRand())
        finally:
            del os.environ["IPD_NO_RESIDENT"]
            del os.environ["IPD_NO_SMALL"]
        Bmax = rhs_block(f, max(ks))
        devs = {k: (Dev(L, h, Bmax[:, :k]), Dev(L, hl, Bmax[:, :k])) for k in ks}
        for k in ks:   # warm-up (first use makes the block work vectors)
            run_multi(L, h, devs[k][0]), run_singles(L, h, devs[k][0]), run_singles(L, hl, devs[k][1])
        for rep in range(args.reps):
            for k in ks:
                d, dl = devs[k]
                rec = {"case": name, "k": k, "rep": rep, "rows": int(Ae.shape[0]), "nnz": int(Ae.nnz),
                       "levels": h.level_sizes()}
                order = ["multi", "planned", "launched"]
                if rep % 2:
                    order.reverse()
                for which in order:
                    if which == "multi":
                        ms, it, rel = run_multi(L, h, d)
                    elif which == "planned":
                        ms, it, rel = run_singles(L, h, d)
                    else:
                        ms, it, rel = run_singles(L, hl, dl)
                    rec[which] = {"ms": ms, "cycles_max": int(it.max()), "cycles_sum": int(it.sum()),
                                  "ms_per_column": ms / k, "rel_res_min": float(rel.min()),
                                  "rel_res_max": float(rel.max())}
                rec["planned"]["mode"] = solve_mode(h)
                rec["launched"]["mode"] = solve_mode(hl)
                rec["speedup_planned"] = rec["planned"]["ms"] / rec["multi"]["ms"]
                rec["speedup_launched"] = rec["launched"]["ms"] / rec["multi"]["ms"]
                line = json.dumps(rec)
                print(line, flush=True)
                if sink:
                    sink.write(line + "\n")
                    sink.flush()
        for d, dl in devs.values():
            for b in (d.B, d.X, dl.B, dl.X):
                b.free()
        h.close()
        hl.close()


if __name__ == "__main__":
    main()
