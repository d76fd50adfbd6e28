#!/usr/bin/env python3
"""AMG-preconditioned CG (AMGHierarchy.pcg) against the stationary Class_AMG solve on the same hierarchy.

Cases: the captured driver systems tests/golden/class1_500_k08/k20/k40, Newton systems of the tree and
hub masks at m = n = 1024 and 2048 (bench.build_newton_system) and the regime-D system of bench.py
(m = n = 1024, Bernoulli rho = 1).  Drivers' options (W cycle, smoth 5, isnsp 1, bigph 1, fnode n).
One JSON line per case and repetition:
  stationary      it, rel_res, wall ms of AMGHierarchy.solve (ends in a device sync), solve mode
                  (ipd_amg_solve_mode: 0 launches, 1 single-workgroup solve, 2 resident kernel)
  launched        the same solve on a hierarchy set up with IPD_NO_RESIDENT=1 IPD_NO_SMALL=1:
                  ms per cycle of the launch path (what AMG-PCG runs)
  pcg             it, res, true relative residual |A d - e| / |e|, wall ms
  planned         the same for AMGHierarchy.pcg(planned=True) and pcg_mode (1: the whole loop was ONE
                  single-workgroup launch; 0: it ran as `pcg` does)
  overhead_us     (pcg_ms - it * launched_cycle_ms) / it: K1-K3 plus the per-iteration read
Every case is warmed up first; --reps repetitions alternate the order of the solvers.
--variant v1 runs the cases with a V cycle and one smoothing sweep instead of the drivers' options.

  python tools/bench_amg_pcg.py [--reps 2] [--cases golden,newton,regimeD] [--variant driver|v1] [--out FILE]"""
import argparse
import json
import os
import sys
import time
from ctypes import byref, c_int32

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def golden(name):
    from oracle import ipd_oracle as O
    from tests.test_golden_oracle import load, problem_from
    pd = problem_from(load(name))
    H0 = O.ASAt(pd["s"], pd["p"], pd["q"])
    Ae = O.build_Ae(H0, pd["T"], pd["p"], pd["q"], pd["bk1"], pd["tk"])[0]
    f = np.concatenate([pd["q"], -pd["p"]]) * pd["z"]
    return sp.csr_matrix(Ae), f, pd["n"]


def cases(ipd, which):
    import bench
    out = []
    if "golden" in which:
        for k in (8, 20, 40):
            name = "class1_500_k%02d" % k
            out.append((name, lambda name=name: golden(name + ".npz")))
    if "newton" in which:
        for n1 in (1024, 2048):
            for kind in ("tree", "hub"):
                def mk(n1=n1, kind=kind):
                    s = bench.build_mask(n1, n1, kind, 1.0)
                    Ae, f, _, _ = bench.build_newton_system(ipd, n1, n1, s)
                    return Ae, f, n1
                out.append(("newton_%s_%d" % (kind, n1), mk))
    if "regimeD" in which:
        def mkd():
            s = bench.build_mask(1024, 1024, "bernoulli", 1.0)
            Ae, f, _, _ = bench.build_newton_system(ipd, 1024, 1024, s)
            return Ae, f, 1024
        out.append(("regimeD_1024", mkd))
    return out


def solve_mode(h):
    from codes_of_ipd_ssn_amg_method_amd import _lib as L
    mode, grid, tmo = c_int32(), c_int32(), c_int32()
    L.check(L.lib.ipd_amg_solve_mode(h.handle, byref(mode), byref(grid), byref(tmo)))
    return int(mode.value)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--cases", default="golden,newton,regimeD")
    ap.add_argument("--variant", default="driver", choices=["driver", "v1"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import codes_of_ipd_ssn_amg_method_amd as ipd
    from oracle import ipd_oracle as O
    sink = open(args.out, "w") if args.out else None
    po = dict(retol=1e-11, maxit=500)
    built = []
    for name, mk in cases(ipd, args.cases.split(",")):
        Ae, f, n = mk()
        o = O.amg_options_class1("w" if args.variant == "driver" else "v")
        o.update(fnode=n)
        if args.variant == "v1":
            o.update(smoth=1)
        h = ipd.AMGHierarchy(Ae, o, ipd.MatlabRand())
        os.environ["IPD_NO_RESIDENT"] = "1"
        os.environ["IPD_NO_SMALL"] = "1"
        try:
            hl = ipd.AMGHierarchy(Ae, o, ipd.MatlabRand())
        finally:
            del os.environ["IPD_NO_RESIDENT"]
            del os.environ["IPD_NO_SMALL"]
        h.solve(f), hl.solve(f), h.pcg(f, po), h.pcg(f, po, planned=True)          # warm-up
        built.append((name, Ae, f, h, hl))
    for rep in range(args.reps):
        for name, Ae, f, h, hl in built:
            order = ("stationary", "pcg", "planned") if rep % 2 == 0 else ("planned", "pcg", "stationary")
            rec = {"case": name, "variant": args.variant, "rep": rep, "rows": int(Ae.shape[0]), "nnz": int(Ae.nnz), "levels": h.level_sizes()}
            for which in order:
                if which == "stationary":
                    (x, it, rr, _, _), ms = timed(lambda: h.solve(f))
                    rec["stationary"] = {"it": it, "rel_res": rr, "ms": ms, "mode": solve_mode(h)}
                    (x, itl, rrl, _, _), msl = timed(lambda: hl.solve(f))
                    rec["launched"] = {"it": itl, "ms": msl, "mode": solve_mode(hl),
                                       "ms_per_cycle": msl / max(itl, 1)}
                elif which == "pcg":
                    (d, it, res, _), ms = timed(lambda: h.pcg(f, po))
                    tr = float(np.linalg.norm(Ae @ d - f) / np.linalg.norm(f))
                    rec["pcg"] = {"it": it, "res": res, "true_rel_res": tr, "ms": ms}
                else:
                    (d, it, res, _), ms = timed(lambda: h.pcg(f, po, planned=True))
                    tr = float(np.linalg.norm(Ae @ d - f) / np.linalg.norm(f))
                    rec["planned"] = {"it": it, "res": res, "true_rel_res": tr, "ms": ms, "mode": h.pcg_mode}
            it = max(rec["pcg"]["it"], 1)
            rec["overhead_us"] = 1e3 * (rec["pcg"]["ms"] - it * rec["launched"]["ms_per_cycle"]) / it
            rec["planned_speedup"] = rec["pcg"]["ms"] / rec["planned"]["ms"]
            line = json.dumps(rec)
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
                sink.flush()
    for _, _, _, h, hl in built:
        h.close()
        hl.close()


if __name__ == "__main__":
    main()
