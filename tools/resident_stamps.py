#!/usr/bin/env python3
"""In-kernel stamps of the level-resident solve kernel on the metric workload (bench.py's
system): where a cycle's time goes inside workgroup 0 -- waiting in hand-off sweeps against
everything else (row dot products, reductions, barriers, transfers, tail solve).
  python tools/resident_stamps.py [--n1 1024] [--cycle v] [--cycles 200] [--no-poly2] [--by-class]
--by-class (the column-slice kernels): workgroup 0's time by class of hand-off, each charged from its start to the
start of the next hand-off -- the level-1 half sweeps, the first half sweep of each run (a barrier of its own),
and the other hand-offs of a cycle each on its own (ipd_amg_bench_resident_classes)."""
import argparse
import os
import sys
from ctypes import byref, c_double, c_int, c_int64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n1", type=int, default=1024)
    ap.add_argument("--rho", type=float, default=1.0)
    ap.add_argument("--cycle", default="v")
    ap.add_argument("--cycles", type=int, default=200)
    ap.add_argument("--no-poly2", action="store_true", help="level 2 as sweeps (33 hand-offs per V cycle)")
    ap.add_argument("--by-class", action="store_true", help="stamps by class of hand-off")
    a = ap.parse_args()
    import codes_of_ipd_ssn_amg_method_amd as ipd
    from codes_of_ipd_ssn_amg_method_amd import _lib
    m = n = a.n1
    s = bench.build_mask(m, n, "bernoulli", a.rho)
    Ae, f, guess, H0 = bench.build_newton_system(ipd, m, n, s)
    opts = dict(retol=1e-11, bigph=1, maxit=30, theta=0.25, smoth=5, cycle=a.cycle, isnsp=1, inter=1, fnode=n)
    h = ipd.AMGHierarchy(Ae, opts, ipd.MatlabRand())
    print("level 1 <-> 2 transfers from the bit mask:", h.attach_mask_transfers(np.ones(m), np.ones(n), bench.TK))
    if a.cycle == "v" and not a.no_poly2:
        print("level 2 composed over a visit (ipd_amg_attach_level2_poly):", h.attach_level2_poly())
    from ctypes import c_int32, create_string_buffer
    name = create_string_buffer(64)
    _lib.check(_lib.lib.ipd_amg_resident_kernel(h.handle, name, c_int32(64), None, None, None))
    colslice = name.value.decode().startswith("k_resident<16,16,0")   # only these write stamps[9] (no remote tail here)
    print("kernel:", name.value.decode())
    db = _lib.DeviceBuffer.from_array(f)
    dx = _lib.DeviceBuffer.from_array(guess)
    st = (c_int64 * 10)()
    ms = c_double()
    if a.by_class:
        by_class(_lib, h, db, dx, a.cycles)
        return
    for rep in range(3):
        _lib.check(_lib.lib.ipd_amg_bench_resident(h.handle, db.ptr, dx.ptr, c_int(a.cycles), byref(ms), st))
        wait, tot, nh, ticks, bar1, store, bar2, xfer, tail, fin = [int(v) for v in st][:10]
        if not colslice:
            fin = 0
        # (stamps[9]: the finishing lanes of the column-slice half sweeps -- this system has no remote tail,
        # whose busy time the slot carries otherwise.  A column-slice half sweep has ONE barrier, counted as the
        # barrier before the publish, and no store phase of its own: "store+sums" is then receipt -> products ->
        # butterfly -> PART, and the closing barrier is that of the other hand-offs alone.)
        clk_mhz = tot / (ticks / 100.0)
        print("cycles=%d  %.3f ms  -> %.2f us/cycle, %d hand-offs (%.1f per cycle, %.2f us each); "
              "workgroup 0: waiting in sweeps %.1f %% (%.2f us per hand-off), shader clock %.0f MHz"
              % (a.cycles, ms.value, 1e3 * ms.value / a.cycles, nh, nh / a.cycles,
                 1e3 * ms.value / nh, 100.0 * wait / tot, wait / clk_mhz / nh, clk_mhz))
        rest = tot - wait - bar1 - store - bar2 - xfer - tail - fin
        print("   per cycle (us): transfers P'rr, P e_2 %.2f | tail level %.2f" % (
            xfer / clk_mhz / a.cycles, tail / clk_mhz / a.cycles))
        print("   per hand-off (us): row work %.2f | barrier before publish %.2f | finishing lanes %.2f | sweep wait %.2f | "
              "store+sums %.2f | closing barrier %.2f" % tuple(v / clk_mhz / nh for v in (rest, bar1, fin, wait, store, bar2)))


CLASSES = ["level-1 half sweep (fed)", "first half sweep of a run", "rr = r - A e", "restriction r_2 = P'rr",
           "level 2", "prolongation e_1 += P e_2", "top r = b - A x"]


def by_class(_lib, h, db, dx, cycles):
    st = (c_int64 * 32)()
    ms = c_double()
    for rep in range(3):
        _lib.check(_lib.lib.ipd_amg_bench_resident_classes(h.handle, db.ptr, dx.ptr, c_int(cycles), byref(ms), st))
        v = [int(x) for x in st]
        clk_mhz = v[1] / (v[3] / 100.0)
        clocks, counts = v[16:24], v[24:32]
        print("cycles=%d  %.3f ms (stamped) -> %.2f us/cycle, %d hand-offs, %d in classes, shader clock %.0f MHz"
              % (cycles, ms.value, 1e3 * ms.value / cycles, v[2], sum(counts), clk_mhz))
        for c, name in enumerate(CLASSES):
            if counts[c]:
                print("   %-28s %5.1f per cycle  %6.3f us each  %6.2f us per cycle" % (
                    name, counts[c] / cycles, clocks[c] / clk_mhz / counts[c], clocks[c] / clk_mhz / cycles))
        print("   all classes %.2f us per cycle" % (sum(clocks) / clk_mhz / cycles))


if __name__ == "__main__":
    main()
