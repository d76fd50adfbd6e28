"""The decisions of the stopping rule on the certified gap (csrc/ipd_apd_script.h: apd_gap_due, apd_gap_lower_side,
apd_gap_upper_side, apd_gap_best, apd_gap_threshold, apd_gap_stops) on the CPU: a small C++ driver
(tests/gap_rule_driver.cpp) is built with the system g++ against the header, with -ffp-contract=off as the library is.
ipd_bracket.hip and the probe of ipd_apd_run call these functions and restate none of them, so what runs here is what
the library runs.  The two picks are held to the expressions of APDWorkspace.certificate and APDWorkspace.bracket.  CPU
only."""
import atexit
import functools
import itertools
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "codes_of_ipd_ssn_amg_method_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))

INF, NAN = math.inf, math.nan
SPECIAL = [0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -52, 5e-324, INF, -INF, NAN]


@functools.lru_cache(maxsize=None)
def driver_exe():
    d = tempfile.mkdtemp(prefix="gap_rule")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "gap_rule_driver")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC,
                          os.path.join(HERE, "gap_rule_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def word(w):
    return float(w).hex() if isinstance(w, (float, np.floating)) else str(w)


def ask(queries):
    """queries: lists of words (floats go as hexadecimal literals); returns each answer's words after its name"""
    lines = [" ".join(word(w) for w in q) for q in queries]
    res = subprocess.run([driver_exe()], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = res.stdout.strip().split("\n")
    assert len(out) == len(queries), (len(out), len(queries))
    for q, l in zip(queries, out):
        assert l.split()[0] == q[0] and l.split()[1:2] not in (["short"], ["unknown"]), (q, l)
    return [l.split()[1:] for l in out]


def same_double(got_word, want):
    got = float.fromhex(got_word) if "x" in got_word else float(got_word)
    if math.isnan(want):
        return math.isnan(got)
    return got == want and math.copysign(1.0, got) == math.copysign(1.0, want)


def values(seed, count):
    rs = np.random.RandomState(seed)
    return [float(v) for v in rs.standard_normal(count)] + SPECIAL


def test_schedule():
    """due = converged || (k >= first && (k - first) % every == 0): probes after first, first + every, ..."""
    cases = list(itertools.product(range(1, 24), (1, 2, 3, 7), (1, 2, 3, 5, 1000), (0, 1)))
    out = ask([["due", k, first, every, conv] for k, first, every, conv in cases])
    for (k, first, every, conv), got in zip(cases, out):
        want = bool(conv) or k in range(first, 10000, every)
        assert got == [str(int(want))], (k, first, every, conv)
    # first = 3, every = 2 over eight iterations: 3, 5, 7
    out = ask([["due", k, 3, 2, 0] for k in range(1, 9)])
    assert [k for k, g in zip(range(1, 9), out) if g == ["1"]] == [3, 5, 7]


def test_lower_pick_is_certificates():
    vals = values(1, 12)
    cases = list(itertools.product(vals, vals))
    out = ask([["lower", d0, d1] for d0, d1 in cases])
    for (d0, d1), got in zip(cases, out):
        assert got == [str(1 if d1 > d0 else 0)], (d0, d1)       # APDWorkspace.certificate


def test_upper_pick_is_brackets():
    vals = values(2, 8)
    cases = list(itertools.product((0, 1), vals, (0, 1), vals))
    out = ask([["upper", ok0, f0, ok1, f1] for ok0, f0, ok1, f1 in cases])
    for (ok0, f0, ok1, f1), got in zip(cases, out):
        ok, fval = (ok0, ok1), (f0, f1)
        want = min((0, 1), key=lambda s: (not ok[s], fval[s]))   # APDWorkspace.bracket; a NaN never compares less
        assert got == [str(want)], (ok0, f0, ok1, f1)
    # equal values and signed zeros keep side 0
    assert ask([["upper", 1, 0.0, 1, -0.0], ["upper", 1, 2.5, 1, 2.5], ["upper", 0, 1.0, 1, INF],
                ["upper", 1, -INF, 0, -INF]]) == [["0"], ["0"], ["1"], ["0"]]


def test_best_update_bit_for_bit():
    vals = values(3, 12)
    cases = list(itertools.product(vals, vals))
    out = ask([["best", lo, best] for lo, best in cases])
    for (lo, best), got in zip(cases, out):
        want = lo if lo > best else best
        assert got[0] == str(int(lo > best)) and same_double(got[1], want), (lo, best, got)
    # from -inf the first finite lower bound enters; a NaN never does
    assert ask([["best", -3.5, -INF]])[0][0] == "1" and ask([["best", NAN, -INF]])[0][0] == "0"


def test_threshold_and_gap_bit_for_bit():
    rs = np.random.RandomState(4)
    tols = [0.0, 1e-6, 1e-2, float(rs.random_sample())]
    uppers = values(5, 10)
    cases = list(itertools.product(tols, tols, uppers))
    out = ask([["thr", gt, gr, up] for gt, gr, up in cases])
    for (gt, gr, up), got in zip(cases, out):
        with np.errstate(invalid="ignore"):
            rel = np.float64(gr) * np.abs(np.float64(up))      # 0 * inf is a NaN, which leaves gap_tol
        want = float(rel) if rel > gt else gt
        assert same_double(got[0], want), (gt, gr, up, got)
    assert same_double(ask([["thr", 0.0, 0.0, 3.0]])[0][0], 0.0)
    assert same_double(ask([["thr", 1e-3, 1e-3, NAN]])[0][0], 1e-3)      # a NaN upper leaves gap_tol
    pairs = list(itertools.product(uppers, uppers))
    with np.errstate(invalid="ignore"):
        for (up, best), got in zip(pairs, ask([["gap", up, best] for up, best in pairs])):
            assert same_double(got[0], float(np.float64(up) - np.float64(best))), (up, best, got)


def test_stop():
    """stop = thr > 0 && upper_ok && gap <= thr"""
    vals = [0.0, -0.0, 1e-3, 1e-3 * (1 + 2.0 ** -52), 1e-3 * (1 - 2.0 ** -53), -1.0, INF, -INF, NAN]
    cases = list(itertools.product([0.0, 1e-3, INF, NAN], (0, 1), vals))
    out = ask([["stop", thr, ok, gap] for thr, ok, gap in cases])
    for (thr, ok, gap), got in zip(cases, out):
        assert got == [str(int(thr > 0 and ok != 0 and gap <= thr))], (thr, ok, gap)
    assert ask([["stop", 1e-3, 1, NAN], ["stop", 1e-3, 0, 0.0], ["stop", 0.0, 1, 0.0], ["stop", 1e-3, 1, 1e-3],
                ["stop", 1e-3, 1, 1e-3 * (1 + 2.0 ** -52)]]) == [["0"], ["0"], ["0"], ["1"], ["0"]]
