"""The drivers' host-clean script header (csrc/ipd_apd_script.h) on the CPU: a small C++ driver
(tests/apd_script_driver.cpp) is built with the system g++ against the header, with -ffp-contract=off as the library
is.  Every scalar decision apd_iterate and the warm start take comes from this header, so what runs here is what the
library runs: the step scalars, the merit and the acceptance rules bit for bit against numpy float64, the line
search's batched shape against the sequential rule of oracle/drivers.py at every position of the first acceptance and
of the cap relative to a batch edge, and the two route tables against tables written out below.  CPU only."""
import atexit
import functools
import itertools
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "codes_of_ipd_ssn_amg_method_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))

f64 = np.float64


@functools.lru_cache(maxsize=None)
def driver_exe():
    d = tempfile.mkdtemp(prefix="apd_script")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "apd_script_driver")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC,
                          os.path.join(HERE, "apd_script_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def hx(x):
    return float(x).hex()


def ask(queries):
    """queries: lists of words (floats go as hexadecimal literals); returns each answer's words after its name"""
    lines = [" ".join(hx(w) if isinstance(w, (float, np.floating)) else str(w) for w in q) for q in queries]
    res = subprocess.run([driver_exe()], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = res.stdout.strip().split("\n")
    assert out[0].startswith("limits ") and len(out) == len(queries) + 1, out[:3]
    for q, l in zip(queries, out[1:]):
        assert l.split()[0] == q[0] and l.split()[1:2] not in (["short"], ["unknown"]), (q, l)
    return [l.split()[1:] for l in out[1:]]


def bits(words):
    return [hx(float.fromhex(w)) for w in words]


def test_limits():
    res = subprocess.run([driver_exe()], input="", capture_output=True, text=True)
    assert res.stdout.split("\n")[0] == "limits MK=8"


# ---------------------------------------------------------------------------------------------------------------
# step scalars, ssn_tol, stall bound
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [1, 2])
def test_step_scalars_bit_for_bit(cls):
    cases = [(k, f64(bk), f64(tol1)) for k in (1, 2, 30) for bk in (1.0, 1e-9, 0.37) for tol1 in (1e-11, 1e-10, 1e-3)]
    out = ask([["step", k, bk, cls, tol1] for k, bk, tol1 in cases])
    for (k, bk, tol1), got in zip(cases, out):
        kk = f64(k)
        ak = np.sqrt(kk * kk * bk)                       # APD_SsN_Class1.m:113
        bk1 = bk / (f64(1.0) + ak)
        tk = bk * (f64(1.0) + ak) / (ak * ak)
        tol = max(bk1 / (kk * kk), tol1)                 # :123
        stall = tol if cls == 2 else tol / f64(100.0)    # :219 / Class2 :207
        assert bits(got) == [hx(v) for v in (ak, bk1, tk, tol, stall)], (k, bk, tol1)


def test_warm_start_recurrences_bit_for_bit():
    """warmup_class1.m:57-77: three iterations of gk, bk and every scalar the two passes take"""
    for gk0, bk0, muf in [(1.0, 1.0, 0.0), (0.7, 0.37, 0.0), (1.0, 1e-9, 0.25)]:
        got = bits(ask([["warm", f64(gk0), f64(bk0), f64(muf), 3]])[0])
        assert len(got) == 45
        gk, bk, muf = f64(gk0), f64(bk0), f64(muf)
        one = f64(1.0)
        want = []
        for _ in range(3):
            ak = bk
            bk1 = bk / (one + ak)
            gk1 = (gk + muf * ak) / (one + ak)
            etafk = (one + ak) * gk + muf * ak
            sgk = one / bk1
            etagk = (one + ak) * bk
            tt = sgk * ak * ak
            sg = one + etafk / tt
            want += [ak, gk, muf, etafk, sgk, one / bk, ak / bk, ak * ak, etafk + tt, ak * ak / etagk, gk + muf * ak,
                     one + ak, sg, gk1, bk1]
            gk, bk = gk1, bk1
        assert got == [hx(v) for v in want]


# ---------------------------------------------------------------------------------------------------------------
# merit
# ---------------------------------------------------------------------------------------------------------------
MERIT_INPUTS = [(0.31, 2.7, 10.5, -3.25, 7.125, 9.0, 1.875), (1e-9, 3e8, 1.234e3, 5.5e-4, 0.1, 0.3, 0.2),
                (0.5, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0), (0.123456789, 987.654321, 1.0 / 3.0, 2.0 / 7.0, 5.0 / 9.0, 0.7, 0.1)]


def test_merit_three_forms_bit_for_bit():
    for bk1, tk, lam2, wl, prox2, z2, zmp2 in [tuple(map(f64, t)) for t in MERIT_INPUTS]:
        f0 = bk1 / f64(2.0) * lam2 - wl                              # :182
        low = f0 + f64(0.5) * tk * prox2                             # :184, prob < 3
        high = f0 + f64(0.5) * tk * (z2 - zmp2)                      # :186, prob 3
        fixed = bk1 / f64(2.0) * lam2 - wl + f64(0.5) * tk * prox2   # what ipd_apd_eval reports: the prob < 3 form
        out = ask([["merit", 0, bk1, tk, lam2, wl, prox2, z2, zmp2], ["merit", 1, bk1, tk, lam2, wl, prox2, z2, zmp2]])
        assert bits(out[0]) == [hx(low)] and bits(out[1]) == [hx(high)]
        assert hx(fixed) == hx(low)


# ---------------------------------------------------------------------------------------------------------------
# acceptance of a step, the loop's stop tests
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [1, 2])
def test_max_rr_and_restart_bit_for_bit(cls):
    kks = [(3e-3, 2e-5, 0.5, 4e-7), (1e-9, 5.0, 1e-3, 80.0), (0.0, 0.0, 0.0, 0.0)]
    kkt0s = [(10.0, 0.25, 3.0, 1e-4), (0.0, 0.0, 0.0, 0.0)]
    for kk, k0 in itertools.product(kks, kkt0s):
        kk, k0 = [f64(v) for v in kk], [f64(v) for v in k0]
        one = f64(1.0)
        rr = max(kk[0] / (one + k0[0]), kk[1] / (one + k0[1]))        # :243 / Class2 :229
        resk = max(kk[0], kk[1])
        if cls == 2:
            rr = max(max(rr, kk[2] / (one + k0[2])), kk[3] / (one + k0[3]))
            resk = max(max(resk, kk[2]), kk[3])
        # the restart test bk1 < 1e-8 && rr > resk at and around both of its edges
        for bk1, res_in in [(9.9e-9, rr), (9.9e-9, np.nextafter(rr, f64(-1.0))), (1e-8, f64(0.0)),
                            (np.nextafter(f64(1e-8), f64(0.0)), f64(-1.0)), (0.37, f64(-1.0))]:
            bk1 = f64(bk1)
            got = ask([["accept", cls, bk1, res_in] + kk + k0])[0]
            assert bits(got[:2]) == [hx(rr), hx(resk)]
            assert int(got[2]) == int(bool(bk1 < f64(1e-8) and rr > res_in)), (bk1, rr, res_in)
            assert bits(got[3:]) == [hx(f64(10.0) * bk1)]             # Class2 :255


def test_stop_tests():
    tol = f64(1e-6)
    up, down = np.nextafter(tol, f64(1.0)), np.nextafter(tol, f64(0.0))
    for cls in (1, 2):
        bound = tol if cls == 2 else tol / f64(100.0)
        cases = [(f64(1.0), tol, 3, 50), (f64(1.0), up, 3, 50), (f64(1.0), down, 50, 50),
                 (f64(0.5) + bound, f64(0.5), 1, 50), (f64(0.5) + np.nextafter(bound, f64(0.0)), f64(0.5), 1, 50),
                 (f64(0.5), f64(0.5) + f64(2.0) * bound, 49, 50), (f64(1.0), f64("nan"), 7, 50)]
        out = ask([["stop", cls, old, new, tol, it, itmax] for old, new, it, itmax in cases])
        for (old, new, it, itmax), got in zip(cases, out):
            want = [new > tol, new <= tol, abs(old - new) < bound, it == itmax]   # :137, :213, :219, :226
            assert [int(g) for g in got] == [int(bool(w)) for w in want], (cls, old, new, it)


# ---------------------------------------------------------------------------------------------------------------
# route tables
# ---------------------------------------------------------------------------------------------------------------
def test_inner_solver_routes():
    """the arm apd_iterate's if-ladder took for every (cls, inner_solver)"""
    want = {(1, 1): "DIRECT", (2, 1): "DIRECT_POT",       # build_jk + spd_solve_dev / direct_pot_dev
            (1, 2): "PCG", (2, 2): "PCG_POT",             # build_jk + pcg_dev / pcg_pot_dev
            (1, 3): "AUG_PCG", (2, 3): "PCG4POT",         # aug_pcg_dev / pcg4pot_dev
            (1, 4): "HYBRID_AMG", (2, 4): "AMG4POT",      # hybrid_amg_dev / amg4pot_dev
            (1, 5): "HYBRID_AMG", (2, 5): "AMG4POT"}      # the same with the two-grid options
    out = ask([["route", c, s] for c, s in want])
    assert {k: g[0] for k, g in zip(want, out)} == want


def test_eval_instantiations():
    """OpEvalT<CLS2, GVEC, M3>: five instantiations exist; class 2 has one and ignores the other two inputs"""
    want = {(1, 0, 0): "GS", (1, 0, 1): "GS_M3", (1, 1, 0): "GVEC", (1, 1, 1): "GVEC_M3",
            (2, 0, 0): "CLS2", (2, 0, 1): "CLS2", (2, 1, 0): "CLS2", (2, 1, 1): "CLS2"}
    out = ask([["evalkind", c, g, m3] for c, g, m3 in want])
    assert {k: g[0] for k, g in zip(want, out)} == want


def test_eval_bytes():
    for (m, n), phi, gama in itertools.product([(500, 500), (300, 147), (4096, 4096)], (0, 1), (0, 1)):
        mn = float(m * n)
        nib, njg = -(-m // 256), -(-n // 16)       # reps = 1 at these sizes (tests/test_apd_geo.py)
        want = 8.0 * mn + mn + 16.0 * (m + n) + (8.0 * mn if phi else 0.0) + (8.0 * mn if gama else 0.0)
        want += 8.0 * (float(njg) * m + 4.0 * nib * n)
        assert bits(ask([["bytes", m, n, phi, gama]])[0]) == [hx(want)]


# ---------------------------------------------------------------------------------------------------------------
# line search
# ---------------------------------------------------------------------------------------------------------------
DELTA, NU, RESS, CF_OLD = f64(0.9), f64(0.2), f64(2.0), f64(1.0)
FIRST = [0, 1, 7, 8, 9, 15, 16, 17, None]            # the first accepted trial; None: never
LL_MAX = [0, 1, 7, 8, 9, 16, 17, 500]


def threshold(ll):
    return CF_OLD - NU * DELTA ** ll * RESS


def merit_sequence(first, nan, length):
    """cF(ll): just above the Armijo threshold of trial ll (rejected) everywhere but at `first`, where it sits ON the
    threshold (not greater: accepted) or is a NaN (not greater either).  A later trial is rejected again, so a pick
    that is not the FIRST acceptance shows."""
    seq = [np.nextafter(threshold(ll), f64(2.0)) for ll in range(length)]
    if first is not None:
        seq[first] = f64("nan") if nan else threshold(first)
    return seq


def oracle_rule(cF, ll_max):
    """oracle/drivers.py:116-125, the sequential rule, over a merit sequence"""
    ll = 0
    while True:
        cF_new = cF[ll]
        if not (cF_new > CF_OLD - NU * DELTA ** ll * RESS) or ll == ll_max:
            break
        ll += 1
    return ll, DELTA ** ll


def ls_query(arm, cF, ll_max, merit3):
    return ["ls", arm, DELTA, NU, RESS, CF_OLD, ll_max, merit3, f64(1e300)] + list(cF)


def _ls(got):
    f = dict(tok.split("=") for tok in got)
    return f["arm"], int(f["ll"]), hx(float.fromhex(f["step"])), int(f["passes"])


@pytest.mark.parametrize("nan", [False, True])
def test_batched_line_search_is_the_sequential_rule(nan):
    """The batched functions, driven by apd_iterate's loop after a rejected first trial, stop where the sequential
    rule of oracle/drivers.py stops: every first acceptance x every cap, i.e. both on either side of a batch edge
    (MK = 8) and beyond one another."""
    cases = [(first, ll_max) for first in FIRST for ll_max in LL_MAX if not (nan and first is None)]
    seqs = [merit_sequence(first, nan, ll_max + 20) for first, ll_max in cases]
    out = ask([ls_query("batched", s, ll_max, 0) for s, (_, ll_max) in zip(seqs, cases)])
    for (first, ll_max), s, got in zip(cases, seqs, out):
        ll, step = oracle_rule(s, ll_max)
        assert ll == (ll_max if first is None else min(first, ll_max))     # the sequence does what it is meant to
        arm, gll, gstep, passes = _ls(got)
        assert (gll, gstep) == (ll, hx(step)), (first, ll_max, got)
        assert arm == ("none" if first == 0 else "batched")
        if first != 0:   # one pass per batch of MK trials up to the accepted (or last allowed) one
            assert passes == -(-ll // 8), (first, ll_max, got)


@pytest.mark.parametrize("merit3", [0, 1])
def test_line_search_as_apd_iterate_selects_it(merit3):
    """arm = auto: the rule that selects the batched shape (first trial rejected, not merit3, ll_max > 0) and then the
    selected arm.  From ll_max = 1 on both arms give the oracle's ll and step.  At ll_max = 0 the sequential arm is
    the scripts' own loop (APD_SsN_Class1.m:199-210), which tests `ll == ll_max` only after it has raised ll and so
    does not stop at trial 0 as oracle/drivers.py does: the batched shape must not take that case over, and which arm
    runs is all this test says about it."""
    cases = [(first, ll_max) for first in FIRST for ll_max in LL_MAX if ll_max > 0]
    seqs = [merit_sequence(first, False, ll_max + 20) for first, ll_max in cases]
    out = ask([ls_query("auto", s, ll_max, merit3) for s, (_, ll_max) in zip(seqs, cases)])
    for (first, ll_max), s, got in zip(cases, seqs, out):
        ll, step = oracle_rule(s, ll_max)
        arm, gll, gstep, _ = _ls(got)
        assert (gll, gstep) == (ll, hx(step)), (first, ll_max, got)
        assert arm == ("none" if first == 0 else "sequential" if merit3 else "batched"), (first, ll_max, got)
    # ll_max = 0: never batched.  (first = 1: the sequential arm stops at trial 1 in the scripts' way)
    for m3 in (0, 1):
        arm, gll, _, _ = _ls(ask([ls_query("auto", merit_sequence(1, False, 20), 0, m3)])[0])
        assert (arm, gll) == ("sequential", 1)
        assert _ls(ask([ls_query("auto", merit_sequence(0, False, 20), 0, m3)])[0])[:2] == ("none", 0)


def test_trial_steps_are_powers_of_delta():
    out = ask([ls_query("batched", merit_sequence(ll, False, 40), 500, 0) for ll in range(1, 20)])
    for ll, got in zip(range(1, 20), out):
        assert _ls(got)[1:3] == (ll, hx(math.pow(0.9, float(ll))))
