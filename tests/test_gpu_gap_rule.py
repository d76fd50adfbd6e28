"""The drivers' stopping rule on the certified gap (csrc/ipd_driver.hip: ipd_apd_set_gap_rule, ipd_apd_gap_records,
ipd_apd_gap_lam, the probe of ipd_apd_run; APDWorkspace.set_gap_rule, gap_records, gap_lam; the gap_* keywords of the
four drivers).

Problems: tests/test_gpu_round.py's problem(cls, m, n, seed=12) at 24 x 24 and 37 x 29, both classes, from the drivers'
warm start.  Two references.  Bit for bit: the loop the rule replaces -- single steps of run() with bracket() after
each, which the suite holds to numpy restatements elsewhere.  For where a run stops: the CPU oracle's trajectory
(oracle/drivers.py with the direct inner solver), its certificates through tests/round_ref.py and a numpy c-transform;
the threshold is put between two consecutive gaps of that trajectory, a factor of at least 1.3 away from either, so
that the device's AMG-solved trajectory, which agrees with the oracle's far closer than that, stops at the same
iteration."""
import functools

import numpy as np
import pytest

from oracle import drivers as D
from tests import round_ref as R
from tests import test_gpu_dual as TD
from tests import test_gpu_round as TR

pytestmark = pytest.mark.gpu

INF = np.inf
CASES = [(1, 24, 24), (1, 37, 29), (2, 24, 24), (2, 37, 29)]
NSTEP = 9
ipd, lib_mod, problem, ws_of, same_bits = TR.ipd, TR.lib_mod, TR.problem, TR.ws_of, TR.same_bits
REC_KEYS = ("k", "lower_side", "upper_side", "upper_ok", "stop", "final", "lower", "lower_dmin", "best", "upper",
            "viol_in", "gap")


def amg(cls):
    return TR.AMG1 if cls == 1 else TR.AMG2


def started(cls, m, n, **kw):
    """a workspace at the drivers' warm start, with its own rand stream"""
    ws = ws_of(cls, problem(cls, m, n, seed=12))
    ws.warmup(0.0, 100)
    if kw:
        ws.set_gap_rule(**kw)
    return ws, ipd().MatlabRand()


def snapshot(ws):
    """everything a run leaves behind, in comparable form"""
    u, v, lam, bk = ws.state()
    return dict(u=u, v=v, lam=lam, bk=bk, hist=ws.history(), recs=repr(ws.records()), reuse=ws.reuse_stats())


def same_snapshot(a, b):
    return (same_bits(a["u"], b["u"]) and same_bits(a["v"], b["v"]) and same_bits(a["lam"], b["lam"])
            and a["bk"] == b["bk"] and a["hist"].keys() == b["hist"].keys()
            and all(same_bits(a["hist"][k], b["hist"][k]) for k in a["hist"]) and a["recs"] == b["recs"]
            and a["reuse"] == b["reuse"])


def same_run_result(a, b):
    keys = [k for k in a if k not in ("gap", "gap_stop")]
    return all(same_bits(a[k], b[k]) if k in ("fval", "kkt", "rr") else a[k] == b[k] for k in keys)


@functools.lru_cache(maxsize=None)
def three_runs(cls, m, n):
    """(plain, ruled, stepped): one run of NSTEP iterations without a rule, one with a record-only rule, and NSTEP
    single steps with bracket() after each -- each with what it left behind"""
    out = []
    ws, rng = started(cls, m, n)
    res = ws.run(amg(cls), rng, iters=NSTEP)
    out.append(dict(res=res, snap=snapshot(ws)))
    ws.close()
    ws, rng = started(cls, m, n, gap_tol=0.0)
    res = ws.run(amg(cls), rng, iters=NSTEP)
    out.append(dict(res=res, snap=snapshot(ws), gap=ws.gap_records(), gap_lam=ws.gap_lam(),
                    lam_dual=ws.dual(ws.gap_lam()[0], side=-1)))
    ws.close()
    ws, rng = started(cls, m, n)
    brackets = []
    for _ in range(NSTEP):
        res = ws.run(amg(cls), rng, iters=1)
        brackets.append(ws.bracket())
    out.append(dict(res=res, snap=snapshot(ws), brackets=brackets))
    ws.close()
    return tuple(out)


# ---------------------------------------------------------------------------
# 1. stepping, and a rule that only records
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cls,m,n", CASES)
def test_single_steps_are_one_run(cls, m, n):
    """the precondition of everything below (it holds without this feature): NSTEP run(iters=1) calls, with the
    read-only bracket() between them, leave the bits of one run(iters=NSTEP)"""
    plain, _, stepped = three_runs(cls, m, n)
    assert plain["res"]["k"] == NSTEP and not plain["res"]["converged"]
    assert same_snapshot(plain["snap"], stepped["snap"]) and same_run_result(plain["res"], stepped["res"])


@pytest.mark.parametrize("cls,m,n", CASES)
def test_a_record_only_rule_changes_nothing(cls, m, n):
    plain, ruled, _ = three_runs(cls, m, n)
    assert same_snapshot(plain["snap"], ruled["snap"]) and same_run_result(plain["res"], ruled["res"])
    assert "gap" not in plain["res"] and "gap_stop" not in plain["res"]
    assert ruled["res"]["gap_stop"] is False and ruled["res"]["gap"] == ruled["gap"][-1]


@pytest.mark.parametrize("cls,m,n", CASES)
def test_records_are_the_composed_loop(cls, m, n):
    """record k of the rule is bracket() after step k, bit for bit; best and gap follow the rule"""
    _, ruled, stepped = three_runs(cls, m, n)
    recs = ruled["gap"]
    assert [r["k"] for r in recs] == list(range(1, NSTEP + 1))
    best, best_k = -INF, None
    for rec, br in zip(recs, stepped["brackets"]):
        what = (cls, m, n, rec["k"])
        assert set(rec) == set(REC_KEYS)
        assert (rec["lower_side"], rec["upper_side"]) == (br["lower"]["side"], br["upper"]["side"]), what
        assert rec["upper_ok"] == br["upper"]["ok"] == 1 and rec["stop"] == 0 and rec["final"] == 0, what
        for key, want in (("lower", br["lower"]["dual"]), ("lower_dmin", br["lower"]["dmin"]),
                          ("upper", br["upper"]["fval"]), ("viol_in", br["upper"]["viol_in"])):
            assert same_bits(rec[key], want), (what, key, rec[key], want)
        if rec["lower"] > best:
            best, best_k = rec["lower"], rec["k"]
        assert same_bits(rec["best"], best) and same_bits(rec["gap"], rec["upper"] - best), what
        print("cls %d %dx%d k %d: lower %.12g best %.12g upper %.12g gap %.3e dmin %.3e"
              % (cls, m, n, rec["k"], rec["lower"], rec["best"], rec["upper"], rec["gap"], rec["lower_dmin"]))
    # the multiplier that attains best: evaluated as it is, it has that dual value and that smallest reduced cost
    lam, b = ruled["gap_lam"]
    assert same_bits(b, best) and same_bits(ruled["lam_dual"]["dual"], best)
    assert same_bits(ruled["lam_dual"]["dmin"], recs[best_k - 1]["lower_dmin"])


# ---------------------------------------------------------------------------
# 2. the stop, placed by the oracle
# ---------------------------------------------------------------------------
def certified_gap_of(cls, pr, m, n, u, lam):
    """(lower, upper, ok) of the oracle's state: the better c-transform's dual value in numpy (test_gpu_dual.py's
    restatement), the better rounding's cost (tests/round_ref.py)"""
    b = np.concatenate([pr["r"], pr["l"]] + ([[pr["mu"]]] if cls == 2 else []))
    duals = [-float(b @ TD.transform_ref(cls, pr, m, n, lam, side)[0]) for side in (0, 1)]
    lower = duals[1] if duals[1] > duals[0] else duals[0]
    rounds = [R.round_ref(cls, pr, m, n, u, 0.0, side) for side in (0, 1)]
    us = min((0, 1), key=lambda s: (not rounds[s]["ok"], rounds[s]["fval"]))
    return lower, float(rounds[us]["fval"]), int(rounds[us]["ok"])


@functools.lru_cache(maxsize=None)
def oracle_gaps(cls, m, n):
    """g_1 .. g_NSTEP of the CPU oracle (direct inner solver): upper - best lower so far after each iteration"""
    pr = problem(cls, m, n, seed=12)
    args = (pr["c"], pr["r"], pr["l"], pr["p"], pr["q"])
    if cls == 1:
        start = D.warmup_class1(*args, INF, 100)
        run = lambda K: D.apd_ssn_class1(*args, INF, inner="direct", maxit=K, start=start)
    else:
        start = D.warmup_class2(*args, pr["mu"], pr["phi"], 100)
        run = lambda K: D.apd_ssn_class2(*args, pr["mu"], pr["phi"], inner="direct", maxit=K, start=start)
    gaps, best = [], -INF
    for K in range(1, NSTEP + 1):
        ref = run(K)
        assert ref["k"] == K and not ref["converged"]
        u = ref["xk"] if cls == 1 else ref["uk"]
        lower, upper, ok = certified_gap_of(cls, pr, m, n, u, ref["lk"])
        assert ok == 1
        best = lower if lower > best else best
        gaps.append(upper - best)
    return tuple(gaps)


def stop_of(cls, m, n):
    """(K*, gap_tol): K* in 6..NSTEP with the largest g_{K*-1}/g_{K*}, the threshold their geometric mean"""
    g = (None,) + oracle_gaps(cls, m, n)
    K = max(range(6, NSTEP + 1), key=lambda k: g[k - 1] / g[k])
    tol = float(np.sqrt(g[K - 1] * g[K]))
    print("cls %d %dx%d: oracle gaps %s -> K* %d gap_tol %.4e, ratios %.3f %.3f"
          % (cls, m, n, " ".join("%.3e" % v for v in g[1:]), K, tol, g[K - 1] / tol, tol / g[K]))
    assert g[K - 1] / tol >= 1.3 and tol / g[K] >= 1.3
    assert all(g[k] / tol >= 1.3 for k in range(1, K))     # and no earlier gap is near the threshold either
    return K, tol


@pytest.mark.parametrize("cls,m,n", CASES)
def test_stops_where_the_oracle_says(cls, m, n):
    K, tol = stop_of(cls, m, n)
    pr = problem(cls, m, n, seed=12)
    fstar, _ = TR.optimum(cls, pr, m, n)
    slack = 1e-12 * abs(fstar)
    ws, rng = started(cls, m, n, gap_tol=tol)
    res = ws.run(amg(cls), rng)
    recs = ws.gap_records()
    for r in recs:
        print("cls %d %dx%d k %d: best %.12g f* %.12g upper %.12g gap %.3e stop %d"
              % (cls, m, n, r["k"], r["best"], fstar, r["upper"], r["gap"], r["stop"]))
    assert res["k"] == K and res["gap_stop"] is True and res["converged"] is False
    assert len(recs) == K and [r["stop"] for r in recs] == [0] * (K - 1) + [1] and res["gap"] == recs[-1]
    assert all(r["final"] == 0 for r in recs)
    last = recs[-1]
    assert last["gap"] <= tol and last["upper_ok"] == 1
    assert last["best"] <= fstar + slack and fstar <= last["upper"] + slack
    assert last["upper"] - fstar <= last["gap"] + slack
    # stopped: a further run does nothing
    snap = snapshot(ws)
    again = ws.run(amg(cls), rng)
    assert again["k"] == K and same_snapshot(snapshot(ws), snap) and len(ws.gap_records()) == K
    # a tighter rule continues: best and the records are kept, the stop is cleared
    ws.set_gap_rule(gap_tol=tol / 4)
    more = ws.run(amg(cls), rng)
    recs2 = ws.gap_records()
    assert more["k"] > K and more["gap_stop"] is True and len(recs2) == more["k"]
    assert [tuple(a[k] for k in REC_KEYS) for a in recs2[:K]] == [tuple(a[k] for k in REC_KEYS) for a in recs]
    assert recs2[-1]["stop"] == 1 and recs2[-1]["gap"] <= tol / 4 and recs2[-1]["best"] >= last["best"]
    assert all(b["best"] >= a["best"] for a, b in zip(recs2, recs2[1:]))
    assert recs2[-1]["best"] <= fstar + slack and fstar <= recs2[-1]["upper"] + slack
    # a restart of the script clears the stop, best and the records; the rule holds
    u, v, lam, bk = ws.state()
    ws.set_state(u, v, lam, bk)
    assert ws.gap_records() == [] and ws.gap_lam() == (None, -INF)
    one = ws.run(amg(cls), rng, iters=1)
    assert one["k"] == 1 and len(ws.gap_records()) == 1
    ws.close()


@pytest.mark.parametrize("cls,m,n", CASES)
def test_install_at_the_stop(cls, m, n):
    """install = 1: the state has the bits of a twin run stopped without install and then
    round_plan(side=upper_side, install=True); the installed plan meets test_gpu_round.py's test_install bounds"""
    K, tol = stop_of(cls, m, n)
    pr = problem(cls, m, n, seed=12)
    ws, rng = started(cls, m, n, gap_tol=tol, install=True)
    twin, rng2 = started(cls, m, n, gap_tol=tol)
    res, res2 = ws.run(amg(cls), rng), twin.run(amg(cls), rng2)
    assert res["k"] == res2["k"] == K and res["gap_stop"] and res2["gap_stop"]
    assert [tuple(a[k] for k in REC_KEYS) for a in ws.gap_records()] == \
        [tuple(a[k] for k in REC_KEYS) for a in twin.gap_records()]
    before = twin.state()
    twin.round_plan(0.0, side=res2["gap"]["upper_side"], install=True)
    a, b = snapshot(ws), snapshot(twin)
    assert same_snapshot(a, b) and not same_bits(a["u"], before[0])
    assert same_bits(a["lam"], before[2]) and a["bk"] == before[3]
    # feasibility of what was installed
    rb, cb = R.feasibility_bounds(pr, m, n)
    e = ws.end(a["lam"], from_w=False)
    bvec = np.concatenate([pr["r"], pr["l"]] + ([[pr["mu"]]] if cls == 2 else []))
    bound = np.concatenate([cb, rb] + ([[4 * R.gamma(m + n + 16) * pr["mu"]]] if cls == 2 else []))
    print("cls %d %dx%d: KKT_lk %.3e, bound %.3e" % (cls, m, n, e["kkt"][1], np.linalg.norm(bound)))
    assert bvec.size == bound.size and e["kkt"][1] <= np.linalg.norm(bound)
    _, _, ax = ws.plan(0.0, stats=True)
    cols, rows = ax[:n] - pr["r"], ax[n:] - pr["l"]
    if cls == 1:
        assert (np.abs(cols) <= cb).all() and (np.abs(rows) <= rb).all()
    else:
        assert (cols <= cb).all() and (rows <= rb).all()
    ws.close()
    twin.close()


# ---------------------------------------------------------------------------
# 3. the schedule, and the probe at CONV
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [1, 2])
def test_schedule(cls):
    ws, rng = started(cls, 24, 24, first=3, every=2)
    res = ws.run(amg(cls), rng, iters=8)
    recs = ws.gap_records()
    assert res["k"] == 8 and [r["k"] for r in recs] == [3, 5, 7] and not res["gap_stop"]
    assert res["gap"] == recs[-1] and all(r["stop"] == 0 and r["final"] == 0 for r in recs)
    # the same three states as the record-only rule at every iteration saw
    every = three_runs(cls, 24, 24)[1]["gap"]
    for r in recs:
        for key in ("lower", "lower_dmin", "upper", "viol_in", "lower_side", "upper_side"):
            assert same_bits(r[key], every[r["k"] - 1][key]), (r["k"], key)
    assert same_bits(recs[0]["best"], recs[0]["lower"])
    ws.close()


def test_final_probe_at_convergence():
    """a whole class-1 run, the schedule never due: one record, final = 1, at the result's k, bit-equal to bracket()"""
    ws, rng = started(1, 24, 24, every=1000, first=1000)
    res = ws.run(amg(1), rng)
    recs = ws.gap_records()
    assert res["converged"] and not res["gap_stop"] and len(recs) == 1
    rec = recs[0]
    assert rec["k"] == res["k"] and rec["final"] == 1 and rec["stop"] == 0 and res["gap"] == rec
    br = ws.bracket()
    assert (rec["lower_side"], rec["upper_side"], rec["upper_ok"]) == (br["lower"]["side"], br["upper"]["side"], 1)
    for key, want in (("lower", br["lower"]["dual"]), ("lower_dmin", br["lower"]["dmin"]),
                      ("best", br["lower"]["dual"]), ("upper", br["upper"]["fval"]),
                      ("viol_in", br["upper"]["viol_in"]), ("gap", br["gap"])):
        assert same_bits(rec[key], want), (key, rec[key], want)
    print("converged at k %d: certified gap %.3e" % (res["k"], rec["gap"]))
    # and the same run without a rule
    plain, rng2 = started(1, 24, 24)
    res2 = plain.run(amg(1), rng2)
    assert same_run_result(res2, res) and same_snapshot(snapshot(plain), snapshot(ws))
    ws.close()
    plain.close()


# ---------------------------------------------------------------------------
# 4. errors, and no rule
# ---------------------------------------------------------------------------
def test_setter_errors_keep_the_rule_in_force():
    L = lib_mod()
    ws, rng = started(1, 24, 24, first=2, every=3)
    good = dict(gap_tol=0.0, gap_rel=0.0, tol=0.0, first=1, every=1, install=False)
    for key, bad in (("gap_tol", -1e-300), ("gap_tol", np.nan), ("gap_tol", INF), ("gap_rel", -1.0),
                     ("gap_rel", np.nan), ("tol", -1.0), ("tol", np.nan), ("first", 0), ("first", -3), ("every", 0),
                     ("install", 2), ("install", -1)):
        with pytest.raises(L.IpdError) as ei:
            ws.set_gap_rule(**dict(good, **{key: bad}))
        assert ei.value.code == L.IPD_E_ARG, (key, bad)
    assert L.lib.ipd_apd_set_gap_rule(None, None) == L.IPD_E_ARG
    res = ws.run(amg(1), rng, iters=5)
    assert [r["k"] for r in ws.gap_records()] == [2, 5] and res["gap_stop"] is False      # the rule of the start
    # None: off.  The records stay, no probe follows, and run() drops its two keys
    ws.set_gap_rule(None)
    res = ws.run(amg(1), rng, iters=2)
    assert res["k"] == 7 and "gap" not in res and "gap_stop" not in res and len(ws.gap_records()) == 2
    ws.close()
    pr = problem(1, 24, 24, seed=12)
    for gama in (0.625, np.full(24 * 24, 0.7)):
        wg = ws_of(1, pr, gama=gama)
        with pytest.raises(L.IpdError) as ei:
            wg.set_gap_rule(gap_tol=1e-3)
        assert ei.value.code == L.IPD_E_UNSUPPORTED
        wg.set_gap_rule(None)
        wg.close()
    for key in ("p", "q"):
        for bad in (0.0, -1.0, INF, np.nan):
            pb = dict(pr)
            pb[key] = pr[key].copy()
            pb[key][5] = bad
            wb = ws_of(1, pb)
            with pytest.raises(L.IpdError) as ei:
                wb.set_gap_rule(gap_tol=1e-3)
            assert ei.value.code == L.IPD_E_ARG, (key, bad)
            wb.close()
    cnt = L.c_int64()
    assert L.lib.ipd_apd_gap_records(None, None, 0, L.byref(cnt)) == L.IPD_E_ARG
    assert L.lib.ipd_apd_gap_lam(None, None, None) == L.IPD_E_ARG


# ---------------------------------------------------------------------------
# 5. the drivers' keywords
# ---------------------------------------------------------------------------
def test_driver_keywords():
    m = n = 24
    K, tol = stop_of(1, m, n)
    pr = problem(1, m, n, seed=12)
    args = (pr["c"], pr["r"], pr["l"], pr["p"], pr["q"])
    plain = ipd().APD_SsN_Class1(*args, maxit=NSTEP)
    assert not {"gap_records", "gap_stop", "gap"} & set(plain)
    rec = ipd().APD_SsN_Class1(*args, maxit=NSTEP, gap_every=1)          # record only
    assert set(rec) - set(plain) == {"gap_records", "gap_stop", "gap"} and rec["gap_stop"] is False
    assert same_bits(rec["lk"], plain["lk"]) and same_bits(rec["xk"], plain["xk"])
    want = three_runs(1, m, n)[1]["gap"]
    assert rec["gap_records"] == want
    got = ipd().APD_SsN_Class1(*args, gap_tol=tol)
    assert got["k"] == K and got["gap_stop"] is True and got["converged"] is False
    assert got["gap_records"] == want[:K - 1] + [dict(want[K - 1], stop=1)] and got["gap"] == got["gap_records"][-1]
    sched = ipd().APD_SsN_Class1(*args, maxit=8, gap_first=3, gap_every=2)
    assert [r["k"] for r in sched["gap_records"]] == [3, 5, 7]
    inst = ipd().APD_SsN_Class1(*args, gap_tol=tol, gap_install=True)
    assert inst["k"] == K and same_bits(inst["lk"], got["lk"]) and not same_bits(inst["xk"], got["xk"])
    # thr = gap_rel*|upper|: the upper bounds of these iterations differ by a few per cent, the margin is 30
    rel = ipd().APD_SsN_Class1(*args, gap_rel=tol / abs(got["gap"]["upper"]))
    assert rel["gap_stop"] is True and rel["k"] == K
    # class 2
    K2, tol2 = stop_of(2, m, n)
    pr2 = problem(2, m, n, seed=12)
    two = ipd().APD_SsN_Class2(pr2["c"], pr2["r"], pr2["l"], pr2["p"], pr2["q"], pr2["mu"], pr2["phi"], gap_tol=tol2)
    assert two["k"] == K2 and two["gap_stop"] is True and len(two["gap_records"]) == K2
    # from points: stored and matrix-free give the same records
    rs = np.random.RandomState(15)
    xs, ys = rs.random_sample((m, 2)), rs.random_sample((n, 2))
    mu = 0.65 * min(pr["r"].sum(), pr["l"].sum())
    for cls in (1, 2):
        outs = []
        for free in (False, True):
            if cls == 1:
                out = ipd().APD_SsN_Class1_points(xs, ys, pr["r"], pr["l"], pr["p"], pr["q"], maxit=4,
                                                  matrix_free=free, gap_every=1)
            else:
                out = ipd().APD_SsN_Class2_points(xs, ys, pr["r"], pr["l"], pr["p"], pr["q"], mu, maxit=4,
                                                  matrix_free=free, gap_every=1)
            outs.append(out)
            assert [r["k"] for r in out["gap_records"]] == [1, 2, 3, 4] and out["gap_stop"] is False
        assert outs[0]["gap_records"] == outs[1]["gap_records"]
