"""The launch planner of the multi-launch path (csrc/ipd_launch_plan.h) on the CPU: a small C++ driver
(tests/launch_plan_driver.cpp) is built with the system g++ against the header and run on synthetic
hierarchies; every record keeps the invariants of the rules, the printed plans are the pinned ones, and each
rule's decision flips at its threshold and nowhere else.  CPU only."""
import hashlib
import os
import re
import subprocess

import pytest

from tests.test_level_plan import SHAPES, Lcg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "codes_of_ipd_ssn_amg_method_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
LIMITS = open(os.path.join(CSRC, "ipd_limits.h")).read()


def _const(name):
    return int(re.search(r"static constexpr int %s = (\d+);" % name, LIMITS).group(1))


BT = _const("BT")
STAGE_MAX = _const("STAGE_MAX")
ROW_U = _const("ROW_U")
QUEUED_NNZ_MAX = 6000        # the measured thresholds, as the issue states them
RRC_T1_NNZ_MAX = 2 ** 18
SWITCHES = ["-", "IPD_NO_PAD", "IPD_NO_STAGE", "IPD_NO_RRC", "IPD_NO_PAD,IPD_NO_STAGE,IPD_NO_RRC"]


def level(nr, nnz, nf=0, maxoff=0, pt=(0, 0, 0), p=(0, 0, 0), t1=(0, 0, 0)):
    """One level as the driver reads it: A_k, F-block size, longest off-diagonal row, then P'_{k+1}
    (rows, columns, entries), P_{k+1} and T1 = P'A (present, rows, entries)."""
    return (nr, nnz, nf, maxoff) + tuple(pt) + tuple(p) + tuple(t1)


def with_transfers(levels, t1=True):
    """A test_level_plan hierarchy (nr, nnz, nf, maxoff, p_nnz per level) with the transfer sizes that go
    with it: P_{k+1} is N_k x N_{k+1}, T1 has a row per coarse row and about p_nnz * (entries per row of A_k)
    entries."""
    out = []
    for k, (nr, nnz, nf, maxoff, _) in enumerate(levels):
        if k + 1 == len(levels):
            out.append(level(nr, nnz, nf, maxoff))
            continue
        nc, pn = levels[k + 1][0], levels[k + 1][4]
        t1n = min(nc * nr, pn * max(1, nnz // max(nr, 1)))
        out.append(level(nr, nnz, nf, maxoff, (nc, nr, pn), (nr, nc, pn), (1 if t1 else 0, nc, t1n)))
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_driver")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC,
                          os.path.join(HERE, "launch_plan_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def case_line(case):
    levels, cu, sw, donor = case
    return " ".join([str(len(levels)), str(cu), sw, str(len(donor))] + [str(v) for w in donor for v in w] +
                    [str(v) for lv in levels for v in lv])


def parse(line):
    """A record line as an ordered dict: the fields behind rrc_rule / rest / prol / pcg carry that prefix,
    a sweep's ranges are a list of (r0, r1, G)."""
    rec, prefix = {}, ""
    for tok in line.split()[2:]:
        m = re.fullmatch(r"\[(\d+),(\d+)\)x(\d+)", tok)
        if m:
            rec[prefix].append(tuple(int(v) for v in m.groups()))
        elif tok in ("pre", "post"):
            prefix = tok
            rec[tok] = []
        elif tok in ("pcg", "rrc"):
            prefix = tok + "."
            rec[tok] = 1
        else:
            key, val = tok.split("=")
            if key in ("rrc_rule", "rest", "prol"):
                prefix = key.split("_")[0] + "."
                key = key if key == "rrc_rule" else key + ".how"
            elif key in ("L", "G", "staged") and prefix.endswith("."):
                key = prefix + key
            else:
                prefix = ""
            rec[key] = int(val) if val.isdigit() else val
    return rec


def run_plans(driver, cases, raw=None):
    res = subprocess.run([driver], input="\n".join(case_line(c) for c in cases) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    assert lines[0].split() == ["limits"] + [str(v) for v in (BT, STAGE_MAX, ROW_U, QUEUED_NNZ_MAX, RRC_T1_NNZ_MAX)]
    plans, cur = [], []
    for ln in lines[1:]:
        if raw is not None:
            raw.append(ln)
        if ln == "end":
            plans.append(cur)
            cur = []
        else:
            assert ln.startswith("level %d " % (len(cur) + 1)), ln
            cur.append(parse(ln))
    assert len(plans) == len(cases) and all(len(p) == len(c[0]) for p, c in zip(plans, cases))
    return plans


DONOR = [(0, 8, 16, 8), (12, 4, 4, 8)]   # levels 1 and 2 of a donor: S, L, G, lanes (level 1 without a padded copy)


def shape_cases():
    out = []
    for name in SHAPES:
        for cu in (256, 8):
            for sw in SWITCHES:
                out.append((with_transfers(SHAPES[name]), cu, sw, []))
        jac = [(nr, nnz, 0, mo, pn) for nr, nnz, _, mo, pn in SHAPES[name]]   # nf = 0 at level 1
        out.append((with_transfers(jac), 256, "-", []))
        out.append((with_transfers(SHAPES[name], t1=False), 256, "-", []))
        out.append((with_transfers(SHAPES[name]), 256, "-", DONOR))
        out.append((with_transfers(SHAPES[name]), 256, "IPD_NO_PAD", DONOR[:1]))
    return out


SWEEP_SEED, SWEEP_COUNT = 20261017, 3000


def sweep_cases(seed=SWEEP_SEED, count=SWEEP_COUNT):
    """Synthetic hierarchies from a generator of this file's own: rows shrink by 20-60 % per level, 3-60
    entries per row (a fifth of the levels dense-ish), transfers with 1-6 or 64 entries per fine row, T1 mostly
    present, its size on either side of the fused rule's bound."""
    g, out = Lcg(seed), []
    for _ in range(count):
        rows = [20 + g.below(9000)]
        while len(rows) < 8:
            nxt = max(1, rows[-1] * (20 + g.below(41)) // 100)
            rows.append(nxt)
            if nxt <= 12 and g.below(2):
                break
        nf = 0 if g.below(3) == 0 else 1 + g.below(rows[0] - 1)
        levels = []
        for k, n in enumerate(rows):
            per = 3 + g.below(58) if g.below(5) else 64 + g.below(2000)
            nnz = min(n * per, n * n)
            maxoff = max(0, min(n - 1, per + g.below(per + 1)))
            if k + 1 == len(rows):
                levels.append(level(n, nnz, nf if k == 0 else 0, maxoff))
                continue
            nc = rows[k + 1]
            pn = min(n * (64 if g.below(8) == 0 else 1 + g.below(6)), n * nc)
            t1n = [min(nc * n, pn * per), RRC_T1_NNZ_MAX - 1 + g.below(3)][g.below(6) == 0]
            t1 = (1 if g.below(10) else 0, nc if g.below(20) else nc + 1, t1n)
            levels.append(level(n, nnz, nf if k == 0 else 0, maxoff, (nc, n, pn), (n, nc, pn), t1))
        cu = (256, 256, 64, 8, 1)[g.below(5)]
        sw = SWITCHES[g.below(len(SWITCHES))] if g.below(3) == 0 else "-"
        donor = DONOR[:1 + g.below(2)] if g.below(10) == 0 else []
        out.append((levels, cu, sw, donor))
    return out


def pow2(v):
    return v >= 1 and v & (v - 1) == 0


def small(rows, L, nnz_est, stage_len):
    return stage_len <= STAGE_MAX and rows * L <= BT and nnz_est <= QUEUED_NNZ_MAX


def check_plan(where, case, plan):
    levels, cu, sw, donor = case
    sws, J = sw.split(","), len(levels)
    for k, (lv, p) in enumerate(zip(levels, plan), start=1):
        nr, nnz, nf, _, pt_nr, pt_nc, pt_nnz, p_nr, p_nc, p_nnz, t1, t1_nr, t1_nnz = lv
        w = (where, k, p)
        given = k <= len(donor)   # the walk is the donor's, as handed in
        assert (p["N"], p["nf"]) == (nr, nf), w
        # lanes are powers of two <= BT, grids lie in [1, cu]
        for key in ("lanes", "L", "rest.L", "prol.L", "rrc.L", "pcg.L"):
            assert key not in p or (pow2(p[key]) and p[key] <= BT), (w, key)
        grids = [p["G_all"]] + [r[2] for r in p["pre"] + p["post"]] + [p[q] for q in ("rest.G", "prol.G", "rrc.G") if q in p]
        assert all(1 <= g <= cu for g in grids + ([] if given else [p["G"]])), w
        # S is a multiple of 4, and zero under IPD_NO_PAD; staging only of what fits, none of the level's under IPD_NO_STAGE
        assert p["S"] % 4 == 0 and (given or "IPD_NO_PAD" not in sws or p["S"] == 0), w
        if given:
            assert (p["S"], p["L"], p["G"], p["lanes"]) == donor[k - 1], w
        assert p["staged"] == int(nr <= STAGE_MAX and "IPD_NO_STAGE" not in sws), w
        # the two half ranges partition [0, N), and post is pre reversed
        pre, post = [r[:2] for r in p["pre"]], [r[:2] for r in p["post"]]
        assert pre == ([(0, nf), (nf, nr)] if nf else [(0, nr)]) and post == pre[::-1], w
        assert sorted(r[2] for r in p["pre"]) == sorted(r[2] for r in p["post"]), w
        # a queued phase covers its rows in one pass, stages its vector and has few entries -- and only such a one is queued
        rows = max(nf, nr - nf) if nf else nr
        assert (p["sweep"] == "queued") == bool(p["staged"] and small(rows, p["L"], nnz * rows / max(nr, 1), nr)), w
        if k == 1:
            assert (p["top"] == "queued") == bool(p["staged"] and small(nr, p["L"], nnz, nr)), w
        if k == J:
            assert p["pcg.L"] <= 64 and "rest.how" not in p, w
            continue
        resid_q = bool(p["staged"] and small(nr, p["L"], nnz, nr))
        for key, (xr, xc, xn) in (("rest", (pt_nr, pt_nc, pt_nnz)), ("prol", (p_nr, p_nc, p_nnz))):
            assert p[key + ".staged"] == int(xc <= STAGE_MAX), (w, key)
            assert (p[key + ".how"] == "queued") == bool(p[key + ".staged"] and small(xr, p[key + ".L"], xn, xc)), (w, key)
        # k_rrc is chosen only where its rule holds and neither part is queued
        rule = "IPD_NO_RRC" not in sws and t1 == 1 and t1_nr == pt_nr and t1_nnz <= RRC_T1_NNZ_MAX
        assert p["rrc_rule"] == int(rule), w
        assert ("rrc" in p) == (rule and not resid_q and p["rest.how"] != "queued"), w
        if "rrc" not in p:
            assert (p["resid"] == "queued") == resid_q, w
        if rule:
            assert p["rrc.staged"] == int(2 * pt_nc <= STAGE_MAX and p["staged"]), w


def test_every_record_keeps_the_invariants(driver):
    cases = shape_cases() + sweep_cases()
    plans = run_plans(driver, cases)
    seen = dict(queued=0, rrc=0, padded=0, two_halves=0)
    for i, (case, plan) in enumerate(zip(cases, plans)):
        check_plan(i, case, plan)
        for p in plan:
            seen["queued"] += p["sweep"] == "queued"
            seen["rrc"] += "rrc" in p
            seen["padded"] += p["S"] > 0
            seen["two_halves"] += len(p["pre"]) == 2
    assert min(seen.values()) > 500, seen


def _sha256(lines):
    return hashlib.sha256("".join(ln + "\n" for ln in lines).encode()).hexdigest()


def test_plans_are_the_pinned_ones(driver):
    """plan_launches decides what the launch code decided while it enqueued: SHA-256 of the driver's output on
    the shapes' cases and on the sweep.  The pinned values were computed by a separate program from the
    functions of the commit before -- pick_lanes, pick_blocks, phase_is_small, the body of build_padded and
    the conditions of prepare_level_runs, prepare_transfers, launch_sweep, amg_cycle, launch_top and
    amg_block_levels, copied unchanged -- on these same case lines."""
    cases = shape_cases()
    assert len(cases) == 140
    raw = []
    run_plans(driver, cases, raw)
    assert _sha256(raw) == "d294528daa6fda7791f91868aec3e4bba54800ea53debb836d88fe8da2ae73fc"
    raw = []
    run_plans(driver, sweep_cases(), raw)
    assert len(raw) == 25264
    assert _sha256(raw) == "5e5cf6311689baf75d97141e35cad36c9f0cc3592b2edc6cccf6ee9b18a7abfc"


def changed(driver, a, b, cu=1, sw="-"):
    """The fields of level 1's record that differ between the two-level hierarchies with level 1 `a` and `b`."""
    tail = level(4, 16)
    (pa, _), (pb, _) = run_plans(driver, [([a, tail], cu, sw, []), ([b, tail], cu, sw, [])])
    assert pa.keys() | pb.keys() >= {"N", "rest.how", "prol.how"}
    return {k: (pa.get(k), pb.get(k)) for k in list(pa) + list(pb) if pa.get(k) != pb.get(k)}


BIG = (4000, 400000)   # rows and entries of a level that no rule queues


def test_queued_phase_bound_on_entries(driver):
    """One entry over 6000: a restriction of 63 rows of 8 lanes (504 threads) leaves the fused program; the same
    on a Jacobi level's matrix moves its sweep, its residual and the top together."""
    rest = lambda n: level(*BIG, pt=(63, 4000, n), p=(4000, 63, 8000))
    assert changed(driver, rest(6000), rest(6001)) == {"rest.how": ("queued", "launched")}
    lv = lambda n: level(63, n, pt=(4, 63, 60000), p=(63, 4, 60000))
    assert changed(driver, lv(6000), lv(6001), sw="IPD_NO_PAD") == {
        "sweep": ("queued", "launched"), "top": ("queued", "launched"), "resid": ("queued", "launched")}


def test_queued_phase_bound_on_threads(driver):
    """rows * L one lane group over BT: 64 rows of 8 lanes (512) against 65."""
    prol = lambda r: level(*BIG, pt=(50, 4000, 60000), p=(r, 50, 5900))
    assert changed(driver, prol(64), prol(65)) == {"prol.how": ("queued", "launched")}


def test_staging_bounds(driver):
    """A vector of STAGE_MAX entries is staged, one more is not: the level's own, a transfer's, and k_rrc's
    two vectors of half that length each."""
    lv = lambda n: level(n, 400000, pt=(50, 4000, 60000), p=(4000, 50, 60000))
    assert changed(driver, lv(STAGE_MAX), lv(STAGE_MAX + 1), sw="IPD_NO_PAD") == {
        "N": (STAGE_MAX, STAGE_MAX + 1), "staged": (1, 0), "pre": ([(0, STAGE_MAX, 1)], [(0, STAGE_MAX + 1, 1)]),
        "post": ([(0, STAGE_MAX, 1)], [(0, STAGE_MAX + 1, 1)])}
    rest = lambda nc: level(*BIG, pt=(50, nc, 60000), p=(4000, 50, 60000))
    assert changed(driver, rest(STAGE_MAX), rest(STAGE_MAX + 1)) == {"rest.staged": (1, 0)}
    rrc = lambda nc: level(*BIG, pt=(50, nc, 60000), p=(4000, 50, 60000), t1=(1, 50, 70000))
    assert changed(driver, rrc(STAGE_MAX // 2), rrc(STAGE_MAX // 2 + 1)) == {"rrc.staged": (1, 0)}


def test_fused_residual_restriction_bound(driver):
    """T1 of 2^18 entries runs fused with the restriction, one more keeps the two launches -- and so does a T1
    whose rows are not the restriction's, an absent one, and IPD_NO_RRC."""
    lv = lambda t1: level(*BIG, pt=(50, 3000, 60000), p=(4000, 50, 60000), t1=t1)
    on = (1, 50, RRC_T1_NNZ_MAX)
    for off in ((1, 50, RRC_T1_NNZ_MAX + 1), (1, 51, RRC_T1_NNZ_MAX), (0, 50, RRC_T1_NNZ_MAX)):
        d = changed(driver, lv(on), lv(off))
        assert set(d) == {"rrc", "resid", "rrc_rule", "rrc.L", "rrc.staged"}, d
        assert d["rrc"] == (1, None) and d["resid"] == (None, "launched") and d["rrc_rule"] == (1, 0), d
    (p,), (q,) = [pl[:1] for pl in run_plans(driver, [([lv(on), level(4, 16)], 1, sw, []) for sw in ("-", "IPD_NO_RRC")])]
    assert "rrc" in p and p["rrc_rule"] == 1 and "rrc" not in q and q["rrc_rule"] == 0


def test_fused_pair_gives_way_to_a_queued_part(driver):
    """Where the restriction is queued the rule still holds (the block solve's flag) but k_rrc is not chosen."""
    lv = lambda n: level(*BIG, pt=(63, 4000, n), p=(4000, 63, 8000), t1=(1, 63, 9000))
    d = changed(driver, lv(6000), lv(6001))
    assert d == {"rest.how": ("queued", "launched"), "resid": ("launched", None), "rrc": (None, 1)}, d


def test_pad_rule_bounds(driver):
    """S = maxoff rounded up to 4 is taken up to 1.3 * mean + 16 (mean 20: 42), from a mean off-diagonal
    length of 0.5, for at most 65535 rows; the fields that move with it are the walk's own."""
    walk = {"S", "L", "G", "G_all", "pre", "post"}
    lv = lambda nr, nnz, mo: level(nr, nnz, maxoff=mo, pt=(50, nr, 60000), p=(nr, 50, 60000))
    for a, b, S in ((lv(1000, 21000, 40), lv(1000, 21000, 41), 40), (lv(1000, 1500, 4), lv(1000, 1499, 4), 4)):
        d = changed(driver, a, b, cu=256)
        assert d["S"] == (S, 0) and set(d) <= walk, d
    d = changed(driver, lv(65535, 655350, 12), lv(65536, 655360, 12), cu=256)
    assert d["S"] == (12, 0) and set(d) <= walk | {"N", "staged"}, d
    assert changed(driver, lv(1000, 21000, 40), lv(1000, 21000, 37), cu=256) == {}   # the same 4-entry vectors


def test_lane_rules(driver):
    """pick_lanes aims at 3 * ROW_U entries per lane from a mean row of 64 entries and at ROW_U / 2 below;
    padded_lanes gives a lane at most 8 batches (32 vectors of 4: S = 128) before it widens."""
    rest = lambda n: level(*BIG, pt=(1000, 4000, n), p=(4000, 50, 60000))
    assert changed(driver, rest(64000), rest(63999)) == {"rest.L": (8, 32)}
    lv = lambda mo: level(1000, 101000, maxoff=mo, pt=(50, 1000, 60000), p=(1000, 50, 60000))
    assert changed(driver, lv(128), lv(129)) == {"S": (128, 132), "L": (4, 8)}
