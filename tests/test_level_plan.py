"""The level planner of the single-workgroup kernels (csrc/ipd_level_plan.h) on the CPU: a small C++
driver (tests/level_plan_driver.cpp) is built with the system g++ against the header and run on
synthetic hierarchies; every image it plans must keep the planner's invariants, every plan is the pinned
one, and every image's layout (image_layout: what pack_image binds to the descriptor) keeps the layout's
invariants and accounts for the planner's prediction.  CPU only."""
import hashlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "codes_of_ipd_ssn_amg_method_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))


def _const(name):
    src = open(os.path.join(CSRC, "ipd_limits.h")).read()
    return int(re.search(r"static constexpr int %s = (\d+);" % name, src).group(1))


def _size_const(name):
    src = open(os.path.join(CSRC, "ipd_limits.h")).read()
    a, b = re.search(r"static constexpr size_t %s = \(size_t\)(\d+) \* (\d+);" % name, src).groups()
    return int(a) * int(b)


BT = _const("BT")
RELOC_MAX = _const("RELOC_MAX")
LDS_BUDGET = _size_const("IMAGE_LDS_BUDGET")
LDS_OPTIN = _size_const("IMAGE_LDS_OPTIN")
SOL_HEAD = int(re.search(r"static constexpr size_t SOL_HEAD = (\d+);",
                         open(os.path.join(CSRC, "ipd_limits.h")).read()).group(1))


def lv(nr, nnz, nf=0, maxoff=None, p_nnz=0):
    """One level: rows, entries, F-block size, longest off-diagonal row, entries of P_k."""
    if maxoff is None:
        maxoff = max(0, min(nr - 1, 2 * nnz // max(nr, 1)))
    return (nr, nnz, nf, maxoff, p_nnz)


def chain(rows, per_row, nf1, p_per_row=2):
    """A Newton-like hierarchy: level 1 bigraph (nf1 F rows), entries per row per level, P_k with
    p_per_row entries per fine row."""
    out = []
    for k, (n, r) in enumerate(zip(rows, per_row)):
        p = 0 if k == 0 else min(rows[k - 1] * p_per_row, rows[k - 1] * n)
        out.append(lv(n, min(n * r, n * n), nf1 if k == 0 else 0, None, p))
    return out


SHAPES = {
    # a 576-row level 3 over a 175-row level 4, level 1 above RES_NMAX
    # (m=n=2000), in block-wide polynomial form
    "design4_576_over_175": [lv(4000, 48000, 2000, 40), lv(2000, 40000, 0, 60, 8000), lv(576, 2304, 0, 6, 8000),
                             lv(175, 7000, 0, 80, 576), lv(16, 256, 0, 15, 175), lv(4, 16, 0, 3, 16)],
    # bench.py's default hierarchy: m=n=1024, regime-D mask, three levels with a one-row tail
    "bench_1024": [lv(2048, 2099200, 1024, 1024), lv(1024, 1048576, 0, 1023, 1024 * 1024 + 1024),
                   lv(1, 1, 0, 0, 1024)],
    "newton_5": chain([2048, 1024, 300, 60, 12], [10, 14, 9, 12, 10], 1024),
    "newton_6": chain([2048, 1024, 420, 120, 30, 6], [8, 16, 10, 20, 12, 6], 1024),
    "newton_6_dense4": chain([2048, 1024, 200, 90, 40, 8], [8, 16, 30, 60, 30, 8], 1024),
    "newton_7": chain([4096, 2048, 700, 200, 60, 20, 4], [8, 16, 12, 30, 20, 10, 4], 2048),
    "newton_7_small": chain([1000, 500, 200, 80, 30, 10, 3], [6, 8, 8, 10, 10, 8, 3], 500),
    "small_4": chain([600, 300, 60, 8], [6, 8, 10, 8], 300),
    "tiny_3": chain([100, 40, 6], [5, 8, 6], 50),
}
PINNED_SHAPES = list(SHAPES)   # the shapes of the pinned plans (test_plans_are_the_pinned_ones)
# no sub-cycle because P_3 is big (a dense 1024 x 50 block), levels 3..J small: an image rooted at level 3 for the
# resident kernels' tail alone (plan_tails, b3)
SHAPES["sub3_dense_p3"] = [lv(2048, 20480, 1024, 12), lv(1024, 16384, 0, 40, 4096), lv(50, 1500, 0, 40, 51200),
                           lv(5, 25, 0, 4, 100)]
OPTS = [("v", 1), ("w", 1), ("w", 3), ("v", 0)]
SWITCHES = ["-", "IPD_NO_SMALL", "IPD_NO_SUBCYCLE", "IPD_NO_BLK", "IPD_NO_POLY", "IPD_NO_BPOLY",
            "IPD_NO_BLKDENSE", "IPD_NO_RESIDENT", "IPD_NO_RESIDENT_THREE", "IPD_NO_RES_POLY4",
            "IPD_NO_SMALL,IPD_NO_SUBCYCLE"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("level_plan") / "level_plan_driver")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC,
                          os.path.join(HERE, "level_plan_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def run_plans(driver, cases, raw=None):
    """The driver's plans of `cases`; raw (a list) receives its plan / image / end lines as printed."""
    lines = []
    for levels, cycle, smoth, sw in cases:
        lines.append(" ".join([str(len(levels)), cycle, str(smoth), "0", "0", sw] +
                              [str(v) for level in levels for v in level]))
    res = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    plans, cur, im = [], None, None
    for ln in res.stdout.splitlines():
        f = ln.split()
        if f[0] in ("plan", "image", "end") and raw is not None:
            raw.append(ln)
        if f[0] == "plan":
            cur = {"small_ok": int(f[1]), "k_sub": int(f[2]), "semi_root": int(f[3]), "sub5": f[4], "images": []}
        elif f[0] == "image":
            im = dict(role=f[1], k_lds=int(f[2]), k_semi=int(f[3]), k_tiny=int(f[4]), k_blk=int(f[5]), stage=int(f[6]),
                      lds=int(f[7]), tpr_rows=int(f[8]), levels={}, pieces=[], layout=None)
            cur["images"].append(im)
        elif f[0] == "level":
            im["levels"][int(f[1])] = (f[2], int(f[3]))   # form, rows
        elif f[0] == "piece":
            im["pieces"].append(dict(level=int(f[1]), slot=f[2], kind=f[3], bytes=int(f[4]), off=int(f[5])))
        elif f[0] == "layout":
            im["layout"] = dict(image_bytes=int(f[1]), total=int(f[2]), relocs=int(f[3]), k_cached=int(f[4]),
                                reserves=dict(zip(RESERVES, map(int, f[5:]))))
        elif f[0] == "end":
            plans.append(cur)
        else:
            assert f[0] == "limits" and [int(v) for v in f[1:]] == [LDS_BUDGET, LDS_OPTIN, RELOC_MAX, SOL_HEAD, BT], ln
    assert len(plans) == len(cases)
    return plans


# the named terms of image_reserves (ipd_level_plan.h), in the order of the driver's layout line
RESERVES = ["head", "xx", "bp_part", "child_pad", "coarsest_lmap", "const_pad", "above_root"]


class Lcg:
    def __init__(self, seed):
        self.x = seed & (2 ** 64 - 1)

    def below(self, n):          # uniform integer in [0, n)
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (self.x >> 33) % n


def sweep_cases(seed=20261016, count=4000):
    """Synthetic hierarchies from a generator of this file's own (no library generator can move them)."""
    g, out = Lcg(seed), []
    for _ in range(count):
        n1 = 200 + g.below(3897)                      # 200..4096 rows on level 1
        rows = [n1]
        while len(rows) < 8:
            nxt = max(1, rows[-1] * (20 + g.below(41)) // 100)
            rows.append(nxt)
            if nxt <= 12 and g.below(2):
                break
        if len(rows) < 3:
            rows.append(1)
        levels = []
        for k, n in enumerate(rows):
            per = 3 + g.below(58)
            nnz = min(n * per, n * n)
            maxoff = max(0, min(n - 1, per + g.below(per + 1)))
            fan = 64 if g.below(8) == 0 else 1 + g.below(6)
            p = 0 if k == 0 else min(rows[k - 1] * fan, rows[k - 1] * n)
            levels.append((n, nnz, n1 // 2 if k == 0 else 0, maxoff, p))
        cycle = "vw"[g.below(2)]
        smoth = g.below(4)
        sw = SWITCHES[g.below(len(SWITCHES))] if g.below(3) == 0 else "-"
        out.append((levels, cycle, smoth, sw))
    return out


ALL_CASES = [(name, cycle, smoth, sw) for name in SHAPES for cycle, smoth in OPTS for sw in SWITCHES]
PINNED_CASES = [c for c in ALL_CASES if c[0] in PINNED_SHAPES]


def _sha256(lines):
    return hashlib.sha256("".join(ln + "\n" for ln in lines).encode()).hexdigest()


def test_plans_are_the_pinned_ones(driver):
    """plan_levels returns what it returned before its byte counts were restated as sums of the layout's
    pieces: SHA-256 of the plan / image / end lines (SOL_HEAD 12592) of the pinned shapes' cases and of the
    sweep, computed with the header and driver of the commit before."""
    assert SOL_HEAD == 12592 and len(PINNED_CASES) == 396
    raw = []
    run_plans(driver, [(SHAPES[n], c, s, sw) for n, c, s, sw in PINNED_CASES], raw)
    assert _sha256(raw) == "718a9a7f06a3161d368767e115c5a86eee19954926ee2d2f5f8198c7e5b59c3d"
    raw = []
    plans = run_plans(driver, sweep_cases(), raw)
    assert len(raw) == 12177
    assert _sha256(raw) == "2d597ee4f902adc28998f2e98c1a34a48e09d3d42102f09d9516de9f686c69c2"
    roles = [im["role"] for p in plans for im in p["images"]]
    assert [roles.count(r) for r in ("solve", "sub", "sub3", "sub4")] == [664, 3122, 0, 391]


def test_the_image_for_the_resident_tail_alone(driver):
    raw = []
    (p,) = run_plans(driver, [(SHAPES["sub3_dense_p3"], "w", 1, "-")], raw)
    assert raw == ["plan 0 0 0 none 1 4", "image sub3 3 0 4 3 16 23888 0", "end"]
    assert p["images"][0]["layout"]["total"] == 23248


def r16(b):
    return (b + 15) // 16 * 16


def bdense_pad(n):   # ipd_limits.h
    g = 4 * (4 if n > 64 else 8)
    return (n + g - 1) // g * g


def check_layout(where, J, im):
    """The invariants of one image's layout, and the account of its prediction."""
    lay, stage = im["layout"], im["stage"]
    pieces = im["pieces"]
    real = [q for q in pieces if q["kind"] != "alias"]
    assert real and real[0]["off"] >= stage + SOL_HEAD, where
    end = 0
    for q in real:   # multiples of 16, strictly increasing in list order, no overlap
        assert q["off"] % 16 == 0 and q["off"] >= end and q["bytes"] > 0, (where, q)
        end = q["off"] + r16(q["bytes"])
        if q["kind"] == "work":
            assert q["off"] >= stage + lay["image_bytes"], (where, q)
        else:
            assert q["off"] + q["bytes"] <= stage + lay["image_bytes"], (where, q)
    assert end == lay["total"] and lay["image_bytes"] % 16 == 0, where
    offs = {q["off"] for q in real}
    assert all(q["off"] in offs for q in pieces if q["kind"] == "alias"), where
    for i, q in enumerate(pieces):   # pMr, pMe, pMc: one behind the other
        if q["slot"] == "pMr":
            a, b = pieces[i + 1], pieces[i + 2]
            assert (a["slot"], b["slot"], a["level"], b["level"]) == ("pMe", "pMc", q["level"], q["level"]), (where, q)
            assert a["off"] == q["off"] + r16(q["bytes"]) and b["off"] == a["off"] + r16(a["bytes"]), (where, q)
    polynomial = ("poly", "lpoly", "bpoly")
    for q in real:   # padding of the work vectors
        if q["slot"] not in ("r", "e", "e2", "rr", "w"):
            continue
        form, rows = im["levels"][q["level"]]
        parent = im["levels"].get(q["level"] - 1, ("none", 0))[0]
        assert q["bytes"] >= 8 * rows, (where, q)
        if form == "bdense":
            assert q["bytes"] == 8 * bdense_pad(rows), (where, q)
        elif form in ("tiny",) + polynomial or parent in polynomial:
            assert q["bytes"] % 64 == 0, (where, q)
    assert set(im["levels"]) == set(range(im["k_lds"], J + 1)), where
    assert lay["relocs"] == len(pieces) <= RELOC_MAX, where
    assert lay["total"] <= im["lds"] <= LDS_BUDGET and lay["total"] <= LDS_OPTIN, (where, im["lds"], lay)
    # the prediction is the layout plus the named reserves; where plan_lds itself returned the image's first
    # level (every solve image, a sub image without semi-cached root that caches nothing above its root) none
    # of them is for levels outside the image
    res = lay["reserves"]
    assert im["lds"] - lay["total"] == sum(res.values()), (where, im["lds"], lay)
    if lay["k_cached"] == im["k_lds"]:
        assert res["above_root"] == 0, (where, lay)
    return lay["k_cached"] == im["k_lds"] and not im["k_semi"]


def test_every_layout_keeps_the_invariants_and_accounts_for_the_prediction(driver):
    cases = [(SHAPES[n], c, s, sw) for n, c, s, sw in ALL_CASES]
    names = ["%s %s smoth=%d %s" % c for c in ALL_CASES]
    sweep = sweep_cases()
    cases += sweep
    names += ["sweep %d" % i for i in range(len(sweep))]
    laid_out = no_layout = exact_root = 0
    by_role = dict(solve=0, sub=0, sub3=0, sub4=0)
    plans = run_plans(driver, cases)
    for where, case, p in zip(names, cases, plans):
        J = len(case[0])
        for im in p["images"]:
            if im["layout"] is None:   # a solve with nothing cached: the descriptor alone
                assert im["role"] == "solve" and im["k_lds"] > J and not im["pieces"], (where, im)
                no_layout += 1
                continue
            laid_out += 1
            by_role[im["role"]] += 1
            exact_root += check_layout((where, im["role"]), J, im)
    assert no_layout + laid_out == sum(len(p["images"]) for p in plans)
    assert laid_out >= 339 + 4177 and by_role["sub3"] > 0 and exact_root > 1000, (laid_out, no_layout, by_role, exact_root)




def test_every_planned_image_keeps_the_invariants(driver):
    plans = run_plans(driver, [(SHAPES[n], c, s, sw) for n, c, s, sw in ALL_CASES])
    planned = 0
    for (name, cycle, smoth, sw), p in zip(ALL_CASES, plans):
        J = len(SHAPES[name])
        where = "%s %s smoth=%d %s" % (name, cycle, smoth, sw)
        roles = [im["role"] for im in p["images"]]
        assert len(roles) == len(set(roles)), where
        for im in p["images"]:
            planned += 1
            if im["role"] != "solve" or im["k_lds"] <= J:   # (a solve with nothing cached has no image)
                assert im["lds"] <= LDS_BUDGET, (where, im)
            if im["k_lds"] >= 2:
                assert im["tpr_rows"] <= BT, (where, im)
            assert im["k_tiny"] >= max(2, im["k_lds"]), (where, im)
            assert im["k_blk"] >= 2, (where, im)
        sws = sw.split(",")
        if "IPD_NO_SMALL" in sws:
            assert "solve" not in roles, where
        if "IPD_NO_SUBCYCLE" in sws:
            assert "sub" not in roles and "sub3" not in roles, where
        if "IPD_NO_RESIDENT" in sws or "IPD_NO_RESIDENT_THREE" in sws:
            assert "sub4" not in roles, where
        if "IPD_NO_BLK" in sws:
            assert all(im["k_blk"] == J + 1 for im in p["images"]), where
        if p["small_ok"]:
            assert roles == ["solve"], where
        if p["k_sub"]:
            assert any(im["role"] == "sub" and im["k_lds"] == p["k_sub"] for im in p["images"]), where
        if p["sub5"] != "none":
            assert p["sub5"] in roles, where
    assert planned > 100


def test_the_576_row_level_is_never_thread_per_row(driver):
    """DESIGN.md section 4's fault: plan_lds admitted a 576-row thread-per-row level into a BT-thread
    sub-cycle.  The sub-cycle must be rooted below it: at the block-wide polynomial level 4, or at level 5
    where the mask-form kernel's deep mode takes the tail (POLY4)."""
    for sw, root in (("-", 5), ("IPD_NO_RES_POLY4", 4)):
        (p,) = run_plans(driver, [(SHAPES["design4_576_over_175"], "w", 1, sw)])
        assert not p["small_ok"] and p["k_sub"] == root, (sw, p)
        sub = p["images"][0]
        assert sub["role"] == "sub" and sub["k_lds"] == root and sub["tpr_rows"] <= BT, (sw, p)


def test_bench_hierarchy_takes_no_image(driver):
    """bench.py's three-level m=n=1024 hierarchy runs on the level-resident kernel with a local tail:
    no level of it fits a single-workgroup image."""
    for cycle in "vw":
        (p,) = run_plans(driver, [(SHAPES["bench_1024"], cycle, 1, "-")])
        assert p["images"] == [] and not p["small_ok"] and p["k_sub"] == 0, p
