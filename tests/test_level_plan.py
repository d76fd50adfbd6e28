"""The level planner of the single-workgroup kernels (csrc/ipd_level_plan.h) on the CPU: a small C++
driver (tests/level_plan_driver.cpp) is built with the system g++ against the header and run on
synthetic hierarchies; every image it plans must keep the planner's invariants.  CPU only."""
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


BT = _const("BT")
LDS_BUDGET = 150 * 1024


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


def run_plans(driver, cases):
    lines = []
    for levels, cycle, smoth, sw in cases:
        lines.append(" ".join([str(len(levels)), cycle, str(smoth), "0", "0", sw] +
                              [str(v) for level in levels for v in level]))
    res = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    plans, cur = [], None
    for ln in res.stdout.splitlines():
        f = ln.split()
        if f[0] == "plan":
            cur = {"small_ok": int(f[1]), "k_sub": int(f[2]), "semi_root": int(f[3]), "sub5": f[4], "images": []}
        elif f[0] == "image":
            cur["images"].append(dict(role=f[1], k_lds=int(f[2]), k_semi=int(f[3]), k_tiny=int(f[4]),
                                      k_blk=int(f[5]), stage=int(f[6]), lds=int(f[7]), tpr_rows=int(f[8])))
        else:
            plans.append(cur)
    assert len(plans) == len(cases)
    return plans


ALL_CASES = [(name, cycle, smoth, sw) for name in SHAPES for cycle, smoth in OPTS for sw in SWITCHES]


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
