"""The planner of the resident kernels (csrc/ipd_resident_plan.h) on the CPU: tests/resident_plan_driver.cpp is
built with the system g++ against the header and run on level shapes.  What the planner returns is checked by
execution: the width rules against their Python mirrors for every stride, the cut-offs at the value and one
past it, invariants over the shapes, options and switches of test_level_plan.py on two CU counts, every key
against the table of instantiations (RESIDENT_KERNELS, csrc/ipd_resident_host.hip, read from the source the
normal build compiles), and named hierarchies against committed records.  CPU only."""
import os
import re
import subprocess

import pytest

from tests.test_level_plan import CSRC, HERE, OPTS, SHAPES, SWITCHES, lv

LDS_MAX = 156 * 1024
FIELDS = ("stage kind big ke ke3 poly2 ke2 rpw deep G grid lds remote three poly3 poly4 tail_root tail_image "
          "tail_bm S1 S2 S3 priv1 priv2 priv3 wident ranks levels").split()


# ---------------------------------------------------------------------------------------------------------------
# the table of instantiations, from the source
# ---------------------------------------------------------------------------------------------------------------
def spelled(big, a, b, flag):
    """An instantiation's name as ipd_amg_resident_kernel reports it, from its key: (ke, ke3, poly2) of
    k_resident, (ke2, rpw, deep) of k_resident_big."""
    if big:
        return "k_resident_big<%d,%d,%s>" % (a, b, "true" if flag else "false")
    return "k_resident<%d,%d,%d%s>" % (a, a, b, ",true" if flag else "")


def resident_table():
    """The rows of RESIDENT_KERNELS as a list of (name, name spelled from the row's key, name spelled from the
    row's kernel).  The table contains no conditionals: every row is compiled."""
    text = open(os.path.join(CSRC, "ipd_resident_host.hip")).read()
    start = text.index("static const ResidentKernel RESIDENT_KERNELS[] = {")
    rows = []
    for line in text[start:text.index("\n};", start)].splitlines()[1:]:
        t = line.strip()
        assert not t.startswith("#"), ("unexpected conditional", t)
        m = re.fullmatch(r'\{"([^"]+)", ResidentKey::(k|mask)\((\d+), (\d+), (true|false)\), '
                         r'IPD_KFN\((k_resident(?:_big)?)<([^>]*)>\)\},', t)
        assert m, ("unexpected row", t)
        name, ctor, a, b, flag, fn, targs = m.groups()
        big = ctor == "mask"
        targs = [v.strip() for v in targs.split(",")]
        if fn == "k_resident":
            assert targs[0] == targs[1] and len(targs) == 4, t
            kern = spelled(False, int(targs[0]), int(targs[2]), targs[3] == "true")
        else:
            assert len(targs) == 3, t
            kern = spelled(True, int(targs[0]), int(targs[1]), targs[2] == "true")
        rows.append((name, spelled(big, int(a), int(b), flag == "true"), kern))
    return rows


def test_table_rows_are_consistent():
    rows = resident_table()
    assert len(rows) == 14
    for name, from_key, from_kernel in rows:
        assert name == from_key == from_kernel, (name, from_key, from_kernel)
    assert len({r[0] for r in rows}) == 14


# ---------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resident_plan") / "resident_plan_driver")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC,
                          os.path.join(HERE, "resident_plan_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def pad4(s):
    return (s + 3) // 4 * 4


def case(levels, cycle="v", smoth=1, sw="-", cus=256, images="plan", S=None, bigph=1, twogrid=0):
    """S: strides of the launches' padded copies of levels 1..3; default: every level has one, as wide as its
    longest row."""
    if S is None:
        S = [pad4(level[3]) for level in levels[:3]]
    S = (list(S) + [0, 0, 0])[:3]
    return " ".join([str(len(levels)), cycle, str(smoth), str(twogrid), str(bigph), sw, str(cus), images] +
                    [str(v) for v in S] + [str(v) for level in levels for v in level])


def run(driver, cases):
    """Per case: {"images": [...], "prepare": plan, "big": plan, "deep": plan, "final": the plan the hierarchy
    ends with, "name": its instantiation or ""}."""
    res = subprocess.run([driver], input="\n".join(cases) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out, cur = [], None
    for ln in res.stdout.splitlines():
        f = ln.split()
        if f[0] == "images":
            cur = {"images": f[1:]}
        elif f[0] == "resident":
            p = {k: (v if k in ("stage", "kind", "tail_image") else int(v)) for k, v in zip(FIELDS, f[1:])}
            assert len(f) == len(FIELDS) + 1
            cur[p["stage"]] = p
        else:
            final = cur["prepare"]
            for stage in ("big", "deep"):
                if cur[stage]["kind"] != "none":
                    final = cur[stage]
            cur["final"] = final
            cur["name"] = name_of(final)
            out.append(cur)
    assert len(out) == len(cases)
    return out


def name_of(p):
    if p["kind"] == "none":
        return ""
    if p["big"]:
        return spelled(True, p["ke2"], p["rpw"], p["deep"])
    return spelled(False, p["ke"], p["ke3"], p["poly2"])


# ---------------------------------------------------------------------------------------------------------------
# the width rules by execution
# ---------------------------------------------------------------------------------------------------------------
DENSE3 = [lv(2048, 2099200, 1024, 1024), lv(1024, 1048576, 0, 1023, 1049600), lv(1, 1, 0, 0, 1024)]
HUB4 = [lv(1024, 200000, 512, 400), lv(512, 100000, 0, 400, 50000), lv(165, 20000, 0, 164, 20000),
        lv(3, 9, 0, 2, 165)]
BIG3 = [lv(4096, 8390656, 2048, 2048), lv(2048, 4194304, 0, 2047, 4196352), lv(1, 1, 0, 0, 2048)]
DEEP7 = SHAPES["newton_7"]


def test_widths_match_the_mirrors_for_every_stride(driver):
    from tests.test_gpu_resident_instantiations import big_ke2, ke3_of, ke_of
    strides = range(1, 2049)
    # k_resident, levels 1-2: ke from max(S1, S2), none beyond 16 entries per lane
    for which in (0, 1):
        plans = run(driver, [case(DENSE3, S=[s, 4] if which == 0 else [4, s], images="none") for s in strides])
        for s, r in zip(strides, plans):
            p = r["prepare"]
            if ke_of(s) <= 16:
                assert (p["kind"], p["ke"], p["ke3"]) == ("k", ke_of(s), 0), (s, p)
            else:
                assert p["kind"] == "none", (s, p)
    assert ke_of(1024) == 16 and ke_of(1025) == 32            # the cut-off sits at 1024 | 1025
    # level 3 resident (four levels, local tail): ke3 from S3; only with S3 <= 512 and max(S1, S2) <= 512,
    # and so never beside 16-entry slices (ke > 8)
    plans = run(driver, [case(HUB4, cycle="w", S=[512, 512, s], images="none") for s in strides])
    for s, r in zip(strides, plans):
        p = r["prepare"]
        if s <= 512:
            assert (p["kind"], p["three"], p["ke"], p["ke3"]) == ("k", 1, 8, ke3_of(s)), (s, p)
        else:
            assert p["kind"] == "none", (s, p)
    for S, taken in (([512, 512, 512], True), ([513, 512, 512], False), ([512, 513, 512], False),
                     ([512, 512, 513], False), ([1024, 1024, 4], False)):
        (r,) = run(driver, [case(HUB4, cycle="w", S=S, images="none")])
        assert (r["prepare"]["kind"] == "k") == taken, (S, r["prepare"])
    # mask-form kernel, three levels: ke2 from S2 up to 2048
    plans = run(driver, [case(BIG3, S=[2048, s]) for s in list(strides) + [2049, 2052]])
    for s, r in zip(list(strides) + [2049, 2052], plans):
        p = r["big"]
        if s <= 2048:
            assert (p["kind"], p["ke2"], p["rpw"], p["deep"]) == ("big", big_ke2(s, False), 1, 0), (s, p)
        else:
            assert p["kind"] == "none", (s, p)
    # ... deep mode: ke2 from S2 up to 512
    plans = run(driver, [case(DEEP7, cycle="w", S=[16, s]) for s in strides])
    for s, r in zip(strides, plans):
        p = r["deep"]
        if s <= 512:
            assert (p["kind"], p["ke2"], p["rpw"], p["deep"]) == ("deep", big_ke2(s, True), 2, 1), (s, p)
        else:
            assert p["kind"] == "none", (s, p)


def test_a_level_without_padded_copy_gets_a_private_one(driver):
    """S = 0 (rows too uneven for the launches' copy): a private copy with the longest row, rounded up to 4, as
    stride; the widths follow that stride."""
    (r,) = run(driver, [case(DENSE3, S=[0, 0], images="none")])
    p = r["prepare"]
    assert (p["S1"], p["S2"], p["priv1"], p["priv2"], p["ke"]) == (1024, 1024, 1, 1, 16), p
    (r,) = run(driver, [case(HUB4, cycle="w", S=[400, 400, 0], images="none")])
    p = r["prepare"]
    assert (p["three"], p["S3"], p["priv3"], p["ke3"]) == (1, 164, 1, 4), p
    (r,) = run(driver, [case(BIG3, S=[2048, 0])])
    assert (r["big"]["S2"], r["big"]["priv2"], r["big"]["ke2"]) == (2048, 1, 32), r["big"]


# ---------------------------------------------------------------------------------------------------------------
# invariants
# ---------------------------------------------------------------------------------------------------------------
RES_SWITCHES = SWITCHES + ["IPD_NO_RESIDENT_REMOTE", "IPD_NO_RESIDENT_BIG", "IPD_NO_RESIDENT_DEEP", "IPD_RESIDENT_BIG",
                           "IPD_RESIDENT_G=150", "IPD_RESIDENT_RANKS=4,IPD_RESIDENT_BIG"]
RES_SHAPES = dict(SHAPES, big_4096=BIG3, hub_4=HUB4)
ALL = [(name, cycle, smoth, sw, cus) for name in RES_SHAPES for cycle, smoth in OPTS for sw in RES_SWITCHES
       for cus in (256, 128)]


def test_every_plan_keeps_the_invariants(driver):
    table = {r[0] for r in resident_table()}
    plans = run(driver, [case(RES_SHAPES[n], cycle, smoth, sw, cus) for n, cycle, smoth, sw, cus in ALL])
    taken = {}
    for (name, cycle, smoth, sw, cus), r in zip(ALL, plans):
        L = RES_SHAPES[name]
        nf, nc, N2 = L[0][2], L[0][0] - L[0][2], L[1][0]
        where = "%s %s smoth=%d %s cus=%d" % (name, cycle, smoth, sw, cus)
        sws = sw.split(",")
        assert not (r["big"]["kind"] != "none" and r["deep"]["kind"] != "none"), where
        for stage in ("prepare", "big", "deep"):
            p = r[stage]
            assert p["kind"] in {"prepare": ("none", "k"), "big": ("none", "big"), "deep": ("none", "deep")}[stage], where
            if p["kind"] == "none":
                assert (p["G"], p["grid"], p["ke"], p["ke2"], p["lds"]) == (0, 0, 0, 0, 0), (where, p)
                continue
            taken[p["kind"]] = taken.get(p["kind"], 0) + 1
            assert name_of(p) in table, (where, name_of(p))
            assert p["grid"] == p["G"] + p["remote"] and p["grid"] <= cus, (where, p)
            assert 1 <= p["G"] <= min(nf, nc, N2), (where, p)
            assert 0 < p["lds"] <= LDS_MAX, (where, p)
            assert (p["tail_image"] != "none") == bool(p["remote"]), (where, p)
            if p["remote"]:
                assert p["tail_image"] in r["images"], (where, p, r["images"])
            assert p["tail_root"] == p["levels"] + 1 and p["levels"] in (2, 3, 4), (where, p)
            assert p["poly4"] <= p["poly3"] and (p["levels"] == 4) == bool(p["poly4"]), (where, p)
            if cycle == "v" and smoth == 0:
                assert not p["poly3"] and p["kind"] == "k", (where, p)     # the polynomial forms need a sweep
            if "IPD_NO_RESIDENT_THREE" in sws:
                assert not p["three"], (where, p)
            if "IPD_NO_RESIDENT_REMOTE" in sws and p["kind"] == "k":
                assert not p["remote"], (where, p)
            if "IPD_NO_POLY" in sws and p["kind"] == "k":
                assert not p["poly3"], (where, p)
            if "IPD_NO_RES_POLY4" in sws:
                assert not p["poly4"], (where, p)
            if "IPD_RESIDENT_G=150" in sws and p["kind"] != "big":
                assert p["G"] >= 150, (where, p)
            if p["kind"] == "big":
                assert p["ranks"] == (4 if "IPD_RESIDENT_RANKS=4" in sws else 1), (where, p)
        if "IPD_NO_RESIDENT" in sws:
            assert r["final"]["kind"] == "none", where
        if "IPD_NO_RESIDENT_BIG" in sws:
            assert r["final"]["kind"] in ("none", "k"), where
        if "IPD_NO_RESIDENT_DEEP" in sws:
            assert r["deep"]["kind"] == "none", where
        if "IPD_RESIDENT_BIG" not in sws and r["prepare"]["kind"] == "k":
            assert r["final"] is r["prepare"], where                      # only a forced mask-form plan replaces one
    assert taken["k"] > 100 and taken["big"] > 20 and taken["deep"] > 20, taken


def test_forced_mask_form_replaces_a_k_resident_plan(driver):
    shape = [lv(2048, 1100000, 1024, 571), lv(1024, 1048576, 0, 1023, 1049600), lv(1, 1, 0, 0, 1024)]
    (free,), (forced,) = run(driver, [case(shape)]), run(driver, [case(shape, sw="IPD_RESIDENT_BIG")])
    assert free["name"] == "k_resident<16,16,0>" and free["big"]["kind"] == "none"
    assert forced["prepare"]["kind"] == "k" and forced["name"] == "k_resident_big<16,1,false>"


# ---------------------------------------------------------------------------------------------------------------
# named hierarchies, expected values from committed records
# ---------------------------------------------------------------------------------------------------------------
def test_the_metric_hierarchy(driver):
    """bench.py's default hierarchy 2048 / 1024 / 1: k_resident<16,16,0>, 128 workgroups, local tail (DESIGN.md
    section 4, mode 5; BENCH_r04.json: resident_grid 128)."""
    for cycle in "vw":
        (r,) = run(driver, [case(SHAPES["bench_1024"], cycle=cycle)])
        p = r["final"]
        assert r["name"] == "k_resident<16,16,0>" and (p["grid"], p["remote"], p["tail_root"]) == (128, 0, 3), p


def test_the_4096_row_hierarchy(driver):
    """4096 / 2048 / 1: the mask-form kernel k_resident_big<32,1,false> on 256 workgroups
    (tests/test_gpu_resident_big.py, test_m2048_resident_big_against_launch_path)."""
    (r,) = run(driver, [case(BIG3)])
    assert r["prepare"]["kind"] == "none"
    assert r["name"] == "k_resident_big<32,1,false>" and r["final"]["grid"] == 256, r["final"]
    (r,) = run(driver, [case(BIG3, cus=128)])
    assert r["name"] == "", r["final"]                                     # 256 workgroups do not fit 128 CUs


def test_the_instantiation_cases_sizes(driver):
    """The level sizes written beside each system of test_gpu_resident_instantiations.py's case table (rows per
    level; longest rows of levels 1-3) and the kernel the table expects there.  Three-level hierarchies have no
    LDS image, so their sizes determine the plan: the whole name is asserted.  Deeper ones also depend on the
    images the level plan packs from entry counts the comments do not give: those stay with the GPU test, and
    here only the widths the strides determine are asserted, on whatever plan the sizes lead to."""
    from tests.test_gpu_resident_instantiations import CASES
    sizes = {  # case id -> rows per level, longest rows (see the comments of the case table)
        "bern256-local": ([512, 256, 1], [176, 255]),
        "bern512-local": ([1024, 512, 1], [189, 511]),
        "bern1024-local": ([2048, 1024, 11], [138, 1023]),
        "bern1024-forced-local": ([2048, 1024, 1], [571, 1023]),
        "bern2000x256-local": ([2256, 2000, 1], [255, 1999]),
        "hub256-local": ([512, 256, 43, 1], [256, 255, 42]),
        "hub512-local": ([1024, 512, 165, 3], [512, 511, 164]),
        "treehub230-remote4": ([2048, 1024, 177, 14, 1], [235, 256, 176]),
        "treehub490-remote4": ([2048, 1024, 180, 15, 1], [494, 510, 179]),
    }
    seen = 0
    for name, cs in CASES.items():
        for c in cs:
            if c["id"] not in sizes:
                continue
            rows, longest = sizes[c["id"]]
            longest = longest + [0] * (len(rows) - len(longest))
            nf = rows[0] - rows[1]
            levels = [lv(n, n * (w + 1), nf if k == 0 else 0, w, 2 * rows[k - 1] if k else 0)
                      for k, (n, w) in enumerate(zip(rows, longest))]
            sw = ",".join(c["kv"]) if c["kv"] else "-"
            (r,) = run(driver, [case(levels, cycle=c["cycle"], smoth=c["smoth"], sw=sw,
                                    images="none" if len(rows) <= 4 else "plan")])
            p = r["final"]
            if len(rows) == 3:
                assert r["name"] == name, (c["id"], r["name"], name)
                assert p["remote"] == 0 and p["tail_root"] == 3 == c["lv"][1], (c["id"], p)
                seen += 1
            elif "local" in c["id"]:                    # four levels, local tail: no image involved either
                assert r["name"] == name and (p["three"], p["remote"]) == (1, 0), (c["id"], r["name"], name)
                seen += 1
            elif p["kind"] != "none":
                assert [p["ke"], p["ke"]] == [int(v) for v in re.findall(r"\d+", name)[:2]], (c["id"], p)
    assert seen == 7
