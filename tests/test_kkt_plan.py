"""The host rules of the KKT operators (csrc/ipd_kkt_plan.h) on the CPU: a small C++ driver
(tests/kkt_plan_driver.cpp) is built with the system g++ against the header and ipd_limits.h, and every rule must
agree with its Python restatement below on a grid that holds every edge.  The restatements are written from the
text of ipd_kkt.hip as it was before the rules got names (one unit, the route logic inline in kkt_asat), literals
included -- not from the header.  CPU only, no library."""
import itertools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "codes_of_ipd_ssn_amg_method_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
LIMITS = open(os.path.join(CSRC, "ipd_limits.h")).read()
ABI = open(os.path.join(ROOT, "include", "ipd_amg.h")).read()


def _const(name):
    return int(re.search(r"static constexpr int %s = (\d+);" % name, LIMITS).group(1))


def _code(name):
    return int(re.search(r"%s = (-?\d+)," % name, ABI).group(1))


NAMES = ["AX_TR", "AX_TC", "ATY_TC", "ASAT_TILE", "PHI_PARTS_MAX", "ASAT_SMALL_WORDS", "ASAT_SMALL_WGS",
         "ASAT_SMALL_HINT_MAX", "ASAT_GAVE_UP"]
C = {k: _const(k) for k in NAMES}
E_ARG, E_LIMIT = _code("IPD_E_ARG"), _code("IPD_E_LIMIT")

SIDES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048]
HINTS = [0, 1, 65535, 65536, 65537]
BASE = 0x7F0000001000          # a 4 KiB aligned address
ADDRS = [BASE + r for r in (0, 8, 4, 1)]
GRID = list(itertools.product(SIDES, SIDES))


# ---- the rules as the single unit had them -----------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def old_check_mn(m, n):
    if not (m > 0 and n > 0):
        return E_ARG, "m and n must be positive"
    if not (m < (1 << 28) and n < (1 << 28) and m * n < (1 << 40)):
        return E_LIMIT, "m*n too large"
    return 0, "-"


def old_asat_check(m, n):
    if not (m > 0 and n > 0):
        return E_ARG, "ASAt: empty p or q"
    if not (2 * m * n + m + n < (1 << 31) - 64):
        return E_LIMIT, "ASAt: 2*m*n + m + n must stay below 2^31 (32-bit row pointers)"
    return 0, "-"


def old_small(hint, m, n, dead_term=True):
    nib, njb, M = cdiv(m, 64), cdiv(n, 64), m + n
    ok = 0 < hint <= 65536 and nib <= 16 and njb <= 16
    return ok and (cdiv(M, 256) <= 64 if dead_term else True)


def old_cap(hint, m, n):
    """the small route's cap and the general route's guess: one expression, written twice; 0 without a hint"""
    return min(2 * m * n + m + n, hint + hint // 4 + 64) if hint > 0 else 0


def old_phi_parts(m, n):
    return max(1, min((m * n + 255) // 256, 1024))


# ---- the driver --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kkt_plan") / "kkt_plan_driver")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC,
                          "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "kkt_plan_driver.cpp"),
                          "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def ask(driver, lines):
    """the driver's answer lines to the given command lines"""
    res = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)
    out = res.stdout.splitlines()
    want = [C["AX_TR"], C["AX_TC"], C["AX_TR"] + 16, C["ATY_TC"]] + [C[k] for k in NAMES[3:]]
    assert out[0].split() == ["limits"] + [str(v) for v in want]
    assert len(out) == len(lines) + 1
    return out[1:]


def ints(driver, lines):
    return [[int(t) for t in o.split()] for o in ask(driver, lines)]


def checks(driver, cmd, cases):
    out = []
    for o in ask(driver, ["%s %d %d" % (cmd, m, n) for m, n in cases]):
        code, msg = o.split(" ", 1)
        out.append((int(code), msg))
    return out


def test_constants_are_the_literals_they_replace():
    assert C == {"AX_TR": 256, "AX_TC": 16, "ATY_TC": 16, "ASAT_TILE": 64, "PHI_PARTS_MAX": 1024,
                 "ASAT_SMALL_WORDS": 16, "ASAT_SMALL_WGS": 64, "ASAT_SMALL_HINT_MAX": 65536,
                 "ASAT_GAVE_UP": 0x7FFFFFFF}
    # 16 tiles of 64 on each side are at most 8 workgroups of 256 rows: within the 64 one sweep reads
    assert cdiv(2 * C["ASAT_SMALL_WORDS"] * C["ASAT_TILE"], 256) == 8 <= C["ASAT_SMALL_WGS"]


def test_check_mn(driver):
    cases = [(1, 1), (0, 5), (5, 0), (-1, 3), (3, -1), ((1 << 28) - 1, 1), (1 << 28, 1), (1, (1 << 28) - 1), (1, 1 << 28),
             (1 << 20, 1 << 20), (1 << 20, (1 << 20) - 1), ((1 << 28) - 1, 4096), ((1 << 28) - 1, 4097)] + GRID
    got = checks(driver, "checkmn", cases)
    assert got == [old_check_mn(m, n) for m, n in cases]
    assert [g[0] for g in got[:11]] == [0, E_ARG, E_ARG, E_ARG, E_ARG, 0, E_LIMIT, 0, E_LIMIT, E_LIMIT, 0]


def test_asat_refuses_what_wraps_32_bits(driver):
    ok, over = 238609286, 238609287
    assert (9 * ok + 4, 9 * over + 4, (1 << 31) - 64) == (2147483578, 2147483587, 2147483584)
    cases = [(ok, 4), (over, 4), (4, ok), (4, over), (0, 3), (3, 0), (40000, 40000), (32767, 32767), (32768, 32768)] + GRID
    got = checks(driver, "asatcheck", cases)
    assert got == [old_asat_check(m, n) for m, n in cases]
    assert [g[0] for g in got[:7]] == [0, E_LIMIT, 0, E_LIMIT, E_ARG, E_ARG, E_LIMIT]
    assert all(g == (0, "-") for g in got[9:])


def test_asat_geometry(driver):
    got = ints(driver, ["geo %d %d" % c for c in GRID])
    for (m, n), g in zip(GRID, got):
        nib, njb, M = cdiv(m, 64), cdiv(n, 64), m + n
        ntiles = nib * njb
        assert g == [nib, njb, M, ntiles,
                     nib * n, njb * m,                      # colmask / coloff, rowmask / rowoff
                     M + 2,                                 # rp
                     cdiv(ntiles, 4), cdiv(M, 256),         # masks and fill; offsets and small
                     cdiv(n, 64) + cdiv(m, 64),             # k_asat_diag (its nbc is njb == cdiv(n, 64))
                     8 * M], (m, n)                         # k_asat_small's dynamic LDS


def test_asat_wide_and_aty_vec2(driver):
    cases = [(m, a) for m in SIDES + [8, 16, 1000] for a in ADDRS]
    got = ints(driver, ["wide %d %d" % c for c in cases])
    assert [g for (g,) in got] == [int(m % 8 == 0 and (a & 7) == 0) for m, a in cases]
    assert {g for (g,) in got} == {0, 1}
    n = 17
    got = ints(driver, ["aty %d %d %d" % (m, n, a) for m, a in cases])
    for (m, a), g in zip(cases, got):
        vec2 = m % 2 == 0 and (a & 15) == 0
        assert g == [int(vec2), cdiv(m // 2, 256) if vec2 else cdiv(m, 256), cdiv(n, 16)], (m, a)
    assert {g[0] for g in got} == {0, 1}


def test_asat_capacity(driver):
    cases = [(h, m, n) for h in HINTS + [1024, 3328, 10 ** 9] for m, n in GRID + [(3, 5)]]
    got = ints(driver, ["cap %d %d %d" % c for c in cases])
    assert [g for (g,) in got] == [old_cap(*c) for c in cases]
    assert ints(driver, ["cap 1000000000 3 5"]) == [[2 * 3 * 5 + 8]]   # a hint far above the problem: 2mn + M
    assert ints(driver, ["cap 1024 256 256", "cap 3328 1088 64"]) == [[1344], [4224]]
    acc = [(1344, 1344), (1345, 1344), (0, 0), (0x7FFFFFFF, 1344), (0x7FFFFFFF, 0x7FFFFFFF)]
    assert [g for (g,) in ints(driver, ["accepts %d %d" % c for c in acc])] == [int(a <= b) for a, b in acc]


def test_asat_small_route(driver):
    cases = [(h, m, n) for h in HINTS for m, n in GRID]
    got = [g for (g,) in ints(driver, ["small %d %d %d" % c for c in cases])]
    assert got == [int(old_small(*c)) for c in cases]
    # the licence for dropping cdiv(M, 256) <= 64: it decides nothing where nib, njb <= 16 already hold
    assert [old_small(*c) for c in cases] == [old_small(*c, dead_term=False) for c in cases]
    table = dict(zip(cases, got))
    assert table[(65536, 1024, 1024)] == 1 and table[(65537, 1024, 1024)] == 0 and table[(0, 64, 64)] == 0
    assert table[(1, 1025, 1)] == 0 and table[(1, 1, 1025)] == 0 and table[(1, 1024, 1)] == 1


def test_asat_hint_updates(driver):
    gave_up = 0x7FFFFFFF
    got = ints(driver, ["hint_small 500 700", "hint_small 500 %d" % gave_up, "hint_small 500 0", "hint_small 500 2000",
                        "hint_general 0", "hint_general 123456"])
    # the one-launch route keeps its count as the hint even when the count exceeds the cap (the general route that
    # follows sizes its arrays by it); a give-up leaves the hint alone; the general route always sets it
    assert [g for (g,) in got] == [700, 500, 0, 2000, 0, 123456]


def test_ax_geometry(driver):
    got = ints(driver, ["ax %d %d" % c for c in GRID + [(257, 17), (256, 16), (255, 15)]])
    for (m, n), g in zip(GRID + [(257, 17), (256, 16), (255, 15)], got):
        nib, njb = cdiv(m, 256), cdiv(n, 16)
        assert g == [nib, njb, njb * m, nib * n, cdiv(m + n, 256)], (m, n)


def test_phi_parts(driver):
    shapes = [(1, 1), (256, 1), (257, 1), (512, 512), (262145, 1), (1, 262145), (4101 * 256, 1)] + GRID
    got = [g for (g,) in ints(driver, ["phi %d %d" % c for c in shapes])]
    assert got == [old_phi_parts(*c) for c in shapes]
    assert got[:5] == [1, 1, 2, 1024, 1024]
