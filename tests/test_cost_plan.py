"""The point-cloud cost's host-clean header (csrc/ipd_cost_plan.h) on the CPU: a small C++ driver
(tests/cost_plan_driver.cpp) is built with the system g++ against the header.  Every validation rule is run at its
boundary (the boundary values come from the driver's `limits` line, not from a copy here), the launch geometry
covers every entry of the shapes of tests/test_gpu_cost.py exactly once, and cost_entry -- the code the kernels fold
an entry with -- is bit-equal to the numpy reference.  CPU only."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "codes_of_ipd_ssn_amg_method_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))

# the shapes of tests/test_gpu_cost.py, and the largest the library takes
SHAPES = [(1, 1), (1, 70), (70, 1), (63, 5), (64, 64), (65, 17), (127, 33), (129, 31), (200, 37), (257, 3)]
METRICS = {"sqeuclidean": 1, "euclidean": 2, "cityblock": 3, "chebyshev": 4}


@functools.lru_cache(maxsize=None)
def driver_exe():
    d = tempfile.mkdtemp(prefix="cost_plan")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "cost_plan_driver")
    # -ffp-contract=off as the library's Makefile: multiply and add stay separate whatever the host's -march
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC,
                          os.path.join(HERE, "cost_plan_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _fields(line):
    rec = {}
    for tok in line.split()[1:]:
        if "=" in tok:
            k, v = tok.split("=")
            rec[k] = int(v)
    return rec


def ask(queries):
    res = subprocess.run([driver_exe()], input="\n".join(queries) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = res.stdout.strip().split("\n")
    assert out[0].startswith("limits ") and len(out) == len(queries) + 1, out
    return out[1:], _fields(out[0])


@functools.lru_cache(maxsize=None)
def limits():
    return ask([])[1]


def check(metric=1, dim=2, m=5, n=4, scale=0, xs="ok", ys="ok"):
    line = ask(["check %d %d %d %d %d %s %s" % (metric, dim, m, n, scale, xs, ys)])[0][0]
    return line.split()[1], _fields(line)["limit"]


# ---------------------------------------------------------------------------------------------------------------
# validation
# ---------------------------------------------------------------------------------------------------------------
def test_limits_are_the_issue_s():
    assert limits()["IPD_COST_DIM_MAX"] == 16 and limits()["IPD_APD_SIDE_MAX"] == 16384


def test_a_good_spec_passes():
    assert check() == ("OK", 0)


def test_null_pointers():
    assert check(xs="null") == ("NULL", 0) and check(ys="null") == ("NULL", 0)


def test_metric_at_its_boundaries():
    assert [check(metric=k)[0] for k in (0, 1, 4, 5, -1)] == ["METRIC", "OK", "OK", "METRIC", "METRIC"]


def test_dim_at_its_boundaries():
    D = limits()["IPD_COST_DIM_MAX"]
    assert [check(dim=d)[0] for d in (0, 1, D, D + 1, -3)] == ["DIM", "OK", "OK", "DIM", "DIM"]


def test_sides_at_their_boundaries_answer_as_a_limit():
    S = limits()["IPD_APD_SIDE_MAX"]
    assert check(m=S, n=1, dim=16) == ("OK", 0) and check(m=1, n=S) == ("OK", 0)
    for kw in (dict(m=S + 1), dict(n=S + 1), dict(m=0), dict(n=0), dict(m=-1)):
        assert check(**kw) == ("SHAPE", 1), kw


def test_scale_flag():
    assert [check(scale=s)[0] for s in (0, 1, 2, -1)] == ["OK", "OK", "SCALE", "SCALE"]


@pytest.mark.parametrize("bad", ["nan", "inf"])
def test_the_last_coordinate_is_read(bad):
    """The bad value sits in the last of the m*d (n*d) coordinates."""
    assert check(xs=bad) == ("COORD", 0) and check(ys=bad) == ("COORD", 0)
    assert check(xs=bad, m=257, dim=16)[0] == "COORD" and check(ys=bad, n=1, dim=1)[0] == "COORD"


def test_largest_entry_for_scaling():
    out = ask(["scaleok %s" % v for v in ("0", "-0.0", "5e-324", "1.5", "1.7976931348623157e308", "inf", "nan", "-1")])[0]
    assert [int(l.split()[1]) for l in out] == [0, 0, 1, 1, 1, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rpl", [1, 2])
def test_every_entry_is_covered_once(rpl):
    shapes = [s for s in SHAPES if rpl == 1 or s[0] % 2 == 0] + [(2, 3), (256, 16), (258, 17), (512, 130), (514, 129)]
    out = ask(["cover %d %d %d" % (m, n, rpl) for m, n in shapes])[0]
    T = limits()["COST_TC"]
    for (m, n), line in zip(shapes, out):
        f = _fields(line)
        assert (f["min"], f["max"], f["outside"]) == (1, 1, 0), (m, n, line)
        assert f["nib"] == -(-m // (256 * rpl)) and f["njg"] * f["reps"] * T >= n > (f["njg"] - 1) * f["reps"] * T
        assert f["waves"] == -(-m // (64 * rpl))


def test_large_grids_walk_more_columns_per_wave():
    """From 4096 workgroups on a wave takes 32 columns and more; the tail group of columns ends early."""
    f = _fields(ask(["cover 16384 2056 1"])[0][0])
    assert (f["min"], f["max"], f["outside"]) == (1, 1, 0) and f["reps"] == 2
    assert _fields(ask(["cover 4096 4096 2"])[0][0])["reps"] == 1


def test_rows_per_lane_rule():
    """Two rows per lane only for an even m, an aligned array and d in registers; the switch picks where both are
    possible."""
    D = limits()["COST_DT_MAX"]
    q = ["rpl 64 2 1 16", "rpl 65 2 1 16", "rpl 64 2 0 16", "rpl 64 %d 1 16" % (D + 1), "rpl 64 %d 1 16" % D,
         "rpl 64 2 1 8", "rpl 64 2 1 other"]
    out = [int(l.split()[1]) for l in ask(q)[0]]
    assert out[:6] == [2, 1, 1, 1, 2, 1]
    assert out[6] == int(ask(["rpl 64 2 1 -"])[0][0].split()[1])     # anything else: the default


# ---------------------------------------------------------------------------------------------------------------
# one entry
# ---------------------------------------------------------------------------------------------------------------
def entry_ref(metric, x, y):
    """The numpy reference of the issue for one pair of points: separate operations, ascending k."""
    acc = np.float64(0.0)
    for k in range(x.size):
        t = x[k] - y[k]
        if metric in (1, 2):
            acc = acc + t * t
        elif metric == 3:
            acc = acc + np.abs(t)
        else:
            acc = np.maximum(acc, np.abs(t))
    return np.sqrt(acc) if metric == 2 else acc


@pytest.mark.parametrize("name", list(METRICS))
def test_cost_entry_is_bit_equal_to_numpy(name):
    metric = METRICS[name]
    rng = np.random.default_rng(1234 + metric)
    cases = []
    for d in (1, 2, 3, 5, 16):
        for _ in range(40):
            cases.append((rng.standard_normal(d), rng.standard_normal(d)))
    x = rng.standard_normal(3)
    cases.append((x, x.copy()))                                        # a duplicated point: exactly +0.0
    cases.append((np.array([1e150, -1e150]), np.array([-1e150, 1e150])))
    q = ["entry %d %d %s" % (metric, x.size, " ".join(float(v).hex() for v in np.concatenate([x, y])))
         for x, y in cases]
    got = np.array([float.fromhex(l.split()[1]) for l in ask(q)[0]])
    with np.errstate(over="ignore"):
        want = np.array([entry_ref(metric, x, y) for x, y in cases])
    assert got.view(np.uint64).tolist() == want.view(np.uint64).tolist()
    assert got[-2] == 0.0 and not np.signbit(got[-2])
    if metric == 3:
        assert got[-1] == 4e150
