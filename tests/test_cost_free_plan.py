"""The matrix-free cost source of csrc/ipd_cost_plan.h (CostSrc, cost_src_entry, cost_free_check)
on the CPU: a small C++ driver (tests/cost_free_driver.cpp) is built with the system g++ against the header.  An
entry recomputed from the source -- the code the matrix-free passes run per entry -- is bit-equal to the numpy
definition of the stored cost (the `cost_ref` of tests/test_gpu_cost.py, restated here), for the four metrics,
d in {1, 2, 3}, scale off and on; a duplicated point gives exactly +0.0; cost_free_check takes 1..3.  CPU only."""
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

METRICS = {"sqeuclidean": 1, "euclidean": 2, "cityblock": 3, "chebyshev": 4}
SHAPES = [(1, 1), (65, 17), (200, 37)]


@functools.lru_cache(maxsize=None)
def driver_exe():
    d = tempfile.mkdtemp(prefix="cost_free")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "cost_free_driver")
    # -ffp-contract=off as the library's Makefile: multiply and add stay separate whatever the host's -march
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC,
                          os.path.join(HERE, "cost_free_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def ask(queries):
    res = subprocess.run([driver_exe()], input="\n".join(queries) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = res.stdout.strip().split("\n")
    assert out[0].startswith("limits ") and len(out) == len(queries) + 1, out[:3]
    return out[1:], dict((k, int(v)) for k, v in (t.split("=") for t in out[0].split()[1:]))


def cost_ref(xs, ys, metric, scale=False):
    """The definition, in numpy: (m, d) and (n, d) points -> (m, n)."""
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    xs = xs[:, None] if xs.ndim == 1 else xs
    ys = ys[:, None] if ys.ndim == 1 else ys
    acc = np.zeros((xs.shape[0], ys.shape[0]))
    for k in range(xs.shape[1]):
        t = xs[:, k][:, None] - ys[:, k][None, :]
        if metric in ("sqeuclidean", "euclidean"):
            acc = acc + t * t
        elif metric == "cityblock":
            acc = acc + np.abs(t)
        else:
            acc = np.maximum(acc, np.abs(t))
    if metric == "euclidean":
        acc = np.sqrt(acc)
    if scale:
        acc = acc / acc.max()
    return acc


def matrix_query(xs, ys, metric, scale):
    """coordinate-major, as the library keeps the coordinates"""
    m, d = xs.shape
    coords = np.concatenate([xs.T.reshape(-1), ys.T.reshape(-1)])
    return "matrix %d %d %d %d %d %s" % (METRICS[metric], d, m, ys.shape[0], 1 if scale else 0,
                                         " ".join(float(v).hex() for v in coords))


def matrix_of(line, m, n):
    vals = np.array([float.fromhex(t) for t in line.split()[1:]])
    assert vals.size == m * n
    return vals.reshape(n, m).T


def test_limits():
    lim = ask([])[1]
    assert lim["COST_FREE_DIM_MAX"] == 3 and lim["COST_DT_MAX"] == 3


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("metric", list(METRICS))
def test_entry_from_the_source_is_bit_equal_to_numpy(metric, d):
    cases = []
    for m, n in SHAPES:
        rs = np.random.RandomState(100 * METRICS[metric] + 10 * d + m)
        xs, ys = rs.standard_normal((m, d)), rs.standard_normal((n, d))
        for scale in (False, True):
            cases.append((xs, ys, scale))
    out = ask([matrix_query(xs, ys, metric, scale) for xs, ys, scale in cases])[0]
    for (xs, ys, scale), line in zip(cases, out):
        m, n = xs.shape[0], ys.shape[0]
        got, want = matrix_of(line, m, n), cost_ref(xs, ys, metric, scale)
        bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
        assert bad.size == 0, (m, n, scale, bad[:5], got.ravel()[bad[:5]], want.ravel()[bad[:5]])
        if scale:
            assert got.max() == 1.0


@pytest.mark.parametrize("metric", list(METRICS))
def test_duplicated_points_give_exact_plus_zero(metric):
    rs = np.random.RandomState(9)
    for d in (1, 2, 3):
        xs, ys = rs.standard_normal((65, d)), rs.standard_normal((17, d))
        ys[4] = xs[60]
        ys[16] = xs[64]
        for scale in (False, True):
            got = matrix_of(ask([matrix_query(xs, ys, metric, scale)])[0][0], 65, 17)
            assert np.array_equal(got.view(np.int64), cost_ref(xs, ys, metric, scale).view(np.int64))
            for i, j in ((60, 4), (64, 16)):
                assert got[i, j] == 0.0 and not np.signbit(got[i, j])


def test_cost_free_check_takes_one_to_three():
    out = ask(["check %d" % d for d in (1, 2, 3, 0, 4, 16)])[0]
    assert [l.split()[1] for l in out] == ["OK", "OK", "OK", "DIM", "DIM", "DIM"]
    # a refusal is a limit (IPD_E_LIMIT), and its text names it
    assert [l.split()[2] for l in out] == ["limit=0"] * 3 + ["limit=1"] * 3
    assert all(l.split()[3] == "text=1" for l in out)
