"""The point-position gradient's host-clean geometry header (csrc/ipd_point_grad_geo.h) on the CPU: a small C++ driver
(tests/point_grad_geo_driver.cpp) is built with the system g++ against the header, with -ffp-contract=off as the
library.  It shows that the header's scalar weights -- the code the kernels call -- have the bits of the numpy
restatement (tests/point_grad_ref.py) on random and on tie inputs, for the four metrics, with and without the divider
and on both sides; that each of the d components belongs to exactly one pass for d = 1 .. 16; and that the partial
buffer and the count records have the sizes the walking and the finishing kernel index.  CPU only."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from tests import point_grad_ref as R
from tests.geo_driver import CSRC, HERE, LARGE, SHAPES, cdiv, fields as _fields

DS = list(range(1, 17))


@functools.lru_cache(maxsize=None)
def exe():
    d = tempfile.mkdtemp(prefix="point_grad_geo")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    out = os.path.join(d, "point_grad_geo_driver")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC, "-I" + HERE,
                          os.path.join(HERE, "point_grad_geo_driver.cpp"), "-o", out], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return out


def ask(queries):
    res = subprocess.run([exe()], input="\n".join(queries) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = res.stdout.strip().split("\n")
    assert out[0].startswith("limits ") and len(out) == len(queries) + 1, out
    return out[1:], _fields(out[0])


def hexbits(v):
    return "%016x" % int(np.float64(v).view(np.uint64))


def test_limits():
    assert ask([])[1] == dict(TR=256, TC=16, APD_WAVES=4, WK_CPG=4, PG_KC=4, PG_NC=5, PG_DT_MAX=3, PG_REC=2,
                              PG_STATS_DOUBLES=3, DIM_MAX=16)


def test_refused_arguments():
    out = ask(["geo 5 5 0 0", "geo 5 5 17 0", "geo 5 5 3 2", "geo 5 5 3 -1", "h 0 3 0 0 0", "h 5 3 0 0 0", "geo 5 5 16 1"])[0]
    assert out[:4] == ["geo refused"] * 4 and out[4:6] == ["h refused"] * 2 and out[6].startswith("geo nib=")


def clouds(kind, m, n, d, seed):
    if kind == "ties":
        return R.tie_points(m, n, d, seed)
    rs = np.random.RandomState(seed)
    return rs.standard_normal((m, d)), rs.standard_normal((n, d))


@pytest.mark.parametrize("kind", ["random", "ties"])
@pytest.mark.parametrize("metric", [1, 2, 3, 4])
def test_weights_have_the_restatements_bits(metric, kind):
    worst_kinks = 0
    for d in (1, 2, 3, 4, 5, 16):
        m, n = 9, 8
        xs, ys = clouds(kind, m, n, d, 100 * metric + d)
        for divide, denom in ((0, 1.0), (1, float(R.cost(xs, ys, metric).max()))):
            H, kink = R.weights(xs, ys, metric, denom if divide else None)
            for side in (0, 1):
                q = ["h %d %d %d %s %d %s %s" % (metric, d, divide, hexbits(denom), side,
                                                 " ".join(hexbits(v) for v in xs[i]), " ".join(hexbits(v) for v in ys[j]))
                     for i in range(m) for j in range(n)]
                out = ask(q)[0]
                got = np.array([[int(t, 16) for t in line.split("w=")[1].split()] for line in out], np.uint64)
                got = got.view(np.float64).reshape(m, n, d)
                gk = np.array([int(line.split()[1].split("=")[1]) for line in out]).reshape(m, n).astype(bool)
                want = -H if side else H
                # bit for bit, the sign of a zero included
                assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), (metric, d, side)
                assert np.array_equal(gk, kink), (metric, d)
        worst_kinks = max(worst_kinks, int(kink.sum()))
    if kind == "ties" and metric > 1:
        assert worst_kinks > 0          # the tie inputs do reach the kinks


@pytest.mark.parametrize("side", [0, 1])
def test_every_component_has_one_pass(side):
    q = ["cover 300 147 %d %d" % (d, side) for d in DS]
    g = ["geo 300 147 %d %d" % (d, side) for d in DS]
    for d, cl, gl in zip(DS, ask(q)[0], ask(g)[0]):
        c, f = _fields(cl), _fields(gl)
        assert (c["cmin"], c["cmax"]) == (1, 1), (d, cl)
        assert c["kcmax"] == min(d, 4) and c["tail"] == (d % 4 or 4)
        assert f["npass"] == f["reads"] == cdiv(d, 4)          # x is read once for d <= 4
        # the passes share the buffer: d does not enter its size
        assert f["part"] == _fields(ask(["geo 300 147 16 %d" % side])[0][0])["part"]


@pytest.mark.parametrize("side", [0, 1])
def test_buffer_sizes_are_what_the_kernels_index(side):
    shapes = SHAPES + LARGE + [(65, 150), (600, 45)]
    geo = ask(["geo %d %d 16 %d" % (m, n, side) for m, n in shapes])[0]
    reach = ask(["reach %d %d 16 %d" % (m, n, side) for m, n in shapes])[0]
    for (m, n), gl, rl in zip(shapes, geo, reach):
        g, r = _fields(gl), _fields(rl)
        assert g["nib"] == cdiv(m, 256) and g["nslot"] == 4 * g["nib"] and g["ng"] == cdiv(cdiv(n, 16), 4)
        assert (g["R"], g["S"]) == ((n, g["nslot"]) if side else (m, g["ng"]))
        assert g["stride"] == g["R"] and g["plane"] == g["S"] * g["R"] and g["part"] == 5 * g["plane"], gl
        assert r["len"] == g["part"] and r["outside"] == 0
        assert r["wmax"] == r["rmax"] == g["part"] - 1, (m, n, rl)
        assert r["unwritten"] == 0 and r["dup"] == 0, (m, n, rl)
        assert g["rec"] == 2 * g["nib"] * g["ng"] == r["reclen"] and r["recw"] == g["rec"] - 1
        assert r["recdup"] == 0 and r["recunwritten"] == 0
        assert g["scratch_dev"] == 8 * (g["part"] + g["rec"] + 3)
        assert g["scratch_host"] == g["scratch_dev"] + 8 * (16 * g["R"] + g["R"])
        assert g["scratch_host_spec"] == g["scratch_host"] + 8 * 16 * (m + n)
        if m >= 1024 and n >= 1024:
            assert g["scratch_host_spec"] <= 2 * m * n, (m, n, side)
