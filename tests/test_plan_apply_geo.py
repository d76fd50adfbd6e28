"""The plan products' host-clean geometry header (csrc/ipd_plan_apply_geo.h) on the CPU: a small C++ driver
(tests/plan_apply_geo_driver.cpp) is built with the system g++ against the header.  Over the shapes of
tests/test_apd_geo.py and k in {1, 3, 4, 5, 15, 16} it shows that each of the k components belongs to exactly one
pass, that the partial buffer has the size the walking kernels' and the finishing kernel's index functions reach, and
that the scratch of a call stays at or below 2*mn bytes from m = n = 1024 on.  The walk of the rows and columns itself
is tests/test_walk_geo.py's.  The group count is not switchable: the natural rule gives three groups with a partly
filled last one at 65 x 150 (pinned below), which tests/test_gpu_plan_apply.py runs.  CPU only."""
import pytest

from tests.geo_driver import LARGE, SHAPES, WALK, GeoDriver, cdiv, fields as _fields

DRV = GeoDriver("plan_apply_geo_driver")
ask, limits = DRV.ask, DRV.limits
KS = [1, 3, 4, 5, 15, 16]


def test_limits():
    assert limits() == dict(TR=256, TC=16, APD_WAVES=4, PA_KMAX=16, PA_KC=4, PA_NC=5, WK_CPG=4)


def test_refused_arguments():
    out = ask(["geo 5 5 0 0", "geo 5 5 17 0", "geo 5 5 -1 1", "geo 5 5 3 2", "geo 5 5 3 -1", "geo 5 5 16 1"])[0]
    assert out[:5] == ["geo refused"] * 5 and out[5].startswith("geo nib=")


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("k", KS)
def test_every_column_and_component_has_one_owner(k, side):
    shapes = SHAPES + LARGE
    out = ask(["cover %d %d %d %d" % (m, n, k, side) for m, n in shapes])[0]
    geo = ask(["geo %d %d %d %d" % (m, n, k, side) for m, n in shapes])[0]
    walk = WALK.ask(["cover %d %d" % s for s in shapes])[0]   # the columns: the walk of tests/test_walk_geo.py
    T, CPG, KC = limits()["TC"], limits()["WK_CPG"], limits()["PA_KC"]
    for (m, n), line, gl, wl in zip(shapes, out, geo, walk):
        f, g, w = _fields(line), _fields(gl), _fields(wl)
        assert (w["min"], w["max"]) == (1, 1), (m, n, wl)
        assert (f["cmin"], f["cmax"]) == (1, 1), (m, n, k, line)
        assert f["kcmax"] == min(k, KC) and f["tail"] == (k % KC or KC)
        assert g["npass"] == cdiv(k, KC)
        # the last group is the only one that can end early, and the groups before it are full
        assert g["ng"] * CPG * T >= n > (g["ng"] - 1) * CPG * T
        assert w["broke"] == (1 if cdiv(n, T) % CPG else 0)
        assert w["idle"] == g["ng"] * CPG - cdiv(n, T)


def test_three_groups_with_a_partly_filled_last_one():
    """The shape tests/test_gpu_plan_apply.py uses for it: 150 columns are 10 chunks, the last with 6 columns, in
    groups of 4, 4 and 2 chunks."""
    g = _fields(ask(["geo 65 150 5 0"])[0][0])
    f = _fields(WALK.ask(["cover 65 150"])[0][0])
    assert (g["nib"], g["ng"], g["nslot"], g["npass"]) == (1, 3, 4, 2)
    assert (f["broke"], f["idle"]) == (1, 2)


@pytest.mark.parametrize("side", [0, 1])
def test_buffer_sizes_are_what_the_kernels_index(side):
    """Side 0: ng partials of PA_NC components per row, side 1: 4*nib per column; every entry the finishing kernel
    reads is written exactly once per pass, and the last one is the buffer's last.  (k does not enter: the passes
    share the buffer.)"""
    shapes = SHAPES + LARGE
    geo = ask(["geo %d %d 16 %d" % (m, n, side) for m, n in shapes])[0]
    reach = ask(["reach %d %d 16 %d" % (m, n, side) for m, n in shapes])[0]
    NC = limits()["PA_NC"]
    for (m, n), gl, rl in zip(shapes, geo, reach):
        g, r = _fields(gl), _fields(rl)
        assert g["nib"] == cdiv(m, limits()["TR"]) and g["nslot"] == 4 * g["nib"]
        assert (g["R"], g["S"]) == ((n, g["nslot"]) if side else (m, g["ng"]))
        assert g["stride"] == NC * g["R"] and g["part"] == g["S"] * NC * g["R"], gl
        assert r["len"] == g["part"] and r["outside"] == 0
        assert r["wmax"] == r["rmax"] == g["part"] - 1, (m, n, rl)
        assert r["unwritten"] == 0 and r["dup"] == 0, (m, n, rl)


def test_other_k_share_the_buffer():
    for k in KS:
        a = ask(["geo 300 147 %d %d" % (k, s) for s in (0, 1)])[0]
        b = ask(["geo 300 147 16 %d" % s for s in (0, 1)])[0]
        assert [_fields(x)["part"] for x in a] == [_fields(x)["part"] for x in b]


def test_scratch_stays_below_a_quarter_of_an_mn_vector():
    """At k = 16, for every shape with m, n >= 1024 (16384 x 16384 among them), both sides, the device entry with its
    own mass vector and the host entry with copies of B, Y and w: at most 2*mn bytes, and the header's formula."""
    shapes = [(m, n) for m, n in SHAPES + LARGE + [(1024, 1024), (1024, 16384), (16384, 1024), (1025, 1025)]
              if m >= 1024 and n >= 1024]
    assert (16384, 16384) in shapes and (1024, 1024) in shapes
    for side in (0, 1):
        out = ask(["geo %d %d 16 %d" % (m, n, side) for m, n in shapes])[0]
        for (m, n), line in zip(shapes, out):
            g = _fields(line)
            R = n if side else m
            part = 8 * 5 * (4 * cdiv(m, 256) * n if side else cdiv(n, 64) * m)
            assert g["scratch_dev"] == part + 8 * R
            assert g["scratch_host"] == part + 8 * (16 * (m + n) + R)
            assert max(g["scratch_dev"], g["scratch_host"]) <= 2 * m * n, (m, n, side, line)
