"""The dual certificate's host-clean geometry header (csrc/ipd_dual_geo.h) on the CPU: a small C++ driver
(tests/dual_geo_driver.cpp) is built with the system g++ against the header.  Over the shapes of tests/test_apd_geo.py
and up to 16384 x 16384 it shows that every partial index the walking kernels write and the finishing kernels read
lies inside the buffers (each read entry written exactly once), and that the scratch of a call stays at or below mn/2
bytes -- a sixteenth of one mn vector -- from m = n = 1024 on.  The walk of the rows and columns itself is
tests/test_walk_geo.py's.  The two shapes tests/test_gpu_dual.py adds to the plan tests' are pinned.  CPU only."""
import pytest

from tests.geo_driver import LARGE, SHAPES, WALK, GeoDriver, cdiv, fields as _fields

DRV = GeoDriver("dual_geo_driver")
ask, limits = DRV.ask, DRV.limits


def test_limits():
    assert limits() == dict(TR=256, TC=16, APD_WAVES=4, WK_CPG=4, EVALPART=40)


def test_refused_arguments():
    out = ask(["geo 5 5 2", "geo 5 5 -1", "reach 5 5 3", "geo 5 5 1"])[0]
    assert out[:3] == ["geo refused", "geo refused", "reach refused"] and out[3].startswith("geo nib=")


def test_the_two_added_gpu_shapes():
    """65 x 150: three column groups of 4, 4 and 2 chunks, the last chunk with 6 columns; 300 x 16: a second row
    block whose first wave is partly filled (rows 256 .. 299) and whose other three have no rows."""
    g = _fields(ask(["geo 65 150 0"])[0][0])
    f = _fields(WALK.ask(["cover 65 150"])[0][0])
    assert (g["nib"], g["ng"], g["nslot"], g["blocks"]) == (1, 3, 4, 3)
    assert (f["broke"], f["idle"]) == (1, 2) and 150 - 9 * 16 == 6
    g = _fields(ask(["geo 300 16 1"])[0][0])
    assert (g["nib"], g["ng"], g["nslot"], g["S"], g["blocks"]) == (2, 1, 8, 8, 2)
    assert 256 < 300 < 256 + 64


@pytest.mark.parametrize("side", [0, 1])
def test_buffer_sizes_are_what_the_kernels_index(side):
    """Side 0: ng partials per row, side 1: 4*nib per column; every entry the finishing kernel reads is written
    exactly once and the last one is the buffer's last.  The evaluation: one partial per workgroup."""
    shapes = SHAPES + LARGE
    geo = ask(["geo %d %d %d" % (m, n, side) for m, n in shapes])[0]
    reach = ask(["reach %d %d %d" % (m, n, side) for m, n in shapes])[0]
    for (m, n), gl, rl in zip(shapes, geo, reach):
        g, r = _fields(gl), _fields(rl)
        assert g["nib"] == cdiv(m, limits()["TR"]) and g["nslot"] == 4 * g["nib"]
        assert (g["R"], g["S"]) == ((n, g["nslot"]) if side else (m, g["ng"]))
        assert g["stride"] == g["R"] and g["part"] == g["S"] * g["R"], gl
        assert r["len"] == g["part"] and r["outside"] == 0
        assert r["wmax"] == r["rmax"] == g["part"] - 1, (m, n, rl)
        assert r["unwritten"] == 0 and r["dup"] == 0, (m, n, rl)
        assert r["elen"] == g["blocks"] == g["nib"] * g["ng"]
        assert r["ewmax"] == r["ermax"] == g["blocks"] - 1 and r["eunwritten"] == 0 and r["edup"] == 0, (m, n, rl)


def test_scratch_stays_below_a_sixteenth_of_an_mn_vector():
    """Class 2 (L = m + n + 1), both sides, the device entry with its own lam_out and the host entry with copies of
    lam, lam_out and arg, for every shape with m, n >= 1024 (16384 x 16384 among them): the header's formula, and at
    most mn/2 bytes."""
    shapes = [(m, n) for m, n in SHAPES + LARGE + [(1024, 1024), (1024, 16384), (16384, 1024), (1025, 1025)]
              if m >= 1024 and n >= 1024]
    assert (16384, 16384) in shapes and (1024, 1024) in shapes
    for side in (0, 1):
        out = ask(["geo %d %d %d" % (m, n, side) for m, n in shapes])[0]
        for (m, n), line in zip(shapes, out):
            g = _fields(line)
            R, L = (n if side else m), m + n + 1
            part = 12 * (4 * cdiv(m, 256) * n if side else cdiv(n, 64) * m)
            fixed = 40 * cdiv(m, 256) * cdiv(n, 64) + 128
            assert g["scratch_dev"] == part + fixed + 8 * L
            assert g["scratch_host"] == part + fixed + 16 * L + 4 * R
            assert max(g["scratch_dev"], g["scratch_host"]) <= m * n // 2, (m, n, side, line)
