"""The primal certificate's host-clean geometry header (csrc/ipd_round_geo.h) on the CPU: a small C++ driver
(tests/round_geo_driver.cpp) is built with the system g++ against the header.  Over the ten shapes of
tests/test_gpu_round.py, the shapes of tests/test_apd_geo.py and up to 16384 x 16384 it shows that every scalar index
the walking kernel writes and the last kernel reads lies inside the buffer (each entry written exactly once, none read
unwritten), and that the scratch of a call stays below mn/2 bytes -- a sixteenth of one mn vector -- from m = n = 1024
on.  The walk of the rows and columns and the row and column partials are tests/test_walk_geo.py's, over the same
shapes.  CPU only."""
from tests.geo_driver import ALL, WALK, GeoDriver, cdiv, fields as _fields

DRV = GeoDriver("round_geo_driver")
ask, limits = DRV.ask, DRV.limits


def test_limits():
    assert limits() == dict(TR=256, TC=16, APD_WAVES=4, WK_CPG=4, RD_NS=2, RD_NVEC=4, RD_SCAL_PASSES=3,
                            RD_RESULT_DOUBLES=24)


def test_buffer_sizes_are_what_the_kernels_index():
    """ng partials per row, 4*nib per column (the walk's layouts, tests/test_walk_geo.py), RD_NS scalars per
    workgroup: every entry the last kernel reads is written exactly once, and the last one is the buffer's last."""
    geo = ask(["geo %d %d" % s for s in ALL])[0]
    reach = ask(["reach %d %d" % s for s in ALL])[0]
    for (m, n), gl, rl in zip(ALL, geo, reach):
        g, r = _fields(gl), _fields(rl)
        assert g["nib"] == cdiv(m, 256) and g["nslot"] == 4 * g["nib"] and g["ng"] == cdiv(n, 64)
        assert g["rows"] == g["ng"] * m and g["cols"] == g["nslot"] * n
        assert g["blocks"] == g["nib"] * g["ng"] and g["scal"] == 2 * g["blocks"]
        assert r["outside"] == 0, (m, n, rl)
        assert r["slen"] == g["scal"] and r["sw"] == r["sr"] == g["scal"] - 1, (m, n, rl)
        assert r["sunwritten"] == 0 and r["sdup"] == 0, (m, n, rl)


def test_the_two_shapes_beyond_the_plan_tests():
    """65 x 150: three column groups of 4, 4 and 2 chunks, the last chunk with 6 columns; 300 x 16: a second row
    block whose first wave is partly filled (rows 256 .. 299) and whose other three have no rows."""
    g = _fields(ask(["geo 65 150"])[0][0])
    f = _fields(WALK.ask(["cover 65 150"])[0][0])
    assert (g["nib"], g["ng"], g["nslot"], g["blocks"]) == (1, 3, 4, 3)
    assert (f["broke"], f["idle"]) == (1, 2) and 150 - 9 * 16 == 6
    g = _fields(ask(["geo 300 16"])[0][0])
    assert (g["nib"], g["ng"], g["nslot"], g["blocks"]) == (2, 1, 8, 2)


def test_scratch_stays_below_a_sixteenth_of_an_mn_vector():
    """The header's formula, and below mn/2 bytes, for every shape with m, n >= 1024 (1024 x 1024 and
    16384 x 16384 among them)."""
    shapes = [(m, n) for m, n in ALL + [(1024, 1024), (1024, 16384), (16384, 1024), (1025, 1025)]
              if m >= 1024 and n >= 1024]
    assert (16384, 16384) in shapes and (1024, 1024) in shapes
    out = ask(["geo %d %d" % s for s in shapes])[0]
    for (m, n), line in zip(shapes, out):
        g = _fields(line)
        want = 8 * (cdiv(n, 64) * m + 4 * cdiv(m, 256) * n + 3 * 2 * cdiv(m, 256) * cdiv(n, 64) + 4 * (m + n) + 24)
        assert g["scratch"] == want, (m, n, line)
        assert g["scratch"] < m * n // 2, (m, n, line)
