"""The column-group walk's host-clean geometry header (csrc/ipd_walk_geo.h) on the CPU: a small C++ driver
(tests/walk_geo_driver.cpp) is built with the system g++ against the header.  Over the union of the shapes the plan
products', the dual certificate's and the primal certificate's tests walk -- the ten shapes of tests/test_gpu_round.py,
the shapes of tests/test_apd_geo.py and up to 16384 x 16384 -- it shows that each row and each column has exactly one
owner, that only the last column group can end early, and that every index of the row, column and workgroup layouts
that a walking kernel writes and a finishing kernel reads lies inside the buffer (each entry written exactly once, none
read unwritten).  What the three units add to the walk: tests/test_plan_apply_geo.py, test_dual_geo.py,
test_round_geo.py.  CPU only."""
from tests.geo_driver import ALL, WALK, cdiv, fields


def test_limits():
    assert WALK.limits() == dict(TR=256, TC=16, APD_WAVES=4, WK_CPG=4)


def test_every_row_and_column_has_one_owner():
    out = WALK.ask(["cover %d %d" % s for s in ALL])[0]
    geo = WALK.ask(["geo %d %d" % s for s in ALL])[0]
    T, CPG = WALK.limits()["TC"], WALK.limits()["WK_CPG"]
    for (m, n), line, gl in zip(ALL, out, geo):
        f, g = fields(line), fields(gl)
        assert (f["rmin"], f["rmax"]) == (1, 1), (m, n, line)
        assert (f["min"], f["max"]) == (1, 1), (m, n, line)
        assert f["first"] == 1, (m, n, line)
        # the last group is the only one that can end early, and the groups before it are full
        assert g["ng"] * CPG * T >= n > (g["ng"] - 1) * CPG * T
        assert f["broke"] == (1 if cdiv(n, T) % CPG else 0)
        assert f["idle"] == g["ng"] * CPG - cdiv(n, T)


def test_layouts_are_what_the_kernels_index():
    """ng partials per row, 4*nib per column, one record per workgroup: every entry a finishing kernel reads is
    written exactly once, and the last one is the buffer's last."""
    geo = WALK.ask(["geo %d %d" % s for s in ALL])[0]
    reach = WALK.ask(["reach %d %d" % s for s in ALL])[0]
    for (m, n), gl, rl in zip(ALL, geo, reach):
        g, r = fields(gl), fields(rl)
        assert g["nib"] == cdiv(m, 256) and g["nslot"] == 4 * g["nib"] and g["ng"] == cdiv(n, 64)
        assert g["rows"] == g["ng"] * m and g["cols"] == g["nslot"] * n and g["blocks"] == g["nib"] * g["ng"]
        assert r["outside"] == 0, (m, n, rl)
        for key, size in (("r", g["rows"]), ("c", g["cols"]), ("b", g["blocks"])):
            assert r[key + "len"] == size
            assert r[key + "w"] == r[key + "r"] == size - 1, (m, n, key, rl)
            assert r[key + "unwritten"] == 0 and r[key + "dup"] == 0, (m, n, key, rl)
