"""The north-west correction's host-clean geometry header (csrc/ipd_round_nw_geo.h) on the CPU: a small C++ driver
(tests/round_nw_geo_driver.cpp) is built with the system g++ against the header.  Over the shapes of
tests/test_gpu_round_nw.py, the shapes of tests/test_apd_geo.py and up to 16384 x 16384 it shows that the scan writes
every prefix exactly once and the merge reads none outside the buffer, that one thread per chunk of one workgroup
reaches every chunk, that the slot of every (k, s) lies in [0, m + n - 2], that the scan marks and the last kernel's
threads own every slot exactly once, and what a side and the workspace take.  CPU only."""
from tests.geo_driver import ALL, GeoDriver, cdiv, fields as _fields

DRV = GeoDriver("round_nw_geo_driver")
ask, limits = DRV.ask, DRV.limits
SHAPES = ALL + [(1000, 90), (90, 1000), (64, 64), (16384, 16383)]


def test_limits():
    assert limits() == dict(NW_CHUNK=64, NW_THREADS=256, NW_MAX_LEN=16384, NW_INFO_DOUBLES=8, NW_DEV_DOUBLES=8)


def test_sizes():
    out = ask(["geo %d %d" % s for s in SHAPES])[0]
    for (m, n), line in zip(SHAPES, out):
        g = _fields(line)
        assert (g["chm"], g["chn"]) == (cdiv(m, 64), cdiv(n, 64)) and max(g["chm"], g["chn"]) <= 256, (m, n, line)
        assert g["pre"] == m + n + 2 and g["slots"] == m + n - 1 and g["cap"] == m + n
        assert g["span"] == cdiv(m + n - 1, 256) and g["span"] * 256 >= g["slots"]
        M = m + n
        assert g["scratch"] == 8 * (M + 2 + 5 * M + 16) + 4 * 2 * M, (m, n, line)
        assert g["workspace"] == 4 * M + 2 * M * 16, (m, n, line)
        if m >= 1024 and n >= 1024:       # beside the mn/2 bytes of the rounding's own scratch: (m+n)-sized
            assert g["scratch"] < m * n // 16


def test_every_index_lies_inside_and_is_written_once():
    out = ask(["reach %d %d" % s for s in SHAPES])[0]
    for (m, n), line in zip(SHAPES, out):
        r = _fields(line)
        assert r["outside"] == 0, (m, n, line)
        assert r["plen"] == m + n + 2 and r["pw"] == r["pr"] == m + n + 1, (m, n, line)
        assert r["punwritten"] == 0 and r["pdup"] == 0, (m, n, line)
        assert r["slen"] == m + n and r["sw"] == m + n - 2 and r["sdup"] == 0, (m, n, line)
        assert (r["slotmin"], r["slotmax"]) == (0, m + n - 2), (m, n, line)
        assert r["owned"] == m + n - 1 and r["owndup"] == 0, (m, n, line)
        assert r["chunkmax"] == cdiv(max(m, n), 64) - 1 <= 255, (m, n, line)
