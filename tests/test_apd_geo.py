"""The tile walker's host-clean geometry header (csrc/ipd_apd_geo.h) on the CPU: a small C++ driver
(tests/apd_geo_driver.cpp) is built with the system g++ against the header.  It pins the natural rule for the
number of column chunks a wave takes (`reps`) at its thresholds, shows that for the natural and every forced
`reps` each column belongs to exactly one (column group, chunk, column-in-chunk), and that the partial-sum buffers a
workspace allocates have the sizes the epilogues index.  tests/test_gpu_driver_passes.py runs `reps` > 1 only
through the switch IPD_APD_REPS (a natural `reps` > 1 needs about 1.2 GB): this file ties that forced geometry to
the natural one -- both come out of the same make_geo, walked by the same loop.  CPU only."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "codes_of_ipd_ssn_amg_method_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))

# tests/test_gpu_driver_passes.py's group f and shapes around the tile, chunk and group boundaries
SHAPES = [(300, 147), (65, 40), (257, 500), (1, 1), (1, 17), (256, 16), (257, 15), (64, 128), (65, 129), (70, 8211),
          (300, 4099), (1793, 17), (10900, 17), (512, 255), (512, 256), (512, 257), (3, 2049)]
LARGE = [(4096, 4096), (8192, 4096), (16384, 16384), (1793, 16353), (1793, 16337), (16384, 1), (1, 16384)]


@functools.lru_cache(maxsize=None)
def driver_exe():
    d = tempfile.mkdtemp(prefix="apd_geo")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "apd_geo_driver")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC,
                          os.path.join(HERE, "apd_geo_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _fields(line):
    return {k: int(v) for k, v in (tok.split("=") for tok in line.split()[1:] if "=" in tok)}


def ask(queries):
    res = subprocess.run([driver_exe()], input="\n".join(queries) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = res.stdout.strip().split("\n")
    assert out[0].startswith("limits ") and len(out) == len(queries) + 1, out
    return out[1:], _fields(out[0])


@functools.lru_cache(maxsize=None)
def limits():
    return ask([])[1]


def cdiv(a, b):
    return -(-a // b)


def test_limits():
    assert limits() == dict(TR=256, TC=16, APD_WAVES=4, APD_REPS_MAX=8)


def test_natural_rule_at_its_thresholds():
    """reps doubles while nib * cdiv(njb, 2*reps) >= 4096: the first shape with reps 2 at m = 1793 (nib = 8) has
    n = 16353 (njb = 1023, 8 * 512 = 4096); one chunk of columns fewer stays at 1."""
    want = {(4096, 4096): 1, (8192, 4096): 2, (16384, 16384): 8, (1793, 16353): 2, (1793, 16337): 1}
    out = ask(["geo %d %d -" % s for s in want])[0]
    assert {s: _fields(l)["reps"] for s, l in zip(want, out)} == want
    # below it nothing the suite, the benchmark or a recorded run uses leaves reps = 1
    small = ask(["geo %d %d -" % s for s in SHAPES])[0]
    assert all(_fields(l)["reps"] == 1 for l in small)


def test_switch_values():
    out = ask(["switch %s" % v for v in ("-", "1", "2", "4", "8", "0", "3", "16", "-2", "2x", "x")])[0]
    assert [int(l.split()[1]) for l in out] == [0, 1, 2, 4, 8, -1, -1, -1, -1, -1, -1]
    assert ask(["geo 5 5 3"])[0] == ["geo refused"]


@pytest.mark.parametrize("sw", ["-", "1", "2", "4", "8"])
def test_every_column_has_one_owner(sw):
    shapes = SHAPES + LARGE
    out = ask(["cover %d %d %s" % (m, n, sw) for m, n in shapes])[0]
    T = limits()["TC"]
    for (m, n), line in zip(shapes, out):
        f = _fields(line)
        assert (f["min"], f["max"]) == (1, 1), (m, n, line)
        if sw != "-":
            assert f["reps"] == int(sw)
        # the last group is the only one that can end early, and the groups before it are full
        assert f["njg"] * f["reps"] * T >= n > (f["njg"] - 1) * f["reps"] * T
        assert f["broke"] == (1 if cdiv(n, T) % f["reps"] else 0)
        assert f["idle"] == f["njg"] * f["reps"] - cdiv(n, T)


def test_group_f_reaches_a_partly_filled_group_and_an_idle_chunk():
    """The forced shapes of the GPU test: (300, 147) has 10 chunks, (65, 40) has 3, (257, 500) has 32 with 4 columns in
    the last."""
    got = {}
    for m, n in [(300, 147), (65, 40), (257, 500)]:
        for r in (2, 4, 8):
            f = _fields(ask(["cover %d %d %d" % (m, n, r)])[0][0])
            got[(m, n, r)] = (f["njg"], f["idle"])
    assert got == {(300, 147, 2): (5, 0), (300, 147, 4): (3, 2), (300, 147, 8): (2, 6),
                   (65, 40, 2): (2, 1), (65, 40, 4): (1, 1), (65, 40, 8): (1, 5),
                   (257, 500, 2): (16, 0), (257, 500, 4): (8, 0), (257, 500, 8): (4, 0)}


@pytest.mark.parametrize("sw", ["-", "1", "2", "4", "8"])
def test_buffer_sizes_are_what_the_epilogues_index(sw):
    """spart holds nib*njg blocks (scal_total walks nblk of them), lpart njg rows of m (ax_entry: njg partials at
    stride m), rpart 4*nib rows of n (4*nib partials at stride n)."""
    shapes = SHAPES + LARGE
    out = ask(["geo %d %d %s" % (m, n, sw) for m, n in shapes])[0]
    for (m, n), line in zip(shapes, out):
        f = _fields(line)
        assert f["nib"] == cdiv(m, limits()["TR"])
        assert f["nblk"] == f["nib"] * f["njg"], line
        assert f["lpart"] == f["njg"] * m, line
        assert f["rpart"] == 4 * f["nib"] * n, line
