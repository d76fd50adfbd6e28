"""The primal certificate's host-clean geometry header (csrc/ipd_round_geo.h) on the CPU: a small C++ driver
(tests/round_geo_driver.cpp) is built with the system g++ against the header.  Over the ten shapes of
tests/test_gpu_round.py, the shapes of tests/test_apd_geo.py and up to 16384 x 16384 it shows that each row and each
column has exactly one owner, that every partial index the walking kernel writes and the finishing and last kernels
read lies inside the buffers (each entry written exactly once, none read unwritten), and that the scratch of a call
stays below mn/2 bytes -- a sixteenth of one mn vector -- from m = n = 1024 on.  CPU only."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "codes_of_ipd_ssn_amg_method_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))

# tests/test_gpu_round.py's shapes, re-stated
GPU_SHAPES = [(1, 1), (1, 37), (37, 1), (63, 17), (64, 16), (65, 33), (257, 19), (600, 45), (65, 150), (300, 16)]
# tests/test_apd_geo.py's shapes, re-stated
SHAPES = [(300, 147), (65, 40), (257, 500), (1, 17), (256, 16), (257, 15), (64, 128), (65, 129), (70, 8211),
          (300, 4099), (1793, 17), (10900, 17), (512, 255), (512, 256), (512, 257), (3, 2049)]
LARGE = [(4096, 4096), (8192, 4096), (16384, 16384), (1793, 16353), (1793, 16337), (16384, 1), (1, 16384)]
ALL = GPU_SHAPES + SHAPES + LARGE


@functools.lru_cache(maxsize=None)
def driver_exe():
    d = tempfile.mkdtemp(prefix="round_geo")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "round_geo_driver")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC,
                          os.path.join(HERE, "round_geo_driver.cpp"), "-o", exe], capture_output=True, text=True)
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
    assert limits() == dict(TR=256, TC=16, APD_WAVES=4, RD_CPG=4, RD_NS=2, RD_NVEC=4, RD_SCAL_PASSES=3,
                            RD_RESULT_DOUBLES=24)


def test_every_row_and_column_has_one_owner():
    out = ask(["cover %d %d" % s for s in ALL])[0]
    geo = ask(["geo %d %d" % s for s in ALL])[0]
    T, CPG = limits()["TC"], limits()["RD_CPG"]
    for (m, n), line, gl in zip(ALL, out, geo):
        f, g = _fields(line), _fields(gl)
        assert (f["rmin"], f["rmax"]) == (1, 1), (m, n, line)
        assert (f["min"], f["max"]) == (1, 1), (m, n, line)
        # the last group is the only one that can end early, and the groups before it are full
        assert g["ng"] * CPG * T >= n > (g["ng"] - 1) * CPG * T
        assert f["broke"] == (1 if cdiv(n, T) % CPG else 0)
        assert f["idle"] == g["ng"] * CPG - cdiv(n, T)


def test_buffer_sizes_are_what_the_kernels_index():
    """ng partials per row, 4*nib per column, RD_NS scalars per workgroup: every entry the finishing and the last
    kernel read is written exactly once, and the last one is the buffer's last."""
    geo = ask(["geo %d %d" % s for s in ALL])[0]
    reach = ask(["reach %d %d" % s for s in ALL])[0]
    for (m, n), gl, rl in zip(ALL, geo, reach):
        g, r = _fields(gl), _fields(rl)
        assert g["nib"] == cdiv(m, 256) and g["nslot"] == 4 * g["nib"] and g["ng"] == cdiv(n, 64)
        assert g["rows"] == g["ng"] * m and g["cols"] == g["nslot"] * n
        assert g["blocks"] == g["nib"] * g["ng"] and g["scal"] == 2 * g["blocks"]
        assert r["outside"] == 0, (m, n, rl)
        for key, size in (("r", g["rows"]), ("c", g["cols"]), ("s", g["scal"])):
            assert r[key + "len"] == size
            assert r[key + "w"] == r[key + "r"] == size - 1, (m, n, key, rl)
            assert r[key + "unwritten"] == 0 and r[key + "dup"] == 0, (m, n, key, rl)


def test_the_two_shapes_beyond_the_plan_tests():
    """65 x 150: three column groups of 4, 4 and 2 chunks, the last chunk with 6 columns; 300 x 16: a second row
    block whose first wave is partly filled (rows 256 .. 299) and whose other three have no rows."""
    g = _fields(ask(["geo 65 150"])[0][0])
    f = _fields(ask(["cover 65 150"])[0][0])
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
