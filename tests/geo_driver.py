"""What the CPU tests of the column-group walk's geometry headers share (tests/test_walk_geo.py and, on top of it,
tests/test_plan_apply_geo.py, test_dual_geo.py, test_round_geo.py): the shapes, and a small C++ driver per header that
is built once with the system g++ and asked one query per line."""
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
SHAPES = [(300, 147), (65, 40), (257, 500), (1, 1), (1, 17), (256, 16), (257, 15), (64, 128), (65, 129), (70, 8211),
          (300, 4099), (1793, 17), (10900, 17), (512, 255), (512, 256), (512, 257), (3, 2049)]
LARGE = [(4096, 4096), (8192, 4096), (16384, 16384), (1793, 16353), (1793, 16337), (16384, 1), (1, 16384)]
ALL = GPU_SHAPES + [s for s in SHAPES if s not in GPU_SHAPES] + LARGE   # the union of what the three units' tests walk


def cdiv(a, b):
    return -(-a // b)


def fields(line):
    return {k: int(v) for k, v in (tok.split("=") for tok in line.split()[1:] if "=" in tok)}


class GeoDriver:
    """tests/<name>.cpp, built against the headers of csrc with -Wall -Werror"""

    def __init__(self, name):
        self.name = name

    @functools.lru_cache(maxsize=None)
    def exe(self):
        d = tempfile.mkdtemp(prefix=self.name)
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, self.name)
        res = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, "-I" + HERE,
                              os.path.join(HERE, self.name + ".cpp"), "-o", exe], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        return exe

    def ask(self, queries):
        """the answers, one per query, and the fields of the limits line the driver prints first"""
        res = subprocess.run([self.exe()], input="\n".join(queries) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        out = res.stdout.strip().split("\n")
        assert out[0].startswith("limits ") and len(out) == len(queries) + 1, out
        return out[1:], fields(out[0])

    @functools.lru_cache(maxsize=None)
    def limits(self):
        return self.ask([])[1]


WALK = GeoDriver("walk_geo_driver")
