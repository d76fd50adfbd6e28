"""The setup's planner (csrc/ipd_setup_plan.h) on the CPU: a small C++ driver (tests/setup_plan_driver.cpp) is
built with the system g++ against the header; every rule is run at its boundary (the boundary values come from
the driver's `limits` line, not from a copy here), and the plans of the level shapes of the nine systems of
tests/test_gpu_setup_at_scale.py are the pinned ones.  CPU only."""
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


@functools.lru_cache(maxsize=None)
def driver_exe():
    d = tempfile.mkdtemp(prefix="setup_plan")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "setup_plan_driver")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC,
                          os.path.join(HERE, "setup_plan_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _fields(line):
    rec = {}
    for tok in line.split()[1:]:
        if "=" in tok:
            k, v = tok.split("=")
            try:
                rec[k] = int(v)
            except ValueError:
                try:
                    rec[k] = float(v)
                except ValueError:
                    rec[k] = v
    return rec


def ask(queries):
    """The driver's answers to a list of query lines, and its limits."""
    res = subprocess.run([driver_exe()], input="\n".join(queries) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = res.stdout.strip().split("\n")
    assert out[0].startswith("limits ") and len(out) == len(queries) + 1, out
    return out[1:], _fields(out[0])


@functools.lru_cache(maxsize=None)
def limits():
    return ask([])[1]


def transfer(level, N, nnz, Nc, hints=(0, 0, 0, 0), bigph=0, fnode=-1, inter=1, sw="-"):
    """The plan of one level's transfer: form, threads, lazy, lazy_prod, rows, the three bounds, mis_small."""
    q = "transfer %s %d %d %d %d %d %d %d %d %d %d %d" % ((sw, level, N, nnz, Nc, bigph, fnode, inter) + tuple(hints))
    return _fields(ask([q])[0][0])


def product(X, Y, lazy=False, x_maxrow=0, sw="-"):
    """The plan of X*Y, X and Y as (rows, columns, entries)."""
    q = "product %s %d %d %d %d %d %d %d %d" % ((sw, int(lazy), x_maxrow) + tuple(X) + tuple(Y))
    return _fields(ask([q])[0][0])


def row_count(lazy, nr, tail):
    return ask(["rowcount %d %d %d" % (int(lazy), nr, int(tail))])[0][0].split()[1]


HINTS = (5, 7, 9, 3)   # any positive counts: the gates only ask whether the last hierarchy left some


# ---------------------------------------------------------------------------------------------------------------
# the row-count ladder
# ---------------------------------------------------------------------------------------------------------------
def test_row_count_table():
    """Every cell: a lazy count is head-scanned while the rows fit the consumer's LDS; else a producer with
    256-thread workgroups scans in its tail and a one-wave producer is followed by a scan launch, the total
    staying on the device (lazy) or going to the host."""
    H = limits()["SCAN_HEAD_MAX"]
    want = {(1, H, 0): "HEAD", (1, H, 1): "HEAD", (1, H + 1, 0): "SCAN_LAZY", (1, H + 1, 1): "TAIL_LAZY",
            (0, H, 0): "SCAN_TOTAL", (0, H, 1): "TAIL_WAIT", (0, H + 1, 0): "SCAN_TOTAL", (0, H + 1, 1): "TAIL_WAIT"}
    for (lazy, nr, tail), mode in want.items():
        assert row_count(lazy, nr, tail) == mode, (lazy, nr, tail)
    assert row_count(1, 1, 0) == "HEAD" and row_count(0, 1, 0) == "SCAN_TOTAL"


# ---------------------------------------------------------------------------------------------------------------
# the transfer, before the split
# ---------------------------------------------------------------------------------------------------------------
def test_mis_small_by_rows_entries_and_switch():
    R, Z = limits()["MIS_SMALL_ROWS"], limits()["MIS_SMALL_NNZ"]
    assert (R, Z) == (1024, 40000)       # the sizes the issue names (tests/test_gpu_setup_at_scale.py MIS_CASES)
    assert transfer(2, R, Z, 10)["mis_small"] == 1
    assert transfer(2, R + 1, Z, 10)["mis_small"] == 0
    assert transfer(2, R, Z + 1, 10)["mis_small"] == 0
    assert transfer(2, R, Z, 10, sw="IPD_NO_MIS_SMALL")["mis_small"] == 0
    assert transfer(2, 1, 1, 1)["mis_small"] == 1 and transfer(2, 0, 0, 0)["mis_small"] == 0


# ---------------------------------------------------------------------------------------------------------------
# the transfer, after the split: the lazy gate
# ---------------------------------------------------------------------------------------------------------------
def test_lazy_at_the_dense_bound():
    """N*Nc equal to SPGEMM_LAZY_MAX and one column more."""
    M = limits()["SPGEMM_LAZY_MAX"]
    N = 2048
    Nc = M // N
    assert N * Nc == M
    p = transfer(2, N, 8 * N, Nc, HINTS)
    assert (p["lazy"], p["lazy_prod"], p["rows"]) == (1, 1, "HEAD")
    assert (p["p_bound"], p["pta_bound"], p["ac_bound"]) == (M, M, Nc * Nc)
    p = transfer(2, N, 8 * N, Nc + 1, HINTS)
    assert (p["lazy"], p["lazy_prod"], p["rows"]) == (0, 0, "SCAN_TOTAL")


def test_lazy_at_the_head_scan_limit():
    """N equal to SCAN_HEAD_MAX and one row more: the bigraph level has the head scan only, a classical level
    goes on to a lazy tail or a lazy scan launch."""
    H, M = limits()["SCAN_HEAD_MAX"], limits()["SPGEMM_LAZY_MAX"]
    Nc = M // (H + 1)
    p = transfer(1, H, 5 * H, Nc, HINTS, bigph=1, fnode=H - Nc)
    assert (p["form"], p["lazy"], p["lazy_prod"], p["rows"]) == ("BIGRAPH", 1, 1, "HEAD")
    assert p["p_bound"] == 5 * H + H     # A's entries and one per C row, below the dense bound
    p = transfer(1, H + 1, 5 * H, Nc, HINTS, bigph=1, fnode=H + 1 - Nc)
    assert (p["form"], p["lazy"], p["lazy_prod"], p["rows"]) == ("BIGRAPH", 0, 1, "TAIL_WAIT")
    p = transfer(2, H, 5 * H, Nc, HINTS)
    assert (p["form"], p["lazy"], p["rows"]) == ("WAVE", 1, "HEAD")
    p = transfer(2, H + 1, 5 * H, Nc, HINTS)
    assert (p["form"], p["lazy"], p["rows"]) == ("WAVE", 1, "SCAN_LAZY")
    p = transfer(2, H + 1, 5 * H, Nc, HINTS, sw="IPD_INTERP=split")
    assert (p["form"], p["lazy"], p["rows"]) == ("SPLIT", 1, "TAIL_LAZY")


@pytest.mark.parametrize("bigph", [0, 1])
def test_lazy_needs_the_hints(bigph):
    """A missing count of P leaves P counted and the products lazy; a missing count of P'A or Ac, or all
    missing, leaves everything counted.  The longest row of P'A is no part of the gate."""
    level, fnode = (1, 600) if bigph else (2, -1)
    def lz(h):
        p = transfer(level, 1000, 5000, 400, h, bigph=bigph, fnode=fnode)
        return p["lazy"], p["lazy_prod"]
    assert lz((5, 7, 9, 0)) == (1, 1)
    assert lz((0, 7, 9, 3)) == (0, 1)
    assert lz((5, 0, 9, 3)) == (0, 0)
    assert lz((5, 7, 0, 3)) == (0, 0)
    assert lz((0, 0, 0, 0)) == (0, 0)


def test_lazy_levels():
    """Hints are kept for levels 1 .. XFER_HINT_LEVELS - 1: level 0 and level 40 count."""
    L = limits()["XFER_HINT_LEVELS"]
    assert L == 40
    for level, want in [(0, 0), (1, 1), (L - 1, 1), (L, 0)]:
        p = transfer(level, 1000, 5000, 400, HINTS)
        assert (p["lazy"], p["lazy_prod"]) == (want, want), level


# ---------------------------------------------------------------------------------------------------------------
# the transfer, after the split: the form
# ---------------------------------------------------------------------------------------------------------------
def test_split_from_256_entries_per_row():
    S = limits()["SPLIT_ROW_MIN"]
    N = 100
    nnz = int(S * N)
    assert nnz / N == 256
    assert transfer(2, N, nnz, 10)["form"] == "SPLIT" and transfer(2, N, nnz, 10)["rows"] == "TAIL_WAIT"
    assert transfer(2, N, nnz - 1, 10)["form"] == "WAVE" and transfer(2, N, nnz - 1, 10)["rows"] == "SCAN_TOTAL"


def test_interp_switch():
    """single and block force the one-kernel forms on long rows, split the product form on short ones; any
    other value is the one-wave kernel."""
    long_, short = (100, 30000, 10), (100, 500, 10)
    assert transfer(2, *long_, sw="IPD_INTERP=single")["form"] == "WAVE"
    assert transfer(2, *long_, sw="IPD_INTERP=block")["form"] == "BLOCK"
    assert transfer(2, *long_, sw="IPD_INTERP=split")["form"] == "SPLIT"
    assert transfer(2, *short, sw="IPD_INTERP=split")["form"] == "SPLIT"
    assert transfer(2, *short, sw="IPD_INTERP=block")["form"] == "BLOCK"
    assert transfer(2, *short, sw="IPD_INTERP=single")["form"] == "WAVE"
    assert transfer(2, *long_, sw="IPD_INTERP=other")["form"] == "WAVE"
    assert transfer(2, *short)["form"] == "WAVE" and transfer(2, *long_)["form"] == "SPLIT"


def test_block_form_is_wide_from_96_entries_per_row():
    W = limits()["WIDE_ROW_MIN"]
    N = 100
    nnz = int(W * N)
    assert nnz / N == 96
    assert transfer(2, N, nnz, 10, sw="IPD_INTERP=block")["threads"] == 256
    assert transfer(2, N, nnz - 1, 10, sw="IPD_INTERP=block")["threads"] == 64


def test_ideal_interpolation():
    """inter = 2 is the ideal interpolation whatever the rows and the switch say; its count launch has a tail."""
    for sw in ["-", "IPD_INTERP=split", "IPD_INTERP=block"]:
        for nnz in [500, 30000]:
            p = transfer(2, 100, nnz, 10, inter=2, sw=sw)
            assert (p["form"], p["rows"]) == ("IDEAL", "TAIL_WAIT")
    assert transfer(2, 100, 500, 10, HINTS, inter=2)["rows"] == "HEAD"
    assert transfer(2, 100, 500, 10, inter=1)["form"] == "WAVE"


def test_bigraph_is_level_1_only():
    assert transfer(1, 1000, 5000, 400, bigph=1, fnode=600)["form"] == "BIGRAPH"
    assert transfer(2, 1000, 5000, 400, bigph=1, fnode=600)["form"] == "WAVE"
    assert transfer(1, 1000, 5000, 400, bigph=0, fnode=600)["form"] == "WAVE"
    assert transfer(1, 1000, 5000, 400, bigph=1, fnode=600, inter=2)["form"] == "BIGRAPH"


# ---------------------------------------------------------------------------------------------------------------
# the product
# ---------------------------------------------------------------------------------------------------------------
def test_product_threads_from_96_entries_per_row_of_y():
    W = limits()["WIDE_ROW_MIN"]
    X = (300, 100, 3000)
    at, below = (100, 200, int(W * 100)), (100, 200, int(W * 100) - 1)
    assert at[2] / at[0] == 96
    assert product(X, at, sw="IPD_PRODUCT=rows")["threads"] == 256
    assert product(X, below, sw="IPD_PRODUCT=rows")["threads"] == 64
    # ... and with them the row kernel's way to its row pointers: the 256-thread kernel scans in its tail
    assert product(X, at, sw="IPD_PRODUCT=rows")["rows"] == "TAIL_WAIT"
    assert product(X, below, sw="IPD_PRODUCT=rows")["rows"] == "SCAN_TOTAL"
    assert product(X, below, sw="IPD_PRODUCT=tiles")["rows"] == "TAIL_WAIT"


def test_product_switch():
    """rows and tiles override the model in both directions; anything else leaves it the choice."""
    sparse = ((1000, 1000, 3000), (1000, 1000, 3000))     # 3 entries per row: the model takes the row kernel
    dense = ((1024, 1024, 1024 * 1024), (1024, 1024, 1024 * 1024))
    assert product(*sparse)["tiles"] == 0 and product(*dense)["tiles"] == 1
    assert product(*sparse)["modelled"] == 1 and product(*dense)["t_tiles"] < product(*dense)["t_rows"]
    assert product(*sparse, sw="IPD_PRODUCT=tiles")["tiles"] == 1
    assert product(*dense, sw="IPD_PRODUCT=rows")["tiles"] == 0
    assert product(*dense, sw="IPD_PRODUCT=rows")["modelled"] == 0
    assert product(*dense, sw="IPD_PRODUCT=other")["tiles"] == 1
    # an empty operand or a dense block above the scratch limit is the row kernel whatever the switch says
    assert product((1000, 1000, 0), sparse[1], sw="IPD_PRODUCT=tiles")["tiles"] == 0
    big = ((40000, 40000, 10 ** 6), (40000, 40000, 10 ** 6))
    assert product(*big)["bytes"] > 12 * 2 ** 30 and product(*big, sw="IPD_PRODUCT=tiles")["tiles"] == 0


def test_tile_edge_at_256_tiles():
    T = limits()["SPGEMM_TILE"]
    X = (16 * T, 512, 50000)
    p = product(X, (512, 16 * T, 50000), sw="IPD_PRODUCT=tiles")
    assert (p["tiles"], p["edge"]) == (1, T)
    p = product(X, (512, 16 * T - T + 1, 50000), sw="IPD_PRODUCT=tiles")     # 16 x 16 tiles still: columns are padded
    assert p["edge"] == T
    p = product(X, (512, 15 * T, 50000), sw="IPD_PRODUCT=tiles")
    assert (p["tiles"], p["edge"]) == (1, T // 2)


def test_lazy_product_at_the_head_scan_limit():
    H = limits()["SCAN_HEAD_MAX"]
    Y = (500, 300, 2000)
    for nr, rows_w, rows_t in [(H, "HEAD", "HEAD"), (H + 1, "SCAN_LAZY", "TAIL_LAZY")]:
        X = (nr, 500, 3 * nr)
        p = product(X, Y, lazy=True, sw="IPD_PRODUCT=rows")
        assert (p["rows"], p["bound"]) == (rows_w, nr * 300)
        assert product(X, Y, lazy=True, sw="IPD_PRODUCT=tiles")["rows"] == rows_t
        assert product(X, Y, lazy=False, sw="IPD_PRODUCT=rows")["rows"] == "SCAN_TOTAL"


def test_product_model_takes_the_longest_row_of_small_products():
    """x_maxrow (the hint's longest row of P'A) replaces the mean row of X while X has at most 2048 rows."""
    Y = (600, 600, 6000)
    a = product((2048, 600, 20480), Y, x_maxrow=500)
    b = product((2048, 600, 20480), Y, x_maxrow=0)
    assert a["t_rows"] == pytest.approx(50 * b["t_rows"], rel=1e-3)
    c = product((2049, 600, 20490), Y, x_maxrow=500)
    assert c["t_rows"] == pytest.approx(b["t_rows"], rel=1e-3)


# ---------------------------------------------------------------------------------------------------------------
# the level shapes of the nine systems of tests/test_gpu_setup_at_scale.py (rows and entries of every level of
# the oracle's hierarchy), each once without hints and once with its own counts as hints.  Expected, per
# transfer, derived by hand from the rules: form, mis_set in one launch, lazy with hints (the products are
# then lazy too), P's row-count mode with hints / without.
#   lazy       N*Nc <= 2^21 and Nc*Nc <= 2^21; the bigraph level also N <= 4096
#   form       level 1: BIGRAPH; nnz/N >= 256: SPLIT; else WAVE
#   mis small  N <= 1024 and nnz <= 40000 (the bigraph level has no mis_set: what the sizes alone say)
#   rows       lazy and N <= 4096: HEAD; counted: TAIL_WAIT behind BIGRAPH and SPLIT, SCAN_TOTAL behind WAVE
# ---------------------------------------------------------------------------------------------------------------
B, S, W = "BIGRAPH", "SPLIT", "WAVE"
EXPECTED = {
    # sizes 2048 1024 177 17 1: level 1 at N*Nc = 2^21 exactly
    "tree1024": [(B, 0, 1, "HEAD", "TAIL_WAIT"), (W, 1, 1, "HEAD", "SCAN_TOTAL"), (W, 1, 1, "HEAD", "SCAN_TOTAL"),
                 (W, 1, 1, "HEAD", "SCAN_TOTAL")],
    # 2049 1024 180 25 1: level 1 one column over the bound
    "tree1024x1025": [(B, 0, 0, "TAIL_WAIT", "TAIL_WAIT"), (W, 1, 1, "HEAD", "SCAN_TOTAL"),
                      (W, 1, 1, "HEAD", "SCAN_TOTAL"), (W, 1, 1, "HEAD", "SCAN_TOTAL")],
    # 2048 1024 292 2, level 2 fully dense (1024 entries per row), level 3 too (292)
    "hub1024": [(B, 0, 1, "HEAD", "TAIL_WAIT"), (S, 0, 1, "HEAD", "TAIL_WAIT"), (S, 0, 1, "HEAD", "TAIL_WAIT")],
    # 2048 1024 16 1, level 2 with 827 entries per row
    "bern1024": [(B, 0, 1, "HEAD", "TAIL_WAIT"), (S, 0, 1, "HEAD", "TAIL_WAIT"), (W, 1, 1, "HEAD", "SCAN_TOTAL")],
    # 4096 2048 357 41 1: level 1 at 2^23; level 3 has 357 entries per row and 127449 entries
    "tree2048": [(B, 0, 0, "TAIL_WAIT", "TAIL_WAIT"), (W, 0, 1, "HEAD", "SCAN_TOTAL"), (S, 0, 1, "HEAD", "TAIL_WAIT"),
                 (W, 1, 1, "HEAD", "SCAN_TOTAL")],
    # 4097 2048 350 48 1
    "tree2048x2049": [(B, 0, 0, "TAIL_WAIT", "TAIL_WAIT"), (W, 0, 1, "HEAD", "SCAN_TOTAL"),
                      (S, 0, 1, "HEAD", "TAIL_WAIT"), (W, 1, 1, "HEAD", "SCAN_TOTAL")],
    # 4096 2048 65 4, level 2 with 380 entries per row
    "bern2048": [(B, 0, 0, "TAIL_WAIT", "TAIL_WAIT"), (S, 0, 1, "HEAD", "TAIL_WAIT"), (W, 1, 1, "HEAD", "SCAN_TOTAL")],
    # 8192 4096 720 100 1: level 2 at 4096 x 720 = 1.4 * 2^21, level 3 with 720 entries per row
    "tree4096": [(B, 0, 0, "TAIL_WAIT", "TAIL_WAIT"), (W, 0, 0, "SCAN_TOTAL", "SCAN_TOTAL"),
                 (S, 0, 1, "HEAD", "TAIL_WAIT"), (W, 1, 1, "HEAD", "SCAN_TOTAL")],
    # 2539 1272 413 138 49 18 5: level 1 at 2539 x 1272 = 1.5 * 2^21
    "comp2048": [(B, 0, 0, "TAIL_WAIT", "TAIL_WAIT"), (W, 0, 1, "HEAD", "SCAN_TOTAL")] +
                [(W, 1, 1, "HEAD", "SCAN_TOTAL")] * 4,
}


def system_plans(name, with_hints):
    """The transfer plans of every level of system `name`'s oracle hierarchy (isnsp = 1), its own counts of P,
    P'A and Ac as the hints or none."""
    from tests import test_gpu_setup_at_scale as AS
    ho = AS.oracle_hierarchy_cpu(name)
    sizes, nnz = ho.level_sizes(), ho.level_nnz()
    fnode = AS.system(name)[1]
    plans = []
    for k in range(1, ho.J):
        hints = (0, 0, 0, 0)
        if with_hints:
            P, A = ho.Prok[k + 1], ho.Ack[k]
            T1 = P.T @ A
            hints = (P.nnz, T1.nnz, ho.Ack[k + 1].nnz, int(max(T1.tocsr().getnnz(axis=1))))
        plans.append(transfer(k, sizes[k - 1], nnz[k - 1], sizes[k], hints, bigph=1, fnode=fnode))
    return plans


@pytest.mark.parametrize("name", list(EXPECTED))
def test_plans_of_the_at_scale_systems(name):
    want = EXPECTED[name]
    hinted, counted = system_plans(name, True), system_plans(name, False)
    assert len(hinted) == len(counted) == len(want)
    for k, (form, small, lazy, rows_hinted, rows_counted) in enumerate(want, 1):
        h, c = hinted[k - 1], counted[k - 1]
        assert (h["form"], h["mis_small"], h["lazy"], h["lazy_prod"], h["rows"]) == \
               (form, small, lazy, lazy, rows_hinted), (name, k, h)
        assert (c["form"], c["mis_small"], c["lazy"], c["lazy_prod"], c["rows"]) == \
               (form, small, 0, 0, rows_counted), (name, k, c)
