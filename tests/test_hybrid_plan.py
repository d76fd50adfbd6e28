"""The host decisions of the problem-level solvers (csrc/ipd_hybrid_plan.h) on the CPU: a small C++ driver
(tests/hybrid_plan_driver.cpp) is built with the system g++ against the header.  The component bookkeeping and the
route of Hybrid_AMG are checked against the oracle (whose inner solver is replaced by a stub, so no AMG runs), the
sharing rule against a table written from the code it replaced, AMG4POT's scalars against numpy bit for bit.  The
boundary values come from the driver's `limits` line, not from a copy here.  CPU only."""
import atexit
import functools
import itertools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ipd_oracle as O
from tests import problems as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "codes_of_ipd_ssn_amg_method_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def driver_exe():
    d = tempfile.mkdtemp(prefix="hybrid_plan")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "hybrid_plan_driver")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC,
                          os.path.join(HERE, "hybrid_plan_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _fields(line):
    return dict(tok.split("=", 1) for tok in line.split()[1:])


def _ints(v):
    return np.array([] if v == "-" else [int(x) for x in v.split(",")], np.int64)


def ask(queries):
    """The driver's answers to a list of query lines (a dict of strings each), and its limits."""
    res = subprocess.run([driver_exe()], input="\n".join(queries) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = res.stdout.strip().split("\n")
    assert out[0].startswith("limits ") and len(out) == len(queries) + 1, out[:2]
    return [_fields(x) for x in out[1:]], {k: int(v) for k, v in _fields(out[0]).items()}


@functools.lru_cache(maxsize=None)
def limits():
    return ask([])[1]


def roots_of(A):
    """root[i] = the smallest member of i's component (what the device's union-find leaves), from scipy's labels"""
    N = A.shape[0]
    ncomp, lab = sp.csgraph.connected_components(sp.csr_matrix(A), directed=False)
    first = np.full(ncomp, N, np.int64)
    np.minimum.at(first, lab, np.arange(N))
    return first[lab]


def components(root, order=()):
    q = "components %d %d %s" % (len(root), len(order), " ".join(str(int(x)) for x in list(root) + list(order)))
    return ask([q])[0][0]


# ---------------------------------------------------------------------------------------------------------------
# components_from_roots
# ---------------------------------------------------------------------------------------------------------------
def _random_graph(N, dens, seed):   # the graphs of tests/test_gpu_hybrid.py::test_components
    G = sp.random(N, N, dens, random_state=np.random.RandomState(seed), format="csr")
    return sp.csr_matrix(G + G.T + sp.identity(N))


GRAPHS = {
    "n1": lambda: _random_graph(1, 0.0, 0),
    "n60": lambda: _random_graph(60, 0.01, 1),
    "n400": lambda: _random_graph(400, 0.002, 2),
    "n2048": lambda: _random_graph(2048, 0.0006, 3),
    "path": lambda: sp.diags([np.ones(299), np.ones(300), np.ones(299)], [-1, 0, 1], format="csr"),
    "isolated": lambda: sp.identity(37, format="csr"),
}


@pytest.mark.parametrize("name", list(GRAPHS))
def test_components_from_roots_against_the_oracle(name):
    G = GRAPHS[name]()
    got = components(roots_of(G))
    ob, osz, op, orr = O.components(G)
    assert got["err"] == "-" and int(got["ncomp"]) == len(osz)
    assert np.array_equal(_ints(got["blocks"]), ob) and np.array_equal(_ints(got["sizes"]), osz)
    assert np.array_equal(_ints(got["p"]), op) and np.array_equal(_ints(got["r"]), orr)


@pytest.mark.parametrize("name", ["n60", "n400"])
def test_injected_order_is_a_relabelling(name):
    G = GRAPHS[name]()
    root = roots_of(G)
    b, sz, p, r = O.components(G)
    ncomp = len(sz)
    assert ncomp > 3
    order = np.random.RandomState(11).permutation(ncomp)          # new component k is old component order[k]
    smallest = np.array([p[r[k]:r[k + 1]].min() for k in order])
    got = components(root, smallest)
    newid = np.empty(ncomp, np.int64)
    newid[order] = np.arange(ncomp)
    b2 = newid[b]
    assert got["err"] == "-"
    assert np.array_equal(_ints(got["blocks"]), b2) and np.array_equal(_ints(got["sizes"]), sz[order])
    assert np.array_equal(_ints(got["p"]), np.argsort(b2, kind="stable"))
    assert np.array_equal(_ints(got["r"]), np.concatenate([[0], np.cumsum(sz[order])]))


def test_injected_order_rejects():
    G = GRAPHS["n60"]()
    root = roots_of(G)
    b, sz, p, r = O.components(G)
    smallest = np.array([p[r[k]:r[k + 1]].min() for k in range(len(sz))])
    big = int(np.argmax(sz))
    non_root = p[r[big] + 1]                                       # a member of a component, not its smallest
    assert sz[big] > 1 and root[non_root] != non_root
    length = "component_order:_as_many_entries_as_there_are_components_expected"
    entry = "component_order:_entries_must_be_the_smallest_members_of_distinct_components"
    assert components(root, smallest[:-1])["err"] == length
    assert components(root, list(smallest) + [smallest[0]])["err"] == length
    bad = smallest.copy()
    bad[big] = non_root
    assert components(root, bad)["err"] == entry
    rep = smallest.copy()
    rep[1] = rep[0]
    assert components(root, rep)["err"] == entry
    out = smallest.copy()
    out[0] = len(root)
    assert components(root, out)["err"] == entry


def test_a_node_that_points_past_itself_is_rejected():
    assert components([0, 2, 2])["err"] == "components:_a_node_does_not_point_at_the_smallest_member_of_its_tree"
    assert components([0, 0, 1])["err"] == "components:_a_node_does_not_point_at_the_smallest_member_of_its_tree"


# ---------------------------------------------------------------------------------------------------------------
# plan_route against the oracle's Hybrid_AMG
# ---------------------------------------------------------------------------------------------------------------
def _block(Y, r0, c0, nr, nc):
    """A connected bipartite block of exactly nr + nc nodes: a path row - column - row ... through min(nr, nc)
    pairs, the rest of the longer side as leaves."""
    k = min(nr, nc)
    for i in range(k):
        Y[r0 + i, c0 + i] = 1
        if i + 1 < k:
            Y[r0 + i + 1, c0 + i] = 1
    Y[r0 + k:r0 + nr, c0] = 1
    Y[r0, c0 + k:c0 + nc] = 1
    return r0 + nr, c0 + nc


def _system(blocks, t_on=()):
    """blocks: (rows, columns) of the diagonal blocks in label order ((1, 0) / (0, 1): a row / a column with no
    active entry); t_on: the blocks on whose nodes T is one (zero elsewhere)."""
    m, n = sum(b[0] for b in blocks), sum(b[1] for b in blocks)
    Y = np.zeros((m, n), np.uint8)
    t = np.zeros(m + n)
    r0 = c0 = 0
    for k, (nr, nc) in enumerate(blocks):
        if k in t_on:
            t[c0:c0 + nc] = 1.0
            t[n + r0:n + r0 + nr] = 1.0
        if nr and nc:
            _block(Y, r0, c0, nr, nc)
        r0, c0 = r0 + nr, c0 + nc
    s = Y.reshape(-1, order="F").copy()
    pd = PR.make_prob(m, n, s, t=t, pq_random=True)
    pd["H0"] = O.ASAt(s, pd["p"], pd["q"])
    return pd


def mixed_system():
    """Small components first, one of exactly HYBRID_N0 nodes next to one of HYBRID_N0 + 1, singletons, and a second
    large component behind them; dK sums to something on the first large component and to zero on the second."""
    N0 = limits()["HYBRID_N0"]
    assert N0 % 2 == 0
    h = N0 // 2
    return _system([(3, 3), (h, h), (h + 1, h), (0, 1), (1, 0), (70, 60), (2, 1), (1, 0)], t_on=(0, 2))


SYSTEMS = {
    "mixed": mixed_system,
    "mixed_no_T": lambda: _system([(3, 3), (52, 50), (1, 0), (70, 60)]),
    "connected": lambda: _system([(40, 37)]),
    "connected_T": lambda: _system([(40, 37)], t_on=(0,)),
    "connected_beyond_N0": lambda: _system([(80, 90)], t_on=(0,)),
    "all_small": lambda: _system([(3, 3), (0, 1), (50, 50), (1, 0), (20, 31), (1, 1)], t_on=(2,)),
    "two_large_first": lambda: _system([(60, 60), (51, 50), (2, 2)], t_on=(1,)),
}


def route(pd, bigph, dK=None, root=None):
    if root is None:
        root = roots_of(pd["H0"])
    dK = [] if dK is None else [float(x).hex() for x in dK]
    q = "route %d %d %d %d %s" % (pd["n"], int(bigph), len(root), len(dK),
                                  " ".join([str(int(x)) for x in root] + dK))
    f = ask([q])[0][0]
    large = [] if f["large"] == "-" else [dict(zip(("k", "off", "len", "fnode", "mask", "isnsp"),
                                                   map(int, x.split(":")))) for x in f["large"].split(",")]
    return f, large


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_route_against_the_oracle(name):
    pd = SYSTEMS[name]()
    N0 = limits()["HYBRID_N0"]
    M = pd["m"] + pd["n"]
    calls = []

    def stub(A, f, o):
        calls.append((A.shape[0], int(o["fnode"]), int(o["isnsp"])))
        return np.zeros(len(f)), 0, 0.0, None, None

    tr = []
    _, _, _, info = O.Hybrid_AMG(pd, O.amg_options_class2("w"), O.matlab_rng(), N0=N0, trace=tr, solver=stub)
    out = O.build_Ae(pd["H0"], pd["T"], pd["p"], pd["q"], pd["bk1"], pd["tk"])
    dK = out[3].diagonal()
    f, large = route(pd, 1, dK if pd["T"].nnz else None)
    p = _ints(f["p"])
    ob, osz, _, _ = O.components(out[1])
    assert np.array_equal(info, [len(osz), int(f["it_num"])])
    assert int(f["connected"]) == (len(osz) == 1) and int(f["one_sided"]) == -1
    # per Class_AMG call, in visiting order
    assert len(large) == len(tr) == len(calls)
    for c, t_, call in zip(large, tr, calls):
        assert np.array_equal(p[c["off"]:c["off"] + c["len"]], t_["pk"])
        assert (c["len"], c["fnode"], c["isnsp"]) == call == (len(t_["pk"]), t_["fnode"], t_["isnsp"])
    # the small components together
    nodes, boff, local = _ints(f["nodes"]), _ints(f["boff"]), _ints(f["local"])
    if len(osz) == 1:
        assert nodes.size == 0 and np.array_equal(boff, [0])
        return
    small = np.flatnonzero(osz[ob] <= N0)                                # Hybrid_AMG.m:85
    order = np.argsort(ob[small], kind="stable")                          # :86
    assert np.array_equal(nodes, small[order])
    sizes = osz[osz <= N0]
    assert np.array_equal(boff, np.concatenate([[0], np.cumsum(sizes)]))
    assert int(f["maxnb"]) == (sizes.max() if sizes.size else 0)
    for b in range(len(sizes)):                                           # a node's row in its block
        assert np.array_equal(local[nodes[boff[b]:boff[b + 1]]], np.arange(sizes[b]))
    assert int(f["small_lds"]) == 8 * (int(f["maxnb"]) * (int(f["maxnb"]) + 1) + int(f["maxnb"]))


def test_route_of_the_mixed_system_hits_the_boundary():
    """the system the GPU test solves: what the cases are there for"""
    N0 = limits()["HYBRID_N0"]
    pd = mixed_system()
    dK = O.build_Ae(pd["H0"], pd["T"], pd["p"], pd["q"], pd["bk1"], pd["tk"])[3].diagonal()
    f, large = route(pd, 1, dK)
    sizes = np.diff(_ints(f["boff"]))
    assert [c["len"] for c in large] == [N0 + 1, 130] and N0 in sizes and 1 in sizes
    assert [c["isnsp"] for c in large] == [0, 1]
    assert large[0]["k"] > 0 and int(f["it_num"]) == large[-1]["k"] + 1   # small components come first
    assert int(f["maxnb"]) == N0
    assert int(f["small_lds"]) == 8 * (N0 * (N0 + 1) + N0) <= limits()["HYBRID_SMALL_LDS_OPTIN"]


@pytest.mark.parametrize("bigph", [0, 1])
def test_mask_form_boundary(bigph):
    """pure sizes: components of RES_MASK_MIN_ROWS and RES_MASK_MIN_ROWS + 1 nodes, interleaved so that each has both sides"""
    R = limits()["RES_MASK_MIN_ROWS"]
    N, n = 2 * R + 1, R
    root = np.arange(N) % 2                     # even nodes: component 0 (R + 1 of them), odd nodes: component 1 (R)
    f, large = route(dict(n=n), bigph, None, root)
    assert [c["len"] for c in large] == [R + 1, R] and int(f["one_sided"]) == -1
    assert [c["mask"] for c in large] == [bigph, 0]
    assert int(f["gather_qp"]) == bigph
    assert [c["fnode"] for c in large] == [int((np.flatnonzero(root == k) < n).sum()) for k in (0, 1)]
    f, large = route(dict(n=n), bigph, None, root[:-1])   # R and R: neither beyond the bound
    assert [c["len"] for c in large] == [R, R] and [c["mask"] for c in large] == [0, 0] and int(f["gather_qp"]) == 0


def test_connected_offers_the_mask_form_and_takes_no_gather():
    f, large = route(dict(n=3), 1, None, np.zeros(7, np.int64))
    assert int(f["connected"]) == 1 and int(f["it_num"]) == 1 and int(f["gather_qp"]) == 0
    assert large == [dict(k=0, off=0, len=7, fnode=3, mask=1, isnsp=1)]
    assert route(dict(n=3), 0, None, np.zeros(7, np.int64))[1][0]["mask"] == 0


def test_a_large_component_on_one_side_is_reported():
    N0 = limits()["HYBRID_N0"]
    root = np.concatenate([np.zeros(N0 + 1, np.int64), np.full(5, N0 + 1)])
    f, _ = route(dict(n=N0 + 1), 1, None, root)
    assert int(f["one_sided"]) == 0
    f, _ = route(dict(n=N0), 1, None, root)
    assert int(f["one_sided"]) == -1


# ---------------------------------------------------------------------------------------------------------------
# the sharing rule
# ---------------------------------------------------------------------------------------------------------------
# (record, from, count, system), written by hand from csrc/ipd_hybrid.hip of the commit before the rule existed:
#   plain call, hybrid_amg_dev :567-579 -- no StepDonors: no cache at all (:568); with them record_donors = true,
#     use_donors = step->same, shared_count = &step->shared whatever `same` (:573-576); IPD_NO_DONOR is not read.
#   AMG4POT's first solve, amg4pot_dev :871-882 -- IPD_NO_DONOR: no cache (:882); else record_donors = true (:875),
#     and the previous step's donors with the count only under step && same (:876-880); the cache carries Ae and
#     the components to the second solve (:619-622, :766).
#   AMG4POT's second solve :883-887, :899-900 -- IPD_NO_DONOR: no cache; else record_donors = false,
#     use_donors = true with donors = the first solve's hierarchies, shared_count = nullptr.
NONE, PREV, FIRST = "none", "prev_step", "first_solve"
SHARING = {
    # (kind, step, no_donor): step 0 = no StepDonors, 1 = same false, 2 = same true
    (0, 0, 0): (0, NONE, 0, 0), (0, 0, 1): (0, NONE, 0, 0),
    (0, 1, 0): (1, NONE, 1, 0), (0, 1, 1): (1, NONE, 1, 0),
    (0, 2, 0): (1, PREV, 1, 0), (0, 2, 1): (1, PREV, 1, 0),
    (1, 0, 0): (1, NONE, 0, 1), (1, 0, 1): (0, NONE, 0, 0),
    (1, 1, 0): (1, NONE, 0, 1), (1, 1, 1): (0, NONE, 0, 0),
    (1, 2, 0): (1, PREV, 1, 1), (1, 2, 1): (0, NONE, 0, 0),
    (2, 0, 0): (0, FIRST, 0, 1), (2, 0, 1): (0, NONE, 0, 0),
    (2, 1, 0): (0, FIRST, 0, 1), (2, 1, 1): (0, NONE, 0, 0),
    (2, 2, 0): (0, FIRST, 0, 1), (2, 2, 1): (0, NONE, 0, 0),
}


def test_sharing_rule():
    keys = list(itertools.product((0, 1, 2), (0, 1, 2), (0, 1)))
    assert sorted(keys) == sorted(SHARING)
    got, _ = ask(["sharing %d %d %d %d" % (kind, step > 0, step == 2, nd) for kind, step, nd in keys])
    for key, g in zip(keys, got):
        assert (int(g["record"]), g["from"], int(g["count"]), int(g["system"])) == SHARING[key], key


# ---------------------------------------------------------------------------------------------------------------
# AMG4POT's scalars
# ---------------------------------------------------------------------------------------------------------------
def test_pot_scalars_bit_for_bit():
    rs = np.random.RandomState(4)
    rows = []
    for _ in range(300):
        epss, tk = np.float64(10.0 ** rs.uniform(-6, 0)), np.float64(10.0 ** rs.uniform(-4, 1))
        sg = np.float64(1.0) / tk                                          # AMG4POT.m:31
        ssum, vvv = np.float64(rs.uniform(0, 1e4)), np.float64(rs.uniform(0, 10))
        z2, vz1 = np.float64(rs.randn()), np.float64(rs.randn() * 100)
        rows.append((epss, sg, ssum, z2, vvv, vz1))
    got, _ = ask(["pot " + " ".join(float(x).hex() for x in row) for row in rows])
    with np.errstate(all="ignore"):
        for (epss, sg, ssum, z2, vvv, vz1), g in zip(rows, got):
            phi_e = epss + sg * ssum                                       # :33
            want = dict(phi_e=phi_e, w=-(sg / phi_e * z2), tt=sg * sg / (phi_e - sg * sg * vvv),   # :53
                        zeta2=(z2 - sg * vz1) / phi_e)                     # :54
            for k, v in want.items():
                assert float.fromhex(g[k]) == v and float.fromhex(g[k]).hex() == float(v).hex(), (k, g[k], v)
