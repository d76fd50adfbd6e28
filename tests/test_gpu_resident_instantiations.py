"""Every instantiation of the level-resident kernels that run_resident (csrc/ipd_resident_host.h) can launch, each
reached on purpose and checked against the oracle.

The row width is a template parameter, so each width is separate machine code: k_resident<KE1,KE2,KE3,POLY2>
(csrc/ipd_resident.h) in ten forms and k_resident_big<KE2,RPW,DEEP> (csrc/ipd_resident_big.h) in four.  A lane
holds the entries lane + 64 q, q < KE, of a padded row (res_load_slice), so the top slot q = KE - 1 carries
real entries only on rows longer than 64 (KE - 1).  plan_resident picks KE as the smallest power of two with
64 KE >= max(S1, S2) (S: the longest off-diagonal row of a level, rounded up to 4), KE3 = 4 for S3 <= 256 and 8
above, or 1 in polynomial form; the mask-form kernel takes KE2 = 16 / 32 (d2.S <= 1024) and, in deep mode,
4 / 8 (d2.S <= 256).  CASES lists one entry per instantiation, and more where the tail differs: a local tail
(J == tail root) and a remote tail workgroup rooted at level 3, 4 and 5 (POLY4).  Per case:

  reach       mode 2, the exact kernel name, (levels, tail root), J, level_forms, no time-out.  Never skipped.
  fill        a resident row reaches the top lane slot of the width under test (S > 64 (KE - 1)), or the
              case records that it does not (`fills`), see below.
  whole solve _against_oracle (level sizes and nnz, cycle count, histories within the oracle's own one-ulp
              sensitivity), at least 4 cycles with oracle rel_res > 1e-9 where the case can have them.
  K cycles    K = 1, 2 loop bodies (bench_cycles) from a guess whose residual is 1e3 |f|, against oracle_cycles:
              |A (x_K - x_K^o)| <= bar = max(4 sens, 1e-12 |f|), sens the same quantity for the oracle run on f
              perturbed by one ulp, and bar <= 1e-3 |f - A x_K^o|, so that the bar is far below what a cycle
              changes.

Where a case does not fill the top slot.  The remote tail rooted at 3 (k_resident<4,4,0> under
IPD_NO_RESIDENT_THREE) needs an LDS image of levels 3..J, and the tail rooted at 5 (POLY4) a sixth level.  In the
search a level-1 or level-2 row longer than 192 entries comes from a hub column, and the hub makes level 3 dense
(a hub of 200 rows: ~177 rows of ~176 entries, beyond any image) in a five-level hierarchy.  These tails are
reached on captured Newton systems, whose level-1 and level-2 rows have at most 14 entries; the other cases of
the same instantiation fill its width.  KE3's top slot: level 3 is resident only with max(S1, S2) <= 512
(three_fits).  In the search, level 3 has at most N1 / 11 rows on tree masks (N1 <= 2048), and on hub masks,
whose level 3 is denser (N1 / 6), S1 is the hub's row count, so the cap of 512 leaves at most 165 rows.  The
longest level-3 row taken in three mode is 179 entries (treehub490), short of the 193 that slot 3 of KE3 = 4
needs; each three-mode case asserts its own (`s3`).

<4,4,8> and <8,8,8> need S3 > 256, a level 3 of at least 258 rows.  The gates admit S3 <= 512, but the
coarsening above keeps S3 at 179 or less.  test_three_mode_s3_search prints the largest S3 it finds among the
hierarchies taken in three mode.  The two table entries are strict xfails: they assert that the planner picks
the form, so they turn red the day it does.

K cycles: the bar is 4 sens rather than 2 sens.  With dense level-2 rows of 1023 entries (bern1024-local) the
device's summation order moves A x_1 by 2.6 sens; every other case stays within 1.1 sens.  The guess's error is
1e3 |f|: the oracle's sensitivity comes from x*, not from the error, so a large error keeps bar <= 1e-3 |f - A x_K|
for K = 2 on the fast dense systems as well.

Mutation power.  Each mutation was made by hand on a scratch copy of the kernels.  This file and the parent's
resident tests (test_gpu_bench_workload, _resident_big, _resident_deep, _resident_remote, _resident_handoff,
_poly_operators, _cycle) then ran against it.  Failing cases are named by instantiation and case id; every one
failed in the whole solve and in the K cycles unless marked (K).
  (a) res_load_slice treats slot KE - 1 as empty, one width at a time (if constexpr):
      KE = 4:  <4,4,0> bern256-local, <4,4,1> and <4,4,4> treehub230-remote4, <4,4,4> hub256-local,
               <4,2,true> treehub1200-deep.  Parent: caught (test_resident_matches_multilaunch[256-256-1.0-1-w]).
      KE = 8:  <8,8,0> bern512-local, <8,8,1> and <8,8,4> treehub490-remote4, <8,8,4> hub512-local,
               <8,2,true> treehub1200-deep.  Parent: caught (test_resident_matches_multilaunch[512-512-1.0-1-v]).
      KE = 16: <16,16,0> bern1024-local, <16,1,false> bern1024-forced-local.  Parent: caught
               (test_metric_workload_against_oracle[v]).
      KE = 32: <32,1,false> bern2000x256-local.  Parent: missed.
  (b) one sweep fewer at the tail.  Local tail: its PCG stops one iteration early (the iterate before the
      last): <4,4,4> hub256-local, <8,8,4> hub512-local.  Parent: missed.  Remote tail: one pre-sweep fewer on
      the sub-cycle's root level in the LDS block path (blk_cycle): <4,4,0> newton1024k31-remote3.  Parent:
      caught (test_realistic_modes_against_the_oracle[k10-long-level3-v]).  The same change in sol_cycle's
      sweep loop fails nothing here or in the parent: every remote root of the table runs in blk_cycle.
  (c) the remote tail's returned correction (P e or e of its root) scaled by 1 + 1e-6: <4,4,0> newton1024k31-remote3,
      <8,8,1> and <8,8,4> treehub490-remote4; (K) <4,4,1> and <4,4,4> treehub230-remote4, both <4,2,true> cases,
      <8,2,true>.  Not failed: <4,4,1> newton1024k21-remote5, whose level-5 correction is too small for 1e-6 of it
      to show.  Parent: caught (test_deep_mode_against_the_oracle_and_the_launches[k25-v]).
  (d) k_resident_big drops its last KE2 slot: all four mask-form cases.  Parent: caught
      (test_forced_big_kernel_against_oracle_and_resident[1024-1024-0.5-True-0-v]).
The new file runs in about 30 s on one MI355X (captures and oracle included)."""
import functools
import os
import re
from ctypes import byref, c_int32

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ipd_oracle as O
from tests import problems as PR

gpu = pytest.mark.gpu
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "codes_of_ipd_ssn_amg_method_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


# ---------------------------------------------------------------------------------------------------------------
# inventory (CPU): the instantiations run_resident launches in the normal build
# ---------------------------------------------------------------------------------------------------------------
def launched_instantiations():
    """Kernel names, as ipd_amg_resident_kernel spells them, of every row of the table run_resident launches from
    (RESIDENT_KERNELS, csrc/ipd_resident_host.h) in the normal build."""
    from tests.test_resident_plan import resident_table
    rows = resident_table()
    for name, from_key, from_kernel in rows:           # a row's name, key and kernel say the same
        assert name == from_key == from_kernel, (name, from_key, from_kernel)
    return [r[0] for r in rows]


# the width rules, mirrored from the planner (csrc/ipd_resident_plan.h): tests/test_resident_plan.py runs the planner
# against them for every stride and checks its cut-offs
def ke_of(smax):
    """plan_resident: ke = 4; while (64 * ke < smax) ke <<= 1;"""
    ke = 4
    while 64 * ke < smax:
        ke <<= 1
    return ke


def ke3_of(s3):
    return 4 if s3 <= 256 else 8


def big_ke2(s2, deep):
    return (4 if s2 <= 64 * 4 else 8) if deep else (16 if s2 <= 64 * 16 else 32)


def pad4(s):
    return (s + 3) // 4 * 4


# ---------------------------------------------------------------------------------------------------------------
# the systems
# ---------------------------------------------------------------------------------------------------------------
def mask_tree_hub(m, n, seed, rows):
    """PR.mask_tree with one hub column: `rows` random rows active in a random column.  Levels 1 and 2 get rows
    of about `rows` entries while the hierarchy keeps the tree's five levels."""
    Y = PR.mask_tree(m, n, seed=seed).reshape((m, n), order="F").copy()
    rs = np.random.RandomState(seed + 100)
    j = rs.choice(n, size=1, replace=False)[0]
    Y[rs.choice(m, size=rows, replace=False), j] = 1
    return Y.reshape(-1, order="F").copy()


@functools.lru_cache(maxsize=None)
def synthetic(kind, m, n, par, seed):
    """(Ae, f, fnode, p, q, tk): build_Ae(ASAt(s, p, q)) with random p and q, the largest component (F side first,
    Hybrid_AMG.m:55-68), f = [q; -p] .* z on it."""
    if kind == "bern":
        s = PR.mask_bernoulli(m, n, par, seed=seed)
    elif kind == "hub":
        s = PR.mask_hub(m, n, seed=seed)
    elif kind == "treehub":
        s = mask_tree_hub(m, n, seed, par)
    else:
        raise ValueError(kind)
    pd = PR.make_prob(m, n, s, pq_random=True)
    H0 = O.ASAt(s, pd["p"], pd["q"])
    Ae = sp.csr_matrix(O.build_Ae(H0, pd["T"], pd["p"], pd["q"], pd["bk1"], pd["tk"])[0])
    f = np.concatenate([pd["q"], -pd["p"]]) * pd["z"]
    ncomp, lab = sp.csgraph.connected_components(Ae)
    if ncomp > 1:
        pk = np.flatnonzero(lab == np.argmax(np.bincount(lab)))
        return sp.csr_matrix(Ae[pk, :][:, pk]), f[pk], int((pk < n).sum()), None, None, pd["tk"]
    return Ae, f, n, pd["p"], pd["q"], pd["tk"]


_captured = {}


def captured(ipd, N, kcap):
    """A Newton system of the Class 1 device driver (tests/newton_capture.py), its largest component."""
    if (N, kcap) not in _captured:
        from tests.newton_capture import capture
        Ae, f, tk = capture(ipd, N, kcap)
        ncomp, lab = sp.csgraph.connected_components(Ae)
        n = N
        if ncomp > 1:
            pk = np.flatnonzero(lab == np.argmax(np.bincount(lab)))
            Ae, f, n = sp.csr_matrix(Ae[pk, :][:, pk]), f[pk], int((pk < N).sum())
        M = Ae.shape[0]
        _captured[(N, kcap)] = (Ae, f, n, np.ones(M - n), np.ones(n), tk)
    return _captured[(N, kcap)]


def system(ipd, key):
    return captured(ipd, *key[1:]) if key[0] == "newton" else synthetic(*key)


# ---------------------------------------------------------------------------------------------------------------
# the case table: kernel name -> cases.  Fields: system key; cycle, smoth, isnsp; IPD_* switches; attach (the mask
# operator, or the composed level 2); (levels, tail root); J; level_forms; fills (the widths
# whose top slot a row reaches: "KE" levels 1-2 / level 2 of the mask-form kernel, "KE3" level 3); s3 (the longest
# level-3 row of a three-mode case); min_inf (oracle cycles with rel_res > 1e-9 the whole solve must have)
# ---------------------------------------------------------------------------------------------------------------
def case(cid, key, cycle, smoth, lv, J, forms, isnsp=1, kv=None, attach=None, fills=("KE",), s3=None, min_inf=4):
    return dict(id=cid, key=key, cycle=cycle, smoth=smoth, isnsp=isnsp, kv=kv or {}, attach=attach, lv=lv, J=J,
                forms=forms, fills=fills, s3=s3, min_inf=min_inf)


BERN256 = ("bern", 256, 256, 0.6, 2)           # 512 / 256 / 1, rows 176 / 255
BERN512 = ("bern", 512, 512, 0.3, 2)           # 1024 / 512 / 1, rows 189 / 511
BERN1024 = ("bern", 1024, 1024, 0.1, 2)        # 2048 / 1024 / 11, rows 138 / 1023
BERN1000 = ("bern", 1000, 1000, 0.9, 5)        # dense level 2: the composed form's system
HUB256 = ("hub", 256, 256, 0, 2)               # 512 / 256 / 43 / 1, rows 256 / 255 / 42
HUB512 = ("hub", 512, 512, 0, 2)               # 1024 / 512 / 165 / 3, rows 512 / 511 / 164
TH230 = ("treehub", 1024, 1024, 230, 8)        # 2048 / 1024 / 177 / 14 / 1, rows 235 / 256 / 176
TH490 = ("treehub", 1024, 1024, 490, 7)        # 2048 / 1024 / 180 / 15 / 1, rows 494 / 510 / 179
TH1200 = ("treehub", 1200, 1200, 215, 6)       # 2400 / 1200 / 200 / 19 / 1, rows 217 / 246
TH1200B = ("treehub", 1200, 1200, 450, 6)      # 2400 / 1200 / 200 / 19 / 1, rows 452 / 473
BIG1024 = ("bern", 1024, 1024, 0.5, 5)         # 2048 / 1024 / 1, rows 571 / 1023
BIG2000 = ("bern", 2000, 256, 0.5, 5)          # 2256 / 2000 / 1, rows 255 / 1999
NEWTON1024 = ("newton", 1024, 20)              # 2044 / 1022 / 306 / 98 / 28 / 7 (k = 21 of the driver run)
NEWTON1024B = ("newton", 1024, 30)             # 2048 / 1024 / 324 / 102 / 34 / 11
NEWTON2048 = ("newton", 2048, 24)              # 4096 / 2048 / 645 / 199 / 48 / 11

MASK_OP = "mask_operator"
COMPOSED = "composed"

CASES = {
    "k_resident<4,4,0>": [
        case("bern256-local", BERN256, "v", 1, (2, 3), 3, [0, 0, 0]),
        case("newton1024k31-remote3", NEWTON1024B, "w", 5, (2, 3), 6, [0, 0, 1, 16, 32, 4],
             kv=dict(IPD_NO_RESIDENT_THREE=1), fills=()),
    ],
    "k_resident<8,8,0>": [case("bern512-local", BERN512, "w", 1, (2, 3), 3, [0, 0, 0], isnsp=0)],
    "k_resident<16,16,0>": [case("bern1024-local", BERN1024, "v", 1, (2, 3), 3, [0, 0, 0])],
    "k_resident<16,16,0,true>": [case("bern1000-composed-local", BERN1000, "v", 1, (2, 3), 3, [0, 128, 0],
                                      attach=COMPOSED, min_inf=1)],
    "k_resident<4,4,1>": [
        case("treehub230-remote4", TH230, "w", 1, (3, 4), 5, [0, 0, 64, 8, 4]),
        case("newton1024k21-remote5", NEWTON1024, "w", 5, (4, 5), 6, [0, 0, 65, 80, 32, 4], fills=()),
    ],
    "k_resident<8,8,1>": [case("treehub490-remote4", TH490, "v", 1, (3, 4), 5, [0, 0, 64, 8, 4])],
    "k_resident<4,4,4>": [
        case("hub256-local", HUB256, "v", 1, (3, 4), 4, [0, 0, 32, 4], isnsp=0, s3=42),
        case("treehub230-remote4", TH230, "w", 1, (3, 4), 5, [0, 0, 0, 4, 4], kv=dict(IPD_NO_POLY=1), s3=176),
    ],
    "k_resident<8,8,4>": [
        case("hub512-local", HUB512, "w", 1, (3, 4), 4, [0, 0, 0, 0], s3=164),
        case("treehub490-remote4", TH490, "v", 1, (3, 4), 5, [0, 0, 0, 4, 4], kv=dict(IPD_NO_POLY=1), s3=179),
    ],
    "k_resident<4,4,8>": [case("hub512-s3", HUB512, "w", 1, (3, 4), 4, None, fills=("KE", "KE3"))],
    "k_resident<8,8,8>": [case("treehub490-s3", TH490, "v", 1, (3, 4), 5, None, kv=dict(IPD_NO_POLY=1),
                               fills=("KE", "KE3"))],
    "k_resident_big<16,1,false>": [case("bern1024-forced-local", BIG1024, "v", 1, (2, 3), 3, [0, 0, 0],
                                        attach=MASK_OP, kv=dict(IPD_RESIDENT_BIG=1))],
    "k_resident_big<32,1,false>": [case("bern2000x256-local", BIG2000, "v", 1, (2, 3), 3, [0, 0, 0], attach=MASK_OP)],
    "k_resident_big<4,2,true>": [
        case("treehub1200-deep", TH1200, "w", 1, (3, 4), 5, [0, 0, 64, 8, 4], attach=MASK_OP),
        case("newton2048k25-deep5", NEWTON2048, "w", 5, (4, 5), 6, [0, 0, 64, 64, 32, 4], attach=MASK_OP, fills=()),
    ],
    "k_resident_big<8,2,true>": [case("treehub1200-deep", TH1200B, "w", 1, (3, 4), 5, [0, 0, 64, 8, 4],
                                      attach=MASK_OP)],
}
UNREACHABLE = {"k_resident<4,4,8>", "k_resident<8,8,8>"}
FLAT = [(name, c) for name, cs in CASES.items() for c in cs]


def _param(name, c):
    marks = [pytest.mark.xfail(strict=True, raises=AssertionError,
                               reason="S3 > 256 in three mode: not reached by any system searched")] \
        if name in UNREACHABLE else []
    return pytest.param(name, c, id="%s-%s" % (name, c["id"]), marks=marks)


PARAMS = [_param(name, c) for name, c in FLAT]
SOLVED = [_param(name, c) for name, c in FLAT if name not in UNREACHABLE]


def test_inventory_matches_the_case_table():
    launched = launched_instantiations()
    assert len(launched) == len(set(launched)) == 14, launched
    assert set(launched) == set(CASES), sorted(set(launched) ^ set(CASES))


def test_width_rules_match_the_sources():
    # (the host's rules: test_resident_plan.py, test_widths_match_the_mirrors_for_every_stride)
    res = _src("ipd_resident.h")
    assert "const int e = lane + 64 * q;\n        const bool ok = valid && e < L.S;" in res
    assert [ke_of(s) for s in (1, 256, 257, 512, 513, 1024, 1025)] == [4, 4, 8, 8, 16, 16, 32]
    assert [ke3_of(s) for s in (1, 256, 257)] == [4, 4, 8]
    assert [big_ke2(s, d) for s, d in ((256, True), (257, True), (1024, False), (1025, False))] == [4, 8, 16, 32]


def test_case_table_is_consistent():
    tails = set()
    for name, c in FLAT:
        big = name.startswith("k_resident_big")
        assert (c["attach"] == MASK_OP) == big, c["id"]
        assert c["lv"] in ((2, 3), (3, 4), (4, 5)), c["id"]
        ke3 = None if big else int(re.findall(r"\d+", name)[2])
        three = ke3 in (4, 8)
        assert (c["s3"] is not None) == (three and name not in UNREACHABLE), c["id"]
        if name not in UNREACHABLE:
            tails.add("local" if "local" in c["id"] else c["lv"][1])
    assert tails == {"local", 3, 4, 5}


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ipd():
    import codes_of_ipd_ssn_amg_method_amd as m
    return m


def longest_rows(h):
    """The longest off-diagonal row of every level of the device hierarchy (what the padded copies hold)."""
    out = []
    for k in range(1, h.J + 1):
        A = sp.csr_matrix(h.A(k))
        out.append(int((np.diff(A.indptr) - (A.diagonal() != 0)).max()))
    return out


def attach_fn(c, sysd):
    Ae, f, n, p, q, tk = sysd
    if c["attach"] == MASK_OP:
        return lambda h: h.attach_mask_operator(p, q, tk)
    if c["attach"] == COMPOSED:
        return lambda h: h.attach_level2_poly()
    return None


def check_reach(name, c, h):
    """Reach and fill, on a hierarchy built for the case."""
    from codes_of_ipd_ssn_amg_method_amd import _lib
    from tests.test_gpu_bench_workload import resident_kernel_name, solve_mode
    lev, root = c_int32(), c_int32()
    _lib.check(_lib.lib.ipd_amg_resident_levels(h.handle, byref(lev), byref(root)))
    got = (solve_mode(h)[0], resident_kernel_name(h), (lev.value, root.value))
    assert got == (2, name, c["lv"]), (got, h.level_sizes(), longest_rows(h))
    if c["J"] is not None:
        assert h.J == c["J"], h.level_sizes()
    local = h.J == c["lv"][1]                      # the tail is the coarsest level, solved by every workgroup
    assert local == ("local" in c["id"]), (c["id"], h.J, c["lv"])
    if c["forms"] is not None:
        assert h.level_forms() == c["forms"], h.level_forms()
    rows = longest_rows(h)
    big = name.startswith("k_resident_big")
    ke = [int(v) for v in re.findall(r"\d+", name)[:3]]
    if big:
        deep = name.endswith("true>")
        assert big_ke2(pad4(rows[1]), deep) == ke[0], rows
        filled = rows[1] > 64 * (ke[0] - 1)
    else:
        assert ke_of(pad4(max(rows[0], rows[1]))) == ke[0] == ke[1], rows
        filled = max(rows[0], rows[1]) > 64 * (ke[0] - 1)
    assert filled == ("KE" in c["fills"]), (rows, c["fills"])
    if not big and ke[2] in (4, 8):
        assert ke3_of(pad4(rows[2])) == ke[2], rows
        assert (rows[2] > 64 * (ke[2] - 1)) == ("KE3" in c["fills"]), (rows, c["fills"])
        if c["s3"] is not None:
            assert rows[2] == c["s3"], rows


@gpu
@pytest.mark.parametrize("name,c", PARAMS)
def test_reach_and_fill(ipd, name, c):
    from tests.test_gpu_bench_workload import env, options
    sysd = system(ipd, c["key"])
    Ae, f, n = sysd[:3]
    opts = options(c["cycle"], n, isnsp=c["isnsp"])
    opts["smoth"] = c["smoth"]
    with env(**c["kv"]):
        h = ipd.AMGHierarchy(Ae, opts, ipd.MatlabRand(5489))
        at = attach_fn(c, sysd)
        if at is not None:
            assert at(h)
    try:
        check_reach(name, c, h)
    finally:
        h.close()


@gpu
@pytest.mark.parametrize("name,c", SOLVED)
def test_whole_solve_against_the_oracle(ipd, name, c):
    from tests.test_gpu_resident_remote import _against_oracle
    sysd = system(ipd, c["key"])
    Ae, f, n = sysd[:3]
    x0 = np.zeros(Ae.shape[0])
    got = _against_oracle(ipd, Ae, f, n, c["cycle"], x0, kv=c["kv"], smoth=c["smoth"], isnsp=c["isnsp"],
                          attach=attach_fn(c, sysd), inspect=lambda h: check_reach(name, c, h))
    it, ito, relk, relko = got
    informative = int(np.sum(np.asarray(relko[:ito + 1]) > 1e-9))
    assert informative >= c["min_inf"], relko
    assert it >= c["min_inf"], relk


@gpu
@pytest.mark.parametrize("name,c", SOLVED)
def test_k_cycles_against_the_oracle(ipd, name, c):
    from tests.test_gpu_bench_workload import bench_cycles, env, options, oracle_cycles, solve_mode
    sysd = system(ipd, c["key"])
    Ae, f, n = sysd[:3]
    opts = options(c["cycle"], n, isnsp=c["isnsp"])
    opts["smoth"] = c["smoth"]
    with env(**c["kv"]):
        h = ipd.AMGHierarchy(Ae, opts, ipd.MatlabRand(5489))
        at = attach_fn(c, sysd)
        if at is not None:
            assert at(h)
    try:
        check_reach(name, c, h)
        A = sp.csr_matrix(Ae)
        nf = np.linalg.norm(f)
        u = np.random.RandomState(7).standard_normal(Ae.shape[0])
        x0 = u * (1e3 * nf / np.linalg.norm(A @ u))         # |f - A x0| ~ 1e3 |f|: a large error
        sgn = np.where(np.random.RandomState(11).random_sample(f.size) < 0.5, -1.0, 1.0)
        fp = f * (1.0 + 2.2e-16 * sgn)
        for K in (1, 2):
            with env(**c["kv"]):
                x = bench_cycles(h, f, x0, K)[0]
            assert solve_mode(h)[2] == 0
            xo = oracle_cycles(Ae, f, x0, opts, K)[0]
            xp = oracle_cycles(Ae, fp, x0, opts, K)[0]
            sens = np.linalg.norm(A @ (xo - xp))
            bar = max(4.0 * sens, 1e-12 * nf)
            dev = np.linalg.norm(A @ (x - xo))
            res = np.linalg.norm(f - A @ xo)
            assert dev <= bar, (K, dev, bar, sens, res)
            assert bar <= 1e-3 * res, (K, bar, res)
    finally:
        h.close()


@gpu
def test_three_mode_s3_search(ipd):
    """The largest level-3 row among the hierarchies of the search that the planner takes in three mode: below the
    257 entries KE3 = 8 needs (see the module docstring)."""
    from tests.test_gpu_bench_workload import resident_kernel_name, solve_mode
    keys = [HUB256, HUB512, TH230, TH490, ("hub", 384, 384, 0, 2), ("hub", 448, 448, 0, 3)] + [
        ("treehub", 1024, 1024, r, s) for r in (200, 300, 400, 505) for s in (2, 6, 7)]
    best = (0, None)
    for key in keys:
        Ae, f, n = synthetic(*key)[:3]
        for cycle in ("v", "w"):
            for kv in ({}, dict(IPD_NO_POLY=1)):
                from tests.test_gpu_bench_workload import env, options
                with env(**kv):
                    h = ipd.AMGHierarchy(Ae, options(cycle, n), ipd.MatlabRand(5489))
                name = resident_kernel_name(h)
                if solve_mode(h)[0] == 2 and re.fullmatch(r"k_resident<\d+,\d+,[48]>", name):
                    sizes, rows = h.level_sizes(), longest_rows(h)
                    assert rows[2] < sizes[2], (key, sizes)
                    if rows[2] > best[0]:
                        best = (rows[2], (key, cycle, kv, name, sizes))
                h.close()
    print("largest S3 taken in three mode: %d %s" % best)
    assert 0 < best[0] <= 256, best
