"""Both certificates in one device call (csrc/ipd_bracket.hip: ipd_apd_bracket, ipd_apd_bracket_dev;
APDWorkspace.gap_probe, gap_probe_dev).

The reference is the composition the call replaces: ipd_apd_dual(side, primal = 1) and ipd_apd_round(tol, side) for
both sides, picked with the expressions of APDWorkspace.certificate and APDWorkspace.bracket.  Those calls are held
to numpy restatements by tests/test_gpu_dual.py and tests/test_gpu_round.py; here every number of the fused call is
compared with theirs bit for bit, which is what the header promises: the fused kernels keep the per-entry operations
and the summation shapes, and a maximum or minimum under its key does not depend on an order.  States are injected
with set_state (test_gpu_round.py's noisy_plan with a random lk); the shapes are that file's ten."""
import ctypes

import numpy as np
import pytest

from tests import test_gpu_round as TR

pytestmark = pytest.mark.gpu

INF = np.inf
SENT = TR.SENT
SHAPES = TR.SHAPES
DUAL_KEYS = ("dual", "bterm", "cap", "dmin", "imin", "jmin", "nneg", "fval", "gap")
ipd, lib_mod, problem, ws_of, same_bits, inject, noisy_plan = (TR.ipd, TR.lib_mod, TR.problem, TR.ws_of, TR.same_bits,
                                                               TR.inject, TR.noisy_plan)


def composed(ws, tol):
    """bracket() out of the single calls, with the vectors and the multiplier of the winners"""
    duals = [ws.dual(side=s, primal=True) for s in (0, 1)]
    rounds = [ws.round_plan(tol, side=s) for s in (0, 1)]
    ls = 1 if duals[1]["dual"] > duals[0]["dual"] else 0                      # APDWorkspace.certificate
    us = min((0, 1), key=lambda s: (not rounds[s]["ok"], rounds[s]["fval"]))  # APDWorkspace.bracket
    lower, upper = dict(duals[ls], side=ls), dict(rounds[us], side=us)
    with np.errstate(invalid="ignore"):
        gap = np.float64(upper["fval"]) - np.float64(lower["dual"])
    return dict(lower=lower, upper=upper, gap=float(gap), duals=duals, rounds=rounds)


def assert_same(got, want, what):
    assert got["lower"]["side"] == want["lower"]["side"] and got["upper"]["side"] == want["upper"]["side"], what
    for k in DUAL_KEYS + ("lam",):
        assert same_bits(got["lower"][k], want["lower"][k]), (what, "lower", k, got["lower"][k], want["lower"][k])
    for k in TR.STAT_KEYS + TR.VEC_KEYS:
        if k in got["upper"] or k in TR.STAT_KEYS:
            assert same_bits(got["upper"][k], want["upper"][k]), (what, "upper", k, got["upper"][k], want["upper"][k])
    assert same_bits(got["gap"], want["gap"]), (what, got["gap"], want["gap"])


# ---------------------------------------------------------------------------
# 1. fused against composed
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", SHAPES)
def test_fused_against_composed(cls, m, n):
    sides = set()
    for pq_random in (False, True):
        pr = problem(cls, m, n, seed=3, pq_random=pq_random)
        ws = ws_of(cls, pr)
        rs = np.random.RandomState(100 * m + n + cls)
        for noise in (1e-6, 0.3):
            inject(ws, noisy_plan(cls, pr, m, n, noise, rs), rs)
            for tol in (0.0, 0.375):
                what = "cls %d %dx%d pq %d noise %g tol %g" % (cls, m, n, pq_random, noise, tol)
                want = composed(ws, tol)
                got = ws.gap_probe(tol, vectors=True)
                assert_same(got, want, what)
                assert_same(ws.gap_probe(tol), want, what)          # vectors NULL: the same statistics
                sides.add((got["lower"]["side"], got["upper"]["side"]))
        ws.close()
    print("cls %d %dx%d: (lower, upper) sides seen %s" % (cls, m, n, sorted(sides)))


@pytest.mark.parametrize("cls", [1, 2])
def test_each_side_can_win(cls):
    """One held entry far too large costs its side 1000 times that entry's marginal, and the other side forms that
    entry anew: lam[j] += 1000 for the column with the largest r leaves side 1 the winner, the row with the largest l
    side 0.  The duals of an O(1) multiplier are below 2*(sum r + sum l) in size, far less."""
    m, n = 65, 33
    pr = problem(cls, m, n, seed=4, pq_random=True)
    ws = ws_of(cls, pr)
    rs = np.random.RandomState(77)
    for held, at in ((0, int(np.argmax(pr["r"]))), (1, n + int(np.argmax(pr["l"])))):
        lam = 0.1 * rs.standard_normal(ws.L)
        lam[at] += 1000.0
        inject(ws, noisy_plan(cls, pr, m, n, 0.2, rs), rs, lam=lam)
        want = composed(ws, 0.0)
        got = ws.gap_probe(0.0, vectors=True)
        assert_same(got, want, (cls, held))
        assert got["lower"]["side"] == 1 - held, (held, [d["dual"] for d in want["duals"]])
    ws.close()


# ---------------------------------------------------------------------------
# 2. ties and NaNs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(65, 33), (64, 16), (65, 150), (300, 16)])
def test_ties(m, n):
    """c constant, and c in four dyadic levels with a dyadic lk: candidates tie in whole rows and columns, the
    differences are exact, and the repaired multiplier and the place of the smallest reduced cost are ipd_apd_dual's."""
    rs = np.random.RandomState(8)
    p, q = np.ones(m), np.ones(n)
    r, l = rs.random_sample(n), rs.random_sample(m)
    l = l * (r @ q) / (l @ p)
    for level in ("constant", "four"):
        C = np.full((m, n), 0.75) if level == "constant" else rs.randint(0, 4, size=(m, n)) / 4.0
        pr = dict(c=C.reshape(-1, order="F"), r=r, l=l, p=p, q=q)
        ws = ws_of(1, pr)
        for lam in (np.zeros(m + n), rs.randint(-2, 3, m + n) / 4.0):
            inject(ws, noisy_plan(1, pr, m, n, 0.3, rs), rs, lam=lam)
            want = composed(ws, 0.0)
            got = ws.gap_probe(0.0, vectors=True)
            assert_same(got, want, (m, n, level))
            # both sides tie in value often: the pick keeps side 0 then, as certificate() does
            if want["duals"][0]["dual"] == want["duals"][1]["dual"]:
                assert got["lower"]["side"] == 0
            assert got["lower"]["dmin"] == 0.0          # multiples of 1/4: every operation is exact
        ws.close()


@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", [(65, 33), (257, 19), (65, 150)])
def test_nans(cls, m, n):
    """NaNs planted in x (a NaN is clamped to 0 by the rounding and poisons <c, x>) and in c (a NaN candidate counts as
    -inf, a NaN reduced cost never wins): the fused call has the composed calls' bits, NaNs included."""
    rs = np.random.RandomState(31 + m)
    pr = problem(cls, m, n, seed=5, pq_random=True)
    for where in ("x", "c", "both"):
        pn = dict(pr)
        if where in ("c", "both"):
            pn["c"] = pr["c"].copy()
            pn["c"][rs.random_sample(m * n) < 0.03] = np.nan
            pn["c"][(m * n) // 2] = np.nan
        ws = ws_of(cls, pn)
        X = noisy_plan(cls, pr, m, n, 0.3, rs)
        if where in ("x", "both"):
            X[rs.random_sample((m, n)) < 0.03] = np.nan
            X[m // 2, n // 2] = np.nan
        inject(ws, X, rs)
        want = composed(ws, 0.0)
        got = ws.gap_probe(0.0, vectors=True)
        assert_same(got, want, (cls, m, n, where))
        assert np.isnan(got["lower"]["fval"]) and np.isnan(got["lower"]["gap"])
        assert np.isnan(got["gap"]) == (where != "x")    # a NaN of x is clamped away by the rounding, one of c stays
        assert np.isfinite(got["lower"]["lam"]).all()
        ws.close()


# ---------------------------------------------------------------------------
# 3. cost sources
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("m,n", [(65, 150), (257, 19)])
def test_cost_sources_agree(cls, d, m, n):
    rs = np.random.RandomState(40 + d)
    xs, ys = rs.random_sample((m, d)), rs.random_sample((n, d))
    r, l = rs.random_sample(n), rs.random_sample(m)
    p, q = 0.5 + rs.random_sample(m), 0.5 + rs.random_sample(n)
    kw = dict(mu=0.65 * min(r.sum(), l.sum()), phi=0.5 + rs.random_sample(m * n)) if cls == 2 else {}
    pr = dict(r=r, l=l, p=p, q=q, **kw)
    if cls == 1:
        pr["l"] = l = l * (r @ q) / (l @ p)
    Xd = noisy_plan(cls, pr, m, n, 0.3, rs)
    for metric in ("sqeuclidean", "cityblock"):
        stored = ipd().APDWorkspace.from_points(cls, xs, ys, r, l, p, q, metric=metric, **kw)
        free = ipd().APDWorkspace.from_points(cls, xs, ys, r, l, p, q, metric=metric, matrix_free=True, **kw)
        assert (stored.cost_info()["form"], free.cost_info()["form"]) == (0, 1)
        host = ipd().APDWorkspace(cls, stored.cost().reshape(-1, order="F"), r, l, p, q, **kw)
        for ws in (host, stored, free):
            inject(ws, Xd, np.random.RandomState(5))
        want = composed(host, 0.0)
        for ws in (host, stored, free):
            assert_same(ws.gap_probe(0.0, vectors=True), want, (cls, d, m, n, metric))
        for ws in (host, stored, free):
            ws.close()


# ---------------------------------------------------------------------------
# 4. install, and install = 0 reads only
# ---------------------------------------------------------------------------
def same_state(a, b):
    return all(same_bits(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


@pytest.mark.parametrize("pq_random", [False, True])
@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", [(65, 150), (300, 16), (257, 19)])
def test_install_is_round_plans(cls, m, n, pq_random):
    """The state after gap_probe(install=True) has the bits of a twin workspace's after
    round_plan(side=upper_side, install=True): x, and class 2's y and z, in u and in v; lk and bk stay."""
    pr = problem(cls, m, n, seed=9, pq_random=pq_random)
    ws, twin = ws_of(cls, pr), ws_of(cls, pr)
    rs = np.random.RandomState(m * n + cls)
    u, v, lam = inject(ws, noisy_plan(cls, pr, m, n, 0.3, rs), rs)
    twin.set_state(u, v, lam, 0.37)
    hist, recs = ws.history(), ws.records()
    plain = ws.gap_probe(0.0, vectors=True)
    assert same_state(ws.state(), (u, v, lam, 0.37))                  # install = 0: the workspace is only read
    got = ws.gap_probe(0.0, install=True, vectors=True)
    assert_same(got, plain, (cls, m, n))
    assert got["upper"]["ok"] == 1
    twin.round_plan(0.0, side=got["upper"]["side"], install=True)
    after, want = ws.state(), twin.state()
    assert same_state(after, want)
    assert not same_bits(after[0][:m * n], u[:m * n]) and same_bits(after[2], lam) and after[3] == 0.37
    if cls == 2:
        assert same_bits(after[0][m * n:], want[0][m * n:]) and same_bits(after[1][m * n:], want[1][m * n:])
        assert not same_bits(after[0][m * n:], u[m * n:])
    h1 = ws.history()
    assert h1.keys() == hist.keys() and all(same_bits(h1[k], hist[k]) for k in hist)
    assert repr(ws.records()) == repr(recs)
    ws.close()
    twin.close()


@pytest.mark.parametrize("m,n", [(65, 33), (300, 16)])
def test_install_without_a_repair(m, n):
    """test_gpu_round.py's test_class2_without_a_repair: ok = 0 on both sides.  install = 0 reports it; install = 1 is
    IPD_E_NUMERIC, the state keeps its bits and no output is written."""
    L = lib_mod()
    pr = problem(2, m, n, seed=6, pq_random=True)
    pr["mu"] = 4.0 * float((pr["phi"].reshape((m, n), order="F") * np.outer(pr["l"], pr["r"])).sum()) + 10.0
    ws = ws_of(2, pr)
    rs = np.random.RandomState(3)
    X = 0.5 * np.outer(pr["l"], pr["r"]) / max(pr["q"] @ pr["r"], pr["p"] @ pr["l"])
    inject(ws, np.where(rs.random_sample((m, n)) < 0.1, -X, X), rs)
    before = ws.state()
    want = composed(ws, 0.0)
    got = ws.gap_probe(0.0, vectors=True)
    assert_same(got, want, (m, n))
    assert got["upper"]["ok"] == 0
    with pytest.raises(L.IpdError) as ei:
        ws.gap_probe(0.0, install=True)
    assert ei.value.code == L.IPD_E_NUMERIC
    for call in raw_calls(L, ws, ws.handle, 0.0, 1):
        assert call[0] == L.IPD_E_NUMERIC and untouched(call)
    assert same_state(ws.state(), before)
    ws.close()


@pytest.mark.parametrize("cls", [1, 2])
def test_workspace_untouched_after_a_run(cls):
    """After a short run (histories and records are not empty) a probe with install = 0 changes nothing."""
    m, n = 24, 24
    pr = problem(cls, m, n, seed=12)
    ws = ws_of(cls, pr)
    ws.warmup(0.0, 40)
    ws.run(TR.AMG1 if cls == 1 else TR.AMG2, ipd().MatlabRand(), iters=2)
    state, hist, recs = ws.state(), ws.history(), ws.records()
    assert len(recs) > 0
    got = ws.gap_probe(0.0, vectors=True)
    assert_same(got, composed(ws, 0.0), cls)
    br = ws.bracket()
    assert same_bits(got["gap"], br["gap"]) and same_bits(got["lower"]["dual"], br["lower"]["dual"])
    assert same_state(ws.state(), state) and repr(ws.records()) == repr(recs)
    h1 = ws.history()
    assert h1.keys() == hist.keys() and all(same_bits(h1[k], hist[k]) for k in hist)
    assert ws.gap_records() == [] and ws.gap_lam() == (None, -INF)
    ws.close()


# ---------------------------------------------------------------------------
# 5. the two entries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [1, 2])
def test_calls_agree(cls):
    L = lib_mod()
    m, n = 600, 150
    pr = problem(cls, m, n, seed=7, pq_random=True)
    ws = ws_of(cls, pr)
    rs = np.random.RandomState(9)
    inject(ws, noisy_plan(cls, pr, m, n, 0.3, rs), rs)
    before = ws.state()
    for tol in (0.0, 1e-4):
        a = ws.gap_probe(tol, vectors=True)
        assert_same(ws.gap_probe(tol, vectors=True), a, "two calls")
        sizes = dict(lam_out=ws.L, rho=m, kappa=n, e=m, f=n)
        bufs = {k: L.DeviceBuffer.from_array(np.full(sizes[k], SENT)) for k in sizes}
        c = ws.gap_probe_dev(tol, **bufs)
        c["lower"]["lam"] = bufs["lam_out"].to_array(np.float64, ws.L)
        c["upper"].update({k: bufs[k].to_array(np.float64, sizes[k]) for k in TR.VEC_KEYS})
        assert_same(c, a, "device entry")
        d = ws.gap_probe_dev(tol)                                     # every pointer NULL
        d["lower"]["lam"] = a["lower"]["lam"]
        assert_same(d, a, "device entry, no vectors")
        e = ws.gap_probe_dev(tol, e=bufs["e"])
        e["lower"]["lam"] = a["lower"]["lam"]
        assert_same(e, a, "device entry, one vector")
        for buf in bufs.values():
            buf.free()
    assert same_state(ws.state(), before)
    t_rho, t_lam = TR.Tensor(np.full(m, SENT)), TR.Tensor(np.full(ws.L, SENT))
    a = ws.gap_probe(0.0, vectors=True)
    ws.gap_probe_dev(0.0, rho=t_rho, lam_out=(t_lam.data_ptr(), ws.L))
    assert same_bits(t_rho.numpy(), a["upper"]["rho"]) and same_bits(t_lam.numpy(), a["lower"]["lam"])
    with pytest.raises(ValueError):
        ws.gap_probe_dev(rho=(t_rho.data_ptr(), m - 1))
    with pytest.raises(ValueError):
        ws.gap_probe_dev(kappa=TR.Tensor(np.zeros(n), np.float32))
    ws.close()


# ---------------------------------------------------------------------------
# 6. errors
# ---------------------------------------------------------------------------
NB = 24   # doubles of an ipd_bracket


def raw_calls(L, ws, h, tol, install, with_out=True):
    """both entries on pre-filled outputs -> [(rc, [lam, rho, kappa, e, f], the result's bytes as doubles)]"""
    lib = L.lib
    m, n = ws.m, ws.n
    sizes = (ws.L, m, n, m, n)
    res = []
    out = (ctypes.c_double * NB)(*([SENT] * NB))
    vec = [np.full(k, SENT) for k in sizes]
    rc = lib.ipd_apd_bracket(h, tol, install, *[v.ctypes.data for v in vec],
                             ctypes.addressof(out) if with_out else None)
    res.append((rc, vec, np.array(out)))
    out = (ctypes.c_double * NB)(*([SENT] * NB))
    dev = [L.DeviceBuffer.from_array(np.full(k, SENT)) for k in sizes]
    rc = lib.ipd_apd_bracket_dev(h, tol, install, *[d.ptr for d in dev], ctypes.addressof(out) if with_out else None)
    res.append((rc, [d.to_array(np.float64, k) for d, k in zip(dev, sizes)], np.array(out)))
    for d in dev:
        d.free()
    return res


def untouched(call):
    rc, vec, out = call
    return all((v == SENT).all() for v in vec) and (out == SENT).all()


def test_argument_errors_write_nothing():
    L = lib_mod()
    assert ctypes.sizeof(L.ipd_bracket) == NB * 8
    m, n = 37, 5
    pr = problem(1, m, n, seed=13)
    ws = ws_of(1, pr)
    rs = np.random.RandomState(14)
    inject(ws, noisy_plan(1, pr, m, n, 0.3, rs), rs)
    before = ws.state()
    h, E = ws.handle, L.IPD_E_ARG
    cases = [("NULL h", None, 0.0, 0, True), ("NULL out", h, 0.0, 0, False), ("install -1", h, 0.0, -1, True),
             ("install 2", h, 0.0, 2, True), ("tol < 0", h, -1e-300, 1, True), ("tol NaN", h, np.nan, 0, True)]
    for name, hh, tol, install, with_out in cases:
        for call in raw_calls(L, ws, hh, tol, install, with_out):
            assert call[0] == E and untouched(call), name
    assert same_state(ws.state(), before)
    # finite gama, scalar and vector
    for gama in (0.625, 0.25 + rs.random_sample(m * n)):
        wg = ws_of(1, pr, gama=gama)
        inject(wg, noisy_plan(1, pr, m, n, 0.3, rs), rs)
        for install in (0, 1):
            for call in raw_calls(L, wg, wg.handle, 0.0, install):
                assert call[0] == L.IPD_E_UNSUPPORTED and untouched(call), install
        with pytest.raises(L.IpdError) as ei:
            wg.gap_probe()
        assert ei.value.code == L.IPD_E_UNSUPPORTED
        wg.close()
    # a divider that is zero, negative or not finite, in p or in q: the call forms both transforms
    for bad in (0.0, -1.0, INF, np.nan):
        for key in ("p", "q"):
            pb = dict(pr)
            pb[key] = pr[key].copy()
            pb[key][3] = bad
            wb = ws_of(1, pb)
            inject(wb, noisy_plan(1, pr, m, n, 0.3, rs), rs)
            kept = wb.state()
            for _ in range(2):
                for call in raw_calls(L, wb, wb.handle, 0.0, 1):
                    assert call[0] == E and untouched(call), (bad, key)
            assert same_state(wb.state(), kept)
            wb.close()
    # and the unedited call is fine
    for call in raw_calls(L, ws, h, 0.0, 0):
        assert call[0] == 0 and not any((v == SENT).any() for v in call[1]) and not (call[2] == SENT).any()
    ws.close()
