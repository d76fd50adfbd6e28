"""The rounding's north-west-corner correction on the device (csrc/ipd_round_nw.hip: ipd_apd_set_correction,
ipd_apd_correction_entries, ipd_apd_correction_info; APDWorkspace.set_correction, correction_entries,
correction_info, projection_order, the drivers' correction keywords).

Reference: tests/round_nw_ref.py, the header's steps N1-N7 re-stated in numpy with the header's scan shape.  The
device's e, f, Se, Sf go into the restatement and the list (i, j, g) must come out bit for bit; on dyadic inputs, where
every sum is exact, cc, cp and fval must too.  The rounded plan is rebuilt in longdouble from the factors and the list
and held to tests/round_ref.py's feasibility bounds gamma(m+n+16)*(l_i + T/p_i): the scans add at most
gamma(max(m,n))*Sf to a marginal, inside that bound.  States are injected with set_state; only the gap-rule and the
driver tests run the solver."""
import ctypes

import numpy as np
import pytest

from tests import round_nw_ref as NW
from tests import round_ref as R
from tests import test_gpu_round as TR

pytestmark = pytest.mark.gpu

LD = np.longdouble
SHAPES = TR.SHAPES + [(1000, 90)]     # m + n just past a scan chunk of the compaction's spans and past 1024
ipd, lib_mod, problem, ws_of, same_bits, same_result = (TR.ipd, TR.lib_mod, TR.problem, TR.ws_of, TR.same_bits,
                                                        TR.same_result)
inject, noisy_plan, SENT = TR.inject, TR.noisy_plan, TR.SENT
KEPT = ("rho", "kappa", "e", "f", "fs", "ms", "se", "sf", "viol_in", "dropped", "ndropped")


def orders(m, n, seed):
    rs = np.random.RandomState(seed)
    return rs.permutation(m).astype(np.int32), rs.permutation(n).astype(np.int32)


def list_of(pr, got, sigma, tau):
    """the restatement's list from what the call returned"""
    return NW.correction(pr["p"], pr["q"], got["e"], got["f"], got["se"], got["sf"], sigma, tau)


def assert_list(ws, ref, what):
    i, j, g = ws.correction_entries()
    info = ws.correction_info()
    assert info["form"] == 1 and info["count"] == len(i) == len(ref["i"]), (what, info, len(ref["i"]))
    assert np.array_equal(i, ref["i"]) and np.array_equal(j, ref["j"]), what
    assert same_bits(g, ref["g"]), what
    assert len(i) <= ws.m + ws.n - 1
    return i, j, g


# ---------------------------------------------------------------------------
# 1. the list, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", SHAPES)
def test_list_bit_for_bit(cls, m, n):
    pr = problem(cls, m, n, seed=3, pq_random=True)
    ws = ws_of(cls, pr)
    rs = np.random.RandomState(100 * m + n + cls)
    X = noisy_plan(cls, pr, m, n, 0.3, rs)
    X[:, ::3] *= 1.5          # rows and columns above their marginals beside rows and columns below them
    X[m // 3:m // 2 + 1, :] *= 2.0
    u, _, _ = inject(ws, X, rs)
    C = pr["c"].reshape((m, n), order="F")
    for sigma, tau in ((None, None), orders(m, n, m + n)):
        ws.set_correction("north_west", sigma, tau)
        for side in (0, 1):
            what = (cls, m, n, side, sigma is None)
            got = ws.round_plan(0.0, side=side)
            ref = list_of(pr, got, sigma, tau)
            i, j, g = assert_list(ws, ref, what)
            terms = C[i, j].astype(LD) * g.astype(LD)
            assert abs(LD(got["cc"]) - terms.sum()) <= R.gamma(len(i) + 16) * float(np.abs(terms).sum()), what
            if cls == 2:
                terms = pr["phi"].reshape((m, n), order="F")[i, j].astype(LD) * g.astype(LD)
                assert abs(LD(got["cp"]) - terms.sum()) <= R.gamma(len(i) + 16) * float(np.abs(terms).sum()), what
    ws.close()


def dyadic_state(cls, m, n, seed, zero=False):
    """x in multiples of 2^-10, p, q in {0.5, 1, 2}, c and phi in multiples of 2^-6, l and r above the first marginals
    by deficits in multiples of 2^-4 with runs of zeros: both scale vectors are 1, e and f are those deficits, and every
    sum of the correction is exact.  The first entries of e and f agree (with p = q = 1 there) and Se = Sf, so prefixes
    of the two vectors tie.  zero: all deficits 0."""
    rs = np.random.RandomState(seed)
    X = rs.randint(0, 4096, size=(m, n)) / 1024.0
    X[rs.random_sample((m, n)) < 0.33] = 0.0
    p, q = rs.choice([0.5, 1.0, 2.0], m), rs.choice([0.5, 1.0, 2.0], n)
    dl, dr = rs.randint(0, 64, m) / 16.0, rs.randint(0, 64, n) / 16.0
    dl[rs.random_sample(m) < 0.3] = 0.0
    dr[rs.random_sample(n) < 0.3] = 0.0
    dl[m // 4:m // 2] = 0.0
    k = min(m, n, 8)
    p[:k] = q[:k] = 1.0
    p[-1] = q[-1] = 1.0
    dr[:k] = dl[:k] = rs.randint(1, 64, k) / 16.0
    if m > 1 and n > 1:
        dl[-1] = dr[-1] = 0.0
        d = float(p @ dl - q @ dr)          # exact
        if d > 0:
            dr[-1] = d
        else:
            dl[-1] = -d
    if zero:
        dl[:], dr[:] = 0.0, 0.0
    a0, b0 = (q[None, :] * X).sum(axis=1), (p[:, None] * X).sum(axis=0)
    pr = dict(c=rs.randint(0, 64, m * n) / 64.0, p=p, q=q, l=a0 + dl, r=b0 + dr)
    if cls == 2:
        pr["phi"] = rs.randint(32, 96, m * n) / 64.0
        ms = float((pr["phi"].reshape((m, n), order="F") * X).sum())
        pr["mu"] = ms + 0.5 if not zero else ms
    return pr, X, dl, dr, rs


@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", SHAPES)
def test_dyadic_sums_bit_for_bit(cls, m, n):
    pr, X, dl, dr, rs = dyadic_state(cls, m, n, 23 * m + n + cls)
    ws = ws_of(cls, pr)
    inject(ws, X, rs)
    C, PHI = pr["c"].reshape((m, n), order="F"), pr.get("phi", np.zeros(m * n)).reshape((m, n), order="F")
    fs, ms = float((C * X).sum()), float((PHI * X).sum())
    for sigma, tau in ((None, None), orders(m, n, 5 * m + n)):
        ws.set_correction("north_west", sigma, tau)
        for side in (0, 1):
            what = (cls, m, n, side, sigma is None)
            got = ws.round_plan(0.0, side=side)
            assert same_bits(got["e"], dl) and same_bits(got["f"], dr) and got["se"] == pr["p"] @ dl, what
            ref = list_of(pr, got, sigma, tau)
            i, j, g = assert_list(ws, ref, what)
            if sigma is None and min(m, n) >= 8:
                assert len(np.intersect1d(ref["R"][1:-1], ref["C"][1:-1])) > 0, what       # exact ties R_k = C_s
            assert np.array_equal((pr["q"][None, :] * NW.dense(m, n, i, j, g)).sum(axis=1), dl * got["sf"]), what
            assert np.array_equal((pr["p"][:, None] * NW.dense(m, n, i, j, g)).sum(axis=0), dr * got["se"]), what
            cc, cp = float((C[i, j] * g).sum()), float((PHI[i, j] * g).sum())
            assert same_bits(got["cc"], cc) and same_bits(got["fs"], fs), (what, got["cc"], cc)
            with np.errstate(divide="ignore", invalid="ignore"):
                if cls == 1:
                    theta, t = 1.0, (1.0 / got["se"] if got["se"] > 0 else 0.0)
                else:
                    assert same_bits(got["cp"], cp) and same_bits(got["ms"], ms), what
                    theta, t = 1.0, np.float64(pr["mu"] - ms) / np.float64(cp)
                fval = theta * fs + t * cc
            assert same_bits(got["t"], t) and same_bits(got["fval"], fval), (what, got["fval"], fval)
    ws.close()


@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", [(1, 1), (65, 33), (1000, 90)])
def test_no_deficit_no_entry(cls, m, n):
    """all deficits 0: count = 0 and every field as the rank-one term's call gives it"""
    pr, X, dl, dr, rs = dyadic_state(cls, m, n, 29 * m + n + cls, zero=True)
    ws = ws_of(cls, pr)
    inject(ws, X, rs)
    for side in (0, 1):
        want = ws.round_plan(0.0, side=side)
        info = ws.correction_info()
        assert (info["mode"], info["form"], info["count"]) == (0, 0, 0) and np.isnan(info["cc"] + info["fval"]).all()
        ws.set_correction("north_west", *orders(m, n, 3))
        got = ws.round_plan(0.0, side=side)
        assert same_result(got, want), (cls, m, n, side)
        assert got["t"] == 0.0 and got["cc"] == 0.0 and (got["e"] == 0).all() and (got["f"] == 0).all()
        info = ws.correction_info()
        assert (info["mode"], info["form"], info["count"]) == (1, 1, 0) and len(ws.correction_entries()[0]) == 0
        ws.set_correction("rank_one")
    ws.close()


# ---------------------------------------------------------------------------
# 2. mode 0 is what it was
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", [(65, 150), (300, 16), (1000, 90)])
def test_mode_0_unchanged(cls, m, n):
    pr = problem(cls, m, n, seed=5, pq_random=True)
    rs = np.random.RandomState(m + n)
    X = noisy_plan(cls, pr, m, n, 0.3, rs)
    plain, setting = ws_of(cls, pr), ws_of(cls, pr)
    for ws in (plain, setting):
        inject(ws, X, np.random.RandomState(7))
    sigma, tau = orders(m, n, 9)
    setting.set_correction("north_west", sigma, tau)
    nw = [setting.round_plan(0.0, side=s) for s in (0, 1)]
    setting.set_correction("rank_one", sigma, tau)       # back to mode 0, the orders kept
    for side in (0, 1):
        a, b = plain.round_plan(0.0, side=side), setting.round_plan(0.0, side=side)
        assert same_result(a, b), (cls, m, n, side)
        (sa, xa), (sb, xb) = TR.x_out_of(plain, side=side), TR.x_out_of(setting, side=side)
        assert same_result(sa, sb) and same_result(sa, a, TR.STAT_KEYS) and same_bits(xa, xb)
        assert setting.correction_info()["form"] == 0 and len(setting.correction_entries()[0]) == 0
        for key in KEPT:                                  # mode 1 leaves everything before the correction alone
            assert same_bits(nw[side][key], a[key]), (cls, m, n, side, key)
        assert nw[side]["ok"] == a["ok"] == 1
    ga, gb = plain.gap_probe(0.0, vectors=True), setting.gap_probe(0.0, vectors=True)
    assert same_result(ga["upper"], gb["upper"]) and ga["upper"]["side"] == gb["upper"]["side"]
    assert all(same_bits(ga["lower"][k], gb["lower"][k]) for k in ga["lower"]) and same_bits(ga["gap"], gb["gap"])
    plain.close()
    setting.close()


# ---------------------------------------------------------------------------
# 3. feasibility and value
# ---------------------------------------------------------------------------
USED = {}


@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", SHAPES)
def test_rounded_plan_is_feasible(cls, m, n):
    worst = 0.0
    for pq_random in (False, True):
        pr = problem(cls, m, n, seed=3, pq_random=pq_random)
        ws = ws_of(cls, pr)
        ws.set_correction("north_west", *orders(m, n, 11 + m))
        C = pr["c"].reshape((m, n), order="F").astype(LD)
        for noise in (1e-6, 0.3):
            rs = np.random.RandomState(1000 * m + 10 * n + cls)
            u, _, _ = inject(ws, noisy_plan(cls, pr, m, n, noise, rs), rs)
            for side in (0, 1):
                what = "cls %d %dx%d pq %d noise %g side %d" % (cls, m, n, pq_random, noise, side)
                res = ws.round_plan(0.0, side=side)
                assert res["ok"] == 1, (what, res)
                i, j, g = ws.correction_entries()
                Xh = NW.rebuild(u, m, n, 0.0, res, i, j, g)
                worst = max(worst, R.check_feasible(cls, pr, m, n, Xh, what))
                err = float(abs(LD(res["fval"]) - (C * Xh).sum()))
                bar = R.gamma(2 * m * n + 16) * float((np.abs(C) * np.abs(Xh)).sum())
                print("%s: fval err %.3e bar %.3e" % (what, err, bar))
                assert err <= bar, (what, err, bar)
        ws.close()
    USED[(cls, m, n)] = worst
    print("cls %d %dx%d: used fraction of the feasibility bound %.4f" % (cls, m, n, worst))
    assert worst <= 1.0


# ---------------------------------------------------------------------------
# 4. mode 2
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", [(63, 17), (65, 150), (1000, 90)])
def test_cheaper_is_the_smaller(cls, m, n):
    rs = np.random.RandomState(m * n + cls)
    xs, ys = rs.random_sample((m, 2)), rs.random_sample((n, 2))
    pr = problem(cls, m, n, seed=4, pq_random=True)
    kw = dict(mu=pr["mu"], phi=pr["phi"]) if cls == 2 else {}
    ws = ipd().APDWorkspace.from_points(cls, xs, ys, pr["r"], pr["l"], pr["p"], pr["q"], **kw)
    inject(ws, noisy_plan(cls, pr, m, n, 0.3, rs), rs)
    forms = set()
    for order in (ipd().projection_order(xs, ys), orders(m, n, 2), (None, None)):
        for side in (0, 1):
            res = {}
            for mode in ("rank_one", "north_west", "cheaper"):
                ws.set_correction(mode, *order)
                res[mode] = ws.round_plan(0.0, side=side)
            info = ws.correction_info()
            r1, nw, ch = res["rank_one"], res["north_west"], res["cheaper"]
            assert r1["ok"] == nw["ok"] == 1
            assert ch["fval"] == min(r1["fval"], nw["fval"]), (cls, m, n, side, r1["fval"], nw["fval"], ch["fval"])
            used = nw if info["form"] == 1 else r1
            assert same_result(ch, used), (cls, m, n, side, info)
            assert info["mode"] == 2 and same_bits(info["cc"], (r1["cc"], nw["cc"]))
            assert same_bits(info["fval"], (r1["fval"], nw["fval"]))
            assert info["count"] == (len(ws.correction_entries()[0]) if info["form"] else 0)
            assert (info["count"] > 0) == (info["form"] == 1)
            forms.add(info["form"])
            print("cls %d %dx%d side %d: cc rank-one %.6e north-west %.6e -> form %d"
                  % (cls, m, n, side, r1["cc"], nw["cc"], info["form"]))
    assert forms == {0, 1} or forms == {1}, forms
    ws.close()


def test_gap_rule_stops_no_later():
    """tests/test_gpu_gap_rule.py's small case: the threshold is the geometric mean of two consecutive gaps of a
    record-only run under mode 0; under mode 2 every probe's upper bound is at most mode 0's, so it stops no later"""
    from tests import test_gpu_gap_rule as TG
    cls, m, n = TG.CASES[0]
    ws, rng = TG.started(cls, m, n, gap_tol=0.0)
    ws.run(TG.amg(cls), rng, iters=TG.NSTEP)
    gaps = [r["gap"] for r in ws.gap_records()]
    ws.close()
    tol = float(np.sqrt(gaps[5] * gaps[6]))
    stops = {}
    for mode in ("rank_one", "cheaper"):
        ws, rng = TG.started(cls, m, n)
        ws.set_correction(mode, *orders(m, n, 1))
        ws.set_gap_rule(gap_tol=tol)
        res = ws.run(TG.amg(cls), rng, iters=TG.NSTEP + 3)
        stops[mode] = (res["k"], res["gap_stop"], [r["upper"] for r in ws.gap_records()])
        assert ws.correction_info()["mode"] == (0 if mode == "rank_one" else 2)
        ws.close()
    print("gap rule: threshold %.4e, stops %s" % (tol, {k: v[:2] for k, v in stops.items()}))
    assert stops["rank_one"][1] is True and stops["cheaper"][1] is True
    assert stops["cheaper"][0] <= stops["rank_one"][0]
    assert all(b <= a for a, b in zip(stops["rank_one"][2], stops["cheaper"][2]))


# ---------------------------------------------------------------------------
# 5. against the linear program
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["north_west", "cheaper"])
@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", [(24, 24), (37, 29)])
def test_against_the_linear_program(cls, m, n, mode):
    pytest.importorskip("scipy")
    pr = problem(cls, m, n, seed=12, pq_random=True)
    fstar, xstar = TR.optimum(cls, pr, m, n)
    ws = ws_of(cls, pr)
    ws.set_correction(mode, *orders(m, n, 8))
    rs = np.random.RandomState(21)
    for factor in (1.0, 1.001, 0.999):
        inject(ws, factor * xstar.reshape((m, n), order="F") + 1e-6 * rs.standard_normal((m, n)), rs)
        for side in (0, 1):
            res = ws.round_plan(0.0, side=side, vectors=False)
            print("cls %d %dx%d %s factor %g side %d: fval - f* %.3e" % (cls, m, n, mode, factor, side,
                                                                         res["fval"] - fstar))
            assert res["ok"] == 1 and res["fval"] >= fstar - 1e-12 * abs(fstar), (factor, side, res["fval"], fstar)
    ws.close()


# ---------------------------------------------------------------------------
# 6. install
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("m,n", [(65, 150), (300, 16), (1000, 90)])
def test_install_keeps_the_plan_sparse(cls, m, n):
    pr = problem(cls, m, n, seed=9)
    ws = ws_of(cls, pr)
    ws.set_correction("north_west", *orders(m, n, 6))
    rs = np.random.RandomState(m * n + cls)
    mn = m * n
    # permutation-like support plus noise below the threshold of the clamp: most entries are dropped
    X = np.zeros((m, n))
    X[np.arange(max(m, n)) % m, np.arange(max(m, n)) % n] = 0.5 * min(pr["l"].min(), pr["r"].min())
    X = X + 1e-9 * rs.standard_normal((m, n))
    tol = 1e-6
    for side in (0, 1):
        u, v, lam = inject(ws, X, rs)
        nnz = int((R.clamp(X, tol)[0] > 0).sum())
        st0, xh = TR.x_out_of(ws, tol=tol, side=side)
        st, xo = TR.x_out_of(ws, tol=tol, side=side, install=True)
        i, j, g = ws.correction_entries()
        assert same_result(st0, st) and same_bits(xh, xo) and st["ok"] == 1 and len(i) > 0
        u1, v1, lam1, bk1 = ws.state()
        assert same_bits(u1[:mn], xh) and same_bits(v1[:mn], xh) and same_bits(lam1, lam) and bk1 == 0.37
        P, stats, ax = ws.plan(0.0, stats=True)
        assert P.nnz <= nnz + m + n - 1 and P.nnz == int((xh != 0).sum()), (cls, m, n, side, P.nnz, nnz)
        Xh = xh.reshape((m, n), order="F").astype(LD)
        rb, cb = R.feasibility_bounds(pr, m, n)
        if cls == 2:
            y, z = u1[mn:mn + n], u1[mn + n:]
            assert same_bits(v1[mn:mn + n], y) and same_bits(v1[mn + n:], z)
            R.check_feasible(2, pr, m, n, Xh, "installed", yz=(y, z))      # the slacks close the marginals
        else:
            R.check_feasible(1, pr, m, n, Xh, "installed")
        again = ws.round_plan(0.0, side=side)
        assert again["ok"] == 1 and again["viol_in"] <= float(pr["p"] @ rb + pr["q"] @ cb)
    ws.close()


def test_x_out_is_one_multiply_and_one_add():
    cls, m, n = 1, 65, 33
    pr = problem(cls, m, n, seed=2, pq_random=True)
    ws = ws_of(cls, pr)
    sigma, tau = orders(m, n, 4)
    ws.set_correction("north_west", sigma, tau)
    rs = np.random.RandomState(3)
    u, _, _ = inject(ws, noisy_plan(cls, pr, m, n, 0.3, rs), rs)
    st, xh = TR.x_out_of(ws, side=0)
    res = ws.round_plan(0.0, side=0)
    i, j, g = ws.correction_entries()
    Xp = R.clamp(u[:m * n].reshape((m, n), order="F"), 0.0)[0]
    want = res["theta"] * ((res["rho"][:, None] * Xp) * res["kappa"][None, :])
    want[i, j] = want[i, j] + res["t"] * g
    assert same_bits(xh.reshape((m, n), order="F"), want)
    ws.close()


def test_install_without_a_repair_is_refused():
    """tests/test_gpu_round.py's state without a repair -- class 2 with mu above what the slacks admit, t*Se > 1:
    ok = 0, IPD_E_NUMERIC, nothing written"""
    L = lib_mod()
    cls, m, n = 2, 65, 33
    pr = problem(cls, m, n, seed=6, pq_random=True)
    pr["mu"] = 4.0 * float((pr["phi"].reshape((m, n), order="F") * np.outer(pr["l"], pr["r"])).sum()) + 10.0
    ws = ws_of(cls, pr)
    ws.set_correction("north_west", *orders(m, n, 5))
    rs = np.random.RandomState(8)
    X = 0.5 * np.outer(pr["l"], pr["r"]) / max(pr["q"] @ pr["r"], pr["p"] @ pr["l"])
    u, v, lam = inject(ws, np.where(rs.random_sample((m, n)) < 0.1, -X, X), rs)
    res = ws.round_plan(0.0, side=0)
    assert res["ok"] == 0 and res["theta"] == 1.0 and res["t"] * min(res["se"], res["sf"]) > 1.0, res
    assert ws.correction_info()["count"] > 0
    buf = L.DeviceBuffer.from_array(np.full(m * n, SENT))
    with pytest.raises(L.IpdError) as ei:
        ws.round_plan_dev(install=True, x_out=buf)
    assert ei.value.code == L.IPD_E_NUMERIC
    assert (buf.to_array(np.float64, m * n) == SENT).all()
    buf.free()
    with pytest.raises(L.IpdError):
        ws.gap_probe(0.0, install=True)
    u1, v1, lam1, _ = ws.state()
    assert same_bits(u1, u) and same_bits(v1, v) and same_bits(lam1, lam)
    ws.close()


# ---------------------------------------------------------------------------
# 7. the same bits across routes and sources
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [1, 2])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_cost_sources_and_routes_agree(cls, d):
    L = lib_mod()
    m, n = 65, 150
    rs = np.random.RandomState(40 + d)
    xs, ys = rs.random_sample((m, d)), rs.random_sample((n, d))
    r, l = rs.random_sample(n), rs.random_sample(m)
    p, q = 0.5 + rs.random_sample(m), 0.5 + rs.random_sample(n)
    kw = dict(mu=0.65 * min(r.sum(), l.sum()), phi=0.5 + rs.random_sample(m * n)) if cls == 2 else {}
    pr = dict(r=r, l=l, p=p, q=q, **kw)
    if cls == 1:
        pr["l"] = l = l * (r @ q) / (l @ p)
    Xd = noisy_plan(cls, pr, m, n, 0.3, rs)
    order = ipd().projection_order(xs, ys)
    for metric, scale in (("sqeuclidean", False), ("cityblock", True)):
        stored = ipd().APDWorkspace.from_points(cls, xs, ys, r, l, p, q, metric=metric, scale=scale, **kw)
        free = ipd().APDWorkspace.from_points(cls, xs, ys, r, l, p, q, metric=metric, scale=scale, matrix_free=True,
                                              **kw)
        host = ipd().APDWorkspace(cls, stored.cost().reshape(-1, order="F"), r, l, p, q, **kw)
        for ws in (host, stored, free):
            inject(ws, Xd, np.random.RandomState(5))
            ws.set_correction("north_west", *order)
        for side in (0, 1):
            got, lists, outs = [], [], []
            for ws in (host, stored, free):
                got.append(ws.round_plan(0.0, side=side))
                lists.append(ws.correction_entries())
                st, xo = TR.x_out_of(ws, side=side)                  # the device entry; a second call
                assert same_result(st, got[-1], TR.STAT_KEYS), (metric, side)
                assert all(np.array_equal(a, b) for a, b in zip(lists[-1][:2], ws.correction_entries()[:2]))
                assert same_bits(lists[-1][2], ws.correction_entries()[2])
                outs.append(xo)
            for k in (1, 2):
                assert same_result(got[0], got[k]), (metric, scale, side, k)
                assert np.array_equal(lists[0][0], lists[k][0]) and np.array_equal(lists[0][1], lists[k][1])
                assert same_bits(lists[0][2], lists[k][2]) and same_bits(outs[0], outs[k])
            assert got[0]["ok"] == 1 and got[0]["cc"] > 0
        # the bracket's upper is round_plan of its side, and its list the list of that side
        for ws in (host, free):
            br = ws.gap_probe(0.0, vectors=True)
            li = ws.correction_entries()
            side = br["upper"]["side"]
            want = ws.round_plan(0.0, side=side)
            assert same_result(br["upper"], want), (metric, side)
            lw = ws.correction_entries()
            assert np.array_equal(li[0], lw[0]) and np.array_equal(li[1], lw[1]) and same_bits(li[2], lw[2])
            other = ws.round_plan(0.0, side=1 - side)
            assert (want["ok"], -want["fval"]) >= (other["ok"], -other["fval"])
            # the device twin of the entries
            cnt = ctypes.c_int64()
            bi, bj = (L.DeviceBuffer.from_array(np.full(len(lw[0]), -7, dtype=np.int32)) for _ in range(2))
            bg = L.DeviceBuffer.from_array(np.full(len(lw[0]), SENT))
            ws.round_plan(0.0, side=side)
            assert L.lib.ipd_apd_correction_entries_dev(ws.handle, bi.ptr, bj.ptr, bg.ptr, len(lw[0]),
                                                        ctypes.byref(cnt)) == 0
            assert cnt.value == len(lw[0]) and np.array_equal(bi.to_array(np.int32, cnt.value), lw[0])
            assert np.array_equal(bj.to_array(np.int32, cnt.value), lw[1])
            assert same_bits(bg.to_array(np.float64, cnt.value), lw[2])
            for b in (bi, bj, bg):
                b.free()
        for ws in (host, stored, free):
            ws.close()


# ---------------------------------------------------------------------------
# 8. errors and the drivers' keywords
# ---------------------------------------------------------------------------
def test_errors_keep_the_setting_and_write_nothing():
    L = lib_mod()
    lib, E = L.lib, L.IPD_E_ARG
    m, n = 37, 5
    pr = problem(1, m, n, seed=13)
    ws = ws_of(1, pr)
    rs = np.random.RandomState(14)
    inject(ws, noisy_plan(1, pr, m, n, 0.3, rs), rs)
    sigma, tau = orders(m, n, 1)
    ws.set_correction("north_west", sigma, tau)
    want = ws.round_plan(0.0)
    lw = ws.correction_entries()
    h = ws.handle
    dup = sigma.copy()
    dup[1] = dup[0]
    for name, args in (("NULL h", (None, 1, None, None)), ("mode -1", (h, -1, None, None)),
                       ("mode 3", (h, 3, None, None)), ("row dup", (h, 0, dup.ctypes.data, None)),
                       ("row range", (h, 1, (sigma + 1).ctypes.data, None)),
                       ("row negative", (h, 1, (sigma - 1).ctypes.data, None)),
                       ("col range", (h, 2, None, (tau + 1).ctypes.data))):
        keep = [a for a in (sigma + 1, sigma - 1, tau + 1)]     # (alive during the call)
        assert lib.ipd_apd_set_correction(*args) == E, name
        del keep
    for bad in (dict(mode="dense"), dict(mode="north_west", row_order=np.arange(m + 1)),
                dict(mode="north_west", col_order=np.zeros(n))):
        with pytest.raises(ValueError):
            ws.set_correction(**bad)
    with pytest.raises(L.IpdError):
        ws.set_correction("north_west", np.zeros(m, dtype=np.int64), None)
    got = ws.round_plan(0.0)                                     # the setting in force stayed
    assert same_result(got, want) and ws.correction_info()["mode"] == 1
    assert all(np.array_equal(a, b) for a, b in zip(ws.correction_entries()[:2], lw[:2]))
    # the entries and the info: NULL arguments, a negative cap; outputs untouched
    cnt = ctypes.c_int64(-5)
    i, j, g = np.full(m + n, -7, dtype=np.int32), np.full(m + n, -7, dtype=np.int32), np.full(m + n, SENT)
    for name, args in (("NULL h", (None, i.ctypes.data, j.ctypes.data, g.ctypes.data, m + n, ctypes.byref(cnt))),
                       ("NULL count", (h, i.ctypes.data, j.ctypes.data, g.ctypes.data, m + n, None)),
                       ("cap < 0", (h, i.ctypes.data, j.ctypes.data, g.ctypes.data, -1, ctypes.byref(cnt)))):
        assert lib.ipd_apd_correction_entries(*args) == E, name
        assert lib.ipd_apd_correction_entries_dev(*((args[0], None, None, None) + args[4:])) == E, name
        assert cnt.value == -5 and (i == -7).all() and (j == -7).all() and (g == SENT).all(), name
    info = L.ipd_correction_info()
    assert lib.ipd_apd_correction_info(None, ctypes.byref(info)) == E and lib.ipd_apd_correction_info(h, None) == E
    # a cap below the count: the first entries, and the full count
    assert lib.ipd_apd_correction_entries(h, i.ctypes.data, None, g.ctypes.data, 2, ctypes.byref(cnt)) == 0
    assert cnt.value == len(lw[0]) > 2 and np.array_equal(i[:2], lw[0][:2]) and (i[2:] == -7).all()
    assert same_bits(g[:2], lw[2][:2]) and (g[2:] == SENT).all() and (j == -7).all()
    # finite gama stays unsupported under every mode
    wg = ws_of(1, pr, gama=0.625)
    inject(wg, noisy_plan(1, pr, m, n, 0.3, rs), rs)
    for mode in ("north_west", "cheaper"):
        wg.set_correction(mode)
        with pytest.raises(L.IpdError) as ei:
            wg.round_plan()
        assert ei.value.code == L.IPD_E_UNSUPPORTED
    wg.close()
    ws.close()


def test_driver_keywords():
    m = n = 24
    pr = problem(1, m, n, seed=12)
    args = (pr["c"], pr["r"], pr["l"], pr["p"], pr["q"])
    plain = ipd().APD_SsN_Class1(*args, maxit=2, bracket=True)
    rank = ipd().APD_SsN_Class1(*args, maxit=2, bracket=True, correction="rank_one")
    assert set(rank) - set(plain) == {"correction"} and rank["correction"]["form"] == 0
    assert same_result(plain["bracket"]["upper"], rank["bracket"]["upper"]) and same_bits(plain["xk"], rank["xk"])
    sigma, tau = orders(m, n, 3)
    nw = ipd().APD_SsN_Class1(*args, maxit=2, bracket=True, correction="north_west", correction_order=(sigma, tau))
    assert nw["correction"]["form"] == 1 and nw["correction"]["count"] > 0 and same_bits(plain["xk"], nw["xk"])
    for key in KEPT:
        if key in plain["bracket"]["upper"] and plain["bracket"]["upper"]["side"] == nw["bracket"]["upper"]["side"]:
            assert same_bits(plain["bracket"]["upper"][key], nw["bracket"]["upper"][key]), key
    with pytest.raises(ValueError):
        ipd().APD_SsN_Class1(*args, maxit=1, correction="north_west", correction_order="projection")
    with pytest.raises(ValueError):
        ipd().APD_SsN_Class1(*args, maxit=1, correction="sparse")
    pr2 = problem(2, m, n, seed=12)
    two = ipd().APD_SsN_Class2(pr2["c"], pr2["r"], pr2["l"], pr2["p"], pr2["q"], pr2["mu"], pr2["phi"], maxit=1,
                               bracket=True, correction="cheaper")
    assert two["bracket"]["upper"]["ok"] == 1 and two["correction"]["mode"] == 2
    rs = np.random.RandomState(15)
    xs, ys = rs.random_sample((m, 2)), rs.random_sample((n, 2))
    mu = 0.65 * min(pr["r"].sum(), pr["l"].sum())
    outs = []
    for free in (False, True):
        out = ipd().APD_SsN_Class2_points(xs, ys, pr["r"], pr["l"], pr["p"], pr["q"], mu, maxit=1, matrix_free=free,
                                          bracket=True, correction="north_west", correction_order="projection")
        outs.append(out)
        assert out["bracket"]["upper"]["ok"] == 1 and out["correction"]["form"] == 1
    assert same_result(outs[0]["bracket"]["upper"], outs[1]["bracket"]["upper"])
    one = ipd().APD_SsN_Class1_points(xs, ys, pr["r"], pr["l"], pr["p"], pr["q"], maxit=3, gap_rel=1e-9,
                                      correction="cheaper", correction_order="projection")
    assert one["correction"]["mode"] == 2 and len(one["gap_records"]) == 3
    assert "correction" not in ipd().APD_SsN_Class1_points(xs, ys, pr["r"], pr["l"], pr["p"], pr["q"], maxit=1)
    # projection_order: stable argsorts along the first principal axis of the union
    line = np.stack([np.array([3.0, 1.0, 2.0, 1.0]), np.zeros(4)], axis=1)
    ro, co = ipd().projection_order(line, line[:2] + 10.0)
    assert ro.tolist() in ([1, 3, 2, 0], [0, 2, 1, 3]) and sorted(co.tolist()) == [0, 1] and ro.dtype == np.int32
