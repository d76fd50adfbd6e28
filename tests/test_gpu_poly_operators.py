"""The polynomial operators the resident kernels read, read back exactly as packed (ipd_amg_packed_operator)
and compared entrywise with the numpy restatement of their algebra (tests/test_poly_form_algebra.py, which
ties it to the oracle's smoothing loops, AMG/MG_Vcycle.m:14-41):

  * form 128 -- level 2 of k_resident<16,16,0,true> composed over a whole visit (amg_attach_poly2,
    k_bpoly_compose): the operator bench.py times, at nu = 5;
  * form 64 -- level 3 / 4 in the row layout of k_resident's `three` mode and of the mask-form kernel's deep
    mode (checked in tests/test_gpu_resident_remote.py and tests/test_gpu_resident_deep.py with the helpers
    below, on the captured Newton systems those files build).

Bars: 1e-11 (1 + max|ref|) per block, 1e-9 (1 + max|ref|) for the rank-one factors (w, -T1 w), as for the
images' form 16, with two exceptions, both from the isnsp term u 1'A of S (u ~ 1/xx, which cancels):
  * the composed factors: 5e-9 (1 + max|ref|) for wB, 5e-8 (1 + |ref|) for ws.  Measured on the metric
    system: wB misses numpy's by 1.45e-9 against max|wB| = 0.13, ws by 1.11e-8 against |ws| = 1.0;
  * the blocks scaled by D^-1 (M2a, B), whose entries are ~1e-5: 5e-10 max|ref| (with the "1 +" six digits of
    them would go unchecked; still 4e3 x tighter than that bar).  Measured: B of the metric system misses
    numpy's by 1.6e-15 against max|B| = 2.5e-5 (6.4e-11 relative, 7.8x below the bar), B of the ragged systems
    by less than 1e-11 relative.  D^-1 scaled by 1 + 1e-6 moves M2a of the metric system by 1.6e-7 relative:
    320 bars.
Every check proves its power: the operator built with nu - 1, nu + 1, isnsp flipped and D^-1 scaled by 1 + 1e-6
must each miss the packed one by at least 100 x the bar."""
from ctypes import POINTER, byref, c_double, c_int32, c_int64

import numpy as np
import pytest
import scipy.sparse as sp

import bench
from oracle import ipd_oracle as O
from tests import problems as PR
from tests.test_poly_form_algebra import composed_operators, stacked_operators

RANK_ONE = ("w", "W_low", "wB", "ws")
SCALED = ("M2a", "B")      # D^-1-scaled blocks: bar relative to their own size


def packed_layout(h, k, form):
    """(ld, seg, n, nc) of level k's operator in `form`: the hook's size query (out = NULL, cap = 0)."""
    from codes_of_ipd_ssn_amg_method_amd import _lib
    ld, seg, n, nc = c_int32(), c_int32(), c_int32(), c_int32()
    _lib.check(_lib.lib.ipd_amg_packed_operator(h.handle, c_int32(k), c_int32(form), None, c_int64(0),
                                                byref(ld), byref(seg), byref(n), byref(nc)))
    return ld.value, seg.value, n.value, nc.value


def packed_raw(h, k, form, cap):
    """The `cap` doubles the hook copies out for level k in `form`, and (ld, seg, n, nc)."""
    from codes_of_ipd_ssn_amg_method_amd import _lib
    ld, seg, n, nc = c_int32(), c_int32(), c_int32(), c_int32()
    buf = np.full(cap, np.nan)
    _lib.check(_lib.lib.ipd_amg_packed_operator(h.handle, c_int32(k), c_int32(form),
                                                buf.ctypes.data_as(POINTER(c_double)), c_int64(cap),
                                                byref(ld), byref(seg), byref(n), byref(nc)))
    return buf, (ld.value, seg.value, n.value, nc.value)


def packed_operator(h, k, form):
    """(rows [N + Nc][ld], factors W [N + Nc], seg, N, Nc) of level k as packed for `form` (64 / 128)."""
    LD, S, N, Nc = packed_layout(h, k, form)
    assert (N, Nc) == (h.level_dims(k)[0], h.level_dims(k + 1)[0])
    assert N <= S and 2 * S + Nc <= LD, (N, Nc, S, LD)
    buf, lay = packed_raw(h, k, form, (N + Nc) * (LD + 1))
    assert lay == (LD, S, N, Nc)
    rows = buf[:(N + Nc) * LD].reshape(N + Nc, LD)
    W = buf[(N + Nc) * LD:]
    assert np.isfinite(rows).all() and np.isfinite(W).all()
    return rows, W, S, N, Nc


def check_image_form_hook(h, k):
    """Form 16 through the hook: the layout query and the copy are ipd_amg_poly_operator's."""
    from codes_of_ipd_ssn_amg_method_amd import _lib
    LD, S, N, Nc = packed_layout(h, k, 16)
    assert (N, Nc) == (h.level_dims(k)[0], h.level_dims(k + 1)[0]) and S == -(-N // 8) * 8
    need = LD * (2 * S + -(-Nc // 8) * 8 + 1)
    got, lay = packed_raw(h, k, 16, need)
    assert lay == (LD, S, N, Nc)
    want = np.zeros(need)
    ld, nn, nc = c_int32(), c_int32(), c_int32()
    _lib.check(_lib.lib.ipd_amg_poly_operator(h.handle, c_int32(k), want.ctypes.data_as(POINTER(c_double)),
                                              c_int64(need), byref(ld), byref(nn), byref(nc)))
    assert (ld.value, nn.value, nc.value) == (LD, N, Nc) and np.array_equal(got, want)
    seg = c_int32()
    assert _lib.lib.ipd_amg_packed_operator(h.handle, c_int32(k), c_int32(16), got.ctypes.data_as(POINTER(c_double)),
                                            c_int64(need - 1), byref(ld), byref(seg), byref(nn), byref(nc)) == -1


def bar(name, want):
    tol = {"wB": 5e-9, "ws": 5e-8}.get(name, 1e-9 if name in RANK_ONE else 1e-11)
    if name in SCALED:
        return 5e-10 * np.abs(want).max()
    return tol * (1.0 + np.abs(want).max())


def check_operator(got, ref, variants):
    """got within the bar of ref, block by block; each variant at least 100 bars away from got."""
    for name in ref:
        d = float(np.abs(np.asarray(got[name]) - np.asarray(ref[name])).max())
        assert d <= bar(name, ref[name]), (name, d, bar(name, ref[name]))
    for label, v in variants.items():
        miss = max(float(np.abs(np.asarray(got[k]) - np.asarray(v[k])).max()) / bar(k, ref[k]) for k in ref)
        assert miss >= 100.0, (label, miss)


def level_operands(h, k):
    A = h.A(k).toarray()
    P = h.P(k + 1).toarray()
    return A, P, 0.5 / np.diag(A)          # Jacobi levels: Class_AMG.m:60-62


def variants_of(build, A, P, dinv, isnsp, nu):
    return {"nu-1": build(A, P, dinv, isnsp, nu - 1) if nu > 1 else None,
            "nu+1": build(A, P, dinv, isnsp, nu + 1),
            "isnsp flipped": build(A, P, dinv, 1 - isnsp, nu),
            "dinv (1 + 1e-6)": build(A, P, dinv * (1.0 + 1e-6), isnsp, nu)}


def check_rows_operator(h, k, isnsp, nu):
    """Form 64: level k in the row layout [M2a | M1 | M1 P] over the stacked restriction rows."""
    rows, W, S, N, Nc = packed_operator(h, k, 64)
    got = {"M2a": rows[:N, :N], "M1": rows[:N, S:S + N], "Mc": rows[:N, 2 * S:2 * S + Nc], "w": W[:N],
           "Mr_low": rows[N:, :N], "Me_low": rows[N:, S:S + N], "W_low": W[N:]}
    A, P, dinv = level_operands(h, k)
    ref = stacked_operators(A, P, dinv, isnsp, nu)
    variants = {kk: v for kk, v in variants_of(stacked_operators, A, P, dinv, isnsp, nu).items() if v is not None}
    check_operator(got, ref, variants)
    # the padding: the deep mode's passes read whole segments (columns beyond N of Mr / Me, all of Mc's)
    assert not rows[:, N:S].any() and not rows[:, S + N:2 * S].any()
    assert not rows[:N, 2 * S + Nc:].any() and not rows[N:, 2 * S:].any()


def check_composed_operator(h, isnsp, nu):
    """Form 128: level 2 composed over a visit: B at the M1 segment, mp at column 2 seg, s in row N, [wB; ws]."""
    rows, W, S, N, Nc = packed_operator(h, 2, 128)
    assert Nc == 1
    got = {"B": rows[:N, S:S + N], "wB": W[:N], "mp": rows[:N, 2 * S], "s": rows[N, :N], "ws": W[N],
           "M2a": rows[:N, :N]}
    A, P, dinv = level_operands(h, 2)

    def build(A_, P_, d_, i_, nu_):
        C = composed_operators(A_, P_, d_, i_, nu_)
        M = stacked_operators(A_, P_, d_, i_, nu_)
        C.update(M2a=M["M2a"])   # (row N's M1 segment, -T1 M1, is not read by the composed pass)
        return C
    ref = build(A, P, dinv, isnsp, nu)
    check_operator(got, ref, {kk: v for kk, v in variants_of(build, A, P, dinv, isnsp, nu).items() if v is not None})
    # the padding: zero beyond N in every segment, beyond mp in the Mc segment
    assert not rows[:, N:S].any() and not rows[:, S + N:2 * S].any()
    assert not rows[:N, 2 * S + 1:].any() and not rows[N, 2 * S:].any()


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ipd():
    import codes_of_ipd_ssn_amg_method_amd as m
    return m


def _options(n, isnsp=1):
    return dict(retol=1e-11, bigph=1, maxit=30, theta=0.25, smoth=5, cycle="v", isnsp=isnsp, inter=1, fnode=n)


def test_metric_composed_operator(ipd):
    """The operator bench.py times: the metric system (m = n = 1024, Bernoulli rho = 1, levels 2048 / 1024 / 1),
    nu = 5, with the mask transfers attached as bench.py does."""
    m = n = 1024
    s = bench.build_mask(m, n, "bernoulli", 1.0)
    Ae, f, guess, H0 = bench.build_newton_system(ipd, m, n, s)
    h = ipd.AMGHierarchy(Ae, _options(n), ipd.MatlabRand())
    assert h.attach_mask_transfers(np.ones(m), np.ones(n), bench.TK) and h.attach_level2_poly()
    assert h.level_sizes() == [2048, 1024, 1] and h.level_forms()[1] & 128
    check_composed_operator(h, 1, 5)
    h.close()


@pytest.mark.parametrize("m,n,rho,pq", [(700, 900, 1.0, True), (1000, 1000, 0.9, True)])
def test_ragged_composed_operators(ipd, m, n, rho, pq):
    """The composed systems of tests/test_gpu_bench_workload.py that take the composed form (N2 = 700 / 1000,
    below the 1024 the dense rows are walked to; random p and q; a mask with holes)."""
    s = PR.mask_bernoulli(m, n, rho, seed=5)
    pd = PR.make_prob(m, n, s, pq_random=pq)
    H0 = O.ASAt(s, pd["p"], pd["q"])
    Ae = sp.csr_matrix(O.build_Ae(H0, pd["T"], pd["p"], pd["q"], pd["bk1"], pd["tk"])[0])
    h = ipd.AMGHierarchy(Ae, _options(n), ipd.MatlabRand())
    assert h.level_sizes() == [m + n, m, 1], h.level_sizes()
    assert h.attach_level2_poly() and h.level_forms()[1] & 128
    check_composed_operator(h, 1, 5)
    h.close()


def test_undefined_forms_are_refused(ipd):
    """IPD_E_ARG for a form the level does not have and for forms the hook does not define."""
    from codes_of_ipd_ssn_amg_method_amd import _lib
    m, n = 700, 900
    s = PR.mask_bernoulli(m, n, 1.0, seed=5)
    pd = PR.make_prob(m, n, s, pq_random=True)
    H0 = O.ASAt(s, pd["p"], pd["q"])
    Ae = sp.csr_matrix(O.build_Ae(H0, pd["T"], pd["p"], pd["q"], pd["bk1"], pd["tk"])[0])
    h = ipd.AMGHierarchy(Ae, _options(n), ipd.MatlabRand())
    buf = np.zeros(8)
    ld, seg, nn, nc = c_int32(), c_int32(), c_int32(), c_int32()
    for k, form in ((2, 128), (2, 64), (3, 64), (2, 8), (2, 0), (1, 128), (0, 64)):
        rc = _lib.lib.ipd_amg_packed_operator(h.handle, c_int32(k), c_int32(form), buf.ctypes.data_as(POINTER(c_double)),
                                              c_int64(buf.size), byref(ld), byref(seg), byref(nn), byref(nc))
        assert rc == -1, (k, form, rc)              # IPD_E_ARG
    assert h.attach_level2_poly()
    rc = _lib.lib.ipd_amg_packed_operator(h.handle, c_int32(2), c_int32(128), buf.ctypes.data_as(POINTER(c_double)),
                                          c_int64(buf.size), byref(ld), byref(seg), byref(nn), byref(nc))
    assert rc == -1                                           # (buffer too small)
    h.close()
