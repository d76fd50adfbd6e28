"""The full-shape form of k_resident's composed instantiation (csrc/ipd_resident.h, template arguments DIAG and
FULL; resident_takes_full in csrc/ipd_resident_plan.h) on the metric's shape, m = n = 1024: F block, C block and
level 2 of 1024 rows, eight rows of each per workgroup, so every size, row range and mode flag is a constant of the
kernel.  Arithmetic and the order of every sum are the general form's, so every check is bit-equality: against the
same hierarchy options under IPD_RES_NO_FULL=1 (the general form), against a rerun, and -- the form with stamps and
test hook -- against the production launch.  Every test asks the library which variant its last launch took: the
forms under test would otherwise silently not run.  The full shape is M = 2048 by definition, so the tests use the
workload's size with one to three cycles."""
from ctypes import byref, c_double, c_int, c_int32, c_int64, create_string_buffer

import numpy as np
import pytest
import scipy.sparse as sp

import bench
from oracle import ipd_oracle as O
from tests import problems as PR

pytestmark = pytest.mark.gpu

COMPOSED = "k_resident<16,16,0,true>"


@pytest.fixture(scope="module")
def ipd():
    import codes_of_ipd_ssn_amg_method_amd as m
    return m


def options(n, smoth=5, isnsp=1, maxit=30, retol=1e-11):
    return dict(retol=retol, bigph=1, maxit=maxit, theta=0.25, smoth=smoth, cycle="v", isnsp=isnsp, inter=1, fnode=n)


def kernel_name(h):
    """(name, hand-offs of the last launch, its cycles)"""
    from codes_of_ipd_ssn_amg_method_amd import _lib
    buf = create_string_buffer(64)
    handoffs, cycles = c_int64(), c_int32()
    _lib.check(_lib.lib.ipd_amg_resident_kernel(h.handle, buf, c_int32(64), byref(handoffs), byref(cycles), None))
    return buf.value.decode(), handoffs.value, cycles.value


def variant(h):
    """(full, diag) of the hierarchy's last resident launch"""
    from codes_of_ipd_ssn_amg_method_amd import _lib
    full, diag = c_int32(-1), c_int32(-1)
    _lib.check(_lib.lib.ipd_amg_resident_variant(h.handle, byref(full), byref(diag)))
    return full.value, diag.value


def run_cycles(h, f, x0, cycles):
    from codes_of_ipd_ssn_amg_method_amd import _lib
    db = _lib.DeviceBuffer.from_array(f)
    dx = _lib.DeviceBuffer.from_array(x0)
    ms, bpc = c_double(), c_double()
    _lib.check(_lib.lib.ipd_amg_bench_cycles(h.handle, db.ptr, dx.ptr, c_int(cycles), byref(ms), byref(bpc)))
    return dx.to_array(np.float64, f.size)


def run_cycles_stamped(h, f, x0, cycles):
    """(iterate, the 32 stamp words) of ipd_amg_bench_resident_classes"""
    from codes_of_ipd_ssn_amg_method_amd import _lib
    db = _lib.DeviceBuffer.from_array(f)
    dx = _lib.DeviceBuffer.from_array(x0)
    ms = c_double()
    st = (c_int64 * 32)()
    _lib.check(_lib.lib.ipd_amg_bench_resident_classes(h.handle, db.ptr, dx.ptr, c_int(cycles), byref(ms), st))
    return dx.to_array(np.float64, f.size), [int(v) for v in st]


_systems = {}


def dense_system(ipd, m, n):
    """(Ae, f, guess, p, q, tk) of bench.py's system on the full m x n mask (rho = 1), built once."""
    if (m, n) not in _systems:
        s = bench.build_mask(m, n, "bernoulli", 1.0)
        Ae, f, guess, _ = bench.build_newton_system(ipd, m, n, s)
        _systems[(m, n)] = (Ae, f, guess, np.ones(m), np.ones(n), bench.TK)
    return _systems[(m, n)]


def holes_system(m, n, rho):
    """A mask with holes and random p, q, built as tests/test_gpu_resident_handoff.py's
    test_slow_first_cycle_against_oracle builds its systems."""
    key = (m, n, rho)
    if key not in _systems:
        s = PR.mask_bernoulli(m, n, rho, seed=5)
        pd = PR.make_prob(m, n, s, pq_random=True)
        H0 = O.ASAt(s, pd["p"], pd["q"])
        Ae = sp.csr_matrix(O.build_Ae(H0, pd["T"], pd["p"], pd["q"], pd["bk1"], pd["tk"])[0])
        f = np.concatenate([pd["q"], -pd["p"]]) * pd["z"]
        guess = pd["bk1"] * pd["tk"] * np.random.RandomState(4).random_sample(m + n)
        _systems[key] = (Ae, f, guess, pd["p"], pd["q"], pd["tk"])
    return _systems[key]


def hierarchy(ipd, monkeypatch, system, opts, env=(), poly2=True):
    """A hierarchy of the system with the mask transfers attached and level 2 composed, set up and attached under
    the switches `env` (they are read at set-up and at the attach calls)."""
    Ae, f, guess, p, q, tk = system
    for k, v in env:
        monkeypatch.setenv(k, v)
    h = ipd.AMGHierarchy(Ae, opts, ipd.MatlabRand())
    xm = h.attach_mask_transfers(p, q, tk)
    p2 = h.attach_level2_poly() if poly2 else False
    for k, _ in env:
        monkeypatch.delenv(k)
    return h, xm, p2


NO_FULL = (("IPD_RES_NO_FULL", "1"),)


@pytest.mark.parametrize("smoth", [5, 1])
def test_metric_system_full_form_is_the_general_form_bit_for_bit(ipd, monkeypatch, smoth):
    """The metric's system: the full-shape production form is taken (full = 1, diag = 0), and the iterates of one,
    two and three timed loop bodies and a Class_AMG solve of two iterations (maxit = 2, retol = 0: x, it, relk, rhok)
    equal the general form's under IPD_RES_NO_FULL=1.  smoth 5 and smoth 1 (one sweep per run: a run's first and
    last half sweep coincide)."""
    m = n = 1024
    sysm = dense_system(ipd, m, n)
    f, guess = sysm[1], sysm[2]
    opts = options(n, smoth=smoth, maxit=2, retol=0.0)
    hf, xm, p2 = hierarchy(ipd, monkeypatch, sysm, opts)
    assert xm and p2 and kernel_name(hf)[0] == COMPOSED, (hf.level_sizes(), kernel_name(hf))
    hg, xm, p2 = hierarchy(ipd, monkeypatch, sysm, opts, env=NO_FULL)
    assert xm and p2 and kernel_name(hg)[0] == COMPOSED
    for K in (1, 2, 3):
        a = run_cycles(hf, f, guess, K)
        assert variant(hf) == (1, 0)
        b = run_cycles(hg, f, guess, K)
        assert variant(hg) == (0, 0)
        assert np.all(np.isfinite(a)) and not np.array_equal(a, guess)
        assert np.array_equal(a, b), (smoth, K, np.max(np.abs(a - b)))
    xf, itf, relf, relkf, rhokf = hf.solve(f, guess)
    assert variant(hf) == (1, 0)
    xg, itg, relg, relkg, rhokg = hg.solve(f, guess)
    assert variant(hg) == (0, 0)
    assert itf == itg and itf >= 1
    assert np.array_equal(xf, xg)
    assert np.array_equal(np.asarray(relkf), np.asarray(relkg), equal_nan=True)
    assert np.array_equal(np.asarray(rhokf), np.asarray(rhokg), equal_nan=True)
    hf.close()
    hg.close()


HOLES_RHO = 0.8   # PR.mask_bernoulli(1024, 1024, 0.8, seed=5): the planner takes the composed form for it (asserted below)


def test_mask_with_holes_full_form_bit_for_bit(ipd, monkeypatch):
    """One 1024 x 1024 system with holes (rho 0.8) and random p, q, smoth 1: the full form is taken and one and two
    cycles are bit-equal to the general form."""
    m = n = 1024
    sysm = holes_system(m, n, HOLES_RHO)
    f, guess = sysm[1], sysm[2]
    opts = options(n, smoth=1)
    hf, xm, p2 = hierarchy(ipd, monkeypatch, sysm, opts)
    assert xm and p2 and kernel_name(hf)[0] == COMPOSED, (hf.level_sizes(), xm, p2, kernel_name(hf))
    hg, xm, p2 = hierarchy(ipd, monkeypatch, sysm, opts, env=NO_FULL)
    assert xm and p2 and kernel_name(hg)[0] == COMPOSED
    for K in (1, 2):
        a = run_cycles(hf, f, guess, K)
        assert variant(hf) == (1, 0)
        b = run_cycles(hg, f, guess, K)
        assert variant(hg) == (0, 0)
        assert np.all(np.isfinite(a)) and not np.array_equal(a, guess)
        assert np.array_equal(a, b), (K, np.max(np.abs(a - b)))
    hf.close()
    hg.close()


OUTSIDE = {
    "1024x1000": dict(m=1024, n=1000),
    "1000x1024": dict(m=1000, n=1024),
    "1023x1024": dict(m=1023, n=1024),
    "isnsp0": dict(m=1024, n=1024, isnsp=0),
    "G256": dict(m=1024, n=1024, env=(("IPD_RESIDENT_G", "256"),)),
}


@pytest.mark.parametrize("case", sorted(OUTSIDE))
def test_shapes_outside_the_predicate_keep_the_general_form(ipd, monkeypatch, case):
    """A row count off the full shape, isnsp = 0 and 256 workgroups: the general production form (full = 0,
    diag = 0), bit-equal on a rerun."""
    c = OUTSIDE[case]
    m, n = c["m"], c["n"]
    sysm = dense_system(ipd, m, n)
    f, guess = sysm[1], sysm[2]
    h, xm, p2 = hierarchy(ipd, monkeypatch, sysm, options(n, isnsp=c.get("isnsp", 1)), env=c.get("env", ()))
    assert kernel_name(h)[0].startswith("k_resident<16,16,0"), (h.level_sizes(), kernel_name(h))
    for K in (1, 2):
        a = run_cycles(h, f, guess, K)
        assert variant(h) == (0, 0), (case, variant(h))
        assert np.all(np.isfinite(a)) and not np.array_equal(a, guess)
        assert np.array_equal(a, run_cycles(h, f, guess, K)), (case, K)
    h.close()


def test_diagnostic_launch_takes_the_diagnostic_full_form(ipd, monkeypatch):
    """ipd_amg_bench_resident_classes on the metric system: the form with the stamps (full = 1, diag = 1), 24
    hand-offs per cycle, and the production launch's iterate."""
    m = n = 1024
    sysm = dense_system(ipd, m, n)
    f, guess = sysm[1], sysm[2]
    h, xm, p2 = hierarchy(ipd, monkeypatch, sysm, options(n))
    assert xm and p2 and kernel_name(h)[0] == COMPOSED
    K = 2
    a = run_cycles(h, f, guess, K)
    assert variant(h) == (1, 0)
    total_prod = kernel_name(h)[1]
    x, st = run_cycles_stamped(h, f, guess, K)
    assert variant(h) == (1, 1)
    name, total, cycles = kernel_name(h)
    counts = st[24:32]
    print("hand-offs %d (production launch %d), per class %s" % (total, total_prod, counts))
    assert name == COMPOSED and cycles == K
    assert total == total_prod == st[2] == sum(counts) == 24 * K + 1      # (+ 1: the residual norm after the last cycle)
    assert np.array_equal(x, a)
    assert np.array_equal(run_cycles(h, f, guess, K), a) and variant(h) == (1, 0)   # ... and back
    h.close()
