"""The fed seams of the full-shape form of k_resident's composed instantiation (csrc/ipd_resident.h, FULL): the
prolongation without its C block and with beta .* e_2 formed at e_2's receipt, rr = r - A e riding the pre run's last
half sweep, top's r = b - A x (with x += e) riding the post run's last half sweep, and the pre run's start fed from
top's local first half.  None of them changes a floating-point operation or the order of a sum, so every check is
bit-equality: against the general form (IPD_RES_NO_FULL=1), which has none of these seams, against one launch of as
many cycles, and -- the form with the stamps -- against the production launch.  The full shape is M = 2048 by
definition, so the tests use the workload's size with one to three cycles.  Every test asks the library which
variant its last launch took and that no hand-off timed out."""
from ctypes import byref, c_int32

import numpy as np
import pytest

from tests.test_gpu_resident_full import (COMPOSED, HOLES_RHO, NO_FULL, dense_system, hierarchy, holes_system,
                                          kernel_name, options, run_cycles, run_cycles_stamped, variant)

pytestmark = pytest.mark.gpu

M = N = 1024


@pytest.fixture(scope="module")
def ipd():
    import codes_of_ipd_ssn_amg_method_amd as m
    return m


def timeouts(h):
    """resident launches of the hierarchy that gave up (bench.py's resident_kernel_timeouts)"""
    from codes_of_ipd_ssn_amg_method_amd import _lib
    mode, grid, tmo = c_int32(), c_int32(), c_int32()
    _lib.check(_lib.lib.ipd_amg_solve_mode(h.handle, byref(mode), byref(grid), byref(tmo)))
    return tmo.value


def system(ipd, which):
    return dense_system(ipd, M, N) if which == "dense" else holes_system(M, N, HOLES_RHO)


def pair(ipd, monkeypatch, sysm, opts):
    """(full-form hierarchy, general-form hierarchy) of one system and one set of options"""
    hf, xm, p2 = hierarchy(ipd, monkeypatch, sysm, opts)
    assert xm and p2 and kernel_name(hf)[0] == COMPOSED, (hf.level_sizes(), xm, p2, kernel_name(hf))
    hg, xm, p2 = hierarchy(ipd, monkeypatch, sysm, opts, env=NO_FULL)
    assert xm and p2 and kernel_name(hg)[0] == COMPOSED
    return hf, hg


# smoth 2: the first and the last sweep of a run are distinct and adjacent; smoth 3: one sweep between them; smoth 1
# with three cycles: the pre run's only half sweep is at once the one top feeds and the one rr rides, and the post
# run's last half sweep is the second it has.  (smoth 5, and smoth 1 at one and two cycles: test_gpu_resident_full.py)
CASES = [("dense", 2, (1, 2, 3)), ("dense", 3, (1, 2, 3)), ("dense", 1, (3,)),
         ("holes", 2, (1, 2, 3)), ("holes", 3, (1, 2, 3)), ("holes", 1, (3,))]


@pytest.mark.parametrize("which,smoth,Ks", CASES, ids=["%s-smoth%d" % (c[0], c[1]) for c in CASES])
def test_full_form_with_fed_seams_is_the_general_form_bit_for_bit(ipd, monkeypatch, which, smoth, Ks):
    """Iterates after K cycles on bench's dense system and on the mask with holes: full form == general form."""
    sysm = system(ipd, which)
    f, guess = sysm[1], sysm[2]
    hf, hg = pair(ipd, monkeypatch, sysm, options(N, smoth=smoth))
    for K in Ks:
        a = run_cycles(hf, f, guess, K)
        assert variant(hf) == (1, 0)
        assert kernel_name(hf)[1] == (4 * smoth + 4) * K + 1   # (24 hand-offs per cycle at smoth 5)
        b = run_cycles(hg, f, guess, K)
        assert variant(hg) == (0, 0)
        assert np.all(np.isfinite(a)) and not np.array_equal(a, guess)
        print("%s smoth %d K %d: max |full - general| = %.3e" % (which, smoth, K, np.max(np.abs(a - b))))
        assert np.array_equal(a, b), (which, smoth, K, np.max(np.abs(a - b)))
    assert timeouts(hf) == 0 and timeouts(hg) == 0
    hf.close()
    hg.close()


@pytest.mark.parametrize("smoth", [2, 5])
def test_solve_to_tolerance_equals_the_general_form(ipd, monkeypatch, smoth):
    """A Class_AMG solve with its stopping rules (retol 1e-11, maxit 30), where the norm of a fused top decides: the
    iterate, the iteration count and the histories relk, rhok equal the general form's."""
    sysm = system(ipd, "dense")
    f, guess = sysm[1], sysm[2]
    hf, hg = pair(ipd, monkeypatch, sysm, options(N, smoth=smoth))
    xf, itf, relf, relkf, rhokf = hf.solve(f, guess)
    assert variant(hf) == (1, 0)
    xg, itg, relg, relkg, rhokg = hg.solve(f, guess)
    assert variant(hg) == (0, 0)
    print("smoth %d: it %d / %d, rel_res %.3e / %.3e" % (smoth, itf, itg, relf, relg))
    assert itf == itg and itf >= 2
    assert relf == relg
    assert np.array_equal(xf, xg)
    assert np.array_equal(np.asarray(relkf), np.asarray(relkg), equal_nan=True)
    assert np.array_equal(np.asarray(rhokf), np.asarray(rhokg), equal_nan=True)
    assert timeouts(hf) == 0 and timeouts(hg) == 0
    hf.close()
    hg.close()


@pytest.mark.parametrize("smoth", [1, 5])
def test_two_launches_equal_one(ipd, monkeypatch, smoth):
    """A K-cycle launch followed by a one-cycle launch from its iterate equals one launch of K + 1 cycles: the first
    top of a launch, which nothing feeds, forms the bits of the fused top that ended the launch before."""
    sysm = system(ipd, "dense")
    f, guess = sysm[1], sysm[2]
    h, xm, p2 = hierarchy(ipd, monkeypatch, sysm, options(N, smoth=smoth))
    assert xm and p2 and kernel_name(h)[0] == COMPOSED
    for K in (1, 2):
        a = run_cycles(h, f, guess, K)
        assert variant(h) == (1, 0)
        b = run_cycles(h, f, a, 1)
        c = run_cycles(h, f, guess, K + 1)
        assert variant(h) == (1, 0)
        assert not np.array_equal(a, b)
        assert np.array_equal(b, c), (smoth, K, np.max(np.abs(b - c)))
    assert timeouts(h) == 0
    h.close()


@pytest.mark.parametrize("smoth", [1, 2, 5])
def test_diagnostic_form_returns_the_production_bits_and_counts_every_hand_off_once(ipd, monkeypatch, smoth):
    """ipd_amg_bench_resident_classes (full = 1, diag = 1): the production launch's iterate; every hand-off is counted
    in exactly one class, 4 smoth + 4 per cycle and one more per launch; no run starts with a barrier of its own
    (class 1 is empty), rr and top are still hand-offs of their own classes."""
    sysm = system(ipd, "dense")
    f, guess = sysm[1], sysm[2]
    h, xm, p2 = hierarchy(ipd, monkeypatch, sysm, options(N, smoth=smoth))
    assert xm and p2 and kernel_name(h)[0] == COMPOSED
    for K in (1, 3):
        a = run_cycles(h, f, guess, K)
        assert variant(h) == (1, 0)
        x, st = run_cycles_stamped(h, f, guess, K)
        assert variant(h) == (1, 1)
        counts = st[24:32]
        print("smoth %d K %d: hand-offs per class %s" % (smoth, K, counts))
        assert np.array_equal(x, a)
        assert kernel_name(h)[1] == st[2] == sum(counts) == (4 * smoth + 4) * K + 1
        assert counts[:7] == [(4 * smoth - 1) * K, 0, K, K, K, K, K + 1]
    assert timeouts(h) == 0
    h.close()
