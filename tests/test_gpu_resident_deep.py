"""Mask-form level-resident kernel, DEEP mode (csrc/ipd_resident_big.h, round 4): REALISTIC hierarchies whose
level 1 exceeds k_resident's 2048 rows -- the Newton systems of the m = n = 2048 Class 1 driver run (levels
about 4096 / 2048 / 640 / 190 / 55 / 15).  Level 1 and the level 1 <-> 2 transfers from the active-set bit
mask, level 2 as register slices, level 3 in polynomial form, the remote tail workgroup rooted at level 4.

Reference behaviour: AMG/Class_AMG.m:86-109, AMG/MG_Wcycle.m:13-46, AMG/MG_Vcycle.m:12-45, Hybrid_AMG.m:40-41.
Checked against the ORACLE directly (hierarchy sizes, cycle counts, residual histories to max(1e-10, 2 x the
oracle's own one-ulp sensitivity) capped at 1e-9, A(x - x_oracle) <= 1e-9 |f|) and against the multi-launch
path (IPD_NO_RESIDENT_DEEP=1)."""
from ctypes import byref, c_int32

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ipd_oracle as O
from tests.newton_capture import capture
from tests.test_gpu_bench_workload import (bench_cycles, env, options, resident_kernel_name, same_history,
                                            solve_mode)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ipd():
    import codes_of_ipd_ssn_amg_method_amd as m
    return m


@pytest.fixture(scope="module", params=[12, 24], ids=["k13", "k25"])
def newton2048(ipd, request):
    """(n, Ae, f, tk): the captured system, or -- when it has several components -- its largest component as
    Hybrid_AMG.m:55-70 takes it (Ae(pk, pk) with pk ascending, so the F side comes first and n = sum(pk <= N)),
    the system ipd_hybrid's gathered mask form serves."""
    N = 2048
    Ae, f, tk = capture(ipd, N, request.param)
    ncomp, lab = sp.csgraph.connected_components(Ae)
    if ncomp > 1:
        pk = np.flatnonzero(lab == np.argmax(np.bincount(lab)))
        return int((pk < N).sum()), sp.csr_matrix(Ae[pk, :][:, pk]), f[pk], tk
    return N, Ae, f, tk


def _deep_hierarchy(ipd, Ae, n, tk, cycle):
    """The hierarchy with the mask form attached for the gathered p (C rows) and q (F rows): all ones in these
    captures (Hybrid_AMG.m:17-24 with p = q = 1)."""
    h = ipd.AMGHierarchy(Ae, options(cycle, n), ipd.MatlabRand(5489))
    h.attach_mask_operator(np.ones(Ae.shape[0] - n), np.ones(n), tk)
    return h


@pytest.mark.parametrize("cycle", ["w", "v"])
def test_deep_mode_against_the_oracle_and_the_launches(ipd, newton2048, cycle):
    N, Ae, f, tk = newton2048
    M = Ae.shape[0]
    # Hybrid_AMG.m:40 starts from bk1 * tk * rand(M, 1): a non-zero guess for the W case, zeros for the V case
    x0 = 1e-4 * np.random.RandomState(4).random_sample(M) if cycle == "w" else np.zeros(M)
    h = _deep_hierarchy(ipd, Ae, N, tk, cycle)
    mode, grid, _ = solve_mode(h)
    assert mode == 2, (h.level_sizes(), [h.level_dims(k)[1] for k in range(1, h.J + 1)])
    # both captures: level-2 rows of at most 16 entries (KE2 = 4), six levels, level 4 resident as well
    # (tests/test_gpu_resident_instantiations.py reaches <8,2,true> and the tail rooted at 4)
    assert resident_kernel_name(h) == "k_resident_big<4,2,true>"
    assert h.J >= 6 and 129 <= grid <= 256
    from codes_of_ipd_ssn_amg_method_amd import _lib
    lev, root = c_int32(), c_int32()
    _lib.check(_lib.lib.ipd_amg_resident_levels(h.handle, byref(lev), byref(root)))
    assert (lev.value, root.value) == (4, 5)
    with env(IPD_NO_RESIDENT_DEEP=1):
        hc = _deep_hierarchy(ipd, Ae, N, tk, cycle)
    assert solve_mode(hc)[0] == 0 and hc.level_sizes() == h.level_sizes()
    x, it, rr, relk, rhok = h.solve(f, x0)
    assert solve_mode(h)[2] == 0, "no hand-off timed out"
    xc, itc, rrc, relkc, rhokc = hc.solve(f, x0)
    nf_ = np.linalg.norm(f)
    same_history(it, np.asarray(relk), itc, np.asarray(relkc), tol=2e-10)
    assert np.linalg.norm(Ae @ (x - xc)) <= 1e-9 * nf_
    # the kernel's own norm (|x| ~ 50, |Ae| ~ 1e3: A*x carries ~1e-11 |f| of rounding at this size)
    assert np.linalg.norm(Ae @ x - f) <= (1.05 * rr + 1e-11) * nf_
    # ... against the oracle directly
    o = dict(options(cycle, N))
    o.update(guess=x0)
    xo, ito, rro, relko, rhoko, ho = O.Class_AMG(Ae, f, o, O.matlab_rng(5489), return_hierarchy=True)
    assert h.level_sizes() == ho.level_sizes()
    assert [h.level_dims(k)[1] for k in range(1, h.J + 1)] == ho.level_nnz()
    sgn = np.where(np.random.RandomState(11).random_sample(f.size) < 0.5, -1.0, 1.0)
    _, itp, _, relkp, _ = O.Class_AMG(Ae, f * (1.0 + 2.2e-16 * sgn), o, O.matlab_rng(5489))
    kk = min(ito, itp) + 1
    sens = float(np.max(np.abs(np.asarray(relko[:kk]) - np.asarray(relkp[:kk]))))
    same_history(it, np.asarray(relk), ito, np.asarray(relko), tol=min(max(1e-10, 2.0 * sens), 1e-9))
    assert np.linalg.norm(Ae @ (x - xo)) <= 1e-9 * nf_
    assert it >= 3, relk
    # K loop bodies (what bench.py times): against the launches, and run-to-run identical bits
    a = bench_cycles(h, f, x0, 3)[0]
    b = bench_cycles(hc, f, x0, 3)[0]
    assert np.linalg.norm(Ae @ (a - b)) <= 5e-9 * nf_
    assert np.array_equal(a, bench_cycles(h, f, x0, 3)[0])
    # zero right-hand side (Class_AMG.m:91-92)
    xz, itz, relz, relkz, rhokz = h.solve(np.zeros(M), None)
    assert itz == 0 and relkz[0] == 0.0 and not xz.any()
    h.close()
    hc.close()


def test_deep_mode_polynomial_operators_against_numpy(ipd, newton2048):
    """Levels 3 and 4 of the deep mode in polynomial form (ResBigDesc::p3rows / p4rows in the RB_P3_SEG /
    RB_P4_SEG row layouts, forms bit 64) as packed, against the numpy restatement of the algebra
    (tests/test_gpu_poly_operators.py: bars, padding -- the deep passes read whole segments -- and the power
    of the check against nu -+ 1, isnsp flipped and D^-1 scaled by 1 + 1e-6)."""
    from tests.test_gpu_poly_operators import check_rows_operator
    N, Ae, f, tk = newton2048
    h = _deep_hierarchy(ipd, Ae, N, tk, "w")
    assert solve_mode(h)[0] == 2, h.level_sizes()
    assert resident_kernel_name(h) == "k_resident_big<4,2,true>"
    forms = h.level_forms()
    assert forms[2] & 64, forms
    levels = [k for k in (3, 4) if k < h.J and forms[k - 1] & 64]
    from codes_of_ipd_ssn_amg_method_amd import _lib
    lev, root = c_int32(), c_int32()
    _lib.check(_lib.lib.ipd_amg_resident_levels(h.handle, byref(lev), byref(root)))
    assert levels == ([3, 4] if (lev.value, root.value) == (4, 5) else [3]), (levels, lev.value, root.value)
    for k in levels:
        check_rows_operator(h, k, 1, 5)
    h.close()
