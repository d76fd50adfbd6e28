"""The references and inputs of tests/test_gpu_dev_abi.py, checked without a GPU: the longdouble references
against exact rational arithmetic, the mask cases against the tile geometry they claim, the SpMV matrices
against the branch and grid-cap rules read from ipd_sparse.hip."""
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import dev_abi as D


def test_longdouble_keeps_more_than_float64():
    # the 2 gamma tolerances stay valid against a float64 reference; with extended precision the reference's
    # own rounding is negligible, which is what this machine has
    assert np.finfo(np.longdouble).nmant >= 52


def dyadic(rs, count):
    """Values k / 64, |k| < 2^10: products and sums of a 6 x 5 case are exact in float64 and longdouble alike."""
    return rs.randint(-1023, 1024, count) / 64.0


def test_ax_reference_is_exact_on_a_6_by_5_case():
    m, n = 6, 5
    rs = np.random.RandomState(1)
    x, p, q = dyadic(rs, m * n), dyadic(rs, m), dyadic(rs, n)
    ref, bound = D.ax_ref(x, p, q)
    F = Fraction
    exact = [sum(F(x[i + j * m]) * F(p[i]) for i in range(m)) for j in range(n)] + \
            [sum(F(x[i + j * m]) * F(q[j]) for j in range(n)) for i in range(m)]
    assert [F(float(v)) for v in ref] == exact and all(float(v) == v for v in ref)
    mags = [sum(abs(F(x[i + j * m]) * F(p[i])) for i in range(m)) for j in range(n)] + \
           [sum(abs(F(x[i + j * m]) * F(q[j])) for j in range(n)) for i in range(m)]
    want = [2 * (m + 1) * F(D.U) * v for v in mags[:n]] + [2 * (n + 1) * F(D.U) * v for v in mags[n:]]
    assert [F(float(b)) for b in bound] == want


def test_spmv_reference_is_exact_on_a_6_by_5_case():
    rs = np.random.RandomState(2)
    A = D.csr_from_lengths([0, 5, 1, 3, 0, 2], 5, seed=4)
    A.data[:] = dyadic(rs, A.nnz)
    x = dyadic(rs, 5)
    ref, bound = D.spmv_ref(A, x)
    F = Fraction
    for r in range(6):
        cols = A.indices[A.indptr[r]:A.indptr[r + 1]]
        vals = A.data[A.indptr[r]:A.indptr[r + 1]]
        assert F(float(ref[r])) == sum(F(a) * F(x[c]) for a, c in zip(vals, cols)), r
        assert F(float(bound[r])) == 2 * (len(cols) + 1) * F(D.U) * sum(abs(F(a) * F(x[c])) for a, c in zip(vals, cols))
    assert ref[0] == 0 and ref[4] == 0 and bound[0] == 0


def test_within_reports_a_miss():
    ref, bound = np.array([1.0], D.LD), np.array([1e-15], D.LD)
    assert D.within(np.array([1.0 + 4e-16]), ref, bound)[0]
    assert not D.within(np.array([1.0 + 4e-15]), ref, bound)[0]
    assert not D.within(np.array([1e-300]), np.zeros(1, D.LD), np.zeros(1, D.LD))[0]


def test_mask_shapes_have_the_tiles_they_claim():
    for (m, n), (full, partial, mult8) in D.ASAT_SHAPES.items():
        assert m // 64 == full and (m % 64 != 0) == partial and (m % 8 == 0) == mult8, (m, n)
    shapes = D.ASAT_SHAPES
    assert any(f >= 1 and not p and w for f, p, w in shapes.values())      # wide loads, full tiles only
    assert any(f >= 1 and p and w for f, p, w in shapes.values())          # tile 0 wide, tile 1 by bytes (m = 72)
    assert any(f == 0 and p and w for f, p, w in shapes.values())          # m % 8 == 0 without a full tile
    assert any(f >= 1 and not w for f, p, w in shapes.values())            # a full tile that can only go by bytes
    assert [o % 8 == 0 for o in D.ASAT_OFFSETS] == [True, True, False, False]


@pytest.mark.parametrize("flavour", sorted(D.MASK_FLAVOURS))
def test_mask_flavours(flavour):
    for (m, n) in D.ASAT_SHAPES:
        for rho in D.ASAT_DENSITIES:
            s = D.mask_bytes(m, n, rho, flavour)
            assert s.dtype == np.uint8 and s.size == m * n
            assert set(np.unique(s)) <= set(D.MASK_FLAVOURS[flavour]) | {0}
            if rho == 0.0:
                assert not s.any()
            if rho == 1.0:
                assert s.all()
            if flavour == "bit0clear":
                assert not (s & 1).any()                                   # no odd byte: bit 0 is never set
    if flavour != "01":
        s = D.mask_bytes(128, 130, 0.5, flavour)
        assert set(np.unique(s)) == set(D.MASK_FLAVOURS[flavour]) | {0}    # every byte value occurs


def test_bytes_to_bits_maps_every_nonzero_byte_to_one():
    for b in range(256):
        for lane in range(8):
            assert D.bytes_to_bits_model(b << (8 * lane)) == ((1 << lane) if b else 0), (b, lane)
    assert D.bytes_to_bits_model(0x80FF021001000200) == 0b11111010
    with open(os.path.join(D.CSRC, "ipd_asat.hip")) as fh:
        src = fh.read()
    assert "x &= 0x0101010101010101ull;" in src and "(x * 0x0102040810204080ull) >> 56" in src


def test_spmv_matrices_take_the_intended_branch_and_exceed_the_cap():
    rules = D.spmv_rules()
    cap, cuts = rules
    assert cap == 8192 and cuts == [(6.0, 4), (24.0, 16), (float("inf"), 64)]
    for name, (make, L) in D.SPMV_MATRICES.items():
        A = make()
        assert D.spmv_branch(A, rules) == L, (name, A.nnz / A.shape[0])
        A.sort_indices()
        assert A.has_canonical_format and not (A.data == 0).any(), name
        lens = np.diff(A.indptr)
        if name in ("L4", "L16", "L64"):
            assert {0, 1, L - 1, L, L + 1, 3 * L + 5} <= set(lens.tolist()), name
            assert A.shape[0] != A.shape[1]
        if name.startswith("cap_"):
            groups = cap * 256 // L                                         # row groups of a capped grid
            assert A.shape[0] == groups + 1, (name, A.shape, groups)       # one row for the grid-stride loop
            assert A.nnz * 12 + 4 * A.shape[0] < 16 << 20, name            # a few MB
    assert D.SPMV_MATRICES["one_row"][0]().shape[0] == 1 and D.SPMV_MATRICES["one_column"][0]().shape[1] == 1
    assert [D.SPMV_MATRICES["cap_" + k][0]().shape[0] for k in ("L4", "L16", "L64")] == [524289, 131073, 32769]


def test_ax_shapes_straddle_the_tile_edges():
    with open(os.path.join(D.CSRC, "ipd_limits.h")) as fh:
        src = fh.read()
    assert "AX_TR = 256;" in src and "AX_TC = 16;" in src and "ATY_TC = 16;" in src
    ms, ns = {m for m, n in D.AX_SHAPES}, {n for m, n in D.AX_SHAPES}
    assert {255, 256, 257} <= ms and {15, 16, 17} <= ns and {1} <= ms & ns
    assert any(m % 2 == 0 for m in ms) and any(m % 2 for m in ms)          # k_aty_v2 needs an even m
