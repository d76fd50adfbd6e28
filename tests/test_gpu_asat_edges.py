"""ASAt at the edges of its route rules (csrc/ipd_kkt_plan.h), bit-exact against the oracle: sequences of calls on one
context whose entry counts land exactly on, and just above, the capacity the previous call's count gives; shapes on
both sides of the one-launch route's 16 mask words per row; counts on both sides of its hint bound; and explicit
zeros at the capacity edge.  The route taken cannot be seen in the result -- tests/test_kkt_plan.py pins the
decisions, this file pins the results on both sides of each decision."""
import numpy as np
import pytest

from oracle import ipd_oracle as O
from tests import problems as PR
from tests.test_gpu_kkt import _csc_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ipd():
    import codes_of_ipd_ssn_amg_method_amd as m
    return m


def cap_after(nnz, m, n):
    """entries the call after one with nnz entries has room for (the rule restated)"""
    return min(2 * m * n + m + n, nnz + nnz // 4 + 64)


def pq(m, n, seed=11):
    rs = np.random.RandomState(seed)
    return 0.5 + rs.random_sample(m), 0.5 + rs.random_sample(n)


def flat(Y):
    return np.ascontiguousarray(Y.reshape(-1, order="F"))


def wrapped_diagonal(m, n, extra):
    """Y[i, i % n] = 1 for every i, and Y[i, (i + 1) % n] = 1 for i < extra: every row and column is touched by the
    first part, so the second adds two entries of H each"""
    Y = np.zeros((m, n), np.uint8)
    Y[np.arange(m), np.arange(m) % n] = 1
    Y[np.arange(extra), (np.arange(extra) + 1) % n] = 1
    return flat(Y)


def stored_before_drop(s, m, n):
    """entries of H the kernels count: 2 E + touched rows and columns, explicit zeros included"""
    Y = s.reshape((m, n), order="F") != 0
    return 2 * int(Y.sum()) + int(Y.any(axis=1).sum()) + int(Y.any(axis=0).sum())


def check(ipd, s, p, q, note):
    Ho = O.ASAt(s, p, q)
    assert _csc_equal(ipd.ASAt(s, p, q), Ho), note
    return Ho.nnz


@pytest.mark.parametrize("m,n,first,room", [(256, 256, 1024, 160), (1088, 64, 3328, 448)])
def test_capacity_edge(ipd, m, n, first, room):
    """(256, 256): the one-launch route is open (nib = njb = 4); (1088, 64): nib = 17 shuts it, the general route's
    guess meets the same edge.  At the cap the first fill stands, two entries above it the assembly is redone."""
    p, q = pq(m, n)
    cap = cap_after(first, m, n)
    assert cap == first + first // 4 + 64 == first + 2 * room
    for extra, want in [(room, cap), (room + 1, cap + 2)]:
        assert check(ipd, wrapped_diagonal(m, n, 0), p, q, (m, n, "first")) == first
        assert check(ipd, wrapped_diagonal(m, n, extra), p, q, (m, n, extra)) == want


@pytest.mark.parametrize("m,n", [(1024, 1024), (1025, 1000), (1000, 1025)])
def test_shape_edge_of_the_small_route(ipd, m, n):
    """16 mask words per row on both sides, 17 on the column side, 17 on the row side: the second and fourth calls
    come with a small count from the call before"""
    p, q = pq(m, n, seed=m + n)
    masks = [PR.mask_tree(m, n, seed=21), PR.mask_tree(m, n, seed=22), np.zeros(m * n, np.uint8),
             PR.mask_tree(m, n, seed=23)]
    for k, s in enumerate(masks):
        check(ipd, s, p, q, (m, n, k))


@pytest.mark.parametrize("one_more", [0, 1])
def test_hint_edge(ipd, one_more):
    """a band of 31 per column: 65536 entries, the largest count that still opens the one-launch route for the next
    call; one more entry of the mask gives 65538"""
    m = n = 1024
    p, q = pq(m, n, seed=5)
    i, j = np.meshgrid(np.arange(m), np.arange(n), indexing="ij")
    Y = ((i - j) % 1024 < 31).astype(np.uint8)
    assert Y.sum() == 31744 and not Y[0, 31]
    Y[0, 31] = one_more
    assert check(ipd, flat(Y), p, q, ("band", one_more)) == 65536 + 2 * one_more
    check(ipd, PR.mask_tree(m, n, seed=24), p, q, ("tree after band", one_more))


def test_zero_squares_at_the_capacity_edge(ipd):
    """p[::7] = 0: the capacity test sees the explicit zeros (1344 and 1346 stored entries), the result has none"""
    m = n = 256
    p, q = pq(m, n)
    pz = p.copy()
    pz[::7] = 0.0
    cap = cap_after(1024, m, n)
    for extra, want in [(160, cap), (161, cap + 2)]:
        s0, s1 = wrapped_diagonal(m, n, 0), wrapped_diagonal(m, n, extra)
        assert stored_before_drop(s0, m, n) == 1024 and stored_before_drop(s1, m, n) == want
        assert check(ipd, s0, pz, q, "first") < 1024
        assert check(ipd, s1, pz, q, extra) < want
