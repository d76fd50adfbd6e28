"""The numpy restatement of the north-west-corner correction (tests/round_nw_ref.py; include/ipd_amg.h steps N1-N7,
DESIGN.md section 4n) on the CPU: on dyadic deficits, where every sum is exact, it is the textbook sequential
north-west-corner loop bit for bit, its coupling has exactly the rank-one term's marginals, its list has at most
m + n - 1 entries, and its prefixes do not decrease across chunk edges on any non-negative input.  CPU only."""
import numpy as np
import pytest

from tests import round_nw_ref as NW

SHAPES = [(1, 1), (3, 70), (65, 64), (257, 129)]


def dyadic_deficits(m, n, seed, order=False):
    """e, f multiples of 2^-3 with runs of zeros and equal totals <p,e> = <q,f>, p = q = 1; Se = Sf a power of two
    times an integer, so every mass (p*e)*Sf and every prefix is exact"""
    rs = np.random.RandomState(seed)
    e = rs.randint(0, 9, m) / 8.0
    f = rs.randint(0, 9, n) / 8.0
    e[rs.random_sample(m) < 0.3] = 0.0
    f[rs.random_sample(n) < 0.3] = 0.0
    if m > 8:
        e[3:8] = 0.0          # a run of zeros
    d = e.sum() - f.sum()      # exact
    if d > 0:
        f[-1] += d
    else:
        e[-1] -= d
    assert e.sum() == f.sum()
    p, q = np.ones(m), np.ones(n)
    sigma = rs.permutation(m) if order else None
    tau = rs.permutation(n) if order else None
    return p, q, e, f, float(e.sum()), float(f.sum()), sigma, tau


@pytest.mark.parametrize("order", [False, True])
@pytest.mark.parametrize("m,n", SHAPES)
def test_restatement_is_the_textbook_loop_on_dyadic_deficits(m, n, order):
    p, q, e, f, se, sf, sigma, tau = dyadic_deficits(m, n, 7 * m + n, order)
    got = NW.correction(p, q, e, f, se, sf, sigma, tau)
    alpha, beta, sg, ta = NW.masses(p, q, e, f, se, sf, sigma, tau)
    want = NW.textbook(alpha, beta)
    assert [(k, s) for k, s, _ in got["ks"]] == [(k, s) for k, s, _ in want]
    assert np.array_equal(got["w"].view(np.int64), np.array([w for _, _, w in want]).view(np.int64))
    assert np.array_equal(got["i"], [sg[k - 1] for k, _, _ in want])
    assert np.array_equal(got["j"], [ta[s - 1] for _, s, _ in want])
    assert se == 0 or len(want) > 0


@pytest.mark.parametrize("order", [False, True])
@pytest.mark.parametrize("m,n", SHAPES)
def test_marginals_are_the_rank_one_terms(m, n, order):
    """sum_j q_j*G_ij = e_i*Sf and sum_i p_i*G_ij = f_j*Se, exactly"""
    p, q, e, f, se, sf, sigma, tau = dyadic_deficits(m, n, 11 * m + n, order)
    got = NW.correction(p, q, e, f, se, sf, sigma, tau)
    G = NW.dense(m, n, got["i"], got["j"], got["g"])
    assert len(set(zip(got["i"].tolist(), got["j"].tolist()))) == len(got["i"])      # each (i, j) once
    assert np.array_equal((q[None, :] * G).sum(axis=1), e * sf)
    assert np.array_equal((p[:, None] * G).sum(axis=0), f * se)


@pytest.mark.parametrize("m,n", SHAPES + [(1000, 90), (64, 64), (128, 1)])
def test_count_is_at_most_m_plus_n_minus_1(m, n):
    for seed in range(3):
        p, q, e, f, se, sf, sigma, tau = dyadic_deficits(m, n, 13 * m + n + seed, seed % 2 == 1)
        got = NW.correction(p, q, e, f, se, sf, sigma, tau)
        assert len(got["i"]) <= m + n - 1
        ks = got["ks"]
        assert all(a[0] <= b[0] and a[1] <= b[1] and a[:2] != b[:2] for a, b in zip(ks, ks[1:]))   # a staircase
    # general (non-dyadic) deficits: the bound and the staircase hold as well
    rs = np.random.RandomState(m + n)
    p, q = 0.5 + rs.random_sample(m), 0.5 + rs.random_sample(n)
    e, f = rs.random_sample(m) * (rs.random_sample(m) < 0.7), rs.random_sample(n) * (rs.random_sample(n) < 0.7)
    got = NW.correction(p, q, e, f, float(p @ e), float(q @ f), rs.permutation(m), rs.permutation(n))
    ks = got["ks"]
    assert len(ks) <= m + n - 1
    assert all(a[0] <= b[0] and a[1] <= b[1] and a[:2] != b[:2] for a, b in zip(ks, ks[1:]))
    assert (got["g"] > 0).all()


@pytest.mark.parametrize("k", [1, 63, 64, 65, 128, 129, 1000, 16384])
def test_prefixes_do_not_decrease_across_chunk_edges(k):
    rs = np.random.RandomState(k)
    for scale in (1.0, 1e-17, 1e17):
        a = rs.random_sample(k) * scale
        a[rs.random_sample(k) < 0.3] = 0.0
        a[::7] *= 1e-9
        P = NW.prefixes(a)
        assert len(P) == k + 1 and P[0] == 0.0
        assert (np.diff(P) >= 0).all()
        for edge in range(64, k, 64):      # P[edge] is the last prefix of a chunk, P[edge + 1] the next chunk's first
            assert P[edge + 1] >= P[edge]
        # the stated shape: within a chunk a sequential sum from the chunk's first entry, plus the chunk's offset
        c = min(k - 1, 70) // 64
        lo = 64 * c
        acc = 0.0
        for t in range(lo, min(k, lo + 64)):
            acc = acc + a[t]
            off = P[lo] if c else 0.0
            assert P[t + 1] == off + acc
