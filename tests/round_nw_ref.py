"""The north-west-corner correction of the primal certificate (include/ipd_amg.h steps N1-N7)
re-stated in numpy, operation by operation, with the header's scan shape; the textbook sequential north-west-corner
loop it is compared with; and the rebuild of X^ from the factors and the list.  No GPU here:
tests/test_round_nw_ref.py runs it on the CPU, tests/test_gpu_round_nw.py compares the device's list with it bit for
bit."""
import numpy as np

from tests import round_ref as R

CHUNK = 64
LD = np.longdouble


def prefixes(a):
    """step N3: [0, the inclusive prefixes of a] -- local prefixes per chunk of 64 entries (cumsum along the chunk),
    the chunk offsets a cumsum of the chunks' last local prefixes, a prefix their sum"""
    a = np.asarray(a, dtype=np.float64)
    k = len(a)
    nch = -(-k // CHUNK)
    pad = np.zeros(nch * CHUNK)
    pad[:k] = a
    loc = np.cumsum(pad.reshape(nch, CHUNK), axis=1)
    off = np.concatenate([[0.0], np.cumsum(loc[:, -1])[:-1]])   # (the padding adds 0.0: the chunk's last prefix)
    out = off[:, None] + loc
    return np.concatenate([[0.0], out.reshape(-1)[:k]])


def masses(p, q, e, f, se, sf, sigma=None, tau=None):
    """step N2 along the orders of step N1 (None: identity)"""
    sigma = np.arange(len(p)) if sigma is None else np.asarray(sigma)
    tau = np.arange(len(q)) if tau is None else np.asarray(tau)
    return (p[sigma] * e[sigma]) * sf, (q[tau] * f[tau]) * se, sigma, tau


def entries_of_prefixes(Rp, Cp):
    """step N4 on the prefixes [R_0..R_m], [C_0..C_n]: (k, s, w), 1-based, ascending.  Stated as the device finds
    them -- an entry ends at the row breakpoint k when R_k <= C_s, at the column breakpoint s otherwise -- which for
    non-decreasing prefixes is the set of all (k, s) with min(R_k, C_s) - max(R_k-1, C_s-1) > 0."""
    m, n = len(Rp) - 1, len(Cp) - 1
    out = []
    with np.errstate(invalid="ignore"):
        # row breakpoints: the first s with C_s >= R_k
        k = np.arange(1, m + 1)
        s = np.searchsorted(Cp[1:], Rp[1:], side="left") + 1
        ok = (Rp[1:] > Rp[:-1]) & (s <= n)
        sc = np.minimum(s, n)
        w = Rp[1:] - np.maximum(Rp[:-1], Cp[sc - 1])
        ok &= w > 0
        out += [(int(a), int(b), float(c)) for a, b, c in zip(k[ok], sc[ok], w[ok])]
        # column breakpoints: the first k with R_k > C_s
        s = np.arange(1, n + 1)
        k = np.searchsorted(Rp[1:], Cp[1:], side="right") + 1
        ok = (Cp[1:] > Cp[:-1]) & (k <= m)
        kc = np.minimum(k, m)
        w = Cp[1:] - np.maximum(Rp[kc - 1], Cp[:-1])
        ok &= w > 0
        out += [(int(a), int(b), float(c)) for a, b, c in zip(kc[ok], s[ok], w[ok])]
    out.sort(key=lambda t: (t[0], t[1]))
    return out


def correction(p, q, e, f, se, sf, sigma=None, tau=None):
    """steps N1-N4: the list (i, j, g) as int32, int32, float64 arrays, with the prefixes it came from"""
    alpha, beta, sigma, tau = masses(p, q, e, f, se, sf, sigma, tau)
    Rp, Cp = prefixes(alpha), prefixes(beta)
    ks = entries_of_prefixes(Rp, Cp)
    i = np.array([sigma[k - 1] for k, _, _ in ks], dtype=np.int32)
    j = np.array([tau[s - 1] for _, s, _ in ks], dtype=np.int32)
    w = np.array([w for _, _, w in ks], dtype=np.float64)
    g = w / (p[i] * q[j]) if len(ks) else w
    return dict(i=i, j=j, g=g, w=w, R=Rp, C=Cp, ks=ks)


def textbook(alpha, beta):
    """the sequential north-west-corner loop on masses with equal totals: (k, s, w), 1-based, the positive entries"""
    alpha, beta = [float(a) for a in alpha], [float(b) for b in beta]
    out = []
    k = s = 0
    a = alpha[0] if alpha else 0.0
    b = beta[0] if beta else 0.0
    while k < len(alpha) and s < len(beta):
        w = min(a, b)
        if w > 0:
            out.append((k + 1, s + 1, w))
        a, b = a - w, b - w
        if a == 0:
            k += 1
            a = alpha[k] if k < len(alpha) else 0.0
        if b == 0:
            s += 1
            b = beta[s] if s < len(beta) else 0.0
    return out


def rebuild(x, m, n, tol, res, i, j, g):
    """X^ (m, n) in longdouble: theta*X2 from the injected x and the factors a call returned, plus t*g at the list"""
    Xp = R.clamp(np.asarray(x, dtype=np.float64)[:m * n].reshape((m, n), order="F"), tol)[0].astype(LD)
    rho, kappa = res["rho"].astype(LD), res["kappa"].astype(LD)
    Xh = LD(res["theta"]) * ((rho[:, None] * Xp) * kappa[None, :])
    np.add.at(Xh, (np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)), LD(res["t"]) * g.astype(LD))
    return Xh


def dense(m, n, i, j, g):
    G = np.zeros((m, n))
    G[i, j] = g
    return G
