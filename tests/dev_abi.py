"""Helpers of tests/test_gpu_dev_abi.py and tests/test_dev_abi_refs.py: the inputs, the high-precision
references and their rounding bounds (no GPU needed), and device arrays placed at a byte offset inside a
guarded `_lib.DeviceBuffer` (imported lazily, so the CPU tests never load the library).

A device array lives GUARD bytes into a buffer that is prefilled with SENTINEL doubles, plus the offset under
test: the base of a buffer is 256-byte aligned, so "+8" is aligned for doubles and not for 16-byte accesses.
Whatever lies outside the array must still hold the sentinel after a call, and an input must come back bit
for bit."""
import ctypes
import os
import re

import numpy as np
import scipy.sparse as sp

SENTINEL = -7.0
GUARD = 256
U = 2.0 ** -53          # unit roundoff of float64
LD = np.longdouble

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "codes_of_ipd_ssn_amg_method_amd", "csrc")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------
# device arrays at an offset
# ---------------------------------------------------------------------------------------------------------------
class DevArray:
    """`host` (any dtype) uploaded `off` bytes past the guard of a sentinel-filled device buffer."""

    def __init__(self, host, off=0):
        from codes_of_ipd_ssn_amg_method_amd import _lib
        self._lib = _lib
        self.host = np.ascontiguousarray(host).reshape(-1).copy()
        assert off % self.host.dtype.itemsize == 0, "the offset keeps the element type's alignment"
        self.off = GUARD + int(off)
        nb = self.host.nbytes
        total = (self.off + nb + GUARD + 7) // 8 * 8
        self.image = np.full(total // 8, SENTINEL).view(np.uint8).copy()
        self.image[self.off:self.off + nb] = self.host.view(np.uint8)
        self.buf = _lib.DeviceBuffer.from_array(self.image)
        assert self.buf.ptr.value % 256 == 0
        self.ptr = ctypes.c_void_p(self.buf.ptr.value + self.off)

    @classmethod
    def empty(cls, count, dtype=np.float64, off=0):
        """An output of `count` entries: prefilled with the sentinel (for float64), guarded on both sides."""
        fill = SENTINEL if np.dtype(dtype) == np.float64 else 0
        return cls(np.full(int(count), fill, dtype=dtype), off)

    def _download(self):
        return self.buf.to_array(np.uint8, self.image.size)

    def read(self):
        """The array's current device content; asserts that nothing outside it was written."""
        now = self._download()
        lo, hi = self.off, self.off + self.host.nbytes
        assert np.array_equal(now[:lo], self.image[:lo]), "written before the array"
        assert np.array_equal(now[hi:], self.image[hi:]), "written behind the array"
        return now[lo:hi].copy().view(self.host.dtype)

    def assert_unchanged(self, what="input"):
        assert np.array_equal(self._download(), self.image), "%s changed on the device" % what

    def free(self):
        self.buf.free()


def free_all(*arrays):
    for a in arrays:
        if a is not None:
            a.free()


# ---------------------------------------------------------------------------------------------------------------
# Ax: reference and bound
# ---------------------------------------------------------------------------------------------------------------
AX_SHAPES = [(1, 1), (2, 1), (2, 17), (64, 64), (255, 15), (256, 16), (257, 17), (130, 257), (512, 33)]


def ax_ref(x, p, q):
    """[X'*p ; X*q] with products and sums in longdouble, and the bound on |y - ref| of a float64 result summed
    in ANY order: 2 (m + 1) u sum_i |x_ij| |p_i| for column j (m products, m - 1 adds: gamma_m; the factor 2
    covers the reference's own rounding), the same with n and q for row i."""
    m, n = len(p), len(q)
    X = np.asarray(x, np.float64).reshape((m, n), order="F").astype(LD)
    pl, ql = np.asarray(p, np.float64).astype(LD), np.asarray(q, np.float64).astype(LD)
    cols = (X * pl[:, None]).sum(axis=0)
    rows = (X * ql[None, :]).sum(axis=1)
    bc = 2 * (m + 1) * LD(U) * (np.abs(X) * np.abs(pl)[:, None]).sum(axis=0)
    br = 2 * (n + 1) * LD(U) * (np.abs(X) * np.abs(ql)[None, :]).sum(axis=1)
    return np.concatenate([cols, rows]), np.concatenate([bc, br])


def within(got, ref, bound):
    """|got - ref| <= bound entry by entry, in longdouble; returns the worst ratio for the report."""
    d = np.abs(np.asarray(got, np.float64).astype(LD) - ref)
    ok = bool(np.all(d <= bound))
    pos = bound > 0
    worst = float(np.max(d[pos] / bound[pos])) if np.any(pos) else 0.0
    return ok and bool(np.all(d[~pos] == 0)), worst


# ---------------------------------------------------------------------------------------------------------------
# ASAt: masks
# ---------------------------------------------------------------------------------------------------------------
# (m, n): full 64-row tiles, a partial last tile, m % 8 == 0 (the 8-byte loads are possible at all)
ASAT_SHAPES = {(8, 3): (0, True, True), (64, 64): (1, False, True), (72, 65): (1, True, True),
               (128, 130): (2, False, True), (65, 63): (1, True, False)}
ASAT_OFFSETS = [0, 8, 1, 4]            # 0, 8: 8-byte aligned (wide loads when m % 8 == 0); 1, 4: byte loads
ASAT_DENSITIES = [0.0, 0.02, 0.5, 1.0]
MASK_FLAVOURS = {"01": (1,), "mixed": (1, 2, 0x10, 0x80, 0xFF), "bit0clear": (2, 0x80)}


def mask_bytes(m, n, density, flavour, seed=0):
    """m*n mask bytes, column-major: an entry is nonzero with probability `density` (0: none, 1: all), a nonzero
    entry is drawn from the flavour's byte values."""
    rs = np.random.RandomState(1000 * m + 10 * n + seed)
    on = rs.random_sample(m * n) < density
    vals = np.array(MASK_FLAVOURS[flavour], np.uint8)
    return np.where(on, vals[rs.randint(0, len(vals), m * n)], 0).astype(np.uint8)


def bytes_to_bits_model(x):
    """ipd_asat.hip's bytes_to_bits on one 64-bit word, in Python integers."""
    x |= x >> 4
    x |= x >> 2
    x |= x >> 1
    x &= 0x0101010101010101
    return ((x * 0x0102040810204080) & 0xFFFFFFFFFFFFFFFF) >> 56


# ---------------------------------------------------------------------------------------------------------------
# SpMV: matrices, reference and bound
# ---------------------------------------------------------------------------------------------------------------
def spmv_rules():
    """(grid cap in workgroups, [(avg row length bound, L), ...]) as csr_spmv (ipd_sparse.hip) states them."""
    with open(os.path.join(CSRC, "ipd_sparse.hip")) as fh:
        src = fh.read()
    body = src[src.index("void csr_spmv("):]
    body = body[:body.index("\n}\n")]
    cap = int(re.search(r"\(threads \+ 255\) / 256, (\d+)\)", body).group(1))
    cuts = [(float(a), int(l)) for a, l in re.findall(r"avg <= (\d+)\)\s*launch\(k_spmv<(\d+)>", body)]
    last = int(re.search(r"else\s*launch\(k_spmv<(\d+)>", body).group(1))
    return cap, cuts + [(float("inf"), last)]


def spmv_branch(A, rules=None):
    cap, cuts = rules or spmv_rules()
    avg = A.nnz / A.shape[0]
    for bound, L in cuts:
        if avg <= bound:
            return L
    raise AssertionError


def csr_from_lengths(lens, nc, seed):
    """Rows of the given lengths, distinct ascending random columns, standard normal values."""
    rs = np.random.RandomState(seed)
    lens = np.asarray(lens, np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)])
    ci = np.concatenate([np.sort(rs.choice(nc, int(k), replace=False)) for k in lens] + [np.zeros(0, np.int64)])
    va = rs.standard_normal(int(indptr[-1]))
    return sp.csr_matrix((va, ci.astype(np.int64), indptr), shape=(len(lens), nc))


def branch_matrix(L, fill, nr=300, nc=257, seed=0):
    """One matrix of branch L: rows of length 0, 1, L-1, L, L+1 and 3L+5 among rows of `fill` entries."""
    special = [0, 1, L - 1, L, L + 1, 3 * L + 5]
    lens = np.full(nr, fill)
    lens[np.linspace(3, nr - 4, len(special)).astype(int)] = special
    lens[0], lens[-1] = special[-1], special[0]        # the longest row first, an empty row last
    return csr_from_lengths(lens, nc, seed + L)


def uniform_matrix(nr, k, nc=64, seed=0):
    """nr rows of exactly k entries each in nc columns (distinct, ascending), built without a Python loop."""
    rs = np.random.RandomState(seed + k)
    if k == 2:
        c0 = rs.randint(0, nc, nr)
        c1 = (c0 + 1 + rs.randint(0, nc - 1, nr)) % nc
        ci = np.sort(np.stack([c0, c1], axis=1), axis=1)
    else:
        ci = np.sort(np.argsort(rs.random_sample((nr, nc)), axis=1)[:, :k], axis=1)
    va = rs.standard_normal(nr * k)
    return sp.csr_matrix((va, ci.reshape(-1).astype(np.int64), np.arange(nr + 1, dtype=np.int64) * k), shape=(nr, nc))


# name -> (builder, branch L); the "cap" matrices have one row more than cap * 256 / L row groups
SPMV_MATRICES = {
    "L4": (lambda: branch_matrix(4, 3), 4),
    "L16": (lambda: branch_matrix(16, 12), 16),
    "L64": (lambda: branch_matrix(64, 40), 64),
    "one_row": (lambda: csr_from_lengths([30], 50, 1), 64),
    "one_column": (lambda: csr_from_lengths([1, 0, 1, 1, 0, 0, 1], 1, 2), 4),
    "one_by_one": (lambda: csr_from_lengths([1], 1, 3), 4),
    "cap_L4": (lambda: uniform_matrix(524289, 2), 4),
    "cap_L16": (lambda: uniform_matrix(131073, 7), 16),
    "cap_L64": (lambda: uniform_matrix(32769, 25), 64),
}


def spmv_ref(A, x):
    """A*x with products and sums in longdouble, and per row 2 (len_r + 1) u sum_t |a_rt| |x_c|."""
    A = sp.csr_matrix(A)
    nr = A.shape[0]
    lens = np.diff(A.indptr)
    prod = A.data.astype(LD) * np.asarray(x, np.float64).astype(LD)[A.indices]
    ref, mag = np.zeros(nr, LD), np.zeros(nr, LD)
    rows = np.flatnonzero(lens)
    if rows.size:
        starts = A.indptr[rows]
        ref[rows] = np.add.reduceat(prod, starts)
        mag[rows] = np.add.reduceat(np.abs(prod), starts)
    return ref, 2 * (lens + 1).astype(LD) * LD(U) * mag
