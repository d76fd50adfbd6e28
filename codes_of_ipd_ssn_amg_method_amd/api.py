"""Host-side mirror of the reference's MATLAB function signatures.

Same names, argument meaning and error behaviour as the reference's ``.m``
files; every call goes through the C ABI of libipdamg.so
(hand-written HIP, gfx950).  MATLAB itself is not available in this pipeline,
so this Python layer plays the role of the MEX gateway for tests and benches;
the gateway a MATLAB maintainer would compile is ``mex/ipd_mex.cpp``.

Differences forced by the host language, all documented in INTEGRATION.md:
 * indices are 0-based;
 * functions that consume MATLAB's global ``rand`` stream take a ``rng``
   argument (``MatlabRand``; seed 5489 reproduces MATLAB's default stream);
 * the reference's ``global Ack Prok J smoth_it Rk`` is the ``AMGHierarchy``
   handle; ``MG_Vcycle``/``MG_Wcycle`` take it as first argument.
"""
from __future__ import annotations

from ctypes import byref, c_double, c_int, c_int32, c_int64, c_void_p, POINTER

import numpy as np
import scipy.sparse as sp

from . import _lib as L
from ._lib import CscIn, IpdError, MatlabRand, bptr, check, csc_out_to_scipy, dptr, f64, get_ctx, \
    iptr, lib, u8

__all__ = [
    "Ax", "Aty", "ASAt", "invAAt", "invHHt", "strength", "cf_split", "mis_set", "transfer",
    "Class_AMG", "AMGHierarchy", "MG_Vcycle", "MG_Wcycle", "PCG", "components", "Hybrid_AMG",
    "AMG4POT", "MatlabRand", "IpdError", "amg_options", "APDWorkspace", "warmup_class1",
    "warmup_class2", "APD_SsN_Class1", "APD_SsN_Class2", "twogrid_bigph", "twogrid", "Hybrid_twogrid",
    "aug_PCG", "PCG4POT", "load_input", "sparse_multiply", "spd_solve", "AMG_PCG",
    "Class_AMG_multi", "AMG_PCG_multi", "Hybrid_AMG_PCG",
    "point_cost", "projection_order", "APD_SsN_Class1_points", "APD_SsN_Class2_points",
]


def _h():
    return get_ctx().handle


# ---------------------------------------------------------------------------
# options structs
# ---------------------------------------------------------------------------
def amg_options(retol=None, bigph=None, maxit=None, theta=None, smoth=None, cycle=None,
                isnsp=None, inter=None, guess=None, fnode=None) -> dict:
    """``struct('retol',..,'bigph',..,...)`` with ``[]`` spelled ``None``."""
    return dict(retol=retol, bigph=bigph, maxit=maxit, theta=theta, smoth=smoth, cycle=cycle,
                isnsp=isnsp, inter=inter, guess=guess, fnode=fnode)


def _opts_struct(o: dict | None) -> L.ipd_amg_opts:
    s = L.ipd_amg_opts()
    lib.ipd_amg_opts_init(byref(s))
    if o is None:
        # Class_AMG.m:22-23 (nargin == 2 defaults; note cycle = 1 selects no cycle)
        o = dict(retol=1e-12, bigph=0, maxit=20, theta=1 / 4, smoth=10, cycle=1, isnsp=1, inter=1)
    for key in ("retol", "theta"):
        if o.get(key) is not None:
            setattr(s, key, float(o[key]))
    for key in ("bigph", "maxit", "smoth", "isnsp", "inter"):
        if o.get(key) is not None:
            setattr(s, key, int(o[key]))
    if o.get("cycle") is not None:
        cyc = o["cycle"]
        s.cycle = ord(cyc) if isinstance(cyc, str) and len(cyc) == 1 else int(cyc)
    if o.get("fnode") is not None:
        s.fnode = int(o["fnode"])
    return s


# ---------------------------------------------------------------------------
# L0 / L1
# ---------------------------------------------------------------------------
def Ax(x, p, q) -> np.ndarray:
    """``y = Ax(x,p,q)`` (``Ax.m:2``)."""
    p, q, x = f64(p), f64(q), f64(x)
    m, n = p.size, q.size
    if x.size != m * n:
        raise ValueError("Ax: length(x) must be length(p)*length(q)")
    y = np.empty(m + n)
    check(lib.ipd_ax(_h(), dptr(x), dptr(p), dptr(q), c_int64(m), c_int64(n), dptr(y)))
    return y


def Aty(y, p, q) -> np.ndarray:
    """``z = Aty(y,p,q)`` (``Aty.m:2``)."""
    p, q, y = f64(p), f64(q), f64(y)
    m, n = p.size, q.size
    if y.size < m + n:
        raise ValueError("Aty: y needs n+m entries")
    z = np.empty(m * n)
    check(lib.ipd_aty(_h(), dptr(y), dptr(p), dptr(q), c_int64(m), c_int64(n), dptr(z)))
    return z


def ASAt(s, p, q) -> sp.csc_matrix:
    """``H = ASAt(s,p,q)`` (``ASAt.m:2``); ``s`` logical of length m*n."""
    p, q, s = f64(p), f64(q), u8(s)
    m, n = p.size, q.size
    if s.size != m * n:
        raise ValueError("ASAt: length(s) must be length(p)*length(q)")
    out = L.ipd_csc_out()
    check(lib.ipd_asat(_h(), bptr(s), dptr(p), dptr(q), c_int64(m), c_int64(n), byref(out)))
    return csc_out_to_scipy(out)


def invAAt(x, p, q, sg1=None, sg2=None) -> np.ndarray:
    """``y = invAAt(x,p,q,sg1,sg2)`` (``invAAt.m:1``; nargin rules ``:7-12``)."""
    if sg1 is None:
        sg1, sg2 = 1.0, 1.0
    elif sg2 is None:
        sg2 = sg1
    p, q, x = f64(p), f64(q), f64(x)
    m, n = p.size, q.size
    y = np.empty(m + n)
    check(lib.ipd_inv_aat(_h(), dptr(x), dptr(p), dptr(q), c_int64(m), c_int64(n), c_double(sg1),
                          c_double(sg2), dptr(y)))
    return y


def invHHt(v, p, q, sg, phi) -> np.ndarray:
    """``y = invHHt(v,p,q,sg,phi)`` (``Class2/invHHt.m:1``)."""
    p, q, v, phi = f64(p), f64(q), f64(v), f64(phi)
    m, n = p.size, q.size
    y = np.empty(m + n + 1)
    check(lib.ipd_inv_hht(_h(), dptr(v), dptr(p), dptr(q), c_int64(m), c_int64(n), c_double(sg),
                          dptr(phi), dptr(y)))
    return y


# ---------------------------------------------------------------------------
# L2: setup pieces
# ---------------------------------------------------------------------------
def strength(A, which: int = 2) -> sp.csc_matrix:
    """``S = strength(A,which)`` (``AMG/strength.m:1``)."""
    a = CscIn(A)
    out = L.ipd_csc_out()
    check(lib.ipd_strength(_h(), a.ref(), c_int(which), byref(out)))
    return csc_out_to_scipy(out)


def cf_split(S):
    """``[indC,indF] = cf_split(S)`` (``AMG/cf_split.m:1``)."""
    a = CscIn(S)
    n = a.struct.nrows
    indC = np.zeros(n, np.uint8)
    indF = np.zeros(n, np.uint8)
    check(lib.ipd_cf_split(_h(), a.ref(), bptr(indC), bptr(indF)))
    return indC.astype(bool), indF.astype(bool)


def mis_set(A, theta: float = 0.025, rng: MatlabRand | None = None):
    """``[isC,isF,As] = mis_set(A,theta)`` (``AMG/mis_set.m:1``)."""
    rng = rng or MatlabRand()
    a = CscIn(A)
    n = a.struct.nrows
    isC = np.zeros(n, np.uint8)
    isF = np.zeros(n, np.uint8)
    out = L.ipd_csc_out()
    check(lib.ipd_mis_set(_h(), a.ref(), c_double(theta), rng.handle, bptr(isC), bptr(isF),
                          byref(out)))
    return isC.astype(bool), isF.astype(bool), csc_out_to_scipy(out)


def sparse_multiply(A, B) -> sp.csc_matrix:
    """``A*B`` for sparse operands with the summation order of MATLAB's sparse ``mtimes`` (every
    entry accumulated in ascending inner index; ``transfer.m:66`` forms ``Pro'*A*Pro`` with it).
    The device kernels are the ones the setup uses (row kernel or register tiles)."""
    a, b = CscIn(A), CscIn(B)
    if a.struct.ncols != b.struct.nrows:
        raise ValueError("sparse_multiply: inner dimensions differ")
    da, db, dc = c_void_p(), c_void_p(), c_void_p()
    out = L.ipd_csc_out()
    try:
        check(lib.ipd_dmat_upload(_h(), a.ref(), c_int32(0), byref(da)))
        check(lib.ipd_dmat_upload(_h(), b.ref(), c_int32(0), byref(db)))
        check(lib.ipd_dmat_multiply(_h(), da, db, byref(dc)))
        check(lib.ipd_dmat_download(_h(), dc, byref(out)))
    finally:
        for d in (da, db, dc):
            if d:
                lib.ipd_dmat_destroy(d)
    return csc_out_to_scipy(out)


def spd_solve(A, B) -> np.ndarray:
    """``X = A \\ B`` for sparse symmetric positive definite ``A`` and dense ``B`` -- the
    reference's direct solves (``APD_SsN_Class1.m:148``, ``APD_SsN_Class2.m:155``,
    ``AMG/transfer.m:58``), a blocked dense Cholesky on the device."""
    a = CscIn(A)
    B = np.asarray(B, dtype=np.float64)
    one = B.ndim == 1
    B2 = B.reshape(-1, 1) if one else B
    n, nrhs = B2.shape
    if n != a.struct.nrows:
        raise ValueError("spd_solve: B must have as many rows as A")
    Bf = np.asfortranarray(B2)
    X = np.empty_like(Bf, order="F")
    check(lib.ipd_spd_solve(_h(), a.ref(), Bf.ctypes.data_as(POINTER(c_double)), c_int64(nrhs),
                            X.ctypes.data_as(POINTER(c_double))))
    return X[:, 0].copy() if one else np.ascontiguousarray(X)


def transfer(A, amg_options: dict, level: int = 2, rng: MatlabRand | None = None):
    """``[Ac,Pro,~,indC] = transfer(A,amg_options)`` (``AMG/transfer.m:1``);
    ``level`` is the reference's ``global J``."""
    rng = rng or MatlabRand()
    a = CscIn(A)
    o = _opts_struct(amg_options)
    Ac, Pro = L.ipd_csc_out(), L.ipd_csc_out()
    indC = np.zeros(a.struct.nrows, np.uint8)
    check(lib.ipd_transfer(_h(), a.ref(), byref(o), c_int(level), rng.handle, byref(Ac),
                           byref(Pro), bptr(indC)))
    return csc_out_to_scipy(Ac), csc_out_to_scipy(Pro), indC.astype(bool)


# ---------------------------------------------------------------------------
# L3: hierarchy, cycles, PCG
# ---------------------------------------------------------------------------
class AMGHierarchy:
    """Device-resident ``Ack/Prok/Rk/J`` (``AMG/Class_AMG.m:42-85``)."""

    def __init__(self, A, amg_options: dict, rng: MatlabRand | None = None, ctx=None):
        self.ctx = ctx or get_ctx()      # an own L.Context = an own HIP stream (concurrent use)
        self.rng = rng or MatlabRand()
        self._a = CscIn(A)
        self.opts = dict(amg_options) if amg_options is not None else None
        o = _opts_struct(amg_options)
        self.handle = c_void_p()
        check(lib.ipd_amg_setup(self.ctx.handle, self._a.ref(), byref(o), self.rng.handle,
                                byref(self.handle)))
        self.maxit = int(o.maxit) if o.maxit >= 0 else 50
        self.N = int(self._a.struct.nrows)

    @property
    def J(self) -> int:
        return int(lib.ipd_amg_num_levels(self.handle))

    def attach_mask_operator(self, p, q, tk) -> bool:
        """Matrix-free level 1 (``ipd_amg_attach_mask_operator``): True when level 1 is exactly
        Hybrid_AMG's rescaled operator for these ``p, q, tk`` and the 1-bit-per-entry sweeps are
        now in use; False leaves the CSR kernels in place."""
        p_, q_ = f64(p), f64(q)
        dp = L.DeviceBuffer.from_array(p_, self.ctx)
        dq = L.DeviceBuffer.from_array(q_, self.ctx)
        got = c_int32(0)
        check(lib.ipd_amg_attach_mask_operator(self.handle, dp.ptr, dq.ptr, c_int64(p_.size),
                                               c_int64(q_.size), c_double(float(tk)), byref(got)))
        self.ctx.sync()
        return bool(got.value)

    def attach_mask_transfers(self, p, q, tk) -> bool:
        """``ipd_amg_attach_mask_transfers``: the level-resident kernel's level 1 <-> 2 transfers from the
        bit mask (True when in use)."""
        p_, q_ = f64(p), f64(q)
        dp = L.DeviceBuffer.from_array(p_, self.ctx)
        dq = L.DeviceBuffer.from_array(q_, self.ctx)
        got = c_int32(0)
        check(lib.ipd_amg_attach_mask_transfers(self.handle, dp.ptr, dq.ptr, c_int64(p_.size),
                                                c_int64(q_.size), c_double(float(tk)), byref(got)))
        self.ctx.sync()
        return bool(got.value)

    def attach_level2_poly(self) -> bool:
        """``ipd_amg_attach_level2_poly``: level 2 of the level-resident kernel composed over a whole visit
        (three levels, one-row tail, V cycle: ONE hand-off per visit instead of ten).  True when in use."""
        got = c_int32(0)
        check(lib.ipd_amg_attach_level2_poly(self.handle, byref(got)))
        self.ctx.sync()
        return bool(got.value)

    def resident_variant(self):
        """``ipd_amg_resident_variant``: (full, diag) of the last resident launch -- the full-shape form of the
        composed kernel, and the form that holds the stamps and the test hook."""
        full, diag = c_int32(0), c_int32(0)
        check(lib.ipd_amg_resident_variant(self.handle, byref(full), byref(diag)))
        return bool(full.value), bool(diag.value)

    def level_dims(self, k: int):
        rows, nnz = c_int64(), c_int64()
        check(lib.ipd_amg_level_dims(self.handle, c_int(k), byref(rows), byref(nnz)))
        return int(rows.value), int(nnz.value)

    def level_sizes(self):
        return [self.level_dims(k)[0] for k in range(1, self.J + 1)]

    def level_forms(self):
        """forms[k - 1] for level k = 1..J: bit mask of how the level runs inside the single-workgroup
        LDS images (include/ipd_amg.h, ipd_amg_level_forms); 0 = in no image."""
        buf = (c_int32 * (self.J + 1))()
        check(lib.ipd_amg_level_forms(self.handle, buf, c_int32(self.J + 1)))
        return [int(buf[k]) for k in range(1, self.J + 1)]

    def A(self, k: int) -> sp.csc_matrix:
        out = L.ipd_csc_out()
        check(lib.ipd_amg_get_A(self.handle, c_int(k), byref(out)))
        return csc_out_to_scipy(out)

    def P(self, k: int) -> sp.csc_matrix:
        out = L.ipd_csc_out()
        check(lib.ipd_amg_get_P(self.handle, c_int(k), byref(out)))
        return csc_out_to_scipy(out)

    def cmask(self, k: int) -> np.ndarray:
        rows = self.level_dims(k - 1)[0]
        m = np.zeros(rows, np.uint8)
        check(lib.ipd_amg_get_cmask(self.handle, c_int(k), bptr(m)))
        return m.astype(bool)

    def solve(self, b, guess=None):
        """Solve phase of Class_AMG: ``x, it, rel_res, rel_resk, rhok``."""
        b = f64(b)
        x = np.empty(self.N)
        it = c_int32()
        rel = c_double()
        rel_resk = np.full(self.maxit + 2, np.nan)
        rhok = np.full(self.maxit + 2, np.nan)
        g = f64(guess) if guess is not None else None
        check(lib.ipd_amg_solve(self.handle, dptr(b), dptr(g) if g is not None else None, dptr(x),
                                byref(it), byref(rel), dptr(rel_resk), dptr(rhok)))
        n = it.value + 1
        return x, int(it.value), float(rel.value), rel_resk[:n].copy(), rhok[:n].copy()

    def solve_multi(self, B, guess=None):
        """Several right-hand sides (``ipd_amg_solve_multi``): column j of ``B`` (N x k) through the
        solve phase of Class_AMG as if solved alone.  Returns ``X`` (N x k), ``it`` (k,), ``rel_res``
        (k,) and the lists of the k ``rel_resk`` and ``rhok`` histories (``it[j] + 1`` entries each).
        For one right-hand side ``solve`` stays the faster call."""
        Bf, gf, k = multi_args(self.N, B, guess)
        X = np.empty((self.N, k), order="F")
        it = np.zeros(k, np.int32)
        rel = np.zeros(k)
        hs = self.maxit + 1
        rel_resk = np.full((hs, k), np.nan, order="F")
        rhok = np.full((hs, k), np.nan, order="F")
        check(lib.ipd_amg_solve_multi(self.handle, dptr(Bf), self.N, k, dptr(gf) if gf is not None else None,
                                      dptr(X), it.ctypes.data_as(POINTER(c_int32)), dptr(rel),
                                      dptr(rel_resk), dptr(rhok)))
        n = [int(v) + 1 for v in it]
        return (X, it.astype(np.int64), rel, [rel_resk[:n[j], j].copy() for j in range(k)],
                [rhok[:n[j], j].copy() for j in range(k)])

    def pcg(self, e, pcg_options: dict | None = None, planned: bool = False):
        """``[d,it,res,resk] = AMG_PCG(h,e,pcg_options)`` (``ipd_amg_pcg``): PCG.m's loop on level 1
        preconditioned by one cycle of this hierarchy, flexible beta.  ``pcg_options``: ``retol``,
        ``maxit``, ``guess``; ``precd`` must stay unset.  ``resk`` has ``maxit`` slots like ``PCG``.
        ``planned=True`` (``ipd_amg_pcg_planned``): the whole loop as ONE single-workgroup launch where
        the hierarchy is planned for the single-workgroup solve and ``maxit`` <= 1000 (the default
        1e4 is beyond it), the same launches elsewhere; ``pcg_mode`` tells which it was."""
        e = f64(e)
        o = _pcg_opts_struct(pcg_options)
        g = None
        if pcg_options is not None and pcg_options.get("guess") is not None:
            g = f64(pcg_options["guess"])
        maxit = int(o.maxit) if o.maxit >= 0 else 10000
        d = np.empty(self.N)
        it = c_int64()
        res = c_double()
        resk = np.zeros(maxit)
        fn = lib.ipd_amg_pcg_planned if planned else lib.ipd_amg_pcg
        check(fn(self.handle, dptr(e), dptr(g) if g is not None else None, byref(o), dptr(d),
                 byref(it), byref(res), dptr(resk)))
        return d, int(it.value), float(res.value), resk

    @property
    def pcg_mode(self) -> int:
        """How the most recent ``pcg`` call on this hierarchy ran (``ipd_amg_pcg_mode``): -1 none yet,
        0 as launches, 1 as one single-workgroup launch."""
        mode = c_int32(-1)
        check(lib.ipd_amg_pcg_mode(self.handle, byref(mode)))
        return int(mode.value)

    def pcg_multi(self, E, pcg_options: dict | None = None):
        """Several right-hand sides (``ipd_amg_pcg_multi``): column j of ``E`` (N x k) through ``pcg``'s
        loop as if solved alone.  Returns ``D`` (N x k), ``it`` (k,), ``res`` (k,) and ``resk``
        (maxit x k, zeros past ``it[j]`` in column j).  ``pcg_options``: ``retol``, ``maxit``, ``guess``
        (N x k); ``precd`` must stay unset."""
        g = None if pcg_options is None else pcg_options.get("guess")
        Ef, gf, k = multi_args(self.N, E, g)
        o = _pcg_opts_struct(pcg_options)
        maxit = int(o.maxit) if o.maxit >= 0 else 10000
        D = np.empty((self.N, k), order="F")
        it = np.zeros(k, np.int64)
        res = np.zeros(k)
        resk = np.zeros((maxit, k), order="F")
        check(lib.ipd_amg_pcg_multi(self.handle, dptr(Ef), self.N, k, dptr(gf) if gf is not None else None,
                                    byref(o), dptr(D), it.ctypes.data_as(POINTER(c_int64)), dptr(res),
                                    dptr(resk)))
        return D, it, res, resk

    def cycle_bytes(self) -> float:
        v = c_double()
        check(lib.ipd_amg_cycle_bytes(self.handle, byref(v)))
        return float(v.value)

    def close(self):
        if self.handle:
            lib.ipd_amg_destroy(self.handle)
            self.handle = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def MG_Vcycle(h: AMGHierarchy, r, isnsp=0, k: int = 1) -> np.ndarray:
    """``e = MG_Vcycle(r,isnsp,k)`` (``AMG/MG_Vcycle.m:2``); ``k`` is 1-based."""
    r = f64(r)
    e = np.empty(h.level_dims(k)[0])
    check(lib.ipd_amg_vcycle(h.handle, dptr(r), c_int(int(isnsp)), c_int(k), dptr(e)))
    return e


def MG_Wcycle(h: AMGHierarchy, r, isnsp=0, k: int = 1, e=None) -> np.ndarray:
    """``e = MG_Wcycle(r,isnsp,k,e)`` (``AMG/MG_Wcycle.m:2``)."""
    r = f64(r)
    out = np.empty(h.level_dims(k)[0])
    ein = f64(e) if e is not None else None
    check(lib.ipd_amg_wcycle(h.handle, dptr(r), c_int(int(isnsp)), c_int(k),
                             dptr(ein) if ein is not None else None, dptr(out)))
    return out


def Class_AMG(A, b, amg_options: dict | None = None, rng: MatlabRand | None = None):
    """``[x,it,rel_res,rel_resk,rhok] = Class_AMG(A,b,amg_options)``
    (``AMG/Class_AMG.m:1``)."""
    h = AMGHierarchy(A, amg_options, rng)
    try:
        guess = None if amg_options is None else amg_options.get("guess")
        return h.solve(b, guess)
    finally:
        h.close()


def multi_args(N: int, B, guess=None):
    """``B`` (N x k, or a vector: k = 1) and ``guess`` (same shape or None) as column-major float64
    blocks with leading dimension N; ValueError on a shape that does not fit."""
    Bf = np.asarray(B, dtype=np.float64)
    if Bf.ndim == 1:
        Bf = Bf.reshape(-1, 1)
    if Bf.ndim != 2 or Bf.shape[0] != N or Bf.shape[1] < 1:
        raise ValueError(f"solve_multi: B must be {N} x k with k >= 1, got shape {np.shape(B)}")
    k = int(Bf.shape[1])
    Bf = np.asfortranarray(Bf)
    gf = None
    if guess is not None:
        gf = np.asarray(guess, dtype=np.float64)
        if gf.ndim == 1:
            gf = gf.reshape(-1, 1)
        if gf.shape != (N, k):
            raise ValueError(f"solve_multi: guess must be {N} x {k}, got shape {np.shape(guess)}")
        gf = np.asfortranarray(gf)
    return Bf, gf, k


def Class_AMG_multi(A, B, amg_options: dict | None = None, rng: MatlabRand | None = None):
    """``[X,it,rel_res,rel_resk,rhok] = Class_AMG_multi(A,B,amg_options)``: one Class_AMG setup, then
    every column of ``B`` through its solve phase (``AMGHierarchy.solve_multi``).  A guess in
    ``amg_options`` is N x k."""
    h = AMGHierarchy(A, amg_options, rng)
    try:
        guess = None if amg_options is None else amg_options.get("guess")
        return h.solve_multi(B, guess)
    finally:
        h.close()


def AMG_PCG(A, b, amg_options: dict, pcg_options: dict | None = None, rng: MatlabRand | None = None,
            planned: bool = False):
    """``[d,it,res,resk] = AMG_PCG(A,b,amg_options,pcg_options)``: Class_AMG's setup, then
    conjugate gradients preconditioned by one cycle of the hierarchy (``AMGHierarchy.pcg``;
    ``planned``: as one launch where the hierarchy allows it)."""
    h = AMGHierarchy(A, amg_options, rng)
    try:
        return h.pcg(b, pcg_options, planned)
    finally:
        h.close()


def AMG_PCG_multi(A, E, amg_options: dict, pcg_options: dict | None = None, rng: MatlabRand | None = None):
    """``[D,it,res,resk] = AMG_PCG_multi(A,E,amg_options,pcg_options)``: Class_AMG's setup, then every
    column of ``E`` through AMG-preconditioned CG as if solved alone (``AMGHierarchy.pcg_multi``).  A
    guess in ``pcg_options`` is N x k."""
    h = AMGHierarchy(A, amg_options, rng)
    try:
        return h.pcg_multi(E, pcg_options)
    finally:
        h.close()


def PCG(H, e, pcg_options: dict | None = None):
    """``[d,it,res,resk] = PCG(H,e,pcg_options)`` (``PCG.m:1``)."""
    e = f64(e)
    a = CscIn(H)
    o = L.ipd_pcg_opts()
    lib.ipd_pcg_opts_init(byref(o))
    guess = None
    if pcg_options is not None:
        if pcg_options.get("retol") is not None:
            o.retol = float(pcg_options["retol"])
        if pcg_options.get("maxit") is not None:
            o.maxit = int(pcg_options["maxit"])
        if pcg_options.get("precd") is not None:
            o.precd = int(pcg_options["precd"])
        if pcg_options.get("nf") is not None:
            o.nf = int(pcg_options["nf"])
        if pcg_options.get("guess") is not None:
            guess = f64(pcg_options["guess"])
        if o.precd == 5 and "nf" not in pcg_options:
            raise ValueError("SSOR for bigraph requires pcg_options.nf!!!")   # PCG.m:64
    maxit = int(o.maxit) if o.maxit >= 0 else 10000
    d = np.empty(e.size)
    it = c_int64()
    res = c_double()
    resk = np.zeros(maxit)
    check(lib.ipd_pcg(_h(), a.ref(), dptr(e), dptr(guess) if guess is not None else None, byref(o),
                      dptr(d), byref(it), byref(res), dptr(resk)))
    return d, int(it.value), float(res.value), resk


# ---------------------------------------------------------------------------
# L4
# ---------------------------------------------------------------------------
def components(A):
    """``[blocks,sizes,p,r] = components(A)`` (``components.m:1``), 0-based."""
    a = CscIn(A)
    n = int(a.struct.nrows)
    blocks = np.zeros(n, np.int64)
    sizes = np.zeros(n, np.int64)
    p = np.zeros(n, np.int64)
    r = np.zeros(n + 1, np.int64)
    nc = c_int64()
    check(lib.ipd_components(_h(), a.ref(), iptr(blocks), iptr(sizes), iptr(p), iptr(r), byref(nc)))
    k = int(nc.value)
    return blocks, sizes[:k].copy(), p, r[:k + 1].copy()


def _prob_struct(pd: dict, need_pot: bool):
    keep = []
    p, q = f64(pd["p"]), f64(pd["q"])
    m, n = p.size, q.size
    T = pd.get("T")
    t = None
    if T is not None:
        t = f64(sp.csr_matrix(T).diagonal() if sp.issparse(T) else np.asarray(T))
        if not np.any(t):
            t = None
    H0 = CscIn(pd["H0"])
    z = f64(pd["z"])
    s = L.ipd_prob()
    s.m, s.n, s.bk1, s.tk = m, n, float(pd["bk1"]), float(pd["tk"])
    s.p, s.q = dptr(p), dptr(q)
    s.t = dptr(t) if t is not None else None
    s.H0 = POINTER(L.ipd_csc)(H0.struct)
    s.z = dptr(z)
    keep += [p, q, t, H0, z]
    if need_pot:
        sm = u8(pd["s"])
        phi = f64(pd["phi"])
        s.s, s.phi = bptr(sm), dptr(phi)
        keep += [sm, phi]
    return s, keep, m, n


def Hybrid_AMG(prob_data: dict, amg_options: dict, rng: MatlabRand | None = None):
    """``[zeta,itamg,resamg,info] = Hybrid_AMG(prob_data,amg_options)``
    (``Hybrid_AMG.m:1``)."""
    rng = rng or MatlabRand()
    s, keep, m, n = _prob_struct(prob_data, False)
    o = _opts_struct(amg_options)
    zeta = np.empty(m + n)
    it = c_int32()
    res = c_double()
    info = np.zeros(2, np.int64)
    check(lib.ipd_hybrid_amg(_h(), byref(s), byref(o), rng.handle, dptr(zeta), byref(it),
                             byref(res), iptr(info)))
    return zeta, int(it.value), float(res.value), info


def Hybrid_AMG_PCG(prob_data: dict, amg_options: dict, rng: MatlabRand | None = None):
    """``[zeta,itamg,resamg,info] = Hybrid_AMG_PCG(prob_data,amg_options)`` (``ipd_hybrid_amg_pcg``):
    ``Hybrid_AMG`` with AMG-preconditioned CG (``AMGHierarchy.pcg(planned=True)``) in place of every
    ``Class_AMG`` solve phase -- same rescaling, components, random guesses (the ``rand`` stream
    advances as in ``Hybrid_AMG``) and small-block direct solves; ``retol`` / ``maxit`` are
    ``amg_options``'; ``itamg`` / ``resamg`` are the largest PCG count / ``res`` over the large
    components."""
    rng = rng or MatlabRand()
    s, keep, m, n = _prob_struct(prob_data, False)
    o = _opts_struct(amg_options)
    zeta = np.empty(m + n)
    it = c_int32()
    res = c_double()
    info = np.zeros(2, np.int64)
    check(lib.ipd_hybrid_amg_pcg(_h(), byref(s), byref(o), rng.handle, dptr(zeta), byref(it),
                                 byref(res), iptr(info)))
    return zeta, int(it.value), float(res.value), info


def Hybrid_twogrid(prob_data: dict, amg_options: dict, rng: MatlabRand | None = None):
    """``[zeta,itamg,resamg,info] = Hybrid_twogrid(prob_data,amg_options)``
    (``Hybrid_twogrid.m:1``)."""
    rng = rng or MatlabRand()
    s, keep, m, n = _prob_struct(prob_data, False)
    o = _opts_struct(amg_options)
    zeta = np.empty(m + n)
    it = c_int32()
    res = c_double()
    info = np.zeros(2, np.int64)
    check(lib.ipd_hybrid_twogrid(_h(), byref(s), byref(o), rng.handle, dptr(zeta), byref(it),
                                 byref(res), iptr(info)))
    return zeta, int(it.value), float(res.value), info


def twogrid_bigph(A, b, amg_options: dict | None = None):
    """``[x,it,rel_res,rel_resk,rhok] = twogrid_bigph(A,b,amg_options)``
    (``AMG/twogrid_bigph.m:1``); ``amg_options.fnode`` is required."""
    b = f64(b)
    if amg_options is None:                       # :6-9 (fnode = 0 cannot work; kept as an error)
        amg_options = dict(retol=1e-12, maxit=20, fnode=0, smoth=10, isnsp=1, guess=None)
    a = CscIn(A)
    o = _opts_struct(dict(amg_options))
    maxit = int(o.maxit) if o.maxit >= 0 else 50
    x = np.empty(b.size)
    it = c_int32()
    rel = c_double()
    rel_resk = np.full(maxit + 2, np.nan)
    rhok = np.full(maxit + 2, np.nan)
    g = amg_options.get("guess")
    g = f64(g) if g is not None else None
    check(lib.ipd_twogrid_bigph(_h(), a.ref(), dptr(b), dptr(g) if g is not None else None, byref(o),
                                dptr(x), byref(it), byref(rel), dptr(rel_resk), dptr(rhok)))
    k = it.value + 1
    return x, int(it.value), float(rel.value), rel_resk[:k].copy(), rhok[:k].copy()


def twogrid(A, b, amg_options: dict | None = None, rng: MatlabRand | None = None):
    """``[x,it,rel_res,rel_resk,rhok] = twogrid(A,b,amg_options)`` (``AMG/twogrid.m:1``)."""
    b = f64(b)
    if amg_options is None:                                               # :6-9
        amg_options = dict(retol=1e-12, bigph=0, maxit=20, smoth=10, isnsp=1, guess=None)
    if amg_options.get("bigph") and not (amg_options.get("fnode") or 0) > 0:
        raise ValueError("bigph = 1 requires fnode > 0")                  # :24-26
    rng = rng or MatlabRand()
    a = CscIn(A)
    o = _opts_struct(dict(amg_options))
    maxit = int(o.maxit) if o.maxit >= 0 else 50
    x = np.empty(b.size)
    it = c_int32()
    rel = c_double()
    rel_resk = np.full(maxit + 2, np.nan)
    rhok = np.full(maxit + 2, np.nan)
    g = amg_options.get("guess")
    g = f64(g) if g is not None else None
    check(lib.ipd_twogrid(_h(), a.ref(), dptr(b), dptr(g) if g is not None else None, byref(o),
                          rng.handle, dptr(x), byref(it), byref(rel), dptr(rel_resk), dptr(rhok)))
    k = it.value + 1
    return x, int(it.value), float(rel.value), rel_resk[:k].copy(), rhok[:k].copy()


def _pcg_opts_struct(o: dict | None) -> L.ipd_pcg_opts:
    s = L.ipd_pcg_opts()
    lib.ipd_pcg_opts_init(byref(s))
    if o:
        if o.get("retol") is not None:
            s.retol = float(o["retol"])
        if o.get("maxit") is not None:
            s.maxit = int(o["maxit"])
        if o.get("precd") is not None:
            s.precd = int(o["precd"])
    return s


def aug_PCG(prob_data: dict, pcg_options: dict | None = None):
    """``[zeta,itpcg,respcg,info] = aug_PCG(prob_data,pcg_options)`` (``aug_PCG.m:1``)."""
    s, keep, m, n = _prob_struct(prob_data, False)
    o = _pcg_opts_struct(pcg_options)
    zeta = np.empty(m + n)
    it = c_int64()
    res = c_double()
    info = np.zeros(2, np.int64)
    check(lib.ipd_aug_pcg(_h(), byref(s), byref(o), dptr(zeta), byref(it), byref(res), iptr(info)))
    return zeta, int(it.value), float(res.value), info


def PCG4POT(prob_data: dict, pcg_options: dict | None = None):
    """``[zeta,itpcg,respcg,info] = PCG4POT(prob_data,pcg_options)``
    (``Class2/PCG4POT.m:1``)."""
    s, keep, m, n = _prob_struct(prob_data, True)
    o = _pcg_opts_struct(pcg_options)
    zeta = np.empty(m + n + 1)
    it = c_int64()
    res = c_double()
    info = np.zeros(2, np.int64)
    check(lib.ipd_pcg4pot(_h(), byref(s), byref(o), dptr(zeta), byref(it), byref(res), iptr(info)))
    return zeta, int(it.value), float(res.value), info


def AMG4POT(prob_data: dict, amg_options: dict, str_: str = "amg", rng: MatlabRand | None = None):
    """``[zeta,itamg,resamg,info] = AMG4POT(prob_data,amg_options,str)``
    (``Class2/AMG4POT.m:1``); ``str`` = ``'amg'`` or ``'twogrid'`` (``:44-51``), or ``'amg_pcg'``: both
    ``Hybrid_AMG`` calls as ``Hybrid_AMG_PCG``."""
    if str_ not in ("amg", "twogrid", "amg_pcg"):
        raise ValueError("AMG4POT: str must be 'amg', 'twogrid' or 'amg_pcg'")
    rng = rng or MatlabRand()
    s, keep, m, n = _prob_struct(prob_data, True)
    o = _opts_struct(amg_options)
    zeta = np.empty(m + n + 1)
    it = c_int32()
    res = c_double()
    info = np.zeros(2, np.int64)
    fn = {"amg": lib.ipd_amg4pot, "twogrid": lib.ipd_amg4pot_twogrid, "amg_pcg": lib.ipd_amg4pot_pcg}[str_]
    check(fn(_h(), byref(s), byref(o), rng.handle, dptr(zeta), byref(it), byref(res), iptr(info)))
    return zeta, int(it.value), float(res.value), info


# ---------------------------------------------------------------------------
# L5: drivers and warm starts
# ---------------------------------------------------------------------------
class APDWorkspace:
    """The workspace of ``Class1/APD_SsN_Class1.m`` / ``Class2/APD_SsN_Class2.m`` in HBM.

    ``cls=1``: ``c, r, l, p, q, gama`` as loaded from ``InputData/data1-*.mat`` (``gama`` scalar,
    ``inf`` allowed, or an mn-vector); ``cls=2``: ``c (= C(:)), r, l, p, q, mu, phi`` of
    ``data4-*.mat``.  The scripts' variables are reachable as attributes/methods: ``state()``
    -> ``(uk, vk, lk, bk)``, ``history()`` -> ``fxk, KKT_xk, KKT_lk[, KKT_yk, KKT_zk],
    SsN_itnum``, ``records()`` -> what the scripts print per Newton step.
    """

    def __init__(self, cls, c, r, l, p, q, gama=np.inf, mu=0.0, phi=None, ctx=None):
        # ctx: an own L.Context (own HIP stream and arenas) lets several workspaces run
        # concurrently from several host threads; default = the process-wide context
        c_ = f64(c)
        d = self._data(cls, r, l, p, q, gama, mu, phi, ctx)
        if c_.size != self.m * self.n:
            raise ValueError("APDWorkspace: need length(l)=length(p)=m, length(r)=length(q)=n, "
                             "length(c)=m*n")
        if self.cls == 2 and phi is None:
            raise ValueError("class 2 needs phi")
        self._keep.append(c_)
        d.c = dptr(c_)
        check(lib.ipd_apd_create((ctx or get_ctx()).handle, byref(d), byref(self.handle)))

    def _data(self, cls, r, l, p, q, gama, mu, phi, ctx) -> L.ipd_apd_data:
        """Everything of ``ipd_apd_data`` but ``c``; sets the sizes and an empty handle."""
        self._ctx = ctx
        self.cls = int(cls)
        self._keep = [f64(r), f64(l), f64(p), f64(q)]
        r_, l_, p_, q_ = self._keep
        m, n = p_.size, q_.size
        if l_.size != m or r_.size != n:
            raise ValueError("APDWorkspace: need length(l)=length(p)=m, length(r)=length(q)=n, "
                             "length(c)=m*n")
        d = L.ipd_apd_data()
        d.cls, d.m, d.n = self.cls, m, n
        d.r, d.l, d.p, d.q = dptr(r_), dptr(l_), dptr(p_), dptr(q_)
        d.mu = float(mu)
        d.gama_scalar = np.inf
        self._gap_rule = False        # set_gap_rule: run() reports gap_stop and gap while a rule is set
        self._finite_gama = False     # class 1 with a finite scalar or a vector gama: the dual keeps its cap term
        if self.cls == 1:
            if np.ndim(gama) == 0 or np.size(gama) == 1:
                d.gama_scalar = float(np.asarray(gama).reshape(-1)[0])
                self._finite_gama = bool(np.isfinite(d.gama_scalar))
            else:
                self._finite_gama = True
                g = f64(gama)
                if g.size != m * n:
                    raise ValueError("gama must be a scalar or an m*n vector")
                self._keep.append(g)
                d.gama = dptr(g)
        elif phi is not None:
            ph = f64(phi)
            if ph.size != m * n:
                raise ValueError("phi must have m*n entries")
            self._keep.append(ph)
            d.phi = dptr(ph)
        self.m, self.n = m, n
        self.M = m + n
        self.L = self.M + (1 if self.cls == 2 else 0)
        self.U = m * n + (self.M if self.cls == 2 else 0)
        self.handle = c_void_p()
        return d

    @classmethod
    def from_points(klass, cls, xs, ys, r, l, p, q, metric="sqeuclidean", scale=False, gama=np.inf,
                    mu=0.0, phi=None, ctx=None, matrix_free=False):
        """The workspace of problem class ``cls`` with ``c = point_cost(xs, ys, metric, scale)`` built on
        the device (``ipd_apd_create_points``): (m+n)*d coordinates go up, nothing mn-sized.  ``xs`` is
        (m, d), ``ys`` (n, d), one point per row (1-D for d = 1); class 2 with ``phi=None`` takes
        ``phi`` as all ones.  ``matrix_free=True`` (``ipd_apd_create_points_free``, d <= 3) never stores
        ``c``: the passes recompute an entry from the coordinates, with the bits of the stored one."""
        self = klass.__new__(klass)
        d = self._data(cls, r, l, p, q, gama, mu, phi, ctx)
        spec, keep = _cost_spec(xs, ys, metric, scale)
        if (spec.m, spec.n) != (self.m, self.n):
            raise ValueError(f"from_points: xs, ys must hold {self.m} and {self.n} points")
        create = lib.ipd_apd_create_points_free if matrix_free else lib.ipd_apd_create_points
        check(create((ctx or get_ctx()).handle, byref(d), byref(spec), byref(self.handle)))
        return self

    def cost_info(self) -> dict:
        """How the workspace holds the cost (``ipd_apd_cost_info``): ``form`` 0 stored / 1 matrix-free,
        ``dim, metric, scale`` of the point-cloud specification (0 for a host matrix) and
        ``device_bytes``, what it keeps on the device for the cost."""
        info = L.ipd_cost_info()
        check(lib.ipd_apd_cost_info(self.handle, byref(info)))
        return dict(form=int(info.form), dim=int(info.dim), metric=int(info.metric), scale=int(info.scale),
                    device_bytes=int(info.device_bytes))

    def cost(self, stats: bool = False):
        """``c`` as an (m, n) array, read back from the workspace (``ipd_apd_get_cost``);
        ``stats=True`` -> ``(c, dict(min, max, sum))``, the statistics computed on the device."""
        c = np.empty(self.m * self.n)
        st = L.ipd_cost_stats()
        check(lib.ipd_apd_get_cost(self.handle, dptr(c), byref(st) if stats else None))
        C = c.reshape(self.n, self.m).T
        return (C, _cost_stats(st)) if stats else C

    def close(self):
        if getattr(self, "handle", None):
            lib.ipd_apd_destroy(self.handle)
            self.handle = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- warm start -----------------------------------------------------------
    def warmup(self, res=None, maxit=None):
        """``warmup_class1.m:3-20`` nargin rules: no res -> (1e-1, inf); no maxit -> inf."""
        if res is None:
            res, maxit = 1e-1, np.inf
        elif maxit is None:
            maxit = np.inf
        mi = -1 if np.isinf(maxit) else int(maxit)
        check(lib.ipd_apd_warmup(self.handle, c_double(float(res)), c_int64(mi)))
        u, _, lam, _ = self.state()
        return u, lam

    # -- workspace ------------------------------------------------------------
    def set_state(self, u=None, v=None, lam=None, bk=1.0):
        u_ = f64(u) if u is not None else None
        v_ = f64(v) if v is not None else None
        l_ = f64(lam) if lam is not None else None
        for a, size, name in ((u_, self.U, "u"), (v_, self.U, "v"), (l_, self.L, "lam")):
            if a is not None and a.size != size:
                raise ValueError(f"{name} must have {size} entries")
        check(lib.ipd_apd_set_state(self.handle, dptr(u_) if u_ is not None else None,
                                    dptr(v_) if v_ is not None else None,
                                    dptr(l_) if l_ is not None else None, c_double(float(bk))))

    def state(self):
        u, v, lam = np.empty(self.U), np.empty(self.U), np.empty(self.L)
        bk = c_double()
        check(lib.ipd_apd_get_state(self.handle, dptr(u), dptr(v), dptr(lam), byref(bk)))
        return u, v, lam, bk.value

    # -- the transport plan as a sparse matrix ---------------------------------
    @staticmethod
    def _plan_stats(st: L.ipd_plan_stats) -> dict:
        return dict(nnz=int(st.nnz), sum_kept=st.sum_kept, sum_dropped=st.sum_dropped,
                    max_dropped=st.max_dropped, fval_kept=st.fval_kept)

    def plan(self, tol: float = 0.0, stats: bool = False):
        """``sparse(reshape(xk,m,n))`` restricted to ``~(abs(x) <= tol)`` as a ``csc_matrix``, built on
        the device: only the kept entries cross to the host (``ipd_apd_plan``).  ``tol = 0`` is
        MATLAB's ``sparse()``.  ``stats=True`` -> ``(X, dict(nnz, sum_kept, sum_dropped, max_dropped,
        fval_kept), ax)`` with ``ax = Ax(x_kept, p, q)``."""
        out = L.ipd_csc_out()
        st = L.ipd_plan_stats()
        ax = np.empty(self.M) if stats else None
        check(lib.ipd_apd_plan(self.handle, c_double(float(tol)), byref(out), byref(st),
                               dptr(ax) if stats else None))
        X = L.csc_out_to_scipy(out)
        return (X, self._plan_stats(st), ax) if stats else X

    def plan_dev(self, tol, jc, ir, pr, ax=None) -> dict:
        """The same into caller-owned device arrays (``ipd_apd_plan_dev``): ``jc`` n+1 int64, ``ir``
        int64 and ``pr`` float64 of equal capacity, ``ax`` n+m float64 or None -- torch tensors on
        the workspace's GPU, ``DeviceBuffer`` objects, or raw device pointers given as
        ``(pointer, entries)`` pairs (``jc`` and ``ax``: a plain pointer will do).  Returns the
        statistics; raises ``IpdError`` with code ``IPD_E_LIMIT`` when the capacity is too small
        (the statistics are then in the exception's ``stats`` attribute and ``jc`` is valid)."""
        def ptr_cap(a, itemsize):
            if a is None:
                return None, 0
            if isinstance(a, tuple):
                return c_void_p(int(a[0])), int(a[1])
            if isinstance(a, L.DeviceBuffer):
                return a.ptr, a.nbytes // itemsize
            if hasattr(a, "data_ptr"):
                if a.element_size() != itemsize or not a.is_contiguous():
                    raise ValueError("plan_dev: tensors must be contiguous int64 / float64")
                return c_void_p(a.data_ptr()), a.numel()
            return c_void_p(int(a)), 0
        jc_p, _ = ptr_cap(jc, 8)
        ir_p, ir_cap = ptr_cap(ir, 8)
        pr_p, pr_cap = ptr_cap(pr, 8)
        ax_p, _ = ptr_cap(ax, 8)
        st = L.ipd_plan_stats()
        try:
            check(lib.ipd_apd_plan_dev(self.handle, c_double(float(tol)), c_int64(min(ir_cap, pr_cap)),
                                       jc_p, ir_p, pr_p, byref(st), ax_p))
        except L.IpdError as e:
            e.stats = self._plan_stats(st)
            raise
        return self._plan_stats(st)

    def set_plan(self, X):
        """``xk = vk = full(X)`` from a sparse m x n matrix (``ipd_apd_set_plan``): a warm start or a
        checkpoint of about m+n numbers; ``lk`` and ``bk`` are kept, the iteration count starts over
        as after ``set_state``."""
        if not sp.issparse(X):
            X = sp.csc_matrix(np.asarray(X, dtype=np.float64))
        if X.shape != (self.m, self.n):
            raise ValueError(f"X must be {self.m} x {self.n}")
        A = L.CscIn(X)
        check(lib.ipd_apd_set_plan(self.handle, A.ref()))

    # -- the plan applied on the device ----------------------------------------
    def _apply_dims(self, side):
        if side not in (0, 1):
            raise ValueError("side must be 0 (X @ B) or 1 (X.T @ B)")
        return (self.n, self.m) if side == 0 else (self.m, self.n)

    def apply_plan(self, B, side: int = 0, tol: float = 0.0, normalize: bool = False, mass: bool = False):
        """``Y = X @ B`` (``side=0``, ``B`` (n, k) or 1-D) or ``Y = X.T @ B`` (``side=1``, ``B`` (m, k))
        with ``X = plan(tol)``, computed where the iterate lives (``ipd_apd_plan_apply``): one streaming
        read of ``x`` per four columns of ``B``, k <= 16, and only ``B``, ``Y`` and the mass cross to the
        host.  ``Y`` has shape (m or n, k).  ``mass=True`` -> ``(Y, w)`` with ``w = X @ 1`` (``X.T @ 1``),
        the plain mass of the kept entries.  ``normalize=True`` divides row r of ``Y`` by ``w[r]``; a row
        without kept mass is ``0/0 = nan``.  A dropped entry contributes ``+0.0`` whatever ``B`` holds there.
        On a plan that is already sparse on the host (a converged run, about m+n entries), and when
        ``plan()`` is needed anyway, ``plan(tol) @ B`` is the better route: both take about the time of one
        read of ``x`` and the product itself is trivial (DESIGN.md section 4j has the measured rows)."""
        rin, rout = self._apply_dims(side)
        B_ = np.asarray(B, dtype=np.float64)
        if B_.ndim == 1:
            B_ = B_.reshape(-1, 1)
        if B_.ndim != 2 or B_.shape[0] != rin:
            raise ValueError(f"B must have {rin} rows")
        k = B_.shape[1]
        Bf = np.asfortranarray(B_)
        Y = np.empty((rout, k), order="F")
        w = np.empty(rout) if mass else None
        check(lib.ipd_apd_plan_apply(self.handle, c_double(float(tol)), c_int32(side), c_int32(k),
                                     c_int32(1 if normalize else 0), Bf.ctypes.data, Y.ctypes.data,
                                     w.ctypes.data if mass else None))
        return (Y, w) if mass else Y

    def apply_plan_dev(self, B, Y, w=None, side: int = 0, tol: float = 0.0, normalize: bool = False) -> None:
        """The same on caller-owned device arrays (``ipd_apd_plan_apply_dev``), column-major float64:
        ``B`` (n or m) x k, ``Y`` (m or n) x k, ``w`` m or n entries or None -- torch tensors on the
        workspace's GPU (contiguous, so a (rows, k) matrix is passed as its transpose's storage),
        ``DeviceBuffer`` objects, or ``(pointer, entries)`` pairs.  k is taken from the entries of ``B``."""
        rin, rout = self._apply_dims(side)

        def ptr_count(a, name):
            if isinstance(a, tuple):
                return c_void_p(int(a[0])), int(a[1])
            if isinstance(a, L.DeviceBuffer):
                return a.ptr, a.nbytes // 8
            if hasattr(a, "data_ptr"):
                if a.element_size() != 8 or not a.is_contiguous():
                    raise ValueError("apply_plan_dev: tensors must be contiguous float64")
                return c_void_p(a.data_ptr()), a.numel()
            raise ValueError(f"apply_plan_dev: {name} must be a tensor, a DeviceBuffer or a (pointer, entries) pair")
        B_p, B_cnt = ptr_count(B, "B")
        Y_p, Y_cnt = ptr_count(Y, "Y")
        k, rest = divmod(B_cnt, rin)
        if rest or k < 1:
            raise ValueError(f"apply_plan_dev: B must hold k columns of {rin} entries")
        if Y_cnt < rout * k:
            raise ValueError(f"apply_plan_dev: Y must hold {k} columns of {rout} entries")
        w_p = None
        if w is not None:
            w_p, w_cnt = ptr_count(w, "w")
            if w_cnt < rout:
                raise ValueError(f"apply_plan_dev: w must hold {rout} entries")
        check(lib.ipd_apd_plan_apply_dev(self.handle, c_double(float(tol)), c_int32(side), c_int32(k),
                                         c_int32(1 if normalize else 0), B_p, Y_p, w_p))

    def barycentric_map(self, points, side: int = 0, tol: float = 0.0):
        """The barycentric projection of the plan, ``apply_plan(points, side, tol, normalize=True)``:
        ``side=0`` with ``points = ys`` (n, d) is where each source point is sent,
        ``T(x_i) = sum_j x_ij y_j / sum_j x_ij``; ``side=1`` with ``points = xs`` (m, d) is the reverse."""
        return self.apply_plan(points, side=side, tol=tol, normalize=True)

    # -- the gradient of the transport cost in the point positions ---------------
    @staticmethod
    def _grad_stats(st: L.ipd_grad_stats) -> dict:
        return dict(kept=int(st.kept), kinks=int(st.kinks), denom=st.denom)

    def point_gradient(self, side: int = 0, tol: float = 0.0, points=None, metric=None, scale=None,
                       mass: bool = False, stats: bool = False):
        """The derivative of ``<c(xs, ys), X>`` in the positions of the points at fixed ``X = plan(tol)``, computed where
        the iterate lives (``ipd_apd_point_grad``): ``side=0`` -> (m, d), row i ``sum_j X_ij dc(xs_i, ys_j)/dxs_i``;
        ``side=1`` -> (n, d), row j ``sum_i X_ij dc(xs_i, ys_j)/dys_j``.  By the envelope theorem that is the gradient of
        the transport cost at an optimal (or rounded feasible, ``gap_probe(install=True)``) plan.  ``points=None`` takes
        the clouds, metric and scale the workspace was made from (``from_points``; a workspace from a host matrix has
        none); ``points=(xs, ys)`` with ``metric`` (default ``"sqeuclidean"``) and ``scale`` (default False) may be
        given to any workspace.  Where the cost is not differentiable (coincident points for ``euclidean``, a zero
        coordinate difference for ``cityblock``, a tied or zero maximum for ``chebyshev``) one subgradient is taken:
        0 for the tied coordinates, the first maximum for ``chebyshev``.  ``scale=True`` divides by the largest
        unscaled entry, which is held constant -- a stop-gradient; the divider comes back as ``denom`` so that the
        missing term can be added.  ``mass=True`` adds ``w``, the mass of the kept entries per row (column);
        ``stats=True`` adds ``dict(kept, kinks, denom)``: the kept entries, those at which the cost is not
        differentiable, and the divider (1.0 without scale).  Returns ``G``, or a tuple ``(G[, w][, stats])``.  For
        ``sqeuclidean`` without scale, ``2 * (w[:, None] * xs - apply_plan(ys, mass=True)[0])`` is the same gradient and
        the faster route (DESIGN.md section 4o has the measured rows)."""
        if side not in (0, 1):
            raise ValueError("side must be 0 (xs) or 1 (ys)")
        R = self.n if side else self.m
        spec_ref, keep = None, None
        if points is not None:
            spec, keep = _cost_spec(points[0], points[1], metric or "sqeuclidean", bool(scale))
            if (spec.m, spec.n) != (self.m, self.n):
                raise ValueError(f"point_gradient: xs, ys must hold {self.m} and {self.n} points")
            spec_ref, d = byref(spec), int(spec.dim)
        else:
            if metric is not None or scale is not None:
                raise ValueError("point_gradient: metric and scale go with points=(xs, ys)")
            d = self.cost_info()["dim"]
            if d == 0:
                raise ValueError("point_gradient: the workspace was made from a host matrix; give points=(xs, ys)")
        G = np.empty((R, d), order="F")
        w = np.empty(R) if mass else None
        st = L.ipd_grad_stats()
        check(lib.ipd_apd_point_grad(self.handle, spec_ref, c_double(float(tol)), c_int32(side), G.ctypes.data,
                                     w.ctypes.data if mass else None, byref(st)))
        out = (G,) + ((w,) if mass else ()) + ((self._grad_stats(st),) if stats else ())
        return out if len(out) > 1 else G

    def point_gradient_dev(self, G, w=None, side: int = 0, tol: float = 0.0, xs=None, ys=None, metric=None,
                           scale=None) -> dict:
        """The same on caller-owned device arrays (``ipd_apd_point_grad_dev``), float64: ``G`` (m or n) x d as
        ``G[r + k*R]``, ``w`` m or n entries or None, and -- both or neither -- ``xs`` m x d as ``xs[i + k*m]`` and ``ys``
        n x d: torch tensors on the workspace's GPU (contiguous), ``DeviceBuffer`` objects, or ``(pointer, entries)``
        pairs.  d is taken from the entries of ``xs`` (the workspace's own without it).  Device coordinates are not
        looked at: they must be finite.  Returns the statistics."""
        if side not in (0, 1):
            raise ValueError("side must be 0 (xs) or 1 (ys)")
        R = self.n if side else self.m

        def ptr_count(a, name):
            if isinstance(a, tuple):
                return c_void_p(int(a[0])), int(a[1])
            if isinstance(a, L.DeviceBuffer):
                return a.ptr, a.nbytes // 8
            if hasattr(a, "data_ptr"):
                if a.element_size() != 8 or not a.is_contiguous():
                    raise ValueError("point_gradient_dev: tensors must be contiguous float64")
                return c_void_p(a.data_ptr()), a.numel()
            raise ValueError(f"point_gradient_dev: {name} must be a tensor, a DeviceBuffer or a (pointer, entries) pair")
        if (xs is None) != (ys is None):
            raise ValueError("point_gradient_dev: give both xs and ys, or neither")
        xs_p = ys_p = None
        code = 0
        if xs is not None:
            if metric is not None and metric not in COST_METRICS:
                raise ValueError(f"metric must be one of {sorted(COST_METRICS)}")
            code = COST_METRICS[metric or "sqeuclidean"]
            xs_p, xs_cnt = ptr_count(xs, "xs")
            ys_p, ys_cnt = ptr_count(ys, "ys")
            d, rest = divmod(xs_cnt, self.m)
            if rest or d < 1:
                raise ValueError(f"point_gradient_dev: xs must hold d coordinates of {self.m} points")
            if ys_cnt < self.n * d:
                raise ValueError(f"point_gradient_dev: ys must hold {d} coordinates of {self.n} points")
        else:
            if metric is not None or scale is not None:
                raise ValueError("point_gradient_dev: metric and scale go with xs and ys")
            d = self.cost_info()["dim"]
            if d == 0:
                raise ValueError("point_gradient_dev: the workspace was made from a host matrix; give xs and ys")
        G_p, G_cnt = ptr_count(G, "G")
        if G_cnt < R * d:
            raise ValueError(f"point_gradient_dev: G must hold {d} columns of {R} entries")
        w_p = None
        if w is not None:
            w_p, w_cnt = ptr_count(w, "w")
            if w_cnt < R:
                raise ValueError(f"point_gradient_dev: w must hold {R} entries")
        st = L.ipd_grad_stats()
        check(lib.ipd_apd_point_grad_dev(self.handle, c_int32(code), c_int32(d), c_int32(1 if scale else 0), xs_p, ys_p,
                                         c_double(float(tol)), c_int32(side), G_p, w_p, byref(st)))
        return self._grad_stats(st)

    def transport_gradients(self, tol: float = 0.0) -> dict:
        """``dict(xs=point_gradient(0, tol), ys=point_gradient(1, tol), stats=...)`` in the workspace's own clouds."""
        gx, st = self.point_gradient(0, tol, stats=True)
        gy = self.point_gradient(1, tol)
        return dict(xs=gx, ys=gy, stats=st)

    # -- the dual certificate --------------------------------------------------
    @staticmethod
    def _dual_stats(st: L.ipd_dual_stats) -> dict:
        return dict(dual=st.dual, bterm=st.bterm, cap=st.cap, dmin=st.dmin, imin=int(st.imin), jmin=int(st.jmin),
                    nneg=int(st.nneg), fval=st.fval, gap=st.gap)

    def _dual_side(self, side):
        if side not in (-1, 0, 1):
            raise ValueError("side must be -1 (evaluate), 0 (hold alpha, new beta) or 1 (hold beta, new alpha)")
        return (self.m, self.n)[side] if side >= 0 else 0

    def dual(self, lam=None, side: int = -1, primal: bool = False, arg: bool = False) -> dict:
        """The dual value of a multiplier, computed where the cost lives (``ipd_apd_dual``): ``lam``
        (``[alpha (n); beta (m)(; tau)]``, None: the workspace's ``lk``) as it is (``side=-1``) or after the
        c-transform of one side -- ``side=0`` holds ``alpha`` and takes ``beta_i = max_j (-C_ij - p_i alpha_j)/q_j``,
        ``side=1`` holds ``beta`` (class 2: with ``tau*phi`` and the clamps at 0).  Returns ``dict(dual, bterm, cap,
        dmin, imin, jmin, nneg, fval, gap)``: ``dual = bterm - cap`` with ``bterm = -<b,lam>`` and ``cap`` the
        finite-``gama`` sum, the smallest reduced cost and its first place, the count of negative ones, and with
        ``primal=True`` ``fval = <c,xk>`` and ``gap = fval - dual`` (nan otherwise).  After a transform the dict
        also holds ``lam``, the repaired multiplier, and with ``arg=True`` ``arg``, the winning column of every
        row (``side=0``) or row of every column (``side=1``): the Laguerre-cell assignment.  Nothing mn-sized
        crosses to the host, and the workspace is only read."""
        rows = self._dual_side(side)
        lam_ = self._lam_sized(lam, "lam") if lam is not None else None
        out = np.empty(self.L) if side >= 0 else None
        am = np.empty(rows, np.int32) if side >= 0 and arg else None
        st = L.ipd_dual_stats()
        check(lib.ipd_apd_dual(self.handle, lam_.ctypes.data if lam_ is not None else None, c_int32(side),
                               c_int32(1 if primal else 0), out.ctypes.data if out is not None else None,
                               am.ctypes.data if am is not None else None, byref(st)))
        res = self._dual_stats(st)
        if out is not None:
            res["lam"] = out
        if am is not None:
            res["arg"] = am
        return res

    def dual_dev(self, lam=None, side: int = -1, primal: bool = False, lam_out=None, arg=None) -> dict:
        """The same on caller-owned device arrays (``ipd_apd_dual_dev``): ``lam`` and ``lam_out`` L float64,
        ``arg`` m (``side=0``) or n (``side=1``) int32, each may be None -- torch tensors on the workspace's GPU,
        ``DeviceBuffer`` objects, or ``(pointer, entries)`` pairs, as ``plan_dev`` takes them.  Returns the
        statistics."""
        rows = self._dual_side(side)

        def ptr_of(a, itemsize, need, name):
            if a is None:
                return None
            if isinstance(a, tuple):
                p, cnt = c_void_p(int(a[0])), int(a[1])
            elif isinstance(a, L.DeviceBuffer):
                p, cnt = a.ptr, a.nbytes // itemsize
            elif hasattr(a, "data_ptr"):
                if a.element_size() != itemsize or not a.is_contiguous():
                    raise ValueError("dual_dev: tensors must be contiguous float64 (arg: int32)")
                p, cnt = c_void_p(a.data_ptr()), a.numel()
            else:
                raise ValueError(f"dual_dev: {name} must be a tensor, a DeviceBuffer or a (pointer, entries) pair")
            if cnt < need:
                raise ValueError(f"dual_dev: {name} must hold {need} entries")
            return p
        lam_p = ptr_of(lam, 8, self.L, "lam")
        out_p = ptr_of(lam_out, 8, self.L, "lam_out")
        arg_p = ptr_of(arg, 4, rows, "arg")
        st = L.ipd_dual_stats()
        check(lib.ipd_apd_dual_dev(self.handle, lam_p, c_int32(side), c_int32(1 if primal else 0), out_p, arg_p,
                                   byref(st)))
        return self._dual_stats(st)

    def c_transform(self, lam=None, side: int = 0):
        """The multiplier with one side replaced by its c-transform (``dual(lam, side)["lam"]``): ``side=0`` holds
        ``alpha`` and returns the best feasible ``beta`` for it, ``side=1`` the reverse.  Alternating the two is a
        loop of the caller's."""
        if side not in (0, 1):
            raise ValueError("c_transform: side must be 0 or 1")
        return self.dual(lam, side=side)["lam"]

    def certificate(self) -> dict:
        """The better of the two repaired multipliers of the workspace's ``lk``: ``dual(side=0)`` and
        ``dual(side=1)`` with ``primal=True`` and ``arg=True``, the one with the larger ``dual`` (a certified lower
        bound when ``dmin >= 0``; ``gap`` is then a bound on ``<c,xk> - f*`` for a feasible ``xk``), marked with
        its ``side``.  With finite ``gama`` (class 1) every multiplier is feasible and no transform applies: the
        evaluation of ``lk`` itself, ``side = -1``."""
        if self._finite_gama:
            res = self.dual(side=-1, primal=True)
            res["side"] = -1
            return res
        both = [self.dual(side=s, primal=True, arg=True) for s in (0, 1)]
        side = 1 if both[1]["dual"] > both[0]["dual"] else 0
        res = both[side]
        res["side"] = side
        return res

    # -- the primal certificate ------------------------------------------------
    @staticmethod
    def _round_stats(st: L.ipd_round_stats) -> dict:
        return dict(fval=st.fval, fs=st.fs, cc=st.cc, theta=st.theta, t=st.t, se=st.se, sf=st.sf, ms=st.ms, cp=st.cp,
                    viol_in=st.viol_in, dropped=st.dropped, ndropped=int(st.ndropped), ok=int(st.ok))

    def _round_args(self, tol, side):
        if side not in (0, 1):
            raise ValueError("side must be 0 (rows scaled first) or 1 (columns scaled first)")
        if not tol >= 0:
            raise ValueError("tol must be >= 0")

    def round_plan(self, tol: float = 0.0, side: int = 0, install: bool = False, vectors: bool = True) -> dict:
        """The iterate rounded onto the feasible set, where it lives (``ipd_apd_round``): the entries with
        ``abs(x) <= tol`` and the negative ones dropped, rows and columns scaled down to their marginals (``side=0``:
        rows first), the missing mass put back as a rank-one term -- ``X^ = theta*(rho_i x+_ij kappa_j) + t*e_i f_j``
        -- with its exact cost ``fval = <c, X^>``, a certified upper bound on ``f*`` when ``ok``.  Returns
        ``dict(fval, fs, cc, theta, t, se, sf, ms, cp, viol_in, dropped, ndropped, ok)`` and with ``vectors`` the
        factors ``rho`` (m), ``kappa`` (n), ``e`` (m), ``f`` (n).  ``install=True`` makes ``X^`` the state (class 2:
        with its slacks; ``lk``, ``bk`` and the histories stay) and raises ``IpdError`` (``IPD_E_NUMERIC``) when
        ``ok == 0``.  Nothing mn-sized crosses to the host."""
        self._round_args(tol, side)
        vec = [np.empty(k) for k in (self.m, self.n, self.m, self.n)] if vectors else [None] * 4
        st = L.ipd_round_stats()
        check(lib.ipd_apd_round(self.handle, c_double(tol), c_int32(side), c_int32(1 if install else 0),
                                *[v.ctypes.data if v is not None else None for v in vec], byref(st)))
        res = self._round_stats(st)
        if vectors:
            res.update(rho=vec[0], kappa=vec[1], e=vec[2], f=vec[3])
        return res

    def round_plan_dev(self, tol: float = 0.0, side: int = 0, install: bool = False, rho=None, kappa=None, e=None,
                       f=None, x_out=None) -> dict:
        """The same on caller-owned device arrays (``ipd_apd_round_dev``): ``rho``, ``e`` m float64, ``kappa``,
        ``f`` n, ``x_out`` mn (receives ``X^`` in full, column-major), each may be None -- torch tensors on the
        workspace's GPU, ``DeviceBuffer`` objects, or ``(pointer, entries)`` pairs, as ``dual_dev`` takes them.
        Returns the statistics."""
        self._round_args(tol, side)

        def ptr_of(a, need, name):
            if a is None:
                return None
            if isinstance(a, tuple):
                p, cnt = c_void_p(int(a[0])), int(a[1])
            elif isinstance(a, L.DeviceBuffer):
                p, cnt = a.ptr, a.nbytes // 8
            elif hasattr(a, "data_ptr"):
                if a.element_size() != 8 or not a.is_contiguous():
                    raise ValueError("round_plan_dev: tensors must be contiguous float64")
                p, cnt = c_void_p(a.data_ptr()), a.numel()
            else:
                raise ValueError(f"round_plan_dev: {name} must be a tensor, a DeviceBuffer or a (pointer, entries) "
                                 "pair")
            if cnt < need:
                raise ValueError(f"round_plan_dev: {name} must hold {need} entries")
            return p
        ptrs = [ptr_of(rho, self.m, "rho"), ptr_of(kappa, self.n, "kappa"), ptr_of(e, self.m, "e"),
                ptr_of(f, self.n, "f"), ptr_of(x_out, self.m * self.n, "x_out")]
        st = L.ipd_round_stats()
        check(lib.ipd_apd_round_dev(self.handle, c_double(tol), c_int32(side), c_int32(1 if install else 0), *ptrs,
                                    byref(st)))
        return self._round_stats(st)

    def bracket(self, tol: float = 0.0) -> dict:
        """``lower <= f* <= upper`` with nothing mn-sized crossing to the host: ``lower`` is ``certificate()``,
        ``upper`` the better of ``round_plan(tol, side=0)`` and ``round_plan(tol, side=1)`` (``ok`` first, then the
        smaller ``fval``), marked with its ``side``, and ``gap = upper["fval"] - lower["dual"]``.  The workspace is
        only read.  Not for finite ``gama``."""
        if self._finite_gama:
            raise ValueError("bracket: rounding does not keep x <= gama; finite gama is not supported")
        lower = self.certificate()
        both = [self.round_plan(tol, side=s) for s in (0, 1)]
        side = min((0, 1), key=lambda s: (not both[s]["ok"], both[s]["fval"]))
        upper = both[side]
        upper["side"] = side
        return dict(lower=lower, upper=upper, gap=upper["fval"] - lower["dual"])

    # -- both certificates in one call, and the stopping rule on their gap -------
    def _gap_result(self, br: L.ipd_bracket) -> dict:
        lower, upper = self._dual_stats(br.lower), self._round_stats(br.upper)
        lower["side"], upper["side"] = int(br.lower_side), int(br.upper_side)
        return dict(lower=lower, upper=upper, gap=br.gap)

    def gap_probe(self, tol: float = 0.0, install: bool = False, vectors: bool = False) -> dict:
        """``bracket()`` as one device call (``ipd_apd_bracket``): both c-transforms of ``lk`` in one walk over the
        cost, both repaired multipliers evaluated in one read of ``c`` and ``xk``, the rounding's first pass shared
        by the two sides, one read-back.  Returns ``dict(lower, upper, gap)`` with the bits of ``dual(side,
        primal=True)`` and ``round_plan(tol, side)`` for the sides picked as ``certificate()`` and ``bracket()`` pick
        them (``lower["side"]``, ``upper["side"]``); ``lower["lam"]`` is the repaired multiplier and with
        ``vectors`` ``upper`` holds ``rho``, ``kappa``, ``e``, ``f``.  ``install=True`` makes the rounded plan the
        state as ``round_plan(tol, upper["side"], install=True)`` does and raises ``IpdError`` (``IPD_E_NUMERIC``)
        when ``upper["ok"] == 0``.  Not for finite ``gama`` (``IPD_E_UNSUPPORTED``)."""
        lam = np.empty(self.L)
        vec = [np.empty(k) for k in (self.m, self.n, self.m, self.n)] if vectors else [None] * 4
        br = L.ipd_bracket()
        check(lib.ipd_apd_bracket(self.handle, c_double(tol), c_int32(1 if install else 0), lam.ctypes.data,
                                  *[v.ctypes.data if v is not None else None for v in vec], byref(br)))
        res = self._gap_result(br)
        res["lower"]["lam"] = lam
        if vectors:
            res["upper"].update(rho=vec[0], kappa=vec[1], e=vec[2], f=vec[3])
        return res

    def gap_probe_dev(self, tol: float = 0.0, install: bool = False, lam_out=None, rho=None, kappa=None, e=None,
                      f=None) -> dict:
        """The same on caller-owned device arrays (``ipd_apd_bracket_dev``): ``lam_out`` L float64, ``rho``, ``e`` m,
        ``kappa``, ``f`` n, each may be None -- torch tensors on the workspace's GPU, ``DeviceBuffer`` objects, or
        ``(pointer, entries)`` pairs, as ``round_plan_dev`` takes them.  Returns the statistics."""
        def ptr_of(a, need, name):
            if a is None:
                return None
            if isinstance(a, tuple):
                p, cnt = c_void_p(int(a[0])), int(a[1])
            elif isinstance(a, L.DeviceBuffer):
                p, cnt = a.ptr, a.nbytes // 8
            elif hasattr(a, "data_ptr"):
                if a.element_size() != 8 or not a.is_contiguous():
                    raise ValueError("gap_probe_dev: tensors must be contiguous float64")
                p, cnt = c_void_p(a.data_ptr()), a.numel()
            else:
                raise ValueError(f"gap_probe_dev: {name} must be a tensor, a DeviceBuffer or a (pointer, entries) pair")
            if cnt < need:
                raise ValueError(f"gap_probe_dev: {name} must hold {need} entries")
            return p
        ptrs = [ptr_of(lam_out, self.L, "lam_out"), ptr_of(rho, self.m, "rho"), ptr_of(kappa, self.n, "kappa"),
                ptr_of(e, self.m, "e"), ptr_of(f, self.n, "f")]
        br = L.ipd_bracket()
        check(lib.ipd_apd_bracket_dev(self.handle, c_double(tol), c_int32(1 if install else 0), *ptrs, byref(br)))
        return self._gap_result(br)

    def set_gap_rule(self, gap_tol=0.0, gap_rel: float = 0.0, tol: float = 0.0, first: int = 1, every: int = 1,
                     install: bool = False) -> None:
        """A stopping rule of ``run`` on the certified gap (``ipd_apd_set_gap_rule``): after iteration ``first``,
        ``first + every``, ... and after the one that converges, ``gap_probe(tol)`` runs on the state; the loop
        stops when the better rounded plan is a repair and ``upper - best <= max(gap_tol, gap_rel*|upper|)``, ``best``
        the largest lower bound of the probes so far.  Both thresholds 0: probe and record only.  ``install``: the
        rounded plan becomes the state at the probe that stops.  ``set_gap_rule(None)`` switches the rule off.  A
        stopped workspace runs on only after the rule is set again."""
        if gap_tol is None:
            check(lib.ipd_apd_set_gap_rule(self.handle, None))
            self._gap_rule = False
            return
        r = L.ipd_gap_rule(gap_tol, gap_rel, tol, int(first), int(every), int(install))
        check(lib.ipd_apd_set_gap_rule(self.handle, byref(r)))
        self._gap_rule = True

    def gap_records(self) -> list:
        """One dict per probe of the rule: ``k, lower_side, upper_side, upper_ok, stop, final, lower, lower_dmin,
        best, upper, viol_in, gap`` with ``gap = upper - best``."""
        cnt = c_int64()
        check(lib.ipd_apd_gap_records(self.handle, None, c_int64(0), byref(cnt)))
        arr = (L.ipd_gap_rec * max(cnt.value, 1))()
        check(lib.ipd_apd_gap_records(self.handle, arr, c_int64(cnt.value), byref(cnt)))
        keys = [f[0] for f in L.ipd_gap_rec._fields_]
        return [{k: getattr(arr[i], k) for k in keys} for i in range(cnt.value)]

    def gap_lam(self):
        """``(lam, best)``: the best lower bound of the probes so far and the multiplier that attains it;
        ``(None, -inf)`` before the first probe."""
        lam, best = np.empty(self.L), c_double()
        check(lib.ipd_apd_gap_lam(self.handle, lam.ctypes.data, byref(best)))
        return (lam if best.value > -np.inf else None), best.value

    # -- the rounding's correction ----------------------------------------------
    CORRECTION_MODES = {"rank_one": 0, "north_west": 1, "cheaper": 2}

    def set_correction(self, mode="rank_one", row_order=None, col_order=None) -> None:
        """What carries the rounding's deficits (``ipd_apd_set_correction``): ``"rank_one"``, the dense term
        ``t*e_i*f_j`` (the default, in the bits of a workspace without the setting); ``"north_west"``, a
        north-west-corner coupling along ``row_order`` and ``col_order`` (permutations of ``0..m-1`` and ``0..n-1``,
        None: the identity) with at most ``m + n - 1`` entries and no walk over the cost; ``"cheaper"``, both, and the
        device keeps the one with ``ok`` first, then the smaller ``fval``.  ``round_plan``, ``round_plan_dev``,
        ``bracket``, ``gap_probe``, ``gap_probe_dev`` and the gap rule's probes obey it."""
        if mode not in self.CORRECTION_MODES:
            raise ValueError("set_correction: mode must be one of %s" % sorted(self.CORRECTION_MODES))
        orders = []
        for a, need, name in ((row_order, self.m, "row_order"), (col_order, self.n, "col_order")):
            if a is not None:
                a = np.ascontiguousarray(a)
                if a.ndim != 1 or a.size != need or not np.issubdtype(a.dtype, np.integer):
                    raise ValueError(f"set_correction: {name} must hold {need} integers")
                # (what does not fit int32 stays outside 0..need-1: the library refuses it)
                a = np.clip(a.astype(np.int64), -1, 2 ** 31 - 1).astype(np.int32)
            orders.append(a)
        check(lib.ipd_apd_set_correction(self.handle, c_int32(self.CORRECTION_MODES[mode]),
                                         *[a.ctypes.data if a is not None else None for a in orders]))

    def correction_info(self) -> dict:
        """Of the last rounding or bracket call (``ipd_apd_correction_info``): ``mode`` of that call, ``form`` it used
        (0 rank-one, 1 north-west), ``count`` of its list and, under ``"cheaper"``, ``cc`` and ``fval`` of both forms
        (``[0]`` rank-one, ``[1]`` north-west; NaN otherwise)."""
        out = L.ipd_correction_info()
        check(lib.ipd_apd_correction_info(self.handle, byref(out)))
        return dict(mode=int(out.mode), form=int(out.form), count=int(out.count), cc=tuple(out.cc),
                    fval=tuple(out.fval))

    def correction_entries(self):
        """``(i, j, g)`` of the last rounding or bracket call's list (``ipd_apd_correction_entries``), in ascending
        order along the two orders: ``X^ = theta*X2`` plus ``t*g`` at ``(i, j)``.  Empty when that call used the
        rank-one term."""
        cnt = c_int64()
        check(lib.ipd_apd_correction_entries(self.handle, None, None, None, c_int64(0), byref(cnt)))
        i, j, g = np.empty(cnt.value, np.int32), np.empty(cnt.value, np.int32), np.empty(cnt.value)
        if cnt.value:
            check(lib.ipd_apd_correction_entries(self.handle, i.ctypes.data, j.ctypes.data, g.ctypes.data,
                                                 c_int64(cnt.value), byref(cnt)))
        return i, j, g

    # -- the loop -------------------------------------------------------------
    def options(self, **kw) -> L.ipd_apd_opts:
        o = L.ipd_apd_opts()
        lib.ipd_apd_opts_init(c_int32(self.cls), byref(o))
        for key, val in kw.items():
            setattr(o, key, val)
        return o

    def run(self, amg_options: dict, rng: MatlabRand | None = None, iters: int | None = None,
            krylov: bool = False, **opts) -> dict:
        """``krylov=True``: ``inner_solver = 4`` runs AMG-preconditioned CG behind ``Hybrid_AMG`` /
        ``AMG4POT`` (``ipd_apd_set_krylov``); the AMG counters then count PCG iterations."""
        o = self.options(**opts)
        ao = _opts_struct(amg_options)
        rng = rng or MatlabRand()
        res = L.ipd_apd_result()
        check(lib.ipd_apd_set_krylov(self.handle, c_int32(1 if krylov else 0)))
        check(lib.ipd_apd_run(self.handle, byref(o), byref(ao), rng.handle,
                              c_int32(o.maxit if iters is None else int(iters)), byref(res)))
        out = dict(converged=bool(res.converged), k=res.k, fval=res.fval, kkt=list(res.kkt),
                   rr=res.rr, SumAMG=res.sum_amg, TotalAMG=res.total_amg, FailAMG=res.fail_amg,
                   MaxAMG=res.max_amg, restarts=res.restarts, nrec=res.nrec)
        if self._gap_rule:
            recs = self.gap_records()
            out["gap"] = recs[-1] if recs else None
            out["gap_stop"] = bool(recs and recs[-1]["stop"])
        return out

    def history(self) -> dict:
        names = ["fxk", "KKT_xk", "KKT_lk", "KKT_yk", "KKT_zk", "SsN_itnum"]
        out = {}
        for which, name in enumerate(names):
            if self.cls == 1 and name in ("KKT_yk", "KKT_zk"):
                continue
            cnt = c_int64()
            check(lib.ipd_apd_history(self.handle, c_int32(which), None, c_int64(0), byref(cnt)))
            buf = np.empty(max(cnt.value, 1))
            check(lib.ipd_apd_history(self.handle, c_int32(which), dptr(buf), c_int64(cnt.value),
                                      byref(cnt)))
            out[name] = buf[:cnt.value].copy()
        return out

    def records(self) -> list:
        cnt = c_int64()
        check(lib.ipd_apd_records(self.handle, None, c_int64(0), byref(cnt)))
        arr = (L.ipd_ssn_rec * max(cnt.value, 1))()
        check(lib.ipd_apd_records(self.handle, arr, c_int64(cnt.value), byref(cnt)))
        keys = [f[0] for f in L.ipd_ssn_rec._fields_]
        return [{k: getattr(arr[i], k) for k in keys} for i in range(cnt.value)]

    def reuse_stats(self):
        """Row f3: (Newton steps solved with AMG, steps whose system repeated the previous one,
        setups that shared the previous step's levels 1-2)."""
        a, b, c = c_int64(0), c_int64(0), c_int64(0)
        check(lib.ipd_apd_reuse_stats(self.handle, byref(a), byref(b), byref(c)))
        return a.value, b.value, c.value

    # -- building blocks ------------------------------------------------------
    def begin(self, k: int):
        vals = (c_double * 3)()
        check(lib.ipd_apd_begin(self.handle, c_int32(int(k)), vals))
        return dict(bk1=vals[0], tk=vals[1], ak=vals[2])

    def eval(self, lam):
        lam = f64(lam)
        if lam.size != self.L:
            raise ValueError(f"lam must have {self.L} entries")
        s = np.empty(self.m * self.n, np.uint8)
        t = np.empty(self.M)
        F = np.empty(self.L)
        vals = (c_double * 6)()
        check(lib.ipd_apd_eval(self.handle, dptr(lam), bptr(s), dptr(t) if self.cls == 2 else None,
                               dptr(F), vals))
        return dict(s=s.astype(bool), t=(t != 0) if self.cls == 2 else None, Fk=F, bk1=vals[0],
                    tk=vals[1], ak=vals[2], Fk_norm=vals[3], cFk=vals[4], E=int(vals[5]))

    def _lam_sized(self, a, name):
        a = f64(a)
        if a.size != self.L:
            raise ValueError(f"{name} must have {self.L} entries")
        return a

    def get_w(self):
        """``(wk, wlk)`` as ``begin`` left them (``ipd_apd_get_w``)."""
        w, wlk = np.empty(self.U), np.empty(self.L)
        check(lib.ipd_apd_get_w(self.handle, w.ctypes.data, wlk.ctypes.data))
        return w, wlk

    def eval_trial(self, lam, zeta=None, step=0.0, Fk_old=None, merit3=False):
        """``eval`` at the line search's trial point ``lam + step*zeta`` (``ipd_apd_eval_trial``):
        what ``eval`` returns plus ``lam_out``, ``fold_zeta = Fk_old'*zeta``, the prob-3 sums
        ``z2``, ``zmp2`` (``merit3=True``: ``cFk`` is that merit) and the raw sums ``lam2``,
        ``wlk_lam``, ``prox2``."""
        lam = self._lam_sized(lam, "lam")
        zeta = self._lam_sized(zeta, "zeta") if zeta is not None else None
        Fo = self._lam_sized(Fk_old, "Fk_old") if Fk_old is not None else None
        s = np.empty(self.m * self.n, np.uint8)
        t, F, lo = np.empty(self.M), np.empty(self.L), np.empty(self.L)
        vals = np.empty(12)
        check(lib.ipd_apd_eval_trial(self.handle, lam.ctypes.data, zeta.ctypes.data if zeta is not None else None,
                                     c_double(float(step)), Fo.ctypes.data if Fo is not None else None,
                                     c_int32(1 if merit3 else 0), s.ctypes.data,
                                     t.ctypes.data if self.cls == 2 else None, F.ctypes.data, lo.ctypes.data,
                                     vals.ctypes.data))
        return dict(s=s.astype(bool), t=(t != 0) if self.cls == 2 else None, Fk=F, lam_out=lo, bk1=vals[0],
                    tk=vals[1], ak=vals[2], Fk_norm=vals[3], cFk=vals[4], E=int(vals[5]), z2=vals[6],
                    zmp2=vals[7], fold_zeta=vals[8], lam2=vals[9], wlk_lam=vals[10], prox2=vals[11])

    def merit(self, lam, zeta, steps):
        """The merit ``cFk`` at ``lam + steps[k]*zeta`` for the 8 trial steps of one line-search pass
        (``ipd_apd_merit``)."""
        lam, zeta, steps = self._lam_sized(lam, "lam"), self._lam_sized(zeta, "zeta"), f64(steps)
        if steps.size != 8:
            raise ValueError("steps must have 8 entries")
        out = np.empty(8)
        check(lib.ipd_apd_merit(self.handle, lam.ctypes.data, zeta.ctypes.data, steps.ctypes.data, out.ctypes.data))
        return out

    def end(self, lam, from_w=True, u=None):
        """``from_w=True``: ``uk1 = prox(zk)``, ``vk1`` at the multiplier ``lam`` become the state
        (with ``lam``); ``from_w=False``: measures the iterate ``u`` (None: the state's).  Returns
        ``dict(kkt=[KKT_xk, KKT_lk, KKT_yk, KKT_zk], fx=c'*x)`` (``ipd_apd_end``)."""
        lam = self._lam_sized(lam, "lam")
        u_ = f64(u) if u is not None else None
        if u_ is not None and u_.size != self.U:
            raise ValueError(f"u must have {self.U} entries")
        kkt = np.empty(4)
        fx = c_double()
        check(lib.ipd_apd_end(self.handle, c_int32(1 if from_w else 0), lam.ctypes.data,
                              u_.ctypes.data if u_ is not None else None, kkt.ctypes.data, byref(fx)))
        return dict(kkt=kkt, fx=fx.value)

    def bench_eval(self, reps: int = 100):
        ms, by = c_double(), c_double()
        check(lib.ipd_apd_bench_eval(self.handle, c_int32(int(reps)), byref(ms), byref(by)))
        return ms.value, by.value


def warmup_class1(c, r, l, p, q, gama, res=None, maxit=None):
    """``[xk,lk] = warmup_class1(c,r,l,p,q,gama,res,maxit)`` (``Class1/warmup_class1.m:2``)."""
    if res is not None and maxit is not None and res == 0 and np.isinf(maxit):
        raise ValueError("res = 0 and maxit = inf")
    ws = APDWorkspace(1, c, r, l, p, q, gama=gama)
    try:
        return ws.warmup(res, maxit)
    finally:
        ws.close()


def warmup_class2(c, r, l, p, q, mu, phi, res=None, maxit=None):
    """``[uk,lk] = warmup_class2(c,r,l,p,q,mu,phi,res,maxit)`` (``Class2/warmup_class2.m:1``)."""
    if res is not None and maxit is not None and res == 0 and np.isinf(maxit):
        raise ValueError("res = 0 and maxit = inf")
    ws = APDWorkspace(2, c, r, l, p, q, mu=mu, phi=phi)
    try:
        return ws.warmup(res, maxit)
    finally:
        ws.close()


def _run_script(ws: APDWorkspace, amg_opts: dict, rng, warm, opts, krylov: bool = False,
                plan_tol=None, certificate: bool = False, bracket: bool = False, gap: dict | None = None,
                correction: dict | None = None, gradient=None) -> dict:
    try:
        if correction is not None:
            ws.set_correction(**correction)
        if bracket and ws._finite_gama:     # before the run, not after it
            raise ValueError("bracket: rounding does not keep x <= gama; finite gama is not supported")
        if warm is not None:
            ws.warmup(*warm)
        if gap is not None:
            ws.set_gap_rule(**gap)
        out = ws.run(amg_opts, rng, krylov=krylov, **opts)
        if gap is not None:
            out["gap_records"] = ws.gap_records()
        u, v, lam, bk = ws.state()
        out.update(ws.history())
        out.update(uk=u, vk=v, lk=lam, bk=bk, records=ws.records(), reuse_stats=ws.reuse_stats())
        out["xk"] = u[:ws.m * ws.n]
        if plan_tol is not None:
            out["plan"], out["plan_stats"], out["plan_ax"] = ws.plan(plan_tol, stats=True)
        if certificate:
            out["certificate"] = ws.certificate()
        if bracket:
            out["bracket"] = ws.bracket()
        if correction is not None and (bracket or gap is not None):
            out["correction"] = ws.correction_info()   # of the last rounding: the bracket's, else the last probe's
        if gradient is not None:    # after bracket / gap_install: an installed plan is the one differentiated
            g = ws.transport_gradients(gradient)
            out.update(grad_xs=g["xs"], grad_ys=g["ys"], grad_stats=g["stats"])
        return out
    finally:
        ws.close()


def _gap_keywords(gap_tol, gap_rel, gap_every, gap_first, gap_install):
    """the drivers' ``gap_*`` keywords as ``set_gap_rule``'s; None when none of them was given"""
    if gap_tol is None and gap_rel is None and gap_every is None and gap_first is None and not gap_install:
        return None
    return dict(gap_tol=gap_tol or 0.0, gap_rel=gap_rel or 0.0, first=1 if gap_first is None else gap_first,
                every=1 if gap_every is None else gap_every, install=bool(gap_install))


def projection_order(xs, ys):
    """``(row_order, col_order)`` for ``set_correction``: the stable argsorts of the two clouds (``xs`` m x d, ``ys``
    n x d) projected on the first principal axis of their union.  numpy, on the host, run once."""
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    xs = xs[:, None] if xs.ndim == 1 else xs
    ys = ys[:, None] if ys.ndim == 1 else ys
    if xs.ndim != 2 or ys.ndim != 2 or xs.shape[1] != ys.shape[1]:
        raise ValueError("projection_order: xs must be (m, d) and ys (n, d), one point per row")
    both = np.concatenate([xs, ys])
    centred = both - both.mean(axis=0)
    axis = np.linalg.svd(centred, full_matrices=False)[2][0]
    lead = np.argmax(np.abs(axis))
    if axis[lead] < 0:    # the sign of a singular vector is arbitrary: its largest component positive
        axis = -axis
    t = centred @ axis
    return (np.argsort(t[:len(xs)], kind="stable").astype(np.int32),
            np.argsort(t[len(xs):], kind="stable").astype(np.int32))


def _correction_keywords(correction, correction_order, points=None):
    """the drivers' ``correction`` and ``correction_order`` keywords as ``set_correction``'s; None when neither was
    given.  ``points``: the two clouds of a ``_points`` driver, which allow ``correction_order="projection"``."""
    if correction is None and correction_order is None:
        return None
    if isinstance(correction_order, str):
        if correction_order != "projection" or points is None:
            raise ValueError('correction_order must be None, (row_order, col_order) or, in the drivers that take '
                             'point clouds, "projection"')
        correction_order = projection_order(*points)
    row, col = correction_order if correction_order is not None else (None, None)
    return dict(mode=correction if correction is not None else "rank_one", row_order=row, col_order=col)


def APD_SsN_Class1(c, r, l, p, q, gama=np.inf, prob=2, rng: MatlabRand | None = None,
                   amg_opts: dict | None = None, krylov: bool = False, plan_tol=None, certificate: bool = False,
                   bracket: bool = False, gap_tol=None, gap_rel=None, gap_every=None, gap_first=None,
                   gap_install=False, correction=None, correction_order=None, **opts) -> dict:
    """The script ``Class1/APD_SsN_Class1.m`` with ``inner_solver = 4`` on the workspace it
    loads (``:27``); returns the variables it leaves behind.  Warm start as ``:53-59``.
    ``krylov``: see ``APDWorkspace.run``.  ``plan_tol``: when given, the result gains ``plan`` (the
    final ``xk`` as a sparse m x n matrix without the entries with ``abs(x) <= plan_tol``),
    ``plan_stats`` and ``plan_ax`` (``APDWorkspace.plan``).  ``certificate=True``: the result gains
    ``certificate``, the dual certificate of the final ``lk`` (``APDWorkspace.certificate``: the better c-transform
    with its dual value, smallest reduced cost and duality gap; with finite ``gama`` the evaluation of ``lk``).
    ``bracket=True``: the result gains ``bracket`` (``APDWorkspace.bracket``: that certificate as ``lower``, the final
    ``xk`` rounded to a feasible plan with its exact cost as ``upper``, and their ``gap``; not with finite ``gama``).
    ``gap_tol``, ``gap_rel``, ``gap_every``, ``gap_first``, ``gap_install``: any of them sets the stopping rule on the
    certified gap (``APDWorkspace.set_gap_rule``; the rounding's ``tol`` is 0) before the run; the result gains
    ``gap_records``, ``gap_stop`` and ``gap``.  ``correction`` (``"rank_one"``, ``"north_west"``, ``"cheaper"``) and
    ``correction_order`` (``(row_order, col_order)``; in the drivers that take point clouds also ``"projection"``,
    ``projection_order`` of the clouds): ``APDWorkspace.set_correction`` before the run, obeyed by ``bracket`` and the
    gap rule; the result then gains ``correction`` (``APDWorkspace.correction_info``).  Without them every result
    keeps its bits."""
    amg_opts = amg_opts or dict(retol=1e-11, bigph=1, maxit=30, theta=1 / 4, smoth=5, cycle="w",
                                isnsp=1, inter=1, guess=None)                          # :87-88
    warm = (0.0, 100) if prob > 0 else (5e-2, np.inf)                                  # :53-58
    ws = APDWorkspace(1, c, r, l, p, q, gama=gama)
    return _run_script(ws, amg_opts, rng, warm, dict(prob=int(prob), **opts), krylov, plan_tol, certificate,
                       bracket, gap=_gap_keywords(gap_tol, gap_rel, gap_every, gap_first, gap_install),
                       correction=_correction_keywords(correction, correction_order))


def APD_SsN_Class2(c, r, l, p, q, mu, phi, rng: MatlabRand | None = None,
                   amg_opts: dict | None = None, krylov: bool = False, plan_tol=None, certificate: bool = False,
                   bracket: bool = False, gap_tol=None, gap_rel=None, gap_every=None, gap_first=None,
                   gap_install=False, correction=None, correction_order=None, **opts) -> dict:
    """The script ``Class2/APD_SsN_Class2.m`` with ``inner_solver = 4`` (AMG4POT 'amg', or
    'amg_pcg' with ``krylov``).  ``plan_tol``, ``certificate``, ``bracket`` and the ``gap_*`` keywords: as in
    ``APD_SsN_Class1``."""
    amg_opts = amg_opts or dict(retol=1e-11, bigph=1, maxit=40, theta=1 / 4, smoth=10, cycle="w",
                                isnsp=1, inter=1, guess=None)
    ws = APDWorkspace(2, c, r, l, p, q, mu=mu, phi=phi)
    return _run_script(ws, amg_opts, rng, (0.0, 100), opts, krylov, plan_tol, certificate, bracket,
                       gap=_gap_keywords(gap_tol, gap_rel, gap_every, gap_first, gap_install),
                       correction=_correction_keywords(correction, correction_order))


# ---------------------------------------------------------------------------
# the cost out of point clouds
# ---------------------------------------------------------------------------
COST_METRICS = {"sqeuclidean": 1, "euclidean": 2, "cityblock": 3, "chebyshev": 4}


def _cost_stats(st: L.ipd_cost_stats) -> dict:
    return dict(min=st.min, max=st.max, sum=st.sum)


def _cost_spec(xs, ys, metric, scale):
    """``ipd_cost_spec`` of (m, d) / (n, d) point arrays (1-D: d = 1), made coordinate-major, and the
    arrays it points to."""
    if metric not in COST_METRICS:
        raise ValueError(f"metric must be one of {sorted(COST_METRICS)}")
    X, Y = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    X = X[:, None] if X.ndim == 1 else X
    Y = Y[:, None] if Y.ndim == 1 else Y
    if X.ndim != 2 or Y.ndim != 2 or X.shape[1] != Y.shape[1]:
        raise ValueError("xs must be (m, d) and ys (n, d), one point per row")
    keep = [np.ascontiguousarray(X.T).reshape(-1), np.ascontiguousarray(Y.T).reshape(-1)]
    spec = L.ipd_cost_spec()
    spec.metric, spec.dim = COST_METRICS[metric], X.shape[1]
    spec.m, spec.n = X.shape[0], Y.shape[0]
    spec.xs, spec.ys = dptr(keep[0]), dptr(keep[1])
    spec.scale = 1 if scale else 0
    return spec, keep


def point_cost(xs, ys, metric="sqeuclidean", scale=False, stats=False, ctx=None):
    """The (m, n) cost matrix of two point clouds, computed on the device (``ipd_cost_points_dev``):
    ``metric`` in ``sqeuclidean, euclidean, cityblock, chebyshev``; ``scale`` divides by the largest
    entry.  ``stats=True`` -> ``(c, dict(min, max, sum))``."""
    spec, keep = _cost_spec(xs, ys, metric, scale)
    ctx = ctx or get_ctx()
    m, n = int(spec.m), int(spec.n)
    buf = L.DeviceBuffer(8 * max(m * n, 1), ctx)
    try:
        st = L.ipd_cost_stats()
        check(lib.ipd_cost_points_dev(ctx.handle, byref(spec), buf.ptr, byref(st)))
        C = buf.to_array(np.float64, m * n).reshape(n, m).T
    finally:
        buf.free()
    return (C, _cost_stats(st)) if stats else C


def APD_SsN_Class1_points(xs, ys, r, l, p, q, metric="sqeuclidean", scale=False, gama=np.inf, prob=2,
                          rng: MatlabRand | None = None, amg_opts: dict | None = None, krylov: bool = False,
                          plan_tol=None, matrix_free=False, certificate: bool = False, bracket: bool = False,
                          gap_tol=None, gap_rel=None, gap_every=None, gap_first=None, gap_install=False,
                          correction=None, correction_order=None, gradient=None, **opts) -> dict:
    """``APD_SsN_Class1`` with ``c = point_cost(xs, ys, metric, scale)`` built on the device
    (``matrix_free=True``: never stored, see ``APDWorkspace.from_points``); ``certificate``, ``bracket`` and the
    ``gap_*`` keywords: as there.  ``gradient=tol``: the result gains ``grad_xs`` (m, d), ``grad_ys`` (n, d) and
    ``grad_stats``, the derivative of the transport cost in the positions of the points at the final plan without its
    entries ``abs(x) <= tol`` (``APDWorkspace.transport_gradients``; with ``gap_install`` the installed feasible plan).
    Without the keyword every result keeps its bits."""
    amg_opts = amg_opts or dict(retol=1e-11, bigph=1, maxit=30, theta=1 / 4, smoth=5, cycle="w",
                                isnsp=1, inter=1, guess=None)
    warm = (0.0, 100) if prob > 0 else (5e-2, np.inf)
    ws = APDWorkspace.from_points(1, xs, ys, r, l, p, q, metric=metric, scale=scale, gama=gama,
                                  matrix_free=matrix_free)
    return _run_script(ws, amg_opts, rng, warm, dict(prob=int(prob), **opts), krylov, plan_tol, certificate,
                       bracket, gap=_gap_keywords(gap_tol, gap_rel, gap_every, gap_first, gap_install),
                       correction=_correction_keywords(correction, correction_order, (xs, ys)), gradient=gradient)


def APD_SsN_Class2_points(xs, ys, r, l, p, q, mu, phi=None, metric="sqeuclidean", scale=False,
                          rng: MatlabRand | None = None, amg_opts: dict | None = None, krylov: bool = False,
                          plan_tol=None, matrix_free=False, certificate: bool = False, bracket: bool = False,
                          gap_tol=None, gap_rel=None, gap_every=None, gap_first=None, gap_install=False,
                          correction=None, correction_order=None, gradient=None, **opts) -> dict:
    """``APD_SsN_Class2`` with the cost built on the device; ``phi=None`` is all ones
    (``matrix_free=True``: never stored, see ``APDWorkspace.from_points``); ``certificate``, ``bracket`` and the
    ``gap_*`` keywords: as in ``APD_SsN_Class1``; ``gradient``: as in ``APD_SsN_Class1_points``."""
    amg_opts = amg_opts or dict(retol=1e-11, bigph=1, maxit=40, theta=1 / 4, smoth=10, cycle="w",
                                isnsp=1, inter=1, guess=None)
    ws = APDWorkspace.from_points(2, xs, ys, r, l, p, q, metric=metric, scale=scale, mu=mu, phi=phi,
                                  matrix_free=matrix_free)
    return _run_script(ws, amg_opts, rng, (0.0, 100), opts, krylov, plan_tol, certificate, bracket,
                       gap=_gap_keywords(gap_tol, gap_rel, gap_every, gap_first, gap_install),
                       correction=_correction_keywords(correction, correction_order, (xs, ys)), gradient=gradient)


def load_input(path: str) -> dict:
    """``load('./InputData/data1-*.mat')`` / ``data4-*.mat`` (``APD_SsN_Class1.m:27``,
    ``APD_SsN_Class2.m``): the reference's MAT-v5 workspaces as float64 arrays.

    The bundled files store ``p``, ``q`` (and ``phi``) as ``uint8`` and ``m``, ``n`` as ``uint16``;
    MATLAB promotes them silently in mixed arithmetic, here they are cast once (SURVEY A-12).
    Returns ``dict(cls, m, n, c, r, l, p, q, gama)`` for Class 1 and
    ``dict(cls, m, n, c, r, l, p, q, mu, phi)`` for Class 2 (``c = C(:)``, column-major)."""
    import scipy.io
    d = scipy.io.loadmat(path)
    vec = lambda k: np.asarray(d[k], dtype=np.float64).reshape(-1, order="F")
    out = dict(r=vec("r"), l=vec("l"), p=vec("p"), q=vec("q"))
    out["m"], out["n"] = out["l"].size, out["r"].size
    if "mu" in d:                                           # Class 2
        out["cls"] = 2
        out["c"] = vec("c") if "c" in d else vec("C")
        out["mu"] = float(np.asarray(d["mu"]).reshape(-1)[0])
        out["phi"] = vec("phi")
    else:
        out["cls"] = 1
        out["c"] = vec("c")
        g = vec("gama")
        out["gama"] = float(g[0]) if g.size == 1 or np.all(g == g[0]) else g
    if out["c"].size != out["m"] * out["n"]:
        raise ValueError("load_input: length(c) != m*n")
    return out
