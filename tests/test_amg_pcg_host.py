"""AMG-preconditioned CG without a GPU: the entry points exist through the C ABI, Python and the MEX
gateway, and the numpy restatement the GPU tests compare against (tests/amg_pcg_ref.py) is PCG.m's
loop."""
import ctypes
import os
import re

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import ipd_oracle as O
from tests import amg_pcg_ref as R
from tests import problems as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ipd_amg_pcg", "ipd_amg_pcg_dev")


def test_header_declares_both_entry_points():
    txt = open(os.path.join(ROOT, "include", "ipd_amg.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*ipd_amg\s*\*" % name, txt), name


def test_library_exports_both_entry_points():
    import __graft_entry__ as g
    g.build()
    from codes_of_ipd_ssn_amg_method_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name


def test_python_api():
    import codes_of_ipd_ssn_amg_method_amd as ipd
    assert callable(getattr(ipd.AMGHierarchy, "pcg", None))
    assert callable(ipd.AMG_PCG) and "AMG_PCG" in ipd.__all__


def test_mex_gateway_and_shim():
    mex = os.path.join(ROOT, "codes_of_ipd_ssn_amg_method_amd", "mex")
    assert '"AMG_PCG"' in open(os.path.join(mex, "ipd_mex.cpp")).read()
    shim = open(os.path.join(mex, "AMG_PCG.m")).read()
    assert "function [d,it,res,resk] = AMG_PCG(varargin)" in shim and "ipd_mex('AMG_PCG'" in shim


def test_restatement_exact_preconditioner_stops_after_one_iteration():
    A = PR.random_sym_graph_laplacian(150, seed=4, eps=0.5).tocsc()
    e = np.random.RandomState(1).randn(150)
    lu = spla.splu(A)
    d, it, res, resk = R.amg_pcg(A, e, lu.solve, retol=1e-11, maxit=50)
    assert it == 1 and res <= 1e-11 and resk.size == 1
    assert np.linalg.norm(A @ d - e) <= 1e-11 * np.linalg.norm(e)


def test_restatement_is_pcg_for_a_symmetric_linear_preconditioner():
    """Jacobi: flexible and Fletcher-Reeves beta agree, so the iterates are O.PCG's (precd = 2)."""
    A = PR.random_sym_graph_laplacian(300, seed=10, eps=0.5)
    e = np.random.RandomState(11).randn(300)
    g = 0.1 * np.random.RandomState(3).randn(300)
    dg = A.diagonal()
    for maxit in (1, 2, 5, 1000):
        d, it, res, resk = R.amg_pcg(A, e, lambda r: r / dg, retol=1e-11, maxit=maxit, guess=g)
        do, ito, reso, resko = O.PCG(A, e, dict(guess=g, retol=1e-11, maxit=maxit, precd=2))
        assert it == ito
        assert np.linalg.norm(d - do) <= 1e-12 * np.linalg.norm(do)
        assert abs(res - reso) <= 1e-12 * max(reso, 1e-300) or abs(res - reso) <= 1e-14
        assert np.allclose(resk, resko, rtol=1e-9, atol=0)


def test_restatement_zero_right_hand_side():
    A = sp.csr_matrix(PR.random_sym_graph_laplacian(50, seed=2, eps=0.5))
    d, it, res, resk = R.amg_pcg(A, np.zeros(50), lambda r: r / A.diagonal())
    assert it == 0 and np.isnan(res) and not d.any()
