"""The one-launch AMG-PCG and its callers without a GPU: the entry points exist through the C ABI,
Python and the MEX gateway."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ipd_amg_pcg_planned", "ipd_amg_pcg_planned_dev", "ipd_amg_pcg_mode", "ipd_hybrid_amg_pcg",
         "ipd_hybrid_amg_pcg_dev", "ipd_amg4pot_pcg", "ipd_apd_set_krylov")


def test_header_declares_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "ipd_amg.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name


def test_library_exports_the_entry_points():
    import __graft_entry__ as g
    g.build()
    from codes_of_ipd_ssn_amg_method_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name


def test_python_api():
    import codes_of_ipd_ssn_amg_method_amd as ipd
    assert "planned" in inspect.signature(ipd.AMGHierarchy.pcg).parameters
    assert "planned" in inspect.signature(ipd.AMG_PCG).parameters
    assert isinstance(ipd.AMGHierarchy.pcg_mode, property)
    assert callable(ipd.Hybrid_AMG_PCG) and "Hybrid_AMG_PCG" in ipd.__all__
    for fn in (ipd.APDWorkspace.run, ipd.APD_SsN_Class1, ipd.APD_SsN_Class2):
        assert inspect.signature(fn).parameters["krylov"].default is False


def test_mex_gateway_and_shims():
    mex = os.path.join(ROOT, "codes_of_ipd_ssn_amg_method_amd", "mex")
    cpp = open(os.path.join(mex, "ipd_mex.cpp")).read()
    for cmd in ('"Hybrid_AMG_PCG"', '"AMG4POT_pcg"', '"apd_krylov"', "ipd_amg_pcg_planned"):
        assert cmd in cpp, cmd
    assert "ipd_mex('Hybrid_AMG_PCG'" in open(os.path.join(mex, "Hybrid_AMG_PCG.m")).read()
    assert "ipd_mex('AMG4POT_pcg'" in open(os.path.join(mex, "AMG4POT.m")).read()
