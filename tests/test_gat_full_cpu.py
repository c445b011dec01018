"""GAT over the whole graph, the parts that need no GPU: the two entry points in
the header, the library and the bindings, their argument checks, and the ABI
version they leave alone."""
import ctypes
import re
import subprocess

from conftest import ROOT

SYMBOLS = {"nts_hip_gat_scores": 8, "nts_hip_gat_graph_fwd": 12}


def test_header_declares_both_entry_points():
    text = (ROOT / "include" / "nts_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, nargs in SYMBOLS.items():
        found = re.findall(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert len(found) == 1, name
        assert len(found[0].split(",")) == nargs, name


def test_library_exports_them_and_the_abi_is_still_11():
    from nts import _abi
    lib = _abi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (nts_hip_\w+)", out))
    assert set(SYMBOLS) <= exported
    assert lib.nts_hip_abi_version() == _abi.ABI_VERSION == 11


def test_bindings_carry_them_with_the_right_argument_counts():
    from nts import _abi
    from nts.hip import HipContext
    lib = _abi.lib()
    for name, nargs in SYMBOLS.items():
        assert name in _abi.EXPORTED
        fn = getattr(lib, name)
        assert len(fn.argtypes) == nargs and fn.restype is ctypes.c_int
    assert callable(HipContext.gat_scores) and callable(HipContext.gat_graph_fwd)


def test_bad_arguments_are_rejected_without_a_gpu():
    from nts import _abi
    lib = _abi.lib()
    g = _abi.GraphDev(10, 0, None, None, None, None)
    for heads, D in ((0, 4), (4, 0)):
        assert lib.nts_hip_gat_scores(None, None, 0, 0, heads, D, None, None) == 1  # NTS_ERR_INVALID
        assert b"heads must be >= 1 and D >= 1" in lib.nts_hip_last_error()
        assert lib.nts_hip_gat_graph_fwd(None, ctypes.byref(g), 0, 10, None, 0, heads, D, None, None,
                                         0, 0) == 1
        assert b"heads must be >= 1 and D >= 1" in lib.nts_hip_last_error()
    assert lib.nts_hip_gat_graph_fwd(None, None, 0, 0, None, 0, 1, 1, None, None, 0, 0) == 1
    assert b"graph is NULL" in lib.nts_hip_last_error()
    assert lib.nts_hip_gat_graph_fwd(None, ctypes.byref(g), 0, 11, None, 0, 1, 1, None, None, 0, 0) == 1
    assert b"vertex range outside the graph" in lib.nts_hip_last_error()
    assert lib.nts_hip_gat_graph_fwd(None, ctypes.byref(g), 5, 3, None, 0, 1, 1, None, None, 0, 0) == 1
    assert b"v_begin > v_end" in lib.nts_hip_last_error()
