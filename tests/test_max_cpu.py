"""GraphSAGE max aggregator, the parts that need no GPU: the exported symbols,
the AGGREGATOR cfg key, the config field and the entry points' argument checks."""
import ctypes

import pytest

from conftest import GOLDEN, ROOT
from nts import dataloader

CFG = GOLDEN / "cora" / "gcn_cora_sample.cfg"
SYMBOLS = ("nts_hip_spmm_csc_fwd_max", "nts_hip_spmm_csr_bwd_max", "nts_hip_spmm_graph_fwd_max")


def test_symbols_are_declared_and_exported():
    from nts import _abi
    header = (ROOT / "include" / "nts_hip.h").read_text()
    lib = _abi.lib()
    for name in SYMBOLS:
        assert f"int {name}(" in header
        assert name in _abi.EXPORTED
        assert getattr(lib, name).argtypes is not None
    assert lib.nts_hip_abi_version() == 11


def test_aggregator_key_parses_and_defaults_to_sum(tmp_path):
    assert dataloader.InputInfo.from_cfg(CFG).aggregator == "sum"
    (tmp_path / "job.cfg").write_text(CFG.read_text() + "AGGREGATOR:max\n")
    info = dataloader.InputInfo.from_cfg(tmp_path / "job.cfg")
    assert info.aggregator == "max"
    assert info.layers == [1433, 256, 7]  # the rest of the job is unchanged
    (tmp_path / "bad.cfg").write_text(CFG.read_text() + "AGGREGATOR:median\n")
    with pytest.raises((ValueError, SystemExit), match="median"):
        dataloader.InputInfo.from_cfg(tmp_path / "bad.cfg")


def test_gcn_config_sets_the_field_and_rejects_unknown_names():
    from nts import host
    assert host.gcn_config([32, 16, 8], [5, 5], 64).aggregator == 0
    assert host.gcn_config([32, 16, 8], [5, 5], 64, aggregator="sum").aggregator == 0
    assert host.gcn_config([32, 16, 8], [5, 5], 64, aggregator="max").aggregator == 1
    with pytest.raises(ValueError, match="median"):
        host.gcn_config([32, 16, 8], [5, 5], 64, aggregator="median")


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from nts import _abi
    lib = _abi.lib()
    buf = (ctypes.c_uint32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)  # any non-NULL address: nothing is launched

    def invalid(rc, what):
        assert rc == 1  # NTS_ERR_INVALID
        assert b"invalid argument" in lib.nts_hip_last_error()
        assert what in lib.nts_hip_last_error()

    fwd, bwd, full = (getattr(lib, s) for s in SYMBOLS)
    # (ctx, co, ri, v, v_cap, x, ldx, map, self, F, y, ldy, arg)
    invalid(fwd(None, p, p, p, 4, p, 8, None, None, 8, p, 8, None), b"NULL")
    invalid(fwd(p, p, p, p, 4, p, 8, None, None, 8, None, 8, None), b"NULL")
    invalid(fwd(p, p, p, p, 4, p, 8, None, None, 0, p, 8, None), b"feature_size")
    invalid(fwd(p, p, p, p, 4, p, 7, None, None, 8, p, 8, None), b"leading dimension")
    invalid(fwd(p, p, p, p, 4, p, 8, None, p, 8, p, 15, None), b"2 feature_size")
    # (ctx, ro, ci, ceid, s, s_cap, g, ld_g, arg, src_dst, x_act, ld_act, scale, F, g_in, ld_gin)
    invalid(bwd(p, p, p, None, p, 4, p, 8, p, None, None, 0, 1.0, 8, p, 8), b"NULL")
    invalid(bwd(p, p, p, p, p, 4, p, 8, None, None, None, 0, 1.0, 8, p, 8), b"NULL")
    invalid(bwd(p, p, p, p, p, 4, p, 15, p, p, None, 0, 1.0, 8, p, 8), b"2 feature_size")
    invalid(bwd(p, p, p, p, p, 4, p, 8, p, None, None, 0, 1.0, 0, p, 8), b"feature_size")
    invalid(bwd(p, p, p, p, p, 4, p, 8, p, None, p, 7, 1.0, 8, p, 8), b"leading dimension")
    # (ctx, graph, v_begin, v_end, relu, x, ldx, F, y, ldy)
    invalid(full(p, None, 0, 4, 0, p, 8, 8, p, 8), b"graph is NULL")
    g = _abi.GraphDev(4, 0, p.value, None, None, None)
    invalid(full(p, ctypes.byref(g), 0, 5, 0, p, 8, 8, p, 8), b"vertex range")
    invalid(full(p, ctypes.byref(g), 3, 2, 0, p, 8, 8, p, 8), b"v_begin")
