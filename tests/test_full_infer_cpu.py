"""Full-graph inference, the parts that need no GPU: the FULL_INFERENCE cfg key
and the argument checks of nts_hip_spmm_graph_fwd."""
import ctypes

from conftest import GOLDEN
from nts import dataloader

CFG = GOLDEN / "cora" / "gcn_cora_sample.cfg"


def test_full_inference_key_parses_and_defaults_to_off(tmp_path):
    assert dataloader.InputInfo.from_cfg(CFG).full_inference == 0
    (tmp_path / "job.cfg").write_text(CFG.read_text() + "FULL_INFERENCE:1\n")
    info = dataloader.InputInfo.from_cfg(tmp_path / "job.cfg")
    assert info.full_inference == 1
    assert info.layers == [1433, 256, 7]  # the rest of the job is unchanged
    (tmp_path / "off.cfg").write_text(CFG.read_text() + "FULL_INFERENCE:0\n")
    assert dataloader.InputInfo.from_cfg(tmp_path / "off.cfg").full_inference == 0


def test_spmm_graph_fwd_rejects_bad_arguments_without_a_gpu():
    from nts import _abi
    lib = _abi.lib()
    # NULL graph
    rc = lib.nts_hip_spmm_graph_fwd(None, None, 0, 0, _abi.NTS_WEIGHT_SUM, 0, None, 0, 0, None, 0)
    assert rc == 1  # NTS_ERR_INVALID
    assert b"invalid argument" in lib.nts_hip_last_error()
    assert b"graph is NULL" in lib.nts_hip_last_error()
    # v_begin > v_end
    g = _abi.GraphDev(10, 0, None, None, None, None)
    rc = lib.nts_hip_spmm_graph_fwd(None, ctypes.byref(g), 5, 3, _abi.NTS_WEIGHT_SUM, 0, None, 0, 0,
                                    None, 0)
    assert rc == 1
    assert b"v_begin > v_end" in lib.nts_hip_last_error()
