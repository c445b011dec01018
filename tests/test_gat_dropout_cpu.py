"""GAT dropout (gat_attn_drop / gat_feat_drop) without a GPU: the two
options through gcn_config, their refusals, the cfg keys, the runner's refusal
for a GCN algorithm, the five new C-ABI entry points, and the torch chain the GPU
tests use as their reference (tests/gat_drop_blocks.py) against an independent
numpy float64 loop on a toy block."""
import subprocess

import numpy as np
import pytest
import torch

import gat_drop_blocks as gdb
from conftest import GOLDEN

CFG = GOLDEN / "cora" / "gcn_cora_sample.cfg"
NEW = ("nts_hip_gat_forward_drop", "nts_hip_gat_backward_drop", "nts_hip_gat_forward_heads_drop",
       "nts_hip_gat_backward_heads_drop", "nts_hip_dropout_f32")


def test_gcn_config_sets_the_rates_and_defaults_to_zero():
    from nts import host
    c = host.gcn_config([32, 16, 8], [5, 5], 64, gat=True, gat_attn_drop=0.6, gat_feat_drop=0.5)
    assert c.gat_attn_drop == 0.6 and c.gat_feat_drop == 0.5
    for kw in (dict(gat=True), dict(gat=False)):
        c = host.gcn_config([32, 16, 8], [5, 5], 64, **kw)
        assert c.gat_attn_drop == 0.0 and c.gat_feat_drop == 0.0
    # explicit zeros are the default, with or without gat
    c = host.gcn_config([32, 16, 8], [5, 5], 64, gat_attn_drop=0.0, gat_feat_drop=0.0)
    assert c.gat_attn_drop == 0.0 and c.gat_feat_drop == 0.0


@pytest.mark.parametrize("name", ["gat_attn_drop", "gat_feat_drop"])
def test_gcn_config_refuses_a_rate_without_gat_or_out_of_range(name):
    from nts import host
    with pytest.raises(ValueError, match=f"{name} is not supported without gat"):
        host.gcn_config([32, 16, 8], [5, 5], 64, gat=False, **{name: 0.5})
    for bad in (1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match=rf"{name} must be in \[0, 1\), got"):
            host.gcn_config([32, 16, 8], [5, 5], 64, gat=True, **{name: bad})


def test_cfg_keys_parse(tmp_path):
    from nts import dataloader
    (tmp_path / "job.cfg").write_text(CFG.read_text() + "GAT_ATTN_DROP:0.6\nGAT_FEAT_DROP:0.25\n")
    info = dataloader.InputInfo.from_cfg(tmp_path / "job.cfg")
    assert info.gat_attn_drop == 0.6 and info.gat_feat_drop == 0.25
    assert "GAT_ATTN_DROP" not in info.extra and "GAT_FEAT_DROP" not in info.extra
    info = dataloader.InputInfo.from_cfg(CFG)
    assert info.gat_attn_drop == 0.0 and info.gat_feat_drop == 0.0


@pytest.mark.parametrize("key", ["GAT_ATTN_DROP", "GAT_FEAT_DROP"])
def test_run_refuses_the_keys_with_a_gcn_algorithm(tmp_path, key):
    from nts import dataloader, run
    (tmp_path / "job.cfg").write_text(CFG.read_text() + f"{key}:0.6\n")
    info = dataloader.InputInfo.from_cfg(tmp_path / "job.cfg")
    assert run.ALGORITHMS[info.algorithm.upper()][0] != "gat"
    with pytest.raises(SystemExit, match=f"{key} is not supported with GCN"):
        run.build_driver(None, info, None, None, None, None, None)


def test_the_library_exports_the_five_entry_points():
    from nts import _abi
    for s in NEW:
        assert s in _abi.EXPORTED, s
    lib = _abi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    for s in NEW:
        assert hasattr(lib, s) and f" T {s}\n" in out, s
    assert lib.nts_hip_abi_version() == 11
    # a refused rate touches no GPU: NaN, negative and above 1
    for p in (float("nan"), -0.5, 1.5):
        rc = lib.nts_hip_dropout_f32(1, 1, 1, 1, 1, p, 0, 0, 1, 1)
        assert rc == 1 and b"[0, 1]" in lib.nts_hip_last_error()


@pytest.mark.parametrize("K,D,mean", [(1, 5, False), (3, 4, False), (2, 3, True)])
def test_the_torch_chain_agrees_with_the_float64_loop(K, D, mean):
    """a toy block (columns of 0, 1, 3 and 6 edges), given masks, q = 0.6, p = 0.5"""
    rng = np.random.default_rng(10 * K + D)
    deg = np.array([3, 0, 1, 6])
    co = np.concatenate([[0], np.cumsum(deg)])
    s, v, e, F = 7, len(deg), int(co[-1]), K * D
    ri = rng.integers(0, s, e)
    dl = rng.permutation(s)[:v]
    H = rng.standard_normal((s, F))
    att = rng.standard_normal(2 * F)
    keepA = rng.random((e, K)) >= 0.6
    keepA[int(co[2])] = False  # the only edge of a column dropped in every head
    keepF = rng.random((v, D if mean else F)) >= 0.5
    sa, sf = gdb.scale(0.6), gdb.scale(0.5)
    assert sa == float(np.float32(1) / np.float32(1 - np.float32(0.6))) and sf == 2.0
    Yl, ml, al = gdb.drop_loop(H, att, co, ri, dl, K, D, mean, keepA, sa, keepF, sf)
    t = torch.from_numpy
    Y, m, a, _ = gdb.drop_chain(t(H), t(att), t(co), t(ri), t(dl), K, D, mean, t(keepA), sa,
                                t(keepF), sf)
    for got, ref in ((Y, Yl), (m, ml), (a, al)):
        assert np.allclose(got.numpy(), ref, rtol=1e-12, atol=1e-13)
    assert not Y[1].any() and not Y[2].any()  # no edges; its one edge dropped
    # the undropped softmax still sums to one over the dropped edges too
    d_of_e = np.repeat(np.arange(v), deg)
    for h in range(K):
        assert np.allclose(np.bincount(d_of_e, weights=al[:, h], minlength=v)[deg > 0], 1.0)
    # without masks the chain is the plain layer
    import gat_heads_blocks as ghb
    Y0, _, _ = ghb.heads_chain(t(H), t(att), t(co), t(ri), t(dl), K, D, mean)
    Y1, _, _, _ = gdb.drop_chain(t(H), t(att), t(co), t(ri), t(dl), K, D, mean)
    assert np.allclose(Y0.numpy(), Y1.numpy(), rtol=1e-12, atol=1e-13)
    assert gdb.scale(1.0) == 0.0
