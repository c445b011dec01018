"""GATv2 (gat_v2) without a GPU: the references of
tests/gatv2_blocks.py against each other and against closed forms, the property
GAT cannot have (two destinations ranking the same neighbours differently), the
backward formulas of the kernels against autograd and their sensitivity to the
plausible kernel mistakes, the GAT_V2 cfg key, the gcn_config / runner refusals
and the two new C-ABI entry points.
"""
import pathlib
import subprocess

import numpy as np
import pytest
import torch

import gat_blocks
import gatv2_blocks as g2b
from conftest import GOLDEN
from step_check import err

CFG = GOLDEN / "cora" / "gcn_cora_sample.cfg"
NEW = ("nts_hip_gatv2_forward", "nts_hip_gatv2_backward")
ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def block():
    b = gat_blocks.make_block()
    return dict(co=torch.from_numpy(b["column_offset"].astype(np.int64)),
                ri=torch.from_numpy(b["row_indices"].astype(np.int64)),
                np=b, v=b["v"], s=b["s"], e=b["e"])


def _inputs(block, K, D, mean, seed=0, scale=0.3):
    g = torch.Generator().manual_seed(seed)
    F = K * D
    Hs = torch.randn(block["s"], F, generator=g, dtype=torch.float64)
    Hd = torch.randn(block["v"], F, generator=g, dtype=torch.float64)
    att = torch.randn(F, generator=g, dtype=torch.float64) * scale
    GY = torch.randn(block["v"], D if mean else F, generator=g, dtype=torch.float64)
    return Hs, Hd, att, GY


@pytest.mark.parametrize("K,D,mean", [(1, 5, False), (3, 4, False), (2, 3, True), (4, 2, True)])
def test_the_chain_equals_the_loop(block, K, D, mean):
    Hs, Hd, att, _ = _inputs(block, K, D, mean)
    Z, u, a = g2b.v2_chain_z(Hs, Hd, att, block["co"], block["ri"], K, D, mean)
    Zl, ul, al = g2b.v2_loop(Hs.numpy(), Hd.numpy(), att.numpy(), block["np"]["column_offset"],
                             block["np"]["row_indices"], K, D, mean)
    for got, ref in ((Z, Zl), (u, ul), (a, al)):
        assert float((got - torch.from_numpy(ref)).abs().max()) <= 1e-12


def test_zero_score_vector_gives_uniform_attention(block):
    K, D = 1, 6
    Hs, Hd, _, _ = _inputs(block, K, D, False)
    Z, u, a = g2b.v2_chain_z(Hs, Hd, torch.zeros(D, dtype=torch.float64), block["co"],
                             block["ri"], K, D, False)
    co, ri = block["co"], block["ri"]
    assert not u.any()
    for d in range(block["v"]):
        b, n = int(co[d]), int(co[d + 1])
        if n == b:
            assert not Z[d].any()
            continue
        assert float((a[b:n] - 1.0 / (n - b)).abs().max()) <= 1e-15
        assert float((Z[d] - Hs[ri[b:n]].mean(0)).abs().max()) <= 1e-12


def test_positive_sums_reduce_to_a_source_only_softmax(block):
    """K = 1 with every Hs + Hd positive: leaky_relu is the identity, the
    destination term is a constant of the softmax, and a = softmax(Hs[src] . att)."""
    K, D = 1, 5
    Hs, Hd, att, _ = _inputs(block, K, D, False)
    Hs, Hd = Hs.abs() + 0.1, Hd.abs() + 0.1
    _, u, a = g2b.v2_chain_z(Hs, Hd, att, block["co"], block["ri"], K, D, False)
    co, ri = block["co"], block["ri"]
    for d in range(block["v"]):
        b, n = int(co[d]), int(co[d + 1])
        if n == b:
            continue
        assert float((u[b:n, 0] - (Hs[ri[b:n]] + Hd[d]) @ att).abs().max()) <= 1e-12
        ref = torch.softmax(Hs[ri[b:n]] @ att, 0)
        assert float((a[b:n, 0] - ref).abs().max()) <= 1e-12


def test_two_destinations_rank_the_same_neighbours_differently():
    """The property GAT cannot have (Brody et al., section 3): with GAT every
    destination orders its neighbours by H[src] . a1 alone; GATv2's order
    depends on the destination."""
    co, ri = torch.tensor([0, 2, 4]), torch.tensor([0, 1, 0, 1])
    f64 = torch.float64
    Hs = torch.tensor([[2.0, -2.0], [-2.0, 2.0]], dtype=f64)
    Hd = torch.tensor([[1.0, -1.0], [-1.0, 1.0]], dtype=f64)
    att = torch.ones(2, dtype=f64)
    _, u, a = g2b.v2_chain_z(Hs, Hd, att, co, ri, 1, 2, False)
    assert torch.allclose(u.view(-1), torch.tensor([2.4, 0.8, 0.8, 2.4], dtype=f64))
    assert a[0, 0] > a[1, 0] and a[2, 0] < a[3, 0]
    # swapping the destinations swaps the attention
    _, _, a2 = g2b.v2_chain_z(Hs, Hd.flip(0), att, co, ri, 1, 2, False)
    assert torch.equal(a2.view(2, 2), a.view(2, 2).flip(0))
    # GAT on the same rows (sources 0, 1; destinations are rows 2, 3): one order
    # for both destinations, whatever the attention vector
    H = torch.cat([Hs, Hd])
    g = torch.Generator().manual_seed(1)
    for _ in range(20):
        watt = torch.randn(4, generator=g, dtype=f64)
        _, _, ag = gat_blocks.gat_chain_z(H, watt, co, ri, torch.tensor([2, 3]), 2)
        assert (ag[0] > ag[1]) == (ag[2] > ag[3])


def _autograd(block, Hs, Hd, att, GY, K, D, mean):
    hs, hd, ad = (t.clone().requires_grad_(True) for t in (Hs, Hd, att))
    Z, _, _ = g2b.v2_chain_z(hs, hd, ad, block["co"], block["ri"], K, D, mean)
    torch.relu(Z).backward(GY)
    return dict(dHs=hs.grad, dHd=hd.grad, datt=ad.grad)


@pytest.mark.parametrize("K,D,mean", [(1, 5, False), (3, 4, False), (4, 3, True)])
def test_the_backward_formulas_are_the_chain_s_gradient(block, K, D, mean):
    """dHs, dHd and datt as the kernels compute them against
    autograd through the materialised chain, in float64"""
    Hs, Hd, att, GY = _inputs(block, K, D, mean)
    ref = _autograd(block, Hs, Hd, att, GY, K, D, mean)
    dHs, dHd, datt, _ = g2b.v2_manual_grads(Hs, Hd, att, block["co"], block["ri"], K, D, mean, GY)
    for name, got in (("dHs", dHs), ("dHd", dHd), ("datt", datt)):
        assert err(got, ref[name]) <= 1e-12, name


@pytest.mark.parametrize("flag,K,D,mean", [("leaky_from_score", 3, 4, False),
                                           ("wrong_head", 3, 4, False),
                                           ("no_inv_k", 4, 3, True),
                                           ("drop_q", 3, 4, False)])
def test_each_plausible_kernel_mistake_is_visible(block, flag, K, D, mean):
    """leaky' taken from the score instead of the sum, a reduction over the
    wrong head, a missing 1/K, q left out of dHs: each moves some quantity by
    1e-2 or more of its size, far above the kernel tests' bounds."""
    Hs, Hd, att, GY = _inputs(block, K, D, mean)
    ref = _autograd(block, Hs, Hd, att, GY, K, D, mean)
    dHs, dHd, datt, _ = g2b.v2_manual_grads(Hs, Hd, att, block["co"], block["ri"], K, D, mean, GY,
                                            **{flag: True})
    moved = {n: err(g, ref[n]) for n, g in (("dHs", dHs), ("dHd", dHd), ("datt", datt))}
    print(flag, {k: f"{v:.3e}" for k, v in moved.items()})
    assert max(moved.values()) >= 1e-2


def test_gcn_config_sets_gat_v2_and_defaults_to_off():
    from nts import host
    assert host.gcn_config([32, 16, 8], [5, 5], 64, gat=True, gat_v2=True).gat_v2 is True
    for kw in (dict(gat=True), dict(gat=False), dict(gat=True, gat_v2=False)):
        assert host.gcn_config([32, 16, 8], [5, 5], 64, **kw).gat_v2 is False
    with pytest.raises(ValueError,
                       match=r"gat_v2 is not supported without gat \(attention layers only\)"):
        host.gcn_config([32, 16, 8], [5, 5], 64, gat=False, gat_v2=True)


def test_the_cfg_key_parses_and_the_runner_refuses_it_where_it_cannot_apply(tmp_path):
    from nts import dataloader, run
    (tmp_path / "job.cfg").write_text(CFG.read_text() + "GAT_V2:1\n")
    info = dataloader.InputInfo.from_cfg(tmp_path / "job.cfg")
    assert info.gat_v2 == 1 and "GAT_V2" not in info.extra
    assert dataloader.InputInfo.from_cfg(CFG).gat_v2 == 0
    assert run.ALGORITHMS[info.algorithm.upper()][0] != "gat"
    with pytest.raises(SystemExit, match="GAT_V2 is not supported with GCN / GraphSAGE algorithms"):
        run.build_driver(None, info, None, None, None, None, None)
    text = CFG.read_text().replace("ALGORITHM:GCNSAMPLEALLGPU", "ALGORITHM:GATSAMPLEALLGPU")
    (tmp_path / "full.cfg").write_text(text + "GAT_V2:1\nFULL_INFERENCE:1\n")
    info = dataloader.InputInfo.from_cfg(tmp_path / "full.cfg")
    with pytest.raises(SystemExit, match="FULL_INFERENCE is not supported with GAT_V2"):
        run.build_driver(None, info, None, None, None, None, None)


def test_the_library_and_the_header_have_the_two_entry_points():
    from nts import _abi
    for s in NEW:
        assert s in _abi.EXPORTED, s
    lib = _abi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    header = (ROOT / "include" / "nts_hip.h").read_text()
    for s in NEW:
        assert hasattr(lib, s) and f" T {s}\n" in out, s
        assert f"int {s}(nts_hip_ctx *ctx" in header, s
    # refusals touch no GPU: a bad rate, no heads, too wide a row
    one = 16  # a non-NULL, 16-byte aligned stand-in for every pointer
    def fwd(heads, D, p):
        return lib.nts_hip_gatv2_forward(one, one, one, 4, one, 2048, one, 2048, heads, D, one, one,
                                         one, one, 2048, 0, p, 0.0, 0, 0, 0)
    for p in (float("nan"), -0.1, 1.5):
        assert fwd(2, 8, p) == 1 and b"[0, 1]" in lib.nts_hip_last_error()
    assert fwd(0, 8, 0.0) == 1 and b"heads must be >= 1" in lib.nts_hip_last_error()
    assert fwd(2, 0, 0.0) == 1 and b"D >= 1" in lib.nts_hip_last_error()
    for heads, D in ((257, 4), (1, 257), (2, 130)):
        assert fwd(heads, D, 0.0) == 1
        msg = lib.nts_hip_last_error()
        assert b"1024" in msg and b"256" in msg, msg
