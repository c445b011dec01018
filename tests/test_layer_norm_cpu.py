"""LAYER_NORM without a GPU: the option reaches GCNConfig, the cfg key parses,
GAT algorithms refuse it, and the backward formulas of nts_hip_ln_act_bwd
(include/nts_hip.h), restated in float64 torch, agree with autograd through
layer_norm -> relu -> mask.  That pins the formulas the GPU tests check the
kernels against."""
import pytest
import torch


def test_gcn_config_carries_the_option():
    from nts import host
    c = host.gcn_config([32, 16, 8], [5, 5], 64)
    assert c.layer_norm is False and c.layer_norm_eps == pytest.approx(1e-5)
    c = host.gcn_config([32, 16, 8], [5, 5], 64, layer_norm=True, layer_norm_eps=1e-3)
    assert c.layer_norm is True and c.layer_norm_eps == pytest.approx(1e-3)


def _cfg(tmp_path, golden, algorithm):
    text = (golden / "cora" / "gcn_cora_sample.cfg").read_text()
    text = text.replace("ALGORITHM:GCNSAMPLEALLGPU", f"ALGORITHM:{algorithm}")
    (tmp_path / "ln.cfg").write_text(text + "LAYER_NORM:1\n")
    return tmp_path / "ln.cfg"


def test_cfg_key_parses(tmp_path, golden):
    from nts import dataloader
    assert dataloader.InputInfo.from_cfg(_cfg(tmp_path, golden, "GCNSAMPLEALLGPU")).layer_norm == 1
    assert dataloader.InputInfo.from_cfg(golden / "cora" / "gcn_cora_sample.cfg").layer_norm == 0


@pytest.mark.parametrize("algorithm", ["GATSAMPLEALLGPU", "GCNSAMPLEPDCACHE"])
def test_gat_and_pd_cache_algorithms_refuse_it(tmp_path, golden, algorithm):
    from nts import dataloader, run
    info = dataloader.InputInfo.from_cfg(_cfg(tmp_path, golden, algorithm))
    with pytest.raises(SystemExit) as ei:
        run.build_driver(None, info, None, None, None, None, None)
    assert str(ei.value) == (f"ALGORITHM {algorithm}: LAYER_NORM is not supported with GAT or "
                             "PD-cache algorithms (GCN / GraphSAGE layers only)")


@pytest.mark.parametrize("rows,F,p", [(5, 7, 0.0), (33, 64, 0.5), (4, 1, 0.0)])
def test_backward_formulas_agree_with_autograd(rows, F, p):
    g = torch.Generator().manual_seed(rows * 100 + F)
    z = torch.randn(rows, F, generator=g, dtype=torch.float64, requires_grad=True)
    gamma = (1 + 0.1 * torch.randn(F, generator=g, dtype=torch.float64)).requires_grad_()
    beta = (0.1 * torch.randn(F, generator=g, dtype=torch.float64)).requires_grad_()
    dy = torch.randn(rows, F, generator=g, dtype=torch.float64)
    keep = (torch.rand(rows, F, generator=g) >= p).double()
    scale, eps = 1.0 / (1.0 - p), 1e-5
    y = torch.relu(torch.nn.functional.layer_norm(z, (F,), gamma, beta, eps)) * keep * scale
    y.backward(dy)
    with torch.no_grad():
        mean = z.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((z - mean) ** 2).mean(1, keepdim=True) + eps)
        xh = (z - mean) * rstd
        gg = dy * (y > 0) * scale
        t = gg * gamma
        dz = rstd * (t - t.mean(1, keepdim=True) - xh * (t * xh).mean(1, keepdim=True))
        torch.testing.assert_close(dz, z.grad, rtol=1e-10, atol=1e-12)
        torch.testing.assert_close(gg.sum(0), beta.grad, rtol=1e-10, atol=1e-12)
        torch.testing.assert_close((gg * xh).sum(0), gamma.grad, rtol=1e-10, atol=1e-12)
