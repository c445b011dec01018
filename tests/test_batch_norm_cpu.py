"""BATCH_NORM without a GPU: the option reaches GCNConfig, the cfg key parses, the
runner's and the driver's refusals have their texts, the header and the
library carry the three entry points, and DESIGN §8s's formulas, restated in
float64 torch, agree with autograd through batch_norm -> relu -> mask.  That
pins the formulas the GPU tests check the kernels against.  The relu-gate cap
of every case of tests/test_batch_norm_kernel.py is asserted here on the
float64 chain alone."""
import ctypes

import pytest
import torch

import batch_norm_cases as bc
from conftest import ROOT
from test_driver_options_cpu import check, refusal
from test_layer_norm_driver import REFUSALS as LN_REFUSALS

LEAD = "batch_norm is not supported with "
REFUSALS = {
    "gat": (dict(gat=True, weight="none"), None, LEAD + "gat (GCN / GraphSAGE layers only)"),
    "pd_cache": (dict(pd_cache=True), None, LEAD + "pd_cache"),
    "transform_first": (dict(transform_first=1), None,
                        LEAD + "transform_first = 1 (BatchNorm does not commute with A: "
                        "aggregate-first only)"),
    "pair_table": (dict(pair_table=1), None, LEAD + "pair_table > 0"),
    "layer_norm": (dict(layer_norm=True), None,
                   LEAD + "layer_norm (one normalisation per hidden layer)"),
    "width": ({}, [8, 1028, 2], LEAD + "a hidden width above 1024 (layer 0: 1028)"),
}


def test_gcn_config_carries_the_option():
    from nts import host
    c = host.gcn_config([32, 16, 8], [5, 5], 64)
    assert c.batch_norm is False and c.batch_norm_eps == pytest.approx(1e-5)
    assert c.batch_norm_momentum == pytest.approx(0.1)
    c = host.gcn_config([32, 16, 8], [5, 5], 64, batch_norm=True, batch_norm_eps=1e-3,
                        batch_norm_momentum=0.25)
    assert c.batch_norm is True and c.batch_norm_eps == pytest.approx(1e-3)
    assert c.batch_norm_momentum == pytest.approx(0.25)


def _cfg(tmp_path, golden, algorithm, extra=""):
    text = (golden / "cora" / "gcn_cora_sample.cfg").read_text()
    text = text.replace("ALGORITHM:GCNSAMPLEALLGPU", f"ALGORITHM:{algorithm}")
    (tmp_path / "bn.cfg").write_text(text + "BATCH_NORM:1\n" + extra)
    return tmp_path / "bn.cfg"


def test_cfg_key_parses(tmp_path, golden):
    from nts import dataloader
    assert dataloader.InputInfo.from_cfg(_cfg(tmp_path, golden, "GCNSAMPLEALLGPU")).batch_norm == 1
    assert dataloader.InputInfo.from_cfg(golden / "cora" / "gcn_cora_sample.cfg").batch_norm == 0


@pytest.mark.parametrize("algorithm,extra,text", [
    ("GATSAMPLEALLGPU", "", "BATCH_NORM is not supported with GAT or PD-cache algorithms (GCN / "
                            "GraphSAGE layers only)"),
    ("GCNSAMPLEPDCACHE", "", "BATCH_NORM is not supported with GAT or PD-cache algorithms (GCN / "
                             "GraphSAGE layers only)"),
    ("GCNSAMPLEALLGPU", "LAYER_NORM:1\n", "BATCH_NORM is not supported with LAYER_NORM:1 (one "
                                          "normalisation per hidden layer)"),
], ids=["gat", "pd_cache", "layer_norm"])
def test_the_runner_refuses_it(tmp_path, golden, algorithm, extra, text):
    from nts import dataloader, run
    info = dataloader.InputInfo.from_cfg(_cfg(tmp_path, golden, algorithm, extra))
    with pytest.raises(SystemExit) as ei:
        run.build_driver(None, info, None, None, None, None, None)
    assert str(ei.value) == f"ALGORITHM {algorithm}: {text}"


def test_the_help_text_names_the_key():
    from nts import run
    assert "BATCH_NORM:1" in run.__doc__


@pytest.mark.parametrize("name", list(REFUSALS))
def test_driver_refusals(name):
    kw, layers, text = REFUSALS[name]
    kw = dict(kw, **({"layers": layers} if layers else {}))
    assert refusal(batch_norm=True, **kw) == text


def test_alone_it_is_accepted_and_earlier_conflicts_come_first():
    check(batch_norm=True)
    check(batch_norm=True, root_weight=True)
    check(batch_norm=True, aggregator="max")
    assert refusal(batch_norm=True, layer_norm=True, pd_cache=True) == LN_REFUSALS["pd_cache"][2]
    # the option's own text reports transform_first = 1, not the generic row
    assert refusal(batch_norm=True, transform_first=1).startswith(LEAD + "transform_first = 1")


def test_header_and_library_carry_the_entry_points():
    from nts import _abi
    header = (ROOT / "include" / "nts_hip.h").read_text()
    lib = ctypes.CDLL(str(_abi.LIB_PATH))
    for name in ("nts_hip_bn_act_fwd", "nts_hip_bn_act_eval", "nts_hip_bn_act_bwd"):
        assert f"int {name}(nts_hip_ctx *ctx" in header
        assert name in _abi.EXPORTED
        assert hasattr(lib, name)
    assert _abi.ABI_VERSION == 11 and "#define NTS_HIP_ABI_VERSION 11" in header


def _formulas(z, gamma, beta, rm, rv, keep, scale, dy, eps, mom):
    """DESIGN §8s, column-wise over n = rows"""
    n = z.shape[0]
    mu = z.mean(0)
    var = ((z - mu) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (z - mu) * rstd
    y = torch.relu(gamma * xh + beta) * keep * scale
    g = dy * (y > 0) * scale
    dbeta, dgamma = g.sum(0), (g * xh).sum(0)
    dz = gamma * rstd * (g - dbeta / n - xh * dgamma / n)
    if n > 1:
        rm = (1 - mom) * rm + mom * mu
        rv = (1 - mom) * rv + mom * var * n / (n - 1)
    return y, dz, dgamma, dbeta, rm, rv


@pytest.mark.parametrize("rows,F,p", [(5, 7, 0.0), (33, 64, 0.5), (2, 3, 0.0), (4, 1, 0.5)])
def test_formulas_agree_with_autograd(rows, F, p):
    g = torch.Generator().manual_seed(rows * 100 + F)
    z = torch.randn(rows, F, generator=g, dtype=torch.float64, requires_grad=True)
    gamma = (1 + 0.1 * torch.randn(F, generator=g, dtype=torch.float64)).requires_grad_()
    beta = (0.1 * torch.randn(F, generator=g, dtype=torch.float64)).requires_grad_()
    dy = torch.randn(rows, F, generator=g, dtype=torch.float64)
    keep = (torch.rand(rows, F, generator=g) >= p).double()
    rm0 = torch.randn(F, generator=g, dtype=torch.float64)
    rv0 = 0.5 + torch.rand(F, generator=g, dtype=torch.float64)
    scale, eps, mom = 1.0 / (1.0 - p), 1e-5, 0.1
    rm, rv = rm0.clone(), rv0.clone()
    y = torch.relu(torch.nn.functional.batch_norm(z, rm, rv, gamma, beta, True, mom, eps)) * keep * scale
    y.backward(dy)
    with torch.no_grad():
        fy, dz, dgamma, dbeta, frm, frv = _formulas(z, gamma, beta, rm0, rv0, keep, scale, dy, eps, mom)
        for a, b in ((fy, y), (dz, z.grad), (dgamma, gamma.grad), (dbeta, beta.grad), (frm, rm),
                     (frv, rv)):
            torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-12)


def test_one_row_leaves_the_buffers_and_gives_the_activation_of_beta():
    g = torch.Generator().manual_seed(9)
    F = 6
    z = torch.randn(1, F, generator=g, dtype=torch.float64)
    gamma = 1 + 0.1 * torch.randn(F, generator=g, dtype=torch.float64)
    beta = torch.randn(F, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(F, dtype=torch.float64), torch.rand(F, dtype=torch.float64) + 0.5
    dy, keep = torch.randn(1, F, dtype=torch.float64), torch.ones(1, F, dtype=torch.float64)
    y, dz, dgamma, dbeta, frm, frv = _formulas(z, gamma, beta, rm, rv, keep, 2.0, dy, 1e-5, 0.1)
    assert torch.equal(frm, rm) and torch.equal(frv, rv)
    assert torch.equal(y, torch.relu(beta)[None] * 2.0)
    assert float(dz.abs().max()) == 0.0 and float(dgamma.abs().max()) == 0.0
    # the shared chain of the GPU tests takes the same path
    q, n = bc.chain(z.float(), gamma.float(), beta.float(), rm.float(), rv.float(), keep, 2.0,
                    dy.float(), torch.float64)
    assert torch.equal(q["running_mean"], rm.float().double()) and float(q["dz"].abs().max()) == 0.0
    assert torch.equal(q["y"], torch.relu(beta.float().double())[None] * 2.0)


@pytest.mark.parametrize("rows,F", [(5, 7), (33, 64)])
def test_eval_formula_agrees_with_batch_norm_in_eval_mode(rows, F):
    g = torch.Generator().manual_seed(rows + F)
    z = torch.randn(rows, F, generator=g, dtype=torch.float64)
    gamma = 1 + 0.1 * torch.randn(F, generator=g, dtype=torch.float64)
    beta = 0.1 * torch.randn(F, generator=g, dtype=torch.float64)
    rm = torch.randn(F, generator=g, dtype=torch.float64)
    rv = 0.5 + torch.rand(F, generator=g, dtype=torch.float64)
    want = torch.relu(torch.nn.functional.batch_norm(z, rm.clone(), rv.clone(), gamma, beta, False,
                                                     0.1, 1e-5))
    got = torch.relu(gamma * (z - rm) / torch.sqrt(rv + 1e-5) + beta)
    torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(bc.eval_chain(z, gamma, beta, rm, rv, torch.float64)[0], want,
                               rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("layout,rows", bc.CASES, ids=[f"{l}-rows{r}" for l, r in bc.CASES])
def test_relu_gate_cap_of_every_kernel_case(layout, rows):
    for kind in bc.KINDS:
        _, near, enear, share = bc.pick(layout, rows, kind)
        assert share <= bc.MASK_CAP, f"{kind}: {share:.2e} of the pre-activations within 1e-4 of zero"
