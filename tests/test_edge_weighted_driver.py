"""Edge weights as aggregation coefficients through the C++ driver
(gcn_config(edge_weighted=True) on a graph with edge_prob).

Shapes of tests/test_weighted_sampling_driver.py (V = 2,000, layers 64-64-7,
fanout 10-5, batch 200, dropout 0) on that graph with its parallel edges
removed, so that the CSC position q of a kept edge is recoverable from its
(src, dst) pair and the block's weights can be held to c * a[q].
"""
import shutil

import numpy as np
import pytest
import torch

import edge_weight_blocks as eb
import step_check

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LAYERS, FANOUT, BATCH = [64, 64, 7], [10, 5], 200
EPS = 1e-5


@pytest.fixture(scope="module")
def E():
    from nts import host
    return host.ext()


@pytest.fixture(scope="module")
def data(E):
    from nts import synthetic
    g = synthetic.chung_lu(2000, 40000, 10.0, device=DEV, seed=5)
    V = g.n_vertices
    pair = np.unique(g.dst.cpu().numpy().astype(np.int64) * V + g.src.cpu().numpy())
    pair = pair[np.random.default_rng(4).permutation(pair.size)]
    src = torch.from_numpy((pair % V).astype(np.int32)).to(DEV)
    dst = torch.from_numpy((pair // V).astype(np.int32)).to(DEV)
    feat = synthetic.features(V, 64, device=DEV)
    labels, masks = synthetic.labels_masks(V, 7, device=DEV)
    train = torch.nonzero(masks == 0).flatten().to(torch.int32).cpu()
    rng = np.random.default_rng(6)
    d = dict(V=V, src=src, dst=dst, feat=feat, labels=labels, masks=masks, train=train,
             multilabels=synthetic.multilabels(V, 7, feat, seed=13))
    d["w_rand"] = torch.from_numpy(np.exp2(rng.uniform(-3, 3, pair.size)).astype(np.float32)).to(DEV)
    d["w_prob"] = torch.from_numpy(np.exp2(rng.uniform(-2, 2, pair.size)).astype(np.float32)).to(DEV)
    d["G_plain"] = E.FullyRepGraph.from_edges(src, dst, V)
    d["G_rand"] = E.FullyRepGraph.from_edges(src, dst, V, d["w_rand"])
    for name, value in (("G_one", 1.0), ("G_two", 2.0)):
        d[name] = E.FullyRepGraph.from_edges(src, dst, V, torch.full_like(d["w_rand"], value))
    G = d["G_rand"]
    d["col"] = G.column_offset.cpu().numpy().astype(np.int64)
    d["rows"] = G.row_indices.cpu().numpy().view(np.uint32)
    d["a"] = G.edge_prob.cpu().numpy()
    return d


def _driver(E, data, G, readout=False, labels=None, layers=LAYERS, fanout=FANOUT, **kw):
    from nts import host
    cfg = host.gcn_config(list(layers), list(fanout), BATCH, drop_rate=0.0, shuffle=False, **kw)
    if readout:
        step_check.readout(cfg)
    return E.GCN_SAMPLE_ALLGPU_impl(data[G], data["feat"], data["labels"] if labels is None else labels,
                                    data["train"], cfg)


def _steps(drv, n):
    losses = []
    for _ in range(n):
        drv.train_batch()
        drv.synchronize()
        losses.append(drv.loss.detach().cpu().clone())
    return losses, [w.cpu().clone() for w in drv.weights()]


ORDERS = {"transform-first": dict(transform_first=1), "aggregate-first": dict(transform_first=0),
          "feature_f16": dict(feature_f16=True)}


@pytest.mark.parametrize("order", list(ORDERS))
def test_coefficients_of_one_are_the_driver_without_the_option(E, data, order):
    kw = ORDERS[order]
    on = _driver(E, data, "G_one", edge_weighted=True, **kw)
    off = _driver(E, data, "G_plain", **kw)
    assert on.transform_first == off.transform_first == (order == "transform-first")
    (la, wa), (lb, wb) = _steps(on, 3), _steps(off, 3)
    assert all(torch.equal(x, y) for x, y in zip(la, lb))
    assert all(torch.equal(x, y) for x, y in zip(wa, wb))


@pytest.mark.parametrize("order", ["transform-first", "aggregate-first"])
def test_coefficients_of_two_scale_every_hop_by_a_power_of_two(E, data, order):
    kw = ORDERS[order]
    on = _driver(E, data, "G_two", edge_weighted=True, **kw)
    off = _driver(E, data, "G_plain", **kw)
    on.set_weights(off.weights())
    seeds = data["train"][:BATCH]
    a, b = on.forward_eval(seeds, 0), off.forward_eval(seeds, 0)
    assert len(a) == len(b) == 4
    if order == "aggregate-first":
        assert torch.equal(a[0], 2 * b[0])  # Y_0 = A X_0
    else:  # transform-first keeps H = X_0[src] W_0 there, before any aggregation: no coefficient in it
        assert torch.equal(a[0], b[0]) and float(b[0].abs().max()) > 0
    assert torch.equal(a[1], 2 * b[1]) and float(b[1].abs().max()) > 0  # X_1 = relu(Y_0 W_0)
    assert torch.equal(a[2], 4 * b[2]) and float(b[2].abs().max()) > 0  # Y_1 = 2^(l+1) Y_l, l = 1
    # the last entry is X_2 = log_softmax(Y_1 W_1), no multiple of the default's;
    # the logits Z = Y_1 W_1 scale by 4 exactly, so the gaps to the row maximum
    # (which log_softmax keeps) do, up to log_softmax's own rounding: each output
    # within 8 ulps of the largest magnitude (subtract, exp-sum, log, subtract),
    # two outputs per gap, the default's error scaled by 4
    gap = lambda t: (t.max(1, keepdim=True).values - t).double()
    assert torch.isfinite(a[3]).all()
    tol = 16 * 2.0 ** -23 * (float(a[3].abs().max()) + 4 * float(b[3].abs().max()))
    torch.testing.assert_close(gap(a[3]), 4 * gap(b[3]), rtol=0, atol=tol)


def _chain(lays, data, ws, dtype, ln=False, labels=None):
    """the model on the trained block (lays: top first) with the block's own
    edge_weight_forward; returns (parameters, loss)"""
    L = len(lays)

    def agg(lay, X):
        co, ri = lay["column_offset"].cpu().long(), lay["row_indices"].cpu().long()
        w = lay["edge_weight_forward"].cpu().to(dtype)
        d_of_e = torch.repeat_interleave(torch.arange(co.numel() - 1), co[1:] - co[:-1])
        return torch.zeros(co.numel() - 1, X.shape[1], dtype=dtype).index_add(0, d_of_e,
                                                                             X[ri] * w[:, None])

    P = [w.to(dtype).requires_grad_() for w in ws]
    X = data["feat"].cpu().to(dtype)[lays[-1]["source"].cpu().long()]
    for l in range(L):
        Z = agg(lays[L - 1 - l], X) @ P[l]
        if l < L - 1:
            if ln:
                Z = torch.nn.functional.layer_norm(Z, (Z.shape[1],), P[L + 2 * l], P[L + 2 * l + 1], EPS)
            X = torch.relu(Z)
    dst = lays[0]["destination"].cpu().long()
    if labels is None:
        loss = torch.nn.functional.nll_loss(Z.log_softmax(1), data["labels"].cpu()[dst])
    else:
        loss = torch.nn.functional.binary_cross_entropy_with_logits(Z, labels.cpu()[dst].to(dtype))
    return P, loss


def _np_layers(lays):
    out = []
    for lay in lays:
        d = {}
        for k in ("destination", "column_offset", "sample_ans", "row_indices", "source"):
            d[k] = lay[k].cpu().numpy().view(np.uint32)
        wf = lay["edge_weight_forward"]  # (None: a driver that builds no weights)
        d["edge_weight_forward"] = None if wf is None else wf.cpu().numpy()
        out.append(d)
    return out


STEP_CASES = {
    "transform-first": dict(transform_first=1),
    "aggregate-first": dict(transform_first=0),
    "layer_norm": dict(layer_norm=True),
    "multi_label": dict(multi_label=True),
    "shared_sampling": dict(shared_sampling=True),
    "weighted_sampling": dict(weighted_sampling=True),
    "weight-none": dict(weight="none"),
}


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_one_readout_step_on_the_trained_block(E, data, case):
    kw = STEP_CASES[case]
    ln = bool(kw.get("layer_norm"))
    labels = data["multilabels"] if kw.get("multi_label") else None
    drv = _driver(E, data, "G_rand", readout=True, labels=labels, edge_weighted=True, **kw)
    W0 = [w.cpu().clone() for w in drv.weights()]
    if ln:  # gamma = 1 + 0.1 randn, beta = 0.1 randn: both gradients are non-trivial
        g = torch.Generator().manual_seed(1)
        for i in range(2, len(W0)):
            r = 0.1 * torch.randn(W0[i].shape, generator=g)
            W0[i] = 1 + r if i % 2 == 0 else r
        drv.set_weights([w.to(DEV) for w in W0])
    drv.train_batch()
    drv.synchronize()
    W1 = [w.cpu().clone() for w in drv.weights()]
    lays = drv.last_layers
    # the block's weights: c (the same block of a driver without the option) times a[q]
    ref = _driver(E, data, "G_rand", readout=True, labels=labels, **kw)
    ref.train_batch()
    ref.synchronize()
    for got, plain in zip(_np_layers(lays), _np_layers(ref.last_layers)):
        for k in ("destination", "column_offset", "sample_ans", "row_indices", "source"):
            assert np.array_equal(got[k], plain[k]), k
        c = np.float32(1) if kw.get("weight") == "none" else plain["edge_weight_forward"]
        q = eb.layer_positions(data["col"], data["rows"], got)
        want = eb.coef_weights(c, data["a"], q)
        assert np.array_equal(got["edge_weight_forward"].view(np.uint32), want.view(np.uint32))
    grads, loss = {}, {}
    for dtype in (torch.float64, torch.float32):
        P, l = _chain(lays, data, W0, dtype, ln, labels)
        l.backward()
        grads[dtype], loss[dtype] = [p.grad for p in P], float(l.detach())
    got = float(drv.loss.detach())
    l64, l32 = loss[torch.float64], loss[torch.float32]
    print(f"edge_weighted {case}: loss {got!r} float64 {l64!r} float32 chain {l32!r}")
    assert abs(got - l64) <= step_check.yardstick_bound(abs(l32 - l64) / abs(l64), step_check.C) * abs(l64)
    names = ["W[0]", "W[1]"] + (["gamma[0]", "beta[0]"] if ln else [])
    step_check.check_step_grads(W0, W1, grads[torch.float64], grads[torch.float32], step_check.C, names)


# infer_full() puts each layer's GEMM on the narrower side: a layer that narrows
# (64 -> 7) is A (X W) there, while the sampled driver's top layer is always
# (A X) W.  Where the two orders coincide the outputs must be equal bit for bit
# (widths 64-64-64: no layer narrows, aggregate-first on both sides); at
# 64-64-7 the top layers associate differently, bit equality cannot hold at
# driver level, and the comparison is the unweighted full-inference tests'
# (rtol = atol = 1e-4) — the bit-for-bit property of the kernels themselves is
# test_edge_weighted_infer_kernel.py::
# test_sub_range_equals_the_take_all_block_and_leaves_other_rows.
@pytest.mark.parametrize("layers", [[64, 64, 64], LAYERS], ids=["same-order", "64-64-7"])
@pytest.mark.parametrize("kw", [dict(), dict(feature_f16=True), dict(weight="mean")],
                         ids=["sum", "feature_f16", "mean"])
def test_evaluate_full_equals_the_take_all_blocks(E, data, kw, layers):
    exact = layers[-1] == 64
    kw = dict(kw, transform_first=0) if exact and not kw.get("feature_f16") else kw
    drv = _driver(E, data, "G_rand", edge_weighted=True, layers=layers, **kw)
    _steps(drv, 3)  # some training, so the rows are not all alike
    take_all = _driver(E, data, "G_rand", edge_weighted=True, layers=layers, fanout=[-1, -1], **kw)
    assert not drv.transform_first or not exact
    take_all.set_weights(drv.weights())
    ids = torch.nonzero(data["masks"].cpu() == 2).flatten().to(torch.int32)[:BATCH]
    full = drv.infer_full().cpu()[ids.long()]
    sampled = take_all.forward_eval(ids, 0)[-1].cpu()
    print(f"edge_weighted infer_full vs take-all blocks ({layers}, {kw}): max |diff| "
          f"{float((full - sampled).abs().max()):.3e}")
    if exact:
        assert torch.equal(sampled, full)
    else:
        torch.testing.assert_close(sampled, full, rtol=1e-4, atol=1e-4)
    correct = int((sampled.argmax(1) == data["labels"].cpu()[ids.long()]).sum())
    assert drv.evaluate_full(ids) == correct / ids.numel()
    # and the coefficients are in it
    plain = _driver(E, data, "G_rand", layers=layers, **kw)
    plain.set_weights(drv.weights())
    assert not torch.equal(plain.infer_full().cpu()[ids.long()], full)


def test_pipeline_on_and_off_give_identical_weights(E, data):
    a = _steps(_driver(E, data, "G_rand", edge_weighted=True, pipeline=True), 4)
    b = _steps(_driver(E, data, "G_rand", edge_weighted=True, pipeline=False), 4)
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0]))
    assert all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    plain = _steps(_driver(E, data, "G_rand", pipeline=False), 4)
    assert not torch.equal(plain[1][0], b[1][0])


def test_evaluate_uses_the_coefficients(E, data):
    ids = torch.nonzero(data["masks"].cpu() == 1).flatten().to(torch.int32)[:150]
    a, b = _driver(E, data, "G_rand", edge_weighted=True), _driver(E, data, "G_rand", edge_weighted=True)
    _steps(a, 2)
    _steps(b, 2)
    first, second = [a.evaluate(ids), a.evaluate(ids)], [b.evaluate(ids), b.evaluate(ids)]
    assert first == second and all(0.0 <= x <= 1.0 for x in first)
    plain = _driver(E, data, "G_rand")
    plain.set_weights(a.weights())
    assert not torch.equal(plain.forward_eval(ids[:64], 0)[-1], a.forward_eval(ids[:64], 0)[-1])


REFUSALS = {
    "edge_prob": ("G_plain", dict()),
    "gat": ("G_rand", dict(gat=True, weight="none")),
    "aggregator = max": ("G_rand", dict(aggregator="max")),
    "root_weight": ("G_rand", dict(root_weight=True)),
    "pd_cache": ("G_rand", dict(pd_cache=True)),
    "sample_gpu": ("G_rand", dict(sample_gpu=True, rng_mode=1)),
    "up_degree": ("G_rand", dict(up_degree=True)),
    "MT19937": ("G_rand", dict(rng_mode=2)),
    "cache_rate": ("G_rand", dict(cache_rate=0.5)),
    "deterministic_backward": ("G_rand", dict(deterministic_backward=False)),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_constructor_refusals_name_the_option(E, data, name):
    G, kw = REFUSALS[name]
    with pytest.raises(RuntimeError) as ei:
        _driver(E, data, G, edge_weighted=True, **kw)
    msg = str(ei.value).splitlines()[0]
    assert msg.startswith("edge_weighted is not supported with ") and name in msg, msg
    _driver(E, data, G, **kw)  # the same configuration without the option is accepted


def test_cfg_runner_cora_with_unit_coefficients_is_the_plain_job(tmp_path):
    from conftest import GOLDEN
    from nts import dataloader, run
    for f in ("cora.2708.edge.self", "cora.featuretable.zip", "cora.labeltable", "cora.mask"):
        shutil.copy(GOLDEN / "cora" / f, tmp_path / f)
    src, _ = dataloader.read_edge_file(tmp_path / "cora.2708.edge.self")
    dataloader.write_edge_weight_file(tmp_path / "ones.weight", np.ones(src.size, np.float32))
    text = (GOLDEN / "cora" / "gcn_cora_sample.cfg").read_text()
    (tmp_path / "plain.cfg").write_text(text + "FULL_INFERENCE:1\n")
    (tmp_path / "job.cfg").write_text(text + "EDGE_WEIGHT_FILE:ones.weight\nEDGE_WEIGHT_AGG:1\n"
                                      "FULL_INFERENCE:1\n")
    a = run.run(tmp_path / "job.cfg", epochs=2, out=lambda s: None)
    b = run.run(tmp_path / "plain.cfg", epochs=2, out=lambda s: None)
    assert [e["loss"] for e in a["epochs"]] == [e["loss"] for e in b["epochs"]]
    assert [e["test_acc"] for e in a["epochs"]] == [e["test_acc"] for e in b["epochs"]]
    assert a["full_test_acc"] == b["full_test_acc"]
    assert all(np.isfinite(e["loss"]) for e in a["epochs"])
