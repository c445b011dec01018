"""GraphSAGE max aggregator through the C++ driver (GCNConfig::aggregator = 1):
every layer's graph op is Y[d] = max over d's sampled edges of X[src] per column,
against the same chain in torch float64 with autograd, built from the trained
batch's own arrays.  The chain picks each column's winner with numpy.argmax
(the first maximum, the kernel's tie rule) and gathers with those indices:
amax's backward would split ties.

Bounds are the project's (tests/test_root_driver.py): one training step's
weights rtol = atol = 1e-5 and its loss rtol 1e-5 / atol 1e-6, forward outputs
rtol = atol = 1e-4.  So that no fp32 / fp64 difference flips a winner, the
float64 chain itself must separate every positive maximum of the top hop from
the best value of another edge by more than 1e-4 (asserted; DATA_SEED was
picked so that the reference alone meets it).
"""
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LAYERS, FANOUT, BATCH = [32, 16, 8], [5, 5], 64
V = 2000
DATA_SEED = 9
GAP = 1e-4


@pytest.fixture(scope="module")
def E():
    from nts import host
    return host.ext()


@pytest.fixture(scope="module")
def data(E):
    return make_data(E, DATA_SEED)


def make_data(E, seed):
    from nts import synthetic
    g = synthetic.chung_lu(V, 24000, 10.0, device=DEV, seed=3)
    # no repeated (src, dst) pair: two edges of one column never carry the same row
    key = torch.unique(g.src.long() * V + g.dst.long())
    g = synthetic.SyntheticGraph(V, (key // V).to(torch.int32), (key % V).to(torch.int32))
    G = E.FullyRepGraph.from_edges(g.src, g.dst, V)
    feat = synthetic.features(V, LAYERS[0], device=DEV, seed=seed)
    labels, masks = synthetic.labels_masks(V, LAYERS[-1], device=DEV)
    train = torch.nonzero(masks == 0).flatten().to(torch.int32).cpu()
    return dict(G=G, g=g, feat=feat, labels=labels, masks=masks, train=train)


def _driver(E, data, labels=None, **kw):
    from nts import host
    cfg = host.gcn_config(LAYERS, FANOUT, BATCH, learn_rate=0.01, drop_rate=0.0, shuffle=False, **kw)
    return E.GCN_SAMPLE_ALLGPU_impl(data["G"], data["feat"], data["labels"] if labels is None else labels,
                                    data["train"], cfg)


def _winners(co, ri, Xn):
    """per (d, c): the source row of the first maximum of the column's edges
    (empty column: row 0 and has = False), and the gap of every positive
    maximum to the best value of another edge"""
    v, F = co.size - 1, Xn.shape[1]
    idx = np.zeros((v, F), np.int64)
    has = np.zeros(v, bool)
    gap = np.inf
    for d in range(v):
        e = ri[co[d]:co[d + 1]]
        if e.size == 0:
            continue
        seg = Xn[e]
        k = seg.argmax(0)
        idx[d] = e[k]
        has[d] = True
        if e.size > 1:
            top = np.sort(seg, 0)
            pos = top[-1] > 0
            if pos.any():
                gap = min(gap, float((top[-1] - top[-2])[pos].min()))
    return idx, has, gap


def _max_agg(lay, X):
    """the max aggregation of one sampled layer in X's dtype (autograd follows
    the gather), and the layer's gap"""
    co = lay["column_offset"].cpu().numpy().astype(np.int64)
    ri = lay["row_indices"].cpu().numpy().astype(np.int64)
    idx, has, gap = _winners(co, ri, X.detach().numpy())
    F = X.shape[1]
    Y = X[torch.from_numpy(idx), torch.arange(F)[None, :]] * torch.from_numpy(has)[:, None].to(X.dtype)
    return Y, gap


def reference_step(drv, data, W0, root):
    top, bottom = drv.last_layers
    feat = data["feat"].cpu().double()
    W = [w.double().requires_grad_() for w in W0]
    X0 = feat[bottom["source"].cpu().long()]
    Y0, _ = _max_agg(bottom, X0)
    if root:
        Y0 = torch.cat([Y0, feat[bottom["destination"].cpu().long()]], 1)
    X1 = torch.relu(Y0 @ W[0])
    Y1, gap = _max_agg(top, X1)
    if root:
        Y1 = torch.cat([Y1, X1[top["dst_local_id"].cpu().long()]], 1)
    out = (Y1 @ W[1]).log_softmax(1)
    tgt = data["labels"].cpu()[top["destination"].cpu().long()]
    loss = torch.nn.functional.nll_loss(out.log_softmax(1), tgt)
    loss.backward()
    new = []
    for w0, w in zip(W0, W):  # learn_local_with_decay_Adam's first step
        wg = w0.double() * 1e-4 + w.grad
        m = 0.1 * wg
        v = (0.001 * wg) * wg
        new.append(w0.double() - (0.01 * m) / (torch.sqrt(v) + 1e-9))
    return float(loss.detach()), new, gap


@pytest.mark.parametrize("fuse_loss", [True, False], ids=["fused_loss", "torch_loss"])
@pytest.mark.parametrize("root", [False, True], ids=["plain", "root_weight"])
def test_one_training_step_matches_the_float64_chain(E, data, root, fuse_loss):
    drv = _driver(E, data, aggregator="max", root_weight=root, fuse_loss=fuse_loss)
    assert not drv.transform_first
    W0 = [w.cpu().clone() for w in drv.weights()]
    assert [tuple(w.shape) for w in W0] == ([(64, 16), (32, 8)] if root else [(32, 16), (16, 8)])
    drv.train_batch()
    drv.synchronize()
    loss, ref, gap = reference_step(drv, data, W0, root)
    print(f"max root={root} fuse_loss={fuse_loss}: top-hop gap {gap:.3e}")
    assert gap > GAP, "the reference's winners are too close: pick another DATA_SEED"
    got = float(drv.loss.detach())
    print(f"  loss {got!r} vs float64 {loss!r}")
    torch.testing.assert_close(torch.tensor(got, dtype=torch.float64),
                               torch.tensor(loss, dtype=torch.float64), rtol=1e-5, atol=1e-6)
    for w1, r in zip(drv.weights(), ref):
        print(f"  max |dW| {float((w1.cpu().double() - r).abs().max()):.3e}")
        torch.testing.assert_close(w1.cpu().double(), r, rtol=1e-5, atol=1e-5)


def _chain_grads(drv, data, W0, root, dtype):
    """the gradients of reference_step's chain in `dtype`, and its top-hop gap"""
    top, bottom = drv.last_layers
    feat = data["feat"].cpu().to(dtype)
    W = [w.to(dtype).requires_grad_() for w in W0]
    X0 = feat[bottom["source"].cpu().long()]
    Y0, _ = _max_agg(bottom, X0)
    if root:
        Y0 = torch.cat([Y0, feat[bottom["destination"].cpu().long()]], 1)
    X1 = torch.relu(Y0 @ W[0])
    Y1, gap = _max_agg(top, X1)
    if root:
        Y1 = torch.cat([Y1, X1[top["dst_local_id"].cpu().long()]], 1)
    out = (Y1 @ W[1]).log_softmax(1)
    tgt = data["labels"].cpu()[top["destination"].cpu().long()]
    torch.nn.functional.nll_loss(out.log_softmax(1), tgt).backward()
    return [w.grad for w in W], gap


@pytest.mark.parametrize("root", [False, True], ids=["plain", "root_weight"])
def test_one_training_step_gradients_keep_their_magnitude(E, data, root):
    """The step above moves each weight by lr * 3.16 * sign(gradient) (epsilon =
    1e-9): it checks signs.  Here the step reads the gradient out
    (tests/step_check.py) and both weights' gradients are held to C times the
    float32 chain's own error of float64 autograd (same winners: the gap is
    asserted as above)."""
    import step_check
    from nts import host
    cfg = step_check.readout(host.gcn_config(LAYERS, FANOUT, BATCH, drop_rate=0.0, shuffle=False,
                                             aggregator="max", root_weight=root))
    drv = E.GCN_SAMPLE_ALLGPU_impl(data["G"], data["feat"], data["labels"], data["train"], cfg)
    W0 = [w.cpu().clone() for w in drv.weights()]
    drv.train_batch()
    drv.synchronize()
    W1 = [w.cpu().clone() for w in drv.weights()]
    g64, gap = _chain_grads(drv, data, W0, root, torch.float64)
    g32, _ = _chain_grads(drv, data, W0, root, torch.float32)
    print(f"max root={root}: top-hop gap {gap:.3e}")
    assert gap > GAP, "the reference's winners are too close: pick another DATA_SEED"
    step_check.check_step_grads(W0, W1, g64, g32, step_check.C)


def _full_reference(data, W, root):
    g = data["g"]
    src, dst = g.src.cpu().numpy().astype(np.int64), g.dst.cpu().numpy().astype(np.int64)
    order = np.argsort(dst, kind="stable")
    ri = src[order]
    co = np.zeros(V + 1, np.int64)
    co[1:] = np.cumsum(np.bincount(dst, minlength=V))
    X = data["feat"].cpu().double().numpy()
    for l, wl in enumerate(W):
        Y = np.zeros_like(X)
        for d in range(V):
            if co[d + 1] > co[d]:
                Y[d] = X[ri[co[d]:co[d + 1]]].max(0)
        Z = (np.concatenate([Y, X], 1) if root else Y) @ wl.cpu().double().numpy()
        X = Z if l == len(W) - 1 else np.maximum(Z, 0.0)
    return torch.from_numpy(X)


@pytest.mark.parametrize("root", [False, True], ids=["plain", "root_weight"])
def test_infer_full_matches_the_float64_chain(E, data, root):
    drv = _driver(E, data, aggregator="max", root_weight=root)
    for _ in range(2):
        drv.train_batch()
    out = drv.infer_full()
    assert tuple(out.shape) == (V, LAYERS[-1])
    ref = _full_reference(data, drv.weights(), root).log_softmax(1)
    print(f"infer_full max root={root}: max |diff| {float((out.cpu().double() - ref).abs().max()):.3e}")
    torch.testing.assert_close(out.cpu().double(), ref, rtol=1e-4, atol=1e-4)
    assert torch.equal(out, drv.infer_full())


@pytest.mark.parametrize("root", [False, True], ids=["plain", "root_weight"])
def test_forward_eval_widths(E, data, root):
    drv = _driver(E, data, aggregator="max", root_weight=root)
    seeds = torch.arange(3, 3 + 64 * 7, 7, dtype=torch.int32)
    acts = drv.forward_eval(seeds, 0)  # [Y_0, X_1, Y_1, X_2]
    assert [tuple(a.shape)[1] for a in acts] == ([64, 16, 32, 8] if root else [32, 16, 16, 8])
    W = [w.cpu().double() for w in drv.weights()]
    torch.testing.assert_close(acts[1].cpu().double(), torch.relu(acts[0].cpu().double() @ W[0]),
                               rtol=1e-4, atol=1e-4)
    # every value of a max row is a value of the layer's input, column by column
    feat = data["feat"].cpu().numpy()
    y0 = acts[0][:, :32].cpu().numpy()
    for c in range(0, 32, 5):
        assert np.isin(y0[:, c], np.append(feat[:, c], np.float32(0))).all()
    acc = drv.evaluate(torch.arange(0, 300, dtype=torch.int32))
    assert 0.0 <= acc <= 1.0


@pytest.mark.parametrize("pipeline", [True, False])
def test_infer_full_does_not_disturb_training(E, data, pipeline):
    a = _driver(E, data, aggregator="max", pipeline=pipeline)
    b = _driver(E, data, aggregator="max", pipeline=pipeline)
    ids = torch.nonzero(data["masks"].cpu() == 1).flatten().to(torch.int32)
    la, lb = [], []
    for step in range(6):
        if step == 2:
            a.infer_full()
        if step == 3:
            assert 0.0 <= a.evaluate_full(ids) <= 1.0
        a.train_batch()
        a.synchronize()
        la.append(float(a.loss.detach()))
        b.train_batch()
        b.synchronize()
        lb.append(float(b.loss.detach()))
    assert la == lb
    for x, y in zip(a.weights(), b.weights()):
        assert torch.equal(x, y)


def test_training_is_deterministic(E, data):
    a = _driver(E, data, aggregator="max")
    b = _driver(E, data, aggregator="max")
    la, lb = [], []
    for _ in range(12):
        for d, l in ((a, la), (b, lb)):
            d.train_batch()
            d.synchronize()
            l.append(float(d.loss.detach()))
    assert la == lb and all(np.isfinite(la))
    for x, y in zip(a.weights(), b.weights()):
        assert torch.equal(x, y)


def test_multi_label_with_max(E, data):
    from nts import synthetic
    labels = synthetic.multilabels(V, LAYERS[-1], data["feat"], seed=13)
    drv = _driver(E, data, labels=labels, aggregator="max", multi_label=True)
    drv.train_batch()
    drv.synchronize()
    assert np.isfinite(float(drv.loss.detach()))
    ids = torch.nonzero(data["masks"].cpu() == 2).flatten().to(torch.int32)
    assert 0.0 <= drv.evaluate_full(ids) <= 1.0


@pytest.mark.parametrize("kw,name", [
    (dict(gat=True), "gat"),
    (dict(pd_cache=True), "pd_cache"),
    (dict(sample_gpu=True, rng_mode=1), "sample_gpu"),
    (dict(transform_first=1), "transform_first"),
    (dict(pair_table=1), "pair_table"),
    (dict(cache_rate=0.5), "cache_rate"),
    (dict(fused_gather=False), "fused_gather"),
    (dict(deterministic_backward=False), "deterministic_backward"),
    (dict(up_degree=True), "up_degree"),
])
def test_refused_combinations_name_the_option(E, data, kw, name):
    with pytest.raises(RuntimeError, match="aggregator") as ei:
        _driver(E, data, aggregator="max", **kw)
    assert name in str(ei.value)
    assert str(ei.value).splitlines()[0] == REFUSALS[name]


# the constructor's refusals, whole (the first line of the error: libtorch appends its trace)
REFUSALS = {
    "gat": "aggregator = max is not supported with gat (GCN / GraphSAGE layers only)",
    "pd_cache": "aggregator = max is not supported with pd_cache",
    "sample_gpu": "aggregator = max is not supported with sample_gpu",
    "transform_first": "aggregator = max is not supported with transform_first = 1 (a maximum does not "
                       "commute with W: aggregate-first only)",
    "pair_table": "aggregator = max is not supported with pair_table > 0",
    "cache_rate": "aggregator = max is not supported with cache_rate >= 0",
    "fused_gather": "aggregator = max is not supported with fused_gather = false",
    "deterministic_backward": "aggregator = max needs deterministic_backward (its backward runs over "
                              "the CSR)",
    "up_degree": "aggregator = max is not supported with up_degree (it takes no edge weights)",
}


def test_sum_is_the_default(E, data):
    a = _driver(E, data, aggregator="sum")
    b = _driver(E, data)
    for d in (a, b):
        for _ in range(3):
            d.train_batch()
        d.synchronize()
    assert float(a.loss.detach()) == float(b.loss.detach())
    for x, y in zip(a.weights(), b.weights()):
        assert torch.equal(x, y)


def test_cfg_runner_trains_with_the_max_aggregator(tmp_path):
    from conftest import GOLDEN
    from nts import run
    for f in ("cora.2708.edge.self", "cora.featuretable.zip", "cora.labeltable", "cora.mask"):
        shutil.copy(GOLDEN / "cora" / f, tmp_path / f)
    text = (GOLDEN / "cora" / "gcn_cora_sample.cfg").read_text()
    (tmp_path / "max.cfg").write_text(text + "AGGREGATOR:max\n")
    lines = []
    res = run.run(tmp_path / "max.cfg", epochs=2, out=lines.append)
    assert len(res["epochs"]) == 2
    for e in res["epochs"]:
        assert 0.0 <= e["train_acc"] <= 1.0 and 0.0 <= e["test_acc"] <= 1.0
    assert res["epochs"][-1]["train_acc"] > 0.5
    for algo in ("GATSAMPLEALLGPU", "GCNSAMPLEPDCACHE", "GCNSAMPLEGPU"):
        (tmp_path / "bad.cfg").write_text(
            text.replace("ALGORITHM:GCNSAMPLEALLGPU", f"ALGORITHM:{algo}") + "AGGREGATOR:max\n")
        with pytest.raises(SystemExit, match="not supported"):
            run.run(tmp_path / "bad.cfg", epochs=1, out=lambda s: None)
