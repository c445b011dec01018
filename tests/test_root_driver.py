"""GraphSAGE root weight through the C++ driver (GCNConfig::root_weight): every
layer X' = act([A X | X_dst] W) with one stacked W, against the same chain in
torch float64 with autograd built from the trained batch's own arrays.

Bounds are the project's: one training step's weights rtol = atol = 1e-5 and
its loss rtol 1e-5 / atol 1e-6 (tests/test_host.py), forward outputs rtol =
atol = 1e-4 (tests/test_full_infer_driver.py).
"""
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LAYERS, FANOUT, BATCH = [32, 16, 8], [5, 5], 64
V = 2000


@pytest.fixture(scope="module")
def E():
    from nts import host
    return host.ext()


@pytest.fixture(scope="module")
def data(E):
    from nts import synthetic
    g = synthetic.chung_lu(V, 24000, 10.0, device=DEV, seed=3)
    G = E.FullyRepGraph.from_edges(g.src, g.dst, V)
    feat = synthetic.features(V, LAYERS[0], device=DEV)
    labels, masks = synthetic.labels_masks(V, LAYERS[-1], device=DEV)
    train = torch.nonzero(masks == 0).flatten().to(torch.int32).cpu()
    return dict(G=G, g=g, feat=feat, labels=labels, masks=masks, train=train)


def _driver(E, data, labels=None, **kw):
    from nts import host
    cfg = host.gcn_config(LAYERS, FANOUT, BATCH, learn_rate=0.01, drop_rate=0.0, shuffle=False, **kw)
    return E.GCN_SAMPLE_ALLGPU_impl(data["G"], data["feat"], data["labels"] if labels is None else labels,
                                    data["train"], cfg)


def _agg(lay, X):
    """A X of one sampled layer in X's dtype (autograd follows)"""
    co = lay["column_offset"].cpu().long()
    ri = lay["row_indices"].cpu().long()
    w = lay["edge_weight_forward"].cpu().to(X.dtype)
    d_of_e = torch.repeat_interleave(torch.arange(co.numel() - 1), co[1:] - co[:-1])
    return torch.zeros(co.numel() - 1, X.shape[1], dtype=X.dtype).index_add(0, d_of_e, X[ri] * w[:, None])


def _reference_step(drv, data, W0):
    top, bottom = drv.last_layers
    feat = data["feat"].cpu().double()
    W = [w.double().requires_grad_() for w in W0]
    X0 = feat[bottom["source"].cpu().long()]
    Ycat0 = torch.cat([_agg(bottom, X0), feat[bottom["destination"].cpu().long()]], 1)
    X1 = torch.relu(Ycat0 @ W[0])
    Ycat1 = torch.cat([_agg(top, X1), X1[top["dst_local_id"].cpu().long()]], 1)
    out = (Ycat1 @ W[1]).log_softmax(1)
    tgt = data["labels"].cpu()[top["destination"].cpu().long()]
    loss = torch.nn.functional.nll_loss(out.log_softmax(1), tgt)
    loss.backward()
    new = []
    for w0, w in zip(W0, W):  # learn_local_with_decay_Adam's first step
        wg = w0.double() * 1e-4 + w.grad
        m = 0.1 * wg
        v = (0.001 * wg) * wg
        new.append(w0.double() - (0.01 * m) / (torch.sqrt(v) + 1e-9))
    return float(loss.detach()), new


def test_weights_are_stacked(E, data):
    drv = _driver(E, data, root_weight=True)
    assert [tuple(w.shape) for w in drv.weights()] == [(64, 16), (32, 8)]
    assert not drv.transform_first


@pytest.mark.parametrize("early", [True, False], ids=["early", "late"])
@pytest.mark.parametrize("fuse_loss", [True, False], ids=["fused_loss", "torch_loss"])
@pytest.mark.parametrize("weight", ["sum", "mean"])
def test_one_training_step_matches_the_float64_chain(E, data, weight, fuse_loss, early):
    if fuse_loss:
        assert E.hip_linear_xent_supported(2 * LAYERS[-2], LAYERS[-1])
    drv = _driver(E, data, root_weight=True, weight=weight, fuse_loss=fuse_loss,
                  early_aggregate=early)
    W0 = [w.cpu().clone() for w in drv.weights()]
    drv.train_batch()
    drv.synchronize()
    top, bottom = drv.last_layers
    assert torch.equal(top["source"][top["dst_local_id"].long()], top["destination"])
    assert top["src_size"] > top["v_size"]  # sources that are no destinations
    loss, ref = _reference_step(drv, data, W0)
    got = float(drv.loss.detach())
    print(f"root {weight} fuse_loss={fuse_loss}: loss {got!r} vs float64 {loss!r}")
    torch.testing.assert_close(torch.tensor(got, dtype=torch.float64),
                               torch.tensor(loss, dtype=torch.float64),
                               rtol=1e-5, atol=1e-6)
    for w1, r in zip(drv.weights(), ref):
        print(f"  max |dW| {float((w1.cpu().double() - r).abs().max()):.3e}")
        torch.testing.assert_close(w1.cpu().double(), r, rtol=1e-5, atol=1e-5)


def _chain_grads(drv, data, W0, dtype):
    """the gradients of _reference_step's chain in `dtype`"""
    top, bottom = drv.last_layers
    feat = data["feat"].cpu().to(dtype)
    W = [w.to(dtype).requires_grad_() for w in W0]
    X0 = feat[bottom["source"].cpu().long()]
    X1 = torch.relu(torch.cat([_agg(bottom, X0), feat[bottom["destination"].cpu().long()]], 1) @ W[0])
    out = (torch.cat([_agg(top, X1), X1[top["dst_local_id"].cpu().long()]], 1) @ W[1]).log_softmax(1)
    tgt = data["labels"].cpu()[top["destination"].cpu().long()]
    torch.nn.functional.nll_loss(out.log_softmax(1), tgt).backward()
    return [w.grad for w in W]


@pytest.mark.parametrize("fuse_loss", [True, False], ids=["fused_loss", "torch_loss"])
@pytest.mark.parametrize("weight", ["sum", "mean"])
def test_one_training_step_gradients_keep_their_magnitude(E, data, weight, fuse_loss):
    """The step above moves each weight by lr * 3.16 * sign(gradient) (epsilon =
    1e-9): it checks signs.  Here the step reads the gradient out
    (tests/step_check.py) and both stacked weights' gradients are held to C
    times the float32 chain's own error of float64 autograd."""
    import step_check
    from nts import host
    cfg = step_check.readout(host.gcn_config(LAYERS, FANOUT, BATCH, drop_rate=0.0, shuffle=False,
                                             root_weight=True, weight=weight, fuse_loss=fuse_loss))
    drv = E.GCN_SAMPLE_ALLGPU_impl(data["G"], data["feat"], data["labels"], data["train"], cfg)
    W0 = [w.cpu().clone() for w in drv.weights()]
    drv.train_batch()
    drv.synchronize()
    W1 = [w.cpu().clone() for w in drv.weights()]
    g64 = _chain_grads(drv, data, W0, torch.float64)
    g32 = _chain_grads(drv, data, W0, torch.float32)
    print(f"root {weight} fuse_loss={fuse_loss}")
    step_check.check_step_grads(W0, W1, g64, g32, step_check.C)


def _full_reference(data, W, mean):
    g = data["g"]
    src, dst = g.src.cpu().long(), g.dst.cpu().long()
    od = torch.bincount(src, minlength=V).double()
    idg = torch.bincount(dst, minlength=V).double()
    w = 1.0 / (od[src].sqrt() * idg[dst].sqrt())
    if mean:
        w = w / idg[dst]
    A = torch.sparse_coo_tensor(torch.stack([dst, src]), w, (V, V)).coalesce()
    X = data["feat"].cpu().double()
    for l, wl in enumerate(W):
        Z = torch.cat([torch.sparse.mm(A, X), X], 1) @ wl.cpu().double()
        X = Z if l == len(W) - 1 else torch.relu(Z)
    return X


@pytest.mark.parametrize("weight", ["sum", "mean"])
def test_infer_full_matches_the_float64_chain(E, data, weight):
    drv = _driver(E, data, root_weight=True, weight=weight)
    for _ in range(2):
        drv.train_batch()
    out = drv.infer_full()
    assert tuple(out.shape) == (V, LAYERS[-1])
    ref = _full_reference(data, drv.weights(), weight == "mean").log_softmax(1)
    print(f"infer_full root {weight}: max |diff| {float((out.cpu().double() - ref).abs().max()):.3e}")
    torch.testing.assert_close(out.cpu().double(), ref, rtol=1e-4, atol=1e-4)
    assert torch.equal(out, drv.infer_full())


def test_forward_eval_uses_the_same_layers(E, data):
    drv = _driver(E, data, root_weight=True)
    seeds = torch.arange(3, 3 + 64 * 7, 7, dtype=torch.int32)
    acts = drv.forward_eval(seeds, 0)  # [Ycat_0, X_1, Ycat_1, X_2]
    assert [tuple(a.shape)[1] for a in acts] == [64, 16, 32, 8]
    W = [w.cpu().double() for w in drv.weights()]
    torch.testing.assert_close(acts[1].cpu().double(), torch.relu(acts[0].cpu().double() @ W[0]),
                               rtol=1e-4, atol=1e-4)
    # the self halves are rows of the layer's input: feature rows, rows of X_1
    feat_rows = {r.tobytes() for r in data["feat"].cpu().numpy()}
    assert all(r.tobytes() in feat_rows for r in acts[0][:, 32:].cpu().numpy())
    x1_rows = {r.tobytes() for r in acts[1].cpu().numpy()}
    assert all(r.tobytes() in x1_rows for r in acts[2][:, 16:].cpu().numpy())
    torch.testing.assert_close(acts[3].cpu().double(),
                               (acts[2].cpu().double() @ W[1]).log_softmax(1), rtol=1e-4, atol=1e-4)
    acc = drv.evaluate(torch.arange(0, 300, dtype=torch.int32))
    assert 0.0 <= acc <= 1.0


@pytest.mark.parametrize("pipeline", [True, False])
def test_infer_full_does_not_disturb_training(E, data, pipeline):
    a = _driver(E, data, root_weight=True, pipeline=pipeline)
    b = _driver(E, data, root_weight=True, pipeline=pipeline)
    ids = torch.nonzero(data["masks"].cpu() == 1).flatten().to(torch.int32)
    la, lb = [], []
    for step in range(6):
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


def test_training_is_deterministic_and_learns(E, data):
    a = _driver(E, data, root_weight=True, weight="mean")
    b = _driver(E, data, root_weight=True, weight="mean")
    la, lb = [], []
    for _ in range(12):
        for d, l in ((a, la), (b, lb)):
            d.train_batch()
            d.synchronize()
            l.append(float(d.loss.detach()))
    assert la == lb and all(np.isfinite(la))
    for x, y in zip(a.weights(), b.weights()):
        assert torch.equal(x, y)


def test_multi_label_with_root_weight(E, data):
    from nts import synthetic
    labels = synthetic.multilabels(V, LAYERS[-1], data["feat"], seed=13)
    drv = _driver(E, data, labels=labels, root_weight=True, multi_label=True)
    drv.train_batch()
    drv.synchronize()
    assert np.isfinite(float(drv.loss.detach()))
    ids = torch.nonzero(data["masks"].cpu() == 2).flatten().to(torch.int32)
    f1 = drv.evaluate_full(ids)
    assert 0.0 <= f1 <= 1.0


@pytest.mark.parametrize("kw,name", [
    (dict(gat=True), "gat"),
    (dict(pd_cache=True), "pd_cache"),
    (dict(sample_gpu=True, rng_mode=1), "sample_gpu"),
    (dict(transform_first=1), "transform_first"),
    (dict(pair_table=1), "pair_table"),
    (dict(cache_rate=0.5), "cache_rate"),
    (dict(fused_gather=False), "fused_gather"),
    (dict(deterministic_backward=False), "deterministic_backward"),
])
def test_refused_combinations_name_the_option(E, data, kw, name):
    with pytest.raises(RuntimeError, match="root_weight") as ei:
        _driver(E, data, root_weight=True, **kw)
    assert name in str(ei.value)
    assert str(ei.value).splitlines()[0] == REFUSALS[name]


# the constructor's refusals, whole (the first line of the error: libtorch appends its trace)
REFUSALS = {
    "gat": "root_weight is not supported with gat (GCN / GraphSAGE layers only)",
    "pd_cache": "root_weight is not supported with pd_cache",
    "sample_gpu": "root_weight is not supported with sample_gpu",
    "transform_first": "root_weight is not supported with transform_first = 1 (aggregate-first only)",
    "pair_table": "root_weight is not supported with pair_table > 0",
    "cache_rate": "root_weight is not supported with cache_rate >= 0",
    "fused_gather": "root_weight is not supported with fused_gather = false",
    "deterministic_backward": "root_weight needs deterministic_backward (its backward runs over the CSR)",
}


def test_cfg_runner_trains_with_root_weight(tmp_path):
    from conftest import GOLDEN
    from nts import run
    for f in ("cora.2708.edge.self", "cora.featuretable.zip", "cora.labeltable", "cora.mask"):
        shutil.copy(GOLDEN / "cora" / f, tmp_path / f)
    text = (GOLDEN / "cora" / "gcn_cora_sample.cfg").read_text()
    (tmp_path / "root.cfg").write_text(text + "ROOT_WEIGHT:1\n")
    lines = []
    res = run.run(tmp_path / "root.cfg", epochs=2, out=lines.append)
    assert len(res["epochs"]) == 2
    for e in res["epochs"]:
        assert 0.0 <= e["train_acc"] <= 1.0 and 0.0 <= e["test_acc"] <= 1.0
    assert res["epochs"][-1]["train_acc"] > 0.5  # it learns Cora from its own rows
    assert sum(l.startswith("Train Acc:") for l in lines) == 2
    for algo in ("GATSAMPLEALLGPU", "GCNSAMPLEPDCACHE", "GCNSAMPLEGPU"):
        (tmp_path / "bad.cfg").write_text(
            text.replace("ALGORITHM:GCNSAMPLEALLGPU", f"ALGORITHM:{algo}") + "ROOT_WEIGHT:1\n")
        with pytest.raises(SystemExit, match="not supported"):
            run.run(tmp_path / "bad.cfg", epochs=1, out=lambda s: None)


def test_default_is_unchanged(E, data):
    a = _driver(E, data, root_weight=False)
    b = _driver(E, data)
    assert [tuple(w.shape) for w in a.weights()] == [(32, 16), (16, 8)]
    for d in (a, b):
        d.train_batch()
        d.synchronize()
    assert float(a.loss.detach()) == float(b.loss.detach())
    for x, y in zip(a.weights(), b.weights()):
        assert torch.equal(x, y)
