"""LayerNorm on the hidden layers through the C++ driver (GCNConfig::layer_norm):
every hidden layer is dropout(relu(LayerNorm((A X) W; gamma, beta))) from the
fused kernels, against the same chain in torch (float64 autograd, float32 as
the yardstick) built from the trained batch's own arrays.

The graph and data are tests/test_max_driver.py's (V = 2000, layers [32, 16, 8],
fanout [5, 5], batch 64, drop_rate 0, no shuffle); a three-layer model
[32, 16, 16, 8] exercises two LayerNorm layers.  gamma and beta are set to
1 + 0.1 randn and 0.1 randn so that their gradients are not degenerate.

Gradients: one readout step (tests/step_check.py), every W, gamma and beta held
to C times the float32 chain's own error.  Forward outputs: rtol = atol = 1e-4,
the project's forward bound.  For the max aggregator the float64 chain must
separate every positive maximum of the top hop from the runner-up by more than
tests/test_max_driver.py's GAP; the seed of gamma / beta is the first of a few
whose float64 chain does (the reference alone decides).
"""
import pytest
import torch

import step_check
import test_max_driver as tmd
from test_root_driver import _agg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
V = tmd.V
L2, F2 = [32, 16, 8], [5, 5]
L3, F3 = [32, 16, 16, 8], [5, 5, 5]
BATCH = 64
EPS = 1e-5


@pytest.fixture(scope="module")
def E():
    from nts import host
    return host.ext()


@pytest.fixture(scope="module")
def data(E):
    return tmd.make_data(E, tmd.DATA_SEED)


def _cfg(layers=L2, fanout=F2, **kw):
    from nts import host
    kw.setdefault("drop_rate", 0.0)
    return host.gcn_config(layers, fanout, BATCH, learn_rate=0.01, shuffle=False, **kw)


def _driver(E, data, cfg, labels=None, comm=None):
    args = (data["G"], data["feat"], data["labels"] if labels is None else labels, data["train"], cfg)
    return E.GCN_SAMPLE_ALLGPU_impl(*args) if comm is None else E.GCN_SAMPLE_ALLGPU_impl(*args, comm)


def _nontrivial(drv, seed):
    """the driver's weights with gamma = 1 + 0.1 randn, beta = 0.1 randn"""
    ws = [w.cpu().clone() for w in drv.weights()]
    L = (len(ws) + 2) // 3
    g = torch.Generator().manual_seed(seed)
    for i in range(L, len(ws)):
        r = 0.1 * torch.randn(ws[i].shape, generator=g)
        ws[i] = 1 + r if (i - L) % 2 == 0 else r
    return ws


def _ln(Z, gamma, beta):
    """LayerNorm over the columns of Z (the expression of every chain here)"""
    return torch.nn.functional.layer_norm(Z, (Z.shape[1],), gamma, beta, EPS)


def _chain(lays, data, ws, dtype, root=False, mx=False, labels=None):
    """the model over the sampled layers `lays` (top first) in `dtype`; returns
    (parameters, loss, hidden outputs, gap of the top hop's maxima)"""
    L = len(lays)
    feat = data["feat"].cpu().to(dtype)
    P = [w.to(dtype).requires_grad_() for w in ws]
    X, gap, hidden = feat[lays[-1]["source"].cpu().long()], None, []
    for l in range(L):
        lay = lays[L - 1 - l]
        if mx:
            Y, gap = tmd._max_agg(lay, X)
        else:
            Y = _agg(lay, X)
        if root:
            own = feat[lay["destination"].cpu().long()] if l == 0 else X[lay["dst_local_id"].cpu().long()]
            Y = torch.cat([Y, own], 1)
        Z = Y @ P[l]
        if l < L - 1:
            X = torch.relu(_ln(Z, P[L + 2 * l], P[L + 2 * l + 1]))
            hidden.append(X)
    dst = lays[0]["destination"].cpu().long()
    if labels is None:
        loss = torch.nn.functional.nll_loss(Z.log_softmax(1), data["labels"].cpu()[dst])
    else:
        loss = torch.nn.functional.binary_cross_entropy_with_logits(Z, labels.cpu()[dst].to(dtype))
    return P, loss, hidden, gap


def _same_layers(a, b):
    return all(torch.equal(x[k], y[k]) for x, y in zip(a, b)
               for k in ("column_offset", "row_indices", "source", "destination"))


CASES = {
    "sum": (L2, F2, {}),
    "sum-3-layers": (L3, F3, {}),
    "root_weight": (L2, F2, dict(root_weight=True)),
    "root_weight-3-layers": (L3, F3, dict(root_weight=True)),
    "max": (L2, F2, dict(aggregator="max")),
    "multi_label": (L2, F2, dict(multi_label=True)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_one_step_gradients_of_every_parameter(E, data, case):
    from nts import synthetic
    layers, fanout, kw = CASES[case]
    root, mx = bool(kw.get("root_weight")), kw.get("aggregator") == "max"
    labels = synthetic.multilabels(V, layers[-1], data["feat"], seed=13) if kw.get("multi_label") else None
    L = len(layers) - 1

    def build():
        return _driver(E, data, step_check.readout(_cfg(layers, fanout, layer_norm=True, **kw)), labels)

    seed = 1
    if mx:  # the batch is the same for every weight: sample it once, pick the seed on float64 alone
        probe = build()
        probe.train_batch()
        probe.synchronize()
        for seed in range(1, 9):
            gap = _chain(probe.last_layers, data, _nontrivial(probe, seed), torch.float64, root, mx)[3]
            if gap > tmd.GAP:
                break
    drv = build()
    assert not drv.transform_first
    W0 = _nontrivial(drv, seed)
    assert len(W0) == L + 2 * (L - 1)
    assert [tuple(w.shape) for w in W0[L:]] == [(layers[l + 1],) for l in range(L - 1) for _ in (0, 1)]
    drv.set_weights([w.to(DEV) for w in W0])
    drv.train_batch()
    drv.synchronize()
    W1 = [w.cpu().clone() for w in drv.weights()]
    lays = drv.last_layers
    if mx:
        assert _same_layers(lays, probe.last_layers)
    grads = {}
    for dtype in (torch.float64, torch.float32):
        P, loss, _, gap = _chain(lays, data, W0, dtype, root, mx, labels)
        loss.backward()
        grads[dtype] = [p.grad for p in P]
        if mx and dtype == torch.float64:
            print(f"max: top-hop gap {gap:.3e} (seed {seed})")
            assert gap > tmd.GAP, "the reference's winners are too close"
    names = [f"W[{l}]" for l in range(L)] + [f"{n}[{l}]" for l in range(L - 1) for n in ("gamma", "beta")]
    print(f"layer_norm {case}")
    step_check.check_step_grads(W0, W1, grads[torch.float64], grads[torch.float32], step_check.C, names)


@pytest.mark.parametrize("layers,fanout", [(L2, F2), (L3, F3)], ids=["2-layers", "3-layers"])
def test_forward_eval_matches_the_float64_chain(E, data, layers, fanout):
    drv = _driver(E, data, _cfg(layers, fanout, layer_norm=True))
    drv.set_weights([w.to(DEV) for w in _nontrivial(drv, 2)])
    ws = [w.cpu().double() for w in drv.weights()]
    L = len(layers) - 1
    acts = drv.forward_eval(torch.arange(3, 3 + 64 * 7, 7, dtype=torch.int32), 0)  # [Y_0, X_1, Y_1, ...]
    assert len(acts) == 2 * L
    for l in range(L - 1):
        Z = acts[2 * l].cpu().double() @ ws[l]
        ref = torch.relu(torch.nn.functional.layer_norm(Z, (Z.shape[1],), ws[L + 2 * l], ws[L + 2 * l + 1], EPS))
        print(f"forward_eval layer {l}: max |diff| {float((acts[2 * l + 1].cpu().double() - ref).abs().max()):.3e}")
        torch.testing.assert_close(acts[2 * l + 1].cpu().double(), ref, rtol=1e-4, atol=1e-4)
    assert 0.0 <= drv.evaluate(torch.arange(0, 300, dtype=torch.int32)) <= 1.0


def _full_reference(data, ws, L):
    g = data["g"]
    src, dst = g.src.cpu().long(), g.dst.cpu().long()
    od = torch.bincount(src, minlength=V).double()
    idg = torch.bincount(dst, minlength=V).double()
    A = torch.sparse_coo_tensor(torch.stack([dst, src]), 1.0 / (od[src].sqrt() * idg[dst].sqrt()),
                                (V, V)).coalesce()
    X = data["feat"].cpu().double()
    for l in range(L):
        Z = torch.sparse.mm(A, X) @ ws[l]
        X = Z if l == L - 1 else torch.relu(
            torch.nn.functional.layer_norm(Z, (Z.shape[1],), ws[L + 2 * l], ws[L + 2 * l + 1], EPS))
    return X.log_softmax(1)


# infer_full() forms a narrowing hidden layer's product as A (X W) and a
# widening one's ([32, 48, 8]) as (A X) W: LayerNorm follows either
@pytest.mark.parametrize("layers,fanout", [(L2, F2), (L3, F3), ([32, 48, 8], F2)],
                         ids=["2-layers", "3-layers", "widening"])
def test_infer_full_matches_the_float64_chain(E, data, layers, fanout):
    drv = _driver(E, data, _cfg(layers, fanout, layer_norm=True))
    drv.set_weights([w.to(DEV) for w in _nontrivial(drv, 3)])
    for _ in range(2):
        drv.train_batch()
    L = len(layers) - 1
    out = drv.infer_full()
    ref = _full_reference(data, [w.cpu().double() for w in drv.weights()], L)
    print(f"infer_full {layers}: max |diff| {float((out.cpu().double() - ref).abs().max()):.3e}")
    torch.testing.assert_close(out.cpu().double(), ref, rtol=1e-4, atol=1e-4)
    assert torch.equal(out, drv.infer_full())
    ids = torch.nonzero(data["masks"].cpu() == 1).flatten()
    acc = float((ref[ids].argmax(1) == data["labels"].cpu()[ids]).double().mean())
    assert drv.evaluate_full(ids.to(torch.int32)) == acc


def test_norm_parameters_are_not_decayed(E, data):
    cfg = _cfg(layer_norm=True, weight_decay=0.1)
    cfg.epsilon = 1.0
    drv = _driver(E, data, cfg)
    ws = _nontrivial(drv, 4)
    ws[1] = torch.zeros_like(ws[1])  # no gradient reaches layer 0: only the decay could move it
    drv.set_weights([w.to(DEV) for w in ws])
    drv.train_batch()
    drv.synchronize()
    after = [w.cpu() for w in drv.weights()]
    assert torch.equal(after[2], ws[2]) and torch.equal(after[3], ws[3])
    assert not torch.equal(after[0], ws[0])  # W_0 is decayed


def _steps(drv, n=3):
    for _ in range(n):
        drv.train_batch()
    drv.synchronize()
    return [w.cpu() for w in drv.weights()]


def test_overlapped_allreduce_carries_gamma_and_beta(E, data):
    from nts import dist as ndist
    comm = ndist.make_host_communicator(E, 1, 0, lambda t, op, root: None)
    a = _steps(_driver(E, data, _cfg(L3, F3, layer_norm=True, overlap_allreduce=1), comm=comm))
    b = _steps(_driver(E, data, _cfg(L3, F3, layer_norm=True)))
    assert len(a) == len(b) == 7
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[3], torch.ones_like(a[3]))  # gamma_0 was trained


def test_dropout_runs_are_deterministic(E, data):
    a = _steps(_driver(E, data, _cfg(layer_norm=True, drop_rate=0.5)))
    b = _steps(_driver(E, data, _cfg(layer_norm=True, drop_rate=0.5)))
    c = _steps(_driver(E, data, _cfg(layer_norm=True, drop_rate=0.0)))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not all(torch.equal(x, y) for x, y in zip(a, c))


def test_off_is_the_default(E, data):
    a = _driver(E, data, _cfg(layer_norm=False))
    b = _driver(E, data, _cfg())
    assert len(a.weights()) == 2
    for x, y in zip(_steps(a), _steps(b)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("weight,kw", [("mean", dict(up_degree=True)), ("sum", dict(cache_rate=0.5)),
                                       ("sum", dict(pipeline=False)), ("sum", dict(early_aggregate=False))],
                         ids=["mean-up_degree", "cache_rate", "no-pipeline", "late-aggregate"])
def test_trains_with_the_other_options(E, data, weight, kw):
    drv = _driver(E, data, _cfg(layer_norm=True, weight=weight, **kw))
    ws = _steps(drv)
    assert all(bool(torch.isfinite(w).all()) for w in ws)
    assert bool(torch.isfinite(drv.loss.detach()).item())


REFUSALS = {
    "gat": (dict(gat=True, weight="none"), L2,
            "layer_norm is not supported with gat (GCN / GraphSAGE layers only)"),
    "pd_cache": (dict(pd_cache=True), L2, "layer_norm is not supported with pd_cache"),
    "transform_first": (dict(transform_first=1), L2,
                        "layer_norm is not supported with transform_first = 1 (LayerNorm does not "
                        "commute with A: aggregate-first only)"),
    "pair_table": (dict(pair_table=1), L2, "layer_norm is not supported with pair_table > 0"),
    "width": ({}, [32, 1028, 8],
              "layer_norm is not supported with a hidden width above 1024 (layer 0: 1028)"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refused_combinations(E, data, name):
    kw, layers, text = REFUSALS[name]
    with pytest.raises(RuntimeError, match="layer_norm") as ei:
        _driver(E, data, _cfg(layers, F2, layer_norm=True, **kw))
    assert str(ei.value).splitlines()[0] == text


def test_auto_order_resolves_to_aggregate_first(E):
    from nts import synthetic
    g = synthetic.chung_lu(V, 24000, 10.0, device=DEV, seed=3)
    G = E.FullyRepGraph.from_edges(g.src, g.dst, V)
    feat = synthetic.features(V, 64, device=DEV)
    labels, masks = synthetic.labels_masks(V, 8, device=DEV)
    train = torch.nonzero(masks == 0).flatten().to(torch.int32).cpu()
    on = E.GCN_SAMPLE_ALLGPU_impl(G, feat, labels, train, _cfg([64, 16, 8], F2, layer_norm=True))
    off = E.GCN_SAMPLE_ALLGPU_impl(G, feat, labels, train, _cfg([64, 16, 8], F2))
    assert not on.transform_first and off.transform_first
    on.train_batch()
    on.synchronize()
    assert bool(torch.isfinite(on.loss.detach()).item())
