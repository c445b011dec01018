"""BatchNorm on the hidden layers through the C++ driver (GCNConfig::batch_norm):
every hidden layer is dropout(relu(BatchNorm((A X) W; gamma, beta))) from the
fused kernels, against the same chain in torch (float64 autograd, float32 as
the yardstick) built from the trained batch's own arrays.

Graph, data and models are tests/test_layer_norm_driver.py's (V = 2000, layers
[32, 16, 8] and [32, 16, 16, 8], fanout 5, batch 64, drop_rate 0, no shuffle).
gamma and beta are set to 1 + 0.1 randn and 0.1 randn.

Bound: tests/step_check.py's rule everywhere, err(driver) <= C err(float32
chain) + FLOOR against float64 (gradients through the one-step readout, with
its resolution).  Training uses the batch's statistics; evaluate(),
forward_eval() and infer_full() the running ones, which they leave alone.
"""
import shutil

import pytest
import torch

import step_check
import test_layer_norm_driver as tld
import test_max_driver as tmd
from step_check import C, err, yardstick_bound
from test_root_driver import _agg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
V = tmd.V
L2, F2, L3, F3, BATCH = tld.L2, tld.F2, tld.L3, tld.F3, tld.BATCH
EPS, MOM = 1e-5, 0.1
E, data = tld.E, tld.data  # the module-scoped fixtures
_driver, _nontrivial, _steps = tld._driver, tld._nontrivial, tld._steps


def _cfg(layers=L2, fanout=F2, **kw):
    kw.setdefault("batch_norm", True)
    return tld._cfg(layers, fanout, **kw)


def _bn(Z, g, b, rm, rv, train):
    return torch.batch_norm(Z, g, b, rm, rv, train, MOM, EPS, False)


def _chain(lays, data, ws, stats, dtype, train, root=False, mx=False, labels=None):
    """the model over the sampled layers `lays` (top first) in `dtype`; returns
    (parameters, loss, hidden outputs, buffers after the pass, top-hop gap)"""
    L = len(lays)
    feat = data["feat"].cpu().to(dtype)
    P = [w.to(dtype).requires_grad_() for w in ws]
    st = [s.cpu().to(dtype).clone() for s in stats]
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
            X = torch.relu(_bn(Z, P[L + 2 * l], P[L + 2 * l + 1], st[2 * l], st[2 * l + 1], train))
            hidden.append(X)
    dst = lays[0]["destination"].cpu().long()
    if labels is None:
        loss = torch.nn.functional.nll_loss(Z.log_softmax(1), data["labels"].cpu()[dst])
    else:
        loss = torch.nn.functional.binary_cross_entropy_with_logits(Z, labels.cpu()[dst].to(dtype))
    return P, loss, hidden, st, gap


def _hold(name, x, r64, r32, bad):
    ek, e32 = err(x, r64), err(r32, r64)
    bound = yardstick_bound(e32, C)
    print(f"  {name}: err(driver) {ek:.3e} err(fp32 chain) {e32:.3e} "
          f"ratio {ek / max(e32, 2.0 ** -30):.2f} bound {bound:.3e}")
    if not ek <= bound:
        bad.append(f"{name}: {ek:.3e} > {bound:.3e}")


@pytest.mark.parametrize("case", list(tld.CASES))
def test_one_step_gradients_and_buffers(E, data, case):
    from nts import synthetic
    layers, fanout, kw = tld.CASES[case]
    root, mx = bool(kw.get("root_weight")), kw.get("aggregator") == "max"
    labels = synthetic.multilabels(V, layers[-1], data["feat"], seed=13) if kw.get("multi_label") else None
    L = len(layers) - 1

    def build():
        return _driver(E, data, step_check.readout(_cfg(layers, fanout, **kw)), labels)

    seed = 1
    if mx:  # sample the batch once, pick the seed of gamma / beta on float64 alone
        probe = build()
        probe.train_batch()
        probe.synchronize()
        for seed in range(1, 9):
            gap = _chain(probe.last_layers, data, _nontrivial(probe, seed), probe_stats(L, layers),
                         torch.float64, True, root, mx)[4]
            if gap > tmd.GAP:
                break
    drv = build()
    assert not drv.transform_first
    W0 = _nontrivial(drv, seed)
    assert len(W0) == L + 2 * (L - 1)
    S0 = drv.norm_stats()
    assert [tuple(s.shape) for s in S0] == [(layers[l + 1],) for l in range(L - 1) for _ in (0, 1)]
    for l in range(L - 1):
        assert float(S0[2 * l].abs().max()) == 0.0 and bool((S0[2 * l + 1] == 1).all())
    drv.set_weights([w.to(DEV) for w in W0])
    drv.train_batch()
    drv.synchronize()
    W1 = [w.cpu().clone() for w in drv.weights()]
    S1 = [s.cpu() for s in drv.norm_stats()]
    lays = drv.last_layers
    grads, stats = {}, {}
    for dtype in (torch.float64, torch.float32):
        P, loss, _, st, gap = _chain(lays, data, W0, S0, dtype, True, root, mx, labels)
        loss.backward()
        grads[dtype], stats[dtype] = [p.grad for p in P], st
        if mx and dtype == torch.float64:
            assert gap > tmd.GAP, "the reference's winners are too close"
    names = [f"W[{l}]" for l in range(L)] + [f"{n}[{l}]" for l in range(L - 1) for n in ("gamma", "beta")]
    print(f"batch_norm {case}")
    step_check.check_step_grads(W0, W1, grads[torch.float64], grads[torch.float32], C, names)
    bad = []
    for i, s in enumerate(S1):
        _hold(f"{('running_mean', 'running_var')[i % 2]}[{i // 2}]", s, stats[torch.float64][i],
              stats[torch.float32][i], bad)
    assert not bad, "; ".join(bad)


def probe_stats(L, layers):
    return [torch.full((layers[l + 1],), float(i)) for l in range(L - 1) for i in (0, 1)]


@pytest.mark.parametrize("layers,fanout", [(L2, F2), (L3, F3)], ids=["2-layers", "3-layers"])
def test_eval_reads_the_running_statistics(E, data, layers, fanout):
    drv = _driver(E, data, _cfg(layers, fanout))
    drv.set_weights([w.to(DEV) for w in _nontrivial(drv, 2)])
    _steps(drv)
    ws, st = [w.cpu() for w in drv.weights()], [s.cpu() for s in drv.norm_stats()]
    assert not torch.equal(st[0], torch.zeros_like(st[0]))  # training moved them
    L = len(layers) - 1
    acts = drv.forward_eval(torch.arange(3, 3 + 64 * 7, 7, dtype=torch.int32), 0)  # [Y_0, X_1, Y_1, ...]
    assert len(acts) == 2 * L
    bad = []
    for l in range(L - 1):
        ref = {}
        for dtype in (torch.float64, torch.float32):
            Z = acts[2 * l].cpu().to(dtype) @ ws[l].to(dtype)
            ref[dtype] = torch.relu(_bn(Z, ws[L + 2 * l].to(dtype), ws[L + 2 * l + 1].to(dtype),
                                        st[2 * l].to(dtype), st[2 * l + 1].to(dtype), False))
        _hold(f"forward_eval X[{l + 1}]", acts[2 * l + 1].cpu(), ref[torch.float64], ref[torch.float32], bad)
    assert not bad, "; ".join(bad)
    assert 0.0 <= drv.evaluate(torch.arange(0, 300, dtype=torch.int32)) <= 1.0
    for a, b in zip(st, drv.norm_stats()):
        assert torch.equal(a, b.cpu())


def _full_reference(data, ws, st, L, dtype):
    g = data["g"]
    src, dst = g.src.cpu().long(), g.dst.cpu().long()
    od = torch.bincount(src, minlength=V).double()
    idg = torch.bincount(dst, minlength=V).double()
    A = torch.sparse_coo_tensor(torch.stack([dst, src]), (1.0 / (od[src].sqrt() * idg[dst].sqrt())).to(dtype),
                                (V, V)).coalesce()
    X = data["feat"].cpu().to(dtype)
    for l in range(L):
        Z = torch.sparse.mm(A, X) @ ws[l].to(dtype)
        X = Z if l == L - 1 else torch.relu(_bn(Z, ws[L + 2 * l].to(dtype), ws[L + 2 * l + 1].to(dtype),
                                                st[2 * l].to(dtype), st[2 * l + 1].to(dtype), False))
    return X.log_softmax(1)


# infer_full() forms a narrowing hidden layer's product as A (X W) and a
# widening one's ([32, 48, 8]) as (A X) W: the eval pass follows either
@pytest.mark.parametrize("layers,fanout", [(L2, F2), (L3, F3), ([32, 48, 8], F2)],
                         ids=["2-layers", "3-layers", "widening"])
def test_infer_full_matches_the_float64_chain_and_the_unlimited_fanout_rows(E, data, layers, fanout):
    big = [V] * len(fanout)  # every neighbour: the sampled eval rows are the full ones
    drv = _driver(E, data, _cfg(layers, big))
    drv.set_weights([w.to(DEV) for w in _nontrivial(drv, 3)])
    for _ in range(2):
        drv.train_batch()
    L = len(layers) - 1
    out = drv.infer_full()
    ws, st = [w.cpu() for w in drv.weights()], [s.cpu() for s in drv.norm_stats()]
    r64, r32 = (_full_reference(data, ws, st, L, d) for d in (torch.float64, torch.float32))
    bad = []
    _hold(f"infer_full {layers}", out.cpu(), r64, r32, bad)
    assert torch.equal(out, drv.infer_full())
    seeds = torch.arange(3, 3 + 64 * 7, 7, dtype=torch.int32)
    acts = drv.forward_eval(seeds, 0)
    rows = (acts[-2].cpu() @ ws[L - 1]).log_softmax(1)
    _hold("sampled rows at unlimited fanout", rows, r64[seeds.long()], r32[seeds.long()], bad)
    print(f"  sampled vs infer_full rows bit-identical: {torch.equal(rows, out.cpu()[seeds.long()])}, "
          f"max |diff| {float((rows - out.cpu()[seeds.long()]).abs().max()):.3e}")
    assert not bad, "; ".join(bad)


def test_eval_leaves_training_alone(E, data):
    a = _driver(E, data, _cfg(L3, F3))
    _steps(a, 3)
    b = _driver(E, data, _cfg(L3, F3))
    _steps(b, 2)
    b.infer_full()
    b.evaluate(torch.arange(0, 300, dtype=torch.int32))
    _steps(b, 1)
    for x, y in zip(a.weights() + a.norm_stats(), b.weights() + b.norm_stats()):
        assert torch.equal(x, y)


def test_set_weights_and_set_norm_stats_round_trip(E, data):
    drv = _driver(E, data, _cfg(L3, F3))
    ws = _nontrivial(drv, 5)
    g = torch.Generator().manual_seed(6)
    st = [torch.randn(s.shape, generator=g) if i % 2 == 0 else 0.5 + torch.rand(s.shape, generator=g)
          for i, s in enumerate(drv.norm_stats())]
    drv.set_weights([w.to(DEV) for w in ws])
    drv.set_norm_stats([s.to(DEV) for s in st])
    for a, b in zip(ws + st, drv.weights() + drv.norm_stats()):
        assert torch.equal(a, b.cpu())
    with pytest.raises(RuntimeError, match="norm_stats"):
        drv.set_norm_stats(st[:1])


def test_two_drivers_on_one_seed_agree_byte_for_byte(E, data):
    outs = []
    for _ in range(2):
        drv = _driver(E, data, _cfg(L3, F3, drop_rate=0.5))
        _steps(drv)
        outs.append([t.cpu() for t in drv.weights() + drv.norm_stats()])
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_off_is_the_default(E, data):
    a = _driver(E, data, _cfg(batch_norm=False))
    b = _driver(E, data, tld._cfg())
    assert len(a.weights()) == 2 and a.norm_stats() == []
    for x, y in zip(_steps(a), _steps(b)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("weight,kw", [("mean", dict(up_degree=True)), ("sum", dict(cache_rate=0.5)),
                                       ("sum", dict(pipeline=False)), ("sum", dict(early_aggregate=False)),
                                       ("sum", dict(feature_f16=True)), ("sum", dict(shared_sampling=True))],
                         ids=["mean-up_degree", "cache_rate", "no-pipeline", "late-aggregate",
                              "feature_f16", "shared_sampling"])
def test_trains_with_the_other_options(E, data, weight, kw):
    drv = _driver(E, data, _cfg(weight=weight, drop_rate=0.5, **kw))
    ws = _steps(drv)
    assert all(bool(torch.isfinite(w).all()) for w in ws + [s.cpu() for s in drv.norm_stats()])
    assert bool(torch.isfinite(drv.loss.detach()).item())


LEAD = "batch_norm is not supported with "
REFUSALS = {
    "gat": (dict(gat=True, weight="none"), L2, LEAD + "gat (GCN / GraphSAGE layers only)"),
    "pd_cache": (dict(pd_cache=True), L2, LEAD + "pd_cache"),
    "transform_first": (dict(transform_first=1), L2,
                        LEAD + "transform_first = 1 (BatchNorm does not commute with A: "
                        "aggregate-first only)"),
    "pair_table": (dict(pair_table=1), L2, LEAD + "pair_table > 0"),
    "layer_norm": (dict(layer_norm=True), L2, LEAD + "layer_norm (one normalisation per hidden layer)"),
    "width": ({}, [32, 1028, 8], LEAD + "a hidden width above 1024 (layer 0: 1028)"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refused_combinations(E, data, name):
    kw, layers, text = REFUSALS[name]
    with pytest.raises(RuntimeError, match="batch_norm") as ei:
        _driver(E, data, _cfg(layers, F2, **kw))
    assert str(ei.value).splitlines()[0] == text


def test_cfg_runner_trains_and_scores_with_full_inference(tmp_path):
    from conftest import GOLDEN
    from nts import run
    for f in ("cora.2708.edge.self", "cora.featuretable.zip", "cora.labeltable", "cora.mask"):
        shutil.copy(GOLDEN / "cora" / f, tmp_path / f)
    text = (GOLDEN / "cora" / "gcn_cora_sample.cfg").read_text()
    acc = {}
    for name, extra in (("plain", "FULL_INFERENCE:1\n"), ("bn", "BATCH_NORM:1\nFULL_INFERENCE:1\n")):
        (tmp_path / f"{name}.cfg").write_text(text + extra)
        lines = []
        res = run.run(tmp_path / f"{name}.cfg", epochs=3, out=lines.append)
        acc[name] = res["epochs"][-1]["train_acc"]
        assert any(l.startswith("Train Acc:") for l in lines)
        assert any(l.startswith("Full Eval Acc:") for l in lines)
        assert any(l.startswith("Full Test Acc:") for l in lines)
    print(f"cora final train accuracy: BATCH_NORM {acc['bn']:.4f}, without {acc['plain']:.4f}")
    assert acc["bn"] >= acc["plain"] - 0.05
