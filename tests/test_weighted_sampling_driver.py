"""Edge-weighted neighbour selection through the C++ driver
(gcn_config(weighted_sampling=True) on a graph with edge_prob).

One training step is checked on the block the driver sampled (drv.last_layers)
against the float64 chain, read out through tests/step_check.py with its bound
(C = step_check.C times the float32 chain's own error); the block itself must
be the restatement's selection (tests/weighted_blocks.py) from the device's
keys (nts_hip_weighted_keys) for the batch's seeds, batch_seq and layer.
"""
import shutil

import numpy as np
import pytest
import torch

import step_check
import weighted_blocks as wb

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEED = 2000
LAYERS, FANOUT, BATCH = [64, 64, 7], [10, 5], 200


@pytest.fixture(scope="module")
def E():
    from nts import host
    return host.ext()


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=SEED)


@pytest.fixture(scope="module")
def data(E):
    from nts import synthetic
    from nts.hip import DeviceGraph
    g = synthetic.chung_lu(2000, 40000, 10.0, device=DEV, seed=5)
    w = torch.from_numpy(np.exp2(np.random.default_rng(6).uniform(-3, 3, g.src.numel()))
                         .astype(np.float32)).to(DEV)
    G = E.FullyRepGraph.from_edges(g.src, g.dst, g.n_vertices, w)
    feat = synthetic.features(g.n_vertices, 64, device=DEV)
    labels, masks = synthetic.labels_masks(g.n_vertices, 7, device=DEV)
    train = torch.nonzero(masks == 0).flatten().to(torch.int32).cpu()
    dg = DeviceGraph(g.n_vertices, g.src.numel(), G.column_offset, G.row_indices, G.in_degree,
                     G.out_degree)
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    host_g = dict(col=G.column_offset.cpu().numpy().view(np.uint64), rows=u32(G.row_indices),
                  idg=u32(G.in_degree), od=u32(G.out_degree))
    return dict(G=G, g=g, w=w, feat=feat, labels=labels, masks=masks, train=train, dg=dg, **host_g)


def _driver(E, data, layers=LAYERS, readout=False, **kw):
    from nts import host
    cfg = host.gcn_config(list(layers), FANOUT, BATCH, drop_rate=0.0, shuffle=False, **kw)
    if readout:
        step_check.readout(cfg)
    return E.GCN_SAMPLE_ALLGPU_impl(data["G"], data["feat"], data["labels"], data["train"], cfg)


def _losses(drv, n):
    out = []
    for _ in range(n):
        drv.train_batch()
        drv.synchronize()
        out.append(float(drv.loss.detach()))
    return out


def _assert_block_is_the_restatement(hip, drv, data, batch_seq, flags, merge):
    """every layer array of the trained block == the selection from the
    device's keys of (batch_seq, layer)"""
    seeds = data["train"].numpy().view(np.uint32)[batch_seq * BATCH:(batch_seq + 1) * BATCH]
    dst, checked = seeds, 0
    for l, got in enumerate(drv.last_layers):
        deg = (data["col"][dst.astype(np.int64) + 1] - data["col"][dst.astype(np.int64)]).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(deg)[:-1]]).astype(np.int64)
        keys = hip.weighted_keys(data["dg"], data["G"].edge_prob,
                                 torch.from_numpy(dst.view(np.int32).copy()).to(DEV), l, batch_seq,
                                 torch.from_numpy(off).to(DEV))
        torch.cuda.synchronize()
        keys = keys.cpu().numpy().view(np.uint32)
        want = wb.weighted_layer(data["col"], data["rows"], data["idg"], data["od"], dst, FANOUT[l],
                                 lambda i, d, beg, n: keys[off[i]:off[i] + n], flags, merge)
        assert (got["v_size"], got["e_size"], got["src_size"]) == (
            want["v_size"], want["e_size"], want["src_size"])
        for k, w in want.items():
            t = got.get(k) if isinstance(w, np.ndarray) else None
            if t is None or not isinstance(t, torch.Tensor):
                continue
            a = t.cpu().numpy()
            a = a.view(np.uint32) if a.dtype == np.int32 else a
            assert np.array_equal(a, w), (l, k)
            checked += 1
        if l == 0:
            assert (deg > FANOUT[0]).sum() > 50  # the selection was exercised
        dst = want["source"]
    assert checked >= 10


def test_from_edges_moves_the_weights_to_csc_order_and_exposes_them(E, data):
    ep = data["G"].edge_prob
    assert ep.dtype == torch.float32 and ep.is_cuda and ep.numel() == data["g"].src.numel()
    want = wb.csc_edge_prob(data["g"].dst.cpu().numpy().view(np.uint32), data["w"].cpu().numpy())
    assert np.array_equal(ep.cpu().numpy(), want)
    with pytest.raises(AttributeError):
        data["G"].edge_prob = ep
    plain = E.FullyRepGraph.from_edges(data["g"].src, data["g"].dst, data["g"].n_vertices)
    assert plain.edge_prob is None
    G2 = E.FullyRepGraph.from_csc(data["G"].column_offset, data["G"].row_indices,
                                  data["G"].in_degree, data["G"].out_degree, edge_prob=ep)
    assert torch.equal(G2.edge_prob, ep)
    assert E.FullyRepGraph.from_csc(data["G"].column_offset, data["G"].row_indices,
                                    data["G"].in_degree, data["G"].out_degree).edge_prob is None


@pytest.mark.parametrize("bad,shown", [(0.0, "0"), (-1.0, "-1"), (float("nan"), "nan"),
                                       (float("inf"), "inf"), (2.0 ** 61, "2.30584"),
                                       (2.0 ** -61, "4.33681")])
def test_a_bad_weight_is_refused_at_load_with_count_and_first_offender(E, data, bad, shown):
    w = data["w"].clone()
    w[[7, 300, 301]] = bad
    with pytest.raises(RuntimeError) as ei:
        E.FullyRepGraph.from_edges(data["g"].src, data["g"].dst, data["g"].n_vertices, w)
    msg = str(ei.value).splitlines()[0]
    assert msg.startswith("edge_weight: 3 value(s) are not finite and in [2^-60, 2^60]")
    assert f"the first is edge 7 with value {shown}" in msg
    ep = data["G"].edge_prob.clone()
    ep[5] = bad
    with pytest.raises(RuntimeError, match=r"edge_prob: 1 value\(s\).*the first is edge 5 "):
        E.FullyRepGraph.from_csc(data["G"].column_offset, data["G"].row_indices,
                                 data["G"].in_degree, data["G"].out_degree, ep)
    with pytest.raises(RuntimeError, match="edge_weight: a float32 CUDA tensor with one value per"):
        E.FullyRepGraph.from_edges(data["g"].src, data["g"].dst, data["g"].n_vertices, w[:-1])


def _gcn_chain(drv, data, W0, dtype):
    """(loss, gradients) of the GCN chain on the trained batch's own block"""
    top, bottom = drv.last_layers

    def agg(lay, X):
        co, ri = lay["column_offset"].cpu().long(), lay["row_indices"].cpu().long()
        w = lay["edge_weight_forward"].cpu().to(dtype)
        d_of_e = torch.repeat_interleave(torch.arange(co.numel() - 1), co[1:] - co[:-1])
        return torch.zeros(co.numel() - 1, X.shape[1], dtype=dtype).index_add(0, d_of_e,
                                                                             X[ri] * w[:, None])

    W = [w.to(dtype).requires_grad_() for w in W0]
    X0 = data["feat"].cpu().to(dtype)[bottom["source"].cpu().long()]
    X1 = torch.relu(agg(bottom, X0) @ W[0])
    out = (agg(top, X1) @ W[1]).log_softmax(1)
    loss = torch.nn.functional.nll_loss(out, data["labels"].cpu()[top["destination"].cpu().long()])
    loss.backward()
    return float(loss.detach()), [w.grad for w in W]


@pytest.mark.parametrize("model", ["gcn", "gat"])
def test_one_training_step_on_the_sampled_block(E, hip, data, model):
    import test_gat_heads_driver as tg
    heads = [8, 1]
    kw = dict(gat=True, pipeline=False, gat_heads=heads) if model == "gat" else {}
    drv = _driver(E, data, readout=True, weighted_sampling=True, **kw)
    W0 = [w.cpu().clone() for w in drv.weights()]
    drv.train_batch()
    drv.synchronize()
    W1 = [w.cpu().clone() for w in drv.weights()]
    _assert_block_is_the_restatement(hip, drv, data, 0, wb.W_NONE if model == "gat" else wb.W_SUM,
                                     model == "gat")
    if model == "gat":
        chain = lambda dt: tg._chain_grads(drv, data, W0, LAYERS, heads, dt)
    else:
        chain = lambda dt: _gcn_chain(drv, data, W0, dt)
    (loss64, g64), (loss32, g32) = chain(torch.float64), chain(torch.float32)
    got = float(drv.loss.detach())
    print(f"weighted sampling, {model} {LAYERS}: loss {got!r} float64 {loss64!r} float32 chain "
          f"{loss32!r}")
    assert abs(got - loss64) <= step_check.yardstick_bound(abs(loss32 - loss64) / abs(loss64),
                                                           step_check.C) * abs(loss64)
    step_check.check_step_grads(W0, W1, g64, g32, step_check.C, tg.NAMES if model == "gat" else None)


def test_pipeline_on_and_off_train_on_the_same_batches(E, hip, data):
    a = _driver(E, data, weighted_sampling=True, pipeline=True)
    b = _driver(E, data, weighted_sampling=True, pipeline=False)
    on, off = _losses(a, 4), _losses(b, 4)
    plain = _losses(_driver(E, data, pipeline=False), 4)
    assert on == off and all(np.isfinite(on))
    assert on != plain  # another selection
    for drv in (a, b):  # the fourth batch of both is the restatement's
        _assert_block_is_the_restatement(hip, drv, data, 3, wb.W_SUM, False)


def test_evaluate_and_forward_eval_run(E, data):
    ids = torch.nonzero(data["masks"].cpu() == 1).flatten().to(torch.int32)[:300]
    a, b = _driver(E, data, weighted_sampling=True), _driver(E, data, weighted_sampling=True)
    _losses(a, 2)
    _losses(b, 2)
    first, second = [a.evaluate(ids), a.evaluate(ids)], [b.evaluate(ids), b.evaluate(ids)]
    assert first == second and all(0.0 <= x <= 1.0 for x in first)
    fa, fb = a.forward_eval(ids[:64], 0), b.forward_eval(ids[:64], 0)
    assert all(torch.equal(x, y) for x, y in zip(fa, fb))
    assert fa[-1].shape == (64, 7) and torch.isfinite(fa[-1]).all()
    plain = _driver(E, data)
    plain.set_weights(a.weights())
    # the evaluation samplers are weighted too: another block, other activations
    assert not torch.equal(plain.forward_eval(ids[:64], 0)[-1], fa[-1])


def test_the_default_is_byte_identical_to_a_config_that_never_names_the_option(E, data):
    from nts import host
    out = []
    for named in (True, False):
        kw = dict(weighted_sampling=False) if named else {}
        cfg = host.gcn_config(LAYERS, FANOUT, BATCH, drop_rate=0.0, shuffle=False, **kw)
        assert cfg.weighted_sampling is False
        # (a graph with and one without edge_prob: the default never reads it)
        G = data["G"] if named else E.FullyRepGraph.from_edges(data["g"].src, data["g"].dst,
                                                               data["g"].n_vertices)
        drv = E.GCN_SAMPLE_ALLGPU_impl(G, data["feat"], data["labels"], data["train"], cfg)
        drv.train_batch()
        drv.synchronize()
        out.append((drv.loss.detach().cpu().clone(), [w.cpu().clone() for w in drv.weights()]))
    assert torch.equal(out[0][0], out[1][0])
    assert all(torch.equal(x, y) for x, y in zip(out[0][1], out[1][1]))


def _refusal(fn):
    with pytest.raises(RuntimeError) as ei:
        fn()
    return str(ei.value).splitlines()[0]


def test_constructor_refusals(E, data):
    """in the constructor's order.  (sample_gpu takes an MT19937 rng_mode, so
    with weighted_sampling the MT19937 refusal is the one that reports it.)"""
    from nts import host
    plain = dict(data, G=E.FullyRepGraph.from_edges(data["g"].src, data["g"].dst,
                                                    data["g"].n_vertices))

    def make(d, weighted=True, **kw):
        cfg = host.gcn_config(LAYERS, FANOUT, BATCH, drop_rate=0.0, shuffle=False, **kw)
        cfg.weighted_sampling = weighted  # (gcn_config refuses two of these itself)
        return lambda: E.GCN_SAMPLE_ALLGPU_impl(d["G"], d["feat"], d["labels"], d["train"], cfg)

    assert _refusal(make(plain)) == (
        "weighted_sampling needs a graph with edge_prob (from_edges(..., edge_weight) or "
        "from_csc(..., edge_prob))")
    for mt in (1, 2):
        assert _refusal(make(data, rng_mode=mt)) == (
            "weighted_sampling is not supported with an MT19937 rng_mode (it draws from a Philox "
            "stream of its own)")
    assert _refusal(make(data, rng_mode=3)) == (
        "weighted_sampling is not supported with rng_mode NTS_RNG_PHILOX_SHARED (shared_sampling)")
    assert _refusal(make(data, pd_cache=True)) == "weighted_sampling is not supported with pd_cache"
    assert "weighted_sampling is not supported with an MT19937" in _refusal(
        make(data, sample_gpu=True, rng_mode=1))
    # an existing option's conflict is reported before the new ones
    assert _refusal(make(data, layer_norm=True, pd_cache=True)) == (
        "layer_norm is not supported with pd_cache")


def _two_class_moments(h, l, wh, n):
    """mean and variance of the number of heavy items among n successive picks
    without replacement from h items of weight wh and l items of weight 1:
    exact, by the chain over (heavy left, light left)"""
    dist = {(h, l): 1.0}
    for _ in range(n):
        nxt = {}
        for (a, b), p in dist.items():
            tot = a * wh + b
            if a:
                nxt[(a - 1, b)] = nxt.get((a - 1, b), 0.0) + p * a * wh / tot
            if b:
                nxt[(a, b - 1)] = nxt.get((a, b - 1), 0.0) + p * b / tot
        dist = nxt
    k = np.array([h - a for (a, b) in dist])
    p = np.array(list(dist.values()))
    mean = float((k * p).sum())
    return mean, float((k * k * p).sum() - mean * mean)


def test_heavy_edge_share_of_the_sampled_block(E):
    """every vertex has 4 heavy in-edges (weight 100, from the vertices below
    100) and 36 light ones (weight 1): the share of heavy edges among the top
    hop's sampled ones against its exact expectation"""
    from nts import host
    rng = np.random.default_rng(8)
    V, H, L, B, F0 = 2000, 4, 36, 500, 10
    src = np.concatenate([np.concatenate([rng.choice(100, H, replace=False),
                                          rng.choice(np.arange(100, V), L, replace=False)])
                          for _ in range(V)]).astype(np.int32)
    dst = np.repeat(np.arange(V), H + L).astype(np.int32)
    w = np.where(src < 100, 100.0, 1.0).astype(np.float32)
    order = rng.permutation(src.size)
    s_t, d_t, w_t = (torch.from_numpy(x[order]).to(DEV) for x in (src, dst, w))
    G = E.FullyRepGraph.from_edges(s_t, d_t, V, w_t)
    feat = torch.randn(V, 16, device=DEV)
    labels = torch.randint(0, 3, (V,), device=DEV)
    train = torch.arange(100, 100 + B, dtype=torch.int32)
    share = {}
    for weighted in (True, False):
        cfg = host.gcn_config([16, 8, 3], [F0, 5], B, drop_rate=0.0, shuffle=False,
                              weighted_sampling=weighted)
        drv = E.GCN_SAMPLE_ALLGPU_impl(G, feat, labels, train, cfg)
        drv.train_batch()
        drv.synchronize()
        top = drv.last_layers[0]
        assert top["e_size"] == B * F0
        share[weighted] = float((top["sample_ans"].cpu() < 100).float().mean())
    mean, var = _two_class_moments(H, L, 100.0, F0)
    want, sd = mean / F0, np.sqrt(B * var) / (B * F0)
    print(f"heavy share: weighted {share[True]:.4f} (exact {want:.4f}, sd {sd:.5f}), "
          f"uniform sampler {share[False]:.4f} (H / (H + L) = {H / (H + L):.2f})")
    assert abs(share[True] - want) <= 5 * sd
    assert abs(share[False] - want) > 20 * sd and share[False] < 0.5 * share[True]


def test_cfg_runner_cora_with_a_weight_file_and_full_inference(tmp_path):
    from conftest import GOLDEN
    from nts import dataloader, run
    for f in ("cora.2708.edge.self", "cora.featuretable.zip", "cora.labeltable", "cora.mask"):
        shutil.copy(GOLDEN / "cora" / f, tmp_path / f)
    src, dst = dataloader.read_edge_file(tmp_path / "cora.2708.edge.self")
    od = np.maximum(np.bincount(src, minlength=2708), 1)
    idg = np.maximum(np.bincount(dst, minlength=2708), 1)
    dataloader.write_edge_weight_file(tmp_path / "cora.weight", 1.0 / np.sqrt(idg[dst] * od[src]))
    text = (GOLDEN / "cora" / "gcn_cora_sample.cfg").read_text()
    (tmp_path / "job.cfg").write_text(text + "EDGE_WEIGHT_FILE:cora.weight\nSAMPLE_WEIGHTED:1\n"
                                      "FULL_INFERENCE:1\n")
    lines = []
    res = run.run(tmp_path / "job.cfg", epochs=3, out=lines.append)
    assert len(res["epochs"]) == 3
    last = res["epochs"][-1]
    print(f"cora, SAMPLE_WEIGHTED:1, 3 epochs: train {last['train_acc']:.4f} eval "
          f"{last['eval_acc']:.4f} test {last['test_acc']:.4f} full test {res['full_test_acc']:.4f}")
    assert all(np.isfinite(e["loss"]) for e in res["epochs"])
    assert last["test_acc"] > 0.5 and res["full_test_acc"] > 0.5  # 7 classes: far above chance
    assert sum(l.startswith("Test Acc:") for l in lines) == 3
    assert any(l.startswith("Full Test Acc:") for l in lines)
    (tmp_path / "cora.weight").write_bytes((tmp_path / "cora.weight").read_bytes()[:-4])
    with pytest.raises(ValueError, match="bytes, expected"):
        run.run(tmp_path / "job.cfg", epochs=1, out=lambda s: None)
