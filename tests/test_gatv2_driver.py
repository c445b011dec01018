"""The GATv2 driver (gat_v2): one training step against float64
autograd through the materialised chain of tests/gatv2_blocks.py over the
trained batch's own sampled layers (drv.last_layers), read out through the Adam
step of tests/step_check.py; parameter shapes; determinism with both dropouts
on; evaluation without masks; the untouched default; the GAT_V2 cfg key through
the runner on Cora; and the refusals.

Loss and all four gradients are held to the yardstick rule

    err(recovered g) <= C * err(float32 chain) + 8 * 2^-24 + resolution / max|g64|.

The layer's W is the stacked [W_s | W_d]: Hs = X W_s over the source rows, Hd =
X[dst_local_id] W_d over the destination rows.
"""
import shutil

import pytest
import torch

import gatv2_blocks as g2b
import step_check

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ["W0", "att0", "W1", "att1"]


@pytest.fixture(scope="module")
def E():
    from nts import host
    return host.ext()


@pytest.fixture(scope="module")
def data(E):
    from nts import synthetic
    g = synthetic.chung_lu(6000, 180000, 20.0, device=DEV, seed=3)
    G = E.FullyRepGraph.from_edges(g.src, g.dst, g.n_vertices)
    feat = synthetic.features(g.n_vertices, 64, device=DEV)
    labels, masks = synthetic.labels_masks(g.n_vertices, 7, device=DEV)
    train = torch.nonzero(masks == 0).flatten().to(torch.int32).cpu()
    return dict(G=G, feat=feat, labels=labels, train=train)


def _driver(E, data, layers, heads, readout=True, **kw):
    from nts import host
    kw.setdefault("gat_v2", True)
    cfg = host.gcn_config(layers, [10, 5], 200, drop_rate=0.0, shuffle=False, gat=True,
                          pipeline=False, gat_heads=heads, **kw)
    if readout:
        step_check.readout(cfg)
    return E.GCN_SAMPLE_ALLGPU_impl(data["G"], data["feat"], data["labels"], data["train"], cfg)


def _chain_grads(drv, data, W0, layers, heads, dtype):
    """(loss, gradients of the four parameters) of the materialised chain in `dtype`"""
    top, bottom = drv.last_layers
    W = [w.to(dtype).requires_grad_() for w in W0]
    X = data["feat"].cpu().to(dtype)[bottom["source"].cpu().long()]
    for l, lay in enumerate((bottom, top)):
        co, ri, dl = (lay[k].cpu().long() for k in ("column_offset", "row_indices", "dst_local_id"))
        assert X.shape[0] == lay["src_size"]
        F = W[2 * l].shape[1] // 2
        Hs, Hd = X @ W[2 * l][:, :F], X[dl] @ W[2 * l][:, F:]
        K = heads[l]
        Z, _, _ = g2b.v2_chain_z(Hs, Hd, W[2 * l + 1].view(-1), co, ri, K, F // K,
                                 mean=l == 1 and K > 1)
        X = torch.relu(Z)
    assert X.shape[1] == layers[-1]
    tgt = data["labels"].cpu()[top["destination"].cpu().long()]
    loss = torch.nn.functional.nll_loss(X.log_softmax(1), tgt)
    loss.backward()
    return float(loss.detach()), [w.grad for w in W]


@pytest.mark.parametrize("layers,heads", [([64, 64, 7], [1, 1]), ([64, 64, 7], [8, 1]),
                                          ([64, 64, 7], [8, 8]), ([64, 264, 7], [2, 1])],
                         ids=["64-64-7-heads1-1", "64-64-7-heads8-1", "64-64-7-heads8-8",
                              "64-264-7-heads2-1"])
def test_v2_step_gradients_match_the_float64_chain(E, data, layers, heads):
    drv = _driver(E, data, layers, heads)
    W0 = [w.cpu().clone() for w in drv.weights()]
    hid, out = layers[1], heads[1] * layers[2]
    assert [tuple(w.shape) for w in W0] == [(64, 2 * hid), (hid, 1), (hid, 2 * out), (out, 1)]
    drv.train_batch()
    drv.synchronize()
    W1 = [w.cpu().clone() for w in drv.weights()]
    loss64, g64 = _chain_grads(drv, data, W0, layers, heads, torch.float64)
    loss32, g32 = _chain_grads(drv, data, W0, layers, heads, torch.float32)
    got = float(drv.loss.detach())
    print(f"GATv2 {layers} heads {heads}: loss {got!r} float64 {loss64!r} float32 chain {loss32!r}")
    assert abs(got - loss64) <= step_check.yardstick_bound(abs(loss32 - loss64) / abs(loss64),
                                                           step_check.C) * abs(loss64)
    step_check.check_step_grads(W0, W1, g64, g32, step_check.C, NAMES)


def _three_steps(drv):
    for _ in range(3):
        drv.train_batch()
    drv.synchronize()
    return float(drv.loss.detach()), [w.cpu().clone() for w in drv.weights()]


def test_two_drivers_with_dropout_are_bit_identical(E, data):
    kw = dict(readout=False, gat_attn_drop=0.6, gat_feat_drop=0.6)
    la, wa = _three_steps(_driver(E, data, [64, 64, 7], [8, 1], **kw))
    lb, wb = _three_steps(_driver(E, data, [64, 64, 7], [8, 1], **kw))
    assert la == lb
    for x, y in zip(wa, wb):
        assert torch.equal(x, y)
    # and the masks are drawn: the weights differ from a rates-0 driver's
    _, w0 = _three_steps(_driver(E, data, [64, 64, 7], [8, 1], readout=False))
    assert any(not torch.equal(x, y) for x, y in zip(wa, w0))


def test_evaluation_draws_no_mask(E, data):
    layers, heads = [64, 64, 7], [8, 1]
    off = _driver(E, data, layers, heads, readout=False)
    on = _driver(E, data, layers, heads, readout=False, gat_attn_drop=0.6, gat_feat_drop=0.6)
    on.set_weights(off.weights())
    for x, y in zip(on.weights(), off.weights()):
        assert torch.equal(x, y)
    seeds = torch.arange(0, 256, dtype=torch.int32)
    for x, y in zip(off.forward_eval(seeds, 0), on.forward_eval(seeds, 0)):
        assert torch.equal(x, y)
    ids = torch.arange(0, 1000, dtype=torch.int32)
    assert off.evaluate(ids) == on.evaluate(ids)
    # no dropout offset was consumed: the first training step after it equals
    # that of a fresh driver with the same options and weights
    fresh = _driver(E, data, layers, heads, readout=False, gat_attn_drop=0.6, gat_feat_drop=0.6)
    fresh.set_weights(off.weights())
    for d in (on, fresh):
        d.train_batch()
        d.synchronize()
    for x, y in zip(on.weights(), fresh.weights()):
        assert torch.equal(x, y)


def test_the_default_is_untouched(E, data):
    """gat = True without gat_v2: the old shapes, and the same first step as a
    driver whose gcn_config call never names gat_v2."""
    from nts import host
    a = _driver(E, data, [64, 64, 7], [8, 1], readout=False, gat_v2=False)
    cfg = host.gcn_config([64, 64, 7], [10, 5], 200, drop_rate=0.0, shuffle=False, gat=True,
                          pipeline=False, gat_heads=[8, 1])
    assert cfg.gat_v2 is False
    b = E.GCN_SAMPLE_ALLGPU_impl(data["G"], data["feat"], data["labels"], data["train"], cfg)
    assert [tuple(w.shape) for w in a.weights()] == [(64, 64), (128, 1), (64, 7), (14, 1)]
    for d in (a, b):
        d.train_batch()
        d.synchronize()
    for x, y in zip(a.weights(), b.weights()):
        assert torch.equal(x, y)


def test_refusals(E, data):
    from nts import host
    with pytest.raises(ValueError, match="gat_v2 is not supported without gat"):
        host.gcn_config([64, 64, 7], [10, 5], 200, gat=False, gat_v2=True)
    cfg = host.gcn_config([64, 64, 7], [10, 5], 200, pipeline=False)
    cfg.gat_v2 = True  # field by field: the driver's own check
    with pytest.raises(RuntimeError,
                       match=r"gat_v2 is not supported without gat \(attention layers only\)"):
        E.GCN_SAMPLE_ALLGPU_impl(data["G"], data["feat"], data["labels"], data["train"], cfg)
    drv = _driver(E, data, [64, 64, 7], [8, 1], readout=False)
    with pytest.raises(RuntimeError, match="full-neighbour inference for GATv2.*not built"):
        drv.infer_full_gat()
    with pytest.raises(RuntimeError, match="full-neighbour inference for GATv2.*not built"):
        drv.evaluate_full_gat(torch.arange(0, 10, dtype=torch.int32))


def test_cfg_runner_trains_cora_with_gat_v2(tmp_path):
    """GAT_V2:1 through the runner: 3 epochs of 1433-64-7 with heads 8-1 on Cora
    train and report accuracies; the key is refused with a GCN algorithm and
    together with FULL_INFERENCE."""
    from conftest import GOLDEN
    from nts import run
    for f in ("cora.2708.edge.self", "cora.featuretable.zip", "cora.labeltable", "cora.mask"):
        shutil.copy(GOLDEN / "cora" / f, tmp_path / f)
    text = (GOLDEN / "cora" / "gcn_cora_sample.cfg").read_text()
    gcn = text.replace("LAYERS:1433-256-7", "LAYERS:1433-64-7")
    text = gcn.replace("ALGORITHM:GCNSAMPLEALLGPU", "ALGORITHM:GATSAMPLEALLGPU")
    (tmp_path / "v2.cfg").write_text(text + "GAT_HEADS:8-1\nGAT_V2:1\n")
    res = run.run(tmp_path / "v2.cfg", epochs=3, out=lambda s: None)
    assert len(res["epochs"]) == 3
    accs = [(round(e["train_acc"], 3), round(e["test_acc"], 3)) for e in res["epochs"]]
    print("GAT_V2:1", accs)
    for e in res["epochs"]:
        assert 0.0 <= e["train_acc"] <= 1.0 and 0.0 <= e["test_acc"] <= 1.0
    assert res["epochs"][-1]["train_acc"] > 2.0 / 7.0  # it learns (chance: 1/7)
    (tmp_path / "bad.cfg").write_text(gcn + "GAT_V2:1\n")
    with pytest.raises(SystemExit, match="GAT_V2 is not supported with GCN"):
        run.run(tmp_path / "bad.cfg", epochs=1, out=lambda s: None)
    (tmp_path / "bad2.cfg").write_text(text + "GAT_V2:1\nFULL_INFERENCE:1\n")
    with pytest.raises(SystemExit, match="FULL_INFERENCE is not supported with GAT_V2"):
        run.run(tmp_path / "bad2.cfg", epochs=1, out=lambda s: None)
