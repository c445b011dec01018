"""The multi-head GAT driver (gat_heads): one training step against float64
autograd through the per-head chain of tests/gat_heads_blocks.py over the
trained batch's own sampled layers (drv.last_layers), read out through the Adam
step of tests/step_check.py; the GAT_HEADS cfg key through the runner on Cora;
the refused combinations; and gat_heads = [1, 1] as the single-head driver.

Hidden layers concatenate their heads (LAYERS keeps the concatenated width);
the last layer with K > 1 averages K heads of 7 columns.  Loss and all four
gradients are held to the yardstick rule

    err(recovered g) <= C * err(float32 chain) + 8 * 2^-24 + resolution / max|g64|.

[64, 64, 7] with heads [8, 1] runs the float4 kernels at g = 2 (and the
single-head scalar output layer), heads [8, 8] adds the scalar mean-mode output
layer (K D = 56), [64, 264, 7] with heads [2, 1] the g = 33 fallback on two
chunks.
"""
import shutil

import pytest
import torch

import gat_heads_blocks as ghb
import step_check

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ["W0", "W_att0", "W1", "W_att1"]


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
    cfg = host.gcn_config(layers, [10, 5], 200, drop_rate=0.0, shuffle=False, gat=True,
                          pipeline=False, gat_heads=heads, **kw)
    if readout:
        step_check.readout(cfg)
    return E.GCN_SAMPLE_ALLGPU_impl(data["G"], data["feat"], data["labels"], data["train"], cfg)


def _chain_grads(drv, data, W0, layers, heads, dtype):
    """(loss, gradients of the four parameters) of the per-head chain in `dtype`"""
    top, bottom = drv.last_layers
    W = [w.to(dtype).requires_grad_() for w in W0]
    X = data["feat"].cpu().to(dtype)[bottom["source"].cpu().long()]
    for l, lay in enumerate((bottom, top)):
        co, ri, dl = (lay[k].cpu().long() for k in ("column_offset", "row_indices", "dst_local_id"))
        assert X.shape[0] == lay["src_size"]
        H = X @ W[2 * l]
        K = heads[l]
        X, _, _ = ghb.heads_chain(H, W[2 * l + 1].view(-1), co, ri, dl, K, H.shape[1] // K,
                                  mean=l == 1 and K > 1)
    assert X.shape[1] == layers[-1]
    tgt = data["labels"].cpu()[top["destination"].cpu().long()]
    loss = torch.nn.functional.nll_loss(X.log_softmax(1), tgt)
    loss.backward()
    return float(loss.detach()), [w.grad for w in W]


@pytest.mark.parametrize("layers,heads", [([64, 64, 7], [8, 1]), ([64, 64, 7], [8, 8]),
                                          ([64, 264, 7], [2, 1])],
                         ids=["64-64-7-heads8-1", "64-64-7-heads8-8", "64-264-7-heads2-1"])
def test_heads_step_gradients_match_the_float64_chain(E, data, layers, heads):
    drv = _driver(E, data, layers, heads)
    W0 = [w.cpu().clone() for w in drv.weights()]
    hid, out = layers[1], heads[1] * layers[2]
    assert [tuple(w.shape) for w in W0] == [(64, hid), (2 * hid, 1), (hid, out), (2 * out, 1)]
    if heads == [8, 8]:
        assert [tuple(w.shape) for w in W0] == [(64, 64), (128, 1), (64, 56), (112, 1)]
    drv.train_batch()
    drv.synchronize()
    W1 = [w.cpu().clone() for w in drv.weights()]
    loss64, g64 = _chain_grads(drv, data, W0, layers, heads, torch.float64)
    loss32, g32 = _chain_grads(drv, data, W0, layers, heads, torch.float32)
    got = float(drv.loss.detach())
    print(f"GAT {layers} heads {heads}: loss {got!r} float64 {loss64!r} float32 chain {loss32!r}")
    assert abs(got - loss64) <= step_check.yardstick_bound(abs(loss32 - loss64) / abs(loss64),
                                                           step_check.C) * abs(loss64)
    step_check.check_step_grads(W0, W1, g64, g32, step_check.C, NAMES)


def test_heads_1_1_is_the_single_head_driver(E, data):
    a = _driver(E, data, [64, 32, 7], [1, 1], readout=False)
    b = _driver(E, data, [64, 32, 7], None, readout=False)
    for d in (a, b):
        for _ in range(3):
            d.train_batch()
        d.synchronize()
    assert float(a.loss.detach()) == float(b.loss.detach())
    for x, y in zip(a.weights(), b.weights()):
        assert torch.equal(x, y)


def test_refused_combinations_name_the_option(E, data):
    from nts import host
    # the driver's own checks (a GCNConfig filled in field by field skips gcn_config's)
    def build(layers, heads, gat=True):
        cfg = host.gcn_config(layers, [10, 5], 200, gat=gat, pipeline=False)
        cfg.gat_heads = heads
        return E.GCN_SAMPLE_ALLGPU_impl(data["G"], data["feat"], data["labels"], data["train"], cfg)

    for layers, heads, gat, msg in [
        ([64, 64, 7], [8, 1], False, "gat_heads is not supported without gat"),
        ([64, 64, 7], [8], True, "gat_heads needs one entry per layer"),
        ([64, 64, 7], [0, 1], True, r"gat_heads\[0\] must be >= 1"),
        ([64, 64, 7], [3, 1], True, r"gat_heads\[0\] = 3 does not divide layer width 64"),
        ([64, 64, 7], [1, 40], True, r"gat_heads\[1\].*width limit"),
        ([64, 1032, 7], [2, 1], True, r"gat_heads\[0\].*width limit"),
    ]:
        with pytest.raises(RuntimeError, match=msg):
            build(layers, heads, gat)
    for kw, msg in [(dict(gat=False, gat_heads=[8, 1]), "gat_heads is not supported without gat"),
                    (dict(gat=True, gat_heads=[3, 1]), "does not divide")]:
        with pytest.raises(ValueError, match=msg):
            host.gcn_config([64, 64, 7], [10, 5], 200, **kw)
    drv = _driver(E, data, [64, 64, 7], [8, 1], readout=False)
    with pytest.raises(RuntimeError, match="infer_full"):
        drv.infer_full()


def test_cfg_runner_trains_cora_with_gat_heads(tmp_path):
    """GAT_HEADS:8-1 through the runner: 3 epochs of 1433-64-7 on Cora run and
    print accuracies in the range the single-head cfg reaches (both figures are
    printed; the multi-head model's final train accuracy is held to the
    single-head one's less 0.2, far above the 1/7 of a model that does not learn
    whenever the single-head one learns)."""
    from conftest import GOLDEN
    from nts import run
    for f in ("cora.2708.edge.self", "cora.featuretable.zip", "cora.labeltable", "cora.mask"):
        shutil.copy(GOLDEN / "cora" / f, tmp_path / f)
    text = (GOLDEN / "cora" / "gcn_cora_sample.cfg").read_text()
    text = text.replace("ALGORITHM:GCNSAMPLEALLGPU", "ALGORITHM:GATSAMPLEALLGPU")
    text = text.replace("LAYERS:1433-256-7", "LAYERS:1433-64-7")
    (tmp_path / "single.cfg").write_text(text)
    (tmp_path / "heads.cfg").write_text(text + "GAT_HEADS:8-1\n")
    res = {}
    for name in ("single", "heads"):
        lines = []
        res[name] = run.run(tmp_path / f"{name}.cfg", epochs=3, out=lines.append)
        assert len(res[name]["epochs"]) == 3
        for e in res[name]["epochs"]:
            assert 0.0 <= e["train_acc"] <= 1.0 and 0.0 <= e["test_acc"] <= 1.0
        print(name, [(round(e["train_acc"], 3), round(e["test_acc"], 3))
                     for e in res[name]["epochs"]])
    single, heads = (res[k]["epochs"][-1]["train_acc"] for k in ("single", "heads"))
    assert heads >= single - 0.2
    (tmp_path / "bad.cfg").write_text(text.replace("GATSAMPLEALLGPU", "GCNSAMPLEALLGPU")
                                      + "GAT_HEADS:8-1\n")
    with pytest.raises(SystemExit, match="not supported"):
        run.run(tmp_path / "bad.cfg", epochs=1, out=lambda s: None)
    (tmp_path / "bad2.cfg").write_text(text + "GAT_HEADS:8-x\n")
    with pytest.raises(ValueError, match="GAT_HEADS"):
        run.run(tmp_path / "bad2.cfg", epochs=1, out=lambda s: None)
