"""GAT dropout through the driver (gat_attn_drop / gat_feat_drop) on
the graph of tests/test_gat_heads_driver.py.

One readout step (tests/step_check.py) of a single-head [64, 32, 7] model and of
a gat_heads = [4, 2] one with rates (0.6, 0.5): every W and W_att is held to the
yardstick rule against float64 autograd through the chain of
tests/gat_drop_blocks.py over the trained batch's own sampled layers, with the
masks rebuilt from cfg.seed and the order of the draws of a training forward —
offset 0 the input pass, then per layer the attention draw and (hidden layers)
the output draw: 1, 2, 3 for two layers.  Then: explicit zero rates and unset
options give the same bytes, two drivers with one seed give the same bytes with
dropout on, evaluation and inference do not see the options, and the
constructor's refusal texts.
"""
import pytest
import torch

import gat_drop_blocks as gdb
import step_check

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ["W0", "W_att0", "W1", "W_att1"]
Q, P = 0.6, 0.5


@pytest.fixture(scope="module")
def E():
    from nts import host
    return host.ext()


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=2000)


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
    return E.GCN_SAMPLE_ALLGPU_impl(data["G"], data["feat"], data["labels"], data["train"], cfg), cfg


def _mask(hip, rows, cols, p, key, offset):
    y = torch.empty(rows, cols, device=DEV)
    hip.relu_dropout(torch.ones(rows, cols, device=DEV), y, p=p, seed=key, offset=offset)
    return (y > 0).cpu()


def _chain_grads(hip, drv, cfg, data, W0, heads, dtype):
    """(loss, gradients) of the dropped chain in `dtype` over drv.last_layers"""
    key = (cfg.seed * 0x9E3779B97F4A7C15 + 1) % 2 ** 64  # the driver's dropout_key()
    top, bottom = drv.last_layers
    W = [w.to(dtype).requires_grad_() for w in W0]
    X = data["feat"].cpu().to(dtype)[bottom["source"].cpu().long()]
    sa, sf = gdb.scale(Q), gdb.scale(P)
    off = 0
    X = X * _mask(hip, X.shape[0], X.shape[1], P, key, off).to(dtype) * sf  # the input pass
    off += 1
    for l, lay in enumerate((bottom, top)):
        co, ri, dl = (lay[k].cpu().long() for k in ("column_offset", "row_indices", "dst_local_id"))
        assert X.shape[0] == lay["src_size"]
        H = X @ W[2 * l]
        K = heads[l]
        D, mean = H.shape[1] // K, l == 1 and K > 1
        keepA = _mask(hip, ri.numel(), K, Q, key, off)
        off += 1
        keepF = None
        if l == 0:  # hidden layers only
            keepF = _mask(hip, co.numel() - 1, H.shape[1], P, key, off)
            off += 1
        X, _, _, _ = gdb.drop_chain(H, W[2 * l + 1].view(-1), co, ri, dl, K, D, mean, keepA, sa,
                                    keepF, sf if l == 0 else 1.0)
    tgt = data["labels"].cpu()[top["destination"].cpu().long()]
    loss = torch.nn.functional.nll_loss(X.log_softmax(1), tgt)
    loss.backward()
    return float(loss.detach()), [w.grad for w in W]


@pytest.mark.parametrize("heads", [None, [4, 2]], ids=["single-head", "heads4-2"])
def test_dropout_step_gradients_match_the_float64_chain(E, hip, data, heads):
    layers = [64, 32, 7]
    drv, cfg = _driver(E, data, layers, heads, gat_attn_drop=Q, gat_feat_drop=P)
    hs = heads or [1, 1]
    W0 = [w.cpu().clone() for w in drv.weights()]
    drv.train_batch()
    drv.synchronize()
    W1 = [w.cpu().clone() for w in drv.weights()]
    loss64, g64 = _chain_grads(hip, drv, cfg, data, W0, hs, torch.float64)
    loss32, g32 = _chain_grads(hip, drv, cfg, data, W0, hs, torch.float32)
    got = float(drv.loss.detach())
    print(f"GAT {layers} heads {hs} rates ({Q}, {P}): loss {got!r} float64 {loss64!r} "
          f"float32 chain {loss32!r}")
    assert abs(got - loss64) <= step_check.yardstick_bound(abs(loss32 - loss64) / abs(loss64),
                                                           step_check.C) * abs(loss64)
    step_check.check_step_grads(W0, W1, g64, g32, step_check.C, NAMES)
    # the dropout is there: the undropped chain's loss is another number
    plain, _ = _driver(E, data, layers, heads)
    plain.train_batch()
    plain.synchronize()
    assert abs(float(plain.loss.detach()) - got) > 1e-3 * abs(got)


def _three_steps(drv):
    for _ in range(3):
        drv.train_batch()
    drv.synchronize()
    return float(drv.loss.detach()), [w.clone() for w in drv.weights()]


@pytest.mark.parametrize("heads", [None, [8, 1]], ids=["single-head", "heads8-1"])
def test_zero_rates_and_determinism(E, data, heads):
    layers = [64, 64, 7]
    la, wa = _three_steps(_driver(E, data, layers, heads, readout=False)[0])
    lb, wb = _three_steps(_driver(E, data, layers, heads, readout=False, gat_attn_drop=0.0,
                                  gat_feat_drop=0.0)[0])
    assert la == lb
    for x, y in zip(wa, wb):
        assert torch.equal(x, y)
    lc, wc = _three_steps(_driver(E, data, layers, heads, readout=False, gat_attn_drop=Q,
                                  gat_feat_drop=P)[0])
    ld, wd = _three_steps(_driver(E, data, layers, heads, readout=False, gat_attn_drop=Q,
                                  gat_feat_drop=P)[0])
    assert lc == ld and lc != la
    for x, y in zip(wc, wd):
        assert torch.equal(x, y)


def test_evaluation_and_inference_do_not_see_the_options(E, data):
    layers, heads = [64, 64, 7], [8, 1]
    off, _ = _driver(E, data, layers, heads, readout=False)
    on, _ = _driver(E, data, layers, heads, readout=False, gat_attn_drop=Q, gat_feat_drop=P)
    on.train_batch()  # (moves the training offsets of `on` only)
    on.synchronize()
    on.set_weights(off.weights())
    seeds = torch.arange(0, 256, dtype=torch.int32)
    for x, y in zip(off.forward_eval(seeds, 0), on.forward_eval(seeds, 0)):
        assert torch.equal(x, y)
    ids = torch.arange(0, 1000, dtype=torch.int32)
    assert off.evaluate(ids) == on.evaluate(ids)
    assert torch.equal(off.infer_full_gat(), on.infer_full_gat())


def test_constructor_refusals(E, data):
    from nts import host

    def build(gat=True, **fields):
        cfg = host.gcn_config([64, 32, 7], [10, 5], 200, gat=gat, pipeline=False)
        for k, v in fields.items():  # (field by field: past gcn_config's own checks)
            setattr(cfg, k, v)
        return E.GCN_SAMPLE_ALLGPU_impl(data["G"], data["feat"], data["labels"], data["train"], cfg)

    for name in ("gat_attn_drop", "gat_feat_drop"):
        with pytest.raises(RuntimeError, match=f"{name} is not supported without gat "
                                               r"\(attention layers only\)"):
            build(gat=False, **{name: 0.5})
        for bad in (1.0, -0.1, float("nan")):
            with pytest.raises(RuntimeError, match=rf"{name} must be in \[0, 1\), got"):
                build(**{name: bad})
        with pytest.raises(ValueError, match=f"{name} is not supported without gat "
                                             r"\(attention layers only\)"):
            host.gcn_config([64, 32, 7], [10, 5], 200, gat=False, **{name: 0.5})
    # after the layer_norm checks: the pinned order of the earlier refusals holds
    with pytest.raises(RuntimeError, match="layer_norm is not supported with gat"):
        build(layer_norm=True, gat_attn_drop=2.0)
