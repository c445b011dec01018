"""GCN_SAMPLE_ALLGPU_impl with 80 classes: above 64 classes the driver now takes
the fused output layer + softmax loss (nts_hip_linear_xent_train / _fwd, the
wide form) where it ran the libtorch chain; `fuse_loss = false` keeps that
chain, which is the comparison here.

Bars: one training step within rtol = atol = 1e-5 (loss and every updated
weight), the bar tests/test_multilabel_driver.py holds for the fused BCE layer.
Accuracy counters of the two drivers may differ by the rows whose two best
logits are within 1e-4 (the fp32 logits of two summation orders).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LAYERS, FANOUT, BATCH = [64, 32, 80], [5, 5], 256
V = 3000


@pytest.fixture(scope="module")
def E():
    from nts import host
    return host.ext()


@pytest.fixture(scope="module")
def data(E):
    from nts import synthetic
    g = synthetic.chung_lu(V, 45000, 10.0, device=DEV, seed=5)
    G = E.FullyRepGraph.from_edges(g.src, g.dst, g.n_vertices)
    feat = synthetic.features(V, LAYERS[0], device=DEV)
    # learnable classes: the largest of 80 random projections of the features
    proj = torch.randn(LAYERS[0], LAYERS[-1], device=DEV,
                       generator=torch.Generator(device=DEV).manual_seed(17))
    labels = (feat @ proj).argmax(1)
    assert int(labels.max()) > 64
    train = torch.arange(0, 2000, dtype=torch.int32)
    return dict(G=G, feat=feat, labels=labels, train=train)


def _driver(E, data, **kw):
    from nts import host
    cfg = host.gcn_config(LAYERS, FANOUT, BATCH, learn_rate=0.01, drop_rate=0.0, shuffle=False, **kw)
    return E.GCN_SAMPLE_ALLGPU_impl(data["G"], data["feat"], data["labels"], data["train"], cfg)


def _near_ties(drv, seeds, seq):
    """rows of the eval-mode forward over `seeds` (sample number seq) whose two
    best classes are within 1e-4"""
    out = drv.forward_eval(seeds, seq)[-1]
    top2 = out.double().topk(2, 1).values
    return int((top2[:, 0] - top2[:, 1] <= 1e-4).sum())


def test_one_training_step_fused_equals_the_libtorch_chain(E, data):
    assert E.hip_linear_xent_supported(LAYERS[-2], LAYERS[-1])  # not the fallback against itself
    a = _driver(E, data, fuse_loss=True)
    b = _driver(E, data, fuse_loss=False)
    for x, y in zip(a.weights(), b.weights()):
        assert torch.equal(x, y)
    # training batch 0 is the first 256 training vertices under sample number 0
    ties = _near_ties(_driver(E, data, fuse_loss=False), data["train"][:BATCH], 0)
    a.train_batch()
    b.train_batch()
    a.synchronize()
    b.synchronize()
    print(f"one step: fused loss {float(a.loss.detach()):.7f}, libtorch chain "
          f"{float(b.loss.detach()):.7f}; correct {a.train_correct()} / {b.train_correct()}, "
          f"{ties} near ties")
    torch.testing.assert_close(a.loss.detach().cpu(), b.loss.detach().cpu(), rtol=1e-5, atol=1e-5)
    for x, y in zip(a.weights(), b.weights()):
        torch.testing.assert_close(x, y, rtol=1e-5, atol=1e-5)
    assert abs(a.train_correct() - b.train_correct()) <= ties
    # the sampled evaluation: the forward-only fused call against argmax of the chain
    ids = torch.arange(2000, 2600, dtype=torch.int32)  # batches of 256, 256, 88
    ties = sum(_near_ties(a, ids[s:s + BATCH], (1 << 40) + k)
               for k, s in enumerate(range(0, ids.numel(), BATCH)))
    ea, eb = a.evaluate(ids), b.evaluate(ids)
    print(f"evaluate: fused {ea!r}, libtorch chain {eb!r}, {ties} near ties")
    assert 0.0 <= ea <= 1.0
    assert abs(ea - eb) * ids.numel() <= ties + 1e-6


def test_training_lowers_the_loss(E, data):
    drv = _driver(E, data)
    losses = []
    for _ in range(30):
        if not drv.sample_not_finished():
            drv.restart()
        drv.train_batch()
        drv.synchronize()
        losses.append(float(drv.loss.detach()))
    print(f"loss of step 1: {losses[0]:.5f}, after 30 steps: {losses[-1]:.5f}")
    assert all(l == l and abs(l) != float("inf") for l in losses) and losses[-1] < losses[0]
