"""One training step of the GAT driver against float64 autograd through the
reference's materialised-message chain (tests/gat_blocks.py), read out through
an Adam step that keeps each gradient's magnitude (tests/step_check.py): the
default step (epsilon = 1e-9) keeps only its sign.

The chain runs over the trained batch's own sampled layers (drv.last_layers):
H = X W, the GAT layer, twice, then nll_loss(log_softmax(.)).  All four
gradients (W0, W_att0, W1, W_att1) are held to the yardstick rule of
tests/test_gat_kernel.py with the readout's resolution added:

    err(recovered g) <= C * err(float32 chain) + 8 * 2^-24 + resolution / max|g64|.

Hidden width 32 runs the (VEC 4, NCH 1) kernels, 264 the (VEC 4, NCH 2) ones;
the output layer (7) the scalar path.
"""
import numpy as np
import pytest
import torch

import gat_blocks
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


def _chain_grads(drv, data, W0, dtype):
    """(loss, gradients of the four parameters) of the chain in `dtype`"""
    top, bottom = drv.last_layers
    W = [w.to(dtype).requires_grad_() for w in W0]
    X = data["feat"].cpu().to(dtype)[bottom["source"].cpu().long()]
    for l, lay in enumerate((bottom, top)):
        co, ri, dl = (lay[k].cpu().long() for k in ("column_offset", "row_indices", "dst_local_id"))
        assert X.shape[0] == lay["src_size"]
        H = X @ W[2 * l]
        X, _, _ = gat_blocks.gat_chain(H, W[2 * l + 1].view(-1), co, ri, dl, H.shape[1])
    tgt = data["labels"].cpu()[top["destination"].cpu().long()]
    loss = torch.nn.functional.nll_loss(X.log_softmax(1), tgt)
    loss.backward()
    return float(loss.detach()), [w.grad for w in W]


@pytest.mark.parametrize("hidden", [32, 264])
def test_gat_step_gradients_match_the_float64_chain(E, data, hidden):
    from nts import host
    cfg = step_check.readout(host.gcn_config([64, hidden, 7], [10, 5], 200, drop_rate=0.0,
                                             shuffle=False, gat=True, pipeline=False))
    drv = E.GCN_SAMPLE_ALLGPU_impl(data["G"], data["feat"], data["labels"], data["train"], cfg)
    W0 = [w.cpu().clone() for w in drv.weights()]
    assert [tuple(w.shape) for w in W0] == [(64, hidden), (2 * hidden, 1), (hidden, 7), (14, 1)]
    drv.train_batch()
    drv.synchronize()
    W1 = [w.cpu().clone() for w in drv.weights()]
    loss64, g64 = _chain_grads(drv, data, W0, torch.float64)
    loss32, g32 = _chain_grads(drv, data, W0, torch.float32)
    got = float(drv.loss.detach())
    print(f"GAT hidden {hidden}: loss {got!r} float64 {loss64!r} float32 chain {loss32!r}")
    assert abs(got - loss64) <= step_check.yardstick_bound(abs(loss32 - loss64) / abs(loss64),
                                                           step_check.C) * abs(loss64)
    step_check.check_step_grads(W0, W1, g64, g32, step_check.C, NAMES)
