"""LinkPredictor (nts/host/linkpred.cpp): one training step
against a float64 restatement built from last_batch(), determinism, an
evaluation that leaves the training stream alone, and the Cora job through
the cfg runner."""
import numpy as np
import pytest
import torch

import linkpred_ref as ref
import step_check as sc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LAYERS, FANOUT, B, K = [16, 8, 8], [3, 3], 32, 2


@pytest.fixture(scope="module")
def data():
    from nts import host, synthetic
    E = host.ext()
    g = synthetic.chung_lu(200, 2400, 6.0, device=DEV, seed=4)
    G = E.FullyRepGraph.from_edges(g.src, g.dst, g.n_vertices)
    feat = synthetic.features(200, LAYERS[0], device=DEV)
    edges = torch.stack([g.src.cpu().to(torch.int64), g.dst.cpu().to(torch.int64)])
    return G, feat, edges[:, :320].contiguous(), edges[:, 320:400].contiguous()


def _driver(data, **kw):
    from nts import host
    G, feat, train, _ = data
    cfg = host.gcn_config(LAYERS, FANOUT, B, drop_rate=0.0, pipeline=False, neg_per_pos=K, **kw)
    return host.link_predictor(G, feat, train, cfg), cfg


def _dense(layer, dtype):
    """A [v_size, src_size] of a sampled block's CSC"""
    co = layer["column_offset"].cpu().numpy().view(np.uint32).astype(np.int64)
    ri = layer["row_indices"].cpu().numpy().view(np.uint32).astype(np.int64)
    w = layer["edge_weight_forward"].cpu().numpy().astype(np.float64)
    A = np.zeros((layer["v_size"], layer["src_size"]))
    np.add.at(A, (np.repeat(np.arange(layer["v_size"]), np.diff(co)), ri), w)
    return torch.from_numpy(A).to(dtype)


def _pair_loss(X, lb):
    """(mean BCE of the batch's pair scores on the embeddings X, the scores)"""
    u = torch.from_numpy(lb["pair_u"].cpu().numpy().view(np.uint32).astype(np.int64))
    v = torch.from_numpy(lb["pair_v"].cpu().numpy().view(np.uint32).astype(np.int64))
    s = (X[u] * X[v]).sum(1)
    y = torch.zeros_like(s)
    y[:lb["B"]] = 1
    return torch.nn.functional.binary_cross_entropy_with_logits(s, y), s


def _chain(W, feat, lb, dtype):
    """the step's loss and weight gradients in libtorch at `dtype`"""
    layers = lb["layers"]
    L = len(W)
    Ws = [w.detach().cpu().to(dtype).requires_grad_(True) for w in W]
    src = layers[L - 1]["source"].cpu().numpy().view(np.uint32).astype(np.int64)
    X = feat.cpu().to(dtype)[src]
    for l in range(L):
        Y = _dense(layers[L - 1 - l], dtype) @ X
        X = Y @ Ws[l]
        if l < L - 1:
            X = torch.relu(X)
    loss, s = _pair_loss(X, lb)
    loss.backward()
    return float(loss.detach()), [w.grad for w in Ws], s.detach()


def test_one_step_matches_the_float64_restatement(data):
    G, feat, train, _ = data
    from nts import host
    cfg = sc.readout(host.gcn_config(LAYERS, FANOUT, B, drop_rate=0.0, pipeline=False, neg_per_pos=K))
    drv = host.link_predictor(G, feat, train, cfg)
    W0 = drv.weights()
    loss = drv.train_batch()
    W1 = drv.weights()
    lb = drv.last_batch()
    assert lb["B"] == B and lb["K"] == K and lb["batch_seq"] == 0
    # the batch is the reference's for these positives
    want = ref.batch(lb["pos_src"].cpu().numpy().view(np.uint32), lb["pos_dst"].cpu().numpy().view(np.uint32),
                     K, 200, 2000, 0)
    for k in ("destination", "pair_u", "pair_v", "inc_offset", "inc_slot"):
        assert np.array_equal(lb[k].cpu().numpy().view(np.uint32), want[k]), k
    assert lb["v_size"] == want["v_size"] == lb["layers"][0]["v_size"]
    assert torch.equal(lb["layers"][0]["destination"], lb["destination"])
    loss64, g64, s64 = _chain(W0, feat, lb, torch.float64)
    loss32, g32, _ = _chain(W0, feat, lb, torch.float32)
    e_loss, e32 = abs(loss - loss64) / abs(loss64), abs(loss32 - loss64) / abs(loss64)
    print(f"loss driver {loss:.7f} fp64 {loss64:.7f} err {e_loss:.2e} (fp32 chain {e32:.2e})")
    assert e_loss <= sc.yardstick_bound(e32, sc.C)
    assert sc.err(lb["score"], s64) <= sc.yardstick_bound(1e-6, sc.C)
    sc.check_step_grads(W0, W1, g64, g32, sc.C)


def test_first_step_of_two_drivers_is_identical(data):
    a, _ = _driver(data)
    b, _ = _driver(data)
    la, lb_ = a.train_batch(), b.train_batch()
    assert la == lb_
    for x, y in zip(a.weights(), b.weights()):
        assert torch.equal(x, y)
    assert torch.equal(a.last_batch()["score"], b.last_batch()["score"])


def test_evaluate_repeats_and_leaves_the_training_stream_alone(data):
    _, _, _, val = data
    a, _ = _driver(data)
    b, _ = _driver(data)
    a.train_batch(), b.train_batch()
    m1, m2 = a.evaluate(val), a.evaluate(val)
    assert m1 == m2 and 1.0 / (1 + K) <= m1 <= 1.0
    assert a.train_seq == b.train_seq == 1
    assert a.train_batch() == b.train_batch()
    for x, y in zip(a.weights(), b.weights()):
        assert torch.equal(x, y)


def test_cora_job_learns_through_the_cfg_runner(tmp_path):
    from nts import run
    cora = GOLDEN / "cora"
    cfg = tmp_path / "lp_cora.cfg"
    cfg.write_text(
        "ALGORITHM:LINKPREDSAMPLE\nVERTICES:2708\nLAYERS:1433-64-32\nFANOUT:10-5\nBATCH_SIZE:512\n"
        "EPOCHS:4\nLEARN_RATE:0.01\nWEIGHT_DECAY:0.0001\nDROP_RATE:0.1\nNEG_PER_POS:4\n"
        "VAL_EDGE_RATE:0.1\nSEED:2000\n"
        f"EDGE_FILE:{cora / 'cora.2708.edge.self'}\nFEATURE_FILE:{cora / 'cora.featuretable'}\n"
        f"LABEL_FILE:{cora / 'cora.labeltable'}\nMASK_FILE:{cora / 'cora.mask'}\n")
    lines = []
    res = run.run(cfg, out=lines.append)
    print("\n".join(lines))
    ep = res["epochs"]
    assert len(ep) == 4 and res["n_val_edges"] == 1356
    assert sum(l.startswith("Epoch ") and "Loss:" in l and "Val MRR:" in l for l in lines) == 4
    assert ep[-1]["val_mrr"] > res["val_mrr_init"], (res["val_mrr_init"], [e["val_mrr"] for e in ep])
    assert ep[-1]["loss"] < ep[0]["loss"], [e["loss"] for e in ep]
