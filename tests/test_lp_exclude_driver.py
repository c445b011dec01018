"""LinkPredictor with target-edge exclusion and filtered negatives:
the blocks keep their structure and the target edges' coefficients are 0 in
CSC and CSR, the loss is the one of the masked aggregation, determinism,
evaluate(), the default path, and the Cora job through ./nts_run."""
import math
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import linkpred_excl_ref as xref
import linkpred_ref as ref
import step_check as sc
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
V, LAYERS, FANOUT, B, K = 200, [16, 8, 8], [4, 3], 32, 2
STRUCT = ("destination", "column_offset", "row_indices", "sample_ans", "source", "row_offset",
          "column_indices")


@pytest.fixture(scope="module")
def data():
    from nts import host, synthetic
    E = host.ext()
    g = synthetic.chung_lu(V, 2400, 6.0, device=DEV, seed=4)
    G = E.FullyRepGraph.from_edges(g.src, g.dst, g.n_vertices)
    feat = synthetic.features(V, LAYERS[0], device=DEV)
    edges = torch.stack([g.src.cpu().to(torch.int64), g.dst.cpu().to(torch.int64)])
    return G, feat, edges.contiguous()  # train_edges: the graph's own edges


def _driver(data, layers=LAYERS, fanout=FANOUT, readout=False, **kw):
    from nts import host
    G, feat, train = data
    cfg = host.gcn_config(layers, fanout, B, drop_rate=0.0, pipeline=False, neg_per_pos=K, **kw)
    if readout:
        sc.readout(cfg)
    return host.link_predictor(G, feat, train, cfg)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _block_hits(lb, layer):
    """(hit per CSC edge, hit per CSR slot or None) from the block's structure
    and the batch's positives, in numpy"""
    table = xref.keys(_u32(lb["pos_src"]), _u32(lb["pos_dst"]), True)
    dest, co = _u32(layer["destination"]), _u32(layer["column_offset"]).astype(np.int64)
    dl = np.repeat(np.arange(layer["v_size"]), np.diff(co))
    hit_f = xref.hits(table, dest[dl], _u32(layer["sample_ans"]))
    if "row_offset" not in layer:
        return hit_f, None
    rows = xref.csr_rows(_u32(layer["row_offset"]), layer["e_size"])
    hit_b = xref.hits(table, dest[_u32(layer["column_indices"]).astype(np.int64)], _u32(layer["source"])[rows])
    return hit_f, hit_b


@pytest.mark.parametrize("weight", ["sum", "none"])
def test_blocks_keep_their_structure_and_target_edges_weigh_zero(data, weight):
    a = _driver(data, weight=weight)
    b = _driver(data, weight=weight, lp_exclude="reverse")
    a.train_batch(), b.train_batch()
    la, lb = a.last_batch(), b.last_batch()
    for k in ("pos_src", "pos_dst", "destination", "pair_u", "pair_v", "inc_offset", "inc_slot"):
        assert torch.equal(la[k], lb[k]), k
    total = 0
    for x, y in zip(la["layers"], lb["layers"]):
        for k in STRUCT:
            if k in x:
                assert torch.equal(x[k], y[k]), k
        hit_f, hit_b = _block_hits(lb, y)
        total += int(hit_f.sum())
        for hit, name in ((hit_f, "edge_weight_forward"), (hit_b, "edge_weight_backward")):
            if hit is None:
                continue
            got = y[name].cpu().numpy()
            want = x[name].cpu().numpy().copy() if weight == "sum" else np.ones(hit.size, np.float32)
            want[hit] = 0.0
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    print(f"weight {weight}: {total} sampled edges excluded")
    assert total >= 1, "the seed must give a batch that samples one of its own target edges"
    assert b.excluded_edges() == total and a.excluded_edges() == 0


def _one_layer(data):
    G, _, _ = data
    fmax = int((G.column_offset[1:] - G.column_offset[:-1]).max().item())
    return [LAYERS[0], 8], [fmax]  # every neighbour is taken


def _masked_embedding(W, feat, lb, w_unmasked, dtype):
    """(A_masked X) W of a one-layer model from the read-back block: the
    unmasked run's coefficients with the target edges dropped in numpy"""
    layer = lb["layers"][0]
    hit_f, _ = _block_hits(lb, layer)
    co = _u32(layer["column_offset"]).astype(np.int64)
    dl = np.repeat(np.arange(layer["v_size"]), np.diff(co))
    w = np.asarray(w_unmasked, np.float64).copy()
    w[hit_f] = 0.0
    A = np.zeros((layer["v_size"], layer["src_size"]), dtype)
    np.add.at(A, (dl, _u32(layer["row_indices"]).astype(np.int64)), w.astype(dtype))
    X = feat.cpu().numpy().astype(dtype)[_u32(layer["source"]).astype(np.int64)]
    return (A @ X) @ W.cpu().numpy().astype(dtype), int(hit_f.sum())


def _ref_batch(lb):
    P = lb["B"] * (1 + lb["K"])
    return {"pair_u": _u32(lb["pair_u"]).astype(np.int64), "pair_v": _u32(lb["pair_v"]).astype(np.int64),
            "inc_offset": _u32(lb["inc_offset"]).astype(np.int64), "inc_slot": _u32(lb["inc_slot"]).astype(np.int64),
            "v_size": lb["v_size"], "P": P, "B": lb["B"], "K": lb["K"]}


def test_loss_is_the_masked_aggregations(data):
    layers, fanout = _one_layer(data)
    a = _driver(data, layers, fanout)
    b = _driver(data, layers, fanout, lp_exclude="reverse")
    W0 = b.weights()[0]
    loss_a, loss_b = a.train_batch(), b.train_batch()
    la, lb = a.last_batch(), b.last_batch()
    w = la["layers"][0]["edge_weight_forward"].cpu().numpy()
    H64, n_hit = _masked_embedding(W0, data[1], lb, w, np.float64)
    H32, _ = _masked_embedding(W0, data[1], lb, w, np.float32)
    assert n_hit >= lb["B"] // 2  # the full neighbourhood holds every target edge
    rb = _ref_batch(lb)
    _, loss64, _ = ref.loss_and_grad(H64, rb)
    s32 = (H32[rb["pair_u"]] * H32[rb["pair_v"]]).sum(1, dtype=np.float32)
    y = (np.arange(rb["P"]) < rb["B"]).astype(np.float32)
    loss32 = float((np.maximum(s32, 0) - s32 * y + np.log1p(np.exp(-np.abs(s32)))).astype(np.float32).mean(dtype=np.float32))
    e_loss, e32 = abs(loss_b - loss64) / abs(loss64), abs(loss32 - loss64) / abs(loss64)
    print(f"loss reverse {loss_b:.7f} fp64 {loss64:.7f} err {e_loss:.2e} (fp32 chain {e32:.2e}); none {loss_a:.7f}")
    assert e_loss <= sc.yardstick_bound(e32, sc.C)
    assert loss_a != loss_b
    assert b.excluded_edges() == n_hit


def test_backward_runs_over_the_masked_csr(data):
    """two layers, the gradient read out of one Adam step: dW of the masked
    chain in float64 (the top hop's backward gathers over the masked CSR)"""
    a = _driver(data, readout=True)
    b = _driver(data, readout=True, lp_exclude="reverse")
    W0 = b.weights()
    a.train_batch(), b.train_batch()
    W1 = b.weights()
    la, lb = a.last_batch(), b.last_batch()

    def chain(dtype):
        Ws = [w.detach().cpu().to(dtype).requires_grad_(True) for w in W0]
        L = len(Ws)
        src = _u32(lb["layers"][L - 1]["source"]).astype(np.int64)
        X = data[1].cpu().to(dtype)[src]
        for l in range(L):
            x, y = la["layers"][L - 1 - l], lb["layers"][L - 1 - l]
            hit_f, _ = _block_hits(lb, y)
            w = x["edge_weight_forward"].cpu().numpy().astype(np.float64)
            w[hit_f] = 0.0
            co = _u32(y["column_offset"]).astype(np.int64)
            A = np.zeros((y["v_size"], y["src_size"]))
            np.add.at(A, (np.repeat(np.arange(y["v_size"]), np.diff(co)), _u32(y["row_indices"]).astype(np.int64)), w)
            X = (torch.from_numpy(A).to(dtype) @ X) @ Ws[l]
            if l < L - 1:
                X = torch.relu(X)
        u = torch.from_numpy(_u32(lb["pair_u"]).astype(np.int64))
        v = torch.from_numpy(_u32(lb["pair_v"]).astype(np.int64))
        s = (X[u] * X[v]).sum(1)
        t = torch.zeros_like(s)
        t[:lb["B"]] = 1
        torch.nn.functional.binary_cross_entropy_with_logits(s, t).backward()
        return [w.grad for w in Ws]

    sc.check_step_grads(W0, W1, chain(torch.float64), chain(torch.float32), sc.C)


def test_exclusion_changes_the_step_and_is_deterministic(data):
    a = _driver(data)
    b, c = _driver(data, lp_exclude="reverse"), _driver(data, lp_exclude="reverse")
    a.train_batch()
    assert b.train_batch() == c.train_batch()
    assert any(not torch.equal(x, y) for x, y in zip(a.weights(), b.weights()))
    for x, y in zip(b.weights(), c.weights()):
        assert torch.equal(x, y)
    assert b.excluded_edges() == c.excluded_edges()


def test_evaluate_repeats_and_leaves_the_training_stream_alone(data):
    val = data[2][:, 400:480].contiguous()
    a, b = _driver(data, lp_exclude="reverse"), _driver(data, lp_exclude="reverse")
    a.train_batch(), b.train_batch()
    n = a.excluded_edges()
    m1, m2 = a.evaluate(val), a.evaluate(val)
    assert m1 == m2 and 1.0 / (1 + K) <= m1 <= 1.0
    assert a.train_seq == b.train_seq == 1 and a.excluded_edges() == n
    assert a.train_batch() == b.train_batch()
    for x, y in zip(a.weights(), b.weights()):
        assert torch.equal(x, y)


def test_filtered_negatives_are_no_edges(data):
    from nts import host, synthetic
    Vs = 30
    rng = np.random.default_rng(8)
    s, d = rng.integers(0, Vs, 300), rng.integers(0, Vs, 300)
    s, d = np.concatenate([s, np.full(Vs, 7)]), np.concatenate([d, np.arange(Vs)])  # 7 -> every vertex
    st = torch.from_numpy(s.astype(np.int32)).to(DEV)
    dt = torch.from_numpy(d.astype(np.int32)).to(DEV)
    G = host.ext().FullyRepGraph.from_edges(st, dt, Vs)
    feat = synthetic.features(Vs, LAYERS[0], device=DEV)
    train = torch.stack([torch.from_numpy(s), torch.from_numpy(d)]).to(torch.int64)
    cfg = host.gcn_config(LAYERS, FANOUT, B, drop_rate=0.0, pipeline=False, neg_per_pos=K, shuffle=False,
                          filter_negatives=True, lp_exclude="self")
    drv = host.link_predictor(G, feat, train, cfg)
    edges = xref.edge_set(s, d)
    seen_unresolved = 0
    for step in range(11):  # the last batch holds the positives with head 7
        loss = drv.train_batch()
        lb = drv.last_batch()
        assert math.isfinite(loss) and lb["batch_seq"] == step
        ps, pd = _u32(lb["pos_src"]), _u32(lb["pos_dst"])
        want = xref.batch(ps, pd, K, Vs, 2000, step, edges)
        dest = _u32(lb["destination"])
        gu, gv = dest[_u32(lb["pair_u"])], dest[_u32(lb["pair_v"])]
        assert np.array_equal(gu, want["gu"]) and np.array_equal(gv, want["gv"])
        bad = sum(int(u) == int(w) or (int(u), int(w)) in edges or (int(w), int(u)) in edges
                  for u, w in zip(gu[lb["B"]:], gv[lb["B"]:]))
        assert bad == want["unresolved"] == drv.unresolved_negatives()
        assert all(int(u) == 7 for u, w in zip(gu[lb["B"]:], gv[lb["B"]:])
                   if int(u) == int(w) or (int(u), int(w)) in edges or (int(w), int(u)) in edges)
        seen_unresolved += bad
    assert seen_unresolved > 0, "the batches with head 7 must hold unresolvable negatives"


def test_all_options_off_is_the_default_path(data):
    a = _driver(data)
    b = _driver(data, lp_exclude="none", filter_negatives=False)
    for _ in range(3):
        assert a.train_batch() == b.train_batch()
    for x, y in zip(a.weights(), b.weights()):
        assert torch.equal(x, y)
    assert a.excluded_edges() == 0 and a.unresolved_negatives() == 0
    assert a.last_batch()["layers"][0]["edge_weight_forward"] is not None  # weight sum: as before


def test_cora_job_through_nts_run(tmp_path):
    cora = GOLDEN / "cora"
    cfg = tmp_path / "lp_cora.cfg"
    cfg.write_text(
        "ALGORITHM:LINKPREDSAMPLE\nVERTICES:2708\nLAYERS:1433-32-16\nFANOUT:5-5\nBATCH_SIZE:2048\n"
        "EPOCHS:1\nLEARN_RATE:0.01\nWEIGHT_DECAY:0.0001\nDROP_RATE:0.1\nNEG_PER_POS:2\n"
        "VAL_EDGE_RATE:0.1\nSEED:2000\nLP_EXCLUDE:reverse\nLP_FILTER_NEG:1\nLP_HOLDOUT_REMOVE:1\n"
        f"EDGE_FILE:{cora / 'cora.2708.edge.self'}\nFEATURE_FILE:{cora / 'cora.featuretable'}\n"
        f"LABEL_FILE:{cora / 'cora.labeltable'}\nMASK_FILE:{cora / 'cora.mask'}\n")
    r = subprocess.run([sys.executable, str(ROOT / "nts_run"), str(cfg)], capture_output=True, text=True,
                       timeout=600)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0
    assert re.search(r"1356 held out \(removed from the message-passing graph with their reverses: "
                     r"\d+ of \d+ edges carry messages\)", r.stdout)
    assert "target-edge exclusion reverse, filtered negatives on" in r.stdout
    m = re.search(r"^Epoch 0: Loss: (\S+) Val MRR: (\S+)$", r.stdout, flags=re.M)
    assert m, r.stdout
    assert math.isfinite(float(m.group(1))) and 0.0 < float(m.group(2)) <= 1.0
