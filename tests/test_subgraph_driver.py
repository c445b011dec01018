"""Subgraph-sampled training through the C++ driver (gcn_config(subgraph=True),
DESIGN §8w) on the Cora fixtures: the trained blocks against the numpy
reference of tests/subgraph_ref.py, dropped training steps against the float64
chain of tests/dropout_chain.py by tests/step_check.py's criterion, the
whole-graph batch against infer_full(), the pipeline, the option off, and the
cfg runner.
"""
import shutil

import numpy as np
import pytest
import torch

import dropout_chain as dc
import step_check as sc
import subgraph_ref as sr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEED = 2000
V = 2708
L3, L2, BATCH = [1433, 32, 16, 7], [1433, 32, 7], 64


@pytest.fixture(scope="module")
def E():
    from nts import host
    return host.ext()


@pytest.fixture(scope="module")
def cora(E):
    from nts import dataloader
    c = GOLDEN / "cora"
    src, dst = dataloader.read_edge_file(c / "cora.2708.edge.self")
    feats, labels, masks = dataloader.read_feature_label_mask(
        c / "cora.featuretable.zip", c / "cora.labeltable", c / "cora.mask", V, 1433)
    G = E.FullyRepGraph.from_edges(torch.from_numpy(src.view(np.int32)).to(DEV),
                                   torch.from_numpy(dst.view(np.int32)).to(DEV), V)
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    host_graph = (G.column_offset.cpu().numpy().view(np.uint64), u32(G.row_indices),
                  u32(G.in_degree), u32(G.out_degree))
    train = torch.from_numpy(np.nonzero(masks == dataloader.MASK_TRAIN)[0].astype(np.int32))
    return dict(G=G, feat=torch.from_numpy(feats).to(DEV), labels=torch.from_numpy(labels).to(DEV),
                train=train, host=host_graph, E=int(src.size))


def _driver(E, data, layers, train=None, batch=BATCH, readout=False, **kw):
    from nts import host
    kw.setdefault("drop_rate", 0.0)
    cfg = host.gcn_config(layers, [-1] * (len(layers) - 1), batch, learn_rate=0.01, shuffle=False,
                          seed=SEED, **kw)
    if readout:
        sc.readout(cfg)
    return E.GCN_SAMPLE_ALLGPU_impl(data["G"], data["feat"], data["labels"],
                                    data["train"] if train is None else train, cfg)


def _step(drv):
    drv.train_batch()
    drv.synchronize()
    return drv.last_layers


def _np(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def _assert_reference(lays, data, seeds, walk, batch_seq, flags, merge):
    col, rows, idg, od = data["host"]
    ref = sr.subgraph_batch(col, rows, idg, od, seeds, len(lays), walk, SEED, batch_seq, flags, merge)
    checked = 0
    for got, want in zip(lays, ref):
        assert (got["v_size"], got["e_size"], got["src_size"]) == (
            want["v_size"], want["e_size"], want["src_size"])
        for k, w in want.items():
            t = got.get(k) if isinstance(w, np.ndarray) else None
            if not isinstance(t, torch.Tensor):
                continue
            assert np.array_equal(_np(t), w), k
            checked += 1
    assert checked >= 6 * len(lays)
    return ref


FORMS = {
    "base": (dict(), sr.W_SUM, False),
    "up_degree": (dict(up_degree=True), sr.W_SUM | sr.W_UP_DEGREE, False),
    "root_weight": (dict(root_weight=True), sr.W_SUM, True),
    "mean": (dict(weight="mean"), sr.W_MEAN, False),
}


@pytest.mark.parametrize("walk", [0, 2])
@pytest.mark.parametrize("form", list(FORMS))
def test_trained_blocks_are_the_reference(E, cora, form, walk):
    kw, flags, merge = FORMS[form]
    drv = _driver(E, cora, L3, subgraph=True, subgraph_walk=walk, **kw)
    seeds = cora["train"].numpy().view(np.uint32)
    for step in range(2):  # the second batch too: batch_seq keys the walks
        lays = _step(drv)
        ref = _assert_reference(lays, cora, seeds[step * BATCH:(step + 1) * BATCH], walk, step, flags,
                                merge)
    S = ref[0]["source"]
    assert (S.size == BATCH) == (walk == 0) and S.size <= BATCH * (1 + walk)
    assert set(seeds[BATCH:2 * BATCH].tolist()) <= set(S.tolist())
    # layers 1 .. L-1 are one block, S x S
    a, b = lays[1], lays[2]
    assert np.array_equal(_np(a["destination"]), S) and np.array_equal(_np(b["source"]), S)
    for k in ("destination", "column_offset", "row_indices", "sample_ans", "source",
              "edge_weight_forward"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("form", ["base", "up_degree", "root_weight"])
def test_dropped_steps_hold_to_the_float64_chain(E, cora, form):
    """the first step's gradients by the readout, then three steps' losses with
    the offsets of tests/dropout_chain.py, all by step_check's criterion"""
    kw, _, _ = FORMS[form]
    root, p, L = form == "root_weight", 0.5, 2
    opts = dict(subgraph=True, subgraph_walk=2, drop_rate=p, **kw)

    def run(lays, ws, dtype, first_offset):
        P, loss, _, masks = dc.chain(lays, cora, ws, dtype, p, SEED, first_offset, root=root)
        loss.backward()
        return [q.grad for q in P], float(loss.detach()), masks

    drv = _driver(E, cora, L2, readout=True, **opts)
    W0 = [w.cpu().clone() for w in drv.weights()]
    lays = _step(drv)
    W1 = [w.cpu().clone() for w in drv.weights()]
    g64, loss64, masks = run(lays, W0, torch.float64, 0)
    g32, loss32, _ = run(lays, W0, torch.float32, 0)
    assert all(bool(m.any()) and not bool(m.all()) for m in masks)
    print(f"subgraph {form}: readout step")
    got = float(drv.loss.detach())
    assert abs(got - loss64) <= sc.yardstick_bound(abs(loss32 - loss64) / abs(loss64), sc.C) * abs(loss64)
    sc.check_step_grads(W0, W1, g64, g32, sc.C)

    drv = _driver(E, cora, L2, **opts)
    for step in range(3):
        W = [w.cpu().clone() for w in drv.weights()]
        lays = _step(drv)
        got = float(drv.loss.detach())
        off = dc.offsets(step, L)[0]
        loss64, loss32 = run(lays, W, torch.float64, off)[1], run(lays, W, torch.float32, off)[1]
        bound = sc.yardstick_bound(abs(loss32 - loss64) / abs(loss64), sc.C)
        print(f"subgraph {form} step {step}: loss {got!r} float64 {loss64!r} float32 chain {loss32!r} "
              f"err {abs(got - loss64) / abs(loss64):.3e} bound {bound:.3e}")
        assert abs(got - loss64) <= bound * abs(loss64)


@pytest.mark.parametrize("weight", ["sum", "mean"])
def test_one_batch_of_every_vertex_is_the_whole_graph(E, cora, weight):
    """walk 0 and a batch holding all 2,708 vertices: the induced block is the
    graph itself, and the eval forward over it equals infer_full() to the bar
    tests/test_full_infer_driver.py applies between the sampled and full passes"""
    everyone = torch.arange(V, dtype=torch.int32)
    drv = _driver(E, cora, L2, train=everyone, batch=V, subgraph=True, subgraph_walk=0,
                  weight=weight)
    full = drv.infer_full()
    sampled = drv.forward_eval(everyone, 0)[-1]
    print(f"subgraph whole-graph batch vs infer_full ({weight}): max |diff| "
          f"{float((sampled - full).abs().max()):.3e}")
    torch.testing.assert_close(sampled.cpu(), full.cpu(), rtol=1e-4, atol=1e-4)
    lays = _step(drv)
    col, rows, _, _ = cora["host"]
    for lay in lays:
        assert (lay["v_size"], lay["e_size"], lay["src_size"]) == (V, cora["E"], V)
        assert np.array_equal(_np(lay["column_offset"]).astype(np.uint64), col)
        assert np.array_equal(_np(lay["sample_ans"]), rows)
        assert np.array_equal(_np(lay["row_indices"]), rows)  # source is 0 .. V-1


def _three_steps(drv):
    out = []
    for _ in range(3):
        lays = _step(drv)
        out.append(([{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in l.items()}
                     for l in lays], float(drv.loss.detach())))
    return out


def test_pipelined_and_unpipelined_drivers_give_the_same_blocks(E, cora):
    kw = dict(subgraph=True, subgraph_walk=2, drop_rate=0.5)
    on = _three_steps(_driver(E, cora, L3, pipeline=True, **kw))
    off = _three_steps(_driver(E, cora, L3, pipeline=False, **kw))
    for (la, a), (lb, b) in zip(on, off):
        assert a == b and np.isfinite(a)
        for x, y in zip(la, lb):
            assert x.keys() == y.keys()
            for k, v in x.items():
                assert torch.equal(v, y[k]) if isinstance(v, torch.Tensor) else v == y[k], k
    assert not torch.equal(on[0][0][0]["source"], on[1][0][0]["source"])


def test_option_off_trains_as_without_the_fields(E, cora):
    """three steps of the neighbour-sampled job, the three fields untouched
    against set beside subgraph = false: the same weights bit for bit"""
    from nts import host

    def drv(edit):
        cfg = host.gcn_config(L2, [10, 5], BATCH, learn_rate=0.01, shuffle=False, seed=SEED,
                              drop_rate=0.5)
        edit(cfg)
        d = E.GCN_SAMPLE_ALLGPU_impl(cora["G"], cora["feat"], cora["labels"], cora["train"], cfg)
        for _ in range(3):
            _step(d)
        return d

    def fields(cfg):
        cfg.subgraph_walk, cfg.subgraph_edge_cap = 3, 5

    a, b = drv(lambda cfg: None), drv(fields)
    for x, y in zip(a.weights(), b.weights()):
        assert torch.equal(x, y)
    for x, y in zip(a.last_layers, b.last_layers):
        assert torch.equal(x["row_indices"], y["row_indices"]) and x["e_size"] == y["e_size"]
    assert a.last_layers[1]["src_size"] > BATCH * 3  # a frontier that grew per hop, not a set


def test_a_block_above_the_edge_capacity_names_the_option(E, cora):
    drv = _driver(E, cora, L2, subgraph=True, subgraph_walk=2, subgraph_edge_cap=20, pipeline=False)
    with pytest.raises(RuntimeError, match=r"exceeded its capacity \(subgraph_edge_cap\)"):
        drv.train_batch()


def test_evaluate_samples_subgraphs_and_is_deterministic(E, cora):
    ids = torch.arange(1000, 1500, dtype=torch.int32)
    scores = []
    for _ in range(2):
        drv = _driver(E, cora, L2, subgraph=True, subgraph_walk=2, drop_rate=0.5)
        for _ in range(3):
            _step(drv)
        scores.append([drv.evaluate(ids), drv.evaluate(ids)])
    assert scores[0] == scores[1] and all(0.0 <= x <= 1.0 for x in scores[0])


def test_cfg_runner_trains_cora_with_subgraph_batches(tmp_path):
    """SUBGRAPH:1, SUBGRAPH_WALK:2, FANOUT:-1--1 through nts.run to the end;
    the full-neighbour test accuracy is above the share of the most frequent label"""
    from nts import run
    for f in ("cora.2708.edge.self", "cora.featuretable.zip", "cora.labeltable", "cora.mask"):
        shutil.copy(GOLDEN / "cora" / f, tmp_path / f)
    text = (GOLDEN / "cora" / "gcn_cora_sample.cfg").read_text().replace("FANOUT:25-10", "FANOUT:-1--1")
    (tmp_path / "job.cfg").write_text(text + "SUBGRAPH:1\nSUBGRAPH_WALK:2\nFULL_INFERENCE:1\n")
    lines = []
    res = run.run(tmp_path / "job.cfg", epochs=3, out=lines.append)
    assert len(res["epochs"]) == 3 and all(np.isfinite(e["loss"]) for e in res["epochs"])
    labels = np.array([int(l.split()[1]) for l in (GOLDEN / "cora" / "cora.labeltable")
                       .read_text().splitlines() if l.strip()])
    share = np.bincount(labels).max() / labels.size
    print(f"cora, subgraph walk 2, 3 epochs: sampled test acc {res['epochs'][-1]['test_acc']:.4f}, "
          f"full eval acc {res['full_eval_acc']:.4f}, full test acc {res['full_test_acc']:.4f}; "
          f"most frequent label {share:.4f}")
    assert res["full_test_acc"] > share and res["full_eval_acc"] > share
