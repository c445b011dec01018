"""GCN_SAMPLE_ALLGPU_impl::infer_full / evaluate_full: full-neighbour layer-wise
inference over the whole graph, against the CPU oracle chain run over the whole
graph, against the sampled path with unlimited fanout, and beside a training
pass it must not disturb.

Tolerance of the forward comparisons: rtol = atol = 1e-4, the project's
forward bar (tests/test_host.py).
"""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
C = 41


@pytest.fixture(scope="module")
def E():
    from nts import host
    return host.ext()


@pytest.fixture(scope="module")
def graph(E):
    from nts import synthetic
    g = synthetic.chung_lu(6000, 180000, 20.0, device=DEV, seed=3)
    G = E.FullyRepGraph.from_edges(g.src, g.dst, g.n_vertices)
    src = g.src.cpu().numpy().view(np.uint32)
    dst = g.dst.cpu().numpy().view(np.uint32)
    V = g.n_vertices
    col, rows = orc.build_csc(V, src, dst)
    od, idg = orc.degrees(V, src, dst)
    # the whole graph as one "sampled layer": the oracle's serial loop over it
    whole = dict(column_offset=col.astype(np.uint32), row_indices=rows,
                 source=np.arange(V, dtype=np.uint32), destination=np.arange(V, dtype=np.uint32),
                 v_size=V, src_size=V, e_size=int(src.size))
    return dict(G=G, V=V, od=od, idg=idg, whole=whole)


def _driver(E, graph, layers, fanout, batch, drop=0.0, **kw):
    from nts import host, synthetic
    feat = synthetic.features(graph["V"], layers[0], device=DEV)
    labels, masks = synthetic.labels_masks(graph["V"], layers[-1], device=DEV)
    train = torch.nonzero(masks == 0).flatten().to(torch.int32).cpu()
    cfg = host.gcn_config(layers, fanout, batch, learn_rate=0.01, drop_rate=drop, shuffle=False, **kw)
    drv = E.GCN_SAMPLE_ALLGPU_impl(graph["G"], feat, labels, train, cfg)
    return drv, feat, labels, masks


def _oracle_chain(graph, feat, W, mean):
    """relu((A X) W) per hidden layer, log_softmax((A X) W) at the top, A over the whole graph"""
    X = feat.cpu()
    for l, w in enumerate(W):
        Y = torch.from_numpy(orc.fuse_fwd(graph["whole"], X.numpy(), graph["od"], graph["idg"],
                                          weight_mean=mean, threads=8))
        Z = Y @ w
        X = Z.log_softmax(1) if l == len(W) - 1 else torch.relu(Z)
    return X


@pytest.mark.parametrize("weight", ["sum", "mean"])
@pytest.mark.parametrize("layers", [[602, 64, C], [48, 64, C], [100, 64, 64, C]])
def test_infer_full_matches_the_oracle_chain_over_the_whole_graph(E, graph, layers, weight):
    fanout = [10, 5, 5][:len(layers) - 1]
    drv, feat, _, _ = _driver(E, graph, layers, fanout, 256, weight=weight)
    out = drv.infer_full()
    assert tuple(out.shape) == (graph["V"], C)
    ref = _oracle_chain(graph, feat, [w.cpu() for w in drv.weights()], weight == "mean")
    err = (out.cpu() - ref).abs()
    print(f"infer_full {layers} {weight}: max |diff| {float(err.max()):.3e}, "
          f"max |ref| {float(ref.abs().max()):.3e}, rows {out.shape[0]}")
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-4, atol=1e-4)
    assert torch.equal(out, drv.infer_full())  # no random stream anywhere


def test_infer_full_agrees_with_the_sampled_path_at_unlimited_fanout(E, graph):
    layers = [100, 64, C]
    a, *_ = _driver(E, graph, layers, [10, 5], 256)
    b, *_ = _driver(E, graph, layers, [-1, -1], 64)
    b.set_weights(a.weights())
    seeds = torch.arange(5, 5 + 64 * 90, 90, dtype=torch.int32)
    assert seeds.numel() == 64
    full = a.infer_full()
    sampled = b.forward_eval(seeds, 0)[-1]
    print(f"sampled fanout -1 vs infer_full: max |diff| "
          f"{float((sampled.cpu() - full.cpu()[seeds.long()]).abs().max()):.3e} over {seeds.numel()} seeds")
    torch.testing.assert_close(sampled.cpu(), full.cpu()[seeds.long()], rtol=1e-4, atol=1e-4)


def test_evaluate_full_is_the_argmax_count_of_infer_full(E, graph):
    drv, _, labels, masks = _driver(E, graph, [48, 64, C], [10, 5], 256)
    for _ in range(3):  # some training, so the rows are not all alike
        drv.train_batch()
    ids = torch.nonzero(masks.cpu() == 2).flatten().to(torch.int32)
    assert ids.numel() > 100
    pred = drv.infer_full().cpu().argmax(1)
    correct = int((pred[ids.long()] == labels.cpu()[ids.long()]).sum())
    got = drv.evaluate_full(ids)
    print(f"evaluate_full {got!r} vs host count {correct} / {ids.numel()}")
    assert got == correct / ids.numel()
    assert drv.evaluate_full(torch.empty(0, dtype=torch.int32)) == 0.0


@pytest.mark.parametrize("pipeline", [True, False])
def test_evaluate_full_does_not_disturb_training(E, graph, pipeline):
    """3 batches, evaluate_full, 3 more: losses and weights bit-identical to a
    driver that never called it (dropout on: the mask offsets, the sampler's
    stream and the prefetched batch are all untouched)."""
    layers = [100, 64, C]
    a, _, _, masks = _driver(E, graph, layers, [10, 5], 256, drop=0.5, pipeline=pipeline)
    b, *_ = _driver(E, graph, layers, [10, 5], 256, drop=0.5, pipeline=pipeline)
    ids = torch.nonzero(masks.cpu() == 1).flatten().to(torch.int32)
    la, lb = [], []
    for step in range(6):
        if step == 3:
            a.evaluate_full(ids)
        a.train_batch()
        a.synchronize()
        la.append(float(a.loss.detach()))
        b.train_batch()
        b.synchronize()
        lb.append(float(b.loss.detach()))
    print(f"losses with evaluate_full {la}\nlosses without       {lb}")
    assert la == lb
    for x, y in zip(a.weights(), b.weights()):
        assert torch.equal(x, y)


def test_infer_full_refuses_gat_and_up_degree(E, graph):
    gat, *_ = _driver(E, graph, [64, 32, 7], [10, 5], 200, gat=True)
    with pytest.raises(RuntimeError, match="GAT"):
        gat.infer_full()
    up, *_ = _driver(E, graph, [64, 32, 7], [10, 5], 200, up_degree=True)
    with pytest.raises(RuntimeError, match="UP_DEGREE"):
        up.infer_full()
    with pytest.raises(RuntimeError, match="UP_DEGREE"):
        up.evaluate_full(torch.arange(10, dtype=torch.int32))


def test_runner_prints_the_full_scores_only_when_asked(tmp_path):
    """FULL_INFERENCE:1 adds the two Full ... Acc lines and the two result
    keys after the last epoch; without the key the runner reports what it did."""
    import shutil
    from conftest import GOLDEN
    from nts import run
    for f in ("cora.2708.edge.self", "cora.featuretable.zip", "cora.labeltable", "cora.mask"):
        shutil.copy(GOLDEN / "cora" / f, tmp_path / f)
    text = (GOLDEN / "cora" / "gcn_cora_sample.cfg").read_text()
    (tmp_path / "full.cfg").write_text(text + "FULL_INFERENCE:1\n")
    (tmp_path / "plain.cfg").write_text(text)
    full, plain = [], []
    r1 = run.run(tmp_path / "full.cfg", epochs=1, out=full.append)
    r0 = run.run(tmp_path / "plain.cfg", epochs=1, out=plain.append)
    print("\n".join(full[-2:]))
    assert [l.split()[:2] for l in full[-2:]] == [["Full", "Eval"], ["Full", "Test"]]
    for line, key in zip(full[-2:], ("full_eval_acc", "full_test_acc")):
        _, _, _, acc, correct, n = line.split()
        assert int(n) > 0 and int(correct) == round(r1[key] * int(n))
        assert abs(float(acc) - r1[key]) < 1e-6 and 0.0 <= r1[key] <= 1.0
    assert not any(l.startswith("Full") for l in plain)
    assert "full_eval_acc" not in r0 and "full_test_acc" not in r0
    # the same job up to the extra lines (sampled scores included: same streams)
    keep = ("Train Acc:", "Eval Acc:", "Test Acc:")
    assert [l for l in full if l.startswith(keep)] == [l for l in plain if l.startswith(keep)]
