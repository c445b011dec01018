"""GCN_SAMPLE_ALLGPU_impl::infer_full_gat / evaluate_full_gat: full-neighbour
inference of a GAT driver over the whole graph (one GEMM, the per-vertex scores
and one fused attention pass per layer), against the float64 whole-graph chain
of tests/gat_heads_blocks.py built from drv.weights(), against the sampled path
at unlimited fanout, beside a training pass it must not disturb, and through
the runner (FULL_INFERENCE:1 with a GAT algorithm).

Bound of the forward comparisons, the yardstick rule of DESIGN §8b with q32 the
same chain in float32 and err(x) = max|x - q64| / max|q64| over the [V, 7]
log-softmax rows (over the 64 seeds' rows in the sampled comparison):

    err(driver) <= C * err(q32) + 8 * 2^-24,   C = step_check.C = 8.

Measured on an MI355X the ratios err(driver) / err(q32) are
1.47, 1.37, 1.49 and 1.36 for the four models below, and 1.15 / 1.15 for the
full and the sampled side of the unlimited-fanout comparison, whose rows came
out bit-identical (max |diff| 0).
"""
import shutil

import numpy as np
import pytest
import torch

import gat_heads_blocks as ghb
from step_check import C, err, yardstick_bound

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODELS = [([64, 64, 7], None), ([64, 64, 7], [8, 1]), ([64, 64, 7], [8, 8]), ([64, 264, 7], [2, 1])]
IDS = ["64-64-7", "64-64-7-heads8-1", "64-64-7-heads8-8", "64-264-7-heads2-1"]


@pytest.fixture(scope="module")
def E():
    from nts import host
    return host.ext()


@pytest.fixture(scope="module")
def data(E):
    from nts import synthetic
    g = synthetic.chung_lu(6000, 180000, 20.0, device=DEV, seed=3)
    V = g.n_vertices
    G = E.FullyRepGraph.from_edges(g.src, g.dst, V)
    feat = synthetic.features(V, 64, device=DEV)
    labels, masks = synthetic.labels_masks(V, 7, device=DEV)
    train = torch.nonzero(masks == 0).flatten().to(torch.int32).cpu()
    src = g.src.cpu().numpy().view(np.uint32).astype(np.int64)
    dst = g.dst.cpu().numpy().view(np.uint32).astype(np.int64)
    order = np.argsort(dst, kind="stable")  # the global CSC
    co = np.zeros(V + 1, np.int64)
    co[1:] = np.cumsum(np.bincount(dst, minlength=V))
    return dict(G=G, V=V, feat=feat, labels=labels, masks=masks, train=train,
                co=torch.from_numpy(co), ri=torch.from_numpy(src[order]))


def _driver(E, data, layers, heads, fanout=(10, 5), batch=200, pipeline=False, **kw):
    from nts import host
    cfg = host.gcn_config(layers, list(fanout), batch, drop_rate=0.0, shuffle=False, gat=True,
                          pipeline=pipeline, gat_heads=heads, **kw)
    return E.GCN_SAMPLE_ALLGPU_impl(data["G"], data["feat"], data["labels"], data["train"], cfg)


def _chain(data, W, heads, dtype):
    """log_softmax of the whole-graph GAT chain in `dtype`: [V, C]"""
    L = len(W) // 2
    heads = heads or [1] * L
    X = data["feat"].cpu().to(dtype)
    dl = torch.arange(data["V"])
    for l in range(L):
        H = X @ W[2 * l].cpu().to(dtype)
        K = heads[l]
        X, _, _ = ghb.heads_chain(H, W[2 * l + 1].cpu().to(dtype).view(-1), data["co"], data["ri"],
                                  dl, K, H.shape[1] // K, mean=l == L - 1 and K > 1)
    return X.log_softmax(1)


def _held(tag, got, r64, r32):
    ek, e32 = err(got, r64), err(r32, r64)
    bound = yardstick_bound(e32, C)
    print(f"{tag}: err(driver) {ek:.3e} err(fp32 chain) {e32:.3e} "
          f"ratio {ek / max(e32, 2.0 ** -30):.2f} bound {bound:.3e}")
    assert ek <= bound, f"{tag}: {ek:.3e} > {bound:.3e}"


@pytest.mark.parametrize("layers,heads", MODELS, ids=IDS)
def test_infer_full_gat_matches_the_float64_chain(E, data, layers, heads):
    drv = _driver(E, data, layers, heads)
    out = drv.infer_full_gat()
    assert tuple(out.shape) == (data["V"], 7)
    W = drv.weights()
    _held(f"infer_full_gat {layers} heads {heads}", out.cpu(), _chain(data, W, heads, torch.float64),
          _chain(data, W, heads, torch.float32))
    assert torch.equal(out, drv.infer_full_gat())  # no random stream, no order left open


def test_infer_full_gat_agrees_with_the_sampled_path_at_unlimited_fanout(E, data):
    layers, heads = [64, 64, 7], [8, 8]
    a = _driver(E, data, layers, heads)
    b = _driver(E, data, layers, heads, fanout=(-1, -1), batch=64)
    b.set_weights(a.weights())
    seeds = torch.arange(5, 5 + 64 * 90, 90, dtype=torch.int32)
    assert seeds.numel() == 64
    full = a.infer_full_gat().cpu()[seeds.long()]
    sampled = b.forward_eval(seeds, 0)[-1].log_softmax(1).cpu()
    W = a.weights()
    r64 = _chain(data, W, heads, torch.float64)[seeds.long()]
    r32 = _chain(data, W, heads, torch.float32)[seeds.long()]
    print(f"sampled fanout -1 vs infer_full_gat: max |diff| "
          f"{float((sampled - full).abs().max()):.3e} over {seeds.numel()} seeds")
    _held("full side", full, r64, r32)
    _held("sampled side", sampled, r64, r32)


def test_evaluate_full_gat_is_the_argmax_count_of_infer_full_gat(E, data):
    drv = _driver(E, data, [64, 64, 7], [8, 1])
    for _ in range(3):  # some training, so the rows are not all alike
        drv.train_batch()
    ids = torch.nonzero(data["masks"].cpu() == 2).flatten().to(torch.int32)
    assert ids.numel() > 100
    pred = drv.infer_full_gat().cpu().argmax(1)
    correct = int((pred[ids.long()] == data["labels"].cpu()[ids.long()]).sum())
    got = drv.evaluate_full_gat(ids)
    print(f"evaluate_full_gat {got!r} vs host count {correct} / {ids.numel()}")
    assert got == correct / ids.numel()
    assert drv.evaluate_full_gat(torch.empty(0, dtype=torch.int32)) == 0.0
    with pytest.raises(RuntimeError, match="vertex id"):
        drv.evaluate_full_gat(torch.tensor([data["V"]], dtype=torch.int32))


@pytest.mark.parametrize("pipeline", [True, False])
def test_evaluate_full_gat_does_not_disturb_training(E, data, pipeline):
    """3 batches, evaluate_full_gat, 3 more: losses and weights bit-identical to
    a driver that never called it (the sampler's stream, the prefetched batch
    and the deferred update are all left as they were)."""
    a = _driver(E, data, [64, 64, 7], [8, 8], pipeline=pipeline)
    b = _driver(E, data, [64, 64, 7], [8, 8], pipeline=pipeline)
    ids = torch.nonzero(data["masks"].cpu() == 1).flatten().to(torch.int32)
    la, lb = [], []
    for step in range(6):
        if step == 3:
            a.evaluate_full_gat(ids)
        a.train_batch()
        a.synchronize()
        la.append(float(a.loss.detach()))
        b.train_batch()
        b.synchronize()
        lb.append(float(b.loss.detach()))
    print(f"losses with evaluate_full_gat {la}\nlosses without           {lb}")
    assert la == lb
    for x, y in zip(a.weights(), b.weights()):
        assert torch.equal(x, y)


def test_refusals(E, data):
    from nts import host
    cfg = host.gcn_config([64, 32, 7], [10, 5], 200, drop_rate=0.0, shuffle=False)
    gcn = E.GCN_SAMPLE_ALLGPU_impl(data["G"], data["feat"], data["labels"], data["train"], cfg)
    with pytest.raises(RuntimeError, match=r"infer_full_gat.*infer_full\(\)"):
        gcn.infer_full_gat()
    with pytest.raises(RuntimeError, match="infer_full_gat"):
        gcn.evaluate_full_gat(torch.arange(10, dtype=torch.int32))
    spilled = _driver(E, data, [64, 32, 7], None, cache_rate=0.5)
    with pytest.raises(RuntimeError, match="infer_full_gat: needs the whole feature table"):
        spilled.infer_full_gat()
    # infer_full() still refuses a GAT driver, and now names the call that does it
    gat = _driver(E, data, [64, 32, 7], None)
    with pytest.raises(RuntimeError, match="infer_full: GAT.*infer_full_gat"):
        gat.infer_full()


def test_runner_scores_a_gat_job_over_the_whole_graph(tmp_path):
    """FULL_INFERENCE:1 with GATSAMPLEALLGPU and GAT_HEADS:8-1: the two Full ...
    Acc lines and result keys after the last epoch, the rest of the job as it
    was without the key."""
    from conftest import GOLDEN
    from nts import run
    for f in ("cora.2708.edge.self", "cora.featuretable.zip", "cora.labeltable", "cora.mask"):
        shutil.copy(GOLDEN / "cora" / f, tmp_path / f)
    text = (GOLDEN / "cora" / "gcn_cora_sample.cfg").read_text()
    assert "ALGORITHM:GCNSAMPLEALLGPU" in text
    text = text.replace("ALGORITHM:GCNSAMPLEALLGPU", "ALGORITHM:GATSAMPLEALLGPU") + "GAT_HEADS:8-1\n"
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
