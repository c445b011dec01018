"""The multi-label mode of GCN_SAMPLE_ALLGPU_impl (GCNConfig::multi_label) and
of the runner (MULTI_LABEL:1): fused BCE top layer against the libtorch
fallback, training, micro-F1 of the sampled and the full-graph evaluation, and
the mode's errors.

Bars: one training step within 1e-5 (loss and updated weights, the one-step
bar of tests/test_host.py); forward logits rtol = atol = 1e-4, the project's
forward bar.  Where a micro-F1 is recomputed on the host from fp32 logits of
another pass, logits near zero may fall on either side there: within 1e-4
(the forward bar) for evaluate_full against the CPU chain, within 1e-5 (ten
times the fp32 rounding of a K = 64 dot product of O(1) terms) where the fused
loss kernel's own logits stand against the layer GEMM's.  The driver's counts
must then lie between the two extreme resolutions, and equal the host's
exactly when no logit is that close to zero.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LAYERS, FANOUT, BATCH = [48, 64, 100], [10, 5], 256
V = 2000


@pytest.fixture(scope="module")
def E():
    from nts import host
    return host.ext()


@pytest.fixture(scope="module")
def data(E):
    from nts import synthetic
    g = synthetic.chung_lu(V, 40000, 10.0, device=DEV, seed=5)
    G = E.FullyRepGraph.from_edges(g.src, g.dst, g.n_vertices)
    feat = synthetic.features(V, LAYERS[0], device=DEV)
    labels = synthetic.multilabels(V, LAYERS[-1], feat, seed=13)
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (V, LAYERS[-1])
    assert 0.3 < float(labels.float().mean()) < 0.7
    src = g.src.cpu().numpy().view(np.uint32)
    dst = g.dst.cpu().numpy().view(np.uint32)
    col, rows = orc.build_csc(V, src, dst)
    od, idg = orc.degrees(V, src, dst)
    whole = dict(column_offset=col.astype(np.uint32), row_indices=rows,
                 source=np.arange(V, dtype=np.uint32), destination=np.arange(V, dtype=np.uint32),
                 v_size=V, src_size=V, e_size=int(src.size))
    train = torch.arange(0, 1300, dtype=torch.int32)
    return dict(G=G, feat=feat, labels=labels, train=train, od=od, idg=idg, whole=whole)


def _driver(E, data, labels=None, layers=LAYERS, **kw):
    from nts import host
    kw.setdefault("multi_label", True)
    cfg = host.gcn_config(layers, FANOUT, BATCH, learn_rate=0.01, drop_rate=0.0, shuffle=False, **kw)
    return E.GCN_SAMPLE_ALLGPU_impl(data["G"], data["feat"][:, :layers[0]].contiguous(),
                                    data["labels"] if labels is None else labels, data["train"], cfg)


def _f1(tp, fp, fn):
    return 2.0 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0


def _counts(logits, t):
    pos = logits > 0
    return int((pos & t).sum()), int((pos & ~t).sum()), int((~pos & t).sum())


def _band(logits, t, eps):
    """(lowest, highest) tp / fp / fn with every |logit| < eps resolved either way"""
    near = logits.abs() < eps
    up, down = _counts(torch.where(near, 1.0, logits.double()), t), \
        _counts(torch.where(near, -1.0, logits.double()), t)
    return (down[0], down[1], up[2]), (up[0], up[1], down[2])


def _f1_band(lo, hi):
    """micro-F1 rises with tp and falls with fp and fn"""
    return _f1(lo[0], hi[1], hi[2]), _f1(hi[0], lo[1], lo[2])


def test_one_training_step_fused_equals_the_libtorch_fallback(E, data):
    assert E.hip_linear_bce_supported(LAYERS[-2], LAYERS[-1])
    a = _driver(E, data, fuse_loss=True)
    b = _driver(E, data, fuse_loss=False)
    for x, y in zip(a.weights(), b.weights()):
        assert torch.equal(x, y)
    a.train_batch()
    b.train_batch()
    a.synchronize()
    b.synchronize()
    print(f"one step: fused loss {float(a.loss.detach()):.7f}, libtorch chain {float(b.loss.detach()):.7f}")
    torch.testing.assert_close(a.loss.detach().cpu(), b.loss.detach().cpu(), rtol=1e-5, atol=1e-5)
    for x, y in zip(a.weights(), b.weights()):
        torch.testing.assert_close(x, y, rtol=1e-5, atol=1e-5)
    ca, cb = a.f1_counts(), b.f1_counts()
    print(f"tp/fp/fn fused {ca}, libtorch chain {cb}")
    assert sum(ca) > 0 and ca[0] + ca[2] == cb[0] + cb[2]  # tp + fn: the batch's positives
    assert max(abs(x - y) for x, y in zip(ca, cb)) <= 2  # logits within rounding of zero


def test_training_lowers_the_loss(E, data):
    drv = _driver(E, data)
    losses = []
    for _ in range(40):
        if not drv.sample_not_finished():
            drv.restart()
        drv.train_batch()
        drv.synchronize()
        losses.append(float(drv.loss.detach()))
    print(f"loss of step 1: {losses[0]:.5f}, after 40 steps: {losses[-1]:.5f}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


@pytest.mark.parametrize("fuse", [True, False])
def test_evaluate_is_the_micro_f1_of_the_sampled_batches(E, data, fuse):
    drv = _driver(E, data, fuse_loss=fuse)
    for _ in range(3):
        drv.train_batch()
    ids = torch.arange(1300, 1300 + 600, dtype=torch.int32)  # batches of 256, 256, 88
    t = data["labels"].cpu().bool()
    # evaluate() draws its batches from the eval stream, one sequence number
    # per batch starting at 2^40: forward_eval over the same seeds and numbers
    # is the same sample and the same eval-mode forward
    lo, hi = np.zeros(3, np.int64), np.zeros(3, np.int64)
    for k, s in enumerate(range(0, ids.numel(), BATCH)):
        seeds = ids[s:s + BATCH]
        logits = drv.forward_eval(seeds, (1 << 40) + k)[-1].cpu()
        assert tuple(logits.shape) == (seeds.numel(), LAYERS[-1])
        # the libtorch chain counts these very logits; the fused kernel its own
        a, b = _band(logits, t[seeds.long()], 1e-5 if fuse else 0.0)
        lo += a
        hi += b
    f_lo, f_hi = _f1_band(lo, hi)
    got = drv.evaluate(ids)
    print(f"evaluate {got!r}, host micro-F1 in [{f_lo!r}, {f_hi!r}] of tp/fp/fn {lo}..{hi}")
    assert f_lo <= got <= f_hi
    assert 0.0 < got <= 1.0
    assert drv.evaluate(torch.empty(0, dtype=torch.int32)) == 0.0


@pytest.mark.parametrize("fuse", [True, False])
def test_training_counters_are_the_sum_over_the_epochs_batches(E, data, fuse):
    """f1_counts() after an epoch against the counts of each batch's own
    logits: before training batch k, forward_eval over its seeds with its
    sequence number draws the same sample under the same weights (dropout is
    off, so the eval-mode forward is the training forward)."""
    drv = _driver(E, data, fuse_loss=fuse, pipeline=False)
    t = data["labels"].cpu().bool()
    drv.reset_correct()
    assert drv.f1_counts() == (0, 0, 0)
    lo, hi, k = np.zeros(3, np.int64), np.zeros(3, np.int64), 0
    drv.restart()
    while drv.sample_not_finished():
        seeds = data["train"][k * BATCH:(k + 1) * BATCH]
        logits = drv.forward_eval(seeds, k)[-1].cpu()  # training batch k: sequence number k
        a, b = _band(logits, t[seeds.long()], 1e-5 if fuse else 0.0)
        lo += a
        hi += b
        drv.train_batch()
        k += 1
    assert k == (data["train"].numel() + BATCH - 1) // BATCH
    got = drv.f1_counts()
    print(f"epoch of {k} batches: f1_counts {got}, sum over the batches {lo}..{hi}")
    assert all(a <= g <= b for g, a, b in zip(got, lo, hi))
    assert sum(got[i] for i in (0, 2)) == int(t[data["train"].long()].sum())  # tp + fn = positives
    drv.reset_correct()
    assert drv.f1_counts() == (0, 0, 0)


def _oracle_chain(data, W):
    """relu((A X) W) per hidden layer, raw (A X) W at the top, A over the whole graph"""
    X = data["feat"].cpu()
    for l, w in enumerate(W):
        Y = torch.from_numpy(orc.fuse_fwd(data["whole"], X.numpy(), data["od"], data["idg"],
                                          weight_mean=False, threads=8))
        Z = Y @ w
        X = Z if l == len(W) - 1 else torch.relu(Z)
    return X


def test_full_inference_returns_logits_and_their_micro_f1(E, data):
    drv = _driver(E, data)
    for _ in range(3):
        drv.train_batch()
    out = drv.infer_full()
    assert tuple(out.shape) == (V, LAYERS[-1])
    ref = _oracle_chain(data, [w.cpu() for w in drv.weights()])
    print(f"infer_full logits: max |diff| {float((out.cpu() - ref).abs().max()):.3e}, "
          f"max |ref| {float(ref.abs().max()):.3e}")
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-4, atol=1e-4)
    assert float(out.min()) < 0 < float(out.max())  # logits, not log-probabilities
    ids = torch.arange(1300, V, dtype=torch.int32)
    z, t = ref[ids.long()].double(), data["labels"].cpu().bool()[ids.long()]
    lo, hi = _f1_band(*_band(z, t, 1e-4))
    got = drv.evaluate_full(ids)
    print(f"evaluate_full {got!r}, host micro-F1 in [{lo!r}, {hi!r}] "
          f"({int((z.abs() < 1e-4).sum())} logits within 1e-4 of zero)")
    assert lo <= got <= hi
    assert got == _f1(*_counts(out.cpu()[ids.long()], t))  # exactly, of its own logits
    assert drv.evaluate_full(torch.empty(0, dtype=torch.int32)) == 0.0


def test_constructor_and_mode_errors(E, data):
    from nts import synthetic
    one_d, _ = synthetic.labels_masks(V, LAYERS[-1], device=DEV)
    with pytest.raises(RuntimeError, match="2-D label tensor"):
        _driver(E, data, labels=one_d)
    with pytest.raises(RuntimeError, match="multi_label"):
        _driver(E, data, multi_label=False)  # 2-D labels without the switch
    with pytest.raises(RuntimeError, match="GAT"):
        _driver(E, data, gat=True, weight="none")
    with pytest.raises(RuntimeError, match="layer_size.back"):
        _driver(E, data, layers=[48, 64, 99])
    with pytest.raises(RuntimeError, match="0 or 1"):
        _driver(E, data, labels=data["labels"] * 2)
    plain = _driver(E, data, labels=one_d, multi_label=False)
    with pytest.raises(RuntimeError, match="multi_label"):
        plain.f1_counts()
    # bool and int64 label tensors are taken as well
    for dt in (torch.bool, torch.int64):
        d = _driver(E, data, labels=data["labels"].to(dt))
        d.train_batch()
        d.synchronize()
        assert np.isfinite(float(d.loss.detach()))


def test_device_packing_matches_the_convention(E, data):
    from nts import dataloader
    for C in (1, 33, 100, 128):
        lab = data["labels"][:, :1].expand(V, C).contiguous() if C == 1 else \
            torch.cat([data["labels"], data["labels"]], 1)[:, :C].contiguous()
        lab[0] = 1  # bit 31 of every full word set
        got = E.pack_label_bits(lab).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, dataloader.pack_label_bits(lab.cpu().numpy()))


def test_runner_reports_f1_only_under_multi_label(tmp_path):
    """cora with a generated 7-column label file (one-hot of the cora label,
    one more random bit per vertex) and MULTI_LABEL:1: one epoch prints the
    three F1 lines; the same job without the key prints none."""
    import shutil
    from conftest import GOLDEN
    from nts import run
    for f in ("cora.2708.edge.self", "cora.featuretable.zip", "cora.labeltable", "cora.mask"):
        shutil.copy(GOLDEN / "cora" / f, tmp_path / f)
    rng = np.random.default_rng(3)
    lines = []
    for line in (tmp_path / "cora.labeltable").read_text().splitlines():
        v, lab = line.split()[:2]
        row = np.zeros(7, np.int64)
        row[int(lab)] = 1
        row[rng.integers(0, 7)] = 1
        lines.append(f"{v} {' '.join(map(str, row))}")
    (tmp_path / "cora.multilabel").write_text("\n".join(lines) + "\n")
    text = (GOLDEN / "cora" / "gcn_cora_sample.cfg").read_text()
    assert "LABEL_FILE:" in text and "-7\n" in text  # 7 output columns
    ml = "\n".join("LABEL_FILE:cora.multilabel" if l.startswith("LABEL_FILE:") else l
                   for l in text.splitlines()) + "\nMULTI_LABEL:1\nFULL_INFERENCE:1\n"
    (tmp_path / "ml.cfg").write_text(ml)
    (tmp_path / "plain.cfg").write_text(text)
    got, plain = [], []
    r1 = run.run(tmp_path / "ml.cfg", epochs=1, out=got.append)
    r0 = run.run(tmp_path / "plain.cfg", epochs=1, out=plain.append)
    f1_lines = [l for l in got if " F1: " in l]
    print("\n".join(f1_lines))
    assert [l.split(" F1:")[0] for l in f1_lines] == ["Train", "Eval", "Test", "Full Eval", "Full Test"]
    for l in f1_lines:
        assert 0.0 <= float(l.split(" F1: ")[1].split()[0]) <= 1.0
    ep = r1["epochs"][0]
    for key, line in zip(("train_f1", "eval_f1", "test_f1"), f1_lines):
        assert abs(ep[key] - float(line.split(" F1: ")[1].split()[0])) < 1e-6
    assert 0.0 <= r1["full_eval_f1"] <= 1.0 and 0.0 <= r1["full_test_f1"] <= 1.0
    assert not any(" Acc: " in l for l in got) and "train_acc" not in ep
    assert not any(" F1: " in l for l in plain) and "train_f1" not in r0["epochs"][0]
    assert [l.split()[0] for l in plain if " Acc: " in l] == ["Train", "Eval", "Test"]
    gat = "\n".join("ALGORITHM:GATSAMPLEALLGPU" if l.startswith("ALGORITHM:") else l
                    for l in ml.splitlines()) + "\n"
    (tmp_path / "gat.cfg").write_text(gat)
    with pytest.raises(SystemExit, match="not supported"):
        run.run(tmp_path / "gat.cfg", epochs=1, out=[].append)
