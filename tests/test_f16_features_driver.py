"""GCNConfig::feature_f16 through the driver.

f16 storage, fp32 arithmetic: a driver with the option computes what a driver
without it computes on table.half().float() with an aggregate-first bottom
layer — the yardstick of every comparison here, torch.equal on the weights, the
loss and the scores.  Only the full-neighbour pass of a narrowing first layer
has no such twin (the fp32 driver transforms first there); it is held against
a float64 restatement of the chain with the forward bar of
tests/test_full_infer_driver.py, rtol = atol = 1e-4.
"""
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
V = 300
LAYERS, FANOUT, BATCH = [32, 16, 4], [3, 2], 8


@pytest.fixture(scope="module")
def E():
    from nts import host
    return host.ext()


@pytest.fixture(scope="module")
def data(E):
    from nts import synthetic
    g = synthetic.chung_lu(V, 1200, 6.0, device=DEV, seed=3)
    deg = torch.bincount(g.dst.long(), minlength=V)
    # in-degrees on both sides of both fanouts
    assert int((deg < 2).sum()) > 0 and int((deg == 3).sum()) > 0 and int((deg > 3).sum()) > 20
    G = E.FullyRepGraph.from_edges(g.src, g.dst, V)
    labels, masks = synthetic.labels_masks(V, 4, device=DEV)
    train = torch.nonzero(masks == 0).flatten().to(torch.int32).cpu()
    feats = {F: synthetic.features(V, F, device=DEV, seed=9) for F in (16, 32, 64, 602)}
    return dict(G=G, g=g, labels=labels, masks=masks, train=train, feats=feats)


def _driver(E, data, layers=LAYERS, f16=False, table=None, labels=None, **kw):
    from nts import host
    kw.setdefault("drop_rate", 0.0)
    if not f16:
        kw.setdefault("transform_first", 0)
    cfg = host.gcn_config(layers, FANOUT[:len(layers) - 1], BATCH, learn_rate=0.01, shuffle=False,
                          feature_f16=f16, **kw)
    if table is None:
        table = data["feats"][layers[0]]
        if not f16:
            table = table.half().float()  # the yardstick's table: the widened halves
    return E.GCN_SAMPLE_ALLGPU_impl(data["G"], table, data["labels"] if labels is None else labels,
                                    data["train"], cfg)


def _steps(drv, n=3):
    for _ in range(n):
        drv.train_batch()
    drv.synchronize()
    return [w.clone() for w in drv.weights()], drv.loss.detach().clone()


def _same(a, b):
    (wa, la), (wb, lb) = a, b
    assert len(wa) == len(wb)
    for x, y in zip(wa, wb):
        assert torch.equal(x, y)
    assert torch.equal(la, lb) and bool(torch.isfinite(la))


def _mt():
    from nts import _abi
    return _abi.NTS_RNG_MT19937_LEMIRE


CASES = {
    "gcn-sum": dict(),
    "sage-mean-up_degree": dict(weight="mean", up_degree=True),
    "mean-sampled": dict(weight="mean-sampled"),
    "layer_norm": dict(layer_norm=True),
    "shared_sampling": dict(shared_sampling=True),
    "sample_gpu": dict(sample_gpu=True, rng_mode=_mt),
    "no-pipeline": dict(pipeline=False),
    "late-aggregate": dict(early_aggregate=False),
    "row-gather": dict(fused_gather=False),
    "dropout": dict(drop_rate=0.5),
}


@pytest.mark.parametrize("case", list(CASES))
def test_three_steps_equal_the_fp32_driver_on_the_widened_table(E, data, case):
    kw = {k: (v() if callable(v) else v) for k, v in CASES[case].items()}
    on = _driver(E, data, f16=True, **kw)
    off = _driver(E, data, **kw)
    assert not on.transform_first and not off.transform_first
    a, b = _steps(on), _steps(off)
    _same(a, b)
    assert not torch.equal(a[0][0], _driver(E, data, f16=True, **kw).weights()[0])  # it trained


def test_multi_label(E, data):
    from nts import synthetic
    labels = synthetic.multilabels(V, 4, data["feats"][32])
    _same(_steps(_driver(E, data, f16=True, labels=labels, multi_label=True)),
          _steps(_driver(E, data, labels=labels, multi_label=True)))


def test_a_wide_bottom_layer_aggregates_first(E, data):
    layers = [602, 16, 4]
    on = _driver(E, data, layers, f16=True)
    auto = _driver(E, data, layers, transform_first=-1)
    assert auto.transform_first  # what the fp32 driver would have chosen
    assert not on.transform_first
    _same(_steps(on), _steps(_driver(E, data, layers)))


def test_evaluate_is_equal(E, data):
    on, off = _driver(E, data, f16=True), _driver(E, data)
    _steps(on), _steps(off)
    ids = torch.nonzero(data["masks"].cpu() == 1).flatten().to(torch.int32)
    assert ids.numel() > 10
    assert on.evaluate(ids) == off.evaluate(ids)


def test_a_half_tensor_is_taken_as_given(E, data):
    feat = data["feats"][32]
    a = _driver(E, data, f16=True)
    b = _driver(E, data, f16=True, table=feat.half())
    assert b.F.dtype == torch.float16 and b.F.data_ptr() != 0
    ref = _steps(a)
    _same(ref, _steps(b))
    # rows that do not allow 16-byte loads are re-laid, values unchanged
    odd = torch.empty(V, 37, dtype=torch.float16, device=DEV)[:, 1:33]
    odd.copy_(feat)
    c = _driver(E, data, f16=True, table=odd)
    assert c.F.stride(0) % 8 == 0 and c.F.data_ptr() % 16 == 0
    _same(ref, _steps(c))


@pytest.mark.parametrize("F", [32, 602])
def test_the_table_is_kept_as_half_at_half_the_bytes(E, data, F):
    on = _driver(E, data, [F, 16, 4], f16=True)
    off = _driver(E, data, [F, 16, 4])
    assert on.F.dtype == torch.float16 and off.F.dtype == torch.float32
    assert tuple(on.F.shape) == (V, F) and on.F.stride(0) % 8 == 0 and on.F.data_ptr() % 16 == 0
    assert torch.equal(on.F, data["feats"][F].half())  # round to nearest even
    # half the fp32 driver's bytes a row, up to the padding of the last 128-byte line
    half_row, row = on.F.stride(0) * 2, off.F.stride(0) * 4
    assert row // 2 <= half_row < row // 2 + 128


def test_infer_full_equals_the_fp32_driver_where_it_aggregates_first(E, data):
    layers = [16, 32, 4]
    on, off = _driver(E, data, layers, f16=True), _driver(E, data, layers)
    _same(_steps(on), _steps(off))
    assert torch.equal(on.infer_full(), off.infer_full())
    ids = torch.nonzero(data["masks"].cpu() == 2).flatten().to(torch.int32)
    assert on.evaluate_full(ids) == off.evaluate_full(ids)
    assert on.F.dtype == torch.float16  # nothing replaced the half table


def test_infer_full_of_a_narrowing_layer_matches_the_float64_chain(E, data):
    layers = [64, 16, 4]
    on = _driver(E, data, layers, f16=True)
    _steps(on, 2)
    ws = [w.cpu().double() for w in on.weights()]
    g = data["g"]
    src, dst = g.src.cpu().long(), g.dst.cpu().long()
    od = torch.bincount(src, minlength=V).double()
    idg = torch.bincount(dst, minlength=V).double()
    A = torch.sparse_coo_tensor(torch.stack([dst, src]), 1.0 / (od[src].sqrt() * idg[dst].sqrt()),
                                (V, V)).coalesce()
    X = data["feats"][64].half().cpu().double()  # the widened table
    for l, w in enumerate(ws):
        Z = torch.sparse.mm(A, X) @ w
        X = Z if l == len(ws) - 1 else torch.relu(Z)
    ref = X.log_softmax(1)
    out = on.infer_full()
    print(f"infer_full {layers} f16: max |diff| {float((out.cpu().double() - ref).abs().max()):.3e}")
    torch.testing.assert_close(out.cpu().double(), ref, rtol=1e-4, atol=1e-4)
    assert torch.equal(out, on.infer_full())


REFUSALS = {
    "gat": (dict(gat=True, weight="none"),
            "feature_f16 is not supported with gat (GCN / GraphSAGE layers only)"),
    "pd_cache": (dict(pd_cache=True), "feature_f16 is not supported with pd_cache"),
    "transform_first": (dict(transform_first=1),
                        "feature_f16 is not supported with transform_first = 1 (the "
                        "transform-first GEMMs gather fp32 rows: aggregate-first only)"),
    "pair_table": (dict(pair_table=1), "feature_f16 is not supported with pair_table > 0"),
    "cache_rate": (dict(cache_rate=0.5), "feature_f16 is not supported with cache_rate >= 0"),
    "root_weight": (dict(root_weight=True), "feature_f16 is not supported with root_weight"),
    "max": (dict(aggregator="max"), "feature_f16 is not supported with aggregator = max"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refused_combinations(E, data, name):
    kw, text = REFUSALS[name]
    with pytest.raises(RuntimeError, match="feature_f16") as ei:
        _driver(E, data, f16=True, **kw)
    assert str(ei.value).splitlines()[0] == text


def test_earlier_refusals_come_first(E, data):
    with pytest.raises(RuntimeError) as ei:
        _driver(E, data, f16=True, root_weight=True, pd_cache=True)
    assert str(ei.value).splitlines()[0] == "root_weight is not supported with pd_cache"


def test_a_value_outside_the_half_range_is_refused(E, data):
    t = data["feats"][32].clone()
    t[17, 5] = 1e6
    t[40, 0] = -1e6
    with pytest.raises(RuntimeError, match="feature_f16") as ei:
        _driver(E, data, f16=True, table=t)
    line = str(ei.value).splitlines()[0]
    assert line.startswith("feature_f16: 2 feature value(s) are not finite as IEEE half")
    assert "the first is in row 17" in line


def test_a_half_table_without_the_option_is_refused(E, data):
    with pytest.raises(RuntimeError, match="feature_f16") as ei:
        _driver(E, data, table=data["feats"][32].half())
    assert str(ei.value).splitlines()[0] == (
        "a float16 feature table needs feature_f16 (FEATURE_F16:1): without it the driver takes "
        "an fp32 table")


def test_cfg_job_with_full_inference(tmp_path):
    from conftest import GOLDEN
    from nts import run
    for f in ("cora.2708.edge.self", "cora.featuretable.zip", "cora.labeltable", "cora.mask"):
        shutil.copy(GOLDEN / "cora" / f, tmp_path / f)
    text = (GOLDEN / "cora" / "gcn_cora_sample.cfg").read_text()
    (tmp_path / "f16.cfg").write_text(text + "FEATURE_F16:1\nFULL_INFERENCE:1\n")
    lines = []
    res = run.run(tmp_path / "f16.cfg", epochs=1, out=lines.append)
    print("\n".join(lines[-4:]))
    full = [l for l in lines if l.startswith("Full Test Acc:")]
    assert len(full) == 1 and 0.0 < res["full_test_acc"] <= 1.0
    assert np.isfinite(res["epochs"][0]["loss"])
