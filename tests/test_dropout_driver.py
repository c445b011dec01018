"""Training steps of the non-GAT drivers with dropout on, against the float64
chain of tests/dropout_chain.py with the keep masks rebuilt from cfg.seed and
the order of the draws (GCN_SAMPLE_ALLGPU_impl's plain, LayerNorm, BatchNorm,
root-weight, max, mean and multi-label forms, and the LinkPredictor).

Gradient cases.  One readout step (tests/step_check.py), shuffle off, random
weights: every parameter's gradient is held to C err(float32 chain) + FLOOR +
resolution against the float64 chain, both over drv.last_layers.  Each case
also shows, without a mutated build, that the bound can tell the faults apart:
  * the float64 gradients of every W differ from the same chain at p = 0 by
    more than 100 times the case's bound;
  * the driver's gradients of every W are outside the bound against the
    float64 chain with its offsets shifted by one, and against the one with
    scale = 1;
  * every mask keeps and drops an element, and keeps one in every column.
The two graphs are tests/test_host.py's (V = 6000; [64, H, 7], fanout [10, 5],
batch 200: the transform-first and pair-table forms) and
tests/test_layer_norm_driver.py's (V = 2000; [32, 16, 8] / [32, 16, 16, 8],
fanout 5, batch 64).  H = 32 has no act_bits layout (the fused backward reads
the output rows), H = 128 has one; both are asserted.

Offsets across steps.  Two batches, pipeline on and off: the second batch's
loss is held to the yardstick rule against the chain over the second batch's
layers with the driver's weights (and BatchNorm buffers) after step 1 and
offsets from L - 1, and is outside it against the chain with offsets from 0.
The second step's gradients are not read out: Adam's moments are no longer
zero after the first step, so the weight change no longer inverts to the
gradient.
"""
import numpy as np
import pytest
import torch

import dropout_chain as dc
import step_check as sc
import test_batch_norm_driver as tbd
import test_layer_norm_driver as tld
import test_link_pred_driver as tlp
import test_max_driver as tmd

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
L2, F2, L3, F3 = tld.L2, tld.F2, tld.L3, tld.F3
BIG_FANOUT, BIG_BATCH = [10, 5], 200


@pytest.fixture(scope="module")
def E():
    from nts import host
    return host.ext()


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=2000)


@pytest.fixture(scope="module")
def small(E):
    return tmd.make_data(E, tmd.DATA_SEED)


@pytest.fixture(scope="module")
def big(E):
    """tests/test_host.py's graph with its 64 features and 7 classes"""
    from nts import synthetic
    g = synthetic.chung_lu(6000, 180000, 20.0, device=DEV, seed=3)
    G = E.FullyRepGraph.from_edges(g.src, g.dst, g.n_vertices)
    feat = synthetic.features(g.n_vertices, 64, device=DEV)
    labels, masks = synthetic.labels_masks(g.n_vertices, 7, device=DEV)
    train = torch.nonzero(masks == 0).flatten().to(torch.int32).cpu()
    return dict(G=G, feat=feat, labels=labels, train=train)


def _big(layers, **kw):
    return dict(graph="big", layers=layers, fanout=BIG_FANOUT, kw=kw)


def _small(layers=L2, fanout=F2, **kw):
    return dict(graph="small", layers=layers, fanout=fanout, kw=kw)


ATOMIC = dict(deterministic_backward=False)  # test_atomic_backward_trains_like_the_csr_backward's
CASES = {
    "agg-first": _big([64, 32, 7], transform_first=0, pair_table=0),
    "agg-first-pairs-1": _big([64, 32, 7], transform_first=0, pair_table=1),
    "agg-first-pairs-3": _big([64, 128, 7], transform_first=0, pair_table=3),
    "tf-rows": _big([64, 32, 7], transform_first=1),
    "tf-bits": _big([64, 128, 7], transform_first=1),
    "tf-atomic": _big([64, 32, 7], transform_first=1, **ATOMIC),
    "three-layer-tf0": _small(L3, F3, transform_first=0),
    "three-layer-tf1": _small(L3, F3, transform_first=1),
    "agg-first-p0.1": _big([64, 32, 7], transform_first=0, pair_table=0, drop_rate=0.1),
    "agg-first-p0.9": _big([64, 32, 7], transform_first=0, pair_table=0, drop_rate=0.9),
    "tf-bits-p0.1": _big([64, 128, 7], transform_first=1, drop_rate=0.1),
    "tf-bits-p0.9": _big([64, 128, 7], transform_first=1, drop_rate=0.9),
    "agg-first-seed7": _big([64, 32, 7], transform_first=0, pair_table=0, seed=7),
    "tf-rows-seed7": _big([64, 32, 7], transform_first=1, seed=7),
    "layer_norm": _small(*tld.CASES["sum"][:2], layer_norm=True),
    "layer_norm-3-layers": _small(*tld.CASES["sum-3-layers"][:2], layer_norm=True),
    "batch_norm": _small(*tld.CASES["sum"][:2], batch_norm=True),
    "batch_norm-3-layers": _small(*tld.CASES["sum-3-layers"][:2], batch_norm=True),
    "root_weight": _small(root_weight=True),
    "max": _small(aggregator="max"),
    "mean-up_degree": _small(weight="mean", up_degree=True),
    "multi_label": _small(multi_label=True),
}


def _norm(kw):
    return "layer" if kw.get("layer_norm") else "batch" if kw.get("batch_norm") else None


def _cfg(c, readout=True, **more):
    from nts import host
    kw = dict(drop_rate=0.5, seed=2000)
    kw.update(c["kw"])
    kw.update(more)
    if c["graph"] == "big":
        cfg = host.gcn_config(c["layers"], c["fanout"], BIG_BATCH, learn_rate=0.01, shuffle=False, **kw)
    else:
        cfg = tld._cfg(c["layers"], c["fanout"], **kw)
    return sc.readout(cfg) if readout else cfg


def _weights(drv, seed, norm):
    """random weights: gamma / beta as tests/test_layer_norm_driver.py's; without
    a norm the driver's own initial W (seed 0), or normal ones of their spread"""
    if norm:
        return tld._nontrivial(drv, seed)
    ws = [w.cpu().clone() for w in drv.weights()]
    if seed:
        g = torch.Generator().manual_seed(seed)
        ws = [torch.randn(w.shape, generator=g) * w.std() for w in ws]
    return ws


def _names(L, norm):
    return [f"W[{l}]" for l in range(L)] + ([f"{n}[{l}]" for l in range(L - 1) for n in ("gamma", "beta")]
                                            if norm else [])


def _bounds(W0, g64, g32):
    """check_step_grads' bound of every parameter"""
    return [sc.yardstick_bound(sc.err(b, a), sc.C, sc.resolution(w) / float(a.abs().max()))
            for w, a, b in zip(W0, g64, g32)]


def _report(tag, ratios, W0, W1, g64, g32):
    """the figures of DESIGN.md's table: the largest net ratio, and the largest
    share of its bound that a parameter's error takes (readout resolution included)"""
    share = max(sc.err(sc.recovered_grads(a, b).reshape(r.shape), r) / bd
                for a, b, r, bd in zip(W0, W1, g64, _bounds(W0, g64, g32)))
    print(f"  {tag}: largest net ratio {max(ratios):.2f}, largest err(driver) / bound {share:.2f}")


def _teeth(tag, L, W0, W1, g64, g32, masks, hidden, alt):
    """the checks that need no mutated build; alt(p=, first_offset=, s=) gives
    the float64 gradients of a changed chain"""
    bounds = _bounds(W0, g64, g32)
    got = [sc.recovered_grads(a, b).reshape(r.shape) for a, b, r in zip(W0, W1, g64)]
    bad = []
    plain = alt(p=0.0)
    for l in range(L):
        d = sc.err(plain[l], g64[l])
        print(f"  {tag} W[{l}]: float64 p = 0 vs dropped {d:.3e} = {d / bounds[l]:.0f} bounds")
        if not d > 100 * bounds[l]:
            bad.append(f"W[{l}]: the dropped and undropped references are {d / bounds[l]:.1f} bounds apart")
    for what, ref in (("offsets + 1", alt(first_offset=1)), ("scale 1", alt(s=1.0))):
        for l in range(L):
            e = sc.err(got[l], ref[l])
            print(f"  {tag} W[{l}] against {what}: err(driver) {e:.3e} = {e / bounds[l]:.0f} bounds")
            if not e > bounds[l]:
                bad.append(f"W[{l}]: inside the bound against the chain with {what}")
    for l, (m, h) in enumerate(zip(masks, hidden)):
        assert tuple(m.shape) == tuple(h.shape)
        if not (bool(m.any()) and not bool(m.all()) and bool(m.any(0).all())):
            bad.append(f"mask {l}: kept {int(m.sum())} of {m.numel()}, "
                       f"{int((~m.any(0)).sum())} columns all dropped")
    assert not bad, "; ".join(bad)


def _hold_loss(tag, got, loss64, loss32):
    e, e32 = abs(got - loss64) / abs(loss64), abs(loss32 - loss64) / abs(loss64)
    print(f"  {tag}: loss {got!r} float64 {loss64!r} float32 chain {loss32!r} err {e:.3e} (chain {e32:.3e})")
    assert e <= sc.yardstick_bound(e32, sc.C)


@pytest.mark.parametrize("case", list(CASES))
def test_dropped_step_gradients_match_the_float64_chain(E, hip, big, small, case):
    from nts import synthetic
    c = CASES[case]
    kw, layers = c["kw"], c["layers"]
    data = big if c["graph"] == "big" else small
    L, norm = len(layers) - 1, _norm(kw)
    p, seed = kw.get("drop_rate", 0.5), kw.get("seed", 2000)
    root, mx = bool(kw.get("root_weight")), kw.get("aggregator") == "max"
    labels = (synthetic.multilabels(tmd.V, layers[-1], data["feat"], seed=13)
              if kw.get("multi_label") else None)
    if case.startswith("tf-bits"):
        assert hip.act_bits_words(layers[1]) > 0
    if case.startswith(("tf-rows", "tf-atomic")):
        assert hip.act_bits_words(layers[1]) == 0

    def build():
        return tld._driver(E, data, _cfg(c), labels)

    def run(ws, dtype, p=p, first_offset=0, s=None, stats=None):
        st = None if stats is None else [x.cpu().to(dtype).clone() for x in stats]
        P, loss, hidden, masks = dc.chain(lays, data, ws, dtype, p, seed, first_offset, norm=norm,
                                          stats=st, root=root, mx=mx, labels=labels, s=s)
        loss.backward()
        return [q.grad for q in P], float(loss.detach()), hidden, masks, st

    wseed = 1 if norm or mx else 0
    if mx:  # the batch is the same for every weight: sample it once, pick the seed on float64 alone
        probe = build()
        probe.train_batch()
        probe.synchronize()
        lays = probe.last_layers
        for wseed in range(wseed, 9):
            gap = dc.top_gap(lays, run(_weights(probe, wseed, norm), torch.float64)[2])
            if gap > tmd.GAP:
                break
    drv = build()
    if "transform_first" in kw:
        assert drv.transform_first == bool(kw["transform_first"])
    W0 = _weights(drv, wseed, norm)
    assert len(W0) == (L + 2 * (L - 1) if norm else L)
    S0 = drv.norm_stats() if norm == "batch" else None
    drv.set_weights([w.to(DEV) for w in W0])
    drv.train_batch()
    drv.synchronize()
    W1 = [w.cpu().clone() for w in drv.weights()]
    if mx:
        assert tld._same_layers(drv.last_layers, lays)
    lays = drv.last_layers
    g64, loss64, hidden, masks, st64 = run(W0, torch.float64, stats=S0)
    g32, loss32, _, _, st32 = run(W0, torch.float32, stats=S0)
    if mx:
        gap = dc.top_gap(lays, hidden)
        print(f"max: top-hop gap {gap:.3e} (weight seed {wseed})")
        assert gap > tmd.GAP, "the reference's winners are too close"
    print(f"dropout {case}: {layers} p {p} seed {seed}")
    _hold_loss(case, float(drv.loss.detach()), loss64, loss32)
    ratios = sc.check_step_grads(W0, W1, g64, g32, sc.C, _names(L, norm))
    _report(case, ratios, W0, W1, g64, g32)
    if norm == "batch":
        bad = []
        for i, s1 in enumerate(drv.norm_stats()):
            tbd._hold(f"{('running_mean', 'running_var')[i % 2]}[{i // 2}]", s1.cpu(), st64[i], st32[i], bad)
        assert not bad, "; ".join(bad)
    _teeth(case, L, W0, W1, g64, g32, masks, hidden,
           lambda **ch: run(W0, torch.float64, stats=S0, **ch)[0])


def test_link_predictor_dropped_step_gradients_match_the_float64_chain():
    from nts import host
    E = host.ext()
    from nts import synthetic
    p, seed, L = 0.5, 2000, 2
    g = synthetic.chung_lu(200, 2400, 6.0, device=DEV, seed=4)  # tests/test_link_pred_driver.py's
    G = E.FullyRepGraph.from_edges(g.src, g.dst, g.n_vertices)
    feat = synthetic.features(200, tlp.LAYERS[0], device=DEV)
    edges = torch.stack([g.src.cpu().to(torch.int64), g.dst.cpu().to(torch.int64)])[:, :320].contiguous()
    cfg = sc.readout(host.gcn_config(tlp.LAYERS, tlp.FANOUT, tlp.B, drop_rate=p, seed=seed, pipeline=False,
                                     neg_per_pos=tlp.K))
    drv = host.link_predictor(G, feat, edges, cfg)
    W0 = drv.weights()
    got = drv.train_batch()
    W1 = drv.weights()
    lb = drv.last_batch()

    def run(dtype, p=p, first_offset=0, s=None):
        P, loss, hidden, masks = dc.lp_chain(lb, feat, W0, dtype, p, seed, first_offset, s)
        loss.backward()
        return [q.grad for q in P], float(loss.detach()), hidden, masks

    g64, loss64, hidden, masks = run(torch.float64)
    g32, loss32, _, _ = run(torch.float32)
    print(f"dropout link predictor: {tlp.LAYERS} p {p}")
    _hold_loss("link-pred", got, loss64, loss32)
    ratios = sc.check_step_grads(W0, W1, g64, g32, sc.C)
    _report("link-pred", ratios, W0, W1, g64, g32)
    _teeth("link-pred", L, W0, W1, g64, g32, masks, hidden, lambda **ch: run(torch.float64, **ch)[0])


STEP_CASES = {"agg-first": "agg-first", "tf-rows": "tf-rows", "three-layer-tf1": "three-layer-tf1",
              "layer_norm": "layer_norm-3-layers", "batch_norm": "batch_norm-3-layers"}


@pytest.mark.parametrize("pipeline", [True, False], ids=["pipeline", "no-pipeline"])
@pytest.mark.parametrize("case", list(STEP_CASES))
def test_second_step_takes_the_next_offsets(E, big, small, case, pipeline):
    """The second batch's loss against the chain at offsets L - 1 ... and, out of
    bounds, at 0 ...  (No gradient readout here: after the first step Adam's
    moments are not zero, so the weight change does not invert to the gradient.)"""
    c = CASES[STEP_CASES[case]]
    kw, layers = c["kw"], c["layers"]
    data = big if c["graph"] == "big" else small
    L, norm = len(layers) - 1, _norm(kw)
    p, seed = kw.get("drop_rate", 0.5), kw.get("seed", 2000)
    drv = tld._driver(E, data, _cfg(c, readout=False, pipeline=pipeline))
    drv.set_weights([w.to(DEV) for w in _weights(drv, 1 if norm else 0, norm)])
    drv.train_batch()
    drv.synchronize()
    first = drv.last_layers
    W = [w.cpu().clone() for w in drv.weights()]
    S = [s.cpu().clone() for s in drv.norm_stats()] if norm == "batch" else None
    drv.train_batch()
    drv.synchronize()
    lays = drv.last_layers
    assert not tld._same_layers(lays, first)  # it is the second batch
    got = float(drv.loss.detach())

    def loss(dtype, first_offset):
        st = None if S is None else [x.to(dtype).clone() for x in S]
        return float(dc.chain(lays, data, W, dtype, p, seed, first_offset, norm=norm, stats=st)[1].detach())

    start = dc.offsets(1, L)[0]
    assert start == L - 1
    loss64, loss32, wrong = loss(torch.float64, start), loss(torch.float32, start), loss(torch.float64, 0)
    bound = sc.yardstick_bound(abs(loss32 - loss64) / abs(loss64), sc.C)
    print(f"second step {case} pipeline={pipeline}: loss {got!r}, float64 at offset {start} {loss64!r} "
          f"(err {abs(got - loss64) / abs(loss64):.3e}, bound {bound:.3e}), at offset 0 {wrong!r} "
          f"(err {abs(got - wrong) / abs(wrong):.3e})")
    assert abs(got - loss64) <= bound * abs(loss64)
    assert abs(got - wrong) > bound * abs(wrong)
    assert abs(loss64 - wrong) > 100 * bound * abs(loss64)  # the reference alone tells the schedules apart
