"""Shared-variate neighbour selection through the C++ driver
(gcn_config(shared_sampling=True) -> GCNConfig::rng_mode = NTS_RNG_PHILOX_SHARED,
DESIGN §8o).

One training step is checked on the block the driver sampled (drv.last_layers)
against the float64 chains of the models' own driver tests, read out through
tests/step_check.py with their bound (C = step_check.C times the float32
chain's own error); the block itself must be the numpy restatement's
(tests/shared_blocks.py) for the batch's seeds and batch_seq.
"""
import shutil

import numpy as np
import pytest
import torch

import shared_blocks as sb
import step_check

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEED = 2000


@pytest.fixture(scope="module")
def E():
    from nts import host
    return host.ext()


@pytest.fixture(scope="module")
def small(E):
    """the max-aggregator tests' data (no repeated (src, dst) pair)"""
    import test_max_driver
    return test_max_driver.make_data(E, test_max_driver.DATA_SEED)


@pytest.fixture(scope="module")
def gat_data(E):
    from nts import synthetic
    g = synthetic.chung_lu(6000, 180000, 20.0, device=DEV, seed=3)
    G = E.FullyRepGraph.from_edges(g.src, g.dst, g.n_vertices)
    feat = synthetic.features(g.n_vertices, 64, device=DEV)
    labels, masks = synthetic.labels_masks(g.n_vertices, 7, device=DEV)
    train = torch.nonzero(masks == 0).flatten().to(torch.int32).cpu()
    return dict(G=G, g=g, feat=feat, labels=labels, masks=masks, train=train)


def _host_graph(data):
    G = data["G"]
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    return (G.column_offset.cpu().numpy().view(np.uint64), u32(G.row_indices), u32(G.in_degree),
            u32(G.out_degree))


def _assert_block_is_the_restatement(drv, data, fanout, batch, batch_seq, flags, merge):
    col, rows, idg, od = _host_graph(data)
    seeds = data["train"].numpy().view(np.uint32)[batch_seq * batch:(batch_seq + 1) * batch]
    ref = sb.shared_sample(col, rows, idg, od, seeds, fanout, SEED, batch_seq, flags, merge)
    checked = 0
    for got, want in zip(drv.last_layers, ref):
        assert (got["v_size"], got["e_size"], got["src_size"]) == (
            want["v_size"], want["e_size"], want["src_size"])
        for k, w in want.items():
            t = got.get(k) if isinstance(w, np.ndarray) else None
            if t is None or not isinstance(t, torch.Tensor):
                continue
            a = t.cpu().numpy()
            a = a.view(np.uint32) if a.dtype == np.int32 else a
            assert np.array_equal(a, w), k
            checked += 1
    assert checked >= 10
    return ref


MODELS = {
    # name: (gcn_config keywords, helper weight flags, merged destinations)
    "sum": (dict(), sb.W_SUM, False),
    "root_weight": (dict(root_weight=True), sb.W_SUM, True),
    "max": (dict(aggregator="max"), sb.W_NONE, False),
}


@pytest.mark.parametrize("model", list(MODELS))
def test_one_training_step_on_the_sampled_block(E, small, model):
    import test_host
    import test_max_driver
    import test_root_driver
    from nts import host
    layers, fanout, batch = test_max_driver.LAYERS, test_max_driver.FANOUT, test_max_driver.BATCH
    kw, flags, merge = MODELS[model]
    cfg = step_check.readout(host.gcn_config(layers, fanout, batch, drop_rate=0.0, shuffle=False,
                                             shared_sampling=True, **kw))
    assert cfg.rng_mode == 3
    drv = E.GCN_SAMPLE_ALLGPU_impl(small["G"], small["feat"], small["labels"], small["train"], cfg)
    W0 = [w.cpu().clone() for w in drv.weights()]
    drv.train_batch()
    drv.synchronize()
    W1 = [w.cpu().clone() for w in drv.weights()]
    ref = _assert_block_is_the_restatement(drv, small, fanout, batch, 0, flags, merge)
    deg = np.diff(_host_graph(small)[0].astype(np.int64))
    assert (deg[ref[1]["destination"]] > fanout[1]).sum() > 50  # the selection was exercised
    if model == "sum":
        chain = lambda dt: test_host._gcn_chain_grads(drv, small["feat"], small["labels"], W0, dt)
    elif model == "root_weight":
        chain = lambda dt: test_root_driver._chain_grads(drv, small, W0, dt)
    else:
        def chain(dt):
            g, gap = test_max_driver._chain_grads(drv, small, W0, False, dt)
            print(f"max: top-hop gap {gap:.3e}")
            assert gap > test_max_driver.GAP, "the reference's winners are too close"
            return g
    print(f"shared sampling, {model}")
    step_check.check_step_grads(W0, W1, chain(torch.float64), chain(torch.float32), step_check.C)


def test_one_gat_training_step_on_the_sampled_block(E, gat_data):
    import test_gat_heads_driver as tg
    from nts import host
    layers, heads, fanout, batch = [64, 64, 7], [8, 1], [10, 5], 200
    cfg = step_check.readout(host.gcn_config(layers, fanout, batch, drop_rate=0.0, shuffle=False,
                                             gat=True, pipeline=False, gat_heads=heads,
                                             shared_sampling=True))
    drv = E.GCN_SAMPLE_ALLGPU_impl(gat_data["G"], gat_data["feat"], gat_data["labels"],
                                   gat_data["train"], cfg)
    W0 = [w.cpu().clone() for w in drv.weights()]
    drv.train_batch()
    drv.synchronize()
    W1 = [w.cpu().clone() for w in drv.weights()]
    _assert_block_is_the_restatement(drv, gat_data, fanout, batch, 0, sb.W_NONE, True)
    loss64, g64 = tg._chain_grads(drv, gat_data, W0, layers, heads, torch.float64)
    loss32, g32 = tg._chain_grads(drv, gat_data, W0, layers, heads, torch.float32)
    got = float(drv.loss.detach())
    print(f"shared sampling, GAT {layers} heads {heads}: loss {got!r} float64 {loss64!r} "
          f"float32 chain {loss32!r}")
    assert abs(got - loss64) <= step_check.yardstick_bound(abs(loss32 - loss64) / abs(loss64),
                                                           step_check.C) * abs(loss64)
    step_check.check_step_grads(W0, W1, g64, g32, step_check.C, tg.NAMES)


def _sum_driver(E, data, layers=(64, 32, 7), fanout=(10, 5), batch=200, **kw):
    from nts import host
    cfg = host.gcn_config(list(layers), list(fanout), batch, drop_rate=0.0, shuffle=False, **kw)
    return E.GCN_SAMPLE_ALLGPU_impl(data["G"], data["feat"], data["labels"], data["train"], cfg)


def _losses(drv, n):
    out = []
    for _ in range(n):
        drv.train_batch()
        drv.synchronize()
        out.append(float(drv.loss.detach()))
    return out


def test_pipeline_on_and_off_train_identically(E, gat_data):
    on = _losses(_sum_driver(E, gat_data, shared_sampling=True, pipeline=True), 4)
    off = _losses(_sum_driver(E, gat_data, shared_sampling=True, pipeline=False), 4)
    plain = _losses(_sum_driver(E, gat_data, pipeline=False), 4)
    assert on == off and all(np.isfinite(on))
    assert on != plain  # another selection


def test_later_batches_are_the_restatement_too(E, gat_data):
    drv = _sum_driver(E, gat_data, shared_sampling=True)
    _losses(drv, 3)
    _assert_block_is_the_restatement(drv, gat_data, [10, 5], 200, 2, sb.W_SUM, False)


def test_the_frontier_is_smaller_than_the_philox_driver_s(E, gat_data):
    shared = _sum_driver(E, gat_data, batch=1024, shared_sampling=True, pipeline=False)
    plain = _sum_driver(E, gat_data, batch=1024, pipeline=False)
    for d in (shared, plain):
        d.train_batch()
        d.synchronize()
    (st, sb_), (pt, pb) = shared.last_layers, plain.last_layers
    assert torch.equal(st["destination"], pt["destination"])  # the same seeds
    print(f"hop-0 sources: philox {pt['src_size']} shared {st['src_size']}; "
          f"hop-1 sources: philox {pb['src_size']} shared {sb_['src_size']}")
    assert st["e_size"] == pt["e_size"]
    assert sb_["src_size"] < pb["src_size"]


def test_evaluate_runs_and_is_deterministic(E, gat_data):
    ids = torch.nonzero(gat_data["masks"].cpu() == 1).flatten().to(torch.int32)[:1000]
    a = _sum_driver(E, gat_data, shared_sampling=True)
    b = _sum_driver(E, gat_data, shared_sampling=True)
    _losses(a, 2)
    _losses(b, 2)
    # (an evaluation advances the driver's evaluation stream, as in the PHILOX
    # mode: the same sequence of calls gives the same sequence of scores)
    first, second = [a.evaluate(ids), a.evaluate(ids)], [b.evaluate(ids), b.evaluate(ids)]
    assert first == second and all(0.0 <= x <= 1.0 for x in first)


OPTIONS = [
    dict(weight="mean"), dict(weight="mean-sampled"), dict(up_degree=True),
    dict(early_aggregate=False), dict(transform_first=1), dict(transform_first=0),
    dict(cache_rate=0.5), dict(cache_rate=0.5, early_aggregate=False), dict(layer_norm=True),
    dict(root_weight=True, aggregator="max"), dict(gat=True, gat_v2=True),
    dict(gat=True, gat_heads=[4, 1], gat_attn_drop=0.2),
]


@pytest.mark.parametrize("kw", OPTIONS, ids=["-".join(f"{k}={v}" for k, v in o.items())
                                             for o in OPTIONS])
def test_the_mode_trains_with_every_option(E, gat_data, kw):
    """two drivers, three batches: finite, deterministic, and the trained
    block is the restatement's"""
    a = _losses(_sum_driver(E, gat_data, shared_sampling=True, **kw), 3)
    drv = _sum_driver(E, gat_data, shared_sampling=True, **kw)
    b = _losses(drv, 3)
    assert a == b and all(np.isfinite(a))
    wt = {"mean": sb.W_MEAN, "mean-sampled": sb.W_MEAN_SAMPLED}.get(kw.get("weight"), sb.W_SUM)
    if kw.get("gat") or kw.get("aggregator") == "max":
        wt = sb.W_NONE
    if kw.get("up_degree"):
        wt |= sb.W_UP_DEGREE
    _assert_block_is_the_restatement(drv, gat_data, [10, 5], 200, 2, wt,
                                     bool(kw.get("gat") or kw.get("root_weight")))


def test_multi_label_and_the_sampler_rate_entry_point(E, gat_data):
    from nts import synthetic
    labels = synthetic.multilabels(gat_data["feat"].shape[0], 7, gat_data["feat"], seed=13)
    from nts import host
    cfg = host.gcn_config([64, 32, 7], [10, 5], 200, drop_rate=0.0, shuffle=False,
                          multi_label=True, shared_sampling=True)
    drv = E.GCN_SAMPLE_ALLGPU_impl(gat_data["G"], gat_data["feat"], labels, gat_data["train"], cfg)
    assert all(np.isfinite(_losses(drv, 2)))
    r3 = E.sampler_throughput(gat_data["G"], gat_data["train"], 512, [10, 5], rng_mode=3, n_batches=4)
    r0 = E.sampler_throughput(gat_data["G"], gat_data["train"], 512, [10, 5], rng_mode=0, n_batches=4)
    assert r3["batches"] == r0["batches"] == 4 and r3["edges"] > 0
    print(f"sampler_throughput edges: philox {r0['edges']} shared {r3['edges']}")


SHARED_REFUSALS = {
    "sample_gpu": "shared sampling is not supported with sample_gpu (the reference's mt19937 stream)",
    "pd_cache": "shared sampling is not supported with pd_cache",
}


def _refusal(E, data, **kw):
    with pytest.raises(RuntimeError) as ei:
        _sum_driver(E, data, **kw)
    return str(ei.value).splitlines()[0]


@pytest.mark.parametrize("name", list(SHARED_REFUSALS))
def test_the_two_constructor_refusals(E, gat_data, name):
    assert _refusal(E, gat_data, shared_sampling=True, **{name: True}) == SHARED_REFUSALS[name]


def test_existing_conflicts_are_reported_before_the_new_ones(E, gat_data):
    from test_max_driver import REFUSALS as MAX_REFUSALS
    from test_root_driver import REFUSALS as ROOT_REFUSALS
    for name in SHARED_REFUSALS:
        assert _refusal(E, gat_data, shared_sampling=True, root_weight=True,
                        **{name: True}) == ROOT_REFUSALS[name]
        assert _refusal(E, gat_data, shared_sampling=True, aggregator="max",
                        **{name: True}) == MAX_REFUSALS[name]
    # the layer_norm / pd_cache one too
    assert _refusal(E, gat_data, shared_sampling=True, layer_norm=True,
                    pd_cache=True) == "layer_norm is not supported with pd_cache"


def test_cfg_runner_cora_accuracy_against_the_plain_job(tmp_path):
    """SAMPLE_SHARED:1 on the Cora job, 3 epochs, against the same cfg without
    the key, both under 5 seeds: seed by seed, the shared run's test accuracy
    is no lower than the plain run's minus the plain runs' own max - min over
    the seeds (what the yardstick cannot resolve).  The ten figures are in DESIGN §8o."""
    from conftest import GOLDEN
    from nts import run
    for f in ("cora.2708.edge.self", "cora.featuretable.zip", "cora.labeltable", "cora.mask"):
        shutil.copy(GOLDEN / "cora" / f, tmp_path / f)
    text = (GOLDEN / "cora" / "gcn_cora_sample.cfg").read_text()
    acc = {0: [], 1: []}
    for seed in (2000, 2001, 2002, 2003, 2004):
        for shared in (0, 1):
            (tmp_path / "job.cfg").write_text(text + f"SEED:{seed}\n" +
                                              ("SAMPLE_SHARED:1\n" if shared else ""))
            res = run.run(tmp_path / "job.cfg", epochs=3, out=lambda s: None)
            assert len(res["epochs"]) == 3
            acc[shared].append(res["epochs"][-1]["test_acc"])
    print("cora test accuracy after 3 epochs, seeds 2000..2004")
    print("  plain :", " ".join(f"{a:.4f}" for a in acc[0]))
    print("  shared:", " ".join(f"{a:.4f}" for a in acc[1]))
    spread = max(acc[0]) - min(acc[0])
    for plain, shared in zip(acc[0], acc[1]):  # seed by seed
        assert shared >= plain - spread, (acc, spread)
