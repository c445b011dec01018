"""Subgraph-sampled training without a GPU: the numpy reference
of tests/subgraph_ref.py against a brute-force dense-adjacency intersection,
the option's refusals through the check_driver_options binding and through a
cfg, and the option's parsing.
"""
import numpy as np
import pytest
import torch

import shared_blocks as sb
import subgraph_ref as sr
from conftest import GOLDEN
from oracle import oracle as orc

LAYERS, FANOUT, BATCH, V = [8, 4, 2], [-1, -1], 4, 16
CFG = GOLDEN / "cora" / "gcn_cora_sample.cfg"


# ---- the reference itself ----
def _random_graph(seed, V, E):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, V, E).astype(np.uint32)  # parallel edges and self loops allowed
    dst = rng.integers(0, V - 3, E).astype(np.uint32)  # the last three vertices: in-degree 0
    col, rows = orc.build_csc(V, src, dst)
    od, idg = orc.degrees(V, src, dst)
    return src, dst, col, rows, od, idg


@pytest.mark.parametrize("seed,V_,E,square", [(0, 40, 300, True), (1, 40, 300, False),
                                              (2, 97, 2000, False), (3, 97, 150, True)])
def test_induced_block_is_the_dense_intersection(seed, V_, E, square):
    src, dst, col, rows, od, idg = _random_graph(seed, V_, E)
    rng = np.random.default_rng(100 + seed)
    members = rng.choice(V_, V_ // 3, replace=False)
    given = rng.permutation(np.concatenate([members, members[:5]])).astype(np.uint32)  # duplicates
    S = np.sort(members).astype(np.uint32)
    d = S if square else rng.permutation(S)[:max(S.size // 2, 1)]
    lay = sr.induced_layer(col, rows, idg, od, d, given, sr.W_SUM, merge=True)
    # multiplicity matrix A[dst, src] of the whole graph
    A = np.zeros((V_, V_), np.int64)
    np.add.at(A, (dst.astype(np.int64), src.astype(np.int64)), 1)
    sub = A[np.ix_(d.astype(np.int64), S.astype(np.int64))]
    assert np.array_equal(lay["source"], S)
    assert lay["e_size"] == sub.sum()
    B = np.zeros_like(sub)
    edst = np.repeat(np.arange(d.size), np.diff(lay["column_offset"].astype(np.int64)))
    np.add.at(B, (edst, lay["row_indices"].astype(np.int64)), 1)
    assert np.array_equal(B, sub)
    assert np.array_equal(lay["source"][lay["row_indices"]], lay["sample_ans"])
    assert np.array_equal(lay["source"][lay["dst_local_id"]], d)
    if square:
        assert np.array_equal(lay["dst_local_id"], np.arange(S.size))
    # CSC order of the graph is kept inside every column
    for i, dd in enumerate(d):
        nb = rows[int(col[dd]):int(col[dd + 1])]
        want = nb[np.isin(nb, S)]
        got = lay["sample_ans"][lay["column_offset"][i]:lay["column_offset"][i + 1]]
        assert np.array_equal(got, want)
    # the CSR is the stable transpose
    T = np.zeros_like(sub)
    esrc = np.repeat(np.arange(S.size), np.diff(lay["row_offset"].astype(np.int64)))
    np.add.at(T, (lay["column_indices"].astype(np.int64), esrc), 1)
    assert np.array_equal(T, sub)
    assert np.array_equal(lay["row_indices"][lay["csr_edge_id"]], esrc)


def test_walk_reference_follows_in_neighbours_and_stays_at_degree_zero():
    src, dst, col, rows, od, idg = _random_graph(7, 60, 500)
    roots = np.array([0, 59, 58, 5, 5, 17], np.uint32)  # 58, 59: in-degree 0
    w = sr.random_walk(col, rows, roots, 4, 2000, 3)
    assert w.shape == (6, 5) and np.array_equal(w[:, 0], roots)
    assert (w[1] == 59).all() and (w[2] == 58).all()
    assert np.array_equal(w[3], w[4])  # the same root walks the same path
    for r in (0, 3, 5):
        for t in range(4):
            u, nxt = int(w[r, t]), int(w[r, t + 1])
            nb = rows[int(col[u]):int(col[u + 1])]
            assert nxt in nb if nb.size else nxt == u
    assert not np.array_equal(w, sr.random_walk(col, rows, roots, 4, 2000, 4))
    # the word is word 0 of the documented counter
    x = sr.walk_word(np.array([5], np.uint32), 2, 2000, 3)[0]
    c = [np.array([v], np.uint32) for v in (0, 5, 0x10000002, 3)]
    assert x == sb.philox4x32_10(c, (2000, 0))[0][0]


# ---- the option ----
def facts(**kw):
    f = dict(feature_dtype=torch.float32, feature_on_gpu=True, feature_cols=LAYERS[0],
             label_shape=[V], label_on_gpu=True, n_vertices=V, has_edge_prob=False)
    f.update(kw)
    return f


def check(cfg_edit=None, inputs=None, fanout=FANOUT, **kw):
    from nts import host
    cfg = host.gcn_config(LAYERS, fanout, BATCH, **kw)
    if cfg_edit:
        cfg_edit(cfg)
    host.ext().check_driver_options(cfg, **facts(**(inputs or {})))
    return cfg


def refusal(cfg_edit=None, **kw):
    with pytest.raises(RuntimeError) as ei:
        check(cfg_edit, **kw)
    return str(ei.value).splitlines()[0]


def _set(**fields):
    def edit(cfg):
        for k, v in fields.items():
            setattr(cfg, k, v)
    return edit


REFUSALS = {
    "fanout": (dict(fanout=[-1, 10]), None,
               "subgraph needs every fanout = -1 (all induced neighbours; other values are kept "
               "for a fanout-capped meaning)"),
    "walk": (dict(subgraph_walk=65), None, "subgraph needs subgraph_walk in [0, 64], got 65"),
    "walk-negative": (dict(subgraph_walk=-1), None,
                      "subgraph needs subgraph_walk in [0, 64], got -1"),
    "edge_cap": (dict(subgraph_edge_cap=-2), None,
                 "subgraph needs subgraph_edge_cap in [0, 2^32) (0 = the default), got -2"),
    "gat": (dict(gat=True, weight="none"), None,
            "subgraph is not supported with gat (GCN / GraphSAGE layers only)"),
    "max": (dict(aggregator="max"), None, "subgraph is not supported with aggregator = max"),
    "pd_cache": (dict(pd_cache=True), None, "subgraph is not supported with pd_cache"),
    "sample_gpu": (dict(sample_gpu=True, rng_mode=1), None,
                   "subgraph is not supported with sample_gpu (the reference's mt19937 stream)"),
    "mt": (dict(rng_mode=1), None,
           "subgraph is not supported with an MT19937 rng_mode (the walks draw from a Philox "
           "stream of their own)"),
    "mt-div": (dict(rng_mode=2), None,
               "subgraph is not supported with an MT19937 rng_mode (the walks draw from a Philox "
               "stream of their own)"),
    "shared": (dict(shared_sampling=True), None,
               "subgraph is not supported with rng_mode NTS_RNG_PHILOX_SHARED (shared_sampling): "
               "an induced block selects nothing"),
    "weighted_sampling": (dict(weighted_sampling=True), dict(has_edge_prob=True),
                          "subgraph is not supported with weighted_sampling (the walks are uniform)"),
    "edge_weighted": (dict(edge_weighted=True), dict(has_edge_prob=True),
                      "subgraph is not supported with edge_weighted"),
    "cache_rate": (dict(cache_rate=0.5), None, "subgraph is not supported with cache_rate >= 0"),
    "layer_norm": (dict(layer_norm=True), None, "subgraph is not supported with layer_norm"),
    "batch_norm": (dict(batch_norm=True), None, "subgraph is not supported with batch_norm"),
    "multi_label": (dict(multi_label=True), dict(label_shape=[V, LAYERS[-1]]),
                    "subgraph is not supported with multi_label"),
    "feature_f16": (dict(feature_f16=True), None, "subgraph is not supported with feature_f16"),
    "transform_first": (dict(transform_first=1), None,
                        "subgraph is not supported with transform_first = 1 (aggregate-first only)"),
    "pair_table": (dict(pair_table=3), None, "subgraph is not supported with pair_table > 0"),
    "fused_gather": (dict(fused_gather=False), None,
                     "subgraph is not supported with fused_gather = false"),
    "deterministic_backward": (dict(deterministic_backward=False), None,
                               "subgraph is not supported with deterministic_backward = false"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_every_refusal_text(name):
    kw, inputs, text = REFUSALS[name]
    kw = dict(kw)
    kw.setdefault("subgraph_walk", 2)
    assert refusal(subgraph=True, inputs=inputs, **kw) == text
    # the same configuration without the option is accepted (its fanout aside)
    kw.pop("subgraph_walk")
    kw.pop("subgraph_edge_cap", None)
    check(inputs=inputs, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(subgraph_walk=2), dict(subgraph_walk=64),
                                dict(up_degree=True), dict(root_weight=True),
                                dict(weight="mean"), dict(weight="mean-sampled"),
                                dict(weight="none"), dict(pipeline=False),
                                dict(subgraph_edge_cap=1000)])
def test_accepted_configurations(kw):
    cfg = check(subgraph=True, **kw)
    assert cfg.subgraph and cfg.subgraph_walk == kw.get("subgraph_walk", 0)
    assert cfg.subgraph_edge_cap == kw.get("subgraph_edge_cap", 0)


def test_an_earlier_options_conflict_is_reported_first():
    """the table is the last of check_driver_options: report order is source order"""
    from test_root_driver import REFUSALS as ROOT_REFUSALS
    assert refusal(subgraph=True, root_weight=True, pd_cache=True) == ROOT_REFUSALS["pd_cache"]
    assert refusal(_set(layer_size=[8, 4, 4, 2]), subgraph=True) == "fanout per layer"


def test_option_off_leaves_the_config_as_it_is():
    from nts import host
    base = host.gcn_config(LAYERS, [2, 2], BATCH)
    off = host.gcn_config(LAYERS, [2, 2], BATCH, subgraph=False, subgraph_walk=3,
                          subgraph_edge_cap=99)
    fresh = host.ext().GCNConfig()
    names = [n for n in dir(base) if not n.startswith("_")]
    assert {"subgraph", "subgraph_walk", "subgraph_edge_cap", "fanout", "rng_mode"} <= set(names)
    for n in names:
        assert getattr(base, n) == getattr(off, n), n
    assert (off.subgraph, off.subgraph_walk, off.subgraph_edge_cap) == (
        fresh.subgraph, fresh.subgraph_walk, fresh.subgraph_edge_cap) == (False, 0, 0)
    check(fanout=[2, 2])  # and the job it describes is accepted as before


# ---- the cfg runner ----
def _job(tmp_path, extra, fanout="-1--1", algorithm=None):
    text = CFG.read_text()
    assert "ALGORITHM:GCNSAMPLEALLGPU" in text
    lines = [l for l in text.splitlines() if not l.startswith("FANOUT:")]
    text = "\n".join(lines) + f"\nFANOUT:{fanout}\n" + extra
    if algorithm:
        text = text.replace("ALGORITHM:GCNSAMPLEALLGPU", f"ALGORITHM:{algorithm}")
    (tmp_path / "job.cfg").write_text(text)
    return tmp_path / "job.cfg"


def test_cfg_keys_parse(tmp_path):
    from nts import dataloader
    info = dataloader.InputInfo.from_cfg(_job(tmp_path, "SUBGRAPH:1\nSUBGRAPH_WALK:2\n"
                                                        "SUBGRAPH_EDGE_CAP:5000\n"))
    assert (info.subgraph, info.subgraph_walk, info.subgraph_edge_cap) == (1, 2, 5000)
    assert info.fanout == [-1, -1]
    plain = dataloader.InputInfo.from_cfg(CFG)
    assert (plain.subgraph, plain.subgraph_walk, plain.subgraph_edge_cap) == (0, 0, 0)


CFG_REFUSALS = [
    ("SUBGRAPH:1\n", "25-10", None, "SUBGRAPH needs FANOUT -1 for every layer"),
    ("SUBGRAPH:1\nSUBGRAPH_WALK:65\n", "-1--1", None, "SUBGRAPH_WALK must be in [0, 64], got 65"),
    ("SUBGRAPH:1\nSUBGRAPH_EDGE_CAP:-1\n", "-1--1", None, "SUBGRAPH_EDGE_CAP must be >= 0, got -1"),
    ("SUBGRAPH:1\n", "-1--1", "GATSAMPLEALLGPU", "SUBGRAPH is not supported with GAT algorithms"),
    ("SUBGRAPH:1\nAGGREGATOR:max\n", "-1--1", None, "SUBGRAPH is not supported with AGGREGATOR:max"),
    ("SUBGRAPH:1\n", "-1--1", "GCNSAMPLEPDCACHE",
     "SUBGRAPH is not supported with the PD-cache algorithms"),
    ("SUBGRAPH:1\n", "-1--1", "GCNSAMPLEGPU", "SUBGRAPH is not supported with GCNSAMPLEGPU"),
    ("SUBGRAPH:1\n", "-1--1", "GCNSAMPLESINGLE",
     "SUBGRAPH is not supported with the mt19937-stream algorithms"),
    ("SUBGRAPH:1\nSAMPLE_SHARED:1\n", "-1--1", None,
     "SUBGRAPH is not supported with SAMPLE_SHARED:1"),
    ("SUBGRAPH:1\nSAMPLE_WEIGHTED:1\nEDGE_WEIGHT_FILE:w.bin\n", "-1--1", None,
     "SUBGRAPH is not supported with SAMPLE_WEIGHTED:1"),
    ("SUBGRAPH:1\nEDGE_WEIGHT_AGG:1\nEDGE_WEIGHT_FILE:w.bin\n", "-1--1", None,
     "SUBGRAPH is not supported with EDGE_WEIGHT_AGG:1"),
    ("SUBGRAPH:1\nLAYER_NORM:1\n", "-1--1", None, "SUBGRAPH is not supported with LAYER_NORM:1"),
    ("SUBGRAPH:1\nBATCH_NORM:1\n", "-1--1", None, "SUBGRAPH is not supported with BATCH_NORM:1"),
    ("SUBGRAPH:1\nMULTI_LABEL:1\n", "-1--1", None, "SUBGRAPH is not supported with MULTI_LABEL:1"),
    ("SUBGRAPH:1\nFEATURE_F16:1\n", "-1--1", None, "SUBGRAPH is not supported with FEATURE_F16:1"),
    ("SUBGRAPH_WALK:2\n", "25-10", None,
     "SUBGRAPH_WALK / SUBGRAPH_EDGE_CAP are not supported without SUBGRAPH:1"),
]


@pytest.mark.parametrize("extra,fanout,algorithm,text", CFG_REFUSALS,
                         ids=[f"{i}-{t[3].split()[-1]}" for i, t in enumerate(CFG_REFUSALS)])
def test_cfg_refusals_before_anything_is_loaded(tmp_path, extra, fanout, algorithm, text):
    """none of the cfg's data files exist beside this copy"""
    from nts import run
    job = _job(tmp_path, extra, fanout, algorithm)
    with pytest.raises(SystemExit) as ei:
        run.run(job, epochs=1, out=lambda s: None)
    alg = algorithm or "GCNSAMPLEALLGPU"
    assert str(ei.value).startswith(f"ALGORITHM {alg}: {text}"), str(ei.value)
