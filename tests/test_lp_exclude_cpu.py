"""Target-edge exclusion and filtered negatives without a GPU: the
numpy reference's own checks, the option plumbing and refusals, the cfg keys,
LP_HOLDOUT_REMOVE's graph and the C-ABI."""
import re
import subprocess

import numpy as np
import pytest
import torch

import linkpred_excl_ref as xref
import linkpred_ref as ref
from conftest import GOLDEN, ROOT

SYMS = ("nts_hip_lp_exclude_keys", "nts_hip_lp_mask_block", "nts_hip_lp_batch_filtered")


# ---- the reference ----------------------------------------------------------
def test_key_table_is_distinct_ascending_and_collapses_duplicates():
    ps = np.array([3, 3, 7, 5, 9], np.uint32)
    pd = np.array([4, 4, 7, 9, 5], np.uint32)  # a repeat, a self pair, a pair with its reverse
    k = xref.keys(ps, pd, False)
    assert k.dtype == np.uint64 and (np.diff(k.astype(object)) > 0).all()
    assert k.tolist() == sorted({(4 << 32) | 3, (7 << 32) | 7, (9 << 32) | 5, (5 << 32) | 9})
    r = xref.keys(ps, pd, True)
    assert r.tolist() == sorted({(4 << 32) | 3, (3 << 32) | 4, (7 << 32) | 7, (9 << 32) | 5, (5 << 32) | 9})
    big = xref.keys([0xFFFFFFFF, 0], [1 << 31, 0xFFFFFFFF], True)
    assert big.tolist() == sorted({((1 << 31) << 32) | 0xFFFFFFFF, (0xFFFFFFFF << 32) | (1 << 31),
                                   (0xFFFFFFFF << 32) | 0, 0xFFFFFFFF})


def test_mask_reference():
    t = xref.keys([1, 2], [5, 6], False)
    hit = xref.hits(t, [5, 5, 6, 6], [1, 2, 2, 1])
    assert hit.tolist() == [True, False, True, False]
    w = np.array([0.5, 0.25, 2.0, 3.0], np.float32)
    assert xref.mask(w, hit, True).tolist() == [0.0, 0.25, 0.0, 3.0]
    assert xref.mask(w, hit, False).tolist() == [0.0, 1.0, 0.0, 1.0]
    assert xref.csr_rows([0, 2, 2, 5], 5).tolist() == [0, 0, 2, 2, 2]


@pytest.mark.parametrize("V,B,K,seq", [(64, 5, 3, 0), (50, 1, 1, 2), (1000, 40, 5, 1 << 40)])
def test_try_0_is_the_unfiltered_draw(V, B, K, seq):
    assert np.array_equal(xref.candidate_tails(B, K, V, 2000, seq, 0), ref.negative_tails(B, K, V, 2000, seq))
    assert not np.array_equal(xref.candidate_tails(B, K, V, 2000, seq, 1),
                              xref.candidate_tails(B, K, V, 2000, seq, 0)) or B * K < 3


def test_no_edge_at_the_heads_gives_the_unfiltered_batch():
    V, B, K = 500, 20, 5
    rng = np.random.default_rng(3)
    ps, pd = rng.integers(0, 250, B), rng.integers(0, V, B)
    # edges among vertices >= 250 only: no head has one
    edges = xref.edge_set(rng.integers(250, V, 400), rng.integers(250, V, 400))
    got = xref.batch(ps, pd, K, V, 2000, 7, edges)
    want = ref.batch(ps, pd, K, V, 2000, 7)
    self_pairs = (want["gu"][B:] == want["gv"][B:]).sum()
    assert self_pairs == 0  # (a self pair would be redrawn: choose another seed)
    assert got["unresolved"] == 0
    for k in ("destination", "pair_u", "pair_v", "inc_offset", "inc_slot", "gu", "gv"):
        assert np.array_equal(got[k], want[k]), k


def test_filtered_reference_rejects_edges_self_pairs_and_counts_the_unresolvable():
    V, B, K = 8, 6, 5
    rng = np.random.default_rng(5)
    s, d = rng.integers(0, V, 30), rng.integers(0, V, 30)
    s, d = np.concatenate([s, np.full(V, 2)]), np.concatenate([d, np.arange(V)])  # 2 -> everyone
    edges = xref.edge_set(s, d)
    ps = np.array([0, 1, 2, 3, 4, 2])
    tails, unresolved = xref.filtered_tails(ps, K, V, 2000, 0, edges)
    bad = 0
    for i in range(B):
        for k in range(K):
            u, w = int(ps[i]), int(tails[i, k])
            if u == w or (u, w) in edges or (w, u) in edges:
                bad += 1
                assert u == 2 and w == xref.candidate_tails(B, K, V, 2000, 0, 15)[i, k]
    assert bad == unresolved == 2 * K


# ---- options ----------------------------------------------------------------
def _cfg(**kw):
    from nts import host
    return host.gcn_config([16, 8, 8], [3, 3], 32, **kw)


def _check(cfg, **over):
    from nts import host
    kw = dict(feature_dtype=torch.float32, feature_on_gpu=True, feature_cols=16, edge_shape=[2, 100],
              edges_on_host=True, n_vertices=200, has_edge_prob=False)
    kw.update(over)
    host.ext().check_link_pred_options(cfg, **kw)


def test_gcn_config_round_trips_the_fields_and_defaults_leave_them_alone():
    from nts import host
    fresh = host.ext().GCNConfig()
    assert fresh.lp_exclude == 0 and fresh.lp_filter_neg is False
    c = _cfg()
    assert c.lp_exclude == 0 and c.lp_filter_neg is False
    assert _cfg(lp_exclude="none").lp_exclude == 0
    assert _cfg(lp_exclude="self").lp_exclude == 1
    c = _cfg(lp_exclude="reverse", filter_negatives=True)
    assert c.lp_exclude == 2 and c.lp_filter_neg is True
    _check(c)
    _check(_cfg(lp_exclude="self", weight="none", shared_sampling=True))
    with pytest.raises(ValueError, match="lp_exclude must be 'none', 'self' or 'reverse'"):
        _cfg(lp_exclude="both")


@pytest.mark.parametrize("fields,text", [
    (dict(lp_exclude=3), "lp_exclude must be 0 (none), 1 (self) or 2 (reverse), got 3"),
    (dict(lp_exclude=-1), "lp_exclude must be 0 (none), 1 (self) or 2 (reverse), got -1"),
    (dict(lp_exclude=1, weight_type="MeanSampled"), "lp_exclude is not supported with the mean-sampled weights"),
    (dict(lp_exclude=2, up_degree=True), "lp_exclude is not supported with up_degree"),
])
def test_each_new_refusal_has_its_own_text(fields, text):
    from nts import host
    c = _cfg()
    for k, v in fields.items():
        setattr(c, k, getattr(host.ext().WeightType, v) if k == "weight_type" else v)
    with pytest.raises(RuntimeError) as e:
        _check(c)
    assert str(e.value).splitlines()[0].startswith(text), str(e.value).splitlines()[0]


def test_filter_refuses_more_than_2_31_vertices():
    with pytest.raises(RuntimeError, match="lp_filter_neg takes a graph of at most 2\\^31 vertices"):
        _check(_cfg(filter_negatives=True), n_vertices=(1 << 31) + 1)
    _check(_cfg(), n_vertices=(1 << 31) + 1)


def test_link_predictor_refuses_before_anything_is_built():
    """host.link_predictor runs the rules on facts about its inputs: no graph
    and no device is touched before the rule's text comes back"""
    from nts import host

    class G:  # what the rules read of a graph
        global_vertices, edge_prob = 200, None
    c = _cfg(lp_exclude="reverse", up_degree=True)
    with pytest.raises(ValueError, match="lp_exclude is not supported with up_degree"):
        host.link_predictor(G, torch.zeros(200, 16), torch.zeros(2, 10, dtype=torch.int64), c)


def test_node_classification_rules_do_not_read_the_fields():
    from nts import host
    c = _cfg(up_degree=True)
    c.lp_exclude, c.lp_filter_neg = 7, True
    host.ext().check_driver_options(c, feature_dtype=torch.float32, feature_on_gpu=True,
                                    feature_cols=16, label_shape=[200], label_on_gpu=True,
                                    n_vertices=200, has_edge_prob=False)


def test_cfg_keys_parse(tmp_path):
    from nts import dataloader
    p = tmp_path / "lp.cfg"
    head = "ALGORITHM:LINKPREDSAMPLE\nVERTICES:10\nLAYERS:4-4-4\nFANOUT:2-2\nBATCH_SIZE:4\n"
    p.write_text(head)
    info = dataloader.InputInfo.from_cfg(p)
    assert (info.lp_exclude, info.lp_filter_neg, info.lp_holdout_remove) == ("none", 0, 0)
    p.write_text(head + "LP_EXCLUDE:Reverse\nLP_FILTER_NEG:1\nLP_HOLDOUT_REMOVE:1\n")
    info = dataloader.InputInfo.from_cfg(p)
    assert (info.lp_exclude, info.lp_filter_neg, info.lp_holdout_remove) == ("reverse", 1, 1)
    assert not info.extra


def test_runner_refuses_an_unknown_lp_exclude_before_any_file_is_loaded(tmp_path):
    from nts import run
    cfg = tmp_path / "lp.cfg"
    cfg.write_text("ALGORITHM:LINKPREDSAMPLE\nVERTICES:10\nLAYERS:4-4-4\nFANOUT:2-2\nBATCH_SIZE:4\n"
                   "EPOCHS:1\nLP_EXCLUDE:both\nEDGE_FILE:./no_such.edge\nFEATURE_FILE:./no_such.feat\n")
    with pytest.raises(SystemExit, match="LP_EXCLUDE must be none, self or reverse, got both"):
        run.run(cfg, out=lambda *_: None)


# ---- LP_HOLDOUT_REMOVE ------------------------------------------------------
def test_holdout_remove_on_the_cora_edges():
    from collections import Counter

    from nts import dataloader, run
    src, dst = dataloader.read_edge_file(GOLDEN / "cora" / "cora.2708.edge.self")
    src, dst = src.astype(np.int64), dst.astype(np.int64)
    tr, va = run.split_edges(src.size, 0.1, 2000)
    keep = run.message_passing_edges(src, dst, va)
    assert (np.diff(keep) > 0).all() and keep.size < tr.size  # reverses left as well
    held = set(zip(src[va].tolist(), dst[va].tolist()))
    gone = held | {(d, s) for s, d in held}
    kept = Counter(zip(src[keep].tolist(), dst[keep].tolist()))
    assert not (set(kept) & gone)
    # every other edge stays with its multiplicity
    every = Counter(zip(src.tolist(), dst.tolist()))
    for e, n in every.items():
        if e not in gone:
            assert kept[e] == n, e
    assert sum(kept.values()) == sum(n for e, n in every.items() if e not in gone)
    # an edge list without any reverse: exactly the held-out positions leave
    s2, d2 = np.arange(10), np.arange(10) + 100
    assert run.message_passing_edges(s2, d2, np.array([2, 5])).tolist() == [0, 1, 3, 4, 6, 7, 8, 9]
    # nothing held out: the whole list, as with the key absent
    assert np.array_equal(run.message_passing_edges(src, dst, np.array([], np.int64)), np.arange(src.size))


# ---- C-ABI ------------------------------------------------------------------
def test_abi_exports_the_new_entries_and_keeps_its_version():
    from nts import _abi
    lib = _abi.lib()
    text = (ROOT / "include" / "nts_hip.h").read_text()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    for s in SYMS:
        assert s in _abi.EXPORTED and hasattr(lib, s)
        assert re.search(rf"\bT {s}\b", out), s
        assert re.search(rf"^int {s}\(", text, flags=re.M), s
    assert lib.nts_hip_abi_version() == _abi.ABI_VERSION == 11
