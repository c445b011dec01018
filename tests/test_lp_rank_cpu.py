"""All-candidate ranking without a GPU: the reference's own
properties (tests/linkpred_rank_ref.py), the option refusals through the pure
validation pass, the cfg keys and the C-ABI entry."""
import re
import subprocess

import numpy as np
import pytest
import torch

import linkpred_rank_ref as ref
from conftest import ROOT


def _case(seed=0, V=40, D=6, M=12):
    rng = np.random.default_rng(seed)
    H = rng.integers(-2, 3, (V, D)).astype(np.float32)
    heads, tails = rng.integers(0, V, M), rng.integers(0, V, M)
    src, dst = rng.integers(0, V, 3 * V), rng.integers(0, V, 3 * V)
    return H, heads, tails, ref.sorted_adj(V, src, dst), (src, dst)


# ---- the reference ----------------------------------------------------------
def test_the_true_tail_is_never_counted():
    H, heads, tails, _, _ = _case()
    g, e, n = ref.counts(H, heads, tails, None, None)
    assert (n == H.shape[0] - 1).all()
    # a list of the true tail alone, however often: nothing is valid
    for i in range(len(heads)):
        g1, e1, n1 = ref.counts(H, heads[i:i + 1], tails[i:i + 1], [tails[i]] * 3, None)
        assert (g1[0], e1[0], n1[0]) == (0, 0, 0)


def test_a_repeated_candidate_counts_once_per_occurrence():
    H, heads, tails, adj, _ = _case(1)
    cand = np.random.default_rng(2).integers(0, H.shape[0], 25)
    for a in (None, adj):
        one = ref.counts(H, heads, tails, cand, a)
        two = ref.counts(H, heads, tails, np.concatenate([cand, cand]), a)
        for x, y in zip(one, two):
            assert np.array_equal(2 * x, y)


def test_the_filter_removes_the_self_pair_and_both_edge_directions():
    V = 6
    H = np.ones((V, 2), np.float32)  # every candidate ties
    adj = ref.sorted_adj(V, [0, 3], [1, 0])  # 0 -> 1 and 3 -> 0
    assert ref.blocked(adj, 0, 0) and ref.blocked(adj, 0, 1) and ref.blocked(adj, 0, 3)
    assert ref.blocked(adj, 1, 0) and not ref.blocked(adj, 0, 2) and not ref.blocked(adj, 1, 3)
    g, e, n = ref.counts(H, [0], [5], None, adj)
    assert (g[0], e[0], n[0]) == (0, 2, 2)  # 2 and 4 stay: not 0 (self), 1, 3 (edges), 5 (the tail)
    g, e, n = ref.counts(H, [0], [5], None, None)
    assert (g[0], e[0], n[0]) == (0, 5, 5)
    # the dense form of the mask is blocked() pair by pair
    H2, heads, tails, adj2, _ = _case(3)
    ok = ref.valid_mask(H2.shape[0], heads, tails, None, adj2)
    for i, (u, v) in enumerate(zip(heads, tails)):
        for w in range(H2.shape[0]):
            assert ok[i, w] == (w != v and not ref.blocked(adj2, int(u), w))


def test_metrics_hits_are_monotone_and_the_optimistic_mrr_is_no_lower():
    rng = np.random.default_rng(5)
    g, e = rng.integers(0, 60, 200), rng.integers(0, 4, 200)
    m = ref.metrics(g, e, ks=(1, 3, 10, 50, 100))
    hits = [m[f"hits@{k}"] for k in (1, 3, 10, 50, 100)]
    assert hits == sorted(hits) and hits[-1] == 1.0
    assert 0.0 < m["mrr"] <= m["mrr_optimistic"] <= 1.0
    assert m["n"] == 200 and m["ties"] == int(e.sum()) and m["mean_rank"] == (1 + g + e).mean()
    assert ref.metrics([0, 0], [0, 0])["mrr"] == 1.0


def test_bands_bracket_the_exact_counts():
    H, heads, tails, adj, _ = _case(7)
    H = (H + np.random.default_rng(8).standard_normal(H.shape)).astype(np.float32)
    g, e, n = ref.counts(H, heads, tails, None, adj)
    lo, hi, ge_lo, ge_hi, nv, amb = ref.bands(H, heads, tails, None, adj)
    assert np.array_equal(nv, n) and amb >= 0
    assert (lo <= g).all() and (g <= hi).all() and (ge_lo <= g + e).all() and (g + e <= ge_hi).all()


# ---- option rules -----------------------------------------------------------
def _cfg(**kw):
    from nts import host
    return host.gcn_config([16, 8, 8], [3, 3], 32, drop_rate=0.0, pipeline=False, neg_per_pos=2, **kw)


@pytest.mark.parametrize("kw,filtered,V,text", [
    (dict(weight="mean-sampled"), False, 200,
     "embed_full: MeanSampled weights are a property of a sample, not of the whole graph"),
    (dict(up_degree=True), False, 200,
     "embed_full: UP_DEGREE weights are a property of a sample, not of the whole graph"),
    (dict(), True, (1 << 31) + 1,
     "evaluate_full: filtered takes a graph of at most 2^31 vertices"),
])
def test_full_evaluation_refusals_carry_their_text(kw, filtered, V, text):
    from nts import host
    with pytest.raises(RuntimeError) as e:
        host.ext().check_link_pred_full(_cfg(**kw), n_vertices=V, filtered=filtered)
    assert str(e.value).splitlines()[0].startswith(text), str(e.value).splitlines()[0]


def test_full_evaluation_takes_what_it_supports():
    from nts import host
    check = host.ext().check_link_pred_full
    for kw in (dict(), dict(weight="mean"), dict(weight="none"), dict(shared_sampling=True)):
        check(_cfg(**kw), n_vertices=200, filtered=True)
    check(_cfg(), n_vertices=(1 << 31) + 1, filtered=False)  # unfiltered: no key table


# ---- cfg keys ---------------------------------------------------------------
HEAD = "VERTICES:10\nLAYERS:4-4-4\nFANOUT:2-2\nBATCH_SIZE:4\nEPOCHS:1\n"


def test_cfg_keys_parse_and_default_to_0(tmp_path):
    from nts import dataloader
    p = tmp_path / "lp.cfg"
    p.write_text("ALGORITHM:LINKPREDSAMPLE\n" + HEAD)
    info = dataloader.InputInfo.from_cfg(p)
    assert (info.lp_full_eval, info.lp_full_filter) == (0, 0)
    p.write_text("ALGORITHM:LINKPREDSAMPLE\n" + HEAD + "LP_FULL_EVAL:1\nLP_FULL_FILTER:1\n")
    info = dataloader.InputInfo.from_cfg(p)
    assert (info.lp_full_eval, info.lp_full_filter) == (1, 1) and not info.extra


@pytest.mark.parametrize("algo,keys,text", [
    ("GCNSAMPLEALLGPU", "LP_FULL_EVAL:1\n", "LP_FULL_EVAL is not supported outside ALGORITHM:LINKPREDSAMPLE"),
    ("GATSAMPLEALLGPU", "LP_FULL_FILTER:1\n", "LP_FULL_FILTER is not supported outside ALGORITHM:LINKPREDSAMPLE"),
    ("LINKPREDSAMPLE", "LP_FULL_FILTER:1\n", "LP_FULL_FILTER needs LP_FULL_EVAL:1"),
])
def test_runner_refuses_the_keys_before_any_file_is_loaded(tmp_path, algo, keys, text):
    from nts import run
    cfg = tmp_path / "job.cfg"
    cfg.write_text(f"ALGORITHM:{algo}\n" + HEAD + keys +
                   "EDGE_FILE:./no_such.edge\nFEATURE_FILE:./no_such.feat\n")
    with pytest.raises(SystemExit) as e:
        run.run(cfg, out=lambda *_: None)
    assert text in str(e.value)


# ---- C-ABI ------------------------------------------------------------------
def test_abi_exports_the_entry_and_keeps_its_version():
    from nts import _abi
    lib = _abi.lib()
    text = (ROOT / "include" / "nts_hip.h").read_text()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    s = "nts_hip_lp_rank"
    assert s in _abi.EXPORTED and hasattr(lib, s)
    assert re.search(rf"\bT {s}\b", out) and re.search(rf"^int {s}\(", text, flags=re.M)
    assert lib.nts_hip_abi_version() == _abi.ABI_VERSION == 11
    # a refusal needs no device: nothing is touched before the argument checks
    assert lib.nts_hip_lp_rank(None, None, 0, 0, 0, None, None, 0, None, 0, None, None, None, None,
                               None) == 1
