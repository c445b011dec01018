"""Link prediction without a GPU: the numpy reference's own
invariants, the option rules, the runner's early refusal and the C-ABI."""
import re
import subprocess

import numpy as np
import pytest
import torch

import linkpred_ref as ref
from conftest import ROOT

SYMS = ("nts_hip_lp_batch", "nts_hip_lp_bce_fwd", "nts_hip_lp_bce_train")


@pytest.mark.parametrize("V,B,K,seq", [(64, 5, 3, 0), (3, 4, 4, 1), (50, 1, 1, 2), (1000, 40, 5, 1 << 40),
                                       (100003, 33, 2, 9)])
def test_reference_invariants(V, B, K, seq):
    rng = np.random.default_rng([V, B, K])
    ps, pd = rng.integers(0, V, B), rng.integers(0, V, B)
    t = ref.negative_tails(B, K, V, 2000, seq)
    assert t.shape == (B, K) and (t < V).all()
    b = ref.batch(ps, pd, K, V, 2000, seq)
    P = B * (1 + K)
    d = b["destination"].astype(np.int64)
    assert (np.diff(d) > 0).all()
    assert set(d.tolist()) == set(b["gu"].tolist()) | set(b["gv"].tolist())
    assert np.array_equal(b["destination"][b["pair_u"]], b["gu"])
    assert np.array_equal(b["destination"][b["pair_v"]], b["gv"])
    assert np.array_equal(b["gu"][B:].reshape(B, K), np.repeat(ps, K).reshape(B, K))
    off, slot = b["inc_offset"].astype(np.int64), b["inc_slot"].astype(np.int64)
    assert off[0] == 0 and off[-1] == 2 * P and off.size == b["v_size"] + 1
    assert np.array_equal(np.sort(slot), np.arange(2 * P))
    for r in range(b["v_size"]):
        s = slot[off[r]:off[r + 1]]
        assert (np.diff(s) > 0).all()
        for x in s:
            assert (b["pair_v"] if x & 1 else b["pair_u"])[x >> 1] == r


def test_tails_differ_between_batches_words_and_positives():
    a = ref.negative_tails(8, 5, 1 << 20, 2000, 0)
    assert not np.array_equal(a, ref.negative_tails(8, 5, 1 << 20, 2000, 1))
    assert not np.array_equal(a, ref.negative_tails(8, 5, 1 << 20, 2001, 0))
    assert len(set(a.reshape(-1).tolist())) > 30
    # the first K words do not depend on K
    assert np.array_equal(a[:, :3], ref.negative_tails(8, 3, 1 << 20, 2000, 0))


def test_rank_counts_ties_against_the_positive():
    s = np.array([1.0, 0.0, 1.0, 0.5, 0.0, -1.0])  # B = 2, K = 2
    assert ref.ranks(s, 2, 2).tolist() == [2, 2]
    assert ref.mrr_counter(s, 2, 2) == np.float32(1.0)


def _cfg(**kw):
    from nts import host
    return host.gcn_config([16, 8, 8], [3, 3], 32, **kw)


def _check(cfg, **over):
    from nts import host
    kw = dict(feature_dtype=torch.float32, feature_on_gpu=True, feature_cols=16, edge_shape=[2, 100],
              edges_on_host=True, n_vertices=200, has_edge_prob=False)
    kw.update(over)
    host.ext().check_link_pred_options(cfg, **kw)


def test_default_link_pred_options_are_accepted():
    c = _cfg()
    assert c.neg_per_pos == 1
    _check(c)
    _check(_cfg(neg_per_pos=3, shared_sampling=True))


def _set(c, **fields):
    for k, v in fields.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("fields,text", [
    (dict(gat=True), "link prediction is not supported with gat"),
    (dict(aggregator=1), "link prediction is not supported with aggregator = max"),
    (dict(root_weight=True), "link prediction is not supported with root_weight"),
    (dict(pd_cache=True), "link prediction is not supported with pd_cache"),
    (dict(sample_gpu=True), "link prediction is not supported with sample_gpu"),
    (dict(rng_mode=1), "link prediction is not supported with an MT19937 rng_mode"),
    (dict(rng_mode=2), "link prediction is not supported with an MT19937 rng_mode"),
    (dict(cache_rate=0.0), "link prediction is not supported with cache_rate >= 0"),
    (dict(multi_label=True), "link prediction is not supported with multi_label"),
    (dict(layer_norm=True), "link prediction is not supported with layer_norm"),
    (dict(batch_norm=True), "link prediction is not supported with batch_norm"),
    (dict(feature_f16=True), "link prediction is not supported with feature_f16"),
    (dict(transform_first=1), "link prediction is not supported with transform_first = 1"),
    (dict(pair_table=1), "link prediction is not supported with pair_table > 0"),
    (dict(neg_per_pos=0), "link prediction needs neg_per_pos >= 1, got 0"),
    (dict(layer_size=[16, 8, 1028]), "link prediction takes an embedding width of at most 1024, got 1028"),
])
def test_each_unsupported_option_is_refused_with_its_own_text(fields, text):
    c = _set(_cfg(), **fields)
    with pytest.raises(RuntimeError) as e:
        _check(c)
    assert str(e.value).splitlines()[0].startswith(text), str(e.value).splitlines()[0]


def test_input_shapes_are_refused():
    with pytest.raises(RuntimeError, match="feature table must be fp32"):
        _check(_cfg(), feature_cols=15)
    with pytest.raises(RuntimeError, match=r"train_edges must be int64 \[2, n\] on the host"):
        _check(_cfg(), edge_shape=[100, 2])
    with pytest.raises(RuntimeError, match="train_edges must be"):
        _check(_cfg(), edges_on_host=False)


def test_check_driver_options_does_not_read_neg_per_pos():
    from nts import host
    c = _cfg(neg_per_pos=0)
    host.ext().check_driver_options(c, feature_dtype=torch.float32, feature_on_gpu=True,
                                    feature_cols=16, label_shape=[200], label_on_gpu=True,
                                    n_vertices=200, has_edge_prob=False)


def test_runner_refuses_neg_per_pos_0_before_any_file_is_loaded(tmp_path):
    from nts import run
    cfg = tmp_path / "lp.cfg"
    cfg.write_text("ALGORITHM:LINKPREDSAMPLE\nVERTICES:10\nLAYERS:4-4-4\nFANOUT:2-2\nBATCH_SIZE:4\n"
                   "EPOCHS:1\nNEG_PER_POS:0\nEDGE_FILE:./no_such.edge\nFEATURE_FILE:./no_such.feat\n")
    with pytest.raises(SystemExit, match="NEG_PER_POS must be >= 1, got 0"):
        run.run(cfg, out=lambda *_: None)


def test_cfg_keys_parse():
    from nts import dataloader
    import tempfile, pathlib
    with tempfile.TemporaryDirectory() as d:
        p = pathlib.Path(d) / "lp.cfg"
        p.write_text("ALGORITHM:LINKPREDSAMPLE\nVERTICES:10\nLAYERS:4-4-4\nFANOUT:2-2\nBATCH_SIZE:4\n"
                     "NEG_PER_POS:3\nVAL_EDGE_RATE:0.25\n")
        info = dataloader.InputInfo.from_cfg(p)
    assert info.algorithm == "LINKPREDSAMPLE" and info.neg_per_pos == 3 and info.val_edge_rate == 0.25


def test_abi_exports_the_link_prediction_entries():
    from nts import _abi
    lib = _abi.lib()
    text = (ROOT / "include" / "nts_hip.h").read_text()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    for s in SYMS:
        assert s in _abi.EXPORTED and hasattr(lib, s)
        assert re.search(rf"\bT {s}\b", out), s
        assert re.search(rf"^int {s}\(", text, flags=re.M), s
    # the entries are additions (no struct or existing signature changed): the
    # library, the header and the bindings agree on one version
    m = re.search(r"^#define NTS_HIP_ABI_VERSION (\d+)\b", text, flags=re.M)
    assert lib.nts_hip_abi_version() == _abi.ABI_VERSION == int(m.group(1))
    # the header says that negatives are not filtered against true edges
    assert "negatives are not filtered" in re.sub(r"[\s*]+", " ", text).lower()
