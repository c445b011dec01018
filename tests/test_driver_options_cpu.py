"""The driver's option and shape rules without a GPU (nts/host/options.cpp):
GCN_SAMPLE_ALLGPU_impl's constructor runs check_driver_options() before it
builds anything, and the same function is bound for a process that never
opens a device.  Here it is called with the facts of a toy job (V = 16, layers
8-4-2, fanout 2-2: the shapes of tests/test_option_refusals.py).  The texts
are the ones the driver tests pin, imported from their tables; importing those
modules allocates nothing.
"""
import ast
import importlib.util
import re
import shlex

import pytest
import torch

import test_option_refusals as order
from conftest import GOLDEN, ROOT
from test_edge_weighted_driver import REFUSALS as EDGE_REFUSALS
from test_f16_features_driver import REFUSALS as F16_REFUSALS
from test_layer_norm_driver import REFUSALS as LN_REFUSALS
from test_max_driver import REFUSALS as MAX_REFUSALS
# the four order properties of tests/test_option_refusals.py, collected here
# too: in this module their `build` fixture is the pure check below
from test_option_refusals import (  # noqa: F401
    test_conflicts_are_reported_in_one_order, test_root_weight_is_reported_before_max,
    test_unknown_aggregator_is_refused_after_root_weight,
    test_up_degree_is_reported_after_the_shared_conflicts)
from test_root_driver import REFUSALS as ROOT_REFUSALS
from test_shared_sampling_driver import SHARED_REFUSALS

LAYERS, FANOUT, BATCH, V = order.LAYERS, order.FANOUT, order.BATCH, order.V
CFG = GOLDEN / "cora" / "gcn_cora_sample.cfg"


def facts(layers=LAYERS, **kw):
    """what the constructor would read of an fp32 table, int64 [V] labels and
    a graph without edge_prob, all on the GPU"""
    f = dict(feature_dtype=torch.float32, feature_on_gpu=True, feature_cols=layers[0],
             label_shape=[V], label_on_gpu=True, n_vertices=V, has_edge_prob=False)
    f.update(kw)
    return f


def check(cfg_edit=None, layers=LAYERS, inputs=None, **kw):
    from nts import host
    cfg = host.gcn_config(layers, FANOUT[:len(layers) - 1], BATCH, **kw)
    if cfg_edit:
        cfg_edit(cfg)
    host.ext().check_driver_options(cfg, **facts(layers, **(inputs or {})))


def refusal(cfg_edit=None, **kw):
    with pytest.raises(RuntimeError) as ei:
        check(cfg_edit, **kw)
    return str(ei.value).splitlines()[0]


@pytest.fixture(scope="module")
def build():
    return refusal


# ---- pinned refusals ----
@pytest.mark.parametrize("name,kw", order.SHARED, ids=[n for n, _ in order.SHARED])
def test_root_weight_refusals(name, kw):
    assert refusal(root_weight=True, **kw) == ROOT_REFUSALS[name]


@pytest.mark.parametrize("name,kw", order.SHARED + [("up_degree", dict(up_degree=True))],
                         ids=[n for n, _ in order.SHARED] + ["up_degree"])
def test_max_refusals(name, kw):
    assert refusal(aggregator="max", **kw) == MAX_REFUSALS[name]


@pytest.mark.parametrize("name", list(LN_REFUSALS))
def test_layer_norm_refusals(name):
    kw, layers, text = LN_REFUSALS[name]
    assert refusal(layers=layers, layer_norm=True, **kw) == text


@pytest.mark.parametrize("name", list(F16_REFUSALS))
def test_feature_f16_refusals(name):
    kw, text = F16_REFUSALS[name]
    assert refusal(feature_f16=True, **kw) == text
    assert refusal(feature_f16=True, inputs=dict(feature_dtype=torch.float16), **kw) == text


@pytest.mark.parametrize("name", list(SHARED_REFUSALS))
def test_shared_sampling_refusals(name):
    assert refusal(shared_sampling=True, **{name: True}) == SHARED_REFUSALS[name]


@pytest.mark.parametrize("name", list(EDGE_REFUSALS))
def test_edge_weighted_refusals(name):
    G, kw = EDGE_REFUSALS[name]
    inputs = dict(has_edge_prob=G != "G_plain")
    msg = refusal(edge_weighted=True, inputs=inputs, **kw)
    assert msg.startswith("edge_weighted is not supported with ") and name in msg, msg
    check(inputs=inputs, **kw)  # the same configuration without the option is accepted


def test_weighted_sampling_refusals():
    """tests/test_weighted_sampling_driver.py holds the five texts (no table
    to import): here that each rule refuses under the option's name"""
    def on(cfg):
        cfg.weighted_sampling = True  # (gcn_config refuses two of these itself)
    with_prob = dict(has_edge_prob=True)
    assert refusal(on).startswith("weighted_sampling needs a graph with edge_prob")
    for kw in (dict(rng_mode=1), dict(rng_mode=2), dict(rng_mode=3), dict(pd_cache=True),
               dict(sample_gpu=True, rng_mode=1)):
        assert refusal(on, inputs=with_prob, **kw).startswith("weighted_sampling is not supported with ")
    check(on, inputs=with_prob)
    # an existing option's conflict is reported before the new ones
    assert refusal(on, inputs=with_prob, layer_norm=True, pd_cache=True) == LN_REFUSALS["pd_cache"][2]


def test_input_shape_rules():
    def layers(*l):
        return lambda cfg: setattr(cfg, "layer_size", list(l))
    assert refusal(layers(8)) == "need at least one layer"
    assert refusal(layers(8, 4, 4, 2)) == "fanout per layer"
    table = "feature table must be fp32 [V, layer_size[0]] on the GPU"
    for bad in (dict(feature_cols=7), dict(feature_cols=-1), dict(feature_on_gpu=False),
                dict(feature_dtype=torch.float64)):
        assert refusal(inputs=bad) == table
    assert refusal(inputs=dict(feature_dtype=torch.float16)).startswith(
        "a float16 feature table needs feature_f16")
    # the label rules, as tests/test_multilabel_driver.py matches them
    two_d = dict(label_shape=[V, LAYERS[-1]])
    assert "2-D label tensor [V, C] of 0/1, got 1-D" in refusal(multi_label=True)
    assert "needs multi_label" in refusal(inputs=two_d)
    assert "GAT" in refusal(multi_label=True, gat=True, weight="none", inputs=two_d)
    for bad in (dict(label_shape=[V, 3]), dict(label_shape=[V + 1, 2]),
                dict(two_d, label_on_gpu=False)):
        assert "layer_size.back()" in refusal(multi_label=True, inputs=bad)
    check(multi_label=True, inputs=two_d)


# ---- order ----
def test_earlier_refusals_come_before_the_later_options():
    first = ROOT_REFUSALS["pd_cache"]
    assert refusal(feature_f16=True, root_weight=True, pd_cache=True) == first
    assert refusal(edge_weighted=True, root_weight=True, pd_cache=True,
                   inputs=dict(has_edge_prob=True)) == first
    for name in SHARED_REFUSALS:
        assert refusal(shared_sampling=True, root_weight=True, **{name: True}) == ROOT_REFUSALS[name]
        assert refusal(shared_sampling=True, aggregator="max", **{name: True}) == MAX_REFUSALS[name]
    assert refusal(shared_sampling=True, layer_norm=True, pd_cache=True) == LN_REFUSALS["pd_cache"][2]


def test_root_weight_reads_the_callers_deterministic_backward():
    """sample_gpu makes the driver run every backward over the CSR, but only
    after the rules: they see the value the caller set"""
    kw = dict(root_weight=True, deterministic_backward=False)
    assert refusal(sample_gpu=True, rng_mode=1, **kw) == ROOT_REFUSALS["sample_gpu"]
    assert refusal(**kw) == ROOT_REFUSALS["deterministic_backward"]
    check(sample_gpu=True, rng_mode=1, deterministic_backward=False)


def test_cache_rate_range_is_checked_where_a_feature_cache_is_built():
    assert refusal(feature_f16=True, cache_rate=0.5) == F16_REFUSALS["cache_rate"][1]
    assert refusal(feature_f16=True, cache_rate=1.5) == F16_REFUSALS["cache_rate"][1]
    assert refusal(cache_rate=1.5) == "cache_rate must be in [0, 1]"
    check(cache_rate=1.0)
    # transform_first = 1 takes no feature cache; the half table builds none
    assert refusal(cache_rate=0.5, transform_first=1).startswith("transform_first needs >= 2 layers")
    assert refusal(feature_f16=True, cache_rate=0.5, transform_first=1) == (
        F16_REFUSALS["transform_first"][1])


# ---- accepted configurations ----
ONE_OPTION = {
    "default": {},
    "root_weight": dict(root_weight=True),
    "max": dict(aggregator="max"),
    "gat": dict(gat=True, weight="none"),
    "gat_heads": dict(gat=True, weight="none", gat_heads=[2, 1]),
    "gat_v2": dict(gat=True, weight="none", gat_v2=True),
    "gat_attn_drop": dict(gat=True, weight="none", gat_attn_drop=0.5),
    "gat_feat_drop": dict(gat=True, weight="none", gat_feat_drop=0.5),
    "layer_norm": dict(layer_norm=True),
    "shared_sampling": dict(shared_sampling=True),
    "feature_f16": dict(feature_f16=True),
    "feature_f16-half-table": dict(feature_f16=True, inputs=dict(feature_dtype=torch.float16)),
    "weighted_sampling": dict(weighted_sampling=True, inputs=dict(has_edge_prob=True)),
    "edge_weighted": dict(edge_weighted=True, inputs=dict(has_edge_prob=True)),
    "multi_label": dict(multi_label=True, inputs=dict(label_shape=[V, LAYERS[-1]])),
    "pd_cache": dict(pd_cache=True),
    "cache_rate": dict(cache_rate=0.5),
    "sample_gpu": dict(sample_gpu=True, rng_mode=1),
    "transform_first": dict(transform_first=1),
    "pair_table": dict(pair_table=3),
    "up_degree": dict(up_degree=True),
    "fused_gather-off": dict(fused_gather=False),
    "deterministic_backward-off": dict(deterministic_backward=False),
    "mt": dict(rng_mode=1),
    "mt-div": dict(rng_mode=2),
}


@pytest.mark.parametrize("name", list(ONE_OPTION))
def test_each_option_alone_is_accepted(name):
    check(**ONE_OPTION[name])


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", ROOT / "bench.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _bench_check(bench, monkeypatch, argv):
    """the config bench.py's main() makes from `argv` (its gcn_config call,
    restated) against the facts of its inputs: synthetic fp32 features, int64
    [V] labels, a graph without edge weights"""
    from nts import host, synthetic
    monkeypatch.setattr("sys.argv", ["bench.py", *argv])
    a = bench.parse()
    n, _, F_dim, C, _ = synthetic.SHAPES[a.shape]
    fan = [int(x) for x in a.fanout.split("-")]
    layers = [int(x) for x in a.layers.split("-")] if a.layers else [F_dim, a.hidden, C]
    cfg = host.gcn_config(
        layers, fan, a.batch, learn_rate=0.001, weight_decay=1e-4, drop_rate=0.5,
        rng_mode=bench.RNG_MODES[a.rng], weight=a.weight, fused_gather=not a.no_fused_gather,
        profile=True, pipeline=not a.no_pipeline, hip_gemm=not a.no_hip_gemm,
        transform_first=a.transform_first, early_aggregate=a.early_agg,
        sampler_priority=(-1 if a.training_priority else 0 if a.no_priority else
                          1 if a.sampler_high_priority else 2),
        fuse_activation=not a.no_fuse_act, fuse_loss=not a.no_fuse_loss, sampler_cus=a.sampler_cus,
        sampler_gate=a.sampler_gate, pad_features=not a.no_pad_features, cache_rate=a.cache_rate,
        deterministic_backward=not a.atomic_backward, gat=a.model == "gat", gemm=a.gemm,
        pair_table=a.pair_table, pd_cache=a.pd_cache, pd_rate=a.pd_rate,
        pd_super_batch=a.pd_super_batch)
    host.ext().check_driver_options(cfg, **facts(layers, label_shape=[n], n_vertices=n))


def _bench_argvs():
    """the headline, the overrides of bench.py's secondary children, and the
    `run` lines of scripts/bench_configs.sh, read from the two files"""
    out = {"headline": []}
    for m in re.finditer(r"child_secondary\((\{[^}]*\})", (ROOT / "bench.py").read_text()):
        flags = ast.literal_eval(m.group(1))
        out["secondary" + "".join(f"{k}={v}" for k, v in flags.items())] = [
            str(x) for kv in flags.items() for x in kv]
    script = (ROOT / "scripts" / "bench_configs.sh").read_text()
    common = shlex.split(re.search(r"bench\.py (.*?) \"\$@\"", script).group(1))
    for line in re.findall(r"^run (.*)$", script, flags=re.M):
        tag, *argv = shlex.split(line)
        out[tag] = common + argv
    return out


BENCH_ARGVS = _bench_argvs()
# every flag of bench.py that reaches the config, alone on the headline job
BENCH_FLAGS = ["--no-fused-gather", "--no-pipeline", "--no-hip-gemm", "--early-agg", "--no-priority",
               "--sampler-high-priority", "--training-priority", "--model gat", "--atomic-backward",
               "--cache-rate 0.5", "--pd-cache", "--no-fuse-act", "--sampler-gate 2",
               "--sampler-cus 8", "--no-pad-features", "--no-fuse-loss", "--weight mean",
               "--gemm f32", "--rng mt-div", "--pair-table 3"]


def test_the_bench_sets_were_found():
    assert len(BENCH_ARGVS) == 1 + 3 + 2 and {"c3", "c4"} <= set(BENCH_ARGVS)


@pytest.mark.parametrize("name", list(BENCH_ARGVS))
def test_bench_configurations_are_accepted(bench, monkeypatch, name):
    _bench_check(bench, monkeypatch, BENCH_ARGVS[name])


@pytest.mark.parametrize("flag", BENCH_FLAGS)
def test_each_bench_flag_alone_is_accepted(bench, monkeypatch, flag):
    _bench_check(bench, monkeypatch, flag.split())


# ---- gcn_config and the cfg runner ----
@pytest.mark.parametrize("rule,args,kw", [
    ("check_gat_heads", (LAYERS, False, [2, 1]), dict(gat_heads=[2, 1])),
    ("check_gat_heads", (LAYERS, True, [2]), dict(gat=True, gat_heads=[2])),
    ("check_gat_heads", (LAYERS, True, [0, 1]), dict(gat=True, gat_heads=[0, 1])),
    ("check_gat_heads", (LAYERS, True, [3, 1]), dict(gat=True, gat_heads=[3, 1])),
    ("check_gat_heads", ([8, 4, 7], True, [1, 40]), dict(gat=True, gat_heads=[1, 40])),
    ("check_gat_drop", ("gat_attn_drop", 0.5, False), dict(gat_attn_drop=0.5)),
    ("check_gat_drop", ("gat_feat_drop", 0.5, False), dict(gat_feat_drop=0.5)),
    ("check_gat_drop", ("gat_attn_drop", 1.0, True), dict(gat=True, gat_attn_drop=1.0)),
    ("check_gat_drop", ("gat_feat_drop", float("nan"), True),
     dict(gat=True, gat_feat_drop=float("nan"))),
    ("check_gat_v2", (True, False), dict(gat_v2=True)),
])
def test_gcn_config_raises_the_drivers_text(rule, args, kw):
    from nts import host
    with pytest.raises(RuntimeError) as ei:
        getattr(host.ext(), rule)(*args)
    text = str(ei.value).splitlines()[0]
    assert text.startswith(rule[len("check_"):] if rule != "check_gat_drop" else args[0])
    with pytest.raises(ValueError) as vi:
        host.gcn_config(args[0] if rule == "check_gat_heads" else LAYERS, FANOUT, BATCH, **kw)
    assert str(vi.value) == text

    def edit(cfg):  # field by field past gcn_config: the full pass reports the same line
        cfg.gat = bool(kw.get("gat"))
        for k, v in kw.items():
            setattr(cfg, k, v)
    assert refusal(edit, layers=args[0] if rule == "check_gat_heads" else LAYERS) == text


@pytest.mark.parametrize("edit,text", [
    (lambda t: t.replace("ALGORITHM:GCNSAMPLEALLGPU", "ALGORITHM:GCNSAMPLENOWHERE"),
     "ALGORITHM GCNSAMPLENOWHERE: not supported by this build (supported: "),
    (lambda t: t.replace("ALGORITHM:GCNSAMPLEALLGPU", "ALGORITHM:GCNSAMPLEPDCACHE") + "ROOT_WEIGHT:1\n",
     "ALGORITHM GCNSAMPLEPDCACHE: ROOT_WEIGHT is not supported with GAT, PD-cache or "
     "GCN_SAMPLE_GPU algorithms"),
], ids=["unknown-algorithm", "root_weight-pd_cache"])
def test_run_refuses_the_cfg_before_anything_is_loaded(tmp_path, edit, text):
    """none of the cfg's data files exist beside this copy"""
    from nts import dataloader, run
    assert "ALGORITHM:GCNSAMPLEALLGPU" in CFG.read_text()
    (tmp_path / "job.cfg").write_text(edit(CFG.read_text()))
    with pytest.raises(SystemExit) as ei:
        run.run(tmp_path / "job.cfg", epochs=1, out=lambda s: None)
    assert str(ei.value).startswith(text)
    with pytest.raises(SystemExit) as bi:  # a direct caller of build_driver is refused the same
        run.build_driver(None, dataloader.InputInfo.from_cfg(tmp_path / "job.cfg"), None, None,
                         None, None, None)
    assert str(bi.value) == str(ei.value)
