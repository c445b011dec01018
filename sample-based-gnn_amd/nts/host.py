"""Python access to the C++ host layer (nts/host/*.cpp, built in-tree).

`ext()` loads nts/lib/host_build/nts_host_ext.so — it raises when the build is
missing; nothing here falls back to a CPU implementation.
"""
from __future__ import annotations

import importlib.machinery
import importlib.util
import pathlib

import torch  # noqa: F401  (torch's HIP runtime first)

from . import _abi

_HERE = pathlib.Path(__file__).resolve().parent
EXT_PATH = _HERE / "lib" / "host_build" / "nts_host_ext.so"
_ext = None


def ext():
    global _ext
    if _ext is None:
        if not EXT_PATH.exists():
            raise ImportError(f"{EXT_PATH} missing: run __graft_entry__.build()")
        _abi.lib()  # libnts_hip.so first (RTLD_GLOBAL)
        loader = importlib.machinery.ExtensionFileLoader("nts_host_ext", str(EXT_PATH))
        spec = importlib.util.spec_from_loader("nts_host_ext", loader)
        mod = importlib.util.module_from_spec(spec)
        loader.exec_module(mod)
        _ext = mod
    return _ext


def _checked(rule, *args, **kwargs):
    """one of the driver's own rules (nts/host/options.cpp) at the time the
    config is made: its text, as a ValueError"""
    try:
        rule(*args, **kwargs)
    except RuntimeError as e:
        raise ValueError(str(e).splitlines()[0]) from None


LP_EXCLUDE = {"none": 0, "self": 1, "reverse": 2}  # GCNConfig.lp_exclude (cfg key LP_EXCLUDE)


def gcn_config(layers, fanout, batch_size, learn_rate=0.01, weight_decay=1e-4, drop_rate=0.5,
               rng_mode=_abi.NTS_RNG_PHILOX, weight="sum", fused_gather=True,
               bias_correction=False, deterministic_backward=True, shuffle=True, profile=False,
               seed=2000, hip_gemm=True, pipeline=True, transform_first=-1,
               early_aggregate=True, sampler_priority=2, fuse_activation=True,
               fuse_loss=True, sampler_cus=0, sampler_gate=0, pad_features=True, cache_rate=-1.0,
               up_degree=False, gat=False, pd_cache=False, pd_rate=0.2, pd_super_batch=4,
               gemm="split3", overlap_allreduce=-1, pair_table=0, sample_gpu=False,
               multi_label=False, root_weight=False, aggregator="sum", epsilon=1e-9,
               gat_heads=None, layer_norm=False, layer_norm_eps=1e-5, gat_attn_drop=0.0,
               gat_feat_drop=0.0, gat_v2=False, shared_sampling=False, feature_f16=False,
               weighted_sampling=False, edge_weighted=False, batch_norm=False,
               batch_norm_eps=1e-5, batch_norm_momentum=0.1, neg_per_pos=1, lp_exclude="none",
               filter_negatives=False, subgraph=False, subgraph_walk=0, subgraph_edge_cap=0):
    if weighted_sampling:  # neighbours drawn in proportion to the graph's edge_prob
        if int(rng_mode) in (_abi.NTS_RNG_MT19937_LEMIRE, _abi.NTS_RNG_MT19937_DIV):
            raise ValueError("weighted_sampling is not supported with an MT19937 rng_mode (it "
                             "draws from a Philox stream of its own)")
        if shared_sampling or int(rng_mode) == _abi.NTS_RNG_PHILOX_SHARED:
            raise ValueError("weighted_sampling is not supported with shared_sampling "
                             "(rng_mode NTS_RNG_PHILOX_SHARED)")
    if shared_sampling:  # one variate per source vertex
        if int(rng_mode) in (_abi.NTS_RNG_MT19937_LEMIRE, _abi.NTS_RNG_MT19937_DIV):
            raise ValueError("shared_sampling is not supported with an MT19937 rng_mode (it "
                             "draws from a Philox stream of its own)")
        rng_mode = _abi.NTS_RNG_PHILOX_SHARED
    if aggregator not in ("sum", "max"):
        raise ValueError(f"aggregator must be 'sum' or 'max', got {aggregator!r}")
    E = ext()
    gat_heads = [int(k) for k in gat_heads or ()]  # empty: single-head
    _checked(E.check_gat_heads, list(layers), bool(gat), gat_heads)
    gat_drop = {"gat_attn_drop": float(gat_attn_drop), "gat_feat_drop": float(gat_feat_drop)}
    for name, rate in gat_drop.items():
        _checked(E.check_gat_drop, name, rate, bool(gat))
    _checked(E.check_gat_v2, bool(gat_v2), bool(gat))
    c = E.GCNConfig()
    c.layer_size = list(layers)
    c.fanout = list(fanout)
    c.batch_size = int(batch_size)
    c.learn_rate = float(learn_rate)
    c.weight_decay = float(weight_decay)
    c.epsilon = float(epsilon)  # Adam's; 1.0 makes the first step read the gradient out (tests)
    c.drop_rate = float(drop_rate)
    c.rng_mode = int(rng_mode)
    c.sample_gpu = bool(sample_gpu)
    c.weight_type = {"sum": E.WeightType.Sum, "mean": E.WeightType.Mean,
                     "mean-sampled": E.WeightType.MeanSampled,
                     "none": getattr(E.WeightType, "None")}[weight]
    c.fused_gather = bool(fused_gather)
    c.bias_correction = bool(bias_correction)
    c.deterministic_backward = bool(deterministic_backward)
    c.hip_gemm = bool(hip_gemm)
    c.pipeline = bool(pipeline)
    c.transform_first = int(transform_first)
    c.gemm_mode = {"f32": _abi.NTS_GEMM_F32, "split3": _abi.NTS_GEMM_SPLIT3}[gemm]
    c.overlap_allreduce = int(overlap_allreduce)
    c.pair_table = int(pair_table)
    c.early_aggregate = bool(early_aggregate)
    c.sampler_priority = int(sampler_priority)
    c.fuse_activation = bool(fuse_activation)
    c.fuse_loss = bool(fuse_loss)
    c.multi_label = bool(multi_label)
    c.root_weight = bool(root_weight)
    c.aggregator = {"sum": 0, "max": 1}[aggregator]
    c.layer_norm = bool(layer_norm)
    c.layer_norm_eps = float(layer_norm_eps)
    c.sampler_cus = int(sampler_cus)
    c.sampler_gate = int(sampler_gate)
    c.pad_features = bool(pad_features)
    c.cache_rate = float(cache_rate)
    c.up_degree = bool(up_degree)
    c.gat = bool(gat)
    c.gat_heads = gat_heads
    c.gat_attn_drop = gat_drop["gat_attn_drop"]  # GAT's own dropouts (drop_rate is not read
    c.gat_feat_drop = gat_drop["gat_feat_drop"]  # by a GAT driver)
    if gat_v2:  # GATv2 scores; the default leaves the field as constructed
        c.gat_v2 = True
    if feature_f16:  # f16 feature table; the default leaves the field as constructed
        c.feature_f16 = True
    if weighted_sampling:  # (the default leaves the field as constructed)
        c.weighted_sampling = True
    if edge_weighted:  # edge_prob as aggregation coefficients; refusals: the driver
        c.edge_weighted = True
    if batch_norm:  # BatchNorm on the hidden layers; refusals: the driver
        c.batch_norm = True
    c.batch_norm_eps = float(batch_norm_eps)
    c.batch_norm_momentum = float(batch_norm_momentum)
    c.pd_cache = bool(pd_cache)
    c.pd_rate = float(pd_rate)
    c.pd_super_batch = int(pd_super_batch)
    c.shuffle = bool(shuffle)
    c.profile = bool(profile)
    c.seed = int(seed)
    c.neg_per_pos = int(neg_per_pos)  # LinkPredictor only; no other driver reads it
    if lp_exclude not in LP_EXCLUDE:
        raise ValueError(f"lp_exclude must be 'none', 'self' or 'reverse', got {lp_exclude!r}")
    if LP_EXCLUDE[lp_exclude]:  # target-edge exclusion; LinkPredictor only
        c.lp_exclude = LP_EXCLUDE[lp_exclude]
    if filter_negatives:  # (the defaults leave both fields as constructed)
        c.lp_filter_neg = True
    if subgraph:  # subgraph-sampled training; refusals: the driver.  Off: the
        c.subgraph = True  # three fields stay as constructed
        c.subgraph_walk = int(subgraph_walk)
        c.subgraph_edge_cap = int(subgraph_edge_cap)
    return c


def link_predictor(graph, feature, train_edges, cfg):
    """A LinkPredictor: `feature` fp32 [V, layers[0]] on the GPU,
    `train_edges` int64 [2, n] on the host, `cfg` from gcn_config(...,
    neg_per_pos=K).  Its option rules (check_link_pred_options) run before
    anything is built; their text comes back as a ValueError."""
    E = ext()
    train_edges = torch.as_tensor(train_edges)
    _checked(E.check_link_pred_options, cfg, **dict(
        feature_dtype=feature.dtype, feature_on_gpu=feature.is_cuda,
        feature_cols=feature.shape[1] if feature.dim() == 2 else -1,
        edge_shape=list(train_edges.shape), edges_on_host=not train_edges.is_cuda,
        n_vertices=int(graph.global_vertices), has_edge_prob=graph.edge_prob is not None))
    return E.LinkPredictor(graph, feature, train_edges.to(torch.int64), cfg)
