"""`nts <cfg>`: run a training job from a reference configuration file.

Mirrors the reference's entry point (toolkits/main.cpp:59-186): read the cfg
(InputInfo::readFromCfgFile, core/GraphSegment.cpp:222-347), load the graph
and the vertex data, pick the driver by ALGORITHM, and run EPOCHS epochs of
train + eval + test with the reference's per-epoch report
(toolkits/GCN_SAMPLE_ALLGPU.hpp:361-383, 467-482).  Every ALGORITHM runs on
the MI355X path of this build; the mapping is:

  GCNSAMPLESINGLE  (GCN_CPU_SAMPLE)   GCN, the reference's mt19937 neighbour
                                      stream and bias-corrected Adam
                                      (learnC2C_with_decay_Adam), on the GPU
  GCNSAMPLEGPU / GCNSAMPLEALLGPU      GCN, Philox sampler, GPU Adam
  GSSAMPLEALLGPU                      the same pipeline with Mean weights
                                      (SURVEY B-5: the reference GPU toolkit
                                      actually runs Sum; MEAN_WEIGHT:gpu selects
                                      its get_mean_weight formula)
  GCNSAMPLEALLMULTI                   data parallel: launch one process per GPU
                                      with torch.distributed.run
  GCNSAMPLEPDCACHE / GSSAMPLEPDCACHE  GCN / GraphSAGE with the NeutronOrch PD
                                      cache: super-batches of PIPELINE_NUM
                                      batches, CACHE_RATE hot vertices each
                                      (preSample; PRE_SAMPLE_FILE read, or
                                      written when missing); with
                                      FEATURE_CACHE_RATE the feature table
                                      moves to pinned host memory with that
                                      fraction cached in HBM
  GATSAMPLEALLGPU                     GAT

MULTI_LABEL:1 (GCN / GraphSAGE algorithms): the label file holds
`id b_0 ... b_{C-1}` (C = the last layer's width), training minimises the mean
sigmoid binary cross-entropy, and the report lines are `Train F1:`, `Eval F1:`,
`Test F1:` (micro-F1 of logits > 0; `Full Eval F1:` / `Full Test F1:` under
FULL_INFERENCE:1) instead of the accuracies.

LAYER_NORM:1 (GCN / GraphSAGE algorithms without PD cache): every hidden layer
is dropout(relu(LayerNorm(.))) in one fused pass, with a gamma and a beta per
hidden layer that are trained without weight decay.

SAMPLE_SHARED:1 (Philox-sampled algorithms without PD cache): neighbour
selection with one random variate per source vertex, shared by every
destination of a hop (fixed-size layer-neighbour sampling): each destination's
set keeps its distribution, the hop's frontier shrinks.  SEED:n sets the
driver's seed (default 2000).

EDGE_WEIGHT_FILE:path / SAMPLE_WEIGHTED:1 (Philox-sampled algorithms without PD
cache, not with SAMPLE_SHARED): the file holds one little-endian fp32 per edge
of EDGE_FILE (finite, in [2^-60, 2^60]); a destination with more neighbours
than its fanout then keeps FANOUT of them with probability proportional to
these weights (successive sampling without replacement).  SAMPLE_WEIGHTED
alone chooses the neighbours only; the aggregation's coefficients do not change.

EDGE_WEIGHT_FILE:path / EDGE_WEIGHT_AGG:1 (Philox-sampled GCN / GraphSAGE
algorithms without PD cache; not with ROOT_WEIGHT, AGGREGATOR:max or UP_DEGREE):
the edge weights are aggregation coefficients: every layer computes
Y[d] = sum_e c(e) a_e X[src(e)], c the algorithm's weight and a_e the edge's
value, in sampled training, evaluation and FULL_INFERENCE.  With or without
SAMPLE_WEIGHTED and SAMPLE_SHARED.

GAT_ATTN_DROP:0.6 / GAT_FEAT_DROP:0.6 (GAT algorithms): dropout of the attention
coefficients and of every layer's input while training, fused into the GAT
kernels.  DROP_RATE is not read by a GAT job (as in the reference).

BATCH_NORM:1 (GCN / GraphSAGE algorithms without PD cache; not with
LAYER_NORM): every hidden layer is dropout(relu(BatchNorm1d(.))) with the
statistics of the batch's rows while training and the running statistics
(momentum 0.1) in the evaluation passes and under FULL_INFERENCE; a gamma and a
beta per hidden layer are trained without weight decay.

ALGORITHM:LINKPREDSAMPLE (no reference counterpart): link
prediction with L GCN layers (sum aggregator, Philox sampler; SAMPLE_SHARED:1
is taken).  LAYERS' last width is the embedding; a batch is BATCH_SIZE edges of
EDGE_FILE plus NEG_PER_POS:k (default 1) uniform negatives per edge; the loss
is the sigmoid BCE of the pairs' dot products.  VAL_EDGE_RATE:r (default 0.1) of
the edge list, chosen by SEED, is held out of the training pairs and scored
after every epoch (`Epoch e: Loss: .. Val MRR: ..`, each positive ranked
against its own negatives).  The held-out edges are NOT removed from the
message-passing graph unless LP_HOLDOUT_REMOVE:1: the graph is
then built without them and without their reverses where EDGE_FILE has them.
LP_EXCLUDE:self|reverse gives every sampled edge of a batch's blocks that is
one of the batch's own positive edges (reverse: turned round as well) the
coefficient 0, after selection, in training and in the validation passes;
LP_FILTER_NEG:1 draws a negative that is a self pair or a graph edge again, up
to 16 times.  LP_FULL_EVAL:1 adds, after the last epoch, `Full Val
MRR: .. Hits@10: ..`: every held-out edge ranked against all VERTICES tails on
full-neighbour embeddings (no sampling, no negatives drawn); LP_FULL_FILTER:1
drops a head's own neighbours from its candidates.  LABEL_FILE and MASK_FILE
are not used.

SUBGRAPH:1 (Philox-sampled GCN / GraphSAGE algorithms without PD cache; DESIGN
§8w): subgraph-sampled training.  A batch is one vertex set — its BATCH_SIZE
seeds and SUBGRAPH_WALK:n (default 0) random-walk steps over in-neighbours from
each — and every layer runs on the subgraph the set induces; the loss rows are
the seeds.  FANOUT must be -1 for every layer.  SUBGRAPH_EDGE_CAP:n bounds the
edges of a block (default min(E, 4 |S|max ceil(E / V))); a block above it stops
the job with the capacity error.  UP_DEGREE:1 gives the subgraph-degree
normalisation of Cluster-GCN / GraphSAINT; ROOT_WEIGHT:1 is taken.  Not with
AGGREGATOR:max, SAMPLE_SHARED, SAMPLE_WEIGHTED, EDGE_WEIGHT_AGG, LAYER_NORM,
BATCH_NORM, MULTI_LABEL or FEATURE_F16.

Usage:  python -m nts.run path/to/job.cfg [--epochs N] [--device D] [--json out.json]
File paths inside the cfg are resolved relative to the cfg's directory.
"""
from __future__ import annotations

import argparse
import json
import os
import pathlib
import sys
import time

import numpy as np
import torch

from . import dataloader

ALGORITHMS = {
    # name: (model, weight, rng, bias_correction, feature placement)
    "GCNSAMPLESINGLE": ("gcn", "sum", "mt", True, None),
    # GCN_SAMPLE_GPU: sample_fast's mt19937 stream (replayed on the device) ->
    # SingleGPUSampleGraphOp (CSR backward), GPU Adam (toolkits/GCN_SAMPLE_GPU.hpp:289-394)
    "GCNSAMPLEGPU": ("gcn", "sum", "mt", False, "sample_gpu"),
    "GCNSAMPLEALLGPU": ("gcn", "sum", "philox", False, None),
    "GSSAMPLEALLGPU": ("gcn", "mean", "philox", False, None),
    "GCNSAMPLEALLMULTI": ("gcn", "sum", "philox", False, None),
    "GCNSAMPLEPDCACHE": ("gcn", "sum", "philox", False, "pd"),
    "GSSAMPLEPDCACHE": ("gcn", "mean", "philox", False, "pd"),
    "GATSAMPLEALLGPU": ("gat", "none", "philox", False, None),
}


LINK_PRED = "LINKPREDSAMPLE"  # its own runner (run_link_pred); not a row of the table above


def _path(base: pathlib.Path, p: str) -> pathlib.Path:
    q = pathlib.Path(p)
    return q if q.is_absolute() else (base / q)


def load_inputs(info: dataloader.InputInfo, base: pathlib.Path, n_classes: int, device=None):
    """Edge list (binary u32 pairs; with `device`, streamed in chunks straight
    into int32 device tensors), features/labels/masks (text or
    FEATURE_FILE:random)."""
    if device is None:
        src, dst = dataloader.read_edge_file(_path(base, info.edge_file))
    else:
        src, dst = dataloader.load_edges_to_device(_path(base, info.edge_file), device)
    V = info.vertices
    F = info.layers[0]
    if info.feature_file in ("", "random"):
        feats, labels, masks = dataloader.random_generate(V, F, n_classes)
        if info.multi_label:
            labels = np.random.default_rng(1).integers(0, 2, (V, n_classes)).astype(np.uint8)
    else:
        fpath = _path(base, info.feature_file)
        if not fpath.exists() and pathlib.Path(str(fpath) + ".zip").exists():
            fpath = pathlib.Path(str(fpath) + ".zip")
        feats, labels, masks = dataloader.read_feature_label_mask(
            fpath, _path(base, info.label_file), _path(base, info.mask_file), V, F)
        if info.multi_label:  # (the lock-step reader kept column 1 only)
            labels = dataloader.read_multilabel_file(_path(base, info.label_file), V, n_classes)
    return src, dst, feats, labels, masks


def refuse_cfg(info: dataloader.InputInfo):
    """Every refusal the cfg alone decides (the driver's rules in cfg terms),
    before anything is loaded: SystemExit with the text of the first row that
    holds.  A new key's rows go at the end."""
    model, _, rng, _, place = ALGORITHMS.get(info.algorithm.upper(), (None,) * 5)
    gat, gcn, pd, mt = model == "gat", model == "gcn", place == "pd", rng == "mt"
    agg, weighted = bool(info.edge_weight_agg), bool(info.sample_weighted)
    sub = bool(info.subgraph)
    rows = (
        (model is None,
         f"not supported by this build (supported: {', '.join(sorted(ALGORITHMS))})"),
        (agg and not info.edge_weight_file,
         "EDGE_WEIGHT_AGG is not supported without an EDGE_WEIGHT_FILE (one fp32 weight per edge)"),
        (agg and gat,
         "EDGE_WEIGHT_AGG is not supported with GAT algorithms (attention layers use no edge "
         "weights)"),
        (agg and info.aggregator == "max",
         "EDGE_WEIGHT_AGG is not supported with AGGREGATOR:max (it uses no edge weights)"),
        (agg and info.root_weight, "EDGE_WEIGHT_AGG is not supported with ROOT_WEIGHT:1"),
        (agg and pd, "EDGE_WEIGHT_AGG is not supported with the PD-cache algorithms"),
        (agg and place == "sample_gpu",
         "EDGE_WEIGHT_AGG is not supported with GCNSAMPLEGPU (the reference's mt19937 stream)"),
        (agg and mt,
         "EDGE_WEIGHT_AGG is not supported with the mt19937-stream algorithms (Philox-sampled "
         "algorithms only)"),
        (agg and info.up_degree, "EDGE_WEIGHT_AGG is not supported with UP_DEGREE:1"),
        (info.multi_label and gat,
         "MULTI_LABEL is not supported with GAT (GCN / GraphSAGE algorithms only)"),
        (info.root_weight and (gat or place is not None),
         "ROOT_WEIGHT is not supported with GAT, PD-cache or GCN_SAMPLE_GPU algorithms"),
        (info.gat_heads and gcn,
         "GAT_HEADS is not supported with GCN / GraphSAGE algorithms (GAT only)"),
        (info.gat_v2 and gcn, "GAT_V2 is not supported with GCN / GraphSAGE algorithms (GAT only)"),
        (info.gat_v2 and info.full_inference,
         "FULL_INFERENCE is not supported with GAT_V2 (full-neighbour inference for GATv2 is not "
         "built)"),
        (info.gat_attn_drop and gcn,
         "GAT_ATTN_DROP is not supported with GCN / GraphSAGE algorithms (GAT only; they read "
         "DROP_RATE)"),
        (info.gat_feat_drop and gcn,
         "GAT_FEAT_DROP is not supported with GCN / GraphSAGE algorithms (GAT only; they read "
         "DROP_RATE)"),
        (info.aggregator == "max" and (gat or place is not None),
         "AGGREGATOR:max is not supported with GAT, PD-cache or GCN_SAMPLE_GPU algorithms"),
        (info.layer_norm and (gat or pd),
         "LAYER_NORM is not supported with GAT or PD-cache algorithms (GCN / GraphSAGE layers "
         "only)"),
        (info.sample_shared and (mt or pd),
         "SAMPLE_SHARED is not supported with the mt19937-stream or PD-cache algorithms "
         "(Philox-sampled algorithms only)"),
        (info.feature_f16 and (gat or pd),
         "FEATURE_F16 is not supported with GAT or PD-cache algorithms (the sum aggregation of "
         "GCN / GraphSAGE only)"),
        (weighted and not info.edge_weight_file,
         "SAMPLE_WEIGHTED is not supported without an EDGE_WEIGHT_FILE (one fp32 weight per edge)"),
        (weighted and (mt or pd),
         "SAMPLE_WEIGHTED is not supported with the mt19937-stream or PD-cache algorithms "
         "(Philox-sampled algorithms only)"),
        (weighted and info.sample_shared,
         "SAMPLE_WEIGHTED is not supported with SAMPLE_SHARED:1 (one selection rule per job)"),
        (info.batch_norm and (gat or pd),
         "BATCH_NORM is not supported with GAT or PD-cache algorithms (GCN / GraphSAGE layers "
         "only)"),
        (info.batch_norm and info.layer_norm,
         "BATCH_NORM is not supported with LAYER_NORM:1 (one normalisation per hidden layer)"),
        (bool(info.lp_full_eval),
         f"LP_FULL_EVAL is not supported outside ALGORITHM:{LINK_PRED} (FULL_INFERENCE:1 is the "
         "node classifiers' exact pass)"),
        (bool(info.lp_full_filter),
         f"LP_FULL_FILTER is not supported outside ALGORITHM:{LINK_PRED}"),
        (sub and any(f != -1 for f in info.fanout),
         "SUBGRAPH needs FANOUT -1 for every layer (all induced neighbours)"),
        (sub and not 0 <= info.subgraph_walk <= 64,
         f"SUBGRAPH_WALK must be in [0, 64], got {info.subgraph_walk}"),
        (sub and info.subgraph_edge_cap < 0,
         f"SUBGRAPH_EDGE_CAP must be >= 0, got {info.subgraph_edge_cap}"),
        (sub and gat, "SUBGRAPH is not supported with GAT algorithms (GCN / GraphSAGE layers only)"),
        (sub and info.aggregator == "max", "SUBGRAPH is not supported with AGGREGATOR:max"),
        (sub and pd, "SUBGRAPH is not supported with the PD-cache algorithms"),
        (sub and place == "sample_gpu",
         "SUBGRAPH is not supported with GCNSAMPLEGPU (the reference's mt19937 stream)"),
        (sub and mt,
         "SUBGRAPH is not supported with the mt19937-stream algorithms (Philox-sampled "
         "algorithms only)"),
        (sub and bool(info.sample_shared), "SUBGRAPH is not supported with SAMPLE_SHARED:1"),
        (sub and weighted, "SUBGRAPH is not supported with SAMPLE_WEIGHTED:1"),
        (sub and agg, "SUBGRAPH is not supported with EDGE_WEIGHT_AGG:1"),
        (sub and bool(info.layer_norm), "SUBGRAPH is not supported with LAYER_NORM:1"),
        (sub and bool(info.batch_norm), "SUBGRAPH is not supported with BATCH_NORM:1"),
        (sub and bool(info.multi_label), "SUBGRAPH is not supported with MULTI_LABEL:1"),
        (sub and bool(info.feature_f16), "SUBGRAPH is not supported with FEATURE_F16:1"),
        (not sub and bool(info.subgraph_walk or info.subgraph_edge_cap),
         "SUBGRAPH_WALK / SUBGRAPH_EDGE_CAP are not supported without SUBGRAPH:1"),
    )
    for hit, text in rows:
        if hit:
            raise SystemExit(f"ALGORITHM {info.algorithm}: {text}")


def build_driver(E, info: dataloader.InputInfo, G, feat, labels, train_ids, device, comm=None):
    from . import host, _abi
    refuse_cfg(info)  # (run() has already; a direct caller has not)
    model, weight, rng, bias, place = ALGORITHMS[info.algorithm.upper()]
    if weight == "mean" and info.extra.get("MEAN_WEIGHT", "").lower() == "gpu":
        weight = "mean-sampled"
    cache_rate = -1.0
    pd = place == "pd"
    if pd and "FEATURE_CACHE_RATE" in info.extra:
        cache_rate = float(info.extra["FEATURE_CACHE_RATE"])
    cfg = host.gcn_config(
        info.layers, info.fanout, info.batch_size, learn_rate=info.learn_rate,
        weight_decay=info.weight_decay, drop_rate=info.drop_rate,
        rng_mode=_abi.NTS_RNG_MT19937_LEMIRE if rng == "mt" else _abi.NTS_RNG_PHILOX,
        weight="none" if model == "gat" else weight, bias_correction=bias,
        pipeline=info.pipeline_num > 1, up_degree=info.up_degree, gat=model == "gat",
        cache_rate=cache_rate, shuffle=True, pd_cache=pd, pd_rate=info.cache_rate,
        pd_super_batch=max(info.pipeline_num, 1), sample_gpu=place == "sample_gpu",
        multi_label=bool(info.multi_label), root_weight=bool(info.root_weight),
        aggregator=info.aggregator, gat_heads=info.gat_heads or None,
        layer_norm=bool(info.layer_norm), gat_attn_drop=info.gat_attn_drop,
        gat_feat_drop=info.gat_feat_drop, gat_v2=bool(info.gat_v2),
        shared_sampling=bool(info.sample_shared), feature_f16=bool(info.feature_f16),
        weighted_sampling=bool(info.sample_weighted),
        edge_weighted=bool(info.edge_weight_agg), seed=info.seed,
        batch_norm=bool(info.batch_norm), subgraph=bool(info.subgraph),
        subgraph_walk=info.subgraph_walk, subgraph_edge_cap=info.subgraph_edge_cap)
    return E.GCN_SAMPLE_ALLGPU_impl(G, feat, labels, train_ids, cfg, comm)


def refuse_link_pred_cfg(info: dataloader.InputInfo):
    """what the cfg alone decides for ALGORITHM:LINKPREDSAMPLE, before anything is loaded"""
    rows = (
        (info.neg_per_pos < 1, f"NEG_PER_POS must be >= 1, got {info.neg_per_pos}"),
        (not 0.0 <= info.val_edge_rate < 1.0,
         f"VAL_EDGE_RATE must be in [0, 1), got {info.val_edge_rate}"),
        (info.lp_exclude not in ("none", "self", "reverse"),
         f"LP_EXCLUDE must be none, self or reverse, got {info.lp_exclude}"),
        (len(info.layers) < 2 or len(info.fanout) != len(info.layers) - 1,
         "LAYERS needs at least one layer and FANOUT one entry per layer"),
        (bool(info.multi_label or info.root_weight or info.layer_norm or info.batch_norm
              or info.feature_f16 or info.gat_heads or info.gat_v2 or info.full_inference
              or info.aggregator != "sum" or info.sample_weighted or info.edge_weight_agg),
         "takes GCN layers with the sum aggregator only (of the model keys, SAMPLE_SHARED alone)"),
        (int(os.environ.get("WORLD_SIZE", "1")) > 1, "is not data parallel (one process)"),
        (bool(info.lp_full_filter) and not info.lp_full_eval,
         "LP_FULL_FILTER needs LP_FULL_EVAL:1 (it filters the full evaluation's candidates)"),
    )
    for hit, text in rows:
        if hit:
            raise SystemExit(f"ALGORITHM {info.algorithm}: {text}")


def split_edges(n_edges: int, rate: float, seed: int):
    """(train, validation) positions of the edge list: a permutation by `seed`,
    its first floor(rate * n) positions held out"""
    perm = np.random.default_rng(seed).permutation(n_edges)
    n_val = int(rate * n_edges)
    return np.sort(perm[n_val:]), np.sort(perm[:n_val])


def message_passing_edges(src: np.ndarray, dst: np.ndarray, val_pos: np.ndarray) -> np.ndarray:
    """LP_HOLDOUT_REMOVE: the positions of the edge list that stay in the
    message-passing graph, ascending.  Position p leaves when (src[p], dst[p])
    is a held-out edge (s, d) (`val_pos`, and every other copy of it in the
    list) or the reverse (d, s) of one; every other edge stays, with its
    multiplicity."""
    s, d = np.asarray(src).astype(np.uint64), np.asarray(dst).astype(np.uint64)
    key = (s << np.uint64(32)) | d
    gone = np.concatenate([key[val_pos], (d[val_pos] << np.uint64(32)) | s[val_pos]])
    return np.flatnonzero(~np.isin(key, gone))


def run_link_pred(info: dataloader.InputInfo, base: pathlib.Path, epochs=None, device=0,
                  out=print) -> dict:
    from . import host
    refuse_link_pred_cfg(info)  # before anything is loaded
    epochs = info.epochs if epochs is None else epochs
    torch.cuda.set_device(device)
    dev = torch.device("cuda", device)
    E = host.ext()
    t0 = time.time()
    src, dst, feats, _, _ = load_inputs(info, base, info.layers[-1], device=dev)
    feat = torch.from_numpy(feats).to(dev)
    edges = torch.stack([src.cpu().to(torch.int64), dst.cpu().to(torch.int64)])
    tr, va = split_edges(edges.shape[1], info.val_edge_rate, info.seed)
    train_edges, val_edges = edges[:, torch.from_numpy(tr)], edges[:, torch.from_numpy(va)]
    if info.lp_holdout_remove:
        keep = torch.from_numpy(message_passing_edges(edges[0].numpy(), edges[1].numpy(), va)).to(dev)
        G = E.FullyRepGraph.from_edges(src[keep].contiguous(), dst[keep].contiguous(), info.vertices)
    else:
        G = E.FullyRepGraph.from_edges(src, dst, info.vertices)  # every edge: held-out ones too
    cfg = host.gcn_config(info.layers, info.fanout, info.batch_size, learn_rate=info.learn_rate,
                          weight_decay=info.weight_decay, drop_rate=info.drop_rate,
                          shared_sampling=bool(info.sample_shared), pipeline=False, shuffle=True,
                          seed=info.seed, neg_per_pos=info.neg_per_pos,
                          lp_exclude=info.lp_exclude, filter_negatives=bool(info.lp_filter_neg))
    drv = host.link_predictor(G, feat, train_edges, cfg)
    kept = "kept in the message-passing graph"
    if info.lp_holdout_remove:
        kept = (f"removed from the message-passing graph with their reverses: "
                f"{int(keep.numel())} of {edges.shape[1]} edges carry messages")
    out(f"link prediction: {train_edges.shape[1]} training edges, {val_edges.shape[1]} held out "
        f"({kept}), {info.neg_per_pos} negative(s) per positive; "
        f"loaded in {time.time() - t0:.2f}s")
    if info.lp_exclude != "none" or info.lp_filter_neg:
        out(f"link prediction: target-edge exclusion {info.lp_exclude}, filtered negatives "
            f"{'on' if info.lp_filter_neg else 'off'}")
    res = {"algorithm": info.algorithm, "n_train_edges": int(train_edges.shape[1]),
           "n_val_edges": int(val_edges.shape[1]), "epochs": []}
    if val_edges.shape[1]:
        res["val_mrr_init"] = drv.evaluate(val_edges)
        out(f"Before training: Val MRR: {res['val_mrr_init']:.6f}")
    for e in range(epochs):
        drv.restart()
        t1 = time.time()
        loss = drv.run_epoch()
        row = {"epoch": e, "loss": float(loss), "seconds": time.time() - t1}
        line = f"Epoch {e}: Loss: {loss:.6f}"
        if val_edges.shape[1]:
            row["val_mrr"] = drv.evaluate(val_edges)
            line += f" Val MRR: {row['val_mrr']:.6f}"
        out(line)
        res["epochs"].append(row)
    if info.lp_full_eval and val_edges.shape[1]:
        # LP_FULL_EVAL:1 — the reportable score of the final weights: every
        # held-out edge ranked against all V tails on full-neighbour embeddings
        # (no sampling, no negatives drawn: the same numbers for every run)
        full = drv.evaluate_full(val_edges, filtered=bool(info.lp_full_filter))
        res["full_val"] = full
        out(f"Full Val MRR: {full['mrr']:.6f} Hits@10: {full['hits@10']:.6f} "
            f"({full['n']} edges against {info.vertices} candidates"
            f"{', filtered' if info.lp_full_filter else ''})")
    res["driver"] = drv
    return res


def pd_presample_file(drv, info, base, out=print, rank=0, world=1):
    """PRE_SAMPLE_FILE (core/ntsBaseOp.hpp:427-497): read the hot vertices of
    every super-batch if the file exists, else keep the device preSample the
    driver ran and write it (default name when the key is unset).  Under
    WORLD_SIZE > 1 each rank has its own train shard and so its own file
    (`.rank<r>` appended): no two ranks write one path."""
    name = info.pre_sample_file or dataloader.presample_file_name(
        _path(base, info.edge_file), info.batch_size, info.fanout_string, info.pipeline_num)
    path = _path(base, name)
    if world > 1:
        path = path.with_name(path.name + f".rank{rank}")
    counts, ids = drv.presample()
    if path.exists():
        kc, kids = dataloader.read_presample_file(path, len(counts))
        drv.set_presample(kc.tolist(), kids.tolist())
        out(f"pre sample file: {path} (read, {len(kc)} super-batches, {kids.size} hot vertices)")
    else:
        try:
            dataloader.write_presample_file(path, counts, ids)
            out(f"pre sample file: {path} (written, {len(counts)} super-batches, {len(ids)} hot vertices)")
        except OSError:
            out(f"pre sample file: {path} not writable; using the device preSample")


def run(cfg_path, epochs=None, device=0, out=print) -> dict:
    from . import host
    from . import dist as ndist
    cfg_path = pathlib.Path(cfg_path)
    info = dataloader.InputInfo.from_cfg(cfg_path)
    if info.algorithm.upper() == LINK_PRED:  # its own task and report
        return run_link_pred(info, cfg_path.parent, epochs, device, out)
    refuse_cfg(info)  # before anything is loaded
    base = cfg_path.parent
    n_classes = info.layers[-1]
    epochs = info.epochs if epochs is None else epochs
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=torch.device("cuda", device))
    torch.cuda.set_device(device)
    dev = torch.device("cuda", device)
    E = host.ext()
    t0 = time.time()
    src, dst, feats, labels, masks = load_inputs(info, base, n_classes, device=dev)
    n_edges = src.numel()
    edge_w = None
    if info.edge_weight_file:  # value i belongs to edge i of the edge file
        edge_w = dataloader.load_edge_weights_to_device(_path(base, info.edge_weight_file),
                                                        n_edges, dev)
    G = E.FullyRepGraph.from_edges(src, dst, info.vertices, edge_w)
    del edge_w
    del src, dst
    if info.feature_f16:  # rounded on the host: the fp32 table never reaches the device
        feats = feats.astype(np.float16)
    feat = torch.from_numpy(feats).to(dev)
    lab =torch.from_numpy(labels).to(dev)
    ids = {k: np.nonzero(masks == v)[0].astype(np.int32) for k, v in
           (("train", dataloader.MASK_TRAIN), ("val", dataloader.MASK_VAL),
            ("test", dataloader.MASK_TEST))}
    train = torch.from_numpy(ndist.shard_nids(ids["train"], world, rank))
    comm = ndist.make_communicator(E, world, rank, device)
    drv = build_driver(E, info, G, feat, lab, train, dev, comm)
    if ALGORITHMS.get(info.algorithm.upper(), ("",) * 5)[4] == "pd":
        pd_presample_file(drv, info, base, out if rank == 0 else (lambda s: None), rank, world)
    if rank == 0:
        out(f"GNNmini::Engine[MI355X.GPU.{info.algorithm}] running [{epochs}] Epochs "
            f"(V={info.vertices}, E={n_edges}, layers {info.layer_string}, fanout "
            f"{info.fanout_string}, batch {info.batch_size}; loaded in {time.time() - t0:.1f}s)")
    hist = []
    for ep in range(epochs):
        te = time.perf_counter()
        drv.reset_correct()
        drv.run_epoch()
        if info.multi_label:
            tp, fp, fn = drv.f1_counts()  # synchronises
        else:
            correct = drv.train_correct()  # synchronises
        loss = float(drv.loss.detach().cpu())
        t_train = time.perf_counter() - te
        acc_val = drv.evaluate(torch.from_numpy(ids["val"])) if ids["val"].size else 0.0
        acc_test = drv.evaluate(torch.from_numpy(ids["test"])) if ids["test"].size else 0.0
        n_train = int(train.numel())
        if info.multi_label:  # evaluate() returned micro-F1s
            f1 = 2.0 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0
            rec = {"epoch": ep, "train_f1": f1, "train_tp": int(tp), "train_fp": int(fp),
                   "train_fn": int(fn), "n_train": n_train, "eval_f1": acc_val, "test_f1": acc_test,
                   "loss": loss, "epoch_time_s": time.perf_counter() - te, "train_time_s": t_train}
        else:
            rec = {"epoch": ep, "train_acc": correct / max(n_train, 1), "train_correct": int(correct),
                   "n_train": n_train, "eval_acc": acc_val, "test_acc": acc_test, "loss": loss,
                   "epoch_time_s": time.perf_counter() - te, "train_time_s": t_train}
        hist.append(rec)
        if rank == 0 and info.multi_label:
            out(f"Train F1: {f1:f} {tp} {fp} {fn}")
            out(f"Eval F1: {acc_val:f} {ids['val'].size}")
            out(f"Test F1: {acc_test:f} {ids['test'].size}")
        elif rank == 0:
            out(f"Train Acc: {rec['train_acc']:f} {correct} {n_train}")
            out(f"Eval Acc: {acc_val:f} {int(round(acc_val * ids['val'].size))} {ids['val'].size}")
            out(f"Test Acc: {acc_test:f} {int(round(acc_test * ids['test'].size))} {ids['test'].size}")
        if rank == 0:
            out(f"GNNmini::Running.Epoch[{ep}]:Times[{rec['epoch_time_s']:f}(s)]:loss\t{loss:f}")
    res = {"cfg": str(cfg_path), "algorithm": info.algorithm, "epochs": hist}
    if info.full_inference:
        # FULL_INFERENCE:1 — the exact score of the final weights: every vertex
        # with its whole neighbourhood, layer by layer over the whole graph
        # (no sampling: the same numbers for every RNG mode and every run)
        # (a GAT job: the fused attention pass over the whole graph)
        full = drv.evaluate_full_gat if info.algorithm == "GATSAMPLEALLGPU" else drv.evaluate_full
        for key, name in (("val", "Eval"), ("test", "Test")):
            n = int(ids[key].size)
            acc = full(torch.from_numpy(ids[key])) if n else 0.0
            if info.multi_label:
                res[f"full_{name.lower()}_f1"] = acc
                if rank == 0:
                    out(f"Full {name} F1: {acc:f} {n}")
                continue
            res[f"full_{name.lower()}_acc"] = acc
            if rank == 0:
                out(f"Full {name} Acc: {acc:f} {int(round(acc * n))} {n}")
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    return res


def main(argv=None):
    p = argparse.ArgumentParser(prog="nts", description=__doc__.split("\n")[0])
    p.add_argument("cfg")
    p.add_argument("--epochs", type=int, default=None)
    p.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    p.add_argument("--json", default=None)
    a = p.parse_args(argv)
    res = run(a.cfg, a.epochs, a.device)
    if a.json:
        pathlib.Path(a.json).write_text(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
