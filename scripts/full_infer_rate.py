#!/usr/bin/env python3
"""Rate of the full-neighbour layer-wise inference pass (infer_full).

Builds the C2-shaped synthetic graph the way bench.py does (nts.synthetic,
reddit shape) and a 602-128-41 driver, runs one warm-up and three timed
infer_full() passes and prints ONE JSON line:

  per layer   device ms of the aggregation (HIP events around
              nts_hip_spmm_graph_fwd, recorded by the driver under cfg.profile),
              its algorithmic bytes E (4 + 4 F) + 4 V F + 8 V at the width F it
              aggregates (the narrower side of the layer), and bytes / ms as a
              fraction of the HBM peak — the aggregation is HBM-bound;
  whole pass  host clock around infer_full(), which ends in a synchronise;
  for comparison only: the sampled evaluate() over the same test ids.

The neighbour rows are re-read per edge, so E 4 F counts every read; rows that
hit in cache make the achieved figure exceed what HBM itself carried.  Needs a
GPU; there is no CPU fallback.

Usage: python scripts/full_infer_rate.py [--shape reddit] [--scale 1.0] [--out FILE]
"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "sample-based-gnn_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E (bench.py's figure)


def agg_widths(layers):
    """the width each layer's aggregation runs at: its narrower side"""
    return [min(a, b) for a, b in zip(layers[:-1], layers[1:])]


def agg_bytes(V, E, F):
    return E * (4 + 4 * F) + 4 * V * F + 8 * V


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", default="reddit")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--batch", type=int, default=10000)
    ap.add_argument("--fanout", default="25-10")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("full_infer_rate: needs a GPU (no CPU fallback)")
    from nts import host, synthetic
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    E_ = host.ext()
    g, F_dim, C = synthetic.shaped(a.shape, device=dev, scale=a.scale)
    G = E_.FullyRepGraph.from_edges(g.src, g.dst, g.n_vertices)
    V, En = g.n_vertices, g.n_edges
    del g
    feat = synthetic.features(V, F_dim, device=dev)
    labels, masks = synthetic.labels_masks(V, C, device=dev)
    train = torch.nonzero(masks == 0).flatten().to(torch.int32).cpu()
    test = torch.nonzero(masks == 2).flatten().to(torch.int32).cpu()
    layers = [F_dim, a.hidden, C]
    fan = [int(x) for x in a.fanout.split("-")]
    cfg = host.gcn_config(layers, fan, a.batch, drop_rate=0.5, shuffle=False, profile=True)
    drv = E_.GCN_SAMPLE_ALLGPU_impl(G, feat, labels, train, cfg)

    drv.infer_full()  # warm-up: code objects, scratch growth, allocator
    torch.cuda.synchronize()
    pass_ms, agg_ms = [], []
    for _ in range(a.passes):
        t = time.perf_counter()
        drv.infer_full()  # synchronises before it returns
        pass_ms.append((time.perf_counter() - t) * 1e3)
        agg_ms.append(list(drv.full_agg_ms))
    widths = agg_widths(layers)
    per_layer = []
    for l, F in enumerate(widths):
        ms = sorted(p[l] for p in agg_ms)
        b = agg_bytes(V, En, F)
        med = ms[len(ms) // 2]
        per_layer.append({"layer": l, "agg_width": F, "ms": ms, "ms_median": med,
                          "algorithmic_bytes": b, "GBs": b / med / 1e6,
                          "frac_of_hbm_peak": b / med / 1e6 / HBM_PEAK_GBS})
    # the sampled path, for comparison only: the same ids, both calls warmed once
    drv.evaluate(test)
    drv.evaluate_full(test)
    t = time.perf_counter()
    acc_s = drv.evaluate(test)
    sampled_ms = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    acc_f = drv.evaluate_full(test)
    full_eval_ms = (time.perf_counter() - t) * 1e3
    rec = {"what": "full_infer_rate", "shape": a.shape, "scale": a.scale, "V": V, "E": En,
           "layers": layers, "bound": "hbm", "hbm_peak_GBs": HBM_PEAK_GBS, "per_layer": per_layer,
           "pass_ms": sorted(pass_ms), "pass_ms_median": sorted(pass_ms)[len(pass_ms) // 2],
           "agg_share_of_pass": sum(p["ms_median"] for p in per_layer) /
           sorted(pass_ms)[len(pass_ms) // 2],
           "n_test": int(test.numel()), "evaluate_full_ms": full_eval_ms, "evaluate_full_acc": acc_f,
           "sampled_evaluate_ms": sampled_ms, "sampled_evaluate_acc": acc_s,
           "sampled_fanout": fan, "sampled_batch": a.batch}
    line = json.dumps(rec)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
