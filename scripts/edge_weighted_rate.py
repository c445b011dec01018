#!/usr/bin/env python3
"""What edge weights as aggregation coefficients (edge_weighted)
cost, one JSON line.

On a synthetic graph of nts.synthetic.shaped (default: the Reddit-shaped one of
the flagship workload; batch 10,000, fanout 25-10, layers F-128-C) with the
coefficients 1 / sqrt(deg_in(dst) deg_out(src)) (gcn_norm's), the option off
against the option on:

  sampler_alone   E.sampler_throughput: us per batch and edges/s
                  (nts_hip_sample_layer against nts_hip_sample_layer_coef);
  steps           wall ms per training step of the driver (default order);
  infer_full      host ms of the whole pass and the device ms of every layer's
                  aggregation (full_agg_ms: nts_hip_spmm_graph_fwd against
                  nts_hip_spmm_graph_fwd_coef).

Expected added traffic: 4 bytes per sampled edge in the selection plus a
read-modify in the relabel pass, and 4 bytes per graph edge per layer in the
full-graph aggregation.  Every timing: a warm-up, then `--repeats` rounds with
the two variants interleaved; all rounds are listed beside their median and
(max - min) / median.  Reported, not gated.  Needs a GPU.

Usage: python scripts/edge_weighted_rate.py [--shape reddit] [--out profiles/edge_weighted_rate.json]
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

VARIANTS = {"off": False, "on": True}


def med(xs):
    return sorted(xs)[len(xs) // 2]


def spread(xs):
    return (max(xs) - min(xs)) / med(xs)


def summary(xs):
    return {"rounds": xs, "median": med(xs), "spread": spread(xs)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", default="reddit")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=10000)
    ap.add_argument("--fanout", default="25-10")
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sampler-batches", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("edge_weighted_rate: needs a GPU (no CPU fallback)")
    from nts import host, synthetic
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    E = host.ext()
    g, F_dim, C = synthetic.shaped(a.shape, device=dev, scale=a.scale)
    V, En = g.n_vertices, g.n_edges
    ind = torch.bincount(g.dst.long(), minlength=V).clamp_(min=1)
    outd = torch.bincount(g.src.long(), minlength=V).clamp_(min=1)
    w = (ind[g.dst.long()] * outd[g.src.long()]).to(torch.float32).rsqrt_()
    del ind, outd
    G = E.FullyRepGraph.from_edges(g.src, g.dst, V, w)
    del g, w
    feat = synthetic.features(V, F_dim, device=dev)
    labels, masks = synthetic.labels_masks(V, C, device=dev)
    train = torch.nonzero(masks == 0).flatten().to(torch.int32).cpu()
    fan = [int(x) for x in a.fanout.split("-")]
    layers = [F_dim, a.hidden, C]
    csr = [True] * (len(fan) - 1) + [False]

    # ---- the sampler alone ---------------------------------------------------
    us = {k: [] for k in VARIANTS}
    eps = {k: [] for k in VARIANTS}
    for k, on in VARIANTS.items():
        E.sampler_throughput(G, train, a.batch, fan, n_batches=4, csr_layers=csr, coef=on)
    for _ in range(a.repeats):
        for k, on in VARIANTS.items():
            r = E.sampler_throughput(G, train, a.batch, fan, n_batches=a.sampler_batches,
                                     csr_layers=csr, coef=on)
            us[k].append(r["seconds"] * 1e6 / r["batches"])
            eps[k].append(r["edges"] / r["seconds"])
    sampler_alone = {k: {"us_per_batch": summary(us[k]), "edges_per_s_median": med(eps[k])}
                     for k in VARIANTS}

    # ---- training steps, then the full-neighbour pass --------------------------
    drv = {}
    for k, on in VARIANTS.items():
        cfg = host.gcn_config(layers, fan, a.batch, learn_rate=0.001, weight_decay=1e-4,
                              drop_rate=0.5, edge_weighted=on, profile=True)
        drv[k] = E.GCN_SAMPLE_ALLGPU_impl(G, feat, labels, train, cfg)

    def run(d, n):
        for _ in range(n):
            if not d.sample_not_finished():
                d.restart()
            d.train_batch()
        d.synchronize()

    ms = {k: [] for k in VARIANTS}
    for d in drv.values():
        run(d, 5)
    for _ in range(a.repeats):
        for k, d in drv.items():
            t0 = time.perf_counter()
            run(d, a.steps)
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    steps = {k: {"ms_per_step": summary(ms[k])} for k in VARIANTS}

    pass_ms = {k: [] for k in VARIANTS}
    agg_ms = {k: [] for k in VARIANTS}
    for d in drv.values():
        d.infer_full()  # warm-up: code objects, scratch growth, allocator
    for _ in range(a.repeats):
        for k, d in drv.items():
            t0 = time.perf_counter()
            d.infer_full()  # synchronises before it returns
            pass_ms[k].append((time.perf_counter() - t0) * 1e3)
            agg_ms[k].append(list(d.full_agg_ms))
    infer = {k: {"pass_ms": summary(pass_ms[k]),
                 "full_agg_ms": [summary([r[l] for r in agg_ms[k]]) for l in range(len(fan))]}
             for k in VARIANTS}

    ratios = {
        "sampler_us_on_over_off": sampler_alone["on"]["us_per_batch"]["median"] /
        sampler_alone["off"]["us_per_batch"]["median"],
        "step_ms_on_over_off": steps["on"]["ms_per_step"]["median"] /
        steps["off"]["ms_per_step"]["median"],
        "infer_pass_ms_on_over_off": infer["on"]["pass_ms"]["median"] / infer["off"]["pass_ms"]["median"],
        "full_agg_ms_on_over_off": [infer["on"]["full_agg_ms"][l]["median"] /
                                    infer["off"]["full_agg_ms"][l]["median"] for l in range(len(fan))],
    }
    out = {"what": "edge_weighted_rate", "device": torch.cuda.get_device_name(0), "shape": a.shape,
           "scale": a.scale, "V": V, "E": En, "layers": layers, "fanout": fan, "batch": a.batch,
           "repeats": a.repeats, "steps_per_round": a.steps,
           "coefficients": "1/sqrt(deg_in(dst) * deg_out(src))",
           "sampler_alone": sampler_alone, "steps": steps, "infer_full": infer, "ratios": ratios}
    line = json.dumps(out)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
