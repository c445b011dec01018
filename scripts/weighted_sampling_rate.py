#!/usr/bin/env python3
"""What edge-weighted neighbour selection (weighted_sampling)
costs, one JSON line.

On a synthetic graph of nts.synthetic.shaped (default: the Reddit-shaped one of
the flagship workload; batch 10,000, fanout 25-10, layers F-128-C) with the
weights 1 / sqrt(deg_in(dst) deg_out(src)), the default PHILOX sampler against
PHILOX_SHARED (k_select_shared: the same one-wave radix select, the fair
yardstick) and the weighted selection (k_select_weighted):

  sampler_alone   E.sampler_throughput: edges/s and ms per batch;
  hops            per hop on the same destinations for every variant (hop 0:
                  the batch's seeds; hop 1: the PHILOX hop-0 frontier): edges,
                  unique sources, and the device time of the whole layer call
                  (HIP events).  On the same destinations the variants differ
                  in the select kernel and, through the frontier's size, in the
                  passes behind it, so the difference of two call times is the
                  select kernels' difference up to the latter;
  steps           wall ms per training step of the driver (default order).

Every timing: a warm-up, then `--repeats` rounds with the variants interleaved;
all rounds are listed beside their median and (max - min) / median.  Reported,
not gated.  Needs a GPU.

Usage: python scripts/weighted_sampling_rate.py [--shape reddit] [--out profiles/weighted_sampling_rate.json]
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

# name: (rng_mode, weighted)
VARIANTS = {"philox": (0, False), "shared": (3, False), "weighted": (0, True)}


def med(xs):
    return sorted(xs)[len(xs) // 2]


def spread(xs):
    return (max(xs) - min(xs)) / med(xs)


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
        raise SystemExit("weighted_sampling_rate: needs a GPU (no CPU fallback)")
    from nts import host, synthetic
    from nts.hip import DeviceGraph, HipContext, LayerBuffers, layer_caps
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

    # ---- the sampler alone ---------------------------------------------------
    alone = {k: [] for k in VARIANTS}
    for k, (m, wtd) in VARIANTS.items():
        E.sampler_throughput(G, train, a.batch, fan, rng_mode=m, n_batches=4, weighted=wtd)
    for _ in range(a.repeats):
        for k, (m, wtd) in VARIANTS.items():
            r = E.sampler_throughput(G, train, a.batch, fan, rng_mode=m,
                                     n_batches=a.sampler_batches, weighted=wtd)
            alone[k].append({"edges_per_s": r["edges"] / r["seconds"],
                             "ms_per_batch": r["seconds"] * 1e3 / r["batches"],
                             "edges_per_batch": r["edges"] / r["batches"]})
    sampler_alone = {k: {"rounds": v, "edges_per_s_median": med([x["edges_per_s"] for x in v]),
                         "ms_per_batch_median": med([x["ms_per_batch"] for x in v]),
                         "ms_per_batch_spread": spread([x["ms_per_batch"] for x in v])}
                     for k, v in alone.items()}

    # ---- per hop, every variant on the same destinations -----------------------
    hip = HipContext(0, seed=2000)
    dg = DeviceGraph(V, En, G.column_offset, G.row_indices, G.in_degree, G.out_degree)
    seeds = train[:a.batch].to(dev)
    caps = layer_caps(int(seeds.numel()), fan, V, En)
    hip.reserve(V, max(max(c) for c in caps))
    vsz0 = torch.tensor([seeds.numel()], dtype=torch.int32, device=dev)
    base = LayerBuffers(*caps[0], seeds, vsz0, dev)  # the PHILOX hop-0 frontier: hop 1's destinations
    hip.sample_layer(dg, base, fan[0], 0, 0, 0, 0)
    torch.cuda.synchronize()
    bufs = {k: [LayerBuffers(*caps[0], seeds, vsz0, dev),
                LayerBuffers(*caps[1], base.source, base.sizes[2:3], dev)] for k in VARIANTS}
    hop_us = {k: [[] for _ in fan] for k in VARIANTS}
    for rnd in range(a.repeats + 2):  # two warm-up rounds
        for k, (m, wtd) in VARIANTS.items():
            for l, (f, lay) in enumerate(zip(fan, bufs[k])):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                hip.sample_layer(dg, lay, f, l, 0, m, 0, edge_prob=G.edge_prob if wtd else None)
                e1.record()
                e1.synchronize()
                if rnd >= 2:
                    hop_us[k][l].append(e0.elapsed_time(e1) * 1e3)
    hops = {}
    for k in VARIANTS:
        hops[k] = []
        for l, lay in enumerate(bufs[k]):
            v, e, s, ovf = lay.sizes_host()
            assert ovf == 0
            hops[k].append({"hop": l, "fanout": fan[l], "destinations": v, "edges": e,
                            "unique_sources": s, "layer_call_us": hop_us[k][l],
                            "layer_call_us_median": med(hop_us[k][l]),
                            "layer_call_us_spread": spread(hop_us[k][l])})
    del bufs, base

    # ---- training steps ------------------------------------------------------
    drv = {}
    for k, (m, wtd) in VARIANTS.items():
        cfg = host.gcn_config(layers, fan, a.batch, learn_rate=0.001, weight_decay=1e-4,
                              drop_rate=0.5, shared_sampling=k == "shared", weighted_sampling=wtd)
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
    steps = {k: {"ms_per_step": ms[k], "ms_per_step_median": med(ms[k]),
                 "ms_per_step_spread": spread(ms[k]),
                 "last_batch": [{"v": int(l["v_size"]), "src": int(l["src_size"]),
                                 "e": int(l["e_size"])} for l in d.last_layers]}
             for k, d in drv.items()}
    ratios = {
        "sampler_ms_weighted_over_shared": sampler_alone["weighted"]["ms_per_batch_median"] /
        sampler_alone["shared"]["ms_per_batch_median"],
        "sampler_ms_weighted_over_philox": sampler_alone["weighted"]["ms_per_batch_median"] /
        sampler_alone["philox"]["ms_per_batch_median"],
        "step_ms_weighted_over_shared": steps["weighted"]["ms_per_step_median"] /
        steps["shared"]["ms_per_step_median"],
        "step_ms_weighted_over_philox": steps["weighted"]["ms_per_step_median"] /
        steps["philox"]["ms_per_step_median"],
    }
    for l in range(len(fan)):
        ratios[f"hop{l}_call_weighted_over_shared"] = (hops["weighted"][l]["layer_call_us_median"] /
                                                      hops["shared"][l]["layer_call_us_median"])
        ratios[f"hop{l}_call_weighted_over_philox"] = (hops["weighted"][l]["layer_call_us_median"] /
                                                      hops["philox"][l]["layer_call_us_median"])

    out = {"what": "weighted_sampling_rate", "device": torch.cuda.get_device_name(0),
           "shape": a.shape, "scale": a.scale, "V": V, "E": En, "layers": layers, "fanout": fan,
           "batch": a.batch, "repeats": a.repeats, "steps_per_round": a.steps,
           "weights": "1/sqrt(deg_in(dst) * deg_out(src))",
           "sampler_alone": sampler_alone, "hops": hops, "steps": steps, "ratios": ratios}
    line = json.dumps(out)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
