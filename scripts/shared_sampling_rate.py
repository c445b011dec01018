#!/usr/bin/env python3
"""What shared-variate neighbour selection (NTS_RNG_PHILOX_SHARED)
costs and gains, one JSON line.

On a synthetic graph of nts.synthetic.shaped (default: the Reddit-shaped one of
the flagship workload; batch 10,000, fanout 25-10, layers F-128-C), PHILOX
against PHILOX_SHARED:

  sampler_alone   E.sampler_throughput: edges/s and ms per batch;
  hops            per hop of one batch on the same seeds: destinations, edges,
                  unique sources, and the device time of the whole
                  nts_hip_sample_layer call (HIP events).  The two modes differ
                  in the select kernel (k_select_shared against
                  k_select_philox / k_select_philox_g16) and in what follows it
                  only through the smaller frontier, so the difference of the
                  call times bounds the select kernels' difference;
  steps           wall ms per training step of the driver in the default
                  bottom-layer order and aggregate-first, with the per-kernel
                  device times of cfg.profile.

Every timing: a warm-up, then `--repeats` rounds with the variants interleaved;
all rounds are listed beside their median.  Reported, not gated.  Needs a GPU.

Usage: python scripts/shared_sampling_rate.py [--shape reddit] [--out profiles/shared_sampling_rate.json]
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

MODES = {"philox": 0, "shared": 3}


def med(xs):
    return sorted(xs)[len(xs) // 2]


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
        raise SystemExit("shared_sampling_rate: needs a GPU (no CPU fallback)")
    from nts import host, synthetic
    from nts.hip import DeviceGraph, HipContext, LayerBuffers, layer_caps
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    E = host.ext()
    g, F_dim, C = synthetic.shaped(a.shape, device=dev, scale=a.scale)
    G = E.FullyRepGraph.from_edges(g.src, g.dst, g.n_vertices)
    V, En = g.n_vertices, g.n_edges
    del g
    feat = synthetic.features(V, F_dim, device=dev)
    labels, masks = synthetic.labels_masks(V, C, device=dev)
    train = torch.nonzero(masks == 0).flatten().to(torch.int32).cpu()
    fan = [int(x) for x in a.fanout.split("-")]
    layers = [F_dim, a.hidden, C]

    # ---- the sampler alone ---------------------------------------------------
    alone = {k: [] for k in MODES}
    for k, m in MODES.items():
        E.sampler_throughput(G, train, a.batch, fan, rng_mode=m, n_batches=4)
    for _ in range(a.repeats):
        for k, m in MODES.items():
            r = E.sampler_throughput(G, train, a.batch, fan, rng_mode=m, n_batches=a.sampler_batches)
            alone[k].append({"edges_per_s": r["edges"] / r["seconds"],
                             "ms_per_batch": r["seconds"] * 1e3 / r["batches"],
                             "edges_per_batch": r["edges"] / r["batches"]})
    sampler_alone = {k: {"rounds": v, "edges_per_s_median": med([x["edges_per_s"] for x in v]),
                         "ms_per_batch_median": med([x["ms_per_batch"] for x in v])}
                     for k, v in alone.items()}

    # ---- per hop: sizes and the layer call's device time ---------------------
    hip = HipContext(0, seed=2000)
    dg = DeviceGraph(V, En, G.column_offset, G.row_indices, G.in_degree, G.out_degree)
    seeds = train[:a.batch].to(dev)
    caps = layer_caps(int(seeds.numel()), fan, V, En)
    hip.reserve(V, max(max(c) for c in caps))
    bufs = {}
    for k in MODES:
        cur, vsz, lays = seeds, torch.tensor([seeds.numel()], dtype=torch.int32, device=dev), []
        for f, (vc, ec, sc) in zip(fan, caps):
            lay = LayerBuffers(vc, ec, sc, cur, vsz, dev)
            lays.append(lay)
            cur, vsz = lay.source, lay.sizes[2:3]
        bufs[k] = lays
    hop_us = {k: [[] for _ in fan] for k in MODES}
    for rnd in range(a.repeats + 2):  # two warm-up rounds
        for k, m in MODES.items():
            for l, (f, lay) in enumerate(zip(fan, bufs[k])):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                hip.sample_layer(dg, lay, f, l, 0, m, 0)
                e1.record()
                e1.synchronize()
                if rnd >= 2:
                    hop_us[k][l].append(e0.elapsed_time(e1) * 1e3)
    hops = {}
    for k in MODES:
        hops[k] = []
        for l, lay in enumerate(bufs[k]):
            v, e, s, ovf = lay.sizes_host()
            assert ovf == 0
            hops[k].append({"hop": l, "fanout": fan[l], "destinations": v, "edges": e,
                            "unique_sources": s, "layer_call_us": hop_us[k][l],
                            "layer_call_us_median": med(hop_us[k][l])})
    del bufs

    # ---- training steps ------------------------------------------------------
    orders = {"default": dict(transform_first=-1), "aggregate_first": dict(transform_first=0)}
    steps = {}
    for oname, okw in orders.items():
        drv = {}
        for k in MODES:
            cfg = host.gcn_config(layers, fan, a.batch, learn_rate=0.001, weight_decay=1e-4,
                                  drop_rate=0.5, profile=True, shared_sampling=k == "shared", **okw)
            drv[k] = E.GCN_SAMPLE_ALLGPU_impl(G, feat, labels, train, cfg)

        def run(d, n):
            for _ in range(n):
                if not d.sample_not_finished():
                    d.restart()
                d.train_batch()
            d.synchronize()

        ms = {k: [] for k in MODES}
        for d in drv.values():
            run(d, 5)
            d.reset_stats()
        for _ in range(a.repeats):
            for k, d in drv.items():
                t0 = time.perf_counter()
                run(d, a.steps)
                ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
        rec = {"transform_first": bool(drv["philox"].transform_first)}
        for k, d in drv.items():
            prof = d.resolve_profile()
            rec[k] = {"ms_per_step": ms[k], "ms_per_step_median": med(ms[k]),
                      "last_batch": [{"v": int(l["v_size"]), "src": int(l["src_size"]),
                                      "e": int(l["e_size"])} for l in d.last_layers],
                      "kernel_us_per_call": {n: p["ms"] * 1e3 / p["calls"]
                                             for n, p in prof.items() if p["calls"]}}
        rec["shared_over_philox"] = rec["shared"]["ms_per_step_median"] / rec["philox"]["ms_per_step_median"]
        steps[oname] = rec
        del drv

    out = {"what": "shared_sampling_rate", "device": torch.cuda.get_device_name(0),
           "shape": a.shape, "scale": a.scale, "V": V, "E": En, "layers": layers, "fanout": fan,
           "batch": a.batch, "repeats": a.repeats, "steps_per_round": a.steps,
           "sampler_alone": sampler_alone, "hops": hops, "steps": steps}
    line = json.dumps(out)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
