#!/usr/bin/env python3
"""What subgraph-sampled training (SUBGRAPH:1) costs, one JSON line.

On a synthetic graph of nts.synthetic.shaped (default: the Reddit-shaped one of
the flagship workload, C2; batch 10,000, layers F-128-C):

  walk            nts_hip_random_walk alone from one batch's seeds, per walk
                  length: device time (HIP events) and steps/s;
  induced         nts_hip_induced_layer alone on the walk-2 set S of that
                  batch: the rectangular block (seeds x S) and the square one
                  (S x S), with their sizes, the longest destination row (the
                  hub: rows are not split, one wave walks each) and the device
                  time of the whole call (SUM weights, CSR built);
  steps           wall ms per training step of the driver with the option
                  (fanout -1) against the neighbour-sampled driver (fanout
                  25-10) in the same process, rounds interleaved, with |S|,
                  the induced edge counts and the edge capacity the blocks had
                  and needed.

Every timing: a warm-up, then `--repeats` rounds; all rounds are listed beside
their median.  Reported, not gated.  Needs a GPU.

Usage: python scripts/subgraph_rate.py [--shape reddit] [--out profiles/subgraph_rate.json]
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


def med(xs):
    return sorted(xs)[len(xs) // 2]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", default="reddit")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=10000)
    ap.add_argument("--walk", type=int, default=2)
    ap.add_argument("--fanout", default="25-10")
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("subgraph_rate: needs a GPU (no CPU fallback)")
    from nts import host, synthetic
    from nts.hip import DeviceGraph, HipContext, LayerBuffers
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

    def timed(fn):
        us = []
        for rnd in range(a.repeats + 2):  # two warm-up rounds
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rnd >= 2:
                us.append(e0.elapsed_time(e1) * 1e3)
        return us

    # ---- the walk alone ------------------------------------------------------
    hip = HipContext(0, seed=2000)
    dg = DeviceGraph(V, En, G.column_offset, G.row_indices, G.in_degree, G.out_degree)
    seeds = train[:a.batch].to(dev)
    n = int(seeds.numel())
    n_dev = torch.tensor([n], dtype=torch.int32, device=dev)
    walk = []
    for wl in sorted({1, 2, 4, a.walk}):
        out = torch.empty(n * (wl + 1), dtype=torch.int32, device=dev)
        us = timed(lambda: hip.random_walk(dg, seeds, n_dev, wl, 0, out))
        walk.append({"walk_len": wl, "roots": n, "us": us, "us_median": med(us),
                     "steps_per_s": n * wl / (med(us) * 1e-6)})

    # ---- the induced layer alone --------------------------------------------
    ids = torch.empty(n * (a.walk + 1), dtype=torch.int32, device=dev)
    hip.random_walk(dg, seeds, n_dev, a.walk, 0, ids)
    ids_n = torch.tensor([ids.numel()], dtype=torch.int32, device=dev)
    S = torch.unique(ids.to(torch.int64)).to(torch.int32)
    deg = G.column_offset[1:] - G.column_offset[:-1]
    mean_deg = -(-En // V)
    e_cap = min(En, ids.numel() * 4 * mean_deg)
    hip.reserve(V, max(e_cap, V))
    induced = {}
    for name, dst in (("rectangular", seeds), ("square", S)):
        vsz = torch.tensor([dst.numel()], dtype=torch.int32, device=dev)
        lay = LayerBuffers(int(dst.numel()), e_cap, int(ids.numel()), dst, vsz, dev)
        us = timed(lambda: hip.induced_layer(dg, lay, ids, ids_n, 0))
        v, e, s, ovf = lay.sizes_host()
        assert ovf == 0, "the default edge capacity fell short"
        induced[name] = {"destinations": v, "edges": e, "sources": s, "e_cap": e_cap,
                         "longest_destination_row": int(deg[dst.long()].max()),
                         "graph_edges_of_the_destinations": int(deg[dst.long()].sum()),
                         "us": us, "us_median": med(us)}
        del lay

    # ---- training steps ------------------------------------------------------
    kinds = {"neighbour": dict(fanout=fan), "subgraph": dict(fanout=[-1] * len(fan), subgraph=True,
                                                              subgraph_walk=a.walk)}
    drv = {}
    for k, kw in kinds.items():
        kw = dict(kw)
        cfg = host.gcn_config(layers, kw.pop("fanout"), a.batch, learn_rate=0.001, weight_decay=1e-4,
                              drop_rate=0.5, **kw)
        drv[k] = E.GCN_SAMPLE_ALLGPU_impl(G, feat, labels, train, cfg)

    def run(d, k):
        for _ in range(k):
            if not d.sample_not_finished():
                d.restart()
            d.train_batch()
        d.synchronize()

    ms = {k: [] for k in drv}
    for d in drv.values():
        run(d, 5)
    for _ in range(a.repeats):
        for k, d in drv.items():
            t0 = time.perf_counter()
            run(d, a.steps)
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    steps = {}
    for k, d in drv.items():
        steps[k] = {"ms_per_step": ms[k], "ms_per_step_median": med(ms[k]),
                    "transform_first": bool(d.transform_first),
                    "last_batch": [{"v": int(l["v_size"]), "src": int(l["src_size"]),
                                    "e": int(l["e_size"])} for l in d.last_layers]}
    steps["subgraph"]["e_cap"] = e_cap
    steps["subgraph"]["e_cap_needed"] = max(l["e"] for l in steps["subgraph"]["last_batch"])
    steps["subgraph_over_neighbour"] = (steps["subgraph"]["ms_per_step_median"] /
                                        steps["neighbour"]["ms_per_step_median"])

    out = {"what": "subgraph_rate", "device": torch.cuda.get_device_name(0), "shape": a.shape,
           "scale": a.scale, "V": V, "E": En, "layers": layers, "batch": a.batch,
           "walk_len": a.walk, "neighbour_fanout": fan, "repeats": a.repeats,
           "steps_per_round": a.steps, "walk": walk, "induced": induced, "steps": steps}
    line = json.dumps(out)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
