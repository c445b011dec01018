#!/usr/bin/env python3
"""Times of target-edge exclusion and filtered negatives.

The shape of scripts/link_pred_rate.py: B = 10,000 positive edges of a
Reddit-shaped synthetic graph, K = 1, D = 128, blocks of fanout 10-5.  One JSON
line with

  exclude_keys   nts_hip_lp_exclude_keys with reverse (2 B keys in);
  mask_block     nts_hip_lp_mask_block on each of the batch's two sampled blocks
                 (hop 0: CSC and CSR; hop 1: CSC only, as the driver builds them);
  lp_batch       nts_hip_lp_batch and nts_hip_lp_batch_filtered on the same
                 positives, and their ratio;
  driver         ms per LinkPredictor.train_batch() with the options off, with
                 lp_exclude = reverse, and with reverse + filtered negatives
                 (host wall time over a pass, the three in turn), and the ratios
                 to the first;
  counts         of one batch: the sampled edges excluded, the negatives redrawn
                 at least once and the negatives left unresolved.

Each device figure is the time between two HIP events around `--iters`
back-to-back calls on one stream, divided by the iterations; `--repeats` such
measurements after a warm-up, all listed, the median reported.  Needs a GPU.

Usage: python scripts/lp_exclude_rate.py [--B 10000] [--K 1] [--D 128] [--out FILE]
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

from link_pred_rate import timed  # noqa: E402  (scripts/ is sys.path[0])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--B", type=int, default=10000)
    ap.add_argument("--K", type=int, default=1)
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--scale", type=float, default=1.0, help="of the Reddit-shaped graph")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lp_exclude_rate: needs a GPU (no CPU fallback)")
    from nts import _abi, host, synthetic
    from nts.hip import DeviceGraph, HipContext, LayerBuffers, layer_caps
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    E = host.ext()
    hip = HipContext(0)
    g, F_in, _ = synthetic.shaped("reddit", device=dev, scale=a.scale)
    V, B, K, D = g.n_vertices, a.B, a.K, a.D
    P = B * (1 + K)
    fan = [10, 5]
    gen = torch.Generator(device=dev).manual_seed(1)
    pick = torch.randperm(g.n_edges, device=dev, generator=gen)[:B]
    ps, pd = g.src[pick].contiguous(), g.dst[pick].contiguous()
    i32 = dict(dtype=torch.int32, device=dev)
    dest, vsz = torch.empty(2 * P, **i32), torch.zeros(1, **i32)
    pu, pv = torch.empty(P, **i32), torch.empty(P, **i32)
    off, slot = torch.empty(2 * P + 1, **i32), torch.empty(2 * P, **i32)
    col, rows = hip.build_csc(g.src, g.dst, V)
    out_d, in_d = hip.degrees(g.src, g.dst, V)
    dg = DeviceGraph(V, g.n_edges, col, rows, in_d, out_d)
    caps = layer_caps(2 * P, fan, V, g.n_edges)
    hip.reserve(V, max(8 * P, max(max(c) for c in caps)))
    # row_indices ascending within each destination (the host layer's torch sort)
    d_of = torch.repeat_interleave(torch.arange(V, device=dev), col[1:] - col[:-1])
    srt = ((d_of << 32) + (rows.long() & 0xFFFFFFFF)).sort().values.bitwise_and(0xFFFFFFFF).to(torch.int32)
    unresolved = torch.zeros(1, **i32)

    def batch():
        hip.lp_batch(ps, pd, K, V, 3, dest, vsz, pu, pv, off, slot)

    def batch_filtered():
        hip.lp_batch_filtered(dg, srt, ps, pd, K, 3, dest, vsz, pu, pv, off, slot, unresolved)

    b_us = timed(batch, a.iters, a.repeats)
    batch()
    tails_plain = dest[pv.long()[B:]].clone()
    bf_us = timed(batch_filtered, a.iters, a.repeats)
    unresolved.zero_()
    batch_filtered()
    redrawn = int((dest[pv.long()[B:]] != tails_plain).sum())
    n_unresolved = int(unresolved.item())

    keys = torch.empty(2 * B, dtype=torch.int64, device=dev)
    n_keys = torch.zeros(1, **i32)

    def exclude_keys():
        hip.lp_exclude_keys(ps, pd, True, V, keys, n_keys)

    k_us = timed(exclude_keys, a.iters, a.repeats)

    # the batch's blocks as the driver builds them: a CSR on every hop but the outermost
    batch()
    cur, cur_n, layers = dest, vsz, []
    for l, (f, (vc, ec, sc)) in enumerate(zip(fan, caps)):
        lay = LayerBuffers(vc, ec, sc, cur, cur_n, dev, csr=l < len(fan) - 1)
        hip.sample_layer(dg, lay, f, l, 3, _abi.NTS_RNG_PHILOX, _abi.NTS_WEIGHT_SUM)
        layers.append(lay)
        cur, cur_n = lay.source, lay.sizes[2:3]
    excluded = torch.zeros(1, **i32)
    m_us, e_live, n_excl = [], [], []
    for lay in layers:
        m_us.append(timed(lambda: hip.lp_mask_block(lay, keys, n_keys, 1, excluded), a.iters, a.repeats))
        excluded.zero_()
        hip.lp_mask_block(lay, keys, n_keys, 1, excluded)
        n_excl.append(int(excluded.item()))
        e_live.append(lay.sizes_host()[1])

    # the driver, three configurations in turn on one graph and one edge order
    n_tr = min(g.n_edges, 20 * B)
    edges = torch.stack([g.src[:n_tr].cpu().long(), g.dst[:n_tr].cpu().long()])
    G = E.FullyRepGraph.from_edges(g.src, g.dst, V)
    feat = synthetic.features(V, F_in, device=dev)
    drivers = {}
    for name, kw in (("off", {}), ("reverse", dict(lp_exclude="reverse")),
                     ("reverse_filtered", dict(lp_exclude="reverse", filter_negatives=True))):
        cfg = host.gcn_config([F_in, 128, D], fan, B, pipeline=False, neg_per_pos=K, **kw)
        drv = host.link_predictor(G, feat, edges, cfg)
        drv.train_batch()
        drv.train_batch()
        drv.synchronize()
        t0, steps = time.perf_counter(), 0
        while drv.sample_not_finished():
            drv.train_batch()
            steps += 1
        drv.synchronize()
        drivers[name] = {"steps": steps, "ms_per_step_host_wall": (time.perf_counter() - t0) * 1e3 / max(steps, 1),
                         "excluded_edges_last": drv.excluded_edges(),
                         "unresolved_negatives_last": drv.unresolved_negatives()}
        del drv
    base = drivers["off"]["ms_per_step_host_wall"]
    for d in drivers.values():
        d["ratio_to_off"] = d["ms_per_step_host_wall"] / base

    med = lambda x: x[len(x) // 2]
    rec = {"what": "lp_exclude_rate", "graph": "reddit-shaped", "V": V, "B": B, "K": K, "P": P, "D": D,
           "fanout": fan, "iters": a.iters, "repeats": a.repeats,
           "clock": "hip events around back-to-back calls",
           "exclude_keys_us": k_us, "exclude_keys_us_median": med(k_us), "n_keys": int(n_keys.item()),
           "mask_block_us": m_us, "mask_block_us_median": [med(x) for x in m_us],
           "mask_block_live_edges": e_live, "mask_block_excluded": n_excl,
           "lp_batch_us": b_us, "lp_batch_us_median": med(b_us),
           "lp_batch_filtered_us": bf_us, "lp_batch_filtered_us_median": med(bf_us),
           "filtered_over_plain": med(bf_us) / med(b_us),
           "negatives_redrawn": redrawn, "negatives_unresolved": n_unresolved,
           "driver": {"layers": [F_in, 128, D], **drivers}}
    line = json.dumps(rec)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
