#!/usr/bin/env python3
"""Times of the link-prediction batch builder, loss and step.

B = 10,000 positive edges of a Reddit-shaped synthetic graph (nts/synthetic.py),
K = 1 negative per positive (P = 20,000 pairs), D = 128.  One JSON line with

  lp_batch   nts_hip_lp_batch: pairs, the distinct endpoints, the incidence CSR;
  fused      nts_hip_lp_bce_train on that batch's pairs and an N(0, 1/sqrt(D))
             embedding: scores, loss, the MRR counter and the gathered dH;
  libtorch   the chain on the same inputs: index_select x2, mul().sum(1),
             binary_cross_entropy_with_logits and autograd's backward
             (index_add_ into dH);
  driver     ms per LinkPredictor.train_batch() (host wall time over a pass; the
             call reads the loss back, so it includes one synchronisation);
  bytes      the loss kernels' compulsory traffic: the forward reads two rows
             per pair, the backward one row per incidence slot and writes one
             row per endpoint, plus the index arrays.

Each device figure is the time between two HIP events around `--iters`
back-to-back calls on one stream, divided by the iterations; `--repeats` such
measurements after a warm-up, all listed, the median reported.  Needs a GPU.

Usage: python scripts/link_pred_rate.py [--B 10000] [--K 1] [--D 128] [--out FILE]
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


def timed(fn, iters, repeats):
    import torch
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)  # us per call
    return sorted(out)


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
        raise SystemExit("link_pred_rate: needs a GPU (no CPU fallback)")
    from nts import host, synthetic
    from nts.hip import HipContext
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    E = host.ext()
    hip = HipContext(0)
    g, F_in, _ = synthetic.shaped("reddit", device=dev, scale=a.scale)
    V, B, K, D = g.n_vertices, a.B, a.K, a.D
    P = B * (1 + K)
    gen = torch.Generator(device=dev).manual_seed(1)
    pick = torch.randperm(g.n_edges, device=dev, generator=gen)[:B]
    ps, pd = g.src[pick].contiguous(), g.dst[pick].contiguous()
    i32 = dict(dtype=torch.int32, device=dev)
    dest, vsz = torch.empty(2 * P, **i32), torch.zeros(1, **i32)
    pu, pv = torch.empty(P, **i32), torch.empty(P, **i32)
    off, slot = torch.empty(2 * P + 1, **i32), torch.empty(2 * P, **i32)
    hip.reserve(V, 8 * P)

    def batch():
        hip.lp_batch(ps, pd, K, V, 3, dest, vsz, pu, pv, off, slot)

    b_us = timed(batch, a.iters, a.repeats)
    v = int(vsz.item())
    H = torch.randn(v, D, device=dev, generator=gen) / D ** 0.25
    score, loss = torch.empty(P, device=dev), torch.empty((), device=dev)
    dH, mrr = torch.empty(v, D, device=dev), torch.zeros(2, device=dev)
    off_v = off[:v + 1]

    def fused():
        hip.lp_bce_train(H, D, pu, pv, B, K, off_v, slot, vsz, score, loss, dH, mrr)

    Hg = H.clone().requires_grad_()
    ul, vl = pu.long(), pv.long()
    y = torch.zeros(P, device=dev)
    y[:B] = 1

    def chain():
        s = (Hg.index_select(0, ul) * Hg.index_select(0, vl)).sum(1)
        l = torch.nn.functional.binary_cross_entropy_with_logits(s, y)
        Hg.grad = None
        l.backward()
        return l

    f_us = timed(fused, a.iters, a.repeats)
    c_us = timed(chain, a.iters, a.repeats)
    ref = chain()
    fused()
    torch.cuda.synchronize()
    deg = (off_v[1:] - off_v[:-1]).long()
    row = 4 * D
    bytes_fwd = 2 * P * row + 2 * P * 4 + P * 4
    bytes_bwd = 2 * P * row + v * row + 2 * P * (4 + 4 + 4) + (v + 1) * 4

    # the driver: one pass over min(n_edges, 20 B) training edges
    n_tr = min(g.n_edges, 20 * B)
    edges = torch.stack([g.src[:n_tr].cpu().long(), g.dst[:n_tr].cpu().long()])
    G = E.FullyRepGraph.from_edges(g.src, g.dst, V)
    feat = synthetic.features(V, F_in, device=dev)
    cfg = host.gcn_config([F_in, 128, D], [10, 5], B, pipeline=False, neg_per_pos=K)
    drv = host.link_predictor(G, feat, edges, cfg)
    drv.train_batch()
    drv.train_batch()
    drv.synchronize()
    t0, steps = time.perf_counter(), 0
    while drv.sample_not_finished():
        drv.train_batch()
        steps += 1
    drv.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3 / max(steps, 1)
    lb = drv.last_batch()

    med = lambda x: x[len(x) // 2]
    rec = {"what": "link_pred_rate", "graph": "reddit-shaped", "V": V, "B": B, "K": K, "P": P, "D": D,
           "endpoints": v, "max_row_slots": int(deg.max()), "iters": a.iters, "repeats": a.repeats,
           "clock": "hip events around back-to-back calls",
           "lp_batch_us": b_us, "lp_batch_us_median": med(b_us),
           "fused_train_us": f_us, "fused_train_us_median": med(f_us),
           "libtorch_us": c_us, "libtorch_us_median": med(c_us),
           "speedup": med(c_us) / med(f_us),
           "bytes_fwd": bytes_fwd, "bytes_bwd": bytes_bwd,
           "fused_GBps_of_bound": (bytes_fwd + bytes_bwd) / (med(f_us) * 1e-6) / 1e9,
           "loss_fused": float(loss), "loss_libtorch": float(ref.detach()),
           "max_abs_dH_diff": float((dH - Hg.grad).abs().max()),
           "driver": {"layers": [F_in, 128, D], "fanout": [10, 5], "steps": steps,
                      "ms_per_step_host_wall": step_ms, "endpoints_last": lb["v_size"],
                      "edges_last": [l["e_size"] for l in lb["layers"]]}}
    line = json.dumps(rec)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
