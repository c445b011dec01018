#!/usr/bin/env python3
"""Rate of the multi-head GAT kernels, one JSON line.

On the sampler's own merged blocks (a GAT driver's trained batch: fanout 10-5,
batch 1024, both hops), for (K, D) = (8, 8), (8, 32), (4, 64), (2, 128):

  heads   one nts_hip_gat_forward_heads / nts_hip_gat_backward_heads call;
  sliced  the yardstick: K calls of the single-head nts_hip_gat_forward /
          nts_hip_gat_backward on the column slices H[:, hD:(h+1)D] (ldh = F),
          each head with buffers of its own.

Device time between two HIP events around `--iters` back-to-back calls, the two
variants interleaved per repeat; every repeat is listed, the median and the
spread (max - min) / median reported, and `faster` is true when the slowest
heads repeat beats the fastest sliced one (faster by more than the spread).
`step_ms` is the wall time per training step of a [64, 64, 7] driver with
gat_heads = [8, 1] and of the single-head one, for the record.  Needs a GPU.

Usage: python scripts/gat_heads_rate.py [--out profiles/gat_heads_rate.json]
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

SHAPES = [(8, 8), (8, 32), (4, 64), (2, 128)]


def med(xs):
    return sorted(xs)[len(xs) // 2]


def interleaved(fns, iters, repeats):
    """us per call of each fn: warm-up, then per repeat every fn in turn"""
    import torch
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                f()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3 / iters)
    return out


def summary(us):
    rec = {"us": us}
    for k, v in us.items():
        rec[f"{k}_us_median"] = med(v)
        rec[f"{k}_spread"] = (max(v) - min(v)) / med(v)
    rec["speedup_median"] = med(us["sliced"]) / med(us["heads"])
    rec["faster"] = max(us["heads"]) < min(us["sliced"])
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gat_heads_rate: needs a GPU (no CPU fallback)")
    from nts import host, synthetic
    from nts.hip import HipContext
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    E = host.ext()
    hip = HipContext(0)
    g = synthetic.chung_lu(100000, 2500000, 25.0, device=dev, seed=3)
    G = E.FullyRepGraph.from_edges(g.src, g.dst, g.n_vertices)
    feat = synthetic.features(g.n_vertices, 64, device=dev)
    labels, masks = synthetic.labels_masks(g.n_vertices, 7, device=dev)
    train = torch.nonzero(masks == 0).flatten().to(torch.int32).cpu()

    def driver(heads):
        cfg = host.gcn_config([64, 64, 7], [10, 5], 1024, drop_rate=0.0, gat=True, gat_heads=heads)
        return E.GCN_SAMPLE_ALLGPU_impl(G, feat, labels, train, cfg)

    drv = {"heads_8_1": driver([8, 1]), "single": driver(None)}
    step_ms = {k: [] for k in drv}
    for d in drv.values():
        for _ in range(5):
            if not d.sample_not_finished():
                d.restart()
            d.train_batch()
        d.synchronize()
    for _ in range(a.repeats):
        for k, d in drv.items():
            t0 = time.perf_counter()
            for _ in range(a.steps):
                if not d.sample_not_finished():
                    d.restart()
                d.train_batch()
            d.synchronize()
            step_ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)

    cases = []
    top, bottom = drv["single"].last_layers
    gen = torch.Generator(device=dev).manual_seed(1)
    for hop, lay in (("bottom", bottom), ("top", top)):
        v, s, e = lay["v_size"], lay["src_size"], lay["e_size"]
        co, ri, dl = lay["column_offset"], lay["row_indices"], lay["dst_local_id"]
        ro, ci, ceid = lay["row_offset"], lay["column_indices"], lay["csr_edge_id"]
        for K, D in SHAPES:
            F = K * D
            H = torch.randn(s, F, device=dev, generator=gen)
            att = torch.randn(2 * F, device=dev, generator=gen) * 0.3
            GY = torch.randn(v, F, device=dev, generator=gen)
            new = lambda *sh: torch.empty(*sh, device=dev)
            m, at, du, ds2, dS = new(e * K), new(e * K), new(e * K), new(s * K), new(s, 2 * K)
            Y, GM, dH = new(v, F), new(v, F), new(s, F)
            # the yardstick's operands: head h's slices of H, Y, GY, GM, dH
            # (pitch F) and its own att [a1_h | a2_h] and per-edge arrays
            sl = [slice(h * D, (h + 1) * D) for h in range(K)]
            att_h = [torch.cat([att[c], att[F + c.start:F + c.stop]]).contiguous() for c in sl]
            mh, ah, duh = ([new(e) for _ in sl] for _ in range(3))
            ds2h, dSh = [new(s) for _ in sl], [new(s, 2) for _ in sl]
            Ys, GMs, dHs = new(v, F), new(v, F), new(s, F)

            def fwd_heads():
                hip.gat_forward_heads(co, ri, dl, v, H, K, att, m, at, Y)

            def fwd_sliced():
                for h, c in enumerate(sl):
                    hip.gat_forward(co, ri, dl, v, H[:, c], att_h[h], mh[h], ah[h], Ys[:, c])

            def bwd_heads():
                hip.gat_backward_heads(co, ri, dl, v, ro, ci, ceid, s, H, K, att, at, m, Y, GY, du,
                                       ds2, dH, dS, GM=GM)

            def bwd_sliced():
                for h, c in enumerate(sl):
                    hip.gat_backward(co, ri, dl, v, ro, ci, ceid, s, H[:, c], att_h[h], ah[h], mh[h],
                                     Ys[:, c], GY[:, c], duh[h], ds2h[h], dHs[:, c], dSh[h],
                                     GM=GMs[:, c])

            fwd = interleaved({"heads": fwd_heads, "sliced": fwd_sliced}, a.iters, a.repeats)
            bwd = interleaved({"heads": bwd_heads, "sliced": bwd_sliced}, a.iters, a.repeats)
            torch.cuda.synchronize()
            same = bool(torch.allclose(Y, Ys, rtol=1e-4, atol=1e-5) and
                        torch.allclose(dH, dHs, rtol=1e-3, atol=1e-4))
            cases.append({"hop": hop, "K": K, "D": D, "v": v, "src": s, "edges": e,
                          "agrees_with_sliced": same, "fwd": summary(fwd), "bwd": summary(bwd)})
    rec = {"what": "gat_heads_rate", "iters": a.iters, "repeats": a.repeats, "steps": a.steps,
           "fanout": [10, 5], "batch": 1024, "cases": cases, "step_ms": step_ms,
           "step_ms_median": {k: med(x) for k, x in step_ms.items()},
           "met": all(c["fwd"]["faster"] and c["bwd"]["faster"] for c in cases)}
    line = json.dumps(rec)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
