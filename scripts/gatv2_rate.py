#!/usr/bin/env python3
"""Rate of the GATv2 kernels, one JSON line.

On the sampler's own merged blocks (a GAT driver's trained batch: fanout 10-5,
batch 1024, both hops), for (K, D) = (8, 8) (the [64, 64, 7] driver's hidden
layer) and (4, 64), forward and backward each:

  v2      nts_hip_gatv2_forward / nts_hip_gatv2_backward (Hd given);
  gat     the multi-head GAT kernels on the same block (H = Hs): GATv2 does
          strictly more work (a second gather per slot in the per-source
          backward, a second pass over the rows in the per-destination one);
  chain   the materialised libtorch chain ([e, F] messages; backward by
          autograd), what the fused kernels replace.

Device time between two HIP events around `--iters` back-to-back calls, the
variants interleaved per repeat; every repeat is listed, with the median and the
spread (max - min) / median.  `step_ms` is the wall time per training step of a
[64, 64, 7] driver with gat_heads = [8, 1], gat_v2 on and off.  The figures are
reported, not gated.  Needs a GPU.

Usage: python scripts/gatv2_rate.py [--out profiles/gatv2_rate.json]
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

SHAPES = [(8, 8), (4, 64)]


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
    rec["v2_over_gat"] = med(us["v2"]) / med(us["gat"])
    rec["chain_over_v2"] = med(us["chain"]) / med(us["v2"])
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
        raise SystemExit("gatv2_rate: needs a GPU (no CPU fallback)")
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

    def driver(v2):
        cfg = host.gcn_config([64, 64, 7], [10, 5], 1024, drop_rate=0.0, gat=True,
                              gat_heads=[8, 1], gat_v2=v2)
        return E.GCN_SAMPLE_ALLGPU_impl(G, feat, labels, train, cfg)

    drv = {"gat_v2": driver(True), "gat": driver(False)}
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
    top, bottom = drv["gat"].last_layers
    gen = torch.Generator(device=dev).manual_seed(1)
    for hop, lay in (("bottom", bottom), ("top", top)):
        v, s, e = lay["v_size"], lay["src_size"], lay["e_size"]
        co, ri, dl = lay["column_offset"], lay["row_indices"], lay["dst_local_id"]
        ro, ci, ceid = lay["row_offset"], lay["column_indices"], lay["csr_edge_id"]
        col, rl = co[:v + 1].long(), ri[:e].long()
        d_of_e = torch.repeat_interleave(torch.arange(v, device=dev), col[1:] - col[:-1])
        for K, D in SHAPES:
            F = K * D
            Hs = torch.randn(s, F, device=dev, generator=gen)
            Hd = torch.randn(v, F, device=dev, generator=gen)
            att = torch.randn(F, device=dev, generator=gen) * 0.3
            att2 = torch.randn(2 * F, device=dev, generator=gen) * 0.3
            GY = torch.randn(v, F, device=dev, generator=gen)
            new = lambda *sh: torch.empty(*sh, device=dev)
            u, at, du, Y, GM = new(e * K), new(e * K), new(e * K), new(v, F), new(v, F)
            dHs, dHd, datt = new(s, F), new(v, F), new(F)
            m, ag, dug, ds2, dS = new(e * K), new(e * K), new(e * K), new(s * K), new(s, 2 * K)
            Yg, GMg, dH = new(v, F), new(v, F), new(s, F)

            def chain(hs, hd, av):
                xs = hs[rl]
                t = torch.nn.functional.leaky_relu(xs + hd[d_of_e], 0.2)
                sc = (t * av).view(e, K, D).sum(2)
                mx = torch.full((v, K), -float("inf"), device=dev).scatter_reduce(
                    0, d_of_e[:, None].expand(e, K), sc, "amax")
                ex = torch.exp(sc - mx[d_of_e])
                sm = torch.zeros(v, K, device=dev).index_add(0, d_of_e, ex)
                al = ex / sm[d_of_e]
                z = torch.zeros(v, K, D, device=dev).index_add(0, d_of_e,
                                                               xs.view(e, K, D) * al[:, :, None])
                return torch.relu(z.reshape(v, F))

            leaf = [t.clone().requires_grad_(True) for t in (Hs, Hd, att)]

            def fwd_v2():
                hip.gatv2_forward(co, ri, v, Hs, Hd, K, att, u, at, Y)

            def fwd_gat():
                hip.gat_forward_heads(co, ri, dl, v, Hs, K, att2, m, ag, Yg)

            def fwd_chain():
                with torch.no_grad():
                    chain(Hs, Hd, att)

            def bwd_v2():
                hip.gatv2_backward(co, ri, v, ro, ci, ceid, s, Hs, Hd, K, att, at, Y, GY, du, dHs,
                                   dHd, datt, GM=GM)

            def bwd_gat():
                hip.gat_backward_heads(co, ri, dl, v, ro, ci, ceid, s, Hs, K, att2, ag, m, Yg, GY,
                                       dug, ds2, dH, dS, GM=GMg)

            def fwdbwd_chain():  # autograd needs its forward: forward + backward
                for t in leaf:
                    t.grad = None
                chain(*leaf).backward(GY)

            fwd = interleaved({"v2": fwd_v2, "gat": fwd_gat, "chain": fwd_chain}, a.iters, a.repeats)
            bwd = interleaved({"v2": bwd_v2, "gat": bwd_gat, "chain": fwdbwd_chain}, a.iters,
                              a.repeats)
            torch.cuda.synchronize()
            same = bool(torch.allclose(Y, chain(Hs, Hd, att), rtol=1e-4, atol=1e-5) and
                        torch.allclose(dHs, leaf[0].grad, rtol=1e-3, atol=1e-4) and
                        torch.allclose(datt, leaf[2].grad, rtol=1e-3, atol=1e-3))
            cases.append({"hop": hop, "K": K, "D": D, "v": v, "src": s, "edges": e,
                          "agrees_with_chain": same, "fwd": summary(fwd),
                          "bwd_chain_includes_its_forward": True, "bwd": summary(bwd)})
    rec = {"what": "gatv2_rate", "iters": a.iters, "repeats": a.repeats, "steps": a.steps,
           "fanout": [10, 5], "batch": 1024, "cases": cases, "step_ms": step_ms,
           "step_ms_median": {k: med(x) for k, x in step_ms.items()}}
    line = json.dumps(rec)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
