#!/usr/bin/env python3
"""Rate of the GAT dropout kernels, one JSON line.

On the sampler's own merged blocks (a GAT driver's trained batch: fanout 10-5,
batch 1024, both hops), for (K, D) = (1, 64), (8, 8), (8, 32), forward and
backward at rates (0.6, 0.6):

  drop    one nts_hip_gat_forward[_heads]_drop / nts_hip_gat_backward[_heads]_drop call;
  plain   yardstick 1: the existing no-dropout entry points (reported, not bounded);
  chain   yardstick 2: dropout done outside the kernels in libtorch — the plain
          call for m and a, then a~ = a * mask * scale materialised ([e, K], the
          mask drawn with torch.rand), the [e, K, D] messages H[src] * a~, their
          index_add into Z, relu and torch dropout (forward); the plain backward
          plus the same materialised products for ga and the aggregation term of
          dH (backward).

Device time between two HIP events around `--iters` back-to-back calls, the
variants interleaved per repeat; every repeat is listed, the median and the
spread (max - min) / median reported, and `faster` is true when the slowest
drop repeat beats the fastest chain one (faster by more than the spread).
`step_ms` is the wall time per training step of a [64, 64, 7] driver with the
options on (0.6, 0.6) and off.  No thresholds are fixed in advance.  Needs a GPU.

Usage: python scripts/gat_dropout_rate.py [--out profiles/gat_dropout_rate.json]
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

SHAPES = [(1, 64), (8, 8), (8, 32)]
Q = P = 0.6


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
    rec["over_plain_median"] = med(us["drop"]) / med(us["plain"])
    rec["chain_over_drop_median"] = med(us["chain"]) / med(us["drop"])
    rec["faster"] = max(us["drop"]) < min(us["chain"])
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
        raise SystemExit("gat_dropout_rate: needs a GPU (no CPU fallback)")
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

    def driver(**kw):
        cfg = host.gcn_config([64, 64, 7], [10, 5], 1024, drop_rate=0.0, gat=True, **kw)
        return E.GCN_SAMPLE_ALLGPU_impl(G, feat, labels, train, cfg)

    drv = {"on": driver(gat_attn_drop=Q, gat_feat_drop=P), "off": driver()}
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
    top, bottom = drv["off"].last_layers
    gen = torch.Generator(device=dev).manual_seed(1)
    sa = 1.0 / (1.0 - Q)
    for hop, lay in (("bottom", bottom), ("top", top)):
        v, s, e = lay["v_size"], lay["src_size"], lay["e_size"]
        co, ri, dl = lay["column_offset"], lay["row_indices"], lay["dst_local_id"]
        ro, ci, ceid = lay["row_offset"], lay["column_indices"], lay["csr_edge_id"]
        deg = (co[1:v + 1] - co[:v]).long()
        d_of_e = torch.repeat_interleave(torch.arange(v, device=dev), deg)
        ril = ri[:e].long()
        for K, D in SHAPES:
            F = K * D
            H = torch.randn(s, F, device=dev, generator=gen)
            att = torch.randn(2 * F, device=dev, generator=gen) * 0.3
            GY = torch.randn(v, F, device=dev, generator=gen)
            new = lambda *sh: torch.empty(*sh, device=dev)
            m, at, du, ds2, dS = new(e * K), new(e * K), new(e * K), new(s * K), new(s, 2 * K)
            Y, GM, dH = new(v, F), new(v, F), new(s, F)
            kw = dict(p_attn=Q, p_out=P, seed=7, off_attn=1)
            one = K == 1

            def fwd(drop):
                if one and drop:
                    hip.gat_forward_drop(co, ri, dl, v, H, att, m, at, Y, off_out=2, **kw)
                elif one:
                    hip.gat_forward(co, ri, dl, v, H, att, m, at, Y)
                elif drop:
                    hip.gat_forward_heads_drop(co, ri, dl, v, H, K, att, m, at, Y, off_out=2, **kw)
                else:
                    hip.gat_forward_heads(co, ri, dl, v, H, K, att, m, at, Y)

            def bwd(drop):
                if one and drop:
                    hip.gat_backward_drop(co, ri, dl, v, ro, ci, ceid, s, H, att, at, m, Y, GY, du,
                                          ds2, dH, dS, GM=GM, **kw)
                elif one:
                    hip.gat_backward(co, ri, dl, v, ro, ci, ceid, s, H, att, at, m, Y, GY, du, ds2,
                                     dH, dS, GM=GM)
                elif drop:
                    hip.gat_backward_heads_drop(co, ri, dl, v, ro, ci, ceid, s, H, K, att, at, m, Y,
                                                GY, du, ds2, dH, dS, GM=GM, **kw)
                else:
                    hip.gat_backward_heads(co, ri, dl, v, ro, ci, ceid, s, H, K, att, at, m, Y, GY,
                                           du, ds2, dH, dS, GM=GM)

            def fwd_chain():
                fwd(False)
                ad = at.view(e, K) * (torch.rand(e, K, device=dev) >= Q) * sa
                Z = torch.zeros(v, K, D, device=dev).index_add_(
                    0, d_of_e, H[ril].view(e, K, D) * ad[:, :, None])
                return torch.nn.functional.dropout(torch.relu(Z.view(v, F)), P)

            def bwd_chain():
                bwd(False)
                ad = at.view(e, K) * (torch.rand(e, K, device=dev) >= Q) * sa
                gm = GM[d_of_e].view(e, K, D)
                ga = (gm * H[ril].view(e, K, D)).sum(-1) * ad
                dh = torch.zeros(s, K, D, device=dev).index_add_(0, ril, gm * ad[:, :, None])
                return ga, dh

            f = interleaved({"drop": lambda: fwd(True), "plain": lambda: fwd(False),
                             "chain": fwd_chain}, a.iters, a.repeats)
            fwd(True)  # (the backward reads the dropped forward's Y)
            b = interleaved({"drop": lambda: bwd(True), "plain": lambda: bwd(False),
                             "chain": bwd_chain}, a.iters, a.repeats)
            torch.cuda.synchronize()
            cases.append({"hop": hop, "K": K, "D": D, "v": v, "src": s, "edges": e,
                          "fwd": summary(f), "bwd": summary(b)})
    rec = {"what": "gat_dropout_rate", "rates": [Q, P], "iters": a.iters, "repeats": a.repeats,
           "steps": a.steps, "fanout": [10, 5], "batch": 1024, "cases": cases, "step_ms": step_ms,
           "step_ms_median": {k: med(x) for k, x in step_ms.items()},
           "faster_than_chain": all(c["fwd"]["faster"] and c["bwd"]["faster"] for c in cases)}
    line = json.dumps(rec)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
