#!/usr/bin/env python3
"""Cost of the GraphSAGE max aggregator, one JSON line.

Per shape (C3: products-shaped 100-256-256-47, fanout 15-10-5, batch 1024;
C2: reddit-shaped 602-128-41, fanout 25-10, batch 10000):

  ms_per_step  training steps of the driver with aggregator sum and max, wall
               time over `--steps` steps between two synchronisations, the two
               drivers interleaved over `--repeats` rounds;
  bottom_fwd   nts_hip_spmm_csc_fwd_max on the trained batch's bottom layer
               (global table, fused gather, no arg: it has no backward)
               against nts_hip_spmm_csc_fwd at the same operands;
  fwd / bwd    on the hop above (its input width): the forward with arg and
               nts_hip_spmm_csr_bwd_max against nts_hip_spmm_csc_fwd /
               nts_hip_spmm_csr_bwd at the same operands (unit weights), and
               against the libtorch chain index_select + scatter_reduce(amax)
               and its autograd, which materialises the [e, F] messages.

Kernel figures are device time between two HIP events around `--iters`
back-to-back calls (the libtorch chain: a tenth as many), the variants
interleaved per repeat; all repeats are listed and the median reported.
`--scale` shrinks the synthetic graph; batch, fanout and widths stay.  Needs a GPU.

Usage: python scripts/max_aggr_rate.py [--scale 1.0] [--out profiles/max_aggr_rate.json]
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

SHAPES = {
    "C3": dict(shape="products", hidden=[256, 256], fanout=[15, 10, 5], batch=1024, weight="mean"),
    "C2": dict(shape="reddit", hidden=[128], fanout=[25, 10], batch=10000, weight="sum"),
}


def med(xs):
    return sorted(xs)[len(xs) // 2]


def interleaved(fns, iters, repeats):
    """us per call of each fn ((fn, iteration divisor) pairs): warm-up, then per
    repeat every fn in turn"""
    import torch
    for f, _ in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, (f, div) in fns.items():
            n = max(iters // div, 3)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                f()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3 / n)
    return out


def summary(us):
    return {"us": us, **{f"{k}_us_median": med(v) for k, v in us.items()}}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="C3,C2")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("max_aggr_rate: needs a GPU (no CPU fallback)")
    from nts import host, synthetic
    from nts.hip import HipContext
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    E = host.ext()
    hip = HipContext(0)
    cases = []
    for name in a.shapes.split(","):
        sh = SHAPES[name]
        g, F, C = synthetic.shaped(sh["shape"], device=dev, scale=a.scale)
        V = g.n_vertices
        layers = [F] + sh["hidden"] + [C]
        G = E.FullyRepGraph.from_edges(g.src, g.dst, V)
        feat = synthetic.features(V, F, device=dev)
        labels, masks = synthetic.labels_masks(V, C, device=dev)
        train = torch.nonzero(masks == 0).flatten().to(torch.int32).cpu()
        drv = {}
        for aggr in ("sum", "max"):
            cfg = host.gcn_config(layers, sh["fanout"], sh["batch"], weight=sh["weight"],
                                  aggregator=aggr)
            drv[aggr] = E.GCN_SAMPLE_ALLGPU_impl(G, feat, labels, train, cfg)
        ms = {k: [] for k in drv}
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
                ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
        tf = {k: bool(d.transform_first) for k, d in drv.items()}
        lay = drv["max"].last_layers
        bottom, up = lay[-1], lay[-2]
        # bottom forward: from the global table, no arg
        v, s = bottom["v_size"], bottom["src_size"]
        vd = torch.tensor([v], dtype=torch.int32, device=dev)
        ld = (F + 31) // 32 * 32
        y1 = torch.empty(v, ld, device=dev)[:, :F]
        y2 = torch.empty(v, ld, device=dev)[:, :F]
        co, ri, src = bottom["column_offset"], bottom["row_indices"], bottom["source"]
        bfwd = interleaved({
            "max": (lambda: hip.spmm_csc_fwd_max(co, ri, vd, v, feat, y1, row_map=src), 1),
            "sum": (lambda: hip.spmm_csc_fwd(co, ri, None, vd, v, feat, y2, row_map=src), 1),
        }, a.iters, a.repeats)
        # the hop above: forward with arg, backward, the libtorch chain
        Fh = layers[1]
        uv, us, ue = up["v_size"], up["src_size"], up["e_size"]
        uvd = torch.tensor([uv], dtype=torch.int32, device=dev)
        usd = torch.tensor([us], dtype=torch.int32, device=dev)
        gen = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(us, Fh, device=dev, generator=gen)
        gy = torch.randn(uv, Fh, device=dev, generator=gen)
        uco, uri = up["column_offset"], up["row_indices"]
        ro, ci, ceid = up["row_offset"], up["column_indices"], up["csr_edge_id"]
        ym, ys = torch.empty(uv, Fh, device=dev), torch.empty(uv, Fh, device=dev)
        arg = torch.empty(uv, Fh, dtype=torch.int32, device=dev)
        gm, gs = torch.empty(us, Fh, device=dev), torch.empty(us, Fh, device=dev)
        rows = uri.long()
        deg = (uco[1:] - uco[:-1]).long()
        dst_of_e = torch.repeat_interleave(torch.arange(uv, device=dev), deg)
        index = dst_of_e[:, None].expand(ue, Fh)
        xg = x.clone().requires_grad_()

        def chain():
            return torch.zeros(uv, Fh, device=dev).scatter_reduce(
                0, index, xg.index_select(0, rows), "amax", include_self=False)

        out = chain()
        fwd = interleaved({
            "max": (lambda: hip.spmm_csc_fwd_max(uco, uri, uvd, uv, x, ym, arg=arg), 1),
            "sum": (lambda: hip.spmm_csc_fwd(uco, uri, None, uvd, uv, x, ys), 1),
            "torch": (chain, 10),
        }, a.iters, a.repeats)
        hip.spmm_csc_fwd_max(uco, uri, uvd, uv, x, ym, arg=arg)
        torch.cuda.synchronize()
        has = deg > 0
        fwd_equal = bool(torch.equal(ym[has], out.detach()[has]))
        bwd = interleaved({
            "max": (lambda: hip.spmm_csr_bwd_max(ro, ci, ceid, usd, us, gy, arg, gm), 1),
            "sum": (lambda: hip.spmm_csr_bwd(ro, ci, None, usd, us, gy, gs), 1),
            "torch": (lambda: torch.autograd.grad(out, xg, gy, retain_graph=True), 10),
        }, a.iters, a.repeats)
        cases.append({
            "shape": name, "V": V, "E": g.n_edges, "layers": layers, "fanout": sh["fanout"],
            "batch": sh["batch"], "weight_of_sum": sh["weight"], "transform_first": tf,
            "ms_per_step": ms, "ms_per_step_median": {k: med(x_) for k, x_ in ms.items()},
            "bottom_fwd": {"v": v, "src": s, "edges": bottom["e_size"], "F": F, **summary(bfwd)},
            "fwd": {"v": uv, "src": us, "edges": ue, "F": Fh, "arg_bytes": 4 * Fh * uv,
                    "equals_torch_amax": fwd_equal, **summary(fwd)},
            "bwd": {"v": uv, "src": us, "edges": ue, "F": Fh, **summary(bwd)},
        })
        del drv, G, feat, g, out, xg
        torch.cuda.empty_cache()
    rec = {"what": "max_aggr_rate", "scale": a.scale, "steps": a.steps, "iters": a.iters,
           "repeats": a.repeats, "cases": cases}
    line = json.dumps(rec)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
