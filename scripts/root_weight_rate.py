#!/usr/bin/env python3
"""Cost of the GraphSAGE root weight, one JSON line.

Per shape (C3: products-shaped GraphSAGE mean 100-256-256-47, fanout 15-10-5,
batch 1024; C2: reddit-shaped 602-128-41, fanout 25-10, batch 10000):

  ms_per_step    training steps of the driver with root_weight off and on,
                 wall time over `--steps` steps between two synchronisations,
                 the two drivers interleaved over `--repeats` rounds;
  fwd_us         nts_hip_spmm_csc_fwd_root on the trained batch's bottom layer
                 (global table, fused gather) against the two calls it
                 replaces: nts_hip_spmm_csc_fwd at ldy = 2F plus
                 nts_hip_gather_rows into the right half;
  bwd_us         nts_hip_spmm_csr_bwd_root on the hop above against
                 nts_hip_spmm_csr_bwd_postmask plus a libtorch index_add_.

Kernel figures are device time between two HIP events around `--iters`
back-to-back calls, the variants interleaved per repeat; all repeats are
listed and the median reported.  `--scale` shrinks the synthetic graph (vertex
and edge counts); the batch, fanout and widths stay.  Needs a GPU.

Usage: python scripts/root_weight_rate.py [--scale 1.0] [--out FILE]
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
    "C3": dict(shape="products", layers=None, hidden=[256, 256], fanout=[15, 10, 5], batch=1024,
               weight="mean"),
    "C2": dict(shape="reddit", layers=None, hidden=[128], fanout=[25, 10], batch=10000,
               weight="sum"),
}


def med(xs):
    return sorted(xs)[len(xs) // 2]


def interleaved(fns, iters, repeats):
    """us per call of each fn: warm-up, then per repeat every fn in turn"""
    import torch
    for f in fns.values():
        for _ in range(5):
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
        raise SystemExit("root_weight_rate: needs a GPU (no CPU fallback)")
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
        for rw in (False, True):
            cfg = host.gcn_config(layers, sh["fanout"], sh["batch"], weight=sh["weight"],
                                  root_weight=rw)
            drv[rw] = E.GCN_SAMPLE_ALLGPU_impl(G, feat, labels, train, cfg)
        ms = {False: [], True: []}
        for d in drv.values():
            for _ in range(5):
                if not d.sample_not_finished():
                    d.restart()
                d.train_batch()
            d.synchronize()
        for _ in range(a.repeats):
            for rw, d in drv.items():
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    if not d.sample_not_finished():
                        d.restart()
                    d.train_batch()
                d.synchronize()
                ms[rw].append((time.perf_counter() - t0) * 1e3 / a.steps)
        lay = drv[True].last_layers
        bottom, up = lay[-1], lay[-2]
        # forward: the bottom layer from the global table
        v, s = bottom["v_size"], bottom["src_size"]
        vd = torch.tensor([v], dtype=torch.int32, device=dev)
        ld = (2 * F + 31) // 32 * 32
        ycat = torch.empty(v, ld, device=dev)[:, :2 * F]
        ycat2 = torch.empty(v, ld, device=dev)[:, :2 * F]
        co, ri, w = bottom["column_offset"], bottom["row_indices"], bottom["edge_weight_forward"]
        dst, src = bottom["destination"], bottom["source"]

        def fwd_root():
            hip.spmm_csc_fwd_root(co, ri, w, vd, v, feat, dst, ycat, row_map=src)

        def fwd_two():
            hip.spmm_csc_fwd(co, ri, w, vd, v, feat, ycat2[:, :F], row_map=src)
            hip.gather_rows(feat, dst, vd, v, ycat2[:, F:])

        fwd = interleaved({"root": fwd_root, "two_calls": fwd_two}, a.iters, a.repeats)
        fwd_root(), fwd_two()
        torch.cuda.synchronize()
        fwd_equal = bool(torch.equal(ycat, ycat2))
        # backward: the hop above (F_h wide), mask = the layer's activation
        Fh = layers[1]  # the input width of the hop above the bottom one
        uv, us = up["v_size"], up["src_size"]
        sd = torch.tensor([us], dtype=torch.int32, device=dev)
        uvd = torch.tensor([uv], dtype=torch.int32, device=dev)
        gen = torch.Generator(device=dev).manual_seed(1)
        gy = torch.randn(uv, 2 * Fh, device=dev, generator=gen)
        act = torch.randn(us, Fh, device=dev, generator=gen)
        inv = torch.empty(us, dtype=torch.int32, device=dev)
        hip.root_inverse_map(up["dst_local_id"], uvd, uv, sd, us, inv)
        has = torch.nonzero(inv != -1).flatten()
        rows = inv[has].long()
        gi, gi2 = torch.empty(us, Fh, device=dev), torch.empty(us, Fh, device=dev)
        ro, ci, wb = up["row_offset"], up["column_indices"], up["edge_weight_backward"]

        def bwd_root():
            hip.spmm_csr_bwd_root(ro, ci, wb, sd, us, gy, inv, gi, x_act=act, scale=1.0)

        def bwd_two():  # (the mask before the self term: the cost of the two calls, not the result)
            hip.spmm_csr_bwd_postmask(ro, ci, wb, sd, us, gy[:, :Fh], act, gi2, scale=1.0)
            gi2.index_add_(0, has, gy[:, Fh:][rows])

        bwd = interleaved({"root": bwd_root, "two_calls": bwd_two}, a.iters, a.repeats)
        cases.append({
            "shape": name, "V": V, "E": g.n_edges, "layers": layers, "fanout": sh["fanout"],
            "batch": sh["batch"], "weight": sh["weight"],
            "ms_per_step_off": ms[False], "ms_per_step_on": ms[True],
            "ms_per_step_off_median": med(ms[False]), "ms_per_step_on_median": med(ms[True]),
            "fwd": {"v": v, "src": s, "edges": bottom["e_size"], "F": F, "us": fwd,
                    "root_us_median": med(fwd["root"]), "two_calls_us_median": med(fwd["two_calls"]),
                    "bit_equal": fwd_equal},
            "bwd": {"v": uv, "src": us, "edges": up["e_size"], "F": Fh, "us": bwd,
                    "root_us_median": med(bwd["root"]), "two_calls_us_median": med(bwd["two_calls"])},
        })
        del drv, G, feat, g
        torch.cuda.empty_cache()
    rec = {"what": "root_weight_rate", "scale": a.scale, "steps": a.steps, "iters": a.iters,
           "repeats": a.repeats, "cases": cases}
    line = json.dumps(rec)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
