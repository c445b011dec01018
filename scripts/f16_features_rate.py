#!/usr/bin/env python3
"""Cost and gain of the f16 feature table, one JSON line.

Per shape (C5: papers100M-shaped 128-256-256-172, C3: products-shaped
100-256-256-47, both fanout 15-10-5, batch 1,024; C2: reddit-shaped
602-128-41, fanout 25-10, batch 10,000), always the fp32 path against the f16
path of the same build in the same run:

  bottom_agg   nts_hip_spmm_csc_fwd on the fp32 table against
               nts_hip_spmm_csc_fwd_h on the half table (the driver's pitch, and
               the pitch of the row rounded up to 8 halves), on the bottom layer
               of a trained batch, fused gather: us per call, the achieved rate of
               the compulsory bytes (GCN_SAMPLE_ALLGPU_impl::bottom_bytes' count)
               and of the gathered rows alone (edges x row bytes) in TB/s;
  ms_per_step  training steps of the driver with the option off and on, wall
               time over `--steps` steps between two synchronisations; off is
               the default driver (at C2: transform-first), and at C2 the fp32
               aggregate-first driver is timed too;
  infer_full   (C2) layer 0's aggregation in infer_full(), cfg.profile's device ms.

Kernel figures are device time between two HIP events around `--iters`
back-to-back calls; the variants are interleaved per repeat, all repeats are
listed and the median reported.  `--scale` multiplies each shape's default
scale (the V that loads in seconds); batch, fanout and widths stay.  Needs a GPU.

Usage: python scripts/f16_features_rate.py [--out profiles/f16_features_rate.json]
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
    "C5": dict(shape="papers100m", scale=0.02, hidden=[256, 256], fanout=[15, 10, 5], batch=1024,
               weight="sum"),
    "C3": dict(shape="products", scale=1.0, hidden=[256, 256], fanout=[15, 10, 5], batch=1024,
               weight="mean"),
    "C2": dict(shape="reddit", scale=1.0, hidden=[128], fanout=[25, 10], batch=10000, weight="sum"),
}


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


def step_ms(drv, steps, repeats):
    ms = {k: [] for k in drv}
    for d in drv.values():
        for _ in range(5):
            if not d.sample_not_finished():
                d.restart()
            d.train_batch()
        d.synchronize()
    for _ in range(repeats):
        for k, d in drv.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                if not d.sample_not_finished():
                    d.restart()
                d.train_batch()
            d.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps)
    return ms


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="C5,C3,C2")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("f16_features_rate: needs a GPU (no CPU fallback)")
    from nts import host, synthetic
    from nts.hip import HipContext
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    E = host.ext()
    hip = HipContext(0)
    cases = []
    for name in a.shapes.split(","):
        sh = SHAPES[name]
        g, F, C = synthetic.shaped(sh["shape"], device=dev, scale=sh["scale"] * a.scale)
        V = g.n_vertices
        layers = [F] + sh["hidden"] + [C]
        G = E.FullyRepGraph.from_edges(g.src, g.dst, V)
        feat = synthetic.features(V, F, device=dev)
        labels, masks = synthetic.labels_masks(V, C, device=dev)
        train = torch.nonzero(masks == 0).flatten().to(torch.int32).cpu()

        def driver(**kw):
            cfg = host.gcn_config(layers, sh["fanout"], sh["batch"], weight=sh["weight"], **kw)
            return E.GCN_SAMPLE_ALLGPU_impl(G, feat, labels, train, cfg)

        drv = {"off": driver(), "f16": driver(feature_f16=True)}
        if drv["off"].transform_first:  # C2: also the fp32 order the f16 driver takes
            drv["off_aggregate_first"] = driver(transform_first=0)
        ms = step_ms(drv, a.steps, a.repeats)
        tf = {k: bool(d.transform_first) for k, d in drv.items()}

        # the bottom aggregation of one trained batch, on the three tables
        bottom = drv["f16"].last_layers[-1]
        v, s, e = bottom["v_size"], bottom["src_size"], bottom["e_size"]
        vd = torch.tensor([v], dtype=torch.int32, device=dev)
        co, ri, src, w = (bottom["column_offset"], bottom["row_indices"], bottom["source"],
                          bottom["edge_weight_forward"])
        x32 = feat if F % 32 == 0 or F < 256 else torch.empty(
            V, (F + 31) // 32 * 32, device=dev)[:, :F].copy_(feat)  # the driver's padded table
        xh = drv["f16"].F
        ld8 = (F + 7) // 8 * 8
        xh8 = torch.empty(V, ld8, dtype=torch.float16, device=dev)[:, :F].copy_(xh)
        ldy = (F + 31) // 32 * 32 if F >= 64 else F
        y = [torch.empty(v, ldy, device=dev)[:, :F] for _ in range(3)]
        us = interleaved({
            "fp32": lambda: hip.spmm_csc_fwd(co, ri, w, vd, v, x32, y[0], row_map=src),
            "f16": lambda: hip.spmm_csc_fwd_h(co, ri, w, vd, v, xh, y[1], row_map=src),
            "f16_pitch8": lambda: hip.spmm_csc_fwd_h(co, ri, w, vd, v, xh8, y[2], row_map=src),
        }, a.iters, a.repeats)
        equal = bool(torch.equal(y[1], y[2]))
        agg = {"v": v, "src": s, "edges": e, "F": F, "pitch_halves": int(xh.stride(0)),
               "pitch8_halves": ld8, "pitch_floats": int(x32.stride(0)), "us": us,
               "pitches_agree": equal}
        for k, xb in (("fp32", 4), ("f16", 2), ("f16_pitch8", 2)):
            t = med(us[k]) * 1e-6
            compulsory = F * xb * s + 8.0 * e + 4.0 * (v + 1) + F * 4.0 * v + 4.0 * s
            agg[f"{k}_us_median"] = med(us[k])
            agg[f"{k}_compulsory_TBps"] = compulsory / t / 1e12
            agg[f"{k}_row_gather_TBps"] = float(e) * F * xb / t / 1e12
        case = {"shape": name, "V": V, "E": g.n_edges, "layers": layers, "fanout": sh["fanout"],
                "batch": sh["batch"], "transform_first": tf, "ms_per_step": ms,
                "ms_per_step_median": {k: med(x_) for k, x_ in ms.items()}, "bottom_agg": agg}
        del drv
        torch.cuda.empty_cache()
        if name == "C2":  # the full-neighbour pass: layer 0's aggregation
            full = {}
            prof = {"fp32": driver(profile=True),
                    "f16": driver(profile=True, feature_f16=True)}
            # (the fp32 pass transforms a narrowing layer first: its layer 0 then
            # aggregates layers[1]-wide rows of X W; listed for the comparison)
            for k, d in prof.items():
                runs = []
                for _ in range(a.repeats + 1):
                    d.infer_full()
                    runs.append(list(d.full_agg_ms))
                full[k] = {"agg_ms_per_layer": runs[1:], "layer0_ms_median": med([r[0] for r in runs[1:]])}
            case["infer_full"] = full
            del prof
        cases.append(case)
        del G, feat, g
        torch.cuda.empty_cache()
    rec = {"what": "f16_features_rate", "scale": a.scale, "steps": a.steps, "iters": a.iters,
           "repeats": a.repeats, "gather_ceiling_TBps": [6.7, 7.2], "cases": cases}
    line = json.dumps(rec)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
