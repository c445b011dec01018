#!/usr/bin/env python3
"""Cost of the fused BatchNorm + relu + dropout pass, one JSON line.

Two parts, each a child process of its own under its own time limit:

  kernels  at C2's hidden shape (110,000 x 128) and at 10,000 x 256:
           nts_hip_bn_act_fwd (p = 0.5, running statistics updated: its three
           kernels) and nts_hip_bn_act_bwd (its three kernels), the LayerNorm
           pair nts_hip_ln_act_fwd / _bwd, and the libtorch chain
           dropout(relu(batch_norm(z))) with that chain's autograd backward, all
           timed in the same process; each fused call's share of the HBM peak on
           its algorithmic bytes (forward: two reads and one write of the rows,
           12 F bytes a row; backward: six reads and one write, 28 F);
  steps    C2-shaped training steps (reddit-shaped 602-128-41, fanout 25-10,
           batch 10000) with batch_norm, with layer_norm, and aggregate-first
           without either, wall time over `--steps` steps between two
           synchronisations, the drivers interleaved over `--repeats` rounds.

Kernel figures are device time between two HIP events around `--iters`
back-to-back calls, the variants interleaved per repeat; all repeats are listed
and the median reported.  `--scale` shrinks the synthetic graph.  Needs a GPU.

Usage: python scripts/batch_norm_rate.py [--out profiles/batch_norm_rate.json]
"""
import argparse
import json
import pathlib
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "sample-based-gnn_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E (bench.py's figure)
SHAPES = [(110000, 128), (10000, 256)]
LIMIT_S = {"kernels": 240, "steps": 420}


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


def part_kernels(a):
    import torch
    from nts.hip import HipContext
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    hip = HipContext(0)
    p, eps = 0.5, 1e-5
    cases = []
    for rows, F in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(1)
        z = torch.randn(rows, F, device=dev, generator=gen)
        dy = torch.randn(rows, F, device=dev, generator=gen)
        gamma = 1 + 0.1 * torch.randn(F, device=dev, generator=gen)
        beta = 0.1 * torch.randn(F, device=dev, generator=gen)
        y, dz = torch.empty_like(z), torch.empty_like(z)
        mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
        bmean, brstd = torch.empty(F, device=dev), torch.empty(F, device=dev)
        rm, rv = torch.zeros(F, device=dev), torch.ones(F, device=dev)
        trm, trv = torch.zeros(F, device=dev), torch.ones(F, device=dev)
        dg, db = torch.empty(F, device=dev), torch.empty(F, device=dev)
        zt = z.clone().requires_grad_()
        gt, bt = gamma.clone().requires_grad_(), beta.clone().requires_grad_()

        def chain():
            return torch.dropout(torch.relu(torch.nn.functional.batch_norm(zt, trm, trv, gt, bt, True, 0.1, eps)),
                                 p, True)

        out = chain()
        hip.bn_act_fwd(z, gamma, beta, y, bmean, brstd, eps, 0.1, p, 1, 0, rm, rv)
        us = interleaved({
            "fused_fwd": lambda: hip.bn_act_fwd(z, gamma, beta, y, bmean, brstd, eps, 0.1, p, 1, 0, rm, rv),
            "torch_fwd": chain,
            "ln_fwd": lambda: hip.ln_act_fwd(z, gamma, beta, y, eps, p, 1, 0, mean, rstd),
            "fused_bwd": lambda: hip.bn_act_bwd(dy, y, z, bmean, brstd, gamma, 2.0, dz, dg, db),
            "torch_bwd": lambda: torch.autograd.grad(out, (zt, gt, bt), dy, retain_graph=True),
            "ln_bwd": lambda: hip.ln_act_bwd(dy, y, z, mean, rstd, gamma, 2.0, dz, dg, db),
        }, a.iters, a.repeats)
        m = {k: med(v) for k, v in us.items()}
        nbytes = {"fused_fwd": 3 * 4 * rows * F, "fused_bwd": 7 * 4 * rows * F}
        cases.append({
            "rows": rows, "F": F, "p": p, "us": us, "us_median": m,
            "algorithmic_bytes": nbytes,
            "frac_of_hbm_peak": {k: b / m[k] / 1e3 / HBM_PEAK_GBS for k, b in nbytes.items()},
            "torch_over_fused": {"fwd": m["torch_fwd"] / m["fused_fwd"],
                                 "bwd": m["torch_bwd"] / m["fused_bwd"]},
        })
    return {"cases": cases}


def part_steps(a):
    import torch
    from nts import host, synthetic
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    E = host.ext()
    g, F, C = synthetic.shaped("reddit", device=dev, scale=a.scale)
    V = g.n_vertices
    layers, fanout, batch = [F, 128, C], [25, 10], 10000
    G = E.FullyRepGraph.from_edges(g.src, g.dst, V)
    feat = synthetic.features(V, F, device=dev)
    labels, masks = synthetic.labels_masks(V, C, device=dev)
    train = torch.nonzero(masks == 0).flatten().to(torch.int32).cpu()
    variants = {"aggregate_first": dict(transform_first=0), "layer_norm": dict(layer_norm=True),
                "batch_norm": dict(batch_norm=True)}
    drv = {k: E.GCN_SAMPLE_ALLGPU_impl(G, feat, labels, train, host.gcn_config(layers, fanout, batch, **kw))
           for k, kw in variants.items()}

    def run(d, n):
        for _ in range(n):
            if not d.sample_not_finished():
                d.restart()
            d.train_batch()
        d.synchronize()

    for d in drv.values():
        run(d, 5)
    ms = {k: [] for k in drv}
    for _ in range(a.repeats):
        for k, d in drv.items():
            t0 = time.perf_counter()
            run(d, a.steps)
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    lay = drv["batch_norm"].last_layers
    return {"shape": "C2", "V": V, "E": g.n_edges, "layers": layers, "fanout": fanout, "batch": batch,
            "hidden_rows": int(lay[-1]["v_size"]),
            "transform_first": {k: bool(d.transform_first) for k, d in drv.items()},
            "ms_per_step": ms, "ms_per_step_median": {k: med(v) for k, v in ms.items()}}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", choices=list(LIMIT_S), default=None, help="(internal) run one part")
    a = ap.parse_args(argv)
    if a.part:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("batch_norm_rate: needs a GPU (no CPU fallback)")
        print(json.dumps({"kernels": part_kernels, "steps": part_steps}[a.part](a)))
        return 0
    rec = {"what": "batch_norm_rate", "scale": a.scale, "steps": a.steps, "iters": a.iters,
           "repeats": a.repeats, "hbm_peak_GBs": HBM_PEAK_GBS}
    for part, limit in LIMIT_S.items():  # a part that fails or runs out of time ends the run
        cmd = [sys.executable, __file__, "--part", part, "--scale", str(a.scale), "--steps", str(a.steps),
               "--iters", str(a.iters), "--repeats", str(a.repeats)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            raise SystemExit(f"batch_norm_rate: part {part} ended with status {r.returncode}")
        rec[part] = json.loads(r.stdout.strip().splitlines()[-1])
    line = json.dumps(rec)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
