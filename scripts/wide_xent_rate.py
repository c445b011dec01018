#!/usr/bin/env python3
"""Time of the output layer + softmax loss's training call above 64 classes
(DESIGN §8f).

At (n, K, C) = (1,024, 256, 172) — the papers100M-shaped configuration's top
layer — and (10,000, 128, 172), one JSON line with

  fused     nts_hip_linear_xent_train: loss, dY, dW and the correct-row counter
            in two kernels (k_top_xent_wide and the fixed-order finish);
  libtorch  the chain the driver runs with fuse_loss off, on the same tensors:
            Z = Y W, log_softmax twice, mean nll_loss, the argmax counter, and
            autograd's backward to dY and dW.

Each figure is device time between two HIP events around `--iters` back-to-back
calls on one stream, divided by the iterations; `--repeats` such measurements
after a warm-up, all listed, the median reported.  Y ~ N(0,1),
W ~ 0.1 N(0,1), uniform random labels.  Needs a GPU; there is no CPU fallback.

Usage: python scripts/wide_xent_rate.py [--shapes 1024x256x172,10000x128x172] [--out FILE]
"""
import argparse
import json
import pathlib
import sys

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
    ap.add_argument("--shapes", default="1024x256x172,10000x128x172", help="n x K x C, comma-separated")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("wide_xent_rate: needs a GPU (no CPU fallback)")
    from nts import host
    from nts.hip import HipContext
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    E = host.ext()
    hip = HipContext(0)
    g = torch.Generator(device=dev).manual_seed(1)
    cases = []
    for n, K, C in (tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")):
        if not E.hip_linear_xent_supported(K, C):
            raise SystemExit(f"wide_xent_rate: K = {K}, C = {C} is outside the fused kernel's range")
        Y = torch.randn(n, K, device=dev, generator=g)
        W = torch.randn(K, C, device=dev, generator=g) * 0.1
        lab = torch.randint(0, C, (n,), device=dev, generator=g)
        loss = torch.empty((), device=dev)
        dY, dW = torch.empty(n, K, device=dev), torch.empty(K, C, device=dev)
        correct = torch.zeros(1, dtype=torch.int32, device=dev)

        def fused():
            hip.linear_xent_train(Y, W, lab, loss, dY, dW, correct)

        Yg, Wg = Y.clone().requires_grad_(), W.clone().requires_grad_()
        ccorrect = torch.zeros(1, dtype=torch.int32, device=dev)

        def chain():
            out = (Yg @ Wg).log_softmax(1)
            ccorrect.add_(out.detach().argmax(1).eq(lab).sum().to(torch.int32))
            l = torch.nn.functional.nll_loss(out.log_softmax(1), lab)
            Yg.grad = Wg.grad = None
            l.backward()
            return l

        f_us = timed(fused, a.iters, a.repeats)
        c_us = timed(chain, a.iters, a.repeats)
        ref = chain()
        fused()
        torch.cuda.synchronize()
        cases.append({"n": n, "K": K, "C": C,
                      "fused_us": f_us, "fused_us_median": f_us[len(f_us) // 2],
                      "libtorch_us": c_us, "libtorch_us_median": c_us[len(c_us) // 2],
                      "speedup": c_us[len(c_us) // 2] / f_us[len(f_us) // 2],
                      "loss_fused": float(loss), "loss_libtorch": float(ref.detach()),
                      "max_abs_dW_diff": float((dW - Wg.grad).abs().max()),
                      "max_abs_dY_diff": float((dY - Yg.grad).abs().max())})
    rec = {"what": "wide_xent_rate", "iters": a.iters, "repeats": a.repeats,
           "clock": "hip events around back-to-back calls", "cases": cases}
    line = json.dumps(rec)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
