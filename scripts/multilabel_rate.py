#!/usr/bin/env python3
"""Time of the multi-label output layer's training call.

At n = 10,000 rows, K = 128 and C = 100 and 121 labels, one JSON line with

  fused     nts_hip_linear_bce_train: loss, dY, dW and the tp/fp/fn counters in
            two kernels (the block kernel and the fixed-order finish);
  libtorch  the chain the driver falls back to, on the same tensors: the
            targets gathered and unpacked from the bit table, Z = Y W,
            binary_cross_entropy_with_logits (mean), the three counters, and
            autograd's backward to dY and dW.

Each figure is device time between two HIP events around `--iters` back-to-back
calls on one stream, divided by the iterations; `--repeats` such measurements
after a warm-up, all listed, the median reported.  Y ~ N(0,1),
W ~ N(0,1)/sqrt(K), uniform random labels, the rows' ids a random permutation
prefix of V = 4 n vertices.  Needs a GPU; there is no CPU fallback.

Usage: python scripts/multilabel_rate.py [--n 10000] [--K 128] [--out FILE]
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
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--K", type=int, default=128)
    ap.add_argument("--labels", default="100,121")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("multilabel_rate: needs a GPU (no CPU fallback)")
    from nts import host
    from nts.hip import HipContext
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    E = host.ext()
    hip = HipContext(0)
    g = torch.Generator(device=dev).manual_seed(1)
    n, K, V = a.n, a.K, 4 * a.n
    cases = []
    for C in (int(x) for x in a.labels.split(",")):
        Y = torch.randn(n, K, device=dev, generator=g)
        W = torch.randn(K, C, device=dev, generator=g) / K ** 0.5
        lab = torch.randint(0, 2, (V, C), device=dev, generator=g, dtype=torch.uint8)
        bits = E.pack_label_bits(lab)
        index = torch.randperm(V, device=dev, generator=g)[:n].to(torch.int32)
        loss = torch.empty((), device=dev)
        dY, dW = torch.empty(n, K, device=dev), torch.empty(K, C, device=dev)
        counts = torch.zeros(3, dtype=torch.int32, device=dev)
        shifts = torch.arange(32, device=dev)

        def fused():
            hip.linear_bce_train(Y, W, bits, loss, dY, dW, index=index, counts=counts)

        Yg, Wg = Y.clone().requires_grad_(), W.clone().requires_grad_()
        ccounts = torch.zeros(3, dtype=torch.int32, device=dev)

        def chain():
            words = bits.index_select(0, index.long())
            t = ((words.long().unsqueeze(2) >> shifts) & 1).view(n, -1)[:, :C].float()
            z = Yg @ Wg
            l = torch.nn.functional.binary_cross_entropy_with_logits(z, t)
            pos, tb = z.detach() > 0, t > 0.5
            ccounts.add_(torch.stack([(pos & tb).sum(), (pos & ~tb).sum(),
                                      (~pos & tb).sum()]).to(torch.int32))
            Yg.grad = Wg.grad = None
            l.backward()
            return l

        if not E.hip_linear_bce_supported(K, C):
            raise SystemExit(f"multilabel_rate: K = {K}, C = {C} is outside the fused kernel's range")
        f_us = timed(fused, a.iters, a.repeats)
        c_us = timed(chain, a.iters, a.repeats)
        ref = chain()
        fused()
        torch.cuda.synchronize()
        cases.append({"C": C, "fused_us": f_us, "fused_us_median": f_us[len(f_us) // 2],
                      "libtorch_us": c_us, "libtorch_us_median": c_us[len(c_us) // 2],
                      "speedup": c_us[len(c_us) // 2] / f_us[len(f_us) // 2],
                      "loss_fused": float(loss), "loss_libtorch": float(ref.detach()),
                      "max_abs_dW_diff": float((dW - Wg.grad).abs().max())})
    rec = {"what": "multilabel_rate", "n": n, "K": K, "V": V, "iters": a.iters,
           "repeats": a.repeats, "clock": "hip events around back-to-back calls", "cases": cases}
    line = json.dumps(rec)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
