#!/usr/bin/env python3
"""Rate of the GAT attention pass over the whole graph (infer_full_gat).

Builds the C2-shaped synthetic graph the way bench.py does (nts.synthetic,
reddit shape) and times, with HIP events on the context's stream, one warm-up
and `--passes` alternating rounds of

  scores      nts_hip_gat_scores over H [V, F]
              (algorithmic bytes 4 V F + 8 F + 8 V K),
  attention   nts_hip_gat_graph_fwd over the global CSC
              (E (4 + 4 F + 4 K) + 4 V F_Y + 4 V K + 8 V: the id, the neighbour
              row and one score per head for every edge; the output rows; the
              destinations' scores; the offsets),

and two yardsticks in the same round, neither of them the code under test:

  bandwidth   nts_hip_spmm_graph_fwd (SUM weights, relu) at the same F on the
              same graph: the same access pattern without the softmax
              (E (4 + 4 F) + 4 V F + 8 V bytes);
  algorithm   nts_hip_gat_forward_heads on the whole graph as ONE block (u32
              offsets, dst_local_id = arange, its two [e, K] arrays allocated),
              at `--yardstick-scale` of the shape (default: the same graph; the
              arrays are 8 E K bytes, 7.4 GB at K = 8).

at F = 128 with K = 8 (concat) and at 41 columns with K = 1.  Prints ONE JSON
line: the raw times, the bytes, bytes / ms against the HBM peak (the pass is
HBM-bound; neighbour rows that hit in cache make the achieved figure exceed
what HBM itself carried) and the two ratios yardstick time / new time.  Needs
a GPU; there is no CPU fallback.

Usage: python scripts/gat_full_infer_rate.py [--scale 1.0] [--yardstick-scale S] [--out FILE]
"""
import argparse
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "sample-based-gnn_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E (bench.py's figure)
CASES = ((8, 16), (1, 41))  # (K, D)


def scores_bytes(V, K, D):
    return 4 * V * K * D + 8 * K * D + 8 * V * K


def attention_bytes(V, E, K, D, mean=False):
    F = K * D
    return E * (4 + 4 * F + 4 * K) + 4 * V * (D if mean else F) + 4 * V * K + 8 * V


def spmm_bytes(V, E, F):
    return E * (4 + 4 * F) + 4 * V * F + 8 * V


def block_bytes(V, E, K, D):
    """the sampled kernel on the whole graph as a block: what attention.cpp counts for it"""
    F = K * D
    return 4 * F * V + 4 * (V + 1) + (4 + 8 * K) * E + 4 * V + 8 * F + 4 * F * V


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", default="reddit")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--yardstick-scale", type=float, default=None)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args(argv)
    ys = a.scale if a.yardstick_scale is None else a.yardstick_scale

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gat_full_infer_rate: needs a GPU (no CPU fallback)")
    from nts import _abi, synthetic
    from nts.hip import DeviceGraph, HipContext
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    hip = HipContext(0, seed=2000)

    def build(scale):
        g, _, _ = synthetic.shaped(a.shape, device=dev, scale=scale)
        V, En = g.n_vertices, g.n_edges
        col, rows = hip.build_csc(g.src, g.dst, V)
        od, idg = hip.degrees(g.src, g.dst, V)
        torch.cuda.synchronize()
        return DeviceGraph(V, En, col, rows, idg, od)

    G = build(a.scale)
    GB = G if ys == a.scale else build(ys)
    assert GB.n_edges < 2 ** 32, "the block yardstick takes u32 offsets"
    co32 = GB.column_offset.to(torch.int32)  # (values below 2^32 wrap to the same u32 bits)
    dl = torch.arange(GB.n_vertices, dtype=torch.int32, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1

    cases = []
    for K, D in CASES:
        F = K * D
        gen = torch.Generator(device=dev).manual_seed(F)
        V, En, Vb, Eb = G.n_vertices, G.n_edges, GB.n_vertices, GB.n_edges
        H = torch.randn(max(V, Vb), F, device=dev, generator=gen)
        att = torch.randn(2 * F, device=dev, generator=gen) * 0.3
        S = torch.empty(V, 2 * K, device=dev)
        Y = torch.empty(V, F, device=dev)
        Ys = torch.empty(V, F, device=dev)
        Yb = torch.empty(Vb, F, device=dev)
        m = torch.empty(Eb * K, device=dev)
        al = torch.empty(Eb * K, device=dev)
        work = {
            "scores": lambda: hip.gat_scores(H[:V], K, att, S),
            "attention": lambda: hip.gat_graph_fwd(G, H[:V], K, S, Y),
            "spmm_graph_fwd": lambda: hip.spmm_graph_fwd(G, H[:V], Ys, _abi.NTS_WEIGHT_SUM, relu=True),
            "gat_forward_heads_block": lambda: hip.gat_forward_heads(
                co32, GB.row_indices, dl, Vb, H[:Vb], K, att, m, al, Yb),
        }
        for fn in work.values():  # warm-up: code objects, scratch growth
            fn()
        torch.cuda.synchronize()
        evs = {k: [] for k in work}
        for _ in range(a.passes):  # the four alternate inside every round
            for k, fn in work.items():
                evs[k].append(timed(fn))
        torch.cuda.synchronize()
        ms = {k: sorted(e0.elapsed_time(e1) for e0, e1 in v) for k, v in evs.items()}
        med = {k: v[len(v) // 2] for k, v in ms.items()}
        same = bool(torch.equal(Y[:Vb], Yb)) if GB is G else None
        diff = float((Y[:Vb] - Yb).abs().max()) if GB is G else None
        nbytes = {"scores": scores_bytes(V, K, D), "attention": attention_bytes(V, En, K, D),
                  "spmm_graph_fwd": spmm_bytes(V, En, F),
                  "gat_forward_heads_block": block_bytes(Vb, Eb, K, D)}
        per = {k: {"ms": ms[k], "ms_median": med[k], "algorithmic_bytes": nbytes[k],
                   "GBs": nbytes[k] / med[k] / 1e6,
                   "frac_of_hbm_peak": nbytes[k] / med[k] / 1e6 / HBM_PEAK_GBS} for k in work}
        # the block kernel computes its scores itself: compare it with scores + attention,
        # per edge where the two graphs differ
        new_per_edge = (med["scores"] + med["attention"]) / En
        cases.append({
            "K": K, "D": D, "F": F, "kernels": per,
            "spmm_over_attention": med["spmm_graph_fwd"] / med["attention"],
            "block_over_new_per_edge": (med["gat_forward_heads_block"] / Eb) / new_per_edge,
            "block_equals_new_bitwise": same, "block_vs_new_max_abs_diff": diff,
            "block_edge_arrays_bytes": 8 * Eb * K})
        del H, S, Y, Ys, Yb, m, al
    rec = {"what": "gat_full_infer_rate", "shape": a.shape, "scale": a.scale, "V": G.n_vertices,
           "E": G.n_edges, "yardstick_scale": ys, "yardstick_V": GB.n_vertices,
           "yardstick_E": GB.n_edges, "passes": a.passes, "bound": "hbm",
           "hbm_peak_GBs": HBM_PEAK_GBS, "cases": cases}
    line = json.dumps(rec)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
