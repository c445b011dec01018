#!/usr/bin/env python3
"""Times of the all-candidate ranking and the full link-prediction evaluation
(DESIGN §8v).

M = 10,000 held-out edges of a Reddit-shaped synthetic graph (nts/synthetic.py)
ranked against all V = 232,965 vertices, D = 128.  One JSON line with

  rank            nts_hip_lp_rank, unfiltered: the [V, D] x [D, M] product on
                  the f32 matrix cores with the compare-and-count epilogue;
                  its fraction of the 157 TF f32 matrix peak (2 M V D flops);
  rank_filtered   the same with the graph filter (lazy searches in the tile
                  kernel plus the n_valid pass over every pair);
  libtorch        the chain on the same inputs in the same session: per chunk
                  of `--chunk` queries H[u] @ H.T, the true tail masked, compare
                  with the positive's score, sum (it writes and re-reads the
                  scores the fused kernel never forms);
  embed_full      LinkPredictor.embed_full() of a [F, 128, D] model;
  evaluate_full   LinkPredictor.evaluate_full() end to end (embed_full, the
                  ranking in chunks of batch_size, the metrics, one read-back).

Device figures: the time between two HIP events around `--iters` back-to-back
calls on one stream, `--repeats` measurements after a warm-up, all listed, the
median reported.  The two driver figures are host wall time around a call that
synchronises.  Needs a GPU.

Usage: python scripts/lp_full_eval_rate.py [--M 10000] [--D 128] [--out FILE]
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

PEAK_F32_MATRIX_TF = 157.0


def timed(fn, iters, repeats, warm=2):
    import torch
    for _ in range(warm):
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
        out.append(a.elapsed_time(b) / iters)  # ms per call
    return sorted(out)


def wall(fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return sorted(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--M", type=int, default=10000)
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--scale", type=float, default=1.0, help="of the Reddit-shaped graph")
    ap.add_argument("--chunk", type=int, default=1000, help="queries per libtorch chunk")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lp_full_eval_rate: needs a GPU (no CPU fallback)")
    from nts import host, synthetic
    from nts.hip import HipContext
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    E = host.ext()
    hip = HipContext(0)
    g, F_in, _ = synthetic.shaped("reddit", device=dev, scale=a.scale)
    V, M, D = g.n_vertices, a.M, a.D
    gen = torch.Generator(device=dev).manual_seed(1)
    pick = torch.randperm(g.n_edges, device=dev, generator=gen)[:M]
    qu, qv = g.src[pick].contiguous(), g.dst[pick].contiguous()
    H = torch.randn(V, D, device=dev, generator=gen) / D ** 0.25
    i32 = dict(dtype=torch.int32, device=dev)
    greater, equal, n_valid = (torch.empty(M, **i32) for _ in range(3))
    G = E.FullyRepGraph.from_edges(g.src, g.dst, V)
    # the filter's arrays, as LinkPredictor builds them
    goff = G.column_offset
    deg = goff[1:] - goff[:-1]
    dst = torch.repeat_interleave(torch.arange(V, device=dev), deg)
    keys = torch.sort(dst * (1 << 32) + (G.row_indices.long() & 0xFFFFFFFF)).values
    srows = (keys & 0xFFFFFFFF).to(torch.int32).contiguous()
    del dst, keys

    def rank():
        hip.lp_rank(H, D, V, qu, qv, greater, equal, n_valid)

    def rank_filtered():
        hip.lp_rank(H, D, V, qu, qv, greater, equal, n_valid, adj_offset=goff, adj_sorted=srows)

    ul, vl = qu.long(), qv.long()
    c_g, c_e = torch.empty(M, dtype=torch.int64, device=dev), torch.empty(M, dtype=torch.int64, device=dev)
    neg_inf = torch.full((a.chunk, 1), float("-inf"), device=dev)

    def chain():
        for o in range(0, M, a.chunk):
            u, v = ul[o:o + a.chunk], vl[o:o + a.chunk]
            hu = H.index_select(0, u)
            sp = (hu * H.index_select(0, v)).sum(1, keepdim=True)
            s = hu @ H.T
            s.scatter_(1, v[:, None], neg_inf[:u.numel()])  # the true tail does not compete
            c_g[o:o + a.chunk] = (s > sp).sum(1)
            c_e[o:o + a.chunk] = (s == sp).sum(1)

    r_ms = timed(rank, a.iters, a.repeats)
    rank()
    torch.cuda.synchronize()
    k_g = greater.long().clone()
    c_ms = timed(chain, 1, a.repeats)
    f_ms = timed(rank_filtered, 1, 3, warm=1)  # (the n_valid pass dominates: fewer repeats)
    # the chain's positive score is a pairwise sum, its product a library GEMM:
    # ranks agree up to rounding, not bit for bit
    rank_diff = (k_g - c_g).abs()

    edges = torch.stack([g.src[pick].cpu().long(), g.dst[pick].cpu().long()])
    feat = synthetic.features(V, F_in, device=dev)
    cfg = host.gcn_config([F_in, 128, D], [10, 5], M, pipeline=False, neg_per_pos=1)
    drv = host.link_predictor(G, feat, edges, cfg)
    e_ms = wall(lambda: drv.embed_full(), a.repeats)
    res = {}
    v_ms = wall(lambda: res.update(drv.evaluate_full(edges)), a.repeats)
    vf_ms = wall(lambda: drv.evaluate_full(edges, filtered=True), 2)

    med = lambda x: x[len(x) // 2]
    flops = 2.0 * M * V * D
    rec = {"what": "lp_full_eval_rate", "graph": "reddit-shaped", "V": V, "E": g.n_edges, "M": M, "D": D,
           "iters": a.iters, "repeats": a.repeats,
           "clock": "hip events around back-to-back calls; drivers: host wall around a synchronising call",
           "rank_ms": r_ms, "rank_ms_median": med(r_ms),
           "rank_TF": flops / (med(r_ms) * 1e-3) / 1e12,
           "rank_fraction_of_f32_matrix_peak": flops / (med(r_ms) * 1e-3) / 1e12 / PEAK_F32_MATRIX_TF,
           "rank_filtered_ms": f_ms, "rank_filtered_ms_median": med(f_ms),
           "libtorch_ms": c_ms, "libtorch_ms_median": med(c_ms), "libtorch_chunk": a.chunk,
           "speedup_vs_libtorch": med(c_ms) / med(r_ms),
           "score_matrix_bytes_not_written": 4 * M * V,
           "rank_vs_libtorch_max_abs_greater_diff": int(rank_diff.max()),
           "rank_vs_libtorch_queries_differing": int((rank_diff != 0).sum()),
           "driver": {"layers": [F_in, 128, D], "embed_full_ms": e_ms, "embed_full_ms_median": med(e_ms),
                      "evaluate_full_ms": v_ms, "evaluate_full_ms_median": med(v_ms),
                      "evaluate_full_filtered_ms": vf_ms, "metrics": res}}
    line = json.dumps(rec)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
