"""LinkPredictor::embed_full / evaluate_full (nts/host/linkpred.cpp):
the full-neighbour embedding against a float64 chain over the whole graph and
against the sampled forward where no neighbour is dropped, beside a training
run it must not disturb, and the metrics against tests/linkpred_rank_ref.py on
the kernel's own counts (the counts themselves: tests/test_lp_rank_kernel.py).

Tolerance of the forward comparisons: rtol = atol = 1e-4, the bound of
tests/test_full_infer_driver.py for the same kernels."""
import numpy as np
import pytest
import torch

import edge_weight_blocks as ewb
import linkpred_rank_ref as ref
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
V, B, K = 300, 32, 2


@pytest.fixture(scope="module")
def E():
    from nts import host
    return host.ext()


@pytest.fixture(scope="module")
def data(E):
    src, dst = ewb.simple_graph(V, 3000, 40, seed=9)  # no parallel edges
    s_t = torch.from_numpy(src.view(np.int32)).to(DEV)
    d_t = torch.from_numpy(dst.view(np.int32)).to(DEV)
    a = np.exp2(np.random.default_rng(3).uniform(-2, 2, src.size)).astype(np.float32)
    G = E.FullyRepGraph.from_edges(s_t, d_t, V)
    Gw = E.FullyRepGraph.from_edges(s_t, d_t, V, torch.from_numpy(a).to(DEV))
    col, rows = orc.build_csc(V, src, dst)
    od, idg = orc.degrees(V, src, dst)
    whole = dict(column_offset=col.astype(np.uint32), row_indices=rows,
                 source=np.arange(V, dtype=np.uint32), destination=np.arange(V, dtype=np.uint32),
                 v_size=V, src_size=V, e_size=int(src.size))
    eye = np.eye(V, dtype=np.float32)
    A = {"sum": orc.fuse_fwd(whole, eye, od, idg, weight_mean=False, threads=4),
         "mean": orc.fuse_fwd(whole, eye, od, idg, weight_mean=True, threads=4)}
    A["none"] = (A["sum"] != 0).astype(np.float32)
    edges = torch.stack([torch.from_numpy(src.astype(np.int64)), torch.from_numpy(dst.astype(np.int64))])
    return dict(G=G, Gw=Gw, A=A, edges=edges, src=src, dst=dst,
                gcol=Gw.column_offset.cpu().numpy().astype(np.int64),
                grows=Gw.row_indices.cpu().numpy().view(np.uint32).astype(np.int64),
                a=Gw.edge_prob.cpu().numpy())


def _driver(data, layers, graph="G", drop=0.0, **kw):
    from nts import host, synthetic
    feat = synthetic.features(V, layers[0], device=DEV)
    cfg = host.gcn_config(layers, [3] * (len(layers) - 1), B, drop_rate=drop, pipeline=False,
                          neg_per_pos=K, **kw)
    return host.link_predictor(data[graph], feat, data["edges"][:, :320].contiguous(), cfg), feat


def _chain64(A, feat, W):
    X = feat.cpu().numpy().astype(np.float64)
    A = A.astype(np.float64)
    for l, w in enumerate(W):
        X = (A @ X) @ w.cpu().numpy().astype(np.float64)
        if l < len(W) - 1:
            X = np.maximum(X, 0.0)
    return X


@pytest.mark.parametrize("layers,weight,coef", [
    ([16, 8, 8], "sum", False), ([16, 8, 8], "mean", False), ([16, 8, 8], "none", False),
    ([16, 8], "sum", False), ([16, 8], "mean", False), ([8, 16, 8], "sum", False),
    ([16, 8, 8], "sum", True), ([16, 8], "none", True),
])
def test_embed_full_matches_the_float64_chain(data, layers, weight, coef):
    drv, feat = _driver(data, layers, "Gw" if coef else "G", weight=weight, edge_weighted=coef)
    A = data["A"][weight]
    if coef:  # fl32(c(e) a_e) per edge, the graph has no parallel edges
        d = ewb.edge_dst_ids(data["gcol"])
        Aw = np.zeros_like(A)
        Aw[d, data["grows"]] = ewb.coef_weights(A[d, data["grows"]], data["a"], np.arange(d.size))
        A = Aw
    out = drv.embed_full()
    assert tuple(out.shape) == (V, layers[-1]) and out.dtype == torch.float32
    want = _chain64(A, feat, drv.weights())
    err = np.abs(out.cpu().numpy() - want).max()
    print(f"embed_full {layers} {weight} coef={coef}: max |diff| {err:.3e}, max |ref| {np.abs(want).max():.3e}")
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-4, atol=1e-4)
    assert torch.equal(out, drv.embed_full())  # no random stream anywhere


def test_embed_full_equals_the_sampled_forward_where_no_neighbour_is_dropped(E):
    """every in-degree <= the fanout: the sampled blocks hold every neighbour"""
    from nts import host, synthetic
    n = 120
    i = np.arange(n)
    src = np.concatenate([(i + 1) % n, (i + 7) % n, (i[::2] + 31) % n]).astype(np.int32)
    dst = np.concatenate([i, i, i[::2]]).astype(np.int32)
    G = E.FullyRepGraph.from_edges(torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV), n)
    feat = synthetic.features(n, 16, device=DEV)
    edges = torch.stack([torch.from_numpy(src.astype(np.int64)), torch.from_numpy(dst.astype(np.int64))])
    cfg = host.gcn_config([16, 8, 8], [3, 3], B, drop_rate=0.5, pipeline=False, neg_per_pos=K)
    drv = host.link_predictor(G, feat, edges, cfg)
    drv.train_batch()  # the predictor is in training mode before both calls
    full = drv.embed_full().cpu()
    ids, rows = drv.embed_sampled(edges[:, 40:40 + B].contiguous())
    ids = ids.cpu().numpy().view(np.uint32).astype(np.int64)
    assert ids.size > B and rows.shape == (ids.size, 8)
    print(f"sampled vs full: max |diff| {float((rows.cpu() - full[ids]).abs().max()):.3e} over {ids.size} rows")
    torch.testing.assert_close(rows.cpu(), full[ids], rtol=1e-4, atol=1e-4)


def test_full_evaluation_does_not_disturb_training(data):
    def steps(between):
        drv, _ = _driver(data, [16, 8, 8], drop=0.5)
        out = []
        for i in range(3):
            out.append(drv.train_batch())
            if between and i == 0:
                drv.embed_full()
                drv.evaluate_full(data["edges"][:, 400:470].contiguous(), filtered=True, both_sides=True)
        return out, [w.cpu() for w in drv.weights()], drv.train_seq
    (la, wa, sa), (lb, wb, sb) = steps(False), steps(True)
    assert la == lb and sa == sb == 3
    assert all(torch.equal(x, y) for x, y in zip(wa, wb))


def _kernel_counts(drv, heads, tails, cand=None, adj=None):
    from nts.hip import HipContext
    H = drv.embed_full()
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)
    out = [torch.zeros(len(heads), dtype=torch.int32, device=DEV) for _ in range(3)]
    hip = HipContext(0, seed=1)
    hip.lp_rank(H, H.shape[1], V, i32(heads), i32(tails), *out,
                cand=None if cand is None else i32(cand),
                adj_offset=None if adj is None else torch.from_numpy(adj[0].view(np.int64)).to(DEV),
                adj_sorted=None if adj is None else i32(adj[1]))
    torch.cuda.synchronize()
    return [o.cpu().numpy().view(np.uint32).astype(np.int64) for o in out]


def test_evaluate_full_is_the_metrics_of_the_kernels_counts(data):
    drv, _ = _driver(data, [16, 8, 8])
    for _ in range(3):
        drv.train_batch()
    val = data["edges"][:, 400:470].contiguous()  # 70 edges: three chunks of batch_size 32
    h, t = val[0].numpy(), val[1].numpy()
    adj = ref.sorted_adj(V, data["src"], data["dst"])
    cand = np.random.default_rng(2).integers(0, V, 90)
    plain = drv.evaluate_full(val)
    assert list(plain) == ["mrr", "mrr_optimistic", "mean_rank", "hits@1", "hits@10", "hits@50", "n", "ties"]
    assert 0.0 < plain["mrr"] <= plain["mrr_optimistic"] <= 1.0 and plain["n"] == 70
    assert plain["hits@1"] <= plain["hits@10"] <= plain["hits@50"]
    assert drv.evaluate_full(val) == plain  # a second call
    cases = [(dict(), h, t, None, None),
             (dict(filtered=True), h, t, None, adj),
             (dict(ks=[3, 20]), h, t, None, None),
             (dict(candidates=torch.from_numpy(cand)), h, t, cand, None),
             (dict(both_sides=True, filtered=True), np.concatenate([h, t]), np.concatenate([t, h]), None, adj)]
    for kw, hh, tt, c, a in cases:
        got = drv.evaluate_full(val, **kw)
        g, e, _ = _kernel_counts(drv, hh, tt, c, a)
        want = ref.metrics(g, e, ks=kw.get("ks", (1, 10, 50)))
        assert list(got) == list(want), kw
        for k in want:
            assert got[k] == pytest.approx(want[k], rel=1e-12, abs=0), (kw, k)
    filt = drv.evaluate_full(val, filtered=True)
    print(f"mrr {plain['mrr']:.4f}, filtered {filt['mrr']:.4f}, ties {plain['ties']}")
    assert filt["mrr"] >= plain["mrr"] and filt["mrr_optimistic"] >= plain["mrr_optimistic"]
    assert drv.evaluate_full(val, both_sides=True)["n"] == 2 * plain["n"]


def test_refusals_carry_their_texts(data, E):
    from nts import host
    for kw, text in ((dict(weight="mean-sampled"), "embed_full: MeanSampled weights are a property of a sample"),
                     (dict(up_degree=True), "embed_full: UP_DEGREE weights are a property of a sample")):
        drv, _ = _driver(data, [16, 8, 8], **kw)
        for call in (drv.embed_full, lambda: drv.evaluate_full(data["edges"][:, :8].contiguous())):
            with pytest.raises(RuntimeError) as e:
                call()
            assert str(e.value).splitlines()[0].startswith(text)
    drv, _ = _driver(data, [16, 8, 8])
    with pytest.raises(RuntimeError, match="evaluate_full: filtered takes a graph of at most 2\\^31 vertices"):
        E.check_link_pred_full(host.gcn_config([16, 8, 8], [3, 3], B, neg_per_pos=K),
                               n_vertices=(1 << 31) + 1, filtered=True)
    with pytest.raises(RuntimeError, match="candidates must be vertex ids in \\[0, V\\)"):
        drv.evaluate_full(data["edges"][:, :8].contiguous(), candidates=torch.tensor([0, V]))
    with pytest.raises(RuntimeError, match="hits@k needs k >= 1"):
        drv.evaluate_full(data["edges"][:, :8].contiguous(), ks=[0])
