"""nts_hip_sample_layer_coef on the device.

The entry is nts_hip_sample_layer / nts_hip_sample_layer_weighted with one more
output: every structure array and size must equal the existing entry's for the
same arguments, bit for bit, and
    edge_weight_forward[k] = fl32(c_k * a[q_k])
with c_k the existing entry's weight of the same kept edge (1 under NONE) and
q_k the edge's CSC position in the graph.  The graph (1,500 vertices, ~20,000
edges, one destination of in-degree 1,200) has no parallel edges, so q_k is
recovered on the host from (sample_ans[k], destination[edge_dst[k]]); the
multigraph case knows its positions by construction.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import edge_weight_blocks as eb
from oracle import oracle as orc
from test_hip_kernels import DEV, _gpu_layer_np, _graph, _np_u32, _t

pytestmark = pytest.mark.gpu
V = 1500
W_SUM, W_MEAN, W_NONE, W_MEAN_SAMPLED, W_UP = 0, 1, 2, 3, 0x10
PHILOX, MT_LEMIRE, MT_DIV, SHARED = 0, 1, 2, 3
STRUCT = ("destination", "column_offset", "sample_ans", "source", "row_indices", "row_offset",
          "column_indices", "dst_local_id", "csr_edge_id")


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=2000)


@pytest.fixture(scope="module")
def world(hip):
    src, dst = eb.simple_graph(V, 20000, 1200, 5)
    col, rows = orc.build_csc(V, src, dst)
    deg = np.diff(col.astype(np.int64))
    assert deg[0] == 1200 and deg[V - 1] == 0 and np.sort(deg)[-2] < 1030
    rng = np.random.default_rng(7)
    a = np.exp2(rng.uniform(-3, 3, rows.size)).astype(np.float32)
    prob = np.exp2(rng.uniform(-2, 2, rows.size)).astype(np.float32)
    seeds = np.concatenate([[0], rng.choice(np.arange(1, V), 199, replace=False)]).astype(np.uint32)
    g = _graph(hip, V, src, dst)
    assert np.array_equal(_np_u32(g.row_indices), rows)
    return dict(g=g, col=col, rows=rows, a=a, a_t=torch.from_numpy(a).to(DEV),
                prob_t=torch.from_numpy(prob).to(DEV), seeds=seeds)


def _layer(hip, g, seeds, fanout, rng_mode, wt, s_cap, merge, *, coef=None, prob=None, bs=3,
           layer=1, weights=True):
    from nts.hip import LayerBuffers
    e_cap = g.n_edges if fanout < 0 else min(len(seeds) * fanout, g.n_edges)
    hip.reserve(g.n_vertices, max(e_cap, g.n_vertices))
    vsz = torch.tensor([len(seeds)], dtype=torch.int32, device=DEV)
    lay = LayerBuffers(len(seeds), e_cap, s_cap, _t(np.asarray(seeds, np.uint32)), vsz,
                       torch.device(DEV), csr=True, weights=weights, merge=merge, edge_ids=True)
    hip.sample_layer(g, lay, fanout, layer, bs, rng_mode, wt, edge_prob=prob, edge_coef=coef)
    torch.cuda.synchronize()
    out = _gpu_layer_np(lay)
    out["edge_dst"] = _np_u32(lay.edge_dst)[:out["e_size"]]
    return out


def _check_pair(ref, got, a, q):
    """structure equal to the existing entry's; weights c * a[q]; CSR weights"""
    assert (ref["v_size"], ref["e_size"], ref["src_size"]) == (got["v_size"], got["e_size"],
                                                             got["src_size"])
    for k in STRUCT + ("edge_dst",):
        if k in ref:
            assert np.array_equal(ref[k], got[k]), k
    c = ref.get("edge_weight_forward", np.float32(1))
    want = eb.coef_weights(c, a, q)
    assert got["edge_weight_forward"].dtype == np.float32
    assert np.array_equal(got["edge_weight_forward"].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got["edge_weight_backward"].view(np.uint32),
                          got["edge_weight_forward"][got["csr_edge_id"]].view(np.uint32))


# name: (fanout, rng_mode, weighted draw, weight_type, s_cap, merge)
#   s_cap 600 -> ceil_log2(601) = 10: the full radix sort + k_csr_finalize;
#   s_cap 4096 -> 13: one radix pass + k_csr_bucket
CASES = {
    "philox-f4-g16-sum-fullsort": (4, PHILOX, False, W_SUM, 600, False),
    "philox-f20-mean-bucket": (20, PHILOX, False, W_MEAN, 4096, False),
    "philox-f1030-big-meansampled": (1030, PHILOX, False, W_MEAN_SAMPLED, 4096, False),
    "philox-takeall-none-bucket": (-1, PHILOX, False, W_NONE, 4096, False),
    "shared-f5-sum-dstlocal": (5, SHARED, False, W_SUM, 4096, True),
    "weighted-f5-none": (5, PHILOX, True, W_NONE, 4096, False),
}


@pytest.mark.parametrize("case", list(CASES))
def test_structure_is_the_existing_entrys_and_weights_are_c_times_a(hip, world, case):
    fanout, rng_mode, weighted, wt, s_cap, merge = CASES[case]
    w = world
    prob = w["prob_t"] if weighted else None
    ref = _layer(hip, w["g"], w["seeds"], fanout, rng_mode, wt, s_cap, merge, prob=prob,
                 weights=wt != W_NONE)
    got = _layer(hip, w["g"], w["seeds"], fanout, rng_mode, wt, s_cap, merge, prob=prob,
                 coef=w["a_t"])
    deg = np.diff(w["col"].astype(np.int64))[w["seeds"]]
    assert ref["e_size"] == int((deg if fanout < 0 else np.minimum(deg, fanout)).sum())
    if fanout == 1030:  # only the hub exceeds it
        assert (deg > fanout).sum() == 1
    if merge:
        assert "dst_local_id" in got
    q = eb.layer_positions(w["col"], w["rows"], got)
    assert np.array_equal(w["rows"][q], got["sample_ans"])
    _check_pair(ref, got, w["a"], q)
    if wt == W_NONE:  # the coefficient itself: a caller's own normalisation
        assert np.array_equal(got["edge_weight_forward"], w["a"][q])


@pytest.fixture(scope="module")
def multi(hip):
    """50 destinations (ids 0..49), each with 6 parallel edges from one source
    (id 100 + d) that carry six different coefficients (file order shuffled)."""
    n = 50
    dst = np.repeat(np.arange(n), 6).astype(np.uint32)
    src = (100 + dst).astype(np.uint32)
    Vm = 200
    rng = np.random.default_rng(3)
    perm = rng.permutation(dst.size)
    g = _graph(hip, Vm, src[perm], dst[perm])
    col = g.column_offset.cpu().numpy().astype(np.int64)
    a = np.exp2(rng.uniform(-3, 3, dst.size)).astype(np.float32)
    for d in range(n):
        assert np.unique(a[col[d]:col[d + 1]]).size == 6
    return dict(g=g, col=col, a=a, a_t=torch.from_numpy(a).to(DEV),
                prob_t=torch.from_numpy(np.exp2(rng.uniform(-1, 1, dst.size)).astype(np.float32)).to(DEV),
                seeds=np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("mode", ["philox", "shared", "weighted"])
def test_parallel_edges_keep_their_own_coefficients(hip, multi, mode):
    m = multi
    rng_mode = SHARED if mode == "shared" else PHILOX
    prob = m["prob_t"] if mode == "weighted" else None
    # fanout 8 > 6: everything is taken in CSC order, positions known exactly
    ref = _layer(hip, m["g"], m["seeds"], 8, rng_mode, W_SUM, 600, False, prob=prob)
    got = _layer(hip, m["g"], m["seeds"], 8, rng_mode, W_SUM, 600, False, prob=prob, coef=m["a_t"])
    assert got["e_size"] == 300
    _check_pair(ref, got, m["a"], np.arange(300))
    # fanout 3: a 3-subset of the destination's six, no repeats (NONE: the
    # coefficient itself; s_cap 600: the full-sort CSR carries it under NONE)
    ref = _layer(hip, m["g"], m["seeds"], 3, rng_mode, W_NONE, 600, False, prob=prob, weights=False)
    got = _layer(hip, m["g"], m["seeds"], 3, rng_mode, W_NONE, 600, False, prob=prob, coef=m["a_t"])
    assert got["e_size"] == 150
    for k in STRUCT + ("edge_dst",):
        if k in ref:
            assert np.array_equal(ref[k], got[k]), k
    wf = got["edge_weight_forward"]
    for d in range(50):
        kept = wf[3 * d:3 * d + 3]
        assert np.unique(kept).size == 3
        assert np.isin(kept, m["a"][m["col"][d]:m["col"][d + 1]]).all()
    if mode != "philox":  # key order: ascending position
        for d in range(50):
            six = m["a"][m["col"][d]:m["col"][d + 1]].tolist()
            pos = [six.index(x) for x in wf[3 * d:3 * d + 3]]
            assert pos == sorted(pos)
    assert np.array_equal(got["edge_weight_backward"].view(np.uint32),
                          wf[got["csr_edge_id"]].view(np.uint32))


def test_refusals_leave_the_outputs_as_they_were(hip, world):
    from nts import _abi
    from nts.hip import LayerBuffers
    w = world
    seeds = w["seeds"]
    dst_t = _t(seeds)
    vsz = torch.tensor([seeds.size], dtype=torch.int32, device=DEV)
    omit = torch.zeros(V, dtype=torch.int32, device=DEV)
    a, p = w["a_t"], w["prob_t"]
    # (buffer kwargs, edge_prob, edge_coef, rng_mode, weight_type, word of the message)
    cases = [
        (dict(), None, None, PHILOX, W_SUM, b"edge_coef"),
        (dict(), None, a, MT_LEMIRE, W_SUM, b"MT19937"),
        (dict(), None, a, MT_DIV, W_SUM, b"MT19937"),
        (dict(), None, a, PHILOX, W_SUM | W_UP, b"UP_DEGREE"),
        (dict(omit_map=omit, omit_key=1, omit_loc=omit), None, a, PHILOX, W_SUM, b"omit_map"),
        (dict(), p, a, SHARED, W_SUM, b"PHILOX_SHARED"),
        (dict(weights=False), None, a, PHILOX, W_NONE, b"edge_weight_forward"),
    ]
    for kw, ep, ec, rng_mode, wt, word in cases:
        lay = LayerBuffers(seeds.size, 3000, 3000, dst_t, vsz, torch.device(DEV), **kw)
        names = [k for k, t in lay.t.items() if t is not None]
        for k in names:
            lay.t[k].view(torch.int32).fill_(0x5A5A5A5A)
        g, o = w["g"].as_struct(), lay.as_struct()
        rc = hip.lib.nts_hip_sample_layer_coef(hip.h, C.byref(g), _abi.ptr(ep), _abi.ptr(ec), 10, 0,
                                               0, rng_mode, wt, C.byref(o))
        torch.cuda.synchronize()
        assert rc == 1 and word in hip.lib.nts_hip_last_error(), word  # NTS_ERR_INVALID
        for k in names:
            assert (lay.t[k].view(torch.int32) == 0x5A5A5A5A).all(), (word, k)


def test_existing_entries_give_the_same_bits_around_a_coef_call(hip, world):
    w = world

    def existing():
        return [_layer(hip, w["g"], w["seeds"], f, m, wt, 4096, False, prob=pr)
                for f, m, wt, pr in ((4, PHILOX, W_SUM, None), (20, PHILOX, W_MEAN, None),
                                     (5, SHARED, W_MEAN_SAMPLED, None),
                                     (5, PHILOX, W_SUM, w["prob_t"]))]
    before = existing()
    _layer(hip, w["g"], w["seeds"], 20, PHILOX, W_SUM, 4096, False, coef=w["a_t"])
    _layer(hip, w["g"], w["seeds"], 5, PHILOX, W_NONE, 4096, False, coef=w["a_t"], prob=w["prob_t"])
    after = existing()
    for x, y in zip(before, after):
        assert x.keys() == y.keys()
        for k in x:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k
