"""GraphSAGE max aggregator (csrc/aggmax.hip, the full-graph call in csrc/infer.hip)
through the C-ABI.

The arithmetic is defined to the bit: per column a serial scan in CSC edge
order that starts from the first edge's value and replaces on a strict >, so
the forward compares np.array_equal (as bit patterns: the sign of a zero is
part of the rule) against the float32 numpy restatement below.  The backward
routes each gradient to the edge that won; its sum follows
nts_hip_spmm_csr_bwd's order, so it is compared exactly where the sum is exact
in any order (integer gradients) or where every slot wins (against that call),
and within 1e-6 * sum|terms| of a float64 restatement otherwise.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NONE = 0xFFFFFFFF
SENTINEL = 12345.0


def _t(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(DEV)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=2000)


# ---------------------------------------------------------------------------
# the rule, restated
# ---------------------------------------------------------------------------
def max_fwd_np(co, ri, x):
    """(y, arg): per column the first edge's value, replaced on a strict > by a
    later edge; an empty column 0.0 / NONE.  x: the rows ri indexes."""
    v, F = co.size - 1, x.shape[1]
    y = np.zeros((v, F), np.float32)
    arg = np.full((v, F), NONE, np.uint32)
    deg = np.diff(co.astype(np.int64))
    for k in range(int(deg.max()) if v else 0):
        d = np.nonzero(deg > k)[0]
        e = co[d].astype(np.int64) + k
        val = x[ri[e]]
        take = np.ones_like(val, bool) if k == 0 else val > y[d]
        y[d] = np.where(take, val, y[d])
        arg[d] = np.where(take, e[:, None].astype(np.uint32), arg[d])
    return y, arg


def max_bwd_np(ro, ci, eid, g_y, arg, F, dtype, src_dst=None, x_act=None, scale=1.0):
    """(g_in, sum of |terms|) in `dtype`"""
    s = ro.size - 1
    rows = np.repeat(np.arange(s), np.diff(ro.astype(np.int64)))
    win = arg[ci] == eid[:, None]
    terms = np.where(win, g_y[ci, :F].astype(dtype), dtype(0))
    g = np.zeros((s, F), dtype)
    mag = np.zeros((s, F), dtype)
    np.add.at(g, rows, terms)
    np.add.at(mag, rows, np.abs(terms))
    if src_dst is not None:
        has = src_dst != NONE
        t = g_y[src_dst[has], F:2 * F].astype(dtype)
        g[has] += t
        mag[has] += np.abs(t)
    if x_act is not None:
        m = (x_act[:s] > 0)
        g = np.where(m, g * dtype(scale), dtype(0))
        mag = np.where(m, mag * dtype(scale), dtype(0))
    return g, mag


# ---------------------------------------------------------------------------
# forward: a hand-built layer with every kind of column
# ---------------------------------------------------------------------------
V_FWD, V_CAP, S_LOC, N_TABLE = 37, 41, 400, 500
FEATS = (1, 7, 100, 128, 602)
# special local source rows (filled by _rows below)
NEG, NINF, SAME, PZERO, NZERO = range(0, 10), (10, 11), (12, 13, 14), 15, 16


@pytest.fixture(scope="module")
def fwd_layer():
    rng = np.random.default_rng(3)
    cols = [
        [],                                              # 0: empty
        [77],                                            # 1: a single edge
        list(rng.choice(np.arange(20, S_LOC), 25, replace=False)),  # 2: fanout 25
        list(rng.integers(20, S_LOC, 300)),              # 3: 300 edges (several id chunks)
        list(rng.choice(NEG, 6)),                        # 4: all negative
        [10, 11, 10],                                    # 5: -inf only
        [13, 12, 14, 12],                                # 6: equal rows: the earliest wins
        [20, 21, 20],                                    # 7: the same source twice
        [NZERO, PZERO],                                  # 8: -0 first: stays -0
        [PZERO, NZERO],                                  # 9: +0 first: stays +0
        [],                                              # 10: another empty one
    ]
    while len(cols) < V_FWD:
        cols.append(list(rng.integers(0, S_LOC, rng.integers(0, 26))))
    co = np.zeros(V_FWD + 1, np.uint32)
    co[1:] = np.cumsum([len(c) for c in cols])
    ri = np.concatenate([np.asarray(c, np.uint32) for c in cols]).astype(np.uint32)
    source = rng.choice(N_TABLE, S_LOC, replace=False).astype(np.uint32)  # local -> table row
    self_loc = rng.integers(0, S_LOC, V_FWD).astype(np.uint32)
    return dict(co=co, ri=ri, source=source, self_loc=self_loc)


def _rows(F, seed):
    """local source rows [S_LOC, F] with the special rows set"""
    x = np.random.default_rng(seed).standard_normal((S_LOC, F)).astype(np.float32)
    x[list(NEG)] = -np.abs(x[list(NEG)]) - 0.5
    x[list(NINF)] = -np.inf
    x[list(SAME)] = x[SAME[0]]
    x[PZERO] = 0.0
    x[NZERO] = -0.0
    x[20, ::2] = x[21, ::2]  # ties between different sources too
    return x


def _pitched(rows, cols, pitch, fill):
    return torch.full((rows, pitch), fill, dtype=torch.float32, device=DEV)[:, :cols]


@pytest.mark.parametrize("F", FEATS)
def test_forward(hip, fwd_layer, F):
    L = fwd_layer
    co, ri = L["co"], L["ri"]
    pitch = 640 if F == 602 else F
    x_np = _rows(F, F)
    y_ref, arg_ref = max_fwd_np(co, ri, x_np)
    # the restatement itself: a winner of its own column, no earlier equal value
    deg = np.diff(co.astype(np.int64))
    for d in range(V_FWD):
        if deg[d] == 0:
            assert (arg_ref[d] == NONE).all() and (_bits(y_ref[d]) == 0).all()
    assert np.signbit(y_ref[8]).all() and not np.signbit(y_ref[9]).any()

    x_loc = _pitched(S_LOC, F, pitch, 3.0)
    x_loc.copy_(_t(x_np))
    table = _pitched(N_TABLE, F, pitch, -5.0)
    table[_t(L["source"]).long()] = x_loc
    co_t, ri_t, src_t = _t(co), _t(ri), _t(L["source"])
    v_dev = torch.tensor([V_FWD], dtype=torch.int32, device=DEV)
    self_loc = _t(L["self_loc"])
    self_glob = _t(L["source"][L["self_loc"]])

    def run(use_map, with_arg, with_self):
        y = _pitched(V_CAP, (2 if with_self else 1) * F, (2 if with_self else 1) * pitch, SENTINEL)
        arg = torch.full((V_CAP, F), 7777, dtype=torch.int32, device=DEV) if with_arg else None
        hip.spmm_csc_fwd_max(co_t, ri_t, v_dev, V_CAP, table if use_map else x_loc, y,
                             row_map=src_t if use_map else None,
                             self_index=(self_glob if use_map else self_loc) if with_self else None,
                             arg=arg)
        torch.cuda.synchronize()
        return y.cpu().numpy(), (_u32(arg) if with_arg else None)

    for use_map in (False, True):
        for with_self in (False, True):
            ys = {}
            for with_arg in (False, True):
                y, arg = run(use_map, with_arg, with_self)
                tag = (F, use_map, with_self, with_arg)
                assert np.array_equal(_bits(y[:V_FWD, :F]), _bits(y_ref)), tag
                assert (y[V_FWD:] == SENTINEL).all(), (tag, "rows past *v written")
                if with_self:
                    assert np.array_equal(_bits(y[:V_FWD, F:]), _bits(x_np[L["self_loc"]])), tag
                if with_arg:
                    assert (arg[V_FWD:] == 7777).all(), (tag, "arg rows past *v written")
                    a = arg[:V_FWD]
                    assert np.array_equal(a, arg_ref), tag
                    live = deg > 0
                    lo, hi = co[:-1][live, None], co[1:][live, None]
                    assert ((a[live] >= lo) & (a[live] < hi)).all(), (tag, "arg outside its column")
                    won = x_np[ri[a[live]], np.arange(F)[None, :]]
                    assert np.array_equal(_bits(won), _bits(y[:V_FWD, :F][live])), tag
                    for d in np.nonzero(live)[0]:  # no earlier edge holds an equal value
                        for e in range(co[d], co[d + 1]):
                            earlier = e < a[d]
                            assert not (earlier & (x_np[ri[e]] == y[d, :F])).any(), (tag, d, e)
                ys[with_arg] = y
            assert np.array_equal(_bits(ys[False]), _bits(ys[True])), (F, "arg changes y")


# ---------------------------------------------------------------------------
# backward: layers from the sampler
# ---------------------------------------------------------------------------
V = 3000
HUB = 5
FANOUT = 5
N_SEEDS = 2500
BWD_FEATS = (7, 100, 256)  # scalar columns; 32 float4 lanes; 64 float4 lanes


def _device_graph(hip, src, dst):
    from nts.hip import DeviceGraph
    s, d = _t(src), _t(dst)
    col, rows = hip.build_csc(s, d, V)
    out_d, in_d = hip.degrees(s, d, V)
    torch.cuda.synchronize()
    return DeviceGraph(V, src.size, col, rows, in_d, out_d)


@pytest.fixture(scope="module")
def hub_graph(hip):
    """every vertex has four in-edges: one from HUB, three from random vertices
    (fanout 5 takes them all: the hub's CSR row has one slot per seed)"""
    rng = np.random.default_rng(9)
    d = np.repeat(np.arange(V, dtype=np.uint32), 4)
    s = rng.integers(0, V, 4 * V).astype(np.uint32)
    s[::4] = HUB
    p = rng.permutation(d.size)
    return _device_graph(hip, s[p], d[p])


@pytest.fixture(scope="module")
def one_edge_graph(hip):
    """every vertex has exactly one in-edge; vertices < 2400 from one of 40
    sources (CSR rows of ~60 slots: long rows), the others from their own"""
    d = np.arange(V, dtype=np.uint32)
    s = np.where(d < 2400, d % 40, (d * 7 + 3) % V).astype(np.uint32)
    return _device_graph(hip, s, d)


def _sample(hip, g, merge):
    from nts import _abi
    from nts.hip import LayerBuffers, layer_caps
    seeds = np.random.default_rng(1).choice(V, N_SEEDS, replace=False).astype(np.uint32)
    (vc, ec, sc), = layer_caps(N_SEEDS, [FANOUT], V, g.n_edges, merge)
    hip.reserve(V, max(vc, ec, sc))
    vsz = torch.tensor([N_SEEDS], dtype=torch.int32, device=DEV)
    lay = LayerBuffers(vc, ec, sc, _t(seeds), vsz, torch.device(DEV), csr=True, weights=False,
                       merge=merge, edge_ids=True)
    hip.sample_layer(g, lay, FANOUT, 0, 2, 0, _abi.NTS_WEIGHT_NONE)
    torch.cuda.synchronize()
    v, e, s, ovf = lay.sizes_host()
    assert ovf == 0
    L = dict(v=v, e=e, s=s, co=_u32(lay.column_offset)[:v + 1], ri=_u32(lay.row_indices)[:e],
             edge_dst=_u32(lay.edge_dst)[:e], ro=_u32(lay.row_offset)[:s + 1],
             ci=_u32(lay.column_indices)[:e], eid=_u32(lay.csr_edge_id)[:e])
    if merge:
        L["dst_local_id"] = _u32(lay.dst_local_id)[:v]
    return lay, L


@pytest.fixture(scope="module")
def hub_layer(hip, hub_graph):
    return _sample(hip, hub_graph, False)


@pytest.fixture(scope="module")
def hub_layer_merged(hip, hub_graph):
    return _sample(hip, hub_graph, True)


def test_edge_ids_without_merge(hub_layer):
    lay, L = hub_layer
    assert lay.dst_local_id is None
    e, s = L["e"], L["s"]
    assert np.array_equal(np.sort(L["eid"]), np.arange(e, dtype=np.uint32))  # a bijection
    rows = np.repeat(np.arange(s, dtype=np.uint32), np.diff(L["ro"].astype(np.int64)))
    assert np.array_equal(L["ri"][L["eid"]], rows)
    assert np.array_equal(L["edge_dst"][L["eid"]], L["ci"])
    assert np.diff(L["ro"].astype(np.int64)).max() >= 2000, "no hub row"


def _forward_arg(hip, lay, L, F, seed):
    x = torch.randn(L["s"], F, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    y = torch.empty(L["v"], F, device=DEV)
    arg = torch.empty(L["v"], F, dtype=torch.int32, device=DEV)
    hip.spmm_csc_fwd_max(lay.column_offset, lay.row_indices, lay.sizes[0:1], L["v"], x, y, arg=arg)
    torch.cuda.synchronize()
    y_ref, arg_ref = max_fwd_np(L["co"], L["ri"], x.cpu().numpy())
    assert np.array_equal(_bits(y.cpu().numpy()), _bits(y_ref))
    assert np.array_equal(_u32(arg), arg_ref)
    return arg, arg_ref


def _run_bwd(hip, lay, L, g_y, arg, F, src_dst=None, x_act=None, scale=1.0):
    g_in = torch.full((L["s"] + 3, F), SENTINEL, device=DEV)
    hip.spmm_csr_bwd_max(lay.row_offset, lay.column_indices, lay.csr_edge_id, lay.sizes[2:3],
                         L["s"] + 3, g_y, arg, g_in, src_dst=src_dst, x_act=x_act, scale=scale)
    torch.cuda.synchronize()
    out = g_in.cpu().numpy()
    assert (out[L["s"]:] == SENTINEL).all(), "rows past *s written"
    return out[:L["s"]]


@pytest.mark.parametrize("F", BWD_FEATS)
@pytest.mark.parametrize("merged", [False, True], ids=["plain", "src_dst"])
def test_backward_routing_exact(hip, hub_layer, hub_layer_merged, merged, F):
    lay, L = hub_layer_merged if merged else hub_layer
    arg, arg_np = _forward_arg(hip, lay, L, F, 100 + F)
    rng = np.random.default_rng(F)
    g_np = rng.integers(-8, 9, (L["v"], (2 if merged else 1) * F)).astype(np.float32)
    g_y = _t(g_np)
    sd_t = sd_np = None
    if merged:
        sd_t = torch.empty(L["s"], dtype=torch.int32, device=DEV)
        hip.root_inverse_map(lay.dst_local_id, lay.sizes[0:1], L["v"], lay.sizes[2:3], L["s"], sd_t)
        torch.cuda.synchronize()
        sd_np = _u32(sd_t)
        assert (sd_np != NONE).any() and (sd_np == NONE).any()
    x_act_np = rng.standard_normal((L["s"] + 3, F)).astype(np.float32)
    for x_act, scale in ((None, 1.0), (x_act_np, 2.0)):
        ref, _ = max_bwd_np(L["ro"], L["ci"], L["eid"], g_np, arg_np, F, np.float32, sd_np,
                            x_act, scale)
        got = _run_bwd(hip, lay, L, g_y, arg, F, sd_t, _t(x_act) if x_act is not None else None,
                       scale)
        assert np.array_equal(_bits(got), _bits(ref + np.float32(0))), (F, merged, scale)


@pytest.mark.parametrize("F", BWD_FEATS)
def test_backward_order_is_the_sum_backwards(hip, one_edge_graph, F):
    lay, L = _sample(hip, one_edge_graph, False)
    assert (np.diff(L["co"].astype(np.int64)) == 1).all()
    deg = np.diff(L["ro"].astype(np.int64))
    assert deg.max() > 32 and (deg == 1).any()  # long rows and short ones
    arg, _ = _forward_arg(hip, lay, L, F, 7)
    g_y = torch.randn(L["v"], F, device=DEV, generator=torch.Generator(device=DEV).manual_seed(F))
    got = _run_bwd(hip, lay, L, g_y, arg, F)
    ref = torch.full((L["s"] + 3, F), SENTINEL, device=DEV)
    hip.spmm_csr_bwd(lay.row_offset, lay.column_indices, None, lay.sizes[2:3], L["s"] + 3, g_y, ref)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got), _bits(ref.cpu().numpy()[:L["s"]])), F


@pytest.mark.parametrize("F", BWD_FEATS)
def test_backward_random_gradient(hip, hub_layer, F):
    lay, L = hub_layer
    arg, arg_np = _forward_arg(hip, lay, L, F, 300 + F)
    g_y = torch.randn(L["v"], F, device=DEV, generator=torch.Generator(device=DEV).manual_seed(F))
    got = _run_bwd(hip, lay, L, g_y, arg, F)
    again = _run_bwd(hip, lay, L, g_y, arg, F)
    assert np.array_equal(_bits(got), _bits(again)), "two runs differ"
    ref, mag = max_bwd_np(L["ro"], L["ci"], L["eid"], g_y.cpu().numpy(), arg_np, F, np.float64)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"F={F}: max err {err.max():.3e}, max bound {(1e-6 * mag).max():.3e}")
    assert (err <= 1e-6 * mag).all()


# ---------------------------------------------------------------------------
# the whole graph
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def skewed(hip):
    """3,000 vertices, ~30,000 random edges, 6,000 edges into vertex 0 (a
    column-sliced hub), vertices 1, 500 and 2999 without in-edges"""
    from nts.hip import DeviceGraph
    rng = np.random.default_rng(21)
    empty = (1, 500, V - 1)
    allowed = np.array([v for v in range(1, V) if v not in empty], np.uint32)
    src = np.concatenate([rng.integers(0, V, 30000), rng.integers(0, V, 6000)]).astype(np.uint32)
    dst = np.concatenate([allowed[rng.integers(0, allowed.size, 30000)],
                          np.zeros(6000, np.uint32)]).astype(np.uint32)
    p = rng.permutation(src.size)
    g = _device_graph(hip, src[p], dst[p])
    co = g.column_offset.cpu().numpy()
    deg = np.diff(co)
    assert deg[0] >= 5000 and all(deg[v] == 0 for v in empty)
    return g, co, _u32(g.row_indices)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("F", (7, 100, 602))
def test_graph_forward(hip, skewed, F, relu):
    g, co, ri = skewed
    # positive inputs keep the sign of a zero maximum out of it; the relu
    # variant gets both signs, so that it has something to cut
    x_np = np.random.default_rng(F).standard_normal((V, F)).astype(np.float32)
    x_np = np.where(x_np == 0, np.float32(1), x_np)
    if not relu:
        x_np = np.abs(x_np)
    pitch = 640 if F == 602 else F
    x = _pitched(V, F, pitch, 0.5)
    x.copy_(_t(x_np))
    y = _pitched(V + 2, F, pitch, SENTINEL)
    hip.spmm_graph_fwd_max(g, x, y, relu=relu)
    torch.cuda.synchronize()
    ref, _ = max_fwd_np(co, ri, x_np)
    if relu:
        ref = np.maximum(ref, np.float32(0))
    got = y.cpu().numpy()
    assert (got[:V] == ref).all(), (F, relu)
    assert (got[V:] == SENTINEL).all()
    # a sub-range leaves the other rows alone
    y2 = _pitched(V, F, pitch, SENTINEL)
    hip.spmm_graph_fwd_max(g, x, y2, relu=relu, v_begin=0, v_end=10)
    torch.cuda.synchronize()
    got2 = y2.cpu().numpy()
    assert (got2[:10] == ref[:10]).all() and (got2[10:] == SENTINEL).all()


def test_graph_forward_refuses_a_bad_vertex_range(hip, skewed):
    g, _, _ = skewed
    x = torch.ones(V, 8, device=DEV)
    y = torch.empty(V, 8, device=DEV)
    with pytest.raises(RuntimeError, match="vertex range"):
        hip.spmm_graph_fwd_max(g, x, y, v_begin=0, v_end=V + 1)
