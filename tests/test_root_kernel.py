"""GraphSAGE root-weight graph op (the root modes of csrc/aggregate.hip) through the C-ABI.

The arithmetic is defined to the bit (the aggregation's serial edge order,
(x*w)+acc without contraction, the self term one more fp32 add), so every
comparison is np.array_equal / torch.equal: against the existing calls, the CPU
oracle and a float32 numpy restatement.  Blocks come from the real sampler
(merged frontier with SUM / MEAN weights) on a synthetic graph.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NONE = 0xFFFFFFFF
V = 3000
FANOUT = 5
SIZES = (1, 17, 300)
FEATS = (1, 41, 64, 128, 602)
WEIGHTS = {"sum": 0, "mean": 1}


def _t(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(DEV)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=2000)


@pytest.fixture(scope="module")
def graph(hip):
    """nts.synthetic power-law graph with every in-edge (the self loop too) of
    the vertices 0, 7, 14, ... removed: those have in-degree 0."""
    from nts import synthetic
    from nts.hip import DeviceGraph
    g = synthetic.chung_lu(V, 30000, 10.0, device=DEV, seed=5)
    keep = (g.dst % 7) != 0
    s, d = g.src[keep].contiguous(), g.dst[keep].contiguous()
    col, rows = hip.build_csc(s, d, V)
    out_d, in_d = hip.degrees(s, d, V)
    torch.cuda.synchronize()
    src, dst = _u32(s), _u32(d)
    return dict(dev=DeviceGraph(V, src.size, col, rows, in_d, out_d), src=src, dst=dst,
                od=_u32(out_d), idg=_u32(in_d))


def _seeds(n):
    if n == 1:
        return np.array([11], np.uint32)
    return np.random.default_rng(n).choice(V, n, replace=False).astype(np.uint32)


def _sample(hip, graph, seeds, weight_type):
    from nts.hip import LayerBuffers, layer_caps
    (vc, ec, sc), = layer_caps(len(seeds), [FANOUT], V, graph["src"].size, True)
    hip.reserve(V, max(vc, ec, sc))
    vsz = torch.tensor([len(seeds)], dtype=torch.int32, device=DEV)
    lay = LayerBuffers(vc, ec, sc, _t(seeds), vsz, torch.device(DEV), csr=True, weights=True,
                       merge=True)
    hip.sample_layer(graph["dev"], lay, FANOUT, 0, 2, 0, weight_type)
    torch.cuda.synchronize()
    return lay


def _layer_np(lay):
    v, e, s, ovf = lay.sizes_host()
    assert ovf == 0
    return dict(v_size=v, e_size=e, src_size=s, destination=_u32(lay.destination)[:v],
                column_offset=_u32(lay.column_offset)[:v + 1], row_indices=_u32(lay.row_indices)[:e],
                sample_ans=_u32(lay.sample_ans)[:e], source=_u32(lay.source)[:s],
                edge_weight_forward=lay.edge_weight_forward.cpu().numpy()[:e],
                row_offset=_u32(lay.row_offset)[:s + 1],
                column_indices=_u32(lay.column_indices)[:e],
                edge_weight_backward=lay.edge_weight_backward.cpu().numpy()[:e],
                dst_local_id=_u32(lay.dst_local_id)[:v], csr_edge_id=_u32(lay.csr_edge_id)[:e])


@pytest.fixture(scope="module")
def blocks(hip, graph):
    """(weight name, v) -> (LayerBuffers, its arrays on the host)"""
    out = {}
    for name, wt in WEIGHTS.items():
        for n in SIZES:
            lay = _sample(hip, graph, _seeds(n), wt)
            out[name, n] = (lay, _layer_np(lay))
    return out


def _inverse_np(L):
    inv = np.full(L["src_size"], NONE, np.uint32)
    inv[L["dst_local_id"]] = np.arange(L["v_size"], dtype=np.uint32)
    return inv


def _buf(rows, cols, dense, fill=float("nan")):
    """[rows, cols] view: dense (16-byte aligned base, pitch = cols) or with
    pitch cols + 3 on a base one float past an aligned address (scalar path)"""
    ld, off = (cols, 0) if dense else (cols + 3, 1)
    flat = torch.full((rows * ld + off + 4,), fill, dtype=torch.float32, device=DEV)
    return flat[off:off + rows * ld].view(rows, ld)[:, :cols]


def _rand_into(view, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    view.copy_(torch.randn(view.shape, generator=g, device=DEV))
    return view


@pytest.mark.parametrize("name", list(WEIGHTS))
def test_block_has_the_three_kinds_of_vertex(blocks, name):
    _, L = blocks[name, 300]
    assert (np.diff(L["column_offset"]) == 0).any(), "no zero in-degree destination"
    empty = np.diff(L["row_offset"]) == 0
    assert empty.any(), "no source with an empty CSR row"
    inv = _inverse_np(L)
    assert (inv[empty] != NONE).all()  # a source nobody sampled is there as a destination
    assert (inv == NONE).any(), "every source is a destination"
    # the serial restatement below holds for rows the backward sums serially:
    # nts_hip_spmm_csr_bwd splits rows above 16 edges (its smallest threshold)
    assert np.diff(L["row_offset"]).max() <= 16


@pytest.mark.parametrize("name", list(WEIGHTS))
def test_merged_weighted_sampler_matches_oracle(blocks, graph, name):
    col, rows = orc.build_csc(V, graph["src"], graph["dst"])
    o = orc.Sampler(col, rows, graph["idg"], graph["od"], [FANOUT], seed=2000,
                    rng_mode=orc.RNG_PHILOX, order_mode=orc.ORDER_DRAW)
    for n in SIZES:
        _, L = blocks[name, n]
        ref, = o.sample(_seeds(n), 2, WEIGHTS[name] | orc.F_MERGE_SRC_DST)
        assert (L["v_size"], L["e_size"], L["src_size"]) == (ref["v_size"], ref["e_size"],
                                                              ref["src_size"])
        for k in ("destination", "column_offset", "sample_ans", "source", "row_indices",
                  "row_offset", "column_indices", "edge_weight_forward", "edge_weight_backward",
                  "dst_local_id", "csr_edge_id"):
            assert np.array_equal(L[k], ref[k]), (n, k)
        assert np.array_equal(L["source"][L["dst_local_id"]], L["destination"])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(WEIGHTS))
def test_inverse_map(hip, blocks, name, n):
    lay, L = blocks[name, n]
    out = torch.full((lay.s_cap + 7,), 12345, dtype=torch.int32, device=DEV)
    hip.root_inverse_map(lay.dst_local_id, lay.sizes[0:1], lay.v_cap, lay.sizes[2:3], lay.s_cap, out)
    torch.cuda.synchronize()
    got = _u32(out)
    s = L["src_size"]
    ref = _inverse_np(L)
    assert np.array_equal(got[:s], ref)
    assert (got[:s][np.setdiff1d(np.arange(s), L["dst_local_id"])] == NONE).all()
    assert (got[s:] == 12345).all()  # nothing past *s


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "odd_pitch"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(WEIGHTS))
def test_forward(hip, blocks, graph, name, n, dense):
    lay, L = blocks[name, n]
    v, s = L["v_size"], L["src_size"]
    v_dev = lay.sizes[0:1]
    rows_cap = v + 5
    for F in FEATS:
        table = _rand_into(_buf(V, F, dense), F)
        x_loc = _buf(s + 3, F, dense)
        x_loc[:s] = table[lay.source[:s].long()]
        x_loc[s:] = 7.0
        ref = torch.empty(rows_cap, F, device=DEV)
        hip.spmm_csc_fwd(lay.column_offset, lay.row_indices, lay.edge_weight_forward, v_dev,
                         rows_cap, x_loc, ref)
        # local form: x the source rows, self = dst_local_id
        ycat = _buf(rows_cap, 2 * F, dense)
        hip.spmm_csc_fwd_root(lay.column_offset, lay.row_indices, lay.edge_weight_forward, v_dev,
                              rows_cap, x_loc, lay.dst_local_id, ycat)
        # bottom form: x the global table through the source map, self = destination
        ycat_b = _buf(rows_cap, 2 * F, dense)
        hip.spmm_csc_fwd_root(lay.column_offset, lay.row_indices, lay.edge_weight_forward, v_dev,
                              rows_cap, table, lay.destination, ycat_b, row_map=lay.source)
        torch.cuda.synchronize()
        orc_y = orc.fuse_fwd(L, x_loc[:s].cpu().numpy(), graph["od"], graph["idg"],
                             weight_mean=name == "mean")
        self_rows = table[lay.destination[:v].long()]
        for got in (ycat, ycat_b):
            assert torch.equal(got[:v, :F], ref[:v]), (F, "left half vs nts_hip_spmm_csc_fwd")
            assert np.array_equal(got[:v, :F].cpu().numpy(), orc_y), (F, "left half vs oracle")
            assert torch.equal(got[:v, F:], self_rows), (F, "right half")
            assert torch.isnan(got[v:]).all(), (F, "rows past *v written")
        empty = np.flatnonzero(np.diff(L["column_offset"]) == 0)
        assert (ycat[:v, :F][torch.from_numpy(empty).to(DEV)] == 0).all()


def _bwd_numpy(L, g, F, inv, x_act, scale):
    """serial CSR sum in float32, then one add of the self row, then the mask"""
    s = L["src_size"]
    ro, ci, wb = L["row_offset"].astype(np.int64), L["column_indices"], L["edge_weight_backward"]
    acc = np.zeros((s, F), np.float32)
    ln = np.diff(ro)
    for k in range(int(ln.max()) if s else 0):
        r = np.flatnonzero(ln > k)
        j = ro[r] + k
        acc[r] = g[ci[j], :F] * wb[j][:, None] + acc[r]
    has = np.flatnonzero(inv != NONE)
    acc[has] = acc[has] + g[inv[has], F:]
    if x_act is not None:
        acc = np.where(x_act > 0, acc * np.float32(scale), np.float32(0)).astype(np.float32)
    return acc


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "odd_pitch"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(WEIGHTS))
def test_backward(hip, blocks, name, n, dense):
    lay, L = blocks[name, n]
    v, s = L["v_size"], L["src_size"]
    s_dev = lay.sizes[2:3]
    rows_cap = s + 5
    inv_np = _inverse_np(L)
    inv = _t(np.concatenate([inv_np, np.zeros(5, np.uint32)]))
    has = torch.from_numpy(np.flatnonzero(inv_np != NONE)).to(DEV)
    scale = 1.25
    for F in FEATS:
        g = _rand_into(_buf(v + 2, 2 * F, dense), 100 + F)
        x_act = _rand_into(_buf(rows_cap, F, dense), 200 + F)
        # the existing call on the same operands, then the self rows and the mask in torch
        ref = _buf(rows_cap, F, dense)
        hip.spmm_csr_bwd(lay.row_offset, lay.column_indices, lay.edge_weight_backward, s_dev,
                         rows_cap, g[:, :F], ref)
        comp = ref[:s].contiguous()
        comp.index_add_(0, has, g[:, F:][inv[has].long()])
        comp_m = torch.where(x_act[:s] > 0, comp * scale, torch.zeros_like(comp))
        for xa, want in ((None, comp), (x_act, comp_m)):
            outs = []
            for _ in range(2):
                gin = _buf(rows_cap, F, dense)
                hip.spmm_csr_bwd_root(lay.row_offset, lay.column_indices,
                                      lay.edge_weight_backward, s_dev, rows_cap, g, inv, gin,
                                      x_act=xa, scale=scale)
                outs.append(gin)
            torch.cuda.synchronize()
            gin = outs[0]
            assert torch.equal(gin[:s], outs[1][:s]), (F, "two runs differ")
            assert torch.isnan(gin[s:]).all() and torch.isnan(outs[1][s:]).all(), (F, "past *s")
            assert torch.equal(gin[:s], want), (F, "vs nts_hip_spmm_csr_bwd + index_add_")
            rest = _bwd_numpy(L, g.cpu().numpy(), F, inv_np,
                              None if xa is None else x_act[:s].cpu().numpy(), scale)
            assert np.array_equal(gin[:s].cpu().numpy(), rest), (F, "vs the numpy restatement")


@pytest.mark.parametrize("F", [4, 41, 64, 256, 602])
def test_backward_long_rows_follow_the_existing_split(hip, F):
    """Sources more popular than the serial limit (16 to 32 edges by row
    width) are summed in pieces by the whole block, exactly as
    nts_hip_spmm_csr_bwd sums them: a hand-made block with hubs of 17, 33 and
    200 edges beside short rows."""
    rng = np.random.default_rng(F)
    s, v = 70, 260
    lens = rng.integers(0, 6, s)
    lens[[3, 40, 69]] = (17, 33, 200)
    ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    e = int(ro[-1])
    ci = rng.integers(0, v, e).astype(np.uint32)
    wb = rng.random(e).astype(np.float32)
    inv_np = np.full(s, NONE, np.uint32)
    pick = rng.choice(s, 40, replace=False)
    inv_np[pick] = rng.choice(v, 40, replace=False).astype(np.uint32)
    inv_np[[3, 69]] = (5, 6)
    inv_np[40] = NONE
    ro_t, ci_t, wb_t, inv = _t(ro), _t(ci), torch.from_numpy(wb).to(DEV), _t(inv_np)
    s_dev = torch.tensor([s], dtype=torch.int32, device=DEV)
    g = _rand_into(_buf(v, 2 * F, True), F)
    x_act = _rand_into(_buf(s, F, True), F + 1)
    ref = _buf(s, F, True)
    hip.spmm_csr_bwd(ro_t, ci_t, wb_t, s_dev, s, g[:, :F], ref)
    has = torch.from_numpy(np.flatnonzero(inv_np != NONE)).to(DEV)
    comp = ref.clone()
    comp.index_add_(0, has, g[:, F:][inv[has].long()])
    comp = torch.where(x_act > 0, comp * 0.5, torch.zeros_like(comp))
    gin = _buf(s, F, True)
    hip.spmm_csr_bwd_root(ro_t, ci_t, wb_t, s_dev, s, g, inv, gin, x_act=x_act, scale=0.5)
    torch.cuda.synchronize()
    assert torch.equal(gin, comp)


def _pitched(rows, cols, fill=float("nan")):
    """[rows, cols] view of a buffer whose row pitch is cols rounded up to 32
    floats (the 128-byte pitch the driver's buffers have)"""
    ld = (cols + 31) // 32 * 32
    return torch.full((rows, ld), fill, dtype=torch.float32, device=DEV)[:, :cols]


@pytest.mark.parametrize("masked", [True, False], ids=["x_act", "no_mask"])
@pytest.mark.parametrize("F", [18, 41, 602])
def test_backward_long_rows_on_padded_pitches(hip, F, masked):
    """The same hand-made block on 128-byte row pitches with F no multiple of
    4: nts_hip_spmm_csr_bwd takes float4 over the pitch padding there and the
    root backward, whose right half starts at column F, a narrower vector.
    The lane-group shape and the long-row threshold must still be the plain
    call's (at F = 18 and 41 the other reading gives 32 against 16 and 16
    against 4 pieces per long row), so the 33- and 200-edge rows agree to the
    bit only if they are."""
    rng = np.random.default_rng(F)
    s, v = 70, 260
    lens = rng.integers(0, 6, s)
    lens[[3, 40, 69]] = (17, 33, 200)
    ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    e = int(ro[-1])
    ci = rng.integers(0, v, e).astype(np.uint32)
    wb = rng.random(e).astype(np.float32)
    inv_np = np.full(s, NONE, np.uint32)
    pick = rng.choice(s, 40, replace=False)
    inv_np[pick] = rng.choice(v, 40, replace=False).astype(np.uint32)
    inv_np[[3, 69]] = (5, 6)
    inv_np[40] = NONE
    ro_t, ci_t, wb_t, inv = _t(ro), _t(ci), torch.from_numpy(wb).to(DEV), _t(inv_np)
    s_dev = torch.tensor([s], dtype=torch.int32, device=DEV)
    g = _rand_into(_pitched(v, 2 * F), F)
    x_act = _rand_into(_pitched(s, F), F + 1)
    ref = _pitched(s, F)
    hip.spmm_csr_bwd(ro_t, ci_t, wb_t, s_dev, s, g[:, :F], ref)
    has = torch.from_numpy(np.flatnonzero(inv_np != NONE)).to(DEV)
    comp = ref.clone()
    comp.index_add_(0, has, g[:, F:][inv[has].long()])
    if masked:
        comp = torch.where(x_act > 0, comp * 0.5, torch.zeros_like(comp))
    gin = _pitched(s, F)
    hip.spmm_csr_bwd_root(ro_t, ci_t, wb_t, s_dev, s, g, inv, gin,
                          x_act=x_act if masked else None, scale=0.5)
    torch.cuda.synchronize()
    assert torch.equal(gin, comp)
