"""nts_hip_spmm_graph_fwd_coef / _coef_h: the full-neighbour
aggregation with per-edge coefficients, bit for bit against

  * the serial fp32 restatement (x * fl32(w * a)) + acc in CSC edge order
    (edge_weight_blocks.serial_spmm), w the weight the sampler writes for the
    edge (read back from nts_hip_sample_layer over every vertex, take-all);
  * nts_hip_sample_layer_coef(fanout = -1) + nts_hip_spmm_csc_fwd{,_h} on the
    same rows: the property infer_full() rests on.

Graph (V = 400): ~6,000 random edges, one hub column of 2,100 edges (past the
2,048-edge switch to column slices; parallel edges and self-loops included)
and an empty column.  Widths 7 (scalar lanes), 64 (one float4 / 8-half slice)
and 130 (float2 lanes; half: 2-half vectors over more than one slice).
"""
import numpy as np
import pytest
import torch

import edge_weight_blocks as eb
from oracle import oracle as orc
from test_hip_kernels import _gpu_layer_np, _np_u32, _t

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
V, HUB, EMPTY = 400, 5, 77
FS = (7, 64, 130)
W_SUM, W_MEAN, W_NONE = 0, 1, 2
SENTINEL = 12345.0
V_BEGIN, V_END = 3, V - 6


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=2000)


@pytest.fixture(scope="module")
def world(hip):
    from nts.hip import DeviceGraph, LayerBuffers
    rng = np.random.default_rng(21)
    allowed = np.array([v for v in range(V) if v not in (HUB, EMPTY)], np.uint32)
    src = np.concatenate([rng.integers(0, V, 6000), rng.integers(0, V, 2100)]).astype(np.uint32)
    dst = np.concatenate([allowed[rng.integers(0, allowed.size, 6000)],
                          np.full(2100, HUB)]).astype(np.uint32)
    perm = rng.permutation(src.size)
    src, dst = src[perm], dst[perm]
    col, rows = orc.build_csc(V, src, dst)
    od, idg = orc.degrees(V, src, dst)
    deg = np.diff(col.astype(np.int64))
    assert deg[HUB] == 2100 and deg[EMPTY] == 0 and np.sort(deg)[-2] <= 2048
    E = int(src.size)
    g = DeviceGraph(V, E, torch.from_numpy(col.view(np.int64)).to(DEV),
                    torch.from_numpy(rows.view(np.int32)).to(DEV),
                    torch.from_numpy(idg.view(np.int32)).to(DEV),
                    torch.from_numpy(od.view(np.int32)).to(DEV))
    a = np.exp2(rng.uniform(-3, 3, E)).astype(np.float32)
    # c(e) of every edge, CSC order: the existing sampler, every vertex, take-all
    hip.reserve(V, E)
    ids = _t(np.arange(V, dtype=np.uint32))
    vsz = torch.tensor([V], dtype=torch.int32, device=DEV)
    c = {W_NONE: np.ones(E, np.float32)}
    for wt in (W_SUM, W_MEAN):
        lay = LayerBuffers(V, E, V, ids, vsz, DEV, csr=False)
        hip.sample_layer(g, lay, -1, 0, 0, 0, wt)
        torch.cuda.synchronize()
        lay = _gpu_layer_np(lay)
        assert lay["e_size"] == E and np.array_equal(lay["sample_ans"], rows)
        c[wt] = lay["edge_weight_forward"]
    return dict(g=g, col=col, rows=rows, a=a, a_t=torch.from_numpy(a).to(DEV), c=c, E=E)


_cache = {}


def _x(F, half):
    if ("x", F, half) not in _cache:  # both signs, so the relu has something to cut
        x = np.random.default_rng(100 + F).standard_normal((V, F)).astype(np.float32)
        _cache[("x", F, half)] = x.astype(np.float16) if half else x
    return _cache[("x", F, half)]


def _ref(world, F, wt, half):
    """the serial restatement over the whole graph, once per (F, weights, table)"""
    if ("y", F, wt, half) not in _cache:
        w = eb.coef_weights(world["c"][wt], world["a"], np.arange(world["E"]))
        y = eb.serial_spmm(world["col"], world["rows"], w, _x(F, half).astype(np.float32))
        y.setflags(write=False)
        _cache[("y", F, wt, half)] = y
    return _cache[("y", F, wt, half)]


def _call(hip, world, xt, y, wt, relu, **kw):
    fn = hip.spmm_graph_fwd_h if xt.dtype == torch.float16 else hip.spmm_graph_fwd
    fn(world["g"], xt, y, wt, relu=relu, edge_coef=world["a_t"], **kw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("wt", [W_SUM, W_MEAN, W_NONE], ids=["sum", "mean", "none"])
@pytest.mark.parametrize("F", FS)
def test_matches_the_serial_restatement_bit_for_bit(hip, world, F, wt, relu, half):
    xt = torch.from_numpy(_x(F, half)).to(DEV)
    y = torch.full((V, F), SENTINEL, device=DEV)
    _call(hip, world, xt, y, wt, relu)
    ref = _ref(world, F, wt, half)
    if relu:
        ref = np.maximum(ref, np.float32(0))
        assert (ref == 0).any() and (ref > 0).any()
    got = y.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert not got[EMPTY].any()  # an empty column is a zero row
    # and the coefficients are in it: the unweighted sibling differs
    plain = torch.empty(V, F, device=DEV)
    (hip.spmm_graph_fwd_h if half else hip.spmm_graph_fwd)(world["g"], xt, plain, wt, relu=relu)
    torch.cuda.synchronize()
    assert not np.array_equal(plain.cpu().numpy(), got)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("wt", [W_SUM, W_MEAN, W_NONE], ids=["sum", "mean", "none"])
@pytest.mark.parametrize("F", FS)
def test_sub_range_equals_the_take_all_block_and_leaves_other_rows(hip, world, F, wt, half):
    """rows [V_BEGIN, V_END) (the hub and the empty column inside): equal to
    nts_hip_sample_layer_coef(fanout = -1) + nts_hip_spmm_csc_fwd{,_h} over the
    same destinations, and the sentinel rows outside are untouched"""
    from nts.hip import LayerBuffers
    xt = torch.from_numpy(_x(F, half)).to(DEV)
    y = torch.full((V, F), SENTINEL, device=DEV)
    _call(hip, world, xt, y, wt, False, v_begin=V_BEGIN, v_end=V_END)
    got = y.cpu().numpy()
    assert np.array_equal(got[V_BEGIN:V_END], _ref(world, F, wt, half)[V_BEGIN:V_END])
    assert (got[:V_BEGIN] == SENTINEL).all() and (got[V_END:] == SENTINEL).all()
    n = V_END - V_BEGIN
    ids = _t(np.arange(V_BEGIN, V_END, dtype=np.uint32))
    vsz = torch.tensor([n], dtype=torch.int32, device=DEV)
    lay = LayerBuffers(n, world["E"], V, ids, vsz, DEV, csr=False)
    hip.sample_layer(world["g"], lay, -1, 0, 0, 0, wt, edge_coef=world["a_t"])
    blk = torch.full((n, F), SENTINEL, device=DEV)
    agg = hip.spmm_csc_fwd_h if half else hip.spmm_csc_fwd
    agg(lay.column_offset, lay.row_indices, lay.edge_weight_forward, lay.sizes[0:1], n, xt, blk,
        row_map=lay.source)
    torch.cuda.synchronize()
    assert lay.sizes_host()[3] == 0
    assert np.array_equal(blk.cpu().numpy().view(np.uint32), got[V_BEGIN:V_END].view(np.uint32))


def test_refusals(hip, world):
    x = torch.zeros(V, 8, device=DEV)
    y = torch.zeros(V, 8, device=DEV)
    for fn, xt in ((hip.spmm_graph_fwd, x), (hip.spmm_graph_fwd_h, x.half())):
        for wt in (3, W_SUM | 0x10):  # MEAN_SAMPLED, the UP_DEGREE bit
            with pytest.raises(RuntimeError, match="weight type"):
                fn(world["g"], xt, y, wt, edge_coef=world["a_t"])
        with pytest.raises(RuntimeError, match="vertex range"):
            fn(world["g"], xt, y, W_SUM, v_end=V + 1, edge_coef=world["a_t"])
    g = world["g"].as_struct()
    import ctypes as C
    from nts import _abi
    rc = hip.lib.nts_hip_spmm_graph_fwd_coef(hip.h, C.byref(g), None, 0, V, W_SUM, 0, _abi.ptr(x), 8,
                                             8, _abi.ptr(y), 8)
    assert rc == 1 and b"edge_coef" in hip.lib.nts_hip_last_error()
