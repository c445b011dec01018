"""nts_hip_spmm_graph_fwd (csrc/infer.hip): the full-neighbour aggregation over
the global CSC, bit for bit against the reference's serial loop.

Reference: orc.fuse_fwd over a "layer" that IS the whole graph (source =
destination = arange(V), column_offset = the global offsets as u32), i.e.
nts_comp's (x*w)+acc sum in CSC edge order for every vertex.  Every comparison
is np.array_equal: the kernel keeps that order at any degree (hub rows are
split by column slice, never by edge range).

Graph (V = 2,000): ~60,000 random edges, a 20,000-edge hub into vertex 0
(duplicates and self-loops included), rows of in-degree exactly 64 / 65 (one
full id chunk of a 64-lane group, and one more) and 2,048 / 2,049 (the last
row a single lane group walks, and the first column-sliced hub), and three
vertices without in-edges.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

V = 2000
EMPTY = (1, 777, V - 1)
EXACT = {10: 64, 11: 65, 12: 2048, 13: 2049}
SENTINEL = 12345.0
# every lane-group width and vector width the dispatch picks: 16 -> 8 lanes of
# float4; 41 -> 64 scalar lanes, or 16 float4 lanes with a 1-float tail when
# padded; 100 / 128 -> 32 float4 lanes; 602 -> five 64-lane float2 slices, or
# three float4 slices with a 2-float tail when padded
FS = (16, 41, 100, 128, 602)


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=2000)


@pytest.fixture(scope="module")
def graph():
    from nts.hip import DeviceGraph
    rng = np.random.default_rng(11)
    fixed = set(EMPTY) | set(EXACT)
    allowed = np.array([v for v in range(V) if v not in fixed], np.uint32)
    src = [rng.integers(0, V, 60000, dtype=np.uint32)]
    dst = [allowed[rng.integers(0, allowed.size, 60000)]]
    src.append(rng.integers(0, V, 20000, dtype=np.uint32))  # the hub (self-loops, duplicates)
    dst.append(np.zeros(20000, np.uint32))
    for v, n in EXACT.items():
        src.append(rng.integers(0, V, n, dtype=np.uint32))
        dst.append(np.full(n, v, np.uint32))
    src, dst = np.concatenate(src), np.concatenate(dst)
    perm = rng.permutation(src.size)  # file order: the rows' edges interleaved
    src, dst = src[perm], dst[perm]
    col, rows = orc.build_csc(V, src, dst)
    od, idg = orc.degrees(V, src, dst)
    deg = np.diff(col.astype(np.int64))
    assert deg[0] > 20000 and all(deg[v] == 0 for v in EMPTY)
    assert all(deg[v] == n for v, n in EXACT.items())
    assert np.any(src == dst)
    g = DeviceGraph(V, int(src.size),
                    torch.from_numpy(col.view(np.int64)).to(DEV),
                    torch.from_numpy(rows.view(np.int32)).to(DEV),
                    torch.from_numpy(idg.view(np.int32)).to(DEV),
                    torch.from_numpy(od.view(np.int32)).to(DEV))
    layer = dict(column_offset=col.astype(np.uint32), row_indices=rows,
                 source=np.arange(V, dtype=np.uint32), destination=np.arange(V, dtype=np.uint32),
                 v_size=V, src_size=V, e_size=int(src.size))
    return dict(g=g, layer=layer, od=od, idg=idg, col=col, rows=rows)


_cache = {}


def _x(F):
    if ("x", F) not in _cache:  # both signs, so the relu has something to cut
        _cache[("x", F)] = np.random.default_rng(100 + F).standard_normal((V, F)).astype(np.float32)
    return _cache[("x", F)]


def _ref(graph, F, mean):
    """the oracle's serial loop over the whole graph, computed once per (F, weights)"""
    if ("y", F, mean) not in _cache:
        y = orc.fuse_fwd(graph["layer"], _x(F), graph["od"], graph["idg"], weight_mean=mean)
        y.setflags(write=False)
        _cache[("y", F, mean)] = y
    return _cache[("y", F, mean)]


def _pitched(a, ld, fill):
    """[V, F] view of a [V, ld] device buffer whose padding holds `fill`"""
    buf = torch.full((a.shape[0], ld), fill, dtype=torch.float32, device=DEV)
    view = buf[:, :a.shape[1]]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return buf, view


def _ld(F, padded):
    return (F + 31) // 32 * 32 if padded else F


def _wt(mean):
    from nts import _abi
    return _abi.NTS_WEIGHT_MEAN if mean else _abi.NTS_WEIGHT_SUM


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("F", FS)
def test_matches_the_serial_loop_bit_for_bit(hip, graph, F, padded, mean, relu):
    ld = _ld(F, padded)
    # NaN in the input pitch padding: a read past the row would poison the sum
    _, x = _pitched(_x(F), ld, float("nan"))
    ybuf, y = _pitched(np.full((V, F), SENTINEL, np.float32), ld, SENTINEL)
    hip.spmm_graph_fwd(graph["g"], x, y, _wt(mean), relu=relu)
    torch.cuda.synchronize()
    ref = _ref(graph, F, mean)
    if relu:
        ref = np.maximum(ref, 0.0)
        assert (ref == 0).any() and (ref > 0).any()
    got = y.cpu().numpy()
    assert np.array_equal(got, ref)
    for v in EMPTY:  # an empty column is a zero row
        assert not got[v].any()
    # the output pitch padding is not written
    assert bool((ybuf[:, F:] == SENTINEL).all())


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("F", FS)
def test_sub_range_leaves_other_rows_alone(hip, graph, F, padded):
    ld = _ld(F, padded)
    _, x = _pitched(_x(F), ld, float("nan"))
    _, y = _pitched(np.full((V, F), SENTINEL, np.float32), ld, SENTINEL)
    hip.spmm_graph_fwd(graph["g"], x, y, _wt(False), v_begin=3, v_end=V - 5)
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert np.array_equal(got[3:V - 5], _ref(graph, F, False)[3:V - 5])
    assert (got[:3] == SENTINEL).all() and (got[V - 5:] == SENTINEL).all()


@pytest.mark.parametrize("F", [41, 602])
def test_two_calls_give_identical_bytes(hip, graph, F):
    x = torch.from_numpy(_x(F)).to(DEV)
    a = torch.empty(V, F, device=DEV)
    b = torch.empty(V, F, device=DEV)
    hip.spmm_graph_fwd(graph["g"], x, a, _wt(True), relu=True)
    hip.spmm_graph_fwd(graph["g"], x, b, _wt(True), relu=True)
    torch.cuda.synchronize()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_no_weights_is_spmm_csc_fwd_without_weights(hip, graph):
    """NTS_WEIGHT_NONE: what nts_hip_spmm_csc_fwd does with weight == NULL
    (weight 1), over the same CSC with u32 offsets."""
    from nts import _abi
    F = 100
    x = torch.from_numpy(_x(F)).to(DEV)
    y = torch.empty(V, F, device=DEV)
    ref = torch.empty(V, F, device=DEV)
    hip.spmm_graph_fwd(graph["g"], x, y, _abi.NTS_WEIGHT_NONE)
    co32 = torch.from_numpy(graph["col"].astype(np.uint32).view(np.int32)).to(DEV)
    n = torch.tensor([V], dtype=torch.int32, device=DEV)
    hip.spmm_csc_fwd(co32, graph["g"].row_indices, None, n, V, x, ref)
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), ref.cpu().numpy())


def test_sample_only_weight_types_are_rejected(hip, graph):
    from nts import _abi
    x = torch.zeros(V, 8, device=DEV)
    y = torch.zeros(V, 8, device=DEV)
    for wt in (_abi.NTS_WEIGHT_MEAN_SAMPLED, _abi.NTS_WEIGHT_SUM | 0x10, _abi.NTS_WEIGHT_MEAN | 0x10):
        with pytest.raises(RuntimeError, match="weight type"):
            hip.spmm_graph_fwd(graph["g"], x, y, wt)
    with pytest.raises(RuntimeError, match="vertex range"):
        hip.spmm_graph_fwd(graph["g"], x, y, _abi.NTS_WEIGHT_SUM, v_end=V + 1)
