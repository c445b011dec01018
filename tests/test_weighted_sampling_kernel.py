"""k_select_weighted (nts_hip_sample_layer_weighted) on the device.

Two questions are kept apart by nts_hip_weighted_keys, which writes the key
bits the select kernel computes (the same __device__ function):
  * are the keys right: against the float64 formula of tests/weighted_blocks.py,
    relative error <= 4 * 2^-23 (u is exact; log2f is documented at 1 ulp, the
    division at <= 2.5 ulp in its fast form, plus one rounding);
  * is the selection right given the keys: every array of every layer
    np.array_equal to the restatement's selection from the device's keys.

One graph (V = 40,000: ten tiles of the marks scan) holds 298 destinations of
every degree class — fanout + 1 for the fanouts 1, 10, 25, 70, then 63 / 64 /
65 (one load round), 1,024 / 1,025 (kShKeys x 64: the last degree of the
register path and the first of the histogram path) and 5,000 (79 rounds) —
one vertex of degree 0 and one of degree 1; a cell samples one class plus
those two: 300 destinations.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import weighted_blocks as wb
from oracle import oracle as orc
from test_hip_kernels import DEV, _assert_layers_equal, _gpu_layer_np, _graph, _np_u32, _t

pytestmark = pytest.mark.gpu
SEED = 2000
V = 40_000
PER = 298
FANOUTS = (1, 10, 25, 70)
DEGREES = sorted({f + 1 for f in FANOUTS} | {63, 64, 65, 1024, 1025, 5000})
Z0, Z1 = PER * len(DEGREES), PER * len(DEGREES) + 1  # the degree-0 and the degree-1 vertex
KEY_TOL = 4 * 2.0 ** -23


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=SEED)


@pytest.fixture(scope="module")
def world(hip):
    rng = np.random.default_rng(11)
    src, dst = [], []
    for k, deg in enumerate(DEGREES):
        ids = np.arange(k * PER, (k + 1) * PER)
        dst.append(np.repeat(ids, deg))
        src.append(rng.integers(0, V, PER * deg))  # parallel edges allowed
    src.append(np.array([17]))
    dst.append(np.array([Z1]))
    src.append(rng.integers(0, V, 100_000))  # background: hop-1 destinations have lists too
    dst.append(rng.integers(Z1 + 1, V, 100_000))
    src = np.concatenate(src).astype(np.uint32)
    dst = np.concatenate(dst).astype(np.uint32)
    order = rng.permutation(src.size)  # file order is not CSC order
    src, dst = src[order], dst[order]
    # weights around 1 (2^-2 .. 2^2), one edge in a hundred at an end of the range
    w = np.exp2(rng.uniform(-2, 2, src.size))
    ext = rng.random(src.size) < 0.01
    w[ext] = np.where(rng.random(int(ext.sum())) < 0.5, wb.W_MIN, wb.W_MAX)
    ep = wb.csc_edge_prob(dst, w)
    col, rows = orc.build_csc(V, src, dst)
    od, idg = orc.degrees(V, src, dst)
    deg = np.diff(col.astype(np.int64))
    assert deg[Z0] == 0 and deg[Z1] == 1
    for k, d in enumerate(DEGREES):
        assert (deg[k * PER:(k + 1) * PER] == d).all()
    g = _graph(hip, V, src, dst)
    assert np.array_equal(_np_u32(g.row_indices), rows)
    return dict(g=g, col=col, rows=rows, od=od, idg=idg, ep=ep, ep_t=torch.from_numpy(ep).to(DEV))


def _cell_seeds(degree):
    k = DEGREES.index(degree)
    ids = np.arange(k * PER, (k + 1) * PER, dtype=np.uint32)
    return np.concatenate([ids[:100], [Z0], ids[100:200], [Z1], ids[200:]]).astype(np.uint32)


def _device_keys(hip, w, dst, layer, batch_seq):
    """per destination: the device's key bits of its whole list"""
    dst = np.asarray(dst, np.uint32)
    deg = (w["col"][dst.astype(np.int64) + 1] - w["col"][dst.astype(np.int64)]).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(deg)[:-1]]).astype(np.int64) if dst.size else deg
    keys = hip.weighted_keys(w["g"], w["ep_t"], _t(dst), layer, batch_seq,
                             torch.from_numpy(off).to(DEV))
    torch.cuda.synchronize()
    keys = _np_u32(keys)
    assert keys.size == int(deg.sum())
    return [keys[int(o):int(o + d)] for o, d in zip(off, deg)]


def _sample(hip, w, seeds, fanouts, batch_seq=0, weight_type=0, csr=True, merge=False, layer0=0):
    from nts.hip import LayerBuffers, layer_caps
    g = w["g"]
    caps = layer_caps(len(seeds), fanouts, g.n_vertices, g.n_edges, merge)
    hip.reserve(g.n_vertices, max(max(c) for c in caps))
    dst = _t(np.asarray(seeds, np.uint32))
    vsz = torch.tensor([len(seeds)], dtype=torch.int32, device=DEV)
    layers = []
    for l, (f, (vc, ec, sc)) in enumerate(zip(fanouts, caps)):
        lay = LayerBuffers(vc, ec, sc, dst, vsz, torch.device(DEV), csr=csr,
                           weights=(weight_type & 0xF) != 2, merge=merge)
        hip.sample_layer(g, lay, f, layer0 + l, batch_seq, 0, weight_type, edge_prob=w["ep_t"])
        layers.append(lay)
        dst, vsz = lay.source, lay.sizes[2:3]
    torch.cuda.synchronize()
    return layers


def _restate(hip, w, seeds, fanouts, batch_seq=0, weight_type=0, merge=False, layer0=0):
    """the restatement's layers, selected from the device's keys"""
    out, dst = [], np.asarray(seeds, np.uint32)
    for l, f in enumerate(fanouts):
        keys = _device_keys(hip, w, dst, layer0 + l, batch_seq)
        lay = wb.weighted_layer(w["col"], w["rows"], w["idg"], w["od"], dst, f,
                                lambda i, d, beg, dg: keys[i], weight_type, merge)
        out.append(lay)
        dst = lay["source"]
    return out


@pytest.mark.parametrize("degree", [1, 65, 1025])
def test_keys_against_the_float64_formula(hip, world, degree):
    """weights spanning 2^-60 .. 2^60 (both ends included) on lists of one
    position, two load rounds and the first histogram-path degree"""
    rng = np.random.default_rng(degree)
    n_dst = 64
    dst = np.repeat(np.arange(n_dst), degree).astype(np.uint32)
    src = rng.integers(0, 500, dst.size).astype(np.uint32)
    wts = np.exp2(rng.uniform(-60, 60, dst.size))
    wts[:2] = (wb.W_MIN, wb.W_MAX)
    wts = np.clip(wts.astype(np.float32), np.float32(wb.W_MIN), np.float32(wb.W_MAX))
    g = _graph(hip, 500, src, dst)
    col = g.column_offset.cpu().numpy().astype(np.int64)
    ep = wb.csc_edge_prob(dst, wts)
    ids = np.arange(n_dst, dtype=np.uint32)
    worst = 0.0
    for layer, bs in ((0, 0), (1, (3 << 32) | 5)):
        got = hip.weighted_keys(g, torch.from_numpy(ep).to(DEV), _t(ids), layer, bs,
                                torch.from_numpy(col[:n_dst].copy()).to(DEV))
        torch.cuda.synchronize()
        bits = _np_u32(got)
        assert bits.size == dst.size
        key = bits.view(np.float32).astype(np.float64)
        assert ((bits >= 0x00800000) & (bits < 0x7F800000)).all()  # normal, positive, finite
        for d in ids:
            a, b = int(col[d]), int(col[d + 1])
            want = wb.keys64(SEED, int(d), layer, bs, ep[a:b])
            worst = max(worst, float(np.max(np.abs(key[a:b] - want) / want)))
    print(f"degree {degree}: largest relative key error {worst / 2.0 ** -23:.3f} x 2^-23 "
          f"(bound 4)")
    assert worst <= KEY_TOL


CELLS = [(f, d) for f in FANOUTS for d in DEGREES if d in (f + 1, 63, 64, 65, 1024, 1025, 5000)]
CELL_OPTS = [(wb.W_SUM, True, False), (wb.W_MEAN, False, False), (wb.W_NONE, True, True),
             (wb.W_SUM | wb.W_UP_DEGREE, True, False)]


@pytest.mark.parametrize("fanout,degree", CELLS, ids=[f"f{f}-deg{d}" for f, d in CELLS])
def test_selection_is_exact_given_the_device_keys(hip, world, fanout, degree):
    """300 destinations: the kept positions are the n smallest (key bits,
    position) pairs in ascending position; deg <= fanout keeps all in CSC
    order; and every other array of the layer is the restatement's"""
    seeds = _cell_seeds(degree)
    wt, csr, merge = CELL_OPTS[(FANOUTS.index(fanout) + DEGREES.index(degree)) % len(CELL_OPTS)]
    bs = 7 + degree
    lay = _gpu_layer_np(_sample(hip, world, seeds, [fanout], bs, wt, csr, merge)[0])
    keys = _device_keys(hip, world, seeds, 0, bs)
    co = lay["column_offset"].astype(np.int64)
    col, rows = world["col"], world["rows"]
    selected = 0
    for i, d in enumerate(seeds):
        beg, dg = int(col[d]), int(col[d + 1] - col[d])
        n = min(dg, fanout)
        assert co[i + 1] - co[i] == n
        pair = (keys[i].astype(np.uint64) << np.uint64(32)) | np.arange(dg, dtype=np.uint64)
        pos = np.sort(np.argsort(pair)[:n])
        if dg <= fanout:
            assert np.array_equal(pos, np.arange(dg))
        else:
            selected += 1
        assert np.array_equal(lay["sample_ans"][co[i]:co[i + 1]], rows[beg + pos]), (i, d)
    assert selected == (PER if degree > fanout else 0)
    _assert_layers_equal([lay], _restate(hip, world, seeds, [fanout], bs, wt, merge))


LAYER_CASES = [
    ((10, 25), wb.W_SUM, False, True),
    ((25, 10), wb.W_MEAN, False, False),
    ((70, 1), wb.W_NONE, True, True),
    ((-1, 10), wb.W_SUM, True, True),
]


@pytest.mark.parametrize("fanouts,wt,merge,csr", LAYER_CASES,
                         ids=[f"{f[0]}_{f[1]}-w{w:#x}{'-merge' if m else ''}{'' if c else '-nocsr'}"
                              for f, w, m, c in LAYER_CASES])
def test_the_rest_of_the_layer_over_two_hops(hip, world, fanouts, wt, merge, csr):
    """source ascending and distinct, local row_indices, edge_dst, the CSR with
    csr_edge_id, dst_local_id merging and the Sum / Mean / None weights: what
    the layer restatement builds from the selected set"""
    seeds = np.concatenate([_cell_seeds(d)[::7] for d in DEGREES if d < 5000 or fanouts[0] > 0])
    seeds = np.unique(seeds).astype(np.uint32)
    gl = [_gpu_layer_np(l) for l in _sample(hip, world, seeds, list(fanouts), 4, wt, csr, merge)]
    for lay in gl:
        assert (np.diff(lay["source"].astype(np.int64)) > 0).all()
        assert np.array_equal(lay["source"][lay["row_indices"]], lay["sample_ans"])
    _assert_layers_equal(gl, _restate(hip, world, seeds, list(fanouts), 4, wt, merge))


def _shared_list_graph(hip, weights, n_dst=4096):
    """n_dst destinations with one and the same neighbour list"""
    k = len(weights)
    Vs = n_dst + k
    dst = np.repeat(np.arange(n_dst), k).astype(np.uint32)
    src = np.tile(np.arange(n_dst, n_dst + k), n_dst).astype(np.uint32)
    ep = torch.from_numpy(np.tile(np.asarray(weights, np.float32), n_dst)).to(DEV)
    return dict(g=_graph(hip, Vs, src, dst), ep_t=ep), np.arange(n_dst, dtype=np.uint32), n_dst


@pytest.mark.parametrize("fanout", [1, 3])
def test_inclusion_counts_on_the_device_are_the_exact_probabilities(hip, fanout):
    weights = np.arange(1, 9, dtype=np.float64)
    w, seeds, n_dst = _shared_list_graph(hip, weights)
    lay = _gpu_layer_np(_sample(hip, w, seeds, [fanout], 2, wb.W_NONE, csr=False)[0])
    assert lay["e_size"] == n_dst * fanout
    counts = np.bincount(lay["sample_ans"].astype(np.int64) - n_dst, minlength=8)
    prob = wb.inclusion_probabilities(weights, fanout)
    sd = np.sqrt(n_dst * prob * (1 - prob))
    print(f"fanout {fanout}: counts {counts.tolist()} expected {(n_dst * prob).round(1).tolist()} "
          f"deviations {((counts - n_dst * prob) / sd).round(2).tolist()}")
    assert (np.abs(counts - n_dst * prob) <= 5 * sd).all()


@pytest.mark.parametrize("fanout", [1, 3])
def test_a_heavy_edge_is_kept(hip, fanout):
    """one weight 2^20 times the others: missed only with the exact
    probability's complement (5 binomial standard deviations above it is below
    one destination in 4,096)"""
    weights = np.ones(8)
    weights[5] = 2.0 ** 20
    w, seeds, n_dst = _shared_list_graph(hip, weights)
    lay = _gpu_layer_np(_sample(hip, w, seeds, [fanout], 9, wb.W_NONE, csr=False)[0])
    kept = int((lay["sample_ans"] == n_dst + 5).sum())
    # the complement, computed directly (1 - p would cancel): every pick a light edge
    q = float(np.prod([(7 - j) / (2.0 ** 20 + 7 - j) for j in range(fanout)]))
    assert abs((1 - wb.inclusion_probabilities(weights, fanout)[5]) - q) < 1e-12
    missed = n_dst - kept
    print(f"fanout {fanout}: heavy edge missed by {missed} of {n_dst} (expected {n_dst * q:.3e})")
    assert missed <= n_dst * q + 5 * np.sqrt(n_dst * q * (1 - q))


def test_two_calls_same_bytes_and_batch_seq_or_layer_changes_the_set(hip, world):
    seeds = _cell_seeds(65)
    run = lambda bs, layer0=0: [_gpu_layer_np(l) for l in _sample(hip, world, seeds, [10, 25], bs,
                                                                  layer0=layer0)]
    a, b = run(7), run(7)
    for x, y in zip(a, b):
        for k in x:
            assert np.array_equal(x[k], y[k]), k
    c, d = run(8), run(7, layer0=1)
    for other in (c, d):
        assert a[0]["e_size"] == other[0]["e_size"]
        assert not np.array_equal(a[0]["sample_ans"], other[0]["sample_ans"])


def test_capacity_overflow_sets_the_flag_and_writes_nothing_past_it(hip, world):
    from nts.hip import LayerBuffers
    seeds = np.arange(0, 14000, dtype=np.uint32)  # 4 scan tiles
    hip.reserve(V, 14000 * 10)
    dst_t = _t(seeds)
    vsz = torch.tensor([seeds.size], dtype=torch.int32, device=DEV)
    big, cap = 14000 * 10, 5000
    lay = LayerBuffers(14000, big, big, dst_t, vsz, torch.device(DEV))
    for name in ("sample_ans", "edge_dst", "row_indices"):
        lay.t[name].fill_(-1)
    lay.e_cap = cap
    hip.sample_layer(world["g"], lay, 10, 0, 2, 0, 0, edge_prob=world["ep_t"])
    torch.cuda.synchronize()
    v, e, s, ovf = lay.sizes_host()
    assert v == 14000 and 0 < e <= cap and (ovf & 1), (v, e, ovf)
    co = _np_u32(lay.column_offset)[:v + 1]
    assert e in set(co.tolist())
    assert (_np_u32(lay.sample_ans)[:e] < V).all() and (_np_u32(lay.row_indices)[:e] < s).all()
    for name in ("sample_ans", "edge_dst", "row_indices"):
        assert (_np_u32(lay.t[name])[cap:] == 0xFFFFFFFF).all(), name
    n_dst = int(np.searchsorted(co, e))  # the kept part is the restatement's
    ref = _restate(hip, world, seeds[:n_dst], [10], 2)[0]
    assert ref["e_size"] == e and np.array_equal(_np_u32(lay.sample_ans)[:e], ref["sample_ans"])
    lay = LayerBuffers(14000, big, big, dst_t, vsz, torch.device(DEV))  # in capacity: no flag
    hip.sample_layer(world["g"], lay, 10, 0, 2, 0, 0, edge_prob=world["ep_t"])
    torch.cuda.synchronize()
    assert lay.sizes_host()[3] == 0


def test_null_edge_prob_and_omit_map_are_refused_and_leave_the_outputs(hip, world):
    from nts import _abi
    from nts.hip import LayerBuffers
    seeds = _cell_seeds(65)
    dst_t = _t(seeds)
    vsz = torch.tensor([seeds.size], dtype=torch.int32, device=DEV)
    omit = torch.zeros(V, dtype=torch.int32, device=DEV)
    for kw, ep, word in ((dict(), None, b"edge_prob"),
                         (dict(omit_map=omit, omit_key=1, omit_loc=omit), world["ep_t"], b"omit_map")):
        lay = LayerBuffers(seeds.size, 3000, 3000, dst_t, vsz, torch.device(DEV), **kw)
        names = [k for k, t in lay.t.items() if t is not None]
        for k in names:
            lay.t[k].view(torch.int32).fill_(0x5A5A5A5A)
        g, o = world["g"].as_struct(), lay.as_struct()
        rc = hip.lib.nts_hip_sample_layer_weighted(hip.h, C.byref(g), _abi.ptr(ep), 10, 0, 0,
                                                   _abi.NTS_WEIGHT_SUM, C.byref(o))
        torch.cuda.synchronize()
        assert rc == 1 and word in hip.lib.nts_hip_last_error()  # NTS_ERR_INVALID
        for k in names:
            assert (lay.t[k].view(torch.int32) == 0x5A5A5A5A).all(), k
