"""k_select_shared (NTS_RNG_PHILOX_SHARED) through
nts_hip_sample_layer against the numpy restatement of tests/shared_blocks.py:
every array of every layer np.array_equal.

The graph (V = 80,000, so the marks scan crosses 20 tiles) has destinations on
every path of the kernel: degree 0, 1, 2, fanout - 1 / fanout / fanout + 1 for
the fanouts 10, 25, 64 and 1,500, 63 / 64 / 65 (one load round), the last degree
of the register path and the first of the multi-pass path (kShKeys x 64 = 1,024
and 1,025, read from csrc/sampler.hip's own constant), hubs of 20,000 and
70,000 edges (the 70,000 one past 2^16, where distinct sources collide in
their 32-bit r and the position half of the key decides), two destinations
whose lists hold each source twice (80 and 1,200 edges: one per path), and one
destination listing all of those, which makes them hop-1 destinations.
"""
import re

import numpy as np
import pytest
import torch

import shared_blocks as sb
from conftest import ROOT
from oracle import oracle as orc
from test_hip_kernels import DEV, _assert_layers_equal, _gpu_layer_np, _graph, _np_u32, _sample_gpu, _t

pytestmark = pytest.mark.gpu
SHARED, PHILOX = 3, 0
SEED = 2000
V = 80_000


def _reg_max():
    text = (ROOT / "sample-based-gnn_amd" / "csrc" / "sampler.hip").read_text()
    keys = int(re.search(r"constexpr int kShKeys = (\d+);", text).group(1))
    assert "kShRegMax = kShKeys * kWave" in text
    return keys * 64


REG_MAX = _reg_max()
DEGREES = sorted({0, 1, 2, 9, 10, 11, 24, 25, 26, 63, 64, 65, 1499, 1500, 1501, REG_MAX - 1,
                  REG_MAX, REG_MAX + 1}) + [20_000, 70_000]
HUBS = (len(DEGREES) - 2, len(DEGREES) - 1)  # destination ids of the two hubs


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=SEED)


@pytest.fixture(scope="module")
def world(hip):
    rng = np.random.default_rng(5)
    src, dst = [], []
    for d, deg in enumerate(DEGREES):  # destination d: `deg` distinct sources
        src.append(rng.choice(V, deg, replace=False))
        dst.append(np.full(deg, d))
    n = len(DEGREES)
    for d, k in ((n, 40), (n + 1, 600)):  # every source twice
        s = rng.choice(V, k, replace=False)
        src.append(np.concatenate([s, s[::-1]]))
        dst.append(np.full(2 * k, d))
    special = n + 2
    src.append(np.arange(special))  # destination `special` lists all of the above
    dst.append(np.full(special, special))
    src.append(rng.integers(0, V, 640_000))  # background, parallel edges allowed
    dst.append(rng.integers(special + 1, V, 640_000))
    src = np.concatenate(src).astype(np.uint32)
    dst = np.concatenate(dst).astype(np.uint32)
    col, rows = orc.build_csc(V, src, dst)
    od, idg = orc.degrees(V, src, dst)
    deg = np.diff(col.astype(np.int64))
    assert deg[:n].tolist() == DEGREES and deg[n] == 80 and deg[n + 1] == 1200
    seeds = np.concatenate([np.arange(special + 1), rng.choice(np.arange(special + 1, V), 200,
                                                               replace=False)]).astype(np.uint32)
    return dict(g=_graph(hip, V, src, dst), col=col, rows=rows, od=od, idg=idg, seeds=seeds,
                special=special)


def _both(hip, w, seeds, fanouts, wt, merge=False, csr=True, batch_seq=3):
    gl = [_gpu_layer_np(l) for l in _sample_gpu(hip, w["g"], seeds, list(fanouts), SHARED,
                                                batch_seq, wt, csr=csr, merge=merge)]
    hl = sb.shared_sample(w["col"], w["rows"], w["idg"], w["od"], seeds, list(fanouts), SEED,
                          batch_seq, wt, merge)
    return gl, hl


CASES = [
    ((10, 25), sb.W_SUM, False, True),
    ((25, 10), sb.W_MEAN, False, False),
    ((1, 64), sb.W_NONE, False, True),
    ((64, 1), sb.W_SUM | sb.W_UP_DEGREE, False, True),
    ((1500, 10), sb.W_SUM, True, True),
    ((64, 1500), sb.W_MEAN, False, True),
    ((64, -1), sb.W_SUM, False, True),
    ((-1, 25), sb.W_NONE, False, False),
]


@pytest.mark.parametrize("fanouts,wt,merge,csr", CASES,
                         ids=[f"{f[0]}_{f[1]}-w{w:#x}{'-merge' if m else ''}{'' if c else '-nocsr'}"
                              for f, w, m, c in CASES])
def test_every_layer_array_equals_the_restatement(hip, world, fanouts, wt, merge, csr):
    seeds = world["seeds"]
    if fanouts[0] < 0:  # (the hubs enter at hop 1, through the listing destination)
        seeds = np.array([s for s in seeds if s not in HUBS], np.uint32)
    gl, hl = _both(hip, world, seeds, fanouts, wt, merge, csr)
    _assert_layers_equal(gl, hl)
    if fanouts[0] >= world["special"]:  # every special destination is a hop-1 destination
        assert set(range(world["special"])) <= set(gl[1]["destination"].tolist())


def test_two_calls_same_bytes_and_batch_seq_changes_the_selection(hip, world):
    a = [_gpu_layer_np(l) for l in _sample_gpu(hip, world["g"], world["seeds"], [10, 25], SHARED, 7)]
    b = [_gpu_layer_np(l) for l in _sample_gpu(hip, world["g"], world["seeds"], [10, 25], SHARED, 7)]
    for x, y in zip(a, b):
        for k in x:
            assert np.array_equal(x[k], y[k]), k
    c = [_gpu_layer_np(l) for l in _sample_gpu(hip, world["g"], world["seeds"], [10, 25], SHARED, 8)]
    assert a[0]["e_size"] == c[0]["e_size"]
    assert not np.array_equal(a[0]["sample_ans"], c[0]["sample_ans"])


def test_philox_is_unchanged_around_a_shared_call(hip, world):
    """the new mode leaves no state behind: PHILOX before == PHILOX after"""
    run = lambda mode: [_gpu_layer_np(l) for l in _sample_gpu(hip, world["g"], world["seeds"],
                                                              [10, 25], mode, 5)]
    before, _, after = run(PHILOX), run(SHARED), run(PHILOX)
    for x, y in zip(before, after):
        for k in x:
            assert np.array_equal(x[k], y[k]), k
    o = orc.Sampler(world["col"], world["rows"], world["idg"], world["od"], [10, 25], seed=SEED,
                    rng_mode=orc.RNG_PHILOX, order_mode=orc.ORDER_DRAW)
    _assert_layers_equal(after, o.sample(world["seeds"], 5))


def test_capacity_overflow_sets_the_flag_and_writes_nothing_past_it(hip, world):
    """the shape of test_capacity_overflow_flag_survives_multi_tile_scan: an
    e_cap too small truncates at a destination boundary and is flagged; the
    buffers (allocated larger, e_cap passed smaller) stay untouched past it"""
    from nts.hip import LayerBuffers
    seeds = np.arange(0, 14000, dtype=np.uint32)  # 4 scan tiles; the special destinations first
    hip.reserve(V, 14000 * 10)
    dst_t = _t(seeds)
    vsz = torch.tensor([seeds.size], dtype=torch.int32, device=DEV)
    big, cap = 14000 * 10, 5000
    lay = LayerBuffers(14000, big, big, dst_t, vsz, torch.device(DEV))
    for name in ("sample_ans", "edge_dst", "row_indices"):
        lay.t[name].fill_(-1)
    lay.e_cap = cap
    hip.sample_layer(world["g"], lay, 10, 0, 2, SHARED, 0)
    torch.cuda.synchronize()
    v, e, s, ovf = lay.sizes_host()
    assert v == 14000 and 0 < e <= cap and (ovf & 1), (v, e, ovf)
    co = _np_u32(lay.column_offset)[:v + 1]
    assert e in set(co.tolist())
    assert (_np_u32(lay.sample_ans)[:e] < V).all() and (_np_u32(lay.row_indices)[:e] < s).all()
    for name in ("sample_ans", "edge_dst", "row_indices"):
        assert (_np_u32(lay.t[name])[cap:] == 0xFFFFFFFF).all(), name
    # the kept part is the restatement's
    n_dst = int(np.searchsorted(co, e))
    ref = sb.shared_layer(world["col"], world["rows"], world["idg"], world["od"], seeds[:n_dst], 10,
                          SEED, 0, 2)
    assert ref["e_size"] == e and np.array_equal(_np_u32(lay.sample_ans)[:e], ref["sample_ans"])
    # in capacity: no flag
    lay = LayerBuffers(14000, big, big, dst_t, vsz, torch.device(DEV))
    hip.sample_layer(world["g"], lay, 10, 0, 2, SHARED, 0)
    torch.cuda.synchronize()
    assert lay.sizes_host()[3] == 0
