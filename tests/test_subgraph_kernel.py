"""nts_hip_random_walk and nts_hip_induced_layer against the
numpy restatement of tests/subgraph_ref.py: every array np.array_equal, the
weights bit for bit.

One graph of V = 9,000 (three 4,096-vertex tiles of the byte map, so the fused
frontier compaction crosses tiles) with: vertices of in-degree 0 (the last 40);
destination 0 of degree 70 and destination 1 of degree 300 (past one and four
64-wide strides of a wave), each with every second neighbour in the set;
destination 2, which lists one source twice; a member of the set that is
nobody's neighbour (vertex 8,990: out-degree 0) and a destination with no
neighbour in the set (vertex 3).
"""
import numpy as np
import pytest
import torch

import subgraph_ref as sr
from oracle import oracle as orc
from test_hip_kernels import DEV, _assert_layers_equal, _gpu_layer_np, _graph, _np_u32, _sample_gpu, _t

pytestmark = pytest.mark.gpu
SEED = 2000
V = 9000
GUARD = 0xFFFFFFFF
LONELY, EMPTY_DST = 8990, 3


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=SEED)


@pytest.fixture(scope="module")
def world(hip):
    rng = np.random.default_rng(11)
    src, dst = [], []
    pool = np.arange(10, 8900)
    n70, n300 = rng.choice(pool, 70, replace=False), rng.choice(pool, 300, replace=False)
    src += [n70, n300]
    dst += [np.full(70, 0), np.full(300, 1)]
    twice = rng.choice(pool, 6, replace=False)
    src.append(np.concatenate([twice, twice[2:3]]))  # destination 2 lists twice[2] twice
    dst.append(np.full(7, 2))
    out3 = rng.choice(pool, 5, replace=False)  # destination 3: no neighbour will be a member
    src.append(out3)
    dst.append(np.full(5, EMPTY_DST))
    bs = rng.integers(0, 8960, 60_000)  # background: parallel edges and self loops allowed;
    bd = rng.integers(4, 8960, 60_000)  # ids >= 8960 are nobody's destination or source
    src.append(bs)
    dst.append(bd)
    src = np.concatenate(src).astype(np.uint32)
    dst = np.concatenate(dst).astype(np.uint32)
    col, rows = orc.build_csc(V, src, dst)
    od, idg = orc.degrees(V, src, dst)
    deg = np.diff(col.astype(np.int64))
    assert deg[0] == 70 and deg[1] == 300 and deg[2] == 7 and (deg[8960:] == 0).all()
    # the set: destinations 0..3, every second neighbour of 0 and 1, destination
    # 2's neighbours, a vertex nobody lists, 1,500 others — none of destination 3's
    members = np.concatenate([np.arange(4), n70[::2], n300[::2], twice, [LONELY],
                              rng.choice(np.arange(4, 8960), 1500, replace=False)])
    members = np.setdiff1d(members, out3)
    S = np.unique(members).astype(np.uint32)
    given = rng.permutation(np.concatenate([S, S[::7]])).astype(np.uint32)  # duplicates, unsorted
    return dict(g=_graph(hip, V, src, dst), col=col, rows=rows, od=od, idg=idg, S=S, given=given,
                rng=rng)


# ---- walk ----
@pytest.mark.parametrize("walk_len", [0, 1, 4])
@pytest.mark.parametrize("n", [1, 65, 257])
def test_walk_is_the_reference_bit_for_bit(hip, world, walk_len, n):
    rng = np.random.default_rng(n * 10 + walk_len)
    roots = rng.choice(8960, n + 3, replace=False).astype(np.uint32)
    roots[0] = 8995  # in-degree 0: stays put
    out = torch.full(((n + 3) * (walk_len + 1),), -1, dtype=torch.int32, device=DEV)
    hip.random_walk(world["g"], _t(roots), torch.tensor([n], dtype=torch.int32, device=DEV),
                    walk_len, 5, out)
    torch.cuda.synchronize()
    got = _np_u32(out).reshape(n + 3, walk_len + 1)
    want = sr.random_walk(world["col"], world["rows"], roots[:n], walk_len, SEED, 5)
    assert np.array_equal(got[:n], want)
    assert (got[0] == 8995).all()
    assert (got[n:] == GUARD).all()  # slots past the live count keep their guard value


def test_walk_depends_on_batch_seq_and_not_on_the_slot(hip, world):
    roots = np.arange(100, 165, dtype=np.uint32)
    n = torch.tensor([65], dtype=torch.int32, device=DEV)

    def run(r, seq):
        o = torch.empty(65 * 5, dtype=torch.int32, device=DEV)
        hip.random_walk(world["g"], _t(r), n, 4, seq, o)
        torch.cuda.synchronize()
        return _np_u32(o).reshape(65, 5)

    a, b, c = run(roots, 1), run(roots, 1), run(roots, 2)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(run(roots[::-1].copy(), 1), a[::-1])
    hi = run(roots, (7 << 32) | 1)  # the high half of batch_seq is in the key
    assert np.array_equal(hi, sr.random_walk(world["col"], world["rows"], roots, 4, SEED, (7 << 32) | 1))
    assert not np.array_equal(hi, a)


# ---- induced layer ----
def _buffers(dst, v_cap, e_cap, s_cap, wt, slack=0, csr=True):
    """a layer's arrays, `slack` guard words past every capacity, all poisoned"""
    from nts.hip import LayerBuffers
    lay = LayerBuffers(v_cap + slack, e_cap + slack, s_cap + slack, _t(dst),
                       torch.tensor([dst.size], dtype=torch.int32, device=DEV), torch.device(DEV),
                       csr=csr, weights=(wt & 0xF) != sr.W_NONE, merge=True)
    for k, t in lay.t.items():
        if t is not None and k != "sizes":
            t.view(torch.int32).fill_(-1)
    lay.v_cap, lay.e_cap, lay.s_cap = v_cap, e_cap, s_cap
    return lay


def _induced(hip, w, dst, wt, given=None, e_cap=None, slack=0):
    given = w["given"] if given is None else given
    ref = sr.induced_layer(w["col"], w["rows"], w["idg"], w["od"], dst, given, wt, merge=True)
    lay = _buffers(dst, dst.size, ref["e_size"] if e_cap is None else e_cap, ref["src_size"], wt,
                   slack)
    hip.induced_layer(w["g"], lay, _t(given),
                      torch.tensor([given.size], dtype=torch.int32, device=DEV), wt)
    torch.cuda.synchronize()
    return lay, ref


def _layer_np(lay):
    out = _gpu_layer_np(lay)
    out["edge_dst"] = _np_u32(lay.edge_dst)[:out["e_size"]]
    return out


def _rect_dst(w):
    """a strict subset of the set, in non-ascending order, the special destinations in it"""
    S = w["S"]
    rest = np.random.default_rng(3).permutation(S[S >= 4])[:300]
    return np.concatenate([rest[:150], [1, 3, 0, 2, LONELY], rest[150:]]).astype(np.uint32)


WEIGHTS = [sr.W_SUM, sr.W_MEAN, sr.W_MEAN_SAMPLED, sr.W_NONE, sr.W_SUM | sr.W_UP_DEGREE]


@pytest.mark.parametrize("wt", WEIGHTS, ids=[f"w{w:#x}" for w in WEIGHTS])
@pytest.mark.parametrize("shape", ["square", "rect"])
def test_induced_block_equals_the_reference(hip, world, shape, wt):
    dst = world["S"] if shape == "square" else _rect_dst(world)
    lay, ref = _induced(hip, world, dst, wt)
    got = _layer_np(lay)
    _assert_layers_equal([got], [ref])
    assert np.array_equal(got["edge_dst"], ref["edge_dst"])
    for k in ("edge_weight_forward", "edge_weight_backward"):
        if k in ref:  # bit for bit
            assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), k
    assert ("edge_weight_forward" in got) == ((wt & 0xF) != sr.W_NONE)
    assert np.array_equal(got["source"], world["S"])  # the whole set, LONELY included
    assert LONELY in got["source"] and LONELY not in got["sample_ans"]
    if shape == "square":
        assert np.array_equal(got["dst_local_id"], np.arange(dst.size))
    co = got["column_offset"].astype(np.int64)
    at = {int(d): i for i, d in enumerate(dst)}
    assert co[at[EMPTY_DST] + 1] == co[at[EMPTY_DST]]  # no neighbour in S: an empty column
    assert co[at[0] + 1] - co[at[0]] >= 35 and co[at[1] + 1] - co[at[1]] >= 150
    two = got["sample_ans"][co[at[2]]:co[at[2] + 1]]
    assert two.size == 7 and np.unique(two).size == 6  # the neighbour listed twice is kept twice


def test_overflow_sets_the_flag_and_leaves_the_guard_words(hip, world):
    dst = _rect_dst(world)
    wt = sr.W_SUM
    full, ref = _induced(hip, world, dst, wt, slack=8)
    assert full.sizes_host() == (dst.size, ref["e_size"], ref["src_size"], 0)
    short, _ = _induced(hip, world, dst, wt, e_cap=ref["e_size"] - 1, slack=8)
    v, e, s, ovf = short.sizes_host()
    co = ref["column_offset"]
    assert (ovf & 1) and v == dst.size and s == ref["src_size"]
    assert e == int(co[np.searchsorted(co, ref["e_size"] - 1, side="right") - 1]) < ref["e_size"]
    assert np.array_equal(_np_u32(short.sample_ans)[:e], ref["sample_ans"][:e])
    # the cut destinations read as empty columns: no offset points past e_size
    assert np.array_equal(_np_u32(short.column_offset)[:v + 1], np.minimum(co, e))
    assert np.array_equal(_np_u32(short.row_indices)[:e], ref["row_indices"][:e])
    for lay, ecap in ((full, ref["e_size"]), (short, ref["e_size"] - 1)):
        past = dict(column_offset=v + 1, source=s, row_offset=s + 1, dst_local_id=v)
        for k in ("row_indices", "sample_ans", "edge_dst", "column_indices", "csr_edge_id",
                  "edge_weight_forward", "edge_weight_backward"):
            past[k] = ecap
        for k, n in past.items():
            assert (_np_u32(lay.t[k].view(torch.int32))[n:] == GUARD).all(), k


def test_two_calls_give_the_same_bytes(hip, world):
    a, _ = _induced(hip, world, world["S"], sr.W_MEAN | sr.W_UP_DEGREE, slack=4)
    b, _ = _induced(hip, world, world["S"], sr.W_MEAN | sr.W_UP_DEGREE, slack=4)
    for k, t in a.t.items():
        if t is not None:
            assert torch.equal(t.view(torch.int32), b.t[k].view(torch.int32)), k


def test_the_byte_map_is_left_clear(hip, world):
    """a plain sampled batch before and after an induced call: identical blocks"""
    seeds = np.arange(0, 600, dtype=np.uint32)
    run = lambda: [_gpu_layer_np(l) for l in _sample_gpu(hip, world["g"], seeds, [10, 5], 0, 5)]
    before = run()
    _induced(hip, world, _rect_dst(world), sr.W_SUM)
    short = sr.induced_layer(world["col"], world["rows"], world["idg"], world["od"], world["S"],
                             world["given"])["e_size"] - 1
    _induced(hip, world, world["S"], sr.W_SUM, e_cap=short)  # an overflowing call clears it too
    after = run()
    for x, y in zip(before, after):
        for k in x:
            assert np.array_equal(x[k], y[k]), k


@pytest.mark.parametrize("case", ["null-set", "null-set-size", "omit_map"])
def test_invalid_arguments_write_nothing(hip, world, case):
    dst = _rect_dst(world)
    lay = _buffers(dst, dst.size, 4000, world["S"].size, sr.W_SUM)
    lay.t["sizes"].fill_(-1)
    given = _t(world["given"])
    n = torch.tensor([world["given"].size], dtype=torch.int32, device=DEV)
    if case == "omit_map":
        lay.omit_map = torch.zeros(V, dtype=torch.int32, device=DEV)
        lay.omit_loc = torch.zeros(V, dtype=torch.int32, device=DEV)
    args = dict(set_ids=None if case == "null-set" else given,
                set_size=None if case == "null-set-size" else n)
    with pytest.raises(RuntimeError, match="nts_hip error 1"):
        hip.induced_layer(world["g"], lay, args["set_ids"], args["set_size"], sr.W_SUM)
    torch.cuda.synchronize()
    for k, t in lay.t.items():
        if t is not None:
            assert (t.view(torch.int32) == -1).all(), k
