"""nts_hip_lp_rank (csrc/lprank.hip) against tests/linkpred_rank_ref.py.

Exact cases: integer embeddings in [-4, 4], so every fp32 partial sum is exact
for D <= 1024 (|s| <= 16,384) and the three count arrays must equal the
reference's bit for bit.  Float case: N(0, 1) embeddings inside the reference's
error band.  Every case pads the rows with NaN, keeps NaN rows past n_rows and
pre-fills the outputs with a poison value."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import linkpred_rank_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NTS_ERR_INVALID = 1
POISON = 0x7FC0DEAD
TILE = 128  # the kernel's block tile, in queries and in candidates

DIMS = [1, 3, 4, 64, 130, 1024]
SHAPES = [(1, 1), (3, 5), (65, 33), (257, 130), (1000, 130)]


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=2000)


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def _u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def _table(H, pad=None, extra=2):
    """H in a [n_rows + extra, D + pad] buffer: NaN in the pad and in the rows
    past n_rows.  pad None: 4 where D % 4 == 0 (the float4 loads), else 3."""
    n, D = H.shape
    pad = pad or (4 if D % 4 == 0 else 3)
    buf = np.full((n + extra, D + pad), np.nan, np.float32)
    buf[:n, :D] = H
    return torch.from_numpy(buf).to(DEV)[:, :D]  # stride(0) = D + pad


def _run(hip, H, heads, tails, cand=None, adj=None, pad=None):
    n_rows, D = H.shape
    M = len(heads)
    out = [torch.full((M,), POISON, dtype=torch.int32, device=DEV) for _ in range(3)]
    t = _table(H, pad)
    assert t.stride(0) > D
    hip.lp_rank(t, D, n_rows, _i32(heads), _i32(tails), *out,
                cand=None if cand is None else _i32(cand),
                adj_offset=None if adj is None else _u64(adj[0]),
                adj_sorted=None if adj is None else _i32(adj[1]))
    torch.cuda.synchronize()
    return [o.cpu().numpy().view(np.uint32).astype(np.int64) for o in out]


@functools.lru_cache(maxsize=None)
def _queries(n_rows, M):
    """heads, tails, the graph (goff, srows).  Heads repeat, query 1 has u == v
    (query 0 when M == 1), and with >= 3 rows query 0 is (0, 1) with the edge
    0 -> 2 in the graph: row 2 is made a bit copy of row 1 by _embedding, a tie
    that the filter removes.  The graph holds both directions of some pairs and
    a self loop."""
    rng = np.random.default_rng(1000 * n_rows + M)
    heads = rng.integers(0, n_rows, M)
    heads[M // 2:] = heads[:M - M // 2]  # repeats
    tails = rng.integers(0, n_rows, M)
    if n_rows >= 3:
        heads[0], tails[0] = 0, 1
    heads[min(1, M - 1)] = tails[min(1, M - 1)]
    n_e = 4 * n_rows
    src, dst = rng.integers(0, n_rows, n_e), rng.integers(0, n_rows, n_e)
    src = np.concatenate([src, dst[: n_e // 2], [n_rows - 1]])  # reverses and a self loop
    dst = np.concatenate([dst, src[: n_e // 2], [n_rows - 1]])
    if n_rows >= 3:
        src, dst = np.append(src, 0), np.append(dst, 2)
    return heads, tails, ref.sorted_adj(n_rows, src, dst)


@functools.lru_cache(maxsize=None)
def _embedding(n_rows, D):
    H = np.random.default_rng(7 * n_rows + D).integers(-4, 5, (n_rows, D)).astype(np.float32)
    if n_rows >= 3:
        H[2] = H[1]  # a bit copy of query 0's true tail
    if n_rows >= 65:
        H[64] = H[1]
    return H


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("n_rows,M", SHAPES)
@pytest.mark.parametrize("D", DIMS)
def test_exact_counts(hip, D, n_rows, M, filtered):
    heads, tails, adj = _queries(n_rows, M)
    H = _embedding(n_rows, D)
    want = ref.counts(H, heads, tails, None, adj if filtered else None)
    # the features this case exists for, on the reference
    assert (heads == tails).any() and np.unique(heads).size < max(M, 2)
    if n_rows >= 3:
        free = ref.counts(H, heads, tails, None, None)
        assert free[1][0] >= 1, "query 0 must tie with the copy of its tail"
        if filtered:  # the copy (s == s_pos) is the head's neighbour: the filter takes it
            assert ref.blocked(adj, 0, 2) and want[1][0] < free[1][0]
            assert (want[2] < free[2]).any()
    if (n_rows, M) in ((257, 130), (1000, 130)):
        assert M % TILE and M > TILE and n_rows % TILE and n_rows > TILE
    got = _run(hip, H, heads, tails, None, adj if filtered else None)
    for name, g, w in zip(("greater", "equal", "n_valid"), got, want):
        assert np.array_equal(g, w), name


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("n_cand", [1, 63, 300])
def test_candidate_list_with_repeats(hip, n_cand, filtered):
    n_rows, M, D = 257, 130, 64
    heads, tails, adj = _queries(n_rows, M)
    H = _embedding(n_rows, D)
    rng = np.random.default_rng(n_cand)
    cand = rng.integers(0, n_rows, n_cand)
    cand[0] = tails[0]  # the true tail of query 0 inside the list
    if n_cand >= 63:
        cand[1:7] = [2, 2, 64, tails[0], cand[10], cand[10]]  # repeats; copies of the tail
    want = ref.counts(H, heads, tails, cand, adj if filtered else None)
    assert want[2][0] <= n_cand - (1 if n_cand == 1 else 2), "the true tail never competes"
    if n_cand >= 63:
        assert np.unique(cand).size < n_cand
        assert ref.counts(H, heads, tails, cand, None)[1][0] >= 3  # 2, 2 and 64 tie
    if n_cand == 300:
        assert n_cand % TILE and n_cand > TILE
    # (pad 3: D % 4 == 0 on rows that are not 16-byte aligned, the scalar loads)
    got = _run(hip, H, heads, tails, cand, adj if filtered else None, pad=3)
    for name, g, w in zip(("greater", "equal", "n_valid"), got, want):
        assert np.array_equal(g, w), name


@functools.lru_cache(maxsize=None)
def _float_case(D, V, M):
    rng = np.random.default_rng(D + V + M)
    H = rng.standard_normal((V, D)).astype(np.float32)
    heads, tails = rng.integers(0, V, M), rng.integers(0, V, M)
    return H, heads, tails, ref.bands(H, heads, tails, None, None)


@pytest.mark.parametrize("D,V,M", [(64, 1000, 130), (130, 1000, 130), (1024, 300, 40)])
def test_float_counts_inside_the_band(hip, D, V, M):
    H, heads, tails, (g_lo, g_hi, ge_lo, ge_hi, n_valid, n_amb) = _float_case(D, V, M)
    print(f"ambiguous: {n_amb} of {M * V} ({n_amb / (M * V):.2e})")
    assert n_amb <= 0.01 * M * V, "the band must not be able to hide a broken kernel"
    greater, equal, valid = _run(hip, H, heads, tails)
    print(f"greater - lo: max {int((greater - g_lo).max())}, hi - greater: min "
          f"{int((g_hi - greater).min())}, equal: sum {int(equal.sum())}")
    assert np.array_equal(valid, n_valid)
    assert (g_lo <= greater).all() and (greater <= g_hi).all()
    assert (ge_lo <= greater + equal).all() and (greater + equal <= ge_hi).all()


def test_two_calls_give_the_same_bytes(hip):
    H, heads, tails, _ = _float_case(130, 1000, 130)
    _, _, adj = _queries(1000, 130)
    for a in (None, adj):
        one, two = _run(hip, H, heads, tails, None, a), _run(hip, H, heads, tails, None, a)
        for x, y in zip(one, two):
            assert x.tobytes() == y.tobytes()


def test_refusals_leave_the_outputs_alone(hip):
    n_rows, D, M = 65, 64, 33
    heads, tails, adj = _queries(n_rows, M)
    t = _table(_embedding(n_rows, D))
    h, v = _i32(heads), _i32(tails)
    goff, srows = _u64(adj[0]), _i32(adj[1])
    out = [torch.full((M,), POISON, dtype=torch.int32, device=DEV) for _ in range(3)]
    p = lambda x: None if x is None else x.data_ptr()
    U64, U32 = C.c_uint64, C.c_uint32

    def call(H=t, D=D, qh=h, qt=v, M=M, go=None, sr=None, o=out):
        return hip.lib.nts_hip_lp_rank(hip.h, p(H), U64(t.stride(0)), U32(D), U32(n_rows), p(qh),
                                       p(qt), U32(M), None, U64(0), p(go), p(sr), p(o[0]), p(o[1]),
                                       p(o[2]))

    bad = [dict(D=0), dict(D=1025), dict(M=0), dict(H=None), dict(qh=None), dict(qt=None),
           dict(o=[None, out[1], out[2]]), dict(o=[out[0], None, out[2]]),
           dict(o=[out[0], out[1], None]), dict(go=goff), dict(sr=srows)]
    for kw in bad:
        assert call(**kw) == NTS_ERR_INVALID, kw
    torch.cuda.synchronize()
    for o in out:
        assert (o.cpu().numpy().view(np.uint32) == POISON).all()
    assert call(go=goff, sr=srows) == 0  # the same arguments, complete
    torch.cuda.synchronize()
    assert (out[2].cpu().numpy().view(np.uint32) != POISON).all()
