"""nts_hip_lp_exclude_keys, nts_hip_lp_mask_block and nts_hip_lp_batch_filtered
(csrc/linkpred.hip) against tests/linkpred_excl_ref.py.  Integer
work and exact 0.0f / 1.0f stores only: every comparison is bit for bit, and
the filtered batch reproduces the Philox stream (no statistical threshold)."""
import numpy as np
import pytest
import torch

import linkpred_excl_ref as xref
import linkpred_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEED = 2000
NTS_ERR_INVALID = 1
POISON = 0x7FC0DEAD
POISON64 = 0x7FC0DEAD7FC0DEAD
W_POISON = -777.5  # a weight no kernel writes


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=SEED)


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def _u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


# ---- key table --------------------------------------------------------------
def _key_case(name):
    """V, pos_src, pos_dst"""
    if name == "b1":
        return 50, [7], [9]
    if name == "repeat":  # B = 5, one positive twice
        return 64, [3, 10, 3, 63, 12], [10, 4, 10, 0, 12]
    if name == "with_reverse":  # a positive and its own reverse in the batch
        return 64, [5, 9, 20], [9, 5, 21]
    if name == "self_pair":
        return 64, [8, 8, 2], [8, 3, 2]
    if name == "edge_ids":  # 0, 2^31 and 2^32 - 1
        return 1 << 32, [0, 1 << 31, 0xFFFFFFFF, 0xFFFFFFFF, 0], [0xFFFFFFFF, 0, 1 << 31, 0xFFFFFFFF, 0]
    if name == "tile":  # past one 4,096-item sort tile, most keys repeated
        rng = np.random.default_rng(11)
        return 50, rng.integers(0, 50, 4097), rng.integers(0, 50, 4097)
    raise KeyError(name)


KEY_CASES = ["b1", "repeat", "with_reverse", "self_pair", "edge_ids", "tile"]


def _run_keys(hip, V, ps, pd, reverse, extra=3):
    B = len(ps)
    cap = (2 * B if reverse else B) + extra
    keys = torch.full((cap,), POISON64, dtype=torch.int64, device=DEV)
    n = torch.full((1,), POISON, dtype=torch.int32, device=DEV)
    hip.reserve(min(V, 1 << 20), 16 * B)
    hip.lp_exclude_keys(_i32(ps), _i32(pd), reverse, V, keys, n)
    torch.cuda.synchronize()
    return keys.cpu().numpy().view(np.uint64), int(n.cpu().numpy().view(np.uint32)[0])


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("name", KEY_CASES)
def test_key_table_equals_np_unique(hip, name, reverse):
    V, ps, pd = _key_case(name)
    want = xref.keys(ps, pd, reverse)
    got, n = _run_keys(hip, V, ps, pd, reverse)
    assert n == want.size
    assert np.array_equal(got[:n], want)
    assert (got[n:] == np.uint64(POISON64)).all(), "entries past the count were written"
    if name == "repeat" or (name in ("self_pair", "with_reverse") and reverse):
        assert n < (2 if reverse else 1) * len(ps), "the case must hold a duplicate"
    again, n2 = _run_keys(hip, V, ps, pd, reverse)
    assert n2 == n and np.array_equal(again, got)


def test_key_table_refusals_leave_the_outputs_untouched(hip):
    from nts._abi import ptr
    V, ps, pd = _key_case("repeat")
    B = len(ps)
    s, d = _i32(ps), _i32(pd)
    keys = torch.full((2 * B,), POISON64, dtype=torch.int64, device=DEV)
    n = torch.full((1,), POISON, dtype=torch.int32, device=DEV)

    def call(src=s, dst=d, B=B, reverse=1, V=V, cap=2 * B, k=keys, cnt=n):
        return hip.lib.nts_hip_lp_exclude_keys(hip.h, ptr(src), ptr(dst), B, reverse, V, cap, ptr(k), ptr(cnt))

    assert call(B=0) == NTS_ERR_INVALID
    assert call(cap=2 * B - 1) == NTS_ERR_INVALID
    assert call(reverse=0, cap=B - 1) == NTS_ERR_INVALID
    assert call(V=0) == NTS_ERR_INVALID and call(V=(1 << 32) + 1) == NTS_ERR_INVALID
    for kw in (dict(src=None), dict(dst=None), dict(k=None), dict(cnt=None)):
        assert call(**kw) == NTS_ERR_INVALID
    torch.cuda.synchronize()
    assert (keys == POISON64).all() and (n == POISON).all()
    assert call(reverse=0, cap=B) == 0  # the smallest capacity that is taken


# ---- mask -------------------------------------------------------------------
def _block_case(name):
    """destination (global ids), edges as (local dst, global src) in CSC order
    (ascending local dst), positives (src, dst), reverse"""
    if name == "no_hit":
        return [10, 11, 12], [(0, 1), (0, 2), (1, 3), (2, 1)], ([5], [10]), True
    if name == "all_hit":
        return [10, 11], [(0, 1), (0, 2), (1, 1)], ([1, 2, 1], [10, 10, 11]), False
    if name == "reverse_only":  # hit through the turned-round key alone
        return [10, 11], [(0, 1), (1, 2), (1, 3)], ([11, 10], [3, 9]), True
    if name == "multi_edge":  # the same (dst, src) sampled twice
        return [10, 11, 12], [(0, 7), (0, 7), (0, 8), (1, 7), (2, 8), (2, 8)], ([7, 8], [10, 12]), False
    if name == "hub":  # a 200-edge destination; more than one 256-thread block in all
        e = [(0, 5)] + [(1, 100 + j) for j in range(200)] + [(2, 100 + j) for j in range(150)]
        return [40, 41, 42], e, (list(range(100, 300, 3)), [41] * 67), True
    if name == "big_ids":
        d = [0x80000001, 0xFFFFFFFF, 5]
        e = [(0, 0xFFFFFFFE), (0, 0x80000000), (1, 0x80000001), (1, 0), (2, 0xFFFFFFFF), (2, 0x80000001)]
        return d, e, ([0xFFFFFFFE, 0xFFFFFFFF, 0x80000001], [0x80000001, 0x80000001, 0x7FFFFFFF]), True
    raise KeyError(name)


BLOCK_CASES = ["no_hit", "all_hit", "reverse_only", "multi_edge", "hub", "big_ids"]


def _build_block(dest, edges, csr=True, pad=(3, 5, 2), seed=0):
    """a LayerBuffers with capacities above the live sizes and sentinels past
    them, and the numpy view of its live arrays"""
    from nts.hip import LayerBuffers
    dest = np.asarray(dest, np.uint32)
    dl = np.array([e[0] for e in edges], np.int64)
    gs = np.array([e[1] for e in edges], np.uint32)
    assert (np.diff(dl) >= 0).all()
    v, e = dest.size, dl.size
    source = np.unique(gs)
    s = source.size
    ri = np.searchsorted(source, gs)
    order = np.argsort(ri, kind="stable")  # CSR slots: by source row, CSC order within a row
    row_offset = np.concatenate([[0], np.cumsum(np.bincount(ri, minlength=s))])
    v_cap, e_cap, s_cap = v + pad[0], e + pad[1], s + pad[2]
    rng = np.random.default_rng(seed)
    w_f = rng.uniform(0.1, 2.0, e).astype(np.float32)

    def padded(a, n, fill=POISON):
        out = np.full(n, fill, np.uint32)
        out[:len(a)] = a
        return out

    lay = LayerBuffers(v_cap, e_cap, s_cap, _i32(padded(dest, v_cap)), _i32([v]), DEV, csr=csr)
    t = lay.t
    t["column_offset"].copy_(_i32(padded(np.concatenate([[0], np.cumsum(np.bincount(dl, minlength=v))]), v_cap + 1)))
    t["row_indices"].copy_(_i32(padded(ri, e_cap)))
    t["sample_ans"].copy_(_i32(padded(gs, e_cap)))
    t["edge_dst"].copy_(_i32(padded(dl, e_cap)))
    t["source"].copy_(_i32(padded(source, s_cap)))
    t["sizes"].copy_(_i32([v, e, s, 0]))
    wf = np.full(e_cap, W_POISON, np.float32)
    wf[:e] = w_f
    t["edge_weight_forward"].copy_(torch.from_numpy(wf).to(DEV))
    if csr:
        t["row_offset"].copy_(_i32(padded(row_offset, s_cap + 1)))
        t["column_indices"].copy_(_i32(padded(dl[order], e_cap)))
        wb = np.full(e_cap, W_POISON, np.float32)
        wb[:e] = w_f[order]
        t["edge_weight_backward"].copy_(torch.from_numpy(wb).to(DEV))
    live = dict(dest=dest, dl=dl, gs=gs, source=source, order=order, row_offset=row_offset, w_f=w_f,
                v=v, e=e, s=s)
    return lay, live


def _expected(live, table, had):
    hit_f = xref.hits(table, live["dest"][live["dl"]], live["gs"])
    rows = xref.csr_rows(live["row_offset"], live["e"])
    hit_b = xref.hits(table, live["dest"][live["dl"][live["order"]]], live["source"][rows])
    assert np.array_equal(hit_b, hit_f[live["order"]])  # the two views agree edge for edge
    return (xref.mask(live["w_f"], hit_f, had), xref.mask(live["w_f"][live["order"]], hit_b, had),
            int(hit_f.sum()))


def _check_block(lay, live, want_f, want_b, csr=True):
    e = live["e"]
    got_f = lay.t["edge_weight_forward"].cpu().numpy()
    assert np.array_equal(got_f[:e].view(np.uint32), want_f.view(np.uint32))
    assert (got_f[e:] == np.float32(W_POISON)).all(), "weights past sizes[1] were written"
    if csr:
        got_b = lay.t["edge_weight_backward"].cpu().numpy()
        assert np.array_equal(got_b[:e].view(np.uint32), want_b.view(np.uint32))
        assert (got_b[e:] == np.float32(W_POISON)).all(), "CSR slots past the live count were written"


@pytest.mark.parametrize("had", [0, 1])
@pytest.mark.parametrize("name", BLOCK_CASES)
def test_mask_equals_the_reference_in_csc_and_csr(hip, name, had):
    dest, edges, (ps, pd), reverse = _block_case(name)
    table = xref.keys(ps, pd, reverse)
    lay, live = _build_block(dest, edges)
    want_f, want_b, count = _expected(live, table, had)
    if name == "no_hit":
        assert count == 0
    if name == "all_hit":
        assert count == live["e"]
    if name == "multi_edge":
        assert count == 4
    if name in ("hub", "big_ids", "reverse_only"):
        assert 0 < count < live["e"]
    excluded = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    hip.lp_mask_block(lay, _u64(np.concatenate([table, [np.uint64(POISON64)]])), _i32([table.size]), had,
                      excluded)
    torch.cuda.synchronize()
    _check_block(lay, live, want_f, want_b)
    assert int(excluded.item()) == 5 + count, "the count is added to"
    if not had:
        assert set(np.unique(want_f).tolist()) <= {0.0, 1.0}


def test_mask_without_csr_and_with_an_empty_table(hip):
    dest, edges, (ps, pd), reverse = _block_case("multi_edge")
    table = xref.keys(ps, pd, reverse)
    lay, live = _build_block(dest, edges, csr=False)
    want_f, _, count = _expected(live, table, 1)
    excluded = torch.zeros(1, dtype=torch.int32, device=DEV)
    hip.lp_mask_block(lay, _u64(table), _i32([table.size]), 1, excluded)
    torch.cuda.synchronize()
    _check_block(lay, live, want_f, None, csr=False)
    assert int(excluded.item()) == count
    # n_keys = 0: nothing is zeroed, whatever the table's bytes
    for had in (0, 1):
        lay, live = _build_block(dest, edges)
        want_f, want_b, _ = _expected(live, np.zeros(0, np.uint64), had)
        excluded.zero_()
        hip.lp_mask_block(lay, _u64(table), _i32([0]), had, excluded)
        torch.cuda.synchronize()
        _check_block(lay, live, want_f, want_b)
        assert int(excluded.item()) == 0 and (want_f != 0).all()


def test_mask_leaves_an_overflowed_block_alone(hip):
    dest, edges, (ps, pd), reverse = _block_case("all_hit")
    lay, live = _build_block(dest, edges)
    lay.t["sizes"].copy_(_i32([live["v"], live["e"], live["s"], 1]))
    before_f = lay.t["edge_weight_forward"].clone()
    before_b = lay.t["edge_weight_backward"].clone()
    excluded = torch.zeros(1, dtype=torch.int32, device=DEV)
    table = xref.keys(ps, pd, reverse)
    hip.lp_mask_block(lay, _u64(table), _i32([table.size]), 0, excluded)
    torch.cuda.synchronize()
    assert torch.equal(lay.t["edge_weight_forward"], before_f)
    assert torch.equal(lay.t["edge_weight_backward"], before_b)
    assert int(excluded.item()) == 0


def test_keys_then_mask_on_the_device(hip):
    dest, edges, (ps, pd), reverse = _block_case("hub")
    lay, live = _build_block(dest, edges)
    want_f, want_b, count = _expected(live, xref.keys(ps, pd, reverse), 1)
    keys = torch.full((2 * len(ps),), POISON64, dtype=torch.int64, device=DEV)
    n = torch.zeros(1, dtype=torch.int32, device=DEV)
    excluded = torch.zeros(1, dtype=torch.int32, device=DEV)
    hip.lp_exclude_keys(_i32(ps), _i32(pd), reverse, 1 << 10, keys, n)
    hip.lp_mask_block(lay, keys, n, 1, excluded)
    torch.cuda.synchronize()
    _check_block(lay, live, want_f, want_b)
    assert int(excluded.item()) == count


def test_mask_refusals_leave_the_weights_untouched(hip):
    import ctypes as C
    from nts._abi import ptr
    dest, edges, (ps, pd), reverse = _block_case("all_hit")
    lay, live = _build_block(dest, edges)
    table = _u64(xref.keys(ps, pd, reverse))
    n = _i32([table.numel()])
    excluded = torch.zeros(1, dtype=torch.int32, device=DEV)
    before_f = lay.t["edge_weight_forward"].clone()
    before_b = lay.t["edge_weight_backward"].clone()

    def call(o, k=table, cnt=n, x=excluded):
        return hip.lib.nts_hip_lp_mask_block(hip.h, C.byref(o) if o is not None else None, ptr(k), ptr(cnt),
                                             0, ptr(x))

    assert call(None) == NTS_ERR_INVALID
    for kw in (dict(k=None), dict(cnt=None), dict(x=None)):
        assert call(lay.as_struct(), **kw) == NTS_ERR_INVALID
    o = lay.as_struct()
    o.edge_weight_forward = None
    assert call(o) == NTS_ERR_INVALID
    o = lay.as_struct()
    o.edge_weight_backward = None  # row_offset without the CSR weights
    assert call(o) == NTS_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(lay.t["edge_weight_forward"], before_f)
    assert torch.equal(lay.t["edge_weight_backward"], before_b)
    assert int(excluded.item()) == 0


# ---- filtered batch ---------------------------------------------------------
def _graph(V, src, dst):
    """DeviceGraph (CSC keyed by dst, file order within a destination) and sorted_rows"""
    from nts.hip import DeviceGraph
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    order = np.argsort(dst, kind="stable")
    rows = src[order]
    col = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=V))]).astype(np.int64)
    srt = rows.copy()
    for d in range(V):
        srt[col[d]:col[d + 1]] = np.sort(rows[col[d]:col[d + 1]])
    one = torch.ones(V, dtype=torch.int32, device=DEV)
    g = DeviceGraph(V, int(src.size), torch.from_numpy(col).to(DEV), _i32(rows if rows.size else [0]), one, one)
    return g, _i32(srt if srt.size else [0])


def _filter_case(name):
    """V, graph src, graph dst, pos_src, pos_dst, K, batch_seq"""
    rng = np.random.default_rng(["dense", "hub", "k5", "empty"].index(name))
    if name == "dense":  # V = 8, most t = 0 draws are rejected
        return 8, rng.integers(0, 8, 30), rng.integers(0, 8, 30), [0, 1, 3, 4, 5, 6], [1, 3, 0, 6, 5, 2], 1, 0
    if name == "hub":  # head 2 adjacent to every vertex: unresolvable
        s = np.concatenate([rng.integers(0, 8, 10), np.full(8, 2)])
        d = np.concatenate([rng.integers(0, 8, 10), np.arange(8)])
        return 8, s, d, [2, 0, 2], [1, 5, 7], 2, 3
    if name == "k5":  # crosses a Philox word group; a batch_seq past 2^32
        return 40, rng.integers(0, 40, 500), rng.integers(0, 40, 500), rng.integers(0, 40, 20), \
            rng.integers(0, 40, 20), 5, (1 << 40) + 2
    if name == "empty":
        return 5000, [], [], rng.integers(0, 5000, 33), rng.integers(0, 5000, 33), 5, 9
    raise KeyError(name)


def _run_filtered(hip, g, srt, ps, pd, K, seq, filtered=True):
    B = len(ps)
    P = B * (1 + K)
    out = {k: torch.full((n,), POISON, dtype=torch.int32, device=DEV)
           for k, n in (("destination", 2 * P), ("v_size", 1), ("pair_u", P), ("pair_v", P),
                        ("inc_offset", 2 * P + 1), ("inc_slot", 2 * P))}
    unresolved = torch.zeros(1, dtype=torch.int32, device=DEV)
    hip.reserve(g.n_vertices, 8 * P)
    args = (out["destination"], out["v_size"], out["pair_u"], out["pair_v"], out["inc_offset"], out["inc_slot"])
    if filtered:
        hip.lp_batch_filtered(g, srt, _i32(ps), _i32(pd), K, seq, *args, unresolved)
    else:
        hip.lp_batch(_i32(ps), _i32(pd), K, g.n_vertices, seq, *args)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy().view(np.uint32) for k, v in out.items()}
    got["unresolved"] = int(unresolved.item())
    return got


@pytest.mark.parametrize("name", ["dense", "hub", "k5", "empty"])
def test_filtered_batch_equals_the_reference_byte_for_byte(hip, name):
    V, gs, gd, ps, pd, K, seq = _filter_case(name)
    g, srt = _graph(V, gs, gd)
    edges = xref.edge_set(gs, gd)
    want = xref.batch(ps, pd, K, V, SEED, seq, edges)
    B, P, v = want["B"], want["P"], want["v_size"]
    t0 = ref.negative_tails(B, K, V, SEED, seq).reshape(-1)
    redrawn = int((t0 != want["gv"][B:]).sum())
    print(f"{name}: {redrawn} of {B * K} negatives redrawn, {want['unresolved']} unresolved")
    if name == "dense":
        assert redrawn > B * K // 2
    if name == "hub":
        assert want["unresolved"] == 2 * K
    if name == "k5":
        assert redrawn > 0
    got = _run_filtered(hip, g, srt, ps, pd, K, seq)
    assert int(got["v_size"][0]) == v and got["unresolved"] == want["unresolved"]
    assert np.array_equal(got["destination"][:v], want["destination"])
    assert (got["destination"][v:] == np.uint32(POISON)).all()
    assert np.array_equal(got["pair_u"], want["pair_u"]) and np.array_equal(got["pair_v"], want["pair_v"])
    assert np.array_equal(got["inc_offset"][:v + 1], want["inc_offset"])
    assert np.array_equal(got["inc_slot"], want["inc_slot"])
    if name == "empty":  # no t = 0 candidate is rejected: the unfiltered entry's bytes
        assert redrawn == 0 and got["unresolved"] == 0
        plain = _run_filtered(hip, g, srt, ps, pd, K, seq, filtered=False)
        for k in ("destination", "v_size", "pair_u", "pair_v", "inc_offset", "inc_slot"):
            assert np.array_equal(got[k], plain[k]), k


def test_filtered_batch_refusals_leave_the_outputs_untouched(hip):
    import ctypes as C
    from nts._abi import ptr
    V, gs, gd, ps, pd, K, seq = _filter_case("dense")
    g, srt = _graph(V, gs, gd)
    P = len(ps) * (1 + K)
    s, d = _i32(ps), _i32(pd)
    bufs = [torch.full((n,), POISON, dtype=torch.int32, device=DEV) for n in (2 * P, 1, P, P, 2 * P + 1, 2 * P)]
    unresolved = torch.full((1,), POISON, dtype=torch.int32, device=DEV)

    def call(graph=g.as_struct(), rows=srt, unres=unresolved, B=len(ps), Vn=V):
        return hip.lib.nts_hip_lp_batch_filtered(
            hip.h, ptr(s), ptr(d), B, K, Vn, seq, 2 * P, *[ptr(t) for t in bufs],
            C.byref(graph) if graph is not None else None, ptr(rows), ptr(unres))

    assert call(graph=None) == NTS_ERR_INVALID
    assert call(rows=None) == NTS_ERR_INVALID
    assert call(unres=None) == NTS_ERR_INVALID
    assert call(B=0) == NTS_ERR_INVALID
    assert call(Vn=V + 1) == NTS_ERR_INVALID
    torch.cuda.synchronize()
    for t in bufs + [unresolved]:
        assert (t == POISON).all()
