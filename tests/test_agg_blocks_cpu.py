"""tests/agg_blocks.py itself: the block holds the degrees it promises, its CSR
is the stable transpose, the widths reach every launch cell, and its references
agree with the CPU oracle on a Cora-sampled layer."""
import numpy as np
import pytest

import agg_blocks as ab
from oracle import oracle as orc


def test_block_degrees_and_transpose():
    B = ab.make_block()
    v, s, e = B["v"], B["s"], B["e"]
    co, ro = B["column_offset"].astype(np.int64), B["row_offset"].astype(np.int64)
    assert co[0] == ro[0] == 0 and co[-1] == ro[-1] == e
    deg, ln = np.diff(co), np.diff(ro)
    assert set(ab.SPECIAL_DEGREES) <= set(deg.tolist())
    assert set(ab.SPECIAL_DEGREES) <= set(ln.tolist())
    rest = sorted(deg.tolist())
    for x in ab.SPECIAL_DEGREES:
        rest.remove(x)
    assert 1 <= min(rest) and max(rest) <= 11
    for r, n in ab.LONG_BLOCK.items():  # one block of long rows at every lane-group width
        assert ln[r] == n > ab.k_long_row(8)
    assert len({r // 4 for r in ab.LONG_BLOCK}) == 1 and len(ab.LONG_BLOCK) == ab.K_AGG_THREADS // 64
    assert B["row_indices"].max() < s and B["column_indices"].max() < v
    # the stable transpose: CSR slots sorted by (source, CSC edge id)
    ceid = B["csr_edge_id"].astype(np.int64)
    assert np.array_equal(np.sort(ceid), np.arange(e))
    src_of_slot = np.repeat(np.arange(s), ln)
    assert np.array_equal(B["row_indices"][ceid], src_of_slot)
    assert np.array_equal(B["column_indices"], np.repeat(np.arange(v), deg)[ceid])
    for r in range(s):
        assert np.all(np.diff(ceid[ro[r]:ro[r + 1]]) > 0)
    assert np.array_equal(B["weight_backward"], B["weight"][ceid])
    assert (B["weight"] > 0).any() and (B["weight"] < 0).any()
    # the root pair's maps
    dl = B["dst_local_id"].astype(np.int64)
    assert len(set(dl.tolist())) == v and dl.max() < s
    assert np.array_equal(B["src_dst"][dl], np.arange(v))
    assert (B["src_dst"] == ab.NOT_CACHED).sum() == s - v
    assert len(set(B["src_map"].tolist())) == s and B["src_map"].max() < ab.N_TABLE


def test_widths_reach_every_cell():
    shapes = [(8, 1), (16, 1), (32, 1)] + [(64, n) for n in range(1, 9)]
    want = {(vec, lpd, nch) for vec in (1, 2, 4) for lpd, nch in shapes}
    table = ab.cell_table()
    for en in ab.ENTRIES:
        if en in ab.FLAT_ENTRIES or en in ("fwd_act_bits", "csr_bwd_postmask_bits",
                                           "csr_bwd_colmax", "fwd_cached"):
            continue
        cells = {k for (e2, k) in table if e2 == en}
        assert want <= {k[:3] for k in cells}, en
        assert {1, 2, 3} <= {k[4] for k in cells}, en  # c0 rounds
        if en in ab._PAD:  # the partial last vector, on one chunk and on several
            assert {(4, 1), (4, 2), (4, 3)} <= {(k[0], k[3]) for k in cells}, en
            assert {1, 2, 3} <= {k[3] for k in cells if k[0] == 4 and k[2] > 1}, en
    # the bits pair: every shape it supports up to 512 float4; colmax: up to 512 columns
    for en in ("fwd_act_bits", "csr_bwd_postmask_bits"):
        assert {(4, 32, 1)} | {(4, 64, n) for n in range(1, 9)} <= {k[:3] for (e2, k) in table if e2 == en}
    cm = {k for (e2, k) in table if e2 == "csr_bwd_colmax"}
    assert {(8, 1), (16, 1), (32, 1), (64, 1), (64, 2)} <= {k[1:3] for k in cm}
    assert {1, 2, 3, 4} <= {k[3] for k in cm}
    # the widths the cells were listed for
    assert ab.cell(513, [(0, 513), (0, 513)], True)["rounds"] == 2
    assert ab.cell(2052, [(0, 2052), (0, 2052)], True) | dict(u=0, long_row=0) == dict(
        vec=4, nv=513, last_valid=4, lpd=64, nch=8, rounds=2, u=0, long_row=0, gpb=4)
    assert ab.cell(1433, [(0, 1433), (0, 1433)], True)["rounds"] == 3
    assert ab.cell(602, [(0, 640), (0, 640)], True) | dict(u=0) == dict(
        vec=4, nv=151, last_valid=2, lpd=64, nch=3, rounds=1, u=0, long_row=20, gpb=4)
    print("\n" + ab.format_cell_table())


def test_references_agree_with_oracle(golden):
    from nts import dataloader
    src, dst = dataloader.read_edge_file(golden / "cora" / "cora.2708.edge.self")
    V = 2708
    col, rows = orc.build_csc(V, src, dst)
    out_d, in_d = orc.degrees(V, src, dst)
    o = orc.Sampler(col, rows, in_d, out_d, [25, 10], rng_mode=orc.RNG_PHILOX,
                    order_mode=orc.ORDER_DRAW)
    l0, l1 = o.sample(np.arange(0, V, 29, dtype=np.uint32))
    rng = np.random.default_rng(5)
    F = 7
    for lay in (l0, l1):
        X = rng.standard_normal((lay["src_size"], F)).astype(np.float32)
        G = rng.standard_normal((lay["v_size"], F)).astype(np.float32)
        for ref, off, idx, w, Z in (
                (orc.fuse_fwd(lay, X, out_d, in_d), lay["column_offset"], lay["row_indices"],
                 lay["edge_weight_forward"], X),
                (orc.fuse_bwd(lay, G, out_d, in_d), lay["row_offset"], lay["column_indices"],
                 lay["edge_weight_backward"], G)):
            assert np.array_equal(ab.agg32(off, idx, w, Z), ref)  # the oracle's order
            S, A = ab.agg64(off, idx, w, Z)
            bound = ab.err_bound(A, np.diff(off.astype(np.int64)), 0)
            assert (np.abs(ref.astype(np.float64) - S) <= bound).all()
            # pieces: a threshold above every row is the serial order; below, within the bound
            assert np.array_equal(ab.agg32_pieces(off, idx, w, Z, 1 << 30, 4), ref)
            P = ab.agg32_pieces(off, idx, w, Z, 2, 4)
            assert (np.abs(P.astype(np.float64) - S) <= bound).all()
