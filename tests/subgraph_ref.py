"""Subgraph sampling restated in numpy: the reference the subgraph
tests compare nts_hip_random_walk and nts_hip_induced_layer against.

Walk: step t of the walk rooted at r, standing at u, moves to the in-neighbour
at CSC position mulhi32(x, deg(u)) with

    x = Philox4x32-10(counter = (0, r, 0x10000000 | t, lo32(batch_seq)),
                      key = (lo32(seed), hi32(seed) ^ hi32(batch_seq)))[0]

and stays at u when deg(u) == 0.

Induced block of a set S on destinations dst (each a member of S): column i
holds the neighbours of dst[i] that are in S, in the graph's CSC order with
their multiplicity; `source` is S, distinct and ascending; the weights, the
CSR and its edge ids follow the sampler's formulas (tests/shared_blocks.py).
"""
import numpy as np

import shared_blocks as sb

W_SUM, W_MEAN, W_NONE, W_MEAN_SAMPLED, W_UP_DEGREE = (sb.W_SUM, sb.W_MEAN, sb.W_NONE,
                                                      sb.W_MEAN_SAMPLED, sb.W_UP_DEGREE)
WALK_TAG = 0x10000000


def walk_word(roots, t, seed, batch_seq):
    """x of step t for an array of roots."""
    r = np.asarray(roots, np.uint32)
    full = lambda v: np.full(r.shape, v & 0xFFFFFFFF, np.uint32)
    c = [full(0), r, full(WALK_TAG | int(t)), full(int(batch_seq))]
    k = (int(seed) & 0xFFFFFFFF, ((int(seed) >> 32) ^ (int(batch_seq) >> 32)) & 0xFFFFFFFF)
    return sb.philox4x32_10(c, k)[0]


def random_walk(col, rows, roots, walk_len, seed, batch_seq):
    """uint32 [n, walk_len + 1]: row i the walk of roots[i], column 0 the root."""
    col = np.asarray(col, np.uint64).astype(np.int64)
    rows = np.asarray(rows, np.uint32)
    roots = np.asarray(roots, np.uint32)
    out = np.empty((roots.size, walk_len + 1), np.uint32)
    out[:, 0] = roots
    u = roots.astype(np.int64)
    for t in range(walk_len):
        beg, deg = col[u], col[u + 1] - col[u]
        x = walk_word(roots, t, seed, batch_seq).astype(np.uint64)
        pos = ((x * deg.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
        live = deg > 0
        nxt = u.copy()
        nxt[live] = rows[beg[live] + pos[live]]
        u = nxt
        out[:, t + 1] = u
    return out


def induced_layer(col, rows, in_deg, out_deg, dst, set_ids, weight_flags=W_SUM, merge=False):
    """The block `set_ids` (any order, duplicates allowed) induces on `dst`."""
    col = np.asarray(col, np.uint64).astype(np.int64)
    rows = np.asarray(rows, np.uint32)
    dst = np.asarray(dst, np.uint32)
    V = col.size - 1
    member = np.zeros(V, bool)
    member[np.asarray(set_ids, np.int64)] = True
    assert member[dst].all(), "every destination must be a member of the set"
    pieces, counts = [], np.zeros(dst.size, np.int64)
    for i, d in enumerate(dst):
        nb = rows[col[d]:col[d + 1]]
        kept = nb[member[nb]]
        pieces.append(kept)
        counts[i] = kept.size
    ans = np.concatenate(pieces).astype(np.uint32) if pieces else np.zeros(0, np.uint32)
    v = dst.size
    co = np.zeros(v + 1, np.uint32)
    np.cumsum(counts, out=co[1:])
    source = np.nonzero(member)[0].astype(np.uint32)
    index = np.zeros(V, np.uint32)
    index[source] = np.arange(source.size, dtype=np.uint32)
    ri = index[ans]
    edst = np.repeat(np.arange(v, dtype=np.uint32), counts)
    order = np.argsort(ri, kind="stable")
    ro = np.zeros(source.size + 1, np.uint32)
    np.cumsum(np.bincount(ri, minlength=source.size), out=ro[1:])
    out = dict(v_size=v, e_size=int(co[-1]), src_size=int(source.size), destination=dst,
               column_offset=co, sample_ans=ans, edge_dst=edst, source=source, row_indices=ri,
               row_offset=ro, column_indices=edst[order], csr_edge_id=order.astype(np.uint32))
    if merge:
        out["dst_local_id"] = index[dst]
    wt = weight_flags & 0xF
    if wt != W_NONE:
        cnt = counts.astype(np.uint32)
        if weight_flags & W_UP_DEGREE:
            od = np.bincount(ri, minlength=source.size).astype(np.uint32)[ri]
            idg = cnt[edst]
        else:
            od = np.asarray(out_deg, np.uint32)[ans]
            idg = np.asarray(in_deg, np.uint32)[dst][edst]
        w = sb._norm_degree(od, idg)
        if wt == W_MEAN:
            w = (w / idg.astype(np.float32)).astype(np.float32)
        if wt == W_MEAN_SAMPLED:
            w = (w / cnt[edst].astype(np.float32)).astype(np.float32)
        out["edge_weight_forward"] = w
        out["edge_weight_backward"] = w[order]
    return out


def subgraph_batch(col, rows, in_deg, out_deg, seeds, layers, walk_len, seed, batch_seq,
                   weight_flags=W_SUM, merge=False):
    """Every layer of a subgraph-sampled batch: layer 0 the seeds x S, layers
    >= 1 the square block S x S, S = the walks' ids."""
    seeds = np.asarray(seeds, np.uint32)
    S = random_walk(col, rows, seeds, walk_len, seed, batch_seq).reshape(-1)
    out, dst = [], seeds
    for _ in range(layers):
        lay = induced_layer(col, rows, in_deg, out_deg, dst, S, weight_flags, merge)
        out.append(lay)
        dst = S = lay["source"]
    return out
