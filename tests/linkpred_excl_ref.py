"""Target-edge exclusion and filtered negatives restated in numpy:
the reference the lp-exclude tests compare against.

Key table: the distinct 64-bit keys (dst << 32) | src of the batch's positive
edges src = pos_src[i] -> dst = pos_dst[i] (with `reverse`, of the edges turned
round as well), ascending.

Mask: a sampled edge whose (global dst, global src) is in the table gets the
coefficient 0; another edge keeps its value (had_weights) or gets 1.

Filtered negative (i, k) of head u: try t = 0 .. 15 draws the tail of
linkpred_ref.negative_tails under the counter word 0x20000000 | t; a tail w is
rejected when w == u or the graph holds u -> w or w -> u; the first accepted
one is taken, else the 16th is kept and counted as unresolved.
"""
import numpy as np

import linkpred_ref as ref
from shared_blocks import philox4x32_10

TRIES = 16


def keys(pos_src, pos_dst, reverse):
    """uint64, ascending and distinct"""
    s = np.asarray(pos_src, np.uint32).astype(np.uint64)
    d = np.asarray(pos_dst, np.uint32).astype(np.uint64)
    k = (d << np.uint64(32)) | s
    if reverse:
        k = np.concatenate([k, (s << np.uint64(32)) | d])
    return np.unique(k)


def hits(table, gdst, gsrc):
    """bool per edge: (gdst, gsrc) is in the table"""
    k = (np.asarray(gdst, np.uint32).astype(np.uint64) << np.uint64(32)) | \
        np.asarray(gsrc, np.uint32).astype(np.uint64)
    return np.isin(k, np.asarray(table, np.uint64))


def mask(w, hit, had_weights):
    """float32 weights after the mask; w: the values before it"""
    out = np.asarray(w, np.float32).copy() if had_weights else np.ones(len(hit), np.float32)
    out[hit] = np.float32(0)
    return out


def csr_rows(row_offset, n_slots):
    """the row of every CSR slot"""
    ro = np.asarray(row_offset, np.int64)
    return np.repeat(np.arange(ro.size - 1), np.diff(ro))[:n_slots]


def candidate_tails(B, K, V, seed, batch_seq, t):
    """uint32 [B, K]: try t of every negative"""
    i = np.repeat(np.arange(B, dtype=np.uint32), K)
    k = np.tile(np.arange(K, dtype=np.uint32), B)
    full = lambda x: np.full(i.shape, x & 0xFFFFFFFF, np.uint32)
    c = [k >> np.uint32(2), i, full(ref.LP_TAG | t), full(int(batch_seq))]
    key = (int(seed) & 0xFFFFFFFF, ((int(seed) >> 32) ^ (int(batch_seq) >> 32)) & 0xFFFFFFFF)
    words = np.stack(philox4x32_10(c, key), axis=1)
    x = words[np.arange(i.size), k & np.uint32(3)].astype(np.uint64)
    return ((x * np.uint64(V)) >> np.uint64(32)).astype(np.uint32).reshape(B, K)


def edge_set(src, dst):
    """the graph's edges src -> dst as a set of (src, dst)"""
    return set(zip(np.asarray(src).astype(np.int64).tolist(), np.asarray(dst).astype(np.int64).tolist()))


def filtered_tails(pos_src, K, V, seed, batch_seq, edges):
    """(uint32 [B, K] tails, the count of unresolved negatives)"""
    pos_src = np.asarray(pos_src, np.uint32)
    B = pos_src.size
    cand = np.stack([candidate_tails(B, K, V, seed, batch_seq, t) for t in range(TRIES)])
    tails = np.empty((B, K), np.uint32)
    unresolved = 0
    for i in range(B):
        u = int(pos_src[i])
        for k in range(K):
            for t in range(TRIES):
                w = int(cand[t, i, k])
                if w != u and (u, w) not in edges and (w, u) not in edges:
                    break
            else:
                unresolved += 1
            tails[i, k] = w
    return tails, unresolved


def batch(pos_src, pos_dst, K, V, seed, batch_seq, edges):
    """linkpred_ref.batch with the filtered tails, and their unresolved count"""
    pos_src = np.asarray(pos_src, np.uint32)
    pos_dst = np.asarray(pos_dst, np.uint32)
    B = pos_src.size
    tails, unresolved = filtered_tails(pos_src, K, V, seed, batch_seq, edges)
    gu = np.concatenate([pos_src, np.repeat(pos_src, K)])
    gv = np.concatenate([pos_dst, tails.reshape(-1)])
    dest = np.unique(np.concatenate([gu, gv]))
    pair_u = np.searchsorted(dest, gu).astype(np.uint32)
    pair_v = np.searchsorted(dest, gv).astype(np.uint32)
    P = gu.size
    rows = np.empty(2 * P, np.int64)
    rows[0::2] = pair_u
    rows[1::2] = pair_v
    order = np.argsort(rows, kind="stable")
    counts = np.bincount(rows, minlength=dest.size)
    inc_offset = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    return {"destination": dest.astype(np.uint32), "v_size": int(dest.size), "pair_u": pair_u,
            "pair_v": pair_v, "inc_offset": inc_offset, "inc_slot": order.astype(np.uint32),
            "gu": gu, "gv": gv, "B": B, "K": K, "P": P, "unresolved": unresolved}
