"""Link prediction restated in numpy / float64: the reference the
link-prediction tests compare against.

Negative (i, k) of a batch keeps the head pos_src[i]; its tail is

    x    = word k % 4 of Philox4x32-10(counter = (k // 4, i, 0x20000000, lo32(batch_seq)),
                                       key = (lo32(seed), hi32(seed) ^ hi32(batch_seq)))
    tail = (x * V) >> 32

(the sampler's counter layout under a layer tag of its own).  Pairs: p < B the
positives, then B + i K + k.  The seed set is the ascending distinct endpoint
ids; pair_u / pair_v index it; the incidence CSR lists, per seed row and in
ascending order, the slots 2p (u-end) and 2p + 1 (v-end) that sit on it.
"""
import numpy as np

from shared_blocks import philox4x32_10

LP_TAG = 0x20000000


def negative_tails(B, K, V, seed, batch_seq):
    """uint32 [B, K]"""
    i = np.repeat(np.arange(B, dtype=np.uint32), K)
    k = np.tile(np.arange(K, dtype=np.uint32), B)
    full = lambda x: np.full(i.shape, x & 0xFFFFFFFF, np.uint32)
    c = [k >> np.uint32(2), i, full(LP_TAG), full(int(batch_seq))]
    key = (int(seed) & 0xFFFFFFFF, ((int(seed) >> 32) ^ (int(batch_seq) >> 32)) & 0xFFFFFFFF)
    words = np.stack(philox4x32_10(c, key), axis=1)  # [B K, 4]
    x = words[np.arange(i.size), k & np.uint32(3)].astype(np.uint64)
    return ((x * np.uint64(V)) >> np.uint64(32)).astype(np.uint32).reshape(B, K)


def batch(pos_src, pos_dst, K, V, seed, batch_seq):
    """dict of destination, v_size, pair_u, pair_v, inc_offset [v_size + 1],
    inc_slot [2 P], and the global ends gu / gv of every pair"""
    pos_src = np.asarray(pos_src, np.uint32)
    pos_dst = np.asarray(pos_dst, np.uint32)
    B = pos_src.size
    tails = negative_tails(B, K, V, seed, batch_seq)
    gu = np.concatenate([pos_src, np.repeat(pos_src, K)])
    gv = np.concatenate([pos_dst, tails.reshape(-1)])
    dest = np.unique(np.concatenate([gu, gv]))  # ascending, distinct
    pair_u = np.searchsorted(dest, gu).astype(np.uint32)
    pair_v = np.searchsorted(dest, gv).astype(np.uint32)
    P = gu.size
    rows = np.empty(2 * P, np.int64)
    rows[0::2] = pair_u
    rows[1::2] = pair_v
    order = np.argsort(rows, kind="stable")  # each row's slots ascending
    counts = np.bincount(rows, minlength=dest.size)
    inc_offset = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    return {"destination": dest.astype(np.uint32), "v_size": int(dest.size), "pair_u": pair_u,
            "pair_v": pair_v, "inc_offset": inc_offset, "inc_slot": order.astype(np.uint32),
            "gu": gu, "gv": gv, "B": B, "K": K, "P": P}


def scores(H, pair_u, pair_v):
    H = np.asarray(H, np.float64)
    return (H[pair_u] * H[pair_v]).sum(1)


def loss_and_grad(H, b):
    """float64: scores, the mean sigmoid BCE (stable form), dH over the
    incidence lists"""
    H = np.asarray(H, np.float64)
    s = scores(H, b["pair_u"], b["pair_v"])
    P, B = b["P"], b["B"]
    y = (np.arange(P) < B).astype(np.float64)
    loss = (np.maximum(s, 0) - s * y + np.log1p(np.exp(-np.abs(s)))).mean()
    g = (1.0 / (1.0 + np.exp(-s)) - y) / P
    dH = np.zeros_like(H)
    for r in range(b["v_size"]):
        for slot in b["inc_slot"][b["inc_offset"][r]:b["inc_offset"][r + 1]]:
            p = int(slot) >> 1
            other = b["pair_u"][p] if (slot & 1) else b["pair_v"][p]
            dH[r] += g[p] * H[other]
    return s, loss, dH


def ranks(s, B, K):
    """rank_i = 1 + #{k : score(neg i, k) >= score(pos i)}"""
    neg = np.asarray(s[B:]).reshape(B, K)
    return 1 + (neg >= np.asarray(s[:B])[:, None]).sum(1)


def mrr_counter(s, B, K):
    """the device counter's first word: 1 / rank in fp32, consecutive runs of 16
    positives summed ascending into one partial each, the partials ascending"""
    rr = (np.float32(1) / ranks(s, B, K).astype(np.float32)).astype(np.float32)
    total = np.float32(0)
    for b0 in range(0, B, 16):
        part = np.float32(0)
        for x in rr[b0:b0 + 16]:
            part = np.float32(part + x)
        total = np.float32(total + part)
    return total
