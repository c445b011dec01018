"""Edge-weighted neighbour selection (nts_hip_sample_layer_weighted)
restated in numpy: the reference the weighted-sampling tests compare against.

For a layer call (seed, layer, batch_seq), position p of destination d's CSC
list, whose edge carries the weight w > 0, owns

    x   = word p of the Philox stream (d, layer | 0x40000000, batch_seq), i.e.
          Philox4x32-10(counter = (p >> 2, d, layer | 0x40000000, lo32(batch_seq)),
                        key = (lo32(seed), hi32(seed) ^ hi32(batch_seq)))[p & 3]
    u   = ((x >> 9) + 0.5) * 2^-23          (a 24-bit value strictly inside (0, 1))
    key = -log2(u) / w                      (an Exp(1) variate, in bits, over w)

and a destination with deg > fanout keeps the `fanout` positions with the
smallest (key, p), written in ascending position (Efraimidis-Spirakis:
successive sampling without replacement with probability proportional to w).
Every other destination copies its list.  The device computes the key in fp32
and orders by (float_as_uint(key) << 32) | p; here the key is float64, and the
selection takes whichever keys it is given.  The rest of a layer is
shared_blocks.layer_from_selection, the default sampler's definition.
"""
import itertools

import numpy as np

import shared_blocks as sb
from shared_blocks import W_MEAN, W_NONE, W_SUM, W_UP_DEGREE, layer_from_selection  # noqa: F401

LAYER_BIT = 0x40000000
W_MIN, W_MAX = 2.0 ** -60, 2.0 ** 60


def philox_word(seed, d, layer, batch_seq, idx):
    """Word idx of the Philox stream of (d, layer, batch_seq); d and idx arrays
    of one shape (or scalars), layer with its domain bit already set."""
    d, idx = np.broadcast_arrays(np.asarray(d, np.uint32), np.asarray(idx, np.uint32))
    full = lambda x: np.full(d.shape, x & 0xFFFFFFFF, np.uint32)
    c = [idx >> np.uint32(2), d, full(int(layer)), full(int(batch_seq))]
    k = (int(seed) & 0xFFFFFFFF, ((int(seed) >> 32) ^ (int(batch_seq) >> 32)) & 0xFFFFFFFF)
    r = np.stack(sb.philox4x32_10(c, k))
    return np.take_along_axis(r, (idx & np.uint32(3)).astype(np.int64)[None], 0)[0]


def uniforms(seed, d, layer, batch_seq, positions):
    """u of the given positions of destination(s) d, float64 (exact)."""
    x = philox_word(seed, d, int(layer) | LAYER_BIT, batch_seq, positions)
    return ((x >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def keys64(seed, d, layer, batch_seq, weights):
    """The float64 keys of one destination's list (weights in CSC order)."""
    w = np.asarray(weights, np.float64)
    return -np.log2(uniforms(seed, d, layer, batch_seq, np.arange(w.size))) / w


def select_positions(keys, n):
    """The kept positions, ascending: the n smallest (key, position) pairs.
    `keys`: float64 keys or the device's uint32 key bits (positive floats order
    as their bit patterns)."""
    keys = np.asarray(keys)
    if n >= keys.size:
        return np.arange(keys.size, dtype=np.int64)
    return np.sort(np.lexsort((np.arange(keys.size), keys))[:n])


def inclusion_probabilities(weights, n):
    """Exact inclusion probability of every item under successive sampling
    without replacement of n items with probability proportional to weight:
    every ordered pick enumerated."""
    w = np.asarray(weights, np.float64)
    out = np.zeros(w.size)
    for picks in itertools.permutations(range(w.size), n):
        p, left = 1.0, w.sum()
        for i in picks:
            p *= w[i] / left
            left -= w[i]
        out[list(picks)] += p
    return out


def weighted_layer(col, rows, in_deg, out_deg, dst, fanout, keys_of, weight_flags=W_SUM,
                   merge=False):
    """One hop.  keys_of(i, d, beg, deg) -> the keys (float64, or the device's
    bits) of every position of destination dst[i] = d."""
    col = np.asarray(col, np.uint64)
    rows = np.asarray(rows, np.uint32)
    dst = np.asarray(dst, np.uint32)
    V = col.size - 1
    deg = (col[dst.astype(np.int64) + 1] - col[dst.astype(np.int64)]).astype(np.int64)
    counts = deg if fanout < 0 else np.minimum(deg, fanout)
    pieces = []
    for i in range(dst.size):
        beg, dg, n = int(col[dst[i]]), int(deg[i]), int(counts[i])
        nb = rows[beg:beg + dg]
        pieces.append(nb if n >= dg else nb[select_positions(keys_of(i, int(dst[i]), beg, dg), n)])
    ans = np.concatenate(pieces) if pieces else np.zeros(0, np.uint32)
    return layer_from_selection(dst, counts, ans, in_deg, out_deg, V, weight_flags, merge)


def weighted_layer64(col, rows, in_deg, out_deg, edge_prob, dst, fanout, seed, layer, batch_seq,
                     weight_flags=W_SUM, merge=False):
    """One hop with the float64 keys of this file."""
    ep = np.asarray(edge_prob, np.float64)
    keys_of = lambda i, d, beg, dg: keys64(seed, d, layer, batch_seq, ep[beg:beg + dg])
    return weighted_layer(col, rows, in_deg, out_deg, dst, fanout, keys_of, weight_flags, merge)


def csc_edge_prob(dst, edge_weight):
    """edge_prob of a graph built from an edge list: the value of file edge i at
    that edge's CSC position (the stable order by destination)."""
    return np.asarray(edge_weight, np.float32)[np.argsort(np.asarray(dst, np.uint32), kind="stable")]
