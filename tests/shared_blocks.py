"""Shared-variate neighbour selection (NTS_RNG_PHILOX_SHARED)
restated in numpy: the reference the shared-sampling tests compare against.

For a layer call (seed, layer, batch_seq) every global source id s owns one
32-bit word

    r(s) = Philox4x32-10(counter = (0, s, layer | 0x80000000, lo32(batch_seq)),
                         key = (lo32(seed), hi32(seed) ^ hi32(batch_seq)))[0]

and a destination with deg > fanout keeps the `fanout` positions p of its
neighbour list with the smallest 64-bit key (r(list[p]) << 32) | p, written in
ascending position.  Every other destination copies its list.  The rest of a
layer (ascending unique `source`, relabelled `row_indices`, weights, the CSR
with `csr_edge_id`) follows the sampler's definition (oracle/ref_cpu.cpp does
not take a selection, so it is restated here from the same formulas).
"""
import numpy as np

W_SUM, W_MEAN, W_NONE, W_MEAN_SAMPLED = 0, 1, 2, 3
W_UP_DEGREE = 0x10
LAYER_BIT = 0x80000000

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)

# Philox4x32-10 known answers (the published Random123 vectors): counter, key, output
PHILOX_KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def philox4x32_10(c, k):
    """c: four uint32 arrays of one shape, k: two ints -> four uint32 arrays."""
    c = [np.asarray(x).astype(np.uint64) for x in c]
    k0, k1 = np.uint64(k[0] & 0xFFFFFFFF), np.uint64(k[1] & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _MASK, (p0 >> _S32) ^ c[3] ^ k1, p0 & _MASK]
        k0 = (k0 + np.uint64(_W0)) & _MASK
        k1 = (k1 + np.uint64(_W1)) & _MASK
    return [x.astype(np.uint32) for x in c]


def shared_r(s, seed, layer, batch_seq):
    """r(s) for an array of global source ids."""
    s = np.asarray(s, np.uint32)
    full = lambda x: np.full(s.shape, x & 0xFFFFFFFF, np.uint32)
    c = [full(0), s, full(int(layer) | LAYER_BIT), full(int(batch_seq))]
    k = (int(seed) & 0xFFFFFFFF, ((int(seed) >> 32) ^ (int(batch_seq) >> 32)) & 0xFFFFFFFF)
    return philox4x32_10(c, k)[0]


def select_positions(nbrs, n, seed, layer, batch_seq, r_all=None):
    """The kept positions of one neighbour list, ascending: the n smallest
    keys (r << 32) | p by a plain argsort.  `r_all`: r of every vertex of the
    graph, computed once by the caller (the same words, looked up)."""
    nbrs = np.asarray(nbrs, np.uint32)
    if n >= nbrs.size:
        return np.arange(nbrs.size, dtype=np.int64)
    r = shared_r(nbrs, seed, layer, batch_seq) if r_all is None else r_all[nbrs]
    key = (r.astype(np.uint64) << _S32) | np.arange(nbrs.size, dtype=np.uint64)
    return np.sort(np.argsort(key, kind="stable")[:n])


def _norm_degree(od, idg):
    a = np.sqrt(od.astype(np.float64)).astype(np.float32)
    b = np.sqrt(idg.astype(np.float64)).astype(np.float32)
    return (np.float32(1) / (a * b)).astype(np.float32)


def layer_from_selection(dst, counts, ans, in_deg, out_deg, V, weight_flags=W_SUM, merge=False):
    """A sampled layer from its selection: `ans` holds the kept global source
    ids of every destination, destination-major, `counts` their number."""
    dst = np.asarray(dst, np.uint32)
    v = dst.size
    co = np.zeros(v + 1, np.uint32)
    np.cumsum(counts, out=co[1:])
    e = int(co[-1])
    ans = np.asarray(ans, np.uint32)
    mark = np.zeros(V, bool)
    mark[ans] = True
    if merge:
        mark[dst] = True
    source = np.nonzero(mark)[0].astype(np.uint32)
    index = np.zeros(V, np.uint32)
    index[source] = np.arange(source.size, dtype=np.uint32)
    ri = index[ans]
    edst = np.repeat(np.arange(v, dtype=np.uint32), np.asarray(counts, np.int64))
    order = np.argsort(ri, kind="stable")  # csc_to_csr: ascending destination per source
    ro = np.zeros(source.size + 1, np.uint32)
    np.cumsum(np.bincount(ri, minlength=source.size), out=ro[1:])
    out = dict(v_size=v, e_size=e, src_size=int(source.size), destination=dst, column_offset=co,
               sample_ans=ans, source=source, row_indices=ri, row_offset=ro,
               column_indices=edst[order], csr_edge_id=order.astype(np.uint32))
    if merge:
        out["dst_local_id"] = index[dst]
    wt = weight_flags & 0xF
    if wt != W_NONE:
        cnt = np.asarray(counts, np.uint32)
        if weight_flags & W_UP_DEGREE:
            od = np.bincount(ri, minlength=source.size).astype(np.uint32)[ri]
            idg = cnt[edst]
        else:
            od = np.asarray(out_deg, np.uint32)[ans]
            idg = np.asarray(in_deg, np.uint32)[dst][edst]
        w = _norm_degree(od, idg)
        if wt == W_MEAN:
            w = (w / idg.astype(np.float32)).astype(np.float32)
        if wt == W_MEAN_SAMPLED:
            w = (w / cnt[edst].astype(np.float32)).astype(np.float32)
        out["edge_weight_forward"] = w
        out["edge_weight_backward"] = w[order]
    return out


def shared_layer(col, rows, in_deg, out_deg, dst, fanout, seed, layer, batch_seq,
                 weight_flags=W_SUM, merge=False, order=None):
    """One hop under shared keys.  `order`: the order in which the destinations
    are evaluated (the result does not depend on it)."""
    col = np.asarray(col, np.uint64)
    rows = np.asarray(rows, np.uint32)
    dst = np.asarray(dst, np.uint32)
    V = col.size - 1
    deg = (col[dst.astype(np.int64) + 1] - col[dst.astype(np.int64)]).astype(np.int64)
    counts = deg if fanout < 0 else np.minimum(deg, fanout)
    pieces = [None] * dst.size
    r_all = shared_r(np.arange(V, dtype=np.uint32), seed, layer, batch_seq)
    for i in (range(dst.size) if order is None else order):
        beg = int(col[dst[i]])
        nb = rows[beg:beg + int(deg[i])]
        pieces[i] = nb[select_positions(nb, int(counts[i]), seed, layer, batch_seq, r_all)]
    ans = np.concatenate(pieces) if pieces else np.zeros(0, np.uint32)
    return layer_from_selection(dst, counts, ans, in_deg, out_deg, V, weight_flags, merge)


def shared_sample(col, rows, in_deg, out_deg, seeds, fanouts, seed=2000, batch_seq=0,
                  weight_flags=W_SUM, merge=False):
    """Every hop of a batch: hop l's destinations are hop l-1's sources."""
    layers, dst = [], np.asarray(seeds, np.uint32)
    for l, f in enumerate(fanouts):
        lay = shared_layer(col, rows, in_deg, out_deg, dst, f, seed, l, batch_seq, weight_flags, merge)
        layers.append(lay)
        dst = lay["source"]
    return layers
