"""Numpy restatements for the edge-coefficient tests.

An edge e of the graph carries a coefficient a_e (fp32, CSC order); a kept
edge k of a sampled layer sits at CSC position q_k and its weight is
fl32(c_k * a[q_k]), c the weight of weight_type.  The aggregation is the
project's serial one: per output element (x * w) + acc from 0 in CSC edge
order, every operation rounded to fp32.
"""
import numpy as np


def coef_weights(c, a, q):
    """fl32(c * a[q]): one fp32 multiply, round to nearest (c: scalar or [e])."""
    a = np.asarray(a, np.float32)
    return (np.asarray(c, np.float32) * a[np.asarray(q, np.int64)]).astype(np.float32)


def edge_dst_ids(col):
    """the destination of every CSC position"""
    col = np.asarray(col).astype(np.int64)
    return np.repeat(np.arange(col.size - 1, dtype=np.int64), np.diff(col))


def edge_positions(col, rows, dst_of_edge, src_of_edge):
    """CSC position of each (src, dst) pair of a graph WITHOUT parallel edges."""
    V = np.asarray(col).size - 1
    key = edge_dst_ids(col) * V + np.asarray(rows).astype(np.int64)
    order = np.argsort(key, kind="stable")
    assert (np.diff(key[order]) > 0).all(), "parallel edges: positions are not recoverable"
    want = np.asarray(dst_of_edge).astype(np.int64) * V + np.asarray(src_of_edge).astype(np.int64)
    at = np.searchsorted(key[order], want)
    assert np.array_equal(key[order][at], want)
    return order[at]


def layer_positions(col, rows, lay):
    """q_k of every kept edge of a sampled layer (dict of numpy arrays with
    destination, column_offset, sample_ans), graph without parallel edges."""
    co = lay["column_offset"].astype(np.int64)
    edst = np.repeat(np.arange(co.size - 1), np.diff(co))
    return edge_positions(col, rows, lay["destination"][edst], lay["sample_ans"])


def serial_spmm(col, rows, w, x, relu=False):
    """Y[d] = sum over d's CSC positions of (x[rows[e]] * w[e]) + acc, fp32,
    in order; every column of the graph (an empty one: zeros)."""
    col = np.asarray(col).astype(np.int64)
    rows = np.asarray(rows).astype(np.int64)
    w = np.asarray(w, np.float32)
    x = np.asarray(x, np.float32)
    deg = np.diff(col)
    y = np.zeros((col.size - 1, x.shape[1]), np.float32)
    for p in range(int(deg.max()) if deg.size else 0):
        d = np.nonzero(deg > p)[0]
        e = col[d] + p
        y[d] = (x[rows[e]] * w[e][:, None]).astype(np.float32) + y[d]
    return np.maximum(y, np.float32(0)) if relu else y


def simple_graph(V, E, hub_degree, seed):
    """Chung-Lu-like edge list without parallel edges, plus one destination
    (vertex 0) of in-degree about hub_degree, and vertex V - 1 without
    in-edges; file order shuffled.  Returns (src, dst) uint32."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, V + 1) ** 0.6
    p /= p.sum()
    src = rng.choice(V, E, p=p)
    dst = rng.choice(V - 2, E, p=p[:V - 2] / p[:V - 2].sum()) + 1  # not 0, not V - 1
    hub_src = rng.choice(V, hub_degree, replace=False)
    src = np.concatenate([src, hub_src])
    dst = np.concatenate([dst, np.zeros(hub_degree, np.int64)])
    pair = np.unique(dst.astype(np.int64) * V + src)
    pair = pair[rng.permutation(pair.size)]
    return (pair % V).astype(np.uint32), (pair // V).astype(np.uint32)
