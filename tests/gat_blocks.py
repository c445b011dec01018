"""A synthetic merged src/dst block for the GAT kernels, and the references of
one GAT layer on it.

The sampler's blocks (fanout 10-5) never have a column or a CSR row longer than
one 64-edge chunk, so the kernels' chunk loops, their carried running max / sum
and their parked per-chunk values would go unrun.  `make_block` builds the
smallest block that crosses every chunk boundary on both sides:

* 96 destinations mapped injectively into 320 sources (`dst_local_id`);
* column degrees 0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 200 and a random
  1..11 for the other columns, shuffled;
* sources uniform in [0, 320) (duplicates inside a column allowed), and source
  HUB once in every non-empty column, so its CSR row has ~95 slots;
* the CSR transpose by a stable sort of the edges by source.

`gat_chain` is the reference's layer with materialised messages
(GAT_SAMPLE_ALL_GPU.hpp:354-388) in torch, in the dtype of its inputs, so the
same code gives the float64 reference (autograd included) and the float32
yardstick.  `gat_loop` is an independent per-destination loop in numpy float64.
"""
import numpy as np
import torch

V_DST, N_SRC, HUB = 96, 320, 7
SPECIAL_DEGREES = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 200)


def make_block(seed=0):
    """dict of numpy arrays: column_offset [v+1], row_indices [e], dst_local_id
    [v], row_offset [s+1], column_indices [e], csr_edge_id [e] (uint32), and
    v, s, e."""
    rng = np.random.default_rng(seed)
    v, s = V_DST, N_SRC
    dl = rng.permutation(s)[:v].astype(np.uint32)
    deg = np.concatenate([np.array(SPECIAL_DEGREES, np.int64),
                          rng.integers(1, 12, v - len(SPECIAL_DEGREES))])
    rng.shuffle(deg)
    co = np.zeros(v + 1, np.int64)
    co[1:] = np.cumsum(deg)
    e = int(co[-1])
    ri = rng.integers(0, s, e)
    for d in range(v):
        if deg[d]:
            ri[co[d] + rng.integers(0, deg[d])] = HUB
    d_of_e = np.repeat(np.arange(v), deg)
    order = np.argsort(ri, kind="stable")
    ro = np.zeros(s + 1, np.int64)
    ro[1:] = np.cumsum(np.bincount(ri, minlength=s))
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
    return dict(v=v, s=s, e=e, column_offset=u32(co), row_indices=u32(ri), dst_local_id=dl,
                row_offset=u32(ro), column_indices=u32(d_of_e[order]), csr_edge_id=u32(order))


def gat_chain_z(H, att, co, ri, dl, F):
    """(Z, m, a): the pre-activation sum a*H[src], the post-leaky scores and the
    attention of every edge, in H's dtype, with materialised messages: msg =
    [H[src], H[dst]], m = leaky(msg W_att), per-dst softmax (max-subtracted,
    edge_softmax_forward_norm_block), sum a*H[src]."""
    v = co.numel() - 1
    deg = (co[1:] - co[:-1]).long()
    d_of_e = torch.repeat_interleave(torch.arange(v, device=H.device), deg)
    msg = torch.cat([H[ri.long()], H[dl.long()[d_of_e]]], 1)
    m = torch.nn.functional.leaky_relu(msg @ att.view(2 * F, 1), 0.2).view(-1)
    mx = torch.full((v,), -float("inf"), dtype=H.dtype, device=H.device).scatter_reduce(
        0, d_of_e, m, "amax")
    ex = torch.exp(m - mx[d_of_e])
    sm = torch.zeros(v, dtype=H.dtype, device=H.device).index_add(0, d_of_e, ex)
    a = ex / sm[d_of_e]
    Z = torch.zeros(v, F, dtype=H.dtype, device=H.device).index_add(0, d_of_e, H[ri.long()] * a[:, None])
    return Z, m, a


def gat_chain(H, att, co, ri, dl, F):
    """(Y, m, a) of the reference layer chain: Y = relu(Z) of gat_chain_z."""
    Z, m, a = gat_chain_z(H, att, co, ri, dl, F)
    return torch.relu(Z), m, a


def gat_loop(H, att, co, ri, dl):
    """The same layer one destination at a time, numpy float64: (Y, m, a)."""
    H = np.asarray(H, np.float64)
    att = np.asarray(att, np.float64).reshape(-1)
    F = H.shape[1]
    a1, a2 = att[:F], att[F:]
    v = len(co) - 1
    Y = np.zeros((v, F))
    m = np.zeros(int(co[-1]))
    a = np.zeros(int(co[-1]))
    for d in range(v):
        b, e = int(co[d]), int(co[d + 1])
        if b == e:
            continue
        s2 = float(H[dl[d]] @ a2)
        z = np.zeros(F)
        scores = []
        for j in range(b, e):
            u = float(H[ri[j]] @ a1) + s2
            scores.append(u if u > 0 else 0.2 * u)
        top = max(scores)
        w = [np.exp(x - top) for x in scores]
        tot = sum(w)
        for j in range(b, e):
            m[j] = scores[j - b]
            a[j] = w[j - b] / tot
            z += a[j] * H[ri[j]]
        Y[d] = np.maximum(z, 0.0)
    return Y, m, a
