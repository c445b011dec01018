"""References of one GAT layer with attention and output dropout on
the blocks of tests/gat_blocks.py, for given keep masks.

`drop_chain` is the materialised chain of tests/gat_heads_blocks.py (K = 1: of
tests/gat_blocks.py) with the attention `a` multiplied by its mask and scale
before the aggregation and the relu'd output by its mask and scale:

    a~[e,h] = keepA[e,h] a[e,h] sa,   Z_h[d] = sum_e a~[e,h] H[src_e]_h,
    Y = relu(concat or mean of Z_h) keepF sf.

It works in the dtype of its inputs (float64 with autograd: the reference;
float32: the yardstick).  `drop_loop` is an independent per-destination loop in
numpy float64.  `scale(p)` is the kernels' float32 1 / (1 - p) (0 for p >= 1).
"""
import numpy as np
import torch

import gat_heads_blocks as ghb


def scale(p):
    p = np.float32(p)
    return float(np.float32(1) / (np.float32(1) - p)) if p < 1 else 0.0


def drop_chain(H, att, co, ri, dl, K, D, mean, keepA=None, sa=1.0, keepF=None, sf=1.0):
    """(Y, m [e, K], a [e, K] undropped, Z): keepA [e, K] / keepF like Y, bool or
    0/1 (None: all kept)"""
    _, m, a = ghb.heads_chain_z(H, att, co, ri, dl, K, D, mean)
    v, e = co.numel() - 1, ri.numel()
    d_of_e = torch.repeat_interleave(torch.arange(v), (co[1:] - co[:-1]).long())
    ad = a * sa if keepA is None else a * keepA.to(H.dtype) * sa
    Z = torch.zeros(v, K, D, dtype=H.dtype).index_add(
        0, d_of_e, H[ri.long()].view(e, K, D) * ad[:, :, None])
    Z = Z.mean(1) if mean else Z.reshape(v, K * D)
    Y = torch.relu(Z)
    Y = Y * sf if keepF is None else Y * keepF.to(H.dtype) * sf
    return Y, m, a, Z


def drop_loop(H, att, co, ri, dl, K, D, mean, keepA, sa, keepF, sf):
    """The same layer one destination and one head at a time, numpy float64:
    (Y, m [e, K], a [e, K])."""
    H = np.asarray(H, np.float64)
    att = np.asarray(att, np.float64).reshape(-1)
    keepA, keepF = np.asarray(keepA, np.float64), np.asarray(keepF, np.float64)
    F = K * D
    v, e = len(co) - 1, int(co[-1])
    Y = np.zeros((v, D if mean else F))
    m, a = np.zeros((e, K)), np.zeros((e, K))
    for d in range(v):
        b, n = int(co[d]), int(co[d + 1])
        if b == n:
            continue
        z = np.zeros((K, D))
        for h in range(K):
            cols = slice(h * D, (h + 1) * D)
            s2 = float(H[dl[d], cols] @ att[F + h * D:F + (h + 1) * D])
            for j in range(b, n):
                u = float(H[ri[j], cols] @ att[cols]) + s2
                m[j, h] = u if u > 0 else 0.2 * u
            w = np.exp(m[b:n, h] - m[b:n, h].max())
            a[b:n, h] = w / w.sum()  # over all edges, dropped ones included
            for j in range(b, n):
                if keepA[j, h]:
                    z[h] += a[j, h] * sa * H[ri[j], cols]
        Y[d] = np.maximum(z.sum(0) / K if mean else z.reshape(-1), 0.0) * keepF[d] * sf
    return Y, m, a
