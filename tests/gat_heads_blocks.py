"""References of one multi-head GAT layer (K heads of D columns, F = K D) on the
blocks of tests/gat_blocks.py.

`heads_chain_z` is the single-head chain `gat_blocks.gat_chain_z` run once per
head on the column slice H[:, hD:(h+1)D] with that head's slices of a1 =
att[0:F] and a2 = att[F:2F], then the concatenation of the heads (concat mode)
or their mean (mean mode).  It works in the dtype of its inputs, so the same
code gives the float64 reference (autograd included) and the float32 yardstick.
`heads_loop` is an independent per-destination loop in numpy float64.
"""
import numpy as np
import torch

import gat_blocks


def head_att(att, K, D, h):
    """head h's [2D] attention vector out of att [2 K D] = [a1 | a2]"""
    F = K * D
    att = att.reshape(-1)
    return torch.cat([att[h * D:(h + 1) * D], att[F + h * D:F + (h + 1) * D]])


def heads_chain_z(H, att, co, ri, dl, K, D, mean):
    """(Z, m, a): the pre-activation ([v, F] concat, [v, D] mean), the post-leaky
    scores and the attention of every edge and head ([e, K])"""
    Zs, ms, as_ = [], [], []
    for h in range(K):
        Z, m, a = gat_blocks.gat_chain_z(H[:, h * D:(h + 1) * D], head_att(att, K, D, h),
                                         co, ri, dl, D)
        Zs.append(Z)
        ms.append(m)
        as_.append(a)
    Z = torch.stack(Zs, 0).mean(0) if mean else torch.cat(Zs, 1)
    return Z, torch.stack(ms, 1), torch.stack(as_, 1)


def heads_chain(H, att, co, ri, dl, K, D, mean):
    """(Y, m, a) of the layer: Y = relu(Z) of heads_chain_z"""
    Z, m, a = heads_chain_z(H, att, co, ri, dl, K, D, mean)
    return torch.relu(Z), m, a


def heads_loop(H, att, co, ri, dl, K, D, mean):
    """The same layer one destination and one head at a time, numpy float64:
    (Y, m [e, K], a [e, K])."""
    H = np.asarray(H, np.float64)
    att = np.asarray(att, np.float64).reshape(-1)
    F = K * D
    assert H.shape[1] == F and att.size == 2 * F
    v, e = len(co) - 1, int(co[-1])
    Y = np.zeros((v, D if mean else F))
    m = np.zeros((e, K))
    a = np.zeros((e, K))
    for d in range(v):
        b, n = int(co[d]), int(co[d + 1])
        if b == n:
            continue
        z = np.zeros((K, D))
        for h in range(K):
            cols = slice(h * D, (h + 1) * D)
            a1, a2 = att[cols], att[F + h * D:F + (h + 1) * D]
            s2 = float(H[dl[d], cols] @ a2)
            for j in range(b, n):
                u = float(H[ri[j], cols] @ a1) + s2
                m[j, h] = u if u > 0 else 0.2 * u
            w = np.exp(m[b:n, h] - m[b:n, h].max())
            a[b:n, h] = w / w.sum()
            for j in range(b, n):
                z[h] += a[j, h] * H[ri[j], cols]
        Y[d] = np.maximum(z.sum(0) / K if mean else z.reshape(-1), 0.0)
    return Y, m, a
