"""References of one GATv2 layer (K heads of D columns, F = K D) on
the blocks of tests/gat_blocks.py.

    t[e]   = leaky_relu(Hs[src_e] + Hd[d_e], 0.2)
    u[e,h] = t[e]_h . att_h,   a[e,h] = softmax over the edges of d of u[., h]
    Z_h[d] = sum_e a~[e,h] Hs[src_e]_h,   Z = concat_h Z_h or (1/K) sum_h Z_h

`v2_chain_z` is the layer with materialised [e, F] messages in torch, in the
dtype of its inputs, so the same code gives the float64 reference (autograd
included) and the float32 yardstick.  `v2_loop` is an independent
per-destination loop in numpy float64.  Hd has one row per destination, in
destination order.
"""
import numpy as np
import torch


def v2_chain_z(Hs, Hd, att, co, ri, K, D, mean, keepA=None, sa=1.0):
    """(Z, u [e, K], a [e, K] undropped): Z is [v, F] (concat) or [v, D] (mean).
    keepA [e, K] (bool or 0/1) and sa: the attention dropout mask and scale."""
    v, e = co.numel() - 1, ri.numel()
    dt = Hs.dtype
    deg = (co[1:] - co[:-1]).long()
    d_of_e = torch.repeat_interleave(torch.arange(v), deg)
    xs = Hs[ri.long()]
    t = torch.nn.functional.leaky_relu(xs + Hd[d_of_e], 0.2)
    u = (t * att.reshape(1, -1)).view(e, K, D).sum(2)
    mx = torch.full((v, K), -float("inf"), dtype=dt).scatter_reduce(
        0, d_of_e[:, None].expand(e, K), u, "amax")
    ex = torch.exp(u - mx[d_of_e])
    sm = torch.zeros(v, K, dtype=dt).index_add(0, d_of_e, ex)
    a = ex / sm[d_of_e]
    ad = a * sa if keepA is None else a * keepA.to(dt) * sa
    Z = torch.zeros(v, K, D, dtype=dt).index_add(0, d_of_e, xs.view(e, K, D) * ad[:, :, None])
    Z = Z.mean(1) if mean else Z.reshape(v, K * D)
    return Z, u, a


def v2_loop(Hs, Hd, att, co, ri, K, D, mean):
    """The same layer one destination and one head at a time, numpy float64:
    (Z, u [e, K], a [e, K])."""
    Hs, Hd = np.asarray(Hs, np.float64), np.asarray(Hd, np.float64)
    att = np.asarray(att, np.float64).reshape(-1)
    F = K * D
    assert Hs.shape[1] == F and Hd.shape[1] == F and att.size == F
    v, e = len(co) - 1, int(co[-1])
    Z = np.zeros((v, D if mean else F))
    u, a = np.zeros((e, K)), np.zeros((e, K))
    for d in range(v):
        b, n = int(co[d]), int(co[d + 1])
        if b == n:
            continue
        z = np.zeros((K, D))
        for h in range(K):
            cols = slice(h * D, (h + 1) * D)
            for j in range(b, n):
                s = Hs[ri[j], cols] + Hd[d, cols]
                u[j, h] = float(np.where(s > 0, s, 0.2 * s) @ att[cols])
            w = np.exp(u[b:n, h] - u[b:n, h].max())
            a[b:n, h] = w / w.sum()
            for j in range(b, n):
                z[h] += a[j, h] * Hs[ri[j], cols]
        Z[d] = z.sum(0) / K if mean else z.reshape(-1)
    return Z, u, a


def v2_manual_grads(Hs, Hd, att, co, ri, K, D, mean, GY, leaky_from_score=False,
                    wrong_head=False, no_inv_k=False, drop_q=False):
    """The backward formulas of DESIGN §8n in float64 torch (no autograd): (dHs, dHd,
    datt, du) for GY = dL/dY, Y = relu(Z).  The flags plant the plausible kernel
    mistakes, one at a time (tests/test_gatv2_cpu.py holds each to a visible
    change): leaky' read off the sign of the score u instead of the sum, the
    softmax-backward reduction taken over the next head, a missing 1/K in mean
    mode, q left out of dHs."""
    v, e, F = co.numel() - 1, ri.numel(), K * D
    deg = (co[1:] - co[:-1]).long()
    d_of_e = torch.repeat_interleave(torch.arange(v), deg)
    Z, u, a = v2_chain_z(Hs, Hd, att, co, ri, K, D, mean)
    GM = torch.where(Z > 0, GY, torch.zeros((), dtype=Hs.dtype))
    if mean:
        GM = (GM if no_inv_k else GM / K).repeat(1, K)
    xs = Hs[ri.long()]
    ssum = xs + Hd[d_of_e]
    ga = (GM[d_of_e] * xs).view(e, K, D).sum(2)
    sag = torch.zeros(v, K, dtype=Hs.dtype).index_add(0, d_of_e, a * ga)
    if wrong_head:
        sag = sag.roll(1, 1)
    du = a * (ga - sag[d_of_e])
    due = du.repeat_interleave(D, 1)
    one, slope = torch.ones((), dtype=Hs.dtype), torch.full((), 0.2, dtype=Hs.dtype)
    if leaky_from_score:
        lp = torch.where(u > 0, one, slope).repeat_interleave(D, 1)
    else:
        lp = torch.where(ssum > 0, one, slope)
    q = due * att.reshape(1, -1) * lp
    dHd = torch.zeros(v, F, dtype=Hs.dtype).index_add(0, d_of_e, q)
    msg = a.repeat_interleave(D, 1) * GM[d_of_e]
    if not drop_q:
        msg = msg + q
    dHs = torch.zeros(Hs.shape[0], F, dtype=Hs.dtype).index_add(0, ri.long(), msg)
    datt = (due * torch.nn.functional.leaky_relu(ssum, 0.2)).sum(0)
    return dHs, dHd, datt, du
