"""The non-GAT models' training step with dropout on, restated in torch over a
trained batch's own sampled layers, with every keep mask rebuilt from cfg.seed
and the order of the draws (the GAT drivers have theirs in
tests/test_gat_dropout_driver.py).  It imports without a GPU.

Every hidden layer l (0 the bottom) computes

    X_{l+1} = keep_l * scale(p) * relu(f_l(agg(X_l))),
    keep_l  = keep(v_size_l, width_{l+1}, p, key(seed), first_offset + l):

the mask's row is the layer's local destination index and its column the
logical column (never a pitch).  f_l is the linear map, linear then LayerNorm,
linear then BatchNorm on the batch's statistics, or the root-stacked
[A X | X_dst] W; agg is the sum with the layer's edge_weight_forward (which
carries the weight type: sum, mean, up-degree) or the max aggregator.  A
transform-first bottom layer A (X W) is the same function of its inputs as
(A X) W and has the same mask, so one chain serves both orders.

The masks come from tests/gemm_layouts.py's numpy Philox4x32-10, never from the
kernels under test.

The offset schedule (nts/host/gcn.cpp, nts/host/linkpred.cpp).  The driver keeps
one counter, dropout_calls_, zero at construction.  A training forward takes
one value per hidden layer, in layer order, bottom first, whichever form the
layer has: the transform-first bottom (hip_bottom_transform in forward()), and
in vertexForward() the GEMM epilogue (hip_linear_act), LayerNorm
(layer_norm_act) and BatchNorm (batch_norm_act).  The output layer draws none.
The forward of batch k runs after that of batch k - 1 with or without the
pipeline (only sampling and the bottom aggregation, which draw nothing, run
ahead), so step k of a model of L layers uses offsets k (L - 1) ... k (L - 1)
+ L - 2: `offsets(k, L)`.  The link predictor counts the same way in training
(ctx.is_train() ? dropout_calls_++ : 0) and takes none in evaluation; of the
node drivers' forms only BatchNorm leaves the counter alone in evaluation, so
these chains hold for steps with no evaluation in between.
"""
import numpy as np
import torch

import gat_drop_blocks as gdb
import gemm_layouts
import test_batch_norm_driver as tbd
import test_layer_norm_driver as tld
import test_link_pred_driver as tlp
import test_max_driver as tmd
from test_root_driver import _agg

scale = gdb.scale  # the same rule as keep_scale (nts/host/ops_util.hpp): float32 1 / (1 - p)


def key(seed):
    """the drivers' dropout_key()"""
    return (int(seed) * 0x9E3779B97F4A7C15 + 1) % 2 ** 64


def keep(rows, cols, p, seed, offset):
    """bool [rows, cols]: the keep mask of Philox key `seed` (a key(cfg.seed)) at `offset`"""
    return torch.from_numpy(gemm_layouts._dropout_keep(int(rows), int(cols), float(p), int(seed), int(offset)))


def offsets(step, n_layers):
    """the offsets of training step `step` (0 the first) of a model of
    `n_layers` layers, one per hidden layer, bottom first"""
    return [step * (n_layers - 1) + l for l in range(n_layers - 1)]


def _drop(X, l, p, seed, first_offset, s, masks):
    m = keep(X.shape[0], X.shape[1], p, key(seed), first_offset + l)
    masks.append(m)
    return X * m.to(X.dtype) * (scale(p) if s is None else s)


def chain(lays, data, ws, dtype, p, seed, first_offset, norm=None, stats=None, root=False, mx=False,
          labels=None, s=None):
    """The model over the sampled layers `lays` (top first, as drv.last_layers)
    in `dtype`.  `ws`: the L weights, then with norm = "layer" / "batch" gamma
    and beta of every hidden layer (the order of drv.weights()); `stats`: the
    BatchNorm buffers in `dtype`, moved in place as the driver's are; `labels`:
    the multi-label targets (BCE with logits instead of the NLL); `s`
    replaces scale(p).  Returns (parameters, loss, hidden activations, masks)."""
    L = len(lays)
    feat = data["feat"].cpu().to(dtype)
    P = [w.detach().cpu().to(dtype).requires_grad_() for w in ws]  # (leaves of their own, whatever ws are)
    X, hidden, masks = feat[lays[-1]["source"].cpu().long()], [], []
    for l in range(L):
        lay = lays[L - 1 - l]
        Y = tmd._max_agg(lay, X)[0] if mx else _agg(lay, X)
        if root:
            own = feat[lay["destination"].cpu().long()] if l == 0 else X[lay["dst_local_id"].cpu().long()]
            Y = torch.cat([Y, own], 1)
        Z = Y @ P[l]
        if l == L - 1:
            break
        if norm == "layer":
            Z = tld._ln(Z, P[L + 2 * l], P[L + 2 * l + 1])
        elif norm == "batch":
            Z = tbd._bn(Z, P[L + 2 * l], P[L + 2 * l + 1], stats[2 * l], stats[2 * l + 1], True)
        else:
            assert norm is None
        X = _drop(torch.relu(Z), l, p, seed, first_offset, s, masks)
        hidden.append(X)
    dst = lays[0]["destination"].cpu().long()
    if labels is None:
        loss = torch.nn.functional.nll_loss(Z.log_softmax(1), data["labels"].cpu()[dst])
    else:
        loss = torch.nn.functional.binary_cross_entropy_with_logits(Z, labels.cpu()[dst].to(dtype))
    return P, loss, hidden, masks


def top_gap(lays, hidden):
    """the max aggregator's winners gap (tests/test_max_driver.py) of the top
    hop over the chain's last hidden activation"""
    return tmd._max_agg(lays[0], hidden[-1].detach())[1]


def lp_chain(lb, feat, ws, dtype, p, seed, first_offset, s=None):
    """The link predictor's step over drv.last_batch() `lb`
    (tests/test_link_pred_driver.py's chain with the masks); returns what
    chain() returns."""
    layers = lb["layers"]
    L = len(ws)
    P = [w.detach().cpu().to(dtype).requires_grad_() for w in ws]
    X = feat.cpu().to(dtype)[layers[L - 1]["source"].cpu().numpy().view(np.uint32).astype(np.int64)]
    hidden, masks = [], []
    for l in range(L):
        X = (tlp._dense(layers[L - 1 - l], dtype) @ X) @ P[l]
        if l < L - 1:
            X = _drop(torch.relu(X), l, p, seed, first_offset, s, masks)
            hidden.append(X)
    return P, tlp._pair_loss(X, lb)[0], hidden, masks
