"""The cases and the torch chains of the BatchNorm + relu + dropout tests
(tests/test_batch_norm_cpu.py checks the relu-gate cap of every case on the
float64 chain alone; tests/test_batch_norm_kernel.py runs the kernels on them).

Chain.  dropout(relu(batch_norm(z))) with a given keep mask, autograd for dz,
dgamma, dbeta, and the running statistics after one training call.  rows > 1:
torch.native_batch_norm(training=True) in the asked dtype.  rows == 1 (torch
gives a NaN unbiased variance there): DESIGN §8s's formulas, var = 0, xh = 0,
the buffers left as they were; tests/test_batch_norm_cpu.py holds the same
formulas to autograd for rows > 1.
"""
import torch

EPS, MOM = 1e-5, 0.1
MASK_EPS, MASK_CAP = 1e-4, 1e-3
# rows: below, at and past the row threads of a tile; 601: 38 blocks of 16 rows,
# the last ragged; 16,400: the first count whose per-block run (20 rows) is past
# its minimum of 16
ROWS = [1, 2, 3, 5, 601]
BIG_ROWS = 16400
# id: (F, pitch, base offset in floats)
LAYOUTS = {
    "F1": (1, 3, 0),
    "F7": (7, 10, 0),
    "F64-v4": (64, 68, 0),
    "F67-s": (67, 70, 0),
    "F128-v4": (128, 132, 0),
    "F260-v4": (260, 264, 0),
    "F1024-v4": (1024, 1028, 0),
    "F128-pitch130-s": (128, 130, 0),
    "F128-base+4B-s": (128, 132, 1),
}
KINDS = ("randn", "offset1e4", "col-offset", "const-col")
PS = (0.0, 0.5)
CASES = [(lay, r) for lay in LAYOUTS for r in ROWS] + [("F7", BIG_ROWS), ("F128-v4", BIG_ROWS)]


def const_col(F):
    return F // 2


def inputs(kind, rows, F, seed):
    """z, gamma, beta (|beta| >= 0.01), dy, running_mean, running_var (> 0)"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, F, generator=g)
    if kind == "offset1e4":
        z = z + 1e4
    elif kind == "col-offset":
        z = z + 100.0 * torch.arange(F, dtype=torch.float32)
    elif kind == "const-col":
        z[:, const_col(F)] = 0.75
    gamma = 1 + 0.1 * torch.randn(F, generator=g)
    b = 0.1 * torch.randn(F, generator=g)
    beta = torch.where(b < 0, b - 0.01, b + 0.01)
    dy = torch.randn(rows, F, generator=g)
    rm = torch.randn(F, generator=g)
    rv = 0.5 + torch.rand(F, generator=g)
    return z, gamma, beta, dy, rm, rv


def seed_of(layout, rows, kind, k=0):
    F = LAYOUTS[layout][0]
    return 100 * F + rows + 1000003 * KINDS.index(kind) + 7919 * k


def chain(z, gamma, beta, rm, rv, keep, scale, dy, dtype):
    """returns (dict of quantities, pre-activation)"""
    rows = z.shape[0]
    z = z.detach().to(dtype).clone().requires_grad_()  # (fresh leaves: the inputs stay as they are)
    g = gamma.detach().to(dtype).clone().requires_grad_()
    b = beta.detach().to(dtype).clone().requires_grad_()
    rm, rv = rm.to(dtype).clone(), rv.to(dtype).clone()
    if rows > 1:
        n, mean, rstd = torch.native_batch_norm(z, g, b, rm, rv, True, MOM, EPS)
    else:
        mean = z.mean(0)  # (in the graph: dz = 0)
        rstd = torch.full_like(mean.detach(), EPS ** -0.5)
        n = g * ((z - mean) * rstd) + b
    y = torch.relu(n) * keep.to(dtype) * scale
    y.backward(dy.to(dtype))
    return dict(y=y.detach(), mean=mean.detach(), rstd=rstd.detach(), running_mean=rm,
                running_var=rv, dz=z.grad, dgamma=g.grad, dbeta=b.grad), n.detach()


def eval_chain(z, gamma, beta, rm, rv, dtype):
    a = [t.to(dtype) for t in (z, gamma, beta, rm, rv)]
    n = torch.batch_norm(a[0], a[1], a[2], a[3], a[4], False, MOM, EPS, False)
    return torch.relu(n), n


def pick(layout, rows, kind):
    """the inputs of a case: the first of a few seeds whose float64 chain has no
    more than MASK_CAP of its pre-activations within MASK_EPS of zero, in the
    training and in the eval chain (the reference alone decides; the keep
    mask does not enter the pre-activation).  Returns
    (inputs, near mask of the training chain, near mask of the eval chain,
    the larger share)."""
    F = LAYOUTS[layout][0]
    for k in range(8):
        t = inputs(kind, rows, F, seed_of(layout, rows, kind, k))
        z, gamma, beta, dy, rm, rv = t
        _, n64 = chain(z, gamma, beta, rm, rv, torch.ones(rows, F), 1.0, dy, torch.float64)
        _, e64 = eval_chain(z, gamma, beta, rm, rv, torch.float64)
        near, enear = n64.abs() < MASK_EPS, e64.abs() < MASK_EPS
        share = max(float(near.double().mean()), float(enear.double().mean()))
        if share <= MASK_CAP:
            break
    return t, near, enear, share
