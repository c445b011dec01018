"""One Adam step as a gradient readout, and the float32-yardstick bound.

With the drivers' defaults (epsilon = 1e-9, zero moments) the first step is

    W1 = W0 - lr (1-b1) g / (sqrt((1-b2) g^2) + 1e-9)  ~=  W0 - 3.16 lr sign(g):

comparing weights after it checks each gradient element's sign and nothing
else.  With weight_decay = 0 and epsilon = 1 (plain GCNConfig fields) the same
step of k_adam (csrc/aggregate.hip) is

    W0 - W1 = lr (1-b1) g / (1 + sqrt(1-b2) |g|),

monotonic in g and nearly linear for |g| << 30, so it inverts:

    u = (W0 - W1) / (lr (1-b1)),   g = u / (1 - sqrt(1-b2) |u|).

lr = 10 makes the weight change about the size of g.  W1 is a float32 near W0,
so g is resolved to ulp(max|W0|) / (lr (1-b1)): `resolution` returns it and the
bound below adds it.  (1-b1) and (1-b2) are k_adam's own float32 differences
1.0f - 0.9f and 1.0f - 0.999f, not 0.1 and 0.001 (these differ by 2.4e-7 and
1.3e-5 relative).
"""
import numpy as np
import torch

LR = 10.0
OMB1 = float(np.float32(1) - np.float32(0.9))
OMB2 = float(np.float32(1) - np.float32(0.999))
FLOOR = 8 * 2.0 ** -24
# The constant of the yardstick rule, one for every test that uses it: the
# smallest power of two at least twice the largest err(kernel) / err(float32
# chain) measured on an MI355X over every case and quantity of
# tests/test_gat_kernel.py (2.52: Y at F = 255, extreme scores; the table is in
# DESIGN.md).  The step tests' ratios, net of the readout's resolution, are
# all below 1.
C = 8


def readout(cfg, lr=LR):
    """Turn a GCNConfig's Adam step into the gradient readout (in place)."""
    cfg.weight_decay = 0.0
    cfg.epsilon = 1.0
    cfg.learn_rate = lr
    return cfg


def recovered_grads(W0, W1, lr=LR):
    """float64 gradients from the weights before and after the first step."""
    u = (W0.detach().cpu().double() - W1.detach().cpu().double()) / (lr * OMB1)
    return u / (1.0 - np.sqrt(OMB2) * u.abs())


def resolution(W0, lr=LR):
    """the absolute step of the readout: one float32 ulp of the largest weight,
    in units of g"""
    top = float(W0.detach().abs().max())
    return float(np.spacing(np.float32(top))) / (lr * OMB1)


def err(x, ref):
    """max|x - ref| / max|ref| in float64"""
    x, ref = x.detach().cpu().double(), ref.detach().cpu().double()
    return float((x - ref).abs().max()) / float(ref.abs().max())


def yardstick_bound(e32, c, extra=0.0):
    """the bound on err(kernel): c times the error of the same chain in float32
    torch, plus a floor for chains that happen to be nearly exact in float32
    (plus the readout's resolution where there is one)"""
    return c * e32 + FLOOR + extra


def check_step_grads(W0, W1, g64, g32, c, names=None, lr=LR, out=print):
    """Recover every parameter's gradient from one readout step and hold it to
    the yardstick bound against the float64 gradients g64, with g32 the float32
    chain's.  Prints every figure before asserting; returns the ratios."""
    ratios, bad = [], []
    for i, (w0, w1, r64, r32) in enumerate(zip(W0, W1, g64, g32)):
        name = names[i] if names else f"W[{i}]"
        g = recovered_grads(w0, w1, lr).reshape(r64.shape)
        top = float(r64.detach().abs().max())
        assert top > 0, f"{name}: the float64 gradient is zero"
        ek, e32 = err(g, r64), err(r32, r64)
        extra = resolution(w0, lr) / top
        bound = yardstick_bound(e32, c, extra)
        ratio = max(ek - extra, 0.0) / max(e32, 2.0 ** -30)  # net of the resolution
        out(f"  {name}: max|g| {top:.3e} err(driver) {ek:.3e} err(fp32 chain) {e32:.3e} "
            f"resolution {extra:.3e} net ratio {ratio:.2f} bound {bound:.3e}")
        ratios.append(ratio)
        if not ek <= bound:
            bad.append(f"{name}: {ek:.3e} > {bound:.3e}")
    assert not bad, "; ".join(bad)
    return ratios
