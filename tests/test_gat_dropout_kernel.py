"""The dropout forms of the GAT kernels (csrc/gat.hip) through the
wrappers, on the synthetic block of tests/gat_blocks.py: columns of 0 ... 200
edges (more than one 64-edge chunk, empty columns, columns that start at edge
positions that are no multiple of 4: the keep bits' word choice) and a CSR row
of ~95 slots.

Reference: the materialised chain of tests/gat_drop_blocks.py in float64
autograd, with the attention multiplied by its mask and 1 / (1 - q) and the
relu'd output by its mask and 1 / (1 - p); q32 is the same chain in float32.
The masks are what relu_dropout leaves of a ones tensor ([e, K] at the attention
offset, the shape of Y at the output offset) for the same seed: a kernel with
another bit convention is wrong by O(1).  Bound, for Y, m, a (the undropped
softmax), dH and dW_att, rates (0.6, 0), (0, 0.5), (0.6, 0.5), moderate and
extreme scores:

    err(kernel) <= C * err(q32) + 8 * 2^-24,   C = 8 (tests/step_check.py).

CELLS adds, with the rates (0.6, 0.5) and moderate scores, a shape for every
(vector width, chunks[, reduction scheme]) combination of the single-head and
the multi-head kernels that the cases above leave out, so that each dropout
kernel the dispatch can pick is run; the scalar-path cells put every row
operand 4 bytes past a 16-byte boundary.

Incoming gradients are zeroed where the float64 pre-activation has 0 < |Z| <
1e-4 (§8b).  The cap on their share, 1e-3 (or one element), counts the elements
of non-empty rows in which a head keeps at least a quarter of its attention
mass mu = sum of keepA a.  Z of a head scales with mu, so an element lands
within 1e-4 of zero with a probability of about 1e-4 / (mu |H|): by
construction, not by a chance of the data, where the dropout took the head's
mass (with one-hot attention, whenever the top edge is dropped), and at the
undropped layer's rate (§8b: about 1e-4) only where mu is of order one; at
mu = 1/4 with 1 / (1 - q) = 2.5 that rate is still below the cap.  Little is
hidden in the other rows: their GM reaches dH and dW_att only through the kept
weights, at most mu / (1 - q).  Z = 0 exactly (every edge of every head
dropped) is no near-zero either: float32 gives the same 0.  The data seed is
the first of 8 whose float64 chain stays inside the cap.
"""
import numpy as np
import pytest
import torch

import gat_blocks
import gat_drop_blocks as gdb
from step_check import C, err, yardstick_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -12345.5
MASK_EPS, MASK_CAP, LIVE = 1e-4, 1e-3, 0.25
SEED, OFF_A, OFF_F = 0x9E3779B97F4A7C15 * 2000 + 1 & (2 ** 64 - 1), 3, (1 << 33) + 7

# id: (K, D, mean)
SINGLE = {"F16-v4n1": (1, 16, False), "F260-v4n2-partial": (1, 260, False),
          "F67-v1n2": (1, 67, False), "F1024-v4n4": (1, 1024, False)}
HEADS = {"K8-D8-concat": (8, 8, False), "K4-D256-concat": (4, 256, False),
         "K3-D20-concat": (3, 20, False), "K3-D7-concat": (3, 7, False),
         "K4-D16-mean": (4, 16, True), "K2-D128-mean": (2, 128, True)}
CASES = {**SINGLE, **HEADS}
RATES = {"attn": (0.6, 0.0), "feat": (0.0, 0.5), "both": (0.6, 0.5)}
# The cells of the kernel dispatch that CASES leaves out: the other four
# (VEC, NCH) of the single-head kernels and, for the multi-head ones, the
# smallest shape of every other (VEC, NCH, MODE) (g = D / 4 lanes per head on the
# float4 path, D on the scalar one; NCH = ceil(K g / 64)).  id: (K, D, mean, base
# offset in floats of every row operand: 1 forces the scalar path).  Run with
# both dropouts in the moderate regime.
CELLS = {
    "cell-F516-v4n3": (1, 516, False, 0),
    "cell-F33-v1n1": (1, 33, False, 0),
    "cell-F129-v1n3": (1, 129, False, 0),
    "cell-F193-v1n4": (1, 193, False, 0),
    "cell-v4-pow2-n2-K8-D64": (8, 64, False, 0),
    "cell-v4-pow2-n3-K5-D128": (5, 128, False, 0),
    "cell-v4-pow2-n4-K8-D128": (8, 128, False, 0),
    "cell-v4-chunk-n1-K1-D256-heads-entry": (1, 256, False, 0),
    "cell-v4-chunk-n2-K2-D256": (2, 256, False, 0),
    "cell-v4-chunk-n3-K3-D256": (3, 256, False, 0),
    "cell-v4-any-n2-K2-D132": (2, 132, False, 0),
    "cell-v4-any-n3-K3-D176": (3, 176, False, 0),
    "cell-v4-any-n4-K4-D208": (4, 208, False, 0),
    "cell-v1-pow2-n1-K8-D8-base+4B": (8, 8, False, 1),
    "cell-v1-pow2-n2-K4-D32-base+4B": (4, 32, False, 1),
    "cell-v1-pow2-n3-K6-D32-base+4B": (6, 32, False, 1),
    "cell-v1-pow2-n4-K8-D32-base+4B": (8, 32, False, 1),
    "cell-v1-chunk-n1-K1-D64-base+4B-heads-entry": (1, 64, False, 1),
    "cell-v1-chunk-n2-K2-D64-base+4B": (2, 64, False, 1),
    "cell-v1-chunk-n3-K3-D64-base+4B": (3, 64, False, 1),
    "cell-v1-chunk-n4-K4-D64-base+4B": (4, 64, False, 1),
    "cell-v1-any-n2-K3-D41": (3, 41, False, 0),
    "cell-v1-any-n3-K3-D51": (3, 51, False, 0),
    "cell-v1-any-n4-K5-D51": (5, 51, False, 0),
}
RUNS = ([(c, r, g) for g in ("moderate", "extreme") for r in RATES for c in CASES]
        + [(c, "both", "moderate") for c in CELLS])


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=2000)


@pytest.fixture(scope="module")
def block():
    b = gat_blocks.make_block()
    dev = {k: torch.from_numpy(b[k].view(np.int32)).to(DEV)
           for k in ("column_offset", "row_indices", "dst_local_id", "row_offset",
                     "column_indices", "csr_edge_id")}
    cpu = {k: torch.from_numpy(b[k].astype(np.int64))
           for k in ("column_offset", "row_indices", "dst_local_id")}
    co = b["column_offset"].astype(np.int64)
    assert np.any(co[:-1][np.diff(co) > 0] % 4 != 0) and np.diff(co).max() > 128
    return dict(np=b, dev=dev, cpu=cpu, v=b["v"], s=b["s"], e=b["e"])


def keep_mask(hip, rows, cols, p, offset, seed=SEED):
    """[rows, cols] bool: what relu_dropout keeps of a ones tensor"""
    if p == 0.0:
        return torch.ones(rows, cols, dtype=torch.bool)
    y = torch.empty(rows, cols, device=DEV)
    hip.relu_dropout(torch.ones(rows, cols, device=DEV), y, p=p, seed=seed, offset=offset)
    return (y > 0).cpu()


def _at(rows, width, off, fill):
    """[rows, width] on the device, contiguous, its base `off` floats past a fresh
    allocation's; fill: a value or the [rows, width] tensor to hold"""
    t = torch.empty(rows * width + 4, device=DEV)[off:off + rows * width].view(rows, width)
    if torch.is_tensor(fill):
        t.copy_(fill)
    else:
        t.fill_(fill)
    return t


class Run:
    """One forward + backward through the wrappers.  new: the _drop entry points
    (single: K = 1 through the single-head ones); else the existing ones.  off:
    the base offset in floats of every row operand."""

    def __init__(self, hip, block, H, att, GY, K, D, mean, q, p, new=True, heads_entry=None,
                 off=0):
        v, s, e = block["v"], block["s"], block["e"]
        d = block["dev"]
        F, FY = K * D, (D if mean else K * D)
        single = K == 1 if heads_entry is None else not heads_entry
        self.H, self.att = _at(s, F, off, H), att.to(DEV)
        self.m = torch.full((e * K,), SENT, device=DEV)
        self.a = torch.full((e * K,), SENT, device=DEV)
        self.Y = _at(v, FY, off, SENT)
        co, ri, dl = d["column_offset"], d["row_indices"], d["dst_local_id"]
        fkw = dict(p_attn=q, p_out=p, seed=SEED, off_attn=OFF_A, off_out=OFF_F) if new else {}
        if single:
            f = hip.gat_forward_drop if new else hip.gat_forward
            f(co, ri, dl, v, self.H, self.att, self.m, self.a, self.Y, **fkw)
        else:
            f = hip.gat_forward_heads_drop if new else hip.gat_forward_heads
            f(co, ri, dl, v, self.H, K, self.att, self.m, self.a, self.Y, mean=mean, **fkw)
        self.GY = _at(v, FY, off, GY)
        self.du = torch.full((e * K,), SENT, device=DEV)
        self.ds2 = torch.full((s * K,), SENT, device=DEV)
        self.dS = torch.full((s, 2 * K), SENT, device=DEV)
        self.dH = _at(s, F, off, SENT)
        self.GM = _at(v, F, off, SENT)
        bkw = dict(p_attn=q, p_out=p, seed=SEED, off_attn=OFF_A) if new else {}
        tail = (d["row_offset"], d["column_indices"], d["csr_edge_id"], s, self.H)
        if single:
            f = hip.gat_backward_drop if new else hip.gat_backward
            f(co, ri, dl, v, *tail, self.att, self.a, self.m, self.Y, self.GY, self.du, self.ds2,
              self.dH, self.dS, GM=self.GM, **bkw)
        else:
            f = hip.gat_backward_heads_drop if new else hip.gat_backward_heads
            f(co, ri, dl, v, *tail, K, self.att, self.a, self.m, self.Y, self.GY, self.du, self.ds2,
              self.dH, self.dS, GM=self.GM, mean=mean, **bkw)
        torch.cuda.synchronize()
        self.K, self.D, self.e, self.s = K, D, e, s

    def outputs(self):
        return {k: getattr(self, k).cpu() for k in ("Y", "m", "a", "du", "ds2", "dS", "dH", "GM")}

    def results(self):
        K, D, e, s = self.K, self.D, self.e, self.s
        dS = self.dS.cpu().double()
        Hh = self.H.cpu().double().view(s, K, D)
        dA1 = torch.einsum("vkd,vk->kd", Hh, dS[:, :K]).reshape(-1)
        dA2 = torch.einsum("vkd,vk->kd", Hh, dS[:, K:]).reshape(-1)
        return dict(Y=self.Y.cpu(), m=self.m.cpu().view(e, K), a=self.a.cpu().view(e, K),
                    dH=self.dH.cpu(), dW_att=torch.cat([dA1, dA2]))


def _inputs(block, K, D, mean, regime, seed):
    F = K * D
    g = torch.Generator().manual_seed(100000 * seed + 1000 * F + 10 * K + 2 * int(mean)
                                      + (regime == "extreme"))
    H = torch.randn(block["s"], F, generator=g)
    sc = 0.3 if regime == "moderate" else 150.0 / (1.4 * D ** 0.5)
    att = torch.randn(2 * F, generator=g) * sc
    GY = torch.randn(block["v"], D if mean else F, generator=g)
    return H, att, GY


def _reference(block, H, att, GY, K, D, mean, keepA, sa, keepF, sf, dtype):
    c = block["cpu"]
    Hd = H.detach().to(dtype).clone().requires_grad_(True)
    ad = att.detach().to(dtype).clone().requires_grad_(True)
    Y, m, a, Z = gdb.drop_chain(Hd, ad, c["column_offset"], c["row_indices"], c["dst_local_id"],
                                K, D, mean, keepA, sa, keepF, sf)
    if GY is not None:
        Y.backward(GY.to(dtype))
    return dict(Y=Y.detach(), m=m.detach(), a=a.detach(), dH=Hd.grad, dW_att=ad.grad,
                Z=Z.detach())


def _near_zero(block, probe, keepA, K, D, mean):
    """(near, share): elements with 0 < |Z| < MASK_EPS, and their share of the
    elements of non-empty rows in which a head keeps LIVE of its attention mass"""
    co = block["cpu"]["column_offset"]
    v = co.numel() - 1
    d_of_e = torch.repeat_interleave(torch.arange(v), (co[1:] - co[:-1]).long())
    mass = torch.zeros(v, K, dtype=torch.float64).index_add(0, d_of_e, probe["a"] * keepA.double())
    live = mass >= LIVE  # [v, K]; an empty row has mass 0
    live = live.any(1, keepdim=True).expand(v, D) if mean else live.repeat_interleave(D, 1)
    Z = probe["Z"]
    near = (Z.abs() < MASK_EPS) & (Z != 0)
    total = int(live.sum())
    return near, int((near & live).sum()), total


def _case_data(hip, block, K, D, mean, regime, q, p, tag):
    v, e = block["v"], block["e"]
    keepA = keep_mask(hip, e, K, q, OFF_A)
    keepF = keep_mask(hip, v, D if mean else K * D, p, OFF_F)
    sa, sf = gdb.scale(q), gdb.scale(p)
    for seed in range(8):  # chosen on the float64 chain alone
        H, att, GY = _inputs(block, K, D, mean, regime, seed)
        probe = _reference(block, H, att, None, K, D, mean, keepA, sa, keepF, sf, torch.float64)
        near, n, total = _near_zero(block, probe, keepA, K, D, mean)
        print(f"{tag} data seed {seed}: 0 < |Z| < {MASK_EPS:g} at {n} of {total} live elements, "
              f"{int(near.sum())} in all")
        if n <= max(MASK_CAP * total, 1):
            break
    else:
        raise AssertionError("no data seed keeps the near-zero share within the cap")
    GY = torch.where(near, torch.zeros(()), GY)
    return H, att, GY, keepA, keepF, sa, sf


@pytest.mark.parametrize("case,rates,regime", RUNS, ids=[f"{c}-{r}-{g}" for c, r, g in RUNS])
def test_dropout_kernels_match_the_float64_chain(hip, block, case, rates, regime):
    K, D, mean, off = (*CASES[case], 0) if case in CASES else CELLS[case]
    q, p = RATES[rates]
    entry = dict(off=off, heads_entry=True if "heads-entry" in case else None)
    tag = f"{case} q={q} p={p} {regime}"
    H, att, GY, keepA, keepF, sa, sf = _case_data(hip, block, K, D, mean, regime, q, p, tag)
    if q:  # the masks are not trivial
        assert 0.3 < float(keepA.float().mean()) < 0.5
    if p:
        assert 0.4 < float(keepF.float().mean()) < 0.6
    r64 = _reference(block, H, att, GY, K, D, mean, keepA, sa, keepF, sf, torch.float64)
    r32 = _reference(block, H, att, GY, K, D, mean, keepA, sa, keepF, sf, torch.float32)
    if regime == "extreme":
        assert float(r64["m"].max()) > 89.0  # float32 exp overflows there
    run = Run(hip, block, H, att, GY, K, D, mean, q, p, **entry)
    got = run.results()
    for k, t in got.items():
        assert bool(torch.isfinite(t).all()), f"{k} has a NaN or inf"
    # exact properties: the dropped outputs are zeros, the kept ones the mask's
    Y = got["Y"]
    assert not Y[~keepF].any()
    gm = torch.where(Y > 0, GY * torch.tensor(sf), torch.zeros(()))
    if mean:
        gm = (gm * (torch.ones(()) / K)).repeat(1, K)
    assert torch.equal(run.GM.cpu(), gm)
    bad = []
    for k in ("Y", "m", "a", "dH", "dW_att"):
        ek, e32 = err(got[k], r64[k]), err(r32[k], r64[k])
        bound = yardstick_bound(e32, C)
        print(f"  RATIO {tag} {k}: err(kernel) {ek:.3e} err(fp32 chain) {e32:.3e} "
              f"ratio {ek / max(e32, 2.0 ** -30):.2f} bound {bound:.3e}")
        if not ek <= bound:
            bad.append(f"{k}: {ek:.3e} > {bound:.3e}")
    if bad:  # does the no-dropout kernel on the same input exceed the bound too?
        ones = dict(keepA=None, sa=1.0, keepF=None, sf=1.0)
        p64 = _reference(block, H, att, GY, K, D, mean, dtype=torch.float64, **ones)
        p32 = _reference(block, H, att, GY, K, D, mean, dtype=torch.float32, **ones)
        plain = Run(hip, block, H, att, GY, K, D, mean, 0.0, 0.0, new=False, **entry).results()
        for k in ("Y", "m", "a", "dH", "dW_att"):
            ek, e32 = err(plain[k], p64[k]), err(p32[k], p64[k])
            print(f"  PLAIN {tag} {k}: err(kernel) {ek:.3e} err(fp32 chain) {e32:.3e} "
                  f"ratio {ek / max(e32, 2.0 ** -30):.2f}")
    assert not bad, "; ".join(bad)
    again = Run(hip, block, H, att, GY, K, D, mean, q, p, **entry).outputs()
    for k, t in run.outputs().items():
        assert torch.equal(t, again[k]), f"{k} differs between two runs"


@pytest.mark.parametrize("case", list(CASES))
def test_zero_rates_are_the_existing_entry_points(hip, block, case):
    K, D, mean = CASES[case]
    H, att, GY = _inputs(block, K, D, mean, "moderate", 0)
    new = Run(hip, block, H, att, GY, K, D, mean, 0.0, 0.0).outputs()
    old = Run(hip, block, H, att, GY, K, D, mean, 0.0, 0.0, new=False).outputs()
    for k in old:
        assert torch.equal(new[k], old[k]), k


@pytest.mark.parametrize("case", ["F67-v1n2", "F260-v4n2-partial", "K8-D8-concat", "K4-D16-mean"])
def test_attention_rate_one_drops_everything(hip, block, case):
    """q = 1: Y = 0 and dH has no aggregation term: dH = ds1 a1 + ds2 a2 with
    ds = 0 too (ga = 0 everywhere), so dH = 0"""
    K, D, mean = CASES[case]
    H, att, GY = _inputs(block, K, D, mean, "moderate", 0)
    out = Run(hip, block, H, att, GY, K, D, mean, 1.0, 0.0).outputs()
    for k in ("Y", "dH", "du", "dS"):
        assert not out[k].any(), k
    assert bool(torch.isfinite(out["a"]).all()) and float(out["a"].max()) > 0


@pytest.mark.parametrize("heads_entry", [False, True])
def test_an_over_wide_row_is_refused_with_the_outputs_untouched(hip, block, heads_entry):
    v, s, e = block["v"], block["s"], block["e"]
    d = block["dev"]
    co, ri, dl = d["column_offset"], d["row_indices"], d["dst_local_id"]
    F = 1028
    H, att = torch.randn(s, F, device=DEV), torch.randn(2 * F, device=DEV)
    outs = {k: torch.full(shape, SENT, device=DEV)
            for k, shape in dict(m=(e,), a=(e,), Y=(v, F), du=(e,), ds2=(s,), dS=(s, 2),
                                 dH=(s, F), GM=(v, F)).items()}
    kw = dict(p_attn=0.6, p_out=0.5, seed=SEED, off_attn=OFF_A)
    GY = torch.randn(v, F, device=DEV)
    tail = (d["row_offset"], d["column_indices"], d["csr_edge_id"], s, H)
    with pytest.raises(RuntimeError, match=r"1024.*256"):
        if heads_entry:
            hip.gat_forward_heads_drop(co, ri, dl, v, H, 1, att, outs["m"], outs["a"], outs["Y"],
                                       off_out=OFF_F, **kw)
        else:
            hip.gat_forward_drop(co, ri, dl, v, H, att, outs["m"], outs["a"], outs["Y"],
                                 off_out=OFF_F, **kw)
    with pytest.raises(RuntimeError, match=r"1024.*256"):
        if heads_entry:
            hip.gat_backward_heads_drop(co, ri, dl, v, *tail, 1, att, outs["a"], outs["m"], outs["Y"],
                                        GY, outs["du"], outs["ds2"], outs["dH"], outs["dS"],
                                        GM=outs["GM"], **kw)
        else:
            hip.gat_backward_drop(co, ri, dl, v, *tail, att, outs["a"], outs["m"], outs["Y"], GY,
                                  outs["du"], outs["ds2"], outs["dH"], outs["dS"], GM=outs["GM"],
                                  **kw)
    # a refused rate, from every entry point, on a width the kernels take
    F = 16
    H, att = torch.randn(s, F, device=DEV), torch.randn(2 * F, device=DEV)
    for bad in (-0.25, float("nan"), 1.5):
        with pytest.raises(RuntimeError, match=r"\[0, 1\]"):
            if heads_entry:
                hip.gat_forward_heads_drop(co, ri, dl, v, H, 1, att, outs["m"], outs["a"],
                                           outs["Y"][:, :F], p_attn=bad)
            else:
                hip.gat_forward_drop(co, ri, dl, v, H, att, outs["m"], outs["a"], outs["Y"][:, :F],
                                     p_out=bad)
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == SENT).all()), k


@pytest.mark.parametrize("F", [1, 7, 602])
@pytest.mark.parametrize("p", [0.5, 0.0, 1.0])
def test_plain_dropout_is_x_times_mask_times_scale(hip, F, p):
    rows, pitch = 37, F + 5
    g = torch.Generator().manual_seed(F)
    x = torch.randn(rows, F, generator=g)
    keep = keep_mask(hip, rows, F, p, 11) if p < 1.0 else torch.zeros(rows, F, dtype=torch.bool)
    want = torch.where(keep, x * torch.tensor(gdb.scale(p), dtype=torch.float32), torch.zeros(()))
    xin = torch.full((rows, pitch), float("nan"), device=DEV)
    xin[:, :F] = x.to(DEV)
    out = torch.full((rows + 1, pitch), SENT, device=DEV)
    hip.dropout(xin[:, :F], out[:rows, :F], p=p, seed=SEED, offset=11)
    torch.cuda.synchronize()
    assert torch.equal(out[:rows, :F].cpu(), want)
    assert bool((out[:rows, F:] == SENT).all()) and bool((out[rows] == SENT).all())
    hip.dropout(xin[:, :F], xin[:, :F], p=p, seed=SEED, offset=11)  # in place
    torch.cuda.synchronize()
    assert torch.equal(xin[:, :F].cpu(), want)
    assert bool(torch.isnan(xin[:, F:]).all())
