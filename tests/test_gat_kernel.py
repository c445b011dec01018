"""The three GAT kernels (csrc/gat.hip) past one chunk, on the synthetic block of
tests/gat_blocks.py: columns of 0 ... 200 edges and a CSR row of ~95 slots, so
the 64-edge chunk loops of k_gat_fwd, k_gat_bwd_dst and k_gat_bwd_src iterate,
the running max / sum is carried, and the parked m / du are read back from a
later chunk.

Widths cover every (VEC, NCH) instantiation gat_dispatch can pick, each in two
score regimes: moderate (att = randn * 0.3) and extreme (att = randn * 150 /
(1.4 sqrt(F)): post-leaky scores from about -100 to several hundred, where a
plain exp overflows and the attention is nearly one-hot).

Bound.  For each quantity q of (Y, m, a, dH, dW_att), with err(x) = max|x -
q64| / max|q64| against float64 autograd through the materialised chain, and
q32 the same chain in float32 torch:

    err(kernel) <= C * err(q32) + 8 * 2^-24.

C = 8 (tests/step_check.py) is one constant: the smallest power of two at least
twice the largest err(kernel) / err(q32) measured on an MI355X over every case
and quantity (the table is in DESIGN.md, "GAT kernels: measured error against
the float32 chain"; the largest ratio is 2.52, Y at F = 255 with extreme
scores, most are below 1).  A chunk-boundary or rescale bug shows as 1e-3 or
worse.

Incoming gradients are zeroed where the float64 pre-activation has |Z| < 1e-4
(the relu mask could differ there); their share is asserted <= 0.1 %.

Every row operand is allocated with extra rows and a pitch wider than F: the
padding of the inputs is NaN (an over-read poisons the result), the padding of
the outputs, the rows past v_size / src_size and the entries past e hold a
sentinel that must survive.
"""
import numpy as np
import pytest
import torch

import gat_blocks
from step_check import C, err, yardstick_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -12345.5
MASK_EPS, MASK_CAP = 1e-4, 1e-3
EXTRA_ROWS, EXTRA_E = 3, 64

# id: (F, pitch, base offset in floats of the forward's rows, of GY alone)
LAYOUTS = {
    "F16-v4n1": (16, 20, 0, 0),
    "F260-v4n2-partial": (260, 264, 0, 0),
    "F516-v4n3": (516, 520, 0, 0),
    "F1024-v4n4-full": (1024, 1028, 0, 0),
    "F33-v1n1": (33, 36, 0, 0),
    "F67-v1n2": (67, 70, 0, 0),
    "F130-v1n3": (130, 133, 0, 0),
    "F255-v1n4": (255, 258, 0, 0),
    "F256-v1n4-base+4B": (256, 260, 1, 1),
    "F256-v1n4-pitch258": (256, 258, 0, 0),
    # the backward alone on the scalar path (GY misaligned): forward VEC 4 NCH 1
    "F256-fwd-v4n1-bwd-v1n4": (256, 260, 0, 1),
}


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
    return dict(np=b, dev=dev, cpu=cpu, v=b["v"], s=b["s"], e=b["e"])


def _rows(rows, F, pitch, off, fill):
    """(flat, view): rows + EXTRA_ROWS rows of `pitch` floats starting `off`
    floats into a fresh allocation, all `fill`; view is [rows + EXTRA_ROWS, pitch]"""
    n = (rows + EXTRA_ROWS) * pitch
    flat = torch.full((n + 4,), fill, device=DEV)
    return flat, flat[off:off + n].view(rows + EXTRA_ROWS, pitch)


def _in_rows(x, pitch, off):
    """x on the device in a NaN-padded allocation; returns the [rows, F] view"""
    rows, F = x.shape
    _, view = _rows(rows, F, pitch, off, float("nan"))
    view[:rows, :F] = x.to(DEV)
    return view[:rows, :F]


def _padding_intact(flat, view, rows, F):
    """everything of the allocation but view[:rows, :F] still holds the sentinel:
    the floats before and after the rows, the rows past `rows`, the columns past F"""
    inside = int((view[:rows, :F] == SENT).sum())
    return int((flat == SENT).sum()) - inside == flat.numel() - rows * F


class Run:
    """One forward + backward through the wrappers on padded buffers."""

    def __init__(self, hip, block, H, att, GY, pitch, off, off_g):
        v, s, e = block["v"], block["s"], block["e"]
        d = block["dev"]
        F = H.shape[1]
        self.v, self.s, self.e, self.F = v, s, e, F
        self.H = _in_rows(H, pitch, off)
        self.att = att.to(DEV)
        self.m = torch.full((e + EXTRA_E,), SENT, device=DEV)
        self.a = torch.full((e + EXTRA_E,), SENT, device=DEV)
        self.Yflat, self.Yv = _rows(v, F, pitch, off, SENT)
        Y = self.Yv[:v, :F]
        co, ri, dl = d["column_offset"], d["row_indices"], d["dst_local_id"]
        hip.gat_forward(co, ri, dl, v, self.H, self.att, self.m, self.a, Y)
        self.bwd = None
        if GY is None:
            torch.cuda.synchronize()
            return
        self.GY = _in_rows(GY, pitch, off_g)
        self.du = torch.full((e + EXTRA_E,), SENT, device=DEV)
        self.ds2 = torch.full((s + 8,), SENT, device=DEV)
        self.dS = torch.full((s + 8, 2), SENT, device=DEV)
        self.dHflat, self.dHv = _rows(s, F, pitch, off, SENT)
        self.GMflat, self.GMv = _rows(v, F, pitch, off, SENT)
        hip.gat_backward(co, ri, dl, v, d["row_offset"], d["column_indices"], d["csr_edge_id"], s,
                         self.H, self.att, self.a, self.m, Y, self.GY, self.du, self.ds2,
                         self.dHv[:s, :F], self.dS, GM=self.GMv[:v, :F])
        torch.cuda.synchronize()
        self.bwd = True

    def outputs(self):
        """every output buffer whole (padding included), for bit comparisons"""
        out = dict(Y=self.Yflat, m=self.m, a=self.a)
        if self.bwd:
            out.update(du=self.du, ds2=self.ds2, dS=self.dS, dH=self.dHflat, GM=self.GMflat)
        return {k: t.cpu() for k, t in out.items()}

    def assert_untouched(self):
        v, s, e, F = self.v, self.s, self.e, self.F
        assert _padding_intact(self.Yflat, self.Yv, v, F), "Y: rows past v_size or padding written"
        assert bool((self.m[e:] == SENT).all()) and bool((self.a[e:] == SENT).all()), "m / a past e"
        if self.bwd:
            assert bool((self.du[e:] == SENT).all()), "du past e"
            assert bool((self.ds2[s:] == SENT).all()) and bool((self.dS[s:] == SENT).all())
            assert _padding_intact(self.dHflat, self.dHv, s, F), "dH: rows past src_size or pitch padding written"
            assert _padding_intact(self.GMflat, self.GMv, v, F), "GM: rows past v_size or pitch padding written"


def _inputs(block, F, regime):
    g = torch.Generator().manual_seed(1000 * F + (regime == "extreme"))
    H = torch.randn(block["s"], F, generator=g)
    scale = 0.3 if regime == "moderate" else 150.0 / (1.4 * F ** 0.5)
    att = torch.randn(2 * F, generator=g) * scale
    GY = torch.randn(block["v"], F, generator=g)
    return H, att, GY


def _reference(block, H, att, GY, dtype):
    """the chain and its autograd in `dtype`: dict of Y, m, a, dH, dW_att, Z"""
    c = block["cpu"]
    F = H.shape[1]
    Hd = H.to(dtype).requires_grad_(True)
    ad = att.to(dtype).requires_grad_(True)
    Z, m, a = gat_blocks.gat_chain_z(Hd, ad, c["column_offset"], c["row_indices"],
                                     c["dst_local_id"], F)
    Y = torch.relu(Z)
    Y.backward(GY.to(dtype))
    return dict(Y=Y.detach(), m=m.detach(), a=a.detach(), dH=Hd.grad, dW_att=ad.grad,
                Z=Z.detach())


@pytest.mark.parametrize("regime", ["moderate", "extreme"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_gat_kernels_match_the_float64_chain(hip, block, layout, regime):
    """Y, m, a, dH and dW_att of the kernels within C times the float32 chain's
    own error of float64 autograd (measured ratios: DESIGN.md, "GAT kernels:
    measured error against the float32 chain"; the largest is 2.52, C = 8), on
    every (VEC, NCH) path and in both score regimes; with the exact properties
    of degenerate columns, untouched padding and run-to-run bit identity."""
    F, pitch, off, off_g = LAYOUTS[layout]
    v, s, e = block["v"], block["s"], block["e"]
    H, att, GY = _inputs(block, F, regime)
    probe = _reference(block, H, att, GY, torch.float64)
    # (an empty column's Z is exactly 0 in every implementation: the mask is
    # certain there, nothing to exclude)
    nonempty = (block["cpu"]["column_offset"][1:] > block["cpu"]["column_offset"][:-1])[:, None]
    near = (probe["Z"].abs() < MASK_EPS) & nonempty
    share = float(near.float().mean())
    print(f"{layout} {regime}: |Z| < {MASK_EPS:g} at {int(near.sum())} of {near.numel()} "
          f"elements ({share:.2e})")
    assert share <= MASK_CAP
    GY = torch.where(near, torch.zeros(()), GY)
    r64 = _reference(block, H, att, GY, torch.float64)
    r32 = _reference(block, H, att, GY, torch.float32)
    if regime == "extreme":
        print(f"  post-leaky scores {float(r64['m'].min()):.1f} ... {float(r64['m'].max()):.1f}")
        assert float(r64["m"].max()) > 89.0  # float32 exp overflows there

    run = Run(hip, block, H, att, GY, pitch, off, off_g)
    run.assert_untouched()
    Y = run.Yv[:v, :F].cpu()
    m, a = run.m[:e].cpu(), run.a[:e].cpu()
    dH = run.dHv[:s, :F].cpu()
    dS = run.dS[:s].cpu().double()
    got = dict(Y=Y, m=m, a=a, dH=dH,
               dW_att=torch.cat([H.double().t() @ dS[:, 0], H.double().t() @ dS[:, 1]]))
    for k, t in got.items():
        assert bool(torch.isfinite(t).all()), f"{k} has a NaN or inf"
    assert bool(torch.isfinite(run.du[:e]).all()) and bool(torch.isfinite(run.ds2[:s]).all())

    # degenerate columns, exactly
    b = block["np"]
    co = b["column_offset"].astype(np.int64)
    ri, dl = b["row_indices"].astype(np.int64), b["dst_local_id"].astype(np.int64)
    deg = np.diff(co)
    for d in np.flatnonzero(deg == 1):
        assert float(a[co[d]]) == 1.0
        assert torch.equal(Y[d], torch.relu(H[ri[co[d]]]))
    for d in np.flatnonzero(deg == 0):
        assert not Y[d].any()
        assert float(run.ds2[dl[d]]) == 0.0
    # ds2 is zero off the destinations
    rest = np.setdiff1d(np.arange(s), dl)
    assert not run.ds2[torch.from_numpy(rest).to(DEV)].any()
    assert torch.equal(run.dS[:s, 1], run.ds2[:s])
    # each non-empty column's attention sums to 1
    d_of_e = np.repeat(np.arange(v), deg)
    sums = np.bincount(d_of_e, weights=a.double().numpy(), minlength=v)
    assert np.all(np.abs(sums - 1.0)[deg > 0] <= deg[deg > 0] * 2.0 ** -23)
    # GM is GY under the relu mask
    assert torch.equal(run.GMv[:v, :F].cpu(), torch.where(Y > 0, GY, torch.zeros(())))

    # the yardstick bound
    bad = []
    for k in ("Y", "m", "a", "dH", "dW_att"):
        ek, e32 = err(got[k], r64[k]), err(r32[k], r64[k])
        bound = yardstick_bound(e32, C)
        print(f"  {k}: err(kernel) {ek:.3e} err(fp32 chain) {e32:.3e} "
              f"ratio {ek / max(e32, 2.0 ** -30):.2f} bound {bound:.3e}")
        if not ek <= bound:
            bad.append(f"{k}: {ek:.3e} > {bound:.3e}")
    assert not bad, "; ".join(bad)

    # forward and backward, run again on fresh buffers: bit-identical everywhere
    again = Run(hip, block, H, att, GY, pitch, off, off_g)
    first, second = run.outputs(), again.outputs()
    for k in first:
        assert torch.equal(first[k], second[k]), f"{k} differs between two runs"


@pytest.mark.parametrize("layout", ["F16-v4n1", "F260-v4n2-partial", "F255-v1n4"])
def test_zero_attention_is_the_float32_mean(hip, block, layout):
    """att = 0: every score is 0, the attention is float32(1) / float32(deg) bit
    for bit, and Y is the relu of the float32 mean (the sum in edge order, times
    that reciprocal), across chunks too."""
    F, pitch, off, off_g = LAYOUTS[layout]
    v, e = block["v"], block["e"]
    H, _, _ = _inputs(block, F, "moderate")
    run = Run(hip, block, H, torch.zeros(2 * F), None, pitch, off, off_g)
    run.assert_untouched()
    b = block["np"]
    co, ri = b["column_offset"].astype(np.int64), b["row_indices"].astype(np.int64)
    m, a, Y = run.m[:e].cpu().numpy(), run.a[:e].cpu().numpy(), run.Yv[:v, :F].cpu().numpy()
    assert not m.any()
    Hn = H.numpy()
    for d in range(v):
        n = int(co[d + 1] - co[d])
        if n == 0:
            assert not Y[d].any()
            continue
        inv = np.float32(1) / np.float32(n)
        assert np.all(a[co[d]:co[d + 1]] == inv), d
        acc = np.zeros(F, np.float32)
        for j in range(co[d], co[d + 1]):
            acc = acc + Hn[ri[j]]
        ref = np.maximum(acc * inv, np.float32(0))
        assert np.array_equal(Y[d], ref), d


@pytest.mark.parametrize("F,pitch,off", [(1028, 1028, 0), (257, 260, 0), (260, 260, 1)],
                         ids=["F1028", "F257", "F260-base+4B"])
def test_too_wide_is_refused_and_writes_nothing(hip, block, F, pitch, off):
    """More than 4 vectors per lane (F > 1024 on the float4 path, F > 256 on the
    scalar one) is an error that names the limit, from the forward and from the
    backward, and no output is written (the backward's clearing of ds2 included)."""
    v, s, e = block["v"], block["s"], block["e"]
    d = block["dev"]
    co, ri, dl = d["column_offset"], d["row_indices"], d["dst_local_id"]
    H = _in_rows(torch.randn(s, F), pitch, off)
    att = torch.randn(2 * F, device=DEV)
    m = torch.full((e,), SENT, device=DEV)
    a = torch.full((e,), SENT, device=DEV)
    Yflat, Yv = _rows(v, F, pitch, off, SENT)
    with pytest.raises(RuntimeError, match=r"1024.*256"):
        hip.gat_forward(co, ri, dl, v, H, att, m, a, Yv[:v, :F])
    torch.cuda.synchronize()
    for t in (m, a, Yflat):
        assert bool((t == SENT).all())
    GY = _in_rows(torch.randn(v, F), pitch, off)
    du = torch.full((e,), SENT, device=DEV)
    ds2 = torch.full((s,), SENT, device=DEV)
    dS = torch.full((s, 2), SENT, device=DEV)
    dHflat, dHv = _rows(s, F, pitch, off, SENT)
    GMflat, GMv = _rows(v, F, pitch, off, SENT)
    with pytest.raises(RuntimeError, match=r"1024.*256"):
        hip.gat_backward(co, ri, dl, v, d["row_offset"], d["column_indices"], d["csr_edge_id"], s,
                         H, att, a, m, Yv[:v, :F], GY, du, ds2, dHv[:s, :F], dS, GM=GMv[:v, :F])
    torch.cuda.synchronize()
    for t in (du, ds2, dS, dHflat, GMflat):
        assert bool((t == SENT).all())
