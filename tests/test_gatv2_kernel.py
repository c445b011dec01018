"""The GATv2 kernels (csrc/gatv2.hip: k_gatv2_fwd, k_gatv2_bwd_dst,
k_gatv2_bwd_src and the datt reduction) through the wrappers, on the synthetic
block of tests/gat_blocks.py (columns of 0 ... 200 edges, a CSR row of ~95
slots), with the padded, NaN-poisoned inputs and sentinel-filled outputs of
tests/test_gat_heads_kernel.py.

Cases cover every reduction scheme (g = D / VEC lanes per head a power of two
below 64, a multiple of 64, anything else), both vector widths, 1 to 4 chunks
and both output modes, each in the moderate (att = randn * 0.3) and the extreme
(att = randn * 150 / (1.4 sqrt(D))) score regime.  CELLS adds, in concat mode
and the moderate regime, the smallest shape of every (vector width, chunks,
scheme) combination the cases leave out, plain and with dropout, and DROP_HAVE
runs the combinations the cases do have with dropout too, so that each of the
48 forward and backward-per-destination kernels the dispatch can pick is run
in its plain and in its dropout form.

Bound, for each of Y, u, a, dHs, dHd, datt against float64 autograd through the
materialised chain of tests/gatv2_blocks.py, with q32 the same chain in float32:

    err(kernel) <= C * err(q32) + 8 * 2^-24,   C = 8 (tests/step_check.py).

The measured ratios are in DESIGN.md §8n.  Incoming gradients are zeroed where
the float64 pre-activation has |Z| < 1e-4; their number is capped at 1e-3 of the
elements of non-empty rows, or one element, whichever is more.  The leaky kink
needs no mask: the float32 sum of two float32 values has the sign of the exact
sum.
"""
import numpy as np
import pytest
import torch

import gat_blocks
import gat_drop_blocks as gdb
import gatv2_blocks as g2b
from step_check import C, err, yardstick_bound

# (case, regime, quantity) -> constant, where the measured ratio needs more than C
C_EXCEPT = {}

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -12345.5
MASK_EPS, MASK_CAP, LIVE = 1e-4, 1e-3, 0.25
EXTRA_ROWS, EXTRA_E = 3, 64
KEYS = ("Y", "u", "a", "dHs", "dHd", "datt")
SEED, OFF_A, OFF_F = 0x9E3779B97F4A7C15 * 2000 + 1 & (2 ** 64 - 1), 3, (1 << 33) + 7

# id: (K, D, mean, base offset in floats of every row operand)
CASES = {
    "K1-D16-single-head": (1, 16, False, 0),
    "K1-D67-scalar-2-chunks": (1, 67, False, 0),
    "K1-D1024-float4-4-chunks": (1, 1024, False, 0),
    "K8-D8-concat-g2": (8, 8, False, 0),
    "K2-D128-concat-g32": (2, 128, False, 0),
    "K4-D256-concat-chunk-per-head": (4, 256, False, 0),
    "K2-D132-concat-g33": (2, 132, False, 0),
    "K3-D20-concat-g5": (3, 20, False, 0),
    "K5-D51-concat-scalar-straddle": (5, 51, False, 0),
    "K8-D32-concat-base+4B-scalar": (8, 32, False, 1),
    "K8-D7-mean-scalar": (8, 7, True, 0),
    "K4-D16-mean": (4, 16, True, 0),
    "K3-D41-mean-scalar": (3, 41, True, 0),
}
# The (VEC, NCH, MODE) cells of the kernel dispatch that CASES leaves out (g = D / 4
# lanes per head on the float4 path, D on the scalar one; NCH = ceil(K g / 64)):
# concat mode, run in the moderate regime, plain and with the rates (0.3, 0.4).
CELLS = {
    "cell-v4-pow2-n2-K8-D64": (8, 64, False, 0),
    "cell-v4-pow2-n3-K5-D128": (5, 128, False, 0),
    "cell-v4-pow2-n4-K8-D128": (8, 128, False, 0),
    "cell-v4-chunk-n1-K1-D256": (1, 256, False, 0),
    "cell-v4-chunk-n2-K2-D256": (2, 256, False, 0),
    "cell-v4-chunk-n3-K3-D256": (3, 256, False, 0),
    "cell-v4-any-n3-K3-D176": (3, 176, False, 0),
    "cell-v4-any-n4-K4-D208": (4, 208, False, 0),
    "cell-v1-pow2-n1-K8-D8-base+4B": (8, 8, False, 1),
    "cell-v1-pow2-n2-K4-D32-base+4B": (4, 32, False, 1),
    "cell-v1-pow2-n3-K6-D32-base+4B": (6, 32, False, 1),
    "cell-v1-chunk-n1-K1-D64-base+4B": (1, 64, False, 1),
    "cell-v1-chunk-n2-K2-D64-base+4B": (2, 64, False, 1),
    "cell-v1-chunk-n3-K3-D64-base+4B": (3, 64, False, 1),
    "cell-v1-chunk-n4-K4-D64-base+4B": (4, 64, False, 1),
    "cell-v1-any-n3-K3-D51": (3, 51, False, 0),
}
ALL = {**CASES, **CELLS}
RUNS = [(c, r) for r in ("moderate", "extreme") for c in CASES] + [(c, "moderate") for c in CELLS]
DROP_CASES = ["K8-D8-concat-g2", "K5-D51-concat-scalar-straddle", "K4-D16-mean"]
DROP_RATES = {"attn": (0.5, 0.0), "feat": (0.0, 0.5), "both": (0.3, 0.4)}
# every cell of the table with both dropouts: the 16 added CELLS and the cells
# CASES already has plain (K8-D8 and K5-D51 run "both" through DROP_CASES)
DROP_HAVE = ["K4-D256-concat-chunk-per-head", "K3-D20-concat-g5", "K2-D132-concat-g33",
             "K8-D32-concat-base+4B-scalar", "K8-D7-mean-scalar", "K3-D41-mean-scalar"]
DROP_RUNS = ([(c, r) for r in DROP_RATES for c in DROP_CASES] +
             [(c, "both") for c in DROP_HAVE] + [(c, "both") for c in CELLS])


def _pitch(width):
    """a pitch wider than the row that keeps float4 rows aligned where they can be"""
    return width + (4 if width % 4 == 0 else 3)


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=2000)


@pytest.fixture(scope="module")
def block():
    b = gat_blocks.make_block()
    dev = {k: torch.from_numpy(b[k].view(np.int32)).to(DEV)
           for k in ("column_offset", "row_indices", "row_offset", "column_indices", "csr_edge_id")}
    cpu = {k: torch.from_numpy(b[k].astype(np.int64)) for k in ("column_offset", "row_indices")}
    return dict(np=b, dev=dev, cpu=cpu, v=b["v"], s=b["s"], e=b["e"])


def _rows(rows, width, off, fill):
    """(flat, view): rows + EXTRA_ROWS rows of _pitch(width) floats starting `off`
    floats into a fresh allocation, all `fill`"""
    pitch = _pitch(width)
    n = (rows + EXTRA_ROWS) * pitch
    flat = torch.full((n + 4,), fill, device=DEV)
    return flat, flat[off:off + n].view(rows + EXTRA_ROWS, pitch)


def _in_rows(x, off):
    rows, width = x.shape
    _, view = _rows(rows, width, off, float("nan"))
    view[:rows, :width] = x.to(DEV)
    return view[:rows, :width]


def _padding_intact(flat, view, rows, width):
    inside = int((view[:rows, :width] == SENT).sum())
    return int((flat == SENT).sum()) - inside == flat.numel() - rows * width


class Run:
    """One forward + backward through the wrappers on padded buffers."""

    def __init__(self, hip, block, Hs, Hd, att, GY, K, D, mean, off, drop=None):
        v, s, e = block["v"], block["s"], block["e"]
        d = block["dev"]
        F, FY = K * D, (D if mean else K * D)
        self.v, self.s, self.e, self.F, self.FY, self.K = v, s, e, F, FY, K
        self.Hs, self.Hd = _in_rows(Hs, off), _in_rows(Hd, off)
        self.att = torch.full((F + 8,), float("nan"), device=DEV)
        self.att[:F] = att.to(DEV)
        self.u = torch.full((e * K + EXTRA_E,), SENT, device=DEV)
        self.a = torch.full((e * K + EXTRA_E,), SENT, device=DEV)
        self.Yflat, self.Yv = _rows(v, FY, off, SENT)
        Y = self.Yv[:v, :FY]
        co, ri = d["column_offset"], d["row_indices"]
        fkw, bkw = {}, {}
        if drop is not None:
            fkw = dict(p_attn=drop[0], p_out=drop[1], seed=SEED, off_attn=OFF_A, off_out=OFF_F)
            bkw = dict(p_attn=drop[0], p_out=drop[1], seed=SEED, off_attn=OFF_A)
        hip.gatv2_forward(co, ri, v, self.Hs, self.Hd, K, self.att[:F], self.u, self.a, Y,
                          mean=mean, **fkw)
        self.bwd = None
        if GY is None:
            torch.cuda.synchronize()
            return
        self.GY = _in_rows(GY, off)
        self.du = torch.full((e * K + EXTRA_E,), SENT, device=DEV)
        self.datt = torch.full((F + 8,), SENT, device=DEV)
        self.dHsflat, self.dHsv = _rows(s, F, off, SENT)
        self.dHdflat, self.dHdv = _rows(v, F, off, SENT)
        self.GMflat, self.GMv = _rows(v, F, off, SENT)
        hip.gatv2_backward(co, ri, v, d["row_offset"], d["column_indices"], d["csr_edge_id"], s,
                           self.Hs, self.Hd, K, self.att[:F], self.a, Y, self.GY, self.du,
                           self.dHsv[:s, :F], self.dHdv[:v, :F], self.datt,
                           GM=self.GMv[:v, :F], mean=mean, **bkw)
        torch.cuda.synchronize()
        self.bwd = True

    def outputs(self):
        out = dict(Y=self.Yflat, u=self.u, a=self.a)
        if self.bwd:
            out.update(du=self.du, datt=self.datt, dHs=self.dHsflat, dHd=self.dHdflat,
                       GM=self.GMflat)
        return {k: t.cpu() for k, t in out.items()}

    def assert_untouched(self):
        v, s, e, F, FY, K = self.v, self.s, self.e, self.F, self.FY, self.K
        assert _padding_intact(self.Yflat, self.Yv, v, FY), "Y: rows past v_size or padding written"
        assert bool((self.u[e * K:] == SENT).all()) and bool((self.a[e * K:] == SENT).all()), \
            "u / a past e K"
        if self.bwd:
            assert bool((self.du[e * K:] == SENT).all()), "du past e K"
            assert bool((self.datt[F:] == SENT).all()), "datt past F"
            assert _padding_intact(self.dHsflat, self.dHsv, s, F), "dHs: past src_size or padding"
            assert _padding_intact(self.dHdflat, self.dHdv, v, F), "dHd: past v_size or padding"
            assert _padding_intact(self.GMflat, self.GMv, v, F), "GM: past v_size or padding"

    def results(self):
        v, s, e, F, FY, K = self.v, self.s, self.e, self.F, self.FY, self.K
        got = dict(Y=self.Yv[:v, :FY].cpu(), u=self.u[:e * K].cpu().view(e, K),
                   a=self.a[:e * K].cpu().view(e, K))
        if self.bwd:
            got.update(dHs=self.dHsv[:s, :F].cpu(), dHd=self.dHdv[:v, :F].cpu(),
                       datt=self.datt[:F].cpu())
        return got


def _inputs(block, K, D, mean, regime):
    F = K * D
    g = torch.Generator().manual_seed(2000 * F + 10 * K + 2 * int(mean) + (regime == "extreme"))
    Hs = torch.randn(block["s"], F, generator=g)
    Hd = torch.randn(block["v"], F, generator=g)
    scale = 0.3 if regime == "moderate" else 150.0 / (1.4 * D ** 0.5)
    att = torch.randn(F, generator=g) * scale
    GY = torch.randn(block["v"], D if mean else F, generator=g)
    return Hs, Hd, att, GY


def _reference(block, Hs, Hd, att, GY, K, D, mean, dtype, keepA=None, sa=1.0, keepF=None, sf=1.0):
    c = block["cpu"]
    hs = Hs.detach().to(dtype).clone().requires_grad_(True)
    hd = Hd.detach().to(dtype).clone().requires_grad_(True)
    ad = att.detach().to(dtype).clone().requires_grad_(True)
    Z, u, a = g2b.v2_chain_z(hs, hd, ad, c["column_offset"], c["row_indices"], K, D, mean,
                             keepA=keepA, sa=sa)
    Y = torch.relu(Z)
    Y = Y * sf if keepF is None else Y * keepF.to(dtype) * sf
    if GY is not None:
        Y.backward(GY.to(dtype))
    return dict(Y=Y.detach(), u=u.detach(), a=a.detach(), dHs=hs.grad, dHd=hd.grad, datt=ad.grad,
                Z=Z.detach())


def _masked_gy(block, Hs, Hd, att, GY, K, D, mean, tag):
    """GY zeroed where the float64 pre-activation is within MASK_EPS of 0"""
    co = block["cpu"]["column_offset"]
    probe = _reference(block, Hs, Hd, att, None, K, D, mean, torch.float64)
    nonempty = (co[1:] > co[:-1])[:, None]
    near = (probe["Z"].abs() < MASK_EPS) & nonempty
    total = int(nonempty.sum()) * probe["Z"].shape[1]
    print(f"{tag}: |Z| < {MASK_EPS:g} at {int(near.sum())} of {total} elements of non-empty rows "
          f"({int(near.sum()) / total:.2e})")
    assert int(near.sum()) <= max(MASK_CAP * total, 1)
    return torch.where(near, torch.zeros(()), GY)


def _check_bound(got, r64, r32, case, regime, keys=KEYS):
    bad = []
    for k in keys:
        ek, e32 = err(got[k], r64[k]), err(r32[k], r64[k])
        bound = yardstick_bound(e32, C_EXCEPT.get((case, regime, k), C))
        print(f"  {k}: err(kernel) {ek:.3e} err(fp32 chain) {e32:.3e} "
              f"ratio {ek / max(e32, 2.0 ** -30):.2f} bound {bound:.3e}")
        if not ek <= bound:
            bad.append(f"{k}: {ek:.3e} > {bound:.3e}")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("case,regime", RUNS, ids=[f"{c}-{r}" for c, r in RUNS])
def test_v2_kernels_match_the_float64_chain(hip, block, case, regime):
    """Y, u, a, dHs, dHd and datt within C times the float32 chain's own error
    (measured ratios: DESIGN.md §8n), with the exact properties of empty
    columns, untouched padding and run-to-run bit identity."""
    K, D, mean, off = ALL[case]
    F = K * D
    v, s, e = block["v"], block["s"], block["e"]
    Hs, Hd, att, GY = _inputs(block, K, D, mean, regime)
    GY = _masked_gy(block, Hs, Hd, att, GY, K, D, mean, f"{case} {regime}")
    r64 = _reference(block, Hs, Hd, att, GY, K, D, mean, torch.float64)
    r32 = _reference(block, Hs, Hd, att, GY, K, D, mean, torch.float32)
    if regime == "extreme":
        print(f"  scores {float(r64['u'].min()):.1f} ... {float(r64['u'].max()):.1f}")
        assert float(r64["u"].max()) > 89.0  # float32 exp overflows there

    run = Run(hip, block, Hs, Hd, att, GY, K, D, mean, off)
    run.assert_untouched()
    got = run.results()
    for k, t in got.items():
        assert bool(torch.isfinite(t).all()), f"{k} has a NaN or inf"
    assert bool(torch.isfinite(run.du[:e * K]).all())
    Y, a = got["Y"], got["a"]

    co = block["np"]["column_offset"].astype(np.int64)
    deg = np.diff(co)
    for d in np.flatnonzero(deg == 1):
        assert bool((a[co[d]] == 1.0).all())
    for d in np.flatnonzero(deg == 0):  # empty columns: zero rows
        assert not Y[d].any()
        assert not got["dHd"][d].any()
    # each head's attention sums to 1 over every non-empty column
    d_of_e = np.repeat(np.arange(v), deg)
    for h in range(K):
        sums = np.bincount(d_of_e, weights=a[:, h].double().numpy(), minlength=v)
        assert np.all(np.abs(sums - 1.0)[deg > 0] <= deg[deg > 0] * 2.0 ** -23)
    # GM: GY (mean: GY times float32(1 / K), for every head) under the relu mask
    gm = torch.where(Y > 0, GY, torch.zeros(()))
    if mean:
        gm = (gm * (torch.ones(()) / K)).repeat(1, K)
    assert torch.equal(run.GMv[:v, :F].cpu(), gm)

    _check_bound(got, r64, r32, case, regime)

    again = Run(hip, block, Hs, Hd, att, GY, K, D, mean, off)
    first, second = run.outputs(), again.outputs()
    for k in first:
        assert torch.equal(first[k], second[k]), f"{k} differs between two runs"


@pytest.mark.parametrize("case", ["K8-D8-concat-g2", "K5-D51-concat-scalar-straddle", "K4-D16-mean"])
def test_zero_attention_is_uniform(hip, block, case):
    """att = 0: every score is 0 and a[e, h] = float32(1) / float32(deg) bit for
    bit for every head; Y is the relu of the float32 mean in edge order."""
    K, D, mean, off = CASES[case]
    F = K * D
    v, e = block["v"], block["e"]
    Hs, Hd, _, _ = _inputs(block, K, D, mean, "moderate")
    run = Run(hip, block, Hs, Hd, torch.zeros(F), None, K, D, mean, off)
    run.assert_untouched()
    b = block["np"]
    co, ri = b["column_offset"].astype(np.int64), b["row_indices"].astype(np.int64)
    u = run.u[:e * K].cpu().numpy().reshape(e, K)
    a = run.a[:e * K].cpu().numpy().reshape(e, K)
    Y = run.Yv[:v, :(D if mean else F)].cpu().numpy()
    assert not u.any()
    Hn = Hs.numpy()
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
        z = acc * inv
        if mean:
            t = z[:D].copy()
            for h in range(1, K):
                t = t + z[h * D:(h + 1) * D]
            z = t * (np.float32(1) / np.float32(K))
        assert np.array_equal(Y[d], np.maximum(z, np.float32(0))), d


def keep_mask(hip, rows, cols, p, offset):
    """[rows, cols] bool: what relu_dropout keeps of a ones tensor"""
    if p == 0.0:
        return torch.ones(rows, cols, dtype=torch.bool)
    y = torch.empty(rows, cols, device=DEV)
    hip.relu_dropout(torch.ones(rows, cols, device=DEV), y, p=p, seed=SEED, offset=offset)
    return (y > 0).cpu()


@pytest.mark.parametrize("case,rates", DROP_RUNS, ids=[f"{c}-{r}" for c, r in DROP_RUNS])
def test_dropout_matches_the_masked_chain(hip, block, case, rates):
    """Attention and output dropout against the chain with the masks that
    relu_dropout leaves of a ones tensor at the same key and offsets (element
    (e, h) at off_attn, element (d, c) of Y at off_out).  GY is zeroed where
    0 < |Z| < 1e-4; the cap on their share counts the rows in which a head keeps
    a quarter of its attention mass, as tests/test_gat_dropout_kernel.py does."""
    K, D, mean, off = ALL[case]
    q, p = DROP_RATES[rates]
    F, FY = K * D, (D if mean else K * D)
    v, e = block["v"], block["e"]
    Hs, Hd, att, GY = _inputs(block, K, D, mean, "moderate")
    keepA, keepF = keep_mask(hip, e, K, q, OFF_A), keep_mask(hip, v, FY, p, OFF_F)
    sa, sf = gdb.scale(q), gdb.scale(p)
    kw = dict(keepA=keepA, sa=sa, keepF=keepF, sf=sf)
    probe = _reference(block, Hs, Hd, att, None, K, D, mean, torch.float64, **kw)
    co = block["cpu"]["column_offset"]
    d_of_e = torch.repeat_interleave(torch.arange(v), (co[1:] - co[:-1]).long())
    mass = torch.zeros(v, K, dtype=torch.float64).index_add(0, d_of_e, probe["a"] * keepA.double())
    live = mass >= LIVE
    live = live.any(1, keepdim=True).expand(v, D) if mean else live.repeat_interleave(D, 1)
    near = (probe["Z"].abs() < MASK_EPS) & (probe["Z"] != 0)
    n, total = int((near & live).sum()), int(live.sum())
    print(f"{case} q={q} p={p}: 0 < |Z| < {MASK_EPS:g} at {n} of {total} live elements")
    assert n <= max(MASK_CAP * total, 1)
    GY = torch.where(near, torch.zeros(()), GY)
    r64 = _reference(block, Hs, Hd, att, GY, K, D, mean, torch.float64, **kw)
    r32 = _reference(block, Hs, Hd, att, GY, K, D, mean, torch.float32, **kw)
    run = Run(hip, block, Hs, Hd, att, GY, K, D, mean, off, drop=(q, p))
    run.assert_untouched()
    got = run.results()
    assert bool(((got["Y"] != 0) <= keepF).all()), "an output element outside the keep mask"
    _check_bound(got, r64, r32, case, f"drop-{q}-{p}")
    again = Run(hip, block, Hs, Hd, att, GY, K, D, mean, off, drop=(q, p))
    first, second = run.outputs(), again.outputs()
    for k in first:
        assert torch.equal(first[k], second[k]), f"{k} differs between two runs"


@pytest.mark.parametrize("case", ["K8-D8-concat-g2", "K5-D51-concat-scalar-straddle", "K4-D16-mean"])
def test_zero_rates_give_the_plain_bytes(hip, block, case):
    K, D, mean, off = CASES[case]
    Hs, Hd, att, GY = _inputs(block, K, D, mean, "moderate")
    plain = Run(hip, block, Hs, Hd, att, GY, K, D, mean, off).outputs()
    zero = Run(hip, block, Hs, Hd, att, GY, K, D, mean, off, drop=(0.0, 0.0)).outputs()
    for k in plain:
        assert torch.equal(plain[k], zero[k]), k


@pytest.mark.parametrize("K,D,rates", [(0, 16, None), (257, 4, None), (1, 257, None), (2, 130, None),
                                       (2, 16, (-0.1, 0.0)), (2, 16, (0.0, 1.5)),
                                       (2, 16, (float("nan"), 0.0))],
                         ids=["heads0", "F1028", "F257-scalar", "K2-D130-aligned", "rate-negative",
                              "rate-above-1", "rate-nan"])
def test_refused_calls_write_nothing(hip, block, K, D, rates):
    """heads = 0, F = 1028 (257 heads of 4: float4-eligible), F = 257 (scalar),
    (2, 130) on aligned rows (D % 4 != 0: scalar, F = 260) and rates outside
    [0, 1] are errors that state the limits, from the forward and from the
    backward, and no output is written."""
    v, s, e = block["v"], block["s"], block["e"]
    d = block["dev"]
    co, ri = d["column_offset"], d["row_indices"]
    Kb = max(K, 1)
    F = Kb * D
    Hs, Hd = _in_rows(torch.randn(s, F), 0), _in_rows(torch.randn(v, F), 0)
    att = torch.randn(F, device=DEV)
    u = torch.full((e * Kb,), SENT, device=DEV)
    a = torch.full((e * Kb,), SENT, device=DEV)
    Yflat, Yv = _rows(v, F, 0, SENT)
    kw = {} if rates is None else dict(p_attn=rates[0], p_out=rates[1])
    msg = (r"dropout probability must be in \[0, 1\]" if rates is not None
           else r"heads must be >= 1" if K == 0 else r"1024.*256")
    with pytest.raises(RuntimeError, match=msg):
        hip.gatv2_forward(co, ri, v, Hs, Hd, K, att, u, a, Yv[:v, :F], **kw)
    torch.cuda.synchronize()
    for t in (u, a, Yflat):
        assert bool((t == SENT).all())
    GY = _in_rows(torch.randn(v, F), 0)
    du = torch.full((e * Kb,), SENT, device=DEV)
    datt = torch.full((F,), SENT, device=DEV)
    dHsflat, dHsv = _rows(s, F, 0, SENT)
    dHdflat, dHdv = _rows(v, F, 0, SENT)
    GMflat, GMv = _rows(v, F, 0, SENT)
    with pytest.raises(RuntimeError, match=msg):
        hip.gatv2_backward(co, ri, v, d["row_offset"], d["column_indices"], d["csr_edge_id"], s,
                           Hs, Hd, K, att, a, Yv[:v, :F], GY, du, dHsv[:s, :F], dHdv[:v, :F], datt,
                           GM=GMv[:v, :F], **kw)
    torch.cuda.synchronize()
    for t in (du, datt, dHsflat, dHdflat, GMflat):
        assert bool((t == SENT).all())
