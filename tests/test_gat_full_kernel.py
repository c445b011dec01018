"""nts_hip_gat_scores and nts_hip_gat_graph_fwd (csrc/infer.hip): the GAT layer
over the whole graph, one fused attention pass, against the float64 chain.

Graph (V = 2,000), that of tests/test_full_infer_kernel.py rebuilt here: ~60,000
random edges, a 20,000-edge hub into vertex 0 (duplicates and self-loops
included), rows of in-degree exactly 64 / 65 (one full id chunk of a 64-lane
group, and one more) and 2,048 / 2,049 (the last row a single lane group walks,
and the first column-sliced hub), and three vertices without in-edges.

Reference: gat_heads_blocks.heads_chain(H, att, co, ri, arange(V), K, D, mean)
in float64; the yardstick q32 is the same chain in float32.  With
err(x) = max|x - q64| / max|q64| the project's rule is

    err(kernel) <= C * err(q32) + 8 * 2^-24,   C = step_check.C = 8,

for Y over all rows, and for S against H @ [a1 | a2] per head (float64;
yardstick: the same product in float32).  The forward is continuous through the
relu, so no element is excluded.

The hub row (0) and the 64 / 65 / 2,048 / 2,049 rows are also held to the rule
on their own (err and the yardstick's err both taken over that row alone), so
that a slicing bug cannot hide in a maximum over all rows.  A single row's
yardstick error is a maximum over as few as 7 elements and can be half an ulp
by luck, so these ratios scatter more; by §8b's own rule (the smallest power
of two at least twice the largest measured ratio) their constant is
C_ROW = 16.  A wrong slice or a lost rescaling shows as 1e-2 or worse.

Measured on an MI355X (the table is in DESIGN.md §8k; padded and unpadded
pitches give the same figures): the largest ratio err(kernel) / err(q32) is
2.94 for Y over all rows (K8-D7 mean, moderate scores), 1.00 for S (K1-D16,
extreme scores), both below 4, so C stays 8 for them; and 5.94 for a row on its
own (row 11, 65 edges, K8-D7 mean, moderate scores: err(kernel) 3.9e-7 against
err(q32) 6.6e-8), hence C_ROW = 16.

Shapes (K, D): the smallest that reach every path of the dispatch --
(1, 16) float4 on 8-lane groups, several rows a wave; (1, 41) scalar; (8, 8)
float4, eight heads inside one 16-lane group; (2, 33) scalar, a head ending
inside a slice; (4, 64) one full 64-lane float4 slice; (1, 300) one head across
two slices; (8, 128) F = 1,024: four slices of two heads; (8, 7) mean, scalar;
(4, 16) mean, float4; and (3, 6) the float2 path (D even, not a multiple of 4).
Each with moderate (att = randn * 0.3) and extreme (att = randn * 150 /
(1.4 sqrt(D)): a plain exp overflows, the 20,000-edge hub stresses the
rescaling) scores, on padded (NaN in the input padding) and unpadded pitches.
"""
import numpy as np
import pytest
import torch

import gat_heads_blocks as ghb
from step_check import C, yardstick_bound

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

V = 2000
EMPTY = (1, 777, V - 1)
EXACT = {10: 64, 11: 65, 12: 2048, 13: 2049}
OWN_ROWS = (0, 10, 11, 12, 13)
C_ROW = 16  # the rows held on their own (see above); Y over all rows and S: C
SENT = -12345.5
EXTRA_ROWS = 3

# id: (K, D, mean)
CASES = {
    "K1-D16-float4-8-lanes": (1, 16, False),
    "K1-D41-scalar": (1, 41, False),
    "K8-D8-float4-heads-in-a-group": (8, 8, False),
    "K2-D33-scalar-head-ends-in-a-slice": (2, 33, False),
    "K4-D64-float4-one-slice": (4, 64, False),
    "K1-D300-head-across-slices": (1, 300, False),
    "K8-D128-four-slices": (8, 128, False),
    "K8-D7-mean-scalar": (8, 7, True),
    "K4-D16-mean-float4": (4, 16, True),
    "K3-D6-float2": (3, 6, False),
}


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=2000)


@pytest.fixture(scope="module")
def graph():
    from nts.hip import DeviceGraph
    rng = np.random.default_rng(11)
    fixed = set(EMPTY) | set(EXACT)
    allowed = np.array([v for v in range(V) if v not in fixed], np.int64)
    src = [rng.integers(0, V, 60000)]
    dst = [allowed[rng.integers(0, allowed.size, 60000)]]
    src.append(rng.integers(0, V, 20000))  # the hub (self-loops, duplicates)
    dst.append(np.zeros(20000, np.int64))
    for v, n in EXACT.items():
        src.append(rng.integers(0, V, n))
        dst.append(np.full(n, v, np.int64))
    src, dst = np.concatenate(src), np.concatenate(dst)
    perm = rng.permutation(src.size)  # file order: the rows' edges interleaved
    src, dst = src[perm], dst[perm]
    order = np.argsort(dst, kind="stable")
    ri = src[order]
    deg = np.bincount(dst, minlength=V)
    co = np.zeros(V + 1, np.int64)
    co[1:] = np.cumsum(deg)
    assert deg[0] > 20000 and all(deg[v] == 0 for v in EMPTY)
    assert all(deg[v] == n for v, n in EXACT.items())
    assert np.any(src == dst)
    assert len(set(ri[co[0]:co[1]].tolist())) < deg[0]  # duplicates inside the hub
    g = DeviceGraph(V, int(src.size), torch.from_numpy(co).to(DEV),
                    torch.from_numpy(ri.astype(np.int32)).to(DEV),
                    torch.from_numpy(deg.astype(np.int32)).to(DEV),
                    torch.from_numpy(np.bincount(src, minlength=V).astype(np.int32)).to(DEV))
    return dict(g=g, co=torch.from_numpy(co), ri=torch.from_numpy(ri), e=int(src.size))


_cache = {}


def _case(graph, case, regime):
    """H, att and the float64 / float32 references of one case, computed once"""
    key = (case, regime)
    if key not in _cache:
        K, D, mean = CASES[case]
        F = K * D
        gen = torch.Generator().manual_seed(1000 * F + 10 * K + 2 * int(mean) + (regime == "extreme"))
        H = torch.randn(V, F, generator=gen)
        att = torch.randn(2 * F, generator=gen) * (0.3 if regime == "moderate"
                                                   else 150.0 / (1.4 * D ** 0.5))
        dl = torch.arange(V)
        ref = {}
        for dtype in (torch.float64, torch.float32):
            Hd, ad = H.to(dtype), att.to(dtype)
            Y, _, _ = ghb.heads_chain(Hd, ad, graph["co"], graph["ri"], dl, K, D, mean)
            Hh = Hd.view(V, K, D)
            S = torch.cat([torch.einsum("vkd,kd->vk", Hh, ad[:F].view(K, D)),
                           torch.einsum("vkd,kd->vk", Hh, ad[F:].view(K, D))], 1)
            ref[dtype] = dict(Y=Y.double(), S=S.double())
        if regime == "extreme":  # a plain exp of these scores overflows float32
            assert float(ref[torch.float64]["S"].abs().max()) > 100.0
        _cache[key] = dict(H=H, att=att, r64=ref[torch.float64], r32=ref[torch.float32])
    return _cache[key]


def _pitch(width, padded):
    """padded: a pitch wider than the row that keeps float4 rows aligned where they can be"""
    return width + ((4 if width % 4 == 0 else 3) if padded else 0)


def _rows(width, padded, fill):
    """(buffer, view): V + EXTRA_ROWS rows of the pitch, all `fill`; view = its [V, width]"""
    buf = torch.full((V + EXTRA_ROWS, _pitch(width, padded)), fill, device=DEV)
    return buf, buf[:V, :width]


def _in_rows(x, padded):
    _, view = _rows(x.shape[1], padded, float("nan"))
    view.copy_(x)
    return view


def _outside_intact(buf, width, lo=0, hi=V):
    """only rows [lo, hi) x [0, width) of a sentinel-filled buffer may have changed"""
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[lo:hi, :width] = False
    return bool((buf[keep] == SENT).all())


def _err(x, ref, rows=None):
    x, ref = x.double(), ref.double()
    if rows is not None:
        x, ref = x[rows], ref[rows]
    return float((x - ref).abs().max()) / float(ref.abs().max())


def _held(tag, got, r64, r32, bad, rows=None):
    ek, e32 = _err(got, r64, rows), _err(r32, r64, rows)
    bound = yardstick_bound(e32, C if rows is None else C_ROW)
    print(f"  {tag}: err(kernel) {ek:.3e} err(fp32 chain) {e32:.3e} "
          f"ratio {ek / max(e32, 2.0 ** -30):.2f} bound {bound:.3e}")
    if not ek <= bound:
        bad.append(f"{tag}: {ek:.3e} > {bound:.3e}")


def _forward(hip, graph, c, K, mean, padded, **rng):
    """(S buffer, Y buffer, Y view) of one scores + attention pass on fresh buffers"""
    F = c["H"].shape[1]
    FY = F // K if mean else F
    H = _in_rows(c["H"], padded)
    att = c["att"].to(DEV)
    Sbuf = torch.full((V + EXTRA_ROWS, 2 * K), SENT, device=DEV)
    hip.gat_scores(H, K, att, Sbuf[:V])
    Ybuf, Y = _rows(FY, padded, SENT)
    hip.gat_graph_fwd(graph["g"], H, K, Sbuf[:V], Y, mean=mean, **rng)
    torch.cuda.synchronize()
    return Sbuf, Ybuf, Y


@pytest.mark.parametrize("padded", [False, True], ids=["unpadded", "padded"])
@pytest.mark.parametrize("regime", ["moderate", "extreme"])
@pytest.mark.parametrize("case", list(CASES))
def test_matches_the_float64_chain(hip, graph, case, regime, padded):
    K, D, mean = CASES[case]
    FY = D if mean else K * D
    c = _case(graph, case, regime)
    Sbuf, Ybuf, Y = _forward(hip, graph, c, K, mean, padded)
    print(f"{case} {regime} {'padded' if padded else 'unpadded'}:")
    bad = []
    _held("S", Sbuf[:V].cpu(), c["r64"]["S"], c["r32"]["S"], bad)
    got = Y.cpu()
    assert bool(torch.isfinite(got).all())
    _held("Y", got, c["r64"]["Y"], c["r32"]["Y"], bad)
    for r in OWN_ROWS:
        _held(f"Y[{r}]", got, c["r64"]["Y"], c["r32"]["Y"], bad, rows=r)
    assert not bad, "; ".join(bad)
    assert float(c["r64"]["Y"].max()) > 0 and bool((c["r64"]["Y"] == 0).any())  # the relu cuts
    for v in EMPTY:  # an empty column is a zero row
        assert not got[v].any()
    # pitch padding and the rows past V are not written, nor anything past S
    assert _outside_intact(Ybuf, FY)
    assert bool((Sbuf[V:] == SENT).all())
    # no order left open: a second call gives the same bytes
    Sbuf2, _, Y2 = _forward(hip, graph, c, K, mean, padded)
    assert Sbuf2[:V].cpu().numpy().tobytes() == Sbuf[:V].cpu().numpy().tobytes()
    assert Y2.cpu().numpy().tobytes() == got.numpy().tobytes()


@pytest.mark.parametrize("padded", [False, True], ids=["unpadded", "padded"])
@pytest.mark.parametrize("case", list(CASES))
def test_sub_range_leaves_other_rows_alone(hip, graph, case, padded):
    K, D, mean = CASES[case]
    FY = D if mean else K * D
    c = _case(graph, case, "moderate")
    _, _, full = _forward(hip, graph, c, K, mean, padded)
    _, Ybuf, Y = _forward(hip, graph, c, K, mean, padded, v_begin=3, v_end=V - 5)
    assert _outside_intact(Ybuf, FY, 3, V - 5)
    assert torch.equal(Y[3:V - 5], full[3:V - 5])  # a row does not depend on the range
    assert not bool((Y[3:V - 5] == SENT).any())


def test_agrees_with_the_sampled_kernel_on_the_same_graph_as_a_block(hip, graph):
    """(8, 8): hip.gat_forward_heads on the whole graph as one block (u32 offsets,
    dst_local_id = arange) and the new kernel, each within its own bound of the
    same float64 rows."""
    case = "K8-D8-float4-heads-in-a-group"
    K, D, mean = CASES[case]
    for regime in ("moderate", "extreme"):
        c = _case(graph, case, regime)
        _, _, Y = _forward(hip, graph, c, K, mean, False)
        H, att = c["H"].to(DEV), c["att"].to(DEV)
        co32 = graph["co"].to(torch.int32).to(DEV)
        dl = torch.arange(V, dtype=torch.int32, device=DEV)
        m = torch.empty(graph["e"] * K, device=DEV)
        a = torch.empty(graph["e"] * K, device=DEV)
        Yb = torch.empty(V, K * D, device=DEV)
        hip.gat_forward_heads(co32, graph["g"].row_indices, dl, V, H, K, att, m, a, Yb)
        torch.cuda.synchronize()
        bad = []
        print(f"{case} {regime}:")
        _held("graph kernel", Y.cpu(), c["r64"]["Y"], c["r32"]["Y"], bad)
        _held("block kernel", Yb.cpu(), c["r64"]["Y"], c["r32"]["Y"], bad)
        assert not bad, "; ".join(bad)


def test_invalid_arguments_raise_and_write_nothing(hip, graph):
    H = torch.randn(V, 16, device=DEV)
    att = torch.randn(32, device=DEV)
    S = torch.full((V, 4), SENT, device=DEV)
    Y = torch.full((V, 16), SENT, device=DEV)
    with pytest.raises(RuntimeError, match="heads"):
        hip.gat_scores(H, 0, att, S)
    with pytest.raises(RuntimeError, match="heads"):
        hip.gat_graph_fwd(graph["g"], H, 0, S, Y)
    with pytest.raises(RuntimeError, match="D >= 1"):
        hip.gat_graph_fwd(graph["g"], H[:, :0], 2, S, Y[:, :0])
    with pytest.raises(RuntimeError, match="D >= 1"):
        hip.gat_scores(H[:, :0], 2, att, S)
    with pytest.raises(RuntimeError, match="vertex range"):
        hip.gat_graph_fwd(graph["g"], H, 2, S, Y, v_end=V + 1)
    with pytest.raises(RuntimeError, match="v_begin > v_end"):
        hip.gat_graph_fwd(graph["g"], H, 2, S, Y, v_begin=5, v_end=4)
    with pytest.raises(ValueError, match="do not divide"):
        hip.gat_graph_fwd(graph["g"], H, 3, S, Y)
    torch.cuda.synchronize()
    assert bool((S == SENT).all()) and bool((Y == SENT).all())
