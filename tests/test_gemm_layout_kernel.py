"""Every dispatch cell of the layer GEMMs over base alignment and row pitch.

tests/gemm_layouts.py holds the layout builders, the cell table (entry point,
GEMM mode, shape, one (base, pitch) per operand, the row map's offset, the
kernel the dispatcher's predicates route the cell to) and the bars.  Each cell
builds its operands as views inside sentinel-filled buffers (NaN around the
inputs, a fixed bit pattern around C), calls the entry point and asserts:

  1. accuracy against torch float64 of the same float32 values, at the bar of
     the kernel family the route ends on (gemm_layouts.f32_bar / split_bar),
     with no NaN in C although every input pad is NaN;
  2. no stray stores: C's pad columns, guard rows and the floats before its
     base still hold the sentinel, and so does every input buffer;
  3. determinism: a second call is bit-identical;
  4. bit equality within a width group: cells that differ from their sibling
     only in a load or store width (AV 4/2/1, bfull, vs, the B image fill, the
     C store, the vector/scalar sum_splits tree at one split count) run the
     same kernel over the same k order, so their results are the same bits.

The kernel-trace evidence that the cells reach the kernels the table names is
profiles/gemm_layout_routes.json.
"""
import pytest
import torch

import gemm_layouts as gl

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctxs():
    from nts.hip import HipContext
    out = {}
    for mode in (gl.F32, gl.SPLIT3, gl.SPLIT3_ALL):
        out[mode] = HipContext(0, seed=2000)
        out[mode].set_gemm_mode(mode)
    return out


_group_bits = {}   # group -> C bits of the group's first cell in table order (its sibling)
_f32_dense = {}    # (entry, shape) -> the fp32 path's result on aligned dense copies


def _dense_f32(ctxs, c, ops):
    """The NTS_GEMM_F32 context on aligned dense copies of the same values:
    the yardstick of the split bar."""
    key = (c.entry, c.shape)
    if key not in _f32_dense:
        A = ops["A"][1].contiguous()
        B = ops["B"][1].contiguous()
        X = ops["X"][1].contiguous() if c.masked else None
        rows = ops["map"][1].clone() if c.mapped else None
        C = torch.full(c.shape[:2], float("nan"), device=DEV)
        gl.call(ctxs[gl.F32], c, A, B, C, X=X, rows=rows)
        torch.cuda.synchronize()
        _f32_dense[key] = C
    return _f32_dense[key]


def _run(ctxs, c):
    """One call of the cell on freshly built operands: (ops, C view, its bits)."""
    M, N, _ = c.shape
    ops = gl.build(c, DEV)
    Cfull = ops["C"][1]
    C = Cfull[:M, :N]
    args = dict(X=ops["X"][1] if c.masked else None, rows=ops["map"][1] if c.mapped else None)
    gl.call(ctxs[c.mode], c, ops["A"][1], ops["B"][1], C if C.numel() else Cfull, **args)
    torch.cuda.synchronize()
    return ops, C, args, C.clone()


def _sibling_bits(ctxs, group):
    """The result of the group's first cell in table order, computed on demand
    (whichever cells were selected, in whatever order)."""
    if group not in _group_bits:
        _group_bits[group] = _run(ctxs, gl.groups()[group][0])[3]
    return _group_bits[group]


def _assert_untouched(ops, C):
    assert gl.untouched(ops["C"][0], C), "a store outside C's [M, N] view"
    for op in ("A", "B", "X", "map"):
        if op in ops:
            assert gl.untouched(*ops[op]), f"operand {op}'s buffer changed"


@pytest.mark.parametrize("cid", [c.id for c in gl.CELLS])
def test_gemm_layout_cell(ctxs, cid):
    c = gl.BY_ID[cid]
    M, N, K = c.shape
    ops, C, args, got = _run(ctxs, c)

    # 2. no stray stores (checked first: a stray store is the worse fault)
    _assert_untouched(ops, C)
    if M == 0 or N == 0:
        return

    # 1. accuracy
    assert not torch.isnan(got).any(), "a NaN pad reached C"
    ref, scale = gl.reference(c, ops)
    if K == 0:
        assert torch.equal(got, torch.zeros_like(got))
    elif c.epi:
        s = 1.0 / (1.0 - gl.DROP_P)
        if gl.on_split_kernel(c):  # test_split3_relu_dropout_epilogue's form
            C32 = _dense_f32(ctxs, c, ops)
            clear = ref.abs() > 1e-5 * scale
            assert torch.equal((C32 != 0) & clear, (got != 0) & clear)
            refe = torch.where(C32 != 0, torch.relu(ref) * s, torch.zeros_like(ref))
            e32, es3 = gl.split_errs(C32, got, refe, scale * s, where=clear)
            print(f"\n[{cid}] {c.route}: e32 {e32:.3e} es3 {es3:.3e}")
            gl.split_bar(e32, es3)
        else:                      # test_gemm_relu_dropout_epilogue's form
            keep = gl.keep_mask(c, DEV)
            refe = torch.where(keep & (ref > 0), ref * s, torch.zeros_like(ref))
            near0 = ref.abs() < 1e-4 * K ** 0.5
            gl.f32_bar(got[~near0], refe[~near0], K, scale=s)
    elif gl.on_split_kernel(c):
        e32, es3 = gl.split_errs(_dense_f32(ctxs, c, ops), got, ref, scale)
        print(f"\n[{cid}] {c.route}: e32 {e32:.3e} es3 {es3:.3e}")
        gl.split_bar(e32, es3)
    else:
        gl.f32_bar(got, ref, K, masked=c.masked)

    # 3. determinism
    C.fill_(float("nan"))  # (the view's elements only)
    gl.call(ctxs[c.mode], c, ops["A"][1], ops["B"][1], C, **args)
    torch.cuda.synchronize()
    assert torch.equal(C, got), "a second call differs"
    _assert_untouched(ops, C)

    # 4. bit equality across load and store widths: against the group's first cell
    if c.group:
        sib = gl.groups()[c.group][0].id
        assert torch.equal(_sibling_bits(ctxs, c.group), got), f"{cid} differs from its sibling {sib}"
