"""tests/gemm_layouts.py on the CPU: the layout builders, the reference and the
bars' sensitivity, and the cell table against the restated dispatch predicates
(no GPU: nothing here launches a kernel)."""
import pytest
import torch

import gemm_layouts as gl


@pytest.mark.parametrize("rows,cols,base,pitch", [(5, 7, 0, 7), (5, 7, 1, 8), (3, 128, 2, 130),
                                                  (4, 40, 3, 41), (1, 1, 1, 1), (0, 7, 1, 9)])
@pytest.mark.parametrize("fill", ["in", "out"])
def test_view_layout_and_guards(rows, cols, base, pitch, fill):
    flat, v = gl.view(rows, cols, base, pitch, "cpu", fill)
    lead = v.storage_offset()
    assert (flat.data_ptr() + 4 * lead) % 16 == (4 * base) % 16
    assert v.shape == (rows, cols) and v.stride() == (pitch, 1)
    assert lead >= pitch and flat.numel() - (lead + rows * pitch) >= pitch  # a guard row each side
    bits = flat.view(torch.int32)
    assert bool((bits == (gl.NAN_BITS if fill == "in" else gl.OUT_BITS)).all())
    if fill == "in":
        assert bool(torch.isnan(flat).all())
    else:
        assert not bool(torch.isnan(flat).any())
    assert gl.untouched(flat, v)
    v.fill_(1.0)
    assert gl.untouched(flat, v)  # the view's own elements may change


def test_untouched_sees_one_changed_float():
    for fill in ("in", "out"):
        for where in ("pad", "before_base", "guard_row", "after"):
            flat, v = gl.view(5, 7, 1, 9, "cpu", fill)
            lead = v.storage_offset()
            at = {"pad": lead + 7, "before_base": lead - 1, "guard_row": lead - 9,
                  "after": lead + 5 * 9 + 3}[where]
            flat[at] = 0.5
            assert not gl.untouched(flat, v), (fill, where)
    # the same value, another bit pattern (-0.0 against 0.0 would compare equal as floats)
    flat, v = gl.view(2, 3, 0, 4, "cpu", "in")
    flat.view(torch.int32)[v.storage_offset() + 3] = gl.NAN_BITS + 1  # another NaN
    assert not gl.untouched(flat, v)


def test_rowmap_offset_and_guards():
    ids = torch.arange(10, dtype=torch.int32) * 3
    for off in (0, 1):
        flat, v = gl.rowmap(ids, off, "cpu")
        assert v.data_ptr() % 16 == 4 * off and torch.equal(v, ids)
        assert v.storage_offset() >= 8 and flat.numel() - v.storage_offset() - 10 >= 8
        assert gl.untouched(flat, v)
        flat[v.storage_offset() - 1] = 5
        assert not gl.untouched(flat, v)


def test_cells_build_with_their_stated_layout():
    for c in gl.CELLS:
        if max(c.shape) > 5000:
            continue
        ops = gl.build(c, "cpu")
        for op in "ABCX":
            if op in ops:
                base, pitch = c.layout(op)
                flat, v = ops[op]
                assert (flat.data_ptr() + 4 * v.storage_offset()) % 16 == (4 * base) % 16, (c.id, op)
                assert v.stride(0) == pitch, (c.id, op)
        if c.mapped:
            assert ops["map"][1].data_ptr() % 16 == 4 * c.mo
            assert int(ops["map"][1].max()) < ops["A"][1].shape[0]


def _cpu_case(cid):
    c = gl.BY_ID[cid]
    ops = gl.build(c, "cpu")
    A, B = gl.effective(c, ops)
    A = A.t() if c.trans else A
    ref, scale = gl.reference(c, ops)
    return c, A.contiguous(), B.contiguous(), ref, scale


@pytest.mark.parametrize("cid", ["kg.nn.av1.bfull0", "kg.tn.split.av1", "kg.bmask.x.base", "g3tn.map",
                                 "g3tn.x.pitch", "tb.r1.split.gather"])
def test_bars_accept_fp32_matmul_and_reject_faults(cid):
    c, A, B, ref, scale = _cpu_case(cid)
    K = c.shape[2]
    good = A @ B  # float32
    gl.f32_bar(good, ref, K, masked=c.masked)
    e32, es3 = gl.split_errs(good, good, ref, scale)
    gl.split_bar(e32, es3)
    # one element off by 1e-3 of its scale
    i, j = good.shape[0] // 2, good.shape[1] // 3
    bad = good.clone()
    bad[i, j] += 1e-3 * float(scale[i, j])
    with pytest.raises(AssertionError):
        gl.f32_bar(bad, ref, K, masked=c.masked)
    with pytest.raises(AssertionError):
        gl.split_bar(*gl.split_errs(good, bad, ref, scale))
    # the last k term dropped
    short = A[:, :-1] @ B[:-1]
    with pytest.raises(AssertionError):
        gl.f32_bar(short, ref, K, masked=c.masked)
    with pytest.raises(AssertionError):
        gl.split_bar(*gl.split_errs(good, short, ref, scale))


def test_epilogue_reference_is_the_documented_philox_mask():
    c = gl.BY_ID["kg.epi.av1.bfull0"]
    keep = gl.keep_mask(c, "cpu")
    assert keep.shape == c.shape[:2] and abs(keep.double().mean().item() - (1 - gl.DROP_P)) < 0.03


def test_table_routes_are_what_the_predicates_say():
    assert len({c.id for c in gl.CELLS}) == len(gl.CELLS)
    for c in gl.CELLS:
        assert c.entry in gl.ENTRY_POINTS and c.mode in (gl.F32, gl.SPLIT3, gl.SPLIT3_ALL)
        assert gl.expected_route(c) == c.route, c.id
        assert c.by
        for op in "ABCX":  # the entry points' own argument checks: ld >= columns
            assert c.layout(op)[1] >= c.cols(op)


def test_every_listed_instance_is_some_cells_route():
    routes = " ".join(c.route for c in gl.CELLS)
    for k in gl.REQUIRED:
        assert k in routes, k
    for k in gl.UNREACHABLE:  # no cell claims an instance the C ABI cannot reach
        assert k not in routes, k
    # every route's kernels translate to a trace name
    for c in gl.CELLS:
        assert all(n.startswith("k_") for n in gl.trace_names(c.route)), c.id
    assert gl.trace_names("k_gemm<TN,AV2,bfull0,EPI0,BMASK1>+k_sum_splits_tree<V1,T64>") == [
        "k_gemm<true, 2, false, false, true>", "k_sum_splits_tree<1, 64>"]


def test_groups_and_sizes():
    for g, cells in gl.groups().items():
        assert len(cells) >= 2, g
        # one kernel family, one entry point, one shape, one split count per group
        assert len({(c.entry, c.shape, c.mode != gl.F32) for c in cells}) == 1, g
        assert len({c.route.split("<")[0] for c in cells}) == 1, g
        assert len({c.route.count("+") for c in cells}) == 1, g
    for c in gl.CELLS:
        assert max(c.shape[0], c.shape[2] if c.trans else 0) <= 40000, c.id


def test_pair_table_gemms_refuse_misaligned_operands_without_a_gpu():
    """The f16 pair-table GEMMs (csrc/gemmh2.hip) take no layout matrix: they
    refuse an operand off 16 bytes or a pitch off 4 floats with
    NTS_ERR_INVALID before anything is launched."""
    import ctypes
    from nts import _abi
    lib = _abi.lib()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a += (-a) % 16          # 16-byte aligned
    off = a + 4             # 4 bytes past it

    def invalid(rc, what):
        assert rc == 1  # NTS_ERR_INVALID
        assert b"invalid argument" in lib.nts_hip_last_error()
        assert what in lib.nts_hip_last_error(), lib.nts_hip_last_error()

    def nn(P=a, ldp=32, W=a, ldw=16):  # (ctx, epi, M, N, Kp, P, ldp, rs, rows, W, ldw, K, C, ldc, p, seed, offset)
        return lib.nts_hip_gemm_h2_gather(a, 0, 4, 16, 32, P, ldp, a, None, W, ldw, 32, a, 16, 0.0, 0, 0)

    invalid(nn(P=off), b"pair table layout")
    invalid(nn(ldp=34), b"pair table layout")
    invalid(nn(W=off), b"float4-aligned")
    invalid(nn(ldw=18), b"float4-aligned")

    def tn(B=a, ldb=16, X=None, ldx=16, rows=None):  # (ctx, M, N, K, P, ldp, rs, rows, B, ldb, X, ldx, bscale, C, ldc)
        return lib.nts_hip_gemm_h2_tn_gather(a, 4, 16, 8, a, 4, a, rows, B, ldb, X, ldx, 1.0, a, 16)

    invalid(tn(B=off), b"B layout")
    invalid(tn(ldb=18), b"B layout")
    invalid(tn(X=off), b"X layout")
    invalid(tn(X=a, ldx=18), b"X layout")
    invalid(tn(rows=off), b"a_rows must be 16-byte aligned")

    def nnd(A=a, lda=32, W=a, ldw=128):  # (ctx, epi, M, N, K, A, lda, W, ldw, C, ldc, p, seed, offset, Q, ldq, rs)
        return lib.nts_hip_gemm_h2d_act(a, 0, 4, 128, 32, A, lda, W, ldw, a, 128, 0.0, 0, 0, None, 0, None)

    invalid(nnd(A=off), b"A rows must be 16-byte aligned")
    invalid(nnd(lda=34), b"A rows must be 16-byte aligned")
    invalid(nnd(W=off), b"ld")
    invalid(nnd(ldw=130), b"ld")
