"""The gathers over an IEEE-half feature table (csrc/agghalf.hip) through the
C-ABI: nts_hip_spmm_csc_fwd_h, nts_hip_gather_rows_h, nts_hip_spmm_graph_fwd_h.

f16 storage, fp32 arithmetic: a half widens to fp32 exactly, and the sums are
the fp32 kernels' (serial in CSC edge order, (x*w)+acc from 0), so every
comparison here is on bit patterns, without a tolerance:
  (a) the fp32 sibling run on the fp32 widening of the same table, and
  (b) for the sampled aggregation, agg32 (tests/agg_blocks.py) in numpy on it.
The widening itself (numpy float16 -> float32) is checked on every finite half
in tests/test_f16_features_cpu.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import agg_blocks as ab

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 12345.0
V_LIVE = 90  # *v below the block's v_cap of 96: the rows beyond keep the sentinel
# 4100: more than 8 chunks of 64 lanes x 8 halves (4096 columns a round at most)
WIDTHS = (1, 3, 4, 7, 8, 41, 64, 100, 128, 130, 256, 602, 4100)


def _up(n, m):
    return (n + m - 1) // m * m


# id: (pitch of the half table, base offset in halves from a 16-byte boundary,
#      pitch of Y) — and the load width the table then allows
LAYOUTS = {
    "pad8": (lambda F: _up(F, 8), 0, lambda F: _up(F, 4) + 4),      # 16-byte loads
    "pad64": (lambda F: _up(F, 64), 0, lambda F: _up(F, 32) + 32),  # the 128-byte pitch
    "pitch+4": (lambda F: _up(F, 8) + 4, 0, lambda F: _up(F, 2) + 2),  # pitch % 8 != 0: 8-byte
    "base+4": (lambda F: _up(F, 8), 4, lambda F: F + 1),            # 8-byte loads
    "base+2": (lambda F: _up(F, 8), 2, lambda F: F + 1),            # 4-byte loads
    "base+1": (lambda F: _up(F, 8), 1, lambda F: F + 3),            # 2-byte loads
}


def _t(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(DEV)


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=2000)


@pytest.fixture(scope="module")
def block():
    b = ab.make_block(0)
    dev = {k: _t(b[k]) for k in ("column_offset", "row_indices", "weight", "src_map")}
    dev["v_live"] = torch.tensor([V_LIVE], dtype=torch.int32, device=DEV)
    return b, dev


_tables, _refs = {}, {}


def half_values(rows, F):
    """float16 [rows, F]: random halves of both signs; row 0 the two zeros, row 1
    subnormals, row 2 the largest finite half, each with mixed signs."""
    if (rows, F) not in _tables:
        rng = np.random.default_rng(1000 + F)
        x = rng.standard_normal((rows, F)).astype(np.float16)
        sign = (rng.integers(0, 2, (3, F)) << 15).astype(np.uint16)
        x[0] = sign[0].view(np.float16)                                      # +0 / -0
        x[1] = (rng.integers(1, 1024, F).astype(np.uint16) | sign[1]).view(np.float16)
        x[2] = (np.uint16(0x7BFF) | sign[2]).view(np.float16)                # +-65504
        assert np.isfinite(x.astype(np.float32)).all()
        _tables[(rows, F)] = x
    return _tables[(rows, F)]


def half_table(x, ld, base):
    """the values of x as a [rows, F] view of pitch ld whose first element lies
    `base` halves past a 16-byte boundary; the storage around it is NaN"""
    rows, F = x.shape
    buf = torch.full((rows * ld + 16,), float("nan"), dtype=torch.float16, device=DEV)
    assert buf.data_ptr() % 16 == 0
    t = buf.as_strided((rows, F), (ld, 1), base)
    t.copy_(torch.from_numpy(x))
    assert t.data_ptr() % 16 == (2 * base) % 16
    return t


def strided_out(rows, F, ld):
    buf = torch.full((rows, ld), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[:, :F]


def agg_ref(b, F, weighted, mapped):
    """agg32 on the widened table, once per case and shared by the layouts"""
    key = (F, weighted, mapped)
    if key not in _refs:
        wide = half_values(ab.N_TABLE, F).astype(np.float32)
        idx = b["src_map"][b["row_indices"]] if mapped else b["row_indices"]
        _refs[key] = ab.agg32(b["column_offset"], idx, b["weight"] if weighted else None, wide,
                              n=V_LIVE)
    return _refs[key]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("F", WIDTHS)
def test_csc_fwd_h_is_the_fp32_call_on_the_widened_table(hip, block, F, layout):
    b, d = block
    ld_of, base, ldy_of = LAYOUTS[layout]
    x = half_values(ab.N_TABLE, F)
    xh = half_table(x, ld_of(F), base)
    wide = xh.float().contiguous()  # the fp32 widening, dense
    assert np.array_equal(wide.cpu().numpy().view(np.uint32), x.astype(np.float32).view(np.uint32))
    for weighted in (True, False):
        for mapped in (True, False):
            w = d["weight"] if weighted else None
            m = d["src_map"] if mapped else None
            got_buf, got = strided_out(b["v"], F, ldy_of(F))
            ref_buf, ref = strided_out(b["v"], F, ldy_of(F))
            hip.spmm_csc_fwd_h(d["column_offset"], d["row_indices"], w, d["v_live"], b["v"], xh,
                               got, row_map=m)
            hip.spmm_csc_fwd(d["column_offset"], d["row_indices"], w, d["v_live"], b["v"], wide,
                             ref, row_map=m)
            torch.cuda.synchronize()
            # (a) the fp32 kernel, the rows beyond *v and Y's pitch padding included
            assert _bits_equal(got_buf, ref_buf), (F, layout, weighted, mapped)
            assert bool((got_buf[V_LIVE:] == SENTINEL).all())
            assert bool((got_buf[:, F:] == SENTINEL).all())
            # (b) the serial fp32 order in numpy
            y = got[:V_LIVE].cpu().numpy()
            assert np.array_equal(y.view(np.uint32), agg_ref(b, F, weighted, mapped).view(np.uint32))
            again_buf, again = strided_out(b["v"], F, ldy_of(F))
            hip.spmm_csc_fwd_h(d["column_offset"], d["row_indices"], w, d["v_live"], b["v"], xh,
                               again, row_map=m)
            assert _bits_equal(got_buf, again_buf)


def test_csc_fwd_h_without_a_device_row_count_writes_v_cap_rows(hip, block):
    b, d = block
    F = 41
    xh = half_table(half_values(ab.N_TABLE, F), 48, 0)
    got_buf, got = strided_out(b["v"], F, 48)
    ref_buf, ref = strided_out(b["v"], F, 48)
    hip.spmm_csc_fwd_h(d["column_offset"], d["row_indices"], d["weight"], None, b["v"], xh, got)
    hip.spmm_csc_fwd(d["column_offset"], d["row_indices"], d["weight"], None, b["v"],
                     xh.float().contiguous(), ref)
    assert _bits_equal(got_buf, ref_buf)
    empty = np.nonzero(np.diff(b["column_offset"].astype(np.int64)) == 0)[0]
    assert empty.size and bool((got[torch.from_numpy(empty).to(DEV)] == 0).all())


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("F", WIDTHS)
def test_gather_rows_h_widens_the_indexed_rows(hip, F, layout):
    ld_of, base, ldo_of = LAYOUTS[layout]
    x = half_values(ab.N_TABLE, F)
    xh = half_table(x, ld_of(F), base)
    n_cap, n = 300, 257
    index = np.random.default_rng(F).integers(0, ab.N_TABLE, n_cap).astype(np.uint32)
    n_dev = torch.tensor([n], dtype=torch.int32, device=DEV)
    out_buf, out = strided_out(n_cap, F, ldo_of(F))
    hip.gather_rows_h(xh, _t(index), n_dev, n_cap, out)
    want = np.full((n_cap, ldo_of(F)), SENTINEL, np.float32)
    want[:n, :F] = x.astype(np.float32)[index[:n]]
    assert np.array_equal(out_buf.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------
# the full-neighbour pass
# ---------------------------------------------------------------------------
HUB = 2048  # kHubEdges (csrc/graph_hubs.hpp): longer columns are split by column slice
V_G = 2000
COLUMNS = {0: 0, 10: 1, 11: 1, 20: HUB - 1, 21: HUB, 22: HUB + 1, 23: HUB + 2, 30: 7 * HUB + 5,
           1999: 0}


@pytest.fixture(scope="module")
def graph(hip):
    from nts.hip import DeviceGraph
    rng = np.random.default_rng(5)
    deg = rng.integers(0, 13, V_G)
    for c, n in COLUMNS.items():
        deg[c] = n
    dst = np.repeat(np.arange(V_G), deg).astype(np.uint32)
    src = rng.integers(0, V_G, dst.size).astype(np.uint32)
    perm = rng.permutation(dst.size)
    s_t, d_t = _t(src[perm]), _t(dst[perm])
    col, rows = hip.build_csc(s_t, d_t, V_G)
    out_d, in_d = hip.degrees(s_t, d_t, V_G)
    got = np.diff(col.cpu().numpy())
    assert np.array_equal(got, deg) and (got == 0).sum() > 2
    return DeviceGraph(V_G, int(dst.size), col, rows, in_d, out_d)


@pytest.mark.parametrize("F", [8, 41, 128])
def test_graph_fwd_h_is_the_fp32_call_on_the_widened_table(hip, graph, F):
    from nts import _abi
    xh = half_table(half_values(V_G, F), _up(F, 8), 0)
    wide = xh.float().contiguous()
    for wt in (_abi.NTS_WEIGHT_SUM, _abi.NTS_WEIGHT_MEAN, _abi.NTS_WEIGHT_NONE):
        for relu in (False, True):
            for lo, hi in ((0, V_G), (15, 1500)):
                got_buf, got = strided_out(V_G, F, _up(F, 4) + 4)
                ref_buf, ref = strided_out(V_G, F, _up(F, 4) + 4)
                hip.spmm_graph_fwd_h(graph, xh, got, wt, relu=relu, v_begin=lo, v_end=hi)
                hip.spmm_graph_fwd(graph, wide, ref, wt, relu=relu, v_begin=lo, v_end=hi)
                assert _bits_equal(got_buf, ref_buf), (F, wt, relu, lo, hi)
                assert bool((got_buf[:lo] == SENTINEL).all()) and bool((got_buf[hi:] == SENTINEL).all())
                assert bool((got_buf[:, F:] == SENTINEL).all())
                assert bool(torch.isfinite(got[lo:hi]).all())
                if lo == 0:  # empty columns: zero rows
                    assert bool((got[0] == 0).all()) and bool((got[V_G - 1] == 0).all())
                if relu:
                    assert bool((got[lo:hi] >= 0).all())


def test_graph_fwd_h_on_an_unaligned_table(hip, graph):
    """2-byte aligned rows (base one half past a 16-byte boundary) over the hub switch"""
    from nts import _abi
    F = 41
    xh = half_table(half_values(V_G, F), 43, 1)
    got_buf, got = strided_out(V_G, F, F)
    ref_buf, ref = strided_out(V_G, F, F)
    hip.spmm_graph_fwd_h(graph, xh, got, _abi.NTS_WEIGHT_MEAN)
    hip.spmm_graph_fwd(graph, xh.float().contiguous(), ref, _abi.NTS_WEIGHT_MEAN)
    assert _bits_equal(got_buf, ref_buf)


# ---------------------------------------------------------------------------
# invalid arguments: NTS_ERR_INVALID, a message, nothing written
# ---------------------------------------------------------------------------
NTS_ERR_INVALID = 1


def _refused(lib, rc, *outs):
    assert rc == NTS_ERR_INVALID
    assert lib.nts_hip_last_error().decode()
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == SENTINEL).all())


def test_invalid_arguments_are_refused_before_any_write(hip, block, graph):
    from nts import _abi
    from nts._abi import ptr
    b, d = block
    lib, h = hip.lib, hip.h
    F, ld = 16, 16
    xh = half_table(half_values(ab.N_TABLE, F), ld, 0)
    y = torch.full((V_G, F), SENTINEL, dtype=torch.float32, device=DEV)
    co, ri, w, v = (ptr(d["column_offset"]), ptr(d["row_indices"]), ptr(d["weight"]),
                    ptr(d["v_live"]))
    idx = _t(np.arange(8, dtype=np.uint32))

    def csc(x=ptr(xh), ldx=ld, feat=F, ldy=F):
        return lib.nts_hip_spmm_csc_fwd_h(h, co, ri, w, v, b["v"], x, ldx, None, feat, ptr(y), ldy)

    def rows(x=ptr(xh), ldx=ld, feat=F, ldo=F):
        return lib.nts_hip_gather_rows_h(h, x, ldx, ptr(idx), None, 8, feat, ptr(y), ldo)

    g = graph.as_struct()
    xg = half_table(half_values(V_G, F), ld, 0)

    def full(x=ptr(xg), ldx=ld, feat=F, lo=0, hi=V_G, wt=_abi.NTS_WEIGHT_SUM):
        return lib.nts_hip_spmm_graph_fwd_h(h, C.byref(g), lo, hi, wt, 0, x, ldx, feat, ptr(y), F)

    for call in (csc, rows, full):
        _refused(lib, call(x=None), y)        # a NULL table
        _refused(lib, call(feat=0), y)        # feature_size == 0
        _refused(lib, call(ldx=F - 1), y)     # pitch below feature_size
        _refused(lib, call(x=ptr(xh) + 1), y)  # an odd table address
    _refused(lib, full(hi=V_G + 1), y)        # a range outside the graph
    _refused(lib, full(lo=5, hi=4), y)
    _refused(lib, full(wt=_abi.NTS_WEIGHT_MEAN_SAMPLED), y)
    _refused(lib, full(wt=_abi.NTS_WEIGHT_SUM | 0x10), y)  # the UP_DEGREE bit
    assert csc() == _abi.NTS_OK and rows() == _abi.NTS_OK and full() == _abi.NTS_OK
