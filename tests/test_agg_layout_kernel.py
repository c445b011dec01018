"""The sum-aggregation family (csrc/aggregate.hip) through the C-ABI, on every
(vector width, lane-group shape, last_valid, row length, layout) cell.

Block.  tests/agg_blocks.py: 96 destinations, 320 sources, column degrees and
CSR row lengths below, at and above the gather's unroll U and the long-row
threshold 4 U for U in {4, 5, 8}, empty rows, one row of 200, a block whose
four 64-lane groups all hold a long row; weights of both signs, and NULL.

Widths and layouts.  agg_blocks.WIDTHS x agg_blocks.LAYOUTS; the cell each pair
reaches is derived from agg_shape.hpp's rules (agg_blocks.cell) and printed once
(test_cell_table).  Every input is a view into a NaN-filled allocation with one
leading and two trailing rows more; every output a view into a sentinel-filled
one, which must keep the sentinel, bit for bit, in its pitch padding, its extra
rows and its rows past the live size.  A padded pitch covers the rounded-up
row, so the pad path's read of padding stays inside the allocation.

Asserted per entry point, width and layout:
* |got - float64 reference| <= 2 (n + k) 2^-24 sum|w x| per element (n the
  row's edges; k below), scaled by the mode's scale;
* bit-equal to the fp32 serial edge order for every CSC column and every CSR
  row of at most kLongRow(U) edges (>= 16, what the suite promises), and to
  the documented in-order pieces for the longer CSR rows;
* no NaN in a live output (a NaN is a read of padding); sentinels intact;
* layout independence: bit-equal to the dense layout's output for every CSC
  mode, gather_rows and act_backward, and for the CSR modes (csr_bwd, masked,
  postmask, root, bits, colmax) on the rows that are short in both cells; a
  row that is long in either is summed in GPB = 256 / LPD pieces, which the
  vector width changes, and is held by the bound and the piece reference only.
  The atomic scatter has no order at all: the bound only.

k (roundings beyond the n products and adds): plain, row map, cached, colmax,
atomic, root forward 0; fused activation 1 (the dropout scale); masked 1 (the
scale on every term); post-mask and its bits form 1; root backward 1 (the self
row's add), 2 with x_act (and the scale).

Thinning.  The NULL weight array is run on the dense and pad32 layouts only:
the weight pointer enters no launch decision (row_vec, pick_shape and gather_u
do not see it), it only replaces a per-edge load.  Of the 6,816 combinations
of entry point, width, layout and weights / NULL, 4,272 run and 2,544 (NULL
weights on the seven other layouts) are left out; no cell is lost.  The
live-size variants (size from the device below the capacity, 0, and a NULL
size pointer) do not enter the launch cell either and run on two widths.
"""
import functools

import numpy as np
import pytest
import torch

import agg_blocks as ab
from test_hip_kernels import _dropout_keep, _pack_act_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -12345.5
SENT_BITS = int(np.float32(SENT).view(np.int32))
SEED, OFFSET = 0x0123_4567_89AB, 9
MASK_SCALE = np.float32(1.0 / 0.7)
EXTRA = 3  # capacity rows past the live size


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=2000)


def _t(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(DEV)


@functools.lru_cache(maxsize=None)
def _block():
    B = ab.make_block()
    dev = {k: _t(v) for k, v in B.items() if isinstance(v, np.ndarray)}
    return B, dev


@functools.lru_cache(maxsize=4)
def _data(F):
    """T [table, F]; X = T[src_map] [s, F]; Gcat [v, 2F], G its left half;
    XaV [v, F], XaS [s, F]: activations (half of them zero)"""
    B, _ = _block()
    rng = np.random.default_rng(1000 + F)
    T = rng.standard_normal((ab.N_TABLE, F)).astype(np.float32)
    Gcat = rng.standard_normal((B["v"], 2 * F)).astype(np.float32)
    XaV = np.maximum(rng.standard_normal((B["v"], F)), 0).astype(np.float32)
    XaS = np.maximum(rng.standard_normal((B["s"], F)), 0).astype(np.float32)
    return dict(T=T, X=np.ascontiguousarray(T[B["src_map"]]), Gcat=Gcat,
                G=np.ascontiguousarray(Gcat[:, :F]), XaV=XaV, XaS=XaS)


# ---- buffers -----------------------------------------------------------------------
def _alloc(rows, width, lay, fill):
    """(flat, view [rows, width]): one leading and two trailing rows of
    `pitch` floats more, `off` floats into a fresh allocation filled with `fill`"""
    rule, off = lay
    p = ab.pitch(rule, width)
    flat = torch.full(((rows + 3) * p + 4,), fill, device=DEV)
    return flat, flat[off + p:off + p + rows * p].view(rows, p)[:, :width]


def _in(x, lay):
    _, v = _alloc(x.shape[0], x.shape[1], lay, float("nan"))
    v.copy_(torch.from_numpy(x))
    return v


def _intact(flat, view, live):
    """the allocation holds the sentinel everywhere but in the view's first `live` rows"""
    bits = flat.view(torch.int32).cpu().numpy().copy()
    if live:
        o = view.storage_offset() - flat.storage_offset()
        idx = (o + np.arange(live)[:, None] * view.stride(0) + np.arange(view.shape[1])[None, :])
        bits[idx.reshape(-1)] = SENT_BITS
    return bool((bits == SENT_BITS).all())


# ---- references (shared between entry points, widths' layouts and tests) -----------------
def _wts(B, csr, wnull):
    return None if wnull else B["weight_backward" if csr else "weight"]


@functools.lru_cache(maxsize=64)
def _csc64(F, wnull, n):
    B, _ = _block()
    return ab.agg64(B["column_offset"], B["row_indices"], _wts(B, False, wnull), _data(F)["X"], n)


@functools.lru_cache(maxsize=64)
def _csc32(F, wnull, n):
    B, _ = _block()
    return ab.agg32(B["column_offset"], B["row_indices"], _wts(B, False, wnull), _data(F)["X"], n)


def _csr_in(F, masked):
    D = _data(F)
    if not masked:
        return D["G"]
    return np.where(D["XaV"] > 0, D["G"] * MASK_SCALE, np.float32(0)).astype(np.float32)


@functools.lru_cache(maxsize=64)
def _csr64(F, wnull, n, masked):
    B, _ = _block()
    return ab.agg64(B["row_offset"], B["column_indices"], _wts(B, True, wnull), _csr_in(F, masked), n)


@functools.lru_cache(maxsize=64)
def _csr32(F, wnull, n, masked, long_row, gpb):
    B, _ = _block()
    return ab.agg32_pieces(B["row_offset"], B["column_indices"], _wts(B, True, wnull),
                           _csr_in(F, masked), long_row, gpb, n)


def _reference(entry, F, wnull, n, c):
    """(ref64 [n, W], bound [n, W], ref32 [n, W] or None) of an entry point on the
    first n rows; c: its launch cell (the long-row rule of the CSR modes)"""
    B, _ = _block()
    D = _data(F)
    if entry in ab.CSC_ENTRIES:
        (S, A), E = _csc64(F, wnull, n), _csc32(F, wnull, n)
        ne = np.diff(B["column_offset"].astype(np.int64))[:n]
        if entry.startswith("fwd_act"):
            p = 0.0 if entry == "fwd_act_p0" else 0.5
            keep = _dropout_keep(n, F, p, SEED, OFFSET) if n else np.zeros((0, F), bool)
            sc = np.float32(1.0 / (1.0 - p))
            r64 = np.where(keep & (S > 0), S * float(sc), 0.0)
            r32 = np.where(keep & (E > 0), E * sc, np.float32(0)).astype(np.float32)
            return r64, ab.err_bound(A, ne, 1) * float(sc), r32
        if entry.startswith("fwd_root"):
            me = D["X"][B["dst_local_id"][:n].astype(np.int64)]
            return (np.concatenate([S, me.astype(np.float64)], 1),
                    np.concatenate([ab.err_bound(A, ne, 0), np.zeros_like(A)], 1),
                    np.concatenate([E, me], 1))
        return S, ab.err_bound(A, ne, 0), E
    if entry in ab.CSR_ENTRIES:
        masked = entry == "csr_bwd_masked"
        (S, A) = _csr64(F, wnull, n, masked)
        E = _csr32(F, wnull, n, masked, c["long_row"], c["gpb"])
        ne = np.diff(B["row_offset"].astype(np.int64))[:n]
        k, sc = (1, 1.0) if masked else (0, 1.0)
        if entry.startswith("csr_bwd_root"):
            sd = B["src_dst"][:n]
            has = sd != ab.NOT_CACHED
            me = np.zeros((n, F), np.float32)
            me[has] = D["Gcat"][sd[has].astype(np.int64), F:]
            S, A, E, k = S + me, A + np.abs(me.astype(np.float64)), E + me, 1
        if entry in ("csr_bwd_postmask", "csr_bwd_postmask_bits", "csr_bwd_root_act"):
            gate = D["XaS"][:n] > 0
            S = np.where(gate, S * float(MASK_SCALE), 0.0)
            E = np.where(gate, E * MASK_SCALE, np.float32(0)).astype(np.float32)
            k, sc = k + 1, float(MASK_SCALE)
        return S, ab.err_bound(A, ne, k) * sc, E
    if entry == "bwd_atomic":  # n live COLUMNS scattered into all s rows
        w = ab._w(_wts(B, False, wnull), B["e"]).astype(np.float64)
        ne_live = int(B["column_offset"][n])
        d_of_e = np.repeat(np.arange(B["v"]), np.diff(B["column_offset"].astype(np.int64)))[:ne_live]
        t = w[:ne_live, None] * D["G"][d_of_e].astype(np.float64)
        S, A = np.zeros((B["s"], F)), np.zeros((B["s"], F))
        ri = B["row_indices"][:ne_live].astype(np.int64)
        np.add.at(S, ri, t)
        np.add.at(A, ri, np.abs(t))
        return S, ab.err_bound(A, np.bincount(ri, minlength=B["s"]), 0), None
    if entry == "gather_rows":
        return D["X"][:n].astype(np.float64), np.zeros((n, F)), D["X"][:n]
    assert entry == "act_backward"
    r32 = np.where(D["XaV"][:n] > 0, D["G"][:n] * MASK_SCALE, np.float32(0)).astype(np.float32)
    return r32.astype(np.float64), np.zeros((n, F)), r32


# ---- one call -----------------------------------------------------------------------
class Refused(Exception):
    pass


def _run(hip, entry, F, layout, wnull=False, live="dev"):
    """Run one entry point; returns dict(got [n, W] numpy, n, intact, extra...).
    live: "dev" (size on the device, capacity EXTRA rows more), "null" (NULL
    size pointer where the entry point takes one), "zero", "part" (about 2/3)."""
    B, d = _block()
    D = _data(F)
    lin, lout, lmask = ab.LAYOUTS[layout]
    csr = entry in ab.CSR_ENTRIES
    rows = B["v"] if entry in ab.CSC_ENTRIES + ("bwd_atomic", "act_backward") else B["s"]
    n = {"dev": rows, "null": rows, "zero": 0, "part": rows * 2 // 3}[live]
    cap = rows if live == "null" else rows + EXTRA
    needs_size = entry.startswith("fwd_root") or entry.startswith("csr_bwd_root")
    ndev = None if live == "null" and not needs_size else torch.tensor([n], dtype=torch.int32,
                                                                       device=DEV)
    off, idx = (d["row_offset"], d["column_indices"]) if csr else (d["column_offset"], d["row_indices"])
    w = None if wnull else d["weight_backward" if csr else "weight"]
    W = 2 * F if entry in ab._OUT_2F else F
    out_rows = B["s"] if entry == "bwd_atomic" else rows if entry == "act_backward" else cap
    flat, y = _alloc(out_rows, W, lout, SENT)
    res = dict(n=n)
    side = []  # (flat, view, live rows) of further sentinel buffers
    try:
        if entry == "fwd":
            hip.spmm_csc_fwd(off, idx, w, ndev, cap, _in(D["X"], lin), y)
        elif entry == "fwd_map":
            hip.spmm_csc_fwd(off, idx, w, ndev, cap, _in(D["T"], lin), y, row_map=d["src_map"])
        elif entry in ("fwd_act_p0", "fwd_act_p5"):
            hip.spmm_csc_fwd_act(off, idx, w, ndev, cap, _in(D["X"], lin), y,
                                 p=0.0 if entry == "fwd_act_p0" else 0.5, seed=SEED, offset=OFFSET)
        elif entry == "fwd_act_bits":
            words = max(hip.act_bits_words(F), 4)
            bits = torch.full((cap + 1, words), SENT_BITS, dtype=torch.int32, device=DEV)
            side.append((bits.view(-1), bits, n))
            hip.spmm_csc_fwd_act_bits(off, idx, w, ndev, cap, _in(D["X"], lin), y, bits, p=0.5,
                                      seed=SEED, offset=OFFSET)
            res["bits"] = bits
        elif entry == "fwd_root":
            hip.spmm_csc_fwd_root(off, idx, w, ndev, cap, _in(D["X"], lin), d["dst_local_id"], y)
        elif entry == "fwd_root_map":
            me = _t(B["src_map"][B["dst_local_id"].astype(np.int64)])
            hip.spmm_csc_fwd_root(off, idx, w, ndev, cap, _in(D["T"], lin), me, y,
                                  row_map=d["src_map"])
        elif entry == "fwd_cached":
            res["host"] = _cached(hip, B, d, D, F, lin, w, ndev, cap, y)
        elif entry == "csr_bwd":
            hip.spmm_csr_bwd(off, idx, w, ndev, cap, _in(D["G"], lin), y)
        elif entry == "csr_bwd_masked":
            hip.spmm_csr_bwd_masked(off, idx, w, ndev, cap, _in(D["G"], lin), _in(D["XaV"], lmask),
                                    y, scale=float(MASK_SCALE))
        elif entry == "csr_bwd_postmask":
            hip.spmm_csr_bwd_postmask(off, idx, w, ndev, cap, _in(D["G"], lin),
                                      _in(D["XaS"], lmask), y, scale=float(MASK_SCALE))
        elif entry == "csr_bwd_postmask_bits":
            words = max(hip.act_bits_words(F), 4)
            packed = np.zeros((cap, words), np.uint32)
            if hip.act_bits_words(F):
                packed[:rows] = _pack_act_bits(D["XaS"], words)
            hip.spmm_csr_bwd_postmask_bits(off, idx, w, ndev, cap, _in(D["G"], lin), _t(packed), y,
                                           scale=float(MASK_SCALE))
        elif entry in ("csr_bwd_root", "csr_bwd_root_act"):
            xa = _in(D["XaS"], lmask) if entry == "csr_bwd_root_act" else None
            hip.spmm_csr_bwd_root(off, idx, w, ndev, cap, _in(D["Gcat"], lin), d["src_dst"], y,
                                  x_act=xa, scale=float(MASK_SCALE))
        elif entry == "csr_bwd_colmax":
            R = max(hip.colmax_rows_per_part(F), 1)
            nparts = (cap + R - 1) // R
            parts = torch.full((nparts + 1, F), SENT_BITS, dtype=torch.int32, device=DEV)
            side.append((parts.view(-1), parts, nparts))
            rs = np.exp2(np.random.default_rng(F).integers(-20, 20, ab.N_TABLE)).astype(np.float32)
            hip.spmm_csr_bwd_colmax(off, idx, w, ndev, cap, _in(D["G"], lin), y, parts, rs=_t(rs),
                                    rows=d["src_map"])
            res.update(parts=parts, nparts=nparts, R=R, rs=rs[B["src_map"].astype(np.int64)])
        elif entry == "bwd_atomic":
            y.zero_()  # the caller zeroes g_in; all s rows are live
            hip.spmm_csc_bwd_atomic(off, idx, w, ndev, cap, _in(D["G"], lin), y)
        elif entry == "gather_rows":
            hip.gather_rows(_in(D["T"], lin), d["src_map"], ndev, cap, y)
        elif entry == "act_backward":
            hip.act_backward(_in(D["G"], lin), _in(D["XaV"], lmask), y, scale=float(MASK_SCALE))
        else:
            raise KeyError(entry)
    except RuntimeError as ex:
        torch.cuda.synchronize()
        assert _intact(flat, y, 0), f"{entry} F={F} {layout}: refused, but wrote its output"
        for f2, v2, _ in side:
            assert _intact(f2, v2, 0), f"{entry} F={F} {layout}: refused, but wrote a side buffer"
        raise Refused(str(ex)) from None
    torch.cuda.synchronize()
    nlive = B["s"] if entry == "bwd_atomic" else n
    res["n"] = nlive
    res["got"] = y[:nlive].cpu().numpy()
    res["intact"] = _intact(flat, y, nlive) and all(_intact(f2, v2, l2) for f2, v2, l2 in side)
    if "host" in res:
        res.pop("host").close()
    return res


def _cached(hip, B, d, D, F, lin, w, ndev, cap, y):
    """the two-tier table: every other table row in an HBM cache laid out as the
    input, the rest in the host table (same pitch rule)"""
    from nts.hip import HostTable
    ld = ab.pitch(lin[0], F)
    host = HostTable(ab.N_TABLE, F, ld)
    host.tensor.as_strided((ab.N_TABLE, ld), (ld, 1)).fill_(float("nan"))
    cmap = np.full(ab.N_TABLE, ab.NOT_CACHED, np.uint32)
    hot = np.arange(0, ab.N_TABLE, 2)
    cmap[hot] = np.arange(hot.size)
    T = D["T"].copy()
    host.tensor.copy_(torch.from_numpy(np.where((cmap == ab.NOT_CACHED)[:, None], T, np.nan)))
    hip.spmm_csc_fwd_cached(d["column_offset"], d["row_indices"], w, ndev, cap, _in(T[hot], lin),
                            _t(cmap), host, d["src_map"], y)
    return host


# ---- checks -------------------------------------------------------------------------
def _check(entry, F, layout, wnull, res, c):
    tag = f"{entry} F={F} {layout} wnull={wnull} cell={c}"
    n, got = res["n"], res["got"]
    assert res["intact"], f"{tag}: sentinel overwritten"
    assert not np.isnan(got).any(), f"{tag}: NaN in a live output (a read of padding)"
    live_in = n if entry != "bwd_atomic" else res["n_in"]
    r64, bound, r32 = _reference(entry, F, wnull, live_in, c)
    err = np.abs(got.astype(np.float64) - r64)
    bad = err > bound
    assert not bad.any(), (f"{tag}: {int(bad.sum())} elements past the bound, worst "
                           f"{err[bad].max():.3e} vs {bound[bad][err[bad].argmax()]:.3e} at row "
                           f"{np.argwhere(bad)[0]}")
    if r32 is not None:
        ne = np.equal(got, r32).all(1)
        assert ne.all(), f"{tag}: rows {np.flatnonzero(~ne)[:8]} differ from the fp32 edge order"


def _colmax_check(F, layout, res):
    B, _ = _block()
    n, R, nparts = res["n"], res["R"], res["nparts"]
    pad = np.zeros((nparts * R, F), np.float32)
    pad[:n] = np.abs(res["got"] * res["rs"][:n, None])
    want = pad.reshape(nparts, R, F).max(1)
    got = res["parts"][:nparts].cpu().numpy().view(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"colmax F={F} {layout}: parts"


def _bits_check(hip, F, layout, res):
    words = hip.act_bits_words(F)
    got = res["bits"][:res["n"]].cpu().numpy().view(np.uint32)
    assert np.array_equal(got, _pack_act_bits(res["got"], words)), f"act bits F={F} {layout}"


def test_cell_table():
    """the cells this file runs (printed once; -s shows it)"""
    print("\n" + ab.format_cell_table())


@pytest.mark.parametrize("entry", ab.ENTRIES)
@pytest.mark.parametrize("F", ab.WIDTHS)
def test_layouts(hip, entry, F):
    B, _ = _block()
    ran = {}
    for layout in ab.layouts_of(entry):
        c = ab.entry_cell(entry, F, layout)
        for wnull in (False, True) if layout in ("dense", "pad32") else (False,):
            try:
                res = _run(hip, entry, F, layout, wnull)
            except Refused as ex:
                assert c is None, f"{entry} F={F} {layout}: refused a layout it documents: {ex}"
                if entry == "csr_bwd_colmax":
                    assert "column maxima" in str(ex), str(ex)
                elif ab.act_bits_words(F):
                    assert "mask bits" in str(ex), str(ex)
                continue
            assert c is not None, f"{entry} F={F} {layout}: ran a layout it documents as refused"
            res["n_in"] = B["v"]
            _check(entry, F, layout, wnull, res, c)
            if entry == "csr_bwd_colmax":
                _colmax_check(F, layout, res)
            if entry == "fwd_act_bits":
                _bits_check(hip, F, layout, res)
            if not wnull:
                ran[layout] = (res["got"], c)
    if not ran:  # a width the entry point refuses on every layout
        assert entry in ("fwd_act_bits", "csr_bwd_postmask_bits", "csr_bwd_colmax")
        return
    # layout independence (the column maxima refuse the dense layout where F % 4:
    # the first layout that ran stands in)
    base, cb = ran.get("dense", next(iter(ran.values())))
    ln = np.diff(B["row_offset"].astype(np.int64))
    for layout, (got, c) in ran.items():
        if entry == "bwd_atomic":
            continue
        same = np.ones(got.shape[0], bool)
        if entry in ab.CSR_ENTRIES and (c["long_row"], c["gpb"]) != (cb["long_row"], cb["gpb"]):
            same = ln <= min(c["long_row"], cb["long_row"])
        eq = np.equal(got, base).all(1)
        assert eq[same].all(), (f"{entry} F={F}: {layout} differs from dense on rows "
                                f"{np.flatnonzero(same & ~eq)[:8]}")


@pytest.mark.parametrize("live", ["null", "zero", "part"])
@pytest.mark.parametrize("F", [6, 68])
@pytest.mark.parametrize("entry", [e for e in ab.ENTRIES if e != "act_backward"])
def test_live_sizes(hip, entry, F, live):
    """the live size: a NULL pointer (the capacity), 0 (nothing written), and a
    device value below the rows the offsets describe (the rest untouched)"""
    layout = "pad32"
    c = ab.entry_cell(entry, F, layout)
    if c is None:
        with pytest.raises(Refused):
            _run(hip, entry, F, layout, live=live)
        return
    res = _run(hip, entry, F, layout, live=live)
    B, _ = _block()
    res["n_in"] = {"null": B["v"], "zero": 0, "part": B["v"] * 2 // 3}[live]
    _check(entry, F, layout, False, res, c)
    if entry == "csr_bwd_colmax":
        _colmax_check(F, layout, res)
    if entry == "fwd_act_bits":
        _bits_check(hip, F, layout, res)
