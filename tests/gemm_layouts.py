"""Operand layouts, the route table and the bars of the GEMM layout suite
(tests/test_gemm_layout_kernel.py on the GPU, tests/test_gemm_layouts_cpu.py
for this helper itself).

One call to a layer GEMM entry point is routed by csrc/gemm.hip's gemm() to
one of about a dozen kernels, each instantiated over load and store widths.
The routing reads the GEMM mode and the shape, the leading dimension of every
operand and the base-pointer alignment of A, B, C, the mask operand X and the
row map.  A fresh torch allocation is 256-byte aligned and dense, so the other
suites only ever reach a narrower width through an odd K, M or N.  Here every
operand is a view carved out of a sentinel-filled buffer at a chosen offset
from a 16-byte boundary and a chosen row pitch:

  view()       a [rows, cols] float32 view `base` floats past a 16-byte
               boundary, row stride `pitch`, one guard row or more on each
               side.  Inputs sit in NaN (a pad that reaches a sum shows), outputs
               in a fixed non-NaN bit pattern.
  rowmap()     the same for the int32 row map (0 or 1 element off 16 bytes).
  untouched()  every element of the buffer outside the view still holds the
               sentinel, bit for bit.

CELLS is the route table.  `route` is what the dispatcher's predicates send the
cell to, written down from reading csrc/gemm.hip, gemm3.hip and gemmx3.hip;
expected_route() restates those predicates in Python and the CPU test holds
the two against each other, so a cell whose literal route drifts from the
predicates fails without a GPU.  `by` names the predicate that decides the
cell against its aligned sibling.  Cells of one `group` differ only in a load
or store width (the kernel, the split count and the k order are the same), so
their results are bit-identical.

Bars (the project's own, no new constant):
  f32_bar()    routes that end on the fp32-input kernels: test_gemm_f32_mfma's
               tol = 2e-6 sqrt(K) + 1e-6, rtol = tol, atol = 4 tol (8 tol for the
               masked TN, as test_gemm_tn_masked).
  split_bar()  routes that end on a split kernel: test_gemm_split3._check — the
               error normalised by |A| |B| per element is at most 1.25 x the
               fp32 path's (on aligned dense copies of the same values) plus
               1e-7, and below 5e-7.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

# GEMM modes (nts/_abi.py)
F32, SPLIT3, SPLIT3_ALL = 0, 1, 2

NAN_BITS = 0x7FC00000                       # input sentinel (torch's quiet NaN)
OUT_BITS = 0xC3A5F00D - (1 << 32)           # output sentinel: -331.875..., as int32
_SENT = {"in": NAN_BITS, "out": OUT_BITS}
MAP_SENT = 0                                # row-map pad: a valid row id (never a wild read)

DROP_P, DROP_SEED, DROP_OFFSET = 0.5, 0x1234_5678_9ABC, 77
MASK_SCALE = 2.0


# ---------------------------------------------------------------------------
# layout builders

def _carve(n_view, lead, dtype, device, sent, shape, strides):
    flat = torch.empty(3 + lead + n_view + 4, dtype=dtype, device=device)
    flat.view(torch.int32).fill_(sent)
    skew = (-(flat.data_ptr() // 4)) % 4     # flat[skew] is 16-byte aligned
    v = flat.as_strided(shape, strides, skew + lead)
    return flat, v


def view(rows, cols, base, pitch, device, fill):
    """(flat, v): v a [rows, cols] float32 view of flat, its first element
    `base` floats past a 16-byte boundary, row stride `pitch`; flat holds the
    `fill` sentinel ("in": NaN, "out": OUT_BITS) everywhere, with at least one
    full row of guard before and after the view."""
    assert pitch >= max(cols, 1) and base >= 0 and rows >= 0
    guard = (pitch + 3) // 4 * 4
    flat, v = _carve(rows * pitch + guard, guard + base, torch.float32, device, _SENT[fill],
                     (rows, cols), (pitch, 1))
    lead = v.storage_offset() - flat.storage_offset()
    # (an empty view reports no data_ptr(): its address is the buffer's + the offset)
    addr = v.data_ptr() if v.numel() else flat.data_ptr() + 4 * lead
    assert addr % 16 == (4 * base) % 16
    assert v.stride() == (pitch, 1) and v.shape == (rows, cols)
    assert lead >= pitch and flat.numel() - (lead + rows * pitch) >= pitch
    return flat, v


def rowmap(ids, offset, device):
    """(flat, v): the int32 row map `offset` (0 or 1) elements past a 16-byte
    boundary, 8 guard elements of MAP_SENT on each side."""
    assert offset in (0, 1)
    n = int(ids.numel())
    flat, v = _carve(n + 8, 8 + offset, torch.int32, device, MAP_SENT, (n,), (1,))
    v.copy_(ids.to(torch.int32))
    assert v.data_ptr() % 16 == 4 * offset
    return flat, v


def untouched(flat, v, sent=None):
    """Every element of `flat` outside the view `v` still holds the sentinel,
    bit for bit.  The sentinel is read off the dtype and the first guard
    element unless given."""
    bits = flat.view(torch.int32)
    if sent is None:
        if flat.dtype == torch.int32:
            sent = MAP_SENT
        else:
            first = int(bits[0].item())
            if first not in (NAN_BITS, OUT_BITS):
                return False
            sent = first
    outside = torch.ones(flat.numel(), dtype=torch.bool, device=flat.device)
    if v.numel():
        start = v.storage_offset() - flat.storage_offset()
        if v.dim() == 1:
            outside[start:start + v.numel()] = False
        else:
            r = torch.arange(v.shape[0], device=flat.device)[:, None] * v.stride(0)
            c = torch.arange(v.shape[1], device=flat.device)[None, :]
            outside[(start + r + c).flatten()] = False
    return bool((bits[outside] == sent).all().item())


# ---------------------------------------------------------------------------
# the Philox keep mask of the relu/dropout epilogue (restated in numpy)

def _philox4x32_10(c, k):
    """Philox4x32-10 reference (numpy uint64 arithmetic), c: 4 x uint32 arrays, k: 2 ints."""
    M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
    c = [x.astype(np.uint64) for x in c]
    k0, k1 = np.uint64(k[0]), np.uint64(k[1])
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & mask
        hi1, lo1 = p1 >> np.uint64(32), p1 & mask
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(W0)) & mask
        k1 = (k1 + np.uint64(W1)) & mask
    return [x.astype(np.uint32) for x in c]


def _dropout_keep(M, N, p, seed, offset):
    """Element (row, col): 16 bits of Philox4x32-10 at counter {row/4, col/2, offset}
    (word row % 4, low half for even col, high half for odd), kept iff >= floor(p * 2^16)."""
    rows = np.arange(M, dtype=np.uint64)[:, None] * np.ones((1, N), np.uint64)
    cols = np.ones((M, 1), np.uint64) * np.arange(N, dtype=np.uint64)[None, :]
    c = [(rows >> np.uint64(2)).astype(np.uint32), (cols >> np.uint64(1)).astype(np.uint32),
         np.full((M, N), offset & 0xFFFFFFFF, np.uint32), np.full((M, N), offset >> 32, np.uint32)]
    w = _philox4x32_10(c, (seed & 0xFFFFFFFF, seed >> 32))
    word = np.choose((rows & np.uint64(3)).astype(np.int64), w).astype(np.uint64)
    bits = np.where((cols & np.uint64(1)) == 1, word >> np.uint64(16), word & np.uint64(0xFFFF))
    thr = 65536 if p >= 1.0 else min(int(p * 65536.0), 65536)
    return bits >= np.uint64(thr)


# ---------------------------------------------------------------------------
# the cell table

NN_ENTRIES = ("gemm", "gather", "relu_dropout")
TN_ENTRIES = ("gemm_tn", "tn_gather", "tn_masked")
ENTRY_POINTS = {
    "gemm": "nts_hip_gemm_f32", "gemm_tn": "nts_hip_gemm_f32",
    "gather": "nts_hip_gemm_gather_f32", "tn_gather": "nts_hip_gemm_tn_gather_f32",
    "relu_dropout": "nts_hip_gemm_relu_dropout_f32", "tn_masked": "nts_hip_gemm_tn_masked_f32",
}


@dataclass(frozen=True)
class Cell:
    """One dispatch cell.  A, B, C, X: (base, pad) — the operand's first
    element `base` floats past a 16-byte boundary, row pitch = its columns +
    `pad` (layout() gives (base, pitch)); mo: the row map's offset in elements."""
    id: str
    entry: str
    mode: int
    shape: tuple            # (M, N, K) of C[M, N] = op(A) B over K
    route: str
    by: str
    A: tuple = (0, 0)
    B: tuple = (0, 0)
    C: tuple = (0, 0)
    X: tuple = (0, 0)
    mo: int = 0
    group: str | None = None

    @property
    def trans(self):
        return self.entry in TN_ENTRIES

    @property
    def epi(self):
        return self.entry == "relu_dropout"

    @property
    def masked(self):
        return self.entry == "tn_masked"

    @property
    def mapped(self):
        return self.entry in ("gather", "tn_gather")

    def cols(self, op):
        M, N, K = self.shape
        return {"A": M if self.trans else K, "B": N, "C": N, "X": N}[op]

    def layout(self, op):
        """(base, pitch) of operand `op`."""
        base, pad = getattr(self, op)
        return base, max(self.cols(op), 1) + pad

    def table_rows(self):
        """Rows of the A operand (a table larger than the map's range when gathered)."""
        M, N, K = self.shape
        n = K if self.trans else M
        return n + n // 3 + 11 if self.mapped else n


def _c(id, entry, mode, shape, route, by, **kw):
    return Cell(id, entry, mode, shape, route, by, **kw)


_T4, _T1, _T1W = "k_sum_splits_tree<V4,T16>", "k_sum_splits_tree<V1,T16>", "k_sum_splits_tree<V1,T64>"
_ROWS = "k_sum_splits_rows"
_AV = "gemm.hip launch(): avec from inner % 4|2, lda % 4|2, A % 16|8"
_BF = "gemm.hip launch(): bfull = N % 128, ldb % 2, B % 8 (BMASK: ldbx % 2, bx % 8)"
_SS = "gemm.hip sum_splits(): v4 = N % 4, ldc % 4, C % 16; rows needs splits >= 64"
_WAV = "gemm.hip launch_wres(): avec from lda % 4|2, A % 16|8"
_WVS = "gemm.hip launch_wres(): vs = ldc % 4, C % 16"
_WB = "gemm.hip k_gemm_wres: B image by float4 iff ldb % 4, B % 16"
_TBA = "gemm.hip launch_tn_big(): a4 = lda % 4, A % 16; a2 = M % 2, lda % 2, A % 8"
_TBC = "gemm.hip k_gemm_tn_big: vec = ldc % 4, Cb % 16"
_TBOK = "gemm.hip tn_big_ok(): ldb % 4, B % 16 (mask: ldbx % 4, bx % 16)"
_V2 = "gemm3.hip gemm3_tn(): v2_ok = ldb % 4, B % 16, ldx % 4, X % 16, amap % 16"
_NNOK = "gemm3.hip gemm3_nn_ok(): lda % 4, A % 16"
_X3NN = "gemmx3.hip x3_nn_ok(): lda >= Kp, lda % 4, A % 16"
_X3ST = "gemmx3.hip k_x3_nn: store by f32x4 iff ldc % 4, C % 16"
_X3TN = "gemmx3.hip x3_tn_ok(): M >= 32, N % 128, K >= 256, lda >= Kp, lda % 4, A % 16, ldb % 4, B % 16 (mask too)"
_THR = "gemm.hip gemm(): NTS_GEMM_SPLIT3 takes (trans_a ? M : K) >= 256 or nnk"
_NNK = "gemm3.hip x3_nnk_ok(): K <= 128, M >= 4096, lda % 4, A % 16"
_NN7 = "gemmx3.hip x3_nn(): k_x3_nn7 iff x3_nn7_ok and (epi or ldc % 4, C % 16)"

KG = "k_gemm<%s,AV%d,bfull%d,EPI%d,BMASK%d>"
WR = "k_gemm_wres<NC%d,AV%d,EPI%d,D2,XT1>[%s,vs%d]"
TB = "k_gemm_tn_big<BMASK%d,AV%d,SG1,R%d>[%s]"
S3B = "k_split3_b+"

CELLS = [
    # ---- generic k_gemm, NTS_GEMM_F32 --------------------------------------
    # NN (70, 128, 40): wres_ncol = 0 (M < 2048); 2 tiles, 2 k-steps: no split
    _c("kg.nn.av4", "gemm", F32, (70, 128, 40), KG % ("NN", 4, 1, 0, 0), _AV, group="kg.nn"),
    _c("kg.nn.av2.base", "gemm", F32, (70, 128, 40), KG % ("NN", 2, 1, 0, 0), _AV, A=(2, 0),
       C=(1, 3), group="kg.nn"),
    _c("kg.nn.av1.base", "gemm", F32, (70, 128, 40), KG % ("NN", 1, 1, 0, 0), _AV, A=(1, 0),
       C=(0, 4), group="kg.nn"),
    _c("kg.nn.av2.pitch", "gemm", F32, (70, 128, 40), KG % ("NN", 2, 1, 0, 0), _AV, A=(0, 2),
       C=(2, 0), group="kg.nn"),
    _c("kg.nn.av1.pitch", "gemm", F32, (70, 128, 40), KG % ("NN", 1, 1, 0, 0), _AV, A=(0, 1),
       C=(3, 1), group="kg.nn"),
    _c("kg.nn.bfull0.base", "gemm", F32, (70, 128, 40), KG % ("NN", 4, 0, 0, 0), _BF, B=(1, 0),
       group="kg.nn"),
    _c("kg.nn.bfull0.pitch", "gemm", F32, (70, 128, 40), KG % ("NN", 4, 0, 0, 0), _BF, B=(0, 1),
       group="kg.nn"),
    _c("kg.nn.av1.bfull0", "gemm", F32, (70, 128, 40), KG % ("NN", 1, 0, 0, 0), _BF, A=(3, 1),
       B=(1, 1), C=(1, 1), group="kg.nn"),
    # the inner size alone
    _c("kg.nn.av2.inner", "gemm", F32, (70, 128, 42), KG % ("NN", 2, 1, 0, 0), _AV, group="kg.nn42"),
    _c("kg.nn.av1.inner42", "gemm", F32, (70, 128, 42), KG % ("NN", 1, 1, 0, 0), _AV, A=(1, 0),
       group="kg.nn42"),
    _c("kg.nn.av1.inner", "gemm", F32, (70, 128, 41), KG % ("NN", 1, 1, 0, 0), _AV, group="kg.nn41"),
    _c("kg.nn.av1.inner.bfull0", "gemm", F32, (70, 128, 41), KG % ("NN", 1, 0, 0, 0), _BF,
       B=(0, 3), group="kg.nn41"),
    # the row map (F32 mode: the same kernels, rows through amap)
    _c("kg.nn.gather", "gather", F32, (70, 128, 40), KG % ("NN", 4, 1, 0, 0), _AV, mo=1,
       group="kg.nng"),
    _c("kg.nn.gather.av1", "gather", F32, (70, 128, 40), KG % ("NN", 1, 1, 0, 0), _AV, A=(1, 4),
       group="kg.nng"),
    # N % 128 != 0 -> bfull 0; 4 tiles, 10 k-steps -> 2 splits, N % 4 != 0 -> scalar tree
    _c("kg.nn.split.av4", "gemm", F32, (70, 130, 300), KG % ("NN", 4, 0, 0, 0) + "+" + _T1, _BF,
       group="kg.nns"),
    _c("kg.nn.split.av2", "gemm", F32, (70, 130, 300), KG % ("NN", 2, 0, 0, 0) + "+" + _T1, _AV,
       A=(2, 2), C=(2, 6), group="kg.nns"),
    _c("kg.nn.split.av1", "gemm", F32, (70, 130, 300), KG % ("NN", 1, 0, 0, 0) + "+" + _T1, _AV,
       A=(3, 1), B=(1, 0), group="kg.nns"),
    # 2 splits with N % 4 == 0: the tree's vector / scalar choice on C alone
    _c("kg.nn.split.tree4", "gemm", F32, (70, 128, 300), KG % ("NN", 4, 1, 0, 0) + "+" + _T4, _SS,
       C=(0, 4), group="kg.nnt"),
    _c("kg.nn.split.tree1.base", "gemm", F32, (70, 128, 300), KG % ("NN", 4, 1, 0, 0) + "+" + _T1,
       _SS, C=(1, 0), group="kg.nnt"),
    _c("kg.nn.split.tree1.pitch", "gemm", F32, (70, 128, 300), KG % ("NN", 4, 1, 0, 0) + "+" + _T1,
       _SS, C=(0, 2), group="kg.nnt"),
    _c("kg.nn.tiny", "gemm", F32, (37, 7, 13), KG % ("NN", 1, 0, 0, 0), _AV, A=(1, 2), B=(3, 0),
       C=(1, 2)),
    _c("kg.tn.tiny", "gemm_tn", F32, (37, 7, 13), KG % ("TN", 1, 0, 0, 0), _AV, A=(2, 1), B=(0, 1),
       C=(3, 0)),
    # TN (132, 128, 40): 129 <= M < 320 keeps it off k_gemm_tn_big
    _c("kg.tn.av4", "gemm_tn", F32, (132, 128, 40), KG % ("TN", 4, 1, 0, 0), _AV, group="kg.tn"),
    _c("kg.tn.av2.base", "gemm_tn", F32, (132, 128, 40), KG % ("TN", 2, 1, 0, 0), _AV, A=(2, 0),
       C=(1, 0), group="kg.tn"),
    _c("kg.tn.av1.base", "gemm_tn", F32, (132, 128, 40), KG % ("TN", 1, 1, 0, 0), _AV, A=(1, 0),
       group="kg.tn"),
    _c("kg.tn.av2.pitch", "gemm_tn", F32, (132, 128, 40), KG % ("TN", 2, 1, 0, 0), _AV, A=(0, 2),
       group="kg.tn"),
    _c("kg.tn.av1.pitch", "gemm_tn", F32, (132, 128, 40), KG % ("TN", 1, 1, 0, 0), _AV, A=(0, 1),
       C=(0, 3), group="kg.tn"),
    _c("kg.tn.bfull0.base", "gemm_tn", F32, (132, 128, 40), KG % ("TN", 4, 0, 0, 0), _BF, B=(1, 0),
       group="kg.tn"),
    _c("kg.tn.bfull0.pitch", "gemm_tn", F32, (132, 128, 40), KG % ("TN", 4, 0, 0, 0), _BF, B=(2, 1),
       group="kg.tn"),
    _c("kg.tn.av2.bfull0", "gemm_tn", F32, (132, 128, 40), KG % ("TN", 2, 0, 0, 0), _BF, A=(2, 0),
       B=(1, 0), C=(0, 4), group="kg.tn"),
    _c("kg.tn.av2.inner", "gemm_tn", F32, (130, 128, 40), KG % ("TN", 2, 1, 0, 0), _AV,
       group="kg.tn130"),
    _c("kg.tn.av1.inner130", "gemm_tn", F32, (130, 128, 40), KG % ("TN", 1, 1, 0, 0), _AV, A=(0, 1),
       group="kg.tn130"),
    _c("kg.tn.av1.inner", "gemm_tn", F32, (131, 128, 40), KG % ("TN", 1, 1, 0, 0), _AV, A=(0, 1)),
    _c("kg.tn.split.av4", "gemm_tn", F32, (132, 130, 300), KG % ("TN", 4, 0, 0, 0) + "+" + _T1, _BF,
       group="kg.tns"),
    _c("kg.tn.split.av1", "gemm_tn", F32, (132, 130, 300), KG % ("TN", 1, 0, 0, 0) + "+" + _T1, _AV,
       A=(1, 0), C=(1, 2), group="kg.tns"),
    # EPI (never split) and BMASK
    _c("kg.epi.av4", "relu_dropout", F32, (70, 128, 40), KG % ("NN", 4, 1, 1, 0), _AV,
       group="kg.epi"),
    _c("kg.epi.av1.bfull0", "relu_dropout", F32, (70, 128, 40), KG % ("NN", 1, 0, 1, 0), _BF,
       A=(1, 0), B=(0, 1), C=(3, 5), group="kg.epi"),
    _c("kg.bmask.bfull1", "tn_masked", F32, (132, 128, 40), KG % ("TN", 4, 1, 0, 1), _BF,
       group="kg.bm"),
    _c("kg.bmask.x.base", "tn_masked", F32, (132, 128, 40), KG % ("TN", 4, 0, 0, 1), _BF, X=(1, 0),
       C=(2, 2), group="kg.bm"),
    _c("kg.bmask.x.pitch", "tn_masked", F32, (132, 128, 40), KG % ("TN", 2, 0, 0, 1), _BF, A=(2, 0),
       X=(0, 1), group="kg.bm"),
    # many splits at a tiny M x N: 1 tile, 256 k-steps -> 64 splits; 1028 -> 257
    _c("ss.rows", "gemm", F32, (8, 8, 8192), KG % ("NN", 4, 0, 0, 0) + "+" + _ROWS, _SS, C=(0, 4)),
    _c("ss.rows.c.base", "gemm", F32, (8, 8, 8192), KG % ("NN", 4, 0, 0, 0) + "+" + _T1, _SS,
       C=(1, 0), group="ss.t1"),
    _c("ss.rows.c.pitch", "gemm", F32, (8, 8, 8192), KG % ("NN", 4, 0, 0, 0) + "+" + _T1, _SS,
       C=(0, 1), group="ss.t1"),
    _c("ss.rows.n6", "gemm", F32, (8, 6, 8192), KG % ("NN", 4, 0, 0, 0) + "+" + _T1, _SS),
    _c("ss.wide.rows", "gemm", F32, (8, 8, 32896), KG % ("NN", 4, 0, 0, 0) + "+" + _ROWS, _SS),
    _c("ss.wide.tree1", "gemm", F32, (8, 8, 32896), KG % ("NN", 4, 0, 0, 0) + "+" + _T1W, _SS,
       C=(0, 1)),

    # ---- k_gemm_wres, NTS_GEMM_F32 ------------------------------------------
    # NC 128, K = 64: two full k-blocks, cross-task prefetch
    _c("wres.128.av4", "gemm", F32, (2048, 128, 64), WR % (128, 4, 0, "bimg4", 1), _WAV,
       group="wres.128"),
    _c("wres.128.av2", "gemm", F32, (2048, 128, 64), WR % (128, 2, 0, "bimg4", 1), _WAV, A=(2, 2),
       B=(0, 4), C=(0, 4), group="wres.128"),
    _c("wres.128.av1.base", "gemm", F32, (2048, 128, 64), WR % (128, 1, 0, "bimg4", 1), _WAV,
       A=(1, 0), group="wres.128"),
    _c("wres.128.av1.pitch", "gemm", F32, (2048, 128, 64), WR % (128, 1, 0, "bimg4", 1), _WAV,
       A=(0, 1), group="wres.128"),
    _c("wres.128.vs0.base", "gemm", F32, (2048, 128, 64), WR % (128, 4, 0, "bimg4", 0), _WVS,
       C=(1, 0), group="wres.128"),
    _c("wres.128.vs0.pitch", "gemm", F32, (2048, 128, 64), WR % (128, 4, 0, "bimg4", 0), _WVS,
       C=(0, 2), group="wres.128"),
    _c("wres.128.bimg1.base", "gemm", F32, (2048, 128, 64), WR % (128, 4, 0, "bimg1", 1), _WB,
       B=(1, 0), group="wres.128"),
    _c("wres.128.bimg1.pitch", "gemm", F32, (2048, 128, 64), WR % (128, 4, 0, "bimg1", 1), _WB,
       B=(0, 2), group="wres.128"),
    # K = 70: a partial last k-block; M = 2049: a last task of one row
    _c("wres.128.tail.av4", "gemm", F32, (2049, 128, 70), WR % (128, 4, 0, "bimg4", 1), _WAV,
       A=(0, 2), group="wres.128t"),
    _c("wres.128.tail.av2", "gemm", F32, (2049, 128, 70), WR % (128, 2, 0, "bimg1", 0), _WAV,
       A=(2, 0), B=(3, 0), C=(2, 0), group="wres.128t"),
    _c("wres.128.tail.epi", "relu_dropout", F32, (2049, 128, 70), WR % (128, 4, 1, "bimg4", 1),
       _WAV, A=(0, 2), group="wres.128e"),
    _c("wres.128.tail.epi.av1", "relu_dropout", F32, (2049, 128, 70), WR % (128, 1, 1, "bimg4", 0),
       _WAV, A=(0, 1), C=(0, 1), group="wres.128e"),
    _c("wres.128.gather", "gather", F32, (2048, 128, 64), WR % (128, 4, 0, "bimg4", 1), _WAV, mo=1),
    # NC 64: N % 128 != 0 (or K > 288); K = 300: 9 full k-blocks and a tail
    _c("wres.64.av4", "gemm", F32, (2048, 64, 300), WR % (64, 4, 0, "bimg4", 1), _WAV,
       group="wres.64"),
    _c("wres.64.av1", "gemm", F32, (2048, 64, 300), WR % (64, 1, 0, "bimg1", 0), _WAV, A=(0, 1),
       B=(3, 0), C=(2, 0), group="wres.64"),
    _c("wres.64.av2", "gemm", F32, (2048, 64, 300), WR % (64, 2, 0, "bimg1", 0), _WAV, A=(2, 0),
       B=(0, 1), C=(0, 1), group="wres.64"),
    # K = 320: ten full k-blocks, three column blocks
    _c("wres.64.full", "gemm", F32, (2049, 192, 320), WR % (64, 4, 0, "bimg4", 1), _WAV,
       group="wres.64f"),
    _c("wres.64.full.epi", "relu_dropout", F32, (2049, 192, 320), WR % (64, 4, 1, "bimg4", 1), _WAV,
       group="wres.64fe"),
    _c("wres.64.full.epi.av2", "relu_dropout", F32, (2049, 192, 320), WR % (64, 2, 1, "bimg4", 0),
       _WAV, A=(2, 2), C=(1, 0), group="wres.64fe"),
    _c("wres.64.full.av1", "gemm", F32, (2049, 192, 320), WR % (64, 1, 0, "bimg4", 1), _WAV,
       A=(3, 0), group="wres.64f"),

    # ---- k_gemm_tn_big, NTS_GEMM_F32 ----------------------------------------
    # R = 1 (M <= 128); K = 64: one split, the direct store
    _c("tb.r1.a4", "gemm_tn", F32, (100, 128, 64), TB % (0, 4, 1, "vec"), _TBA, group="tb.r1"),
    _c("tb.r1.a4.c.base", "gemm_tn", F32, (100, 128, 64), TB % (0, 4, 1, "scalar"), _TBC, C=(1, 0),
       group="tb.r1"),
    _c("tb.r1.a4.c.pitch", "gemm_tn", F32, (100, 128, 64), TB % (0, 4, 1, "scalar"), _TBC,
       C=(0, 2), group="tb.r1"),
    _c("tb.r1.a2", "gemm_tn", F32, (100, 128, 64), TB % (0, 2, 1, "vec"), _TBA, A=(2, 0), C=(0, 4),
       group="tb.r1"),
    _c("tb.r1.a1", "gemm_tn", F32, (100, 128, 64), TB % (0, 1, 1, "vec"), _TBA, A=(0, 1),
       group="tb.r1"),
    # lda % 4 == 0 with lda >= M already gives lda >= roundup(M, 4): a dense
    # [K, 98] operand (lda = 98) loses a4 on lda % 4, an aligned base or not
    _c("tb.r1.m98.dense", "gemm_tn", F32, (98, 128, 64), TB % (0, 2, 1, "vec"), _TBA,
       group="tb.r1m98"),
    _c("tb.r1.m98.a4", "gemm_tn", F32, (98, 128, 64), TB % (0, 4, 1, "vec"), _TBA, A=(0, 2),
       group="tb.r1m98"),
    # 5 splits of 64 (K = 300)
    _c("tb.r1.split", "gemm_tn", F32, (128, 128, 300), TB % (0, 4, 1, "vec") + "+" + _T4, _TBA,
       group="tb.r1s"),
    _c("tb.r1.split.a1", "gemm_tn", F32, (128, 128, 300), TB % (0, 1, 1, "vec") + "+" + _T1, _SS,
       A=(1, 0), C=(1, 0), group="tb.r1s"),
    _c("tb.r1.split.gather", "tn_gather", F32, (128, 128, 300), TB % (0, 4, 1, "vec") + "+" + _T4,
       _TBA, mo=1),
    _c("tb.r1.bmask", "tn_masked", F32, (128, 128, 300), TB % (1, 4, 1, "vec") + "+" + _T4, _TBOK,
       X=(0, 4), group="tb.r1bm"),
    _c("tb.r1.bmask.a2", "tn_masked", F32, (128, 128, 300), TB % (1, 2, 1, "vec") + "+" + _T1, _TBA,
       A=(2, 0), C=(0, 1), group="tb.r1bm"),
    # R = 5 (M >= 320)
    _c("tb.r5.a4", "gemm_tn", F32, (320, 128, 64), TB % (0, 4, 5, "vec"), _TBA, group="tb.r5"),
    _c("tb.r5.a2", "gemm_tn", F32, (320, 128, 64), TB % (0, 2, 5, "scalar"), _TBA, A=(2, 0),
       C=(3, 0), group="tb.r5"),
    _c("tb.r5.a1.base", "gemm_tn", F32, (320, 128, 64), TB % (0, 1, 5, "vec"), _TBA, A=(1, 0),
       group="tb.r5"),
    _c("tb.r5.a1.pitch", "gemm_tn", F32, (320, 128, 64), TB % (0, 1, 5, "scalar"), _TBA, A=(0, 1),
       C=(0, 3), group="tb.r5"),
    # M = 322: the a4 loads run into the row padding (lda = 324), zeroed when staged
    _c("tb.r5.split.a4.pad", "gemm_tn", F32, (322, 128, 300), TB % (0, 4, 5, "vec") + "+" + _T4,
       _TBA, A=(0, 2), group="tb.r5s"),
    _c("tb.r5.split.a2", "gemm_tn", F32, (322, 128, 300), TB % (0, 2, 5, "vec") + "+" + _T1, _TBA,
       C=(2, 0), group="tb.r5s"),
    _c("tb.r5.bmask", "tn_masked", F32, (320, 128, 64), TB % (1, 4, 5, "vec"), _TBOK),
    # off k_gemm_tn_big on alignment alone
    _c("tb.fall.b.base", "gemm_tn", F32, (100, 128, 64), KG % ("TN", 4, 1, 0, 0), _TBOK, B=(2, 0)),
    _c("tb.fall.b.pitch", "gemm_tn", F32, (100, 128, 64), KG % ("TN", 4, 1, 0, 0), _TBOK, B=(0, 2)),
    _c("tb.fall.x.base", "tn_masked", F32, (100, 128, 64), KG % ("TN", 4, 1, 0, 1), _TBOK, X=(2, 0)),
    _c("tb.fall.x.odd", "tn_masked", F32, (100, 128, 64), KG % ("TN", 4, 0, 0, 1), _TBOK, X=(1, 0)),

    # ---- split paths ---------------------------------------------------------
    # k_gemm3_nn<E, MP>: 256 <= M < 4096 off the x3 forms
    _c("g3nn.dense", "gemm", SPLIT3_ALL, (256, 16, 40), S3B + "k_gemm3_nn<E0,MP0>", _NNOK, A=(0, 4),
       C=(1, 3)),
    _c("g3nn.epi", "relu_dropout", SPLIT3_ALL, (257, 144, 40), S3B + "k_gemm3_nn<E1,MP0>", _NNOK,
       C=(2, 0)),
    _c("g3nn.map.short_pitch", "gather", SPLIT3_ALL, (257, 144, 40), S3B + "k_gemm3_nn<E0,MP1>",
       _X3NN, mo=1, C=(0, 4)),
    _c("g3nn.fall.base", "gemm", SPLIT3_ALL, (256, 16, 40), KG % ("NN", 1, 0, 0, 0), _NNOK,
       A=(1, 0)),
    _c("g3nn.fall.pitch", "gemm", SPLIT3_ALL, (256, 16, 40), KG % ("NN", 2, 0, 0, 0), _NNOK,
       A=(0, 2)),
    # k_x3_nn through a row map (the pitch covers Kp = 64), its C store both ways
    _c("x3nn.map", "gather", SPLIT3_ALL, (257, 16, 40), S3B + "k_x3_nn<E0>[vec]", _X3NN, A=(0, 24),
       group="x3nn"),
    _c("x3nn.map.c.base", "gather", SPLIT3_ALL, (257, 16, 40), S3B + "k_x3_nn<E0>[scalar]", _X3ST,
       A=(0, 24), C=(1, 0), mo=1, group="x3nn"),
    _c("x3nn.map.c.pitch", "gather", SPLIT3_ALL, (257, 16, 40), S3B + "k_x3_nn<E0>[scalar]", _X3ST,
       A=(0, 28), C=(0, 2), group="x3nn"),
    _c("x3nn.fall.table.base", "gather", SPLIT3_ALL, (257, 16, 40), KG % ("NN", 1, 0, 0, 0), _NNOK,
       A=(1, 24)),
    # k_x3_nnk: dense rows, M >= 4096, K <= 128
    _c("nnk.dense", "gemm", SPLIT3_ALL, (4096, 16, 40), S3B + "k_x3_nnk<E0>", _NNK, A=(0, 4),
       C=(1, 0)),
    _c("nnk.epi", "relu_dropout", SPLIT3_ALL, (4097, 144, 100), S3B + "k_x3_nnk<E1>", _NNK,
       C=(0, 3)),
    _c("nnk.split3", "gemm", SPLIT3, (4096, 16, 40), S3B + "k_x3_nnk<E0>", _THR),
    _c("nnk.split3.fall.base", "gemm", SPLIT3, (4096, 16, 40), KG % ("NN", 1, 0, 0, 0), _NNK,
       A=(1, 0)),
    _c("nnk.all.fall.pitch", "gemm", SPLIT3_ALL, (4096, 16, 40), KG % ("NN", 1, 0, 0, 0), _NNOK,
       A=(0, 1)),
    # the % 256 threshold of NTS_GEMM_SPLIT3, both sides
    _c("thr.nn.256", "gemm", SPLIT3, (257, 16, 256), S3B + "k_gemm3_nn<E0,MP0>", _THR),
    _c("thr.nn.255", "gemm", SPLIT3, (257, 16, 255), KG % ("NN", 1, 0, 0, 0) + "+" + _T4, _THR),
    _c("thr.tn.256", "gemm_tn", SPLIT3, (256, 16, 256), "k_s3_tn<TPW3,BM0,MP0>+" + _T4, _THR),
    _c("thr.tn.255", "gemm_tn", SPLIT3, (255, 16, 256), KG % ("TN", 1, 0, 0, 0) + "+" + _T4, _THR),
    # k_x3_nn7 (M >= 32768, >= 4 k-steps); its plain store is always 16 bytes
    _c("nn7.dense", "gemm", SPLIT3_ALL, (32768, 16, 128), S3B + "k_x3_nn7<RT7,E0>", _NN7, A=(0, 4),
       C=(0, 4)),
    _c("nn7.epi", "relu_dropout", SPLIT3_ALL, (32768, 16, 128), S3B + "k_x3_nn7<RT7,E1>", _NN7,
       C=(1, 2)),
    _c("nn7.c.base", "gemm", SPLIT3_ALL, (32768, 16, 128), S3B + "k_x3_nn<E0>[scalar]", _NN7,
       C=(1, 0)),
    _c("nn7.c.pitch", "gemm", SPLIT3_ALL, (32768, 16, 128), S3B + "k_x3_nn<E0>[scalar]", _NN7,
       C=(0, 2)),
    # k_x3_tn (row-gathered TN) and the fall-back for every conjunct of x3_tn_ok
    _c("x3tn", "tn_gather", SPLIT3_ALL, (40, 128, 256), "k_x3_tn<TPW5,PR1,BM0>+" + _T4, _X3TN,
       A=(0, 24), group="x3tn"),
    _c("x3tn.c", "tn_gather", SPLIT3_ALL, (40, 128, 256), "k_x3_tn<TPW5,PR1,BM0>+" + _T1, _SS,
       A=(0, 24), C=(1, 0), mo=1, group="x3tn"),
    _c("x3tn.fall.lda_kp", "tn_gather", SPLIT3_ALL, (40, 128, 256), "k_s3_tn<TPW3,BM0,MP1>+" + _T4,
       _X3TN, group="x3tn.s3"),
    _c("x3tn.fall.lda4", "tn_gather", SPLIT3_ALL, (40, 128, 256), "k_s3_tn<TPW3,BM0,MP1>+" + _T4,
       _X3TN, A=(0, 25), group="x3tn.s3"),
    _c("x3tn.fall.a.base", "tn_gather", SPLIT3_ALL, (40, 128, 256), "k_s3_tn<TPW3,BM0,MP1>+" + _T4,
       _X3TN, A=(1, 24), group="x3tn.s3"),
    _c("x3tn.fall.ldb4", "tn_gather", SPLIT3_ALL, (40, 128, 256), "k_gemm3_tn<BM0,MP1>+" + _T4,
       _X3TN, A=(0, 24), B=(0, 2), group="x3tn.g3"),
    _c("x3tn.fall.b.base", "tn_gather", SPLIT3_ALL, (40, 128, 256), "k_gemm3_tn<BM0,MP1>+" + _T4,
       _X3TN, A=(0, 24), B=(1, 0), group="x3tn.g3"),
    _c("x3tn.fall.n128", "tn_gather", SPLIT3_ALL, (40, 16, 256), "k_s3_tn<TPW3,BM0,MP1>+" + _T4,
       _X3TN, A=(0, 24)),
    _c("x3tn.fall.m32", "tn_gather", SPLIT3_ALL, (24, 128, 256), "k_s3_tn<TPW3,BM0,MP1>+" + _T4,
       _X3TN, A=(0, 8)),
    _c("x3tn.fall.k256", "tn_gather", SPLIT3_ALL, (40, 128, 255),
       TB % (0, 4, 1, "vec") + "+" + _T4, _X3TN, A=(0, 24)),
    # the masked one-tile form (any split mode), and its fall-backs
    _c("x3tnbm", "tn_masked", SPLIT3, (40, 128, 256), "k_x3_tn<TPW1,PR1,BM1>+" + _T4, _X3TN,
       A=(0, 24), X=(0, 4), group="x3tnbm"),
    _c("x3tnbm.c", "tn_masked", SPLIT3_ALL, (40, 128, 256), "k_x3_tn<TPW1,PR1,BM1>+" + _T1, _SS,
       A=(0, 24), C=(0, 1), group="x3tnbm"),
    _c("x3tnbm.fall.x.base", "tn_masked", SPLIT3_ALL, (40, 128, 256), "k_gemm3_tn<BM1,MP0>+" + _T4,
       _X3TN, A=(0, 24), X=(1, 0), group="x3tnbm.g3"),
    _c("x3tnbm.fall.ldx4", "tn_masked", SPLIT3_ALL, (40, 128, 256), "k_gemm3_tn<BM1,MP0>+" + _T4,
       _X3TN, A=(0, 24), X=(0, 2), group="x3tnbm.g3"),
    _c("x3tnbm.fall.lda_kp", "tn_masked", SPLIT3_ALL, (40, 128, 256),
       "k_s3_tn<TPW3,BM1,MP0>+" + _T4, _X3TN, group="x3tnbm.s3"),
    _c("x3tnbm.fall.a.base", "tn_masked", SPLIT3_ALL, (40, 128, 256), "k_s3_tn<TPW3,BM1,MP0>+" + _T4,
       _X3TN, A=(1, 24), group="x3tnbm.s3"),
    _c("x3tnbm.fall.lda4", "tn_masked", SPLIT3_ALL, (40, 128, 256), "k_s3_tn<TPW3,BM1,MP0>+" + _T4,
       _X3TN, A=(0, 25), group="x3tnbm.s3"),
    _c("x3tnbm.fall.b.base", "tn_masked", SPLIT3_ALL, (40, 128, 256), "k_gemm3_tn<BM1,MP0>+" + _T4,
       _X3TN, A=(0, 24), B=(1, 0), group="x3tnbm.g3"),
    _c("x3tnbm.fall.ldb4", "tn_masked", SPLIT3_ALL, (40, 128, 256), "k_gemm3_tn<BM1,MP0>+" + _T4,
       _X3TN, A=(0, 24), B=(0, 2), group="x3tnbm.g3"),
    _c("x3tnbm.fall.n128", "tn_masked", SPLIT3_ALL, (40, 16, 256), "k_s3_tn<TPW3,BM1,MP0>+" + _T4,
       _X3TN, A=(0, 24)),
    _c("x3tnbm.fall.m32", "tn_masked", SPLIT3_ALL, (24, 128, 256), "k_s3_tn<TPW3,BM1,MP0>+" + _T4,
       _X3TN, A=(0, 8)),
    _c("x3tnbm.fall.m128", "tn_masked", SPLIT3_ALL, (160, 128, 256), "k_s3_tn<TPW3,BM1,MP0>+" + _T4,
       "gemmx3.hip x3_tn_bm_ok(): M <= 128"),
    _c("x3tnbm.fall.k256", "tn_masked", SPLIT3_ALL, (40, 128, 255),
       TB % (1, 4, 1, "vec") + "+" + _T4, _X3TN, A=(0, 24)),
    _c("x3tnbm.fall.split3.m", "tn_masked", SPLIT3, (40, 128, 256),
       TB % (1, 4, 1, "vec") + "+" + _T4, _THR),
    # k_s3_tn<TPW, BM, MP> (BM1 with MP1 has no entry point: the masked TN takes no row map)
    _c("s3tn", "gemm_tn", SPLIT3_ALL, (41, 64, 300), "k_s3_tn<TPW3,BM0,MP0>+" + _T4, _V2,
       A=(1, 2), group="g3tn.s3"),
    _c("s3tn.c", "gemm_tn", SPLIT3_ALL, (41, 64, 300), "k_s3_tn<TPW3,BM0,MP0>+" + _T1, _SS,
       C=(1, 0), group="g3tn.s3"),
    _c("s3tn.bmask", "tn_masked", SPLIT3_ALL, (333, 128, 777), "k_s3_tn<TPW3,BM1,MP0>+" + _T4, _V2,
       A=(0, 3), X=(0, 4)),
    # k_gemm3_tn<BM, MP>, by each cause that fails v2_ok
    _c("g3tn.b.base", "gemm_tn", SPLIT3_ALL, (41, 64, 300), "k_gemm3_tn<BM0,MP0>+" + _T4, _V2,
       B=(1, 0), group="g3tn"),
    _c("g3tn.b.pitch", "gemm_tn", SPLIT3_ALL, (41, 64, 300), "k_gemm3_tn<BM0,MP0>+" + _T4, _V2,
       A=(1, 2), B=(0, 2), C=(0, 4), group="g3tn"),
    _c("g3tn.b.base.c", "gemm_tn", SPLIT3_ALL, (41, 64, 300), "k_gemm3_tn<BM0,MP0>+" + _T1, _SS,
       B=(3, 0), C=(1, 0), group="g3tn"),
    _c("g3tn.x.base", "tn_masked", SPLIT3_ALL, (333, 128, 777), "k_gemm3_tn<BM1,MP0>+" + _T4, _V2,
       X=(1, 0), group="g3tn.bm"),
    _c("g3tn.x.pitch", "tn_masked", SPLIT3_ALL, (333, 128, 777), "k_gemm3_tn<BM1,MP0>+" + _T1, _V2,
       X=(0, 2), C=(2, 0), group="g3tn.bm"),
    _c("g3tn.map", "tn_gather", SPLIT3_ALL, (100, 16, 256), "k_gemm3_tn<BM0,MP1>+" + _T4, _V2,
       mo=1, group="g3tn.mp"),
    _c("g3tn.map.c", "tn_gather", SPLIT3_ALL, (100, 16, 256), "k_gemm3_tn<BM0,MP1>+" + _T1, _SS,
       mo=1, A=(2, 1), C=(0, 1), group="g3tn.mp"),
    _c("s3tn.map", "tn_gather", SPLIT3_ALL, (100, 16, 256), "k_s3_tn<TPW3,BM0,MP1>+" + _T4, _V2),
    # one split: 129 row groups of 160 leave no room to split K; the direct store
    _c("g3tn.direct", "gemm_tn", SPLIT3_ALL, (20500, 16, 256), "k_gemm3_tn<BM0,MP0>", _V2, B=(1, 0),
       group="g3tn.d"),
    _c("g3tn.direct.c", "gemm_tn", SPLIT3_ALL, (20500, 16, 256), "k_gemm3_tn<BM0,MP0>", _V2,
       B=(0, 1), C=(1, 2), group="g3tn.d"),

    # ---- degenerate shapes on a padded, offset C ------------------------------
    _c("deg.k0", "gemm", F32, (37, 7, 0), "memset", "gemm.hip gemm(): K == 0", C=(1, 2)),
    _c("deg.k0.tn", "gemm_tn", SPLIT3_ALL, (37, 16, 0), "memset", "gemm.hip gemm(): K == 0",
       C=(3, 4)),
    _c("deg.m1", "gemm", F32, (1, 7, 13), KG % ("NN", 1, 0, 0, 0), _AV, C=(1, 2)),
    _c("deg.m1.tn", "gemm_tn", F32, (1, 128, 40), TB % (0, 1, 1, "scalar"), _TBA, C=(1, 0)),
    _c("deg.n1", "gemm", F32, (37, 1, 13), KG % ("NN", 1, 0, 0, 0), _AV, C=(1, 2)),
    _c("deg.n1.tn", "gemm_tn", F32, (37, 1, 13), KG % ("TN", 1, 0, 0, 0), _AV, B=(1, 1), C=(2, 3)),
    _c("deg.m0", "gemm", F32, (0, 7, 13), "none", "NTS_GEMM_ARGS_CHECK: M == 0 || N == 0", C=(1, 2)),
    _c("deg.n0", "gemm_tn", F32, (37, 0, 13), "none", "NTS_GEMM_ARGS_CHECK: M == 0 || N == 0",
       C=(1, 2)),
]

BY_ID = {c.id: c for c in CELLS}

# Instances the C ABI cannot reach (found while writing the table):
#   k_gemm3_tn<BM1,MP1>, k_s3_tn<TPW3,BM1,MP1>   the masked TN takes no row map
#   k_gemm3_nn<E1,MP1>, k_x3_nn<E1>              the epilogue NN takes no row map
#   k_sum_splits_tree<V4,T64>                    v4 with >= 64 splits is k_sum_splits_rows
UNREACHABLE = ("k_gemm3_tn<BM1,MP1>", "k_s3_tn<TPW3,BM1,MP1>", "k_gemm3_nn<E1,MP1>", "k_x3_nn<E1>",
               "k_sum_splits_tree<V4,T64>")

# every kernel / instance the suite pins (each is the route of at least one cell)
REQUIRED = tuple(
    [KG % (t, av, bf, 0, 0) for t in ("NN", "TN") for av in (4, 2, 1) for bf in (0, 1)] +
    [KG % ("NN", 4, 1, 1, 0), KG % ("NN", 1, 0, 1, 0), KG % ("TN", 4, 1, 0, 1), KG % ("TN", 4, 0, 0, 1)] +
    ["k_gemm_wres<NC%d,AV%d,EPI0" % (nc, av) for nc in (128, 64) for av in (4, 2, 1)] +
    ["k_gemm_wres<NC128,AV4,EPI1", "k_gemm_wres<NC64,AV4,EPI1", "bimg1", "vs0"] +
    ["k_gemm_tn_big<BMASK0,AV%d,SG1,R%d>" % (av, r) for av in (4, 2, 1) for r in (1, 5)] +
    ["k_gemm_tn_big<BMASK1,AV4,SG1,R1>", "k_gemm_tn_big<BMASK1,AV4,SG1,R5>"] +
    [_ROWS, _T4, _T1, _T1W, "k_split3_b"] +
    ["k_gemm3_nn<E0,MP0>", "k_gemm3_nn<E1,MP0>", "k_gemm3_nn<E0,MP1>", "k_x3_nnk<E0>", "k_x3_nnk<E1>",
     "k_x3_nn<E0>[vec]", "k_x3_nn<E0>[scalar]", "k_x3_nn7<RT7,E0>", "k_x3_nn7<RT7,E1>",
     "k_x3_tn<TPW5,PR1,BM0>", "k_x3_tn<TPW1,PR1,BM1>",
     "k_s3_tn<TPW3,BM0,MP0>", "k_s3_tn<TPW3,BM0,MP1>", "k_s3_tn<TPW3,BM1,MP0>",
     "k_gemm3_tn<BM0,MP0>", "k_gemm3_tn<BM0,MP1>", "k_gemm3_tn<BM1,MP0>", "memset"])


def groups():
    g = {}
    for c in CELLS:
        if c.group:
            g.setdefault(c.group, []).append(c)
    return g


# ---------------------------------------------------------------------------
# the dispatcher's predicates, restated (csrc/gemm.hip gemm() and what it calls)

def _cd(a, b):
    return (a + b - 1) // b


def _sum_splits(splits, N, cbase, ldc):
    v4 = N % 4 == 0 and ldc % 4 == 0 and cbase % 4 == 0
    if v4 and splits >= 64:          # the partials are M * N apart in 256-byte aligned scratch
        return _ROWS
    return "k_sum_splits_tree<V%d,T%d>" % (4 if v4 else 1, 64 if splits > 256 else 16)


def _x3_tn_ok(M, N, K, ab, lda, bb, ldb, masked, xb, ldx):
    Kp = _cd(M, 32) * 32
    lds = 3 * 16 * 4 * Kp + 2 * 8192 + 6 * 4096 + (2 * 8192 if masked else 0) + 4 * 16 * 3 + 4 * 256
    return (M >= 32 and lds <= 160 * 1024 and N % 128 == 0 and K >= 256 and lda >= Kp and
            lda % 4 == 0 and ab % 4 == 0 and ldb % 4 == 0 and bb % 4 == 0 and
            (not masked or (ldx % 4 == 0 and xb % 4 == 0)))


def _x3_tn(M, N, K, masked, cbase, ldc):
    RB = 4 * _cd(M, 32) * 32
    nnb, ksteps = N // 128, _cd(K, 16)
    splits = max(1, min(256 // nnb, ksteps // 8))
    kchunk = _cd(ksteps, splits) * 16
    fixed = 3 * 16 * RB + 2 * 8192 + 6 * 4096 + (2 * 8192 if masked else 0) + 4 * 16 * 3
    kchunk = min(kchunk, (160 * 1024 - fixed) // 4 // 16 * 16)
    splits = _cd(K, kchunk)
    pr, tpw = _cd(RB, 1024), (_cd(M, 32) + 3) // 4
    if masked:
        assert tpw <= 1 and pr == 1
        k = "k_x3_tn<TPW1,PR1,BM1>"
    else:
        k = "k_x3_tn<TPW5,PR%d,BM0>" % pr
    return k + ("+" + _sum_splits(splits, N, cbase, ldc) if splits > 1 else "")


def expected_route(c: Cell) -> str:
    M, N, K = c.shape
    (ab, lda), (bb, ldb), (cb, ldc), (xb, ldx) = (c.layout(o) for o in "ABCX")
    trans, epi, bm, amap = c.trans, c.epi, c.masked, c.mapped
    if M == 0 or N == 0:
        return "none"
    if K == 0:
        return "memset"
    a16, a8 = ab % 4 == 0, ab % 2 == 0
    c16 = ldc % 4 == 0 and cb % 4 == 0
    nnk_ok = 1 <= K <= 128 and M >= 4096 and lda >= K and lda % 4 == 0 and a16
    nnk = not trans and not bm and not amap and nnk_ok
    if trans and bm and c.mode != F32 and M <= 128 and _x3_tn_ok(M, N, K, ab, lda, bb, ldb, True, xb, ldx):
        return _x3_tn(M, N, K, True, cb, ldc)
    if c.mode == SPLIT3_ALL or (c.mode == SPLIT3 and ((M if trans else K) >= 256 or nnk)):
        if not trans and not bm and M >= 256 and N % 16 == 0 and lda % 4 == 0 and a16:
            x3_nn = lda >= _cd(K, 32) * 32          # with gemm3_nn_ok: x3_nn_ok
            nn7 = x3_nn and _cd(K, 32) >= 4 and M >= 32768
            if (amap and x3_nn) or (c.mode == SPLIT3_ALL and nn7):
                if nn7 and (epi or c16):
                    return S3B + "k_x3_nn7<RT7,E%d>" % epi
                return S3B + "k_x3_nn<E%d>[%s]" % (epi, "scalar" if epi else "vec" if c16 else "scalar")
            if not amap and nnk_ok:
                return S3B + "k_x3_nnk<E%d>" % epi
            return S3B + "k_gemm3_nn<E%d,MP%d>" % (epi, amap)
        if trans and not epi and M >= 1 and K >= 256 and N % 16 == 0:
            if amap and not bm and _x3_tn_ok(M, N, K, ab, lda, bb, ldb, False, 0, 0):
                return _x3_tn(M, N, K, False, cb, ldc)
            v2 = (ldb % 4 == 0 and bb % 4 == 0 and (not bm or (ldx % 4 == 0 and xb % 4 == 0)) and
                  (not amap or c.mo == 0))
            if v2:
                nmb, nnb, ksteps = _cd(_cd(M, 16), 24), _cd(N, 128), _cd(K, 32)
                splits = max(1, min(256 // (nmb * nnb), ksteps // 4))
                splits = _cd(K, _cd(ksteps, splits) * 32)
                k = "k_s3_tn<TPW3,BM%d,MP%d>" % (bm, amap)
            else:
                nrg, ncb = _cd(M, 160), _cd(N, 128)
                splits = max(1, min(256 // (nrg * ncb), _cd(K, 128)))
                splits = _cd(K, _cd(_cd(K, splits), 32) * 32)
                k = "k_gemm3_tn<BM%d,MP%d>" % (bm, amap)
            return k + ("+" + _sum_splits(splits, N, cb, ldc) if splits > 1 else "")
    if not trans and not bm and M >= 2048 and K >= 1:
        nc = 128 if (K <= 288 and N % 128 == 0) else 64 if (K <= 608 and N % 64 == 0) else 0
        if nc:
            av = 4 if (lda % 4 == 0 and a16) else 2 if (lda % 2 == 0 and a8) else 1
            return WR % (nc, av, epi, "bimg4" if (ldb % 4 == 0 and bb % 4 == 0) else "bimg1", c16)
    if (trans and not epi and (M >= 320 or M <= 128) and N % 128 == 0 and ldb % 4 == 0 and
            bb % 4 == 0 and (not bm or (ldx % 4 == 0 and xb % 4 == 0))):
        rt1 = M <= 128
        nrg, ncb = _cd(M, 128 if rt1 else 640), N // 128
        splits = max(1, min((512 if rt1 else 256) // (nrg * ncb), _cd(K, 64)))
        splits = _cd(K, _cd(_cd(K, splits), 16) * 16)
        av = (4 if (lda % 4 == 0 and lda >= _cd(M, 4) * 4 and a16) else
              2 if (M % 2 == 0 and lda % 2 == 0 and a8) else 1)
        vec = True if splits > 1 else c16      # the partials' slabs are dense and aligned
        k = TB % (bm, av, 1 if rt1 else 5, "vec" if vec else "scalar")
        return k + ("+" + _sum_splits(splits, N, cb, ldc) if splits > 1 else "")
    tiles, ksteps = _cd(M, 64) * _cd(N, 128), _cd(K, 32)
    splits = 1
    if not epi and tiles < 384:
        splits = max(1, min(768 // tiles, ksteps // 4))
    splits = _cd(K, _cd(ksteps, splits) * 32)
    inner = M if trans else K
    av = (4 if (inner % 4 == 0 and lda % 4 == 0 and a16) else
          2 if (inner % 2 == 0 and lda % 2 == 0 and a8) else 1)
    bfull = N % 128 == 0 and ldb % 2 == 0 and bb % 2 == 0
    if bm:
        bfull = bfull and ldx % 2 == 0 and xb % 2 == 0
    k = KG % ("TN" if trans else "NN", av, bfull, epi, bm)
    return k + ("+" + _sum_splits(splits, N, cb, ldc) if splits > 1 else "")


SPLIT_KERNELS = ("k_gemm3_nn", "k_gemm3_tn", "k_s3_tn", "k_x3_")


def on_split_kernel(c: Cell) -> bool:
    return any(k in c.route for k in SPLIT_KERNELS)


def trace_names(route: str):
    """The kernels of a route as rocprofv3's kernel trace names them (the
    demangled template instance, without the namespace and the argument list)."""
    b = {"0": "false", "1": "true"}
    out = []
    for part in route.split("+"):
        part = part.split("[")[0]
        if part in ("memset", "none"):
            continue
        if "<" not in part:
            out.append(part)
            continue
        name, args = part[:-1].split("<")
        a = args.split(",")
        if name == "k_gemm":
            t = ["true" if a[0] == "TN" else "false", a[1][2:], b[a[2][-1]], b[a[3][-1]], b[a[4][-1]]]
        elif name == "k_gemm_wres":
            t = [a[0][2:], a[1][2:], b[a[2][-1]], "2", "true"]
        elif name == "k_gemm_tn_big":
            t = [b[a[0][-1]], a[1][2:], "true", a[3][1:]]
        elif name == "k_sum_splits_tree":
            t = [a[0][1:], a[1][1:]]
        elif name in ("k_gemm3_nn", "k_gemm3_tn"):
            t = [b[a[0][-1]], b[a[1][-1]]]
        elif name == "k_s3_tn":
            t = ["3", b[a[1][-1]], b[a[2][-1]]]
        elif name == "k_x3_tn":
            t = [a[0][3:], a[1][2:], b[a[2][-1]]]
        elif name == "k_x3_nn7":
            t = ["7", b[a[1][-1]]]
        else:  # k_x3_nn<E>, k_x3_nnk<E>
            t = [b[a[0][-1]]]
        out.append("%s<%s>" % (name, ", ".join(t)))
    return out


# ---------------------------------------------------------------------------
# operands, reference and bars

def _seed(c: Cell):
    M, N, K = c.shape
    return 1000003 * M + 1009 * N + K + 7 * (NN_ENTRIES + TN_ENTRIES).index(c.entry)


def values(c: Cell):
    """The cell's operand values (CPU, float32): a function of the entry point
    and the shape only, so the cells of a group multiply the same numbers."""
    M, N, K = c.shape
    g = torch.Generator().manual_seed(_seed(c))
    R = c.table_rows()
    v = {"A": torch.randn(R, c.cols("A"), generator=g),
         "B": torch.randn(K, N, generator=g) + torch.arange(N) * 0.01}
    if c.masked:
        v["X"] = torch.relu(torch.randn(K, N, generator=g))
    if c.mapped:
        n = K if c.trans else M
        v["map"] = (torch.randperm(R, generator=g)[:n] if not c.trans
                    else torch.randint(0, R, (n,), generator=g)).to(torch.int32)
    return v


def build(c: Cell, device):
    """The cell's operands on `device`: {"A": (flat, view), "B": ..., "C": ...,
    ["X": ...], ["map": ...]}, inputs filled with the cell's values."""
    M, N, K = c.shape
    vals = values(c)
    ops = {}
    for op in ("A", "B") + (("X",) if c.masked else ()):
        base, pitch = c.layout(op)
        rows = c.table_rows() if op == "A" else K
        flat, v = view(rows, c.cols(op), base, pitch, device, "in")
        v.copy_(vals[op].to(device))
        ops[op] = (flat, v)
    base, pitch = c.layout("C")
    # (an empty tensor has no pointer to pass: the M == 0 / N == 0 cells get a
    # one-row / one-column C and hand the true sizes to the entry point)
    ops["C"] = view(max(M, 1), max(N, 1), base, pitch, device, "out")
    if c.mapped:
        ops["map"] = rowmap(vals["map"].to(device), c.mo, device)
    return ops


def effective(c: Cell, ops):
    """(A_eff, B_eff): the float32 matrices whose product the call computes —
    A's gathered rows, B under the mask (values exactly representable)."""
    A, B = ops["A"][1], ops["B"][1]
    if c.mapped:
        A = A[ops["map"][1].long()]
    if c.masked:
        B = B * (ops["X"][1] > 0) * MASK_SCALE
    return A, B


def reference(c: Cell, ops):
    """(ref, scale) in float64: op(A) B of the float32 operand values and
    |op(A)| |B| per element."""
    A, B = effective(c, ops)
    A, B = A.double(), B.double()
    if c.trans:
        A = A.t()
    return A @ B, A.abs() @ B.abs() + 1e-30


def keep_mask(c: Cell, device):
    M, N, _ = c.shape
    return torch.from_numpy(_dropout_keep(M, N, DROP_P, DROP_SEED, DROP_OFFSET)).to(device)


def f32_bar(got, ref, K, masked=False, scale=1.0):
    """test_gemm_f32_mfma's bound (test_gemm_tn_masked's for the masked TN;
    test_gemm_relu_dropout_epilogue's atol for the epilogue's 1 / (1 - p))."""
    tol = 2e-6 * max(K, 1) ** 0.5 + 1e-6
    torch.testing.assert_close(got.double(), ref, rtol=tol, atol=tol * (8 if masked else 4) * max(scale, 1))


def split_errs(got32, got3, ref, scale, where=None):
    e32 = (got32.double() - ref).abs() / scale
    es3 = (got3.double() - ref).abs() / scale
    if where is not None:
        e32, es3 = e32[where], es3[where]
    return e32.max().item(), es3.max().item()


def split_bar(e32, es3):
    """test_gemm_split3._check, unchanged."""
    assert es3 <= 1.25 * e32 + 1e-7, (es3, e32)
    assert es3 < 5e-7, es3


def call(ctx, c: Cell, A, B, C, X=None, rows=None):
    M, N, K = c.shape
    if M == 0 or N == 0:  # the wrappers read the sizes off the tensors
        rc = ctx.lib.nts_hip_gemm_f32(ctx.h, int(c.trans), M, N, K, A.data_ptr(), A.stride(0),
                                      B.data_ptr(), B.stride(0), C.data_ptr(), C.stride(0))
        assert rc == 0, rc
    elif c.entry == "gemm":
        ctx.gemm(A, B, C)
    elif c.entry == "gemm_tn":
        ctx.gemm(A, B, C, trans_a=True)
    elif c.entry == "gather":
        ctx.gemm_gather(A, rows, B, C)
    elif c.entry == "tn_gather":
        ctx.gemm_tn_gather(A, rows, B, C)
    elif c.entry == "relu_dropout":
        ctx.gemm_relu_dropout(A, B, C, p=DROP_P, seed=DROP_SEED, offset=DROP_OFFSET)
    else:
        ctx.gemm_tn_masked(A, B, X, C, scale=MASK_SCALE)
