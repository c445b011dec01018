"""A synthetic CSC block with its CSR transpose for the sum-aggregation kernels
(csrc/aggregate.hip), the launch cell a width and a layout reach, and the
references of every mode on that block.

The sampler's blocks (fanout <= 25, dense 16-byte aligned operands) leave most
of `launch_gather`'s specialisations unrun.  `make_block` builds the smallest
block that crosses every row-length boundary on both sides:

* 96 destinations, 320 sources, `dst_local_id` injective (the root pair);
* the column degrees AND the CSR row lengths each hold SPECIAL_DEGREES: 0, the
  values one below, at and one above U and 4 U for the gather's unroll U in
  {4, 5, 8} (`gather_u`; a CSR row of more than kLongRow(U) = 4 U edges is
  summed in pieces by the whole block), 65 (two 64-edge id batches at 64-lane
  groups) and one row of 200;
* the other columns get a random 1..11 edges; the other CSR rows a random
  1..11 each until the block's edges are used up, the rest stay empty;
* CSR rows 4..7 are all long (33, 34, 65 and 200 edges): at every lane-group
  width these four consecutive rows fall into one block, so every lane group
  of a 64-lane block enters a row into the block's long-row list.  More than
  kCoopRows long rows in ONE lane group's share cannot be built: the grid
  gives every lane group exactly one row until the row count passes
  kGatherGridCap blocks (2^26 rows at 64 lanes), and 17 rows a group would
  need 17 times that;
* edge weights random with both signs (cancellation); the backward weights
  are the same weights in CSR order, so the CSR and the atomic CSC backward
  share one reference.  Every kernel is also run with a NULL weight array.

References.  `agg64` is the header's definition, one row at a time in float64,
with the float64 sum of |w x| beside it for the error bound
|err| <= 2 (n + k) 2^-24 sum|w x| (n edges, k further roundings of the mode).
`agg32` is the serial edge order in fp32, (x * w) + acc from 0 with no
contraction — the order every CSC column and every short CSR row promises bit
for bit.  `agg32_pieces` is a long CSR row's documented order: the block's GPB
lane groups each sum a contiguous GPB-th of the edges in order from 0, and the
partial sums are added in group order.

`cell` restates agg_shape.hpp (row_vec, pick_shape, gather_u, kLongRow) so that
a test can name the (vec, LPD, NCH, last_valid) cell a width and a layout reach.
"""
import numpy as np

V_DST, N_SRC, N_TABLE = 96, 320, 401
SPECIAL_DEGREES = (0, 1, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 20, 21, 32, 33, 65, 200)
LONG_BLOCK = {4: 33, 5: 34, 6: 65, 7: 200}  # CSR row -> length: one block of long rows
K_AGG_THREADS = 256
K_COOP_ROWS = 16
NOT_CACHED = 0xFFFFFFFF


# ---- agg_shape.hpp restated ---------------------------------------------------
def row_vec(F, ops, pad=False):
    """ops: (base offset in floats from a 16-byte aligned address, pitch in
    floats) of every operand present."""
    def fits(cols, vec):
        return cols % vec == 0 and all(cols <= ld and ld % vec == 0 and off % vec == 0
                                       for off, ld in ops)
    if pad and fits((F + 3) // 4 * 4, 4):
        return 4
    return 4 if fits(F, 4) else 2 if fits(F, 2) else 1


def pick_shape(nv):
    for lpd in (8, 16, 32, 64):
        if nv <= lpd:
            return lpd, 1
    return 64, min((nv + 63) // 64, 8)


def gather_u(floats_per_lane):
    return 8 if floats_per_lane <= 4 else 5 if floats_per_lane <= 12 else 4


def k_long_row(u):
    return 4 * u


def cell(F, ops, pad=False, root_bwd_ops=None):
    """The launch cell of launch_gather: dict(vec, nv, last_valid, lpd, nch,
    rounds, u, long_row, gpb).  root_bwd_ops: (g_ycat, g_in) of the root
    backward, which takes the shape and the long-row rule of the plain CSR
    backward on those two operands."""
    vec = row_vec(F, ops, pad)
    nv = (F + vec - 1) // vec
    lpd, nch = pick_shape(nv)
    u = gather_u(vec * nch)
    long_row = k_long_row(u)
    if root_bwd_ops is not None:
        plain = row_vec(F, root_bwd_ops, True)
        lpd, nch = pick_shape((F + plain - 1) // plain)
        long_row = k_long_row(gather_u(plain * nch))
        u = gather_u(vec * nch)
    return dict(vec=vec, nv=nv, last_valid=F - (nv - 1) * vec, lpd=lpd, nch=nch,
                rounds=(nv + lpd * nch - 1) // (lpd * nch), u=u, long_row=long_row,
                gpb=K_AGG_THREADS // lpd)


# ---- the block ------------------------------------------------------------------
def make_block(seed=0):
    """dict of numpy arrays: column_offset [v+1], row_indices [e], weight [e],
    dst_local_id [v], src_dst [s] (its inverse, NOT_CACHED elsewhere), row_offset
    [s+1], column_indices [e], csr_edge_id [e], weight_backward [e], src_map [s]
    (injective into a table of N_TABLE rows), and v, s, e."""
    rng = np.random.default_rng(seed)
    v, s = V_DST, N_SRC
    deg = np.concatenate([np.array(SPECIAL_DEGREES, np.int64),
                          rng.integers(1, 12, v - len(SPECIAL_DEGREES))])
    rng.shuffle(deg)
    e = int(deg.sum())
    # CSR row lengths: the long block, the other special lengths on random rows,
    # then 1..11 a row while edges last
    rl = np.zeros(s, np.int64)
    for r, n in LONG_BLOCK.items():
        rl[r] = n
    rest = [n for n in SPECIAL_DEGREES if n not in (33, 65, 200)]
    free = rng.permutation(np.setdiff1d(np.arange(s), list(LONG_BLOCK)))
    rl[free[:len(rest)]] = rest
    left = e - int(rl.sum())
    assert left > 0
    for r in free[len(rest):]:
        n = min(int(rng.integers(1, 12)), left)
        rl[r] = n
        left -= n
        if left == 0:
            break
    assert left == 0
    ri = rng.permutation(np.repeat(np.arange(s), rl))
    co = np.zeros(v + 1, np.int64)
    co[1:] = np.cumsum(deg)
    d_of_e = np.repeat(np.arange(v), deg)
    order = np.argsort(ri, kind="stable")
    ro = np.zeros(s + 1, np.int64)
    ro[1:] = np.cumsum(np.bincount(ri, minlength=s))
    w = rng.standard_normal(e).astype(np.float32)
    dl = rng.permutation(s)[:v]
    src_dst = np.full(s, NOT_CACHED, np.int64)
    src_dst[dl] = np.arange(v)
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
    return dict(v=v, s=s, e=e, column_offset=u32(co), row_indices=u32(ri), weight=w,
                dst_local_id=u32(dl), src_dst=u32(src_dst), row_offset=u32(ro),
                column_indices=u32(d_of_e[order]), csr_edge_id=u32(order),
                weight_backward=np.ascontiguousarray(w[order]),
                src_map=u32(rng.permutation(N_TABLE)[:s]))


# ---- references -----------------------------------------------------------------
def _w(w, n):
    return np.ones(n, np.float32) if w is None else w


def agg64(off, idx, w, X, n=None):
    """(S, A): S[r] = sum_e w[e] X[idx[e]] and A[r] = sum_e |w[e] X[idx[e]]| over
    e in [off[r], off[r+1]), float64, for the first n rows."""
    n = len(off) - 1 if n is None else n
    w = _w(w, len(idx)).astype(np.float64)
    X = np.asarray(X, np.float64)
    S = np.zeros((n, X.shape[1]))
    A = np.zeros((n, X.shape[1]))
    for r in range(n):
        b, e = int(off[r]), int(off[r + 1])
        if b == e:
            continue
        t = w[b:e, None] * X[idx[b:e].astype(np.int64)]
        S[r] = t.sum(0)
        A[r] = np.abs(t).sum(0)
    return S, A


def _serial32(b, e, idx, w, X):
    acc = np.zeros(X.shape[1], np.float32)
    for j in range(b, e):
        acc = X[idx[j]] * w[j] + acc
    return acc


def agg32(off, idx, w, X, n=None):
    """The serial edge order in fp32: acc = (x * w) + acc from 0."""
    n = len(off) - 1 if n is None else n
    w = _w(w, len(idx))
    X = np.asarray(X, np.float32)
    Y = np.zeros((n, X.shape[1]), np.float32)
    for r in range(n):
        Y[r] = _serial32(int(off[r]), int(off[r + 1]), idx, w, X)
    return Y


def agg32_pieces(off, idx, w, X, long_row, gpb, n=None):
    """agg32 with the CSR backward's long-row rule: a row of more than long_row
    edges is the sum, in group order, of gpb in-order pieces."""
    n = len(off) - 1 if n is None else n
    w = _w(w, len(idx))
    X = np.asarray(X, np.float32)
    Y = np.zeros((n, X.shape[1]), np.float32)
    for r in range(n):
        b, e = int(off[r]), int(off[r + 1])
        ln = e - b
        if ln <= long_row:
            Y[r] = _serial32(b, e, idx, w, X)
            continue
        acc = None
        for g in range(gpb):
            p = _serial32(b + ln * g // gpb, b + ln * (g + 1) // gpb, idx, w, X)
            acc = p if acc is None else acc + p
        Y[r] = acc
    return Y


def err_bound(A, n_edges, k):
    """2 (n + k) 2^-24 A per element; n_edges [rows]."""
    return 2.0 * (np.asarray(n_edges, np.float64)[:, None] + k) * 2.0 ** -24 * A


def act_mask(x_act, scale):
    """[x_act > 0] * scale in fp32"""
    return np.where(np.asarray(x_act) > 0, np.float32(scale), np.float32(0)).astype(np.float32)


# ---- widths, layouts and the cell each reaches ----------------------------------
# The issue's widths, then one width per (vec, LPD, NCH) cell they leave out
# (the same F gives the float4 / float2 / scalar cell by layout):
#   20: scalar (32, 1); 196: scalar (64, 4); 324: scalar (64, 6);
#   388: float2 (64, 4), scalar (64, 7); 644: float4 (64, 3), float2 (64, 6);
#   772: float4 (64, 4), float2 (64, 7); 1028 / 1284 / 1540: float4 (64, 5 / 6 / 7)
#   for the modes without the pad path; 263: pad with last_valid 3 on two chunks;
#   2048: float4 (64, 8) in one round, the widest row the mask bits take.
WIDTHS = (1, 3, 6, 10, 12, 20, 36, 68, 132, 196, 260, 263, 324, 388, 513, 602, 644, 772, 1028,
          1284, 1433, 1540, 2048, 2052)


def pitch(rule, width):
    if rule == "dense":
        return width
    if rule == "pad32":
        return (width + 31) // 32 * 32
    return width + {"+1": 1, "+2": 2}[rule]


# id: (input, output, mask operand), each (pitch rule, base offset in floats)
_D, _P = ("dense", 0), ("pad32", 0)
LAYOUTS = {
    "dense": (_D, _D, _D),
    "pad32": (_P, _P, _P),
    "pitch+1": (("+1", 0),) * 3,
    "pitch+2": (("+2", 0),) * 3,
    "base+1": (("pad32", 1),) * 3,
    "base+2": (("pad32", 2),) * 3,
    "in0-out1": (_P, ("pad32", 1), _P),
    "in1-out0": (("pad32", 1), _P, ("pad32", 1)),
    "mask1": (_P, _P, ("pad32", 1)),  # modes with a mask operand only
}
# entry point -> (operands of row_vec among in/out/mask, pad path, has mask operand)
CSC_ENTRIES = ("fwd", "fwd_map", "fwd_act_p0", "fwd_act_p5", "fwd_root", "fwd_root_map",
               "fwd_act_bits", "fwd_cached")
CSR_ENTRIES = ("csr_bwd", "csr_bwd_masked", "csr_bwd_postmask", "csr_bwd_root",
               "csr_bwd_root_act", "csr_bwd_postmask_bits", "csr_bwd_colmax")
FLAT_ENTRIES = ("bwd_atomic", "gather_rows", "act_backward")
ENTRIES = CSC_ENTRIES + CSR_ENTRIES + FLAT_ENTRIES
_PAD = ("fwd", "fwd_map", "fwd_cached", "csr_bwd", "csr_bwd_colmax")
_MASKED = ("csr_bwd_masked", "csr_bwd_postmask", "csr_bwd_root_act", "act_backward")
_IN_2F = ("csr_bwd_root", "csr_bwd_root_act")
_OUT_2F = ("fwd_root", "fwd_root_map")


def act_bits_words(F):
    if F == 0 or F % 4:
        return 0
    lpd, nch = pick_shape(F // 4)
    return 0 if lpd < 32 or F // 4 > lpd * nch else lpd // 32 * nch * 4


def layouts_of(entry):
    """the layouts an entry point is run on"""
    if entry == "fwd_cached":
        return ("dense", "pad32")
    return tuple(k for k in LAYOUTS if k != "mask1" or entry in _MASKED)


def entry_ops(entry, F, layout):
    (ri, oi), (ro, oo), (rm, om) = LAYOUTS[layout]
    ops = [(oi, pitch(ri, 2 * F if entry in _IN_2F else F)),
           (oo, pitch(ro, 2 * F if entry in _OUT_2F else F))]
    if entry in _MASKED:
        ops.append((om, pitch(rm, F)))
    if entry == "fwd_cached":
        ops.append((0, pitch(ri, F)))  # the host table: the input's pitch
    return ops


def entry_cell(entry, F, layout):
    """The cell of `cell`, or None where the entry point refuses the width or
    the layout (the bits pair, the column maxima); FLAT_ENTRIES: vec and lpd only."""
    ops = entry_ops(entry, F, layout)
    if entry in FLAT_ENTRIES:
        if entry == "act_backward":
            flat = all(off == 0 and ld == F for off, ld in ops) and (V_DST * F) % 4 == 0
            return dict(vec=4 if flat else 1, lpd=0, nch=0, last_valid=0, rounds=1)
        vec = row_vec(F, ops)
        nv = F // vec
        return dict(vec=vec, lpd=16 if nv <= 16 else 32 if nv <= 32 else 64, nch=0,
                    last_valid=vec, rounds=1)
    c = cell(F, ops, entry in _PAD, root_bwd_ops=ops[:2] if entry in _IN_2F else None)
    if entry == "csr_bwd_colmax" and (F > 512 or c["vec"] != 4):
        return None
    if entry in ("fwd_act_bits", "csr_bwd_postmask_bits") and (
            act_bits_words(F) == 0 or c["vec"] != 4):
        return None
    return c


def cell_table(entries=ENTRIES, widths=WIDTHS):
    """{(entry, (vec, lpd, nch, last_valid, rounds)): [(F, layout), ...]}"""
    out = {}
    for en in entries:
        for F in widths:
            for lay in layouts_of(en):
                c = entry_cell(en, F, lay)
                if c is not None:
                    key = (en, (c["vec"], c["lpd"], c["nch"], c["last_valid"], c["rounds"]))
                    out.setdefault(key, []).append((F, lay))
    return out


def format_cell_table(entries=ENTRIES, widths=WIDTHS):
    """one line per (vec, LPD, NCH, last_valid, c0 rounds) cell: the entry points
    that reach it and one (F, layout) that does"""
    by_cell = {}
    for (en, key), hits in cell_table(entries, widths).items():
        by_cell.setdefault(key, []).append((en, hits[0]))
    lines = ["vec LPD NCH last rounds | entry points (first F:layout)"]
    for key in sorted(by_cell):
        who = ", ".join(f"{en} ({F}:{lay})" for en, (F, lay) in by_cell[key])
        lines.append("%3d %3d %3d %4d %6d | %s" % (*key, who))
    return "\n".join(lines)
