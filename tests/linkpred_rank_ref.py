"""All-candidate ranking in numpy / float64: the counts
nts_hip_lp_rank returns, the band an fp32 kernel may move inside, and the
metrics evaluate_full() forms from the counts.

adj: None (unfiltered) or (goff, srows): the graph's column_offset [V + 1] and
its row_indices sorted ascending within each destination's segment, the two
arrays nts_hip_lp_batch_filtered takes."""
import numpy as np

U24 = 2.0 ** -24  # fp32 unit roundoff


def sorted_adj(V, src, dst):
    """(goff, srows) of the edge list src -> dst"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    order = np.lexsort((src, dst))
    goff = np.zeros(V + 1, np.uint64)
    goff[1:] = np.cumsum(np.bincount(dst, minlength=V))
    return goff, src[order].astype(np.uint32)


def blocked(adj, u, w):
    """nts_hip_lp_batch_filtered's test: w == u, or the graph holds u -> w or w -> u"""
    goff, srows = adj
    if w == u:
        return True
    seg_w = srows[int(goff[w]):int(goff[w + 1])]
    seg_u = srows[int(goff[u]):int(goff[u + 1])]
    return bool((seg_w == u).any() or (seg_u == w).any())


def _cand(H, cand):
    return np.arange(H.shape[0], dtype=np.int64) if cand is None else np.asarray(cand, np.int64)


def valid_mask(n_rows, heads, tails, cand, adj):
    """[M, n_cand] bool: candidate j is valid for query i"""
    c = np.arange(n_rows, dtype=np.int64) if cand is None else np.asarray(cand, np.int64)
    heads, tails = np.asarray(heads, np.int64), np.asarray(tails, np.int64)
    ok = c[None, :] != tails[:, None]
    if adj is not None:  # blocked() for every pair at once, from a dense adjacency
        goff, srows = adj
        A = np.zeros((n_rows, n_rows), bool)  # A[s, d]: the graph holds s -> d
        A[srows.astype(np.int64), np.repeat(np.arange(n_rows), np.diff(goff.astype(np.int64)))] = True
        blk = A | A.T | np.eye(n_rows, dtype=bool)
        ok &= ~blk[heads[:, None], c[None, :]]
    return ok


def scores64(H, heads, tails, cand):
    """(s [M, n_cand], s_pos [M]) in float64"""
    H64 = np.asarray(H, np.float64)
    c = _cand(H, cand)
    hu = H64[np.asarray(heads, np.int64)]
    return hu @ H64[c].T, (hu * H64[np.asarray(tails, np.int64)]).sum(1)


def counts(H, heads, tails, cand, adj):
    """greater / equal / n_valid (int64 [M]) with exact (float64) scores: the
    kernel's answer wherever every fp32 partial sum is exact"""
    s, sp = scores64(H, heads, tails, cand)
    ok = valid_mask(H.shape[0], heads, tails, cand, adj)
    return ((ok & (s > sp[:, None])).sum(1), (ok & (s == sp[:, None])).sum(1), ok.sum(1))


def gamma(D):
    return D * U24 / (1.0 - D * U24)


def bands(H, heads, tails, cand, adj):
    """For fp32 H: band(a, b) = 2 gamma_D sum_k |a_k b_k| bounds (twice over)
    the error of any fp32 dot product.  Candidate w of query (u, v) is
    AMBIGUOUS when |s64(u, w) - s64(u, v)| <= band(u, w) + band(u, v).  Returns
    (greater_lo, greater_hi, ge_lo, ge_hi, n_valid, n_ambiguous): the valid
    candidates certainly above / possibly above, certainly / possibly at least
    equal (the bounds of greater + equal), and the ambiguous count."""
    H64 = np.abs(np.asarray(H, np.float64))
    D = H64.shape[1]
    c = _cand(H, cand)
    s, sp = scores64(H, heads, tails, cand)
    au = H64[np.asarray(heads, np.int64)]
    band = 2.0 * gamma(D) * (au @ H64[c].T)
    band_pos = 2.0 * gamma(D) * (au * H64[np.asarray(tails, np.int64)]).sum(1)
    ok = valid_mask(H.shape[0], heads, tails, cand, adj)
    diff = s - sp[:, None]
    amb = np.abs(diff) <= band + band_pos[:, None]
    sure_gt = ok & ~amb & (diff > 0)
    maybe = ok & amb
    lo, hi = sure_gt.sum(1), (sure_gt | maybe).sum(1)
    return lo, hi, lo, hi, ok.sum(1), int(maybe.sum())


def metrics(greater, equal, ks=(1, 10, 50)):
    """evaluate_full()'s dict from the count arrays: rank = 1 + greater + equal
    (ties count against the positive), the optimistic rank 1 + greater"""
    g, e = np.asarray(greater, np.float64), np.asarray(equal, np.float64)
    rank, opt = 1.0 + g + e, 1.0 + g
    out = {"mrr": float((1.0 / rank).mean()), "mrr_optimistic": float((1.0 / opt).mean()),
           "mean_rank": float(rank.mean())}
    for k in ks:
        out[f"hits@{k}"] = float((rank <= k).mean())
    out["n"] = int(g.size)
    out["ties"] = int(np.asarray(equal, np.int64).sum())
    return out
