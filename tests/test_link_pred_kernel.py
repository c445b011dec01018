"""nts_hip_lp_batch and nts_hip_lp_bce_fwd / _train (csrc/linkpred.hip, DESIGN
§8t) against tests/linkpred_ref.py.

nts_hip_lp_batch: every output bit for bit (destination, v_size, pair_u,
pair_v, inc_offset over the live rows + the end offset, inc_slot).

Loss entries, on the same pair sets, D in {1, 3, 4, 64, 130, 1024}, ldh > D:
the bounds of tests/test_multilabel_kernel.py for the fused BCE (loss rtol =
atol = 1e-5; gradient rtol 1e-4, atol 1e-6) against float64.  H is drawn
N(0, 3 / sqrt(D)), so a score of two distinct rows has a standard deviation of
about 3, and is scaled down as a whole where a score (a self pair's |h|^2 at a
large D) would pass 20: max |score| <= 20 is asserted on the float64 reference
before any kernel runs.  Every case runs at a row pitch above D with NaN in the
pad, on the 16-byte path where D % 4 == 0 and on the scalar path elsewhere.
"""
import numpy as np
import pytest
import torch

import linkpred_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEED = 2000
NTS_ERR_INVALID = 1
POISON = 0x7FC0DEAD  # a NaN pattern as int32, unlikely as an id


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=SEED)


def _positives(name, rng):
    """V, heads, tails, K, batch_seq"""
    if name == "v64":  # repeated endpoints
        return 64, np.array([3, 3, 10, 63, 10]), np.array([10, 4, 3, 0, 63]), 3, 7
    if name == "v3":  # collisions and self pairs certain
        return 3, np.array([0, 1, 2, 1]), np.array([1, 1, 0, 2]), 4, 1
    if name == "b1":
        return 50, np.array([7]), np.array([9]), 1, 0
    if name == "hub":  # 40 positives sharing one head: 200 slots on its row
        return 5000, np.full(40, 17), np.arange(100, 140), 4, 3
    if name == "k5":  # crosses a Philox block of 4 words; a batch_seq past 2^32
        return 300, rng.integers(0, 300, 20), rng.integers(0, 300, 20), 5, (1 << 40) + 2
    if name == "v100003":  # a non-power-of-two multiply-shift
        return 100003, rng.integers(0, 100003, 33), rng.integers(0, 100003, 33), 2, 12345
    raise KeyError(name)


CASES = ["v64", "v3", "b1", "hub", "k5", "v100003"]
_cache = {}


def _case(name):
    if name not in _cache:
        V, ps, pd, K, seq = _positives(name, np.random.default_rng(CASES.index(name)))
        b = ref.batch(ps, pd, K, V, SEED, seq)
        b.update(V=V, seq=seq, ps=np.asarray(ps, np.uint32), pd=np.asarray(pd, np.uint32))
        _cache[name] = b
    return _cache[name]


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def _run_batch(hip, b, v_cap=None):
    P = b["P"]
    v_cap = 2 * P if v_cap is None else v_cap
    out = {k: torch.full((n,), POISON, dtype=torch.int32, device=DEV)
           for k, n in (("destination", v_cap), ("v_size", 1), ("pair_u", P), ("pair_v", P),
                        ("inc_offset", v_cap + 1), ("inc_slot", 2 * P))}
    hip.reserve(b["V"], 8 * P)
    hip.lp_batch(_i32(b["ps"]), _i32(b["pd"]), b["K"], b["V"], b["seq"], out["destination"],
                 out["v_size"], out["pair_u"], out["pair_v"], out["inc_offset"], out["inc_slot"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().view(np.uint32) for k, v in out.items()}


def test_reference_cases_hold_what_they_are_for():
    b = _case("v3")
    assert (b["pair_u"] == b["pair_v"]).any(), "the V = 3 case must contain a self pair"
    assert b["v_size"] <= 3 < 2 * b["P"]
    h = _case("hub")
    assert np.diff(h["inc_offset"].astype(np.int64)).max() >= 200
    assert _case("k5")["K"] == 5 and _case("b1")["P"] == 2


@pytest.mark.parametrize("name", CASES)
def test_lp_batch_equals_the_reference_bit_for_bit(hip, name):
    b = _case(name)
    got = _run_batch(hip, b)
    v, P = b["v_size"], b["P"]
    assert int(got["v_size"][0]) == v
    assert np.array_equal(got["destination"][:v], b["destination"])
    assert (got["destination"][v:] == np.uint32(POISON)).all(), "entries past v_size were written"
    assert np.array_equal(got["pair_u"], b["pair_u"]) and np.array_equal(got["pair_v"], b["pair_v"])
    assert np.array_equal(got["inc_offset"][:v + 1], b["inc_offset"])
    assert (got["inc_offset"][v:] == 2 * P).all(), "rows past v_size must be empty"
    assert np.array_equal(got["inc_slot"], b["inc_slot"])


def test_lp_batch_refusals_leave_the_outputs_untouched(hip):
    from nts import _abi
    from nts._abi import ptr
    b = _case("v64")
    P = b["P"]
    ps, pd = _i32(b["ps"]), _i32(b["pd"])
    bufs = [torch.full((n,), POISON, dtype=torch.int32, device=DEV)
            for n in (2 * P, 1, P, P, 2 * P + 1, 2 * P)]

    def call(src=ps, dst=pd, B=b["B"], K=b["K"], v_cap=2 * P, drop=None):
        out = [ptr(t) for t in bufs]
        if drop is not None:
            out[drop] = None
        return hip.lib.nts_hip_lp_batch(hip.h, ptr(src), ptr(dst), B, K, b["V"], 0, v_cap, *out)

    assert call(K=0) == NTS_ERR_INVALID
    assert call(B=0) == NTS_ERR_INVALID
    assert call(v_cap=2 * P - 1) == NTS_ERR_INVALID
    assert call(src=None) == NTS_ERR_INVALID and call(dst=None) == NTS_ERR_INVALID
    for i in range(len(bufs)):
        assert call(drop=i) == NTS_ERR_INVALID
    assert b"invalid argument" in _abi.lib().nts_hip_last_error()
    torch.cuda.synchronize()
    for t in bufs:
        assert (t == POISON).all()


# ---- loss entries ----------------------------------------------------------
DS = [1, 3, 4, 64, 130, 1024]


def _embedding(b, D, seed):
    rng = np.random.default_rng([D, seed])
    H = (rng.standard_normal((b["v_size"], D)) * np.sqrt(3.0 / np.sqrt(D))).astype(np.float32)
    s = np.abs(ref.scores(H, b["pair_u"], b["pair_v"])).max()
    if s > 20.0:
        H = (H * np.float32(np.sqrt(19.0 / s))).astype(np.float32)
    assert np.abs(ref.scores(H, b["pair_u"], b["pair_v"])).max() <= 20.0
    return H


def _device_pairs(b, v_cap):
    off = np.full(v_cap + 1, 2 * b["P"], np.uint32)
    off[:b["v_size"] + 1] = b["inc_offset"]
    return dict(pair_u=_i32(b["pair_u"]), pair_v=_i32(b["pair_v"]), inc_offset=_i32(off),
                inc_slot=_i32(b["inc_slot"]), v_size=_i32([b["v_size"]]))


def _padded(H, pad):
    """H on the device at a pitch of D + pad floats, NaN in the pad"""
    n, D = H.shape
    buf = torch.full((n, D + pad), float("nan"), device=DEV)
    view = buf[:, :D]
    view.copy_(torch.from_numpy(H))
    return view


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("name", CASES)
def test_lp_bce_matches_float64(hip, name, D):
    b = _case(name)
    v, P, B, K = b["v_size"], b["P"], b["B"], b["K"]
    H = _embedding(b, D, CASES.index(name))
    s64, loss64, dH64 = ref.loss_and_grad(H, b)
    extra = 3  # rows past v_size: must keep the poison
    dp = _device_pairs(b, v + extra)
    # pitch D + 4 keeps 16-byte rows where D % 4 == 0 (the vector path), D + 3 elsewhere
    Hd = _padded(np.concatenate([H, np.zeros((extra, D), np.float32)]), 4 if D % 4 == 0 else 3)
    hip.reserve(b["V"], 8 * P)

    score_f = torch.empty(P, device=DEV)
    loss_f = torch.empty((), device=DEV)
    hip.lp_bce_fwd(Hd, D, dp["pair_u"], dp["pair_v"], B, K, score_f, loss_f, None)  # NULL counter

    runs = []
    for _ in range(2):
        score = torch.empty(P, device=DEV)
        loss = torch.empty((), device=DEV)
        dH = torch.full((v + extra, D + 4), 12345.0, device=DEV)[:, :D]
        hip.lp_bce_train(Hd, D, dp["pair_u"], dp["pair_v"], B, K, dp["inc_offset"], dp["inc_slot"],
                         dp["v_size"], score, loss, dH, None)
        torch.cuda.synchronize()
        runs.append((score.cpu().numpy(), float(loss), dH.cpu().numpy().copy()))
    (sc, ls, g), (sc2, ls2, g2) = runs
    print(f"{name} D={D}: loss {ls:.7f} ref {loss64:.7f}; max |dH - ref| "
          f"{np.abs(g[:v] - dH64).max():.3e}; max |score - ref| {np.abs(sc - s64).max():.3e}")
    np.testing.assert_allclose(ls, loss64, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(float(loss_f), loss64, rtol=1e-5, atol=1e-5)
    assert float(loss_f) == ls and np.array_equal(score_f.cpu().numpy(), sc), "fwd != train"
    np.testing.assert_allclose(sc, s64, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(g[:v], dH64, rtol=1e-4, atol=1e-6)
    assert np.array_equal(g.view(np.uint32), g2.view(np.uint32)) and ls == ls2, "two runs differ"
    assert (g[v:] == 12345.0).all(), "rows >= v_size of dH were written"


@pytest.mark.parametrize("name,D", [("v3", 4), ("hub", 3), ("k5", 1), ("v100003", 64), ("v64", 130)])
def test_mrr_counter_is_exact_on_integer_embeddings(hip, name, D):
    b = _case(name)
    v, P, B, K = b["v_size"], b["P"], b["B"], b["K"]
    rng = np.random.default_rng([7, D])
    H = rng.integers(-2, 3, (v, D)).astype(np.float32)  # scores exact in fp32, ties plenty
    s = ref.scores(H, b["pair_u"], b["pair_v"])
    assert np.abs(s).max() < 2 ** 20
    rk = ref.ranks(s, B, K)
    if D <= 4:
        assert (s[B:].reshape(B, K) == s[:B, None]).any(), "the case is meant to hold ties"
    dp = _device_pairs(b, v)
    Hd = _padded(H, 4 if D % 4 == 0 else 3)
    counter = torch.tensor([0.5, 3.0], device=DEV)  # accumulated into, not overwritten
    score = torch.empty(P, device=DEV)
    loss = torch.empty((), device=DEV)
    hip.reserve(b["V"], 8 * P)
    hip.lp_bce_fwd(Hd, D, dp["pair_u"], dp["pair_v"], B, K, score, loss, counter)
    torch.cuda.synchronize()
    assert np.array_equal(score.cpu().numpy().astype(np.float64), s)
    got = counter.cpu().numpy()
    want = np.float32(np.float32(0.5) + ref.mrr_counter(s, B, K))
    print(f"{name}: ranks {np.bincount(rk)} sum 1/rank {got[0] - 0.5:.7f}")
    assert got[0] == want and got[1] == 3.0 + B
    # the training entry keeps the same counter
    counter2 = torch.tensor([0.5, 3.0], device=DEV)
    dH = torch.empty(v, D, device=DEV)
    hip.lp_bce_train(Hd, D, dp["pair_u"], dp["pair_v"], B, K, dp["inc_offset"], dp["inc_slot"],
                     dp["v_size"], score, loss, dH, counter2)
    torch.cuda.synchronize()
    assert np.array_equal(counter2.cpu().numpy(), got)


def test_lp_bce_refusals_leave_the_outputs_untouched(hip):
    from nts._abi import ptr
    b = _case("v64")
    v, P, B, K = b["v_size"], b["P"], b["B"], b["K"]
    D = 8
    dp = _device_pairs(b, v)
    H = torch.zeros(v, D, device=DEV)
    score = torch.full((P,), 7.0, device=DEV)
    loss = torch.full((), 7.0, device=DEV)
    dH = torch.full((v, D), 7.0, device=DEV)
    L = hip.lib

    def fwd(H_=H, ldh=D, D_=D, u=dp["pair_u"], B_=B, K_=K, sc=score, ls=loss):
        return L.nts_hip_lp_bce_fwd(hip.h, ptr(H_), ldh, D_, ptr(u), ptr(dp["pair_v"]), B_, K_,
                                    ptr(sc), ptr(ls), None)

    def train(D_=D, lddh=D, off=dp["inc_offset"], g=dH, B_=B):
        return L.nts_hip_lp_bce_train(hip.h, ptr(H), D, D_, ptr(dp["pair_u"]), ptr(dp["pair_v"]),
                                      B_, K, ptr(off), ptr(dp["inc_slot"]), ptr(dp["v_size"]), v,
                                      ptr(score), ptr(loss), ptr(g), lddh, None)

    for rc in (fwd(H_=None), fwd(u=None), fwd(sc=None), fwd(ls=None), fwd(D_=0), fwd(D_=1025, ldh=1025),
               fwd(ldh=D - 1), fwd(B_=0), fwd(K_=0), train(D_=0), train(lddh=D - 1), train(off=None),
               train(g=None), train(B_=0)):
        assert rc == NTS_ERR_INVALID
    torch.cuda.synchronize()
    assert (score == 7.0).all() and float(loss) == 7.0 and (dH == 7.0).all()
