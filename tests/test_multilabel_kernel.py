"""nts_hip_linear_bce_fwd / _train (csrc/top.hip): the multi-label output layer
fused with the mean sigmoid binary cross-entropy and the micro-F1 counters.

Reference: the same chain in torch float64 on the CPU with autograd,
binary_cross_entropy_with_logits(Y W, T) (mean) and its backward.

Bounds: the project's own for the fused xent layer (tests/test_hip_kernels.py,
test_linear_xent_fused): loss rtol = atol = 1e-5; dY, dW rtol 1e-4, atol 1e-6.

Counters: the kernel's logits are fp32, so an entry whose float64 logit is
within 1e-4 of zero may be predicted either way; tp, fp and fn must lie
between the reference counts with those entries all resolved one way and all
the other.  Such entries are first asserted to be at most 0.1 % of n C (for
N(0,1) logits about 0.008 % are expected).

Inputs: Y ~ N(0,1), W ~ N(0,1)/sqrt(K), so the logits are about N(0,1).  Every
case runs twice: dense Y without an index, and Y at a pitch of K + 3 floats
(the scalar staging path) with NaN pad floats, read through an index with
repeated ids that are not rows 0..n-1.  Bits >= C of the last label word are
set to 1 in every table.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
AMBIG = 1e-4
NTS_ERR_INVALID = 1


def max_k(C):
    """largest K the kernel takes at C labels: W [K x Cp], 16 Y
    rows at pitch K + 4, 5 x 16 logit rows and 16 words within 160 KB of LDS"""
    Cp = (C + 15) // 16 * 16
    return (160 * 1024 // 4 - 16 - 80 * Cp - 64) // (Cp + 16) // 16 * 16


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=2000)


def _pack(T):
    """uint8 [V, C] -> int32 [V, wpr] with the bits >= C of the last word set"""
    from nts import dataloader
    C = T.shape[1]
    bits = dataloader.pack_label_bits(T)
    if C % 32:
        bits[:, -1] |= np.uint32((0xFFFFFFFF << (C % 32)) & 0xFFFFFFFF)
    return torch.from_numpy(bits.view(np.int32)).to(DEV)


def _case(n, K, C, indexed, w_scale=1.0):
    # at a handful of entries (n C = 121) one logit within 1e-4 of zero already
    # exceeds the 0.1 % cap on the reference: such a draw is replaced by the
    # next one (judged on the float64 logits alone, before any kernel runs)
    for draw in range(8):
        rng = np.random.default_rng([n, K, C, int(indexed), draw])
        Y = rng.standard_normal((n, K)).astype(np.float32)
        W = (rng.standard_normal((K, C)) / np.sqrt(K) * w_scale).astype(np.float32)
        if (np.abs(Y.astype(np.float64) @ W.astype(np.float64)) < AMBIG).sum() <= 1e-3 * n * C:
            break
    if indexed:
        V = n + 37
        idx = rng.integers(0, V, n).astype(np.int32)
        idx[0] = V - 1  # not row 0
        if n > 1:
            idx[1] = idx[0]  # a repeated id
    else:
        V, idx = n, None
    T = rng.integers(0, 2, (V, C)).astype(np.uint8)
    Yd = torch.full((n, K + 3 if indexed else K), float("nan"), device=DEV)
    Yv = Yd[:, :K]
    Yv.copy_(torch.from_numpy(Y))
    rows = T[idx] if indexed else T
    return dict(n=n, K=K, C=C, Y=Yv, W=torch.from_numpy(W).to(DEV), bits=_pack(T),
                index=torch.from_numpy(idx).to(DEV) if indexed else None,
                Y64=torch.from_numpy(Y).double(), W64=torch.from_numpy(W).double(),
                T64=torch.from_numpy(rows).double())


def _reference(c):
    Y, W = c["Y64"].clone().requires_grad_(), c["W64"].clone().requires_grad_()
    Z = Y @ W
    loss = torch.nn.functional.binary_cross_entropy_with_logits(Z, c["T64"])
    loss.backward()
    z, t = Z.detach(), c["T64"] > 0.5
    amb = int((z.abs() < AMBIG).sum())
    lo = [int(((z >= AMBIG) & t).sum()), int(((z >= AMBIG) & ~t).sum()), int(((z <= -AMBIG) & t).sum())]
    hi = [int(((z > -AMBIG) & t).sum()), int(((z > -AMBIG) & ~t).sum()), int(((z < AMBIG) & t).sum())]
    return loss.detach(), Y.grad, W.grad, amb, lo, hi, float(z.abs().max())


def _train(hip, c, base=(5, 6, 7)):
    n, K, C = c["n"], c["K"], c["C"]
    loss = torch.full((), float("nan"), device=DEV)
    dY = torch.full((n, K), float("nan"), device=DEV)
    dW = torch.full((K, C), float("nan"), device=DEV)
    counts = torch.tensor(base, dtype=torch.int32, device=DEV)
    hip.linear_bce_train(c["Y"], c["W"], c["bits"], loss, dY, dW, index=c["index"], counts=counts)
    torch.cuda.synchronize()
    return loss.cpu(), dY.cpu(), dW.cpu(), counts.cpu()


def _check(hip, c):
    ref_loss, ref_dY, ref_dW, amb, lo, hi, zmax = _reference(c)
    n, C = c["n"], c["C"]
    assert amb <= 1e-3 * n * C, f"{amb} logits within {AMBIG} of zero out of {n * C}"
    loss, dY, dW, counts = _train(hip, c)
    got = [int(x) - b for x, b in zip(counts, (5, 6, 7))]
    print(f"n={n} K={c['K']} C={C} index={c['index'] is not None}: loss {float(loss):.7f} ref "
          f"{float(ref_loss):.7f}; max|dY err| {float((dY.double() - ref_dY).abs().max()):.2e} "
          f"max|dW err| {float((dW.double() - ref_dW).abs().max()):.2e}; tp/fp/fn {got} in "
          f"{lo}..{hi} ({amb} ambiguous); max|z| {zmax:.1f}")
    assert torch.isfinite(loss)
    torch.testing.assert_close(loss.double(), ref_loss, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dY.double(), ref_dY, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(dW.double(), ref_dW, rtol=1e-4, atol=1e-6)
    for g, a, b in zip(got, lo, hi):
        assert a <= g <= b
    # _fwd: the same loss and counts, bit for bit; counts may be NULL
    loss_f = torch.full((), float("nan"), device=DEV)
    counts_f = torch.tensor([5, 6, 7], dtype=torch.int32, device=DEV)
    hip.linear_bce_fwd(c["Y"], c["W"], c["bits"], loss_f, index=c["index"], counts=counts_f)
    loss_n = torch.full((), float("nan"), device=DEV)
    hip.linear_bce_fwd(c["Y"], c["W"], c["bits"], loss_n, index=c["index"])
    torch.cuda.synchronize()
    assert torch.equal(loss_f.cpu(), loss) and torch.equal(counts_f.cpu(), counts)
    assert torch.equal(loss_n.cpu(), loss)
    # a second _train: everything bit for bit
    again = _train(hip, c)
    for x, y in zip((loss, dY, dW, counts), again):
        assert torch.equal(x, y)


@pytest.mark.parametrize("C", [1, 31, 32, 33, 100, 121, 128])
@pytest.mark.parametrize("K", [16, 128, "max"])
@pytest.mark.parametrize("n", [1, 16, 17, 1000])
def test_linear_bce_matches_the_float64_chain(hip, n, K, C):
    K = max_k(C) if K == "max" else K
    for indexed in (False, True):
        _check(hip, _case(n, K, C, indexed))


def test_padded_rows_on_the_vector_staging_path(hip):
    """ldy = K + 4: 16-byte row loads next to NaN pad floats"""
    c = _case(77, 64, 100, False)
    Yd = torch.full((77, 68), float("nan"), device=DEV)
    Yd[:, :64].copy_(c["Y"])
    c["Y"] = Yd[:, :64]
    assert c["Y"].stride(0) == 68 and c["Y"].data_ptr() % 16 == 0
    _check(hip, c)


@pytest.mark.parametrize("n,K,C", [(17, 128, 100), (1000, 16, 33)])
def test_loss_is_finite_and_right_at_logits_near_100(hip, n, K, C):
    c = _case(n, K, C, True, w_scale=30.0)
    ref_loss, _, _, _, _, _, zmax = _reference(c)
    assert 80.0 < zmax < 250.0, zmax
    loss, dY, dW, _ = _train(hip, c)
    print(f"max|z| {zmax:.1f}: loss {float(loss):.6f} ref {float(ref_loss):.6f}")
    assert torch.isfinite(loss) and torch.isfinite(dY).all() and torch.isfinite(dW).all()
    torch.testing.assert_close(loss.double(), ref_loss, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("K,C", [(256, 128), (max_k(128) + 16, 128), (max_k(100) + 16, 100),
                                 (24, 10), (128, 129), (128, 0)])
def test_unsupported_shapes_are_refused_and_launch_nothing(hip, K, C):
    from nts import _abi
    n, Cw = 20, max(C, 1)
    Y = torch.zeros(n, K, device=DEV)
    W = torch.zeros(K, Cw, device=DEV)
    bits = torch.zeros(n, (Cw + 31) // 32, dtype=torch.int32, device=DEV)
    loss = torch.full((), 123.0, device=DEV)
    dY = torch.full((n, K), 123.0, device=DEV)
    dW = torch.full((K, Cw), 123.0, device=DEV)
    counts = torch.tensor([5, 6, 7], dtype=torch.int32, device=DEV)
    p = _abi.ptr
    rc = hip.lib.nts_hip_linear_bce_train(hip.h, p(Y), K, n, K, p(W), C, p(bits), bits.shape[1], None,
                                          p(loss), p(dY), p(dW), p(counts))
    assert rc == NTS_ERR_INVALID
    assert b"invalid argument" in hip.lib.nts_hip_last_error()
    rc = hip.lib.nts_hip_linear_bce_fwd(hip.h, p(Y), K, n, K, p(W), C, p(bits), bits.shape[1], None,
                                        p(loss), p(counts))
    assert rc == NTS_ERR_INVALID
    torch.cuda.synchronize()
    assert float(loss) == 123.0 and counts.tolist() == [5, 6, 7]
    assert bool((dY == 123.0).all()) and bool((dW == 123.0).all())


def test_supported_matches_the_host_layer_predicate():
    """hip_linear_bce_supported (what the driver asks) agrees with max_k at its edge"""
    from nts import host
    E = host.ext()
    for C in (1, 33, 100, 128):
        assert E.hip_linear_bce_supported(max_k(C), C)
        assert not E.hip_linear_bce_supported(max_k(C) + 16, C)
    assert not E.hip_linear_bce_supported(128, 129) and not E.hip_linear_bce_supported(24, 10)
    assert not E.hip_linear_bce_supported(256, 128)
