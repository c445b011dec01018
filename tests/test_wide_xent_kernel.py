"""nts_hip_linear_xent_fwd / _bwd / _train at 64 < C <= 512 (csrc/top.hip,
k_top_xent_wide): the fused output layer + softmax loss with W streamed from
global memory.

Reference: libtorch in float64 on the same tensors — Y @ W, log_softmax twice,
mean nll_loss, autograd's backward (the reference of test_linear_xent_fused).

Bounds: the project's own from tests/test_hip_kernels.py::test_linear_xent_fused:
loss rtol = atol = 1e-5; dY, dW rtol 1e-4, atol 1e-6.  `correct` as that test
counts it: rows whose two best float64 logits differ by <= 1e-4 may go either
way.

Inputs: Y ~ N(0,1), W ~ 0.1 N(0,1), uniform labels.  Shapes (n, K, C) are the
smallest at which the kernel can still go wrong:
  (1, 16, 65)        first wide class count, one row
  (17, 16, 512)      largest C, partial second row tile
  (77, 32, 80)       Cp == C
  (33, 64, 349)      odd C: unaligned W rows
  (1024, 256, 172)   the papers100M-shaped configuration's top layer
  (300, 512, 512)    both limits, the LDS worst case
  (2100, 512, 512)   132 row tiles on 128 blocks: four blocks walk a second
                     tile and add onto their dW slab
K > 512 is refused above 64 classes, so (528, 512) is among the refusals.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NTS_ERR_INVALID = 1
SHAPES = [(1, 16, 65), (17, 16, 512), (77, 32, 80), (33, 64, 349), (1024, 256, 172),
          (300, 512, 512), (2100, 512, 512)]


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=2000)


def _reference(Y, W, lab):
    """float64 loss, (dY, dW) for d loss = 1, the logits"""
    Yr, Wr = Y.double().requires_grad_(), W.double().requires_grad_()
    Z = Yr @ Wr
    ref = torch.nn.functional.nll_loss(Z.log_softmax(1).log_softmax(1), lab)
    ref.backward()
    return ref.detach(), Yr.grad, Wr.grad, Z.detach()


@functools.lru_cache(maxsize=None)
def _case(n, K, C, w_scale=0.1):
    g = torch.Generator(device=DEV).manual_seed(n + K + C)
    Y = torch.randn(n, K, device=DEV, generator=g)
    W = torch.randn(K, C, device=DEV, generator=g) * w_scale
    lab = torch.randint(0, C, (n,), device=DEV, generator=g)
    return Y, W, lab, _reference(Y, W, lab)


def _outputs(n, K, C):
    return (torch.full((), float("nan"), device=DEV), torch.full((n, K), float("nan"), device=DEV),
            torch.full((K, C), float("nan"), device=DEV))


def _train(hip, Y, W, lab, base=5):
    n, K = Y.shape
    loss, dY, dW = _outputs(n, K, W.shape[1])
    correct = torch.full((1,), base, dtype=torch.int32, device=DEV)
    hip.linear_xent_train(Y, W, lab, loss, dY, dW, correct)
    torch.cuda.synchronize()
    return loss, dY, dW, int(correct) - base


def _assert_close(got, ref, what):
    loss, dY, dW = got
    ref_loss, ref_dY, ref_dW = ref
    print(f"{what}: loss {float(loss):.7f} ref {float(ref_loss):.7f}; max|dY err| "
          f"{float((dY.double() - ref_dY).abs().max()):.2e} max|dW err| "
          f"{float((dW.double() - ref_dW).abs().max()):.2e}")
    torch.testing.assert_close(loss.double(), ref_loss, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dY.double(), ref_dY, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(dW.double(), ref_dW, rtol=1e-4, atol=1e-6)


def _correct_band(Z, lab):
    top2 = Z.topk(2, 1).values
    clear = top2[:, 0] - top2[:, 1] > 1e-4
    want = int(((Z.argmax(1) == lab) & clear).sum())
    return want, want + int((~clear).sum())


@pytest.mark.parametrize("n,K,C", SHAPES)
def test_train_matches_the_float64_chain(hip, n, K, C):
    Y, W, lab, (ref_loss, ref_dY, ref_dW, Z) = _case(n, K, C)
    loss, dY, dW, correct = _train(hip, Y, W, lab)
    _assert_close((loss, dY, dW), (ref_loss, ref_dY, ref_dW), f"({n}, {K}, {C})")
    lo, hi = _correct_band(Z, lab)
    print(f"correct {correct} in [{lo}, {hi}]")
    assert lo <= correct <= hi
    # a second training call: scratch and partials leave nothing behind
    again = _train(hip, Y, W, lab)
    assert torch.equal(loss, again[0]) and torch.equal(dY, again[1]) and torch.equal(dW, again[2])
    assert correct == again[3]


@pytest.mark.parametrize("n,K,C", SHAPES)
def test_train_is_forward_then_backward_bit_for_bit(hip, n, K, C):
    Y, W, lab, (ref_loss, ref_dY, ref_dW, Z) = _case(n, K, C)
    loss, dY, dW, correct = _train(hip, Y, W, lab)
    loss2, dY2, dW2 = _outputs(n, K, C)
    correct2 = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    hip.linear_xent_fwd(Y, W, lab, loss2, correct2)
    hip.linear_xent_bwd(Y, W, lab, torch.ones((), device=DEV), dY2, dW2)
    loss3 = torch.full((), float("nan"), device=DEV)
    hip.linear_xent_fwd(Y, W, lab, loss3)  # correct may be NULL
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2) and torch.equal(loss, loss3)
    assert torch.equal(dY, dY2) and torch.equal(dW, dW2)
    assert int(correct2) - 5 == correct
    # an upstream gradient other than 1: autograd's backward is linear in it
    loss4, dY4, dW4 = _outputs(n, K, C)
    hip.linear_xent_bwd(Y, W, lab, torch.tensor(1.7, device=DEV), dY4, dW4)
    torch.cuda.synchronize()
    torch.testing.assert_close(dY4.double(), 1.7 * ref_dY, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(dW4.double(), 1.7 * ref_dW, rtol=1e-4, atol=1e-6)


def test_labels_in_the_last_class_and_the_last_partial_column_tile(hip):
    n, K, C = 33, 64, 349  # the last column tile holds classes 336 .. 348
    Y, W, _, _ = _case(n, K, C)
    lab = torch.randint(0, C, (n,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
    lab[0::3] = C - 1
    lab[1::3] = 340
    lab[32] = 336
    ref_loss, ref_dY, ref_dW, Z = _reference(Y, W, lab)
    loss, dY, dW, correct = _train(hip, Y, W, lab)
    _assert_close((loss, dY, dW), (ref_loss, ref_dY, ref_dW), "targeted labels")
    lo, hi = _correct_band(Z, lab)
    assert lo <= correct <= hi


@pytest.mark.parametrize("j1,j2", [(19, 81), (5, 69), (3, 171)])
def test_argmax_takes_the_first_of_two_equal_classes(hip, j1, j2):
    """Two identical columns of W give bit-equal logits (the same chain of
    products in both lanes); a dominant first feature makes them each row's
    largest.  (19, 81): the lower class sits on the higher lane of another
    wave's column tile; (5, 69): the same lane; (3, 171): the last class."""
    n, K, C = 77, 32, 172
    Y, W, _, _ = _case(n, K, C)
    Y, W = Y.clone(), W.clone()
    Y[:, 0] = 5.0
    W[:, j2] = W[:, j1]
    W[0, j1] = W[0, j2] = 3.0
    Z = Y.double() @ W.double()
    assert bool((Z.topk(3, 1).values[:, 1] - Z.topk(3, 1).values[:, 2] > 1.0).all())
    for label, want in ((j2, 0), (j1, n)):
        lab = torch.full((n,), label, dtype=torch.int64, device=DEV)
        ref_loss, ref_dY, ref_dW, _ = _reference(Y, W, lab)
        loss, dY, dW, correct = _train(hip, Y, W, lab)
        assert correct == want
        _assert_close((loss, dY, dW), (ref_loss, ref_dY, ref_dW), f"tie, label {label}")


@pytest.mark.parametrize("n,K,C", [(33, 64, 349), (77, 32, 80)])
def test_padded_unaligned_rows_and_rows_past_n(hip, n, K, C):
    Y, W, lab, (ref_loss, ref_dY, ref_dW, _) = _case(n, K, C)
    loss, dY, dW, correct = _train(hip, Y, W, lab)
    # pitch K + 3: the scalar staging path, NaN pad floats
    Yb = torch.full((n, K + 3), float("nan"), device=DEV)
    Yb[:, :K].copy_(Y)
    got = _train(hip, Yb[:, :K], W, lab)
    _assert_close(got[:3], (ref_loss, ref_dY, ref_dW), "pitch K + 3")
    assert torch.equal(got[0], loss) and torch.equal(got[1], dY) and torch.equal(got[2], dW)
    # a NaN-filled allocation of n + 5 rows, n rows passed: rows past n reach no result
    Yc = torch.full((n + 5, K), float("nan"), device=DEV)
    Yc[:n].copy_(Y)
    got = _train(hip, Yc[:n], W, lab)
    assert torch.isfinite(got[0]) and torch.isfinite(got[1]).all() and torch.isfinite(got[2]).all()
    assert torch.equal(got[0], loss) and torch.equal(got[1], dY) and torch.equal(got[2], dW)
    assert got[3] == correct


@pytest.mark.parametrize("n,K,C,w_scale", [(17, 256, 65, 2.0), (33, 64, 349, 3.0)])
def test_large_logits_stay_finite_and_the_loss_right(hip, n, K, C, w_scale):
    """max |z| about 105-116: every softmax is max-subtracted.  The gradient
    bounds are not applied here: the fp32 libtorch chain itself uses 40-70 % of
    them at these shapes."""
    Y, W, lab, (ref_loss, _, _, Z) = _case(n, K, C, w_scale)
    zmax = float(Z.abs().max())
    assert 80.0 < zmax < 250.0, zmax
    loss, dY, dW, _ = _train(hip, Y, W, lab)
    print(f"max|z| {zmax:.1f}: loss {float(loss):.6f} ref {float(ref_loss):.6f}")
    assert torch.isfinite(loss) and torch.isfinite(dY).all() and torch.isfinite(dW).all()
    torch.testing.assert_close(loss.double(), ref_loss, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("K,C", [(16, 513), (24, 100), (528, 512)])
def test_unsupported_shapes_are_refused_and_launch_nothing(hip, K, C):
    from nts import _abi
    n = 20
    Y = torch.zeros(n, K, device=DEV)
    W = torch.zeros(K, C, device=DEV)
    lab = torch.zeros(n, dtype=torch.int64, device=DEV)
    loss = torch.full((), 123.0, device=DEV)
    dY = torch.full((n, K), 123.0, device=DEV)
    dW = torch.full((K, C), 123.0, device=DEV)
    correct = torch.tensor([5], dtype=torch.int32, device=DEV)
    one = torch.ones((), device=DEV)
    p = _abi.ptr
    for rc in (hip.lib.nts_hip_linear_xent_train(hip.h, p(Y), K, n, K, p(W), C, p(lab), p(loss),
                                                 p(dY), p(dW), p(correct)),
               hip.lib.nts_hip_linear_xent_fwd(hip.h, p(Y), K, n, K, p(W), C, p(lab), p(loss),
                                               p(correct)),
               hip.lib.nts_hip_linear_xent_bwd(hip.h, p(Y), K, n, K, p(W), C, p(lab), p(one), p(dY),
                                               p(dW))):
        assert rc == NTS_ERR_INVALID
        assert b"invalid argument" in hip.lib.nts_hip_last_error()
    torch.cuda.synchronize()
    assert float(loss) == 123.0 and int(correct) == 5
    assert bool((dY == 123.0).all()) and bool((dW == 123.0).all())


@pytest.mark.parametrize("n,K,C", [(33, 16, 7), (1, 16, 64)])
def test_narrow_shapes_still_take_their_own_kernels(hip, n, K, C):
    """a cheap guard that the dispatch did not reroute C <= 64: right against
    float64 and bit-identical between two calls"""
    Y, W, lab, (ref_loss, ref_dY, ref_dW, _) = _case(n, K, C)
    a, b = _train(hip, Y, W, lab), _train(hip, Y, W, lab)
    _assert_close(a[:3], (ref_loss, ref_dY, ref_dW), f"narrow ({n}, {K}, {C})")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert a[3] == b[3]


def test_supported_matches_the_host_layer_predicate(hip):
    """hip_linear_xent_supported (what the driver asks) is the argument check"""
    from nts import _abi, host
    E = host.ext()
    p = _abi.ptr
    for K, C in [(16, 65), (512, 512), (528, 512), (528, 65), (16, 513), (24, 100), (128, 349),
                 (512, 64), (128, 64), (16, 64)]:
        Y = torch.zeros(1, K, device=DEV)
        W = torch.zeros(K, C, device=DEV)
        lab = torch.zeros(1, dtype=torch.int64, device=DEV)
        loss = torch.zeros((), device=DEV)
        rc = hip.lib.nts_hip_linear_xent_fwd(hip.h, p(Y), K, 1, K, p(W), C, p(lab), p(loss), None)
        torch.cuda.synchronize()
        assert (rc == 0) == E.hip_linear_xent_supported(K, C), (K, C, rc)
