"""The helpers of the GAT kernel / driver tests, checked on the CPU: the
synthetic block (tests/gat_blocks.py) and the Adam-step gradient readout
(tests/step_check.py)."""
import numpy as np
import pytest
import torch

import gat_blocks
import step_check


@pytest.fixture(scope="module")
def block():
    return gat_blocks.make_block()


def test_block_shape_and_degrees(block):
    b = block
    assert (b["v"], b["s"]) == (96, 320)
    co, ri = b["column_offset"].astype(np.int64), b["row_indices"]
    deg = np.diff(co)
    assert co[0] == 0 and co[-1] == b["e"] == ri.size and 1300 < b["e"] < 1700
    for d in gat_blocks.SPECIAL_DEGREES:  # every chunk boundary of a column
        assert (deg == d).sum() >= 1, d
    assert (deg == 0).sum() == 1
    assert ri.max() < b["s"]
    # the hub is in every non-empty column: a CSR row of more than one chunk
    for d in range(b["v"]):
        assert deg[d] == 0 or gat_blocks.HUB in ri[co[d]:co[d + 1]]
    ro = b["row_offset"].astype(np.int64)
    assert ro[gat_blocks.HUB + 1] - ro[gat_blocks.HUB] >= 95 > 64
    # dst_local_id is injective into the sources
    dl = b["dst_local_id"]
    assert np.unique(dl).size == b["v"] and dl.max() < b["s"]


def test_block_csr_is_the_transpose(block):
    b = block
    co, ri = b["column_offset"].astype(np.int64), b["row_indices"].astype(np.int64)
    ro, ci, eid = (b[k].astype(np.int64) for k in ("row_offset", "column_indices", "csr_edge_id"))
    e, s = b["e"], b["s"]
    assert np.array_equal(np.sort(eid), np.arange(e))  # a permutation of the edges
    assert ro[0] == 0 and ro[-1] == e and np.all(np.diff(ro) >= 0)
    d_of_e = np.repeat(np.arange(b["v"]), np.diff(co))
    row_of_slot = np.repeat(np.arange(s), np.diff(ro))
    assert np.array_equal(ri[eid], row_of_slot)   # slot k of row r is an edge from r
    assert np.array_equal(d_of_e[eid], ci)        # ... to the slot's destination
    for r in range(s):                            # stable: edge order kept inside a row
        assert np.all(np.diff(eid[ro[r]:ro[r + 1]]) > 0)
    assert np.array_equal(np.bincount(ri, minlength=s), np.diff(ro))


@pytest.mark.parametrize("F,scale", [(16, 0.3), (67, 0.3), (67, 150 / (1.4 * 67 ** 0.5))])
def test_chain_matches_the_per_destination_loop(block, F, scale):
    b = block
    g = torch.Generator().manual_seed(F)
    H = torch.randn(b["s"], F, generator=g, dtype=torch.float64)
    att = torch.randn(2 * F, generator=g, dtype=torch.float64) * scale
    co, ri, dl = (torch.from_numpy(b[k].astype(np.int64))
                  for k in ("column_offset", "row_indices", "dst_local_id"))
    Y, m, a = gat_blocks.gat_chain(H, att, co, ri, dl, F)
    Yl, ml, al = gat_blocks.gat_loop(H.numpy(), att.numpy(), co.numpy(), ri.numpy(), dl.numpy())
    assert np.abs(m.numpy() - ml).max() <= 1e-12 * max(1.0, np.abs(ml).max())
    assert np.abs(a.numpy() - al).max() <= 1e-12
    assert np.abs(Y.numpy() - Yl).max() <= 1e-12 * max(1.0, np.abs(Yl).max())
    # the empty column: a zero row, and nothing non-finite anywhere
    d0 = int(np.flatnonzero(np.diff(co.numpy()) == 0)[0])
    assert not Y[d0].any() and torch.isfinite(Y).all() and torch.isfinite(a).all()
    Z, _, _ = gat_blocks.gat_chain_z(H, att, co, ri, dl, F)
    assert torch.equal(torch.relu(Z), Y)


def _adam_first_step_fp32(W0, G, lr, eps, wd):
    """k_adam's no-bias-correction branch (csrc/aggregate.hip) from zero moments,
    restated in float32 torch"""
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    omb1, omb2 = f(1.0) - f(0.9), f(1.0) - f(0.999)
    wg = W0 * f(wd) + G
    m = f(0.9) * torch.zeros_like(W0) + omb1 * wg
    v = f(0.999) * torch.zeros_like(W0) + (omb2 * wg) * wg
    return W0 - (f(lr) * m) / (torch.sqrt(v) + f(eps))


@pytest.mark.parametrize("gscale", [1e-3, 1e-2, 1.0, 8.0])
def test_recovered_grads_invert_the_adam_step(gscale):
    g = torch.Generator().manual_seed(5)
    W0 = (torch.rand(200, 33, generator=g) - 0.5) * 0.6
    G = torch.randn(200, 33, generator=g) * gscale
    G[0, :4] = torch.tensor([0.0, -0.0, gscale * 1e-3, -gscale * 30])
    W1 = _adam_first_step_fp32(W0, G, step_check.LR, 1.0, 0.0)
    got = step_check.recovered_grads(W0, W1)
    # float32 rounding of W1 (half an ulp of W0 - update, in units of g) and of
    # the four float32 operations of the update (2^-24 each, relative to g)
    top_w = float(torch.maximum(W0.abs(), W1.abs()).max())
    floor = float(np.spacing(np.float32(top_w))) / (step_check.LR * step_check.OMB1)
    assert floor >= step_check.resolution(W0) > 0
    diff = (got - G.double()).abs()
    # the inversion's slope dg/du = (1 + sqrt(1-b2)|g|)^2 amplifies the ulp
    slope = (1.0 + np.sqrt(step_check.OMB2) * G.double().abs()) ** 2
    assert bool((diff <= slope * (floor + 8 * 2.0 ** -24 * G.double().abs())).all())
    # magnitude-sensitive: a doubled gradient is told apart by far more than that
    W2 = _adam_first_step_fp32(W0, 2 * G, step_check.LR, 1.0, 0.0)
    assert step_check.err(step_check.recovered_grads(W0, W2), G) > 0.9
    # ... which the default step (epsilon = 1e-9) cannot see
    lr = 0.01
    A = _adam_first_step_fp32(W0, G, lr, 1e-9, 0.0)
    B = _adam_first_step_fp32(W0, 2 * G, lr, 1e-9, 0.0)
    big = G.abs() > 1e-4
    torch.testing.assert_close(A[big], B[big], rtol=1e-5, atol=1e-5)


def test_check_step_grads_bounds(capsys):
    g = torch.Generator().manual_seed(6)
    W0 = (torch.rand(64, 32, generator=g) - 0.5) * 0.6
    G64 = torch.randn(64, 32, generator=g, dtype=torch.float64) * 1e-2
    G32 = (G64 * (1 + 1e-6)).float()
    W1 = _adam_first_step_fp32(W0, G64.float(), step_check.LR, 1.0, 0.0)
    step_check.check_step_grads([W0], [W1], [G64], [G32], c=4, names=["W"])
    assert "ratio" in capsys.readouterr().out
    W2 = _adam_first_step_fp32(W0, G64.float() * 1.01, step_check.LR, 1.0, 0.0)
    with pytest.raises(AssertionError, match="W:"):
        step_check.check_step_grads([W0], [W2], [G64], [G32], c=4, names=["W"])
