"""tests/dropout_chain.py without a GPU: at p = 0 it is the undropped chains the
driver tests already use, bit for bit in float64; the rebuilt masks have the
rate, offset and key dependence of the kernels' rule; a dropped column cuts the
gradient exactly; and the offset schedule.  The layers are random bipartite
blocks in the sampler's layout (top first; every destination is a source)."""
import types

import numpy as np
import pytest
import torch

import dropout_chain as dc
import test_host
import test_layer_norm_driver as tld

V = 300


def _toy_layers(widths, seeds, fan, seed):
    """len(widths) - 1 sampled layers, top first, over vertices 0 .. V - 1"""
    rng = np.random.default_rng(seed)
    dst, lays = np.asarray(seeds, np.int64), []
    for _ in range(len(widths) - 1):
        deg = rng.integers(1, fan + 1, dst.size)
        nbr = rng.integers(0, V, int(deg.sum()))
        source = np.unique(np.concatenate([dst, nbr]))
        t = lambda a, dt=torch.int32: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
        lays.append({"column_offset": t(np.concatenate([[0], np.cumsum(deg)])),
                     "row_indices": t(np.searchsorted(source, nbr)),
                     "edge_weight_forward": t(rng.uniform(0.1, 1.0, nbr.size), torch.float32),
                     "source": t(source), "destination": t(dst),
                     "dst_local_id": t(np.searchsorted(source, dst)),
                     "v_size": int(dst.size), "src_size": int(source.size)})
        dst = source
    return lays


def _data(widths, seed):
    g = torch.Generator().manual_seed(seed)
    return {"feat": torch.randn(V, widths[0], generator=g),
            "labels": torch.randint(0, widths[-1], (V,), generator=g)}


def _weights(widths, seed, norm=False):
    g = torch.Generator().manual_seed(seed)
    ws = [0.3 * torch.randn(a, b, generator=g) for a, b in zip(widths[:-1], widths[1:])]
    for w in widths[1:-1] if norm else ():
        ws += [1 + 0.1 * torch.randn(w, generator=g), 0.1 * torch.randn(w, generator=g)]
    return ws


def _grads(P, loss):
    loss.backward()
    return [p.grad for p in P]


def test_p0_is_the_plain_gcn_chain_of_test_host():
    widths = [12, 6, 5]
    lays, data, ws = _toy_layers(widths, range(0, 40, 2), 4, 1), _data(widths, 2), _weights(widths, 3)
    P, loss, hidden, masks = dc.chain(lays, data, ws, torch.float64, 0.0, 2000, 0)
    assert len(hidden) == len(masks) == 1 and bool(masks[0].all())
    want = test_host._gcn_chain_grads(types.SimpleNamespace(last_layers=lays), data["feat"], data["labels"],
                                      ws, torch.float64)
    for a, b in zip(_grads(P, loss), want):
        assert float(b.abs().max()) > 0 and torch.equal(a, b)


@pytest.mark.parametrize("widths", [[12, 6, 5], [12, 6, 7, 5]], ids=["2-layers", "3-layers"])
def test_p0_is_the_layer_norm_chain(widths):
    lays = _toy_layers(widths, range(1, 50, 3), 4, 4)
    data, ws = _data(widths, 5), _weights(widths, 6, norm=True)
    P, loss, hidden, _ = dc.chain(lays, data, ws, torch.float64, 0.0, 2000, 0, norm="layer")
    Q, want, hidden_q, _ = tld._chain(lays, data, ws, torch.float64)
    assert torch.equal(loss.detach(), want.detach())
    for a, b in zip(hidden, hidden_q):
        assert torch.equal(a, b)
    for a, b in zip(_grads(P, loss), _grads(Q, want)):
        assert float(b.abs().max()) > 0 and torch.equal(a, b)


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_kept_fraction(p):
    m = dc.keep(4096, 128, p, dc.key(2000), 3)
    assert m.dtype == torch.bool and tuple(m.shape) == (4096, 128)
    q = 1 - int(p * 65536) / 65536  # kept iff 16 uniform bits >= floor(p 2^16)
    n = m.numel()
    got = float(m.double().mean())
    print(f"p {p}: kept {got:.6f}, expected {q:.6f}, sigma {np.sqrt(q * (1 - q) / n):.2e}")
    assert abs(got - q) <= 5 * np.sqrt(q * (1 - q) / n)


def test_masks_depend_on_the_offset_and_on_both_words_of_the_key():
    assert dc.key(0) == 1 and dc.key(1) == 0x9E3779B97F4A7C16
    assert dc.key(2000) == (2000 * 0x9E3779B97F4A7C15 + 1) % 2 ** 64
    a = dc.keep(64, 32, 0.5, dc.key(2000), 0)
    assert torch.equal(a, dc.keep(64, 32, 0.5, dc.key(2000), 0))
    assert not torch.equal(a, dc.keep(64, 32, 0.5, dc.key(2000), 1))
    # 2^32 more in the seed moves only the key's high word
    assert dc.key(2000 + 2 ** 32) & 0xFFFFFFFF == dc.key(2000) & 0xFFFFFFFF
    assert dc.key(2000 + 2 ** 32) >> 32 != dc.key(2000) >> 32
    assert not torch.equal(a, dc.keep(64, 32, 0.5, dc.key(2000 + 2 ** 32), 0))
    assert dc.scale(0.5) == 2.0 and dc.scale(0.0) == 1.0
    assert dc.scale(0.9) == float(np.float32(1) / (np.float32(1) - np.float32(0.9)))


def test_a_dropped_column_cuts_the_gradient_exactly():
    """One hidden unit: where its whole mask column is zero nothing reaches the
    loss through it, so both weights' float64 gradients are exactly zero; an
    offset that keeps a row gives gradients that are not."""
    widths, p = [6, 1, 3], 0.9
    lays, data, ws = _toy_layers(widths, [5, 9, 11], 2, 7), _data(widths, 8), _weights(widths, 9)
    ws[0] = ws[0].abs()  # with the positive features below: the unit is on in every row
    data["feat"] = data["feat"].abs()
    v = lays[1]["v_size"]
    cut = next(o for o in range(64) if not dc.keep(v, 1, p, dc.key(2000), o).any())
    used = lays[0]["row_indices"].long()  # the hidden rows that the top hop reads
    kept = next(o for o in range(64) if dc.keep(v, 1, p, dc.key(2000), o)[used].any())
    P, loss, hidden, masks = dc.chain(lays, data, ws, torch.float64, p, 2000, cut)
    assert not masks[0].any() and float(hidden[0].detach().abs().max()) == 0.0
    for g in _grads(P, loss):
        assert torch.equal(g, torch.zeros_like(g))
    P, loss, hidden, masks = dc.chain(lays, data, ws, torch.float64, p, 2000, kept)
    g0, g1 = _grads(P, loss)
    assert float(g0.abs().max()) > 0 and float(g1.abs().max()) > 0
    # the kept rows carry scale(p) times the undropped activation, the others nothing
    plain = dc.chain(lays, data, ws, torch.float64, 0.0, 2000, 0)[2][0]
    assert torch.equal(hidden[0], plain * masks[0].double() * dc.scale(p))


def test_schedule():
    assert [dc.offsets(k, 3) for k in (0, 1)] == [[0, 1], [2, 3]]
    assert [dc.offsets(k, 2) for k in (0, 1, 2)] == [[0], [1], [2]]
    assert dc.offsets(5, 4) == [15, 16, 17]
    # chain() draws them in layer order from first_offset
    widths = [8, 4, 4, 3]
    lays, data, ws = _toy_layers(widths, range(0, 30, 2), 3, 10), _data(widths, 11), _weights(widths, 12)
    masks = dc.chain(lays, data, ws, torch.float64, 0.5, 2000, dc.offsets(1, 3)[0])[3]
    for l, off in enumerate(dc.offsets(1, 3)):
        assert torch.equal(masks[l], dc.keep(lays[2 - l]["v_size"], widths[l + 1], 0.5, dc.key(2000), off))
