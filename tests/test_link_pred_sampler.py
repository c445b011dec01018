"""FastSampler::issue_gpu_sample_dev: the issue path with the
layer-0 destinations in the caller's device buffers gives, bit for bit, the
blocks issue_gpu_sample gives for the same ids under the same batch_seq."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PHILOX, MT_LEMIRE, SHARED = 0, 1, 3
KEYS = ("destination", "column_offset", "row_indices", "sample_ans", "source",
        "edge_weight_forward", "row_offset", "column_indices", "edge_weight_backward")


@pytest.fixture(scope="module")
def data():
    from nts import host, synthetic
    E = host.ext()
    g = synthetic.chung_lu(2000, 40000, 10.0, device=DEV, seed=3)
    G = E.FullyRepGraph.from_edges(g.src, g.dst, g.n_vertices)
    ids = torch.from_numpy(np.random.default_rng(5).choice(2000, 150, replace=False).astype(np.int64))
    return E, G, ids


@pytest.mark.parametrize("mode", [PHILOX, SHARED])
def test_dev_issue_equals_the_host_issue_bit_for_bit(data, mode):
    E, G, ids = data
    n, cap, fan, seq = ids.numel(), 256, [4, 3], 11
    a = E.FastSampler(G, ids, 2, cap, fan, rng_mode=mode)
    a.batch_seq = seq
    want = a.sample_gpu_fast(n)
    b = E.FastSampler(G, torch.empty(0, dtype=torch.int64), 2, cap, fan, rng_mode=mode)
    b.batch_seq = seq
    dest = torch.full((cap,), -1, dtype=torch.int32, device=DEV)  # more room than ids
    dest[:n] = ids.to(torch.int32).to(DEV)
    vsz = torch.tensor([n], dtype=torch.int32, device=DEV)
    b.issue_dev(dest, vsz, cap)  # the bound, not the live count
    got = b.finish(0)
    assert b.batch_seq == seq + 1 and b.work_offset == 0
    for l, (x, y) in enumerate(zip(want, got)):
        assert (x["v_size"], x["e_size"], x["src_size"]) == (y["v_size"], y["e_size"], y["src_size"])
        assert x["e_size"] > 0
        for k in KEYS:
            assert torch.equal(x[k].view(torch.int32) if x[k].dtype == torch.float32 else x[k],
                               y[k].view(torch.int32) if y[k].dtype == torch.float32 else y[k]), (l, k)
    assert got[0]["v_size"] == n


def test_dev_issue_refuses_an_mt19937_mode(data):
    E, G, ids = data
    s = E.FastSampler(G, ids, 2, 256, [4, 3], rng_mode=MT_LEMIRE)
    dest = ids.to(torch.int32).to(DEV)
    vsz = torch.tensor([ids.numel()], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="MT19937"):
        s.issue_dev(dest, vsz, ids.numel())
