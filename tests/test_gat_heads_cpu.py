"""Multi-head GAT, the parts that need no GPU: the references of
tests/gat_heads_blocks.py against each other, the exported symbols and their
argument checks, the GAT_HEADS cfg key, gcn_config's validation, and numpy
emulations of two wrong kernels (never run on a GPU) that show the kernel
test's bound would catch them."""
import ctypes

import numpy as np
import pytest
import torch

import gat_blocks
import gat_heads_blocks as ghb
from conftest import GOLDEN, ROOT
from nts import dataloader
from step_check import C, err, yardstick_bound

CFG = GOLDEN / "cora" / "gcn_cora_sample.cfg"
SYMBOLS = ("nts_hip_gat_forward_heads", "nts_hip_gat_backward_heads")


@pytest.fixture(scope="module")
def block():
    b = gat_blocks.make_block()
    cpu = {k: torch.from_numpy(b[k].astype(np.int64))
           for k in ("column_offset", "row_indices", "dst_local_id")}
    return dict(np=b, cpu=cpu, v=b["v"], s=b["s"], e=b["e"])


def _inputs(block, K, D, seed=5):
    g = torch.Generator().manual_seed(seed)
    H = torch.randn(block["s"], K * D, generator=g, dtype=torch.float64)
    att = torch.randn(2 * K * D, generator=g, dtype=torch.float64) * 0.3
    return H, att


def test_one_head_is_the_single_head_chain(block):
    c = block["cpu"]
    H, att = _inputs(block, 1, 12)
    args = (c["column_offset"], c["row_indices"], c["dst_local_id"])
    Y1, m1, a1 = gat_blocks.gat_chain(H, att, *args, 12)
    for mean in (False, True):
        Y, m, a = ghb.heads_chain(H, att, *args, 1, 12, mean)
        assert torch.equal(Y, Y1) and torch.equal(m[:, 0], m1) and torch.equal(a[:, 0], a1)


@pytest.mark.parametrize("K,D,mean", [(3, 7, False), (8, 7, True)])
def test_chain_matches_the_per_destination_loop(block, K, D, mean):
    c, b = block["cpu"], block["np"]
    H, att = _inputs(block, K, D)
    Y, m, a = ghb.heads_chain(H, att, c["column_offset"], c["row_indices"], c["dst_local_id"],
                              K, D, mean)
    Yl, ml, al = ghb.heads_loop(H.numpy(), att.numpy(), b["column_offset"].astype(np.int64),
                                b["row_indices"].astype(np.int64),
                                b["dst_local_id"].astype(np.int64), K, D, mean)
    assert Y.shape == (block["v"], D if mean else K * D) and m.shape == (block["e"], K)
    for got, ref in ((Y, Yl), (m, ml), (a, al)):
        np.testing.assert_allclose(got.numpy(), ref, rtol=1e-12, atol=1e-13)


def test_symbols_are_declared_and_exported():
    from nts import _abi
    header = (ROOT / "include" / "nts_hip.h").read_text()
    lib = _abi.lib()
    for name in SYMBOLS:
        assert name in header and name in _abi.EXPORTED
        assert getattr(lib, name).argtypes is not None
    assert lib.nts_hip_abi_version() == 11


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from nts import _abi
    lib = _abi.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)  # 16-byte aligned or not: nothing is launched

    def invalid(rc, what):
        assert rc == 1  # NTS_ERR_INVALID
        assert b"invalid argument" in lib.nts_hip_last_error()
        assert what in lib.nts_hip_last_error(), lib.nts_hip_last_error()

    fwd, bwd = (getattr(lib, s) for s in SYMBOLS)

    def f(heads, D, ldh, ldy, mean, ctx=p):  # (ctx, co, ri, dl, v, H, ldh, K, D, att, m, a, Y, ldy, mean)
        return fwd(ctx, p, p, p, 4, p, ldh, heads, D, p, p, p, p, ldy, mean)

    def g(heads, D, ld, ldy, mean, dS=p):
        return bwd(p, p, p, p, 4, p, p, p, 4, p, ld, heads, D, p, p, p, p, ldy, p, ldy, p, p, p, ld,
                   p, ld, dS, mean)

    invalid(f(2, 8, 16, 16, 0, ctx=None), b"NULL")
    invalid(g(2, 8, 16, 16, 0, dS=None), b"NULL")
    for call in (f, g):
        invalid(call(0, 8, 16, 16, 0), b"heads must be >= 1")
        invalid(call(2, 0, 16, 16, 0), b"heads must be >= 1")
        invalid(call(257, 4, 1028, 1028, 0), b"1024")   # F = 1028, float4-eligible
        invalid(call(4, 257, 1028, 1028, 0), b"1024")   # F = 1028
        invalid(call(1, 257, 260, 260, 0), b"256")      # scalar, F = 257
        invalid(call(2, 130, 260, 260, 0), b"D a multiple of 4")  # D % 4 != 0: scalar, F = 260
        invalid(call(2, 8, 15, 16, 0), b"leading dimension")
        invalid(call(2, 8, 16, 15, 0), b"leading dimension")
        invalid(call(2, 8, 16, 7, 1), b"leading dimension")  # mean: Y is D wide


def test_gat_heads_key_parses_and_names_itself_in_errors(tmp_path):
    assert dataloader.InputInfo.from_cfg(CFG).gat_heads == []
    (tmp_path / "job.cfg").write_text(CFG.read_text() + "GAT_HEADS:8-1\n")
    info = dataloader.InputInfo.from_cfg(tmp_path / "job.cfg")
    assert info.gat_heads == [8, 1]
    assert info.layers == [1433, 256, 7]  # the rest of the job is unchanged
    for bad in ("8-x", "8--1", "0-1", "", "8,1", "-1"):
        (tmp_path / "bad.cfg").write_text(CFG.read_text() + f"GAT_HEADS:{bad}\n")
        with pytest.raises(ValueError, match="GAT_HEADS"):
            dataloader.InputInfo.from_cfg(tmp_path / "bad.cfg")


def test_run_refuses_gat_heads_with_a_non_gat_algorithm(tmp_path):
    from nts import run
    (tmp_path / "job.cfg").write_text(CFG.read_text() + "GAT_HEADS:8-1\n")
    info = dataloader.InputInfo.from_cfg(tmp_path / "job.cfg")
    assert run.ALGORITHMS[info.algorithm.upper()][0] != "gat"
    with pytest.raises(SystemExit, match="GAT_HEADS is not supported"):
        run.build_driver(None, info, None, None, None, None, None)


def test_gcn_config_validates_gat_heads():
    from nts import host
    assert list(host.gcn_config([32, 16, 8], [5, 5], 64, gat=True).gat_heads) == []
    assert list(host.gcn_config([32, 16, 8], [5, 5], 64, gat=True, gat_heads=[8, 1]).gat_heads) == [8, 1]
    assert list(host.gcn_config([32, 16, 8], [5, 5], 64, gat=True, gat_heads=[4, 8]).gat_heads) == [4, 8]
    bad = [
        (dict(gat=False, gat_heads=[8, 1]), "gat_heads is not supported without gat"),
        (dict(gat=True, gat_heads=[8]), "gat_heads needs one entry per layer"),
        (dict(gat=True, gat_heads=[8, 1, 1]), "gat_heads needs one entry per layer"),
        (dict(gat=True, gat_heads=[0, 1]), r"gat_heads\[0\] must be >= 1"),
        (dict(gat=True, gat_heads=[3, 1]), r"gat_heads\[0\] = 3 does not divide layer width 16"),
        # mean-mode output with K C > 256 and C % 4 != 0
        (dict(gat=True, gat_heads=[1, 40], layers=[32, 16, 7]), r"gat_heads\[1\].*width limit"),
        (dict(gat=True, gat_heads=[2, 1], layers=[32, 260, 7]), r"gat_heads\[0\].*width limit"),
    ]
    for kw, msg in bad:
        layers = kw.pop("layers", [32, 16, 8])
        with pytest.raises(ValueError, match=msg):
            host.gcn_config(layers, [5, 5], 64, **kw)


# ---- "seen to fail": wrong kernels emulated in numpy, held to the kernel test's bound ----
def _chain(block, H, att, GY, K, D, mean, dtype):
    c = block["cpu"]
    Hd = H.detach().to(dtype).clone().requires_grad_(True)
    ad = att.detach().to(dtype).clone().requires_grad_(True)
    Z, m, a = ghb.heads_chain_z(Hd, ad, c["column_offset"], c["row_indices"], c["dst_local_id"],
                                K, D, mean)
    Y = torch.relu(Z)
    Y.backward(GY.to(dtype))
    return dict(Y=Y.detach(), m=m.detach(), dH=Hd.grad)


def test_a_whole_wave_reduction_would_exceed_the_bound(block):
    """A forward whose dot products are reduced over the whole wave gives every
    head the sum of all heads' pre-leaky scores.  Emulated in float64 on the
    (8, 8) case: m and Y miss the kernel test's bound by orders of magnitude."""
    K, D = 8, 8
    b = block["np"]
    H, att = _inputs(block, K, D, seed=64080)
    H32, att32 = H.float(), att.float()
    GY = torch.zeros(block["v"], K * D, dtype=torch.float64)
    r64 = _chain(block, H, att, GY, K, D, False, torch.float64)
    r32 = _chain(block, H32, att32, GY, K, D, False, torch.float32)
    co = b["column_offset"].astype(np.int64)
    ri, dl = b["row_indices"].astype(np.int64), b["dst_local_id"].astype(np.int64)
    Hn, an = H.numpy(), att.numpy()
    F = K * D
    m = np.zeros((block["e"], K))
    Y = np.zeros((block["v"], F))
    for d in range(block["v"]):
        lo, hi = co[d], co[d + 1]
        if lo == hi:
            continue
        u = Hn[ri[lo:hi]] @ an[:F] + Hn[dl[d]] @ an[F:]  # the whole row's dot product
        s = np.where(u > 0, u, 0.2 * u)
        m[lo:hi] = s[:, None]
        w = np.exp(s - s.max())
        Y[d] = np.maximum((w / w.sum()) @ Hn[ri[lo:hi]], 0)
    for k, wrong in (("m", torch.from_numpy(m)), ("Y", torch.from_numpy(Y))):
        bound = yardstick_bound(err(r32[k], r64[k]), C)
        e = err(wrong, r64[k])
        print(f"whole-wave reduction, {k}: err {e:.3e} bound {bound:.3e} ({e / bound:.1e} x)")
        assert e > 1000 * bound


def test_a_mean_backward_without_one_over_k_would_exceed_the_bound(block):
    """Mean mode whose backward forgets the 1/K hands every head GY instead of
    GY / K: dH comes out K times too large.  Emulated with float64 autograd on
    the (4, 16, mean) case."""
    K, D = 4, 16
    H, att = _inputs(block, K, D, seed=64042)
    g = torch.Generator().manual_seed(1)
    GY = torch.randn(block["v"], D, generator=g, dtype=torch.float64)
    r64 = _chain(block, H, att, GY, K, D, True, torch.float64)
    r32 = _chain(block, H.float(), att.float(), GY, K, D, True, torch.float32)
    wrong = _chain(block, H, att, GY * K, K, D, True, torch.float64)
    bound = yardstick_bound(err(r32["dH"], r64["dH"]), C)
    e = err(wrong["dH"], r64["dH"])
    print(f"mean backward without 1/K, dH: err {e:.3e} bound {bound:.3e} ({e / bound:.1e} x)")
    assert e > 1000 * bound
