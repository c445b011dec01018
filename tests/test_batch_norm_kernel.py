"""The fused BatchNorm + relu + dropout kernels (csrc/norm.hip) through the C-ABI.

Cases (tests/batch_norm_cases.py).  rows 1, 2, 3, 5, 601 (38 blocks of 16
rows, the last ragged) over nine layouts: F 1, 7, 64, 67, 128, 260, 1024, F = 128
with pitch 130 and with a base 4 bytes off (both force the scalar path); rows
16,400 (the first count whose per-block run is past its minimum) at F = 7 and
F = 128; F = 1028 must be refused with nothing written.  Inputs: randn; 1e4 +
randn (a one-pass variance loses everything there); column c offset by 100 c (a
cross-column mix-up shows); one column constant over the rows; p 0 and 0.5;
random starting buffers; |beta| >= 0.01.

Bound.  The project's rule (tests/step_check.py): for every quantity q of
(y, mean, rstd, running_mean, running_var, dz, dgamma, dbeta) and the eval
kernel's y, err(kernel) <= C err(float32 torch chain) + FLOOR against the
float64 chain, err(x) = max|x - q64| / max|q64|.  A quantity whose float64 value
is identically zero (dz at rows == 1; dz and dgamma at F = 1 with the constant
column) must be exactly zero.  Every ratio is printed (the table is in DESIGN
§8s).

Elements whose float64 pre-activation lies within 1e-4 of zero are left out of
the y comparison and get a zero incoming gradient (the relu gate may flip
there); their share is asserted <= 1e-3 in every case
(tests/test_batch_norm_cpu.py asserts the same on the float64 chain alone).

The constant column.  var = 0, so rstd = 1 / sqrt(eps), mean = the constant and
xh = 0 exactly: y = dropout(relu(beta)) and dgamma = 0 bit for bit.  dz of that
column is gamma rstd (g - mean_r g), as autograd through torch's batch_norm
gives it: zero exactly where the gate is shut (beta < 0) and whenever rows == 1,
held to the bound with the rest of dz otherwise.

Every row operand sits in an allocation with a pitch wider than F and extra
rows: input padding is NaN, output padding a sentinel that must survive.
"""
import numpy as np
import pytest
import torch

import batch_norm_cases as bc
from batch_norm_cases import EPS, MOM
from step_check import C, FLOOR, err, yardstick_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -12345.5
SEED, OFFSET = 0x1234567, 5
TRAIN_Q = ("y", "mean", "rstd", "running_mean", "running_var", "dz", "dgamma", "dbeta")
RATIOS = {}  # (layout, rows, input, p, quantity) -> err(kernel) / err(fp32 chain)


@pytest.fixture(scope="module")
def hip():
    from nts.hip import HipContext
    return HipContext(0, seed=2000)


def _buf(rows, F, pitch, off, fill):
    """(flat, view [rows, F]): rows + 2 rows of `pitch` floats, `off` floats into
    a fresh allocation filled with `fill`"""
    n = (rows + 2) * pitch
    flat = torch.full((n + 4,), fill, device=DEV)
    return flat, flat[off:off + n].view(rows + 2, pitch)[:rows, :F]


def _in(x, pitch, off):
    _, v = _buf(x.shape[0], x.shape[1], pitch, off, float("nan"))
    v.copy_(x.to(DEV))
    return v


def _vec(x=None, F=None):
    """an [F] operand with two sentinel elements behind it"""
    F = x.numel() if x is not None else F
    t = torch.full((F + 2,), SENT, device=DEV)
    if x is not None:
        t[:F].copy_(x.to(DEV))
    return t


def _intact(flat, view):
    return int((flat == SENT).sum()) - int((view == SENT).sum()) == flat.numel() - view.numel()


def _keep(hip, rows, F, p):
    """the keep pattern of nts_hip_relu_dropout_f32 for (SEED, OFFSET)"""
    if p == 0:
        return torch.ones(rows, F, dtype=torch.bool)
    y = torch.empty(rows, F, device=DEV)
    hip.relu_dropout(torch.ones(rows, F, device=DEV), y, p, SEED, OFFSET)
    return (y > 0).cpu()


class Run:
    def __init__(self, hip, t, pitch, off, p, running=True):
        z, gamma, beta, dy, rm, rv = t
        rows, F = z.shape
        self.rows, self.F, self.scale = rows, F, 1.0 / (1.0 - p)
        self.z, self.dy = _in(z, pitch, off), _in(dy, pitch, off)
        self.gamma, self.beta = gamma.to(DEV), beta.to(DEV)
        self.y_flat, self.y = _buf(rows, F, pitch, off, SENT)
        self.dz_flat, self.dz = _buf(rows, F, pitch, off, SENT)
        self.mean, self.rstd = _vec(F=F), _vec(F=F)
        self.rm, self.rv = (_vec(rm), _vec(rv)) if running else (None, None)
        self.dgamma, self.dbeta = _vec(F=F), _vec(F=F)
        hip.bn_act_fwd(self.z, self.gamma, self.beta, self.y, self.mean, self.rstd, EPS, MOM, p,
                       SEED, OFFSET, self.rm, self.rv)

    def backward(self, hip):
        hip.bn_act_bwd(self.dy, self.y, self.z, self.mean, self.rstd, self.gamma, self.scale,
                       self.dz, self.dgamma, self.dbeta)
        torch.cuda.synchronize()

    def eval(self, hip, rm, rv):
        flat, y = _buf(self.rows, self.F, self.y.stride(0), self.y.storage_offset(), SENT)
        hip.bn_act_eval(self.z, self.gamma, self.beta, rm.to(DEV), rv.to(DEV), y, EPS)
        torch.cuda.synchronize()
        assert _intact(flat, y), "the eval kernel wrote outside the rows"
        return y.cpu()

    def out(self):
        F = self.F
        d = dict(y=self.y.cpu(), mean=self.mean[:F].cpu(), rstd=self.rstd[:F].cpu(),
                 dz=self.dz.cpu(), dgamma=self.dgamma[:F].cpu(), dbeta=self.dbeta[:F].cpu())
        if self.rm is not None:
            d.update(running_mean=self.rm[:F].cpu(), running_var=self.rv[:F].cpu())
        return d

    def padding_intact(self):
        F = self.F
        vecs = [self.mean, self.rstd, self.dgamma, self.dbeta] + (
            [self.rm, self.rv] if self.rm is not None else [])
        return (_intact(self.y_flat, self.y) and _intact(self.dz_flat, self.dz) and
                all(bool((v[F:] == SENT).all()) for v in vecs))


def _hold(tag, name, x, r64, r32, bad):
    if float(r64.abs().max()) == 0.0:
        assert float(x.abs().max()) == 0.0, f"{name}: float64 is zero, kernel is not"
        return
    ek, e32 = err(x, r64), err(r32, r64)
    ratio = ek / max(e32, 2.0 ** -30)
    RATIOS[tag + (name,)] = ratio
    bound = yardstick_bound(e32, C)
    print(f"  {name}: err(kernel) {ek:.3e} err(fp32 chain) {e32:.3e} ratio {ratio:.2f} "
          f"bound {bound:.3e}")
    if not ek <= bound:
        bad.append(f"{tag[2]} p={tag[3]} {name}: {ek:.3e} > {bound:.3e}")


@pytest.mark.parametrize("layout,rows", bc.CASES, ids=[f"{l}-rows{r}" for l, r in bc.CASES])
def test_forward_backward_and_eval_within_the_float32_yardstick(hip, layout, rows):
    F, pitch, off = bc.LAYOUTS[layout]
    cc = bc.const_col(F)
    bad = []
    for kind in bc.KINDS:
        t, near, enear, share = bc.pick(layout, rows, kind)
        print(f"{layout} rows {rows} {kind}: excluded share {share:.2e}")
        assert share <= bc.MASK_CAP
        z, gamma, beta, dy, rm, rv = t
        dy = dy.masked_fill(near, 0.0)
        t = (z, gamma, beta, dy, rm, rv)
        for p in bc.PS:
            tag = (layout, rows, kind, p)
            keep, scale = _keep(hip, rows, F, p), 1.0 / (1.0 - p)
            q64, n64 = bc.chain(z, gamma, beta, rm, rv, keep, scale, dy, torch.float64)
            q32, _ = bc.chain(z, gamma, beta, rm, rv, keep, scale, dy, torch.float32)
            run = Run(hip, t, pitch, off, p)
            run.backward(hip)
            got = run.out()
            assert run.padding_intact(), "a write outside the rows"
            # the keep pattern, where the float64 pre-activation is clearly off zero
            sure = n64 > 1e-2
            assert torch.equal((got["y"] > 0)[sure], keep[sure]), "keep pattern differs"
            assert bool((got["y"][n64 < -1e-2] == 0).all())
            if rows == 1:
                assert torch.equal(got["running_mean"], rm) and torch.equal(got["running_var"], rv)
                assert float(got["dz"].abs().max()) == 0.0
            for name in TRAIN_Q:
                x, r64, r32 = got[name], q64[name], q32[name]
                if name == "y":
                    x, r32, r64 = (v.masked_fill(near, 0.0) for v in (x, r32, r64))
                _hold(tag, name, x, r64, r32, bad)
            if kind == "const-col":
                ref =torch.relu(beta[cc]) * keep[:, cc] * np.float32(scale)
                assert torch.equal(got["y"][:, cc], ref.float()), "constant column: y"
                assert float(got["mean"][cc]) == 0.75
                assert float(got["dgamma"][cc]) == 0.0
                e = abs(float(got["rstd"][cc]) * np.sqrt(EPS) - 1.0)
                assert e <= FLOOR, f"constant column: rstd off by {e:.3e}"
                if float(beta[cc]) < 0:
                    assert float(got["dz"][:, cc].abs().max()) == 0.0
        # eval: the running statistics the case started from
        y64, _ = bc.eval_chain(z, gamma, beta, rm, rv, torch.float64)
        y32, _ = bc.eval_chain(z, gamma, beta, rm, rv, torch.float32)
        ye = run.eval(hip, rm, rv)
        _hold((layout, rows, kind, "eval"), "eval_y", ye.masked_fill(enear, 0.0),
              y64.masked_fill(enear, 0.0), y32.masked_fill(enear, 0.0), bad)
    assert not bad, "; ".join(bad)


def test_largest_ratios_summary():
    """prints the largest measured ratio per quantity (runs after the cases above)"""
    for name in TRAIN_Q + ("eval_y",):
        rs = {k: v for k, v in RATIOS.items() if k[4] == name}
        if rs:
            k = max(rs, key=rs.get)
            print(f"largest ratio {name}: {rs[k]:.2f} at {k[:4]}")


@pytest.mark.parametrize("layout,rows", [("F67-s", 601), ("F128-v4", 601), ("F1024-v4", 601),
                                         ("F128-v4", bc.BIG_ROWS)])
def test_two_calls_give_the_same_bytes(hip, layout, rows):
    F, pitch, off = bc.LAYOUTS[layout]
    t = bc.inputs("randn", rows, F, 3)
    outs = []
    for _ in range(2):
        run = Run(hip, t, pitch, off, 0.5)
        run.backward(hip)
        outs.append(run.out())
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


@pytest.mark.parametrize("layout", ["F7", "F128-v4", "F260-v4"])
def test_null_running_statistics_give_the_same_bits(hip, layout):
    F, pitch, off = bc.LAYOUTS[layout]
    t = bc.inputs("randn", 601, F, 4)
    a = Run(hip, t, pitch, off, 0.5)
    b = Run(hip, t, pitch, off, 0.5, running=False)
    torch.cuda.synchronize()
    for k in ("y", "mean", "rstd"):
        assert torch.equal(a.out()[k], b.out()[k]), k
    assert b.padding_intact()


def test_zero_rows(hip):
    F = 64
    gamma, beta = torch.ones(F, device=DEV), torch.zeros(F, device=DEV)
    z = torch.empty(0, F, device=DEV)
    st = {k: torch.full((F,), SENT, device=DEV) for k in ("mean", "rstd", "rm", "rv", "dg", "db")}
    hip.bn_act_fwd(z, gamma, beta, z, st["mean"], st["rstd"], EPS, MOM, 0.5, 1, 2, st["rm"], st["rv"])
    hip.bn_act_eval(z, gamma, beta, st["rm"], st["rv"], z, EPS)
    hip.bn_act_bwd(z, z, z, st["mean"], st["rstd"], gamma, 2.0, z, st["dg"], st["db"])
    torch.cuda.synchronize()
    assert float(st["dg"].abs().max()) == 0.0 and float(st["db"].abs().max()) == 0.0
    for k in ("mean", "rstd", "rm", "rv"):
        assert bool((st[k] == SENT).all()), k


def test_a_wider_row_is_refused_with_nothing_written(hip):
    from nts import _abi
    from nts._abi import ptr
    lib = _abi.lib()
    rows, F = 5, 1028
    z = torch.randn(rows, F, device=DEV)
    gamma, beta = torch.ones(F, device=DEV), torch.zeros(F, device=DEV)
    outs = {k: torch.full(s, SENT, device=DEV)
            for k, s in (("y", (rows, F)), ("mean", (F,)), ("rstd", (F,)), ("rm", (F,)), ("rv", (F,)),
                         ("dz", (rows, F)), ("dgamma", (F,)), ("dbeta", (F,)))}
    rc = lib.nts_hip_bn_act_fwd(hip.h, rows, F, ptr(z), F, ptr(gamma), ptr(beta), EPS, MOM, 0.5, 1, 2,
                                ptr(outs["y"]), F, ptr(outs["mean"]), ptr(outs["rstd"]),
                                ptr(outs["rm"]), ptr(outs["rv"]))
    assert rc == 1  # NTS_ERR_INVALID
    rc = lib.nts_hip_bn_act_eval(hip.h, rows, F, ptr(z), F, ptr(gamma), ptr(beta), ptr(outs["rm"]),
                                 ptr(outs["rv"]), EPS, ptr(outs["y"]), F)
    assert rc == 1
    rc = lib.nts_hip_bn_act_bwd(hip.h, rows, F, ptr(z), F, ptr(z), F, ptr(z), F, ptr(outs["mean"]),
                                ptr(outs["rstd"]), ptr(gamma), 2.0, ptr(outs["dz"]), F,
                                ptr(outs["dgamma"]), ptr(outs["dbeta"]))
    assert rc == 1
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == SENT).all()), k
