"""The fused LayerNorm + relu + dropout kernels (csrc/norm.hip) through the C-ABI.

Shapes.  rows 1, 3, 5 (below, at and across one block's four waves) and 601
(38 backward blocks of 16 rows, the last one ragged: the dgamma / dbeta
reduction sums several partials); F 1, 7, 64, 67, 128, 260, 1024 (every
instantiation of both paths), F = 128 again with pitch 130 and with a base 4
bytes off (both force the scalar path), and F = 1028, which must be refused
with nothing written.

Inputs.  z = randn; z = 1e4 + randn (a one-pass variance loses everything
here); a constant row (variance 0: y = dropout(relu(beta)), rstd = 1/sqrt(eps)).

Bound.  The project's rule (tests/step_check.py): for every quantity q of
(y, mean, rstd, dz, dgamma, dbeta), err(kernel) <= C err(float32 torch chain) +
FLOOR against float64 autograd through layer_norm -> relu -> mask, err(x) =
max|x - q64| / max|q64|.  A quantity whose float64 value is identically zero
(dz and dgamma at F = 1, where z - mean = 0) must be exactly zero.  Every ratio
is printed (the table is in DESIGN §8l).

Elements whose float64 pre-activation lies within 1e-4 of zero are left out of
the y comparison and get a zero incoming gradient (the relu gate may flip
there); their share is asserted <= 1e-3.  The constant-row case leaves out
nothing.

Every row operand sits in an allocation with a pitch wider than F and extra
rows: input padding is NaN, output padding a sentinel that must survive.
"""
import numpy as np
import pytest
import torch

from step_check import C, FLOOR, err, yardstick_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -12345.5
EPS = 1e-5
MASK_EPS, MASK_CAP = 1e-4, 1e-3
SEED, OFFSET = 0x1234567, 5
ROWS = [1, 3, 5, 601]
# id: (F, pitch, base offset in floats)
LAYOUTS = {
    "F1": (1, 3, 0),
    "F7": (7, 10, 0),
    "F64-v4n1": (64, 68, 0),
    "F67-s4": (67, 70, 0),
    "F128-v4n1": (128, 132, 0),
    "F260-v4n2": (260, 264, 0),
    "F1024-v4n4": (1024, 1028, 0),
    "F128-pitch130-s4": (128, 130, 0),
    "F128-base+4B-s4": (128, 132, 1),
}
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


def _intact(flat, view):
    """everything of the allocation but the view still holds the sentinel"""
    return int((flat == SENT).sum()) - int((view == SENT).sum()) == flat.numel() - view.numel()


def _keep(hip, rows, F, p):
    """the keep pattern of nts_hip_relu_dropout_f32 for (SEED, OFFSET)"""
    if p == 0:
        return torch.ones(rows, F, dtype=torch.bool)
    y = torch.empty(rows, F, device=DEV)
    hip.relu_dropout(torch.ones(rows, F, device=DEV), y, p, SEED, OFFSET)
    return (y > 0).cpu()


def _chain(z, gamma, beta, keep, scale, dy, dtype):
    """layer_norm -> relu -> mask in `dtype` with autograd; returns the dict of
    quantities and the pre-activation"""
    z = z.to(dtype).requires_grad_()
    g, b = gamma.to(dtype).requires_grad_(), beta.to(dtype).requires_grad_()
    n, mean, rstd = torch.native_layer_norm(z, (z.shape[1],), g, b, EPS)
    y = torch.relu(n) * keep.to(dtype) * scale
    y.backward(dy.to(dtype))
    return dict(y=y.detach(), mean=mean.detach().flatten(), rstd=rstd.detach().flatten(),
                dz=z.grad, dgamma=g.grad, dbeta=b.grad), n.detach()


class Run:
    def __init__(self, hip, z, gamma, beta, dy, pitch, off, p, stats=True):
        rows, F = z.shape
        self.z, self.dy = _in(z, pitch, off), _in(dy, pitch, off)
        self.gamma, self.beta = gamma.to(DEV), beta.to(DEV)
        self.y_flat, self.y = _buf(rows, F, pitch, off, SENT)
        self.dz_flat, self.dz = _buf(rows, F, pitch, off, SENT)
        self.mean = torch.full((rows + 2,), SENT, device=DEV) if stats else None
        self.rstd = torch.full((rows + 2,), SENT, device=DEV) if stats else None
        self.dgamma = torch.full((F + 2,), SENT, device=DEV)
        self.dbeta = torch.full((F + 2,), SENT, device=DEV)
        self.rows, self.F, self.scale = rows, F, 1.0 / (1.0 - p)
        hip.ln_act_fwd(self.z, self.gamma, self.beta, self.y, EPS, p, SEED, OFFSET, self.mean,
                       self.rstd)

    def backward(self, hip):
        hip.ln_act_bwd(self.dy, self.y, self.z, self.mean, self.rstd, self.gamma, self.scale,
                       self.dz, self.dgamma, self.dbeta)
        torch.cuda.synchronize()

    def out(self):
        r, F = self.rows, self.F
        return dict(y=self.y.cpu(), mean=self.mean[:r].cpu(), rstd=self.rstd[:r].cpu(),
                    dz=self.dz.cpu(), dgamma=self.dgamma[:F].cpu(), dbeta=self.dbeta[:F].cpu())

    def padding_intact(self):
        r, F = self.rows, self.F
        return (_intact(self.y_flat, self.y) and _intact(self.dz_flat, self.dz) and
                bool((self.mean[r:] == SENT).all()) and bool((self.rstd[r:] == SENT).all()) and
                bool((self.dgamma[F:] == SENT).all()) and bool((self.dbeta[F:] == SENT).all()))


def _inputs(kind, rows, F, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, F, generator=g)
    if kind == "offset1e4":
        z = z + 1e4
    gamma = 1 + 0.1 * torch.randn(F, generator=g)
    beta = 0.1 * torch.randn(F, generator=g)
    dy = torch.randn(rows, F, generator=g)
    return z, gamma, beta, dy


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_forward_and_backward_within_the_float32_yardstick(hip, layout, rows):
    F, pitch, off = LAYOUTS[layout]
    bad = []
    for kind in ("randn", "offset1e4"):
        for p in (0.0, 0.5):
            keep = _keep(hip, rows, F, p)
            scale = 1.0 / (1.0 - p)
            # in a small case one element near zero is already past the cap: the
            # inputs are the first of a few seeds whose float64 chain has none
            # too many (the reference alone decides, as for tests/test_max_driver.py)
            for k in range(8):
                z, gamma, beta, dy = _inputs(kind, rows, F, 100 * F + rows + 7919 * k)
                _, n64 = _chain(z, gamma, beta, keep, scale, dy, torch.float64)
                near = n64.abs() < MASK_EPS
                share = float(near.double().mean())
                if share <= MASK_CAP:
                    break
            print(f"{layout} rows {rows} {kind} p {p}: excluded share {share:.2e}")
            assert share <= MASK_CAP
            dy = dy.masked_fill(near, 0.0)
            q64, _ = _chain(z, gamma, beta, keep, scale, dy, torch.float64)
            q32, n32 = _chain(z, gamma, beta, keep, scale, dy, torch.float32)
            run = Run(hip, z, gamma, beta, dy, pitch, off, p)
            run.backward(hip)
            got = run.out()
            assert run.padding_intact(), "a write outside the rows"
            # the zero pattern: the reference kernel's mask on the float32 chain's n
            if p > 0:
                ref = torch.empty(rows, F, device=DEV)
                hip.relu_dropout(n32.to(DEV), ref, p, SEED, OFFSET)
                # (1e4 + randn: float32 torch's n is only good to ~1e-3 there; where
                # its sign is already wrong against float64 it is no reference)
                same = ((got["y"] == 0) == (ref.cpu() == 0)) | near | (n32.double() * n64 <= 0)
                assert bool(same.all()), "zero pattern differs from nts_hip_relu_dropout_f32"
                kept = (got["y"] > 0) & ~near
                torch.testing.assert_close(got["y"][kept].double(),
                                           (torch.relu(n64) * scale)[kept], rtol=1e-3, atol=1e-3)
            for name in ("y", "mean", "rstd", "dz", "dgamma", "dbeta"):
                x, r64, r32 = got[name], q64[name], q32[name]
                if name == "y":
                    x, r32 = x.masked_fill(near, 0.0), r32.masked_fill(near, 0.0)
                    r64 = r64.masked_fill(near, 0.0)
                if float(r64.abs().max()) == 0.0:
                    assert float(x.abs().max()) == 0.0, f"{name}: float64 is zero, kernel is not"
                    continue
                ek, e32 = err(x, r64), err(r32, r64)
                ratio = ek / max(e32, 2.0 ** -30)
                RATIOS[(layout, rows, kind, p, name)] = ratio
                bound = yardstick_bound(e32, C)
                print(f"  {name}: err(kernel) {ek:.3e} err(fp32 chain) {e32:.3e} ratio {ratio:.2f} "
                      f"bound {bound:.3e}")
                if not ek <= bound:
                    bad.append(f"{kind} p={p} {name}: {ek:.3e} > {bound:.3e}")
    assert not bad, "; ".join(bad)


def test_largest_ratios_summary():
    """prints the largest measured ratio per quantity (runs after the cases above)"""
    for name in ("y", "mean", "rstd", "dz", "dgamma", "dbeta"):
        rs = {k: v for k, v in RATIOS.items() if k[4] == name}
        if rs:
            k = max(rs, key=rs.get)
            print(f"largest ratio {name}: {rs[k]:.2f} at {k[:4]}")


@pytest.mark.parametrize("rows", [1, 5, 601])
@pytest.mark.parametrize("layout", ["F7", "F128-v4n1", "F128-pitch130-s4", "F1024-v4n4"])
def test_constant_row_gives_the_activation_of_beta(hip, layout, rows):
    F, pitch, off = LAYOUTS[layout]
    g = torch.Generator().manual_seed(7 * F + rows)
    b = 0.1 * torch.randn(F, generator=g)
    beta = torch.where(b < 0, b - 0.01, b + 0.01)  # |beta| >= 0.01
    gamma = 1 + 0.1 * torch.randn(F, generator=g)
    z = torch.full((rows, F), 0.75)
    dy = torch.randn(rows, F, generator=g)
    for p in (0.0, 0.5):
        run = Run(hip, z, gamma, beta, dy, pitch, off, p)
        run.backward(hip)
        want = torch.empty(rows, F, device=DEV)
        hip.relu_dropout(beta.to(DEV).expand(rows, F).contiguous(), want, p, SEED, OFFSET)
        assert torch.equal(run.y, want)
        rstd = run.rstd[:rows].cpu().double()
        assert bool(torch.isfinite(rstd).all())
        e = float((rstd - 1.0 / np.sqrt(EPS)).abs().max()) * np.sqrt(EPS)
        print(f"{layout} rows {rows} p {p}: rstd rel. error {e:.3e}")
        assert e <= FLOOR
        assert torch.equal(run.mean[:rows].cpu(), torch.full((rows,), 0.75))
        for t in (run.dz, run.dgamma[:F], run.dbeta[:F]):
            assert bool(torch.isfinite(t).all())
        assert run.padding_intact()


@pytest.mark.parametrize("layout", ["F67-s4", "F128-v4n1", "F1024-v4n4"])
def test_backward_is_bit_identical_from_run_to_run(hip, layout):
    F, pitch, off = LAYOUTS[layout]
    z, gamma, beta, dy = _inputs("randn", 601, F, 3)
    run = Run(hip, z, gamma, beta, dy, pitch, off, 0.5)
    run.backward(hip)
    first = [t.clone() for t in (run.dz, run.dgamma, run.dbeta)]
    for t in (run.dz_flat, run.dgamma, run.dbeta):
        t.fill_(SENT)
    run.backward(hip)
    for a, b in zip(first, (run.dz, run.dgamma, run.dbeta)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("layout", ["F7", "F128-v4n1", "F260-v4n2"])
def test_null_stats_give_the_same_bits(hip, layout):
    F, pitch, off = LAYOUTS[layout]
    z, gamma, beta, dy = _inputs("randn", 601, F, 4)
    a = Run(hip, z, gamma, beta, dy, pitch, off, 0.5)
    b = Run(hip, z, gamma, beta, dy, pitch, off, 0.5, stats=False)
    torch.cuda.synchronize()
    assert torch.equal(a.y, b.y)
    assert _intact(b.y_flat, b.y)


def test_zero_rows(hip):
    F = 64
    gamma, beta = torch.ones(F, device=DEV), torch.zeros(F, device=DEV)
    z = torch.empty(0, F, device=DEV)
    hip.ln_act_fwd(z, gamma, beta, z, EPS, 0.0, 0, 0)
    dg, db = torch.full((F,), SENT, device=DEV), torch.full((F,), SENT, device=DEV)
    e = torch.empty(0, device=DEV)
    hip.ln_act_bwd(z, z, z, e, e, gamma, 1.0, z, dg, db)
    assert float(dg.abs().max()) == 0.0 and float(db.abs().max()) == 0.0


def test_a_wider_row_is_refused_with_nothing_written(hip):
    from nts import _abi
    from nts._abi import ptr
    lib = _abi.lib()
    rows, F = 5, 1028
    z = torch.randn(rows, F, device=DEV)
    gamma, beta = torch.ones(F, device=DEV), torch.zeros(F, device=DEV)
    outs = {k: torch.full(s, SENT, device=DEV)
            for k, s in (("y", (rows, F)), ("mean", (rows,)), ("rstd", (rows,)), ("dz", (rows, F)),
                         ("dgamma", (F,)), ("dbeta", (F,)))}
    rc = lib.nts_hip_ln_act_fwd(hip.h, rows, F, ptr(z), F, ptr(gamma), ptr(beta), EPS, 0.5, 1, 2,
                                ptr(outs["y"]), F, ptr(outs["mean"]), ptr(outs["rstd"]))
    assert rc == 1  # NTS_ERR_INVALID
    rc = lib.nts_hip_ln_act_bwd(hip.h, rows, F, ptr(z), F, ptr(z), F, ptr(z), F, ptr(outs["mean"]),
                                ptr(outs["rstd"]), ptr(gamma), 2.0, ptr(outs["dz"]), F,
                                ptr(outs["dgamma"]), ptr(outs["dbeta"]))
    assert rc == 1
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == SENT).all()), k
