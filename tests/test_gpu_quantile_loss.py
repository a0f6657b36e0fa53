"""GPU: the pinball criterion (csrc/loss.hip pinball_fwd_kernel / pinball_bwd_kernel; QuantileLoss)
against a float64 numpy restatement on the same fp32 inputs, tau and 1 - tau taken as the fp32
values the kernels hold.

Inputs are seeded: t = 3 randn, y_q = t + randn + offset_q (offsets spread over [-1, 1]), 3 % of the
predictions set equal to their target (d = 0), 30 % of the targets marked (-9999 for the != mode,
NaN for the NaN mode, none under the no-mask mode).

Bounds (derived as DESIGN §11.3 derives the criterion's; none of them measured):
  loss  <= 1e-6 relative: every term is non-negative and carries at most three fp32 roundings (d,
        the 1 - tau constant, the product: 3 * 2^-24 = 1.8e-7), every add is fp64, and the final
        fp32 cast adds 2^-24.
  dy    <= 1e-6 |dy| elementwise: the 1 - tau constant, the fp32 cast of gout / (count Q) and the
        product, 3 * 2^-24.  Exactly 0 (all bits) at masked entries and where d = 0.

Measured on the MI355X, worst over the cases below: loss 4.5e-8, dy 7.1e-8.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
REL = 1e-6
MODES = {"none": None, "neq": -9999.0, "nan": NAN}
TILE = 4096  # dstagnn_loss_tile_elems()

# (M, Q)
CASES = {
    "1x1": (1, 1),
    "1x16": (1, 16),
    "37x3": (37, 3),
    "1025x4-one-whole-tile-one-partial": (TILE // 4 + 1, 4),
    "65280x3-pems08-head": (65280, 3),
    "999x7-load-straddles-entries": (999, 7),
    "1049602x4-over-1024-tiles": (1025 * TILE // 4 + 2, 4),
}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def levels_of(Q):
    return tuple((q + 1.0) / (Q + 1.0) for q in range(Q))


def _valid(t, marker):
    if marker is None:
        return np.ones(t.shape, dtype=bool)
    return ~np.isnan(t) if marker != marker else t != np.float32(marker)


@functools.lru_cache(maxsize=None)
def _inputs(M, Q, mode, seed=0):
    """(y (M, Q), t (M)) fp32 numpy arrays, made once and shared (never modified)."""
    marker = MODES[mode]
    g = torch.Generator().manual_seed(4000 + 7 * M + Q + seed)
    t = 3.0 * torch.randn(M, generator=g)
    off = torch.linspace(-1.0, 1.0, Q) if Q > 1 else torch.zeros(1)
    y = t[:, None] + torch.randn(M, Q, generator=g) + off
    if M > 1:
        same = torch.rand(M, Q, generator=g) < 0.03
        y = torch.where(same, t[:, None].expand(M, Q), y)
        if marker is not None:
            t = torch.where(torch.rand(M, generator=g) < 0.3, torch.tensor(marker), t)
    return y.numpy(), t.numpy()


def restate(y, t, levels, marker, gout=1.0):
    """float64 loss and gradient; the fp32 tau and 1 - tau."""
    tau32 = np.asarray(levels, dtype=np.float32)
    tau, omt = tau32.astype(np.float64), (np.float32(1.0) - tau32).astype(np.float64)
    v = _valid(t, marker)
    Q = y.shape[-1]
    d = y.astype(np.float64) - np.where(v, t, 0.0).astype(np.float64)[..., None]
    term = np.where(d > 0, omt * d, np.where(d < 0, tau * -d, 0.0))
    slope = np.where(d > 0, omt, np.where(d < 0, -tau, 0.0)) * np.ones_like(d)
    cnt = int(v.sum())
    if cnt == 0:
        return 0.0, np.zeros_like(d), v, d
    loss = term[v].sum() / (cnt * Q)
    grad = np.where(v[..., None], slope * (gout / (cnt * Q)), 0.0)
    return loss, grad, v, d


def run_hip(y, t, levels, marker, scale=None):
    from dstagnn_drought_amd import QuantileLoss
    crit = QuantileLoss(levels, null_val=marker)
    yg = (y if torch.is_tensor(y) else torch.from_numpy(y).cuda()).detach().requires_grad_(True)
    tg = t if torch.is_tensor(t) else torch.from_numpy(t).cuda()
    loss = crit(yg, tg)
    (loss if scale is None else loss * scale).backward()
    return loss.detach(), yg.grad


def check(case, y, t, levels, marker, loss, grad, gout=1.0):
    want, gwant, v, d = restate(y, t, levels, marker, gout)
    got, g = float(loss.double().cpu()), grad.double().cpu().numpy()
    err = abs(got - want) / max(abs(want), 1e-300)
    gerr = float(np.max(np.abs(g - gwant) / np.where(gwant != 0, np.abs(gwant), 1.0)))
    print(f"{case}: loss {got!r} want {want!r} rel {err:.2e}; dy worst rel {gerr:.2e}")
    assert err <= REL or got == want, f"{case}: loss {got!r} vs {want!r}"
    assert np.all(np.abs(g - gwant) <= REL * np.abs(gwant)), f"{case}: dy worst relative error {gerr:.3e}"
    bits = grad.cpu().numpy().view(np.int32)
    zero = ~v[..., None] | (d == 0)
    assert not bits[np.broadcast_to(zero, bits.shape)].any(), f"{case}: a masked or d = 0 entry is not all-bits zero"
    if y.size > 10000:
        assert (d == 0)[v].any()  # the d = 0 row is exercised


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("case", list(CASES))
def test_loss_and_gradient_vs_float64(case, mode):
    _need_gpu()
    M, Q = CASES[case]
    y, t = _inputs(M, Q, mode)
    loss, grad = run_hip(y, t, levels_of(Q), MODES[mode])
    assert loss.dtype == torch.float32 and loss.dim() == 0 and grad.shape == (M, Q)
    check(f"{case}/{mode}", y, t, levels_of(Q), MODES[mode], loss, grad)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_unaligned_slice_takes_the_scalar_path(mode):
    """y[1:] of an (M + 1, 3) tensor starts 12 bytes in: no 16-byte loads although a tile is whole."""
    _need_gpu()
    M, Q = 2000, 3
    y, t = _inputs(M + 1, Q, mode, seed=1)
    yd, td = torch.from_numpy(y).cuda()[1:], torch.from_numpy(t).cuda()[1:]
    assert yd.data_ptr() % 16 != 0 and yd.is_contiguous() and yd.numel() > TILE
    loss, grad = run_hip(yd, td, levels_of(Q), MODES[mode])
    check(f"slice/{mode}", y[1:], t[1:], levels_of(Q), MODES[mode], loss, grad)


def test_all_masked_gives_zero_loss_and_gradient():
    _need_gpu()
    y, _ = _inputs(37, 3, "none")
    for marker in (NAN, -9999.0):
        t = np.full(37, marker, dtype=np.float32)
        loss, grad = run_hip(y, t, levels_of(3), marker)
        assert float(loss) == 0.0 and not grad.cpu().numpy().view(np.int32).any()


def test_nan_prediction():
    _need_gpu()
    y, t = _inputs(999, 7, "nan")
    v = _valid(t, NAN)
    bad = y.copy()
    bad[np.flatnonzero(v)[3], 2] = NAN  # at a valid entry: the loss is NaN
    loss, _ = run_hip(bad, t, levels_of(7), NAN)
    assert np.isnan(float(loss))
    ok = y.copy()
    ok[np.flatnonzero(~v)[3], :] = NAN  # at a masked entry: selected out
    loss, grad = run_hip(ok, t, levels_of(7), NAN)
    check("nan-at-masked", y, t, levels_of(7), NAN, loss, grad)


def test_two_launches_give_the_same_bits_and_no_grad_saves_nothing():
    _need_gpu()
    from dstagnn_drought_amd import QuantileLoss
    y, t = _inputs(65280, 3, "nan")
    a, ga = run_hip(y, t, levels_of(3), NAN)
    b, gb = run_hip(y, t, levels_of(3), NAN)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ga, gb)
    crit = QuantileLoss(levels_of(3), null_val=NAN)
    yd, td = torch.from_numpy(y).cuda().requires_grad_(True), torch.from_numpy(t).cuda()
    with torch.no_grad():
        c = crit(yd, td)
    assert c.grad_fn is None and torch.equal(a.view(torch.int32), c.view(torch.int32))
    assert crit(yd.detach(), td).grad_fn is None
    with pytest.raises(RuntimeError):
        crit(yd, td.clone().requires_grad_(True))
    with pytest.raises(RuntimeError):
        crit(yd.double(), td.double())
    # a non-contiguous prediction is made contiguous
    yt = torch.from_numpy(np.ascontiguousarray(y.T)).cuda().t()
    assert not yt.is_contiguous()
    assert torch.equal(crit(yt, td).view(torch.int32), a.view(torch.int32))


def test_median_is_half_the_mae():
    _need_gpu()
    from dstagnn_drought_amd import HipLoss
    for mode in sorted(MODES):
        y, t = _inputs(65280, 1, mode)
        loss, grad = run_hip(y, t, (0.5,), MODES[mode])
        yd, td = torch.from_numpy(y[:, 0].copy()).cuda().requires_grad_(True), torch.from_numpy(t).cuda()
        mae = HipLoss("mae", null_val=MODES[mode])(yd, td)
        mae.backward()
        half, ghalf = 0.5 * float(mae.detach().double()), 0.5 * yd.grad.double().cpu().numpy()
        assert abs(float(loss.double()) - half) <= REL * half
        g = grad.double().cpu().numpy()[:, 0]
        assert np.all(np.abs(g - ghalf) <= REL * np.abs(ghalf))


def test_upstream_gradient_is_honoured():
    _need_gpu()
    y, t = _inputs(999, 7, "neq")
    loss, grad = run_hip(y, t, levels_of(7), -9999.0, scale=3.0)
    check("gout3", y, t, levels_of(7), -9999.0, loss, grad, gout=3.0)
    _, g1 = run_hip(y, t, levels_of(7), -9999.0)
    assert float((grad - 3.0 * g1).abs().max()) <= 3e-7 * float(grad.abs().max())
