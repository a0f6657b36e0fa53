"""The training criterion and the test-set scores on the device (csrc/loss.hip).

``HipLoss``: the reference's ``nn.SmoothL1Loss()`` (train_DSTAGNN_my.py:132, :156-157), Huber,
MAE and MSE with mean reduction, each optionally masked: an entry whose target equals
``null_val`` (NaN: is NaN) contributes neither to the loss nor to the gradient, and the mean is
taken over the entries that remain.  One launch forward, one backward, no host synchronisation.

``ForecastMetrics``: the per-horizon MAE / RMSE / MAPE list of
``predict_and_save_results_mstgcn`` (lib/utils1.py:418-431, lib/metrics.py:6-17) accumulated in
a (P, 4) fp64 table on the device: one launch per batch, one device-to-host copy at the end.

HIP tensors only: there is no CPU fallback.
"""
import math

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib

HIP_ONLY = ("dstagnn_drought_amd: HipLoss / ForecastMetrics run only on the MI355X HIP path; "
            "move the tensors to a 'cuda' (HIP) device. There is no CPU fallback.")

# DSTAGNN_LOSS_* / DSTAGNN_MASK_* (include/dstagnn.h)
LOSS_SMOOTH_L1, LOSS_HUBER, LOSS_MAE, LOSS_MSE = 0, 1, 2, 3
MASK_NONE, MASK_NEQ, MASK_NAN = 0, 1, 2

KINDS = ("smooth_l1", "huber", "mae", "mse", "masked_mae", "masked_mse")
_KIND_CODE = {"smooth_l1": LOSS_SMOOTH_L1, "huber": LOSS_HUBER, "mae": LOSS_MAE, "mse": LOSS_MSE,
              "masked_mae": LOSS_MAE, "masked_mse": LOSS_MSE}


def mask_of(null_val):
    """(mask mode, null value) of a ``null_val`` option: None masks nothing, NaN masks the NaN
    targets, any other number the targets equal to it."""
    if null_val is None:
        return MASK_NONE, 0.0
    null_val = float(null_val)
    return (MASK_NAN, 0.0) if math.isnan(null_val) else (MASK_NEQ, null_val)


class _HipLossFn(torch.autograd.Function):
    """loss_fwd / loss_bwd as one autograd node.  Saved: the two inputs and the forward's two
    doubles (sum, valid count); the backward recomputes the differences."""

    @staticmethod
    def forward(ctx, y, target, kind, param, mask_mode, null_val):
        loss, stat = _lib.load().loss_fwd(y, target, kind, param, mask_mode, null_val)
        ctx.save_for_backward(y, target, stat)
        ctx.cfg = (kind, param, mask_mode, null_val)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        y, target, stat = ctx.saved_tensors
        if gout.dtype != torch.float32 or not gout.is_contiguous():
            gout = gout.float().contiguous()
        dy = _lib.load().loss_bwd(y, target, stat, gout, *ctx.cfg)
        return dy, None, None, None, None, None


class HipLoss(nn.Module):
    """Mean-reduced regression loss in one HIP launch per direction.

    kind: ``smooth_l1`` (``beta``; 0 is ``mae``), ``huber`` (``delta``), ``mae``, ``mse``,
    ``masked_mae``, ``masked_mse``.  The ``masked_*`` names need ``null_val``; a ``null_val``
    given with any other kind masks it the same way (NaN: the NaN targets).  With every entry
    masked the loss and the gradient are 0.

    ``forward(input, target)``: equal shapes (no broadcasting, ValueError), fp32 HIP tensors
    (RuntimeError otherwise), made contiguous if they are not; a 0-dim fp32 tensor.  The target
    takes no gradient (one that requires it raises) and the backward is once-differentiable."""

    def __init__(self, kind="smooth_l1", beta=1.0, delta=1.0, null_val=None):
        super().__init__()
        if kind not in _KIND_CODE:
            raise ValueError(f"HipLoss: unknown kind {kind!r} (one of {', '.join(KINDS)})")
        if kind.startswith("masked_") and null_val is None:
            raise ValueError(f"HipLoss: {kind} needs null_val (the target value that marks a missing entry)")
        param = float(beta) if kind == "smooth_l1" else float(delta) if kind == "huber" else 0.0
        if not param >= 0.0:  # (a NaN fails too)
            raise ValueError(f"HipLoss: invalid beta / delta {param!r}")
        self.kind, self.beta, self.delta, self.null_val = kind, float(beta), float(delta), null_val
        self._cfg = (_KIND_CODE[kind], param) + mask_of(null_val)

    def extra_repr(self):
        return f"kind={self.kind!r}, beta={self.beta}, delta={self.delta}, null_val={self.null_val}"

    def forward(self, input, target):
        if input.shape != target.shape:
            raise ValueError(f"HipLoss: input {tuple(input.shape)} and target {tuple(target.shape)} differ "
                             "(no broadcasting)")
        if not (input.is_cuda and target.is_cuda):
            raise RuntimeError(HIP_ONLY)
        if input.dtype != torch.float32 or target.dtype != torch.float32:
            raise RuntimeError("HipLoss: fp32 tensors only")
        if target.requires_grad:
            raise RuntimeError("HipLoss: the target takes no gradient (detach it)")
        input, target = input.contiguous(), target.contiguous()
        if torch.is_grad_enabled() and input.requires_grad:
            return _HipLossFn.apply(input, target, *self._cfg)
        return _lib.load().loss_fwd(input, target, *self._cfg)[0]  # nothing saved


class ForecastMetrics:
    """Running per-horizon scores of (S, N, P) predictions against their targets.

    ``update(pred, target)``: one launch, no sync.  ``compute()``: one device-to-host copy; the
    list ``predict_and_save_results_mstgcn`` returns, ``[MAE_0, RMSE_0, MAPE_0, ..., MAE_all,
    RMSE_all, MAPE_all]`` as Python floats: MAE_p = sum |e| / (S N), RMSE_p = sqrt(sum e^2 /
    (S N)), MAPE_p = 100 sum |e / t| / count over the targets != ``null_val`` (0 where there is
    none, as masked_mape_np gives); the overall three from the column sums.  ``reset()`` clears."""

    def __init__(self, num_for_predict, null_val=0.0, device=None):
        self.P = int(num_for_predict)
        if not 1 <= self.P <= 256:
            raise ValueError(f"ForecastMetrics: num_for_predict must be in [1, 256], got {num_for_predict!r}")
        self.null_val = float(null_val)
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(HIP_ONLY)
        self.table = torch.zeros(self.P, 4, dtype=torch.float64, device=device)
        self.rows = 0

    def reset(self):
        self.table.zero_()
        self.rows = 0

    def update(self, pred, target):
        if pred.shape != target.shape or pred.dim() < 1 or pred.shape[-1] != self.P:
            raise ValueError(f"ForecastMetrics: pred {tuple(pred.shape)} / target {tuple(target.shape)} must be "
                             f"equal (..., {self.P}) shapes")
        if not (pred.is_cuda and target.is_cuda):
            raise RuntimeError(HIP_ONLY)
        if pred.numel() == 0:
            return
        _lib.load().metrics_update(pred.detach().contiguous(), target.detach().contiguous(), self.null_val,
                                   self.table)
        self.rows += pred.numel() // self.P

    def compute(self):
        tab = self.table.cpu().numpy()  # the one copy (and the one sync)
        rows = max(self.rows, 1)

        def three(abs_sum, sq_sum, ape_sum, count, n):
            return [float(abs_sum / n), float(math.sqrt(sq_sum / n)),
                    float(100.0 * ape_sum / count) if count > 0 else 0.0]
        out = []
        for p in range(self.P):
            out.extend(three(*tab[p], rows))
        out.extend(three(*tab.sum(0), rows * self.P))
        return out
