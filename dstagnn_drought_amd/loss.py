"""The training criterion and the test-set scores on the device (csrc/loss.hip).

``HipLoss``: the reference's ``nn.SmoothL1Loss()`` (train_DSTAGNN_my.py:132, :156-157), Huber,
MAE and MSE with mean reduction, each optionally masked: an entry whose target equals
``null_val`` (NaN: is NaN) contributes neither to the loss nor to the gradient, and the mean is
taken over the entries that remain.  One launch forward, one backward, no host synchronisation.

``ForecastMetrics``: the per-horizon MAE / RMSE / MAPE list of
``predict_and_save_results_mstgcn`` (lib/utils1.py:418-431, lib/metrics.py:6-17) accumulated in
a (P, 4) fp64 table on the device: one launch per batch, one device-to-host copy at the end.
With a missing value and / or a node count: the masked (P, 8) and (N, 8) tables of
``metrics_masked_kernel``, which also give the bias, the Nash-Sutcliffe skill and per-node scores.

``QuantileLoss`` / ``QuantileMetrics``: the pinball criterion of a (..., P, Q) quantile forecast and
its calibration scores (coverage, pinball, interval width, crossing rate), on the same kernels' plan.

``BaselineSkill``: the skill of a forecast over persistence and over the seasonal climatology, and
the anomaly correlation, both baselines read out of a ``WindowedSeries``' raw series inside the
scoring launch (``skill_kernel``, csrc/windows.hip ``climatology_kernel``).

``EventScores``: the class contingency tables of a forecast against drought thresholds (fixed, or
per node from ``node_percentile_thresholds``) and the categorical scores read from them (POD, FAR,
CSI, frequency bias, Heidke and Gilbert skill, the class confusion matrix), per horizon and per node
(``events_kernel``).

HIP tensors only: there is no CPU fallback.
"""
import math

import numpy as np
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


class _RunningTables:
    """What ``ForecastMetrics`` and ``QuantileMetrics`` share: the checked horizon and node counts,
    the device, the mask of ``missing_value``, the running fp64 tables (``table`` (P, cols) and
    ``node_table`` (num_nodes, cols) or None) and their reset / merge / all-reduce.  A subclass
    supplies ``scores_of_table`` and ``_config()``."""

    def _check_horizon(self, num_for_predict):
        self.P = int(num_for_predict)
        if not 1 <= self.P <= 256:
            raise ValueError(f"{type(self).__name__}: num_for_predict must be in [1, 256], got {num_for_predict!r}")

    def _init_tables(self, cols, device, missing_value, num_nodes):
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(HIP_ONLY)
        self.missing_value = None if missing_value is None else float(missing_value)
        self.num_nodes = None if num_nodes is None else int(num_nodes)
        if self.num_nodes is not None and self.num_nodes < 1:
            raise ValueError(f"{type(self).__name__}: num_nodes must be >= 1, got {num_nodes!r}")
        self._mask = mask_of(missing_value)
        self.table = torch.zeros(self.P, cols, dtype=torch.float64, device=device)
        self.node_table = (None if self.num_nodes is None else
                           torch.zeros(self.num_nodes, cols, dtype=torch.float64, device=device))

    def _check_nodes(self, pred, axis):
        if self.num_nodes is not None and pred.shape[axis] != self.num_nodes:
            raise ValueError(f"{type(self).__name__}: pred {tuple(pred.shape)} has {pred.shape[axis]} nodes, "
                             f"num_nodes is {self.num_nodes}")

    def reset(self):
        self.table.zero_()
        if self.node_table is not None:
            self.node_table.zero_()

    def node_scores(self):
        if self.node_table is None:
            raise ValueError(f"{type(self).__name__}: node_scores() needs num_nodes")
        return self.scores_of_table(self.node_table.cpu().numpy(), overall=False)

    def merge(self, other):
        """Adds ``other``'s tables into this object's (the sums are additive)."""
        if not isinstance(other, type(self)) or other._config() != self._config():
            raise ValueError(f"{type(self).__name__}.merge: the other object has a different configuration")
        self.table += other.table.to(self.table.device)
        if self.node_table is not None:
            self.node_table += other.node_table.to(self.node_table.device)
        return self

    def all_reduce(self):
        """One SUM all-reduce per table when a process group is up; nothing otherwise."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.table)
            if self.node_table is not None:
                dist.all_reduce(self.node_table)
        return self


class ForecastMetrics(_RunningTables):
    """Running per-horizon scores of (S, N, P) predictions against their targets.

    ``update(pred, target)``: one launch, no sync.  ``compute()``: one device-to-host copy; the
    list ``predict_and_save_results_mstgcn`` returns, ``[MAE_0, RMSE_0, MAPE_0, ..., MAE_all,
    RMSE_all, MAPE_all]`` as Python floats: MAE_p = sum |e| / (S N), RMSE_p = sqrt(sum e^2 /
    (S N)), MAPE_p = 100 sum |e / t| / count over the targets != ``null_val`` (0 where there is
    none, as masked_mape_np gives); the overall three from the column sums.  ``reset()`` clears.

    Series with gaps, per-node scores.  ``missing_value`` (a number, or NaN for the NaN targets:
    ``mask_of``) leaves the targets equal to it out of every sum, as ``HipLoss(null_val=)`` leaves
    them out of the loss; ``num_nodes`` adds ``node_table``, the same sums per node over all
    samples and horizons.  Either one switches the object to ``metrics_masked_kernel``: ``table``
    is then (P, 8) (count, sum e, sum |e|, sum e^2, sum |e / t| over t != ``null_val``, its count,
    sum t, sum t^2 over the valid entries), ``node_table`` (num_nodes, 8) or None, the divisors of
    ``compute()`` are the valid counts, and MAE / RMSE are NaN where a horizon has no valid entry
    (MAPE stays 0.0 where its own count is 0).  With neither keyword the object is the (P, 4) one
    above, untouched.

    ``scores()``: a dict of float64 arrays of shape (P + 1,), the overall value last: ``count``,
    ``mae``, ``rmse``, ``mape`` and, from the eight-column table, ``bias`` (sum e / count) and
    ``nse`` (1 - sum e^2 / (sum t^2 - (sum t)^2 / count)); NaN wherever a divisor is 0.
    ``node_scores()``: the same keys in shape (num_nodes,).  ``merge(other)`` adds another
    object's tables; ``all_reduce()`` sums them over the ranks of the process group."""

    def __init__(self, num_for_predict, null_val=0.0, device=None, *, missing_value=None, num_nodes=None):
        self._check_horizon(num_for_predict)
        self.null_val = float(null_val)
        self.masked = missing_value is not None or num_nodes is not None
        self._init_tables(8 if self.masked else 4, device, missing_value, num_nodes)
        self.rows = 0

    def reset(self):
        super().reset()
        self.rows = 0

    def update(self, pred, target):
        if self.masked:
            return self._update_masked(pred, target)
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

    def _update_masked(self, pred, target):
        if pred.shape != target.shape or pred.dim() < 2 or pred.shape[-1] != self.P:
            raise ValueError(f"ForecastMetrics: pred {tuple(pred.shape)} / target {tuple(target.shape)} must be "
                             f"equal (..., N, {self.P}) shapes")
        self._check_nodes(pred, -2)
        if not (pred.is_cuda and target.is_cuda):
            raise RuntimeError(HIP_ONLY)
        if pred.numel() == 0:
            return
        _lib.load().metrics_update_masked(pred.detach().contiguous(), target.detach().contiguous(), self._mask[0],
                                          self._mask[1], self.null_val, self.table, self.node_table)
        self.rows += pred.numel() // self.P

    def compute(self):
        if self.masked:
            return self.list_of_table(self.table.cpu().numpy())
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

    @staticmethod
    def list_of_table(table):
        """``compute()``'s list from a (K, 8) table of the masked sums (a numpy array): three
        entries per row, then the three of the column sums.  MAE / RMSE NaN at a zero count, MAPE
        0.0 at a zero count of its own."""
        tab = np.asarray(table, dtype=np.float64).reshape(-1, 8)

        def three(r):
            n = r[0]
            return [float(r[2] / n) if n > 0 else float("nan"),
                    float(math.sqrt(r[3] / n)) if n > 0 else float("nan"),
                    float(100.0 * r[4] / r[5]) if r[5] > 0 else 0.0]
        out = []
        for r in tab:
            out.extend(three(r))
        out.extend(three(tab.sum(0)))
        return out

    @staticmethod
    def scores_of_table(table, rows=None, overall=True):
        """The scores of a table of sums (a numpy array), one entry per row and, with ``overall``,
        one more from the column sums.  (K, 8): the masked sums; count, mae, rmse, mape, bias,
        nse.  (K, 4): the unmasked object's columns with ``rows`` entries behind each row; count,
        mae, rmse, mape.  NaN wherever a divisor is 0."""
        tab = np.asarray(table, dtype=np.float64)
        if tab.ndim != 2 or tab.shape[1] not in (4, 8):
            raise ValueError(f"ForecastMetrics: a table of sums is (K, 4) or (K, 8), got {tab.shape}")
        if overall:
            tab = np.concatenate([tab, tab.sum(0, keepdims=True)], 0)

        def over(a, b):
            out = np.full(a.shape, np.nan)
            np.divide(a, b, out=out, where=b != 0)
            return out
        if tab.shape[1] == 4:
            count = np.full(tab.shape[0], float(rows or 0))
            if overall:
                count[-1] *= tab.shape[0] - 1
            return {"count": count, "mae": over(tab[:, 0], count), "rmse": np.sqrt(over(tab[:, 1], count)),
                    "mape": 100.0 * over(tab[:, 2], tab[:, 3])}
        count = tab[:, 0].copy()
        var = tab[:, 7] - over(tab[:, 6] * tab[:, 6], count)  # NaN at a zero count
        return {"count": count, "mae": over(tab[:, 2], count), "rmse": np.sqrt(over(tab[:, 3], count)),
                "mape": 100.0 * over(tab[:, 4], tab[:, 5]), "bias": over(tab[:, 1], count),
                "nse": 1.0 - over(tab[:, 3], np.where(np.isnan(var), 0.0, var))}

    def scores(self):
        return self.scores_of_table(self.table.cpu().numpy(), self.rows)

    def _config(self):
        return (self.P, repr(self.null_val), self.masked, self._mask[0], repr(self._mask[1]), self.num_nodes)

    def merge(self, other):
        """Adds ``other``'s tables and row count into this object's (the sums are additive)."""
        super().merge(other)
        self.rows += other.rows
        return self

    def all_reduce(self):
        """One SUM all-reduce per table (and one of the row count) when a process group is up;
        nothing otherwise."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            super().all_reduce()
            rows = torch.tensor([self.rows], dtype=torch.int64, device=self.table.device)
            dist.all_reduce(rows)
            self.rows = int(rows.item())
        return self


# ---- quantile forecasts ------------------------------------------------------------------------
MAX_QUANTILES = 16  # include/dstagnn.h DSTAGNN_MAX_QUANTILES


def check_quantiles(quantiles, who="quantiles"):
    """The level rule (include/dstagnn.h): 1 <= Q <= 16 levels, each strictly inside (0, 1),
    strictly increasing, all of it as the fp32 values the kernels hold.  Returns the levels as a
    tuple of Python floats; a ValueError that names the broken rule otherwise.  No device."""
    try:
        levels = [float(v) for v in quantiles]
    except TypeError:
        raise ValueError(f"{who}: a sequence of quantile levels, got {quantiles!r}") from None
    if not 1 <= len(levels) <= MAX_QUANTILES:
        raise ValueError(f"{who}: between 1 and {MAX_QUANTILES} quantile levels, got {len(levels)}")
    held = [float(np.float32(v)) for v in levels]  # what the kernels see
    for v in held:
        if not 0.0 < v < 1.0:  # (a NaN fails too)
            raise ValueError(f"{who}: every quantile level must be strictly inside (0, 1), got {v!r}")
    for a, b in zip(held, held[1:]):
        if not a < b:
            raise ValueError(f"{who}: the quantile levels must be strictly increasing, got {a!r} before {b!r}")
    return tuple(levels)


def point_index_of(quantiles):
    """The column that serves as the point forecast: the level nearest 0.5, ties to the lower
    index."""
    levels = [float(np.float32(v)) for v in check_quantiles(quantiles)]
    return min(range(len(levels)), key=lambda q: (abs(levels[q] - 0.5), q))


class _PinballFn(torch.autograd.Function):
    """pinball_fwd / pinball_bwd as one autograd node; saved as _HipLossFn saves."""

    @staticmethod
    def forward(ctx, y, target, levels, mask_mode, null_val):
        loss, stat = _lib.load().pinball_fwd(y, target, levels, mask_mode, null_val)
        ctx.save_for_backward(y, target, stat)
        ctx.cfg = (levels, mask_mode, null_val)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        y, target, stat = ctx.saved_tensors
        if gout.dtype != torch.float32 or not gout.is_contiguous():
            gout = gout.float().contiguous()
        dy = _lib.load().pinball_bwd(y, target, stat, gout, *ctx.cfg)
        return dy, None, None, None, None


class QuantileLoss(nn.Module):
    """The pinball (quantile) loss of a (..., P, Q) prediction against a (..., P) target in one HIP
    launch per direction: with d = input[..., q] - target, the term is (1 - tau_q) d for d > 0,
    tau_q (-d) for d < 0 and 0 at d = 0 (slope 0 there), and

        loss = sum over valid entries and levels of the term / (count_valid * Q).

    ``quantiles``: 1 to 16 strictly increasing levels strictly inside (0, 1) (ValueError
    otherwise), held as fp32.  ``null_val`` masks by the TARGET as ``HipLoss(null_val=)`` does (NaN:
    the NaN targets); a masked entry gives no term and a gradient of exactly 0 to all its Q
    predictions, and with every entry masked the loss and the gradient are 0.  ``QuantileLoss((0.5,))``
    is half of ``HipLoss('mae')``.

    ``forward(input, target)``: ``input.shape[:-1] == target.shape`` and ``input.shape[-1] == Q`` (no
    broadcasting, ValueError), fp32 HIP tensors (RuntimeError otherwise), made contiguous if they
    are not; a 0-dim fp32 tensor.  The target takes no gradient (one that requires it raises) and
    the backward is once-differentiable.  ``point_index``: the column nearest 0.5."""

    def __init__(self, quantiles, null_val=None):
        super().__init__()
        self.quantiles = check_quantiles(quantiles, "QuantileLoss")
        self.point_index = point_index_of(self.quantiles)
        self.null_val = null_val
        self._cfg = (list(self.quantiles),) + mask_of(null_val)

    def extra_repr(self):
        return f"quantiles={self.quantiles}, null_val={self.null_val}"

    def forward(self, input, target):
        Q = len(self.quantiles)
        if input.dim() < 1 or tuple(input.shape[:-1]) != tuple(target.shape) or input.shape[-1] != Q:
            raise ValueError(f"QuantileLoss: input {tuple(input.shape)} must be target {tuple(target.shape)} with a "
                             f"last axis of {Q} quantiles (no broadcasting)")
        if not (input.is_cuda and target.is_cuda):
            raise RuntimeError(HIP_ONLY)
        if input.dtype != torch.float32 or target.dtype != torch.float32:
            raise RuntimeError("QuantileLoss: fp32 tensors only")
        if target.requires_grad:
            raise RuntimeError("QuantileLoss: the target takes no gradient (detach it)")
        input, target = input.contiguous(), target.contiguous()
        if torch.is_grad_enabled() and input.requires_grad:
            return _PinballFn.apply(input, target, *self._cfg)
        return _lib.load().pinball_fwd(input, target, *self._cfg)[0]  # nothing saved


class QuantileMetrics(_RunningTables):
    """Running calibration scores of (S, N, P, Q) quantile predictions against (S, N, P) targets,
    in the mould of ``ForecastMetrics``: ``update(pred, target)`` is one launch of
    ``metrics_quantile_kernel`` and no sync, no prediction is copied to the host.

    ``table`` is (P, 2 + 3 Q) fp64 on the device and ``node_table`` (num_nodes, 2 + 3 Q) or None,
    sums over the valid entries (``missing_value``: a number, or NaN for the NaN targets):
    column 0 the valid count, 1 the count of crossing entries (some prediction below its lower
    neighbour), 2 + 3 q the pinball sum of level q, 3 + 3 q the count of ``t <= pred_q``, 4 + 3 q the
    sum of ``pred_q``.

    ``scores()``: float64 arrays with one entry per horizon and a last, overall one from the column
    sums; NaN wherever the divisor is 0.  ``count`` (P + 1,), ``crossing_rate`` (P + 1,), ``pinball``
    (P + 1, Q), ``mean_pinball`` (P + 1,), ``coverage`` (P + 1, Q) (hits / count: a calibrated model
    gives about tau_q), ``mean_quantile`` (P + 1, Q), and for the pairs (q, Q - 1 - q), q < Q // 2:
    ``interval_width`` = mean_quantile[hi] - mean_quantile[lo] and ``interval_coverage`` =
    coverage[hi] - coverage[lo], both (P + 1, Q // 2).  ``interval_coverage`` is the share of targets
    in (pred_lo, pred_hi]; it is exact where no entry crosses (a crossing entry with pred_hi < t <=
    pred_lo counts -1).  ``node_scores()``: the same keys per node, without the overall entry.
    ``merge(other)`` adds another object's tables; ``all_reduce()`` sums them over the ranks."""

    def __init__(self, num_for_predict, quantiles, *, missing_value=None, num_nodes=None, device=None):
        self._check_horizon(num_for_predict)
        self.quantiles = check_quantiles(quantiles, "QuantileMetrics")
        self.point_index = point_index_of(self.quantiles)
        self.Q = len(self.quantiles)
        self._init_tables(2 + 3 * self.Q, device, missing_value, num_nodes)

    def update(self, pred, target):
        if (pred.dim() < 3 or tuple(pred.shape[:-1]) != tuple(target.shape) or pred.shape[-1] != self.Q
                or pred.shape[-2] != self.P):
            raise ValueError(f"QuantileMetrics: pred {tuple(pred.shape)} / target {tuple(target.shape)} must be "
                             f"(..., N, {self.P}, {self.Q}) and (..., N, {self.P})")
        self._check_nodes(pred, -3)
        if not (pred.is_cuda and target.is_cuda):
            raise RuntimeError(HIP_ONLY)
        if pred.numel() == 0:
            return
        _lib.load().metrics_update_quantile(pred.detach().contiguous(), target.detach().contiguous(),
                                            list(self.quantiles), self._mask[0], self._mask[1], self.table,
                                            self.node_table)

    @staticmethod
    def scores_of_table(table, overall=True):
        """The scores of a (K, 2 + 3 Q) table of sums (a numpy array), one entry per row and, with
        ``overall``, one more from the column sums.  NaN wherever a divisor is 0."""
        tab = np.asarray(table, dtype=np.float64)
        if tab.ndim != 2 or tab.shape[1] < 5 or (tab.shape[1] - 2) % 3:
            raise ValueError(f"QuantileMetrics: a table of sums is (K, 2 + 3 Q), got {tab.shape}")
        if overall:
            tab = np.concatenate([tab, tab.sum(0, keepdims=True)], 0)
        Q = (tab.shape[1] - 2) // 3
        count = tab[:, 0].copy()

        def over(a):
            b = count if a.ndim == 1 else np.broadcast_to(count[:, None], a.shape)
            out = np.full(a.shape, np.nan)
            np.divide(a, b, out=out, where=b != 0)
            return out
        pin, cov, mq = over(tab[:, 2::3]), over(tab[:, 3::3]), over(tab[:, 4::3])
        lo, hi = np.arange(Q // 2), Q - 1 - np.arange(Q // 2)
        return {"count": count, "crossing_rate": over(tab[:, 1]), "pinball": pin, "mean_pinball": pin.mean(1),
                "coverage": cov, "mean_quantile": mq, "interval_width": mq[:, hi] - mq[:, lo],
                "interval_coverage": cov[:, hi] - cov[:, lo]}

    def scores(self):
        return self.scores_of_table(self.table.cpu().numpy())

    def _config(self):
        return (self.P, self.quantiles, self._mask[0], repr(self._mask[1]), self.num_nodes)


# ---- skill against the forecasts that cost nothing -----------------------------------------------
SKILL_COLS = 13  # include/dstagnn.h DSTAGNN_SKILL_COLS
BASELINES = (("persistence", 0), ("climatology", 5))  # (name, first column of its five sums)


def check_period(period, L, who="BaselineSkill"):
    """The climatology period as an int in [1, L]; ValueError for a missing or any other one."""
    if period is None or isinstance(period, bool):
        raise ValueError(f"{who}: a climatology period is needed (an int in [1, {int(L)}]), got {period!r}")
    try:
        p = int(period)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: the climatology period must be an int in [1, {int(L)}], got {period!r}") from None
    if p != period or not 1 <= p <= int(L):
        raise ValueError(f"{who}: the climatology period must be an int in [1, {int(L)}] (the series' length), "
                         f"got {period!r}")
    return p


class BaselineSkill(_RunningTables):
    """Running skill of (B, N, P) forecasts over persistence ("the next P steps equal the last
    observed value") and over the seasonal climatology (the node's mean training value at this
    phase ``t mod period`` of the cycle), plus the anomaly correlation, per horizon and per node.
    Both baseline forecasts are read out of the raw series ``series`` (a windows.WindowedSeries)
    keeps on the device, inside the scoring launch (``skill_kernel``): nothing is materialised and
    no prediction is copied to the host.

    ``missing_value`` (a number, or NaN for the NaN values: ``mask_of``): a target equal to it
    reaches no sum, a series element equal to it is not observed.  Persistence then takes the latest
    observed value at any distance back, from an unlimited forward fill made once
    (``series.filled`` when that was built with ``fill='ffill'`` and ``max_gap=None`` under the same
    missing value, else one ``dstagnn::window_fill_forward``), and is undefined where there is none;
    the climatology (``dstagnn::climatology``, once: the observed training steps
    ``[0, labels['train'][-1] + P)`` only) is undefined at a (phase, node) never observed in training.
    The model and a baseline are always summed over the same entries.

    ``update(pred, target, split, idx)``: ``idx`` as ``WindowedSeries.batch`` takes it (a slice, a
    sequence, or an int64 tensor of positions in ``split``); one launch, no sync.  A position outside
    the split contributes nothing.  A (..., P, Q) quantile forecast is refused: pass its
    ``point_index`` column.  ``table`` is (P, 13) fp64 on the device, ``node_table`` (num_nodes, 13)
    or None (columns: include/dstagnn.h).

    ``scores()``: float64 arrays of shape (P + 1,), the overall value last (from the column sums),
    NaN wherever a divisor is 0; for b in persistence, climatology: ``count_b``, ``rmse_b`` /
    ``mae_b`` (the baseline's own), ``model_rmse_b`` / ``model_mae_b`` (the model on that entry
    set), ``mse_skill_b`` = 1 - sum e_m^2 / sum e_b^2, ``mae_skill_b`` = 1 - sum |e_m| / sum |e_b|;
    and ``acc``.  ``node_scores()``: the same keys in shape (num_nodes,).  ``climatology()``: the
    (period, N) fp64 table and its int32 counts as numpy arrays.  ``reset`` / ``merge`` /
    ``all_reduce`` as ``ForecastMetrics``."""

    def __init__(self, series, period, *, missing_value=None, num_nodes=None):
        for name in ("L", "N", "F", "P", "labels", "device"):
            if not hasattr(series, name):
                raise TypeError(f"BaselineSkill: series must be a windows.WindowedSeries, got {type(series).__name__}")
        self.period = check_period(period, series.L)
        self._check_horizon(series.P)
        if num_nodes is not None and int(num_nodes) != int(series.N):
            raise ValueError(f"BaselineSkill: num_nodes is {num_nodes!r}, the series has {series.N} nodes")
        if missing_value is not None:
            from .windows import check_missing_options
            check_missing_options(missing_value)  # (a marker float32 does not hold is refused)
        self.N, self.L = int(series.N), int(series.L)
        self.t_end = int(series.labels["train"][-1]) + self.P
        self._init_tables(SKILL_COLS, series.device, missing_value, num_nodes)
        self.series = series
        ops = _lib.load()
        masked = self.missing_value is not None
        null = self.missing_value if masked else 0.0
        self._src_mask = (masked, null)
        self._clim, self._cnt = ops.climatology(series.series, self.period, self.t_end, masked, null)
        if not masked:
            self._pers = series.series
        elif (getattr(series, "filled", None) is not None and series.fill == "ffill" and series.max_gap is None
              and mask_of(series.missing_value) == self._mask):
            self._pers = series.filled
        else:
            self._pers = ops.window_fill_forward(series.series, null, 0)[0]

    def climatology(self):
        return self._clim.cpu().numpy(), self._cnt.cpu().numpy()

    def _positions(self, split, idx):
        """(B,) int64 label positions on the device; -1 for a position outside the split."""
        labels = getattr(self.series, "_labels", {}).get(split)
        if labels is None:
            raise KeyError(f"BaselineSkill: no split {split!r}")
        S = labels.numel()
        if isinstance(idx, slice):
            return labels[idx].contiguous()  # (a view for a unit step: no launch)
        if not torch.is_tensor(idx):
            i = np.asarray(idx, dtype=np.int64).reshape(-1)
            ok = (i >= 0) & (i < S)
            pos = np.where(ok, self.series.labels[split][np.where(ok, i, 0)], -1)
            return torch.from_numpy(np.ascontiguousarray(pos, dtype=np.int64)).to(labels.device)
        if idx.dtype != torch.int64 or idx.dim() != 1:
            raise ValueError("BaselineSkill.update: idx must be a 1-D int64 tensor")
        idx = idx.to(labels.device)
        ok = (idx >= 0) & (idx < S)
        return torch.where(ok, labels[idx.clamp(0, S - 1)], torch.full_like(idx, -1))

    def update(self, pred, target, split, idx):
        if pred.dim() == target.dim() + 1 and tuple(pred.shape[:-1]) == tuple(target.shape):
            raise ValueError(f"BaselineSkill: pred {tuple(pred.shape)} is a (..., P, Q) quantile forecast; pass its "
                             "point_index column (pred[..., point_index])")
        if pred.shape != target.shape or pred.dim() != 3 or pred.shape[-1] != self.P or pred.shape[-2] != self.N:
            raise ValueError(f"BaselineSkill: pred {tuple(pred.shape)} / target {tuple(target.shape)} must be equal "
                             f"(B, {self.N}, {self.P}) shapes")
        if not (pred.is_cuda and target.is_cuda):
            raise RuntimeError(HIP_ONLY)
        pos = self._positions(split, idx)
        if pos.numel() != pred.shape[0]:
            raise ValueError(f"BaselineSkill: {pos.numel()} positions for {pred.shape[0]} samples")
        if pred.numel() == 0:
            return
        _lib.load().skill_update(pred.detach().contiguous(), target.detach().contiguous(), self._mask[0],
                                 self._mask[1], self._pers, self._src_mask[0], self._src_mask[1], pos, self._clim,
                                 self._cnt, self.table, self.node_table)

    @staticmethod
    def scores_of_table(table, overall=True):
        """The scores of a (K, 13) table of sums (a numpy array), one entry per row and, with
        ``overall``, one more from the column sums.  NaN wherever a divisor is 0."""
        tab = np.asarray(table, dtype=np.float64)
        if tab.ndim != 2 or tab.shape[1] != SKILL_COLS:
            raise ValueError(f"BaselineSkill: a table of sums is (K, {SKILL_COLS}), got {tab.shape}")
        if overall:
            tab = np.concatenate([tab, tab.sum(0, keepdims=True)], 0)

        def over(a, b):
            out = np.full(a.shape, np.nan)
            np.divide(a, b, out=out, where=b != 0)
            return out
        out = {}
        for name, c in BASELINES:
            n = tab[:, c]
            out[f"count_{name}"] = n.copy()
            out[f"rmse_{name}"], out[f"mae_{name}"] = np.sqrt(over(tab[:, c + 2], n)), over(tab[:, c + 4], n)
            out[f"model_rmse_{name}"], out[f"model_mae_{name}"] = np.sqrt(over(tab[:, c + 1], n)), over(tab[:, c + 3], n)
            out[f"mse_skill_{name}"] = 1.0 - over(tab[:, c + 1], tab[:, c + 2])
            out[f"mae_skill_{name}"] = 1.0 - over(tab[:, c + 3], tab[:, c + 4])
        out["acc"] = over(tab[:, 10], np.sqrt(tab[:, 11] * tab[:, 12]))
        return out

    def scores(self):
        return self.scores_of_table(self.table.cpu().numpy())

    def _config(self):
        return (self.P, self.N, self.L, self.period, self.t_end, self._mask[0], repr(self._mask[1]), self.num_nodes)


# ---- drought event scores ------------------------------------------------------------------------
MAX_EVENT_LEVELS = 7  # include/dstagnn.h DSTAGNN_MAX_EVENT_LEVELS
DIRECTIONS = ("below", "above")
_EVENT_MAX_LDS = 64 * 1024  # csrc/loss.hip kEvMaxLds


def check_direction(direction, who="EventScores"):
    """``below`` (event k is v <= thr_k) or ``above`` (v >= thr_k); ValueError otherwise."""
    if direction not in DIRECTIONS:
        raise ValueError(f"{who}: direction must be 'below' or 'above', got {direction!r}")
    return direction


def check_thresholds(thresholds, direction="below", who="EventScores"):
    """The threshold rule (include/dstagnn.h, the events section), checked on the host on the fp32
    values the kernel compares with.  A sequence, array or tensor of shape (K,) (one set for all
    nodes) or (K, N) (one column per node), 1 <= K <= 7, mildest first, none infinite.  (K,): no NaN,
    strictly decreasing for ``below`` / strictly increasing for ``above`` (two thresholds that round
    to the same float are an error).  (K, N): every column either all NaN (the node is excluded) or
    free of NaN and non-increasing / non-decreasing (ties are allowed).  Returns a C-contiguous
    float32 array; a ValueError that names the broken rule otherwise.  No device."""
    check_direction(direction, who)
    if torch.is_tensor(thresholds):
        thresholds = thresholds.detach().cpu().numpy()
    try:
        wide = np.asarray(thresholds, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: thresholds must be numbers in a (K,) or (K, N) array, got {thresholds!r}") from None
    if wide.ndim not in (1, 2) or wide.size == 0:
        raise ValueError(f"{who}: thresholds must have shape (K,) or (K, N), got {wide.shape}")
    if not 1 <= wide.shape[0] <= MAX_EVENT_LEVELS:
        raise ValueError(f"{who}: between 1 and {MAX_EVENT_LEVELS} thresholds, got {wide.shape[0]}")
    with np.errstate(over="ignore"):
        thr = np.ascontiguousarray(wide.astype(np.float32))  # what the kernel sees
    if np.isinf(thr).any():
        raise ValueError(f"{who}: an infinite threshold (as float32) defines no event class")
    nan = np.isnan(thr)
    if thr.ndim == 1:
        if nan.any():
            raise ValueError(f"{who}: a (K,) threshold set holds no NaN (only a node's whole column of a (K, N) table "
                             "may, which excludes the node)")
    elif (nan.any(0) & ~nan.all(0)).any():
        n = int(np.flatnonzero(nan.any(0) & ~nan.all(0))[0])
        raise ValueError(f"{who}: the threshold column of node {n} mixes NaN and numbers (all NaN excludes a node)")
    d = np.diff(np.where(nan, 0.0, thr.astype(np.float64)), axis=0)
    if direction == "above":
        d = -d
    if thr.ndim == 1 and not (d < 0).all():
        raise ValueError(f"{who}: (K,) thresholds are listed mildest first: strictly "
                         f"{'decreasing' if direction == 'below' else 'increasing'} for direction {direction!r} as "
                         f"float32 (two that round to the same float are an error), got {thr.tolist()}")
    if thr.ndim == 2 and not (d <= 0).all():
        n = int(np.flatnonzero((d > 0).any(0))[0])
        raise ValueError(f"{who}: the threshold column of node {n} must be "
                         f"{'non-increasing' if direction == 'below' else 'non-decreasing'} (mildest first) for "
                         f"direction {direction!r}, got {thr[:, n].tolist()}")
    return thr


def check_percentiles(percentiles, direction="below", who="node_percentile_thresholds"):
    """1 to 7 percentiles strictly inside (0, 100), mildest first: strictly decreasing for ``below``,
    strictly increasing for ``above``.  Returns a tuple of floats; ValueError otherwise."""
    check_direction(direction, who)
    try:
        pct = [float(v) for v in percentiles]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: a sequence of percentiles, got {percentiles!r}") from None
    if not 1 <= len(pct) <= MAX_EVENT_LEVELS:
        raise ValueError(f"{who}: between 1 and {MAX_EVENT_LEVELS} percentiles, got {len(pct)}")
    for v in pct:
        if not 0.0 < v < 100.0:  # (a NaN fails too)
            raise ValueError(f"{who}: every percentile must be strictly inside (0, 100), got {v!r}")
    for a, b in zip(pct, pct[1:]):
        if not (a > b if direction == "below" else a < b):
            raise ValueError(f"{who}: the percentiles are listed mildest first: strictly "
                             f"{'decreasing' if direction == 'below' else 'increasing'} for direction {direction!r}, "
                             f"got {a!r} before {b!r}")
    return tuple(pct)


def node_percentile_thresholds(series, percentiles, *, direction="below", missing_value=None):
    """(K, N) fp32 thresholds on the series' device for ``EventScores``: per node the
    ``percentiles[k]``-th percentile (linear interpolation, fp64, ``torch.nanquantile``) of the
    observed target-feature values of ``series`` (a windows.WindowedSeries) over the training steps
    ``[0, labels['train'][-1] + P)``, ``BaselineSkill``'s ``t_end``: nothing of validation or test
    enters.  ``missing_value`` (a number, or NaN) marks the elements that are not observed, by the
    series' own dtype; a node with no observed training value gets an all-NaN column, which excludes
    it.  ``percentiles``: ``check_percentiles`` under ``direction``.  An init-time torch call over
    L N values: no kernel of its own."""
    pct = check_percentiles(percentiles, direction)
    for name in ("series", "P", "labels"):
        if not hasattr(series, name):
            raise TypeError(f"node_percentile_thresholds: series must be a windows.WindowedSeries, got "
                            f"{type(series).__name__}")
    if missing_value is not None:
        from .windows import check_missing_options
        check_missing_options(missing_value)  # (a marker float32 does not hold is refused)
    t_end = int(series.labels["train"][-1]) + int(series.P)
    raw = series.series[:t_end, :, -1]
    v = raw.to(torch.float64)
    if missing_value is not None and not math.isnan(float(missing_value)):
        v = torch.where(raw == float(missing_value), torch.full_like(v, float("nan")), v)
    q = torch.tensor(pct, dtype=torch.float64, device=v.device) / 100.0
    return torch.nanquantile(v, q, dim=0).to(torch.float32).contiguous()


class EventScores(_RunningTables):
    """Running class contingency tables of (B, N, P) forecasts against K thresholds on the index,
    per horizon and per node, and the categorical scores drought verification reads from them.
    ``update(pred, target)`` is one launch of ``events_kernel`` and no sync; no prediction is copied
    to the host.

    ``thresholds`` (``check_thresholds``): (K,) for all nodes or (K, N) per node (that form fixes
    ``num_nodes`` at N; ``node_percentile_thresholds`` makes one), 1 <= K <= 7, mildest first, in the
    units of the raw targets.  ``direction``: ``below`` (event k is v <= thr_k, e.g. SPI -1, -1.5, -2)
    or ``above`` (v >= thr_k); every compare in fp32, a value equal to the threshold is an event.  The
    class of a value is the number of its events, 0 .. K.  ``missing_value`` (a number, or NaN:
    ``mask_of``): a target equal to it reaches no count.  A node whose column is all NaN is excluded
    (``excluded``).

    ``table`` is (P, 2 + (K + 1)^2) fp64 on the device, ``node_table`` (num_nodes, ...) or None, all
    integers: column 0 the entries with a valid target on a node that is not excluded, 1 those among
    them whose prediction is NaN (they reach no cell), 2 + co (K + 1) + cf the entries of observed
    class co and forecast class cf.

    ``scores()``: float64 arrays with one entry per horizon and a last, overall one from the column
    sums, NaN wherever a divisor is 0.  ``count``, ``nan_pred`` (P + 1,); ``confusion``
    (P + 1, K + 1, K + 1); ``observed_freq``, ``forecast_freq`` (P + 1, K + 1).  Per threshold k,
    (P + 1, K), from a = sum over co > k, cf > k (hits), b = co <= k, cf > k (false alarms), c = co > k,
    cf <= k (misses), d the rest, n = a + b + c + d: ``hits``, ``false_alarms``, ``misses``,
    ``correct_negatives``, ``base_rate`` (a + c) / n, ``pod`` a / (a + c), ``far`` b / (a + b), ``pofd``
    b / (b + d), ``csi`` a / (a + b + c), ``freq_bias`` (a + b) / (a + c), ``accuracy`` (a + d) / n,
    ``ets`` (a - a_r) / (a + b + c - a_r) with a_r = (a + b)(a + c) / n, ``hss`` 2 (a d - b c) /
    ((a + c)(c + d) + (a + b)(b + d)).  Multi-category, (P + 1,): ``class_accuracy`` and
    ``hss_multi``.  ``node_scores()``: the same keys per node, without the overall entry.
    ``reset`` / ``merge`` / ``all_reduce`` as ``ForecastMetrics``; ``merge`` refuses another
    definition (thresholds, direction, mask)."""

    def __init__(self, num_for_predict, thresholds, *, direction="below", missing_value=None, num_nodes=None,
                 device=None):
        self._check_horizon(num_for_predict)
        self.direction = check_direction(direction)
        thr = check_thresholds(thresholds, direction)
        self.K = int(thr.shape[0])
        if thr.ndim == 2:
            if num_nodes is not None and int(num_nodes) != thr.shape[1]:
                raise ValueError(f"EventScores: num_nodes is {num_nodes!r}, the thresholds are per node for "
                                 f"{thr.shape[1]} nodes")
            num_nodes = int(thr.shape[1])
        if num_nodes is not None and int(num_nodes) < 1:  # (judged before the device is)
            raise ValueError(f"EventScores: num_nodes must be >= 1, got {num_nodes!r}")
        cols =2 + (self.K + 1) ** 2
        if (self.P + 256 // self.P) * cols * 4 > _EVENT_MAX_LDS:
            raise ValueError(f"EventScores: K = {self.K} thresholds with num_for_predict = {self.P} need more than "
                             f"{_EVENT_MAX_LDS} bytes of LDS for the histograms (K = 7 takes 2 <= P <= 247)")
        if missing_value is not None:
            from .windows import check_missing_options
            check_missing_options(missing_value)  # (a marker float32 does not hold is refused)
        self._thr_host = thr
        self._init_tables(cols, device, missing_value, num_nodes)
        self._thr = torch.from_numpy(thr).to(self.table.device)

    @property
    def thresholds(self):
        return self._thr_host.copy()

    @property
    def excluded(self):
        return None if self._thr_host.ndim == 1 else np.isnan(self._thr_host).all(0)

    def update(self, pred, target):
        if pred.dim() == target.dim() + 1 and tuple(pred.shape[:-1]) == tuple(target.shape):
            raise ValueError(f"EventScores: pred {tuple(pred.shape)} is a (..., P, Q) quantile forecast; pass its "
                             "point_index column (pred[..., point_index])")
        if pred.shape != target.shape or pred.dim() < 2 or pred.shape[-1] != self.P:
            raise ValueError(f"EventScores: pred {tuple(pred.shape)} / target {tuple(target.shape)} must be "
                             f"equal (..., N, {self.P}) shapes")
        self._check_nodes(pred, -2)
        if not (pred.is_cuda and target.is_cuda):
            raise RuntimeError(HIP_ONLY)
        if pred.numel() == 0:
            return
        _lib.load().events_update(pred.detach().contiguous(), target.detach().contiguous(), self._mask[0],
                                  self._mask[1], self._thr, self.direction == "above", self.table, self.node_table)

    @staticmethod
    def scores_of_table(table, overall=True):
        """The scores of a (R, 2 + (K + 1)^2) table of counts (a numpy array), one entry per row and,
        with ``overall``, one more from the column sums.  NaN wherever a divisor is 0."""
        tab = np.asarray(table, dtype=np.float64)
        K1 = math.isqrt(tab.shape[1] - 2) if tab.ndim == 2 and tab.shape[1] >= 6 else 0
        if not 2 <= K1 <= MAX_EVENT_LEVELS + 1 or K1 * K1 != tab.shape[1] - 2:
            raise ValueError(f"EventScores: a table of counts is (R, 2 + (K + 1)^2) with 1 <= K <= "
                             f"{MAX_EVENT_LEVELS}, got {tab.shape}")
        if overall:
            tab = np.concatenate([tab, tab.sum(0, keepdims=True)], 0)
        R, K = tab.shape[0], K1 - 1
        M = tab[:, 2:].reshape(R, K1, K1)

        def over(a, b):
            a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
            out = np.full(a.shape, np.nan)
            np.divide(a, b, out=out, where=(b != 0) & ~np.isnan(b))
            return out
        n = M.sum((1, 2))
        out = {"count": tab[:, 0].copy(), "nan_pred": tab[:, 1].copy(), "confusion": M.copy(),
               "observed_freq": over(M.sum(2), n[:, None]), "forecast_freq": over(M.sum(1), n[:, None])}
        a = np.stack([M[:, k + 1:, k + 1:].sum((1, 2)) for k in range(K)], 1)
        b = np.stack([M[:, :k + 1, k + 1:].sum((1, 2)) for k in range(K)], 1)
        c = np.stack([M[:, k + 1:, :k + 1].sum((1, 2)) for k in range(K)], 1)
        d = np.stack([M[:, :k + 1, :k + 1].sum((1, 2)) for k in range(K)], 1)
        n2 = a + b + c + d
        a_r = over((a + b) * (a + c), n2)  # NaN at n = 0: so is ets
        out.update(hits=a, false_alarms=b, misses=c, correct_negatives=d, base_rate=over(a + c, n2),
                   pod=over(a, a + c), far=over(b, a + b), pofd=over(b, b + d), csi=over(a, a + b + c),
                   freq_bias=over(a + b, a + c), accuracy=over(a + d, n2), ets=over(a - a_r, a + b + c - a_r),
                   hss=over(2.0 * (a * d - b * c), (a + c) * (c + d) + (a + b) * (b + d)))
        p = over(M, n[:, None, None])
        agree = np.trace(p, axis1=1, axis2=2)
        chance = (p.sum(2) * p.sum(1)).sum(1)
        out["class_accuracy"] = over(np.trace(M, axis1=1, axis2=2), n)
        out["hss_multi"] = over(agree - chance, 1.0 - chance)
        return out

    def scores(self):
        return self.scores_of_table(self.table.cpu().numpy())

    def _config(self):
        return (self.P, self.K, self.direction, self._thr_host.shape, self._thr_host.tobytes(), self._mask[0],
                repr(self._mask[1]), self.num_nodes)
