"""Training driver: the counterpart of train_DSTAGNN_my.py on MI355X.

    python -m dstagnn_drought_amd.train --config configurations/PEMS08_dstagnn.conf
    torchrun --nproc-per-node 8 -m dstagnn_drought_amd.train --config ...   (one rank per GPU)

Same configuration files, graph loading, model construction (make_model), loss
(SmoothL1), optimiser (Adam, the config's learning rate), epoch loop, validation,
best-epoch checkpoints ``myexperiments/{dataset}/{model}_{h}h{d}d{w}w_channel{c}_{lr}/
epoch_{e}.params`` in the reference's state_dict format, and final test loss
(train_DSTAGNN_my.py:30-191).  Where the reference runs on torch_xla, this runs one
process per GPU with torch.distributed over RCCL:

  * ``xm.optimizer_step`` (:148, :158) = mean all-reduce of the gradients over the ranks
    (dp.GradAllReducer, bucketed, cheb-mask grads as their support) + ``optimizer.step()``.
    The reference's double step per batch (quirk 14: the step at :148 re-applies the
    previous batch's gradients before ``zero_grad``) is kept by default
    (``double_step=True``; its gradients are already reduced, so no second collective).
  * data parallelism shards the training set (DistributedSampler order: rank r takes
    positions r, r+W, ... of the epoch permutation) instead of every replica training on
    the full set (quirk 15); validation / test batches are split across ranks and their
    per-batch losses all-reduced, so the reported mean over batches is the reference's.
  * batches are cut on the device (one index_select per batch from HBM-resident tensors)
    instead of DataLoader collation + MpDeviceLoader; the epoch permutation is drawn as
    torch's RandomSampler draws it (a seed from the global RNG, then randperm), so the
    first epoch visits samples in the reference's order.
  * the missing ``graph`` key of the PEMS03/07/08 configs (quirk 16: KeyError in the
    reference) defaults to 'AG'.
  * with ``stream_windows`` (a [Training] key, ``--stream-windows``) the raw series stays on the
    device once and every batch's windows are gathered from it in one launch
    (windows.WindowedSeries) instead of loading the prepared, ``len_input``-times larger file.
  * the criterion is the reference's ``nn.SmoothL1Loss()`` unless the configuration
    (loss_options()) or ``--loss`` / ``--missing-value`` name one: then loss.HipLoss, on the
    HIP path, optionally leaving targets equal to a missing value out of the loss.  With
    ``input_fill`` (input_options(), ``--input-fill``) the streamed inputs equal to that value are
    imputed in the gather launch and the statistics taken over the observed values.
  * with ``quantiles`` (quantile_options(), ``--quantiles 0.1,0.5,0.9``) the model has a quantile head
    ((B, N, P, Q) forecasts), the criterion is the pinball loss.QuantileLoss, and the test scores gain
    coverage / pinball / interval width / crossing rate (loss.QuantileMetrics).
"""
import argparse
import configparser
import math
import os
import random
import time

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn
import torch.utils.data

from . import data as data_io
from .dp import GradAllReducer, mask_support_of
from .model import make_model, set_direct_grads, set_dropout


def seed_torch(seed):
    """train_DSTAGNN_my.py:20-28."""
    random.seed(seed)
    os.environ['PYTHONHASHSEED'] = str(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def _world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


class DeviceBatches:
    """Mini-batches of HBM-resident (x, y) tensors.  shuffle: a fresh permutation per epoch
    drawn as torch's shuffled DataLoader draws it (same global-RNG consumption); with
    world > 1 rank r takes permutation positions r, r+W, ... (DistributedSampler order,
    padded by wrapping so every rank runs the same number of steps)."""

    def __init__(self, x, y, batch_size, shuffle, rank=0, world=1):
        self.x, self.y, self.bs, self.shuffle = x, y, int(batch_size), shuffle
        self.rank, self.world = rank, world

    def _order(self):
        n = self.x.shape[0]
        # the permutation (and every global-RNG draw) exactly as iterating the reference's
        # shuffled DataLoader would make it: one batch of a DataLoader over the positions
        perm = next(iter(torch.utils.data.DataLoader(torch.arange(n), batch_size=n, shuffle=self.shuffle)))
        if self.world > 1:
            per = -(-n // self.world)
            perm = torch.cat([perm, perm[:per * self.world - n]])[self.rank::self.world]
        return perm

    def __len__(self):
        n = -(-self.x.shape[0] // self.world) if self.world > 1 else self.x.shape[0]
        return -(-n // self.bs)

    def __iter__(self):
        perm = self._order().to(self.x.device)
        for i in range(0, perm.numel(), self.bs):
            idx = perm[i:i + self.bs]
            yield self.x.index_select(0, idx), self.y.index_select(0, idx)


class StreamBatches(DeviceBatches):
    """DeviceBatches over the ``x`` / ``y`` of a windows.WindowedSeries split: the same
    permutation, global-RNG draws, sharding and wrap-around padding (DeviceBatches._order), each
    batch gathered from the raw series in ONE launch instead of two
    index_selects from materialised tensors."""

    def __init__(self, x, y, batch_size, shuffle, rank=0, world=1):
        if not _is_streamed(x) or not _is_streamed(y) or (x.owner, x.name) != (y.owner, y.name):
            raise ValueError("StreamBatches: x and y must be the two arrays of one WindowedSeries split")
        super().__init__(x, y, batch_size, shuffle, rank, world)

    def __iter__(self):
        perm = self._order().to(self.x.device)
        for i in range(0, perm.numel(), self.bs):
            yield self.x.owner.batch(self.x.name, perm[i:i + self.bs])


def _is_streamed(t):
    return hasattr(t, "owner") and hasattr(t.owner, "batch")


def make_batches(x, y, batch_size, shuffle, rank=0, world=1):
    """StreamBatches for the arrays of a WindowedSeries split, DeviceBatches for tensors."""
    cls = StreamBatches if _is_streamed(x) else DeviceBatches
    return cls(x, y, batch_size, shuffle, rank, world)


def _cut(x, y, b, e):
    """Samples b .. e of (x, y): views of tensors; one gather launch for a streamed split."""
    if _is_streamed(x) and _is_streamed(y) and (x.owner, x.name) == (y.owner, y.name):
        return x.owner.batch(x.name, slice(b, e))
    return x[b:e], y[b:e]


def eval_batches(net, x, y, batch_size, criterion):
    """Mean over batches of the batch-mean loss (train_DSTAGNN_my.py:164-172), with the
    batches split round-robin over the ranks and the sums all-reduced.  x, y: tensors, or the
    arrays of a windows.WindowedSeries split (each batch then gathered from the raw series)."""
    rank, world = _world()
    iter(torch.utils.data.DataLoader(range(1)))  # the global-RNG draw a DataLoader iteration makes
    n = x.shape[0]
    starts = list(range(0, n, batch_size))
    tot = torch.zeros(2, dtype=torch.float64, device=x.device)
    with torch.no_grad():
        for b in starts[rank::world]:
            xb, yb = _cut(x, y, b, b + batch_size)
            tot[0] += criterion(net(xb), yb).double()
            tot[1] += 1
    if world > 1:
        dist.all_reduce(tot)
    return float(tot[0] / max(1.0, float(tot[1])))


def compute_val_loss_mstgcn(net, val_loader, criterion, sw, epoch, limit=None):
    """lib/utils1.py:348-383: mean validation loss over the batches of `val_loader`
    (eval mode, no grad); `sw` (a SummaryWriter or None) gets 'validation_loss'."""
    net.train(False)
    with torch.no_grad():
        tmp = []
        for batch_index, (encoder_inputs, labels) in enumerate(val_loader):
            loss = criterion(net(encoder_inputs), labels)
            tmp.append(loss.item())
            if (limit is not None) and batch_index >= limit:
                break
        validation_loss = sum(tmp) / len(tmp)
        if sw is not None:
            sw.add_scalar('validation_loss', validation_loss, epoch)
    return validation_loss


def evaluate_on_test_mstgcn(net, test_loader, test_target_tensor, sw, epoch, _mean, _std):
    """lib/utils1.py:381-432: MAE / RMSE / MAPE of the predictions over `test_loader` for every
    horizon, printed as the reference prints them and written to `sw` (a SummaryWriter or None)
    as 'MAE_{i}_points', 'RMSE_{i}_points', 'MAPE_{i}_points'.  The reference copies every
    prediction to the host and scores with sklearn; here each batch is scored on the device
    against its slice of `test_target_tensor` in loader order (loss.ForecastMetrics: one launch
    per batch) and only the (P, 4) table of sums comes back.  Also returns the list
    predict_and_save_results_mstgcn returns (the overall three last); the reference returns
    None.  `_mean` / `_std` are unused, as in the reference.  Every target is scored: for a series
    with gaps, or per-node scores, evaluate_on_test_masked."""
    return evaluate_on_test_masked(net, test_loader, test_target_tensor, sw, epoch)


def evaluate_on_test_masked(net, test_loader, test_target_tensor, sw, epoch, *, missing_value=None, per_node=False):
    """evaluate_on_test_mstgcn's loop, printed lines and `sw` scalars with two options (that
    function keeps the reference's parameter list).  missing_value (a number, or NaN for the NaN
    targets) leaves those targets out of every score, as the masked criterion leaves them out of
    the loss.  per_node: returns (list, ForecastMetrics.node_scores()), the per-node count / mae /
    rmse / mape / bias / nse arrays from the (N, 8) device table; no prediction is copied to the
    host.  With neither, the unmasked (P, 4) object of evaluate_on_test_mstgcn."""
    from .loss import ForecastMetrics
    net.train(False)
    with torch.no_grad():
        test_loader_length = len(test_loader)
        metrics, at = None, 0
        for batch_index, (encoder_inputs, labels) in enumerate(test_loader):
            outputs = net(encoder_inputs)
            if metrics is None:
                metrics = ForecastMetrics(outputs.shape[-1], 0.0, outputs.device, missing_value=missing_value,
                                          num_nodes=outputs.shape[-2] if per_node else None)
                test_target_tensor = test_target_tensor.to(outputs.device, torch.float32)
            metrics.update(outputs, test_target_tensor[at:at + outputs.shape[0]])
            at += outputs.shape[0]
            if batch_index % 100 == 0:
                print('predicting testing set batch %s / %s' % (batch_index + 1, test_loader_length))
        assert metrics is not None and test_target_tensor.shape[0] == at
        excel_list = metrics.compute()
        for i in range(metrics.P):
            mae, rmse, mape = excel_list[3 * i:3 * i + 3]
            print('current epoch: %s, predict %s points' % (epoch, i))
            print('MAE: %.2f' % (mae))
            print('RMSE: %.2f' % (rmse))
            print('MAPE: %.2f' % (mape))
            print()
            if sw:
                sw.add_scalar('MAE_%s_points' % (i), mae, epoch)
                sw.add_scalar('RMSE_%s_points' % (i), rmse, epoch)
                sw.add_scalar('MAPE_%s_points' % (i), mape, epoch)
    return (excel_list, metrics.node_scores()) if per_node else excel_list


def score_batches(net, x, y, batch_size, missing_value=None, per_node=False, quantiles=None, skill=None, events=None):
    """The test-set scores of `net` over (x, y), batched and sharded as eval_batches does it
    (batches of `batch_size` cut with _cut, round-robin over the ranks), accumulated on the device
    and summed over the ranks at the end.  Returns the loss.ForecastMetrics: masked by
    missing_value when there is one, with the node table when per_node; with neither, the
    unmasked (P, 4) object.  x, y: tensors, or the arrays of a windows.WindowedSeries split.
    quantiles (the levels of a quantile model): the ForecastMetrics is fed the ``point_index`` column
    of the (B, N, P, Q) forecasts, and a loss.QuantileMetrics, fed all of them in the same pass, is
    returned beside it: (ForecastMetrics, QuantileMetrics).
    skill (a loss.BaselineSkill over the WindowedSeries whose split x and y are): fed in the same
    pass with the same (b, e) cuts, one more launch per batch (the ``point_index`` column of a
    quantile model), and all-reduced at the end; the returned value is unchanged.  None: nothing
    is launched for it.
    events (a loss.EventScores): fed the same way (the same cuts, one more launch per batch, the
    ``point_index`` column of a quantile model, all-reduced at the end); works on tensors and on a
    streamed split alike.  None: nothing is launched for it and the returned value is unchanged."""
    from .loss import ForecastMetrics, QuantileMetrics
    rank, world = _world()
    if skill is not None and not (_is_streamed(y) and y.owner is skill.series):
        raise ValueError("score_batches: skill needs the y of a split of the BaselineSkill's own WindowedSeries")
    nodes = y.shape[-2] if per_node else None
    metrics = ForecastMetrics(y.shape[-1], 0.0, x.device, missing_value=missing_value, num_nodes=nodes)
    qm = None
    if quantiles is not None:
        qm = QuantileMetrics(y.shape[-1], quantiles, missing_value=missing_value, num_nodes=nodes, device=x.device)
    with torch.no_grad():
        for b in list(range(0, x.shape[0], batch_size))[rank::world]:
            xb, yb = _cut(x, y, b, b + batch_size)
            out = net(xb)
            if qm is not None:
                qm.update(out, yb)
                out = out[..., qm.point_index]
            metrics.update(out, yb)
            if skill is not None:
                skill.update(out, yb, y.name, slice(b, b + batch_size))
            if events is not None:
                events.update(out, yb)
    if skill is not None:
        skill.all_reduce()
    if events is not None:
        events.all_reduce()
    return metrics.all_reduce() if qm is None else (metrics.all_reduce(), qm.all_reduce())


def predict_and_save_results_mstgcn(net, data_loader, data_target_tensor, global_step, _mean, _std, params_path,
                                    type, missing_value=None, quantiles=None):
    """lib/utils1.py:441-510: predictions over `data_loader`, saved with the de-normalised
    inputs as ``output_epoch_{step}_{type}.npz`` (keys input, prediction,
    data_target_tensor); returns the per-horizon [MAE, RMSE, MAPE] list + the overall three.
    missing_value (a number, or NaN for the NaN targets): the targets equal to it are left out of
    the list, which then comes from the masked loss.ForecastMetrics on the device, each batch
    scored against its slice of the targets in loader order (sklearn raises on a NaN target and
    scores a sentinel as data); the file is saved as before.
    quantiles (the levels of a quantile model): ``prediction`` is stored as (S, N, P, Q) with the
    levels beside it (key ``quantiles``), and the list is taken from the ``point_index`` column."""
    net.train(False)
    point = None
    if quantiles is not None:
        from .loss import point_index_of
        point = point_index_of(quantiles)
    with torch.no_grad():
        metrics, at = None, 0
        if missing_value is not None:
            from .loss import ForecastMetrics
            metrics = ForecastMetrics(data_target_tensor.shape[-1], 0.0, next(net.parameters()).device,
                                      missing_value=missing_value)
            target_dev = data_target_tensor.to(metrics.table.device, torch.float32)
        data_target_tensor = data_target_tensor.cpu().numpy()
        prediction, inputs = [], []
        for encoder_inputs, labels in data_loader:
            inputs.append(encoder_inputs[:, :, 0:1].cpu().numpy())
            outputs = net(encoder_inputs)
            if metrics is not None:
                metrics.update(outputs if point is None else outputs[..., point],
                               target_dev[at:at + outputs.shape[0]])
                at += outputs.shape[0]
            prediction.append(outputs.detach().cpu().numpy())
        inputs = data_io.re_normalization(np.concatenate(inputs, 0), _mean, _std)
        prediction = np.concatenate(prediction, 0)
        extra = {} if quantiles is None else {"quantiles": np.asarray(quantiles, dtype=np.float32)}
        np.savez(os.path.join(params_path, 'output_epoch_%s_%s' % (global_step, type)), input=inputs,
                 prediction=prediction, data_target_tensor=data_target_tensor, **extra)
        if point is not None:
            prediction = prediction[..., point]
        if metrics is not None:
            assert data_target_tensor.shape[0] == at
            return metrics.compute()
        from sklearn.metrics import mean_absolute_error, mean_squared_error
        excel_list = []
        for i in range(prediction.shape[2]):
            assert data_target_tensor.shape[0] == prediction.shape[0]
            t, p = data_target_tensor[:, :, i], prediction[:, :, i]
            excel_list.extend([mean_absolute_error(t, p), mean_squared_error(t, p) ** 0.5,
                               data_io.masked_mape_np(t, p, 0)])
        t, p = data_target_tensor.reshape(-1, 1), prediction.reshape(-1, 1)
        excel_list.extend([mean_absolute_error(t, p), mean_squared_error(t, p) ** 0.5,
                           data_io.masked_mape_np(t, p, 0)])
    return excel_list


def build(config, device, multi_feature=None, quantiles=None):
    """Graphs + model exactly as train_DSTAGNN_my.py:62-107 (model built on CPU, then moved).
    multi_feature (None: the [Training] key, model_options()) and quantiles (None: the [Training]
    key, quantile_options(); absent: the point model) go to make_model."""
    dc, tc = config['Data'], config['Training']
    N = int(dc['num_of_vertices'])
    if dc['dataset_name'] in ['PEMS04', 'PEMS08', 'PEMS07', 'PEMS03']:
        adj_mx = data_io.get_adjacency_matrix2(dc['adj_filename'], N, id_filename=dc.get('id_filename'))
    else:
        adj_mx = data_io.load_weighted_adjacency_matrix2(dc['adj_filename'], N)
    adj_TMD = data_io.load_weighted_adjacency_matrix(dc['stag_filename'], N)
    adj_pa = data_io.load_PA(dc['strg_filename'])
    adj_mx, adj_TMD, adj_pa = torch.FloatTensor(adj_mx), torch.FloatTensor(adj_TMD), torch.FloatTensor(adj_pa)
    adj_merge = adj_mx if tc.get('graph', 'AG') == 'G' else adj_TMD
    net = make_model('cpu', int(tc['in_channels']), int(tc['nb_block']), int(tc['in_channels']), int(tc['K']),
                     int(tc['nb_chev_filter']), int(tc['nb_time_filter']), 1, adj_merge, adj_pa, adj_TMD,
                     int(dc['num_for_predict']), int(dc['len_input']), N, int(tc['d_model']), int(tc['d_k']),
                     int(tc['d_k']), int(tc['n_heads']),
                     multi_feature=model_options(tc) if multi_feature is None else bool(multi_feature),
                     quantiles=quantile_options(tc) if quantiles is None else quantiles)
    return net.to(device)


def params_path_of(config, root='myexperiments'):
    """train_DSTAGNN_my.py:115-123."""
    tc = config['Training']
    folder_dir = '{}_{}h{}d{}w_channel{}_{}'.format(tc['model_name'], tc['num_of_hours'], tc['num_of_days'],
                                                    tc['num_of_weeks'], tc['in_channels'],
                                                    float(tc['learning_rate']))
    return os.path.join(root, config['Data']['dataset_name'], folder_dir)


class HipAdam(torch.optim.Optimizer):
    """torch.optim.Adam as train_DSTAGNN_my.py:126 builds it (betas (0.9, 0.999), eps 1e-8, no
    weight decay) with the whole update in ONE launch of the library's Adam kernel
    (``dstagnn::adam_step``, csrc/optim.hip) over every parameter that has a gradient — torch's
    fused Adam takes four ~43 us launches after ~0.2 ms of host-side grouping at PEMS08
    nb_block=4.  fp32 CUDA parameters only; state per parameter as torch's Adam
    (``step``, ``exp_avg``, ``exp_avg_sq``).

    Opt-in, on the data the launch already streams (``dstagnn::adam_step_ex``; with none of them
    given the step is the single ``adam_step`` launch above, bit for bit):

    * ``max_grad_norm``: clipping by the global L2 norm, torch.nn.utils.clip_grad_norm_'s
      ``coef = min(1, max_norm / (norm + 1e-6))``.  The norm is taken ONCE per ``step()`` over
      every parameter with a gradient in ALL param groups (one ``dstagnn::grad_sumsq`` launch,
      fp64 fold) before any update launch, also where differing step counts split a group into
      several launches.  The gradients themselves are not written: the kernel uses ``coef * g``.
    * ``weight_decay`` with ``decoupled_weight_decay=False``: ``g += wd * p`` after clipping
      (torch.optim.Adam(weight_decay=)); ``True``: ``p *= 1 - lr * wd`` before the update
      (torch.optim.AdamW).
    * ``skip_nonfinite``: when the squared norm is inf / nan the update launches store nothing
      (``p``, ``exp_avg``, ``exp_avg_sq`` keep their values) and ``skipped_steps`` (a device
      int32) goes up by one.  The host never learns of it (no sync), so the per-parameter
      ``step`` counts still advance: the bias corrections of the next step are those of t + 1.

    ``grad_norm``: a 0-dim fp64 device tensor, the pre-clip global norm of the last step that
    needed it (clipping or skipping on; None before).  The new hyper-parameters live in
    ``param_groups`` (the norm is global, each group clips to its own ``max_grad_norm``) and
    travel through ``state_dict`` / ``load_state_dict``."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 decoupled_weight_decay=False, max_grad_norm=None, skip_nonfinite=False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                        decoupled_weight_decay=decoupled_weight_decay, max_grad_norm=max_grad_norm,
                        skip_nonfinite=skip_nonfinite)
        self._check_options(defaults)
        super().__init__(params, defaults)
        # per group, after a step through the grouping below: (params list, which params had a
        # gradient, and per step count — one launch each — [positions in the params list, those
        # params, their state dicts, exp_avgs, exp_avg_sqs, step]).  The per-parameter grouping
        # costs ~2 us per Parameter in Python (~0.3 ms at nb_block=4, with the GPU idle); the
        # cached path gathers the gradients and launches while the same parameters carry gradients.
        self._plans = {}
        self._sumsq = None
        self._count = True
        first = self.param_groups[0]["params"][0]
        self.skipped_steps = torch.zeros((), dtype=torch.int32, device=first.device)
        self._none = {}  # per device: (empty fp64 stat, empty int32 counter) for "not given"

    @staticmethod
    def _check_options(group):
        wd, mn = group["weight_decay"], group["max_grad_norm"]
        if not (isinstance(wd, (int, float)) and wd >= 0.0):  # (a NaN fails too)
            raise ValueError(f"HipAdam: invalid weight_decay {wd!r}")
        if mn is not None and not (isinstance(mn, (int, float)) and mn > 0.0):
            raise ValueError(f"HipAdam: invalid max_grad_norm {mn!r} (None: no clipping)")

    @property
    def grad_norm(self):
        """Element 1 of grad_sumsq's two-double buffer (the kernel stores the root beside the
        sum): a view, no launch."""
        return None if self._sumsq is None else _norm_of(self._sumsq)

    def load_state_dict(self, state_dict):
        """Accepts HipAdam's and torch.optim.Adam's / AdamW's state_dicts alike: torch keeps
        ``step`` as a (float) tensor, HipAdam as a Python int (a tensor step would key ``by_step``
        below by identity: one launch per parameter and no cached plan), so it is converted here.
        torch's groups carry ``weight_decay`` (and, newer ones, ``decoupled_weight_decay``), which
        are taken over; the options they lack keep this optimiser's defaults."""
        self._plans = {}
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize"):
                raise ValueError("HipAdam: amsgrad / maximize are not supported")
            for k, v in self.defaults.items():
                group.setdefault(k, v)
            self._check_options(group)
        for st in self.state.values():
            if "step" in st and torch.is_tensor(st["step"]):
                st["step"] = int(st["step"].item())

    def state_dict(self):
        """torch.optim.Adam's format: ``step`` as a float32 CPU tensor (the live state keeps the
        int; the returned per-parameter dicts are copies)."""
        sd = super().state_dict()
        sd["state"] = {k: (dict(v, step=torch.tensor(float(v["step"]), dtype=torch.float32))
                           if "step" in v and not torch.is_tensor(v["step"]) else v)
                       for k, v in sd["state"].items()}
        return sd

    def zero_grad(self, set_to_none=True):
        """torch's zero_grad(set_to_none=True) spends ~1 us per parameter in profiler /
        foreach bookkeeping (~0.15 ms at nb_block=4, before the forward can start); dropping
        the references is all it does here."""
        if not set_to_none:
            return super().zero_grad(set_to_none=False)
        for group in self.param_groups:
            for p in group["params"]:
                p.grad = None

    @staticmethod
    def _plain(group):
        return (group["weight_decay"] == 0.0 and group["max_grad_norm"] is None and not group["skip_nonfinite"])

    def _launch(self, ops, group, ps, gs, ms, vs, t, stat):
        """One update launch at step count t: today's ``adam_step`` when the group has no option
        on, else ``adam_step_ex``.  Of the launches of one step() the first with skip_nonfinite
        set is handed the ``skipped_steps`` counter, so a skipped step counts once."""
        b1, b2 = group["betas"]
        step_size, bc2_sqrt = group["lr"] / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)
        if self._plain(group):
            ops.adam_step(ps, gs, ms, vs, b1, b2, group["eps"], step_size, bc2_sqrt)
            return
        dev = ps[0].device
        none = self._none.get(dev)
        if none is None:
            none = self._none[dev] = (torch.empty(0, dtype=torch.float64, device=dev),
                                      torch.empty(0, dtype=torch.int32, device=dev))
        mn, skip = group["max_grad_norm"], bool(group["skip_nonfinite"])
        count = skip and self._count
        if count:
            self._count = False
            if self.skipped_steps.device != dev:
                self.skipped_steps = self.skipped_steps.to(dev)
        ops.adam_step_ex(ps, gs, ms, vs, b1, b2, group["eps"], step_size, bc2_sqrt, group["lr"],
                         float(group["weight_decay"]), bool(group["decoupled_weight_decay"]),
                         0.0 if mn is None else float(mn), skip,
                         stat if (mn is not None or skip) else none[0],
                         self.skipped_steps if count else none[1])

    def _fast_step(self, ops, group, grads, stat):
        plan = self._plans.get(id(group))
        params = group["params"]
        if plan is None or plan[0] is not params or len(plan[1]) != len(params):
            return False
        if [g is not None for g in grads] != plan[1]:
            return False
        for launch in plan[2]:
            idx, ps, states, ms, vs, t = launch
            t += 1
            self._launch(ops, group, ps, [grads[i] for i in idx], ms, vs, t, stat)
            for st in states:
                st["step"] = t
            launch[5] = t
        return True

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        from . import _lib
        ops = _lib.load()
        groups = self.param_groups
        grads = [[p.grad for p in group["params"]] for group in groups]
        stat = None
        if any(g["max_grad_norm"] is not None or g["skip_nonfinite"] for g in groups):
            every = [g for gl in grads for g in gl if g is not None]
            if every:  # the global norm: once, over all groups, before any update launch
                stat = self._sumsq = ops.grad_sumsq(every)
        self._count = True
        for group, glist in zip(groups, grads):
            if self._fast_step(ops, group, glist, stat):
                continue
            self._plans.pop(id(group), None)
            by_step = {}
            for i, (p, g) in enumerate(zip(group["params"], glist)):
                if g is None:
                    continue
                if g.is_sparse or not p.is_cuda or p.dtype != torch.float32:
                    raise RuntimeError("HipAdam: dense fp32 CUDA parameters only")
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["step"] = int(st["step"]) + 1  # (a tensor step from a foreign state_dict)
                lists = by_step.setdefault(st["step"], ([], [], [], [], []))
                lists[0].append(p if p.is_contiguous() else p.data)
                lists[1].append(g)  # a strided gradient is copied contiguous by the op
                lists[2].append(st["exp_avg"])
                lists[3].append(st["exp_avg_sq"])
                lists[4].append(i)
            for t, (ps, gs, ms, vs, _) in by_step.items():
                if any(not q.is_contiguous() for q in ps):
                    raise RuntimeError("HipAdam: non-contiguous parameter")
                self._launch(ops, group, ps, gs, ms, vs, t, stat)
            if by_step:
                present = [g is not None for g in glist]
                self._plans[id(group)] = (group["params"], present,
                                          [[idx, ps, [self.state[group["params"][i]] for i in idx], ms, vs, t]
                                           for t, (ps, _, ms, vs, idx) in by_step.items()])
        return loss


def _norm_of(sumsq):
    """The norm beside ``dstagnn::grad_sumsq``'s sum: the op returns element 0 of a two-double
    buffer and the kernel stores the root in element 1."""
    return sumsq.as_strided((), (), 1)


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm):
    """torch.nn.utils.clip_grad_norm_(parameters, max_norm) (L2: ``g *= min(1, max_norm / (norm +
    1e-6))`` over all gradients, the pre-clip norm returned) in two launches and no host sync:
    ``dstagnn::grad_sumsq`` (fp64 fold, the same bits on every call) and ``dstagnn::grad_scale``.
    For users of other optimisers; HipAdam(max_grad_norm=) clips inside its update launch.
    Returns a 0-dim fp64 device tensor.  fp32 CUDA gradients only."""
    if torch.is_tensor(parameters):
        parameters = [parameters]
    max_norm = float(max_norm)
    if not max_norm > 0.0:
        raise ValueError(f"clip_grad_norm_: invalid max_norm {max_norm!r}")
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.zeros((), dtype=torch.float64)
    from . import _lib
    ops = _lib.load()
    sumsq = ops.grad_sumsq(grads)
    ops.grad_scale(grads, sumsq, max_norm)
    return _norm_of(sumsq)


def training_options(tc):
    """Optional [Training] keys of a configuration (a ConfigParser section): ``max_grad_norm``,
    ``weight_decay``, ``decoupled_weight_decay`` -> (float or None, float, bool).  The
    reference's .conf files have none of them: (None, 0.0, False), today's behaviour."""
    mn = tc.get('max_grad_norm', None)
    return (None if mn is None else float(mn), float(tc.get('weight_decay', 0.0)),
            tc.getboolean('decoupled_weight_decay', fallback=False))


def loss_options(tc):
    """Optional [Training] keys of a configuration (a ConfigParser section): ``loss_function``,
    ``missing_value``, ``smooth_l1_beta``, ``huber_delta`` -> (str or None, float or None, float,
    float).  The reference's .conf files have none of them: (None, None, 1.0, 1.0), today's
    criterion.  ``missing_value = nan`` masks the NaN targets."""
    mv = tc.get('missing_value', None)
    return (tc.get('loss_function', None), None if mv is None else float(mv),
            float(tc.get('smooth_l1_beta', 1.0)), float(tc.get('huber_delta', 1.0)))


def input_options(tc):
    """Optional [Training] keys of a configuration (a ConfigParser section) for a series with
    gaps: ``input_fill`` (``none`` | ``mean`` | ``ffill``) and ``input_max_gap`` -> (str or None,
    int or None).  Absent, or ``none``: (None, None), today's behaviour.  What counts as missing
    is loss_options()' ``missing_value``, the value the criterion masks with."""
    fill = tc.get('input_fill', None)
    fill = None if fill is None or fill.strip().lower() == 'none' else fill.strip().lower()
    if fill is not None and fill not in ('mean', 'ffill'):
        raise ValueError(f"[Training] input_fill must be none, mean or ffill, got {fill!r}")
    gap = tc.get('input_max_gap', None)
    return fill, None if gap is None or gap.strip().lower() in ('', 'none') else int(gap)


def scoring_options(tc):
    """Optional [Training] keys of a configuration (a ConfigParser section): ``test_metrics`` and
    ``node_scores`` -> (bool, bool).  Absent: (False, False), today's behaviour (a test loss only)."""
    return tc.getboolean('test_metrics', fallback=False), tc.getboolean('node_scores', fallback=False)


def skill_options(tc, dc=None):
    """Optional [Training] keys of a configuration (a ConfigParser section): ``baseline_skill`` and
    ``climatology_period`` -> (bool, int or None).  The period defaults to the [Data] key ``period``
    (dc: that section) and is None where neither is there.  Absent: (False, ...), today's behaviour."""
    period = tc.get('climatology_period', None)
    if period is None and dc is not None:
        period = dc.get('period', None)
    try:
        period = None if period is None or not str(period).strip() else int(str(period).strip())
    except ValueError:
        raise ValueError(f"climatology_period / [Data] period must be an int, got {period!r}") from None
    return tc.getboolean('baseline_skill', fallback=False), period


def parse_event_levels(text, what="event_thresholds"):
    """``"-1.0, -1.5, -2.0"`` (or a sequence of numbers) -> (-1.0, -1.5, -2.0); ValueError for
    anything that is not a non-empty list of numbers.  The order and range rules are loss.py's
    (check_thresholds / check_percentiles)."""
    try:
        parts = str(text).replace(';', ',').split(',') if isinstance(text, str) else list(text)
        levels = tuple(float(v) for v in parts if not isinstance(v, str) or v.strip())
    except (TypeError, ValueError):
        raise ValueError(f"{what}: a comma separated list of numbers, got {text!r}") from None
    if not levels:
        raise ValueError(f"{what}: a comma separated list of numbers, got {text!r}")
    return levels


def event_options(tc):
    """Optional [Training] keys of a configuration (a ConfigParser section) for the drought event
    scores: ``event_thresholds`` (fixed thresholds in the units of the targets, e.g. ``-1.0, -1.5,
    -2.0``), ``event_percentiles`` (per-node percentiles of the training steps, e.g. ``20, 10, 5``)
    and ``event_direction`` (``below`` | ``above``) -> (tuple or None, tuple or None, str), each
    list checked by loss.check_thresholds / loss.check_percentiles under the direction.  Both
    threshold keys together is a ValueError.  Absent: (None, None, 'below'), today's behaviour."""
    return resolve_events(*_event_keys(tc))


def _event_keys(tc):
    """The three keys as written (None where absent; the direction lower-cased, 'below' by default)."""
    return (tc.get('event_thresholds', None), tc.get('event_percentiles', None),
            tc.get('event_direction', 'below').strip().lower())


def resolve_events(thresholds, percentiles, direction):
    """The three event options, from the keys, the keywords or the flags, checked on the host."""
    from .loss import check_direction, check_percentiles, check_thresholds
    check_direction(direction, "event_direction")
    if thresholds is not None and percentiles is not None:
        raise ValueError("event_thresholds and event_percentiles are two ways to define the same classes: give one")
    if thresholds is not None:
        thresholds = parse_event_levels(thresholds, "event_thresholds")
        check_thresholds(thresholds, direction, "event_thresholds")
    if percentiles is not None:
        percentiles = check_percentiles(parse_event_levels(percentiles, "event_percentiles"), direction,
                                        "event_percentiles")
    return thresholds, percentiles, direction


def model_options(tc):
    """Optional [Training] key ``multi_feature`` of a configuration (a ConfigParser section) -> bool.
    True: the first block takes all ``in_channels`` input features (model.make_model's
    multi_feature; 1 <= in_channels <= 8).  Absent: False, today's model (which fails in its first
    forward for 1 < in_channels < nb_time_filter, like the reference)."""
    return tc.getboolean('multi_feature', fallback=False)


def quantile_options(tc):
    """Optional [Training] key ``quantiles`` of a configuration (a ConfigParser section), a comma
    separated list such as ``0.1, 0.5, 0.9`` -> a tuple of levels checked by loss.check_quantiles
    (ValueError for an empty list, more than 16, a level outside (0, 1), unsorted or repeated
    levels).  Absent: None, today's point model and criterion."""
    text = tc.get('quantiles', None)
    return None if text is None else parse_quantiles(text)


def parse_quantiles(text):
    """``"0.1,0.5,0.9"`` -> (0.1, 0.5, 0.9), checked by loss.check_quantiles."""
    from .loss import check_quantiles
    try:
        levels = [float(v) for v in str(text).replace(';', ',').split(',') if v.strip()]
    except ValueError:
        raise ValueError(f"quantiles: a comma separated list of numbers, got {text!r}") from None
    return check_quantiles(levels, "quantiles")


def check_quantile_loss(name, quantiles):
    """``loss_function`` (or ``--loss``) beside ``quantiles``: only absent or ``pinball``."""
    if quantiles is not None and name is not None and name != 'pinball':
        raise ValueError(f"quantiles are trained with the pinball loss: loss_function must be absent or 'pinball' "
                         f"when quantiles are given, got {name!r}")
    if quantiles is None and name == 'pinball':
        raise ValueError("loss_function = pinball needs quantiles ([Training] quantiles or quantiles=)")


def check_input_features(F, in_channels):
    """The data's feature count against the model's ``in_channels`` (run() with multi_feature): a
    ValueError that names both, instead of a shape error out of the first forward."""
    if int(F) != int(in_channels):
        raise ValueError(f"the data has F = {int(F)} features per node but [Training] in_channels = {int(in_channels)}: "
                         f"a multi-feature model takes exactly in_channels features")


def make_criterion(name=None, missing_value=None, smooth_l1_beta=1.0, huber_delta=1.0, quantiles=None):
    """The driver's criterion.  With quantiles: loss.QuantileLoss(quantiles, null_val=missing_value)
    (the name absent or ``pinball``: check_quantile_loss).  Otherwise, as ever:
    With no name and no missing value: ``nn.SmoothL1Loss()``
    (train_DSTAGNN_my.py:132), the object every run without the keys of loss_options() has
    always used.  Any explicit name (``smooth_l1`` included) or missing value: a loss.HipLoss,
    one HIP launch per direction; a missing value alone masks the default ``smooth_l1``.  Raises
    ValueError for an unknown name and for ``masked_mae`` / ``masked_mse`` without a missing
    value."""
    check_quantile_loss(name, quantiles)
    if quantiles is not None:
        from .loss import QuantileLoss
        return QuantileLoss(quantiles, null_val=missing_value)
    if name is None and missing_value is None:
        return nn.SmoothL1Loss()
    from .loss import HipLoss
    return HipLoss('smooth_l1' if name is None else name, beta=smooth_l1_beta, delta=huber_delta,
                   null_val=missing_value)


def make_adam(params, lr, weight_decay=0.0, decoupled=False, max_grad_norm=None):
    """The driver's optimiser (train_DSTAGNN_my.py:126): HipAdam (one launch) when every
    parameter is an fp32 GPU tensor; DSTAGNN_ADAM=torch-fused / torch for torch's fused or
    default Adam (A/B).  weight_decay / decoupled / max_grad_norm: HipAdam's options; under the
    torch modes (and off the GPU) the same options as torch.optim.Adam(weight_decay=) or
    torch.optim.AdamW, and torch.nn.utils.clip_grad_norm_ in a step pre-hook (which, unlike
    HipAdam, writes the clipped gradients back)."""
    params = list(params)
    mode = os.environ.get("DSTAGNN_ADAM", "hip")
    on_gpu = bool(params) and all(p.is_cuda and p.dtype == torch.float32 for p in params)
    if on_gpu and mode == "hip":
        return HipAdam(params, lr=lr, weight_decay=weight_decay, decoupled_weight_decay=decoupled,
                       max_grad_norm=max_grad_norm)
    if weight_decay < 0.0 or (max_grad_norm is not None and not max_grad_norm > 0.0):
        raise ValueError("make_adam: invalid weight_decay / max_grad_norm")
    kw = dict(fused=True) if on_gpu and mode == "torch-fused" else {}
    if weight_decay and decoupled:
        opt = torch.optim.AdamW(params, lr=lr, weight_decay=weight_decay, **kw)
    else:
        opt = torch.optim.Adam(params, lr=lr, weight_decay=weight_decay, **kw)
    if max_grad_norm is not None:
        def clip(*_):
            torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
        opt.register_step_pre_hook(clip)
    return opt


def fit(net, train_x, train_y, val_x, val_y, *, epochs, start_epoch=0, batch_size, lr, params_path,
        double_step=True, max_batches=None, log=print, max_grad_norm=None, weight_decay=0.0,
        decoupled_weight_decay=False, criterion=None):
    """The epoch loop of train_DSTAGNN_my.py:136-178.  Returns (best_epoch, best_val, history).
    max_grad_norm / weight_decay / decoupled_weight_decay: make_adam's options (off by default,
    as in the reference).  Under data parallelism ``reducer.all_reduce()`` precedes
    ``optimizer.step()``, so the clipping norm is taken on the averaged gradients and is the
    same on every rank: the ranks clip alike and their parameters stay equal.
    criterion: training and validation loss (make_criterion(); None: ``nn.SmoothL1Loss()``).  A
    masked criterion divides by the valid count of the rank's own batch and the gradients are
    then averaged over the ranks: a mean of batch means, as the unmasked path has always been.
    train_x / train_y / val_x / val_y: HBM-resident tensors, or the ``x`` / ``y`` of
    windows.WindowedSeries splits (StreamBatches: same sample order, one gather launch per batch)."""
    rank, world = _world()
    criterion = (nn.SmoothL1Loss() if criterion is None else criterion).to(train_x.device)
    optimizer = make_adam(net.parameters(), lr, weight_decay=weight_decay, decoupled=decoupled_weight_decay,
                          max_grad_norm=max_grad_norm)
    reducer = None
    if world > 1:  # block gradients all-reduced beside the backward (attach)
        reducer = GradAllReducer(net.named_parameters(), mask_support=mask_support_of(net)).attach(net)
    loader = make_batches(train_x, train_y, batch_size, True, rank, world)

    def optimizer_step(reduce=True):  # xm.optimizer_step
        if reducer is not None and reduce:
            reducer.all_reduce()
        optimizer.step()  # (the global-norm clip, if any, after the all-reduce)

    best_val, best_epoch, history = float('inf'), 0, []
    for epoch in range(start_epoch, epochs):
        net.train()
        t0 = time.time()
        total = torch.zeros((), dtype=torch.float64, device=train_x.device)
        nb = 0
        for batch_idx, (encoder_inputs, labels) in enumerate(loader):
            if max_batches is not None and batch_idx >= max_batches:
                break
            if double_step:
                optimizer_step(reduce=False)  # :148 re-applies the (already reduced) previous grads
            optimizer.zero_grad()
            loss = criterion(net(encoder_inputs), labels)
            loss.backward()
            optimizer_step()
            total += loss.detach().double()
            nb += 1
        net.eval()
        val = eval_batches(net, val_x, val_y, batch_size, criterion)
        history.append({"epoch": epoch, "train_loss": float(total) / max(1, nb), "val_loss": val,
                        "time_s": time.time() - t0, "batches": nb})
        if rank == 0:
            log(f'Epoch {epoch} Val Loss: {val:.4f} Time: {time.time() - t0:.2f}s')
            if val < best_val:
                best_val, best_epoch = val, epoch
                torch.save({k: v.detach().cpu() for k, v in net.state_dict().items()},
                           os.path.join(params_path, f'epoch_{epoch}.params'))
        elif val < best_val:
            best_val, best_epoch = val, epoch
    return best_epoch, best_val, history


def load_best(net, path):
    """train_DSTAGNN_my.py:184 (torch.load of the best checkpoint).  Only rank 0 wrote the file
    and only rank 0 reads it; the other ranks receive its tensors by broadcast (no shared
    filesystem assumed)."""
    rank, world = _world()
    if rank == 0:
        net.load_state_dict(torch.load(path, weights_only=True))
    if world > 1:
        with torch.no_grad():
            for t in net.state_dict().values():
                dist.broadcast(t, src=0)


def run(config_path, *, epochs=None, double_step=True, dropout=None, max_batches=None, root='myexperiments',
        log=print, max_grad_norm=None, weight_decay=None, loss=None, missing_value=None, stream_windows=None,
        input_fill=None, input_max_gap=None, test_metrics=None, node_scores=None, multi_feature=None,
        quantiles=None, baseline_skill=None, climatology_period=None, event_thresholds=None, event_percentiles=None,
        event_direction=None):
    """Whole script: data, graphs, model, training, best-checkpoint test loss.  The optional
    [Training] keys of training_options() switch clipping / weight decay on; max_grad_norm /
    weight_decay given here override them.  loss / missing_value override the keys of
    loss_options() the same way; the criterion make_criterion() builds from them is used for
    training, validation and the final test loss.
    stream_windows (None: the [Training] key ``stream_windows``, off when absent): read the raw
    ``graph_signal_matrix_filename`` instead of the prepared ``*_dstagnn.npz``, keep it on the
    device once and gather every batch's windows from it (windows.WindowedSeries); none of the
    materialised arrays is read or built.  Where the prepared file exists only its ``mean`` and
    ``std`` are read, and the run sees the inputs of the materialised run bit for bit; otherwise
    the statistics are computed on the device from the raw series.
    input_fill / input_max_gap override the keys of input_options(): with ``mean`` or ``ffill`` the
    inputs equal to the missing value (the criterion's) are imputed inside the gather launch and
    the z-score statistics are those of the observed values, always computed on the device (a
    prepared file's would be NaN or polluted by the sentinel).  Needs a missing value and
    stream_windows (the materialised path has no imputation): ValueError otherwise.
    test_metrics / node_scores (None: the [Training] keys of scoring_options(), off when absent):
    after the final test loss the test split is scored with the best checkpoint (score_batches:
    MAE / RMSE / MAPE / bias / NSE per horizon and overall, masked by the run's missing value when
    there is one; with node_scores also per node, which implies test_metrics).  Rank 0 logs one
    line per horizon and one overall and writes ``test_metrics.json`` (and
    ``test_node_scores.npz``) into the params path; the returned dict gains ``test_metrics`` (the
    list of predict_and_save_results_mstgcn), ``test_scores`` and ``test_node_scores``.
    multi_feature (None: the [Training] key of model_options(), off when absent): the model's first
    block takes all ``in_channels`` features of the data (both data paths feed (B, N, F, T));
    ValueError when the data's F differs from in_channels.
    quantiles (None: the [Training] key of quantile_options(), absent: a point model): a tuple of
    levels or a ``"0.1,0.5,0.9"`` string.  The model gets a quantile head, the criterion is
    loss.QuantileLoss(levels, null_val=missing_value) for training, validation and test loss (a
    loss name other than ``pinball`` beside it is a ValueError, raised before any data is read), and
    with test_metrics the existing scores are taken from the ``point_index`` column (same keys and
    files) while the result gains ``test_quantile_scores`` (and ``test_node_quantile_scores`` with
    node_scores), written as ``test_quantile_scores.json`` (and ``test_node_quantile_scores.npz``).
    baseline_skill / climatology_period (None: the [Training] keys of skill_options(); the period
    defaults to the [Data] key ``period``): in the same scoring pass the test split is also scored
    against persistence and the seasonal climatology of the training steps (loss.BaselineSkill,
    masked by the run's missing value; a quantile model's ``point_index`` column).  Implies
    test_metrics and needs stream_windows (the materialised path keeps no raw series on the
    device): ValueError otherwise, and for a missing period or one outside [1, L], before any data
    is read where the configuration already shows it.  Rank 0 logs one line per horizon and one
    overall (``mse_skill_persistence``, ``mse_skill_climatology``, ``acc``) and writes
    ``test_skill.json`` (with node_scores also ``test_node_skill.npz``); the result gains
    ``test_skill`` (and ``test_node_skill``).
    event_thresholds / event_percentiles / event_direction (None: the [Training] keys of
    event_options()): in the same scoring pass the test split is also scored as a drought event
    forecast (loss.EventScores, masked by the run's missing value; a quantile model's ``point_index``
    column): fixed thresholds in the units of the targets, or per-node percentiles of the training
    steps (loss.node_percentile_thresholds).  A threshold keyword replaces both threshold keys;
    giving both is a ValueError.  Either implies test_metrics; the percentiles need stream_windows
    (the materialised path keeps no raw series): ValueError before any data is read.  Rank 0 logs
    one ``Test events`` line per horizon and one overall (pod / far / csi / hss per threshold and
    ``hss_multi``) and the number of excluded nodes, and writes ``test_event_scores.json`` (with
    node_scores also ``test_node_event_scores.npz``); the result gains ``test_event_scores`` (and
    ``test_node_event_scores``)."""
    config = configparser.ConfigParser()
    config.read(config_path)
    dc, tc = config['Data'], config['Training']
    rank, world = _world()
    device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
    seed_torch(1)
    if stream_windows is None:
        stream_windows = tc.getboolean('stream_windows', fallback=False)
    cfg_loss, cfg_missing, beta, delta = loss_options(tc)
    missing_value = cfg_missing if missing_value is None else missing_value
    if quantiles is None:
        quantiles = quantile_options(tc)
    elif isinstance(quantiles, str):
        quantiles = parse_quantiles(quantiles)
    else:
        from .loss import check_quantiles
        quantiles = check_quantiles(quantiles, "quantiles")
    check_quantile_loss(cfg_loss if loss is None else loss, quantiles)
    cfg_scores, cfg_nodes = scoring_options(tc)
    node_scores = cfg_nodes if node_scores is None else bool(node_scores)
    test_metrics = (cfg_scores if test_metrics is None else bool(test_metrics)) or node_scores
    cfg_skill, cfg_period = skill_options(tc, dc)
    baseline_skill = cfg_skill if baseline_skill is None else bool(baseline_skill)
    climatology_period = cfg_period if climatology_period is None else climatology_period
    if baseline_skill:
        test_metrics = True
        if not stream_windows:
            raise ValueError("baseline_skill needs stream_windows: the materialised path keeps no raw series on "
                             "the device to read the baselines from")
        if climatology_period is None or isinstance(climatology_period, bool) or \
                climatology_period != int(climatology_period) or int(climatology_period) < 1:
            raise ValueError("baseline_skill needs a climatology period >= 1 ([Training] climatology_period, [Data] "
                             f"period or climatology_period=), got {climatology_period!r}")
    cfg_thr, cfg_pct, cfg_dir = _event_keys(tc)  # (checked below, under the direction that holds)
    if event_thresholds is not None or event_percentiles is not None:
        cfg_thr = cfg_pct = None  # a threshold keyword replaces the keys' definition
    event_thresholds, event_percentiles, event_direction = resolve_events(
        cfg_thr if event_thresholds is None else event_thresholds,
        cfg_pct if event_percentiles is None else event_percentiles,
        cfg_dir if event_direction is None else str(event_direction).strip().lower())
    if event_thresholds is not None or event_percentiles is not None:
        test_metrics = True
        if event_percentiles is not None and not stream_windows:
            raise ValueError("event_percentiles needs stream_windows: the materialised path keeps no raw series on "
                             "the device to take the percentiles of (fixed event_thresholds work on both paths)")
    cfg_fill, cfg_gap = input_options(tc)
    input_fill = cfg_fill if input_fill is None else (None if str(input_fill).lower() == 'none' else input_fill)
    input_max_gap = cfg_gap if input_max_gap is None else input_max_gap
    if input_fill is not None:
        if missing_value is None:
            raise ValueError("input_fill needs a missing value ([Training] missing_value or missing_value=)")
        if not stream_windows:
            raise ValueError("input_fill needs stream_windows: the materialised path has no imputation")
    if stream_windows:
        ws = _windowed_series(dc, tc, device, missing_value if input_fill is not None else None, input_fill,
                              input_max_gap)
        if input_fill is not None and rank == 0:
            log(f'Input gaps (fill {input_fill}, max_gap {input_max_gap}): missing per feature '
                f'{ws.missing_count.tolist()}, filled per feature {ws.filled_count.tolist()}')
        if baseline_skill:  # refused here, before the training it would otherwise follow
            from .loss import check_period
            climatology_period = check_period(climatology_period, ws.L, "baseline_skill")
        (train_x, train_y), (val_x, val_y), (test_x, test_y) = ((ws.split(k).x, ws.split(k).y)
                                                                for k in ('train', 'val', 'test'))
        # the reference's one-batch probe (:59-61): its draws from the global RNG do not depend on the data
        next(iter(torch.utils.data.DataLoader(torch.arange(train_x.shape[0]), batch_size=int(tc['batch_size']),
                                              shuffle=True)))
    else:
        (train_x, train_loader, train_y, val_x, _, val_y, test_x, _, test_y, mean, std) = \
            data_io.load_graphdata_channel1(dc['graph_signal_matrix_filename'], int(tc['num_of_hours']),
                                            int(tc['num_of_days']), int(tc['num_of_weeks']), 'cpu',
                                            int(tc['batch_size']))
        next(iter(train_loader))  # the reference probes one batch (:59-61): same RNG draw before the init
    multi_feature = model_options(tc) if multi_feature is None else bool(multi_feature)
    if multi_feature:
        check_input_features(train_x.shape[2], tc['in_channels'])
    net = build(config, device, multi_feature, quantiles)
    set_direct_grads(net)  # the loop only uses loss.backward() + .grad
    if dropout is not None:
        set_dropout(net, dropout)
    if not stream_windows:
        train_x, train_y, val_x, val_y, test_x, test_y = (t.to(device) for t in
                                                          (train_x, train_y, val_x, val_y, test_x, test_y))
    params_path = params_path_of(config, root)
    if rank == 0:
        os.makedirs(params_path, exist_ok=True)
        log(f'Params path: {params_path}')
    bs = int(tc['batch_size'])
    n_epochs = int(tc['epochs']) if epochs is None else int(epochs)
    cfg_norm, cfg_wd, decoupled = training_options(tc)
    criterion = make_criterion(cfg_loss if loss is None else loss, missing_value, beta, delta, quantiles)
    best_epoch, best_val, history = fit(net, train_x, train_y, val_x, val_y, epochs=n_epochs,
                                        start_epoch=int(tc['start_epoch']), batch_size=bs,
                                        lr=float(tc['learning_rate']), params_path=params_path,
                                        double_step=double_step, max_batches=max_batches, log=log,
                                        max_grad_norm=cfg_norm if max_grad_norm is None else max_grad_norm,
                                        weight_decay=cfg_wd if weight_decay is None else weight_decay,
                                        decoupled_weight_decay=decoupled, criterion=criterion)
    load_best(net, os.path.join(params_path, f'epoch_{best_epoch}.params'))
    net.eval()
    test_loss = eval_batches(net, test_x, test_y, bs, criterion)
    if rank == 0:
        log(f'Final Test Loss: {test_loss:.4f}')
    result = {"best_epoch": best_epoch, "best_val": best_val, "test_loss": test_loss, "history": history,
              "params_path": params_path, "net": net}
    if test_metrics:
        skill = None
        if baseline_skill:
            from .loss import BaselineSkill
            skill = BaselineSkill(ws, climatology_period, missing_value=missing_value,
                                  num_nodes=ws.N if node_scores else None)
        events = None
        if event_thresholds is not None or event_percentiles is not None:
            from .loss import EventScores, node_percentile_thresholds
            thr = event_thresholds if event_percentiles is None else node_percentile_thresholds(
                ws, event_percentiles, direction=event_direction, missing_value=missing_value)
            events = EventScores(test_y.shape[-1], thr, direction=event_direction, missing_value=missing_value,
                                 num_nodes=test_y.shape[-2] if node_scores else None, device=device)
        result.update(_score_test_split(net, test_x, test_y, bs, missing_value, node_scores, params_path, log,
                                        quantiles, skill, events))
    return result


def _score_test_split(net, test_x, test_y, bs, missing_value, per_node, params_path, log, quantiles=None, skill=None,
                      events=None):
    """run()'s test-set scores: score_batches, rank 0's log lines and files, the result keys.  With
    quantiles the point scores come from the ``point_index`` column and the calibration scores are
    logged (coverage per level and mean pinball, one line per horizon) and written beside them.
    With skill (a loss.BaselineSkill, fed in the same pass): ``test_skill`` (and ``test_node_skill``),
    one ``Test skill`` line per horizon and one overall, ``test_skill.json`` (``test_node_skill.npz``).
    With events (a loss.EventScores, fed in the same pass): ``test_event_scores`` (and
    ``test_node_event_scores``), one ``Test events`` line per horizon and one overall, the number of
    excluded nodes, ``test_event_scores.json`` (the scores, the direction, the thresholds; per-node
    thresholds as their shape only) and ``test_node_event_scores.npz`` (with ``thresholds`` and
    ``excluded``)."""
    import json
    rank, _ = _world()
    metrics, qm = score_batches(net, test_x, test_y, bs, missing_value, per_node, quantiles, skill, events), None
    if quantiles is not None:
        metrics, qm = metrics
    excel_list, scores = metrics.compute(), metrics.scores()
    out = {"test_metrics": excel_list, "test_scores": scores}
    if per_node:
        out["test_node_scores"] = metrics.node_scores()
    if rank == 0:
        for i in range(metrics.P + 1):
            log('Test %s: ' % ('overall' if i == metrics.P else 'horizon %d' % i)
                + ' '.join('%s %.4f' % (k, v[i]) for k, v in scores.items()))
        with open(os.path.join(params_path, 'test_metrics.json'), 'w') as f:
            json.dump(dict({k: v.tolist() for k, v in scores.items()}, list=excel_list), f, indent=1)
        if per_node:
            np.savez(os.path.join(params_path, 'test_node_scores.npz'), **out["test_node_scores"])
    if qm is not None:
        qs = out["test_quantile_scores"] = qm.scores()
        if per_node:
            out["test_node_quantile_scores"] = qm.node_scores()
        if rank == 0:
            for i in range(qm.P + 1):
                log('Test quantiles %s: ' % ('overall' if i == qm.P else 'horizon %d' % i)
                    + ' '.join('coverage[%g] %.4f' % (tau, qs["coverage"][i, q]) for q, tau in enumerate(qm.quantiles))
                    + ' mean_pinball %.4f' % qs["mean_pinball"][i])
            with open(os.path.join(params_path, 'test_quantile_scores.json'), 'w') as f:
                json.dump(dict({k: v.tolist() for k, v in qs.items()}, quantiles=list(qm.quantiles),
                               point_index=qm.point_index), f, indent=1)
            if per_node:
                np.savez(os.path.join(params_path, 'test_node_quantile_scores.npz'),
                         **out["test_node_quantile_scores"])
    if skill is not None:
        ss = out["test_skill"] = skill.scores()
        if per_node:
            out["test_node_skill"] = skill.node_scores()
        if rank == 0:
            for i in range(skill.P + 1):
                log('Test skill %s: ' % ('overall' if i == skill.P else 'horizon %d' % i)
                    + ' '.join('%s %.4f' % (k, ss[k][i]) for k in ('mse_skill_persistence', 'mse_skill_climatology',
                                                                  'acc')))
            with open(os.path.join(params_path, 'test_skill.json'), 'w') as f:
                json.dump(dict({k: v.tolist() for k, v in ss.items()}, period=skill.period), f, indent=1)
            if per_node:
                np.savez(os.path.join(params_path, 'test_node_skill.npz'), **out["test_node_skill"])
    if events is not None:
        es = out["test_event_scores"] = events.scores()
        if per_node:
            out["test_node_event_scores"] = events.node_scores()
        if rank == 0:
            thr, excluded = events.thresholds, events.excluded
            names = ['%g' % v for v in thr] if thr.ndim == 1 else ['#%d' % k for k in range(events.K)]
            for i in range(events.P + 1):
                log('Test events %s: ' % ('overall' if i == events.P else 'horizon %d' % i)
                    + ' '.join('%s[%s] %.4f' % (s, name, es[s][i, k]) for k, name in enumerate(names)
                               for s in ('pod', 'far', 'csi', 'hss'))
                    + ' hss_multi %.4f' % es["hss_multi"][i])
            if excluded is not None:
                log('Test events: %d of %d nodes excluded (no observed training value)'
                    % (int(excluded.sum()), excluded.size))
            with open(os.path.join(params_path, 'test_event_scores.json'), 'w') as f:
                json.dump(dict({k: v.tolist() for k, v in es.items()}, direction=events.direction,
                               thresholds=thr.tolist() if thr.ndim == 1 else {"shape": list(thr.shape)}), f, indent=1)
            if per_node:
                np.savez(os.path.join(params_path, 'test_node_event_scores.npz'), thresholds=thr,
                         excluded=np.zeros(0, dtype=bool) if excluded is None else excluded,
                         **out["test_node_event_scores"])
    return out


def _windowed_series(dc, tc, device, missing_value=None, fill=None, max_gap=None):
    """The configuration's raw series as a windows.WindowedSeries; the prepared file's mean / std
    where that file exists (np.load reads an .npz per key: the materialised arrays stay on disk).
    With a fill (input_options()) that file is not read: its statistics include the gaps."""
    from .windows import WindowedSeries
    raw = dc['graph_signal_matrix_filename']
    nh, nd, nw = int(tc['num_of_hours']), int(tc['num_of_days']), int(tc['num_of_weeks'])
    prepared, stats = data_io.dataset_filename(raw, nh, nd, nw) + '.npz', None
    if fill is not None:
        return WindowedSeries.from_file(raw, nw, nd, nh, int(dc['num_for_predict']),
                                        points_per_hour=int(dc['points_per_hour']), device=device,
                                        missing_value=missing_value, fill=fill, max_gap=max_gap)
    if os.path.exists(prepared):
        with np.load(prepared) as f:
            stats = (f['mean'], f['std'])
    return WindowedSeries.from_file(raw, nw, nd, nh, int(dc['num_for_predict']),
                                    points_per_hour=int(dc['points_per_hour']), device=device, stats=stats)


def arg_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default='configurations/PEMS04_dstagnn.conf', type=str)
    ap.add_argument("--epochs", type=int, default=None, help="override [Training] epochs")
    ap.add_argument("--max-batches", type=int, default=None, help="cap the training batches per epoch")
    ap.add_argument("--no-double-step", action="store_true",
                    help="one optimizer step per batch (the reference steps twice: quirk 14)")
    ap.add_argument("--dropout", type=float, default=None, help="override the blocks' Dropout(0.05)")
    ap.add_argument("--out-root", default="myexperiments")
    ap.add_argument("--max-grad-norm", type=float, default=None,
                    help="clip the gradients to this global L2 norm (overrides [Training] max_grad_norm)")
    ap.add_argument("--weight-decay", type=float, default=None,
                    help="Adam weight decay (overrides [Training] weight_decay; AdamW style with "
                         "[Training] decoupled_weight_decay = true)")
    ap.add_argument("--loss", default=None,
                    help="criterion on the HIP path: smooth_l1, huber, mae, mse, masked_mae, masked_mse "
                         "(overrides [Training] loss_function; default: torch's SmoothL1Loss)")
    ap.add_argument("--missing-value", type=float, default=None,
                    help="targets equal to this value (nan: NaN targets) are left out of the loss and its "
                         "gradient (overrides [Training] missing_value)")
    ap.add_argument("--stream-windows", action="store_true", default=None,
                    help="cut every batch's windows from the raw series on the device instead of loading the "
                         "prepared *_dstagnn.npz (overrides [Training] stream_windows)")
    ap.add_argument("--input-fill", default=None, choices=("none", "mean", "ffill"),
                    help="with --stream-windows and a missing value: impute the missing inputs inside the gather "
                         "launch, by the training mean or the last observed value (overrides [Training] input_fill)")
    ap.add_argument("--input-max-gap", type=int, default=None,
                    help="the furthest, in time steps, --input-fill ffill carries a value (overrides [Training] "
                         "input_max_gap; default: any distance)")
    ap.add_argument("--test-metrics", action="store_true", default=None,
                    help="after the final test loss, score the test split with the best checkpoint: MAE / RMSE / "
                         "MAPE / bias / NSE per horizon and overall, masked by the missing value when there is one "
                         "(overrides [Training] test_metrics)")
    ap.add_argument("--node-scores", action="store_true", default=None,
                    help="also score every node over all samples and horizons (test_node_scores.npz; implies "
                         "--test-metrics; overrides [Training] node_scores)")
    ap.add_argument("--multi-feature", action="store_true", default=None,
                    help="the first block takes all in_channels input features (1 <= in_channels <= 8) instead of "
                         "failing for 1 < in_channels < nb_time_filter (overrides [Training] multi_feature)")
    ap.add_argument("--quantiles", default=None,
                    help="comma separated quantile levels, e.g. 0.1,0.5,0.9: a quantile head trained with the pinball "
                         "loss; --test-metrics then also reports coverage, pinball, interval width and crossing rate "
                         "(overrides [Training] quantiles)")
    ap.add_argument("--baseline-skill", action="store_true", default=None,
                    help="with --stream-windows: also score the test split against persistence and the seasonal "
                         "climatology (MSE / MAE skill, anomaly correlation; test_skill.json; implies --test-metrics; "
                         "overrides [Training] baseline_skill)")
    ap.add_argument("--climatology-period", type=int, default=None,
                    help="steps of the seasonal cycle of --baseline-skill (overrides [Training] climatology_period; "
                         "default: [Data] period)")
    ap.add_argument("--event-thresholds", default=None,
                    help="comma separated drought thresholds in the units of the targets, mildest first, e.g. "
                         "--event-thresholds=-1.0,-1.5,-2.0 (with '=': the list starts with a minus sign): also score the test split as an event forecast (POD, FAR, CSI, HSS, the class "
                         "confusion matrix; test_event_scores.json; implies --test-metrics; overrides [Training] "
                         "event_thresholds)")
    ap.add_argument("--event-percentiles", default=None,
                    help="with --stream-windows: the thresholds are these percentiles of each node's own training "
                         "steps, mildest first, e.g. 20,10,5 (overrides [Training] event_percentiles)")
    ap.add_argument("--event-direction", default=None, choices=("below", "above"),
                    help="an event is a value at or below (default) or at or above its threshold (overrides "
                         "[Training] event_direction)")
    return ap


def main(argv=None):
    a = arg_parser().parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        local = int(os.environ.get("LOCAL_RANK", "0"))
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    try:
        run(a.config, epochs=a.epochs, double_step=not a.no_double_step, dropout=a.dropout,
            max_batches=a.max_batches, root=a.out_root, max_grad_norm=a.max_grad_norm,
            weight_decay=a.weight_decay, loss=a.loss, missing_value=a.missing_value,
            stream_windows=a.stream_windows, input_fill=a.input_fill, input_max_gap=a.input_max_gap,
            test_metrics=a.test_metrics, node_scores=a.node_scores, multi_feature=a.multi_feature,
            quantiles=a.quantiles, baseline_skill=a.baseline_skill, climatology_period=a.climatology_period,
            event_thresholds=a.event_thresholds, event_percentiles=a.event_percentiles,
            event_direction=a.event_direction)
    finally:
        if world > 1:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
