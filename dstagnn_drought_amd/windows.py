"""Training windows cut from the raw series on the device, per batch (csrc/windows.hip).

The reference windows the whole series on the host once (prepareData.py:63-147), stores every
time step once per window that contains it (``len_input`` copies: 12 at the PEMS configurations,
144 at GAMBIA) and copies all of that to the device (lib/utils1.py:294-343).  ``WindowedSeries``
keeps the raw ``(L, N, F)`` series in HBM once instead and gathers each batch's
``x (B, N, F, Tin)`` and ``y (B, N, P)`` from it in one launch, which also transposes and applies
the z-score.  Label positions, window offsets and the 60/20/20 split are
``read_and_generate_dataset``'s own arithmetic; the values are its values bit for bit when given
its statistics (``stats=``), and to fp64 rounding when the statistics are computed here
(``window_stats``: numpy's own fp32 statistics of an fp32 series are ~1e-6 off the fp64 value).

Series with gaps (``missing_value=``): a missing input would otherwise reach the model as NaN (or as
a z-scored sentinel) and one NaN in the training windows would make every statistic NaN.  With a
missing value set the statistics are taken over the observed values only
(``window_stats_masked``), a missing input is imputed inside the gather launch
(``window_gather_masked``: the training mean, i.e. exactly 0 after the z-score, or, with
``fill='ffill'``, the last observed value of that node and feature, forward-filled once at
construction by ``window_fill_forward``), and the targets stay raw so that a masked criterion
(loss.HipLoss) leaves them out.

The host side (tables, weights, checks) needs no device; the gather and the statistics run only
on the HIP path: there is no CPU fallback.
"""
import numpy as np
import torch

from . import _lib
from .data import _valid_labels

HIP_ONLY = ("dstagnn_drought_amd: WindowedSeries gathers on the MI355X HIP path only; "
            "give it a 'cuda' (HIP) device. There is no CPU fallback.")
SPLITS = ("train", "val", "test")


def window_offsets(num_of_weeks, num_of_days, num_of_hours, num_for_predict, points_per_hour=1):
    """``rel`` (Tin,) int32: the time offsets of an input window relative to its label position,
    in the order read_and_generate_dataset concatenates them (its ``tsteps``): the enabled kinds
    week, day, hour, each kind's windows oldest first.  An offset is >= 0 where
    ``points_per_hour * units < num_for_predict`` (the window overlaps the target)."""
    comps = [(d, u) for d, u in ((num_of_weeks, 7 * 24), (num_of_days, 24), (num_of_hours, 1)) if d > 0]
    starts = [-points_per_hour * u * np.arange(d, 0, -1, dtype=np.int64) for d, u in comps]
    if not starts:
        return np.zeros(0, dtype=np.int32)
    rel = (np.concatenate(starts)[:, None] + np.arange(num_for_predict, dtype=np.int64)[None, :]).reshape(-1)
    return rel.astype(np.int32)


def check_offsets(L, labels, rel, num_for_predict):
    """Every time step a gather would read lies in [0, L): ``label + rel[t]`` and
    ``label + p``, p < num_for_predict, for every label.  ValueError otherwise: the tables are
    refused here, on the host, and the kernel never sees them."""
    labels, rel = np.asarray(labels, dtype=np.int64), np.asarray(rel, dtype=np.int64)
    if labels.size == 0 or rel.size == 0:
        return
    lo = int(labels.min()) + min(int(rel.min()), 0)
    hi = int(labels.max()) + max(int(rel.max()), int(num_for_predict) - 1)
    if lo < 0 or hi >= int(L):
        raise ValueError(f"WindowedSeries: the windows reach time steps {lo} .. {hi}, outside the series' "
                         f"[0, {int(L)})")


def window_tables(L, num_of_weeks, num_of_days, num_of_hours, num_for_predict, points_per_hour=1):
    """(labels {split: (S,) int64}, rel (Tin,) int32) of a series of L steps: the label positions
    read_and_generate_dataset keeps (data._valid_labels), cut 60/20/20 in its way; the same
    ValueError where a split would be empty."""
    labels, _ = _valid_labels(int(L), num_of_weeks, num_of_days, num_of_hours, num_for_predict, points_per_hour)
    rel = window_offsets(num_of_weeks, num_of_days, num_of_hours, num_for_predict, points_per_hour)
    S = len(labels)
    s1, s2 = int(S * 0.6), int(S * 0.8)
    if rel.size == 0 or s1 == 0 or s2 == s1 or S == s2:
        raise ValueError("need at least one sample in each of the train / val / test splits "
                         "(the reference fails in np.concatenate)")
    check_offsets(L, labels, rel, num_for_predict)
    return {"train": labels[:s1], "val": labels[s1:s2], "test": labels[s2:]}, rel


def window_weights(L, labels, rel):
    """``w`` (L,) int32: how many (label, window offset) pairs land on each time step.  The
    mean / std over the windows of these labels are the w-weighted moments of the raw series."""
    labels, rel = np.asarray(labels, dtype=np.int64), np.asarray(rel, dtype=np.int64)
    w = np.zeros(int(L), dtype=np.int64)
    for r in rel:  # Tin slices of S: no (S, Tin) table
        w[labels + r] += 1  # (labels are distinct: no repeated index within one slice)
    if w.max(initial=0) >= 2 ** 31:
        raise ValueError("WindowedSeries: a time step is used by 2^31 or more windows")
    return w.astype(np.int32)


FILLS = ("mean", "ffill")


def check_missing_options(missing_value, fill='mean', max_gap=None):
    """The gap options of WindowedSeries, checked on the host: (missing value as a float, fill,
    max_gap or None); (None, None, None) without a missing value (fill and max_gap are then
    ignored).  ValueError for an unknown fill, a max_gap that is not an int >= 1 or that comes with
    fill='mean', and a numeric missing value float32 does not hold exactly (the fp32 targets must
    still equal it for the loss to mask them)."""
    if missing_value is None:
        return None, None, None
    mv = float(missing_value)
    if mv == mv and float(np.float32(mv)) != mv:
        raise ValueError(f"WindowedSeries: missing_value {mv!r} is not exactly representable in float32; the "
                         "float32 targets would no longer equal it")
    if fill not in FILLS:
        raise ValueError(f"WindowedSeries: fill must be one of {', '.join(map(repr, FILLS))}, got {fill!r}")
    if max_gap is not None:
        if isinstance(max_gap, bool) or not isinstance(max_gap, (int, np.integer)) or int(max_gap) < 1:
            raise ValueError(f"WindowedSeries: max_gap must be None or an int >= 1, got {max_gap!r}")
        if fill != "ffill":
            raise ValueError("WindowedSeries: max_gap limits the forward fill; it needs fill='ffill'")
        max_gap = int(max_gap)
    return mv, fill, max_gap


class _SplitArray:
    """``x`` or ``y`` of a split as the training loop uses a tensor: ``shape``, ``device``,
    ``dtype``, ``len``, ``index_select(0, idx)`` and first-axis slicing, each a gather launch
    that returns a real tensor."""

    def __init__(self, owner, name, which, shape):
        self.owner, self.name, self.which, self.shape = owner, name, which, torch.Size(shape)
        self.device, self.dtype = owner.device, torch.float32

    def __len__(self):
        return self.shape[0]

    def index_select(self, dim, idx):
        if dim != 0:
            raise ValueError("a windowed split selects on axis 0 only")
        return self.owner.batch(self.name, idx)[self.which]

    def __getitem__(self, key):
        if not isinstance(key, slice):
            raise TypeError("a windowed split is sliced on axis 0 (or index_select(0, idx))")
        return self.owner.batch(self.name, key)[self.which]


class WindowSplit:
    """One of train / val / test: ``x`` (S, N, F, Tin) and ``y`` (S, N, P) (_SplitArray), the
    label positions ``timestamp`` (S, 1) as the prepared file stores them, and
    ``batch(idx) -> (x, y)`` from one launch."""

    def __init__(self, owner, name):
        self.owner, self.name = owner, name
        S = len(owner.labels[name])
        self.x = _SplitArray(owner, name, 0, (S, owner.N, owner.F, owner.Tin))
        self.y = _SplitArray(owner, name, 1, (S, owner.N, owner.P))
        self.timestamp = owner.labels[name][:, None]

    def __len__(self):
        return self.x.shape[0]

    def batch(self, idx):
        return self.owner.batch(self.name, idx)


class WindowedSeries:
    """The raw series on the device once, batches gathered from it.

    series: (L, N, F) array (a (L, N, 1, F) one is squeezed as the reference does), float32 or
    float64 (kept in that dtype: the z-score is computed in it, as numpy does; any other dtype is
    converted to float64).  The window arguments are read_and_generate_dataset's.
    stats=(mean, std): per-feature statistics to use, any shape with F values (a prepared file's
    ``mean`` / ``std``): the batches then equal that file's arrays bit for bit.  stats=None: the
    training windows' mean and std (ddof 0), computed on the device in fp64 from the raw series
    (``dstagnn::window_stats``) and cast to the series' dtype.
    ``mean`` / ``std``: (1, 1, F, 1) numpy arrays, the prepared file's layout (device values
    copied back on first use).

    missing_value=None: no gap handling (fill and max_gap are ignored).  A number or NaN: the
    elements equal to it (NaN: the NaN elements) are missing.  The statistics (stats=None) are then
    those of the observed values in the training windows (``dstagnn::window_stats_masked``; a
    feature with none is a ValueError), a missing input is imputed in the gather launch
    (``dstagnn::window_gather_masked``) and the targets keep the marker for a masked criterion.
    fill='mean': a missing input becomes exactly 0.0, the training mean.  fill='ffill': it takes
    the latest observed value of its node and feature at an earlier step of the whole series, at
    most max_gap steps back (None: any distance), from one ``dstagnn::window_fill_forward`` at
    construction; what that cannot fill becomes 0.0.  Nothing is ever taken from a later step.
    ``valid_weight`` (F,) int64: the statistics' divisor per feature (None without a missing value
    or with stats=); ``missing_count`` / ``filled_count`` (F,) int64: the series' missing elements
    per feature and how many of them the forward fill replaced (zeros under fill='mean');
    ``filled``: the forward-filled series on the device (fill='ffill'), else None."""

    def __init__(self, series, num_of_weeks, num_of_days, num_of_hours, num_for_predict, points_per_hour=1,
                 device=None, stats=None, missing_value=None, fill='mean', max_gap=None):
        series = np.asarray(series)
        if series.ndim == 4:
            series = series.squeeze(axis=2)
        if series.ndim != 3:
            raise ValueError(f"WindowedSeries: the series must be (L, N, F), got {series.shape}")
        if series.dtype not in (np.float32, np.float64):
            series = series.astype(np.float64)
        self.L, self.N, self.F = (int(v) for v in series.shape)
        self.P = int(num_for_predict)
        # host tables first: every ValueError is raised before the device is touched
        self.labels, self.rel = window_tables(self.L, num_of_weeks, num_of_days, num_of_hours, self.P,
                                              points_per_hour)
        self.Tin = int(self.rel.size)
        if stats is not None:
            mean, std = (np.asarray(s).reshape(-1) for s in stats)
            if mean.size != self.F or std.size != self.F:
                raise ValueError(f"WindowedSeries: stats must hold F = {self.F} values each, got {mean.size} "
                                 f"and {std.size}")
        self.missing_value, self.fill, self.max_gap = check_missing_options(missing_value, fill, max_gap)
        self.valid_weight = self.missing_count = self.filled_count = self.filled = None
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError(HIP_ONLY)
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(HIP_ONLY)
        self._ops = _lib.load()
        dev = self.device
        self.series = torch.from_numpy(np.ascontiguousarray(series)).to(dev)
        self._rel = torch.from_numpy(self.rel).to(dev)
        self._labels = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in self.labels.items()}
        self._arange = torch.arange(max(len(v) for v in self.labels.values()), device=dev)
        self.stats64 = None  # (2, F) fp64 on the device when computed here
        if stats is None:
            w = window_weights(self.L, self.labels["train"], self.rel)
            if self.missing_value is None:
                self.stats64 = self._ops.window_stats(self.series, torch.from_numpy(w).to(dev),
                                                      float(self.N) * float(w.astype(np.int64).sum()))
            else:  # the observed values only, never the filled ones
                self.stats64, wvalid = self._ops.window_stats_masked(self.series, torch.from_numpy(w).to(dev),
                                                                     self.missing_value)
                self.valid_weight = wvalid.cpu().numpy()
                empty = np.flatnonzero(self.valid_weight == 0)
                if empty.size:
                    raise ValueError(f"WindowedSeries: feature {', '.join(map(str, empty))} has no observed value "
                                     "in the training windows: no statistics to normalise it with")
            self._mean, self._std = (self.stats64[i].to(self.series.dtype).contiguous() for i in (0, 1))
        else:
            self._mean, self._std = (torch.from_numpy(np.ascontiguousarray(s.astype(series.dtype))).to(dev)
                                     for s in (mean, std))
        self._xsrc = self.series  # where the gather reads the inputs
        if self.fill == "ffill":
            self.filled, counts = self._ops.window_fill_forward(self.series, self.missing_value, self.max_gap or 0)
            self._xsrc = self.filled
            self.missing_count, self.filled_count = counts.cpu().numpy()
        elif self.fill == "mean":  # nothing to launch: counted on the host copy
            miss = np.isnan(series) if self.missing_value != self.missing_value \
                else series == series.dtype.type(self.missing_value)
            self.missing_count = miss.sum(axis=(0, 1), dtype=np.int64)
            self.filled_count = np.zeros(self.F, dtype=np.int64)
        self._splits = {k: WindowSplit(self, k) for k in SPLITS}

    @classmethod
    def from_file(cls, graph_signal_matrix_filename, num_of_weeks, num_of_days, num_of_hours, num_for_predict,
                  points_per_hour=1, device=None, stats=None, missing_value=None, fill='mean', max_gap=None):
        """From the raw ``.npz`` (key ``data``) read_and_generate_dataset reads."""
        return cls(np.load(graph_signal_matrix_filename)["data"], num_of_weeks, num_of_days, num_of_hours,
                   num_for_predict, points_per_hour, device=device, stats=stats, missing_value=missing_value,
                   fill=fill, max_gap=max_gap)

    @property
    def mean(self):
        return self._mean.cpu().numpy().reshape(1, 1, self.F, 1)

    @property
    def std(self):
        return self._std.cpu().numpy().reshape(1, 1, self.F, 1)

    def tile_nodes(self):
        """Nodes one workgroup of the gather handles at this F and Tin."""
        return int(self._ops.window_tile_nodes(self.F, self.Tin))

    def _iota(self, n):
        return self._arange[:n]

    def split(self, name):
        if name not in self._splits:
            raise KeyError(f"WindowedSeries: no split {name!r} (one of {', '.join(SPLITS)})")
        return self._splits[name]

    def batch(self, name, idx):
        """(x (B, N, F, Tin), y (B, N, P)) fp32 of the samples ``idx`` (positions in the split:
        an int64 tensor, taken as it is when it lives on the device; a slice; or a sequence) from
        one launch.  A position outside the split gives NaN, never a read outside the series.
        With a missing value: the masked gather (a missing input is 0.0, ``y`` keeps the marker)."""
        labels = self._labels[name] if name in self._labels else self.split(name)
        if isinstance(idx, slice):
            idx = self._iota(labels.numel())[idx]
        elif not torch.is_tensor(idx):
            idx = torch.as_tensor(idx, dtype=torch.int64)
        if idx.dtype != torch.int64 or idx.dim() != 1:
            raise ValueError("WindowedSeries.batch: idx must be a 1-D int64 tensor")
        idx = idx.to(self.device).contiguous()
        if self.missing_value is None:
            return self._ops.window_gather(self.series, self._rel, labels, idx, self._mean, self._std, self.P)
        return self._ops.window_gather_masked(self._xsrc, self.series, self._rel, labels, idx, self._mean, self._std,
                                              self.P, self.missing_value)
