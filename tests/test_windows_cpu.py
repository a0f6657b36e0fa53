"""CPU: the host side of dstagnn_drought_amd.windows (no device): the window offsets, label
tables and split of read_and_generate_dataset, held against the files the reference's
prepareData.py itself wrote (tests/golden/g10_prepare_*.npz); the weight vector of the on-device
statistics against a bincount over the explicit windows; the errors; the operator registration.
"""
import os

import numpy as np
import pytest
import torch

from dstagnn_drought_amd import windows as W

GOLDENS = ("g10_prepare_a", "g10_prepare_b", "g10_prepare_c")


def load_golden(golden_dir, name):
    """(arrays, window arguments) of a prepareData.py golden; meta = [T, N, F, hours, days,
    weeks, points_per_hour, num_for_predict] (tests/golden/gen_golden_data.py)."""
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    nh, nd, nw, pph, nfp = (int(v) for v in g["meta"][3:8])
    return g, dict(num_of_weeks=nw, num_of_days=nd, num_of_hours=nh, num_for_predict=nfp, points_per_hour=pph)


def explicit_steps(labels, rel):
    """(S, Tin) time steps of every window: the table the streaming path never builds."""
    return np.asarray(labels, np.int64)[:, None] + np.asarray(rel, np.int64)[None, :]


@pytest.mark.parametrize("name", GOLDENS)
def test_tables_match_the_reference_files(golden_dir, name):
    g, kw = load_golden(golden_dir, name)
    L = g["data"].shape[0]
    labels, rel = W.window_tables(L, **kw)
    assert rel.dtype == np.int32 and rel.size == g["out_train_x"].shape[-1]
    for split in W.SPLITS:
        assert labels[split].dtype == np.int64
        np.testing.assert_array_equal(labels[split][:, None], g[f"out_{split}_timestamp"])
    # the offsets reproduce the reference's un-normalised windows exactly (a pure gather)
    raw = g["data"][explicit_steps(labels["val"], rel)].transpose(0, 2, 3, 1)  # (S, N, F, Tin)
    mean, std = g["out_mean"], g["out_std"]
    np.testing.assert_array_equal((raw - mean) / std, g["out_val_x"])
    tgt = g["data"][labels["val"][:, None] + np.arange(kw["num_for_predict"])[None, :]][..., -1].transpose(0, 2, 1)
    np.testing.assert_array_equal(tgt, g["out_val_target"])


def test_offsets_order_and_overlap(golden_dir):
    # week, day, hour kinds in that order, each oldest first
    rel = W.window_offsets(1, 2, 1, 3, points_per_hour=2)
    assert rel.tolist() == [-336, -335, -334, -96, -95, -94, -48, -47, -46, -2, -1, 0]
    # golden c: points_per_hour * units < num_for_predict, so offsets reach into the target
    _, kw = load_golden(golden_dir, "g10_prepare_c")
    assert W.window_offsets(**kw).max() >= 0
    _, kwb = load_golden(golden_dir, "g10_prepare_b")
    assert W.window_offsets(**kwb).min() == -288 and W.window_offsets(**kwb).size == 36
    assert W.window_offsets(0, 0, 0, 12).size == 0


@pytest.mark.parametrize("name", GOLDENS)
def test_weights_are_the_bincount_of_the_explicit_windows(golden_dir, name):
    g, kw = load_golden(golden_dir, name)
    L = g["data"].shape[0]
    labels, rel = W.window_tables(L, **kw)
    w = W.window_weights(L, labels["train"], rel)
    assert w.dtype == np.int32 and w.shape == (L,)
    steps = explicit_steps(labels["train"], rel)
    np.testing.assert_array_equal(w, np.bincount(steps.reshape(-1), minlength=L))
    assert int(w.sum()) == steps.size
    # the weighted moments ARE the statistics over the windows (exact rational identity; fp64 here)
    x = g["data"].astype(np.float64)
    ref = x[steps]  # (S, Tin, N, F)
    wm = np.tensordot(w.astype(np.float64), x, axes=(0, 0)).sum(0) / (w.sum() * x.shape[1])
    np.testing.assert_allclose(wm, ref.mean(axis=(0, 1, 2)), rtol=1e-13)


def test_empty_split_raises_like_read_and_generate_dataset(tmp_path):
    from dstagnn_drought_amd.data import read_and_generate_dataset
    series = np.arange(25 * 2 * 1, dtype=np.float64).reshape(25, 2, 1)
    path = os.path.join(str(tmp_path), "short.npz")
    np.savez(path, data=series)
    with pytest.raises(ValueError) as ref:  # 2 label positions: int(2 * 0.6) == int(2 * 0.8), no val sample
        read_and_generate_dataset(path, 0, 0, 1, 12, points_per_hour=12)
    with pytest.raises(ValueError) as got:
        W.window_tables(25, 0, 0, 1, 12, points_per_hour=12)
    assert str(got.value) == str(ref.value)
    # the constructor raises it before it looks for a device
    with pytest.raises(ValueError, match="train / val / test"):
        W.WindowedSeries(series, 0, 0, 1, 12, points_per_hour=12)
    with pytest.raises(ValueError, match="train / val / test"):
        W.WindowedSeries(series, 0, 0, 0, 12)  # no dependency kind enabled
    with pytest.raises(ValueError, match=r"\(L, N, F\)"):
        W.WindowedSeries(series[:, :, 0], 0, 0, 1, 12)


def test_offsets_leaving_the_series_are_rejected_when_the_table_is_built():
    labels, rel = W.window_tables(100, 0, 0, 1, 12, points_per_hour=12)
    every = np.concatenate([labels[k] for k in W.SPLITS])
    W.check_offsets(100, every, rel, 12)  # what the constructor's own tables pass
    with pytest.raises(ValueError, match="outside the series"):
        W.check_offsets(100, every, rel - 1, 12)        # one step before the series' start
    with pytest.raises(ValueError, match="outside the series"):
        W.check_offsets(100, every + 1, rel, 12)        # the last target step past the end
    with pytest.raises(ValueError, match="outside the series"):
        W.check_offsets(100, every, rel + 24, 12)       # a window past the end
    with pytest.raises(ValueError, match="outside the series"):
        W.check_offsets(99, every, rel, 12)             # a shorter series under the same tables
    W.check_offsets(100, every[:-1], rel + 1, 12)       # inside again without the last label


def test_stats_argument_is_checked_before_the_device():
    series = np.zeros((100, 3, 2), dtype=np.float32)
    with pytest.raises(ValueError, match="F = 2"):
        W.WindowedSeries(series, 0, 0, 1, 12, points_per_hour=12, stats=(np.zeros(3), np.ones(3)))


def test_ops_registered_and_refuse_cpu_tensors():
    from dstagnn_drought_amd import _lib
    ops = _lib.load()
    for n in ("window_gather", "window_stats", "window_tile_nodes"):
        assert hasattr(ops, n), f"torch.ops.dstagnn.{n} missing"
    # the tile: as many nodes as fit a 32 KiB padded image, at most 64
    assert ops.window_tile_nodes(1, 12) == 64 and ops.window_tile_nodes(4, 144) == 13
    assert ops.window_tile_nodes(4, 7) == 64 and ops.window_tile_nodes(64, 144) == 1
    series = torch.zeros(40, 3, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError):
        ops.window_gather(series, torch.zeros(12, dtype=torch.int32), torch.arange(12, 20), torch.arange(4),
                          torch.zeros(2, dtype=torch.float64), torch.ones(2, dtype=torch.float64), 12)
    with pytest.raises(RuntimeError):
        ops.window_stats(series, torch.ones(40, dtype=torch.int32), 120.0)
    import dstagnn_drought_amd as D
    assert D.WindowedSeries is W.WindowedSeries
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP"):
            W.WindowedSeries(np.zeros((100, 3, 2)), 0, 0, 1, 12, points_per_hour=12)
