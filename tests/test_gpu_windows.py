"""GPU: training windows gathered from the raw series on the device (csrc/windows.hip,
dstagnn_drought_amd/windows.py) against the files the reference's prepareData.py wrote
(tests/golden/g10_prepare_*.npz), against a numpy restatement in the same dtype arithmetic, and
through the training loop.

Every value comparison of the gather is BIT equality (assert_array_equal): the kernel performs
numpy's operations, `(x - mean) / std` in the series' dtype with IEEE division, then one rounding
to fp32, and a gather has no summation order.

The statistics' bounds are derived, never fitted.  With u = 2^-53, n = L N
weighted terms per feature, A = sum w |x| / W (the windows' mean absolute value):
    |mean - ref|      <= 2 n u A
    |std - ref| / ref <= 2 (n + 8) u + (2 n u A / ref)^2
The device sum is a product and an add per term in some fixed order: at most (n + 1) u sum |w x|
after the division by W, for any order; numpy's pairwise fp64 reference is far inside another
n u, which the factor 2 covers.  The centred second moment adds four roundings per term (the
subtraction, the square, the weight, the add), the division and the square root (halved by the
root: (n + 8) u covers it), and the error of the centre enters squared:
sum w (x - m')^2 = sum w (x - m)^2 + W (m - m')^2.

Why `stats=` exists: numpy's own statistics of a float32 series are taken in float32.  For
g10_prepare_b the reference file's mean lies 3.1e-6 / 1.4e-6 (relative, per feature) and its std
4e-7 / 1.7e-7 from the fp64 values of the same windows, while the fp64 values rounded to float32
lie <= 4.5e-8 from them: a run that must reproduce a prepared file takes that file's statistics.
"""
import gc
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDENS = ("g10_prepare_a", "g10_prepare_b", "g10_prepare_c")
U = 2.0 ** -53


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.set_device(0)


def load_golden(golden_dir, name):
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    nh, nd, nw, pph, nfp = (int(v) for v in g["meta"][3:8])
    return g, dict(num_of_weeks=nw, num_of_days=nd, num_of_hours=nh, num_for_predict=nfp, points_per_hour=pph)


def gather_ref(series, labels, rel, idx, mean, std, P):
    """The gather in numpy: the same operations in the series' dtype, one rounding to fp32."""
    S = series.dtype
    lab = np.asarray(labels, np.int64)[np.asarray(idx, np.int64)]
    steps = lab[:, None] + np.asarray(rel, np.int64)[None, :]
    xs = series[steps]  # (B, Tin, N, F)
    x = ((xs - np.asarray(mean, S).reshape(-1)) / np.asarray(std, S).reshape(-1)).transpose(0, 2, 3, 1)
    y = series[lab[:, None] + np.arange(P)[None, :]][..., -1].transpose(0, 2, 1)
    return np.ascontiguousarray(x.astype(np.float32)), np.ascontiguousarray(y.astype(np.float32))


def bits_equal(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=what)


# ---------------------------------------------------------------------------------------------
# 1. the reference's own files, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_gather_reproduces_the_reference_files(golden_dir, name):
    _need_gpu()
    from dstagnn_drought_amd import WindowedSeries
    g, kw = load_golden(golden_dir, name)
    ws = WindowedSeries(g["data"], stats=(g["out_mean"], g["out_std"]), **kw)
    assert ws.series.dtype == {np.dtype("float32"): torch.float32, np.dtype("float64"): torch.float64}[g["data"].dtype]
    gen = torch.Generator().manual_seed(7)
    for split in ("train", "val", "test"):
        want_x = np.ascontiguousarray(g[f"out_{split}_x"].astype(np.float32))
        want_y = np.ascontiguousarray(g[f"out_{split}_target"].astype(np.float32))
        sp = ws.split(split)
        np.testing.assert_array_equal(sp.timestamp, g[f"out_{split}_timestamp"])
        np.testing.assert_array_equal(ws._labels[split].cpu().numpy()[:, None], g[f"out_{split}_timestamp"])
        S = want_x.shape[0]
        assert tuple(sp.x.shape) == want_x.shape and tuple(sp.y.shape) == want_y.shape
        # every sample as a single batch
        x, y = ws.batch(split, torch.arange(S, device=ws.device))
        bits_equal(x, want_x, f"{name}/{split}/x whole")
        bits_equal(y, want_y, f"{name}/{split}/y whole")
        # batches of 4 through a shuffled device index tensor, slices of it used as they are
        perm = torch.randperm(S, generator=gen)
        dperm = perm.to(ws.device)
        for i in range(0, S, 4):
            x, y = ws.batch(split, dperm[i:i + 4])
            sel = perm[i:i + 4].numpy()
            bits_equal(x, want_x[sel], f"{name}/{split}/x batch {i}")
            bits_equal(y, want_y[sel], f"{name}/{split}/y batch {i}")
        # the tensor-like surface the loop uses
        bits_equal(sp.x[1:3], want_x[1:3], "x slice")
        bits_equal(sp.y[1:3], want_y[1:3], "y slice")
        bits_equal(sp.x.index_select(0, dperm[:3]), want_x[perm[:3].numpy()], "x index_select")
        bits_equal(sp.y.index_select(0, dperm[:3]), want_y[perm[:3].numpy()], "y index_select")
        assert sp.x.device == ws.device and len(sp.x) == S


# ---------------------------------------------------------------------------------------------
# 2. tile and alignment edges
# ---------------------------------------------------------------------------------------------
def _synthetic(L, N, F, dtype, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((L, N, F)) * 3.0 + 10.0 * np.arange(1, F + 1)).astype(dtype)


def _edge_case(series, kw, B):
    from dstagnn_drought_amd import WindowedSeries
    F = series.shape[2]
    rng = np.random.default_rng(3)
    mean = (rng.standard_normal(F) + 10.0).astype(series.dtype)
    std = (rng.random(F) + 0.5).astype(series.dtype)
    ws = WindowedSeries(series, stats=(mean, std), **kw)
    S = len(ws.labels["train"])
    idx = rng.permutation(S)[:B]
    x, y = ws.batch("train", torch.from_numpy(idx).to(ws.device))
    want_x, want_y = gather_ref(series, ws.labels["train"], ws.rel, idx, mean, std, ws.P)
    bits_equal(x, want_x, "x")
    bits_equal(y, want_y, "y")
    return ws


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("F", [1, 4])
@pytest.mark.parametrize("dn", [-1, 0, 1])
def test_gather_tile_edges_odd_run(dtype, F, dn):
    """Tin = 7: N F Tin is odd for odd N F, so x[b] starts off a 16-byte boundary for odd b (scalar
    head and tail); N on both sides of a tile edge; B = 3 and B = 1."""
    _need_gpu()
    from dstagnn_drought_amd import _lib
    kw = dict(num_of_weeks=0, num_of_days=0, num_of_hours=1, num_for_predict=7, points_per_hour=7)
    tile = int(_lib.load().window_tile_nodes(F, 7))
    assert tile >= 2
    series = _synthetic(40, tile + dn, F, dtype, 11 + dn)
    ws = _edge_case(series, kw, 3)
    assert ws.Tin == 7 and ws.tile_nodes() == tile
    _edge_case(series, kw, 1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gather_gambia_rows(dtype):
    """The GAMBIA row geometry: F = 4, Tin = 144 (twelve hour-windows of 12), N = tile + 3, B = 2."""
    _need_gpu()
    from dstagnn_drought_amd import _lib
    kw = dict(num_of_weeks=0, num_of_days=0, num_of_hours=12, num_for_predict=12, points_per_hour=12)
    tile = int(_lib.load().window_tile_nodes(4, 144))
    ws = _edge_case(_synthetic(180, tile + 3, 4, dtype, 5), kw, 2)
    assert ws.Tin == 144 and ws.rel.min() == -144 and ws.rel.max() == -1


# ---------------------------------------------------------------------------------------------
# 3. statistics
# ---------------------------------------------------------------------------------------------
def _stats_case(series, kw):
    from dstagnn_drought_amd import WindowedSeries, _lib
    from dstagnn_drought_amd import windows as W
    ws = WindowedSeries(series, **kw)
    L, N, F = series.shape
    steps = ws.labels["train"][:, None] + ws.rel.astype(np.int64)[None, :]
    win = series.astype(np.float64)[steps]  # (S, Tin, N, F): the materialised training windows
    ref_mean, ref_std = win.mean(axis=(0, 1, 2)), win.std(axis=(0, 1, 2))
    A = np.abs(win).mean(axis=(0, 1, 2))
    n = L * N
    got = ws.stats64.cpu().numpy()
    dmean = 2 * n * U * A
    err_mean = np.abs(got[0] - ref_mean)
    err_std = np.abs(got[1] - ref_std) / ref_std
    bound_std = 2 * (n + 8) * U + (dmean / ref_std) ** 2
    print(f"window_stats n={n}: |dmean| {err_mean} (bound {dmean}); rel dstd {err_std} (bound {bound_std})")
    assert (err_mean <= dmean).all(), (err_mean, dmean)
    assert (err_std <= bound_std).all(), (err_std, bound_std)
    # the same bits on every call
    w = torch.from_numpy(W.window_weights(L, ws.labels["train"], ws.rel)).to(ws.device)
    wtotal = float(N) * float(steps.size)
    ops = _lib.load()
    again = [ops.window_stats(ws.series, w, wtotal).cpu().numpy() for _ in range(2)]
    for a in again:
        np.testing.assert_array_equal(a.view(np.uint64), got.view(np.uint64))
    # the batches are normalised with these statistics cast to the series' dtype
    np.testing.assert_array_equal(ws.mean.reshape(-1), got[0].astype(series.dtype))
    np.testing.assert_array_equal(ws.std.reshape(-1), got[1].astype(series.dtype))
    idx = np.arange(min(3, len(ws.labels["val"])))
    x, y = ws.batch("val", torch.from_numpy(idx).to(ws.device))
    want_x, want_y = gather_ref(series, ws.labels["val"], ws.rel, idx, ws.mean, ws.std, ws.P)
    bits_equal(x, want_x, "x under computed statistics")
    bits_equal(y, want_y, "y under computed statistics")


@pytest.mark.parametrize("name", GOLDENS)
def test_stats_of_the_goldens(golden_dir, name):
    _need_gpu()
    g, kw = load_golden(golden_dir, name)
    _stats_case(g["data"], kw)


def test_stats_synthetic_fp32():
    """Values of order 1 around per-feature offsets >= 0.5 (the mean does not cancel); more time
    steps than the statistics launch has workgroups, N F no multiple of the row stride."""
    _need_gpu()
    rng = np.random.default_rng(17)
    L, N, F = 700, 37, 3
    series = (rng.standard_normal((L, N, F)) + np.array([0.5, -1.25, 3.0])).astype(np.float32)
    _stats_case(series, dict(num_of_weeks=0, num_of_days=1, num_of_hours=2, num_for_predict=6, points_per_hour=2))


# ---------------------------------------------------------------------------------------------
# 4. the loop's iterator
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2)])
def test_stream_batches_equal_device_batches(golden_dir, rank, world):
    _need_gpu()
    from dstagnn_drought_amd import WindowedSeries
    from dstagnn_drought_amd.train import DeviceBatches, StreamBatches
    g, kw = load_golden(golden_dir, "g10_prepare_a")
    ws = WindowedSeries(g["data"], stats=(g["out_mean"], g["out_std"]), **kw)
    mx = torch.from_numpy(g["out_train_x"]).type(torch.FloatTensor).to(ws.device)
    my = torch.from_numpy(g["out_train_target"]).type(torch.FloatTensor).to(ws.device)
    sp = ws.split("train")
    loaders = (DeviceBatches(mx, my, 8, True, rank, world), StreamBatches(sp.x, sp.y, 8, True, rank, world))
    assert len(loaders[0]) == len(loaders[1])
    runs, states = [], []
    for loader in loaders:
        torch.manual_seed(123)
        runs.append([[(x.cpu(), y.cpu()) for x, y in loader] for _epoch in range(2)])
        states.append(torch.get_rng_state())
    assert torch.equal(states[0], states[1])  # the same draws from the global RNG
    for ea, eb in zip(*runs):
        assert len(ea) == len(eb) == len(loaders[0])
        for (xa, ya), (xb, yb) in zip(ea, eb):
            assert xa.shape == xb.shape and torch.equal(xa.view(torch.int32), xb.view(torch.int32))
            assert ya.shape == yb.shape and torch.equal(ya.view(torch.int32), yb.view(torch.int32))
    assert not torch.equal(runs[0][0][0][0], runs[0][1][0][0])  # the second epoch is another permutation


# ---------------------------------------------------------------------------------------------
# 5. the driver
# ---------------------------------------------------------------------------------------------
def test_driver_streams_windows(golden_dir, tmp_path):
    _need_gpu()
    from dstagnn_drought_amd import train as TR
    from dstagnn_drought_amd.data import dataset_filename, read_and_generate_dataset
    g = dict(np.load(os.path.join(golden_dir, "g12_train.npz"), allow_pickle=False))
    td = str(tmp_path)
    for k in ("adj.csv", "stag.csv", "strg.csv"):
        with open(os.path.join(td, k), "w") as f:
            f.write(str(g[k + "_text"]))
    np.savez(os.path.join(td, "SYN.npz"), data=g["series"])
    read_and_generate_dataset(os.path.join(td, "SYN.npz"), 0, 0, 1, 12, points_per_hour=12, save=True)
    conf = os.path.join(td, "train.conf")
    with open(conf, "w") as f:
        f.write(str(g["config_text"]).replace("@DIR@", td))
    with np.load(dataset_filename(os.path.join(td, "SYN.npz"), 1, 0, 0) + ".npz") as f:
        train_x_bytes = int(np.prod(f["train_x"].shape)) * 4  # as the fp32 device tensor

    def one(stream, **kw):
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        kw.setdefault("epochs", 2)
        res = TR.run(conf, dropout=0.0, root=os.path.join(td, "exp_stream" if stream else "exp_mat"),
                     log=lambda *_: None, stream_windows=stream, **kw)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        vals = [h["val_loss"] for h in res["history"]]
        del res
        return vals, peak

    # warm-up (one batch each way): the library's one-time device state is part of neither peak
    one(False, epochs=1, max_batches=1)
    one(True, epochs=1, max_batches=1)
    vals_m, peak_m = one(False)
    vals_s, peak_s = one(True)
    print(f"val losses materialised {vals_m} streamed {vals_s}; peak bytes {peak_m} vs {peak_s}, "
          f"train_x {train_x_bytes}")
    assert len(vals_s) == len(vals_m) == 2
    assert np.abs(np.array(vals_s) - np.array(vals_m)).max() <= 1e-4, (vals_s, vals_m)
    assert np.abs(np.array(vals_s) - g["val_losses"][:2]).max() <= 1e-4, (vals_s, g["val_losses"])
    # the materialised tensors were never built: at least train_x's size is missing from the peak
    assert peak_s <= peak_m - train_x_bytes, (peak_s, peak_m, train_x_bytes)
