"""GPU: the drought event counts (csrc/loss.hip events_kernel through loss.EventScores) against the
numpy reference tests/events_ref.py, bit for bit: the tables are integers, so every comparison is
np.array_equal and there is no tolerance.  The scores are compared with the reference's, which
counts each threshold's 2 x 2 table directly from the event masks, at rtol = 1e-12 (a handful of
fp64 operations on identical integers).

Predictions and targets are drawn independently and uniformly from events_ref.grid: each threshold's
fp32 value, its two nextafter neighbours and one value beyond either end, so that every cell of the
confusion matrix and both sides of every <= / >= are hit (asserted on the reference).  Every run has
2 % NaN predictions, a +inf and a -inf prediction, and hands the kernel a batch slice ``big[1:]`` of
a larger tensor (a start that is not 16-byte aligned for odd N P).
"""
import warnings

import numpy as np
import pytest
import torch

import events_ref as ER

pytestmark = pytest.mark.gpu

NAN = float("nan")
SEED = 0
MODES = {"none": None, "neq": -9999.0, "nan": NAN}
DIRECTIONS = ("below", "above")
KS = (1, 3, 7)

# (B, N, P), the sizes of the updates along B
SHAPES = {
    "1x1x1": ((1, 1, 1), [1]),
    "5x23x12-two-strips-one-partial-two-updates": ((5, 23, 12), [2, 3]),
    "3x40x7-idle-threads": ((3, 40, 7), [3]),
    "3x257x1-256-nodes-per-strip": ((3, 257, 1), [3]),
    "2x3x256-one-node-per-strip": ((2, 3, 256), [2]),
    "2x9x129": ((2, 9, 129), [2]),
    "6x2200x12-105-workgroups": ((6, 2200, 12), [6]),
}
# the shapes on which every cell of the overall confusion matrix must be hit, for every K that runs
COVERED = ("5x23x12-two-strips-one-partial-two-updates", "3x40x7-idle-threads", "2x3x256-one-node-per-strip",
           "3x257x1-256-nodes-per-strip")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _admitted(P, K):
    """The LDS rule: (P + 256 / P) rows of 2 + (K + 1)^2 uint32 counters within 64 KiB."""
    return (P + 256 // P) * (2 + (K + 1) ** 2) * 4 <= 64 * 1024


def _thresholds(K, direction, N=None):
    """-1 - 0.5 k, mildest first (mirrored for ``above``).  With N: a (K, N) table, each node's set
    shifted by its own offset, with a tied column (where K > 1) and an excluded node (where N > 1)."""
    base = (-1.0 - 0.5 * np.arange(K)).astype(np.float32) * np.float32(1.0 if direction == "below" else -1.0)
    if N is None:
        return base
    thr = (base[:, None] + np.linspace(-0.2, 0.2, N, dtype=np.float32)[None, :]).astype(np.float32)
    if K > 1:
        thr[1, N // 2] = thr[0, N // 2]
    if N > 1:
        thr[:, N - 1] = NAN
    return thr


def _inputs(shape, thr, marker, seed=SEED):
    rng = np.random.default_rng(seed)
    target, pred = ER.draw(rng, thr, shape), ER.draw(rng, thr, shape)
    pred[rng.random(shape) < 0.02] = NAN
    pred.reshape(-1)[0] = np.inf
    if pred.size > 1:
        pred.reshape(-1)[-1] = -np.inf
    if marker is not None:
        target[rng.random(shape) < 0.15] = marker
    return pred, target


def _device_pair(pred, target):
    """(pred, target) on the device, pred as the slice [1:] of a tensor one sample larger."""
    big = torch.full((pred.shape[0] + 1,) + pred.shape[1:], 7.0, dtype=torch.float32, device="cuda")
    big[1:] = torch.from_numpy(pred).cuda()
    return big[1:], torch.from_numpy(target).cuda()


def _run(pred, target, thr, direction, marker, nodes, updates):
    from dstagnn_drought_amd import EventScores
    B, N, P = pred.shape
    ev = EventScores(P, thr, direction=direction, missing_value=marker, num_nodes=N if nodes else None, device="cuda")
    pd, tg = _device_pair(pred, target)
    at = 0
    for u in updates:
        ev.update(pd[at:at + u], tg[at:at + u])
        at += u
    assert at == B
    return ev


def _check_tables(ev, want, what):
    tab = ev.table.cpu().numpy()
    assert tab.dtype == np.float64 and tab.shape == want["horizon"].shape, what
    assert np.array_equal(tab, want["horizon"]), what
    assert np.array_equal(tab[:, 0], tab[:, 1] + tab[:, 2:].sum(1)), what
    if ev.node_table is not None:
        node = ev.node_table.cpu().numpy()
        assert node.shape == want["node"].shape and np.array_equal(node, want["node"]), what
        assert np.array_equal(node[:, 0], node[:, 1] + node[:, 2:].sum(1)), what


def _check_scores(got, want, what):
    assert sorted(got) == sorted(want), what
    for k, v in want.items():
        assert got[k].shape == v.shape and got[k].dtype == np.float64, (what, k)
        assert np.allclose(got[k], v, rtol=1e-12, atol=0, equal_nan=True), (what, k)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("case", list(SHAPES))
def test_tables_and_scores_vs_reference(case, K):
    """Every direction, mask and threshold form at one (shape, K); the (K,) form with the node table
    off and on, the (K, N) form (which fixes the node table) with a tied column and an excluded node."""
    _need_gpu()
    from dstagnn_drought_amd import EventScores
    shape, updates = SHAPES[case]
    B, N, P = shape
    if not _admitted(P, K):
        with pytest.raises(ValueError, match="LDS"):
            EventScores(P, _thresholds(K, "below"), device="cuda")
        return
    for direction in DIRECTIONS:
        for mode, marker in MODES.items():
            for per_node in (False, True):
                what = (case, K, direction, mode, per_node)
                thr = _thresholds(K, direction, N if per_node else None)
                pred, target = _inputs(shape, thr, marker)
                want = ER.counts(pred, target, thr, direction, marker)
                quads = ER.two_by_two(pred, target, thr, direction, marker)
                if case in COVERED and not per_node:  # no cell and no <= against < boundary goes untested
                    assert want["horizon"][:, 2:].sum(0).min() >= 1, what
                assert want["horizon"][:, 0].sum() > 0 or shape == (1, 1, 1), what
                for nodes in ((True,) if per_node else (False, True)):
                    ev = _run(pred, target, thr, direction, marker, nodes, updates)
                    assert (ev.node_table is not None) == nodes and ev.num_nodes == (N if nodes else None)
                    _check_tables(ev, want, what)
                    _check_scores(ev.scores(), ER.scores(want["horizon"], quads["horizon"]), what)
                    if nodes:
                        _check_scores(ev.node_scores(), ER.scores(want["node"], quads["node"], overall=False), what)
                if per_node:
                    ex = ER.excluded_nodes(thr, N)
                    assert np.array_equal(ev.excluded, ex) and ex.sum() == (1 if N > 1 else 0)
                    assert not ev.node_table.cpu().numpy()[ex].any()  # none of its entries reaches any count
                    assert np.array_equal(ev.thresholds, thr, equal_nan=True)
                else:
                    assert ev.excluded is None and np.array_equal(ev.thresholds, thr)


def test_seven_levels_are_refused_where_the_histograms_do_not_fit():
    _need_gpu()
    from dstagnn_drought_amd import EventScores
    from dstagnn_drought_amd import _lib
    thr = _thresholds(7, "below")
    for P in (256, 248, 1):
        with pytest.raises(ValueError, match="LDS"):
            EventScores(P, thr, device="cuda")
    EventScores(247, thr, device="cuda")
    z = torch.zeros(1, 2, 256, device="cuda")
    with pytest.raises(RuntimeError, match="LDS"):  # the library's own refusal behind the op
        _lib.load().events_update(z, z, 0, 0.0, torch.from_numpy(thr).cuda(), False,
                                  torch.zeros(256, 66, dtype=torch.float64, device="cuda"), None)


@pytest.mark.parametrize("mode", list(MODES))
def test_two_updates_equal_one_determinism_and_merge(mode):
    _need_gpu()
    marker = MODES[mode]
    shape, K = (7, 37, 5), 3
    thr = _thresholds(K, "below", shape[1])
    pred, target = _inputs(shape, thr, marker, seed=11)
    want = ER.counts(pred, target, thr, "below", marker)
    one = _run(pred, target, thr, "below", marker, True, [7])
    again = _run(pred, target, thr, "below", marker, True, [7])
    parts = _run(pred, target, thr, "below", marker, True, [3, 1, 3])
    for ev in (one, again, parts):
        _check_tables(ev, want, mode)
    assert torch.equal(one.table, again.table) and torch.equal(one.node_table, again.node_table)
    # merge: the two halves scored by two objects
    a = _run(pred[:4], target[:4], thr, "below", marker, True, [4])
    b = _run(pred[4:], target[4:], thr, "below", marker, True, [3])
    assert a.merge(b) is a
    _check_tables(a, want, mode)
    other = _run(pred[:1], target[:1], _thresholds(K, "below"), "below", marker, True, [1])
    with pytest.raises(ValueError, match="configuration"):
        a.merge(other)  # another definition of the classes
    a.reset()
    assert not a.table.any() and not a.node_table.any()


def test_an_all_invalid_batch_and_an_empty_one_leave_the_tables_zero():
    _need_gpu()
    from dstagnn_drought_amd import EventScores
    shape = (3, 23, 12)
    thr = _thresholds(3, "below")
    pred, _ = _inputs(shape, thr, None)
    for marker in (NAN, -9999.0):
        ev = _run(pred, np.full(shape, marker, dtype=np.float32), thr, "below", marker, True, [3])
        assert not ev.table.any() and not ev.node_table.any()
    ev = EventScores(12, thr, num_nodes=23, device="cuda")
    ev.update(torch.zeros(0, 23, 12, device="cuda"), torch.zeros(0, 23, 12, device="cuda"))
    assert not ev.table.any()
    # a NaN target that no mask marks is an ordinary value of class 0
    ev = _run(pred, np.full(shape, NAN, dtype=np.float32), thr, "below", None, False, [3])
    want = ER.counts(pred, np.full(shape, NAN, dtype=np.float32), thr, "below", None)
    _check_tables(ev, want, "NaN targets, no mask")
    assert ev.table[:, 2 + 4:].sum() == 0 and ev.table[:, 0].sum() == 3 * 23 * 12


def test_a_quantile_forecast_and_a_wrong_shape_are_refused():
    _need_gpu()
    from dstagnn_drought_amd import EventScores
    ev = EventScores(12, [-1.0, -1.5, -2.0], num_nodes=5, device="cuda")
    t = torch.zeros(2, 5, 12, device="cuda")
    with pytest.raises(ValueError, match="point_index"):
        ev.update(torch.zeros(2, 5, 12, 3, device="cuda"), t)
    with pytest.raises(ValueError, match="num_nodes"):
        ev.update(torch.zeros(2, 6, 12, device="cuda"), torch.zeros(2, 6, 12, device="cuda"))
    with pytest.raises(RuntimeError, match="HIP"):
        ev.update(t.cpu(), t.cpu())
    assert not ev.table.any()
    ev.update(torch.zeros(2, 5, 12, 3, device="cuda")[..., 1], t)  # its point_index column is taken
    assert ev.table[:, 0].sum() == 2 * 5 * 12 and ev.table[:, 2].sum() == 2 * 5 * 12


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mode", list(MODES))
def test_node_percentile_thresholds_vs_numpy(mode, dtype):
    _need_gpu()
    import skill_ref as SR
    from dstagnn_drought_amd import EventScores, WindowedSeries, node_percentile_thresholds
    marker = MODES[mode]
    L, N, F, P = 160, 9, 2, 5
    series = SR.gapped_series(L, N, F, dtype, marker, seed=21, period=12, t_end=(L * 3) // 5, lead=(L * 4) // 5)
    ws = WindowedSeries(series, 0, 0, 1, P, points_per_hour=P, device="cuda", missing_value=marker)
    t_end = int(ws.labels["train"][-1]) + P
    assert t_end < (L * 4) // 5 < L - P  # (node 0's leading gap covers the training steps)
    obs = series[:t_end, :, -1].astype(np.float64)
    obs[SR.missing(series[:t_end, :, -1], marker)] = np.nan
    for pct, direction in (((20, 10, 5, 2), "below"), ((80, 90, 95), "above")):
        got = node_percentile_thresholds(ws, pct, direction=direction, missing_value=marker)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == (len(pct), N) and got.is_contiguous()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # (the all-NaN column of node 0)
            want = np.nanpercentile(obs, pct, axis=0)
        g = got.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(want))
        assert np.allclose(g, want, rtol=1e-6, atol=0, equal_nan=True)
        if marker is not None:
            assert np.isnan(g[:, 0]).all() and not np.isnan(g[:, 1:]).any()  # node 0: no observed training value
        # a value at or beyond t_end does not change it
        moved = series.copy()
        moved[t_end:] = np.where(SR.missing(moved[t_end:], marker), moved[t_end:], moved[t_end:] + 1000.0)
        ws2 = WindowedSeries(moved, 0, 0, 1, P, points_per_hour=P, device="cuda", missing_value=marker)
        assert torch.equal(node_percentile_thresholds(ws2, pct, direction=direction, missing_value=marker).isnan(),
                           got.isnan())
        assert np.array_equal(node_percentile_thresholds(ws2, pct, direction=direction, missing_value=marker)
                              .cpu().numpy(), g, equal_nan=True)
        # ... and the table is one EventScores takes: node 0 excluded under a marker
        ev = EventScores(P, got, direction=direction, missing_value=marker)
        assert ev.num_nodes == N and ev.excluded.tolist() == [marker is not None] + [False] * (N - 1)
        _, y = ws.split("test").batch(slice(None))
        y = y.contiguous()
        pred = torch.roll(torch.nan_to_num(y, nan=0.0), 1, 0)
        ev.update(pred, y)
        want_t = ER.counts(pred.cpu().numpy(), y.cpu().numpy(), g, direction, marker)
        _check_tables(ev, want_t, (mode, direction))


def _tiny_model(N, P, T):
    import dstagnn_drought_amd as D
    adj = np.zeros((N, N))
    for i in range(N):
        adj[i, (i + 1) % N] = adj[(i + 1) % N, i] = 1.0
        adj[i, (i + 5) % N] = adj[(i + 5) % N, i] = 1.0
    torch.manual_seed(1)
    return D.make_model("cpu", 1, 2, 1, 3, 32, 32, 1, adj, adj, adj, P, T, N, 64, 32, 32, 3).cuda().eval()


def test_score_batches_feeds_the_events_in_the_same_pass():
    """A tiny model (N = 16), two batches: the events table equals one update on the concatenated
    outputs, and events=None returns exactly what the call returned before."""
    _need_gpu()
    from dstagnn_drought_amd import EventScores
    from dstagnn_drought_amd import train as TR
    N, P, T, S, bs = 16, 12, 12, 6, 4
    net = _tiny_model(N, P, T)
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(S, N, 1, T, device="cuda", generator=gen)
    with torch.no_grad():
        outs = torch.cat([net(x[:bs]), net(x[bs:])], 0)
    o = outs.cpu().numpy().astype(np.float64)
    thr = np.quantile(o, [0.4, 0.2, 0.1]).astype(np.float32)  # mildest first for ``below``
    assert thr[0] > thr[1] > thr[2]
    y = torch.from_numpy(ER.draw(np.random.default_rng(6), thr, (S, N, P))).cuda()
    y[0, 3, 2] = NAN

    def scorer():
        return EventScores(P, thr, missing_value=NAN, num_nodes=N, device="cuda")
    ev = scorer()
    with_ev = TR.score_batches(net, x, y, bs, NAN, True, events=ev)
    without = TR.score_batches(net, x, y, bs, NAN, True)
    none_ev = TR.score_batches(net, x, y, bs, NAN, True, events=None)
    for other in (with_ev, none_ev):  # the returned ForecastMetrics: the same bits
        assert type(other) is type(without)
        assert torch.equal(other.table, without.table) and torch.equal(other.node_table, without.node_table)
        assert other.compute() == without.compute() or np.array_equal(other.compute(), without.compute(), equal_nan=True)
    once = scorer()
    once.update(outs, y)
    assert torch.equal(ev.table, once.table) and torch.equal(ev.node_table, once.node_table)
    want = ER.counts(outs.cpu().numpy(), y.cpu().numpy(), thr, "below", NAN)
    _check_tables(ev, want, "score_batches")
    assert want["horizon"][:, 0].sum() == S * N * P - 1 and (want["horizon"][:, 2:].sum(0) > 0).sum() >= 8
    _check_scores(ev.scores(), ER.scores(want["horizon"], ER.two_by_two(outs.cpu().numpy(), y.cpu().numpy(), thr,
                                                                       "below", NAN)["horizon"]), "score_batches")


def test_score_test_split_reports_and_writes_the_event_scores(tmp_path):
    """The driver's scoring step with events=: the new result keys, log lines and files, and every
    pre-existing key, line and file as without it."""
    _need_gpu()
    import json
    import os
    from dstagnn_drought_amd import EventScores
    from dstagnn_drought_amd import train as TR
    N, P, T, S, bs, K = 16, 12, 12, 6, 4, 3
    net = _tiny_model(N, P, T)
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(S, N, 1, T, device="cuda", generator=gen)
    thr = _thresholds(K, "below", N)  # per node: a tied column, node N - 1 excluded
    y = torch.from_numpy(ER.draw(np.random.default_rng(6), thr, (S, N, P))).cuda()
    y[1, 2, 3] = NAN
    ev = EventScores(P, thr, missing_value=NAN, device="cuda")
    with_dir, base_dir = tmp_path / "with", tmp_path / "base"
    with_dir.mkdir(), base_dir.mkdir()
    lines, base_lines = [], []
    out = TR._score_test_split(net, x, y, bs, NAN, True, str(with_dir), lines.append, None, None, ev)
    base = TR._score_test_split(net, x, y, bs, NAN, True, str(base_dir), base_lines.append)
    assert set(out) == set(base) | {"test_event_scores", "test_node_event_scores"}
    assert out["test_metrics"] == base["test_metrics"] or np.array_equal(out["test_metrics"], base["test_metrics"],
                                                                        equal_nan=True)
    for key in ("test_scores", "test_node_scores"):
        for k, v in base[key].items():
            assert np.array_equal(out[key][k], v, equal_nan=True), (key, k)
    assert [ln for ln in lines if not ln.startswith("Test events")] == base_lines
    ev_lines = [ln for ln in lines if ln.startswith("Test events")]
    assert len(ev_lines) == P + 2 and ev_lines[P].startswith("Test events overall: ")
    assert all(w in ev_lines[0] for w in ("pod[#0]", "far[#1]", "csi[#2]", "hss[#2]", "hss_multi"))
    assert "1 of 16 nodes excluded" in ev_lines[-1]
    assert sorted(os.listdir(with_dir)) == sorted(os.listdir(base_dir) + ["test_event_scores.json",
                                                                         "test_node_event_scores.npz"])
    with open(with_dir / "test_event_scores.json") as f:
        rec = json.load(f)
    assert rec["direction"] == "below" and rec["thresholds"] == {"shape": [K, N]}
    got = out["test_event_scores"]
    assert np.array_equal(np.array(rec["pod"]), got["pod"], equal_nan=True) and got["pod"].shape == (P + 1, K)
    with np.load(with_dir / "test_node_event_scores.npz") as f:
        assert np.array_equal(f["thresholds"], thr, equal_nan=True)
        assert f["excluded"].tolist() == [False] * (N - 1) + [True]
        assert np.array_equal(f["csi"], out["test_node_event_scores"]["csi"], equal_nan=True) and f["csi"].shape == (N, K)
    with torch.no_grad():
        outs = torch.cat([net(x[:bs]), net(x[bs:])], 0)
    want = ER.counts(outs.cpu().numpy(), y.cpu().numpy(), thr, "below", NAN)
    _check_tables(ev, want, "_score_test_split")


@pytest.mark.parametrize("how", ["percentiles", "thresholds"])
def test_driver_scores_events_beside_the_existing_scores(golden_dir, tmp_path, how):
    """run() with the event options on the gapped streamed configuration of the masked-metrics
    tests: the result keys, the files and the scores of a fresh object fed the returned net."""
    _need_gpu()
    import configparser
    import os
    import test_gpu_metrics_masked as tmm
    from dstagnn_drought_amd import EventScores, node_percentile_thresholds
    from dstagnn_drought_amd import train as TR
    conf, td = tmm._g12_gapped(golden_dir, tmp_path)
    torch.cuda.set_device(0)
    kw = dict(event_percentiles="60,30,10") if how == "percentiles" else dict(event_thresholds=(60.0, 40.0, 20.0))
    lines = []
    res = TR.run(conf, root=os.path.join(td, "exp_events"), log=lines.append, stream_windows=True, missing_value=NAN,
                 input_fill="mean", epochs=1, max_batches=2, dropout=0.0, node_scores=True, loss="masked_mae", **kw)
    cp = configparser.ConfigParser()
    cp.read(conf)
    dc, tc = cp["Data"], cp["Training"]
    P, N, bs = int(dc["num_for_predict"]), int(dc["num_of_vertices"]), int(tc["batch_size"])
    assert {"test_metrics", "test_scores", "test_node_scores", "test_event_scores", "test_node_event_scores"} <= set(res)
    files = os.listdir(res["params_path"])
    assert "test_event_scores.json" in files and "test_node_event_scores.npz" in files
    assert len([ln for ln in lines if ln.startswith("Test events ")]) == P + 1
    ws = TR._windowed_series(dc, tc, torch.device("cuda", 0), NAN, "mean", None)
    thr = (node_percentile_thresholds(ws, (60, 30, 10), missing_value=NAN) if how == "percentiles"
           else (60.0, 40.0, 20.0))
    ev = EventScores(P, thr, missing_value=NAN, num_nodes=N, device="cuda")
    sp = ws.split("test")
    with torch.no_grad():
        for b in range(0, sp.x.shape[0], bs):
            xb, yb = TR._cut(sp.x, sp.y, b, b + bs)
            ev.update(res["net"](xb), yb)
    assert ev.table[:, 0].sum() > 0
    for k, v in ev.scores().items():
        assert np.array_equal(res["test_event_scores"][k], v, equal_nan=True), k
    for k, v in ev.node_scores().items():
        assert np.array_equal(res["test_node_event_scores"][k], v, equal_nan=True), k
