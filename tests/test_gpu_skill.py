"""GPU: the skill over persistence and over the seasonal climatology (csrc/loss.hip skill_kernel,
csrc/windows.hip climatology_kernel; loss.BaselineSkill; the driver's baseline_skill) against the
numpy reference tests/skill_ref.py on the same fp32 inputs.

Series are seeded (skill_ref.gapped_series): a 12-step (or `period`-step) cycle plus N(0, 1), with,
under a mask, a leading gap at node 0 that outlasts the first test label (no persistence there), a
(phase, node) never observed in training, and 15 % of everything else missing.  Targets are cut from
the series as the gather cuts them; pred = target + N(0, 1).

Bounds (derived; none of them measured):
  counts (columns 0, 5)   exact.
  every other column      |got - want| <= 1e-6 * (the reference's sum of that column's magnitudes):
                          a term carries at most three fp32 roundings on either side (a difference,
                          then a square) and the kernel forms the same fp32 terms as the reference,
                          so what is left is the order of the fp64 adds: n 2^-53 of the magnitudes.
                          The bound of tests/test_gpu_metrics_masked.py for these tables.
  climatology             counts exact; values 1e-12 relative: both sides add the same doubles in
                          increasing t and divide once (in fact the same bits).
"""
import json
import os

import numpy as np
import pytest
import torch

import skill_ref as SR

pytestmark = pytest.mark.gpu

NAN = float("nan")
REL = 1e-6
MODES = {"none": None, "neq": -9999.0, "nan": NAN}

# (B, N, P), the sizes of the updates along B
SHAPES = {
    "1x1x1": ((1, 1, 1), [1]),
    "5x101x3-two-strips-two-updates": ((5, 101, 3), [2, 3]),
    "4x170x12-pems08-head": ((4, 170, 12), [4]),
    "3x7x19-idle-threads": ((3, 7, 19), [3]),
    "2x9x129-one-node-per-strip": ((2, 9, 129), [2]),
    "2x5x256": ((2, 5, 256), [2]),
    "6x2200x12-105-workgroups": ((6, 2200, 12), [6]),
}
PERIODS = ("1", "7", "P", "beyond-training", "L")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _geometry(P):
    """(L, t_end) of a case: training steps [0, t_end), test labels from t_end on."""
    return 3 * P + 40, 2 * P + 20


def _period(kind, P):
    L, t_end = _geometry(P)
    return {"1": 1, "7": 7, "P": P, "beyond-training": t_end + 3, "L": L}[kind]


def _inputs(shape, dtype, mode, period, seed, F=2, extra_pos=()):
    """(pred, target, pos, series, t_end): the series with its gaps, B label positions spread over
    the test range (the first one right at t_end, inside node 0's leading gap), targets as the gather
    cuts them (fp32, markers kept), pred = target + N(0, 1) (finite everywhere)."""
    B, N, P = shape
    L, t_end = _geometry(P)
    marker = MODES[mode]
    series = SR.gapped_series(L, N, F, dtype, marker, seed, period=12, t_end=t_end, lead=t_end + 2)
    if marker is not None and N > 1:  # phase 1 of THIS period, node 1: never observed in training
        series[np.arange(1 % period, t_end, period), 1, :] = marker
    pos = np.concatenate([np.linspace(t_end, L - P, B).astype(np.int64), np.asarray(extra_pos, dtype=np.int64)])
    rng = np.random.default_rng(seed + 1)
    target = np.full((len(pos), N, P), np.nan, dtype=np.float32)
    for b, l in enumerate(pos):
        if 0 <= l and l + P <= L:
            target[b] = series[l:l + P, :, -1].T.astype(np.float32)
    fin = np.where(np.isnan(target) | (target == np.float32(-9999.0)), np.float32(1.0), target)
    pred = (fin + rng.normal(0, 1, target.shape)).astype(np.float32)
    return pred, target, pos, series, t_end


def _device_tables(series, period, t_end, mode):
    """(series, persistence source, clim, cnt, masked, null) on the device."""
    from dstagnn_drought_amd import _lib
    ops = _lib.load()
    marker = MODES[mode]
    masked, null = marker is not None, (0.0 if marker is None else marker)
    s = torch.from_numpy(np.ascontiguousarray(series)).cuda()
    clim, cnt = ops.climatology(s, period, t_end, masked, null)
    src = ops.window_fill_forward(s, null, 0)[0] if masked else s
    return s, src, clim, cnt, masked, null


def _run(pred, target, pos, series, period, t_end, mode, nodes=True, updates=None):
    """The op fed in `updates` cuts along B -> (htable, ntable or None) as numpy arrays."""
    from dstagnn_drought_amd import _lib
    from dstagnn_drought_amd.loss import mask_of
    ops = _lib.load()
    _, src, clim, cnt, masked, null = _device_tables(series, period, t_end, mode)
    mask = mask_of(MODES[mode])
    B, N, P = target.shape
    ht = torch.zeros(P, 13, dtype=torch.float64, device="cuda")
    nt = torch.zeros(N, 13, dtype=torch.float64, device="cuda") if nodes else None
    p, t, l = torch.from_numpy(pred).cuda(), torch.from_numpy(target).cuda(), torch.from_numpy(pos).cuda()
    at = 0
    for k in updates or [B]:
        ops.skill_update(p[at:at + k].contiguous(), t[at:at + k].contiguous(), mask[0], mask[1], src, masked, null,
                         l[at:at + k].contiguous(), clim, cnt, ht, nt)
        at += k
    assert at == B
    return ht.cpu().numpy(), None if nt is None else nt.cpu().numpy()


def _check(got, want, mag, what):
    assert got.shape == want.shape and not np.isnan(got).any(), what
    assert np.array_equal(got[:, [0, 5]], want[:, [0, 5]]), f"{what}: the counts differ"
    ratio = np.abs(got - want) / np.where(mag > 0, mag, 1.0)
    worst = float(ratio.max())
    print(f"{what}: worst ratio {worst:.2e}")
    assert worst <= REL, f"{what}: worst |got - want| / sum of magnitudes {worst:.2e} at column {int(ratio.max(0).argmax())}"


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", list(SHAPES))
def test_tables_vs_reference(case, mode):
    _need_gpu()
    shape, updates = SHAPES[case]
    k = list(SHAPES).index(case) + list(MODES).index(mode)
    dtype = (np.float32, np.float64)[k % 2]
    period = _period(PERIODS[k % len(PERIODS)], shape[2])
    nodes = (k // 2) % 2 == 0 or case.startswith("6x2200")
    pred, target, pos, series, t_end = _inputs(shape, dtype, mode, period, seed=100 + k)
    want, mag = SR.skill_sums(pred, target, pos, series, period, t_end, MODES[mode], MODES[mode])
    ht, nt = _run(pred, target, pos, series, period, t_end, mode, nodes, updates)
    what = f"{case} {mode} {np.dtype(dtype).name} period {period}"
    _check(ht, want["horizon"], mag["horizon"], what + " horizon")
    if nodes:
        _check(nt, want["node"], mag["node"], what + " node")
    else:
        assert nt is None
    if shape != (1, 1, 1):  # (a period beyond the training steps leaves the test phases unobserved)
        assert want["horizon"][:, 0].sum() > 0 and (want["horizon"][:, 5].sum() > 0 or period > t_end)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", PERIODS)
@pytest.mark.parametrize("mode", ["none", "nan"])
def test_every_period_on_the_pems08_head(kind, dtype, mode):
    _need_gpu()
    shape = (4, 170, 12)
    period = _period(kind, 12)
    pred, target, pos, series, t_end = _inputs(shape, dtype, mode, period, seed=300 + PERIODS.index(kind))
    want, mag = SR.skill_sums(pred, target, pos, series, period, t_end, MODES[mode], MODES[mode])
    ht, nt = _run(pred, target, pos, series, period, t_end, mode)
    what = f"period {kind} = {period} {mode} {np.dtype(dtype).name}"
    _check(ht, want["horizon"], mag["horizon"], what + " horizon")
    _check(nt, want["node"], mag["node"], what + " node")
    if kind == "beyond-training":  # some phases were never observed: the climatology count falls short
        assert 0 < want["horizon"][:, 5].sum() < want["horizon"][:, 0].sum() or mode == "nan"
        assert want["horizon"][:, 5].sum() < np.isfinite(target).sum()


def test_the_gapped_series_exercises_every_undefined_case():
    """The inputs of the masked cases hold, non-empty, each situation the definitions single out."""
    shape, period = (4, 170, 12), 12
    pred, target, pos, series, t_end = _inputs(shape, np.float32, "nan", period, seed=7)
    clim, cnt = SR.climatology(series, period, t_end, NAN)
    q, qok = SR.persistence(series, pos, NAN)
    assert not qok[0, 0] and qok[:, 1:].all(axis=0).any()       # node 0: nothing observed before the first test label
    assert np.isnan(series[:t_end + 2, 0, -1]).all()            # ... a leading gap
    assert cnt[1, 1] == 0 and np.isnan(clim[1, 1]) and (cnt > 0).sum() > cnt.size // 2  # a never-observed (phase, node)
    cok = cnt[(pos[:, None] + np.arange(12)[None, :]) % period][:, :, :].transpose(0, 2, 1) > 0   # (B, N, P)
    both = qok[:, :, None] & cok
    assert (np.isnan(target) & both).any()                      # a missing target where both baselines are defined
    assert (~np.isnan(target) & ~both).any()                    # and a valid one where a baseline is not


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", ["7", "beyond-training", "L", "1"])
def test_climatology_table(kind, mode, dtype):
    _need_gpu()
    P, N = 12, 301  # two workgroups at period 1, many more otherwise
    period = _period(kind, P)
    _, _, _, series, t_end = _inputs((2, N, P), dtype, mode, period, seed=500)
    want, wcnt = SR.climatology(series, period, t_end, MODES[mode])
    s, _, clim, cnt, masked, null = _device_tables(series, period, t_end, mode)
    got, gcnt = clim.cpu().numpy(), cnt.cpu().numpy()
    assert got.shape == (period, N) and got.dtype == np.float64 and gcnt.dtype == np.int32
    assert np.array_equal(gcnt, wcnt)
    assert np.array_equal(np.isnan(got), gcnt == 0)
    ok = gcnt > 0
    worst = float(np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok])))
    print(f"climatology period {period} {mode} {np.dtype(dtype).name}: worst {worst:.2e}")
    assert worst <= 1e-12, worst
    if kind == "beyond-training":
        assert (gcnt == 0).any()
    # nothing at or beyond t_end influences it: the same bits after that range is overwritten
    from dstagnn_drought_amd import _lib
    pert = series.copy()
    pert[t_end:] = 1e6
    if masked:
        pert[t_end::2] = MODES[mode]
    c2, n2 = _lib.load().climatology(torch.from_numpy(pert).cuda(), period, t_end, masked, null)
    assert torch.equal(n2, cnt) and np.array_equal(c2.cpu().numpy().view(np.int64), got.view(np.int64))


@pytest.mark.parametrize("mode", list(MODES))
def test_exact_identities(mode):
    _need_gpu()
    from dstagnn_drought_amd import BaselineSkill
    shape, period = (4, 170, 12), 12
    marker = MODES[mode]
    pred, target, pos, series, t_end = _inputs(shape, np.float32, mode, period, seed=40)
    clim, cnt = SR.climatology(series, period, t_end, marker)
    q, qok = SR.persistence(series, pos, marker)
    # the prediction is the persistence forecast
    p1 = np.where(qok[:, :, None], q.astype(np.float32)[:, :, None], pred).astype(np.float32)
    ht, nt = _run(p1, target, pos, series, period, t_end, mode)
    for tab in (ht, nt):
        assert np.array_equal(tab[:, 1].view(np.int64), tab[:, 2].view(np.int64))
        assert np.array_equal(tab[:, 3].view(np.int64), tab[:, 4].view(np.int64))
    s = BaselineSkill.scores_of_table(ht)
    assert (ht[:, 2] > 0).all() and (s["mse_skill_persistence"] == 0.0).all() and (s["mae_skill_persistence"] == 0.0).all()
    # the prediction is float(clim)
    phase = (pos[:, None] + np.arange(12)[None, :]) % period
    c32 = clim[phase[:, None, :], np.arange(170)[None, :, None]].astype(np.float32)
    p2 = np.where(np.isnan(c32), pred, c32).astype(np.float32)
    ht, nt = _run(p2, target, pos, series, period, t_end, mode)
    for tab in (ht, nt):
        assert np.array_equal(tab[:, 6].view(np.int64), tab[:, 7].view(np.int64))
        assert (tab[:, 11] == 0.0).all()
    s = BaselineSkill.scores_of_table(ht)
    assert np.isnan(s["acc"]).all() and (s["mse_skill_climatology"] == 0.0).all()
    # the prediction equals the target (anything where the target is masked)
    p3 = np.where(SR.valid_target(target, marker), target, np.float32(3.0)).astype(np.float32)
    ht, _ = _run(p3, target, pos, series, period, t_end, mode)
    s = BaselineSkill.scores_of_table(ht)
    assert (ht[:, 2] > 0).all() and (ht[:, 7] > 0).all()
    assert (s["mse_skill_persistence"] == 1.0).all() and (s["mse_skill_climatology"] == 1.0).all()
    assert (s["mae_skill_persistence"] == 1.0).all() and (s["mae_skill_climatology"] == 1.0).all()


def test_nan_prediction_and_nan_target():
    _need_gpu()
    shape, period = (3, 7, 19), 7
    pred, target, pos, series, t_end = _inputs(shape, np.float64, "nan", period, seed=41)
    b, n, p = [int(v[0]) for v in np.nonzero(np.isnan(target))]  # a NaN target: a NaN prediction there changes nothing
    clean, _ = _run(pred, target, pos, series, period, t_end, "nan")
    pred2 = pred.copy()
    pred2[b, n, p] = NAN
    same, _ = _run(pred2, target, pos, series, period, t_end, "nan")
    assert np.array_equal(clean.view(np.int64), same.view(np.int64)) and not np.isnan(clean).any()
    want, _ = SR.skill_sums(pred, target, pos, series, period, t_end, NAN, NAN)
    hit = np.argwhere(~np.isnan(target) & (np.arange(7)[None, :, None] > 1))[0]  # a counted entry
    pred2 = pred.copy()
    pred2[tuple(hit)] = NAN
    bad, _ = _run(pred2, target, pos, series, period, t_end, "nan")
    assert np.isnan(bad[hit[2], [1, 3]]).all() and np.array_equal(bad[:, [0, 5]], want["horizon"][:, [0, 5]])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_out_of_range_labels_contribute_nothing(dtype):
    _need_gpu()
    shape, period = (5, 101, 3), 7
    L, _ = _geometry(3)
    extra = (-1, -7, L - 2, L, 1 << 40, -(1 << 40))  # l < 0, or l + P > L
    pred, target, pos, series, t_end = _inputs(shape, dtype, "neq", period, seed=42, extra_pos=extra)
    assert len(pos) == 11
    order = np.array([5, 0, 6, 1, 2, 7, 8, 3, 9, 4, 10])  # the bad ones between the good ones
    all_, nall = _run(pred[order], target[order], pos[order], series, period, t_end, "neq")
    good, ngood = _run(pred[:5], target[:5], pos[:5], series, period, t_end, "neq")
    assert np.array_equal(all_.view(np.int64), good.view(np.int64))
    assert np.array_equal(nall.view(np.int64), ngood.view(np.int64))
    want, mag = SR.skill_sums(pred[order], target[order], pos[order], series, period, t_end, -9999.0, -9999.0)
    _check(all_, want["horizon"], mag["horizon"], "out-of-range labels")


def _windowed(L, N, F, P, dtype, marker, seed, **kw):
    from dstagnn_drought_amd import WindowedSeries
    series = SR.gapped_series(L, N, F, dtype, marker, seed, period=12, t_end=(L * 3) // 5, lead=(L * 4) // 5 + 3)
    return series, WindowedSeries(series, 0, 0, 1, P, points_per_hour=P, device="cuda", missing_value=marker, **kw)


def _split_inputs(ws, series, marker, seed):
    sp = ws.split("test")
    _, y = sp.batch(slice(None))
    t = y.cpu().numpy()
    fin = np.where(np.isnan(t) | (t == np.float32(-9999.0)), np.float32(1.0), t)
    pred = (fin + np.random.default_rng(seed).normal(0, 1, t.shape)).astype(np.float32)
    return torch.from_numpy(pred).cuda(), y, ws.labels["test"]


@pytest.mark.parametrize("mode", list(MODES))
def test_class_vs_reference_determinism_additivity_and_merge(mode):
    _need_gpu()
    from dstagnn_drought_amd import BaselineSkill
    marker = MODES[mode]
    L, N, F, P, period = 160, 37, 2, 5, 12
    series, ws = _windowed(L, N, F, P, np.float32, marker, seed=60)
    pred, y, labels = _split_inputs(ws, series, marker, 61)
    B = len(labels)
    t_end = int(ws.labels["train"][-1]) + P
    assert B >= 8 and t_end <= labels[0]
    want, mag = SR.skill_sums(pred.cpu().numpy(), y.cpu().numpy(), labels, series, period, t_end, marker, marker)

    def fed(cuts, idx_kind="slice"):
        sk = BaselineSkill(ws, period, missing_value=marker, num_nodes=N)
        for b, e in cuts:
            idx = {"slice": slice(b, e), "list": list(range(b, e)),
                   "tensor": torch.arange(b, e, device="cuda")}[idx_kind]
            sk.update(pred[b:e], y[b:e], "test", idx)
        return sk
    one = fed([(0, B)])
    assert one.t_end == t_end and one.table.shape == (P, 13) and one.node_table.shape == (N, 13)
    ht, nt = one.table.cpu().numpy(), one.node_table.cpu().numpy()
    _check(ht, want["horizon"], mag["horizon"], f"class {mode} horizon")
    _check(nt, want["node"], mag["node"], f"class {mode} node")
    clim, cnt = one.climatology()
    wclim, wcnt = SR.climatology(series, period, t_end, marker)
    assert np.array_equal(cnt, wcnt) and np.array_equal(np.isnan(clim), wcnt == 0)
    # the scores are the reference's arithmetic on the table; per node without the overall entry
    for k, v in SR.scores(ht).items():
        assert np.array_equal(one.scores()[k], v, equal_nan=True) and v.shape == (P + 1,), k
    assert all(v.shape == (N,) for v in one.node_scores().values())
    # determinism: equal bits, whatever form idx takes
    for kind in ("slice", "list", "tensor"):
        again = fed([(0, B)], kind)
        assert torch.equal(again.table.view(torch.int64), one.table.view(torch.int64)), kind
        assert torch.equal(again.node_table.view(torch.int64), one.node_table.view(torch.int64)), kind
    # two half-batches: the same counts, the rest within the bound; merge equals one object fed everything
    h = B // 2
    halves = fed([(0, h), (h, B)])
    _check(halves.table.cpu().numpy(), want["horizon"], mag["horizon"], "two halves horizon")
    _check(halves.node_table.cpu().numpy(), want["node"], mag["node"], "two halves node")
    assert torch.equal(halves.table[:, [0, 5]], one.table[:, [0, 5]])
    a, b = fed([(0, h)]), fed([(h, B)])
    merged = a.merge(b)
    _check(merged.table.cpu().numpy(), ht, mag["horizon"], "merge horizon")
    _check(merged.node_table.cpu().numpy(), nt, mag["node"], "merge node")
    with pytest.raises(ValueError):
        a.merge(BaselineSkill(ws, 7, missing_value=marker, num_nodes=N))
    # a position outside the split contributes nothing; reset clears
    one.reset()
    assert not one.table.any() and not one.node_table.any()
    idx = torch.tensor([0, -1, 1, B, 2], device="cuda")
    sel = torch.tensor([0, 0, 1, 0, 2], device="cuda")
    one.update(pred[sel], y[sel], "test", idx)
    three = fed([(0, 3)])
    assert torch.equal(one.table.view(torch.int64), three.table.view(torch.int64))
    # refusals on the device too
    with pytest.raises(ValueError, match="point_index"):
        one.update(pred[:2, :, :, None].expand(2, N, P, 3), y[:2], "test", slice(0, 2))
    with pytest.raises(ValueError):
        one.update(pred[:2], y[:2], "test", slice(0, 3))


def test_the_forward_fill_is_reused_or_made_once():
    _need_gpu()
    from dstagnn_drought_amd import BaselineSkill
    series, ws = _windowed(160, 11, 2, 5, np.float64, NAN, seed=62, fill="ffill")
    sk = BaselineSkill(ws, 12, missing_value=NAN)
    assert sk._pers is ws.filled and sk.node_table is None
    series, ws2 = _windowed(160, 11, 2, 5, np.float64, NAN, seed=62, fill="ffill", max_gap=2)
    sk2 = BaselineSkill(ws2, 12, missing_value=NAN)
    assert sk2._pers is not ws2.filled
    assert torch.equal(sk2._pers.view(torch.int64), ws.filled.view(torch.int64))  # the unlimited fill
    series, ws3 = _windowed(160, 11, 2, 5, np.float64, None, seed=62)
    assert BaselineSkill(ws3, 12)._pers is ws3.series
    pred, y, labels = _split_inputs(ws, series, NAN, 63)
    sk.update(pred, y, "test", slice(None))
    sk2.update(pred, y, "test", slice(None))
    assert torch.equal(sk.table.view(torch.int64), sk2.table.view(torch.int64))


@pytest.mark.parametrize("mode", list(MODES))
def test_agrees_with_forecast_metrics_on_a_gap_free_series(mode):
    _need_gpu()
    from dstagnn_drought_amd import BaselineSkill, ForecastMetrics
    marker = MODES[mode]
    L, N, P = 160, 37, 5
    series, ws = _windowed(L, N, 2, P, np.float32, None, seed=64)  # no gaps: both baselines defined everywhere
    pred, y, labels = _split_inputs(ws, series, None, 65)
    if marker is not None:  # ... but some targets are masked
        y = y.clone()
        y[torch.from_numpy(np.random.default_rng(66).random(tuple(y.shape)) < 0.3).cuda()] = marker
    sk = BaselineSkill(ws, 12, missing_value=marker, num_nodes=N)
    fm = ForecastMetrics(P, 0.0, "cuda", missing_value=marker, num_nodes=N)
    sk.update(pred, y, "test", slice(None))
    fm.update(pred, y)
    for got, ref, what in ((sk.table, fm.table, "horizon"), (sk.node_table, fm.node_table, "node")):
        got, ref = got.cpu().numpy(), ref.cpu().numpy()
        assert np.array_equal(got[:, 0], ref[:, 0]) and np.array_equal(got[:, 5], ref[:, 0]), what
        for c in (3, 8):
            worst = float(np.max(np.abs(got[:, c] - ref[:, 2]) / ref[:, 2]))
            assert worst <= REL, (what, c, worst)
        assert (ref[:, 0] > 0).all()


@pytest.mark.parametrize("quantiles", [None, "0.1,0.5,0.9"])
def test_driver_scores_skill_beside_the_existing_scores(golden_dir, tmp_path, quantiles):
    _need_gpu()
    import configparser
    import test_gpu_metrics_masked as tmm
    from dstagnn_drought_amd import BaselineSkill
    from dstagnn_drought_amd import train as TR
    conf, td = tmm._g12_gapped(golden_dir, tmp_path)
    torch.cuda.set_device(0)
    kw = dict(stream_windows=True, missing_value=NAN, input_fill="mean", epochs=1, max_batches=2, dropout=0.0,
              test_metrics=True, node_scores=True, quantiles=quantiles)
    if quantiles is None:
        kw["loss"] = "masked_mae"
    lines = []
    res = TR.run(conf, root=os.path.join(td, "exp_skill"), log=lines.append, baseline_skill=True, climatology_period=12,
                 **kw)
    cp = configparser.ConfigParser()
    cp.read(conf)
    dc, tc = cp["Data"], cp["Training"]
    P, N, bs = int(dc["num_for_predict"]), int(dc["num_of_vertices"]), int(tc["batch_size"])
    net = res["net"]
    ws = TR._windowed_series(dc, tc, torch.device("cuda", 0), NAN, "mean", None)
    sp = ws.split("test")

    # every pre-existing key and file: what the same scoring pass without the option gives for this net
    # (two trainings are not compared: the scoring of one net is what the option could touch)
    base_dir = os.path.join(td, "base_scores")
    os.makedirs(base_dir)
    base_lines = []
    base = TR._score_test_split(net, sp.x, sp.y, bs, NAN, True, base_dir, base_lines.append,
                                TR.parse_quantiles(quantiles) if quantiles else None)
    fixed = {"best_epoch", "best_val", "test_loss", "history", "params_path", "net"}
    assert set(res) == fixed | set(base) | {"test_skill", "test_node_skill"}
    assert "test_skill" not in base and res["test_metrics"] == base["test_metrics"]
    for key in ("test_scores", "test_node_scores") + (("test_quantile_scores", "test_node_quantile_scores")
                                                      if quantiles else ()):
        assert sorted(res[key]) == sorted(base[key])
        for k, v in base[key].items():
            assert np.array_equal(res[key][k], v, equal_nan=True), (key, k)
    files = sorted(os.listdir(base_dir))
    assert sorted(f for f in os.listdir(res["params_path"]) if f.startswith("test_")) == \
        sorted(files + ["test_skill.json", "test_node_skill.npz"])
    for f in files:
        if f.endswith(".json"):
            with open(os.path.join(base_dir, f)) as a, open(os.path.join(res["params_path"], f)) as b:
                assert a.read() == b.read(), f
    assert [ln for ln in lines if ln.startswith("Test ") and not ln.startswith("Test skill ")] == base_lines

    # the skill scores: a fresh object fed the same cuts of predictions recomputed from the returned net
    sk = BaselineSkill(ws, 12, missing_value=NAN, num_nodes=N)
    preds, targets = [], []
    with torch.no_grad():
        for b in range(0, sp.x.shape[0], bs):
            xb, yb = TR._cut(sp.x, sp.y, b, b + bs)
            out = net(xb)
            if quantiles:
                assert out.shape[1:] == (N, P, 3)
                out = out[..., 1]
            sk.update(out, yb, "test", slice(b, b + bs))
            preds.append(out.cpu().numpy())
            targets.append(yb.cpu().numpy())
    got = res["test_skill"]
    for k, v in sk.scores().items():
        assert got[k].shape == (P + 1,) and np.array_equal(got[k], v, equal_nan=True), k
    for k, v in sk.node_scores().items():
        assert res["test_node_skill"][k].shape == (N,) and np.array_equal(res["test_node_skill"][k], v, equal_nan=True), k
    # ... and the table behind them against the reference
    p, t = np.concatenate(preds, 0), np.concatenate(targets, 0)
    series = ws.series.cpu().numpy()
    t_end = int(ws.labels["train"][-1]) + P
    want, mag = SR.skill_sums(p, t, ws.labels["test"], series, 12, t_end, NAN, NAN)
    _check(sk.table.cpu().numpy(), want["horizon"], mag["horizon"], "driver horizon")
    _check(sk.node_table.cpu().numpy(), want["node"], mag["node"], "driver node")
    assert (want["horizon"][:, 0] > 0).all() and (want["horizon"][:, 5] > 0).all()

    # one line per horizon and one overall; the files
    sl = [ln for ln in lines if ln.startswith("Test skill ")]
    assert len(sl) == P + 1 and sl[-1].startswith("Test skill overall: ") and sl[0].startswith("Test skill horizon 0: ")
    for i, ln in enumerate(sl):
        for k in ("mse_skill_persistence", "mse_skill_climatology", "acc"):
            assert "%s %.4f" % (k, got[k][i]) in ln, (i, k)
    with open(os.path.join(res["params_path"], "test_skill.json")) as f:
        saved = json.load(f)
    assert saved.pop("period") == 12 and sorted(saved) == sorted(got)
    for k in got:
        assert np.array_equal(np.array(saved[k], dtype=np.float64), got[k], equal_nan=True), k
    with np.load(os.path.join(res["params_path"], "test_node_skill.npz")) as f:
        assert sorted(f.files) == sorted(got)
        assert all(np.array_equal(f[k], res["test_node_skill"][k], equal_nan=True) for k in got)
