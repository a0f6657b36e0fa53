"""GPU: the masked test-set scores (csrc/loss.hip metrics_masked_kernel; ForecastMetrics with
missing_value / num_nodes; the driver's test_metrics / node_scores) against a float64 restatement
with numpy boolean masks on the same fp32 inputs.

Inputs are seeded: target ~ 3 N(0, 1), pred = target + N(0, 1), 20 % of the targets set to 0
(left out of MAPE), then 30 % set to the marker (NaN, or -9999 for the != mode; none under the
no-mask mode).

Bounds (derived; none of them measured):
  MAE, RMSE, MAPE  <= 1e-6 relative: every term is non-negative and carries at most three fp32
                   roundings (pred - t, then e * e or e / t), every add is fp64.  Counts are exact.
  bias             |got - want| <= 1e-6 MAE: a signed sum of terms, each within 2^-24 of its magnitude.
  NSE              |got - want| <= 1e-6 |1 - want|: 1 - NSE = sum e^2 / D with D = sum t^2 -
                   (sum t)^2 / n.  sum t and sum t^2 are fp64 sums of exact terms, so D's relative
                   error is at most k n 2^-53 with the cancellation factor k = sum t^2 / D =
                   1 + mean^2 / var: 1 - NSE inherits the bound of sum e^2.  k <= 2 where
                   |mean| <= std, as over the many entries of t = 3 randn; a horizon or node of a
                   handful of entries can have its mean beyond its spread, so the precondition
                   asserted on the reference is k <= 1e4 (1e4 * 1e5 entries * 2^-53 ~ 1e-7 of
                   the bound).

Measured on the MI355X, worst over the cases below: list 6.9e-8; horizon scores MAPE 6.9e-8,
NSE 6.7e-8; node scores MAPE 8.9e-8, NSE 8.4e-8; the driver test 1.5e-8.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
REL = 1e-6
MODES = {"none": None, "neq": -9999.0, "nan": NAN}
KEYS = ("count", "mae", "rmse", "mape", "bias", "nse")

# (B, N, P), the sizes of the updates along B, (emptied horizon, emptied node) or None
CASES = {
    "1x1x1-valid": ((1, 1, 1), [1], None),
    "1x1x1-masked": ((1, 1, 1), [1], "all"),
    "5x101x3-two-strips-two-updates": ((5, 101, 3), [2, 3], None),
    "4x170x12-pems08-head": ((4, 170, 12), [4], None),
    "3x7x19-idle-threads": ((3, 7, 19), [3], (5, 2)),
    "3x23x100-tn2": ((3, 23, 100), [3], None),
    "2x9x129-tn1-idle": ((2, 9, 129), [2], None),
    "2x5x256-tn1-full": ((2, 5, 256), [2], None),
    "6x2200x12-105-workgroups": ((6, 2200, 12), [6], None),
}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _valid(t, marker):
    if marker is None:
        return np.ones(t.shape, dtype=bool)
    return ~np.isnan(t) if marker != marker else t != np.float32(marker)


def _inputs(case, mode):
    """(pred, target) fp32 numpy arrays of a case under a mask mode, and whether rows were emptied."""
    shape, _, emptied = CASES[case]
    marker = MODES[mode]
    g = torch.Generator().manual_seed(9000 + 31 * list(CASES).index(case))
    t = 3.0 * torch.randn(shape, generator=g)
    p = t + torch.randn(shape, generator=g)
    if shape != (1, 1, 1):
        t[torch.rand(shape, generator=g) < 0.2] = 0.0
    if marker is not None:
        if shape != (1, 1, 1):
            t[torch.rand(shape, generator=g) < 0.3] = marker
        if emptied == "all":
            t[...] = marker
        elif emptied is not None:
            t[:, :, emptied[0]] = marker
            t[:, emptied[1], :] = marker
    return p.numpy(), t.numpy(), (emptied if marker is not None else None)


def ref_sums(p, t, marker, axes):
    """The eight float64 sums over the valid entries, reduced over `axes` of (B, N, P): a (K, 8)
    array, and the (K, 8) sums of the terms' magnitudes (the scale of an add-order difference)."""
    p64, t64 = p.astype(np.float64), t.astype(np.float64)
    v = _valid(t, marker)
    ape = v & (t64 != 0.0)
    tz = np.where(v, t64, 0.0)  # the masked targets (NaN among them) never reach a sum
    e = np.where(v, p64 - tz, 0.0)
    er = np.zeros_like(e)
    np.divide(e, t64, out=er, where=ape)
    cols = [v.astype(np.float64), e, np.abs(e), e * e, np.abs(er), ape.astype(np.float64), tz, tz * tz]
    sums = np.stack([c.sum(axis=axes) for c in cols], -1)
    mags = np.stack([np.abs(c).sum(axis=axes) for c in cols], -1)
    return sums, mags


def ref_scores(tab):
    """The scores of a (K, 8) float64 table, NaN where a divisor is 0."""
    def over(a, b):
        out = np.full(a.shape, np.nan)
        np.divide(a, b, out=out, where=b != 0)
        return out
    n = tab[:, 0]
    d = tab[:, 7] - over(tab[:, 6] ** 2, n)
    return {"count": n, "mae": over(tab[:, 2], n), "rmse": np.sqrt(over(tab[:, 3], n)),
            "mape": 100.0 * over(tab[:, 4], tab[:, 5]), "bias": over(tab[:, 1], n),
            "nse": 1.0 - over(tab[:, 3], np.where(np.isnan(d), 0.0, d))}


def ref_list(tab):
    tab = np.concatenate([tab, tab.sum(0, keepdims=True)], 0)
    s = ref_scores(tab)
    out = []
    for i in range(tab.shape[0]):
        out.extend([float(s["mae"][i]), float(s["rmse"][i]), 0.0 if tab[i, 5] == 0 else float(s["mape"][i])])
    return out


def check_scores(got, want, what):
    """The module's bounds on a dict of score arrays; NaN exactly where the reference is NaN.
    Returns the worst measured value of each bound's left side over its right side's scale."""
    worst = {}
    assert sorted(got) == sorted(KEYS), (what, sorted(got))
    assert np.array_equal(got["count"], want["count"]), what
    for k in KEYS[1:]:
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == np.float64, (what, k)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, k, g, w)
        ok = ~np.isnan(w)
        if not ok.any():
            continue
        scale = {"bias": want["mae"], "nse": np.abs(1.0 - w)}.get(k, np.abs(w))[ok]
        err = np.abs(g[ok] - w[ok])
        worst[k] = float((err / np.where(scale > 0, scale, 1.0)).max())
        assert (err <= REL * scale).all(), (what, k, worst[k])
    return worst


def check_list(got, want, what):
    assert len(got) == len(want) and all(isinstance(v, float) for v in got), what
    worst = 0.0
    for i, (a, b) in enumerate(zip(got, want)):
        if math.isnan(b):
            assert math.isnan(a), (what, i, a)
            continue
        assert abs(a - b) <= REL * abs(b), (what, i, a, b)
        if b != 0:
            worst = max(worst, abs(a - b) / abs(b))
    return worst


def _bits(t):
    return t.clone().view(torch.int64)


# every case under the three mask modes (a single masked entry needs a mask)
GRID = [(c, m) for c in CASES for m in MODES if not (c == "1x1x1-masked" and m == "none")]


@pytest.mark.parametrize("case,mode", GRID)
def test_masked_tables_match_fp64(case, mode):
    _need_gpu()
    from dstagnn_drought_amd import ForecastMetrics
    marker = MODES[mode]
    (B, N, P), parts, _ = CASES[case]
    p, t, emptied = _inputs(case, mode)
    hsum, hmag = ref_sums(p, t, marker, (0, 1))
    nsum, nmag = ref_sums(p, t, marker, (0, 2))
    # the precondition, on the reference alone: every horizon and node has a valid entry except
    # those emptied on purpose; the NSE bound's cancellation factor
    hz = set(np.flatnonzero(hsum[:, 0] == 0).tolist())
    nz = set(np.flatnonzero(nsum[:, 0] == 0).tolist())
    if emptied == "all":
        assert hz == {0} and nz == {0}
    elif emptied is not None:
        assert hz == {emptied[0]} and nz == {emptied[1]}
    else:
        assert not hz and not nz
    for tab in (np.concatenate([hsum, hsum.sum(0, keepdims=True)]), nsum):
        d = tab[:, 7] - tab[:, 6] ** 2 / np.maximum(tab[:, 0], 1)
        live = d > 0
        assert (tab[live, 7] / d[live] <= 1e4).all(), (case, mode, float((tab[live, 7] / d[live]).max()))

    pd, td = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
    m = ForecastMetrics(P, 0.0, "cuda", missing_value=marker, num_nodes=N)
    assert m.table.shape == (P, 8) and m.node_table.shape == (N, 8)
    runs = []
    for _ in range(2):
        at = 0
        for s in parts:
            m.update(pd[at:at + s], td[at:at + s])
            at += s
        runs.append((_bits(m.table), _bits(m.node_table), m.compute(), m.scores(), m.node_scores()))
        m.reset()
        assert float(m.table.abs().sum()) == 0.0 and float(m.node_table.abs().sum()) == 0.0 and m.rows == 0
    ht, nt, lst, sc, nsc = runs[0]
    # the same updates again: the same bits in both tables
    assert torch.equal(ht, runs[1][0]) and torch.equal(nt, runs[1][1])
    htab, ntab = ht.view(torch.float64).cpu().numpy(), nt.view(torch.float64).cpu().numpy()
    assert np.isfinite(htab).all() and np.isfinite(ntab).all()
    # counts exact, against the reference and between the two tables; the rest of the column sums
    # within 1e-12 of the terms' magnitudes (two add orders of the same fp64 terms)
    assert np.array_equal(htab[:, [0, 5]], hsum[:, [0, 5]]) and np.array_equal(ntab[:, [0, 5]], nsum[:, [0, 5]])
    a, b = htab.sum(0), ntab.sum(0)
    assert a[0] == b[0] and a[5] == b[5]
    assert (np.abs(a - b) <= 1e-12 * hmag.sum(0)).all(), (case, mode, a, b)

    w1 = check_list(lst, ref_list(hsum), (case, mode))
    assert len(lst) == 3 * P + 3
    w2 = check_scores(sc, ref_scores(np.concatenate([hsum, hsum.sum(0, keepdims=True)])), (case, mode, "scores"))
    w3 = check_scores(nsc, ref_scores(nsum), (case, mode, "node_scores"))
    assert all(v.shape == (P + 1,) for v in sc.values()) and all(v.shape == (N,) for v in nsc.values())
    print(f"{case} / {mode}: worst list {w1:.2e}, scores {w2}, node scores {w3}")
    if emptied == "all":
        assert math.isnan(lst[0]) and math.isnan(lst[1]) and lst[2] == 0.0 and sc["count"].tolist() == [0.0, 0.0]
        assert all(np.isnan(sc[k]).all() for k in KEYS[1:])


def test_without_a_node_table_and_against_the_unmasked_object():
    """ntable = NULL computes the same horizon table; with no mask the list is the old object's
    to 1e-6 (its sums are taken in another order and from the same fp32 terms)."""
    _need_gpu()
    from dstagnn_drought_amd import ForecastMetrics
    p, t, _ = _inputs("4x170x12-pems08-head", "none")
    pd, td = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
    old = ForecastMetrics(12, 0.0, "cuda")
    with_nodes = ForecastMetrics(12, 0.0, "cuda", num_nodes=170)
    for m in (old, with_nodes):
        m.update(pd, td)
    assert old.table.shape == (12, 4) and with_nodes.table.shape == (12, 8)
    worst = check_list(with_nodes.compute(), old.compute(), "unmasked")
    print(f"masked kernel, no mask, against the (P, 4) object: worst {worst:.2e}")
    so = old.scores()
    assert sorted(so) == ["count", "mae", "mape", "rmse"] and so["count"][-1] == 4 * 170 * 12
    assert abs(so["mae"][-1] - old.compute()[-3]) <= 1e-15 * so["mae"][-1]
    with pytest.raises(ValueError):
        old.node_scores()
    # a mask without a node table: the same horizon bits as with one
    pn, tn, _ = _inputs("4x170x12-pems08-head", "nan")
    pn, tn = torch.from_numpy(pn).cuda(), torch.from_numpy(tn).cuda()
    a = ForecastMetrics(12, 0.0, "cuda", missing_value=NAN)
    b = ForecastMetrics(12, 0.0, "cuda", missing_value=NAN, num_nodes=170)
    a.update(pn, tn)
    b.update(pn, tn)
    assert a.node_table is None and torch.equal(_bits(a.table), _bits(b.table))
    with pytest.raises(ValueError):
        b.update(pn[:, :169], tn[:, :169])  # num_nodes is checked
    # a NaN null value of the != mode is the NaN mode
    from dstagnn_drought_amd import _lib
    ops = _lib.load()
    h = torch.zeros(12, 8, dtype=torch.float64, device="cuda")
    ops.metrics_update_masked(pn, tn, 1, NAN, 0.0, h, None)
    assert torch.equal(_bits(h), _bits(a.table))


def test_the_shared_ticket_and_the_old_path_keep_their_bits():
    """The masked kernel draws the stream's one ticket counter and leaves it at zero: old-path
    objects fed before and after a masked update hold the same bits, and so does the loss."""
    _need_gpu()
    from dstagnn_drought_amd import ForecastMetrics, HipLoss
    g = torch.Generator().manual_seed(11)
    t = 3.0 * torch.randn(32, 170, 12, generator=g)
    y = (t + torch.randn(32, 170, 12, generator=g)).cuda()
    t[torch.rand(t.shape, generator=g) < 0.3] = 0.0
    t = t.cuda()
    crit = HipLoss("smooth_l1", null_val=0.0)
    first_loss = crit(y, t).clone()
    before = ForecastMetrics(12, 0.0, "cuda")
    before.update(y, t)
    masked = ForecastMetrics(12, 0.0, "cuda", missing_value=0.0, num_nodes=170)
    masked.update(y, t)
    masked.update(y[:3], t[:3])
    after = ForecastMetrics(12, 0.0, "cuda")
    after.update(y, t)
    last_loss = crit(y, t)
    assert torch.equal(_bits(before.table), _bits(after.table))
    assert torch.equal(first_loss.view(torch.int32), last_loss.view(torch.int32))
    again = ForecastMetrics(12, 0.0, "cuda", missing_value=0.0, num_nodes=170)
    again.update(y, t)
    again.update(y[:3], t[:3])
    assert torch.equal(_bits(masked.table), _bits(again.table))
    assert torch.equal(_bits(masked.node_table), _bits(again.node_table))


def test_nan_targets_are_selected_out():
    _need_gpu()
    from dstagnn_drought_amd import ForecastMetrics
    p, t, _ = _inputs("5x101x3-two-strips-two-updates", "nan")
    assert np.isnan(t).any() and np.isfinite(p).all()
    pd, td = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
    a = ForecastMetrics(3, 0.0, "cuda", missing_value=NAN, num_nodes=101)
    a.update(pd, td)
    assert bool(torch.isfinite(a.table).all()) and bool(torch.isfinite(a.node_table).all())
    # a NaN (or infinite) prediction at a masked position changes nothing
    p2 = pd.clone()
    hole = torch.isnan(td)
    p2[hole] = NAN
    p2[hole & (torch.rand(p2.shape, generator=torch.Generator().manual_seed(5)).cuda() < 0.5)] = float("inf")
    b = ForecastMetrics(3, 0.0, "cuda", missing_value=NAN, num_nodes=101)
    b.update(p2, td)
    assert torch.equal(_bits(a.table), _bits(b.table)) and torch.equal(_bits(a.node_table), _bits(b.node_table))
    # a NaN prediction at a VALID entry shows, as in the loss
    p3 = pd.clone()
    where = (~hole).nonzero()[0]
    p3[tuple(where)] = NAN
    c = ForecastMetrics(3, 0.0, "cuda", missing_value=NAN, num_nodes=101)
    c.update(p3, td)
    assert math.isnan(c.compute()[3 * int(where[2])]) and math.isnan(float(c.node_table[int(where[1]), 2]))
    assert c.table[:, 0].equal(a.table[:, 0])


def test_merge_equals_one_object_fed_everything():
    _need_gpu()
    from dstagnn_drought_amd import ForecastMetrics
    p, t, _ = _inputs("5x101x3-two-strips-two-updates", "neq")
    pd, td = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
    kw = dict(missing_value=-9999.0, num_nodes=101)
    whole, left, right = (ForecastMetrics(3, 0.0, "cuda", **kw) for _ in range(3))
    for b in range(5):
        whole.update(pd[b:b + 1], td[b:b + 1])
        (left if b < 2 else right).update(pd[b:b + 1], td[b:b + 1])
    assert left.merge(right) is left and left.rows == whole.rows == 5 * 101
    # counts exact; the rest within 1e-12 of the terms' magnitudes (another order of the same adds)
    for got, want, axes in ((left.table, whole.table, (0, 1)), (left.node_table, whole.node_table, (0, 2))):
        got, want = got.cpu().numpy(), want.cpu().numpy()
        _, mag = ref_sums(p, t, -9999.0, axes)
        assert np.array_equal(got[:, [0, 5]], want[:, [0, 5]])
        assert (np.abs(got - want) <= 1e-12 * mag).all()
    assert left.all_reduce() is left  # no process group: nothing happens
    assert left.rows == 5 * 101
    for other in (ForecastMetrics(3, 0.0, "cuda", missing_value=-9999.0), ForecastMetrics(3, 0.0, "cuda"),
                  ForecastMetrics(3, 0.0, "cuda", missing_value=NAN, num_nodes=101),
                  ForecastMetrics(3, 1.0, "cuda", **kw)):
        with pytest.raises(ValueError):
            left.merge(other)
    old_a, old_b = ForecastMetrics(3, 0.0, "cuda"), ForecastMetrics(3, 0.0, "cuda")
    old_a.update(pd[:2], td[:2])
    old_b.update(pd[2:], td[2:])
    assert old_a.merge(old_b).rows == 5 * 101


def _g12_gapped(golden_dir, tmp_path):
    """The g12 fixture laid out as tests/test_gpu_loss.py::_g12 does, 20 % of the series NaN."""
    g = dict(np.load(os.path.join(golden_dir, "g12_train.npz"), allow_pickle=False))
    td = str(tmp_path)
    for k in ("adj.csv", "stag.csv", "strg.csv"):
        with open(os.path.join(td, k), "w") as f:
            f.write(str(g[k + "_text"]))
    series = np.array(g["series"], copy=True)
    series[np.random.default_rng(61).random(series.shape) < 0.2] = NAN
    np.savez(os.path.join(td, "SYN.npz"), data=series)
    conf = os.path.join(td, "train.conf")
    with open(conf, "w") as f:
        f.write(str(g["config_text"]).replace("@DIR@", td))
    return conf, td


def test_driver_scores_the_test_split_of_a_gapped_series(golden_dir, tmp_path, capsys):
    _need_gpu()
    import configparser
    from dstagnn_drought_amd import train as TR
    conf, td = _g12_gapped(golden_dir, tmp_path)
    torch.cuda.set_device(0)
    kw = dict(stream_windows=True, loss="masked_mae", missing_value=NAN, input_fill="mean", epochs=1, max_batches=2,
              dropout=0.0)
    lines = []
    res = TR.run(conf, root=os.path.join(td, "exp_scored"), log=lines.append, test_metrics=True, node_scores=True,
                 **kw)
    cp = configparser.ConfigParser()
    cp.read(conf)
    dc, tc = cp["Data"], cp["Training"]
    P, N, bs = int(dc["num_for_predict"]), int(dc["num_of_vertices"]), int(tc["batch_size"])
    got = res["test_metrics"]
    assert len(got) == 3 * P + 3 and all(math.isfinite(v) for v in got)

    # the float64 restatement over predictions recomputed batch by batch from the returned net
    net = res["net"]
    ws = TR._windowed_series(dc, tc, torch.device("cuda", 0), NAN, "mean", None)
    sp = ws.split("test")
    loader, preds, targets = [], [], []
    with torch.no_grad():
        for b in range(0, sp.x.shape[0], bs):
            xb, yb = TR._cut(sp.x, sp.y, b, b + bs)
            loader.append((xb, yb))
            preds.append(net(xb).cpu().numpy())
            targets.append(yb.cpu().numpy())
    p, t = np.concatenate(preds, 0), np.concatenate(targets, 0)
    assert np.isnan(t).any() and np.isfinite(p).all() and t.shape == (sp.x.shape[0], N, P)
    hsum, _ = ref_sums(p, t, NAN, (0, 1))
    nsum, _ = ref_sums(p, t, NAN, (0, 2))
    assert (hsum[:, 0] > 0).all() and (nsum[:, 0] > 0).all()
    w1 = check_list(got, ref_list(hsum), "run")
    want_scores = ref_scores(np.concatenate([hsum, hsum.sum(0, keepdims=True)]))
    w2 = check_scores(res["test_scores"], want_scores, "run scores")
    w3 = check_scores(res["test_node_scores"], ref_scores(nsum), "run node scores")
    with capsys.disabled():
        print(f"\ndriver: worst list {w1:.2e}, scores {w2}, node scores {w3}")
    scored = [ln for ln in lines if ln.startswith("Test ")]
    assert len(scored) == P + 1 and scored[-1].startswith("Test overall: ") and "mae %.4f" % got[-3] in scored[-1]
    assert lines.index(scored[0]) > [i for i, ln in enumerate(lines) if ln.startswith("Final Test Loss")][0]

    # the files hold the same numbers
    with open(os.path.join(res["params_path"], "test_metrics.json")) as f:
        saved = json.load(f)
    assert saved["list"] == got
    for k in KEYS:
        assert np.array_equal(np.array(saved[k], dtype=np.float64), res["test_scores"][k], equal_nan=True), k
    with np.load(os.path.join(res["params_path"], "test_node_scores.npz")) as f:
        assert sorted(f.files) == sorted(KEYS)
        for k in KEYS:
            assert f[k].shape == (N,) and np.array_equal(f[k], res["test_node_scores"][k], equal_nan=True), k

    # the same run without the option: no such keys, no such files
    plain = TR.run(conf, root=os.path.join(td, "exp_plain"), log=lambda *_: None, **kw)
    assert not [k for k in plain if k.startswith("test_") and k != "test_loss"]
    assert sorted(plain) == ["best_epoch", "best_val", "history", "net", "params_path", "test_loss"]
    assert not os.path.exists(os.path.join(plain["params_path"], "test_metrics.json"))
    assert not os.path.exists(os.path.join(plain["params_path"], "test_node_scores.npz"))
    # test_metrics alone: no node scores
    only = TR.run(conf, root=os.path.join(td, "exp_only"), log=lambda *_: None, test_metrics=True, **kw)
    assert len(only["test_metrics"]) == 3 * P + 3 and sorted(only["test_scores"]) == sorted(KEYS)
    assert "test_node_scores" not in only
    assert os.path.exists(os.path.join(only["params_path"], "test_metrics.json"))
    assert not os.path.exists(os.path.join(only["params_path"], "test_node_scores.npz"))

    # the loader-style functions on the same net
    target = torch.from_numpy(t).cuda()
    capsys.readouterr()
    lst, node = TR.evaluate_on_test_masked(net, loader, target, None, 3, missing_value=NAN, per_node=True)
    out = capsys.readouterr().out
    assert lst == got  # the same batches in the same order: the same bits
    assert "current epoch: 3, predict %d points" % (P - 1) in out and "MAE: %.2f" % got[0] in out
    for k in KEYS:
        assert np.array_equal(node[k], res["test_node_scores"][k], equal_nan=True)
    assert TR.evaluate_on_test_masked(net, loader, target, None, 3, missing_value=NAN) == got
    mean, std = ws.mean, ws.std
    saved_list = TR.predict_and_save_results_mstgcn(net, loader, target, 0, mean, std, td, "test", missing_value=NAN)
    assert saved_list == got
    with np.load(os.path.join(td, "output_epoch_0_test.npz")) as f:
        assert sorted(f.files) == ["data_target_tensor", "input", "prediction"]
        assert np.array_equal(f["prediction"], p) and np.array_equal(f["data_target_tensor"], t, equal_nan=True)
    # the defaults on NaN targets: NaN MAE, today's behaviour (the default path is untouched)
    default = TR.evaluate_on_test_mstgcn(net, loader, target, None, 4, mean, std)
    capsys.readouterr()
    assert len(default) == 3 * P + 3 and math.isnan(default[-3]) and math.isnan(default[-2])
