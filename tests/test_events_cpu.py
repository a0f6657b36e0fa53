"""CPU: the surface of the drought event scores (csrc/loss.hip events_kernel behind its C-ABI,
dstagnn_drought_amd/loss.py EventScores / node_percentile_thresholds, the driver options of train.py)
that needs no GPU: the symbols are exported and the op registered, the C-ABI checks every argument
before anything touches the device (shape first, scratch last), nothing falls back to the CPU, every
threshold / percentile / option rule is a ValueError, the options resolve the same way from the key,
the keyword and the flag, the arithmetic from a table of counts to the scores is right (zero
divisors included), the update path holds no host synchronisation, and the numpy reference of
tests/test_gpu_events.py agrees with a naive triple loop.
"""
import configparser
import ctypes
import inspect
import math
import types

import numpy as np
import pytest
import torch

import events_ref as ER

E_SHAPE, E_ARG, E_SPACE = 10001, 10002, 10003
MASK_NONE, MASK_NEQ, MASK_NAN = 0, 1, 2
NAN = float("nan")
I64, I32, VP = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p


def c_abi():
    from dstagnn_drought_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.dstagnn_last_error.restype = ctypes.c_char_p
    lib.dstagnn_events_scratch_bytes.restype = I64
    lib.dstagnn_events_scratch_bytes.argtypes = [I64, I64, I32, I32]
    lib.dstagnn_events_accumulate.argtypes = [I64, I64, I32, I32, I32, VP, VP, I32, ctypes.c_float, VP, I32, VP, VP, VP,
                                              ctypes.c_size_t, VP]
    return lib


def _host_args():
    """Host memory standing in for the device buffers: every call below must return before it
    touches any of them."""
    buf = (ctypes.c_double * 64)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _events(lib, p, B=2, N=8, P=12, K=3, above=0, mask=MASK_NONE, per_node=0, scratch_bytes=1 << 24, **ptr):
    a = dict(pred=p, target=p, thr=p, htable=p, ntable=p, scratch=p)
    a.update(ptr)
    return lib.dstagnn_events_accumulate(B, N, P, K, above, a["pred"], a["target"], mask, 0.0, a["thr"], per_node,
                                         a["htable"], a["ntable"], a["scratch"], scratch_bytes, None)


def test_symbols_exported_op_registered_and_no_cpu_kernel():
    from dstagnn_drought_amd import _lib
    import dstagnn_drought_amd as D
    lib = c_abi()
    assert lib.dstagnn_events_scratch_bytes and lib.dstagnn_events_accumulate
    assert D.EventScores is D.loss.EventScores and "EventScores" in D.__all__
    assert D.node_percentile_thresholds is D.loss.node_percentile_thresholds
    assert "node_percentile_thresholds" in D.__all__
    ops = _lib.load()
    assert hasattr(ops, "events_update")
    z = torch.zeros(2, 3, 4)
    with pytest.raises(RuntimeError):  # no CPU kernel behind the op
        ops.events_update(z, z, 0, 0.0, torch.tensor([-1.0, -2.0]), False, torch.zeros(4, 11, dtype=torch.float64), None)


@pytest.mark.parametrize("kw", [dict(P=257), dict(P=0), dict(P=-3), dict(K=0), dict(K=8), dict(K=-1), dict(B=0),
                                dict(B=-1), dict(N=0), dict(N=-5), dict(B=1 << 14, N=1 << 14, P=8),
                                dict(B=1 << 40, N=1 << 40, P=1), dict(B=1, N=(1 << 31) // 7 + 1, P=1, K=7),
                                dict(K=7, P=256), dict(K=7, P=248), dict(K=7, P=1)])
def test_rejects_shapes_before_the_pointers(kw):
    lib = c_abi()
    buf, p = _host_args()
    assert _events(lib, p, **kw) == E_SHAPE, kw
    assert b"events_accumulate" in lib.dstagnn_last_error()
    # the shape is judged first
    assert _events(lib, p, pred=None, mask=9, above=2, per_node=-1, scratch_bytes=0, **kw) == E_SHAPE
    a = dict(B=2, N=8, P=12, K=3)
    a.update(kw)
    assert lib.dstagnn_events_scratch_bytes(a["B"], a["N"], a["P"], a["K"]) == 0
    del buf


def test_the_lds_rule_concerns_only_seven_levels_at_the_ends_of_the_horizon_range():
    """(P + 256 / P) (2 + (K + 1)^2) 4 bytes against 64 KiB: 257 rows of 66 counters do not fit, and
    257 rows are needed at P = 256 (one node per strip) and at P = 1 (256 nodes per strip) alike."""
    lib = c_abi()
    sb = lib.dstagnn_events_scratch_bytes
    for K in range(1, 8):
        for P in (1, 2, 3, 12, 128, 129, 247, 248, 256):
            lds = (P + 256 // P) * (2 + (K + 1) ** 2) * 4
            assert (sb(2, 9, P, K) == 0) == (lds > 65536) == (K == 7 and (P >= 248 or P == 1)), (K, P, lds)


def test_scratch_follows_the_grid():
    lib = c_abi()
    sb = lib.dstagnn_events_scratch_bytes
    for (B, N, P), K in [((1, 1, 1), 1), ((5, 23, 12), 3), ((3, 40, 7), 7), ((3, 257, 1), 6), ((2, 3, 256), 3),
                         ((2, 9, 129), 1), ((6, 2200, 12), 3)]:
        got = sb(B, N, P, K)
        assert got > 0 and got == -(-N // (256 // P)) * (2 + (K + 1) ** 2) * P * 8, (B, N, P, K, got)
    assert sb(6, 2200, 12, 3) // (18 * 12 * 8) == 105


@pytest.mark.parametrize("case", ["pred", "target", "thr", "htable", "scratch", "mask-1", "mask3", "above2", "above-1",
                                  "per_node2", "per_node-1"])
def test_rejects_null_pointers_modes_and_flags(case):
    lib = c_abi()
    buf, p = _host_args()
    if case.startswith("mask"):
        rc = _events(lib, p, mask=int(case[4:]))
    elif case.startswith("above"):
        rc = _events(lib, p, above=int(case[5:]))
    elif case.startswith("per_node"):
        rc = _events(lib, p, per_node=int(case[8:]))
    else:
        rc = _events(lib, p, **{case: None})
    assert rc == E_ARG
    assert b"events_accumulate" in lib.dstagnn_last_error()
    assert _events(lib, p, scratch_bytes=0, **({case: None} if case in ("pred", "thr") else dict(mask=7))) == E_ARG
    del buf


def test_rejects_small_scratch_last():
    lib = c_abi()
    buf, p = _host_args()
    need = lib.dstagnn_events_scratch_bytes(2, 170, 12, 3)
    assert need > 0
    assert _events(lib, p, N=170, ntable=None, scratch_bytes=need - 1) == E_SPACE
    assert b"scratch" in lib.dstagnn_last_error() and b"events_accumulate" in lib.dstagnn_last_error()
    assert _events(lib, p, N=170, pred=None, scratch_bytes=0) == E_ARG  # the pointers before the space
    del buf


def _row(a, b, c, d, nan_pred=0.0):
    """One K = 1 row: [count, nan_pred, M00 = d, M01 = b, M10 = c, M11 = a]."""
    return [a + b + c + d + nan_pred, nan_pred, d, b, c, a]


def test_scores_of_a_hand_filled_table():
    from dstagnn_drought_amd import EventScores
    tab = np.array([_row(3, 1, 2, 4, nan_pred=2), _row(0, 0, 0, 5), [0.0] * 6])
    s = EventScores.scores_of_table(tab)
    per_k = ["hits", "false_alarms", "misses", "correct_negatives", "base_rate", "pod", "far", "pofd", "csi",
             "freq_bias", "accuracy", "ets", "hss"]
    assert sorted(s) == sorted(["count", "nan_pred", "confusion", "observed_freq", "forecast_freq", "class_accuracy",
                                "hss_multi"] + per_k)
    assert all(v.dtype == np.float64 for v in s.values())
    assert all(s[k].shape == (4, 1) for k in per_k) and s["confusion"].shape == (4, 2, 2)
    assert s["observed_freq"].shape == s["forecast_freq"].shape == (4, 2)
    assert all(s[k].shape == (4,) for k in ("count", "nan_pred", "class_accuracy", "hss_multi"))
    assert s["count"].tolist() == [12.0, 5.0, 0.0, 17.0] and s["nan_pred"].tolist() == [2.0, 0.0, 0.0, 2.0]
    # row 0: a, b, c, d = 3, 1, 2, 4
    assert [s[k][0, 0] for k in ("hits", "false_alarms", "misses", "correct_negatives")] == [3.0, 1.0, 2.0, 4.0]
    assert s["pod"][0, 0] == pytest.approx(0.6, rel=1e-15) and s["far"][0, 0] == 0.25 and s["csi"][0, 0] == 0.5
    assert s["freq_bias"][0, 0] == pytest.approx(0.8, rel=1e-15) and s["hss"][0, 0] == pytest.approx(0.4, rel=1e-15)
    assert s["ets"][0, 0] == 0.25 and s["pofd"][0, 0] == pytest.approx(0.2, rel=1e-15)
    assert s["base_rate"][0, 0] == 0.5 and s["accuracy"][0, 0] == pytest.approx(0.7, rel=1e-15)
    assert s["confusion"][0].tolist() == [[4.0, 1.0], [2.0, 3.0]]
    assert s["observed_freq"][0].tolist() == [0.5, 0.5] and s["forecast_freq"][0].tolist() == [0.6, 0.4]
    assert s["class_accuracy"][0] == pytest.approx(0.7, rel=1e-15)
    assert s["hss_multi"][0] == pytest.approx(0.4, rel=1e-14)  # two classes: the Heidke score itself
    # row 1: no event observed or forecast: a + c = a + b = a + b + c = 0 -> NaN; hss has a zero divisor too
    for k in ("pod", "far", "csi", "freq_bias", "ets", "hss"):
        assert math.isnan(s[k][1, 0]), k
    assert s["pofd"][1, 0] == 0.0 and s["accuracy"][1, 0] == 1.0 and s["base_rate"][1, 0] == 0.0
    assert s["class_accuracy"][1] == 1.0 and math.isnan(s["hss_multi"][1])
    # the empty row: every divisor is 0
    for k in s:
        if k not in ("count", "nan_pred", "confusion", "hits", "false_alarms", "misses", "correct_negatives"):
            assert np.isnan(s[k][2]).all(), k
    # overall, from the column sums: a, b, c, d = 3, 1, 2, 9
    assert s["pod"][3, 0] == pytest.approx(0.6, rel=1e-15) and s["pofd"][3, 0] == 0.1
    assert s["hss"][3, 0] == pytest.approx(2.0 * (27 - 2) / (5 * 11 + 4 * 10), rel=1e-15)
    n = EventScores.scores_of_table(tab, overall=False)
    assert n["pod"].shape == (3, 1) and n["count"].shape == (3,)
    for bad in (np.zeros((3, 8)), np.zeros((3, 5)), np.zeros(6), np.zeros((3, 2 + 81))):
        with pytest.raises(ValueError):
            EventScores.scores_of_table(bad)


def test_scores_of_a_three_threshold_table_follow_the_nesting():
    """K = 3: the 2 x 2 table of threshold k is the confusion matrix cut at class k."""
    from dstagnn_drought_amd import EventScores
    rng = np.random.default_rng(3)
    M = rng.integers(0, 9, (5, 4, 4)).astype(np.float64)
    tab = np.concatenate([M.sum((1, 2))[:, None] + 1.0, np.ones((5, 1)), M.reshape(5, 16)], 1)
    s = EventScores.scores_of_table(tab, overall=False)
    for r in range(5):
        for k in range(3):
            a = sum(M[r, i, j] for i in range(4) for j in range(4) if i > k and j > k)
            b = sum(M[r, i, j] for i in range(4) for j in range(4) if i <= k and j > k)
            c = sum(M[r, i, j] for i in range(4) for j in range(4) if i > k and j <= k)
            d = sum(M[r, i, j] for i in range(4) for j in range(4) if i <= k and j <= k)
            assert (s["hits"][r, k], s["false_alarms"][r, k], s["misses"][r, k], s["correct_negatives"][r, k]) == \
                (a, b, c, d)
            assert s["csi"][r, k] == pytest.approx(a / (a + b + c), rel=1e-15)
        n = M[r].sum()
        pe = sum(M[r, i].sum() * M[r, :, i].sum() for i in range(4)) / n ** 2
        assert s["hss_multi"][r] == pytest.approx((np.trace(M[r]) / n - pe) / (1 - pe), rel=1e-12)


def test_threshold_rules_are_value_errors_that_name_the_rule():
    from dstagnn_drought_amd import EventScores
    from dstagnn_drought_amd.loss import check_thresholds
    ok = check_thresholds([-1.0, -1.5, -2.0])
    assert ok.dtype == np.float32 and ok.shape == (3,) and ok.flags["C_CONTIGUOUS"]
    assert check_thresholds(torch.tensor([1.0, 2.0]), "above").tolist() == [1.0, 2.0]
    assert check_thresholds(np.array([[-1.0, NAN], [-1.0, NAN]])).shape == (2, 2)  # a tie and an excluded node
    for thr, direction, word in [
            ([], "below", "shape"), (np.zeros((2, 2, 2)), "below", "shape"), (list(range(0, -8, -1)), "below", "between 1"),
            ("abc", "below", "numbers"), ([-1.0, -1.0], "below", "strictly decreasing"),
            ([-2.0, -1.0], "below", "strictly decreasing"), ([1.0, 1.0], "above", "strictly increasing"),
            ([2.0, 1.0], "above", "strictly increasing"), ([-1.0, -1.0 - 1e-9], "below", "same float"),
            ([-1.0, NAN], "below", "NaN"), ([NAN], "below", "NaN"), ([-1.0, -math.inf], "below", "infinite"),
            ([1e39], "above", "infinite"), (np.array([[-1.0, NAN], [-2.0, -2.0]]), "below", "mixes NaN"),
            (np.array([[-2.0, -1.0], [-1.0, -2.0]]), "below", "non-increasing"),
            (np.array([[1.0, 2.0], [2.0, 1.0]]), "above", "non-decreasing"),
            (np.array([[1.0, math.inf]]), "above", "infinite"), ([-1.0], "sideways", "direction")]:
        with pytest.raises(ValueError, match=word):
            check_thresholds(thr, direction)
        with pytest.raises(ValueError, match=word):  # the constructor refuses before it needs a device
            EventScores(12, thr, direction=direction, device="cpu")
    with pytest.raises(ValueError, match="num_nodes"):
        EventScores(12, np.array([[-1.0, -1.0, -1.0]]), num_nodes=4, device="cpu")
    with pytest.raises(ValueError, match="num_nodes"):
        EventScores(12, [-1.0], num_nodes=0, device="cpu")
    for P in (0, 257):
        with pytest.raises(ValueError, match="num_for_predict"):
            EventScores(P, [-1.0], device="cpu")
    for P in (1, 248, 256):
        with pytest.raises(ValueError, match="LDS"):
            EventScores(P, list(range(0, -7, -1)), device="cpu")
    with pytest.raises(ValueError):
        EventScores(12, [-1.0], missing_value=0.1, device="cpu")  # float32 does not hold it
    with pytest.raises(RuntimeError, match="HIP"):  # valid configurations on the CPU: no fallback
        EventScores(12, [-1.0, -1.5, -2.0], device="cpu")
    with pytest.raises(RuntimeError, match="HIP"):
        EventScores(247, list(range(0, -7, -1)), device="cpu")
    sig = inspect.signature(EventScores.__init__).parameters
    assert list(sig)[:3] == ["self", "num_for_predict", "thresholds"] and sig["direction"].default == "below"
    for k in ("direction", "missing_value", "num_nodes", "device"):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY


def test_update_judges_the_shapes_first_and_has_no_cpu_path():
    from dstagnn_drought_amd import EventScores
    ev = object.__new__(EventScores)
    ev.P, ev.num_nodes = 4, 3
    t = torch.zeros(2, 3, 4)
    with pytest.raises(ValueError, match="point_index"):
        ev.update(torch.zeros(2, 3, 4, 3), t)
    with pytest.raises(ValueError):
        ev.update(torch.zeros(2, 3, 5), torch.zeros(2, 3, 5))
    with pytest.raises(ValueError):
        ev.update(torch.zeros(2, 3, 4), torch.zeros(2, 3, 1))
    with pytest.raises(ValueError, match="num_nodes"):
        ev.update(torch.zeros(2, 4, 4), torch.zeros(2, 4, 4))
    with pytest.raises(ValueError):
        ev.update(torch.zeros(4), torch.zeros(4))
    with pytest.raises(RuntimeError, match="HIP"):
        ev.update(t, t)
    with pytest.raises(ValueError, match="num_nodes"):
        ev.node_table = None
        ev.node_scores()


def _fake_series(values, P=2, train_last=5):
    """What node_percentile_thresholds reads of a WindowedSeries: the (L, N, F) series on a device
    (the CPU here: the function is one torch call), the training labels and P."""
    return types.SimpleNamespace(series=torch.as_tensor(values), P=P,
                                 labels={"train": np.arange(1, train_last + 1, dtype=np.int64)})


def test_percentile_rules_and_the_training_steps_only():
    from dstagnn_drought_amd import node_percentile_thresholds
    from dstagnn_drought_amd.loss import check_percentiles
    assert check_percentiles([20, 10, 5]) == (20.0, 10.0, 5.0) and check_percentiles((80, 95), "above") == (80.0, 95.0)
    rng = np.random.default_rng(0)
    s = rng.normal(0, 1, (12, 3, 2)).astype(np.float32)
    ws = _fake_series(s)  # t_end = 5 + 2 = 7
    for pct, direction, word in [([], "below", "between 1"), (list(range(90, 10, -10)), "below", "between 1"),
                                 ([0, 10], "above", "inside"), ([100.0], "below", "inside"), ([NAN], "below", "inside"),
                                 ([10, 20], "below", "strictly decreasing"), ([20, 20], "below", "strictly decreasing"),
                                 ([20, 10], "above", "strictly increasing"), ("x", "below", "percentiles"),
                                 ([20, 10], "down", "direction")]:
        with pytest.raises(ValueError, match=word):
            node_percentile_thresholds(ws, pct, direction=direction)
    with pytest.raises(TypeError):
        node_percentile_thresholds(s, [20, 10])
    with pytest.raises(ValueError):
        node_percentile_thresholds(ws, [20, 10], missing_value=0.1)
    thr = node_percentile_thresholds(ws, [50, 20, 10])
    assert thr.dtype == torch.float32 and thr.shape == (3, 3) and thr.is_contiguous()
    want = np.percentile(s[:7, :, -1].astype(np.float64), [50, 20, 10], axis=0)
    assert np.allclose(thr.numpy(), want, rtol=1e-6, atol=0)
    s2 = s.copy()
    s2[7:] += 100.0  # nothing at or beyond t_end enters
    assert torch.equal(node_percentile_thresholds(_fake_series(s2), [50, 20, 10]), thr)
    # a marker: those elements are not observed; a node never observed in training is excluded
    s3 = s.copy()
    s3[:7, 1, :] = -9999.0
    s3[2, 0, -1] = -9999.0
    got = node_percentile_thresholds(_fake_series(s3), [50, 20], missing_value=-9999.0).numpy()
    assert np.isnan(got[:, 1]).all() and not np.isnan(got[:, [0, 2]]).any()
    obs = np.delete(s[:7, 0, -1].astype(np.float64), 2)
    assert np.allclose(got[:, 0], np.percentile(obs, [50, 20]), rtol=1e-6, atol=0)
    s4 = np.where(s3 == -9999.0, np.float32(NAN), s3)
    assert np.array_equal(node_percentile_thresholds(_fake_series(s4), [50, 20], missing_value=NAN).numpy(), got,
                          equal_nan=True)
    up = node_percentile_thresholds(ws, [80, 90], direction="above").numpy()
    assert (np.diff(up, axis=0) >= 0).all()


def test_event_options_key_keyword_and_flag(monkeypatch):
    from dstagnn_drought_amd import train as TR
    cp = configparser.ConfigParser()
    cp.read_string("[Training]\n")
    assert TR.event_options(cp["Training"]) == (None, None, "below")
    cp.read_string("[Training]\nevent_thresholds = -1.0, -1.5, -2.0\n")
    assert TR.event_options(cp["Training"]) == ((-1.0, -1.5, -2.0), None, "below")
    cp.read_string("[Training]\nevent_percentiles = 20, 10, 5\n")
    with pytest.raises(ValueError, match="give one"):
        TR.event_options(cp["Training"])
    cp = configparser.ConfigParser()
    cp.read_string("[Training]\nevent_percentiles = 80, 90\nevent_direction = Above\n")
    assert TR.event_options(cp["Training"]) == (None, (80.0, 90.0), "above")
    for keys in ("event_direction = sideways\n", "event_thresholds = a, b\n", "event_thresholds = \n",
                 "event_thresholds = -2, -1\n", "event_thresholds = 1, 2\n", "event_percentiles = 5, 10\n",
                 "event_percentiles = 0, 10\nevent_direction = above\n", "event_thresholds = 0,-1,-2,-3,-4,-5,-6,-7\n",
                 "event_thresholds = -1, -inf\n"):
        cp = configparser.ConfigParser()
        cp.read_string("[Training]\n" + keys)
        with pytest.raises(ValueError):
            TR.event_options(cp["Training"])
    rp = inspect.signature(TR.run).parameters
    for k in ("event_thresholds", "event_percentiles", "event_direction"):
        assert rp[k].default is None and rp[k].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(TR.score_batches).parameters["events"].default is None

    seen = {}

    def fake_run(config_path, **kw):
        seen.update(kw, config_path=config_path)
    monkeypatch.setattr(TR, "run", fake_run)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    TR.main(["--config", "x.conf"])
    assert seen["event_thresholds"] is None and seen["event_percentiles"] is None and seen["event_direction"] is None
    TR.main(["--config", "x.conf", "--event-thresholds=-1.0,-1.5", "--event-direction", "below"])
    assert seen["event_thresholds"] == "-1.0,-1.5" and seen["event_direction"] == "below"
    TR.main(["--config", "x.conf", "--event-percentiles", "80,90", "--event-direction", "above"])
    assert seen["event_percentiles"] == "80,90" and seen["event_thresholds"] is None


def test_run_resolves_key_keyword_and_flag_alike_and_refuses_before_any_data(monkeypatch, tmp_path):
    """run() up to the point where the options are resolved: the key, the keyword and the flag's
    string give the same (thresholds, percentiles, direction, test_metrics); the keyword wins; either
    threshold option implies test_metrics; percentiles without stream_windows, both definitions at
    once, or a broken list: a ValueError before any data is read (the configuration names no data
    file at all)."""
    from dstagnn_drought_amd import train as TR

    class Stop(Exception):
        pass

    got = []

    def fake_input_options(tc):  # the first thing run() does after resolving the scoring options
        loc = inspect.currentframe().f_back.f_locals
        got.append((loc["event_thresholds"], loc["event_percentiles"], loc["event_direction"], loc["test_metrics"]))
        raise Stop
    monkeypatch.setattr(TR, "input_options", fake_input_options)

    def resolved(keys, **kw):
        conf = tmp_path / "c.conf"
        conf.write_text("[Data]\n[Training]\n" + keys)
        with pytest.raises(Stop):
            TR.run(str(conf), **kw)
        return got[-1]
    assert resolved("") == (None, None, "below", False)
    fixed = ((-1.0, -1.5, -2.0), None, "below", True)
    assert resolved("event_thresholds = -1.0, -1.5, -2.0\n") == fixed
    assert resolved("", event_thresholds=(-1.0, -1.5, -2.0)) == fixed
    assert resolved("", event_thresholds="-1.0,-1.5,-2.0") == fixed  # what the flag hands over
    assert resolved("event_thresholds = -3, -4\n", event_thresholds=[-1.0, -1.5, -2.0]) == fixed
    pct = (None, (80.0, 90.0), "above", True)
    on = "stream_windows = true\n"
    assert resolved(on + "event_percentiles = 80, 90\nevent_direction = above\n") == pct
    assert resolved("", stream_windows=True, event_percentiles=(80, 90), event_direction="above") == pct
    assert resolved("", stream_windows=True, event_percentiles="80,90", event_direction="above") == pct
    # a threshold keyword replaces the keys' definition, whichever kind it is
    assert resolved(on + "event_thresholds = 1, 2\nevent_direction = above\n", event_percentiles="80,90") == pct
    assert resolved("event_thresholds = 1, 2\n", event_direction="above") == ((1.0, 2.0), None, "above", True)

    def refused(keys, **kw):
        conf = tmp_path / "c.conf"
        conf.write_text("[Data]\n[Training]\n" + keys)
        n = len(got)
        with pytest.raises(ValueError) as ei:
            TR.run(str(conf), **kw)
        assert len(got) == n  # raised before the options after it were even read
        return str(ei.value)
    assert "stream_windows" in refused("event_percentiles = 20, 10\n")
    assert "stream_windows" in refused("", event_percentiles=(20, 10))
    assert "give one" in refused(on + "event_percentiles = 20, 10\nevent_thresholds = -1, -2\n")
    assert "give one" in refused(on, event_percentiles=(20, 10), event_thresholds=(-1, -2))
    assert "strictly" in refused("event_thresholds = -2, -1\n")
    assert "strictly" in refused("event_thresholds = -1, -2\n", event_direction="above")
    assert "direction" in refused("", event_thresholds=(-1, -2), event_direction="sideways")


def test_the_update_path_holds_no_host_synchronisation():
    """One launch per batch and no host sync: update() reads nothing back, and score_batches'
    events branch only calls update()."""
    from dstagnn_drought_amd import EventScores
    from dstagnn_drought_amd import train as TR
    src = inspect.getsource(EventScores.update)
    for word in (".item(", ".cpu(", ".tolist(", ".numpy(", "synchronize", ".any(", ".all("):
        assert word not in src, word
    assert src.count("events_update(") == 1
    src = inspect.getsource(TR.score_batches)
    assert "events.update(out, yb)" in src
    for word in (".item(", ".cpu(", "synchronize"):
        assert word not in src


def test_config_separates_different_definitions():
    from dstagnn_drought_amd import EventScores
    from dstagnn_drought_amd.loss import check_thresholds, mask_of

    def cfg(thr, direction="below", mv=None, nodes=None, P=4):
        ev = object.__new__(EventScores)
        ev._thr_host = check_thresholds(thr, direction)
        ev.P, ev.K, ev.direction, ev.num_nodes, ev._mask = P, ev._thr_host.shape[0], direction, nodes, mask_of(mv)
        return ev._config()
    assert cfg([-1.0, -2.0]) == cfg([-1.0, -2.0]) and cfg([-1.0], mv=NAN) == cfg([-1.0], mv=NAN)
    per_node = np.array([[-1.0, -1.0], [-2.0, -2.0]])
    distinct = [cfg([-1.0, -2.0]), cfg([-1.0, -2.5]), cfg([-1.0]), cfg([-1.0, -2.0], mv=NAN), cfg([-1.0, -2.0], mv=-9999.0),
                cfg([1.0, 2.0], "above"), cfg([-1.0, -2.0], nodes=2), cfg(per_node, nodes=2), cfg([-1.0, -2.0], P=5),
                cfg(np.array([[-1.0, -1.0], [-2.0, -2.5]]), nodes=2), cfg([-1.0, -2.0, -2.0 - 1e-6])]
    assert len(set(distinct)) == len(distinct)
    assert cfg([-1.0], "below") != cfg([-1.0], "above")  # the same bytes, the other direction


@pytest.mark.parametrize("direction", ["below", "above"])
@pytest.mark.parametrize("marker", [None, NAN, -9999.0])
@pytest.mark.parametrize("per_node", [False, True])
def test_the_vectorised_reference_agrees_with_the_triple_loop(direction, marker, per_node):
    B, N, P, K = 4, 5, 3, 3
    rng = np.random.default_rng(7)
    base = np.array([-1.0, -1.5, -2.0], dtype=np.float32) * (1 if direction == "below" else -1)
    thr = base
    if per_node:
        thr = base[:, None] + np.linspace(-0.2, 0.2, N, dtype=np.float32)[None, :]
        thr[1, 2] = thr[0, 2]   # a tied column
        thr[:, 3] = NAN         # an excluded node
    target, pred = ER.draw(rng, thr, (B, N, P)), ER.draw(rng, thr, (B, N, P))
    pred[rng.random(pred.shape) < 0.1] = NAN
    pred[0, 0, 0], pred[1, 0, 1] = np.inf, -np.inf
    if marker is not None:
        target[rng.random(target.shape) < 0.15] = marker
    got, want = ER.counts(pred, target, thr, direction, marker), ER.counts_naive(pred, target, thr, direction, marker)
    quads = ER.two_by_two(pred, target, thr, direction, marker)
    for k in ("horizon", "node"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
        assert np.array_equal(got[k][:, 0], got[k][:, 1] + got[k][:, 2:].sum(1))
        assert got[k][:, 1].sum() > 0 and got[k][:, 0].sum() > 0
        # the directly counted 2 x 2 tables are the confusion matrix cut at each class (the nesting)
        M = got[k][:, 2:].reshape(-1, K + 1, K + 1)
        for j in range(K):
            cut = np.stack([M[:, j + 1:, j + 1:].sum((1, 2)), M[:, :j + 1, j + 1:].sum((1, 2)),
                            M[:, j + 1:, :j + 1].sum((1, 2)), M[:, :j + 1, :j + 1].sum((1, 2))], -1)
            assert np.array_equal(cut, quads[k][:, j]), (k, j)
    assert got["horizon"].sum(0).tolist() == got["node"].sum(0).tolist()
    if per_node:
        assert not got["node"][3].any() and ER.excluded_nodes(thr, N).tolist() == [False, False, False, True, False]
    # ... and the library's arithmetic agrees with the reference's on these tables
    from dstagnn_drought_amd import EventScores
    mine, ref = EventScores.scores_of_table(got["horizon"]), ER.scores(got["horizon"], quads["horizon"])
    assert sorted(mine) == sorted(ref)
    for key, v in ref.items():
        assert mine[key].shape == v.shape, key
        assert np.allclose(mine[key], v, rtol=1e-12, atol=0, equal_nan=True), key


def test_the_grid_sits_on_both_sides_of_every_threshold():
    thr = np.array([-1.0, -1.5, -2.0], dtype=np.float32)
    g = ER.grid(thr)
    assert g.dtype == np.float32 and len(g) == 11 and len(set(g.tolist())) == 11
    for t in thr:
        assert t in g and (g < t).any() and (g > t).any()
        assert np.nextafter(t, np.float32(np.inf)) in g and np.nextafter(t, np.float32(-np.inf)) in g
    assert g.min() < thr.min() - 0.5 and g.max() > thr.max() + 0.5
    assert sorted(set(ER.classes(g[None, None, :], thr, "below").ravel().tolist())) == [0, 1, 2, 3]
