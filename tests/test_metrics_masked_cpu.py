"""CPU: the surface of the masked test-set scores (csrc/loss.hip metrics_masked_kernel's C-ABI,
dstagnn_drought_amd/loss.py ForecastMetrics(missing_value=, num_nodes=), the driver options of
train.py) that needs no GPU: the symbols are exported and the op registered, the C-ABI checks its
arguments before anything touches the device, nothing falls back to the CPU, the options resolve
the same way from the key, the keyword and the flag, and the arithmetic from a table of sums to
the scores is right, zero counts included.  The numbers are tests/test_gpu_metrics_masked.py's.
"""
import configparser
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

E_SHAPE, E_ARG, E_SPACE = 10001, 10002, 10003
MASK_NONE, MASK_NEQ, MASK_NAN = 0, 1, 2


def c_abi():
    from dstagnn_drought_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.dstagnn_last_error.restype = ctypes.c_char_p
    lib.dstagnn_metrics_masked_scratch_bytes.restype = ctypes.c_int64
    lib.dstagnn_metrics_masked_scratch_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int]
    vp = ctypes.c_void_p
    lib.dstagnn_metrics_accumulate_masked.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, vp, vp,
                                                      ctypes.c_int, ctypes.c_float, ctypes.c_float, vp, vp, vp,
                                                      ctypes.c_size_t, vp]
    return lib


def _host_args():
    """Host memory standing in for the device buffers: every call below must return before it
    touches any of them."""
    buf = (ctypes.c_double * 64)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_symbols_exported_and_op_registered():
    from dstagnn_drought_amd import _lib
    lib = c_abi()
    assert lib.dstagnn_metrics_masked_scratch_bytes and lib.dstagnn_metrics_accumulate_masked
    ops = _lib.load()
    assert hasattr(ops, "metrics_update_masked"), "torch.ops.dstagnn.metrics_update_masked missing"
    z = torch.zeros(2, 3, 4)
    with pytest.raises(RuntimeError):  # no CPU kernel behind the op either
        ops.metrics_update_masked(z, z, 0, 0.0, 0.0, torch.zeros(4, 8, dtype=torch.float64), None)


@pytest.mark.parametrize("P", [257, 0, -3])
def test_rejects_horizon_count(P):
    lib = c_abi()
    buf, p = _host_args()
    assert lib.dstagnn_metrics_accumulate_masked(2, 8, P, p, p, MASK_NONE, 0.0, 0.0, p, p, p, 1 << 20, None) == E_SHAPE
    assert b"P" in lib.dstagnn_last_error()
    assert lib.dstagnn_metrics_masked_scratch_bytes(2, 8, P) == 0
    del buf


@pytest.mark.parametrize("B,N,P", [(0, 8, 12), (-1, 8, 12), (2, 0, 12), (2, -5, 12), (1 << 14, 1 << 14, 8),
                                   (1 << 40, 1 << 40, 1), (1, (1 << 31) // 12 + 1, 12)])
def test_rejects_counts_and_the_index_range(B, N, P):
    lib = c_abi()
    buf, p = _host_args()
    assert lib.dstagnn_metrics_accumulate_masked(B, N, P, p, p, MASK_NONE, 0.0, 0.0, p, p, p, 1 << 20, None) == E_SHAPE
    assert b"metrics_accumulate_masked" in lib.dstagnn_last_error()
    assert lib.dstagnn_metrics_masked_scratch_bytes(B, N, P) == 0
    del buf


@pytest.mark.parametrize("case", ["pred", "target", "htable", "scratch", "mask-1", "mask3"])
def test_rejects_null_pointers_and_mask_modes(case):
    lib = c_abi()
    buf, p = _host_args()
    a = dict(pred=p, target=p, htable=p, scratch=p)
    mask = MASK_NEQ
    if case.startswith("mask"):
        mask = int(case[4:])
    else:
        a[case] = None
    rc = lib.dstagnn_metrics_accumulate_masked(2, 8, 12, a["pred"], a["target"], mask, 0.0, 0.0, a["htable"], p,
                                               a["scratch"], 1 << 20, None)
    assert rc == E_ARG
    assert b"metrics_accumulate_masked" in lib.dstagnn_last_error()
    del buf


def test_rejects_small_scratch_and_a_shape_error_comes_first():
    lib = c_abi()
    buf, p = _host_args()
    need = lib.dstagnn_metrics_masked_scratch_bytes(2, 170, 12)
    assert need > 0
    assert lib.dstagnn_metrics_accumulate_masked(2, 170, 12, p, p, MASK_NAN, 0.0, 0.0, p, None, p, need - 1,
                                                 None) == E_SPACE
    assert b"scratch" in lib.dstagnn_last_error()
    # the shape is judged before the pointers, the pointers before the space
    assert lib.dstagnn_metrics_accumulate_masked(2, 170, 300, None, p, 9, 0.0, 0.0, p, None, p, 0, None) == E_SHAPE
    assert lib.dstagnn_metrics_accumulate_masked(2, 170, 12, None, p, MASK_NAN, 0.0, 0.0, p, None, p, 0, None) == E_ARG
    del buf


def test_scratch_follows_the_grid():
    lib = c_abi()
    sb = lib.dstagnn_metrics_masked_scratch_bytes
    for B, N, P in [(1, 1, 1), (5, 101, 3), (4, 170, 12), (3, 7, 19), (3, 23, 100), (2, 9, 129), (2, 5, 256),
                    (6, 2200, 12), (32, 4096, 12)]:
        got = sb(B, N, P)
        assert got > 0 and got % (8 * P * 8) == 0, (B, N, P, got)
        tn = 256 // P
        assert got // (8 * P * 8) == -(-N // tn), (B, N, P, got)  # one partial per strip of 256 // P nodes
    assert sb(32, 4096, 12) // (8 * 12 * 8) == 196  # not capped
    assert sb(1, 4096, 12) == sb(32, 4096, 12)      # B only deepens a thread's walk


def test_masked_metrics_have_no_cpu_path():
    from dstagnn_drought_amd import ForecastMetrics
    for kw in (dict(missing_value=float("nan")), dict(missing_value=-9999.0), dict(num_nodes=7),
               dict(missing_value=0.0, num_nodes=7)):
        with pytest.raises(RuntimeError, match="HIP"):
            ForecastMetrics(4, device="cpu", **kw)
    with pytest.raises(ValueError):
        ForecastMetrics(257, device="cuda", missing_value=0.0)
    with pytest.raises(ValueError):
        ForecastMetrics(4, device="cuda", num_nodes=0)
    sig = inspect.signature(ForecastMetrics.__init__).parameters
    assert sig["missing_value"].kind is inspect.Parameter.KEYWORD_ONLY and sig["missing_value"].default is None
    assert sig["num_nodes"].kind is inspect.Parameter.KEYWORD_ONLY and sig["num_nodes"].default is None


def test_scoring_options_key_keyword_and_flag(monkeypatch, tmp_path):
    from dstagnn_drought_amd import train as TR
    cp = configparser.ConfigParser()
    cp.read_string("[Training]\n")
    assert TR.scoring_options(cp["Training"]) == (False, False)
    cp.read_string("[Training]\ntest_metrics = true\n")
    assert TR.scoring_options(cp["Training"]) == (True, False)
    cp.read_string("[Training]\ntest_metrics = false\nnode_scores = yes\n")
    assert TR.scoring_options(cp["Training"]) == (False, True)
    rp = inspect.signature(TR.run).parameters
    assert rp["test_metrics"].default is None and rp["node_scores"].default is None
    assert rp["test_metrics"].kind is inspect.Parameter.KEYWORD_ONLY

    # the flag reaches run() as the keyword; absent, run() gets None and reads the key
    seen = {}

    def fake_run(config_path, **kw):
        seen.update(kw, config_path=config_path)
    monkeypatch.setattr(TR, "run", fake_run)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    TR.main(["--config", "x.conf"])
    assert seen["test_metrics"] is None and seen["node_scores"] is None
    TR.main(["--config", "x.conf", "--test-metrics"])
    assert seen["test_metrics"] is True and seen["node_scores"] is None
    TR.main(["--config", "x.conf", "--node-scores"])
    assert seen["test_metrics"] is None and seen["node_scores"] is True


def test_run_resolves_key_and_keyword_alike(monkeypatch, tmp_path):
    """run() up to the point where the options are resolved: the [Training] key and the keyword
    give the same (test_metrics, node_scores); the keyword wins over the key; node_scores implies
    test_metrics."""
    from dstagnn_drought_amd import train as TR

    class Stop(Exception):
        pass

    got = []

    def fake_input_options(tc):  # the first thing run() does after resolving the scoring options
        frame = inspect.currentframe().f_back
        got.append((frame.f_locals["test_metrics"], frame.f_locals["node_scores"]))
        raise Stop
    monkeypatch.setattr(TR, "input_options", fake_input_options)

    def resolved(keys, **kw):
        conf = tmp_path / "c.conf"
        conf.write_text("[Data]\n[Training]\n" + keys)
        with pytest.raises(Stop):
            TR.run(str(conf), **kw)
        return got[-1]
    assert resolved("") == (False, False)
    assert resolved("test_metrics = true\n") == (True, False) == resolved("", test_metrics=True)
    assert resolved("node_scores = true\n") == (True, True) == resolved("", node_scores=True)
    both = "test_metrics = true\nnode_scores = true\n"
    assert resolved(both) == (True, True) and resolved(both, test_metrics=False, node_scores=False) == (False, False)
    assert resolved("test_metrics = false\n", test_metrics=True) == (True, False)


def _table():
    """Three rows of the eight sums: a plain one, one with no MAPE entry, an empty one."""
    #        count  Σe    Σ|e|  Σe²   Σ|e/t|  n_ape  Σt    Σt²
    return np.array([[4.0, -2.0, 6.0, 10.0, 1.5, 3.0, 8.0, 36.0],
                     [2.0, 1.0, 1.0, 0.5, 0.0, 0.0, 0.0, 0.0],
                     [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])


def test_list_of_a_hand_filled_table():
    from dstagnn_drought_amd import ForecastMetrics
    got = ForecastMetrics.list_of_table(_table())
    assert len(got) == 12 and all(isinstance(v, float) for v in got)
    assert got[0:3] == [1.5, math.sqrt(2.5), 50.0]
    assert got[3:6] == [0.5, 0.5, 0.0]                    # MAPE 0.0 where its own count is 0
    assert math.isnan(got[6]) and math.isnan(got[7]) and got[8] == 0.0  # no valid entry: NaN MAE / RMSE
    assert got[9:12] == [7.0 / 6.0, math.sqrt(10.5 / 6.0), 50.0]
    assert ForecastMetrics.list_of_table(np.zeros((2, 8)))[6:] == pytest.approx([float("nan")] * 2 + [0.0], nan_ok=True)


def test_scores_of_a_hand_filled_table():
    from dstagnn_drought_amd import ForecastMetrics
    s = ForecastMetrics.scores_of_table(_table())
    assert sorted(s) == ["bias", "count", "mae", "mape", "nse", "rmse"]
    assert all(v.shape == (4,) and v.dtype == np.float64 for v in s.values())
    assert s["count"].tolist() == [4.0, 2.0, 0.0, 6.0]
    assert s["mae"][:2].tolist() == [1.5, 0.5] and s["mae"][3] == 7.0 / 6.0
    assert s["rmse"][0] == math.sqrt(2.5) and s["rmse"][3] == math.sqrt(10.5 / 6.0)
    assert s["bias"][[0, 1, 3]].tolist() == [-0.5, 0.5, -1.0 / 6.0]
    assert s["mape"][0] == 50.0 and math.isnan(s["mape"][1]) and s["mape"][3] == 50.0
    # NSE: 1 - Σe² / (Σt² - (Σt)² / count); row 0: 1 - 10 / (36 - 16) = 0.5; row 1: zero variance
    assert s["nse"][0] == 0.5 and math.isnan(s["nse"][1])
    assert s["nse"][3] == 1.0 - 10.5 / (36.0 - 64.0 / 6.0)
    for k in s:  # the empty row: every divisor is 0
        assert math.isnan(s[k][2]) or k == "count", k
    n = ForecastMetrics.scores_of_table(_table(), overall=False)
    assert all(v.shape == (3,) for v in n.values()) and n["mae"].tolist()[:2] == [1.5, 0.5]


def test_scores_of_the_unmasked_table():
    from dstagnn_drought_amd import ForecastMetrics
    tab = np.array([[6.0, 10.0, 1.5, 3.0], [1.0, 0.5, 0.0, 0.0]])  # Σ|e|, Σe², Σ|e/t|, n_ape
    s = ForecastMetrics.scores_of_table(tab, rows=4)
    assert sorted(s) == ["count", "mae", "mape", "rmse"]  # what four columns allow
    assert s["count"].tolist() == [4.0, 4.0, 8.0]
    assert s["mae"].tolist() == [1.5, 0.25, 7.0 / 8.0] and s["rmse"][0] == math.sqrt(2.5)
    assert s["mape"][0] == 50.0 and math.isnan(s["mape"][1])
    z = ForecastMetrics.scores_of_table(tab, rows=0)
    assert np.isnan(z["mae"]).all()
    with pytest.raises(ValueError):
        ForecastMetrics.scores_of_table(np.zeros((3, 5)))


def test_driver_signatures():
    from dstagnn_drought_amd import train as TR
    ps = inspect.signature(TR.predict_and_save_results_mstgcn).parameters
    assert ps["missing_value"].default is None
    em = inspect.signature(TR.evaluate_on_test_masked).parameters
    assert em["missing_value"].default is None and em["per_node"].default is False
    assert list(em)[:5] == ["net", "test_loader", "test_target_tensor", "sw", "epoch"]
