"""CPU: the surface of the baseline skill scores (csrc/loss.hip skill_kernel and csrc/windows.hip
climatology_kernel behind their C-ABI, dstagnn_drought_amd/loss.py BaselineSkill, the driver options
of train.py) that needs no GPU: the symbols are exported and the ops registered, the C-ABI checks
every argument before anything touches the device, nothing falls back to the CPU, the options
resolve the same way from the key, the keyword and the flag, the ValueErrors fire, the arithmetic
from a table of sums to the scores is right (zero counts included), the update path holds no host
synchronisation, and the numpy reference of tests/test_gpu_skill.py agrees with a naive triple loop.
"""
import configparser
import ctypes
import inspect
import math
import types

import numpy as np
import pytest
import torch

import skill_ref as SR

E_SHAPE, E_ARG, E_SPACE = 10001, 10002, 10003
MASK_NONE, MASK_NEQ, MASK_NAN = 0, 1, 2
NAN = float("nan")
I64, I32, VP = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p


def c_abi():
    from dstagnn_drought_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.dstagnn_last_error.restype = ctypes.c_char_p
    lib.dstagnn_skill_scratch_bytes.restype = I64
    lib.dstagnn_skill_scratch_bytes.argtypes = [I64, I64, I32]
    lib.dstagnn_climatology.argtypes = [I32, VP, I64, I64, I64, I64, I64, I32, ctypes.c_double, VP, VP, VP]
    lib.dstagnn_skill_accumulate.argtypes = [I64, I64, I32, VP, VP, I32, ctypes.c_float, I32, VP, I64, I64, I32,
                                             ctypes.c_double, VP, VP, VP, I64, VP, VP, VP, ctypes.c_size_t, VP]
    return lib


def _host_args():
    """Host memory standing in for the device buffers: every call below must return before it
    touches any of them."""
    buf = (ctypes.c_double * 64)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _skill(lib, p, B=2, N=8, P=12, L=100, F=1, period=12, mask=MASK_NONE, src_masked=0, src_null=0.0,
           scratch_bytes=1 << 20, **ptr):
    a = dict(pred=p, target=p, src=p, pos=p, clim=p, cnt=p, htable=p, ntable=p, scratch=p)
    a.update(ptr)
    return lib.dstagnn_skill_accumulate(B, N, P, a["pred"], a["target"], mask, 0.0, 0, a["src"], L, F, src_masked,
                                        src_null, a["pos"], a["clim"], a["cnt"], period, a["htable"], a["ntable"],
                                        a["scratch"], scratch_bytes, None)


def _clim(lib, p, L=100, N=8, F=1, period=12, t_end=60, masked=0, null=0.0, **ptr):
    a = dict(series=p, clim=p, cnt=p)
    a.update(ptr)
    return lib.dstagnn_climatology(0, a["series"], L, N, F, period, t_end, masked, null, a["clim"], a["cnt"], None)


def test_symbols_exported_ops_registered_and_no_cpu_kernel():
    from dstagnn_drought_amd import _lib
    import dstagnn_drought_amd as D
    lib = c_abi()
    assert lib.dstagnn_climatology and lib.dstagnn_skill_scratch_bytes and lib.dstagnn_skill_accumulate
    assert D.BaselineSkill is D.loss.BaselineSkill and "BaselineSkill" in D.__all__
    ops = _lib.load()
    assert hasattr(ops, "climatology") and hasattr(ops, "skill_update")
    with pytest.raises(RuntimeError):  # no CPU kernel behind either op
        ops.climatology(torch.zeros(20, 3, 1), 4, 10, False, 0.0)
    z = torch.zeros(2, 3, 4)
    with pytest.raises(RuntimeError):
        ops.skill_update(z, z, 0, 0.0, torch.zeros(20, 3, 1), False, 0.0, torch.zeros(2, dtype=torch.int64),
                         torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.int32),
                         torch.zeros(4, 13, dtype=torch.float64), None)


@pytest.mark.parametrize("kw", [dict(P=257), dict(P=0), dict(P=-3), dict(B=0), dict(B=-1), dict(N=0), dict(N=-5),
                                dict(L=0), dict(F=0), dict(F=-2), dict(B=1 << 14, N=1 << 14, P=8, L=1, period=1),
                                dict(B=1 << 40, N=1 << 40, P=1), dict(L=1 << 20, N=1 << 11, F=1),
                                dict(L=1 << 40, N=1 << 40, F=1 << 40), dict(L=1 << 12, N=1 << 9, F=1 << 10),
                                dict(L=1 << 15, N=1 << 15, period=1 << 16, F=1), dict(period=0), dict(period=-1),
                                dict(period=101)])
def test_skill_rejects_shapes_before_the_pointers(kw):
    lib = c_abi()
    buf, p = _host_args()
    assert _skill(lib, p, **kw) == E_SHAPE, kw
    assert b"skill_accumulate" in lib.dstagnn_last_error()
    assert _skill(lib, p, pred=None, mask=9, scratch_bytes=0, **kw) == E_SHAPE  # the shape is judged first
    del buf


def test_skill_scratch_is_zero_for_a_rejected_shape_and_follows_the_grid():
    lib = c_abi()
    sb = lib.dstagnn_skill_scratch_bytes
    for B, N, P in [(2, 8, 257), (2, 8, 0), (0, 8, 12), (2, 0, 12), (1 << 14, 1 << 14, 8)]:
        assert sb(B, N, P) == 0
    for B, N, P in [(1, 1, 1), (5, 101, 3), (4, 170, 12), (3, 7, 19), (2, 9, 129), (2, 5, 256), (6, 2200, 12)]:
        got = sb(B, N, P)
        assert got > 0 and got == -(-N // (256 // P)) * 13 * P * 8, (B, N, P, got)
    assert sb(6, 2200, 12) // (13 * 12 * 8) == 105


@pytest.mark.parametrize("case", ["pred", "target", "src", "pos", "clim", "cnt", "htable", "scratch", "mask-1",
                                  "mask3", "nan-null-unmasked"])
def test_skill_rejects_null_pointers_modes_and_a_nan_marker_without_the_mask(case):
    lib = c_abi()
    buf, p = _host_args()
    if case.startswith("mask"):
        rc = _skill(lib, p, mask=int(case[4:]))
    elif case == "nan-null-unmasked":
        rc = _skill(lib, p, src_masked=0, src_null=NAN)
    else:
        rc = _skill(lib, p, **{case: None})
    assert rc == E_ARG
    assert b"skill_accumulate" in lib.dstagnn_last_error()
    del buf


def test_skill_rejects_small_scratch_last():
    lib = c_abi()
    buf, p = _host_args()
    need = lib.dstagnn_skill_scratch_bytes(2, 170, 12)
    assert need > 0
    assert _skill(lib, p, N=170, ntable=None, scratch_bytes=need - 1) == E_SPACE
    assert b"scratch" in lib.dstagnn_last_error() and b"skill_accumulate" in lib.dstagnn_last_error()
    assert _skill(lib, p, N=170, pred=None, scratch_bytes=0) == E_ARG  # the pointers before the space
    del buf


@pytest.mark.parametrize("kw", [dict(L=0), dict(N=0), dict(F=0), dict(N=-3), dict(L=1 << 20, N=1 << 11),
                                dict(L=1 << 40, N=1 << 40, F=1 << 40), dict(L=1 << 15, N=1 << 15, period=1 << 16),
                                dict(period=0), dict(period=101), dict(period=-4), dict(t_end=0), dict(t_end=101),
                                dict(t_end=-1)])
def test_climatology_rejects_shapes_before_the_pointers(kw):
    lib = c_abi()
    buf, p = _host_args()
    assert _clim(lib, p, **kw) == E_SHAPE, kw
    assert b"climatology" in lib.dstagnn_last_error()
    assert _clim(lib, p, series=None, **kw) == E_SHAPE
    del buf


@pytest.mark.parametrize("case", ["series", "clim", "cnt", "nan-null-unmasked"])
def test_climatology_rejects_null_pointers_and_a_nan_marker_without_the_mask(case):
    lib = c_abi()
    buf, p = _host_args()
    rc = _clim(lib, p, masked=0, null=NAN) if case == "nan-null-unmasked" else _clim(lib, p, **{case: None})
    assert rc == E_ARG
    assert b"climatology" in lib.dstagnn_last_error()
    del buf


def _table():
    """Three rows of the 13 sums: a plain one, one whose baselines made no error, an empty one."""
    #         n_p  Σem²  Σep²  Σ|em| Σ|ep|  n_c  Σem²  Σec²  Σ|em| Σ|ec|  Σaf·ao Σaf²  Σao²
    return np.array([[4.0, 2.0, 8.0, 2.0, 5.0, 2.0, 1.0, 4.0, 1.0, 4.0, 3.0, 4.0, 9.0],
                     [2.0, 1.0, 0.0, 1.0, 0.0, 2.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 5.0],
                     [0.0] * 13])


def test_scores_of_a_hand_filled_table():
    from dstagnn_drought_amd import BaselineSkill
    s = BaselineSkill.scores_of_table(_table())
    names = ["count", "rmse", "mae", "model_rmse", "model_mae", "mse_skill", "mae_skill"]
    assert sorted(s) == sorted([f"{k}_{b}" for k in names for b in ("persistence", "climatology")] + ["acc"])
    assert all(v.shape == (4,) and v.dtype == np.float64 for v in s.values())
    assert s["count_persistence"].tolist() == [4.0, 2.0, 0.0, 6.0]
    assert s["count_climatology"].tolist() == [2.0, 2.0, 0.0, 4.0]
    # row 0, the formulas written out
    assert s["rmse_persistence"][0] == math.sqrt(8.0 / 4.0) and s["mae_persistence"][0] == 5.0 / 4.0
    assert s["model_rmse_persistence"][0] == math.sqrt(2.0 / 4.0) and s["model_mae_persistence"][0] == 2.0 / 4.0
    assert s["mse_skill_persistence"][0] == 1.0 - 2.0 / 8.0 and s["mae_skill_persistence"][0] == 1.0 - 2.0 / 5.0
    assert s["rmse_climatology"][0] == math.sqrt(4.0 / 2.0) and s["mae_climatology"][0] == 4.0 / 2.0
    assert s["model_rmse_climatology"][0] == math.sqrt(1.0 / 2.0) and s["model_mae_climatology"][0] == 1.0 / 2.0
    assert s["mse_skill_climatology"][0] == 1.0 - 1.0 / 4.0 and s["mae_skill_climatology"][0] == 1.0 - 1.0 / 4.0
    assert s["acc"][0] == 3.0 / math.sqrt(4.0 * 9.0)
    # row 1: a perfect baseline leaves the skill's divisor at 0 -> NaN; a zero anomaly variance -> NaN acc
    for k in ("mse_skill_persistence", "mae_skill_persistence", "mse_skill_climatology", "mae_skill_climatology", "acc"):
        assert math.isnan(s[k][1]), k
    assert s["rmse_persistence"][1] == 0.0 and s["model_rmse_persistence"][1] == math.sqrt(0.5)
    # the empty row: every divisor is 0
    for k in s:
        assert math.isnan(s[k][2]) or k.startswith("count_"), k
    # overall, from the column sums
    assert s["mse_skill_persistence"][3] == 1.0 - 3.0 / 8.0 and s["mae_skill_climatology"][3] == 1.0 - 2.0 / 4.0
    assert s["rmse_climatology"][3] == math.sqrt(4.0 / 4.0) and s["acc"][3] == 3.0 / math.sqrt(4.0 * 14.0)
    n = BaselineSkill.scores_of_table(_table(), overall=False)
    assert all(v.shape == (3,) for v in n.values()) and n["acc"][0] == 0.5
    for k, v in SR.scores(_table()).items():  # the reference's own arithmetic agrees
        assert np.array_equal(v, s[k], equal_nan=True), k
    with pytest.raises(ValueError):
        BaselineSkill.scores_of_table(np.zeros((3, 8)))


def test_skill_options_key_keyword_and_flag(monkeypatch):
    from dstagnn_drought_amd import train as TR
    cp = configparser.ConfigParser()
    cp.read_string("[Data]\n[Training]\n")
    assert TR.skill_options(cp["Training"], cp["Data"]) == (False, None)
    cp.read_string("[Data]\nperiod = 12\n[Training]\nbaseline_skill = true\n")
    assert TR.skill_options(cp["Training"], cp["Data"]) == (True, 12)
    assert TR.skill_options(cp["Training"]) == (True, None)
    cp.read_string("[Training]\nbaseline_skill = no\nclimatology_period = 288\n")
    assert TR.skill_options(cp["Training"], cp["Data"]) == (False, 288)  # the [Training] key wins over [Data] period
    cp.read_string("[Training]\nclimatology_period = weekly\n")
    with pytest.raises(ValueError):
        TR.skill_options(cp["Training"], cp["Data"])
    rp = inspect.signature(TR.run).parameters
    assert rp["baseline_skill"].default is None and rp["climatology_period"].default is None
    assert rp["baseline_skill"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(TR.score_batches).parameters["skill"].default is None

    seen = {}

    def fake_run(config_path, **kw):
        seen.update(kw, config_path=config_path)
    monkeypatch.setattr(TR, "run", fake_run)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    TR.main(["--config", "x.conf"])
    assert seen["baseline_skill"] is None and seen["climatology_period"] is None
    TR.main(["--config", "x.conf", "--baseline-skill", "--climatology-period", "7"])
    assert seen["baseline_skill"] is True and seen["climatology_period"] == 7


def test_run_resolves_key_and_keyword_alike_and_refuses_before_any_data(monkeypatch, tmp_path):
    """run() up to the point where the options are resolved: the key and the keyword give the same
    (baseline_skill, period, test_metrics); the keyword wins; baseline_skill implies test_metrics;
    without stream_windows, or without a usable period, a ValueError before any data is read (the
    configuration names no data file at all)."""
    from dstagnn_drought_amd import train as TR

    class Stop(Exception):
        pass

    got = []

    def fake_input_options(tc):  # the first thing run() does after resolving the scoring options
        loc = inspect.currentframe().f_back.f_locals
        got.append((loc["baseline_skill"], loc["climatology_period"], loc["test_metrics"]))
        raise Stop
    monkeypatch.setattr(TR, "input_options", fake_input_options)

    def resolved(data, keys, **kw):
        conf = tmp_path / "c.conf"
        conf.write_text("[Data]\n" + data + "[Training]\n" + keys)
        with pytest.raises(Stop):
            TR.run(str(conf), **kw)
        return got[-1]
    assert resolved("", "") == (False, None, False)
    on = "stream_windows = true\nbaseline_skill = true\n"
    assert resolved("period = 12\n", on) == (True, 12, True)
    assert resolved("period = 12\n", "", stream_windows=True, baseline_skill=True) == (True, 12, True)
    assert resolved("period = 12\n", on + "climatology_period = 7\n") == (True, 7, True)
    assert resolved("period = 12\n", on, climatology_period=5) == (True, 5, True)
    assert resolved("period = 12\n", on, baseline_skill=False) == (False, 12, False)

    def refused(data, keys, **kw):
        conf = tmp_path / "c.conf"
        conf.write_text("[Data]\n" + data + "[Training]\n" + keys)
        n = len(got)
        with pytest.raises(ValueError) as ei:
            TR.run(str(conf), **kw)
        assert len(got) == n  # raised before the options after it were even read
        return str(ei.value)
    assert "stream_windows" in refused("period = 12\n", "baseline_skill = true\n")
    assert "stream_windows" in refused("period = 12\n", "", baseline_skill=True)
    assert "period" in refused("", on)
    assert "period" in refused("period = 0\n", on)
    assert "period" in refused("period = 12\n", on, climatology_period=-3)


def _fake_series(L=40, N=3, F=1, P=4, device="cpu"):
    return types.SimpleNamespace(L=L, N=N, F=F, P=P, labels={"train": np.arange(4, 20, dtype=np.int64)},
                                 device=torch.device(device))


def test_baseline_skill_value_errors_and_no_cpu_path():
    from dstagnn_drought_amd import BaselineSkill
    for bad in (None, 0, -1, 41, 2.5, True, "x"):
        with pytest.raises(ValueError, match="period"):
            BaselineSkill(_fake_series(), bad)
    with pytest.raises(ValueError, match="num_nodes"):
        BaselineSkill(_fake_series(), 12, num_nodes=4)
    with pytest.raises(ValueError):
        BaselineSkill(_fake_series(), 12, missing_value=0.1)  # float32 does not hold it
    with pytest.raises(TypeError):
        BaselineSkill(np.zeros((40, 3, 1)), 12)
    with pytest.raises(RuntimeError, match="HIP"):  # a valid configuration on the CPU: no fallback
        BaselineSkill(_fake_series(), 12)
    sig = inspect.signature(BaselineSkill.__init__).parameters
    assert list(sig)[:3] == ["self", "series", "period"]
    for k in ("missing_value", "num_nodes"):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY and sig[k].default is None

    # update(): the shapes are judged before anything else
    sk = object.__new__(BaselineSkill)
    sk.P, sk.N, sk.num_nodes = 4, 3, None
    t = torch.zeros(2, 3, 4)
    with pytest.raises(ValueError, match="point_index"):
        sk.update(torch.zeros(2, 3, 4, 3), t, "test", slice(0, 2))
    with pytest.raises(ValueError):
        sk.update(torch.zeros(2, 3, 5), torch.zeros(2, 3, 5), "test", slice(0, 2))
    with pytest.raises(ValueError):
        sk.update(torch.zeros(2, 4, 4), torch.zeros(2, 4, 4), "test", slice(0, 2))
    with pytest.raises(RuntimeError, match="HIP"):
        sk.update(t, t, "test", slice(0, 2))


def test_the_update_path_holds_no_host_synchronisation():
    """One launch per batch and no host sync: neither update() nor what it calls for a slice or a
    device tensor reads a value back, and score_batches' skill branch only calls update()."""
    from dstagnn_drought_amd import BaselineSkill
    from dstagnn_drought_amd import train as TR
    for fn in (BaselineSkill.update, BaselineSkill._positions):
        src = inspect.getsource(fn)
        for word in (".item(", ".cpu(", ".tolist(", ".numpy(", "synchronize"):
            assert word not in src, (fn.__name__, word)
    assert inspect.getsource(BaselineSkill.update).count("skill_update(") == 1
    src = inspect.getsource(TR.score_batches)
    assert "skill.update(out, yb, y.name, slice(b, b + batch_size))" in src
    for word in (".item(", ".cpu(", "synchronize"):
        assert word not in src


def test_config_includes_the_period_and_the_mask():
    from dstagnn_drought_amd import BaselineSkill
    from dstagnn_drought_amd.loss import mask_of

    def cfg(period, mv):
        sk = object.__new__(BaselineSkill)
        sk.P, sk.N, sk.L, sk.period, sk.t_end, sk.num_nodes = 4, 3, 40, period, 24, None
        sk._mask = mask_of(mv)
        return sk._config()
    assert cfg(12, None) == cfg(12, None) and cfg(12, NAN) == cfg(12, NAN)
    assert len({cfg(12, None), cfg(7, None), cfg(12, NAN), cfg(12, -9999.0), cfg(12, 0.0)}) == 5


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("marker", [None, NAN, -9999.0])
def test_the_vectorised_reference_agrees_with_the_triple_loop(dtype, marker):
    L, N, F, P, period, t_end = 30, 3, 2, 3, 4, 18
    series = SR.gapped_series(L, N, F, dtype, marker, seed=5, period=period, t_end=t_end, lead=26)
    rng = np.random.default_rng(6)
    pos = np.array([20, 1, 0, 24, 27, 28, -2], dtype=np.int64)  # 28 + 3 > 30 and -2: outside the series
    B = len(pos)
    target = np.full((B, N, P), np.nan, dtype=np.float32)
    for b, l in enumerate(pos):
        if 0 <= l and l + P <= L:
            target[b] = series[l:l + P, :, -1].T.astype(np.float32)
    pred = (np.nan_to_num(target, nan=1.0) + rng.normal(0, 1, target.shape)).astype(np.float32)
    sums, mags = SR.skill_sums(pred, target, pos, series, period, t_end, marker, marker)
    naive = SR.skill_sums_naive(pred, target, pos, series, period, t_end, marker, marker)
    for k in ("horizon", "node"):
        assert sums[k].shape == naive[k].shape == mags[k].shape
        assert np.array_equal(sums[k][:, [0, 5]], naive[k][:, [0, 5]])  # the counts: exact
        assert np.all(np.abs(sums[k] - naive[k]) <= 1e-12 * np.maximum(mags[k], 1.0)), k
        assert sums[k][:, 0].sum() > 0 and sums[k][:, 5].sum() > 0
    if marker is not None:  # the gaps do what the GPU tests need them to do
        clim, cnt = SR.climatology(series, period, t_end, marker)
        assert (cnt[1, 1] == 0) and np.isnan(clim[1, 1]) and (cnt > 0).any()
        q, ok = SR.persistence(series, pos, marker)
        assert not ok[:4, 0].any() and ok[:, 1:].any()  # node 0: nothing observed before step 26
        assert sums["node"][0, 5] == 0                   # ... nor in training: no climatology either
    # the climatology is the plain per-phase mean
    clim, cnt = SR.climatology(series, period, t_end, marker)
    s = series[:t_end, :, -1].astype(np.float64)
    miss = SR.missing(series[:t_end, :, -1], marker)
    for ph in range(period):
        for n in range(N):
            vals = s[ph::period, n][~miss[ph::period, n]]
            assert cnt[ph, n] == len(vals)
            if len(vals):
                assert abs(clim[ph, n] - vals.mean()) <= 1e-12 * abs(vals.mean())
