"""CPU: the surface of the quantile forecasts that needs no GPU: the level rule (Python and C-ABI),
the driver's ``quantiles`` option and its conflict with ``loss_function``, ``point_index`` and its
tie rule, the C-ABI argument checks (before anything touches the device), the model switch's keys
and shapes (and the untouched point model), the arithmetic from a table of sums to the scores, and
that nothing falls back to the CPU."""
import configparser
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

E_SHAPE, E_ARG, E_SPACE = 10001, 10002, 10003
MASK_NONE, MASK_NEQ, MASK_NAN = 0, 1, 2
MAXQ = 16

BAD_LEVELS = {"empty": (), "17 levels": tuple((i + 1) / 18.0 for i in range(17)), "unsorted": (0.5, 0.1),
              "duplicate": (0.1, 0.5, 0.5), "zero": (0.0, 0.5), "one": (0.5, 1.0), "nan": (0.1, float("nan")),
              "negative": (-0.1, 0.5)}
# the words of the rule each message names
RULE = {"empty": "between 1 and 16", "17 levels": "between 1 and 16", "unsorted": "strictly increasing",
        "duplicate": "strictly increasing", "zero": "inside (0, 1)", "one": "inside (0, 1)", "nan": "inside (0, 1)",
        "negative": "inside (0, 1)"}


@pytest.fixture(autouse=True)
def _no_arpack_draws(monkeypatch):
    """As tests/test_multifeature_cpu.py: a model built here must not move ARPACK's generator."""
    import scipy.sparse.linalg as sla

    def eigs(A, k=1, which="LR", **kw):
        ev = np.linalg.eigvals(np.asarray(A))
        return ev[np.argsort(-ev.real)[:k]], None
    monkeypatch.setattr(sla, "eigs", eigs)


# ---------------------------------------------------------------------------------------------
# levels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(BAD_LEVELS))
def test_level_rule_in_python(case):
    from dstagnn_drought_amd import QuantileLoss, QuantileMetrics
    from dstagnn_drought_amd.loss import check_quantiles
    import re
    for make in (check_quantiles, QuantileLoss, lambda q: QuantileMetrics(4, q, device="cpu")):
        with pytest.raises(ValueError, match=re.escape(RULE[case])):
            make(BAD_LEVELS[case])


def test_levels_kept_and_point_index():
    from dstagnn_drought_amd import QuantileLoss
    from dstagnn_drought_amd.loss import check_quantiles, point_index_of
    assert check_quantiles([0.1, 0.5, 0.9]) == (0.1, 0.5, 0.9)
    assert check_quantiles(tuple((i + 1) / 17.0 for i in range(16)))  # 16 are allowed
    assert point_index_of((0.1, 0.5, 0.9)) == 1
    assert point_index_of((0.05,)) == 0
    assert point_index_of((0.1, 0.2, 0.3)) == 2
    assert point_index_of((0.25, 0.75)) == 0          # an exact tie goes to the lower index
    assert point_index_of((0.125, 0.375, 0.625, 0.875)) == 1
    assert point_index_of((0.6, 0.7)) == 0
    crit = QuantileLoss((0.1, 0.5, 0.9), null_val=float("nan"))
    assert crit.quantiles == (0.1, 0.5, 0.9) and crit.point_index == 1 and isinstance(crit, torch.nn.Module)
    assert not list(crit.parameters()) and not list(crit.buffers())


def test_quantile_options_parsing():
    from dstagnn_drought_amd import train as TR
    cp = configparser.ConfigParser()
    cp.read_string("[Training]\n")
    assert TR.quantile_options(cp["Training"]) is None
    cp.read_string("[Training]\nquantiles = 0.1, 0.5, 0.9\n")
    assert TR.quantile_options(cp["Training"]) == (0.1, 0.5, 0.9)
    cp.read_string("[Training]\nquantiles = 0.5\n")
    assert TR.quantile_options(cp["Training"]) == (0.5,)
    for bad in ("0.9, 0.1", "", "0.5, 0.5", "0, 0.5", "a, b", "1.0"):
        cp.read_string(f"[Training]\nquantiles = {bad}\n")
        with pytest.raises(ValueError):
            TR.quantile_options(cp["Training"])
    assert TR.parse_quantiles("0.1,0.5,0.9") == (0.1, 0.5, 0.9)
    rp = inspect.signature(TR.run).parameters
    assert rp["quantiles"].default is None and rp["quantiles"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(TR.predict_and_save_results_mstgcn).parameters["quantiles"].default is None


def test_flag_reaches_run(monkeypatch):
    from dstagnn_drought_amd import train as TR
    seen = {}
    monkeypatch.setattr(TR, "run", lambda config_path, **kw: seen.update(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    TR.main(["--config", "x.conf"])
    assert seen["quantiles"] is None
    TR.main(["--config", "x.conf", "--quantiles", "0.1,0.5,0.9"])
    assert seen["quantiles"] == "0.1,0.5,0.9"


def test_loss_function_conflicts_with_quantiles(tmp_path):
    from dstagnn_drought_amd import train as TR
    from dstagnn_drought_amd import QuantileLoss
    for name in ("mae", "smooth_l1", "masked_mae", "huber"):
        with pytest.raises(ValueError, match="pinball"):
            TR.make_criterion(name, None, quantiles=(0.1, 0.9))
    with pytest.raises(ValueError, match="quantiles"):
        TR.make_criterion("pinball", None)
    for name in (None, "pinball"):
        crit = TR.make_criterion(name, -9999.0, quantiles=(0.1, 0.9))
        assert isinstance(crit, QuantileLoss) and crit.quantiles == (0.1, 0.9) and crit.null_val == -9999.0
    assert isinstance(TR.make_criterion(), torch.nn.SmoothL1Loss)  # today's default, untouched
    # run() refuses the pair before it reads any data: key + key, key + keyword, keyword + key
    conf = tmp_path / "c.conf"
    conf.write_text("[Data]\n[Training]\nloss_function = mae\nquantiles = 0.1, 0.9\n")
    with pytest.raises(ValueError, match="pinball"):
        TR.run(str(conf))
    conf.write_text("[Data]\n[Training]\nloss_function = mae\n")
    with pytest.raises(ValueError, match="pinball"):
        TR.run(str(conf), quantiles=(0.1, 0.9))
    conf.write_text("[Data]\n[Training]\nquantiles = 0.1, 0.9\n")
    with pytest.raises(ValueError, match="pinball"):
        TR.run(str(conf), loss="huber")
    with pytest.raises(ValueError, match="strictly increasing"):
        TR.run(str(conf), quantiles="0.9,0.1")


# ---------------------------------------------------------------------------------------------
# C-ABI
# ---------------------------------------------------------------------------------------------
class Cfg(ctypes.Structure):  # dstagnn_pinball_cfg (include/dstagnn.h)
    _fields_ = [("mask_mode", ctypes.c_int), ("null_val", ctypes.c_float), ("num_quantiles", ctypes.c_int),
                ("tau", ctypes.c_float * MAXQ)]


def cfg_of(levels, mask=MASK_NONE, null=0.0, count=None):
    c = Cfg(mask, null, len(levels) if count is None else count)
    for i, v in enumerate(levels[:MAXQ]):
        c.tau[i] = v
    return c


def c_abi():
    from dstagnn_drought_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    i64, vp, cp = ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(Cfg)
    lib.dstagnn_last_error.restype = ctypes.c_char_p
    lib.dstagnn_pinball_scratch_bytes.restype = i64
    lib.dstagnn_pinball_scratch_bytes.argtypes = [i64, ctypes.c_int]
    lib.dstagnn_pinball_forward.argtypes = [cp, i64, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    lib.dstagnn_pinball_backward.argtypes = [cp, i64, vp, vp, vp, vp, vp, vp]
    lib.dstagnn_metrics_quantile_scratch_bytes.restype = i64
    lib.dstagnn_metrics_quantile_scratch_bytes.argtypes = [i64, i64, ctypes.c_int, ctypes.c_int]
    lib.dstagnn_metrics_accumulate_quantile.argtypes = [i64, i64, ctypes.c_int, cp, vp, vp, vp, vp, vp,
                                                        ctypes.c_size_t, vp]
    return lib


def _host_args():
    """Host memory standing in for the device buffers: every call below returns before it touches it."""
    buf = (ctypes.c_double * 64)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_header_declares_symbols_exported_ops_registered():
    import os
    import re
    from dstagnn_drought_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "dstagnn.h")) as f:
        src = f.read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(dstagnn_\w+)\s*\(", src, re.M))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("dstagnn_pinball_forward", "dstagnn_pinball_backward", "dstagnn_pinball_scratch_bytes",
              "dstagnn_metrics_accumulate_quantile", "dstagnn_metrics_quantile_scratch_bytes"):
        assert n in declared, f"include/dstagnn.h does not declare {n}"
        assert hasattr(lib, n), f"libdstagnn.so does not export {n}"
    assert "DSTAGNN_MAX_QUANTILES 16" in src and "dstagnn_pinball_cfg" in src
    ops = _lib.load()
    for n in ("pinball_fwd", "pinball_bwd", "metrics_update_quantile"):
        assert hasattr(ops, n), f"torch.ops.dstagnn.{n} missing"
    y, t = torch.zeros(2, 3, 4, 3), torch.zeros(2, 3, 4)
    with pytest.raises(RuntimeError):  # no CPU kernel behind the ops
        ops.pinball_fwd(y, t, [0.1, 0.5, 0.9], 0, 0.0)
    with pytest.raises(RuntimeError):
        ops.metrics_update_quantile(y, t, [0.1, 0.5, 0.9], 0, 0.0, torch.zeros(4, 11, dtype=torch.float64), None)


@pytest.mark.parametrize("case", sorted(BAD_LEVELS))
def test_level_rule_in_the_c_abi(case):
    lib = c_abi()
    buf, p = _host_args()
    levels = BAD_LEVELS[case]
    c = cfg_of(levels)
    assert lib.dstagnn_pinball_forward(ctypes.byref(c), 8, p, p, p, p, p, 1 << 20, None) == E_ARG
    msg = lib.dstagnn_last_error()
    assert (b"[1, 16]" in msg) if len(levels) in (0, 17) else (b"(0, 1)" in msg or b"increasing" in msg), msg
    assert lib.dstagnn_pinball_backward(ctypes.byref(c), 8, p, p, p, None, p, None) == E_ARG
    if 1 <= len(levels) <= MAXQ:  # (the metrics call files a Q outside [1, 16] under its shape limits)
        assert lib.dstagnn_metrics_accumulate_quantile(2, 8, 4, ctypes.byref(c), p, p, p, None, p, 1 << 20,
                                                       None) == E_ARG
    del buf


def test_pinball_argument_checks():
    lib = c_abi()
    buf, p = _host_args()
    c = cfg_of((0.1, 0.5, 0.9))
    ref = ctypes.byref(c)
    assert lib.dstagnn_pinball_forward(None, 8, p, p, p, p, p, 1 << 20, None) == E_ARG
    for m in (0, -1, (1 << 31) // 3 + 1, 1 << 40):
        assert lib.dstagnn_pinball_forward(ref, m, p, p, p, p, p, 1 << 20, None) == E_SHAPE
        assert lib.dstagnn_pinball_backward(ref, m, p, p, p, None, p, None) == E_SHAPE
        assert lib.dstagnn_pinball_scratch_bytes(m, 3) == 0
    for hole in range(5):  # y, target, loss, stat, scratch
        a = [p] * 5
        a[hole] = None
        assert lib.dstagnn_pinball_forward(ref, 8, *a, 1 << 20, None) == E_ARG
        assert b"pinball_forward" in lib.dstagnn_last_error()
    for hole in (0, 1, 2, 4):  # y, target, stat, dy (gout may be NULL)
        a = [p, p, p, None, p]
        a[hole] = None
        assert lib.dstagnn_pinball_backward(ref, 8, *a, None) == E_ARG
    for mask in (-1, 3):
        cm = cfg_of((0.5,), mask=mask)
        assert lib.dstagnn_pinball_forward(ctypes.byref(cm), 8, p, p, p, p, p, 1 << 20, None) == E_ARG
        assert b"mask" in lib.dstagnn_last_error()
    need = lib.dstagnn_pinball_scratch_bytes(65280, 3)
    tile = lib.dstagnn_loss_tile_elems()
    assert need == -(-65280 * 3 // tile) * 16  # {sum, count} per workgroup of one tile
    assert lib.dstagnn_pinball_scratch_bytes(1 << 26, 16) == 1024 * 16  # the grid cap
    assert lib.dstagnn_pinball_forward(ref, 65280, p, p, p, p, p, need - 1, None) == E_SPACE
    assert b"scratch" in lib.dstagnn_last_error()
    assert lib.dstagnn_pinball_scratch_bytes(8, 0) == 0 and lib.dstagnn_pinball_scratch_bytes(8, 17) == 0
    del buf


def test_metrics_quantile_argument_checks():
    lib = c_abi()
    buf, p = _host_args()
    c = cfg_of((0.1, 0.5, 0.9), MASK_NAN)
    ref = ctypes.byref(c)

    def call(B=2, N=8, P=4, cfg=ref, pred=p, target=p, htable=p, ntable=None, scratch=p, nbytes=1 << 20):
        return lib.dstagnn_metrics_accumulate_quantile(B, N, P, cfg, pred, target, htable, ntable, scratch, nbytes, None)
    for P in (0, 257, -3):
        assert call(P=P) == E_SHAPE and b"P" in lib.dstagnn_last_error()
        assert lib.dstagnn_metrics_quantile_scratch_bytes(2, 8, P, 3) == 0
    for Q in (0, 17, -1):
        cq = cfg_of((0.5,), count=Q)
        assert call(cfg=ctypes.byref(cq)) == E_SHAPE and b"Q" in lib.dstagnn_last_error()
        assert lib.dstagnn_metrics_quantile_scratch_bytes(2, 8, 4, Q) == 0
    for B, N, P in [(0, 8, 4), (2, 0, 4), (-1, 8, 4), (1 << 14, 1 << 14, 8), (1, (1 << 31) // 12 + 1, 4),
                    (1 << 40, 1 << 40, 1)]:
        assert call(B=B, N=N, P=P) == E_SHAPE
        assert lib.dstagnn_metrics_quantile_scratch_bytes(B, N, P, 3) == 0
    assert call(cfg=None) == E_ARG
    for hole in ("pred", "target", "htable", "scratch"):
        assert call(**{hole: None}) == E_ARG and b"metrics_accumulate_quantile" in lib.dstagnn_last_error()
    for mask in (-1, 3):
        cm = cfg_of((0.5,), mask=mask)
        assert call(cfg=ctypes.byref(cm)) == E_ARG
    need = lib.dstagnn_metrics_quantile_scratch_bytes(4, 170, 12, 3)
    assert need == -(-170 // (256 // 12)) * 11 * 12 * 8  # one (2 + 3 Q, P) partial per strip of 256 // P nodes
    assert call(B=4, N=170, P=12, nbytes=need - 1) == E_SPACE and b"scratch" in lib.dstagnn_last_error()
    # the shape is judged before the pointers, the pointers before the space
    assert call(P=300, pred=None, nbytes=0) == E_SHAPE
    assert call(pred=None, nbytes=0) == E_ARG
    del buf


# ---------------------------------------------------------------------------------------------
# the model switch
# ---------------------------------------------------------------------------------------------
def _model(seed=5, **kw):
    import dstagnn_drought_amd as D_
    N, T, K, h, D, dk, C, F, P = 10, 12, 3, 2, 16, 8, 8, 1, 12
    rs = np.random.RandomState(0)
    tmd, pa = np.eye(N), np.zeros((N, N))
    for i in range(N):
        tmd[i, rs.choice(N, 2, replace=False)] = 1.0
        pa[i, rs.choice(N, 4, replace=False)] = 1.0
    torch.manual_seed(seed)
    return D_.make_model("cpu", F, 2, F, K, C, C, 1, torch.from_numpy(tmd).float(), torch.from_numpy(pa).float(),
                         torch.from_numpy(pa).float(), P, T, N, D, dk, dk, h, **kw)


def test_quantile_model_keys_shapes_and_the_untouched_point_model():
    point, explicit_none = _model(), _model(quantiles=None)
    qm = _model(quantiles=(0.1, 0.5, 0.9))
    sp, sq = point.state_dict(), qm.state_dict()
    assert [k for k in sq if k != "quantile_levels"] == list(sp) and "quantile_levels" in sq  # one more key
    assert "quantile_levels" not in sp and not hasattr(point, "quantile_levels")
    assert point.quantiles is None and point.point_index is None
    assert sp["final_fc.weight"].shape == (12, 128) and sq["final_fc.weight"].shape == (36, 128)
    assert sq["final_fc.bias"].shape == (36,)
    assert sq["quantile_levels"].dtype == torch.float32
    assert torch.equal(sq["quantile_levels"], torch.tensor([0.1, 0.5, 0.9], dtype=torch.float32))
    assert qm.quantiles == (0.1, 0.5, 0.9) and qm.point_index == 1
    # every tensor but the head's last layer has the same shape
    assert all(sq[k].shape == sp[k].shape for k in sp if not k.startswith("final_fc."))
    # quantiles=None is the constructor of old: same keys, same init draws, bit for bit
    se = explicit_none.state_dict()
    assert list(se) == list(sp) and all(torch.equal(se[k], sp[k]) for k in sp)
    sig = inspect.signature(type(point).__init__).parameters
    assert sig["quantiles"].kind is inspect.Parameter.KEYWORD_ONLY and sig["quantiles"].default is None
    with pytest.raises(ValueError, match="strictly increasing"):
        _model(quantiles=(0.9, 0.1))


def test_checkpoints_do_not_cross():
    point, qa, qb = _model(), _model(quantiles=(0.1, 0.5, 0.9)), _model(quantiles=(0.05, 0.5, 0.95))
    qa2 = _model(seed=6, quantiles=(0.1, 0.5, 0.9))
    qa2.load_state_dict(qa.state_dict())  # the same levels load
    assert all(torch.equal(v, qa.state_dict()[k]) for k, v in qa2.state_dict().items())
    with pytest.raises(ValueError, match="quantile_levels") as e:
        qb.load_state_dict(qa.state_dict())
    assert "0.1" in str(e.value) and "0.05" in str(e.value)  # names both
    with pytest.raises(RuntimeError):  # strict loading: key set and final_fc shape differ
        qa.load_state_dict(point.state_dict())
    with pytest.raises(RuntimeError):
        point.load_state_dict(qa.state_dict())
    with pytest.raises(ValueError, match="quantile_levels"):  # another Q is other levels, too
        _model(quantiles=(0.1, 0.9)).load_state_dict(qa.state_dict())


# ---------------------------------------------------------------------------------------------
# scores from a table of sums
# ---------------------------------------------------------------------------------------------
def _table():
    """Q = 3; three rows: a plain one, one with crossings, an empty one."""
    #        count cross  pin0 hit0 Σy0   pin1 hit1 Σy1   pin2 hit2 Σy2
    return np.array([[8.0, 0.0, 2.0, 1.0, -8.0, 4.0, 4.0, 0.0, 1.0, 7.0, 16.0],
                     [4.0, 2.0, 1.0, 2.0, 2.0, 3.0, 2.0, 4.0, 2.0, 3.0, 3.0],
                     [0.0] * 11])


def test_scores_of_a_hand_filled_table():
    from dstagnn_drought_amd import QuantileMetrics
    s = QuantileMetrics.scores_of_table(_table())
    assert sorted(s) == ["count", "coverage", "crossing_rate", "interval_coverage", "interval_width", "mean_pinball",
                         "mean_quantile", "pinball"]
    assert all(v.dtype == np.float64 for v in s.values())
    assert s["count"].shape == (4,) and s["pinball"].shape == (4, 3) and s["interval_width"].shape == (4, 1)
    assert s["count"].tolist() == [8.0, 4.0, 0.0, 12.0]
    assert s["crossing_rate"][[0, 1, 3]].tolist() == [0.0, 0.5, 2.0 / 12.0]
    assert s["pinball"][0].tolist() == [0.25, 0.5, 0.125] and s["pinball"][3].tolist() == [0.25, 7.0 / 12.0, 0.25]
    assert s["mean_pinball"][0] == (0.25 + 0.5 + 0.125) / 3.0
    assert s["coverage"][0].tolist() == [0.125, 0.5, 0.875] and s["coverage"][1].tolist() == [0.5, 0.5, 0.75]
    assert s["mean_quantile"][0].tolist() == [-1.0, 0.0, 2.0]
    assert s["interval_width"][:2, 0].tolist() == [3.0, 0.25] and s["interval_coverage"][:2, 0].tolist() == [0.75, 0.25]
    assert s["interval_coverage"][3, 0] == 10.0 / 12.0 - 3.0 / 12.0
    for k, v in s.items():  # the empty row: every divisor is 0
        assert k == "count" or np.isnan(v[2]).all(), k
    n = QuantileMetrics.scores_of_table(_table(), overall=False)
    assert n["count"].shape == (3,) and n["coverage"].shape == (3, 3)
    one = QuantileMetrics.scores_of_table(np.array([[2.0, 0.0, 1.0, 1.0, 3.0]]))  # Q = 1: no interval
    assert one["interval_width"].shape == (2, 0) and one["pinball"][0, 0] == 0.5 and math.isclose(one["coverage"][1, 0], 0.5)
    even = QuantileMetrics.scores_of_table(np.zeros((1, 2 + 3 * 4)))
    assert even["interval_width"].shape == (2, 2)
    for bad in (np.zeros((3, 4)), np.zeros((3, 6)), np.zeros(11)):
        with pytest.raises(ValueError):
            QuantileMetrics.scores_of_table(bad)


# ---------------------------------------------------------------------------------------------
# no CPU path
# ---------------------------------------------------------------------------------------------
def test_no_cpu_fallback():
    from dstagnn_drought_amd import QuantileLoss, QuantileMetrics
    crit = QuantileLoss((0.1, 0.5, 0.9))
    y, t = torch.zeros(2, 3, 4, 3), torch.zeros(2, 3, 4)
    with pytest.raises(RuntimeError, match="HIP"):
        crit(y, t)
    with pytest.raises(RuntimeError, match="HIP"):
        QuantileMetrics(4, (0.1, 0.5, 0.9), device="cpu")
    # the shape rule comes first and needs no device: no broadcasting
    for yy, tt in ((torch.zeros(2, 3, 4, 2), t), (torch.zeros(2, 3, 4), t), (y, torch.zeros(2, 3, 1)),
                   (y, torch.zeros(3, 4)), (torch.zeros(2, 3, 4, 3), torch.zeros(2, 3, 4, 1))):
        with pytest.raises(ValueError, match="broadcasting"):
            crit(yy, tt)
    sig = inspect.signature(QuantileMetrics.__init__).parameters
    assert list(sig)[1:3] == ["num_for_predict", "quantiles"]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY and sig[k].default is None
               for k in ("missing_value", "num_nodes", "device"))
    with pytest.raises(ValueError):
        QuantileMetrics(257, (0.5,), device="cuda")
    with pytest.raises(ValueError):
        QuantileMetrics(4, (0.5,), device="cuda", num_nodes=0)
