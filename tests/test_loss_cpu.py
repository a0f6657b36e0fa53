"""CPU: the surface of the on-device criterion and test-set scores (csrc/loss.hip,
dstagnn_drought_amd/loss.py, the driver options in train.py) that needs no GPU: the ops are
registered, the C-ABI checks its arguments before anything touches the device, the driver's
defaults are today's, and nothing falls back to the CPU.  The numbers are tests/test_gpu_loss.py's.
"""
import configparser
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

E_SHAPE, E_ARG = 10001, 10002


class LossCfg(ctypes.Structure):  # dstagnn_loss_cfg (include/dstagnn.h)
    _fields_ = [("kind", ctypes.c_int), ("param", ctypes.c_float), ("mask_mode", ctypes.c_int),
                ("null_val", ctypes.c_float)]


def c_abi():
    from dstagnn_drought_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.dstagnn_last_error.restype = ctypes.c_char_p
    lib.dstagnn_loss_scratch_bytes.restype = ctypes.c_int64
    lib.dstagnn_loss_scratch_bytes.argtypes = [ctypes.c_int64]
    lib.dstagnn_metrics_scratch_bytes.restype = ctypes.c_int64
    lib.dstagnn_metrics_scratch_bytes.argtypes = [ctypes.c_int64, ctypes.c_int]
    vp = ctypes.c_void_p
    lib.dstagnn_loss_forward.argtypes = [ctypes.POINTER(LossCfg), ctypes.c_int64, vp, vp, vp, vp, vp, ctypes.c_size_t,
                                         vp]
    lib.dstagnn_loss_backward.argtypes = [ctypes.POINTER(LossCfg), ctypes.c_int64, vp, vp, vp, vp, vp, vp]
    lib.dstagnn_metrics_accumulate.argtypes = [ctypes.c_int64, ctypes.c_int, vp, vp, ctypes.c_float, vp, vp,
                                               ctypes.c_size_t, vp]
    return lib


def test_ops_registered():
    from dstagnn_drought_amd import _lib
    ops = _lib.load()
    for n in ("loss_fwd", "loss_bwd", "metrics_update"):
        assert hasattr(ops, n), f"torch.ops.dstagnn.{n} missing"
    with pytest.raises(RuntimeError):  # no CPU kernel behind the op either
        ops.loss_fwd(torch.zeros(4), torch.zeros(4), 0, 1.0, 0, 0.0)


def _host_args():
    """Host memory standing in for the device buffers: every call below must return before it
    touches any of them."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    return buf, p


@pytest.mark.parametrize("case", ["n0", "kind99", "null_y", "n2p31", "mask7", "neg_param", "nan_param", "null_cfg"])
def test_loss_forward_rejects_before_the_device(case):
    lib = c_abi()
    buf, p = _host_args()
    cfg, n, y = LossCfg(0, 1.0, 0, 0.0), 16, p
    if case == "n0":
        n = 0
    elif case == "n2p31":
        n = 1 << 31
    elif case == "kind99":
        cfg.kind = 99
    elif case == "mask7":
        cfg.mask_mode = 7
    elif case == "neg_param":
        cfg.param = -0.5
    elif case == "nan_param":
        cfg.param = float("nan")
    elif case == "null_y":
        y = None
    ref = None if case == "null_cfg" else ctypes.byref(cfg)
    assert lib.dstagnn_loss_forward(ref, n, y, p, p, p, p, 512, None) == E_ARG
    assert lib.dstagnn_last_error(), case
    assert lib.dstagnn_loss_backward(ref, n, y, p, p, None, p, None) == E_ARG
    del buf


def test_loss_forward_rejects_null_outputs():
    lib = c_abi()
    buf, p = _host_args()
    cfg = LossCfg(2, 0.0, 1, 0.0)
    assert lib.dstagnn_loss_forward(ctypes.byref(cfg), 16, p, p, None, p, p, 512, None) == E_ARG
    assert lib.dstagnn_loss_forward(ctypes.byref(cfg), 16, p, p, p, None, p, 512, None) == E_ARG
    assert lib.dstagnn_loss_backward(ctypes.byref(cfg), 16, p, p, None, None, p, None) == E_ARG
    assert b"loss_backward" in lib.dstagnn_last_error()
    del buf


@pytest.mark.parametrize("P", [257, 0, -3])
def test_metrics_rejects_horizon_count(P):
    lib = c_abi()
    buf, p = _host_args()
    assert lib.dstagnn_metrics_accumulate(8, P, p, p, 0.0, p, p, 512, None) == E_SHAPE
    assert b"P" in lib.dstagnn_last_error()
    assert lib.dstagnn_metrics_scratch_bytes(8, P) == 0
    del buf


def test_metrics_rejects_null_and_rows():
    lib = c_abi()
    buf, p = _host_args()
    assert lib.dstagnn_metrics_accumulate(8, 12, None, p, 0.0, p, p, 512, None) == E_ARG
    assert lib.dstagnn_metrics_accumulate(0, 12, p, p, 0.0, p, p, 512, None) == E_SHAPE
    assert lib.dstagnn_metrics_accumulate(1 << 28, 12, p, p, 0.0, p, p, 512, None) == E_SHAPE  # rows * P >= 2^31
    del buf


def test_scratch_sizes_follow_the_grid():
    lib = c_abi()
    tile = lib.dstagnn_loss_tile_elems()
    assert tile > 0 and tile % 4 == 0
    assert lib.dstagnn_loss_scratch_bytes(0) == 0
    assert lib.dstagnn_loss_scratch_bytes(1) == 16 == lib.dstagnn_loss_scratch_bytes(tile)
    assert lib.dstagnn_loss_scratch_bytes(tile + 1) == 32
    big = lib.dstagnn_loss_scratch_bytes((1 << 31) - 1)
    assert big % 16 == 0 and big // 16 < ((1 << 31) - 1) // tile  # the grid is capped
    assert lib.dstagnn_metrics_scratch_bytes(1, 1) == 32
    assert lib.dstagnn_metrics_scratch_bytes(1 << 20, 12) % (4 * 12 * 8) == 0


def test_loss_options_defaults_and_keys():
    from dstagnn_drought_amd import train as TR
    cp = configparser.ConfigParser()
    cp.read_string("[Training]\n")
    assert TR.loss_options(cp["Training"]) == (None, None, 1.0, 1.0)
    crit = TR.make_criterion()
    assert type(crit) is nn.SmoothL1Loss and crit.beta == 1.0 and crit.reduction == "mean"
    cp.read_string("[Training]\nloss_function = masked_mae\nmissing_value = nan\nsmooth_l1_beta = 0.25\n"
                   "huber_delta = 2\n")
    name, mv, beta, delta = TR.loss_options(cp["Training"])
    assert (name, beta, delta) == ("masked_mae", 0.25, 2.0) and mv != mv


def test_make_criterion_names():
    from dstagnn_drought_amd import HipLoss
    from dstagnn_drought_amd import train as TR
    with pytest.raises(ValueError):
        TR.make_criterion("masked_mae")
    with pytest.raises(ValueError):
        TR.make_criterion("masked_mse")
    with pytest.raises(ValueError):
        TR.make_criterion("l3")
    with pytest.raises(ValueError):
        HipLoss("smooth_l1", beta=-1.0)
    for name in ("smooth_l1", "huber", "mae", "mse"):  # any explicit name: the HIP criterion
        assert isinstance(TR.make_criterion(name), HipLoss)
    assert isinstance(TR.make_criterion("masked_mae", 0.0), HipLoss)
    masked_default = TR.make_criterion(None, float("nan"))
    assert isinstance(masked_default, HipLoss) and masked_default.kind == "smooth_l1"


def test_hiploss_has_no_cpu_path():
    from dstagnn_drought_amd import ForecastMetrics, HipLoss
    a, b = torch.zeros(2, 3, 4), torch.ones(2, 3, 4)
    with pytest.raises(RuntimeError, match="HIP"):
        HipLoss()(a, b)
    with pytest.raises(ValueError):
        HipLoss()(a, b[:, :1])  # no broadcasting
    with pytest.raises(RuntimeError, match="HIP"):
        ForecastMetrics(4, device="cpu")
    with pytest.raises(ValueError):
        ForecastMetrics(257, device="cuda")


def test_fit_and_run_take_a_criterion():
    import inspect
    from dstagnn_drought_amd import train as TR
    assert inspect.signature(TR.fit).parameters["criterion"].default is None
    rp = inspect.signature(TR.run).parameters
    assert rp["loss"].default is None and rp["missing_value"].default is None
    assert list(inspect.signature(TR.evaluate_on_test_mstgcn).parameters) == \
        ["net", "test_loader", "test_target_tensor", "sw", "epoch", "_mean", "_std"]


def test_refpaths_export_evaluate_on_test():
    script = ("import dstagnn_drought_amd.refpaths as r\nr.install()\n"
              "from lib.utils1 import evaluate_on_test_mstgcn\n"
              "from dstagnn_drought_amd.train import evaluate_on_test_mstgcn as e\n"
              "assert evaluate_on_test_mstgcn is e\nprint('ok')\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", script], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
