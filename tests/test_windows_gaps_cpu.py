"""CPU: the host side of training on a series with gaps (dstagnn_drought_amd.windows /
.train): the [Training] keys ``input_fill`` / ``input_max_gap``, every argument error raised before
a device is looked for, the new keywords' defaults, the operator registration.  What runs on the
device is in tests/test_gpu_windows_gaps.py."""
import configparser
import inspect
import os

import numpy as np
import pytest
import torch

from dstagnn_drought_amd import train as TR
from dstagnn_drought_amd import windows as W

KW = dict(num_of_weeks=0, num_of_days=0, num_of_hours=1, num_for_predict=12, points_per_hour=12)


def _training(text):
    cp = configparser.ConfigParser()
    cp.read_string("[Training]\n" + text)
    return cp["Training"]


def test_input_options_defaults_and_parsing():
    assert TR.input_options(_training("batch_size = 4\n")) == (None, None)
    assert TR.input_options(_training("input_fill = none\n")) == (None, None)
    assert TR.input_options(_training("input_fill = mean\n")) == ("mean", None)
    assert TR.input_options(_training("input_fill = ffill\ninput_max_gap = 6\n")) == ("ffill", 6)
    assert TR.input_options(_training("input_fill = FFILL\n")) == ("ffill", None)
    with pytest.raises(ValueError, match="input_fill"):
        TR.input_options(_training("input_fill = linear\n"))
    # loss_options() keeps its four values: the new keys live in their own function
    assert TR.loss_options(_training("input_fill = mean\nmissing_value = nan\n"))[0] is None
    assert len(TR.loss_options(_training("input_fill = mean\n"))) == 4


def test_signatures_carry_the_new_keywords():
    for f in (W.WindowedSeries.__init__, W.WindowedSeries.from_file):
        p = inspect.signature(f).parameters
        assert p["missing_value"].default is None and p["fill"].default == "mean" and p["max_gap"].default is None
    p = inspect.signature(TR.run).parameters
    assert p["input_fill"].default is None and p["input_max_gap"].default is None
    assert p["input_fill"].kind is inspect.Parameter.KEYWORD_ONLY


@pytest.mark.parametrize("device", ["cpu", None])
def test_gap_arguments_are_checked_before_the_device(device):
    series = np.zeros((100, 3, 2), dtype=np.float32)

    def make(**kw):
        return W.WindowedSeries(series, device=device, **KW, **kw)

    with pytest.raises(ValueError, match="fill must be one of"):
        make(missing_value=float("nan"), fill="linear")
    with pytest.raises(ValueError, match="fill must be one of"):
        make(missing_value=-9999.0, fill=None)
    for bad in (0, -3, 2.0, "4", True):
        with pytest.raises(ValueError, match="max_gap"):
            make(missing_value=float("nan"), fill="ffill", max_gap=bad)
    with pytest.raises(ValueError, match="max_gap"):
        make(missing_value=float("nan"), fill="mean", max_gap=3)
    with pytest.raises(ValueError, match="max_gap"):
        make(missing_value=float("nan"), max_gap=3)  # fill defaults to 'mean'
    with pytest.raises(ValueError, match="float32"):
        make(missing_value=0.1)
    with pytest.raises(ValueError, match="float32"):
        make(missing_value=-9999.0 - 2.0 ** -20, fill="ffill")
    # accepted values get as far as the device question
    if device == "cpu" or not torch.cuda.is_available():
        for kw in (dict(missing_value=float("nan")), dict(missing_value=-9999.0, fill="ffill", max_gap=4),
                   dict(missing_value=np.float32(0.5), fill="ffill", max_gap=np.int64(2))):
            with pytest.raises(RuntimeError, match="HIP"):
                make(**kw)
        # without a missing value the other two are ignored, and the object is today's
        with pytest.raises(RuntimeError, match="HIP"):
            make(fill="anything", max_gap=-1)
        with pytest.raises(RuntimeError, match="HIP"):
            make()


def test_check_missing_options_values():
    assert W.check_missing_options(None, "anything", -1) == (None, None, None)
    mv, fill, gap = W.check_missing_options(float("nan"))
    assert mv != mv and fill == "mean" and gap is None
    assert W.check_missing_options(-9999, "ffill", 7) == (-9999.0, "ffill", 7)
    assert W.check_missing_options(float("inf"), "ffill") == (float("inf"), "ffill", None)


def _conf(tmp_path, training):
    path = os.path.join(str(tmp_path), "gaps.conf")
    with open(path, "w") as f:
        f.write("[Data]\ngraph_signal_matrix_filename = " + os.path.join(str(tmp_path), "absent.npz") + "\n"
                "num_for_predict = 12\npoints_per_hour = 12\n[Training]\nbatch_size = 4\nnum_of_hours = 1\n"
                "num_of_days = 0\nnum_of_weeks = 0\n" + training)
    return path


def test_run_refuses_a_fill_it_cannot_apply(tmp_path):
    """Both errors come before any file of the configuration is opened (absent.npz does not exist)."""
    quiet = dict(log=lambda *_: None, root=str(tmp_path))
    with pytest.raises(ValueError, match="missing value"):
        TR.run(_conf(tmp_path, ""), stream_windows=True, input_fill="mean", **quiet)
    with pytest.raises(ValueError, match="missing value"):
        TR.run(_conf(tmp_path, "input_fill = ffill\nstream_windows = true\n"), **quiet)
    with pytest.raises(ValueError, match="stream_windows"):
        TR.run(_conf(tmp_path, "missing_value = nan\n"), input_fill="ffill", **quiet)
    with pytest.raises(ValueError, match="stream_windows"):
        TR.run(_conf(tmp_path, "input_fill = mean\n"), missing_value=-9999.0, stream_windows=False, **quiet)


def test_command_line_has_the_two_options(tmp_path):
    with pytest.raises(ValueError, match="missing value"):
        TR.main(["--config", _conf(tmp_path, ""), "--stream-windows", "--input-fill", "ffill", "--input-max-gap", "3",
                 "--out-root", str(tmp_path)])
    with pytest.raises(SystemExit):
        TR.main(["--config", _conf(tmp_path, ""), "--input-fill", "linear"])


def test_gap_ops_registered_and_refuse_cpu_tensors():
    from dstagnn_drought_amd import _lib
    ops = _lib.load()
    for n in ("window_stats_masked", "window_fill_forward", "window_gather_masked", "window_fill_chunk",
              "window_fill_cols"):
        assert hasattr(ops, n), f"torch.ops.dstagnn.{n} missing"
    assert ops.window_fill_chunk() >= 2 and ops.window_fill_cols() >= 2
    series = torch.zeros(40, 3, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError):
        ops.window_stats_masked(series, torch.ones(40, dtype=torch.int32), float("nan"))
    with pytest.raises(RuntimeError):
        ops.window_fill_forward(series, float("nan"), 0)
    with pytest.raises(RuntimeError):
        ops.window_gather_masked(series, series, torch.zeros(12, dtype=torch.int32), torch.arange(12, 20),
                                 torch.arange(4), torch.zeros(2, dtype=torch.float64),
                                 torch.ones(2, dtype=torch.float64), 12, float("nan"))


def test_c_abi_argument_checks_come_before_any_launch():
    """Null pointers DSTAGNN_E_ARG, shapes DSTAGNN_E_SHAPE, a short scratch DSTAGNN_E_SPACE, each with a
    last-error text: all returned before the device is touched (the buffers here are host memory
    that is never dereferenced)."""
    import ctypes
    from dstagnn_drought_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.dstagnn_last_error.restype = ctypes.c_char_p
    E_SHAPE, E_ARG, E_SPACE = 10001, 10002, 10003
    i64, i32, dbl, vp, sz = ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
    for f in (lib.dstagnn_window_stats_masked_scratch_bytes, lib.dstagnn_window_fill_scratch_bytes):
        f.restype = i64
    lib.dstagnn_window_stats_masked_scratch_bytes.argtypes = [i64, i32]
    lib.dstagnn_window_fill_scratch_bytes.argtypes = [i64, i32, i32]
    chunk, cols = lib.dstagnn_window_fill_chunk(), lib.dstagnn_window_fill_cols()
    assert chunk >= 2 and cols >= 2
    assert lib.dstagnn_window_fill_scratch_bytes(chunk + 1, 5, 3) == 2 * 15 * 4
    assert lib.dstagnn_window_fill_scratch_bytes(chunk, 5, 3) == 15 * 4
    assert lib.dstagnn_window_fill_scratch_bytes(0, 5, 3) == 0
    assert lib.dstagnn_window_stats_masked_scratch_bytes(1000, 3) == 2 * 512 * 3 * 8  # fp64 sums + int64 counts
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, vp)

    def err(rc, want, text):
        assert rc == want, (rc, want, lib.dstagnn_last_error())
        assert text in lib.dstagnn_last_error().decode()

    fill = lib.dstagnn_window_fill_forward
    fill.argtypes = [i32, vp, i64, i32, i32, dbl, i64, vp, vp, vp, sz, vp]
    q = ctypes.cast(ctypes.create_string_buffer(64), vp)
    err(fill(0, None, 100, 3, 2, 0.0, 0, q, p, p, 1 << 20, None), E_ARG, "window_fill_forward: null")
    err(fill(0, p, 100, 3, 2, 0.0, 0, p, q, q, 1 << 20, None), E_ARG, "filled == series")
    err(fill(0, p, 100, 3, 2, 0.0, -1, q, q, q, 1 << 20, None), E_ARG, "max_gap")
    err(fill(0, p, 100, 3, 300, 0.0, 0, q, q, q, 1 << 20, None), E_SHAPE, "F in [1, 256]")
    err(fill(0, p, 1 << 31, 3, 2, 0.0, 0, q, q, q, 1 << 20, None), E_SHAPE, "L in [1, 2^31)")
    err(fill(0, p, 100, 3, 2, 0.0, 0, q, q, q, 2 * 6 * 4 - 1, None), E_SPACE, "dstagnn_window_fill_scratch_bytes")

    stats = lib.dstagnn_window_stats_masked
    stats.argtypes = [i32, vp, i64, i32, i32, vp, dbl, vp, vp, vp, sz, vp]
    err(stats(0, p, 100, 3, 2, p, 0.0, p, None, p, 1 << 20, None), E_ARG, "window_stats_masked: null")
    err(stats(0, p, 100, 3, 257, p, 0.0, p, p, p, 1 << 20, None), E_SHAPE, "F in [1, 256]")
    err(stats(0, p, 100, 3, 2, p, 0.0, p, p, p, 2 * 100 * 2 * 8 - 1, None), E_SPACE, "scratch smaller")

    gather = lib.dstagnn_window_gather_masked
    gather.argtypes = [i32, vp, vp, i64, i32, i32, vp, i32, i32, vp, i64, vp, i32, vp, vp, dbl, vp, vp, vp]
    err(gather(0, None, p, 100, 3, 2, p, 12, 12, p, 5, p, 4, p, p, 0.0, p, p, None), E_ARG, "null xsrc")
    err(gather(0, p, None, 100, 3, 2, p, 12, 12, p, 5, p, 4, p, p, 0.0, p, p, None), E_ARG,
        "window_gather_masked: null")
    err(gather(0, p, p, 0, 3, 2, p, 12, 12, p, 5, p, 4, p, p, 0.0, p, p, None), E_SHAPE, "window_gather_masked: L")
    err(gather(0, p, p, 100, 3, 2, p, 1 << 20, 12, p, 5, p, 4, p, p, 0.0, p, p, None), E_SHAPE, "bytes of LDS")
