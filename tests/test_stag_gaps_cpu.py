"""CPU: the host-side surface of the STAG graph on a series with gaps
(dstagnn_drought_amd/stag_gen.py): the command line, the argument checks that run before
anything touches the device, the HIP-only error, and the reference helper itself
(tests/stag_gaps_ref.py: its reduced LP equals its zero-marginal LP).  The device path is
tests/test_gpu_stag_gaps.py."""
import inspect
import math

import numpy as np
import pytest

import stag_gaps_ref as gref
from oracle import stag_ref as ref


def test_cli_parser():
    from dstagnn_drought_amd import stag_gen as sg
    ap = sg.build_parser()
    a = ap.parse_args(["--input", "x.npz", "--dataset", "G"])
    assert (a.input, a.dataset, a.period, a.sparsity, a.missing_value, a.min_observed) == ("x.npz", "G", 12, 0.01, None, 1)
    a = ap.parse_args(["--input", "x.npz", "--dataset", "G", "--period", "6", "--sparsity", "0.05",
                       "--missing-value", "nan", "--min-observed", "4"])
    assert isinstance(a.missing_value, float) and math.isnan(a.missing_value)
    assert (a.period, a.sparsity, a.min_observed) == (6, 0.05, 4)
    assert math.isnan(ap.parse_args(["--input", "x", "--dataset", "G", "--missing-value", "NaN"]).missing_value)
    a = ap.parse_args(["--input", "x.npz", "--dataset", "G", "--missing-value", "-9999"])
    assert isinstance(a.missing_value, float) and a.missing_value == -9999.0
    assert ap.parse_args(["--input", "x", "--dataset", "G", "--missing-value=1e20"]).missing_value == 1e20
    with pytest.raises(SystemExit):
        ap.parse_args(["--input", "x.npz", "--dataset", "G", "--missing-value", "none"])
    with pytest.raises(SystemExit):
        ap.parse_args(["--dataset", "G"])                       # --input is required, as in the reference
    assert callable(sg.main) and list(inspect.signature(sg.main).parameters) == ["argv"]


def test_signatures_keep_todays_calls():
    from dstagnn_drought_amd import stag_gen as sg

    def defaults(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not v.empty}
    assert defaults(sg.NodeData.__init__) == {"device": None, "missing_value": None, "min_observed": 1}
    assert defaults(sg.process_node_pair) == {"device": None, "missing_value": None}
    assert defaults(sg.sta_matrix) == {"device": None, "chunk": 1 << 20, "progress": None, "missing_value": None,
                                       "min_observed": 1}
    assert defaults(sg.adjacency) == {"device": None, "exclude": None}
    assert defaults(sg.process_dataset) == {"period": 12, "sparsity": 0.01, "device": None, "missing_value": None,
                                            "min_observed": 1}


@pytest.mark.parametrize("bad", [0, -3, 1.5])
def test_min_observed_below_one_raises(bad, tmp_path):
    from dstagnn_drought_amd import stag_gen as sg
    data = np.zeros((4, 3, 2))
    with pytest.raises(ValueError, match="min_observed"):
        sg.NodeData(data, "cpu", missing_value=float("nan"), min_observed=bad)
    with pytest.raises(ValueError, match="min_observed"):
        sg.sta_matrix(data, "cpu", missing_value=-1.0, min_observed=bad)
    path = tmp_path / "Z.npz"
    np.savez(path, data=data)
    with pytest.raises(ValueError, match="min_observed"):
        sg.process_dataset(str(path), "Z", device="cpu", missing_value=float("nan"), min_observed=bad)


def test_cpu_device_raises_hip_only_error():
    from dstagnn_drought_amd import stag_gen as sg
    data = np.random.RandomState(0).randn(6, 3, 2)
    data[1, 1, 0] = np.nan
    for call in (lambda: sg.NodeData(data, "cpu", missing_value=float("nan")),
                 lambda: sg.process_node_pair((0, 1, data), "cpu", missing_value=float("nan")),
                 lambda: sg.sta_matrix(data, "cpu", missing_value=float("nan"), min_observed=2),
                 lambda: sg.adjacency(np.zeros((3, 3)), 0.4, "cpu", exclude=np.array([False, True, False]))):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()


def test_ops_and_symbols_present():
    import ctypes
    from dstagnn_drought_amd import _lib
    ops = _lib.load()
    for n in ("stag_prep_masked", "stag_emd_pairs_masked", "stag_emd_lds_bytes_rect", "graph_topk_masked"):
        assert hasattr(ops, n), f"torch.ops.dstagnn.{n} missing"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.dstagnn_stag_emd_lds_bytes_rect.restype = ctypes.c_int64
    lib.dstagnn_stag_emd_lds_bytes.restype = ctypes.c_int64
    # a square workspace is the old one (F = 0: the kernels keep the unit rows in global memory)
    for T in (1, 7, 64, 287):
        assert ops.stag_emd_lds_bytes_rect(T, T) == ops.stag_emd_lds_bytes(T, 0) == lib.dstagnn_stag_emd_lds_bytes_rect(T, T)
    assert ops.stag_emd_lds_bytes_rect(205, 206) < ops.stag_emd_lds_bytes_rect(287, 287)
    assert ops.stag_emd_lds_bytes_rect(3, 200) == ops.stag_emd_lds_bytes_rect(200, 3)


@pytest.mark.parametrize("case", [0, 1, 2])
def test_helper_reduced_lp_equals_zero_marginal_lp(case):
    """The two statements of the masked EMD agree under HiGHS (both solved to ~1e-12)."""
    rs = np.random.RandomState(40 + case)
    T, F = (9, 16, 24)[case], (2, 4, 3)[case]
    x, y = rs.randn(T, F), rs.randn(T, F)
    ox, oy = rs.rand(T) >= 0.3, rs.rand(T) >= (0.1, 0.6, 0.45)[case]
    ox[0] = oy[1] = True
    if case == 2:
        x[::3] = 0.0                                            # observed zero rows
    full = ref.emd_linprog(*gref.zero_marginal_problem(x, y, ox, oy))
    _, _, p, q, D = gref.reduced_problem(x, y, ox, oy)
    assert len(p) == ox.sum() and len(q) == oy.sum()
    assert abs(full - gref.rect_linprog(p, q, D)) <= 1e-9
    assert 0.0 < full < 1.0
    # the rule itself: a marker in one feature hides the step; with a numeric marker a nan is valid
    d = np.array([[[1.0, -9999.0]], [[np.nan, 2.0]], [[3.0, 4.0]]])
    assert gref.observed(d, -9999.0)[:, 0].tolist() == [False, True, True]
    assert gref.observed(d, float("nan"))[:, 0].tolist() == [True, False, True]


def test_c_abi_argument_checks():
    """Checked before anything touches the device: null pointers and min_observed < 1 ->
    DSTAGNN_E_ARG; dimensions, Tmax outside [1, T] or beyond the int16 node ids / the LDS ->
    DSTAGNN_E_SHAPE; an empty pair list is a no-op."""
    import ctypes
    from dstagnn_drought_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.dstagnn_last_error.restype = ctypes.c_char_p
    E_SHAPE, E_ARG = 10001, 10002
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    i32, i64, f64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
    prep = lib.dstagnn_stag_prep_masked
    prep.argtypes = [vp, i32, i32, i32, f64, vp, vp, vp, vp, vp, vp]
    assert prep(p, 4, 3, 2, float("nan"), p, p, p, None, p, None) == E_ARG
    assert prep(p, 0, 3, 2, float("nan"), p, p, p, p, p, None) == E_SHAPE
    emd = lib.dstagnn_stag_emd_pairs_masked
    emd.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, i64, vp, vp, vp, vp]

    def call(T=8, Tmax=8, mo=1, cnt=p, P=0):
        return emd(p, p, p, cnt, T, Tmax, mo, 3, 2, p, P, p, p, None, None)
    assert call() == 0                                           # P = 0: nothing to do
    assert call(cnt=None) == E_ARG
    assert call(mo=0) == E_ARG and b"min_observed" in lib.dstagnn_last_error()
    assert call(Tmax=0) == E_SHAPE and call(Tmax=9) == E_SHAPE and b"Tmax" in lib.dstagnn_last_error()
    assert call(T=20000, Tmax=16384) == E_SHAPE and b"int16" in lib.dstagnn_last_error()
    assert call(T=20000, Tmax=8000) == E_SHAPE and b"LDS" in lib.dstagnn_last_error()
    assert call(P=-1) == E_SHAPE
    topk = lib.dstagnn_graph_topk_masked
    topk.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp]
    assert topk(None, 4, 2, 1, p, p, p, None, None) == E_ARG
    assert topk(p, 4, 5, 1, p, p, p, None, None) == E_SHAPE      # k > N
