"""CPU: the surface of HipAdam's opt-in clipping / weight decay / non-finite skip — the three
C-ABI symbols (declared in include/dstagnn.h, exported by the library), the three torch ops, the
constructor's validation, the new hyper-parameters through state_dict / load_state_dict (and a
torch.optim.Adam state_dict still loading), and the driver's optional [Training] keys."""
import configparser
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from dstagnn_drought_amd import train as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dstagnn_grad_sumsq", "dstagnn_adam_step_ex", "dstagnn_grad_scale"]


def test_header_declares_and_library_exports_the_symbols():
    from dstagnn_drought_amd import _lib
    with open(os.path.join(ROOT, "include", "dstagnn.h")) as f:
        src = f.read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(dstagnn_\w+)\s*\(", src, re.M))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in SYMBOLS + ["dstagnn_adam_step", "dstagnn_adam_chunk_elems"]:
        assert n in declared, f"include/dstagnn.h does not declare {n}"
        assert hasattr(lib, n), f"libdstagnn.so does not export {n}"
    assert "dstagnn_adam_hyper" in src  # the hyper-parameters of _ex travel in one struct
    ops = _lib.load()
    for n in ("grad_sumsq", "adam_step_ex", "grad_scale", "adam_step"):
        assert hasattr(ops, n), f"torch.ops.dstagnn.{n} missing"


def test_c_abi_refuses_bad_arguments():
    """No launch happens on these paths: null tables / missing stat are argument errors."""
    from dstagnn_drought_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)

    class Hyper(ctypes.Structure):  # dstagnn_adam_hyper (include/dstagnn.h)
        _fields_ = [(n, ctypes.c_float) for n in ("beta1", "beta2", "eps", "step_size", "bc2_sqrt", "lr",
                                                  "weight_decay")] + \
            [("decoupled", ctypes.c_int), ("max_norm", ctypes.c_float), ("skip_nonfinite", ctypes.c_int)]

    h = Hyper(0.9, 0.999, 1e-8, 1e-3, 1.0, 1e-3, 0.0, 0, 1.0, 0)
    assert lib.dstagnn_adam_step_ex(None, None, 0, ctypes.byref(h), None, None, None) == 10002  # clip without stat
    h.max_norm = 0.0
    assert lib.dstagnn_adam_step_ex(None, None, 0, ctypes.byref(h), None, None, None) == 0  # nothing to do
    h.weight_decay = -1.0
    assert lib.dstagnn_adam_step_ex(None, None, 0, ctypes.byref(h), None, None, None) == 10002
    assert lib.dstagnn_adam_step_ex(None, None, 1, None, None, None, None) == 10002
    assert lib.dstagnn_grad_sumsq(None, None, 1, None, None, None) == 10002
    assert lib.dstagnn_grad_scale(None, None, 0, None, ctypes.c_float(1.0), None) == 10002


def _params():
    return [nn.Parameter(torch.randn(3, 2)), nn.Parameter(torch.randn(4))]


def test_invalid_options_raise_value_error():
    for kw in (dict(max_grad_norm=-1.0), dict(max_grad_norm=0.0), dict(weight_decay=-0.1),
               dict(weight_decay=float("nan")), dict(max_grad_norm=float("nan"))):
        with pytest.raises(ValueError):
            TR.HipAdam(_params(), lr=1e-3, **kw)
    with pytest.raises(ValueError):
        TR.make_adam(_params(), 1e-3, weight_decay=-1.0)
    with pytest.raises(ValueError):
        TR.clip_grad_norm_(_params(), -1.0)
    ok = TR.HipAdam(_params(), lr=1e-3)  # the defaults: nothing on
    g = ok.param_groups[0]
    assert (g["weight_decay"], g["decoupled_weight_decay"], g["max_grad_norm"], g["skip_nonfinite"]) == \
        (0.0, False, None, False)
    assert ok.grad_norm is None and int(ok.skipped_steps) == 0


def test_new_hyper_parameters_survive_state_dict():
    p = _params()
    a = TR.HipAdam(p, lr=2e-3, weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=0.5,
                   skip_nonfinite=True)
    sd = a.state_dict()
    b = TR.HipAdam(p, lr=1e-3)
    b.load_state_dict(sd)
    g = b.param_groups[0]
    assert (g["lr"], g["weight_decay"], g["decoupled_weight_decay"], g["max_grad_norm"], g["skip_nonfinite"]) == \
        (2e-3, 0.01, True, 0.5, True)
    bad = a.state_dict()
    bad["param_groups"][0]["max_grad_norm"] = -2.0
    with pytest.raises(ValueError):
        b.load_state_dict(bad)


def test_torch_adam_state_dict_still_loads():
    p = _params()
    ref = torch.optim.Adam(p, lr=1e-3, weight_decay=0.02)
    for q in p:
        q.grad = torch.ones_like(q)
    ref.step()
    ha = TR.HipAdam(p, lr=5e-3, max_grad_norm=2.0, skip_nonfinite=True)
    ha.load_state_dict(ref.state_dict())
    g = ha.param_groups[0]
    assert [ha.state[q]["step"] for q in p] == [1, 1]
    assert g["lr"] == 1e-3 and g["weight_decay"] == 0.02  # torch's own keys are taken over
    assert g["max_grad_norm"] == 2.0 and g["skip_nonfinite"] is True  # the ones it lacks keep the defaults
    assert g["decoupled_weight_decay"] in (False, 0)


def _section(text):
    cp = configparser.ConfigParser()
    cp.read_string(text)
    return cp["Training"]


def test_training_options_parse():
    assert TR.training_options(_section("[Training]\nlearning_rate = 0.0001\n")) == (None, 0.0, False)
    got = TR.training_options(_section("[Training]\nmax_grad_norm = 5\nweight_decay = 1e-4\n"
                                       "decoupled_weight_decay = true\n"))
    assert got == (5.0, 1e-4, True)
    assert TR.training_options(_section("[Training]\nweight_decay = 0.01\n")) == (None, 0.01, False)


def test_make_adam_maps_the_options_to_torch_off_the_gpu():
    """CPU parameters take make_adam's torch branch (as DSTAGNN_ADAM=torch does on the GPU): L2
    decay -> Adam(weight_decay=), decoupled -> AdamW, clipping -> clip_grad_norm_ before the step."""
    p = _params()
    o = TR.make_adam(p, 1e-3, weight_decay=0.1)
    assert type(o) is torch.optim.Adam and o.param_groups[0]["weight_decay"] == 0.1
    o = TR.make_adam(p, 1e-3, weight_decay=0.1, decoupled=True)
    assert type(o) is torch.optim.AdamW and o.param_groups[0]["weight_decay"] == 0.1
    o = TR.make_adam(p, 1e-3, max_grad_norm=0.5)
    for q in p:
        q.grad = torch.full_like(q, 3.0)
    o.step()
    norm = torch.sqrt(sum((q.grad.double() ** 2).sum() for q in p))
    assert abs(float(norm) - 0.5) < 1e-5  # the hook clipped the gradients in place
    assert type(TR.make_adam(p, 1e-3)) is torch.optim.Adam  # nothing given: as before
