"""CPU: the forward-only block entry point (dstagnn_block_forward_only) — exported, registered as
ops, the same dims errors as dstagnn_block_sizes, and a workspace that holds no tensor only the
backward reads (a bound computed from shapes, not from what the library returns).  The save arena
itself: the parent build's size minus exactly the slots DESIGN.md §14.4 drops, both ways."""
import ctypes
import json
import os

import pytest

import kernel_coverage as kc
import test_abi_module_cpu as ab
import test_gpu_parity as tp

PATH = {"FLASH": 2, "CHEB_AGG": 8, "TAT_FUSED_FWD": 16, "TAT_FUSED_BWD": 32, "GTU_FUSED_FWD": 64,
        "GTU_FUSED_BWD": 128}  # include/dstagnn.h DSTAGNN_PATH_*
K_GEMM_WS, K_PART = 8 << 20, 2 << 20  # floats: block.hip kGemmWs, kPart
BASELINE_B = {"pems08": 32, "pems04": 32, "pems07": 12, "gambia": 4, "syn": 32}


def test_exports_and_ops():
    from dstagnn_drought_amd import _lib
    lib = ab.c_abi()
    for n in ("dstagnn_block_forward_only_size", "dstagnn_block_forward_only"):
        assert hasattr(lib, n), f"libdstagnn.so does not export {n}"
        assert n in ab.header_functions(), f"include/dstagnn.h does not declare {n}"
    ops = _lib.load()
    for n in ("block_fwd_only", "block_fwd_only_bytes"):
        assert hasattr(ops, n), f"torch.ops.dstagnn.{n} missing"


def test_size_errors_match_block_sizes():
    lib = ab.c_abi()
    wb, sv, sc = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    ok = ab.BlockDims(32, 170, 32, 12, 3, 32, 32, 512, 3, 32, 1, 1, 0.05, 0)
    assert lib.dstagnn_block_forward_only_size(ctypes.byref(ok), ctypes.byref(wb)) == 0
    assert wb.value > 0
    bad = ab.BlockDims(1, 16, 4, 12, 2, 8, 8, 16, 2, 8, 0, 0, 0.05, 0)  # GAMBIA in_channels=4 (quirk 8)
    neg = ab.BlockDims(32, 170, 32, 12, 3, 32, 32, 512, 3, 32, 1, 1, 0.05, 0)
    neg.sample_base = -1
    for dims, code, text in ((bad, 10001, b"must match"), (neg, 10002, b"sample_base")):
        rc_ref = lib.dstagnn_block_sizes(ctypes.byref(dims), ctypes.byref(sv), ctypes.byref(sc))
        text_ref = lib.dstagnn_last_error()
        rc = lib.dstagnn_block_forward_only_size(ctypes.byref(dims), ctypes.byref(wb))
        assert rc == rc_ref == code
        assert lib.dstagnn_last_error() == text_ref and text in text_ref
    assert lib.dstagnn_block_forward_only_size(ctypes.byref(ok), None) == 10002


def _dims(name, first, B):
    N, T, K, h, D, dk, C, dv = tp.config(name)
    d = ab.BlockDims(B, N, 1 if first else C, T, h, dk, dv, D, K, C, 0 if first else 1, 0, 0.05, 0)
    d.cheb_sparse, d.cheb_flash, d.cheb_nnz, d.cheb_apa_nnz = 1, int(dk == 32), 3 * N, 4 * N  # block_fn.use_flash
    return d


def plan_of(lib, d):
    """(path bits, save bytes, scratch bytes, forward-only work bytes) the library plans for d."""
    bits, sv, sc, wb = ctypes.c_uint32(0), ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.dstagnn_block_paths(ctypes.byref(d), ctypes.byref(bits)) == 0
    assert lib.dstagnn_block_sizes(ctypes.byref(d), ctypes.byref(sv), ctypes.byref(sc)) == 0
    assert lib.dstagnn_block_forward_only_size(ctypes.byref(d), ctypes.byref(wb)) == 0
    return bits.value, sv.value, sc.value, wb.value


def row_key(name, first, B):
    return "%s-%s-B%d" % (name, "first" if first else "inner", B)


DTH_BASE_ROWS = [("dth_base", False, 3), ("dth_base", True, 2)]  # tests/test_gpu_cheb_dtheta.py GEOM


def size_rows():
    """Every row the size tests may ask the fixture for (tools/record_save_plan.py): the geometries
    of test_gpu_parity.CONFIGS, with those the other GPU modules add to it at import."""
    import test_gpu_cheb_dtheta  # noqa: F401
    import test_gpu_gtu_dw  # noqa: F401
    return [(n, f, BASELINE_B.get(n, 2)) for n in sorted(tp.CONFIGS) for f in (True, False)] + DTH_BASE_ROWS


def parent_row(name, first, B):
    """The parent build's plan of this row (tests/golden/save_plan_parent_sizes.json: recorded on the
    host from the commit before the save slots were dropped)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "save_plan_parent_sizes.json")) as f:
        rows = json.load(f)["rows"]
    assert row_key(name, first, B) in rows, f"no parent record of {row_key(name, first, B)}"
    return rows[row_key(name, first, B)]


def dropped_slots(d, bits):
    """{slot: floats} of the save slots the training plan drops on the path the bits name (the
    table of DESIGN.md §14.4); the in-kernel dTheta has no path bit, so tests/kernel_coverage.py's
    mirror of its predicate decides it."""
    B, N, F, T, K, C, h = d.B, d.N, d.F, d.T, d.K, d.C, d.n_heads
    BN, BFT, S, QW = B * N, B * F * T, 3 * T - 12, 2 * h * d.d_k + h * d.d_v
    on = {k: bool(bits & v) for k, v in PATH.items()}
    out = {}
    if on["CHEB_AGG"] and kc.cheb_agg_dtheta_fused(B, N, F, C, K, T):
        out["xth"] = BN * K * C * T
    if on["GTU_FUSED_FWD"] and on["GTU_FUSED_BWD"]:
        out["G"] = BN * C * S
    if on["TAT_FUSED_FWD"] and F != 1:
        out["E"] = BFT * N
    for g, ks in enumerate((3, 5, 7)):
        if on["GTU_FUSED_BWD"]:
            out[f"Wgb{g}"] = 2 * C * C * ks
        if on["GTU_FUSED_FWD"] and not on["GTU_FUSED_BWD"]:
            out[f"Wgf{g}"] = 2 * C * C * ks
    if on["TAT_FUSED_FWD"] and on["TAT_FUSED_BWD"]:
        out["Wqkv"] = QW * N
    return out


def align256(n):
    return (n + 255) & ~255


def _check_row(name, first, B):
    lib = ab.c_abi()
    d = _dims(name, first, B)
    N, T, K, h, D, dk, C, dv = tp.config(name)
    F = d.F
    bits, sv, sc, wb = plan_of(lib, d)
    par = parent_row(name, first, B)
    assert bits == par["paths"], (bits, par["paths"])
    dropped = dropped_slots(d, bits)
    dead = sum(align256(4 * n) for n in dropped.values())
    print(f"{name} first={first} B={B}: work {wb} (parent {par['work']}) save {sv} (parent {par['save']}, "
          f"dropped {dead}: {sorted(dropped)}) scratch {sc}")
    # the forward-only workspace and the scratch arena are the parent's; the save arena is the
    # parent's less exactly the dropped slots (every slot starts 256-aligned: only the last slot's
    # unrounded tail depends on the order)
    assert abs(wb - par["work"]) <= 256, (wb, par["work"])
    assert sc == par["scratch"], (sc, par["scratch"])
    assert abs(sv - (par["save"] - dead)) <= 256, (sv, par["save"], dead, sorted(dropped))
    # work_bytes <= save_bytes - 4 floor + W, save_bytes the parent's (the size this bound was stated in)
    BN, BFT, S = B * N, B * F * T, 3 * T - 12
    QW, HV = 2 * h * dk + h * dv, h * dv
    floor = 3 * BN * C * T + BN * C * S
    if bits & PATH["GTU_FUSED_FWD"]:
        floor += BN * 2 * C * S
    if bits & PATH["TAT_FUSED_FWD"]:
        floor += BFT * (QW + HV + N)
    if bits & PATH["CHEB_AGG"]:
        floor += B * N * K * F * T
    W = 4 * (2 * K_GEMM_WS + 2 * K_PART) + 65536
    bound = par["save"] - 4 * floor + W
    assert wb <= bound, (wb, bound)
    assert wb < sv + sc
    return par["save"] - sv, dropped


@pytest.mark.parametrize("first", [True, False], ids=["first", "inner"])
@pytest.mark.parametrize("name", sorted(tp.CONFIGS))
def test_workspace_holds_no_backward_state(name, first):
    """work_bytes <= save_bytes - 4 floor + W: floor counts (in floats) tensors only the backward
    reads on the path the dims select — tco, r, G; conv_k where the GTU stage is fused; Q|K|V, ctx
    and u where the TAt stage is fused; the (B,N,K,F,T) aggregates on the aggregate-first path —
    and W the two GEMM and two column-sum workspaces of plan_scratch plus alignment slack;
    save_bytes is the parent build's.  Against that build: work_bytes within 256 bytes, scratch_bytes
    equal, and save_bytes the parent's minus the slots of DESIGN.md §14.4 to within 256 bytes."""
    _check_row(name, first, BASELINE_B.get(name, 2))


def test_baseline_and_dth_base_rows_shrink():
    """The drop is not vacuous (it would be if a knob's default changed): the PEMS rows lose at
    least the aggregates, G and the flipped GTU weights (50 453 760 bytes at PEMS08 inner, B = 32,
    28.5 % of the parent's arena), dth_base inner every slot of the table that can go together,
    dth_base first all of those but E (its EmbedT LayerNorm writes E)."""
    for name in ("pems08", "pems04", "pems07"):
        for first in (True, False):
            shrunk, dropped = _check_row(name, first, BASELINE_B[name])
            assert {"xth", "G", "Wgb0", "Wgb1", "Wgb2"} <= set(dropped) and shrunk > 0, (name, first, sorted(dropped))
    shrunk, _ = _check_row("pems08", False, 32)
    assert abs(shrunk - 50453760) <= 256, shrunk
    import test_gpu_cheb_dtheta  # noqa: F401  (adds dth_base to test_gpu_parity.CONFIGS)
    six = {"xth", "G", "E", "Wqkv", "Wgb0", "Wgb1", "Wgb2"}
    for (name, first, B), want in zip(DTH_BASE_ROWS, (six, six - {"E"})):
        shrunk, dropped = _check_row(name, first, B)
        assert set(dropped) == want and shrunk > 0, (first, sorted(dropped))
