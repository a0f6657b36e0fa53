"""CPU: the forward-only block entry point (dstagnn_block_forward_only) — exported, registered as
ops, the same dims errors as dstagnn_block_sizes, and a workspace that holds no tensor only the
backward reads (a bound computed from shapes, not from what the library returns)."""
import ctypes

import pytest

import test_abi_module_cpu as ab
import test_gpu_parity as tp

PATH = {"FLASH": 2, "CHEB_AGG": 8, "TAT_FUSED_FWD": 16, "GTU_FUSED_FWD": 64}  # include/dstagnn.h DSTAGNN_PATH_*
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


@pytest.mark.parametrize("first", [True, False], ids=["first", "inner"])
@pytest.mark.parametrize("name", sorted(tp.CONFIGS))
def test_workspace_holds_no_backward_state(name, first):
    """work_bytes <= save_bytes - 4 floor + W: floor counts (in floats) tensors only the backward
    reads on the path the dims select — tco, r, G; conv_k where the GTU stage is fused; Q|K|V, ctx
    and u where the TAt stage is fused; the (B,N,K,F,T) aggregates on the aggregate-first path —
    and W the two GEMM and two column-sum workspaces of plan_scratch plus alignment slack."""
    lib = ab.c_abi()
    B = BASELINE_B.get(name, 2)
    d = _dims(name, first, B)
    N, T, K, h, D, dk, C, dv = tp.config(name)
    F = d.F
    bits, sv, sc, wb = ctypes.c_uint32(0), ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.dstagnn_block_paths(ctypes.byref(d), ctypes.byref(bits)) == 0, lib.dstagnn_last_error()
    assert lib.dstagnn_block_sizes(ctypes.byref(d), ctypes.byref(sv), ctypes.byref(sc)) == 0
    assert lib.dstagnn_block_forward_only_size(ctypes.byref(d), ctypes.byref(wb)) == 0
    BN, BFT, S = B * N, B * F * T, 3 * T - 12
    QW, HV = 2 * h * dk + h * dv, h * dv
    floor = 3 * BN * C * T + BN * C * S
    if bits.value & PATH["GTU_FUSED_FWD"]:
        floor += BN * 2 * C * S
    if bits.value & PATH["TAT_FUSED_FWD"]:
        floor += BFT * (QW + HV + N)
    if bits.value & PATH["CHEB_AGG"]:
        floor += B * N * K * F * T
    W = 4 * (2 * K_GEMM_WS + 2 * K_PART) + 65536
    bound = sv.value - 4 * floor + W
    print(f"{name} first={first} B={B}: work {wb.value} bound {bound} save {sv.value} scratch {sc.value}")
    assert wb.value <= bound, (wb.value, bound)
    assert wb.value < sv.value + sc.value
