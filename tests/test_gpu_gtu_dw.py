"""The GTU convolution weight / bias gradients as one sliding-window kernel and a fixed-order fold
(gtu_dw.hip: gtu_dw_kernel, gtu_dw_fold_kernel) in place of the grouped split-K GEMM.

1. Exact values through the direct op (dstagnn::gtu_dw): integer-valued operands in [-3, 3], so
   every sum is an integer far below 2^24 (at most 9 * 17 * 10 here) and the float64 einsum is met
   EXACTLY.  With S = nodes per LDS stage (dstagnn::gtu_dw_plan): BN in {1, S-1, S, S+1, 2S+1} x forced
   chunk counts {1, 2, 3}, one count above BN (empty chunks) and the planner's own partition.  The
   op hands the kernel a NaN-filled workspace, so a partial nobody wrote shows.
2. Determinism: normal operands, the same call three times, all six outputs bit-identical.
3. The block against the fp64 oracle through test_gpu_parity._run_config_vs_oracle and its own
   bound (no new number), the fused GTU backward asserted.
4. Which path ran, from the library's GEMM log in one child process: the cases of 3 log no GEMM of
   the shapes M=64 N=97|161|225; T = 8 and C = 16 (no fused backward: M = 2C, N = C kw + 1) still log
   all three.  (A weight frozen by requires_grad_(False) does not reach the gate: the operator
   boundary asks the library for every used parameter's gradient and drops the unwanted ones.)
"""
import os
import subprocess
import sys

import pytest
import torch

import test_gpu_parity as P
from test_gpu_parity import _run_config_vs_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GEOM = {  # name: (N, T, K, h, D, dk, C)
    "gdw_base": (40, 12, 3, 3, 64, 32, 32),  # fused GTU forward and backward: the new kernel
    "gdw_t8": (40, 8, 3, 3, 64, 32, 32),     # T != 12: the padded rows and the grouped GEMM
    "gdw_c16": (40, 12, 3, 3, 64, 32, 16),   # C != 32: the same
}
P.CONFIGS.update(GEOM)

# (name, first, B, train)
CASES = [("gdw_base", False, 3, True), ("gdw_base", False, 3, False), ("gdw_base", False, 1, False),
         ("gdw_base", True, 2, True)]
REFUSED = [("gdw_t8", False, 3, False), ("gdw_c16", False, 3, False)]
KWS = (3, 5, 7)
T, C = 12, 32


def _ops():
    from dstagnn_drought_amd import _lib
    return _lib.load()


def _operands(BN, gen, integer):
    def draw(*shape):
        if integer:
            return torch.randint(-3, 4, shape, generator=gen).float()
        return torch.randn(*shape, generator=gen)
    return [draw(BN * (T - kw + 1), 2 * C) for kw in KWS], draw(BN, T, C)


def _reference(dconv, X):
    """float64: dW[o, c, j] = sum_{bn, t'} dconv[(bn, t'), o] X[bn, t' + j, c]; db[o] = sum dconv[., o]."""
    BN = X.shape[0]
    ws, bs = [], []
    for kw, d in zip(KWS, dconv):
        Tg = T - kw + 1
        win = X.double().unfold(1, kw, 1)  # (BN, Tg, C, kw): X[bn, t' + j, c]
        ws.append(torch.einsum("nto,ntcj->ocj", d.double().view(BN, Tg, 2 * C), win))
        bs.append(d.double().sum(0))
    return ws + bs


def _stage_nodes():
    return int(_ops().gtu_dw_plan(64)[3])


def _bns():
    S = _stage_nodes()
    return sorted({1, S - 1, S, S + 1, 2 * S + 1})


_REF = {}


def _exact_case(BN):
    if BN not in _REF:
        gen = torch.Generator().manual_seed(100 + BN)
        dconv, X = _operands(BN, gen, integer=True)
        _REF[BN] = (dconv, X, _reference(dconv, X))
    return _REF[BN]


@pytest.mark.parametrize("pos", range(5))
def test_exact_integer_values(pos):
    P._need_gpu()
    BN = _bns()[pos]
    dconv, X, ref = _exact_case(BN)
    dev = [d.cuda() for d in dconv] + [X.cuda()]
    for chunks in (1, 2, 3, BN + 3, 0):  # BN + 3: more chunks than nodes; 0: the planner's partition
        got = _ops().gtu_dw(*dev, chunks)
        torch.cuda.synchronize()
        assert len(got) == 6
        for q, (g, r) in enumerate(zip(got, ref)):
            what = "dW%d" % KWS[q] if q < 3 else "db%d" % KWS[q - 3]
            assert g.shape == r.shape, (what, g.shape, r.shape)
            assert torch.equal(g.double().cpu(), r), (BN, chunks, what, float((g.double().cpu() - r).abs().max()))


def test_plan_is_proportional_and_bounded():
    P._need_gpu()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    c3, c5, c7, S = [int(v) for v in _ops().gtu_dw_plan(5440)]
    assert S % 4 == 0 and S >= 4
    assert abs(c3 + c5 + c7 - cus) <= 2, (c3, c5, c7, cus)           # about one round of the device
    assert c3 < c5 < c7 and abs(c3 * 42 - c7 * 30) <= 42 + 30, (c3, c5, c7)  # 30 : 40 : 42 up to rounding
    assert [int(v) for v in _ops().gtu_dw_plan(5440)] == [c3, c5, c7, S]     # a function of BN and the device
    small = [int(v) for v in _ops().gtu_dw_plan(5)]
    assert small[:3] == [2, 2, 2], small                               # never more chunks than 4-node groups


def test_bit_identical_over_reruns():
    P._need_gpu()
    gen = torch.Generator().manual_seed(7)
    dconv, X = _operands(1030, gen, integer=False)
    dev = [d.cuda() for d in dconv] + [X.cuda()]
    ref = _reference(dconv, X)
    runs = [_ops().gtu_dw(*dev, 0) for _ in range(3)]
    torch.cuda.synchronize()
    for q in range(6):
        # (fp32 sums of 1030 * Tg unit-normal products: far inside 1e-4 of the result's scale)
        r = ref[q]
        assert float((runs[0][q].double().cpu() - r).abs().max()) <= 1e-4 * max(1.0, float(r.abs().max())), q
        for rep in (1, 2):
            assert torch.equal(runs[0][q].view(torch.int32), runs[rep][q].view(torch.int32)), (q, rep)


def _id(c):
    return "%s-%s-B%d-%s" % (c[0], "first" if c[1] else "inner", c[2], "train" if c[3] else "eval")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_block_vs_oracle(case):
    name, first, B, train = case
    _run_config_vs_oracle(name, first, B, train=train, paths={"gtu_fused_bwd"})


# ---------------------------------------------------------------------------------------
# which path ran: the library's own GEMM log
# ---------------------------------------------------------------------------------------
PATH_RUNS = CASES + REFUSED

PATH_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
import dstagnn_drought_amd as D
import test_gpu_parity as T
import test_gpu_gtu_dw as M
for name, first, B, train in M.PATH_RUNS:
    N, Tn, K, h, Dm, dk, C = M.GEOM[name]
    ref, p, x, res, cheb, apa, dims, gen = T._oracle_case(B, N, Tn, K, h, Dm, dk, C, first, 0 if first else 1, seed=3)
    F = x.shape[2]
    blk = D.DSTAGNN_block("cpu", F, F, K, C, C, 1, cheb, apa, apa, N, Tn, Dm, dk, dk, h)
    blk.load_state_dict(p)
    blk = blk.cuda().train(train)
    xg = x.cuda().requires_grad_(True)
    rg = res.cuda().requires_grad_(True) if torch.is_tensor(res) else 0
    torch.cuda.synchronize()
    sys.stderr.write("[case] %s %d %d %d\\n" % (name, int(first), B, int(train))); sys.stderr.flush()
    out, re_at = blk(xg, rg)
    (out.sum() + re_at.sum()).backward()
    torch.cuda.synchronize()
print("LOG_OK")
"""


def _dw_shapes(C):
    return ["M=%d N=%d " % (2 * C, C * kw + 1) for kw in KWS]


def test_dw_gemm_only_where_refused():
    P._need_gpu()
    e = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", DSTAGNN_GEMM_LOG="1")
    r = subprocess.run([sys.executable, "-c", PATH_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))],
                       cwd=ROOT, env=e, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0 and "LOG_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    per, cur = {}, None
    for ln in r.stderr.splitlines():
        if ln.startswith("[case] "):
            cur = ln[7:]
            per[cur] = []
        elif ln.startswith("[gemm]") and cur is not None:
            per[cur].append(ln)
    assert len(per) == len(PATH_RUNS), sorted(per)
    for case in PATH_RUNS:
        name, first, B, train = case
        lines = per["%s %d %d %d" % (name, int(first), B, int(train))]
        assert lines, (name, "the block logged no GEMM")
        shapes = _dw_shapes(GEOM[name][6])
        hit = [sh for sh in shapes if any(sh in ln for ln in lines)]
        if case in REFUSED:
            assert hit == shapes, (name, "the refused geometry lost its weight-gradient GEMMs", hit)
        else:
            assert shapes == ["M=64 N=97 ", "M=64 N=161 ", "M=64 N=225 "]
            assert not hit, (case, "the GTU weight gradients still run as GEMMs", hit)
