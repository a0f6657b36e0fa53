"""The in-kernel folds share one pool of ticket counters per stream (csrc/handoff.hpp;
stream_counters in streams.hip): every kernel that hands partial sums between its workgroups draws
its tickets from the start of that pool and must leave them at zero for whichever user the stream
runs next.  tests/test_gpu_colsum.py checks that for colsum2d alone; this is the same pattern
across the users a test can reach in one process:

  - the block backward at the geometry of test_gpu_parity's "n40" case (B = 141, inner block,
    broadcast res_att): tat_fused_bwd_kernel (res_att ticket per sample, LayerNorm tree of 71
    level-1 groups, the last of 8, five level-2 chunks) and gtu_bwd_fused_kernel (17 level-1
    groups, the last of one workgroup, two level-2 chunks), plus the block's own colsum2d and
    skinny GEMM launches
  - colsum2d_kernel at (7, 3, 5) and (333, 40, 16)
  - skinny_dw_kernel with its two-level fold (test_gemm_skinny_two_level_fold's shape)
  - grad_sumsq_kernel over two tensors of 4099 and 31 x 17 floats

Each runs once, then the whole list five more times in rotated order on one stream; every result
must be torch.equal to its first.  A user that leaves a ticket non-zero, or reads a partial before
its acquire, shows up as a changed sum in its neighbour.  Fixed inputs: a determinism check, not a
stress loop.

Not here: the DSTAGNN_TAIL_FOLD=1 tail fold and the unfused temporal attention's res_att fold
(DSTAGNN_TAT_FUSED=0).  The library reads its switches once per process, so no in-process test
reaches them; they stay with their rows of tests/test_gpu_knobs.py.
"""
import pytest
import torch

import test_gpu_parity as tp

pytestmark = pytest.mark.gpu

ROUNDS = 5


def _block_backward():
    import dstagnn_drought_amd as D_
    from dstagnn_drought_amd.block_fn import block_paths
    B = 141
    N, T, K, h, D, dk, C = tp.CONFIGS["n40"]
    _, p, x, res, cheb, apa, _, gen = tp._oracle_case(B, N, T, K, h, D, dk, C, False, 1, seed=3)
    blk = D_.DSTAGNN_block("cpu", C, C, K, C, C, 1, cheb, apa, apa, N, T, D, dk, dk, h)
    blk.load_state_dict(p)
    blk = blk.cuda().eval()
    g_out = torch.randn(B, N, C, T, generator=gen).cuda()
    g_re = torch.randn(B, C, h, T, T, generator=gen).cuda()
    xg = x.cuda().requires_grad_(True)
    rg = res.cuda().requires_grad_(True)
    took = block_paths(blk, xg, rg)
    assert {"tat_fused_bwd", "gtu_fused_bwd"} <= took, sorted(took)
    params = [prm for _, prm in blk.named_parameters()]

    def run():
        for t in [xg, rg] + params:
            t.grad = None
        out, re_at = blk(xg, rg)
        ((out * g_out).sum() + (re_at * g_re).sum()).backward()
        return [xg.grad, rg.grad] + [prm.grad for prm in params if prm.grad is not None]
    return run


def _colsum(A, O, I):
    from dstagnn_drought_amd import _lib
    ops = _lib.load()
    x = torch.randn(A, O, I, generator=torch.Generator().manual_seed(A * 131 + O * 7 + I)).cuda()
    return lambda: [ops.colsum(x, O, I)]


def _skinny_two_level():
    g = torch.Generator().manual_seed(12)
    BN, K, F, T, C = 5440, 3, 32, 12, 32
    agg = torch.randn(BN, K, F, T, generator=g).cuda()
    gp = torch.randn(BN, T, C, generator=g).cuda()

    def run():
        Cd = torch.empty(K * F, C, device="cuda")
        tp._gemm(agg, gp, Cd, K * F, C, BN * T, (0, T, 0), (T, 1, K * F * T), (0, C, 0), (0, 1, 0), (0, C, 0), (0, 1, 0))
        return [Cd]
    return run


def _grad_sumsq():
    from dstagnn_drought_amd import _lib
    ops = _lib.load()
    g = torch.Generator().manual_seed(7)
    gs = [torch.randn(4099, generator=g).cuda(), torch.randn(31, 17, generator=g).cuda()]
    return lambda: [ops.grad_sumsq(gs)]


def test_every_fold_leaves_the_shared_tickets_at_zero():
    tp._need_gpu()
    users = [("block backward", _block_backward()), ("colsum (7, 3, 5)", _colsum(7, 3, 5)),
             ("colsum (333, 40, 16)", _colsum(333, 40, 16)), ("skinny two-level", _skinny_two_level()),
             ("grad_sumsq", _grad_sumsq())]
    first = {name: [t.clone() for t in run()] for name, run in users}
    torch.cuda.synchronize()
    for r in range(1, ROUNDS + 1):
        k = r % len(users)
        for name, run in users[k:] + users[:k]:
            got = run()
            assert len(got) == len(first[name])
            for j, (a, b) in enumerate(zip(got, first[name])):
                assert torch.equal(a, b), f"round {r}: {name}, result {j} differs from its first run"
