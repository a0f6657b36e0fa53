"""dTheta from the transposed SpMM itself (cheb_agg.hip cheb_agg_spmm_t2_kernel<., ., DTH>), the
forward that no longer stores agg_k, and the fused GTU forward that no longer stores G when the
fused backward follows.

Values: the block forward + backward against the fp64 oracle through test_gpu_parity's own
machinery (_run_config_vs_oracle: the HIP's ReLU decisions handed to the oracle, every output and
gradient within max(1e-4 * scale, 2 x the fp32 oracle's own error) — the bound the existing oracle
rows apply to the Theta_k gradients; no new number here).  The geometries are small (N = 40:
ceil(2 * 40 / 4) = 20 workgroups at B = 3, rounded up to 24 rows of partial sums of which four are
padding; the fold kernel's 16 row subsets then hold two rows or one; B = 1: 10 of 16 rows, one row or
none per subset) and are added to that module's CONFIGS table at import.

Paths: one child process with DSTAGNN_GEMM_LOG=1 runs every geometry once; a case on the new path
logs no GEMM of the dTheta shape (M = K F, N = C, K = B N T), a Chebyshev order the predicate
refuses (K = 6: the KM = 8 template) still logs it — and so does a batch whose fold rows pass the
scratch (WS_CASES: the last batch admitted and the first refused at <4, 5>, and the plain forms
<8, 5>, <6, 5>, <4, 3> just past the bound, which nothing else runs).
"""
import os
import subprocess
import sys

import pytest
import torch

import test_gpu_parity as P
from test_gpu_parity import _oracle_case, _run_config_vs_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GEOM = {  # name: (N, T, K, h, D, dk, C)
    "dth_base": (40, 12, 3, 3, 64, 32, 32),  # spmm_t2<6, 3>, fused GTU forward and backward
    "dth_k1": (40, 12, 1, 3, 64, 32, 32),    # <6, 2> with K < KM
    "dth_k5": (40, 12, 5, 3, 64, 32, 32),    # <6, 5>
    "dth_t8": (40, 8, 3, 3, 64, 32, 32),     # <4, 3>: the x operand in LDS
    "dth_t16": (40, 16, 3, 3, 64, 32, 32),   # <8, 3>: a pair fills all 32 MFMA rows
    "dth_c16": (40, 12, 3, 3, 64, 32, 16),   # the narrow channel count (<4, 3>)
    "dth_n64": (64, 12, 3, 3, 64, 32, 32),   # with hub = 40: a support row past one 32-entry chunk
    "dth_k6": (40, 12, 6, 3, 64, 32, 32),    # refused (KM = 8): agg_k and the GEMM stay
    # both sides of the fold-scratch bound (cheb_agg_dtheta_ws_floats <= kGemmWs = 8 388 608 floats), K = 5,
    # F = C = 32, N = 40: B = 325 is 163 pairs, 1632 workgroup rows of 5120 floats = 8 355 840 (in-kernel);
    # B = 327 is 1640 rows, 8 396 800 floats (refused: the plain spmm_t2 form, agg_k and the GEMM)
    "dth_ws_t8": (40, 8, 5, 3, 64, 32, 32),   # <4, 5>
    "dth_ws_t16": (40, 16, 5, 3, 64, 32, 32),  # <8, 5>
    "dth_ws_t9": (40, 9, 5, 3, 64, 32, 32),    # <6, 5>, refused at B = 327 like the two above
    # K = 3: rows of 3072 floats, so the first refused batch is larger; B = 545 is 273 pairs (the last a lone sample), 2736 rows, 8 404 992 floats
    "dth_ws_k3t7": (40, 7, 3, 3, 64, 32, 32),  # <4, 3>
}
P.CONFIGS.update(GEOM)

# (name, first, B, train, hub)
BASE_CASES = [("dth_base", False, 3, False, 0), ("dth_base", False, 3, True, 0),   # one pair + a lone sample
              ("dth_base", False, 1, False, 0), ("dth_base", False, 1, True, 0),   # a lone sample only
              ("dth_base", True, 2, False, 0), ("dth_base", True, 2, True, 0)]     # the first block (F = 1)
SHAPE_CASES = [("dth_k1", False, 3, False, 0), ("dth_k5", False, 3, False, 0), ("dth_t8", False, 3, False, 0),
               ("dth_t16", False, 3, False, 0), ("dth_c16", False, 3, False, 0), ("dth_n64", False, 3, False, 40)]
REFUSED = ("dth_k6", False, 3, False, 0)
# (name, first, B, train, hub) -> whether the dTheta scratch admits the batch
WS_CASES = {("dth_ws_t8", False, 325, False, 0): True, ("dth_ws_t8", False, 327, False, 0): False,
            ("dth_ws_t16", False, 327, False, 0): False, ("dth_ws_t9", False, 327, False, 0): False,
            ("dth_ws_k3t7", False, 545, False, 0): False}


def _id(c):
    return "%s-%s-B%d-%s%s" % (c[0], "first" if c[1] else "inner", c[2], "train" if c[3] else "eval",
                               "-hub%d" % c[4] if c[4] else "")


@pytest.mark.parametrize("case", BASE_CASES + SHAPE_CASES + [REFUSED], ids=_id)
def test_block_vs_oracle(case):
    name, first, B, train, hub = case
    _run_config_vs_oracle(name, first, B, train=train, hub=hub, paths={"sparse", "cheb_agg"})


@pytest.mark.parametrize("case", list(WS_CASES), ids=_id)
def test_scratch_bound_sides_vs_oracle(case):
    """The last batch the fold scratch admits and the first it refuses, at the suite's bound, with
    test_gpu_parity.FLIP_CAP on the ReLU decisions that differ (these rows compare 5e6 of them).
    FLIP_CAP's condition, checked on the CPU (seed 3): the fp32 oracle against the fp64 oracle flips
    0 of 9 984 000 (B = 325, T = 8), 2 of 10 045 440 (B = 327, T = 8), 1 of 20 090 880 (B = 327, T = 16),
    0 of 11 301 120 (B = 327, T = 9) and 1 of 14 649 600 (B = 545, T = 7) decisions, at most 2e-7 against the 1e-5 the cap
    presumes.  The rows' time is the
    fp64 oracle's on the host."""
    name, first, B, train, hub = case
    errs, stats, owns = {}, {}, {}
    flips = _run_config_vs_oracle(name, first, B, train=train, hub=hub, paths={"sparse", "cheb_agg"}, errs=errs,
                                  stats=stats, owns=owns)
    worst = max(errs, key=errs.get)
    own_arm = {k: f"{owns[k]:.1e}" for k in errs if errs[k] > P.TOL}
    print(f"DTH_WS {_id(case)}: flips {flips} / {stats['mask_elems']}, worst err/scale {errs[worst]:.3e} on {worst}"
          + (f"; 2 x own arm: {own_arm}" if own_arm else ""))
    assert flips <= P.FLIP_CAP * stats["mask_elems"], f"{name}: {flips} ReLU decisions of {stats['mask_elems']} differ"


# ---------------------------------------------------------------------------------------
# which path ran: the library's own GEMM log
# ---------------------------------------------------------------------------------------
PATH_RUNS = [c for c in BASE_CASES if not c[3]] + SHAPE_CASES + [REFUSED] + list(WS_CASES)

PATH_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
import dstagnn_drought_amd as D
import test_gpu_parity as T
import test_gpu_cheb_dtheta as M
for name, first, B, train, hub in M.PATH_RUNS:
    N, Tn, K, h, Dm, dk, C = M.GEOM[name]
    ref, p, x, res, cheb, apa, dims, gen = T._oracle_case(B, N, Tn, K, h, Dm, dk, C, first, 0 if first else 1, seed=3,
                                                          hub=hub)
    F = x.shape[2]
    blk = D.DSTAGNN_block("cpu", F, F, K, C, C, 1, cheb, apa, apa, N, Tn, Dm, dk, dk, h)
    blk.load_state_dict(p)
    blk = blk.cuda().eval()
    xg = x.cuda().requires_grad_(True)
    rg = res.cuda().requires_grad_(True) if torch.is_tensor(res) else 0
    torch.cuda.synchronize()
    sys.stderr.write("[case] %s %d %d\\n" % (name, int(first), B)); sys.stderr.flush()
    out, re_at = blk(xg, rg)
    (out.sum() + re_at.sum()).backward()
    torch.cuda.synchronize()
print("LOG_OK")
"""


def _child(code, **env):
    e = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", **env)
    r = subprocess.run([sys.executable, "-c", code.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], cwd=ROOT,
                       env=e, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0 and "LOG_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stderr.splitlines()


def test_dtheta_gemm_only_where_refused():
    P._need_gpu()
    per, cur = {}, None
    for ln in _child(PATH_CHILD, DSTAGNN_GEMM_LOG="1"):
        if ln.startswith("[case] "):
            cur = ln[7:]
            per[cur] = []
        elif ln.startswith("[gemm]") and cur is not None:
            per[cur].append(ln)
    assert len(per) == len(PATH_RUNS), sorted(per)
    for name, first, B, _, _ in PATH_RUNS:
        N, T, K, _, _, _, C = GEOM[name]
        lines = per["%s %d %d" % (name, int(first), B)]
        assert lines, (name, "the block logged no GEMM")
        shape = "M=%d N=%d K=%d " % (K * (1 if first else C), C, B * N * T)  # dTheta[(k,f), c] over (b, j, t)
        hit = [ln for ln in lines if shape in ln]
        if (name, first, B) == REFUSED[:3] or WS_CASES.get((name, first, B, False, 0)) is False:
            assert len(hit) == 1, (name, shape, "the refused order / batch lost its dTheta GEMM", lines)
        else:
            assert not hit, (name, shape, "dTheta still runs as a GEMM", hit)


# ---------------------------------------------------------------------------------------
# the fold: the same bits every run
# ---------------------------------------------------------------------------------------
def _base_block(B, seed=3, first=False, train=False):
    import dstagnn_drought_amd as D
    N, T, K, h, Dm, dk, C = GEOM["dth_base"]
    ref, p, x, res, cheb, apa, dims, gen = _oracle_case(B, N, T, K, h, Dm, dk, C, first, 0 if first else 1, seed=seed)
    F = x.shape[2]
    blk = D.DSTAGNN_block("cpu", F, F, K, C, C, 1, cheb, apa, apa, N, T, Dm, dk, dk, h)
    blk.load_state_dict(p)
    g_out = torch.randn(B, N, C, T, generator=gen).cuda()
    g_re = torch.randn(B, F, h, T, T, generator=gen).cuda()
    return blk.cuda().train(train), x.cuda(), res.cuda() if torch.is_tensor(res) else res, g_out, g_re


def _fwd_bwd(blk, x, res, g_out, g_re):
    for p in blk.parameters():
        p.grad = None
    xg = x.clone().requires_grad_(True)
    if blk.training:
        torch.manual_seed(P.TRAIN_SEED)  # the forward draws its dropout seed from the global generator
    out, re_at = blk(xg, res)
    torch.autograd.backward([out, re_at], [g_out, g_re])
    torch.cuda.synchronize()
    r = {"out": out.detach().clone(), "re_at": re_at.detach().clone(), "grad_x": xg.grad.clone()}
    r.update({n: p.grad.clone() for n, p in blk.named_parameters() if p.grad is not None})
    return r


def _theta(r):
    th = {n: v for n, v in r.items() if "Theta" in n}
    assert th, sorted(r)
    return th


def test_theta_gradients_bit_identical_over_reruns():
    P._need_gpu()
    args = _base_block(3)
    first = _theta(_fwd_bwd(*args))
    for n, v in first.items():
        assert torch.isfinite(v).all() and float(v.abs().max()) > 0.0, n
    for rep in range(19):
        again = _theta(_fwd_bwd(*args))
        for n in first:
            assert torch.equal(first[n].view(torch.int32), again[n].view(torch.int32)), (n, "rerun", rep + 1)


# ---------------------------------------------------------------------------------------
# the slots the default path no longer has (agg_k; G with the fused GTU forward and backward)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,B", [(False, 3), (True, 2)], ids=["inner-B3", "first-B2"])
def test_dropped_save_slots_are_never_read(first, B):
    """The save buffer has no agg_k, G, E (inner block) or unused weight re-layout slot on this
    path: a run whose buffers start as NaN (block_fn._POISON) equals a plain run
    bit for bit and stays finite."""
    P._need_gpu()
    from dstagnn_drought_amd import block_fn
    args = _base_block(B, first=first)
    took = block_fn.block_paths(args[0], args[1].clone().requires_grad_(True), args[2])
    assert {"cheb_agg", "gtu_fused_fwd", "gtu_fused_bwd", "tat_fused_fwd", "tat_fused_bwd"} <= took, sorted(took)
    saved = block_fn._POISON
    try:
        block_fn._POISON = False
        plain = _fwd_bwd(*args)
        block_fn._POISON = True
        poisoned = _fwd_bwd(*args)
    finally:
        block_fn._POISON = saved
    assert plain.keys() == poisoned.keys()
    for k in plain:
        assert torch.isfinite(poisoned[k]).all(), f"{k}: NaN from a slot nothing wrote"
        assert torch.equal(plain[k], poisoned[k]), f"{k}: differs with poisoned buffers"


UNFUSED_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import torch
import test_gpu_parity as T
import test_gpu_cheb_dtheta as M
# G is still written and read: the whole case against the oracle, the fcmy weight gradient included
T._run_config_vs_oracle("dth_base", False, 3, paths=({{"cheb_agg", "gtu_fused_fwd"}}, {{"gtu_fused_bwd"}}))
r = M._fwd_bwd(*M._base_block(3))
np.savez({out!r}, **{{k: v.cpu().numpy() for k, v in r.items()}})
print("LOG_OK")
"""


def test_g_still_saved_for_the_unfused_backward(tmp_path):
    """DSTAGNN_GTU_FUSED_BWD=0 keeps the old G path: the child's run matches the oracle (its fcmy
    weight gradient is a GEMM over the stored G), and the forward outputs equal this process's
    (fused backward, G not stored) bit for bit.  Every gradient passes through the GTU stage's
    backward, where the two paths round differently, so the gradients of both are held to the
    oracle (test_block_vs_oracle here, _run_config_vs_oracle in the child), not to each other."""
    P._need_gpu()
    import numpy as np
    out = str(tmp_path / "unfused.npz")
    _child(UNFUSED_CHILD.replace("{out!r}", repr(out)), DSTAGNN_GTU_FUSED_BWD="0")
    child = dict(np.load(out))
    here = _fwd_bwd(*_base_block(3))
    assert set(child) == set(here)
    for k in ("out", "re_at"):
        assert np.array_equal(child[k].view(np.int32), here[k].cpu().numpy().view(np.int32)), k
