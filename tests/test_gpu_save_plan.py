"""The save arena's plan (block.hip plan_bufs) on the device, at dth_base =
(N 40, T 12, K 3, h 3, D 64, d_k 32, C 32): the smallest geometry that takes the fused TAt forward
and backward, the fused GTU forward and backward, the aggregate-first order and the in-kernel dTheta
at once, so the inner block (B = 3) drops every slot the plan can drop and the first block (B = 2)
all of them but E.

1. Kept slots: each switch that takes a block off one of those paths, in a child process of its own
   (the knobs are read once per process) whose buffers start as NaN (DSTAGNN_POISON=1), runs the
   inner block in train mode and the first block against the fp64 oracle at the suite's bound
   (test_gpu_parity._run_config_vs_oracle).  These are the paths on which a slot must STAY: one
   dropped too eagerly is a null or NaN operand here.
2. Bit identity: on the default path every output and gradient equals the bytes the parent build
   produced (tests/golden/save_plan_parent_hashes.json, tools/record_save_plan.py).  The dropped
   slots are neither written nor read there, so nothing may move.  (The poisoned-run test of the
   dropped slots themselves is test_gpu_cheb_dtheta.test_dropped_save_slots_are_never_read.)
"""
import hashlib
import json
import os

import pytest

import test_gpu_cheb_dtheta as M
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# switch -> (paths the child must take, paths it must not): what the switch turns off and nothing else
SWITCHES = {
    "DSTAGNN_GTU_FUSED": ({"gtu_fused_bwd", "tat_fused_fwd", "tat_fused_bwd", "cheb_agg"}, {"gtu_fused_fwd"}),
    "DSTAGNN_GTU_FUSED_BWD": ({"gtu_fused_fwd", "tat_fused_fwd", "tat_fused_bwd", "cheb_agg"}, {"gtu_fused_bwd"}),
    "DSTAGNN_TAT_FUSED": ({"gtu_fused_fwd", "gtu_fused_bwd", "cheb_agg"}, {"tat_fused_fwd", "tat_fused_bwd"}),
    "DSTAGNN_TAT_FUSED_BWD": ({"gtu_fused_fwd", "gtu_fused_bwd", "tat_fused_fwd", "cheb_agg"}, {"tat_fused_bwd"}),
    "DSTAGNN_CHEB_AGG": ({"gtu_fused_fwd", "gtu_fused_bwd", "tat_fused_fwd", "tat_fused_bwd"}, {"cheb_agg"}),
    # (the in-kernel dTheta has no path bit: without the sample-pair kernels the aggregates are stored
    # and dTheta is a GEMM over them again, on the aggregate-first path)
    "DSTAGNN_AGG_PAIR": ({"gtu_fused_fwd", "gtu_fused_bwd", "tat_fused_fwd", "tat_fused_bwd", "cheb_agg"}, set()),
}

KEPT_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_gpu_parity as T
import test_gpu_cheb_dtheta as M
from dstagnn_drought_amd import block_fn
assert block_fn._POISON
paths = (MUST, MUST_NOT)
T._run_config_vs_oracle("dth_base", False, 3, train=True, paths=paths)
T._run_config_vs_oracle("dth_base", True, 2, paths=paths)
print("LOG_OK")
"""


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_kept_slots_hold_what_the_other_paths_read(switch):
    P._need_gpu()
    must, must_not = SWITCHES[switch]
    code = KEPT_CHILD.replace("MUST_NOT", "set(%r)" % sorted(must_not)).replace("MUST", "set(%r)" % sorted(must))
    M._child(code, DSTAGNN_POISON="1", **{switch: "0"})


# ---------------------------------------------------------------------------------------
# the default path: the parent build's bytes
# ---------------------------------------------------------------------------------------
BIT_CASES = [(False, 3, True), (True, 2, False)]  # (first, B, train)


def case_id(first, B, train):
    return "%s-B%d-%s" % ("first" if first else "inner", B, "train" if train else "eval")


def run_case(first, B, train):
    """{name: tensor} of out, re_at, grad_x and every parameter gradient of a fresh dth_base block."""
    return M._fwd_bwd(*M._base_block(B, first=first, train=train))


@pytest.mark.parametrize("case", BIT_CASES, ids=lambda c: case_id(*c))
def test_default_path_bit_identical_to_parent(case):
    """Every tensor the parent build reproduced over two runs of its own is held to its sha256; one
    it did not reproduce is listed in the fixture without a hash and is held to the oracle by
    test_gpu_cheb_dtheta.test_block_vs_oracle's dth_base rows instead."""
    P._need_gpu()
    from dstagnn_drought_amd import block_fn
    with open(os.path.join(ROOT, "tests", "golden", "save_plan_parent_hashes.json")) as f:
        rec = json.load(f)
    want, loose = rec["cases"][case_id(*case)], rec["unreproducible"][case_id(*case)]
    first, B, train = case
    args = M._base_block(B, first=first, train=train)
    took = block_fn.block_paths(args[0], args[1].clone().requires_grad_(True), args[2], train=train)
    assert {"cheb_agg", "gtu_fused_fwd", "gtu_fused_bwd", "tat_fused_fwd", "tat_fused_bwd"} <= took, sorted(took)
    got = M._fwd_bwd(*args)
    assert set(got) == set(want) | set(loose), sorted(set(got) ^ (set(want) | set(loose)))
    bad = [k for k in want
           if hashlib.sha256(got[k].cpu().contiguous().numpy().tobytes()).hexdigest() != want[k]]
    assert not bad, f"{case_id(*case)}: differ from the parent build's bytes: {bad}"
