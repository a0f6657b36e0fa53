"""GPU: the forward-only block path (dstagnn_block_forward_only) gives the bits of the training
forward, per kernel family; calls that record no autograd node take it; it allocates one
workspace and nothing of the backward's.

SAVE = false instantiations the build contains, and the bit-identity rows that reach each
(default knobs):
  gtu_fwd_fused_kernel<false,false> / <true,false>      pems08 inner, n401, n520 inner / pems08, n520 first
  gtu_tail_fwd_ct_kernel<32,24,256,false|true,false>    t24 inner / first
  gtu_tail_fwd_kernel<true,0,kNT,false>                 t7, t13 (first and inner), t8h3, t16h3, k8t16, c16t12 (C = 16)
  gtu_tail_fwd_kernel<false,2,kSplitNT,false>           t144k3 (first and inner), k8t41; k3t32 at B = 66 (first and
                                                        inner: G in two node chunks through the GEMM workspace)
  tat_fused_fwd_kernel<8,1,8,false>                     t8h3
  tat_fused_fwd_kernel<12,1,8,false> / <12,3,8,false>   c16t12 (N = 40) / pems08 (N = 170)
  tat_fused_fwd_kernel<16,1,8,false>                    t16h3, k8t16
  cheb_agg_fwd2_kernel<NQ,KM,false>                     (6,3) pems08, n401, n520 inner; (1,3) pems08, n520, t7, t13 first;
                                                        (4,3) t8h3, t7 inner, c16t12; (8,3) t16h3, t13 inner; (8,8) k8t16
  cheb_agg_fwd_kernel<NQ,KM,false>                      (12,3) t24 inner; (1,3) t24, t144k3, k3t32 first; (16,3) k3t32 inner
  flash_small_fwd_kernel<1,false> / <2,..> / <4,..>     N <= 128 rows / pems08 / n401
  flash_psupp_kernel<false>                             n520 (the streamed pair)
  ln_fwd_* (scalar guard on mu / rs, u null)            every row (EmbedS); first rows (EmbedT); the unfused-TAt rows
                                                        (n401, n520, t24, t144k3, k8t41, t7, t13, k3t32)
  and, in the rows after k3t32: tat_fused_fwd_kernel<12,NTW,8,false> NTW = 2, 4, 5 (n101, n200, n320),
  flash_small_fwd_kernel<3,false> (n320), twelve more (NQ, KM) of cheb_agg_fwd2_kernel and four of
  cheb_agg_fwd_kernel (named there)
Not reached by a row: gtu_tail_fwd_ct_kernel<32,12,256,*,false> (runs only with the fused GTU
forward switched off by its knob), the 4-wave tat_fused forms (DSTAGNN_TF_WAVES=4), the fused TAt
at T = 8 / 16 with NTW > 1, and of the (NQ, KM) pairs an F = 1 or F = C geometry admits
(tests/test_parity_coverage_cpu.py enumerates them) only cheb_agg_fwd_kernel<12, 5, false> (C = 32 at
T in 17..24 with K = 4 or 5: no geometry of test_gpu_parity.CONFIGS).  The last rows reach
cheb_agg_fwd_kernel<8, KM> and <6, KM> and cheb_agg_fwd2_kernel<2, KM> at every KM (C = 16 inner blocks
at T = 25, 17 | 24 and 8), then <1, 2 | 5 | 8> and <16, 2> of cheb_agg_fwd_kernel and fwd2<4, 5>.  The forms
only a multi-feature first block admits (cheb_agg_fwd_kernel<4, KM>, <2, 5>, <2, 8>) have their
bit-identity rows in test_gpu_multifeature (test_no_grad_forward_has_the_training_forward_bits).
"""
import json

import numpy as np
import pytest
import torch

import test_gpu_parity as tp

pytestmark = pytest.mark.gpu

_FS = {"sparse", "flash", "flash_small"}
# (name, first, B, knobs, must, must_not)
CASES = [
    ("pems08", False, 3, {}, _FS | {"tat_fused_fwd", "cheb_agg", "gtu_fused_fwd"}, set()),
    ("pems08", True, 2, {}, _FS | {"tat_fused_fwd", "cheb_agg", "gtu_fused_fwd"}, set()),
    ("t8h3", False, 2, {}, {"tat_fused_fwd"}, set()),
    ("t16h3", False, 2, {}, {"tat_fused_fwd"}, set()),
    ("n401", False, 2, {}, _FS, set()),
    ("n520", False, 2, {}, {"sparse", "flash"}, {"flash_small"}),
    ("n520", True, 1, {}, {"sparse", "flash"}, {"flash_small"}),
    ("pems08", False, 2, {"flash": False}, {"sparse"}, {"flash"}),
    ("pems08", False, 2, {"sparse": False}, set(), {"sparse", "flash"}),
    ("t24", False, 2, {}, {"cheb_agg"}, {"tat_fused_fwd", "gtu_fused_fwd"}),
    ("t24", True, 1, {}, {"cheb_agg"}, {"tat_fused_fwd", "gtu_fused_fwd"}),
    ("t144k3", False, 1, {}, {"sparse"}, {"cheb_agg", "gtu_fused_fwd"}),
    ("t144k3", True, 1, {}, {"sparse"}, {"gtu_fused_fwd"}),
    ("k8t41", False, 2, {}, {"sparse"}, {"cheb_agg"}),
    ("t7", False, 3, {}, set(), {"tat_fused_fwd", "gtu_fused_fwd"}),
    ("t7", True, 2, {}, set(), {"tat_fused_fwd", "gtu_fused_fwd"}),
    ("t13", False, 3, {}, set(), {"tat_fused_fwd", "gtu_fused_fwd"}),
    ("t13", True, 2, {}, set(), {"tat_fused_fwd", "gtu_fused_fwd"}),
    ("c16t12", False, 3, {}, {"cheb_agg"}, {"gtu_fused_fwd"}),
    ("k8t16", False, 3, {}, {"cheb_agg", "tat_fused_fwd"}, set()),
    # the split tail's G goes through the 8M-float GEMM workspace: 3120 nodes of C (3T - 12) =
    # 2688 floats fit, B N = 66 * 48 = 3168 nodes take two chunks (the second 48 nodes)
    ("k3t32", False, 66, {}, {"cheb_agg"}, {"gtu_fused_fwd"}),
    ("k3t32", True, 66, {}, {"cheb_agg"}, {"gtu_fused_fwd"}),
    # further values of the same templates, at the geometries test_gpu_parity pins them with:
    # fused TAt at NTW = 2, 4, 5 (n320 also flash_small_fwd<3>)
    ("n101", False, 2, {}, _FS | {"tat_fused_fwd"}, set()),
    ("n200", False, 2, {}, _FS | {"tat_fused_fwd"}, set()),
    ("n320", False, 2, {}, _FS | {"tat_fused_fwd"}, set()),
    # cheb_agg_fwd2 (NQ, KM): (6,2) (6,5) (8,5) (8,2) (4,8) (4,2) (6,8) (2,8), first blocks (1,2) (1,5) (1,8)
    ("k1t12", False, 2, {}, {"cheb_agg"}, set()), ("k4t12", False, 2, {}, {"cheb_agg"}, set()),
    ("k5t16", False, 2, {}, {"cheb_agg"}, set()), ("k2t16", False, 2, {}, {"cheb_agg"}, set()),
    ("k6t8", False, 2, {}, {"cheb_agg"}, set()), ("k2t8", False, 2, {}, {"cheb_agg"}, set()),
    ("k8t12", False, 2, {}, {"cheb_agg"}, set()), ("c16k8t8", False, 2, {}, {"cheb_agg"}, set()),
    ("k2t12", True, 2, {}, {"cheb_agg"}, set()), ("k5t8", True, 2, {}, {"cheb_agg"}, set()),
    ("k8t16", True, 2, {}, {"cheb_agg"}, set()),
    # cheb_agg_fwd (NQ, KM): (12,8) (12,2) (16,5) (16,8); k4t48 and k8t40 also the split tail
    ("k8t24", False, 2, {}, {"cheb_agg"}, set()), ("k2t24", False, 2, {}, {"cheb_agg"}, set()),
    ("k4t48", False, 2, {}, {"cheb_agg"}, set()), ("k8t40", False, 2, {}, {"cheb_agg"}, set()),
    # C = 16 inner: cheb_agg_fwd (8, KM) at T = 25 and (6, KM) at T = 17 / 24, cheb_agg_fwd2 (2, KM) at T = 8
    # (KM = 8: c16k8t8 above), every order template; T >= 20 also the split tail at C = 16
] + [(n, False, 2, {}, {"cheb_agg"}, {"gtu_fused_fwd"}) for n in (
    "c16k2t25", "c16t25", "c16k5t25", "c16k8t25", "c16k2t17", "c16t24", "c16k5t17", "c16k8t17", "c16k2t8", "c16t8",
    "c16k5t8")] + [
    # cheb_agg_fwd (1, 2) (1, 5) (1, 8): first blocks at T > 16; (16, 2); cheb_agg_fwd2 (4, 5)
    ("k2t24", True, 1, {}, {"cheb_agg"}, set()), ("k4t48", True, 1, {}, {"cheb_agg"}, set()),
    ("k8t24", True, 1, {}, {"cheb_agg"}, set()), ("t63", False, 2, {}, {"cheb_agg"}, set()),
    ("k5t8", False, 2, {}, {"cheb_agg"}, set())]


def _case_id(c):
    return f"{c[0]}-{'first' if c[1] else 'inner'}-B{c[2]}" + "".join(f"-{k}={v}" for k, v in c[3].items())


def _block(name, first, B, seed=5, knobs=None):
    import dstagnn_drought_amd as D_
    N, T, K, h, D, dk, C = tp.CONFIGS[name]
    _, p, x, res, cheb, apa, _, _ = tp._oracle_case(B, N, T, K, h, D, dk, C, first, 0 if first else 1, seed=seed)
    F = x.shape[2]
    blk = D_.DSTAGNN_block("cpu", F, F, K, C, C, 1, cheb, apa, apa, N, T, D, dk, dk, h)
    blk.load_state_dict(p)
    blk = blk.cuda().eval()
    for k, v in (knobs or {}).items():
        setattr(blk, {"flash": "flash_cheb", "sparse": "sparse_cheb"}[k], v)
    return blk, x.cuda(), (res.cuda() if torch.is_tensor(res) else 0)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_bit_identity(case, train):
    """block_fwd_only == block_fwd's (out, re_at), bit for bit, both over NaN-poisoned buffers."""
    tp._need_gpu()
    from dstagnn_drought_amd import _lib, block_fn as bf
    name, first, B, knobs, must, must_not = case
    blk, x, res = _block(name, first, B, knobs=knobs)
    took = bf.block_paths(blk, x, res, train=train)
    assert must <= took and not (must_not & took), f"{name}: kernel path {sorted(took)}, expected {sorted(must)} " \
                                                   f"and none of {sorted(must_not)}"
    seed = tp._train_seed() if train else 0
    args = bf._explicit_args(blk, x, res, train=train, seed=seed, poison=True)
    ops = _lib.load()
    out_f, re_f, _save = ops.block_fwd(*args)
    out_l, re_l = ops.block_fwd_only(*args)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out_f).all()) and bool(torch.isfinite(re_f).all())
    assert torch.equal(re_l, re_f), f"re_at differs: max |d| {float((re_l - re_f).abs().max()):.3e}"
    assert torch.equal(out_l, out_f), f"out differs: max |d| {float((out_l - out_f).abs().max()):.3e}"


def test_dispatch_takes_the_lean_path_where_no_node_is_recorded():
    tp._need_gpu()
    blk, x, res = _block("pems08", False, 2)
    xg = x.clone().requires_grad_(True)
    out_g, re_g = blk(xg, res)
    assert out_g.requires_grad and out_g.grad_fn is not None
    results = {}
    with torch.no_grad():
        results["no_grad"] = blk(x, res)
    with torch.inference_mode():
        results["inference_mode"] = blk(x, res)
    for p in blk.parameters():
        p.requires_grad_(False)
    results["nothing requires grad"] = blk(x, res)
    blk.forward_only = False
    with torch.no_grad():
        results["forward_only=False"] = blk(x, res)
    for what, (out, re_at) in results.items():
        assert not out.requires_grad and not re_at.requires_grad, what
        assert torch.equal(out, out_g) and torch.equal(re_at, re_g), what


def test_no_grad_call_allocates_one_workspace():
    """Peak allocation of a no-grad call <= workspace + outputs + 8 MiB of allocator rounding
    (the full forward allocates save + scratch: over 400 MB here)."""
    tp._need_gpu()
    from dstagnn_drought_amd import block_fn as bf
    blk, x, res = _block("pems08", False, 32)
    with torch.no_grad():
        blk(x, res)  # graph index data, plan caches
    wb = bf.forward_only_bytes(blk, x, res)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        out, re_at = blk(x, res)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    bound = wb + out.numel() * 4 + re_at.numel() * 4 + (8 << 20)
    print(f"peak {peak} bound {bound} workspace {wb}")
    assert peak <= bound, (peak, bound)


def _model(golden_dir):
    import dstagnn_drought_amd as D
    g = tp.load(golden_dir, "g4_model.npz")
    m = json.loads(str(g["meta"]))
    torch.manual_seed(0)
    model = D.make_model("cpu", 1, 2, 1, m["K"], m["C"], m["C"], 1, torch.FloatTensor(g["adj_tmd"]),
                         torch.FloatTensor(g["adj_pa"]), torch.FloatTensor(g["adj_tmd"]), m["num_for_predict"],
                         m["T"], m["N"], m["D"], m["d_k"], m["d_k"], m["n_heads"])
    cheb = torch.from_numpy(np.stack([g[f"cheb_{k}"] for k in range(m["K"])]))
    for b in model.BlockList:  # (make_model's ARPACK lambda_max depends on the calls before it)
        b.cheb_conv_SAt.cheb_stack.copy_(cheb)
    x = torch.from_numpy(np.asarray(g["x"])).cuda()
    y = torch.from_numpy(np.asarray(g["target"])).cuda()
    return model.cuda(), x, y


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_model_no_grad_equals_grad_mode(golden_dir, train):
    tp._need_gpu()
    model, x, _ = _model(golden_dir)
    model.train(train)
    torch.manual_seed(77)
    ref = model(x)
    assert ref.requires_grad
    torch.manual_seed(77)
    with torch.no_grad():
        out = model(x)
    assert not out.requires_grad
    assert torch.equal(out, ref)


@pytest.mark.parametrize("direct", [False, True], ids=["autograd", "direct"])
def test_training_step_after_no_grad_call(golden_dir, direct):
    """The same training step with and without a no-grad call before it: equal gradients — the
    forward-only call leaves the cached BlockPlan (direct-gradient mode) as it was."""
    tp._need_gpu()
    import dstagnn_drought_amd as D
    model, x, y = _model(golden_dir)
    D.set_direct_grads(model, direct)
    model.train()

    def step(seed):
        model.zero_grad(set_to_none=True)
        torch.manual_seed(seed)
        torch.nn.SmoothL1Loss()(model(x), y).backward()
        return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    step(1)  # builds the plan caches
    g0 = step(2)
    with torch.no_grad():
        model(x)
    g1 = step(2)
    assert g0.keys() == g1.keys() and len(g0) > 10
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_eval_batches_value(golden_dir):
    tp._need_gpu()
    import dstagnn_drought_amd as D
    from dstagnn_drought_amd import train
    model, x, y = _model(golden_dir)
    model.eval()
    xs, ys = torch.cat([x, x.flip(0), x]), torch.cat([y, y.flip(0), y])
    crit = torch.nn.SmoothL1Loss()
    lean = train.eval_batches(model, xs, ys, x.shape[0], crit)
    for b in model.BlockList:
        b.forward_only = False
    full = train.eval_batches(model, xs, ys, x.shape[0], crit)
    assert D.DSTAGNN_block.forward_only is True
    assert lean == full, (lean, full)
