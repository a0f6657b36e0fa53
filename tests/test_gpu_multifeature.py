"""GPU: the multi-feature first block and the multi-feature model against the fp64 helper
(tests/multifeature_ref.py: the unchanged oracle functions, the three first-block branches keyed
on "first block"), at test_gpu_parity's bound 1e-4 * max(1, max|ref|) with its ReLU-aware
procedure and RELU_EPS.  A tensor past that bound may only pass on the arm
_run_config_vs_oracle already has, twice the fp32 restatement's own error against fp64; every
case prints which tensors needed it (NEEDED_FP32_ARM collects them).
Measured on an MI355X: no tensor of any case needed that arm (errors 3e-8 ... 3e-6 of the
scale over all block and model cases); no ReLU decision of a block case fell within rounding of 0.

Shapes (the smallest that reach each first-block path at F > 1):
  A  C=32 T=12 h=3 d_k=32 D=64 K=3 N=37 B=3 F=4  fused TAt (N no multiple of 16), aggregate-first
     Chebyshev sample pairs with an odd B, the C = 32 / T = 12 tail -> the runtime-generic MF tail
     (never gtu_fused, never the compile-time tail);  A at F = 2, 3, 8: an odd F and the limit
  B  C=8 T=9 h=2 d_k=8 D=16 K=2 N=20 B=2 F=4     generic MF tail, unfused TAt, Theta-first, odd T
  C  C=32 T=24 N=16 B=2 F=4                        T = 24: the split path instead of the ct24 template
  D  C=32 T=144 h=2 D=64 K=2 N=12 B=1 F=4          the split long-series path (GAMBIA in small)
and the rows of MF_DISPATCH below: the aggregate-first templates only a multi-feature first block
admits, the MF = true tail forms off "generic c32 / cx" and "split c32", and EmbedT's LayerNorm over
B F T rows past one value a lane (tests/kernel_coverage.py names each row's templates;
tests/test_parity_coverage_cpu.py holds BLOCK_CASES to what the gates admit).
"""
import functools
import os

import numpy as np
import pytest
import torch

import kernel_coverage as kc
import multifeature_ref as mfr
import test_gpu_parity as tp

pytestmark = pytest.mark.gpu

NEEDED_FP32_ARM = []  # (case, tensor) pairs that passed only on the fp32-restatement arm


@pytest.fixture(autouse=True)
def _no_arpack_draws(monkeypatch):
    """make_model's scaled_Laplacian asks ARPACK for lambda_max with a start vector drawn from
    ARPACK's own generator, whose state lives as long as the process: a model built here would
    move the Chebyshev polynomials of every test that runs later by ~1e-6.  These tests take the
    exact dense eigenvalue instead and leave that state alone."""
    import scipy.sparse.linalg as sla

    def eigs(A, k=1, which="LR", **kw):
        ev = np.linalg.eigvals(np.asarray(A))
        return ev[np.argsort(-ev.real)[:k]], None
    monkeypatch.setattr(sla, "eigs", eigs)

#        N,  T,  K, h, D,  dk, C,  B
SHAPES = {"A": (37, 12, 3, 3, 64, 32, 32, 3), "B": (20, 9, 2, 2, 16, 8, 8, 2), "C": (16, 24, 3, 3, 64, 32, 32, 2),
          "D": (12, 144, 2, 2, 64, 32, 32, 1)}
# name: (shape row, F, what only this row reaches).  N = 40, D = 64, d_k = 32, B = 2 unless the comment says otherwise.
MF_DISPATCH = {
    # C = 16, T = 17, F = 8: rows of 8 * 17 = 136 floats on the single-sample kernels, cheb_agg_fwd_kernel<4, KM>
    # and cheb_agg_sddmm_kernel<4, KM> at every order template (no F = 1 or F = C geometry gives NQ = 4
    # there); the generic MF tail at C = 16
    "c16t17k2": ((40, 17, 2, 2, 64, 32, 16, 2), 8), "c16t17k3": ((40, 17, 3, 2, 64, 32, 16, 2), 8),
    "c16t17k5": ((40, 17, 5, 2, 64, 32, 16, 2), 8), "c16t17k8": ((40, 17, 8, 2, 64, 32, 16, 2), 8),
    # C = 32, T = 24, F = 4: rows of 96 floats, fwd / sddmm <2, 5> (K = 4 < KM) and <2, 8> (K = 6 < KM)
    "t24k4": ((40, 24, 4, 2, 64, 32, 32, 2), 4), "t24k6": ((40, 24, 6, 2, 64, 32, 32, 2), 4),
    # the split MF tail at C = 16 (T >= 20) and at a C off {16, 32} (Theta-first Chebyshev, K-concatenated dx)
    "c16t24": ((40, 24, 3, 2, 64, 32, 16, 2), 8), "c8t20": ((40, 20, 3, 2, 64, 32, 8, 2), 4),
    # the two tail gates disagree (F = 1 layout: forward 28 172 B, backward 33 236 B > 32 KB): the generic
    # MF forward's saved state feeds the split MF backward
    "c72t19": ((40, 19, 3, 2, 64, 32, 72, 2), 4),
    # F T = 21: rows no multiple of 4 floats at the minimum T, an odd F, h = 3 (T = 7: the G = 64 VALU TAt)
    "t7f3": ((40, 7, 3, 3, 64, 32, 32, 2), 3),
    # EmbedT / TAt LayerNorm over B F T rows of N floats read with element stride F T (h = 2: the fused TAt
    # refuses, the matrix-core TAt runs B F problems): VPT<2>; the float4 backward (EmbedT) and both float4
    # directions (TAt); B = 1, N = 1030: the workgroup-per-row kernels with the contribution-form backward
    "n100": ((100, 12, 3, 2, 64, 32, 32, 2), 4), "n256": ((256, 12, 3, 2, 64, 32, 32, 2), 4),
    "n1030": ((1030, 12, 3, 2, 64, 32, 32, 1), 4),
}
SHAPES.update({k: v[0] for k, v in MF_DISPATCH.items()})


def d64(t):
    return t.double() if torch.is_tensor(t) else t


@functools.lru_cache(maxsize=None)
def _graph(N, K, seed):
    import dstagnn_drought_amd as D_
    rs = np.random.RandomState(seed)
    tmd, pa = np.eye(N), np.zeros((N, N))
    for i in range(N):
        tmd[i, rs.choice(N, 2, replace=False)] = 1.0
        pa[i, rs.choice(N, 4, replace=False)] = 1.0
    Lt = tp._scaled_laplacian_fixed_start(tmd)
    cheb = [torch.from_numpy(c).float() for c in D_.cheb_polynomial(Lt, K)][:K]
    return cheb, torch.from_numpy(pa).float(), torch.from_numpy(tmd).float()


@functools.lru_cache(maxsize=None)
def _case(shape, F, seed=3):
    """Inputs of a block case, made once and shared (never modified): parameters, x, upstream grads."""
    N, T, K, h, D, dk, C, B = SHAPES[shape]
    gen = torch.Generator().manual_seed(seed)
    cheb, apa, _ = _graph(N, K, seed)
    p = mfr.random_block_params(gen, F, K, C, N, T, D, dk, dk, h)
    x = torch.randn(B, N, F, T, generator=gen)
    g_out = torch.randn(B, N, C, T, generator=gen)
    g_re = torch.randn(B, F, h, T, T, generator=gen)
    return p, x, g_out, g_re, cheb, apa, dict(n_heads=h, d_k=dk, d_v=dk, K=K)


def _block(shape, F, p=None, multi_feature=True, train=False, sparse=True):
    import dstagnn_drought_amd as D_
    N, T, K, h, D, dk, C, B = SHAPES[shape]
    cheb, apa, _ = _graph(N, K, 3)
    kw = {"multi_feature": True} if multi_feature else {}
    blk = D_.DSTAGNN_block("cpu", F, F, K, C, C, 1, cheb, apa, apa, N, T, D, dk, dk, h, **kw)
    if p is not None:
        blk.load_state_dict(p)
    blk = blk.cuda().train(train)
    blk.sparse_cheb = sparse
    return blk


def hip_relu_masks(blk, x, res, train=False, seed=0):
    """test_gpu_parity.hip_relu_masks with the block's own flags (the first-block flag included)."""
    from dstagnn_drought_amd import _lib, block_fn as bf
    args = bf._explicit_args(blk, x, res, train=train, seed=seed)
    ops = _lib.load()
    X, tco, r = (ops.block_relu_out(*args, w) for w in (0, 1, 2))
    return ((X > 0).permute(0, 1, 3, 2).contiguous().cpu(), (tco > 0).permute(0, 2, 1, 3).contiguous().cpu(),
            (r > 0).permute(0, 2, 1, 3).contiguous().cpu())


def predicted(shape, F, sparse=True, train=False):
    """The dispatch mirror's tokens for a multi-feature first block of this shape (res_att = 0)."""
    N, T, K, h, D, dk, C, B = SHAPES[shape]
    return kc.kernels(N, T, K, F, C, B, sparse=sparse, d_k=dk, h=h, D=D, first=True, res_kind=0, train=train)


def expected_paths(shape, F, sparse=True):
    """(must, must_not): the multi-feature tail always; the rest from the dispatch mirror's tokens."""
    fam = {f for f, _ in predicted(shape, F, sparse)}
    assert not fam & {"gtu_fused_fwd", "gtu_fused_bwd", "tat_fused_fwd", "tat_fused_bwd"}, sorted(fam)  # the F = 1 | C names
    must, must_not = {"first_multi"}, {"gtu_fused_fwd", "gtu_fused_bwd"}
    (must if fam & {"fwd", "fwd2"} else must_not).add("cheb_agg")
    (must if "tat_fused_fwd_mf" in fam else must_not).add("tat_fused_fwd")
    (must if "tat_fused_bwd_mf" in fam else must_not).add("tat_fused_bwd")
    (must if sparse else must_not).add("sparse")
    assert sparse == bool(fam & {"fwd", "fwd2", "theta_first"})
    return must, must_not


def _close(case, key, got, want64, want32, tol=tp.TOL):
    """close()'s bound; past it only twice the fp32 restatement's own error (recorded)."""
    want64 = want64.double()
    scale = max(1.0, float(want64.abs().max()))
    d = got.detach().double().cpu()
    assert d.shape == want64.shape, (case, key, d.shape, want64.shape)
    err = float((d - want64).abs().max())
    own = float((want32.double() - want64).abs().max())
    print(f"{case} {key}: err {err / scale:.3e} (fp32 restatement's own {own / scale:.3e})")
    if err > tol * scale:
        NEEDED_FP32_ARM.append((case, key))
        print(f"{case} {key}: past 1e-4, held to twice the fp32 restatement's own error")
    assert err <= max(tol * scale, 2.0 * own), \
        f"{case} {key}: max err {err:.3e} > {tol:.0e} * {scale:.3e} and > 2 x fp32 own {own:.3e}"


def _run_block_case(shape, F, sparse=True, train=False, flip_cap=False):
    from dstagnn_drought_amd.block_fn import block_paths, dropout_masks
    case = f"{shape}/F{F}" + ("" if sparse else "/dense") + ("/train" if train else "")
    p, x, g_out, g_re, cheb, apa, dims = _case(shape, F)
    blk = _block(shape, F, p, train=train, sparse=sparse)
    xg = x.cuda().requires_grad_(True)
    must, must_not = expected_paths(shape, F, sparse)
    took = block_paths(blk, xg, 0, train=train)
    assert must <= took and not (must_not & took), f"{case}: kernel path {sorted(took)}, expected {sorted(must)} " \
                                                   f"and none of {sorted(must_not)}"
    dseed, dm = 0, None
    if train:
        dseed = tp._train_seed()
        m0, m1 = dropout_masks(blk.meta, x.shape, dseed)
        keep = float((m1 > 0).float().mean())
        assert 0.93 < keep < 0.97, keep
        dm = (m0.cpu(), m1.cpu().permute(0, 2, 1, 3).contiguous())
    masks = hip_relu_masks(blk, xg, 0, train=train, seed=dseed)
    flips = tp.relu_aware_mask(mfr, p, x, 0, cheb, apa, dims, masks, case, eps=tp.RELU_EPS, drop_masks=dm)
    elems = sum(int(m.numel()) for m in masks)
    kw = dict(relu_mask=masks[0], tail_masks=masks[1:], train=train)
    r64 = mfr.block_forward_backward({k: d64(v) for k, v in p.items()}, d64(x), 0, [d64(c) for c in cheb], d64(apa),
                                     dims, d64(g_out), d64(g_re), drop_masks=None if dm is None else tuple(map(d64, dm)),
                                     **kw)
    r32 = mfr.block_forward_backward(p, x, 0, cheb, apa, dims, g_out, g_re, drop_masks=dm, **kw)
    if train:
        torch.manual_seed(tp.TRAIN_SEED)  # the forward draws dseed again
    out, re_at = blk(xg, 0)
    assert re_at.shape == (x.shape[0], F, dims["n_heads"], x.shape[3], x.shape[3])
    _close(case, "out", out, r64[0], r32[0])
    _close(case, "re_At", re_at, r64[1], r32[1])
    ((out * g_out.cuda()).sum() + (re_at * g_re.cuda()).sum()).backward()
    assert xg.grad.shape == x.shape
    _close(case, "dx", xg.grad, r64[2], r32[2])
    for n, prm in blk.named_parameters():
        assert r64[4][n] is not None and prm.grad is not None, f"{case}: {n} has no gradient"
        assert prm.grad.shape == prm.shape
        _close(case, n, prm.grad, r64[4][n], r32[4][n])
    print(f"{case}: {flips} / {elems} ReLU decisions within rounding of 0; fp32 arm so far: {NEEDED_FP32_ARM}")
    if flip_cap:  # test_gpu_parity.test_pinned_templates_vs_oracle's cap, for the MF_DISPATCH rows
        print(f"{case}: kernels {sorted(kc.dispatch_only(predicted(shape, F, sparse, train)))}")
        assert flips <= tp.FLIP_CAP * elems, f"{case}: {flips} ReLU decisions of {elems} differ"
    return out.detach()


BLOCK_CASES = [("A", 4), ("A", 2), ("A", 3), ("A", 8), ("B", 4), ("C", 4), ("D", 4)]


@pytest.mark.parametrize("shape,F", BLOCK_CASES, ids=[f"{s}-F{f}" for s, f in BLOCK_CASES])
def test_block_vs_fp64_helper(shape, F):
    tp._need_gpu()
    _run_block_case(shape, F)


# (shape, F, train): every MF_DISPATCH row in eval mode; train where the dropout rides in a tail form no
# other row runs it in — the (generic forward, split backward) pairing and the split form.
#
# FLIP_CAP's condition, checked on the CPU for every row (seed 3): the fp32 restatement against the fp64 one
# flips 0 of the 38 400 .. 1 186 560 ReLU decisions of each row.
# Measured on the MI355X (worst err / scale over all tensors; every row 0 flips, none on the fp32 arm):
#   c16t17 K = 2 6.0e-7  K = 3 6.6e-7  K = 5 7.2e-7  K = 8 9.4e-7    t24k4 7.5e-7  t24k6 6.8e-7
#   c16t24 6.5e-7  c8t20 7.4e-7  c72t19 8.7e-7 (train 6.5e-7)  C train 8.6e-7  t7f3 2.3e-6
#   n100 7.2e-7  n256 8.4e-7  n1030 5.7e-7
MF_DISPATCH_CASES = [(n, MF_DISPATCH[n][1], False) for n in MF_DISPATCH] + [("c72t19", 4, True), ("C", 4, True)]


@pytest.mark.parametrize("shape,F,train", MF_DISPATCH_CASES,
                         ids=[f"{s}-F{f}" + ("-train" if t else "") for s, f, t in MF_DISPATCH_CASES])
def test_block_dispatch_rows_vs_fp64_helper(shape, F, train):
    """The rows of MF_DISPATCH at the bound and procedure of test_block_vs_fp64_helper, path bits (from the
    extended mirror) asserted first, and test_gpu_parity.FLIP_CAP on the decisions that differ."""
    tp._need_gpu()
    _run_block_case(shape, F, train=train, flip_cap=True)


def test_block_dense_cheb_vs_fp64_helper():
    tp._need_gpu()
    _run_block_case("A", 4, sparse=False)


def test_block_train_mode_vs_fp64_helper():
    """Both dropout sites on; the helper gets the keep-masks the HIP forward draws (dropout_masks)."""
    tp._need_gpu()
    _run_block_case("A", 4, train=True)


@pytest.mark.parametrize("shape", ["A", "D", "c16t17k2", "c16t17k3", "c16t17k5", "c16t17k8", "t24k4", "t24k6"])
def test_no_grad_forward_has_the_training_forward_bits(shape):
    """torch.no_grad() takes dstagnn_block_forward_only (lean plan, SAVE = false kernel forms; the
    MF_DISPATCH rows: cheb_agg_fwd_kernel<4, KM, false> and <2, 5 | 8, false>, which no other block admits)."""
    tp._need_gpu()
    from dstagnn_drought_amd import _lib, block_fn as bf
    F = MF_DISPATCH[shape][1] if shape in MF_DISPATCH else 4
    p, x, *_ = _case(shape, F)
    blk = _block(shape, F, p)
    xg = x.cuda().requires_grad_(True)
    out, re_at = blk(xg, 0)
    assert out.grad_fn is not None
    with torch.no_grad():
        o2, r2 = blk(x.cuda(), 0)
    assert o2.grad_fn is None
    assert torch.equal(out.detach(), o2) and torch.equal(re_at.detach(), r2)
    o3, r3 = _lib.load().block_fwd_only(*bf._explicit_args(blk, x.cuda(), 0))
    assert torch.equal(out.detach(), o3) and torch.equal(re_at.detach(), r3)
    assert bf.forward_only_bytes(blk, x.cuda(), 0) > 0


@pytest.mark.parametrize("shape", ["A", "B"])
def test_switch_with_one_feature_is_the_default_first_block(shape):
    """multi_feature=True at F = 1: the same kernels, so the same bits, outputs and gradients."""
    tp._need_gpu()
    from dstagnn_drought_amd.block_fn import block_paths
    p, x, g_out, g_re, *_ = _case(shape, 1)
    got = []
    for mf in (False, True):
        blk = _block(shape, 1, p, multi_feature=mf)
        xg = x.cuda().requires_grad_(True)
        out, re_at = blk(xg, 0)
        ((out * g_out.cuda()).sum() + (re_at * g_re.cuda()).sum()).backward()
        got.append((block_paths(blk, xg, 0), out.detach(), re_at.detach(), xg.grad,
                    {n: q.grad for n, q in blk.named_parameters()}))
    assert got[0][0] == got[1][0] and "first_multi" not in got[1][0]
    for a, b in zip(got[0][1:4], got[1][1:4]):
        assert torch.equal(a, b)
    assert all(torch.equal(got[0][4][n], got[1][4][n]) for n in got[0][4])


@pytest.mark.parametrize("T", [12, 144])
def test_multi_feature_block_never_reads_unwritten_memory(T):
    """test_block_never_reads_unwritten_memory for a multi-feature first block: save / scratch /
    outputs / the flat gradient buffer start as NaN; the buffers resized by F (E, u_et, gcon_e,
    du_et, the residual_conv partials) are where an overrun would show."""
    tp._need_gpu()
    import dstagnn_drought_amd as D
    from dstagnn_drought_amd import block_fn
    N, F, K, h, Dm, dk, C, B = 20, 4, 3, 3, 64, 16, 32, 2
    cheb, apa, tmd = _graph(N, K, 5)
    torch.manual_seed(0)
    blk = D.DSTAGNN_block("cpu", F, F, K, C, C, 1, cheb, apa, tmd, N, T, Dm, dk, dk, h, multi_feature=True)
    for q in blk.parameters():
        (torch.nn.init.xavier_uniform_ if q.dim() > 1 else torch.nn.init.uniform_)(q)
    blk = blk.cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, N, F, T, device="cuda", generator=g)
    go = torch.randn(B, N, C, T, device="cuda", generator=g)
    gr = torch.randn(B, F, h, T, T, device="cuda", generator=g)

    def run():
        for q in blk.parameters():
            q.grad = None
        xg = x.clone().requires_grad_(True)
        o, r = blk(xg, 0)
        torch.autograd.backward([o, r], [go, gr])
        with torch.no_grad():
            o2, _ = blk(x, 0)
        out = {"out": o.detach().clone(), "re_at": r.detach().clone(), "grad_x": xg.grad.clone(), "out_nograd": o2}
        out.update({n: q.grad.clone() for n, q in blk.named_parameters()})
        return out

    saved = block_fn._POISON
    try:
        block_fn._POISON = False
        plain = run()
        block_fn._POISON = True
        poisoned = run()
    finally:
        block_fn._POISON = saved
    assert plain.keys() == poisoned.keys()
    for k in plain:
        assert torch.isfinite(poisoned[k]).all(), f"{k}: NaN from an unwritten buffer"
        assert torch.equal(plain[k], poisoned[k]), f"{k}: differs with poisoned buffers"


# ---------------------------------------------------------------------------------------------
# the model: multi-feature block 0, the (B,1,h,T,T) mean hand-off, inner blocks, the head
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb_block,C", [(2, 8), (3, 8), (2, 32), (3, 32)])
def test_model_vs_fp64_helper(nb_block, C):
    tp._need_gpu()
    import dstagnn_drought_amd as D_
    from oracle import dstagnn_ref as ref
    from dstagnn_drought_amd.block_fn import block_paths
    case = f"model/nb{nb_block}/C{C}"
    N, T, K, h, D, dk, F, B, P = 16, 12, 3, 3, 64, 32, 4, 2, 12
    cheb, apa, tmd = _graph(N, K, 7)
    torch.manual_seed(11)
    net = D_.make_model("cpu", F, nb_block, F, K, C, C, 1, tmd, apa, apa, P, T, N, D, dk, dk, h, multi_feature=True)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.cuda().eval()
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(B, N, F, T, generator=gen)
    g_y = torch.randn(B, N, P, generator=gen)
    dims = dict(n_heads=h, d_k=dk, d_v=dk, K=K)
    # each block's input and res_att as the model hands them on (forward pre-hooks), for the ReLU decisions
    seen = []
    hooks = [b.register_forward_pre_hook(lambda m, a: seen.append((m, a[0].detach(), a[1]))) for b in net.BlockList]
    xg = x.cuda().requires_grad_(True)
    y = net(xg)
    for hk in hooks:
        hk.remove()
    assert len(seen) == nb_block and not torch.is_tensor(seen[0][2])
    assert seen[1][2].shape == (B, 1, h, T, T)  # the hand-off
    assert all(s[2].shape == (B, C, h, T, T) for s in seen[2:])
    assert "first_multi" in block_paths(seen[0][0], seen[0][1], 0)
    assert all("first_multi" not in block_paths(m, xi, ri) for m, xi, ri in seen[1:])
    masks = [hip_relu_masks(m, xi, ri.detach() if torch.is_tensor(ri) else ri) for m, xi, ri in seen]
    blocks, final = ref.split_state_dict(sd, nb_block)
    cheb_net = [c.clone() for c in net.BlockList[0].cheb_conv_SAt.cheb_stack.cpu().unbind(0)]

    def helper(cast):
        bl = [{k: cast(v).requires_grad_(True) for k, v in b.items()} for b in blocks]
        fi = {k: cast(v).requires_grad_(True) for k, v in final.items()}
        xx = cast(x).requires_grad_(True)
        hand, pre = [], [{} for _ in blocks]
        yy = mfr.model_forward(bl, fi, xx, [cast(c) for c in cheb_net], cast(apa), dims, masks=masks, handoff=hand,
                               pre_out=pre)
        (yy * cast(g_y)).sum().backward()
        grads = {f"BlockList.{i}.{k}": v.grad for i, b in enumerate(bl) for k, v in b.items()}
        grads.update({k: v.grad for k, v in fi.items()})
        return yy.detach(), hand[0].detach(), xx.grad, grads, pre

    y64, hand64, gx64, g64, pre = helper(lambda t: t.detach().clone().double())
    y32, hand32, gx32, g32, _ = helper(lambda t: t.detach().clone().float())
    # ReLU-aware: a HIP decision may differ from the fp64 sign only within RELU_EPS * max|z| of 0
    for i, (m3, pr) in enumerate(zip(masks, pre)):
        for m, name in zip(m3, ("z", "z_tco", "z_r")):
            z = pr[name]
            flip = m != (z > 0)
            if bool(flip.any()):
                worst, scale = float(z[flip].abs().max()), float(z.abs().max())
                assert worst <= tp.RELU_EPS * scale, f"{case} block {i} {name}: ReLU decision differs at |z| = {worst:.3e}"
    _close(case, "handoff", seen[1][2], hand64, hand32)
    _close(case, "y", y, y64, y32)
    (y * g_y.cuda()).sum().backward()
    _close(case, "dx", xg.grad, gx64, gx32)
    for n, prm in net.named_parameters():
        if g64[n] is None:  # an inner block's EmbedT / residual_conv
            assert prm.grad is None and not n.startswith("BlockList.0."), n
        else:
            assert prm.grad is not None, n
            _close(case, n, prm.grad, g64[n], g32[n])
    assert all(p_.grad is not None for n, p_ in net.BlockList[0].named_parameters())
    print(f"{case}: fp32 arm so far: {NEEDED_FP32_ARM}")


# ---------------------------------------------------------------------------------------------
# end to end: the driver on a gapped four-feature series
# ---------------------------------------------------------------------------------------------
def test_driver_trains_a_multi_feature_model_on_a_gapped_series(tmp_path):
    tp._need_gpu()
    from dstagnn_drought_amd import train as TR
    import configparser
    td, L, N, F, T, P = str(tmp_path), 200, 16, 4, 12, 12
    rs = np.random.RandomState(21)
    _, apa, tmd = _graph(N, 3, 9)
    adj = tmd.numpy() - np.eye(N)
    np.savetxt(os.path.join(td, "adj.csv"), adj + adj.T, delimiter=",")
    np.savetxt(os.path.join(td, "stag.csv"), tmd.numpy() * (0.5 + rs.rand(N, N)), delimiter=",")
    np.savetxt(os.path.join(td, "strg.csv"), apa.numpy(), delimiter=",")
    t = np.arange(L)[:, None, None]
    series = np.sin(t / 7.0 + rs.rand(1, N, F) * 6.0) * (1.0 + rs.rand(1, N, F)) + 0.1 * rs.randn(L, N, F)
    series[rs.rand(L, N, F) < 0.03] = np.nan  # a few gaps, the target feature's included
    series[0] = np.where(np.isnan(series[0]), 0.0, series[0])  # the forward fill has a value to carry
    np.savez(os.path.join(td, "SYN.npz"), data=series)
    conf = os.path.join(td, "mf.conf")
    with open(conf, "w") as f:
        f.write(f"""[Data]
adj_filename = {td}/adj.csv
graph_signal_matrix_filename = {td}/SYN.npz
stag_filename = {td}/stag.csv
strg_filename = {td}/strg.csv
num_of_vertices = {N}
points_per_hour = 12
num_for_predict = {P}
len_input = {T}
dataset_name = SYN

[Training]
in_channels = {F}
nb_block = 2
n_heads = 3
K = 3
d_k = 32
d_model = 64
nb_chev_filter = 32
nb_time_filter = 32
batch_size = 8
graph = AG
model_name = dstagnn
num_of_weeks = 0
num_of_days = 0
num_of_hours = 1
start_epoch = 0
epochs = 2
learning_rate = 0.001
missing_value = nan
""")
    lines = []
    res = TR.run(conf, epochs=2, max_batches=4, root=os.path.join(td, "exp"), log=lines.append, stream_windows=True,
                 input_fill="ffill", loss="masked_mae", multi_feature=True, test_metrics=True)
    vals = [h_["val_loss"] for h_ in res["history"]]
    print(f"multi-feature run: val losses {vals}, test loss {res['test_loss']}")
    assert len(vals) == 2 and np.isfinite(vals).all() and np.isfinite(res["test_loss"])
    assert "test_scores" in res and np.isfinite(res["test_scores"]["mae"]).all() and res["test_scores"]["count"][-1] > 0
    net = res["net"]
    assert net.multi_feature and net.BlockList[0].residual_conv.weight.shape == (32, F, 1, 1)
    # the best checkpoint reloads into a fresh multi-feature model
    cfg = configparser.ConfigParser()
    cfg.read(conf)
    fresh = TR.build(cfg, torch.device("cuda"), True)
    TR.load_best(fresh, os.path.join(res["params_path"], f"epoch_{res['best_epoch']}.params"))
    sd = net.state_dict()
    assert all(torch.equal(v, sd[k]) for k, v in fresh.state_dict().items())
    with pytest.raises(RuntimeError):  # ... and not into the default one (pre_conv of the inner block differs)
        TR.load_best(TR.build(cfg, torch.device("cuda"), False),
                     os.path.join(res["params_path"], f"epoch_{res['best_epoch']}.params"))
    # the non-target features reach the network
    fresh.eval()
    xb = torch.randn(2, N, F, T, device="cuda").requires_grad_(True)
    fresh(xb).square().sum().backward()
    assert float(xb.grad[:, :, 0, :].abs().max()) > 0 and torch.isfinite(xb.grad).all()
    assert all(float(xb.grad[:, :, f_, :].abs().max()) > 0 for f_ in range(F))
