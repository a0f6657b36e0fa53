"""GPU: HipAdam's opt-in global-norm clipping, weight decay (L2 / decoupled) and non-finite
skip (csrc/optim.hip: grad_sumsq_kernel, adam_ex_kernel, grad_scale_kernel) and the stand-alone
clip_grad_norm_.

Tensors: shapes (1,), (7,), (4095,), (4096,), (4097,), (33, 65), (3, 170, 170) — below, at and
above the 4096-element chunk, 33 chunks in all; the gradients are views at offset 3 of one flat
buffer (not 16-byte aligned), the (33, 65) one a transposed view (strided).

Yardstick: a float64 restatement of clip + Adam on the CPU (``ref_step`` below).  Bound per
parameter tensor: the larger of 1e-6 * max(1, |p|) elementwise (test_gpu_adam.py's bound) and
twice the largest error, on that tensor, of torch's own fp32 path (clip_grad_norm_ and Adam /
AdamW, both foreach=False) against the same float64 result.

grad_sumsq against float64: a thread adds 16 squares sequentially, the wave and workgroup trees
add 8 more levels (the bound below allows 12), each square rounds once: (16 + 12 + 1) * 2^-24
= 1.7e-6 on a chunk's sum, half of that on the root; the fold over chunks is fp64.  Asserted:
2e-6 relative on the norm."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (7,), (4095,), (4096,), (4097,), (33, 65), (3, 170, 170)]
TRANSPOSED = 5
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def make_grads(gen, dev, scale=1.0):
    """One flat buffer; gradient i is a view at offset 3 + (sizes before it)."""
    total = sum(math.prod(s) for s in SHAPES)
    flat = torch.randn(total + 3, device=dev, generator=gen) * scale
    out, off = [], 3
    for i, s in enumerate(SHAPES):
        n = math.prod(s)
        v = flat[off:off + n]
        out.append(v.view(s[1], s[0]).t() if i == TRANSPOSED else v.view(s))
        off += n
    assert not out[TRANSPOSED].is_contiguous()
    return out


def make_params(dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    base = [torch.randn(s, device=dev, generator=gen) for s in SHAPES]
    return gen, base


class Ref64:
    """clip + Adam in float64 on the CPU, one state per parameter, torch's formulas."""

    def __init__(self, base, max_norm=None, wd=0.0, decoupled=False, skip=False):
        self.p = [b.double().cpu() for b in base]
        self.m = [torch.zeros_like(q) for q in self.p]
        self.v = [torch.zeros_like(q) for q in self.p]
        self.t = [0] * len(self.p)
        self.max_norm, self.wd, self.decoupled, self.skip = max_norm, wd, decoupled, skip

    def step(self, grads):
        """grads: list with None for a missing gradient.  Returns the pre-clip global norm."""
        g64 = [None if g is None else g.double().cpu() for g in grads]
        norm = math.sqrt(sum(float((g * g).sum()) for g in g64 if g is not None))
        for i, g in enumerate(g64):
            if g is not None:
                self.t[i] += 1
        if self.skip and not math.isfinite(norm):
            return norm
        coef = 1.0 if self.max_norm is None else min(1.0, self.max_norm / (norm + 1e-6))
        for i, g in enumerate(g64):
            if g is None:
                continue
            t = self.t[i]
            g = g * coef
            if self.wd and not self.decoupled:
                g = g + self.wd * self.p[i]
            if self.wd and self.decoupled:
                self.p[i] = self.p[i] * (1.0 - LR * self.wd)
            self.m[i] = B1 * self.m[i] + (1.0 - B1) * g
            self.v[i] = B2 * self.v[i] + (1.0 - B2) * g * g
            denom = self.v[i].sqrt() / math.sqrt(1.0 - B2 ** t) + EPS
            self.p[i] = self.p[i] - LR / (1.0 - B1 ** t) * self.m[i] / denom
        return norm


def torch_path(params, max_norm, wd, decoupled):
    cls = torch.optim.AdamW if (wd and decoupled) else torch.optim.Adam
    opt = cls(params, lr=LR, weight_decay=wd, foreach=False)

    def step():
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
        opt.step()
    return opt, step


def check(pa, pb, ref, what=""):
    """|p_hip - p_64| <= max(1e-6 * max(1, |p|), 2 * max|p_torch32 - p_64|) per parameter tensor."""
    for i, (a, b, r) in enumerate(zip(pa, pb, ref.p)):
        e_hip = (a.detach().double().cpu() - r).abs()
        e_torch = float((b.detach().double().cpu() - r).abs().max())
        bound = torch.clamp(1e-6 * torch.clamp(r.abs(), min=1.0), min=2.0 * e_torch)
        print(f"{what} param {i} {tuple(a.shape)}: hip err {float(e_hip.max()):.3e}  torch fp32 err {e_torch:.3e}")
        assert bool((e_hip <= bound).all()), (what, i, float(e_hip.max()), e_torch)


def run_steps(max_norm, wd, decoupled, scales, seed):
    """HipAdam, torch's fp32 path and the float64 restatement on the same gradients."""
    from dstagnn_drought_amd.train import HipAdam
    dev = _dev()
    gen, base = make_params(dev, seed)
    pa = [torch.nn.Parameter(t.clone()) for t in base]
    pb = [torch.nn.Parameter(t.clone()) for t in base]
    oa = HipAdam(pa, lr=LR, max_grad_norm=max_norm, weight_decay=wd, decoupled_weight_decay=decoupled)
    _, tstep = torch_path(pb, max_norm, wd, decoupled)
    ref = Ref64(base, max_norm, wd, decoupled)
    norms = []
    for sc in scales:
        gs = make_grads(gen, dev, sc)
        for a, b, g in zip(pa, pb, gs):
            a.grad = g
            b.grad = g.clone()
        kept = [g.clone() for g in gs]
        oa.step()
        tstep()
        n64 = ref.step(gs)
        assert all(torch.equal(g, k) for g, k in zip(gs, kept))  # HipAdam clips inside: g is not written
        if max_norm is not None:
            got = float(oa.grad_norm)
            assert oa.grad_norm.dim() == 0 and oa.grad_norm.is_cuda
            assert abs(got - n64) <= 2e-6 * n64, (got, n64)
            norms.append(got)
    return pa, pb, ref, norms


def test_grad_sumsq_matches_fp64_and_repeats_bit_for_bit():
    from dstagnn_drought_amd import _lib
    ops = _lib.load()
    dev = _dev()
    gen = torch.Generator(device=dev).manual_seed(11)
    gs = make_grads(gen, dev)
    want = math.sqrt(sum(float((g.double().cpu() ** 2).sum()) for g in gs))
    first = ops.grad_sumsq(gs)
    assert first.dim() == 0 and first.dtype == torch.float64 and first.is_cuda
    got = math.sqrt(float(first))
    print(f"norm: hip {got!r}  fp64 {want!r}  rel {abs(got - want) / want:.3e}")
    assert abs(got - want) <= 2e-6 * want
    runs = [ops.grad_sumsq(gs) for _ in range(20)]
    bits = torch.stack([first] + runs).view(torch.int64)
    assert bool((bits == bits[0]).all()), bits.tolist()
    # one tensor, one short chunk; and the zero gradient
    one = torch.full((5,), 3.0, device=dev)
    assert float(ops.grad_sumsq([one])) == 45.0
    assert float(ops.grad_sumsq([torch.zeros(4097, device=dev)])) == 0.0


def test_clipped_steps_match_fp64_restatement():
    max_norm = 100.0  # |g| ~ 321 * scale over the 103 131 elements: scale 1 clips, 0.1 does not
    pa, pb, ref, norms = run_steps(max_norm, 0.0, False, [1.0, 0.1, 1.0, 0.1, 1.0, 0.1], seed=21)
    assert sum(n > max_norm for n in norms) == 3 and sum(n < max_norm for n in norms) == 3, norms
    check(pa, pb, ref, "clip")


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("max_norm", [None, 100.0])
def test_weight_decay_matches_torch_adam_and_adamw(decoupled, max_norm):
    pa, pb, ref, norms = run_steps(max_norm, 0.05, decoupled, [1.0, 0.1, 1.0, 0.1, 1.0, 0.1], seed=22)
    if max_norm is not None:
        assert any(n > max_norm for n in norms) and any(n < max_norm for n in norms), norms
    check(pa, pb, ref, f"wd decoupled={decoupled} max_norm={max_norm}")


def test_nonfinite_gradient_skips_the_step():
    from dstagnn_drought_amd.train import HipAdam
    dev = _dev()
    gen, base = make_params(dev, 23)
    pa = [torch.nn.Parameter(t.clone()) for t in base]
    pb = [torch.nn.Parameter(t.clone()) for t in base]
    oa = HipAdam(pa, lr=LR, max_grad_norm=100.0, skip_nonfinite=True)
    ob, tstep = torch_path(pb, 100.0, 0.0, False)
    ref = Ref64(base, 100.0, skip=True)
    for step in range(6):
        gs = make_grads(gen, dev)
        if step == 3:
            gs[6][1, 7, 9] = float("inf")
        for a, b, g in zip(pa, pb, gs):
            a.grad = g
            b.grad = g.clone()
        before = [(a.detach().clone(), oa.state[a]["exp_avg"].clone(), oa.state[a]["exp_avg_sq"].clone())
                  for a in pa] if step == 3 else None
        oa.step()
        ref.step(gs)
        if step == 3:
            for st in ob.state.values():  # torch's path skips alike: no update, the step count advances
                st["step"] += 1
            for a, (p0, m0, v0) in zip(pa, before):
                assert torch.equal(a.detach(), p0)
                assert torch.equal(oa.state[a]["exp_avg"], m0) and torch.equal(oa.state[a]["exp_avg_sq"], v0)
            assert int(oa.skipped_steps) == 1 and oa.skipped_steps.is_cuda
            assert not math.isfinite(float(oa.grad_norm))
        else:
            tstep()
            assert math.isfinite(float(oa.grad_norm))
    assert int(oa.skipped_steps) == 1
    assert all(oa.state[a]["step"] == 6 for a in pa)  # the host count advanced over the skipped step
    check(pa, pb, ref, "skip")


def test_missing_gradient_two_launches_one_norm_then_cached_plan():
    from dstagnn_drought_amd.train import HipAdam
    dev = _dev()
    gen, base = make_params(dev, 24)
    pa = [torch.nn.Parameter(t.clone()) for t in base]
    pb = [torch.nn.Parameter(t.clone()) for t in base]
    oa = HipAdam(pa, lr=LR, max_grad_norm=100.0)
    _, tstep = torch_path(pb, 100.0, 0.0, False)
    ref = Ref64(base, 100.0)

    def one(missing):
        gs = make_grads(gen, dev)
        for i, (a, b, g) in enumerate(zip(pa, pb, gs)):
            a.grad = None if i == missing else g
            b.grad = None if i == missing else g.clone()
        oa.step()
        tstep()
        n64 = ref.step([a.grad for a in pa])
        assert abs(float(oa.grad_norm) - n64) <= 2e-6 * n64  # every gradient, once
        assert n64 > 100.0  # (clipped)

    one(None)
    one(4)      # (4097,) sits out: its step count lags from here on, two update launches per step
    one(None)
    assert oa.state[pa[4]]["step"] == 2 and oa.state[pa[0]]["step"] == 3
    check(pa, pb, ref, "lagging")
    for _ in range(5):
        one(None)
    assert oa._plans, "cached path not taken"
    assert len(next(iter(oa._plans.values()))[2]) == 2  # two step counts: two launches, cached
    assert oa.state[pa[4]]["step"] == 7 and oa.state[pa[0]]["step"] == 8
    check(pa, pb, ref, "lagging, cached")


def test_defaults_are_todays_single_launch_bit_for_bit():
    from dstagnn_drought_amd import _lib
    from dstagnn_drought_amd.train import HipAdam
    ops = _lib.load()
    dev = _dev()
    gen, base = make_params(dev, 25)
    pa = [torch.nn.Parameter(t.clone()) for t in base]
    oa = HipAdam(pa, lr=LR)
    ps = [t.clone() for t in base]
    ms = [torch.zeros_like(t) for t in base]
    vs = [torch.zeros_like(t) for t in base]
    for t in range(1, 4):
        gs = make_grads(gen, dev)
        for a, g in zip(pa, gs):
            a.grad = g
        oa.step()
        ops.adam_step(ps, gs, ms, vs, B1, B2, EPS, LR / (1.0 - B1 ** t), math.sqrt(1.0 - B2 ** t))
    for a, p, m, v in zip(pa, ps, ms, vs):
        assert torch.equal(a.detach(), p)
        assert torch.equal(oa.state[a]["exp_avg"], m) and torch.equal(oa.state[a]["exp_avg_sq"], v)
    assert oa.grad_norm is None and int(oa.skipped_steps) == 0


def test_standalone_clip_grad_norm():
    import dstagnn_drought_amd as D
    dev = _dev()
    gen = torch.Generator(device=dev).manual_seed(26)
    gs = make_grads(gen, dev)
    pa = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in SHAPES]
    pb = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in SHAPES]
    for a, b, g in zip(pa, pb, gs):
        a.grad = g
        b.grad = g.clone()
    n_t = float(torch.nn.utils.clip_grad_norm_(pb, 100.0, foreach=False))
    got = D.clip_grad_norm_(pa, 100.0)
    assert got.dim() == 0 and got.is_cuda
    n_h = float(got)
    print(f"norm: hip {n_h!r} torch {n_t!r}")
    assert n_t > 100.0 and abs(n_h - n_t) <= 2e-6 * n_t
    for a, b in zip(pa, pb):  # (the transposed view was scaled where it lies)
        assert bool(((a.grad - b.grad).abs() <= 2e-6 * b.grad.abs()).all())
    after = math.sqrt(sum(float((a.grad.double() ** 2).sum()) for a in pa))
    assert abs(after - 100.0) <= 1e-4
    # a norm below max_norm: every bit stays
    kept = [a.grad.clone() for a in pa]
    n2 = float(D.clip_grad_norm_(pa, 1000.0))
    assert abs(n2 - after) <= 2e-6 * after
    assert all(torch.equal(a.grad, k) for a, k in zip(pa, kept))
    # a strided gradient that does not cover its storage goes through a copy and comes back
    wide = torch.randn(8, 10, device=dev, generator=gen)
    q = torch.nn.Parameter(torch.zeros(8, 5, device=dev))
    q.grad = wide[:, ::2]
    want = (wide[:, ::2].double() * (1.0 / (float(wide[:, ::2].double().norm()) + 1e-6))).float()
    untouched = wide[:, 1::2].clone()
    D.clip_grad_norm_([q], 1.0)
    assert bool(((q.grad - want).abs() <= 2e-6 * want.abs()).all()) and torch.equal(wide[:, 1::2], untouched)
