"""Worker of tests/test_gpu_adam_clip_dp.py.  Two ways to run it:

  * under torch.distributed.run, world 2 (both ranks on cuda:0, gloo over device tensors): rank r
    takes ONE fit-style step on its shard x[4r:4r+4] — zero_grad, forward, SmoothL1, backward with
    GradAllReducer.attach, ``reducer.all_reduce()``, then ``optimizer.step()`` of
    train.make_adam(max_grad_norm=...) — and saves its parameters and the step's norm;
  * as a plain process (no WORLD_SIZE): the same step on the concatenated batch of 8, plus, for
    the record, the gradient norm of each half batch on its own (what a rank would see BEFORE the
    all-reduce).

Model: make_model, N = 40, T = 12, nb_block = 2, train mode, dropout 0, split-K off (every
tiled reduction in one fixed order).  ``max_grad_norm`` is 1e-8 * sqrt(number of parameters):
the clipped gradients then have an RMS of eps = 1e-8, where Adam's first step
lr * g / (|g| + eps) still depends on the gradient's scale (0.25 lr per unit relative change at
|g| = eps; at |g| >> eps it is lr * sign(g) whatever the clipping coefficient was)."""
import json
import math
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LR = 1e-3


def main():
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = 0
    if world > 1:
        dist.init_process_group("gloo")
        rank = dist.get_rank()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import dstagnn_drought_amd as D
    from dstagnn_drought_amd import _lib
    from dstagnn_drought_amd.dp import GradAllReducer, mask_support_of
    from dstagnn_drought_amd.train import make_adam
    ops = _lib.load()
    ops.set_splitk_target(1)
    Bl, N, T, K, h, Dm, dk, C, P = 4, 40, 12, 3, 3, 64, 32, 32, 12
    B = 2 * Bl
    rs = np.random.RandomState(0)
    adj = np.zeros((N, N))
    for i in range(N):
        for j in rs.choice([q for q in range(N) if q != i], 3, replace=False):
            adj[i, j] = adj[j, i] = 1.0
    pa = (rs.rand(N, N) < 0.1).astype(np.float64)
    torch.manual_seed(1)  # identical parameters in every process
    net = D.make_model("cpu", 1, 2, 1, K, C, C, 1, adj, pa, adj, P, T, N, Dm, dk, dk, h).to(dev)
    D.set_direct_grads(net)
    D.set_dropout(net, 0.0)
    net.train()
    gen = torch.Generator(device=dev).manual_seed(100)  # the same global batch in every process
    x = torch.randn(B, N, 1, T, device=dev, generator=gen)
    y = torch.randn(B, N, P, device=dev, generator=gen)
    numel = sum(p.numel() for p in net.parameters())
    max_norm = 1e-8 * math.sqrt(numel)
    rec = {"rank": rank, "world": world, "max_grad_norm": max_norm, "numel": numel}

    def backward(xb, yb):
        for p in net.parameters():
            p.grad = None
        torch.nn.functional.smooth_l1_loss(net(xb), yb).backward()

    if world == 1:
        D.set_sample_base(net, 0)
        for r in range(2):  # for the record: each half batch's own norm (no update)
            backward(x[r * Bl:(r + 1) * Bl], y[r * Bl:(r + 1) * Bl])
            rec[f"half_norm{r}"] = float(torch.sqrt(ops.grad_sumsq([p.grad for p in net.parameters()
                                                                    if p.grad is not None])))
    opt = make_adam(net.parameters(), LR, max_grad_norm=max_norm)
    rec["optimizer"] = type(opt).__name__
    red = None
    if world > 1:
        red = GradAllReducer(net.named_parameters(), mask_support=mask_support_of(net)).attach(net)
    sl = slice(rank * Bl, (rank + 1) * Bl) if world > 1 else slice(0, B)
    opt.zero_grad()
    loss = torch.nn.functional.smooth_l1_loss(net(x[sl]), y[sl])
    loss.backward()
    if red is not None:
        red.all_reduce()
    opt.step()  # the norm is taken here: after the all-reduce
    torch.cuda.synchronize()
    rec["grad_norm"] = float(opt.grad_norm)
    out = os.environ["DSTAGNN_DP_OUT"]
    name = f"clip_rank{rank}" if world > 1 else "clip_ref"
    torch.save({n: p.detach().cpu() for n, p in net.named_parameters()}, os.path.join(out, name + ".pt"))
    with open(os.path.join(out, name + ".json"), "w") as f:
        json.dump(rec, f)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
