#!/usr/bin/env python
"""What a multi-feature first block costs against the F = 1 first block of the same build:
forward + backward of ONE first block (train mode, direct gradients, inputs resident in HBM) at

  PEMS08  N = 170,  T = 12,  K = 3, h = 3, D = 512, C = 32, B = 32
  GAMBIA  N = 2139, T = 144, K = 2, h = 2, D = 64,  C = 32, B = 4

for F = 1 and F = 4, both built with ``multi_feature=True`` (at F = 1 that is the default first
block, bit for bit, on its usual kernels: the fused GTU stage at PEMS08).  There is no parent to
compare with — the parent cannot run F = 4 — so the F = 1 block is the yardstick and the ratio is
reported, not judged.

Protocol: every (geometry, F) runs in three fresh processes, the two variants alternating
(F1 F4 F1 F4 F1 F4) on one device, each process timing --steps steps between two device events
after --warmup steps; reported per variant: the three figures, their median and the spread
(max - min) / median, beside the kernel-path names of dstagnn_block_paths for the timed call.

    python tools/bench_multifeature.py --out profiles/multifeature_first_block.json

The JSON carries the library stamp (dstagnn_drought_amd._lib.build_stamp).  There is no fallback:
without a HIP device the tool fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (N, T, K, h, D, dk, C, B)
GEOMETRIES = {"PEMS08": (170, 12, 3, 3, 512, 32, 32, 32), "GAMBIA": (2139, 144, 2, 2, 64, 32, 32, 4)}
FEATURES = (1, 4)


def child(name, F, steps, warmup):
    import numpy as np
    import torch
    import dstagnn_drought_amd as D_
    from dstagnn_drought_amd.block_fn import block_paths
    N, T, K, h, Dm, dk, C, B = GEOMETRIES[name]
    rs = np.random.RandomState(0)
    tmd, pa = np.eye(N), np.zeros((N, N))
    for i in range(N):
        tmd[i, rs.choice(N, 2, replace=False)] = 1.0
        pa[i, rs.choice(N, 4, replace=False)] = 1.0
    cheb = [torch.from_numpy(c).float() for c in D_.cheb_polynomial(D_.scaled_Laplacian(tmd), K)][:K]
    torch.manual_seed(1)
    blk = D_.DSTAGNN_block("cpu", F, F, K, C, C, 1, cheb, pa, tmd, N, T, Dm, dk, dk, h, multi_feature=True)
    for p in blk.parameters():
        (torch.nn.init.xavier_uniform_ if p.dim() > 1 else torch.nn.init.uniform_)(p)
    blk = D_.set_direct_grads(blk.cuda().train())
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn(B, N, F, T, device="cuda", generator=g).requires_grad_(True)
    go = torch.randn(B, N, C, T, device="cuda", generator=g)
    gr = torch.randn(B, F, h, T, T, device="cuda", generator=g)
    paths = sorted(block_paths(blk, x, 0, train=True))

    def step():
        for p in blk.parameters():
            p.grad = None
        x.grad = None
        o, r = blk(x, 0)
        torch.autograd.backward([o, r], [go, gr])

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    e1.synchronize()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in blk.parameters())
    print(json.dumps({"ms_per_step": round(e0.elapsed_time(e1) / steps, 4), "paths": paths}))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multifeature_first_block.json"))
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="processes per variant")
    ap.add_argument("--child", nargs=2, metavar=("GEOMETRY", "F"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), a.steps, a.warmup)
    from dstagnn_drought_amd import _lib
    result = {"build": _lib.build_stamp(), "steps": a.steps, "warmup": a.warmup, "processes_per_variant": a.rounds,
              "what": "one first block, forward + backward, train mode, ms per step", "geometries": {}}
    for name, geo in GEOMETRIES.items():
        runs = {F: [] for F in FEATURES}
        paths = {}
        for _ in range(a.rounds):
            for F in FEATURES:  # alternating: F1 F4 F1 F4 ...
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, str(F), "--steps",
                                      str(a.steps), "--warmup", str(a.warmup)], check=True, capture_output=True,
                                     text=True, timeout=600).stdout
                rec = json.loads(out.strip().splitlines()[-1])
                runs[F].append(rec["ms_per_step"])
                paths[F] = rec["paths"]
        med = {F: statistics.median(r) for F, r in runs.items()}
        result["geometries"][name] = {
            "N_T_K_h_D_dk_C_B": list(geo),
            **{f"F{F}": {"ms_per_step_runs": runs[F], "median_ms": med[F],
                         "spread": round((max(runs[F]) - min(runs[F])) / med[F], 4), "paths": paths[F]}
               for F in FEATURES},
            "ratio_F4_over_F1": round(med[4] / med[1], 4)}
        print(name, json.dumps(result["geometries"][name]), flush=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
