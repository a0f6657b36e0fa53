#!/usr/bin/env python
"""No-grad forward time of one inner DSTAGNN_block and of the full model (make_model, nb_block=4)
at a BASELINE config, through the public module call only:

    python tools/bench_infer.py PEMS08            # this tree
    LD_LIBRARY_PATH=abtest/parent DSTAGNN_EXT=abtest/parent/_C.so python tools/bench_infer.py PEMS08
    python tools/bench_infer.py PEMS08 --full-forward      # DSTAGNN_block.forward_only = False

Every shape is warmed up first; a timed window is a fixed number of calls between two HIP
events, sized from the warm-up to last at least --window seconds (default 0.5); --repeats
windows (default 5) are timed and the median, extremes and spread (max - min over median) are
printed, so a difference between two builds can be held against the run-to-run spread of each.
One JSON line: ms per call, the forward-only workspace bytes (null where the loaded library has
no such entry point), torch.cuda.max_memory_allocated over the timed calls, the bytes of
backward-only state the forward-only path does not write (computed here from the shapes and the
library's path bits), and the library stamp."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {  # name: (N, T, K, h, D, dk, C, B)  (BASELINE.json; tools/bench_configs.py)
    "PEMS08": (170, 12, 3, 3, 512, 32, 32, 32),
    "PEMS04": (307, 12, 3, 3, 512, 32, 32, 32),
    "PEMS07": (883, 12, 3, 4, 512, 32, 32, 12),
    "GAMBIA": (2139, 144, 2, 2, 64, 32, 32, 4),
    "SYN": (4096, 24, 5, 8, 512, 32, 32, 32),
}


def graphs(N):
    rs = np.random.RandomState(0)
    tmd = np.eye(N)
    pa = np.zeros((N, N))
    for i in range(N):
        tmd[i, rs.choice(N, 2, replace=False)] = 1.0
        pa[i, rs.choice(N, 4, replace=False)] = 1.0
    return tmd, pa


def skipped_bytes(B, N, F, T, K, h, dk, C, paths, nnz, apa_nnz):
    """Bytes of tensors only the backward reads, which the full forward writes and the
    forward-only path does not (forward-only section), for the paths the library takes."""
    BN, BFT, S = B * N, B * F * T, 3 * T - 12
    QW, HV = 3 * h * dk, h * dk
    n = 2 * BN * C * T + 2 * BN * T + 2 * BN + 2 * BFT  # tco, r; mu / rs of the three LayerNorms
    if F == 1:
        n += 2 * B * T  # EmbedT statistics (its u is not a separate copy of anything the forward reads)
        n += B * T * N  # u_et
    if "gtu_fused_fwd" in paths:
        n += BN * C * S + BN * 2 * C * S  # G, conv_k
    elif T >= 20 and not (C == 32 and T == 24):
        pass  # split tail: G is an intermediate of the forward itself
    else:
        n += BN * C * S
    if "tat_fused_fwd" in paths:
        n += BFT * (QW + h * T + HV + N)  # Q|K|V, A, ctx, u
    if "cheb_agg" in paths:
        n += B * N * K * F * T
    if "flash" in paths:
        n += B * K * nnz
        if "flash_small" in paths:
            n += B * K * apa_nnz + B * K * N  # P on the A_pa support, lse
    return 4 * n


def timed(fn, window, repeats):
    """ms per call over `repeats` windows of at least `window` seconds each (HIP events)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 4
    while True:  # size the window from warm calls
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 200.0 or n >= (1 << 16):
            break
        n *= 2
    n = max(n, int(n * window * 1e3 / max(ms, 1e-3)) + 1)
    out = []
    for _ in range(repeats):
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / n)
    med = statistics.median(out)
    return {"ms_per_call": round(med, 5), "min": round(min(out), 5), "max": round(max(out), 5),
            "spread": round((max(out) - min(out)) / med, 4), "calls_per_window": n,
            "window_s": round(med * n / 1e3, 3), "repeats": [round(v, 5) for v in out]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", choices=sorted(CONFIGS))
    ap.add_argument("--what", choices=["block", "model", "both"], default="both")
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--full-forward", action="store_true", help="DSTAGNN_block.forward_only = False")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    import dstagnn_drought_amd as D_
    from dstagnn_drought_amd import _lib, block_fn as bf
    N, T, K, h, Dm, dk, C, B = CONFIGS[a.config]
    tmd, pa = graphs(N)
    if a.full_forward:
        D_.DSTAGNN_block.forward_only = False
    res = {"config": a.config, "B": B, "tag": a.tag, "full_forward": bool(a.full_forward), "stamp": _lib.build_stamp()}
    gen = torch.Generator(device="cuda").manual_seed(2)
    if a.what in ("block", "both"):
        cheb = [torch.from_numpy(c).float() for c in D_.cheb_polynomial(D_.scaled_Laplacian(tmd), K)][:K]
        torch.manual_seed(1)
        blk = D_.DSTAGNN_block("cpu", C, C, K, C, C, 1, cheb, pa, tmd, N, T, Dm, dk, dk, h)
        for p in blk.parameters():
            (torch.nn.init.xavier_uniform_ if p.dim() > 1 else torch.nn.init.uniform_)(p)
        blk = blk.cuda().eval()
        x = torch.randn(B, N, C, T, device="cuda", generator=gen)
        ra = torch.randn(B, 1, h, T, T, device="cuda", generator=gen)

        def call():
            with torch.no_grad():
                blk(x, ra)

        r = timed(call, a.window, a.repeats)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        call()
        torch.cuda.synchronize()
        r["max_memory_allocated"] = torch.cuda.max_memory_allocated()
        r["peak_over_resident"] = r["max_memory_allocated"] - base
        try:  # (a library from before the forward-only entry point has no such op)
            r["workspace_bytes"] = bf.forward_only_bytes(blk, x, ra)
        except (AttributeError, RuntimeError):
            r["workspace_bytes"] = None
        paths = bf.block_paths(blk, x, ra)
        g = blk._graph()
        nnz = int(g["csc_row"].numel()) if g.get("csc_row") is not None else 0
        apa_nnz = int(g["apa_row"].numel()) if "apa_row" in g else 0
        r["paths"] = sorted(paths)
        r["backward_only_bytes_skipped"] = skipped_bytes(B, N, C, T, K, h, dk, C, paths, nnz, apa_nnz)
        res["block"] = r
        del blk, x, ra
    if a.what in ("model", "both"):
        torch.manual_seed(1)
        net = D_.make_model("cuda", 1, 4, 1, K, C, C, 1, tmd, pa, tmd, T, T, N, Dm, dk, dk, h).eval()
        x = torch.randn(B, N, 1, T, device="cuda", generator=gen)

        def call_m():
            with torch.no_grad():
                net(x)

        r = timed(call_m, a.window, a.repeats)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        call_m()
        torch.cuda.synchronize()
        r["max_memory_allocated"] = torch.cuda.max_memory_allocated()
        r["peak_over_resident"] = r["max_memory_allocated"] - base
        res["model"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
