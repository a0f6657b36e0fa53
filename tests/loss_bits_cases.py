"""The launches whose output BITS are pinned (tests/golden/g16_loss_bits.npz): shared by the
fixture's generator (tests/golden/gen_golden_loss_bits.py) and tests/test_gpu_loss_bits.py.

The kernels of csrc/loss.hip are deterministic: their output is a function of the input and of the
add order alone.  Every input here comes from an integer formula (no RNG stream is part of the
contract):

    series(n, k)[i] = (((i * MULT[k] + ADD[k]) mod 667) - 333) / 32      as fp32, exact

with period 667 = 23 * 29 in i (the recorded gradients repeat, so the fixture compresses); a masked
target sits at every index i with i mod 29 == 5 and holds -9999 (the != mode) or NaN (the NaN mode).
Each group below is a function (ops, device) -> {name: tensor}; the names are the fixture's keys.
Every case is the smallest shape that reaches its branch (see the comments at each).
"""
import torch

MULT = (1103515245, 22695477, 134775813, 1664525)  # each coprime to 667: every series takes all 667 values
ADD = (12345, 1, 5, 1013904223)
PERIOD, STRIDE, PHASE = 667, 29, 5
NULL = -9999.0
MODES = {"none": (0, 0.0, None), "neq": (1, NULL, NULL), "nan": (2, 0.0, float("nan"))}  # mode, null_val, marker
NEQ_NAN = (1, float("nan"), float("nan"))  # the != mode with a NaN null value: the library makes it the NaN mode
TILE = 4096  # dstagnn_loss_tile_elems()
N_TILES = 2 * TILE + 37  # two whole vector tiles and a scalar tail
KINDS = {"smooth_l1": (0, 1.0), "huber": (1, 0.5), "mae": (2, 0.0), "mse": (3, 0.0)}


def series(n, k, device, scale=32.0, square=False):
    i = torch.arange(n, dtype=torch.int64, device=device)
    if square:  # i^2 in place of i: neighbours no longer differ by a constant mod 667
        i = (i % PERIOD) * (i % PERIOD)
    return ((i * MULT[k] + ADD[k]) % PERIOD - 333).to(torch.float32) / scale


def mark(t, marker, every=False):
    """the flat view of t with `marker` at the fixed stride (or everywhere); None marks nothing"""
    if marker is not None:
        flat = t.view(-1)
        i = torch.arange(flat.numel(), device=t.device)
        flat[(i >= 0) if every else (i % STRIDE == PHASE)] = marker
    return t


def levels_of(Q):
    return [(q + 1.0) / (Q + 1.0) for q in range(Q)]


def _gout(device, v):
    return torch.full((1,), v, dtype=torch.float32, device=device)


def criterion(ops, device):
    out = {}

    def run(name, y, t, kind, mode, gout=None):
        code, param = KINDS[kind]
        mask, null, _ = MODES.get(mode, NEQ_NAN)
        assert y.is_contiguous() and t.is_contiguous()
        loss, stat = ops.loss_fwd(y, t, code, param, mask, null)
        dy = ops.loss_bwd(y, t, stat, gout, code, param, mask, null)
        out[f"crit/{name}/loss"], out[f"crit/{name}/stat"], out[f"crit/{name}/dy"] = loss, stat, dy

    n = N_TILES
    ybuf = series(n + 1, 0, device)
    for mode, (_, _, marker) in MODES.items():
        tbuf = mark(series(n + 1, 1, device), marker)
        assert ybuf.data_ptr() % 16 == 0 and tbuf.data_ptr() % 16 == 0
        for kind in KINDS:
            run(f"{kind}/{mode}/tiles", ybuf[:n], tbuf[:n], kind, mode)  # 16-byte loads, then the tail
            run(f"{kind}/{mode}/unaligned", ybuf[1:], tbuf[1:], kind, mode)  # from element 1: all scalar
            run(f"{kind}/{mode}/n5", ybuf[:5].clone(), tbuf[3:8].clone(), kind, mode)  # one partial tile
        if marker is not None:  # every entry masked: loss 0, stat {0, 0}, dy 0
            run(f"smooth_l1/{mode}/all-masked", ybuf[:n], mark(series(n, 1, device), marker, every=True),
                "smooth_l1", mode)
    run("smooth_l1/neq/gout-half", ybuf[:n], mark(series(n + 1, 1, device), NULL)[:n], "smooth_l1", "neq",
        _gout(device, 0.5))
    run("mae/neq-nan/tiles", ybuf[:n], mark(series(n + 1, 1, device), float("nan"))[:n], "mae", "neq-nan")
    return out


def grid_cap_inputs(device):
    n = 1025 * TILE  # one tile more than the grid cap of 1024: workgroup 0 walks two
    return series(n, 0, device), series(n, 1, device)


def grid_cap(ops, device):
    y, t = grid_cap_inputs(device)
    loss, stat = ops.loss_fwd(y, t, *KINDS["mae"], 0, 0.0)
    return {"cap/mae/loss": loss, "cap/mae/stat": stat}


def grid_cap_dy(ops, device, stat):
    """(dy of the kernel, sign(y - t) * scale with the scale the kernel forms from `stat`): equal
    bit for bit under mae (the slope is -1, 0 or 1), so the 16 MB gradient is not recorded"""
    y, t = grid_cap_inputs(device)
    stat = stat.to(device)
    dy = ops.loss_bwd(y, t, stat, None, *KINDS["mae"], 0, 0.0)
    scale = (1.0 / stat[1]).to(torch.float32)  # (float)((double)1.f / count)
    return dy, torch.sign(y - t) * scale


# Q -> m with m Q >= two whole tiles and a tail (3 * 2743 = 2 * 4096 + 37; 4 and 16 do not divide
# 8229: 8232 and 8240).  Q = 3: the walk wraps inside a float4.
PINBALL_M = {1: N_TILES, 3: 2743, 4: 2058, 16: 515}


def pinball(ops, device):
    out = {}

    def run(name, y, t, Q, mode, gout=None):
        mask, null, _ = MODES.get(mode, NEQ_NAN)
        assert y.is_contiguous() and t.is_contiguous()
        loss, stat = ops.pinball_fwd(y, t, levels_of(Q), mask, null)
        dy = ops.pinball_bwd(y, t, stat, gout, levels_of(Q), mask, null)
        out[f"pin/{name}/loss"], out[f"pin/{name}/stat"], out[f"pin/{name}/dy"] = loss, stat, dy

    for Q, m in PINBALL_M.items():
        ybuf = series(m * Q + 1, 0, device)
        for mode, (_, _, marker) in MODES.items():
            t = mark(series(m, 1, device), marker)
            run(f"Q{Q}/{mode}/tiles", ybuf[:m * Q].view(m, Q), t, Q, mode)
            run(f"Q{Q}/{mode}/unaligned", ybuf[1:].view(m, Q), t, Q, mode)
    m = PINBALL_M[3]
    run("Q3/nan/gout-half", series(m * 3, 0, device).view(m, 3), mark(series(m, 1, device), float("nan")), 3, "nan",
        _gout(device, 0.5))
    run("Q3/neq-nan/tiles", series(m * 3, 0, device).view(m, 3), mark(series(m, 1, device), float("nan")), 3, "neq-nan")
    return out


def metrics(ops, device):
    out = {}
    # 400 rows of P = 12: 21 rows a pass, 8 passes a workgroup -> three workgroups, a partial last
    # pass; 7 rows of P = 5: one workgroup.  Two successive updates into one table.
    for rows, P in ((400, 12), (7, 5)):
        table = torch.zeros(P, 4, dtype=torch.float64, device=device)
        for k, null in ((0, 0.0), (2, float("nan"))):
            pred = series(rows * P, k, device).view(rows, P)
            tg = series(rows * P, k + 1, device).view(rows, P)
            # null 0: zeros at the stride (and the formula's own); null NaN: no target is NaN and,
            # moved by 1 / 64, none is 0 (every entry counts, no e / 0)
            tg = mark(tg, 0.0) if k == 0 else tg + 0.015625
            ops.metrics_update(pred, tg, null, table)
            out[f"met/{rows}x{P}/update{k // 2}"] = table.clone()
    return out


# (B, N, P): 21 nodes a strip with four idle threads, three strips (the last partial), one unrolled
# group of 4 samples plus 2; P = 1: two strips of 256 nodes; P = 256: one node a strip
MASKED_SHAPES = ((6, 47, 12), (2, 300, 1), (2, 3, 256))


def metrics_masked(ops, device):
    out = {}
    for B, N, P in MASKED_SHAPES:
        for mode, (mask, null, marker) in MODES.items():
            for nodes in (False, True):
                if (B, N, P) != MASKED_SHAPES[0] and not (mode == "nan" and nodes):
                    continue
                ht = torch.zeros(P, 8, dtype=torch.float64, device=device)
                nt = torch.zeros(N, 8, dtype=torch.float64, device=device) if nodes else None
                for k in (0, 2):  # two successive updates
                    pred = series(B * N * P, k, device).view(B, N, P)
                    tg = mark(series(B * N * P, k + 1, device), marker).view(B, N, P)
                    ops.metrics_update_masked(pred, tg, mask, null, 0.0, ht, nt)
                    name = f"mm/{B}x{N}x{P}/{mode}/{'nodes' if nodes else 'plain'}/update{k // 2}"
                    out[name + "/htable"] = ht.clone()
                    if nodes:
                        out[name + "/ntable"] = nt.clone()
    return out


def metrics_quantile(ops, device):
    out = {}
    B, N, P = 5, 25, 12  # 21 nodes a strip: two strips, the second partial
    for Q in (2, 3, 16):  # 8 columns: one chunk; 11: a partial second chunk; 50: seven chunks
        for mode, nodes in (("nan", True), ("neq", False), ("none", True)):
            mask, null, marker = MODES[mode]
            tg = mark(series(B * N * P, 1, device), marker).view(B, N, P)
            # level q sits 0.5 (q - (Q - 1) / 2) above the target plus noise in [-0.33, 0.33]: some
            # neighbours cross, most do not
            off = 0.5 * (torch.arange(Q, dtype=torch.float32, device=device) - (Q - 1) / 2.0)
            base = torch.where(torch.isnan(tg) | (tg == NULL), torch.zeros_like(tg), tg)
            pred = (base[..., None] + series(B * N * P * Q, 2, device, 1024.0, square=True).view(B, N, P, Q) + off).contiguous()
            ht = torch.zeros(P, 2 + 3 * Q, dtype=torch.float64, device=device)
            nt = torch.zeros(N, 2 + 3 * Q, dtype=torch.float64, device=device) if nodes else None
            ops.metrics_update_quantile(pred, tg, levels_of(Q), mask, null, ht, nt)
            name = f"qm/Q{Q}/{mode}/{'nodes' if nodes else 'plain'}"
            out[name + "/htable"] = ht.clone()
            assert 0 < float(ht[:, 1].sum()) < float(ht[:, 0].sum())  # some entries cross, not all
            if nodes:
                out[name + "/ntable"] = nt.clone()
    return out


GROUPS = {"criterion": criterion, "grid_cap": grid_cap, "pinball": pinball, "metrics": metrics,
          "metrics_masked": metrics_masked, "metrics_quantile": metrics_quantile}
PREFIX = {"criterion": "crit/", "grid_cap": "cap/", "pinball": "pin/", "metrics": "met/", "metrics_masked": "mm/",
          "metrics_quantile": "qm/"}
