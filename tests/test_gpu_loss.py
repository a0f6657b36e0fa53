"""GPU: the on-device criterion and test-set scores (csrc/loss.hip: loss_fwd_kernel,
loss_bwd_kernel, metrics_accum_kernel; dstagnn_drought_amd/loss.py; the driver options of
train.py) against a float64 restatement of their formulas on the CPU, computed from the same
fp32 inputs upcast.

Inputs are seeded: target ~ 3 N(0, 1), y = target + N(0, 1), so both branches of smooth_l1 and
huber are well populated; masked cases set ~30 % of the targets to the null value (0.0 or NaN).

Bounds (derived, not measured):
  loss     <= 1e-6 relative.  Every term is non-negative and carries at most three fp32
           roundings (y - t, then two of the term's own), every add is fp64, one rounding to
           fp32 at the end: <= 4 * 2^-24 = 2.4e-7.  The bound is four times that.
  dy       <= 1e-6 |dy| elementwise (y - t, d / beta, gout / count, their product: four
           roundings) and exactly 0 at masked entries.
  metrics  <= 1e-6 relative per entry of compute(): <= 3 roundings per term, fp64 sums.

The largest parity shape, (32, 170, 12) = 65280 elements, is checked against the kernel's own tile
(dstagnn_loss_tile_elems() = 4096, read through the C-ABI): 16 workgroups, the last one partial, so
no further shape was added for that.  Two extra cases take the remaining paths: a loss of more
tiles than the grid cap (workgroups walk several tiles) and a metrics update of more row groups
than its cap.
"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KINDS = [("smooth_l1", 1.0), ("smooth_l1", 0.25), ("huber", 0.5), ("mae", 0.0), ("mse", 0.0)]
MASKS = [None, 0.0, float("nan")]
SHAPES = ["1x1x1", "1x5x3", "3x101x3-unaligned", "2x170x12", "32x170x12"]
REL = 1e-6


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _pair(shape_id, null, seed=0):
    """(y, target) on the device for a SHAPES id; ~30 % of the targets set to `null`."""
    g = torch.Generator().manual_seed(1000 + seed + 17 * SHAPES.index(shape_id))
    if shape_id == "3x101x3-unaligned":
        full = (5, 101, 3)
    else:
        full = tuple(int(v) for v in shape_id.split("x"))
    t = 3.0 * torch.randn(full, generator=g)
    y = t + torch.randn(full, generator=g)
    if null is not None:
        t[torch.rand(full, generator=g) < 0.3] = null
    y, t = y.cuda(), t.cuda()
    if shape_id == "3x101x3-unaligned":  # buf[1:4]: 1212 bytes into the buffer, not 16-byte aligned
        y, t = y[1:4], t[1:4]
        assert y.data_ptr() % 16 != 0 and t.data_ptr() % 16 != 0 and y.is_contiguous()
    return y, t


def _valid(t64, null):
    if null is None:
        return torch.ones_like(t64, dtype=torch.bool)
    return ~torch.isnan(t64) if math.isnan(null) else t64 != null


def ref64(y, t, kind, param, null, gout=1.0):
    """float64 loss and gradient of DESIGN §11.1's table from the fp32 inputs upcast."""
    y64, t64 = y.detach().double().cpu(), t.detach().double().cpu()
    valid = _valid(t64, null)
    d = torch.where(valid, y64 - t64, torch.zeros_like(y64))
    a = d.abs()
    if kind == "smooth_l1" and param > 0:
        term = torch.where(a < param, 0.5 * d * d / param, a - 0.5 * param)
        slope = torch.where(a < param, d / param, torch.sign(d))
    elif kind == "huber":
        term = torch.where(a <= param, 0.5 * d * d, param * (a - 0.5 * param))
        slope = torch.where(a <= param, d, param * torch.sign(d))
    elif kind in ("mae", "smooth_l1"):
        term, slope = a, torch.sign(d)
    else:
        term, slope = d * d, 2.0 * d
    count = int(valid.sum())
    if count == 0:
        return 0.0, torch.zeros_like(y64), valid
    zero = torch.zeros_like(term)
    loss = float(torch.where(valid, term, zero).sum()) / count
    return loss, torch.where(valid, slope * (gout / count), zero), valid


def _make(kind, param, null):
    from dstagnn_drought_amd import HipLoss
    return HipLoss(kind, beta=param, delta=param, null_val=null)


def _run(crit, y, t, factor=None):
    yl = y.detach().requires_grad_(True)  # (a view of y's storage: the same, possibly unaligned, pointer)
    assert yl.data_ptr() == y.data_ptr()
    loss = crit(yl, t)
    (loss if factor is None else factor * loss).backward()
    return loss.detach(), yl.grad


def _check(loss, dy, want, want_dy, valid, what):
    got = float(loss)
    print(f"{what}: loss {got!r} want {want!r} rel {abs(got - want) / max(abs(want), 1e-300):.2e}")
    assert loss.dim() == 0 and loss.dtype == torch.float32
    assert abs(got - want) <= REL * abs(want), what
    dyc = dy.double().cpu()
    err = (dyc - want_dy).abs()
    rel = float((err / want_dy.abs().clamp_min(1e-300))[want_dy != 0].max()) if bool((want_dy != 0).any()) else 0.0
    print(f"{what}: dy worst rel {rel:.2e}")
    assert bool((err <= REL * want_dy.abs()).all()), what
    assert bool((dyc[~valid] == 0).all()), what + ": a masked gradient entry is not exactly 0"


def test_largest_parity_shape_has_a_partial_last_workgroup():
    from dstagnn_drought_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.dstagnn_loss_scratch_bytes.restype = ctypes.c_int64
    lib.dstagnn_loss_scratch_bytes.argtypes = [ctypes.c_int64]
    n, tile = 32 * 170 * 12, lib.dstagnn_loss_tile_elems()
    wgs = lib.dstagnn_loss_scratch_bytes(n) // 16  # one {sum, count} pair of doubles per workgroup
    assert wgs == -(-n // tile) >= 3 and n % tile != 0, (n, tile, wgs)


@pytest.mark.parametrize("null", MASKS, ids=["nomask", "null0", "nan"])
@pytest.mark.parametrize("shape_id", SHAPES)
def test_parity_every_kind(shape_id, null):
    _need_gpu()
    y, t = _pair(shape_id, null)
    for kind, param in KINDS:
        crit = _make(kind, param, null)
        what = f"{kind}({param}) {shape_id} null={null}"
        for factor in (None, 2.5):
            loss, dy = _run(crit, y, t, factor)
            want, want_dy, valid = ref64(y, t, kind, param, null, 1.0 if factor is None else factor)
            _check(loss, dy, want, want_dy, valid, what + f" x{factor}")
            assert dy.shape == y.shape


@pytest.mark.parametrize("shape_id", ["1x5x3", "3x101x3-unaligned", "32x170x12"])
def test_masked_kind_without_masked_entries_keeps_the_bits(shape_id):
    _need_gpu()
    y, t = _pair(shape_id, None)
    assert not bool((t == 0).any()) and not bool(torch.isnan(t).any())
    for kind, param in KINDS:
        loss0, dy0 = _run(_make(kind, param, None), y, t)
        for null in (0.0, float("nan")):
            loss1, dy1 = _run(_make(kind, param, null), y, t)
            assert torch.equal(loss0.view(torch.int32), loss1.view(torch.int32)), (kind, null)
            assert torch.equal(dy0.view(torch.int32), dy1.view(torch.int32)), (kind, null)
    for name, base in (("masked_mae", "mae"), ("masked_mse", "mse")):
        a, da = _run(_make(name, 0.0, 0.0), y, t)
        b, db = _run(_make(base, 0.0, None), y, t)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(da, db)


def test_loss_past_the_grid_cap():
    """More tiles than the forward's grid cap: workgroups walk tiles w, w + grid, ...; the
    backward has one workgroup per tile."""
    _need_gpu()
    from dstagnn_drought_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.dstagnn_loss_scratch_bytes.restype = ctypes.c_int64
    lib.dstagnn_loss_scratch_bytes.argtypes = [ctypes.c_int64]
    shape = (1027, 4099, 1)
    n, tile = shape[0] * shape[1], lib.dstagnn_loss_tile_elems()
    assert lib.dstagnn_loss_scratch_bytes(n) // 16 < -(-n // tile)  # capped
    g = torch.Generator().manual_seed(5)
    t = 3.0 * torch.randn(shape, generator=g)
    y = t + torch.randn(shape, generator=g)
    for kind, param, null in (("smooth_l1", 1.0, None), ("mae", 0.0, 0.0)):
        tt = t.clone()
        if null is not None:
            tt[torch.rand(shape, generator=g) < 0.3] = null
        yc, tc = y.cuda(), tt.cuda()
        loss, dy = _run(_make(kind, param, null), yc, tc)
        want, want_dy, valid = ref64(yc, tc, kind, param, null)
        _check(loss, dy, want, want_dy, valid, f"{kind} capped grid null={null}")


def test_exact_integer_case():
    """mae at (2, 128, 4) on small integers: every term and the sum are exact, so the loss is the
    float64 value bit for bit and dy is in {0, +-1/1024} exactly.  Repeated with exactly 512
    targets set to the null value: the valid count is then 512, so by loss = sum / count_valid
    the exact gradient values are {0, +-1/512} (0 at every masked entry).  Targets are non-zero
    integers in [-8, 8], so a null value of 0.0 masks the 512 chosen entries and no other."""
    _need_gpu()
    g = torch.Generator().manual_seed(11)
    shape = (2, 128, 4)
    mag = torch.randint(1, 9, shape, generator=g).float()
    t = torch.where(torch.rand(shape, generator=g) < 0.5, -mag, mag)
    d = torch.randint(-3, 4, shape, generator=g).float()
    y = t + d
    loss, dy = _run(_make("mae", 0.0, None), y.cuda(), t.cuda())
    want = float(d.double().abs().sum()) / 1024.0
    assert float(loss) == want and float(np.float32(want)) == want
    assert torch.equal(dy.cpu(), torch.sign(d) / 1024.0)
    assert set(dy.cpu().unique().tolist()) <= {0.0, 1.0 / 1024, -1.0 / 1024}
    pick = torch.randperm(1024, generator=g)[:512]
    for null in (0.0, float("nan")):
        tm = t.clone().view(-1)
        tm[pick] = null
        tm = tm.view(shape)
        keep = torch.ones(1024, dtype=torch.bool)
        keep[pick] = False
        keep = keep.view(shape)
        loss, dy = _run(_make("masked_mae", 0.0, null), y.cuda(), tm.cuda())
        want = float(d.double().abs()[keep].sum()) / 512.0
        assert float(loss) == want, (null, float(loss), want)
        assert torch.equal(dy.cpu(), torch.where(keep, torch.sign(d) / 512.0, torch.zeros(shape)))
        assert int((dy.cpu()[~keep] != 0).sum()) == 0


def test_edge_semantics():
    _need_gpu()
    y, t = _pair("2x170x12", None, seed=3)
    # every target masked: loss 0, gradient 0
    for null, fill in ((0.0, 0.0), (float("nan"), float("nan")), (-7.5, -7.5)):
        for kind, param in KINDS:
            loss, dy = _run(_make(kind, param, null), y, torch.full_like(t, fill))
            assert float(loss) == 0.0 and not bool(dy.any()), (kind, null)
    # a NaN prediction at one valid entry: the loss is NaN (masked or not)
    ybad = y.clone()
    ybad[1, 7, 3] = float("nan")
    for null in (None, 0.0, float("nan")):
        for kind, param in KINDS:
            loss, _ = _run(_make(kind, param, null), ybad, t)
            assert math.isnan(float(loss)), (kind, null)
    # ... and none when that entry is masked out
    tm = t.clone()
    tm[1, 7, 3] = 0.0
    loss, dy = _run(_make("smooth_l1", 1.0, 0.0), ybad, tm)
    assert math.isfinite(float(loss)) and float(dy[1, 7, 3]) == 0.0 and bool(torch.isfinite(dy).all())
    # NaN targets under the NaN mode: a finite loss, gradient exactly 0 there
    tn = t.clone()
    holes = torch.rand(t.shape, generator=torch.Generator().manual_seed(9)) < 0.3
    tn[holes.cuda()] = float("nan")
    for kind, param in KINDS:
        loss, dy = _run(_make(kind, param, float("nan")), y, tn)
        want, want_dy, valid = ref64(y, tn, kind, param, float("nan"))
        _check(loss, dy, want, want_dy, valid, f"{kind} NaN targets")
        assert math.isfinite(float(loss)) and bool((dy[holes.cuda()] == 0).all())
        assert bool(torch.isfinite(dy).all())


def test_module_contract():
    _need_gpu()
    from dstagnn_drought_amd import HipLoss
    y, t = _pair("2x170x12", None)
    crit = HipLoss()
    with torch.no_grad():
        out = crit(y.clone().requires_grad_(True), t)
    assert out.grad_fn is None and not out.requires_grad and out.dim() == 0
    assert crit(y, t).grad_fn is None  # no input requires grad: the plain op, nothing saved
    with pytest.raises(RuntimeError):
        crit(y, t.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        crit(y, t[:, :, :1])
    # non-contiguous inputs are made contiguous
    yt, tt = y.transpose(0, 1), t.transpose(0, 1)
    assert not yt.is_contiguous()
    a = crit(yt, tt)
    assert torch.equal(a, crit(yt.contiguous(), tt.contiguous()))
    yl = y.clone().requires_grad_(True)
    crit(yl.transpose(0, 1), tt).backward()
    _, want_dy, _ = ref64(y, t, "smooth_l1", 1.0, None)
    assert bool(((yl.grad.double().cpu() - want_dy).abs() <= REL * want_dy.abs()).all())
    # beta = 0 is mae (no division by zero)
    z, dz = _run(HipLoss("smooth_l1", beta=0.0), y, t)
    m, dm = _run(HipLoss("mae"), y, t)
    assert torch.equal(z, m) and torch.equal(dz, dm) and math.isfinite(float(z))
    # against torch's own criterion (fp32): a coarse cross-check of the restatement itself
    ref = torch.nn.SmoothL1Loss()(y, t)
    assert abs(float(a) - float(ref)) <= 1e-5 * float(ref)


def _ref_metrics(pred, target):
    """The float64 formulas of the per-horizon list."""
    p64, t64 = pred.double().cpu().numpy(), target.double().cpu().numpy()
    P = p64.shape[-1]
    p64, t64 = p64.reshape(-1, P), t64.reshape(-1, P)

    def three(p, t):
        e = p - t
        m = t != 0
        return [float(np.abs(e).mean()), float(np.sqrt((e * e).mean())),
                float(100.0 * np.abs(e[m] / t[m]).sum() / m.sum()) if m.any() else 0.0]
    out = []
    for i in range(P):
        out.extend(three(p64[:, i], t64[:, i]))
    out.extend(three(p64.reshape(-1), t64.reshape(-1)))
    return out


METRIC_CASES = {
    "1x1x1": ((1, 1, 1), [1], None),
    "5x101x3-two-updates": ((5, 101, 3), [2, 3], None),
    "4x170x12": ((4, 170, 12), [4], None),
    "3x7x19-zero-horizon": ((3, 7, 19), [3], 5),
    "300x170x12-capped-grid": ((300, 170, 12), [300], None),
}


@pytest.mark.parametrize("case", list(METRIC_CASES))
def test_metrics_match_fp64(case):
    _need_gpu()
    from dstagnn_drought_amd import ForecastMetrics
    shape, parts, zero_h = METRIC_CASES[case]
    g = torch.Generator().manual_seed(77 + len(case))
    t = 3.0 * torch.randn(shape, generator=g)
    p = t + torch.randn(shape, generator=g)
    t[torch.rand(shape, generator=g) < 0.3] = 0.0
    if zero_h is not None:
        t[..., zero_h] = 0.0
    p, t = p.cuda(), t.cuda()
    want = _ref_metrics(p, t)
    m = ForecastMetrics(shape[-1], 0.0, "cuda")
    runs = []
    for _ in range(2):
        at = 0
        for s in parts:
            m.update(p[at:at + s], t[at:at + s])
            at += s
        runs.append((m.table.clone(), m.compute()))
        m.reset()
        assert m.compute() == [0.0] * (3 * shape[-1] + 3)
    got = runs[0][1]
    assert len(got) == 3 * shape[-1] + 3 and all(isinstance(v, float) for v in got)
    worst = max(abs(a - b) / abs(b) for a, b in zip(got, want) if b != 0)
    print(f"{case}: worst rel {worst:.2e}")
    for i, (a, b) in enumerate(zip(got, want)):
        assert abs(a - b) <= REL * abs(b), (case, i, a, b)
    if zero_h is not None:
        assert got[3 * zero_h + 2] == 0.0 and want[3 * zero_h + 2] == 0.0
    # the same updates again: the same bits
    assert torch.equal(runs[0][0].view(torch.int64), runs[1][0].view(torch.int64)) and runs[0][1] == runs[1][1]


def test_metrics_nan_null_counts_the_non_nan_targets():
    _need_gpu()
    from dstagnn_drought_amd import ForecastMetrics
    g = torch.Generator().manual_seed(4)
    t = 3.0 * torch.randn(4, 9, 5, generator=g)
    p = t + torch.randn(4, 9, 5, generator=g)
    m0 = ForecastMetrics(5, -1000.0, "cuda")  # no target equals it: every entry counts
    m1 = ForecastMetrics(5, float("nan"), "cuda")
    m0.update(p.cuda(), t.cuda())
    m1.update(p.cuda(), t.cuda())
    assert torch.equal(m0.table, m1.table) and float(m1.table[:, 3].sum()) == 4 * 9 * 5


def test_determinism_and_the_shared_ticket():
    """The loss and the metrics draw the stream's one ticket counter and must leave it at zero:
    after three loss calls and two metric updates the gradient norm of optim.hip (the same
    counter) still matches its float64 value at its own 2e-6 bound, and a repeated call gives
    the same bits."""
    _need_gpu()
    from dstagnn_drought_amd import ForecastMetrics, _lib
    import dstagnn_drought_amd as D
    ops = _lib.load()
    y, t = _pair("32x170x12", 0.0)
    crit = _make("smooth_l1", 1.0, 0.0)
    first = _run(crit, y, t)
    again = _run(crit, y, t)
    assert torch.equal(first[0].view(torch.int32), again[0].view(torch.int32))
    assert torch.equal(first[1].view(torch.int32), again[1].view(torch.int32))
    third = _run(_make("huber", 0.5, None), y, t)
    assert math.isfinite(float(third[0]))
    m = ForecastMetrics(12, 0.0, "cuda")
    m.update(y, t)
    m.update(y, t)
    g = torch.Generator().manual_seed(7)
    gs = [torch.randn(4099, generator=g).cuda(), torch.randn(31, 17, generator=g).cuda()]
    want = math.sqrt(sum(float((x.double() ** 2).sum()) for x in gs))
    got = math.sqrt(float(ops.grad_sumsq(gs)))
    assert abs(got - want) <= 2e-6 * want, (got, want)
    ps = [torch.nn.Parameter(torch.zeros_like(x)) for x in gs]
    for prm, x in zip(ps, gs):
        prm.grad = x.clone()
    norm = float(D.clip_grad_norm_(ps, 1e9))
    assert abs(norm - want) <= 2e-6 * want, (norm, want)
    # and the loss still gives its first bits after them
    last = _run(crit, y, t)
    assert torch.equal(first[0].view(torch.int32), last[0].view(torch.int32))
    assert torch.equal(first[1].view(torch.int32), last[1].view(torch.int32))
    two = m.compute()
    m.reset()
    m.update(y, t)
    one = m.compute()
    for a, b in zip(one, two):  # twice the sums over twice the rows: the same scores
        assert abs(a - b) <= 1e-12 * abs(b)


def _g12(golden_dir, tmp_path):
    """The g12 fixture laid out as tests/test_gpu_train.py does."""
    g = dict(np.load(os.path.join(golden_dir, "g12_train.npz"), allow_pickle=False))
    td = str(tmp_path)
    for k in ("adj.csv", "stag.csv", "strg.csv"):
        with open(os.path.join(td, k), "w") as f:
            f.write(str(g[k + "_text"]))
    np.savez(os.path.join(td, "SYN.npz"), data=g["series"])
    from dstagnn_drought_amd.data import read_and_generate_dataset
    read_and_generate_dataset(os.path.join(td, "SYN.npz"), 0, 0, 1, 12, points_per_hour=12, save=True)
    conf = os.path.join(td, "train.conf")
    with open(conf, "w") as f:
        f.write(str(g["config_text"]).replace("@DIR@", td))
    return conf, td


def test_end_to_end_on_the_train_fixture(golden_dir, tmp_path, capsys):
    _need_gpu()
    import configparser
    from dstagnn_drought_amd import HipLoss
    from dstagnn_drought_amd import data as data_io
    from dstagnn_drought_amd import train as TR
    conf, td = _g12(golden_dir, tmp_path)
    torch.cuda.set_device(0)
    quiet = lambda *_: None  # noqa: E731
    base = TR.run(conf, dropout=0.0, root=os.path.join(td, "exp_torch"), log=quiet)  # torch's criterion
    hip = TR.run(conf, dropout=0.0, root=os.path.join(td, "exp_hip"), log=quiet, loss="smooth_l1")
    va = np.array([h["val_loss"] for h in base["history"]])
    vb = np.array([h["val_loss"] for h in hip["history"]])
    with capsys.disabled():
        print("\nval", va.tolist(), vb.tolist(), "test", base["test_loss"], hip["test_loss"])
    assert len(va) == len(vb) >= 1
    assert np.abs(va - vb).max() <= 1e-4, (va, vb)
    assert abs(base["test_loss"] - hip["test_loss"]) <= 1e-4
    assert isinstance(TR.make_criterion("smooth_l1"), HipLoss)
    short = TR.run(conf, dropout=0.0, root=os.path.join(td, "exp_masked"), log=quiet, loss="masked_mae",
                   missing_value=0.0, epochs=1, max_batches=2)
    assert len(short["history"]) == 1 and short["history"][0]["batches"] == 2
    assert all(math.isfinite(h["train_loss"]) and math.isfinite(h["val_loss"]) for h in short["history"])
    assert math.isfinite(short["test_loss"])
    # the trained net's test-set scores: on the device vs the float64 formulas over the host path's file
    cp = configparser.ConfigParser()
    cp.read(conf)
    dc, tc = cp["Data"], cp["Training"]
    loaded = data_io.load_graphdata_channel1(dc["graph_signal_matrix_filename"], int(tc["num_of_hours"]),
                                             int(tc["num_of_days"]), int(tc["num_of_weeks"]), "cuda:0",
                                             int(tc["batch_size"]))
    test_loader, test_target, mean, std = loaded[7], loaded[8], loaded[9], loaded[10]
    net = hip["net"]
    TR.predict_and_save_results_mstgcn(net, test_loader, test_target, 0, mean, std, td, "test")
    saved = np.load(os.path.join(td, "output_epoch_0_test.npz"))
    capsys.readouterr()

    class Writer:
        def __init__(self):
            self.rows = {}

        def add_scalar(self, name, value, step):
            self.rows[name] = (value, step)

    sw = Writer()
    got = TR.evaluate_on_test_mstgcn(net, test_loader, test_target, sw, 3, mean, std)
    out = capsys.readouterr().out
    want = _ref_metrics(torch.from_numpy(saved["prediction"]), torch.from_numpy(saved["data_target_tensor"]))
    P = saved["prediction"].shape[2]
    assert len(got) == len(want) == 3 * P + 3
    for i, (a, b) in enumerate(zip(got, want)):
        assert abs(a - b) <= REL * abs(b), (i, a, b)
    assert "predicting testing set batch 1 / %d" % len(test_loader) in out
    assert "current epoch: 3, predict %d points" % (P - 1) in out and "MAE: %.2f" % got[0] in out
    assert sorted(sw.rows) == sorted(f"{m}_{i}_points" for m in ("MAE", "RMSE", "MAPE") for i in range(P))
    assert sw.rows["RMSE_0_points"] == (got[1], 3)
    # the forward-only path is deterministic: a second pass scores the same bits
    assert TR.evaluate_on_test_mstgcn(net, test_loader, test_target, None, 4, mean, std) == got
