"""GPU: the calibration sums of quantile forecasts (csrc/loss.hip metrics_quantile_kernel;
QuantileMetrics) against a float64 numpy restatement on the same fp32 inputs.

Inputs are seeded: t = 3 randn, pred_q = t + randn + offset_q sorted along q, then the Q predictions
of 10 % of the entries shuffled (so the crossing count is non-trivial), 30 % of the targets marked
(-9999 for the != mode, NaN for the NaN mode, none under the no-mask mode).

Bounds (derived; none of them measured):
  counts (valid, hits, crossings)  exact: fp32 compares, sums of ones in fp64.
  pinball sums   <= 1e-6 relative: non-negative terms of at most three fp32 roundings, fp64 adds.
  sums of pred   within 1e-12 of the sum of |pred|: every term is exact as a double, so only the
                 add order differs; a sum passes through fewer than 400 adds on its way (B per
                 thread, 256 / P or P in LDS, one per workgroup), 400 * 2^-53 = 4.4e-14.
  merge(), split updates, node-table column sums against the horizon table's: within 1e-12 of the
                 sum of |term| (add order alone).

Measured on the MI355X, worst over the cases below: pinball sums 7.8e-8; the sums of pred equal the
restatement's to the last bit.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
REL, ORDER = 1e-6, 1e-12
MODES = {"none": None, "neq": -9999.0, "nan": NAN}

# (B, N, P, Q), the sizes of the updates along B, (emptied horizon, emptied node) / "all" / None
CASES = {
    "1x1x1xQ1-valid": ((1, 1, 1, 1), [1], None),
    "1x1x1xQ1-masked": ((1, 1, 1, 1), [1], "all"),
    "5x101x3xQ3-two-updates": ((5, 101, 3, 3), [2, 3], None),
    "4x170x12xQ3-pems08-head": ((4, 170, 12, 3), [4], None),
    "3x7x19xQ7-emptied": ((3, 7, 19, 7), [3], (5, 2)),
    "2x9x129xQ2-tn1-idle": ((2, 9, 129, 2), [2], None),
    "2x5x256xQ16-limits": ((2, 5, 256, 16), [2], None),
    "6x2200x12xQ5-105-workgroups": ((6, 2200, 12, 5), [6], None),
}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def levels_of(Q):
    return tuple((q + 1.0) / (Q + 1.0) for q in range(Q))


def _valid(t, marker):
    if marker is None:
        return np.ones(t.shape, dtype=bool)
    return ~np.isnan(t) if marker != marker else t != np.float32(marker)


@functools.lru_cache(maxsize=None)
def _inputs(case, mode, shuffle=True):
    """(pred (B, N, P, Q), target (B, N, P)) fp32 numpy arrays, made once and shared."""
    (B, N, P, Q), _, emptied = CASES[case]
    marker = MODES[mode]
    g = torch.Generator().manual_seed(7000 + 13 * list(CASES).index(case))
    t = 3.0 * torch.randn(B, N, P, generator=g)
    off = torch.linspace(-1.0, 1.0, Q) if Q > 1 else torch.zeros(1)
    p = (t[..., None] + torch.randn(B, N, P, Q, generator=g) + off).sort(dim=-1).values
    if shuffle and Q > 1:
        perm = torch.rand(B, N, P, Q, generator=g).argsort(dim=-1)
        pick = (torch.rand(B, N, P, generator=g) < 0.1)[..., None]
        p = torch.where(pick, p.gather(-1, perm), p)
    if marker is not None:
        if t.numel() > 1:
            t[torch.rand(B, N, P, generator=g) < 0.3] = marker
        if emptied == "all":
            t[...] = marker
        elif emptied is not None:
            t[:, :, emptied[0]] = marker
            t[:, emptied[1], :] = marker
    return p.contiguous().numpy(), t.numpy()


def ref_sums(p, t, levels, marker, axes):
    """The 2 + 3 Q float64 sums over the valid entries reduced over `axes` of (B, N, P): (K, cols), and
    the sums of the terms' magnitudes."""
    tau32 = np.asarray(levels, dtype=np.float32)
    tau, omt = tau32.astype(np.float64), (np.float32(1.0) - tau32).astype(np.float64)
    v = _valid(t, marker)
    tz = np.where(v, t, np.float32(0.0))
    d = p.astype(np.float64) - tz.astype(np.float64)[..., None]
    term = np.where(d > 0, omt * d, np.where(d < 0, tau * -d, 0.0))
    hit = tz[..., None] <= p  # fp32 compare
    cross = (np.diff(p, axis=-1) < 0).any(-1) if p.shape[-1] > 1 else np.zeros(t.shape, dtype=bool)
    cols = [v.astype(np.float64), (v & cross).astype(np.float64)]
    for q in range(p.shape[-1]):
        cols += [np.where(v, term[..., q], 0.0), (v & hit[..., q]).astype(np.float64),
                 np.where(v, p[..., q].astype(np.float64), 0.0)]
    sums = np.stack([c.sum(axis=axes) for c in cols], -1)
    mags = np.stack([np.abs(c).sum(axis=axes) for c in cols], -1)
    return sums, mags


def check_table(what, got, want, mags):
    Q = (want.shape[1] - 2) // 3
    exact = [0, 1] + [3 + 3 * q for q in range(Q)]
    assert np.array_equal(got[:, exact], want[:, exact]), f"{what}: a count differs"
    pin = [2 + 3 * q for q in range(Q)]
    err = np.abs(got[:, pin] - want[:, pin])
    worst = float(np.max(err / np.where(want[:, pin] != 0, want[:, pin], 1.0)))
    assert np.all(err <= REL * want[:, pin]), f"{what}: pinball sums, worst relative error {worst:.3e}"
    sy = [4 + 3 * q for q in range(Q)]
    serr = np.abs(got[:, sy] - want[:, sy])
    assert np.all(serr <= ORDER * mags[:, sy]), f"{what}: sums of pred off by {float(serr.max()):.3e}"
    print(f"{what}: pinball worst rel {worst:.2e}, sum-of-pred worst abs {float(serr.max()):.2e}")


def run_hip(case, mode, nodes=True, shuffle=True):
    from dstagnn_drought_amd import QuantileMetrics
    (B, N, P, Q), splits, _ = CASES[case]
    p, t = _inputs(case, mode, shuffle)
    m = QuantileMetrics(P, levels_of(Q), missing_value=MODES[mode], num_nodes=N if nodes else None, device="cuda")
    pd, td = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
    at = 0
    for n in splits:
        m.update(pd[at:at + n], td[at:at + n])
        at += n
    assert at == B
    return m, p, t


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("case", list(CASES))
def test_tables_vs_float64(case, mode):
    _need_gpu()
    (B, N, P, Q), _, emptied = CASES[case]
    if emptied is not None and MODES[mode] is None:
        emptied = None
    m, p, t = run_hip(case, mode)
    assert m.table.shape == (P, 2 + 3 * Q) and m.node_table.shape == (N, 2 + 3 * Q)
    hw, hm = ref_sums(p, t, levels_of(Q), MODES[mode], (0, 1))
    nw, nm = ref_sums(p, t, levels_of(Q), MODES[mode], (0, 2))
    ht, nt = m.table.cpu().numpy(), m.node_table.cpu().numpy()
    check_table(f"{case}/{mode} horizon", ht, hw, hm)
    check_table(f"{case}/{mode} node", nt, nw, nm)
    # the two tables are two reductions of the same terms
    assert np.all(np.abs(nt.sum(0) - ht.sum(0)) <= ORDER * hm.sum(0))
    if Q > 1 and B * N * P > 100:
        assert 0 < hw[:, 1].sum() < hw[:, 0].sum()  # some entries cross, not all
    s = m.scores()
    assert s["count"].shape == (P + 1,) and s["coverage"].shape == (P + 1, Q)
    assert s["interval_width"].shape == (P + 1, Q // 2) == s["interval_coverage"].shape
    assert s["count"][-1] == hw[:, 0].sum()
    if emptied == "all":
        assert all(np.isnan(v).all() for k, v in s.items() if k != "count") and s["count"].tolist() == [0.0, 0.0]
    elif emptied is not None:
        ns = m.node_scores()
        assert s["count"][emptied[0]] == 0 and np.isnan(s["coverage"][emptied[0]]).all()
        assert ns["count"][emptied[1]] == 0 and np.isnan(ns["mean_pinball"][emptied[1]])
        assert np.isfinite(s["mean_pinball"][-1]) and ns["count"].shape == (N,)
    # without the node table: the same horizon bits
    m2, _, _ = run_hip(case, mode, nodes=False)
    assert m2.node_table is None and torch.equal(m2.table, m.table)
    with pytest.raises(ValueError):
        m2.node_scores()


@pytest.mark.parametrize("case", ["5x101x3xQ3-two-updates", "6x2200x12xQ5-105-workgroups"])
def test_same_bits_on_every_call_merge_and_split_updates(case):
    _need_gpu()
    from dstagnn_drought_amd import QuantileMetrics
    (B, N, P, Q), _, _ = CASES[case]
    a, p, t = run_hip(case, "nan")
    b, _, _ = run_hip(case, "nan")
    assert torch.equal(a.table, b.table) and torch.equal(a.node_table, b.node_table)
    _, mags = ref_sums(p, t, levels_of(Q), NAN, (0, 1))
    _, nmags = ref_sums(p, t, levels_of(Q), NAN, (0, 2))
    pd, td = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
    kw = dict(missing_value=NAN, num_nodes=N, device="cuda")
    one, x, y = (QuantileMetrics(P, levels_of(Q), **kw) for _ in range(3))
    one.update(pd, td)
    x.update(pd[:1], td[:1])
    y.update(pd[1:], td[1:])
    x.merge(y)
    for got in (a, x):  # split updates, and a merge of two objects
        assert np.all(np.abs(got.table.cpu().numpy() - one.table.cpu().numpy()) <= ORDER * mags)
        assert np.all(np.abs(got.node_table.cpu().numpy() - one.node_table.cpu().numpy()) <= ORDER * nmags)
    with pytest.raises(ValueError):
        x.merge(QuantileMetrics(P, levels_of(Q), missing_value=-9999.0, num_nodes=N, device="cuda"))
    x.reset()
    assert not x.table.any() and not x.node_table.any()
    assert x.all_reduce() is x  # no process group: nothing to do
    with pytest.raises(ValueError):
        x.update(pd[..., :Q - 1], td)
    with pytest.raises(RuntimeError, match="HIP"):
        x.update(pd.cpu(), td.cpu())


@pytest.mark.parametrize("case", ["4x170x12xQ3-pems08-head", "6x2200x12xQ5-105-workgroups", "2x5x256xQ16-limits"])
def test_interval_coverage_is_exact_where_nothing_crosses(case):
    _need_gpu()
    (B, N, P, Q), _, _ = CASES[case]
    m, p, t = run_hip(case, "neq", shuffle=False)
    tab = m.table.cpu().numpy()
    assert not tab[:, 1].any()  # well ordered
    v = _valid(t, -9999.0)
    s = m.scores()
    for k in range(Q // 2):
        lo, hi = k, Q - 1 - k
        inside = (v & (p[..., lo] < t) & (t <= p[..., hi])).sum(axis=(0, 1)).astype(np.float64)
        assert np.array_equal(tab[:, 3 + 3 * hi] - tab[:, 3 + 3 * lo], inside)  # the counts, exactly
        n = tab[:, 0]
        assert np.array_equal(s["interval_coverage"][:-1, k], tab[:, 3 + 3 * hi] / n - tab[:, 3 + 3 * lo] / n)
        assert np.all(np.abs(s["interval_coverage"][:-1, k] - inside / n) <= 2.0 ** -52)
        assert abs(s["interval_coverage"][-1, k] - inside.sum() / n.sum()) <= 2.0 ** -52
        assert np.all(s["interval_width"][:, k] > 0)
