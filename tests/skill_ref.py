"""numpy reference of the baseline skill sums (csrc/loss.hip skill_kernel, csrc/windows.hip
climatology_kernel; include/dstagnn.h, the skill section), used by tests/test_skill_cpu.py and
tests/test_gpu_skill.py.  No torch, no device.

The climatology and the persistence values are built from the series in float64 / the series' own
dtype; the differences and the squares of columns 1, 2, 6, 7 are formed with np.float32 arithmetic,
as the kernel forms them; the anomaly products and every sum are float64.  ``skill_sums`` is
vectorised; ``skill_sums_naive`` is the same definition as a triple loop over (b, n, p), for a
check of the vectorised one on a tiny case.
"""
import numpy as np

COLS = 13


def missing(v, marker):
    """The windows section's rule for series elements: None marks nothing, NaN the NaN elements,
    a number the elements equal to it in the series' dtype."""
    v = np.asarray(v)
    if marker is None:
        return np.zeros(v.shape, dtype=bool)
    if marker != marker:
        return np.isnan(v)
    return v == v.dtype.type(marker)


def valid_target(t, marker):
    """The criterion's rule for fp32 targets."""
    t = np.asarray(t, dtype=np.float32)
    if marker is None:
        return np.ones(t.shape, dtype=bool)
    return ~np.isnan(t) if marker != marker else t != np.float32(marker)


def climatology(series, period, t_end, marker):
    """(clim (period, N) float64, cnt (period, N) int32): the mean of the observed
    series[t, n, F - 1] over t in [0, t_end) with t % period == phase, added in increasing t."""
    s = np.asarray(series)[:, :, -1]
    miss = missing(s, marker)
    N = s.shape[1]
    tot, cnt = np.zeros((period, N), dtype=np.float64), np.zeros((period, N), dtype=np.int32)
    for t in range(int(t_end)):
        ok = ~miss[t]
        tot[t % period, ok] += s[t, ok].astype(np.float64)
        cnt[t % period, ok] += 1
    clim = np.full((period, N), np.nan)
    np.divide(tot, cnt, out=clim, where=cnt > 0)
    return clim, cnt


def persistence(series, pos, marker):
    """(q (B, N) in the series' dtype, defined (B, N) bool): the latest observed
    series[t, n, F - 1] with t <= pos[b] - 1, at any distance back."""
    s = np.asarray(series)[:, :, -1]
    L, N = s.shape
    miss = missing(s, marker)
    last = np.full((L, N), -1, dtype=np.int64)  # the latest observed step <= t
    cur = np.full(N, -1, dtype=np.int64)
    for t in range(L):
        cur = np.where(miss[t], cur, t)
        last[t] = cur
    pos = np.asarray(pos, dtype=np.int64)
    q, ok = np.zeros((len(pos), N), dtype=s.dtype), np.zeros((len(pos), N), dtype=bool)
    for b, l in enumerate(pos):
        if 1 <= l <= L:
            src = last[l - 1]
            ok[b] = src >= 0
            q[b] = np.where(ok[b], s[np.maximum(src, 0), np.arange(N)], 0)
    return q, ok


def entry_terms(pred, target, pos, series, period, t_end, target_marker, series_marker):
    """(B, N, P, 13) float64: what each entry adds to each column (0 where it is selected out)."""
    pred, target = np.asarray(pred, dtype=np.float32), np.asarray(target, dtype=np.float32)
    B, N, P = target.shape
    L = np.asarray(series).shape[0]
    pos = np.asarray(pos, dtype=np.int64)
    clim, cnt = climatology(series, period, t_end, series_marker)
    q, qok = persistence(series, pos, series_marker)
    inside = (pos >= 0) & (pos + P <= L)
    phase = (np.where(inside, pos, 0)[:, None] + np.arange(P)[None, :]) % period            # (B, P)
    c32 = clim[phase[:, None, :], np.arange(N)[None, :, None]].astype(np.float32)           # (B, N, P)
    cok = cnt[phase[:, None, :], np.arange(N)[None, :, None]] > 0
    q32 = np.broadcast_to(q.astype(np.float32)[:, :, None], target.shape)
    ok = valid_target(target, target_marker) & inside[:, None, None]
    sp, sc = ok & qok[:, :, None], ok & cok
    with np.errstate(invalid="ignore", over="ignore"):
        em = pred - target
        ep, ec, af, ao = q32 - target, c32 - target, pred - c32, target - c32
        em2, ema = (em * em).astype(np.float64), np.abs(em).astype(np.float64)
        af64, ao64 = af.astype(np.float64), ao.astype(np.float64)
        cols = [(sp, np.ones_like(ema)), (sp, em2), (sp, (ep * ep).astype(np.float64)), (sp, ema),
                (sp, np.abs(ep).astype(np.float64)),
                (sc, np.ones_like(ema)), (sc, em2), (sc, (ec * ec).astype(np.float64)), (sc, ema),
                (sc, np.abs(ec).astype(np.float64)), (sc, af64 * ao64), (sc, af64 * af64), (sc, ao64 * ao64)]
    return np.stack([np.where(sel, term, 0.0) for sel, term in cols], -1)


def skill_sums(pred, target, pos, series, period, t_end, target_marker=None, series_marker=None):
    """{"horizon": (P, 13), "node": (N, 13)} float64 sums, and the same two of the terms'
    magnitudes (the scale of an add-order difference): (sums, mags)."""
    terms = entry_terms(pred, target, pos, series, period, t_end, target_marker, series_marker)
    with np.errstate(invalid="ignore"):
        sums = {"horizon": terms.sum(axis=(0, 1)), "node": terms.sum(axis=(0, 2))}
        mags = {"horizon": np.abs(terms).sum(axis=(0, 1)), "node": np.abs(terms).sum(axis=(0, 2))}
    return sums, mags


def skill_sums_naive(pred, target, pos, series, period, t_end, target_marker=None, series_marker=None):
    """The same sums written as a loop over every (b, n, p), straight from the definitions."""
    pred, target = np.asarray(pred, dtype=np.float32), np.asarray(target, dtype=np.float32)
    series = np.asarray(series)
    B, N, P = target.shape
    L = series.shape[0]

    def is_missing(v):
        if series_marker is None:
            return False
        return bool(np.isnan(v)) if series_marker != series_marker else bool(v == series.dtype.type(series_marker))

    def is_valid(t):
        if target_marker is None:
            return True
        return not np.isnan(t) if target_marker != target_marker else bool(t != np.float32(target_marker))
    hor, node = np.zeros((P, COLS)), np.zeros((N, COLS))
    for b in range(B):
        l = int(pos[b])
        if l < 0 or l + P > L:
            continue
        for n in range(N):
            q = None
            for t in range(l - 1, -1, -1):
                if not is_missing(series[t, n, -1]):
                    q = np.float32(series[t, n, -1])
                    break
            for p in range(P):
                y, t = pred[b, n, p], target[b, n, p]
                if not is_valid(t):
                    continue
                vals = [float(series[s, n, -1]) for s in range((l + p) % period, t_end, period)
                        if not is_missing(series[s, n, -1])]
                add = np.zeros(COLS)
                em = np.float32(y - t)
                if q is not None:
                    ep = np.float32(q - t)
                    add[0:5] = [1.0, float(np.float32(em * em)), float(np.float32(ep * ep)), abs(float(em)),
                                abs(float(ep))]
                if vals:
                    tot = 0.0
                    for v in vals:
                        tot += v
                    c = np.float32(tot / len(vals))
                    ec, af, ao = np.float32(c - t), np.float32(y - c), np.float32(t - c)
                    add[5:13] = [1.0, float(np.float32(em * em)), float(np.float32(ec * ec)), abs(float(em)),
                                 abs(float(ec)), float(af) * float(ao), float(af) * float(af), float(ao) * float(ao)]
                hor[p] += add
                node[n] += add
    return {"horizon": hor, "node": node}


def scores(tab, overall=True):
    """The scores of a (K, 13) table, written out; NaN where a divisor is 0."""
    tab = np.asarray(tab, dtype=np.float64)
    if overall:
        tab = np.concatenate([tab, tab.sum(0, keepdims=True)], 0)

    def over(a, b):
        out = np.full(a.shape, np.nan)
        np.divide(a, b, out=out, where=b != 0)
        return out
    out = {}
    for name, c in (("persistence", 0), ("climatology", 5)):
        n = tab[:, c]
        out["count_" + name] = n
        out["model_rmse_" + name], out["rmse_" + name] = np.sqrt(over(tab[:, c + 1], n)), np.sqrt(over(tab[:, c + 2], n))
        out["model_mae_" + name], out["mae_" + name] = over(tab[:, c + 3], n), over(tab[:, c + 4], n)
        out["mse_skill_" + name] = 1.0 - over(tab[:, c + 1], tab[:, c + 2])
        out["mae_skill_" + name] = 1.0 - over(tab[:, c + 3], tab[:, c + 4])
    out["acc"] = over(tab[:, 10], np.sqrt(tab[:, 11] * tab[:, 12]))
    return out


def gapped_series(L, N, F, dtype, marker, seed, period=12, t_end=None, lead=None):
    """A seasonal (L, N, F) series with the gaps the tests need (marker None: no gaps): node 0 has a
    leading gap of `lead` steps (3 L / 4 by default: no persistence value for a long time), node 1
    (where N > 1) is never observed in phase 1 of `period` before t_end, and ~15 % of everything else
    is missing."""
    rng = np.random.default_rng(seed)
    t = np.arange(L)[:, None, None]
    s = 10.0 + 3.0 * np.sin(2 * np.pi * t / period + np.arange(N)[None, :, None]) + rng.normal(0, 1, (L, N, F))
    s = s.astype(dtype)
    if marker is None:
        return s
    s[rng.random((L, N, F)) < 0.15] = marker
    s[: max(1, (3 * L) // 4 if lead is None else lead), 0, :] = marker
    if N > 1:
        stop = L if t_end is None else t_end
        s[np.arange(1 % period, stop, period), 1, :] = marker      # phase 1 of node 1: never observed in training
    return s
