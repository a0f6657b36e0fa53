"""numpy reference of the drought event counts (csrc/loss.hip events_kernel; include/dstagnn.h, the
events section) and of the scores read from them, used by tests/test_events_cpu.py and
tests/test_gpu_events.py.  No torch, no device.

Every compare is an np.float32 compare, as the kernel makes it.  The confusion matrix is filled with
np.add.at into int64; the 2 x 2 table of each threshold is counted DIRECTLY from the event masks, not
from the confusion matrix, so that the nesting identity the library relies on (event k + 1 implies
event k) is itself tested.  ``counts_naive`` is the same definition as a triple loop over (b, n, p).
"""
import numpy as np


def valid_target(t, marker):
    """The criterion's rule for fp32 targets: None marks nothing, NaN the NaN targets, a number the
    targets equal to it."""
    t = np.asarray(t, dtype=np.float32)
    if marker is None:
        return np.ones(t.shape, dtype=bool)
    return ~np.isnan(t) if marker != marker else t != np.float32(marker)


def _per_entry(thr, N):
    """thr (K,) or (K, N) -> (K, 1, N, 1) float32, ready to compare with (B, N, P)."""
    thr = np.asarray(thr, dtype=np.float32)
    if thr.ndim == 1:
        thr = np.repeat(thr[:, None], N, 1)
    assert thr.shape[1] == N
    return thr[:, None, :, None]


def excluded_nodes(thr, N):
    """(N,) bool: the nodes whose threshold column is all NaN (none for a (K,) set)."""
    thr = np.asarray(thr, dtype=np.float32)
    return np.zeros(N, dtype=bool) if thr.ndim == 1 else np.isnan(thr).all(0)


def event_masks(v, thr, direction):
    """(K, B, N, P) bool: event k of every value (fp32 compares; a NaN value is no event)."""
    v = np.asarray(v, dtype=np.float32)
    th = _per_entry(thr, v.shape[1])
    with np.errstate(invalid="ignore"):
        return v[None] <= th if direction == "below" else v[None] >= th


def classes(v, thr, direction):
    """(B, N, P) int64: the number of events each value is."""
    return event_masks(v, thr, direction).sum(0).astype(np.int64)


def _selection(pred, target, thr, marker):
    pred, target = np.asarray(pred, dtype=np.float32), np.asarray(target, dtype=np.float32)
    counted = valid_target(target, marker) & ~excluded_nodes(thr, target.shape[1])[None, :, None]
    return pred, target, counted, counted & np.isnan(pred)


def counts(pred, target, thr, direction, marker=None):
    """{"horizon": (P, cols), "node": (N, cols)} int64 with cols = 2 + (K + 1)^2: column 0 the counted
    entries, 1 those with a NaN prediction, 2 + co (K + 1) + cf the cells."""
    pred, target, counted, nanp = _selection(pred, target, thr, marker)
    B, N, P = target.shape
    K1 = np.asarray(thr).shape[0] + 1
    co, cf = classes(target, thr, direction), classes(pred, thr, direction)
    cell = 2 + co * K1 + cf
    cell = np.where(nanp, 1, cell)
    hor, node = np.zeros((P, 2 + K1 * K1), dtype=np.int64), np.zeros((N, 2 + K1 * K1), dtype=np.int64)
    b, n, p = np.nonzero(counted)
    np.add.at(hor, (p, cell[b, n, p]), 1)
    np.add.at(node, (n, cell[b, n, p]), 1)
    np.add.at(hor, (p, 0), 1)
    np.add.at(node, (n, 0), 1)
    return {"horizon": hor, "node": node}


def counts_naive(pred, target, thr, direction, marker=None):
    """The same counts as a loop over every (b, n, p), straight from the definitions."""
    pred, target = np.asarray(pred, dtype=np.float32), np.asarray(target, dtype=np.float32)
    thr = np.asarray(thr, dtype=np.float32)
    B, N, P = target.shape
    K = thr.shape[0]
    hor, node = np.zeros((P, 2 + (K + 1) ** 2), dtype=np.int64), np.zeros((N, 2 + (K + 1) ** 2), dtype=np.int64)

    def cls(v, th):
        c = 0
        for k in range(K):
            if (v <= th[k]) if direction == "below" else (v >= th[k]):
                c += 1
        return c
    for n in range(N):
        th = thr if thr.ndim == 1 else thr[:, n]
        if np.isnan(th).all():
            continue
        for b in range(B):
            for p in range(P):
                y, t = pred[b, n, p], target[b, n, p]
                if marker is not None and (np.isnan(t) if marker != marker else t == np.float32(marker)):
                    continue
                col = 1 if np.isnan(y) else 2 + cls(t, th) * (K + 1) + cls(y, th)
                for tab, r in ((hor, p), (node, n)):
                    tab[r, 0] += 1
                    tab[r, col] += 1
    return {"horizon": hor, "node": node}


def two_by_two(pred, target, thr, direction, marker=None):
    """{"horizon": (P, K, 4), "node": (N, K, 4)} int64: hits, false alarms, misses and correct
    negatives of every threshold, counted from the event masks of the entries that reach a cell."""
    pred, target, counted, nanp = _selection(pred, target, thr, marker)
    use = counted & ~nanp
    eo, ef = event_masks(target, thr, direction), event_masks(pred, thr, direction)
    quad = np.stack([eo & ef, ~eo & ef, eo & ~ef, ~eo & ~ef], -1) & use[None, ..., None]   # (K, B, N, P, 4)
    return {"horizon": quad.sum((1, 2)).transpose(1, 0, 2).astype(np.int64),
            "node": quad.sum((1, 3)).transpose(1, 0, 2).astype(np.int64)}


def _over(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    out = np.full(a.shape, np.nan)
    ok = (b != 0) & ~np.isnan(b) & ~np.isnan(a)
    out[ok] = a[ok] / b[ok]
    return out


def scores(tab, quads, overall=True):
    """The scores from a (R, cols) table of counts and the directly counted (R, K, 4) 2 x 2 tables,
    written out; NaN where a divisor is 0.  With ``overall`` one more row from the column sums."""
    tab, quads = np.asarray(tab, dtype=np.float64), np.asarray(quads, dtype=np.float64)
    if overall:
        tab = np.concatenate([tab, tab.sum(0, keepdims=True)], 0)
        quads = np.concatenate([quads, quads.sum(0, keepdims=True)], 0)
    R = tab.shape[0]
    K1 = int(round(np.sqrt(tab.shape[1] - 2)))
    M = tab[:, 2:].reshape(R, K1, K1)
    n = M.sum((1, 2))
    a, b, c, d = (quads[..., i] for i in range(4))
    nn = a + b + c + d
    a_r = _over((a + b) * (a + c), nn)
    p = _over(M, n[:, None, None])
    diag = np.stack([p[:, i, i] for i in range(K1)], 1).sum(1)
    chance = (p.sum(2) * p.sum(1)).sum(1)
    return {"count": tab[:, 0], "nan_pred": tab[:, 1], "confusion": M,
            "observed_freq": _over(M.sum(2), n[:, None]), "forecast_freq": _over(M.sum(1), n[:, None]),
            "hits": a, "false_alarms": b, "misses": c, "correct_negatives": d,
            "base_rate": _over(a + c, nn), "pod": _over(a, a + c), "far": _over(b, a + b), "pofd": _over(b, b + d),
            "csi": _over(a, a + b + c), "freq_bias": _over(a + b, a + c), "accuracy": _over(a + d, nn),
            "ets": _over(a - a_r, a + b + c - a_r),
            "hss": _over(2.0 * (a * d - b * c), (a + c) * (c + d) + (a + b) * (b + d)),
            "class_accuracy": _over(np.stack([M[:, i, i] for i in range(K1)], 1).sum(1), n),
            "hss_multi": _over(diag - chance, 1.0 - chance)}


def grid(thr):
    """The values that probe one threshold set (K,): each threshold's fp32 value, its two
    np.nextafter neighbours, and one value beyond either end; float32, 3 K + 2 of them."""
    thr = np.asarray(thr, dtype=np.float32).reshape(-1)
    inf = np.float32(np.inf)
    vals = [np.float32(thr.min() - 1.0), np.float32(thr.max() + 1.0)]
    for t in thr:
        vals += [t, np.nextafter(t, -inf), np.nextafter(t, inf)]
    return np.array(vals, dtype=np.float32)


def draw(rng, thr, shape):
    """A (B, N, P) float32 array drawn uniformly from grid(thr) (for a (K, N) table: each node from
    the grid of its own column; an excluded node from the grid of the row means)."""
    thr = np.asarray(thr, dtype=np.float32)
    B, N, P = shape
    K = thr.shape[0]
    if thr.ndim == 1:
        return grid(thr)[rng.integers(0, 3 * K + 2, shape)]
    fallback = np.nanmean(thr.astype(np.float64), 1).astype(np.float32)
    G = np.stack([grid(fallback if np.isnan(thr[:, n]).all() else thr[:, n]) for n in range(N)])   # (N, 3 K + 2)
    return G[np.arange(N)[None, :, None], rng.integers(0, 3 * K + 2, shape)]
