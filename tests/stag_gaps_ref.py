"""numpy / scipy reference of the STAG graph on a series with gaps (TEST INFRASTRUCTURE ONLY:
imported by tests/test_emd_rect_cpu.py, test_stag_gaps_cpu.py and test_gpu_stag_gaps.py, never
by the product path).  Built on oracle/stag_ref.py, which stays the LP solver of record
(emd_linprog = the reference's scipy linprog/HiGHS call).

Semantics.  An element is missing when it is nan (missing_value nan) or == the
marker; a step of a node is observed when none of its F features is missing.  The masked EMD of
a pair is the transport cost between the two nodes' norm distributions, each on its own observed
steps.  Two equivalent statements of that LP:

  zero_marginal_problem  the full T x T problem of the reference with p_t = 0 / q_t = 0 at the
                         missing steps and a finite cost there (no mass can move through them);
                         solved by oracle.stag_ref.emd_linprog unchanged — the form the tests use
  reduced_problem        only the observed rows and columns (Tr x Tc), what the device solves
"""
import numpy as np

from oracle import stag_ref as ref


def is_missing(data, missing_value):
    """Element-wise rule of include/dstagnn.h: nan marker -> v != v, else IEEE v == marker."""
    data = np.asarray(data, dtype=np.float64)
    if missing_value != missing_value:
        return data != data
    return data == np.float64(missing_value)


def observed(data, missing_value):
    """data (..., F) -> (...) bool: no feature of the step is missing."""
    return ~is_missing(data, missing_value).any(axis=-1)


def _norms(x, obs):
    """(T, F), (T) -> unit rows (T, F) and marginal (T), zeros at the missing steps."""
    xz = np.where(obs[:, None], x, 0.0)
    nr = np.linalg.norm(xz, axis=1, keepdims=True)
    nr[nr == 0] = 1e-12                                  # data/STAG_gen.py:48-49, observed zero rows
    xh = xz / nr
    p = np.where(obs, nr[:, 0], 0.0)
    p = p / (p.sum() + 1e-12)
    return xh, p


def zero_marginal_problem(x, y, ox, oy):
    """The reference's T x T LP with zero marginals at the missing steps -> p (T), q (T), D (T, T)."""
    xh, p = _norms(x, ox)
    yh, q = _norms(y, oy)
    D = np.clip(np.nan_to_num(1 - xh @ yh.T, nan=1.0), 0, 1)
    D[~ox, :] = 0.5                                      # any finite cost: no mass there
    D[:, ~oy] = 0.5
    return p, q, D


def reduced_problem(x, y, ox, oy):
    """Only the observed rows / columns -> xh (Tr, F), yh (Tc, F), p (Tr), q (Tc), D (Tr, Tc)."""
    xh, p = _norms(x, ox)
    yh, q = _norms(y, oy)
    xh, p, yh, q = xh[ox], p[ox], yh[oy], q[oy]
    D = np.clip(np.nan_to_num(1 - xh @ yh.T, nan=1.0), 0, 1)
    return np.ascontiguousarray(xh), np.ascontiguousarray(yh), np.ascontiguousarray(p), np.ascontiguousarray(q), D


def rect_linprog(p, q, D):
    """linprog/HiGHS on a Tr x Tc transportation problem (emd_linprog is square only); 1.0 on failure."""
    from scipy.optimize import linprog
    nr, nc = len(p), len(q)
    if nr == 0 or nc == 0:
        return 1.0
    A = np.zeros((nr + nc, nr * nc))
    for i in range(nr):
        A[i, i * nc:(i + 1) * nc] = 1
    for j in range(nc):
        A[nr + j, j::nc] = 1
    r = linprog(D.reshape(-1), A_eq=A, b_eq=np.concatenate([p, q]), method="highs")
    return r.fun if r.success else 1.0


def masked_emd(x, y, ox, oy, min_observed=1):
    """The masked EMD of one pair by emd_linprog on the zero-marginal problem; 1.0 for a pair
    with an excluded node (fewer than min_observed observed steps)."""
    if ox.sum() < min_observed or oy.sum() < min_observed:
        return 1.0
    return ref.emd_linprog(*zero_marginal_problem(x, y, ox, oy))


def sta_matrix(data, missing_value, min_observed=1):
    """All pairs of data (T, N, F), symmetric, zero diagonal."""
    obs = observed(data, missing_value)
    n = data.shape[1]
    sta = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            sta[i, j] = masked_emd(data[:, i], data[:, j], obs[:, i], obs[:, j], min_observed)
    return sta + sta.T


def prep(data, missing_value):
    """numpy statement of the masked prep: count (N), tidx (N, T) (-1 padded), p (N, T)
    compacted marginals (0 padded)."""
    T, N, _ = data.shape
    obs = observed(data, missing_value)
    count = obs.sum(0).astype(np.int32)
    tidx = np.full((N, T), -1, np.int32)
    p = np.zeros((N, T))
    for n in range(N):
        steps = np.flatnonzero(obs[:, n])
        tidx[n, :len(steps)] = steps
        p[n, :len(steps)] = _norms(data[:, n], obs[:, n])[1][steps]
    return count, tidx, p


def adjacency(sta, sparsity, exclude):
    """oracle.stag_ref.stag_adjacency with excluded nodes: adj = 1 - sta + I, per non-excluded
    row the first min(top, #eligible) eligible columns of a stable argsort -> A, R, nbr (-1
    padded); an excluded row stays zero."""
    n = sta.shape[0]
    exclude = np.asarray(exclude, dtype=bool)
    adj = 1 - sta + np.identity(n)
    top = max(1, int(n * sparsity))
    A, R = np.zeros_like(adj), np.zeros_like(adj)
    nbr = np.full((n, top), -1, np.int32)
    for i in range(n):
        if exclude[i]:
            continue
        order = np.argsort(adj[i], kind="stable")
        nb = order[~exclude[order]][:top]
        A[i, nb] = 1
        R[i, nb] = adj[i, nb]
        nbr[i, :len(nb)] = nb
    return A, R, nbr
