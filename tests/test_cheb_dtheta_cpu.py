"""The identity behind the in-kernel dTheta of the aggregate-first Chebyshev backward
(dstagnn_drought_amd/csrc/cheb_agg.hip, cheb_agg_spmm_t2_kernel<., ., DTH = true>), restated in
numpy float64 on a random sparse support.

With W_k[b] (N x N, zero off the support), x[b,i] (F x T) and g[b,j] = d(pre-ReLU X)[b,j] (T x C):

    forward     agg_k[b,j] = sum_i W_k[b,i,j] x[b,i]                       (F x T)
    old dTheta  dTheta_k   = sum_{b,j} agg_k[b,j] g[b,j]                   (F x C), needs agg_k saved
    backward    h_k[b,i]   = sum_j W_k[b,i,j] g[b,j]                       (T x C), the transposed SpMM's rows
    new dTheta  dTheta_k   = sum_{b,i} x[b,i] h_k[b,i]                     needs only x and h_k

Both are sum_{b,i,j} W_k[b,i,j] x[b,i] g[b,j]; the kernel forms the second per sample pair, with
the pair's h_k rows stacked (m = s T + t) and a lone last sample contributing its T rows only.
"""
import numpy as np
import pytest


def _case(B, N, F, T, C, K, deg, seed):
    rs = np.random.RandomState(seed)
    supp = np.eye(N, dtype=bool)
    for i in range(N):
        supp[i, rs.choice(N, deg, replace=False)] = True
    W = rs.standard_normal((B, K, N, N)) * supp  # zero off the support
    x = rs.standard_normal((B, N, F, T))
    g = rs.standard_normal((B, N, T, C))
    return supp, W, x, g


def _dtheta_from_agg(W, x, g):
    agg = np.einsum("bkij,bift->bjkft", W, x)      # the saved (B,N,K,F,T) tensor
    return np.einsum("bjkft,bjtc->kfc", agg, g)


def _dtheta_from_h_pairs(supp, W, x, g):
    """As the kernel walks it: per (sample pair, row i) the support entries of row i only, the
    pair's h_k rows stacked into one (2T x C) operand against the stacked x rows (F x 2T)."""
    B, K, N, _ = W.shape
    F, T, C = x.shape[2], x.shape[3], g.shape[3]
    out = np.zeros((K, F, C))
    for b0 in range(0, B, 2):
        nb = min(2, B - b0)
        for i in range(N):
            cols = np.nonzero(supp[i])[0]
            for k in range(K):
                hs = np.zeros((nb * T, C))
                xs = np.zeros((F, nb * T))
                for s in range(nb):
                    hs[s * T:(s + 1) * T] = np.einsum("j,jtc->tc", W[b0 + s, k, i, cols], g[b0 + s, cols])
                    xs[:, s * T:(s + 1) * T] = x[b0 + s, i]
                out[k] += xs @ hs
    return out


@pytest.mark.parametrize("B,N,F,T,C,K", [(3, 17, 5, 12, 8, 3),   # odd batch: one pair and a lone sample
                                         (1, 9, 1, 8, 4, 1),    # lone sample only, F = 1
                                         (4, 12, 6, 16, 6, 5)])
def test_dtheta_from_h_equals_dtheta_from_agg(B, N, F, T, C, K):
    supp, W, x, g = _case(B, N, F, T, C, K, deg=3, seed=B * 100 + N)
    a = _dtheta_from_agg(W, x, g)
    b = _dtheta_from_h_pairs(supp, W, x, g)
    # float64, sums of B*N*deg*T products of O(1) terms in two orders
    assert a.shape == b.shape == (K, F, C)
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(a).max())


def test_dense_h_matches_pairwise_walk():
    """h_k by one dense contraction gives the same dTheta as the pairwise support walk."""
    supp, W, x, g = _case(3, 11, 4, 12, 8, 2, deg=2, seed=5)
    h = np.einsum("bkij,bjtc->bkitc", W, g)
    a = np.einsum("bift,bkitc->kfc", x, h)
    b = _dtheta_from_h_pairs(supp, W, x, g)
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(a).max())
