"""CPU: the rectangular entry of the network-simplex EMD solver (csrc/emd_simplex.hpp, Tr rows x
Tc columns; host build tests/native/emd_rect_host.cpp) against scipy linprog/HiGHS.

A series with gaps gives every node a distribution on its own observed steps, so a pair's
transportation problem is cnt[i] x cnt[j].  The reference of record is
oracle.stag_ref.emd_linprog on the equivalent full T x T problem with zero marginals at the
missing steps (tests/stag_gaps_ref.py).  Tolerance: |difference| <= 1e-9, the project's EMD
tolerance (tests/test_emd_solver_cpu.py), status 0.  The GPU kernel runs the same solver code
(tests/test_gpu_stag_gaps.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import stag_gaps_ref as gref
from oracle import stag_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_D = ctypes.POINTER(ctypes.c_double)
_I = ctypes.POINTER(ctypes.c_int)
_L = ctypes.POINTER(ctypes.c_longlong)


def _lib(name):
    path = os.path.join(ROOT, "tests", "native", name)
    if not os.path.exists(path):
        subprocess.run(["make", "-C", ROOT, f"tests/native/{name}"], check=True)
    return ctypes.CDLL(path)


def _ptr(a):
    return a.ctypes.data_as(_D)


@pytest.fixture(scope="module")
def rect():
    lib = _lib("libemd_rect_host.so")
    lib.emd_rect_host.restype = ctypes.c_double
    lib.emd_rect_host.argtypes = [_D, _D, _D, _D, _D, ctypes.c_int, ctypes.c_int, ctypes.c_int, _I, _L]

    def solve(xh, yh, p, q):
        st, pv = ctypes.c_int(-1), ctypes.c_longlong(-1)
        xh, yh, p, q = (np.ascontiguousarray(a, dtype=np.float64) for a in (xh, yh, p, q))
        r = lib.emd_rect_host(_ptr(xh), _ptr(yh), _ptr(p), _ptr(q), None, len(p), len(q), xh.shape[1],
                              ctypes.byref(st), ctypes.byref(pv))
        return r, st.value, pv.value
    return solve


@pytest.fixture(scope="module")
def square():
    lib = _lib("libemd_host.so")
    lib.emd_host.restype = ctypes.c_double
    lib.emd_host.argtypes = [_D, _D, _D, _D, _D, ctypes.c_int, ctypes.c_int, _I, _L]

    def solve(xh, yh, p, q):
        st, pv = ctypes.c_int(-1), ctypes.c_longlong(-1)
        r = lib.emd_host(_ptr(xh), _ptr(yh), _ptr(p), _ptr(q), None, len(p), xh.shape[1], ctypes.byref(st),
                         ctypes.byref(pv))
        return r, st.value, pv.value
    return solve


def _mask(rs, T, share):
    """(T) bool observed steps, at least one."""
    o = rs.rand(T) >= share
    if not o.any():
        o[rs.randint(T)] = True
    return o


def _masked_case(rs, T, k):
    """Case k of length T: x, y (T, F) and their observed steps."""
    F = 1 + k % 4
    x, y = rs.randn(T, F), rs.randn(T, F)
    ox = _mask(rs, T, (0.0, 0.1, 0.3, 0.6, 0.9)[k % 5])       # shares set independently per node
    oy = _mask(rs, T, (0.3, 0.9, 0.0, 0.1, 0.6, 0.45)[k % 6])
    if k % 4 == 1:
        y, oy = x.copy(), ox.copy()                             # identical series on a common support
    if k % 4 == 2:
        x, y = np.abs(x), np.abs(y)                             # non-negative: costs clipped at 0 / small
    if k % 4 == 3:
        if T > 1:
            x[::3] = 0.0                                        # observed zero rows: 1e-12 guards
            ox[:2] = True                                       # ... one zero, one not: the totals balance
        y = np.round(y)                                         # many tied costs
        if not np.abs(y[oy]).sum():
            y[np.flatnonzero(oy)[0]] = 1.0
    return x, y, ox, oy


def _check(rect, x, y, ox, oy, what):
    want = ref.emd_linprog(*gref.zero_marginal_problem(x, y, ox, oy))
    xh, yh, p, q, _ = gref.reduced_problem(x, y, ox, oy)
    got, st, piv = rect(xh, yh, p, q)
    print(f"{what}: Tr={len(p)} Tc={len(q)} got={got!r} linprog={want!r} diff={abs(got - want):.2e} st={st} piv={piv}")
    return got, st, want


@pytest.mark.parametrize("T", [1, 2, 5, 12, 33, 64])
def test_masked_cases_vs_linprog(rect, T):
    """9 cases per length (54 in all), F = 1..4, gap shares 0..0.9 per node."""
    rs = np.random.RandomState(1000 + T)
    for k in range(9):
        x, y, ox, oy = _masked_case(rs, T, k)
        got, st, want = _check(rect, x, y, ox, oy, f"T={T} k={k}")
        assert st == 0, (T, k, st)
        assert abs(got - want) <= 1e-9, (T, k, got, want)


def test_gambia_length_pair_with_gaps(rect):
    """T = 287 with about 30 % gaps in both nodes: one pair against the 287 x 287 LP."""
    rs = np.random.RandomState(287)
    x, y = rs.randn(287, 4), rs.randn(287, 4)
    ox, oy = _mask(rs, 287, 0.3), _mask(rs, 287, 0.3)
    assert ox.sum() != oy.sum() and 150 < ox.sum() < 250
    got, st, want = _check(rect, x, y, ox, oy, "T=287")
    assert st == 0
    assert abs(got - want) <= 1e-9


def test_unbalanced_returns_reference_fallback(rect):
    """A node whose observed rows are all zero: totals cnt * 1e-12 / (cnt * 1e-12 + 1e-12) vs 1."""
    rs = np.random.RandomState(3)
    T = 12
    x, y = rs.randn(T, 3), rs.randn(T, 3)
    ox, oy = _mask(rs, T, 0.3), _mask(rs, T, 0.3)
    x[ox] = 0.0
    got, st, want = _check(rect, x, y, ox, oy, "unbalanced")
    assert (got, st) == (1.0, 1)
    assert want == 1.0                                           # HiGHS: infeasible


@pytest.mark.parametrize("nr,nc", [(1, 1), (1, 9), (9, 1), (1, 40), (40, 1), (5, 12), (12, 5), (33, 64), (64, 33)])
def test_single_row_column_and_rectangular(rect, nr, nc):
    """Tr = 1, Tc = 1 and Tr != Tc, each in both orders, on a T = 70 series."""
    rs = np.random.RandomState(100 * nr + nc)
    T = 70
    x, y = rs.randn(T, 4), rs.randn(T, 4)
    ox, oy = np.zeros(T, bool), np.zeros(T, bool)
    ox[rs.choice(T, nr, replace=False)] = True
    oy[rs.choice(T, nc, replace=False)] = True
    got, st, want = _check(rect, x, y, ox, oy, f"{nr}x{nc}")
    xh, yh, p, q, D = gref.reduced_problem(x, y, ox, oy)
    assert (len(p), len(q)) == (nr, nc)
    assert st == 0
    assert abs(got - want) <= 1e-9
    assert abs(got - gref.rect_linprog(p, q, D)) <= 1e-9
    if nr == 1 or nc == 1:                                       # one feasible plan: p q^T
        assert abs(got - float(p @ D @ q)) <= 1e-12


def test_square_call_equals_square_solver_bits(rect, square, golden_dir):
    """Tc == T through the rectangular entry = the square entry on the g7 golden pairs: the
    same value bits and the same pivot count (same arithmetic in the same order)."""
    g = np.load(os.path.join(golden_dir, "g7_stag_pairs.npz"), allow_pickle=False)
    n = 0
    for T in (12, 48):
        data, pairs, emd = g[f"data_T{T}"], g[f"pairs_T{T}"], g[f"emd_T{T}"]
        full = np.ones(T, bool)
        for (i, j), e in zip(pairs, emd):
            xh, yh, p, q, _ = gref.reduced_problem(data[:, i], data[:, j], full, full)
            a, b = rect(xh, yh, p, q), square(xh, yh, p, q)
            assert a[1] == b[1] and a[2] == b[2], (T, i, j, a, b)
            assert np.float64(a[0]).tobytes() == np.float64(b[0]).tobytes(), (T, i, j, a, b)
            assert abs(a[0] - e) <= 1e-9
            n += a[1] == 0 and a[2] > 0
    assert n > 0                                                 # some pair really pivoted
