"""Which kernel templates a block geometry runs: a plain-Python mirror of the dispatch
arithmetic in dstagnn_drought_amd/csrc (no torch, no device), so a CPU test can hold the
parity suite's case tables against the set of templates the gates admit
(tests/test_parity_coverage_cpu.py).

Every function cites the source it mirrors; a change to one of those lines must be made
here too, and the coverage test then says which admitted template lost its case.
"""

FLASH_SMALL_N = 512  # cheb_flash.hip kSmallN (flash_small(N): N <= kSmallN)
LDS_BYTES = 160 << 10  # the CU's LDS: cheb_agg.hip cheb_agg_ok / op_cheb_agg_sddmm


def nq_of(n):
    """cheb_agg.hip nq_of: float4 quads a lane holds for a row of n floats."""
    return 1 if n <= 64 else 2 if n <= 128 else 4 if n <= 256 else 6 if n <= 384 else 8 if n <= 512 else \
        12 if n <= 768 else 16


def km_of(K):
    """cheb_agg.hip km_of: the order template a Chebyshev order K runs in."""
    return 2 if K <= 2 else 3 if K <= 3 else 5 if K <= 5 else 8


def sddmm_lds_bytes(K, F, T):
    """cheb_agg.hip sddmm_lds_bytes: 4 waves x K x F x T floats."""
    return 4 * K * F * T * 4


def cheb_agg_ok(F, C, K, T):
    """cheb_agg.hip cheb_agg_ok."""
    return 1 <= F <= 32 and C in (16, 32) and 1 <= K <= 8 and T >= 1 and sddmm_lds_bytes(K, F, T) <= LDS_BYTES


def cheb_agg_kernels(T, K, F, C):
    """(family, (NQ, KM)) of the three aggregate-first launches: op_cheb_agg_fwd,
    op_cheb_agg_sddmm and op_cheb_agg_spmm_t (cheb_agg.hip), default DSTAGNN_* knobs.
    The *2 families are the sample-pair kernels (T <= 16)."""
    km, FT = km_of(K), F * T
    out = set()
    if T <= 16 and FT <= 512:                      # op_cheb_agg_fwd
        out.add(("fwd2", (nq_of(FT), km)))
    else:
        out.add(("fwd", (nq_of(F * min(32, T)), km)))
    if T <= 16 and FT <= 512 and 2 * sddmm_lds_bytes(K, F, T) <= LDS_BYTES:  # op_cheb_agg_sddmm
        out.add(("sddmm2", (nq_of(FT), km)))
    else:
        out.add(("sddmm", (nq_of(min(FT, 1024)), km)))
    if T <= 16 and T * C <= 512:                   # op_cheb_agg_spmm_t
        out.add(("spmm_t2", (nq_of(T * C), km)))
    else:
        out.add(("spmm_t", (nq_of(min(32, T) * C), km)))
    if K < km:  # the order loops' `k < a.K` guards inside a KM-wide template
        out.add(("k_lt_km", (km,)))
    return out


def flash_small_kernels(N):
    """(family, template args) of the small-graph flash launches: op_flash_forward and
    op_flash_dqk (cheb_flash.hip), default knobs."""
    nt = (N + 31) >> 5
    tpw = (nt + 3) // 4  # tiles per wave
    out = {("flash_small_fwd", (tpw,))}
    if nt <= 6:  # two strips per workgroup
        out.add(("flash_small_dqk2", ((nt + 1) // 2,)))
    else:
        out.add(("flash_small_dqk", (tpw, 4 if tpw <= 2 else 1)))
    return out


def flash_small_fwd_lds_bytes(N):
    """op_flash_forward's dynamic LDS (over 64 KB: the raised-limit branch of allow_lds)."""
    return ((N + 31) >> 5) * 32 * 33 * 4


def kernels(N, T, K, F, C, B, sparse=True, flash=True, d_k=32):
    """The set of (kernel family, template args) a block of this geometry runs.  sparse: the
    union support is <= 1/4 dense (block_fn.use_sparse); flash: not forced off
    (block_fn.use_flash: on the sparse path, d_k == 32, B <= 128).  Mirrors block.hip mkdims."""
    out = set()
    if not sparse:
        return out
    if cheb_agg_ok(F, C, K, T):
        out |= cheb_agg_kernels(T, K, F, C)
    if flash and d_k == 32 and B <= 128:
        out |= flash_small_kernels(N) if N <= FLASH_SMALL_N else {("flash_streamed", ())}
    return out
