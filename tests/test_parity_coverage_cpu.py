"""The parity suite's case tables (tests/test_gpu_parity.py) against the kernel templates the
library's gates admit (tests/kernel_coverage.py, a mirror of the dispatch arithmetic): every
template in REQUIRED must be run by at least one oracle-held case.  No device needed: a case
deleted from a table, or a gate widened past the cases, fails here and names the template.
"""
import kernel_coverage as kc
import test_gpu_parity as tp


def _block_cases():
    """(label, N, T, K, F, C, B, flash) of every case that goes through
    _run_config_vs_oracle at the fp32 bound (the bf16-operand variant's cases are not counted)."""
    rows = [(n, first, B, flash) for n, first, B, flash in tp.CONFIG_CASES + tp.TRAIN_CASES]
    rows += [(c[0], c[1], c[3], None) for c in tp.TAT_FUSED_CASES]
    rows += [(n, False, B, flash) for n, B, flash in tp.FLASH_LARGE_BATCH_CASES]
    rows += [(c[0], c[1], c[2], c[4]) for c in tp.PINNED_CASES]
    for name, first, B, flash in rows:
        N, T, K, h, D, dk, C = tp.CONFIGS[name]
        yield f"{name}/{'first' if first else 'inner'}/B{B}", N, T, K, (1 if first else C), C, B, flash is not False, dk


def _reached():
    got = {}
    for label, N, T, K, F, C, B, flash, dk in _block_cases():
        for t in kc.kernels(N, T, K, F, C, B, sparse=True, flash=flash, d_k=dk):
            got.setdefault(t, label)
    return got


_KMS = (2, 3, 5, 8)
REQUIRED = (
    [("flash_small_fwd", (t,)) for t in (1, 2, 3, 4)] + [("flash_small_dqk2", (t,)) for t in (1, 2, 3)] +
    [("flash_small_dqk", a) for a in ((2, 4), (3, 1), (4, 1))] + [("flash_streamed", ())] +
    # sample-pair kernels: every order template at NQ = 4, 6, 8; NQ = 1 (first block: rows of T
    # floats) at every order too.  NQ = 2 needs a row of 65..128 floats: F = 16 at T = 7, 8, or
    # T C = 128 in spmm_t2 — pinned at KM = 8, the template that spills.  spmm_t2's rows are
    # T C >= 7 * 16 floats, so it has no NQ = 1.
    [(f, (nq, km)) for f in ("fwd2", "sddmm2", "spmm_t2") for nq in (4, 6, 8) for km in _KMS] +
    [(f, (1, km)) for f in ("fwd2", "sddmm2") for km in _KMS] +
    [(f, (2, 8)) for f in ("fwd2", "sddmm2", "spmm_t2")] +
    # single-sample kernels (T > 16)
    [(f, a) for f in ("fwd", "sddmm", "spmm_t") for a in ((12, 2), (12, 3), (12, 5), (12, 8), (16, 2), (16, 3), (16, 5), (16, 8))] +
    # ... NQ = 1 (first block); spmm_t's rows are min(32, T) C >= 17 * 16 floats: no NQ = 1 there
    [(f, (1, km)) for f in ("fwd", "sddmm") for km in _KMS] +
    # an order below the template's (K = 1; 4; 6 or 7 — KM = 3 only ever runs K = 3)
    [("k_lt_km", (km,)) for km in (2, 5, 8)])


def test_every_required_template_has_a_case():
    got = _reached()
    missing = [f"{f}<{', '.join(map(str, a))}>" for f, a in REQUIRED if (f, a) not in got]
    assert not missing, "no parity case reaches: " + "; ".join(missing)


def test_pinned_geometries_run_the_templates_their_comments_name():
    k = lambda name, first: kc.kernels(*_geom(name, first))  # noqa: E731
    assert ("spmm_t2", (8, 8)) in k("k8t16", False) and ("sddmm2", (8, 8)) in k("k8t16", False)
    assert ("fwd", (16, 8)) in k("k8t40", False) and ("spmm_t", (16, 5)) in k("k4t48", False)
    assert ("fwd2", (2, 8)) in k("c16k8t8", False) and ("fwd2", (4, 3)) in k("c16t12", False)
    assert ("flash_small_fwd", (4,)) in k("n401", False) and ("flash_small_dqk", (4, 1)) in k("n512", True)
    assert ("flash_streamed", ()) in k("n520", False) and ("flash_small_dqk2", (3,)) in k("n150", False)
    # the forward's raised dynamic-LDS branch: N in (480, 512] only
    assert kc.flash_small_fwd_lds_bytes(512) == 67584 > (64 << 10) >= kc.flash_small_fwd_lds_bytes(480)
    assert kc.flash_small_fwd_lds_bytes(tp.CONFIGS["n401"][0]) <= (64 << 10)
    # the cases that must not take cheb_agg say so themselves
    for c in tp.PINNED_CASES:
        N, T, K, F, C, B = _geom(c[0], c[1])
        assert kc.cheb_agg_ok(F, C, K, T) == ("cheb_agg" in c[6]) == ("cheb_agg" not in c[7]), c[:3]


def _geom(name, first, B=2):
    N, T, K, h, D, dk, C = tp.CONFIGS[name]
    return N, T, K, (1 if first else C), C, B


def test_lds_gate_equality_and_one_past():
    assert kc.sddmm_lds_bytes(8, 32, 40) == 160 << 10
    assert kc.cheb_agg_ok(32, 32, 8, 40) and not kc.cheb_agg_ok(32, 32, 8, 41)
    assert kc.cheb_agg_ok(1, 32, 8, 41)  # the first block's F = 1 image fits
    assert not kc.cheb_agg_ok(32, 32, 3, 144)  # t144k3: Theta-first
    assert not kc.cheb_agg_ok(32, 32, 9, 12) and not kc.cheb_agg_ok(33, 32, 3, 12) and not kc.cheb_agg_ok(32, 24, 3, 12)
    # the tables hold both sides of the gate
    names = {c[0] for c in tp.PINNED_CASES if not c[1]}
    assert {"k8t40", "k8t41"} <= names


def test_dispatch_thresholds():
    assert [kc.nq_of(n) for n in (64, 65, 128, 129, 256, 257, 384, 385, 512, 513, 768, 769)] == \
        [1, 2, 2, 4, 4, 6, 6, 8, 8, 12, 12, 16]
    assert [kc.km_of(K) for K in range(1, 9)] == [2, 2, 3, 5, 5, 8, 8, 8]
    # T <= 16 takes the sample-pair kernels, T = 17 the single-sample ones
    assert {f for f, _ in kc.cheb_agg_kernels(16, 3, 32, 32)} == {"fwd2", "sddmm2", "spmm_t2"}
    assert {f for f, _ in kc.cheb_agg_kernels(17, 3, 32, 32)} == {"fwd", "sddmm", "spmm_t"}
    assert kc.flash_small_kernels(192) == {("flash_small_fwd", (2,)), ("flash_small_dqk2", (3,))}
    assert kc.flash_small_kernels(193) == {("flash_small_fwd", (2,)), ("flash_small_dqk", (2, 4))}
    assert kc.flash_small_kernels(385) == {("flash_small_fwd", (4,)), ("flash_small_dqk", (4, 1))}
    assert ("flash_streamed", ()) in kc.kernels(513, 12, 3, 32, 32, 2)
