"""The parity suite's case tables (tests/test_gpu_parity.py) against the kernel templates the
library's gates admit (tests/kernel_coverage.py, a mirror of the dispatch arithmetic): every
template in REQUIRED must be run by at least one oracle-held case.  No device needed: a case
deleted from a table, or a gate widened past the cases, fails here and names the template.
"""
import kernel_coverage as kc
import test_gpu_parity as tp


def _block_cases():
    """(label, N, T, K, F, C, B, flash, d_k, h, D, d_v, res_kind, train) of every case that goes
    through _run_config_vs_oracle at the fp32 bound (the bf16-operand variant's cases are not
    counted).  res_kind None: the suite's default, 0 on the first block and 1 on an inner one."""
    rows = [(n, first, B, flash, None, False) for n, first, B, flash in tp.CONFIG_CASES]
    rows += [(n, first, B, flash, None, True) for n, first, B, flash in tp.TRAIN_CASES]
    rows += [(c[0], c[1], c[3], None, c[2], c[4]) for c in tp.TAT_FUSED_CASES]
    rows += [(n, False, B, flash, None, False) for n, B, flash in tp.FLASH_LARGE_BATCH_CASES]
    rows += [(c[0], c[1], c[2], c[4], None, c[3]) for c in tp.PINNED_CASES]
    rows += [(c[0], c[1], c[2], None, c[4], c[3]) for c in _dispatch_cases()]
    for name, first, B, flash, res_kind, train in rows:
        N, T, K, h, D, dk, C, dv = tp.config(name)
        yield (f"{name}/{'first' if first else 'inner'}/B{B}", N, T, K, (1 if first else C), C, B, flash is not False,
               dk, h, D, dv, res_kind, train)


def _dispatch_cases():
    return tp.DISPATCH_CASES


def _reached():
    got = {}
    for label, N, T, K, F, C, B, flash, dk, h, D, dv, res_kind, train in _block_cases():
        for t in kc.kernels(N, T, K, F, C, B, sparse=True, flash=flash, d_k=dk, h=h, D=D, d_v=dv, res_kind=res_kind,
                            train=train):
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


_LN_SHAPES = [("v4", v) for v in (1, 2, 4)] + [("vpt", v) for v in (1, 2, 4, 8, 16)] + [("wg", v) for v in (8, 16)]
_TAT_PATHS = [("mfma", T) for T in (8, 12, 16)] + [("valu64",), ("valu256",), ("cols", "full"), ("cols", "partial")]
# The LayerNorm, unfused temporal-attention, GTU-tail and Theta-first branches that some admitted
# geometry reaches (test_dispatch_required_is_what_the_gates_admit enumerates the mirrors over the
# gates' domain and holds this list to the result).
REQUIRED_DISPATCH = (
    # forward: every row shape at every site, but float4 at EmbedT (UNREACHABLE below)
    [("ln_fwd/" + s, a) for s in ("tat", "embedS") for a in _LN_SHAPES] +
    [("ln_fwd/embedT", a) for a in _LN_SHAPES if a[0] != "v4"] +
    # backward: partial slabs up to 1024 floats, the contribution form in the workgroup-per-row kernels
    [("ln_bwd/" + s, a + ("contrib" if a[0] == "wg" else "part",)) for s in ("embedT", "tat", "embedS")
     for a in _LN_SHAPES] +
    [("ln_drop", (k,)) for k in ("v4", "vpt", "wg")] + [("preconv_bias", (k,)) for k in ("xpart", "colsum")] +
    [(d, a) for d in ("tat_fwd", "tat_bwd") for a in _TAT_PATHS] +
    [(d + "_dkv", (p,)) for d in ("tat_fwd", "tat_bwd") for p in ("valu64", "valu256", "cols")] +
    [("tat_dkv_order", (o,)) for o in ("dk>dv", "dk<dv")] +
    # the residual tile the forward adds (none: first block) and where the backward puts d res_att
    [("tat_res", (p, m)) for p in ("mfma", "valu64", "valu256", "cols") for m in ("none", "bcast", "full")] +
    [("tat_edge", (d, e)) for d in ("fwd", "bwd") for e in ("last_valu256", "first_cols")] +
    [("tat_dres", ("fold",))] + [("tat_dres", (k, p)) for k in ("sum_middle", "full") for p in ("mfma", "valu64", "valu256", "cols")] +
    [(d, (k, cc, fi)) for d in ("gtu_tail_fwd", "gtu_tail_bwd") for k in ("generic", "split") for cc in ("c16", "c32", "cx")
     for fi in ("first", "inner")] +
    [(d, ("ct24", "c32", fi)) for d in ("gtu_tail_fwd", "gtu_tail_bwd") for fi in ("first", "inner")] +
    [(f, p) for f in ("gtu_tail_pair", "gtu_tail_drop")
     for p in (("generic", "generic"), ("split", "split"), ("ct24", "ct24"), ("generic", "split"))] +
    [("gtu_dx", ("tconv",)), ("gtu_dx", ("kcat",))] +
    [("theta_first", (nq,)) for nq in (1, 2, 3, 4, 6, 8, 12, 16)] + [("theta_first_chunked", ())])
REQUIRED = REQUIRED + REQUIRED_DISPATCH

# Instantiations in csrc that no admitted geometry reaches under default knobs, each with the reason
# the mirror gives (kept in the library: the knob suite or a C-ABI caller may still select them).
UNREACHABLE = {
    "ln_bwd_kernel<VPT, false> (VPT <= 16)":
        "L <= 1024 always takes the partial slabs: EmbedS asks only ln_bwd_partials_ok(D), and 2 pb <= R "
        "holds for every R >= 2 while the TAt / EmbedT rows number B F T, B T >= 7",
    "ln_fwd_v4_kernel at EmbedT":
        "its source 0 reads x (B,N,1,T) with element stride T >= 7, and ln_fwd_v4_ok needs unit strides",
    "ln_*_kernel<4 | 8 | 16> at L = 256 | 512 | 1024 in the block":
        "every operand is an arena slot or a parameter and the row strides are multiples of 4 floats, so "
        "the float4 kernels take these lengths (DSTAGNN_LN_V4=0 selects the scalar ones)",
    "gtu_tail_*_ct_kernel<32, 12, ...>":
        "C = 32, T = 12 is exactly gtu_fused_*_ok, so the fused GTU kernels run (DSTAGNN_GTU_FUSED=0 selects these)",
    "gtu_tail_pair (split, generic)":
        "T >= 20 splits both directions; for T < 20 the backward's LDS total passes 32 KB at a smaller C than the "
        "forward's, so the backward splits wherever the forward does",
}


def test_every_required_template_has_a_case():
    got = _reached()
    missing = [f"{f}<{', '.join(map(str, a))}>" for f, a in REQUIRED if (f, a) not in got]
    assert not missing, "no parity case reaches: " + "; ".join(missing)


def _admitted_dispatch():
    """Every LayerNorm / unfused-TAt / GTU-tail / Theta-first token the mirrors give over the
    gates' domain (check_dims: positive sizes, T >= 7; F in {1, C}), row lengths on both sides of
    every threshold."""
    S = set()
    Ls = [1, 64, 65, 128, 129, 200, 256, 257, 500, 512, 513, 1000, 1024, 1025, 2048, 2049, 4096]
    for N in Ls:
        for D in Ls:
            for F in (1, 32):
                for B in (1, 2):
                    for fused in ((False, False), (True, False), (True, True)):
                        for train in (False, True):
                            S |= kc.ln_sites(N, 7, F, D, B, *fused, train=train)
    for T in range(7, 200):
        for dk, dv in ((32, 32), (32, 16), (16, 32), (12, 20)):
            for F in (1, 6, 32):
                for rk in (0, 1, 2):
                    S |= {t for t in kc.kernels(40, T, 2, F, 32 if F == 1 else F, 2, d_k=dk, h=2, D=64, d_v=dv, res_kind=rk)
                          if t[0].startswith("tat_") and "fused" not in t[0]}
    for C in range(1, 129):
        for T in range(7, 200):
            for first in (False, True):
                S |= {t for t in kc.kernels(40, T, 3, 1 if first else C, C, 2, h=2, D=64, train=True) if t[0].startswith("gtu_tail")
                      or t[0] == "gtu_dx"}
            if not all(kc.cheb_agg_ok(F, C, K, T) for F in (1, C) for K in range(1, 9)):
                S |= kc.theta_first_kernels(C, T)
    return S


def test_dispatch_required_is_what_the_gates_admit():
    S = _admitted_dispatch()
    assert S == set(REQUIRED_DISPATCH), (sorted(S - set(REQUIRED_DISPATCH), key=str),
                                         sorted(set(REQUIRED_DISPATCH) - S, key=str))
    # the unreachable ones, from the same mirrors
    assert not any(f.startswith("ln_bwd/") and a[-1] == "contrib" and a[0] != "wg" for f, a in S)
    assert not any(f == "ln_fwd/embedT" and a[0] == "v4" for f, a in S)
    assert ("gtu_tail_pair", ("split", "generic")) not in S
    # (T >= 20 splits both directions whatever C; below that the backward's 3 C T floats pass 32 KB first)
    assert not any(kc.tail_split_fwd(C, T) and not kc.tail_split_bwd(C, T) for C in range(1, 4097) for T in range(7, 20))
    assert kc.gtu_kernels(32, 12) == {("gtu_fused_fwd", ()), ("gtu_fused_bwd", ())}
    assert all(2 * kc.ln_bwd_part_blocks(R) <= R for R in range(2, 4096))
    # a row past 4096 floats is refused at every site (test_layernorm_row_too_long_is_refused holds the message)
    assert kc.ln_kernels(4097, part=False) == (("refused", ()), ("refused", ()))
    assert ("ln_fwd/embedS", ("refused", ())) in kc.ln_sites(40, 12, 32, 4097, 1, True, True)


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
    N, T, K, h, D, dk, C, dv = tp.config(name)
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


def test_ln_tat_gtu_dispatch_thresholds():
    # unfused TAt: the G = 256 VALU kernels' LDS image against 64 KB, per direction
    fw, bw = kc.tat_valu_fwd_floats, kc.tat_valu_bwd_floats
    assert [4 * bw(T, 32, 32) for T in (63, 64)] == [65016, 66560] and [4 * fw(T, 32, 32) for T in (87, 88)] == [64728, 65824]
    tk = lambda T, dv=32, F=32, rk=1: kc.tat_kernels(T, 2, 32, dv, F, rk)  # noqa: E731
    assert ("tat_bwd", ("valu256",)) in tk(63) and ("tat_bwd", ("cols", "full")) in tk(64)
    assert {("tat_fwd", ("valu256",)), ("tat_bwd", ("cols", "partial"))} <= tk(87)
    assert {("tat_fwd", ("cols", "partial")), ("tat_bwd", ("cols", "partial"))} <= tk(88)
    # d_v = 16 moves both: backward 68 | 69, forward 93 | 94
    assert [4 * bw(T, 32, 16) for T in (68, 69)] == [64192, 65688] and [4 * fw(T, 32, 16) for T in (93, 94)] == [65472, 66552]
    assert ("tat_bwd", ("valu256",)) in tk(68, 16) and ("tat_bwd", ("cols", "partial")) in tk(69, 16)
    assert ("tat_fwd", ("valu256",)) in tk(93, 16) and ("tat_fwd", ("cols", "partial")) in tk(94, 16)
    assert {("tat_fwd", ("cols", "partial")), ("tat_bwd", ("cols", "partial"))} <= tk(100, 16)  # dv16t100
    # G = 64 up to T = 16, the matrix cores only at d_k = d_v = 32 and T % 4 == 0
    assert ("tat_fwd", ("valu64",)) in tk(16, 16) and ("tat_fwd", ("valu256",)) in tk(17, 16)
    assert ("tat_fwd", ("mfma", 16)) in tk(16) and ("tat_fwd", ("valu64",)) in tk(15) and ("tat_fwd", ("valu256",)) in tk(20)
    assert ("tat_dres", ("fold",)) in tk(12) and ("tat_dres", ("sum_middle", "mfma")) in tk(12, F=6)
    assert ("tat_dres", ("full", "mfma")) in tk(12, rk=2) and not any(f == "tat_dres" for f, _ in tk(12, rk=0))
    # the fused gates (predicted the same way by test_gpu_parity._pin / _disp)
    assert kc.tat_fused_fwd_ok(320, 12, 3, 32, 32) and not kc.tat_fused_fwd_ok(321, 12, 3, 32, 32)
    assert not kc.tat_fused_fwd_ok(40, 12, 3, 32, 16) and not kc.tat_fused_fwd_ok(40, 12, 2, 32, 32)
    assert kc.tat_fused_bwd_ok(40, 12, 3, 32, 32, 32, 1) and not kc.tat_fused_bwd_ok(40, 8, 3, 32, 32, 32, 1)
    # LayerNorm rows
    sh = lambda L: kc.ln_kernels(L, part=kc.ln_bwd_partials_ok(L))  # noqa: E731
    assert [sh(L)[0] for L in (64, 65, 128, 129, 255, 256, 257, 512, 513)] == \
        [("vpt", 1), ("vpt", 2), ("vpt", 2), ("vpt", 4), ("vpt", 4), ("v4", 1), ("vpt", 8), ("v4", 2), ("vpt", 16)]
    assert sh(1024) == (("v4", 4), ("v4", 4, "part")) and sh(1025) == (("wg", 8), ("wg", 8, "contrib"))
    assert sh(2048)[0] == ("wg", 8) and sh(2049) == (("wg", 16), ("wg", 16, "contrib"))
    assert sh(4096)[0] == ("wg", 16) and sh(4097) == (("refused", ()), ("refused", ()))
    assert kc.ln_kernels(1024, v4_fwd=False)[0] == ("vpt", 16)  # EmbedT's forward at N = 1024
    # the pre_conv bias rides on the EmbedS slab launch up to D = 1024
    assert ("preconv_bias", ("xpart",)) in kc.ln_sites(40, 12, 32, 1024, 2, True, True)
    assert ("preconv_bias", ("colsum",)) in kc.ln_sites(40, 12, 32, 1025, 2, True, True)
    # GTU tail: the two gates read different LDS totals against the same 32 KB and disagree at (72, 19)
    assert (kc.tail_fwd_lds_bytes(72, 19), kc.tail_bwd_lds_bytes(72, 19)) == (28172, 33236)
    assert not kc.tail_split_fwd(72, 19) and kc.tail_split_bwd(72, 19)
    assert ("gtu_tail_pair", ("generic", "split")) in kc.gtu_kernels(72, 19)
    assert kc.tail_split_fwd(32, 20) and not kc.tail_split_fwd(32, 19) and not kc.tail_split_fwd(32, 24)  # ct24
    assert kc.gtu_kernels(16, 24) >= {("gtu_tail_fwd", ("split", "c16", "inner")), ("gtu_dx", ("kcat",))}
    # Theta-first row templates
    assert [next(a[0] for f, a in kc.theta_first_kernels(1, n) if f == "theta_first") for n in
            (64, 65, 128, 129, 192, 193, 256, 257, 384, 385, 512, 513, 768, 769, 1024, 1025)] == \
        [1, 2, 2, 3, 3, 4, 4, 6, 6, 8, 8, 12, 12, 16, 16, 16]
    assert ("theta_first_chunked", ()) not in kc.theta_first_kernels(32, 32) and \
        ("theta_first_chunked", ()) in kc.theta_first_kernels(1, 1025)
    # the new tables hold both sides of each hand-over
    names = {c[0] for c in tp.DISPATCH_CASES}
    assert {"t63", "t64k2", "t87", "t88", "d1024", "d1040", "n1024h2", "n1030h2", "c72t19"} <= names


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
