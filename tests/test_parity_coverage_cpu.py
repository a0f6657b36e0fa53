"""The parity suite's case tables (tests/test_gpu_parity.py, and the oracle-held rows of
tests/test_gpu_cheb_dtheta.py and tests/test_gpu_multifeature.py) against the kernel templates the
library's gates admit (tests/kernel_coverage.py, a mirror of the dispatch arithmetic): every
template in REQUIRED must be run by at least one oracle-held case.  No device needed: a case
deleted from a table, or a gate widened past the cases, fails here and names the template.
REQUIRED itself is held to what the mirror admits over the gates' domain (the test_*_required_is_what_
the_gates_admit tests), so it cannot fall behind a gate either.
"""
import kernel_coverage as kc
import test_gpu_cheb_dtheta as tdt  # (adds its geometries to test_gpu_parity.CONFIGS at import)
import test_gpu_multifeature as tmf
import test_gpu_parity as tp


def _block_cases():
    """(label, N, T, K, F, C, B, flash, d_k, h, D, d_v, res_kind, train, first, sparse) of every case
    that goes through _run_config_vs_oracle at the fp32 bound (the bf16-operand variant's cases are
    not counted) — the tables of test_gpu_parity and test_gpu_cheb_dtheta — or through
    test_gpu_multifeature._run_block_case (multi-feature first blocks: first with F > 1).
    res_kind None: the suite's default, 0 on the first block and 1 on an inner one."""
    rows = [(n, first, B, flash, None, False) for n, first, B, flash in tp.CONFIG_CASES]
    rows += [(n, first, B, flash, None, True) for n, first, B, flash in tp.TRAIN_CASES]
    rows += [(c[0], c[1], c[3], None, c[2], c[4]) for c in tp.TAT_FUSED_CASES]
    rows += [(n, False, B, flash, None, False) for n, B, flash in tp.FLASH_LARGE_BATCH_CASES]
    rows += [(c[0], c[1], c[2], c[4], None, c[3]) for c in tp.PINNED_CASES]
    rows += [(c[0], c[1], c[2], None, c[4], c[3]) for c in _dispatch_cases()]
    rows += [(n, first, B, None, None, train) for n, first, B, train, _ in _dtheta_cases()]
    for name, first, B, flash, res_kind, train in rows:
        N, T, K, h, D, dk, C, dv = tp.config(name)
        yield (f"{name}/{'first' if first else 'inner'}/B{B}", N, T, K, (1 if first else C), C, B, flash is not False,
               dk, h, D, dv, res_kind, train, first, True)
    for shape, F, train, sparse in _multifeature_cases():
        N, T, K, h, D, dk, C, B = tmf.SHAPES[shape]
        yield (f"mf/{shape}/F{F}", N, T, K, F, C, B, True, dk, h, D, dk, 0, train, True, sparse)


def _dispatch_cases():
    return tp.DISPATCH_CASES


def _dtheta_cases():
    """test_gpu_cheb_dtheta's oracle-held rows: test_block_vs_oracle and test_scratch_bound_sides_vs_oracle."""
    return tdt.BASE_CASES + tdt.SHAPE_CASES + [tdt.REFUSED] + list(tdt.WS_CASES)


def _multifeature_cases():
    """(shape, F, train, sparse) of test_gpu_multifeature's _run_block_case rows: test_block_vs_fp64_helper,
    its dense and train-mode variants (shape A at F = 4) and test_block_dispatch_rows_vs_fp64_helper."""
    return [(s_, F, False, True) for s_, F in tmf.BLOCK_CASES] + [("A", 4, False, False), ("A", 4, True, True)] + \
        [(s_, F, train, True) for s_, F, train in tmf.MF_DISPATCH_CASES]


def _reached():
    got = {}
    for label, N, T, K, F, C, B, flash, dk, h, D, dv, res_kind, train, first, sparse in _block_cases():
        for t in kc.kernels(N, T, K, F, C, B, sparse=sparse, flash=flash, d_k=dk, h=h, D=D, d_v=dv, res_kind=res_kind,
                            train=train, first=first):
            got.setdefault(t, label)
    return got


_KMS = (2, 3, 5, 8)
# The aggregate-first instantiations some admitted geometry reaches (test_cheb_agg_required_is_what_the_gates_admit
# enumerates the mirror over the gates' domain and holds this list to the result): products, but
#   spmm_t     rows of min(32, T) C >= 17 * 16 = 272 floats: no NQ < 6;
#   spmm_t2    rows of T C >= 7 * 16 = 112 floats: no NQ = 1; the form that also produces dTheta where
#              dth_form_ok(NQ, KM), the plain one elsewhere (while the fold scratch admits B N);
#   *2         the sample-pair kernels stop at NQ = 8 (F T, T C <= 512).
_NQS, _NQS2 = (1, 2, 4, 6, 8, 12, 16), (1, 2, 4, 6, 8)
REQUIRED_CHEB_AGG = (
    [(f, (nq, km)) for f in ("fwd", "sddmm") for nq in _NQS for km in _KMS] +
    [(f, (nq, km)) for f in ("fwd2", "sddmm2") for nq in _NQS2 for km in _KMS] +
    [("spmm_t", (nq, km)) for nq in _NQS if nq >= 6 for km in _KMS] +
    [("spmm_t2_dth" if kc.dth_form_ok(nq, km) else "spmm_t2", (nq, km)) for nq in _NQS2 if nq >= 2 for km in _KMS])
# Past the fold-scratch bound (cheb_agg_dtheta_ws_floats > kGemmWs) the ten dth_form_ok forms run plain
# instead.  Five have a case on that side: pems07 at B = 66, and test_gpu_cheb_dtheta.WS_CASES at B = 327 / 545.
REQUIRED_PAST_WS = [("spmm_t2", a) for a in ((6, 3), (4, 5), (8, 5), (6, 5), (4, 3))]
# ... and five have none: the smallest batch that passes the bound at N = 40 is 820 samples at K = 2, 545 at
# K = 3 and T = 13 (twice the 20 M decisions of the costliest row here), or, for <2, 3> (C = 16), 2185 — each
# through the fp64 oracle on the host four times over, 4 to 12 s a row (scaled from the rows at B = 327 / 545,
# which take 2.6 to 8 s) and about 35 s together.  The plain form is the DTH one without its accumulators and epilogue (the same walk
# and dx arithmetic: cheb_agg.hip cheb_agg_spmm_t2_kernel, `if constexpr (DTH)`), and the hand-over itself
# is held on both sides at <4, 5>.  test_cheb_agg_required_is_what_the_gates_admit holds this list exact.
PAST_WS_UNPINNED = [("spmm_t2", a) for a in ((2, 3), (4, 2), (6, 2), (8, 2), (8, 3))]

REQUIRED = (
    [("flash_small_fwd", (t,)) for t in (1, 2, 3, 4)] + [("flash_small_dqk2", (t,)) for t in (1, 2, 3)] +
    [("flash_small_dqk", a) for a in ((2, 4), (3, 1), (4, 1))] + [("flash_streamed", ())] +
    REQUIRED_CHEB_AGG + REQUIRED_PAST_WS +
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
# What only a multi-feature first block (first, 1 < F <= 8) runs (test_multifeature_required_is_what_the_gates_admit):
# the MF = true tail forms, and the EmbedT / TAt LayerNorm and temporal-attention launches over B F T rows
# / B F problems by kernel family (kernel_coverage.mf_class).
_MF_PAIRS = [("generic", "generic", "first_mf"), ("split", "split", "first_mf"), ("generic", "split", "first_mf")]
REQUIRED_MF = (
    [(d, (k, cc, "first_mf")) for d in ("gtu_tail_fwd", "gtu_tail_bwd") for k in ("generic", "split")
     for cc in ("c16", "c32", "cx")] +
    [(f, p) for f in ("gtu_tail_pair", "gtu_tail_drop") for p in _MF_PAIRS] +
    [("ln_fwd_mf/embedT", (k,)) for k in ("vpt1", "vptN", "wg")] +  # (es = F T: never float4)
    [("ln_fwd_mf/tat", (k,)) for k in ("vpt1", "vptN", "v4", "wg")] +
    [("ln_bwd_mf/" + s, a) for s in ("embedT", "tat")
     for a in (("vpt1", "part"), ("vptN", "part"), ("v4", "part"), ("wg", "contrib"))] +
    [(d, (p,)) for d in ("tat_fwd_mf", "tat_bwd_mf") for p in ("mfma", "valu64", "valu256", "cols")] +
    [("tat_fused_fwd_mf", ()), ("tat_fused_bwd_mf", ())])
REQUIRED = REQUIRED + REQUIRED_DISPATCH + REQUIRED_MF

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


_FAR = (1 << 12, 1 << 12)  # a (B, N) whose fold rows pass kGemmWs at every (F, C, K): 2^21 rows of >= 16 floats


def _admitted_cheb_agg(B, N):
    """Every aggregate-first token the mirror gives over cheb_agg_ok's domain at this (B, N): C in {16, 32},
    T in 7..199 (check_dims: T >= 7), K in 1..8, an inner block (F = C) or a first block with F in 1..8."""
    S = set()
    for C in (16, 32):
        for T in range(7, 200):
            for K in range(1, 9):
                for F in (C,) + tuple(range(1, 9)):
                    if kc.cheb_agg_ok(F, C, K, T):
                        S |= {t for t in kc.cheb_agg_kernels(T, K, F, C, B, N) if t[0] != "k_lt_km"}
    return S


def test_cheb_agg_required_is_what_the_gates_admit():
    near, far = _admitted_cheb_agg(2, 40), _admitted_cheb_agg(*_FAR)
    req = set(REQUIRED_CHEB_AGG)
    assert len(REQUIRED_CHEB_AGG) == len(req) == 128
    assert near == req, (sorted(near - req, key=str), sorted(req - near, key=str))
    # past the scratch bound: no DTH form, each as the plain one; nothing else moves
    dth = {t for t in req if t[0] == "spmm_t2_dth"}
    assert len(dth) == 10 and far == (req - dth) | {("spmm_t2", a) for _, a in dth}
    assert {("spmm_t2", a) for _, a in dth} == set(REQUIRED_PAST_WS) | set(PAST_WS_UNPINNED)
    assert not set(REQUIRED_PAST_WS) & set(PAST_WS_UNPINNED)
    # what the F = 1 | C geometries alone admit (the domain the hand-written list was made for) lacks exactly
    # the forms only a multi-feature first block reaches
    S1 = set()
    for C in (16, 32):
        for T in range(7, 200):
            for K in range(1, 9):
                for F in (1, C):
                    if kc.cheb_agg_ok(F, C, K, T):
                        S1 |= {t for t in kc.cheb_agg_kernels(T, K, F, C) if t[0] != "k_lt_km"}
    # (the SDDMM walks whole F T rows, so a long first block gives it NQ = 2 and 4; the forward's 32-step chunks do not)
    assert req - S1 == {("fwd", (nq, km)) for nq in (2, 4) for km in _KMS}, sorted(req - S1, key=str)


def test_no_admitted_cheb_agg_instantiation_lacks_a_case():
    got = _reached()
    adm = _admitted_cheb_agg(2, 40) | _admitted_cheb_agg(*_FAR)
    unreached = sorted((t for t in adm if t not in got), key=str)
    assert unreached == sorted(PAST_WS_UNPINNED, key=str), unreached


def test_dtheta_scratch_bound():
    """dth_form_ok, the fold-scratch arithmetic and the two batch sizes test_gpu_cheb_dtheta.WS_CASES runs."""
    assert kc.GEMM_WS_FLOATS == 8388608
    assert [kc.grid_rows(w) for w in (1, 32, 33, 6520, 6560)] == [8, 8, 16, 1632, 1640]
    assert kc.cheb_agg_dtheta_ws_floats(325, 40, 32, 32, 5) == 1632 * 5120 == 8355840 <= kc.GEMM_WS_FLOATS
    assert kc.cheb_agg_dtheta_ws_floats(327, 40, 32, 32, 5) == 1640 * 5120 == 8396800 > kc.GEMM_WS_FLOATS
    assert kc.cheb_agg_dtheta_ws_floats(326, 40, 32, 32, 5) == 8355840  # the lone sample of an odd batch has its pair's rows
    for (name, first, B, _, _), within in tdt.WS_CASES.items():
        N, T, K, h, D, dk, C, dv = tp.config(name)
        assert kc.cheb_agg_dtheta_fused(B, N, C, C, K, T) == within
        fam = "spmm_t2_dth" if within else "spmm_t2"
        assert (fam, (kc.nq_of(T * C), kc.km_of(K))) in kc.cheb_agg_kernels(T, K, C, C, B, N)
    sides = {(kc.nq_of(tp.config(n)[1] * 32), kc.km_of(tp.config(n)[2]), w) for (n, _, _, _, _), w in tdt.WS_CASES.items()}
    assert sides == {(4, 5, True), (4, 5, False), (8, 5, False), (6, 5, False), (4, 3, False)}, \
        f"WS_CASES lost a side of the scratch bound: has (NQ, KM, within) {sorted(sides)}"
    assert kc.cheb_agg_dtheta_ws_floats(545, 40, 32, 32, 3) == 2736 * 3072 == 8404992 > kc.GEMM_WS_FLOATS
    assert kc.cheb_agg_dtheta_fused(544, 40, 32, 32, 3, 7) and not kc.cheb_agg_dtheta_fused(545, 40, 32, 32, 3, 7)
    # pems07 at B = 66 (FLASH_LARGE_BATCH_CASES) is the other far-side row
    assert not kc.cheb_agg_dtheta_fused(66, 883, 32, 32, 3, 12) and kc.cheb_agg_dtheta_fused(32, 170, 32, 32, 3, 12)
    # the forms: K <= 5, 2 <= NQ <= 8, and at NQ = 2 only KM = 3
    assert [(nq, km) for nq in _NQS for km in _KMS if kc.dth_form_ok(nq, km)] == \
        [(2, 3)] + [(nq, km) for nq in (4, 6, 8) for km in (2, 3, 5)]
    assert not kc.cheb_agg_dtheta_fused(2, 40, 32, 32, 3, 17)  # the single-sample kernels never
    assert ("spmm_t2_dth", (2, 3)) in kc.cheb_agg_kernels(8, 3, 16, 16) and ("spmm_t2", (2, 2)) in kc.cheb_agg_kernels(8, 2, 16, 16)
    assert ("spmm_t2_dth", (4, 3)) in kc.cheb_agg_kernels(12, 3, 1, 16)  # a first block: T C decides, not F T


def _admitted_multifeature():
    """Every token only a multi-feature first block gives, over F in 2..8 and the domains of _admitted_dispatch."""
    S = set()
    Ls = [1, 64, 65, 128, 129, 200, 256, 257, 500, 512, 513, 1000, 1024, 1025, 2048, 2049, 4096]
    for N in Ls:
        for F in range(2, 9):
            for B in (1, 2):
                for fused in ((False, False), (True, False), (True, True)):
                    S |= {t for t in kc.ln_sites(N, 7, F, 64, B, *fused, first=True) if "_mf/" in t[0]}
    for T in range(7, 200):
        for F in range(2, 9):
            for dk, dv, h, N in ((32, 32, 2, 40), (32, 32, 3, 40), (32, 16, 2, 40), (12, 20, 2, 40)):
                S |= {t for t in kc.kernels(N, T, 2, F, 32, 2, d_k=dk, h=h, D=64, d_v=dv, first=True)
                      if t[0].startswith("tat_") and t[0].endswith("_mf")}
    for C in range(1, 129):
        for T in range(7, 200):
            for F in (2, 8):
                S |= {t for t in kc.kernels(40, T, 3, F, C, 2, h=2, D=64, first=True, train=True) if t[0].startswith("gtu_tail")}
    return S


def test_multifeature_required_is_what_the_gates_admit():
    S = _admitted_multifeature()
    assert S == set(REQUIRED_MF), (sorted(S - set(REQUIRED_MF), key=str), sorted(set(REQUIRED_MF) - S, key=str))
    # tail_mf routing (gtu_tail.hip:1049-1064; block.hip:96-97): never the fused GTU nor a compile-time tail —
    # C = 32 at T = 12 takes the generic MF form, at T = 24 the split one — and the F = 1 LDS layout decides
    g = lambda C, T, F: kc.gtu_kernels(C, T, True, F)  # noqa: E731
    assert ("gtu_tail_pair", ("generic", "generic", "first_mf")) in g(32, 12, 4)
    assert ("gtu_tail_pair", ("split", "split", "first_mf")) in g(32, 24, 4)
    assert g(32, 12, 1) == kc.gtu_kernels(32, 12, True) == {("gtu_fused_fwd", ()), ("gtu_fused_bwd", ())}
    assert ("gtu_tail_fwd", ("ct24", "c32", "first")) in g(32, 24, 1)
    assert all(g(C, T, 2) == g(C, T, 8) for C in (8, 16, 32, 72) for T in (7, 12, 19, 20, 24))
    assert ("gtu_tail_pair", ("generic", "split", "first_mf")) in g(72, 19, 4)
    assert not any(t[1][0] in ("ct24",) for t in S if t[0].startswith("gtu_tail"))
    # a multi-feature block's tokens never stand in for an F = 1 | C block's, nor the reverse
    mf, f1 = kc.kernels(40, 12, 3, 4, 32, 2, h=2, D=64, first=True), kc.kernels(40, 12, 3, 1, 32, 2, h=2, D=64)
    fams = lambda ks: {f for f, _ in ks if f.startswith(("ln_fwd", "ln_bwd", "tat_", "gtu_tail", "gtu_fused"))  # noqa: E731
                       and "embedS" not in f}
    assert not fams(mf) & fams(f1) - {"gtu_tail_fwd", "gtu_tail_bwd", "gtu_tail_pair"}, fams(mf) & fams(f1)
    assert not {t for t in mf if t[0].startswith("gtu_tail")} & {t for t in f1 if t[0].startswith("gtu_tail")}
    # EmbedT over B F T rows (block.hip:606-607): the slab condition reads B F T, and es = F T keeps float4 out
    assert ("ln_fwd_mf/embedT", ("vptN",)) in kc.ln_sites(256, 12, 4, 64, 2, False, False, first=True)
    assert ("ln_bwd_mf/embedT", ("v4", "part")) in kc.ln_sites(256, 12, 4, 64, 2, False, False, first=True)


def test_no_admitted_multifeature_token_lacks_a_case():
    got = _reached()
    unreached = sorted((t for t in _admitted_multifeature() if t not in got), key=str)
    assert not unreached, unreached


def test_mirrored_gates_read_as_recorded():
    """cheb_agg_ok, dth_form_ok, the dTheta scratch bound, the (NQ, KM) dispatch arguments and the tail_mf
    routing in csrc read as kernel_coverage.MIRRORED_SOURCE records them (comments and whitespace aside):
    a gate changed without the mirror fails here, on a machine without a device."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dstagnn_drought_amd", "csrc")
    for fname, lines in kc.MIRRORED_SOURCE.items():
        with open(os.path.join(csrc, fname)) as f:
            text = re.sub(r"//[^\n]*", "", f.read())
        text = " ".join(text.split())
        for ln in lines:
            assert " ".join(ln.split()) in text, f"{fname} no longer reads `{ln}`: bring tests/kernel_coverage.py in line with it"


def test_rows_no_token_tells_apart_are_in_the_tables():
    """Rows whose templates another row also reaches, kept for what the mirror has no token for."""
    pinned = {(c[0], c[1]) for c in tp.PINNED_CASES}
    assert ("c16t25", True) in pinned, "the first block at C = 16, T = 25"
    mf = set(tmf.MF_DISPATCH_CASES)
    assert ("c16t17k3", 8, False) in mf, "cheb_agg_fwd_kernel<4, 3> / sddmm<4, 3> at 136-float rows (c16t24 reaches them at 192)"
    assert {("c72t19", 4, False), ("c72t19", 4, True)} <= mf, "generic MF forward feeding a split MF backward, eval and train"
    assert ("t7f3", 3, False) in mf and (3 * tmf.SHAPES["t7f3"][1]) % 4 == 1, "F T = 21: rows no multiple of 4 floats"
    # every MF_DISPATCH row runs, and its geometry is what its comment says
    assert {s_ for s_, _, t_ in tmf.MF_DISPATCH_CASES if not t_} == set(tmf.MF_DISPATCH)
    k = lambda n: tmf.predicted(n, tmf.MF_DISPATCH[n][1])  # noqa: E731
    for K, km in ((2, 2), (3, 3), (5, 5), (8, 8)):
        assert {("fwd", (4, km)), ("sddmm", (4, km)), ("gtu_tail_fwd", ("generic", "c16", "first_mf"))} <= k(f"c16t17k{K}")
    assert {("fwd", (2, 5)), ("sddmm", (2, 5)), ("k_lt_km", (5,))} <= k("t24k4") and ("fwd", (2, 8)) in k("t24k6")
    assert ("theta_first", (3,)) in k("c8t20") and ("gtu_dx", ("kcat",)) in k("c8t20")
    assert {("tat_fwd_mf", ("valu64",)), ("fwd2", (1, 3))} <= k("t7f3")
    assert {("tat_fwd_mf", ("mfma",)), ("ln_fwd_mf/embedT", ("vptN",)), ("ln_fwd/embedT", ("vpt", 2))} & k("n100") == \
        {("tat_fwd_mf", ("mfma",)), ("ln_fwd_mf/embedT", ("vptN",))}
    # the forward-only table holds the new inner geometries too
    import test_gpu_forward_only as fo
    assert {"c16k2t25", "c16t25", "c16k5t25", "c16k8t25", "c16k2t17", "c16k5t17", "c16k8t17", "c16k2t8", "c16t8",
            "c16k5t8"} <= {c[0] for c in fo.CASES if not c[1]}


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
    assert {f for f, _ in kc.cheb_agg_kernels(16, 3, 32, 32)} == {"fwd2", "sddmm2", "spmm_t2_dth"}
    assert {f for f, _ in kc.cheb_agg_kernels(16, 8, 32, 32)} == {"fwd2", "sddmm2", "spmm_t2"}
    assert {f for f, _ in kc.cheb_agg_kernels(17, 3, 32, 32)} == {"fwd", "sddmm", "spmm_t"}
    assert kc.flash_small_kernels(192) == {("flash_small_fwd", (2,)), ("flash_small_dqk2", (3,))}
    assert kc.flash_small_kernels(193) == {("flash_small_fwd", (2,)), ("flash_small_dqk", (2, 4))}
    assert kc.flash_small_kernels(385) == {("flash_small_fwd", (4,)), ("flash_small_dqk", (4, 1))}
    assert ("flash_streamed", ()) in kc.kernels(513, 12, 3, 32, 32, 2)
