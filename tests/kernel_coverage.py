"""Which kernel templates a block geometry runs: a plain-Python mirror of the dispatch
arithmetic in dstagnn_drought_amd/csrc (no torch, no device), so a CPU test can hold the
parity suite's case tables against the set of templates the gates admit
(tests/test_parity_coverage_cpu.py).

Every function cites the source it mirrors; a change to one of those lines must be made
here too, and the coverage test then says which admitted template lost its case.
"""

# The source text of the gates mirrored for the aggregate-first templates, the in-kernel dTheta and the
# multi-feature first block, as it stands in dstagnn_drought_amd/csrc (whitespace aside).
# tests/test_parity_coverage_cpu.py::test_mirrored_gates_read_as_recorded looks each one up, so a gate
# edited without this file fails there; change the function below and the line here together.
MIRRORED_SOURCE = {
    "cheb_agg.hip": [
        "constexpr bool dth_form_ok(int nq, int km) { return km <= 5 && nq >= 2 && nq <= 8 && !(nq == 2 && km != 3); }",
        "int nq_of(int n) { return n <= 64 ? 1 : n <= 128 ? 2 : n <= 256 ? 4 : n <= 384 ? 6 : n <= 512 ? 8 : n <= 768 ? 12 : 16; }",
        "int km_of(int K) { return K <= 2 ? 2 : K <= 3 ? 3 : K <= 5 ? 5 : 8; }",
        "unsigned grid_rows(int64_t waves) { return (unsigned)(cdiv64(cdiv64(waves, 4), 8) * 8); }",
        "size_t sddmm_lds_bytes(int K, int F, int T) { return (size_t)4 * K * F * T * sizeof(float); }",
        "return (int64_t)grid_rows((int64_t)((B + 1) / 2) * N) * K * F * C;",
        "if (!pair_env || B < 1 || N < 1 || !cheb_agg_ok(F, C, K, T) || T > 16) return false;",
        "if (!dth_form_ok(nq_of(T * C), km_of(K))) return false;",
        "return cheb_agg_dtheta_ws_floats(B, N, F, C, K) <= ws_floats;",
        "return F >= 1 && F <= 32 && (C == 16 || C == 32) && K >= 1 && K <= 8 && T >= 1 && "
        "sddmm_lds_bytes(K, F, T) <= (160u << 10);",
        "if (pair_env && a.T <= 16 && a.F * a.T <= 512) {",
        "const bool pair = pair_env && a.T <= 16 && FT <= 512 && 2 * sddmm_lds_bytes(a.K, a.F, a.T) <= (160u << 10);",
        "if (pair_env && a.T <= 16 && a.T * a.C <= 512) {",
        "if (save) dispatch<FwdL>(nq_of(a.F * std::min(32, a.T)), km_of(a.K), l);",
        "dispatch<SddmmL>(nq_of(std::min(FT, 1024)), km_of(a.K),",
        "dispatch<SpmmT2DL>(nq_of(a.T * a.C), km_of(a.K),",
        "dispatch<SpmmTL>(nq_of(std::min(32, a.T) * a.C), km_of(a.K),",
    ],
    "block.hip": [
        "constexpr size_t kGemmWs = size_t(8) << 20;",
        "m.first = first_flag(d) || m.F == 1;",
        "m.mf = m.first && m.F > 1;",
        "m.agg = agg_env && m.sparse && cheb_agg_ok(m.F, m.C, m.K, m.T);",
        "m.dth = m.agg && cheb_agg_dtheta_fused(m.B, m.N, m.F, m.C, m.K, m.T, (int64_t)kGemmWs);",
        "m.gfused = !m.mf && gtu_fused_fwd_ok(m.C, m.T);",
        "m.gbfused = !m.mf && gtu_fused_bwd_ok(m.C, m.T);",
        "a.R = (int)m.BFT; a.L = m.N; a.src[0].p = x; a.src[0].row = idx2(m.FT, 1, (int64_t)m.N * m.FT); a.src[0].es = m.FT;",
        "const int64_t pb = ln_bwd_part_blocks(m.BFT); const bool part = ln_bwd_partials_ok(m.N) && 2 * pb <= m.BFT;",
    ],
    "gtu_tail.hip": [
        "bool tail_mf(const GtuTailArgs& a) { return a.first && a.F > 1; }",
        "size_t fwd_lds_f1(const GtuTailArgs& a) { return sizeof(float) * (size_t)TailFwdLds(a.C, a.T, true).total; }",
        "size_t bwd_lds_f1(const GtuTailArgs& a) { return sizeof(float) * (size_t)TailBwdLds(a.C, a.T, true).total; }",
        "constexpr int kTailSplitT = 20;",
        "return on && a.C == 32 && a.T == 24 && !tail_mf(a);",
        "static bool tail_ct(const GtuTailArgs& a) { return !tail_mf(a) && (tail_ct24(a) || (a.C == 32 && a.T == 12)); }",
        "if (tail_ct24(a)) return false; return fwd_lds_f1(a) > 32 * 1024 || a.T >= kTailSplitT;",
        "if (tail_ct24(a)) return false; return bwd_lds_f1(a) > 32 * 1024 || a.T >= kTailSplitT;",
    ],
}

FLASH_SMALL_N = 512  # cheb_flash.hip kSmallN (flash_small(N): N <= kSmallN)
LDS_BYTES = 160 << 10  # the CU's LDS: cheb_agg.hip cheb_agg_ok / op_cheb_agg_sddmm


def cdiv(a, b):
    return -(-a // b)


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


GEMM_WS_FLOATS = 8 << 20  # block.hip:47 kGemmWs: the split-K slab the in-kernel dTheta's fold rows must fit


def grid_rows(waves):
    """cheb_agg.hip:906 grid_rows: workgroups of four waves, rounded up to a multiple of 8."""
    return cdiv(cdiv(waves, 4), 8) * 8


def dth_form_ok(nq, km):
    """cheb_agg.hip:705 dth_form_ok: the spmm_t2 forms that hold the K dTheta accumulators."""
    return km <= 5 and 2 <= nq <= 8 and not (nq == 2 and km != 3)


def cheb_agg_dtheta_ws_floats(B, N, F, C, K):
    """cheb_agg.hip:1040 cheb_agg_dtheta_ws_floats: one fold row of K F C floats per workgroup."""
    return grid_rows(((B + 1) // 2) * N) * K * F * C


def cheb_agg_dtheta_fused(B, N, F, C, K, T, ws_floats=GEMM_WS_FLOATS):
    """cheb_agg.hip:1048 cheb_agg_dtheta_fused, default DSTAGNN_AGG_PAIR; block.hip:89 (mkdims m.dth)
    asks it with ws_floats = kGemmWs."""
    if B < 1 or N < 1 or not cheb_agg_ok(F, C, K, T) or T > 16:
        return False
    if not dth_form_ok(nq_of(T * C), km_of(K)):
        return False
    return cheb_agg_dtheta_ws_floats(B, N, F, C, K) <= ws_floats


def cheb_agg_kernels(T, K, F, C, B=2, N=40):
    """(family, (NQ, KM)) of the three aggregate-first launches: op_cheb_agg_fwd:1065,
    op_cheb_agg_sddmm:1084 and op_cheb_agg_spmm_t:1106 (cheb_agg.hip), default DSTAGNN_* knobs.
    The *2 families are the sample-pair kernels (T <= 16); "spmm_t2_dth" is
    cheb_agg_spmm_t2_kernel<NQ, KM, DTH = true>, taken where cheb_agg_dtheta_fused(B, N, ...)
    holds (B, N enter only through the fold scratch: the suite's B = 2, N = 40 sit far inside it)."""
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
    if cheb_agg_dtheta_fused(B, N, F, C, K, T):    # op_cheb_agg_spmm_t: a.dth set by the block
        out.add(("spmm_t2_dth", (nq_of(T * C), km)))
    elif T <= 16 and T * C <= 512:
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


# ---------------------------------------------------------------------------------------
# LayerNorm (ops.hip op_ln_fwd / op_ln_bwd) and the block's three call sites (block.hip)
# ---------------------------------------------------------------------------------------
LN_MAX_L = 4096  # ops.hip op_ln_fwd / op_ln_bwd: "ln_fwd: row too long" above
LN_V4_L = (256, 512, 1024)  # ops.hip ln_fwd_v4_ok / ln_bwd_v4_ok


def ln_bwd_part_blocks(R):
    """ops.hpp ln_bwd_part_blocks (kLnRowsPerWave = 1: four rows a workgroup)."""
    return cdiv(R, 4)


def ln_bwd_partials_ok(L):
    """ops.hpp ln_bwd_partials_ok."""
    return L <= 1024


def _ln_shape(L, v4):
    """The template both directions pick for a row of L floats (ops.hip op_ln_fwd:1097-1123,
    op_ln_bwd:1133-1158): ("v4", L / 256), ("vpt", VPT), ("wg", 8 | 16) or None (refused)."""
    if v4 and L in LN_V4_L:
        return ("v4", L // 256)
    vpt = cdiv(L, 64)
    for v in (1, 2, 4, 8, 16):
        if vpt <= v:
            return ("vpt", v)
    if L <= LN_MAX_L:
        return ("wg", 8 if L <= 2048 else 16)  # fwd: cdiv(L, 256) <= 8; bwd: L <= 2048 — the same split
    return None


def ln_kernels(L, v4_fwd=True, v4_bwd=True, part=True):
    """(forward, backward) templates of one LayerNorm over rows of L floats, default DSTAGNN_LN_V4.

    v4_fwd / v4_bwd: the float4 kernels' preconditions other than L in {256, 512, 1024} hold
    (ln_fwd_v4_ok / ln_bwd_v4_ok: unit element strides, row maps whose strides are multiples of 4
    floats, 16-B aligned pointers).  In the block they hold by construction wherever L is one of the
    three lengths: every buffer is an Arena::take slot (256-B aligned) or a parameter tensor, a
    partial slab's second half starts pb * L floats in (L % 4 == 0), and the row maps are idx1(L)
    or idx2(FT, BN, N) with BN = B N a multiple of 4 when N is — except the first block's EmbedT
    FORWARD, whose source 0 reads x (B,N,1,T) with element stride es = T (>= 7), so that launch
    never takes v4 (its backward reads dE / writes du_et with unit stride and does).

    part: the backward writes per-workgroup partial slabs (gpart / bpart) rather than the (R, L)
    contribution tensors.  The slabs need ln_bwd_partials_ok(L); the v4 backward exists only in
    the slab form.  Backward third field: "part" | "contrib".  Refused: ("refused", ())."""
    f, b = _ln_shape(L, v4_fwd), None
    if part and not ln_bwd_partials_ok(L):
        raise ValueError("partial slabs need L <= 1024")  # op_ln_bwd:1131
    if part:
        b = _ln_shape(L, v4_bwd)  # L <= 1024: v4 or vpt, never wg
    else:
        b = _ln_shape(L, False)   # op_ln_bwd:1148-1158 has no float4 contribution kernel
    fwd = ("refused", ()) if f is None else f
    bwd = ("refused", ()) if b is None else b + ("part" if part else "contrib",)
    return fwd, bwd


def mf_class(shape):
    """The kernel family of an ln_kernels() shape, the granularity of the multi-feature tokens:
    ("vpt1",) one value a lane, ("vptN",) more than one, ("v4",) float4, ("wg",) a workgroup a row
    — then "part" | "contrib" where the shape carries it.  The per-length templates are pinned at
    F = 1 / F = C; what a multi-feature first block changes is the row count B F T and EmbedT's
    element stride F T, which each family walks in its own way."""
    kind = ("vpt1" if shape[1] == 1 else "vptN") if shape[0] == "vpt" else shape[0]
    return (kind,) + tuple(shape[2:])


def ln_sites(N, T, F, D, B, fused_fwd, fused_bwd, train=False, first=None):
    """The block's LayerNorm launches as (family, args) with family "ln_fwd/<site>" /
    "ln_bwd/<site>" (block.hip stage_tat:588-639, stage_sat:708-721, backward :1229-1245,
    embedT_backward:1336-1354, stage_tat:1359-1371):
      embedT  first block only, rows B F T of N floats (stage_tat:603-613, embedT_backward:1366-1380:
              a.R = m.BFT; F = 1 on the default first block); it runs whether or not the fused TAt
              kernels do.  Slabs iff ln_bwd_partials_ok(N) and 2 pb <= B F T.  Its forward reads x
              with element stride es = F T >= 7, so it never takes float4.
      tat     rows B F T of N floats, per direction only where the fused kernel is refused
              (tat_fused_*_ok).  Slabs iff tat_part(): ln_bwd_partials_ok(N) and 2 pb <= B F T.
      embedS  rows B N of D floats; slabs iff ln_bwd_partials_ok(D) (whatever the row count).
              train: dropout in the forward's epilogue / on the backward's dy, recorded as
              ("ln_drop", (kernel kind,)).  The pre_conv bias gradient rides on the slab launch
              (preconv_bias_part: ln_bwd_partials_ok(D) and 2 pb <= B N) or takes its own column sum.
    A forward over L > 4096 is refused before any backward is planned.
    first defaults to F == 1.  On a multi-feature first block (first and F > 1: block.hip:82 m.mf)
    the EmbedT and TAt launches are recorded under "ln_fwd_mf/<site>" / "ln_bwd_mf/<site>" with
    mf_class() args instead, so a case at F = 1 or F = C does not stand in for them."""
    out = set()
    first = (F == 1) if first is None else first
    mf = first and F > 1

    def add(site, L, R, v4_fwd, part, fwd=True, bwd=True, mark=False):
        f, b = ln_kernels(L, v4_fwd=v4_fwd, part=part)
        if fwd:
            out.add(("ln_fwd_mf/" + site, mf_class(f)) if mark and f[0] != "refused" else ("ln_fwd/" + site, f))
        if bwd and f[0] != "refused":
            out.add(("ln_bwd_mf/" + site, mf_class(b)) if mark else ("ln_bwd/" + site, b))
        return f

    R = B * F * T
    if first:
        add("embedT", N, R, False, ln_bwd_partials_ok(N) and 2 * ln_bwd_part_blocks(R) <= R, mark=mf)
    add("tat", N, R, True, ln_bwd_partials_ok(N) and 2 * ln_bwd_part_blocks(R) <= R,
        fwd=not fused_fwd, bwd=not fused_bwd, mark=mf)
    f = add("embedS", D, B * N, True, ln_bwd_partials_ok(D))
    if f[0] != "refused":
        if train:
            out.add(("ln_drop", (f[0],)))
        xpart = ln_bwd_partials_ok(D) and 2 * ln_bwd_part_blocks(B * N) <= B * N
        out.add(("preconv_bias", ("xpart" if xpart else "colsum",)))
    return out


# ---------------------------------------------------------------------------------------
# temporal attention (tat_fused.hip gates; tat.hip unfused paths)
# ---------------------------------------------------------------------------------------
TAT_LDS = 64 << 10  # tat.hip tat_path: a VALU problem's LDS bound
TAT_CW = 16         # tat.hip kTatCW


def tat_fused_fwd_ok(N, T, h, dk, dv):
    """tat_fused.hip tat_fused_fwd_ok (kTfH = 3, kTfD = 32, kTfNmax = 320), default knobs."""
    return h == 3 and dk == 32 and dv == 32 and 1 <= N <= 320 and T in (8, 12, 16)


def tat_fused_bwd_ok(N, T, h, dk, dv, F, res_kind):
    """tat_fused.hip tat_fused_bwd_ok: broadcast res_att (res_kind 1) needs whole 48-row
    workgroups per sample."""
    return tat_fused_fwd_ok(N, T, h, dk, dv) and (res_kind != 1 or (F * T) % 48 == 0)


def tat_mfma_ok(T, dk, dv):
    """tat.hip tat_mfma_ok (kTatD = 32), default knobs; its operands are Arena slots or whole
    tensors, so the 16-B alignment holds."""
    return dk == 32 and dv == 32 and T % 4 == 0 and 4 <= T <= 16


def tat_valu_fwd_floats(T, dk, dv):
    """tat.hip tat_valu_fwd_floats."""
    return 2 * T * (dk + 1) + T * (dv + 1) + T * T


def tat_valu_bwd_floats(T, dk, dv):
    """tat.hip tat_valu_bwd_floats."""
    return 2 * T * (dk + 1) + 2 * T * (dv + 1) + 2 * T * T


def tat_path(mfma, T, valu_floats):
    """tat.hip tat_path (kTatW = 4 problems per G = 64 workgroup)."""
    if mfma:
        return "mfma"
    if T <= 16 and 4 * valu_floats * 4 <= TAT_LDS:
        return "valu64"
    return "cols" if valu_floats * 4 > TAT_LDS else "valu256"


def tat_kernels(T, h, dk, dv, F, res_kind, fused_fwd=False, fused_bwd=False, multi=False):
    """The unfused temporal-attention launches (tat.hip op_tat_fwd / op_tat_bwd), per direction
    only where the fused kernel is refused.  ("tat_fwd" | "tat_bwd", args) with args ("mfma", T),
    ("valu64",), ("valu256",) or ("cols", "full" | "partial") — partial: T % 16 != 0, the last
    column chunk has cw < 16 (and the batched GEMM behind it an M = T off its tile).  With a
    broadcast res_att (res_kind 1) the backward's sum over f is ("tat_dres", ("fold",)) — in-kernel,
    the matrix-core path with F % 4 == 0 (op_tat_bwd:610) — or ("tat_dres", ("sum_middle", path));
    with a full one (res_kind 2) ("tat_dres", ("full", path)).  ("tat_res", (forward path, "none" |
    "bcast" | "full")) is the residual tile the forward adds to the scores; ("tat_edge", (direction,
    "last_valu256" | "first_cols")) marks a T on either side of that direction's hand-over from
    the G = 256 kernel (largest LDS image) to the column chunks.
    multi (a multi-feature first block, 1 < F <= 8 problems a sample and no res_att): only
    ("tat_fwd_mf" | "tat_bwd_mf", (path,)), so that a case at F = 1 or F = C does not stand in."""
    out = set()

    def args(path):
        return ("mfma", T) if path == "mfma" else ("cols", "partial" if T % TAT_CW else "full") \
            if path == "cols" else (path,)

    def edge(d, floats):  # T sits on the G = 256 | column-chunk hand-over of direction d
        at = lambda t: tat_path(tat_mfma_ok(t, dk, dv), t, floats(t, dk, dv))  # noqa: E731
        if at(T) == "valu256" and at(T + 1) == "cols":
            out.add(("tat_edge", (d, "last_valu256")))
        if at(T) == "cols" and at(T - 1) == "valu256":
            out.add(("tat_edge", (d, "first_cols")))

    mf = tat_mfma_ok(T, dk, dv)
    mode = ("none", "bcast", "full")[res_kind]
    if not fused_fwd:
        path = tat_path(mf, T, tat_valu_fwd_floats(T, dk, dv))
        out.add(("tat_fwd", args(path)))
        out.add(("tat_res", (path, mode)))  # tat_res_tile: no residual tile, one per (b, head), one per problem
        edge("fwd", tat_valu_fwd_floats)
    if not fused_bwd:
        path = tat_path(mf, T, tat_valu_bwd_floats(T, dk, dv))
        out.add(("tat_bwd", args(path)))
        edge("bwd", tat_valu_bwd_floats)
        if res_kind == 1:
            out.add(("tat_dres", ("fold",) if path == "mfma" and F % 4 == 0 else ("sum_middle", path)))
        elif res_kind == 2:  # block.hip stage_tat:1382: dS is written straight into d res_att
            out.add(("tat_dres", ("full", path)))
    if multi:  # the B F problems of a multi-feature first block (op_tat_fwd / op_tat_bwd take m.F: block.hip:631, :1415)
        return {(f + "_mf", a[:1]) for f, a in out if f in ("tat_fwd", "tat_bwd")}
    return out


# ---------------------------------------------------------------------------------------
# GTU stage (gtu_fused.hip gates; gtu_tail.hip; block.hip stage_tail)
# ---------------------------------------------------------------------------------------
TAIL_NT = 64          # gtu_tail.hip kNT
TAIL_SPLIT_T = 20     # gtu_tail.hip kTailSplitT
TAIL_SPLIT_LDS = 32 << 10  # gtu_tail.hip tail_split_fwd / tail_split_bwd


def tail_fwd_lds_bytes(C, T, stage_w=True, has_g=True, nt=TAIL_NT):
    """gtu_tail.hip TailFwdLds(...).total floats, as bytes (fwd_lds)."""
    S = 3 * T - 12
    SP, CP, P = S + 1, C + 1, (nt // T if T < nt else 1)
    total = (C * SP if has_g else 0) + C * T + T * CP + max(P * T, nt) + 2 * T + (T * SP if stage_w else 0)
    return 4 * total


def tail_bwd_lds_bytes(C, T, stage_w=True, has_g=True, nt=TAIL_NT):
    """gtu_tail.hip TailBwdLds(...).total floats, as bytes (bwd_lds)."""
    S = 3 * T - 12
    SP, CP, P = S + 1, C + 1, (nt // T if T < nt else 1)
    shared = max(C * SP if has_g else 0, T * CP, 2 * max(P * T, nt))
    return 4 * (3 * C * T + shared + 2 * T + (T * S if stage_w else 0))


def tail_ct24(C, T):
    """gtu_tail.hip tail_ct24, default DSTAGNN_TAIL_CT24."""
    return C == 32 and T == 24


def tail_split_fwd(C, T):
    """gtu_tail.hip tail_split_fwd."""
    return not tail_ct24(C, T) and (tail_fwd_lds_bytes(C, T) > TAIL_SPLIT_LDS or T >= TAIL_SPLIT_T)


def tail_split_bwd(C, T):
    """gtu_tail.hip tail_split_bwd."""
    return not tail_ct24(C, T) and (tail_bwd_lds_bytes(C, T) > TAIL_SPLIT_LDS or T >= TAIL_SPLIT_T)


def gtu_fused_ok(C, T):
    """gtu_fused.hip gtu_fused_fwd_ok / gtu_fused_bwd_ok (kGC = 32, kGT = 12), default knobs."""
    return C == 32 and T == 12


def gtu_kernels(C, T, first=False, F=1):
    """The GTU stage's launches (block.hip stage_tail forward :769-816, backward :960-1019).
    Fused (C = 32, T = 12): ("gtu_fused_fwd", ()), ("gtu_fused_bwd", ()).  Otherwise
    ("gtu_tail_fwd" | "gtu_tail_bwd", (kind, cc)) with kind "split" (gates | GEMM | tail), "ct24"
    (tail_ct: C = 32 at T = 24; its T = 12 twin runs only with the fused kernels switched off) or
    "generic" (gtu_tail_*_kernel<true>), the two directions decided independently, and cc the
    channel class "c32" | "c16" | "cx" (any other C: the runtime-C kernels off the two widths the
    Chebyshev stage's aggregate-first kernels admit), then "first" | "inner" (a.first: the
    residual_conv branch and its rpart / dpart sums); ("gtu_tail_pair", (fwd kind, bwd kind));
    and the input gradient ("gtu_dx", ("tconv",)) (gtu_tconv_ok: C = 32) or ("gtu_dx", ("kcat",)).
    F > 1 on a first block is the multi-feature first block (block.hip:82 m.mf, :96-97: never the
    fused GTU; gtu_tail.hip:992 tail_mf, :1049-1056: tail_ct24 and tail_ct are false under it): the
    MF = true forms of the runtime-generic kernels, third state "first_mf", the split decided by the
    F = 1 LDS layout whatever F (gtu_tail.hip:1000-1001 fwd_lds_f1 / bwd_lds_f1, :1057-1064), and
    the pairing as ("gtu_tail_pair", (fwd kind, bwd kind, "first_mf"))."""
    mf = first and F > 1
    if gtu_fused_ok(C, T) and not mf:
        return {("gtu_fused_fwd", ()), ("gtu_fused_bwd", ())}
    cc = "c32" if C == 32 else "c16" if C == 16 else "cx"
    if mf:
        lds_f, lds_b = tail_fwd_lds_bytes(C, T) > TAIL_SPLIT_LDS, tail_bwd_lds_bytes(C, T) > TAIL_SPLIT_LDS
        f = "split" if lds_f or T >= TAIL_SPLIT_T else "generic"
        b = "split" if lds_b or T >= TAIL_SPLIT_T else "generic"
        return {("gtu_tail_fwd", (f, cc, "first_mf")), ("gtu_tail_bwd", (b, cc, "first_mf")),
                ("gtu_tail_pair", (f, b, "first_mf")), ("gtu_dx", ("tconv" if C == 32 else "kcat",))}

    def kind(split):
        return "split" if split else "ct24" if tail_ct24(C, T) else "generic"
    f, b = kind(tail_split_fwd(C, T)), kind(tail_split_bwd(C, T))
    fi = "first" if first else "inner"
    return {("gtu_tail_fwd", (f, cc, fi)), ("gtu_tail_bwd", (b, cc, fi)), ("gtu_tail_pair", (f, b)),
            ("gtu_dx", ("tconv" if C == 32 else "kcat",))}


# ---------------------------------------------------------------------------------------
# Theta-first sparse Chebyshev (cheb_sparse.hip), where cheb_agg_ok refuses
# ---------------------------------------------------------------------------------------
CHEB_CHUNK = 1024  # cheb_sparse.hip kChunk = 64 * kMaxNQ


def theta_first_kernels(C, T):
    """cheb_sparse.hip DS_NQ_DISPATCH over rows of C T floats, the same template for
    cheb_spmm_fwd / cheb_sddmm_bwd / cheb_spmm_t_bwd: ("theta_first", (NQ,)), and
    ("theta_first_chunked", ()) when a row is walked in more than one 1024-float chunk."""
    nq = cdiv(min(C * T, CHEB_CHUNK), 64)
    nq = next(v for v in (1, 2, 3, 4, 6, 8, 12, 16) if nq <= v)
    out = {("theta_first", (nq,))}
    if C * T > CHEB_CHUNK:
        out.add(("theta_first_chunked", ()))
    return out


DISPATCH_FAMILIES = ("ln_", "preconv_bias", "tat_fwd", "tat_bwd", "tat_dres", "tat_res", "tat_edge", "tat_dkv", "gtu_tail", "gtu_dx", "theta_first")


def dispatch_only(ks):
    """The members of a kernels() set that belong to the LayerNorm, unfused temporal-attention,
    GTU-tail and Theta-first dispatchers, as "family<args>" strings."""
    return {f"{f}<{', '.join(map(str, a))}>" for f, a in ks if f.startswith(DISPATCH_FAMILIES)}


def kernels(N, T, K, F, C, B, sparse=True, flash=True, d_k=32, h=None, D=None, d_v=None, first=None,
            res_kind=None, train=False):
    """The set of (kernel family, template args) a block of this geometry runs.  sparse: the
    union support is <= 1/4 dense (block_fn.use_sparse); flash: not forced off
    (block_fn.use_flash: on the sparse path, d_k == 32, B <= 128).  Mirrors block.hip mkdims:73-99.
    first (default F == 1) and F are independent: an inner block has F = C, a first block F in 1..8
    (mkdims:81-82: m.first = the caller's flag or F == 1, m.mf = m.first && F > 1, the multi-feature
    first block).  With h and D given the LayerNorm, temporal-attention and GTU dispatchers are
    included too (d_v defaults to d_k, res_kind to 0 on a first block and 1 — broadcast res_att —
    on an inner one, the parity suite's default)."""
    out = set()
    first = (F == 1) if first is None else first
    assert first or F == C, "an inner block has F == C"
    assert not first or 1 <= F <= 8, "a first block takes 1..8 features (DSTAGNN_MAX_FIRST_F)"
    mf = first and F > 1
    if h is not None and D is not None:
        d_v = d_k if d_v is None else d_v
        res_kind = (0 if first else 1) if res_kind is None else res_kind
        ff = tat_fused_fwd_ok(N, T, h, d_k, d_v)
        fb = ff and tat_fused_bwd_ok(N, T, h, d_k, d_v, F, res_kind)
        if ff:
            out.add(("tat_fused_fwd_mf" if mf else "tat_fused_fwd", ()))
        if fb:
            out.add(("tat_fused_bwd_mf" if mf else "tat_fused_bwd", ()))
        out |= ln_sites(N, T, F, D, B, ff, fb, train=train, first=first)
        out |= tat_kernels(T, h, d_k, d_v, F, res_kind, ff, fb, multi=mf)
        if d_k != d_v and not mf:  # the same kernels with two different widths in the [Q | K | V] row: (path,)
            out |= {(f + "_dkv", a[:1]) for f, a in out if f in ("tat_fwd", "tat_bwd")}
            out.add(("tat_dkv_order", ("dk>dv" if d_k > d_v else "dk<dv",)))  # which of the row's blocks is the wider
        gk = gtu_kernels(C, T, first, F)
        out |= gk
        if train and not (gtu_fused_ok(C, T) and not mf):  # the fcmy dropout rides in the tail kernels, both directions
            out |= {("gtu_tail_drop", a) for f, a in gk if f == "gtu_tail_pair"}
    if not sparse:
        return out
    if cheb_agg_ok(F, C, K, T):
        out |= cheb_agg_kernels(T, K, F, C, B, N)
    else:
        out |= theta_first_kernels(C, T)
    if flash and d_k == 32 and B <= 128:
        out |= flash_small_kernels(N) if N <= FLASH_SMALL_N else {("flash_streamed", ())}
    return out
