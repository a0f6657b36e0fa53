"""GPU: every GEMM kernel template (gemm.hip / gemm_kern.hpp) pinned by an exact case.

Oracle.  A, B, C0 and the bias hold integers in [-4, 4] stored as fp32, alpha and beta come from
{1, 0.5, 2, -1}.  Every product and every partial sum is then an integer (or a half-integer
after alpha / beta) far below 2^24 — asserted per case as 16 K + |beta| 4 + 4 < 2^23 — so the
fp32 result is the same under ANY summation order (split-K slabs, ACC2, the skinny kernel's LDS
and ticket folds) and also with bf16 operands ([-4, 4] is exact in bf16).  The expected result
is the float64 product on the CPU cast to fp32, and the assertion is torch.equal: no tolerance.

Every case embeds its operands in larger buffers at non-zero element offsets:
  * the margins of A and B (every element outside the maps' image) are NaN: a read outside the
    image that reaches a stored output shows as NaN;
  * the C buffer is pre-filled with a sentinel bit pattern that every element outside the image
    of (c_z, c_m, c_n) must still hold after the call;
  * with beta == 0 the image of C is pre-filled with NaN, which the epilogue must not read.

Tables.  case_for(key) builds the case of a template key (tests/gemm_coverage.py mirrors the
dispatch and says which key a case runs; tests/test_gemm_coverage_cpu.py holds the two
together without a device):
  TILED_KEYS   the full cross product (var, cfg, ktwo, akc, bnc, va, vb) for var f32 / bf
               (3 x 2^3 x 2^2 = 96 each) and a2 (cfg 0 and 2: 64), less UNREACHABLE
  SKINNY_CASES every (MT, NT, A4) of skinny_dw_kernel, both fold depths, tail waves
  SPLITK_CASES plain split-K (short last slab, re-derived splitk, red_g > 1, K = 4095)
  EDGE_CASES   index-map edges (no key of their own)
and two tests run a child process with DSTAGNN_GEMM_LOG=1: the library's own "[gemm]" log line
of every case against the mirror, and the keys a PEMS08 block logs against the table's.

Not reached by direct cases, because the public descriptor (dstagnn_gemm_desc) does not expose
them: the column-sum column (ones=1), masks and output maps of the epilogue, grouped launches
and K-concatenated launches.  Those stay with the whole-block parity tests.
"""
import os
import subprocess
import sys
import zlib

import pytest
import torch

import gemm_coverage as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SENT_BITS = 0x5EADBEEF  # the C buffer's fill: a finite fp32 pattern no integer-valued result takes
ALPHAS = (1.0, 0.5, 2.0, -1.0)
BETAS = (0.0, 1.0, 0.5, 2.0, -1.0)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _up4(x):
    return (x + 3) // 4 * 4


# ---------------------------------------------------------------------------------------
# case descriptors (plain Python: the CPU coverage test imports them without a device)
# ---------------------------------------------------------------------------------------
def _case(cid, M, N, K, am, ak, bk, bn, a_off, b_off, batch=1, az=(0, 0, 0), bz=(0, 0, 0), cm=None, cn=(0, 1, 0),
          cz=None, c_off=5, epi=0, bias_stride=1, twice=False):
    """epi picks alpha, beta, bias and ReLU (every table walks all combinations)."""
    ldc = N + 3
    cm = (0, ldc, 0) if cm is None else cm
    cz = (0, M * ldc + 7, 0) if cz is None else cz
    return dict(id=cid, M=M, N=N, K=K, batch=batch, maps=[am, ak, az, bk, bn, bz, cm, cn, cz],
                offs=(a_off, b_off, c_off), alpha=ALPHAS[epi % 4], beta=BETAS[epi % 5], bias=epi % 2 == 1,
                bias_stride=bias_stride, relu=epi % 3 == 0, twice=twice)


def _a_layout(M, K, akc, two_level, wide):
    """(a_m, a_k, a_off, floats of one A window).  akc: rows of K (k-contiguous); else k-rows of
    M (m-contiguous), two_level: twelve k-rows a period with a NaN row between periods.  wide:
    leading dimension and offset multiples of 4 (16-B DMA, given M % 4 == 0 where the quads
    run along m); else an odd leading dimension and an odd offset."""
    if akc:
        ld = _up4(K) + (4 if wide else 5)
        return (0, ld, 0), (0, 1, 0), (8 if wide else 7), M * ld
    ld = _up4(M) + (4 if wide else 3)
    if two_level:
        return (0, 1, 0), (12, ld, 13 * ld), (8 if wide else 7), 13 * ld * gc.cdiv(K, 12)
    return (0, 1, 0), (0, ld, 0), (8 if wide else 7), K * ld


def _b_layout(N, K, bnc, two_level, wide):
    """(b_k, b_n, b_off, floats of one B window).  bnc: k-rows of N (n-contiguous), two_level:
    seven k-rows a period, a NaN row between; else columns of K (k-contiguous), two_level
    (width 1 only): seven k then two NaN floats."""
    if bnc:
        ld = _up4(N) + (4 if wide else 3)
        if two_level:
            return (7, ld, 8 * ld), (0, 1, 0), (12 if wide else 9), 8 * ld * gc.cdiv(K, 7)
        return (0, ld, 0), (0, 1, 0), (12 if wide else 9), K * ld
    if two_level:
        assert not wide
        ld = 9 * gc.cdiv(K, 7) + 2
        return (7, 1, 9), (0, ld, 0), 9, N * ld
    ld = _up4(K) + (4 if wide else 5)
    return (0, 1, 0), (0, ld, 0), (12 if wide else 9), N * ld


def _tiled_case(key):
    """The case of a tiled template key, or the reason (a string) the public descriptor cannot
    reach it."""
    var, cfg, ktwo, akc, bnc, va, vb = key
    two_a = ktwo and not akc
    two_b = ktwo and (bnc or vb == 1)
    if ktwo and not (two_a or two_b):
        return ("A k-contiguous (akc) leaves ktwo to B's k map, and B k-major (not bnc) at 16-B DMA width "
                "needs a single-level unit-stride k map (dma_width, kmaj)")
    wide_rows_a, wide_rows_b = (not akc and va == 4), (bnc and vb == 4)
    batch, az, bz, zper = 1, (0, 0, 0), (0, 0, 0), 0
    if var == "a2":      # split-K slabs longer than kAcc2MinK, batch > 1 keeps the skinny gate shut
        M, N = ((40 if wide_rows_a else 41), (40 if wide_rows_b else 39)) if cfg == 0 else \
               ((8 if wide_rows_a else 9), (8 if wide_rows_b else 7))
        K, batch, zper = 8200, 64, 8
    elif cfg == 1:       # 128x128: >= 4096 64x64 tiles and K >= 1024
        M, N, K, batch, zper = (68 if wide_rows_a else 65), (68 if wide_rows_b else 65), 1051, 1024, 8
    elif cfg == 0:
        M, N, K = (100 if wide_rows_a else 101), (68 if wide_rows_b else 70), 77
    else:
        M, N, K = (148 if wide_rows_a else 150), (28 if wide_rows_b else 25), 77
    am, ak, a_off, _ = _a_layout(M, K, akc, two_a, va == 4)
    bk, bn, b_off, bwin = _b_layout(N, K, bnc, two_b, vb == 4)
    if zper:  # A broadcast over the batch, B in zper windows walked by a two-level z map with s1 = 0
        bz = (zper, _up4(bwin) + (4 if vb == 4 else 5), 0)
    cid = "%s-c%d-k%d-a%d-b%d-v%d%d" % (var, cfg, ktwo, akc, bnc, va, vb)
    epi = zlib.crc32(cid.encode()) % 60
    return _case(cid, M, N, K, am, ak, bk, bn, a_off, b_off, batch=batch, az=az, bz=bz, epi=epi)


def _skinny_cases():
    out = []
    i = 0
    for M in (5, 20, 40, 60, 90):
        for N in (7, 25):
            # A4: an aligned unit-stride k map, K % 4 == 0 (K = 4100: the last workgroup's wave 0
            # holds one k quad, its waves 1..15 start past K)
            am, ak, a_off, _ = _a_layout(M, 4100, True, False, True)
            bk, bn, b_off, _ = _b_layout(N, 4100, True, False, i % 2 == 0)
            out.append(_case("sk-m%d-n%d-a4" % (M, N), M, N, 4100, am, ak, bk, bn, a_off, b_off, epi=i, twice=True))
            # not A4: an m-contiguous A, or (every other shape) the aligned k-contiguous A with
            # K % 4 != 0 (K = 4097: one k in the last workgroup's wave 0, a partial quad)
            if i % 2 == 0:
                am, ak, a_off, _ = _a_layout(M, 4100, False, False, True)
                K = 4100
            else:
                am, ak, a_off, _ = _a_layout(M, 4097, True, False, True)
                K = 4097
            bk, bn, b_off, _ = _b_layout(N, K, i % 4 < 2, False, False)
            out.append(_case("sk-m%d-n%d-a1" % (M, N), M, N, K, am, ak, bk, bn, a_off, b_off, epi=i + 7, twice=True))
            i += 1
    # the two-level fold: the dTheta shape (A = agg[j,k,f,t] read with a two-level k map, A4) ...
    T, KFT = 12, 96 * 12
    bk, bn, b_off, _ = _b_layout(32, 65280, True, False, True)
    out.append(_case("sk-fold2-dtheta", 96, 32, 65280, (0, T, 0), (T, 1, KFT), bk, bn, 4, b_off, epi=2, twice=True))
    # ... and a shape that is not A4 (m-contiguous A; 65 workgroups: four full groups and one of 1)
    am, ak, a_off, _ = _a_layout(96, 4100, False, False, False)
    bk, bn, b_off, _ = _b_layout(32, 4100, False, False, False)
    out.append(_case("sk-fold2-a1", 96, 32, 4100, am, ak, bk, bn, a_off, b_off, epi=4, twice=True))
    return out


def _splitk_cases():
    def mk(cid, M, N, K, epi, akc=True, bnc=True):
        am, ak, a_off, _ = _a_layout(M, K, akc, False, True)
        bk, bn, b_off, _ = _b_layout(N, K, bnc, False, False)
        return _case(cid, M, N, K, am, ak, bk, bn, a_off, b_off, epi=epi)
    return [mk("splitk-c0-short-last", 70, 50, 1000, 1),          # 7 slabs of 160, the last 40
            mk("splitk-c0-rederived", 70, 50, 1100, 2, akc=False),  # K / 128 = 8 slabs asked, 7 of 160 taken
            mk("splitk-c0-redg2", 70, 50, 2100, 3, bnc=False),     # 14 slabs: red_g = 2
            mk("splitk-c2-rederived", 150, 25, 1100, 4),
            mk("splitk-c2-k4095", 20, 25, 4095, 5)]                # one below the skinny gate: tiled, 26 slabs


def _edge_cases():
    out = []
    M, N, K = 37, 41, 50
    lda, ldb = K + 3, N + 2
    plain_a = ((0, lda, 0), (0, 1, 0))
    plain_b = ((0, ldb, 0), (0, 1, 0))
    # negative k strides (the flipped-kernel gradient: abias / bbias rebasing)
    out.append(_case("edge-neg-k", M, N, K, (0, lda, 0), (0, -1, 0), (0, -ldb, 0), (0, 1, 0), 4 + K - 1,
                     3 + (K - 1) * ldb, epi=1))
    # a two-level map with div = 1: off(i) = i * s1, s0 never used
    out.append(_case("edge-div1", M, N, K, (1, 999, lda), (0, 1, 0), (1, 0, ldb), (0, 1, 0), 4, 3, epi=2))
    # a two-level map with div > count: off(i) = i * s0, s1 never used
    out.append(_case("edge-div-gt-count", M, N, K, (200, lda, 7777), (60, 1, 5555), (64, ldb, 3333), (0, 1, 0), 4, 3,
                     epi=3))
    # a two-level c_m scatter (rows (i, t) -> C[i][n][t]) with ReLU + beta + bias, bias_stride 3
    Tn, Nn, KC, Kk = 12, 10, 9, 5
    c = _case("edge-cm-scatter", Nn * Tn, KC, Kk, (0, Kk + 2, 0), (0, 1, 0), (0, KC + 1, 0), (0, 1, 0), 3, 2,
              cm=(Tn, 1, KC * Tn), cn=(0, Tn, 0), bias_stride=3, epi=3)
    c.update(alpha=0.5, beta=2.0, bias=True, relu=True)
    out.append(c)
    # two-level a_z / b_z / c_z, batch 6 (periods 4, 3, 2)
    wa, wb, wc = M * lda, K * ldb, M * (N + 3)
    out.append(_case("edge-z-two-level", M, N, K, *plain_a, *plain_b, 4, 3, batch=6, az=(4, wa, 4 * wa + 11),
                     bz=(3, wb + 1, 3 * wb + 8), cz=(2, wc + 1, 2 * wc + 5), epi=7))
    out.append(_case("edge-m1n1k1", 1, 1, 1, (0, 1, 0), (0, 1, 0), (0, 1, 0), (0, 1, 0), 3, 2, epi=13))
    # K = 0: alpha * 0 + beta * C + bias
    c = _case("edge-k0", M, N, 0, *plain_a, *plain_b, 4, 3, epi=7)
    c.update(alpha=2.0, beta=0.5, bias=True, relu=False)
    out.append(c)
    return out


TILED_KEYS = [(var, cfg, bool(kt), bool(a), bool(b), va, vb)
              for var, cfgs in (("f32", (0, 1, 2)), ("bf", (0, 1, 2)), ("a2", (0, 2)))
              for cfg in cfgs for kt in (0, 1) for a in (0, 1) for b in (0, 1) for va in (1, 4) for vb in (1, 4)]
SKINNY_KEYS = [("skinny", mt, nt, gc.SK_U[mt], a4) for mt in (1, 2, 3, 4, 6) for nt in (1, 2) for a4 in (False, True)]
_TILED = {k: _tiled_case(k) for k in TILED_KEYS}
UNREACHABLE = {k: v for k, v in _TILED.items() if isinstance(v, str)}  # key -> reason
REACHABLE_TILED = [k for k in TILED_KEYS if k not in UNREACHABLE]
SKINNY_CASES = _skinny_cases()
SPLITK_CASES = _splitk_cases()
EDGE_CASES = _edge_cases()


def case_for(key):
    """The exact case that pins template `key` (a tiled key's own case; a skinny key's first
    case in SKINNY_CASES).  KeyError for a key in UNREACHABLE."""
    if key[0] == "skinny":
        for c in SKINNY_CASES:
            if gc.plan_case(c)["key"] == tuple(key):
                return c
        raise KeyError(key)
    c = _TILED[tuple(key)]
    if isinstance(c, str):
        raise KeyError(f"{key}: {c}")
    return c


def all_runs():
    """(case, bf16) of every direct case, in the order the log child runs them."""
    runs = [(_TILED[k], k[0] == "bf") for k in REACHABLE_TILED]
    runs += [(c, False) for c in SKINNY_CASES + SPLITK_CASES + EDGE_CASES]
    return runs


def _key_id(k):
    return _TILED[k]["id"] if k[0] != "skinny" else "skinny-mt%d-nt%d-u%d-a4%d" % k[1:]


# ---------------------------------------------------------------------------------------
# running a case
# ---------------------------------------------------------------------------------------
def _sizes(c):
    """Floats of the A, B, C and bias buffers (6 margin floats behind the last image element;
    the offsets keep at least one in front of the first)."""
    M, N, K, Z = c["M"], c["N"], c["K"], c["batch"]
    am, ak, az, bk, bn, bz, cm, cn, cz = c["maps"]
    lens = []
    for o, parts in zip(c["offs"], (((am, M), (ak, K), (az, Z)), ((bk, K), (bn, N), (bz, Z)), ((cm, M), (cn, N), (cz, Z)))):
        assert o + sum(gc.idx_min(m, n) for m, n in parts) >= 1, (c["id"], "no margin in front")
        lens.append(o + sum(gc.idx_max(m, n) for m, n in parts) + 7)
    return lens + [(N - 1) * c["bias_stride"] + 1]


def _offs(m, n):
    i = torch.arange(n, dtype=torch.int64)
    d, s0, s1 = m
    return (i % d) * s0 + torch.div(i, d, rounding_mode="floor") * s1 if d > 0 else i * s0


def _launch(c, A, B, C, bias):
    from dstagnn_drought_amd import _lib
    _lib.load().gemm_f32(A, B, C, [c["M"], c["N"], c["K"], c["batch"]], _lib.gemm_maps(*c["maps"]), list(c["offs"]),
                         c["alpha"], c["beta"], bias, c["bias_stride"], bool(c["relu"]))


def launch_only(c):
    """The case's launch on zero operands of the right sizes (the log child: no oracle)."""
    la, lb, lc, lbias = _sizes(c)
    z = lambda n: torch.zeros(n, device="cuda")  # noqa: E731
    _launch(c, z(la), z(lb), z(lc), z(lbias) if c["bias"] else None)


def _ints(gen, *shape):
    return torch.randint(-4, 5, shape, generator=gen).float()


def build(c):
    """Operand buffers and the expected C buffer of a case (CPU tensors)."""
    M, N, K, Z = c["M"], c["N"], c["K"], c["batch"]
    am, ak, az, bk, bn, bz, cm, cn, cz = c["maps"]
    a_off, b_off, c_off = c["offs"]
    alpha, beta = c["alpha"], c["beta"]
    assert alpha in ALPHAS and beta in BETAS
    # every product, partial sum and epilogue term an exactly representable fp32 (see the module docstring)
    assert 16 * K + abs(beta) * 4 + 4 < 2 ** 23, c["id"]
    la, lb, lc, lbias = _sizes(c)
    gen = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    # the distinct (A window, B window) pairs of the batch (broadcast operands: few products)
    zab = torch.stack([_offs(az, Z), _offs(bz, Z)], 1)
    uniq, inv = torch.unique(zab, dim=0, return_inverse=True)
    ai = a_off + uniq[:, 0, None, None] + _offs(am, M)[None, :, None] + _offs(ak, K)[None, None, :]
    bi = b_off + uniq[:, 1, None, None] + _offs(bk, K)[None, :, None] + _offs(bn, N)[None, None, :]
    ci = c_off + _offs(cz, Z)[:, None, None] + _offs(cm, M)[None, :, None] + _offs(cn, N)[None, None, :]
    for idx, n in ((ai, la), (bi, lb), (ci, lc)):
        assert idx.numel() == 0 or (int(idx.min()) >= 1 and int(idx.max()) < n - 1), c["id"]
    assert ci.flatten().unique().numel() == ci.numel(), (c["id"], "the C maps overlap")
    A = torch.full((la,), float("nan"))
    B = torch.full((lb,), float("nan"))
    A[ai.flatten()] = _ints(gen, ai.numel())
    B[bi.flatten()] = _ints(gen, bi.numel())
    prod = (A[ai].double() @ B[bi].double())[inv]  # (Z, M, N)
    assert bool(torch.isfinite(prod).all())
    exp = alpha * prod
    sent = torch.tensor([SENT_BITS], dtype=torch.int32).view(torch.float32).item()
    C = torch.full((lc,), sent)
    if beta != 0.0:
        C0 = _ints(gen, Z, M, N)
        C[ci.flatten()] = C0.flatten()
        exp = exp + beta * C0.double()
    else:
        C[ci.flatten()] = float("nan")
    bias = None
    if c["bias"]:
        bias = torch.full((lbias,), float("nan"))
        bv = _ints(gen, N)
        bias[torch.arange(N) * c["bias_stride"]] = bv
        exp = exp + bv.double()[None, None, :]
    if c["relu"]:
        exp = exp.clamp_min(0.0)
    want = torch.full((lc,), sent)
    want[ci.flatten()] = exp.float().flatten()
    inside = torch.zeros(lc, dtype=torch.bool)
    inside[ci.flatten()] = True
    return A, B, C, bias, want, inside, ci


def run_exact(c, bf16=False):
    """Run the case and require the exact result; returns the output buffer."""
    _need_gpu()
    from dstagnn_drought_amd import _lib
    A, B, C, bias, want, inside, ci = build(c)
    Ad, Bd, bd = A.cuda(), B.cuda(), (bias.cuda() if bias is not None else None)
    ops = _lib.load()
    outs = []
    prev = ops.set_gemm_bf16(1 if bf16 else 0)
    try:
        for _ in range(2 if c["twice"] else 1):
            Cd = C.cuda()
            _launch(c, Ad, Bd, Cd, bd)
            torch.cuda.synchronize()
            outs.append(Cd.cpu())
    finally:
        ops.set_gemm_bf16(prev)
    got = outs[0]
    p = gc.plan_case(c, bf16=bf16)
    what = f"{c['id']} (template {p['key']}, splitk {p['splitk']} x {p['kchunk']}, skinny {p['skinny']})"
    g_in, w_in = got[inside], want[inside]
    if not torch.equal(g_in, w_in):
        bad = ~(g_in == w_in)
        first = int(torch.nonzero(bad)[0])
        pos = int(torch.nonzero(inside)[first])
        zmn = tuple(int(v) for v in torch.nonzero(ci == pos)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {g_in.numel()} outputs differ, {int(torch.isnan(g_in).sum())} "
                             f"NaN; first at (z, m, n) = {zmn}: got {float(g_in[first])}, want {float(w_in[first])}")
    touched = got.view(torch.int32)[~inside] != SENT_BITS
    assert not bool(touched.any()), f"{what}: {int(touched.sum())} C elements outside the image were written"
    if len(outs) > 1:
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), f"{what}: a rerun changed bits"
    return got


# ---------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [k for k in REACHABLE_TILED if k[0] != "bf"], ids=_key_id)
def test_tiled_template_exact(key):
    """One case per fp32 tiled template (f32 and the two-level-accumulation a2 units)."""
    c = case_for(key)
    assert gc.plan_case(c)["key"] == key
    run_exact(c)


@pytest.mark.parametrize("key", [k for k in REACHABLE_TILED if k[0] == "bf"], ids=_key_id)
def test_tiled_template_exact_bf16(key):
    """The same table under set_gemm_bf16(1) (restored in run_exact's finally): integers in
    [-4, 4] are exact in bf16 and the accumulation is fp32, so the result is still exact.  The
    bf16 variant has no a2 and no skinny kernel (plan_gemm / plan_skinny gate on g_bf16)."""
    c = case_for(key)
    p = gc.plan_case(c, bf16=True)
    assert p["key"] == key and not p["acc2"] and p["skinny"] is None
    run_exact(c, bf16=True)


@pytest.mark.parametrize("c", SKINNY_CASES, ids=lambda c: c["id"])
def test_skinny_template_exact(c):
    """Every (MT, NT, A4) of skinny_dw_kernel, both fold depths, a last workgroup whose tail
    waves have an empty or partial k range; each case twice with identical bits."""
    assert gc.plan_case(c)["skinny"] is not None and c["twice"]
    run_exact(c)


@pytest.mark.parametrize("c", SPLITK_CASES, ids=lambda c: c["id"])
def test_splitk_exact(c):
    """Plain split-K (slabs <= kAcc2MinK, splitk_reduce_kernel): a short last slab, a splitk
    re-derived from the rounded kchunk, red_g > 1, and K = 4095 one below the skinny gate."""
    p = gc.plan_case(c)
    assert p["splitk"] > 1 and not p["acc2"] and p["skinny"] is None
    run_exact(c)


@pytest.mark.parametrize("c", EDGE_CASES, ids=lambda c: c["id"])
def test_map_edges_exact(c):
    """Index-map edges: negative k strides, div = 1, div > count, a two-level c_m scatter with
    ReLU + beta + a strided bias, two-level z maps, M = N = K = 1, K = 0."""
    run_exact(c)


def test_acc2_randn():
    """An a2 template on non-integer data at the existing GEMM bound (1e-5 sqrt(K) of the
    result's scale, tests/test_gpu_parity.py close())."""
    _need_gpu()
    from test_gpu_parity import close
    key = ("a2", 0, False, True, True, 4, 4)
    c = dict(case_for(key), alpha=1.0, beta=0.0, bias=False, relu=False)
    assert gc.plan_case(c)["key"] == key
    M, N, K, Z = c["M"], c["N"], c["K"], c["batch"]
    am, ak, az, bk, bn, bz, cm, cn, cz = c["maps"]
    la, lb, lc, _ = _sizes(c)
    gen = torch.Generator().manual_seed(5)
    A, B = torch.randn(la, generator=gen), torch.randn(lb, generator=gen)
    ai = c["offs"][0] + _offs(am, M)[:, None] + _offs(ak, K)[None, :]
    bi = c["offs"][1] + _offs(bz, Z)[:, None, None] + _offs(bk, K)[None, :, None] + _offs(bn, N)[None, None, :]
    ci = c["offs"][2] + _offs(cz, Z)[:, None, None] + _offs(cm, M)[None, :, None] + _offs(cn, N)[None, None, :]
    ref = (A[ai].double()[None] @ B[bi].double()).float()
    Cd = torch.zeros(lc, device="cuda")
    _launch(c, A.cuda(), B.cuda(), Cd, None)
    torch.cuda.synchronize()
    close(Cd.cpu()[ci], ref, tol=1e-5 * K ** 0.5, what="acc2 randn")


LOG_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
import test_gpu_gemm as G
from dstagnn_drought_amd import _lib
ops = _lib.load()
for c, bf in G.all_runs():
    sys.stderr.write("[case] %s %d\\n" % (c["id"], bf)); sys.stderr.flush()
    prev = ops.set_gemm_bf16(1 if bf else 0)
    try:
        G.launch_only(c)
    finally:
        ops.set_gemm_bf16(prev)
torch.cuda.synchronize()
print("LOG_OK")
"""


def _child(code):
    e = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", DSTAGNN_GEMM_LOG="1")
    r = subprocess.run([sys.executable, "-c", code.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], cwd=ROOT,
                       env=e, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0 and "LOG_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stderr.splitlines()


def test_log_matches_mirror():
    """The mirror against the library's own plan: a child with DSTAGNN_GEMM_LOG=1 runs every
    case once; exactly one "[gemm]" line follows each case id, and its cfg, splitk, akc, bnc,
    ktwo, va, vb, bf, acc2, workgroups and skinny kpw / nwg / ngrp / mt / nt / a4 equal the
    mirror's."""
    _need_gpu()
    lines = [ln for ln in _child(LOG_CHILD) if ln.startswith(("[case]", "[gemm]"))]
    runs = all_runs()
    assert len(lines) == 2 * len(runs), f"{len(lines)} log lines for {len(runs)} cases"
    bad = []
    for (c, bf), head, body in zip(runs, lines[0::2], lines[1::2]):
        assert head == "[case] %s %d" % (c["id"], bf) and body.startswith("[gemm]"), (head, body)
        probs = gc.parse_log_line(body)
        assert probs is not None and len(probs) == 1, body
        diff = gc.log_mismatch(gc.plan_case(c, bf16=bf), probs[0])
        if diff:
            bad.append(f"{c['id']}: " + ", ".join(diff))
    assert not bad, "log != mirror:\n" + "\n".join(bad)


BLOCK_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
import dstagnn_drought_amd as D
import test_gpu_parity as T
N, Tn, K, h, Dm, dk, C = T.CONFIGS["pems08"]
for first in (False, True):
    for B in (2, 32):
        ref, p, x, res, cheb, apa, dims, gen = T._oracle_case(B, N, Tn, K, h, Dm, dk, C, first, 0 if first else 1, seed=3)
        F = x.shape[2]
        blk = D.DSTAGNN_block("cpu", F, F, K, C, C, 1, cheb, apa, apa, N, Tn, Dm, dk, dk, h)
        blk.load_state_dict(p)
        blk = blk.cuda().eval()
        xg = x.cuda().requires_grad_(True)
        rg = res.cuda().requires_grad_(True) if torch.is_tensor(res) else 0
        out, re_at = blk(xg, rg)
        (out.sum() + re_at.sum()).backward()
        torch.cuda.synchronize()
print("LOG_OK")
"""


def table_keys():
    """Every template key a direct fp32 / a2 / skinny case reaches, by the mirror."""
    return {gc.plan_case(c, bf16=bf)["key"] for c, bf in all_runs()}


def test_block_runs_only_pinned_templates():
    """The tiled and skinny templates a PEMS08 inner and first block run (forward and backward,
    B = 2 and B = 32, from the library's log) are all templates a direct case pins.  Epilogue
    features the public descriptor does not expose (the column-sum column ones=1, masks, output
    maps), grouped launches and K-concatenated launches are runtime variations of these
    templates (kcat: its own instantiation) and stay with the block parity tests."""
    _need_gpu()
    logged = {}
    for ln in _child(BLOCK_CHILD):
        if ln.startswith("[gemm]"):
            for f in gc.parse_log_line(ln) or []:
                logged.setdefault(f["key"], ln)
    assert logged, "the block logged no GEMM"
    have = table_keys()
    missing = {k: v for k, v in logged.items() if k not in have}
    print("block keys:", sorted(logged, key=str))
    assert not missing, "the block runs templates no direct case pins:\n" + "\n".join(
        f"{k}: {v}" for k, v in sorted(missing.items(), key=str))
