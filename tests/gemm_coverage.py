"""A plain-Python mirror of the GEMM family's dispatch (dstagnn_drought_amd/csrc/gemm.hip and
gemm_kern.hpp): which kernel template a dstagnn::gemm_f32 call runs, from its shape, its nine
(div, s0, s1) index maps, its three element offsets and the bf16 switch.  No torch, no device.

Every function names the source it mirrors (file:function, line numbers as of this commit).
Default knobs only: no DSTAGNN_GEMM_CFG / _SPLITK / _SKINNY / DSTAGNN_SKINNY_* override, the
default split-K target, no per-call target, no column-sum column, no output map, no mask (the
public descriptor exposes none of them).  Allocation bases are taken as 256-B aligned, so an
operand's 16-B alignment is decided by its element offset alone.

Template keys:
  tiled   (var, cfg, ktwo, akc, bnc, va, vb)     var in "f32" | "bf" | "a2", cfg 0: 64x64,
                                                  1: 128x128, 2: 128x32 (gemm.hip:kCfgs)
  skinny  ("skinny", MT, NT, U, A4)
tests/test_gpu_gemm.py holds one exact case per key; tests/test_gemm_coverage_cpu.py checks the
table against this mirror, and one GPU test checks this mirror against the library's own log.
"""

BKMAX = 32             # gemm_kern.hpp:62
K_SK_WAVES = 16        # gemm.hip:96
K_SK_MAX_WG = 256      # gemm.hip:97
K_SK_GROUP = 16        # gemm.hip:98
K_SKINNY_MIN_K = 4096  # gemm.hip:99
K_SK_MAX_M = 96        # gemm.hip:100
K_ACC2_MIN_K = 1024    # gemm.hip:556
SPLITK_TARGET = 448    # gemm.hip:391 g_splitk_target
MIN_GRID, MIN_K = 128, 512  # gemm.hip:634 plan_gemm
FOLD1_KB = 512         # gemm.hip:533 plan_skinny (DSTAGNN_SKINNY_FOLD1_KB default)
CFG_TILES = ((64, 64), (128, 128), (128, 32))  # gemm.hip:352 kCfgs as (bm, bn)
WS_FLOATS = 8 << 20    # torch_ops.cpp:486 kGemmWsBytes / 4 (block.hip:1673 takes 256 B off the +256)
SK_U = {1: 16, 2: 16, 3: 8, 4: 8, 6: 4}  # gemm.hip:339-343 launch_skinny's SK_L table

MAP_NAMES = ("a_m", "a_k", "a_z", "b_k", "b_n", "b_z", "c_m", "c_n", "c_z")  # torch_ops.cpp:607


def cdiv(a, b):
    return -(-a // b)


# --- index maps (common.hpp:55-109) ------------------------------------------------------------
def two(m):
    """common.hpp:62 make_idx: a map is two-level iff div > 0."""
    return m[0] > 0


def off(m, i):
    """common.hpp:79 ioff: (i % d) * s0 + (i / d) * s1, or i * s0."""
    d, s0, s1 = m
    return (i % d) * s0 + (i // d) * s1 if d > 0 else i * s0


def idx_min(m, count):
    """common.hpp:103 idx_min."""
    d, s0, s1 = m
    if count <= 0:
        return 0
    if d <= 0:
        return min(0, s0 * (count - 1))
    return min(0, s0 * (min(d, count) - 1)) + min(0, s1 * ((count - 1) // d))


def idx_max(m, count):
    """Largest offset over [0, count) (the upper twin of idx_min; buffer sizing only)."""
    d, s0, s1 = m
    if count <= 0:
        return 0
    if d <= 0:
        return max(0, s0 * (count - 1))
    return max(0, s0 * (min(d, count) - 1)) + max(0, s1 * ((count - 1) // d))


# --- 16-B DMA eligibility (gemm.hip:360-366) ---------------------------------------------------
def quad_ok(m):
    """gemm.hip:360."""
    return m[1] % 4 == 0 and (not two(m) or m[2] % 4 == 0)


def rows_quad(m):
    """gemm.hip:361."""
    return m[1] == 1 and (not two(m) or (m[0] % 4 == 0 and m[2] % 4 == 0))


def dma_width(base_off, rowmap, rows, kmap, zmap, kmaj):
    """gemm.hip:362 dma_width; base_off: the operand's element offset from a 256-B aligned base."""
    if base_off % 4 != 0 or not quad_ok(zmap):
        return 1
    if kmaj:
        return 4 if (not two(kmap) and kmap[1] == 1 and quad_ok(rowmap)) else 1
    return 4 if (rows_quad(rowmap) and rows % 4 == 0 and quad_ok(kmap)) else 1


# --- the skinny kernel (gemm.hip:318-345, 518-552) ---------------------------------------------
def skinny_a4(M, K, am, ak, a_off, kpw):
    """gemm.hip:318 skinny_a4.  The kernel's A pointer is A + a_off - abias (plan_gemm,
    gemm.hip:574-578), so with an aligned base its 16-B alignment is (a_off - abias) % 4."""
    abias = -(idx_min(am, M) + idx_min(ak, K))
    quads = ak[1] == 1 and (not two(ak) or ak[0] % 4 == 0) and ak[2] % 4 == 0
    rows = (a_off - abias) % 4 == 0 and abias % 4 == 0 and K % 4 == 0 and kpw % 4 == 0
    return quads and rows and all(off(am, m) % 4 == 0 for m in range(M))


def plan_skinny(M, N, K, batch, am, ak, a_off, bf16, ws_floats):
    """gemm.hip:518 plan_skinny and gemm.hip:329 launch_skinny; None: the tiled kernel."""
    if bf16 or ws_floats <= 0 or batch != 1 or M > K_SK_MAX_M or N > 32 or K < K_SKINNY_MIN_K:
        return None
    kpw = max(4, cdiv(cdiv(K, K_SK_MAX_WG * K_SK_WAVES), 4) * 4)
    nwg = cdiv(K, K_SK_WAVES * kpw)
    P4 = (M * N + 3) // 4 * 4
    ngrp = cdiv(nwg, K_SK_GROUP) if nwg * P4 * 4 > FOLD1_KB * 1024 else 0
    if (nwg + ngrp) * P4 > ws_floats:
        return None
    mt = cdiv(M, 16)
    MT = mt if mt <= 4 else 6
    NT = 2 if N > 16 else 1
    a4 = skinny_a4(M, K, am, ak, a_off, kpw)
    return dict(key=("skinny", MT, NT, SK_U[MT], a4), kpw=kpw, nwg=nwg, ngrp=ngrp)


# --- the tiled kernel (gemm.hip:559-680 plan_gemm, 695-714 launch_plans) ------------------------
def tile_cfg(M, N, K, batch):
    """gemm.hip:620-628: the `best` choice (no DSTAGNN_GEMM_CFG, no output map)."""
    b64 = cdiv(M, 64) * cdiv(N, 64) * batch
    if N <= 32:
        return 2
    return 1 if (b64 >= 4096 and K >= 1024) else 0


def plan_splitk(M, N, K, batch, cfg, ws_floats):
    """gemm.hip:630-656: (blocks, splitk, kchunk, red_g)."""
    bm, bn = CFG_TILES[cfg]
    blocks = cdiv(M, bm) * cdiv(N, bn) * batch
    splitk = 1
    if K > 0 and blocks < MIN_GRID and K >= MIN_K and ws_floats > 0:
        want = min(512, cdiv(SPLITK_TARGET, blocks))
        maxk = K // 128
        splitk = max(1, min(want, maxk))
        while splitk > 1 and batch * splitk * M * N > ws_floats:
            splitk -= 1
    kchunk = K
    if splitk > 1:
        kchunk = cdiv(cdiv(K, splitk), BKMAX) * BKMAX
        splitk = cdiv(K, kchunk)
    if K <= 0:
        splitk, kchunk = 1, 0
    red_g = 1
    while red_g < 64 and red_g * 8 < splitk:
        red_g *= 2
    return blocks, splitk, kchunk, red_g


def plan(M, N, K, batch, maps, offs, bf16=False, ws_floats=WS_FLOATS):
    """The launch plan of one gemm_f32 call.  maps: the nine (div, s0, s1) in MAP_NAMES order;
    offs: (a_off, b_off, c_off).  Returns a dict: `key` (the template that runs), the tiled
    plan's fields as the "[gemm]" log line prints them (cfg, splitk, akc, bnc, ktwo, va, vb, bf,
    acc2, blocks = workgroups; kchunk, red_g), and `skinny` (None or kpw / nwg / ngrp / key).
    The log prints the tiled plan's splitk even when the skinny kernel then takes the call."""
    maps = [tuple(m) + (0,) * (3 - len(m)) for m in maps]
    am, ak, az, bk, bn, bz, cm, cn, cz = maps
    a_off, b_off, c_off = offs
    cfg = tile_cfg(M, N, K, batch)
    blocks, splitk, kchunk, red_g = plan_splitk(M, N, K, batch, cfg, ws_floats)
    acc2 = (not bf16) and cfg in (0, 2) and splitk > 1 and kchunk > K_ACC2_MIN_K  # gemm.hip:662
    akc = not two(ak) and ak[1] == 1        # gemm.hip:663
    bnc = not two(bn) and bn[1] == 1        # gemm.hip:664
    ktwo = two(ak) or two(bk)               # gemm.hip:665
    va = dma_width(a_off, am, M, ak, az, akc)       # gemm.hip:667
    vb = dma_width(b_off, bn, N, bk, bz, not bnc)   # gemm.hip:668
    var = "a2" if acc2 else ("bf" if bf16 else "f32")  # gemm.hip:709 launch_plans
    tiled_key = (var, cfg, ktwo, akc, bnc, va, vb)
    sk = plan_skinny(M, N, K, batch, am, ak, a_off, bf16, ws_floats)  # run_gemm_group, gemm.hip:734
    return dict(key=sk["key"] if sk else tiled_key, tiled_key=tiled_key, cfg=cfg, splitk=splitk, kchunk=kchunk,
                red_g=red_g, blocks=blocks * splitk, akc=akc, bnc=bnc, ktwo=ktwo, va=va, vb=vb, bf=int(bool(bf16)),
                acc2=acc2, skinny=sk)


def plan_case(case, bf16=False):
    """plan() of a case descriptor (tests/test_gpu_gemm.py)."""
    return plan(case["M"], case["N"], case["K"], case["batch"], case["maps"], case["offs"], bf16=bf16)


# --- the "[gemm]" log line (gemm.hip:672-677 plan_gemm, 545-551 plan_skinny, 758-762) -----------
def parse_log_line(line):
    """One "[gemm] ..." stderr line -> a list of problems (a grouped launch joins its problems
    with " | "), each a dict of its integer fields plus `key`; None for a K-concatenated launch
    ("[gemm] kcat ...": its own kernel instantiation, run_gemm_kcat)."""
    body = line.strip()
    assert body.startswith("[gemm]"), line
    body = body[6:].strip()
    if body.startswith("kcat"):
        return None
    out = []
    for part in body.split(" | "):
        f = {}
        for tok in part.split():
            if "=" in tok:
                k, v = tok.split("=", 1)
                f[k] = int(v)
        f["is_skinny"] = " skinny " in " " + part + " "
        if f["is_skinny"]:
            f["key"] = ("skinny", f["mt"], f["nt"], SK_U[f["mt"]], bool(f["a4"]))
        else:
            var = "a2" if f["acc2"] else ("bf" if f["bf"] else "f32")
            f["key"] = (var, f["cfg"], bool(f["ktwo"]), bool(f["akc"]), bool(f["bnc"]), f["va"], f["vb"])
        out.append(f)
    return out


def log_mismatch(p, f):
    """Fields of a parsed log problem `f` that disagree with the mirror's plan `p` (a list of
    "name: log != mirror" strings, empty when they agree)."""
    bad = []
    for name in ("cfg", "splitk", "akc", "bnc", "ktwo", "va", "vb", "bf", "acc2", "blocks"):
        if int(p[name]) != f[name]:
            bad.append(f"{name}: {f[name]} != {int(p[name])}")
    if (p["skinny"] is not None) != f["is_skinny"]:
        bad.append(f"skinny: {f['is_skinny']} != {p['skinny'] is not None}")
    elif p["skinny"]:
        for name in ("kpw", "nwg", "ngrp"):
            if p["skinny"][name] != f[name]:
                bad.append(f"{name}: {f[name]} != {p['skinny'][name]}")
    if tuple(p["key"]) != tuple(f["key"]):
        bad.append(f"key: {f['key']} != {p['key']}")
    return bad
