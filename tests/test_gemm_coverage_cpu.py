"""The GEMM case tables (tests/test_gpu_gemm.py) against the mirror of the GEMM dispatch
(tests/gemm_coverage.py): every kernel template must be run by the case built for it.  No
device needed: a case whose shape drifts off its template, or a planner threshold moved past
the cases, fails here and names the template.  (The mirror itself is held to the library's own
log by tests/test_gpu_gemm.py::test_log_matches_mirror.)
"""
import gemm_coverage as gc
import test_gpu_gemm as tg

# Templates the public descriptor cannot reach.  The only family: A k-contiguous (akc) with a
# two-level k map somewhere (ktwo) means B's k map is the two-level one, and B k-major (not bnc)
# is moved by 16-B DMA (vb = 4) only under a single-level unit-stride k map (gemm.hip dma_width,
# kmaj branch).  That is (akc, ktwo, not bnc, vb = 4) x va in {1, 4}: 2 keys per tile shape and
# variant — 3 x 2 (f32) + 3 x 2 (bf) + 2 x 2 (a2).
UNREACHABLE_CAP = 16


def test_every_reachable_key_is_run_by_its_case():
    wrong = []
    for key in tg.TILED_KEYS + tg.SKINNY_KEYS:
        if key in tg.UNREACHABLE:
            continue
        got = gc.plan_case(tg.case_for(key), bf16=key[0] == "bf")["key"]
        if got != key:
            wrong.append(f"{key}: its case runs {got}")
    assert not wrong, "\n".join(wrong)
    assert len(tg.TILED_KEYS) == 96 + 96 + 64 and len(tg.SKINNY_KEYS) == 20


def test_unreachable_is_the_one_documented_family():
    assert len(tg.UNREACHABLE) <= UNREACHABLE_CAP
    for (var, cfg, ktwo, akc, bnc, va, vb), why in tg.UNREACHABLE.items():
        assert ktwo and akc and not bnc and vb == 4, (var, cfg, ktwo, akc, bnc, va, vb)
        assert isinstance(why, str) and "k map" in why


def test_tiled_cases_bite():
    """Clamped rows and columns, a partial k-tile after at least two full ones, more than one
    tile where the tile shape allows, and the variant the key names."""
    for key in tg.REACHABLE_TILED:
        c = tg.case_for(key)
        p = gc.plan_case(c, bf16=key[0] == "bf")
        M, N, K = c["M"], c["N"], c["K"]
        assert M % 32 and N % 32 and K % 32 and (p["splitk"] == 1 or p["kchunk"] % 32 == 0), c["id"]
        last = K - (p["splitk"] - 1) * p["kchunk"]
        assert 0 < last <= p["kchunk"] and min(last, p["kchunk"]) >= 64 + 1, c["id"]
        assert all(o > 0 for o in c["offs"]), c["id"]
        assert p["acc2"] == (key[0] == "a2") and (p["splitk"] > 1) == (key[0] == "a2"), c["id"]
        if key[0] == "a2":
            assert p["kchunk"] > gc.K_ACC2_MIN_K and c["batch"] > 1 and p["skinny"] is None
        if key[1] == 1:
            assert gc.cdiv(M, 64) * gc.cdiv(N, 64) * c["batch"] >= 4096 and K >= 1024
        if key[2]:  # a two-level k map whose period is no power of two
            divs = [m[0] for m in (c["maps"][1], c["maps"][3]) if m[0] > 0]
            assert divs and all(d & (d - 1) for d in divs), c["id"]


def test_skinny_table():
    plans = {c["id"]: gc.plan_case(c) for c in tg.SKINNY_CASES}
    assert all(p["skinny"] for p in plans.values())
    assert {p["key"] for p in plans.values()} == set(tg.SKINNY_KEYS)
    # both fold depths, each under an A4 and a non-A4 template
    for a4 in (False, True):
        depths = {p["skinny"]["ngrp"] > 0 for p in plans.values() if p["key"][4] == a4}
        assert depths == {False, True}, (a4, depths)
    assert plans["sk-fold2-dtheta"]["skinny"] == dict(key=("skinny", 6, 2, 4, True), kpw=16, nwg=255, ngrp=16)
    assert plans["sk-fold2-a1"]["skinny"] == dict(key=("skinny", 6, 2, 4, False), kpw=4, nwg=65, ngrp=5)
    # a last workgroup whose tail waves start past K (empty) and whose wave 0 is partial
    for c in tg.SKINNY_CASES:
        s = plans[c["id"]]["skinny"]
        k0_last_wave = (s["nwg"] * gc.K_SK_WAVES - 1) * s["kpw"]
        if c["K"] in (4100, 4097):
            assert k0_last_wave >= c["K"], c["id"]
    assert {c["K"] % 4 for c in tg.SKINNY_CASES} == {0, 1}
    # A4 off both ways: an m-contiguous A (K % 4 == 0), and the aligned k-contiguous A at K % 4 != 0
    off = [c for c in tg.SKINNY_CASES if not plans[c["id"]]["key"][4]]
    assert any(c["maps"][0][1] == 1 and c["K"] % 4 == 0 for c in off)
    assert any(c["maps"][1] == (0, 1, 0) and c["K"] % 4 for c in off)


def test_splitk_table():
    p = {c["id"]: gc.plan_case(c) for c in tg.SPLITK_CASES}
    c = {c["id"]: c for c in tg.SPLITK_CASES}
    assert all(q["splitk"] > 1 and q["kchunk"] <= gc.K_ACC2_MIN_K and not q["acc2"] and not q["skinny"]
               for q in p.values())
    assert {q["cfg"] for q in p.values()} == {0, 2}
    q = p["splitk-c0-short-last"]
    assert (q["splitk"], q["kchunk"]) == (7, 160) and c["splitk-c0-short-last"]["K"] - 6 * 160 == 40
    for name in ("splitk-c0-rederived", "splitk-c2-rederived"):  # K / 128 = 8 slabs asked for
        assert c[name]["K"] // 128 == 8 and (p[name]["splitk"], p[name]["kchunk"]) == (7, 160)
    assert p["splitk-c0-redg2"]["splitk"] == 14 and p["splitk-c0-redg2"]["red_g"] == 2
    q = p["splitk-c2-k4095"]
    assert q["key"][0] == "f32" and (q["splitk"], q["kchunk"], q["red_g"]) == (26, 160, 4)


def _sk(M, N, K, batch=1, bf16=False):
    lda = K + 4 - K % 4
    maps = [(0, lda, 0), (0, 1, 0), (0, 0, 0), (0, N, 0), (0, 1, 0), (0, 0, 0), (0, N, 0), (0, 1, 0), (0, 0, 0)]
    return gc.plan(M, N, K, batch, maps, (0, 0, 0), bf16=bf16)


def test_dispatch_thresholds():
    # the skinny gate: K = 4095 / 4096, M = 96 / 97, N = 32 / 33, batch 1, fp32 only
    assert _sk(20, 25, 4095)["skinny"] is None and _sk(20, 25, 4096)["skinny"] is not None
    assert _sk(96, 25, 4096)["skinny"] is not None and _sk(97, 25, 4096)["skinny"] is None
    assert _sk(20, 32, 4096)["skinny"] is not None and _sk(20, 33, 4096)["skinny"] is None
    assert _sk(20, 25, 4096, batch=2)["skinny"] is None and _sk(20, 25, 4096, bf16=True)["skinny"] is None
    assert [_sk(m, 7, 4096)["key"][1] for m in (16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96)] == \
        [1, 2, 2, 3, 3, 4, 4, 6, 6, 6, 6]
    assert [_sk(5, n, 4096)["key"][2] for n in (16, 17)] == [1, 2]
    # k per wave: 4 up to 256 * 16 * 4 k, then the next multiple of 4
    assert [_sk(5, 7, k)["skinny"]["kpw"] for k in (16384, 16385, 32768, 32769)] == [4, 8, 8, 12]
    # one fold level up to 512 KB of partials: 64 workgroups x 2048 floats x 4 B, one more workgroup is past
    assert _sk(64, 32, 4096)["skinny"]["ngrp"] == 0 and _sk(64, 32, 4097)["skinny"]["ngrp"] == 5
    # ACC2: kchunk = 1024 / 1056 (batch 64: 64 blocks ask for 7 slabs, and the skinny gate stays shut)
    a, b = _sk(8, 8, 7 * 1024, batch=64), _sk(8, 8, 7 * 1024 + 1, batch=64)
    assert (a["splitk"], a["kchunk"], a["acc2"], a["key"][0]) == (7, 1024, False, "f32")
    assert (b["splitk"], b["kchunk"], b["acc2"], b["key"][0]) == (7, 1056, True, "a2")
    assert _sk(8, 8, 7 * 1024 + 1, batch=64, bf16=True)["key"][0] == "bf"  # fp32 operands only
    # 128x128 tiles: 4095 / 4096 64x64 tiles, K = 1023 / 1024
    assert gc.tile_cfg(65, 65, 1024, 1024) == 1 and gc.tile_cfg(65, 65, 1023, 1024) == 0
    assert gc.tile_cfg(64 * 4095, 64, 1024, 1) == 0 and gc.tile_cfg(64 * 4096, 64, 1024, 1) == 1
    assert gc.tile_cfg(64 * 4096, 32, 1024, 1) == 2 and gc.tile_cfg(100, 33, 77, 1) == 0
    # split-K: 127 / 128 blocks, K = 511 / 512
    assert gc.plan_splitk(64, 64, 512, 127, 0, gc.WS_FLOATS)[1] == 4 and gc.plan_splitk(64, 64, 512, 128, 0, gc.WS_FLOATS)[1] == 1
    assert gc.plan_splitk(64, 64, 511, 127, 0, gc.WS_FLOATS)[1] == 1
    # the workspace clamp: slabs must fit
    assert gc.plan_splitk(64, 64, 512, 127, 0, 64 * 64 * 127 * 3)[1] == 3
    # red_g: the smallest power of two with 8 red_g >= splitk
    assert [gc.plan_splitk(70, 50, 128 * s, 1, 0, gc.WS_FLOATS)[3] for s in (8, 9, 16, 17)] == [1, 2, 2, 4]


def test_dma_width_levers():
    one, row = (0, 1, 0), (0, 80, 0)
    assert gc.dma_width(8, row, 100, one, (0, 0, 0), True) == 4
    assert gc.dma_width(7, row, 100, one, (0, 0, 0), True) == 1          # odd offset
    assert gc.dma_width(8, (0, 81, 0), 100, one, (0, 0, 0), True) == 1   # odd leading dimension
    assert gc.dma_width(8, row, 100, (12, 1, 16), (0, 0, 0), True) == 1  # two-level k map, k-major
    assert gc.dma_width(8, row, 100, one, (0, 81, 0), True) == 1         # odd batch stride
    assert gc.dma_width(8, one, 100, row, (0, 0, 0), False) == 4
    assert gc.dma_width(8, one, 101, row, (0, 0, 0), False) == 1         # row count
    assert gc.dma_width(8, one, 100, (12, 80, 1040), (0, 0, 0), False) == 4
    assert gc.dma_width(8, (6, 1, 8), 100, row, (0, 0, 0), False) == 1   # quads straddle a level


def test_log_line_parser():
    line = ("[gemm] M=96 N=32 K=65280 batch=1 cfg=2 splitk=448 akc=0 bnc=1 ktwo=1 blocks=448 ns=2 va=1 vb=4 bf=0 "
            "ones=0 acc2=0 skinny kpw=16 nwg=255 ngrp=16 mt=6 nt=2 a4=1")
    (f,) = gc.parse_log_line(line)
    assert f["key"] == ("skinny", 6, 2, 4, True) and f["kpw"] == 16 and f["splitk"] == 448
    two = gc.parse_log_line("[gemm] M=1 N=2 K=3 batch=1 cfg=0 splitk=1 akc=1 bnc=1 ktwo=0 blocks=1 ns=2 va=4 vb=1 "
                            "bf=0 ones=0 acc2=0 | M=1 N=2 K=3 batch=1 cfg=0 splitk=1 akc=1 bnc=1 ktwo=0 blocks=1 ns=2 "
                            "va=4 vb=1 bf=1 ones=0 acc2=0")
    assert [f["key"] for f in two] == [("f32", 0, False, True, True, 4, 1), ("bf", 0, False, True, True, 4, 1)]
    assert gc.parse_log_line("[gemm] kcat M=1 N=2 K=3 + M=1 N=2 K=3") is None
