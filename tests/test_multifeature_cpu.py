"""Multi-feature first block, the parts that need no device: the fp64 helper against the
reference-pinned oracle, the constructors, the default's unchanged failure, the C ABI's flag bit
(through ctypes with the unchanged struct), and the training driver's option.
"""
import configparser
import ctypes
import os

import numpy as np
import pytest
import torch

import multifeature_ref as mfr
import test_abi_module_cpu as abi

FIRST_MULTI = 256  # include/dstagnn.h DSTAGNN_TRAIN_FIRST_MULTI
PATH_FIRST_MULTI, PATH_GTU_FUSED = 512, 64 | 128


@pytest.fixture(autouse=True)
def _no_arpack_draws(monkeypatch):
    """make_model's scaled_Laplacian asks ARPACK for lambda_max with a start vector drawn from
    ARPACK's own generator, whose state lives as long as the process: a model built here would
    move the Chebyshev polynomials of every test that runs later by ~1e-6.  These tests take the
    exact dense eigenvalue instead and leave that state alone."""
    import scipy.sparse.linalg as sla

    def eigs(A, k=1, which="LR", **kw):
        ev = np.linalg.eigvals(np.asarray(A))
        return ev[np.argsort(-ev.real)[:k]], None
    monkeypatch.setattr(sla, "eigs", eigs)


def _graph(N, K, seed=0):
    import dstagnn_drought_amd as D
    rs = np.random.RandomState(seed)
    tmd, pa = np.eye(N), np.zeros((N, N))
    for i in range(N):
        tmd[i, rs.choice(N, 2, replace=False)] = 1.0
        pa[i, rs.choice(N, 4, replace=False)] = 1.0
    Lap = np.diag(tmd.sum(axis=1)) - tmd
    ev = np.linalg.eigvals(Lap)
    Lt = (2.0 * Lap) / ev[np.argmax(ev.real)].real - np.eye(N)
    return [torch.from_numpy(c).float() for c in D.cheb_polynomial(Lt, K)][:K], torch.from_numpy(pa).float(), tmd


# ---------------------------------------------------------------------------------------------
# the helper is the oracle where the oracle is defined
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [False, True])
def test_helper_at_f1_is_the_oracle_bit_for_bit(train):
    from oracle import dstagnn_ref as ref
    B, N, T, K, h, D, dk, C = 2, 9, 12, 3, 2, 16, 8, 8
    gen = torch.Generator().manual_seed(3)
    cheb, apa, _ = _graph(N, K)
    dims = dict(n_heads=h, d_k=dk, d_v=dk, K=K)
    p = ref.random_block_params(gen, 1, 1, K, C, N, T, D, dk, dk, h)
    x = torch.randn(B, N, 1, T, generator=gen)
    dm = None
    if train:
        dm = ((torch.rand(B, N, D, generator=gen) > 0.05).float() / 0.95,
              (torch.rand(B, C, N, T, generator=gen) > 0.05).float() / 0.95)
    for hoist in (False, True):
        a = ref.block_forward(p, x, 0, cheb, apa, dims, train=train, drop_masks=dm, hoist=hoist)
        b = mfr.block_forward(p, x, 0, cheb, apa, dims, first=True, train=train, drop_masks=dm, hoist=hoist)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # ... and an inner block (first=False) too, with the ReLU-decision hooks handed over
    p = ref.random_block_params(gen, C, C, K, C, N, T, D, dk, dk, h)
    x = torch.randn(B, N, C, T, generator=gen)
    res = torch.randn(B, 1, h, T, T, generator=gen)
    pre_a, pre_b = {}, {}
    m = (torch.rand(B, N, C, T, generator=gen) > 0.5, torch.rand(B, C, N, T, generator=gen) > 0.5,
         torch.rand(B, C, N, T, generator=gen) > 0.5)
    a = ref.block_forward(p, x, res, cheb, apa, dims, hoist=True, relu_mask=m[0], tail_masks=m[1:], pre_out=pre_a)
    b = mfr.block_forward(p, x, res, cheb, apa, dims, first=False, relu_mask=m[0], tail_masks=m[1:], pre_out=pre_b)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(pre_a[k], pre_b[k]) for k in ("z", "z_tco", "z_r"))


def test_helper_multi_feature_shapes_and_every_parameter_has_a_gradient():
    B, N, T, K, h, D, dk, C, F = 2, 9, 12, 2, 2, 16, 8, 8, 4
    gen = torch.Generator().manual_seed(4)
    cheb, apa, _ = _graph(N, K)
    dims = dict(n_heads=h, d_k=dk, d_v=dk, K=K)
    p = {k: v.double() for k, v in mfr.random_block_params(gen, F, K, C, N, T, D, dk, dk, h).items()}
    assert p["residual_conv.weight"].shape == (C, F, 1, 1) and p["pre_conv.weight"].shape == (D, T, 1, F)
    x = torch.randn(B, N, F, T, generator=gen).double()
    out, re_at, gx, gra, grads = mfr.block_forward_backward(
        p, x, 0, [c.double() for c in cheb], apa.double(), dims, torch.randn(B, N, C, T, generator=gen).double(),
        torch.randn(B, F, h, T, T, generator=gen).double())
    assert out.shape == (B, N, C, T) and re_at.shape == (B, F, h, T, T) and gx.shape == x.shape and gra is None
    assert out.dtype == torch.float64
    assert all(g is not None and bool(g.abs().sum() > 0) for g in grads.values()), \
        [k for k, g in grads.items() if g is None]


# ---------------------------------------------------------------------------------------------
# constructors
# ---------------------------------------------------------------------------------------------
def _model(F, multi_feature=None, nb_block=2, C=8, seed=5):
    import dstagnn_drought_amd as D_
    N, T, K, h, D, dk = 10, 12, 3, 2, 16, 8
    _, apa, tmd = _graph(N, K)
    kw = {} if multi_feature is None else {"multi_feature": multi_feature}
    torch.manual_seed(seed)
    return D_.make_model("cpu", F, nb_block, F, K, C, C, 1, torch.from_numpy(tmd).float(), apa, apa, 12, T, N, D, dk,
                         dk, h, **kw)


def test_constructor_shapes_and_key_order():
    F, C, D, T = 4, 8, 16, 12
    default, multi = _model(F), _model(F, True, nb_block=3)
    sd, sm = default.state_dict(), multi.state_dict()
    keys = [k for k in sm if not k.startswith("BlockList.2.")]
    assert keys == list(sd)  # names and registration order unchanged
    assert [k[12:] for k in sm if k.startswith("BlockList.2.")] == [k[12:] for k in sm if k.startswith("BlockList.1.")]
    assert sm["BlockList.0.pre_conv.weight"].shape == (D, T, 1, F)
    assert sm["BlockList.1.pre_conv.weight"].shape == (D, T, 1, C) == sm["BlockList.2.pre_conv.weight"].shape
    assert sd["BlockList.1.pre_conv.weight"].shape == (D, T, 1, F * C)  # the reference's width, as ever
    assert sm["BlockList.0.residual_conv.weight"].shape == (C, F, 1, 1)
    assert sm["BlockList.0.cheb_conv_SAt.Theta.0"].shape == (F, C)
    assert sm["BlockList.0.EmbedT.pos_embed.weight"].shape == (T, 10)
    assert multi.multi_feature and multi.BlockList[0].multi_feature and not multi.BlockList[1].multi_feature


def test_switch_with_one_feature_builds_the_default_model():
    a, b = _model(1).state_dict(), _model(1, True).state_dict()
    assert list(a) == list(b)
    assert all(a[k].shape == b[k].shape and torch.equal(a[k], b[k]) for k in a)  # same RNG draws


@pytest.mark.parametrize("F", [0, 9, 32])
def test_feature_limit_is_a_value_error_that_names_it(F):
    import dstagnn_drought_amd as D_
    cheb, apa, _ = _graph(10, 3)
    with pytest.raises(ValueError, match=r"1 <= F <= 8"):
        D_.DSTAGNN_block("cpu", F, F, 3, 8, 8, 1, cheb, apa, apa, 10, 12, 16, 8, 8, 2, multi_feature=True)
    with pytest.raises(TypeError):  # keyword-only: the positional reference signature is unchanged
        D_.DSTAGNN_block("cpu", 4, 4, 3, 8, 8, 1, cheb, apa, apa, 10, 12, 16, 8, 8, 2, True)


def test_default_still_raises_the_golden_message(golden_dir):
    import json
    import dstagnn_drought_amd as D_
    with open(os.path.join(golden_dir, "g9_gambia_error.json")) as f:
        golden = json.load(f)
    cheb, apa, _ = _graph(10, 3)
    blk = D_.DSTAGNN_block("cpu", 4, 4, 3, 8, 8, 1, cheb, apa, apa, 10, 12, 16, 8, 8, 2)
    with pytest.raises(RuntimeError, match=r"The size of tensor a \(4\) must match the size of tensor b \(8\)"):
        blk(torch.zeros(1, 10, 4, 12), 0)
    assert "must match the size of tensor b" in json.dumps(golden)
    # the switch admits the shape; there is still no CPU path behind it
    multi = D_.DSTAGNN_block("cpu", 4, 4, 3, 8, 8, 1, cheb, apa, apa, 10, 12, 16, 8, 8, 2, multi_feature=True)
    with pytest.raises(RuntimeError, match="HIP"):
        multi(torch.zeros(1, 10, 4, 12), 0)
    with pytest.raises(RuntimeError, match="in_channels = 4"):
        multi(torch.zeros(1, 10, 3, 12), 0)


# ---------------------------------------------------------------------------------------------
# C ABI: the flag bit in dstagnn_block_dims::train, the struct as test_abi_module_cpu builds it
# ---------------------------------------------------------------------------------------------
def _dims(F, C=8, T=12, train=0, N=16):
    return abi.BlockDims(2, N, F, T, 2, 8, 8, 16, 2, C, 0, train, 0.05, 0)


def _sizes(lib, d):
    sv, sc = ctypes.c_size_t(0), ctypes.c_size_t(0)
    return lib.dstagnn_block_sizes(ctypes.byref(d), ctypes.byref(sv), ctypes.byref(sc)), sv.value, sc.value


def test_abi_flag_admits_f_up_to_8_and_sizes_grow_with_f():
    lib = abi.c_abi()
    got = {F: _sizes(lib, _dims(F, train=FIRST_MULTI)) for F in (1, 2, 4, 8)}
    assert all(rc == 0 for rc, _, _ in got.values()), got
    assert got[1][1] < got[2][1] < got[4][1] < got[8][1]      # save: E, u_et, qkv, ... hold B F T rows
    assert got[1][2] < got[2][2] < got[4][2] < got[8][2]      # scratch: gcon_e, du_et, dE, ...
    # the flag at F = 1 plans what the default first block plans; the dropout bit changes nothing
    assert got[1] == _sizes(lib, _dims(1)) == _sizes(lib, _dims(1, train=FIRST_MULTI | 1))
    # E and u_et are (B F T, N) floats each: the save buffer grows by at least that much
    B, N, T = 2, 16, 12
    assert got[4][1] - got[1][1] >= 2 * B * 3 * T * N * 4
    # work buffer of the forward-only call and the save offsets follow
    wb = ctypes.c_size_t(0)
    d = _dims(4, train=FIRST_MULTI)
    assert lib.dstagnn_block_forward_only_size(ctypes.byref(d), ctypes.byref(wb)) == 0 and wb.value > 0
    off, cnt = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.dstagnn_block_save_offset(ctypes.byref(d), 2, ctypes.byref(off), ctypes.byref(cnt)) == 0
    assert cnt.value == B * N * 8 * T and off.value + 4 * cnt.value <= got[4][1]


def test_abi_limit_and_flag_off_errors():
    lib = abi.c_abi()
    rc, _, _ = _sizes(lib, _dims(9, C=32, train=FIRST_MULTI))
    assert rc == 10001  # DSTAGNN_E_SHAPE
    msg = lib.dstagnn_last_error()
    assert b"limit of 8" in msg and b"F = 9" in msg, msg
    rc, _, _ = _sizes(lib, _dims(0, train=FIRST_MULTI))
    assert rc == 10001 and b"non-positive" in lib.dstagnn_last_error()
    for train in (0, 1):  # flag off: today's error, today's text
        rc, _, _ = _sizes(lib, _dims(4, train=train))
        assert rc == 10001
        assert lib.dstagnn_last_error() == \
            b"The size of tensor a (4) must match the size of tensor b (8) at non-singleton dimension 1"


def test_abi_paths_name_the_multi_feature_tail():
    lib = abi.c_abi()

    def paths(d):
        bits = ctypes.c_uint32(0)
        assert lib.dstagnn_block_paths(ctypes.byref(d), ctypes.byref(bits)) == 0
        return bits.value

    for T in (12, 24, 144):
        for F in (2, 4, 8):
            b = paths(_dims(F, C=32, T=T, train=FIRST_MULTI))
            assert b & PATH_FIRST_MULTI and not b & PATH_GTU_FUSED, (T, F, hex(b))
        # F = 1 under the flag is the default first block: same bits, fused GTU at C = 32, T = 12
        assert paths(_dims(1, C=32, T=T, train=FIRST_MULTI)) == paths(_dims(1, C=32, T=T))
    assert paths(_dims(1, C=32, T=12, train=FIRST_MULTI)) & PATH_GTU_FUSED == PATH_GTU_FUSED
    assert not paths(_dims(32, C=32, T=12)) & PATH_FIRST_MULTI


# ---------------------------------------------------------------------------------------------
# the training driver's option
# ---------------------------------------------------------------------------------------------
def test_option_parsing():
    from dstagnn_drought_amd import train as TR
    cp = configparser.ConfigParser()
    cp.read_string("[Training]\nin_channels = 4\n")
    assert TR.model_options(cp["Training"]) is False
    cp.read_string("[Training]\nmulti_feature = true\n")
    assert TR.model_options(cp["Training"]) is True
    ap = TR.arg_parser()
    assert ap.parse_args([]).multi_feature is None  # absent: the configuration decides
    assert ap.parse_args(["--multi-feature"]).multi_feature is True
    TR.check_input_features(4, "4")
    with pytest.raises(ValueError, match=r"F = 2 .* in_channels = 4"):
        TR.check_input_features(2, 4)


def test_run_refuses_data_whose_feature_count_differs(tmp_path):
    """run(multi_feature=True) on prepared data with F = 2 and in_channels = 3: a ValueError that
    names both, before any model is built (so no device is needed)."""
    from dstagnn_drought_amd import data as data_io, train as TR
    td, N, T, P = str(tmp_path), 6, 12, 12
    rs = np.random.RandomState(0)
    for k in ("adj.csv", "stag.csv", "strg.csv"):
        np.savetxt(os.path.join(td, k), (rs.rand(N, N) > 0.6).astype(float), delimiter=",")
    raw = os.path.join(td, "SYN.npz")
    arrays = {}
    for split, S in (("train", 8), ("val", 3), ("test", 3)):
        arrays[split + "_x"] = rs.randn(S, N, 2, T).astype(np.float32)
        arrays[split + "_target"] = rs.randn(S, N, P).astype(np.float32)
    np.savez(data_io.dataset_filename(raw, 1, 0, 0) + ".npz", mean=np.zeros((1, 1, 2, 1)), std=np.ones((1, 1, 2, 1)),
             **arrays)
    conf = os.path.join(td, "mf.conf")
    with open(conf, "w") as f:
        f.write(f"""[Data]
adj_filename = {td}/adj.csv
graph_signal_matrix_filename = {raw}
stag_filename = {td}/stag.csv
strg_filename = {td}/strg.csv
num_of_vertices = {N}
points_per_hour = 12
num_for_predict = {P}
len_input = {T}
dataset_name = SYN

[Training]
in_channels = 3
nb_block = 2
n_heads = 2
K = 2
d_k = 8
d_model = 16
nb_chev_filter = 8
nb_time_filter = 8
batch_size = 4
graph = AG
model_name = dstagnn
num_of_weeks = 0
num_of_days = 0
num_of_hours = 1
start_epoch = 0
epochs = 1
learning_rate = 0.001
""")
    with pytest.raises(ValueError, match=r"F = 2 .* in_channels = 3"):
        TR.run(conf, multi_feature=True, root=os.path.join(td, "exp"), log=lambda *_: None)
    with open(conf, "a") as f:
        f.write("multi_feature = true\n")
    with pytest.raises(ValueError, match=r"F = 2 .* in_channels = 3"):
        TR.run(conf, root=os.path.join(td, "exp"), log=lambda *_: None)
