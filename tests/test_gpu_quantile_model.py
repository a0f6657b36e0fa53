"""GPU: the quantile head through the model and the driver.

Head: DSTAGNNHeadFunction (head.hip) at the output widths P Q a quantile head gives it, against
oracle.dstagnn_ref.model_head, forward and every gradient.
Full model: make_model(quantiles=(0.1, 0.5, 0.9)) at the geometry of
tests/test_gpu_multifeature.py::test_model_vs_fp64_helper (the smallest a GPU test builds), with
QuantileLoss + backward, against the fp64 helper model with num_for_predict = 3 P, the same
parameters and the float64 pinball restatement.
Both at test_gpu_parity's rule, restated here: max |got - want| <= TOL * max(1, max |want|),
TOL = 1e-4.
Driver: run() on the g12 training fixture (20 % of the series NaN, streamed, mean fill, two
epochs): the calibration scores against the float64 restatement over predictions recomputed batch
by batch (1e-6), the point scores against ForecastMetrics fed the point_index column, the files.

Measured on the MI355X: head and model 4.8e-7 of the scale at most; driver scores 2.9e-9 at most.
"""
import json
import os

import numpy as np
import pytest
import torch

import multifeature_ref as mfr
import test_gpu_multifeature as tmf
import test_gpu_parity as tp
import test_gpu_quantile_metrics as tqm

pytestmark = pytest.mark.gpu

TOL = 1e-4
NAN = float("nan")
LEVELS = (0.1, 0.5, 0.9)


def close(a, b, tol=TOL, what=""):
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(np.abs(b).max()) if b.size else 1.0)
    err = float(np.abs(a - b).max()) if b.size else 0.0
    print(f"{what}: err {err / scale:.3e} of the scale")
    assert err <= tol * scale, f"{what}: max err {err:.3e} > {tol:.0e} * {scale:.3e}"


_no_arpack_draws = tmf._no_arpack_draws  # (autouse) a model built here leaves ARPACK's generator alone


@pytest.mark.parametrize("P,Q", [(5, 7), (12, 3), (12, 16)], ids=["width35", "width36", "width192"])
def test_head_at_quantile_widths_vs_oracle(P, Q):
    tp._need_gpu()
    from oracle import dstagnn_ref as ref
    from dstagnn_drought_amd.head_fn import DSTAGNNHeadFunction
    B, N, C, T, nb, O, W = 3, 37, 16, 12, 2, 128, P * Q
    gen = torch.Generator().manual_seed(100 + W)
    outs = [torch.randn(B, N, C, T, generator=gen) for _ in range(nb)]
    final = {"final_conv.weight": torch.randn(O, nb * T, 1, C, generator=gen) * 0.05,
             "final_conv.bias": torch.randn(O, generator=gen),
             "final_fc.weight": torch.randn(W, O, generator=gen) * 0.1,
             "final_fc.bias": torch.randn(W, generator=gen)}
    dy = torch.randn(B, N, W, generator=gen)
    fr = {k: v.double().requires_grad_(True) for k, v in final.items()}
    orr = [o.double().requires_grad_(True) for o in outs]
    y_ref = ref.model_head(fr, orr)
    y_ref.backward(dy.double())
    fg = {k: v.cuda().requires_grad_(True) for k, v in final.items()}
    og = [o.cuda().requires_grad_(True) for o in outs]
    y = DSTAGNNHeadFunction.apply(fg["final_conv.weight"], fg["final_conv.bias"], fg["final_fc.weight"],
                                  fg["final_fc.bias"], *og)
    assert y.shape == (B, N, W)
    y.view(B, N, P, Q).backward(dy.cuda().view(B, N, P, Q))  # the view the quantile model returns
    close(y, y_ref, what=f"head {W} y")
    for k in final:
        close(fg[k].grad, fr[k].grad, what=f"head {W} {k}")
    for j in range(nb):
        close(og[j].grad, orr[j].grad, what=f"head {W} d out_{j}")


def pinball64(y, t, levels):
    """The float64 pinball loss of y (..., Q) against t (...), autograd-able; the fp32 levels."""
    tau = torch.tensor(np.asarray(levels, dtype=np.float32).astype(np.float64))
    omt = torch.tensor((np.float32(1.0) - np.asarray(levels, dtype=np.float32)).astype(np.float64))
    d = y - t[..., None]
    return torch.where(d > 0, omt * d, tau * -d).mean()


def test_quantile_model_and_loss_vs_fp64_helper():
    tp._need_gpu()
    import dstagnn_drought_amd as D_
    from oracle import dstagnn_ref as ref
    N, T, K, h, D, dk, F, B, P, C, nb_block = 16, 12, 3, 3, 64, 32, 4, 2, 12, 8, 2
    Q = len(LEVELS)
    cheb, apa, tmd = tmf._graph(N, K, 7)
    torch.manual_seed(11)
    net = D_.make_model("cpu", F, nb_block, F, K, C, C, 1, tmd, apa, apa, P, T, N, D, dk, dk, h, multi_feature=True,
                        quantiles=LEVELS)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    assert sd["final_fc.weight"].shape == (P * Q, 128) and net.point_index == 1
    net = net.cuda().eval()
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(B, N, F, T, generator=gen)
    target = torch.randn(B, N, P, generator=gen)
    dims = dict(n_heads=h, d_k=dk, d_v=dk, K=K)
    seen = []
    hooks = [b.register_forward_pre_hook(lambda m, a: seen.append((m, a[0].detach(), a[1]))) for b in net.BlockList]
    xg = x.cuda().requires_grad_(True)
    y = net(xg)
    for hk in hooks:
        hk.remove()
    assert y.shape == (B, N, P, Q) and y.is_contiguous()
    loss = D_.QuantileLoss(LEVELS)(y, target.cuda())
    loss.backward()
    # the HIP blocks' ReLU decisions go to the helper, as test_model_vs_fp64_helper hands them over
    masks = [tmf.hip_relu_masks(m, xi, ri.detach() if torch.is_tensor(ri) else ri) for m, xi, ri in seen]
    sd.pop("quantile_levels")
    blocks, final = ref.split_state_dict(sd, nb_block)
    cheb_net = [c.clone() for c in net.BlockList[0].cheb_conv_SAt.cheb_stack.cpu().unbind(0)]
    bl = [{k: v.double().requires_grad_(True) for k, v in b.items()} for b in blocks]
    fi = {k: v.double().requires_grad_(True) for k, v in final.items()}
    xx = x.double().requires_grad_(True)
    pre = [{} for _ in blocks]
    yy = mfr.model_forward(bl, fi, xx, [c.double() for c in cheb_net], apa.double(), dims, masks=masks, handoff=[],
                           pre_out=pre)  # num_for_predict = 3 P: (B, N, 36)
    assert yy.shape == (B, N, P * Q)
    for i, (m3, pr) in enumerate(zip(masks, pre)):  # ReLU-aware, as there
        for m, name in zip(m3, ("z", "z_tco", "z_r")):
            z = pr[name]
            flip = m != (z > 0)
            if bool(flip.any()):
                assert float(z[flip].abs().max()) <= tp.RELU_EPS * float(z.abs().max()), (i, name)
    want = pinball64(yy.view(B, N, P, Q), target.double(), LEVELS)
    want.backward()
    close(y, yy.detach().view(B, N, P, Q), what="model y")
    close(loss, want.detach(), what="model loss")
    close(xg.grad, xx.grad, what="model dx")
    grads = {f"BlockList.{i}.{k}": v.grad for i, b in enumerate(bl) for k, v in b.items()}
    grads.update({k: v.grad for k, v in fi.items()})
    for n, prm in net.named_parameters():
        if grads[n] is None:
            assert prm.grad is None, n
        else:
            close(prm.grad, grads[n], what=f"model {n}")


def test_driver_trains_and_scores_a_quantile_model(golden_dir, tmp_path):
    tp._need_gpu()
    import configparser
    import test_gpu_metrics_masked as tmm
    from dstagnn_drought_amd import ForecastMetrics
    from dstagnn_drought_amd import train as TR
    conf, td = tmm._g12_gapped(golden_dir, tmp_path)
    torch.cuda.set_device(0)
    lines = []
    res = TR.run(conf, root=os.path.join(td, "exp_q"), log=lines.append, stream_windows=True, missing_value=NAN,
                 input_fill="mean", epochs=2, dropout=0.0, quantiles="0.1,0.5,0.9", test_metrics=True, node_scores=True)
    vals = [h_["val_loss"] for h_ in res["history"]]
    assert len(vals) == 2 and np.isfinite(vals).all() and np.isfinite(res["test_loss"])
    net = res["net"]
    assert net.quantiles == LEVELS and net.point_index == 1
    cp = configparser.ConfigParser()
    cp.read(conf)
    dc, tc = cp["Data"], cp["Training"]
    P, N, bs, Q = int(dc["num_for_predict"]), int(dc["num_of_vertices"]), int(tc["batch_size"]), 3

    # predictions recomputed batch by batch from the returned net
    ws = TR._windowed_series(dc, tc, torch.device("cuda", 0), NAN, "mean", None)
    sp = ws.split("test")
    fm = ForecastMetrics(P, 0.0, "cuda", missing_value=NAN, num_nodes=N)
    preds, targets = [], []
    with torch.no_grad():
        for b in range(0, sp.x.shape[0], bs):
            xb, yb = TR._cut(sp.x, sp.y, b, b + bs)
            out = net(xb)
            assert out.shape[1:] == (N, P, Q)
            fm.update(out[..., 1], yb)
            preds.append(out.cpu().numpy())
            targets.append(yb.cpu().numpy())
    p, t = np.concatenate(preds, 0), np.concatenate(targets, 0)
    assert np.isnan(t).any() and np.isfinite(p).all()

    # the point scores are ForecastMetrics over the point_index column, in the same keys
    assert res["test_metrics"] == fm.compute()
    for k, v in fm.scores().items():
        assert np.array_equal(res["test_scores"][k], v, equal_nan=True), k
    for k, v in fm.node_scores().items():
        assert np.array_equal(res["test_node_scores"][k], v, equal_nan=True), k

    # the calibration scores against the float64 restatement, 1e-6
    from dstagnn_drought_amd import QuantileMetrics
    hsum, _ = tqm.ref_sums(p, t, LEVELS, NAN, (0, 1))
    nsum, _ = tqm.ref_sums(p, t, LEVELS, NAN, (0, 2))
    assert (hsum[:, 0] > 0).all()
    want = QuantileMetrics.scores_of_table(hsum)       # (the arithmetic itself: tests/test_quantile_cpu.py)
    nwant = QuantileMetrics.scores_of_table(nsum, overall=False)
    for got_s, want_s, what in ((res["test_quantile_scores"], want, "horizon"),
                                (res["test_node_quantile_scores"], nwant, "node")):
        assert sorted(got_s) == sorted(want_s)
        for k in want_s:
            a, b = got_s[k], want_s[k]
            assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), (what, k)
            ok = ~np.isnan(b)
            err = float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1.0))) if ok.any() else 0.0
            print(f"driver {what} {k}: worst {err:.2e}")
            assert err <= 1e-6, (what, k, err)
    qs = res["test_quantile_scores"]
    assert qs["coverage"].shape == (P + 1, Q) and qs["interval_width"].shape == (P + 1, 1)

    # one line per horizon and one overall, after the point scores' lines; the files
    ql = [ln for ln in lines if ln.startswith("Test quantiles ")]
    assert len(ql) == P + 1 and ql[-1].startswith("Test quantiles overall: ")
    assert "coverage[0.1] %.4f" % qs["coverage"][-1, 0] in ql[-1] and "mean_pinball %.4f" % qs["mean_pinball"][-1] in ql[-1]
    pp = res["params_path"]
    with open(os.path.join(pp, "test_quantile_scores.json")) as f:
        saved = json.load(f)
    assert saved["quantiles"] == list(LEVELS) and saved["point_index"] == 1
    for k in qs:
        assert np.array_equal(np.array(saved[k], dtype=np.float64), qs[k], equal_nan=True), k
    with np.load(os.path.join(pp, "test_node_quantile_scores.npz")) as f:
        assert sorted(f.files) == sorted(qs)
        assert all(np.array_equal(f[k], res["test_node_quantile_scores"][k], equal_nan=True) for k in qs)
    assert os.path.exists(os.path.join(pp, "test_metrics.json")) and os.path.exists(os.path.join(pp, "test_node_scores.npz"))

    # predict_and_save_results_mstgcn keeps the quantile axis and the levels
    loader = [TR._cut(sp.x, sp.y, b, b + bs) for b in range(0, sp.x.shape[0], bs)]
    lst = TR.predict_and_save_results_mstgcn(net, loader, torch.from_numpy(t), 7, ws.mean, ws.std, td, "test",
                                             missing_value=NAN, quantiles=LEVELS)
    with np.load(os.path.join(td, "output_epoch_7_test.npz")) as f:
        assert f["prediction"].shape == p.shape and np.array_equal(f["prediction"], p)
        assert np.array_equal(f["quantiles"], np.asarray(LEVELS, dtype=np.float32))
    assert lst == res["test_metrics"]

    # a checkpoint saved with other levels refuses to load; the right levels load
    best = os.path.join(pp, f"epoch_{res['best_epoch']}.params")
    other = TR.build(cp, torch.device("cuda"), None, (0.05, 0.5, 0.95))
    with pytest.raises(ValueError, match="quantile_levels"):
        TR.load_best(other, best)
    same = TR.build(cp, torch.device("cuda"), None, LEVELS)
    TR.load_best(same, best)
    assert all(torch.equal(v, net.state_dict()[k]) for k, v in same.state_dict().items())
    with pytest.raises(RuntimeError):  # and a point model does not take it
        TR.load_best(TR.build(cp, torch.device("cuda")), best)
