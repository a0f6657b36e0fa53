"""Reference of record for the multi-feature first block and the multi-feature model.

The reference project cannot run a first block over 1 < F < C features (its three
``num_of_features == 1`` branches stand for "first block"), so there is nothing
to record from it.  This helper composes the UNCHANGED, reference-pinned functions of
``oracle/dstagnn_ref.py`` (embed_t, temporal_attention, pre_conv, embed_s,
spatial_attention_scores, cheb_conv_sat, gtu, layer_norm, model_head) in the order of the
oracle's own ``block_forward``, with those three branches keyed on ``first`` instead of
``F == 1``:

  1. E = LN_N(x.permute(0,2,3,1) + P_T[t, :])          (embed_t at num_of_features = F)
  2. TAt, pre_conv (D, T, 1, F), EmbedS, SAt, cheb_conv_withSAt with Theta_k (F, C)
  3. tco = ReLU(tc);  xres = residual_conv(x) (F -> C, 1x1);  out = LN_C(ReLU(xres + tco))

and the model with the hand-off ``re_At.mean(dim=1, keepdim=True)`` from block 0 to block 1.
With F = 1 and first=True, ``block_forward`` is the oracle's, operation for operation
(tests/test_multifeature_cpu.py holds the two bit-equal).  Whatever dtype the inputs have is the
dtype it works in; the parity tests hand it fp64.
"""
import torch
import torch.nn.functional as F

from oracle import dstagnn_ref as ref


def block_forward(p, x, res_att, cheb, adj_pa, dims, first=True, train=False, drop_masks=None, hoist=True,
                  relu_mask=None, pre_out=None, tail_masks=None):
    """(x_out (B,N,C,T), re_At (B,F,h,T,T)); the arguments and hooks of oracle.block_forward
    (relu_mask / tail_masks: the ReLU decisions of the implementation under test; drop_masks:
    (mask_S (B,N,D), mask_T (B,C,N,T)) scaled by 1/(1-p); pre_out receives the three ReLUs'
    pre-activations "z", "z_tco", "z_r").  first=False: an inner block (F == C), as the oracle."""
    h, dk, dv, K = dims["n_heads"], dims["d_k"], dims["d_v"], dims["K"]
    TEmx = ref.embed_t(p, x) if first else x.permute(0, 2, 3, 1)
    TATout, re_at = ref.temporal_attention(p, TEmx, res_att, h, dk, dv)
    x_TAt = ref.pre_conv(p, TATout)
    SEmx = ref.embed_s(p, x_TAt)
    if train and drop_masks is not None:
        SEmx = SEmx * drop_masks[0]
    STAt = ref.spatial_attention_scores(p, SEmx, K, dk)
    thetas = [p[f"cheb_conv_SAt.Theta.{k}"] for k in range(K)]
    masks = [p[f"cheb_conv_SAt.mask.{k}"] for k in range(K)]
    spatial_gcn = ref.cheb_conv_sat(x, STAt, adj_pa, thetas, masks, cheb, hoist=hoist, relu_mask=relu_mask,
                                    pre_out=pre_out)
    X = spatial_gcn.permute(0, 2, 1, 3)
    tc = torch.cat([ref.gtu(p, "gtu3", X, 3), ref.gtu(p, "gtu5", X, 5), ref.gtu(p, "gtu7", X, 7)], dim=-1)
    tc = tc @ p["fcmy.0.weight"].t() + p["fcmy.0.bias"]
    if train and drop_masks is not None:
        tc = tc * drop_masks[1]
    relu = (lambda z, m: z * m.to(z.dtype)) if tail_masks is not None else (lambda z, m: F.relu(z))  # noqa: E731
    if first:
        z_tco = tc
        xres = F.conv2d(x.permute(0, 2, 1, 3), p["residual_conv.weight"], p["residual_conv.bias"])
    else:
        z_tco = X + tc
        xres = x.permute(0, 2, 1, 3)
    tco = relu(z_tco, tail_masks[0] if tail_masks is not None else None)
    z_r = xres + tco
    if pre_out is not None:
        pre_out["z_tco"], pre_out["z_r"] = z_tco.detach(), z_r.detach()
    out = ref.layer_norm(relu(z_r, tail_masks[1] if tail_masks is not None else None).permute(0, 3, 2, 1),
                         p["ln.weight"], p["ln.bias"]).permute(0, 2, 3, 1)
    return out, re_at


def block_forward_backward(p, x, res_att, cheb, adj_pa, dims, g_out, g_re, first=True, **kw):
    """As oracle.block_forward_backward: (out, re_at, grad_x, grad_res_att | None, {name: grad | None})."""
    pp = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    xx = x.detach().clone().requires_grad_(True)
    ra = res_att.detach().clone().requires_grad_(True) if torch.is_tensor(res_att) else res_att
    out, re_at = block_forward(pp, xx, ra, cheb, adj_pa, dims, first=first, **kw)
    loss = (out * g_out).sum()
    if g_re is not None:
        loss = loss + (re_at * g_re).sum()
    loss.backward()
    gra = ra.grad if torch.is_tensor(ra) else None
    return out.detach(), re_at.detach(), xx.grad, gra, {k: v.grad for k, v in pp.items()}


def model_forward(blocks, final, x, cheb, adj_pa, dims, masks=None, handoff=None, pre_out=None):
    """The multi-feature model: block 0 a multi-feature first block over x (B,N,F,T), the hand-off
    res_att = re_At.mean(dim=1, keepdim=True) (B,1,h,T,T), inner blocks with that broadcast
    res_att, then the oracle's head.  masks: per block None or the triple (relu_mask, tco mask,
    r mask) of that block's ReLU decisions; handoff (list, optional) receives the hand-off tensor;
    pre_out (list of dicts, optional): per block, the ReLUs' pre-activations."""
    need = []
    res_att = 0
    for i, p in enumerate(blocks):
        m = None if masks is None else masks[i]
        kw = {} if m is None else {"relu_mask": m[0], "tail_masks": m[1:]}
        x, res_att = block_forward(p, x, res_att, cheb, adj_pa, dims, first=(i == 0),
                                   pre_out=None if pre_out is None else pre_out[i], **kw)
        if i == 0:
            res_att = res_att.mean(dim=1, keepdim=True)
            if handoff is not None:
                handoff.append(res_att)
        need.append(x)
    return ref.model_head(final, need)


def random_block_params(gen, F_in, K, C, N, T, D, dk, dv, h, first=True):
    """oracle.random_block_params for a multi-feature first block (num_of_d = in_channels = F_in)
    or, first=False, an inner block of the multi-feature model (num_of_d = in_channels = C)."""
    f = F_in if first else C
    return ref.random_block_params(gen, f, f, K, C, N, T, D, dk, dv, h)
