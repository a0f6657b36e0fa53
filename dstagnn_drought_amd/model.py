"""DSTAGNN model surface, MI355X-native (drop-in for model/DSTAGNN_my.py).

Same class names, constructor signatures, submodule / parameter names (hence
identical state_dict keys) and construction order (hence the
identical RNG-driven make_model init, quirk 9) as the reference.  The compute
of DSTAGNN_block — temporal attention, pre_conv, spatial attention,
cheb_conv_withSAt, the three GTUs, fcmy, residual and LayerNorms, forward AND
backward — runs in libdstagnn.so (hand-written gfx950 kernels) through ONE
C++ autograd op per block, ``torch.ops.dstagnn.block`` (csrc/torch_ops.cpp).
There is no CPU/eager fallback: a block called on a non-HIP tensor raises.

Differences from the reference that do not change results:
  * adj_pa and the Chebyshev polynomials are non-persistent buffers (they follow
    .to(device); state_dict keys are unchanged — quirk 10).
  * the T x K softmax loop of cheb_conv_withSAt is computed once per k (quirk 3).
"""
import numpy as np
import torch
import torch.nn as nn

from .block_fn import FLASH_SMALL_N, block_call, slots_of, use_flash
from .head_fn import DSTAGNNHeadFunction
from .graph import cheb_polynomial, scaled_Laplacian

MAX_FIRST_F = 8  # include/dstagnn.h DSTAGNN_MAX_FIRST_F: input features of a multi-feature first block


def _check_first_f(F):
    if not 1 <= F <= MAX_FIRST_F:
        raise ValueError(f"multi_feature: a multi-feature first block takes 1 <= F <= {MAX_FIRST_F} input features, "
                         f"got F = {F} (the limit is {MAX_FIRST_F})")


HIP_ONLY = ("dstagnn_drought_amd: DSTAGNN_block runs only on the MI355X HIP path; "
            "move the model and inputs to a 'cuda' (HIP) device. There is no CPU fallback.")


class SScaledDotProductAttention(nn.Module):
    """Spatial scores Q K^T / sqrt(d_k), no softmax (model/DSTAGNN_my.py:8-22)."""

    def __init__(self, d_k):
        super().__init__()
        self.d_k = d_k


class ScaledDotProductAttention(nn.Module):
    """Temporal attention core (model/DSTAGNN_my.py:24-42); executed inside the HIP block."""

    def __init__(self, d_k, num_of_d):
        super().__init__()
        self.d_k = d_k
        self.num_of_d = num_of_d


class SMultiHeadAttention(nn.Module):
    """model/DSTAGNN_my.py:44-67 — parameters W_Q, W_K (d_model -> d_k * n_heads, no bias)."""

    def __init__(self, DEVICE, d_model, d_k, d_v, n_heads):
        super().__init__()
        self.d_model, self.d_k, self.d_v, self.n_heads, self.DEVICE = d_model, d_k, d_v, n_heads, DEVICE
        self.W_Q = nn.Linear(d_model, d_k * n_heads, bias=False)
        self.W_K = nn.Linear(d_model, d_k * n_heads, bias=False)


class MultiHeadAttention(nn.Module):
    """model/DSTAGNN_my.py:69-100 — W_Q, W_K, W_V, fc and layer_norm over d_model (= N)."""

    def __init__(self, DEVICE, d_model, d_k, d_v, n_heads, num_of_d):
        super().__init__()
        self.d_model, self.d_k, self.d_v, self.n_heads, self.num_of_d = d_model, d_k, d_v, n_heads, num_of_d
        self.DEVICE = DEVICE
        self.W_Q = nn.Linear(d_model, d_k * n_heads, bias=False)
        self.W_K = nn.Linear(d_model, d_k * n_heads, bias=False)
        self.W_V = nn.Linear(d_model, d_v * n_heads, bias=False)
        self.fc = nn.Linear(n_heads * d_v, d_model, bias=False)
        self.layer_norm = nn.LayerNorm(self.d_model)


class cheb_conv_withSAt(nn.Module):
    """K-order Chebyshev graph convolution with spatial attention (model/DSTAGNN_my.py:102-133).
    Parameters Theta.k (in_channels, out_channels) and mask.k (N, N), left uninitialised
    exactly like the reference (make_model initialises them)."""

    def __init__(self, K, cheb_polynomials, in_channels, out_channels, num_of_vertices, DEVICE):
        super().__init__()
        self.K = K
        self.in_channels, self.out_channels, self.DEVICE = in_channels, out_channels, DEVICE
        self.Theta = nn.ParameterList([nn.Parameter(torch.empty(in_channels, out_channels)) for _ in range(K)])
        self.mask = nn.ParameterList([nn.Parameter(torch.empty(num_of_vertices, num_of_vertices)) for _ in range(K)])
        cp = torch.stack([torch.as_tensor(np.asarray(c), dtype=torch.float32) for c in cheb_polynomials[:K]])
        self.register_buffer("cheb_stack", cp.contiguous(), persistent=False)
        # union support of T_0..T_{K-1} (elementwise recurrence => support of L~ u I, quirk 4)
        csc_ptr, csc_row, csr_ptr, csr_col = support_index(cp)
        self.register_buffer("csc_ptr", csc_ptr, persistent=False)
        self.register_buffer("csc_row", csc_row, persistent=False)
        self.register_buffer("csr_ptr", csr_ptr, persistent=False)
        self.register_buffer("csr_col", csr_col, persistent=False)

    def graph(self, adj_pa):
        return {"cheb": self.cheb_stack, "adj_pa": adj_pa, "csc_ptr": self.csc_ptr, "csc_row": self.csc_row,
                "csr_ptr": self.csr_ptr, "csr_col": self.csr_col}

    @property
    def cheb_polynomials(self):
        return list(self.cheb_stack.unbind(0))


def support_index(cheb_stack):
    """int32 CSC (per destination column j: source rows i) and CSR (per row i: columns j)
    of the union support of the stacked Chebyshev polynomials (K,N,N)."""
    nz = (cheb_stack != 0).any(dim=0)
    N = nz.shape[0]

    def pack(m):  # rows of m in order -> (ptr, column indices)
        r, c = torch.nonzero(m, as_tuple=True)
        ptr = torch.zeros(N + 1, dtype=torch.int32)
        ptr[1:] = torch.cumsum(torch.bincount(r, minlength=N), 0).to(torch.int32)
        return ptr, c.to(torch.int32)

    csc_ptr, csc_row = pack(nz.t())
    csr_ptr, csr_col = pack(nz)
    return csc_ptr, csc_row, csr_ptr, csr_col


def _bits(m):
    """(N, ceil(N/32)) int32 words: bit (c % 32) of word [r][c // 32] = m[r][c]."""
    R, C = m.shape
    nw = (C + 31) // 32
    pad = torch.zeros(R, nw * 32, dtype=torch.int64, device=m.device)
    pad[:, :C] = m.to(torch.int64)
    w = (pad.view(R, nw, 32) << torch.arange(32, device=m.device, dtype=torch.int64)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).contiguous()


def flash_support(cheb_stack, csc_ptr, csc_row, csr_ptr, csr_col, adj_pa):
    """Index data of the fused (flash-style) Chebyshev attention (cheb_flash.hip): csr2csc
    (the CSC position of every CSR entry of the T_k union support), tsupp (K, nnz) = T_k on
    that support in CSC order, the A_pa support as bit rows (apa_bits: row i, bit j) and bit
    columns (apa_bits_t: column j, bit i), and its CSC (apa_ptr, apa_row).  For the
    small-graph kernels (N <= FLASH_SMALL_N) also csc2csr (the inverse of csr2csc), apa_idx
    (N, N): the A_pa-CSC index of (i, j) or -1, and apa2t (apa_nnz): the union-support CSC
    position of every A_pa entry or -1 (empty tensors for larger graphs).  Built on adj_pa's
    device."""
    dev = adj_pa.device
    N = adj_pa.shape[0]
    cp, cr = csc_ptr.to(dev).long(), csc_row.to(dev).long()
    rp, rc = csr_ptr.to(dev).long(), csr_col.to(dev).long()
    ccol = torch.repeat_interleave(torch.arange(N, device=dev), cp[1:] - cp[:-1])
    rrow = torch.repeat_interleave(torch.arange(N, device=dev), rp[1:] - rp[:-1])
    csc_key = ccol * N + cr                      # sorted (column-major order)
    csr2csc = torch.searchsorted(csc_key, rc * N + rrow).to(torch.int32)
    tsupp = cheb_stack.to(dev)[:, cr, ccol].contiguous()
    nz = adj_pa != 0
    apa_ptr, apa_row, _, _ = support_index(nz.unsqueeze(0).cpu())
    apa_ptr, apa_row = apa_ptr.to(dev), apa_row.to(dev)
    out = {"csr2csc": csr2csc, "tsupp": tsupp, "apa_bits": _bits(nz), "apa_bits_t": _bits(nz.t()),
           "apa_ptr": apa_ptr, "apa_row": apa_row}
    empty = torch.zeros(0, dtype=torch.int32, device=dev)
    if N <= FLASH_SMALL_N:
        nnz = cr.numel()
        csc2csr = torch.empty(nnz, dtype=torch.int64, device=dev)
        csc2csr[csr2csc.long()] = torch.arange(nnz, device=dev)
        ap, ar = apa_ptr.long(), apa_row.long()
        acol = torch.repeat_interleave(torch.arange(N, device=dev), ap[1:] - ap[:-1])
        apa_idx = torch.full((N, N), -1, dtype=torch.int32, device=dev)
        apa_idx[ar, acol] = torch.arange(ar.numel(), device=dev, dtype=torch.int32)
        key = acol * N + ar
        pos = torch.searchsorted(csc_key, key).clamp(max=max(nnz - 1, 0))
        hit = (csc_key[pos] == key) if nnz else torch.zeros_like(key, dtype=torch.bool)
        apa2t = torch.where(hit, pos, torch.full_like(pos, -1)).to(torch.int32)
        out.update({"csc2csr": csc2csr.to(torch.int32), "apa_idx": apa_idx.contiguous(), "apa2t": apa2t})
    else:
        out.update({"csc2csr": empty, "apa_idx": empty, "apa2t": empty})
    return out


class cheb_conv(nn.Module):
    """Plain K-order Chebyshev conv (model/DSTAGNN_my.py:135-160).  Never instantiated by
    DSTAGNN; kept for API completeness (parameters only)."""

    def __init__(self, K, cheb_polynomials, in_channels, out_channels):
        super().__init__()
        self.K, self.in_channels, self.out_channels = K, in_channels, out_channels
        self.Theta = nn.ParameterList([nn.Parameter(torch.empty(in_channels, out_channels)) for _ in range(K)])


class Embedding(nn.Module):
    """Positional embedding + LayerNorm (model/DSTAGNN_my.py:162-182); 'T' over N, 'S' over d_model."""

    def __init__(self, nb_seq, d_Em, num_of_features, Etype, DEVICE):
        super().__init__()
        self.nb_seq, self.Etype, self.num_of_features, self.DEVICE = nb_seq, Etype, num_of_features, DEVICE
        self.pos_embed = nn.Embedding(nb_seq, d_Em)
        self.norm = nn.LayerNorm(d_Em)


class GTU(nn.Module):
    """Gated temporal unit (model/DSTAGNN_my.py:184-197): Conv2d(C -> 2C, (1,k)), tanh * sigmoid."""

    def __init__(self, in_channels, time_strides, kernel_size):
        super().__init__()
        self.in_channels = in_channels
        self.con2out = nn.Conv2d(in_channels, 2 * in_channels, kernel_size=(1, kernel_size), stride=(1, time_strides))


def _default_sample_base(B):
    """Global index of this rank's first sample: rank * B under torch.distributed (equal shards,
    as dp.shard_batch / train.DeviceBatches cut them), else 0.  Every rank draws the same dropout
    seed from torch's global RNG (all ranks keep one RNG state: the epoch permutation must be
    identical), and the library keys each keep-mask by (seed, global sample index, position), so
    the shards drop different positions and a data-parallel train step draws exactly the masks
    of the 1-GPU step on the concatenated batch (the reference's 8 replicas see the same batch,
    quirk 15; here they do not)."""
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return torch.distributed.get_rank() * B
    return 0


class DSTAGNN_block(nn.Module):
    """One spatial-temporal block (model/DSTAGNN_my.py:199-253), forward/backward on the HIP path."""

    # a call that records no autograd node (torch.no_grad(), torch.inference_mode(), nothing
    # requiring grad) takes the forward-only library call: no backward state written or
    # allocated, same output bits.  False keeps the full forward there (tools/bench_infer.py A/B)
    forward_only = True

    def __init__(self, DEVICE, num_of_d, in_channels, K, nb_chev_filter, nb_time_filter, time_strides,
                 cheb_polynomials, adj_pa, adj_TMD, num_of_vertices, num_of_timesteps, d_model, d_k, d_v, n_heads,
                 *, multi_feature=False):
        """multi_feature=True: this is a FIRST block over x (B, N, F, T) with F = in_channels = num_of_d
        input features, 1 <= F <= 8 — the reference's block with its three `num_of_features == 1`
        branches keyed on "first block": EmbedT over the F features (one position row per t),
        tco = ReLU(tc), the residual through residual_conv (F -> C).  Every parameter is used."""
        super().__init__()
        self.multi_feature = bool(multi_feature)
        self.in_channels = in_channels
        if self.multi_feature:
            _check_first_f(in_channels)
            if num_of_d != in_channels:
                raise ValueError(f"multi_feature: num_of_d ({num_of_d}) must equal in_channels ({in_channels})")
        if time_strides != 1:
            raise ValueError("time_strides must be 1 (train_DSTAGNN_my.py:93 forces it)")
        if nb_chev_filter != nb_time_filter:
            raise ValueError("nb_chev_filter must equal nb_time_filter (GTU consumes the cheb output)")
        self.sigmoid = nn.Sigmoid()
        self.tanh = nn.Tanh()
        self.relu = nn.ReLU(inplace=True)
        apa = adj_pa.detach().cpu().float() if torch.is_tensor(adj_pa) else torch.as_tensor(np.asarray(adj_pa), dtype=torch.float32)
        self.register_buffer("adj_pa", apa.contiguous(), persistent=False)
        self.pre_conv = nn.Conv2d(num_of_timesteps, d_model, kernel_size=(1, num_of_d))
        self.EmbedT = Embedding(num_of_timesteps, num_of_vertices, num_of_d, "T", DEVICE)
        self.EmbedS = Embedding(num_of_vertices, d_model, num_of_d, "S", DEVICE)
        self.TAt = MultiHeadAttention(DEVICE, num_of_vertices, d_k, d_v, n_heads, num_of_d)
        self.SAt = SMultiHeadAttention(DEVICE, d_model, d_k, d_v, K)
        self.cheb_conv_SAt = cheb_conv_withSAt(K, cheb_polynomials, in_channels, nb_chev_filter, num_of_vertices,
                                               DEVICE)
        self.gtu3 = GTU(nb_time_filter, time_strides, 3)
        self.gtu5 = GTU(nb_time_filter, time_strides, 5)
        self.gtu7 = GTU(nb_time_filter, time_strides, 7)
        self.pooling = nn.MaxPool2d(kernel_size=(1, 2), stride=None, padding=0)  # unused, as in the reference
        self.residual_conv = nn.Conv2d(in_channels, nb_time_filter, kernel_size=(1, 1), stride=(1, time_strides))
        self.dropout = nn.Dropout(p=0.05)
        self.fcmy = nn.Sequential(nn.Linear(3 * num_of_timesteps - 12, num_of_timesteps), nn.Dropout(0.05))
        self.ln = nn.LayerNorm(nb_time_filter)
        self.meta = dict(n_heads=n_heads, d_k=d_k, d_v=d_v, d_model=d_model, K=K, C=nb_chev_filter, drop_p=0.05)
        self.num_of_d = num_of_d
        self.nb_time_filter = nb_time_filter
        self.sparse_cheb = True  # use the CSC/CSR support path when the support is sparse
        # fused (flash-style) Chebyshev attention: None = automatic (sparse path, d_k == 32),
        # True / False force it (block_fn.use_flash)
        self.flash_cheb = None
        self.direct_grads = False  # see set_direct_grads
        self.grads_ready = None    # DP hook: called with the block once its gradients are final
        # global index of x[0] for the dropout masks (None: rank * B under torch.distributed,
        # else 0; set it for unequal shards, see set_sample_base)
        self.sample_base = None

    def forward(self, x, res_att):
        B, N, Fd, T = x.shape
        if self.multi_feature:
            _check_first_f(Fd)
            if Fd != self.in_channels:
                raise RuntimeError(f"multi_feature: x has {Fd} features, the block was built for in_channels = "
                                   f"{self.in_channels}")
        elif Fd != 1 and Fd != self.nb_time_filter:
            # reference: RuntimeError at model/DSTAGNN_my.py:252 (quirk 8)
            raise RuntimeError(f"The size of tensor a ({Fd}) must match the size of tensor b "
                               f"({self.nb_time_filter}) at non-singleton dimension 1")
        if x.device.type != "cuda":
            raise RuntimeError(HIP_ONLY)
        meta = dict(self.meta)
        meta["train"] = bool(self.training)
        meta["direct_grads"] = self.direct_grads
        # a fresh dropout seed per training forward, drawn from torch's global RNG (no draw
        # when dropout is off: like F.dropout(p=0), which consumes no random numbers)
        drop = self.training and meta.get("drop_p", 0.0) > 0.0
        meta["seed"] = int(torch.randint(0, 2 ** 62, (1,)).item()) if drop else 0
        base = (self.sample_base if self.sample_base is not None else _default_sample_base(B)) if drop else 0
        names, params, slots = self._param_list()
        graph = self._graph()
        if use_flash(graph, meta, T, self.flash_cheb, B):
            graph = self._flash_graph(graph)
        out, re_at = block_call(x, res_att, params, slots, graph, meta, meta["train"], meta["seed"],
                                self.direct_grads, flash=self.flash_cheb, plan_cache=self.__dict__.setdefault("_pcache", {}),
                                sample_base=base, forward_only=self.forward_only, first_multi=self.multi_feature)
        if self.grads_ready is not None and out.requires_grad:
            # DP overlap (dp.GradAllReducer.attach): once this block's backward node has run,
            # its parameter gradients are final — hand them over from a post-hook on the node
            out.grad_fn.register_hook(self._post_backward)
        return out, re_at

    def _post_backward(self, grad_inputs, grad_outputs):
        self.grads_ready(self)

    # the host-side caches hold library objects (a torch.classes BlockPlan has no pickler) and
    # Parameter identities: rebuilt on demand, never pickled (torch.save(model) / deepcopy)
    _CACHES = ("_pcache", "_plist", "_gcache")

    def __getstate__(self):
        state = self.__dict__.copy()
        for k in self._CACHES:
            state.pop(k, None)
        return state

    # host-side caches (the launch path is host-bound at these sizes): the parameter list
    # (Parameter objects survive .to()/.cuda()) and the graph dict (rebuilt when a buffer
    # is replaced, e.g. by .to())
    def _param_list(self):
        c = self.__dict__.get("_plist")
        # valid while every (submodule, attribute) still holds the same Parameter object
        # (in-place updates such as load_state_dict keep them; re-assignment does not)
        if c is None or any(mod._parameters.get(attr) is not prm for mod, attr, prm in c[2]):
            names, params = zip(*self.named_parameters())
            slots = []
            for n in names:
                mod_name, _, attr = n.rpartition(".")
                mod = self.get_submodule(mod_name) if mod_name else self
                slots.append((mod, attr, mod._parameters[attr]))
            c = (tuple(names), tuple(params), tuple(slots), slots_of(names))
            self.__dict__["_plist"] = c
        return c[0], c[1], c[3]

    def _graph(self):
        cc = self.cheb_conv_SAt
        key = (id(cc.cheb_stack), id(self.adj_pa), id(cc.csc_row), bool(self.sparse_cheb))
        c = self.__dict__.get("_gcache")
        if c is None or c[0] != key:
            graph = cc.graph(self.adj_pa)
            if not self.sparse_cheb:
                graph = {"cheb": graph["cheb"], "adj_pa": graph["adj_pa"]}
            c = (key, graph)
            self.__dict__["_gcache"] = c
        return c[1]

    def _flash_graph(self, graph):
        """graph + the flash-attention index data (built once per graph, on its device)."""
        if "csr2csc" not in graph:
            cc = self.cheb_conv_SAt
            graph.update(flash_support(cc.cheb_stack, graph["csc_ptr"], graph["csc_row"], graph["csr_ptr"],
                                       graph["csr_col"], graph["adj_pa"]))
        return graph


class DSTAGNN_submodule(nn.Module):
    """Stack of blocks + final_conv / final_fc (model/DSTAGNN_my.py:255-280)."""

    def __init__(self, DEVICE, num_of_d, nb_block, in_channels, K, nb_chev_filter, nb_time_filter, time_strides,
                 cheb_polynomials, adj_pa, adj_TMD, num_for_predict, len_input, num_of_vertices, d_model, d_k, d_v,
                 n_heads, *, multi_feature=False, quantiles=None):
        """multi_feature=True: block 0 is a multi-feature first block over the F = in_channels input
        features; the inner blocks are built for the C features block 0 hands them (pre_conv
        (D, T, 1, C), where the reference's num_of_d * nb_time_filter is wrong for F > 1), and they
        receive block 0's re_At averaged over its F features, (B, 1, h, T, T), in the broadcast form.
        With F = 1 this is the default model, bit for bit.
        quantiles=(tau_0 < ... < tau_{Q-1}) (loss.check_quantiles: 1 to 16 levels strictly inside
        (0, 1)): a quantile head.  final_fc is Linear(128, num_for_predict * Q) with row p Q + q, forward
        returns (B, N, num_for_predict, Q), and the module carries the persistent fp32 buffer
        ``quantile_levels`` (Q,), ``quantiles`` and ``point_index`` (the column nearest 0.5).  None: the
        point model, with no buffer, the same keys and the same init draws as ever."""
        super().__init__()
        self.multi_feature = bool(multi_feature)
        self.quantiles = self.point_index = None
        self.num_for_predict = num_for_predict
        if quantiles is not None:
            from .loss import check_quantiles, point_index_of
            self.quantiles = check_quantiles(quantiles, "quantiles")
            self.point_index = point_index_of(self.quantiles)
        inner_d = nb_time_filter if self.multi_feature else num_of_d * nb_time_filter
        self.BlockList = nn.ModuleList([DSTAGNN_block(DEVICE, num_of_d, in_channels, K, nb_chev_filter,
                                                      nb_time_filter, time_strides, cheb_polynomials, adj_pa,
                                                      adj_TMD, num_of_vertices, len_input, d_model, d_k, d_v,
                                                      n_heads, multi_feature=self.multi_feature)])
        self.BlockList.extend([DSTAGNN_block(DEVICE, inner_d, nb_chev_filter, K, nb_chev_filter,
                                             nb_time_filter, 1, cheb_polynomials, adj_pa, adj_TMD, num_of_vertices,
                                             len_input // time_strides, d_model, d_k, d_v, n_heads)
                               for _ in range(nb_block - 1)])
        self.final_conv = nn.Conv2d(int((len_input / time_strides) * nb_block), 128, kernel_size=(1, nb_time_filter))
        self.final_fc = nn.Linear(128, num_for_predict * (1 if self.quantiles is None else len(self.quantiles)))
        if self.quantiles is not None:
            self.register_buffer("quantile_levels", torch.tensor(self.quantiles, dtype=torch.float32))
        self.DEVICE = DEVICE
        self.to(DEVICE)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # a checkpoint trained for other levels has the right shapes and the wrong meaning
        theirs = state_dict.get(prefix + "quantile_levels")
        if self.quantiles is not None and theirs is not None:
            mine = self.quantile_levels.detach().cpu()
            if tuple(theirs.shape) != tuple(mine.shape) or not torch.equal(theirs.detach().cpu().float(), mine):
                def show(t):
                    return "(" + ", ".join(f"{float(v):.6g}" for v in t.flatten()) + ")"
                raise ValueError(f"the checkpoint's quantile_levels {show(theirs)} differ from the model's "
                                 f"{show(mine)}")
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, x):
        need_concat = []
        res_att = 0
        for i, block in enumerate(self.BlockList):
            x, res_att = block(x, res_att)
            if self.multi_feature and i == 0 and res_att.shape[1] > 1:
                # the hand-off: the mean over block 0's F features (the identity at F = 1, and a
                # score scale that does not grow with F)
                res_att = res_att.mean(dim=1, keepdim=True)
            need_concat.append(x)
        # cat -> final_conv -> [..., -1] -> final_fc as one HIP head op (head.hip): the
        # concatenation is never materialised (model/DSTAGNN_my.py:276-280)
        y = DSTAGNNHeadFunction.apply(self.final_conv.weight, self.final_conv.bias, self.final_fc.weight,
                                      self.final_fc.bias, *need_concat)
        if self.quantiles is None:
            return y
        return y.view(y.shape[0], y.shape[1], self.num_for_predict, len(self.quantiles))  # row p Q + q


def make_model(DEVICE, num_of_d, nb_block, in_channels, K, nb_chev_filter, nb_time_filter, time_strides, adj_mx,
               adj_pa, adj_TMD, num_for_predict, len_input, num_of_vertices, d_model, d_k, d_v, n_heads,
               *, multi_feature=False, quantiles=None):
    """model/DSTAGNN_my.py:282-297: scaled Laplacian + Chebyshev polynomials, then the
    xavier (dim>1) / U(0,1) (dim<=1, LayerNorm gamma/beta included) initialisation.
    multi_feature=True: a model whose first block takes all F = in_channels = num_of_d input
    features, 1 <= F <= 8 (DSTAGNN_submodule).  quantiles=(...): a quantile head, output
    (B, N, num_for_predict, Q) (DSTAGNN_submodule); the levels are checked before anything is built."""
    if quantiles is not None:
        from .loss import check_quantiles
        quantiles = check_quantiles(quantiles, "quantiles")
    L_tilde = scaled_Laplacian(adj_mx)
    Lt = L_tilde if isinstance(L_tilde, np.ndarray) else L_tilde.cpu().numpy()
    cheb_polynomials = [torch.from_numpy(np.asarray(c)).type(torch.FloatTensor) for c in cheb_polynomial(Lt, K)]
    model = DSTAGNN_submodule(DEVICE, num_of_d, nb_block, in_channels, K, nb_chev_filter, nb_time_filter,
                              time_strides, cheb_polynomials, adj_pa, adj_TMD, num_for_predict, len_input,
                              num_of_vertices, d_model, d_k, d_v, n_heads, multi_feature=multi_feature,
                              quantiles=quantiles)
    for p in model.parameters():
        if p.dim() > 1:
            nn.init.xavier_uniform_(p)
        else:
            nn.init.uniform_(p)
    return model


def set_dropout(model, p):
    """Set the probability of both Dropout sites of every DSTAGNN_block in `model` (the
    reference hard-codes 0.05 at model/DSTAGNN_my.py:218,221; 0 turns them off, e.g. for
    trajectory parity runs)."""
    for m in model.modules():
        if isinstance(m, DSTAGNN_block):
            m.meta["drop_p"] = float(p)
            m.dropout.p = float(p)
            m.fcmy[1].p = float(p)
    return model


def set_sample_base(model, base):
    """Global index of the first sample of `model`'s input batch on this process (dropout masks
    are keyed by it); None restores the default rank * B under torch.distributed."""
    for m in model.modules():
        if isinstance(m, DSTAGNN_block):
            m.sample_base = None if base is None else int(base)
    return model


def set_direct_grads(model, enabled=True):
    """Direct-gradient mode for every DSTAGNN_block in `model`: the block's backward writes
    its parameter gradients into ``param.grad`` (set, or added when a gradient is already
    there) instead of handing them to autograd's per-parameter AccumulateGrad nodes — about
    4 us of host time per parameter per step (36 per block).  ``loss.backward()`` /
    optimiser semantics are unchanged; what it gives up: ``torch.autograd.grad(..., inputs=
    <block parameters>)`` no longer returns those gradients, and post-accumulate-grad hooks on
    them do not fire.  Off by default; the training driver and the benchmark turn it on."""
    for m in model.modules():
        if isinstance(m, DSTAGNN_block):
            m.direct_grads = bool(enabled)
    return model
