"""The graph-convolution stack of the GCN feature extractor (reference: GraphConvolution, layers.py:153-198; the layer
loop of GCN.forward, model.py:409-427) and the graph-attention stack of the GAT one (GraphAttention, layers.py:201-257;
GAT.forward, model.py:453-469), each as one autograd operator over all its layers."""
import torch
import torch.nn.functional as F
from torch.autograd import Function

from .. import _hip as H
from .elementwise import _c, _next_salt

MAX_LAYERS = H.GRAPHCONV_MAX_PAIRS


class EdgeConvFn(Function):
    """A bias-free nn.Conv2d of the edge encoder on the library convolution, with the library's deterministic algorithms
    asked for around the forward and the backward call: its default weight gradient accumulates with atomics (two calls
    differ in the last bits), which would break the run-to-run and eager-to-replay identity the rest of the path keeps."""

    @staticmethod
    def forward(ctx, x, weight, stride, padding, dilation):
        H.need_f32_cuda(x, weight)
        ctx.save_for_backward(x, weight)
        ctx.cfg = (stride, padding, dilation)
        with _deterministic_library():
            return F.conv2d(x, weight, None, stride, padding, dilation)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        stride, padding, dilation = ctx.cfg
        with _deterministic_library():
            dx, dw, _ = torch.ops.aten.convolution_backward(
                gy.contiguous(), x, weight, None, list(stride), list(padding), list(dilation), False, [0, 0], 1,
                [ctx.needs_input_grad[0], ctx.needs_input_grad[1], False])
        return dx, dw, None, None, None


class _deterministic_library:
    def __enter__(self):
        self.was = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True

    def __exit__(self, *exc):
        torch.backends.cudnn.deterministic = self.was


def edge_conv(x, conv):
    """conv(x) for a bias-free nn.Conv2d (groups 1) through EdgeConvFn."""
    if conv.bias is not None or conv.groups != 1 or conv.padding_mode != "zeros" or isinstance(conv.padding, str):
        raise NotImplementedError("edge_conv: a bias-free, ungrouped, zero-padded nn.Conv2d")
    return EdgeConvFn.apply(x, conv.weight, tuple(conv.stride), tuple(conv.padding), tuple(conv.dilation))


class GraphConvStackFn(Function):
    """h_0 = x;  s_l = h_l W_l;  h_{l+1}[b,i,c] = act_l(sum_j E[b,c,i,j] s_l[b,j,c] + bias_l[c])  for l < L.

    E is given as its channel groups (dense [B, c_g, n, n] tensors, sum c_g = C) and is never concatenated.  Forward, per
    layer: the support product on gt_gemm, then gt_graphconv_fwd with the bias and the ReLU on its store.  Backward, from
    the last layer down: the ReLU gate from the saved output, the bias gradient as the column sums of the gated gradient,
    the support's gradient by gt_graphconv_bwd_data, dW_l = h_l^T dS_l and dh_l = dS_l W_l^T on gt_gemm; the layers'
    (gradient, support) pairs are kept and ONE gt_graphconv_bwd_edge at the end writes the gradient of every group that
    needs one -- a rank-L update written once instead of L passes over an [B, C, n, n] tensor and L - 1 adds."""

    @staticmethod
    def forward(ctx, x, n_groups: int, relu, *tensors):
        L = len(relu)
        edges, weights, biases = tensors[:n_groups], tensors[n_groups:n_groups + L], tensors[n_groups + L:]
        H.need_f32_cuda(x, *tensors)
        B, n, K0 = x.shape
        Cc = weights[0].shape[1]
        T = B * n
        edges = tuple(_c(e) for e in edges)
        ws = tuple(_c(w) for w in weights)
        h = _c(x).reshape(T, K0)
        hs, Ss = [h], []
        for l in range(L):
            K = ws[l].shape[0]
            S = torch.empty(T, Cc, dtype=torch.float32, device=x.device)
            H.gemm(h, ws[l], S, T, Cc, K, layout_b=1, lda=K, ldb=Cc, ldc=Cc)
            h = H.graphconv_fwd(edges, S, biases[l], B, n, Cc, H.ACT_RELU if relu[l] else H.ACT_NONE).reshape(T, Cc)
            Ss.append(S)
            hs.append(h)
        ctx.save_for_backward(*edges, *ws, *hs, *Ss)
        ctx.cfg = (n_groups, tuple(relu), B, n, Cc, tuple(b is not None for b in biases))
        return h.reshape(B, n, Cc)

    @staticmethod
    def backward(ctx, gy):
        n_groups, relu, B, n, Cc, has_bias = ctx.cfg
        L = len(relu)
        sv = ctx.saved_tensors
        edges, ws = sv[:n_groups], sv[n_groups:n_groups + L]
        hs, Ss = sv[n_groups + L:n_groups + 2 * L + 1], sv[n_groups + 2 * L + 1:]
        need = ctx.needs_input_grad
        need_e, need_w, need_b = need[3:3 + n_groups], need[3 + n_groups:3 + n_groups + L], need[3 + n_groups + L:]
        dev, T = gy.device, B * n
        G = _c(gy).reshape(T, Cc)
        Gs, dws, dbs, dx = [None] * L, [None] * L, [None] * L, None
        for l in range(L - 1, -1, -1):
            if relu[l]:
                G = H.act_bwd(G, hs[l + 1], H.ACT_RELU)
            Gs[l] = G
            if has_bias[l] and need_b[l]:
                dbs[l] = H.colsum(G, T, Cc, Cc)
            want_dh = l > 0 or need[0]
            if not (want_dh or need_w[l]):
                continue
            K = ws[l].shape[0]
            dS = H.graphconv_bwd_data(edges, G, B, n, Cc).reshape(T, Cc)
            if need_w[l]:
                dws[l] = torch.empty(K, Cc, dtype=torch.float32, device=dev)
                H.gemm(hs[l], dS, dws[l], K, Cc, T, layout_a=1, layout_b=1, lda=K, ldb=Cc, ldc=Cc, split_k=0)
            if want_dh:
                G = torch.empty(T, K, dtype=torch.float32, device=dev)
                H.gemm(dS, ws[l], G, T, K, Cc, lda=Cc, ldb=Cc, ldc=K)
                if l == 0:
                    dx = G.reshape(B, n, K)
        des = [None] * n_groups
        if any(need_e):
            des = [torch.empty_like(e) if w else None for e, w in zip(edges, need_e)]
            H.graphconv_bwd_edge([(None, e.shape[1]) if d is None else d for e, d in zip(edges, des)], Gs, Ss, B, n, Cc)
        return (dx, None, None, *des, *dws, *dbs)


def graph_conv_stack(x, edges, weights, biases, relu):
    """x [B, n, in] -> [B, n, C] through len(weights) graph-convolution layers that share the edge tensor.

    edges: one tensor [B, C, n, n] or a sequence of 1..3 channel groups [B, c_g, n, n]; weights[l]: [in_l, C] (in_0 = in,
    then C); biases[l]: [C] or None; relu[l]: a ReLU behind layer l."""
    if isinstance(edges, torch.Tensor):
        edges = (edges,)
    edges, weights, biases, relu = tuple(edges), tuple(weights), tuple(biases), tuple(bool(r) for r in relu)
    L = len(weights)
    if L < 1 or len(biases) != L or len(relu) != L:
        raise ValueError("graph_conv_stack: one weight, bias (or None) and ReLU flag per layer")
    if L > MAX_LAYERS:
        raise NotImplementedError(f"graph_conv_stack: {L} layers; gt_graphconv_bwd_edge takes at most {MAX_LAYERS} "
                                  f"(gradient, support) pairs")
    if not 1 <= len(edges) <= 3:
        raise ValueError("graph_conv_stack: 1..3 edge channel groups")
    H.need_f32_cuda(x, *edges, *weights, *biases)
    if x.dim() != 3:
        raise ValueError(f"graph_conv_stack: x is {tuple(x.shape)}, wanted [B, n, in]")
    B, n, K0 = x.shape
    Cc = weights[0].shape[1]
    if n > H.GRAPHCONV_MAX_N:
        raise H.GtNotSupported(f"graph_conv_stack: n = {n} > {H.GRAPHCONV_MAX_N}")
    if sum(e.shape[1] for e in edges) != Cc or any(e.dim() != 4 or e.shape[0] != B or tuple(e.shape[2:]) != (n, n)
                                                   for e in edges):
        raise ValueError(f"graph_conv_stack: edge groups {[tuple(e.shape) for e in edges]} against x {tuple(x.shape)}, "
                         f"C = {Cc}")
    for l, w in enumerate(weights):
        if tuple(w.shape) != ((K0 if l == 0 else Cc), Cc) or (biases[l] is not None and tuple(biases[l].shape) != (Cc,)):
            raise ValueError(f"graph_conv_stack: layer {l} weight {tuple(w.shape)}")
    return GraphConvStackFn.apply(x, len(edges), relu, *edges, *weights, *biases)


class GraphAttentionStackFn(Function):
    """x_0 = x;  h_l = x_l W_l;  s_l = h_l a_l[:F];  t_l = h_l a_l[F:];
    P_l = softmax_j(LeakyReLU(s_i + t_j) where keep_ij, else -9e15);  U_l = dropout(P_l) h_l;  x_{l+1} = relu_l?(ELU?(U_l)).

    The keep bits of adj are packed once (gt_graphattn_mask) and shared by all layers and both directions; no pass forms an
    n x n float tensor.  Forward, per layer: h on gt_gemm, (s, t) as one [T, 2] product on gt_gemm, gt_graphattn_fwd.  The two
    thin products around `a` run in the f32 arithmetic whatever the precision mode: the scores feed an exponential, and
    da = [ds dt]^T h sums a gradient that cancels row by row (sum_j P_ij (dP_ij - D_i) = 0).  Saved
    per layer: x_l, h_l, (s, t)_l, U_l and the row statistics L_l; the dropout mask is regenerated from (seed, salt).
    Backward, from the last layer down: gt_graphattn_bwd_row (dU, ds, the partial sums of dt), gt_graphattn_bwd_col (dt and
    dH with ds a1^T + dt a2^T added), then da = [ds dt]^T h, dW = x^T dH and dx = dH W^T on gt_gemm.  adj gets no gradient."""

    @staticmethod
    def forward(ctx, x, adj, relu, cfg, *tensors):
        L = len(relu)
        alpha, concat, graph_lap, thresh, p = cfg
        H.need_f32_cuda(x, adj, *tensors)
        B, n, K0 = x.shape
        Fd = tensors[0].shape[1]
        T = B * n
        ws = tuple(_c(w) for w in tensors[:L])
        avs = tuple(_c(a).reshape(2, Fd) for a in tensors[L:])
        dev = x.device
        save = any(ctx.needs_input_grad)
        bits, bitsT, w0 = H.graphattn_mask(adj, graph_lap, thresh)      # (dense, or a channel of an edge tensor in place)
        salts = tuple(_next_salt(1) if p > 0 else 0 for _ in range(L))
        xin = _c(x).reshape(T, K0)
        kept = []
        for l in range(L):
            K = ws[l].shape[0]
            h = torch.empty(T, Fd, dtype=torch.float32, device=dev)
            H.gemm(xin, ws[l], h, T, Fd, K, layout_b=1, lda=K, ldb=Fd, ldc=Fd)
            st = torch.empty(T, 2, dtype=torch.float32, device=dev)
            H.gemm(h, avs[l], st, T, 2, Fd, lda=Fd, ldb=Fd, ldc=2, precision="f32")
            U = torch.empty(T, Fd, dtype=torch.float32, device=dev) if save else None
            out = torch.empty(T, Fd, dtype=torch.float32, device=dev)
            Lg = torch.empty(B, n, dtype=torch.float32, device=dev)
            H.graphattn_fwd(bits, w0, st, st[:, 1], 2, h, U, out, Lg, B, n, Fd, alpha, concat, relu[l],
                            H.dropout_desc(p, salts[l], dev))
            if save:
                kept += [xin, h, st, U, Lg]
            xin = out
        if save:
            ctx.save_for_backward(bits, bitsT, w0, *ws, *avs, *kept)
        ctx.cfg = (tuple(relu), alpha, concat, p, salts, B, n, Fd)
        return xin.reshape(B, n, Fd)

    @staticmethod
    def backward(ctx, gy):
        relu, alpha, concat, p, salts, B, n, Fd = ctx.cfg
        L = len(relu)
        sv = ctx.saved_tensors
        bits, bitsT, w0 = sv[:3]
        ws, avs, kept = sv[3:3 + L], sv[3 + L:3 + 2 * L], sv[3 + 2 * L:]
        need = ctx.needs_input_grad
        need_w, need_a = need[4:4 + L], need[4 + L:]
        dev, T = gy.device, B * n
        G = _c(gy).reshape(T, Fd)
        dws, das, dx = [None] * L, [None] * L, None
        for l in range(L - 1, -1, -1):
            xin, h, st, U, Lg = kept[5 * l:5 * l + 5]
            drop = H.dropout_desc(p, salts[l], dev)
            dU = torch.empty(T, Fd, dtype=torch.float32, device=dev)
            dst = torch.empty(T, 2, dtype=torch.float32, device=dev)
            dtp = torch.empty(B, H.graphattn_words(n), n, dtype=torch.float32, device=dev)
            H.graphattn_bwd_row(bits, st, st[:, 1], 2, Lg, G, U, h, dU, dst, dtp, B, n, Fd, alpha, concat, relu[l], drop)
            dH = torch.empty(T, Fd, dtype=torch.float32, device=dev)
            H.graphattn_bwd_col(bitsT, w0, st, st[:, 1], 2, Lg, dU, avs[l], dst, dtp, dst[:, 1], dH, B, n, Fd, alpha, drop)
            K = ws[l].shape[0]
            if need_a[l]:
                da = torch.empty(2, Fd, dtype=torch.float32, device=dev)
                H.gemm(dst, h, da, 2, Fd, T, layout_a=1, layout_b=1, lda=2, ldb=Fd, ldc=Fd, split_k=0, precision="f32")
                das[l] = da.reshape(2 * Fd, 1)
            if need_w[l]:
                dws[l] = torch.empty(K, Fd, dtype=torch.float32, device=dev)
                H.gemm(xin, dH, dws[l], K, Fd, T, layout_a=1, layout_b=1, lda=K, ldb=Fd, ldc=Fd, split_k=0)
            if l > 0 or need[0]:
                G = torch.empty(T, K, dtype=torch.float32, device=dev)
                H.gemm(dH, ws[l], G, T, K, Fd, lda=Fd, ldb=Fd, ldc=K)
                if l == 0:
                    dx = G.reshape(B, n, K)
        return (dx, None, None, None, *dws, *das)


def graph_attention_stack(x, adj, Ws, as_, relu, *, alpha=1e-2, concat=True, graph_lap=True, thresh=1e-6, p=0.0):
    """x [B, n, in] -> [B, n, F] through len(Ws) graph-attention layers that share adj [B, n, n].

    Ws[l]: [in_l, F] (in_0 = in, then F); as_[l]: [2F, 1]; relu[l]: a ReLU behind layer l's ELU; concat: the ELU itself;
    graph_lap / thresh: keep |adj| > thresh, else adj > 0; p: the dropout of the attention weights (0: none)."""
    Ws, as_, relu = tuple(Ws), tuple(as_), tuple(bool(r) for r in relu)
    L = len(Ws)
    if L < 1 or len(as_) != L or len(relu) != L:
        raise ValueError("graph_attention_stack: one W, one a and one ReLU flag per layer")
    if x.dim() != 3 or adj.dim() != 3:
        raise ValueError(f"graph_attention_stack: x is {tuple(x.shape)}, adj {tuple(adj.shape)}; wanted [B, n, in], [B, n, n]")
    B, n, K0 = x.shape
    Fd = Ws[0].shape[1]
    if tuple(adj.shape) != (B, n, n) or B < 1 or n < 1:
        raise ValueError(f"graph_attention_stack: adj {tuple(adj.shape)} against x {tuple(x.shape)}")
    for l, (w, a) in enumerate(zip(Ws, as_)):
        if tuple(w.shape) != ((K0 if l == 0 else Fd), Fd) or tuple(a.shape) != (2 * Fd, 1):
            raise ValueError(f"graph_attention_stack: layer {l} W {tuple(w.shape)}, a {tuple(a.shape)}")
    if not 0.0 <= p < 1.0:
        raise ValueError(f"graph_attention_stack: dropout p = {p}")
    if Fd % 4 or Fd > H.GRAPHATTN_MAX_F:
        raise H.GtNotSupported(f"graph_attention_stack: F = {Fd}; the gt_graphattn_* kernels take F % 4 == 0, F <= "
                               f"{H.GRAPHATTN_MAX_F}")
    if n > H.GRAPHATTN_MAX_N:
        raise H.GtNotSupported(f"graph_attention_stack: n = {n} > {H.GRAPHATTN_MAX_N}")
    if alpha < 0:
        raise H.GtNotSupported("graph_attention_stack: a negative LeakyReLU slope")
    H.need_f32_cuda(x, adj, *Ws, *as_)
    return GraphAttentionStackFn.apply(x, adj, relu, (float(alpha), bool(concat), bool(graph_lap), float(thresh), float(p)),
                                       *Ws, *as_)
