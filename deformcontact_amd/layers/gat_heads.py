"""Multi-head GATConv, without and with edge features (they share the backward)."""
from __future__ import annotations

import torch

from .. import _lib
from .._host import _grad_layout, _ptr, _rowmajor
from ..deferred import resolve
from ..graph import GraphIndex, SortedAdjacency, _require_cuda, current_stream_ptr
from .gnn import _ParamGrads, _mask_and_bias_grad, fused_gnn_ok


# --------------------------------------------------------------------------- #
# GATConv with several heads (dc_gat_heads.hip): h is [N, H*C], per-node vectors [N, H], per-edge vectors
# [capacity, H] edge-major in g.fwd order.  One launcher per C entry.
# --------------------------------------------------------------------------- #
def _heads_alpha_fwd(h, a_s, a_d, nh: int, c: int):
    """(a_src, a_dst) [N, H]: both attention dot products of every head in one pass over ``h``."""
    n, dev = h.size(0), h.device
    a_src = torch.empty((n, nh), dtype=torch.float32, device=dev)
    a_dst = torch.empty((n, nh), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dc_gat_alpha_heads_fwd(h.data_ptr(), _rowmajor(h, "h"), a_s.data_ptr(), a_d.data_ptr(),
                                                 a_src.data_ptr(), a_dst.data_ptr(), n, nh, c, current_stream_ptr(dev)),
               "dc_gat_alpha_heads_fwd")
    return a_src, a_dst


def _heads_edge_vector(g: GraphIndex, nh: int, dev) -> torch.Tensor:
    return torch.zeros((max(g.capacity, 1), nh), dtype=torch.float32, device=dev)


def _heads_softmax_fwd(g: GraphIndex, a_src, a_dst, slope: float, n: int, nh: int) -> torch.Tensor:
    alpha = _heads_edge_vector(g, nh, a_src.device)
    _lib.check(_lib.lib().dc_gat_edge_softmax_heads_fwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), a_src.data_ptr(),
                                                        a_dst.data_ptr(), slope, alpha.data_ptr(), n, nh,
                                                        current_stream_ptr(a_src.device)), "dc_gat_edge_softmax_heads_fwd")
    return alpha


def _heads_agg(adj: SortedAdjacency, alpha, x, bias, relu: bool, mean: bool, nh: int, c: int) -> torch.Tensor:
    """``act(sum_p alpha[p, head] x[other[p]] + bias)`` at width H*C, or its mean over heads at width C."""
    n, dev = x.size(0), x.device
    y = torch.empty((n, c if mean else nh * c), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dc_spmm_f32_heads_bias_act(adj.ptr.data_ptr(), adj.other.data_ptr(), alpha.data_ptr(),
                                                     x.data_ptr(), _rowmajor(x, "x"), _ptr(bias), int(relu), int(mean),
                                                     y.data_ptr(), y.size(1), n, nh, c, current_stream_ptr(dev)),
               "dc_spmm_f32_heads_bias_act")
    return y


def _heads_sddmm(g: GraphIndex, gm, h, nh: int, c: int) -> torch.Tensor:
    galpha = _heads_edge_vector(g, nh, h.device)
    _lib.check(_lib.lib().dc_sddmm_f32_heads(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), gm.data_ptr(),
                                             _rowmajor(gm, "gm"), h.data_ptr(), _rowmajor(h, "h"), galpha.data_ptr(),
                                             h.size(0), nh, c, current_stream_ptr(h.device)), "dc_sddmm_f32_heads")
    return galpha


def _heads_softmax_bwd(g: GraphIndex, a_src, a_dst, slope: float, alpha, galpha, n: int, nh: int):
    dev = alpha.device
    ge = _heads_edge_vector(g, nh, dev)
    g_a_dst = torch.empty((n, nh), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dc_gat_edge_softmax_heads_bwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), a_src.data_ptr(),
                                                        a_dst.data_ptr(), slope, alpha.data_ptr(), galpha.data_ptr(),
                                                        ge.data_ptr(), g_a_dst.data_ptr(), n, nh,
                                                        current_stream_ptr(dev)), "dc_gat_edge_softmax_heads_bwd")
    return ge, g_a_dst


def _heads_segment_sum(ptr, index_map, v, n: int, w: int) -> torch.Tensor:
    out = torch.empty((n, w), dtype=torch.float32, device=v.device)
    _lib.check(_lib.lib().dc_segment_sum_f32_heads(ptr.data_ptr(), _ptr(index_map), v.data_ptr(), out.data_ptr(), n, w,
                                                   current_stream_ptr(v.device)), "dc_segment_sum_f32_heads")
    return out


def _heads_gather(g: GraphIndex, v, idx, w: int) -> torch.Tensor:
    """``out[p, :] = v[idx[p], :]`` for the edges the adjacency holds (counted on the device, ``g.fwd.ptr[-1]``)."""
    out = _heads_edge_vector(g, w, v.device)
    _lib.check(_lib.lib().dc_gather_f32_heads(v.data_ptr(), idx.data_ptr(), out.data_ptr(), g.fwd.ptr[-1:].data_ptr(),
                                              g.capacity, w, current_stream_ptr(v.device)), "dc_gather_f32_heads")
    return out


def _heads_spread(gm, nh: int, c: int) -> torch.Tensor:
    """The gradient of the mean over heads: ``out[i, k*C + c] = gm[i, c] / H``."""
    n, dev = gm.size(0), gm.device
    out = torch.empty((n, nh * c), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dc_spread_heads_f32(gm.data_ptr(), _rowmajor(gm, "gm"), out.data_ptr(), nh * c, n, nh, c,
                                              current_stream_ptr(dev)), "dc_spread_heads_f32")
    return out


def _heads_out_grad(ctx, gy, y, bias):
    """How the multi-head backward passes open: ``gy`` in a layout the kernels take, the ReLU mask and the bias
    gradient in one pass (``bias`` is input 4 of every one of them), and - the heads averaged - the gradient spread to
    the heads.  -> (gm [N, H*C], gb)."""
    gy = _grad_layout(gy, 0)
    gm, gb = _mask_and_bias_grad(gy, y, bias, bias is not None and ctx.needs_input_grad[4])
    if ctx.mean:
        gm = _heads_spread(gm, ctx.nh, ctx.c)
    return gm, gb


def _heads_alpha_bwd(h, g_a_src, g_a_dst, a_s, a_d, gh, nh: int, c: int, gs, gd, accumulate: bool) -> None:
    n, f, dev = h.size(0), nh * c, h.device
    L = _lib.lib()
    ws = torch.empty(max(L.dc_colsum_workspace_bytes(n, f, 2), 16), dtype=torch.uint8, device=dev)
    _lib.check(L.dc_gat_alpha_heads_bwd(h.data_ptr(), f, g_a_src.data_ptr(), g_a_dst.data_ptr(), a_s.data_ptr(),
                                        a_d.data_ptr(), gh.data_ptr(), f, n, nh, c, ws.data_ptr(), ws.numel(),
                                        gs.data_ptr(), gd.data_ptr(), int(accumulate), current_stream_ptr(dev)),
               "dc_gat_alpha_heads_bwd")


def _gat_heads_edge_backward(g: GraphIndex, gm, h, a_src, a_dst, alpha, slope: float, nh: int, c: int, a_edge=None):
    """``_gat_edge_backward`` for H heads, from the gradient ``gm`` [N, H*C] of the concatenated aggregation:
    -> (gh [N, H*C], g_a_src [N, H], g_a_dst [N, H], ge [capacity, H]); ``a_edge``: the logits' per-edge addend."""
    n = h.size(0)
    b2f = g.bwd_to_fwd()
    # d out / d h : transposed aggregation with alpha re-ordered by source, H floats per edge
    gh = _heads_agg(g.bwd, _heads_gather(g, alpha, b2f, nh), gm, None, False, False, nh, c)
    # d out / d alpha, through the softmax, summed per source
    galpha = _heads_sddmm(g, gm, h, nh, c)
    if a_edge is None:
        ge, g_a_dst = _heads_softmax_bwd(g, a_src, a_dst, slope, alpha, galpha, n, nh)
    else:
        ge, g_a_dst = _edge_softmax_bwd(g, a_src, a_dst, a_edge, slope, alpha, galpha, n, nh)
    return gh, _heads_segment_sum(g.bwd.ptr, b2f, ge, n, nh), g_a_dst, ge


class _GatHeadsAggregateFn(torch.autograd.Function):
    """The unfused multi-head aggregation (edge softmax + weighted sum per head, concatenated or averaged over the
    heads): the sibling of ``_GatAggregateFn``; ``_GatHeadsConvFn`` is the whole layer."""

    @staticmethod
    def forward(ctx, g: GraphIndex, h, a_src, a_dst, slope: float, nh: int, mean: bool):
        h, a_src, a_dst = h.contiguous(), a_src.contiguous(), a_dst.contiguous()
        c = h.size(1) // nh
        alpha = _heads_softmax_fwd(g, a_src, a_dst, slope, h.size(0), nh)
        out = _heads_agg(g.fwd, alpha, h, None, False, mean, nh, c)
        ctx.g, ctx.slope, ctx.nh, ctx.c, ctx.mean = g, slope, nh, c, mean
        ctx.save_for_backward(h, a_src, a_dst, alpha)
        return out

    @staticmethod
    def backward(ctx, gout):
        h, a_src, a_dst, alpha = ctx.saved_tensors
        gm = _grad_layout(gout, 0)
        if ctx.mean:
            gm = _heads_spread(gm, ctx.nh, ctx.c)
        gh, g_a_src, g_a_dst, _ = _gat_heads_edge_backward(ctx.g, gm, h, a_src, a_dst, alpha, ctx.slope, ctx.nh, ctx.c)
        return None, gh, g_a_src, g_a_dst, None, None, None


def gat_heads_aggregate(g: GraphIndex, h, a_src, a_dst, slope: float, heads: int, mean: bool = False,
                        edge_attr=None, edge_m=None, fill_value="mean") -> torch.Tensor:
    """``h`` [N, H*C], ``a_src`` / ``a_dst`` [N, H] -> [N, H*C], or [N, C] with ``mean`` (PyG ``concat=False``).
    ``edge_attr`` [E, D] with the folded ``edge_m`` [D, H] (``gat_edge_fold``): the logits' edge-feature term."""
    h = resolve(h)
    if h.dim() != 2 or heads < 1 or h.size(1) % heads or a_src.shape != (h.size(0), heads) or a_dst.shape != a_src.shape:
        raise ValueError("gat_heads_aggregate: h must be [N, H*C] and a_src / a_dst [N, H]")
    if edge_attr is None:
        return _GatHeadsAggregateFn.apply(g, h, a_src, a_dst, float(slope), int(heads), bool(mean))
    edge_attr, fill_mean, fill = _edge_operands(g, edge_attr, edge_m, int(heads), fill_value)
    return _GatHeadsEdgeAggregateFn.apply(g, h, a_src, a_dst, float(slope), int(heads), bool(mean), edge_attr, edge_m,
                                          fill_mean, fill)


def gat_heads_fused_ok(h: torch.Tensor, heads: int, mean: bool) -> bool:
    """Widths the row-wise passes of ``gat_heads_conv`` take: ``fused_gnn_ok`` at H*C, and at C - the width of the
    output, where the mask and the bias gradient are formed - when the heads are averaged."""
    return fused_gnn_ok(h) and (not mean or fused_gnn_ok(h[:, :h.size(1) // heads]))


class _GatHeadsConvFn(torch.autograd.Function):
    """Everything of a multi-head GATConv layer behind its ``lin`` - ``_GatConvFn`` with H weights per edge: the dot
    products of all heads in one pass over h, edge softmax, ``act(aggregation + bias)`` (concatenated, or the mean over
    the heads) as one launch that gathers every neighbour row once; backward: mask + bias gradient in one pass, (mean:
    the gradient spread to the heads,) transposed aggregation, SDDMM + softmax backward, and the dot products' backward
    with the two ``[H, C]`` attention gradients in one pass."""

    @staticmethod
    def forward(ctx, g: GraphIndex, h, att_src, att_dst, bias, slope: float, relu: bool, nh: int, mean: bool):
        h = h.contiguous()
        n, f = h.shape
        c = f // nh
        a_s, a_d = att_src.reshape(-1).contiguous(), att_dst.reshape(-1).contiguous()
        a_src, a_dst = _heads_alpha_fwd(h, a_s, a_d, nh, c)
        alpha = _heads_softmax_fwd(g, a_src, a_dst, slope, n, nh)
        y = _heads_agg(g.fwd, alpha, h, bias, relu, mean, nh, c)
        ctx.g, ctx.slope, ctx.relu, ctx.nh, ctx.c, ctx.mean = g, slope, relu, nh, c, mean
        ctx.params = (att_src, att_dst, bias)
        ctx.save_for_backward(h, a_src, a_dst, alpha, a_s, a_d, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        h, a_src, a_dst, alpha, a_s, a_d, y = ctx.saved_tensors
        g, slope, nh, c = ctx.g, ctx.slope, ctx.nh, ctx.c
        att_src, att_dst, bias = ctx.params
        gm, gb = _heads_out_grad(ctx, gy, y, bias)
        gh, g_a_src, g_a_dst, _ = _gat_heads_edge_backward(g, gm, h, a_src, a_dst, alpha, slope, nh, c)
        # the attention dot products' backward: gh += ga_src att_src + ga_dst att_dst per head, the two [H, C] gradients
        pg = _ParamGrads([att_src, att_dst], ctx.needs_input_grad[2:4], h.device)
        _heads_alpha_bwd(h, g_a_src, g_a_dst, a_s, a_d, gh, nh, c, *pg.bufs, pg.direct)
        gs, gd = pg.done()
        return None, gh, gs, gd, gb, None, None, None, None


def gat_heads_conv(g: GraphIndex, h, att_src, att_dst, bias, slope: float, relu: bool = False, heads: int = 1,
                   mean: bool = False) -> torch.Tensor:
    """The layer behind ``lin`` for ``heads`` >= 1 (``h`` [N, H*C], ``att_*`` [1, H, C]; ``gat_heads_fused_ok``)."""
    h = resolve(h)
    if h.dim() != 2 or heads < 1 or h.size(1) != att_src.numel() or att_src.numel() % heads:
        raise ValueError("gat_heads_conv: h must be [N, H*C] and att_src / att_dst [1, H, C]")
    return _GatHeadsConvFn.apply(g, h, att_src, att_dst, bias, float(slope), bool(relu), int(heads), bool(mean))


# --------------------------------------------------------------------------- #
# GATConv with edge features (dc_gat_edge.hip; the softmax with the per-edge addend shares dc_gat_heads.hip's templates).
# The edge term <lin_edge(edge_attr[p])[k, :], att_edge[k, :]> is linear in edge_attr: a_edge = edge_attr @ M with the
# folded M [D, H] formed by ordinary torch ops OUTSIDE the Functions below, so autograd turns their gM into the
# gradients of lin_edge.weight and att_edge.  One launcher per C entry.
# --------------------------------------------------------------------------- #
GAT_EDGE_MAX_DIM = _lib.DEFINES["DC_GAT_EDGE_MAX_DIM"]


def gat_edge_fold(lin_edge_weight: torch.Tensor, att_edge: torch.Tensor) -> torch.Tensor:
    """``M[d, k] = sum_c lin_edge.weight[k C + c, d] att_edge[k, c]`` ([D, H]; differentiable, D*H*C flops)."""
    _, nh, c = att_edge.shape
    return (lin_edge_weight.view(nh, c, -1) * att_edge.view(nh, c, 1)).sum(1).t().contiguous()


def gat_edge_fill(fill_value):
    """``fill_value`` of the appended self loops' attribute -> (mean?, constant): ``"mean"`` or a Python number."""
    if isinstance(fill_value, str):
        if fill_value != "mean":
            raise ValueError(f"fill_value must be 'mean' or a float, got {fill_value!r}")
        return True, 0.0
    if isinstance(fill_value, bool) or not isinstance(fill_value, (int, float)):
        raise ValueError(f"fill_value must be 'mean' or a float, got {fill_value!r}")
    return False, float(fill_value)


def _edge_operands(g: GraphIndex, edge_attr, m, nh: int, fill_value):
    """Checked operands of the edge-feature kernels: ``edge_attr`` float32 [E, D] with inner stride 1 on the graph's
    device, ``m`` [D, H], the graph a plain self-loop adjacency (its ``perm`` holds this ``edge_index``'s edge ids)."""
    fill_mean, fill = gat_edge_fill(fill_value)
    if m is None or m.dim() != 2 or m.size(1) != nh:
        raise ValueError("edge_m must be the folded [edge_dim, heads] matrix (ops.gat_edge_fold)")
    d = m.size(0)
    if not 1 <= d <= GAT_EDGE_MAX_DIM:
        raise ValueError(f"edge_dim = {d}: the edge-feature kernels take 1 <= edge_dim <= {GAT_EDGE_MAX_DIM}")
    if not isinstance(g, GraphIndex) or g.parts is not None or not g.self_loops:
        raise ValueError("edge features need the layer's own self-loop adjacency of this edge_index (not a merged one)")
    _require_cuda(edge_attr, "edge_attr")
    if edge_attr.dtype != torch.float32:
        raise ValueError(f"edge_attr must be float32, got {edge_attr.dtype}")
    if edge_attr.dim() == 1 and d == 1:
        edge_attr = edge_attr.unsqueeze(-1)
    if edge_attr.dim() != 2 or edge_attr.size(1) != d:
        raise ValueError(f"edge_attr must be [E, {d}] (edge_dim = {d}), got {tuple(edge_attr.shape)}")
    if edge_attr.size(0) != g.num_input_edges:
        raise ValueError(f"edge_attr has {edge_attr.size(0)} rows for {g.num_input_edges} edges")
    if edge_attr.device != g.device:
        raise RuntimeError(f"edge_attr is on {edge_attr.device} but the graph is on {g.device}")
    if edge_attr.stride(1) != 1 or (edge_attr.size(0) > 1 and edge_attr.stride(0) < d):
        edge_attr = edge_attr.contiguous()                       # (a row stride is taken as it is)
    return edge_attr, fill_mean, fill


def _edge_lda(edge_attr) -> int:
    return edge_attr.stride(0) if edge_attr.size(0) > 1 else edge_attr.size(1)


def _edge_term_fwd(g: GraphIndex, edge_attr, m, fill_mean: bool, fill: float, n: int, nh: int):
    """(a_edge [capacity, H] in ``g.fwd`` order, loop_attr [N, D]: the attribute row of every appended self loop)"""
    dev, d = m.device, m.size(0)
    a_edge = _heads_edge_vector(g, nh, dev)
    loop_attr = torch.empty((n, d), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dc_gat_edge_attr_fwd(g.fwd.ptr.data_ptr(), g.fwd.perm.data_ptr(), _ptr(edge_attr) or None,
                                               _edge_lda(edge_attr), m.data_ptr(), int(fill_mean), fill,
                                               a_edge.data_ptr(), loop_attr.data_ptr(), n, g.num_input_edges, d, nh,
                                               current_stream_ptr(dev)), "dc_gat_edge_attr_fwd")
    return a_edge, loop_attr


def _edge_softmax_fwd(g: GraphIndex, a_src, a_dst, a_edge, slope: float, n: int, nh: int) -> torch.Tensor:
    alpha = _heads_edge_vector(g, nh, a_src.device)
    _lib.check(_lib.lib().dc_gat_edge_attr_softmax_fwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), a_src.data_ptr(),
                                                       a_dst.data_ptr(), a_edge.data_ptr(), slope, alpha.data_ptr(), n, nh,
                                                       current_stream_ptr(a_src.device)), "dc_gat_edge_attr_softmax_fwd")
    return alpha


def _edge_softmax_bwd(g: GraphIndex, a_src, a_dst, a_edge, slope: float, alpha, galpha, n: int, nh: int):
    dev = alpha.device
    ge = _heads_edge_vector(g, nh, dev)
    g_a_dst = torch.empty((n, nh), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dc_gat_edge_attr_softmax_bwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), a_src.data_ptr(),
                                                       a_dst.data_ptr(), a_edge.data_ptr(), slope, alpha.data_ptr(),
                                                       galpha.data_ptr(), ge.data_ptr(), g_a_dst.data_ptr(), n, nh,
                                                       current_stream_ptr(dev)), "dc_gat_edge_attr_softmax_bwd")
    return ge, g_a_dst


def _edge_term_bwd(g: GraphIndex, ge, edge_attr, loop_attr, m, fill_mean: bool, n: int, nh: int, need_attr: bool,
                   need_m: bool):
    """(g_edge_attr [E, D] or None, gM [D, H] or None) from ``ge``, the gradient of the logits (= of a_edge)."""
    if not (need_attr or need_m):
        return None, None
    L = _lib.lib()
    dev, d, e = m.device, m.size(0), g.num_input_edges
    g_attr = torch.empty((e, d), dtype=torch.float32, device=dev) if need_attr else None
    g_m = torch.empty((d, nh), dtype=torch.float32, device=dev) if need_m else None
    ws = torch.empty(max(L.dc_gat_edge_attr_bwd_workspace_bytes(g.capacity, d, nh), 16), dtype=torch.uint8, device=dev)
    _lib.check(L.dc_gat_edge_attr_bwd(g.fwd.ptr.data_ptr(), g.fwd.perm.data_ptr(), ge.data_ptr(), _ptr(edge_attr) or None,
                                      _edge_lda(edge_attr), loop_attr.data_ptr(), m.data_ptr(), int(fill_mean),
                                      _ptr(g_attr) or None, d, _ptr(g_m), n, e, d, nh, g.capacity, ws.data_ptr(),
                                      ws.numel(), current_stream_ptr(dev)), "dc_gat_edge_attr_bwd")
    return g_attr, g_m


class _GatHeadsEdgeAggregateFn(torch.autograd.Function):
    """``_GatHeadsAggregateFn`` with the edge-feature term in the logits: the unfused aggregation at the widths
    ``gat_heads_fused_ok`` does not take."""

    @staticmethod
    def forward(ctx, g: GraphIndex, h, a_src, a_dst, slope: float, nh: int, mean: bool, edge_attr, m, fill_mean: bool,
                fill: float):
        h, a_src, a_dst, m = h.contiguous(), a_src.contiguous(), a_dst.contiguous(), m.contiguous()
        n, c = h.size(0), h.size(1) // nh
        a_edge, loop_attr = _edge_term_fwd(g, edge_attr, m, fill_mean, fill, n, nh)
        alpha = _edge_softmax_fwd(g, a_src, a_dst, a_edge, slope, n, nh)
        out = _heads_agg(g.fwd, alpha, h, None, False, mean, nh, c)
        ctx.g, ctx.slope, ctx.nh, ctx.c, ctx.mean, ctx.fill_mean = g, slope, nh, c, mean, fill_mean
        ctx.save_for_backward(h, a_src, a_dst, alpha, a_edge, loop_attr, edge_attr, m)
        return out

    @staticmethod
    def backward(ctx, gout):
        h, a_src, a_dst, alpha, a_edge, loop_attr, edge_attr, m = ctx.saved_tensors
        gm = _grad_layout(gout, 0)
        if ctx.mean:
            gm = _heads_spread(gm, ctx.nh, ctx.c)
        gh, g_a_src, g_a_dst, ge = _gat_heads_edge_backward(ctx.g, gm, h, a_src, a_dst, alpha, ctx.slope, ctx.nh, ctx.c,
                                                            a_edge)
        g_attr, g_m = _edge_term_bwd(ctx.g, ge, edge_attr, loop_attr, m, ctx.fill_mean, h.size(0), ctx.nh,
                                     ctx.needs_input_grad[7], ctx.needs_input_grad[8])
        return None, gh, g_a_src, g_a_dst, None, None, None, g_attr, g_m, None, None


class _GatHeadsEdgeConvFn(torch.autograd.Function):
    """``_GatHeadsConvFn`` with the edge-feature term in the logits (every H >= 1): the edge-term launch in front of the
    softmax, the softmax entries with the per-edge addend, and in backward one more entry for the gradients of
    ``edge_attr`` (through the loops' mean fill too) and of the folded ``M``."""

    @staticmethod
    def forward(ctx, g: GraphIndex, h, att_src, att_dst, bias, slope: float, relu: bool, nh: int, mean: bool, edge_attr,
                m, fill_mean: bool, fill: float):
        h, m = h.contiguous(), m.contiguous()
        n, f = h.shape
        c = f // nh
        a_s, a_d = att_src.reshape(-1).contiguous(), att_dst.reshape(-1).contiguous()
        a_src, a_dst = _heads_alpha_fwd(h, a_s, a_d, nh, c)
        a_edge, loop_attr = _edge_term_fwd(g, edge_attr, m, fill_mean, fill, n, nh)
        alpha = _edge_softmax_fwd(g, a_src, a_dst, a_edge, slope, n, nh)
        y = _heads_agg(g.fwd, alpha, h, bias, relu, mean, nh, c)
        ctx.g, ctx.slope, ctx.relu, ctx.nh, ctx.c, ctx.mean, ctx.fill_mean = g, slope, relu, nh, c, mean, fill_mean
        ctx.params = (att_src, att_dst, bias)
        ctx.save_for_backward(h, a_src, a_dst, alpha, a_s, a_d, y if relu else None, a_edge, loop_attr, edge_attr, m)
        return y

    @staticmethod
    def backward(ctx, gy):
        h, a_src, a_dst, alpha, a_s, a_d, y, a_edge, loop_attr, edge_attr, m = ctx.saved_tensors
        g, slope, nh, c = ctx.g, ctx.slope, ctx.nh, ctx.c
        att_src, att_dst, bias = ctx.params
        gm, gb = _heads_out_grad(ctx, gy, y, bias)
        gh, g_a_src, g_a_dst, ge = _gat_heads_edge_backward(g, gm, h, a_src, a_dst, alpha, slope, nh, c, a_edge)
        g_attr, g_m = _edge_term_bwd(g, ge, edge_attr, loop_attr, m, ctx.fill_mean, h.size(0), nh,
                                     ctx.needs_input_grad[9], ctx.needs_input_grad[10])
        pg = _ParamGrads([att_src, att_dst], ctx.needs_input_grad[2:4], h.device)
        _heads_alpha_bwd(h, g_a_src, g_a_dst, a_s, a_d, gh, nh, c, *pg.bufs, pg.direct)
        gs, gd = pg.done()
        return None, gh, gs, gd, gb, None, None, None, None, g_attr, g_m, None, None


def gat_heads_edge_conv(g: GraphIndex, h, att_src, att_dst, bias, slope: float, edge_attr, edge_m, relu: bool = False,
                        heads: int = 1, mean: bool = False, fill_value="mean") -> torch.Tensor:
    """``gat_heads_conv`` with edge features: ``edge_attr`` [E, D] in the order of the graph's ``edge_index``, ``edge_m``
    [D, H] = ``gat_edge_fold(lin_edge.weight, att_edge)``; ``fill_value``: the appended self loops' attribute."""
    h = resolve(h)
    if h.dim() != 2 or heads < 1 or h.size(1) != att_src.numel() or att_src.numel() % heads:
        raise ValueError("gat_heads_edge_conv: h must be [N, H*C] and att_src / att_dst [1, H, C]")
    edge_attr, fill_mean, fill = _edge_operands(g, edge_attr, edge_m, int(heads), fill_value)
    return _GatHeadsEdgeConvFn.apply(g, h, att_src, att_dst, bias, float(slope), bool(relu), int(heads), bool(mean),
                                     edge_attr, edge_m, fill_mean, fill)
