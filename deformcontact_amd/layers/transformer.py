"""TransformerConv on the multi-head launchers of ``gat_heads``."""
from __future__ import annotations

import torch

from .. import _lib
from .._host import _rowmajor
from ..deferred import resolve
from ..graph import GraphIndex, current_stream_ptr
from .gat_heads import _heads_agg, _heads_edge_vector, _heads_out_grad, _heads_sddmm, gat_heads_fused_ok


# --------------------------------------------------------------------------- #
# TransformerConv (dc_transformer.hip): q = lin_query(x), k = lin_key(x), v = lin_value(x) [N, H*C]; the logit is the
# scaled dot product <q_i, k_j> / sqrt(C) per edge and head.  Score + edge softmax and both sides of the backward are
# gather kernels of their own; aggregation, SDDMM, spread and the mask / bias gradient pass are the multi-head
# launchers above.  One launcher per C entry.
# --------------------------------------------------------------------------- #
def _tconv_scale(c: int) -> float:
    """``float32(1 / sqrt(C))`` (the C entries take a float: ctypes rounds the double to nearest)"""
    return 1.0 / float(c) ** 0.5


def _tconv_softmax_fwd(g: GraphIndex, q, k, nh: int, c: int) -> torch.Tensor:
    """alpha [capacity, H]: the edge softmax of ``e[p, h] = <q[i, h, :], k[j, h, :]> / sqrt(C)``."""
    alpha = _heads_edge_vector(g, nh, q.device)
    _lib.check(_lib.lib().dc_tconv_softmax_fwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), q.data_ptr(),
                                               _rowmajor(q, "q"), k.data_ptr(), _rowmajor(k, "k"), _tconv_scale(c),
                                               alpha.data_ptr(), q.size(0), nh, c, current_stream_ptr(q.device)),
               "dc_tconv_softmax_fwd")
    return alpha


def _tconv_softmax_bwd(g: GraphIndex, alpha, galpha, k, nh: int, c: int):
    """-> (gl [capacity, H], the gradient of the dot products; g_q [N, H*C])"""
    n, dev = k.size(0), k.device
    gl = _heads_edge_vector(g, nh, dev)
    g_q = torch.empty((n, nh * c), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dc_tconv_softmax_bwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), alpha.data_ptr(),
                                               galpha.data_ptr(), k.data_ptr(), _rowmajor(k, "k"), _tconv_scale(c),
                                               gl.data_ptr(), g_q.data_ptr(), nh * c, n, nh, c,
                                               current_stream_ptr(dev)), "dc_tconv_softmax_bwd")
    return gl, g_q


def _tconv_source_bwd(g: GraphIndex, alpha, gl, q, gm, nh: int, c: int):
    """-> (g_k, g_v) [N, H*C] over the transposed set: the score's key term and the transposed aggregation in one walk."""
    n, dev = q.size(0), q.device
    g_k = torch.empty((n, nh * c), dtype=torch.float32, device=dev)
    g_v = torch.empty((n, nh * c), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dc_tconv_source_bwd(g.bwd.ptr.data_ptr(), g.bwd.other.data_ptr(), g.bwd_to_fwd().data_ptr(),
                                              alpha.data_ptr(), gl.data_ptr(), q.data_ptr(), _rowmajor(q, "q"),
                                              gm.data_ptr(), _rowmajor(gm, "gm"), g_k.data_ptr(), nh * c, g_v.data_ptr(),
                                              nh * c, n, nh, c, current_stream_ptr(dev)), "dc_tconv_source_bwd")
    return g_k, g_v


class _TransformerAggFn(torch.autograd.Function):
    """The attention of a TransformerConv layer behind its three linears: score + edge softmax in one launch, then
    ``act(aggregation of v + bias)`` (concatenated, or the mean over the heads) as for ``_Gatv2ConvFn``; backward: mask
    + bias gradient in one pass (only with ``relu`` / ``bias``), (mean: the gradient spread to the heads,) SDDMM, then
    the destination side (gl, g_q) and the source side (g_k, g_v in one walk).  The node ends at the aggregation: the
    skip connection and the gate are the layer's."""

    @staticmethod
    def forward(ctx, g: GraphIndex, q, k, v, bias, relu: bool, nh: int, mean: bool):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        n, c = q.size(0), q.size(1) // nh
        ctx.g, ctx.relu, ctx.nh, ctx.c, ctx.mean, ctx.bias = g, relu, nh, c, mean, bias
        ctx.empty = n == 0
        if ctx.empty:                        # no rows: nothing to launch (an empty tensor has no address)
            return q.new_empty((0, c if mean else nh * c))
        alpha = _tconv_softmax_fwd(g, q, k, nh, c)
        y = _heads_agg(g.fwd, alpha, v, bias, relu, mean, nh, c)
        ctx.save_for_backward(q, k, v, alpha, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        g, nh, c, bias = ctx.g, ctx.nh, ctx.c, ctx.bias
        need_b = bias is not None and ctx.needs_input_grad[4]
        if ctx.empty:                        # sums over no rows
            z = gy.new_zeros((0, nh * c))
            return None, z, z, z, (gy.new_zeros(gy.size(1)) if need_b else None), None, None, None
        q, k, v, alpha, y = ctx.saved_tensors
        gm, gb = _heads_out_grad(ctx, gy, y, bias)
        galpha = _heads_sddmm(g, gm, v, nh, c)
        gl, g_q = _tconv_softmax_bwd(g, alpha, galpha, k, nh, c)
        g_k, g_v = _tconv_source_bwd(g, alpha, gl, q, gm, nh, c)
        return None, g_q, g_k, g_v, gb, None, None, None


def transformer_conv(g: GraphIndex, q, k, v, bias=None, relu: bool = False, heads: int = 1,
                     mean: bool = False) -> torch.Tensor:
    """The attention of a TransformerConv layer behind ``lin_query`` / ``lin_key`` / ``lin_value`` (``q`` / ``k`` / ``v``
    [N, H*C]) on the edge set of ``g`` as it is: [N, H*C], or [N, C] with ``mean``; a row without edges is 0 (+ bias).
    With ``bias`` or ``relu`` the widths must pass ``gat_heads_fused_ok`` (the mask / bias-gradient pass); the bare
    aggregation runs at every width."""
    q, k, v = resolve(q), resolve(k), resolve(v)
    if q.dim() != 2 or heads < 1 or q.size(1) % heads or q.size(1) == 0 or k.shape != q.shape or v.shape != q.shape:
        raise ValueError("transformer_conv: q / k / v must be [N, H*C]")
    if (bias is not None or relu) and not gat_heads_fused_ok(v, heads, mean):
        raise ValueError(f"transformer_conv: bias / relu need widths the fused row passes take (gat_heads_fused_ok), got "
                         f"H*C = {q.size(1)}, H = {heads}; call it without them and apply them outside")
    return _TransformerAggFn.apply(g, q, k, v, bias, bool(relu), int(heads), bool(mean))
