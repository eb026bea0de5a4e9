"""GATv2Conv on the multi-head launchers of ``gat_heads``."""
from __future__ import annotations

import torch

from .. import _lib
from .._host import _rowmajor
from ..deferred import resolve
from ..graph import GraphIndex, current_stream_ptr
from .gat_heads import _heads_agg, _heads_edge_vector, _heads_out_grad, _heads_sddmm, gat_heads_fused_ok
from .gnn import _ParamGrads


# --------------------------------------------------------------------------- #
# GATv2Conv (dc_gatv2.hip): xl = lin_l(x), xr = lin_r(x) [N, H*C]; the logit is per edge, head and channel, so the score
# and both sides of its backward are gather kernels of their own.  Aggregation, SDDMM, spread and the mask / bias
# gradient pass are the multi-head launchers above.  One launcher per C entry.
# --------------------------------------------------------------------------- #
def _gatv2_softmax_fwd(g: GraphIndex, xl, xr, att, slope: float, nh: int, c: int) -> torch.Tensor:
    """alpha [capacity, H]: the edge softmax of ``e[p, k] = sum_c att[k, c] leaky_relu(xl[j, k, c] + xr[i, k, c])``."""
    alpha = _heads_edge_vector(g, nh, xl.device)
    _lib.check(_lib.lib().dc_gatv2_softmax_fwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), xl.data_ptr(),
                                               _rowmajor(xl, "xl"), xr.data_ptr(), _rowmajor(xr, "xr"), att.data_ptr(),
                                               slope, alpha.data_ptr(), xl.size(0), nh, c, current_stream_ptr(xl.device)),
               "dc_gatv2_softmax_fwd")
    return alpha


def _gatv2_softmax_bwd(g: GraphIndex, alpha, galpha, xl, xr, att, slope: float, nh: int, c: int, g_att,
                       accumulate: bool):
    """-> (ge [capacity, H], g_xr [N, H*C]); ``g_att`` [H*C] is written (``accumulate``: added to)."""
    n, dev = xl.size(0), xl.device
    L = _lib.lib()
    ge = _heads_edge_vector(g, nh, dev)
    g_xr = torch.empty((n, nh * c), dtype=torch.float32, device=dev)
    ws = torch.empty(max(L.dc_gatv2_workspace_bytes(n, nh, c), 16), dtype=torch.uint8, device=dev)
    _lib.check(L.dc_gatv2_softmax_bwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), alpha.data_ptr(), galpha.data_ptr(),
                                      xl.data_ptr(), _rowmajor(xl, "xl"), xr.data_ptr(), _rowmajor(xr, "xr"),
                                      att.data_ptr(), slope, ge.data_ptr(), g_xr.data_ptr(), nh * c, g_att.data_ptr(),
                                      int(accumulate), ws.data_ptr(), ws.numel(), n, nh, c, current_stream_ptr(dev)),
               "dc_gatv2_softmax_bwd")
    return ge, g_xr


def _gatv2_source_bwd(g: GraphIndex, alpha, ge, gm, xl, xr, att, slope: float, nh: int, c: int) -> torch.Tensor:
    """g_xl [N, H*C] over the transposed set: the transposed aggregation of ``gm`` and the score's source term at once."""
    n, dev = xl.size(0), xl.device
    g_xl = torch.empty((n, nh * c), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dc_gatv2_source_bwd(g.bwd.ptr.data_ptr(), g.bwd.other.data_ptr(), g.bwd_to_fwd().data_ptr(),
                                              alpha.data_ptr(), ge.data_ptr(), gm.data_ptr(), _rowmajor(gm, "gm"),
                                              xl.data_ptr(), _rowmajor(xl, "xl"), xr.data_ptr(), _rowmajor(xr, "xr"),
                                              att.data_ptr(), slope, g_xl.data_ptr(), nh * c, n, nh, c,
                                              current_stream_ptr(dev)), "dc_gatv2_source_bwd")
    return g_xl


class _Gatv2ConvFn(torch.autograd.Function):
    """Everything of a GATv2Conv layer behind its two linears: score + edge softmax in one launch, then
    ``act(aggregation of xl + bias)`` (concatenated, or the mean over the heads) as for ``_GatHeadsConvFn``; backward:
    mask + bias gradient in one pass, (mean: the gradient spread to the heads,) SDDMM, then the destination side (ge,
    g_xr, g_att) and the source side (g_xl: the transposed aggregation and the score's term in one walk).  With
    ``bias`` None and ``relu`` False it is the bare aggregation, at every width."""

    @staticmethod
    def forward(ctx, g: GraphIndex, xl, xr, att, bias, slope: float, relu: bool, nh: int, mean: bool):
        shared = xl is xr
        xl = xl.contiguous()
        xr = xl if shared else xr.contiguous()
        c = xl.size(1) // nh
        a = att.reshape(-1).contiguous()
        alpha = _gatv2_softmax_fwd(g, xl, xr, a, slope, nh, c)
        y = _heads_agg(g.fwd, alpha, xl, bias, relu, mean, nh, c)
        ctx.g, ctx.slope, ctx.relu, ctx.nh, ctx.c, ctx.mean = g, slope, relu, nh, c, mean
        ctx.params = (att, bias)
        ctx.save_for_backward(xl, xr, alpha, a, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        xl, xr, alpha, a, y = ctx.saved_tensors
        g, slope, nh, c = ctx.g, ctx.slope, ctx.nh, ctx.c
        att, bias = ctx.params
        gm, gb = _heads_out_grad(ctx, gy, y, bias)
        galpha = _heads_sddmm(g, gm, xl, nh, c)
        pg = _ParamGrads([att], ctx.needs_input_grad[3:4], xl.device)
        ge, g_xr = _gatv2_softmax_bwd(g, alpha, galpha, xl, xr, a, slope, nh, c, pg.bufs[0], pg.direct)
        g_xl = _gatv2_source_bwd(g, alpha, ge, gm, xl, xr, a, slope, nh, c)
        (g_att,) = pg.done()
        return None, g_xl, g_xr, g_att, gb, None, None, None, None


def gatv2_conv(g: GraphIndex, xl, xr, att, bias, slope: float, relu: bool = False, heads: int = 1,
               mean: bool = False) -> torch.Tensor:
    """The GATv2Conv layer behind ``lin_l`` / ``lin_r`` (``xl`` / ``xr`` [N, H*C] - the same tensor with shared weights -
    ``att`` [1, H, C]).  With ``bias`` or ``relu`` the widths must pass ``gat_heads_fused_ok`` (the mask / bias-gradient
    pass); the bare aggregation (``bias`` None, ``relu`` False) runs at every width."""
    xl, xr = resolve(xl), resolve(xr)
    if (xl.dim() != 2 or heads < 1 or xl.shape != xr.shape or xl.size(1) != att.numel() or att.numel() % heads):
        raise ValueError("gatv2_conv: xl / xr must be [N, H*C] and att [1, H, C]")
    if (bias is not None or relu) and not gat_heads_fused_ok(xl, heads, mean):
        raise ValueError(f"gatv2_conv: bias / relu need widths the fused row passes take (gat_heads_fused_ok), got "
                         f"H*C = {xl.size(1)}, H = {heads}; call it without them and apply them outside")
    return _Gatv2ConvFn.apply(g, xl, xr, att, bias, float(slope), bool(relu), int(heads), bool(mean))
