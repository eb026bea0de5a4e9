"""GINEConv's aggregation."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from .._host import _graph_check, _ptr, _rowmajor, _rows
from ..deferred import resolve
from ..graph import GraphIndex, _require_cuda, current_stream_ptr
from .sage import _sage_grad


# --------------------------------------------------------------------------- #
# GINEConv (dc_gine.hip): (1 + eps) x_i + the sum over the in-edges of relu(x_j + e_ji) on the edge set as it is given,
# e [E, F] in the order of the input edges (read through the adjacency's ``perm``).  The backward recomputes the ReLU
# mask from x and e.  One launcher per C entry.
# --------------------------------------------------------------------------- #
def _gine_fwd(g: GraphIndex, x, e, eps) -> torch.Tensor:
    """y [N, F]: ``(1 + eps) x[i] + sum_p max(x[other[p]] + e[perm[p]], 0)`` in p order; ``eps`` None: no root term."""
    n, f = x.shape
    y = torch.empty((n, f), dtype=torch.float32, device=x.device)
    if e.size(0) == 0:
        e = x                                # no edge: e has no address, and the kernel reads it per edge only
    _lib.check(_lib.lib().dc_gine_fwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), g.fwd.perm.data_ptr(), x.data_ptr(),
                                      _rowmajor(x, "x"), e.data_ptr(), _rowmajor(e, "e"), _ptr(eps), y.data_ptr(), f,
                                      n, f, current_stream_ptr(x.device)), "dc_gine_fwd")
    return y


def _gine_bwd_x(g: GraphIndex, x, e, eps, gy) -> torch.Tensor:
    """g_x [N, F] over the transposed set: ``(1 + eps) g_y[j] + sum_t (x[j] + e[perm_t[t]] > 0) g_y[other_t[t]]``."""
    n, f = x.shape
    gx = torch.empty((n, f), dtype=torch.float32, device=x.device)
    if e.size(0) == 0:
        e = x
    _lib.check(_lib.lib().dc_gine_bwd_x(g.bwd.ptr.data_ptr(), g.bwd.other.data_ptr(), g.bwd.perm.data_ptr(),
                                        x.data_ptr(), _rowmajor(x, "x"), e.data_ptr(), _rowmajor(e, "e"), _ptr(eps),
                                        gy.data_ptr(), _rowmajor(gy, "gy"), gx.data_ptr(), f, n, f,
                                        current_stream_ptr(x.device)), "dc_gine_bwd_x")
    return gx


def _gine_bwd_e(g: GraphIndex, x, e, gy) -> torch.Tensor:
    """g_e [E, F] in the order of the input edges: ``(x[src_q] + e[q] > 0) g_y[dst_q]``, every row written once."""
    n, f = x.shape
    ne = e.size(0)
    ge = torch.empty((ne, f), dtype=torch.float32, device=x.device)
    if ne == 0:
        return ge
    ei = g.edge_index
    _lib.check(_lib.lib().dc_gine_bwd_e(ei[0].data_ptr(), ei[1].data_ptr(), x.data_ptr(), _rowmajor(x, "x"),
                                        e.data_ptr(), _rowmajor(e, "e"), gy.data_ptr(), _rowmajor(gy, "gy"),
                                        ge.data_ptr(), f, n, ne, f, current_stream_ptr(x.device)), "dc_gine_bwd_e")
    return ge


class _GineAggFn(torch.autograd.Function):
    """``(1 + eps) x_i + sum relu(x_j + e_ji)``: one launch forward; backward one launch for g_x, one for g_e (skipped
    when e needs no gradient) and a torch reduction ``sum(g_y * x)`` for a trained eps.  Saved: x, e, eps - the ReLU
    mask is recomputed."""

    @staticmethod
    def forward(ctx, g: GraphIndex, x, e, eps):
        ctx.g, ctx.empty = g, x.size(0) == 0
        if ctx.empty:                        # no rows: nothing to launch (an empty tensor has no address)
            return x.new_empty(x.shape)
        ctx.save_for_backward(x, e, eps)
        return _gine_fwd(g, x, e, eps)

    @staticmethod
    def backward(ctx, gy):
        need = ctx.needs_input_grad
        if ctx.empty:
            return (None, gy.new_zeros(gy.shape) if need[1] else None, gy.new_zeros(gy.shape) if need[2] else None,
                    gy.new_zeros(1) if need[3] else None)
        x, e, eps = ctx.saved_tensors
        gy = _sage_grad(gy)
        gx = _gine_bwd_x(ctx.g, x, e, eps, gy) if need[1] else None
        ge = _gine_bwd_e(ctx.g, x, e, gy) if need[2] else None
        geps = (gy * x).sum().reshape(1) if need[3] else None
        return None, gx, ge, geps


def gine_aggregate(g: Optional[GraphIndex], x: torch.Tensor, e: torch.Tensor,
                   eps: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``(1 + eps) x_i + sum_{j->i} relu(x_j + e_ji)`` over the edges of ``g`` - a ``GraphIndex`` of one ``edge_index``
    built with ``self_loops=False, normalize=False``: the edge set as given, duplicates counting; a row without edges
    is ``(1 + eps) x_i``.  ``x``: float32 ``[N, F]``; ``e``: float32 ``[E, F]`` with rows in the order of that
    ``edge_index``; both on the graph's device with unit inner stride (column slices pass as they are).  ``eps``: a
    float32 ``[1]`` tensor on the same device, read BY THE KERNEL (a parameter changed in place between two replays of
    a captured step is followed); None: no root term.  One autograd node, differentiable in ``x``, ``e`` and - when it
    requires a gradient - ``eps``; ``relu'(0) = 0``.  The gradient of ``e`` reads the endpoints
    from ``g.edge_index`` at backward time while the forward read the sorted set built from it: the edge list must stay
    unchanged until the backward has run.  ``N = 0`` returns an empty tensor without
    a launch (``g`` may then be None)."""
    x, e = resolve(x), resolve(e)
    _require_cuda(x, "x")
    _require_cuda(e, "e")
    if x.dim() != 2 or x.dtype != torch.float32 or x.size(1) == 0:
        raise ValueError(f"gine_aggregate: x must be a float32 [N, F >= 1] tensor, got {tuple(x.shape)} {x.dtype}")
    if e.dim() != 2 or e.dtype != torch.float32 or e.size(1) != x.size(1):
        raise ValueError(f"gine_aggregate: e must be a float32 [E, {x.size(1)}] tensor, got {tuple(e.shape)} {e.dtype}")
    if e.device != x.device:
        raise RuntimeError(f"gine_aggregate: x is on {x.device} but e is on {e.device}")
    if eps is not None:
        if not isinstance(eps, torch.Tensor) or eps.dtype != torch.float32 or eps.numel() != 1:
            raise ValueError("gine_aggregate: eps must be a float32 tensor of one element (or None)")
        if eps.device != x.device:
            raise RuntimeError(f"gine_aggregate: x is on {x.device} but eps is on {eps.device}")
    if x.size(0) == 0:
        if e.size(0) != 0:
            raise ValueError(f"gine_aggregate: e has {e.size(0)} rows but x has no node")
        return _GineAggFn.apply(None, x, e, eps)
    if g is None:
        raise ValueError("gine_aggregate: g may be None only for an x without rows")
    _graph_check("gine_aggregate", g, False, x, "x")
    if g.num_nodes != x.size(0):
        raise ValueError(f"gine_aggregate: x has {x.size(0)} rows but the graph has {g.num_nodes} nodes")
    if g.num_input_edges != e.size(0):
        raise ValueError(f"gine_aggregate: e has {e.size(0)} rows but the graph has {g.num_input_edges} edges")
    return _GineAggFn.apply(g, _rows(x), _rows(e), eps)
