"""SAGEConv's aggregation: mean / max / sum over a node's in-edges."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from .._host import _grad_layout, _ptr, _rowmajor, _rows
from ..deferred import resolve
from ..graph import GraphIndex, _require_cuda, current_stream_ptr
from ..ops import propagate


# --------------------------------------------------------------------------- #
# SAGEConv (dc_sage.hip): the mean and the max over a node's in-edges on the edge set as it is given.  Segment
# reductions over the sorted adjacency, their backward over the transposed set; the sum is the unweighted hop.  One
# launcher per C entry.
# --------------------------------------------------------------------------- #
def _sage_mean_fwd(g: GraphIndex, x) -> torch.Tensor:
    """y [N, F]: the hop's sum over the in-edges divided by the in-degree; 0 for a row without edges."""
    n, f = x.shape
    y = torch.empty((n, f), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dc_sage_mean_fwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), x.data_ptr(), _rowmajor(x, "x"),
                                           y.data_ptr(), f, n, f, current_stream_ptr(x.device)), "dc_sage_mean_fwd")
    return y


def _sage_mean_bwd(g: GraphIndex, gy) -> torch.Tensor:
    """g_x [N, F] over the transposed set: ``sum g_y[i] / deg_i``, the in-degree read from the forward ``ptr``."""
    n, f = gy.shape
    gx = torch.empty((n, f), dtype=torch.float32, device=gy.device)
    _lib.check(_lib.lib().dc_sage_mean_bwd(g.bwd.ptr.data_ptr(), g.bwd.other.data_ptr(), g.fwd.ptr.data_ptr(),
                                           gy.data_ptr(), _rowmajor(gy, "gy"), gx.data_ptr(), f, n, f,
                                           current_stream_ptr(gy.device)), "dc_sage_mean_bwd")
    return gx


def _sage_max_fwd(g: GraphIndex, x, want_cnt: bool):
    """-> (m [N, F], cnt int32 [N, F] or None): the maximum over the in-edges and the number of edges that attain it."""
    n, f = x.shape
    m = torch.empty((n, f), dtype=torch.float32, device=x.device)
    cnt = torch.empty((n, f), dtype=torch.int32, device=x.device) if want_cnt else None
    _lib.check(_lib.lib().dc_sage_max_fwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), x.data_ptr(), _rowmajor(x, "x"),
                                          m.data_ptr(), f, _ptr(cnt), f, n, f, current_stream_ptr(x.device)),
               "dc_sage_max_fwd")
    return m, cnt


def _sage_max_bwd(g: GraphIndex, x, m, cnt, gm) -> torch.Tensor:
    """g_x [N, F] over the transposed set: the gradient of every maximum split evenly among the edges that attain it."""
    n, f = x.shape
    gx = torch.empty((n, f), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dc_sage_max_bwd(g.bwd.ptr.data_ptr(), g.bwd.other.data_ptr(), x.data_ptr(), _rowmajor(x, "x"),
                                          m.data_ptr(), _rowmajor(m, "m"), cnt.data_ptr(),
                                          _rowmajor(cnt, "cnt", (torch.int32,)), gm.data_ptr(), _rowmajor(gm, "gm"),
                                          gx.data_ptr(), f, n, f, current_stream_ptr(x.device)), "dc_sage_max_bwd")
    return gx


def _sage_grad(g: torch.Tensor) -> torch.Tensor:
    """The incoming gradient with unit inner stride and rows that do not overlap (an expanded one is copied)."""
    return _rows(_grad_layout(g, 1))


class _SageMeanFn(torch.autograd.Function):
    """``mean`` over the in-edges: one launch forward, one backward; nothing is saved but the graph."""

    @staticmethod
    def forward(ctx, g: GraphIndex, x):
        ctx.g, ctx.empty = g, x.size(0) == 0
        if ctx.empty:                        # no rows: nothing to launch (an empty tensor has no address)
            return x.new_empty(x.shape)
        return _sage_mean_fwd(g, x)

    @staticmethod
    def backward(ctx, gy):
        if ctx.empty:
            return None, gy.new_zeros(gy.shape)
        return None, _sage_mean_bwd(ctx.g, _sage_grad(gy))


class _SageMaxFn(torch.autograd.Function):
    """``max`` over the in-edges; with a gradient wanted the forward also stores the tie counts, and x, m, cnt are
    saved for the even split of the backward."""

    @staticmethod
    def forward(ctx, g: GraphIndex, x):
        ctx.g, ctx.empty = g, x.size(0) == 0
        if ctx.empty:
            return x.new_empty(x.shape)
        m, cnt = _sage_max_fwd(g, x, ctx.needs_input_grad[1])
        if cnt is not None:
            ctx.save_for_backward(x, m, cnt)
        return m

    @staticmethod
    def backward(ctx, gm):
        if ctx.empty:
            return None, gm.new_zeros(gm.shape)
        x, m, cnt = ctx.saved_tensors
        return None, _sage_max_bwd(ctx.g, x, m, cnt, _sage_grad(gm))


def aggregate(g: Optional[GraphIndex], x: torch.Tensor, reduce: str = "mean") -> torch.Tensor:
    """``reduce`` (``"sum"`` / ``"mean"`` / ``"max"``) of ``x[j]`` over the edges ``j -> i`` of ``g`` - a ``GraphIndex``
    built with ``self_loops=False, normalize=False``: the edge set as given, duplicates counting - per destination ``i``;
    a row without edges is 0.  ``"sum"`` is ``propagate(g, x, weighted=False)``; ``"mean"`` is that sum divided by the
    in-degree in the same launch; ``"max"`` sends the gradient of every maximum in equal shares to ALL edges that
    attain it.  ``x``: float32 ``[N, F]`` on the graph's device, unit inner stride (a column slice
    passes as it is).  ``N = 0`` returns an empty tensor without a launch (``g`` may then be None)."""
    if not isinstance(reduce, str) or reduce not in ("sum", "mean", "max"):
        raise ValueError(f"aggregate: reduce must be 'sum', 'mean' or 'max', got {reduce!r}")
    x = resolve(x)
    _require_cuda(x, "x")
    if x.dim() != 2 or x.dtype != torch.float32 or x.size(1) == 0:
        raise ValueError(f"aggregate: x must be a float32 [N, F >= 1] tensor, got {tuple(x.shape)} {x.dtype}")
    if x.size(0) == 0:
        return _SageMeanFn.apply(None, x)
    if g is None:
        raise ValueError("aggregate: g may be None only for an x without rows")
    if g.self_loops or g.normalize:
        raise ValueError("aggregate: the graph must be built with self_loops=False, normalize=False")
    if g.device != x.device:
        raise RuntimeError(f"aggregate: x is on {x.device} but the graph is on {g.device}")
    if g.num_nodes != x.size(0):
        raise ValueError(f"aggregate: x has {x.size(0)} rows but the graph has {g.num_nodes} nodes")
    if reduce == "sum":
        return propagate(g, x, weighted=False)
    if x.size(1) > 1 and x.stride(1) != 1:
        x = x.contiguous()
    return (_SageMeanFn if reduce == "mean" else _SageMaxFn).apply(g, x)
