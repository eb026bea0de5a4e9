"""The per-edge primitives of EdgeConv: pair rows and their reduction per destination."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from .._host import _graph_check, _ptr, _rowmajor, _rows
from ..deferred import resolve
from ..graph import GraphIndex, _require_cuda, current_stream_ptr
from .sage import _sage_grad


# --------------------------------------------------------------------------- #
# Per-edge primitives (dc_edge.hip): the pair rows [x_i, x_j - x_i] of every input edge, and the reduction per
# destination of rows that live on the edges - what a "module per edge" layer (EdgeConv) puts around the user's module.
# Edge rows are in the order of the input edges; the per-edge kernels read the endpoints from ``g.edge_index``, the
# per-node kernels walk the sorted sets through their ``perm``.  One launcher per C entry.
# --------------------------------------------------------------------------- #
EDGE_REDUCE_MODES = {"sum": 0, "mean": 1, "max": 2}


def _edge_pair_fwd(g: GraphIndex, x) -> torch.Tensor:
    """z [E, 2F] in the order of the input edges: ``[x[dst_q], x[src_q] - x[dst_q]]``, every row written once."""
    n, f = x.shape
    ne = g.num_input_edges
    z = torch.empty((ne, 2 * f), dtype=torch.float32, device=x.device)
    ei = g.edge_index
    _lib.check(_lib.lib().dc_edge_pair_fwd(ei[0].data_ptr(), ei[1].data_ptr(), x.data_ptr(), _rowmajor(x, "x"),
                                           z.data_ptr(), 2 * f, n, ne, f, current_stream_ptr(x.device)),
               "dc_edge_pair_fwd")
    return z


def _edge_pair_bwd(g: GraphIndex, gz) -> torch.Tensor:
    """g_x [N, F]: per node the compensated sum of ``g_z[q, :F] - g_z[q, F:]`` over its in-edges, then of
    ``g_z[q, F:]`` over its out-edges."""
    n, f = g.num_nodes, gz.size(1) // 2
    gx = torch.empty((n, f), dtype=torch.float32, device=gz.device)
    _lib.check(_lib.lib().dc_edge_pair_bwd(g.fwd.ptr.data_ptr(), g.fwd.perm.data_ptr(), g.bwd.ptr.data_ptr(),
                                           g.bwd.perm.data_ptr(), gz.data_ptr(), _rowmajor(gz, "gz"), gx.data_ptr(), f,
                                           n, f, current_stream_ptr(gz.device)), "dc_edge_pair_bwd")
    return gx


def _edge_reduce_fwd(g: GraphIndex, m, mode: int, n: Optional[int] = None):
    """-> (y [N, C], cnt int32 [N, C] for the max, else None): sum / mean / max of the edge rows per destination.
    ``n``: reduce the first ``n`` rows of the adjacency alone (the destinations of a bipartite set; default: all)."""
    n, c = g.num_nodes if n is None else n, m.size(1)
    y = torch.empty((n, c), dtype=torch.float32, device=m.device)
    cnt = torch.empty((n, c), dtype=torch.int32, device=m.device) if mode == 2 else None
    _lib.check(_lib.lib().dc_edge_reduce_fwd(g.fwd.ptr.data_ptr(), g.fwd.perm.data_ptr(), m.data_ptr(),
                                             _rowmajor(m, "m"), y.data_ptr(), c, _ptr(cnt), c, mode, n, c,
                                             current_stream_ptr(m.device)), "dc_edge_reduce_fwd")
    return y, cnt


def _edge_reduce_bwd(g: GraphIndex, m, y, cnt, gy, mode: int) -> torch.Tensor:
    """g_m [E, C] in the order of the input edges, every row written once; ``m``, ``y``, ``cnt``: the max only."""
    n, c = gy.shape
    ne = g.num_input_edges
    gm = torch.empty((ne, c), dtype=torch.float32, device=gy.device)
    ei = g.edge_index
    saved = [m.data_ptr(), _rowmajor(m, "m"), y.data_ptr(), _rowmajor(y, "y"), cnt.data_ptr(),
             _rowmajor(cnt, "cnt", (torch.int32,))] if mode == 2 else [None, c, None, c, None, c]
    _lib.check(_lib.lib().dc_edge_reduce_bwd(ei[0].data_ptr(), ei[1].data_ptr(), g.fwd.ptr.data_ptr(), *saved,
                                             gy.data_ptr(), _rowmajor(gy, "gy"), gm.data_ptr(), c, mode, n, ne, c,
                                             current_stream_ptr(gy.device)), "dc_edge_reduce_bwd")
    return gm


class _EdgePairFn(torch.autograd.Function):
    """``[x_i, x_j - x_i]`` per input edge: one launch forward, one backward; nothing is saved but the graph."""

    @staticmethod
    def forward(ctx, g: Optional[GraphIndex], x):
        ne = g.num_input_edges if g is not None else 0
        ctx.g, ctx.empty = g, ne == 0 or x.size(0) == 0
        if ctx.empty:                        # no edge or no node: nothing to launch (an empty tensor has no address)
            return x.new_empty((ne, 2 * x.size(1)))
        return _edge_pair_fwd(g, x)

    @staticmethod
    def backward(ctx, gz):
        if ctx.empty:
            return None, gz.new_zeros((ctx.g.num_nodes if ctx.g is not None else 0, gz.size(1) // 2))
        return None, _edge_pair_bwd(ctx.g, _sage_grad(gz))


class _EdgeReduceFn(torch.autograd.Function):
    """``sum`` / ``mean`` / ``max`` of edge rows per destination: one launch forward, one backward.  The max saves m,
    y and cnt for the even split of the backward; sum and mean save nothing but the graph."""

    @staticmethod
    def forward(ctx, g: Optional[GraphIndex], m, mode: int):
        n = g.num_nodes if g is not None else 0
        ctx.g, ctx.mode, ctx.empty = g, mode, n == 0 or m.size(0) == 0
        if ctx.empty:                        # no edge: every row is 0; no node: no row
            return m.new_zeros((n, m.size(1)))
        y, cnt = _edge_reduce_fwd(g, m, mode)
        if mode == 2:
            ctx.save_for_backward(m, y, cnt)
        return y

    @staticmethod
    def backward(ctx, gy):
        if ctx.empty:
            return None, gy.new_zeros((ctx.g.num_input_edges if ctx.g is not None else 0, gy.size(1))), None
        m, y, cnt = ctx.saved_tensors if ctx.mode == 2 else (None, None, None)
        return None, _edge_reduce_bwd(ctx.g, m, y, cnt, _sage_grad(gy), ctx.mode), None


_edge_rows = _rows              # the layout of every operand that holds rows per edge or per node


def edge_pairs(g: Optional[GraphIndex], x: torch.Tensor) -> torch.Tensor:
    """``z [E, 2F]`` with ``z[q] = [x[i], x[j] - x[i]]`` for every edge ``q = (j -> i)`` of ``g``, rows in the order of
    the ``edge_index`` the graph was built from - the per-edge input of PyG's ``EdgeConv``.  ``g``: a ``GraphIndex`` of
    one ``edge_index`` built with ``self_loops=False, normalize=False`` (the edge set as given, duplicates counting).
    ``x``: float32 ``[N, F >= 1]`` on the graph's device with unit inner stride (a column slice passes as it is).  One
    autograd node; the backward sums per node in a fixed order without float atomics and reads
    nothing but the graph.  The forward reads the endpoints from ``g.edge_index`` while the backward walks the sorted
    set built from it: the edge list must stay unchanged until the backward has run.  ``E = 0`` or ``N = 0`` returns
    an empty ``[E, 2F]`` tensor without a launch (``g`` may be None when ``N = 0``)."""
    x = resolve(x)
    _require_cuda(x, "x")
    if x.dim() != 2 or x.dtype != torch.float32 or x.size(1) == 0:
        raise ValueError(f"edge_pairs: x must be a float32 [N, F >= 1] tensor, got {tuple(x.shape)} {x.dtype}")
    if g is None:
        if x.size(0) != 0:
            raise ValueError("edge_pairs: g may be None only for an x without rows")
        return _EdgePairFn.apply(None, x)
    _graph_check("edge_pairs", g, False, x, "x")
    if g.num_nodes != x.size(0):
        raise ValueError(f"edge_pairs: x has {x.size(0)} rows but the graph has {g.num_nodes} nodes")
    return _EdgePairFn.apply(g, _edge_rows(x))


def edge_aggregate(g: Optional[GraphIndex], m: torch.Tensor, reduce: str = "max") -> torch.Tensor:
    """``reduce`` (``"sum"`` / ``"mean"`` / ``"max"``) per destination ``i`` of the rows ``m[q]`` that live on the edges
    ``q = (j -> i)`` of ``g`` -> ``[N, C]``; a node without in-edges gets 0.  ``m``: float32 ``[E, C >= 1]`` with rows
    in the order of the ``edge_index`` the graph was built from (``E = g.num_input_edges``), on the graph's device,
    unit inner stride (a column slice passes as it is).  ``g`` as for ``edge_pairs``.  The sum is a plain fp32 sum in
    the order of the sorted set, the mean that sum divided by the in-degree; ``"max"`` sends the gradient of every
    maximum in equal shares to ALL edges that attain it, a duplicate edge counting as an edge (INTEGRATION.md 1.5,
    1.10).  One autograd node; the backward writes every row of the gradient once and reads the endpoints from
    ``g.edge_index``: the edge list must stay unchanged until the backward has run.  ``N = 0``: ``g`` may be None and
    the result is an empty ``[0, C]`` tensor; nothing is launched for ``E = 0`` either."""
    if not isinstance(reduce, str) or reduce not in EDGE_REDUCE_MODES:
        raise ValueError(f"edge_aggregate: reduce must be 'sum', 'mean' or 'max', got {reduce!r}")
    m = resolve(m)
    _require_cuda(m, "m")
    if m.dim() != 2 or m.dtype != torch.float32 or m.size(1) == 0:
        raise ValueError(f"edge_aggregate: m must be a float32 [E, C >= 1] tensor, got {tuple(m.shape)} {m.dtype}")
    mode = EDGE_REDUCE_MODES[reduce]
    if g is None:
        if m.size(0) != 0:
            raise ValueError("edge_aggregate: g may be None only for an m without rows (a graph without nodes)")
        return _EdgeReduceFn.apply(None, m, mode)
    _graph_check("edge_aggregate", g, False, m, "m")
    if g.num_input_edges != m.size(0):
        raise ValueError(f"edge_aggregate: m has {m.size(0)} rows but the graph has {g.num_input_edges} edges")
    return _EdgeReduceFn.apply(g, _edge_rows(m), mode)
