"""The per-edge primitives of PointNetConv on a bipartite edge set."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib, ops
from .._host import _graph_check, _ptr, _rowmajor
from ..deferred import resolve
from ..graph import GraphIndex, _require_cuda, current_stream_ptr, graph_index
from .edge import EDGE_REDUCE_MODES, _edge_reduce_fwd, _edge_rows
from .sage import _sage_grad


# --------------------------------------------------------------------------- #
# PointNetConv (dc_pointnet.hip): the per-edge primitives on a BIPARTITE edge set - sources ``x_src`` / ``pos_src`` with
# ``Ns`` rows, destinations ``pos_dst`` with ``Nd`` rows - what PointNet++'s set-abstraction layer puts around the
# user's modules.  The adjacency is ONE ``GraphIndex`` over ``max(Ns, Nd)`` rows (``pointnet_graph``): rows beyond
# ``Nd`` (by destination) or ``Ns`` (by source) are empty, and the kernels are told the two counts.  With ``loops`` (one
# node set, an adjacency built with ``self_loops=True``) the edge rows are ``E' = E + N``: input edges in input order,
# then node ``i``'s loop at row ``E + i``; an input edge with ``src == dst`` keeps its row and takes no part.  The
# forward reduction is ``dc_edge_reduce_fwd`` as it stands.  One launcher per C entry.
# --------------------------------------------------------------------------- #
def pointnet_graph(edge_index: torch.Tensor, n_src: int, n_dst: int, loops: bool = False) -> GraphIndex:
    """The adjacency ``pointnet_pairs`` / ``pointnet_aggregate`` run on: ``graph_index(edge_index, max(n_src, n_dst),
    self_loops=loops, normalize=False)``."""
    return graph_index(edge_index, max(int(n_src), int(n_dst)), self_loops=bool(loops), normalize=False)


def _pointnet_edge_rows(g: GraphIndex, loops: bool) -> int:
    return g.num_input_edges + (g.num_nodes if loops else 0)


def _pointnet_pair_fwd(g: GraphIndex, x, pos_src, pos_dst, loops: bool, pad: bool = False) -> torch.Tensor:
    """z [E', F + 3] in the order of the edge rows: ``[x[src_q], pos_src[src_q] - pos_dst[dst_q]]``, a loop row
    ``[x[i], 0, 0, 0]``; every row written once.  ``x`` None: F = 0.  ``pad``: a row stride rounded up to 4; the
    result is then a view of the padded buffer, whose padding columns the kernel writes as zeros."""
    from ..neighbors import _ld
    ns, nd = pos_src.size(0), pos_dst.size(0)
    f = x.size(1) if x is not None else 0
    rows = _pointnet_edge_rows(g, loops)
    ldz = (f + 3 + 3) // 4 * 4 if pad else f + 3
    z = torch.empty((rows, ldz), dtype=torch.float32, device=pos_src.device)
    ei = g.edge_index
    _lib.check(_lib.lib().dc_pointnet_pair_fwd(
        ei[0].data_ptr(), ei[1].data_ptr(), _ptr(x), _rowmajor(x, "x") if x is not None else f, pos_src.data_ptr(),
        _ld(pos_src), pos_dst.data_ptr(), _ld(pos_dst), z.data_ptr(), ldz, ns, nd, g.num_input_edges, f, int(loops),
        ldz - (f + 3), current_stream_ptr(pos_src.device)), "dc_pointnet_pair_fwd")
    return z[:, :f + 3] if pad else z


def _pointnet_pair_bwd(g: GraphIndex, gz, ns: int, nd: int, loops: bool, want=(True, True, True)):
    """-> (g_x [Ns, F], g_pos_src [Ns, 3], g_pos_dst [Nd, 3]), each None where ``want`` says so (and g_x for F = 0):
    compensated sums over the sorted sets in their order."""
    f, dev = gz.size(1) - 3, gz.device
    gx = torch.empty((ns, f), dtype=torch.float32, device=dev) if want[0] and f > 0 else None
    gps = torch.empty((ns, 3), dtype=torch.float32, device=dev) if want[1] else None
    gpd = torch.empty((nd, 3), dtype=torch.float32, device=dev) if want[2] else None
    _lib.check(_lib.lib().dc_pointnet_pair_bwd(
        g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), g.fwd.perm.data_ptr(), g.bwd.ptr.data_ptr(),
        g.bwd.other.data_ptr(), g.bwd.perm.data_ptr(), gz.data_ptr(), _rowmajor(gz, "gz"), _ptr(gx), max(f, 1),
        _ptr(gps), 3, _ptr(gpd), 3, ns, nd, g.num_input_edges, f, int(loops), current_stream_ptr(dev)),
        "dc_pointnet_pair_bwd")
    return gx, gps, gpd


def _pointnet_reduce_bwd(g: GraphIndex, m, y, cnt, gy, mode: int, loops: bool) -> torch.Tensor:
    """g_m [E', C] in the order of the edge rows, every row written once (a removed input loop: zeros); ``m``, ``y``,
    ``cnt``: the max only.  ``gy`` has the destinations' rows."""
    nd, c = gy.shape
    rows = _pointnet_edge_rows(g, loops)
    gm = torch.empty((rows, c), dtype=torch.float32, device=gy.device)
    ei = g.edge_index
    saved = [m.data_ptr(), _rowmajor(m, "m"), y.data_ptr(), _rowmajor(y, "y"), cnt.data_ptr(),
             _rowmajor(cnt, "cnt", (torch.int32,))] if mode == 2 else [None, c, None, c, None, c]
    _lib.check(_lib.lib().dc_pointnet_reduce_bwd(
        ei[0].data_ptr(), ei[1].data_ptr(), g.fwd.ptr.data_ptr(), *saved, gy.data_ptr(), _rowmajor(gy, "gy"),
        gm.data_ptr(), c, mode, g.num_nodes, nd, g.num_input_edges, c, int(loops), current_stream_ptr(gy.device)),
        "dc_pointnet_reduce_bwd")
    return gm


class _PointnetPairFn(torch.autograd.Function):
    """``[x_j, pos_j - pos_i]`` per edge row: one launch forward, one backward; nothing is saved but the graph."""

    @staticmethod
    def forward(ctx, g: Optional[GraphIndex], x, pos_src, pos_dst, loops: bool, pad: bool):
        ns, nd = pos_src.size(0), pos_dst.size(0)
        f = x.size(1) if x is not None else 0
        rows = _pointnet_edge_rows(g, loops) if g is not None else 0
        ctx.g, ctx.loops, ctx.sizes = g, loops, (ns, nd, f)
        ctx.empty = rows == 0 or ns == 0 or nd == 0              # no row, or every edge names a node that is not there
        if ctx.empty:                        # nothing to launch (an empty tensor has no address)
            return pos_src.new_zeros((rows, f + 3))
        return _pointnet_pair_fwd(g, x, pos_src, pos_dst, loops, pad)

    @staticmethod
    def backward(ctx, gz):
        ns, nd, f = ctx.sizes
        want = (f > 0 and ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.needs_input_grad[3])
        if ctx.empty:
            gx, gps, gpd = gz.new_zeros((ns, f)), gz.new_zeros((ns, 3)), gz.new_zeros((nd, 3))
        else:
            gx, gps, gpd = _pointnet_pair_bwd(ctx.g, _sage_grad(gz), ns, nd, ctx.loops, want)
        return (None, gx if want[0] else None, gps if want[1] else None, gpd if want[2] else None, None, None)


class _PointnetReduceFn(torch.autograd.Function):
    """``sum`` / ``mean`` / ``max`` of edge rows per destination of a bipartite (or loops) set: one launch forward
    (``dc_edge_reduce_fwd``), one backward (``dc_pointnet_reduce_bwd``).  The max saves m, y and cnt."""

    @staticmethod
    def forward(ctx, g: Optional[GraphIndex], m, mode: int, nd: int, loops: bool):
        ctx.g, ctx.mode, ctx.loops, ctx.rows = g, mode, loops, m.size(0)
        ctx.empty = nd == 0 or m.size(0) == 0
        if ctx.empty:                        # no edge row: every destination is 0; no destination: no row
            return m.new_zeros((nd, m.size(1)))
        y, cnt = _edge_reduce_fwd(g, m, mode, nd)
        if mode == 2:
            ctx.save_for_backward(m, y, cnt)
        return y

    @staticmethod
    def backward(ctx, gy):
        if ctx.empty:
            return None, gy.new_zeros((ctx.rows, gy.size(1))), None, None, None
        m, y, cnt = ctx.saved_tensors if ctx.mode == 2 else (None, None, None)
        return None, _pointnet_reduce_bwd(ctx.g, m, y, cnt, _sage_grad(gy), ctx.mode, ctx.loops), None, None, None


def pointnet_pairs(g: Optional[GraphIndex], x_src: Optional[torch.Tensor], pos_src: torch.Tensor,
                   pos_dst: torch.Tensor, loops: bool = False, pad: Optional[bool] = None) -> torch.Tensor:
    """``z [E', F + 3]`` with ``z[q] = [x_src[j], pos_src[j] - pos_dst[i]]`` for every edge ``q = (j -> i)`` of ``g``, rows
    in the order of the ``edge_index`` the graph was built from - the per-edge input of PyG's ``PointNetConv``.
    ``g``: ``pointnet_graph(edge_index, Ns, Nd, loops)``.  ``x_src``: float32 ``[Ns, F >= 1]`` with unit inner stride (a
    column slice passes as it is) or None (``F = 0``: positions alone); ``pos_src`` ``[Ns, 3]``, ``pos_dst`` ``[Nd, 3]``:
    float32 positions as ``neighbors`` takes them (a row stride is allowed).  An edge that names a source outside
    ``[0, Ns)`` or a destination outside ``[0, Nd)`` gets a zero row.  ``loops``: one node set (``Ns == Nd == N``); ``E' =
    E + N``, row ``E + i`` is ``[x_src[i], 0, 0, 0]``.  One autograd node: the backward is one launch
    of compensated sums in the order of the sorted sets, for ``x_src``, ``pos_src`` and ``pos_dst`` - each only where it
    wants a gradient; pass the same tensor as both positions and autograd adds the two.  The edge list must stay
    unchanged until the backward has run.  No edge row, ``Ns = 0`` or ``Nd = 0``: zeros of the right shape, no launch.
    ``pad``: ``z``'s row stride rounded up to 4 floats - ``z`` is then a non-contiguous view (unit inner stride) of a buffer
    whose padding columns hold zeros; default: ``POINTNET_PAD_Z``'s rule, padded exactly where ``F % 4 == 0``."""
    from ..neighbors import _check_points
    loops = bool(loops)
    if x_src is not None:
        x_src = resolve(x_src)
        _require_cuda(x_src, "x_src")
        if x_src.dim() != 2 or x_src.dtype != torch.float32 or x_src.size(1) == 0:
            raise ValueError(f"pointnet_pairs: x_src must be a float32 [Ns, F >= 1] tensor or None, got "
                             f"{tuple(x_src.shape)} {x_src.dtype}")
    _check_points(pos_src, "pos_src")
    _check_points(pos_dst, "pos_dst")
    ns, nd = pos_src.size(0), pos_dst.size(0)
    if x_src is not None and x_src.size(0) != ns:
        raise ValueError(f"pointnet_pairs: x_src has {x_src.size(0)} rows but pos_src has {ns} points")
    if pos_dst.device != pos_src.device or (x_src is not None and x_src.device != pos_src.device):
        raise RuntimeError("pointnet_pairs: x_src, pos_src and pos_dst must be on one device")
    if loops and ns != nd:
        raise ValueError(f"pointnet_pairs: loops need one node set (Ns={ns}, Nd={nd})")
    f = x_src.size(1) if x_src is not None else 0
    pad = (ops.POINTNET_PAD_Z and f > 0 and f % 4 == 0) if pad is None else bool(pad)
    if g is None:
        if max(ns, nd) != 0:
            raise ValueError("pointnet_pairs: g may be None only without any node")
        return _PointnetPairFn.apply(None, x_src, pos_src, pos_dst, loops, pad)
    _graph_check("pointnet_pairs", g, loops, pos_src, "pos_src")
    if g.num_nodes != max(ns, nd):
        raise ValueError(f"pointnet_pairs: the graph has {g.num_nodes} rows but max(Ns, Nd) = {max(ns, nd)}")
    return _PointnetPairFn.apply(g, None if x_src is None else _edge_rows(x_src), pos_src, pos_dst, loops, pad)


def pointnet_aggregate(g: Optional[GraphIndex], m: torch.Tensor, reduce: str = "max", num_dst: Optional[int] = None,
                       loops: bool = False) -> torch.Tensor:
    """``reduce`` (``"sum"`` / ``"mean"`` / ``"max"``) per destination ``i < num_dst`` of the rows ``m[q]`` that live on the
    edge rows of ``g`` -> ``[num_dst, C]`` - ``edge_aggregate`` for a bipartite set (``g = pointnet_graph(...)``, only
    ``num_dst`` rows are reduced; default: all rows of ``g``) and for ``loops`` (``m`` has ``E + N`` rows, an input edge
    with ``src == dst`` is ignored, the mean's degree counts the loop).  Sums, the max's even split and the layouts as
    ``edge_aggregate``.  One autograd node; the backward writes every row of the gradient
    once - zeros for an ignored row - and reads the endpoints from ``g.edge_index``."""
    if not isinstance(reduce, str) or reduce not in EDGE_REDUCE_MODES:
        raise ValueError(f"pointnet_aggregate: reduce must be 'sum', 'mean' or 'max', got {reduce!r}")
    m = resolve(m)
    _require_cuda(m, "m")
    if m.dim() != 2 or m.dtype != torch.float32 or m.size(1) == 0:
        raise ValueError(f"pointnet_aggregate: m must be a float32 [E', C >= 1] tensor, got {tuple(m.shape)} {m.dtype}")
    mode, loops = EDGE_REDUCE_MODES[reduce], bool(loops)
    if g is None:
        if m.size(0) != 0 or (num_dst or 0) != 0:
            raise ValueError("pointnet_aggregate: g may be None only for an m without rows and no destination")
        return _PointnetReduceFn.apply(None, m, mode, 0, loops)
    _graph_check("pointnet_aggregate", g, loops, m, "m")
    nd = g.num_nodes if num_dst is None else int(num_dst)
    if not 0 <= nd <= g.num_nodes or (loops and nd != g.num_nodes):
        raise ValueError(f"pointnet_aggregate: num_dst = {nd} does not fit the graph's {g.num_nodes} rows"
                         f"{' (loops need all of them)' if loops else ''}")
    rows = _pointnet_edge_rows(g, loops)
    if rows != m.size(0):
        raise ValueError(f"pointnet_aggregate: m has {m.size(0)} rows but the graph has {rows} edge rows")
    return _PointnetReduceFn.apply(g, _edge_rows(m), mode, nd, loops)
