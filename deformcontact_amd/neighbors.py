"""kNN and radius graphs on the device: PyG 2.5's ``knn``, ``knn_graph``, ``radius`` and ``radius_graph`` on the HIP
kernels of ``csrc/dc_neighbors.hip`` (``dc_neighbors_fill`` / ``dc_neighbors_compact``) and, for rows of any other
width - the feature-space search of DGCNN - ``csrc/dc_neighbors_nd.hip`` (``dc_neighbors_nd_fill``).

The reference builds point-cloud graphs with ``radius_graph(pc, r, loop=False)`` / ``knn_graph(pc, k, loop=False)``
(``/root/reference/utils/pointcloud_utils.py:7-13``).  Two layers:

* ``knn_padded`` / ``radius_padded``: the capturable form.  It returns a padded ``[Nq, cap]`` int32 neighbour array
  (row ``i`` = query ``i``'s neighbours in rank order, then ``-1``) and the int32 counts, and reads nothing on the host,
  so it may be recorded in ``torch.cuda.graph``.
* The PyG-shaped functions.  They read the edge total once, as PyG does, and compact to the exact ``[2, M]`` int64
  list.  With a ``batch`` vector, ``*_graph`` also reads the graph count (PyG reads it too) and attaches the batch
  layout to the result, so ``conv(x, knn_graph(pos, k, batch))`` takes the one-launch segmented adjacency build.

Rules (the contract):

1. Positions are float32 HIP tensors ``[N, 3]`` (a row stride is allowed, the inner stride must be 1); a CPU tensor,
   float64 and ``cosine=True`` raise.  ``batch*`` are sorted int64 graph ids; a query's candidates are the points
   of its own graph.  ``num_workers`` / ``batch_size`` are accepted and ignored.  The kNN functions also take rows
   ``[N, F]`` of any other width ``F >= 1`` (features): an ``[N, 3]`` operand takes the grid search, any other width
   the exact tiled brute force of ``knn_padded_nd`` (which takes ``F = 3`` too, with the same bits).  ``radius*``
   stay three-dimensional.
2. ``d2 = ((dx*dx + dy*dy) + dz*dz)`` in fp32, ``dx = x_j - y_i``, each product and sum rounded on its own.  At
   width ``F``: ``d2 = d_0*d_0``, then ``d2 = d2 + d_c*d_c`` for ``c = 1 .. F-1`` in column order, ``d_c = x[j,c] -
   y[i,c]``, every difference, product and sum rounded on its own - for ``F = 3`` the same formula.
3. Candidates are ranked by ``(d2, j)`` ascending.  ``knn`` keeps the first ``k``.  ``radius`` keeps those with
   ``d2 < r2``, ``r2 = float32(r) * float32(r)`` rounded once, then the first ``max_num_neighbors`` by rank: under the
   cap, the nearest (PyG leaves that choice open; ``synth.radius_graph_points`` makes the same one).
4. ``loop=False`` drops ``j == i`` by index; a duplicate point ``j != i`` stays, at distance 0.
5. Output grouped by query ascending, by rank inside a query, exact size.  Empty inputs and ``k = 0`` give
   ``[2, 0]``.  No atomic order or scheduling enters the result: two calls are bit-identical.
6. ``k`` and ``max_num_neighbors`` are at most 64 (``MAX_CAP``) on this path; a larger value raises ``ValueError``.

Where PyG's own rule is unspecified (the choice under the cap, the order inside a query, a pair at exactly ``r``),
agreement with PyG is not pinned: real PyG is not part of this project's test environment.
"""
from __future__ import annotations

import operator
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from .graph import _require_cuda, current_stream_ptr

#: the most neighbours one query keeps on this path (a lane per rank)
MAX_CAP = _lib.DEFINES["DC_NEIGHBORS_MAX_CAP"]
#: columns the width-F kernel stages per pass: widths below, at and above it and its multiples take different code
#: paths, which is what the tests pick their widths by
ND_CHUNK = _lib.DEFINES["DC_NEIGHBORS_ND_CHUNK"]
_KNN, _RADIUS = _lib.DEFINES["DC_NEIGHBORS_KNN"], _lib.DEFINES["DC_NEIGHBORS_RADIUS"]
_FLOWS = ("source_to_target", "target_to_source")


def _check_points(t: Tensor, what: str) -> None:
    if not isinstance(t, Tensor):
        raise TypeError(f"{what} must be a tensor (got {type(t).__name__})")
    _require_cuda(t, what)
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32 (got {t.dtype}): distances are defined in fp32, rounded per "
                        "operation, and a float64 search would rank near-ties differently")
    if t.dim() != 2 or t.size(1) != 3:
        raise ValueError(f"{what} must be [N, 3] positions (got shape {tuple(t.shape)}): the grid search is "
                         "three-dimensional")
    if t.size(0) >= 2 ** 31 - 1:
        raise ValueError(f"{what}: {t.size(0)} points exceed int32 indexing")
    if t.size(0) > 1 and (t.stride(1) != 1 or t.stride(0) < 3):
        raise ValueError(f"{what} must have an inner stride of 1 and non-overlapping rows (got strides "
                         f"{tuple(t.stride())})")


def _ld(t: Tensor) -> int:
    return t.stride(0) if t.size(0) > 1 else 3


def _check_rows(t: Tensor, what: str) -> None:
    """``_check_points`` for the width-F search: any width ``>= 1``."""
    if not isinstance(t, Tensor):
        raise TypeError(f"{what} must be a tensor (got {type(t).__name__})")
    _require_cuda(t, what)
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32 (got {t.dtype}): distances are defined in fp32, rounded per "
                        "operation, and a float64 search would rank near-ties differently")
    if t.dim() != 2 or t.size(1) < 1:
        raise ValueError(f"{what} must be [N, F] rows of width F >= 1 (got shape {tuple(t.shape)})")
    if t.size(0) >= 2 ** 31 - 65:
        raise ValueError(f"{what}: {t.size(0)} rows exceed int32 indexing")
    if t.size(0) > 1 and (t.stride(1) != 1 or t.stride(0) < t.size(1)):
        raise ValueError(f"{what} must have an inner stride of 1 and non-overlapping rows (got strides "
                         f"{tuple(t.stride())} at width {t.size(1)})")


def _is_nd(t) -> bool:
    """Does this first operand of a kNN call take the width-F search?  A float32 device matrix of a width other than 3;
    everything else goes to the grid path, which takes ``[N, 3]`` and refuses the rest as it always has."""
    return isinstance(t, Tensor) and t.dim() == 2 and t.size(1) >= 1 and t.size(1) != 3 and t.is_cuda \
        and t.dtype == torch.float32


def _check_batch(b: Optional[Tensor], n: int, device, what: str) -> Optional[Tensor]:
    if b is None:
        return None
    if not isinstance(b, Tensor):
        raise TypeError(f"{what} must be a tensor or None (got {type(b).__name__})")
    _require_cuda(b, what)
    if b.dtype != torch.int64 or b.dim() != 1 or b.numel() != n:
        raise ValueError(f"{what} must be a sorted int64 vector of {n} graph ids (got {b.dtype} {tuple(b.shape)})")
    if b.device != device:
        raise ValueError(f"{what} is on {b.device}, the positions on {device}")
    return b.contiguous()


def _check_cap(v, what: str) -> int:
    v = operator.index(v)
    if v < 0:
        raise ValueError(f"{what} must be >= 0 (got {v})")
    if v > MAX_CAP:
        raise ValueError(f"{what}={v} exceeds {MAX_CAP}, the most neighbours per query this path keeps")
    return v


def _check_radius(r) -> float:
    r = float(r)
    if not r >= 0.0:
        raise ValueError(f"r must be >= 0 (got {r})")
    return r


def _fill(x: Tensor, y: Tensor, cap: int, r: Optional[float], batch_x, batch_y, exclude_self: bool):
    _check_points(x, "x")
    _check_points(y, "y")
    if x.device != y.device:
        raise ValueError(f"x is on {x.device}, y on {y.device}")
    dev = x.device
    nx, ny = x.size(0), y.size(0)
    batch_x = _check_batch(batch_x, nx, dev, "batch_x")
    batch_y = _check_batch(batch_y, ny, dev, "batch_y")
    nbr = torch.empty(ny, cap, dtype=torch.int32, device=dev)
    counts = torch.empty(ny, dtype=torch.int32, device=dev)
    L = _lib.lib()
    nbytes = int(L.dc_neighbors_workspace_bytes(nx, ny))
    if nbytes < 0:
        raise ValueError(f"neighbour search: unsupported sizes nx={nx}, ny={ny}")
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _lib.check(L.dc_neighbors_fill(
        x.data_ptr(), _ld(x), nx, None if batch_x is None else batch_x.data_ptr(),
        y.data_ptr(), _ld(y), ny, None if batch_y is None else batch_y.data_ptr(),
        _KNN if r is None else _RADIUS, 0.0 if r is None else r, cap, int(bool(exclude_self)),
        nbr.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes, current_stream_ptr(dev)), "dc_neighbors_fill")
    return nbr, counts


def knn_padded(x: Tensor, y: Tensor, k: int, batch_x: Optional[Tensor] = None, batch_y: Optional[Tensor] = None,
               exclude_self: bool = False) -> Tuple[Tensor, Tensor]:
    """The ``k`` nearest points of ``x`` to every point of ``y`` (rules 1-6 of the module docstring), without a host
    read: ``(nbr [Ny, k] int32, counts [Ny] int32)``; row ``i`` of ``nbr`` holds ``counts[i]`` indices into ``x`` in
    rank order, then ``-1``.  ``exclude_self`` drops ``j == i`` (``knn_graph(loop=False)``)."""
    if _is_nd(x):
        return knn_padded_nd(x, y, k, batch_x, batch_y, exclude_self)
    return _fill(x, y, _check_cap(k, "k"), None, batch_x, batch_y, exclude_self)


def knn_padded_nd(x: Tensor, y: Tensor, k: int, batch_x: Optional[Tensor] = None, batch_y: Optional[Tensor] = None,
                  exclude_self: bool = False) -> Tuple[Tensor, Tensor]:
    """``knn_padded`` for rows of any width ``F >= 1`` (3 included: the grid path's bits): ``x [Nx, F]``, ``y [Ny,
    F]`` float32 on one HIP device, unit inner stride, non-overlapping rows.  An exact brute force per graph on the
    kernel of ``csrc/dc_neighbors_nd.hip`` - ``Ny x n_graph x F`` subtract / multiply / add triples, so it is the grid
    path that wins on large three-dimensional clouds.  Same result layout, no host read, no workspace: capturable."""
    cap = _check_cap(k, "k")
    _check_rows(x, "x")
    _check_rows(y, "y")
    if x.device != y.device:
        raise ValueError(f"x is on {x.device}, y on {y.device}")
    if x.size(1) != y.size(1):
        raise ValueError(f"x and y must have the same width (got {x.size(1)} and {y.size(1)} columns)")
    dev, f = x.device, x.size(1)
    nx, ny = x.size(0), y.size(0)
    batch_x = _check_batch(batch_x, nx, dev, "batch_x")
    batch_y = _check_batch(batch_y, ny, dev, "batch_y")
    nbr = torch.empty(ny, cap, dtype=torch.int32, device=dev)
    counts = torch.empty(ny, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().dc_neighbors_nd_fill(
        x.data_ptr(), x.stride(0) if nx > 1 else f, nx, None if batch_x is None else batch_x.data_ptr(),
        y.data_ptr(), y.stride(0) if ny > 1 else f, ny, None if batch_y is None else batch_y.data_ptr(),
        f, cap, int(bool(exclude_self)), nbr.data_ptr(), counts.data_ptr(), current_stream_ptr(dev)),
        "dc_neighbors_nd_fill")
    return nbr, counts


def radius_padded(x: Tensor, y: Tensor, r: float, batch_x: Optional[Tensor] = None,
                  batch_y: Optional[Tensor] = None, max_num_neighbors: int = 32,
                  exclude_self: bool = False) -> Tuple[Tensor, Tensor]:
    """The nearest (at most ``max_num_neighbors``) points of ``x`` with ``d2 < float32(r)**2`` for every point of
    ``y``, without a host read: ``(nbr [Ny, max_num_neighbors] int32, counts [Ny] int32)`` as ``knn_padded``."""
    return _fill(x, y, _check_cap(max_num_neighbors, "max_num_neighbors"), _check_radius(r), batch_x, batch_y,
                 exclude_self)


def _edges(nbr: Tensor, counts: Tensor, query_row: int, batch: Optional[Tensor] = None) -> Tensor:
    """Compact a padded result to the exact ``[2, M]`` int64 edge list: row ``query_row`` holds the query, the other
    the neighbour.  One host read of the total (two with ``batch``: the graph count, then the node and edge offsets
    of the graphs, which are attached to the result as ``data.Batch`` attaches them)."""
    dev = counts.device
    ny, cap = nbr.shape
    seg = None
    if batch is None:
        m = int(counts.sum()) if ny > 0 and cap > 0 else 0
    else:
        nb = int(batch[-1]) + 1
        if nb < 1:
            raise ValueError("batch must hold sorted graph ids >= 0")
        ptr = torch.searchsorted(batch, torch.arange(nb + 1, dtype=torch.int64, device=dev))
        offs = torch.zeros(ny + 1, dtype=torch.int64, device=dev)
        offs[1:] = counts.cumsum(0)
        host = torch.cat([ptr, offs[ptr]]).tolist()
        seg = (tuple(host[:nb + 1]), tuple(host[nb + 1:]))
        m = seg[1][-1]
    out = torch.empty(2, m, dtype=torch.int64, device=dev)
    if m > 0:
        L = _lib.lib()
        nbytes = int(L.dc_neighbors_compact_workspace_bytes(ny))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _lib.check(L.dc_neighbors_compact(nbr.data_ptr(), cap, counts.data_ptr(), ny, query_row, out.data_ptr(), m,
                                          ws.data_ptr(), nbytes, current_stream_ptr(dev)), "dc_neighbors_compact")
    if seg is not None:
        out._dc_segments = (seg, out._version)          # graph.edge_layout: the one-launch segmented build
    return out


def _empty(x: Tensor) -> Tensor:
    return torch.empty(2, 0, dtype=torch.int64, device=x.device)


def _check_flow(flow: str) -> int:
    if flow not in _FLOWS:
        raise ValueError(f"flow must be one of {_FLOWS} (got {flow!r})")
    return 1 if flow == "source_to_target" else 0        # the output row of the centre (the query)


def _no_cosine(cosine: bool) -> None:
    if cosine:
        raise ValueError("cosine=True is not supported: this path ranks by the fp32 squared Euclidean distance")


def knn(x: Tensor, y: Tensor, k: int, batch_x: Optional[Tensor] = None, batch_y: Optional[Tensor] = None,
        cosine: bool = False, num_workers: int = 1, batch_size: Optional[int] = None) -> Tensor:
    """PyG ``knn``: for every point of ``y`` its ``k`` nearest points of ``x`` in the same graph.  Returns
    ``[2, M]`` int64: row 0 indexes ``y`` (the query), row 1 indexes ``x``.  ``[N, 3]`` positions or ``[N, F]``
    feature rows.  Rules: module docstring."""
    _no_cosine(cosine)
    nbr, counts = knn_padded(x, y, k, batch_x, batch_y)
    return _edges(nbr, counts, 0)


def knn_graph(x: Tensor, k: int, batch: Optional[Tensor] = None, loop: bool = False,
              flow: str = "source_to_target", cosine: bool = False, num_workers: int = 1,
              batch_size: Optional[int] = None) -> Tensor:
    """PyG ``knn_graph``: every point's ``k`` nearest points of its graph.  ``flow="source_to_target"``:
    ``edge_index[0]`` is the neighbour, ``edge_index[1]`` the centre; ``"target_to_source"`` swaps the rows.
    ``loop=False`` drops ``j == i``.  ``[N, 3]`` positions or ``[N, F]`` feature rows (the graph DGCNN rebuilds in
    every layer).  Rules: module docstring."""
    _no_cosine(cosine)
    query_row = _check_flow(flow)
    nbr, counts = knn_padded(x, x, k, batch, batch, exclude_self=not loop)
    if x.size(0) == 0:
        return _empty(x)
    return _edges(nbr, counts, query_row, None if batch is None else batch.contiguous())


def radius(x: Tensor, y: Tensor, r: float, batch_x: Optional[Tensor] = None, batch_y: Optional[Tensor] = None,
           max_num_neighbors: int = 32, num_workers: int = 1, batch_size: Optional[int] = None) -> Tensor:
    """PyG ``radius``: for every point of ``y`` the nearest (at most ``max_num_neighbors``) points of ``x`` in the
    same graph with ``d2 < r*r``.  Returns ``[2, M]`` int64: row 0 indexes ``y``, row 1 indexes ``x``."""
    nbr, counts = radius_padded(x, y, r, batch_x, batch_y, max_num_neighbors)
    return _edges(nbr, counts, 0)


def radius_graph(x: Tensor, r: float, batch: Optional[Tensor] = None, loop: bool = False,
                 max_num_neighbors: int = 32, flow: str = "source_to_target", num_workers: int = 1,
                 batch_size: Optional[int] = None) -> Tensor:
    """PyG ``radius_graph``: every point's nearest (at most ``max_num_neighbors``) points of its graph with
    ``d2 < r*r``; rows as ``knn_graph``.  Rules: module docstring."""
    query_row = _check_flow(flow)
    nbr, counts = radius_padded(x, x, r, batch, batch, max_num_neighbors, exclude_self=not loop)
    if x.size(0) == 0:
        return _empty(x)
    return _edges(nbr, counts, query_row, None if batch is None else batch.contiguous())
