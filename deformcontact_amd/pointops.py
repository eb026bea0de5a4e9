"""Point-set sampling, transfer and pooling on the device: PyG 2.5's ``fps`` and ``knn_interpolate`` on the HIP kernels
of ``csrc/dc_pointops.hip`` (``dc_fps`` / ``dc_knn_interpolate_fwd`` / ``dc_knn_interpolate_bwd``), and ``global_add_pool``
/ ``global_mean_pool`` / ``global_max_pool`` on those of ``csrc/dc_pointnet.hip`` (``dc_pool_fwd`` / ``dc_pool_bwd``).

``fps`` is the sampling step of PointNet++ set abstraction (the grouping step is ``neighbors.radius``);
``knn_interpolate`` is its feature propagation: node rows of one point set carried onto another by
inverse-squared-distance weights over the ``k`` nearest neighbours, on the padded result of ``neighbors.knn_padded``.

Rules (the contract).  Positions follow ``neighbors._check_points`` and distances are rule 2 of
``neighbors``: ``d2 = ((dx*dx + dy*dy) + dz*dz)`` in fp32, each operation rounded on its own.  Inputs are taken to be
finite.

``fps(x, batch=None, ratio=0.5, random_start=True, batch_size=None, ptr=None) -> int64 [M]``

1. ``batch`` is a sorted int64 ``[N]`` vector of graph ids or ``ptr`` an int64 ``[B+1]`` vector of node offsets, not
   both.  ``ratio`` is a Python float in ``(0, 1]``.
2. Graph ``g`` with ``n_g`` nodes gives ``m_g = ceil(float32(n_g) * float32(ratio))`` picks, the product rounded once in
   fp32 as torch_cluster computes it (``fps_count``; never more than ``n_g``).  A graph id without nodes gives none.
3. Per graph with the nodes ``[a, b)``: ``p_0 = start``, ``dist[j] = d2(j, p_0)``; for ``t = 1 .. m_g - 1``, ``p_t`` is
   the ``j`` with the largest ``dist[j]``, the LOWEST ``j`` among equals, then ``dist[j] = min(dist[j], d2(j, p_t))``.
   Once every distinct point is taken all distances are 0 and the rule keeps returning the graph's first node.
4. ``random_start=False``: ``start = a``.  ``True``: ``start = a + floor(u_g * n_g)`` with ``u_g`` drawn on the device by
   torch's generator, one draw per graph, without a host read.
5. Output: global node indices, graphs in ascending order, pick order inside a graph (PyG does not sort them either).
6. With ``batch=None`` and ``ptr=None`` the call reads nothing on the host and may be recorded in
   ``torch.cuda.graph``.  With a batch it reads the node offsets of the graphs once to size the output (and the graph
   count before that, unless ``batch_size`` is given).
7. One workgroup per graph.  Graphs of up to ``FPS_RESIDENT_POINTS`` points keep positions and distances in registers;
   a launch whose largest graph is bigger keeps them in a workspace of 16 bytes per node.

Where PyG's own rule is unspecified - which of several equally far points is taken - agreement with PyG is not pinned.

``knn_interpolate(x, pos_x, pos_y, batch_x=None, batch_y=None, k=3, num_workers=1) -> float32 [Ny, F]``

1. ``x`` is float32 ``[Nx, F >= 1]`` with unit inner stride (a column slice passes as it is; the deferred result of a
   conv call is resolved).  Positions and batches as for ``knn``; ``k <= neighbors.MAX_CAP``.
2. Neighbours: ``neighbors.knn_padded(pos_x, pos_y, k, batch_x, batch_y)`` under ``no_grad``.
3. Per query ``i``, over the ranks ``r < counts[i]`` with ``j = nbr[i, r]``: ``w = 1.0f / max(d2, 1e-16f)``;
   ``num[c] = num[c] + w * x[j, c]`` and ``den = den + w`` from 0 in rank order, product and sum rounded separately;
   ``y[i, c] = num[c] / den``.  A query without a neighbour gets a row of ZEROS - PyG returns NaN there (0/0): the one
   deliberate difference.
4. Only ``x`` receives a gradient (PyG computes neighbours and weights under ``no_grad``):
   ``g_x[j, c]`` = the compensated sum over the slots ``(i, r)`` with ``nbr[i, r] == j``, in ascending ``(i, r)`` order,
   of ``w_ir * (g_y[i, c] / den_i)``; a source no query selected gets a zero row.  The by-source list of slots is built
   on the device (a stable sort of the flattened neighbour array), in the backward only.
5. No host read anywhere: forward and backward may be recorded in ``torch.cuda.graph``.  No float atomics: two runs
   give the same bits.

``global_add_pool(x, batch, size=None)``, ``global_mean_pool``, ``global_max_pool`` ``-> float32 [B, C]``

1. ``x`` is float32 ``[N, C >= 1]`` with unit inner stride (a column slice passes as it is; a deferred result is
   resolved).  ``batch`` is a sorted int64 ``[N]`` vector of graph ids; ``batch=None`` is one graph and gives ``[1, C]``
   (``size`` is then ignored, as in PyG).
2. ``size=None`` reads the graph count ``batch[-1] + 1`` once on the host, as ``fps`` does.  With ``size`` the call
   reads nothing on the host and may be recorded in ``torch.cuda.graph``; rows whose id is not below ``size`` take no
   part and get a zero gradient.  The row offsets of the graphs are made on the device (``torch.searchsorted``).
3. A graph id without rows gets 0.  The mean divides the sum by ``float(rows)`` (a true division).  The max sends its
   gradient in equal shares to ALL rows that attain it; an int32 count per output is saved.
4. Order of the sums: one workgroup per (graph, column block) of 16 slots; slot ``s`` adds the
   rows ``a + s, a + s + 16, ...`` in ascending order from 0, and the 16 partial sums are added in slot order, all plain
   fp32 - a numpy loop reproduces every bit.  Per graph it stays one workgroup per column block: a cooperative form
   that spreads ONE huge cloud over the device is not built (as for ``fps``).
5. Each function is one autograd node with one launch forward and one backward; no float atomics.
"""
from __future__ import annotations

import operator
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib, neighbors
from .deferred import resolve
from .graph import _require_cuda, current_stream_ptr

#: the most points of one graph that ``fps`` keeps in registers; a launch whose largest graph has more takes the
#: workspace kernel
FPS_RESIDENT_POINTS = _lib.DEFINES["DC_FPS_RESIDENT_POINTS"]


def fps_count(n, ratio: float):
    """``m = ceil(float32(n) * float32(ratio))``, the product rounded once in fp32, at most ``n``: the picks of a graph
    of ``n`` nodes.  ``n``: an int or an integer array."""
    m = np.ceil(np.asarray(n).astype(np.float32) * np.float32(ratio)).astype(np.int64)
    m = np.minimum(m, np.asarray(n, dtype=np.int64))
    return int(m) if m.ndim == 0 else m


def _check_ratio(ratio) -> float:
    if isinstance(ratio, Tensor):
        raise TypeError("fps: ratio must be a Python float (a tensor ratio would need a host read per call)")
    ratio = float(ratio)
    if not (0.0 < ratio <= 1.0):
        raise ValueError(f"fps: ratio must lie in (0, 1] (got {ratio})")
    return ratio


def _graph_offsets(x: Tensor, batch: Optional[Tensor], batch_size, ptr: Optional[Tensor]):
    """``(ptr tensor int64 [B+1] on the device, its host copy)``: the ONE host read of the node counts."""
    n, dev = x.size(0), x.device
    if ptr is not None:
        if not isinstance(ptr, Tensor):
            raise TypeError(f"fps: ptr must be a tensor or None (got {type(ptr).__name__})")
        _require_cuda(ptr, "ptr")
        if ptr.dtype != torch.int64 or ptr.dim() != 1 or ptr.numel() < 1 or ptr.device != dev:
            raise ValueError(f"fps: ptr must be an int64 [B+1] vector of node offsets on {dev} (got {ptr.dtype} "
                             f"{tuple(ptr.shape)} on {ptr.device})")
        ptr = ptr.contiguous()
    else:
        batch = neighbors._check_batch(batch, n, dev, "batch")
        nb = operator.index(batch_size) if batch_size is not None else int(batch[-1]) + 1
        if nb < 1:
            raise ValueError("fps: batch must hold sorted graph ids >= 0")
        ptr = torch.searchsorted(batch, torch.arange(nb + 1, dtype=torch.int64, device=dev))
    host = np.asarray(ptr.tolist(), dtype=np.int64)
    if host[0] != 0 or host[-1] != n or (np.diff(host) < 0).any():
        raise ValueError(f"fps: the node offsets must rise from 0 to N={n} (got {host[:8].tolist()}"
                         f"{'...' if host.size > 8 else ''}; is batch sorted, with every id < batch_size?)")
    return ptr, host


def fps(x: Tensor, batch: Optional[Tensor] = None, ratio: float = 0.5, random_start: bool = True,
        batch_size: Optional[int] = None, ptr: Optional[Tensor] = None) -> Tensor:
    """PyG ``fps``: farthest point sampling of every graph, ``ceil(ratio * n_g)`` points each.  Returns the int64
    ``[M]`` global indices of the picks, graphs ascending, pick order inside a graph.  Rules: module docstring."""
    ratio = _check_ratio(ratio)
    if batch is not None and ptr is not None:
        raise ValueError("fps: give batch or ptr, not both")
    neighbors._check_points(x, "x")
    n, dev = x.size(0), x.device
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=dev)
    L = _lib.lib()
    if batch is None and ptr is None:
        dptr = doptr = None
        nb, max_n, m = 1, n, fps_count(n, ratio)
        start = (torch.rand(1, device=dev) * n).to(torch.int64).clamp_(max=n - 1) if random_start else None
    else:
        dptr, host = _graph_offsets(x, batch, batch_size, ptr)
        counts = np.diff(host)
        nb, max_n = counts.size, int(counts.max(initial=0))
        optr = np.zeros(nb + 1, dtype=np.int64)
        np.cumsum(fps_count(counts, ratio), out=optr[1:])
        m = int(optr[-1])
        doptr = torch.from_numpy(optr).to(dev)
        start = None
        if random_start:
            cnt = dptr[1:] - dptr[:-1]
            off = (torch.rand(nb, device=dev) * cnt.to(torch.float32)).to(torch.int64)
            start = dptr[:-1] + torch.minimum(off, (cnt - 1).clamp_(min=0))
    out = torch.empty(m, dtype=torch.int64, device=dev)
    if m == 0:
        return out
    nbytes = int(L.dc_fps_workspace_bytes(n, max_n))
    if nbytes < 0:
        raise ValueError(f"fps: unsupported sizes N={n}, largest graph {max_n}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    _lib.check(L.dc_fps(x.data_ptr(), neighbors._ld(x), n, None if dptr is None else dptr.data_ptr(),
                        None if doptr is None else doptr.data_ptr(), nb, max_n,
                        None if start is None else start.data_ptr(), out.data_ptr(), m,
                        None if ws is None else ws.data_ptr(), nbytes, current_stream_ptr(dev)), "dc_fps")
    return out


def _by_source(nbr: Tensor, nx: int):
    """The slots ``s = i*k + r`` of ``nbr`` grouped by the source they name, ascending inside a group:
    ``(ptr int64 [nx+1] into slots, slots int64 [Ny*k])`` - the padding (-1) sorts in front of ``ptr[0]``.  On the
    device, no host read; the sort is stable, so the result does not depend on scheduling."""
    key, slots = torch.sort(nbr.reshape(-1), stable=True)
    ptr = torch.searchsorted(key, torch.arange(nx + 1, dtype=key.dtype, device=key.device))
    return ptr.contiguous(), slots.contiguous()


def _grad_rows(g: Tensor) -> Tensor:
    """The incoming gradient with unit inner stride and rows that do not overlap (``layers.sage._sage_grad``)."""
    if g.stride(1) != 1:
        g = g.contiguous()
    return g if g.size(0) <= 1 or g.stride(0) >= g.size(1) else g.contiguous()


def _ldf(t: Tensor) -> int:
    return t.stride(0) if t.size(0) > 1 else t.size(1)


class _KnnInterpolateFn(torch.autograd.Function):
    """One launch forward; with a gradient wanted it also stores ``w`` and ``den``, and the backward is the by-source
    list (torch, on the device) and one launch.  The positions get no gradient."""

    @staticmethod
    def forward(ctx, x, pos_x, pos_y, nbr, counts):
        nx, f = x.shape
        ny, k = nbr.shape
        ctx.shape, ctx.launched = (nx, ny, k, f), False
        y = torch.empty(ny, f, dtype=torch.float32, device=x.device)
        if ny == 0 or nx == 0 or k == 0:
            return y.zero_()
        want = ctx.needs_input_grad[0]
        w = torch.empty(ny, k, dtype=torch.float32, device=x.device) if want else None
        den = torch.empty(ny, dtype=torch.float32, device=x.device) if want else None
        _lib.check(_lib.lib().dc_knn_interpolate_fwd(
            x.data_ptr(), _ldf(x), pos_x.data_ptr(), neighbors._ld(pos_x), pos_y.data_ptr(), neighbors._ld(pos_y),
            nbr.data_ptr(), counts.data_ptr(), k, y.data_ptr(), f, None if w is None else w.data_ptr(),
            None if den is None else den.data_ptr(), nx, ny, f, current_stream_ptr(x.device)),
            "dc_knn_interpolate_fwd")
        if want:
            ctx.launched = True
            ctx.save_for_backward(nbr, w, den)
        return y

    @staticmethod
    def backward(ctx, gy):
        nx, ny, k, f = ctx.shape
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        if not ctx.launched:
            return gy.new_zeros(nx, f), None, None, None, None
        nbr, w, den = ctx.saved_tensors
        gy = _grad_rows(gy)
        ptr, slots = _by_source(nbr, nx)
        gx = torch.empty(nx, f, dtype=torch.float32, device=gy.device)
        _lib.check(_lib.lib().dc_knn_interpolate_bwd(
            ptr.data_ptr(), slots.data_ptr(), w.data_ptr(), den.data_ptr(), gy.data_ptr(), _ldf(gy), gx.data_ptr(), f,
            k, nx, ny, f, current_stream_ptr(gy.device)), "dc_knn_interpolate_bwd")
        return gx, None, None, None, None


def _feature_rows(t: Tensor) -> Tensor:
    """unit inner stride and rows that do not overlap; a column slice passes as it is (``_host._rows``)"""
    if (t.size(1) > 1 and t.stride(1) != 1) or (t.size(0) > 1 and t.stride(0) < t.size(1)):
        return t.contiguous()
    return t


def knn_interpolate(x: Tensor, pos_x: Tensor, pos_y: Tensor, batch_x: Optional[Tensor] = None,
                    batch_y: Optional[Tensor] = None, k: int = 3, num_workers: int = 1) -> Tensor:
    """PyG ``knn_interpolate`` (PointNet++ feature propagation): the rows of ``x`` (at ``pos_x``) carried onto the points
    ``pos_y`` by inverse-squared-distance weights over the ``k`` nearest points of the same graph.  Returns float32
    ``[Ny, F]``; a query without a neighbour gets a row of zeros.  Only ``x`` receives a gradient.  Rules: module
    docstring."""
    x = resolve(x)
    if not isinstance(x, Tensor):
        raise TypeError(f"knn_interpolate: x must be a tensor (got {type(x).__name__})")
    _require_cuda(x, "x")
    if x.dtype != torch.float32 or x.dim() != 2 or x.size(1) == 0:
        raise ValueError(f"knn_interpolate: x must be a float32 [Nx, F >= 1] tensor, got {tuple(x.shape)} {x.dtype}")
    k = neighbors._check_cap(k, "k")
    neighbors._check_points(pos_x, "pos_x")
    if pos_x.size(0) != x.size(0):
        raise ValueError(f"knn_interpolate: x has {x.size(0)} rows but pos_x has {pos_x.size(0)} points")
    if x.device != pos_x.device:
        raise ValueError(f"knn_interpolate: x is on {x.device}, the positions on {pos_x.device}")
    with torch.no_grad():
        nbr, counts = neighbors.knn_padded(pos_x, pos_y, k, batch_x, batch_y)
    return _KnnInterpolateFn.apply(_feature_rows(x), pos_x, pos_y, nbr, counts)


#: the rows of one graph are dealt to this many slots of a workgroup (dc_pointnet.hip kPoolSlots): the order of the sums
POOL_SLOTS = 16
_POOL_MODES = {"add": 0, "mean": 1, "max": 2}


class _GlobalPoolFn(torch.autograd.Function):
    """One launch forward, one backward.  ``batch`` and the graph offsets are saved for the backward (autograd's version
    check covers them); the max also saves ``x``, ``y`` and the tie counts."""

    @staticmethod
    def forward(ctx, x, batch, ptr, nb: int, mode: int):
        n, c = x.shape
        ctx.mode, ctx.nb, ctx.shape = mode, nb, (n, c)
        y = torch.empty(nb, c, dtype=torch.float32, device=x.device)
        if nb == 0:
            return y
        cnt = torch.empty(nb, c, dtype=torch.int32, device=x.device) if mode == 2 else None
        _lib.check(_lib.lib().dc_pool_fwd(None if ptr is None else ptr.data_ptr(), x.data_ptr() if n else None, _ldf(x),
                                          y.data_ptr(), c, None if cnt is None else cnt.data_ptr(), c, mode, n, nb, c,
                                          current_stream_ptr(x.device)), "dc_pool_fwd")
        ctx.save_for_backward(batch, ptr, *((x, y, cnt) if mode == 2 else (None, None, None)))
        return y

    @staticmethod
    def backward(ctx, gy):
        n, c = ctx.shape
        if n == 0 or ctx.nb == 0:
            return gy.new_zeros(n, c), None, None, None, None
        batch, ptr, x, y, cnt = ctx.saved_tensors
        gy = _grad_rows(gy)
        gx = torch.empty(n, c, dtype=torch.float32, device=gy.device)
        p = lambda t: None if t is None else t.data_ptr()
        _lib.check(_lib.lib().dc_pool_bwd(p(batch), p(ptr), p(x), _ldf(x) if x is not None else c, p(y), c, p(cnt),
                                          c, gy.data_ptr(), _ldf(gy), gx.data_ptr(), c, ctx.mode, n, ctx.nb, c,
                                          current_stream_ptr(gy.device)), "dc_pool_bwd")
        return gx, None, None, None, None


def _global_pool(who: str, x: Tensor, batch: Optional[Tensor], size, mode: str) -> Tensor:
    x = resolve(x)
    if not isinstance(x, Tensor):
        raise TypeError(f"{who}: x must be a tensor (got {type(x).__name__})")
    if x.dtype != torch.float32 or x.dim() != 2 or x.size(1) == 0:
        raise ValueError(f"{who}: x must be a float32 [N, C >= 1] tensor, got {tuple(x.shape)} {x.dtype}")
    if batch is not None and isinstance(batch, Tensor) and (batch.dtype != torch.int64 or batch.dim() != 1
                                                              or batch.numel() != x.size(0)):
        raise ValueError(f"{who}: batch must be a sorted int64 vector of {x.size(0)} graph ids (got {batch.dtype} "
                         f"{tuple(batch.shape)})")
    if size is not None:
        size = operator.index(size)
        if size < 0:
            raise ValueError(f"{who}: size must be >= 0 (got {size})")
    _require_cuda(x, "x")
    batch = neighbors._check_batch(batch, x.size(0), x.device, "batch")
    x = _feature_rows(x)
    if batch is None:
        return _GlobalPoolFn.apply(x, None, None, 1, _POOL_MODES[mode])
    if size is None:
        size = int(batch[-1]) + 1 if batch.numel() else 0        # the one host read
    ptr = torch.searchsorted(batch, torch.arange(size + 1, dtype=torch.int64, device=x.device))
    return _GlobalPoolFn.apply(x, batch, ptr, size, _POOL_MODES[mode])


def global_add_pool(x: Tensor, batch: Optional[Tensor], size: Optional[int] = None) -> Tensor:
    """PyG ``global_add_pool``: the sum of the rows of every graph, float32 ``[B, C]``.  Rules: module docstring."""
    return _global_pool("global_add_pool", x, batch, size, "add")


def global_mean_pool(x: Tensor, batch: Optional[Tensor], size: Optional[int] = None) -> Tensor:
    """PyG ``global_mean_pool``: the mean of the rows of every graph, float32 ``[B, C]``; a graph without rows gets 0.
    Rules: module docstring."""
    return _global_pool("global_mean_pool", x, batch, size, "mean")


def global_max_pool(x: Tensor, batch: Optional[Tensor], size: Optional[int] = None) -> Tensor:
    """PyG ``global_max_pool``: the maximum per column of the rows of every graph, float32 ``[B, C]``; a graph without
    rows gets 0; the gradient goes in equal shares to all rows that attain the maximum.  Rules: module docstring."""
    return _global_pool("global_max_pool", x, batch, size, "max")
