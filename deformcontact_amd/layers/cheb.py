"""ChebConv's basis on the fused recurrence hop."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from .._host import _grad_layout, _ptr, _rowmajor
from ..deferred import resolve
from ..graph import GraphIndex, SortedAdjacency, _require_cuda, current_stream_ptr


# --------------------------------------------------------------------------- #
# ChebConv (dc_cheb.hip): the Chebyshev basis [Tx_0 | ... | Tx_{K-1}] of the scaled Laplacian as ONE autograd node.
# Every recurrence step - the hop, the diagonal term, the doubling and the "- Tx_{k-2}" - is one launch; the backward
# is the adjoint recurrence over the by-source set, K - 1 launches on a private copy of the slab's gradient.
# --------------------------------------------------------------------------- #
CHEB_MODES = {"sym": 0, "rw": 1}


def cheb_diagonal(lam: float) -> float:
    """``b = 2 / lambda_max - 1``: the diagonal term of the scaled Laplacian, the same for every node."""
    return 2.0 / lam - 1.0


def _cheb_norm(g: GraphIndex, mode: int, lam: float):
    """-> (wl_fwd, wl_bwd): ``(2 * -w) / lam`` per slot of the by-destination and of the by-source set, 0 for a self
    loop; ``w`` from the out-degrees over the non-loop edges (``dc_cheb_norm``: two launches)."""
    dev, cap, n = g.device, max(g.capacity, 1), max(g.num_nodes, 1)
    wl_fwd, wl_bwd, dinv = torch.empty(2 * cap + n, dtype=torch.float32, device=dev).split((cap, cap, n))
    _lib.check(_lib.lib().dc_cheb_norm(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), g.bwd.ptr.data_ptr(),
                                       g.bwd.other.data_ptr(), mode, lam, dinv.data_ptr(), wl_fwd.data_ptr(),
                                       wl_bwd.data_ptr(), g.num_nodes, current_stream_ptr(dev)), "dc_cheb_norm")
    return wl_fwd, wl_bwd


def _cheb_hop(adj: SortedAdjacency, wl: torch.Tensor, x: torch.Tensor, y: torch.Tensor, b: float, k: int, c: int,
              z: Optional[torch.Tensor] = None, z2: Optional[torch.Tensor] = None,
              y2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One recurrence step (``dc_cheb_hop``): ``y = k (sum_p wl[p] x[other[p]] + b x) + c z`` and, with ``y2``,
    ``y2 = z2 - x``.  Every operand a row-major (possibly column-sliced) ``[N, F]`` view; ``y`` may be ``z`` and ``y2``
    may be ``z2``, neither may be ``x``."""
    n, f = x.shape
    for name, t in (("y", y), ("z", z), ("z2", z2), ("y2", y2)):
        if t is not None and t.shape != x.shape:
            raise ValueError(f"cheb hop: {name} shape mismatch")
    if (c != 0) != (z is not None) or (y2 is None) != (z2 is None):
        raise ValueError("cheb hop: z goes with c != 0, z2 with y2")
    if adj.ptr.numel() != n + 1:
        raise ValueError(f"cheb hop: x has {n} rows but the graph has {adj.ptr.numel() - 1} nodes")

    def ld(t, what):
        return _rowmajor(t, what) if t is not None else 0
    _lib.check(_lib.lib().dc_cheb_hop(adj.ptr.data_ptr(), adj.other.data_ptr(), wl.data_ptr(), x.data_ptr(), ld(x, "x"),
                                      _ptr(z), ld(z, "z"), y.data_ptr(), ld(y, "y"), _ptr(z2), ld(z2, "z2"), _ptr(y2),
                                      ld(y2, "y2"), b, k, c, n, f, current_stream_ptr(x.device)), "dc_cheb_hop")
    return y


class _ChebBasisFn(torch.autograd.Function):
    """``[Tx_0 | ... | Tx_{K-1}]``: a copy of x and K - 1 step launches forward; backward K - 1 launches of the adjoint
    recurrence.  Saved: the two weight arrays (recomputed on every forward: a rebuilt adjacency is followed), nothing
    of the features - the recurrence is linear."""

    @staticmethod
    def forward(ctx, g: Optional[GraphIndex], x, k: int, mode: int, lam: float):
        n, f = x.shape
        ctx.g, ctx.k, ctx.b, ctx.f = g, k, cheb_diagonal(lam), f
        slab = torch.empty((n, k * f), dtype=torch.float32, device=x.device)
        if n == 0:
            return slab                          # no rows: nothing to launch (an empty tensor has no address)
        slab[:, :f] = x
        if k == 1:
            return slab
        wl_fwd, ctx.wl_bwd = _cheb_norm(g, mode, lam)
        blk = [slab[:, i * f:(i + 1) * f] for i in range(k)]
        _cheb_hop(g.fwd, wl_fwd, blk[0], blk[1], ctx.b, 1, 0)
        for i in range(2, k):
            _cheb_hop(g.fwd, wl_fwd, blk[i - 1], blk[i], ctx.b, 2, -1, z=blk[i - 2])
        return slab

    @staticmethod
    def backward(ctx, gslab):
        k, f = ctx.k, ctx.f
        if gslab.size(0) == 0:
            return None, gslab.new_zeros((0, f)), None, None, None
        if k == 1:
            return None, _grad_layout(gslab, 0), None, None, None
        # a private copy: the steps below update it in place, and the gradient autograd handed in is not ours to write
        grad = _grad_layout(gslab, 0)
        if grad.data_ptr() == gslab.data_ptr():
            grad = grad.clone()
        blk = [grad[:, i * f:(i + 1) * f] for i in range(k)]
        g, wl = ctx.g, ctx.wl_bwd
        for i in range(k - 1, 1, -1):            # G_{i-1} += 2 L^T G_i  and  G_{i-2} -= G_i, one launch
            _cheb_hop(g.bwd, wl, blk[i], blk[i - 1], ctx.b, 2, 1, z=blk[i - 1], z2=blk[i - 2], y2=blk[i - 2])
        _cheb_hop(g.bwd, wl, blk[1], blk[0], ctx.b, 1, 1, z=blk[0])          # G_0 += L^T G_1
        return None, blk[0], None, None, None


def cheb_lambda(lambda_max, what: str = "cheb_basis") -> float:
    """``lambda_max`` as the Python float the kernels take: None -> 2.0; a tensor or a value <= 0 raises."""
    if lambda_max is None:
        return 2.0
    if isinstance(lambda_max, torch.Tensor):
        raise NotImplementedError(f"{what}: a tensor lambda_max (per-graph values included) is not supported; pass a "
                                  "Python number")
    if isinstance(lambda_max, bool) or not isinstance(lambda_max, (int, float)):
        raise TypeError(f"{what}: lambda_max must be None or a Python number, got {type(lambda_max).__name__}")
    if not lambda_max > 0:
        raise ValueError(f"{what}: lambda_max must be > 0, got {lambda_max}")
    return float(lambda_max)


def cheb_basis(g: Optional[GraphIndex], x: torch.Tensor, K: int, normalization: str = "sym",
               lambda_max=None) -> torch.Tensor:
    """The Chebyshev basis ``[Tx_0 | Tx_1 | ... | Tx_{K-1}]`` ``[N, K*F]`` of PyG's ``ChebConv``: ``Tx_0 = x``,
    ``Tx_1 = L^ x``, ``Tx_k = 2 L^ Tx_{k-1} - Tx_{k-2}`` with ``L^ x_i = sum_{j->i} wl x_j + (2 / lambda_max - 1) x_i``,
    ``wl = (2 * -w) / lambda_max`` and ``w`` the ``normalization`` (``"sym"``: ``deg_j^-1/2 deg_i^-1/2``, ``"rw"``:
    ``1 / deg_j``) by OUT-degree over the edges of ``g`` without its self loops - a ``GraphIndex`` built with
    ``self_loops=False, normalize=False``; self loops in it are dropped here, duplicates count.  ``lambda_max``: None
    (2.0) or a Python number > 0.  ``x``: float32 ``[N, F >= 1]`` on the graph's device.  One autograd node,
    differentiable in ``x``.  ``K = 1`` and ``N = 0`` need no graph (``g`` may be None) and launch no hop."""
    if not isinstance(K, int) or isinstance(K, bool) or K < 1:
        raise ValueError(f"cheb_basis: K must be an int >= 1, got {K!r}")
    if normalization not in CHEB_MODES:
        raise ValueError(f"cheb_basis: normalization must be 'sym' or 'rw', got {normalization!r}")
    lam = cheb_lambda(lambda_max)
    x = resolve(x)
    _require_cuda(x, "x")
    if x.dim() != 2 or x.dtype != torch.float32 or x.size(1) == 0:
        raise ValueError(f"cheb_basis: x must be a float32 [N, F >= 1] tensor, got {tuple(x.shape)} {x.dtype}")
    if x.size(0) and K > 1:
        if g is None:
            raise ValueError("cheb_basis: g may be None only for K = 1 or an x without rows")
        if g.self_loops or g.normalize or g.fwd.row_offset or g.bwd.row_offset:
            raise ValueError("cheb_basis: the graph must be built with self_loops=False, normalize=False (and be no row "
                             "window of a merged adjacency)")
        if g.device != x.device:
            raise RuntimeError(f"cheb_basis: x is on {x.device} but the graph is on {g.device}")
        if g.num_nodes != x.size(0):
            raise ValueError(f"cheb_basis: x has {x.size(0)} rows but the graph has {g.num_nodes} nodes")
    return _ChebBasisFn.apply(g, x, K, CHEB_MODES[normalization], lam)
