"""GMMConv's aggregation."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from .._host import _grad_layout, _graph_check, _ptr, _rowmajor, _rows
from ..deferred import resolve
from ..graph import GraphIndex, _require_cuda, current_stream_ptr
from .gnn import _mask_and_bias_grad
from .sage import _sage_grad


# --------------------------------------------------------------------------- #
# GMMConv (dc_gmm.hip): per in-edge a mixture of K Gaussians over the edge's D pseudo-coordinates weights the K column
# blocks of the source row of h = x @ g.  The weights w [E, K] are formed once, in the order of the input edges (read
# through the adjacency's ``perm``), and saved for the backward.  One launcher per C entry.
# --------------------------------------------------------------------------- #
GMM_MAX_K = _lib.DEFINES["DC_GMM_MAX_K"]
GMM_MAX_D = _lib.DEFINES["DC_GMM_MAX_D"]
GMM_REDUCES = ("mean", "add")


def gmm_relu_ok(m: int) -> bool:
    """Output widths at which ``gmm_aggregate(relu=True)`` runs: those of the mask pass of its backward
    (``dc_mask_colsum_f32``: a multiple of 4 that divides 1024).  At any other width the ReLU goes behind the call."""
    return m % 4 == 0 and 4 <= m <= 1024 and 256 % (m // 4) == 0


def _gmm_weights(a, mu, sigma) -> torch.Tensor:
    """w [E, K]: ``exp(sum_d -0.5 (a[q,d] - mu[k,d])^2 / (1e-15 + sigma[k,d]^2))`` in the order of the input edges."""
    ne, (k, d) = a.size(0), mu.shape
    w = torch.empty((ne, k), dtype=torch.float32, device=a.device)
    if ne == 0:
        return w
    _lib.check(_lib.lib().dc_gmm_weights(a.data_ptr(), _rowmajor(a, "edge_attr"), mu.data_ptr(), sigma.data_ptr(),
                                         w.data_ptr(), ne, k, d, current_stream_ptr(a.device)), "dc_gmm_weights")
    return w


def _gmm_fwd(g: GraphIndex, w, h, m: int, mean: bool, base=None, relu: bool = False) -> torch.Tensor:
    """y [N, M]: ``sum_p sum_k w[perm[p], k] h[other[p], k*M:(k+1)*M]`` in p, then k order; ``mean``: divided by the
    in-degree; ``+ base``; ``relu``: ``max(., 0)``."""
    n, k = h.size(0), w.size(1)
    y = torch.empty((n, m), dtype=torch.float32, device=h.device)
    _lib.check(_lib.lib().dc_gmm_fwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), g.fwd.perm.data_ptr(),
                                     w.data_ptr() if w.size(0) else None, h.data_ptr(), _rowmajor(h, "h"), _ptr(base),
                                     _rowmajor(base, "base") if base is not None else 0, int(mean), int(relu),
                                     y.data_ptr(), m, n, w.size(0), k, m, current_stream_ptr(h.device)), "dc_gmm_fwd")
    return y


def _gmm_bwd_h(g: GraphIndex, w, gy, mean: bool) -> torch.Tensor:
    """g_h [N, K*M] over the transposed set: ``sum_t w[perm_t[t], k] gs[other_t[t], c]``, ``gs = g_y / deg`` (mean, the
    in-degree read from the forward ``ptr``) or ``g_y``."""
    (n, m), k = gy.shape, w.size(1)
    gh = torch.empty((n, k * m), dtype=torch.float32, device=gy.device)
    _lib.check(_lib.lib().dc_gmm_bwd_h(g.bwd.ptr.data_ptr(), g.bwd.other.data_ptr(), g.bwd.perm.data_ptr(),
                                       g.fwd.ptr.data_ptr() if mean else None, w.data_ptr() if w.size(0) else None,
                                       gy.data_ptr(), _rowmajor(gy, "gy"), gh.data_ptr(), k * m, n, w.size(0), k, m,
                                       current_stream_ptr(gy.device)), "dc_gmm_bwd_h")
    return gh


def _gmm_bwd_w(g: GraphIndex, h, gy, k: int, mean: bool) -> torch.Tensor:
    """g_w [E, K] in the order of the input edges: ``sum_c gs[dst_q, c] h[src_q, k*M + c]``."""
    n, m = gy.shape
    ne = g.num_input_edges
    gw = torch.empty((ne, k), dtype=torch.float32, device=gy.device)
    if ne == 0:
        return gw
    ei = g.edge_index
    _lib.check(_lib.lib().dc_gmm_bwd_w(ei[0].data_ptr(), ei[1].data_ptr(), g.fwd.ptr.data_ptr() if mean else None,
                                       h.data_ptr(), _rowmajor(h, "h"), gy.data_ptr(), _rowmajor(gy, "gy"),
                                       gw.data_ptr(), n, ne, k, m, current_stream_ptr(gy.device)), "dc_gmm_bwd_w")
    return gw


def _gmm_bwd_params(gw, w, a, mu, sigma, want_a: bool):
    """-> (g_mu [K, D], g_sigma [K, D], g_a [E, D] or None) from ``t = g_w w`` and ``r = (a - mu) / (1e-15 +
    sigma^2)``: ``sum_q t r``, ``(sum_q t r r) sigma``, ``-sum_k t r``."""
    ne, (k, d), dev = a.size(0), mu.shape, a.device
    ga = torch.empty((ne, d), dtype=torch.float32, device=dev) if want_a else None
    if ne == 0:
        return torch.zeros_like(mu), torch.zeros_like(sigma), ga
    gmu, gsigma = torch.empty((2, k, d), dtype=torch.float32, device=dev).unbind(0)
    L = _lib.lib()
    ws = torch.empty(max(L.dc_gmm_params_workspace_bytes(ne, k, d), 16), dtype=torch.uint8, device=dev)
    _lib.check(L.dc_gmm_bwd_params(gw.data_ptr(), w.data_ptr(), a.data_ptr(), _rowmajor(a, "edge_attr"), mu.data_ptr(),
                                   sigma.data_ptr(), ws.data_ptr(), ws.numel(), gmu.data_ptr(), gsigma.data_ptr(),
                                   _ptr(ga), d, ne, k, d, current_stream_ptr(dev)), "dc_gmm_bwd_params")
    return gmu, gsigma, ga


class _GmmAggFn(torch.autograd.Function):
    """The Gaussian-mixture aggregation: two launches forward (the weights, the K-way gather); backward the ReLU mask
    (``relu``), one launch for g_h, one for g_w and two for g_mu / g_sigma (three with g_a) - the last three skipped when
    neither ``edge_attr`` nor ``mu`` nor ``sigma`` needs a gradient.  Saved: h, edge_attr, mu, sigma, the weights
    w [E, K] and, with ``relu``, the output."""

    @staticmethod
    def forward(ctx, g: GraphIndex, h, a, mu, sigma, base, m: int, mean: bool, relu: bool):
        ctx.g, ctx.m, ctx.mean, ctx.relu, ctx.empty = g, m, mean, relu, h.size(0) == 0
        if ctx.empty:                        # no rows: nothing to launch (an empty tensor has no address)
            ctx.shapes = (h.shape, a.shape, mu.shape)
            return h.new_empty((0, m))
        w = _gmm_weights(a, mu, sigma)
        y = _gmm_fwd(g, w, h, m, mean, base, relu)
        ctx.save_for_backward(h, a, mu, sigma, w, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        need = ctx.needs_input_grad
        if ctx.empty:
            hs, as_, ps = ctx.shapes
            return (None, gy.new_zeros(hs) if need[1] else None, gy.new_zeros(as_) if need[2] else None,
                    gy.new_zeros(ps) if need[3] else None, gy.new_zeros(ps) if need[4] else None,
                    gy.new_zeros(gy.shape) if need[5] else None, None, None, None)
        h, a, mu, sigma, w, y = ctx.saved_tensors
        if ctx.relu:
            gy, _ = _mask_and_bias_grad(_grad_layout(gy, 0), y, None, False)
        else:
            gy = _sage_grad(gy)
        gh = _gmm_bwd_h(ctx.g, w, gy, ctx.mean) if need[1] else None
        ga = gmu = gsigma = None
        if need[2] or need[3] or need[4]:
            gw = _gmm_bwd_w(ctx.g, h, gy, w.size(1), ctx.mean)
            gmu, gsigma, ga = _gmm_bwd_params(gw, w, a, mu, sigma, need[2])
        return (None, gh, ga, gmu if need[3] else None, gsigma if need[4] else None, gy if need[5] else None, None,
                None, None)


def gmm_aggregate(g: Optional[GraphIndex], h: torch.Tensor, edge_attr: torch.Tensor, mu: torch.Tensor,
                  sigma: torch.Tensor, reduce: str = "mean", base: Optional[torch.Tensor] = None,
                  relu: bool = False) -> torch.Tensor:
    """PyG ``GMMConv``'s aggregation (``separate_gaussians=False``): ``s_i = sum_{j->i} sum_k w_k(e_ji) h[j, k*M:(k+1)*M]``
    with ``w_k(e) = exp(sum_d -0.5 (e_d - mu[k,d])^2 / (1e-15 + sigma[k,d]^2))`` over the edges of ``g`` - a
    ``GraphIndex`` of one ``edge_index`` built with ``self_loops=False, normalize=False``: the edge set as given,
    duplicates counting.  ``reduce="mean"`` divides by the in-degree (duplicates counted; a row without edges is 0),
    ``"add"`` does not; then ``+ base`` (``[N, M]``, the root term with its bias; None: none) and, with ``relu``, the
    ReLU - all in the gather's epilogue.  ``h``: float32 ``[N, K*M]``, column ``k*M + c`` kernel k, channel c;
    ``edge_attr``: float32 ``[E, D]`` with rows in the order of that ``edge_index``; ``mu``, ``sigma``: float32 ``[K, D]``,
    ``1 <= K <= 64``, ``1 <= D <= 16``, read BY THE KERNELS (parameters changed in place between two replays of a
    captured step are followed).  All on the graph's device; ``h``, ``edge_attr`` and ``base`` with unit inner stride
    (column slices pass as they are).  One autograd node, differentiable in ``h``, ``edge_attr`` (skipped when it needs
    no gradient), ``mu``, ``sigma`` and ``base``; with ``relu`` the backward masks by ``y > 0``: ``relu'(0) = 0``, and
    ``M`` must be a width of the mask pass (``gmm_relu_ok``).  The gradient of ``edge_attr``, ``mu`` and ``sigma`` reads
    the endpoints from ``g.edge_index`` at backward time while the forward read the sorted set built from it: the edge
    list must stay unchanged until the backward has run.  ``N = 0`` returns an empty tensor
    without a launch (``g`` may then be None)."""
    if not isinstance(reduce, str) or reduce not in GMM_REDUCES:
        raise ValueError(f"gmm_aggregate: reduce must be 'mean' or 'add', got {reduce!r}")
    h, edge_attr = resolve(h), resolve(edge_attr)
    for name, t in (("h", h), ("edge_attr", edge_attr), ("mu", mu), ("sigma", sigma)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"gmm_aggregate: {name} must be a tensor, got {type(t).__name__}")
    if mu.dim() != 2 or mu.dtype != torch.float32 or sigma.shape != mu.shape or sigma.dtype != torch.float32:
        raise ValueError(f"gmm_aggregate: mu and sigma must be float32 [K, D] tensors of one shape, got "
                         f"{tuple(mu.shape)} {mu.dtype} and {tuple(sigma.shape)} {sigma.dtype}")
    k, d = mu.shape
    if not 1 <= k <= GMM_MAX_K:
        raise ValueError(f"gmm_aggregate: kernel_size K must be within 1..{GMM_MAX_K}, got {k}")
    if not 1 <= d <= GMM_MAX_D:
        raise ValueError(f"gmm_aggregate: dim D must be within 1..{GMM_MAX_D}, got {d}")
    if h.dim() != 2 or h.dtype != torch.float32 or h.size(1) == 0 or h.size(1) % k:
        raise ValueError(f"gmm_aggregate: h must be a float32 [N, K*M] tensor with K = {k}, M >= 1, got "
                         f"{tuple(h.shape)} {h.dtype}")
    m = h.size(1) // k
    if edge_attr.dim() != 2 or edge_attr.dtype != torch.float32 or edge_attr.size(1) != d:
        raise ValueError(f"gmm_aggregate: edge_attr must be a float32 [E, {d}] tensor, got {tuple(edge_attr.shape)} "
                         f"{edge_attr.dtype}")
    if base is not None:
        base = resolve(base)
        if not isinstance(base, torch.Tensor) or base.dim() != 2 or base.dtype != torch.float32 or \
                base.shape != (h.size(0), m):
            raise ValueError(f"gmm_aggregate: base must be a float32 [{h.size(0)}, {m}] tensor (or None)")
    if relu and not gmm_relu_ok(m):
        raise ValueError(f"gmm_aggregate: relu=True needs M to be a multiple of 4 that divides 1024, got {m}; apply "
                         "the ReLU behind the call")
    _require_cuda(h, "h")
    for name, t in (("edge_attr", edge_attr), ("mu", mu), ("sigma", sigma), ("base", base)):
        if t is not None:
            _require_cuda(t, name)
            if t.device != h.device:
                raise RuntimeError(f"gmm_aggregate: h is on {h.device} but {name} is on {t.device}")
    mean = reduce == "mean"
    mu, sigma = mu.contiguous(), sigma.contiguous()
    if h.size(0) == 0:
        if edge_attr.size(0) != 0:
            raise ValueError(f"gmm_aggregate: edge_attr has {edge_attr.size(0)} rows but h has no node")
        return _GmmAggFn.apply(None, h, edge_attr, mu, sigma, base, m, mean, bool(relu))
    if g is None:
        raise ValueError("gmm_aggregate: g may be None only for an h without rows")
    _graph_check("gmm_aggregate", g, False, h, "h")
    if g.num_nodes != h.size(0):
        raise ValueError(f"gmm_aggregate: h has {h.size(0)} rows but the graph has {g.num_nodes} nodes")
    if g.num_input_edges != edge_attr.size(0):
        raise ValueError(f"gmm_aggregate: edge_attr has {edge_attr.size(0)} rows but the graph has "
                         f"{g.num_input_edges} edges")
    return _GmmAggFn.apply(g, _rows(h), _rows(edge_attr), mu, sigma, _rows(base) if base is not None else None, m, mean,
                           bool(relu))
