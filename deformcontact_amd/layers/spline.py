"""SplineConv's aggregation."""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from .. import _lib
from .._host import _grad_layout, _graph_check, _i64_array, _ptr, _rowmajor, _rows
from ..deferred import resolve
from ..graph import GraphIndex, _require_cuda, current_stream_ptr
from ..ops import hop
from .gmm import gmm_relu_ok
from .gnn import _mask_and_bias_grad
from .sage import _sage_grad


# --------------------------------------------------------------------------- #
# SplineConv (dc_spline.hip): per in-edge a B-spline of degree 1..3 over the edge's D pseudo-coordinates names S =
# (degree+1)^D of the K column blocks of the source row of h = x @ weight[k] and weights them.  The basis values
# b [E, S] and the block indices wi [E, S] are formed once, in the order of the input edges (read through the
# adjacency's ``perm``), and saved for the backward.  ``kernel_size``, ``is_open_spline`` and ``degree`` are host values
# copied into the kernel arguments.  One launcher per C entry.
# --------------------------------------------------------------------------- #
SPLINE_MAX_D = _lib.DEFINES["DC_SPLINE_MAX_D"]
SPLINE_MAX_S = _lib.DEFINES["DC_SPLINE_MAX_S"]
SPLINE_MAX_K = _lib.DEFINES["DC_SPLINE_MAX_K"]
SPLINE_REDUCES = ("mean", "add")


def spline_geometry(kernel_size, is_open_spline, degree, dim: Optional[int] = None, who: str = "spline_aggregate"):
    """``(ks, open, degree, K, S)`` as host ints - ``ks`` / ``open``: tuples of ``D`` ints - from an int or a sequence
    of ``D`` ints, a bool or a sequence of ``D`` bools, and the degree; every cap of the layer checked (``ValueError``).
    ``dim``: D where it is not given by a sequence."""
    def seq(v, scalar, name):
        if isinstance(v, torch.Tensor):
            v = v.tolist()
        if isinstance(v, scalar) and not (scalar is int and isinstance(v, bool)):
            if dim is None:
                raise ValueError(f"{who}: {name} must be a sequence of D values where dim is not given")
            return [v] * dim
        if not isinstance(v, (list, tuple)) or not all(isinstance(t, scalar) for t in v):
            raise ValueError(f"{who}: {name} must be {'an int' if scalar is int else 'a bool'} or a sequence of them, "
                             f"got {v!r}")
        return list(v)
    if isinstance(degree, bool) or not isinstance(degree, int) or degree not in (1, 2, 3):
        raise ValueError(f"{who}: degree must be 1, 2 or 3, got {degree!r}")
    if dim is not None and (isinstance(dim, bool) or not isinstance(dim, int) or not 1 <= dim <= SPLINE_MAX_D):
        raise ValueError(f"{who}: dim must be an int within 1..{SPLINE_MAX_D}, got {dim!r}")
    ks, op = seq(kernel_size, int, "kernel_size"), seq(is_open_spline, (bool, int), "is_open_spline")
    d = dim if dim is not None else len(ks)
    if not 1 <= d <= SPLINE_MAX_D:
        raise ValueError(f"{who}: dim must be within 1..{SPLINE_MAX_D}, got {d}")
    if len(ks) != d or len(op) != d:
        raise ValueError(f"{who}: kernel_size and is_open_spline must have dim = {d} entries, got {len(ks)} and "
                         f"{len(op)}")
    s = (degree + 1) ** d
    if s > SPLINE_MAX_S:
        raise ValueError(f"{who}: (degree+1)^dim = {s} slots per edge, at most {SPLINE_MAX_S} are supported")
    if any(isinstance(t, bool) or t < 1 for t in ks):
        raise ValueError(f"{who}: every kernel_size must be an int >= 1, got {ks}")
    k = math.prod(ks)
    if k > SPLINE_MAX_K:
        raise ValueError(f"{who}: the product of kernel_size is {k}, at most {SPLINE_MAX_K} is supported")
    return tuple(ks), tuple(int(bool(t)) for t in op), degree, k, s


def _spline_host(ks, op):
    return _i64_array(list(ks)), (ctypes.c_int32 * len(op))(*op)


def _spline_basis(a, ks, op, degree: int):
    """-> (b [E, S] float32, wi [E, S] int32) in the order of the input edges: the basis products and the indices of
    the weight matrices they belong to."""
    ne, d = a.shape
    s = (degree + 1) ** d
    b = torch.empty((ne, s), dtype=torch.float32, device=a.device)
    wi = torch.empty((ne, s), dtype=torch.int32, device=a.device)
    if ne == 0:
        return b, wi
    hks, hop = _spline_host(ks, op)
    _lib.check(_lib.lib().dc_spline_basis(a.data_ptr(), _rowmajor(a, "edge_attr"), hks, hop, degree, b.data_ptr(),
                                          wi.data_ptr(), ne, d, current_stream_ptr(a.device)), "dc_spline_basis")
    return b, wi


def _spline_fwd(g: GraphIndex, b, wi, h, k: int, m: int, mean: bool, base=None, relu: bool = False) -> torch.Tensor:
    """y [N, M]: ``sum_p (sum_s b[perm[p], s] h[other[p], wi[perm[p], s]*M:+M])`` - per edge the message over s in order,
    the messages in p order; ``mean``: divided by the in-degree; ``+ base``; ``relu``: ``max(., 0)``."""
    n, (ne, s) = h.size(0), b.shape
    y = torch.empty((n, m), dtype=torch.float32, device=h.device)
    _lib.check(_lib.lib().dc_spline_fwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), g.fwd.perm.data_ptr(),
                                        b.data_ptr() if ne else None, wi.data_ptr() if ne else None, h.data_ptr(),
                                        _rowmajor(h, "h"), _ptr(base), _rowmajor(base, "base") if base is not None else 0,
                                        int(mean), int(relu), y.data_ptr(), m, n, ne, s, k, m,
                                        current_stream_ptr(h.device)), "dc_spline_fwd")
    return y


def _spline_bwd_h(g: GraphIndex, b, wi, gy, k: int, mean: bool) -> torch.Tensor:
    """g_h [N, K*M] over the transposed set: ``sum_t sum_{s: wi[perm_t[t], s] == k} b[perm_t[t], s] gs[other_t[t], c]``,
    ``gs = g_y / deg`` (mean, the in-degree read from the forward ``ptr``) or ``g_y``; every column is written."""
    (n, m), (ne, s) = gy.shape, b.shape
    gh = torch.empty((n, k * m), dtype=torch.float32, device=gy.device)
    _lib.check(_lib.lib().dc_spline_bwd_h(g.bwd.ptr.data_ptr(), g.bwd.other.data_ptr(), g.bwd.perm.data_ptr(),
                                          g.fwd.ptr.data_ptr() if mean else None, b.data_ptr() if ne else None,
                                          wi.data_ptr() if ne else None, gy.data_ptr(), _rowmajor(gy, "gy"),
                                          gh.data_ptr(), k * m, n, ne, s, k, m, current_stream_ptr(gy.device)),
               "dc_spline_bwd_h")
    return gh


def _spline_bwd_b(g: GraphIndex, wi, h, gy, k: int, mean: bool) -> torch.Tensor:
    """g_b [E, S] in the order of the input edges: ``sum_c gs[dst_q, c] h[src_q, wi[q, s]*M + c]``."""
    (n, m), (ne, s) = gy.shape, wi.shape
    gb = torch.empty((ne, s), dtype=torch.float32, device=gy.device)
    if ne == 0:
        return gb
    ei = g.edge_index
    _lib.check(_lib.lib().dc_spline_bwd_b(ei[0].data_ptr(), ei[1].data_ptr(), g.fwd.ptr.data_ptr() if mean else None,
                                          wi.data_ptr(), h.data_ptr(), _rowmajor(h, "h"), gy.data_ptr(),
                                          _rowmajor(gy, "gy"), gb.data_ptr(), n, ne, s, k, m,
                                          current_stream_ptr(gy.device)), "dc_spline_bwd_b")
    return gb


def _spline_bwd_a(gb, a, ks, op, degree: int) -> torch.Tensor:
    """g_a [E, D]: ``float(ks[d] - degree open[d]) sum_s g_b[q, s] B'(f_d) prod_{d' != d} B(f_d')``."""
    ne, d = a.shape
    ga = torch.empty((ne, d), dtype=torch.float32, device=a.device)
    if ne == 0:
        return ga
    hks, hop = _spline_host(ks, op)
    _lib.check(_lib.lib().dc_spline_bwd_a(gb.data_ptr(), a.data_ptr(), _rowmajor(a, "edge_attr"), hks, hop, degree,
                                          ga.data_ptr(), d, ne, d, current_stream_ptr(a.device)), "dc_spline_bwd_a")
    return ga


class _SplineAggFn(torch.autograd.Function):
    """The B-spline aggregation: two launches forward (the basis, the S-way gather); backward the ReLU mask (``relu``),
    one launch for g_h and - only when ``edge_attr`` needs a gradient - one for g_b and one for g_a.  Saved: h, the
    basis b and the indices wi [E, S], ``edge_attr`` when its gradient is wanted and, with ``relu``, the output."""

    @staticmethod
    def forward(ctx, g: GraphIndex, h, a, base, geom, m: int, mean: bool, relu: bool):
        ctx.g, ctx.geom, ctx.m, ctx.mean, ctx.relu, ctx.empty = g, geom, m, mean, relu, h.size(0) == 0
        if ctx.empty:                        # no rows: nothing to launch (an empty tensor has no address)
            ctx.shapes = (h.shape, a.shape)
            return h.new_empty((0, m))
        ks, op, degree, k, _ = geom
        b, wi = _spline_basis(a, ks, op, degree)
        y = _spline_fwd(g, b, wi, h, k, m, mean, base, relu)
        ctx.save_for_backward(h, b, wi, a if ctx.needs_input_grad[2] else None, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        need = ctx.needs_input_grad
        if ctx.empty:
            hs, as_ = ctx.shapes
            return (None, gy.new_zeros(hs) if need[1] else None, gy.new_zeros(as_) if need[2] else None,
                    gy.new_zeros(gy.shape) if need[3] else None, None, None, None, None)
        h, b, wi, a, y = ctx.saved_tensors
        ks, op, degree, k, _ = ctx.geom
        if ctx.relu:
            gy, _ = _mask_and_bias_grad(_grad_layout(gy, 0), y, None, False)
        else:
            gy = _sage_grad(gy)
        gh = _spline_bwd_h(ctx.g, b, wi, gy, k, ctx.mean) if need[1] else None
        ga = None
        if need[2]:
            ga = _spline_bwd_a(_spline_bwd_b(ctx.g, wi, h, gy, k, ctx.mean), a, ks, op, degree)
        return None, gh, ga, gy if need[3] else None, None, None, None, None


def spline_aggregate(g: Optional[GraphIndex], h: torch.Tensor, edge_attr: torch.Tensor, kernel_size, is_open_spline,
                     degree: int = 1, reduce: str = "mean", base: Optional[torch.Tensor] = None,
                     relu: bool = False) -> torch.Tensor:
    """PyG ``SplineConv``'s aggregation (torch-spline-conv's basis and weighting): ``s_i = sum_{j->i} sum_s b_s(e_ji)
    h[j, wi_s(e_ji)*M:+M]`` over the edges of ``g`` - a ``GraphIndex`` of one ``edge_index`` built with
    ``self_loops=False, normalize=False``: the edge set as given, duplicates counting - with the ``S = (degree+1)^D``
    basis products ``b_s`` and weight indices ``wi_s`` of INTEGRATION.md 1.9.  ``reduce="mean"`` divides by the
    in-degree (duplicates counted; a row without edges is 0), ``"add"`` does not; then ``+ base`` (``[N, M]``, the root
    term with its bias; None: none) and, with ``relu``, the ReLU - all in the gather's epilogue.  ``h``: float32
    ``[N, K*M]``, column ``k*M + c`` weight matrix k, channel c, ``K`` the product of ``kernel_size``; ``edge_attr``:
    float32 ``[E, D]`` in [0, 1] with rows in the order of that ``edge_index`` (outside [0, 1] the index wraps, NaN
    propagates; nothing is validated by a host read).  ``kernel_size`` (D ints), ``is_open_spline`` (D bools) and
    ``degree`` (1..3) are host values.  Caps: ``D <= 4``, ``S <= 64``, ``K <= 1024``, ``E*S < 2^31``, ``N*K*M < 2^31``
    (``ValueError``).  All tensors on the graph's device; ``h``, ``edge_attr`` and ``base`` with unit inner stride
    (column slices pass as they are).  One autograd node, differentiable in ``h``, ``edge_attr`` (two launches, skipped
    when it needs no gradient) and ``base``; with ``relu`` the backward masks by ``y > 0``: ``relu'(0) = 0``, and ``M``
    must be a width of the mask pass (``gmm_relu_ok``).  The gradient of ``edge_attr`` reads the endpoints from
    ``g.edge_index`` at backward time: the edge list must stay unchanged until the backward has run.  ``N = 0``
    returns an empty tensor without a launch (``g`` may then be None)."""
    if not isinstance(reduce, str) or reduce not in SPLINE_REDUCES:
        raise ValueError(f"spline_aggregate: reduce must be 'mean' or 'add', got {reduce!r}")
    h, edge_attr = resolve(h), resolve(edge_attr)
    for name, t in (("h", h), ("edge_attr", edge_attr)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"spline_aggregate: {name} must be a tensor, got {type(t).__name__}")
    geom = spline_geometry(kernel_size, is_open_spline, degree,
                           None if isinstance(kernel_size, (list, tuple, torch.Tensor)) else
                           (edge_attr.size(1) if edge_attr.dim() == 2 else -1))
    ks, _, _, k, s = geom
    d = len(ks)
    if h.dim() != 2 or h.dtype != torch.float32 or h.size(1) == 0 or h.size(1) % k:
        raise ValueError(f"spline_aggregate: h must be a float32 [N, K*M] tensor with K = {k}, M >= 1, got "
                         f"{tuple(h.shape)} {h.dtype}")
    m = h.size(1) // k
    if edge_attr.dim() != 2 or edge_attr.dtype != torch.float32 or edge_attr.size(1) != d:
        raise ValueError(f"spline_aggregate: edge_attr must be a float32 [E, {d}] tensor, got "
                         f"{tuple(edge_attr.shape)} {edge_attr.dtype}")
    if edge_attr.size(0) * s >= 2 ** 31:
        raise ValueError(f"spline_aggregate: E*S = {edge_attr.size(0)}*{s} must stay below 2^31")
    if h.size(0) * k * m >= 2 ** 31:
        raise ValueError(f"spline_aggregate: N*K*M = {h.size(0)}*{k}*{m} must stay below 2^31")
    if base is not None:
        base = resolve(base)
        if not isinstance(base, torch.Tensor) or base.dim() != 2 or base.dtype != torch.float32 or \
                base.shape != (h.size(0), m):
            raise ValueError(f"spline_aggregate: base must be a float32 [{h.size(0)}, {m}] tensor (or None)")
    if relu and not gmm_relu_ok(m):
        raise ValueError(f"spline_aggregate: relu=True needs M to be a multiple of 4 that divides 1024, got {m}; apply "
                         "the ReLU behind the call")
    _require_cuda(h, "h")
    for name, t in (("edge_attr", edge_attr), ("base", base)):
        if t is not None:
            _require_cuda(t, name)
            if t.device != h.device:
                raise RuntimeError(f"spline_aggregate: h is on {h.device} but {name} is on {t.device}")
    mean = reduce == "mean"
    if h.size(0) == 0:
        if edge_attr.size(0) != 0:
            raise ValueError(f"spline_aggregate: edge_attr has {edge_attr.size(0)} rows but h has no node")
        return _SplineAggFn.apply(None, h, edge_attr, base, geom, m, mean, bool(relu))
    if g is None:
        raise ValueError("spline_aggregate: g may be None only for an h without rows")
    _graph_check("spline_aggregate", g, False, h, "h")
    if g.num_nodes != h.size(0):
        raise ValueError(f"spline_aggregate: h has {h.size(0)} rows but the graph has {g.num_nodes} nodes")
    if g.num_input_edges != edge_attr.size(0):
        raise ValueError(f"spline_aggregate: edge_attr has {edge_attr.size(0)} rows but the graph has "
                         f"{g.num_input_edges} edges")
    return _SplineAggFn.apply(g, _rows(h), _rows(edge_attr), _rows(base) if base is not None else None, geom, m, mean,
                              bool(relu))
