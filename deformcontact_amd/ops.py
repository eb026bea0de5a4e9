"""Host-side operator layer: thin launches of the C ABI + autograd wiring.

Mirrors what PyG's ``TAGConv`` / ``GCNConv`` / ``GATConv`` ``forward`` do for the
reference (``models/model.py:71,77``), with every gather /
scatter step executed by ``libdeformcontact_hip.so`` on the current HIP stream.
PyTorch is used for device memory, autograd bookkeeping and (for now) the plain
dense GEMMs.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import List, Optional

import torch

from . import _lib
from .deferred import resolve
from .graph import GraphIndex, SortedAdjacency, _require_cuda, capture_id, current_stream_ptr, graph_index


def _rowmajor(t: torch.Tensor, what: str, dtypes=(torch.float32,)) -> int:
    """Return the leading dimension of a 2-D row-major (possibly column-sliced) view of one of ``dtypes``."""
    if t.dim() != 2 or t.dtype not in dtypes:
        raise ValueError(f"{what}: expected a 2-D tensor of {dtypes}, got {tuple(t.shape)} {t.dtype}")
    if t.size(1) > 1 and t.stride(1) != 1:
        raise ValueError(f"{what}: innermost dimension must be contiguous")
    return t.stride(0) if t.size(0) > 1 else max(t.stride(0), t.size(1))


def _vp_array(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _ptr_array(tensors):
    return _vp_array([t.data_ptr() for t in tensors])


def _i64_array(vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def _spmm(adj: SortedAdjacency, w: Optional[torch.Tensor], x: torch.Tensor, out: Optional[torch.Tensor] = None,
          addend: Optional[torch.Tensor] = None, rowmax: Optional[torch.Tensor] = None, rowmax_mode: int = 0):
    """The one launch path of the fp32 hop: ``out = addend + A x`` with the edge weights ``w`` (None: ones),
    ``dc_spmm_f32`` or its ``_rowmax`` / ``_window`` forms (``rowmax`` given / ``adj`` a row window of a merged
    adjacency, whose operands hold only the window's rows)."""
    n, f = x.shape
    if out is None:
        out = torch.empty((n, f), dtype=torch.float32, device=x.device)
    args = [adj.ptr.data_ptr(), adj.other.data_ptr(), _ptr(w), x.data_ptr(), _rowmajor(x, "x"),
            _ptr(addend), _rowmajor(addend, "addend") if addend is not None else 0,
            out.data_ptr(), _rowmajor(out, "out"), n, f]
    name = "dc_spmm_f32"
    if rowmax is not None:
        name += "_rowmax"
        args += [rowmax.data_ptr(), int(rowmax_mode)]
    if adj.row_offset:
        name += "_window"
        args.append(int(adj.row_offset))
    _lib.check(getattr(_lib.lib(), name)(*args, current_stream_ptr(x.device)), name)
    return out


def hop(adj: SortedAdjacency, x: torch.Tensor, out: Optional[torch.Tensor] = None,
        addend: Optional[torch.Tensor] = None, weighted: bool = True,
        rowmax: Optional[torch.Tensor] = None, rowmax_mode: int = 0) -> torch.Tensor:
    """``out[i] = addend[i] + sum_{p in seg(i)} w[p] * x[other[p]]`` (one launch).

    ``x`` / ``out`` / ``addend`` may be column slices of wider row-major buffers.  With ``rowmax``
    (float32 ``[N]``) the launch also records ``max |out[i, :]|`` there (``rowmax_mode`` bit 0:
    joined with ``max |x[i, :]|``, bit 1: joined with the value already stored)."""
    _require_cuda(x, "x")
    n, f = x.shape
    if adj.ptr.numel() != n + 1:
        raise ValueError(f"hop: x has {n} rows but the graph has {adj.ptr.numel() - 1} nodes")
    if out is not None and out.shape != x.shape:
        raise ValueError("hop: out shape mismatch")
    if addend is not None and addend.shape != x.shape:
        raise ValueError("hop: addend shape mismatch")
    if rowmax is not None and (rowmax.dtype != torch.float32 or rowmax.numel() != n or not rowmax.is_contiguous()):
        raise ValueError("hop: rowmax must be a contiguous float32 [N] tensor")
    return _spmm(adj, adj.w if weighted else None, x, out, addend, rowmax, rowmax_mode)


def weight_rowmax(ws) -> torch.Tensor:
    """``out[o] = max_s,f |W_s[o, f]|`` over the K+1 weight blocks of a TAGConv layer
    (``dc_tag_weight_rowmax``): the per-output-row scale of the fp16x2 dense block."""
    fo, fi = ws[0].shape
    out = torch.empty(fo, dtype=torch.float32, device=ws[0].device)
    rc = _lib.lib().dc_tag_weight_rowmax(_ptr_array(ws), len(ws), fo, fi, out.data_ptr(),
                                         current_stream_ptr(out.device))
    _lib.check(rc, "dc_tag_weight_rowmax")
    return out


def rowabsmax(x: torch.Tensor) -> torch.Tensor:
    """``out[i] = max |x[i, :]|`` of a row-major 2-D float32 view (``dc_rowabsmax_f32``)."""
    _require_cuda(x, "x")
    n, f = x.shape
    out = torch.empty(n, dtype=torch.float32, device=x.device)
    rc = _lib.lib().dc_rowabsmax_f32(x.data_ptr(), _rowmajor(x, "x"), n, f, out.data_ptr(),
                                     current_stream_ptr(x.device))
    _lib.check(rc, "dc_rowabsmax_f32")
    return out


def hop_bf16(adj: SortedAdjacency, x: torch.Tensor, out: Optional[torch.Tensor] = None,
             addend: Optional[torch.Tensor] = None, weighted: bool = True,
             out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """The hop over bf16-stored features with fp32 accumulation (``dc_spmm_bf16``; SURVEY.md 8(d)
    config 5).  ``x`` is bfloat16; ``out`` / ``addend`` are ``out_dtype`` (bfloat16: the fp32 sum
    is rounded once on store; float32: the fp32 sum itself)."""
    _require_cuda(x, "x")
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("hop_bf16: out_dtype must be bfloat16 or float32")
    ldx = _rowmajor(x, "x", (torch.bfloat16,))
    n, f = x.shape
    if adj.ptr.numel() != n + 1:
        raise ValueError(f"hop_bf16: x has {n} rows but the graph has {adj.ptr.numel() - 1} nodes")
    if out is None:
        out = torch.empty((n, f), dtype=out_dtype, device=x.device)
    if out.shape != x.shape:
        raise ValueError("hop_bf16: out shape mismatch")
    ldy = _rowmajor(out, "out", (out_dtype,))
    lda = 0
    if addend is not None:
        if addend.shape != x.shape:
            raise ValueError("hop_bf16: addend shape mismatch")
        lda = _rowmajor(addend, "addend", (out_dtype,))
    rc = _lib.lib().dc_spmm_bf16(
        adj.ptr.data_ptr(), adj.other.data_ptr(), _ptr(adj.w if weighted else None), x.data_ptr(), ldx,
        _ptr(addend), lda, out.data_ptr(), ldy, n, f, 1 if out_dtype == torch.float32 else 0,
        current_stream_ptr(x.device))
    _lib.check(rc, "dc_spmm_bf16")
    return out


class _HopFn(torch.autograd.Function):
    """Differentiable single hop ``y = A x`` (``A`` = weighted sorted adjacency)."""

    @staticmethod
    def forward(ctx, g: GraphIndex, x: torch.Tensor, weighted: bool):
        ctx.g, ctx.weighted = g, weighted
        return hop(g.fwd, x.contiguous(), weighted=weighted)

    @staticmethod
    def backward(ctx, gy):
        return None, hop(ctx.g.bwd, _grad_layout(gy, 0), weighted=ctx.weighted), None


def propagate(g: GraphIndex, x: torch.Tensor, weighted: bool = True) -> torch.Tensor:
    """Autograd-aware hop (PyG ``propagate(edge_index, x=x, edge_weight=w)``)."""
    return _HopFn.apply(g, resolve(x), weighted)


def _grad_layout(g: torch.Tensor, row_align: int) -> torch.Tensor:
    """The incoming gradient ``g`` in a layout the backward kernels of the calling site take, copied only if it is not
    in one already.  ``row_align`` = 0: dense rows (plain contiguous); 1: unit inner stride, any row stride (column
    slices pass as they are); 4: unit inner stride, and row stride and base address multiples of 4 floats (16 bytes)."""
    ok = row_align == 1 or (row_align == 4 and g.stride(0) % 4 == 0 and g.data_ptr() % 16 == 0)
    return g if (ok and g.stride(1) == 1) else g.contiguous()


MAX_SEG = 4   # DC_MAX_SEG in include/deformcontact.h

#: Direct parameter-gradient mode (opt-in, ``dp.GradBucket(params, direct=True)``): the dW
#: slab-reduce kernel accumulates weight / bias gradients straight into the bucket's views instead
#: of returning them to autograd (which would run one elementwise ``add`` kernel per parameter).
#: Only parameters the bucket has marked are written that way (``requires_grad`` ones whose
#: ``.grad`` still is the bucket's view); every such write is reported to the bucket
#: (``GradBucket.note_direct_write``), which makes its consumers (``all_reduce_mean``,
#: ``FlatAdam.step``) wait for the writing stream.  Tensor hooks on those parameters do not fire
#: and ``torch.autograd.grad`` gets ``None`` for them - hence opt-in.  Setting this to False
#: disables the mode globally.
DIRECT_PARAM_GRAD = True


#: Run the dense blocks (forward, dX, dW) on the bf16 matrix cores with every fp32 operand split
#: exactly into hi + mid + lo bf16 terms and six MFMA products (``dc_tag_linear_*_split``):
#: fp32-accurate (measured error vs float64 equal to the fp32-MFMA / rocBLAS kernels,
#: profiles/r01/d_split_accuracy.txt) at up to 2.7x the fp32 MFMA peak.  ``DC_DENSE_SPLIT=0``
#: (or setting this to False) keeps everything on ``v_mfma_f32_32x32x2_f32``.
DENSE_SPLIT_BF16 = os.environ.get("DC_DENSE_SPLIT", "1") != "0"

#: bf16 MFMA products per tile in split mode: 6 = fp32-accurate (the C-ABI also takes 3 = ~4e-6 relative and
#: 1 = plain bf16 operands with fp32 accumulation; nothing in this package asks for them)
DENSE_PRODUCTS = 6


#: the short-reduction forward kernel for the first layers (``dc_tag_linear_fwd_narrow``: persistent, weights resident in
#: registers, no packing launch; bit-identical to the six-product split kernel); ``DC_NARROW_FWD=0``: ``dc_tag_pack_weights`` +
#: ``dc_tag_linear_fwd_split``
NARROW_FWD = os.environ.get("DC_NARROW_FWD", "1") != "0"

#: that kernel on weights PREPARED once per call (``dc_tag_linear_fwd_narrow_img``): the bf16x3 fragment image of the
#: layer's weights is written by the layer's own pack + first-hop launch (``dc_spmm_f32_pack_wprep``), or by
#: ``dc_tag_narrow_wimage`` where the call has no such launch, instead of by every workgroup of the block; same bits.
#: ``DC_NARROW_PREP=0``: the kernel that prepares its weights itself (``dc_tag_linear_fwd_narrow``).
NARROW_PREP = os.environ.get("DC_NARROW_PREP", "1") != "0"


class _NarrowImage:
    """The weight image of a narrow layer's forward block: a temporary of ONE call (the weights change from step to
    step, also under graph replay), like the outputs of ``_h2_weight_prep``.  ``filled``: a launch of this call has
    written it already."""

    STEP_BYTES = 3 * 8 * 64 * 16         # per 16 columns of the padded reduction (dc_narrow_image.h)

    def __init__(self, ws, wpad: int, dev):
        self.ws, self.wpad, self.filled = ws, wpad, False
        self.buf = torch.empty(wpad // 16 * self.STEP_BYTES, dtype=torch.uint8, device=dev)

    def ensure(self, st) -> int:
        """Address of the image, written on stream ``st`` by a launch of its own if no other launch has."""
        if not self.filled:
            fi = self.ws[0].size(1)
            _lib.check(_lib.lib().dc_tag_narrow_wimage(_ptr_array(self.ws), len(self.ws), fi, self.wpad,
                                                       self.buf.data_ptr(), st), "dc_tag_narrow_wimage")
            self.filled = True
        return self.buf.data_ptr()

#: fp16x2 mode of the wide (Fi % 16 == 0, unconcatenated) dense blocks: two power-of-two-scaled
#: fp16 planes per operand and THREE MFMA products instead of the six of the bf16 split - still
#: fp32-accurate (error below that of fp32 accumulation), half the matrix work.  The row maxima
#: the scaling needs come out of the hop launches.  ``DC_DENSE_F16X2=0`` keeps the bf16x3 split.
DENSE_F16X2 = os.environ.get("DC_DENSE_F16X2", "1") != "0"


#: K chained hops of a batch with a known layout as ONE launch with every graph's slice resident in LDS
#: (``dc_hop_chain_f32``, bit-identical to the K single hops); ``DC_HOP_CHAIN=0``: hop by hop.
HOP_CHAIN = os.environ.get("DC_HOP_CHAIN", "1") != "0"
_CHAIN_MAX_NODES = None


def hop_chain_eligible(g, adj: SortedAdjacency, slab: torch.Tensor, f: int, k: int) -> bool:
    """Can ``dc_hop_chain_f32`` run this chain?  Needs the batch layout (``graph_index(..., segments=)``), graphs
    of at most ``dc_hop_chain_max_nodes()`` nodes (4,096: 32-column slices up to 1,024 nodes, 16 up to 2,048, 8 beyond),
    F % 32 == 0 and 16-byte aligned slab rows."""
    global _CHAIN_MAX_NODES
    seg = getattr(g, "_layout", None)
    if not HOP_CHAIN or seg is None or k < 1 or f % 32 != 0 or adj.row_offset:
        return False
    if _CHAIN_MAX_NODES is None:
        _CHAIN_MAX_NODES = int(_lib.lib().dc_hop_chain_max_nodes())
    return (0 < g._seg_max_nodes <= _CHAIN_MAX_NODES and slab.dtype == torch.float32 and slab.dim() == 2
            and slab.stride(1) == 1 and slab.stride(0) % 4 == 0 and slab.data_ptr() % 16 == 0
            and adj.ptr.numel() == slab.size(0) + 1)


#: re-form gcn_norm weights from an LDS-resident degree table inside ``dc_hop_chain_f32`` (no vector-memory loads in its
#: hop loop) instead of loading ``w``; same bits.  False (tests): always load them.  No size rule: every chain workgroup
#: owns the whole LDS of its compute unit (``dc_hopchain.hip: kChainLdsRequest``).
HOP_CHAIN_GCN = True


def hop_chain(g, adj: SortedAdjacency, slab: torch.Tensor, f: int, k: int, weighted: bool = True,
              rowmax: Optional[torch.Tensor] = None, rowmax_mode: int = 0, src_block: int = 0, direction: int = 1) -> None:
    """``dc_hop_chain_f32``: blocks ``src_block + direction .. src_block + k * direction`` of ``slab`` from block
    ``src_block``, one launch (see ``hop_chain_eligible``)."""
    nptr, nseg = g._layout
    w = adj.w if weighted else None
    # the adjacency's weights are gcn_norm's (graph.GraphIndex builds nothing else): tell the kernel so
    deg = g.fwd.ptr if (HOP_CHAIN_GCN and w is not None and g.normalize and not g.self_loops) else None
    rc = _lib.lib().dc_hop_chain_f32(
        adj.ptr.data_ptr(), adj.other.data_ptr(), _ptr(w), _ptr(deg), adj.other.numel(),
        nptr, nseg, slab.data_ptr(), slab.stride(0), slab.size(0), f, k, int(src_block), int(direction),
        _ptr(rowmax), int(rowmax_mode), current_stream_ptr(slab.device))
    _lib.check(rc, "dc_hop_chain_f32")


#: diagnostic tap (tools/exp/dp_flake2.py): ``DEBUG_TAP(name, tensor)`` is called with intermediate tensors of
#: ``_TagConvFn.backward`` when set; None in production
DEBUG_TAP = None
#: diagnostic hook (tools/exp/chain_hunt.py): called as ``DEBUG_CHAIN(g, adj, slab, f, k, transposed)`` right after a
#: ``dc_hop_chain_f32`` launch of ``chained_hops`` (``DEBUG_CHAIN_PRE``: right before it); None in production
DEBUG_CHAIN = None
DEBUG_CHAIN_PRE = None


def chained_hops(g: GraphIndex, slab: torch.Tensor, f: int, k: int, backward: bool,
                 rowmax: Optional[torch.Tensor] = None, transposed: bool = False,
                 rowmax_has_block0: bool = False, rowmax_zeroed: bool = False) -> None:
    """In place on ``slab`` ([N, ld], K+1 column blocks of width ``f``).  Forward: block j+1 =
    A block j (j = 0..k-1).  Backward: block j-1 += A^T block j (j = k..1).  Forward with
    ``rowmax`` ([N]): also ``rowmax[i] = max_j max |block j [i, :]|`` (needs k >= 1;
    ``rowmax_has_block0``: it already holds the maxima of block 0).  ``transposed`` (forward
    direction only): block j+1 = A^T block j."""
    if k == 0:
        return
    adj = g.bwd if (backward or transposed) else g.fwd
    blocks = [slab[:, j * f:(j + 1) * f] for j in range(k + 1)]
    if backward:
        for j in range(k, 0, -1):
            hop(adj, blocks[j], out=blocks[j - 1], addend=blocks[j - 1], weighted=g.normalize)
    elif hop_chain_eligible(g, adj, slab, f, k):
        # mode: 1 = fresh maxima over blocks 0..K (the entry clears the buffer first), 2 = joined with block 0's, which
        # the buffer already holds, 3 = over blocks 0..K joined with a buffer the caller has cleared (``rowmax_zeroed``)
        if DEBUG_CHAIN_PRE is not None:
            DEBUG_CHAIN_PRE(g, adj, slab, f, k, transposed)
        hop_chain(g, adj, slab, f, k, weighted=g.normalize, rowmax=rowmax,
                  rowmax_mode=2 if rowmax_has_block0 else (3 if rowmax_zeroed else 1))
        if DEBUG_CHAIN is not None:
            DEBUG_CHAIN(g, adj, slab, f, k, transposed)
    else:
        for j in range(k):
            hop(adj, blocks[j], out=blocks[j + 1], weighted=g.normalize, rowmax=rowmax,
                rowmax_mode=1 if (j == 0 and not rowmax_has_block0) else 2)


#: Cache the hop slab ``[x | A x | ... | A^K x]`` (+ row maxima) of TAGConv layers whose input
#: needs no gradient - the FIRST layer of each branch (``models/model.py:71,77`` with the raw
#: ``graph.x``): it is a parameter-free function of (x, edge_index), so it is computed once per
#: batch (by the first forward, or ahead of time by ``precompute_input_hops`` on the loader's
#: stream) instead of once per step.  Keyed on the input tensor's address + version and stored on
#: the ``GraphIndex`` (i.e. dropped with the topology); under stream capture the same rule as for
#: the adjacency applies (``graph.graph_index``).  ``DC_HOP_CACHE=0`` disables.
HOP_CACHE = os.environ.get("DC_HOP_CACHE", "1") != "0"
_HOP_CACHE_ENTRIES = 2


def _hop_cache_key(x: torch.Tensor, k: int, wpad: int, want_rowmax: bool):
    return (x.data_ptr(), tuple(x.shape), tuple(x.stride()), int(k), int(wpad), bool(want_rowmax))


def _hop_cache_get(g, key, x, dev):
    """(slab, rowmax) cached for this input tensor in its CURRENT state, or None."""
    cache = getattr(g, "_hop_cache", None)
    if not cache or key not in cache:
        return None
    cid = capture_id(dev)
    slab, rowmax, ecid, _ref, version = cache[key]
    if version == x._version and (ecid == cid or (cid != 0 and g._static_ok)):
        return slab, rowmax
    return None


def _hop_cache_put(g, key, x, slab, rowmax, dev):
    cache = g.__dict__.setdefault("_hop_cache", {})
    if key not in cache:
        while len(cache) >= _HOP_CACHE_ENTRIES:
            cache.pop(next(iter(cache)))
    # x kept alive: its address is part of the key
    cache[key] = (slab, rowmax, capture_id(dev), x, x._version)


#: pack + first hop of a narrow layer's input in one launch (``dc_spmm_f32_pack``); ``DC_FUSED_PACK=0``: two launches
FUSED_PACK = os.environ.get("DC_FUSED_PACK", "1") != "0"


def _build_input_slab(g: GraphIndex, x: torch.Tensor, k: int, want_rowmax: bool, into=None, nimg=None):
    """Pack ``x`` into block 0 of a ``[N, wpad]`` slab (fresh, or the buffers ``into`` = (slab,
    rowmax) of an earlier call) and run the K hops (+ row maxima).  ``nimg``: the ``_NarrowImage`` of the layer this
    slab is for - the fused pack launch fills it on the side."""
    n, fi = x.shape
    concat, width, wpad = tag_slab_geometry(fi, k)
    dev = x.device
    slab = into[0] if into is not None else _alloc_slab(n, wpad, dev)
    xin = x if (x.dim() == 2 and x.stride(1) == 1) else x.contiguous()
    adj = g.fwd if (g is not None and k >= 1) else None
    if (FUSED_PACK and adj is not None and not want_rowmax and fi <= 32 and not adj.row_offset and g.normalize
            and adj.ptr.numel() == n + 1):
        # the packing pass and the first hop in one launch (the chain of small dependent kernels a new batch starts with)
        args = (adj.ptr.data_ptr(), adj.other.data_ptr(), adj.w.data_ptr(), xin.data_ptr(), xin.stride(0),
                slab.data_ptr(), slab.stride(0), n, fi, width, wpad)
        if nimg is not None and not nimg.filled and len(nimg.ws) == k + 1:
            _lib.check(_lib.lib().dc_spmm_f32_pack_wprep(*args, _ptr_array(nimg.ws), k + 1, nimg.buf.data_ptr(),
                                                         current_stream_ptr(dev)), "dc_spmm_f32_pack_wprep")
            nimg.filled = True
        else:
            _lib.check(_lib.lib().dc_spmm_f32_pack(*args, current_stream_ptr(dev)), "dc_spmm_f32_pack")
        for j in range(1, k):
            hop(adj, slab[:, j * fi:(j + 1) * fi], out=slab[:, (j + 1) * fi:(j + 2) * fi], weighted=True)
        return slab, None
    _lib.check(_lib.lib().dc_tag_pack_input(xin.data_ptr(), xin.stride(0), slab.data_ptr(), slab.stride(0), n,
                                            fi, width, wpad, current_stream_ptr(dev)),
               "dc_tag_pack_input")
    rowmax = None
    if want_rowmax:
        rowmax = into[1] if into is not None else torch.empty(n, dtype=torch.float32, device=dev)
    chained_hops(g, slab, fi, k, backward=False, rowmax=rowmax)
    return slab, rowmax


def _tag_uses_h2(fi: int, k: int, fo: Optional[int] = None) -> bool:
    """Does a TAGConv layer of these widths run its dense blocks on the fp16x2 kernels (``DENSE_F16X2``)?  K = 0 layers
    (``dense_linear``: the ``lin`` of GCNConv / GATConv, the attention heads' Linear, the decoder) do too: no hop
    records their row maxima, so a ``dc_rowabsmax_f32`` pass over the input is added (8 us for [32768, 256]) and three
    MFMA products replace six.  From 128 input columns on, outputs a multiple of 16 wide (the 256 -> 3 output layer
    stays on the six-product split); ``fo`` None: a K = 0 layer that asked for six products."""
    concat, _, wpad = tag_slab_geometry(fi, k)
    ok = (DENSE_F16X2 and DENSE_SPLIT_BF16 and DENSE_PRODUCTS == 6 and not concat and fi % 16 == 0 and wpad % 4 == 0)
    if k >= 1:
        return ok
    return ok and fo is not None and fi >= 128 and fi % 32 == 0 and fo % 16 == 0 and fo >= 64


def precompute_input_hops(g: GraphIndex, x: torch.Tensor, k: int = 3) -> None:
    """Compute and cache, on the current stream, the hop slab a ``TAGConv(in, out, K=k)`` layer
    will need for the no-grad input ``x`` over topology ``g`` (what ``loaders.PrefetchLoader`` does
    for the next batch while the current one trains).

    Refilled static inputs are not refreshed in place: they rebuild their slabs inside the captured step, as ``bench.py``
    does (recomputing INTO cached buffers freed one that a captured graph still wrote to,
    ``profiles/r05/j_refresh_mode_memory_fault.txt``)."""
    _require_cuda(x, "x")
    if not HOP_CACHE or k < 1 or x.dtype != torch.float32 or x.dim() != 2:
        return
    fi = x.size(1)
    want = _tag_uses_h2(fi, k)
    key = _hop_cache_key(x, k, tag_slab_geometry(fi, k)[2], want)
    if _hop_cache_get(g, key, x, x.device) is None:
        slab, rowmax = _build_input_slab(g, x, k, want)
        _hop_cache_put(g, key, x, slab, rowmax, x.device)


def _grad_sink(p):
    """The ``dp.GradBucket`` that owns ``p.grad`` in direct mode, or None."""
    ref = getattr(p, "_dc_grad_sink", None)
    bucket = ref() if ref is not None else None
    if bucket is None or not p.requires_grad:
        return None
    g = p.grad
    if (g is None or g.dtype != torch.float32 or not g.is_contiguous() or g.device != p.device
            or g.shape != p.shape or not bucket.owns(p, g)):
        return None
    return bucket


def _direct_sink(params, needed):
    """The ``dp.GradBucket`` a backward kernel may accumulate the gradients of ``params`` into directly
    (``DIRECT_PARAM_GRAD``): autograd is not recording, every one of them is ``needed`` and every ``.grad`` is a view
    of that one bucket - else None.  The caller writes through ``p.grad`` and reports it (``note_direct_write``)."""
    if not (DIRECT_PARAM_GRAD and not torch.is_grad_enabled() and all(needed)):
        return None
    sinks = [_grad_sink(p) for p in params]
    return sinks[0] if all(s is sinks[0] for s in sinks) else None


def tag_slab_geometry(fi: int, k: int):
    """(concat, width, padded width) of the ``[N, (K+1)*Fi]`` hop slab of a TAGConv layer."""
    concat = (fi * (k + 1) <= 128) or (fi % 16 != 0)
    width = (k + 1) * fi
    wpad = (width + 15) // 16 * 16 if concat else width
    return concat, width, wpad


_SLAB_TAG = "_dc_hop_slab"

#: floats of padding behind every row of a hop slab whose row is a multiple of 1 KiB: with the natural
#: leading dimension (1024 floats = 4 KiB for the hidden-256 layers) the rows of a tile / the neighbour
#: rows of a hop sit a power of two apart and alias in the memory channels - measured on MI355X
#: (tools/exp/ld_pad.py, operands from beyond the Infinity Cache): F = 256 hop 20.7 -> 18.3 us, wide
#: forward block 92.6 -> 82.3 us with 64 floats (256 B) of padding; +16 / +80 floats (rows no longer
#: 128-byte aligned) give nothing.
SLAB_PAD = 64


def _alloc_slab(n: int, wpad: int, dev, tag=None) -> torch.Tensor:
    """``[n, wpad]`` view of a fresh row-major buffer whose leading dimension is padded off the power of
    two (``SLAB_PAD``); ``tag`` marks the BASE as a slab this library owns (``_as_slab_block0``)."""
    pad = SLAB_PAD if (SLAB_PAD > 0 and (wpad * 4) % 1024 == 0) else 0
    base = torch.empty((n, wpad + pad), dtype=torch.float32, device=dev)
    if tag is not None:
        setattr(base, _SLAB_TAG, tag)
    return base[:, :wpad] if pad else base


_SLAB_CLAIMED = "_dc_hop_slab_claimed"


def _as_slab_block0(x: torch.Tensor, n: int, fi: int, wpad: int):
    """If ``x`` is column block 0 of a ``[n, wpad]`` hop slab THIS LIBRARY allocated for it (the
    previous layer's forward wrote its output there and tagged the buffer) and no layer has adopted
    that slab yet, claim it and return it (a ``[n, wpad]`` view of the possibly row-padded buffer);
    else None.  Shape and stride alone are not enough: a caller's own ``feat[:, :fi]`` view of a wider
    tensor looks the same, and the hops would overwrite its other columns.  One adoption per slab: a
    second consumer of the same output (two heads, two edge sets, one conv applied twice) would write
    its hops over the ones the first saved for backward - the raw kernels bump no version counter, so
    autograd would not notice - and packs a slab of its own instead."""
    base = x._base
    if (base is not None and getattr(base, _SLAB_TAG, None) == (n, fi, wpad)
            and not getattr(base, _SLAB_CLAIMED, False)
            and base.dim() == 2 and base.size(0) == n and base.size(1) >= wpad
            and base.is_contiguous() and x.stride() == (base.size(1), 1) and x.shape == (n, fi)
            and x.data_ptr() == base.data_ptr() and base.dtype == torch.float32):
        setattr(base, _SLAB_CLAIMED, True)
        return base[:, :wpad] if base.size(1) > wpad else base
    return None


def _h2_weight_prep(L, ws, k: int, fo: int, fi: int, want_t: bool, dev, st, zero: Optional[torch.Tensor] = None):
    """``dc_tag_weight_prep(_zero)``: row maxima and scaled fp16x2 image of the layer's weights over the concatenated
    reduction, the same for the transposed weights (``want_t``: the forward-shaped dX block), and - on the side -
    ``zero`` cleared.  -> (wmax, wimg, wt, wt_rowmax)."""
    width = (k + 1) * fi
    wmax = torch.empty(fo, dtype=torch.float32, device=dev)
    wimg = torch.empty((fo, width), dtype=torch.float32, device=dev)     # 4 B / element
    wt = wt_rowmax = None
    if want_t:
        wt = torch.empty((fi, (k + 1) * fo), dtype=torch.float32, device=dev)
        wt_rowmax = torch.empty(fi, dtype=torch.float32, device=dev)
    _lib.check(L.dc_tag_weight_prep_zero(_ptr_array(ws), k + 1, fo, fi, wmax.data_ptr(), wimg.data_ptr(), _ptr(wt),
                                         _ptr(wt_rowmax), _ptr(zero), zero.numel() if zero is not None else 0, st),
               "dc_tag_weight_prep")
    return wmax, wimg, wt, wt_rowmax


#: In the backward of a wide layer dW needs the masked gradient and the forward's slab only - not the transposed hop chain,
#: not dX - so its place in the sequence mask -> chain -> dX is free.  With both encoder branches running the same sequence
#: on two streams the two ``k_dw_h2w`` launches run side by side - two launches of one 512-thread workgroup per CU each - and
#: take 151 us together where they take 49 + 66 us one after the other (``profiles/r05/w_step_timeline_headline_*.txt``).
#: Staggered: dW between chain and dX everywhere EXCEPT on the streams listed here (``graphnet.ContactEncoder`` registers the
#: side stream its rigid branch runs on), where it stays behind dX.  Measured, three boxes (``profiles/r05/x_dw_first.txt``):
#: 0.617 ms per step against 0.627 with both branches in the old order (dW in front of the chain on the soft branch: between
#: -7 and +5 us depending on the box; any other combination: slower).  Same kernels, same operands: same bits.
DW_LAST_STREAMS: set = set()
#: where dW goes in a wide layer's backward, by class of the current stream ("listed" = in DW_LAST_STREAMS): "first" (in front
#: of the transposed chain), "mid" (between chain and dX) or "last" (behind dX: the order of rounds 1 - 4 on both streams)
DW_POSITION = {"unlisted": "mid", "listed": "last"}


def _dw_position(dev) -> str:
    return DW_POSITION["listed" if current_stream_ptr(dev) in DW_LAST_STREAMS else "unlisted"]


def _pack_weights(ws, fo: int, fi: int, wpad: int, st) -> torch.Tensor:
    """``dc_tag_pack_weights``: the K+1 ``[Fo, Fi]`` weight blocks side by side, zero-padded to ``[Fo, wpad]``."""
    wcat = torch.empty((fo, wpad), dtype=torch.float32, device=ws[0].device)
    _lib.check(_lib.lib().dc_tag_pack_weights(_ptr_array(ws), len(ws), wcat.data_ptr(), fo, fi, wpad, st),
               "dc_tag_pack_weights")
    return wcat


def _dense_path(fi: int, k: int, fo: int, six: bool = False, narrow_ok: bool = False) -> str:
    """Which dense block runs a TAGConv / ``dense_linear`` layer of these widths, by the module switches as they are
    now.  "h2": fp16x2 planes, three products, one segment over the whole slab (``six``: the layer asked to stay off
    it).  "narrow": the short-reduction forward kernel of the first layers (``narrow_ok``: the answer of
    ``dc_tag_linear_fwd_narrow_ok``); its backward is that of "concat".  "concat": six-product bf16 split, ONE
    segment over the concatenated slab, zero-padded to a multiple of 16 (84 -> 96, 100 -> 112: aligned float4 loads,
    no K tail).  "split": the same kernels with the K+1 column blocks as separate segments.  "fp32": fp32 MFMA
    (``DENSE_SPLIT_BF16`` off), operands concatenated or not as ``tag_slab_geometry`` says."""
    if not DENSE_SPLIT_BF16:
        return "fp32"
    if _tag_uses_h2(fi, k, None if six else fo):
        return "h2"
    if not tag_slab_geometry(fi, k)[0]:
        return "split"
    return "narrow" if (NARROW_FWD and DENSE_PRODUCTS == 6 and narrow_ok) else "concat"


def _dense_operands(slab: torch.Tensor, fi: int, k: int, concat: bool):
    """(xs, ldxs, fi_eff, nseg): a ``[N, wpad]`` slab as the segment list of the dense blocks - the whole slab as
    one segment (``concat``) or its K+1 column blocks."""
    ld = slab.stride(0)
    if concat:
        return [slab], [ld], slab.size(1), 1
    return [slab[:, j * fi:(j + 1) * fi] for j in range(k + 1)], [ld] * (k + 1), fi, k + 1


def _tag_slab(g, x: torch.Tensor, weights, h2: bool, need_x: bool, nimg=None):
    """First step of a TAGConv layer's forward: the hop slab ``[x | A x | ... | A^K x]`` and, for the fp16x2 block
    (``h2``), its row maxima.  -> (slab, rowmax, prepped); ``prepped``: the layer's ``_h2_weight_prep`` where it had
    to be launched here already, else None.  ``nimg``: the layer's ``_NarrowImage``, for the pack launch to fill."""
    n, fi = x.shape
    k = len(weights) - 1
    dev = x.device
    wpad = tag_slab_geometry(fi, k)[2]
    slab = _as_slab_block0(x, n, fi, wpad)
    if slab is None and k == 0 and wpad == fi and x.is_contiguous() and x.data_ptr() % 16 == 0:
        slab = x                                 # no hops: the input itself is the (1-block) slab
    rowmax = prepped = None
    if slab is None:
        # the layer's own input: pack + K hops, or the cached slab when x needs no gradient
        key = None
        if HOP_CACHE and g is not None and k >= 1 and not need_x:
            key = _hop_cache_key(x, k, wpad, h2)
            hit = _hop_cache_get(g, key, x, dev)
            if hit is not None:
                slab, rowmax = hit
        if slab is None:
            slab, rowmax = _build_input_slab(g, x, k, h2, nimg=nimg)
            if key is not None:
                _hop_cache_put(g, key, x, slab, rowmax, dev)
    else:
        rowmax = torch.empty(n, dtype=torch.float32, device=dev) if h2 else None
        zeroed = False
        if h2 and g is not None and hop_chain_eligible(g, g.fwd, slab, fi, k):
            # the chain launch joins its row maxima into `rowmax` with atomics: the weight preparation - one launch
            # anyway, independent of the slab - clears it on the side (a memset node of its own: ~5 us per chain)
            fo = weights[0].size(0)
            prepped = _h2_weight_prep(_lib.lib(), [w.contiguous() for w in weights], k, fo, fi,
                                      need_x and fo % 16 == 0, dev, current_stream_ptr(dev), zero=rowmax)
            zeroed = True
        chained_hops(g, slab, fi, k, backward=False, rowmax=rowmax, rowmax_zeroed=zeroed)
    if h2 and k == 0:
        rowmax = rowabsmax(slab)                 # no hop has recorded the rows' maxima: one pass over the input
    return slab, rowmax, prepped


def _tag_out_buffer(next_geom, n: int, fo: int, dev) -> torch.Tensor:
    """Second step: where the layer's ``[N, Fo]`` output goes (``next_geom`` of ``tag_conv``)."""
    if isinstance(next_geom, OutInto):
        # rows of a buffer the caller owns (a part's rows of block 0 of a MERGED hop slab: both encoder branches
        # feed one grouped layer)
        out = next_geom.view
        if out.shape != (n, fo) or out.stride(1) != 1 or out.dtype != torch.float32 or out.device != dev:
            raise ValueError("tag_conv: out_into view has the wrong shape / layout")
        return out
    if next_geom is None:
        return torch.empty((n, fo), dtype=torch.float32, device=dev)
    # the output IS column block 0 of the next TAGConv layer's hop slab (no copy there)
    next_width, next_wpad = next_geom
    nxt = _alloc_slab(n, next_wpad, dev, tag=(n, fo, next_wpad))   # recognised by _as_slab_block0
    if next_wpad > next_width:
        nxt[:, next_width:].zero_()          # K padding of a narrow next layer
    return nxt[:, :fo]


def _tag_weight_gradients(ctx, slab, g: torch.Tensor, mask_ptr, ldm: int, g_rowmax=None, xrowmax=None):
    """dW + bias gradient of a ``_TagConvFn`` layer from the gradient ``g`` (masked by the output at ``mask_ptr``
    unless that is None) and the forward's slab: one output block per ``lins[k].weight`` in either layout of the
    dense block.  -> (gws, gb) for autograd; all None where the kernel wrote into the parameters' bucket."""
    k, fi, fo = ctx.k, ctx.fi, ctx.fo
    need_ws, need_b = ctx.needs_input_grad[5:], ctx.has_bias and ctx.needs_input_grad[2]
    gws: List[Optional[torch.Tensor]] = [None] * (k + 1)
    if not (any(need_ws) or need_b):
        return gws, None
    L = _lib.lib()
    n, dev = slab.size(0), slab.device
    st = current_stream_ptr(dev)
    bucket = _direct_sink(list(ctx.params) + ([ctx.bias_param] if ctx.has_bias else []),
                          list(need_ws) + [need_b or not ctx.has_bias])
    if bucket is not None:
        outs = [p.grad for p in ctx.params]
        gb_out = ctx.bias_param.grad if ctx.has_bias else None
    else:
        outs = [torch.empty((fo, fi), dtype=torch.float32, device=dev) for _ in range(k + 1)]
        gb_out = torch.empty(fo, dtype=torch.float32, device=dev) if need_b else None
    xs, ldxs, fi_eff, nseg = _dense_operands(slab, fi, k, ctx.concat)
    nbytes = L.dc_tag_linear_bwd_dw_workspace_bytes(n, fi_eff, fo, nseg)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    args = (g.data_ptr(), g.stride(0), mask_ptr, ldm, _ptr_array(xs), _i64_array(ldxs), nseg,
            _ptr_array(outs), k + 1, fi, _ptr(gb_out), int(bucket is not None), scratch.data_ptr(), nbytes,
            n, fi_eff, fo)
    if g_rowmax is not None and n % 16 == 0:
        rc = L.dc_tag_linear_bwd_dw_h2(*args, g_rowmax.data_ptr(), xrowmax.data_ptr(), st)
    elif ctx.path != "fp32":
        rc = L.dc_tag_linear_bwd_dw_split(*args, DENSE_PRODUCTS, st)
    else:
        rc = L.dc_tag_linear_bwd_dw(*args, st)
    _lib.check(rc, "dc_tag_linear_bwd_dw")
    if bucket is not None:
        bucket.note_direct_write(torch.cuda.current_stream(dev))
        return gws, None
    return [outs[j] if need_ws[j] else None for j in range(k + 1)], gb_out


def _tap_h2_backward(g, fi: int, fo: int, hop_rowmax, g_rowmax, gx, gslab) -> None:
    """The ``DEBUG_TAP`` calls of ``_tag_backward_h2`` (tools/exp/dp_flake2.py; ``HUNT_TAP_ADJ`` / ``HUNT_TAP_BIG``
    = 1 add the adjacency arrays / the big intermediates)."""
    DEBUG_TAP(f"bwd{fi}x{fo}.hop_rowmax", hop_rowmax)
    DEBUG_TAP(f"bwd{fi}x{fo}.g_rowmax", g_rowmax)
    if os.environ.get("HUNT_TAP_ADJ") == "1":
        for nm, t in (("bwd.ptr", g.bwd.ptr), ("bwd.other", g.bwd.other), ("bwd.w", g.bwd.w), ("fwd.ptr", g.fwd.ptr)):
            DEBUG_TAP(f"bwd{fi}x{fo}.adj.{nm}", t)
    if os.environ.get("HUNT_TAP_BIG") == "1":
        DEBUG_TAP(f"bwd{fi}x{fo}.gx", gx)
        DEBUG_TAP(f"bwd{fi}x{fo}.gslab", gslab)


def _tag_backward_h2(ctx, gout: torch.Tensor):
    """Backward of an fp16x2 layer, in the forward's shape: gx = sum_j ((A^T)^j gm) W_j with gm = g * relu' - K
    transposed hops on gm (which also record the row maxima), then ONE dense block with the (K+1)*Fo reduction and
    the transposed weights.  gm and its row maxima also feed dW (no mask reads there), whose place in the sequence
    is ``_dw_position``'s.  -> (gx, gws, gb)."""
    slab, out, xrowmax, wt, wt_rowmax, *ws = ctx.saved_tensors
    g, k, fi, fo = ctx.g, ctx.k, ctx.fi, ctx.fo
    L = _lib.lib()
    n, dev = slab.size(0), slab.device
    st = current_stream_ptr(dev)
    need_x = ctx.needs_input_grad[1]
    ldm = out.stride(0) if out is not None else fo
    gwid = (k + 1) * fo
    gslab = _alloc_slab(n, gwid, dev)
    gld = gslab.stride(0)
    g_rowmax = torch.empty(n, dtype=torch.float32, device=dev)
    hop_rowmax = torch.empty(n, dtype=torch.float32, device=dev) if need_x else None
    # (folding this pass into the transposed chain's staging was built and measured - bit-identical, one launch and
    # 100 MB less, and 0 - 2 % SLOWER on the step: this pass runs in the shadow of the other branch's dense blocks,
    # the chain launch does not; tools/exp/hopchain_masked.hip keeps the kernel)
    _lib.check(L.dc_tag_mask_grad(gout.data_ptr(), gout.stride(0), _ptr(out), ldm, gslab.data_ptr(), gld, n, fo,
                                  g_rowmax.data_ptr(), _ptr(hop_rowmax), st), "dc_tag_mask_grad")

    def weight_gradients():
        return _tag_weight_gradients(ctx, slab, gslab, None, ldm, g_rowmax, xrowmax)

    dw_pos = _dw_position(dev)
    if not need_x:
        return (None, *weight_gradients())
    # dW needs gm (block 0) and the forward's slab only - not the transposed chain: "first" puts it in FRONT of chain
    # + dX, "mid" between them, so that the two encoder branches' dW kernels do not run side by side (DW_LAST_STREAMS)
    grads = weight_gradients() if dw_pos == "first" else None
    chained_hops(g, gslab, fo, k, backward=False, rowmax=hop_rowmax, transposed=True, rowmax_has_block0=True)
    if dw_pos == "mid":
        grads = weight_gradients()
    if wt is None:                       # forward ran without needs_input_grad
        wt = torch.empty((fi, gwid), dtype=torch.float32, device=dev)
        wt_rowmax = torch.empty(fi, dtype=torch.float32, device=dev)
        _lib.check(L.dc_tag_weight_prep(_ptr_array(ws), k + 1, fo, fi, torch.empty(fo, device=dev).data_ptr(), None,
                                        wt.data_ptr(), wt_rowmax.data_ptr(), st), "dc_tag_weight_prep")
    gx = torch.empty((n, fi), dtype=torch.float32, device=dev)
    rc = L.dc_tag_linear_fwd_h2p(gslab.data_ptr(), gld, wt.data_ptr(), None, 0, gx.data_ptr(), fi, n, gwid, fi,
                                 hop_rowmax.data_ptr(), wt_rowmax.data_ptr(), None, 0, st)
    _lib.check(rc, "dc_tag_linear_fwd_h2 (dX)")
    if DEBUG_TAP is not None:
        _tap_h2_backward(g, fi, fo, hop_rowmax, g_rowmax, gx, gslab)
    if grads is None:
        grads = weight_gradients()
    return (gx, *grads)


def _tag_backward_generic(ctx, gout: torch.Tensor):
    """Backward of every other layer: one dW kernel (+ bias gradient), one dX kernel writing the per-hop gradient
    slab, K transposed hops that fold it into block 0.  -> (gx, gws, gb)."""
    slab, out, _, _, _, *ws = ctx.saved_tensors
    k, fi, fo = ctx.k, ctx.fi, ctx.fo
    L = _lib.lib()
    n, dev = slab.size(0), slab.device
    st = current_stream_ptr(dev)
    mask_ptr, ldm = _ptr(out), (out.stride(0) if out is not None else fo)
    gws, gb = _tag_weight_gradients(ctx, slab, gout, mask_ptr, ldm)
    if not ctx.needs_input_grad[1]:
        return None, gws, gb
    wpad = slab.size(1)
    if ctx.path == "narrow":
        # the forward read the lins[k].weight matrices directly; the one-segment dX block wants them concatenated
        ws = [_pack_weights(ws, fo, fi, wpad, st)]
    gslab = _alloc_slab(n, wpad, dev)
    gxs, ldgs, fi_eff, nseg = _dense_operands(gslab, fi, k, ctx.concat)
    if ctx.path != "fp32":
        wsb = L.dc_tag_linear_bwd_dx_split_workspace_bytes(fi_eff, fo, nseg)
        wsx = torch.empty(wsb, dtype=torch.uint8, device=dev)
        rc = L.dc_tag_linear_bwd_dx_split(gout.data_ptr(), gout.stride(0), mask_ptr, ldm, _ptr_array(ws), nseg,
                                          _ptr_array(gxs), _i64_array(ldgs), wsx.data_ptr(), wsb, n, fi_eff, fo,
                                          DENSE_PRODUCTS, st)
    else:
        rc = L.dc_tag_linear_bwd_dx(gout.data_ptr(), gout.stride(0), mask_ptr, ldm, _ptr_array(ws), nseg,
                                    _ptr_array(gxs), _i64_array(ldgs), n, fi_eff, fo, st)
    _lib.check(rc, "dc_tag_linear_bwd_dx")
    chained_hops(ctx.g, gslab, fi, k, backward=True)  # g_{j-1} = G_{j-1} + A^T g_j
    return gslab[:, :fi], gws, gb


class _TagConvFn(torch.autograd.Function):
    """Whole TAGConv layer (+ optional fused ReLU): K hops into one ``[N, (K+1)*Fi]`` slab, then ONE dense kernel
    (``_dense_path``) for ``act(x W_0^T + sum_k (A^k x) W_k^T + b)`` - PyG ``tag_conv.py`` forward followed by
    ``F.relu`` (``models/model.py:71,77``).  Backward: ``_tag_backward_h2`` / ``_tag_backward_generic``."""

    @staticmethod
    def forward(ctx, g: GraphIndex, x: torch.Tensor, bias: Optional[torch.Tensor], relu: bool,
                next_geom, *weights):
        n, fi = x.shape
        k = len(weights) - 1
        fo = weights[0].size(0)
        if k + 1 > MAX_SEG:
            raise NotImplementedError(f"TAGConv K={k} > {MAX_SEG - 1} is not supported by the fused dense block")
        dev = x.device
        L = _lib.lib()
        st = current_stream_ptr(dev)
        six = next_geom is SIX_PRODUCTS
        if six:
            next_geom = None
        ctx.empty = n == 0
        if ctx.empty:
            # no rows: nothing to launch (the kernels' entry points refuse the null pointers of empty tensors)
            ctx.fi, ctx.has_bias = fi, bias is not None
            ctx.save_for_backward(*weights)
            return _tag_out_buffer(next_geom, n, fo, dev)
        concat, width, wpad = tag_slab_geometry(fi, k)
        path = _dense_path(fi, k, fo, six, concat and bool(L.dc_tag_linear_fwd_narrow_ok(fi, k + 1, wpad, fo)))
        need_x = ctx.needs_input_grad[1]
        # the short-reduction kernel takes the lins[k].weight matrices themselves: their fragment image is made once per
        # call, by the pack launch of _tag_slab where there is one
        ws = [w.contiguous() for w in weights]
        nimg = _NarrowImage(ws, wpad, dev) if (path == "narrow" and NARROW_PREP) else None
        slab, rowmax, prepped = _tag_slab(g, x, weights, path == "h2", need_x, nimg)
        if concat and path != "narrow":
            ws = [_pack_weights(ws, fo, fi, wpad, st)]
        out = _tag_out_buffer(next_geom, n, fo, dev)
        ldo = out.stride(0)
        b = bias.contiguous() if bias is not None else None
        wt = wt_rowmax = None
        if path == "h2":
            # one launch: the weights scaled and split into their fp16 planes over the concatenated
            # reduction (the dense block runs as ONE segment over the whole slab and pulls them into
            # LDS by DMA), their row maxima and, when the input needs a gradient, the same for the
            # transposed weights (forward-shaped dX block)
            if prepped is None:
                prepped = _h2_weight_prep(L, ws, k, fo, fi, need_x and fo % 16 == 0, dev, st)
            wmax, wimg, wt, wt_rowmax = prepped
            rc = L.dc_tag_linear_fwd_h2p(slab.data_ptr(), slab.stride(0), wimg.data_ptr(), _ptr(b), int(relu),
                                         out.data_ptr(), ldo, n, width, fo, rowmax.data_ptr(), wmax.data_ptr(),
                                         None, 0, st)
        elif path == "narrow" and nimg is not None:
            rc = L.dc_tag_linear_fwd_narrow_img(slab.data_ptr(), slab.stride(0), nimg.ensure(st), _ptr(b), int(relu),
                                                out.data_ptr(), ldo, n, wpad, fo, st)
        elif path == "narrow":
            rc = L.dc_tag_linear_fwd_narrow(slab.data_ptr(), slab.stride(0), _ptr_array(ws), k + 1, fi, _ptr(b),
                                            int(relu), out.data_ptr(), ldo, n, wpad, fo, st)
        else:
            xs, ldxs, fi_eff, nseg = _dense_operands(slab, fi, k, concat)
            args = (_ptr_array(xs), _i64_array(ldxs), _ptr_array(ws), nseg, _ptr(b), int(relu), out.data_ptr(), ldo,
                    n, fi_eff, fo)
            rc = L.dc_tag_linear_fwd(*args, st) if path == "fp32" else L.dc_tag_linear_fwd_split(*args, DENSE_PRODUCTS, st)
        _lib.check(rc, "dc_tag_linear_fwd")
        ctx.g, ctx.k, ctx.fi, ctx.fo, ctx.has_bias, ctx.relu, ctx.concat, ctx.path = \
            g, k, fi, fo, bias is not None, relu, concat, path
        ctx.params, ctx.bias_param = weights, bias       # the Parameter objects themselves
        ctx.save_for_backward(slab, out if relu else None, rowmax, wt, wt_rowmax, *ws)
        return out

    @staticmethod
    def backward(ctx, gout):
        if ctx.empty:                        # sums over no rows: an empty dX, zero dW and bias gradient
            need = ctx.needs_input_grad
            ws = ctx.saved_tensors
            gx = gout.new_zeros((0, ctx.fi)) if need[1] else None
            gb = gout.new_zeros(gout.size(1)) if (ctx.has_bias and need[2]) else None
            return (None, gx, gb, None, None, *[torch.zeros_like(w) if need[5 + j] else None for j, w in enumerate(ws)])
        gout = _grad_layout(gout, 4)         # column-slice views (e.g. the dX slab) pass as is
        if ctx.path == "h2" and ctx.fo % 16 == 0:
            gx, gws, gb = _tag_backward_h2(ctx, gout)
        else:
            gx, gws, gb = _tag_backward_generic(ctx, gout)
        return (None, gx, gb, None, None, *gws)


class OutInto:
    """Destination of a layer's output chosen by the caller (``tag_conv(..., next_geom=OutInto(view))``):
    a ``[N, Fo]`` row-major view, e.g. one part's rows of block 0 of a merged hop slab.  A plain object, so
    autograd does not see the buffer as an input of the layer."""

    def __init__(self, view: torch.Tensor):
        self.view = view


# --------------------------------------------------------------------------- #
# grouped TAGConv layer: both encoder branches as ONE block-diagonal launch
# --------------------------------------------------------------------------- #
_MERGED_TAG = "_dc_merged_slab"


def alloc_merged_slab(mg: GraphIndex, fi: int, k: int, dev) -> torch.Tensor:
    """``[N_total, (K+1)*fi]`` hop slab over the merged node space of ``mg`` (``GraphIndex.from_parts``)
    for a grouped TAGConv layer, tagged so that ``tag_conv_grouped`` recognises the parts' block-0 views
    (``merged_slab_part``).  The padding rows of block 0 are zeroed here (their other blocks are written
    - as zeros - by the hops: padding nodes are isolated)."""
    concat, width, wpad = tag_slab_geometry(fi, k)
    if concat:
        raise ValueError("alloc_merged_slab: wide layers only (Fi a multiple of 16, (K+1)*Fi > 128)")
    n = mg.num_nodes
    slab = _alloc_slab(n, wpad, dev, tag=("merged", n, fi, wpad, tuple(mg.row_beg), tuple(mg.rows)))
    ends = list(mg.row_beg[1:]) + [n]
    for r0, rows, r1 in zip(mg.row_beg, mg.rows, ends):
        if r0 + rows < r1:
            slab[r0 + rows:r1, :fi].zero_()
    return slab


def merged_slab_part(slab: torch.Tensor, mg: GraphIndex, g: int, fi: int) -> torch.Tensor:
    """Rows of part ``g`` in column block 0 of a merged slab: where that part's previous layer writes."""
    r0 = mg.row_beg[g]
    return slab[r0:r0 + mg.rows[g], :fi]


def _as_merged_slab(xs, mg: GraphIndex, fi: int, wpad: int):
    """The merged slab whose block 0 the tensors ``xs`` (one per part) are the part views of, or None."""
    base = xs[0]._base
    tag = ("merged", mg.num_nodes, fi, wpad, tuple(mg.row_beg), tuple(mg.rows))
    if base is None or getattr(base, _SLAB_TAG, None) != tag or base.dim() != 2 or not base.is_contiguous():
        return None
    ld = base.size(1)
    for g, x in enumerate(xs):
        if (x._base is not base or x.shape != (mg.rows[g], fi) or x.stride() != (ld, 1)
                or x.data_ptr() != base.data_ptr() + 4 * ld * mg.row_beg[g]):
            return None
    return base[:, :wpad] if ld > wpad else base


def grouped_eligible(fi: int, fo: int, k: int) -> bool:
    """Can ``tag_conv_grouped`` run a layer of these widths (the grouped kernels' shape limits)?"""
    return (_tag_uses_h2(fi, k) and fi == 256 and fo % 128 == 0 and fo % 16 == 0
            and ((k + 1) * fi) % 32 == 0 and ((k + 1) * fo) % 32 == 0)


class _TagConvGroupedFn(torch.autograd.Function):
    """The same TAGConv layer (+ fused ReLU) of SEVERAL branches - same widths, each branch its own
    weights - over the merged node space of ``mg``: K hops over the merged adjacency (one launch each for
    all branches), ONE grouped forward block, and in backward one grouped mask kernel, K transposed merged
    hops, one grouped forward-shaped dX block, one grouped dW block + slab reduce
    (``dc_tag_grouped_*``).  Replaces the second ``conv(x, edge_index)`` call of both encoder loops of
    ``models/model.py:69-78``.  Row by row the arithmetic is that of ``_TagConvFn`` on each branch alone:
    outputs and gradients are bit-identical to it.

    ``apply(mg, relu, next_geom, ngroups, x_0..x_{G-1}, bias_0, W_0,0..W_0,K, bias_1, W_1,0.., ...)``
    returns one output per group (views of one merged buffer)."""

    @staticmethod
    def forward(ctx, mg: GraphIndex, relu: bool, next_geom, ngroups: int, *args):
        xs = args[:ngroups]
        per = (len(args) - ngroups) // ngroups
        k = per - 2
        biases = [args[ngroups + g * per] for g in range(ngroups)]
        weights = [list(args[ngroups + g * per + 1: ngroups + (g + 1) * per]) for g in range(ngroups)]
        fo, fi = weights[0][0].shape
        dev = xs[0].device
        n = mg.num_nodes
        concat, width, wpad = tag_slab_geometry(fi, k)
        if not _tag_uses_h2(fi, k) or width % 32 != 0 or any(b is None for b in biases) != all(b is None for b in biases):
            raise NotImplementedError("tag_conv_grouped: wide fp16x2 layers only, bias on all groups or none")
        L = _lib.lib()
        st = current_stream_ptr(dev)
        slab = _as_merged_slab(xs, mg, fi, wpad)
        if slab is None:
            slab = alloc_merged_slab(mg, fi, k, dev)
            for g, x in enumerate(xs):
                merged_slab_part(slab, mg, g, fi).copy_(x)
        rowmax = torch.empty(n, dtype=torch.float32, device=dev)
        chained_hops(mg, slab, fi, k, backward=False, rowmax=rowmax)
        # weights of all groups: scaled fp16x2 images (+ transposed images for dX) in one launch
        need_x = any(ctx.needs_input_grad[4:4 + ngroups])
        wmax = torch.empty((ngroups, fo), dtype=torch.float32, device=dev)
        wimg = torch.empty((ngroups, fo, width), dtype=torch.float32, device=dev)
        wt = wt_rowmax = None
        if need_x and fo % 16 == 0:
            wt = torch.empty((ngroups, fi, (k + 1) * fo), dtype=torch.float32, device=dev)
            wt_rowmax = torch.empty((ngroups, fi), dtype=torch.float32, device=dev)
        wcs = [[w.contiguous() for w in ws] for ws in weights]
        wmax_p, wimg_p = _ptr_array(list(wmax)), _ptr_array(list(wimg))
        _lib.check(L.dc_tag_grouped_weight_prep(
            _ptr_array([w for ws in wcs for w in ws]), ngroups, k + 1, fo, fi, wmax_p, wimg_p,
            _ptr_array(list(wt)) if wt is not None else None,
            _ptr_array(list(wt_rowmax)) if wt is not None else None, st), "dc_tag_grouped_weight_prep")
        if isinstance(next_geom, tuple):
            nxt = alloc_merged_slab(mg, fo, next_geom[0], dev)      # next grouped layer's slab: (K_next,)
            out = nxt[:, :fo]
        else:
            out = torch.empty((n, fo), dtype=torch.float32, device=dev)
        bcs = [b.contiguous() if b is not None else None for b in biases]
        row_beg, rows = _i64_array(mg.row_beg), _i64_array(mg.rows)
        _lib.check(L.dc_tag_grouped_fwd_h2p(
            slab.data_ptr(), slab.stride(0), ngroups, row_beg, rows, n, wimg_p, _vp_array([_ptr(b) for b in bcs]),
            int(relu), out.data_ptr(), out.stride(0), width, fo, rowmax.data_ptr(), wmax_p, st), "dc_tag_grouped_fwd_h2p")
        ctx.mg, ctx.k, ctx.fi, ctx.fo, ctx.relu, ctx.ngroups = mg, k, fi, fo, relu, ngroups
        ctx.params, ctx.bias_params = weights, biases
        ctx.save_for_backward(slab, out if relu else None, rowmax, wt, wt_rowmax)
        outs = tuple(out[r0:r0 + r] for r0, r in zip(mg.row_beg, mg.rows))
        return outs

    @staticmethod
    def backward(ctx, *gouts):
        slab, out, xrowmax, wt, wt_rowmax = ctx.saved_tensors
        mg, k, fi, fo, ngroups = ctx.mg, ctx.k, ctx.fi, ctx.fo, ctx.ngroups
        L = _lib.lib()
        dev = slab.device
        st = current_stream_ptr(dev)
        n = mg.num_nodes
        per = k + 2
        need_x = any(ctx.needs_input_grad[4:4 + ngroups])
        need_p = any(ctx.needs_input_grad[4 + ngroups:])
        gs = []
        for g, go in enumerate(gouts):
            if go is None:
                go = torch.zeros((mg.rows[g], fo), dtype=torch.float32, device=dev)
            gs.append(_grad_layout(go, 4))
        row_beg, rows = _i64_array(mg.row_beg), _i64_array(mg.rows)
        gwid = (k + 1) * fo
        gslab = _alloc_slab(n, gwid, dev)
        g_rowmax = torch.empty(n, dtype=torch.float32, device=dev)
        hop_rowmax = torch.empty(n, dtype=torch.float32, device=dev) if need_x else None
        _lib.check(L.dc_tag_grouped_mask_grad(
            _ptr_array(gs), _i64_array([t.stride(0) for t in gs]), ngroups, row_beg, rows, n,
            _ptr(out), out.stride(0) if out is not None else fo, gslab.data_ptr(), gslab.stride(0), fo,
            g_rowmax.data_ptr(), _ptr(hop_rowmax), st), "dc_tag_grouped_mask_grad")
        gxs = [None] * ngroups
        if need_x:
            if wt is None:
                raise RuntimeError("tag_conv_grouped: input gradient requested but the forward ran without it")
            chained_hops(mg, gslab, fo, k, backward=False, rowmax=hop_rowmax, transposed=True,
                         rowmax_has_block0=True)
            gx = torch.empty((n, fi), dtype=torch.float32, device=dev)
            _lib.check(L.dc_tag_grouped_fwd_h2p(
                gslab.data_ptr(), gslab.stride(0), ngroups, row_beg, rows, n,
                _ptr_array(list(wt)), None, 0, gx.data_ptr(), fi, gwid, fi, hop_rowmax.data_ptr(),
                _ptr_array(list(wt_rowmax)), st), "dc_tag_grouped_fwd_h2p (dX)")
            gxs = [gx[r0:r0 + r] if ctx.needs_input_grad[4 + g] else None
                   for g, (r0, r) in enumerate(zip(mg.row_beg, mg.rows))]
        pgrads = [None] * (ngroups * per)
        if need_p:
            has_bias = ctx.bias_params[0] is not None
            flat_params = [p for g in range(ngroups) for p in ([ctx.bias_params[g]] if has_bias else []) + ctx.params[g]]
            bucket = _direct_sink(flat_params, [ctx.needs_input_grad[4 + ngroups + g * per + j] for g in range(ngroups)
                                                for j in range(per) if (j > 0 or has_bias)])
            direct = bucket is not None
            if direct:
                gw_out = [[p.grad for p in ctx.params[g]] for g in range(ngroups)]
                gb_out = [ctx.bias_params[g].grad if has_bias else None for g in range(ngroups)]
            else:
                gw_out = [[torch.empty((fo, fi), dtype=torch.float32, device=dev) for _ in range(k + 1)]
                          for _ in range(ngroups)]
                gb_out = [torch.empty(fo, dtype=torch.float32, device=dev) if has_bias else None
                          for _ in range(ngroups)]
            nbytes = L.dc_tag_grouped_bwd_dw_workspace_bytes(rows, ngroups, fi, fo, k + 1)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            xblocks = [slab[:, j * fi:(j + 1) * fi] for j in range(k + 1)]
            _lib.check(L.dc_tag_grouped_bwd_dw_h2(
                gslab.data_ptr(), gslab.stride(0), _ptr_array(xblocks), _i64_array([slab.stride(0)] * (k + 1)),
                k + 1, ngroups, row_beg, rows, n, _ptr_array([t for ws in gw_out for t in ws]),
                _vp_array([_ptr(t) for t in gb_out]), int(direct), scratch.data_ptr(), nbytes, fi, fo,
                g_rowmax.data_ptr(), xrowmax.data_ptr(), st), "dc_tag_grouped_bwd_dw_h2")
            if direct:
                bucket.note_direct_write(torch.cuda.current_stream(dev))
            else:
                for g in range(ngroups):
                    base = g * per
                    if has_bias and ctx.needs_input_grad[4 + ngroups + base]:
                        pgrads[base] = gb_out[g]
                    for j in range(k + 1):
                        if ctx.needs_input_grad[4 + ngroups + base + 1 + j]:
                            pgrads[base + 1 + j] = gw_out[g][j]
        return (None, None, None, None, *gxs, *pgrads)


def tag_conv_grouped(mg: GraphIndex, xs, weights, biases, relu: bool = False, next_k=None):
    """One TAGConv layer of ``len(xs)`` branches over the merged adjacency ``mg``: ``xs[g]`` ``[rows_g, Fi]``,
    ``weights[g]`` = that branch's ``lins[0..K].weight``, ``biases[g]`` its bias.  Returns one output per
    branch.  ``next_k``: K of a grouped layer that consumes the outputs - they are then written as the part
    views of block 0 of that layer's merged slab."""
    flat = []
    xs = [resolve(x) for x in xs]
    for b, ws in zip(biases, weights):
        flat += [b] + list(ws)
    return _TagConvGroupedFn.apply(mg, bool(relu), (int(next_k),) if next_k is not None else None, len(xs),
                                   *xs, *flat)


class _SixProducts:
    """``next_geom`` marker of ``dense_linear(..., six_products=True)``."""


SIX_PRODUCTS = _SixProducts()


def dense_linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                 relu: bool = False, six_products: bool = False) -> torch.Tensor:
    """``act(x @ weight.T + bias)`` on the library's dense block (a TAGConv layer with K = 0: no hops):
    the ``lin`` of ``GCNConv`` / ``GATConv`` (PyG ``nn/dense/linear.py``), forward and backward.
    ``six_products``: stay on the exact three-way bf16 split (24 bits) where the three-product fp16 split (22 bits)
    would apply - GATConv's ``lin``: the gradient of its attention vectors is a sum of terms that cancel to 1 % of
    their size and sits at the parity bar already."""
    return _TagConvFn.apply(None, resolve(x), bias, bool(relu), SIX_PRODUCTS if six_products else None, weight)


def tag_conv(g: GraphIndex, x: torch.Tensor, weights, bias, relu: bool = False,
             next_geom=None) -> torch.Tensor:
    """``next_geom``: ``(width, padded width)`` of the hop slab of the TAGConv layer that consumes
    this output (None = none): the output is then allocated as column block 0 of that slab."""
    return _TagConvFn.apply(g, resolve(x), bias, bool(relu), next_geom, *weights)


# --------------------------------------------------------------------------- #
# TAGConv over bf16-stored features (BASELINE.json configs[4]): forward + backward
# --------------------------------------------------------------------------- #
_SLAB_TAG_BF16 = "_dc_hop_slab_bf16"


def _alloc_bf16(rows: int, wid: int, dev, tag=None) -> torch.Tensor:
    pad = 2 * SLAB_PAD if (SLAB_PAD > 0 and (wid * 2) % 1024 == 0) else 0      # same byte padding as fp32
    b = torch.empty((rows, wid + pad), dtype=torch.bfloat16, device=dev)
    if tag is not None:
        setattr(b, _SLAB_TAG_BF16, tag)
    return b[:, :wid] if pad else b


class _TagConvBf16Fn(torch.autograd.Function):
    """``TAGConv.forward`` (+ optional ReLU) with the features STORED as bfloat16 and fp32 master weights.
    Forward: K hops ``dc_spmm_bf16`` (bf16 rows gathered, fp32 running sum in the stable edge order, one rounding per
    stored element) into a ``[N, (K+1) * Fi]`` bf16 slab, then ONE bf16 MFMA dense block
    (``dc_tag_linear_fwd_bf16``, fp32 accumulate) with the weights rounded to bf16.  Backward, in the forward's
    shape: ``gm = g * relu'`` as bf16 (``dc_tag_mask_grad_bf16``), K TRANSPOSED bf16 hops on gm, the same dense
    block over that gradient slab with the transposed weights for ``gx``, and ``dc_tag_linear_bwd_dw_bf16`` for the
    fp32 weight / bias gradients.  What PyG reaches under ``torch.autocast(bfloat16)``, with every aggregation and
    every contraction accumulated in fp32."""

    @staticmethod
    def forward(ctx, g: GraphIndex, x: torch.Tensor, bias, relu: bool, out_dtype, next_k, *weights):
        n, fi = x.shape
        k = len(weights) - 1
        fo = weights[0].size(0)
        width = (k + 1) * fi
        dev = x.device
        L = _lib.lib()
        st = current_stream_ptr(dev)
        base = x._base
        if (base is not None and getattr(base, _SLAB_TAG_BF16, None) == (n, fi, width)
                and base.size(0) == n and base.size(1) >= width and base.is_contiguous()
                and x.data_ptr() == base.data_ptr() and x.stride() == (base.size(1), 1)):
            slab = base[:, :width] if base.size(1) > width else base   # the previous layer wrote block 0 in place
        else:
            slab = _alloc_bf16(n, width, dev)
            slab[:, :fi].copy_(x)
        for j in range(k):
            hop_bf16(g.fwd, slab[:, j * fi:(j + 1) * fi], out=slab[:, (j + 1) * fi:(j + 2) * fi],
                     weighted=g.normalize, out_dtype=torch.bfloat16)
        ws = [w.detach().contiguous() for w in weights]
        wcat = torch.empty((fo, width), dtype=torch.bfloat16, device=dev)
        _lib.check(L.dc_to_bf16(_ptr_array(ws), k + 1, fo, fi, fi, wcat.data_ptr(), width, st), "dc_to_bf16")
        if next_k is not None and out_dtype == torch.bfloat16:
            nwidth = (next_k + 1) * fo
            nxt = _alloc_bf16(n, nwidth, dev, tag=(n, fo, nwidth))
            out = nxt[:, :fo]
        else:
            out = torch.empty((n, fo), dtype=out_dtype, device=dev)
        b = bias.detach().contiguous() if bias is not None else None
        rc = L.dc_tag_linear_fwd_bf16(slab.data_ptr(), slab.stride(0), wcat.data_ptr(), _ptr(b), int(relu),
                                      out.data_ptr(), out.stride(0), int(out.dtype == torch.bfloat16), n, width, fo, st)
        _lib.check(rc, "dc_tag_linear_fwd_bf16")
        ctx.g, ctx.k, ctx.fi, ctx.fo, ctx.relu, ctx.has_bias, ctx.x_dtype = g, k, fi, fo, relu, bias is not None, x.dtype
        ctx.save_for_backward(slab, out if relu else None, *ws)
        return out

    @staticmethod
    def backward(ctx, gout):
        slab, out, *ws = ctx.saved_tensors
        g, k, fi, fo = ctx.g, ctx.k, ctx.fi, ctx.fo
        n, dev = slab.size(0), slab.device
        L = _lib.lib()
        st = current_stream_ptr(dev)
        if gout.dtype not in (torch.bfloat16, torch.float32):
            gout = gout.float()
        gout = _grad_layout(gout, 1)
        need_x = ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        need_w = any(ctx.needs_input_grad[6:])
        gwid = (k + 1) * fo
        gslab = _alloc_bf16(n, gwid if need_x else fo, dev)
        _lib.check(L.dc_tag_mask_grad_bf16(
            gout.data_ptr(), gout.stride(0), int(gout.dtype == torch.bfloat16),
            _ptr(out), out.stride(0) if out is not None else fo,
            int(out is not None and out.dtype == torch.bfloat16), gslab.data_ptr(), gslab.stride(0), n, fo, st),
            "dc_tag_mask_grad_bf16")
        gx = gb = None
        gws = [None] * (k + 1)
        if need_x:
            if gwid % 32 != 0 or fo % 8 != 0:
                raise NotImplementedError("tag_conv_bf16 backward: (K+1)*Fo must be a multiple of 32")
            for j in range(k):
                hop_bf16(g.bwd, gslab[:, j * fo:(j + 1) * fo], out=gslab[:, (j + 1) * fo:(j + 2) * fo],
                         weighted=g.normalize, out_dtype=torch.bfloat16)
            wt = torch.empty((k + 1, fi, fo), dtype=torch.float32, device=dev)
            _lib.check(L.dc_tag_transpose_weights(_ptr_array(ws), k + 1, fo, fi, wt.data_ptr(), st),
                       "dc_tag_transpose_weights")
            wtcat = torch.empty((fi, gwid), dtype=torch.bfloat16, device=dev)
            _lib.check(L.dc_to_bf16(_ptr_array([wt[j] for j in range(k + 1)]), k + 1, fi, fo, fo,
                                    wtcat.data_ptr(), gwid, st), "dc_to_bf16")
            gx = torch.empty((n, fi), dtype=ctx.x_dtype, device=dev)
            _lib.check(L.dc_tag_linear_fwd_bf16(gslab.data_ptr(), gslab.stride(0), wtcat.data_ptr(), None, 0,
                                                gx.data_ptr(), fi, int(gx.dtype == torch.bfloat16), n, gwid, fi, st),
                       "dc_tag_linear_fwd_bf16 (dX)")
        if need_w or need_b:
            outs = [torch.empty((fo, fi), dtype=torch.float32, device=dev) for _ in range(k + 1)]
            gb_out = torch.empty(fo, dtype=torch.float32, device=dev) if need_b else None
            nbytes = L.dc_tag_linear_bwd_dw_bf16_workspace_bytes(n, fi, fo, k + 1)
            if nbytes < 0:
                raise NotImplementedError("tag_conv_bf16 backward: unsupported layer shape")
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.check(L.dc_tag_linear_bwd_dw_bf16(
                gslab.data_ptr(), gslab.stride(0), slab.data_ptr(), slab.stride(0), k + 1, _ptr_array(outs),
                _ptr(gb_out), 0, scratch.data_ptr(), nbytes, n, fi, fo, st),
                "dc_tag_linear_bwd_dw_bf16")
            gws = [outs[j] if ctx.needs_input_grad[6 + j] else None for j in range(k + 1)]
            gb = gb_out
        return (None, gx, gb, None, None, None, *gws)


def tag_conv_bf16(g: GraphIndex, x: torch.Tensor, weights, bias, relu: bool = False,
                  out_dtype: torch.dtype = torch.bfloat16, next_k: Optional[int] = None) -> torch.Tensor:
    """``TAGConv.forward`` (+ optional ReLU) over bfloat16-STORED features, differentiable w.r.t. ``x`` and the
    (fp32) parameters (``_TagConvBf16Fn``).  ``next_k``: K of the bf16 TAGConv layer that consumes the output - it is
    then written as column block 0 of that layer's slab (bf16 output only)."""
    _require_cuda(x, "x")
    if x.dtype != torch.bfloat16 or x.dim() != 2:
        raise ValueError("tag_conv_bf16: x must be a 2-D bfloat16 tensor")
    fi = x.size(1)
    k = len(weights) - 1
    if ((k + 1) * fi) % 32 != 0 or fi % 8 != 0:
        raise ValueError(f"tag_conv_bf16: (K+1)*Fi = {(k + 1) * fi} must be a multiple of 32 and Fi of 8")
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("tag_conv_bf16: out_dtype must be bfloat16 or float32")
    grad = torch.is_grad_enabled() and (x.requires_grad or any(w.requires_grad for w in weights)
                                        or (bias is not None and bias.requires_grad))
    fo = weights[0].size(0)
    if grad and (fo % 128 != 0 or fi % 256 != 0):
        raise NotImplementedError("tag_conv_bf16: the backward needs Fo % 128 == 0 and Fi % 256 == 0 "
                                  "(call under torch.no_grad() for other widths)")
    return _TagConvBf16Fn.apply(g, x, bias, bool(relu), out_dtype, next_k, *weights)


# --------------------------------------------------------------------------- #
# GATConv (heads = 1): edge softmax + weighted aggregation
# --------------------------------------------------------------------------- #
def _gat_edge_softmax(g: GraphIndex, a_src: torch.Tensor, a_dst: torch.Tensor, slope: float, n: int) -> torch.Tensor:
    """``alpha[p] = softmax over the edges into i of leaky_relu(a_src[j] + a_dst[i])``, in ``g.fwd`` order."""
    alpha = torch.zeros(max(g.capacity, 1), dtype=torch.float32, device=a_src.device)
    _lib.check(_lib.lib().dc_gat_edge_softmax_fwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), a_src.data_ptr(),
                                                  a_dst.data_ptr(), slope, alpha.data_ptr(), n,
                                                  current_stream_ptr(a_src.device)), "dc_gat_edge_softmax_fwd")
    return alpha


def _gat_edge_backward(g: GraphIndex, gm, h, a_src, a_dst, alpha, slope: float):
    """Backward of ``out = sum_j alpha_ij h_j`` with ``alpha`` = ``_gat_edge_softmax``, from the gradient ``gm`` of
    ``out``: -> (gh, g_a_src, g_a_dst)."""
    L = _lib.lib()
    n, f = h.shape
    dev = h.device
    st = current_stream_ptr(dev)
    cap = max(g.capacity, 1)
    b2f = g.bwd_to_fwd()
    cnt = g.fwd.ptr[-1:]
    # d out / d h : transposed aggregation with alpha re-ordered by source
    alpha_b = torch.zeros(cap, dtype=torch.float32, device=dev)
    _lib.check(L.dc_gather_f32(alpha.data_ptr(), b2f.data_ptr(), alpha_b.data_ptr(), cnt.data_ptr(), g.capacity, st),
               "dc_gather_f32")
    gh = _spmm(g.bwd, alpha_b, gm)
    # d out / d alpha, through the softmax, summed per source
    galpha = torch.zeros(cap, dtype=torch.float32, device=dev)
    _lib.check(L.dc_sddmm_f32(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), gm.data_ptr(), f, h.data_ptr(), f,
                              galpha.data_ptr(), n, f, st), "dc_sddmm_f32")
    ge = torch.zeros(cap, dtype=torch.float32, device=dev)
    g_a_dst = torch.empty(n, dtype=torch.float32, device=dev)
    _lib.check(L.dc_gat_edge_softmax_bwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), a_src.data_ptr(),
                                         a_dst.data_ptr(), slope, alpha.data_ptr(), galpha.data_ptr(),
                                         ge.data_ptr(), g_a_dst.data_ptr(), n, st), "dc_gat_edge_softmax_bwd")
    g_a_src = torch.empty(n, dtype=torch.float32, device=dev)
    _lib.check(L.dc_segment_sum_f32(g.bwd.ptr.data_ptr(), b2f.data_ptr(), ge.data_ptr(), g_a_src.data_ptr(), n, st),
               "dc_segment_sum_f32")
    return gh, g_a_src, g_a_dst


class _GatAggregateFn(torch.autograd.Function):
    """The unfused GATConv aggregation (edge softmax + weighted sum); ``_GatConvFn`` is the whole layer."""

    @staticmethod
    def forward(ctx, g: GraphIndex, h, a_src, a_dst, slope: float):
        h, a_src, a_dst = h.contiguous(), a_src.contiguous(), a_dst.contiguous()
        alpha = _gat_edge_softmax(g, a_src, a_dst, slope, h.size(0))
        out = _spmm(g.fwd, alpha, h)
        ctx.g, ctx.slope = g, slope
        ctx.save_for_backward(h, a_src, a_dst, alpha)
        return out

    @staticmethod
    def backward(ctx, gout):
        h, a_src, a_dst, alpha = ctx.saved_tensors
        gh, g_a_src, g_a_dst = _gat_edge_backward(ctx.g, _grad_layout(gout, 0), h, a_src, a_dst, alpha, ctx.slope)
        return None, gh, g_a_src, g_a_dst, None


def gat_aggregate(g: GraphIndex, h, a_src, a_dst, slope: float) -> torch.Tensor:
    return _GatAggregateFn.apply(g, h, a_src, a_dst, float(slope))


# --------------------------------------------------------------------------- #
# GCNConv / GATConv: aggregation + bias + ReLU as one node, row-wise passes fused (dc_gnn_epi.hip)
# --------------------------------------------------------------------------- #
FUSED_GNN_EPILOGUE = True          # (False: the unfused layer composition - tests compare the two)


def fused_gnn_ok(h: torch.Tensor) -> bool:
    """Widths / layouts the fused GCN / GAT layer kernels take (F % 4 == 0, F / 4 divides 256, aligned rows)."""
    f = h.size(1)
    return (FUSED_GNN_EPILOGUE and h.is_cuda and h.dtype == torch.float32 and f % 4 == 0 and 4 <= f <= 1024
            and 256 % (f // 4) == 0)


def _agg_bias_act(adj: SortedAdjacency, w: torch.Tensor, h: torch.Tensor, bias, relu: bool) -> torch.Tensor:
    n, f = h.shape
    y = torch.empty((n, f), dtype=torch.float32, device=h.device)
    _lib.check(_lib.lib().dc_spmm_f32_bias_act(adj.ptr.data_ptr(), adj.other.data_ptr(), w.data_ptr(), h.data_ptr(),
                                               _rowmajor(h, "h"), _ptr(bias), int(relu), y.data_ptr(), f, n, f,
                                               current_stream_ptr(h.device)), "dc_spmm_f32_bias_act")
    return y


def _mask_and_bias_grad(gy: torch.Tensor, y: Optional[torch.Tensor], bias_param, need_bias: bool):
    """gm = gy * (y > 0) (y None: gm is gy) and the bias gradient sum_i gm[i, :] in one pass.  The bias gradient
    goes straight into the bucket's view in direct mode (-> None), else it is returned."""
    n, f = gy.shape
    dev = gy.device
    if y is None and not need_bias:
        return gy, None
    L = _lib.lib()
    gm = torch.empty((n, f), dtype=torch.float32, device=dev) if y is not None else None
    sink = _direct_sink([bias_param], [need_bias and bias_param is not None])
    direct = sink is not None
    if need_bias:
        gb = bias_param.grad if direct else torch.empty(f, dtype=torch.float32, device=dev)
    else:
        gb = torch.empty(f, dtype=torch.float32, device=dev)         # (the kernel always forms it: one pass either way)
    nb = L.dc_colsum_workspace_bytes(n, f, 1)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
    _lib.check(L.dc_mask_colsum_f32(gy.data_ptr(), gy.stride(0), _ptr(y), y.stride(0) if y is not None else 0,
                                    _ptr(gm), gm.stride(0) if gm is not None else 0, n, f, ws.data_ptr(), ws.numel(),
                                    gb.data_ptr(), int(direct), current_stream_ptr(dev)), "dc_mask_colsum_f32")
    if direct:
        sink.note_direct_write(torch.cuda.current_stream(dev))
    return (gm if gm is not None else gy), (None if (direct or not need_bias) else gb)


class _ParamGrads:
    """Where a backward kernel writes the gradients of ``params``: ``bufs`` are flat views of their ``.grad`` when the
    kernel may accumulate there (``_direct_sink``; ``direct``), else fresh buffers.  ``done()`` behind the launch
    reports the direct write, or shapes the buffers like the parameters: what ``backward`` returns for them."""

    def __init__(self, params, needed, dev):
        self.params, self.dev = params, dev
        self.bucket = _direct_sink(params, needed)
        self.direct = self.bucket is not None
        self.bufs = [p.grad.view(-1) if self.direct else torch.empty(p.numel(), dtype=torch.float32, device=dev)
                     for p in params]

    def done(self):
        if self.direct:
            self.bucket.note_direct_write(torch.cuda.current_stream(self.dev))
            return [None] * len(self.params)
        return [b.view_as(p) for b, p in zip(self.bufs, self.params)]


class _GcnAggFn(torch.autograd.Function):
    """``act(A_hat h + bias)`` of a GCNConv layer (PyG gcn_conv.py: ``propagate`` + ``out + bias``, then the encoder's
    ReLU, models/model.py:71,77) as ONE aggregation launch; backward: mask + bias gradient in one pass, then the
    transposed aggregation."""

    @staticmethod
    def forward(ctx, g: GraphIndex, h, bias, relu: bool):
        h = h.contiguous()
        y = _agg_bias_act(g.fwd, g.fwd.w, h, bias, relu)
        ctx.g, ctx.relu, ctx.bias_param = g, relu, bias
        ctx.save_for_backward(y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gy = _grad_layout(gy, 0)
        need_b = ctx.bias_param is not None and ctx.needs_input_grad[2]
        gm, gb = _mask_and_bias_grad(gy, y, ctx.bias_param, need_b)
        gh = hop(ctx.g.bwd, gm, weighted=True) if ctx.needs_input_grad[1] else None
        return None, gh, gb, None


def gcn_aggregate(g: GraphIndex, h: torch.Tensor, bias, relu: bool = False) -> torch.Tensor:
    return _GcnAggFn.apply(g, resolve(h), bias, bool(relu))


class _GatConvFn(torch.autograd.Function):
    """Everything of a GATConv layer (heads = 1) behind its ``lin``: both attention dot products in one pass over h,
    edge softmax, ``act(sum_j a_ij h_j + bias)`` as one aggregation launch; backward: mask + bias gradient in one
    pass, transposed aggregation, SDDMM + softmax backward, and the dot products' backward (rank-one updates of dh
    and the two attention-vector gradients) in one pass (PyG gat_conv.py, utils/_softmax.py)."""

    @staticmethod
    def forward(ctx, g: GraphIndex, h, att_src, att_dst, bias, slope: float, relu: bool):
        L = _lib.lib()
        h = h.contiguous()
        n, f = h.shape
        dev = h.device
        st = current_stream_ptr(dev)
        a_s, a_d = att_src.reshape(-1).contiguous(), att_dst.reshape(-1).contiguous()
        a_src = torch.empty(n, dtype=torch.float32, device=dev)
        a_dst = torch.empty(n, dtype=torch.float32, device=dev)
        _lib.check(L.dc_gat_alpha_fwd(h.data_ptr(), f, a_s.data_ptr(), a_d.data_ptr(), a_src.data_ptr(),
                                      a_dst.data_ptr(), n, f, st), "dc_gat_alpha_fwd")
        alpha = _gat_edge_softmax(g, a_src, a_dst, slope, n)
        y = _agg_bias_act(g.fwd, alpha, h, bias, relu)
        ctx.g, ctx.slope, ctx.relu = g, slope, relu
        ctx.params = (att_src, att_dst, bias)
        ctx.save_for_backward(h, a_src, a_dst, alpha, a_s, a_d, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        L = _lib.lib()
        h, a_src, a_dst, alpha, a_s, a_d, y = ctx.saved_tensors
        g, slope = ctx.g, ctx.slope
        att_src, att_dst, bias = ctx.params
        gy = _grad_layout(gy, 0)
        n, f = h.shape
        dev = h.device
        st = current_stream_ptr(dev)
        need_b = bias is not None and ctx.needs_input_grad[4]
        gm, gb = _mask_and_bias_grad(gy, y, bias, need_b)
        gh, g_a_src, g_a_dst = _gat_edge_backward(g, gm, h, a_src, a_dst, alpha, slope)
        # the attention dot products' backward: gh += ga_src att_src + ga_dst att_dst, the two vector gradients
        pg = _ParamGrads([att_src, att_dst], ctx.needs_input_grad[2:4], dev)
        gs, gd = pg.bufs
        nb = L.dc_colsum_workspace_bytes(n, f, 2)
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
        _lib.check(L.dc_gat_alpha_bwd(h.data_ptr(), f, g_a_src.data_ptr(), g_a_dst.data_ptr(), a_s.data_ptr(),
                                      a_d.data_ptr(), gh.data_ptr(), f, n, f, ws.data_ptr(), ws.numel(), gs.data_ptr(),
                                      gd.data_ptr(), int(pg.direct), st), "dc_gat_alpha_bwd")
        gs, gd = pg.done()
        return None, gh, gs, gd, gb, None, None


def gat_conv(g: GraphIndex, h, att_src, att_dst, bias, slope: float, relu: bool = False) -> torch.Tensor:
    return _GatConvFn.apply(g, resolve(h), att_src, att_dst, bias, float(slope), bool(relu))


# --------------------------------------------------------------------------- #
# GATConv with several heads (dc_gat_heads.hip): h is [N, H*C], per-node vectors [N, H], per-edge vectors
# [capacity, H] edge-major in g.fwd order.  One launcher per C entry.
# --------------------------------------------------------------------------- #
def _heads_alpha_fwd(h, a_s, a_d, nh: int, c: int):
    """(a_src, a_dst) [N, H]: both attention dot products of every head in one pass over ``h``."""
    n, dev = h.size(0), h.device
    a_src = torch.empty((n, nh), dtype=torch.float32, device=dev)
    a_dst = torch.empty((n, nh), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dc_gat_alpha_heads_fwd(h.data_ptr(), _rowmajor(h, "h"), a_s.data_ptr(), a_d.data_ptr(),
                                                 a_src.data_ptr(), a_dst.data_ptr(), n, nh, c, current_stream_ptr(dev)),
               "dc_gat_alpha_heads_fwd")
    return a_src, a_dst


def _heads_edge_vector(g: GraphIndex, nh: int, dev) -> torch.Tensor:
    return torch.zeros((max(g.capacity, 1), nh), dtype=torch.float32, device=dev)


def _heads_softmax_fwd(g: GraphIndex, a_src, a_dst, slope: float, n: int, nh: int) -> torch.Tensor:
    alpha = _heads_edge_vector(g, nh, a_src.device)
    _lib.check(_lib.lib().dc_gat_edge_softmax_heads_fwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), a_src.data_ptr(),
                                                        a_dst.data_ptr(), slope, alpha.data_ptr(), n, nh,
                                                        current_stream_ptr(a_src.device)), "dc_gat_edge_softmax_heads_fwd")
    return alpha


def _heads_agg(adj: SortedAdjacency, alpha, x, bias, relu: bool, mean: bool, nh: int, c: int) -> torch.Tensor:
    """``act(sum_p alpha[p, head] x[other[p]] + bias)`` at width H*C, or its mean over heads at width C."""
    n, dev = x.size(0), x.device
    y = torch.empty((n, c if mean else nh * c), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dc_spmm_f32_heads_bias_act(adj.ptr.data_ptr(), adj.other.data_ptr(), alpha.data_ptr(),
                                                     x.data_ptr(), _rowmajor(x, "x"), _ptr(bias), int(relu), int(mean),
                                                     y.data_ptr(), y.size(1), n, nh, c, current_stream_ptr(dev)),
               "dc_spmm_f32_heads_bias_act")
    return y


def _heads_sddmm(g: GraphIndex, gm, h, nh: int, c: int) -> torch.Tensor:
    galpha = _heads_edge_vector(g, nh, h.device)
    _lib.check(_lib.lib().dc_sddmm_f32_heads(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), gm.data_ptr(),
                                             _rowmajor(gm, "gm"), h.data_ptr(), _rowmajor(h, "h"), galpha.data_ptr(),
                                             h.size(0), nh, c, current_stream_ptr(h.device)), "dc_sddmm_f32_heads")
    return galpha


def _heads_softmax_bwd(g: GraphIndex, a_src, a_dst, slope: float, alpha, galpha, n: int, nh: int):
    dev = alpha.device
    ge = _heads_edge_vector(g, nh, dev)
    g_a_dst = torch.empty((n, nh), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dc_gat_edge_softmax_heads_bwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), a_src.data_ptr(),
                                                        a_dst.data_ptr(), slope, alpha.data_ptr(), galpha.data_ptr(),
                                                        ge.data_ptr(), g_a_dst.data_ptr(), n, nh,
                                                        current_stream_ptr(dev)), "dc_gat_edge_softmax_heads_bwd")
    return ge, g_a_dst


def _heads_segment_sum(ptr, index_map, v, n: int, w: int) -> torch.Tensor:
    out = torch.empty((n, w), dtype=torch.float32, device=v.device)
    _lib.check(_lib.lib().dc_segment_sum_f32_heads(ptr.data_ptr(), _ptr(index_map), v.data_ptr(), out.data_ptr(), n, w,
                                                   current_stream_ptr(v.device)), "dc_segment_sum_f32_heads")
    return out


def _heads_gather(g: GraphIndex, v, idx, w: int) -> torch.Tensor:
    """``out[p, :] = v[idx[p], :]`` for the edges the adjacency holds (counted on the device, ``g.fwd.ptr[-1]``)."""
    out = _heads_edge_vector(g, w, v.device)
    _lib.check(_lib.lib().dc_gather_f32_heads(v.data_ptr(), idx.data_ptr(), out.data_ptr(), g.fwd.ptr[-1:].data_ptr(),
                                              g.capacity, w, current_stream_ptr(v.device)), "dc_gather_f32_heads")
    return out


def _heads_spread(gm, nh: int, c: int) -> torch.Tensor:
    """The gradient of the mean over heads: ``out[i, k*C + c] = gm[i, c] / H``."""
    n, dev = gm.size(0), gm.device
    out = torch.empty((n, nh * c), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dc_spread_heads_f32(gm.data_ptr(), _rowmajor(gm, "gm"), out.data_ptr(), nh * c, n, nh, c,
                                              current_stream_ptr(dev)), "dc_spread_heads_f32")
    return out


def _heads_out_grad(ctx, gy, y, bias):
    """How the multi-head backward passes open: ``gy`` in a layout the kernels take, the ReLU mask and the bias
    gradient in one pass (``bias`` is input 4 of every one of them), and - the heads averaged - the gradient spread to
    the heads.  -> (gm [N, H*C], gb)."""
    gy = _grad_layout(gy, 0)
    gm, gb = _mask_and_bias_grad(gy, y, bias, bias is not None and ctx.needs_input_grad[4])
    if ctx.mean:
        gm = _heads_spread(gm, ctx.nh, ctx.c)
    return gm, gb


def _heads_alpha_bwd(h, g_a_src, g_a_dst, a_s, a_d, gh, nh: int, c: int, gs, gd, accumulate: bool) -> None:
    n, f, dev = h.size(0), nh * c, h.device
    L = _lib.lib()
    ws = torch.empty(max(L.dc_colsum_workspace_bytes(n, f, 2), 16), dtype=torch.uint8, device=dev)
    _lib.check(L.dc_gat_alpha_heads_bwd(h.data_ptr(), f, g_a_src.data_ptr(), g_a_dst.data_ptr(), a_s.data_ptr(),
                                        a_d.data_ptr(), gh.data_ptr(), f, n, nh, c, ws.data_ptr(), ws.numel(),
                                        gs.data_ptr(), gd.data_ptr(), int(accumulate), current_stream_ptr(dev)),
               "dc_gat_alpha_heads_bwd")


def _gat_heads_edge_backward(g: GraphIndex, gm, h, a_src, a_dst, alpha, slope: float, nh: int, c: int, a_edge=None):
    """``_gat_edge_backward`` for H heads, from the gradient ``gm`` [N, H*C] of the concatenated aggregation:
    -> (gh [N, H*C], g_a_src [N, H], g_a_dst [N, H], ge [capacity, H]); ``a_edge``: the logits' per-edge addend."""
    n = h.size(0)
    b2f = g.bwd_to_fwd()
    # d out / d h : transposed aggregation with alpha re-ordered by source, H floats per edge
    gh = _heads_agg(g.bwd, _heads_gather(g, alpha, b2f, nh), gm, None, False, False, nh, c)
    # d out / d alpha, through the softmax, summed per source
    galpha = _heads_sddmm(g, gm, h, nh, c)
    if a_edge is None:
        ge, g_a_dst = _heads_softmax_bwd(g, a_src, a_dst, slope, alpha, galpha, n, nh)
    else:
        ge, g_a_dst = _edge_softmax_bwd(g, a_src, a_dst, a_edge, slope, alpha, galpha, n, nh)
    return gh, _heads_segment_sum(g.bwd.ptr, b2f, ge, n, nh), g_a_dst, ge


class _GatHeadsAggregateFn(torch.autograd.Function):
    """The unfused multi-head aggregation (edge softmax + weighted sum per head, concatenated or averaged over the
    heads): the sibling of ``_GatAggregateFn``; ``_GatHeadsConvFn`` is the whole layer."""

    @staticmethod
    def forward(ctx, g: GraphIndex, h, a_src, a_dst, slope: float, nh: int, mean: bool):
        h, a_src, a_dst = h.contiguous(), a_src.contiguous(), a_dst.contiguous()
        c = h.size(1) // nh
        alpha = _heads_softmax_fwd(g, a_src, a_dst, slope, h.size(0), nh)
        out = _heads_agg(g.fwd, alpha, h, None, False, mean, nh, c)
        ctx.g, ctx.slope, ctx.nh, ctx.c, ctx.mean = g, slope, nh, c, mean
        ctx.save_for_backward(h, a_src, a_dst, alpha)
        return out

    @staticmethod
    def backward(ctx, gout):
        h, a_src, a_dst, alpha = ctx.saved_tensors
        gm = _grad_layout(gout, 0)
        if ctx.mean:
            gm = _heads_spread(gm, ctx.nh, ctx.c)
        gh, g_a_src, g_a_dst, _ = _gat_heads_edge_backward(ctx.g, gm, h, a_src, a_dst, alpha, ctx.slope, ctx.nh, ctx.c)
        return None, gh, g_a_src, g_a_dst, None, None, None


def gat_heads_aggregate(g: GraphIndex, h, a_src, a_dst, slope: float, heads: int, mean: bool = False,
                        edge_attr=None, edge_m=None, fill_value="mean") -> torch.Tensor:
    """``h`` [N, H*C], ``a_src`` / ``a_dst`` [N, H] -> [N, H*C], or [N, C] with ``mean`` (PyG ``concat=False``).
    ``edge_attr`` [E, D] with the folded ``edge_m`` [D, H] (``gat_edge_fold``): the logits' edge-feature term."""
    h = resolve(h)
    if h.dim() != 2 or heads < 1 or h.size(1) % heads or a_src.shape != (h.size(0), heads) or a_dst.shape != a_src.shape:
        raise ValueError("gat_heads_aggregate: h must be [N, H*C] and a_src / a_dst [N, H]")
    if edge_attr is None:
        return _GatHeadsAggregateFn.apply(g, h, a_src, a_dst, float(slope), int(heads), bool(mean))
    edge_attr, fill_mean, fill = _edge_operands(g, edge_attr, edge_m, int(heads), fill_value)
    return _GatHeadsEdgeAggregateFn.apply(g, h, a_src, a_dst, float(slope), int(heads), bool(mean), edge_attr, edge_m,
                                          fill_mean, fill)


def gat_heads_fused_ok(h: torch.Tensor, heads: int, mean: bool) -> bool:
    """Widths the row-wise passes of ``gat_heads_conv`` take: ``fused_gnn_ok`` at H*C, and at C - the width of the
    output, where the mask and the bias gradient are formed - when the heads are averaged."""
    return fused_gnn_ok(h) and (not mean or fused_gnn_ok(h[:, :h.size(1) // heads]))


class _GatHeadsConvFn(torch.autograd.Function):
    """Everything of a multi-head GATConv layer behind its ``lin`` - ``_GatConvFn`` with H weights per edge: the dot
    products of all heads in one pass over h, edge softmax, ``act(aggregation + bias)`` (concatenated, or the mean over
    the heads) as one launch that gathers every neighbour row once; backward: mask + bias gradient in one pass, (mean:
    the gradient spread to the heads,) transposed aggregation, SDDMM + softmax backward, and the dot products' backward
    with the two ``[H, C]`` attention gradients in one pass."""

    @staticmethod
    def forward(ctx, g: GraphIndex, h, att_src, att_dst, bias, slope: float, relu: bool, nh: int, mean: bool):
        h = h.contiguous()
        n, f = h.shape
        c = f // nh
        a_s, a_d = att_src.reshape(-1).contiguous(), att_dst.reshape(-1).contiguous()
        a_src, a_dst = _heads_alpha_fwd(h, a_s, a_d, nh, c)
        alpha = _heads_softmax_fwd(g, a_src, a_dst, slope, n, nh)
        y = _heads_agg(g.fwd, alpha, h, bias, relu, mean, nh, c)
        ctx.g, ctx.slope, ctx.relu, ctx.nh, ctx.c, ctx.mean = g, slope, relu, nh, c, mean
        ctx.params = (att_src, att_dst, bias)
        ctx.save_for_backward(h, a_src, a_dst, alpha, a_s, a_d, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        h, a_src, a_dst, alpha, a_s, a_d, y = ctx.saved_tensors
        g, slope, nh, c = ctx.g, ctx.slope, ctx.nh, ctx.c
        att_src, att_dst, bias = ctx.params
        gm, gb = _heads_out_grad(ctx, gy, y, bias)
        gh, g_a_src, g_a_dst, _ = _gat_heads_edge_backward(g, gm, h, a_src, a_dst, alpha, slope, nh, c)
        # the attention dot products' backward: gh += ga_src att_src + ga_dst att_dst per head, the two [H, C] gradients
        pg = _ParamGrads([att_src, att_dst], ctx.needs_input_grad[2:4], h.device)
        _heads_alpha_bwd(h, g_a_src, g_a_dst, a_s, a_d, gh, nh, c, *pg.bufs, pg.direct)
        gs, gd = pg.done()
        return None, gh, gs, gd, gb, None, None, None, None


def gat_heads_conv(g: GraphIndex, h, att_src, att_dst, bias, slope: float, relu: bool = False, heads: int = 1,
                   mean: bool = False) -> torch.Tensor:
    """The layer behind ``lin`` for ``heads`` >= 1 (``h`` [N, H*C], ``att_*`` [1, H, C]; ``gat_heads_fused_ok``)."""
    h = resolve(h)
    if h.dim() != 2 or heads < 1 or h.size(1) != att_src.numel() or att_src.numel() % heads:
        raise ValueError("gat_heads_conv: h must be [N, H*C] and att_src / att_dst [1, H, C]")
    return _GatHeadsConvFn.apply(g, h, att_src, att_dst, bias, float(slope), bool(relu), int(heads), bool(mean))


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


# --------------------------------------------------------------------------- #
# GATConv with edge features (dc_gat_edge.hip; the softmax with the per-edge addend shares dc_gat_heads.hip's templates).
# The edge term <lin_edge(edge_attr[p])[k, :], att_edge[k, :]> is linear in edge_attr: a_edge = edge_attr @ M with the
# folded M [D, H] formed by ordinary torch ops OUTSIDE the Functions below, so autograd turns their gM into the
# gradients of lin_edge.weight and att_edge.  One launcher per C entry.
# --------------------------------------------------------------------------- #
GAT_EDGE_MAX_DIM = 64              # DC_GAT_EDGE_MAX_DIM of include/deformcontact.h


def gat_edge_fold(lin_edge_weight: torch.Tensor, att_edge: torch.Tensor) -> torch.Tensor:
    """``M[d, k] = sum_c lin_edge.weight[k C + c, d] att_edge[k, c]`` ([D, H]; differentiable, D*H*C flops)."""
    _, nh, c = att_edge.shape
    return (lin_edge_weight.view(nh, c, -1) * att_edge.view(nh, c, 1)).sum(1).t().contiguous()


def gat_edge_fill(fill_value):
    """``fill_value`` of the appended self loops' attribute -> (mean?, constant): ``"mean"`` or a Python number."""
    if isinstance(fill_value, str):
        if fill_value != "mean":
            raise ValueError(f"fill_value must be 'mean' or a float, got {fill_value!r}")
        return True, 0.0
    if isinstance(fill_value, bool) or not isinstance(fill_value, (int, float)):
        raise ValueError(f"fill_value must be 'mean' or a float, got {fill_value!r}")
    return False, float(fill_value)


def _edge_operands(g: GraphIndex, edge_attr, m, nh: int, fill_value):
    """Checked operands of the edge-feature kernels: ``edge_attr`` float32 [E, D] with inner stride 1 on the graph's
    device, ``m`` [D, H], the graph a plain self-loop adjacency (its ``perm`` holds this ``edge_index``'s edge ids)."""
    fill_mean, fill = gat_edge_fill(fill_value)
    if m is None or m.dim() != 2 or m.size(1) != nh:
        raise ValueError("edge_m must be the folded [edge_dim, heads] matrix (ops.gat_edge_fold)")
    d = m.size(0)
    if not 1 <= d <= GAT_EDGE_MAX_DIM:
        raise ValueError(f"edge_dim = {d}: the edge-feature kernels take 1 <= edge_dim <= {GAT_EDGE_MAX_DIM}")
    if not isinstance(g, GraphIndex) or g.parts is not None or not g.self_loops:
        raise ValueError("edge features need the layer's own self-loop adjacency of this edge_index (not a merged one)")
    _require_cuda(edge_attr, "edge_attr")
    if edge_attr.dtype != torch.float32:
        raise ValueError(f"edge_attr must be float32, got {edge_attr.dtype}")
    if edge_attr.dim() == 1 and d == 1:
        edge_attr = edge_attr.unsqueeze(-1)
    if edge_attr.dim() != 2 or edge_attr.size(1) != d:
        raise ValueError(f"edge_attr must be [E, {d}] (edge_dim = {d}), got {tuple(edge_attr.shape)}")
    if edge_attr.size(0) != g.num_input_edges:
        raise ValueError(f"edge_attr has {edge_attr.size(0)} rows for {g.num_input_edges} edges")
    if edge_attr.device != g.device:
        raise RuntimeError(f"edge_attr is on {edge_attr.device} but the graph is on {g.device}")
    if edge_attr.stride(1) != 1 or (edge_attr.size(0) > 1 and edge_attr.stride(0) < d):
        edge_attr = edge_attr.contiguous()                       # (a row stride is taken as it is)
    return edge_attr, fill_mean, fill


def _edge_lda(edge_attr) -> int:
    return edge_attr.stride(0) if edge_attr.size(0) > 1 else edge_attr.size(1)


def _edge_term_fwd(g: GraphIndex, edge_attr, m, fill_mean: bool, fill: float, n: int, nh: int):
    """(a_edge [capacity, H] in ``g.fwd`` order, loop_attr [N, D]: the attribute row of every appended self loop)"""
    dev, d = m.device, m.size(0)
    a_edge = _heads_edge_vector(g, nh, dev)
    loop_attr = torch.empty((n, d), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dc_gat_edge_attr_fwd(g.fwd.ptr.data_ptr(), g.fwd.perm.data_ptr(), _ptr(edge_attr) or None,
                                               _edge_lda(edge_attr), m.data_ptr(), int(fill_mean), fill,
                                               a_edge.data_ptr(), loop_attr.data_ptr(), n, g.num_input_edges, d, nh,
                                               current_stream_ptr(dev)), "dc_gat_edge_attr_fwd")
    return a_edge, loop_attr


def _edge_softmax_fwd(g: GraphIndex, a_src, a_dst, a_edge, slope: float, n: int, nh: int) -> torch.Tensor:
    alpha = _heads_edge_vector(g, nh, a_src.device)
    _lib.check(_lib.lib().dc_gat_edge_attr_softmax_fwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), a_src.data_ptr(),
                                                       a_dst.data_ptr(), a_edge.data_ptr(), slope, alpha.data_ptr(), n, nh,
                                                       current_stream_ptr(a_src.device)), "dc_gat_edge_attr_softmax_fwd")
    return alpha


def _edge_softmax_bwd(g: GraphIndex, a_src, a_dst, a_edge, slope: float, alpha, galpha, n: int, nh: int):
    dev = alpha.device
    ge = _heads_edge_vector(g, nh, dev)
    g_a_dst = torch.empty((n, nh), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dc_gat_edge_attr_softmax_bwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), a_src.data_ptr(),
                                                       a_dst.data_ptr(), a_edge.data_ptr(), slope, alpha.data_ptr(),
                                                       galpha.data_ptr(), ge.data_ptr(), g_a_dst.data_ptr(), n, nh,
                                                       current_stream_ptr(dev)), "dc_gat_edge_attr_softmax_bwd")
    return ge, g_a_dst


def _edge_term_bwd(g: GraphIndex, ge, edge_attr, loop_attr, m, fill_mean: bool, n: int, nh: int, need_attr: bool,
                   need_m: bool):
    """(g_edge_attr [E, D] or None, gM [D, H] or None) from ``ge``, the gradient of the logits (= of a_edge)."""
    if not (need_attr or need_m):
        return None, None
    L = _lib.lib()
    dev, d, e = m.device, m.size(0), g.num_input_edges
    g_attr = torch.empty((e, d), dtype=torch.float32, device=dev) if need_attr else None
    g_m = torch.empty((d, nh), dtype=torch.float32, device=dev) if need_m else None
    ws = torch.empty(max(L.dc_gat_edge_attr_bwd_workspace_bytes(g.capacity, d, nh), 16), dtype=torch.uint8, device=dev)
    _lib.check(L.dc_gat_edge_attr_bwd(g.fwd.ptr.data_ptr(), g.fwd.perm.data_ptr(), ge.data_ptr(), _ptr(edge_attr) or None,
                                      _edge_lda(edge_attr), loop_attr.data_ptr(), m.data_ptr(), int(fill_mean),
                                      _ptr(g_attr) or None, d, _ptr(g_m), n, e, d, nh, g.capacity, ws.data_ptr(),
                                      ws.numel(), current_stream_ptr(dev)), "dc_gat_edge_attr_bwd")
    return g_attr, g_m


class _GatHeadsEdgeAggregateFn(torch.autograd.Function):
    """``_GatHeadsAggregateFn`` with the edge-feature term in the logits: the unfused aggregation at the widths
    ``gat_heads_fused_ok`` does not take."""

    @staticmethod
    def forward(ctx, g: GraphIndex, h, a_src, a_dst, slope: float, nh: int, mean: bool, edge_attr, m, fill_mean: bool,
                fill: float):
        h, a_src, a_dst, m = h.contiguous(), a_src.contiguous(), a_dst.contiguous(), m.contiguous()
        n, c = h.size(0), h.size(1) // nh
        a_edge, loop_attr = _edge_term_fwd(g, edge_attr, m, fill_mean, fill, n, nh)
        alpha = _edge_softmax_fwd(g, a_src, a_dst, a_edge, slope, n, nh)
        out = _heads_agg(g.fwd, alpha, h, None, False, mean, nh, c)
        ctx.g, ctx.slope, ctx.nh, ctx.c, ctx.mean, ctx.fill_mean = g, slope, nh, c, mean, fill_mean
        ctx.save_for_backward(h, a_src, a_dst, alpha, a_edge, loop_attr, edge_attr, m)
        return out

    @staticmethod
    def backward(ctx, gout):
        h, a_src, a_dst, alpha, a_edge, loop_attr, edge_attr, m = ctx.saved_tensors
        gm = _grad_layout(gout, 0)
        if ctx.mean:
            gm = _heads_spread(gm, ctx.nh, ctx.c)
        gh, g_a_src, g_a_dst, ge = _gat_heads_edge_backward(ctx.g, gm, h, a_src, a_dst, alpha, ctx.slope, ctx.nh, ctx.c,
                                                            a_edge)
        g_attr, g_m = _edge_term_bwd(ctx.g, ge, edge_attr, loop_attr, m, ctx.fill_mean, h.size(0), ctx.nh,
                                     ctx.needs_input_grad[7], ctx.needs_input_grad[8])
        return None, gh, g_a_src, g_a_dst, None, None, None, g_attr, g_m, None, None


class _GatHeadsEdgeConvFn(torch.autograd.Function):
    """``_GatHeadsConvFn`` with the edge-feature term in the logits (every H >= 1): the edge-term launch in front of the
    softmax, the softmax entries with the per-edge addend, and in backward one more entry for the gradients of
    ``edge_attr`` (through the loops' mean fill too) and of the folded ``M``."""

    @staticmethod
    def forward(ctx, g: GraphIndex, h, att_src, att_dst, bias, slope: float, relu: bool, nh: int, mean: bool, edge_attr,
                m, fill_mean: bool, fill: float):
        h, m = h.contiguous(), m.contiguous()
        n, f = h.shape
        c = f // nh
        a_s, a_d = att_src.reshape(-1).contiguous(), att_dst.reshape(-1).contiguous()
        a_src, a_dst = _heads_alpha_fwd(h, a_s, a_d, nh, c)
        a_edge, loop_attr = _edge_term_fwd(g, edge_attr, m, fill_mean, fill, n, nh)
        alpha = _edge_softmax_fwd(g, a_src, a_dst, a_edge, slope, n, nh)
        y = _heads_agg(g.fwd, alpha, h, bias, relu, mean, nh, c)
        ctx.g, ctx.slope, ctx.relu, ctx.nh, ctx.c, ctx.mean, ctx.fill_mean = g, slope, relu, nh, c, mean, fill_mean
        ctx.params = (att_src, att_dst, bias)
        ctx.save_for_backward(h, a_src, a_dst, alpha, a_s, a_d, y if relu else None, a_edge, loop_attr, edge_attr, m)
        return y

    @staticmethod
    def backward(ctx, gy):
        h, a_src, a_dst, alpha, a_s, a_d, y, a_edge, loop_attr, edge_attr, m = ctx.saved_tensors
        g, slope, nh, c = ctx.g, ctx.slope, ctx.nh, ctx.c
        att_src, att_dst, bias = ctx.params
        gm, gb = _heads_out_grad(ctx, gy, y, bias)
        gh, g_a_src, g_a_dst, ge = _gat_heads_edge_backward(g, gm, h, a_src, a_dst, alpha, slope, nh, c, a_edge)
        g_attr, g_m = _edge_term_bwd(g, ge, edge_attr, loop_attr, m, ctx.fill_mean, h.size(0), nh,
                                     ctx.needs_input_grad[9], ctx.needs_input_grad[10])
        pg = _ParamGrads([att_src, att_dst], ctx.needs_input_grad[2:4], h.device)
        _heads_alpha_bwd(h, g_a_src, g_a_dst, a_s, a_d, gh, nh, c, *pg.bufs, pg.direct)
        gs, gd = pg.done()
        return None, gh, gs, gd, gb, None, None, None, None, g_attr, g_m, None, None


def gat_heads_edge_conv(g: GraphIndex, h, att_src, att_dst, bias, slope: float, edge_attr, edge_m, relu: bool = False,
                        heads: int = 1, mean: bool = False, fill_value="mean") -> torch.Tensor:
    """``gat_heads_conv`` with edge features: ``edge_attr`` [E, D] in the order of the graph's ``edge_index``, ``edge_m``
    [D, H] = ``gat_edge_fold(lin_edge.weight, att_edge)``; ``fill_value``: the appended self loops' attribute."""
    h = resolve(h)
    if h.dim() != 2 or heads < 1 or h.size(1) != att_src.numel() or att_src.numel() % heads:
        raise ValueError("gat_heads_edge_conv: h must be [N, H*C] and att_src / att_dst [1, H, C]")
    edge_attr, fill_mean, fill = _edge_operands(g, edge_attr, edge_m, int(heads), fill_value)
    return _GatHeadsEdgeConvFn.apply(g, h, att_src, att_dst, bias, float(slope), bool(relu), int(heads), bool(mean),
                                     edge_attr, edge_m, fill_mean, fill)


# --------------------------------------------------------------------------- #
# the two training losses in one pass (train.py:51-53, models/losses.py:7-19)
# --------------------------------------------------------------------------- #
class _ContactLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g: GraphIndex, pred: torch.Tensor, target: torch.Tensor):
        L = _lib.lib()
        n = pred.size(0)
        dev = pred.device
        pred_c = pred if pred.stride(1) == 1 else pred.contiguous()
        tgt_c = target if target.stride(1) == 1 else target.contiguous()
        g1 = torch.empty((n, 3), dtype=torch.float32, device=dev)
        g2 = torch.empty((n, 3), dtype=torch.float32, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        nb = L.dc_contact_loss_workspace_bytes(n)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        rc = L.dc_contact_loss(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), g.bwd.ptr.data_ptr(),
                               g.bwd.other.data_ptr(), pred_c.data_ptr(), pred_c.stride(0),
                               tgt_c.data_ptr(), tgt_c.stride(0), n, g.num_input_edges, g1.data_ptr(),
                               g2.data_ptr(), out.data_ptr(), ws.data_ptr(), nb, current_stream_ptr(dev))
        _lib.check(rc, "dc_contact_loss")
        ctx.save_for_backward(g1, g2)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_l1, g_gcl):
        g1, g2 = ctx.saved_tensors
        return None, g1 * g_l1 + g2 * g_gcl, None


def contact_losses(g: GraphIndex, pred_pos: torch.Tensor, target_pos: torch.Tensor):
    """``(L1Loss(pred, target), GradientConsistencyLoss(pred, target))`` over the edge set of ``g``
    (``train.py:51-53``) in one node pass, differentiable w.r.t. ``pred_pos`` (the target is data)."""
    pred_pos, target_pos = resolve(pred_pos), resolve(target_pos)
    _require_cuda(pred_pos, "pred_pos")
    for name, t in (("pred_pos", pred_pos), ("target_pos", target_pos)):
        if t.dim() != 2 or t.size(1) != 3 or t.dtype != torch.float32:
            raise ValueError(f"contact_losses: {name} must be float32 [N, 3]")
    if pred_pos.shape != target_pos.shape or pred_pos.size(0) != g.num_nodes:
        raise ValueError("contact_losses: pred / target / graph sizes differ")
    if g.self_loops:
        raise ValueError("contact_losses: needs the adjacency of the raw edge set (no self-loop rewriting)")
    if pred_pos.size(0) == 0:
        raise ValueError("contact_losses: empty graph")
    return _ContactLossFn.apply(g, pred_pos, target_pos)


# --------------------------------------------------------------------------- #
# TransformerConv (dc_transformer.hip): q = lin_query(x), k = lin_key(x), v = lin_value(x) [N, H*C]; the logit is the
# scaled dot product <q_i, k_j> / sqrt(C) per edge and head.  Score + edge softmax and both sides of the backward are
# gather kernels of their own; aggregation, SDDMM, spread and the mask / bias gradient pass are the multi-head
# launchers above.  One launcher per C entry.
# --------------------------------------------------------------------------- #
def _tconv_scale(c: int) -> float:
    """``float32(1 / sqrt(C))`` (the C entries take a float: ctypes rounds the double to nearest)"""
    return 1.0 / float(c) ** 0.5


def _tconv_softmax_fwd(g: GraphIndex, q, k, nh: int, c: int) -> torch.Tensor:
    """alpha [capacity, H]: the edge softmax of ``e[p, h] = <q[i, h, :], k[j, h, :]> / sqrt(C)``."""
    alpha = _heads_edge_vector(g, nh, q.device)
    _lib.check(_lib.lib().dc_tconv_softmax_fwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), q.data_ptr(),
                                               _rowmajor(q, "q"), k.data_ptr(), _rowmajor(k, "k"), _tconv_scale(c),
                                               alpha.data_ptr(), q.size(0), nh, c, current_stream_ptr(q.device)),
               "dc_tconv_softmax_fwd")
    return alpha


def _tconv_softmax_bwd(g: GraphIndex, alpha, galpha, k, nh: int, c: int):
    """-> (gl [capacity, H], the gradient of the dot products; g_q [N, H*C])"""
    n, dev = k.size(0), k.device
    gl = _heads_edge_vector(g, nh, dev)
    g_q = torch.empty((n, nh * c), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dc_tconv_softmax_bwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), alpha.data_ptr(),
                                               galpha.data_ptr(), k.data_ptr(), _rowmajor(k, "k"), _tconv_scale(c),
                                               gl.data_ptr(), g_q.data_ptr(), nh * c, n, nh, c,
                                               current_stream_ptr(dev)), "dc_tconv_softmax_bwd")
    return gl, g_q


def _tconv_source_bwd(g: GraphIndex, alpha, gl, q, gm, nh: int, c: int):
    """-> (g_k, g_v) [N, H*C] over the transposed set: the score's key term and the transposed aggregation in one walk."""
    n, dev = q.size(0), q.device
    g_k = torch.empty((n, nh * c), dtype=torch.float32, device=dev)
    g_v = torch.empty((n, nh * c), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().dc_tconv_source_bwd(g.bwd.ptr.data_ptr(), g.bwd.other.data_ptr(), g.bwd_to_fwd().data_ptr(),
                                              alpha.data_ptr(), gl.data_ptr(), q.data_ptr(), _rowmajor(q, "q"),
                                              gm.data_ptr(), _rowmajor(gm, "gm"), g_k.data_ptr(), nh * c, g_v.data_ptr(),
                                              nh * c, n, nh, c, current_stream_ptr(dev)), "dc_tconv_source_bwd")
    return g_k, g_v


class _TransformerAggFn(torch.autograd.Function):
    """The attention of a TransformerConv layer behind its three linears: score + edge softmax in one launch, then
    ``act(aggregation of v + bias)`` (concatenated, or the mean over the heads) as for ``_Gatv2ConvFn``; backward: mask
    + bias gradient in one pass (only with ``relu`` / ``bias``), (mean: the gradient spread to the heads,) SDDMM, then
    the destination side (gl, g_q) and the source side (g_k, g_v in one walk).  The node ends at the aggregation: the
    skip connection and the gate are the layer's."""

    @staticmethod
    def forward(ctx, g: GraphIndex, q, k, v, bias, relu: bool, nh: int, mean: bool):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        n, c = q.size(0), q.size(1) // nh
        ctx.g, ctx.relu, ctx.nh, ctx.c, ctx.mean, ctx.bias = g, relu, nh, c, mean, bias
        ctx.empty = n == 0
        if ctx.empty:                        # no rows: nothing to launch (an empty tensor has no address)
            return q.new_empty((0, c if mean else nh * c))
        alpha = _tconv_softmax_fwd(g, q, k, nh, c)
        y = _heads_agg(g.fwd, alpha, v, bias, relu, mean, nh, c)
        ctx.save_for_backward(q, k, v, alpha, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        g, nh, c, bias = ctx.g, ctx.nh, ctx.c, ctx.bias
        need_b = bias is not None and ctx.needs_input_grad[4]
        if ctx.empty:                        # sums over no rows
            z = gy.new_zeros((0, nh * c))
            return None, z, z, z, (gy.new_zeros(gy.size(1)) if need_b else None), None, None, None
        q, k, v, alpha, y = ctx.saved_tensors
        gm, gb = _heads_out_grad(ctx, gy, y, bias)
        galpha = _heads_sddmm(g, gm, v, nh, c)
        gl, g_q = _tconv_softmax_bwd(g, alpha, galpha, k, nh, c)
        g_k, g_v = _tconv_source_bwd(g, alpha, gl, q, gm, nh, c)
        return None, g_q, g_k, g_v, gb, None, None, None


def transformer_conv(g: GraphIndex, q, k, v, bias=None, relu: bool = False, heads: int = 1,
                     mean: bool = False) -> torch.Tensor:
    """The attention of a TransformerConv layer behind ``lin_query`` / ``lin_key`` / ``lin_value`` (``q`` / ``k`` / ``v``
    [N, H*C]) on the edge set of ``g`` as it is: [N, H*C], or [N, C] with ``mean``; a row without edges is 0 (+ bias).
    With ``bias`` or ``relu`` the widths must pass ``gat_heads_fused_ok`` (the mask / bias-gradient pass); the bare
    aggregation runs at every width."""
    q, k, v = resolve(q), resolve(k), resolve(v)
    if q.dim() != 2 or heads < 1 or q.size(1) % heads or q.size(1) == 0 or k.shape != q.shape or v.shape != q.shape:
        raise ValueError("transformer_conv: q / k / v must be [N, H*C]")
    if (bias is not None or relu) and not gat_heads_fused_ok(v, heads, mean):
        raise ValueError(f"transformer_conv: bias / relu need widths the fused row passes take (gat_heads_fused_ok), got "
                         f"H*C = {q.size(1)}, H = {heads}; call it without them and apply them outside")
    return _TransformerAggFn.apply(g, q, k, v, bias, bool(relu), int(heads), bool(mean))


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
    g = _grad_layout(g, 1)
    return g if g.size(0) <= 1 or g.stride(0) >= g.size(1) else g.contiguous()


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
    if g.self_loops or g.normalize or g.edge_index is None or g.fwd.row_offset or g.bwd.row_offset:
        raise ValueError("gine_aggregate: the graph must be built from one edge_index with self_loops=False, "
                         "normalize=False (not a merged adjacency or a row window of one)")
    if g.device != x.device:
        raise RuntimeError(f"gine_aggregate: x is on {x.device} but the graph is on {g.device}")
    if g.num_nodes != x.size(0):
        raise ValueError(f"gine_aggregate: x has {x.size(0)} rows but the graph has {g.num_nodes} nodes")
    if g.num_input_edges != e.size(0):
        raise ValueError(f"gine_aggregate: e has {e.size(0)} rows but the graph has {g.num_input_edges} edges")
    # unit inner stride and rows that do not overlap (an expanded operand is copied); a column slice passes as it is
    if (x.size(1) > 1 and x.stride(1) != 1) or (x.size(0) > 1 and x.stride(0) < x.size(1)):
        x = x.contiguous()
    if (e.size(1) > 1 and e.stride(1) != 1) or (e.size(0) > 1 and e.stride(0) < e.size(1)):
        e = e.contiguous()
    return _GineAggFn.apply(g, x, e, eps)


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


def _edge_graph_check(who: str, g: GraphIndex, t: torch.Tensor, what: str) -> None:
    if g.self_loops or g.normalize or g.edge_index is None or g.fwd.row_offset or g.bwd.row_offset:
        raise ValueError(f"{who}: the graph must be built from one edge_index with self_loops=False, "
                         "normalize=False (not a merged adjacency or a row window of one)")
    if g.device != t.device:
        raise RuntimeError(f"{who}: {what} is on {t.device} but the graph is on {g.device}")


def _edge_rows(t: torch.Tensor) -> torch.Tensor:
    """unit inner stride and rows that do not overlap (an expanded operand is copied); a column slice passes as it is"""
    if (t.size(1) > 1 and t.stride(1) != 1) or (t.size(0) > 1 and t.stride(0) < t.size(1)):
        return t.contiguous()
    return t


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
    _edge_graph_check("edge_pairs", g, x, "x")
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
    _edge_graph_check("edge_aggregate", g, m, "m")
    if g.num_input_edges != m.size(0):
        raise ValueError(f"edge_aggregate: m has {m.size(0)} rows but the graph has {g.num_input_edges} edges")
    return _EdgeReduceFn.apply(g, _edge_rows(m), mode)


# --------------------------------------------------------------------------- #
# PointNetConv (dc_pointnet.hip): the per-edge primitives on a BIPARTITE edge set - sources ``x_src`` / ``pos_src`` with
# ``Ns`` rows, destinations ``pos_dst`` with ``Nd`` rows - what PointNet++'s set-abstraction layer puts around the
# user's modules.  The adjacency is ONE ``GraphIndex`` over ``max(Ns, Nd)`` rows (``pointnet_graph``): rows beyond
# ``Nd`` (by destination) or ``Ns`` (by source) are empty, and the kernels are told the two counts.  With ``loops`` (one
# node set, an adjacency built with ``self_loops=True``) the edge rows are ``E' = E + N``: input edges in input order,
# then node ``i``'s loop at row ``E + i``; an input edge with ``src == dst`` keeps its row and takes no part.  The
# forward reduction is ``dc_edge_reduce_fwd`` as it stands.  One launcher per C entry.
# --------------------------------------------------------------------------- #
#: ``pointnet_pairs`` lays ``z`` out with its row stride rounded up to 4 floats where that gives the pair kernel 16-byte
#: stores (F % 4 == 0, F > 0: one padding column, written as zeros; ``z`` is then a NON-CONTIGUOUS ``[E', F + 3]`` view of
#: ``[E', F + 4]`` rows - a user's module that calls ``.view()`` on it must call ``.contiguous()`` first); contiguous
#: ``[E', F + 3]`` rows otherwise, and everywhere when cleared.  Measured by tools/pointnet_bench.py:
#: at F = 64 the pair forward takes 0.128 ms padded against 0.203 ms contiguous and a Linear behind it loses nothing to
#: the strided operand; at F = 3 (6 columns, 8 padded) the two layouts tie, so nothing is padded there
POINTNET_PAD_Z = True


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
    from .neighbors import _ld
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


def _pointnet_graph_check(who: str, g: GraphIndex, loops: bool, t: torch.Tensor, what: str) -> None:
    if g.self_loops != bool(loops) or g.normalize or g.edge_index is None or g.fwd.row_offset or g.bwd.row_offset:
        raise ValueError(f"{who}: the graph must be built from one edge_index with self_loops={bool(loops)}, "
                         "normalize=False (not a merged adjacency or a row window of one)")
    if g.device != t.device:
        raise RuntimeError(f"{who}: {what} is on {t.device} but the graph is on {g.device}")


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
    from .neighbors import _check_points
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
    pad = (POINTNET_PAD_Z and f > 0 and f % 4 == 0) if pad is None else bool(pad)
    if g is None:
        if max(ns, nd) != 0:
            raise ValueError("pointnet_pairs: g may be None only without any node")
        return _PointnetPairFn.apply(None, x_src, pos_src, pos_dst, loops, pad)
    _pointnet_graph_check("pointnet_pairs", g, loops, pos_src, "pos_src")
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
    _pointnet_graph_check("pointnet_aggregate", g, loops, m, "m")
    nd = g.num_nodes if num_dst is None else int(num_dst)
    if not 0 <= nd <= g.num_nodes or (loops and nd != g.num_nodes):
        raise ValueError(f"pointnet_aggregate: num_dst = {nd} does not fit the graph's {g.num_nodes} rows"
                         f"{' (loops need all of them)' if loops else ''}")
    rows = _pointnet_edge_rows(g, loops)
    if rows != m.size(0):
        raise ValueError(f"pointnet_aggregate: m has {m.size(0)} rows but the graph has {rows} edge rows")
    return _PointnetReduceFn.apply(g, _edge_rows(m), mode, nd, loops)


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


# --------------------------------------------------------------------------- #
# GMMConv (dc_gmm.hip): per in-edge a mixture of K Gaussians over the edge's D pseudo-coordinates weights the K column
# blocks of the source row of h = x @ g.  The weights w [E, K] are formed once, in the order of the input edges (read
# through the adjacency's ``perm``), and saved for the backward.  One launcher per C entry.
# --------------------------------------------------------------------------- #
GMM_MAX_K = 64        # DC_GMM_MAX_K in include/deformcontact.h
GMM_MAX_D = 16        # DC_GMM_MAX_D
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
    if g.self_loops or g.normalize or g.edge_index is None or g.fwd.row_offset or g.bwd.row_offset:
        raise ValueError("gmm_aggregate: the graph must be built from one edge_index with self_loops=False, "
                         "normalize=False (not a merged adjacency or a row window of one)")
    if g.device != h.device:
        raise RuntimeError(f"gmm_aggregate: h is on {h.device} but the graph is on {g.device}")
    if g.num_nodes != h.size(0):
        raise ValueError(f"gmm_aggregate: h has {h.size(0)} rows but the graph has {g.num_nodes} nodes")
    if g.num_input_edges != edge_attr.size(0):
        raise ValueError(f"gmm_aggregate: edge_attr has {edge_attr.size(0)} rows but the graph has "
                         f"{g.num_input_edges} edges")

    def rows(t):
        # unit inner stride and rows that do not overlap (an expanded operand is copied); a column slice passes as it is
        return t.contiguous() if (t.size(1) > 1 and t.stride(1) != 1) or (t.size(0) > 1 and t.stride(0) < t.size(1)) else t
    return _GmmAggFn.apply(g, rows(h), rows(edge_attr), mu, sigma, rows(base) if base is not None else None, m, mean,
                           bool(relu))


# --------------------------------------------------------------------------- #
# SplineConv (dc_spline.hip): per in-edge a B-spline of degree 1..3 over the edge's D pseudo-coordinates names S =
# (degree+1)^D of the K column blocks of the source row of h = x @ weight[k] and weights them.  The basis values
# b [E, S] and the block indices wi [E, S] are formed once, in the order of the input edges (read through the
# adjacency's ``perm``), and saved for the backward.  ``kernel_size``, ``is_open_spline`` and ``degree`` are host values
# copied into the kernel arguments.  One launcher per C entry.
# --------------------------------------------------------------------------- #
SPLINE_MAX_D = 4       # DC_SPLINE_MAX_D in include/deformcontact.h
SPLINE_MAX_S = 64      # DC_SPLINE_MAX_S
SPLINE_MAX_K = 1024    # DC_SPLINE_MAX_K
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
    if g.self_loops or g.normalize or g.edge_index is None or g.fwd.row_offset or g.bwd.row_offset:
        raise ValueError("spline_aggregate: the graph must be built from one edge_index with self_loops=False, "
                         "normalize=False (not a merged adjacency or a row window of one)")
    if g.device != h.device:
        raise RuntimeError(f"spline_aggregate: h is on {h.device} but the graph is on {g.device}")
    if g.num_nodes != h.size(0):
        raise ValueError(f"spline_aggregate: h has {h.size(0)} rows but the graph has {g.num_nodes} nodes")
    if g.num_input_edges != edge_attr.size(0):
        raise ValueError(f"spline_aggregate: edge_attr has {edge_attr.size(0)} rows but the graph has "
                         f"{g.num_input_edges} edges")

    def rows(t):
        # unit inner stride and rows that do not overlap (an expanded operand is copied); a column slice passes as it is
        return t.contiguous() if (t.size(1) > 1 and t.stride(1) != 1) or (t.size(0) > 1 and t.stride(0) < t.size(1)) else t
    return _SplineAggFn.apply(g, rows(h), rows(edge_attr), rows(base) if base is not None else None, geom, m, mean,
                              bool(relu))
