"""Host helpers every operator module shares: pointers and leading dimensions for the C ABI, the layouts the kernels
take, and the graph check of the per-edge operators.  No run-time switch lives here (they are all in ``ops.py``)."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch


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


def _grad_layout(g: torch.Tensor, row_align: int) -> torch.Tensor:
    """The incoming gradient ``g`` in a layout the backward kernels of the calling site take, copied only if it is not
    in one already.  ``row_align`` = 0: dense rows (plain contiguous); 1: unit inner stride, any row stride (column
    slices pass as they are); 4: unit inner stride, and row stride and base address multiples of 4 floats (16 bytes)."""
    ok = row_align == 1 or (row_align == 4 and g.stride(0) % 4 == 0 and g.data_ptr() % 16 == 0)
    return g if (ok and g.stride(1) == 1) else g.contiguous()


def _rows(t: torch.Tensor) -> torch.Tensor:
    """unit inner stride and rows that do not overlap (an expanded operand is copied); a column slice passes as it is"""
    if (t.size(1) > 1 and t.stride(1) != 1) or (t.size(0) > 1 and t.stride(0) < t.size(1)):
        return t.contiguous()
    return t


def _graph_check(who: str, g, loops: bool, t: torch.Tensor, what: str) -> None:
    """The graph of a per-edge operator: the sorted sets of ONE edge list (the kernels read ``g.edge_index`` and the
    sets' ``perm`` side by side), with loops exactly where the caller's edge rows have them, on ``t``'s device."""
    if g.self_loops != bool(loops) or g.normalize or g.edge_index is None or g.fwd.row_offset or g.bwd.row_offset:
        raise ValueError(f"{who}: the graph must be built from one edge_index with self_loops={bool(loops)}, "
                         "normalize=False (not a merged adjacency or a row window of one)")
    if g.device != t.device:
        raise RuntimeError(f"{who}: {what} is on {t.device} but the graph is on {g.device}")
