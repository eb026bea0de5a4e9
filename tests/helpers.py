"""Shared test helpers (tests may import oracle/; the product may not)."""
import contextlib
import os
import sys

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


def rel_err(a, b):
    """max |a-b| / max |b|  -- the tolerance north_star states is 1e-5 on this."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def row_rel_err(a, b):
    """max over rows i of  max_j |a_ij - b_ij| / max_j |b_ij|  (rows of b that are all zero are
    compared absolutely against the global scale): stricter than ``rel_err`` for rows whose
    magnitude is far below the tensor's maximum."""
    a = np.asarray(a, dtype=np.float64).reshape(len(a), -1)
    b = np.asarray(b, dtype=np.float64).reshape(len(b), -1)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    scale = np.abs(b).max(axis=1)
    scale = np.where(scale > 0, scale, max(np.abs(b).max(), 1e-30))
    return float((np.abs(a - b).max(axis=1) / scale).max())


def col_rel_err(a, b):
    """``row_rel_err`` over the columns: each column of a 2-D result on its own scale."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.ndim == 2 and a.shape == b.shape, (a.shape, b.shape)
    return row_rel_err(a.T, b.T)


def cw_err(got, exact, S):
    """Component-wise distance max |got - exact| / S, where ``S`` is the sum of the absolute values of the terms
    ``exact`` sums (tests/h2_model.py).  A component with S = 0 sums only zeros: it must be exactly 0 in ``got``."""
    got, exact, S = (np.asarray(v, dtype=np.float64) for v in (got, exact, S))
    assert got.shape == exact.shape == S.shape, (got.shape, exact.shape, S.shape)
    zero = S == 0
    assert not got[zero].any(), "a component whose terms are all zero is not exactly 0"
    if zero.all():
        return 0.0
    return float((np.abs(got - exact)[~zero] / S[~zero]).max())


def h2_parity_operands(n, fi, fo, nseg, regime):
    """(slab [N, nseg * Fi], g [N, Fo], [W_s [Fo, Fi]], bias [Fo]) in fp32: the operands of
    tests/test_gpu_parity.py::test_dense_block_fp16x2_vs_float64 - one generator for that test and for the CPU test that
    proves which of its metrics the arithmetic's model supports (tests/test_h2_model.py)."""
    from oracle.weights import hashed_uniform
    slab, g = hashed_uniform((n, nseg * fi), 5, 2.0), hashed_uniform((n, fo), 91, 2.0)
    wscale = 2.0 / np.sqrt(fi)
    if regime == "wide_rows":                                    # node rows over 1e6, g against x
        rs = np.logspace(-6, 0, n, dtype=np.float32)[:, None]
        slab, g = slab * rs, g * rs[::-1]
    elif regime == "tiny":
        slab, g, wscale = slab * np.float32(1e-12), g * np.float32(1e-12), wscale * 1e-6
    elif regime == "huge":
        slab, g, wscale = slab * np.float32(1e12), g * np.float32(1e10), wscale * 1e3
    else:
        assert regime == "unit", regime
    slab, g = np.ascontiguousarray(slab, np.float32), np.ascontiguousarray(g, np.float32)
    ws = [hashed_uniform((fo, fi), 40 + s, wscale) for s in range(nseg)]
    bias = (hashed_uniform((fo,), 77, 0.5) * np.float32(np.abs(slab).max()) * np.float32(wscale)).astype(np.float32)
    return slab, g, ws, bias


#: every parity comparison of a test run: (test id, tensor, HIP-vs-fp32-oracle distance, did the float64 widening fire,
#: HIP-vs-float64, oracle-vs-float64) - tests/conftest.py writes it to gpurun_out/parity_distances.json at session end
#: ("nothing records how often the widening fires or the worst HIP-vs-fp32-oracle distance")
PARITY_LOG = []


def record_parity(name, d, widened=False, e_h=None, e_o=None, tol=1e-5, metric="rel_err", special=None):
    """``special``: why this comparison is not on north_star's 1e-5 scale (e.g. a gradient that is mathematically zero,
    parameters after several Adam steps) - listed apart and kept out of the summary's worst-case figures."""
    test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
    PARITY_LOG.append({"test": test, "tensor": name, "special": special,
                       "hip_vs_fp32_oracle": None if d is None else float(d),
                       "tol": tol, "metric": metric, "float64_widening_fired": bool(widened),
                       "hip_vs_float64": None if e_h is None else float(e_h),
                       "fp32_oracle_vs_float64": None if e_o is None else float(e_o)})


def three_way(d, e_h_fn, e_o_fn, tol=1e-5, name="", metric="rel_err", special=None, special_bound=None):
    """The parity rule on already computed distances: ``d`` (HIP vs fp32 oracle) < tol, or - evaluated lazily - HIP
    within ``tol`` of the float64 truth (round 5: the ``2 x the oracle's own distance`` allowance is gone; every
    widened comparison of round 4 was within 4.4e-6 of float64).  Only a comparison registered ``special`` (a stated
    reason why it is not on north_star's scale) may pass a wider ``special_bound(e_o)``.  Records the outcome."""
    if d < tol:
        record_parity(name, d, tol=tol, metric=metric, special=special)
        return d
    e_h, e_o = e_h_fn(), e_o_fn()
    record_parity(name, d, True, e_h, e_o, tol=tol, metric=metric, special=special)
    bound = tol if special is None else max(tol, special_bound(e_o))
    assert e_h <= bound, (
        f"{name}: HIP vs fp32 oracle {d:.2e} >= {tol:g}, and vs the float64 truth the HIP path is off by "
        f"{e_h:.2e} > {bound:.2e} (the fp32 oracle is off by {e_o:.2e})")
    return d


def assert_parity(got, ref32, truth64=None, tol=1e-5, name="", metric=None, special=None, special_bound=None):
    """north_star's bar: ``metric(got, fp32 oracle) < tol`` (1e-5).  Where two correct fp32 evaluations legitimately
    differ by more (gradients through several layers: different but equally valid summation orders), the HIP result has
    to be within ``tol`` of a float64 evaluation of the same maths - nothing wider, unless the comparison is registered
    ``special`` with its own stated bound (``three_way``).  Returns the HIP-vs-oracle distance."""
    metric = metric or rel_err
    d = metric(got, ref32)
    if d >= tol:
        assert truth64 is not None, f"{name}: {d:.2e} >= {tol:g} vs the fp32 oracle and no float64 truth given"
    return three_way(d, lambda: metric(got, truth64), lambda: metric(ref32, truth64), tol=tol, name=name,
                     metric=metric.__name__, special=special, special_bound=special_bound)


class G:
    """duck-typed graph batch"""

    def __init__(self, x, edge_index, pos=None):
        self.x, self.edge_index, self.pos = x, edge_index, pos

    def clone(self):
        return G(self.x.clone(), self.edge_index.clone(),
                 None if self.pos is None else self.pos.clone())


def golden_graphs(z, device="cpu"):
    t = lambda k, dt=None: torch.from_numpy(z[k]).to(device)
    rest = G(t("rest_x"), t("rest_edge_index"), t("rest_pos"))
    rig = G(t("rig_x"), t("rig_edge_index"), t("rig_pos"))
    return rest, rig


def random_multigraph(n, e, seed, self_loops=True, isolated=True):
    """edge_index with duplicate edges, self loops and zero-in-degree nodes."""
    rng = np.random.default_rng(seed)
    hi = n - (max(1, n // 10) if isolated else 0)      # last nodes never a target
    src = rng.integers(0, n, e)
    dst = rng.integers(0, max(hi, 1), e)
    if e >= 8:
        src[:4] = src[4:8]                              # duplicates
        dst[:4] = dst[4:8]
        if self_loops:
            src[8:12] = dst[8:12]
    return np.stack([src, dst]).astype(np.int64)


# --------------------------------------------------------------------------- #
# non-finite values (tests/test_nonfinite.py): ONE poison in clean finite inputs.  No tolerance:
# every assertion is isfinite, a float64 equality or torch.equal on bits.
# --------------------------------------------------------------------------- #
#: the three poisons, NaN first (its float64 restatement defines the reach set)
POISONS = (("nan", float("nan")), ("+inf", float("inf")), ("-inf", float("-inf")))


def poisoned(inputs, name, index, value):
    """A copy of the dict of tensors ``inputs`` with ``inputs[name][index] = value`` (``index``: a tuple; a whole row is
    ``(r,)`` or ``(r, slice(None))``); the other tensors are shared, none is modified."""
    out = dict(inputs)
    t = inputs[name].clone()
    t[index] = value
    out[name] = t
    return out


def reach_sets(ref, inputs64, name, index, value=float("nan")):
    """-> list of bool tensors, one per output of ``ref`` (a float64 restatement: dict of float64 CPU tensors -> list
    of float64 tensors): where the restatement is NON-FINITE with ``value`` placed at ``inputs64[name][index]``.  With
    the NaN poison this is the reach set R."""
    outs = ref(poisoned(inputs64, name, index, value))
    return [~torch.isfinite(o) for o in outs]


def assert_not_swallowed(out, must, what=""):
    """Rule 1: ``out`` (any device / float dtype) is non-finite at every position of the bool mask ``must``."""
    bad = torch.isfinite(out.detach().cpu().float()) & must
    assert not bool(bad.any()), (f"{what}: a non-finite value was swallowed at {int(bad.sum())} of {int(must.sum())} "
                                 f"positions, first {tuple(int(v) for v in bad.nonzero()[0])}")


def assert_contained(out, clean, reach, what=""):
    """Rule 2: outside the reach set ``reach`` the output has the bits of the same kernel's output on the clean inputs."""
    keep = ~reach
    a, b = out.detach().cpu(), clean.detach().cpu()
    assert a.shape == b.shape == keep.shape, (what, a.shape, b.shape, keep.shape)
    a, b = a[keep], b[keep]
    same = torch.equal(a, b) if a.dtype != torch.float32 else torch.equal(a.view(torch.int32), b.view(torch.int32))
    if not same:
        diff = (out.detach().cpu() != clean.detach().cpu()) & keep     # (a clean output is finite: != is a bit difference
        raise AssertionError(f"{what}: {int(diff.sum())} positions outside the reach set changed, first "   # up to +-0)
                             f"{tuple(int(v) for v in diff.nonzero()[0]) if diff.any() else 'a sign of zero'}")


def assert_selection(out, ref64, what=""):
    """Rule 3: the output equals the float64 restatement exactly, everywhere (+-Inf compare equal to themselves)."""
    a = out.detach().cpu().double()
    assert a.shape == ref64.shape, (what, a.shape, ref64.shape)
    bad = ~((a == ref64) | (torch.isnan(a) & torch.isnan(ref64)))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} positions differ from the float64 restatement"


def graph_rows(edge_index, n):
    """Rows the poison placements use: a MID row with in-edges and out-edges that is neither row 0 nor the last, and
    the last row.  ``edge_index``: int array [2, E]."""
    src, dst = np.asarray(edge_index[0]), np.asarray(edge_index[1])
    both = sorted(set(src.tolist()) & set(dst.tolist()) - {0, n - 1})
    mid = both[len(both) // 2] if both else 0
    return mid, n - 1


def element_placements(edge_index, n, f):
    """The placements of a poison in a node-valued [n, f] input: element [0, 0] (padded lanes and tail iterations
    conventionally read element 0: the containment probe), an element of a mid row with in- and out-edges, an
    element of the last row, an element in the last column."""
    mid, last = graph_rows(edge_index, n)
    out = {"first": (0, 0), "mid": (mid, f // 2), "lastrow": (last, min(1, f - 1)), "lastcol": (mid // 2, f - 1)}
    return {k: v for k, v in out.items() if k == "first" or n > 1}


def edge_placements(edge_index, c, unroll=8):
    """The placements of a poison in an edge-valued [E, c] input: edge 0, and the last input edge of a destination
    whose in-degree is not a multiple of the kernels' unroll (its tail iteration is partly predicated off)."""
    dst = np.asarray(edge_index[1])
    out = {"edge0": (0, 0)}
    deg = np.bincount(dst)
    odd = [d for d in np.nonzero(deg % unroll)[0] if deg[d] >= 2]
    if odd:
        d = odd[len(odd) // 2]
        out["segtail"] = (int(np.nonzero(dst == d)[0][-1]), c - 1)
    return out


def linear_spline_basis(a, kernel_size, is_open):
    """The degree-1 B-spline basis of SplineConv in float32, as the kernel forms it: for
    pseudo-coordinates ``a`` [E, D] in [0, 1] -> (b float32 [E, 2^D], wi int64 [E, 2^D]).  Per dimension ``v = a_d *
    (kernel_size_d - open_d)``, ``f = v - floor(v)``; slot ``s`` takes digit ``k_d = (s >> d) & 1`` (dimension 0 runs
    fastest), the factor ``1 - f - k_d + 2 f k_d`` and the index digit ``(floor(v) + k_d) mod kernel_size_d``."""
    a = np.asarray(a, np.float32).reshape(len(a), -1)
    dim = a.shape[1]
    slots = np.arange(2 ** dim)
    b = np.ones((a.shape[0], len(slots)), np.float32)
    wi = np.zeros(b.shape, np.int64)
    off = 1
    for d in range(dim):
        v = a[:, d] * np.float32(kernel_size[d] - int(bool(is_open[d])))
        fl = np.floor(v)
        f = (v - fl).astype(np.float32)[:, None]
        k = ((slots >> d) & 1)[None]
        wi += ((fl.astype(np.int64)[:, None] + k) % kernel_size[d]) * off
        off *= kernel_size[d]
        kf = k.astype(np.float32)
        b = (b * (1 - f - kf + 2 * f * kf)).astype(np.float32)
    return b, wi


# --------------------------------------------------------------------------- #
# guard bands ("Memory contract"; tests/test_guard_bands.py): what a kernel does AROUND its tensors.
# No tolerance: every comparison is on bits.
# --------------------------------------------------------------------------- #
#: rows of the largest row tile of the kernels (dc_dense.hip: 64 * MB rows; the attention 128-query tile)
GUARD_TILE_ROWS = 128
GUARD_MIN_BAND = 4096
GUARD_ALIGN = 512

_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_EMPTY, _ZEROS, _ONES, _FULL = "empty", "zeros", "ones", "full"


def bits(t):
    """``t`` as a contiguous integer tensor of the same element size: equality on it is equality of bits (NaN payloads
    and the sign of zero included)."""
    t = t.detach().contiguous()
    return t if not (t.is_floating_point() or t.dtype == torch.bool) else t.view(_INT_OF_SIZE[t.element_size()])


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def guard_band_bytes(shape, itemsize):
    """One full tile of the largest row tile at this tensor's row pitch, at least 4 KiB, rounded up to 512 bytes: the
    interior keeps the alignment class of a fresh allocation, so the same kernels are dispatched as in a plain run."""
    pitch = (int(shape[-1]) if len(shape) >= 2 else 1) * itemsize
    band = max(GUARD_MIN_BAND, GUARD_TILE_ROWS * pitch)
    return -(-band // GUARD_ALIGN) * GUARD_ALIGN


def _sentinel(dtype, value=None):
    """The bytes of one fill element: NaN for float types, 1 for integer types, the float32 NaN pattern per 4 bytes for
    byte buffers (workspaces); ``value``: an explicit element (the valid index in the slack of an index input)."""
    if value is not None:
        return torch.tensor([value], dtype=dtype).view(torch.uint8).clone()
    if dtype == torch.uint8:
        return torch.tensor([float("nan")], dtype=torch.float32).view(torch.uint8).clone()
    if dtype.is_floating_point:
        return torch.tensor([float("nan")], dtype=dtype).view(torch.uint8).clone()
    return torch.ones(1, dtype=dtype).view(torch.uint8).clone()


class _Buffer:
    """front band | interior | back band of one flat byte allocation, plus the gap columns of a strided interior"""

    def __init__(self, name, flat, front, nbytes, pattern, view, kind):
        self.name, self.flat, self.front, self.nbytes, self.view, self.kind = name, flat, front, nbytes, view, kind
        self.pattern = pattern.to(flat.device)             # uint8 [k]
        self.gap, self.gap_fill = None, None               # a strided view of the gap columns and their fill, or None
        self.source_guarded = False                        # a clone: did its source lie inside a guarded allocation?
        self.snapshot = None                               # hosted inputs: the bits the interior must keep (rule 2)
        self.in_place = None                               # ... or the reason it may change

    def region(self, side):
        lo, hi = (0, self.front) if side == "front" else (self.front + self.nbytes, self.flat.numel())
        return self.flat[lo:hi]

    def _as_words(self, region):
        k = self.pattern.numel()
        n = region.numel() // k * k
        if region.storage_offset() % k:                    # behind a byte workspace of a ragged size: byte by byte
            return region[:n].view(-1, k), self.pattern.view(1, k)
        return region[:n].view(_INT_OF_SIZE[k]), self.pattern.view(_INT_OF_SIZE[k])

    def fill(self, region):
        words, p = self._as_words(region)
        words.copy_(p.expand_as(words))
        rest = region.numel() % self.pattern.numel()
        if rest:
            region[region.numel() - rest:].copy_(self.pattern[:rest])

    def differs(self, region):
        """-> bool tensor over the whole words of ``region`` (a byte buffer's ragged end is compared as bytes)"""
        words, p = self._as_words(region)
        return words != p

    def contains(self, t):
        """``t`` lies inside the interior.  The copy ``clone`` makes counts only where its SOURCE lay inside a guarded
        allocation: it is an ATen result, and what a kernel wrote is the source."""
        if self.kind == "clone" and not self.source_guarded:
            return False
        if t.numel() == 0:
            return True
        lo = self.flat.data_ptr() + self.front
        a = t.data_ptr()
        b = a + (1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride()))) * t.element_size()
        return t.device == self.flat.device and lo <= a and b <= lo + self.nbytes


class Guard:
    """While active, the Python-level factories (``torch.empty / zeros / ones / full``, their ``*_like`` forms,
    ``Tensor.new_empty / new_zeros / new_ones / new_full``) return, for tensors on ``device_type``, the interior of a
    flat buffer ``front band | interior | back band`` as a contiguous view of the requested shape and dtype; every other
    call passes through.  Bands hold NaN (float, bf16), 1 (integer types) or the float32 NaN pattern (bytes).  ``zeros``
    / ``ones`` / ``full`` keep their meaning in the interior; an ``empty`` interior holds zeros (a young process: fresh
    pages) or, with ``dirty``, the band's own fill.  ``ones_for``: a predicate on (file name, function name) of the
    calling wrapper, naming ONE byte workspace that carries integers which form addresses: it is dirtied with the int32
    value 1 per word.

    ``host`` copies an input into a guarded buffer, ``strided`` makes an output with a leading dimension; ``check``
    (after a synchronize) compares every band and gap bit for bit with its fill."""

    active = None
    _NAMES = ("empty", "zeros", "ones", "full", "empty_like", "zeros_like", "ones_like", "full_like")
    _METHODS = ("new_empty", "new_zeros", "new_ones", "new_full", "clone")

    def __init__(self, monkeypatch, device_type="cuda", dirty=False, ones_for=None):
        self.mp, self.device_type, self.dirty, self.ones_for = monkeypatch, device_type, dirty, ones_for
        self.buffers, self._busy, self._ctx, self._caller = [], False, None, ("", "")
        self._orig = {n: getattr(torch, n) for n in self._NAMES}
        self._orig.update({n: getattr(torch.Tensor, n) for n in self._METHODS})

    # ---- activation ----------------------------------------------------------------------------------------------------
    def __enter__(self):
        assert Guard.active is None, "guards do not nest"
        self._ctx = self.mp.context()
        m = self._ctx.__enter__()
        for n in self._NAMES:
            m.setattr(torch, n, self._wrap(n))
        for n in self._METHODS:
            m.setattr(torch.Tensor, n, self._wrap(n))
        Guard.active = self
        return self

    def __exit__(self, *exc):
        Guard.active = None
        return self._ctx.__exit__(*exc)

    # ---- the factories -------------------------------------------------------------------------------------------------
    @staticmethod
    def _shape(args, kw):
        if "size" in kw:
            return kw.pop("size"), args
        if args and isinstance(args[0], (tuple, list, torch.Size)):
            return args[0], args[1:]
        n = 0
        while n < len(args) and not isinstance(args[n], (str, torch.dtype, torch.device)) and hasattr(args[n], "__index__"):
            n += 1
        return args[:n], args[n:]

    def _wrap(self, name):
        orig, kind = self._orig[name], name.replace("new_", "").replace("_like", "")
        like, method = name.endswith("_like"), name.startswith("new_")

        def clone(src, *args, **kw):
            """``Tensor.clone`` with a contiguous result, outside autograd: the copy is what a runner hands to an in-place
            kernel (Adam's p / m / v) or returns as its output"""
            from torch._prims_common import is_non_overlapping_and_dense
            # torch gives a contiguous copy of a contiguous tensor and of one with gaps (a column slice); a dense
            # permuted tensor keeps its strides, which a contiguous interior cannot offer
            contiguous_result = src.is_contiguous() or not is_non_overlapping_and_dense(src)
            in_autograd = src.requires_grad and torch.is_grad_enabled()       # (the copy must stay in the graph)
            plain_call = not args and not kw
            ours = src.device.type == self.device_type and src.layout == torch.strided and src.dtype in _ITEMSIZE_OK
            if self._busy or not (plain_call and ours and contiguous_result and not in_autograd):
                return orig(src, *args, **kw)
            guarded = self.owns(src)
            t = self._alloc(f"clone{list(src.shape)}:{str(src.dtype)[6:]}", tuple(src.shape), src.dtype, src.device, "clone")
            self.buffers[-1].source_guarded = guarded
            self._busy = True
            try:
                t.copy_(src.detach())
            finally:
                self._busy = False
            return t
        if name == "clone":
            return clone

        def factory(*args, **kw):
            if self._busy:
                return orig(*args, **kw)
            args0, kw0 = args, dict(kw)
            try:
                src = None
                if like or method:
                    src, args = args[0], args[1:]
                    if "input" in kw and like:
                        raise TypeError
                if kw.get("out") is not None or kw.get("names") is not None or kw.get("pin_memory") \
                        or kw.get("layout", torch.strided) != torch.strided \
                        or kw.get("memory_format", torch.contiguous_format) not in (torch.contiguous_format,
                                                                                    torch.preserve_format):
                    return orig(*args0, **kw0)
                if like:
                    if not src.is_contiguous() or src.layout != torch.strided:
                        return orig(*args0, **kw0)            # (preserve_format would keep the strides)
                    shape = src.shape
                else:
                    shape, args = self._shape(args, kw)
                fill = None
                if kind == _FULL:
                    fill = kw.pop("fill_value") if "fill_value" in kw else args[0]
                    args = args[1:] if "fill_value" not in kw0 else args
                if args:
                    raise TypeError                        # positional dtype etc.: not a form the package uses
                device = kw.get("device")
                device = torch.device(device) if device is not None else (src.device if src is not None
                                                                         else torch.get_default_device())
                if device.type != self.device_type:
                    return orig(*args0, **kw0)
                dtype = kw.get("dtype")
                if dtype is None:
                    if src is not None:
                        dtype = src.dtype
                    elif kind == _FULL and not isinstance(fill, float):
                        dtype = torch.bool if isinstance(fill, bool) else torch.int64 if isinstance(fill, int) else None
                        if dtype is None:
                            return orig(*args0, **kw0)       # a tensor fill value: let torch infer
                    else:
                        dtype = torch.get_default_dtype()
                if dtype.is_complex or dtype not in _ITEMSIZE_OK:
                    return orig(*args0, **kw0)
                shape = tuple(int(s) for s in shape)
            except (TypeError, IndexError, AttributeError):
                return orig(*args0, **kw0)
            frame = sys._getframe(1)
            self._caller = (os.path.basename(frame.f_code.co_filename), frame.f_code.co_name)
            t = self._alloc(f"{name}{list(shape)}:{str(dtype)[6:]}", shape, dtype, device, kind, fill)
            return t.requires_grad_() if kw.get("requires_grad") else t
        return factory

    # ---- allocation ----------------------------------------------------------------------------------------------------
    def _flat(self, nbytes, device):
        return self._orig["empty"](nbytes, dtype=torch.uint8, device=device)

    def _alloc(self, name, shape, dtype, device, kind, fill=None, band_value=None, ld=None):
        """``ld``: leading dimension in elements of a 2-D interior (gap columns ld - cols, registered and filled)"""
        self._busy = True
        try:
            item = torch.empty((), dtype=dtype).element_size()
            numel = int(np.prod(shape)) if shape else 1
            if ld is not None and numel:
                rows, cols = shape
                numel = (rows - 1) * ld + cols               # the last row ends at its last column: the back band is tight
            nbytes = numel * item
            band = guard_band_bytes(shape if ld is None else (shape[0], ld), item)
            flat = self._flat(band + nbytes + band, device)
            buf = _Buffer(f"#{len(self.buffers)} {name}", flat, band, nbytes, _sentinel(dtype, band_value), None, kind)
            buf.fill(buf.region("front"))
            buf.fill(buf.region("back"))
            # (not a view: a tensor of its own on the flat buffer's storage, as a fresh allocation has no ._base - the
            # slab hand-off recognises a buffer the library allocated by the tag on the tensor a slice's ._base names)
            def own(shape_, stride_, offset=0):
                return self._orig["empty"](0, dtype=dtype, device=device).set_(flat.untyped_storage(),
                                                                              band // item + offset, shape_, stride_)
            inner = own((numel,), (1,))
            if kind == _EMPTY:
                if self.dirty:
                    if dtype == torch.uint8 and self.ones_for is not None and self.ones_for(*self._caller):
                        buf.pattern = torch.ones(1, dtype=torch.int32).view(torch.uint8).to(device)   # the int32 value 1
                        buf.fill(flat[band:band + nbytes])
                        buf.pattern = _sentinel(dtype, band_value).to(device)
                    else:
                        buf.fill(flat[band:band + nbytes])
                else:
                    inner.zero_()
            elif kind == _ZEROS:
                inner.zero_()
            elif kind == _ONES:
                inner.fill_(1)
            elif kind == _FULL:
                inner.fill_(fill)
            if ld is None:
                strides, acc = [], 1
                for d in reversed(shape):
                    strides.append(acc)
                    acc *= max(d, 1)
                buf.view = own(shape, tuple(reversed(strides)))
            else:
                buf.view = own(shape, (ld, 1))
                if numel and shape[0] > 1 and ld > shape[1]:
                    buf.gap = torch.as_strided(inner, (shape[0] - 1, ld - shape[1]), (ld, 1),
                                               inner.storage_offset() + shape[1])
                    buf.gap_fill = torch.tensor([band_value], dtype=dtype, device=device) if band_value is not None \
                        else buf.pattern.view(dtype) if dtype != torch.uint8 else torch.ones(1, dtype=dtype, device=device)
                    buf.gap.copy_(buf.gap_fill.expand_as(buf.gap))
            self.buffers.append(buf)
            return buf.view
        finally:
            self._busy = False

    def host(self, t, slack_fill=None, name="input", in_place=None, device=None):
        """``t`` copied into a guarded buffer on ``device`` (a [rows, cols] tensor with row stride > cols keeps its leading
        dimension, the gap columns holding the slack).  The slack - both bands, the gaps - holds NaN, or ``slack_fill``
        (index inputs: a valid index).  ``in_place``: the section of INTEGRATION.md that documents this operand as
        written in place; every other hosted input must keep its bits (rule 2)."""
        device = torch.device(device) if device is not None else t.device
        ld = t.stride(0) if t.dim() == 2 and t.size(0) > 1 and t.stride(1) == 1 and t.stride(0) > t.size(1) else None
        v = self._alloc(f"{name}{list(t.shape)}:{str(t.dtype)[6:]}", tuple(t.shape), t.dtype, device, "host",
                        band_value=slack_fill, ld=ld)
        self._busy = True
        try:
            v.copy_(t)
            buf = self.buffers[-1]
            buf.snapshot, buf.in_place = v.clone(), in_place
        finally:
            self._busy = False
        return v

    def watch(self, t, name=None):
        """Treat the whole interior of the registered buffer that holds ``t`` as an input from now on: its bits, slack
        and gap columns included, must not change (rule 2)."""
        self._busy = True
        try:
            buf = next(b for b in self.buffers if b.contains(t))
            buf.view = buf.flat[buf.front:buf.front + buf.nbytes]
            buf.snapshot = buf.view.clone()
            buf.name = buf.name if name is None else f"{buf.name} ({name})"
        finally:
            self._busy = False

    def strided(self, rows, cols, ld, dtype=torch.float32, device=None, name="strided output"):
        """a dirty [rows, cols] output with leading dimension ``ld``: the gap columns hold the sentinel (rule 1)"""
        device = torch.device(device if device is not None else self.device_type)
        return self._alloc(f"{name}[{rows}, {cols}; ld {ld}]", (rows, cols), dtype, device, _EMPTY if self.dirty else _ZEROS,
                           ld=ld if ld != cols else None)

    # ---- the checks ----------------------------------------------------------------------------------------------------
    def owns(self, t):
        """``t`` lies inside the interior of a registered buffer"""
        return any(b.contains(t) for b in self.buffers)

    def _probes(self):
        for b in self.buffers:
            yield b, "front band", b.differs(b.region("front"))
            yield b, "back band", b.differs(b.region("back"))
            if b.gap is not None:
                yield b, "gap columns", bits(b.gap) != bits(b.gap_fill)
            if b.snapshot is not None and b.in_place is None:
                yield b, "interior of an input", bits(b.view) != bits(b.snapshot)

    def violations(self):
        """-> [(rule, text)]: rule 1, a band or a gap no longer holds its fill (buffer, side, first offset in elements of
        the comparison); rule 2, the interior of a hosted input changed.  Call after a synchronize."""
        self._busy = True
        try:
            probes = list(self._probes())
            if not probes or not bool(torch.stack([d.any() for _, _, d in probes]).any()):
                return []
            out = []
            for b, side, d in probes:
                if bool(d.any()):
                    first = int(d.reshape(-1).nonzero()[0])
                    if side == "front band":                  # distance from the interior, in words of the fill
                        first = first - d.numel()
                    out.append((2 if side.startswith("interior") else 1,
                                f"{b.name}: {side} changed, {int(d.sum())} words, first at offset {first}"))
            return out
        finally:
            self._busy = False

    def check(self):
        bad = self.violations()
        assert not bad, "\n".join(f"rule {r}: {t}" for r, t in bad)


_ITEMSIZE_OK = {torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.int8, torch.uint8, torch.int16,
                torch.int32, torch.int64, torch.bool}


def strided_out(rows, cols, ld, dtype=torch.float32, device="cuda"):
    """A [rows, cols] output with leading dimension ``ld``: under an active Guard a guarded one with registered gap
    columns, otherwise a plain view of one flat allocation."""
    if Guard.active is not None:
        return Guard.active.strided(rows, cols, ld, dtype, device)
    flat = torch.zeros(max((rows - 1) * ld + cols, 0), dtype=dtype, device=device)
    return torch.as_strided(flat, (rows, cols), (ld, 1))


def guard_rules(run, inputs, monkeypatch, device="cuda", index_inputs=None, in_place=None, trace=None, ones_for=None,
                plain=contextlib.nullcontext, sync=None):
    """The four rules on one case.  ``run``: dict of device tensors -> list of output tensors; ``inputs``: dict of CPU
    tensors; ``index_inputs``: {name: largest valid index} (their slack is run once with 0 and once with that index);
    ``in_place``: {name: where the library documents that operand as written in place}; ``trace``: callable(fn) ->
    (result, {kernel: launches}), or None.

    -> {"violations": [(rule, text)], "buffers": buffers guarded, "owned": per output, inside a registered buffer,
        "plain": the outputs of the first plain run, "launched": what ``trace`` recorded for the second}
       rule 0: two plain runs differ in some bit;   rule 1: a band or gap was written;   rule 2: an input changed;
       rule 3: the guarded run (NaN / index slack, fresh interiors) differs from the plain run;
       rule 4: the guarded run with every ``empty`` interior dirty differs from the guarded run with fresh interiors;
       rule "dispatch": the guarded run launched other kernels than the plain run."""
    index_inputs, in_place = index_inputs or {}, in_place or {}
    sync = sync or (torch.cuda.synchronize if torch.device(device).type == "cuda" else (lambda: None))
    trace = trace or (lambda fn: (fn(), None))
    out = {"violations": [], "buffers": 0, "owned": None, "plain": None}
    bad = out["violations"]

    def fresh():
        return {k: v.to(device, copy=True) for k, v in inputs.items()}

    def differing(a, b):
        return [j for j, (x, y) in enumerate(zip(a, b))if not bits_equal(x, y)] + ([-1] if len(a) != len(b) else [])

    with plain():
        keep = [fresh(), fresh()]
        # (the launches of the SECOND run: the first may build what the case keeps, a graph index, prepared weights)
        (p1, _), (p2, counts1) = trace(lambda: run(keep[0])), trace(lambda: run(keep[1]))
        sync()
    out["plain"], out["launched"] = p1, counts1
    if differing(p1, p2):
        bad.append((0, f"two plain runs differ in outputs {differing(p1, p2)}"))

    def guarded(dirty, slack):
        with Guard(monkeypatch, torch.device(device).type, dirty=dirty, ones_for=ones_for) as g:
            hosted = {k: g.host(v, slack_fill=None if k not in index_inputs else 0 if slack == 0 else index_inputs[k],
                                 name=k, in_place=in_place.get(k), device=device) for k, v in inputs.items()}
            res, counts = trace(lambda: run(hosted))
            sync()
            bad.extend(g.violations())
            if counts is not None and counts != counts1:
                bad.append(("dispatch", f"guarded run launched {counts}, plain run {counts1}"))
            out["buffers"] += len(g.buffers)
            out["owned"] = [g.owns(o) for o in res]
            return res
    clean = guarded(False, 0)
    if differing(clean, p1):
        bad.append((3, f"outputs {differing(clean, p1)} depend on the slack next to an input (NaN / index 0)"))
    if index_inputs:
        other = guarded(False, 1)
        if differing(other, p1):
            bad.append((3, f"outputs {differing(other, p1)} depend on the slack next to an index input (N - 1)"))
    dirty = guarded(True, 0)
    if differing(dirty, clean):
        bad.append((4, f"outputs {differing(dirty, clean)} depend on what their buffers or a workspace held before"))
    return out
