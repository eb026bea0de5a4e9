"""NaN and Inf are never swallowed and never leak.

Every case fixes an operation, clean finite inputs and ONE poison (NaN, +Inf, -Inf) at one position, and compares the
HIP kernel with a plain float64 restatement of the same operation on the CPU (``index_add_``, ``scatter_reduce(...,
'amax', include_self=False)``, per-segment ``softmax``, ``clamp_min(0)``), in which NaN is absorbing through ``+``,
``*``, ReLU, softmax and max.  R, the reach set, is where that restatement is non-finite under the NaN poison.

1. no swallowing: with NaN the kernel is non-finite on all of R; with +-Inf wherever the restatement for that poison is;
2. containment:   outside R the kernel's output has the bits of its own output on the clean inputs, for all three;
3. selection:     the max aggregations with +-Inf equal the restatement exactly, everywhere.

No tolerance anywhere: ``isfinite``, a float64 equality, or ``torch.equal`` on bits.  Only kernels that form no address
and no loop bound from a float value are fed a poison (dense, hop, segment, softmax, attention, loss, Adam); fps, knn,
radius, knn_interpolate, DynamicEdgeConv's graph build, NodeOrder.morton, the SplineConv basis and the CSR builds select
indices by their input and are out of scope.

``test_references_propagate_and_reach_sets_are_proper`` runs without a GPU: it checks the restatements themselves (NaN
through ReLU, amax and a softmax segment) and that in every case both R and its complement are non-empty, so that no
case passes vacuously.

Graphs: ``helpers.random_multigraph`` (duplicates, self loops, isolated tail nodes) at N = 67 and N = 259 - ragged
against 4 and 8 rows per workgroup - with E = 6 N, and N = 1 with one self loop.
"""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import (POISONS, assert_contained, assert_not_swallowed, assert_selection, edge_placements,
                           element_placements, graph_rows, linear_spline_basis, load_golden, poisoned, random_multigraph,
                           reach_sets)

gpu = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


# --------------------------------------------------------------------------- #
# the cases: built on the CPU at import (random inputs, index arrays, closures), run on the GPU by test_nonfinite
# --------------------------------------------------------------------------- #
class Case:
    """``inputs``: dict of CPU tensors (float32 / bfloat16); ``ref``: dict of float64 tensors -> list of float64
    outputs; ``run``: dict of device tensors -> list of device outputs (fresh tensors, inputs untouched); ``targets``:
    placement id -> (input name, index tuple).  ``selection``: rule 3 applies; ``contain``: rule 2 applies (not where
    the issue states that R is whole rows / columns of a reduction over the nodes and only rule 1 is informative);
    ``poisons``: the poison ids used (layers: NaN alone)."""

    def __init__(self, inputs, ref, run, targets, selection=False, contain=True, poisons=("nan", "+inf", "-inf"),
                 env=None):
        #: a dict, or - the large shapes, shared between their cases - a callable -> (dict, its float64 copy)
        self._inputs, self._inputs64 = inputs, None
        self.ref, self.run, self.targets = ref, run, targets
        self.selection, self.contain, self.poisons, self.env = selection, contain, poisons, env or {}

    @property
    def inputs(self):
        return self._inputs()[0] if callable(self._inputs) else self._inputs

    def inputs64(self):
        if callable(self._inputs):
            return self._inputs()[1]
        if self._inputs64 is None:
            self._inputs64 = {k: v.double() for k, v in self._inputs.items()}
        return self._inputs64

    @functools.lru_cache(maxsize=32)
    def reach(self, pid, poison="nan"):
        name, index = self.targets[pid]
        return reach_sets(self.ref, self.inputs64(), name, index, dict(POISONS)[poison])


CASES = {}


def add(cid, *args, **kw):
    assert cid not in CASES, cid
    CASES[cid] = Case(*args, **kw)


def _rand(gen, *shape, scale=1.0):
    """uniform in +-scale, no exact zero (a zero weight would cut a row out of a reach set)"""
    t = (torch.rand(*shape, generator=gen) * 2 - 1) * scale
    return torch.where(t == 0, torch.full_like(t, 0.5 * scale), t)


def _grid(gen, *shape):
    """multiples of 0.25 in [-2, 2]: ties between the candidates of a maximum are certain"""
    return torch.randint(-8, 9, shape, generator=gen).float() / 4


def _gen(*key):
    """a generator seeded by the case's key (not by hash(): that changes from process to process)"""
    return torch.Generator().manual_seed(sum((i + 1) * sum(map(ord, str(k))) for i, k in enumerate(key)))


#: N -> edge_index (numpy int64 [2, E])
GRAPHS = {67: random_multigraph(67, 6 * 67, 67), 259: random_multigraph(259, 6 * 259, 259),
          1: np.zeros((2, 1), np.int64)}


def cpu_csr(ei, n):
    """the stably sorted by-destination set: ptr [n + 1], other (sources), perm (input edge of each position)"""
    order = np.argsort(ei[1], kind="stable")
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(ei[1], minlength=n), out=ptr[1:])
    return ptr, ei[0][order], order


def gcn_weights(ei, n, loops=False):
    """float64 gcn_norm: deg^-1/2 (inf -> 0) at both ends; -> (edge_index with the remaining self loops, weights)"""
    if loops:
        keep = ei[0] != ei[1]
        ei = np.concatenate([ei[:, keep], np.stack([np.arange(n), np.arange(n)])], axis=1)
    deg = np.bincount(ei[1], minlength=n).astype(np.float64)
    dis = np.where(deg > 0, np.maximum(deg, 1.0) ** -0.5, 0.0)
    return ei, torch.from_numpy(dis[ei[0]] * dis[ei[1]])


def ref_spmm(ei, w, x, n_out=None):
    """sum over the edges j -> i of w_e x[j]: index_add_ in float64"""
    src, dst = torch.from_numpy(ei[0]), torch.from_numpy(ei[1])
    msg = x[src] if w is None else w.unsqueeze(1) * x[src]
    return torch.zeros(n_out if n_out is not None else x.size(0), x.size(1), dtype=torch.float64).index_add_(0, dst, msg)


def ref_amax(index, rows, n_out):
    """scatter_reduce amax, include_self=False on zeros: a row without candidates is 0, a NaN candidate wins"""
    idx = index.unsqueeze(1).expand(-1, rows.size(1))
    return torch.zeros(n_out, rows.size(1), dtype=torch.float64).scatter_reduce(0, idx, rows, "amax", include_self=False)


def ref_segment_softmax(logit, index, n):
    """softmax of the rows of ``logit`` [E, H] per segment ``index``: one NaN logit makes its whole segment NaN"""
    out = torch.empty_like(logit)
    for i in index.unique().tolist():
        sel = index == i
        out[sel] = torch.softmax(logit[sel], dim=0)
    return out


def _graph(ei, n, **kw):
    from deformcontact_amd.graph import GraphIndex
    return GraphIndex(torch.from_numpy(ei).to(DEV), n, **kw)


def _lazy(fn):
    """device-side state of a case (a GraphIndex, prepared weights), built at the first run"""
    return functools.lru_cache(maxsize=None)(fn)


def _st():
    from deformcontact_amd.graph import current_stream_ptr
    return current_stream_ptr(torch.device(DEV))


# ---- dense blocks through the C entries --------------------------------------------------------------------------------
DENSE_SHAPES = [(208, 256, 256, 4), (144, 32, 48, 2), (67, 7, 256, 1)]
RELU_BIAS = [(1, 1), (0, 0), (1, 0), (0, 1)]


def _dense_ref(nseg, fi, relu, bias_on):
    def ref(t):
        x, w = t["x"], t["w"]
        out = sum(x[:, s * fi:(s + 1) * fi] @ w[s].t() for s in range(nseg))
        if bias_on:
            out = out + t["b"]
        return [out.clamp_min(0) if relu else out]
    return ref


def _dense_run(entry, n, fi, fo, nseg, relu, bias_on):
    def run(t):
        from deformcontact_amd import _lib, ops
        from deformcontact_amd.ops import _i64_array, _ptr_array
        L, st = _lib.lib(), _st()
        slab, ws = t["x"], [t["w"][s] for s in range(nseg)]
        xs, ld = [slab[:, s * fi:(s + 1) * fi] for s in range(nseg)], [nseg * fi] * nseg
        bp = t["b"].data_ptr() if bias_on else None
        out = torch.empty(n, fo, device=DEV)
        head = (_ptr_array(xs), _i64_array(ld), _ptr_array(ws), nseg, bp, relu, out.data_ptr(), fo, n, fi, fo)
        if entry == "fwd":
            rc = L.dc_tag_linear_fwd(*head, st)
        elif entry in ("split6", "split3"):
            rc = L.dc_tag_linear_fwd_split(*head, int(entry[-1]), st)
        else:
            # the row maxima are the product's own (auxiliary outputs: judged through their consumer)
            rowmax, wmax = ops.rowabsmax(slab), ops.weight_rowmax(ws)
            if entry == "h2":
                rc = L.dc_tag_linear_fwd_h2(*head, rowmax.data_ptr(), wmax.data_ptr(), st)
            else:
                k = nseg * fi
                wm, wimg = torch.empty(fo, device=DEV), torch.empty(fo, k, device=DEV)
                _lib.check(L.dc_tag_weight_prep(_ptr_array(ws), nseg, fo, fi, wm.data_ptr(), wimg.data_ptr(), None, None,
                                                st), "weight_prep")
                wsk, wsb = None, 0
                if entry == "h2p_splitk":
                    wsb = L.dc_tag_linear_fwd_h2p_workspace_bytes(n, k, fo)
                    assert wsb > 0, "this shape has no cut reduction: the case would not run the split-K form"
                    wsk = torch.empty(wsb, dtype=torch.uint8, device=DEV)
                rc = L.dc_tag_linear_fwd_h2p(slab.data_ptr(), k, wimg.data_ptr(), bp, relu, out.data_ptr(), fo, n, k, fo,
                                             rowmax.data_ptr(), wm.data_ptr(), wsk.data_ptr() if wsk is not None else None,
                                             wsb, st)
        _lib.check(rc, entry)
        return [out]
    return run


def _dense_inputs(n, fi, fo, nseg, key):
    gen = _gen("dense", n, fi, fo, nseg, key)
    return {"x": _rand(gen, n, nseg * fi), "w": _rand(gen, nseg, fo, fi, scale=fi ** -0.5), "b": _rand(gen, fo, scale=0.5)}


def _dense_targets(n, k, fo, nseg, fi):
    return {"x_first": ("x", (0, 0)), "x_mid": ("x", (n // 2, k // 2)), "x_lastrow": ("x", (n - 1, 1)),
            "x_lastcol": ("x", (n // 3, k - 1)), "w": ("w", (nseg - 1, fo // 2 + 1, fi - 1))}


for (n, fi, fo, nseg) in DENSE_SHAPES:
    for entry in ("fwd", "split6", "split3", "h2", "h2p", "h2p_splitk"):
        if entry.startswith("h2") and fi % 16:
            continue                                     # the fp16x2 block needs Fi % 16 == 0
        if entry == "h2p_splitk" and (n, fi) != (208, 256):
            continue                                     # the cut reduction exists from a long K on
        for relu, bias_on in ([(0, 0)] if entry == "h2p_splitk" else RELU_BIAS):
            add(f"dense-{entry}-{n}x{fi}x{fo}x{nseg}-relu{relu}-bias{bias_on}", _dense_inputs(n, fi, fo, nseg, 0),
                _dense_ref(nseg, fi, relu, bias_on), _dense_run(entry, n, fi, fo, nseg, relu, bias_on),
                _dense_targets(n, nseg * fi, fo, nseg, fi))


def _narrow_run(img, n, fi, nseg, wpad, relu, bias_on):
    def run(t):
        from deformcontact_amd import _lib
        from deformcontact_amd.ops import _ptr_array
        L, st, fo = _lib.lib(), _st(), 256
        assert L.dc_tag_linear_fwd_narrow_ok(fi, nseg, wpad, fo) == 1
        slab = torch.zeros(n, wpad, device=DEV)
        slab[:, :nseg * fi] = t["x"]
        ws = [t["w"][s] for s in range(nseg)]
        bp = t["b"].data_ptr() if bias_on else None
        out = torch.empty(n, fo, device=DEV)
        if img:
            buf = torch.zeros(wpad // 16 * 24576, dtype=torch.uint8, device=DEV)
            _lib.check(L.dc_tag_narrow_wimage(_ptr_array(ws), nseg, fi, wpad, buf.data_ptr(), st), "wimage")
            rc = L.dc_tag_linear_fwd_narrow_img(slab.data_ptr(), wpad, buf.data_ptr(), bp, relu, out.data_ptr(), fo, n,
                                                wpad, fo, st)
        else:
            rc = L.dc_tag_linear_fwd_narrow(slab.data_ptr(), wpad, _ptr_array(ws), nseg, fi, bp, relu, out.data_ptr(), fo,
                                            n, wpad, fo, st)
        _lib.check(rc, "narrow")
        return [out]
    return run


for (n, fi, nseg, wpad) in [(67, 3, 4, 96), (259, 32, 4, 128)]:
    for img in (False, True):
        for relu, bias_on in RELU_BIAS:
            add(f"dense-narrow{'_img' if img else ''}-{n}x{fi}x{nseg}-relu{relu}-bias{bias_on}",
                _dense_inputs(n, fi, 256, nseg, 1), _dense_ref(nseg, fi, relu, bias_on),
                _narrow_run(img, n, fi, nseg, wpad, relu, bias_on), _dense_targets(n, nseg * fi, 256, nseg, fi))


def _bf16_run(n, k, fo, relu, bias_on, out_bf16):
    def run(t):
        from deformcontact_amd import _lib
        L = _lib.lib()
        a, w = t["x"].contiguous(), t["w"][0].contiguous()
        out = torch.empty(n, fo, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=DEV)
        _lib.check(L.dc_tag_linear_fwd_bf16(a.data_ptr(), k, w.data_ptr(), t["b"].data_ptr() if bias_on else None, relu,
                                            out.data_ptr(), fo, int(out_bf16), n, k, fo, _st()), "fwd_bf16")
        return [out]
    return run


for (n, k, fo) in [(67, 64, 40), (208, 256, 256)]:
    for relu, bias_on in RELU_BIAS:
        for out_bf16 in (False, True):
            inp = _dense_inputs(n, k, fo, 1, 2)
            inp["x"], inp["w"] = inp["x"].bfloat16(), inp["w"].bfloat16()
            add(f"dense-bf16-{n}x{k}x{fo}-relu{relu}-bias{bias_on}-{'bf16' if out_bf16 else 'f32'}", inp,
                _dense_ref(1, k, relu, bias_on), _bf16_run(n, k, fo, relu, bias_on, out_bf16),
                _dense_targets(n, k, fo, 1, k))


# The tile kernels of the shipped sizes.  A launch takes them only when it fills the chip: k_fwd_h2d / k_fwd_h2w from 128
# tiles of 128 x 256 on (h2d from K = 256 on, k_fwd_h2w below), k_fwd_bf16x from 160 tiles of 256 x 256 on.  Rows that fill
# the tiles (the FULL form) and rows that do not; the kernel that ran is read from the library's launch log.
def _traced(run, expect):
    def traced(t):
        from deformcontact_amd import _lib
        _lib.kernel_trace(True)
        try:
            out = run(t)
            counts = _lib.kernel_trace_counts()
        finally:
            _lib.kernel_trace(False)
        assert any(expect in name for name in counts), (expect, counts)
        return out
    return traced


@functools.lru_cache(maxsize=2)
def _big_inputs(n, k, fo, bf16):
    inp = _dense_inputs(n, k, fo, 1, 3)
    if bf16:
        inp["x"], inp["w"] = inp["x"].bfloat16(), inp["w"].bfloat16()
    return inp, {name: v.double() for name, v in inp.items()}


def _big_targets(n, k, fo, x_first=True):
    tg = {"x_first": ("x", (0, 0))} if x_first else {}
    tg.update({"x_last": ("x", (n - 1, k - 1)), "w": ("w", (0, fo // 2 + 1, k - 1))})
    return tg


for k, kern in ((256, "k_fwd_h2d"), (96, "k_fwd_h2w")):
    for n, full in ((16384, "true"), (16384 + 67, "false")):
        for relu, bias_on in RELU_BIAS:
            add(f"dense-{kern[6:]}-{n}x{k}x256-relu{relu}-bias{bias_on}", functools.partial(_big_inputs, n, k, 256, False),
                _dense_ref(1, k, relu, bias_on), _traced(_dense_run("h2p", n, k, 256, 1, relu, bias_on), f"{kern}<{full}>"),
                _big_targets(n, k, 256))
for n in (40960, 40960 + 3):
    for i, (relu, bias_on) in enumerate(RELU_BIAS):
        add(f"dense-bf16x-{n}x64x256-relu{relu}-bias{bias_on}-{'bf16' if i % 2 else 'f32'}",
            functools.partial(_big_inputs, n, 64, 256, True), _dense_ref(1, 64, relu, bias_on),
            _traced(_bf16_run(n, 64, 256, relu, bias_on, bool(i % 2)), "k_fwd_bf16x"), _big_targets(n, 64, 256, False))


# ---- dense backward: the poison sits in the incoming gradient (one element, one whole row) ---------------------------
def _masked(t):
    """threshold_backward: a SELECTION by the forward output (out > 0), not a product with a 0 / 1 mask"""
    return torch.where(t["y"] > 0, t["g"], torch.zeros_like(t["g"])) if "y" in t else t["g"]


def _bwd_inputs(n, fi, fo, nseg, masked, targets):
    gen = _gen("bwd", n, fi, fo, nseg, masked)
    inp = {"g": _rand(gen, n, fo), "w": _rand(gen, nseg, fo, fi, scale=fi ** -0.5), "x": _rand(gen, n, nseg * fi)}
    if masked:
        inp["y"] = _rand(gen, n, fo)                     # the forward output the ReLU mask is read from
        for _, index in targets.values():
            inp["y"][index] = 1.0                        # the poisoned gradient elements pass the mask
    return inp


def _dx_run(entry, n, fi, fo, nseg):
    def run(t):
        from deformcontact_amd import _lib, ops
        from deformcontact_amd.ops import _i64_array, _ptr_array
        L, st = _lib.lib(), _st()
        g, ws = t["g"], [t["w"][s] for s in range(nseg)]
        mask = t["y"].data_ptr() if "y" in t else None
        gslab = torch.zeros(n, nseg * fi, device=DEV)
        gxs, ld = [gslab[:, s * fi:(s + 1) * fi] for s in range(nseg)], [nseg * fi] * nseg
        if entry == "dx":
            rc = L.dc_tag_linear_bwd_dx(g.data_ptr(), fo, mask, fo, _ptr_array(ws), nseg, _ptr_array(gxs), _i64_array(ld),
                                        n, fi, fo, st)
        else:
            wsb = L.dc_tag_linear_bwd_dx_split_workspace_bytes(fi, fo, nseg)
            wsx = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
            if entry == "dx_h2":
                gmax, wmax = ops.rowabsmax(g), ops.weight_rowmax(ws)
                rc = L.dc_tag_linear_bwd_dx_h2(g.data_ptr(), fo, mask, fo, _ptr_array(ws), nseg, _ptr_array(gxs),
                                               _i64_array(ld), wsx.data_ptr(), wsb, n, fi, fo, gmax.data_ptr(),
                                               wmax.data_ptr(), st)
            else:
                rc = L.dc_tag_linear_bwd_dx_split(g.data_ptr(), fo, mask, fo, _ptr_array(ws), nseg, _ptr_array(gxs),
                                                  _i64_array(ld), wsx.data_ptr(), wsb, n, fi, fo, 6, st)
        _lib.check(rc, entry)
        return [gslab]
    return run


def _dx_ref(nseg):
    return lambda t: [torch.cat([_masked(t) @ t["w"][s] for s in range(nseg)], dim=1)]


def _g_targets(n, fo):
    return {"g_first": ("g", (0, 0)), "g_mid": ("g", (n // 2, fo // 2)), "g_last": ("g", (n - 1, fo - 1)),
            "g_row": ("g", (n // 2 + 1,))}


for (n, fi, fo, nseg) in DENSE_SHAPES:
    for entry in ("dx", "dx_split6", "dx_h2"):
        if entry == "dx_h2" and (fo % 16 or fi % 4):
            continue
        for masked in (False, True):
            tg = _g_targets(n, fo)
            add(f"dense-{entry}-{n}x{fi}x{fo}x{nseg}-mask{int(masked)}", _bwd_inputs(n, fi, fo, nseg, masked, tg),
                _dx_ref(nseg), _dx_run(entry, n, fi, fo, nseg), tg)


def _dw_run(entry, n, fi, fo, nseg):
    def run(t):
        from deformcontact_amd import _lib, ops
        from deformcontact_amd.ops import _i64_array, _ptr_array
        L, st = _lib.lib(), _st()
        g, slab = t["g"], t["x"]
        gws, gb = [torch.empty(fo, fi, device=DEV) for _ in range(nseg)], torch.empty(fo, device=DEV)
        if entry == "dw_bf16":
            nbytes = L.dc_tag_linear_bwd_dw_bf16_workspace_bytes(n, fi, fo, nseg)
            scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
            rc = L.dc_tag_linear_bwd_dw_bf16(g.data_ptr(), fo, slab.data_ptr(), nseg * fi, nseg, _ptr_array(gws),
                                             gb.data_ptr(), 0, scratch.data_ptr(), nbytes, n, fi, fo, st)
        else:
            mask = t["y"].data_ptr() if "y" in t else None
            xs, ld = [slab[:, s * fi:(s + 1) * fi] for s in range(nseg)], [nseg * fi] * nseg
            nbytes = L.dc_tag_linear_bwd_dw_workspace_bytes(n, fi, fo, nseg)
            scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
            head = (g.data_ptr(), fo, mask, fo, _ptr_array(xs), _i64_array(ld), nseg, _ptr_array(gws), nseg, fi,
                    gb.data_ptr(), 0, scratch.data_ptr(), nbytes, n, fi, fo)
            if entry == "dw":
                rc = L.dc_tag_linear_bwd_dw(*head, st)
            else:
                gmax, xmax = ops.rowabsmax(g), ops.rowabsmax(slab)
                rc = L.dc_tag_linear_bwd_dw_h2(*head, gmax.data_ptr(), xmax.data_ptr(), st)
        _lib.check(rc, entry)
        return gws + [gb]
    return run


def _dw_ref(nseg, fi):
    def ref(t):
        gm = _masked(t)
        return [gm.t() @ t["x"][:, s * fi:(s + 1) * fi] for s in range(nseg)] + [gm.sum(0)]
    return ref


for (n, fi, fo, nseg) in DENSE_SHAPES:
    for entry in ("dw", "dw_h2", "dw_bf16"):
        if (entry == "dw_h2" and (n % 16 or fi % 4)) or (entry == "dw_bf16" and (fo % 128 or fi % 256)):
            continue
        tg = _g_targets(n, fo)
        inp = _bwd_inputs(n, fi, fo, nseg, entry != "dw_bf16", tg)
        if entry == "dw_bf16":
            inp["g"], inp["x"] = inp["g"].bfloat16(), inp["x"].bfloat16()
        # R is whole rows of dW (and an element of the bias gradient): the contraction runs over the nodes, every
        # scale is per node chunk - only rule 1 is informative
        add(f"dense-{entry}-{n}x{fi}x{fo}x{nseg}", inp, _dw_ref(nseg, fi), _dw_run(entry, n, fi, fo, nseg), tg,
            contain=False)


# ---- hops ---------------------------------------------------------------------------------------------------------------
def _hop_ref(ei, n, weighted, addend):
    w = gcn_weights(ei, n)[1] if weighted else None

    def ref(t):
        y = ref_spmm(ei, w, t["x"])
        return [y + t["a"] if addend else y]
    return ref


def _hop_run(ei, n, weighted, addend, form="plain"):
    g = _lazy(lambda: _graph(ei, n))

    def run(t):
        from deformcontact_amd import ops
        x, a = t["x"], t["a"] if addend else None
        if form == "plain":
            return [ops.hop(g().fwd, x, addend=a, weighted=weighted)]
        if form.startswith("rowmax"):
            rm = torch.zeros(n, device=DEV)
            return [ops.hop(g().fwd, x, addend=a, weighted=weighted, rowmax=rm, rowmax_mode=int(form[-1]))]
        if form.startswith("bf16"):
            od = torch.bfloat16 if form == "bf16_bf16" else torch.float32
            return [ops.hop_bf16(g().fwd, x, addend=None if a is None else a.to(od), weighted=weighted, out_dtype=od)]
        raise AssertionError(form)
    return run


def _hop_inputs(n, f, key):
    gen = _gen("hop", n, f, key)
    return {"x": _rand(gen, n, f), "a": _rand(gen, n, f)}


def _x_targets(ei, n, f):
    return {k: ("x", v) for k, v in element_placements(ei, n, f).items()}


for n in (67, 259, 1):
    for f in (7, 30, 32, 64, 260):                       # every launch_sub / k_spmm_wave branch, vec4 and scalar
        for weighted, addend in [(True, False), (True, True), (False, False), (False, True)]:
            add(f"hop-n{n}-f{f}-w{int(weighted)}-a{int(addend)}", _hop_inputs(n, f, 0),
                _hop_ref(GRAPHS[n], n, weighted, addend), _hop_run(GRAPHS[n], n, weighted, addend),
                _x_targets(GRAPHS[n], n, f))
for n, f, form in [(67, 64, "rowmax0"), (259, 30, "rowmax1"), (259, 256, "rowmax1")]:
    add(f"hop-{form}-n{n}-f{f}", _hop_inputs(n, f, 1), _hop_ref(GRAPHS[n], n, True, False),
        _hop_run(GRAPHS[n], n, True, False, form), _x_targets(GRAPHS[n], n, f))
for n in (67, 259):
    for f in (30, 64):
        for form in ("bf16_bf16", "bf16_f32"):
            for addend in (False, True):
                inp = _hop_inputs(n, f, 2)
                inp["x"] = inp["x"].bfloat16()
                if form == "bf16_bf16":
                    inp["a"] = inp["a"].bfloat16()
                add(f"hop-{form}-n{n}-f{f}-a{int(addend)}", inp, _hop_ref(GRAPHS[n], n, True, addend),
                    _hop_run(GRAPHS[n], n, True, addend, form), _x_targets(GRAPHS[n], n, f))


def _window_case(f):
    """the hop over a ROW WINDOW of a merged (block-diagonal) adjacency: part 1 of two, its rows alone"""
    parts = [(GRAPHS[67], 67), (GRAPHS[259], 259)]
    mg = _lazy(lambda: __import__("deformcontact_amd").graph.GraphIndex.from_parts(
        [(torch.from_numpy(e).to(DEV), k) for e, k in parts]))

    def run(t):
        from deformcontact_amd import ops
        win = mg().window(1)
        assert win.fwd.row_offset > 0
        return [ops.hop(win.fwd, t["x"], weighted=True)]
    ei, n = parts[1]
    add(f"hop-window-f{f}", _hop_inputs(n, f, 3), _hop_ref(ei, n, True, False), run, _x_targets(ei, n, f))


for f in (30, 64):
    _window_case(f)


def _pack_case(n, f):
    """dc_spmm_f32_pack: slab = [x | A x | 0]: the first layer's input copy and first hop in one launch"""
    ei, width, wpad = GRAPHS[n], 4 * f, 96 if 4 * f <= 96 else 128
    g, w = _lazy(lambda: _graph(ei, n)), gcn_weights(ei, n)[1]

    def run(t):
        from deformcontact_amd import _lib
        x, adj = t["x"], g().fwd
        slab = torch.full((n, wpad), 7.0, device=DEV)
        _lib.check(_lib.lib().dc_spmm_f32_pack(adj.ptr.data_ptr(), adj.other.data_ptr(), adj.w.data_ptr(), x.data_ptr(), f,
                                               slab.data_ptr(), wpad, n, f, width, wpad, _st()), "pack")
        return [slab[:, :2 * f].clone(), slab[:, width:].clone()]

    def ref(t):
        return [torch.cat([t["x"], ref_spmm(ei, w, t["x"])], dim=1), torch.zeros(n, wpad - width, dtype=torch.float64)]
    add(f"hop-pack-n{n}-f{f}", _hop_inputs(n, f, 4), ref, run, _x_targets(ei, n, f))


_pack_case(67, 21)
_pack_case(259, 32)


def _bias_act_case(n, f, relu, bias_on):
    """dc_spmm_f32_bias_act: y = act(A x + bias), the GCNConv / GATConv aggregation with its epilogue"""
    ei = GRAPHS[n]
    ei_l, w = gcn_weights(ei, n, loops=True)
    g = _lazy(lambda: _graph(ei, n, self_loops=True))

    def run(t):
        from deformcontact_amd import ops
        return [ops._agg_bias_act(g().fwd, g().fwd.w, t["x"], t["b"] if bias_on else None, bool(relu))]

    def ref(t):
        y = ref_spmm(ei_l, w, t["x"])
        y = y + t["b"] if bias_on else y
        return [y.clamp_min(0) if relu else y]
    inp = _hop_inputs(n, f, 5)
    inp["b"] = _rand(_gen("b", n, f), f, scale=0.5)
    del inp["a"]
    add(f"hop-bias_act-n{n}-f{f}-relu{relu}-bias{bias_on}", inp, ref, run, _x_targets(ei, n, f))


for n, f in [(67, 32), (259, 64), (67, 30)]:             # (30: the scalar form of the epilogue)
    for relu, bias_on in RELU_BIAS:
        _bias_act_case(n, f, relu, bias_on)


def _heads_case(n, nh, c, relu):
    """dc_spmm_f32_heads_bias_act: y[i, h C + j] = act(sum_p alpha[p, h] x[other[p], h C + j] + bias), on a sorted set built here"""
    ei = GRAPHS[n]
    ptr, other, _ = cpu_csr(ei, n)
    e = ei.shape[1]
    dst_sorted = np.repeat(np.arange(n), np.diff(ptr))
    ei_sorted = np.stack([other, dst_sorted])

    def run(t):
        from deformcontact_amd import ops
        from deformcontact_amd.graph import SortedAdjacency
        adj = SortedAdjacency(torch.from_numpy(ptr.astype(np.int32)).to(DEV), torch.from_numpy(other.astype(np.int32)).to(DEV),
                              torch.arange(e, dtype=torch.int32, device=DEV), None)
        return [ops._heads_agg(adj, t["alpha"].contiguous(), t["x"], t["b"], bool(relu), False, nh, c)]

    def ref(t):
        y = torch.cat([ref_spmm(ei_sorted, t["alpha"][:, h], t["x"][:, h * c:(h + 1) * c]) for h in range(nh)], dim=1)
        y = y + t["b"]
        return [y.clamp_min(0) if relu else y]
    gen = _gen("heads", n, nh, c)
    inp = {"x": _rand(gen, n, nh * c), "alpha": torch.rand(e, nh, generator=gen) + 0.1, "b": _rand(gen, nh * c, scale=0.5)}
    tg = _x_targets(ei, n, nh * c)
    tg.update({"alpha_" + k: ("alpha", (v[0], nh - 1 if v[1] else 0)) for k, v in edge_placements(ei_sorted, nh).items()})
    add(f"hop-heads_bias_act-n{n}-h{nh}-c{c}-relu{relu}", inp, ref, run, tg)


for n, nh, c in [(67, 3, 8), (259, 1, 64), (259, 3, 64), (67, 3, 7)]:       # (C = 7: the scalar form)
    for relu in (0, 1):
        _heads_case(n, nh, c, relu)


def _chain_case(f, k):
    """dc_hop_chain_f32: K chained hops of a batch of two graphs with every graph's slice resident in LDS"""
    sizes = (67, 259)
    ei = np.concatenate([GRAPHS[67], GRAPHS[259] + 67], axis=1)
    n = sum(sizes)
    segs = ((0, 67, n), (0, GRAPHS[67].shape[1], ei.shape[1]))
    g, w = _lazy(lambda: _graph(ei, n, segments=segs)), gcn_weights(ei, n)[1]

    def run(t):
        from deformcontact_amd import ops
        slab = ops._alloc_slab(n, (k + 1) * f, DEV)
        slab.zero_()
        slab[:, :f] = t["x"]
        assert ops.hop_chain_eligible(g(), g().fwd, slab, f, k)
        ops.hop_chain(g(), g().fwd, slab, f, k)
        return [slab[:, :(k + 1) * f].clone()]

    def ref(t):
        blocks = [t["x"]]
        for _ in range(k):
            blocks.append(ref_spmm(ei, w, blocks[-1]))
        return [torch.cat(blocks, dim=1)]
    add(f"hop-chain-f{f}-k{k}", _hop_inputs(n, f, 6), ref, run, _x_targets(ei, n, f))


_chain_case(32, 2)


# ---- segment kernels ----------------------------------------------------------------------------------------------------
WIDTHS = (3, 32, 256)


def _raw_graph(ei, n):
    return _lazy(lambda: _graph(ei, n, self_loops=False, normalize=False))


def _ref_aggregate(ei, n_out, rows_of, reduce):
    """sum / mean / max per destination of the rows ``rows_of(t)`` [E, C] (in input-edge order)"""
    dst = torch.from_numpy(ei[1])
    deg = torch.bincount(dst, minlength=n_out).clamp(min=1).double().unsqueeze(1)

    def ref(t):
        rows = rows_of(t)
        if reduce == "max":
            return [ref_amax(dst, rows, n_out)]
        s = torch.zeros(n_out, rows.size(1), dtype=torch.float64).index_add_(0, dst, rows)
        return [s / deg if reduce == "mean" else s]
    return ref


def _sage_fwd_case(n, f, reduce):
    ei = GRAPHS[n]
    g, src = _raw_graph(ei, n), torch.from_numpy(ei[0])

    def run(t):
        from deformcontact_amd import ops
        return [ops.aggregate(g(), t["x"], reduce)]
    gen = _gen("sage", n, f, reduce)
    add(f"seg-sage-{reduce}-n{n}-f{f}", {"x": _grid(gen, n, f) if reduce == "max" else _rand(gen, n, f)},
        _ref_aggregate(ei, n, lambda t: t["x"][src], reduce), run, _x_targets(ei, n, f), selection=reduce == "max")


def _sage_bwd_case(n, f, reduce):
    """finite forward, the poison in the incoming gradient.  The max backward is the library's selection: the gradient
    of m[i, c] goes in equal shares to the edges that attain it, NOTHING (not 0 * g) to the others."""
    ei = GRAPHS[n]
    g, src, dst = _raw_graph(ei, n), torch.from_numpy(ei[0]), torch.from_numpy(ei[1])
    deg = torch.bincount(dst, minlength=n).clamp(min=1).double().unsqueeze(1)

    def run(t):
        from deformcontact_amd import ops
        x = t["x"].clone().requires_grad_(True)
        return list(torch.autograd.grad(ops.aggregate(g(), x, reduce), x, t["gy"]))

    def ref(t):
        x, gy = t["x"], t["gy"]
        if reduce == "max":
            hit = x[src] == ref_amax(dst, x[src], n)[dst]
            cnt = torch.zeros(n, f, dtype=torch.float64).index_add_(0, dst, hit.double())
            msg = torch.where(hit, gy[dst] / cnt[dst].clamp(min=1), torch.zeros_like(gy[dst]))
        else:
            msg = gy[dst] / deg[dst] if reduce == "mean" else gy[dst]
        return [torch.zeros(n, f, dtype=torch.float64).index_add_(0, src, msg)]
    gen = _gen("sageb", n, f, reduce)
    mid, _ = graph_rows(ei, n)
    tg = {"gy_first": ("gy", (0, 0)), "gy_mid": ("gy", (mid, f // 2)), "gy_lastcol": ("gy", (mid // 2, f - 1)),
          "gy_row": ("gy", (mid,))}
    add(f"seg-sage-bwd-{reduce}-n{n}-f{f}", {"x": _grid(gen, n, f) if reduce == "max" else _rand(gen, n, f),
                                             "gy": _rand(gen, n, f)}, ref, run, tg)


for n in (67, 259, 1):
    for f in WIDTHS:
        for reduce in ("mean", "max", "sum"):
            _sage_fwd_case(n, f, reduce)
for n, f in [(67, 3), (259, 32), (67, 256)]:
    for reduce in ("mean", "max"):
        _sage_bwd_case(n, f, reduce)


def _edge_case(n, c, reduce, pointnet):
    ei = GRAPHS[n]
    e = ei.shape[1]
    nd = int(ei[1].max()) + 1 if pointnet else n         # bipartite: only the first nd rows are destinations
    g = _raw_graph(ei, n)

    def run(t):
        from deformcontact_amd import ops
        if pointnet:
            return [ops.pointnet_aggregate(g(), t["m"], reduce, num_dst=nd)]
        return [ops.edge_aggregate(g(), t["m"], reduce)]
    gen = _gen("edge", n, c, reduce, pointnet)
    tg = {k: ("m", v) for k, v in edge_placements(ei, c).items()}
    if e > 1:
        tg["lastedge"] = ("m", (e - 1, c // 2))
    add(f"seg-{'pointnet' if pointnet else 'edge'}-{reduce}-n{n}-c{c}", {"m": _grid(gen, e, c) if reduce == "max" else
                                                                             _rand(gen, e, c)},
        _ref_aggregate(ei, nd, lambda t: t["m"], reduce), run, tg, selection=reduce == "max")


for n in (67, 259, 1):
    for c in WIDTHS:
        for reduce in ("max", "mean", "sum"):
            _edge_case(n, c, reduce, False)
            if n > 1:
                _edge_case(n, c, reduce, True)


def _pool_case(sizes, c, mode):
    """global_{add,mean,max}_pool over a ragged batch with an EMPTY graph in it"""
    n, b = sum(sizes), len(sizes)
    batch = torch.repeat_interleave(torch.arange(b), torch.tensor(sizes))
    cnt = torch.tensor(sizes).clamp(min=1).double().unsqueeze(1)

    def run(t):
        from deformcontact_amd import nn as dcnn
        fn = {"add": dcnn.global_add_pool, "mean": dcnn.global_mean_pool, "max": dcnn.global_max_pool}[mode]
        return [fn(t["x"], batch.to(DEV) if b > 1 else None, b if b > 1 else None)]

    def ref(t):
        if mode == "max":
            return [ref_amax(batch, t["x"], b)]
        s = torch.zeros(b, c, dtype=torch.float64).index_add_(0, batch, t["x"])
        return [s / cnt if mode == "mean" else s]
    gen = _gen("pool", n, c, mode)
    tg = {"first": ("x", (0, 0))}
    if n > 1:
        tg.update({"mid": ("x", (n // 2, c // 2)), "lastrow": ("x", (n - 1, min(1, c - 1))), "lastcol": ("x", (n // 3, c - 1))})
    add(f"seg-pool-{mode}-n{n}-c{c}", {"x": _grid(gen, n, c) if mode == "max" else _rand(gen, n, c)}, ref, run, tg,
        selection=mode == "max")


for sizes in [(1, 37, 0, 150, 71), (67,), (1,)]:
    for c in WIDTHS:
        for mode in ("max", "mean", "add"):
            _pool_case(sizes, c, mode)


def _gine_case(n, f, with_eps):
    ei = GRAPHS[n]
    g, src, dst = _raw_graph(ei, n), torch.from_numpy(ei[0]), torch.from_numpy(ei[1])
    eps = 0.25

    def run(t):
        from deformcontact_amd import ops
        return [ops.gine_aggregate(g(), t["x"], t["e"], torch.tensor([eps], device=DEV) if with_eps else None)]

    def ref(t):
        s = torch.zeros(n, f, dtype=torch.float64).index_add_(0, dst, (t["x"][src] + t["e"]).clamp_min(0))
        return [s + (1 + eps) * t["x"] if with_eps else s]
    gen = _gen("gine", n, f)
    tg = _x_targets(ei, n, f)
    tg.update({k: ("e", v) for k, v in edge_placements(ei, f).items()})
    add(f"seg-gine-n{n}-f{f}-eps{int(with_eps)}", {"x": _rand(gen, n, f), "e": _rand(gen, ei.shape[1], f)}, ref, run, tg)


for n in (67, 259):
    for f in WIDTHS:
        _gine_case(n, f, f != 32)


# ---- loss and optimiser -------------------------------------------------------------------------------------------------
def _loss_case(n):
    ei = GRAPHS[n]
    g, src, dst = _raw_graph(ei, n), torch.from_numpy(ei[0]), torch.from_numpy(ei[1])

    def run(t):
        from deformcontact_amd import ops
        p = t["pred"].clone().requires_grad_(True)
        l1, gcl = ops.contact_losses(g(), p, t["tgt"])
        (grad,) = torch.autograd.grad(l1 + gcl, p)          # train.py: one backward of the weighted sum
        return [l1.detach().reshape(1), gcl.detach().reshape(1), grad]

    def ref(t):
        p = t["pred"].clone().requires_grad_(True)
        l1 = (p - t["tgt"]).abs().mean()
        d = (t["tgt"][dst] - t["tgt"][src]) - (p[dst] - p[src])
        gcl = torch.linalg.vector_norm(d, dim=1).mean()
        (grad,) = torch.autograd.grad(l1 + gcl, p)
        return [l1.detach().reshape(1), gcl.detach().reshape(1), grad]
    gen = _gen("loss", n)
    mid, last = graph_rows(ei, n)
    add(f"loss-n{n}", {"pred": _rand(gen, n, 3), "tgt": _rand(gen, n, 3)}, ref, run,
        {"first": ("pred", (0, 0)), "mid": ("pred", (mid, 1)), "lastrow": ("pred", (last, 2))})


_loss_case(67)
_loss_case(259)


def _adam_case(n=1027):
    lr, b1, b2, eps = 4e-4, 0.9, 0.999, 1e-8

    def run(t):
        from deformcontact_amd import _lib
        p, g, m, v = (t[k].clone() for k in ("p", "g", "m", "v"))
        step = torch.zeros(34, dtype=torch.float32, device=DEV)
        _lib.check(_lib.lib().dc_adam_flat(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, step.data_ptr(), lr,
                                           b1, b2, eps, 0, _st()), "adam")
        return [p, m, v]

    def ref(t):
        m = b1 * t["m"] + (1 - b1) * t["g"]
        v = b2 * t["v"] + (1 - b2) * t["g"] * t["g"]
        p = t["p"] - lr * (m / (1 - b1)) / ((v / (1 - b2)).sqrt() + eps)
        return [p, m, v]
    gen = _gen("adam")
    add("adam-n1027", {"p": _rand(gen, n), "g": _rand(gen, n), "m": _rand(gen, n, scale=0.1),
                       "v": torch.rand(n, generator=gen) * 0.01 + 1e-4}, ref, run,
        {"first": ("g", (0,)), "mid": ("g", (513,)), "last": ("g", (n - 1,))})


_adam_case()


# ---- layers end to end: a NaN in one input feature reaches the layer output exactly on R ------------------------------
def _layer_case(cid, n, fi, make_gpu, ref, params, f_out_note=""):
    ei = GRAPHS[n]

    def run(t):
        from deformcontact_amd.deferred import resolve
        from deformcontact_amd.graph import clear_cache
        clear_cache()                                      # no hop slab cached for another input at a reused address
        with torch.no_grad():
            return [resolve(make_gpu(t)(t["x"], torch.from_numpy(ei).to(DEV))).clone()]
    gen = _gen("layer", cid)
    inp = {"x": _rand(gen, n, fi)}
    inp.update(params(gen))
    add(cid, inp, ref(ei), run, _x_targets(ei, n, fi), poisons=("nan",))


def _tag_ref(ei, n, k, names):
    _, w = gcn_weights(ei, n)

    def layer(t, x, p):
        out, h = x @ t[f"{p}w"][0].t(), x
        for j in range(1, k + 1):
            h = ref_spmm(ei, w, h)
            out = out + h @ t[f"{p}w"][j].t()
        return out + t[f"{p}b"]
    return layer


def _tag2_case(n, fi, fh, fo, k=2):
    """TAGConv(K = 2, relu=True) then a second TAGConv: the deferred / fused ReLU and the slab hand-off"""
    def make(t):
        import deformcontact_amd as dc

        def fwd(x, ei):
            convs = [dc.nn.TAGConv(fi, fh, K=k).to(DEV), dc.nn.TAGConv(fh, fo, K=k).to(DEV)]
            for conv, p in zip(convs, ("1", "2")):
                for j in range(k + 1):
                    conv.lins[j].weight.data.copy_(t[f"{p}w"][j])
                conv.bias.data.copy_(t[f"{p}b"])
            return convs[1](convs[0](x, ei, relu=True, next_conv=convs[1]), ei)
        return fwd

    def ref(ei):
        layer = _tag_ref(ei, n, k, None)
        return lambda t: [layer(t, layer(t, t["x"], "1").clamp_min(0), "2")]

    def params(gen):
        return {"1w": _rand(gen, k + 1, fh, fi, scale=fi ** -0.5), "1b": _rand(gen, fh, scale=0.5),
                "2w": _rand(gen, k + 1, fo, fh, scale=fh ** -0.5), "2b": _rand(gen, fo, scale=0.5)}
    _layer_case(f"layer-tag2-n{n}-{fi}-{fh}-{fo}", n, fi, make, ref, params)


_tag2_case(67, 21, 256, 256)
_tag2_case(259, 32, 64, 16)


def _tag_deferred_case(n, fi, fo, k=2):
    """``F.relu(conv(x, edge_index))`` as the reference writes it: the deferred result runs the layer with the ReLU fused"""
    def make(t):
        import deformcontact_amd as dc
        import torch.nn.functional as F

        def fwd(x, ei):
            conv = dc.nn.TAGConv(fi, fo, K=k).to(DEV)
            for j in range(k + 1):
                conv.lins[j].weight.data.copy_(t["1w"][j])
            conv.bias.data.copy_(t["1b"])
            return F.relu(conv(x, ei))
        return fwd

    def ref(ei):
        layer = _tag_ref(ei, n, k, None)
        return lambda t: [layer(t, t["x"], "1").clamp_min(0)]
    _layer_case(f"layer-tag-deferred-n{n}-{fi}-{fo}", n, fi, make, ref,
                lambda gen: {"1w": _rand(gen, k + 1, fo, fi, scale=fi ** -0.5), "1b": _rand(gen, fo, scale=0.5)})


_tag_deferred_case(67, 256, 256)
_tag_deferred_case(259, 25, 256)


def _gcn_case(n, fi, fo):
    def make(t):
        import deformcontact_amd as dc

        def fwd(x, ei):
            conv = dc.nn.GCNConv(fi, fo).to(DEV)
            conv.lin.weight.data.copy_(t["w"])
            conv.bias.data.copy_(t["b"])
            return conv(x, ei, relu=True)
        return fwd

    def ref(ei):
        ei_l, w = gcn_weights(ei, n, loops=True)
        return lambda t: [(ref_spmm(ei_l, w, t["x"] @ t["w"].t()) + t["b"]).clamp_min(0)]
    _layer_case(f"layer-gcn-n{n}-{fi}-{fo}", n, fi, make, ref,
                lambda gen: {"w": _rand(gen, fo, fi, scale=fi ** -0.5), "b": _rand(gen, fo, scale=0.5)})


_gcn_case(67, 21, 64)
_gcn_case(259, 32, 256)


def _sage_layer_case(n, fi, fo):
    def make(t):
        import deformcontact_amd as dc

        def fwd(x, ei):
            conv = dc.nn.SAGEConv(fi, fo, aggr="max").to(DEV)
            conv.lin_l.weight.data.copy_(t["wl"])
            conv.lin_l.bias.data.copy_(t["b"])
            conv.lin_r.weight.data.copy_(t["wr"])
            return conv(x, ei)
        return fwd

    def ref(ei):
        src, dst = torch.from_numpy(ei[0]), torch.from_numpy(ei[1])
        return lambda t: [ref_amax(dst, t["x"][src], n) @ t["wl"].t() + t["b"] + t["x"] @ t["wr"].t()]
    _layer_case(f"layer-sage-max-n{n}-{fi}-{fo}", n, fi, make, ref,
                lambda gen: {"wl": _rand(gen, fo, fi, scale=fi ** -0.5), "wr": _rand(gen, fo, fi, scale=fi ** -0.5),
                             "b": _rand(gen, fo, scale=0.5)})


_sage_layer_case(67, 21, 64)
_sage_layer_case(259, 32, 32)


def _edgeconv_case(n, fi, fo):
    def make(t):
        import deformcontact_amd as dc

        def fwd(x, ei):
            lin = torch.nn.Linear(2 * fi, fo).to(DEV)
            lin.weight.data.copy_(t["w"])
            lin.bias.data.copy_(t["b"])
            return dc.nn.EdgeConv(lin, aggr="max")(x, ei)
        return fwd

    def ref(ei):
        src, dst = torch.from_numpy(ei[0]), torch.from_numpy(ei[1])
        return lambda t: [ref_amax(dst, torch.cat([t["x"][dst], t["x"][src] - t["x"][dst]], dim=1) @ t["w"].t() + t["b"], n)]
    _layer_case(f"layer-edgeconv-max-n{n}-{fi}-{fo}", n, fi, make, ref,
                lambda gen: {"w": _rand(gen, fo, 2 * fi, scale=fi ** -0.5), "b": _rand(gen, fo, scale=0.5)})


_edgeconv_case(67, 3, 64)
_edgeconv_case(259, 16, 32)


def _gmm_case(n, m, relu, reduce):
    """gmm_aggregate: finite pseudo-coordinates, the poison in h (and in the root term ``base``)"""
    ei, k, d = GRAPHS[n], 3, 2
    g, src, dst = _raw_graph(ei, n), torch.from_numpy(ei[0]), torch.from_numpy(ei[1])
    deg = torch.bincount(dst, minlength=n).clamp(min=1).double().unsqueeze(1)

    def run(t):
        from deformcontact_amd import ops
        return [ops.gmm_aggregate(g(), t["x"], t["e"], t["mu"], t["sigma"], reduce, base=t["base"], relu=bool(relu))]

    def ref(t):
        w = torch.exp((-0.5 * (t["e"].unsqueeze(1) - t["mu"]) ** 2 / (1e-15 + t["sigma"] ** 2)).sum(-1))      # [E, K]
        msg = sum(w[:, j:j + 1] * t["x"][src, j * m:(j + 1) * m] for j in range(k))
        s = torch.zeros(n, m, dtype=torch.float64).index_add_(0, dst, msg)
        s = (s / deg if reduce == "mean" else s) + t["base"]
        return [s.clamp_min(0) if relu else s]
    gen = _gen("gmm", n, m)
    inp = {"x": _rand(gen, n, k * m), "e": torch.rand(ei.shape[1], d, generator=gen), "mu": torch.rand(k, d, generator=gen),
           "sigma": torch.rand(k, d, generator=gen) + 0.5, "base": _rand(gen, n, m)}
    tg = _x_targets(ei, n, k * m)
    tg["base"] = ("base", (graph_rows(ei, n)[0], m - 1))
    add(f"seg-gmm-{reduce}-n{n}-m{m}-relu{relu}", inp, ref, run, tg)


for n, m, relu, reduce in [(67, 3, 0, "mean"), (259, 32, 1, "mean"), (67, 256, 1, "add"), (259, 32, 0, "add")]:
    _gmm_case(n, m, relu, reduce)


def _spline_case(n, m, relu, reduce):
    """spline_aggregate: finite pseudo-coordinates (the basis selects indices: only h and the root term are poisoned);
    the basis and the block indices are the float32 restatement ``helpers.linear_spline_basis``"""
    ei, degree = GRAPHS[n], 1
    ks, op = (3, 4), (1, 0)
    k = ks[0] * ks[1]
    g, src, dst = _raw_graph(ei, n), torch.from_numpy(ei[0]), torch.from_numpy(ei[1])
    deg = torch.bincount(dst, minlength=n).clamp(min=1).double().unsqueeze(1)
    gen = _gen("spline", n, m)
    e = torch.rand(ei.shape[1], 2, generator=gen) * 0.98 + 0.01
    b32, wi = linear_spline_basis(e.numpy(), ks, op)
    b, wi = torch.from_numpy(b32).double(), torch.from_numpy(wi)
    cols = torch.arange(m)

    def run(t):
        from deformcontact_amd import ops
        return [ops.spline_aggregate(g(), t["x"], e.to(DEV), list(ks), [bool(o) for o in op], degree, reduce, base=t["base"],
                                     relu=bool(relu))]

    def ref(t):
        msg = sum(b[:, s:s + 1] * t["x"][src.unsqueeze(1), wi[:, s:s + 1] * m + cols] for s in range(b.size(1)))
        out = torch.zeros(n, m, dtype=torch.float64).index_add_(0, dst, msg)
        out = (out / deg if reduce == "mean" else out) + t["base"]
        return [out.clamp_min(0) if relu else out]
    tg = {}
    mid, last = graph_rows(ei, n)
    for pid, r, c in (("first", 0, 0), ("mid", mid, m // 2), ("lastrow", last, min(1, m - 1)), ("lastcol", mid // 2, m - 1)):
        out_edges = np.nonzero(ei[0] == r)[0]
        if len(out_edges):                                 # a column block that an edge out of r selects
            tg[pid] = ("x", (r, int(wi[out_edges[-1], -1]) * m + c))
    tg["base"] = ("base", (mid, m - 1))
    add(f"seg-spline-{reduce}-n{n}-m{m}-relu{relu}", {"x": _rand(gen, n, k * m), "base": _rand(gen, n, m)}, ref, run, tg)


for n, m, relu, reduce in [(67, 3, 0, "mean"), (259, 32, 1, "mean"), (67, 256, 1, "add")]:
    _spline_case(n, m, relu, reduce)


def _cheb_case(n, f, k=3, lam=3.0):
    """the Chebyshev recurrence hop: Tx_0 = x, Tx_1 = L^ x, Tx_k = 2 L^ Tx_{k-1} - Tx_{k-2}; L^ x_i = sum_{j->i} wl x_j + b x_i,
    wl = (2 * -w) / lambda_max, w = deg_j^-1/2 deg_i^-1/2 by out-degree over the non-loop edges, b = 2 / lambda_max - 1"""
    ei = GRAPHS[n]
    g = _raw_graph(ei, n)
    noloop = ei[:, ei[0] != ei[1]]
    deg = np.bincount(noloop[0], minlength=n).astype(np.float64)
    dis = np.where(deg > 0, np.maximum(deg, 1.0) ** -0.5, 0.0)
    wl = torch.from_numpy(2.0 * -(dis[noloop[0]] * dis[noloop[1]]) / lam)
    b = 2.0 / lam - 1.0

    def run(t):
        from deformcontact_amd import ops
        with torch.no_grad():
            return [ops.cheb_basis(g(), t["x"], k, "sym", lam)]

    def ref(t):
        lap = lambda h: ref_spmm(noloop, wl, h) + b * h
        tx = [t["x"], lap(t["x"])]
        for _ in range(2, k):
            tx.append(2 * lap(tx[-1]) - tx[-2])
        return [torch.cat(tx[:k], dim=1)]
    add(f"seg-cheb-n{n}-f{f}", {"x": _rand(_gen("cheb", n, f), n, f)}, ref, run, _x_targets(ei, n, f))


for n, f in [(67, 3), (259, 32), (67, 256)]:
    _cheb_case(n, f)


# ---- edge softmax: GATConv's aggregation, one head and several --------------------------------------------------------
def _gat_case(n, nh, c, slope=0.2):
    """softmax over the in-edges of i (self loops removed, then one added per node) of leaky_relu(a_src[j] + a_dst[i]) per
    head, out[i] = sum_j alpha_ij h[j]; the poison in one source feature, then in one logit term"""
    ei = GRAPHS[n]
    keep = ei[0] != ei[1]
    ei_l = np.concatenate([ei[:, keep], np.stack([np.arange(n), np.arange(n)])], axis=1)
    src, dst = torch.from_numpy(ei_l[0]), torch.from_numpy(ei_l[1])
    g = _lazy(lambda: _graph(ei, n, self_loops=True, normalize=False))

    def run(t):
        from deformcontact_amd import ops
        if nh == 1:
            return [ops.gat_aggregate(g(), t["x"], t["a_src"][:, 0].contiguous(), t["a_dst"][:, 0].contiguous(), slope)]
        return [ops.gat_heads_aggregate(g(), t["x"], t["a_src"], t["a_dst"], slope, nh)]

    def ref(t):
        logit = torch.nn.functional.leaky_relu(t["a_src"][src] + t["a_dst"][dst], slope)
        alpha = ref_segment_softmax(logit, dst, n)                                     # [E, H]
        msg = (alpha.unsqueeze(2) * t["x"][src].view(-1, nh, c)).reshape(-1, nh * c)
        return [torch.zeros(n, nh * c, dtype=torch.float64).index_add_(0, dst, msg)]
    gen = _gen("gat", n, nh, c)
    mid, last = graph_rows(ei, n)
    tg = _x_targets(ei, n, nh * c)
    tg.update({"a_src_first": ("a_src", (0, 0)), "a_src_mid": ("a_src", (mid, nh - 1)), "a_dst_mid": ("a_dst", (mid, 0)),
               "a_dst_last": ("a_dst", (last, nh - 1))})
    add(f"softmax-gat-n{n}-h{nh}-c{c}", {"x": _rand(gen, n, nh * c), "a_src": _rand(gen, n, nh), "a_dst": _rand(gen, n, nh)},
        ref, run, tg)


for n, nh, c in [(67, 1, 8), (259, 1, 64), (67, 3, 8), (259, 3, 64)]:
    _gat_case(n, nh, c)


def _loops(ei, n):
    keep = ei[0] != ei[1]
    return np.concatenate([ei[:, keep], np.stack([np.arange(n), np.arange(n)])], axis=1)


def _attend(logit, dst, vals, n, nh, c):
    """out[i] = sum over the in-edges of i of softmax_i(logit)[e, h] vals[e, h, :]"""
    alpha = ref_segment_softmax(logit, dst, n)
    msg = (alpha.unsqueeze(2) * vals.view(-1, nh, c)).reshape(-1, nh * c)
    return torch.zeros(n, nh * c, dtype=torch.float64).index_add_(0, dst, msg)


def _add_with_params(cid, inp, ref, run, ei, n, nh, c, names):
    """two cases: a source feature at the node placements (its reach set is rows of out-neighbours: containment holds at
    every H), and one attention parameter per name, which reaches its whole head in every row - with one head that is
    everything, and only rule 1 says something"""
    add(cid, inp, ref, run, _x_targets(ei, n, nh * c))
    add(cid + "-param", inp, ref, run, {name: (name, (0, nh - 1, c // 2)) for name in names}, contain=nh > 1)


def _gat_conv_case(n, nh, c, slope=0.2):
    """gat_heads_conv / gat_conv: the whole GATConv layer behind ``lin`` with bias and the fused ReLU"""
    ei = GRAPHS[n]
    ei_l = _loops(ei, n)
    src, dst = torch.from_numpy(ei_l[0]), torch.from_numpy(ei_l[1])
    g = _lazy(lambda: _graph(ei, n, self_loops=True, normalize=False))

    def run(t):
        from deformcontact_amd import ops
        with torch.no_grad():
            assert ops.gat_heads_fused_ok(t["x"], nh, False)
            if nh == 1:
                return [ops.gat_conv(g(), t["x"], t["att_src"], t["att_dst"], t["b"], slope, relu=True)]
            return [ops.gat_heads_conv(g(), t["x"], t["att_src"], t["att_dst"], t["b"], slope, relu=True, heads=nh)]

    def ref(t):
        h = t["x"].view(n, nh, c)
        a_s, a_d = (h * t["att_src"]).sum(-1), (h * t["att_dst"]).sum(-1)
        logit = torch.nn.functional.leaky_relu(a_s[src] + a_d[dst], slope)
        return [(_attend(logit, dst, t["x"][src], n, nh, c) + t["b"]).clamp_min(0)]
    gen = _gen("gatconv", n, nh, c)
    _add_with_params(f"softmax-gat_conv-n{n}-h{nh}-c{c}",
                     {"x": _rand(gen, n, nh * c), "att_src": _rand(gen, 1, nh, c), "att_dst": _rand(gen, 1, nh, c),
                      "b": _rand(gen, nh * c, scale=0.5)}, ref, run, ei, n, nh, c, ("att_src", "att_dst"))


def _gatv2_case(n, nh, c, fused, slope=0.2):
    ei = GRAPHS[n]
    ei_l = _loops(ei, n)
    src, dst = torch.from_numpy(ei_l[0]), torch.from_numpy(ei_l[1])
    g = _lazy(lambda: _graph(ei, n, self_loops=True, normalize=False))

    def run(t):
        from deformcontact_amd import ops
        with torch.no_grad():
            return [ops.gatv2_conv(g(), t["x"], t["xr"], t["att"], t["b"] if fused else None, slope, relu=fused, heads=nh)]

    def ref(t):
        s = torch.nn.functional.leaky_relu(t["x"][src].view(-1, nh, c) + t["xr"][dst].view(-1, nh, c), slope)
        out = _attend((s * t["att"]).sum(-1), dst, t["x"][src], n, nh, c)
        return [(out + t["b"]).clamp_min(0) if fused else out]
    gen = _gen("gatv2", n, nh, c)
    _add_with_params(f"softmax-gatv2-n{n}-h{nh}-c{c}-fused{int(fused)}",
                     {"x": _rand(gen, n, nh * c), "xr": _rand(gen, n, nh * c), "att": _rand(gen, 1, nh, c),
                      "b": _rand(gen, nh * c, scale=0.5)}, ref, run, ei, n, nh, c, ("att",))


def _tconv_case(n, nh, c, fused):
    """TransformerConv's attention on the edge set as it is given: a row without in-edges is 0 (+ bias)"""
    ei = GRAPHS[n]
    src, dst = torch.from_numpy(ei[0]), torch.from_numpy(ei[1])
    g = _raw_graph(ei, n)

    def run(t):
        from deformcontact_amd import ops
        with torch.no_grad():
            return [ops.transformer_conv(g(), t["q"], t["x"], t["v"], t["b"] if fused else None, relu=fused, heads=nh)]

    def ref(t):
        logit = (t["q"][dst].view(-1, nh, c) * t["x"][src].view(-1, nh, c)).sum(-1) / c ** 0.5
        out = _attend(logit, dst, t["v"][src], n, nh, c)
        return [(out + t["b"]).clamp_min(0) if fused else out]
    gen = _gen("tconv", n, nh, c)
    tg = _x_targets(ei, n, nh * c)                         # "x" is the key: a source feature
    mid, _ = graph_rows(ei, n)
    tg.update({"v_mid": ("v", (mid, nh * c - 1)), "q_mid": ("q", (mid, 0)), "q_first": ("q", (0, 0))})
    add(f"softmax-transformer-n{n}-h{nh}-c{c}-fused{int(fused)}",
        {"x": _rand(gen, n, nh * c), "q": _rand(gen, n, nh * c), "v": _rand(gen, n, nh * c), "b": _rand(gen, nh * c, scale=0.5)},
        ref, run, tg)


# (with bias / ReLU the fused row passes take H*C / 4 dividing 256: H = 3 runs as the bare aggregation)
for n, nh, c in [(67, 1, 8), (259, 1, 64), (67, 2, 8), (259, 2, 64)]:
    _gat_conv_case(n, nh, c)
for n, nh, c, fused in [(67, 1, 8, True), (259, 3, 64, False), (67, 3, 8, False), (259, 2, 64, True)]:
    _gatv2_case(n, nh, c, fused)
    _tconv_case(n, nh, c, fused)


def _gat_edge_case(n, nh, c, d=3, slope=0.2):
    """the multi-head aggregation with edge features: logit = leaky_relu(a_src[j] + a_dst[i] + (edge_attr @ M)[e, h]); the
    appended self loop of i carries the mean attribute of the non-loop edges into i (fill_value="mean")"""
    ei = GRAPHS[n]
    keep = np.nonzero(ei[0] != ei[1])[0]
    ei_l = _loops(ei, n)
    src, dst = torch.from_numpy(ei_l[0]), torch.from_numpy(ei_l[1])
    kdst = torch.from_numpy(ei[1][keep])
    cnt = torch.bincount(kdst, minlength=n).clamp(min=1).double().unsqueeze(1)
    g = _lazy(lambda: _graph(ei, n, self_loops=True, normalize=False))

    def run(t):
        from deformcontact_amd import ops
        with torch.no_grad():
            return [ops.gat_heads_aggregate(g(), t["x"], t["a_src"], t["a_dst"], slope, nh, edge_attr=t["e"], edge_m=t["m"],
                                            fill_value="mean")]

    def ref(t):
        ea = t["e"][torch.from_numpy(keep)]
        loop = torch.zeros(n, d, dtype=torch.float64).index_add_(0, kdst, ea) / cnt
        logit = torch.nn.functional.leaky_relu(t["a_src"][src] + t["a_dst"][dst] + torch.cat([ea, loop]) @ t["m"], slope)
        return [_attend(logit, dst, t["x"][src], n, nh, c)]
    gen = _gen("gatedge", n, nh, c)
    tg = _x_targets(ei, n, nh * c)
    for pid, (e, _) in edge_placements(ei, d).items():
        e = e if ei[0][e] != ei[1][e] else int(keep[0])        # (an input self loop takes no part: not a placement)
        tg["e_" + pid] = ("e", (e, d - 1))
    tg["m"] = ("m", (0, nh - 1))                               # one folded attention parameter: its whole head, every row
    add(f"softmax-gat_edge-n{n}-h{nh}-c{c}", {"x": _rand(gen, n, nh * c), "a_src": _rand(gen, n, nh), "a_dst": _rand(gen, n, nh),
                                              "e": _rand(gen, ei.shape[1], d), "m": _rand(gen, d, nh)}, ref, run, tg,
        contain=True)


for n, nh, c in [(67, 3, 8), (259, 3, 64)]:
    _gat_edge_case(n, nh, c)


# ---- attention -------------------------------------------------------------------------------------------------------------
def _attn_ref(t):
    return torch.softmax(t["q"] @ t["k"].t(), dim=-1) @ t["v"]


def _attn_inputs(ns, nr, d):
    gen = _gen("attn", ns, nr, d)
    return {"q": _rand(gen, ns, d, scale=d ** -0.5), "k": _rand(gen, nr, d), "v": _rand(gen, nr, d), "go": _rand(gen, ns, d)}


def _attn_fwd_case(ns, nr, d, env, tag):
    def run(t):
        from deformcontact_amd.attention import attention_core
        with torch.no_grad():
            return [attention_core(t["q"], t["k"], t["v"])]
    inp = _attn_inputs(ns, nr, d)
    del inp["go"]
    # a q row reaches its own output row; one v element its output column; one k element every score of its key
    add(f"attn-fwd-{tag}-{ns}x{nr}-d{d}", inp, lambda t: [_attn_ref(t)], run,
        {"q_row": ("q", (ns // 2,)), "q_first": ("q", (0, 0)), "q_lastrow": ("q", (ns - 1, d - 1)),
         "v_first": ("v", (0, 0)), "v_last": ("v", (nr - 1, d - 1))}, env=env)
    add(f"attn-fwd-k-{tag}-{ns}x{nr}-d{d}", inp, lambda t: [_attn_ref(t)], run,
        {"k_first": ("k", (0, 0)), "k_last": ("k", (nr - 1, d // 2))}, contain=False, env=env)


def _attn_bwd_case(ns, nr, d, env, tag):
    def run(t):
        from deformcontact_amd.attention import attention_core
        q, k, v = (t[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
        return list(torch.autograd.grad(attention_core(q, k, v), (q, k, v), t["go"]))

    def ref(t):
        q, k, v = (t[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
        return list(torch.autograd.grad(_attn_ref({"q": q, "k": k, "v": v}), (q, k, v), t["go"]))
    # a row of go reaches its own row of dq, and all of dk and dv
    add(f"attn-bwd-{tag}-{ns}x{nr}-d{d}", _attn_inputs(ns, nr, d), ref, run,
        {"go_row": ("go", (ns // 2,)), "go_first": ("go", (0,)), "go_last": ("go", (ns - 1,))}, env=env)


for ns, nr in [(131, 70), (33, 64)]:
    _attn_fwd_case(ns, nr, 256, {}, "flash")
    _attn_fwd_case(ns, nr, 32, {}, "blocked")
    _attn_bwd_case(ns, nr, 256, {}, "flash_single")
    _attn_bwd_case(ns, nr, 256, {"FLASH_BWD_SINGLE": False}, "flash_two_sweeps")
    _attn_bwd_case(ns, nr, 256, {"FLASH_BWD": False}, "blocked_bwd")
    _attn_bwd_case(ns, nr, 32, {}, "blocked")


def _grouped_case(fo=128, k=1, relu=1):
    """ops.tag_conv_grouped: the same TAGConv layer of two branches over a merged (block-diagonal) adjacency in grouped
    launches; a poison in part 0 leaves part 1 bit-identical (its reach set lies in part 0's output)"""
    parts, fi = [(GRAPHS[67], 67), (GRAPHS[259], 259)], 256
    mg = _lazy(lambda: __import__("deformcontact_amd").graph.GraphIndex.from_parts(
        [(torch.from_numpy(e).to(DEV), m) for e, m in parts]))

    def run(t):
        from deformcontact_amd import ops
        assert ops.grouped_eligible(fi, fo, k)
        with torch.no_grad():
            outs = ops.tag_conv_grouped(mg(), [t["x0"], t["x1"]], [[t["w"][g][j] for j in range(k + 1)] for g in range(2)],
                                        [t["b"][g] for g in range(2)], relu=bool(relu))
        return [o.clone() for o in outs]

    def ref(t):
        outs = []
        for g, (ei, n) in enumerate(parts):
            w = gcn_weights(ei, n)[1]
            h = t[f"x{g}"]
            out = h @ t["w"][g][0].t()
            for j in range(1, k + 1):
                h = ref_spmm(ei, w, h)
                out = out + h @ t["w"][g][j].t()
            out = out + t["b"][g]
            outs.append(out.clamp_min(0) if relu else out)
        return outs
    gen = _gen("grouped", fo, k)
    inp = {"x0": _rand(gen, 67, fi), "x1": _rand(gen, 259, fi), "w": _rand(gen, 2, k + 1, fo, fi, scale=fi ** -0.5),
           "b": _rand(gen, 2, fo, scale=0.5)}
    tg = {"p0_" + p: ("x0", v) for p, v in element_placements(GRAPHS[67], 67, fi).items()}
    tg.update({"p1_" + p: ("x1", v) for p, v in element_placements(GRAPHS[259], 259, fi).items()})
    add(f"dense-grouped-fo{fo}-k{k}-relu{relu}", inp, ref, run, tg)


_grouped_case()


def _encoder_case():
    """the two-layer TAGConv encoder of graphnet.py (both branches, ReLU fused, slab hand-off between the layers) on the
    h32 golden graphs: a NaN in one feature of the resting graph reaches its own branch exactly on R, the other not at all"""
    z = load_golden("graphnet_tag_h32.npz")
    eis = {"rest": z["rest_edge_index"], "rig": z["rig_edge_index"]}
    x, xr = torch.from_numpy(z["rest_x"]), torch.from_numpy(z["rig_x"])
    hidden = int(z["hidden"])

    @_lazy
    def models():
        from deformcontact_amd.graphnet import ContactEncoder
        from oracle import pyg_ref
        torch.manual_seed(11)
        enc = ContactEncoder([x.size(1), xr.size(1)], hidden)
        ref = ContactEncoder([x.size(1), xr.size(1)], hidden, conv_module=pyg_ref)
        ref.load_state_dict(enc.state_dict())
        return enc, ref.double()

    def batch(a, b, dev):
        from tests.helpers import G
        return (G(a, torch.from_numpy(eis["rest"]).to(dev), torch.from_numpy(z["rest_pos"]).to(dev)),
                G(b, torch.from_numpy(eis["rig"]).to(dev), torch.from_numpy(z["rig_pos"]).to(dev)))

    def run(t):
        from deformcontact_amd.deferred import resolve
        from deformcontact_amd.graph import clear_cache
        clear_cache()
        with torch.no_grad():
            a, b = models()[0].to(DEV)(*batch(t["x"], t["xr"], DEV))
            return [resolve(a).clone(), resolve(b).clone()]

    def ref(t):
        with torch.no_grad():
            a, b = models()[1](*batch(t["x"], t["xr"], "cpu"))
        return [a, b]
    add("layer-encoder-h32", {"x": x, "xr": xr}, ref, run, _x_targets(eis["rest"], x.size(0), x.size(1)), poisons=("nan",))


_encoder_case()


# --------------------------------------------------------------------------- #
# the tests
# --------------------------------------------------------------------------- #
PARAMS = [(cid, pid) for cid, c in CASES.items() for pid in c.targets]


def test_references_propagate_and_reach_sets_are_proper():
    """The float64 restatements themselves (no GPU): NaN through ReLU stays NaN, NaN through amax propagates, a NaN
    logit makes its whole segment NaN and no other; and in EVERY case both the reach set and its complement are
    non-empty, so that neither rule 1 nor rule 2 can pass vacuously."""
    t = torch.tensor([NAN, -1.0, 2.0], dtype=torch.float64)
    assert torch.isnan(t.clamp_min(0)[0]) and t.clamp_min(0)[1:].tolist() == [0.0, 2.0]
    idx = torch.tensor([0, 0, 1, 1, 3])
    rows = torch.tensor([[1.0], [NAN], [2.0], [float("-inf")], [float("-inf")]], dtype=torch.float64)
    m = ref_amax(idx, rows, 4)
    assert torch.isnan(m[0, 0]) and m[1:, 0].tolist() == [2.0, 0.0, float("-inf")]     # row 2 has no candidate: 0
    sm = ref_segment_softmax(rows.clone().fill_(1.0).index_put_((torch.tensor([1]),), torch.tensor(NAN, dtype=torch.float64)),
                             idx, 4)
    assert torch.isnan(sm[:2]).all() and torch.isfinite(sm[2:]).all()
    for cid, pid in PARAMS:
        c = CASES[cid]
        clean = c.ref(c.inputs64())
        assert all(bool(torch.isfinite(o).all()) for o in clean), f"{cid}: the clean restatement is not finite"
        reach = c.reach(pid)
        assert len(reach) == len(clean)
        assert any(bool(r.any()) for r in reach), f"{cid}[{pid}]: empty reach set"
        if c.contain:
            assert any(not bool(r.all()) for r in reach), f"{cid}[{pid}]: the reach set is everything"
        for r, o in zip(reach, clean):
            assert r.shape == o.shape


@gpu
@pytest.mark.parametrize("cid,pid", PARAMS, ids=[f"{c}[{p}]" for c, p in PARAMS])
def test_nonfinite(cid, pid, monkeypatch):
    c = CASES[cid]
    for k, v in c.env.items():                                 # the switches of attention.py (read at call time)
        from deformcontact_amd import attention
        monkeypatch.setattr(attention, k, v)
    name, index = c.targets[pid]
    keep = []                                                  # every input stays alive: no address is reused in a case
    dev = {k: v.to(DEV) for k, v in c.inputs.items()}
    keep.append(dev)
    clean = c.run(dev)
    for j, o in enumerate(clean):
        assert bool(torch.isfinite(o.float()).all()), f"{cid}: clean output {j} is not finite"
    reach = c.reach(pid)
    assert len(reach) == len(clean)
    for pname, value in POISONS:
        if pname not in c.poisons:
            continue
        bad = poisoned(dev, name, index, value)
        keep.append(bad)
        out = c.run(bad)
        must = c.reach(pid, pname)
        ref = c.ref(poisoned(c.inputs64(), name, index, value)) if c.selection and pname != "nan" else None
        for j, o in enumerate(out):
            what = f"{cid}[{pid}] {pname} output {j}"
            assert_not_swallowed(o, must[j], what)
            if c.contain:
                assert_contained(o, clean[j], reach[j], what)
            if ref is not None:
                assert_selection(o, ref[j], what)
