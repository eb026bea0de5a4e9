"""Guard bands: what the kernels do AROUND their tensors ("Memory contract").

Every other file of the suite looks inside the tensors a kernel is meant to produce.  Here every buffer a case allocates
(``tests.helpers.Guard``: the Python-level factories are intercepted for device tensors; so is ``clone``, whose copy
counts as a guarded output only where its source lay in a guarded allocation) and every input
sits between two bands of one full 128-row tile (at least 4 KiB) of NaN / 1, and four rules hold, none with a tolerance:

  0. two plain runs give the same bits (the library documents run-to-run bit identity);
  1. no write outside: all bands and gap columns of all buffers allocated during the call, and of the inputs, keep
     their fill;
  2. inputs are read-only: the interior of every hosted input keeps its bits (exceptions are the operands
     INTEGRATION.md documents as written in place; each is named in its case);
  3. slack independence: with NaN next to every float input and a valid index (0, then N - 1) next to every index
     input, the outputs equal the plain run bit for bit - an over-read is allowed, an effect on an output bit is not;
  4. no reliance on initial contents: the same outputs with every ``empty`` interior dirty (NaN, 1, the float32 NaN
     pattern in byte workspaces).

The guarded run must launch the kernels the plain run launched (``_lib.kernel_trace_counts``), or rules 3 and 4 would
compare different code: bands are multiples of 512 bytes, so the interior keeps the alignment class of a fresh
allocation.

Cases: (a) every entry of ``tests/test_nonfinite.py:CASES`` on its clean inputs; (b) the launch-site rows of
``tests/test_launch_sites.py`` (tail-heavy by construction); (c) the operations that form addresses from their input
(graph builds, kNN / radius, fps, knn_interpolate, the feature-space kNN, the Morton order, the spline basis, the
pools), their plain outputs also compared with the suite's CPU restatements; (d) outputs with a leading dimension
through the C ABI (``ld = cols + 4`` and ``cols + 1``), the gap columns holding the sentinel.

The (b) runners build their operands themselves: the dense rows get NaN slack and watched operands (rules 2 and 3), but
their outputs are ``torch.full(NaN)`` in every run, so rule 4 is blind there and is carried by (d); the chain, bf16-hop,
pack and Morton rows host no input and serve rules 1 and 4 and the dispatch check.

The CPU tests plant one error of each kind in a Python "kernel" and require that exactly its rule trips.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

from tests import test_launch_sites as tls
from tests import test_nonfinite as nf
from tests.helpers import Guard, guard_band_bytes, guard_rules, linear_spline_basis, strided_out

gpu = pytest.mark.gpu
DEV = "cuda:0"

#: byte workspaces that carry integers which form addresses are dirtied with the int32 value 1 per word, not with the
#: NaN pattern (a counter that wrongly assumes 0 then moves an index by one element, into a band).  One entry per
#: buffer, by the (file, function) that allocates it; every other byte workspace holds floats (split-K and dW partial
#: sums, column sums, fps' points and running minima) and gets the NaN pattern.
INTEGER_WORKSPACES = {
    ("graph.py", "__init__"): "GraphIndex._workspace: int32 counters, cursors, group lists and bucket starts of the CSR "
                              "build (csrc/dc_csr.hip)",
    ("graph.py", "morton"): "NodeOrder.morton: 64-bit sort keys (code << 32 | index) and radix histograms",
    ("neighbors.py", "_fill"): "dc_neighbors_fill: int32 cell counts, cell starts and the cell-sorted point order",
    ("neighbors.py", "_edges"): "dc_neighbors_compact: the scan of the counts (int64 offsets)",
    ("test_guard_bands.py", "_csr_workspace"): "the dc_csr_build workspace of the c:csr-build cases (as GraphIndex's)",
}

#: cases with an output outside every registered buffer: case id prefix -> (the function that produces that output,
#: "module:qualified name", the reason).  A copy made by ``clone`` counts as guarded only where its source was.  The
#: producer must be plain ATen code: the CPU test loads it and requires that it hands no pointer to the library, so no
#: entry can stand for the output of a kernel (training path or not); such an output is checked by calling the C entry
#: with test-owned outputs instead.  At most 15.
UNGUARDED = {
    "layer-sage-max-": ("deformcontact_amd.nn.conv:SAGEConv._layer",
                        "out = lin_l(agg) + lin_r(x): two torch.nn.Linear calls and an ATen add; the aggregation (dc_sage.hip) "
                        "writes its guarded buffer, which the d:layer-sage_* cases also check with test-owned outputs"),
    "loss-": ("deformcontact_amd.ops:_ContactLossFn.backward",
              "the gradient autograd returns is g1 * g_l1 + g2 * g_gcl, formed by ATen; what dc_contact_loss itself writes "
              "(g1, g2, the two loss values, its workspace) is allocated by torch.empty: guarded, and e:contact-loss-direct "
              "calls the entry with test-owned outputs"),
}
MAX_UNGUARDED = 15


class GCase:
    """``run``: dict of device tensors -> list of device outputs; ``inputs``: dict of CPU tensors, or a callable;
    ``index_inputs``: {name: largest valid index}; ``in_place``: {name: section of INTEGRATION.md}; ``reference``:
    callable(list of plain outputs on the CPU) that asserts them against a CPU restatement; ``partial``: (rows of an
    output, rows per tile) of an output whose last tile is partial, ``slack``: the name of an input with non-empty
    slack (both required of (c) and (d): the CPU vacuity test; the rows are checked against the outputs on the GPU);
    ``env``: switches of attention.py; ``setenv``: environment switches the library reads at call time."""

    def __init__(self, run, inputs, index_inputs=None, in_place=None, reference=None, partial=None, slack=None, env=None,
                 setenv=None):
        self.run, self._inputs, self.index_inputs, self.in_place = run, inputs, index_inputs or {}, in_place or {}
        self.reference, self.partial, self.slack, self.env, self.setenv = reference, partial, slack, env or {}, setenv or {}

    @property
    def inputs(self):
        return self._inputs() if callable(self._inputs) else self._inputs


GCASES = {}


def gadd(cid, *args, **kw):
    assert cid not in GCASES, cid
    GCASES[cid] = GCase(*args, **kw)


def _st():
    return nf._st()


# ---- (a) every case of tests/test_nonfinite.py on its clean inputs -------------------------------------------------------
for _cid, _c in nf.CASES.items():
    gadd("a:" + _cid, _c.run, (lambda c=_c: c.inputs), env=_c.env)


# ---- (b) the launch-site rows -------------------------------------------------------------------------------------------
def _nan_slack(d, off):
    """The operands of a ``_Dense`` are views into flat zero buffers ``[off | rows * ld | 4]``: under a guard, turn every
    element outside the views (the shift, the gap columns, the tail) into NaN and watch the whole buffers as inputs."""
    g = Guard.active
    if g is None:
        return
    for name, v in [("slab", d.slab), ("g", d.g), ("mask", d.maskt)] + [(f"w{s}", w) for s, w in enumerate(d.ws)]:
        rows, ld = v.size(0), v.stride(0)
        flat = torch.as_strided(v, (rows * ld + off + 4,), (1,), v.storage_offset() - off)
        keep = v.clone()
        flat.fill_(float("nan"))
        v.copy_(keep)
        g.watch(flat, name)


def _dense_row_run(what, n, fi, fo, nseg, kw):
    def run(t):
        k = dict(kw)
        off = k.pop("off", 0)
        d = tls._Dense(n, fi, fo, nseg, off=off, ldpad=k.pop("ldpad", 0))
        _nan_slack(d, off)
        products = k.pop("products", 0)
        if what == "fwd":
            tls._dense_fwd(d, k.pop("relu"), products)
        elif what == "dx":
            tls._dense_dx(d, k.pop("mask"), products)
        else:
            tls._dense_dw(d, k.pop("mask"), products, **k)
        return d.outputs
    return run


for _p in tls.DENSE_ROWS:
    _kernels, _what, _n, _fi, _fo, _nseg, _kw = _p.values
    gadd("b:dense-" + _p.id, _dense_row_run(_what, _n, _fi, _fo, _nseg, _kw), {})
# the same harness with widened leading dimensions (no row of the census has one): the gap columns are slack
for _what, _n, _fi, _fo, _nseg, _kw in [("fwd", 129, 16, 136, 2, dict(relu=True, ldpad=4)),
                                        ("fwd", 129, 5, 7, 2, dict(relu=True, ldpad=1)),
                                        ("dx", 129, 16, 32, 2, dict(mask=True, ldpad=4)),
                                        ("dx", 129, 5, 7, 2, dict(mask=True, ldpad=1)),
                                        ("dw", 129, 16, 128, 2, dict(mask=True, ldpad=4)),
                                        ("dw", 67, 5, 7, 2, dict(mask=True, ldpad=1))]:
    gadd(f"b:dense-{_what}-n{_n}-fi{_fi}-fo{_fo}-ldpad{_kw['ldpad']}", _dense_row_run(_what, _n, _fi, _fo, _nseg, _kw), {})


def _chain_row_run(kernel, big, weighted, gcn):
    def run(t):
        from deformcontact_amd.graph import GraphIndex
        from tests.test_hop_chain import batch_of_graphs, run_both
        ei, segs = batch_of_graphs((37, big, 130), (3, 5, 2), seed=big, hub=(1, 41))
        n = segs[0][-1]
        g = GraphIndex(ei.to(DEV), n, segments=segs)
        return [run_both(g, g.fwd, n, 32, 2, 1, weighted=weighted, gcn=gcn, seed=big)]
    return run


for _kernel, _big, _weighted, _gcn in tls.CHAIN_ROWS:
    gadd("b:chain-" + _kernel, _chain_row_run(_kernel, _big, _weighted, _gcn), {})
for _f, _kernel, _form in tls.BF16_HOP_ROWS:
    gadd(f"b:bf16-hop-f{_f}", (lambda t, a=(_f, _kernel, _form): list(tls._bf16_hop_run(*a)[3].values())), {})
for _fi, _l in tls.PACK_WPREP_ROWS:
    gadd(f"b:pack-wprep-fi{_fi}", (lambda t, a=(_fi, _l): (lambda r: [r[3], r[4]])(tls._pack_wprep_run(*a))), {})
gadd("b:morton-codes", lambda t: [tls._morton_codes_run()[3]], {})


# ---- (c) operations that form addresses from their input -----------------------------------------------------------------
SIZES = (67, 259, 1)
BATCH = (1, 67, 259)


def _points(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).random((n, 3), dtype=np.float32))


def _batch_graph():
    """the three graphs (1, 67, 259) as one block-diagonal edge_index with its layout"""
    eis, nptr, eptr = [], [0], [0]
    for n in BATCH:
        ei = nf.GRAPHS[n]
        eis.append(ei + nptr[-1])
        nptr.append(nptr[-1] + n), eptr.append(eptr[-1] + ei.shape[1])
    return np.concatenate(eis, axis=1), (tuple(nptr), tuple(eptr))


def _loops(ei, n):
    keep = ei[0] != ei[1]
    return np.concatenate([ei[:, keep], np.stack([np.arange(n), np.arange(n)])], axis=1)


#: DC_CSR_BUCKETS=1 (read by dc_csr.hip at every build) forces the bucketed pipeline - k_bk_count / k_bk_scan /
#: k_bk_scatter / k_bk_build / k_bk_weights, whose bucket starts rely on a memset - at sizes where the plan would pick
#: the windowed one; a shift of 5 gives 32-node buckets: several buckets, the last one ragged, at N = 67 and 259
BUCKETED = {"DC_CSR_BUCKETS": "1", "DC_CSR_BUCKET_SHIFT": "5"}


def _check_sides(out, ei, n, self_loops, normalize, cid, per):
    """both sorted sets against the stable argsort (tests/test_gpu_parity.py: _check_csr): ptr, other and perm exact, the
    gcn_norm weights within 1e-6 of float64"""
    ref = _loops(ei, n) if self_loops else ei
    # (with self loops the kept input edges keep their ids, node i's loop has id E + i)
    ids = np.concatenate([np.nonzero(ei[0] != ei[1])[0], ei.shape[1] + np.arange(n)]) if self_loops \
        else np.arange(ei.shape[1])
    deg = np.bincount(ref[1], minlength=n).astype(np.float64)
    dis = np.where(deg > 0, np.maximum(deg, 1.0) ** -0.5, 0.0)
    for side, key_row in ((0, 1), (1, 0)):
        order = np.argsort(ref[key_row], kind="stable")
        ptr = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(ref[key_row], minlength=n), out=ptr[1:])
        got = [o.numpy() for o in out[side * per:(side + 1) * per]]
        assert np.array_equal(got[0], ptr), (cid, "ptr", side)
        assert np.array_equal(got[1], ref[1 - key_row][order]), (cid, "other", side)
        assert np.array_equal(got[2], ids[order]), (cid, "perm", side)
        if normalize:
            w = (dis[ref[0]] * dis[ref[1]])[order]
            assert np.abs(got[3] - w).max() <= 1e-6 * max(np.abs(w).max(), 1e-30), (cid, "w", side)


def _graph_case(cid, ei, n, self_loops=False, segments=None, normalize=True, rebuild=False, setenv=None):
    e_out = _loops(ei, n).shape[1] if self_loops else ei.shape[1]

    def run(t):
        from deformcontact_amd import graph
        from deformcontact_amd.graph import GraphIndex
        graph._SHARED_STATUS.clear()                               # the device's shared status word: allocated by this run
        g = GraphIndex(t["ei"], n, self_loops=self_loops, normalize=normalize, segments=segments,
                       loops_segmented=segments is not None)
        assert (g._segments is not None) == (segments is not None), "the build this case names did not run"
        if rebuild:
            g.rebuild()
        out = []
        for adj in (g.fwd, g.bwd):
            out += [adj.ptr, adj.other[:e_out].contiguous(), adj.perm[:e_out].contiguous()]
            if normalize:
                out.append(adj.w[:e_out].contiguous())
        return out + [g._status]

    def reference(out):
        _check_sides(out, ei, n, self_loops, normalize, cid, 4 if normalize else 3)
        assert int(out[-1]) == 0
    gadd(cid, run, {"ei": torch.from_numpy(ei)}, index_inputs={"ei": n - 1}, reference=reference,
         partial=(next(r for r in (n + 1, e_out) if all(r % t for t in (8, 16, 32, 64, 128, 256, 1024))), 256), slack="ei",
         setenv=setenv)


for _n in SIZES:
    _graph_case(f"c:graph-build-bucketed-n{_n}", nf.GRAPHS[_n], _n, setenv=BUCKETED)
    _graph_case(f"c:graph-build-bucketed-loops-n{_n}", nf.GRAPHS[_n], _n, self_loops=True, setenv=BUCKETED)
    _graph_case(f"c:graph-build-n{_n}", nf.GRAPHS[_n], _n)
    _graph_case(f"c:graph-build-loops-n{_n}", nf.GRAPHS[_n], _n, self_loops=True)
    _graph_case(f"c:graph-rebuild-n{_n}", nf.GRAPHS[_n], _n, rebuild=True)
_bei, _bseg = _batch_graph()
_graph_case("c:graph-build-batch", _bei, sum(BATCH))
_graph_case("c:graph-build-bucketed-batch", _bei, sum(BATCH), setenv=BUCKETED)
_graph_case("c:graph-build-segmented-batch", _bei, sum(BATCH), segments=_bseg)
_graph_case("c:graph-build-segmented-loops-batch", _bei, sum(BATCH), self_loops=True, segments=_bseg, normalize=False)
_graph_case("c:graph-build-unnormalised-batch", _bei, sum(BATCH), normalize=False)


def _csr_workspace(nbytes):
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)


def _csr_case(n, self_loops=False, setenv=None):
    """dc_csr_build: one side per call, test-owned outputs; the status word starts at 1 (the entry clears it)"""
    ei = nf.GRAPHS[n]
    e = ei.shape[1]
    cap = e + (n if self_loops else 0)
    e_out = _loops(ei, n).shape[1] if self_loops else e
    cid = f"c:csr-build{'-bucketed' if setenv else ''}{'-loops' if self_loops else ''}-n{n}"

    def run(t):
        from deformcontact_amd import _lib
        L = _lib.lib()
        status = torch.ones(1, dtype=torch.int32, device=DEV)
        ws = _csr_workspace(L.dc_csr_workspace_bytes(e, n))
        out, deg = [], None
        for key_row in (1, 0):
            ptr = torch.empty(n + 1, dtype=torch.int32, device=DEV)
            other, perm = (torch.empty(cap, dtype=torch.int32, device=DEV) for _ in range(2))
            w = torch.empty(cap, dtype=torch.float32, device=DEV)
            _lib.check(L.dc_csr_build(t["ei"].data_ptr(), e, n, key_row, int(self_loops), ptr.data_ptr(), other.data_ptr(),
                                      perm.data_ptr(), deg, w.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                      _st()), "csr_build")
            deg = ptr.data_ptr() if key_row else deg
            out += [ptr, other[:e_out], perm[:e_out], w[:e_out]]
        return out + [status]

    def reference(out):
        _check_sides(out, ei, n, self_loops, True, cid, 4)
        assert int(out[-1]) == 0
    gadd(cid, run, {"ei": torch.from_numpy(ei)}, index_inputs={"ei": n - 1}, reference=reference,
         partial=(n + 1, 256), slack="ei", setenv=setenv)


for _n in SIZES:
    _csr_case(_n)
    _csr_case(_n, setenv=BUCKETED)
    _csr_case(_n, self_loops=True, setenv=BUCKETED)


def _batch_ids(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


def _neighbor_case(kind, sizes, cap, r=None, f=3):
    """knn / radius on positions (the grid path) and knn on feature rows of width ``f`` (the search inside
    DynamicEdgeConv): the padded result and the compacted edge list"""
    n = sum(sizes)
    batched = len(sizes) > 1
    rng = np.random.default_rng(n + cap + f)
    x = torch.from_numpy(rng.random((n, f), dtype=np.float32))
    inputs = {"x": x}
    if batched:
        inputs["batch"] = _batch_ids(sizes)

    def run(t):
        from deformcontact_amd import neighbors
        b = t.get("batch")
        if kind == "radius":
            nbr, counts = neighbors.radius_padded(t["x"], t["x"], r, b, b, cap, exclude_self=True)
        else:
            nbr, counts = neighbors.knn_padded(t["x"], t["x"], cap, b, b, exclude_self=True)
        edges = neighbors._edges(nbr, counts, 1, b)
        # the padding of a row (slots from counts[i] on) is -1 by contract: part of the output
        return [nbr, counts, edges]

    def reference(out):
        b = inputs["batch"].numpy() if batched else None
        if f == 3:
            from tests.test_neighbors import ref_graph
            want = ref_graph(x.numpy(), cap, r, b, loop=False)
        else:
            from tests.nd_reference import edges_ref, knn_ref
            nbr, counts = knn_ref(x.numpy(), x.numpy(), cap, b, b, exclude_self=True)
            assert np.array_equal(out[0].numpy(), nbr) and np.array_equal(out[1].numpy(), counts)
            want = torch.from_numpy(edges_ref(nbr, counts, 1))
        assert torch.equal(out[2], want), (kind, sizes, cap)
    gadd(f"c:{kind}{'-nd' + str(f) if f != 3 else ''}-n{'+'.join(map(str, sizes))}-cap{cap}", run, inputs,
         index_inputs={"batch": len(sizes) - 1} if batched else {}, reference=reference, partial=(n, 32), slack="x")


for _sizes in [(67,), (259,), (1,), BATCH]:
    _neighbor_case("knn", _sizes, 6)
    _neighbor_case("radius", _sizes, 9, r=0.3)
    _neighbor_case("knn", _sizes, 5, f=35)                       # DynamicEdgeConv: one past the 32-column chunk


def _fps_case(sizes, ratio=0.5):
    n = sum(sizes)
    p = _points(n, 300 + n)
    batched = len(sizes) > 1
    inputs = {"x": p}
    if batched:
        inputs["batch"] = _batch_ids(sizes)

    def run(t):
        from deformcontact_amd import pointops
        return [pointops.fps(t["x"], t.get("batch"), ratio=ratio, random_start=False)]

    def reference(out):
        from tests.test_fps import ref_batch
        assert np.array_equal(out[0].numpy(), ref_batch(p.numpy(), sizes, ratio))
    m = int(sum(min(int(np.ceil(np.float32(s) * np.float32(ratio))), s) for s in sizes))
    gadd(f"c:fps-n{'+'.join(map(str, sizes))}", run, inputs, index_inputs={"batch": len(sizes) - 1} if batched else {},
         reference=reference, partial=(m, 64), slack="x")


def _interp_case(sizes, f, k=3):
    nx = sum(sizes)
    sy = tuple(max(1, s // 2 + 1) for s in sizes)
    ny = sum(sy)
    px, py = _points(nx, 400 + nx), _points(ny, 500 + ny)
    x = torch.from_numpy(np.random.default_rng(f).standard_normal((nx, f), dtype=np.float32))
    batched = len(sizes) > 1
    inputs = {"x": x, "px": px, "py": py}
    if batched:
        inputs.update(bx=_batch_ids(sizes), by=_batch_ids(sy))

    def run(t):
        from deformcontact_amd import neighbors, pointops
        with torch.no_grad():
            y = pointops.knn_interpolate(t["x"], t["px"], t["py"], t.get("bx"), t.get("by"), k=k)
        xg = t["x"].clone().requires_grad_(True)
        yg = pointops.knn_interpolate(xg, t["px"], t["py"], t.get("bx"), t.get("by"), k=k)
        (gx,) = torch.autograd.grad(yg, xg, torch.ones_like(yg))
        nbr, counts = neighbors.knn_padded(t["px"], t["py"], k, t.get("bx"), t.get("by"))
        return [y, yg.detach(), gx, nbr, counts]

    def reference(out):
        from tests.nd_reference import knn_ref
        from tests.test_knn_interpolate import ref_backward, ref_forward
        bx, by = (inputs[k].numpy() if batched else None for k in ("bx", "by"))
        nbr, counts = knn_ref(px.numpy(), py.numpy(), k, bx, by)      # (three columns: the grid path's d2 and ranking)
        assert np.array_equal(out[3].numpy(), nbr) and np.array_equal(out[4].numpy(), counts)
        want = ref_forward(x.numpy(), px.numpy(), py.numpy(), nbr, counts)
        assert np.array_equal(out[0].numpy(), want) and np.array_equal(out[1].numpy(), want)
        gx = ref_backward(np.ones((ny, f), np.float32), px.numpy(), py.numpy(), nbr, counts, nx, np.float64)
        assert np.abs(out[2].numpy() - gx).max() <= 1e-5 * max(np.abs(gx).max(), 1e-30)
    idx = {"bx": len(sizes) - 1, "by": len(sizes) - 1} if batched else {}
    gadd(f"c:knn_interpolate-n{'+'.join(map(str, sizes))}-f{f}", run, inputs, index_inputs=idx, reference=reference,
         partial=(ny, 64), slack="x")


def _morton_case(n):
    rng = np.random.default_rng(n)
    pos = np.concatenate([rng.uniform(-1, 2, (n - n // 3, 3)), 0.5 + rng.normal(0, 0.01, (n // 3, 3))]).astype(np.float32)
    if n > 10:
        pos[5] = pos[3]

    def run(t):
        from deformcontact_amd.graph import NodeOrder
        o = NodeOrder.morton(t["pos"])
        return [o.perm, o.inv]

    def reference(out):
        from tests.test_node_order import _codes
        perm, inv = out[0].numpy(), out[1].numpy()
        assert sorted(perm.tolist()) == list(range(n)) and np.array_equal(inv[perm], np.arange(n))
        c = _codes(pos)[perm].astype(np.int64)
        assert (np.diff(c) >= 0).all() and (np.diff(perm)[np.diff(c) == 0] > 0).all()
    gadd(f"c:morton-n{n}", run, {"pos": torch.from_numpy(pos)}, reference=reference, partial=(n, 256), slack="pos")


def _spline_case(n, dim):
    e = nf.GRAPHS[n].shape[1]
    ks, op = (5, 3, 4)[:dim], (1, 0, 1)[:dim]
    a = torch.from_numpy(np.random.default_rng(e + dim).random((e, dim), dtype=np.float32))
    a[0], a[-1] = 0.0, 1.0                                          # both ends of the knot range

    def run(t):
        from deformcontact_amd import ops
        b, wi = ops._spline_basis(t["a"], ks, op, 1)
        return [b, wi]

    def reference(out):
        b, wi = linear_spline_basis(a.numpy(), ks, op)
        assert np.array_equal(out[0].numpy(), b) and np.array_equal(out[1].numpy().astype(np.int64), wi)
    gadd(f"c:spline-basis-n{n}-d{dim}", run, {"a": a}, reference=reference, partial=(e, 256), slack="a")


def _pool_case(sizes, c, mode):
    """the global pools with the batch vector as a hosted index input, forward and backward"""
    n, nb = sum(sizes), len(sizes)
    x = torch.from_numpy(np.random.default_rng(n + c).integers(-8, 9, (n, c)).astype(np.float32) / 4)

    def run(t):
        from deformcontact_amd import pointops
        fn = {"add": pointops.global_add_pool, "mean": pointops.global_mean_pool, "max": pointops.global_max_pool}[mode]
        xg = t["x"].clone().requires_grad_(True)
        y = fn(xg, t["batch"], nb)
        (gx,) = torch.autograd.grad(y, xg, torch.ones_like(y))
        return [y.detach(), gx]

    def reference(out):
        b = _batch_ids(sizes)
        x64 = x.double()
        if mode == "max":
            want = nf.ref_amax(b, x64, nb)
        else:
            want = torch.zeros(nb, c, dtype=torch.float64).index_add_(0, b, x64)
            if mode == "mean":
                want = want / torch.tensor(sizes).clamp(min=1).double().unsqueeze(1)
        # (multiples of 0.25 in [-2, 2]: sums of up to 259 rows and their maxima are exact in float32; the mean rounds)
        if mode == "mean":
            assert (out[0].double() - want).abs().max() <= 1e-6 * want.abs().max().clamp(min=1e-30), (sizes, c)
        else:
            assert torch.equal(out[0].double(), want), (sizes, c, mode)
    gadd(f"c:pool-{mode}-n{'+'.join(map(str, sizes))}-c{c}", run, {"x": x, "batch": _batch_ids(sizes)},
         index_inputs={"batch": nb - 1}, reference=reference, partial=(n, 16), slack="x")


for _sizes in [(67,), (259,), (1,), BATCH]:
    _fps_case(_sizes)
    _interp_case(_sizes, 67)
    for _mode in ("add", "mean", "max"):
        _pool_case(_sizes, 35, _mode)
for _n in SIZES:
    _morton_case(_n)
    _spline_case(_n, 2)
_spline_case(259, 3)


# ---- (d) outputs with a leading dimension through the C ABI ---------------------------------------------------------------
def _frand(shape, seed, scale=1.0):
    return tls._rand(shape, seed, scale)


def _dense_ld_case(entry, n, fi, fo, nseg, pad):
    """the dense entries with ``ld = cols + pad`` on the output (forward: out; dX: the gradient slab; dW: the weight
    gradients), contiguous operands"""
    inputs = {"x": _frand((n, nseg * fi), 1), "w": _frand((nseg, fo, fi), 2, fi ** -0.5), "b": _frand((fo,), 3, 0.5),
              "g": _frand((n, fo), 4), "y": _frand((n, fo), 5)}

    def run(t):
        from deformcontact_amd import _lib, ops
        from deformcontact_amd.ops import _i64_array, _ptr_array
        L, st = _lib.lib(), _st()
        ws = [t["w"][s] for s in range(nseg)]
        xs, ldx = [t["x"][:, s * fi:(s + 1) * fi] for s in range(nseg)], [nseg * fi] * nseg
        h2 = entry.endswith(("h2", "h2p"))                       # (the maxima stay alive until the launch is enqueued)
        xmax, gmax, wmax = (ops.rowabsmax(t["x"]), ops.rowabsmax(t["g"]), ops.weight_rowmax(ws)) if h2 else (None,) * 3
        if entry.startswith("fwd"):
            out = strided_out(n, fo, fo + pad, device=DEV)
            head = (_ptr_array(xs), _i64_array(ldx), _ptr_array(ws), nseg, t["b"].data_ptr(), 1, out.data_ptr(), fo + pad,
                    n, fi, fo)
            if entry == "fwd":
                rc = L.dc_tag_linear_fwd(*head, st)
            elif entry == "fwd_split":
                rc = L.dc_tag_linear_fwd_split(*head, 6, st)
            elif entry == "fwd_h2":
                rc = L.dc_tag_linear_fwd_h2(*head, xmax.data_ptr(), wmax.data_ptr(), st)
            else:
                k = nseg * fi
                wm, wimg = torch.empty(fo, device=DEV), torch.empty(fo, k, device=DEV)
                _lib.check(L.dc_tag_weight_prep(_ptr_array(ws), nseg, fo, fi, wm.data_ptr(), wimg.data_ptr(), None, None,
                                                st), "weight_prep")
                rc = L.dc_tag_linear_fwd_h2p(t["x"].data_ptr(), k, wimg.data_ptr(), t["b"].data_ptr(), 1, out.data_ptr(),
                                             fo + pad, n, k, fo, xmax.data_ptr(), wm.data_ptr(), None, 0, st)
            _lib.check(rc, entry)
            return [out]
        if entry.startswith("dx"):
            ld = nseg * fi + pad
            gslab = strided_out(n, nseg * fi, ld, device=DEV)
            gxs = [gslab[:, s * fi:(s + 1) * fi] for s in range(nseg)]
            head = (t["g"].data_ptr(), fo, t["y"].data_ptr(), fo, _ptr_array(ws), nseg, _ptr_array(gxs),
                    _i64_array([ld] * nseg))
            if entry == "dx":
                rc = L.dc_tag_linear_bwd_dx(*head, n, fi, fo, st)
            else:
                wsb = L.dc_tag_linear_bwd_dx_split_workspace_bytes(fi, fo, nseg)
                wsx = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
                if entry == "dx_split":
                    rc = L.dc_tag_linear_bwd_dx_split(*head, wsx.data_ptr(), wsb, n, fi, fo, 6, st)
                else:
                    rc = L.dc_tag_linear_bwd_dx_h2(*head, wsx.data_ptr(), wsb, n, fi, fo, gmax.data_ptr(), wmax.data_ptr(), st)
            _lib.check(rc, entry)
            return [gslab]
        raise AssertionError(entry)

    def reference(out):
        x, w, g = inputs["x"].double(), inputs["w"].double(), inputs["g"].double()
        gm = g * (inputs["y"] > 0).double()
        if entry.startswith("fwd"):
            want = [(sum(x[:, s * fi:(s + 1) * fi] @ w[s].t() for s in range(nseg)) + inputs["b"].double()).clamp_min(0)]
        elif entry.startswith("dx"):
            want = [torch.cat([gm @ w[s] for s in range(nseg)], dim=1)]
        for o, r in zip(out, want):                                 # TOL of tests/test_launch_sites.py, products 0 / 6 / 2
            assert (o.double() - r).abs().max() <= 2e-6 * r.abs().max(), (entry, n, fi, fo)
    gadd(f"d:dense-{entry}-{n}x{fi}x{fo}x{nseg}-ld+{pad}", run, inputs, reference=reference, partial=(n, 64), slack="x")


# (dW takes no leading dimension for its outputs: gw_cols is the column count of dense [Fo, gw_cols] blocks)
for _entry in ("fwd", "fwd_split", "fwd_h2", "fwd_h2p", "dx", "dx_split", "dx_h2"):
    _dense_ld_case(_entry, 129, 16, 136 if _entry.startswith("fwd") else 144, 2, 4)
    if _entry in ("fwd", "dx"):                                     # the generic kernels take any leading dimension
        _dense_ld_case(_entry, 129, 5, 7, 2, 1)


def _dense_ld_case2(entry, n, fi, fo, nseg, pad):
    """the remaining forward entries with an output leading dimension: the narrow first-layer block (slab of width
    ``wpad``, weights as given or as the prepared image) and the bf16 block (fp32 or bf16 output)"""
    wpad = 96
    inputs = {"x": _frand((n, nseg * fi), 18), "w": _frand((nseg, fo, fi), 19, fi ** -0.5), "b": _frand((fo,), 20, 0.5)}
    if entry.startswith("bf16"):
        inputs["x"], inputs["w"] = inputs["x"].bfloat16(), inputs["w"].bfloat16()

    def run(t):
        from deformcontact_amd import _lib
        from deformcontact_amd.ops import _ptr_array
        L, st, ldo = _lib.lib(), _st(), fo + pad
        bp = t["b"].data_ptr()
        if entry.startswith("bf16"):
            od = torch.bfloat16 if entry == "bf16_bf16" else torch.float32
            out = strided_out(n, fo, ldo, dtype=od, device=DEV)
            w = t["w"][0]
            rc = L.dc_tag_linear_fwd_bf16(t["x"].data_ptr(), fi, w.data_ptr(), bp, 1, out.data_ptr(), ldo,
                                          int(od == torch.bfloat16), n, fi, fo, st)
        else:
            assert L.dc_tag_linear_fwd_narrow_ok(fi, nseg, wpad, fo) == 1
            slab = torch.zeros(n, wpad, device=DEV)
            slab[:, :nseg * fi] = t["x"]
            ws = [t["w"][s] for s in range(nseg)]
            out = strided_out(n, fo, ldo, device=DEV)
            if entry == "narrow_img":
                buf = torch.zeros(wpad // 16 * 24576, dtype=torch.uint8, device=DEV)
                _lib.check(L.dc_tag_narrow_wimage(_ptr_array(ws), nseg, fi, wpad, buf.data_ptr(), st), "wimage")
                rc = L.dc_tag_linear_fwd_narrow_img(slab.data_ptr(), wpad, buf.data_ptr(), bp, 1, out.data_ptr(), ldo, n,
                                                    wpad, fo, st)
            else:
                rc = L.dc_tag_linear_fwd_narrow(slab.data_ptr(), wpad, _ptr_array(ws), nseg, fi, bp, 1, out.data_ptr(), ldo,
                                                n, wpad, fo, st)
        _lib.check(rc, entry)
        return [out]

    def reference(out):
        x, w = inputs["x"].double(), inputs["w"].double()
        want = (sum(x[:, s * fi:(s + 1) * fi] @ w[s].t() for s in range(nseg)) + inputs["b"].double()).clamp_min(0)
        # bf16 output: one rounding to bf16 on store; bf16 operands: exact products, fp32 accumulation over K = 64
        tol = {"bf16_bf16": 2.0 ** -8, "bf16_f32": 1e-5}.get(entry, 2e-6)
        assert (out[0].double() - want).abs().max() <= tol * want.abs().max(), (entry, n, fi, fo)
    gadd(f"d:dense-{entry}-{n}x{fi}x{fo}x{nseg}-ld+{pad}", run, inputs, reference=reference, partial=(n, 64), slack="x")


_dense_ld_case2("narrow", 67, 21, 256, 4, 4)
_dense_ld_case2("narrow_img", 259, 21, 256, 4, 4)
_dense_ld_case2("bf16_f32", 67, 64, 40, 1, 4)
_dense_ld_case2("bf16_bf16", 259, 64, 40, 1, 8)


def _pack_ld_case(n, f, pad):
    """dc_spmm_f32_pack with ``lds = wpad + pad``: slab = [x | A x | (untouched) | 0]"""
    ei, width, wpad = nf.GRAPHS[n], 4 * f, 96
    g, w = nf._lazy(lambda: nf._graph(ei, n)), nf.gcn_weights(ei, n)[1]
    inputs = {"x": _frand((n, f), 21)}

    def run(t):
        from deformcontact_amd import _lib
        adj = g().fwd
        slab = strided_out(n, wpad, wpad + pad, device=DEV)
        slab[:, 2 * f:width] = 7.0                                # blocks 2..K belong to the later hops: not written here
        _lib.check(_lib.lib().dc_spmm_f32_pack(adj.ptr.data_ptr(), adj.other.data_ptr(), adj.w.data_ptr(), t["x"].data_ptr(),
                                               f, slab.data_ptr(), wpad + pad, n, f, width, wpad, _st()), "pack")
        return [slab]

    def reference(out):
        x = inputs["x"].double()
        assert torch.equal(out[0][:, :f], inputs["x"]) and (out[0][:, 2 * f:width] == 7.0).all()
        assert not out[0][:, width:].any()
        hop = nf.ref_spmm(ei, w, x)
        assert (out[0][:, f:2 * f].double() - hop).abs().max() <= 1e-5 * hop.abs().max()
    gadd(f"d:spmm-pack-n{n}-f{f}-ld+{pad}", run, inputs, reference=reference, partial=(n, 8), slack="x")


_pack_ld_case(259, 21, 4)
_pack_ld_case(67, 21, 1)


def _spmm_ld_case(entry, n, f, pad):
    ei = nf.GRAPHS[n]
    g = nf._lazy(lambda: nf._graph(ei, n, self_loops=entry == "bias_act"))
    inputs = {"x": _frand((n, f), 6), "a": _frand((n, f), 7), "b": _frand((f,), 8, 0.5)}
    if entry.startswith("bf16"):
        inputs["x"] = inputs["x"].bfloat16()
        if entry == "bf16_bf16":
            inputs["a"] = inputs["a"].bfloat16()

    def run(t):
        from deformcontact_amd import _lib
        L, adj, ld = _lib.lib(), g().fwd, f + pad
        head = (adj.ptr.data_ptr(), adj.other.data_ptr(), adj.w.data_ptr(), t["x"].data_ptr(), f)
        if entry == "f32":
            y = strided_out(n, f, ld, device=DEV)
            rc = L.dc_spmm_f32(*head, t["a"].data_ptr(), f, y.data_ptr(), ld, n, f, _st())
            out = [y]
        elif entry == "rowmax":
            y, rm = strided_out(n, f, ld, device=DEV), torch.empty(n, device=DEV)
            rc = L.dc_spmm_f32_rowmax(*head, t["a"].data_ptr(), f, y.data_ptr(), ld, n, f, rm.data_ptr(), 1, _st())
            out = [y, rm]
        elif entry == "bias_act":
            y = strided_out(n, f, ld, device=DEV)
            rc = L.dc_spmm_f32_bias_act(*head, t["b"].data_ptr(), 1, y.data_ptr(), ld, n, f, _st())
            out = [y]
        else:
            od = torch.bfloat16 if entry == "bf16_bf16" else torch.float32
            y = strided_out(n, f, ld, dtype=od, device=DEV)
            rc = L.dc_spmm_bf16(*head, t["a"].data_ptr(), f, y.data_ptr(), ld, n, f, int(od == torch.float32), _st())
            out = [y]
        _lib.check(rc, entry)
        return out

    def reference(out):
        ei_l, w = nf.gcn_weights(ei, n, loops=entry == "bias_act")
        y = nf.ref_spmm(ei_l, w, inputs["x"].double())
        y = (y + inputs["b"].double()).clamp_min(0) if entry == "bias_act" else y + inputs["a"].double()
        tol = 1e-5 if entry != "bf16_bf16" else 2.0 ** -8           # (one rounding to bf16 on store)
        assert (out[0].double() - y).abs().max() <= tol * y.abs().max(), (entry, n, f)
        if entry == "rowmax":
            want = torch.maximum(out[0].abs().amax(1), inputs["x"].abs().amax(1))
            assert torch.equal(out[1], want)
    gadd(f"d:spmm-{entry}-n{n}-f{f}-ld+{pad}", run, inputs, reference=reference, partial=(n, 8), slack="x")


for _entry in ("f32", "rowmax", "bias_act", "bf16_bf16", "bf16_f32"):
    for _n, _f, _pad in [(259, 64, 4), (67, 30, 1), (259, 260, 4)]:
        _spmm_ld_case(_entry, _n, _f, _pad)


def _layer_ld_case(entry, n, f, pad):
    """segment kernels of the layers through the C ABI with ``ldy = F + pad``: SAGE mean / max (with its tie counts),
    GINE, and the global pools over a ragged batch with an empty graph"""
    ei = nf.GRAPHS[n]
    g = nf._raw_graph(ei, n)
    src = torch.from_numpy(ei[0])
    sizes = (1, 37, 0, n - 38)
    grid = torch.from_numpy(np.random.default_rng(n + f).integers(-8, 9, (n, f)).astype(np.float32) / 4)
    inputs = {"x": grid if entry in ("sage_max", "pool_max") else _frand((n, f), 14), "e": _frand((ei.shape[1], f), 15)}

    def run(t):
        from deformcontact_amd import _lib
        L, ld = _lib.lib(), f + pad
        adj = g().fwd
        if entry == "sage_mean":
            y = strided_out(n, f, ld, device=DEV)
            rc = L.dc_sage_mean_fwd(adj.ptr.data_ptr(), adj.other.data_ptr(), t["x"].data_ptr(), f, y.data_ptr(), ld, n, f, _st())
            out = [y]
        elif entry == "sage_max":
            y, cnt = strided_out(n, f, ld, device=DEV), strided_out(n, f, ld, dtype=torch.int32, device=DEV)
            rc = L.dc_sage_max_fwd(adj.ptr.data_ptr(), adj.other.data_ptr(), t["x"].data_ptr(), f, y.data_ptr(), ld,
                                   cnt.data_ptr(), ld, n, f, _st())
            out = [y, cnt]
        elif entry == "gine":
            y = strided_out(n, f, ld, device=DEV)
            rc = L.dc_gine_fwd(adj.ptr.data_ptr(), adj.other.data_ptr(), adj.perm.data_ptr(), t["x"].data_ptr(), f,
                               t["e"].data_ptr(), f, None, y.data_ptr(), ld, n, f, _st())
            out = [y]
        else:
            mode = {"pool_add": 0, "pool_mean": 1, "pool_max": 2}[entry]
            ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64).to(DEV)
            y = strided_out(len(sizes), f, ld, device=DEV)
            cnt = strided_out(len(sizes), f, ld, dtype=torch.int32, device=DEV) if mode == 2 else None
            rc = L.dc_pool_fwd(ptr.data_ptr(), t["x"].data_ptr(), f, y.data_ptr(), ld, None if cnt is None else cnt.data_ptr(),
                               ld, mode, n, len(sizes), f, _st())
            out = [y] + ([cnt] if cnt is not None else [])
        _lib.check(rc, entry)
        return out

    def reference(out):
        t64 = {k: v.double() for k, v in inputs.items()}
        if entry.startswith("sage"):
            want = nf._ref_aggregate(ei, n, lambda t: t["x"][src], entry[5:])(t64)[0]
        elif entry == "gine":
            want = nf._ref_aggregate(ei, n, lambda t: (t["x"][src] + t["e"]).clamp_min(0), "sum")(t64)[0]
        else:
            b = _batch_ids(sizes)
            if entry == "pool_max":
                want = nf.ref_amax(b, t64["x"], len(sizes))
            else:
                want = torch.zeros(len(sizes), f, dtype=torch.float64).index_add_(0, b, t64["x"])
                if entry == "pool_mean":
                    want = want / torch.tensor(sizes).clamp(min=1).double().unsqueeze(1)
        if entry.endswith("max"):
            assert torch.equal(out[0].double(), want), entry       # a selection: exact
        else:
            assert (out[0].double() - want).abs().max() <= 1e-5 * want.abs().max(), entry
    rows = n if not entry.startswith("pool") else len(sizes)
    gadd(f"d:layer-{entry}-n{n}-f{f}-ld+{pad}", run, inputs, reference=reference, partial=(rows, 8), slack="x")


for _entry in ("sage_mean", "sage_max", "gine", "pool_add", "pool_mean", "pool_max"):
    _layer_ld_case(_entry, 259, 32, 4)
    _layer_ld_case(_entry, 67, 35, 1)


def _window_ld_case(entry, f, pad):
    """dc_spmm_f32_window / dc_spmm_f32_rowmax_window: the hop over part 1 of a merged adjacency (rows 256.. of the
    merged node space) on that part's own feature matrix, ``ldy = F + pad``"""
    parts = [(nf.GRAPHS[67], 67), (nf.GRAPHS[259], 259)]
    ei, n = parts[1]
    mg = nf._lazy(lambda: __import__("deformcontact_amd").graph.GraphIndex.from_parts(
        [(torch.from_numpy(e).to(DEV), k) for e, k in parts]))
    inputs = {"x": _frand((n, f), 22), "a": _frand((n, f), 23)}

    def run(t):
        from deformcontact_amd import _lib
        L, adj, ld = _lib.lib(), mg().window(1).fwd, f + pad
        assert adj.row_offset > 0
        y = strided_out(n, f, ld, device=DEV)
        head = (adj.ptr.data_ptr(), adj.other.data_ptr(), adj.w.data_ptr(), t["x"].data_ptr(), f, t["a"].data_ptr(), f,
                y.data_ptr(), ld, n, f)
        if entry == "window":
            _lib.check(L.dc_spmm_f32_window(*head, adj.row_offset, _st()), entry)
            return [y]
        rm = torch.empty(n, device=DEV)
        _lib.check(L.dc_spmm_f32_rowmax_window(*head, rm.data_ptr(), 1, adj.row_offset, _st()), entry)
        return [y, rm]

    def reference(out):
        want = nf.ref_spmm(ei, nf.gcn_weights(ei, n)[1], inputs["x"].double()) + inputs["a"].double()
        assert (out[0].double() - want).abs().max() <= 1e-5 * want.abs().max()
        if entry == "rowmax_window":
            assert torch.equal(out[1], torch.maximum(out[0].abs().amax(1), inputs["x"].abs().amax(1)))
    gadd(f"d:spmm-{entry}-f{f}-ld+{pad}", run, inputs, reference=reference, partial=(n, 8), slack="x")


for _entry in ("window", "rowmax_window"):
    _window_ld_case(_entry, 64, 4)
    _window_ld_case(_entry, 30, 1)


def _mask_grad_ld_case(n, f, pad):
    """dc_tag_mask_grad: gm = g * (out > 0) into a column block of a slab (``ldgm = F + pad``) and its row maxima"""
    inputs = {"g": _frand((n, f), 24), "y": _frand((n, f), 25)}

    def run(t):
        from deformcontact_amd import _lib
        gm, rm = strided_out(n, f, f + pad, device=DEV), torch.empty(n, device=DEV)
        _lib.check(_lib.lib().dc_tag_mask_grad(t["g"].data_ptr(), f, t["y"].data_ptr(), f, gm.data_ptr(), f + pad, n, f,
                                               rm.data_ptr(), None, _st()), "mask_grad")
        return [gm, rm]

    def reference(out):
        gm = inputs["g"] * (inputs["y"] > 0)
        assert torch.equal(out[0], gm) and torch.equal(out[1], gm.abs().amax(1))
    gadd(f"d:mask-grad-n{n}-f{f}-ld+{pad}", run, inputs, reference=reference, partial=(n, 64), slack="g")


_mask_grad_ld_case(259, 64, 4)
_mask_grad_ld_case(67, 36, 4)


def _h2p_variant_ld_case(entry, n, k, fo, pad):
    """dc_tag_linear_fwd_h2p_exp (out = exp(x W^T - lse), zeros from ``ncols_valid`` on) and dc_tag_linear_fwd_h2p_corr
    (left operand x - coef[row] * x2, the 128 x 256 tile kernel on ragged tiles), ``ldo = Fo + pad``"""
    ncols = fo - 2
    inputs = {"x": _frand((n, k), 26, 0.5), "x2": _frand((n, k), 27, 0.5), "coef": _frand((n,), 28, 0.5),
              "w": _frand((fo, k), 29, k ** -0.5)}
    inputs["lse"] = torch.logsumexp(inputs["x"].double() @ inputs["w"].double().t()[:, :ncols], dim=1).float()

    def run(t):
        from deformcontact_amd import _lib, ops
        from deformcontact_amd.ops import _ptr_array
        L, st = _lib.lib(), _st()
        wmax, wimg = ops.weight_rowmax([t["w"]]), torch.empty(fo, k, device=DEV)
        _lib.check(L.dc_tag_weight_prep(_ptr_array([t["w"]]), 1, fo, k, wmax.data_ptr(), wimg.data_ptr(), None, None, st),
                   "weight_prep")
        out = strided_out(n, fo, fo + pad, device=DEV)
        if entry == "h2p_exp":
            xmax = ops.rowabsmax(t["x"])
            rc = L.dc_tag_linear_fwd_h2p_exp(t["x"].data_ptr(), k, wimg.data_ptr(), out.data_ptr(), fo + pad, n, k, fo,
                                             xmax.data_ptr(), wmax.data_ptr(), t["lse"].data_ptr(), ncols, st)
        else:
            xmax = (t["x"] - t["coef"].unsqueeze(1) * t["x2"]).abs().amax(1).contiguous()
            rc = L.dc_tag_linear_fwd_h2p_corr(t["x"].data_ptr(), k, t["x2"].data_ptr(), t["coef"].data_ptr(), wimg.data_ptr(),
                                              out.data_ptr(), fo + pad, n, k, fo, xmax.data_ptr(), wmax.data_ptr(), st)
        _lib.check(rc, entry)
        torch.cuda.current_stream().synchronize()                 # (xmax, wmax and the image stay alive until the launch ran)
        return [out]

    def reference(out):
        x, w = inputs["x"].double(), inputs["w"].double()
        if entry == "h2p_exp":
            want = torch.exp(x @ w.t() - inputs["lse"].double().unsqueeze(1))
            # scores within 2e-6 of their row scale (<= 6 here), so exp within 1.2e-5 relative; the values are <= 1
            assert (out[0][:, :ncols].double() - want[:, :ncols]).abs().max() <= 2e-5 and not out[0][:, ncols:].any()
        else:
            want = (x - inputs["coef"].double().unsqueeze(1) * inputs["x2"].double()) @ w.t()
            assert (out[0].double() - want).abs().max() <= 2e-6 * want.abs().max()      # tests/test_launch_sites.py
    gadd(f"d:dense-{entry}-{n}x{k}x{fo}-ld+{pad}", run, inputs, reference=reference, partial=(n, 128), slack="x")


_h2p_variant_ld_case("h2p_exp", 131, 32, 72, 4)
_h2p_variant_ld_case("h2p_corr", 130, 64, 260, 4)


def _edge_ld_case(entry, n, f, pad):
    """dc_edge_pair_fwd (z[e] = [x_i, x_j - x_i], ``ldz = 2 F + pad``) and dc_edge_reduce_fwd (sum / mean / max of the
    per-edge rows per destination, ``ldy = C + pad``, the max with its tie counts)"""
    ei = nf.GRAPHS[n]
    e = ei.shape[1]
    g = nf._raw_graph(ei, n)
    grid = torch.from_numpy(np.random.default_rng(e + f).integers(-8, 9, (e, f)).astype(np.float32) / 4)
    inputs = {"x": _frand((n, f), 30), "m": grid if entry == "reduce_max" else _frand((e, f), 31), "ei": torch.from_numpy(ei)}

    def run(t):
        from deformcontact_amd import _lib
        L = _lib.lib()
        if entry == "pair":
            z = strided_out(e, 2 * f, 2 * f + pad, device=DEV)
            _lib.check(L.dc_edge_pair_fwd(t["ei"][0].data_ptr(), t["ei"][1].data_ptr(), t["x"].data_ptr(), f, z.data_ptr(),
                                          2 * f + pad, n, e, f, _st()), entry)
            return [z]
        adj, mode = g().fwd, {"reduce_sum": 0, "reduce_mean": 1, "reduce_max": 2}[entry]
        y = strided_out(n, f, f + pad, device=DEV)
        cnt = strided_out(n, f, f + pad, dtype=torch.int32, device=DEV) if mode == 2 else None
        _lib.check(L.dc_edge_reduce_fwd(adj.ptr.data_ptr(), adj.perm.data_ptr(), t["m"].data_ptr(), f, y.data_ptr(), f + pad,
                                        None if cnt is None else cnt.data_ptr(), f + pad, mode, n, f, _st()), entry)
        return [y] + ([cnt] if cnt is not None else [])

    def reference(out):
        src, dst = torch.from_numpy(ei[0]), torch.from_numpy(ei[1])
        if entry == "pair":
            x = inputs["x"]
            assert torch.equal(out[0], torch.cat([x[dst], x[src] - x[dst]], dim=1))
            return
        want = nf._ref_aggregate(ei, n, lambda t: t["m"], entry[7:])({"m": inputs["m"].double()})[0]
        if entry == "reduce_max":
            assert torch.equal(out[0].double(), want)
        else:
            assert (out[0].double() - want).abs().max() <= 1e-5 * want.abs().max()
    rows = e if entry == "pair" else n
    gadd(f"d:edge-{entry}-n{n}-f{f}-ld+{pad}", run, inputs, index_inputs={"ei": n - 1}, reference=reference,
         partial=(rows, 8), slack="x")


for _entry in ("pair", "reduce_sum", "reduce_mean", "reduce_max"):
    _edge_ld_case(_entry, 259, 32, 4)
    _edge_ld_case(_entry, 67, 35, 1)


def _flash_ld_case(ns=131, nr=70, nrp=96, d=256, pad=4):
    """dc_attn_flash_fwd (``ldo = d + pad``) and the two-sweep dc_attn_flash_ds (``ldp = nr_padded + pad``) at 131 queries:
    one full 128-query tile and a ragged one of 3; the operands prepared as attention.py prepares them"""
    inputs = {"q": _frand((ns, d), 32, d ** -0.5), "k": _frand((nr, d), 33), "v": _frand((nr, d), 34),
              "go": _frand((ns, d), 35)}

    def run(t):
        from deformcontact_amd import _lib, attention
        L, st = _lib.lib(), _st()
        kp, vp = torch.zeros(nrp, d, device=DEV), torch.zeros(nrp, d, device=DEV)
        kp[:nr], vp[:nr] = t["k"], t["v"]
        kmax, kimg, _, _ = attention._prep(L, kp, False, st)
        vmax, vimg, vtimg, vtmax = attention._prep(L, vp, True, st)
        qmax, gomax = attention._rowabsmax(L, t["q"], st), attention._rowabsmax(L, t["go"], st)
        kuns, vuns = torch.empty_like(kmax), torch.empty_like(vmax)
        o, lse = strided_out(ns, d, d + pad, device=DEV), torch.empty(ns, device=DEV)
        _lib.check(L.dc_attn_flash_prep(vtimg.data_ptr(), d, nrp, kmax.data_ptr(), kuns.data_ptr(), st), "flash_prep")
        _lib.check(L.dc_attn_flash_fwd(t["q"].data_ptr(), d, qmax.data_ptr(), kimg.data_ptr(), kuns.data_ptr(),
                                       vtimg.data_ptr(), vtmax.data_ptr(), ns, nr, nrp, d, o.data_ptr(), d + pad,
                                       lse.data_ptr(), st), "flash_fwd")
        _lib.check(L.dc_attn_flash_prep(None, 0, nrp, vmax.data_ptr(), vuns.data_ptr(), st), "flash_prep")
        pm, ds = strided_out(ns, nrp, nrp + pad, device=DEV), strided_out(ns, nrp, nrp + pad, device=DEV)
        dsmax = torch.empty(ns, device=DEV)
        _lib.check(L.dc_attn_flash_ds(t["q"].data_ptr(), d, qmax.data_ptr(), t["go"].data_ptr(), d, gomax.data_ptr(),
                                      kimg.data_ptr(), kuns.data_ptr(), vimg.data_ptr(), vuns.data_ptr(), lse.data_ptr(),
                                      ns, nr, nrp, d, pm.data_ptr(), ds.data_ptr(), nrp + pad, dsmax.data_ptr(), None, None,
                                      st), "flash_ds")
        torch.cuda.current_stream().synchronize()                 # (the prepared operands stay alive until the launches ran)
        return [o, lse, pm, ds, dsmax]

    def reference(out):
        q, k, v, go = (inputs[n].double() for n in ("q", "k", "v", "go"))
        s = q @ k.t()
        p = torch.softmax(s, dim=1)
        # the fp16x2 products are within 2e-6 of their row scale (tests/test_gpu_parity.py): |q . k| <= 16 here, so a score
        # is within 3.2e-5, a weight within 3.2e-5 relative; |go . v| <= 256, so dP is within 5.2e-4
        assert (out[0].double() - p @ v).abs().max() <= 4e-5 * float(v.abs().max())
        assert (out[1].double() - torch.logsumexp(s, dim=1)).abs().max() <= 4e-5
        assert (out[2][:, :nr].double() - p).abs().max() <= 4e-5 and not out[2][:, nr:].any()
        dp = go @ v.t()
        want = p * (dp - (p * dp).sum(1, keepdim=True))
        assert (out[3][:, :nr].double() - want).abs().max() <= 6e-4 and not out[3][:, nr:].any()
        assert torch.equal(out[4], out[3].abs().amax(1))
    gadd(f"d:attn-flash-{ns}x{nr}of{nrp}-ld+{pad}", run, inputs, reference=reference, partial=(ns, 128), slack="q")


_flash_ld_case()


def _grouped_ld_case(k=64, fo=72, pad=4):
    """dc_tag_grouped_fwd_h2p: two groups (67 and 259 rows, each starting at a multiple of 256 rows of a merged space of
    768) with their own weights in one launch, ``ldo = Fo + pad``; the rows between the groups are padding"""
    row_beg, rows, total = (0, 256), (67, 259), 768
    x = torch.zeros(total, k)
    for g, (r0, r) in enumerate(zip(row_beg, rows)):
        x[r0:r0 + r] = _frand((r, k), 36 + g)
    inputs = {"x": x, "w": _frand((2, fo, k), 38, k ** -0.5), "b": _frand((2, fo), 39, 0.5)}

    def run(t):
        from deformcontact_amd import _lib, ops
        from deformcontact_amd.ops import _i64_array, _ptr_array, _vp_array
        L, st = _lib.lib(), _st()
        wmax, wimg = torch.empty(2, fo, device=DEV), torch.empty(2, fo, k, device=DEV)
        wmax_p, wimg_p = _ptr_array(list(wmax)), _ptr_array(list(wimg))
        _lib.check(L.dc_tag_grouped_weight_prep(_ptr_array([t["w"][0], t["w"][1]]), 2, 1, fo, k, wmax_p, wimg_p, None, None,
                                                st), "grouped_weight_prep")
        xmax = ops.rowabsmax(t["x"])
        out = strided_out(total, fo, fo + pad, device=DEV)
        _lib.check(L.dc_tag_grouped_fwd_h2p(t["x"].data_ptr(), k, 2, _i64_array(row_beg), _i64_array(rows), total, wimg_p,
                                            _vp_array([t["b"][0].data_ptr(), t["b"][1].data_ptr()]), 1, out.data_ptr(),
                                            fo + pad, k, fo, xmax.data_ptr(), wmax_p, st), "grouped_fwd_h2p")
        torch.cuda.current_stream().synchronize()
        return [out[r0:r0 + r] for r0, r in zip(row_beg, rows)]    # (the padding rows belong to nobody)

    def reference(out):
        for g, (r0, r) in enumerate(zip(row_beg, rows)):
            want = (x[r0:r0 + r].double() @ inputs["w"][g].double().t() + inputs["b"][g].double()).clamp_min(0)
            assert (out[g].double() - want).abs().max() <= 2e-6 * want.abs().max(), g
    gadd(f"d:dense-grouped_fwd_h2p-{k}x{fo}-ld+{pad}", run, inputs, reference=reference, partial=(67, 64), slack="x")


_grouped_ld_case()


def _pointnet_pair_ld_case(n, f, pad, loops):
    """dc_pointnet_pair_fwd: z[q] = [x_j, pos_j - pos_i] per edge row (with ``loops`` the N appended loop rows), ``ldz = F +
    3 + pad``"""
    ei = nf.GRAPHS[n]
    e = ei.shape[1]
    inputs = {"x": _frand((n, f), 40), "pos": _frand((n, 3), 41), "ei": torch.from_numpy(ei)}

    def run(t):
        from deformcontact_amd import _lib
        rows, ld = e + (n if loops else 0), f + 3 + pad
        z = strided_out(rows, f + 3, ld, device=DEV)
        _lib.check(_lib.lib().dc_pointnet_pair_fwd(t["ei"][0].data_ptr(), t["ei"][1].data_ptr(), t["x"].data_ptr(), f,
                                                   t["pos"].data_ptr(), 3, t["pos"].data_ptr(), 3, z.data_ptr(), ld, n, n, e,
                                                   f, int(loops), 0, _st()), "pointnet_pair_fwd")
        return [z]

    def reference(out):
        src, dst = torch.from_numpy(ei[0]), torch.from_numpy(ei[1])
        x, pos = inputs["x"], inputs["pos"]
        want = torch.cat([x[src], pos[src] - pos[dst]], dim=1)
        if loops:
            keep = (src != dst).unsqueeze(1)                       # (an input self loop takes no part: its row is not judged)
            assert torch.equal(out[0][:e] * keep, want * keep)
            assert torch.equal(out[0][e:], torch.cat([x, torch.zeros(n, 3)], dim=1))
        else:
            assert torch.equal(out[0], want)
    gadd(f"d:pointnet-pair-n{n}-f{f}-loops{int(loops)}-ld+{pad}", run, inputs, index_inputs={"ei": n - 1},
         reference=reference, partial=(e + (n if loops else 0), 8), slack="x")


_pointnet_pair_ld_case(259, 32, 4, False)
_pointnet_pair_ld_case(67, 35, 1, True)


def _bwd_ld_case(entry, n, f, pad):
    """the backward entries of the layers with a gradient leading dimension ``ld = width + pad``: dc_edge_pair_bwd,
    dc_edge_reduce_bwd and dc_pointnet_reduce_bwd (sum / mean / max, the max on the outputs of a forward launch),
    dc_gine_bwd_x, dc_gine_bwd_e, dc_pool_bwd"""
    ei = nf.GRAPHS[n]
    e = ei.shape[1]
    g = nf._raw_graph(ei, n)
    sizes = (1, 37, 0, n - 38)
    kind, _, mode_name = entry.partition("-")
    mode = {"sum": 0, "add": 0, "mean": 1, "max": 2}.get(mode_name, 0)
    rng = np.random.default_rng(n + f + len(entry))

    def grid(rows, cols):
        return torch.from_numpy(rng.integers(-8, 9, (rows, cols)).astype(np.float32) / 4)
    inputs = {"ei": torch.from_numpy(ei), "x": grid(n, f) if mode == 2 else _frand((n, f), 42),
              "m": grid(e, f) if mode == 2 else _frand((e, f), 43), "gy": _frand((n, f), 44), "gz": _frand((e, 2 * f), 45),
              "gyb": _frand((len(sizes), f), 46)}

    def run(t):
        from deformcontact_amd import _lib
        L, st, gi = _lib.lib(), _st(), g()
        src, dst = t["ei"][0].data_ptr(), t["ei"][1].data_ptr()
        if kind == "edge_pair_bwd":
            gx = strided_out(n, f, f + pad, device=DEV)
            rc = L.dc_edge_pair_bwd(gi.fwd.ptr.data_ptr(), gi.fwd.perm.data_ptr(), gi.bwd.ptr.data_ptr(),
                                    gi.bwd.perm.data_ptr(), t["gz"].data_ptr(), 2 * f, gx.data_ptr(), f + pad, n, f, st)
            out = [gx]
        elif kind in ("edge_reduce_bwd", "pointnet_reduce_bwd"):
            y = cnt = None
            if mode == 2:                                          # the forward's maximum and tie counts, contiguous
                y, cnt = torch.empty(n, f, device=DEV), torch.empty(n, f, dtype=torch.int32, device=DEV)
                _lib.check(L.dc_edge_reduce_fwd(gi.fwd.ptr.data_ptr(), gi.fwd.perm.data_ptr(), t["m"].data_ptr(), f,
                                                y.data_ptr(), f, cnt.data_ptr(), f, 2, n, f, st), "edge_reduce_fwd")
            gm = strided_out(e, f, f + pad, device=DEV)
            head = (src, dst, gi.fwd.ptr.data_ptr(), t["m"].data_ptr() if mode == 2 else None, f,
                    y.data_ptr() if mode == 2 else None, f, cnt.data_ptr() if mode == 2 else None, f, t["gy"].data_ptr(), f,
                    gm.data_ptr(), f + pad, mode)
            if kind == "edge_reduce_bwd":
                rc = L.dc_edge_reduce_bwd(*head, n, e, f, st)
            else:
                rc = L.dc_pointnet_reduce_bwd(*head, n, n, e, f, 0, st)
            out = [gm]
        elif kind == "gine_bwd_x":
            gx = strided_out(n, f, f + pad, device=DEV)
            rc = L.dc_gine_bwd_x(gi.bwd.ptr.data_ptr(), gi.bwd.other.data_ptr(), gi.bwd.perm.data_ptr(), t["x"].data_ptr(), f,
                                 t["m"].data_ptr(), f, None, t["gy"].data_ptr(), f, gx.data_ptr(), f + pad, n, f, st)
            out = [gx]
        elif kind == "gine_bwd_e":
            ge = strided_out(e, f, f + pad, device=DEV)
            rc = L.dc_gine_bwd_e(src, dst, t["x"].data_ptr(), f, t["m"].data_ptr(), f, t["gy"].data_ptr(), f, ge.data_ptr(),
                                 f + pad, n, e, f, st)
            out = [ge]
        else:                                                      # pool_bwd
            nb = len(sizes)
            ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64).to(DEV)
            batch = _batch_ids(sizes).to(DEV)
            y = cnt = None
            if mode == 2:
                y, cnt = torch.empty(nb, f, device=DEV), torch.empty(nb, f, dtype=torch.int32, device=DEV)
                _lib.check(L.dc_pool_fwd(ptr.data_ptr(), t["x"].data_ptr(), f, y.data_ptr(), f, cnt.data_ptr(), f, 2, n, nb, f,
                                         st), "pool_fwd")
            gx = strided_out(n, f, f + pad, device=DEV)
            rc = L.dc_pool_bwd(batch.data_ptr(), ptr.data_ptr(), t["x"].data_ptr() if mode == 2 else None, f,
                               y.data_ptr() if mode == 2 else None, f, cnt.data_ptr() if mode == 2 else None, f,
                               t["gyb"].data_ptr(), f, gx.data_ptr(), f + pad, mode, n, nb, f, st)
            out = [gx]
        _lib.check(rc, entry)
        torch.cuda.current_stream().synchronize()
        return out

    def reference(out):
        """float64 autograd of the float64 restatement of the forward; a maximum splits evenly among its ties"""
        src, dst = torch.from_numpy(ei[0]), torch.from_numpy(ei[1])
        t64 = {k: v.double() for k, v in inputs.items() if k != "ei"}
        if kind == "edge_pair_bwd":
            x = torch.zeros(n, f, dtype=torch.float64, requires_grad=True)
            z = torch.cat([x[dst], x[src] - x[dst]], dim=1)
            (want,) = torch.autograd.grad(z, x, t64["gz"])
        elif kind in ("edge_reduce_bwd", "pointnet_reduce_bwd"):
            m = t64["m"]
            deg = torch.bincount(dst, minlength=n).clamp(min=1).double().unsqueeze(1)
            if mode == 2:
                hit = m == nf.ref_amax(dst, m, n)[dst]
                cnt = torch.zeros(n, f, dtype=torch.float64).index_add_(0, dst, hit.double())
                want = torch.where(hit, t64["gy"][dst] / cnt[dst].clamp(min=1), torch.zeros_like(m))
            else:
                want = t64["gy"][dst] / deg[dst] if mode == 1 else t64["gy"][dst]
        elif kind.startswith("gine"):
            on = ((inputs["x"][src] + inputs["m"]) > 0).double()   # (the mask from the same fp32 add as the forward)
            ge = on * t64["gy"][dst]
            want = ge if kind == "gine_bwd_e" else torch.zeros(n, f, dtype=torch.float64).index_add_(0, src, ge)
        else:
            b = _batch_ids(sizes)
            rows = torch.tensor(sizes).clamp(min=1).double().unsqueeze(1)
            if mode == 2:
                hit = t64["x"] == nf.ref_amax(b, t64["x"], len(sizes))[b]
                cnt = torch.zeros(len(sizes), f, dtype=torch.float64).index_add_(0, b, hit.double())
                want = torch.where(hit, t64["gyb"][b] / cnt[b].clamp(min=1), torch.zeros_like(t64["x"]))
            else:
                want = t64["gyb"][b] / rows[b] if mode == 1 else t64["gyb"][b]
        assert (out[0].double() - want).abs().max() <= 1e-5 * want.abs().max(), entry
    rows = e if kind in ("edge_reduce_bwd", "pointnet_reduce_bwd", "gine_bwd_e") else n
    gadd(f"d:layer-{entry}-n{n}-f{f}-ld+{pad}", run, inputs, index_inputs={"ei": n - 1}, reference=reference,
         partial=(rows, 8), slack="gy")


for _entry in ("edge_pair_bwd", "edge_reduce_bwd-sum", "edge_reduce_bwd-mean", "edge_reduce_bwd-max",
               "pointnet_reduce_bwd-sum", "pointnet_reduce_bwd-mean", "pointnet_reduce_bwd-max", "gine_bwd_x", "gine_bwd_e",
               "pool_bwd-add", "pool_bwd-mean", "pool_bwd-max"):
    _bwd_ld_case(_entry, 259, 32, 4)
    _bwd_ld_case(_entry, 67, 35, 1)


def _heads_ld_case(n, nh, c, pad):
    """dc_spmm_f32_heads_bias_act: y[i, h C + j] = relu(sum_p alpha[p, h] x[other[p], h C + j] + bias), ``ldy = H C + pad``"""
    ei = nf.GRAPHS[n]
    e = ei.shape[1]
    g = nf._raw_graph(ei, n)
    ptr, other, _ = nf.cpu_csr(ei, n)
    gen = torch.Generator().manual_seed(n + nh + c)
    inputs = {"x": _frand((n, nh * c), 47), "alpha": torch.rand(e, nh, generator=gen) + 0.1, "b": _frand((nh * c,), 48, 0.5)}

    def run(t):
        from deformcontact_amd import _lib
        adj, w = g().fwd, nh * c
        y = strided_out(n, w, w + pad, device=DEV)
        _lib.check(_lib.lib().dc_spmm_f32_heads_bias_act(adj.ptr.data_ptr(), adj.other.data_ptr(), t["alpha"].data_ptr(),
                                                         t["x"].data_ptr(), w, t["b"].data_ptr(), 1, 0, y.data_ptr(), w + pad,
                                                         n, nh, c, _st()), "heads_bias_act")
        return [y]

    def reference(out):
        sorted_ei = np.stack([other, np.repeat(np.arange(n), np.diff(ptr))])
        x, a = inputs["x"].double(), inputs["alpha"].double()
        want = torch.cat([nf.ref_spmm(sorted_ei, a[:, h], x[:, h * c:(h + 1) * c]) for h in range(nh)], dim=1)
        want = (want + inputs["b"].double()).clamp_min(0)
        assert (out[0].double() - want).abs().max() <= 1e-5 * want.abs().max()
    gadd(f"d:spmm-heads_bias_act-n{n}-h{nh}-c{c}-ld+{pad}", run, inputs, reference=reference, partial=(n, 8), slack="x")


_heads_ld_case(259, 3, 64, 4)
_heads_ld_case(67, 3, 7, 1)


def _pack_wprep_ld_case(n, f, pad):
    """dc_spmm_f32_pack_wprep with ``lds = wpad + pad``: the slab as dc_spmm_f32_pack writes it and the weight image"""
    ei, nseg, wpad = nf.GRAPHS[n], 4, 96
    width = nseg * f
    g, w = nf._lazy(lambda: nf._graph(ei, n)), nf.gcn_weights(ei, n)[1]
    inputs = {"x": _frand((n, f), 49)}

    def run(t):
        from deformcontact_amd import _lib
        from deformcontact_amd.ops import _ptr_array
        from tests.test_narrow_prepared import _image_buffer, _weights
        adj = g().fwd
        ws = _weights(f, nseg, "contiguous", torch.Generator().manual_seed(f))
        buf = _image_buffer(wpad)
        slab = strided_out(n, wpad, wpad + pad, device=DEV)
        slab[:, 2 * f:width] = 7.0                                # blocks 2..K belong to the later hops
        _lib.check(_lib.lib().dc_spmm_f32_pack_wprep(adj.ptr.data_ptr(), adj.other.data_ptr(), adj.w.data_ptr(),
                                                     t["x"].data_ptr(), f, slab.data_ptr(), wpad + pad, n, f, width, wpad,
                                                     _ptr_array(ws), nseg, buf.data_ptr(), _st()), "pack_wprep")
        torch.cuda.current_stream().synchronize()
        return [slab, buf]

    def reference(out):
        from tests.test_narrow_prepared import _check_image, _weights
        assert torch.equal(out[0][:, :f], inputs["x"]) and (out[0][:, 2 * f:width] == 7.0).all()
        assert not out[0][:, width:].any()
        hop = nf.ref_spmm(ei, w, inputs["x"].double())
        assert (out[0][:, f:2 * f].double() - hop).abs().max() <= 1e-5 * hop.abs().max()
        _check_image(out[1], [v.cpu() for v in _weights(f, nseg, "contiguous", torch.Generator().manual_seed(f))], f, nseg, wpad)
    gadd(f"d:spmm-pack_wprep-n{n}-f{f}-ld+{pad}", run, inputs, reference=reference, partial=(n, 8), slack="x")


_pack_wprep_ld_case(259, 21, 4)


def _pack_input_ld_case(n, f, pad):
    """dc_tag_pack_input with ``ld_slab = wpad + pad``: slab[:, :F] = x, slab[:, width:wpad] = 0, the rest untouched"""
    width, wpad = 4 * f, 96
    inputs = {"x": _frand((n, f), 50)}

    def run(t):
        from deformcontact_amd import _lib
        slab = strided_out(n, wpad, wpad + pad, device=DEV)
        slab[:, f:width] = 7.0
        _lib.check(_lib.lib().dc_tag_pack_input(t["x"].data_ptr(), f, slab.data_ptr(), wpad + pad, n, f, width, wpad, _st()),
                   "pack_input")
        return [slab]

    def reference(out):
        assert torch.equal(out[0][:, :f], inputs["x"]) and (out[0][:, f:width] == 7.0).all() and not out[0][:, width:].any()
    gadd(f"d:dense-pack_input-n{n}-f{f}-ld+{pad}", run, inputs, reference=reference, partial=(n, 64), slack="x")


_pack_input_ld_case(259, 21, 4)
_pack_input_ld_case(67, 21, 1)


def _mask_grad_bf16_ld_case(n, f, pad):
    """dc_tag_mask_grad_bf16: gm = bf16(g * (out > 0)) from fp32 operands, ``ldgm = F + pad``"""
    inputs = {"g": _frand((n, f), 51), "y": _frand((n, f), 52)}

    def run(t):
        from deformcontact_amd import _lib
        gm = strided_out(n, f, f + pad, dtype=torch.bfloat16, device=DEV)
        _lib.check(_lib.lib().dc_tag_mask_grad_bf16(t["g"].data_ptr(), f, 0, t["y"].data_ptr(), f, 0, gm.data_ptr(), f + pad,
                                                    n, f, _st()), "mask_grad_bf16")
        return [gm]

    def reference(out):
        want = (inputs["g"] * (inputs["y"] > 0)).double()
        assert ((out[0].double() - want).abs() <= 2.0 ** -8 * want.abs()).all()      # one rounding to bf16
    gadd(f"d:dense-mask_grad_bf16-n{n}-f{f}-ld+{pad}", run, inputs, reference=reference, partial=(n, 64), slack="g")


_mask_grad_bf16_ld_case(259, 64, 8)


def _grouped_mask_grad_ld_case(f=64, pad=4):
    """dc_tag_grouped_mask_grad: gm = g * (out > 0) for two groups (67 and 259 rows of a merged space of 768) into a
    slab block with ``ldgm = F + pad``, and the groups' row maxima"""
    row_beg, rows, total = (0, 256), (67, 259), 768
    inputs = {"g0": _frand((67, f), 53), "g1": _frand((259, f), 54), "y": _frand((total, f), 55)}

    def run(t):
        from deformcontact_amd import _lib
        from deformcontact_amd.ops import _i64_array, _ptr_array
        gm, rm = strided_out(total, f, f + pad, device=DEV), torch.empty(total, device=DEV)
        _lib.check(_lib.lib().dc_tag_grouped_mask_grad(_ptr_array([t["g0"], t["g1"]]), _i64_array([f, f]), 2,
                                                       _i64_array(row_beg), _i64_array(rows), total, t["y"].data_ptr(), f,
                                                       gm.data_ptr(), f + pad, f, rm.data_ptr(), None, _st()),
                   "grouped_mask_grad")
        return [v[r0:r0 + r] for v in (gm, rm) for r0, r in zip(row_beg, rows)]   # (the padding rows belong to nobody)

    def reference(out):
        for j, (r0, r) in enumerate(zip(row_beg, rows)):
            want = inputs[f"g{j}"] * (inputs["y"][r0:r0 + r] > 0)
            assert torch.equal(out[j], want) and torch.equal(out[2 + j], want.abs().amax(1))
    gadd(f"d:dense-grouped_mask_grad-f{f}-ld+{pad}", run, inputs, reference=reference, partial=(67, 64), slack="g0")


_grouped_mask_grad_ld_case()


def _colsum_ld_case(n, f, pad):
    """dc_mask_colsum_f32: gm = g * (y > 0) with ``ldgm = F + pad`` and the column sums"""
    inputs = {"g": _frand((n, f), 9), "y": _frand((n, f), 10)}

    def run(t):
        from deformcontact_amd import _lib
        L = _lib.lib()
        gm, gb = strided_out(n, f, f + pad, device=DEV), torch.empty(f, device=DEV)
        nb = L.dc_colsum_workspace_bytes(n, f, 1)
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
        _lib.check(L.dc_mask_colsum_f32(t["g"].data_ptr(), f, t["y"].data_ptr(), f, gm.data_ptr(), f + pad, n, f,
                                        ws.data_ptr(), ws.numel(), gb.data_ptr(), 0, _st()), "mask_colsum")
        return [gm, gb]

    def reference(out):
        gm = inputs["g"] * (inputs["y"] > 0)
        assert torch.equal(out[0], gm)
        s = gm.double().sum(0)
        assert (out[1].double() - s).abs().max() <= 2e-6 * max(float(gm.abs().double().sum(0).max()), 1e-30)
    gadd(f"d:mask-colsum-n{n}-f{f}-ld+{pad}", run, inputs, reference=reference, partial=(n, 64), slack="g")


_colsum_ld_case(259, 64, 4)
_colsum_ld_case(67, 32, 4)


def _attn_rows_case(rows, ncols, npad, pad, with_delta):
    """dc_attn_softmax_rows / dc_attn_exp_rows / dc_attn_ds_rows: row passes over a score block ``[rows, npad]`` with
    leading dimension ``npad + pad``, IN PLACE (include/deformcontact.h: "s" is read and written) - the block is an
    operand the entries document as written in place, so it is copied into a strided output first"""
    inputs = {"s": _frand((rows, npad), 11, 3.0), "dp": _frand((rows, npad), 12), "delta": _frand((rows,), 13)}

    def run(t):
        from deformcontact_amd import _lib
        L, ld = _lib.lib(), npad + pad
        s1, s2, dp = (strided_out(rows, npad, ld, device=DEV) for _ in range(3))
        s1.copy_(t["s"]), s2.copy_(t["s"]), dp.copy_(t["dp"])
        lse, rm = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
        _lib.check(L.dc_attn_softmax_rows(s1.data_ptr(), ld, rows, ncols, npad, lse.data_ptr(), _st()), "softmax_rows")
        _lib.check(L.dc_attn_exp_rows(s2.data_ptr(), ld, rows, ncols, npad, lse.data_ptr(), _st()), "exp_rows")
        _lib.check(L.dc_attn_ds_rows(s1.data_ptr(), dp.data_ptr(), ld, rows, npad,
                                     t["delta"].data_ptr() if with_delta else None, rm.data_ptr(), _st()), "ds_rows")
        return [s1, lse, s2, dp, rm]

    def reference(out):
        s = inputs["s"].double()[:, :ncols]
        p = torch.softmax(s, dim=1)
        assert (out[0][:, :ncols].double() - p).abs().max() <= 1e-6 and not out[0][:, ncols:].any()
        assert (out[1].double() - torch.logsumexp(s, dim=1)).abs().max() <= 1e-5
        assert (out[2][:, :ncols].double() - p).abs().max() <= 1e-6 and not out[2][:, ncols:].any()
        pk, dp = out[0].double(), inputs["dp"].double()
        delta = inputs["delta"].double() if with_delta else (pk * dp).sum(1) / pk.sum(1)
        assert (out[3].double() - pk * (dp - delta.unsqueeze(1))).abs().max() <= 1e-5
        assert torch.equal(out[4], out[3].abs().amax(1))
    gadd(f"d:attn-rows-{rows}x{ncols}of{npad}-ld+{pad}-delta{int(with_delta)}", run, inputs, reference=reference, partial=(rows, 64), slack="s")


_attn_rows_case(131, 70, 128, 4, False)                         # 16-byte rows: the register-resident kernels
_attn_rows_case(131, 70, 128, 1, True)                          # any leading dimension: the strided kernels
_attn_rows_case(33, 64, 64, 4, True)


def _adam_case(n=1027):
    """dc_adam_flat on hosted p / m / v: the three are written IN PLACE ("Memory contract": Adam's p, m,
    v), g is read-only (zero_grad = 0)"""
    gen = torch.Generator().manual_seed(5)
    inputs = {"p": torch.rand(n, generator=gen) - 0.5, "g": torch.rand(n, generator=gen) - 0.5,
              "m": (torch.rand(n, generator=gen) - 0.5) * 0.1, "v": torch.rand(n, generator=gen) * 0.01 + 1e-4}
    lr, b1, b2, eps = 4e-4, 0.9, 0.999, 1e-8

    def run(t):
        from deformcontact_amd import _lib
        step = torch.zeros(34, dtype=torch.float32, device=DEV)
        _lib.check(_lib.lib().dc_adam_flat(t["p"].data_ptr(), t["g"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), n,
                                           step.data_ptr(), lr, b1, b2, eps, 0, _st()), "adam")
        return [t["p"], t["m"], t["v"], step]

    def reference(out):
        p, g, m, v = (inputs[k].double() for k in "pgmv")
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        p = p - lr * (m / (1 - b1)) / ((v / (1 - b2)).sqrt() + eps)
        for o, r in zip(out, (p, m, v)):
            assert (o.double() - r).abs().max() <= 1e-6 * r.abs().max()
        assert out[3].tolist() == [1.0] + [0.0] * 33
    sec = "INTEGRATION.md 2, Memory contract: Adam's p / m / v"
    gadd("d:adam-in-place-n1027", run, inputs, in_place={"p": sec, "m": sec, "v": sec}, reference=reference,
         partial=(n, 1024), slack="g")


_adam_case()


# ---- end to end with the backward: every buffer an autograd Function allocates and saves is under guard ------------------
def _encoder_train_case():
    """The two-branch TAGConv encoder of graphnet.py on the h32 golden graphs, forward and backward: the outputs of both
    branches and the gradient of every parameter.  The edge indices are hosted index inputs."""
    z = nf.load_golden("graphnet_tag_h32.npz")
    x, xr = torch.from_numpy(z["rest_x"]), torch.from_numpy(z["rig_x"])
    inputs = {"x": x, "xr": xr, "ei": torch.from_numpy(z["rest_edge_index"]), "eir": torch.from_numpy(z["rig_edge_index"])}

    @nf._lazy
    def model():
        from deformcontact_amd.graphnet import ContactEncoder
        torch.manual_seed(11)
        return ContactEncoder([x.size(1), xr.size(1)], int(z["hidden"])).to(DEV)

    def run(t):
        from deformcontact_amd.deferred import resolve
        from deformcontact_amd.graph import clear_cache
        from tests.helpers import G
        clear_cache()
        enc = model()
        a, b = enc(G(t["x"], t["ei"], torch.from_numpy(z["rest_pos"]).to(DEV)),
                   G(t["xr"], t["eir"], torch.from_numpy(z["rig_pos"]).to(DEV)))
        a, b = resolve(a), resolve(b)
        params = [p for p in enc.parameters() if p.requires_grad]
        grads = torch.autograd.grad((a * a).sum() + (b * b).sum(), params, allow_unused=True)
        return [a.detach(), b.detach()] + [gr for gr in grads if gr is not None]
    gadd("e:encoder-train-h32", run, inputs, index_inputs={"ei": x.size(0) - 1, "eir": xr.size(0) - 1})


_encoder_train_case()


def _contact_loss_direct_case(n):
    """dc_contact_loss with test-owned outputs (the operator's gradient leaves through ATen: UNGUARDED["loss-"]): the two
    per-node gradient arrays, the two loss values, the workspace"""
    ei = nf.GRAPHS[n]
    g = nf._raw_graph(ei, n)
    inputs = {"pred": _frand((n, 3), 16), "tgt": _frand((n, 3), 17)}

    def run(t):
        from deformcontact_amd import _lib
        L, gi = _lib.lib(), g()
        g1, g2, out = torch.empty(n, 3, device=DEV), torch.empty(n, 3, device=DEV), torch.empty(2, device=DEV)
        nb = L.dc_contact_loss_workspace_bytes(n)
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
        _lib.check(L.dc_contact_loss(gi.fwd.ptr.data_ptr(), gi.fwd.other.data_ptr(), gi.bwd.ptr.data_ptr(),
                                     gi.bwd.other.data_ptr(), t["pred"].data_ptr(), 3, t["tgt"].data_ptr(), 3, n,
                                     gi.num_input_edges, g1.data_ptr(), g2.data_ptr(), out.data_ptr(), ws.data_ptr(), nb,
                                     _st()), "contact_loss")
        return [g1, g2, out]

    def reference(out):
        src, dst = torch.from_numpy(ei[0]), torch.from_numpy(ei[1])
        p, t = inputs["pred"].double().requires_grad_(True), inputs["tgt"].double()
        l1 = (p - t).abs().mean()
        gcl = torch.linalg.vector_norm((t[dst] - t[src]) - (p[dst] - p[src]), dim=1).mean()
        ga, gb = torch.autograd.grad(l1, p, retain_graph=True)[0], torch.autograd.grad(gcl, p)[0]
        assert (out[2].double() - torch.stack([l1, gcl]).detach()).abs().max() <= 1e-5 * float(max(l1.detach(), gcl.detach()))
        for got, want in ((out[0], ga), (out[1], gb)):
            assert (got.double() - want).abs().max() <= 1e-5 * want.abs().max()
    gadd(f"e:contact-loss-direct-n{n}", run, inputs, reference=reference)


_contact_loss_direct_case(67)
_contact_loss_direct_case(259)


# --------------------------------------------------------------------------- #
# CPU: the harness finds planted errors, and no case can pass vacuously
# --------------------------------------------------------------------------- #
@contextlib.contextmanager
def _young_process():
    """plain runs of the planted kernels see what a young process sees: ``torch.empty`` hands out zeroed pages"""
    mp = pytest.MonkeyPatch()
    zeros, zeros_like = torch.zeros, torch.zeros_like
    mp.setattr(torch, "empty", lambda *a, **k: zeros(*a, **k))
    mp.setattr(torch, "empty_like", lambda *a, **k: zeros_like(*a, **k))
    try:
        yield
    finally:
        mp.undo()


def _room(t, before=0, after=0):
    """a planted overrun happens only where it lands in memory the test owns: inside a guarded allocation"""
    store = t.untyped_storage().nbytes() // t.element_size()
    return Guard.active is not None and t.storage_offset() >= before and t.storage_offset() + t.numel() + after <= store


def _planted(kind):
    """out = 2 x, with one error of the named kind"""
    def kernel(t):
        x = t["x"]
        rows, cols = x.shape
        out = strided_out(rows, cols, cols + 3, device="cpu") if kind == "gap" else torch.empty(rows, cols)
        if kind == "unwritten":                                    # the tail element is skipped
            out.view(-1)[:-1] = (x * 2).view(-1)[:-1]
            return [out]
        out.copy_(x * 2)
        if kind == "before" and _room(out, before=1):
            torch.as_strided(out, (1,), (1,), out.storage_offset() - 1)[0] = 7.0
        if kind == "after" and _room(out, after=1):
            torch.as_strided(out, (1,), (1,), out.storage_offset() + out.numel())[0] = 7.0
        if kind == "gap" and Guard.active is not None:
            torch.as_strided(out, (1,), (1,), out.storage_offset() + cols + 1)[0] = 7.0
        if kind == "input":
            x[1, 1] += 1.0
        if kind == "slack" and _room(x, after=1):                   # the 16-byte load of the last row, unmasked
            out[-1, -1] += torch.as_strided(x, (1,), (1,), x.storage_offset() + x.numel())[0]
        return [out]
    return kernel


@pytest.mark.parametrize("kind,rule", [("none", None), ("before", 1), ("after", 1), ("gap", 1), ("input", 2),
                                       ("slack", 3), ("unwritten", 4)])
def test_the_harness_finds_planted_errors(kind, rule, monkeypatch):
    """One planted "kernel" per way of going wrong, a Python function on CPU tensors: writes one element before the
    interior, one after it, one into a gap column; modifies an input; reads one slack element into its result; leaves
    one output element unwritten.  Each trips exactly its rule; the clean kernel trips none."""
    x = torch.arange(15, dtype=torch.float32).view(3, 5) + 1
    rep = guard_rules(_planted(kind), {"x": x}, monkeypatch, device="cpu", plain=_young_process)
    rules = {r for r, _ in rep["violations"]}
    assert rules == ({rule} if rule is not None else set()), rep["violations"]
    assert rep["buffers"] >= 4 and all(rep["owned"])               # the input and the output of both guarded runs
    if kind in ("before", "after", "gap"):
        text = rep["violations"][0][1]
        side = {"before": "front band", "after": "back band", "gap": "gap columns"}[kind]
        assert side in text and ("offset -1" if kind == "before" else "offset") in text, text


def test_index_slack_is_run_with_both_valid_indices(monkeypatch):
    """A gather that reads one index past its list: with slack 0 it adds row 0, with slack N - 1 the last row; only one
    of the two is visible in the output of this kernel - the harness runs both."""
    x = torch.arange(8, dtype=torch.float32).view(4, 2)
    x[0] = 0.0                                                     # row 0 is the additive identity: slack 0 hides the read
    idx = torch.tensor([2, 1, 3])

    def kernel(t):
        i = t["idx"]
        more = torch.as_strided(i, (i.numel() + 1,), (1,), i.storage_offset()) if _room(i, after=1) else i
        out = torch.empty(1, 2)
        out[0] = t["x"][more].sum(0)
        return [out]
    rep = guard_rules(kernel, {"x": x, "idx": idx}, monkeypatch, device="cpu", index_inputs={"idx": 3}, plain=_young_process)
    assert [r for r, _ in rep["violations"]] == [3] and "N - 1" in rep["violations"][0][1], rep["violations"]


def test_guard_layout_and_fills(monkeypatch):
    """Bands: one 128-row tile at the row pitch, at least 4 KiB, a multiple of 512 bytes; NaN / 1 / the float32 NaN
    pattern; zeros / ones / full keep their meaning; an empty interior is dirty; other devices pass through."""
    assert guard_band_bytes((1000, 256), 4) == 128 * 1024 and guard_band_bytes((7,), 4) == 4096
    assert guard_band_bytes((5, 9), 4) == 4608 and guard_band_bytes((5, 9), 4) % 512 == 0
    with Guard(monkeypatch, "cpu", dirty=True, ones_for=lambda file, fn: (file, fn) == (os.path.basename(__file__), "_int_workspace")) as g:
        a, z, o, f = torch.empty(3, 5), torch.zeros((4,), dtype=torch.int32), torch.ones(2, 2), torch.full((2,), 7)
        def _int_workspace():
            return torch.empty(10, dtype=torch.uint8)
        i, h, ws = torch.empty(6, dtype=torch.int64), a.new_empty(3, dtype=torch.bfloat16), _int_workspace()
        like, meta = torch.empty_like(z), torch.empty(3, device="meta")
        lin = torch.nn.Linear(4, 3)
        assert all(t.is_contiguous() for t in (a, z, o, f, i, h, ws, like)) and a.shape == (3, 5)
        assert torch.isnan(a).all() and torch.isnan(h.float()).all() and (i == 1).all() and (like == 1).all()
        # (named by ones_for: a workspace that carries integers reads 1 in every int32 word, not 0x01010101)
        assert ws[:8].view(torch.int32).tolist() == [1, 1] and ws.tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0]
        assert not z.any() and (o == 1).all() and f.tolist() == [7, 7] and f.dtype == torch.int64
        assert meta.device.type == "meta" and lin.weight.shape == (3, 4)
        assert all(g.owns(t) for t in (a, z, o, f, i, h, ws, like, lin.weight.data)) and not g.owns(torch.arange(3))
        assert (a.data_ptr() - a.untyped_storage().data_ptr()) % 512 == 0      # the band keeps the alignment class
        g.check()
        torch.as_strided(z, (1,), (1,), z.storage_offset() + 4)[0] = 5
        with pytest.raises(AssertionError, match=r"rule 1: #1 zeros\[4\]:int32: back band changed, 1 words, first at offset 0"):
            g.check()
    with Guard(monkeypatch, "cpu", dirty=True) as g:
        assert torch.empty(8, dtype=torch.uint8).view(torch.float32).isnan().all()   # the float32 NaN pattern per 4 bytes
    assert Guard.active is None and torch.empty(3).untyped_storage().nbytes() == 12      # the factories are restored


def test_every_case_family_is_present_and_unguarded_is_small():
    """(a) is every case of tests/test_nonfinite.py, (b) every launch-site row; the UNGUARDED table is short, reasoned
    and names nothing from the training-path files."""
    assert {c[2:] for c in GCASES if c.startswith("a:")} == set(nf.CASES) and "e:encoder-train-h32" in GCASES
    assert sum(c.startswith("b:dense-") for c in GCASES) >= len(tls.DENSE_ROWS)
    assert sum(c.startswith("b:chain-") for c in GCASES) == len(tls.CHAIN_ROWS)
    for fam in ("graph-build", "graph-rebuild", "graph-build-segmented", "csr-build", "knn", "radius", "knn-nd", "fps",
                "knn_interpolate", "morton", "spline-basis", "pool"):
        assert any(c.startswith("c:" + fam) for c in GCASES), fam
    assert len(UNGUARDED) <= MAX_UNGUARDED
    import importlib
    import inspect
    for prefix, (producer, reason) in UNGUARDED.items():
        assert reason.strip() and any(c[2:].startswith(prefix) for c in GCASES), prefix
        mod, _, qual = producer.partition(":")
        fn = importlib.import_module(mod)
        for part in qual.split("."):
            fn = getattr(fn, part)
        src = inspect.getsource(fn)
        assert "data_ptr" not in src and "_lib" not in src, (prefix, "the named producer launches a kernel")


#: rows per workgroup / per tile of the kernels: 8 and 16 (segment and hop kernels: rows per wave and per workgroup, the
#: pool's 16 slots), 32 (kNN queries per workgroup, hop chain steps), 64 and 128 (dense 64 * MB, the attention query
#: tile), 256 (one row or edge per thread of a 256-thread workgroup), 1024 (Adam: 256 threads x 4)
KERNEL_ROW_TILES = (8, 16, 32, 64, 128, 256, 1024)


def test_cases_of_c_and_d_have_slack_and_a_partial_last_tile():
    for cid, c in GCASES.items():
        if cid[:2] in ("c:", "d:"):
            assert c.slack in c.inputs and c.inputs[c.slack].numel() > 0, cid    # hosted: both bands are its slack
            rows, tile = c.partial                                 # (tile: the one the case was written for)
            assert tile in KERNEL_ROW_TILES, (cid, tile)
            for t in KERNEL_ROW_TILES:                                # ragged against EVERY row tile, not a declared one
                assert rows % t != 0, (cid, "an output's rows fill whole tiles of", t, rows)
            assert c.reference is not None, cid


# --------------------------------------------------------------------------- #
# GPU
# --------------------------------------------------------------------------- #
STATS = {"cases": 0, "buffers": 0}


def _trace(fn):
    """-> (result, (launch log, launch sites whose count moved)).  The log is cleared by every ``kernel_trace(True)``, so
    a runner that traces for itself (tests/test_launch_sites.py) leaves only its last traced call in it; the site counts
    are cumulative and see every launch made while coverage is on - all of such a runner's, which switches it on."""
    from deformcontact_amd import _lib
    _lib.launch_coverage(True)
    before = _lib.launch_site_counts()
    _lib.kernel_trace(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        sites = {s: n - before.get(s, 0) for s, n in _lib.launch_site_counts().items() if n > before.get(s, 0)}
        return out, (_lib.kernel_trace_counts(), sites)
    finally:
        _lib.kernel_trace(False)
        _lib.launch_coverage(tls._coverage_default())


def _unguarded_ok(cid):
    return any(cid[2:].startswith(p) for p in UNGUARDED)


@gpu
@pytest.mark.parametrize("cid", list(GCASES))
def test_guard_bands(cid, monkeypatch):
    c = GCASES[cid]
    for k, v in c.setenv.items():
        monkeypatch.setenv(k, v)
    for k, v in c.env.items():
        from deformcontact_amd import attention
        monkeypatch.setattr(attention, k, v)
    inputs = c.inputs
    rep = guard_rules(c.run, inputs, monkeypatch, device=DEV, index_inputs=c.index_inputs, in_place=c.in_place,
                      trace=_trace, ones_for=lambda file, fn: (file, fn) in INTEGER_WORKSPACES)
    if c.reference is not None:                                    # the plain run against the suite's CPU restatement
        c.reference([o.detach().cpu() for o in rep["plain"]])
    if c.partial is not None:                                      # the declared partial tile is an output's own row count
        assert any(o.dim() >= 1 and o.size(0) == c.partial[0] for o in rep["plain"]), (c.partial, [o.shape for o in rep["plain"]])
    if c.setenv.get("DC_CSR_BUCKETS") == "1":
        assert any(k.startswith("k_bk_") for k in rep["launched"][0]), ("the bucketed kernels did not run", rep["launched"][0])
    STATS["cases"] += 1
    STATS["buffers"] += rep["buffers"]
    print(f"{cid}: {rep['buffers']} buffers guarded, outputs inside a registered buffer: {rep['owned']}")
    assert not rep["violations"], "\n".join(f"rule {r}: {t}" for r, t in rep["violations"])
    assert rep["buffers"] >= 1, "the case guards no buffer"
    assert all(rep["owned"]) or _unguarded_ok(cid), f"outputs outside every registered buffer: {rep['owned']}"
    assert not (all(rep["owned"]) and _unguarded_ok(cid)), "UNGUARDED names a case whose outputs are all guarded"
