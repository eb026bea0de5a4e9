"""``SAGEConv``: the layer, ``ops.aggregate`` and the C entries of dc_sage.hip.

The reference is this file's own restatement of the contract in INTEGRATION.md 1.5 (PyG 2.5.2 sage_conv.py):
``RefSage``, a torch CPU module evaluated in float32 (``ref32``) and float64 (``truth64``) with gradients from torch
autograd, and numpy / torch-CPU formulas for the entries called directly.

The max is written as ``m = segment max; mask = (x[j] == m[i]); cnt = scatter_sum(mask); out = scatter_sum(mask * x[j]
/ cnt)`` with ``mask`` and ``cnt`` constant: autograd then yields the library's tie rule, the EVEN split among all edges
that attain the maximum.  ``scatter_reduce_(amax)`` is deliberately not the reference: on a zero-initialised output it
counts its own initial 0 among the ties.

Inputs.  mean / sum: unrounded, x ~ N(0, 1), default-initialised parameters.  max: the selection has to be the same in
every evaluation or the gradients differ by whole terms, so x comes from a coarse grid - multiples of 0.25 in [-2, 2],
about a third exact zeros: ties between distinct sources and through duplicate edges are certain - and with
``project=True`` ``lin``'s weight and bias are multiples of 1/8 in [-1, 1]: a projected value is a sum of at most 65
multiples of 1/32 below 2^8, an exact float32 in any order and in the dense block's split products (asserted on the
device before the layer is compared: ``test_projected_sources_are_exact``).

Metrics.  The layer through ``helpers.assert_parity`` at 1e-5 (nothing registered ``special``).  One combination of
the cross, ``normalize=True`` with a single output channel, has a constant output (+-1) and gradients that are all
mathematically zero: they are held to 1e-5 of the scale of the terms that cancel (``_zero_gradient_scale``).  The entries: the mean
forward bit-identical to the unweighted hop divided by the in-degree, m and cnt equal element for element, the two
backward entries within 1e-5 of float64 per row (``row_rel_err``: short sums of exactly weighted terms).

The adjacencies are built WITHOUT self-loop handling: ``seg_graph`` of ``seg_lens`` gives in-degrees 0, 1, 6, ... and
the hub, ``random_multigraph`` keeps its self loops, duplicates and isolated nodes.
"""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import deformcontact_amd as dc
from deformcontact_amd import _lib, ops
from deformcontact_amd.graph import GraphIndex, clear_cache
from deformcontact_amd.nn import SAGEConv  # noqa: F401  (the module needs the layer: no test runs without it)
from oracle import pyg_ref
from tests.helpers import assert_parity, load_golden, random_multigraph, record_parity, rel_err, row_rel_err
from tests.test_gat_edge_kernels import HUB, _dev, _np, seg_graph, seg_lens

gpu = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5

#: (in, out) of the layer tests
SHAPES = [(21, 64), (25, 256), (64, 20), (16, 1)]
AGGRS = ["mean", "max", "sum"]
MAIN_GRAPHS = ["multigraph", "hub", "golden_rest"]
EDGE_GRAPHS = ["n1", "e0", "n0", "golden_rig"]
#: layer options beside the default (normalize=False, root_weight=True, project=False, bias=True, relu=False)
VARIANTS = {"default": {}, "noroot": dict(root_weight=False), "project": dict(project=True),
            "normalize": dict(normalize=True), "nobias": dict(bias=False), "relu": dict(relu=True)}
#: widths of the direct tests: the general form (1, 3, 70: lane groups of 4, 4, 64) and the 16-byte form (20, 64, 256,
#: 1100: groups of 8, 16, 64, and 64 lanes over five column chunks)
WIDTHS = [1, 3, 20, 64, 70, 256, 1100]
DIRECT_GRAPHS = ["seg", "multigraph"]


# --------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------- #
def grid_values(rng, shape):
    """multiples of 0.25 in [-2, 2], about a third of them exact zeros"""
    v = rng.integers(-8, 9, shape) / 4.0
    v[rng.random(shape) < 1.0 / 3.0] = 0.0
    return v.astype(np.float32)


def grid_weights(rng, shape):
    """multiples of 1/8 in [-1, 1]"""
    return (rng.integers(-8, 9, shape) / 8.0).astype(np.float32)


def _graph(kind, seed):
    """(n, edge_index [2, E] int64)"""
    if kind == "multigraph":
        return 300, random_multigraph(300, 2400, seed)          # self loops, duplicates, 30 nodes without in-edges
    if kind == "hub":
        return 300, seg_graph(seg_lens(300, HUB), seed)         # one segment of HUB - 1 edges, in-degree-0 rows
    if kind == "seg":
        return 131, seg_graph(seg_lens(131, HUB), seed)         # in-degrees 0, 1, 6, 7, 8, 14, ..., 64 and the hub
    if kind == "n1":
        return 1, np.zeros((2, 0), np.int64)                    # one node with no edge
    if kind == "e0":
        return 50, np.zeros((2, 0), np.int64)
    if kind == "n0":
        return 0, np.zeros((2, 0), np.int64)
    z = load_golden("graphnet_gat_h32.npz")
    key = "rest" if kind == "golden_rest" else "rig"
    return z[key + "_x"].shape[0], z[key + "_edge_index"].astype(np.int64)


def host_adjacency(n, ei):
    """(ptr, other, dst) by destination, stable.  Every reference below is independent of the order inside a segment."""
    order = np.argsort(ei[1], kind="stable")
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(ei[1], minlength=n), out=ptr[1:])
    return ptr, ei[0][order], ei[1][order]


def seg_max(vals, ptr):
    """per-segment maximum of the destination-sorted rows ``vals`` [E, F]; a row without edges is 0"""
    out = np.zeros((len(ptr) - 1, vals.shape[1]), vals.dtype)
    full = np.flatnonzero(np.diff(ptr) > 0)                     # (their starts increase strictly: each reduction ends where
    if full.size:                                               # the next non-empty segment begins, the last at E)
        out[full] = np.maximum.reduceat(vals, ptr[:-1][full], axis=0)
    return out


def _index_add(n, idx, terms):
    return torch.zeros((n, terms.shape[1]), dtype=torch.float64).index_add_(
        0, torch.from_numpy(idx), torch.from_numpy(np.ascontiguousarray(terms, np.float64))).numpy()


def mean_bwd_ref(ptr, other, dst, gy):
    """float64: g_x[j] = sum over the edges j -> i of g_y[i] / deg_i"""
    deg = np.diff(ptr).astype(np.float64)
    return _index_add(len(ptr) - 1, other, gy.astype(np.float64)[dst] / deg[dst][:, None])


def max_fwd_ref(ptr, other, dst, x):
    """(m, cnt): exact in any dtype - m is one of the gathered values, cnt counts equalities"""
    n = len(ptr) - 1
    m = seg_max(x[other], ptr)
    hit = x[other] == m[dst]
    cnt = np.zeros((n, x.shape[1]), np.int64)
    np.add.at(cnt, dst, hit)
    return m, cnt.astype(np.int32)


def max_bwd_ref(ptr, other, dst, x, m, cnt, gm):
    """float64: g_x[j] = sum over the edges j -> i of (x[j] == m[i]) g_m[i] / cnt[i]: the hand-written formula"""
    hit = x[other] == m[dst]
    share = gm.astype(np.float64)[dst] / np.maximum(cnt[dst], 1)
    return _index_add(len(ptr) - 1, other, np.where(hit, share, 0.0))


@functools.lru_cache(maxsize=None)
def direct_case(kind, f, values):
    """adjacency, inputs and references of one direct case (computed once, never modified)"""
    n, ei = _graph(kind, 9)
    ptr, other, dst = host_adjacency(n, ei)
    rng = np.random.default_rng(1000 + f + len(kind))
    x = grid_values(rng, (n, f)) if values == "grid" else rng.standard_normal((n, f)).astype(np.float32)
    gup = (rng.uniform(0.5, 1.5, (n, f)) * np.where(rng.random((n, f)) < 0.5, -1.0, 1.0)).astype(np.float32)
    m, cnt = max_fwd_ref(ptr, other, dst, x)
    return dict(n=n, ei=ei, ptr=ptr, other=other, dst=dst, x=x, gup=gup, m=m, cnt=cnt,
                mean_bwd=mean_bwd_ref(ptr, other, dst, gup), max_bwd=max_bwd_ref(ptr, other, dst, x, m, cnt, gup))


# --------------------------------------------------------------------------- #
# the restatement as a torch module (float32: ref32, .double(): truth64)
# --------------------------------------------------------------------------- #
def ref_max(src, j, i, n):
    """the masked formula: mask and cnt are constants, autograd gives every attaining edge 1 / cnt of the gradient"""
    with torch.no_grad():
        order = torch.argsort(i, stable=True)
        ptr = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(i.numpy(), minlength=n), out=ptr[1:])
        m = torch.from_numpy(seg_max(src[j[order]].numpy(), ptr))
        mask = (src[j] == m[i]).to(src.dtype)
        cnt = pyg_ref.scatter_sum(mask, i, n)
    return pyg_ref.scatter_sum(mask * src[j] / cnt[i].clamp(min=1), i, n)


class RefSage(nn.Module):
    def __init__(self, fi, fo, aggr="mean", normalize=False, root_weight=True, project=False, bias=True):
        super().__init__()
        self.aggr, self.normalize = aggr, normalize
        if project:
            self.lin = nn.Linear(fi, fi)                         # (nn.Linear's default: U(+-1/sqrt(in)), weight and bias)
        self.lin_l = nn.Linear(fi, fo, bias=bias)
        if root_weight:
            self.lin_r = nn.Linear(fi, fo, bias=False)

    def sources(self, x):
        return torch.relu(self.lin(x)) if hasattr(self, "lin") else x

    def aggregate(self, src, edge_index):
        n, (j, i) = src.size(0), edge_index
        if self.aggr == "max":
            return ref_max(src, j, i, n)
        s = pyg_ref.scatter_sum(src[j], i, n)
        if self.aggr == "mean":
            s = s / torch.bincount(i, minlength=n).clamp(min=1).to(src.dtype).unsqueeze(-1)
        return s

    def forward(self, x, edge_index, relu=False):
        out = self.lin_l(self.aggregate(self.sources(x), edge_index))
        if hasattr(self, "lin_r"):
            out = out + self.lin_r(x)
        if self.normalize:
            out = F.normalize(out, p=2.0, dim=-1)
        return torch.relu(out) if relu else out


def _ref_run(mod, x, ei, gup, relu, dtype):
    for p in mod.parameters():
        p.grad = None
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    out = mod(xt, torch.from_numpy(ei), relu=relu)
    (out * torch.from_numpy(gup).to(dtype)).sum().backward()
    grads = {n: p.grad.detach().numpy().copy() for n, p in mod.named_parameters()}
    return out.detach().numpy(), xt.grad.numpy(), grads


@functools.lru_cache(maxsize=None)
def layer_case(fi, fo, aggr, kind, variant):
    """inputs, the reference module and its float32 / float64 results of one layer case"""
    torch.set_num_threads(1)
    opts = dict(VARIANTS[variant])
    relu = opts.pop("relu", False)
    n, ei = _graph(kind, 3)
    rng = np.random.default_rng(fi + fo)
    x = grid_values(rng, (n, fi)) if aggr == "max" else rng.standard_normal((n, fi)).astype(np.float32)
    gup = rng.uniform(0.5, 1.5, (n, fo)).astype(np.float32)
    torch.manual_seed(12)
    cpu = RefSage(fi, fo, aggr=aggr, **opts)                     # default initialisation
    if aggr == "max" and opts.get("project"):
        with torch.no_grad():
            cpu.lin.weight.copy_(torch.from_numpy(grid_weights(rng, (fi, fi))))
            cpu.lin.bias.copy_(torch.from_numpy(grid_weights(rng, (fi,))))
    if fo == 1 and kind == "hub" and aggr != "max":
        # a single output channel is ONE dot product per row, and the hub's terms are sums over 5,000 edges: lin_l's
        # weights take the signs of the hub's aggregated columns, so that by construction - whatever was drawn - that
        # dot product is a sum of positive terms and the comparison measures the layer, not a cancellation
        with torch.no_grad():
            agg = cpu.aggregate(cpu.sources(torch.from_numpy(x)), torch.from_numpy(ei))[n // 2]
            cpu.lin_l.weight.copy_(cpu.lin_l.weight.abs() * torch.where(agg < 0, -1.0, 1.0))
    r32 = _ref_run(cpu, x, ei, gup, relu, torch.float32)
    r64 = _ref_run(copy.deepcopy(cpu).double(), x, ei, gup, relu, torch.float64)
    return dict(n=n, ei=ei, x=x, gup=gup, cpu=cpu, relu=relu, opts=opts, r32=r32, r64=r64,
                zero_scale=_zero_gradient_scale(cpu, x, ei, gup, relu) if opts.get("normalize") and fo == 1 else None)


def _zero_gradient_scale(cpu, x, ei, gup, relu):
    """``normalize=True`` with ONE output channel: the output is ``pre / |pre|`` = +-1, a constant, and EVERY gradient
    is mathematically zero - ``g / |pre| - (g pre) pre / |pre|^3`` cancels to rounding noise in front of the linears.
    What an evaluation returns has no scale of its own to be compared on; the scale of the two terms that cancel is the
    gradient the layer WITHOUT the normalisation has for the upstream gradient ``g / |pre|``, and the noise is held to
    the same 1e-5 of that (as ``key_bias_mass`` of tests/test_transformer_conv.py).  -> {name: max |gradient|}"""
    mod = copy.deepcopy(cpu).double()
    mod.normalize = False
    with torch.no_grad():
        pre = mod(torch.from_numpy(x).double(), torch.from_numpy(ei), relu=False).numpy()
    up = gup.astype(np.float64) / np.abs(pre)
    _, gx, grads = _ref_run(mod, x, ei, up.astype(np.float64), False, torch.float64)
    scale = {"x.grad": float(np.abs(gx).max())}
    scale.update({name + ".grad": float(np.abs(g).max()) for name, g in grads.items()})
    assert all(v > 0 for v in scale.values())
    return scale


def check_against_references(tag, got, case, side):
    """output and gradients of one evaluation (``side``: "e_o" the float32 restatement against float64, "e_h" the
    device) against the references at 1e-5; the gradients of a case with ``zero_scale`` on that scale"""
    for name, a, a32, a64 in _pairs(got, case["r32"], case["r64"]):
        if case["zero_scale"] is not None and name != "forward":
            d = float(np.abs(np.asarray(a, np.float64)).max()) / case["zero_scale"][name]
            record_parity(f"{tag} {name} (mathematically zero) over the scale of its terms", None,
                          metric="abs_over_term_scale", **{side: d})
            assert d < TOL, (tag, name, d)
            assert float(np.abs(a64).max()) / case["zero_scale"][name] < 1e-12      # float64: the gradient IS zero
        elif side == "e_o":
            d = rel_err(a32, a64)
            record_parity(f"{tag} {name}", None, e_o=d)
            assert d < TOL, (tag, name, d)
        else:
            assert_parity(a, a32, a64, TOL, f"{tag} {name}")


def _layer_cases():
    cases = [(s, a, kind, v) for s in SHAPES for a in AGGRS for kind in MAIN_GRAPHS for v in VARIANTS]
    cases += [(s, a, kind, "default") for s in SHAPES for a in AGGRS for kind in EDGE_GRAPHS]
    return cases


def _pairs(got, r32, r64):
    """(name, got, ref32, truth64) over the output, x.grad and every parameter gradient"""
    out = [("forward", got[0], r32[0], r64[0]), ("x.grad", got[1], r32[1], r64[1])]
    return out + [(name + ".grad", got[2][name], r32[2][name], r64[2][name]) for name in r32[2]]


# --------------------------------------------------------------------------- #
# CPU
# --------------------------------------------------------------------------- #
def test_constructor_parameters_and_state_dict():
    for root in (True, False):
        for project in (True, False):
            for bias in (True, False):
                conv = dc.nn.SAGEConv(21, 64, root_weight=root, project=project, bias=bias)
                want = {"lin_l.weight": (64, 21)}
                if bias:
                    want["lin_l.bias"] = (64,)
                if root:
                    want["lin_r.weight"] = (64, 21)
                if project:
                    want["lin.weight"], want["lin.bias"] = (21, 21), (21,)
                assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == want
                assert len(list(conv.parameters())) == len(want) and not hasattr(conv, "bias")
                assert (conv.lin_r is None) == (not root) and (conv.lin is None) == (not project)
                assert conv.graph_flags() == dict(self_loops=False, normalize=False)
                assert conv.supports_fused_relu is True
                r = repr(conv)
                assert r.startswith("SAGEConv(") and "21, 64, aggr=mean" in r
                assert ("root_weight=False" in r) == (not root) and ("project=True" in r) == project
                ref = RefSage(21, 64, root_weight=root, project=project, bias=bias)
                assert set(ref.state_dict()) == set(conv.state_dict())
                conv.load_state_dict(ref.state_dict(), strict=True)
                assert torch.equal(conv.lin_l.weight, ref.lin_l.weight)
    one = dc.nn.SAGEConv(21, 64)
    assert (one.aggr, one.normalize, one.root_weight, one.project) == ("mean", False, True, False)
    assert one.lin_l.bias is not None and one.lin_r.bias is None
    assert dc.nn.SAGEConv(21, 64, "max").aggr == "max"           # aggr is the third positional argument, as in PyG
    assert dc.nn.SAGEConv(21, 64, aggr="add").aggr == "sum" and dc.nn.SAGEConv(21, 64, aggr="sum").aggr == "sum"
    bound = float(1 / np.sqrt(21.0))
    conv, seen = dc.nn.SAGEConv(21, 64, project=True), []
    for _ in range(3):
        conv.reset_parameters()
        seen.append(conv.lin_l.weight.detach().clone())
        for t in (conv.lin_l.weight, conv.lin_l.bias, conv.lin_r.weight, conv.lin.weight, conv.lin.bias):
            assert 0.5 * bound < float(t.detach().abs().max()) <= bound
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    for bad in ("min", "lstm", "median", None, ["mean", "max"], ("mean",), nn.Identity()):
        with pytest.raises(ValueError):
            dc.nn.SAGEConv(21, 64, aggr=bad)
    for unsupported in (dict(size=(3, 3)), dict(dropout=0.1), dict(aggr_kwargs={})):
        with pytest.raises(TypeError):
            dc.nn.SAGEConv(21, 64, **unsupported)                # not supported: absent from the signature
    with pytest.raises(TypeError):
        dc.nn.SAGEConv((21, 25), 64)                             # bipartite input
    with pytest.raises(TypeError):
        one(torch.zeros(5, 21), torch.zeros(2, 3, dtype=torch.long), size=(5, 5))
    with pytest.raises(RuntimeError, match="HIP device"):
        one(torch.zeros(5, 21), torch.zeros(2, 3, dtype=torch.long))
    with pytest.raises(ValueError):
        ops.aggregate(None, torch.zeros(5, 21), "min")           # the reduction is checked first
    with pytest.raises(ValueError):
        ops.aggregate(None, torch.zeros(5, 21), ["mean"])
    assert "SAGEConv" in dc.nn.__all__
    assert dc.nn.__all__[:9] == ["TAGConv", "GCNConv", "GATConv", "GATv2Conv", "TransformerConv", "knn", "knn_graph",
                                 "radius", "radius_graph"]


def test_importable_through_the_torch_geometric_alias():
    import sys
    from deformcontact_amd.pyg_alias import install_as_torch_geometric
    names = ("torch_geometric", "torch_geometric.nn", "torch_geometric.data")
    saved = {k: sys.modules.get(k) for k in names}
    try:
        install_as_torch_geometric(force=True)
        from torch_geometric.nn import SAGEConv as aliased
        assert aliased is dc.nn.SAGEConv
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def _entry_calls():
    """name -> call(N, F, pointers given?, leading dimension) of every entry of dc_sage.hip, otherwise valid"""
    L = _lib.lib()
    p = lambda ok: 64 if ok else None                           # any non-null address: rejected calls never touch it
    return {
        "dc_sage_mean_fwd": lambda n, f, ok, ld: L.dc_sage_mean_fwd(p(ok), p(ok), p(ok), ld, 128 if ok else None, ld, n, f,
                                                                    None),
        "dc_sage_mean_bwd": lambda n, f, ok, ld: L.dc_sage_mean_bwd(p(ok), p(ok), p(ok), p(ok), ld, 128 if ok else None,
                                                                    ld, n, f, None),
        "dc_sage_max_fwd": lambda n, f, ok, ld: L.dc_sage_max_fwd(p(ok), p(ok), p(ok), ld, 128 if ok else None, ld,
                                                                  192 if ok else None, ld, n, f, None),
        "dc_sage_max_bwd": lambda n, f, ok, ld: L.dc_sage_max_bwd(p(ok), p(ok), p(ok), ld, p(ok), ld, p(ok), ld, p(ok), ld,
                                                                  128 if ok else None, ld, n, f, None),
    }


def test_abi_argument_errors_of_the_sage_entries_without_gpu():
    """null pointers, negative N, F < 1, sizes out of range, short leading dimensions, aliased outputs: -1 and the
    entry's name, before any HIP call; N = 0 returns 0 with no pointer at all."""
    L = _lib.lib()
    calls = _entry_calls()
    declared = [n for n in _lib.exported_names() if "sage" in n]
    assert sorted(declared) == sorted(calls)
    for name, call in calls.items():
        assert call(3, 16, False, 64) == -1 and name.encode() in L.dc_last_error() and b"null" in L.dc_last_error(), name
        assert call(-1, 16, True, 64) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, 0, True, 64) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, -2, True, 64) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, 1 << 24, True, 1 << 24) == -1 and b"range" in L.dc_last_error(), name
        assert call(1 << 30, 16, True, 64) == -1 and b"range" in L.dc_last_error(), name
        assert call(3, 16, True, 15) == -1 and name.encode() in L.dc_last_error() and b"leading" in L.dc_last_error(), name
        assert call(3, 16, False, 15) == -1 and b"leading" in L.dc_last_error(), name      # sizes, strides, then nulls
        assert call(0, 16, False, 64) == 0, name                 # no row: nothing is read, written or launched
        assert call(0, 16, False, 15) == -1, name
    # outputs that alias an operand
    assert L.dc_sage_mean_fwd(64, 64, 128, 16, 128, 16, 3, 16, None) == -1 and b"alias" in L.dc_last_error()
    assert L.dc_sage_mean_bwd(64, 64, 64, 128, 16, 128, 16, 3, 16, None) == -1 and b"alias" in L.dc_last_error()
    assert L.dc_sage_max_fwd(64, 64, 128, 16, 128, 16, None, 16, 3, 16, None) == -1 and b"alias" in L.dc_last_error()
    assert L.dc_sage_max_fwd(64, 64, 128, 16, 192, 16, 192, 16, 3, 16, None) == -1 and b"alias" in L.dc_last_error()
    assert L.dc_sage_max_bwd(64, 64, 128, 16, 192, 16, 256, 16, 320, 16, 192, 16, 3, 16, None) == -1
    assert b"alias" in L.dc_last_error()
    # the max forward without the counts takes a null cnt (and then no leading dimension for it)
    assert L.dc_sage_max_fwd(64, 64, 128, 16, 192, 16, None, 0, 0, 16, None) == 0


def test_float32_restatement_within_the_bar_of_float64_on_the_layer_inputs():
    """Every layer case of the GPU tests: float32 RefSage within 1e-5 of float64, output and every gradient."""
    for (fi, fo), aggr, kind, variant in _layer_cases():
        case = layer_case(fi, fo, aggr, kind, variant)
        check_against_references(f"RefSage fp32 vs fp64 {fi}->{fo} {aggr} {kind} {variant}", case["r32"], case, "e_o")
        if case["n"] and fo > 1:                                 # the per-row metric of the GPU test
            assert row_rel_err(case["r32"][0], case["r64"][0]) < TOL, (fi, fo, aggr, kind, variant)


@pytest.mark.parametrize("kind", DIRECT_GRAPHS)
def test_direct_inputs_have_ties_and_the_references_agree(kind):
    """The grid inputs of the direct max tests: at least 10 % of the (i, c) cells have two or more edges at the
    maximum, so the tie path cannot go untested; and the hand-written backward formula (float64) equals torch autograd
    through the masked formula (float64) - on these inputs, ties through distinct sources and duplicate edges
    included - as does the mean's."""
    for f in (3, 20):
        case = direct_case(kind, f, "grid")
        n, ptr, other, dst = case["n"], case["ptr"], case["other"], case["dst"]
        deg = np.diff(ptr)
        assert (deg == 0).any() and (case["cnt"][deg == 0] == 0).all() and (case["m"][deg == 0] == 0).all()
        assert (case["cnt"][deg > 0] >= 1).all()
        tied = float((case["cnt"] >= 2).mean())
        assert tied >= 0.10, (kind, f, tied)
        if kind == "multigraph":                                 # a duplicate edge that attains the maximum counts twice
            pairs = np.stack([other, dst], 1)
            _, inv, mult = np.unique(pairs, axis=0, return_inverse=True, return_counts=True)
            dup = mult[inv.ravel()] > 1
            assert dup.any() and ((case["x"][other] == case["m"][dst]) & dup[:, None]).any()
        xt = torch.from_numpy(case["x"]).double().requires_grad_(True)
        gup = torch.from_numpy(case["gup"]).double()
        j, i = torch.from_numpy(other), torch.from_numpy(dst)
        out = ref_max(xt, j, i, n)
        assert rel_err(out.detach().numpy(), case["m"]) < 1e-12
        (out * gup).sum().backward()
        assert rel_err(case["max_bwd"], xt.grad.numpy()) < 1e-12
        # the even split: what the edges of one cell receive adds up to the cell's gradient
        hit = case["x"][other] == case["m"][dst]
        share = np.where(hit, case["gup"].astype(np.float64)[dst] / np.maximum(case["cnt"][dst], 1), 0.0)
        back = np.zeros((n, f))
        np.add.at(back, dst, share)
        assert np.abs(back - np.where(deg[:, None] > 0, case["gup"], 0.0)).max() < 1e-12
        xt.grad = None
        mean = pyg_ref.scatter_sum(xt[j], i, n) / torch.from_numpy(np.maximum(deg, 1)).double().unsqueeze(-1)
        (mean * gup).sum().backward()
        assert rel_err(case["mean_bwd"], xt.grad.numpy()) < 1e-12


def test_three_tied_zeros_split_evenly():
    """The case of INTEGRATION.md 1.5: three sources at 0 into one destination, upstream gradient 2 - 2/3 each here
    (zero-initialised ``scatter_reduce_(amax, include_self=False)`` gives 0.5: it counts its own initial 0)."""
    x = torch.zeros(4, 1, dtype=torch.float64, requires_grad=True)
    j, i = torch.tensor([0, 1, 2]), torch.tensor([3, 3, 3])
    (ref_max(x, j, i, 4) * 2.0).sum().backward()
    assert np.allclose(x.grad.numpy().ravel(), [2 / 3, 2 / 3, 2 / 3, 0.0], atol=1e-15)
    ptr, other, dst = host_adjacency(4, np.stack([j.numpy(), i.numpy()]))
    m, cnt = max_fwd_ref(ptr, other, dst, np.zeros((4, 1), np.float32))
    assert cnt.ravel().tolist() == [0, 0, 0, 3] and (m == 0).all()
    got = max_bwd_ref(ptr, other, dst, np.zeros((4, 1), np.float32), m, cnt, np.full((4, 1), 2.0, np.float32))
    assert np.allclose(got.ravel(), [2 / 3, 2 / 3, 2 / 3, 0.0], atol=1e-15)


# --------------------------------------------------------------------------- #
# GPU: the entries called directly
# --------------------------------------------------------------------------- #
def _device_graph(case):
    g = GraphIndex(torch.from_numpy(case["ei"]).to(DEV), case["n"], self_loops=False, normalize=False, validate=True)
    assert np.array_equal(_np(g.fwd.ptr).astype(np.int64), case["ptr"])
    return g


def _wide(t, pad=12, off=4):
    """``t`` as a column slice of a wider buffer (row stride > width; rows stay 16-byte aligned)"""
    buf = torch.full((t.size(0), t.size(1) + pad), 1e30, device=t.device)
    buf[:, off:off + t.size(1)] = t
    return buf[:, off:off + t.size(1)]


def _odd(t):
    """``t`` as a column slice whose rows are NOT 16-byte aligned (the general form at every width)"""
    buf = torch.full((t.size(0), t.size(1) + 3), 1e30, device=t.device)
    buf[:, 1:1 + t.size(1)] = t
    return buf[:, 1:1 + t.size(1)]


def _within_bar_of_float64(got, want64, name):
    d = row_rel_err(got, want64)
    record_parity(name, None, e_h=d, metric="row_rel_err")
    assert d < TOL, (name, d)


@gpu
@pytest.mark.parametrize("kind", DIRECT_GRAPHS)
@pytest.mark.parametrize("f", WIDTHS)
def test_mean_entries(f, kind):
    """forward bit-identical to the unweighted hop divided by the in-degree, rows without edges exactly 0; backward
    within 1e-5 of float64 per row; strided operands and a non-contiguous upstream gradient: the same bits; twice:
    the same bits."""
    case = direct_case(kind, f, "normal")
    g, n = _device_graph(case), case["n"]
    deg = np.diff(case["ptr"])
    x, gy = _dev(case["x"]), _dev(case["gup"])
    y = ops._sage_mean_fwd(g, x)
    hop = ops.propagate(g, x, weighted=False)
    tdeg = torch.from_numpy(deg).to(DEV).clamp(min=1).to(torch.float32).unsqueeze(-1)
    assert torch.equal(y, hop / tdeg)
    assert (y[torch.from_numpy(deg == 0).to(DEV)] == 0).all() and torch.isfinite(y).all()
    assert torch.equal(y, ops._sage_mean_fwd(g, x))
    assert torch.equal(y, ops._sage_mean_fwd(g, _wide(x))) and torch.equal(y, ops._sage_mean_fwd(g, _odd(x)))
    assert torch.equal(y, ops.aggregate(g, x, "mean")) and torch.equal(hop, ops.aggregate(g, x, "sum"))
    gx = ops._sage_mean_bwd(g, gy)
    assert torch.equal(gx, ops._sage_mean_bwd(g, gy))
    assert torch.equal(gx, ops._sage_mean_bwd(g, _wide(gy))) and torch.equal(gx, ops._sage_mean_bwd(g, _odd(gy)))
    _within_bar_of_float64(_np(gx), case["mean_bwd"], f"mean g_x F={f} {kind}")
    # strided OUTPUTS: the entries called with row strides f + 8 write the same values and nothing beside them
    L, st, ld = _lib.lib(), torch.cuda.current_stream().cuda_stream, f + 8
    o_y, o_g = torch.full((n, ld), 7.0, device=DEV), torch.full((n, ld), 7.0, device=DEV)
    _lib.check(L.dc_sage_mean_fwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), x.data_ptr(), f, o_y.data_ptr(), ld, n, f,
                                  st), "dc_sage_mean_fwd")
    _lib.check(L.dc_sage_mean_bwd(g.bwd.ptr.data_ptr(), g.bwd.other.data_ptr(), g.fwd.ptr.data_ptr(), gy.data_ptr(), f,
                                  o_g.data_ptr(), ld, n, f, st), "dc_sage_mean_bwd")
    for wide_out, dense in ((o_y, y), (o_g, gx)):
        assert torch.equal(wide_out[:, :f], dense) and (wide_out[:, f:] == 7.0).all()
    # through autograd, the gradient arriving non-contiguous (every second column of a wider buffer) and expanded
    wide_g = torch.full((n, 2 * f), 1e30, device=DEV)
    wide_g[:, ::2] = gy
    xs = _wide(x).detach().requires_grad_(True)
    assert not xs.is_contiguous() and (f == 1 or not wide_g[:, ::2].is_contiguous())
    torch.autograd.backward([ops.aggregate(g, xs, "mean")], [wide_g[:, ::2]])
    assert torch.equal(xs.grad, gx)
    xs.grad = None
    ops.aggregate(g, xs, "mean").sum().backward()                # an expanded gradient of ones
    assert torch.equal(xs.grad, ops._sage_mean_bwd(g, torch.ones_like(gy)))


def _check_max_entries(values, f, kind):
    case = direct_case(kind, f, values)
    g, n = _device_graph(case), case["n"]
    deg = np.diff(case["ptr"])
    x, gm = _dev(case["x"]), _dev(case["gup"])
    m, cnt = ops._sage_max_fwd(g, x, True)
    assert cnt.dtype == torch.int32 and cnt.shape == (n, f)
    assert np.array_equal(_np(m), case["m"]) and np.array_equal(_np(cnt), case["cnt"])
    if values == "normal":
        # no two sources share a value: every edge that attains a maximum comes from ONE source, and the count is the
        # number of copies of that edge (``seg_graph`` draws duplicate edges)
        hit = case["x"][case["other"]] == case["m"][case["dst"]]
        src = np.broadcast_to(case["other"][:, None], hit.shape)
        lo, hi = np.full((n, f), n), np.full((n, f), -1)
        np.minimum.at(lo, case["dst"], np.where(hit, src, n))
        np.maximum.at(hi, case["dst"], np.where(hit, src, -1))
        assert (lo == hi)[deg > 0].all() and (case["cnt"] == 1).mean() > 0.5 and (case["cnt"] >= 1)[deg > 0].all()
    else:
        assert (case["cnt"] >= 2).mean() >= 0.10
    none = torch.from_numpy(deg == 0).to(DEV)
    assert (m[none] == 0).all() and (cnt[none] == 0).all()
    m2, no_cnt = ops._sage_max_fwd(g, x, False)
    assert no_cnt is None and torch.equal(m2, m)
    for xx in (x, _wide(x), _odd(x)):
        mm, cc = ops._sage_max_fwd(g, xx, True)
        assert torch.equal(mm, m) and torch.equal(cc, cnt)
    gx = ops._sage_max_bwd(g, x, m, cnt, gm)
    assert torch.equal(gx, ops._sage_max_bwd(g, x, m, cnt, gm))
    assert torch.equal(gx, ops._sage_max_bwd(g, _wide(x), _wide(m), cnt, _wide(gm)))
    assert torch.equal(gx, ops._sage_max_bwd(g, _odd(x), m, cnt, _odd(gm)))
    _within_bar_of_float64(_np(gx), case["max_bwd"], f"max g_x F={f} {kind} {values}")
    L, st, ld = _lib.lib(), torch.cuda.current_stream().cuda_stream, f + 8
    o_m, o_g = torch.full((n, ld), 7.0, device=DEV), torch.full((n, ld), 7.0, device=DEV)
    o_c = torch.full((n, ld), 7, dtype=torch.int32, device=DEV)
    _lib.check(L.dc_sage_max_fwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), x.data_ptr(), f, o_m.data_ptr(), ld,
                                 o_c.data_ptr(), ld, n, f, st), "dc_sage_max_fwd")
    _lib.check(L.dc_sage_max_bwd(g.bwd.ptr.data_ptr(), g.bwd.other.data_ptr(), x.data_ptr(), f, o_m.data_ptr(), ld,
                                 o_c.data_ptr(), ld, gm.data_ptr(), f, o_g.data_ptr(), ld, n, f, st), "dc_sage_max_bwd")
    for wide_out, dense in ((o_m, m), (o_c, cnt), (o_g, gx)):
        assert torch.equal(wide_out[:, :f], dense) and (wide_out[:, f:] == 7).all()
    # through autograd: the counts are written because a gradient is wanted; without one the forward is the same
    xs = _wide(x).detach().requires_grad_(True)
    out = ops.aggregate(g, xs, "max")
    assert torch.equal(out, m) and torch.equal(ops.aggregate(g, x, "max"), m)
    wide_g = torch.full((n, 2 * f), 1e30, device=DEV)
    wide_g[:, ::2] = gm
    torch.autograd.backward([out], [wide_g[:, ::2]])
    assert torch.equal(xs.grad, gx)


@gpu
@pytest.mark.parametrize("kind", DIRECT_GRAPHS)
@pytest.mark.parametrize("f", WIDTHS)
def test_max_entries(f, kind):
    """grid values - ties between distinct sources and through duplicate edges: m and cnt equal to the restatement
    element for element, g_x within 1e-5 of float64 per row; strided operands: the same bits; twice: the same bits."""
    _check_max_entries("grid", f, kind)


@gpu
@pytest.mark.parametrize("f", [3, 256])
def test_max_entries_plain_values(f):
    """x ~ N(0, 1): no tie between distinct sources, a count above 1 only through duplicate edges - the general and the
    16-byte form"""
    _check_max_entries("normal", f, "seg")


@gpu
def test_entries_with_no_rows_and_with_no_edges():
    """N = 0: every entry returns 0 without a launch, ``aggregate`` an empty tensor that carries a gradient; N > 0
    without any edge: zeros everywhere."""
    L = _lib.lib()
    zi = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert L.dc_sage_mean_fwd(zi.data_ptr(), zi.data_ptr(), None, 15, None, 15, 0, 15, None) == 0
    assert L.dc_sage_mean_bwd(zi.data_ptr(), zi.data_ptr(), zi.data_ptr(), None, 15, None, 15, 0, 15, None) == 0
    assert L.dc_sage_max_fwd(zi.data_ptr(), zi.data_ptr(), None, 15, None, 15, None, 15, 0, 15, None) == 0
    assert L.dc_sage_max_bwd(zi.data_ptr(), zi.data_ptr(), None, 15, None, 15, None, 15, None, 15, None, 15, 0, 15,
                             None) == 0
    for reduce in ("sum", "mean", "max"):
        x0 = torch.zeros((0, 15), device=DEV, requires_grad=True)
        y0 = ops.aggregate(None, x0, reduce)
        assert y0.shape == (0, 15) and y0.requires_grad
        y0.sum().backward()
        assert x0.grad.shape == (0, 15)
    n, f = 37, 15
    g = GraphIndex(torch.zeros((2, 0), dtype=torch.int64, device=DEV), n, self_loops=False, normalize=False)
    x = torch.randn(n, f, device=DEV)
    assert (ops._sage_mean_fwd(g, x) == 0).all() and (ops._sage_mean_bwd(g, x) == 0).all()
    m, cnt = ops._sage_max_fwd(g, x, True)
    assert (m == 0).all() and (cnt == 0).all() and (ops._sage_max_bwd(g, x, m, cnt, x + 1) == 0).all()
    with pytest.raises(ValueError):
        ops.aggregate(g, x, "min")
    with pytest.raises(ValueError):
        ops.aggregate(g, x.double(), "mean")
    with pytest.raises(ValueError, match="None"):
        ops.aggregate(None, x, "mean")
    with pytest.raises(ValueError):
        ops.aggregate(g, x[:5], "mean")
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.aggregate(g, x.cpu(), "mean")
    with pytest.raises(ValueError):
        ops.aggregate(GraphIndex(torch.zeros((2, 0), dtype=torch.int64, device=DEV), n, self_loops=True,
                                 normalize=False), x, "mean")


# --------------------------------------------------------------------------- #
# GPU: the layer
# --------------------------------------------------------------------------- #
def _device_conv(cpu, fi, fo, aggr, **opts):
    conv = dc.nn.SAGEConv(fi, fo, aggr=aggr, **opts)
    conv.load_state_dict({k: v.clone() for k, v in cpu.state_dict().items()}, strict=True)
    return conv.to(DEV)


def _device_run(conv, x, ei, gup, **kw):
    for p in conv.parameters():
        p.grad = None
    xg = (x if isinstance(x, torch.Tensor) else torch.from_numpy(x).to(DEV)).detach().requires_grad_(True)
    out = ops.resolve(conv(xg, torch.from_numpy(ei).to(DEV), **kw))
    gup = gup if isinstance(gup, torch.Tensor) else torch.from_numpy(gup).to(DEV)
    torch.autograd.backward([out], [gup])
    torch.cuda.synchronize()
    return out.detach(), xg.grad, {n: (None if p.grad is None else p.grad.detach().clone())
                                   for n, p in conv.named_parameters()}


def _check_layer(fi, fo, aggr, kind, variant):
    case = layer_case(fi, fo, aggr, kind, variant)
    clear_cache()
    conv = _device_conv(case["cpu"], fi, fo, aggr, **case["opts"])
    tag = f"SAGEConv {fi}->{fo} {aggr} {kind} {variant}"
    if aggr == "max" and case["opts"].get("project"):
        # the precondition of a max over projected sources: they are the same numbers in every evaluation
        with torch.no_grad():
            src = ops.dense_linear(_dev(case["x"]), conv.lin.weight, conv.lin.bias, relu=True)
            want = case["cpu"].sources(torch.from_numpy(case["x"]))
        assert torch.equal(src.cpu(), want), f"{tag}: the projected sources are not exact"
        assert float((want == 0).float().mean()) > 0.3           # ReLU outputs: exact zero ties are the rule
    og, gxg, gpg = _device_run(conv, case["x"], case["ei"], case["gup"], relu=case["relu"])
    got = (_np(og), _np(gxg), {k: (None if v is None else _np(v)) for k, v in gpg.items()})
    assert got[0].shape == case["r32"][0].shape and set(got[2]) == set(case["r32"][2])
    assert all(v is not None for v in got[2].values())
    check_against_references(tag, got, case, "e_h")
    if case["n"] and fo > 1:
        # (``row_rel_err`` takes at least one row; with ONE output channel a row is a single number and its relative
        # error the conditioning of that one dot product, not a property of the layer)
        assert_parity(got[0], case["r32"][0], case["r64"][0], TOL, f"{tag} forward per row", metric=row_rel_err)


@gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("kind", MAIN_GRAPHS)
@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("fi,fo", SHAPES)
def test_layer_parity(fi, fo, aggr, kind, variant):
    """forward and the gradients of x and of every parameter against RefSage at 1e-5: every shape x aggregation x
    graph x variant; with ``aggr="max"`` on grid inputs (module docstring)."""
    _check_layer(fi, fo, aggr, kind, variant)


@gpu
@pytest.mark.parametrize("kind", EDGE_GRAPHS)
@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("fi,fo", SHAPES)
def test_layer_parity_edge_graphs(fi, fo, aggr, kind):
    """one node, no edge, no node, and the second golden mesh"""
    _check_layer(fi, fo, aggr, kind, "default")
    if kind in ("n1", "e0", "n0"):
        case = layer_case(fi, fo, aggr, kind, "default")
        for opts in (dict(root_weight=False), dict(root_weight=False, bias=False)):
            clear_cache()
            torch.manual_seed(2)
            conv = dc.nn.SAGEConv(fi, fo, aggr=aggr, **opts).to(DEV)
            out = ops.resolve(conv(_dev(case["x"]), torch.from_numpy(case["ei"]).to(DEV)))
            want = torch.zeros((case["n"], fo), device=DEV) + (conv.lin_l.bias.detach() if "bias" not in opts else 0.0)
            assert out.shape == (case["n"], fo) and torch.equal(out, want)   # nothing aggregated: the bias alone, or 0


@gpu
def test_projected_sources_are_exact():
    """``project=True`` under a max: grid x, grid ``lin`` - the library's ``relu(lin(x))`` equals the float32 CPU
    evaluation bit for bit at every ``in_channels`` of the layer tests, and the float64 one."""
    for fi in sorted({s[0] for s in SHAPES}):
        rng = np.random.default_rng(fi)
        x, w, b = grid_values(rng, (300, fi)), grid_weights(rng, (fi, fi)), grid_weights(rng, (fi,))
        got = ops.dense_linear(_dev(x), _dev(w), _dev(b), relu=True).cpu()
        want32 = torch.relu(F.linear(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b)))
        want64 = torch.relu(F.linear(torch.from_numpy(x).double(), torch.from_numpy(w).double(),
                                     torch.from_numpy(b).double()))
        assert torch.equal(want32.double(), want64) and torch.equal(got, want32), fi


# --------------------------------------------------------------------------- #
# GPU: call patterns
# --------------------------------------------------------------------------- #
def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert set(a[2]) == set(b[2])
    for name in a[2]:
        assert (a[2][name] is None and b[2][name] is None) or torch.equal(a[2][name], b[2][name]), name


@gpu
@pytest.mark.parametrize("variant", ["default", "noroot", "project", "normalize"])
@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("fi,fo", [(25, 256), (64, 20)])
def test_bit_for_bit_relu_deferred_and_repeat(fi, fo, aggr, variant, monkeypatch):
    case = layer_case(fi, fo, aggr, "hub", variant)
    n, ei, x, gup, opts = case["n"], case["ei"], case["x"], case["gup"], case["opts"]
    clear_cache()
    conv = _device_conv(case["cpu"], fi, fo, aggr, **opts)
    tei, xg = torch.from_numpy(ei).to(DEV), torch.from_numpy(x).to(DEV)
    plain = ops.resolve(conv(xg, tei)).clone()
    assert plain.shape == (n, fo)
    want = torch.relu(plain)
    assert (plain < 0).any() and (plain > 0).any()
    assert torch.equal(conv(xg, tei, relu=True), want)
    assert torch.equal(conv(xg, tei, relu=True, next_conv=conv), want)      # next_conv: accepted and ignored
    y = conv(xg, tei)
    assert type(y).__name__ == "DeferredActivation" and y.shape == plain.shape
    assert torch.equal(F.relu(y), want)
    for kw in ({}, {"relu": True}):
        _same(_device_run(conv, x, ei, gup, **kw), _device_run(conv, x, ei, gup, **kw))
    deferred_run = _device_run(conv, x, ei, gup)
    monkeypatch.setattr(dc.nn.conv, "DEFER_ACTIVATION", False)
    direct = conv(xg, tei)
    assert isinstance(direct, torch.Tensor) and torch.equal(direct, plain)
    assert torch.equal(F.relu(conv(xg, tei)), want)
    _same(_device_run(conv, x, ei, gup), deferred_run)


@gpu
def test_launches_of_one_layer_step():
    """forward + backward: mean and max one kernel of dc_sage.hip each way, the sum the unweighted hop each way; no
    attention kernel."""
    for aggr, fwd, bwd in (("mean", "k_sage_mean_fwd", "k_sage_mean_bwd"), ("max", "k_sage_max_fwd", "k_sage_max_bwd"),
                           ("sum", "k_spmm", "k_spmm")):
        case = layer_case(25, 256, aggr, "multigraph", "default")
        clear_cache()
        conv = _device_conv(case["cpu"], 25, 256, aggr)
        _lib.kernel_trace(True)
        _device_run(conv, case["x"], case["ei"], case["gup"])
        counts = _lib.kernel_trace_counts()
        _lib.kernel_trace(False)
        sage = {name: v for name, v in counts.items() if "k_sage" in name}
        if aggr == "sum":
            assert not sage and sum(v for name, v in counts.items() if "k_spmm" in name) == 2, counts
        else:
            assert sum(sage.values()) == 2 and all(v == 1 for v in sage.values()), counts
            assert any(fwd in name for name in sage) and any(bwd in name for name in sage), counts
            assert not any("k_spmm" in name for name in counts), counts
        assert not any("tconv" in name or "gatv2" in name or "k_gat_" in name for name in counts), counts


@gpu
@pytest.mark.parametrize("aggr", AGGRS)
def test_strided_input_and_gradient_give_the_same_bits(aggr):
    fi, fo = 25, 256
    case = layer_case(fi, fo, aggr, "multigraph", "default")
    n, ei, x, gup = case["n"], case["ei"], case["x"], case["gup"]
    clear_cache()
    conv = _device_conv(case["cpu"], fi, fo, aggr)
    want = _device_run(conv, x, ei, gup)
    wide_x = torch.full((n, fi + 7), 1e30, device=DEV)
    wide_x[:, 3:3 + fi] = torch.from_numpy(x).to(DEV)
    wide_g = torch.full((n, 2 * gup.shape[1]), 1e30, device=DEV)
    wide_g[:, ::2] = torch.from_numpy(gup).to(DEV)
    xs, gs = wide_x[:, 3:3 + fi], wide_g[:, ::2]
    for p in conv.parameters():
        p.grad = None
    xg = xs.detach().requires_grad_(True)
    assert not xg.is_contiguous() and not gs.is_contiguous()
    out = ops.resolve(conv(xg, torch.from_numpy(ei).to(DEV)))
    torch.autograd.backward([out], [gs])
    torch.cuda.synchronize()
    _same((out.detach(), xg.grad, {k: p.grad for k, p in conv.named_parameters()}), want)


@gpu
def test_forward_and_backward_captured_and_replayed():
    """forward + backward of three stacked layers (max with projection, mean, sum) on ONE stream under
    torch.cuda.graph (no host read anywhere); two replays with new x in the static input, each bit-identical to the
    eager run on that input."""
    n, ei = _graph("multigraph", 12)
    fi, h = 32, 64
    torch.manual_seed(3)
    l1 = dc.nn.SAGEConv(fi, h, aggr="max", project=True).to(DEV)
    l2 = dc.nn.SAGEConv(h, h, aggr="mean", root_weight=False).to(DEV)
    l3 = dc.nn.SAGEConv(h, 20, aggr="sum", normalize=True).to(DEV)
    params = [p for l in (l1, l2, l3) for p in l.parameters()]
    tei = torch.from_numpy(ei).to(DEV)
    rng = np.random.default_rng(1)
    xs = [torch.from_numpy(grid_values(rng, (n, fi))).to(DEV) for _ in range(3)]
    gup = torch.from_numpy(rng.uniform(0.5, 1.5, (n, 20)).astype(np.float32)).to(DEV)
    static_x = xs[0].clone().requires_grad_(True)
    leaves = [static_x] + params
    for t in leaves:
        t.grad = torch.zeros_like(t)

    def step():
        for t in leaves:
            t.grad.zero_()
        out = l3(l2(l1(static_x, tei, relu=True), tei, relu=True), tei, relu=True)
        torch.autograd.backward([out], [gup])
        return out

    def snapshot(out):
        return [out.detach().clone()] + [t.grad.clone() for t in leaves]

    eager = []
    for x in xs:
        with torch.no_grad():
            static_x.copy_(x)
        clear_cache()
        eager.append(snapshot(step()))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        clear_cache()
        step()                                                   # warm-up off the default stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    clear_cache()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for i in (1, 2):
        with torch.no_grad():
            static_x.copy_(xs[i])
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(snapshot(out), eager[i]):
            assert torch.equal(got, want), i
