"""``EdgeConv``: the layer, ``ops.edge_pairs`` / ``ops.edge_aggregate`` and the C entries of dc_edge.hip.

The reference is this file's own restatement of the contract in INTEGRATION.md 1.10 (PyG 2.5.2 edge_conv.py):
``RefEdgeConv``, a torch CPU module evaluated in float32 (``ref32``) and float64 (``truth64``) with gradients from torch
autograd, and numpy formulas for the entries called directly.  Its max is the mask / count form of
tests/test_sage_conv.py - ``m = segment max; mask = (msg == m[i]); cnt = sum(mask); out = sum(mask * msg / cnt)`` with
``mask`` and ``cnt`` constant - so autograd yields the library's tie rule, the EVEN split among all edges that attain
the maximum (``scatter_reduce_(amax)`` counts the output's initial 0 among the ties and is not used).

One selection in every evaluation.  A maximum that is attained by different edges in float32, in float64 and on the
device changes a gradient by a whole term, and so does a ReLU inside ``nn`` whose mask differs.  The cases with
``aggr="max"`` and all cases with ``nn = Sequential(Linear, ReLU, Linear)`` therefore take ``x`` from multiples of 1/4
in [-2, 2] and ``nn``'s parameters from multiples of 1/8 in [-1, 1]: a pair row holds multiples of 1/4 in [-4, 4], a
first-layer output is a sum of at most 2 * 64 + 1 multiples of 1/32 below 2^10, and with 16 hidden units a second-layer
output a sum of 17 multiples of 1/256 below 2^14 - exact float32 numbers in any summation order (23 bits suffice up to
2^15 at a step of 1/256).  That exactness is asserted on the CPU (float32 == float64) and on the device before a layer
is compared.  ``Linear`` under mean / sum runs on N(0, 1) inputs with the default initialisation.

On the device ``nn`` is built from ``Linear64``: ``torch.nn.Linear`` with the same parameters and forward whose weight
and bias gradients - sums over the E edge rows inside the USER's module - are taken in float64, so that the bar
measures the layer's kernels and not a BLAS's summation order (figures: see ``Linear64``); plain ``torch.nn.Linear``
runs on the graph without a hub (``test_layer_parity_with_plain_torch_modules``).

Metrics.  The layer through ``helpers.assert_parity`` at 1e-5 (nothing registered ``special``).  The entries:
``dc_edge_pair_fwd`` bit-identical to numpy (a copy and ONE fp32 subtraction); ``dc_edge_pair_bwd`` within 1e-5 per row
(``row_rel_err``) of a float64 ``index_add`` of the same terms (the difference formed in fp32 first), the ``ops`` node
against the float64 autograd gradient of the torch composition - 1e-5 of the tensor's scale and, per element, 4 * 2^-24
of the sum of its terms' absolute values (``term_rel_err``); ``dc_edge_reduce_fwd`` sum bit-identical to a numpy
float32 loop over the device's own ``ptr`` / ``perm`` in p order, mean that sum divided by ``np.float32(deg)``, max ``y``
and ``cnt`` equal element for element; ``dc_edge_reduce_bwd`` bit-identical to the numpy float32 formula (every term one
copy or one division).  Max inputs come from a coarse grid (multiples of 0.25, a third of them zeros), so ties between
distinct edges and through duplicates are certain.

The adjacencies are built WITHOUT self-loop handling: ``seg_graph`` of ``seg_lens`` gives in-degrees 0, 1, 6, ..., 64
and the hub, ``random_multigraph`` keeps its self loops, duplicates and isolated nodes.
"""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import deformcontact_amd as dc
from deformcontact_amd import _lib, ops
from deformcontact_amd.graph import GraphIndex, clear_cache
from deformcontact_amd.nn import EdgeConv  # noqa: F401  (the module needs the layer: no test runs without it)
from tests.helpers import assert_parity, random_multigraph, record_parity, rel_err, row_rel_err
from tests.test_gat_edge_kernels import HUB, _dev, _np, seg_graph, seg_lens

gpu = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5

#: (in, out) of the layer tests
SHAPES = [(3, 64), (21, 64), (64, 20), (16, 1)]
AGGRS = ["max", "mean", "sum"]
HIDDEN = 16
MAIN_GRAPHS = ["seg", "multigraph"]
EDGE_GRAPHS = ["n1", "e0", "n0"]
#: pair kernels: the general form (1, 3, 70: lane groups of 4, 4, 64) and the 16-byte form (20, 64, 256: 8, 16, 64)
PAIR_WIDTHS = [1, 3, 20, 64, 70, 256]
#: reduce kernels: the same and 1100 - 64 lanes over five column chunks
REDUCE_WIDTHS = [1, 3, 20, 64, 70, 256, 1100]
MODES = {"sum": 0, "mean": 1, "max": 2}


# --------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------- #
def grid_values(rng, shape):
    """multiples of 1/4 in [-2, 2]"""
    return (rng.integers(-8, 9, shape) / 4.0).astype(np.float32)


def grid_weights(rng, shape):
    """multiples of 1/8 in [-1, 1]"""
    return (rng.integers(-8, 9, shape) / 8.0).astype(np.float32)


def coarse_grid(rng, shape):
    """multiples of 0.25 in [-1, 1], a third of them zeros: ties are certain"""
    v = (rng.integers(-4, 5, shape) / 4.0).astype(np.float32)
    v[rng.random(shape) < 1 / 3] = 0
    return v


def signed(rng, shape):
    return (rng.uniform(0.5, 1.5, shape) * np.where(rng.random(shape) < 0.5, -1.0, 1.0)).astype(np.float32)


def _graph(kind, seed):
    """(n, edge_index [2, E] int64)"""
    if kind == "multigraph":
        return 300, random_multigraph(300, 2400, seed)          # self loops, duplicates, 30 nodes without in-edges
    if kind == "seg":
        return 131, seg_graph(seg_lens(131, HUB), seed)         # in-degrees 0, 1, 6, 7, 8, 14, ..., 64 and the hub
    if kind == "n1":
        return 1, np.zeros((2, 0), np.int64)                    # one node with no edge
    if kind == "e0":
        return 50, np.zeros((2, 0), np.int64)
    assert kind == "n0"
    return 0, np.zeros((2, 0), np.int64)


def _index_add(n, idx, terms):
    return torch.zeros((n, terms.shape[1]), dtype=torch.float64).index_add_(
        0, torch.from_numpy(idx), torch.from_numpy(np.ascontiguousarray(terms, np.float64))).numpy()


def segment_max(n, dst, m):
    """(y, cnt): exact in any dtype - y is one of the reduced values, cnt counts equalities; 0 for a row without edges"""
    y = np.full((n, m.shape[1]), -np.inf, m.dtype)
    np.maximum.at(y, dst, m)
    y[np.bincount(dst, minlength=n) == 0] = 0
    cnt = np.zeros(y.shape, np.int64)
    np.add.at(cnt, dst, m == y[dst])
    return y, cnt.astype(np.int32)


@functools.lru_cache(maxsize=None)
def pair_case(kind, f):
    """inputs and order-independent references of the pair kernels (computed once, never modified)"""
    n, ei = _graph(kind, 9)
    src, dst = ei
    rng = np.random.default_rng(3000 + f + len(kind))
    x = rng.standard_normal((n, f)).astype(np.float32)
    gz = rng.standard_normal((ei.shape[1], 2 * f)).astype(np.float32)
    z = np.concatenate([x[dst], x[src] - x[dst]], axis=1)       # a copy and ONE fp32 subtraction
    assert z.dtype == np.float32
    diff = gz[:, :f] - gz[:, f:]                                 # the kernel's term: formed in fp32 first
    gx64 = _index_add(n, dst, diff) + _index_add(n, src, gz[:, f:])
    xt = torch.from_numpy(x).double().requires_grad_(True)
    j, i = torch.from_numpy(ei)
    (torch.cat([xt[i], xt[j] - xt[i]], dim=1) * torch.from_numpy(gz).double()).sum().backward()
    abs64 = _index_add(n, dst, np.abs(diff)) + _index_add(n, src, np.abs(gz[:, f:]))
    return dict(n=n, ei=ei, x=x, gz=gz, z=z, gx64=gx64, gx_autograd64=xt.grad.numpy(), abs64=abs64)


#: float32 unit roundoff
U32 = 2.0 ** -24


def term_rel_err(a, b, abs_sum):
    """max over elements of |a - b| / (the sum of the absolute values of the element's terms): the scale fp32 rounding
    errors of a sum live on, whatever the terms cancel to"""
    if a.size == 0:
        return 0.0
    return float((np.abs(np.asarray(a, np.float64) - b) / np.maximum(abs_sum, 1e-30)).max())


@functools.lru_cache(maxsize=None)
def reduce_case(kind, c):
    n, ei = _graph(kind, 9)
    rng = np.random.default_rng(4000 + c + len(kind))
    ne = ei.shape[1]
    deg = np.bincount(ei[1], minlength=n)
    m, mg, gy = rng.standard_normal((ne, c)).astype(np.float32), coarse_grid(rng, (ne, c)), signed(rng, (n, c))
    y, cnt = segment_max(n, ei[1], mg)
    degf = np.maximum(deg, 1).astype(np.float32)[:, None]
    gm = {"sum": gy[ei[1]], "mean": gy[ei[1]] / degf[ei[1]],
          "max": np.where(mg == y[ei[1]], gy[ei[1]] / np.maximum(cnt, 1).astype(np.float32)[ei[1]], np.float32(0))}
    assert all(v.dtype == np.float32 for v in gm.values())
    return dict(n=n, ei=ei, deg=deg, m=m, mg=mg, gy=gy, y=y, cnt=cnt, gm=gm, sum64=_index_add(n, ei[1], m),
                abs64=_index_add(n, ei[1], np.abs(m)))


def sum_loop_f32(ptr, perm, m):
    """y [N, C] float32: per row, in p order, ``acc = acc + m[perm[p]]`` - the kernel's adds, one by one"""
    y = np.zeros((len(ptr) - 1, m.shape[1]), np.float32)
    for i in range(len(ptr) - 1):
        acc = y[i]
        for p in range(ptr[i], ptr[i + 1]):
            acc += m[perm[p]]
    return y


# --------------------------------------------------------------------------- #
# the restatement as a torch module (float32: ref32, .double(): truth64)
# --------------------------------------------------------------------------- #
class RefEdgeConv(nn.Module):
    def __init__(self, inner, aggr="max"):
        super().__init__()
        self.nn, self.aggr = inner, aggr

    def messages(self, x, edge_index):
        j, i = edge_index
        return self.nn(torch.cat([x[i], x[j] - x[i]], dim=1))

    def forward(self, x, edge_index):
        i, n = edge_index[1], x.size(0)
        msg = self.messages(x, edge_index)
        zeros = msg.new_zeros((n, msg.size(1)))
        if self.aggr == "max":
            with torch.no_grad():                                # mask and cnt are constants: the even split
                y, _ = segment_max(n, i.numpy(), msg.numpy())
                mask = (msg == torch.from_numpy(y)[i]).to(msg.dtype)
                cnt = zeros.clone().index_add_(0, i, mask)
            return zeros.index_add_(0, i, mask * msg / cnt[i].clamp(min=1))
        out = zeros.index_add_(0, i, msg)
        if self.aggr == "mean":
            out = out / torch.bincount(i, minlength=n).clamp(min=1).to(msg.dtype)[:, None]
        return out


def _ref_run(mod, x, ei, gup, dtype):
    for p in mod.parameters():
        p.grad = None
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    out = mod(xt, torch.from_numpy(ei))
    (out * torch.from_numpy(gup).to(dtype)).sum().backward()
    grads = {"x": xt.grad.numpy()}
    grads.update({name: p.grad.detach().numpy().copy() for name, p in mod.named_parameters()})
    return out.detach().numpy(), grads


def make_inner(fi, fo, seq):
    return nn.Sequential(nn.Linear(2 * fi, HIDDEN), nn.ReLU(), nn.Linear(HIDDEN, fo)) if seq else nn.Linear(2 * fi, fo)


@functools.lru_cache(maxsize=None)
def layer_case(fi, fo, aggr, seq, kind):
    """inputs, the reference module and its float32 / float64 results of one EdgeConv case; ``exact``: grid inputs
    and grid parameters (every max case, every Sequential case)"""
    torch.set_num_threads(1)
    n, ei = _graph(kind, 3)
    rng = np.random.default_rng(fi + fo + len(aggr) + 7 * seq)
    gup = rng.uniform(0.5, 1.5, (n, fo)).astype(np.float32)
    torch.manual_seed(12)
    cpu = RefEdgeConv(make_inner(fi, fo, seq), aggr)
    exact = aggr == "max" or seq
    if exact:
        x = grid_values(rng, (n, fi))
        with torch.no_grad():
            for p in cpu.parameters():
                p.copy_(torch.from_numpy(grid_weights(rng, tuple(p.shape))))
    else:
        x = rng.standard_normal((n, fi)).astype(np.float32)
    r32 = _ref_run(cpu, x, ei, gup, torch.float32)
    r64 = _ref_run(copy.deepcopy(cpu).double(), x, ei, gup, torch.float64)
    y_max = None
    if aggr == "max":                                            # the maximum of exact messages: an exact float32 itself
        with torch.no_grad():
            y_max = segment_max(n, ei[1], cpu.messages(torch.from_numpy(x), torch.from_numpy(ei)).numpy())[0]
    return dict(n=n, ei=ei, x=x, gup=gup, cpu=cpu, aggr=aggr, exact=exact, r32=r32, r64=r64, y_max=y_max)


def _layer_cases(graphs):
    return [(fi, fo, aggr, seq, kind) for (fi, fo) in SHAPES for aggr in AGGRS for seq in (False, True) for kind in graphs]


def check_against_references(tag, got, case, side):
    """output and gradients of one evaluation (``side``: "e_o" the float32 restatement against float64, "e_h" the
    device) against the references at 1e-5"""
    (o, g), (o32, g32), (o64, g64) = got, case["r32"], case["r64"]
    assert set(g) == set(g32), (tag, sorted(g), sorted(g32))
    for name, a, a32, a64 in [("forward", o, o32, o64)] + [(k + ".grad", g[k], g32[k], g64[k]) for k in g32]:
        assert a is not None, (tag, name)
        assert a.shape == a32.shape, (tag, name, a.shape, a32.shape)
        if side == "e_o":
            # a check of the REFERENCE, not of the library: torch's float32 index_add_ adds the hub's 5,000 terms one
            # by one, uncompensated, so the restatement's own x.grad is up to 1.2e-5 from float64 there; 1e-4 only
            # says that the two restatements state the same maths.  The device is held to 1e-5 (assert_parity: of
            # the float32 restatement or, failing that, of float64 - never anything wider).
            d = rel_err(a32, a64)
            record_parity(f"{tag} {name}", None, e_o=d)
            assert d < 1e-4, (tag, name, d)
        else:
            assert_parity(a, a32, a64, TOL, f"{tag} {name}")


# --------------------------------------------------------------------------- #
# CPU
# --------------------------------------------------------------------------- #
def test_constructor_repr_state_dict_and_reset_parameters():
    seq = nn.Sequential(nn.Linear(42, 32), nn.ReLU(), nn.Linear(32, 64))
    conv = dc.nn.EdgeConv(seq)
    assert conv.aggr == "max" and conv.nn is seq
    assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == {
        "nn.0.weight": (32, 42), "nn.0.bias": (32,), "nn.2.weight": (64, 32), "nn.2.bias": (64,)}
    assert repr(conv).startswith("EdgeConv(nn=Sequential(") and repr(dc.nn.EdgeConv(nn.Linear(6, 4))).startswith(
        "EdgeConv(nn=Linear(")
    assert conv.graph_flags() == dict(self_loops=False, normalize=False)
    assert not hasattr(conv, "supports_fused_relu") and not hasattr(conv, "bias") and not hasattr(conv, "lin")
    ref = RefEdgeConv(copy.deepcopy(seq))
    assert set(ref.state_dict()) == set(conv.state_dict())
    with torch.no_grad():
        for p in ref.parameters():
            p.add_(1.0)
    conv.load_state_dict(ref.state_dict(), strict=True)
    back = dc.nn.EdgeConv(copy.deepcopy(seq), aggr="mean")
    back.load_state_dict(conv.state_dict(), strict=True)         # round trip
    for k, v in ref.state_dict().items():
        assert torch.equal(conv.state_dict()[k], v) and torch.equal(back.state_dict()[k], v), k
    before = [p.detach().clone() for p in conv.parameters()]
    conv.reset_parameters()
    after = [p.detach() for p in conv.parameters()]
    assert len(after) == 4 and all(not torch.equal(a, b) for a, b in zip(after, before))
    # the second positional argument is aggr, as in PyG
    assert dc.nn.EdgeConv(nn.Linear(6, 4), "mean").aggr == "mean"


def test_aggr_is_validated_and_add_is_sum():
    for aggr, want in (("max", "max"), ("mean", "mean"), ("sum", "sum"), ("add", "sum")):
        assert dc.nn.EdgeConv(nn.Linear(6, 4), aggr=aggr).aggr == want
    for bad in ("min", "mul", "", None, 2, ["max"], ["max", "mean"], ("sum",), nn.Identity()):
        with pytest.raises(ValueError, match="aggr"):
            dc.nn.EdgeConv(nn.Linear(6, 4), aggr=bad)


def test_errors_raised_on_the_host():
    x, ei = torch.zeros(5, 3), torch.zeros(2, 4, dtype=torch.long)
    conv = dc.nn.EdgeConv(nn.Linear(6, 2))
    for pair in ((x, x), [x, x], (x, None)):
        with pytest.raises(TypeError, match="bipartite"):
            conv(pair, ei)
    for unsupported in (dict(size=(5, 5)), dict(relu=True), dict(next_conv=None), dict(edge_attr=None)):
        with pytest.raises(TypeError):
            conv(x, ei, **unsupported)                           # not supported: absent from the signature
    with pytest.raises(RuntimeError, match="HIP device"):
        conv(x, ei)                                              # every host check passed: no CPU path
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.edge_pairs(None, x)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.edge_aggregate(None, torch.zeros(4, 2))
    for reduce in AGGRS:
        with pytest.raises(RuntimeError, match="HIP device"):
            ops.edge_aggregate(None, torch.zeros(4, 2), reduce)
    # the reduce check comes before anything else, the device check included
    for bad in ("add", "min", None, 3, ["max"]):
        with pytest.raises(ValueError, match="reduce must be"):
            ops.edge_aggregate(None, torch.zeros(4, 2), bad)
        with pytest.raises(ValueError, match="reduce must be"):
            ops.edge_aggregate(None, "not a tensor", bad)


def test_exports_and_the_torch_geometric_alias():
    import sys
    from deformcontact_amd.pyg_alias import install_as_torch_geometric
    names = dc.nn.__all__
    assert names.count("EdgeConv") == 1 and names.index("EdgeConv") == names.index("GINEConv") + 1
    assert names[-3:] == ["SplineConv", "GMMConv", "ChebConv"] and dc.nn.EdgeConv is EdgeConv
    mods = ("torch_geometric", "torch_geometric.nn", "torch_geometric.data")
    saved = {k: sys.modules.get(k) for k in mods}
    try:
        install_as_torch_geometric(force=True)
        from torch_geometric.nn import EdgeConv as aliased
        assert aliased is dc.nn.EdgeConv
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def _entry_calls():
    """name -> call(rows, width, pointers given?, leading dimension, mode) of every entry of dc_edge.hip, otherwise
    valid; ``rows`` is the entry's row count (E for the entries that walk the input edges, N for the others)"""
    L = _lib.lib()
    p = lambda ok, a=64: a if ok else None                      # any non-null address: rejected calls never touch it
    return {
        "dc_edge_pair_fwd": lambda r, f, ok, ld, mode=0: L.dc_edge_pair_fwd(
            p(ok), p(ok), p(ok, 128), ld, p(ok, 256), 2 * ld, 3, r, f, None),
        "dc_edge_pair_bwd": lambda r, f, ok, ld, mode=0: L.dc_edge_pair_bwd(
            p(ok), p(ok), p(ok), p(ok), p(ok, 128), 2 * ld, p(ok, 256), ld, r, f, None),
        "dc_edge_reduce_fwd": lambda r, f, ok, ld, mode=0: L.dc_edge_reduce_fwd(
            p(ok), p(ok), p(ok, 128), ld, p(ok, 256), ld, p(ok and mode == 2, 320), ld, mode, r, f, None),
        "dc_edge_reduce_bwd": lambda r, f, ok, ld, mode=0: L.dc_edge_reduce_bwd(
            p(ok), p(ok), p(ok), p(ok and mode == 2, 128), ld, p(ok and mode == 2, 256), ld, p(ok and mode == 2, 320), ld,
            p(ok, 384), ld, p(ok, 448), ld, mode, 3, r, f, None),
    }


def test_abi_argument_errors_of_the_edge_entries_without_gpu():
    """short leading dimensions, null pointers, aliased outputs, a bad mode, cnt given for a sum or missing for the
    max, sizes out of range: -1 and the entry's own message, before any HIP call; a zero row count returns 0 with no
    pointer at all."""
    L = _lib.lib()
    calls = _entry_calls()
    declared = [n for n in _lib.exported_names() if n.startswith("dc_edge_")]
    assert sorted(declared) == sorted(calls)
    for name, call in calls.items():
        modes = (0, 1, 2) if "reduce" in name else (0,)
        for mode in modes:
            assert call(3, 16, False, 64, mode) == -1 and name.encode() in L.dc_last_error() \
                and b"null" in L.dc_last_error(), (name, mode)
            assert call(3, 16, True, 15, mode) == -1 and name.encode() in L.dc_last_error() \
                and b"leading" in L.dc_last_error(), (name, mode)
            assert call(3, 16, False, 15, mode) == -1 and b"leading" in L.dc_last_error(), name   # sizes, strides, nulls
            assert call(0, 16, False, 64, mode) == 0, (name, mode)   # no row: nothing is read, written or launched
            assert call(0, 16, False, 15, mode) == -1, (name, mode)
        assert call(-1, 16, True, 64) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, 0, True, 64) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, -2, True, 64) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, 1 << 24, True, 1 << 24) == -1 and b"range" in L.dc_last_error(), name
        assert call(1 << 30, 16, True, 64) == -1 and b"range" in L.dc_last_error(), name
        if "reduce" in name:
            for mode in (-1, 3, 7):
                assert call(3, 16, True, 64, mode) == -1 and b"mode" in L.dc_last_error() \
                    and name.encode() in L.dc_last_error(), (name, mode)
                assert call(0, 16, False, 64, mode) == -1 and b"mode" in L.dc_last_error(), (name, mode)
    # the pair rows are 2F wide: z and gz need a leading dimension of 2F, and 2F must be in range
    assert L.dc_edge_pair_fwd(64, 64, 128, 16, 256, 31, 3, 5, 16, None) == -1 and b"leading" in L.dc_last_error()
    assert L.dc_edge_pair_bwd(64, 64, 64, 64, 128, 31, 256, 16, 3, 16, None) == -1 and b"leading" in L.dc_last_error()
    assert L.dc_edge_pair_fwd(64, 64, 128, 1 << 23, 256, 1 << 24, 3, 5, 1 << 23, None) == -1 and b"range" in L.dc_last_error()
    assert L.dc_edge_pair_fwd(64, 64, 128, 16, 256, 32, 3, -1, 16, None) == -1 and b"range" in L.dc_last_error()
    assert L.dc_edge_reduce_bwd(64, 64, 64, None, 16, None, 16, None, 16, 384, 16, 448, 16, 0, 3, -1, 16, None) == -1
    assert b"range" in L.dc_last_error()
    # outputs that alias an operand
    assert L.dc_edge_pair_fwd(64, 64, 128, 16, 128, 32, 3, 5, 16, None) == -1 and b"alias" in L.dc_last_error()
    assert L.dc_edge_pair_bwd(64, 64, 64, 64, 128, 32, 128, 16, 3, 16, None) == -1 and b"alias" in L.dc_last_error()
    assert L.dc_edge_reduce_fwd(64, 64, 128, 16, 128, 16, None, 16, 0, 3, 16, None) == -1 and b"alias" in L.dc_last_error()
    assert L.dc_edge_reduce_fwd(64, 64, 128, 16, 256, 16, 128, 16, 2, 3, 16, None) == -1 and b"alias" in L.dc_last_error()
    assert L.dc_edge_reduce_fwd(64, 64, 128, 16, 256, 16, 256, 16, 2, 3, 16, None) == -1 and b"alias" in L.dc_last_error()
    assert L.dc_edge_reduce_bwd(64, 64, 64, None, 16, None, 16, None, 16, 384, 16, 384, 16, 0, 3, 5, 16, None) == -1
    assert b"alias" in L.dc_last_error()
    for k, other in enumerate((128, 256, 320)):                  # gm on m, y, cnt of the max
        assert L.dc_edge_reduce_bwd(64, 64, 64, 128, 16, 256, 16, 320, 16, 384, 16, other, 16, 2, 3, 5, 16, None) == -1
        assert b"alias" in L.dc_last_error(), k
    # cnt: written by the max only
    for mode in (0, 1):
        assert L.dc_edge_reduce_fwd(64, 64, 128, 16, 256, 16, 320, 16, mode, 3, 16, None) == -1
        assert b"cnt" in L.dc_last_error() and b"dc_edge_reduce_fwd" in L.dc_last_error()
    assert L.dc_edge_reduce_fwd(64, 64, 128, 16, 256, 16, None, 16, 2, 3, 16, None) == -1
    assert b"cnt" in L.dc_last_error() and b"null" in L.dc_last_error()
    assert L.dc_edge_reduce_bwd(64, 64, 64, 128, 16, 256, 16, None, 16, 384, 16, 448, 16, 2, 3, 5, 16, None) == -1
    assert b"null" in L.dc_last_error()
    assert L.dc_edge_reduce_bwd(64, 64, None, None, 16, None, 16, None, 16, 384, 16, 448, 16, 1, 3, 5, 16, None) == -1
    assert b"null" in L.dc_last_error()                          # the mean reads ptr


def test_float32_restatement_within_the_bar_of_float64_and_exact_where_it_has_to_be():
    """Every layer case of the GPU tests: the float32 and the float64 restatement agree, output and every gradient; in
    the exact cases the messages - and with them every selection - are the same numbers in float32 and float64,
    and the max cases do hold ties."""
    for fi, fo, aggr, seq, kind in _layer_cases(MAIN_GRAPHS + EDGE_GRAPHS):
        case = layer_case(fi, fo, aggr, seq, kind)
        tag = f"RefEdgeConv fp32 vs fp64 {fi}->{fo} {aggr} seq={seq} {kind}"
        check_against_references(tag, case["r32"], case, "e_o")
        assert case["r32"][0].shape == (case["n"], fo)
        if case["exact"]:
            with torch.no_grad():
                tei = torch.from_numpy(case["ei"])
                m32 = case["cpu"].messages(torch.from_numpy(case["x"]), tei)
                m64 = copy.deepcopy(case["cpu"]).double().messages(torch.from_numpy(case["x"]).double(), tei)
            assert torch.equal(m32.double(), m64), tag
            if aggr == "max" and kind in MAIN_GRAPHS:
                _, cnt = segment_max(case["n"], case["ei"][1], m32.numpy())
                assert (cnt >= 2).any(), tag


def test_reference_formulas_agree_with_autograd():
    """the pair backward's float64 sum of fp32 differences against float64 autograd of the torch composition: they
    differ by the rounding of the differences alone, at most 2^-24 of the sum of the terms' absolute values - which,
    where a row's terms cancel (F = 1: up to 1.7e-5 of the row's value), is more than 1e-5 of the row itself, hence
    the metric of the ``ops`` node below; the hand-written reduce gradients equal autograd through the mask / count
    form in float64"""
    for kind in MAIN_GRAPHS:
        for f in PAIR_WIDTHS:
            case = pair_case(kind, f)
            assert term_rel_err(case["gx64"], case["gx_autograd64"], case["abs64"]) <= U32, (kind, f)
        case = reduce_case(kind, 20)
        n, ei = case["n"], case["ei"]
        assert (case["deg"] == 0).any() and case["deg"].max() >= (HUB - 1 if kind == "seg" else 8)
        assert (case["cnt"][case["deg"] == 0] == 0).all() and (case["cnt"][case["deg"] > 0] >= 1).all()
        assert (case["cnt"] >= 2).mean() > 0.1                  # ties
        i = torch.from_numpy(ei[1])
        for mode, values in (("sum", "m"), ("mean", "m"), ("max", "mg")):
            mt = torch.from_numpy(case[values]).double().requires_grad_(True)
            zeros = torch.zeros((n, 20), dtype=torch.float64)
            if mode == "max":
                mask = (mt.detach() == torch.from_numpy(case["y"]).double()[i]).double()
                cnt = zeros.clone().index_add_(0, i, mask)
                assert torch.equal(cnt, torch.from_numpy(case["cnt"]).double())
                out = zeros.index_add_(0, i, mask * mt / cnt[i].clamp(min=1))
                assert rel_err(out.detach().numpy(), case["y"]) < 1e-14     # (cnt shares of y / cnt, summed)
            else:
                out = zeros.index_add_(0, i, mt)
                if mode == "mean":
                    out = out / torch.from_numpy(np.maximum(case["deg"], 1)).double()[:, None]
            (out * torch.from_numpy(case["gy"]).double()).sum().backward()
            assert rel_err(case["gm"][mode], mt.grad.numpy()) < 1e-6, (kind, mode)


# --------------------------------------------------------------------------- #
# GPU: the entries called directly
# --------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def _device_graph(kind):
    """the adjacency of the direct cases of ``kind`` and its forward side read back: (g, ptr, perm)"""
    n, ei = _graph(kind, 9)
    g = GraphIndex(torch.from_numpy(ei).to(DEV), n, self_loops=False, normalize=False, validate=True)
    ne = ei.shape[1]
    ptr, perm = (_np(t).astype(np.int64) for t in (g.fwd.ptr, g.fwd.perm[:ne]))
    # the device's own sorted set: perm is a bijection over the input edges and names each position's edge
    assert ptr[0] == 0 and ptr[-1] == ne and np.array_equal(np.sort(perm), np.arange(ne))
    assert np.array_equal(ei[1][perm], np.repeat(np.arange(n), np.diff(ptr)))
    tperm, tptr = _np(g.bwd.perm[:ne]).astype(np.int64), _np(g.bwd.ptr).astype(np.int64)
    assert np.array_equal(np.sort(tperm), np.arange(ne)) and np.array_equal(ei[0][tperm], np.repeat(np.arange(n), np.diff(tptr)))
    return g, ptr, perm


@functools.lru_cache(maxsize=None)
def _sum_f32(kind, c):
    _, ptr, perm = _device_graph(kind)
    return sum_loop_f32(ptr, perm, reduce_case(kind, c)["m"])


def _wide(t, pad=12, off=4):
    """``t`` as a column slice of a wider buffer (row stride > width; rows stay 16-byte aligned)"""
    buf = torch.full((t.size(0), t.size(1) + pad), 3 if t.dtype == torch.int32 else 1e30, dtype=t.dtype, device=t.device)
    buf[:, off:off + t.size(1)] = t
    return buf[:, off:off + t.size(1)]


def _odd(t):
    """``t`` as a column slice whose rows are NOT 16-byte aligned (the general form at every width)"""
    buf = torch.full((t.size(0), t.size(1) + 3), 3 if t.dtype == torch.int32 else 1e30, dtype=t.dtype, device=t.device)
    buf[:, 1:1 + t.size(1)] = t
    return buf[:, 1:1 + t.size(1)]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _within_bar_of_float64(got, want64, name):
    d = row_rel_err(got, want64)
    print(f"{name}: row_rel_err vs float64 = {d:.3e}")
    record_parity(name, None, e_h=d, metric="row_rel_err")
    assert d < TOL, (name, d)


@gpu
@pytest.mark.parametrize("kind", MAIN_GRAPHS)
@pytest.mark.parametrize("f", PAIR_WIDTHS)
def test_pair_forward_entry(f, kind):
    """bit-identical to numpy; x as a column slice (aligned and not): the same bits; z a slice of a wider buffer: the
    same values and nothing beside them; ``ops.edge_pairs``: the same bits; twice: the same bits"""
    case = pair_case(kind, f)
    g, n, ne = _device_graph(kind)[0], case["n"], case["ei"].shape[1]
    x = _dev(case["x"])
    z = ops._edge_pair_fwd(g, x)
    assert z.shape == (ne, 2 * f) and np.array_equal(_np(z), case["z"]), (f, kind)
    assert torch.equal(z, ops._edge_pair_fwd(g, x)) and torch.equal(z, ops.edge_pairs(g, x))
    assert torch.equal(z, ops._edge_pair_fwd(g, _wide(x))) and torch.equal(z, ops._edge_pair_fwd(g, _odd(x)))
    assert torch.equal(z, ops.edge_pairs(g, _wide(x))) and torch.equal(z, ops.edge_pairs(g, _odd(x)))
    L, ei = _lib.lib(), g.edge_index
    for ld, off in ((2 * f + 8, 4), (2 * f + 3, 1)):             # rows 16-byte aligned where 2F is, and not
        buf = torch.full((ne, ld), 7.0, device=DEV)
        o_z, xs = buf[:, off:off + 2 * f], _wide(x)
        _lib.check(L.dc_edge_pair_fwd(ei[0].data_ptr(), ei[1].data_ptr(), xs.data_ptr(), xs.stride(0), o_z.data_ptr(), ld,
                                      n, ne, f, _st()), "dc_edge_pair_fwd")
        assert torch.equal(o_z, z) and (buf[:, :off] == 7.0).all() and (buf[:, off + 2 * f:] == 7.0).all()


@gpu
@pytest.mark.parametrize("kind", MAIN_GRAPHS)
@pytest.mark.parametrize("f", PAIR_WIDTHS)
def test_pair_backward_entry_and_node(f, kind):
    """g_x within 1e-5 per row of the float64 sum of the same terms; g_z as a column slice, a strided output: the same
    bits; twice: the same bits; the ``ops`` node against the float64 autograd gradient of the torch composition, with a
    non-contiguous and an expanded gradient: the bits of a contiguous one"""
    case = pair_case(kind, f)
    g, n = _device_graph(kind)[0], case["n"]
    x, gz = _dev(case["x"]), _dev(case["gz"])
    gx = ops._edge_pair_bwd(g, gz)
    assert gx.shape == (n, f)
    _within_bar_of_float64(_np(gx), case["gx64"], f"edge pair g_x F={f} {kind}")
    assert torch.equal(gx, ops._edge_pair_bwd(g, gz))
    assert torch.equal(gx, ops._edge_pair_bwd(g, _wide(gz))) and torch.equal(gx, ops._edge_pair_bwd(g, _odd(gz)))
    deg = np.bincount(case["ei"][1], minlength=n) + np.bincount(case["ei"][0], minlength=n)
    assert (gx[_dev(deg == 0)] == 0).all()                       # a node without edges
    L, ld = _lib.lib(), f + 8
    o_x = torch.full((n, ld), 7.0, device=DEV)
    _lib.check(L.dc_edge_pair_bwd(g.fwd.ptr.data_ptr(), g.fwd.perm.data_ptr(), g.bwd.ptr.data_ptr(), g.bwd.perm.data_ptr(),
                                  gz.data_ptr(), 2 * f, o_x.data_ptr(), ld, n, f, _st()), "dc_edge_pair_bwd")
    assert torch.equal(o_x[:, :f], gx) and (o_x[:, f:] == 7.0).all()
    # through autograd
    xs = _wide(x).detach().requires_grad_(True)
    torch.autograd.backward([ops.edge_pairs(g, xs)], [gz])
    assert torch.equal(xs.grad, gx)
    # against float64 autograd of the torch composition: 1e-5 of the tensor's scale, and per element 4 * 2^-24 of the
    # sum of the terms' absolute values (one rounding per fp32 difference, two of the compensated sum, one stored)
    d = rel_err(_np(xs.grad), case["gx_autograd64"])
    t = term_rel_err(_np(xs.grad), case["gx_autograd64"], case["abs64"])
    print(f"edge_pairs x.grad F={f} {kind}: rel_err = {d:.3e}, per-term error = {t / U32:.2f} x 2^-24")
    record_parity(f"edge_pairs x.grad F={f} {kind}", None, e_h=d)
    assert d < TOL and t <= 4 * U32, (f, kind, d, t)
    wide_g = torch.full((gz.size(0), 4 * f), 1e30, device=DEV)
    wide_g[:, ::2] = gz
    for strided in (wide_g[:, ::2], _wide(gz), _odd(gz)):
        assert not strided.is_contiguous()
        xs.grad = None
        torch.autograd.backward([ops.edge_pairs(g, xs)], [strided])
        assert torch.equal(xs.grad, gx)
    xs.grad = None
    ops.edge_pairs(g, xs).sum().backward()                       # an expanded gradient of ones
    assert torch.equal(xs.grad, ops._edge_pair_bwd(g, torch.ones_like(gz)))


@gpu
@pytest.mark.parametrize("kind", MAIN_GRAPHS)
@pytest.mark.parametrize("c", REDUCE_WIDTHS)
def test_reduce_forward_entry(c, kind):
    """sum bit-identical to the float32 loop over the device's own sorted set and within a plain sum's bound of float64; mean
    that sum divided by ``np.float32(deg)``, bit for bit; max: y and cnt equal element for element on the coarse grid;
    m as a column slice, strided outputs: the same bits; ``ops.edge_aggregate``: the same bits"""
    case = reduce_case(kind, c)
    g, n, deg = _device_graph(kind)[0], case["n"], case["deg"]
    s32 = _sum_f32(kind, c)
    m, mg = _dev(case["m"]), _dev(case["mg"])
    y, none = ops._edge_reduce_fwd(g, m, 0)
    assert none is None and np.array_equal(_np(y), s32), (c, kind)
    # against float64: a plain fp32 sum of deg terms is within (deg - 1) * 2^-24 of the sum of their absolute values
    t = term_rel_err(_np(y), case["sum64"], case["abs64"] * np.maximum(deg - 1, 1)[:, None])
    print(f"edge reduce sum C={c} {kind}: error = {t / U32:.3f} x (deg - 1) x 2^-24 of the terms' absolute sum")
    assert rel_err(_np(y), case["sum64"]) < TOL and t <= U32, (c, kind, t)
    mean, none = ops._edge_reduce_fwd(g, m, 1)
    want = np.where(deg[:, None] > 0, s32 / np.maximum(deg, 1).astype(np.float32)[:, None], np.float32(0))
    assert none is None and want.dtype == np.float32 and np.array_equal(_np(mean), want), (c, kind)
    mx, cnt = ops._edge_reduce_fwd(g, mg, 2)
    assert cnt.dtype == torch.int32 and cnt.shape == (n, c)
    assert np.array_equal(_np(mx), case["y"]) and np.array_equal(_np(cnt), case["cnt"]), (c, kind)
    assert (mx[_dev(deg == 0)] == 0).all() and (cnt[_dev(deg == 0)] == 0).all() and (y[_dev(deg == 0)] == 0).all()
    for mode, src, want_y in ((0, m, y), (1, m, mean), (2, mg, mx)):
        for view in (src, _wide(src), _odd(src)):
            yy, cc = ops._edge_reduce_fwd(g, view, mode)
            assert torch.equal(yy, want_y) and (mode != 2 or torch.equal(cc, cnt)), (mode, c, kind)
        assert torch.equal(want_y, ops.edge_aggregate(g, src, ("sum", "mean", "max")[mode]))
        assert torch.equal(want_y, ops.edge_aggregate(g, _odd(src), ("sum", "mean", "max")[mode]))
    # strided OUTPUTS: the same values and nothing beside them
    L, ld = _lib.lib(), c + 8
    for mode, src, want_y in ((0, m, y), (1, m, mean), (2, mg, mx)):
        o_y = torch.full((n, ld), 7.0, device=DEV)
        o_c = torch.full((n, ld), 7, dtype=torch.int32, device=DEV) if mode == 2 else None
        _lib.check(L.dc_edge_reduce_fwd(g.fwd.ptr.data_ptr(), g.fwd.perm.data_ptr(), src.data_ptr(), c, o_y.data_ptr(), ld,
                                        o_c.data_ptr() if mode == 2 else None, ld, mode, n, c, _st()), "dc_edge_reduce_fwd")
        assert torch.equal(o_y[:, :c], want_y) and (o_y[:, c:] == 7.0).all()
        if mode == 2:
            assert torch.equal(o_c[:, :c], cnt) and (o_c[:, c:] == 7).all()


@gpu
@pytest.mark.parametrize("kind", MAIN_GRAPHS)
@pytest.mark.parametrize("c", REDUCE_WIDTHS)
def test_reduce_backward_entry_and_node(c, kind):
    """sum, mean and max bit-identical to the numpy float32 formula; operands as column slices, a strided output: the
    same bits; through autograd with a contiguous, a non-contiguous and an expanded gradient: the same bits"""
    case = reduce_case(kind, c)
    g, n, ne = _device_graph(kind)[0], case["n"], case["ei"].shape[1]
    m, mg, gy = _dev(case["m"]), _dev(case["mg"]), _dev(case["gy"])
    y, cnt = _dev(case["y"]), _dev(case["cnt"])
    L, ld, ei = _lib.lib(), c + 8, g.edge_index
    for name, mode in MODES.items():
        src = mg if mode == 2 else m
        sv = (src, y, cnt) if mode == 2 else (None, None, None)
        gm = ops._edge_reduce_bwd(g, *sv, gy, mode)
        assert gm.shape == (ne, c) and np.array_equal(_np(gm), case["gm"][name]), (name, c, kind)
        assert torch.equal(gm, ops._edge_reduce_bwd(g, *sv, gy, mode))
        assert torch.equal(gm, ops._edge_reduce_bwd(g, *sv, _wide(gy), mode))
        assert torch.equal(gm, ops._edge_reduce_bwd(g, *sv, _odd(gy), mode))
        if mode == 2:
            assert torch.equal(gm, ops._edge_reduce_bwd(g, _wide(src), _wide(y), _wide(cnt), gy, mode))
            assert torch.equal(gm, ops._edge_reduce_bwd(g, _odd(src), y, _odd(cnt), _odd(gy), mode))
            # the shares of every maximum add up to its gradient: nothing is lost or counted twice
            total = _index_add(n, case["ei"][1], _np(gm))
            hit = case["cnt"] > 0
            assert np.abs(total[hit] - case["gy"][hit]).max() < 1e-5 * 1.5 and (total[~hit] == 0).all()
        o_g = torch.full((ne, ld), 7.0, device=DEV)
        ptrs = [t.data_ptr() for t in sv] if mode == 2 else [None, None, None]
        _lib.check(L.dc_edge_reduce_bwd(ei[0].data_ptr(), ei[1].data_ptr(), g.fwd.ptr.data_ptr(), ptrs[0], c, ptrs[1], c,
                                        ptrs[2], c, gy.data_ptr(), c, o_g.data_ptr(), ld, mode, n, ne, c, _st()),
                   "dc_edge_reduce_bwd")
        assert torch.equal(o_g[:, :c], gm) and (o_g[:, c:] == 7.0).all()
        # through autograd
        ms = _wide(src).detach().requires_grad_(True)
        wide_g = torch.full((n, 2 * c), 1e30, device=DEV)
        wide_g[:, ::2] = gy
        for grad in (gy, wide_g[:, ::2], _wide(gy), _odd(gy)):
            ms.grad = None
            torch.autograd.backward([ops.edge_aggregate(g, ms, name)], [grad])
            assert torch.equal(ms.grad, gm), (name, c, kind)
        ms.grad = None
        ops.edge_aggregate(g, ms, name).sum().backward()         # an expanded gradient of ones
        out = ops.edge_aggregate(g, src, name)
        assert torch.equal(ms.grad, ops._edge_reduce_bwd(g, *((src, out, cnt) if mode == 2 else sv), torch.ones_like(gy),
                                                         mode))


@gpu
def test_edges_with_an_endpoint_out_of_range_get_a_zero_row():
    """the two per-edge entries called on an edge list that names nodes outside [0, N): those rows are zeros, the
    others are not touched by it"""
    n, f = 20, 12
    rng = np.random.default_rng(2)
    ei = rng.integers(0, n, (2, 64))
    bad = np.zeros(64, bool)
    ei[0, 3], ei[1, 7], ei[0, 11], ei[1, 12], bad[[3, 7, 11, 12]] = n, n + 5, -1, -3, True
    x, gy = rng.standard_normal((n, f)).astype(np.float32), rng.standard_normal((n, f)).astype(np.float32)
    tei, tx, tgy = torch.from_numpy(ei).to(DEV), _dev(x), _dev(gy)
    L = _lib.lib()
    z = torch.full((64, 2 * f), 7.0, device=DEV)
    _lib.check(L.dc_edge_pair_fwd(tei[0].data_ptr(), tei[1].data_ptr(), tx.data_ptr(), f, z.data_ptr(), 2 * f, n, 64, f,
                                  _st()), "dc_edge_pair_fwd")
    src, dst = np.where(bad, 0, ei[0]), np.where(bad, 0, ei[1])
    want = np.where(bad[:, None], np.float32(0), np.concatenate([x[dst], x[src] - x[dst]], axis=1))
    assert np.array_equal(_np(z), want)
    ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(dst[~bad], minlength=n))]).astype(np.int32)).to(DEV)
    deg = np.maximum(np.bincount(dst[~bad], minlength=n), 1).astype(np.float32)
    for mode, want in ((0, gy[dst]), (1, gy[dst] / deg[dst][:, None])):
        gm = torch.full((64, f), 7.0, device=DEV)
        _lib.check(L.dc_edge_reduce_bwd(tei[0].data_ptr(), tei[1].data_ptr(), ptr.data_ptr(), None, f, None, f, None, f,
                                        tgy.data_ptr(), f, gm.data_ptr(), f, mode, n, 64, f, _st()), "dc_edge_reduce_bwd")
        assert np.array_equal(_np(gm), np.where(bad[:, None], np.float32(0), want)), mode


@gpu
def test_ops_with_no_rows_and_with_no_edges_and_their_checks():
    """E = 0 or N = 0: empty or zero results without a launch, gradients of the right shape; the host checks"""
    L = _lib.lib()
    assert L.dc_edge_pair_fwd(None, None, None, 15, None, 30, 0, 0, 15, None) == 0
    assert L.dc_edge_pair_bwd(None, None, None, None, None, 30, None, 15, 0, 15, None) == 0
    assert L.dc_edge_reduce_fwd(None, None, None, 15, None, 15, None, 15, 2, 0, 15, None) == 0
    assert L.dc_edge_reduce_bwd(None, None, None, None, 15, None, 15, None, 15, None, 15, None, 15, 2, 0, 0, 15, None) == 0
    x0 = torch.zeros((0, 15), device=DEV, requires_grad=True)
    z0 = ops.edge_pairs(None, x0)
    assert z0.shape == (0, 30) and z0.requires_grad
    z0.sum().backward()
    assert x0.grad.shape == (0, 15)
    for reduce in AGGRS:
        m0 = torch.zeros((0, 7), device=DEV, requires_grad=True)
        y0 = ops.edge_aggregate(None, m0, reduce)
        assert y0.shape == (0, 7)
        y0.sum().backward()
        assert m0.grad.shape == (0, 7)
    n, f = 37, 15
    g = GraphIndex(torch.zeros((2, 0), dtype=torch.int64, device=DEV), n, self_loops=False, normalize=False)
    x = torch.randn(n, f, device=DEV, requires_grad=True)
    z = ops.edge_pairs(g, x)
    assert z.shape == (0, 2 * f)
    z.sum().backward()
    assert x.grad.shape == (n, f) and (x.grad == 0).all()
    for reduce in AGGRS:
        m = torch.zeros((0, 7), device=DEV, requires_grad=True)
        y = ops.edge_aggregate(g, m, reduce)
        assert y.shape == (n, 7) and (y == 0).all()
        y.sum().backward()
        assert m.grad.shape == (0, 7)
    xd = x.detach()
    with pytest.raises(ValueError, match="None"):
        ops.edge_pairs(None, xd)
    with pytest.raises(ValueError, match="None"):
        ops.edge_aggregate(None, torch.zeros((3, f), device=DEV))
    with pytest.raises(ValueError, match="rows"):
        ops.edge_pairs(g, xd[:5])
    with pytest.raises(ValueError, match="3 rows.*0 edges"):
        ops.edge_aggregate(g, torch.zeros((3, f), device=DEV))   # both numbers are named
    for bad in (xd.double(), xd[0], torch.zeros((n, 0), device=DEV)):
        with pytest.raises(ValueError):
            ops.edge_pairs(g, bad)
        with pytest.raises(ValueError):
            ops.edge_aggregate(g, bad)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.edge_pairs(g, xd.cpu())
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.edge_aggregate(g, torch.zeros((0, f)))
    loops = GraphIndex(torch.zeros((2, 0), dtype=torch.int64, device=DEV), n, self_loops=True, normalize=False)
    ei2 = torch.tensor([[0, 1, 2], [1, 2, 0]], device=DEV)
    merged = GraphIndex.from_parts([(ei2, 3), (ei2, 3)], self_loops=False, normalize=False)
    for bad, rows in ((loops, n), (merged, merged.num_nodes), (merged.window(1), 3)):
        with pytest.raises(ValueError, match="self_loops=False"):
            ops.edge_pairs(bad, torch.zeros((rows, f), device=DEV))
        with pytest.raises(ValueError, match="self_loops=False"):
            ops.edge_aggregate(bad, torch.zeros((bad.num_input_edges, f), device=DEV))


# --------------------------------------------------------------------------- #
# GPU: the layer
# --------------------------------------------------------------------------- #
class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, weight, bias):
        ctx.save_for_backward(z, weight)
        return torch.nn.functional.linear(z, weight, bias)

    @staticmethod
    def backward(ctx, g):
        z, weight = ctx.saved_tensors
        return g @ weight, (g.double().t() @ z.double()).float(), g.double().sum(0).float()


class Linear64(nn.Linear):
    """``torch.nn.Linear`` (same parameters, same forward) whose two reductions over the E edge rows - the gradients of
    weight and bias - are summed in float64.  These are sums INSIDE the user's module, not the layer's: on ``seg`` the
    hub's 5,000 edges send 5,000 identical terms, and a float32 GEMM that adds them one after the other drifts -
    measured with plain ``torch.nn.Linear`` on the device: weight.grad 6.0e-5 to 7.6e-5 from float64 for mean and sum
    at every shape on ``seg`` (the CPU restatement itself: 5.7e-5 at 3 -> 64) while forward and x.grad, the layer's own
    kernels, were inside 1e-5.  With the module's sums out of the way, the bar measures the layer."""

    def forward(self, z):
        return _LinearFn.apply(z, self.weight, self.bias)


def _device_nn(inner, plain=False):
    """``inner`` with the same parameters on the device, every Linear a ``Linear64`` (``plain``: as it is)"""
    def lin(m):
        if plain or not isinstance(m, nn.Linear):
            return copy.deepcopy(m)
        new = Linear64(m.in_features, m.out_features)
        new.load_state_dict(m.state_dict())
        return new
    mod = nn.Sequential(*[lin(m) for m in inner]) if isinstance(inner, nn.Sequential) else lin(inner)
    assert set(mod.state_dict()) == set(inner.state_dict())
    return mod


def _device_conv(case, plain=False):
    """the layer with the reference's parameters"""
    return dc.nn.EdgeConv(_device_nn(case["cpu"].nn, plain), aggr=case["aggr"]).to(DEV)


def _device_run(conv, x, ei, gup):
    for p in conv.parameters():
        p.grad = None
    xg = (x if isinstance(x, torch.Tensor) else _dev(x)).detach().requires_grad_(True)
    out = conv(xg, ei if isinstance(ei, torch.Tensor) else torch.from_numpy(ei).to(DEV))
    assert type(out) is torch.Tensor                             # the reduction's result: nothing deferred
    torch.autograd.backward([out], [gup if isinstance(gup, torch.Tensor) else _dev(gup)])
    torch.cuda.synchronize()
    grads = {"x": xg.grad}
    grads.update({name: p.grad for name, p in conv.named_parameters()})
    return out.detach(), grads


def _host(run):
    return _np(run[0]), {k: (None if v is None else _np(v)) for k, v in run[1].items()}


def _check_layer(fi, fo, aggr, seq, kind, plain=False):
    case = layer_case(fi, fo, aggr, seq, kind)
    clear_cache()
    conv = _device_conv(case, plain)
    tag = f"EdgeConv {fi}->{fo} {aggr} seq={seq} {kind}"
    if case["exact"] and case["ei"].shape[1]:
        # the precondition of one selection in every evaluation: the messages are the same numbers on the device
        with torch.no_grad():
            tei = torch.from_numpy(case["ei"]).to(DEV)
            got_m = conv.nn(ops.edge_pairs(conv.graph(tei, case["n"]), _dev(case["x"])))
            want = copy.deepcopy(case["cpu"]).double().messages(torch.from_numpy(case["x"]).double(),
                                                                torch.from_numpy(case["ei"]))
        assert torch.equal(got_m.cpu().double(), want), f"{tag}: the messages are not exact"
    got = _host(_device_run(conv, case["x"], case["ei"], case["gup"]))
    assert got[0].shape == (case["n"], fo)
    check_against_references(tag, got, case, "e_h")
    if aggr == "max" and case["ei"].shape[1]:
        assert np.array_equal(got[0], case["y_max"]), f"{tag}: the maximum of exact messages is one of them"
    return case, got


@gpu
@pytest.mark.parametrize("kind", MAIN_GRAPHS)
@pytest.mark.parametrize("seq", [False, True], ids=["linear", "mlp"])
@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("fi,fo", SHAPES)
def test_layer_parity(fi, fo, aggr, seq, kind):
    """forward and the gradients of x and of every parameter of nn against RefEdgeConv at 1e-5: every shape x aggr x
    nn x graph"""
    _check_layer(fi, fo, aggr, seq, kind)


@gpu
@pytest.mark.parametrize("seq", [False, True], ids=["linear", "mlp"])
@pytest.mark.parametrize("aggr", AGGRS)
def test_layer_parity_with_plain_torch_modules(aggr, seq):
    """``nn`` built from ``torch.nn.Linear`` as it is, on the graph without a hub: the same bar"""
    _check_layer(21, 64, aggr, seq, "multigraph", plain=True)


@gpu
@pytest.mark.parametrize("kind", EDGE_GRAPHS)
@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("fi,fo", [(3, 64), (16, 1)])
def test_layer_on_edge_graphs(fi, fo, aggr, kind):
    """one node, no edge, no node: the output has nn's width and is 0; the backward runs and every gradient is 0"""
    for seq in (False, True):
        case, (out, grads) = _check_layer(fi, fo, aggr, seq, kind)
        assert out.shape == (case["n"], fo) and (out == 0).all()
        assert grads["x"].shape == (case["n"], fi) and all((v == 0).all() for v in grads.values())
    torch.cuda.synchronize()


class Mix(nn.Module):
    """an ``nn`` without a matrix product: bits are compared, which a BLAS behind ``torch.nn.Linear`` does not promise"""

    def __init__(self, width, out):
        super().__init__()
        self.scale = nn.Parameter(torch.linspace(0.5, 1.5, width))
        self.out = out

    def forward(self, z):
        return torch.tanh(z * self.scale)[:, :self.out]


@gpu
@pytest.mark.parametrize("aggr", AGGRS)
def test_gradient_layouts_and_a_repeat_give_the_same_bits(aggr):
    """``out.sum().backward()`` sends an expanded gradient, a weighted loss through a column slice a strided one: the
    bits of ``x.grad`` (and of nn's gradient) are those of a contiguous gradient of the same values; x as a column
    slice: the same bits; forward + backward twice on the multigraph: identical bits"""
    n, ei = _graph("multigraph", 3)
    fi, fo = 20, 24
    rng = np.random.default_rng(11)
    x = _dev(coarse_grid(rng, (n, fi)) if aggr == "max" else rng.standard_normal((n, fi)).astype(np.float32))
    w = _dev(rng.uniform(0.5, 1.5, (n, fo)).astype(np.float32))
    tei = torch.from_numpy(ei).to(DEV)
    clear_cache()
    conv = dc.nn.EdgeConv(Mix(2 * fi, fo), aggr=aggr).to(DEV)

    def run(loss, xin=x):
        conv.nn.scale.grad = None
        xg = xin.detach().requires_grad_(True)
        out = conv(xg, tei)
        loss(out)
        torch.cuda.synchronize()
        return out.detach().clone(), xg.grad.clone(), conv.nn.scale.grad.clone()

    def same(a, b):
        assert all(torch.equal(s, t) for s, t in zip(a, b))

    ones = run(lambda out: torch.autograd.backward([out], [torch.ones_like(out)]))
    same(run(lambda out: out.sum().backward()), ones)            # expanded (stride 0)
    assert ones[1].abs().max() > 0
    dense = run(lambda out: torch.autograd.backward([out], [w]))
    same(run(lambda out: torch.autograd.backward([out], [w])), dense)          # a repeat: identical bits
    padded = torch.zeros((n, fo + 8), device=DEV)
    padded[:, 4:4 + fo] = w
    wide_w = torch.full((n, 2 * fo), 1e30, device=DEV)
    wide_w[:, ::2] = w
    same(run(lambda out: torch.autograd.backward([out], [padded[:, 4:4 + fo]])), dense)     # a column slice
    same(run(lambda out: torch.autograd.backward([out], [wide_w[:, ::2]])), dense)          # inner stride 2
    # a weighted loss through a column slice of the output against the same weights, zero elsewhere, sent contiguous
    part = torch.zeros((n, fo), device=DEV)
    part[:, 3:11] = w[:, 3:11]
    same(run(lambda out: (out[:, 3:11] * w[:, 3:11]).sum().backward())[1:],
         run(lambda out: torch.autograd.backward([out], [part]))[1:])
    same(run(lambda out: torch.autograd.backward([out], [w]), _wide(x)), dense)
    same(run(lambda out: torch.autograd.backward([out], [w]), _odd(x)), dense)


@gpu
def test_launches_of_one_layer_step():
    """forward + backward of EdgeConv: one kernel of dc_edge.hip per entry and no hop, no SAGE or GINE kernel"""
    case = layer_case(21, 64, "max", False, "multigraph")
    clear_cache()
    conv = _device_conv(case)
    x, gup, tei = _dev(case["x"]).requires_grad_(True), _dev(case["gup"]), torch.from_numpy(case["ei"]).to(DEV)
    _lib.kernel_trace(True)
    torch.autograd.backward([conv(x, tei)], [gup])
    counts = _lib.kernel_trace_counts()
    _lib.kernel_trace(False)
    edge = {name: v for name, v in counts.items() if "k_edge" in name}
    want = ("k_edge_pair_fwd", "k_edge_max_fwd", "k_edge_reduce_bwd", "k_edge_pair_bwd")
    assert sum(edge.values()) == 4 and all(any(k + "<" in name for name in edge) for k in want), counts
    assert not any("k_spmm" in name or "k_sage" in name or "k_gine" in name for name in counts), counts


@gpu
def test_a_deferred_x_is_resolved_and_nn_sees_the_edges_in_input_order():
    n, ei = _graph("multigraph", 3)
    tei = torch.from_numpy(ei).to(DEV)
    torch.manual_seed(7)
    pre = dc.nn.GCNConv(8, 16).to(DEV)
    seen = []

    class Spy(nn.Module):
        def forward(self, z):
            seen.append(z)
            return z[:, :5] + z[:, 16:21]

    conv = dc.nn.EdgeConv(Spy(), aggr="sum").to(DEV)
    x = torch.randn(n, 8, device=DEV)
    with torch.no_grad():
        h = pre(x, tei)
        assert type(h).__name__ == "DeferredActivation"
        value = ops.resolve(h)
        a, b = conv(h, tei), conv(value, tei)
    assert type(a) is torch.Tensor and torch.equal(a, b) and len(seen) == 2
    want = torch.cat([value[tei[1]], value[tei[0]] - value[tei[1]]], dim=1)
    assert seen[0].shape == (ei.shape[1], 32) and torch.equal(seen[0], want)
    for bad in (lambda z: z.double(), lambda z: z[:-1], lambda z: z[:, :0], lambda z: z.sum(1)):
        with pytest.raises(ValueError, match="nn must return"):
            dc.nn.EdgeConv(_Fn(bad), aggr="sum")(value, tei)     # nn's result must be float32 [E, C >= 1]


class _Fn(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, z):
        return self.fn(z)
