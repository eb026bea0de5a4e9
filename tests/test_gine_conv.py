"""``GINConv`` / ``GINEConv``: the layers, ``ops.gine_aggregate`` and the C entries of dc_gine.hip.

The reference is this file's own restatement of the contract in INTEGRATION.md 1.6 (PyG 2.5.2 gin_conv.py):
``RefGin`` / ``RefGine``, torch CPU modules evaluated in float32 (``ref32``) and float64 (``truth64``) with gradients
from torch autograd, and numpy formulas for the entries called directly.  ``oracle/pyg_ref`` has no GIN.

Mask stability.  A ReLU mask that differs between two evaluations changes a gradient by a whole term, so the mask has
to be the same in float32, in float64 and on the device.  With ``e = edge_attr`` (no ``edge_dim``) the mask is the sign
of ONE fp32 add of two float32 numbers; the sign of a correctly rounded sum is the sign of the exact sum, so the three
agree for any inputs (e ~ N(0, 1), x ~ N(+-0.5, 1): ``node_features``).  With ``edge_dim`` ``e`` comes out of the dense block's split products, so
``edge_attr`` is taken from multiples of 1/4 in [-2, 2] and ``lin.weight`` / ``lin.bias`` from multiples of 1/8 in
[-1, 1] with D <= 16: ``e`` is a sum of at most 17 multiples of 1/32 below 2^6, an exact float32 in any order - asserted
on the device against the exact float64 value before a layer is compared (``test_lin_edge_features_are_exact`` and
``_check_gine``).  For gradient parity ``nn = torch.nn.Linear(in, out)``: an inner ReLU in ``nn`` would bring the same
hazard back through the rounding of the library that runs ``nn``; one forward-only case runs ``Sequential(Linear, ReLU,
Linear)`` to show that an arbitrary module is called.  ``relu'(0) = 0``: the direct cases set a tenth of the entries
of ``e`` to ``-x[src]``, so ``x + e`` is exactly 0 there.

Metrics.  The layers through ``helpers.assert_parity`` at 1e-5 (nothing registered ``special``).  The entries:
``dc_gine_fwd`` bit-identical to a numpy float32 loop that walks the device's own ``ptr`` / ``other`` / ``perm`` in p
order (``s = 0; s += max(x + e, 0); y = (1 + eps) * x + s``, 1 + eps formed first) and within 1e-5 per row of float64;
``dc_gine_bwd_e`` bit-identical to ``mask * gy[dst]``; ``dc_gine_bwd_x`` within 1e-5 per row of float64
(``row_rel_err``); two calls of each: equal bits.

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
from deformcontact_amd.data import Batch, Data
from deformcontact_amd.graph import GraphIndex, clear_cache
from deformcontact_amd.nn import GINConv, GINEConv  # noqa: F401  (the module needs the layers: no test runs without them)
from tests.helpers import assert_parity, load_golden, random_multigraph, record_parity, rel_err, row_rel_err
from tests.test_gat_edge_kernels import HUB, _dev, _np, seg_graph, seg_lens

gpu = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5

#: (in, out) of the layer tests
SHAPES = [(21, 64), (64, 20), (25, 256), (16, 1)]
#: None: e = edge_attr of width in; 1: with [E] input
EDGE_DIMS = [None, 1, 3, 16]
#: (eps, train_eps)
EPS_MODES = {"eps0": (0.0, False), "eps03": (0.3, False), "train": (0.3, True)}
MAIN_GRAPHS = ["seg", "multigraph", "golden_rest"]
EDGE_GRAPHS = ["n1", "e0", "n0"]
#: widths of the direct tests: the general form (1, 3, 70: lane groups of 4, 4, 64) and the 16-byte form (20, 64, 256,
#: 1100: groups of 8, 16, 64, and 64 lanes over five column chunks)
WIDTHS = [1, 3, 20, 64, 70, 256, 1100]
DIRECT_GRAPHS = ["seg", "multigraph"]
DIRECT_EPS = [None, 0.0, 0.3]


# --------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------- #
def grid_values(rng, shape):
    """multiples of 1/4 in [-2, 2]"""
    return (rng.integers(-8, 9, shape) / 4.0).astype(np.float32)


def grid_weights(rng, shape):
    """multiples of 1/8 in [-1, 1]"""
    return (rng.integers(-8, 9, shape) / 8.0).astype(np.float32)


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
    if kind == "n0":
        return 0, np.zeros((2, 0), np.int64)
    z = load_golden("graphnet_gat_h32.npz")
    return z["rest_x"].shape[0], z["rest_edge_index"].astype(np.int64)


def _index_add(n, idx, terms):
    return torch.zeros((n, terms.shape[1]), dtype=torch.float64).index_add_(
        0, torch.from_numpy(idx), torch.from_numpy(np.ascontiguousarray(terms, np.float64))).numpy()


@functools.lru_cache(maxsize=None)
def direct_case(kind, f):
    """graph, inputs and the order-independent references of one direct case (computed once, never modified)"""
    n, ei = _graph(kind, 9)
    ne = ei.shape[1]
    rng = np.random.default_rng(2000 + f + len(kind))
    x = rng.standard_normal((n, f)).astype(np.float32)
    e = rng.standard_normal((ne, f)).astype(np.float32)
    zero = rng.random((ne, f)) < 0.1
    e[zero] = -x[ei[0]][zero]                                    # x + e exactly 0: relu'(0) = 0
    gy = (rng.uniform(0.5, 1.5, (n, f)) * np.where(rng.random((n, f)) < 0.5, -1.0, 1.0)).astype(np.float32)
    pre = x[ei[0]] + e                                           # the ONE fp32 add the mask is the sign of
    assert (pre == 0).mean() > 0.05 and np.array_equal(pre > 0, x[ei[0]].astype(np.float64) + e > 0)
    mask = pre > 0
    ge = np.where(mask, gy[ei[1]], np.float32(0))                # exact: a copy or a zero
    s64 = _index_add(n, ei[1], np.maximum(x[ei[0]].astype(np.float64) + e, 0.0))
    gxs64 = _index_add(n, ei[0], np.where(mask, gy[ei[1]].astype(np.float64), 0.0))
    return dict(n=n, ei=ei, x=x, e=e, gy=gy, mask=mask, ge=ge, s64=s64, gxs64=gxs64)


def one_plus(eps):
    """1 + eps as the kernel forms it: one fp32 add"""
    return np.float32(1) + np.float32(eps)


def fwd_loop_f32(ptr, other, perm, x, e):
    """s [N, F] float32: per row, in p order, ``s += max(x[other[p]] + e[perm[p]], 0)`` - the kernel's adds, one by one"""
    s = np.zeros((len(ptr) - 1, x.shape[1]), np.float32)
    zero = np.float32(0)
    for i in range(len(ptr) - 1):
        acc = s[i]
        for p in range(ptr[i], ptr[i + 1]):
            acc += np.maximum(x[other[p]] + e[perm[p]], zero)
    return s


# --------------------------------------------------------------------------- #
# the restatement as torch modules (float32: ref32, .double(): truth64)
# --------------------------------------------------------------------------- #
class _RefEps(nn.Module):
    def __init__(self, inner, eps, train_eps):
        super().__init__()
        self.nn = inner
        if train_eps:
            self.eps = nn.Parameter(torch.full((1,), float(eps)))
        else:
            self.register_buffer("eps", torch.full((1,), float(eps)))


class RefGin(_RefEps):
    def forward(self, x, edge_index):
        j, i = edge_index
        agg = torch.zeros_like(x).index_add_(0, i, x[j])
        return self.nn((1 + self.eps) * x + agg)


class RefGine(_RefEps):
    def __init__(self, inner, eps=0.0, train_eps=False, edge_dim=None, in_channels=None):
        super().__init__(inner, eps, train_eps)
        if edge_dim is not None:
            self.lin = nn.Linear(edge_dim, in_channels)

    def edge_features(self, edge_attr):
        if edge_attr.dim() == 1:
            edge_attr = edge_attr.unsqueeze(-1)
        return self.lin(edge_attr) if hasattr(self, "lin") else edge_attr

    def forward(self, x, edge_index, edge_attr):
        j, i = edge_index
        agg = torch.zeros_like(x).index_add_(0, i, torch.relu(x[j] + self.edge_features(edge_attr)))
        return self.nn((1 + self.eps) * x + agg)


def _ref_run(mod, x, ei, ea, gup, dtype):
    for p in mod.parameters():
        p.grad = None
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    args = [xt, torch.from_numpy(ei)]
    if ea is not None:
        args.append(torch.from_numpy(ea).to(dtype).requires_grad_(True))
    out = mod(*args)
    (out * torch.from_numpy(gup).to(dtype)).sum().backward()
    grads = {"x": xt.grad.numpy()}
    if ea is not None:
        grads["edge_attr"] = (args[2].grad if args[2].grad is not None else torch.zeros_like(args[2])).numpy()
    grads.update({name: p.grad.detach().numpy().copy() for name, p in mod.named_parameters()})
    return out.detach().numpy(), grads


def node_features(rng, n, inner):
    """x ~ N(0, 1) + 0.5 sign(column sum of ``nn``'s weight).  The gradient of eps is ONE number, ``sum(g x)`` with
    ``g = gup @ W`` the gradient behind ``nn``: with a positive ``gup`` the sign of ``g[:, c]`` is that of W's column
    sum, and with a centred x the terms would cancel to whatever the draw leaves - a figure on which no relative bar
    means anything.  The shift makes it, by construction, a sum of terms most of which share their sign."""
    if inner.out_features == 1:
        # a single output channel is ONE dot product per row, and the hub's terms are sums over 5,000 edges: with
        # positive weights (and the aggregated columns positive by the shift below) it is, by construction, a sum of
        # positive terms and the comparison measures the layer, not a cancellation
        with torch.no_grad():
            inner.weight.abs_()
    x = rng.standard_normal((n, inner.in_features))
    return (x + 0.5 * np.sign(inner.weight.detach().sum(0).numpy())).astype(np.float32)


@functools.lru_cache(maxsize=None)
def gine_case(fi, fo, edge_dim, mode, kind):
    """inputs, the reference module and its float32 / float64 results of one GINEConv case"""
    torch.set_num_threads(1)
    eps, train = EPS_MODES[mode]
    n, ei = _graph(kind, 3)
    ne = ei.shape[1]
    rng = np.random.default_rng(fi + fo + (edge_dim or 0))
    gup = rng.uniform(0.5, 1.5, (n, fo)).astype(np.float32)
    torch.manual_seed(12)
    cpu = RefGine(nn.Linear(fi, fo), eps, train, edge_dim, fi)   # nn: default initialisation
    x = node_features(rng, n, cpu.nn)
    if edge_dim is None:
        ea = rng.standard_normal((ne, fi)).astype(np.float32)
    else:
        ea = grid_values(rng, (ne,) if edge_dim == 1 else (ne, edge_dim))
        with torch.no_grad():
            cpu.lin.weight.copy_(torch.from_numpy(grid_weights(rng, (fi, edge_dim))))
            cpu.lin.bias.copy_(torch.from_numpy(grid_weights(rng, (fi,))))
    r32 = _ref_run(cpu, x, ei, ea, gup, torch.float32)
    r64 = _ref_run(copy.deepcopy(cpu).double(), x, ei, ea, gup, torch.float64)
    return dict(n=n, ei=ei, x=x, ea=ea, gup=gup, cpu=cpu, eps=eps, train=train, edge_dim=edge_dim, r32=r32, r64=r64)


@functools.lru_cache(maxsize=None)
def gin_case(fi, fo, mode, kind):
    torch.set_num_threads(1)
    eps, train = EPS_MODES[mode]
    n, ei = _graph(kind, 3)
    rng = np.random.default_rng(fi + fo)
    gup = rng.uniform(0.5, 1.5, (n, fo)).astype(np.float32)
    torch.manual_seed(12)
    cpu = RefGin(nn.Linear(fi, fo), eps, train)
    x = node_features(rng, n, cpu.nn)
    r32 = _ref_run(cpu, x, ei, None, gup, torch.float32)
    r64 = _ref_run(copy.deepcopy(cpu).double(), x, ei, None, gup, torch.float64)
    return dict(n=n, ei=ei, x=x, ea=None, gup=gup, cpu=cpu, eps=eps, train=train, r32=r32, r64=r64)


def _gine_cases():
    cases = [(s, d, m, kind) for s in SHAPES for d in EDGE_DIMS for m in EPS_MODES for kind in MAIN_GRAPHS]
    return cases + [(s, d, "train", kind) for s in SHAPES for d in (None, 3) for kind in EDGE_GRAPHS]


def _gin_cases():
    return [(s, m, kind) for s in SHAPES for m in EPS_MODES for kind in MAIN_GRAPHS + EDGE_GRAPHS]


def check_against_references(tag, got, case, side):
    """output and gradients of one evaluation (``side``: "e_o" the float32 restatement against float64, "e_h" the
    device) against the references at 1e-5"""
    (o, g), (o32, g32), (o64, g64) = got, case["r32"], case["r64"]
    assert set(g) == set(g32), (tag, sorted(g), sorted(g32))
    for name, a, a32, a64 in [("forward", o, o32, o64)] + [(k + ".grad", g[k], g32[k], g64[k]) for k in g32]:
        assert a is not None, (tag, name)
        assert a.shape == a32.shape, (tag, name, a.shape, a32.shape)
        if side == "e_o":
            d = rel_err(a32, a64)
            record_parity(f"{tag} {name}", None, e_o=d)
            assert d < TOL, (tag, name, d)
        else:
            assert_parity(a, a32, a64, TOL, f"{tag} {name}")


# --------------------------------------------------------------------------- #
# CPU
# --------------------------------------------------------------------------- #
def _shapes(mod):
    return {k: tuple(v.shape) for k, v in mod.state_dict().items()}


def test_constructor_parameters_and_state_dict():
    for train in (False, True):
        conv = dc.nn.GINConv(nn.Linear(21, 64), eps=0.3, train_eps=train)
        assert _shapes(conv) == {"eps": (1,), "nn.weight": (64, 21), "nn.bias": (64,)}
        assert isinstance(conv.eps, nn.Parameter) == train and conv.eps.requires_grad == train
        assert ("eps" in dict(conv.named_parameters())) == train and ("eps" in dict(conv.named_buffers())) == (not train)
        assert conv.eps.dtype == torch.float32 and float(conv.eps.detach()) == float(np.float32(0.3))
        assert conv.graph_flags() == dict(self_loops=False, normalize=False)
        assert not hasattr(conv, "supports_fused_relu") and not hasattr(conv, "lin")
        assert repr(conv).startswith("GINConv(nn=Linear(")
        ref = RefGin(nn.Linear(21, 64), 0.7, train)
        assert set(ref.state_dict()) == set(conv.state_dict())
        conv.load_state_dict(ref.state_dict(), strict=True)
        assert torch.equal(conv.nn.weight, ref.nn.weight) and float(conv.eps.detach()) == float(np.float32(0.7))
        for edge_dim in (None, 1, 3):
            seq = nn.Sequential(nn.Linear(21, 32), nn.ReLU(), nn.Linear(32, 64))
            conv = dc.nn.GINEConv(seq, eps=0.3, train_eps=train, edge_dim=edge_dim)
            want = {"eps": (1,), "nn.0.weight": (32, 21), "nn.0.bias": (32,), "nn.2.weight": (64, 32), "nn.2.bias": (64,)}
            if edge_dim is not None:
                want.update({"lin.weight": (21, edge_dim), "lin.bias": (21,)})
            assert _shapes(conv) == want
            assert (conv.lin is None) == (edge_dim is None) and isinstance(conv.eps, nn.Parameter) == train
            assert not hasattr(conv, "supports_fused_relu") and conv.graph_flags() == dict(self_loops=False, normalize=False)
            assert repr(conv).startswith("GINEConv(nn=Sequential(")
            ref = RefGine(copy.deepcopy(seq), 0.9, train, edge_dim, 21)
            assert set(ref.state_dict()) == set(conv.state_dict())
            conv.load_state_dict(ref.state_dict(), strict=True)
            back = dc.nn.GINEConv(copy.deepcopy(seq), train_eps=train, edge_dim=edge_dim)
            back.load_state_dict(conv.state_dict(), strict=True)                 # round trip
            for k, v in conv.state_dict().items():
                assert torch.equal(back.state_dict()[k], v), k
            assert float(back.eps.detach()) == float(np.float32(0.9))
    one = dc.nn.GINEConv(nn.Linear(5, 7))
    assert float(one.eps.detach()) == 0.0 and not isinstance(one.eps, nn.Parameter) and one.edge_dim is None
    # the second and third positional arguments are eps and train_eps, as in PyG
    assert isinstance(dc.nn.GINConv(nn.Linear(5, 7), 0.5, True).eps, nn.Parameter)
    assert "GINConv" in dc.nn.__all__ and "GINEConv" in dc.nn.__all__


def test_reset_parameters_restores_eps_and_resets_nn_and_lin():
    for cls, kw in ((dc.nn.GINConv, {}), (dc.nn.GINEConv, dict(edge_dim=3))):
        for train in (False, True):
            conv = cls(nn.Sequential(nn.Linear(8, 8), nn.ReLU(), nn.Linear(8, 4)), eps=0.25, train_eps=train, **kw)
            with torch.no_grad():
                conv.eps.fill_(5.0)
                before = [p.detach().clone() for n_, p in conv.named_parameters() if n_ != "eps"]
            conv.reset_parameters()
            assert float(conv.eps.detach()) == 0.25 and conv.eps.shape == (1,)
            after = [p.detach() for n_, p in conv.named_parameters() if n_ != "eps"]
            assert len(after) == (6 if kw else 4) and all(not torch.equal(a, b) for a, b in zip(after, before))
    bound = 1 / np.sqrt(3.0)
    conv = dc.nn.GINEConv(nn.Linear(8, 4), edge_dim=3)
    assert conv.lin.weight.shape == (8, 3) and conv.lin.bias.shape == (8,)
    assert float(conv.lin.weight.detach().abs().max()) <= bound and float(conv.lin.bias.detach().abs().max()) <= bound


def test_in_channels_are_inferred_as_pyg_does():
    class Chan(nn.Module):
        in_channels = 9

    class Feat(nn.Module):
        in_features, in_channels = 11, 9

    assert dc.nn.GINEConv(nn.Sequential(nn.Linear(7, 3), nn.ReLU()), edge_dim=2).lin.weight.shape == (7, 2)
    assert dc.nn.GINEConv(nn.Linear(6, 3), edge_dim=2).lin.weight.shape == (6, 2)
    assert dc.nn.GINEConv(Chan(), edge_dim=2).lin.weight.shape == (9, 2)
    assert dc.nn.GINEConv(Feat(), edge_dim=2).lin.weight.shape == (11, 2)          # in_features first
    assert dc.nn.GINEConv(nn.Sequential(Chan(), nn.ReLU()), edge_dim=2).lin.weight.shape == (9, 2)
    with pytest.raises(ValueError, match="Could not infer input channels from `nn`."):
        dc.nn.GINEConv(nn.ReLU(), edge_dim=2)
    with pytest.raises(ValueError, match="Could not infer input channels"):
        dc.nn.GINEConv(nn.Sequential(nn.ReLU(), nn.Linear(4, 4)), edge_dim=2)
    dc.nn.GINEConv(nn.ReLU())                                    # without edge_dim nothing has to be inferred


def test_errors_raised_on_the_host():
    x, ei = torch.zeros(5, 4), torch.zeros(2, 3, dtype=torch.long)
    plain, proj, one = dc.nn.GINEConv(nn.Linear(4, 2)), dc.nn.GINEConv(nn.Linear(4, 2), edge_dim=3), \
        dc.nn.GINEConv(nn.Linear(4, 2), edge_dim=1)
    with pytest.raises(ValueError, match="edge_attr"):
        plain(x, ei)                                             # GINEConv without edge_attr
    with pytest.raises(ValueError, match="edge_attr"):
        proj(x, ei, None)
    for bad in (3, "mean", [1.0, 2.0], np.zeros((3, 4), np.float32), True):
        with pytest.raises(TypeError, match="edge_attr"):
            plain(x, ei, bad)                                    # a non-tensor third argument
    with pytest.raises(ValueError, match="rows"):
        plain(x, ei, torch.zeros(4, 4))                          # a wrong row count
    with pytest.raises(ValueError, match="rows"):
        proj(x, ei, torch.zeros(2, 3))
    with pytest.raises(ValueError, match="edge_dim"):
        plain(x, ei, torch.zeros(3, 3))                          # no edge_dim: the width must be x's
    with pytest.raises(ValueError, match="do not match"):
        plain(x, ei, torch.zeros(3, 1))
    with pytest.raises(ValueError):
        plain(x, ei, torch.zeros(3))                             # [E] only where the width is 1
    with pytest.raises(ValueError):
        proj(x, ei, torch.zeros(3, 4))                           # edge_dim = 3, width 4
    with pytest.raises(ValueError):
        proj(x, ei, torch.zeros(3))                              # [E] only where the width is 1
    with pytest.raises(ValueError, match="float32"):
        plain(x, ei, torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(ValueError):
        plain(x, ei, torch.zeros(3, 4, 1))
    with pytest.raises(ValueError, match="contiguous"):
        plain(x, ei, torch.zeros(3, 8)[:, ::2])                  # a column slice needs inner stride 1
    for conv, ea in ((plain, torch.zeros(3, 4)), (proj, torch.zeros(3, 3)), (one, torch.zeros(3))):
        with pytest.raises(RuntimeError, match="HIP device"):
            conv(x, ei, ea)                                      # every host check passed: no CPU path
    with pytest.raises(RuntimeError, match="HIP device"):
        dc.nn.GINConv(nn.Linear(4, 2))(x, ei)
    for conv, args in ((plain, (x, ei, torch.zeros(3, 4))), (dc.nn.GINConv(nn.Linear(4, 2)), (x, ei))):
        for unsupported in (dict(size=(5, 5)), dict(relu=True), dict(next_conv=None)):
            with pytest.raises(TypeError):
                conv(*args, **unsupported)                       # not supported: absent from the signature
    with pytest.raises(TypeError):
        dc.nn.GINConv(nn.Linear(4, 2), edge_dim=3)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.gine_aggregate(None, x, torch.zeros(3, 4))


def test_importable_through_the_torch_geometric_alias():
    import sys
    from deformcontact_amd.pyg_alias import install_as_torch_geometric
    names = ("torch_geometric", "torch_geometric.nn", "torch_geometric.data")
    saved = {k: sys.modules.get(k) for k in names}
    try:
        install_as_torch_geometric(force=True)
        from torch_geometric.nn import GINConv as a_gin, GINEConv as a_gine
        assert a_gin is dc.nn.GINConv and a_gine is dc.nn.GINEConv
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def _entry_calls():
    """name -> call(N, F, pointers given?, leading dimension) of every entry of dc_gine.hip, otherwise valid (E = 5)"""
    L = _lib.lib()
    p = lambda ok: 64 if ok else None                           # any non-null address: rejected calls never touch it
    out = lambda ok: 128 if ok else None
    return {
        "dc_gine_fwd": lambda n, f, ok, ld: L.dc_gine_fwd(p(ok), p(ok), p(ok), p(ok), ld, 192 if ok else None, ld, None,
                                                          out(ok), ld, n, f, None),
        "dc_gine_bwd_x": lambda n, f, ok, ld: L.dc_gine_bwd_x(p(ok), p(ok), p(ok), p(ok), ld, 192 if ok else None, ld,
                                                              None, 256 if ok else None, ld, out(ok), ld, n, f, None),
        "dc_gine_bwd_e": lambda n, f, ok, ld: L.dc_gine_bwd_e(p(ok), p(ok), p(ok), ld, 192 if ok else None, ld,
                                                              256 if ok else None, ld, out(ok), ld, n, 5 if n else 0, f,
                                                              None),
    }


def test_abi_argument_errors_of_the_gine_entries_without_gpu():
    """null pointers, negative N, F < 1, sizes out of range, short leading dimensions, aliased outputs: -1 and the
    entry's name, before any HIP call; N = 0 (and with it E = 0) returns 0 with no pointer at all; eps may be null."""
    L = _lib.lib()
    calls = _entry_calls()
    declared = [n for n in _lib.exported_names() if "gine" in n]
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
    assert L.dc_gine_fwd(64, 64, 64, 128, 16, 192, 16, None, 128, 16, 3, 16, None) == -1 and b"alias" in L.dc_last_error()
    assert L.dc_gine_fwd(64, 64, 64, 128, 16, 192, 16, None, 192, 16, 3, 16, None) == -1 and b"alias" in L.dc_last_error()
    assert L.dc_gine_bwd_x(64, 64, 64, 128, 16, 192, 16, None, 256, 16, 256, 16, 3, 16, None) == -1
    assert b"alias" in L.dc_last_error()
    assert L.dc_gine_bwd_e(64, 64, 128, 16, 192, 16, 256, 16, 192, 16, 3, 5, 16, None) == -1 and b"alias" in L.dc_last_error()
    # the edge count of dc_gine_bwd_e
    assert L.dc_gine_bwd_e(64, 64, 128, 16, 192, 16, 256, 16, 320, 16, 3, -1, 16, None) == -1 and b"range" in L.dc_last_error()
    assert L.dc_gine_bwd_e(64, 64, 128, 16, 192, 16, 256, 16, 320, 16, 3, 1 << 30, 16, None) == -1
    assert L.dc_gine_bwd_e(None, None, None, 16, None, 16, None, 16, None, 16, 3, 0, 16, None) == 0      # nodes without edges


def test_float32_restatement_within_the_bar_of_float64_on_the_layer_inputs():
    """Every layer case of the GPU tests: the float32 restatement within 1e-5 of float64, output and every gradient;
    without ``train_eps`` eps has no gradient."""
    for (fi, fo), d, mode, kind in _gine_cases():
        case = gine_case(fi, fo, d, mode, kind)
        check_against_references(f"RefGine fp32 vs fp64 {fi}->{fo} D={d} {mode} {kind}", case["r32"], case, "e_o")
        assert ("eps" in case["r32"][1]) == case["train"]
    for (fi, fo), mode, kind in _gin_cases():
        case = gin_case(fi, fo, mode, kind)
        check_against_references(f"RefGin fp32 vs fp64 {fi}->{fo} {mode} {kind}", case["r32"], case, "e_o")


def test_lin_edge_features_of_the_reference_are_exact():
    """grid ``edge_attr``, grid ``lin``: float32 and float64 give the same ``e``, so every evaluation has one mask"""
    for (fi, fo) in SHAPES:
        for d in (1, 3, 16):
            case = gine_case(fi, fo, d, "eps0", "multigraph")
            with torch.no_grad():
                e32 = case["cpu"].edge_features(torch.from_numpy(case["ea"]))
                e64 = copy.deepcopy(case["cpu"]).double().edge_features(torch.from_numpy(case["ea"]).double())
            assert torch.equal(e32.double(), e64) and float(e32.abs().max()) > 1


def test_direct_inputs_hold_exact_zeros_and_the_formulas_agree_with_autograd():
    """the direct cases: a tenth of ``x + e`` is exactly 0, and the hand-written backward formulas (float64, mask with
    relu'(0) = 0) equal torch autograd through ``relu`` in float64"""
    for kind in DIRECT_GRAPHS:
        case = direct_case(kind, 20)
        n, ei = case["n"], case["ei"]
        deg = np.bincount(ei[1], minlength=n)
        assert (deg == 0).any() and deg.max() >= (HUB - 1 if kind == "seg" else 8)
        xt = torch.from_numpy(case["x"]).double().requires_grad_(True)
        et = torch.from_numpy(case["e"]).double().requires_grad_(True)
        j, i = torch.from_numpy(ei)
        s = torch.zeros_like(xt).index_add_(0, i, torch.relu(xt[j] + et))
        assert rel_err(s.detach().numpy(), case["s64"]) < 1e-14
        (s * torch.from_numpy(case["gy"]).double()).sum().backward()
        assert rel_err(case["gxs64"], xt.grad.numpy()) < 1e-14
        assert np.array_equal(et.grad.numpy(), case["ge"].astype(np.float64))


# --------------------------------------------------------------------------- #
# GPU: the entries called directly
# --------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def _device_graph(kind):
    """the adjacency of the direct cases of ``kind`` and its forward side read back: (g, ptr, other, perm)"""
    n, ei = _graph(kind, 9)
    g = GraphIndex(torch.from_numpy(ei).to(DEV), n, self_loops=False, normalize=False, validate=True)
    ne = ei.shape[1]
    ptr, other, perm = (_np(t).astype(np.int64) for t in (g.fwd.ptr, g.fwd.other[:ne], g.fwd.perm[:ne]))
    # the device's own sorted set: perm is a bijection over the input edges and names each position's edge
    assert ptr[0] == 0 and ptr[-1] == ne and np.array_equal(np.sort(perm), np.arange(ne))
    assert np.array_equal(ei[0][perm], other) and np.array_equal(ei[1][perm], np.repeat(np.arange(n), np.diff(ptr)))
    tperm = _np(g.bwd.perm[:ne]).astype(np.int64)
    assert np.array_equal(np.sort(tperm), np.arange(ne)) and np.array_equal(ei[1][tperm], _np(g.bwd.other[:ne]))
    return g, ptr, other, perm


@functools.lru_cache(maxsize=None)
def _fwd_sum_f32(kind, f):
    _, ptr, other, perm = _device_graph(kind)
    case = direct_case(kind, f)
    return fwd_loop_f32(ptr, other, perm, case["x"], case["e"])


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


def _eps_dev(eps):
    return None if eps is None else torch.full((1,), eps, dtype=torch.float32, device=DEV)


def _within_bar_of_float64(got, want64, name):
    d = row_rel_err(got, want64)
    print(f"{name}: row_rel_err vs float64 = {d:.3e}")
    record_parity(name, None, e_h=d, metric="row_rel_err")
    assert d < TOL, (name, d)


@gpu
@pytest.mark.parametrize("kind", DIRECT_GRAPHS)
@pytest.mark.parametrize("f", WIDTHS)
def test_forward_entry(f, kind):
    """bit-identical to the float32 loop over the device's own sorted set, for eps = NULL, 0 and 0.3; within 1e-5 of
    float64 per row; x and e as column slices (aligned and not), a strided output: the same bits; twice: the same bits"""
    case = direct_case(kind, f)
    g, n = _device_graph(kind)[0], case["n"]
    s32 = _fwd_sum_f32(kind, f)
    x, e = _dev(case["x"]), _dev(case["e"])
    for eps in DIRECT_EPS:
        te = _eps_dev(eps)
        y = ops._gine_fwd(g, x, e, te)
        want = s32 if eps is None else one_plus(eps) * case["x"] + s32
        assert want.dtype == np.float32 and np.array_equal(_np(y), want), (f, kind, eps)
        want64 = case["s64"] + (0.0 if eps is None else float(one_plus(eps)) * case["x"].astype(np.float64))
        _within_bar_of_float64(_np(y), want64, f"gine fwd F={f} {kind} eps={eps}")
        assert torch.equal(y, ops._gine_fwd(g, x, e, te))
        assert torch.equal(y, ops._gine_fwd(g, _wide(x), e, te)) and torch.equal(y, ops._gine_fwd(g, x, _wide(e), te))
        assert torch.equal(y, ops._gine_fwd(g, _odd(x), _odd(e), te))
        assert torch.equal(y, ops.gine_aggregate(g, x, e, te))
    # a strided OUTPUT (row stride f + 8), eps = 0.3: the same values and nothing beside them
    te = _eps_dev(0.3)
    y = ops._gine_fwd(g, x, e, te)
    L, st, ld = _lib.lib(), torch.cuda.current_stream().cuda_stream, f + 8
    o_y = torch.full((n, ld), 7.0, device=DEV)
    _lib.check(L.dc_gine_fwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), g.fwd.perm.data_ptr(), x.data_ptr(), f,
                             e.data_ptr(), f, te.data_ptr(), o_y.data_ptr(), ld, n, f, st), "dc_gine_fwd")
    assert torch.equal(o_y[:, :f], y) and (o_y[:, f:] == 7.0).all()


@gpu
@pytest.mark.parametrize("kind", DIRECT_GRAPHS)
@pytest.mark.parametrize("f", WIDTHS)
def test_backward_entries(f, kind):
    """g_e bit-identical to ``mask * gy[dst]`` (zero where x + e is exactly 0); g_x within 1e-5 of float64 per row for
    eps = NULL, 0 and 0.3; x, e and gy as column slices, strided outputs: the same bits; twice: the same bits; through
    autograd with a non-contiguous and an expanded gradient: the same bits"""
    case = direct_case(kind, f)
    g, n, ne = _device_graph(kind)[0], case["n"], case["ei"].shape[1]
    x, e, gy = _dev(case["x"]), _dev(case["e"]), _dev(case["gy"])
    ge = ops._gine_bwd_e(g, x, e, gy)
    assert np.array_equal(_np(ge), case["ge"]) and (ge[_dev(~case["mask"])] == 0).all()
    assert torch.equal(ge, ops._gine_bwd_e(g, x, e, gy))
    assert torch.equal(ge, ops._gine_bwd_e(g, _wide(x), e, gy)) and torch.equal(ge, ops._gine_bwd_e(g, x, _wide(e), gy))
    assert torch.equal(ge, ops._gine_bwd_e(g, x, e, _wide(gy))) and torch.equal(ge, ops._gine_bwd_e(g, _odd(x), _odd(e),
                                                                                                      _odd(gy)))
    for eps in DIRECT_EPS:
        te = _eps_dev(eps)
        gx = ops._gine_bwd_x(g, x, e, te, gy)
        want64 = case["gxs64"] + (0.0 if eps is None else float(one_plus(eps)) * case["gy"].astype(np.float64))
        _within_bar_of_float64(_np(gx), want64, f"gine g_x F={f} {kind} eps={eps}")
        assert torch.equal(gx, ops._gine_bwd_x(g, x, e, te, gy))
        assert torch.equal(gx, ops._gine_bwd_x(g, _wide(x), e, te, gy))
        assert torch.equal(gx, ops._gine_bwd_x(g, x, _wide(e), te, gy))
        assert torch.equal(gx, ops._gine_bwd_x(g, x, e, te, _wide(gy)))
        assert torch.equal(gx, ops._gine_bwd_x(g, _odd(x), _odd(e), te, _odd(gy)))
    # strided OUTPUTS (eps = 0.3): the entries called with row strides f + 8 write the same values and nothing beside them
    te = _eps_dev(0.3)
    gx = ops._gine_bwd_x(g, x, e, te, gy)
    L, st, ld = _lib.lib(), torch.cuda.current_stream().cuda_stream, f + 8
    o_x, o_e = torch.full((n, ld), 7.0, device=DEV), torch.full((ne, ld), 7.0, device=DEV)
    _lib.check(L.dc_gine_bwd_x(g.bwd.ptr.data_ptr(), g.bwd.other.data_ptr(), g.bwd.perm.data_ptr(), x.data_ptr(), f,
                               e.data_ptr(), f, te.data_ptr(), gy.data_ptr(), f, o_x.data_ptr(), ld, n, f, st),
               "dc_gine_bwd_x")
    _lib.check(L.dc_gine_bwd_e(g.edge_index[0].data_ptr(), g.edge_index[1].data_ptr(), x.data_ptr(), f, e.data_ptr(), f,
                               gy.data_ptr(), f, o_e.data_ptr(), ld, n, ne, f, st), "dc_gine_bwd_e")
    for wide_out, dense in ((o_x, gx), (o_e, ge)):
        assert torch.equal(wide_out[:, :f], dense) and (wide_out[:, f:] == 7.0).all()
    # through autograd (eps = 0.3 a trained parameter), the gradient arriving non-contiguous, then expanded
    tp = te.clone().requires_grad_(True)
    xs, es = _wide(x).detach().requires_grad_(True), _wide(e).detach().requires_grad_(True)
    wide_g = torch.full((n, 2 * f), 1e30, device=DEV)
    wide_g[:, ::2] = gy
    torch.autograd.backward([ops.gine_aggregate(g, xs, es, tp)], [wide_g[:, ::2]])
    assert torch.equal(xs.grad, gx) and torch.equal(es.grad, ge)
    want_eps = float((case["gy"].astype(np.float64) * case["x"]).sum())
    scale = float(np.abs(case["gy"].astype(np.float64) * case["x"]).sum())
    assert tp.grad.shape == (1,) and abs(float(tp.grad) - want_eps) < TOL * scale
    xs.grad = es.grad = None
    ops.gine_aggregate(g, xs, es, te).sum().backward()           # an expanded gradient of ones; eps needs no gradient
    assert torch.equal(xs.grad, ops._gine_bwd_x(g, x, e, te, torch.ones_like(gy)))
    assert torch.equal(es.grad, ops._gine_bwd_e(g, x, e, torch.ones_like(gy)))


@gpu
def test_entries_with_no_rows_and_with_no_edges():
    """N = 0: every entry returns 0 without a launch, ``gine_aggregate`` an empty tensor that carries a gradient;
    N > 0 without any edge: y = (1 + eps) x, g_x = (1 + eps) g_y, g_e empty; the checks of ``gine_aggregate``."""
    L = _lib.lib()
    zi = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert L.dc_gine_fwd(zi.data_ptr(), zi.data_ptr(), zi.data_ptr(), None, 15, None, 15, None, None, 15, 0, 15, None) == 0
    assert L.dc_gine_bwd_x(zi.data_ptr(), zi.data_ptr(), zi.data_ptr(), None, 15, None, 15, None, None, 15, None, 15, 0,
                           15, None) == 0
    assert L.dc_gine_bwd_e(None, None, None, 15, None, 15, None, 15, None, 15, 0, 0, 15, None) == 0
    x0 = torch.zeros((0, 15), device=DEV, requires_grad=True)
    e0 = torch.zeros((0, 15), device=DEV, requires_grad=True)
    p0 = torch.full((1,), 0.3, device=DEV, requires_grad=True)
    y0 = ops.gine_aggregate(None, x0, e0, p0)
    assert y0.shape == (0, 15) and y0.requires_grad
    y0.sum().backward()
    assert x0.grad.shape == (0, 15) and e0.grad.shape == (0, 15) and float(p0.grad) == 0.0
    n, f = 37, 15
    g = GraphIndex(torch.zeros((2, 0), dtype=torch.int64, device=DEV), n, self_loops=False, normalize=False)
    x = torch.randn(n, f, device=DEV, requires_grad=True)
    e = torch.zeros((0, f), device=DEV, requires_grad=True)
    te = _eps_dev(0.3)
    y = ops.gine_aggregate(g, x, e, te)
    assert torch.equal(y, (1 + te) * x) and (ops.gine_aggregate(g, x, e) == 0).all()
    gy = torch.randn(n, f, device=DEV)
    torch.autograd.backward([y], [gy])
    assert torch.equal(x.grad, (1 + te) * gy) and e.grad.shape == (0, f)
    xd = x.detach()
    with pytest.raises(ValueError, match="rows"):
        ops.gine_aggregate(g, xd, torch.zeros((3, f), device=DEV))
    with pytest.raises(ValueError):
        ops.gine_aggregate(g, xd, torch.zeros((0, f + 1), device=DEV))
    with pytest.raises(ValueError):
        ops.gine_aggregate(g, xd.double(), e.detach())
    with pytest.raises(ValueError, match="None"):
        ops.gine_aggregate(None, xd, e.detach())
    with pytest.raises(ValueError):
        ops.gine_aggregate(g, xd[:5], e.detach())
    with pytest.raises(ValueError, match="eps"):
        ops.gine_aggregate(g, xd, e.detach(), 0.3)
    with pytest.raises(RuntimeError):
        ops.gine_aggregate(g, xd, e.detach(), torch.zeros(1))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.gine_aggregate(g, xd.cpu(), e.detach())
    with pytest.raises(ValueError):
        ops.gine_aggregate(GraphIndex(torch.zeros((2, 0), dtype=torch.int64, device=DEV), n, self_loops=True,
                                      normalize=False), xd, e.detach())
    # a merged adjacency and a row window of one: their perm names merged edge ids, the kernels take no row offset
    ei2 = torch.tensor([[0, 1, 2], [1, 2, 0]], device=DEV)
    merged = GraphIndex.from_parts([(ei2, 3), (ei2, 3)], self_loops=False, normalize=False)
    for bad, rows in ((merged, merged.num_nodes), (merged.window(1), 3)):
        with pytest.raises(ValueError, match="merged"):
            ops.gine_aggregate(bad, torch.zeros((rows, f), device=DEV), torch.zeros((bad.num_input_edges, f), device=DEV))


# --------------------------------------------------------------------------- #
# GPU: the layers
# --------------------------------------------------------------------------- #
def _device_gine(case, dense_block=False):
    """the layer with the reference's parameters; ``dense_block``: ``nn`` on the package's own dense block (same keys) -
    for the tests that compare BITS between runs and operand layouts, which a BLAS behind ``torch.nn.Linear`` does not
    promise"""
    fi, fo = case["cpu"].nn.in_features, case["cpu"].nn.out_features
    inner = dc.nn.conv._Lin(fi, fo, bias=True) if dense_block else nn.Linear(fi, fo)
    conv = dc.nn.GINEConv(inner, eps=case["eps"], train_eps=case["train"], edge_dim=case["edge_dim"])
    conv.load_state_dict({k: v.clone() for k, v in case["cpu"].state_dict().items()}, strict=True)
    return conv.to(DEV)


def _device_run(conv, x, ei, ea, gup):
    for p in conv.parameters():
        p.grad = None
    xg = (x if isinstance(x, torch.Tensor) else _dev(x)).detach().requires_grad_(True)
    args = [xg, ei if isinstance(ei, torch.Tensor) else torch.from_numpy(ei).to(DEV)]
    if ea is not None:
        args.append((ea if isinstance(ea, torch.Tensor) else _dev(ea)).detach().requires_grad_(True))
    out = conv(*args)
    assert type(out) is torch.Tensor                             # the layer's result is nn's result: nothing deferred
    torch.autograd.backward([out], [gup if isinstance(gup, torch.Tensor) else _dev(gup)])
    torch.cuda.synchronize()
    grads = {"x": xg.grad}
    if ea is not None:
        grads["edge_attr"] = args[2].grad
    grads.update({name: p.grad for name, p in conv.named_parameters()})
    return out.detach(), grads


def _host(run):
    return _np(run[0]), {k: (None if v is None else _np(v)) for k, v in run[1].items()}


def _check_gine(fi, fo, d, mode, kind):
    case = gine_case(fi, fo, d, mode, kind)
    clear_cache()
    conv = _device_gine(case)
    tag = f"GINEConv {fi}->{fo} D={d} {mode} {kind}"
    if d is not None and case["ei"].shape[1]:
        # the precondition of one mask in every evaluation: the projected edge features are the same numbers
        with torch.no_grad():
            ea = _dev(case["ea"])
            got_e = conv.lin(ea.unsqueeze(-1) if ea.dim() == 1 else ea)
            want = copy.deepcopy(case["cpu"]).double().edge_features(torch.from_numpy(case["ea"]).double())
        assert torch.equal(got_e.cpu().double(), want), f"{tag}: the projected edge features are not exact"
    got = _host(_device_run(conv, case["x"], case["ei"], case["ea"], case["gup"]))
    assert ("eps" in got[1]) == case["train"] and "eps" in conv.state_dict()
    check_against_references(tag, got, case, "e_h")
    if case["n"] and fo > 1:
        assert_parity(got[0], case["r32"][0], case["r64"][0], TOL, f"{tag} forward per row", metric=row_rel_err)


@gpu
@pytest.mark.parametrize("kind", MAIN_GRAPHS)
@pytest.mark.parametrize("mode", list(EPS_MODES))
@pytest.mark.parametrize("d", EDGE_DIMS)
@pytest.mark.parametrize("fi,fo", SHAPES)
def test_gine_layer_parity(fi, fo, d, mode, kind):
    """forward and the gradients of x, edge_attr, nn, lin and eps against RefGine at 1e-5: every shape x edge_dim x
    eps mode x graph"""
    _check_gine(fi, fo, d, mode, kind)


@gpu
@pytest.mark.parametrize("kind", EDGE_GRAPHS)
@pytest.mark.parametrize("d", [None, 3])
@pytest.mark.parametrize("fi,fo", SHAPES)
def test_gine_layer_parity_edge_graphs(fi, fo, d, kind):
    """one node, no edge, no node: out = nn((1 + eps) x), the gradient of edge_attr an empty tensor"""
    _check_gine(fi, fo, d, "train", kind)
    case = gine_case(fi, fo, d, "train", kind)
    conv = _device_gine(case)
    out, grads = _device_run(conv, case["x"], case["ei"], case["ea"], case["gup"])
    x = _dev(case["x"])
    with torch.no_grad():
        assert torch.equal(out, conv.nn((1 + conv.eps) * x))
    assert grads["edge_attr"].shape == case["ea"].shape and grads["edge_attr"].numel() == 0


@gpu
@pytest.mark.parametrize("kind", MAIN_GRAPHS + EDGE_GRAPHS)
@pytest.mark.parametrize("mode", list(EPS_MODES))
@pytest.mark.parametrize("fi,fo", SHAPES)
def test_gin_layer_parity(fi, fo, mode, kind):
    """GINConv on the same graphs: the unweighted hop plus the root term"""
    case = gin_case(fi, fo, mode, kind)
    clear_cache()
    conv = dc.nn.GINConv(nn.Linear(fi, fo), eps=case["eps"], train_eps=case["train"])
    conv.load_state_dict({k: v.clone() for k, v in case["cpu"].state_dict().items()}, strict=True)
    conv = conv.to(DEV)
    got = _host(_device_run(conv, case["x"], case["ei"], None, case["gup"]))
    assert ("eps" in got[1]) == case["train"] and "eps" in conv.state_dict()
    check_against_references(f"GINConv {fi}->{fo} {mode} {kind}", got, case, "e_h")


@gpu
def test_lin_edge_features_are_exact():
    """grid ``edge_attr``, grid ``lin``: the dense block's ``lin(edge_attr)`` equals the float32 CPU evaluation bit for
    bit at every (in_channels, edge_dim) of the layer tests, and the float64 one."""
    for fi in sorted({s[0] for s in SHAPES}):
        for d in (1, 3, 16):
            rng = np.random.default_rng(fi + d)
            ea, w, b = grid_values(rng, (2400, d)), grid_weights(rng, (fi, d)), grid_weights(rng, (fi,))
            got = ops.dense_linear(_dev(ea), _dev(w), _dev(b)).cpu()
            want32 = torch.nn.functional.linear(torch.from_numpy(ea), torch.from_numpy(w), torch.from_numpy(b))
            want64 = torch.nn.functional.linear(torch.from_numpy(ea).double(), torch.from_numpy(w).double(),
                                                torch.from_numpy(b).double())
            assert torch.equal(want32.double(), want64) and torch.equal(got, want32), (fi, d)


@gpu
def test_an_arbitrary_module_is_called_forward_only():
    """``nn = Sequential(Linear, ReLU, Linear)``: the layer's output is that module applied to the aggregation"""
    n, ei = _graph("multigraph", 3)
    rng = np.random.default_rng(5)
    x, ea = rng.standard_normal((n, 21)).astype(np.float32), rng.standard_normal((ei.shape[1], 21)).astype(np.float32)
    torch.manual_seed(4)
    seq = nn.Sequential(nn.Linear(21, 32), nn.ReLU(), nn.Linear(32, 64))
    ref = RefGine(copy.deepcopy(seq), 0.3).double()
    with torch.no_grad():
        want64 = ref(torch.from_numpy(x).double(), torch.from_numpy(ei), torch.from_numpy(ea).double()).numpy()
        want32 = RefGine(copy.deepcopy(seq), 0.3)(torch.from_numpy(x), torch.from_numpy(ei), torch.from_numpy(ea)).numpy()
    calls = []
    seq[1].register_forward_hook(lambda *a: calls.append(1))
    conv = dc.nn.GINEConv(seq, eps=0.3).to(DEV)
    clear_cache()
    with torch.no_grad():
        out = conv(_dev(x), torch.from_numpy(ei).to(DEV), _dev(ea))
    assert calls == [1] and out.shape == (n, 64)
    assert_parity(_np(out), want32, want64, TOL, "GINEConv Sequential(Linear, ReLU, Linear) forward")


# --------------------------------------------------------------------------- #
# GPU: call patterns
# --------------------------------------------------------------------------- #
def _same(a, b):
    assert torch.equal(a[0], b[0]) and set(a[1]) == set(b[1])
    for name in a[1]:
        assert (a[1][name] is None and b[1][name] is None) or torch.equal(a[1][name], b[1][name]), name


@gpu
def test_launches_of_one_layer_step():
    """forward + backward of GINEConv: one kernel of dc_gine.hip per entry, no hop; without a gradient wanted for
    edge_attr (and no ``lin``) the g_e launch is skipped; GINConv: the unweighted hop each way and no GINE kernel."""
    case = gine_case(25, 256, None, "train", "multigraph")
    clear_cache()
    conv = _device_gine(case)
    x, ea, gup, tei = _dev(case["x"]), _dev(case["ea"]), _dev(case["gup"]), torch.from_numpy(case["ei"]).to(DEV)
    for ea_grad, want in ((True, {"k_gine_fwd": 1, "k_gine_bwd_x": 1, "k_gine_bwd_e": 1}),
                          (False, {"k_gine_fwd": 1, "k_gine_bwd_x": 1})):
        xg = x.clone().requires_grad_(True)
        _lib.kernel_trace(True)
        torch.autograd.backward([conv(xg, tei, ea.clone().requires_grad_(ea_grad))], [gup])
        counts = _lib.kernel_trace_counts()
        _lib.kernel_trace(False)
        gine = {name: v for name, v in counts.items() if "k_gine" in name}
        assert sum(gine.values()) == len(want) and all(any(k + "<" in name for name in gine) for k in want), counts
        assert not any("k_spmm" in name or "k_sage" in name for name in counts), counts
    gcase = gin_case(25, 256, "train", "multigraph")
    gin = dc.nn.GINConv(nn.Linear(25, 256), eps=0.3, train_eps=True).to(DEV)
    _lib.kernel_trace(True)
    _device_run(gin, gcase["x"], gcase["ei"], None, gcase["gup"])
    counts = _lib.kernel_trace_counts()
    _lib.kernel_trace(False)
    assert sum(v for name, v in counts.items() if "k_spmm" in name) == 2 and not any("k_gine" in n_ for n_ in counts), counts


@gpu
@pytest.mark.parametrize("d", [None, 3])
def test_strided_inputs_and_gradient_and_a_repeat_give_the_same_bits(d):
    fi, fo = 25, 256
    case = gine_case(fi, fo, d, "train", "multigraph")
    n, ei, x, ea, gup = case["n"], case["ei"], case["x"], case["ea"], case["gup"]
    clear_cache()
    conv = _device_gine(case, dense_block=True)
    want = _device_run(conv, x, ei, ea, gup)
    _same(_device_run(conv, x, ei, ea, gup), want)
    wide_g = torch.full((n, 2 * fo), 1e30, device=DEV)
    wide_g[:, ::2] = _dev(gup)
    xs, es, gs = _wide(_dev(x), 7, 3), _wide(_dev(ea), 5, 2), wide_g[:, ::2]
    assert not xs.is_contiguous() and not es.is_contiguous() and not gs.is_contiguous()
    _same(_device_run(conv, xs, ei, es, gs), want)


@gpu
def test_a_deferred_x_and_a_deferred_edge_attr_are_resolved():
    n, ei = _graph("multigraph", 3)
    tei = torch.from_numpy(ei).to(DEV)
    torch.manual_seed(7)
    pre = dc.nn.GCNConv(8, 16).to(DEV)
    lin = dc.nn.conv._Lin                                        # (bits are compared: ``nn`` on the package's dense block)
    conv, gin = dc.nn.GINEConv(lin(16, 4, bias=True), eps=0.3).to(DEV), dc.nn.GINConv(lin(16, 4, bias=True)).to(DEV)
    x, ea = torch.randn(n, 8, device=DEV), torch.randn(ei.shape[1], 16, device=DEV)
    with torch.no_grad():
        h = pre(x, tei)
        assert type(h).__name__ == "DeferredActivation"
        value = ops.resolve(h)
        assert torch.equal(conv(h, tei, ea), conv(value, tei, ea)) and torch.equal(gin(h, tei), gin(value, tei))
        assert type(conv(h, tei, ea)) is torch.Tensor
        # (edge features produced by a layer of this package: a conv over the line graph, say - here any deferred
        # result with E rows)
        lg_ei = torch.stack([torch.arange(ei.shape[1], device=DEV), torch.arange(ei.shape[1], device=DEV).roll(1)])
        he = dc.nn.GCNConv(16, 16).to(DEV)(ea, lg_ei)
        assert type(he).__name__ == "DeferredActivation"
        assert torch.equal(conv(value, tei, he), conv(value, tei, ops.resolve(he)))


@gpu
def test_a_batch_with_edge_attr_equals_its_graphs_run_separately():
    """``Batch.from_data_list`` of three small graphs with ``edge_attr`` through GINEConv: bit for bit the three graphs
    run one by one (the sums keep their order: the sorted set is stable within every destination)"""
    class Halve(nn.Module):
        """an ``nn`` without a matrix product: the comparison is about the aggregation, not about what a BLAS does
        with 116 rows against 40, 1 and 75"""
        in_features = 21

        def forward(self, h):
            return 0.5 * h

    rng = np.random.default_rng(8)
    datas = []
    for n, e in ((40, 300), (1, 0), (75, 500)):
        datas.append(Data(x=torch.from_numpy(rng.standard_normal((n, 21)).astype(np.float32)).to(DEV),
                          edge_index=torch.from_numpy(random_multigraph(n, e, n) if e else np.zeros((2, 0), np.int64)).to(DEV),
                          edge_attr=torch.from_numpy(grid_values(rng, (e, 3))).to(DEV)))
    conv = dc.nn.GINEConv(Halve(), eps=0.3, edge_dim=3).to(DEV)
    with torch.no_grad():
        conv.lin.weight.copy_(_dev(grid_weights(rng, (21, 3))))
        conv.lin.bias.copy_(_dev(grid_weights(rng, (21,))))
    b = Batch.from_data_list(datas)
    assert b.edge_attr.shape == (800, 3) and b.x.shape == (116, 21)
    with torch.no_grad():
        whole = conv(b.x, b.edge_index, b.edge_attr)
        parts = [conv(d.x, d.edge_index, d.edge_attr) for d in datas]
    assert whole.shape == (116, 21) and torch.equal(whole, torch.cat(parts))


@gpu
def test_a_captured_step_follows_eps_changed_in_place():
    """forward + backward with ``train_eps=True`` on ONE stream under torch.cuda.graph (no host read anywhere); eps is
    then changed in place and the graph replayed: the replay equals the eager step at the new value - the kernels read
    eps through its device pointer - and differs from the step at the old one."""
    n, ei = _graph("multigraph", 12)
    fi, fo = 32, 20
    torch.manual_seed(3)
    # (``nn`` on the package's own dense block, whose launches are known to capture)
    conv = dc.nn.GINEConv(dc.nn.conv._Lin(fi, fo, bias=True), eps=0.3, train_eps=True, edge_dim=3).to(DEV)
    tei = torch.from_numpy(ei).to(DEV)
    rng = np.random.default_rng(1)
    static_x = _dev(rng.standard_normal((n, fi)).astype(np.float32)).requires_grad_(True)
    ea = _dev(grid_values(rng, (ei.shape[1], 3))).requires_grad_(True)
    gup = _dev(rng.uniform(0.5, 1.5, (n, fo)).astype(np.float32))
    leaves = [static_x, ea] + list(conv.parameters())
    for t in leaves:
        t.grad = torch.zeros_like(t)

    def step():
        for t in leaves:
            t.grad.zero_()
        out = conv(static_x, tei, ea)
        torch.autograd.backward([out], [gup])
        return out

    def snapshot(out):
        return [out.detach().clone()] + [t.grad.clone() for t in leaves]

    eager = {}
    for eps in (0.3, -0.45):
        with torch.no_grad():
            conv.eps.fill_(eps)
        clear_cache()
        eager[eps] = snapshot(step())
    torch.cuda.synchronize()
    assert not torch.equal(eager[0.3][0], eager[-0.45][0]) and not torch.equal(eager[0.3][1], eager[-0.45][1])
    with torch.no_grad():
        conv.eps.fill_(0.3)
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
    for eps in (0.3, -0.45, 0.3):
        with torch.no_grad():
            conv.eps.fill_(eps)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(snapshot(out), eager[eps]):
            assert torch.equal(got, want), eps
