"""``PointNetConv``: the layer, ``ops.pointnet_pairs`` / ``ops.pointnet_aggregate`` and the C entries of dc_pointnet.hip
that serve it, and one small PointNet++ through the ``torch_geometric`` alias.

The reference is this file's own restatement of the contract in INTEGRATION.md 1.12 (PyG 2.5.2 point_conv.py):
``RefPointNetConv``, a torch CPU module evaluated in float32 (``ref32``) and float64 (``truth64``) with gradients from
torch autograd, and numpy formulas for the entries called directly.  Its max is the mask / count form of
tests/test_edge_conv.py, so autograd yields the library's tie rule (the even split among all edge rows that attain the
maximum).  ``add_self_loops=True`` is restated as PyG's remove-then-add: the input edges with ``src == dst`` are dropped
and one loop per node is appended.

One selection in every evaluation, as in tests/test_edge_conv.py: the cases with ``aggr="max"`` and all cases whose
``local_nn`` is ``Sequential(Linear, ReLU, Linear)`` take ``x`` and the positions from multiples of 1/4 in [-2, 2] and
the parameters from multiples of 1/8 in [-1, 1]: a message row holds multiples of 1/4 in [-4, 4] (F + 3 <= 67 of them),
so a first-layer output is a sum of at most 68 multiples of 1/32 below 2^9 and, with 16 hidden units, a second-layer
output a sum of 17 multiples of 1/256 below 2^13 - exact float32 numbers in any summation order.  That exactness is
asserted on the CPU (float32 == float64) and on the device before a layer is compared.  ``Linear`` under mean / sum
runs on N(0, 1) inputs with the default initialisation.

Shapes.  ``bip``: Ns = 37 sources, Nd = 13 destinations, 220 edges with duplicates, destination 12 without in-edges
and source 36 without out-edges.  ``sq``: a 40-node multigraph of 300 edges with input self loops, duplicates and nodes
without in-edges, run with ``add_self_loops`` False (``sq``) and True (``sql``).  No graph has a hub, so the float32
restatement itself stays within the 1e-5 bar of float64, which is asserted.

Metrics.  The layer through ``helpers.assert_parity`` at 1e-5.  The entries: ``dc_pointnet_pair_fwd`` bit-identical to
numpy (a copy and ONE fp32 subtraction); ``dc_pointnet_pair_bwd`` (compensated sums) within 1e-5 per row of a float64
``index_add`` of the same terms; the forward reduction bit-identical to a numpy float32 loop over the device's own
``ptr`` / ``perm``; ``dc_pointnet_reduce_bwd`` bit-identical to the numpy float32 formula (every term one copy or one
division).
"""
import copy
import functools
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import deformcontact_amd as dc
from deformcontact_amd import _lib, ops
from deformcontact_amd.graph import GraphIndex, clear_cache
from deformcontact_amd.nn import PointNetConv  # noqa: F401  (the module needs the layer: no test runs without it)
from tests.helpers import assert_parity, random_multigraph, record_parity, rel_err, row_rel_err
from tests.test_edge_conv import (Mix, _device_nn, _index_add, _odd, _wide, coarse_grid, grid_values, grid_weights,
                                  segment_max, signed, sum_loop_f32)
from tests.test_gat_edge_kernels import _dev, _np

gpu = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5

#: (F, C) of the layer tests; F = 0: x = None
SHAPES = [(3, 64), (0, 20), (64, 20), (16, 1)]
AGGRS = ["max", "mean", "sum"]
HIDDEN = 16
GLOBAL_OUT = 8
#: kind -> add_self_loops
KINDS = {"bip": False, "sq": False, "sql": True}
#: pair kernels: F = 0 (positions alone), the general form (1, 3, 70) and the 16-byte form of the x columns (20, 64, 256)
PAIR_WIDTHS = [0, 1, 3, 20, 64, 70, 256]
REDUCE_WIDTHS = [1, 3, 20, 64, 70, 256, 1100]
MODES = {"sum": 0, "mean": 1, "max": 2}


# --------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------- #
def _graph(kind):
    """(ns, nd, edge_index [2, E] int64, loops)"""
    if kind == "bip":
        rng = np.random.default_rng(5)
        src, dst = rng.integers(0, 36, 220), rng.integers(0, 12, 220)        # source 36, destination 12: no edge
        src[:6], dst[:6] = src[6:12], dst[6:12]                              # duplicates
        return 37, 13, np.stack([src, dst]).astype(np.int64), False
    if kind in ("sq", "sql"):
        return 40, 40, random_multigraph(40, 300, 4), KINDS[kind]
    if kind == "e0":
        return 9, 5, np.zeros((2, 0), np.int64), False
    if kind == "nd0":
        return 6, 0, np.zeros((2, 0), np.int64), False
    if kind == "ns0":
        return 0, 4, np.zeros((2, 0), np.int64), False
    assert kind == "n0"
    return 0, 0, np.zeros((2, 0), np.int64), False


def edge_rows(kind):
    """the edge rows that take part: (row ids, src, dst, number of rows E') - with loops the input edges with src != dst
    and then row E + i = (i, i)"""
    ns, nd, ei, loops = _graph(kind)
    ne = ei.shape[1]
    if not loops:
        return np.arange(ne), ei[0], ei[1], ne
    keep = np.flatnonzero(ei[0] != ei[1])
    loop = np.arange(ns)
    return np.concatenate([keep, ne + loop]), np.concatenate([ei[0][keep], loop]), np.concatenate([ei[1][keep], loop]), ne + ns


def _positions(rng, n, grid):
    return grid_values(rng, (n, 3)) if grid else rng.standard_normal((n, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pair_case(kind, f):
    """inputs and order-independent references of the pair kernels (computed once, never modified)"""
    ns, nd, ei, loops = _graph(kind)
    rows, src, dst, nrows = edge_rows(kind)
    ne = ei.shape[1]
    rng = np.random.default_rng(3000 + f + len(kind))
    x = rng.standard_normal((ns, f)).astype(np.float32)
    ps = _positions(rng, ns, False)
    pd = ps if ns == nd and kind != "bip" else _positions(rng, nd, False)
    gz = rng.standard_normal((nrows, f + 3)).astype(np.float32)
    z = np.concatenate([x[ei[0]], ps[ei[0]] - pd[ei[1]]], axis=1)            # a copy and ONE fp32 subtraction
    if loops:
        z = np.concatenate([z, np.concatenate([x, np.zeros((ns, 3), np.float32)], axis=1)])
    assert z.dtype == np.float32 and z.shape == (nrows, f + 3)
    real = rows < ne                                                         # the loops carry no position gradient
    gx64 = _index_add(ns, src, gz[rows][:, :f])
    gps64 = _index_add(ns, src[real], gz[rows[real]][:, f:])
    gpd64 = -_index_add(nd, dst[real], gz[rows[real]][:, f:])
    return dict(ns=ns, nd=nd, ei=ei, loops=loops, x=x, ps=ps, pd=pd, gz=gz, z=z, gx64=gx64, gps64=gps64, gpd64=gpd64)


@functools.lru_cache(maxsize=None)
def reduce_case(kind, c):
    ns, nd, ei, loops = _graph(kind)
    rows, src, dst, nrows = edge_rows(kind)
    rng = np.random.default_rng(4000 + c + len(kind))
    deg = np.bincount(dst, minlength=nd)
    m, mg, gy = rng.standard_normal((nrows, c)).astype(np.float32), coarse_grid(rng, (nrows, c)), signed(rng, (nd, c))
    y, cnt = segment_max(nd, dst, mg[rows])
    degf = np.maximum(deg, 1).astype(np.float32)[:, None]
    part = {"sum": gy[dst], "mean": gy[dst] / degf[dst],
            "max": np.where(mg[rows] == y[dst], gy[dst] / np.maximum(cnt, 1).astype(np.float32)[dst], np.float32(0))}
    gm = {}
    for name, v in part.items():
        assert v.dtype == np.float32
        gm[name] = np.zeros((nrows, c), np.float32)                          # a removed input loop: a zero row
        gm[name][rows] = v
    return dict(ns=ns, nd=nd, ei=ei, loops=loops, deg=deg, m=m, mg=mg, gy=gy, y=y, cnt=cnt, gm=gm,
                sum64=_index_add(nd, dst, m[rows]))


# --------------------------------------------------------------------------- #
# the restatement as a torch module (float32: ref32, .double(): truth64)
# --------------------------------------------------------------------------- #
def ref_segment(msg, i, n, aggr):
    """sum / mean / max (mask / count form: the even split) of the rows ``msg`` per index ``i`` -> [n, C]"""
    zeros = msg.new_zeros((n, msg.size(1)))
    if aggr == "max":
        with torch.no_grad():                                    # mask and cnt are constants
            y, _ = segment_max(n, i.numpy(), msg.numpy())
            mask = (msg == torch.from_numpy(y)[i]).to(msg.dtype)
            cnt = zeros.clone().index_add_(0, i, mask)
        return zeros.index_add_(0, i, mask * msg / cnt[i].clamp(min=1))
    out = zeros.index_add_(0, i, msg)
    if aggr == "mean":
        out = out / torch.bincount(i, minlength=n).clamp(min=1).to(msg.dtype)[:, None]
    return out


class RefPointNetConv(nn.Module):
    def __init__(self, local_nn=None, global_nn=None, add_self_loops=True, aggr="max"):
        super().__init__()
        self.local_nn, self.global_nn, self.add_self_loops, self.aggr = local_nn, global_nn, add_self_loops, aggr

    def edges(self, edge_index, n):
        j, i = edge_index
        if self.add_self_loops:                                  # PyG: remove_self_loops, then add_self_loops
            keep = j != i
            loop = torch.arange(n)
            j, i = torch.cat([j[keep], loop]), torch.cat([i[keep], loop])
        return j, i

    def messages(self, x_src, pos_src, pos_dst, edge_index):
        j, i = self.edges(edge_index, pos_dst.size(0))
        msg = pos_src[j] - pos_dst[i]
        if x_src is not None:
            msg = torch.cat([x_src[j], msg], dim=1)
        return (self.local_nn(msg) if self.local_nn is not None else msg), i

    def forward(self, x_src, pos_src, pos_dst, edge_index):
        msg, i = self.messages(x_src, pos_src, pos_dst, edge_index)
        out = ref_segment(msg, i, pos_dst.size(0), self.aggr)
        return self.global_nn(out) if self.global_nn is not None else out


def _ref_run(mod, case, dtype):
    for p in mod.parameters():
        p.grad = None
    leaf = lambda a: None if a is None else torch.from_numpy(a).to(dtype).requires_grad_(True)
    x, ps = leaf(case["x"]), leaf(case["ps"])
    pd = ps if case["one_pos"] else leaf(case["pd"])
    out = mod(x, ps, pd, torch.from_numpy(case["ei"]))
    (out * torch.from_numpy(case["gup"]).to(dtype)).sum().backward()
    none = lambda t: None if t is None else (np.zeros(t.shape, t.detach().numpy().dtype) if t.grad is None else t.grad.numpy())
    grads = {"pos_src": none(ps)}
    if x is not None:
        grads["x"] = none(x)
    if not case["one_pos"]:
        grads["pos_dst"] = none(pd)
    grads.update({name: p.grad.detach().numpy().copy() for name, p in mod.named_parameters()})
    return out.detach().numpy(), grads


def make_local(fi, fo, seq):
    return nn.Sequential(nn.Linear(fi + 3, HIDDEN), nn.ReLU(), nn.Linear(HIDDEN, fo)) if seq else nn.Linear(fi + 3, fo)


def _with_global(fi, aggr, seq):
    return (len(aggr) + seq + fi) % 2 == 0


@functools.lru_cache(maxsize=None)
def layer_case(fi, fo, aggr, seq, kind):
    """inputs, the reference module and its float32 / float64 results of one PointNetConv case; ``exact``: grid inputs
    and grid parameters (every max case, every Sequential case)"""
    torch.set_num_threads(1)
    ns, nd, ei, loops = _graph(kind)
    rng = np.random.default_rng(fi + fo + len(aggr) + 7 * seq + len(kind))
    glob = _with_global(fi, aggr, seq)
    gup = rng.uniform(0.5, 1.5, (nd, GLOBAL_OUT if glob else fo)).astype(np.float32)
    torch.manual_seed(12)
    cpu = RefPointNetConv(make_local(fi, fo, seq), nn.Linear(fo, GLOBAL_OUT) if glob else None, loops, aggr)
    exact = aggr == "max" or seq
    one_pos = kind != "bip" and ns == nd
    if exact:
        with torch.no_grad():
            for p in cpu.parameters():
                p.copy_(torch.from_numpy(grid_weights(rng, tuple(p.shape))))
    x = None if fi == 0 else (grid_values(rng, (ns, fi)) if exact else rng.standard_normal((ns, fi)).astype(np.float32))
    ps = _positions(rng, ns, exact)
    pd = ps if one_pos else _positions(rng, nd, exact)
    case = dict(ns=ns, nd=nd, ei=ei, loops=loops, x=x, ps=ps, pd=pd, one_pos=one_pos, gup=gup, cpu=cpu, aggr=aggr,
                exact=exact, glob=glob)
    case["r32"] = _ref_run(cpu, case, torch.float32)
    case["r64"] = _ref_run(copy.deepcopy(cpu).double(), case, torch.float64)
    return case


MAIN_KINDS = ["bip", "sq", "sql"]
EDGE_KINDS = ["e0", "nd0", "ns0", "n0"]


def _layer_cases(kinds):
    return [(fi, fo, aggr, seq, kind) for (fi, fo) in SHAPES for aggr in AGGRS for seq in (False, True) for kind in kinds]


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
def test_constructor_repr_state_dict_and_reset_parameters():
    local = nn.Sequential(nn.Linear(6, 32), nn.ReLU(), nn.Linear(32, 64))
    glob = nn.Linear(64, 10)
    conv = dc.nn.PointNetConv(local, glob)
    assert conv.aggr == "max" and conv.add_self_loops is True and conv.local_nn is local and conv.global_nn is glob
    assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == {
        "local_nn.0.weight": (32, 6), "local_nn.0.bias": (32,), "local_nn.2.weight": (64, 32), "local_nn.2.bias": (64,),
        "global_nn.weight": (10, 64), "global_nn.bias": (10,)}
    assert repr(conv).startswith("PointNetConv(local_nn=Sequential(") and "global_nn=Linear(" in repr(conv)
    assert repr(dc.nn.PointNetConv()) == "PointNetConv(local_nn=None, global_nn=None)"
    assert conv.graph_flags() == dict(self_loops=True, normalize=False)
    assert dc.nn.PointNetConv(local, add_self_loops=False).graph_flags() == dict(self_loops=False, normalize=False)
    assert not hasattr(conv, "supports_fused_relu") and not hasattr(conv, "bias") and not hasattr(conv, "lin")
    assert dc.nn.PointNetConv().state_dict() == {} and not hasattr(dc.nn, "PointConv")
    ref = RefPointNetConv(copy.deepcopy(local), copy.deepcopy(glob))
    assert set(ref.state_dict()) == set(conv.state_dict())
    with torch.no_grad():
        for p in ref.parameters():
            p.add_(1.0)
    conv.load_state_dict(ref.state_dict(), strict=True)
    for k, v in ref.state_dict().items():
        assert torch.equal(conv.state_dict()[k], v), k
    before = [p.detach().clone() for p in conv.parameters()]
    conv.reset_parameters()
    after = [p.detach() for p in conv.parameters()]
    assert len(after) == 6 and all(not torch.equal(a, b) for a, b in zip(after, before))
    dc.nn.PointNetConv().reset_parameters()                      # no module: nothing to reset
    # positional order as in PyG: local_nn, global_nn, add_self_loops
    c = dc.nn.PointNetConv(None, glob, False, aggr="mean")
    assert c.local_nn is None and c.global_nn is glob and c.add_self_loops is False and c.aggr == "mean"


def test_aggr_is_validated_and_add_is_sum():
    for aggr, want in (("max", "max"), ("mean", "mean"), ("sum", "sum"), ("add", "sum")):
        assert dc.nn.PointNetConv(nn.Linear(6, 4), aggr=aggr).aggr == want
    for bad in ("min", "mul", "", None, 2, ["max"], ["max", "mean"], ("sum",), nn.Identity()):
        with pytest.raises(ValueError, match="aggr"):
            dc.nn.PointNetConv(nn.Linear(6, 4), aggr=bad)


def test_errors_raised_on_the_host():
    x, pos, ei = torch.zeros(5, 3), torch.zeros(5, 3), torch.zeros(2, 4, dtype=torch.long)
    pos_d = torch.zeros(2, 3)
    loops, plain = dc.nn.PointNetConv(nn.Linear(6, 2)), dc.nn.PointNetConv(nn.Linear(6, 2), add_self_loops=False)
    # a pair needs add_self_loops=False: the message says what to pass
    for xx, pp in ((x, (pos, pos_d)), ((x, None), pos), ((x, x), (pos, pos)), ([x, None], [pos, pos_d]), (None, (pos, pos_d))):
        with pytest.raises(ValueError, match="add_self_loops=False"):
            loops(xx, pp, ei)
    for conv in (loops, plain):
        for bad in (torch.zeros(5, 2), torch.zeros(5, 4), torch.zeros(5), torch.zeros(5, 3, 1)):
            with pytest.raises(ValueError, match=r"\[N, 3\]"):
                conv(x, bad, ei)                                 # position widths other than 3
        with pytest.raises(ValueError, match="float32"):
            conv(x, pos.double(), ei)
        with pytest.raises(ValueError, match="float32"):
            conv(x.double(), pos, ei)
        with pytest.raises(ValueError, match="4 rows.*5"):
            conv(x[:4], pos, ei)                                 # both numbers are named
        for bad in (x[0], torch.zeros(5, 0)):
            with pytest.raises(ValueError, match="F >= 1"):
                conv(bad, pos, ei)
        with pytest.raises(TypeError, match="tensor"):
            conv(x, "pos", ei)
        with pytest.raises(TypeError, match="tensor"):
            conv("x", pos, ei)
        with pytest.raises(TypeError, match="SparseTensor"):
            conv(x, pos, None)
        for unsupported in (dict(size=(5, 5)), dict(relu=True), dict(next_conv=None), dict(edge_attr=None)):
            with pytest.raises(TypeError):
                conv(x, pos, ei, **unsupported)                  # not supported: absent from the signature
        with pytest.raises(RuntimeError, match="HIP device"):
            conv(x, pos, ei)                                     # every host check passed: no CPU path
        with pytest.raises(RuntimeError, match="HIP device"):
            conv(None, pos, ei)
    with pytest.raises(ValueError, match="float32"):
        plain((x, None), (pos, pos_d.double()), ei)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        plain((x, None), (pos, torch.zeros(2, 2)), ei)
    with pytest.raises(ValueError, match="3 rows.*5"):
        plain((x[:3], None), (pos, pos_d), ei)
    with pytest.raises(ValueError, match="x_dst has 5 rows.*2"):
        plain((x, x), (pos, pos_d), ei)
    with pytest.raises(ValueError, match="2 entries"):
        plain(x, (pos, pos_d, pos_d), ei)
    with pytest.raises(RuntimeError, match="HIP device"):
        plain((x, None), (pos, pos_d), ei)
    with pytest.raises(RuntimeError, match="HIP device"):
        plain((x, x[:2]), (pos, pos_d), ei)
    # the ops: the reduce check comes before anything else, the device check included
    for bad in ("add", "min", None, 3, ["max"]):
        with pytest.raises(ValueError, match="reduce must be"):
            ops.pointnet_aggregate(None, torch.zeros(4, 2), bad)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.pointnet_aggregate(None, torch.zeros(4, 2))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.pointnet_pairs(None, x, pos, pos)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.pointnet_pairs(None, None, pos, pos_d)


def test_exports_and_the_torch_geometric_alias():
    from deformcontact_amd.pyg_alias import install_as_torch_geometric
    names = dc.nn.__all__
    at = names.index("SAGEConv")
    assert names[at:at + 6] == ["SAGEConv", "PointNetConv", "global_add_pool", "global_mean_pool", "global_max_pool",
                                "GINConv"]
    assert len(names) == len(set(names)) and names[-3:] == ["SplineConv", "GMMConv", "ChebConv"]
    assert dc.nn.PointNetConv is PointNetConv
    mods = ("torch_geometric", "torch_geometric.nn", "torch_geometric.data")
    saved = {k: sys.modules.get(k) for k in mods}
    try:
        install_as_torch_geometric(force=True)
        from torch_geometric.nn import PointNetConv as aliased, global_max_pool, global_mean_pool, global_add_pool
        assert aliased is dc.nn.PointNetConv and global_max_pool is dc.pointops.global_max_pool
        assert global_mean_pool is dc.pointops.global_mean_pool and global_add_pool is dc.pointops.global_add_pool
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_the_exact_set_of_new_symbols():
    import os
    new = sorted(n for n in _lib.exported_names() if n.startswith(("dc_pointnet_", "dc_pool_")))
    assert new == ["dc_pointnet_pair_bwd", "dc_pointnet_pair_fwd", "dc_pointnet_reduce_bwd", "dc_pool_bwd", "dc_pool_fwd"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "deformcontact.h")) as fh:
        header = fh.read()
    for name in new:
        assert f"int {name}(" in header and hasattr(_lib.lib(), name)


def _pair_fwd(L, rows, f, ok, ld, ns=3, nd=3, loops=0):
    p = lambda a: a if ok else None
    return L.dc_pointnet_pair_fwd(p(64), p(64), p(128), ld, p(192), 3, p(320), 3, p(256), ld + 3, ns, nd, rows, f, loops, 0,
                                  None)


def _pair_bwd(L, rows, f, ok, ld, nd=None, loops=0):
    p = lambda a: a if ok else None                              # (the outputs are given: without any there is no work)
    return L.dc_pointnet_pair_bwd(p(64), p(64), p(64), p(64), p(64), p(64), p(128), ld + 3, 256, ld, 320, 3, 384,
                                  3, rows, rows if nd is None else nd, 5, f, loops, None)


def _reduce_bwd(L, rows, c, ok, ld, mode=0, loops=0):
    p = lambda a, on=True: a if ok and on else None
    return L.dc_pointnet_reduce_bwd(p(64), p(64), p(64), p(128, mode == 2), ld, p(256, mode == 2), ld, p(320, mode == 2),
                                    ld, p(384), ld, p(448), ld, mode, 3, 3, rows, c, loops, None)


def test_abi_argument_errors_of_the_pointnet_entries_without_gpu():
    """short leading dimensions, null pointers, aliased outputs, a bad mode, loops on two node sets, sizes out of
    range: -1 and the entry's own message, before any HIP call; a zero row count returns 0 with no pointer at all."""
    L = _lib.lib()
    err = L.dc_last_error
    for name, call in (("dc_pointnet_pair_fwd", _pair_fwd), ("dc_pointnet_pair_bwd", _pair_bwd),
                       ("dc_pointnet_reduce_bwd", _reduce_bwd)):
        tag = name.encode()
        assert call(L, 3, 16, False, 64) == -1 and tag in err() and b"null" in err(), name
        assert call(L, 3, 16, True, 15) == -1 and tag in err() and b"leading" in err(), name
        assert call(L, 3, 16, False, 15) == -1 and b"leading" in err(), name          # sizes, strides, then nulls
        assert call(L, 0, 16, False, 64) == 0, name              # no row: nothing is read, written or launched
        assert call(L, 0, 16, False, 15) == -1, name
        assert call(L, -1, 16, True, 64) == -1 and tag in err(), name
        assert call(L, 3, -2, True, 64) == -1 and tag in err(), name
        assert call(L, 3, 1 << 24, True, 1 << 24) == -1 and b"range" in err(), name
        assert call(L, 1 << 30, 16, True, 64) == -1 and b"range" in err(), name
    # F = 0 is legal for the pair entries (x and gx may be NULL then), a width of 0 is not for the reduction
    assert L.dc_pointnet_pair_fwd(None, None, None, 0, None, 3, None, 3, None, 3, 3, 3, 0, 0, 0, 0, None) == 0
    assert L.dc_pointnet_pair_fwd(64, 64, None, 0, None, 3, 320, 3, 256, 3, 3, 3, 5, 0, 0, 0, None) == -1 and b"null" in err()
    assert L.dc_pointnet_pair_bwd(None, None, None, None, None, None, None, 3, None, 1, None, 3, None, 3, 0, 0, 0, 0, 0,
                                  None) == 0
    assert _reduce_bwd(L, 3, 0, True, 64) == -1 and b"dc_pointnet_reduce_bwd" in err()
    # no output wanted: nothing to do, whatever else is NULL
    assert L.dc_pointnet_pair_bwd(None, None, None, None, None, None, None, 19, None, 16, None, 3, None, 3, 3, 3, 5, 16, 0,
                                  None) == 0
    # loops need one node set; with loops the N appended rows are rows too (E = 0 launches)
    assert _pair_fwd(L, 3, 16, True, 64, ns=3, nd=4, loops=1) == -1 and b"loops" in err()
    assert _pair_bwd(L, 3, 16, True, 64, nd=4, loops=1) == -1 and b"loops" in err()
    assert L.dc_pointnet_reduce_bwd(64, 64, 64, None, 16, None, 16, None, 16, 384, 16, 448, 16, 0, 4, 3, 5, 16, 1,
                                    None) == -1 and b"loops" in err()
    assert _pair_fwd(L, 0, 16, False, 64, loops=1) == -1 and b"null" in err()
    assert _reduce_bwd(L, 0, 16, False, 64, loops=1) == -1 and b"null" in err()
    # n_dst beyond the adjacency's rows
    assert L.dc_pointnet_reduce_bwd(64, 64, 64, None, 16, None, 16, None, 16, 384, 16, 448, 16, 0, 3, 4, 5, 16, 0,
                                    None) == -1 and b"n_dst" in err()
    # the position operands and z of the pair rows: 3 and F + 3 columns
    assert L.dc_pointnet_pair_fwd(64, 64, 128, 16, 192, 2, 320, 3, 256, 19, 3, 3, 5, 16, 0, 0, None) == -1 and b"leading" in err()
    assert L.dc_pointnet_pair_fwd(64, 64, 128, 16, 192, 3, 320, 3, 256, 18, 3, 3, 5, 16, 0, 0, None) == -1 and b"leading" in err()
    assert L.dc_pointnet_pair_bwd(64, 64, 64, 64, 64, 64, 128, 18, 256, 16, 320, 3, 384, 3, 3, 3, 5, 16, 0, None) == -1 \
        and b"leading" in err()
    # zpad: 0..3 further zero columns of z, which the leading dimension must hold
    for bad in (-1, 4):
        assert L.dc_pointnet_pair_fwd(64, 64, 128, 16, 192, 3, 320, 3, 256, 24, 3, 3, 5, 16, 0, bad, None) == -1 \
            and b"zpad" in err()
    assert L.dc_pointnet_pair_fwd(64, 64, 128, 16, 192, 3, 320, 3, 256, 19, 3, 3, 5, 16, 0, 1, None) == -1 and b"leading" in err()
    assert L.dc_pointnet_pair_fwd(None, None, None, 16, None, 3, None, 3, None, 20, 3, 3, 0, 16, 0, 1, None) == 0
    # outputs that alias an operand or each other
    assert L.dc_pointnet_pair_fwd(64, 64, 128, 16, 192, 3, 320, 3, 128, 19, 3, 3, 5, 16, 0, 0, None) == -1 and b"alias" in err()
    assert L.dc_pointnet_pair_fwd(64, 64, 128, 16, 192, 3, 320, 3, 320, 19, 3, 3, 5, 16, 0, 0, None) == -1 and b"alias" in err()
    assert L.dc_pointnet_pair_bwd(64, 64, 64, 64, 64, 64, 128, 19, 128, 16, 320, 3, 384, 3, 3, 3, 5, 16, 0, None) == -1 \
        and b"alias" in err()
    assert L.dc_pointnet_pair_bwd(64, 64, 64, 64, 64, 64, 128, 19, 256, 16, 320, 3, 320, 3, 3, 3, 5, 16, 0, None) == -1 \
        and b"alias" in err()
    assert L.dc_pointnet_reduce_bwd(64, 64, 64, None, 16, None, 16, None, 16, 384, 16, 384, 16, 0, 3, 3, 5, 16, 0,
                                    None) == -1 and b"alias" in err()
    for other in (128, 256, 320):                                # gm on m, y, cnt of the max
        assert L.dc_pointnet_reduce_bwd(64, 64, 64, 128, 16, 256, 16, 320, 16, 384, 16, other, 16, 2, 3, 3, 5, 16, 0,
                                        None) == -1 and b"alias" in err()
    for mode in (0, 1, 2):
        assert _reduce_bwd(L, 3, 16, False, 64, mode) == -1 and b"null" in err(), mode
        assert _reduce_bwd(L, 3, 16, True, 15, mode) == -1 and b"leading" in err(), mode
        assert _reduce_bwd(L, 0, 16, False, 64, mode) == 0, mode
    for mode in (-1, 3, 7):
        assert _reduce_bwd(L, 3, 16, True, 64, mode) == -1 and b"mode" in err() and b"dc_pointnet_reduce_bwd" in err()
        assert _reduce_bwd(L, 0, 16, False, 64, mode) == -1 and b"mode" in err(), mode
    assert L.dc_pointnet_reduce_bwd(64, 64, None, None, 16, None, 16, None, 16, 384, 16, 448, 16, 1, 3, 3, 5, 16, 0,
                                    None) == -1 and b"null" in err()          # the mean reads ptr
    assert L.dc_pointnet_reduce_bwd(64, 64, 64, 128, 16, 256, 16, None, 16, 384, 16, 448, 16, 2, 3, 3, 5, 16, 0,
                                    None) == -1 and b"null" in err()          # the max reads cnt


def test_float32_restatement_within_the_bar_of_float64_and_exact_where_it_has_to_be():
    """Every layer case of the GPU tests: the float32 and the float64 restatement agree within 1e-5, output and every
    gradient; in the exact cases the messages - and with them every selection - are the same numbers in float32 and
    float64, and the max cases do hold ties."""
    for fi, fo, aggr, seq, kind in _layer_cases(MAIN_KINDS + EDGE_KINDS):
        case = layer_case(fi, fo, aggr, seq, kind)
        tag = f"RefPointNetConv fp32 vs fp64 {fi}->{fo} {aggr} seq={seq} {kind}"
        check_against_references(tag, case["r32"], case, "e_o")
        assert case["r32"][0].shape == (case["nd"], GLOBAL_OUT if case["glob"] else fo)
        if case["exact"]:
            t = lambda a, dt: None if a is None else torch.from_numpy(a).to(dt)
            with torch.no_grad():
                tei = torch.from_numpy(case["ei"])
                m32, i = case["cpu"].messages(t(case["x"], torch.float32), t(case["ps"], torch.float32),
                                              t(case["pd"], torch.float32), tei)
                m64, _ = copy.deepcopy(case["cpu"]).double().messages(
                    t(case["x"], torch.float64), t(case["ps"], torch.float64), t(case["pd"], torch.float64), tei)
            assert torch.equal(m32.double(), m64), tag
            if aggr == "max" and kind in MAIN_KINDS:
                _, cnt = segment_max(case["nd"], i.numpy(), m32.numpy())
                assert (cnt >= 2).any(), tag


def test_reference_formulas_agree_with_autograd():
    """the hand-written gradients of the entry tests against float64 autograd of the torch composition: the pair
    backward (sums of the same terms) and the reduce gradients through the mask / count form"""
    for kind in MAIN_KINDS:
        rows, src, dst, nrows = edge_rows(kind)
        case = pair_case(kind, 20)
        ns, nd, ne, f = case["ns"], case["nd"], case["ei"].shape[1], 20
        leaf = lambda a: torch.from_numpy(a).double().requires_grad_(True)
        x, ps, pd = leaf(case["x"]), leaf(case["ps"]), leaf(case["pd"])
        j, i = torch.from_numpy(src), torch.from_numpy(dst)
        real = torch.from_numpy(rows < ne).double()[:, None]    # a loop's position columns are the constant 0
        z = torch.cat([x[j], (ps[j] - pd[i]) * real], dim=1)
        (z * torch.from_numpy(case["gz"][rows]).double()).sum().backward()
        assert rel_err(case["gx64"], x.grad.numpy()) < 1e-12 and rel_err(case["gps64"], ps.grad.numpy()) < 1e-12
        assert rel_err(case["gpd64"], pd.grad.numpy()) < 1e-12, kind
        if case["loops"]:                                        # the rows of the restated set are the library's rows
            assert np.array_equal(_np(z[len(rows) - ns:, :f]), case["z"][ne:, :f].astype(np.float64))
            assert (case["z"][ne:, f:] == 0).all() and (_np(z[len(rows) - ns:, f:]) == 0).all()
        case = reduce_case(kind, 20)
        assert (case["cnt"] >= 2).mean() > 0.1                  # ties
        assert (case["deg"] == 0).any() != case["loops"]        # a destination without in-edges, unless loops are added
        i = torch.from_numpy(dst)
        for mode, values in (("sum", "m"), ("mean", "m"), ("max", "mg")):
            mt = torch.from_numpy(case[values]).double().requires_grad_(True)
            out = ref_segment(mt[torch.from_numpy(rows)], i, nd, mode)
            if mode == "max":
                assert rel_err(out.detach().numpy(), case["y"]) < 1e-14
            (out * torch.from_numpy(case["gy"]).double()).sum().backward()
            assert rel_err(case["gm"][mode], mt.grad.numpy()) < 1e-6, (kind, mode)
            removed = np.setdiff1d(np.arange(nrows), rows)
            assert (case["gm"][mode][removed] == 0).all() and (removed.size > 0) == case["loops"]


# --------------------------------------------------------------------------- #
# GPU: the entries called directly
# --------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def _device_graph(kind):
    """the adjacency of ``kind`` and its two sorted sets read back: (g, ptr, perm, ptr_t, perm_t)"""
    ns, nd, ei, loops = _graph(kind)
    rows, src, dst, nrows = edge_rows(kind)
    n, ne = max(ns, nd), ei.shape[1]
    g = GraphIndex(torch.from_numpy(ei).to(DEV), n, self_loops=loops, normalize=False, validate=True)
    ptr, tptr = _np(g.fwd.ptr).astype(np.int64), _np(g.bwd.ptr).astype(np.int64)
    perm, tperm = _np(g.fwd.perm).astype(np.int64)[:ptr[-1]], _np(g.bwd.perm).astype(np.int64)[:tptr[-1]]
    # the device's own sorted sets: the rows that take part, each once; a loop is E + i and the LAST of its groups
    assert ptr[0] == 0 and ptr[-1] == len(rows) and np.array_equal(np.sort(perm), np.sort(rows))
    assert tptr[-1] == len(rows) and np.array_equal(np.sort(tperm), np.sort(rows))
    lookup_s, lookup_d = np.zeros(nrows, np.int64), np.zeros(nrows, np.int64)
    lookup_s[rows], lookup_d[rows] = src, dst
    assert np.array_equal(lookup_d[perm], np.repeat(np.arange(n), np.diff(ptr)))
    assert np.array_equal(lookup_s[tperm], np.repeat(np.arange(n), np.diff(tptr)))
    assert np.array_equal(_np(g.fwd.other).astype(np.int64)[:ptr[-1]], lookup_s[perm])
    assert np.array_equal(_np(g.bwd.other).astype(np.int64)[:tptr[-1]], lookup_d[tperm])
    if loops:
        assert np.array_equal(perm[ptr[1:] - 1], ne + np.arange(n)) and np.array_equal(tperm[tptr[1:] - 1], ne + np.arange(n))
    else:
        assert (np.diff(ptr)[nd:] == 0).all() and (np.diff(tptr)[ns:] == 0).all()
    return g, ptr, perm, tptr, tperm


def _strided_pos(t, off):
    """positions as a row-strided view: ``[N, 3]`` inside a ``[N, 5]`` buffer at column ``off``"""
    buf = torch.full((t.size(0), 5), 1e30, device=t.device)
    buf[:, off:off + 3] = t
    return buf[:, off:off + 3]


def _quad(t):
    """``t`` as a column slice at offset 4 of a buffer 16 columns wider: rows 16-byte aligned, and a row stride that is
    a multiple of 4 where the width + 3 is one (the pair rows of F % 4 == 0: F + 3 + 13) - what the 16-byte forms need"""
    buf = torch.full((t.size(0), t.size(1) + 13), 1e30, device=t.device)
    buf[:, 4:4 + t.size(1)] = t
    return buf[:, 4:4 + t.size(1)]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _within_bar_of_float64(got, want64, name):
    d = row_rel_err(got, want64)
    print(f"{name}: row_rel_err vs float64 = {d:.3e}")
    record_parity(name, None, e_h=d, metric="row_rel_err")
    assert d < TOL, (name, d)


def _pair_inputs(case):
    x = _dev(case["x"]) if case["x"].shape[1] else None
    ps = _dev(case["ps"])
    return x, ps, (ps if case["pd"] is case["ps"] else _dev(case["pd"]))


@gpu
@pytest.mark.parametrize("kind", MAIN_KINDS)
@pytest.mark.parametrize("f", PAIR_WIDTHS)
def test_pair_forward_entry(f, kind):
    """bit-identical to numpy; x as a column slice (aligned and not), positions with a row stride: the same bits; z with
    a padded row stride or inside a wider buffer: the same values and nothing beside them; ``ops.pointnet_pairs``: the
    same bits; twice: the same bits"""
    case = pair_case(kind, f)
    g = _device_graph(kind)[0]
    ns, nd, ne, loops = case["ns"], case["nd"], case["ei"].shape[1], case["loops"]
    x, ps, pd = _pair_inputs(case)
    z = ops._pointnet_pair_fwd(g, x, ps, pd, loops)
    assert z.shape == case["z"].shape and np.array_equal(_np(z), case["z"]), (f, kind)
    assert not np.signbit(_np(z)[ne:, f:]).any()                 # the loops' position columns are +0
    assert torch.equal(z, ops._pointnet_pair_fwd(g, x, ps, pd, loops)) and torch.equal(z, ops.pointnet_pairs(g, x, ps, pd, loops))
    padded = ops._pointnet_pair_fwd(g, x, ps, pd, loops, pad=True)
    assert padded.stride(0) % 4 == 0 and torch.equal(padded, z) and torch.equal(ops.pointnet_pairs(g, x, ps, pd, loops, pad=True), z)
    base = padded._base if padded._base is not None else padded  # the padding columns are written too: zeros
    assert base.shape == (z.size(0), (f + 6) // 4 * 4) and (base[:, f + 3:] == 0).all()
    auto = ops.pointnet_pairs(g, x, ps, pd, loops)               # the default pads exactly where it buys 16-byte stores
    assert torch.equal(auto, z) and auto.is_contiguous() == (f == 0 or f % 4 != 0)
    views = [(x, _strided_pos(ps, 0), _strided_pos(pd, 1)), (x, _strided_pos(ps, 2), _strided_pos(pd, 2))]
    if x is not None:
        views += [(_wide(x), ps, pd), (_odd(x), _strided_pos(ps, 1), pd)]
    for xv, psv, pdv in views:
        assert torch.equal(z, ops._pointnet_pair_fwd(g, xv, psv, pdv, loops))
        assert torch.equal(z, ops.pointnet_pairs(g, xv, psv, pdv, loops))
    L, ei = _lib.lib(), g.edge_index
    for ld, off in ((f + 3 + 9, 4), (f + 3 + 4, 1)):             # rows 16-byte aligned (where F % 4 == 0), and not
        buf = torch.full((z.size(0), ld), 7.0, device=DEV)
        o_z = buf[:, off:off + f + 3]
        _lib.check(L.dc_pointnet_pair_fwd(ei[0].data_ptr(), ei[1].data_ptr(), None if x is None else x.data_ptr(), f,
                                          ps.data_ptr(), 3, pd.data_ptr(), 3, o_z.data_ptr(), ld, ns, nd, ne, f, int(loops), 0,
                                          _st()), "dc_pointnet_pair_fwd")
        assert torch.equal(o_z, z) and (buf[:, :off] == 7.0).all() and (buf[:, off + f + 3:] == 7.0).all()
        for zpad in (1, 3):                                      # zpad zero columns behind the row and nothing beside them
            buf.fill_(7.0)
            _lib.check(L.dc_pointnet_pair_fwd(ei[0].data_ptr(), ei[1].data_ptr(), None if x is None else x.data_ptr(), f,
                                              ps.data_ptr(), 3, pd.data_ptr(), 3, o_z.data_ptr(), ld, ns, nd, ne, f,
                                              int(loops), zpad, _st()), "dc_pointnet_pair_fwd")
            end = off + f + 3
            assert torch.equal(o_z, z) and (buf[:, end:end + zpad] == 0).all() and (buf[:, end + zpad:] == 7.0).all()
            assert (buf[:, :off] == 7.0).all()


@gpu
@pytest.mark.parametrize("kind", MAIN_KINDS)
@pytest.mark.parametrize("f", PAIR_WIDTHS)
def test_pair_backward_entry_and_node(f, kind):
    """g_x, g_pos_src, g_pos_dst within 1e-5 per row of the float64 sums of the same terms; g_z as a column slice, any
    subset of the outputs: the same bits; twice: the same bits; the ``ops`` node with a contiguous, a non-contiguous and
    an expanded gradient: the bits of a contiguous one; one ``pos`` tensor: the sum of the two position gradients"""
    case = pair_case(kind, f)
    g = _device_graph(kind)[0]
    ns, nd, loops = case["ns"], case["nd"], case["loops"]
    x, ps, pd = _pair_inputs(case)
    gz = _dev(case["gz"])
    gx, gps, gpd = ops._pointnet_pair_bwd(g, gz, ns, nd, loops)
    assert (gx is None) == (f == 0) and gps.shape == (ns, 3) and gpd.shape == (nd, 3)
    tag = f"pointnet pair F={f} {kind}"
    if f:
        assert gx.shape == (ns, f)
        _within_bar_of_float64(_np(gx), case["gx64"], tag + " g_x")
    _within_bar_of_float64(_np(gps), case["gps64"], tag + " g_pos_src")
    _within_bar_of_float64(_np(gpd), case["gpd64"], tag + " g_pos_dst")
    same = lambda a, b: all((s is None and t is None) or torch.equal(s, t) for s, t in zip(a, b))
    assert same((gx, gps, gpd), ops._pointnet_pair_bwd(g, gz, ns, nd, loops))
    assert same((gx, gps, gpd), ops._pointnet_pair_bwd(g, _wide(gz), ns, nd, loops))
    assert same((gx, gps, gpd), ops._pointnet_pair_bwd(g, _odd(gz), ns, nd, loops))
    # which form ran: the views above have row strides F + 3, F + 15, F + 6 - never a multiple of 4 where F is one - so
    # they are the scalar form at every width.  ``_quad`` has a row stride of F + 16 and 16-byte aligned rows: where
    # F % 4 == 0 it runs the 16-byte form, which must give the scalar form's bits (the same sums, column by column)
    for view, vec in ((gz, False), (_quad(gz), f > 0 and f % 4 == 0)):
        _lib.kernel_trace(True)
        got = ops._pointnet_pair_bwd(g, view, ns, nd, loops)
        names = _lib.kernel_trace_counts()
        _lib.kernel_trace(False)
        assert sum(names.values()) == 1 and any(("k_pointnet_pair_bwd<4" in k) == vec for k in names), (names, f)
        assert same((gx, gps, gpd), got), (f, kind, vec)
        if vec:
            _within_bar_of_float64(_np(got[0]), case["gx64"], tag + " g_x, 16-byte form")
            o_x = torch.full((ns, f + 8), 7.0, device=DEV)       # a strided g_x (rows stay 16-byte aligned): the same form
            _lib.kernel_trace(True)
            _lib.check(_lib.lib().dc_pointnet_pair_bwd(
                g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), g.fwd.perm.data_ptr(), g.bwd.ptr.data_ptr(),
                g.bwd.other.data_ptr(), g.bwd.perm.data_ptr(), view.data_ptr(), view.stride(0), o_x.data_ptr(), f + 8, None,
                3, None, 3, ns, nd, case["ei"].shape[1], f, int(loops), _st()), "dc_pointnet_pair_bwd")
            names = _lib.kernel_trace_counts()
            _lib.kernel_trace(False)
            assert any("k_pointnet_pair_bwd<4" in k for k in names), names
            assert torch.equal(o_x[:, :f], gx) and (o_x[:, f:] == 7.0).all()
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        part = ops._pointnet_pair_bwd(g, gz, ns, nd, loops, want)
        assert same(part, [t if w else None for t, w in zip((gx, gps, gpd), want)]), want
    # a node without edges (bip: source 36, destination 12) gets zero rows
    if kind == "bip":
        assert (gps[36] == 0).all() and (gpd[12] == 0).all() and (f == 0 or (gx[36] == 0).all())
    # through autograd
    leaf = lambda t: None if t is None else t.detach().requires_grad_(True)

    def run(grad, xin=x):
        xs, p1 = leaf(xin), leaf(ps)
        p2 = p1 if pd is ps else leaf(pd)
        torch.autograd.backward([ops.pointnet_pairs(g, xs, p1, p2, loops)], [grad])
        return (None if xs is None else xs.grad), p1.grad, (None if p2 is p1 else p2.grad)

    want = (gx, gps + gpd, None) if pd is ps else (gx, gps, gpd)
    assert same(run(gz), want)
    wide_g = torch.full((gz.size(0), 2 * (f + 3)), 1e30, device=DEV)
    wide_g[:, ::2] = gz
    for strided in (wide_g[:, ::2], _wide(gz), _odd(gz), _quad(gz)):
        assert not strided.is_contiguous() and same(run(strided), want)
    if x is not None:
        assert same(run(gz, _wide(x)), want) and same(run(gz, _odd(x)), want)
    ones = ops._pointnet_pair_bwd(g, torch.ones_like(gz), ns, nd, loops)
    xs, p1 = leaf(x), leaf(ps)
    p2 = p1 if pd is ps else leaf(pd)
    ops.pointnet_pairs(g, xs, p1, p2, loops).sum().backward()    # an expanded gradient of ones
    got = (None if xs is None else xs.grad), p1.grad, (None if p2 is p1 else p2.grad)
    assert same(got, (ones[0], ones[1] + ones[2], None) if pd is ps else ones)
    # only the inputs that want a gradient get one
    p1 = leaf(ps)
    torch.autograd.backward([ops.pointnet_pairs(g, x, p1, pd if pd is not ps else ps, loops)], [gz])
    assert torch.equal(p1.grad, gps)


@functools.lru_cache(maxsize=None)
def _sum_f32(kind, c):
    _, ptr, perm, _, _ = _device_graph(kind)
    nd = reduce_case(kind, c)["nd"]
    return sum_loop_f32(ptr[:nd + 1], perm, reduce_case(kind, c)["m"])


@gpu
@pytest.mark.parametrize("kind", MAIN_KINDS)
@pytest.mark.parametrize("c", REDUCE_WIDTHS)
def test_reduce_forward_entry(c, kind):
    """the Nd destination rows: sum bit-identical to the float32 loop over the device's own sorted set, mean that sum
    divided by ``np.float32(deg)`` (the loop counts), max: y and cnt equal element for element on the coarse grid; m as a
    column slice: the same bits; ``ops.pointnet_aggregate``: the same bits"""
    case = reduce_case(kind, c)
    g = _device_graph(kind)[0]
    nd, deg, loops = case["nd"], case["deg"], case["loops"]
    s32 = _sum_f32(kind, c)
    m, mg = _dev(case["m"]), _dev(case["mg"])
    y, none = ops._edge_reduce_fwd(g, m, 0, nd)
    assert none is None and y.shape == (nd, c) and np.array_equal(_np(y), s32), (c, kind)
    assert rel_err(_np(y), case["sum64"]) < TOL
    mean, _ = ops._edge_reduce_fwd(g, m, 1, nd)
    want = np.where(deg[:, None] > 0, s32 / np.maximum(deg, 1).astype(np.float32)[:, None], np.float32(0))
    assert want.dtype == np.float32 and np.array_equal(_np(mean), want), (c, kind)
    mx, cnt = ops._edge_reduce_fwd(g, mg, 2, nd)
    assert cnt.dtype == torch.int32 and cnt.shape == (nd, c)
    assert np.array_equal(_np(mx), case["y"]) and np.array_equal(_np(cnt), case["cnt"]), (c, kind)
    assert (mx[_dev(deg == 0)] == 0).all() and (cnt[_dev(deg == 0)] == 0).all() and (y[_dev(deg == 0)] == 0).all()
    for mode, src, want_y in ((0, m, y), (1, m, mean), (2, mg, mx)):
        name = ("sum", "mean", "max")[mode]
        for view in (src, _wide(src), _odd(src)):
            assert torch.equal(want_y, ops.pointnet_aggregate(g, view, name, nd, loops)), (mode, c, kind)
        assert torch.equal(want_y, ops.pointnet_aggregate(g, src, name, nd, loops))          # twice: the same bits


@gpu
@pytest.mark.parametrize("kind", MAIN_KINDS)
@pytest.mark.parametrize("c", REDUCE_WIDTHS)
def test_reduce_backward_entry_and_node(c, kind):
    """sum, mean and max bit-identical to the numpy float32 formula, a removed input loop a zero row; operands as
    column slices, a strided output: the same bits; through autograd with a contiguous, a non-contiguous and an
    expanded gradient: the same bits"""
    case = reduce_case(kind, c)
    g = _device_graph(kind)[0]
    nd, ne, loops = case["nd"], case["ei"].shape[1], case["loops"]
    m, mg, gy = _dev(case["m"]), _dev(case["mg"]), _dev(case["gy"])
    y, cnt = _dev(case["y"]), _dev(case["cnt"])
    L, ld, ei = _lib.lib(), c + 8, g.edge_index
    for name, mode in MODES.items():
        src = mg if mode == 2 else m
        sv = (src, y, cnt) if mode == 2 else (None, None, None)
        gm = ops._pointnet_reduce_bwd(g, *sv, gy, mode, loops)
        assert gm.shape == case["gm"][name].shape and np.array_equal(_np(gm), case["gm"][name]), (name, c, kind)
        assert torch.equal(gm, ops._pointnet_reduce_bwd(g, *sv, gy, mode, loops))
        assert torch.equal(gm, ops._pointnet_reduce_bwd(g, *sv, _wide(gy), mode, loops))
        assert torch.equal(gm, ops._pointnet_reduce_bwd(g, *sv, _odd(gy), mode, loops))
        if mode == 2:
            assert torch.equal(gm, ops._pointnet_reduce_bwd(g, _wide(src), _wide(y), _wide(cnt), gy, mode, loops))
            assert torch.equal(gm, ops._pointnet_reduce_bwd(g, _odd(src), y, _odd(cnt), _odd(gy), mode, loops))
        o_g = torch.full((gm.size(0), ld), 7.0, device=DEV)
        ptrs = [t.data_ptr() for t in sv] if mode == 2 else [None, None, None]
        _lib.check(L.dc_pointnet_reduce_bwd(ei[0].data_ptr(), ei[1].data_ptr(), g.fwd.ptr.data_ptr(), ptrs[0], c, ptrs[1],
                                            c, ptrs[2], c, gy.data_ptr(), c, o_g.data_ptr(), ld, mode, g.num_nodes, nd, ne,
                                            c, int(loops), _st()), "dc_pointnet_reduce_bwd")
        assert torch.equal(o_g[:, :c], gm) and (o_g[:, c:] == 7.0).all()
        # through autograd
        ms = _wide(src).detach().requires_grad_(True)
        wide_g = torch.full((nd, 2 * c), 1e30, device=DEV)
        wide_g[:, ::2] = gy
        for grad in (gy, wide_g[:, ::2], _wide(gy), _odd(gy)):
            ms.grad = None
            torch.autograd.backward([ops.pointnet_aggregate(g, ms, name, nd, loops)], [grad])
            assert torch.equal(ms.grad, gm), (name, c, kind)
        ms.grad = None
        ops.pointnet_aggregate(g, ms, name, nd, loops).sum().backward()      # an expanded gradient of ones
        out = ops.pointnet_aggregate(g, src, name, nd, loops)
        assert torch.equal(ms.grad, ops._pointnet_reduce_bwd(g, *((src, out, cnt) if mode == 2 else sv),
                                                             torch.ones_like(gy), mode, loops))


@gpu
def test_edges_with_an_endpoint_out_of_range_get_a_zero_row():
    """an edge list that names a source outside [0, Ns) - a source in [Ns, max(Ns, Nd)) included, which only the
    bipartite check catches - or a destination outside [0, Nd): those rows are zeros in the pair forward and in the
    reduce backward, and add nothing in the pair backward; the others are not touched by it"""
    ns, nd, f, ne = 9, 14, 12, 64
    rng = np.random.default_rng(2)
    ei = np.stack([rng.integers(0, ns, ne), rng.integers(0, nd, ne)])
    bad = np.zeros(ne, bool)
    ei[0, 3], ei[0, 5], ei[1, 7], ei[0, 11], ei[1, 12], bad[[3, 5, 7, 11, 12]] = ns, nd - 1, nd + 5, -1, -3, True
    x, ps, pd = (rng.standard_normal(s).astype(np.float32) for s in ((ns, f), (ns, 3), (nd, 3)))
    gy = rng.standard_normal((nd, f)).astype(np.float32)
    gz = rng.standard_normal((ne, f + 3)).astype(np.float32)
    tei = torch.from_numpy(ei).to(DEV)
    src, dst = np.where(bad, 0, ei[0]), np.where(bad, 0, ei[1])
    L = _lib.lib()
    z = torch.full((ne, f + 3), 7.0, device=DEV)
    tx, tps, tpd = _dev(x), _dev(ps), _dev(pd)
    _lib.check(L.dc_pointnet_pair_fwd(tei[0].data_ptr(), tei[1].data_ptr(), tx.data_ptr(), f, tps.data_ptr(), 3,
                                      tpd.data_ptr(), 3, z.data_ptr(), f + 3, ns, nd, ne, f, 0, 0, _st()),
               "dc_pointnet_pair_fwd")
    want = np.where(bad[:, None], np.float32(0), np.concatenate([x[src], ps[src] - pd[dst]], axis=1))
    assert np.array_equal(_np(z), want)
    # the sorted sets of max(Ns, Nd) rows hold the edges 3 and 5 (sources in [Ns, Nd)): the pair backward leaves them out
    g = GraphIndex(tei, max(ns, nd), self_loops=False, normalize=False)
    gx, gps, gpd = ops._pointnet_pair_bwd(g, _dev(gz), ns, nd, False)
    ok = ~bad
    _within_bar_of_float64(_np(gx), _index_add(ns, src[ok], gz[ok][:, :f]), "out of range g_x")
    _within_bar_of_float64(_np(gps), _index_add(ns, src[ok], gz[ok][:, f:]), "out of range g_pos_src")
    _within_bar_of_float64(_np(gpd), -_index_add(nd, dst[ok], gz[ok][:, f:]), "out of range g_pos_dst")
    # the reduce backward: rows 7, 11, 12 (not in the sorted set) are zeros; 3 and 5 are in it and the forward reduced them
    in_set = ~bad | np.isin(np.arange(ne), [3, 5])
    deg = np.maximum(np.bincount(ei[1][in_set], minlength=nd), 1).astype(np.float32)
    assert np.array_equal(_np(g.fwd.ptr).astype(np.int64)[1:nd + 1] - _np(g.fwd.ptr).astype(np.int64)[:nd],
                          np.bincount(ei[1][in_set], minlength=nd))
    d = np.where(in_set, ei[1], 0)
    for mode, want in ((0, gy[d]), (1, gy[d] / deg[d][:, None])):
        gm = ops._pointnet_reduce_bwd(g, None, None, None, _dev(gy), mode, False)
        assert np.array_equal(_np(gm), np.where(in_set[:, None], want, np.float32(0))), mode


@gpu
def test_ops_with_no_rows_and_their_checks():
    """E = 0, Nd = 0, Ns = 0: zero or empty results without a launch, gradients of the right shape; the host checks"""
    L = _lib.lib()
    assert L.dc_pointnet_pair_fwd(None, None, None, 15, None, 3, None, 3, None, 18, 0, 0, 0, 15, 0, 0, None) == 0
    assert L.dc_pointnet_reduce_bwd(None, None, None, None, 15, None, 15, None, 15, None, 15, None, 15, 2, 0, 0, 0, 15, 0,
                                    None) == 0
    _lib.kernel_trace(True)
    for kind in EDGE_KINDS:
        ns, nd, ei, loops = _graph(kind)
        tei = torch.from_numpy(ei).to(DEV)
        g = ops.pointnet_graph(tei, ns, nd) if max(ns, nd) else None
        x = torch.randn(ns, 7, device=DEV, requires_grad=True)
        ps, pd = torch.randn(ns, 3, device=DEV, requires_grad=True), torch.randn(nd, 3, device=DEV, requires_grad=True)
        z = ops.pointnet_pairs(g, x, ps, pd)
        assert z.shape == (0, 10) and z.requires_grad
        z.sum().backward()
        assert x.grad.shape == (ns, 7) and ps.grad.shape == (ns, 3) and pd.grad.shape == (nd, 3)
        assert (x.grad == 0).all() and (ps.grad == 0).all() and (pd.grad == 0).all()
        for reduce in AGGRS:
            m = torch.zeros((0, 5), device=DEV, requires_grad=True)
            y = ops.pointnet_aggregate(g, m, reduce, nd)
            assert y.shape == (nd, 5) and (y == 0).all()
            y.sum().backward()
            assert m.grad.shape == (0, 5)
    counts = _lib.kernel_trace_counts()
    _lib.kernel_trace(False)
    assert not any("k_pointnet" in k or "k_edge" in k for k in counts), counts
    # edges, but no source or no destination: every edge names a node that is not there - zero rows, no launch
    tei = torch.tensor([[0, 1], [0, 0]], device=DEV)
    g = ops.pointnet_graph(tei, 0, 3)
    z = ops.pointnet_pairs(g, None, torch.zeros(0, 3, device=DEV), torch.zeros(3, 3, device=DEV))
    assert z.shape == (2, 3) and (z == 0).all()
    n, f = 12, 6
    tei = torch.from_numpy(random_multigraph(n, 40, 1)).to(DEV)
    g, gl = ops.pointnet_graph(tei, n, n), ops.pointnet_graph(tei, n, n, True)
    x, pos = torch.randn(n, f, device=DEV), torch.randn(n, 3, device=DEV)
    with pytest.raises(ValueError, match="self_loops=True"):
        ops.pointnet_pairs(g, x, pos, pos, loops=True)
    with pytest.raises(ValueError, match="self_loops=False"):
        ops.pointnet_pairs(gl, x, pos, pos)
    with pytest.raises(ValueError, match="self_loops=False"):
        ops.pointnet_aggregate(gl, torch.zeros(40, f, device=DEV))
    with pytest.raises(ValueError, match="40 rows.*52"):
        ops.pointnet_aggregate(gl, torch.zeros(40, f, device=DEV), loops=True)
    with pytest.raises(ValueError, match="num_dst"):
        ops.pointnet_aggregate(g, torch.zeros(40, f, device=DEV), num_dst=13)
    with pytest.raises(ValueError, match="num_dst"):
        ops.pointnet_aggregate(gl, torch.zeros(52, f, device=DEV), num_dst=5, loops=True)
    with pytest.raises(ValueError, match="rows"):
        ops.pointnet_pairs(g, x[:5], pos, pos)
    with pytest.raises(ValueError, match="max"):
        ops.pointnet_pairs(g, None, pos[:5], pos[:7])
    with pytest.raises(ValueError, match="None"):
        ops.pointnet_pairs(None, x, pos, pos)
    for bad in (x.double(), x[0], torch.zeros((n, 0), device=DEV)):
        with pytest.raises(ValueError):
            ops.pointnet_pairs(g, bad, pos, pos)
        with pytest.raises(ValueError):
            ops.pointnet_aggregate(g, bad)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.pointnet_pairs(g, x.cpu(), pos, pos)


# --------------------------------------------------------------------------- #
# GPU: the layer
# --------------------------------------------------------------------------- #
def _device_conv(case, plain=False):
    """the layer with the reference's parameters (every Linear a ``Linear64`` unless ``plain``)"""
    cpu = case["cpu"]
    return dc.nn.PointNetConv(_device_nn(cpu.local_nn, plain), None if cpu.global_nn is None else _device_nn(cpu.global_nn, plain),
                              add_self_loops=case["loops"], aggr=case["aggr"]).to(DEV)


def _device_run(conv, case, form="auto"):
    for p in conv.parameters():
        p.grad = None
    leaf = lambda a: None if a is None else _dev(a).requires_grad_(True)
    x, ps = leaf(case["x"]), leaf(case["ps"])
    pd = ps if case["one_pos"] else leaf(case["pd"])
    tei = torch.from_numpy(case["ei"]).to(DEV)
    if case["one_pos"]:
        out = conv(x, ps, tei) if form == "auto" else conv((x, x), (ps, ps), tei)
    else:
        xd = None if form == "auto" or x is None else torch.zeros(case["nd"], x.size(1), device=DEV)
        out = conv(None if x is None else (x, xd), (ps, pd), tei)
    assert type(out) is torch.Tensor                             # the reduction's or global_nn's result: nothing deferred
    torch.autograd.backward([out], [_dev(case["gup"])])
    torch.cuda.synchronize()
    grads = {"pos_src": ps.grad}
    if x is not None:
        grads["x"] = x.grad
    if not case["one_pos"]:
        grads["pos_dst"] = pd.grad
    grads.update({name: p.grad for name, p in conv.named_parameters()})
    zero = lambda k, v: v if v is not None else torch.zeros_like({"pos_src": ps, "x": x, "pos_dst": pd}[k])
    return out.detach(), {k: zero(k, v) for k, v in grads.items()}


def _host(run):
    return _np(run[0]), {k: _np(v) for k, v in run[1].items()}


def _check_layer(fi, fo, aggr, seq, kind, plain=False, form="auto"):
    case = layer_case(fi, fo, aggr, seq, kind)
    clear_cache()
    conv = _device_conv(case, plain)
    tag = f"PointNetConv {fi}->{fo} {aggr} seq={seq} {kind}"
    if case["exact"] and case["ei"].shape[1]:
        # the precondition of one selection in every evaluation: the messages are the same numbers on the device
        t64 = lambda a: None if a is None else torch.from_numpy(a).double()
        with torch.no_grad():
            tei = torch.from_numpy(case["ei"]).to(DEV)
            g = ops.pointnet_graph(tei, case["ns"], case["nd"], case["loops"])
            ps = _dev(case["ps"])
            z = ops.pointnet_pairs(g, None if case["x"] is None else _dev(case["x"]), ps,
                                   ps if case["one_pos"] else _dev(case["pd"]), case["loops"])
            got_m = conv.local_nn(z)
            want, _ = copy.deepcopy(case["cpu"]).double().messages(t64(case["x"]), t64(case["ps"]), t64(case["pd"]),
                                                                   torch.from_numpy(case["ei"]))
        rows = edge_rows(kind)[0]
        assert torch.equal(got_m.cpu().double()[torch.from_numpy(rows)], want), f"{tag}: the messages are not exact"
    got = _host(_device_run(conv, case, form))
    assert got[0].shape == case["r32"][0].shape
    check_against_references(tag, got, case, "e_h")
    return case, got


@gpu
@pytest.mark.parametrize("kind", MAIN_KINDS)
@pytest.mark.parametrize("seq", [False, True], ids=["linear", "mlp"])
@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("fi,fo", SHAPES)
def test_layer_parity(fi, fo, aggr, seq, kind):
    """forward and the gradients of x, of the positions (source and destination) and of every parameter of local_nn and
    global_nn against RefPointNetConv at 1e-5: every shape x aggr x local_nn x graph; global_nn present in half of the
    cases; ``bip`` is called with pairs ``(x_src, None)`` / ``(pos_src, pos_dst)``, F = 0 with ``x = None``, ``sql``
    with ``add_self_loops=True``"""
    _check_layer(fi, fo, aggr, seq, kind)


@gpu
@pytest.mark.parametrize("kind", ["bip", "sq"])
def test_pair_forms_read_x_src_alone(kind):
    """``(x_src, x_dst)`` with a tensor ``x_dst`` (``bip``) and pairs of one tensor (``sq``): ``x_dst`` is not read"""
    _check_layer(3, 64, "max", True, kind, form="pairs")
    _check_layer(64, 20, "mean", False, kind, form="pairs")


@gpu
@pytest.mark.parametrize("kind", MAIN_KINDS)
@pytest.mark.parametrize("seq", [False, True], ids=["linear", "mlp"])
@pytest.mark.parametrize("aggr", AGGRS)
def test_layer_parity_with_plain_torch_modules(aggr, seq, kind):
    """``local_nn`` / ``global_nn`` built from ``torch.nn.Linear`` as it is (no graph here has a hub): the same bar"""
    _check_layer(64, 20, aggr, seq, kind, plain=True)
    _check_layer(3, 64, aggr, seq, kind, plain=True)


@gpu
@pytest.mark.parametrize("kind", EDGE_KINDS)
@pytest.mark.parametrize("aggr", AGGRS)
def test_layer_on_edge_graphs(aggr, kind):
    """no edge, no destination, no source, no node: the output has Nd rows of the module's width; the backward runs"""
    for fi, fo in ((3, 64), (0, 20)):
        for seq in (False, True):
            case, (out, grads) = _check_layer(fi, fo, aggr, seq, kind)
            assert out.shape[0] == case["nd"]
            assert all((grads[k] == 0).all() for k in grads if k in ("x", "pos_src", "pos_dst"))
            if not case["glob"]:
                assert (out == 0).all()
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("kind", MAIN_KINDS)
@pytest.mark.parametrize("aggr", AGGRS)
def test_gradient_layouts_and_a_repeat_give_the_same_bits(aggr, kind):
    """``out.sum().backward()`` sends an expanded gradient, a column slice a strided one: the bits of every gradient
    are those of a contiguous gradient of the same values; x as a column slice and positions with a row stride: the
    same bits; forward + backward twice: identical bits"""
    ns, nd, ei, loops = _graph(kind)
    fi, fo = 20, 23                                              # (the module keeps the position columns)
    rng = np.random.default_rng(11)
    grid = aggr == "max"
    x = _dev(coarse_grid(rng, (ns, fi)) if grid else rng.standard_normal((ns, fi)).astype(np.float32))
    ps = _dev(_positions(rng, ns, grid))
    pd = ps if kind != "bip" else _dev(_positions(rng, nd, grid))
    w = _dev(rng.uniform(0.5, 1.5, (nd, fo)).astype(np.float32))
    tei = torch.from_numpy(ei).to(DEV)
    clear_cache()
    conv = dc.nn.PointNetConv(Mix(fi + 3, fo), None, add_self_loops=loops, aggr=aggr).to(DEV)

    def run(loss, xin=x, p1=ps, p2=pd):
        conv.local_nn.scale.grad = None
        xg, a = xin.detach().requires_grad_(True), p1.detach().requires_grad_(True)
        b = a if pd is ps else p2.detach().requires_grad_(True)
        out = conv(xg, a, tei) if pd is ps else conv((xg, None), (a, b), tei)
        loss(out)
        torch.cuda.synchronize()
        return [out.detach().clone(), xg.grad.clone(), a.grad.clone(), b.grad.clone(), conv.local_nn.scale.grad.clone()]

    def same(a, b):
        assert all(torch.equal(s, t) for s, t in zip(a, b))

    ones = run(lambda out: torch.autograd.backward([out], [torch.ones_like(out)]))
    same(run(lambda out: out.sum().backward()), ones)            # expanded (stride 0)
    assert ones[1].abs().max() > 0 and ones[2].abs().max() > 0
    dense = run(lambda out: torch.autograd.backward([out], [w]))
    same(run(lambda out: torch.autograd.backward([out], [w])), dense)          # a repeat: identical bits
    padded = torch.zeros((nd, fo + 8), device=DEV)
    padded[:, 4:4 + fo] = w
    wide_w = torch.full((nd, 2 * fo), 1e30, device=DEV)
    wide_w[:, ::2] = w
    same(run(lambda out: torch.autograd.backward([out], [padded[:, 4:4 + fo]])), dense)     # a column slice
    same(run(lambda out: torch.autograd.backward([out], [wide_w[:, ::2]])), dense)          # inner stride 2
    same(run(lambda out: torch.autograd.backward([out], [w]), _wide(x), _strided_pos(ps, 1), _strided_pos(pd, 2)), dense)
    same(run(lambda out: torch.autograd.backward([out], [w]), _odd(x), _strided_pos(ps, 0), _strided_pos(pd, 0)), dense)


@gpu
@pytest.mark.parametrize("kind", ["bip", "sql"])
def test_launches_of_one_layer_step(kind):
    """forward + backward of PointNetConv and global_max_pool behind it: one kernel per entry - pair forward, the max of
    dc_edge.hip, the pool, and their three backwards - and nothing else of the library"""
    case = layer_case(3, 64, "max", False, kind)
    clear_cache()
    conv = _device_conv(case)
    leaf = lambda a: _dev(a).requires_grad_(True)
    x, ps, tei = leaf(case["x"]), leaf(case["ps"]), torch.from_numpy(case["ei"]).to(DEV)
    pd = ps if case["one_pos"] else leaf(case["pd"])
    ops.pointnet_graph(tei, case["ns"], case["nd"], case["loops"])           # built (and cached) before the log starts
    batch = torch.zeros(case["nd"], dtype=torch.int64, device=DEV)
    _lib.kernel_trace(True)
    out = conv(x, ps, tei) if case["one_pos"] else conv((x, None), (ps, pd), tei)
    dc.pointops.global_max_pool(out, batch, 1).sum().backward()
    counts = _lib.kernel_trace_counts()
    _lib.kernel_trace(False)
    want = ("k_pointnet_pair_fwd", "k_edge_max_fwd", "k_pool_fwd", "k_pool_bwd", "k_pointnet_reduce_bwd", "k_pointnet_pair_bwd")
    assert sum(counts.values()) == 6 and all(any(k + "<" in name for name in counts) for k in want), counts


@gpu
def test_capture_of_layer_and_pool_forward_and_backward():
    """PointNetConv (bipartite, then with loops) + global_max_pool, forward + backward, recorded in ``torch.cuda.graph``:
    the replays give the bits of the eager runs on new inputs"""
    ns, nd, ei, _ = _graph("bip")
    n2, _, ei2, _ = _graph("sql")
    assert n2 >= nd
    rng = np.random.default_rng(8)
    tei, tei2 = torch.from_numpy(ei).to(DEV), torch.from_numpy(ei2[:, (ei2 < nd).all(0)]).to(DEV)
    conv1 = dc.nn.PointNetConv(Mix(9, 9), None, add_self_loops=False, aggr="max").to(DEV)
    conv2 = dc.nn.PointNetConv(Mix(12, 12), None, add_self_loops=True, aggr="mean").to(DEV)
    batch = torch.from_numpy(np.sort(rng.integers(0, 3, nd))).to(DEV)
    ins = [[_dev(coarse_grid(rng, s)) for s in ((ns, 6), (ns, 3), (nd, 3))] for _ in range(3)]
    leaves = [t.clone().requires_grad_(True) for t in ins[0]] + [conv1.local_nn.scale, conv2.local_nn.scale]
    for t in leaves:
        t.grad = torch.zeros_like(t)
    x, ps, pd = leaves[:3]

    def step():
        for t in leaves:
            t.grad.zero_()
        h = conv1((x, None), (ps, pd), tei)
        h = conv2(h, pd, tei2)
        out = dc.pointops.global_max_pool(h, batch, 3)
        torch.autograd.backward([out], [torch.ones_like(out)])
        return out

    def snapshot(out):
        return [out.detach().clone()] + [t.grad.clone() for t in leaves]

    eager = []
    for vals in ins:
        with torch.no_grad():
            for t, v in zip(leaves[:3], vals):
                t.copy_(v)
        clear_cache()
        eager.append(snapshot(step()))
    assert eager[0][1].abs().max() > 0 and eager[0][3].abs().max() > 0
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
            for t, v in zip(leaves[:3], ins[i]):
                t.copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(snapshot(out), eager[i]):
            assert torch.equal(got, want), i


@gpu
def test_a_deferred_x_is_resolved_and_local_nn_sees_the_rows_in_input_order():
    n, _, ei, _ = _graph("sql")
    tei = torch.from_numpy(ei).to(DEV)
    torch.manual_seed(7)
    pre = dc.nn.GCNConv(8, 16).to(DEV)
    seen = []

    class Spy(nn.Module):
        def forward(self, z):
            seen.append(z)
            return z[:, :5] + z[:, 14:19]

    conv = dc.nn.PointNetConv(Spy(), aggr="sum").to(DEV)
    x, pos = torch.randn(n, 8, device=DEV), torch.randn(n, 3, device=DEV)
    with torch.no_grad():
        h = pre(x, tei)
        assert type(h).__name__ == "DeferredActivation"
        value = ops.resolve(h)
        a, b = conv(h, pos, tei), conv(value, pos, tei)
    assert type(a) is torch.Tensor and torch.equal(a, b) and len(seen) == 2
    want = torch.cat([torch.cat([value[tei[0]], pos[tei[0]] - pos[tei[1]]], dim=1),
                      torch.cat([value, torch.zeros(n, 3, device=DEV)], dim=1)])
    assert seen[0].shape == (ei.shape[1] + n, 19) and torch.equal(seen[0], want)
    for bad in (lambda z: z.double(), lambda z: z[:-1], lambda z: z[:, :0], lambda z: z.sum(1)):
        with pytest.raises(ValueError, match="local_nn must return"):
            dc.nn.PointNetConv(_Fn(bad), aggr="sum")(value, pos, tei)


class _Fn(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, z):
        return self.fn(z)


# --------------------------------------------------------------------------- #
# one small PointNet++ through the torch_geometric alias
# --------------------------------------------------------------------------- #
def _mlp(widths):
    layers = []
    for a, b in zip(widths[:-1], widths[1:]):
        layers += [nn.Linear(a, b), nn.Tanh()]
    return nn.Sequential(*layers[:-1])                           # a plain last layer, as PyG's MLP


class PointNet2(nn.Module):
    """PyG's pointnet2_segmentation example in small: two SAModules, a GlobalSAModule, two FPModules.  ``api`` supplies
    fps / radius / the conv call / global_max_pool / knn_interpolate - the aliased package on the device, the float
    restatement on the CPU (which replays the device's sample indices and edge lists: they are discrete)."""

    def __init__(self):
        super().__init__()
        self.sa1, self.sa2 = _mlp([3 + 3, 16, 24]), _mlp([24 + 3, 24, 32])
        self.sa3 = _mlp([32 + 3, 32, 40])
        self.fp3, self.fp2 = _mlp([40 + 32, 32]), _mlp([32 + 24, 24, 5])

    def sa(self, api, local_nn, ratio, r, x, pos, batch):
        idx = api.fps(pos, batch, ratio)
        row, col = api.radius(pos, pos[idx], r, batch, batch[idx])
        edge_index = torch.stack([col, row], dim=0)
        x = api.conv(local_nn, (x, x[idx]), (pos, pos[idx]), edge_index)
        return x, pos[idx], batch[idx]

    def fp(self, api, inner, k, x, pos, batch, x_skip, pos_skip, batch_skip):
        x = api.knn_interpolate(x, pos, pos_skip, batch, batch_skip, k)
        return inner(torch.cat([x, x_skip], dim=1)), pos_skip, batch_skip

    def forward(self, api, x, pos, batch, nb):
        l0 = (x, pos, batch)
        l1 = self.sa(api, self.sa1, 0.5, 0.6, *l0)
        l2 = self.sa(api, self.sa2, 0.5, 1.0, *l1)
        h = api.global_max_pool(self.sa3(torch.cat([l2[0], l2[1]], dim=1)), l2[2], nb)
        l3 = (h, pos.new_zeros((nb, 3)), torch.arange(nb, device=batch.device))
        f3 = self.fp(api, self.fp3, 1, *l3, *l2)
        return self.fp(api, self.fp2, 3, *f3, *l1)[0]


class _DeviceApi:
    def __init__(self):
        from torch_geometric.nn import PointNetConv as Conv, fps, global_max_pool, knn_interpolate, radius
        self.Conv, self._fps, self._radius = Conv, fps, radius
        self.global_max_pool, self.knn_interpolate = global_max_pool, knn_interpolate
        self.tape = []

    def fps(self, pos, batch, ratio):
        idx = self._fps(pos, batch, ratio=ratio)
        self.tape.append(idx.cpu())
        return idx

    def radius(self, x, y, r, bx, by):
        pair = self._radius(x, y, r, bx, by, max_num_neighbors=64)
        self.tape.append(pair.cpu())
        return pair

    def conv(self, local_nn, x, pos, edge_index):
        return self.Conv(local_nn, None, add_self_loops=False)(x, pos, edge_index)


class _RefApi:
    def __init__(self, tape):
        self.tape = list(tape)

    def fps(self, pos, batch, ratio):
        return self.tape.pop(0)

    def radius(self, x, y, r, bx, by):
        return self.tape.pop(0)

    def conv(self, local_nn, x, pos, edge_index):
        return RefPointNetConv(local_nn, None, False, "max")(x[0], pos[0], pos[1], edge_index)

    def global_max_pool(self, x, batch, nb):
        return ref_segment(x, batch, nb, "max")

    def knn_interpolate(self, x, pos_x, pos_y, bx, by, k):
        with torch.no_grad():
            d2 = ((pos_y[:, None, :] - pos_x[None, :, :]) ** 2).sum(-1)
            d2 = torch.where(by[:, None] == bx[None, :], d2, torch.full_like(d2, float("inf")))
            val, nbr = torch.topk(d2, k, dim=1, largest=False)
            assert torch.isfinite(val).all()
            w = 1.0 / val.clamp(min=1e-16)
        return (x[nbr] * w[:, :, None]).sum(1) / w.sum(1, keepdim=True)


@gpu
def test_a_small_pointnet2_through_the_alias():
    """2 clouds of 96 points, fps -> radius -> PointNetConv((x, x[idx]), (pos, pos[idx]), edge_index) twice ->
    global_max_pool -> knn_interpolate twice, imported from ``torch_geometric.nn``: the output and the gradients of x,
    pos and every parameter against the same model on the CPU restatement (float32, float64) at 1e-5"""
    torch.set_num_threads(1)
    rng = np.random.default_rng(21)
    n, nb = 192, 2
    pos = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    x = rng.standard_normal((n, 3)).astype(np.float32)
    batch = np.repeat(np.arange(nb), n // nb)
    torch.manual_seed(3)
    cpu = PointNet2()
    mods = ("torch_geometric", "torch_geometric.nn", "torch_geometric.data")
    saved = {k: sys.modules.get(k) for k in mods}
    try:
        dc.install_as_torch_geometric(force=True)
        api = _DeviceApi()
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    clear_cache()
    dev = copy.deepcopy(cpu).to(DEV)
    xd, pd = _dev(x).requires_grad_(True), _dev(pos).requires_grad_(True)
    out = dev(api, xd, pd, torch.from_numpy(batch).to(DEV), nb)
    gup = rng.uniform(0.5, 1.5, tuple(out.shape)).astype(np.float32)
    torch.autograd.backward([out], [_dev(gup)])
    torch.cuda.synchronize()
    assert out.shape == (n // 2, 5) and len(api.tape) == 4
    got = {"forward": _np(out), "x.grad": _np(xd.grad), "pos.grad": _np(pd.grad)}
    got.update({k + ".grad": _np(p.grad) for k, p in dev.named_parameters()})
    refs = []
    for dtype in (torch.float32, torch.float64):
        mod = copy.deepcopy(cpu).to(dtype)
        xc, pc = (torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (x, pos))
        o = mod(_RefApi(api.tape), xc, pc, torch.from_numpy(batch), nb)
        (o * torch.from_numpy(gup).to(dtype)).sum().backward()
        ref = {"forward": o.detach().numpy(), "x.grad": xc.grad.numpy(), "pos.grad": pc.grad.numpy()}
        ref.update({k + ".grad": p.grad.numpy() for k, p in mod.named_parameters()})
        refs.append(ref)
    assert set(got) == set(refs[0])
    for k in got:
        assert_parity(got[k], refs[0][k], refs[1][k], TOL, f"PointNet2 {k}")
