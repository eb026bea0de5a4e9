"""``GATv2Conv``: the layer, its autograd Function and the C entries of dc_gatv2.hip.

The reference is this file's own restatement of the contract in INTEGRATION.md 1.3 (PyG 2.5.2 gatv2_conv.py): ``RefGATv2``,
a torch CPU module evaluated in float32 (``ref32``) and float64 (``truth64``) with gradients from torch autograd, and a
numpy restatement of the per-edge formulas (dtype-parametrised) for the entries called directly.

CPU: constructor / state_dict contract, argument checks of every new C entry, the restatements against each other
(float32 within the bar of float64 on every input the GPU tests use - the distance goes to ``record_parity`` - and the
hand-written backward formulas against torch autograd in float64).

GPU: the layer at 1e-5 (``helpers.assert_parity``: within 1e-5 of the float32 restatement or of float64; nothing wider,
nothing registered ``special``), the entries per edge / row under the per-segment metric of
``tests/test_gat_edge_kernels.py``, the bit-for-bit properties, capture.

Inputs that come from conditioning, not from what the kernels give: default-initialised parameters and x ~ N(0, 1) for
the layer, with x and the parameters of the two linears rounded to 8 significant bits (``_dyadic``): the gradient of
GATv2 is DISCONTINUOUS in s = lin_l(x_j) + lin_r(x_i) at s = 0 (leaky_relu'), a layer case has up to 6 million such s, and
with unrounded inputs a few of them lie within float32 rounding of 0 - two correct evaluations then take different
branches and differ by 1e-3 in the gradients of lin_r (seen on the CPU: float32 against float64 torch, one branch of
288,768).  With 8-bit operands every product and every partial sum of the linears is exact in float32 and in float64, in
any order, so s is the same number in every evaluation (asserted on the CPU) and no branch can differ.  The cases of
``UNROUNDED`` keep the inputs as they come and compare what is continuous in s (the output, bias.grad; with
negative_slope = 1, where there is no branch, every gradient): they are the ones that see the linears round.  For the direct
tests s is one float32 addition of given operands, whose sign is that of the exact sum; there xl, xr ~ 0.5 N(0, 1) and att ~ U(+-1.5 / sqrt(C)), so a segment's logits spread over a few
units, and the upstream ``galpha`` of ``test_gat_edge_kernels.galpha_for`` (alternating sign, magnitude in [1, 2)): the
difference ``galpha - dot`` in ``ge`` then does not cancel.  The long sums of the float32 numpy restatement are numpy's
pairwise ones, as in ``test_gat_edge_kernels._seg_sum``.
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
from oracle import pyg_ref
from tests.helpers import assert_parity, load_golden, random_multigraph, record_parity, rel_err, row_rel_err
from tests.test_gat_edge_kernels import (HUB, _dev, _np, _seg_sum, device_graph, galpha_for, host_adjacency,
                                         run_softmax_fwd, seg_graph, seg_lens, seg_of, seg_rel_err_on)

gpu = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5

#: (in, H, C, concat) of the layer tests
SHAPES = [(21, 1, 64, True), (25, 2, 256, True), (64, 3, 20, True), (32, 5, 3, True), (16, 4, 1, True),
          (64, 3, 20, False), (32, 1, 64, False)]
GRAPHS = ["multigraph", "hub", "n1", "e0", "golden_rest", "golden_rig"]
#: layer options beside the default (share_weights=False, bias=True, relu=False, negative_slope=0.2)
VARIANTS = {"default": {}, "shared": dict(share_weights=True), "nobias": dict(bias=False), "relu": dict(relu=True),
            "slope0": dict(negative_slope=0.0), "shared_relu_nobias": dict(share_weights=True, relu=True, bias=False)}
#: cases on UNROUNDED inputs (module docstring) -> the tensors compared: what is continuous in s.  They see the rounding of
#: the two linears (24-bit products, bias in the epilogue), which the 8-bit operands of every other case make exact
#: (with slope 1 the xr term of the logit is the same for every edge of a segment and drops out of the softmax: the
#: gradients of lin_r are mathematically zero, so they are not among the tensors compared)
UNROUNDED = {"unrounded": ("forward", "bias.grad"),
             "unrounded_slope1": ("forward", "x.grad", "lin_l.weight.grad", "lin_l.bias.grad", "att.grad", "bias.grad")}
VARIANTS.update({"unrounded": {}, "unrounded_slope1": dict(negative_slope=1.0)})
VARIANT_SHAPES = [(25, 2, 256, True), (64, 3, 20, True), (64, 3, 20, False), (32, 1, 64, False)]
#: (H, C) of the direct tests: 16-byte forms with a head = 16 / 64 lanes, and one wider than the registers hold; the
#: general form with C = 20 (groups of 32 lanes), 3, 1 and one wider than a wave
DIRECT = [(1, 64), (2, 256), (1, 1100), (3, 20), (5, 3), (4, 1), (2, 70)]


# --------------------------------------------------------------------------- #
# the restatement as a torch module (float32: ref32, .double(): truth64)
# --------------------------------------------------------------------------- #
class RefGATv2(nn.Module):
    def __init__(self, fi, c, heads=1, concat=True, negative_slope=0.2, bias=True, share_weights=False):
        super().__init__()
        self.fi, self.c, self.heads, self.concat, self.slope = fi, c, heads, concat, negative_slope
        self.lin_l = nn.Linear(fi, heads * c, bias=bias)
        self.lin_r = self.lin_l if share_weights else nn.Linear(fi, heads * c, bias=bias)
        self.att = nn.Parameter(torch.empty(1, heads, c))
        self.bias = nn.Parameter(torch.zeros(heads * c if concat else c)) if bias else None
        a = float(np.sqrt(6.0 / (heads + c)))
        with torch.no_grad():
            self.att.uniform_(-a, a)
            for lin in {id(self.lin_l): self.lin_l, id(self.lin_r): self.lin_r}.values():
                g = float(np.sqrt(6.0 / (fi + heads * c)))
                lin.weight.uniform_(-g, g)

    def pre_activation(self, x, edge_index):
        """(s [E', H, C], xl [N, H, C], j, i) over the edges with the self loops removed, then added"""
        n, nh, c = x.size(0), self.heads, self.c
        xl = self.lin_l(x).view(n, nh, c)
        xr = self.lin_r(x).view(n, nh, c)
        ei = pyg_ref.add_self_loops(pyg_ref.remove_self_loops(edge_index), n)
        j, i = ei[0], ei[1]
        return xl[j] + xr[i], xl, j, i

    def forward(self, x, edge_index, relu=False):
        n, nh, c = x.size(0), self.heads, self.c
        s, xl, j, i = self.pre_activation(x, edge_index)
        e = (F.leaky_relu(s, self.slope) * self.att).sum(-1)
        alpha = pyg_ref.segment_softmax(e, i, n)
        out = pyg_ref.scatter_sum(alpha.unsqueeze(-1) * xl[j], i, n)
        out = out.reshape(n, nh * c) if self.concat else out.mean(1)
        if self.bias is not None:
            out = out + self.bias
        return torch.relu(out) if relu else out


# --------------------------------------------------------------------------- #
# the per-edge formulas in numpy (dt = np.float32: ref32, np.float64: truth64); xl, xr [N, H*C], att [H*C],
# per-edge arrays [E, H] in destination-sorted order
# --------------------------------------------------------------------------- #
def _col_sum(a, dt):
    """sum over axis 0 of a 2-D array in dt, pairwise (numpy sums pairwise along the contiguous axis only)"""
    return np.ascontiguousarray(a.T).sum(-1, dtype=dt)


def v2_s(ptr, other, xl, xr, nh, dt):
    n, c = len(ptr) - 1, xl.shape[1] // nh
    return xl.astype(dt).reshape(n, nh, c)[other] + xr.astype(dt).reshape(n, nh, c)[seg_of(ptr)]


def v2_logits(ptr, other, xl, xr, att, slope, nh, dt):
    s = v2_s(ptr, other, xl, xr, nh, dt)
    l = np.where(s > 0, s, dt(np.float32(slope)) * s)
    return (l * att.astype(dt).reshape(1, nh, -1)).sum(-1, dtype=dt)


def v2_softmax(ptr, e, dt):
    seg, n = seg_of(ptr), len(ptr) - 1
    out = np.empty_like(e, dtype=dt)
    for k in range(e.shape[1]):
        m = np.full(n, -np.inf, dt)
        np.maximum.at(m, seg, e[:, k].astype(dt))
        ex = np.exp(e[:, k].astype(dt) - m[seg])
        out[:, k] = ex / (_seg_sum(ex, seg, n) + dt(1e-16))[seg]
    return out


def v2_alpha(ptr, other, xl, xr, att, slope, nh, dt):
    return v2_softmax(ptr, v2_logits(ptr, other, xl, xr, att, slope, nh, dt), dt)


def v2_backward(ptr, other, xl, xr, att, slope, alpha, galpha, gm, nh, dt):
    """(ge [E, H], g_xr [N, H*C], g_xl [N, H*C], g_att [H*C]) by the formulas of the contract"""
    seg, n = seg_of(ptr), len(ptr) - 1
    c = xl.shape[1] // nh
    sl = dt(np.float32(slope))
    al, ga = alpha.astype(dt), galpha.astype(dt)
    dot = np.stack([_seg_sum(np.ascontiguousarray((al * ga)[:, k]), seg, n) for k in range(nh)], 1)
    ge = al * (ga - dot[seg])
    s = v2_s(ptr, other, xl, xr, nh, dt)
    t = ge[:, :, None] * att.astype(dt).reshape(1, nh, c) * np.where(s > 0, dt(1), sl)
    t = t.reshape(len(seg), nh * c)
    g_xr = np.stack([_col_sum(t[ptr[i]:ptr[i + 1]], dt) for i in range(n)]) if n else np.zeros((0, nh * c), dt)
    contrib = (al[:, :, None] * gm.astype(dt).reshape(n, nh, c)[seg]).reshape(len(seg), nh * c) + t
    order = np.argsort(other, kind="stable")
    bounds = np.searchsorted(other[order], np.arange(n + 1))
    g_xl = np.stack([_col_sum(contrib[order[bounds[j]:bounds[j + 1]]], dt) for j in range(n)]) if n else \
        np.zeros((0, nh * c), dt)
    g_att = _col_sum((ge[:, :, None] * np.where(s > 0, s, sl * s)).reshape(len(seg), nh * c), dt)
    return ge, g_xr.astype(dt), g_xl.astype(dt), g_att


def check_g_xr_rows(ptr, other, xl, xr, att, slope, ge, g_xr, nh):
    """Per row and column g_xr is the float32 sum of the segment's t = ge att leaky_relu'(s): within (len + 2) 2^-23
    sum |t| of their exact sum, the bound of any summation order with the two roundings of each t.  Needs no reference:
    sum_p ge[p, k] is mathematically zero, so in a short segment whose s share a sign the row cancels to rounding noise
    and has no value to compare per row (``check_g_a_dst`` of test_gat_edge_kernels.py, for the same reason) - the
    VALUE of g_xr is compared on the scale of the whole tensor."""
    c = xl.shape[1] // nh
    s = v2_s(ptr, other, xl, xr, nh, np.float32)
    t = ge.astype(np.float64)[:, :, None] * att.astype(np.float64).reshape(1, nh, c) * np.where(s > 0, 1.0, float(np.float32(slope)))
    t = t.reshape(len(t), nh * c)
    for i in range(len(ptr) - 1):
        seg = t[ptr[i]:ptr[i + 1]]
        bound = (len(seg) + 2) * 2.0 ** -23 * np.abs(seg).sum(0)
        assert (np.abs(g_xr[i] - seg.sum(0)) <= bound).all(), i


def direct_inputs(n, nh, c, seed):
    rng = np.random.default_rng(seed)
    xl = (0.5 * rng.standard_normal((n, nh * c))).astype(np.float32)
    xr = (0.5 * rng.standard_normal((n, nh * c))).astype(np.float32)
    att = rng.uniform(-1.5, 1.5, nh * c).astype(np.float32) / np.float32(np.sqrt(c))
    gm = (rng.uniform(0.5, 1.5, (n, nh * c)) * np.where(rng.random((n, 1)) < 0.5, -1.0, 1.0)).astype(np.float32)
    return xl, xr, att, gm


def heads_galpha(ptr, nh, seed):
    return np.ascontiguousarray(np.stack([galpha_for(ptr, seed + k) for k in range(nh)], 1))


# --------------------------------------------------------------------------- #
# the layer cases (shared by the CPU conditioning test and the GPU tests; computed once, never modified)
# --------------------------------------------------------------------------- #
def _graph(kind, seed):
    """(n, edge_index [2, E] int64)"""
    if kind == "multigraph":
        return 300, random_multigraph(300, 2400, seed)
    if kind == "hub":
        return 300, seg_graph(seg_lens(300, HUB), seed)        # one segment of HUB = 5,000 edges: far longer than a wave
    if kind == "n1":
        return 1, np.zeros((2, 1), np.int64)                    # one node and its self loop
    if kind == "e0":
        return 50, np.zeros((2, 0), np.int64)
    z = load_golden("graphnet_gat_h32.npz")
    key = "rest" if kind == "golden_rest" else "rig"
    return z[key + "_x"].shape[0], z[key + "_edge_index"].astype(np.int64)


def _ref_run(mod, x, ei, gup, relu, dtype):
    for p in mod.parameters():
        p.grad = None
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    out = mod(xt, torch.from_numpy(ei), relu=relu)
    (out * torch.from_numpy(gup).to(dtype)).sum().backward()
    grads = {n: p.grad.detach().numpy().copy() for n, p in mod.named_parameters()}
    return out.detach().numpy(), xt.grad.numpy(), grads


def _dyadic(a, bits=7):
    """``a`` rounded to ``bits`` bits below the power of two that bounds it (8 significant bits at the most)"""
    top = float(np.abs(a).max()) if a.size else 0.0
    if top == 0.0:
        return a
    grid = 2.0 ** (int(np.ceil(np.log2(top))) - bits)
    return (np.round(a / grid) * grid).astype(a.dtype)


@functools.lru_cache(maxsize=None)
def layer_case(fi, nh, c, concat, kind, variant):
    """inputs, the reference module and its float32 / float64 results of one layer case"""
    torch.set_num_threads(1)
    opts = dict(VARIANTS[variant])
    relu = opts.pop("relu", False)
    n, ei = _graph(kind, 3)
    rng = np.random.default_rng(fi + nh + c)
    exact = variant not in UNROUNDED
    x = rng.standard_normal((n, fi))
    x = (np.clip(np.round(x * 32) / 32, -4, 4) if exact else x).astype(np.float32)
    gup = rng.uniform(0.5, 1.5, (n, nh * c if concat else c)).astype(np.float32)
    torch.manual_seed(11)
    cpu = RefGATv2(fi, c, heads=nh, concat=concat, **opts)      # default initialisation; the output bias is zeros
    with torch.no_grad():                                       # (module docstring: s exact in float32)
        for name, p in cpu.named_parameters():
            if exact and name.startswith("lin_"):
                p.copy_(torch.from_numpy(_dyadic(p.numpy().copy())))
    r32 = _ref_run(cpu, x, ei, gup, relu, torch.float32)
    r64 = _ref_run(copy.deepcopy(cpu).double(), x, ei, gup, relu, torch.float64)
    return dict(n=n, ei=ei, x=x, gup=gup, cpu=cpu, relu=relu, opts=opts, r32=r32, r64=r64, exact=exact,
                only=UNROUNDED.get(variant))


def _layer_cases():
    cases = [(s, kind, "default") for s in SHAPES for kind in GRAPHS]
    cases += [(s, "multigraph", v) for s in VARIANT_SHAPES for v in VARIANTS if v != "default"]
    cases += [(s, "hub", v) for s in VARIANT_SHAPES for v in UNROUNDED]
    return cases


def _pairs(got, r32, r64, only=None):
    """(name, got, ref32, truth64) over the output, x.grad and every parameter gradient of the reference (``only``: of
    these names)"""
    out = [("forward", got[0], r32[0], r64[0]), ("x.grad", got[1], r32[1], r64[1])]
    out += [(name + ".grad", got[2][name], r32[2][name], r64[2][name]) for name in r32[2]]
    return [t for t in out if only is None or t[0] in only]


# --------------------------------------------------------------------------- #
# CPU
# --------------------------------------------------------------------------- #
def test_constructor_parameters_and_state_dict():
    for concat in (True, False):
        for share in (False, True):
            for bias in (True, False):
                conv = dc.nn.GATv2Conv(21, 64, heads=4, concat=concat, bias=bias, share_weights=share)
                want = {"lin_l.weight": (256, 21), "lin_r.weight": (256, 21), "att": (1, 4, 64)}
                if bias:
                    want.update({"lin_l.bias": (256,), "lin_r.bias": (256,), "bias": (256,) if concat else (64,)})
                assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == want
                assert (conv.lin_r is conv.lin_l) == share
                assert len(list(conv.parameters())) == (1 + (1 if share else 2) * (2 if bias else 1) + (1 if bias else 0))
                assert conv.out_width == (256 if concat else 64)
                assert conv.graph_flags() == dict(self_loops=True, normalize=False)
                r = repr(conv)
                assert r.startswith("GATv2Conv(") and "21, 64, heads=4" in r
                assert ("concat=False" in r) == (not concat) and ("share_weights=True" in r) == share
                ref = RefGATv2(21, 64, heads=4, concat=concat, bias=bias, share_weights=share)
                assert set(ref.state_dict()) == set(conv.state_dict())
                conv.load_state_dict(ref.state_dict(), strict=True)
    conv = dc.nn.GATv2Conv(21, 64, heads=4)
    glorot, att_b, lin_b = float(np.sqrt(6.0 / (21 + 256))), float(np.sqrt(6.0 / (4 + 64))), float(1 / np.sqrt(21.0))
    seen = []
    for _ in range(3):
        conv.reset_parameters()
        seen.append(conv.att.detach().clone())
        assert 0.5 * att_b < float(conv.att.detach().abs().max()) <= att_b
        for lin in (conv.lin_l, conv.lin_r):
            assert 0.5 * glorot < float(lin.weight.detach().abs().max()) <= glorot
            assert 0.5 * lin_b < float(lin.bias.detach().abs().max()) <= lin_b
        assert float(conv.bias.detach().abs().max()) == 0.0
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    one = dc.nn.GATv2Conv(21, 64)
    assert one.heads == 1 and one.concat is True and one.negative_slope == 0.2 and one.share_weights is False
    with pytest.raises(ValueError):
        dc.nn.GATv2Conv(21, 64, heads=0)
    with pytest.raises(TypeError):
        dc.nn.GATv2Conv(21, 64, edge_dim=3)                      # not supported: absent from the signature
    with pytest.raises(RuntimeError, match="HIP device"):
        conv(torch.zeros(5, 21), torch.zeros(2, 3, dtype=torch.long))
    assert "GATv2Conv" in dc.nn.__all__


def test_importable_through_the_torch_geometric_alias():
    import sys
    from deformcontact_amd.pyg_alias import install_as_torch_geometric
    names = ("torch_geometric", "torch_geometric.nn", "torch_geometric.data")
    saved = {k: sys.modules.get(k) for k in names}
    try:
        install_as_torch_geometric(force=True)
        from torch_geometric.nn import GATv2Conv
        assert GATv2Conv is dc.nn.GATv2Conv
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def _entry_calls():
    """name -> call(N, H, C, pointers given?, leading dimension) of every entry of dc_gatv2.hip, otherwise valid"""
    L = _lib.lib()
    p = lambda ok: 64 if ok else None                           # any non-null address: rejected calls never touch it

    def ws(n, h, c):
        return max(L.dc_gatv2_workspace_bytes(max(n, 0), max(h, 1), max(c, 1)), 16)
    return {
        "dc_gatv2_softmax_fwd": lambda n, h, c, ok, ld: L.dc_gatv2_softmax_fwd(
            p(ok), p(ok), p(ok), ld, p(ok), ld, p(ok), 0.2, p(ok), n, h, c, None),
        "dc_gatv2_softmax_bwd": lambda n, h, c, ok, ld: L.dc_gatv2_softmax_bwd(
            p(ok), p(ok), p(ok), p(ok), p(ok), ld, p(ok), ld, p(ok), 0.2, p(ok), p(ok), ld, p(ok), 0, p(ok), ws(n, h, c),
            n, h, c, None),
        "dc_gatv2_source_bwd": lambda n, h, c, ok, ld: L.dc_gatv2_source_bwd(
            p(ok), p(ok), p(ok), p(ok), p(ok), p(ok), ld, p(ok), ld, p(ok), ld, p(ok), 0.2, p(ok), ld, n, h, c, None),
    }


def test_abi_argument_errors_of_the_gatv2_entries_without_gpu():
    """null pointers, negative N, H < 1, C < 1, short leading dimensions: -1 and the entry's name, before any HIP call."""
    L = _lib.lib()
    calls = _entry_calls()
    declared = [n for n in _lib.exported_names() if "gatv2" in n and not n.endswith("workspace_bytes")]
    assert sorted(declared) == sorted(calls)
    assert not any("heads" in n or "edge_attr" in n for n in declared)
    for name, call in calls.items():
        assert call(3, 4, 16, False, 64) == -1 and name.encode() in L.dc_last_error() and b"null" in L.dc_last_error(), name
        assert call(-1, 4, 16, True, 64) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, 0, 16, True, 64) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, -2, 16, True, 64) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, 4, 0, True, 64) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, 4, -1, True, 64) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, 4, 16, True, 63) == -1 and name.encode() in L.dc_last_error() and b"leading" in L.dc_last_error(), name
    # the workspace: one row of H*C floats per DC_GATV2_ROWS = 32 destinations, at every width
    assert L.dc_gatv2_workspace_bytes(0, 5, 3) == 0
    assert L.dc_gatv2_workspace_bytes(33, 5, 3) == 2 * 15 * 4
    assert L.dc_gatv2_workspace_bytes(-1, 5, 3) < 0 and L.dc_gatv2_workspace_bytes(3, 0, 3) < 0
    assert L.dc_gatv2_softmax_bwd(64, 64, 64, 64, 64, 15, 64, 15, 64, 0.2, 64, 64, 15, 64, 0, 64, 2 * 15 * 4 - 1, 33, 5, 3,
                                  None) == -1 and b"workspace" in L.dc_last_error()


@pytest.mark.parametrize("nh,c", [(4, 16), (3, 5), (1, 8)])
def test_backward_formulas_against_autograd_on_the_cpu(nh, c):
    """The hand-written backward of the contract (numpy, float64) == torch autograd through RefGATv2 (float64)."""
    lens = seg_lens(67, hub=300)
    n = len(lens)
    ptr, other, dst = host_adjacency(lens, 5)
    rng = np.random.default_rng(nh * 100 + c)
    fi = 12
    x = rng.standard_normal((n, fi))
    gup = rng.uniform(0.5, 1.5, (n, nh * c))
    torch.manual_seed(nh + c)
    slope = float(np.float32(0.2))
    mod = RefGATv2(fi, c, heads=nh, negative_slope=slope).double()
    xl_t = mod.lin_l(torch.from_numpy(x)).detach().requires_grad_(True)
    xr_t = mod.lin_r(torch.from_numpy(x)).detach().requires_grad_(True)
    att_t = mod.att.detach().clone().requires_grad_(True)
    to, tdst = torch.from_numpy(other), torch.from_numpy(dst)
    s = xl_t.view(n, nh, c)[to] + xr_t.view(n, nh, c)[tdst]
    e = (F.leaky_relu(s, slope) * att_t).sum(-1)
    al = pyg_ref.segment_softmax(e, tdst, n)
    al.retain_grad()
    e.retain_grad()
    out = pyg_ref.scatter_sum(al.unsqueeze(-1) * xl_t.view(n, nh, c)[to], tdst, n).reshape(n, nh * c)
    (out * torch.from_numpy(gup)).sum().backward()
    xl, xr, att = xl_t.detach().numpy(), xr_t.detach().numpy(), att_t.detach().numpy().reshape(-1)
    seg_err = seg_rel_err_on(ptr)
    a64 = v2_alpha(ptr, other, xl, xr, att, slope, nh, np.float64)
    assert max(seg_err(a64[:, k], al.detach().numpy()[:, k]) for k in range(nh)) < 1e-12
    # the whole layer: the edge list with its loops handed to the module gives the same output
    want = mod(torch.from_numpy(x), torch.from_numpy(np.stack([other, dst]))).detach().numpy()
    assert rel_err(out.detach().numpy() + mod.bias.detach().numpy(), want) < 1e-12
    galpha = np.einsum("pkc,pkc->pk", gup.reshape(n, nh, c)[dst], xl.reshape(n, nh, c)[other])
    assert rel_err(galpha, al.grad.numpy()) < 1e-12
    ge, g_xr, g_xl, g_att = v2_backward(ptr, other, xl, xr, att, slope, a64, galpha, gup, nh, np.float64)
    assert rel_err(ge, e.grad.numpy()) < 1e-10
    assert rel_err(g_xr, xr_t.grad.numpy()) < 1e-10
    assert rel_err(g_xl, xl_t.grad.numpy()) < 1e-10
    assert rel_err(g_att, att_t.grad.numpy().reshape(-1)) < 1e-10


def test_float32_restatement_within_the_bar_of_float64_on_the_layer_inputs():
    """Every layer case of the GPU tests: float32 RefGATv2 within 1e-5 of float64, output and every gradient."""
    worst = 0.0
    for (fi, nh, c, concat), kind, variant in _layer_cases():
        case = layer_case(fi, nh, c, concat, kind, variant)
        xt, te = torch.from_numpy(case["x"]), torch.from_numpy(case["ei"])
        s32 = case["cpu"].pre_activation(xt, te)[0]
        s64 = copy.deepcopy(case["cpu"]).double().pre_activation(xt.double(), te)[0]
        if case["exact"]:
            assert torch.equal(s32.double(), s64), "s is not exact in float32: leaky_relu' could differ between evaluations"
        else:
            assert not torch.equal(s32.double(), s64)           # these cases do see the rounding of the linears
        for name, _, a32, a64 in _pairs(case["r32"], case["r32"], case["r64"], case["only"]):
            d = rel_err(a32, a64)
            record_parity(f"RefGATv2 fp32 vs fp64 {fi}->{nh}x{c} concat={concat} {kind} {variant} {name}", None, e_o=d)
            assert d < TOL, (fi, nh, c, concat, kind, variant, name, d)
            worst = max(worst, d)
    assert worst < TOL


@pytest.mark.parametrize("nh,c", DIRECT)
def test_float32_restatement_within_the_bar_of_float64_on_the_direct_inputs(nh, c):
    n = 131
    lens = seg_lens(n)
    ptr, other, _ = host_adjacency(lens, 9 + nh)
    seg_err = seg_rel_err_on(ptr)
    for slope in (0.2, 0.0):
        xl, xr, att, gm = direct_inputs(n, nh, c, 40 + nh + c)
        a32 = v2_alpha(ptr, other, xl, xr, att, slope, nh, np.float32)
        a64 = v2_alpha(ptr, other, xl, xr, att, slope, nh, np.float64)
        assert a32.dtype == np.float32
        e64 = v2_logits(ptr, other, xl, xr, att, slope, nh, np.float64)
        spread = max(float((np.maximum.reduceat(e64[:, k], ptr[:-1]) - np.minimum.reduceat(e64[:, k], ptr[:-1])).max())
                     for k in range(nh))
        assert spread < 12.0, spread                             # a few units: the backward stays well conditioned
        galpha = heads_galpha(ptr, nh, 11)
        b32 = v2_backward(ptr, other, xl, xr, att, slope, a32, galpha, gm, nh, np.float32)
        b64 = v2_backward(ptr, other, xl, xr, att, slope, a32, galpha, gm, nh, np.float64)
        dists = {"alpha": max(seg_err(a32[:, k], a64[:, k]) for k in range(nh)),
                 "ge": max(seg_err(b32[0][:, k], b64[0][:, k]) for k in range(nh)),
                 "g_xr": rel_err(b32[1], b64[1]), "g_xl": row_rel_err(b32[2], b64[2]), "g_att": rel_err(b32[3], b64[3])}
        for name, d in dists.items():
            record_parity(f"numpy fp32 vs fp64 {nh}x{c} slope={slope} {name}", None, e_o=d)
            assert d < 0.5 * TOL, (name, slope, d)


# --------------------------------------------------------------------------- #
# GPU: the layer
# --------------------------------------------------------------------------- #
def _device_conv(cpu, fi, nh, c, concat, **opts):
    conv = dc.nn.GATv2Conv(fi, c, heads=nh, concat=concat, **opts)
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
    return out.detach(), xg.grad, {n: p.grad.detach().clone() for n, p in conv.named_parameters()}


def _check_layer(fi, nh, c, concat, kind, variant):
    case = layer_case(fi, nh, c, concat, kind, variant)
    clear_cache()
    conv = _device_conv(case["cpu"], fi, nh, c, concat, **case["opts"])
    _lib.kernel_trace(True)
    og, gxg, gpg = _device_run(conv, case["x"], case["ei"], case["gup"], relu=case["relu"])
    counts = _lib.kernel_trace_counts()
    _lib.kernel_trace(False)
    for k in ("k_gatv2_softmax_fwd", "k_gatv2_logit_grad", "k_gatv2_dst_bwd", "k_gatv2_colsum", "k_gatv2_src_bwd",
              "k_spmm_heads", "k_sddmm_heads"):
        assert any(k in name for name in counts), (k, counts)
    tag = f"GATv2Conv {fi}->{nh}x{c} concat={concat} {kind} {variant}"
    got = (_np(og), _np(gxg), {k: _np(v) for k, v in gpg.items()})
    assert got[0].shape == case["r32"][0].shape and set(got[2]) == set(case["r32"][2])
    for name, a, a32, a64 in _pairs(got, case["r32"], case["r64"], case["only"]):
        assert_parity(a, a32, a64, TOL, f"{tag} {name}")
    assert_parity(got[0], case["r32"][0], case["r64"][0], TOL, f"{tag} forward per row", metric=row_rel_err)


@gpu
@pytest.mark.parametrize("kind", GRAPHS)
@pytest.mark.parametrize("fi,nh,c,concat", SHAPES)
def test_layer_parity(fi, nh, c, concat, kind):
    """forward and the gradients of x, lin_l / lin_r weight and bias, att and bias against RefGATv2 at 1e-5."""
    _check_layer(fi, nh, c, concat, kind, "default")


@gpu
@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "default"])
@pytest.mark.parametrize("fi,nh,c,concat", VARIANT_SHAPES)
def test_layer_parity_options(fi, nh, c, concat, variant):
    """share_weights, bias=False, relu=True, negative_slope=0 - on the fused and on the odd-width route; and the
    unrounded inputs, see below."""
    _check_layer(fi, nh, c, concat, "multigraph", variant)


@gpu
@pytest.mark.parametrize("variant", list(UNROUNDED))
@pytest.mark.parametrize("fi,nh,c,concat", VARIANT_SHAPES)
def test_layer_parity_unrounded_inputs(fi, nh, c, concat, variant):
    """x ~ N(0, 1) and default-initialised parameters as they come, on the hub graph: the two linears round (24-bit
    products, bias in the epilogue).  ``unrounded``: the output and bias.grad, which are continuous in s;
    ``unrounded_slope1``: negative_slope = 1, where leaky_relu has no branch - the output and every gradient that is
    not mathematically zero."""
    _check_layer(fi, nh, c, concat, "hub", variant)


# --------------------------------------------------------------------------- #
# GPU: the entries called directly
# --------------------------------------------------------------------------- #
@gpu
@pytest.mark.parametrize("slope", [0.2, 0.0])
@pytest.mark.parametrize("nh,c", DIRECT)
def test_entries_per_edge_and_row(nh, c, slope):
    """LENS + the 5,000-edge hub: alpha per edge and head, ge per segment, g_xr / g_xl per row, g_att; twice: same bits."""
    n = 131
    g, ptr, other, lens = device_graph(n, 9 + nh)
    e, cap = int(ptr[-1]), g.capacity
    seg_err = seg_rel_err_on(ptr)
    xl, xr, att, gm = direct_inputs(n, nh, c, 40 + nh + c)
    txl, txr, tatt, tgm = _dev(xl), _dev(xr), _dev(att), _dev(gm)
    alpha = ops._gatv2_softmax_fwd(g, txl, txr, tatt, slope, nh, c)
    assert alpha.shape == (max(cap, 1), nh) and (alpha[e:] == 0).all()
    assert torch.equal(alpha, ops._gatv2_softmax_fwd(g, txl, txr, tatt, slope, nh, c))
    got = _np(alpha)[:e]
    a32 = v2_alpha(ptr, other, xl, xr, att, slope, nh, np.float32)
    a64 = v2_alpha(ptr, other, xl, xr, att, slope, nh, np.float64)
    assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
    for k in range(nh):
        assert_parity(got[:, k], a32[:, k], a64[:, k], TOL, f"alpha {nh}x{c} slope={slope} head {k}", metric=seg_err)
        sums = _seg_sum(got[:, k].astype(np.float64), seg_of(ptr), n)
        assert np.abs(sums - 1).max() <= 1e-6, float(np.abs(sums - 1).max())
        assert (got[ptr[:-1][lens == 1], k] == 1.0).all()       # a one-edge segment: exactly 1
    # operands in a wider buffer (ld > H*C) give the same bits
    wide = torch.full((n, nh * c + 12), 1e30, device=DEV)
    wide[:, 4:4 + nh * c] = txl
    assert torch.equal(alpha, ops._gatv2_softmax_fwd(g, wide[:, 4:4 + nh * c], txr, tatt, slope, nh, c))
    # backward from the device's alpha
    galpha = heads_galpha(ptr, nh, 11)
    tg = torch.zeros_like(alpha)
    tg[:e] = _dev(galpha)
    runs = []
    for _ in range(2):
        g_att = torch.full((nh * c,), 7.0, device=DEV)
        ge, g_xr = ops._gatv2_softmax_bwd(g, alpha, tg, txl, txr, tatt, slope, nh, c, g_att, False)
        g_xl = ops._gatv2_source_bwd(g, alpha, ge, tgm, txl, txr, tatt, slope, nh, c)
        runs.append((ge, g_xr, g_xl, g_att))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    ge, g_xr, g_xl, g_att = runs[0]
    assert (ge[e:] == 0).all() and all(torch.isfinite(t).all() for t in runs[0])
    b32 = v2_backward(ptr, other, xl, xr, att, slope, got, galpha, gm, nh, np.float32)
    b64 = v2_backward(ptr, other, xl, xr, att, slope, got, galpha, gm, nh, np.float64)
    tag = f"{nh}x{c} slope={slope}"
    for k in range(nh):
        assert_parity(_np(ge)[:e, k], b32[0][:, k], b64[0][:, k], TOL, f"ge {tag} head {k}", metric=seg_err)
    assert_parity(_np(g_xr), b32[1], b64[1], TOL, f"g_xr {tag}")
    check_g_xr_rows(ptr, other, xl, xr, att, slope, _np(ge)[:e], _np(g_xr), nh)
    assert_parity(_np(g_xl), b32[2], b64[2], TOL, f"g_xl {tag}", metric=row_rel_err)
    assert_parity(_np(g_att), b32[3], b64[3], TOL, f"g_att {tag}")
    # accumulate: into what the buffer holds (direct parameter-gradient mode)
    acc = g_att.clone()
    ops._gatv2_softmax_bwd(g, alpha, tg, txl, txr, tatt, slope, nh, c, acc, True)
    assert torch.equal(acc, g_att + g_att)


@gpu
def test_one_channel_positive_att_unit_slope_is_gat():
    """C = 1, att > 0, slope = 1: e[p, k] = att[k] xl[j, k] + att[k] xr[i, k] up to rounding - GATConv's a_src + a_dst."""
    n, nh = 131, 4
    g, ptr, other, lens = device_graph(n, 23)
    e = int(ptr[-1])
    rng = np.random.default_rng(6)
    xl = rng.standard_normal((n, nh)).astype(np.float32)
    xr = rng.standard_normal((n, nh)).astype(np.float32)
    att = rng.uniform(0.5, 1.5, nh).astype(np.float32)
    alpha = ops._gatv2_softmax_fwd(g, _dev(xl), _dev(xr), _dev(att), 1.0, nh, 1)
    gat = ops._heads_softmax_fwd(g, _dev(xl * att), _dev(xr * att), 1.0, n, nh)
    seg_err = seg_rel_err_on(ptr)
    for k in range(nh):
        d = seg_err(_np(alpha)[:e, k], _np(gat)[:e, k])
        record_parity(f"alpha C=1 head {k} vs dc_gat_edge_softmax_heads_fwd", d, metric="seg_rel_err")
        assert d < TOL, (k, d)
        one = run_softmax_fwd(g.fwd.ptr, g.fwd.other, _dev(xl[:, k] * att[k]), _dev(xr[:, k] * att[k]), 1.0, n, g.capacity)
        assert seg_err(_np(alpha)[:e, k], _np(one)[:e]) < TOL


@gpu
def test_entries_with_no_rows():
    """N = 0: every entry returns 0 without a launch that reads anything; g_att is written (zeros)."""
    L = _lib.lib()
    z = torch.zeros(16, device=DEV)
    zi = torch.zeros(4, dtype=torch.int32, device=DEV)
    g_att = torch.full((15,), 3.0, device=DEV)
    assert L.dc_gatv2_softmax_fwd(zi.data_ptr(), zi.data_ptr(), None, 15, None, 15, z.data_ptr(), 0.2, None, 0, 5, 3,
                                  None) == 0
    assert L.dc_gatv2_softmax_bwd(zi.data_ptr(), zi.data_ptr(), None, None, None, 15, None, 15, z.data_ptr(), 0.2, None,
                                  None, 15, g_att.data_ptr(), 0, None, 0, 0, 5, 3, None) == 0
    assert L.dc_gatv2_source_bwd(zi.data_ptr(), zi.data_ptr(), zi.data_ptr(), None, None, None, 15, None, 15, None, 15,
                                 z.data_ptr(), 0.2, None, 15, 0, 5, 3, None) == 0
    torch.cuda.synchronize()
    assert (g_att == 0).all()


# --------------------------------------------------------------------------- #
# GPU: bit-for-bit properties, capture
# --------------------------------------------------------------------------- #
def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert set(a[2]) == set(b[2])
    for name in a[2]:
        assert torch.equal(a[2][name], b[2][name]), name


@gpu
@pytest.mark.parametrize("fi,nh,c,concat", [(25, 2, 256, True), (64, 3, 20, True), (64, 3, 20, False), (32, 1, 64, False)])
def test_bit_for_bit_relu_deferred_and_repeat(fi, nh, c, concat):
    case = layer_case(fi, nh, c, concat, "hub", "default")
    n, ei, x, gup = case["n"], case["ei"], case["x"], case["gup"]
    clear_cache()
    conv = _device_conv(case["cpu"], fi, nh, c, concat)
    with torch.no_grad():
        conv.bias.uniform_(-0.3, 0.3)
    tei, xg = torch.from_numpy(ei).to(DEV), torch.from_numpy(x).to(DEV)
    plain = ops.resolve(conv(xg, tei)).clone()
    assert plain.shape == (n, conv.out_width)
    want = torch.relu(plain)
    assert (plain < 0).any() and (plain > 0).any()
    assert torch.equal(conv(xg, tei, relu=True), want)
    y = conv(xg, tei)
    assert type(y).__name__ == "DeferredActivation" and y.shape == plain.shape
    assert torch.equal(F.relu(y), want)
    for kw in ({}, {"relu": True}):
        _same(_device_run(conv, x, ei, gup, **kw), _device_run(conv, x, ei, gup, **kw))


@gpu
@pytest.mark.parametrize("fi,nh,c,concat", [(25, 2, 256, True), (64, 3, 20, False)])
def test_shared_weights_equal_a_copied_lin_r(fi, nh, c, concat):
    case = layer_case(fi, nh, c, concat, "multigraph", "shared")
    ei, x, gup = case["ei"], case["x"], case["gup"]
    clear_cache()
    shared = _device_conv(case["cpu"], fi, nh, c, concat, share_weights=True)
    two = dc.nn.GATv2Conv(fi, c, heads=nh, concat=concat).to(DEV)
    with torch.no_grad():
        for lin in (two.lin_l, two.lin_r):
            lin.weight.copy_(shared.lin_l.weight)
            lin.bias.copy_(shared.lin_l.bias)
        two.att.copy_(shared.att)
        two.bias.copy_(shared.bias)
    a = _device_run(shared, x, ei, gup)
    b = _device_run(two, x, ei, gup)
    assert torch.equal(a[0], b[0])
    r64 = case["r64"][2]
    for p in ("weight", "bias"):
        both = b[2][f"lin_l.{p}"] + b[2][f"lin_r.{p}"]
        assert_parity(_np(a[2][f"lin_l.{p}"]), _np(both), r64[f"lin_l.{p}"], TOL, f"shared lin_l.{p}.grad vs the sum of two")
    assert_parity(_np(a[2]["att"]), _np(b[2]["att"]), r64["att"], TOL, "shared att.grad")
    assert_parity(_np(a[1]), _np(b[1]), case["r64"][1], TOL, "shared x.grad")


@gpu
@pytest.mark.parametrize("fi,nh,c,concat", [(25, 2, 256, True), (64, 3, 20, True)])
def test_strided_input_and_gradient_give_the_same_bits(fi, nh, c, concat):
    case = layer_case(fi, nh, c, concat, "multigraph", "default")
    n, ei, x, gup = case["n"], case["ei"], case["x"], case["gup"]
    clear_cache()
    conv = _device_conv(case["cpu"], fi, nh, c, concat)
    want = _device_run(conv, x, ei, gup)
    wide_x = torch.full((n, fi + 7), 1e30, device=DEV)
    wide_x[:, 3:3 + fi] = torch.from_numpy(x).to(DEV)
    wide_g = torch.full((n, 2 * gup.shape[1]), 1e30, device=DEV)
    wide_g[:, ::2] = torch.from_numpy(gup).to(DEV)
    xs, gs = wide_x[:, 3:3 + fi], wide_g[:, ::2]
    assert not xs.is_contiguous() and not gs.is_contiguous()
    for p in conv.parameters():
        p.grad = None
    xg = xs.detach().requires_grad_(True)
    assert not xg.is_contiguous()
    out = ops.resolve(conv(xg, torch.from_numpy(ei).to(DEV)))
    torch.autograd.backward([out], [gs])
    torch.cuda.synchronize()
    _same((out.detach(), xg.grad, {k: p.grad for k, p in conv.named_parameters()}), want)


@gpu
def test_forward_and_backward_captured_and_replayed():
    """forward + backward of two stacked layers on ONE stream under torch.cuda.graph; two replays with new x in the
    static input, each bit-identical to the eager run on that input."""
    n, ei = _graph("multigraph", 12)
    fi, nh, c = 32, 4, 16
    torch.manual_seed(3)
    l1 = dc.nn.GATv2Conv(fi, c, heads=nh).to(DEV)
    l2 = dc.nn.GATv2Conv(nh * c, c, heads=nh, concat=False, share_weights=True).to(DEV)
    with torch.no_grad():
        l1.bias.uniform_(-0.3, 0.3)
        l2.bias.uniform_(-0.3, 0.3)
    params = list(l1.parameters()) + list(l2.parameters())
    tei = torch.from_numpy(ei).to(DEV)
    rng = np.random.default_rng(1)
    xs = [torch.from_numpy(rng.standard_normal((n, fi)).astype(np.float32)).to(DEV) for _ in range(3)]
    gup = torch.from_numpy(rng.uniform(0.5, 1.5, (n, c)).astype(np.float32)).to(DEV)
    static_x = xs[0].clone().requires_grad_(True)
    leaves = [static_x] + params
    for t in leaves:
        t.grad = torch.zeros_like(t)

    def step():
        for t in leaves:
            t.grad.zero_()
        out = l2(l1(static_x, tei, relu=True), tei, relu=True)
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
