"""``TransformerConv``: the layer, its autograd Function and the C entries of dc_transformer.hip.

The reference is this file's own restatement of the contract in INTEGRATION.md 1.4 (PyG 2.5.2 transformer_conv.py):
``RefTransformer``, a torch CPU module evaluated in float32 (``ref32``) and float64 (``truth64``) with gradients from
torch autograd, and a numpy restatement of the per-edge formulas (dtype-parametrised) for the entries called directly.

CPU: constructor / state_dict contract, argument checks of every new C entry, the restatements against each other
(float32 within the bar of float64 on every input the GPU tests use - the distance goes to ``record_parity`` - and the
hand-written backward formulas against torch autograd in float64).

GPU: the layer at 1e-5 (``helpers.assert_parity``: within 1e-5 of the float32 restatement or of float64; nothing wider,
nothing registered ``special``), the entries per edge / row, the bit-for-bit properties, capture.  One gradient of
the layer, ``lin_key.bias.grad``, is mathematically zero and is held to 1e-5 of the scale of its terms instead of its
own (``key_bias_mass``).

The adjacencies are built WITHOUT self-loop handling: the layer takes the edge set as given, so the graphs of
``tests/test_gat_edge_kernels.py`` (``seg_graph`` of ``seg_lens``) give in-degrees ``LENS - 1`` = 0, 1, 6, ... and the
hub, and ``random_multigraph`` keeps its self loops, duplicates and isolated nodes.

Everything is smooth (no branch like GATv2's leaky_relu'), so the inputs are unrounded: default-initialised parameters
and x ~ N(0, 1) for the layer; q, k, v, gm ~ N(0, 1) for the direct tests (the logits are about N(0, 1) after the
scale) with the upstream ``galpha`` of ``test_gat_edge_kernels.galpha_for``.

Metrics of the direct tests.  alpha and gl per segment, g_v per row (``seg_rel_err_on`` / ``row_rel_err``).
``sum_p ge[p, h] = 0`` over a segment, so a row of g_q of a destination with in-degree <= 1 is mathematically zero, and
so is a row of g_k all of whose out-edges enter such destinations; short segments cancel partly.  g_q and g_k are
therefore compared on the scale of the whole tensor, and every row is held to the rounding bound of a float32 sum of
its terms (``check_row_sums``; as ``check_g_xr_rows`` of tests/test_gatv2.py).  Rows of g_q without in-edges are
exactly 0.
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
from deformcontact_amd.nn import TransformerConv  # noqa: F401  (the module needs the layer: no test runs without it)
from oracle import pyg_ref
from tests.helpers import assert_parity, load_golden, random_multigraph, record_parity, rel_err, row_rel_err
from tests.test_gat_edge_kernels import (HUB, _dev, _np, _seg_sum, galpha_for, seg_graph, seg_lens, seg_of,
                                         seg_rel_err_on)

gpu = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5

#: (in, H, C, concat) of the layer tests
SHAPES = [(21, 1, 64, True), (25, 2, 256, True), (64, 3, 20, True), (32, 5, 3, True), (16, 4, 1, True),
          (64, 3, 20, False), (32, 1, 64, False)]
GRAPHS = ["multigraph", "hub", "n1", "e0", "n0", "golden_rest", "golden_rig"]
#: layer options beside the default (beta=False, bias=True, root_weight=True, relu=False)
VARIANTS = {"default": {}, "noroot": dict(root_weight=False), "noroot_relu": dict(root_weight=False, relu=True),
            "relu": dict(relu=True), "beta": dict(beta=True), "nobias": dict(bias=False),
            "beta_relu_nobias": dict(beta=True, relu=True, bias=False)}
#: the fused epilogue takes H*C = 512 and the mean at C = 64; H*C = 60 (and its mean, C = 20) does not pass
#: ops.gat_heads_fused_ok, so root_weight=False with relu=True runs both routes
VARIANT_SHAPES = [(25, 2, 256, True), (64, 3, 20, True), (64, 3, 20, False), (32, 1, 64, False)]
#: (H, C) of the direct tests: 16-byte forms with a head = 16 / 64 lanes, and one wider than the registers hold; the
#: general form with C = 20 (groups of 32 lanes), 3, 1 and one wider than a wave
DIRECT = [(1, 64), (2, 256), (1, 1100), (3, 20), (5, 3), (4, 1), (2, 70)]


def scale_of(c):
    """float32(1 / sqrt(C)) as a Python float: the factor of the contract, the same number in every evaluation"""
    return float(np.float32(1.0 / np.sqrt(float(c))))


# --------------------------------------------------------------------------- #
# the restatement as a torch module (float32: ref32, .double(): truth64)
# --------------------------------------------------------------------------- #
class RefTransformer(nn.Module):
    def __init__(self, fi, c, heads=1, concat=True, beta=False, bias=True, root_weight=True):
        super().__init__()
        self.fi, self.c, self.heads, self.concat, self.root_weight = fi, c, heads, concat, root_weight
        w = heads * c if concat else c
        self.lin_key = nn.Linear(fi, heads * c)                  # (nn.Linear's default: U(+-1/sqrt(in)), weight and bias)
        self.lin_query = nn.Linear(fi, heads * c)
        self.lin_value = nn.Linear(fi, heads * c)
        self.lin_skip = nn.Linear(fi, w, bias=bias)
        self.lin_beta = nn.Linear(3 * w, 1, bias=False) if beta else None

    def attention(self, x, edge_index):
        """(e [E, H], alpha [E, H], aggregation [N, H, C]) on the edge set exactly as given"""
        n, nh, c = x.size(0), self.heads, self.c
        q = self.lin_query(x).view(n, nh, c)
        k = self.lin_key(x).view(n, nh, c)
        v = self.lin_value(x).view(n, nh, c)
        if k.requires_grad:
            k.retain_grad()                                     # (``key_bias_mass``: the terms of lin_key.bias.grad)
        self.k_rows = k
        j, i = edge_index[0], edge_index[1]
        e = (q[i] * k[j]).sum(-1) * scale_of(c)
        alpha = pyg_ref.segment_softmax(e, i, n)
        return e, alpha, pyg_ref.scatter_sum(alpha.unsqueeze(-1) * v[j], i, n)

    def forward(self, x, edge_index, relu=False):
        n = x.size(0)
        out = self.attention(x, edge_index)[2]
        out = out.reshape(n, self.heads * self.c) if self.concat else out.mean(1)
        if self.root_weight:
            r = self.lin_skip(x)
            if self.lin_beta is not None:
                b = torch.sigmoid(self.lin_beta(torch.cat([out, r, out - r], -1)))
                out = b * r + (1 - b) * out
            else:
                out = out + r
        return torch.relu(out) if relu else out


# --------------------------------------------------------------------------- #
# the per-edge formulas in numpy (dt = np.float32: ref32, np.float64: truth64); q, k, v, gm [N, H*C], per-edge arrays
# [E, H] in destination-sorted order.  Long sums are numpy's pairwise ones, as ``test_gat_edge_kernels._seg_sum``.
# --------------------------------------------------------------------------- #
def _col_sum(a, dt):
    """sum over axis 0 of a 2-D array in dt, pairwise (numpy sums pairwise along the contiguous axis only)"""
    return np.ascontiguousarray(a.T).sum(-1, dtype=dt)


def tc_logits(ptr, other, q, k, nh, dt):
    n, c = len(ptr) - 1, q.shape[1] // nh
    prod = q.astype(dt).reshape(n, nh, c)[seg_of(ptr)] * k.astype(dt).reshape(n, nh, c)[other]
    return prod.sum(-1, dtype=dt) * dt(scale_of(c))


def tc_softmax(ptr, e, dt):
    seg, n = seg_of(ptr), len(ptr) - 1
    out = np.empty_like(e, dtype=dt)
    for h in range(e.shape[1]):
        m = np.full(n, -np.inf, dt)
        np.maximum.at(m, seg, e[:, h].astype(dt))
        ex = np.exp(e[:, h].astype(dt) - m[seg])
        out[:, h] = ex / (_seg_sum(ex, seg, n) + dt(1e-16))[seg]
    return out


def tc_alpha(ptr, other, q, k, nh, dt):
    return tc_softmax(ptr, tc_logits(ptr, other, q, k, nh, dt), dt)


def _by_source(other, n):
    order = np.argsort(other, kind="stable")
    return order, np.searchsorted(other[order], np.arange(n + 1))


def tc_backward(ptr, other, q, k, alpha, galpha, gm, nh, dt):
    """(gl [E, H], g_q, g_k, g_v [N, H*C]) by the formulas of the contract"""
    seg, n = seg_of(ptr), len(ptr) - 1
    c = q.shape[1] // nh
    al, ga = alpha.astype(dt), galpha.astype(dt)
    dot = np.stack([_seg_sum(np.ascontiguousarray((al * ga)[:, h]), seg, n) for h in range(nh)], 1)
    gl = al * (ga - dot[seg]) * dt(scale_of(c))
    empty = np.zeros((0, nh * c), dt)
    tq = (gl[:, :, None] * k.astype(dt).reshape(n, nh, c)[other]).reshape(len(seg), nh * c)
    g_q = np.stack([_col_sum(tq[ptr[i]:ptr[i + 1]], dt) for i in range(n)]) if n else empty
    tk = (gl[:, :, None] * q.astype(dt).reshape(n, nh, c)[seg]).reshape(len(seg), nh * c)
    tv = (al[:, :, None] * gm.astype(dt).reshape(n, nh, c)[seg]).reshape(len(seg), nh * c)
    order, bounds = _by_source(other, n)
    g_k = np.stack([_col_sum(tk[order[bounds[j]:bounds[j + 1]]], dt) for j in range(n)]) if n else empty
    g_v = np.stack([_col_sum(tv[order[bounds[j]:bounds[j + 1]]], dt) for j in range(n)]) if n else empty
    return gl, g_q.astype(dt), g_k.astype(dt), g_v.astype(dt)


def check_row_sums(name, groups, terms, got):
    """``got[r]`` is the float32 sum (per column) of the rows ``groups[r]`` of ``terms`` (float64, each term a float32
    product of two given numbers): within (len + 2) 2^-23 sum |t| of their exact sum, the bound of any summation order
    with the rounding of each term.  Needs no reference: where the row cancels to rounding noise it has no value to
    compare per row - the VALUE is compared on the scale of the whole tensor."""
    for r, idx in enumerate(groups):
        t = terms[idx]
        bound = (len(t) + 2) * 2.0 ** -23 * np.abs(t).sum(0)
        assert (np.abs(got[r] - t.sum(0)) <= bound).all(), (name, r)


def direct_inputs(n, nh, c, seed):
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal((n, nh * c)).astype(np.float32) for _ in range(4))       # q, k, v, gm


def heads_galpha(ptr, nh, seed):
    return np.ascontiguousarray(np.stack([galpha_for(ptr, seed + h) for h in range(nh)], 1))


def in_degrees(n, hub=HUB):
    """LENS - 1 cyclically (0, 1, 6, 7, 8, 14, ... in-edges) and the hub: rows without edges are part of every graph"""
    return seg_lens(n, hub) - 1


def host_adjacency_raw(n, seed, hub=HUB):
    """(ptr, other, dst) by destination of ``seg_graph`` as it is: no self loop added (stable by destination)"""
    deg = in_degrees(n, hub)
    ei = seg_graph(deg + 1, seed)
    order = np.argsort(ei[1], kind="stable")
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(ei[1], minlength=n), out=ptr[1:])
    assert np.array_equal(np.diff(ptr), deg) and (deg == 0).any()
    return ptr, ei[0][order], ei[1][order]


def device_graph_raw(n, seed, hub=HUB):
    deg = in_degrees(n, hub)
    ei = torch.from_numpy(seg_graph(deg + 1, seed)).to(DEV)
    g = GraphIndex(ei, n, self_loops=False, normalize=False, validate=True)
    ptr = _np(g.fwd.ptr).astype(np.int64)
    assert np.array_equal(np.diff(ptr), deg), "the build did not give the prescribed segment lengths"
    return g, ptr, _np(g.fwd.other).astype(np.int64)[:ptr[-1]], deg


# --------------------------------------------------------------------------- #
# the layer cases (shared by the CPU conditioning test and the GPU tests; computed once, never modified)
# --------------------------------------------------------------------------- #
def _graph(kind, seed):
    """(n, edge_index [2, E] int64)"""
    if kind == "multigraph":
        return 300, random_multigraph(300, 2400, seed)          # self loops, duplicates, 30 nodes without in-edges
    if kind == "hub":
        return 300, seg_graph(seg_lens(300, HUB), seed)         # one segment of HUB - 1 edges, in-degree-0 rows
    if kind == "n1":
        return 1, np.zeros((2, 0), np.int64)                    # one node with no edge
    if kind == "e0":
        return 50, np.zeros((2, 0), np.int64)
    if kind == "n0":
        return 0, np.zeros((2, 0), np.int64)
    z = load_golden("graphnet_gat_h32.npz")
    key = "rest" if kind == "golden_rest" else "rig"
    return z[key + "_x"].shape[0], z[key + "_edge_index"].astype(np.int64)


def _ref_run(mod, x, ei, gup, relu, dtype):
    for p in mod.parameters():
        p.grad = None
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    out = mod(xt, torch.from_numpy(ei), relu=relu)
    (out * torch.from_numpy(gup).to(dtype)).sum().backward()
    grads = {n: (None if p.grad is None else p.grad.detach().numpy().copy()) for n, p in mod.named_parameters()}
    return out.detach().numpy(), xt.grad.numpy(), grads, key_bias_mass(mod)


ZERO = "lin_key.bias"


def key_bias_mass(mod):
    """``lin_key.bias.grad = sum_j g_k[j, :]`` is MATHEMATICALLY ZERO: the bias adds <q_i, b> to every logit of segment
    i, which the softmax does not see (sum_j g_k[j] = sum_i q_i sum_{p into i} gl[p] = 0).  What an evaluation returns is
    the rounding noise of that sum, so it has no scale of its own to be compared on; the scale of its terms is
    max_col sum_j |g_k[j, col]| - the sum of the magnitudes, against which the error of any sum is measured.  It is held
    to the same 1e-5 of THAT scale (``key_bias_distance``), like every tensor whose terms do not cancel."""
    g, mod.k_rows = mod.k_rows.grad, None
    return max(float(g.abs().sum(0).max()) if g.numel() else 0.0, 1e-30)


def key_bias_distance(a, b, mass):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) / mass


@functools.lru_cache(maxsize=None)
def layer_case(fi, nh, c, concat, kind, variant):
    """inputs, the reference module and its float32 / float64 results of one layer case"""
    torch.set_num_threads(1)
    opts = dict(VARIANTS[variant])
    relu = opts.pop("relu", False)
    n, ei = _graph(kind, 3)
    rng = np.random.default_rng(fi + nh + c)
    x = rng.standard_normal((n, fi)).astype(np.float32)
    gup = rng.uniform(0.5, 1.5, (n, nh * c if concat else c)).astype(np.float32)
    torch.manual_seed(11)
    cpu = RefTransformer(fi, c, heads=nh, concat=concat, **opts)          # default initialisation
    r32 = _ref_run(cpu, x, ei, gup, relu, torch.float32)
    r64 = _ref_run(copy.deepcopy(cpu).double(), x, ei, gup, relu, torch.float64)
    return dict(n=n, ei=ei, x=x, gup=gup, cpu=cpu, relu=relu, opts=opts, r32=r32, r64=r64)


def _layer_cases():
    cases = [(s, kind, "default") for s in SHAPES for kind in GRAPHS]
    cases += [(s, "multigraph", v) for s in VARIANT_SHAPES for v in VARIANTS if v != "default"]
    return cases


def _pairs(got, r32, r64):
    """(name, got, ref32, truth64) over the output, x.grad and every parameter gradient the reference has"""
    out = [("forward", got[0], r32[0], r64[0]), ("x.grad", got[1], r32[1], r64[1])]
    for name in r32[2]:
        if name == ZERO:
            continue                                            # (mathematically zero: ``key_bias_mass``)
        if r32[2][name] is None:
            assert got[2][name] is None and r64[2][name] is None, name
        else:
            out.append((name + ".grad", got[2][name], r32[2][name], r64[2][name]))
    return out


# --------------------------------------------------------------------------- #
# CPU
# --------------------------------------------------------------------------- #
def test_constructor_parameters_and_state_dict():
    for concat in (True, False):
        for beta in (False, True):
            for bias in (True, False):
                for root in (True, False):
                    if beta and not root:
                        with pytest.raises(ValueError):
                            dc.nn.TransformerConv(21, 64, heads=4, concat=concat, beta=True, bias=bias, root_weight=False)
                        continue
                    conv = dc.nn.TransformerConv(21, 64, heads=4, concat=concat, beta=beta, bias=bias, root_weight=root)
                    w = 256 if concat else 64
                    want = {f"lin_{k}.{p}": s for k in ("key", "query", "value") for p, s in
                            (("weight", (256, 21)), ("bias", (256,)))}
                    want["lin_skip.weight"] = (w, 21)            # exists with root_weight=False too: its use is gated
                    if bias:
                        want["lin_skip.bias"] = (w,)
                    if beta:
                        want["lin_beta.weight"] = (1, 3 * w)
                    assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == want
                    assert (conv.lin_beta is None) == (not beta) and not hasattr(conv, "bias")
                    assert len(list(conv.parameters())) == len(want)
                    assert conv.out_width == w and conv.supports_fused_relu is True
                    assert conv.graph_flags() == dict(self_loops=False, normalize=False)
                    assert all(lin.six_products for lin in (conv.lin_key, conv.lin_query, conv.lin_value, conv.lin_skip))
                    r = repr(conv)
                    assert r.startswith("TransformerConv(") and "21, 64, heads=4" in r
                    assert ("concat=False" in r) == (not concat) and ("beta=True" in r) == beta
                    assert ("root_weight=False" in r) == (not root)
                    ref = RefTransformer(21, 64, heads=4, concat=concat, beta=beta, bias=bias, root_weight=root)
                    assert set(ref.state_dict()) == set(conv.state_dict())
                    conv.load_state_dict(ref.state_dict(), strict=True)
    conv = dc.nn.TransformerConv(21, 64, heads=4, beta=True)
    lin_b, beta_b = float(1 / np.sqrt(21.0)), float(1 / np.sqrt(3 * 256.0))
    seen = []
    for _ in range(3):
        conv.reset_parameters()
        seen.append(conv.lin_key.weight.detach().clone())
        for lin in (conv.lin_key, conv.lin_query, conv.lin_value, conv.lin_skip):
            assert 0.5 * lin_b < float(lin.weight.detach().abs().max()) <= lin_b
            assert 0.5 * lin_b < float(lin.bias.detach().abs().max()) <= lin_b
        assert 0.5 * beta_b < float(conv.lin_beta.weight.detach().abs().max()) <= beta_b
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    one = dc.nn.TransformerConv(21, 64)
    assert one.heads == 1 and one.concat is True and one.beta is False and one.root_weight is True
    assert one.lin_skip.bias is not None
    with pytest.raises(ValueError):
        dc.nn.TransformerConv(21, 64, heads=0)
    for unsupported in (dict(edge_dim=3), dict(dropout=0.1), dict(return_attention_weights=True)):
        with pytest.raises(TypeError):
            dc.nn.TransformerConv(21, 64, **unsupported)         # not supported: absent from the signature
    with pytest.raises(RuntimeError, match="HIP device"):
        conv(torch.zeros(5, 21), torch.zeros(2, 3, dtype=torch.long))
    assert "TransformerConv" in dc.nn.__all__


def test_importable_through_the_torch_geometric_alias():
    import sys
    from deformcontact_amd.pyg_alias import install_as_torch_geometric
    names = ("torch_geometric", "torch_geometric.nn", "torch_geometric.data")
    saved = {k: sys.modules.get(k) for k in names}
    try:
        install_as_torch_geometric(force=True)
        from torch_geometric.nn import TransformerConv
        assert TransformerConv is dc.nn.TransformerConv
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def _entry_calls():
    """name -> call(N, H, C, pointers given?, leading dimension) of every entry of dc_transformer.hip, otherwise valid"""
    L = _lib.lib()
    p = lambda ok: 64 if ok else None                           # any non-null address: rejected calls never touch it
    return {
        "dc_tconv_softmax_fwd": lambda n, h, c, ok, ld: L.dc_tconv_softmax_fwd(
            p(ok), p(ok), p(ok), ld, p(ok), ld, 0.25, p(ok), n, h, c, None),
        "dc_tconv_softmax_bwd": lambda n, h, c, ok, ld: L.dc_tconv_softmax_bwd(
            p(ok), p(ok), p(ok), p(ok), p(ok), ld, 0.25, p(ok), p(ok), ld, n, h, c, None),
        "dc_tconv_source_bwd": lambda n, h, c, ok, ld: L.dc_tconv_source_bwd(
            p(ok), p(ok), p(ok), p(ok), p(ok), p(ok), ld, p(ok), ld, p(ok), ld, p(ok), ld, n, h, c, None),
    }


def test_abi_argument_errors_of_the_tconv_entries_without_gpu():
    """null pointers, negative N, H < 1, C < 1, short leading dimensions: -1 and the entry's name, before any HIP call;
    N = 0 returns 0 with no pointer at all."""
    L = _lib.lib()
    calls = _entry_calls()
    declared = [n for n in _lib.exported_names() if "tconv" in n]
    assert sorted(declared) == sorted(calls)
    for name, call in calls.items():
        assert call(3, 4, 16, False, 64) == -1 and name.encode() in L.dc_last_error() and b"null" in L.dc_last_error(), name
        assert call(-1, 4, 16, True, 64) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, 0, 16, True, 64) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, -2, 16, True, 64) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, 4, 0, True, 64) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, 4, -1, True, 64) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, 1 << 16, 16, True, 1 << 21) == -1 and b"range" in L.dc_last_error(), name
        assert call(3, 4, 16, True, 63) == -1 and name.encode() in L.dc_last_error() and b"leading" in L.dc_last_error(), name
        assert call(3, 4, 16, False, 63) == -1 and b"leading" in L.dc_last_error(), name     # sizes, strides, then nulls
        assert call(0, 4, 16, False, 64) == 0, name              # no row: nothing is read, written or launched
        assert call(0, 4, 16, False, 63) == -1, name
    # outputs that alias an operand
    assert L.dc_tconv_softmax_bwd(64, 64, 64, 64, 128, 64, 0.25, 192, 128, 64, 3, 4, 16, None) == -1
    assert b"alias" in L.dc_last_error()
    assert L.dc_tconv_source_bwd(64, 64, 64, 64, 64, 128, 64, 192, 64, 256, 64, 256, 64, 3, 4, 16, None) == -1
    assert b"alias" in L.dc_last_error()


@pytest.mark.parametrize("nh,c", [(4, 16), (3, 5), (1, 8)])
def test_backward_formulas_against_autograd_on_the_cpu(nh, c):
    """The hand-written backward of the contract (numpy, float64) == torch autograd (float64), rows without edges
    included; and RefTransformer's attention is the same softmax."""
    n = 67
    ptr, other, dst = host_adjacency_raw(n, 5, hub=300)
    deg = np.diff(ptr)
    rng = np.random.default_rng(nh * 100 + c)
    q_t, k_t, v_t = (torch.from_numpy(rng.standard_normal((n, nh * c))).requires_grad_(True) for _ in range(3))
    gup = rng.uniform(0.5, 1.5, (n, nh * c)) * np.where(rng.random((n, 1)) < 0.5, -1.0, 1.0)
    to, tdst = torch.from_numpy(other), torch.from_numpy(dst)
    e = (q_t.view(n, nh, c)[tdst] * k_t.view(n, nh, c)[to]).sum(-1) * scale_of(c)
    al = pyg_ref.segment_softmax(e, tdst, n)
    al.retain_grad()
    e.retain_grad()
    out = pyg_ref.scatter_sum(al.unsqueeze(-1) * v_t.view(n, nh, c)[to], tdst, n).reshape(n, nh * c)
    (out * torch.from_numpy(gup)).sum().backward()
    q, k, v = q_t.detach().numpy(), k_t.detach().numpy(), v_t.detach().numpy()
    seg_err = seg_rel_err_on(ptr)
    a64 = tc_alpha(ptr, other, q, k, nh, np.float64)
    assert max(seg_err(a64[:, h], al.detach().numpy()[:, h]) for h in range(nh)) < 1e-12
    assert (out.detach().numpy()[deg == 0] == 0).all()
    galpha = np.einsum("pkc,pkc->pk", gup.reshape(n, nh, c)[dst], v.reshape(n, nh, c)[other])
    assert rel_err(galpha, al.grad.numpy()) < 1e-12
    gl, g_q, g_k, g_v = tc_backward(ptr, other, q, k, a64, galpha, gup, nh, np.float64)
    assert rel_err(gl, e.grad.numpy() * scale_of(c)) < 1e-10       # gl = ge * scale, ge the gradient of e
    assert rel_err(g_q, q_t.grad.numpy()) < 1e-10 and (g_q[deg == 0] == 0).all()
    assert rel_err(g_k, k_t.grad.numpy()) < 1e-10
    assert rel_err(g_v, v_t.grad.numpy()) < 1e-10
    # the module: the same attention from x through identity-like linears is covered by its own forward
    torch.manual_seed(nh + c)
    mod = RefTransformer(12, c, heads=nh, root_weight=False).double()
    x = torch.from_numpy(rng.standard_normal((n, 12)))
    ei = torch.from_numpy(np.stack([other, dst]))
    qm, km = mod.lin_query(x).detach().numpy(), mod.lin_key(x).detach().numpy()
    e_m, a_m, agg = mod.attention(x, ei)
    assert rel_err(tc_logits(ptr, other, qm, km, nh, np.float64), e_m.detach().numpy()) < 1e-12
    assert max(seg_err(tc_alpha(ptr, other, qm, km, nh, np.float64)[:, h], a_m.detach().numpy()[:, h])
               for h in range(nh)) < 1e-12
    assert rel_err(mod(x, ei).detach().numpy(), agg.reshape(n, nh * c).detach().numpy()) == 0.0


def test_float32_restatement_within_the_bar_of_float64_on_the_layer_inputs():
    """Every layer case of the GPU tests: float32 RefTransformer within 1e-5 of float64, output and every gradient."""
    worst = 0.0
    for (fi, nh, c, concat), kind, variant in _layer_cases():
        case = layer_case(fi, nh, c, concat, kind, variant)
        for name, _, a32, a64 in _pairs(case["r32"], case["r32"], case["r64"]):
            d = rel_err(a32, a64)
            record_parity(f"RefTransformer fp32 vs fp64 {fi}->{nh}x{c} concat={concat} {kind} {variant} {name}", None,
                          e_o=d)
            assert d < TOL, (fi, nh, c, concat, kind, variant, name, d)
            worst = max(worst, d)
        d = key_bias_distance(case["r32"][2][ZERO], case["r64"][2][ZERO], case["r64"][3])
        record_parity(f"RefTransformer fp32 vs fp64 {fi}->{nh}x{c} concat={concat} {kind} {variant} {ZERO}.grad over "
                      "the mass of its terms", None, e_o=d, metric="abs_over_term_mass")
        assert d < TOL and abs(case["r32"][3] / case["r64"][3] - 1) < 1e-3, (fi, nh, c, concat, kind, variant, d)
        # float64 itself returns noise far below its terms: the gradient IS zero
        assert key_bias_distance(case["r64"][2][ZERO], 0.0, case["r64"][3]) < 1e-12
    assert worst < TOL


@pytest.mark.parametrize("nh,c", DIRECT)
def test_float32_restatement_within_the_bar_of_float64_on_the_direct_inputs(nh, c):
    n = 131
    ptr, other, _ = host_adjacency_raw(n, 9 + nh)
    seg_err = seg_rel_err_on(ptr)
    q, k, v, gm = direct_inputs(n, nh, c, 40 + nh + c)
    a32 = tc_alpha(ptr, other, q, k, nh, np.float32)
    a64 = tc_alpha(ptr, other, q, k, nh, np.float64)
    assert a32.dtype == np.float32
    e64 = tc_logits(ptr, other, q, k, nh, np.float64)
    assert 0.5 < float(e64.std()) < 2.0                         # about N(0, 1) after the scale
    galpha = heads_galpha(ptr, nh, 11)
    b32 = tc_backward(ptr, other, q, k, a32, galpha, gm, nh, np.float32)
    b64 = tc_backward(ptr, other, q, k, a32, galpha, gm, nh, np.float64)
    dists = {"alpha": max(seg_err(a32[:, h], a64[:, h]) for h in range(nh)),
             "gl": max(seg_err(b32[0][:, h], b64[0][:, h]) for h in range(nh)),
             "g_q": rel_err(b32[1], b64[1]), "g_k": rel_err(b32[2], b64[2]), "g_v": row_rel_err(b32[3], b64[3])}
    for name, d in dists.items():
        record_parity(f"numpy fp32 vs fp64 {nh}x{c} {name}", None, e_o=d)
        assert d < TOL, (name, d)


# --------------------------------------------------------------------------- #
# GPU: the layer
# --------------------------------------------------------------------------- #
def _device_conv(cpu, fi, nh, c, concat, **opts):
    conv = dc.nn.TransformerConv(fi, c, heads=nh, concat=concat, **opts)
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


def _check_layer(fi, nh, c, concat, kind, variant):
    case = layer_case(fi, nh, c, concat, kind, variant)
    clear_cache()
    conv = _device_conv(case["cpu"], fi, nh, c, concat, **case["opts"])
    og, gxg, gpg = _device_run(conv, case["x"], case["ei"], case["gup"], relu=case["relu"])
    tag = f"TransformerConv {fi}->{nh}x{c} concat={concat} {kind} {variant}"
    got = (_np(og), _np(gxg), {k: (None if v is None else _np(v)) for k, v in gpg.items()})
    assert got[0].shape == case["r32"][0].shape and set(got[2]) == set(case["r32"][2])
    if not case["opts"].get("root_weight", True):
        assert got[2]["lin_skip.weight"] is None                # created, loaded, unused: no gradient (None, not zeros)
        deg = np.bincount(case["ei"][1], minlength=case["n"])
        assert (got[0][deg == 0] == 0).all()                    # the aggregation of a row without in-edges: exactly 0
    for name, a, a32, a64 in _pairs(got, case["r32"], case["r64"]):
        assert_parity(a, a32, a64, TOL, f"{tag} {name}")
    if case["n"]:                                               # (``row_rel_err`` takes at least one row)
        assert_parity(got[0], case["r32"][0], case["r64"][0], TOL, f"{tag} forward per row", metric=row_rel_err)
    d = key_bias_distance(got[2][ZERO], case["r64"][2][ZERO], case["r64"][3])
    record_parity(f"{tag} {ZERO}.grad over the mass of its terms", None, e_h=d, metric="abs_over_term_mass")
    assert d < TOL, (tag, d)


@gpu
@pytest.mark.parametrize("kind", GRAPHS)
@pytest.mark.parametrize("fi,nh,c,concat", SHAPES)
def test_layer_parity(fi, nh, c, concat, kind):
    """forward and the gradients of x and of the weight and bias of all four linears against RefTransformer at 1e-5."""
    _check_layer(fi, nh, c, concat, kind, "default")


@gpu
@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "default"])
@pytest.mark.parametrize("fi,nh,c,concat", VARIANT_SHAPES)
def test_layer_parity_options(fi, nh, c, concat, variant):
    """root_weight=False (lin_skip gradients None; with relu=True the fused epilogue where the width passes), relu=True
    behind the skip, beta=True (lin_beta.weight.grad compared), bias=False."""
    _check_layer(fi, nh, c, concat, "multigraph", variant)


# --------------------------------------------------------------------------- #
# GPU: the entries called directly
# --------------------------------------------------------------------------- #
def _wide(t, pad=12, off=4):
    """``t`` as a column slice of a wider buffer (row stride > width; rows stay 16-byte aligned)"""
    buf = torch.full((t.size(0), t.size(1) + pad), 1e30, device=t.device)
    buf[:, off:off + t.size(1)] = t
    return buf[:, off:off + t.size(1)]


@gpu
@pytest.mark.parametrize("nh,c", DIRECT)
def test_entries_per_edge_and_row(nh, c):
    """in-degrees LENS - 1 (0 included) + the hub: alpha and gl per segment, g_v per row, g_q / g_k on the scale of the
    tensor with every row inside its rounding bound; strided operands and outputs; twice: same bits."""
    n, f = 131, nh * c
    g, ptr, other, deg = device_graph_raw(n, 9 + nh)
    e, cap = int(ptr[-1]), g.capacity
    seg, seg_err = seg_of(ptr), seg_rel_err_on(ptr)
    q, k, v, gm = direct_inputs(n, nh, c, 40 + nh + c)
    tq, tk, tv, tgm = _dev(q), _dev(k), _dev(v), _dev(gm)
    alpha = ops._tconv_softmax_fwd(g, tq, tk, nh, c)
    assert alpha.shape == (max(cap, 1), nh) and (alpha[e:] == 0).all()
    assert torch.equal(alpha, ops._tconv_softmax_fwd(g, tq, tk, nh, c))
    got = _np(alpha)[:e]
    a32 = tc_alpha(ptr, other, q, k, nh, np.float32)
    a64 = tc_alpha(ptr, other, q, k, nh, np.float64)
    assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
    for h in range(nh):
        assert_parity(got[:, h], a32[:, h], a64[:, h], TOL, f"alpha {nh}x{c} head {h}", metric=seg_err)
        sums = _seg_sum(got[:, h].astype(np.float64), seg, n)
        assert np.abs(sums - 1)[deg > 0].max() <= 1e-6 and (sums[deg == 0] == 0).all()
        assert (got[ptr[:-1][deg == 1], h] == 1.0).all()        # a one-edge segment: exactly 1
    # operands in wider buffers (ld > H*C) give the same bits
    wq, wk, wgm = _wide(tq), _wide(tk), _wide(tgm)
    assert torch.equal(alpha, ops._tconv_softmax_fwd(g, wq, wk, nh, c))
    # q = 0: every logit is 0, the weights are 1 / in-degree
    uni = _np(ops._tconv_softmax_fwd(g, torch.zeros_like(tq), tk, nh, c))[:e]
    assert np.abs(uni - (1.0 / deg[seg])[:, None]).max() <= 1e-6
    # backward from the device's alpha
    galpha = heads_galpha(ptr, nh, 11)
    tg = torch.zeros_like(alpha)
    tg[:e] = _dev(galpha)
    runs = []
    for kk, qq, mm in ((tk, tq, tgm), (tk, tq, tgm), (wk, wq, wgm)):
        gl, g_q = ops._tconv_softmax_bwd(g, alpha, tg, kk, nh, c)
        g_k, g_v = ops._tconv_source_bwd(g, alpha, gl, qq, mm, nh, c)
        runs.append((gl, g_q, g_k, g_v))
    for other_run in runs[1:]:
        for a, b in zip(runs[0], other_run):
            assert torch.equal(a, b)
    gl, g_q, g_k, g_v = runs[0]
    assert (gl[e:] == 0).all() and all(torch.isfinite(t).all() for t in runs[0])
    assert (g_q[torch.from_numpy(deg == 0).to(DEV)] == 0).all()  # no edge into the row: exactly 0
    # strided OUTPUTS: the entries called with row strides f + 8 write the same values and nothing beside them
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    ld = f + 8
    o_q, o_k, o_v = (torch.full((n, ld), 7.0, device=DEV) for _ in range(3))
    gl2 = torch.zeros_like(gl)
    _lib.check(L.dc_tconv_softmax_bwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), alpha.data_ptr(), tg.data_ptr(),
                                      tk.data_ptr(), f, ops._tconv_scale(c), gl2.data_ptr(), o_q.data_ptr(), ld, n, nh, c,
                                      st), "dc_tconv_softmax_bwd")
    _lib.check(L.dc_tconv_source_bwd(g.bwd.ptr.data_ptr(), g.bwd.other.data_ptr(), g.bwd_to_fwd().data_ptr(),
                                     alpha.data_ptr(), gl2.data_ptr(), tq.data_ptr(), f, tgm.data_ptr(), f, o_k.data_ptr(),
                                     ld, o_v.data_ptr(), ld, n, nh, c, st), "dc_tconv_source_bwd")
    assert torch.equal(gl2, gl)
    for wide_out, dense in ((o_q, g_q), (o_k, g_k), (o_v, g_v)):
        assert torch.equal(wide_out[:, :f], dense) and (wide_out[:, f:] == 7.0).all()
    # values
    b32 = tc_backward(ptr, other, q, k, got, galpha, gm, nh, np.float32)
    b64 = tc_backward(ptr, other, q, k, got, galpha, gm, nh, np.float64)
    tag = f"{nh}x{c}"
    gl_h = _np(gl)[:e]
    for h in range(nh):
        assert_parity(gl_h[:, h], b32[0][:, h], b64[0][:, h], TOL, f"gl {tag} head {h}", metric=seg_err)
    assert (gl_h[deg[seg] == 1] == 0).all()                     # alpha = 1, dot = galpha: exactly 0
    assert_parity(_np(g_q), b32[1], b64[1], TOL, f"g_q {tag}")
    assert_parity(_np(g_k), b32[2], b64[2], TOL, f"g_k {tag}")
    assert_parity(_np(g_v), b32[3], b64[3], TOL, f"g_v {tag}", metric=row_rel_err)
    gl64 = gl_h.astype(np.float64)[:, :, None]
    tq_terms = (gl64 * k.astype(np.float64).reshape(n, nh, c)[other]).reshape(e, f)
    check_row_sums(f"g_q {tag}", [np.arange(ptr[i], ptr[i + 1]) for i in range(n)], tq_terms, _np(g_q))
    tk_terms = (gl64 * q.astype(np.float64).reshape(n, nh, c)[seg]).reshape(e, f)
    order, bounds = _by_source(other, n)
    check_row_sums(f"g_k {tag}", [order[bounds[j]:bounds[j + 1]] for j in range(n)], tk_terms, _np(g_k))


@gpu
def test_entries_with_no_rows_and_with_no_edges():
    """N = 0: every entry returns 0 without a launch; N > 0 without any edge: nothing in alpha / gl is touched, the row
    gradients are zeros."""
    L = _lib.lib()
    zi = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert L.dc_tconv_softmax_fwd(zi.data_ptr(), zi.data_ptr(), None, 15, None, 15, 0.5, None, 0, 5, 3, None) == 0
    assert L.dc_tconv_softmax_bwd(zi.data_ptr(), zi.data_ptr(), None, None, None, 15, 0.5, None, None, 15, 0, 5, 3,
                                  None) == 0
    assert L.dc_tconv_source_bwd(zi.data_ptr(), zi.data_ptr(), zi.data_ptr(), None, None, None, 15, None, 15, None, 15,
                                 None, 15, 0, 5, 3, None) == 0
    n, nh, c = 37, 5, 3
    g = GraphIndex(torch.zeros((2, 0), dtype=torch.int64, device=DEV), n, self_loops=False, normalize=False)
    q, k, v, gm = (_dev(a) for a in direct_inputs(n, nh, c, 1))
    alpha = ops._tconv_softmax_fwd(g, q, k, nh, c)
    assert alpha.shape == (1, nh) and (alpha == 0).all()
    gl, g_q = ops._tconv_softmax_bwd(g, alpha, torch.zeros_like(alpha), k, nh, c)
    g_k, g_v = ops._tconv_source_bwd(g, alpha, gl, q, gm, nh, c)
    torch.cuda.synchronize()
    assert (gl == 0).all() and all(t.shape == (n, nh * c) and (t == 0).all() for t in (g_q, g_k, g_v))


# --------------------------------------------------------------------------- #
# GPU: bit-for-bit properties, launches, capture
# --------------------------------------------------------------------------- #
def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert set(a[2]) == set(b[2])
    for name in a[2]:
        assert (a[2][name] is None and b[2][name] is None) or torch.equal(a[2][name], b[2][name]), name


@gpu
@pytest.mark.parametrize("opts", [{}, dict(root_weight=False), dict(beta=True)], ids=["skip", "noroot", "beta"])
@pytest.mark.parametrize("fi,nh,c,concat", [(25, 2, 256, True), (64, 3, 20, True), (64, 3, 20, False), (32, 1, 64, False)])
def test_bit_for_bit_relu_deferred_and_repeat(fi, nh, c, concat, opts):
    variant = "noroot" if "root_weight" in opts else ("beta" if opts else "default")
    case = layer_case(fi, nh, c, concat, "hub", "default") if not opts else layer_case(fi, nh, c, concat, "multigraph", variant)
    n, ei, x, gup = case["n"], case["ei"], case["x"], case["gup"]
    clear_cache()
    conv = _device_conv(case["cpu"], fi, nh, c, concat, **opts)
    tei, xg = torch.from_numpy(ei).to(DEV), torch.from_numpy(x).to(DEV)
    plain = ops.resolve(conv(xg, tei)).clone()
    assert plain.shape == (n, conv.out_width)
    want = torch.relu(plain)
    assert (plain < 0).any() and (plain > 0).any()
    assert torch.equal(conv(xg, tei, relu=True), want)
    assert torch.equal(conv(xg, tei, relu=True, next_conv=conv), want)      # next_conv: accepted and ignored
    y = conv(xg, tei)
    assert type(y).__name__ == "DeferredActivation" and y.shape == plain.shape
    assert torch.equal(F.relu(y), want)
    for kw in ({}, {"relu": True}):
        _same(_device_run(conv, x, ei, gup, **kw), _device_run(conv, x, ei, gup, **kw))


@gpu
def test_launches_of_one_layer_step():
    """forward + backward at H = 2: the three kernels of dc_transformer.hip once each, the multi-head aggregation and
    SDDMM of dc_gat_heads.hip, and none of the GAT / GATv2 score kernels."""
    case = layer_case(25, 2, 256, True, "multigraph", "default")
    clear_cache()
    conv = _device_conv(case["cpu"], 25, 2, 256, True)
    _lib.kernel_trace(True)
    _device_run(conv, case["x"], case["ei"], case["gup"])
    counts = _lib.kernel_trace_counts()
    _lib.kernel_trace(False)
    for kname in ("k_tconv_softmax_fwd", "k_tconv_dst_bwd", "k_tconv_src_bwd"):
        assert sum(v for name, v in counts.items() if kname in name) == 1, (kname, counts)
    for kname in ("k_spmm_heads", "k_sddmm_heads"):
        assert sum(v for name, v in counts.items() if kname in name) == 1, (kname, counts)
    assert not any("gatv2" in name or "k_gat_" in name for name in counts), counts


@gpu
def test_strided_input_and_gradient_give_the_same_bits():
    fi, nh, c, concat = 25, 2, 256, True
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
    """forward + backward of two stacked layers on ONE stream under torch.cuda.graph (no host read anywhere); two
    replays with new x in the static input, each bit-identical to the eager run on that input."""
    n, ei = _graph("multigraph", 12)
    fi, nh, c = 32, 4, 16
    torch.manual_seed(3)
    l1 = dc.nn.TransformerConv(fi, c, heads=nh, root_weight=False).to(DEV)
    l2 = dc.nn.TransformerConv(nh * c, c, heads=nh, concat=False, beta=True).to(DEV)
    params = [p for p in list(l1.parameters()) + list(l2.parameters())]
    used = [p for name, p in list(l1.named_parameters()) if not name.startswith("lin_skip")] + list(l2.parameters())
    tei = torch.from_numpy(ei).to(DEV)
    rng = np.random.default_rng(1)
    xs = [torch.from_numpy(rng.standard_normal((n, fi)).astype(np.float32)).to(DEV) for _ in range(3)]
    gup = torch.from_numpy(rng.uniform(0.5, 1.5, (n, c)).astype(np.float32)).to(DEV)
    static_x = xs[0].clone().requires_grad_(True)
    leaves = [static_x] + used
    assert len(params) == len(used) + 2
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
