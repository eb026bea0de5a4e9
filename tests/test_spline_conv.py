"""``SplineConv`` (SplineCNN): the layer, ``ops.spline_aggregate`` and the C entries of dc_spline.hip.

The reference is this file's own restatement of the contract in INTEGRATION.md 1.9 (PyG 2.5.2 spline_conv.py with
torch-spline-conv's basis and weighting): ``RefSpline``, a torch CPU module evaluated in float32 (``ref32``) and float64
(``truth64``) with gradients from torch autograd - ``floor`` detached, the basis polynomials in torch, so autograd yields
the ``edge_attr`` gradient - and numpy formulas for the entries called directly.  ``oracle/pyg_ref`` has no SplineConv.

Inputs, the same everywhere unless a test says otherwise: ``x ~ N(0, 1)``, upstream gradients of magnitude [0.5, 1.5]
with a random sign, ``weight`` and ``lin.weight`` at their initialisation, ``bias ~ N(0, 1)``.  The pseudo-coordinates
stay OFF THE KNOTS: at degree 1 the ``edge_attr`` gradient is discontinuous where ``v = a * (ks - degree * open)`` is an
integer, and a float32 and a float64 evaluation that disagree on ``floor(v)`` are then both right and far apart.  On
``seg`` and ``multigraph`` ``a[:, d] = (cell + U[0.05, 0.95]) / mult_d`` with ``cell`` uniform in ``0..mult_d-1``; on
``golden_rest`` (D = 3) the normalised Cartesian offsets of test_gmm_conv.py with the fraction of ``v`` clamped into
[1e-3, 1 - 1e-3].  A CPU test asserts that the float32 and the float64 ``floor(v)`` agree for every layer input.

Metrics.  The layers through ``helpers.assert_parity`` at 1e-5, output and every gradient (nothing registered
``special``).  The entries: ``dc_spline_fwd`` bit-identical to a numpy float32 loop that walks the device's own ``ptr`` /
``other`` / ``perm`` in p order with the device's own ``b`` / ``wi`` (per edge the message ``t += b * h`` over s in order,
the product rounded first, then ``acc += t``; mean: one division by the degree; ``+ base``; ``max(., 0)``) and within 1e-5
per row of float64 (summed FLAT over the hub's 5,000 x 9 (edge, slot) pairs, as the issue sketched the kernel, the same
operands measured 1.12e-5 there on the MI355X: the rounding error of a sequential float32 sum grows with the root of its
length, and the message-first order keeps that length at the in-degree); ``dc_spline_basis``:
``wi`` equal to the restatement's, ``b`` within 1e-5 of float64; ``dc_spline_bwd_h`` / ``_b`` / ``_a`` within 1e-5 per row
of float64 formulas over the SAME float32 operands; two calls of each: equal bits.

The adjacencies are built WITHOUT self-loop handling: ``seg_graph`` of ``seg_lens`` gives in-degrees 0, 1, 6, ..., 64
and the hub, ``random_multigraph`` keeps its self loops, duplicates and isolated nodes.
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import deformcontact_amd as dc
from deformcontact_amd import _lib, ops
from deformcontact_amd.graph import GraphIndex, clear_cache
from deformcontact_amd.nn import SplineConv  # noqa: F401  (the module needs the layer: no test runs without it)
from tests.helpers import assert_parity, load_golden, random_multigraph, record_parity, rel_err, row_rel_err
from tests.test_gat_edge_kernels import HUB, _dev, _np, seg_graph, seg_lens

gpu = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5

#: (in, M, kernel_size, is_open_spline, degree, dim) of the layer tests; the sixth has S = 64, the cap
SHAPES = [(21, 64, 5, True, 1, 3), (25, 256, (3, 4), (True, False), 2, 2), (16, 1, (4,), True, 3, 1),
          (8, 16, (2, 2, 2, 2), True, 1, 4), (64, 20, 5, False, 1, 3), (4, 8, (4, 4, 4), True, 3, 3),
          (12, 32, (3, 4, 5), (True, False, True), 2, 3)]
AGGRS = ["mean", "add"]
MAIN_GRAPHS = ["seg", "multigraph", "golden_rest"]
EDGE_GRAPHS = ["n1", "e0", "n0"]
#: widths of the direct forward test: the general form (1, 3, 70: lane groups of 4, 4, 64) and the 16-byte form (20, 64,
#: 256: groups of 8, 16, 64); 1100: 64 lanes over five column chunks (one case)
WIDTHS = [1, 3, 20, 64, 70, 256]
#: (kernel_size, D, degree) of the direct forward test, ``open`` mixed per dimension
FWD_GEOMS = [(5, 3, 1), ((3, 4), 2, 2), (4, 1, 3)]
DIRECT_GRAPHS = ["seg", "multigraph"]
#: (M, kernel_size, D, degree) of the direct backward tests
BWD_SHAPES = [(3, (4,), 1, 1), (20, 5, 3, 1), (64, (3, 4), 2, 2), (70, (4, 4, 4), 3, 3), (256, (2, 2), 2, 1)]
MIXED_OPEN = (True, False, True, False)


def geometry(ks, op, degree, dim):
    """(ks, open as 0/1, mult = ks - degree*open) as tuples of ``dim`` ints"""
    ks = tuple(ks) if isinstance(ks, (tuple, list)) else (ks,) * dim
    op = tuple(int(o) for o in op) if isinstance(op, (tuple, list)) else (int(op),) * dim
    assert len(ks) == dim and len(op) == dim
    return ks, op, tuple(k - degree * o for k, o in zip(ks, op))


# --------------------------------------------------------------------------- #
# the contract's polynomials, for numpy and torch alike (``xp.where``); f [E, 1], k [1, S]
# --------------------------------------------------------------------------- #
def bspline(xp, degree, f, k):
    if degree == 1:
        return 1 - f - k + 2 * f * k
    if degree == 2:
        return xp.where(k == 0, 0.5 * f * f - f + 0.5, xp.where(k == 1, -f * f + f + 0.5, 0.5 * f * f + 0 * k))
    return xp.where(k == 0, (1 - f) ** 3 / 6, xp.where(k == 1, (3 * f ** 3 - 6 * f * f + 4) / 6, xp.where(
        k == 2, (-3 * f ** 3 + 3 * f * f + 3 * f + 1) / 6, f ** 3 / 6 + 0 * k)))


def bspline_d(xp, degree, f, k):
    if degree == 1:
        return 2.0 * k - 1 + 0 * f
    if degree == 2:
        return xp.where(k == 0, f - 1, xp.where(k == 1, -2 * f + 1, f + 0 * k))
    return xp.where(k == 0, (-f * f + 2 * f - 1) / 2, xp.where(k == 1, (3 * f * f - 4 * f) / 2, xp.where(
        k == 2, (-3 * f * f + 2 * f + 1) / 2, f * f / 2 + 0 * k)))


def slot_digits(degree, dim):
    """k_mod [D, S] int64: digit d of slot s in base degree+1, dimension 0 running fastest"""
    s = np.arange((degree + 1) ** dim)
    return np.stack([(s // (degree + 1) ** d) % (degree + 1) for d in range(dim)])


def basis_np(a, ks, mult, degree, dtype):
    """(b [E, S] ``dtype``, wi [E, S] int64, f [E, D] ``dtype``, floor [E, D]) with every operation in ``dtype``"""
    a = np.asarray(a, dtype).reshape(len(a), -1)
    dim = a.shape[1]
    km = slot_digits(degree, dim)
    b = np.ones((a.shape[0], km.shape[1]), dtype)
    wi = np.zeros(b.shape, np.int64)
    off, fs, fls = 1, [], []
    for d in range(dim):
        v = a[:, d] * dtype(mult[d])
        fl = np.floor(v)
        f = (v - fl).astype(dtype)
        wi += ((fl.astype(np.int64)[:, None] + km[d][None]) % ks[d]) * off
        off *= ks[d]
        b = (b * bspline(np, degree, f[:, None], km[d][None].astype(dtype))).astype(dtype)
        fs.append(f)
        fls.append(fl)
    return b, wi, np.stack(fs, 1), np.stack(fls, 1)


# --------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------- #
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


def signed(rng, shape):
    """magnitudes in [0.5, 1.5], random sign"""
    return (rng.uniform(0.5, 1.5, shape) * np.where(rng.random(shape) < 0.5, -1.0, 1.0)).astype(np.float32)


def pseudo(rng, kind, ei, mult):
    """edge_attr [E, D] in [0, 1] off the knots of ``v = a * mult``: on ``golden_rest`` (D = 3) the normalised Cartesian
    offsets with the fraction of v clamped into [1e-3, 1 - 1e-3], else ``(cell + U[0.05, 0.95]) / mult``"""
    ne, m = ei.shape[1], np.asarray(mult, np.float64)
    assert (m >= 1).all()
    if kind == "golden_rest":
        assert len(mult) == 3
        pos = load_golden("graphnet_gat_h32.npz")["rest_pos"].astype(np.float64)
        cart = pos[ei[0]] - pos[ei[1]]
        v = (cart / (2 * np.abs(cart).max()) + 0.5) * m
        fl = np.clip(np.floor(v), 0, m - 1)
        return ((fl + np.clip(v - fl, 1e-3, 1 - 1e-3)) / m).astype(np.float32)
    cell = np.stack([rng.integers(0, int(t), ne) for t in mult], 1)
    return ((cell + rng.uniform(0.05, 0.95, (ne, len(mult)))) / m).astype(np.float32)


def _index_add(n, idx, terms):
    return torch.zeros((n, terms.shape[1]), dtype=torch.float64).index_add_(
        0, torch.from_numpy(idx), torch.from_numpy(np.ascontiguousarray(terms, np.float64))).numpy()


# --------------------------------------------------------------------------- #
# the restatement as a torch module (float32: ref32, .double(): truth64)
# --------------------------------------------------------------------------- #
class RefSpline(nn.Module):
    def __init__(self, fi, m, dim, kernel_size, is_open_spline=True, degree=1, aggr="mean", root_weight=True, bias=True):
        super().__init__()
        self.ks, self.op, self.mult = geometry(kernel_size, is_open_spline, degree, dim)
        self.m, self.dim, self.degree, self.aggr = m, dim, degree, aggr
        self.k = int(np.prod(self.ks))
        self.register_buffer("kernel_size", torch.tensor(self.ks, dtype=torch.long))
        self.register_buffer("is_open_spline", torch.tensor(self.op, dtype=torch.uint8))
        self.weight = nn.Parameter(torch.empty(self.k, fi, m))
        nn.init.uniform_(self.weight, -(self.k * fi) ** -0.5, (self.k * fi) ** -0.5)
        if root_weight:
            self.lin = nn.Linear(fi, m, bias=False)
            nn.init.uniform_(self.lin.weight, -fi ** -0.5, fi ** -0.5)
        if bias:
            self.bias = nn.Parameter(torch.zeros(m))

    def basis(self, a):
        """(b [E, S] in the dtype of ``a``, wi [E, S] int64): the contract's walk over the dimensions"""
        km = torch.from_numpy(slot_digits(self.degree, self.dim))
        b = torch.ones((a.size(0), km.size(1)), dtype=a.dtype)
        wi = torch.zeros(b.shape, dtype=torch.long)
        off = 1
        for d in range(self.dim):
            v = a[:, d] * float(self.mult[d])
            fl = v.detach().floor()
            wi = wi + torch.remainder(fl.long().unsqueeze(1) + km[d].unsqueeze(0), self.ks[d]) * off
            off *= self.ks[d]
            b = b * bspline(torch, self.degree, (v - fl).unsqueeze(1), km[d].unsqueeze(0).to(a.dtype))
        return b, wi

    def forward(self, x, edge_index, edge_attr):
        j, i = edge_index
        if edge_attr.dim() == 1:
            edge_attr = edge_attr.unsqueeze(-1)
        n = x.size(0)
        b, wi = self.basis(edge_attr)
        h = torch.einsum("ni,kim->nkm", x, self.weight)          # x_j @ weight[k] for every k
        msg = (h[j.unsqueeze(1), wi] * b.unsqueeze(-1)).sum(dim=1)
        s = torch.zeros((n, self.m), dtype=x.dtype).index_add_(0, i, msg)
        if self.aggr == "mean":
            s = s / torch.bincount(i, minlength=n).clamp(min=1).to(x.dtype).unsqueeze(-1)
        if hasattr(self, "lin"):
            s = s + self.lin(x)
        return s + self.bias if hasattr(self, "bias") else s


def _ref_run(mod, x, ei, ea, gup, dtype):
    for p in mod.parameters():
        p.grad = None
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    et = torch.from_numpy(ea).to(dtype).requires_grad_(True)
    out = mod(xt, torch.from_numpy(ei), et)
    (out * torch.from_numpy(gup).to(dtype)).sum().backward()
    grads = {"x": xt.grad.numpy(), "edge_attr": (et.grad if et.grad is not None else torch.zeros_like(et)).numpy()}
    grads.update({name: p.grad.detach().numpy().copy() for name, p in mod.named_parameters()})
    return out.detach().numpy(), grads


@functools.lru_cache(maxsize=None)
def spline_case(shape, aggr, kind, root_weight=True, bias=True, flat=False):
    """inputs, the reference module and its float32 / float64 results of one layer case (computed once, never modified);
    ``flat``: D = 1 with ``edge_attr`` of shape [E]"""
    torch.set_num_threads(1)
    fi, m, ks, op, degree, dim = shape
    n, ei = _graph(kind, 3)
    rng = np.random.default_rng(2000 + fi + m + 7 * degree + dim)
    torch.manual_seed(12)
    cpu = RefSpline(fi, m, dim, ks, op, degree, aggr, root_weight, bias)
    if bias:
        with torch.no_grad():
            cpu.bias.copy_(torch.from_numpy(rng.standard_normal(m).astype(np.float32)))
    x = rng.standard_normal((n, fi)).astype(np.float32)
    ea = pseudo(rng, kind, ei, cpu.mult)
    if flat:
        ea = ea[:, 0].copy()
    gup = signed(rng, (n, m))
    r32 = _ref_run(cpu, x, ei, ea, gup, torch.float32)
    r64 = _ref_run(copy.deepcopy(cpu).double(), x, ei, ea, gup, torch.float64)
    return dict(n=n, ei=ei, x=x, ea=ea, gup=gup, cpu=cpu, aggr=aggr, root_weight=root_weight, bias=bias, r32=r32, r64=r64,
                shape=shape)


def _layer_cases():
    return [(s, aggr, kind) for s in SHAPES for aggr in AGGRS for kind in MAIN_GRAPHS
            if kind != "golden_rest" or s[5] == 3]


def _tag(shape):
    fi, m, ks, op, degree, dim = shape
    return f"{fi}->{m} ks={ks} open={op} degree={degree} D={dim}"


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
            print(f"{tag} {name}: vs fp32 {rel_err(a, a32):.3e}, vs float64 {rel_err(a, a64):.3e} "
                  f"(fp32 restatement {rel_err(a32, a64):.3e})")
            assert_parity(a, a32, a64, TOL, f"{tag} {name}")


# --------------------------------------------------------------------------- #
# CPU
# --------------------------------------------------------------------------- #
def _shapes(mod):
    return {k: (tuple(v.shape), v.dtype) for k, v in mod.state_dict().items()}


def test_surface_and_alias():
    import sys
    from deformcontact_amd.pyg_alias import install_as_torch_geometric
    names = dc.nn.__all__
    assert "SplineConv" in names and names[-1] == "ChebConv"
    assert names.index("SplineConv") == names.index("GMMConv") - 1 == len(names) - 3
    assert (ops.SPLINE_MAX_D, ops.SPLINE_MAX_S, ops.SPLINE_MAX_K) == (4, 64, 1024)
    mods = ("torch_geometric", "torch_geometric.nn", "torch_geometric.data")
    saved = {k: sys.modules.get(k) for k in mods}
    try:
        install_as_torch_geometric(force=True)
        from torch_geometric.nn import SplineConv as alias
        assert alias is dc.nn.SplineConv
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_constructor_parameters_state_dict_and_repr():
    f32 = torch.float32
    for root_weight in (True, False):
        for bias in (True, False):
            conv = dc.nn.SplineConv(21, 64, dim=3, kernel_size=[3, 4, 5], is_open_spline=[True, False, True], degree=2,
                                    root_weight=root_weight, bias=bias)
            want = {"weight": ((60, 21, 64), f32), "kernel_size": ((3,), torch.int64), "is_open_spline": ((3,), torch.uint8)}
            if root_weight:
                want["lin.weight"] = ((64, 21), f32)
            if bias:
                want["bias"] = ((64,), f32)
            assert _shapes(conv) == want
            assert set(dict(conv.named_parameters())) == set(want) - {"kernel_size", "is_open_spline"}
            ref = RefSpline(21, 64, 3, [3, 4, 5], [True, False, True], 2, "mean", root_weight, bias)
            assert _shapes(ref) == want
            conv.load_state_dict(ref.state_dict(), strict=True)
            ref.load_state_dict(conv.state_dict(), strict=True)
            assert torch.equal(conv.weight, ref.weight)
            assert conv.kernel_size.tolist() == [3, 4, 5] and conv.is_open_spline.tolist() == [1, 0, 1]
            assert (conv.lin is None) == (not root_weight) and (conv.bias is None) == (not bias)
    conv = dc.nn.SplineConv(21, 64, 3, 5)                          # dim and kernel_size positional, as in PyG
    assert (conv.dim, conv.degree, conv.aggr) == (3, 1, "mean")
    assert conv.kernel_size.tolist() == [5, 5, 5] and conv.is_open_spline.tolist() == [1, 1, 1]
    assert conv.weight.shape == (125, 21, 64)
    assert conv.graph_flags() == dict(self_loops=False, normalize=False) and conv.supports_fused_relu
    assert repr(conv) == "SplineConv(21, 64, dim=3)"
    assert dc.nn.SplineConv(4, 4, 2, 3, aggr="add").aggr == "add"


def test_initialisation_bounds_and_reset_parameters():
    torch.manual_seed(0)
    conv = dc.nn.SplineConv(40, 48, dim=2, kernel_size=[3, 4])
    for p, a in ((conv.weight, (12 * 40) ** -0.5), (conv.lin.weight, 40 ** -0.5)):
        top = float(p.detach().abs().max())
        assert 0.97 * a < top <= a and abs(float(p.detach().mean())) < 0.05 * a
    assert (conv.bias == 0).all()
    with torch.no_grad():
        before = {name: p.detach().clone() for name, p in conv.named_parameters()}
        conv.bias.fill_(3.0)
    conv.reset_parameters()
    assert (conv.bias == 0).all()
    assert not torch.equal(conv.weight, before["weight"]) and not torch.equal(conv.lin.weight, before["lin.weight"])
    assert float(conv.weight.detach().abs().max()) <= (12 * 40) ** -0.5
    assert conv.kernel_size.tolist() == [3, 4]


def test_errors_raised_on_the_host():
    C = dc.nn.SplineConv
    with pytest.raises(NotImplementedError, match="bipartite"):
        C((4, 4), 4, 2, 3)
    with pytest.raises(NotImplementedError, match="max"):
        C(4, 4, 2, 3, aggr="max")
    for bad in ("min", "sum", "softmax", None, ["mean"]):
        with pytest.raises(ValueError, match="aggr"):
            C(4, 4, 2, 3, aggr=bad)
    for lazy in (-1, 0):
        with pytest.raises(NotImplementedError, match="lazy"):
            C(lazy, 4, 2, 3)
    for degree in (0, 4, 1.0, True):
        with pytest.raises(ValueError, match="degree"):
            C(4, 4, 2, 3, degree=degree)
    with pytest.raises(ValueError, match="entries"):
        C(4, 4, 3, [3, 4])
    with pytest.raises(ValueError, match="entries"):
        C(4, 4, 2, 3, is_open_spline=[True, False, True])
    # the caps: a breach is a ValueError, the cap itself is accepted
    for dim in (0, 5):
        with pytest.raises(ValueError, match="dim"):
            C(4, 4, dim, 2)
    for degree in (2, 3):
        with pytest.raises(ValueError, match="slots"):
            C(4, 4, 4, 2, degree=degree)                         # 81 and 256 slots
    with pytest.raises(ValueError, match=">= 1"):
        C(4, 4, 2, [3, 0])
    with pytest.raises(ValueError, match="1024"):
        C(4, 4, 2, [32, 33])
    assert C(4, 4, 4, 2).weight.shape == (16, 4, 4)                                  # dim = 4
    assert C(2, 2, 3, [4, 4, 4], degree=3).weight.shape == (64, 2, 2)                # S = 64
    assert C(1, 1, 2, [32, 32]).weight.shape == (1024, 1, 1)                         # K = 1024
    assert C(2, 2, 2, [1, 1], degree=3).weight.shape == (1, 2, 2)                    # ks = 1
    x, ei = torch.zeros(5, 4), torch.zeros(2, 3, dtype=torch.long)
    conv, one = C(4, 2, 3, 2), C(4, 2, 1, 2)
    with pytest.raises(NotImplementedError, match="bipartite"):
        conv((x, x), ei, torch.zeros(3, 3))
    with pytest.raises(NotImplementedError, match="bf16"):
        conv(x.bfloat16(), ei, torch.zeros(3, 3))
    with pytest.raises(ValueError, match="edge_attr"):
        conv(x, ei)
    for bad in (3, "mean", [1.0, 2.0], np.zeros((3, 3), np.float32), True):
        with pytest.raises(TypeError, match="edge_attr"):
            conv(x, ei, bad)
    with pytest.raises(ValueError, match="rows"):
        conv(x, ei, torch.zeros(4, 3))
    with pytest.raises(ValueError):
        conv(x, ei, torch.zeros(3, 2))                           # dim = 3, width 2
    with pytest.raises(ValueError):
        conv(x, ei, torch.zeros(3))                              # [E] only where dim is 1
    with pytest.raises(ValueError, match="float32"):
        conv(x, ei, torch.zeros(3, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="contiguous"):
        conv(x, ei, torch.zeros(3, 6)[:, ::2])
    for layer, ea in ((conv, torch.zeros(3, 3)), (one, torch.zeros(3)), (one, torch.zeros(3, 1))):
        for kw in (dict(), dict(relu=True)):
            with pytest.raises(RuntimeError, match="HIP device"):
                layer(x, ei, ea, **kw)                           # every host check passed: no CPU path


def test_host_checks_of_spline_aggregate():
    h, ea = torch.zeros(5, 16), torch.zeros(3, 3)                 # K = 8, M = 2
    agg = ops.spline_aggregate
    with pytest.raises(ValueError, match="reduce"):
        agg(None, h, ea, [2, 2, 2], [1, 1, 1], 1, reduce="max")
    with pytest.raises(ValueError, match="degree"):
        agg(None, h, ea, [2, 2, 2], [1, 1, 1], 4)
    with pytest.raises(ValueError, match="entries"):
        agg(None, h, ea, [2, 2, 2], [1, 1], 1)
    with pytest.raises(ValueError, match="dim"):
        agg(None, h, torch.zeros(3, 5), [2] * 5, [1] * 5, 1)
    with pytest.raises(ValueError, match="slots"):
        agg(None, h, torch.zeros(3, 4), [2] * 4, [1] * 4, 2)
    with pytest.raises(ValueError, match=">= 1"):
        agg(None, h, ea, [2, 0, 2], [1, 1, 1], 1)
    with pytest.raises(ValueError, match="1024"):
        agg(None, h, ea, [16, 16, 16], [1, 1, 1], 1)
    with pytest.raises(ValueError, match=r"K\*M"):
        agg(None, torch.zeros(5, 7), ea, [2, 2, 2], [1, 1, 1], 1)       # 7 columns are no multiple of K = 8
    with pytest.raises(ValueError, match=r"K\*M"):
        agg(None, h.double(), ea, [2, 2, 2], [1, 1, 1], 1)
    with pytest.raises(ValueError, match="edge_attr"):
        agg(None, h, torch.zeros(3, 2), [2, 2, 2], [1, 1, 1], 1)
    with pytest.raises(ValueError, match="edge_attr"):
        agg(None, h, ea.double(), [2, 2, 2], [1, 1, 1], 1)
    with pytest.raises(ValueError, match="base"):
        agg(None, h, ea, [2, 2, 2], [1, 1, 1], 1, base=torch.zeros(5, 16))
    with pytest.raises(ValueError, match="relu"):
        agg(None, h, ea, [2, 2, 2], [1, 1, 1], 1, relu=True)             # M = 2: no width of the mask pass
    with pytest.raises(TypeError, match="edge_attr"):
        agg(None, h, 0.5, [2, 2, 2], [1, 1, 1], 1)
    # E*S and N*K*M must stay below 2^31 (shapes only: expanded tensors own no such memory)
    with pytest.raises(ValueError, match=r"E\*S"):
        agg(None, h, torch.zeros(1, 3).expand(1 << 28, 3), [2, 2, 2], [1, 1, 1], 1)
    with pytest.raises(ValueError, match=r"N\*K\*M"):
        agg(None, torch.zeros(1, 16).expand(1 << 27, 16), ea, [2, 2, 2], [1, 1, 1], 1)
    with pytest.raises(RuntimeError, match="HIP device"):
        agg(None, h, ea, [2, 2, 2], [1, 1, 1], 1)                        # every host check passed: no CPU path
    with pytest.raises(RuntimeError, match="HIP device"):
        agg(None, h, ea, 2, True, 1)                                     # an int and a bool: repeated D times


I64x4 = ctypes.c_int64 * 4
I32x4 = ctypes.c_int32 * 4


def _entry_calls(ks=(3, 4, 1, 1), op=(1, 0, 1, 1)):
    """name -> call(rows, M, D, degree, S, K, pointers given?, leading dimension) of every entry of dc_spline.hip,
    otherwise valid; the host arrays ``ks`` / ``open`` are real, the device addresses are never touched by a rejected
    call"""
    L = _lib.lib()
    p = lambda ok, at=64: at if ok else None                     # any non-null address: rejected calls never touch it
    hk, ho = I64x4(*ks), I32x4(*op)
    host = lambda ok, arr: arr if ok else None
    return {
        "dc_spline_basis": lambda r, m, d, deg, s, k, ok, ld: L.dc_spline_basis(
            p(ok), min(ld, d), host(ok, hk), host(ok, ho), deg, p(ok, 128), p(ok, 192), r, d, None),
        "dc_spline_fwd": lambda r, m, d, deg, s, k, ok, ld: L.dc_spline_fwd(
            p(ok), p(ok), p(ok), p(ok), p(ok, 320), p(ok, 192), ld * k, None, 0, 1, 0, p(ok, 128), ld, r,
            5 if r > 0 else 0, s, k, m, None),
        "dc_spline_bwd_h": lambda r, m, d, deg, s, k, ok, ld: L.dc_spline_bwd_h(
            p(ok), p(ok), p(ok), p(ok), p(ok), p(ok, 320), p(ok, 192), ld, p(ok, 128), ld * k, r, 5 if r > 0 else 0, s, k,
            m, None),
        "dc_spline_bwd_b": lambda r, m, d, deg, s, k, ok, ld: L.dc_spline_bwd_b(
            p(ok), p(ok), p(ok), p(ok, 320), p(ok, 192), ld * k, p(ok, 256), ld, p(ok, 128), 3, r, s, k, m, None),
        "dc_spline_bwd_a": lambda r, m, d, deg, s, k, ok, ld: L.dc_spline_bwd_a(
            p(ok), p(ok, 192), min(ld, d), host(ok, hk), host(ok, ho), deg, p(ok, 128), min(ld, d), r, d, None),
    }


def test_abi_argument_errors_of_the_spline_entries_without_gpu():
    """null pointers, negative sizes, D / S / K / degree out of range, a ks entry < 1, short leading dimensions, aliased
    outputs, E*S and N*K*M overflow: -1, the entry's name and the cause, before any HIP call; no row (no edge) returns 0
    with no pointer at all.  EVERY call below is rejected or returns before a launch: none may be valid."""
    L = _lib.lib()
    calls = _entry_calls()
    geom = ("dc_spline_basis", "dc_spline_bwd_a")               # the entries that take D, degree, ks, open
    assert sorted(n for n in _lib.exported_names() if "spline" in n) == sorted(calls)
    err = lambda: L.dc_last_error()
    for name, call in calls.items():
        tag = name.encode()
        # (rows, M, D, degree, S, K): D = 2, degree = 2 -> S = 9, ks = (3, 4) -> K = 12
        assert call(3, 16, 2, 2, 9, 12, False, 64) == -1 and tag in err() and b"null" in err(), name
        assert call(-1, 16, 2, 2, 9, 12, True, 64) == -1 and tag in err(), name
        assert call(0, 16, 2, 2, 9, 12, False, 64) == 0, name     # no row / no edge: nothing is read, written or launched
        assert call(3, 16, 2, 2, 9, 12, True, 1 if name in geom else 15) == -1 and tag in err() and b"leading" in err(), name
        if name in geom:
            for d in (0, 5):
                assert call(3, 16, d, 1, 0, 0, True, 64) == -1 and tag in err() and b"D" in err(), (name, d)
            for deg in (0, 4):
                assert call(3, 16, 2, deg, 0, 0, True, 64) == -1 and tag in err() and b"degree" in err(), (name, deg)
            assert call(3, 16, 4, 3, 0, 0, True, 64) == -1 and tag in err() and b"S =" in err(), name       # S = 256
            assert call(1 << 28, 16, 2, 2, 0, 0, True, 64) == -1 and tag in err() and b"E out of range" in err(), name
        else:
            assert call(3, 0, 2, 2, 9, 12, True, 64) == -1 and tag in err(), name
            for s in (0, 65):
                assert call(3, 16, 2, 2, s, 12, True, 64) == -1 and tag in err() and b"S" in err(), (name, s)
            for k in (0, 1025):
                assert call(3, 16, 2, 2, 9, k, True, 64) == -1 and tag in err() and b"K" in err(), (name, k)
            assert call(3, 1 << 24, 2, 2, 9, 12, True, 1 << 24) == -1 and b"range" in err(), name
    # a ks entry < 1, and K = prod ks above the cap (the host arrays are read, the device addresses are not)
    for name in geom:
        bad = _entry_calls(ks=(3, 0, 1, 1))[name]
        assert bad(3, 16, 2, 2, 9, 12, True, 64) == -1 and name.encode() in err() and b"ks[" in err(), name
        big = _entry_calls(ks=(33, 32, 1, 1))[name]
        assert big(3, 16, 2, 2, 9, 12, True, 64) == -1 and name.encode() in err() and b"K =" in err(), name
    # E*S and N*K*M must stay below 2^31
    hk, ho = I64x4(3, 4, 1, 1), I32x4(1, 0, 1, 1)
    assert L.dc_spline_basis(64, 3, hk, ho, 3, 128, 192, 1 << 26, 3, None) == -1 and b"E out of range" in err()
    assert L.dc_spline_bwd_a(64, 192, 3, hk, ho, 3, 128, 3, 1 << 26, 3, None) == -1 and b"E out of range" in err()
    assert L.dc_spline_fwd(64, 64, 64, 64, 320, 192, 12 * 16, None, 0, 1, 0, 128, 16, 3, 1 << 28, 9, 12, 16, None) == -1
    assert b"E out of range" in err()
    assert L.dc_spline_bwd_h(64, 64, 64, 64, 64, 320, 192, 16, 128, 12 * 16, 3, 1 << 28, 9, 12, 16, None) == -1
    assert b"E out of range" in err()
    assert L.dc_spline_bwd_b(64, 64, 64, 320, 192, 12 * 16, 256, 16, 128, 3, 1 << 28, 9, 12, 16, None) == -1
    assert b"E out of range" in err()
    n, k, m = 1 << 17, 1024, 16                                  # N*K*M = 2^31
    assert L.dc_spline_fwd(64, 64, 64, 64, 320, 192, k * m, None, 0, 1, 0, 128, m, n, 5, 9, k, m, None) == -1
    assert b"dc_spline_fwd" in err() and b"range" in err()
    assert L.dc_spline_bwd_h(64, 64, 64, 64, 64, 320, 192, m, 128, k * m, n, 5, 9, k, m, None) == -1
    assert b"dc_spline_bwd_h" in err() and b"range" in err()
    assert L.dc_spline_bwd_b(64, 64, 64, 320, 192, k * m, 256, m, 128, n, 5, 9, k, m, None) == -1
    assert b"dc_spline_bwd_b" in err() and b"range" in err()
    # outputs that alias an operand
    assert L.dc_spline_basis(64, 2, hk, ho, 2, 64, 192, 5, 2, None) == -1 and b"alias" in err()
    assert L.dc_spline_basis(64, 2, hk, ho, 2, 128, 128, 5, 2, None) == -1 and b"alias" in err()
    assert L.dc_spline_fwd(64, 64, 64, 64, 320, 192, 192, None, 0, 1, 0, 192, 16, 3, 5, 9, 12, 16, None) == -1 and b"alias" in err()
    assert L.dc_spline_fwd(64, 64, 64, 64, 320, 192, 192, None, 0, 1, 0, 320, 16, 3, 5, 9, 12, 16, None) == -1 and b"alias" in err()
    assert L.dc_spline_fwd(64, 64, 64, 64, 320, 192, 192, 128, 16, 1, 0, 128, 16, 3, 5, 9, 12, 16, None) == -1 and b"alias" in err()
    assert L.dc_spline_bwd_h(64, 64, 64, 64, 64, 320, 192, 16, 192, 192, 3, 5, 9, 12, 16, None) == -1 and b"alias" in err()
    assert L.dc_spline_bwd_h(64, 64, 64, 64, 64, 320, 192, 16, 320, 192, 3, 5, 9, 12, 16, None) == -1 and b"alias" in err()
    assert L.dc_spline_bwd_b(64, 64, 64, 320, 192, 192, 256, 16, 256, 3, 5, 9, 12, 16, None) == -1 and b"alias" in err()
    assert L.dc_spline_bwd_b(64, 64, 64, 320, 192, 192, 256, 16, 320, 3, 5, 9, 12, 16, None) == -1 and b"alias" in err()
    assert L.dc_spline_bwd_a(64, 192, 2, hk, ho, 2, 192, 2, 5, 2, None) == -1 and b"alias" in err()
    assert L.dc_spline_bwd_a(64, 192, 2, hk, ho, 2, 64, 2, 5, 2, None) == -1 and b"alias" in err()


def test_partition_of_unity_and_index_range_of_the_restatement():
    """sum_s b = 1 within 1e-6 for each degree (float32 and float64), every index in [0, K), and the numpy walk of the
    direct tests equals the torch one"""
    rng = np.random.default_rng(5)
    for degree in (1, 2, 3):
        for dim in (1, 2, 3):
            ks, op = (3, 4, 5)[:dim], MIXED_OPEN[:dim]
            ref = RefSpline(2, 2, dim, ks, op, degree)
            a = rng.uniform(0, 1, (500, dim)).astype(np.float32)
            for dtype, npt in ((torch.float32, np.float32), (torch.float64, np.float64)):
                b, wi = ref.basis(torch.from_numpy(a).to(dtype))
                assert b.shape == (500, (degree + 1) ** dim) and float((b.sum(1) - 1).abs().max()) < 1e-6
                assert int(wi.min()) >= 0 and int(wi.max()) < ref.k
                bn, win, _, _ = basis_np(a, ref.ks, ref.mult, degree, npt)
                assert np.array_equal(win, wi.numpy()) and rel_err(bn, b.numpy()) < (1e-6 if npt is np.float32 else 1e-14)
            assert float(b.min()) >= 0.0


def test_float32_and_float64_agree_on_floor_for_every_layer_input():
    """the draw keeps v = a * mult off the knots: both precisions pick the same cell, with a margin"""
    for shape, aggr, kind in _layer_cases():
        case = spline_case(shape, aggr, kind)
        mult = case["cpu"].mult
        ea = case["ea"]
        assert ea.min() >= 0.0 and ea.max() <= 1.0
        _, w32, f32, fl32 = basis_np(ea, case["cpu"].ks, mult, shape[4], np.float32)
        _, w64, f64, fl64 = basis_np(ea, case["cpu"].ks, mult, shape[4], np.float64)
        assert np.array_equal(fl32, fl64) and np.array_equal(w32, w64), (shape, kind)
        assert f64.min() > 5e-4 and f64.max() < 1 - 5e-4, (shape, kind, f64.min(), f64.max())


def test_float32_restatement_within_the_bar_of_float64_on_the_layer_inputs():
    """Every layer case of the GPU tests: the float32 restatement within 1e-5 of float64, output and every gradient"""
    for shape, aggr, kind in _layer_cases():
        case = spline_case(shape, aggr, kind)
        check_against_references(f"RefSpline fp32 vs fp64 {_tag(shape)} {aggr} {kind}", case["r32"], case, "e_o")
        assert set(case["r32"][1]) == {"x", "edge_attr", "weight", "lin.weight", "bias"}


def test_backward_formulas_of_the_direct_tests_agree_with_autograd():
    """the hand-written float64 formulas the entries are held against equal torch autograd through ``RefSpline``"""
    for m, ks, dim, degree in BWD_SHAPES[:4]:
        for aggr in AGGRS:
            case = bwd_case("multigraph", m, ks, dim, degree)
            n, ei, k = case["n"], case["ei"], case["K"]
            ref = RefSpline(5, m, dim, ks, MIXED_OPEN[:dim], degree, aggr, root_weight=False, bias=False).double()
            h = torch.from_numpy(case["h"]).double().requires_grad_(True)
            a = torch.from_numpy(case["a"]).double().requires_grad_(True)
            j, i = torch.from_numpy(ei)
            b, wi = ref.basis(a)
            b.retain_grad()
            s = torch.zeros((n, m), dtype=torch.float64).index_add_(
                0, i, (h.view(n, k, m)[j.unsqueeze(1), wi] * b.unsqueeze(-1)).sum(1))
            if aggr == "mean":
                s = s / torch.bincount(i, minlength=n).clamp(min=1).double().unsqueeze(-1)
            (s * torch.from_numpy(case["gy"]).double()).sum().backward()
            want = bwd_truth(case, b.detach().numpy(), wi.numpy(), aggr == "mean", None, exact=True)
            assert rel_err(want["gh"], h.grad.numpy()) < 1e-12 and rel_err(want["gb"], b.grad.numpy()) < 1e-12
            assert rel_err(want["ga"], a.grad.numpy()) < 1e-12


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
    assert ptr[0] == 0 and ptr[-1] == ne and np.array_equal(np.sort(perm), np.arange(ne))
    assert np.array_equal(ei[0][perm], other) and np.array_equal(ei[1][perm], np.repeat(np.arange(n), np.diff(ptr)))
    return g, ptr, other, perm


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


def _within_bar_of_float64(got, want64, name, metric=row_rel_err):
    d = metric(got, want64)
    print(f"{name}: {metric.__name__} vs float64 = {d:.3e}")
    record_parity(name, None, e_h=d, metric=metric.__name__)
    assert d < TOL, (name, d)


@gpu
@pytest.mark.parametrize("degree,dim", [(g, d) for g in (1, 2, 3) for d in (1, 2, 3)] + [(1, 4)])
def test_basis_entry(degree, dim):
    """wi equals the restatement's exactly (the inputs are off the knots), b within 1e-5 of float64; ``a`` as an
    unaligned column slice: the same bits; twice: the same bits"""
    ks, op, mult = geometry((3, 4, 5, 2)[:dim], MIXED_OPEN[:dim], degree, dim)
    mult_draw = tuple(max(t, 1) for t in mult)
    rng = np.random.default_rng(70 + degree + 10 * dim)
    a = pseudo(rng, "multigraph", np.zeros((2, 2400), np.int64), mult_draw)
    ta = _dev(a)
    b, wi = ops._spline_basis(ta, ks, op, degree)
    s, k = (degree + 1) ** dim, int(np.prod(ks))
    assert b.shape == (2400, s) and b.dtype == torch.float32 and wi.shape == (2400, s) and wi.dtype == torch.int32
    b32, wi32, _, _ = basis_np(a, ks, mult, degree, np.float32)
    b64, wi64, _, _ = basis_np(a, ks, mult, degree, np.float64)
    assert np.array_equal(wi32, wi64) and np.array_equal(_np(wi).astype(np.int64), wi64)
    assert int(wi.min()) >= 0 and int(wi.max()) < k
    _within_bar_of_float64(_np(b), b64, f"spline basis degree={degree} D={dim}", rel_err)
    for again in (ops._spline_basis(ta, ks, op, degree), ops._spline_basis(_odd(ta), ks, op, degree)):
        assert torch.equal(b, again[0]) and torch.equal(wi, again[1])


@gpu
def test_basis_entry_on_the_ends_of_the_interval_and_outside_it():
    """a exactly 0.0 and exactly 1.0, open and closed: the indices are the restatement's (1.0 on an open dimension wraps
    to index 0 with a basis value of 0 there), all finite; a = -0.25, 1.75, NaN: every wi in [0, K), by value"""
    for degree in (1, 2, 3):
        for op in (True, False):
            ks, opn, mult = geometry((5, 4), op, degree, 2)
            a = np.array([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 0.0]], np.float32)
            b, wi = ops._spline_basis(_dev(a), ks, opn, degree)
            b32, wi32, _, _ = basis_np(a, ks, mult, degree, np.float32)
            assert np.array_equal(_np(wi).astype(np.int64), wi32) and torch.isfinite(b).all()
            assert rel_err(_np(b), b32) < 1e-6 and abs(float(b.sum(1).max()) - 1) < 1e-6
            if op and degree == 1:                                # v = ks - 1: the slots with k_mod = 1 wrap to index 0
                assert float(b[1, 1]) == 0.0 and float(b[1, 0]) == 1.0
    ks, opn, _ = geometry((5, 4, 3), (True, False, True), 2, 3)
    a = np.array([[-0.25, 1.75, 0.5], [1.75, -0.25, -7.5], [np.nan, 0.5, 0.5], [3e9, -3e9, np.inf], [-np.inf, 0.1, np.nan]],
                 np.float32)
    b, wi = ops._spline_basis(_dev(a), ks, opn, 2)
    wi = _np(wi)
    assert wi.shape == (5, 27) and wi.min() >= 0 and wi.max() < 60
    assert torch.isfinite(b[:2]).all() and torch.isnan(b[2]).all()


def slot_geometry(case_or_ks, dim, degree):
    ks, op, mult = geometry(case_or_ks, MIXED_OPEN[:dim], degree, dim)
    return ks, op, tuple(max(t, 1) for t in mult)


@functools.lru_cache(maxsize=None)
def fwd_case(kind, m, ks, dim, degree):
    n, ei = _graph(kind, 9)
    ks_, op, mult_draw = slot_geometry(ks, dim, degree)
    k = int(np.prod(ks_))
    rng = np.random.default_rng(3000 + m + 11 * k + len(kind))
    # h ~ N(1, 1).  The rows are also held against float64 PER ROW, at M = 1 against a single sum.  With a centred h that
    # sum may cancel to any fraction of its terms and a relative bar on it would measure the draw; with a mean of 1 and
    # the non-negative weights of a B-spline the terms mostly share their sign and the comparison measures the kernel's
    # operations (test_gmm_conv.py states the same).  What remains is the error of a sequential float32 sum.
    # The same holds for ``base``: one of the sign opposite to the row's sum can cancel it, and the bar would again measure
    # the draw.  ``base ~ N(0, 1)`` serves the bit comparisons (the ReLU then has something to clamp), ``base_pos`` in
    # [0.5, 1.5] the comparison with float64.
    return dict(n=n, ei=ei, ks=ks_, op=op, K=k, h=(1.0 + rng.standard_normal((n, k * m))).astype(np.float32),
                a=pseudo(rng, kind, ei, mult_draw), base=rng.standard_normal((n, m)).astype(np.float32),
                base_pos=rng.uniform(0.5, 1.5, (n, m)).astype(np.float32))


def fwd_loop_f32(ptr, other, perm, b, wi, h, m):
    """acc [N, M] float32: per row, in p order, the edge's message ``t += b[perm[p], s] * h[other[p], wi[perm[p], s]*M:+M]``
    over s in order, then ``acc += t`` - the kernel's operations one by one (numpy rounds the product, then the add)"""
    s = b.shape[1]
    out = np.zeros((len(ptr) - 1, m), np.float32)
    for i in range(len(ptr) - 1):
        acc = out[i]
        for p in range(ptr[i], ptr[i + 1]):
            row, bq, wq = h[other[p]], b[perm[p]], wi[perm[p]]
            t = np.zeros(m, np.float32)
            for ss in range(s):
                t += bq[ss] * row[wq[ss] * m:(wq[ss] + 1) * m]
            acc += t
    return out


@gpu
@pytest.mark.parametrize("kind", DIRECT_GRAPHS)
@pytest.mark.parametrize("ks,dim,degree", FWD_GEOMS)
@pytest.mark.parametrize("m", WIDTHS)
def test_forward_entry(m, ks, dim, degree, kind):
    """bit-identical to the float32 loop over the device's own sorted set, basis and indices, for both reductions, with
    and without ``base`` and the ReLU; within 1e-5 of float64 per row; operands as column slices (aligned and not): the
    same bits; twice: the same bits"""
    case = fwd_case(kind, m, ks, dim, degree)
    (g, ptr, other, perm), n, k = _device_graph(kind), case["n"], case["K"]
    h, a, base, base_pos = (_dev(case[t]) for t in ("h", "a", "base", "base_pos"))
    b, wi = ops._spline_basis(a, case["ks"], case["op"], degree)
    bn, win = _np(b), _np(wi).astype(np.int64)
    s32 = fwd_loop_f32(ptr, other, perm, bn, win, case["h"], m)
    deg = np.diff(ptr)
    degf = np.maximum(deg, 1).astype(np.float32)[:, None]
    src = case["ei"][0]
    h3 = case["h"].astype(np.float64).reshape(n, k, m)
    msg64 = (h3[src[:, None], win] * bn.astype(np.float64)[:, :, None]).sum(1)
    s64 = _index_add(n, case["ei"][1], msg64)
    for mean in (True, False):
        for with_base in (False, True):
            for relu in (False, True):
                agg = np.where(deg[:, None] > 0, s32 / degf, s32) if mean else s32
                agg64 = s64 / np.maximum(deg, 1)[:, None] if mean else s64
                want = agg + case["base"] if with_base else agg
                if relu:
                    want = np.maximum(want, np.float32(0))
                tb = base if with_base else None
                y = ops._spline_fwd(g, b, wi, h, k, m, mean, tb, relu)
                assert want.dtype == np.float32 and np.array_equal(_np(y), want), (m, ks, kind, mean, with_base, relu)
                if not relu:
                    tag = f"spline fwd M={m} ks={ks} degree={degree} {kind} mean={mean} base={with_base}"
                    if with_base:                                # (the positive base: see ``fwd_case``)
                        yp = _np(ops._spline_fwd(g, b, wi, h, k, m, mean, base_pos, False))
                        assert np.array_equal(yp, agg + case["base_pos"])
                        _within_bar_of_float64(yp, agg64 + case["base_pos"], tag)
                    else:
                        _within_bar_of_float64(_np(y), agg64, tag)
                assert torch.equal(y, ops._spline_fwd(g, b, wi, h, k, m, mean, tb, relu))
                assert torch.equal(y, ops._spline_fwd(g, b, wi, _wide(h), k, m, mean, _wide(tb) if with_base else None, relu))
                assert torch.equal(y, ops._spline_fwd(g, b, wi, _odd(h), k, m, mean, _odd(tb) if with_base else None, relu))
                if not relu or ops.gmm_relu_ok(m):
                    assert torch.equal(y, ops.spline_aggregate(g, h, a, case["ks"], case["op"], degree,
                                                               "mean" if mean else "add", tb, relu))
    # a strided OUTPUT (row stride m + 8): the same values and nothing beside them
    y = ops._spline_fwd(g, b, wi, h, k, m, True, base, False)
    L, st, ld = _lib.lib(), torch.cuda.current_stream().cuda_stream, m + 8
    o_y = torch.full((n, ld), 7.0, device=DEV)
    _lib.check(L.dc_spline_fwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), g.fwd.perm.data_ptr(), b.data_ptr(),
                               wi.data_ptr(), h.data_ptr(), k * m, base.data_ptr(), m, 1, 0, o_y.data_ptr(), ld, n,
                               b.size(0), b.size(1), k, m, st), "dc_spline_fwd")
    assert torch.equal(o_y[:, :m], y) and (o_y[:, m:] == 7.0).all()


@gpu
def test_forward_entry_over_several_column_chunks():
    """M = 1100: 64 lanes walk five column chunks of a row"""
    m, ks, dim, degree, kind = 1100, (3, 4), 2, 2, "multigraph"
    case = fwd_case(kind, m, ks, dim, degree)
    g, ptr, other, perm = _device_graph(kind)
    h, a = _dev(case["h"]), _dev(case["a"])
    b, wi = ops._spline_basis(a, case["ks"], case["op"], degree)
    y = ops._spline_fwd(g, b, wi, h, case["K"], m, False)
    assert np.array_equal(_np(y), fwd_loop_f32(ptr, other, perm, _np(b), _np(wi).astype(np.int64), case["h"], m))
    assert torch.equal(y, ops._spline_fwd(g, b, wi, _odd(h), case["K"], m, False))


@functools.lru_cache(maxsize=None)
def bwd_case(kind, m, ks, dim, degree):
    n, ei = _graph(kind, 9)
    ne = ei.shape[1]
    ks_, op, mult_draw = slot_geometry(ks, dim, degree)
    k, s = int(np.prod(ks_)), (degree + 1) ** dim
    rng = np.random.default_rng(4000 + m + 11 * k + dim + len(kind))
    return dict(n=n, ei=ei, ks=ks_, op=op, mult=geometry(ks, MIXED_OPEN[:dim], degree, dim)[2], K=k, S=s, m=m, dim=dim,
                degree=degree, h=rng.standard_normal((n, k * m)).astype(np.float32), a=pseudo(rng, kind, ei, mult_draw),
                gy=signed(rng, (n, m)), gb=signed(rng, (ne, s)))


def bwd_truth(case, b, wi, mean, gb, exact=False):
    """float64 formulas of the backward over float32 operands.  ``b`` / ``wi``: the basis the entries are given; ``gb``:
    the g_b the ``edge_attr`` entry is given (None: the formula's own); ``gs`` and the fraction ``f`` are the float32
    values the kernels form (``exact``: the float64 ones, for the comparison with autograd)"""
    n, ei, m, k, dim, degree = case["n"], case["ei"], case["m"], case["K"], case["dim"], case["degree"]
    deg = np.maximum(np.bincount(ei[1], minlength=n), 1)
    gy = case["gy"]
    if not mean:
        gs = gy.astype(np.float64)
    elif exact:
        gs = gy.astype(np.float64) / deg[:, None]
    else:
        gs = (gy / deg.astype(np.float32)[:, None]).astype(np.float64)
    b = np.asarray(b, np.float64)
    gh = np.zeros((n, k, m))
    h3 = case["h"].astype(np.float64).reshape(n, k, m)
    gb64 = np.zeros(b.shape)
    for s in range(b.shape[1]):
        np.add.at(gh, (ei[0], wi[:, s]), b[:, s, None] * gs[ei[1]])
        gb64[:, s] = (gs[ei[1]] * h3[ei[0], wi[:, s]]).sum(1)
    t = gb64 if gb is None else np.asarray(gb, np.float64)
    f = basis_np(case["a"], case["ks"], case["mult"], degree, np.float64 if exact else np.float32)[2].astype(np.float64)
    km = slot_digits(degree, dim)
    ga = np.zeros((ei.shape[1], dim))
    for d in range(dim):
        term = t.copy()
        for e in range(dim):
            fn = bspline_d if e == d else bspline
            term = term * fn(np, degree, f[:, e, None], km[e][None].astype(np.float64))
        ga[:, d] = float(case["mult"][d]) * term.sum(1)
    return dict(gh=gh.reshape(n, k * m), gb=gb64, ga=ga)


@gpu
@pytest.mark.parametrize("kind", DIRECT_GRAPHS)
@pytest.mark.parametrize("m,ks,dim,degree", BWD_SHAPES)
def test_backward_entries(m, ks, dim, degree, kind):
    """g_h, g_b and g_a within 1e-5 per row of the float64 formulas, both reductions; operands as column slices: the
    same bits; twice: the same bits; the columns of g_h that no slot names are exactly 0"""
    case = bwd_case(kind, m, ks, dim, degree)
    g, n, ne, k, s = _device_graph(kind)[0], case["n"], case["ei"].shape[1], case["K"], case["S"]
    h, a, gy, gb_in = (_dev(case[t]) for t in ("h", "a", "gy", "gb"))
    b, wi = ops._spline_basis(a, case["ks"], case["op"], degree)
    win = _np(wi).astype(np.int64)
    named = np.zeros((n, k), bool)
    named[np.repeat(case["ei"][0], s), win.reshape(-1)] = True
    for mean in (True, False):
        tag = f"M={m} ks={ks} degree={degree} {kind} mean={mean}"
        want = bwd_truth(case, _np(b), win, mean, case["gb"])
        gh = ops._spline_bwd_h(g, b, wi, gy, k, mean)
        assert gh.shape == (n, k * m)
        _within_bar_of_float64(_np(gh), want["gh"], f"spline g_h {tag}")
        assert (_np(gh).reshape(n, k, m)[~named] == 0).all() and ((~named).any() or k <= 64)
        assert torch.equal(gh, ops._spline_bwd_h(g, b, wi, gy, k, mean))
        assert torch.equal(gh, ops._spline_bwd_h(g, b, wi, _wide(gy), k, mean))
        assert torch.equal(gh, ops._spline_bwd_h(g, b, wi, _odd(gy), k, mean))
        gb = ops._spline_bwd_b(g, wi, h, gy, k, mean)
        assert gb.shape == (ne, s)
        _within_bar_of_float64(_np(gb), want["gb"], f"spline g_b {tag}")
        assert torch.equal(gb, ops._spline_bwd_b(g, wi, h, gy, k, mean))
        assert torch.equal(gb, ops._spline_bwd_b(g, wi, _wide(h), _wide(gy), k, mean))
        assert torch.equal(gb, ops._spline_bwd_b(g, wi, _odd(h), _odd(gy), k, mean))
    ga = ops._spline_bwd_a(gb_in, a, case["ks"], case["op"], degree)
    assert ga.shape == (ne, dim)
    _within_bar_of_float64(_np(ga), want["ga"], f"spline g_a M={m} ks={ks} degree={degree} {kind}")
    assert torch.equal(ga, ops._spline_bwd_a(gb_in, a, case["ks"], case["op"], degree))
    assert torch.equal(ga, ops._spline_bwd_a(gb_in, _odd(a), case["ks"], case["op"], degree))


@gpu
def test_backward_in_b_gives_an_edge_with_a_bad_endpoint_a_zero_row():
    n, m, k, s = 6, 8, 3, 2
    ei = torch.tensor([[0, 1, 7, 2, -1], [1, 2, 3, 9, 0]], device=DEV)
    h, gy = torch.randn(n, k * m, device=DEV), torch.randn(n, m, device=DEV)
    wi = torch.tensor([[0, 1], [2, 0], [1, 2], [0, 0], [2, 1]], dtype=torch.int32, device=DEV)
    gb = torch.full((5, s), 7.0, device=DEV)
    _lib.check(_lib.lib().dc_spline_bwd_b(ei[0].data_ptr(), ei[1].data_ptr(), None, wi.data_ptr(), h.data_ptr(), k * m,
                                          gy.data_ptr(), m, gb.data_ptr(), n, 5, s, k, m,
                                          torch.cuda.current_stream().cuda_stream), "dc_spline_bwd_b")
    h3 = h.double().view(n, k, m)
    want = torch.stack([(gy[[1, 2]].double() * h3[[0, 1], wi[:2, c].long()]).sum(1) for c in range(s)], 1)
    assert (gb[2:] == 0).all() and rel_err(_np(gb[:2]), _np(want)) < TOL


@gpu
def test_entries_with_no_rows_and_with_no_edges():
    """N = 0: ``spline_aggregate`` returns an empty tensor that carries a gradient, without a launch; N > 0 without any
    edge: y = base (or 0), every gradient a zero of the right shape; the checks of ``spline_aggregate``"""
    m, ks, op, d = 5, (2, 3), (1, 0), 2
    k = 6
    agg = lambda g, h, a, *rest: ops.spline_aggregate(g, h, a, ks, op, 1, *rest)
    h0 = torch.zeros((0, k * m), device=DEV, requires_grad=True)
    a0 = torch.zeros((0, d), device=DEV, requires_grad=True)
    y0 = agg(None, h0, a0)
    assert y0.shape == (0, m) and y0.requires_grad
    y0.sum().backward()
    assert h0.grad.shape == (0, k * m) and a0.grad.shape == (0, d)
    n = 37
    g = GraphIndex(torch.zeros((2, 0), dtype=torch.int64, device=DEV), n, self_loops=False, normalize=False)
    h = torch.randn(n, k * m, device=DEV, requires_grad=True)
    base = torch.randn(n, m, device=DEV, requires_grad=True)
    a0.grad = None
    for reduce in AGGRS:
        assert (agg(g, h, a0, reduce) == 0).all()
    y = agg(g, h, a0, "mean", base)
    assert torch.equal(y, base)
    gy = torch.randn(n, m, device=DEV)
    torch.autograd.backward([y], [gy])
    assert torch.equal(base.grad, gy) and (h.grad == 0).all() and h.grad.shape == h.shape and a0.grad.shape == (0, d)
    hd = h.detach()
    with pytest.raises(ValueError, match="rows"):
        agg(g, hd, torch.zeros((3, d), device=DEV))
    with pytest.raises(ValueError, match="None"):
        agg(None, hd, a0.detach())
    with pytest.raises(ValueError):
        agg(g, hd[:5], a0.detach())
    with pytest.raises(RuntimeError):
        agg(g, hd, a0.detach().cpu())
    with pytest.raises(RuntimeError, match="HIP device"):
        agg(g, hd.cpu(), a0.detach())
    with pytest.raises(ValueError):
        agg(GraphIndex(torch.zeros((2, 0), dtype=torch.int64, device=DEV), n, self_loops=True, normalize=False), hd,
            a0.detach())
    # a merged adjacency and a row window of one: their perm names merged edge ids, the kernels take no row offset
    ei2 = torch.tensor([[0, 1, 2], [1, 2, 0]], device=DEV)
    merged = GraphIndex.from_parts([(ei2, 3), (ei2, 3)], self_loops=False, normalize=False)
    for bad, rows in ((merged, merged.num_nodes), (merged.window(1), 3)):
        with pytest.raises(ValueError, match="merged"):
            agg(bad, torch.zeros((rows, k * m), device=DEV), torch.zeros((bad.num_input_edges, d), device=DEV))


# --------------------------------------------------------------------------- #
# GPU: the layer
# --------------------------------------------------------------------------- #
def _device_spline(case):
    fi, m, ks, op, degree, dim = case["shape"]
    conv = dc.nn.SplineConv(fi, m, dim, list(ks) if isinstance(ks, tuple) else ks,
                            list(op) if isinstance(op, tuple) else op, degree, aggr=case["aggr"],
                            root_weight=case["root_weight"], bias=case["bias"])
    conv.load_state_dict({key: v.clone() for key, v in case["cpu"].state_dict().items()}, strict=True)
    return conv.to(DEV)


def _device_run(conv, x, ei, ea, gup, ea_grad=True, call=None):
    for p in conv.parameters():
        p.grad = None
    xg = (x if isinstance(x, torch.Tensor) else _dev(x)).detach().requires_grad_(True)
    eg = (ea if isinstance(ea, torch.Tensor) else _dev(ea)).detach().requires_grad_(ea_grad)
    tei = ei if isinstance(ei, torch.Tensor) else torch.from_numpy(ei).to(DEV)
    out = ops.resolve(call(conv, xg, tei, eg) if call is not None else conv(xg, tei, eg))
    torch.autograd.backward([out], [gup if isinstance(gup, torch.Tensor) else _dev(gup)])
    torch.cuda.synchronize()
    grads = {"x": xg.grad, "edge_attr": eg.grad}
    grads.update({name: p.grad for name, p in conv.named_parameters()})
    return out.detach(), grads


def _host(run):
    return _np(run[0]), {k: (None if v is None else _np(v)) for k, v in run[1].items()}


def _check_layer(case, tag):
    clear_cache()
    conv = _device_spline(case)
    got = _host(_device_run(conv, case["x"], case["ei"], case["ea"], case["gup"]))
    check_against_references(tag, got, case, "e_h")
    return conv, got


@gpu
@pytest.mark.parametrize("shape,aggr,kind", _layer_cases())
def test_layer_parity(shape, aggr, kind):
    """forward and the gradients of x, edge_attr, weight, lin.weight and bias against RefSpline at 1e-5"""
    case = spline_case(shape, aggr, kind)
    _check_layer(case, f"SplineConv {_tag(shape)} {aggr} {kind}")


@gpu
@pytest.mark.parametrize("variant", ["no_root", "no_bias", "no_root_no_bias", "flat_edge_attr"])
def test_layer_parity_variants(variant):
    kw = dict(no_root=dict(root_weight=False), no_bias=dict(bias=False), no_root_no_bias=dict(root_weight=False, bias=False),
              flat_edge_attr=dict(flat=True))[variant]
    shape = SHAPES[2] if variant == "flat_edge_attr" else SHAPES[0]
    case = spline_case(shape, "mean", "multigraph", **kw)
    assert (case["ea"].ndim == 1) == (variant == "flat_edge_attr")
    conv, got = _check_layer(case, f"SplineConv {_tag(shape)} {variant}")
    assert ("lin.weight" in got[1]) == case["root_weight"] and ("bias" in got[1]) == case["bias"]


def _spline_launches(counts):
    """launches per kernel family of dc_spline.hip"""
    fam = {}
    for name, v in counts.items():
        for key in ("k_spline_basis", "k_spline_fwd", "k_spline_bwd_h", "k_spline_bwd_b", "k_spline_bwd_a"):
            if key in name:
                fam[key] = fam.get(key, 0) + v
    assert sum(fam.values()) == sum(v for name, v in counts.items() if "k_spline" in name), counts
    return fam


@gpu
def test_edge_attr_without_a_gradient_skips_its_two_launches():
    case = spline_case(SHAPES[0], "mean", "multigraph")
    clear_cache()
    conv = _device_spline(case)
    want = _device_run(conv, case["x"], case["ei"], case["ea"], case["gup"])
    for ea_grad in (True, False):
        _lib.kernel_trace(True)
        got = _device_run(conv, case["x"], case["ei"], case["ea"], case["gup"], ea_grad=ea_grad)
        counts = _lib.kernel_trace_counts()
        _lib.kernel_trace(False)
        names = ["k_spline_basis", "k_spline_fwd", "k_spline_bwd_h"] + (["k_spline_bwd_b", "k_spline_bwd_a"] if ea_grad else [])
        assert _spline_launches(counts) == {name: 1 for name in names}, counts
        assert not any(bad in name for name in counts for bad in ("k_spmm", "k_sage", "k_gine", "k_gmm")), counts
        assert (got[1]["edge_attr"] is None) == (not ea_grad)
        for name in want[1]:
            if name != "edge_attr" or ea_grad:
                assert torch.equal(got[1][name], want[1][name]), name


@gpu
@pytest.mark.parametrize("kind", EDGE_GRAPHS)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]])
def test_layer_on_graphs_without_edges(shape, kind):
    """one node, no edge, no node: out = lin(x) + bias (or an empty tensor); the gradients of edge_attr and weight are
    zeros of the right shapes"""
    fi, m, ks, op, degree, dim = shape
    case = spline_case(shape, "mean", kind)
    conv, got = _check_layer(case, f"SplineConv {_tag(shape)} {kind}")
    out, grads = _device_run(conv, case["x"], case["ei"], case["ea"], case["gup"])
    assert out.shape == (case["n"], m) and grads["edge_attr"].shape == (0, dim)
    assert grads["weight"].shape == conv.weight.shape and (grads["weight"] == 0).all()
    if case["n"]:
        with torch.no_grad():
            assert torch.equal(out, ops.dense_linear(_dev(case["x"]), conv.lin.weight, conv.bias))


@gpu
@pytest.mark.parametrize("m", [64, 20])
def test_relu_fused_deferred_and_plain_agree(m):
    """``relu=True`` (in the gather's epilogue at M = 64, behind the layer at M = 20), the deferred
    ``F.relu(conv(x, ei, ea))`` and ``torch.relu`` of the plain output: the same bits; their gradients within 1e-5"""
    case = spline_case(SHAPES[0] if m == 64 else SHAPES[4], "mean", "multigraph")
    assert case["shape"][1] == m
    clear_cache()
    conv = _device_spline(case)
    x, ei, ea, gup = case["x"], case["ei"], case["ea"], case["gup"]
    plain = _device_run(conv, x, ei, ea, gup, call=lambda c, *a: torch.relu(ops.resolve(c(*a))))
    fused = _device_run(conv, x, ei, ea, gup, call=lambda c, *a: c(*a, relu=True))
    deferred = _device_run(conv, x, ei, ea, gup, call=lambda c, *a: F.relu(c(*a)))
    with torch.no_grad():
        tei = torch.from_numpy(ei).to(DEV)
        assert type(conv(_dev(x), tei, _dev(ea))).__name__ == "DeferredActivation"
        assert type(conv(_dev(x), tei, _dev(ea), relu=True)) is torch.Tensor
    assert (plain[0] == 0).any() and (plain[0] > 0).any()
    for name, run in (("relu=True", fused), ("deferred", deferred)):
        assert torch.equal(run[0], plain[0]), name
        for key in plain[1]:
            d = rel_err(_np(run[1][key]), _np(plain[1][key]))
            print(f"M={m} {name} {key}.grad vs the plain call: {d:.3e}")
            assert d < TOL, (name, key, d)
    if ops.gmm_relu_ok(m):
        _lib.kernel_trace(True)
        _device_run(conv, x, ei, ea, gup, call=lambda c, *a: c(*a, relu=True))
        counts = _lib.kernel_trace_counts()
        _lib.kernel_trace(False)
        assert sum(v for name, v in counts.items() if "k_mask_colsum" in name) == 1, counts


@gpu
def test_strided_inputs_and_gradient_and_a_repeat_give_the_same_bits():
    case = spline_case(SHAPES[1], "mean", "multigraph")
    n, ei, x, ea, gup = case["n"], case["ei"], case["x"], case["ea"], case["gup"]
    clear_cache()
    conv = _device_spline(case)
    want = _device_run(conv, x, ei, ea, gup)

    def same(a, b):
        assert torch.equal(a[0], b[0]) and set(a[1]) == set(b[1])
        for name in a[1]:
            assert torch.equal(a[1][name], b[1][name]), name
    same(_device_run(conv, x, ei, ea, gup), want)
    wide_g = torch.full((n, 2 * 256), 1e30, device=DEV)
    wide_g[:, ::2] = _dev(gup)
    xs, es, gs = _wide(_dev(x), 7, 3), _wide(_dev(ea), 5, 2), wide_g[:, ::2]
    assert not xs.is_contiguous() and not es.is_contiguous() and not gs.is_contiguous()
    same(_device_run(conv, xs, ei, es, gs), want)


@gpu
def test_a_captured_step_follows_weight_changed_in_place():
    """forward + backward on ONE stream under torch.cuda.graph (no host read anywhere); ``weight`` is then changed in
    place and the graph replayed: the replay equals the eager step at the new value and differs from the step at the
    old one."""
    n, ei = _graph("multigraph", 12)
    fi, m, dim, ks = 32, 64, 3, [3, 4, 5]                        # (M = 64: the ReLU and its mask pass are captured too)
    torch.manual_seed(3)
    conv = dc.nn.SplineConv(fi, m, dim, ks, [True, False, True], degree=2).to(DEV)
    tei = torch.from_numpy(ei).to(DEV)
    rng = np.random.default_rng(1)
    static_x = _dev(rng.standard_normal((n, fi)).astype(np.float32)).requires_grad_(True)
    ea = _dev(pseudo(rng, "multigraph", ei, (1, 4, 3))).requires_grad_(True)
    gup = _dev(signed(rng, (n, m)))
    ws = [_dev(rng.uniform(-0.1, 0.1, tuple(conv.weight.shape)).astype(np.float32)) for _ in range(2)]
    leaves = [static_x, ea] + list(conv.parameters())
    for t in leaves:
        t.grad = torch.zeros_like(t)

    def step():
        for t in leaves:
            t.grad.zero_()
        out = conv(static_x, tei, ea, relu=True)
        torch.autograd.backward([out], [gup])
        return out

    def snapshot(out):
        return [out.detach().clone()] + [t.grad.clone() for t in leaves]

    eager = []
    for w in ws:
        with torch.no_grad():
            conv.weight.copy_(w)
        clear_cache()
        eager.append(snapshot(step()))
    torch.cuda.synchronize()
    assert not torch.equal(eager[0][0], eager[1][0]) and not torch.equal(eager[0][1], eager[1][1])
    with torch.no_grad():
        conv.weight.copy_(ws[0])
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
    for which in (0, 1, 0):
        with torch.no_grad():
            conv.weight.copy_(ws[which])
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(snapshot(out), eager[which]):
            assert torch.equal(got, want), which
