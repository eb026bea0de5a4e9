"""``GMMConv`` (MoNet): the layer, ``ops.gmm_aggregate`` and the C entries of dc_gmm.hip.

The reference is this file's own restatement of the contract in INTEGRATION.md 1.8 (PyG 2.5.2 gmm_conv.py with
``separate_gaussians=False``): ``RefGmm``, a torch CPU module evaluated in float32 (``ref32``) and float64
(``truth64``) with gradients from torch autograd, and numpy formulas for the entries called directly.
``oracle/pyg_ref`` has no GMM.

Inputs, the same everywhere unless a test says otherwise: ``edge_attr`` uniform in [0, 1] (PyG's Cartesian convention;
on ``golden_rest`` the normalised ``rest_pos[src] - rest_pos[dst]``), ``mu`` uniform in [0, 1], ``|sigma|`` uniform in
[0.5, 1.5] with a random sign, ``x ~ N(0, 1)``, upstream gradients of magnitude [0.5, 1.5] with a random sign, ``g`` and
``root.weight`` at their glorot initialisation.  The exponent of a weight then stays above -2 D.

Metrics.  The layers through ``helpers.assert_parity`` at 1e-5, output and every gradient (nothing registered
``special``).  The entries: ``dc_gmm_fwd`` bit-identical to a numpy float32 loop that walks the device's own ``ptr`` /
``other`` / ``perm`` in p, then k order with the device's own weights (``s += w * h``, the product rounded first; mean:
one division by the degree; ``+ base``; ``max(., 0)``) and within 1e-5 per row of float64; ``dc_gmm_weights`` within 1e-5
of the float64 formula (the device ``exp`` is not numpy's: no bit comparison); ``dc_gmm_bwd_h`` / ``_w`` / ``_params``
within 1e-5 of float64 formulas over the SAME float32 operands (``row_rel_err`` for g_h, g_w and g_a, ``rel_err`` for g_mu
and g_sigma); two calls of each: equal bits.

The adjacencies are built WITHOUT self-loop handling: ``seg_graph`` of ``seg_lens`` gives in-degrees 0, 1, 6, ..., 64
and the hub, ``random_multigraph`` keeps its self loops, duplicates and isolated nodes.
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
from deformcontact_amd.nn import GMMConv  # noqa: F401  (the module needs the layer: no test runs without it)
from tests.helpers import assert_parity, load_golden, random_multigraph, record_parity, rel_err, row_rel_err
from tests.test_gat_edge_kernels import HUB, _dev, _np, seg_graph, seg_lens

gpu = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5

#: (in, M, K, D) of the layer tests
SHAPES = [(21, 64, 3, 3), (25, 256, 2, 2), (16, 1, 1, 1), (64, 20, 5, 3), (8, 16, 25, 2)]
AGGRS = ["mean", "add"]
MAIN_GRAPHS = ["seg", "multigraph", "golden_rest"]
EDGE_GRAPHS = ["n1", "e0", "n0"]
#: widths of the direct forward test: the general form (1, 3, 70: lane groups of 4, 4, 64) and the 16-byte form (20, 64,
#: 256: groups of 8, 16, 64); 1100: 64 lanes over five column chunks (one case)
WIDTHS = [1, 3, 20, 64, 70, 256]
KERNELS = [1, 3, 8]
DIRECT_GRAPHS = ["seg", "multigraph"]
#: (M, K, D) of the direct backward tests: general and 16-byte form, K below / at / above the kernels in flight of g_w,
#: K*D below and above the 128 pairs at which the [K, D] sums change their form
BWD_SHAPES = [(3, 1, 1), (20, 3, 3), (64, 8, 2), (70, 5, 16), (256, 2, 3), (4, 25, 8)]


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


def pseudo(rng, kind, ei, d):
    """edge_attr [E, d] in [0, 1]: on ``golden_rest`` (d = 3) the normalised Cartesian offsets, else uniform"""
    if kind == "golden_rest":
        assert d == 3
        pos = load_golden("graphnet_gat_h32.npz")["rest_pos"].astype(np.float32)
        cart = pos[ei[0]] - pos[ei[1]]
        return (cart / (2 * np.abs(cart).max()) + 0.5).astype(np.float32)
    return rng.uniform(0.0, 1.0, (ei.shape[1], d)).astype(np.float32)


def weights64(a, mu, sigma):
    """w [E, K] float64 from float32 operands: the contract's formula"""
    a, mu, sigma = (np.asarray(t, np.float64) for t in (a, mu, sigma))
    return np.exp((-0.5 * (a[:, None, :] - mu[None]) ** 2 / (1e-15 + sigma[None] ** 2)).sum(-1))


def _index_add(n, idx, terms):
    return torch.zeros((n, terms.shape[1]), dtype=torch.float64).index_add_(
        0, torch.from_numpy(idx), torch.from_numpy(np.ascontiguousarray(terms, np.float64))).numpy()


# --------------------------------------------------------------------------- #
# the restatement as a torch module (float32: ref32, .double(): truth64)
# --------------------------------------------------------------------------- #
class RefGmm(nn.Module):
    def __init__(self, fi, m, d, k, aggr="mean", root_weight=True, bias=True):
        super().__init__()
        self.m, self.k, self.d, self.aggr = m, k, d, aggr
        self.g = nn.Parameter(torch.empty(fi, k * m))
        self.mu = nn.Parameter(torch.empty(k, d))
        self.sigma = nn.Parameter(torch.empty(k, d))
        if root_weight:
            self.root = nn.Linear(fi, m, bias=False)
        if bias:
            self.bias = nn.Parameter(torch.zeros(m))
        for p in (self.g, self.mu, self.sigma) + ((self.root.weight,) if root_weight else ()):
            a = (6.0 / (p.size(-2) + p.size(-1))) ** 0.5
            nn.init.uniform_(p, -a, a)

    def weights(self, edge_attr):
        e = edge_attr.size(0)
        gauss = -0.5 * (edge_attr.view(e, 1, self.d) - self.mu.view(1, self.k, self.d)).pow(2)
        gauss = gauss / (1e-15 + self.sigma.view(1, self.k, self.d).pow(2))
        return torch.exp(gauss.sum(dim=-1))

    def forward(self, x, edge_index, edge_attr):
        j, i = edge_index
        if edge_attr.dim() == 1:
            edge_attr = edge_attr.unsqueeze(-1)
        e, n = edge_attr.size(0), x.size(0)
        h = x @ self.g
        msg = (h[j].view(e, self.k, self.m) * self.weights(edge_attr).view(e, self.k, 1)).sum(dim=-2)
        s = torch.zeros((n, self.m), dtype=x.dtype).index_add_(0, i, msg)
        if self.aggr == "mean":
            s = s / torch.bincount(i, minlength=n).clamp(min=1).to(x.dtype).unsqueeze(-1)
        if hasattr(self, "root"):
            s = s + self.root(x)
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
def gmm_case(fi, m, k, d, aggr, kind, root_weight=True, bias=True, flat=False):
    """inputs, the reference module and its float32 / float64 results of one layer case (computed once, never modified);
    ``flat``: D = 1 with ``edge_attr`` of shape [E]"""
    torch.set_num_threads(1)
    n, ei = _graph(kind, 3)
    rng = np.random.default_rng(1000 + fi + m + 7 * k + d)
    torch.manual_seed(12)
    cpu = RefGmm(fi, m, d, k, aggr, root_weight, bias)
    with torch.no_grad():
        cpu.mu.copy_(torch.from_numpy(rng.uniform(0.0, 1.0, (k, d)).astype(np.float32)))
        cpu.sigma.copy_(torch.from_numpy(signed(rng, (k, d))))
        if bias:
            cpu.bias.copy_(torch.from_numpy(rng.standard_normal(m).astype(np.float32)))
    x = rng.standard_normal((n, fi)).astype(np.float32)
    ea = pseudo(rng, kind, ei, d)
    if flat:
        ea = ea[:, 0].copy()
    gup = signed(rng, (n, m))
    r32 = _ref_run(cpu, x, ei, ea, gup, torch.float32)
    r64 = _ref_run(copy.deepcopy(cpu).double(), x, ei, ea, gup, torch.float64)
    return dict(n=n, ei=ei, x=x, ea=ea, gup=gup, cpu=cpu, aggr=aggr, root_weight=root_weight, bias=bias, r32=r32, r64=r64,
                shape=(fi, m, k, d))


def _layer_cases():
    cases = [(s, aggr, kind) for s in SHAPES for aggr in AGGRS for kind in MAIN_GRAPHS
             if kind != "golden_rest" or s[3] == 3]
    return cases


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
    return {k: tuple(v.shape) for k, v in mod.state_dict().items()}


def test_surface_and_alias():
    import sys
    from deformcontact_amd.pyg_alias import install_as_torch_geometric
    assert "GMMConv" in dc.nn.__all__ and dc.nn.__all__[-1] == "ChebConv"
    assert dc.nn.__all__.index("GMMConv") == len(dc.nn.__all__) - 2
    names = ("torch_geometric", "torch_geometric.nn", "torch_geometric.data")
    saved = {k: sys.modules.get(k) for k in names}
    try:
        install_as_torch_geometric(force=True)
        from torch_geometric.nn import GMMConv as alias
        assert alias is dc.nn.GMMConv
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_constructor_parameters_state_dict_and_repr():
    for root_weight in (True, False):
        for bias in (True, False):
            conv = dc.nn.GMMConv(21, 64, dim=3, kernel_size=5, root_weight=root_weight, bias=bias)
            want = {"g": (21, 320), "mu": (5, 3), "sigma": (5, 3)}
            if root_weight:
                want["root.weight"] = (64, 21)
            if bias:
                want["bias"] = (64,)
            assert _shapes(conv) == want
            assert set(dict(conv.named_parameters())) == set(want)
            ref = RefGmm(21, 64, 3, 5, "mean", root_weight, bias)
            assert _shapes(ref) == want
            conv.load_state_dict(ref.state_dict(), strict=True)
            assert torch.equal(conv.g, ref.g) and torch.equal(conv.sigma, ref.sigma)
            assert (conv.root is None) == (not root_weight) and (conv.bias is None) == (not bias)
    conv = dc.nn.GMMConv(21, 64, 3, 5)                            # dim and kernel_size positional, as in PyG
    assert (conv.dim, conv.kernel_size, conv.aggr, conv.separate_gaussians) == (3, 5, "mean", False)
    assert conv.graph_flags() == dict(self_loops=False, normalize=False) and conv.supports_fused_relu
    assert repr(conv) == "GMMConv(21, 64, dim=3)" and conv.extra_repr() == "21, 64, dim=3"
    assert dc.nn.GMMConv(4, 4, 2, 3, aggr="add").aggr == "add"


def test_initialisation_is_glorot_and_zero_bias():
    torch.manual_seed(0)
    conv = dc.nn.GMMConv(40, 48, dim=3, kernel_size=7)
    for p, rows, cols in ((conv.g, 40, 336), (conv.mu, 7, 3), (conv.sigma, 7, 3), (conv.root.weight, 48, 40)):
        a = (6.0 / (rows + cols)) ** 0.5
        assert p.shape == (rows, cols) and float(p.detach().abs().max()) <= a
        if p.numel() > 500:
            assert float(p.detach().abs().max()) > 0.97 * a and abs(float(p.detach().mean())) < 0.05 * a
    assert (conv.bias == 0).all()
    with torch.no_grad():
        before = [p.detach().clone() for p in conv.parameters()]
        conv.bias.fill_(3.0)
    conv.reset_parameters()
    assert (conv.bias == 0).all()
    assert all(not torch.equal(a, b) for a, b in zip(list(conv.parameters())[:3], before[:3]))


def test_errors_raised_on_the_host():
    with pytest.raises(NotImplementedError, match="separate_gaussians"):
        dc.nn.GMMConv(4, 4, 2, 3, separate_gaussians=True)
    with pytest.raises(NotImplementedError, match="bipartite"):
        dc.nn.GMMConv((4, 4), 4, 2, 3)
    with pytest.raises(NotImplementedError, match="max"):
        dc.nn.GMMConv(4, 4, 2, 3, aggr="max")
    for bad in ("min", "sum", "softmax", None, ["mean"]):
        with pytest.raises(ValueError, match="aggr"):
            dc.nn.GMMConv(4, 4, 2, 3, aggr=bad)
    for kw in (dict(dim=0), dict(dim=17), dict(kernel_size=0), dict(kernel_size=65), dict(kernel_size=2.0)):
        with pytest.raises(ValueError, match="within"):
            dc.nn.GMMConv(4, 4, **{**dict(dim=2, kernel_size=3), **kw})
    dc.nn.GMMConv(4, 4, 16, 64)                                  # the caps themselves are allowed
    x, ei = torch.zeros(5, 4), torch.zeros(2, 3, dtype=torch.long)
    conv, one = dc.nn.GMMConv(4, 2, 3, 2), dc.nn.GMMConv(4, 2, 1, 2)
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


def test_host_checks_of_gmm_aggregate():
    h, ea, mu, sg = torch.zeros(5, 8), torch.zeros(3, 3), torch.zeros(2, 3), torch.ones(2, 3)
    with pytest.raises(ValueError, match="reduce"):
        ops.gmm_aggregate(None, h, ea, mu, sg, reduce="max")
    with pytest.raises(ValueError, match="mu and sigma"):
        ops.gmm_aggregate(None, h, ea, mu, torch.ones(2, 2))
    with pytest.raises(ValueError, match="mu and sigma"):
        ops.gmm_aggregate(None, h, ea, mu.double(), sg.double())
    with pytest.raises(ValueError, match="kernel_size"):
        ops.gmm_aggregate(None, torch.zeros(5, 65), torch.zeros(3, 1), torch.zeros(65, 1), torch.ones(65, 1))
    with pytest.raises(ValueError, match="dim"):
        ops.gmm_aggregate(None, h, torch.zeros(3, 17), torch.zeros(2, 17), torch.ones(2, 17))
    with pytest.raises(ValueError, match=r"K\*M"):
        ops.gmm_aggregate(None, torch.zeros(5, 7), ea, mu, sg)   # 7 columns are no multiple of K = 2
    with pytest.raises(ValueError, match=r"K\*M"):
        ops.gmm_aggregate(None, h.double(), ea, mu, sg)
    with pytest.raises(ValueError, match="edge_attr"):
        ops.gmm_aggregate(None, h, torch.zeros(3, 2), mu, sg)
    with pytest.raises(ValueError, match="base"):
        ops.gmm_aggregate(None, h, ea, mu, sg, base=torch.zeros(5, 8))
    with pytest.raises(ValueError, match="relu"):
        ops.gmm_aggregate(None, torch.zeros(5, 6), ea, mu, sg, relu=True)        # M = 3: no width of the mask pass
    with pytest.raises(TypeError, match="mu"):
        ops.gmm_aggregate(None, h, ea, 0.5, sg)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.gmm_aggregate(None, h, ea, mu, sg)                   # every host check passed: no CPU path
    assert ops.gmm_relu_ok(64) and ops.gmm_relu_ok(256) and ops.gmm_relu_ok(4) and not ops.gmm_relu_ok(20)
    assert not ops.gmm_relu_ok(1) and not ops.gmm_relu_ok(70) and not ops.gmm_relu_ok(2048)


def _entry_calls():
    """name -> call(rows, M, K, D, pointers given?, leading dimension) of every entry of dc_gmm.hip, otherwise valid"""
    L = _lib.lib()
    p = lambda ok, at=64: at if ok else None                     # any non-null address: rejected calls never touch it
    return {
        "dc_gmm_weights": lambda r, m, k, d, ok, ld: L.dc_gmm_weights(p(ok), ld if ld < d else d, p(ok), p(ok), p(ok, 128),
                                                                      r, k, d, None),
        "dc_gmm_fwd": lambda r, m, k, d, ok, ld: L.dc_gmm_fwd(p(ok), p(ok), p(ok), p(ok), p(ok, 192), ld * k, None, 0, 1, 0,
                                                              p(ok, 128), ld, r, 5 if r > 0 else 0, k, m, None),
        "dc_gmm_bwd_h": lambda r, m, k, d, ok, ld: L.dc_gmm_bwd_h(p(ok), p(ok), p(ok), p(ok), p(ok), p(ok, 192), ld,
                                                                  p(ok, 128), ld * k, r, 5 if r > 0 else 0, k, m, None),
        "dc_gmm_bwd_w": lambda r, m, k, d, ok, ld: L.dc_gmm_bwd_w(p(ok), p(ok), p(ok), p(ok, 192), ld * k, p(ok, 256), ld,
                                                                  p(ok, 128), 3, r, k, m, None),
        "dc_gmm_bwd_params": lambda r, m, k, d, ok, ld: L.dc_gmm_bwd_params(
            p(ok), p(ok), p(ok), ld if ld < d else d, p(ok), p(ok), p(ok, 512), 1 << 20, p(ok, 128), p(ok, 192), None, 0,
            r, k, d, None),
    }


def test_abi_argument_errors_of_the_gmm_entries_without_gpu():
    """null pointers, negative sizes, M < 1, the caps of K and D, sizes out of range, short leading dimensions, aliased
    outputs: -1 and the entry's name, before any HIP call; no row (no edge) returns 0 with no pointer at all"""
    L = _lib.lib()
    calls = _entry_calls()
    declared = [n for n in _lib.exported_names() if "gmm" in n]
    assert sorted(declared) == sorted(list(calls) + ["dc_gmm_params_workspace_bytes"])
    for name, call in calls.items():
        err = lambda: L.dc_last_error()
        assert call(3, 16, 2, 3, False, 64) == -1 and name.encode() in err() and b"null" in err(), name
        assert call(-1, 16, 2, 3, True, 64) == -1 and name.encode() in err(), name
        assert call(3, 16, 0, 3, True, 64) == -1 and name.encode() in err() and b"K" in err(), name
        assert call(3, 16, 65, 3, True, 64) == -1 and name.encode() in err() and b"K" in err(), name
        assert call(1 << 30, 16, 2, 3, True, 64) == -1 and b"range" in err(), name
        assert call(0, 16, 2, 3, False, 64) == 0, name           # no row / no edge: nothing is read, written or launched
        assert call(3, 16, 2, 3, True, 2 if name in ("dc_gmm_weights", "dc_gmm_bwd_params") else 15) == -1 \
            and name.encode() in err() and b"leading" in err(), name
        if name in ("dc_gmm_weights", "dc_gmm_bwd_params"):
            assert call(3, 16, 2, 0, True, 64) == -1 and b"D" in err(), name
            assert call(3, 16, 2, 17, True, 64) == -1 and b"D" in err(), name
        else:
            assert call(3, 0, 2, 3, True, 64) == -1 and name.encode() in err(), name
            assert call(3, 1 << 24, 2, 3, True, 1 << 24) == -1 and b"range" in err(), name
    # E * K must stay below 2^31
    assert L.dc_gmm_weights(64, 3, 64, 64, 128, 1 << 26, 64, 3, None) == -1 and b"range" in L.dc_last_error()
    # outputs that alias an operand
    assert L.dc_gmm_weights(64, 3, 128, 192, 64, 5, 2, 3, None) == -1 and b"alias" in L.dc_last_error()
    assert L.dc_gmm_fwd(64, 64, 64, 64, 192, 32, None, 0, 1, 0, 192, 16, 3, 5, 2, 16, None) == -1 and b"alias" in L.dc_last_error()
    assert L.dc_gmm_fwd(64, 64, 64, 64, 192, 32, 128, 16, 1, 0, 128, 16, 3, 5, 2, 16, None) == -1 and b"alias" in L.dc_last_error()
    assert L.dc_gmm_bwd_h(64, 64, 64, 64, 64, 192, 16, 192, 32, 3, 5, 2, 16, None) == -1 and b"alias" in L.dc_last_error()
    assert L.dc_gmm_bwd_w(64, 64, 64, 192, 32, 256, 16, 256, 3, 5, 2, 16, None) == -1 and b"alias" in L.dc_last_error()
    assert L.dc_gmm_bwd_params(64, 128, 192, 3, 256, 320, 512, 1 << 20, 256, 384, None, 0, 5, 2, 3, None) == -1
    assert b"alias" in L.dc_last_error()
    assert L.dc_gmm_bwd_params(64, 128, 192, 3, 256, 320, 512, 1 << 20, 384, 384, None, 0, 5, 2, 3, None) == -1
    assert b"alias" in L.dc_last_error()
    # the workspace of the [K, D] sums
    assert L.dc_gmm_params_workspace_bytes(0, 2, 3) == 0 and L.dc_gmm_params_workspace_bytes(5, 2, 3) == 2 * 6 * 8
    assert L.dc_gmm_params_workspace_bytes(1 << 20, 64, 16) == 1024 * 2 * 1024 * 8
    assert L.dc_gmm_bwd_params(64, 128, 192, 3, 256, 320, 512, 95, 384, 448, None, 0, 5, 2, 3, None) == -1
    assert b"workspace" in L.dc_last_error()
    assert L.dc_gmm_bwd_params(64, 128, 192, 3, 256, 320, None, 1 << 20, 384, 448, None, 0, 5, 2, 3, None) == -1


def test_float32_restatement_within_the_bar_of_float64_on_the_layer_inputs():
    """Every layer case of the GPU tests: the float32 restatement within 1e-5 of float64, output and every gradient"""
    for (fi, m, k, d), aggr, kind in _layer_cases():
        case = gmm_case(fi, m, k, d, aggr, kind)
        check_against_references(f"RefGmm fp32 vs fp64 {fi}->{m} K={k} D={d} {aggr} {kind}", case["r32"], case, "e_o")
        assert set(case["r32"][1]) == {"x", "edge_attr", "g", "mu", "sigma", "root.weight", "bias"}


def test_backward_formulas_of_the_direct_tests_agree_with_autograd():
    """the hand-written float64 formulas the entries are held against equal torch autograd through ``RefGmm``"""
    for aggr in AGGRS:
        case = bwd_case("multigraph", 20, 3, 3)
        n, ei = case["n"], case["ei"]
        ref = RefGmm(5, 20, 3, 3, aggr, root_weight=False, bias=False).double()
        with torch.no_grad():
            ref.mu.copy_(torch.from_numpy(case["mu"]))
            ref.sigma.copy_(torch.from_numpy(case["sigma"]))
        h = torch.from_numpy(case["h"]).double().requires_grad_(True)
        a = torch.from_numpy(case["a"]).double().requires_grad_(True)
        j, i = torch.from_numpy(ei)
        w = ref.weights(a)
        assert rel_err(w.detach().numpy(), weights64(case["a"], case["mu"], case["sigma"])) < 1e-14
        s = torch.zeros((n, 20), dtype=torch.float64).index_add_(0, i, (h[j].view(-1, 3, 20) * w.view(-1, 3, 1)).sum(-2))
        if aggr == "mean":
            s = s / torch.bincount(i, minlength=n).clamp(min=1).double().unsqueeze(-1)
        (s * torch.from_numpy(case["gy"]).double()).sum().backward()
        want = bwd_truth(case, w.detach().numpy(), aggr == "mean", None, exact_gs=True)
        assert rel_err(want["gh"], h.grad.numpy()) < 1e-13 and rel_err(want["ga"], a.grad.numpy()) < 1e-12
        assert rel_err(want["gmu"], ref.mu.grad.numpy()) < 1e-12 and rel_err(want["gsigma"], ref.sigma.grad.numpy()) < 1e-12


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


@functools.lru_cache(maxsize=None)
def fwd_case(kind, m, k):
    n, ei = _graph(kind, 9)
    rng = np.random.default_rng(3000 + m + 11 * k + len(kind))
    d = 3
    # h ~ N(1, 1).  The rows are also held against float64 PER ROW, at M = 1 against a single sum.  With a centred h that
    # sum may cancel to any fraction of its terms and a relative bar on it would measure the draw; with a mean of 1 and
    # positive weights the terms mostly share their sign and the comparison measures the kernel's operations (as
    # ``node_features`` of test_gine_conv.py).  What remains is the error of a sequential float32 sum, which is the
    # contract: for the hub's n = 8 * 5,000 terms about 3.4e-8 sqrt(n / 3) = 4e-6 of the sum is expected (measured on
    # the MI355X: 8.6e-6 at K = 8, the worst of all cases; 9.4e-6 at M = K = 1 with a ``base`` of either sign added).
    return dict(n=n, ei=ei, h=(1.0 + rng.standard_normal((n, k * m))).astype(np.float32),
                a=rng.uniform(0, 1, (ei.shape[1], d)).astype(np.float32),
                mu=rng.uniform(0, 1, (k, d)).astype(np.float32), sigma=signed(rng, (k, d)),
                base=rng.standard_normal((n, m)).astype(np.float32))


def fwd_loop_f32(ptr, other, perm, w, h, m):
    """s [N, M] float32: per row, in p then k order, ``s += w[perm[p], k] * h[other[p], k*M:(k+1)*M]`` - the kernel's
    operations one by one (numpy rounds the product, then the add)"""
    k = w.shape[1]
    s = np.zeros((len(ptr) - 1, m), np.float32)
    for i in range(len(ptr) - 1):
        acc = s[i]
        for p in range(ptr[i], ptr[i + 1]):
            row, wq = h[other[p]], w[perm[p]]
            for kk in range(k):
                acc += wq[kk] * row[kk * m:(kk + 1) * m]
    return s


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
@pytest.mark.parametrize("kind", DIRECT_GRAPHS)
@pytest.mark.parametrize("k", KERNELS)
@pytest.mark.parametrize("m", WIDTHS)
def test_forward_entry(m, k, kind):
    """bit-identical to the float32 loop over the device's own sorted set and weights, for both reductions, with and
    without ``base`` and the ReLU; within 1e-5 of float64 per row; operands as column slices (aligned and not): the same
    bits; twice: the same bits"""
    case = fwd_case(kind, m, k)
    (g, ptr, other, perm), n = _device_graph(kind), case["n"]
    h, a, mu, sg, base = (_dev(case[t]) for t in ("h", "a", "mu", "sigma", "base"))
    w = ops._gmm_weights(a, mu, sg)
    s32 = fwd_loop_f32(ptr, other, perm, _np(w), case["h"], m)
    deg = np.diff(ptr)
    degf = np.maximum(deg, 1).astype(np.float32)[:, None]
    w64 = _np(w).astype(np.float64)
    msg64 = (case["h"].astype(np.float64)[case["ei"][0]].reshape(-1, k, m) * w64[:, :, None]).sum(1)
    s64 = _index_add(n, case["ei"][1], msg64)
    for mean in (True, False):
        for with_base in (False, True):
            for relu in (False, True):
                want = np.where(deg[:, None] > 0, s32 / degf, s32) if mean else s32
                want64 = s64 / np.maximum(deg, 1)[:, None] if mean else s64
                if with_base:
                    want, want64 = want + case["base"], want64 + case["base"]
                if relu:
                    want, want64 = np.maximum(want, np.float32(0)), np.maximum(want64, 0.0)
                tb = base if with_base else None
                y = ops._gmm_fwd(g, w, h, m, mean, tb, relu)
                assert want.dtype == np.float32 and np.array_equal(_np(y), want), (m, k, kind, mean, with_base, relu)
                if not relu:
                    _within_bar_of_float64(_np(y), want64, f"gmm fwd M={m} K={k} {kind} mean={mean} base={with_base}")
                assert torch.equal(y, ops._gmm_fwd(g, w, h, m, mean, tb, relu))
                assert torch.equal(y, ops._gmm_fwd(g, w, _wide(h), m, mean, _wide(tb) if with_base else None, relu))
                assert torch.equal(y, ops._gmm_fwd(g, w, _odd(h), m, mean, _odd(tb) if with_base else None, relu))
                if not relu or ops.gmm_relu_ok(m):
                    assert torch.equal(y, ops.gmm_aggregate(g, h, a, mu, sg, "mean" if mean else "add", tb, relu))
    # a strided OUTPUT (row stride m + 8): the same values and nothing beside them
    y = ops._gmm_fwd(g, w, h, m, True, base, False)
    L, st, ld = _lib.lib(), torch.cuda.current_stream().cuda_stream, m + 8
    o_y = torch.full((n, ld), 7.0, device=DEV)
    _lib.check(L.dc_gmm_fwd(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), g.fwd.perm.data_ptr(), w.data_ptr(), h.data_ptr(),
                            k * m, base.data_ptr(), m, 1, 0, o_y.data_ptr(), ld, n, w.size(0), k, m, st), "dc_gmm_fwd")
    assert torch.equal(o_y[:, :m], y) and (o_y[:, m:] == 7.0).all()


@gpu
def test_forward_entry_over_several_column_chunks():
    """M = 1100: 64 lanes walk five column chunks of a row"""
    m, k, kind = 1100, 3, "multigraph"
    case = fwd_case(kind, m, k)
    g, ptr, other, perm = _device_graph(kind)
    h, a, mu, sg = (_dev(case[t]) for t in ("h", "a", "mu", "sigma"))
    w = ops._gmm_weights(a, mu, sg)
    y = ops._gmm_fwd(g, w, h, m, False)
    assert np.array_equal(_np(y), fwd_loop_f32(ptr, other, perm, _np(w), case["h"], m))
    assert torch.equal(y, ops._gmm_fwd(g, w, _odd(h), m, False))


@gpu
@pytest.mark.parametrize("d", [1, 2, 3, 16])
@pytest.mark.parametrize("k", [1, 3, 25, 64])
def test_weights_entry(k, d):
    """within 1e-5 of the float64 formula; ``edge_attr`` as a column slice: the same bits; twice: the same bits; one
    sigma exactly 0 with a != mu: the weight is exactly 0 and everything stays finite, as torch float32 gives"""
    rng = np.random.default_rng(50 + k + 100 * d)
    ne = 2400
    a = rng.uniform(0, 1, (ne, d)).astype(np.float32)
    mu, sigma = rng.uniform(0, 1, (k, d)).astype(np.float32), signed(rng, (k, d))
    ta, tm, ts = _dev(a), _dev(mu), _dev(sigma)
    w = ops._gmm_weights(ta, tm, ts)
    assert w.shape == (ne, k) and torch.isfinite(w).all() and (w >= 0).all() and (w <= 1).all()
    _within_bar_of_float64(_np(w), weights64(a, mu, sigma), f"gmm weights K={k} D={d}", rel_err)
    assert torch.equal(w, ops._gmm_weights(ta, tm, ts)) and torch.equal(w, ops._gmm_weights(_odd(ta), tm, ts))
    sigma[k // 2, d - 1] = 0.0
    assert (a[:, d - 1] != mu[k // 2, d - 1]).all()
    ref = RefGmm(2, 1, d, k)
    with torch.no_grad():
        ref.mu.copy_(torch.from_numpy(mu))
        ref.sigma.copy_(torch.from_numpy(sigma))
        w32 = ref.weights(torch.from_numpy(a)).numpy()
    assert (w32[:, k // 2] == 0).all() and np.isfinite(w32).all()
    w0 = ops._gmm_weights(ta, tm, _dev(sigma))
    assert torch.isfinite(w0).all() and (w0[:, k // 2] == 0).all()
    others = [c for c in range(k) if c != k // 2]
    assert torch.equal(w0[:, others], w[:, others])


@functools.lru_cache(maxsize=None)
def bwd_case(kind, m, k, d):
    n, ei = _graph(kind, 9)
    ne = ei.shape[1]
    rng = np.random.default_rng(4000 + m + 11 * k + d + len(kind))
    return dict(n=n, ei=ei, h=rng.standard_normal((n, k * m)).astype(np.float32),
                a=rng.uniform(0, 1, (ne, d)).astype(np.float32), mu=rng.uniform(0, 1, (k, d)).astype(np.float32),
                sigma=signed(rng, (k, d)), gy=signed(rng, (n, m)), gw=signed(rng, (ne, k)), m=m, k=k, d=d)


def bwd_truth(case, w, mean, gw, exact_gs=False):
    """float64 formulas of the backward over float32 operands.  ``w``: the weights the entries are given; ``gw``: the
    g_w the parameter entry is given (None: the formula's own); ``gs`` is the float32 quotient the kernels form
    (``exact_gs``: the float64 one, for the comparison with autograd)"""
    n, ei, m, k = case["n"], case["ei"], case["m"], case["k"]
    deg = np.maximum(np.bincount(ei[1], minlength=n), 1)
    gy = case["gy"]
    if not mean:
        gs = gy.astype(np.float64)
    elif exact_gs:
        gs = gy.astype(np.float64) / deg[:, None]
    else:
        gs = (gy / deg.astype(np.float32)[:, None]).astype(np.float64)
    w = np.asarray(w, np.float64)
    gh = _index_add(n, ei[0], (w[:, :, None] * gs[ei[1]][:, None, :]).reshape(-1, k * m))
    gw64 = np.einsum("ec,ekc->ek", gs[ei[1]], case["h"].astype(np.float64)[ei[0]].reshape(-1, k, m))
    t = (gw64 if gw is None else np.asarray(gw, np.float64)) * w
    a, mu, sigma = (case[x].astype(np.float64) for x in ("a", "mu", "sigma"))
    r = (a[:, None, :] - mu[None]) / (1e-15 + sigma[None] ** 2)
    return dict(gh=gh, gw=gw64, gmu=np.einsum("ek,ekd->kd", t, r), gsigma=np.einsum("ek,ekd->kd", t, r * r) * sigma,
                ga=-np.einsum("ek,ekd->ed", t, r))


@gpu
@pytest.mark.parametrize("kind", DIRECT_GRAPHS)
@pytest.mark.parametrize("m,k,d", BWD_SHAPES)
def test_backward_entries(m, k, d, kind):
    """g_h, g_w and g_a within 1e-5 per row, g_mu and g_sigma within 1e-5 of the float64 formulas, both reductions;
    operands as column slices: the same bits; twice: the same bits; g_a skipped when not asked for"""
    case = bwd_case(kind, m, k, d)
    g, n, ne = _device_graph(kind)[0], case["n"], case["ei"].shape[1]
    h, a, mu, sg, gy, gw_in = (_dev(case[t]) for t in ("h", "a", "mu", "sigma", "gy", "gw"))
    w = ops._gmm_weights(a, mu, sg)
    for mean in (True, False):
        tag = f"M={m} K={k} D={d} {kind} mean={mean}"
        want = bwd_truth(case, _np(w), mean, case["gw"])
        gh = ops._gmm_bwd_h(g, w, gy, mean)
        assert gh.shape == (n, k * m)
        _within_bar_of_float64(_np(gh), want["gh"], f"gmm g_h {tag}")
        assert torch.equal(gh, ops._gmm_bwd_h(g, w, gy, mean)) and torch.equal(gh, ops._gmm_bwd_h(g, w, _wide(gy), mean))
        assert torch.equal(gh, ops._gmm_bwd_h(g, w, _odd(gy), mean))
        gw = ops._gmm_bwd_w(g, h, gy, k, mean)
        assert gw.shape == (ne, k)
        _within_bar_of_float64(_np(gw), want["gw"], f"gmm g_w {tag}")
        assert torch.equal(gw, ops._gmm_bwd_w(g, h, gy, k, mean))
        assert torch.equal(gw, ops._gmm_bwd_w(g, _wide(h), _wide(gy), k, mean))
        assert torch.equal(gw, ops._gmm_bwd_w(g, _odd(h), _odd(gy), k, mean))
    gmu, gsigma, ga = ops._gmm_bwd_params(gw_in, w, a, mu, sg, True)
    assert gmu.shape == (k, d) and gsigma.shape == (k, d) and ga.shape == (ne, d)
    tag = f"M={m} K={k} D={d} {kind}"
    _within_bar_of_float64(_np(gmu), want["gmu"], f"gmm g_mu {tag}", rel_err)
    _within_bar_of_float64(_np(gsigma), want["gsigma"], f"gmm g_sigma {tag}", rel_err)
    _within_bar_of_float64(_np(ga), want["ga"], f"gmm g_a {tag}")
    again = ops._gmm_bwd_params(gw_in, w, _odd(a), mu, sg, True)
    assert torch.equal(gmu, again[0]) and torch.equal(gsigma, again[1]) and torch.equal(ga, again[2])
    skipped = ops._gmm_bwd_params(gw_in, w, a, mu, sg, False)
    assert torch.equal(gmu, skipped[0]) and torch.equal(gsigma, skipped[1]) and skipped[2] is None


@gpu
def test_backward_in_w_gives_an_edge_with_a_bad_endpoint_a_zero_row():
    n, m, k = 6, 8, 3
    ei = torch.tensor([[0, 1, 7, 2, -1], [1, 2, 3, 9, 0]], device=DEV)
    h, gy = torch.randn(n, k * m, device=DEV), torch.randn(n, m, device=DEV)
    gw = torch.full((5, k), 7.0, device=DEV)
    _lib.check(_lib.lib().dc_gmm_bwd_w(ei[0].data_ptr(), ei[1].data_ptr(), None, h.data_ptr(), k * m, gy.data_ptr(), m,
                                       gw.data_ptr(), n, 5, k, m, torch.cuda.current_stream().cuda_stream), "dc_gmm_bwd_w")
    want = torch.einsum("ec,ekc->ek", gy[[1, 2]].double(), h[[0, 1]].double().view(2, k, m))
    assert (gw[2:] == 0).all() and rel_err(_np(gw[:2]), _np(want)) < TOL


@gpu
def test_entries_with_no_rows_and_with_no_edges():
    """N = 0: every entry returns 0 without a launch, ``gmm_aggregate`` an empty tensor that carries a gradient;
    N > 0 without any edge: y = base (or 0), every gradient a zero of the right shape; the checks of ``gmm_aggregate``"""
    m, k, d = 5, 3, 2
    mu = torch.rand(k, d, device=DEV, requires_grad=True)
    sg = torch.rand(k, d, device=DEV).add_(0.5).requires_grad_(True)
    h0 = torch.zeros((0, k * m), device=DEV, requires_grad=True)
    a0 = torch.zeros((0, d), device=DEV, requires_grad=True)
    y0 = ops.gmm_aggregate(None, h0, a0, mu, sg)
    assert y0.shape == (0, m) and y0.requires_grad
    y0.sum().backward()
    assert h0.grad.shape == (0, k * m) and a0.grad.shape == (0, d)
    assert mu.grad.shape == (k, d) and (mu.grad == 0).all() and (sg.grad == 0).all()
    n = 37
    g = GraphIndex(torch.zeros((2, 0), dtype=torch.int64, device=DEV), n, self_loops=False, normalize=False)
    h = torch.randn(n, k * m, device=DEV, requires_grad=True)
    base = torch.randn(n, m, device=DEV, requires_grad=True)
    mu.grad = sg.grad = a0.grad = None
    for reduce in AGGRS:
        assert (ops.gmm_aggregate(g, h, a0, mu, sg, reduce) == 0).all()
    y = ops.gmm_aggregate(g, h, a0, mu, sg, "mean", base)
    assert torch.equal(y, base)
    gy = torch.randn(n, m, device=DEV)
    torch.autograd.backward([y], [gy])
    assert torch.equal(base.grad, gy) and (h.grad == 0).all() and h.grad.shape == h.shape and a0.grad.shape == (0, d)
    assert (mu.grad == 0).all() and (sg.grad == 0).all() and mu.grad.shape == (k, d)
    hd, md, sd = h.detach(), mu.detach(), sg.detach()
    with pytest.raises(ValueError, match="rows"):
        ops.gmm_aggregate(g, hd, torch.zeros((3, d), device=DEV), md, sd)
    with pytest.raises(ValueError, match="None"):
        ops.gmm_aggregate(None, hd, a0.detach(), md, sd)
    with pytest.raises(ValueError):
        ops.gmm_aggregate(g, hd[:5], a0.detach(), md, sd)
    with pytest.raises(RuntimeError):
        ops.gmm_aggregate(g, hd, a0.detach(), md.cpu(), sd)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.gmm_aggregate(g, hd.cpu(), a0.detach(), md, sd)
    with pytest.raises(ValueError):
        ops.gmm_aggregate(GraphIndex(torch.zeros((2, 0), dtype=torch.int64, device=DEV), n, self_loops=True,
                                     normalize=False), hd, a0.detach(), md, sd)
    # a merged adjacency and a row window of one: their perm names merged edge ids, the kernels take no row offset
    ei2 = torch.tensor([[0, 1, 2], [1, 2, 0]], device=DEV)
    merged = GraphIndex.from_parts([(ei2, 3), (ei2, 3)], self_loops=False, normalize=False)
    for bad, rows in ((merged, merged.num_nodes), (merged.window(1), 3)):
        with pytest.raises(ValueError, match="merged"):
            ops.gmm_aggregate(bad, torch.zeros((rows, k * m), device=DEV),
                              torch.zeros((bad.num_input_edges, d), device=DEV), md, sd)


# --------------------------------------------------------------------------- #
# GPU: the layer
# --------------------------------------------------------------------------- #
def _device_gmm(case):
    fi, m, k, d = case["shape"]
    conv = dc.nn.GMMConv(fi, m, d, k, aggr=case["aggr"], root_weight=case["root_weight"], bias=case["bias"])
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
    conv = _device_gmm(case)
    got = _host(_device_run(conv, case["x"], case["ei"], case["ea"], case["gup"]))
    check_against_references(tag, got, case, "e_h")
    return conv, got


@gpu
@pytest.mark.parametrize("shape,aggr,kind", _layer_cases())
def test_layer_parity(shape, aggr, kind):
    """forward and the gradients of x, g, mu, sigma, root.weight, bias and edge_attr against RefGmm at 1e-5"""
    fi, m, k, d = shape
    case = gmm_case(fi, m, k, d, aggr, kind)
    _, got = _check_layer(case, f"GMMConv {fi}->{m} K={k} D={d} {aggr} {kind}")
    if m > 1:
        assert_parity(got[0], case["r32"][0], case["r64"][0], TOL, f"GMMConv {shape} {aggr} {kind} forward per row",
                      metric=row_rel_err)


@gpu
@pytest.mark.parametrize("variant", ["no_root", "no_bias", "no_root_no_bias", "flat_edge_attr"])
def test_layer_parity_variants(variant):
    kw = dict(no_root=dict(root_weight=False), no_bias=dict(bias=False), no_root_no_bias=dict(root_weight=False, bias=False),
              flat_edge_attr=dict(flat=True))[variant]
    shape = (16, 1, 1, 1) if variant == "flat_edge_attr" else (21, 64, 3, 3)
    case = gmm_case(*shape, "mean", "multigraph", **kw)
    assert (case["ea"].ndim == 1) == (variant == "flat_edge_attr")
    conv, got = _check_layer(case, f"GMMConv {shape} {variant}")
    assert ("root.weight" in got[1]) == case["root_weight"] and ("bias" in got[1]) == case["bias"]


@gpu
def test_edge_attr_without_a_gradient_skips_its_launch():
    case = gmm_case(21, 64, 3, 3, "mean", "multigraph")
    clear_cache()
    conv = _device_gmm(case)
    want = _device_run(conv, case["x"], case["ei"], case["ea"], case["gup"])
    for ea_grad, launches in ((True, 1), (False, 0)):
        _lib.kernel_trace(True)
        got = _device_run(conv, case["x"], case["ei"], case["ea"], case["gup"], ea_grad=ea_grad)
        counts = _lib.kernel_trace_counts()
        _lib.kernel_trace(False)
        gmm = {name: v for name, v in counts.items() if "k_gmm" in name}
        assert sum(v for name, v in gmm.items() if "k_gmm_bwd_a" in name) == launches, counts
        # one launch per kernel: weights, gather, g_h, g_w, the two passes of the [K, D] sums
        assert sum(gmm.values()) == 6 + launches and all(v == 1 for v in gmm.values()), counts
        assert not any("k_spmm" in name or "k_sage" in name or "k_gine" in name for name in counts), counts
        assert (got[1]["edge_attr"] is None) == (not ea_grad)
        for name in want[1]:
            if name != "edge_attr" or ea_grad:
                assert torch.equal(got[1][name], want[1][name]), name


@gpu
@pytest.mark.parametrize("kind", EDGE_GRAPHS)
@pytest.mark.parametrize("shape", [(21, 64, 3, 3), (16, 1, 1, 1)])
def test_layer_on_graphs_without_edges(shape, kind):
    """one node, no edge, no node: out = root(x) + bias (or an empty tensor); the gradients of edge_attr, mu and sigma
    are zeros of the right shapes"""
    fi, m, k, d = shape
    case = gmm_case(fi, m, k, d, "mean", kind)
    conv, got = _check_layer(case, f"GMMConv {shape} {kind}")
    out, grads = _device_run(conv, case["x"], case["ei"], case["ea"], case["gup"])
    assert out.shape == (case["n"], m) and grads["edge_attr"].shape == (0, d)
    assert grads["mu"].shape == (k, d) and (grads["mu"] == 0).all() and (grads["sigma"] == 0).all()
    assert grads["g"].shape == (fi, k * m) and (grads["g"] == 0).all()
    if case["n"]:
        with torch.no_grad():
            assert torch.equal(out, ops.dense_linear(_dev(case["x"]), conv.root.weight, conv.bias))


@gpu
@pytest.mark.parametrize("m", [64, 20])
def test_relu_fused_deferred_and_plain_agree(m):
    """``relu=True`` (in the gather's epilogue at M = 64, behind the layer at M = 20), the deferred
    ``F.relu(conv(x, ei, ea))`` and ``torch.relu`` of the plain output: the same bits; their gradients within 1e-5"""
    case = gmm_case(21, 64, 3, 3, "mean", "multigraph") if m == 64 else gmm_case(64, 20, 5, 3, "mean", "multigraph")
    clear_cache()
    conv = _device_gmm(case)
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
    case = gmm_case(25, 256, 2, 2, "mean", "multigraph")
    n, ei, x, ea, gup = case["n"], case["ei"], case["x"], case["ea"], case["gup"]
    clear_cache()
    conv = _device_gmm(case)
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
def test_a_captured_step_follows_mu_changed_in_place():
    """forward + backward on ONE stream under torch.cuda.graph (no host read anywhere); mu is then changed in place and
    the graph replayed: the replay equals the eager step at the new value - the kernels read mu and sigma through their
    device pointers - and differs from the step at the old one."""
    n, ei = _graph("multigraph", 12)
    fi, m, k, d = 32, 64, 3, 3                                   # (M = 64: the ReLU and its mask pass are captured too)
    torch.manual_seed(3)
    conv = dc.nn.GMMConv(fi, m, d, k).to(DEV)
    tei = torch.from_numpy(ei).to(DEV)
    rng = np.random.default_rng(1)
    static_x = _dev(rng.standard_normal((n, fi)).astype(np.float32)).requires_grad_(True)
    ea = _dev(rng.uniform(0, 1, (ei.shape[1], d)).astype(np.float32)).requires_grad_(True)
    gup = _dev(signed(rng, (n, m)))
    mus = [_dev(rng.uniform(0, 1, (k, d)).astype(np.float32)) for _ in range(2)]
    with torch.no_grad():
        conv.sigma.copy_(_dev(signed(rng, (k, d))))
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
    for mu in mus:
        with torch.no_grad():
            conv.mu.copy_(mu)
        clear_cache()
        eager.append(snapshot(step()))
    torch.cuda.synchronize()
    assert not torch.equal(eager[0][0], eager[1][0]) and not torch.equal(eager[0][1], eager[1][1])
    with torch.no_grad():
        conv.mu.copy_(mus[0])
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
            conv.mu.copy_(mus[which])
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(snapshot(out), eager[which]):
            assert torch.equal(got, want), which
