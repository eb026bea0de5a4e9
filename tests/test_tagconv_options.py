"""``nn.TAGConv(in, out, K, bias, normalize)`` away from its defaults: the host layer that turns ``(fi, K, fo, bias,
normalize)`` into kernel launches (``ops._TagConvFn`` and what it calls) at K = 0..3, ``bias=False`` and
``normalize=False``, against ``oracle/pyg_ref.TAGConv`` in fp32 and float64 at the bar of the layer parity tests
(``TOL`` = 1e-5, nothing ``special``).

* the dispatch table (``tag_slab_geometry`` / ``_dense_path`` / which backward) and the conditioning of every GPU case
  run without a GPU;
* layer parity forward + backward for every row of the table, with and without bias / ReLU / gcn_norm / input gradient,
  with the forward kernel family checked through the launch log;
* bit-identity with and without the hop chain and the fused pack, and of the narrow kernel with the split kernel;
* the alternative dense paths at K < 3, two-layer stacks with different K (``next_conv`` / deferred / learned geometry),
  the hop cache across K, ``precompute_input_hops``, the direct-gradient bucket with ``bias=False``;
* the edges of the contract: K = 4, no edges, one node, no nodes, ``GCNConv`` / ``GATConv`` with ``bias=False``."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deformcontact_amd as dc
from deformcontact_amd import _lib, ops
from deformcontact_amd.deferred import resolve
from deformcontact_amd.graph import clear_cache
from oracle import pyg_ref
from oracle.weights import fill_state_dict_, hashed_uniform
from tests.helpers import assert_parity, random_multigraph, rel_err, row_rel_err
from tests.test_hop_chain import batch_of_graphs

gpu = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda:0"

# fi, fo, K -> dense path, padded slab width, segments of the (generic) dense blocks, h2 backward?
# Read off the code (ops.tag_slab_geometry: concat <=> fi*(K+1) <= 128 or fi % 16 != 0, padded to a multiple of 16;
# dc_tag_linear_fwd_narrow_ok: Fo = 256, fi <= 32 and a padded width of 96 / 112 / 128; ops._tag_uses_h2).
TABLE = [
    (21, 256, 0, "concat", 32, 1, False), (21, 256, 1, "concat", 48, 1, False), (21, 256, 2, "concat", 64, 1, False),
    (32, 256, 2, "narrow", 96, 1, False),          # 3 segments of 32
    (30, 256, 2, "narrow", 96, 1, False),          # 90 padded to 96
    (24, 256, 3, "narrow", 96, 1, False), (28, 256, 3, "narrow", 112, 1, False),
    (32, 256, 1, "concat", 64, 1, False),          # 64 is no width of the narrow kernel
    (64, 256, 1, "concat", 128, 1, False),         # one segment of exactly 128; fi > 32: not narrow
    (40, 64, 1, "concat", 80, 1, False),           # 80 is a multiple of 16 already: no padding
    (40, 64, 2, "concat", 128, 1, False),          # 120 padded to 128
    (72, 64, 1, "concat", 144, 1, False),          # beyond 128 columns: concatenated because fi % 16 != 0 alone
    (72, 64, 2, "concat", 224, 1, False),          # 216 padded to 224
    (64, 256, 2, "h2", 192, 3, True), (256, 256, 1, "h2", 512, 2, True), (256, 256, 2, "h2", 768, 3, True),
    (64, 24, 2, "h2", 192, 3, False), (48, 3, 3, "h2", 192, 4, False),      # fo % 16 != 0: generic backward, K+1 segments
    (144, 32, 1, "h2", 288, 2, True),              # F % 32 != 0: never the hop chain
    (256, 256, 0, "h2", 256, 1, True),             # the K = 0 rule; the input is the slab; rowabsmax pass
    (256, 3, 0, "split", 256, 1, False),           # one segment; not concat, not h2
    (144, 64, 0, "split", 144, 1, False),          # K = 0 with fi % 32 != 0: not h2 either
]
ROWS = [t[:3] for t in TABLE]
ROW = {t[:3]: t[3:] for t in TABLE}
NS = (208, 203)                                    # dc_tag_linear_bwd_dw_h2 runs only where n % 16 == 0
# normalize=False / x without gradient: one row per path (concat with one and two hops, narrow, h2 with either backward)
UNNORMALIZED = [(21, 256, 1), (21, 256, 2), (32, 256, 2), (256, 256, 2), (64, 24, 2)]
NO_XGRAD = [(21, 256, 1), (32, 256, 2), (256, 256, 1), (64, 24, 2), (256, 256, 0), (256, 3, 0)]
# forward kernel family per path, by the names in the launch log
FAMILY = {"concat": "k_fwd_split", "split": "k_fwd_split", "narrow": "k_fwd_narrow", "h2": "k_fwd_h2"}
FAMILIES = ("k_fwd_split", "k_fwd_narrow", "k_fwd_h2", "k_tag_linear_fwd", "k_fwd_fast")
_HOPS = ("k_spmm", "k_hop_chain", "k_pack_input")


def _np(t):
    return t.detach().cpu().numpy()


def _narrow_ok(fi, k, fo):
    concat, _, wpad = ops.tag_slab_geometry(fi, k)
    return concat and bool(_lib.lib().dc_tag_linear_fwd_narrow_ok(fi, k + 1, wpad, fo))


# --------------------------------------------------------------------------- #
# the oracle, fp32 and float64, computed once per case
# --------------------------------------------------------------------------- #
def _evaluate(model, x, ei, gup, relu, dtype, xgrad=True):
    m = copy.deepcopy(model).to(dtype)
    m.zero_grad()
    xt = torch.from_numpy(x).to(dtype).requires_grad_(xgrad)
    out = m(xt, torch.from_numpy(ei))
    if relu:
        out = F.relu(out)
    (out * torch.from_numpy(gup).to(dtype)).sum().backward()
    return {"out": _np(out), "gx": _np(xt.grad) if xgrad else None,
            "grads": {k: _np(p.grad) for k, p in m.named_parameters()}}


def _conv_oracle(kind, fi, fo, n, relu, seed, **kw):
    torch.set_num_threads(1)
    ei = random_multigraph(n, 8 * n, seed)
    x = hashed_uniform((n, fi), 31, 2.0)
    gup = hashed_uniform((n, fo), 37, 2.0)
    cpu = getattr(pyg_ref, kind)(fi, fo, **kw)
    fill_state_dict_(cpu, salt0=fi)
    if fo == 3:
        _tilt_(cpu, x)
    return {"ei": ei, "x": x, "gup": gup, "state": cpu.state_dict(),
            "r32": _evaluate(cpu, x, ei, gup, relu, torch.float32), "r64": _evaluate(cpu, x, ei, gup, relu, torch.float64)}


def _tilt_(module, x):
    """Three output columns with zero-mean inputs and weights: among 200 rows one has a largest entry near 1 % of the
    tensor's scale (less behind a ReLU), and the per-row metric magnifies fp32 rounding 60 to 100 times there - the
    fp32 oracle alone then lands on either side of TOL / 2 from one host's BLAS to the next.  So these cases shift
    ``x`` to [0, 2) and the weight rows by (+1, -1, 0) / sqrt(fan_in): column 0 is large and positive in every row,
    column 1 negative (the ReLU cuts it), column 2 of either sign."""
    x += 1.0
    with torch.no_grad():
        for p in module.parameters():
            if p.dim() == 2:
                t = 1.0 / np.sqrt(p.shape[1])
                p[0] += t
                p[1] -= t


@functools.lru_cache(maxsize=None)
def _tag_oracle(fi, fo, k, n, bias, relu, normalize):
    return _conv_oracle("TAGConv", fi, fo, n, relu, n + fi + fo + k, K=k, bias=bias, normalize=normalize)


@functools.lru_cache(maxsize=None)
def _other_oracle(kind, fi, fo, relu):
    return _conv_oracle(kind, fi, fo, 120, relu, fi + fo, bias=False)


class _Stack(torch.nn.Module):
    """``relu(c2(relu(c1(x))))``: two TAGConv layers as the reference's encoder loops chain them."""

    def __init__(self, mod, a, b):
        super().__init__()
        self.c1, self.c2 = mod.TAGConv(a[0], a[1], K=a[2]), mod.TAGConv(b[0], b[1], K=b[2])

    def forward(self, x, ei):
        return self.c2(F.relu(self.c1(x, ei)), ei)


@functools.lru_cache(maxsize=None)
def _tiny_oracle(k, n, loops, bias, relu):
    """TAGConv(16, 8, K=k) on ``n`` nodes whose only edges are ``loops`` self loops of node 0."""
    torch.set_num_threads(1)
    fi, fo = 16, 8
    ei = np.zeros((2, loops), np.int64)
    x, gup = hashed_uniform((n, fi), 31, 2.0), hashed_uniform((n, fo), 37, 2.0)
    cpu = pyg_ref.TAGConv(fi, fo, K=k, bias=bias)
    fill_state_dict_(cpu, salt0=fi)
    return {"ei": ei, "x": x, "gup": gup, "state": cpu.state_dict(),
            "r32": _evaluate(cpu, x, ei, gup, relu, torch.float32), "r64": _evaluate(cpu, x, ei, gup, relu, torch.float64)}


STACKS = [((21, 64, 3), (64, 32, 1)), ((21, 256, 1), (256, 256, 2))]
STACK_N = 203


@functools.lru_cache(maxsize=None)
def _stack_oracle(a, b):
    torch.set_num_threads(1)
    n = STACK_N
    ei = random_multigraph(n, 8 * n, a[0] + b[1])
    x = hashed_uniform((n, a[0]), 31, 2.0)
    gup = hashed_uniform((n, b[1]), 37, 2.0)
    cpu = _Stack(pyg_ref, a, b)
    fill_state_dict_(cpu, salt0=a[0])
    return {"ei": ei, "x": x, "gup": gup, "state": cpu.state_dict(),
            "r32": _evaluate(cpu, x, ei, gup, True, torch.float32), "r64": _evaluate(cpu, x, ei, gup, True, torch.float64)}


def _conditioned(o, what):
    """The fp32 oracle alone within TOL / 2 of float64 on everything a GPU case compares: else the case could not
    tell a wrong kernel from a badly conditioned sum."""
    r32, r64 = o["r32"], o["r64"]
    d = {"out": rel_err(r32["out"], r64["out"]), "out rows": row_rel_err(r32["out"], r64["out"]),
         "gx": rel_err(r32["gx"], r64["gx"])}
    d.update({k: rel_err(v, r64["grads"][k]) for k, v in r32["grads"].items()})
    bad = {k: v for k, v in d.items() if not v < TOL / 2}
    assert not bad, (what, bad)


# --------------------------------------------------------------------------- #
# 1. dispatch table and conditioning: no GPU
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("fi,fo,k", ROWS)
def test_dispatch_table(fi, fo, k):
    path, wpad, nseg, bwd_h2 = ROW[(fi, fo, k)]
    assert (ops.DENSE_SPLIT_BF16, ops.DENSE_F16X2, ops.NARROW_FWD, ops.DENSE_PRODUCTS) == (True, True, True, 6)
    concat = path in ("concat", "narrow")
    assert ops.tag_slab_geometry(fi, k) == (concat, (k + 1) * fi, wpad)
    assert _narrow_ok(fi, k, fo) == (path == "narrow")
    got = ops._dense_path(fi, k, fo, False, _narrow_ok(fi, k, fo))
    assert got == path
    assert (got == "h2" and fo % 16 == 0) == bwd_h2
    # segments of the generic dense blocks (forward of "concat" / "split", dW and dX of everything but the h2 backward)
    slab = torch.empty(1, wpad)
    assert ops._dense_operands(slab, fi, k, concat)[3] == nseg == (1 if concat else k + 1)
    assert ops._tag_uses_h2(fi, k, fo) == (path == "h2")
    if k >= 1:
        assert ops._tag_uses_h2(fi, k) == (path == "h2")      # what precompute_input_hops asks: the same answer


def test_dispatch_table_coverage():
    """Every path twice at K < 3, both backward forms at K = 1 and at K = 2 - with the default switches."""
    for path in ("concat", "narrow", "h2", "split"):
        assert sum(1 for t in TABLE if t[3] == path and t[2] < 3) >= 2, path
    for k in (1, 2):
        assert {t[6] for t in TABLE if t[2] == k} == {True, False}, k
    for rows in (UNNORMALIZED, NO_XGRAD):
        assert {ROW[r][0] for r in rows} >= {"concat", "narrow", "h2"}
        assert {ROW[r][3] for r in rows if ROW[r][0] == "h2"} == {True, False}
    assert "split" in {ROW[r][0] for r in NO_XGRAD}


@pytest.mark.parametrize("fi,fo,k", ROWS)
def test_oracle_conditioning_of_the_layer_cases(fi, fo, k):
    for n in NS:
        for bias in (True, False):
            for relu in (False, True):
                _conditioned(_tag_oracle(fi, fo, k, n, bias, relu, True), (n, bias, relu))
        if (fi, fo, k) in UNNORMALIZED:
            for relu in (False, True):
                _conditioned(_tag_oracle(fi, fo, k, n, n == 208, relu, False), (n, relu, "normalize=False"))


def test_oracle_conditioning_of_the_other_cases():
    for a, b in STACKS:
        _conditioned(_stack_oracle(a, b), (a, b))
    for kind in ("GCNConv", "GATConv"):
        for f in (32, 256):
            for relu in (False, True):
                _conditioned(_other_oracle(kind, f, f, relu), (kind, f, relu))
    for bias in (True, False):
        _conditioned(_tiny_oracle(0, 5, 0, bias, False), "no edges")
    _conditioned(_tiny_oracle(2, 1, 1, True, True), "one node")


# --------------------------------------------------------------------------- #
# running a layer on the GPU, comparing it with its oracle
# --------------------------------------------------------------------------- #
def _traced(fn):
    """``fn()`` with the launch log on -> (result, {kernel name: launches})."""
    _lib.kernel_trace(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, _lib.kernel_trace_counts()
    finally:
        _lib.kernel_trace(False)


def _launched(trace, *prefixes):
    return sorted(k for k in trace if k.startswith(prefixes))


def _run_layer(conv, o, relu, xgrad=True, keep=None):
    """Forward (``relu=True``: the fused epilogue; else the plain PyG call, resolved) and backward of ``conv`` on the
    oracle's inputs -> (out, x.grad, {name: grad}, forward launches), on the host.  ``keep``: a dict that holds the
    device tensors from one call to the next (the caches key on the tensors themselves)."""
    conv.zero_grad(set_to_none=True)
    keep = {} if keep is None else keep
    if "x" not in keep:
        keep["x"] = torch.from_numpy(o["x"]).to(DEV).requires_grad_(xgrad)
        keep["ei"] = torch.from_numpy(o["ei"]).to(DEV)
    xg, eig = keep["x"], keep["ei"]
    xg.grad = None
    og, fwd = _traced(lambda: conv(xg, eig, relu=True) if relu else resolve(conv(xg, eig)))
    (og * torch.from_numpy(o["gup"]).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return _np(og), (_np(xg.grad) if xgrad else None), {k: _np(p.grad) for k, p in conv.named_parameters()}, fwd


def _device_conv(kind, fi, fo, o, **kw):
    conv = getattr(dc.nn, kind)(fi, fo, **kw)
    conv.load_state_dict(o["state"])
    return conv.to(DEV)


def _compare(got, o, tag, xgrad=True):
    """The bar of ``test_conv_forward_backward_vs_oracle``: TOL vs the fp32 oracle, else TOL vs float64."""
    out, gx, grads, _ = got
    r32, r64 = o["r32"], o["r64"]
    assert_parity(out, r32["out"], r64["out"], TOL, f"{tag}/forward")
    assert_parity(out, r32["out"], r64["out"], TOL, f"{tag}/per-row forward", metric=row_rel_err)
    if xgrad:
        assert_parity(gx, r32["gx"], r64["gx"], TOL, f"{tag}/x.grad")
    assert set(grads) == set(r32["grads"])
    for name, g in grads.items():
        assert_parity(g, r32["grads"][name], r64["grads"][name], TOL, f"{tag}/{name}")


def _same_bits(a, b):
    assert np.array_equal(a[0], b[0]), "outputs differ"
    assert (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1])), "x.grad differs"
    assert set(a[2]) == set(b[2])
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), f"{k}.grad differs"


def _tag_case(fi, fo, k, n, bias, relu, normalize, xgrad=True, family=None, tag=None, keep=None):
    o = _tag_oracle(fi, fo, k, n, bias, relu, normalize)
    conv = _device_conv("TAGConv", fi, fo, o, K=k, bias=bias, normalize=normalize)
    assert (conv.bias is None) == (not bias) and len(conv.lins) == k + 1
    clear_cache()
    got = _run_layer(conv, o, relu, xgrad, keep)
    path = ROW[(fi, fo, k)][0]
    family = FAMILY[path] if family is None else family
    ran = _launched(got[3], *FAMILIES)
    assert ran and all(r.startswith(family) for r in ran), (family, got[3])
    _compare(got, o, tag or path, xgrad)
    return conv, o, got


# --------------------------------------------------------------------------- #
# 2. layer parity, forward and backward
# --------------------------------------------------------------------------- #
@gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("fi,fo,k", ROWS)
def test_layer_vs_oracle(fi, fo, k, n, bias, relu):
    _tag_case(fi, fo, k, n, bias, relu, True)


@gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("fi,fo,k", UNNORMALIZED)
def test_layer_without_gcn_norm_vs_oracle(fi, fo, k, n, relu):
    _, _, got = _tag_case(fi, fo, k, n, n == 208, relu, False, tag=ROW[(fi, fo, k)][0] + " normalize=False")
    assert _launched(got[3], "k_pack_input"), got[3]     # the fused pack + first hop applies gcn_norm weights: bypassed


@gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("fi,fo,k", NO_XGRAD)
def test_layer_on_an_input_without_gradient_vs_oracle(fi, fo, k, n):
    """The first layer of a branch: the hop slab comes from the cache on the second call, and the h2 backward forms no
    transposed weight image (``wt is None``).  Both calls: same bits, same parity."""
    keep = {}
    conv, o, first = _tag_case(fi, fo, k, n, n == 203, True, True, xgrad=False, keep=keep)
    assert bool(_launched(first[3], *_HOPS)) == (k >= 1), first[3]
    again = _run_layer(conv, o, True, False, keep)
    assert not _launched(again[3], *_HOPS), again[3]
    _compare(again, o, ROW[(fi, fo, k)][0] + " cached", xgrad=False)
    _same_bits(first, again)


# --------------------------------------------------------------------------- #
# 3. chain and no chain, fused pack and not: bitwise
# --------------------------------------------------------------------------- #
def _batch():
    return batch_of_graphs((300, 1, 0, 129, 64), (6, 2, 0, 5, 3), seed=11, hub=(0, 45))


def _tag_conv_run(conv, g, x0, gup):
    """``ops.tag_conv`` + backward on a graph with a known layout -> (out, x.grad, grads, launches)."""
    conv.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_(True)

    def step():
        out = ops.tag_conv(g, x, [lin.weight for lin in conv.lins], conv.bias, relu=True)
        (out * gup).sum().backward()
        return out
    out, trace = _traced(step)
    return _np(out), _np(x.grad), {k: _np(p.grad) for k, p in conv.named_parameters()}, trace


def _switch_pair(name, k, f, fo, normalize):
    """One layer over the batch with the module switch ``name`` on, then off (fresh adjacency each time)."""
    ei, segs = _batch()
    n = segs[0][-1]
    ei = ei.to(DEV)
    torch.manual_seed(k + f)
    conv = dc.nn.TAGConv(f, fo, K=k, normalize=normalize).to(DEV)
    with torch.no_grad():
        conv.bias.uniform_(-0.3, 0.3)
    x0 = torch.randn(n, f, device=DEV)
    gup = torch.randn(n, fo, device=DEV)
    keep = getattr(ops, name)
    runs = []
    try:
        for on in (True, False):
            setattr(ops, name, on)
            clear_cache()
            g = conv.graph(ei, n, segments=segs)
            assert g._layout is not None and g.normalize == normalize
            runs.append(_tag_conv_run(conv, g, x0, gup))
    finally:
        setattr(ops, name, keep)
        clear_cache()
    return runs


@gpu
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("f", [32, 64, 256])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_layer_identical_with_and_without_the_hop_chain(k, f, normalize):
    on, off = _switch_pair("HOP_CHAIN", k, f, 64, normalize)
    fused_pack = ops.FUSED_PACK and f <= 32 and normalize            # pack + first hop in one launch: no forward chain
    assert bool(_launched(on[3], "k_hop_chain")) == (not fused_pack), on[3]
    assert not _launched(off[3], "k_hop_chain"), off[3]
    _same_bits(on, off)


@gpu
@pytest.mark.parametrize("f", [21, 32])
@pytest.mark.parametrize("k", [1, 2])
def test_layer_identical_with_and_without_the_fused_pack(k, f):
    on, off = _switch_pair("FUSED_PACK", k, f, 256, True)
    assert _launched(off[3], "k_pack_input") and not _launched(on[3], "k_pack_input"), (on[3], off[3])
    _same_bits(on, off)


# --------------------------------------------------------------------------- #
# 4. the alternative dense paths at K < 3
# --------------------------------------------------------------------------- #
class _switches:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.saved = {k: getattr(ops, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(ops, k, v)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            setattr(ops, k, v)


@gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("fi,fo,k", [(256, 256, 1), (64, 24, 2)])
def test_six_product_split_with_two_and_three_segments_vs_oracle(fi, fo, k, n):
    with _switches(DENSE_F16X2=False):
        assert ops._dense_path(fi, k, fo, False, _narrow_ok(fi, k, fo)) == "split"
        _tag_case(fi, fo, k, n, n == 208, True, True, family="k_fwd_split", tag="split (DENSE_F16X2 off)")


@gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("fi,fo,k", [(256, 256, 1), (64, 24, 2), (21, 256, 1)])
def test_fp32_mfma_path_vs_oracle(fi, fo, k, n):
    with _switches(DENSE_SPLIT_BF16=False):
        assert ops._dense_path(fi, k, fo, False, _narrow_ok(fi, k, fo)) == "fp32"
        _tag_case(fi, fo, k, n, n == 208, True, True, family=("k_tag_linear_fwd", "k_fwd_fast"),
                  tag="fp32 (DENSE_SPLIT_BF16 off)")


@gpu
@pytest.mark.parametrize("bias", [True, False])
def test_narrow_kernel_identical_to_the_split_kernel_at_three_segments(bias):
    conv, o, narrow = _tag_case(32, 256, 2, 203, bias, True, True)
    with _switches(NARROW_FWD=False):
        clear_cache()
        split = _run_layer(conv, o, True)
    assert _launched(split[3], "k_fwd_split") and not _launched(split[3], "k_fwd_narrow"), split[3]
    _same_bits(narrow, split)


# --------------------------------------------------------------------------- #
# 5. stacks and caches
# --------------------------------------------------------------------------- #
@gpu
@pytest.mark.parametrize("a,b", STACKS)
def test_two_layers_with_different_k_vs_oracle(a, b):
    o = _stack_oracle(a, b)
    ei = torch.from_numpy(o["ei"]).to(DEV)
    gup = torch.from_numpy(o["gup"]).to(DEV)
    geom = ops.tag_slab_geometry(b[0], b[2])[1:]

    def fresh():
        m = _Stack(dc.nn, a, b)
        m.load_state_dict(o["state"])
        return m.to(DEV)

    def run(m, call):
        m.zero_grad(set_to_none=True)
        x = torch.from_numpy(o["x"]).to(DEV).requires_grad_(True)
        h, y = call(m, x)
        (y * gup).sum().backward()
        torch.cuda.synchronize()
        in_slab = h._base is not None and getattr(h._base, ops._SLAB_TAG, None) == (STACK_N, b[0], geom[1])
        return (_np(y), _np(x.grad), {k: _np(p.grad) for k, p in m.named_parameters()}, None), in_slab

    def handed(m, x):
        h = m.c1(x, ei, relu=True, next_conv=m.c2)
        return h, m.c2(h, ei, relu=True)

    def plain(m, x):
        h = F.relu(m.c1(x, ei))
        return h, F.relu(m.c2(h, ei))

    clear_cache()
    with_next, in_slab = run(fresh(), handed)
    assert in_slab, "next_conv= must put the output into block 0 of the consumer's slab"
    m = fresh()
    first, in_slab = run(m, plain)
    assert not in_slab and m.c1._consumer_geom == {True: geom} and m.c2._consumer_geom == {}
    learned, in_slab = run(m, plain)
    assert in_slab, "the second step must write into the slab geometry the consumer reported"
    for got, tag in ((with_next, "next_conv"), (first, "deferred"), (learned, "learned geometry")):
        _compare(got, o, f"stack K={a[2]},{b[2]} {tag}")
    _same_bits(with_next, learned)


@gpu
@pytest.mark.parametrize("fi", [21, 32, 256])
def test_hop_cache_keeps_layers_of_different_k_apart(fi):
    """K = 1 and K = 2 over the same no-grad ``x`` and ``edge_index``: each slab is its own cache entry."""
    n = 203
    ei = torch.from_numpy(random_multigraph(n, 8 * n, fi)).to(DEV)
    x = torch.from_numpy(hashed_uniform((n, fi), 3, 2.0)).to(DEV)
    torch.manual_seed(fi)
    convs = [dc.nn.TAGConv(fi, 64, K=k).to(DEV) for k in (1, 2)]
    clear_cache()
    with torch.no_grad():
        for order in (convs, convs[::-1]):
            shared = [[c(x, ei, relu=True).clone() for c in order] for _ in range(2)]     # second round: cache hits
            g = convs[0].graph(ei, n)
            assert sorted(key[3] for key in g._hop_cache) == [1, 2] and len({key[4] for key in g._hop_cache}) == 2
            for i, c in enumerate(order):
                clear_cache()
                alone = c(x, ei, relu=True).clone()
                assert torch.equal(shared[0][i], alone) and torch.equal(shared[1][i], alone), (c.K, i)
            clear_cache()


@gpu
@pytest.mark.parametrize("fi", [21, 256])
@pytest.mark.parametrize("k", [1, 2])
def test_precompute_input_hops_then_the_layer(k, fi):
    n = 208
    ei = torch.from_numpy(random_multigraph(n, 8 * n, fi + k)).to(DEV)
    x = torch.from_numpy(hashed_uniform((n, fi), 3, 2.0)).to(DEV)
    torch.manual_seed(fi + k)
    conv = dc.nn.TAGConv(fi, 256, K=k).to(DEV)
    clear_cache()
    _, built = _traced(lambda: ops.precompute_input_hops(conv.graph(ei, n), x, k))
    assert _launched(built, *_HOPS), built
    y, trace = _traced(lambda: conv(x, ei, relu=True))
    assert not _launched(trace, *_HOPS), trace
    clear_cache()
    alone, trace = _traced(lambda: conv(x, ei, relu=True))
    assert _launched(trace, *_HOPS), trace
    assert torch.equal(y, alone)
    clear_cache()


@gpu
def test_direct_gradient_bucket_without_bias():
    """``dp.GradBucket(direct=True)`` over two layers that have no bias parameter: the dW kernels accumulate into the
    bucket; two backward passes leave twice the gradients autograd returns."""
    from deformcontact_amd import dp
    n = 208
    ei = torch.from_numpy(random_multigraph(n, 8 * n, 17)).to(DEV)
    x = torch.from_numpy(hashed_uniform((n, 21), 3, 2.0)).to(DEV)
    gup = torch.from_numpy(hashed_uniform((n, 256), 4, 2.0)).to(DEV)
    torch.manual_seed(5)
    c1 = dc.nn.TAGConv(21, 256, K=1, bias=False).to(DEV)
    c2 = dc.nn.TAGConv(256, 256, K=2, bias=False).to(DEV)
    params = dict([("c1." + k, p) for k, p in c1.named_parameters()] + [("c2." + k, p) for k, p in c2.named_parameters()])
    assert len(params) == 5 and not any("bias" in k for k in params)

    def run():
        (c2(c1(x, ei, relu=True, next_conv=c2), ei, relu=True) * gup).sum().backward()

    clear_cache()
    run()
    ref = {k: p.grad.clone() for k, p in params.items()}
    bucket = dp.GradBucket(params.values(), direct=True)
    bucket.zero()
    ptrs = {k: p.grad.data_ptr() for k, p in params.items()}
    for step in (1, 2):
        run()
        assert bucket._pending, "direct writes must be reported to the bucket"
        bucket.wait_direct_writes()
        torch.cuda.synchronize()
        for k, p in params.items():
            assert p.grad.data_ptr() == ptrs[k], "direct mode must write in place"
            assert rel_err(_np(p.grad), step * _np(ref[k])) < 1e-6, (k, step)
    clear_cache()


# --------------------------------------------------------------------------- #
# 6. edges of the contract
# --------------------------------------------------------------------------- #
@gpu
def test_k_beyond_three_raises_before_anything_is_launched():
    conv = dc.nn.TAGConv(8, 8, K=4).to(DEV)
    x = torch.randn(20, 8, device=DEV)
    ei = torch.from_numpy(random_multigraph(20, 60, 1)).to(DEV)
    clear_cache()
    torch.cuda.synchronize()
    for call in (lambda: conv(x, ei, relu=True), lambda: resolve(conv(x, ei))):
        _lib.kernel_trace(True)
        try:
            with pytest.raises(NotImplementedError, match="K=4"):
                call()
            assert _lib.kernel_trace_counts() == {}
        finally:
            _lib.kernel_trace(False)


@gpu
@pytest.mark.parametrize("bias", [True, False])
def test_k0_on_an_empty_edge_set(bias):
    o = _tiny_oracle(0, 5, 0, bias, False)
    conv = _device_conv("TAGConv", 16, 8, o, K=0, bias=bias)
    _compare(_run_layer(conv, o, False), o, "K=0, no edges")


@gpu
def test_k2_on_one_node_with_a_self_loop():
    o = _tiny_oracle(2, 1, 1, True, True)
    _compare(_run_layer(_device_conv("TAGConv", 16, 8, o, K=2), o, True), o, "K=2, one node")


@gpu
@pytest.mark.parametrize("fi,fo,k", [(21, 256, 1), (32, 256, 2), (256, 256, 2), (64, 24, 2), (256, 256, 0), (256, 3, 0)])
def test_no_rows(fi, fo, k):
    """n = 0: an empty output, an empty ``x.grad`` and zero parameter gradients, as the oracle gives."""
    conv = dc.nn.TAGConv(fi, fo, K=k).to(DEV)
    ei = torch.zeros((2, 0), dtype=torch.int64, device=DEV)
    for relu in (True, False):
        conv.zero_grad(set_to_none=True)
        x = torch.zeros((0, fi), device=DEV, requires_grad=True)
        out = conv(x, ei, relu=True) if relu else resolve(conv(x, ei))
        assert out.shape == (0, fo)
        out.sum().backward()
        torch.cuda.synchronize()
        assert x.grad.shape == (0, fi)
        for name, p in conv.named_parameters():
            assert p.grad is not None and p.grad.shape == p.shape and not p.grad.any(), name


@gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("f", [32, 256])
@pytest.mark.parametrize("kind", ["GCNConv", "GATConv"])
def test_gcn_and_gat_without_bias_vs_oracle(kind, f, relu):
    o = _other_oracle(kind, f, f, relu)
    conv = _device_conv(kind, f, f, o, bias=False)
    assert conv.bias is None and "bias" not in dict(conv.named_parameters())
    clear_cache()
    _compare(_run_layer(conv, o, relu), o, f"{kind} bias=False")
