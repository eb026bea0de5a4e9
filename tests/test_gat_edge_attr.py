"""``GATConv(edge_dim=D)`` / ``conv(x, edge_index, edge_attr)``: the layer, its autograd Functions, the C entries of
dc_gat_edge.hip (and the two softmax entries with the per-edge addend in dc_gat_heads.hip), ``Batch`` with ``edge_attr``.

The truth lives here (``oracle/`` has no edge features): ``np_layer`` restates the whole layer in numpy the PyG way -
explicit ``lin_edge`` projection to [E', H, C], remove / add self loops with the ``fill_value`` attribute, segment softmax,
hand-written backward - dtype-parametrised (float32: ``ref32``, float64: ``truth64``); ``torch_layer`` restates it in torch
double through the folded ``M`` [D, H] with autograd.  On the CPU the two must agree to ~1e-12, outputs and every gradient:
that pins the truth and proves the fold.  GPU comparisons go through ``helpers.assert_parity`` at 1e-5, nothing wider,
nothing ``special``; the per-edge entries are compared with the per-segment metric and under the conditioning rules of
``tests/test_gat_edge_kernels.py`` (value parity of ``ge``-derived quantities where a segment's logits spread over a few
units; one-signed operands where a sum of mixed-sign products could cancel to nothing).
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deformcontact_amd as dc
from deformcontact_amd import _lib, ops
from deformcontact_amd.data import Batch, Data
from deformcontact_amd.graph import GraphIndex, _segment_arrays, clear_cache
from tests.helpers import assert_parity, load_golden, random_multigraph, rel_err, row_rel_err
from tests.test_gat_edge_kernels import (BWD_CASES, _dev, _np, _seg_sum, check_g_a_dst, device_graph, galpha_for,
                                         seg_of, seg_rel_err_on)
from tests.test_gat_heads import SHAPES, _graph, heads_galpha, heads_logits

gpu = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
SLOPE = float(np.float32(0.2))
PARAMS = ("lin.weight", "att_src", "att_dst", "lin_edge.weight", "att_edge", "bias")

#: (shape of test_gat_heads.SHAPES, edge_dim): fused and unfused widths, H = 1, concat=False; D in {1, 3, 4, 7, 32}
LAYER_CASES = [((256, 4, 64, True), 3), ((64, 3, 20, True), 7), ((32, 1, 64, False), 1), ((256, 4, 64, False), 32),
               ((32, 5, 3, True), 4), ((256, 8, 32, True), 32), ((64, 3, 20, False), 1)]
assert all(s in SHAPES for s, _ in LAYER_CASES)
GRAPHS = ["multigraph", "hub", "n1", "e0", "golden_rest", "golden_rig"]
#: (relu, fill_value)
MODES = [(False, "mean"), (True, 0.5), (True, "mean"), (False, -1.25)]


# --------------------------------------------------------------------------- #
# inputs and the two restatements
# --------------------------------------------------------------------------- #
def make_params(fi, nh, c, d, concat, seed):
    """float32 parameters, PyG initialisers (glorot everywhere, a non-zero bias so that its gradient path is seen)"""
    rng = np.random.default_rng(seed)
    u = lambda shape, a: rng.uniform(-a, a, shape).astype(np.float32)
    att = np.sqrt(6.0 / (nh + c))
    return {"lin.weight": u((nh * c, fi), np.sqrt(6.0 / (fi + nh * c))), "att_src": u((1, nh, c), att),
            "att_dst": u((1, nh, c), att), "lin_edge.weight": u((nh * c, d), np.sqrt(6.0 / (d + nh * c))),
            "att_edge": u((1, nh, c), att), "bias": u((nh * c if concat else c,), 0.3)}


def make_inputs(kind, fi, nh, c, d, concat, seed):
    n, ei = _graph(kind, seed)
    rng = np.random.default_rng(seed + fi + nh + c + d)
    x = rng.uniform(-1, 1, (n, fi)).astype(np.float32)
    ea = rng.uniform(-1, 1, (ei.shape[1], d)).astype(np.float32)
    gup = rng.uniform(0.5, 1.5, (n, nh * c if concat else c)).astype(np.float32)
    return n, ei, x, ea, gup


def loop_fill(n, dst_k, ea_k, fill, dt):
    """(attribute rows of the appended loops [n, D], in-edge counts): the mean of the kept rows into each node, summed in
    input order (= the destination-sorted order inside a segment: the sort is stable), or the constant"""
    cnt = np.bincount(dst_k, minlength=n)
    if fill != "mean":
        return np.full((n, ea_k.shape[1]), fill, dt), cnt
    la = np.zeros((n, ea_k.shape[1]), dt)
    np.add.at(la, dst_k, ea_k.astype(dt))
    return np.where(cnt[:, None] > 0, la / np.maximum(cnt, 1).astype(dt)[:, None], dt(0)), cnt


def seg_total(v, dst, n):
    """per-destination sums of the rows of v [E', H], each by numpy's pairwise ``sum`` (``_seg_sum`` of
    test_gat_edge_kernels.py: a running fp32 sum over a 5,000-edge hub of near-equal terms drifts past the bar by itself)"""
    order = np.argsort(dst, kind="stable")
    ptr = np.searchsorted(dst[order], np.arange(n + 1))
    vt = np.ascontiguousarray(v[order].T)
    return np.stack([vt[:, ptr[i]:ptr[i + 1]].sum(1, dtype=v.dtype) for i in range(n)])


def np_layer(x, ei, ea, P, nh, c, concat, fill, relu, gup, dt, use_edge=True):
    """The layer the PyG way in dtype ``dt``: (out, {gradient name: array}) with 'x' and 'edge_attr' among the names."""
    n, d = len(x), ea.shape[1]
    x, ea, gup = x.astype(dt), ea.astype(dt), gup.astype(dt)
    W, a_s, a_d = P["lin.weight"].astype(dt), P["att_src"].astype(dt)[0], P["att_dst"].astype(dt)[0]
    We, a_e, b = P["lin_edge.weight"].astype(dt), P["att_edge"].astype(dt)[0], P["bias"].astype(dt)
    slope = dt(np.float32(0.2))
    keep = ei[0] != ei[1]                                              # remove_self_loops, rows of edge_attr with them
    src_k, dst_k, ea_k = ei[0][keep], ei[1][keep], ea[keep]
    la, cnt = loop_fill(n, dst_k, ea_k, fill, dt)                      # add_self_loops(fill_value)
    src, dst = np.concatenate([src_k, np.arange(n)]), np.concatenate([dst_k, np.arange(n)])
    eal = np.concatenate([ea_k, la])
    h = (x @ W.T).reshape(n, nh, c)
    al_s, al_d = (h * a_s).sum(-1), (h * a_d).sum(-1)
    he = (eal @ We.T).reshape(len(eal), nh, c)                         # lin_edge(edge_attr) as [E', H, C]
    al_e = (he * a_e).sum(-1) if use_edge else np.zeros((len(eal), nh), dt)
    s = (al_s[src] + al_d[dst]) + al_e
    e = np.where(s > 0, s, slope * s)
    m = np.full((n, nh), -np.inf, dt)
    np.maximum.at(m, dst, e)
    ex = np.exp(e - m[dst])
    alpha = ex / (seg_total(ex, dst, n) + dt(1e-16))[dst]
    agg = np.zeros((n, nh, c), dt)
    np.add.at(agg, dst, alpha[:, :, None] * h[src])
    out = (agg.reshape(n, nh * c) if concat else agg.mean(1, dtype=dt)) + b
    if relu:
        out = np.maximum(out, dt(0))
    # backward
    go = gup * (out > 0) if relu else gup
    gagg = go.reshape(n, nh, c) if concat else np.repeat(go[:, None, :] / dt(nh), nh, 1)
    galpha = (gagg[dst] * h[src]).sum(-1)
    gh = np.zeros((n, nh, c), dt)
    np.add.at(gh, src, alpha[:, :, None] * gagg[dst])
    dot = seg_total(alpha * galpha, dst, n)
    ge = alpha * (galpha - dot[dst]) * np.where(s > 0, dt(1), slope)
    g_s, g_d = np.zeros((n, nh), dt), np.zeros((n, nh), dt)
    np.add.at(g_s, src, ge)
    np.add.at(g_d, dst, ge)
    gh = gh + g_s[:, :, None] * a_s + g_d[:, :, None] * a_d
    ghe = (ge[:, :, None] * a_e).reshape(len(eal), nh * c) if use_edge else np.zeros((len(eal), nh * c), dt)
    geal = ghe @ We
    gea = np.zeros_like(ea)
    gk = geal[:len(ea_k)].copy()
    if fill == "mean":                                                 # through the mean back to the contributing rows
        gk += np.where(cnt[:, None] > 0, geal[len(ea_k):] / np.maximum(cnt, 1).astype(dt)[:, None], dt(0))[dst_k]
    gea[keep] = gk
    grads = {"x": gh.reshape(n, nh * c) @ W, "lin.weight": gh.reshape(n, nh * c).T @ x,
             "att_src": (g_s[:, :, None] * h).sum(0)[None], "att_dst": (g_d[:, :, None] * h).sum(0)[None],
             "lin_edge.weight": ghe.T @ eal, "att_edge": ((ge[:, :, None] * he).sum(0) if use_edge else 0 * a_e)[None],
             "bias": go.sum(0), "edge_attr": gea}
    return out, grads


def torch_layer(x, ei, ea, P, nh, c, concat, fill, relu, gup):
    """The layer in torch double through the folded M [D, H], differentiated by autograd."""
    n = len(x)
    t = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in P.items()}
    tx, tea = torch.from_numpy(x).double().requires_grad_(True), torch.from_numpy(ea).double().requires_grad_(True)
    keep = torch.from_numpy(ei[0] != ei[1])
    src_k, dst_k = torch.from_numpy(ei[0])[keep], torch.from_numpy(ei[1])[keep]
    ea_k = tea[keep]
    if fill == "mean":
        cnt = torch.bincount(dst_k, minlength=n).double()
        la = torch.zeros(n, ea.shape[1], dtype=torch.float64).index_add(0, dst_k, ea_k) / cnt.clamp(min=1)[:, None]
    else:
        la = torch.full((n, ea.shape[1]), float(fill), dtype=torch.float64)
    src, dst = torch.cat([src_k, torch.arange(n)]), torch.cat([dst_k, torch.arange(n)])
    M = ops.gat_edge_fold(t["lin_edge.weight"], t["att_edge"])
    assert M.shape == (ea.shape[1], nh)
    h = (tx @ t["lin.weight"].T).view(n, nh, c)
    s = ((h * t["att_src"]).sum(-1)[src] + (h * t["att_dst"]).sum(-1)[dst]) + torch.cat([ea_k, la]) @ M
    e = F.leaky_relu(s, SLOPE)
    m = torch.full((n, nh), -np.inf, dtype=torch.float64).scatter_reduce(0, dst[:, None].expand(-1, nh), e, "amax")
    ex = torch.exp(e - m[dst])
    alpha = ex / (torch.zeros(n, nh, dtype=torch.float64).index_add(0, dst, ex) + 1e-16)[dst]
    agg = torch.zeros(n, nh, c, dtype=torch.float64).index_add(0, dst, alpha[:, :, None] * h[src])
    out = (agg.view(n, nh * c) if concat else agg.mean(1)) + t["bias"]
    if relu:
        out = torch.relu(out)
    (out * torch.from_numpy(gup).double()).sum().backward()
    grads = {k: v.grad.numpy() for k, v in t.items()}
    grads.update(x=tx.grad.numpy(), edge_attr=tea.grad.numpy())
    return out.detach().numpy(), grads


# --------------------------------------------------------------------------- #
# CPU
# --------------------------------------------------------------------------- #
def test_constructor_parameters_and_state_dict():
    for concat in (True, False):
        torch.manual_seed(0)
        conv = dc.nn.GATConv(21, 64, heads=4, concat=concat, edge_dim=3)
        sd = conv.state_dict()
        assert set(sd) == {"lin.weight", "att_src", "att_dst", "lin_edge.weight", "att_edge", "bias"}
        assert sd["lin_edge.weight"].shape == (256, 3) and sd["att_edge"].shape == (1, 4, 64)
        assert sd["bias"].shape == ((256,) if concat else (64,))
        assert "edge_dim=3" in repr(conv) and "fill_value='mean'" in repr(conv)
        assert conv.edge_dim == 3 and conv.fill_value == "mean"
        bound = float(np.sqrt(6.0 / (4 + 64)))
        for _ in range(3):
            conv.reset_parameters()
            assert 0.5 * bound < float(conv.att_edge.detach().abs().max()) <= bound
            w = float(conv.lin_edge.weight.detach().abs().max())
            assert 0.5 * float(np.sqrt(6.0 / (3 + 256))) < w <= float(np.sqrt(6.0 / (3 + 256)))
        other = dc.nn.GATConv(21, 64, heads=4, concat=concat, edge_dim=3, fill_value=0.25)
        other.load_state_dict(sd, strict=True)
        for k, v in sd.items():
            assert torch.equal(other.state_dict()[k], v)
        with pytest.raises(RuntimeError):                            # a state_dict without the edge parameters is not this layer
            conv.load_state_dict(dc.nn.GATConv(21, 64, heads=4, concat=concat).state_dict(), strict=True)
    # edge_dim=None: exactly the layer as it was - same keys, same random stream, positional arguments keep their meaning
    torch.manual_seed(5)
    plain = dc.nn.GATConv(21, 64, 4, False, 0.1)
    torch.manual_seed(5)
    same = dc.nn.GATConv(21, 64, heads=4, concat=False, negative_slope=0.1, edge_dim=None)
    assert (plain.heads, plain.concat, plain.negative_slope, plain.edge_dim) == (4, False, 0.1, None)
    assert list(plain.state_dict()) == ["att_src", "att_dst", "bias", "lin.weight"]
    for k, v in plain.state_dict().items():
        assert torch.equal(same.state_dict()[k], v)
    assert "edge_dim" not in repr(plain) and plain.lin_edge is None and plain.att_edge is None
    for bad in ("sum", None, [0.0], True):
        with pytest.raises(ValueError, match="fill_value"):
            dc.nn.GATConv(21, 64, edge_dim=3, fill_value=bad)
    with pytest.raises(ValueError, match=str(ops.GAT_EDGE_MAX_DIM)):   # past the cap: refused by name, no fall-back
        dc.nn.GATConv(21, 64, edge_dim=ops.GAT_EDGE_MAX_DIM + 1)
    with pytest.raises(ValueError):
        dc.nn.GATConv(21, 64, edge_dim=0)
    assert ops.GAT_EDGE_MAX_DIM >= 32


def test_call_argument_errors():
    conv, plain = dc.nn.GATConv(21, 8, heads=2, edge_dim=3), dc.nn.GATConv(21, 8, heads=2)
    x, ei = torch.zeros(5, 21), torch.zeros(2, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="without edge_dim"):
        plain(x, ei, torch.zeros(4, 3))
    with pytest.raises(ValueError, match=r"\[E, 3\]"):
        conv(x, ei, torch.zeros(4, 2))
    with pytest.raises(ValueError, match=r"\[E, 3\]"):
        conv(x, ei, torch.zeros(4))                                  # [E] only with edge_dim = 1
    with pytest.raises(ValueError, match="5 rows"):
        conv(x, ei, torch.zeros(5, 3))
    with pytest.raises(ValueError, match="float32"):
        conv(x, ei, torch.zeros(4, 3, dtype=torch.float64))
    for third in (True, False, 1, "mean"):                           # never taken for relu
        with pytest.raises(TypeError, match="edge_attr"):
            conv(x, ei, third)
    with pytest.raises(RuntimeError, match="HIP device"):           # no CPU path
        conv(x, ei, torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="HIP device"):
        dc.nn.GATConv(21, 8, edge_dim=1)(x, ei, torch.zeros(4))


@pytest.mark.parametrize("nh,c,d,concat,fill,relu", [(4, 16, 3, True, "mean", False), (3, 5, 7, False, "mean", True),
                                                     (1, 8, 1, True, 0.5, True), (2, 4, 32, False, -1.25, False)])
def test_restatements_agree_on_the_cpu(nh, c, d, concat, fill, relu):
    """numpy the PyG way (explicit [E', H, C] projection, hand-written backward) == torch double through the folded M."""
    fi = 12
    n, ei = 300, random_multigraph(300, 2400, nh + d)
    assert (ei[0] == ei[1]).any() and len(np.unique(ei.T, axis=0)) < ei.shape[1]       # self loops, duplicates
    assert (np.bincount(ei[1], minlength=n) == 0).any()                                # zero in-degree
    rng = np.random.default_rng(d)
    x, ea = rng.uniform(-1, 1, (n, fi)).astype(np.float32), rng.uniform(-1, 1, (ei.shape[1], d)).astype(np.float32)
    gup = rng.uniform(0.5, 1.5, (n, nh * c if concat else c)).astype(np.float32)
    P = make_params(fi, nh, c, d, concat, 3)
    o64, g64 = np_layer(x, ei, ea, P, nh, c, concat, fill, relu, gup, np.float64)
    ot, gt = torch_layer(x, ei, ea, P, nh, c, concat, fill, relu, gup)
    assert rel_err(o64, ot) < 1e-12
    for k in g64:
        assert rel_err(g64[k], gt[k]) < 1e-11, k
    assert (g64["edge_attr"][ei[0] == ei[1]] == 0).all() and np.abs(g64["edge_attr"]).max() > 0
    # the edge term is in the function: without it the output differs
    o_no, _ = np_layer(x, ei, ea, P, nh, c, concat, fill, relu, gup, np.float64, use_edge=False)
    assert rel_err(o_no, o64) > 1e-3
    o32, g32 = np_layer(x, ei, ea, P, nh, c, concat, fill, relu, gup, np.float32)
    assert o32.dtype == np.float32 and rel_err(o32, o64) < 0.5 * TOL


@pytest.mark.parametrize("kind", GRAPHS)
@pytest.mark.parametrize("shape,d", LAYER_CASES)
def test_conditioning_of_the_gpu_cases(shape, d, kind):
    """Every (shape, graph) case the GPU layer test runs, on the CPU: the float32 restatement's forward is within half the
    bar of float64 at the tensor's scale (per row a ReLU output next to zero has no scale of its own: there the float64
    rule decides); the gradients (sums over up to 5,000-edge hubs
    and thousands of rows in numpy's running float32 order) are either inside the bar too or are judged against
    ``truth64`` by the float64 rule of ``helpers.assert_parity`` - nothing is registered special, nothing is wider."""
    fi, nh, c, concat = shape
    relu, fill = MODES[(d + nh) % len(MODES)]
    n, ei, x, ea, gup = make_inputs(kind, fi, nh, c, d, concat, 3)
    P = make_params(fi, nh, c, d, concat, 11)
    o32, g32 = np_layer(x, ei, ea, P, nh, c, concat, fill, relu, gup, np.float32)
    o64, g64 = np_layer(x, ei, ea, P, nh, c, concat, fill, relu, gup, np.float64)
    assert rel_err(o32, o64) < 0.5 * TOL
    for k in g64:
        assert np.isfinite(g32[k]).all()
        assert rel_err(g32[k], g64[k]) < 1e-3, k                      # (a restatement bug, not rounding, would show here)
        if kind not in ("n1", "e0"):
            assert np.abs(g64[k]).max() > 0, k                        # the comparison has something to compare


@pytest.mark.parametrize("relu,fill", MODES)
@pytest.mark.parametrize("d", [1, 3, 4, 7, 32])
@pytest.mark.parametrize("shape", [(256, 4, 64, True), (64, 3, 20, True)])
def test_conditioning_of_the_every_dim_and_mode_cases(shape, d, relu, fill):
    """The inputs of ``test_layer_parity_every_dim_and_mode`` on the CPU, as ``test_conditioning_of_the_gpu_cases``."""
    fi, nh, c, concat = shape
    n, ei, x, ea, gup = make_inputs("multigraph", fi, nh, c, d, concat, 5)
    P = make_params(fi, nh, c, d, concat, 13)
    o32, g32 = np_layer(x, ei, ea, P, nh, c, concat, fill, relu, gup, np.float32)
    o64, g64 = np_layer(x, ei, ea, P, nh, c, concat, fill, relu, gup, np.float64)
    assert rel_err(o32, o64) < 0.5 * TOL
    for k in g64:
        assert np.isfinite(g32[k]).all() and np.abs(g64[k]).max() > 0, k
        assert rel_err(g32[k], g64[k]) < 1e-3, k


def _edge_entry_calls():
    """name -> call(N, E, D, H, ptrs given?) of every edge-feature entry with otherwise valid arguments"""
    L = _lib.lib()
    p = lambda ok: 64 if ok else None                               # any non-null address: rejected calls never touch it

    def ws(n, e, d, h):
        return max(L.dc_gat_edge_attr_bwd_workspace_bytes(max(n + e, 0), min(max(d, 1), 64), max(h, 1)), 16)
    return {
        "dc_gat_edge_attr_fwd": lambda n, e, d, h, ok: L.dc_gat_edge_attr_fwd(p(ok), p(ok), p(ok), d, p(ok), 1, 0.0, p(ok), p(ok), n, e, d, h, None),
        "dc_gat_edge_attr_softmax_fwd": lambda n, e, d, h, ok: L.dc_gat_edge_attr_softmax_fwd(p(ok), p(ok), p(ok), p(ok), p(ok), 0.2, p(ok), n, h, None),
        "dc_gat_edge_attr_softmax_bwd": lambda n, e, d, h, ok: L.dc_gat_edge_attr_softmax_bwd(p(ok), p(ok), p(ok), p(ok), p(ok), 0.2, p(ok), p(ok), p(ok), p(ok), n, h, None),
        "dc_gat_edge_attr_bwd": lambda n, e, d, h, ok: L.dc_gat_edge_attr_bwd(p(ok), p(ok), p(ok), p(ok), d, p(ok), p(ok), 1, p(ok), d, p(ok), n, e, d, h, n + e, p(ok), ws(n, e, d, h), None),
    }


def test_abi_argument_errors_of_the_edge_entries_without_gpu():
    """null pointers, negative N / E, D < 1 or over the cap, H < 1: -1 and a message, before any HIP call (no device here)."""
    L = _lib.lib()
    calls = _edge_entry_calls()
    # the self-loop form of the segmented build validates like the form without
    ok = (ctypes.c_int64 * 2)(0, 3), (ctypes.c_int64 * 2)(0, 5)
    args = lambda ptrs, e=5, n=3, np_=ok[0], ep=ok[1]: (ptrs, e, n, np_, ep, 1) + (ptrs,) * 3 + (None,) + (ptrs,) * 3 + (None, ptrs, None)
    assert L.dc_graph_build_segmented_loops(*args(None)) == -1 and b"null" in L.dc_last_error()
    assert L.dc_graph_build_segmented_loops(*args(64, e=0)) == -1
    assert L.dc_graph_build_segmented_loops(*args(64, ep=(ctypes.c_int64 * 2)(0, 4))) == -1 and b"cover" in L.dc_last_error()
    assert L.dc_graph_build_segmented_loops(*args(64, e=20000, ep=(ctypes.c_int64 * 2)(0, 20000))) == -1 \
        and b"caps" in L.dc_last_error()
    declared = [n for n in _lib.exported_names() if "edge_attr" in n and "workspace" not in n]
    assert sorted(declared) == sorted(calls)
    header = open(__file__.replace("tests/test_gat_edge_attr.py", "include/deformcontact.h")).read()
    for name in list(calls) + ["dc_gat_edge_attr_bwd_workspace_bytes"]:
        assert hasattr(L, name) and f"{name}(" in header, name
    assert f"#define DC_GAT_EDGE_MAX_DIM {ops.GAT_EDGE_MAX_DIM}" in header
    for name, call in calls.items():
        assert call(3, 5, 4, 2, False) == -1 and name.encode() in L.dc_last_error() and b"null" in L.dc_last_error(), name
        assert call(-1, 5, 4, 2, True) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, 5, 4, 0, True) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, 5, 4, -2, True) == -1, name
        if "softmax" not in name:                                    # (the softmax entries see neither E nor D)
            assert call(3, -1, 4, 2, True) == -1 and name.encode() in L.dc_last_error(), name
            assert call(3, 5, 0, 2, True) == -1 and name.encode() in L.dc_last_error(), name
            assert call(3, 5, ops.GAT_EDGE_MAX_DIM + 1, 2, True) == -1 and b"cap" in L.dc_last_error(), name
    # leading dimensions, capacity, workspace
    assert L.dc_gat_edge_attr_fwd(64, 64, 64, 3, 64, 1, 0.0, 64, 64, 3, 5, 4, 2, None) == -1 and b"leading" in L.dc_last_error()
    assert L.dc_gat_edge_attr_bwd(64, 64, 64, 64, 4, 64, 64, 1, 64, 4, 64, 3, 5, 4, 2, 9, 64, 1 << 20, None) == -1 \
        and b"capacity" in L.dc_last_error()
    assert L.dc_gat_edge_attr_bwd(64, 64, 64, 64, 4, 64, 64, 1, 128, 4, 64, 3, 5, 4, 2, 8, 64, 4, None) == -1 \
        and b"workspace" in L.dc_last_error()
    assert L.dc_gat_edge_attr_bwd(64, 64, 64, 64, 4, 64, 64, 1, 64, 4, 64, 3, 5, 4, 2, 8, 64, 1 << 20, None) == -1 \
        and b"alias" in L.dc_last_error()
    assert L.dc_gat_edge_attr_bwd_workspace_bytes(8, 4, 2) == 4 * 2 * 4
    assert L.dc_gat_edge_attr_bwd_workspace_bytes(1025, 4, 2) == 2 * 4 * 2 * 4
    assert L.dc_gat_edge_attr_bwd_workspace_bytes(0, 4, 2) == 0
    for bad in ((-1, 4, 2), (8, 0, 2), (8, 65, 2), (8, 4, 0)):
        assert L.dc_gat_edge_attr_bwd_workspace_bytes(*bad) < 0


def test_batch_concatenates_edge_attr_in_edge_order():
    rng = np.random.default_rng(0)
    sizes = [(5, 7), (3, 3), (4, 0), (6, 11)]                        # (nodes, edges): E_i differ, one E == N, one E == 0
    datas = []
    for n, e in sizes:
        datas.append(Data(x=torch.from_numpy(rng.random((n, 2)).astype(np.float32)),
                          edge_index=torch.from_numpy(rng.integers(0, n, (2, e))),
                          edge_attr=torch.from_numpy(rng.random((e, 3)).astype(np.float32)),
                          y=torch.tensor([float(n)])))
    b = Batch.from_data_list(datas)
    assert b._kinds["edge_attr"] == "edge_attr" and b._kinds["x"] == "node" and b._kinds["y"] == "graph"
    assert b.edge_attr.shape == (21, 3) and b.edge_index.shape == (2, 21) and b.y.shape == (4, 1)
    assert torch.equal(b.edge_attr, torch.cat([d.edge_attr for d in datas]))
    eptr = [0, 7, 10, 10, 21]
    for i, d in enumerate(datas):                                    # row p of edge_attr belongs to column p of edge_index
        assert torch.equal(b.edge_attr[eptr[i]:eptr[i + 1]], d.edge_attr)
        assert torch.equal(b.edge_index[:, eptr[i]:eptr[i + 1]] - int(b.ptr[i]), d.edge_index)
        for got in (b[i], b.get_example(i), b.to_data_list()[i], b.clone()[i], b.clone().to("cpu")[i]):
            assert torch.equal(got.edge_attr, d.edge_attr) and torch.equal(got.edge_index, d.edge_index)
            assert torch.equal(got.x, d.x)
    c = b.clone()
    assert c.edge_attr.data_ptr() != b.edge_attr.data_ptr() and torch.equal(c.edge_attr, b.edge_attr)
    # [E] attributes (edge_dim = 1) concatenate too
    flat = Batch.from_data_list([Data(x=d.x, edge_index=d.edge_index, edge_attr=d.edge_attr[:, 0]) for d in datas])
    assert flat.edge_attr.shape == (21,) and torch.equal(flat[3].edge_attr, datas[3].edge_attr[:, 0])
    # a batch without edge_attr is what it was
    plain = Batch.from_data_list([Data(x=d.x, edge_index=d.edge_index, y=d.y) for d in datas])
    assert "edge_attr" not in plain._kinds and getattr(plain, "edge_attr", None) is None
    assert plain._kinds == {"x": "node", "edge_index": "edge", "y": "graph"}
    assert torch.equal(plain.edge_index, b.edge_index) and torch.equal(plain.x, b.x) and torch.equal(plain.y, b.y)
    # any other key whose first dimension happens to equal E still follows the old rules
    odd = Batch.from_data_list([Data(x=torch.zeros(4, 1), edge_index=torch.zeros(2, 2, dtype=torch.long),
                                     edge_w=torch.ones(2)) for _ in range(2)])
    assert odd._kinds["edge_w"] == "graph" and odd.edge_w.shape == (2, 2)


# --------------------------------------------------------------------------- #
# GPU: the layer
# --------------------------------------------------------------------------- #
def _device_conv(P, fi, nh, c, concat, d, fill="mean"):
    conv = dc.nn.GATConv(fi, c, heads=nh, concat=concat, edge_dim=d, fill_value=fill)
    conv.load_state_dict({k: torch.from_numpy(v).clone() for k, v in P.items()}, strict=True)
    return conv.to(DEV)


def _device_run(conv, x, ei, ea, gup, **kw):
    for p in conv.parameters():
        p.grad = None
    xg = torch.from_numpy(x).to(DEV).requires_grad_(True)
    eg = None if ea is None else torch.from_numpy(ea).to(DEV).requires_grad_(True)
    out = ops.resolve(conv(xg, torch.from_numpy(ei).to(DEV), eg, **kw))
    (out * torch.from_numpy(gup).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in conv.named_parameters() if p.grad is not None}
    grads["x"] = xg.grad
    if eg is not None:
        grads["edge_attr"] = eg.grad
    return out.detach(), grads


def _check_layer(tag, conv, P, x, ei, ea, gup, nh, c, concat, fill, relu):
    o32, g32 = np_layer(x, ei, ea, P, nh, c, concat, fill, relu, gup, np.float32)
    o64, g64 = np_layer(x, ei, ea, P, nh, c, concat, fill, relu, gup, np.float64)
    og, gg = _device_run(conv, x, ei, ea, gup, relu=relu)
    assert og.shape == o32.shape
    assert_parity(_np(og), o32, o64, TOL, f"{tag} forward")
    assert_parity(_np(og), o32, o64, TOL, f"{tag} forward per row", metric=row_rel_err)
    for name in ("x",) + PARAMS + ("edge_attr",):
        print(f"{tag} {name}.grad: vs ref32 {rel_err(_np(gg[name]), g32[name]):.3e} vs truth64 "
              f"{rel_err(_np(gg[name]), g64[name]):.3e}")
        assert_parity(_np(gg[name]), g32[name], g64[name], TOL, f"{tag} {name}.grad")
    assert (_np(gg["edge_attr"])[ei[0] == ei[1]] == 0).all(), tag          # dropped input self loops: exact zeros
    return og, gg


@gpu
@pytest.mark.parametrize("kind", GRAPHS)
@pytest.mark.parametrize("shape,d", LAYER_CASES)
def test_layer_parity(shape, d, kind):
    """forward and the gradients of x, every parameter and edge_attr against ``np_layer`` (float32 / float64) at 1e-5."""
    torch.set_num_threads(1)
    fi, nh, c, concat = shape
    relu, fill = MODES[(d + nh) % len(MODES)]
    n, ei, x, ea, gup = make_inputs(kind, fi, nh, c, d, concat, 3)
    P = make_params(fi, nh, c, d, concat, 11)
    clear_cache()
    conv = _device_conv(P, fi, nh, c, concat, d, fill)
    _lib.kernel_trace(True)
    _check_layer(f"GATConv {fi}->{nh}x{c} concat={concat} D={d} fill={fill} relu={relu} {kind}", conv, P, x, ei, ea, gup,
                 nh, c, concat, fill, relu)
    counts = _lib.kernel_trace_counts()
    _lib.kernel_trace(False)
    for k in ("k_gat_edge_term_fwd", "k_gat_softmax_heads_fwd", "k_gat_softmax_heads_bwd", "k_gat_edge_gm_partial",
              "k_gat_edge_gm_final", "k_spmm_heads", "k_sddmm_heads"):
        assert any(k in name for name in counts), (k, counts)
    if ei.shape[1]:
        assert any("k_gat_edge_term_bwd" in name for name in counts), counts
    assert not any(k in name for name in counts for k in ("k_gat_softmax_fwd", "k_sddmm<", "k_spmm_wave")), counts


@gpu
@pytest.mark.parametrize("relu,fill", MODES)
@pytest.mark.parametrize("d", [1, 3, 4, 7, 32])
@pytest.mark.parametrize("shape", [(256, 4, 64, True), (64, 3, 20, True)])
def test_layer_parity_every_dim_and_mode(shape, d, relu, fill):
    """D in {1, 3, 4, 7, 32} x relu on / off x mean / constant fill, at a fused and an unfused width, on the multigraph
    (duplicate edges, input self loops, zero-in-degree nodes); D = 1 also as a [E] tensor and with a row stride."""
    torch.set_num_threads(1)
    fi, nh, c, concat = shape
    n, ei, x, ea, gup = make_inputs("multigraph", fi, nh, c, d, concat, 5)
    P = make_params(fi, nh, c, d, concat, 13)
    clear_cache()
    conv = _device_conv(P, fi, nh, c, concat, d, fill)
    og, gg = _check_layer(f"GATConv {fi}->{nh}x{c} D={d} fill={fill} relu={relu}", conv, P, x, ei, ea, gup, nh, c, concat,
                          fill, relu)
    tei, xg = torch.from_numpy(ei).to(DEV), torch.from_numpy(x).to(DEV)
    wide = torch.full((ei.shape[1], d + 5), 1e30, device=DEV)
    wide[:, 2:2 + d] = torch.from_numpy(ea).to(DEV)
    assert torch.equal(conv(xg, tei, wide[:, 2:2 + d], relu=relu), og)     # row stride > D, inner stride 1
    if d == 1:
        assert torch.equal(conv(xg, tei, torch.from_numpy(ea[:, 0].copy()).to(DEV), relu=relu), og)


@gpu
@pytest.mark.parametrize("fi,nh,c,concat,d", [(256, 4, 64, True, 3), (64, 3, 20, True, 7), (32, 1, 64, False, 4),
                                              (256, 4, 64, False, 32), (32, 1, 64, True, 1)])
def test_zero_edge_attr_and_no_edge_attr_are_the_layer_without_edge_features_bitwise(fi, nh, c, concat, d):
    """(a_src + a_dst) + 0 is a_src + a_dst: ``GATConv(edge_dim=D)`` fed zeros equals ``GATConv()`` with the shared
    weights bit for bit - output and the gradients of x, lin.weight, att_src, att_dst, bias - and so does the layer
    called without edge_attr; constant fill 0 and mean fill alike."""
    n, ei, x, ea, gup = make_inputs("multigraph", fi, nh, c, d, concat, 7)
    P = make_params(fi, nh, c, d, concat, 17)
    clear_cache()
    plain = dc.nn.GATConv(fi, c, heads=nh, concat=concat)
    plain.load_state_dict({k: torch.from_numpy(v).clone() for k, v in P.items() if "edge" not in k}, strict=True)
    plain = plain.to(DEV)
    xg, tei = torch.from_numpy(x).to(DEV), torch.from_numpy(ei).to(DEV)
    for relu in (False, True):
        for p in plain.parameters():
            p.grad = None
        xp = xg.clone().requires_grad_(True)
        want = ops.resolve(plain(xp, tei, relu=relu))
        (want * torch.from_numpy(gup).to(DEV)).sum().backward()
        for fill in ("mean", 0.0):
            conv = _device_conv(P, fi, nh, c, concat, d, fill)
            for attr in (np.zeros_like(ea), None):
                og, gg = _device_run(conv, x, ei, attr, gup, relu=relu)
                tag = f"relu={relu} fill={fill} attr={'zeros' if attr is not None else None}"
                assert torch.equal(og, want), tag
                assert torch.equal(gg["x"], xp.grad), tag
                for name, p in plain.named_parameters():
                    assert torch.equal(gg[name], p.grad), (tag, name)
                if attr is None:
                    assert "lin_edge.weight" not in gg and "att_edge" not in gg


@gpu
@pytest.mark.parametrize("fi,nh,c,concat,d", [(256, 4, 64, True, 3), (64, 3, 20, True, 7), (256, 4, 64, False, 32),
                                              (32, 1, 64, False, 1)])
def test_bit_for_bit_relu_deferred_and_repeat(fi, nh, c, concat, d):
    n, ei, x, ea, gup = make_inputs("hub", fi, nh, c, d, concat, 4)
    P = make_params(fi, nh, c, d, concat, 31)
    clear_cache()
    conv = _device_conv(P, fi, nh, c, concat, d)
    tei, xg, eg = torch.from_numpy(ei).to(DEV), torch.from_numpy(x).to(DEV), torch.from_numpy(ea).to(DEV)
    plain = ops.resolve(conv(xg, tei, eg)).clone()
    assert plain.shape == (n, nh * c if concat else c)
    want = torch.relu(plain)
    assert (plain < 0).any() and (plain > 0).any()
    assert torch.equal(conv(xg, tei, eg, relu=True), want)
    y = conv(xg, tei, eg)
    assert type(y).__name__ == "DeferredActivation" and y.shape == plain.shape
    assert torch.equal(F.relu(y), want)
    assert torch.equal(conv(xg, tei, edge_attr=eg, relu=True), want)
    # edge_attr is guarded like the other inputs of a deferred call
    y = conv(xg, tei, eg)
    eg.add_(1.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        y.value()
    # a gradient wanted by edge_attr alone is recorded
    for p in conv.parameters():
        p.requires_grad_(False)
    e2 = torch.from_numpy(ea).to(DEV).requires_grad_(True)
    y = conv(xg, tei, e2)
    assert y.requires_grad
    F.relu(y).sum().backward()
    assert e2.grad is not None and float(e2.grad.abs().max()) > 0
    for p in conv.parameters():
        p.requires_grad_(True)
    # two consecutive runs: same bits in the output and in every gradient
    for kw in ({}, {"relu": True}):
        a = _device_run(conv, x, ei, ea, gup, **kw)
        b = _device_run(conv, x, ei, ea, gup, **kw)
        assert torch.equal(a[0], b[0])
        for name in a[1]:
            assert torch.equal(a[1][name], b[1][name]), name


@gpu
def test_branch_streams_give_the_same_bits(monkeypatch):
    from deformcontact_amd.nn import conv as conv_mod
    fi, nh, c, d = 32, 4, 16, 3
    P = make_params(fi, nh, c, d, True, 3)
    n, ei, x, ea, gup = make_inputs("multigraph", fi, nh, c, d, True, 9)
    n2, ei2, x2, ea2, _ = make_inputs("hub", fi, nh, c, d, True, 10)
    a, b = _device_conv(P, fi, nh, c, True, d), _device_conv(P, fi, nh, c, True, d, 0.5)
    t = lambda v: torch.from_numpy(v).to(DEV)
    ins = (t(x), t(ei), t(ea)), (t(x2), t(ei2), t(ea2))

    def both():
        clear_cache()
        ya, yb = F.relu(a(*ins[0])), F.relu(b(*ins[1]))
        torch.cuda.synchronize()
        return ya.clone(), yb.clone()
    want = both()
    monkeypatch.setattr(conv_mod, "BRANCH_STREAMS", True)
    got = both()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@gpu
def test_two_stacked_layers_captured_and_replayed():
    """forward + backward of two edge-feature layers under torch.cuda.graph (no host read: capture would fail on one);
    three replays with new x and edge_attr in the static inputs, each bit-identical to the eager run on them."""
    n, ei = _graph("multigraph", 12)
    fi, nh, c, d = 32, 4, 16, 3
    torch.manual_seed(3)
    l1 = dc.nn.GATConv(fi, c, heads=nh, edge_dim=d).to(DEV)
    l2 = dc.nn.GATConv(nh * c, c, heads=nh, concat=False, edge_dim=d, fill_value=0.5).to(DEV)
    with torch.no_grad():
        l1.bias.uniform_(-0.3, 0.3)
        l2.bias.uniform_(-0.3, 0.3)
    params = list(l1.parameters()) + list(l2.parameters())
    tei = torch.from_numpy(ei).to(DEV)
    rng = np.random.default_rng(1)
    xs = [torch.from_numpy(rng.uniform(-1, 1, (n, fi)).astype(np.float32)).to(DEV) for _ in range(4)]
    es = [torch.from_numpy(rng.uniform(-1, 1, (ei.shape[1], d)).astype(np.float32)).to(DEV) for _ in range(4)]
    gup = torch.from_numpy(rng.uniform(0.5, 1.5, (n, c)).astype(np.float32)).to(DEV)
    static_x, static_e = xs[0].clone().requires_grad_(True), es[0].clone().requires_grad_(True)
    leaves = [static_x, static_e] + params
    for t in leaves:
        t.grad = torch.zeros_like(t)

    def step():
        for t in leaves:
            t.grad.zero_()
        out = l2(l1(static_x, tei, static_e, relu=True), tei, static_e, relu=True)
        torch.autograd.backward([out], [gup])
        return out

    def snapshot(out):
        return [out.detach().clone()] + [t.grad.clone() for t in leaves]

    eager = []
    for x, e in zip(xs, es):
        with torch.no_grad():
            static_x.copy_(x)
            static_e.copy_(e)
        clear_cache()
        eager.append(snapshot(step()))
    torch.cuda.synchronize()
    assert float(eager[0][2].abs().max()) > 0                        # edge_attr.grad
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        clear_cache()
        step()                                                       # warm-up off the default stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    clear_cache()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for i in (1, 2, 3):
        with torch.no_grad():
            static_x.copy_(xs[i])
            static_e.copy_(es[i])
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(snapshot(out), eager[i]):
            assert torch.equal(got, want), i


def _knn_case():
    z = load_golden("graphnet_gat_h32.npz")
    pos = torch.from_numpy(z["rest_pos"].astype(np.float32)).to(DEV)
    n = pos.size(0)
    half = n // 2
    batch = torch.cat([torch.zeros(half, dtype=torch.long), torch.ones(n - half, dtype=torch.long)]).to(DEV)
    ei = dc.nn.knn_graph(pos, 6, batch)
    return pos, batch, ei, pos[ei[0]] - pos[ei[1]]


@gpu
def test_knn_graph_with_relative_positions_end_to_end():
    """``conv(x, knn_graph(pos, k, batch), pos[src] - pos[dst])``: device-built graph, per-edge geometry, against truth64."""
    torch.set_num_threads(1)
    pos, batch, ei, ea = _knn_case()
    fi, nh, c, d = 21, 4, 16, 3
    n = pos.size(0)
    P = make_params(fi, nh, c, d, True, 23)
    x = np.random.default_rng(1).uniform(-1, 1, (n, fi)).astype(np.float32)
    gup = np.random.default_rng(2).uniform(0.5, 1.5, (n, nh * c)).astype(np.float32)
    clear_cache()
    conv = _device_conv(P, fi, nh, c, True, d)
    eg = ea.clone().requires_grad_(True)
    xg = torch.from_numpy(x).to(DEV).requires_grad_(True)
    out = F.relu(conv(xg, ei, eg))
    (out * torch.from_numpy(gup).to(DEV)).sum().backward()
    o32, g32 = np_layer(x, _np(ei), _np(ea), P, nh, c, True, "mean", True, gup, np.float32)
    o64, g64 = np_layer(x, _np(ei), _np(ea), P, nh, c, True, "mean", True, gup, np.float64)
    assert_parity(_np(out), o32, o64, TOL, "knn end to end forward", metric=row_rel_err)
    assert_parity(_np(xg.grad), g32["x"], g64["x"], TOL, "knn end to end x.grad")
    assert_parity(_np(eg.grad), g32["edge_attr"], g64["edge_attr"], TOL, "knn end to end edge_attr.grad")
    assert_parity(_np(conv.lin_edge.weight.grad), g32["lin_edge.weight"], g64["lin_edge.weight"], TOL,
                  "knn end to end lin_edge.weight.grad")


@gpu
def test_knn_graph_edge_features_take_the_segmented_build():
    """The end-to-end call builds its self-loop adjacency in the one-launch segmented build (``knn_graph`` tags its result
    with the batch layout): ``k_build_segment_loops`` in the launch log, none of the global pipeline's kernels; an
    untagged copy of the same ``edge_index`` takes the global pipeline and gives the same bits."""
    pos, batch, ei, ea = _knn_case()
    conv = _device_conv(make_params(21, 4, 16, 3, True, 23), 21, 4, 16, True, 3)
    x = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, (pos.size(0), 21)).astype(np.float32)).to(DEV)
    outs, logs = [], []
    for edges in (ei, ei.clone()):
        clear_cache()
        _lib.kernel_trace(True)
        try:
            outs.append(conv(x, edges, ea, relu=True).clone())
            torch.cuda.synchronize()
            logs.append(_lib.kernel_trace_counts())
        finally:
            _lib.kernel_trace(False)
    segmented = sum(v for k, v in logs[0].items() if "k_build_segment" in k)
    print("k_build_segment* launches:", segmented, "| untagged:", sum(v for k, v in logs[1].items() if "k_build_segment" in k))
    assert segmented >= 1, logs[0]
    assert not any(k in logs[0] for k in ("k_count", "k_emit")), logs[0]
    assert not any("k_build_segment" in k for k in logs[1]), logs[1]
    assert torch.equal(outs[0], outs[1])


@gpu
def test_layers_without_edge_dim_keep_the_global_adjacency_build(monkeypatch):
    """Only ``GATConv(edge_dim=...)`` asks for the self-loop segmented build: a plain ``GATConv`` and a ``GCNConv`` on the
    same tagged batch run the global pipeline's launches as before; past ``SEG_LOOPS_MAX_WORK`` (graphs x edges) the
    edge-feature layer does too.  Same arrays either way."""
    from deformcontact_amd import graph as graph_mod
    pos, batch, ei, ea = _knn_case()
    x = torch.zeros(pos.size(0), 21, device=DEV)

    def log(conv, *args):
        clear_cache()
        _lib.kernel_trace(True)
        try:
            out = ops.resolve(conv(x, ei, *args)).clone()
            torch.cuda.synchronize()
            return out, _lib.kernel_trace_counts()
        finally:
            _lib.kernel_trace(False)
    torch.manual_seed(0)
    for plain in (dc.nn.GATConv(21, 16, heads=4).to(DEV), dc.nn.GATConv(21, 64).to(DEV), dc.nn.GCNConv(21, 64).to(DEV)):
        _, counts = log(plain)
        assert not any("k_build_segment" in k for k in counts) and "k_count" in counts and "k_emit" in counts, counts
    conv = _device_conv(make_params(21, 4, 16, 3, True, 23), 21, 4, 16, True, 3)
    want, counts = log(conv, ea)
    assert counts.get("k_build_segment_loops", 0) == 1 and "k_count" not in counts, counts
    monkeypatch.setattr(graph_mod, "SEG_LOOPS_MAX_WORK", 2 * ei.size(1) - 1)
    got, counts = log(conv, ea)
    assert not any("k_build_segment" in k for k in counts) and "k_count" in counts, counts
    assert torch.equal(got, want)


@gpu
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("sizes", [[(300, 2400)], [(5, 7), (3, 3), (4, 0), (6, 11), (1, 1), (1024, 6000)],
                                   [(7 + i % 5, 3 * (i % 4)) for i in range(200)], [(4096, 16384), (2, 9)]])
def test_segmented_build_with_self_loops_equals_the_global_build(sizes, normalize):
    """dc_graph_build_segmented_loops against dc_graph_build(self_loops=1) bit for bit - ptr, other, perm, gcn_norm
    weights, both sides, up to ptr[N] - on batches with input self loops, duplicates, graphs without edges, more than 96
    graphs (two launches) and a graph at the LDS caps."""
    rng = np.random.default_rng(len(sizes))
    parts, noff, eoff = [], [0], [0]
    for n, e in sizes:
        g = random_multigraph(n, e, n + e, isolated=n > 10) if e >= 8 else rng.integers(0, n, (2, e))
        parts.append(g + noff[-1])
        noff.append(noff[-1] + n)
        eoff.append(eoff[-1] + e)
    ei = torch.from_numpy(np.concatenate(parts, 1).astype(np.int64)).to(DEV)
    assert (ei[0] == ei[1]).any()
    n = noff[-1]
    want = GraphIndex(ei, n, self_loops=True, normalize=normalize, validate=True)
    # (GraphIndex itself takes this build for GATConv's normalize=False adjacency only; the entry forms gcn_norm too)
    assert GraphIndex(ei, n, self_loops=True, normalize=normalize, segments=(noff, eoff))._segments is None   # opt-in only
    got = GraphIndex(ei, n, self_loops=True, normalize=normalize, segments=(noff, eoff), loops_segmented=not normalize)
    assert (got._segments is not None) == (not normalize)
    got._segments = _segment_arrays((noff, eoff), n, ei.size(1), ei.device)
    for adj in (got.fwd, got.bwd):
        adj.ptr.fill_(-1)
    _lib.kernel_trace(True)
    got.rebuild()
    torch.cuda.synchronize()
    counts = _lib.kernel_trace_counts()
    _lib.kernel_trace(False)
    got.validate()
    assert counts.get("k_build_segment_loops", 0) == (len(sizes) + 95) // 96, counts
    for a, b in ((got.fwd, want.fwd), (got.bwd, want.bwd)):
        assert torch.equal(a.ptr, b.ptr)
        m = int(b.ptr[-1])
        assert m == ei.size(1) - int((ei[0] == ei[1]).sum()) + n
        assert torch.equal(a.other[:m], b.other[:m]) and torch.equal(a.perm[:m], b.perm[:m])
        if normalize:
            assert torch.equal(a.w[:m], b.w[:m])
    # an edge that leaves its graph is flagged
    if len(sizes) > 1 and ei.size(1):
        bad = ei.clone()
        bad[0, 0] = n - 1
        with pytest.raises(IndexError):
            GraphIndex(bad, n, self_loops=True, normalize=False, validate=True, segments=(noff, eoff), loops_segmented=True)
        bad = ei.clone()
        bad[:, 0] = n - 1                                            # a self loop outside its graph: dropped, and flagged
        with pytest.raises(IndexError):
            GraphIndex(bad, n, self_loops=True, normalize=False, validate=True, segments=(noff, eoff), loops_segmented=True)


# --------------------------------------------------------------------------- #
# GPU: the entries called directly
# --------------------------------------------------------------------------- #
def _fwd_rows(ei, perm, e_in, ea, la):
    """attribute row of every sorted edge: row perm[p] of edge_attr, or the loop attribute of node perm[p] - E"""
    return np.where((perm < e_in)[:, None], ea[np.minimum(perm, max(e_in - 1, 0))] if e_in else 0.0, la[np.maximum(perm - e_in, 0)])


def _direct_graph(kind):
    if kind == "hub":
        g, ptr, other, lens = device_graph(131, 41)
        ei = _np(g.edge_index)
    else:
        ei = random_multigraph(300, 2400, 6)
        g = GraphIndex(torch.from_numpy(ei).to(DEV), 300, self_loops=True, normalize=False, validate=True)
        ptr = _np(g.fwd.ptr).astype(np.int64)
        other = _np(g.fwd.other).astype(np.int64)[:ptr[-1]]
    perm = _np(g.fwd.perm).astype(np.int64)[:ptr[-1]]
    return g, ei, ptr, other, perm


@gpu
@pytest.mark.parametrize("kind", ["hub", "multigraph"])
@pytest.mark.parametrize("d,nh", [(1, 1), (3, 4), (4, 2), (7, 5), (32, 8), (32, 11), (64, 3)])
def test_edge_term_entries_per_edge_and_head(d, nh, kind):
    """dc_gat_edge_attr_fwd / _bwd called directly: a_edge per edge and head (one-signed operands: a sum of mixed-sign
    products can cancel to nothing and then no fp32 evaluation is within 1e-5 of it), the loop attribute bit for bit
    against an fp32 numpy sum in the same order, g_edge_attr per row with exact zeros for dropped self loops, gM."""
    g, ei, ptr, other, perm = _direct_graph(kind)
    n, e_in, e = g.num_nodes, ei.shape[1], int(ptr[-1])
    seg_err = seg_rel_err_on(ptr)
    rng = np.random.default_rng(d * 10 + nh)
    ea = (0.5 + rng.random((e_in, d))).astype(np.float32)
    m = (0.5 + rng.random((d, nh))).astype(np.float32)
    keep = ei[0] != ei[1]
    assert sorted(perm[perm < e_in]) == sorted(np.flatnonzero(keep)) and (perm >= e_in).sum() == n
    tm, tea = _dev(m), _dev(ea)
    for fill in ("mean", 0.75):
        fill_mean, fv = ops.gat_edge_fill(fill)
        a_edge, loop_attr = ops._edge_term_fwd(g, tea, tm, fill_mean, fv, n, nh)
        a2, l2 = ops._edge_term_fwd(g, tea, tm, fill_mean, fv, n, nh)
        assert torch.equal(a_edge, a2) and torch.equal(loop_attr, l2) and (a_edge[e:] == 0).all()
        la32, cnt = loop_fill(n, ei[1][keep], ea[keep], fill, np.float32)
        assert la32.dtype == np.float32 and np.array_equal(_np(loop_attr), la32)        # bit for bit
        rows = _fwd_rows(ei, perm, e_in, ea, la32).astype(np.float32)
        for k in range(nh):
            w32 = (rows * m[:, k]).sum(1, dtype=np.float32)
            w64 = (rows.astype(np.float64) * m[:, k].astype(np.float64)).sum(1)
            assert_parity(_np(a_edge)[:e, k], w32, w64, TOL, f"a_edge D={d} H={nh} head {k} fill={fill} {kind}", metric=seg_err)
        # backward: one-signed ge
        ge = np.zeros((max(g.capacity, 1), nh), np.float32)
        ge[:e] = 0.5 + rng.random((e, nh))
        tge = _dev(ge)
        g_attr, g_m = ops._edge_term_bwd(g, tge, tea, loop_attr, tm, fill_mean, n, nh, True, True)
        g_attr2, g_m2 = ops._edge_term_bwd(g, tge, tea, loop_attr, tm, fill_mean, n, nh, True, True)
        assert torch.equal(g_attr, g_attr2) and torch.equal(g_m, g_m2)
        only_m = ops._edge_term_bwd(g, tge, tea, loop_attr, tm, fill_mean, n, nh, False, True)
        assert only_m[0] is None and torch.equal(only_m[1], g_m)
        assert (_np(g_attr)[~keep] == 0).all()                       # dropped input self loops: exactly zero

        def want(dt):
            t = ge[:e].astype(dt).copy()
            seg = seg_of(ptr)
            if fill == "mean":
                loop_p = np.flatnonzero(perm >= e_in)
                gl = np.zeros((n, nh), dt)
                gl[perm[loop_p] - e_in] = ge[loop_p].astype(dt)
                t = t + np.where(cnt[:, None] > 0, gl / np.maximum(cnt, 1).astype(dt)[:, None], dt(0))[seg]
            out = np.zeros((e_in, d), dt)
            inp = perm < e_in
            out[perm[inp]] = t[inp] @ m.astype(dt).T
            return out, rows.astype(dt).T @ ge[:e].astype(dt)
        (ga32, gm32), (ga64, gm64) = want(np.float32), want(np.float64)
        assert_parity(_np(g_attr), ga32, ga64, TOL, f"g_edge_attr D={d} H={nh} fill={fill} {kind}", metric=row_rel_err)
        assert_parity(_np(g_m), gm32, gm64, TOL, f"gM D={d} H={nh} fill={fill} {kind}")


@gpu
@pytest.mark.parametrize("nh", [1, 2, 5, 8, 11])
@pytest.mark.parametrize("case", ["normal0.1", "normal1", "normal8", "slope0"])
def test_edge_softmax_with_the_addend_per_edge_and_head(case, nh):
    """dc_gat_edge_attr_softmax_fwd / _bwd per edge and head; value parity of ge where the backward is well conditioned
    (BWD_CASES of test_gat_edge_kernels.py); an addend of zeros gives the bits of the entries without it; the leaky-relu
    derivative looks at the full logit."""
    n = 131
    g, ptr, other, lens = device_graph(n, 9 + nh)
    e = int(ptr[-1])
    seg, seg_err = seg_of(ptr), seg_rel_err_on(ptr)
    a_src, a_dst, slope = heads_logits(case, ptr, other, nh, 300)
    scale = float(case[len("normal"):]) if case.startswith("normal") else 0.5
    a_e = np.zeros((max(g.capacity, 1), nh), np.float32)
    a_e[:e] = np.random.default_rng(nh).standard_normal((e, nh)) * scale
    ts, td, te = _dev(a_src), _dev(a_dst), _dev(a_e)

    def ref(dt, alpha=None, galpha=None):
        s = (a_src.astype(dt)[other] + a_dst.astype(dt)[seg]) + a_e[:e].astype(dt)
        if alpha is None:
            lr = np.where(s > 0, s, dt(np.float32(slope)) * s)
            mx = np.full((n, nh), -np.inf, dt)
            np.maximum.at(mx, seg, lr)
            ex = np.exp(lr - mx[seg])
            den = np.stack([_seg_sum(np.ascontiguousarray(ex[:, k]), seg, n) for k in range(nh)], 1)
            return ex / (den + dt(1e-16))[seg]
        al, ga = alpha.astype(dt), galpha.astype(dt)
        dot = np.stack([_seg_sum(np.ascontiguousarray((al * ga)[:, k]), seg, n) for k in range(nh)], 1)
        return al * (ga - dot[seg]) * np.where(s > 0, dt(1), dt(np.float32(slope))), s
    alpha = ops._edge_softmax_fwd(g, ts, td, te, slope, n, nh)
    assert torch.equal(alpha, ops._edge_softmax_fwd(g, ts, td, te, slope, n, nh)) and (alpha[e:] == 0).all()
    got = _np(alpha)[:e]
    a32, a64 = ref(np.float32), ref(np.float64)
    galpha = heads_galpha(ptr, nh, 11)
    tg = torch.zeros_like(alpha)
    tg[:e] = _dev(galpha)
    ge, gd = ops._edge_softmax_bwd(g, ts, td, te, slope, alpha, tg, n, nh)
    ge2, gd2 = ops._edge_softmax_bwd(g, ts, td, te, slope, alpha, tg, n, nh)
    assert torch.equal(ge, ge2) and torch.equal(gd, gd2) and (ge[e:] == 0).all() and torch.isfinite(ge).all()
    (ge32, _), (ge64, s64) = ref(np.float32, got, galpha), ref(np.float64, got, galpha)
    for k in range(nh):
        tag = f"{case} H={nh} head {k} with a_edge"
        assert_parity(got[:, k], a32[:, k], a64[:, k], TOL, f"alpha {tag}", metric=seg_err)
        check_g_a_dst(tag, ptr, _np(ge)[:, k], _np(gd)[:, k])
        if case in BWD_CASES:
            assert_parity(_np(ge)[:e, k], ge32[:, k], ge64[:, k], TOL, f"ge {tag}", metric=seg_err)
    if case == "slope0":                                             # the derivative is that of the FULL logit
        assert (_np(ge)[:e][s64 <= 0] == 0.0).all()
        flipped = ((a_src[other] + a_dst[seg]) > 0) != (s64 > 0)
        assert flipped.any()
    # zeros: the entries without the addend, bit for bit
    z = torch.zeros_like(te)
    al0 = ops._edge_softmax_fwd(g, ts, td, z, slope, n, nh)
    alh = ops._heads_softmax_fwd(g, ts, td, slope, n, nh)
    assert torch.equal(al0, alh)
    ge0, gd0 = ops._edge_softmax_bwd(g, ts, td, z, slope, alh, tg, n, nh)
    geh, gdh = ops._heads_softmax_bwd(g, ts, td, slope, alh, tg, n, nh)
    assert torch.equal(ge0, geh) and torch.equal(gd0, gdh)
