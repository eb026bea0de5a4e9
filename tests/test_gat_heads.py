"""``GATConv(heads > 1)``: the layer, its autograd Functions and the C entries of dc_gat_heads.hip.

CPU: constructor / state_dict contract, argument checks of every new C entry, and this file's numpy restatements of the
per-edge formulas for H heads (dtype-parametrised: float32 is ``ref32``, float64 ``truth64``) against
``oracle.pyg_ref`` in double and torch autograd.

GPU: the layer against ``oracle.pyg_ref.GATConv`` (float32 and float64) at 1e-5 - nothing wider, nothing registered
``special``; the per-edge entries called directly, per edge and per head with the per-segment metric and under the
conditioning rules of ``tests/test_gat_edge_kernels.py`` (value parity of ``ge`` / ``g_a_dst`` only where a segment's logits
spread over a few units, one-signed SDDMM operands), head k of every result against the single-head entry on column block
k; a multi-head layer against H ``heads=1`` layers built from its weight slices; the bit-for-bit properties; capture.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deformcontact_amd as dc
from deformcontact_amd import _lib, ops
from deformcontact_amd.graph import GraphIndex, clear_cache
from oracle import pyg_ref
from tests.helpers import assert_parity, load_golden, random_multigraph, record_parity, rel_err, row_rel_err
from tests.test_gat_edge_kernels import (BWD_CASES, GD_CASES, HUB, _dev, _np, _seg_sum, _st, check_g_a_dst, device_graph,
                                         galpha_for, host_adjacency, logits_case, ref_sddmm, ref_softmax_bwd,
                                         ref_softmax_fwd, run_softmax_bwd, run_softmax_fwd, sddmm_operands, seg_graph,
                                         seg_lens, seg_of, seg_rel_err_on)

gpu = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5

#: (in, H, C, concat) of the layer tests
SHAPES = [(256, 4, 64, True), (256, 8, 32, True), (25, 2, 256, True), (21, 2, 128, True), (64, 3, 20, True),
          (32, 5, 3, True), (16, 4, 1, True), (32, 1, 64, False), (256, 4, 64, False), (64, 3, 20, False)]
GRAPHS = ["multigraph", "hub", "n1", "e0", "golden_rest", "golden_rig"]
#: logit regimes of the direct tests: scales 0.1 / 1 / 8 / 30 at slope 0.2, and slope 0
HEAD_CASES = ["normal0.1", "normal1", "normal8", "normal30", "slope0"]


# --------------------------------------------------------------------------- #
# restatements for H heads (dt = np.float32: ref32, np.float64: truth64); per-node arrays [N, H], per-edge [E, H]
# --------------------------------------------------------------------------- #
def heads_softmax_fwd(ptr, other, a_src, a_dst, slope, dt):
    return np.stack([ref_softmax_fwd(ptr, other, a_src[:, k], a_dst[:, k], slope, dt) for k in range(a_src.shape[1])], 1)


def heads_softmax_bwd(ptr, other, a_src, a_dst, slope, alpha, galpha, dt):
    """(ge [E, H], g_a_dst [N, H])"""
    r = [ref_softmax_bwd(ptr, other, a_src[:, k], a_dst[:, k], slope, alpha[:, k], galpha[:, k], dt)
         for k in range(a_src.shape[1])]
    return np.stack([a for a, _ in r], 1), np.stack([b for _, b in r], 1)


def heads_sddmm(ptr, other, g, h, nh, dt):
    c = h.shape[1] // nh
    return np.stack([ref_sddmm(ptr, other, g[:, k * c:(k + 1) * c], h[:, k * c:(k + 1) * c], dt) for k in range(nh)], 1)


def heads_aggregate(ptr, other, alpha, x, nh, mean, dt):
    """out[i, k, :] = sum_p alpha[p, k] x[other[p], k, :], heads side by side or averaged"""
    n, c = len(ptr) - 1, x.shape[1] // nh
    msg = alpha.astype(dt)[:, :, None] * x.astype(dt).reshape(len(x), nh, c)[other]
    out = np.zeros((n, nh, c), dt)
    np.add.at(out, seg_of(ptr), msg)
    return out.mean(1, dtype=dt) if mean else out.reshape(n, nh * c)


def heads_by_source(other, v, n, dt):
    out = np.zeros((n, v.shape[1]), dt)
    np.add.at(out, other, v.astype(dt))
    return out


def heads_logits(case, ptr, other, nh, seed):
    per = [logits_case(case, ptr, other, seed + 17 * k) for k in range(nh)]
    return (np.ascontiguousarray(np.stack([p[0] for p in per], 1)), np.ascontiguousarray(np.stack([p[1] for p in per], 1)),
            per[0][2])


def heads_galpha(ptr, nh, seed):
    return np.ascontiguousarray(np.stack([galpha_for(ptr, seed + k) for k in range(nh)], 1))


# --------------------------------------------------------------------------- #
# CPU
# --------------------------------------------------------------------------- #
def test_constructor_parameters_and_state_dict():
    for concat in (True, False):
        torch.manual_seed(0)
        conv = dc.nn.GATConv(21, 64, heads=4, concat=concat)
        sd = conv.state_dict()
        assert set(sd) == {"lin.weight", "att_src", "att_dst", "bias"}
        assert sd["lin.weight"].shape == (256, 21)
        assert sd["att_src"].shape == (1, 4, 64) and sd["att_dst"].shape == (1, 4, 64)
        assert sd["bias"].shape == ((256,) if concat else (64,))
        assert "heads=4" in repr(conv)
        assert conv.graph_flags() == dict(self_loops=True, normalize=False)
        bound = float(np.sqrt(6.0 / (4 + 64)))
        for _ in range(3):
            conv.reset_parameters()
            for att in (conv.att_src, conv.att_dst):
                assert 0.5 * bound < float(att.detach().abs().max()) <= bound
            assert float(conv.lin.weight.detach().abs().max()) <= float(np.sqrt(6.0 / (21 + 256)))
            assert float(conv.bias.detach().abs().max()) == 0.0
        assert dc.nn.GATConv(21, 64, heads=4, concat=concat, bias=False).bias is None
    ref = pyg_ref.GATConv(21, 64, heads=4)
    conv = dc.nn.GATConv(21, 64, heads=4)
    conv.load_state_dict(ref.state_dict(), strict=True)
    for k, v in ref.state_dict().items():
        assert torch.equal(conv.state_dict()[k], v)
    one = dc.nn.GATConv(21, 64)                                  # unchanged
    assert one.heads == 1 and one.concat is True
    assert {k: tuple(v.shape) for k, v in one.state_dict().items()} == {
        "lin.weight": (64, 21), "att_src": (1, 1, 64), "att_dst": (1, 1, 64), "bias": (64,)}
    with pytest.raises(ValueError):
        dc.nn.GATConv(21, 64, heads=0)
    with pytest.raises(RuntimeError, match="HIP device"):       # no CPU path with several heads either
        conv(torch.zeros(5, 21), torch.zeros(2, 3, dtype=torch.long))


def _entry_calls():
    """name -> call(N, H, C, ptrs given?) of every entry of dc_gat_heads.hip with otherwise valid arguments"""
    L = _lib.lib()
    p = lambda ok: 64 if ok else None                           # any non-null address: rejected calls never touch it

    def ws(n, h, c):
        return max(L.dc_colsum_workspace_bytes(max(n, 0), max(h * c, 1), 2), 16)
    return {
        "dc_gat_alpha_heads_fwd": lambda n, h, c, ok: L.dc_gat_alpha_heads_fwd(p(ok), h * c, p(ok), p(ok), p(ok), p(ok), n, h, c, None),
        "dc_gat_edge_softmax_heads_fwd": lambda n, h, c, ok: L.dc_gat_edge_softmax_heads_fwd(p(ok), p(ok), p(ok), p(ok), 0.2, p(ok), n, h, None),
        "dc_spmm_f32_heads_bias_act": lambda n, h, c, ok: L.dc_spmm_f32_heads_bias_act(p(ok), p(ok), p(ok), p(ok), h * c, None, 0, 0, p(ok), h * c, n, h, c, None),
        "dc_sddmm_f32_heads": lambda n, h, c, ok: L.dc_sddmm_f32_heads(p(ok), p(ok), p(ok), h * c, p(ok), h * c, p(ok), n, h, c, None),
        "dc_gat_edge_softmax_heads_bwd": lambda n, h, c, ok: L.dc_gat_edge_softmax_heads_bwd(p(ok), p(ok), p(ok), p(ok), 0.2, p(ok), p(ok), p(ok), p(ok), n, h, None),
        "dc_segment_sum_f32_heads": lambda n, h, c, ok: L.dc_segment_sum_f32_heads(p(ok), None, p(ok), p(ok), n, h, None),
        "dc_gather_f32_heads": lambda n, h, c, ok: L.dc_gather_f32_heads(p(ok), p(ok), p(ok), p(ok), n, h, None),
        "dc_spread_heads_f32": lambda n, h, c, ok: L.dc_spread_heads_f32(p(ok), c, p(ok), h * c, n, h, c, None),
        "dc_gat_alpha_heads_bwd": lambda n, h, c, ok: L.dc_gat_alpha_heads_bwd(p(ok), h * c, p(ok), p(ok), p(ok), p(ok), p(ok), h * c, n, h, c, p(ok), ws(n, h, c), p(ok), p(ok), 0, None),
    }


def test_abi_argument_errors_of_the_heads_entries_without_gpu():
    """null pointers, H < 1, C < 1 and negative N: -1 and a message, before any HIP call (no device here)."""
    L = _lib.lib()
    calls = _entry_calls()
    declared = [n for n in _lib.exported_names() if "heads" in n]
    assert sorted(declared) == sorted(calls)
    for name, call in calls.items():
        assert call(3, 4, 16, False) == -1 and name.encode() in L.dc_last_error() and b"null" in L.dc_last_error(), name
        assert call(-1, 4, 16, True) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, 0, 16, True) == -1 and name.encode() in L.dc_last_error(), name
        assert call(3, -2, 16, True) == -1, name
        if name not in ("dc_gat_edge_softmax_heads_fwd", "dc_gat_edge_softmax_heads_bwd", "dc_segment_sum_f32_heads",
                        "dc_gather_f32_heads"):                 # (these have no C: rows of H / W floats)
            assert call(3, 4, 0, True) == -1 and name.encode() in L.dc_last_error(), name
            assert call(3, 4, -1, True) == -1, name
    # the column-sum pass keeps the divisibility rule of dc_gnn_epi.hip
    assert calls["dc_gat_alpha_heads_bwd"](3, 3, 20, True) == -1 and b"divides" in L.dc_last_error()
    # leading dimensions
    assert L.dc_sddmm_f32_heads(64, 64, 64, 8, 64, 64, 64, 3, 4, 16, None) == -1 and b"leading" in L.dc_last_error()


@pytest.mark.parametrize("nh,c", [(4, 16), (3, 5), (1, 8)])
def test_restatements_on_the_cpu(nh, c):
    """float64 restatements == oracle.pyg_ref (double) and torch autograd; float32 ones well inside the bar."""
    lens = seg_lens(257)
    n = len(lens)
    ptr, other, dst = host_adjacency(lens, 5)
    ei = np.stack([other, dst])                                  # self loops included: the oracle removes and re-adds them
    seg_err = seg_rel_err_on(ptr)
    rng = np.random.default_rng(nh * 100 + c)
    fi = 12
    x = rng.uniform(-1, 1, (n, fi)).astype(np.float32)
    gup = rng.uniform(0.5, 1.5, (n, nh * c)).astype(np.float32)
    torch.manual_seed(nh + c)
    slope = float(np.float32(0.2))                               # the kernels' slope is a float32
    conv = pyg_ref.GATConv(fi, c, heads=nh, negative_slope=slope).double()
    with torch.no_grad():
        conv.bias.uniform_(-0.3, 0.3)
    h = conv.lin(torch.from_numpy(x).double()).detach()
    a_src = (h.view(n, nh, c) * conv.att_src).sum(-1).detach().numpy()
    a_dst = (h.view(n, nh, c) * conv.att_dst).sum(-1).detach().numpy()
    a64 = heads_softmax_fwd(ptr, other, a_src, a_dst, 0.2, np.float64)
    out64 = heads_aggregate(ptr, other, a64, h.numpy(), nh, False, np.float64)
    want = conv(torch.from_numpy(x).double(), torch.from_numpy(ei)).detach().numpy()
    assert rel_err(out64 + conv.bias.detach().numpy(), want) < 1e-12
    mean64 = heads_aggregate(ptr, other, a64, h.numpy(), nh, True, np.float64)
    assert rel_err(mean64, out64.reshape(n, nh, c).mean(1)) < 1e-12
    # backward through the same graph in torch
    ts = torch.from_numpy(a_src).requires_grad_(True)
    td = torch.from_numpy(a_dst).requires_grad_(True)
    th = h.clone().requires_grad_(True)
    to, tdst = torch.from_numpy(other), torch.from_numpy(dst)
    al = pyg_ref.segment_softmax(F.leaky_relu(ts[to] + td[tdst], slope), tdst, n)
    al.retain_grad()
    out = pyg_ref.scatter_sum(al.unsqueeze(-1) * th.view(n, nh, c)[to], tdst, n).view(n, nh * c)
    (out * torch.from_numpy(gup).double()).sum().backward()
    assert max(seg_err(a64[:, k], al.detach().numpy()[:, k]) for k in range(nh)) < 1e-12
    galpha = heads_sddmm(ptr, other, gup, h.numpy(), nh, np.float64)
    assert rel_err(galpha, al.grad.numpy()) < 1e-12
    ge64, gd64 = heads_softmax_bwd(ptr, other, a_src, a_dst, 0.2, a64, galpha, np.float64)
    assert rel_err(gd64, td.grad.numpy()) < 1e-9
    assert rel_err(heads_by_source(other, ge64, n, np.float64), ts.grad.numpy()) < 1e-9
    gh64 = np.zeros((n, nh, c))
    np.add.at(gh64, other, a64[:, :, None] * gup.astype(np.float64).reshape(n, nh, c)[seg_of(ptr)])
    assert rel_err(gh64.reshape(n, -1), th.grad.numpy()) < 1e-12
    # float32 restatements: what fp32 alone costs here
    a32 = heads_softmax_fwd(ptr, other, a_src.astype(np.float32), a_dst.astype(np.float32), 0.2, np.float32)
    assert a32.dtype == np.float32
    a64f = heads_softmax_fwd(ptr, other, a_src.astype(np.float32), a_dst.astype(np.float32), 0.2, np.float64)
    for k in range(nh):
        assert seg_err(a32[:, k], a64f[:, k]) < 0.5 * TOL
    h32 = h.numpy().astype(np.float32)
    assert row_rel_err(heads_aggregate(ptr, other, a32, h32, nh, False, np.float32),
                       heads_aggregate(ptr, other, a32, h32, nh, False, np.float64)) < 0.5 * TOL


# --------------------------------------------------------------------------- #
# GPU: the layer
# --------------------------------------------------------------------------- #
def _graph(kind, seed):
    """(n, edge_index [2, E] int64)"""
    if kind == "multigraph":
        return 300, random_multigraph(300, 2400, seed)
    if kind == "hub":
        lens = seg_lens(300)
        return 300, seg_graph(lens, seed)
    if kind == "n1":
        return 1, np.zeros((2, 1), np.int64)                    # one node and its self loop
    if kind == "e0":
        return 50, np.zeros((2, 0), np.int64)
    z = load_golden("graphnet_gat_h32.npz")
    key = "rest" if kind == "golden_rest" else "rig"
    return z[key + "_x"].shape[0], z[key + "_edge_index"].astype(np.int64)


def _oracle_pair(fi, nh, c, seed):
    torch.manual_seed(seed)
    cpu = pyg_ref.GATConv(fi, c, heads=nh)
    with torch.no_grad():
        cpu.bias.uniform_(-0.3, 0.3)
    return cpu, copy.deepcopy(cpu).double()


def _oracle_run(mod, x, ei, gup, concat, dtype):
    """forward + backward of the oracle; concat=False: its bias-free concat output, mean over heads, + bias[:C]"""
    for p in mod.parameters():
        p.grad = None
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    if concat:
        out = mod(xt, torch.from_numpy(ei))
    else:
        nh, c = mod.heads, mod.out_channels
        out = (mod(xt, torch.from_numpy(ei)) - mod.bias).view(-1, nh, c).mean(1) + mod.bias[:c]
    (out * torch.from_numpy(gup).to(dtype)).sum().backward()
    grads = {n: p.grad.detach().numpy().copy() for n, p in mod.named_parameters()}
    if not concat:
        grads["bias"] = grads["bias"][:mod.out_channels]
    return out.detach().numpy(), xt.grad.numpy(), grads


def _device_conv(cpu, fi, nh, c, concat):
    conv = dc.nn.GATConv(fi, c, heads=nh, concat=concat)
    sd = {k: v.clone() for k, v in cpu.state_dict().items()}
    if not concat:
        sd["bias"] = sd["bias"][:c].clone()
    conv.load_state_dict(sd, strict=True)
    return conv.to(DEV)


def _device_run(conv, x, ei, gup, **kw):
    for p in conv.parameters():
        p.grad = None
    xg = torch.from_numpy(x).to(DEV).requires_grad_(True)
    out = ops.resolve(conv(xg, torch.from_numpy(ei).to(DEV), **kw))
    (out * torch.from_numpy(gup).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), xg.grad, {n: p.grad.detach().clone() for n, p in conv.named_parameters()}


@gpu
@pytest.mark.parametrize("kind", GRAPHS)
@pytest.mark.parametrize("fi,nh,c,concat", SHAPES)
def test_layer_parity(fi, nh, c, concat, kind):
    """forward and every gradient against oracle.pyg_ref.GATConv, float32 and float64, at 1e-5."""
    torch.set_num_threads(1)
    n, ei = _graph(kind, 3)
    rng = np.random.default_rng(fi + nh + c)
    x = rng.uniform(-1, 1, (n, fi)).astype(np.float32)
    gup = rng.uniform(0.5, 1.5, (n, nh * c if concat else c)).astype(np.float32)
    cpu, c64 = _oracle_pair(fi, nh, c, 11)
    o32, gx32, gp32 = _oracle_run(cpu, x, ei, gup, concat, torch.float32)
    o64, gx64, gp64 = _oracle_run(c64, x, ei, gup, concat, torch.float64)
    clear_cache()
    conv = _device_conv(cpu, fi, nh, c, concat)
    _lib.kernel_trace(True)
    og, gxg, gpg = _device_run(conv, x, ei, gup)
    counts = _lib.kernel_trace_counts()
    _lib.kernel_trace(False)
    if nh > 1:                                                   # the per-edge work runs on the new kernels at every width
        for k in ("k_gat_softmax_heads_fwd", "k_gat_softmax_heads_bwd", "k_spmm_heads", "k_sddmm_heads",
                  "k_segment_sum_heads", "k_gather_heads"):
            assert any(k in name for name in counts), (k, counts)
        assert not any(k in name for name in counts for k in ("k_gat_softmax_fwd", "k_sddmm<", "k_spmm_wave")), counts
    tag = f"GATConv {fi}->{nh}x{c} concat={concat} {kind}"
    assert og.shape == o32.shape
    assert_parity(_np(og), o32, o64, TOL, f"{tag} forward")
    assert_parity(_np(og), o32, o64, TOL, f"{tag} forward per row", metric=row_rel_err)
    assert_parity(_np(gxg), gx32, gx64, TOL, f"{tag} x.grad")
    for name in ("lin.weight", "att_src", "att_dst", "bias"):
        assert_parity(_np(gpg[name]), gp32[name], gp64[name], TOL, f"{tag} {name}.grad")


@gpu
@pytest.mark.parametrize("fi,nh,c", [(256, 4, 64), (25, 3, 20)])
def test_multi_head_layer_equals_its_heads_as_single_head_layers(fi, nh, c):
    """A multi-head layer against H existing heads=1 layers built from its weight slices, concatenated."""
    torch.set_num_threads(1)
    n, ei = _graph("multigraph", 8)
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (n, fi)).astype(np.float32)
    gup = rng.uniform(0.5, 1.5, (n, nh * c)).astype(np.float32)
    cpu, c64 = _oracle_pair(fi, nh, c, 21)
    o64, gx64, gp64 = _oracle_run(c64, x, ei, gup, True, torch.float64)
    clear_cache()
    conv = _device_conv(cpu, fi, nh, c, True)
    og, gxg, gpg = _device_run(conv, x, ei, gup)
    singles = []
    for k in range(nh):
        s = dc.nn.GATConv(fi, c).to(DEV)
        with torch.no_grad():
            s.lin.weight.copy_(conv.lin.weight[k * c:(k + 1) * c])
            s.att_src.copy_(conv.att_src[:, k:k + 1])
            s.att_dst.copy_(conv.att_dst[:, k:k + 1])
            s.bias.copy_(conv.bias[k * c:(k + 1) * c])
        singles.append(s)
    xg = torch.from_numpy(x).to(DEV).requires_grad_(True)
    tei = torch.from_numpy(ei).to(DEV)
    oc = torch.cat([ops.resolve(s(xg, tei)) for s in singles], 1)
    (oc * torch.from_numpy(gup).to(DEV)).sum().backward()
    tag = f"heads vs singles {fi}->{nh}x{c}"
    assert_parity(_np(og), _np(oc), o64, TOL, f"{tag} forward")
    assert_parity(_np(gxg), _np(xg.grad), gx64, TOL, f"{tag} x.grad")
    cat = lambda name, dim: torch.cat([dict(s.named_parameters())[name].grad for s in singles], dim)
    assert_parity(_np(gpg["lin.weight"]), _np(cat("lin.weight", 0)), gp64["lin.weight"], TOL, f"{tag} lin.weight.grad")
    assert_parity(_np(gpg["att_src"]), _np(cat("att_src", 1)), gp64["att_src"], TOL, f"{tag} att_src.grad")
    assert_parity(_np(gpg["att_dst"]), _np(cat("att_dst", 1)), gp64["att_dst"], TOL, f"{tag} att_dst.grad")
    assert_parity(_np(gpg["bias"]), _np(cat("bias", 0)), gp64["bias"], TOL, f"{tag} bias.grad")


@gpu
@pytest.mark.parametrize("fi,nh,c,concat", [(256, 4, 64, True), (64, 3, 20, True), (256, 4, 64, False), (64, 3, 20, False)])
def test_bit_for_bit_relu_deferred_and_repeat(fi, nh, c, concat):
    n, ei = _graph("hub", 4)
    rng = np.random.default_rng(9)
    x = rng.uniform(-1, 1, (n, fi)).astype(np.float32)
    gup = rng.uniform(0.5, 1.5, (n, nh * c if concat else c)).astype(np.float32)
    cpu, _ = _oracle_pair(fi, nh, c, 31)
    clear_cache()
    conv = _device_conv(cpu, fi, nh, c, concat)
    tei, xg = torch.from_numpy(ei).to(DEV), torch.from_numpy(x).to(DEV)
    plain = ops.resolve(conv(xg, tei)).clone()
    assert plain.shape == (n, nh * c if concat else c)
    want = torch.relu(plain)
    assert (plain < 0).any() and (plain > 0).any()
    assert torch.equal(conv(xg, tei, relu=True), want)
    y = conv(xg, tei)
    assert type(y).__name__ == "DeferredActivation" and y.shape == plain.shape
    assert torch.equal(F.relu(y), want)
    # two consecutive runs: same bits in the output and in every gradient
    for kw in ({}, {"relu": True}):
        a = _device_run(conv, x, ei, gup, **kw)
        b = _device_run(conv, x, ei, gup, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for name in a[2]:
            assert torch.equal(a[2][name], b[2][name]), name


@gpu
def test_one_head_mean_equals_one_head_concat_bitwise():
    fi, c = 32, 64
    n, ei = _graph("multigraph", 6)
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, (n, fi)).astype(np.float32)
    gup = rng.uniform(0.5, 1.5, (n, c)).astype(np.float32)
    cpu, _ = _oracle_pair(fi, 1, c, 41)
    clear_cache()
    a = _device_run(_device_conv(cpu, fi, 1, c, True), x, ei, gup)
    b = _device_run(_device_conv(cpu, fi, 1, c, False), x, ei, gup)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for name in a[2]:
        assert torch.equal(a[2][name], b[2][name]), name
    # ... and the multi-head entries at H = 1 give the bits of the single-head ones where the order of sums is the same
    g = GraphIndex(torch.from_numpy(ei).to(DEV), n, self_loops=True, normalize=False)
    h = torch.from_numpy(rng.uniform(-1, 1, (n, c)).astype(np.float32)).to(DEV)
    a_src, a_dst = (torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV) for _ in range(2))
    al1 = ops._gat_edge_softmax(g, a_src, a_dst, 0.2, n)
    alh = ops._heads_softmax_fwd(g, a_src.view(n, 1), a_dst.view(n, 1), 0.2, n, 1)
    assert torch.equal(al1, alh.view(-1))
    bias = torch.from_numpy(rng.standard_normal(c).astype(np.float32)).to(DEV)
    for mean in (False, True):
        assert torch.equal(ops._agg_bias_act(g.fwd, al1, h, bias, True), ops._heads_agg(g.fwd, alh, h, bias, True, mean, 1, c))


@gpu
def test_two_stacked_layers_captured_and_replayed():
    """forward + backward of two GATConv(heads=4) layers on one stream under torch.cuda.graph; three replays with new x
    in the static input, each bit-identical to the eager run on that input."""
    n, ei = _graph("multigraph", 12)
    fi, nh, c = 32, 4, 16
    torch.manual_seed(3)
    l1 = dc.nn.GATConv(fi, c, heads=nh).to(DEV)
    l2 = dc.nn.GATConv(nh * c, c, heads=nh, concat=False).to(DEV)
    with torch.no_grad():
        l1.bias.uniform_(-0.3, 0.3)
        l2.bias.uniform_(-0.3, 0.3)
    params = list(l1.parameters()) + list(l2.parameters())
    tei = torch.from_numpy(ei).to(DEV)
    rng = np.random.default_rng(1)
    xs = [torch.from_numpy(rng.uniform(-1, 1, (n, fi)).astype(np.float32)).to(DEV) for _ in range(4)]
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
    for i in (1, 2, 3):
        with torch.no_grad():
            static_x.copy_(xs[i])
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(snapshot(out), eager[i]):
            assert torch.equal(got, want), i


# --------------------------------------------------------------------------- #
# GPU: the per-edge entries called directly
# --------------------------------------------------------------------------- #
@gpu
@pytest.mark.parametrize("nh", [2, 5, 8, 11])
@pytest.mark.parametrize("case", HEAD_CASES)
def test_edge_softmax_heads_per_edge_and_head(case, nh):
    """LENS + the 5,000-edge hub, H = 2 / 5 / 8 / 11 (one block of heads; a partly filled one; two blocks), forward and
    backward per edge and head; head k against the single-head entries on column k."""
    n = 131
    g, ptr, other, lens = device_graph(n, 9 + nh)
    e, cap = int(ptr[-1]), g.capacity
    seg_err = seg_rel_err_on(ptr)
    a_src, a_dst, slope = heads_logits(case, ptr, other, nh, 300)
    ts, td = _dev(a_src), _dev(a_dst)
    alpha = ops._heads_softmax_fwd(g, ts, td, slope, n, nh)
    assert alpha.shape == (max(cap, 1), nh) and (alpha[e:] == 0).all()
    assert torch.equal(alpha, ops._heads_softmax_fwd(g, ts, td, slope, n, nh))
    got = _np(alpha)[:e]
    a32 = heads_softmax_fwd(ptr, other, a_src, a_dst, slope, np.float32)
    a64 = heads_softmax_fwd(ptr, other, a_src, a_dst, slope, np.float64)
    galpha = heads_galpha(ptr, nh, 11)
    tg = torch.zeros_like(alpha)
    tg[:e] = _dev(galpha)
    ge, gd = ops._heads_softmax_bwd(g, ts, td, slope, alpha, tg, n, nh)
    ge2, gd2 = ops._heads_softmax_bwd(g, ts, td, slope, alpha, tg, n, nh)
    assert torch.equal(ge, ge2) and torch.equal(gd, gd2) and (ge[e:] == 0).all()
    assert torch.isfinite(ge).all() and torch.isfinite(gd).all()
    ge32, gd32 = heads_softmax_bwd(ptr, other, a_src, a_dst, slope, got, galpha, np.float32)
    ge64, gd64 = heads_softmax_bwd(ptr, other, a_src, a_dst, slope, got, galpha, np.float64)
    g_a_src = ops._heads_segment_sum(g.bwd.ptr, g.bwd_to_fwd(), ge, n, nh)
    for k in range(nh):
        tag = f"{case} H={nh} head {k}"
        assert_parity(got[:, k], a32[:, k], a64[:, k], TOL, f"alpha {tag}", metric=seg_err)
        sums = _seg_sum(got[:, k].astype(np.float64), seg_of(ptr), n)
        assert (np.abs(sums - 1) <= lens * 2.0 ** -23).all(), tag
        check_g_a_dst(tag, ptr, _np(ge)[:, k], _np(gd)[:, k])
        if case in BWD_CASES:
            assert_parity(_np(ge)[:e, k], ge32[:, k], ge64[:, k], TOL, f"ge {tag}", metric=seg_err)
        if case in GD_CASES:
            assert_parity(_np(gd)[:, k], gd32[:, k], gd64[:, k], TOL, f"g_a_dst {tag}")
        # the single-head entries on column k
        a1 = run_softmax_fwd(g.fwd.ptr, g.fwd.other, ts[:, k].contiguous(), td[:, k].contiguous(), slope, n, cap)
        d = seg_err(got[:, k], _np(a1)[:e])
        record_parity(f"alpha {tag} vs dc_gat_edge_softmax_fwd", d, metric="seg_rel_err")
        assert d < TOL
        ge1, gd1 = run_softmax_bwd(g.fwd.ptr, g.fwd.other, ts[:, k].contiguous(), td[:, k].contiguous(), slope, a1,
                                   tg[:, k].contiguous(), n)
        d = max(rel_err(_np(ge)[:e, k], _np(ge1)[:e]), rel_err(_np(gd)[:, k], _np(gd1)))
        record_parity(f"ge, g_a_dst {tag} vs dc_gat_edge_softmax_bwd", d)
        assert d < TOL
        s1 = torch.empty(n, device=DEV)
        _lib.check(_lib.lib().dc_segment_sum_f32(g.bwd.ptr.data_ptr(), g.bwd_to_fwd().data_ptr(),
                                                 ge[:, k].contiguous().data_ptr(), s1.data_ptr(), n, _st()), "segsum")
        assert torch.equal(g_a_src[:, k], s1), tag
    if case == "slope0":
        assert (_np(ge)[:e][(a_src[other] + a_dst[seg_of(ptr)]) <= 0] == 0.0).all()
    # re-ordering by source, H floats per edge
    b2f = _np(g.bwd_to_fwd()).astype(np.int64)[:e]
    ab = ops._heads_gather(g, alpha, g.bwd_to_fwd(), nh)
    assert np.array_equal(_np(ab)[:e], got[b2f]) and (ab[e:] == 0).all()


@gpu
@pytest.mark.parametrize("nh,c", [(4, 64), (8, 32), (2, 128), (3, 20), (5, 3), (4, 1), (2, 512), (1, 64), (6, 64)])
def test_sddmm_and_aggregation_heads(nh, c):
    """dc_sddmm_f32_heads (one-signed operands) and dc_spmm_f32_heads_bias_act per edge / row and head: the 16-byte forms
    (a head = 1 .. 64 lanes; rows wider than the register-held 512 columns), the general form; column windows."""
    n, f = 131, nh * c
    g, ptr, other, lens = device_graph(n, 70 + nh, hub=600)
    e = int(ptr[-1])
    seg_err = seg_rel_err_on(ptr)
    hg, hh = sddmm_operands(n, f, f)
    d32, d64 = heads_sddmm(ptr, other, hg, hh, nh, np.float32), heads_sddmm(ptr, other, hg, hh, nh, np.float64)
    tg, th = _dev(hg), _dev(hh)
    _lib.kernel_trace(True)
    d = ops._heads_sddmm(g, tg, th, nh, c)
    counts = _lib.kernel_trace_counts()
    _lib.kernel_trace(False)
    fast = c % 4 == 0 and (c // 4) & (c // 4 - 1) == 0 and c // 4 <= 64
    assert any(("k_sddmm_heads_v4" if fast else "k_sddmm_heads_any") in k for k in counts), counts
    assert (d[e:] == 0).all() and torch.equal(d, ops._heads_sddmm(g, tg, th, nh, c))
    wide_g = torch.full((n, f + 12), 1e30, device=DEV)
    wide_g[:, 4:4 + f] = tg
    assert torch.equal(d, ops._heads_sddmm(g, wide_g[:, 4:4 + f], th, nh, c))      # ld > F, same form
    for k in range(nh):
        assert_parity(_np(d)[:e, k], d32[:, k], d64[:, k], TOL, f"sddmm heads {nh}x{c} head {k}", metric=seg_err)
        d1 = torch.zeros(max(g.capacity, 1), device=DEV)
        _lib.check(_lib.lib().dc_sddmm_f32(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), tg[:, k * c:].data_ptr(), f,
                                           th[:, k * c:].data_ptr(), f, d1.data_ptr(), n, c, _st()), "dc_sddmm_f32")
        dist = seg_err(_np(d)[:e, k], _np(d1)[:e])
        record_parity(f"sddmm heads {nh}x{c} head {k} vs dc_sddmm_f32", dist, metric="seg_rel_err")
        assert dist < TOL
    # aggregation: weights of a softmax, features of both signs against float64 per row; head k = the single-head launch
    a_src, a_dst, slope = heads_logits("normal1", ptr, other, nh, 5)
    alpha = ops._heads_softmax_fwd(g, _dev(a_src), _dev(a_dst), slope, n, nh)
    al = _np(alpha)[:e]
    rng = np.random.default_rng(c)
    x = rng.uniform(-1, 1, (n, f)).astype(np.float32)
    tx = _dev(x)
    bias_c, bias_m = _dev(rng.standard_normal(f).astype(np.float32)), _dev(rng.standard_normal(c).astype(np.float32))
    y = ops._heads_agg(g.fwd, alpha, tx, None, False, False, nh, c)
    assert_parity(_np(y), heads_aggregate(ptr, other, al, x, nh, False, np.float32),
                  heads_aggregate(ptr, other, al, x, nh, False, np.float64), TOL, f"aggregation {nh}x{c} per row",
                  metric=row_rel_err)
    for k in range(nh):
        y1 = ops._agg_bias_act(g.fwd, alpha[:, k].contiguous(), tx[:, k * c:(k + 1) * c], None, False)
        assert torch.equal(y[:, k * c:(k + 1) * c], y1), k      # same sums in the same order
    assert torch.equal(ops._heads_agg(g.fwd, alpha, tx, bias_c, True, False, nh, c), torch.relu(y + bias_c))
    assert torch.equal(ops._heads_agg(g.fwd, alpha, tx, bias_c, False, False, nh, c), y + bias_c)
    m = ops._heads_agg(g.fwd, alpha, tx, None, False, True, nh, c)
    assert m.shape == (n, c)
    assert_parity(_np(m), heads_aggregate(ptr, other, al, x, nh, True, np.float32),
                  heads_aggregate(ptr, other, al, x, nh, True, np.float64), TOL, f"mean aggregation {nh}x{c} per row",
                  metric=row_rel_err)
    assert torch.equal(ops._heads_agg(g.fwd, alpha, tx, bias_m, True, True, nh, c), torch.relu(m + bias_m))
    # the gradient of the mean
    sp = ops._heads_spread(m, nh, c)
    for k in range(1, nh):
        assert torch.equal(sp[:, k * c:(k + 1) * c], sp[:, :c]), k
    want = _np(m).astype(np.float64) / nh                        # one rounding of the exact quotient
    assert (np.abs(_np(sp[:, :c]) - want) <= 2.0 ** -24 * np.abs(want)).all()


@gpu
@pytest.mark.parametrize("nh,c", [(4, 64), (8, 32), (2, 128), (3, 20), (5, 3), (4, 1), (2, 512)])
def test_attention_dot_products_heads(nh, c):
    """dc_gat_alpha_heads_fwd at every width; dc_gat_alpha_heads_bwd where the column-sum pass takes the width."""
    n, f = 1000, nh * c
    rng = np.random.default_rng(f)
    h = (0.5 + rng.random((n, f))).astype(np.float32)            # one-signed: no cancellation in the dot products
    a_s, a_d = (0.5 + rng.random(f)).astype(np.float32), (0.5 + rng.random(f)).astype(np.float32)
    th, ts, td = _dev(h), _dev(a_s), _dev(a_d)
    a_src, a_dst = ops._heads_alpha_fwd(th, ts, td, nh, c)
    for got, att, nm in ((a_src, a_s, "a_src"), (a_dst, a_d, "a_dst")):
        w32 = (h.reshape(n, nh, c) * att.reshape(1, nh, c)).sum(-1, dtype=np.float32)
        w64 = (h.astype(np.float64).reshape(n, nh, c) * att.astype(np.float64).reshape(1, nh, c)).sum(-1)
        assert_parity(_np(got), w32, w64, TOL, f"{nm} heads {nh}x{c}", metric=row_rel_err)
    if not ops.fused_gnn_ok(th):
        return
    if c % 4 == 0:
        for k in range(nh):
            s1, d1 = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
            _lib.check(_lib.lib().dc_gat_alpha_fwd(th[:, k * c:].data_ptr(), f, ts[k * c:].data_ptr(), td[k * c:].data_ptr(),
                                                   s1.data_ptr(), d1.data_ptr(), n, c, _st()), "dc_gat_alpha_fwd")
            dist = max(rel_err(_np(a_src[:, k]), _np(s1)), rel_err(_np(a_dst[:, k]), _np(d1)))
            record_parity(f"a_src, a_dst heads {nh}x{c} head {k} vs dc_gat_alpha_fwd", dist)
            assert dist < TOL
    ga_s = (0.5 + rng.random((n, nh))).astype(np.float32)
    ga_d = (0.5 + rng.random((n, nh))).astype(np.float32)
    gh0 = rng.uniform(-1, 1, (n, f)).astype(np.float32)
    outs = []
    for _ in range(2):
        gh = _dev(gh0)
        gs, gd = torch.empty(f, device=DEV), torch.empty(f, device=DEV)
        ops._heads_alpha_bwd(th, _dev(ga_s), _dev(ga_d), ts, td, gh, nh, c, gs, gd, False)
        outs.append((gh, gs, gd))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    gh, gs, gd = outs[0]

    def want(dt):
        s, d = np.repeat(ga_s.astype(dt), c, 1), np.repeat(ga_d.astype(dt), c, 1)
        return (gh0.astype(dt) + s * a_s.astype(dt) + d * a_d.astype(dt), (s * h.astype(dt)).sum(0, dtype=dt),
                (d * h.astype(dt)).sum(0, dtype=dt))
    for got, w32, w64, nm in zip((gh, gs, gd), want(np.float32), want(np.float64), ("gh", "g_att_src", "g_att_dst")):
        assert_parity(_np(got), w32, w64, TOL, f"{nm} heads {nh}x{c}")
    # accumulate into what the buffers hold (direct parameter-gradient mode)
    gs2, gd2 = gs.clone(), gd.clone()
    ops._heads_alpha_bwd(th, _dev(ga_s), _dev(ga_d), ts, td, _dev(gh0), nh, c, gs2, gd2, True)
    assert torch.equal(gs2, gs + gs) and torch.equal(gd2, gd + gd)
