"""``dc_contact_loss`` (dc_loss.hip: L1 + gradient-consistency loss and both gradients in one node pass, then a
one-workgroup reduction of the per-block partial sums) at the sizes and layouts the suite did not reach: 1 - 257 nodes,
more than 256 partials (N > 65,536: the strided loop of ``k_loss_final``), a 5,000-edge hub, isolated nodes, leading
dimensions above 3, exact zeros, no edges at all, and the error returns.

Reference: the stock formulation (``F.l1_loss`` + ``graphnet.gradient_consistency_loss``, models/losses.py:7-19) on the
CPU in fp32 and float64.  Gradients are compared PER NODE (``row_rel_err`` on [N, 3]) and for each loss separately.

Inputs, chosen for conditioning (``test_stock_formulation_and_conditioning_on_the_cpu`` keeps the choice checked):
the gradient of the consistency loss at node i is ``(1 / E) sum_k unit(n_i - n_k)`` over its neighbours k, with
``n = pred - target``.  Two things make a per-node comparison of PLAIN random data meaningless in fp32, whatever
computes it: ``n_i - n_k`` is formed as ``(t_i - t_k) - (p_i - p_k)``, a difference of numbers of order 1 whose rounding
error is 2^-24 / noise relative to the result; and the unit vectors of a node of degree 2 or 3 cancel to a few per cent
of their size somewhere among 70,000 nodes (the stock fp32 formulation is then 1e-4 - 1e-3 from float64 per node).  So
positions lie on a 2^-12 grid (the differences are exact), and the noise of every other node carries an offset of six
noise widths along x, so that a node's unit vectors to the other class all point the same way.
"""
import numpy as np
import pytest
import torch

from deformcontact_amd import _lib, ops
from deformcontact_amd.graph import GraphIndex, clear_cache, current_stream_ptr, graph_index
from deformcontact_amd.graphnet import gradient_consistency_loss
from tests.helpers import G, assert_parity, random_multigraph, row_rel_err

gpu = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
SIZES = [2, 255, 256, 257, 65536, 65537, 70001]
NOISE = [1.0, 0.1, 0.01]
HUB_EDGES = 5000


def make_edges(n, seed):
    """~6 edges per node with duplicates and self loops; from 255 nodes on a 5,000-edge hub (node 3, with 40 edges
    back out of it); the last n / 16 nodes are isolated - no edge at all."""
    m = n if n < 16 else n - n // 16
    ei = random_multigraph(m, 6 * m, seed)
    if n >= 255:
        rng = np.random.default_rng(seed + 1)
        hub = np.stack([rng.integers(0, m, HUB_EDGES), np.full(HUB_EDGES, 3)])
        ei = np.concatenate([ei, hub, hub[::-1][:, :40]], axis=1)
    return np.ascontiguousarray(ei).astype(np.int64)


def make_positions(n, noise, seed):
    """(pred, target) float32 [n, 3] on a 2^-12 grid; pred - target = noise * (normal + 6 e_x on odd nodes)."""
    rng = np.random.default_rng(seed)
    q = 2.0 ** -12
    tgt = np.round(rng.standard_normal((n, 3)) / q) * q
    nz = noise * (rng.standard_normal((n, 3)) + 6.0 * (np.arange(n) % 2)[:, None] * np.array([1.0, 0.0, 0.0]))
    pred = tgt + np.round(nz / q) * q
    assert np.array_equal(pred.astype(np.float32), pred) and np.array_equal(tgt.astype(np.float32), tgt)
    return pred.astype(np.float32), tgt.astype(np.float32)


def stock(pred, tgt, ei, dtype):
    """(l1, grad_l1, gcl, grad_gcl) of the stock formulation: ``backward`` once per loss."""
    t, e = torch.from_numpy(tgt).to(dtype), torch.from_numpy(ei)
    out = []
    for which in ("l1", "gcl"):
        p = torch.from_numpy(pred).to(dtype).requires_grad_(True)
        loss = torch.nn.functional.l1_loss(p, t) if which == "l1" else \
            gradient_consistency_loss(G(None, e, p), G(None, e, t))
        loss.backward()
        out += [float(loss.detach()), p.grad.numpy()]
    return out


def test_stock_formulation_and_conditioning_on_the_cpu():
    worst = 0.0
    for n in (2, 255, 500, 70001):
        ei = make_edges(n, n)
        for noise in NOISE:
            pred, tgt = make_positions(n, noise, n)
            l1_32, g1_32, gc_32, g2_32 = stock(pred, tgt, ei, torch.float32)
            l1_64, g1_64, gc_64, g2_64 = stock(pred, tgt, ei, torch.float64)
            assert abs(l1_32 - l1_64) <= 1e-6 * l1_64 and abs(gc_32 - gc_64) <= 1e-6 * gc_64, (n, noise)
            assert row_rel_err(g1_32, g1_64) < TOL
            worst = max(worst, row_rel_err(g2_32, g2_64))
            if n > 500:
                continue
            # the float64 reference against the formulas written out per edge
            p, t = pred.astype(np.float64), tgt.astype(np.float64)
            d = (t[ei[1]] - t[ei[0]]) - (p[ei[1]] - p[ei[0]])
            nrm = np.linalg.norm(d, axis=1)
            assert abs(nrm.sum() / ei.shape[1] - gc_64) <= 1e-12 * gc_64
            u = np.divide(d, nrm[:, None], out=np.zeros_like(d), where=nrm[:, None] > 0) / ei.shape[1]
            want = np.zeros_like(p)
            np.add.at(want, ei[1], -u)
            np.add.at(want, ei[0], u)
            assert row_rel_err(g2_64, want) < 1e-9
            assert np.array_equal(g1_64, np.sign(p - t) / (3 * n))
    # the fp32 formulation alone is inside the bar, per node, for every input the GPU tests use
    assert worst < TOL, worst
    # ... and 70,001 nodes make more partial sums than the final reduction has threads
    assert (70001 + 255) // 256 == 274 and (65537 + 255) // 256 == 257 and (65536 + 255) // 256 == 256


# --------------------------------------------------------------------------- #
# GPU
# --------------------------------------------------------------------------- #
def _np(t):
    return t.detach().cpu().numpy()


def fused(g, pred_t, tgt_t):
    """(l1, grad_l1, gcl, grad_gcl) through ``ops.contact_losses``: ``backward`` once on each loss."""
    p = pred_t.detach().requires_grad_(True)
    l1, gcl = ops.contact_losses(g, p, tgt_t)
    l1.backward(retain_graph=True)
    g1 = p.grad.clone()
    p.grad = None
    gcl.backward()
    return float(l1.detach()), _np(g1), float(gcl.detach()), _np(p.grad)


def entry(g, pred_t, ld_pred, tgt_t, ld_tgt, n, e, ws_short=0, stream=None, keep=None):
    """``dc_contact_loss`` itself -> (rc, losses [2], grad_l1, grad_gcl); with ``stream``: buffers, their fills and the
    launches all on that stream; ``keep`` takes the workspace (calls in flight at once must not share one)."""
    if stream is not None:
        with torch.cuda.stream(stream):
            return entry(g, pred_t, ld_pred, tgt_t, ld_tgt, n, e, ws_short=ws_short, keep=keep)
    L = _lib.lib()
    g1 = torch.full((max(n, 1), 3), 9.0, device=DEV)
    g2 = torch.full((max(n, 1), 3), 9.0, device=DEV)
    out = torch.full((2,), 9.0, device=DEV)
    nb = max(int(L.dc_contact_loss_workspace_bytes(max(n, 0))), 16)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    st = current_stream_ptr(torch.device(DEV))
    if keep is not None:
        keep.append(ws)
    rc = L.dc_contact_loss(g.fwd.ptr.data_ptr(), g.fwd.other.data_ptr(), g.bwd.ptr.data_ptr(), g.bwd.other.data_ptr(),
                           pred_t.data_ptr(), ld_pred, tgt_t.data_ptr(), ld_tgt, n, e, g1.data_ptr(), g2.data_ptr(),
                           out.data_ptr(), ws.data_ptr(), nb - ws_short, st)
    return rc, out, g1, g2


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_losses_and_each_gradient_per_node(n):
    ei = make_edges(n, n)
    tei = torch.from_numpy(ei).to(DEV)
    g = GraphIndex(tei, n, validate=True)
    for noise in NOISE:
        pred, tgt = make_positions(n, noise, n)
        l1_32, g1_32, gc_32, g2_32 = stock(pred, tgt, ei, torch.float32)
        l1_64, g1_64, gc_64, g2_64 = stock(pred, tgt, ei, torch.float64)
        l1, g1, gcl, g2 = fused(g, torch.from_numpy(pred).to(DEV), torch.from_numpy(tgt).to(DEV))
        print(f"N={n} noise={noise}: l1 {abs(l1 - l1_64) / l1_64:.2e} gcl {abs(gcl - gc_64) / gc_64:.2e} "
              f"grad_l1 {row_rel_err(g1, g1_64):.2e} grad_gcl {row_rel_err(g2, g2_64):.2e}")
        assert abs(l1 - l1_64) <= 1e-6 * abs(l1_64), (n, noise)
        assert abs(gcl - gc_64) <= 1e-6 * abs(gc_64), (n, noise)
        assert_parity(g1, g1_32, g1_64, TOL, f"grad_l1 per node N={n} noise={noise}", metric=row_rel_err)
        assert_parity(g2, g2_32, g2_64, TOL, f"grad_gcl per node N={n} noise={noise}", metric=row_rel_err)
        if n >= 16:                                          # isolated nodes: no consistency term at all
            assert (g2[n - n // 16:] == 0).all()


@gpu
def test_exact_zeros_where_prediction_equals_target():
    """pred == target on nodes 0..99: sign(0) = 0 in grad_l1; a consistency term between two such nodes is zero and
    has zero gradient (torch's norm at 0) - nodes 0..89 have all their neighbours among them."""
    n = 300
    inner = random_multigraph(100, 700, 1, isolated=False)
    outer = 100 + random_multigraph(200, 1400, 2, isolated=False)
    cross = np.stack([np.arange(90, 100), np.arange(100, 110)])
    ei = np.concatenate([inner[:, (inner < 90).all(0) | (inner >= 90).all(0)], outer, cross, cross[::-1]], axis=1)
    pred, tgt = make_positions(n, 0.1, 5)
    pred[:100] = tgt[:100]
    g = GraphIndex(torch.from_numpy(ei).to(DEV), n, validate=True)
    l1, g1, gcl, g2 = fused(g, torch.from_numpy(pred).to(DEV), torch.from_numpy(tgt).to(DEV))
    assert (g1[:100] == 0).all() and (g1[100:] != 0).any(axis=1).all()
    assert (g2[:90] == 0).all() and (np.abs(g2[90:100]).max(axis=1) > 0).all()
    l1_64, g1_64, gc_64, g2_64 = stock(pred, tgt, ei, torch.float64)
    l1_32, g1_32, gc_32, g2_32 = stock(pred, tgt, ei, torch.float32)
    assert (g1_64[:100] == 0).all() and (g2_64[:90] == 0).all() and np.array_equal(g1 == 0, g1_64 == 0)
    assert abs(l1 - l1_64) <= 1e-6 * l1_64 and abs(gcl - gc_64) <= 1e-6 * gc_64
    assert_parity(g1, g1_32, g1_64, TOL, "grad_l1 per node, exact zeros", metric=row_rel_err)
    assert_parity(g2, g2_32, g2_64, TOL, "grad_gcl per node, exact zeros", metric=row_rel_err)


@gpu
@pytest.mark.parametrize("n", [257, 70001])
def test_leading_dimensions_strided_views_streams_same_bits(n):
    ei = make_edges(n, n)
    e = ei.shape[1]
    g = GraphIndex(torch.from_numpy(ei).to(DEV), n, validate=True)
    pred, tgt = make_positions(n, 0.1, n)
    tp, tt = torch.from_numpy(pred).to(DEV), torch.from_numpy(tgt).to(DEV)
    rc, out0, a0, b0 = entry(g, tp, 3, tt, 3, n, e)
    assert rc == 0
    l1, g1, gcl, g2 = fused(g, tp, tt)
    assert l1 == float(out0[0]) and gcl == float(out0[1])
    assert np.array_equal(g1, _np(a0)) and np.array_equal(g2, _np(b0))      # (backward scales by exactly 1.0)
    # column windows of wider buffers: ld_pred = 8, ld_target = 5
    wp = torch.full((n, 8), float("nan"), device=DEV)
    wt = torch.full((n, 5), float("nan"), device=DEV)
    wp[:, 2:5], wt[:, 1:4] = tp, tt
    vp, vt = wp[:, 2:5], wt[:, 1:4]
    assert vp.stride(0) == 8 and vt.stride(0) == 5
    rc, out, a, b = entry(g, vp, 8, vt, 5, n, e)
    assert rc == 0 and torch.equal(out, out0) and torch.equal(a, a0) and torch.equal(b, b0)
    r = fused(g, vp, vt)                                     # the wrapper passes the row stride on
    assert r[0] == l1 and r[2] == gcl and np.array_equal(r[1], g1) and np.array_equal(r[3], g2)
    # stride(1) != 1: the wrapper's contiguous() branch
    cp, ct = tp.t().contiguous().t(), tt.t().contiguous().t()
    assert cp.stride(1) != 1 and torch.equal(cp, tp)
    r = fused(g, cp, ct)
    assert r[0] == l1 and r[2] == gcl and np.array_equal(r[1], g1) and np.array_equal(r[3], g2)
    # twice more, once on each of two side streams: bit-identical
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    keep = []
    res = [entry(g, tp, 3, tt, 3, n, e, stream=s, keep=keep) for s in (s1, s2, None)]
    torch.cuda.synchronize()
    for rc, out, a, b in res:
        assert rc == 0 and torch.equal(out, out0) and torch.equal(a, a0) and torch.equal(b, b0)


@gpu
@pytest.mark.parametrize("n", [1, 4])
def test_no_edges(n):
    """E = 0: the consistency loss is the stock formulation's mean over nothing, NaN; L1 and ``grad_l1`` are exact.
    What ``grad_gcl`` holds here is not pinned by the reference (its backward runs through 0 / 0) and nothing is
    asserted about it - nor, therefore, about ``pred.grad`` behind ``ops.contact_losses``, whose backward adds
    ``grad_gcl`` times the (zero) upstream gradient of the unused loss."""
    ei = np.zeros((2, 0), dtype=np.int64)
    pred, tgt = make_positions(n, 1.0, 3)
    clear_cache()
    g = graph_index(torch.from_numpy(ei).to(DEV), n)
    tp, tt = torch.from_numpy(pred).to(DEV), torch.from_numpy(tgt).to(DEV)
    l1, gcl = ops.contact_losses(g, tp, tt)
    rc, out, g1, _ = entry(g, tp, 3, tt, 3, n, 0)
    assert rc == 0 and float(out[0]) == float(l1) and np.isnan(float(out[1]))
    l1_64, g1_64, gc_64, _ = stock(pred, tgt, ei, torch.float64)
    l1_32, g1_32, _, _ = stock(pred, tgt, ei, torch.float32)
    assert np.isnan(gc_64) and np.isnan(float(gcl))
    assert abs(float(l1) - l1_64) <= 1e-6 * l1_64
    assert_parity(_np(g1), g1_32, g1_64, TOL, f"grad_l1 per node, E = 0, N={n}", metric=row_rel_err)
    assert np.array_equal(_np(g1), g1_32)                    # sign / (3 N): nothing to round differently


@gpu
def test_error_returns_launch_nothing():
    L = _lib.lib()
    n = 300
    ei = make_edges(n, 1)
    e = ei.shape[1]
    g = GraphIndex(torch.from_numpy(ei).to(DEV), n, validate=True)
    pred, tgt = make_positions(n, 0.1, 1)
    tp, tt = torch.from_numpy(pred).to(DEV), torch.from_numpy(tgt).to(DEV)
    torch.cuda.synchronize()
    cases = {"N = 0": dict(n=0), "ld_pred < 3": dict(ld_pred=2), "ld_target < 3": dict(ld_tgt=2),
             "workspace one byte short": dict(ws_short=1)}
    for what, kw in cases.items():
        _lib.kernel_trace(True)
        rc, out, a, b = entry(g, tp, kw.get("ld_pred", 3), tt, kw.get("ld_tgt", 3), kw.get("n", n), e,
                              ws_short=kw.get("ws_short", 0))
        counts = _lib.kernel_trace_counts()
        _lib.kernel_trace(False)
        torch.cuda.synchronize()
        assert rc != 0, what
        msg = L.dc_last_error()
        assert msg and b"dc_contact_loss" in msg, (what, msg)
        assert not counts, (what, counts)
        assert (out == 9.0).all() and (a == 9.0).all() and (b == 9.0).all(), what
    assert L.dc_contact_loss_workspace_bytes(-1) < 0
    rc, out, a, b = entry(g, tp, 3, tt, 3, n, e)             # and the same call, valid, still works
    assert rc == 0 and torch.isfinite(out).all()
