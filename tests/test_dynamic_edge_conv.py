"""GPU: ``DynamicEdgeConv`` - ``EdgeConv`` on the kNN graph of its own input, rebuilt in feature space at every call.

The edge set is never taken from this package's search: ``ref_edges`` comes from the numpy restatement of the kNN rule
in tests/nd_reference.py (``knn_graph(x, k, batch, loop=True)``: the point itself is among its neighbours).  On those
edges the layer must equal ``EdgeConv`` with ``torch.equal`` - output and every gradient - and, through
``helpers.assert_parity`` at the project's 1e-5, the float64 restatement ``aggr_j nn([x_i, x_j - x_i])`` of
tests/test_edge_conv.py (``RefEdgeConv``; its inputs are the exact grids of that file, so the maximum and the ReLU
select the same entries in float32, in float64 and on the device - and distances on a grid tie constantly)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import deformcontact_amd as dc
from deformcontact_amd.deferred import resolve
from deformcontact_amd.graph import clear_cache
from deformcontact_amd.nn import DynamicEdgeConv, EdgeConv
from tests import nd_reference as ref
from tests.helpers import assert_parity
from tests.test_edge_conv import RefEdgeConv, _device_nn, _ref_run, grid_values, grid_weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K, F, HIDDEN, C = 8, 5, 16, 6
RAGGED = [1, 5, 64, 13, 67]                   # two graphs smaller than K; a skipped id: one empty graph
N = sum(RAGGED)


def _dev(a):
    return torch.from_numpy(a).to(DEV)


def _inputs(batched):
    rng = np.random.default_rng(5)
    x = grid_values(rng, (N, F))
    b = ref.batch_of(RAGGED, skip=3) if batched else None
    inner = nn.Sequential(nn.Linear(2 * F, HIDDEN), nn.ReLU(), nn.Linear(HIDDEN, C))
    with torch.no_grad():
        for p in inner.parameters():
            p.copy_(torch.from_numpy(grid_weights(rng, tuple(p.shape))))
    gup = grid_values(rng, (N, C))
    ei = ref.edges_ref(*ref.knn_ref(x, x, K, b, b), 1)              # row 0 = the neighbour j, row 1 = the centre i
    return x, b, inner, gup, ei


def _run(conv, x, second, gup):
    for p in conv.parameters():
        p.grad = None
    xg = _dev(x).requires_grad_(True)
    out = conv(xg, second)
    assert type(out) is torch.Tensor
    torch.autograd.backward([out], [_dev(gup)])
    torch.cuda.synchronize()
    grads = {"x": xg.grad.clone()}
    grads.update({name: p.grad.clone() for name, p in conv.named_parameters()})
    return out.detach(), grads


@pytest.mark.parametrize("batched", [False, True], ids=["one_graph", "ragged"])
@pytest.mark.parametrize("aggr", ["max", "mean", "sum"])
def test_equals_edge_conv_on_reference_edges_and_float64(aggr, batched):
    x, b, inner, gup, ei = _inputs(batched)
    assert ei.shape[1] == (sum(min(K, n) * n for n in RAGGED) if batched else K * N)
    clear_cache()
    dev_nn = _device_nn(inner).to(DEV)
    dyn = DynamicEdgeConv(dev_nn, K, aggr=aggr)
    out, grads = _run(dyn, x, None if b is None else _dev(b), gup)
    # bit for bit EdgeConv on the reference's edges (the same module: the same parameters)
    out_e, grads_e = _run(EdgeConv(dev_nn, aggr=aggr), x, _dev(ei), gup)
    assert torch.equal(out, out_e)
    assert set(grads) == set(grads_e) == {"x", "nn.0.weight", "nn.0.bias", "nn.2.weight", "nn.2.bias"}
    for name in grads:
        assert torch.equal(grads[name], grads_e[name]), name
    # float64
    o32, g32 = _ref_run(RefEdgeConv(inner, aggr), x, ei, gup, torch.float32)
    inner64 = nn.Sequential(nn.Linear(2 * F, HIDDEN), nn.ReLU(), nn.Linear(HIDDEN, C)).double()
    inner64.load_state_dict(inner.state_dict())
    o64, g64 = _ref_run(RefEdgeConv(inner64, aggr), x, ei, gup, torch.float64)
    tag = f"dynamic_edge_conv[{aggr},{'ragged' if batched else 'one'}]"
    assert_parity(out.cpu().numpy(), o32, o64, tol=1e-5, name=f"{tag} out")
    for name in grads:
        assert_parity(grads[name].cpu().numpy(), g32[name], g64[name], tol=1e-5, name=f"{tag} d{name}")


def _grad_fn_names(t):
    seen, stack, names = set(), [t.grad_fn], []
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        stack.extend(f for f, _ in fn.next_functions)
    return names


def test_no_gradient_goes_through_the_search():
    x, b, inner, gup, ei = _inputs(True)
    lin = nn.Linear(2 * F, C).to(DEV)
    xg = _dev(x).requires_grad_(True)
    out = DynamicEdgeConv(lin, K)(xg, _dev(b))
    names = _grad_fn_names(out)
    # exactly the nodes of EdgeConv on a given graph: the pair rows, nn, the reduction - nothing from the search
    xs = _dev(x).requires_grad_(True)
    static = _grad_fn_names(EdgeConv(lin)(xs, _dev(ei)))
    assert sorted(names) == sorted(static), (names, static)
    assert names.count("_EdgePairFnBackward") == 1 and names.count("_EdgeReduceFnBackward") == 1
    assert names[0] == "_EdgeReduceFnBackward"
    # and an input that wants no gradient gives an output that wants none from x
    with torch.no_grad():
        assert not DynamicEdgeConv(lin, K)(_dev(x), _dev(b)).requires_grad


def test_two_layer_dgcnn():
    """3 -> 64 -> 64, k = 8, ReLU inside nn, three clouds, global max pool: the second layer searches 64 post-ReLU
    columns (the brute-force kernel, on tie-rich rows), the first 3 (the grid)."""
    torch.manual_seed(3)
    rng = np.random.default_rng(3)
    sizes = [40, 64, 70]
    pos = rng.standard_normal((sum(sizes), 3)).astype(np.float32)
    b = ref.batch_of(sizes)
    conv1 = DynamicEdgeConv(nn.Sequential(nn.Linear(6, 64), nn.ReLU()), 8).to(DEV)
    conv2 = DynamicEdgeConv(nn.Sequential(nn.Linear(128, 64), nn.ReLU()), 8).to(DEV)
    x, batch = _dev(pos).requires_grad_(True), _dev(b)
    h1 = conv1(x, batch)
    h2 = conv2(h1, batch)
    out = dc.nn.global_max_pool(h2, batch)
    assert tuple(h1.shape) == (174, 64) and tuple(out.shape) == (3, 64)
    # the second layer's edge set, recovered on the first layer's output, against numpy on that same output
    h1_host = h1.detach().cpu().numpy()
    assert (h1_host == 0).any() and (h1_host >= 0).all()             # post-ReLU maxima: zeros, hence ties
    ei2 = dc.nn.knn_graph(h1.detach(), 8, batch, loop=True)
    want = ref.edges_ref(*ref.knn_ref(h1_host, h1_host, 8, b, b), 1)
    assert torch.equal(ei2.cpu(), torch.from_numpy(want))
    assert torch.equal(h2, EdgeConv(conv2.nn)(h1, _dev(want)))
    (out * out).sum().backward()
    torch.cuda.synchronize()
    for name, p in list(conv1.named_parameters()) + list(conv2.named_parameters()) + [("pos", x)]:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name


def test_no_node_and_a_deferred_input():
    lin = nn.Linear(2 * F, C).to(DEV)
    conv = DynamicEdgeConv(lin, K)
    out = conv(torch.empty(0, F, device=DEV))
    assert tuple(out.shape) == (0, C) and out.dtype == torch.float32
    out = conv(torch.empty(0, F, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV))
    assert tuple(out.shape) == (0, C)
    # a deferred x (the plain call of a preceding TAGConv) is resolved
    x, b, inner, gup, ei = _inputs(True)
    tag = dc.nn.TAGConv(F, F, K=1).to(DEV)
    h = tag(_dev(x), _dev(ei))
    got = conv(h, _dev(b))
    h_plain = resolve(tag(_dev(x), _dev(ei))).detach()
    hb = h_plain.cpu().numpy()
    want_ei = ref.edges_ref(*ref.knn_ref(hb, hb, K, b, b), 1)
    assert torch.equal(got, EdgeConv(lin)(h_plain, _dev(want_ei)))
