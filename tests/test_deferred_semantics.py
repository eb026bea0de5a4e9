"""`deferred.DeferredActivation` (what a plain `conv(x, edge_index)` returns) against the eager tensor an undeferred conv
would have returned, op sequence by op sequence: values, `w.grad` and how often the layer ran.

The layer is a stub `run(relu)` computing `x @ w.T` (and the ReLU) in float64; the eager side runs the same sequence on
`x @ w.T` itself.  Every sequence ends with a plain use of `y` under grad mode, so a wrapper that forgot what was done to
`y` (an in-place ReLU that left it standing for the pre-activation, a ReLU that re-ran the layer over an in-place edit)
shows up in the values."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from deformcontact_amd.deferred import DeferredActivation, deferred

N, FI, FO = 6, 3, 4
_X = torch.tensor([[1.0, -2.0, 0.5], [0.25, 1.5, -1.0], [-0.75, 0.5, 2.0],
                   [2.0, 1.0, 1.0], [-1.0, -1.0, 0.25], [0.0, 3.0, -0.5]], dtype=torch.float64)
_W = torch.tensor([[0.5, -1.0, 0.25], [-0.5, 0.75, 1.0], [1.0, 0.5, -0.25], [0.25, 0.25, 0.5]], dtype=torch.float64)
_M = torch.linspace(-1.0, 1.0, FO * 5, dtype=torch.float64).reshape(5, FO)

INPLACE = {
    "Tensor.relu_": lambda y: y.relu_(),
    "torch.relu_": lambda y: torch.relu_(y),
    "F.relu_": lambda y: F.relu_(y),
    "F.relu(inplace=True)": lambda y: F.relu(y, inplace=True),
    "nn.ReLU(inplace=True)": lambda y: nn.ReLU(inplace=True)(y),
}
OUT_OF_PLACE = {
    "F.relu": lambda y: F.relu(y),
    "torch.relu": lambda y: torch.relu(y),
    "Tensor.relu": lambda y: y.relu(),
}
USES = {
    "y * 1": lambda y: y * 1,
    "y.sum()": lambda y: y.sum(),
    "passed on": lambda y: F.linear(y, _M),
    "repr": lambda y: repr(y),
}
PLAIN_FIRST = {
    "y.sum()": lambda y: y.sum(),
    "y.add_(c)": lambda y: y.add_(1.5),
    "y.mul_(c)": lambda y: y.mul_(-2.0),
    "y[0] = 0": lambda y: y.__setitem__(0, 0.0),
}


def _strip(r):
    """A result to compare: tensors as they are, ``repr`` strings without the autograd node's name."""
    return r.split(", grad_fn")[0].split(", requires_grad")[0] if isinstance(r, str) else r


def _run(seq, deferring, grad_call=True, grad_use=True):
    w = _W.clone().requires_grad_()
    calls = []

    def run(relu):
        calls.append(relu)
        z = _X @ w.t()
        return torch.relu(z) if relu else z
    with torch.set_grad_enabled(grad_call):
        if deferring:
            y = deferred(run, N, FO, _X, torch.is_grad_enabled() and w.requires_grad)
            assert isinstance(y, DeferredActivation) and calls == []
        else:
            y = _X @ w.t()
    with torch.set_grad_enabled(grad_use):
        res = [r for r in seq(y) if r is not None]          # (`y[0] = 0` returns nothing)
    res.append(y * 1)                                          # y itself, afterwards
    res = [_strip(r) for r in res]
    assert not any(isinstance(r, DeferredActivation) for r in res)
    grad = err = None
    wanted = [r for r in res if isinstance(r, torch.Tensor) and r.requires_grad]
    if wanted:
        loss = sum((r * torch.linspace(-1.0, 2.0, r.numel(), dtype=r.dtype).reshape(r.shape)).sum() for r in wanted)
        try:
            loss.backward()
            grad = w.grad
        except RuntimeError as e:                              # (eager refuses some sequences: so must the wrapper)
            err = "modified by an inplace operation" in str(e)
    return res, grad, err, calls


def _check(seq, want_calls, **kw):
    got, g_got, e_got, calls = _run(seq, True, **kw)
    want, g_want, e_want, _ = _run(seq, False, **kw)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        if isinstance(b, str):
            assert a == b, (i, a, b)
            continue
        assert type(a) is torch.Tensor, (i, type(a))
        assert a.requires_grad == b.requires_grad, (i, a.requires_grad, b.requires_grad)
        assert torch.equal(a.detach(), b.detach()), (i, a, b)
    assert e_got == e_want, (e_got, e_want)
    assert (g_got is None) == (g_want is None)
    if g_want is not None:
        if len(want_calls) == 1:
            assert torch.equal(g_got, g_want), (g_got, g_want)
        else:       # two runs of the layer: two matmul nodes add into w.grad where eager has one - another rounding order
            assert torch.allclose(g_got, g_want, rtol=1e-13, atol=0.0), (g_got, g_want)
    assert calls == want_calls, calls


@pytest.mark.parametrize("use", USES)
@pytest.mark.parametrize("form", INPLACE)
def test_inplace_relu_then_use_aliases_the_activated_result(form, use):
    """`y.relu_(); y * 1`: y stands for the activated tensor from then on; the layer runs once, fused."""
    _check(lambda y: (INPLACE[form](y), USES[use](y)), [True])


@pytest.mark.parametrize("form", INPLACE)
def test_inplace_relu_returns_the_plain_activated_tensor_that_y_then_is(form):
    w = _W.clone().requires_grad_()
    calls = []

    def run(relu):
        calls.append(relu)
        return torch.relu(_X @ w.t()) if relu else _X @ w.t()
    y = deferred(run, N, FO, _X, True)
    r = INPLACE[form](y)
    assert type(r) is torch.Tensor and y.value() is r and y.value(True) is r and calls == [True]


@pytest.mark.parametrize("act", ["F.relu", "Tensor.relu_", "F.relu(inplace=True)"])
@pytest.mark.parametrize("first", PLAIN_FIRST)
def test_plain_use_then_relu_is_the_real_op_on_the_pre_activation(first, act):
    """`y.add_(10); F.relu(y)`: the pre-activation already exists (and may be edited): the ReLU applies to it, the
    layer does not run a second time."""
    fn = {**OUT_OF_PLACE, **INPLACE}[act]
    _check(lambda y: (PLAIN_FIRST[first](y), fn(y)), [False])


@pytest.mark.parametrize("act", OUT_OF_PLACE)
def test_out_of_place_relu_then_plain_use_gets_the_pre_activation(act):
    """`r = F.relu(y); y * 1`: y is still the pre-activation, so the layer runs a second time, without the ReLU."""
    _check(lambda y: (OUT_OF_PLACE[act](y),), [True, False])


@pytest.mark.parametrize("form", INPLACE)
def test_out_of_place_relu_then_inplace_relu_leaves_the_first_result_alone(form):
    """`r = F.relu(y); y.relu_()`: y is activated in place from its pre-activation; r is a tensor of its own."""
    def seq(y):
        r = F.relu(y)
        keep = r.detach().clone()
        out = INPLACE[form](y)
        assert out.data_ptr() != r.data_ptr()
        return r, keep, out
    _check(seq, [True, False])


def test_relu_twice():
    _check(lambda y: (y.relu_(), y.relu_()), [True])              # eager backward refuses this (output of the first
    _check(lambda y: (F.relu(F.relu(y)),), [True, False])          # ReLU edited in place): the wrapper does too
    _check(lambda y: (F.relu(y), F.relu(y)), [True, False])
    _check(lambda y: (F.relu(y, inplace=True), F.relu(y)), [True])


@pytest.mark.parametrize("grad_call,grad_use", [(False, True), (True, False)])
@pytest.mark.parametrize("form", INPLACE)
def test_inplace_relu_across_grad_modes(form, grad_call, grad_use):
    """Called under `no_grad`, used with gradients: nothing is recorded, as for the eager call.  Called with gradients, the
    in-place ReLU under `no_grad`: recorded layer, unrecorded ReLU - the gradient has no mask, as in eager mode."""
    _check(lambda y: (INPLACE[form](y),), [True] if not grad_call else [False], grad_call=grad_call, grad_use=grad_use)


@pytest.mark.parametrize("grad_call,grad_use", [(False, True), (True, False)])
def test_plain_use_across_grad_modes(grad_call, grad_use):
    _check(lambda y: (y.sum(),), [False], grad_call=grad_call, grad_use=grad_use)
